"""CPU checks of the model-inspection layer (csrc/interpret.hip, interpret.py): the C entry points reject bad shapes
and limits before any launch, the Python layer raises ValueError for bad shapes and WaferHipError for host tensors,
the ViT exposes dino's inspection methods, and the figure script selects wafers by failure type.  No GPU needed."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
EINVAL, EUNSUPPORTED, EALIGN = -1, -2, -4
FAKE = 1 << 20   # a non-null, 16-byte aligned address: never dereferenced, every call below fails validation first


@pytest.fixture(scope="module")
def lib():
    from ssl_wafermap_amd import _lib

    if not _lib.LIB_PATH.exists():
        from importlib import import_module

        import_module("ssl_wafermap_amd.build").build(verbose=False)
    return _lib.load()


def test_attention_probs_entry_rejects_bad_arguments(lib):
    f = lib.wm_attention_probs
    assert f(FAKE, 1, 2, 257, 6, 64, 0.125, 0, FAKE, None) == EUNSUPPORTED   # S > 256
    assert f(FAKE, 1, 2, 197, 6, 48, 0.125, 0, FAKE, None) == EUNSUPPORTED   # head_dim
    assert f(FAKE, 2, 2, 197, 6, 64, 0.125, 0, FAKE, None) == EUNSUPPORTED   # dtype
    assert f(FAKE, 1, 0, 197, 6, 64, 0.125, 0, FAKE, None) == EINVAL
    assert f(FAKE, 1, 2, 0, 6, 64, 0.125, 1, FAKE, None) == EINVAL
    assert f(None, 1, 2, 197, 6, 64, 0.125, 0, FAKE, None) == EINVAL
    assert f(FAKE, 0, 2, 197, 6, 64, 0.125, 0, None, None) == EINVAL
    assert f(FAKE + 4, 0, 2, 197, 6, 64, 0.125, 0, FAKE, None) == EALIGN


def test_mass_mask_entry_rejects_bad_arguments(lib):
    f = lib.wm_attention_mass_mask
    assert f(FAKE, 4, 257, 257, 0.6, FAKE, None) == EUNSUPPORTED   # more than 256 entries
    assert f(FAKE, 4, 196, 195, 0.6, FAKE, None) == EINVAL         # pitch below the row length
    assert f(FAKE, 4, 196, 197, 1.5, FAKE, None) == EINVAL
    assert f(FAKE, 4, 196, 197, -0.1, FAKE, None) == EINVAL
    assert f(FAKE, 4, 196, 197, float("nan"), FAKE, None) == EINVAL
    assert f(FAKE, 0, 196, 197, 0.6, FAKE, None) == EINVAL
    assert f(None, 4, 196, 197, 0.6, FAKE, None) == EINVAL


def test_eigencam_entry_rejects_bad_arguments(lib):
    f = lib.wm_eigencam
    assert f(FAKE, 1, 2, 512, 9, 9, 224, 224, FAKE, None) == EUNSUPPORTED   # 81 positions
    assert f(FAKE, 1, 2, 512, 8, 8, 5000, 224, FAKE, None) == EUNSUPPORTED  # output too large
    assert f(FAKE, 3, 2, 512, 7, 7, 224, 224, FAKE, None) == EUNSUPPORTED   # dtype
    assert f(FAKE, 1, 0, 512, 7, 7, 224, 224, FAKE, None) == EINVAL
    assert f(FAKE, 1, 2, 512, 7, 7, 0, 224, FAKE, None) == EINVAL
    assert f(None, 1, 2, 512, 7, 7, 224, 224, FAKE, None) == EINVAL
    assert f(FAKE, 1, 2, 512, 7, 7, 224, 224, None, None) == EINVAL


def test_python_layer_validates_shapes_then_device():
    from ssl_wafermap_amd import _lib
    from ssl_wafermap_amd.interpret import attention_mass_mask, attention_probs, eigencam_maps

    with pytest.raises(ValueError):
        attention_probs(torch.zeros(2 * 257, 3 * 6 * 64), 2, 257, 6, 0.125)     # S > 256
    with pytest.raises(ValueError):
        attention_probs(torch.zeros(2 * 197, 3 * 6 * 48), 2, 197, 6, 0.125)     # head_dim 48
    with pytest.raises(ValueError):
        attention_probs(torch.zeros(2 * 196, 3 * 6 * 64), 2, 197, 6, 0.125)     # rows != B * S
    with pytest.raises(_lib.WaferHipError):
        attention_probs(torch.zeros(2 * 197, 3 * 6 * 64, dtype=torch.bfloat16), 2, 197, 6, 0.125)
    with pytest.raises(ValueError):
        attention_mass_mask(torch.zeros(4, 258), 0.6)
    with pytest.raises(ValueError):
        attention_mass_mask(torch.zeros(4, 197), 1.2)
    with pytest.raises(_lib.WaferHipError):
        attention_mass_mask(torch.zeros(4, 197), 0.6)
    with pytest.raises(ValueError):
        eigencam_maps(torch.zeros(2, 512, 9, 9))                                 # HW > 64
    with pytest.raises(ValueError):
        eigencam_maps(torch.zeros(2, 512, 7))
    with pytest.raises(_lib.WaferHipError):
        eigencam_maps(torch.zeros(2, 512, 7, 7))


def test_model_level_functions_validate_images():
    from ssl_wafermap_amd import _lib
    from ssl_wafermap_amd.interpret import attention_maps, eigencam
    from ssl_wafermap_amd.models import ResNet18, vit_tiny

    vit, net = vit_tiny(), ResNet18()
    with pytest.raises(ValueError):
        attention_maps(vit, torch.zeros(1, 3, 224, 208))   # not square
    with pytest.raises(ValueError):
        attention_maps(vit, torch.zeros(1, 3, 200, 200))   # not a multiple of the patch size
    with pytest.raises(ValueError):
        attention_maps(vit, torch.zeros(1, 3, 256, 256))   # 257 tokens
    with pytest.raises(_lib.WaferHipError):
        attention_maps(vit, torch.zeros(1, 3, 224, 224))
    with pytest.raises(ValueError):
        eigencam(net, torch.zeros(1, 3, 224, 200))
    with pytest.raises(ValueError):
        eigencam(net, torch.zeros(1, 3, 288, 288))          # 9 x 9 layer4 map
    with pytest.raises(_lib.WaferHipError):
        eigencam(net, torch.zeros(1, 3, 256, 256))


def test_vit_has_dino_inspection_methods():
    from ssl_wafermap_amd.models import VisionTransformer

    assert callable(VisionTransformer.get_last_selfattention)
    assert callable(VisionTransformer.get_intermediate_layers)


def test_script_selects_wafers_by_failure_type():
    spec = importlib.util.spec_from_file_location("attention_figures_amd", ROOT / "scripts/attention_figures_amd.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    store, labels = mod.load_wafers(mod.FIXTURE)
    assert len(store) == len(labels) == 623
    idx = mod.select(labels, ["Scratch", "Edge-Loc"], 2)
    assert list(labels[idx]) == [7, 7, 2, 2]
    assert list(idx) == sorted(idx[:2]) + sorted(idx[2:])
    with pytest.raises(ValueError):
        mod.select(labels, ["Ring"], 1)
    with pytest.raises(ValueError):
        mod.select(np.full(5, 8), ["Scratch"], 1)
