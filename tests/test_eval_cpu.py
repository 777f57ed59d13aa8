"""CPU checks of the MixedWM38 evaluation pieces: the early-stopping rule, pos_weight, the driver's subset split,
Lightning-layout checkpoints, and the argument validation of the evaluation entry points (csrc/evalops.hip, WM_ACT_MISH)
before any launch."""
import importlib.util
import math
import pickle
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent


def _driver():
    spec = importlib.util.spec_from_file_location("mixedwm38_evals_amd", ROOT / "scripts" / "mixedwm38_evals_amd.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _run(stopper, values):
    """Epochs run until the rule stops (or all values)."""
    for i, v in enumerate(values):
        if stopper.step(v):
            return i + 1
    return len(values)


# ------------------------------------------------------------------------------------ early stopping
def test_early_stopping_stops_after_patience_epochs_of_plateau():
    from ssl_wafermap_amd.models import EarlyStopping

    es = EarlyStopping(patience=3)
    assert _run(es, [1.0, 0.9, 0.8, 0.8, 0.8, 0.8, 0.1]) == 6   # best 0.8 at epoch 3, three non-improvements
    assert es.stopped and es.best == 0.8 and es.wait == 3


def test_early_stopping_ties_are_not_improvements():
    from ssl_wafermap_amd.models import EarlyStopping

    es = EarlyStopping(patience=2)
    assert _run(es, [0.5, 0.5, 0.5, 0.4]) == 3
    es = EarlyStopping(patience=2)
    assert _run(es, [0.5, 0.5, 0.49999, 0.5, 0.49998, 0.6, 0.6]) == 7   # each strict improvement resets the count
    assert es.best == 0.49998


def test_early_stopping_patience_boundary():
    from ssl_wafermap_amd.models import EarlyStopping

    # wait reaches patience exactly at the last value: stops there, not one later
    es = EarlyStopping(patience=4)
    assert _run(es, [1.0, 2.0, 2.0, 2.0, 2.0, 0.0]) == 5
    es = EarlyStopping(patience=4)
    assert _run(es, [1.0, 2.0, 2.0, 2.0, 0.5, 2.0]) == 6 and not es.stopped
    # patience 0: the first non-improvement stops; the first value always improves on +inf
    es = EarlyStopping(patience=0)
    assert _run(es, [3.0, 2.0, 2.5]) == 3


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
def test_early_stopping_stops_on_non_finite(bad):
    from ssl_wafermap_amd.models import EarlyStopping

    es = EarlyStopping(patience=50)
    assert _run(es, [1.0, 0.5, bad, 0.1]) == 3
    assert es.best == 0.5


# ------------------------------------------------------------------------------------ pos_weight
def test_pos_weight_is_negative_over_positive_frequency():
    from ssl_wafermap_amd.models import pos_weight_from_labels

    y = np.array([[1, 0, 1], [0, 1, 1], [0, 0, 1], [1, 0, 0]])
    pw = pos_weight_from_labels(y)
    assert pw.dtype == torch.float32
    assert torch.allclose(pw, torch.tensor([1.0, 3.0, 1 / 3]))
    assert torch.equal(pos_weight_from_labels(torch.as_tensor(y)), pw)


def test_pos_weight_rejects_a_label_without_positives():
    from ssl_wafermap_amd.models import pos_weight_from_labels

    y = np.array([[1, 0, 1], [0, 0, 1]])
    with pytest.raises(ValueError, match=r"label\(s\) \[1\]"):
        pos_weight_from_labels(y)


# ------------------------------------------------------------------------------------ subset split
def test_subset_split_properties():
    drv = _driver()
    with np.load(drv.FIXTURE) as z:
        labels = z["multilabel"].astype(np.int64)
    tr, va, te = drv.subset_split(labels)
    n = labels.shape[0]
    assert n == 381 and labels.shape[1] == 8
    assert len(set(tr) | set(va) | set(te)) == n == len(tr) + len(va) + len(te)     # disjoint, covering
    assert labels[tr].sum(0).min() >= 1                                              # every label has a train positive
    assert abs(len(tr) - 0.6 * n) <= 8 and len(va) >= 60 and len(te) >= 60
    again = drv.subset_split(labels)
    assert all(np.array_equal(a, b) for a, b in zip((tr, va, te), again))            # deterministic
    # label 5 has two positives in the fixture: val or test lacks it, the case the single-class AUROC rule covers
    assert labels[:, 5].sum() == 2
    assert labels[va, 5].sum() == 0 or labels[te, 5].sum() == 0


# ------------------------------------------------------------------------------------ checkpoints
def test_checkpoint_round_trip(tmp_path):
    from ssl_wafermap_amd.models import TwoLayerMultilabelClassifier
    from ssl_wafermap_amd.utils.checkpoint import load_checkpoint, save_checkpoint

    torch.manual_seed(0)
    a = TwoLayerMultilabelClassifier(32, 8, pos_weight=torch.arange(1, 9, dtype=torch.float32))
    assert list(a.model.state_dict()) == ["0.weight", "0.bias", "3.weight", "3.bias"]   # the reference's keys
    p = save_checkpoint(a, tmp_path / "m" / "checkpoints" / "last.ckpt", epoch=4, global_step=123)
    raw = torch.load(p, weights_only=True)
    assert set(raw) == {"state_dict", "epoch", "global_step"} and raw["epoch"] == 4 and raw["global_step"] == 123
    assert all(v.device.type == "cpu" for v in raw["state_dict"].values())
    torch.manual_seed(1)
    b = TwoLayerMultilabelClassifier(32, 8, pos_weight=torch.ones(8))
    assert not torch.equal(a.model[0].weight, b.model[0].weight)
    ck = load_checkpoint(b, p)
    assert ck["global_step"] == 123
    for k, v in a.state_dict().items():
        assert torch.equal(v, b.state_dict()[k]), k


def test_checkpoint_with_lightning_keys_and_unknown_class(tmp_path):
    from ssl_wafermap_amd.utils.checkpoint import load_checkpoint

    m = torch.nn.Linear(4, 3)
    lightning = {"epoch": 149, "global_step": 62250, "pytorch-lightning_version": "2.0.0",
                 "state_dict": {k: v.clone() + 1 for k, v in m.state_dict().items()},
                 "loops": {"fit_loop": {"epoch_progress": {"current": 150}}}, "callbacks": {"EarlyStopping": {"wait": 3}},
                 "optimizer_states": [{"state": {}, "param_groups": [{"lr": 0.001}]}], "lr_schedulers": [],
                 "hparams_name": "kwargs", "hyper_parameters": {"batch_size": 64, "max_epochs": 150}}
    torch.save(lightning, tmp_path / "l.ckpt")
    ck = load_checkpoint(m, tmp_path / "l.ckpt")
    assert ck["epoch"] == 149 and torch.equal(m.state_dict()["bias"], lightning["state_dict"]["bias"])
    torch.save({"state_dict": {}, "hyper_parameters": {"loss": torch.nn.MSELoss()}}, tmp_path / "bad.ckpt")
    with pytest.raises(pickle.UnpicklingError, match="MSELoss"):
        load_checkpoint(m, tmp_path / "bad.ckpt")
    torch.save({"model": m.state_dict()}, tmp_path / "nolayout.ckpt")
    with pytest.raises(KeyError, match="state_dict"):
        load_checkpoint(m, tmp_path / "nolayout.ckpt")


# ------------------------------------------------------------------------------------ C entry validation
@pytest.fixture(scope="module")
def lib():
    from ssl_wafermap_amd import _lib

    if not _lib.LIB_PATH.exists():
        from importlib import import_module

        import_module("ssl_wafermap_amd.build").build(verbose=False)
    return _lib.load()


def test_eval_entry_points_are_exported_and_bound(lib):
    from ssl_wafermap_amd import _lib

    for name in ("wm_multilabel_auroc_workspace_bytes", "wm_multilabel_auroc", "wm_dropout_fwd", "wm_dropout_bwd"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.wm_version() == 4


def test_auroc_validation_needs_no_gpu(lib):
    assert lib.wm_multilabel_auroc_workspace_bytes(0, 8) == 0
    assert lib.wm_multilabel_auroc_workspace_bytes(100, 0) == 0
    assert lib.wm_multilabel_auroc_workspace_bytes(100, 2000) == 0            # more labels than supported
    assert lib.wm_multilabel_auroc_workspace_bytes(1 << 29, 8) == 0           # rows * L beyond 2^31
    need = lib.wm_multilabel_auroc_workspace_bytes(26609, 8)
    assert need >= 26609 * 8 * 4
    fake = 4096   # never dereferenced: every call below fails validation first
    assert lib.wm_multilabel_auroc(None, 0, fake, 97, 8, fake, None, fake, need, None) == -1
    assert lib.wm_multilabel_auroc(fake, 0, None, 97, 8, fake, None, fake, need, None) == -1
    assert lib.wm_multilabel_auroc(fake, 0, fake, 97, 8, None, None, fake, need, None) == -1
    assert lib.wm_multilabel_auroc(fake, 0, fake, 97, 8, fake, None, None, need, None) == -1
    assert lib.wm_multilabel_auroc(fake, 0, fake, 0, 8, fake, None, fake, need, None) == -1
    assert lib.wm_multilabel_auroc(fake, 0, fake, 97, 0, fake, None, fake, need, None) == -1
    assert lib.wm_multilabel_auroc(fake, 7, fake, 97, 8, fake, None, fake, need, None) == -2   # unknown dtype
    assert lib.wm_multilabel_auroc(fake, 1, fake, 26609, 8, fake, None, fake, 64, None) == -3  # workspace too small
    assert lib.wm_multilabel_auroc(fake + 4, 1, fake, 97, 8, fake, None, fake + 4, need, None) == -4   # misaligned ws


def test_dropout_validation_needs_no_gpu(lib):
    fake = 4096
    for fn in (lib.wm_dropout_fwd, lib.wm_dropout_bwd):
        assert fn(None, 1, 64, 0.5, 7, fake, None) == -1
        assert fn(fake, 1, 64, 0.5, 7, None, None) == -1
        assert fn(fake, 1, 0, 0.5, 7, fake, None) == -1
        assert fn(fake, 1, (1 << 32) + 1, 0.5, 7, fake, None) == -1   # the element counter is 32-bit
        for p in (-0.1, 1.5, math.nan):
            assert fn(fake, 1, 64, p, 7, fake, None) == -1
        assert fn(fake, 5, 64, 0.5, 7, fake, None) == -2


def test_mish_code_is_validated_and_float32_preset_rejects_it(lib):
    fake = 4096
    assert lib.wm_bias_act_fwd(fake, None, None, 4, 16, 64, fake, None) == -2          # unknown activation
    assert lib.wm_bias_act_fwd(fake, None, None, 3, 16, 60, fake, None) == -1          # C % 8
    assert lib.wm_bias_act_bwd(fake, None, fake, 4, 16, 64, fake, None, None) == -2
    assert lib.wm_bias_act_bwd(None, None, fake, 3, 16, 64, fake, None, None) == -1    # Mish needs the pre-activation
    assert lib.wm_bias_act_bwd_parts(fake, None, fake, 3, 16, 64, None, fake, None) == -1
    assert lib.wm_f32_bias_act_bwd(fake, None, fake, 3, 16, 64, fake, None) == -1      # not in the float32 preset

    from ssl_wafermap_amd import nn as hnn
    from ssl_wafermap_amd.precision import precision

    with precision("float32"):
        with pytest.raises(NotImplementedError):
            hnn.Mish()(torch.zeros(4, 8))


def test_dropout_module_is_identity_without_a_launch():
    from ssl_wafermap_amd import nn as hnn

    x = torch.randn(4, 8)           # a CPU tensor: any launch would raise
    d = hnn.Dropout(0.5).eval()
    assert d(x) is x
    assert hnn.Dropout(0.0).train()(x) is x
    with pytest.raises(ValueError):
        hnn.Dropout(1.5)
