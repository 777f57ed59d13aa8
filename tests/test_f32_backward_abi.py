"""CPU checks of the float32 preset's transformer backward entry points (csrc/f32path.hip): exported, in the ctypes table,
and argument validation that rejects null pointers, bad sizes and unsupported head dims before any launch."""
import pytest

NEW = ("wm_f32_layernorm_bwd_workspace_bytes", "wm_f32_layernorm_bwd", "wm_f32_bias_act_bwd", "wm_f32_attention_bwd",
       "wm_f32_loss_bwd")


@pytest.fixture(scope="module")
def lib():
    from ssl_wafermap_amd import _lib

    if not _lib.LIB_PATH.exists():
        from importlib import import_module

        import_module("ssl_wafermap_amd.build").build(verbose=False)
    return _lib.load()


def test_entry_points_are_exported_and_bound(lib):
    from ssl_wafermap_amd import _lib

    for name in NEW:
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name


def test_layernorm_backward_validation_needs_no_gpu(lib):
    assert lib.wm_f32_layernorm_bwd_workspace_bytes(0, 384) == 0
    assert lib.wm_f32_layernorm_bwd_workspace_bytes(1576, 0) == 0
    need = lib.wm_f32_layernorm_bwd_workspace_bytes(1576, 384)
    assert need >= 64 * 2 * 384 * 8 + 1576 * 2 * 4
    fake = 4096   # never dereferenced: every call below fails validation first
    assert lib.wm_f32_layernorm_bwd(None, fake, fake, 1e-6, 16, 384, fake, fake, fake, fake, need, None) == -1
    assert lib.wm_f32_layernorm_bwd(fake, fake, fake, 1e-6, 16, 384, None, fake, fake, fake, need, None) == -1
    assert lib.wm_f32_layernorm_bwd(fake, fake, fake, 1e-6, 0, 384, fake, fake, fake, fake, need, None) == -1
    assert lib.wm_f32_layernorm_bwd(fake, fake, fake, 1e-6, 16, 384, fake, fake, fake, None, need, None) == -1
    # too small a workspace
    assert lib.wm_f32_layernorm_bwd(fake, fake, fake, 1e-6, 1576, 384, fake, fake, fake, fake, 16, None) == -3


def test_bias_act_backward_validation_needs_no_gpu(lib):
    fake = 4096
    assert lib.wm_f32_bias_act_bwd(fake, None, None, 1, 16, 64, fake, None) == -1      # no dy
    assert lib.wm_f32_bias_act_bwd(fake, None, fake, 1, 16, 64, None, None) == -1      # no dx
    assert lib.wm_f32_bias_act_bwd(None, None, fake, 1, 16, 64, fake, None) == -1      # GELU needs the pre-activation
    assert lib.wm_f32_bias_act_bwd(fake, None, fake, 3, 16, 64, fake, None) == -1      # unknown activation
    assert lib.wm_f32_bias_act_bwd(fake, None, fake, 1, 0, 64, fake, None) == -1


def test_attention_backward_validation_needs_no_gpu(lib):
    fake = 4096
    assert lib.wm_f32_attention_bwd(None, fake, fake, 2, 50, 16, 32, 0.17, fake, None) == -1
    assert lib.wm_f32_attention_bwd(fake, fake, None, 2, 50, 16, 32, 0.17, fake, None) == -1
    assert lib.wm_f32_attention_bwd(fake, fake, fake, 2, 50, 16, 32, 0.17, None, None) == -1
    assert lib.wm_f32_attention_bwd(fake, fake, fake, 0, 50, 16, 32, 0.17, fake, None) == -1
    # head dims other than 64 / 32, and sequences whose operands do not fit the LDS, are unsupported
    for hd in (16, 48, 128):
        assert lib.wm_f32_attention_bwd(fake, fake, fake, 2, 50, 4, hd, 0.1, fake, None) == -2
    assert lib.wm_f32_attention_bwd(fake, fake, fake, 2, 400, 6, 64, 0.125, fake, None) == -2


def test_loss_backward_validation_needs_no_gpu(lib):
    fake = 4096
    assert lib.wm_f32_loss_bwd(None, fake, 96, 1, 1 / 96, None, fake, None) == -1
    assert lib.wm_f32_loss_bwd(fake, None, 96, 1, 1 / 96, None, fake, None) == -1
    assert lib.wm_f32_loss_bwd(fake, fake, 96, 1, 1 / 96, None, None, None) == -1
    assert lib.wm_f32_loss_bwd(fake, fake, 0, 1, 1.0, None, fake, None) == -1
    for mode in (0, 3):   # 0 (plain sum) has no elementwise gradient here; 3 is unknown
        assert lib.wm_f32_loss_bwd(fake, fake, 96, mode, 1 / 96, None, fake, None) == -1
