"""CPU checks of the BatchNorm entry points (csrc/bn.hip): the workspace size and, for each of the twelve entry points,
which argument error is reported and which one wins when several apply.

No call here may pass validation: the pointers are fake, so a call that did would launch a kernel on a bad address.
`call` therefore asserts a negative code on everything it sends (a launch error would be a positive hipError_t)."""
import pytest

EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -3
FAKE = 4096        # never dereferenced: every call fails validation first
AMPLE = 1 << 30    # workspace_bytes that no case below finds too small

# argument names in ABI order (include/wafer_hip.h)
ARGS = {
    "wm_bn_train_fwd": "y residual gamma beta running_mean running_var nbt rows C G eps momentum relu save_mean "
                       "save_invstd out relu_mask workspace workspace_bytes stream",
    "wm_bn_train_fwd_from_stats": "y residual gamma beta running_mean running_var nbt rows C G eps momentum relu save_mean "
                                  "save_invstd out relu_mask stat_part stat_tiles workspace workspace_bytes stream",
    "wm_bn_train_stats": "y gamma beta running_mean running_var nbt rows C G eps momentum save_mean save_invstd scale shift "
                         "stat_part stat_tiles workspace workspace_bytes stream",
    "wm_bn_eval_scale_shift": "gamma beta running_mean running_var C eps scale shift stream",
    "wm_bn_eval_fwd": "y residual gamma beta running_mean running_var rows C eps relu out workspace workspace_bytes stream",
    "wm_bn_train_bwd": "y dout out_relu relu_from_y gamma beta save_mean save_invstd rows C G dgamma dbeta accumulate dy dz "
                       "workspace workspace_bytes stream",
    "wm_bn_train_bwd_from_stats": "y g gamma beta save_mean save_invstd rows C G dgamma dbeta accumulate dy stat_part "
                                  "stat_tiles workspace workspace_bytes stream",
    "wm_bn_relu_maxpool_bwd": "y ysel pooled_dy pool_idx N H W C gamma beta save_mean save_invstd G dgamma dbeta accumulate "
                              "dy workspace workspace_bytes stream",
    "wm_bn_sync_fwd_sums": "y rows C G stat_part stat_tiles sums workspace workspace_bytes stream",
    "wm_bn_sync_fwd_apply": "y residual gamma beta running_mean running_var nbt rows C G group_count eps momentum relu "
                            "save_mean save_invstd out sums workspace workspace_bytes stream",
    "wm_bn_sync_bwd_sums": "y dout out_relu relu_from_y gamma beta save_mean save_invstd rows C G dgamma dbeta accumulate "
                           "sums workspace workspace_bytes stream",
    "wm_bn_sync_bwd_apply": "y dout out_relu relu_from_y gamma beta save_mean save_invstd rows C G group_count sums dy dz "
                            "workspace workspace_bytes stream",
}
# the pointers each entry point refuses to take as NULL
REQUIRED = {
    "wm_bn_train_fwd": "y out save_mean save_invstd workspace",
    "wm_bn_train_fwd_from_stats": "y out save_mean save_invstd workspace stat_part",
    "wm_bn_train_stats": "y save_mean save_invstd scale shift workspace",
    "wm_bn_eval_scale_shift": "running_mean running_var scale shift",
    "wm_bn_eval_fwd": "y out running_mean running_var workspace",
    "wm_bn_train_bwd": "y dout save_mean save_invstd dy workspace",
    "wm_bn_train_bwd_from_stats": "y g save_mean save_invstd dy stat_part workspace",
    "wm_bn_relu_maxpool_bwd": "pooled_dy pool_idx gamma beta y save_mean save_invstd dy workspace",
    "wm_bn_sync_fwd_sums": "y sums workspace",
    "wm_bn_sync_fwd_apply": "y out save_mean save_invstd sums workspace",
    "wm_bn_sync_bwd_sums": "y dout save_mean save_invstd sums workspace",
    "wm_bn_sync_bwd_apply": "y dout save_mean save_invstd sums dy workspace",
}
# Base case: [1024][64] in two statistics groups (the stem's [2*8*8][64] for the pooled backward).  Optional pointers are
# NULL, statistics slots are given only where the entry point requires them.
SCALARS = dict(rows=1024, C=64, G=2, N=2, H=8, W=8, eps=1e-5, momentum=0.1, relu=1, relu_from_y=0, accumulate=0,
               stat_tiles=4, group_count=512, workspace_bytes=AMPLE)
OPTIONAL = ("residual", "relu_mask", "out_relu", "dz", "stream")
SLOTS_OPTIONAL = ("wm_bn_train_stats", "wm_bn_sync_fwd_sums")


def full_bytes(rows, C, G):
    """wm_bn_workspace_bytes: G*nblk*2*C floats of partial sums + 7*G*C of coefficients + 256 bytes, nblk from reduce_blocks
    (rows per pass = max(256 / (C/8), 1); 16 passes per block; clamped to [1, 256] blocks per group)."""
    rpp = max(256 // (C // 8), 1)
    nblk = min(max(-(-(rows // G) // (rpp * 16)), 1), 256)
    return (G * nblk * 2 * C + 7 * G * C) * 4 + 256


def scratch_bytes(tiles, C, G):
    """Pre-reduction scratch of the convolution's statistics slots: none up to 512 slots per group, else 128 per group."""
    return G * 128 * 2 * C * 4 if tiles > 512 else 0


@pytest.fixture(scope="module")
def lib():
    from ssl_wafermap_amd import _lib

    if not _lib.LIB_PATH.exists():
        from importlib import import_module

        import_module("ssl_wafermap_amd.build").build(verbose=False)
    return _lib.load()


def call(lib, name, **over):
    names = ARGS[name].split()
    unknown = set(over) - set(names)
    assert not unknown, f"{name} has no argument {unknown}"
    args = []
    for n in names:
        if n in over:
            args.append(over[n])
        elif n in SCALARS:
            args.append(SCALARS[n])
        elif n in OPTIONAL or (n == "stat_part" and name in SLOTS_OPTIONAL):
            args.append(None)
        else:
            args.append(FAKE)
    rc = getattr(lib, name)(*args)
    assert rc < 0, f"{name}({over}) passed validation (returned {rc}): it would launch on fake pointers"
    return rc


def shape(name, rows=None, C=None, G=None):
    """Shape overrides in the entry point's own terms: wm_bn_relu_maxpool_bwd takes rows as N * H * W (rows = (N, H, W)
    there), wm_bn_eval_fwd has one statistics group."""
    o = {}
    if rows is not None:
        o.update(dict(zip("NHW", rows)) if name == "wm_bn_relu_maxpool_bwd" else {"rows": rows[0] * rows[1] * rows[2]})
    if C is not None:
        o["C"] = C
    if G is not None and name != "wm_bn_eval_fwd":
        o["G"] = G
    return o


SHAPED = [n for n in ARGS if n != "wm_bn_eval_scale_shift"]     # everything with a [rows][C] tensor
WIDE = dict(rows=512, C=4096)                                   # a projection head: one thread per channel
WIDE_POOLED = dict(N=2, H=16, W=16, C=4096)


def test_entry_points_are_exported_and_bound(lib):
    from ssl_wafermap_amd import _lib

    for name in ("wm_bn_workspace_bytes", *ARGS):
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    assert len(ARGS) == 12 and set(ARGS) == set(REQUIRED)


def test_workspace_bytes(lib):
    for rows, C, G in ((0, 64, 2), (-8, 64, 2), (1024, 0, 2), (1024, -64, 2), (1024, 64, 0), (1024, 64, -1), (1024, 60, 2),
                       (1024, 4, 2)):
        assert lib.wm_bn_workspace_bytes(rows, C, G) == 0, (rows, C, G)
    # (G*nblk*2*C + 7*G*C) * 4 + 256 with nblk = clamp(ceil(rows/G / (16 * max(256 / (C/8), 1))), 1, 256), by hand for the
    # BatchNorm shapes of the ResNet-18 SimCLR step at batch 256 per view (G = 2 views) and its head:
    #   stem/layer1  rows/G = 802816, C =   64: 32 rows per pass, ceil(802816/512) = 1568 -> 256 blocks
    #                (2*256*2*64   + 14*64)   * 4 + 256 = ( 65536 +   896) * 4 + 256 =  265984
    #   layer2       rows/G = 200704, C =  128: 16 rows per pass, ceil(200704/256) =  784 -> 256 blocks
    #                (2*256*2*128  + 14*128)  * 4 + 256 = (131072 +  1792) * 4 + 256 =  531712
    #   layer3       rows/G =  50176, C =  256:  8 rows per pass, ceil(50176/128)  =  392 -> 256 blocks
    #                (2*256*2*256  + 14*256)  * 4 + 256 = (262144 +  3584) * 4 + 256 = 1063168
    #   layer4       rows/G =  12544, C =  512:  4 rows per pass, ceil(12544/64)   =  196 blocks
    #                (2*196*2*512  + 14*512)  * 4 + 256 = (401408 +  7168) * 4 + 256 = 1634560
    #   head 2048    rows/G =    256, C = 2048:  1 row per pass,  ceil(256/16)     =   16 blocks
    #                (2*16*2*2048  + 14*2048) * 4 + 256 = (131072 + 28672) * 4 + 256 =  639232
    #   head 4096    rows/G =    256, C = 4096:  256 / 512 = 0 -> 1 row per pass, 16 blocks
    #                (2*16*2*4096  + 14*4096) * 4 + 256 = (262144 + 57344) * 4 + 256 = 1278208
    #   one group    rows/G =     16, C =   64: 32 rows per pass, 1 block
    #                (1*1*2*64     + 7*64)    * 4 + 256 = (   128 +   448) * 4 + 256 =    2560
    for (rows, C, G), want in {(2 * 256 * 56 * 56, 64, 2): 265984, (2 * 256 * 28 * 28, 128, 2): 531712,
                               (2 * 256 * 14 * 14, 256, 2): 1063168, (2 * 256 * 7 * 7, 512, 2): 1634560,
                               (512, 2048, 2): 639232, (512, 4096, 2): 1278208, (16, 64, 1): 2560}.items():
        assert lib.wm_bn_workspace_bytes(rows, C, G) == want, (rows, C, G)
        assert full_bytes(rows, C, G) == want, (rows, C, G)   # (the restatement the cases below size workspaces with)


@pytest.mark.parametrize("name", list(ARGS))
def test_null_required_pointer_is_einval_and_comes_first(lib, name):
    for p in REQUIRED[name].split():
        assert call(lib, name, **{p: None}) == EINVAL, p
        # ... ahead of the shape and workspace checks
        bad = {"C": 60} if name == "wm_bn_eval_scale_shift" else {"C": 60, "workspace_bytes": 0}
        assert call(lib, name, **{p: None}, **bad) == EINVAL, p


@pytest.mark.parametrize("name", SHAPED)
def test_non_positive_sizes_are_einval(lib, name):
    assert call(lib, name, C=0) == EINVAL
    assert call(lib, name, C=-64) == EINVAL
    if name == "wm_bn_relu_maxpool_bwd":
        for o in (dict(N=0), dict(H=1), dict(W=1), dict(H=0), dict(N=4, H=32768, W=16384)):   # (the last: 2^31 rows)
            assert call(lib, name, **o) == EINVAL, o
    else:
        assert call(lib, name, rows=0) == EINVAL
        assert call(lib, name, rows=-1024) == EINVAL
    if name != "wm_bn_eval_fwd":
        assert call(lib, name, G=0) == EINVAL
        assert call(lib, name, G=-2) == EINVAL


def test_eval_scale_shift_validation(lib):
    assert call(lib, "wm_bn_eval_scale_shift", C=0) == EINVAL
    assert call(lib, "wm_bn_eval_scale_shift", C=-8) == EINVAL


@pytest.mark.parametrize("name", SHAPED)
def test_unsupported_shapes_come_before_the_workspace_check(lib, name):
    for ws in (AMPLE, 0):
        assert call(lib, name, C=60, workspace_bytes=ws) == EUNSUPPORTED                       # C % 8
        assert call(lib, name, **shape(name, C=16392), workspace_bytes=ws) == EUNSUPPORTED     # wider than any path
        # C > 2048 is served only up to 65536 rows per group
        assert call(lib, name, **shape(name, rows=(2, 257, 256), C=4096, G=2), workspace_bytes=ws) == EUNSUPPORTED
        assert call(lib, name, **shape(name, rows=(1, 257, 256), C=4096, G=1), workspace_bytes=ws) == EUNSUPPORTED
        if name != "wm_bn_eval_fwd":                                                           # rows % G
            assert call(lib, name, **shape(name, rows=(3, 11, 31), G=2), workspace_bytes=ws) == EUNSUPPORTED
            assert call(lib, name, **shape(name, rows=(2, 8, 8), G=3), workspace_bytes=ws) == EUNSUPPORTED


def test_workspace_one_byte_short_is_eworkspace(lib):
    full, wide = full_bytes(1024, 64, 2), full_bytes(512, 4096, 2)
    G, C = 2, 64
    minimum = {   # the base case's smallest accepted workspace_bytes, per entry point
        "wm_bn_train_fwd": full, "wm_bn_train_fwd_from_stats": 2 * G * C * 4, "wm_bn_train_stats": full,
        "wm_bn_eval_fwd": 2 * C * 4, "wm_bn_train_bwd": full, "wm_bn_train_bwd_from_stats": 7 * G * C * 4,
        "wm_bn_relu_maxpool_bwd": full_bytes(2 * 8 * 8, 64, 2), "wm_bn_sync_fwd_sums": full,
        "wm_bn_sync_fwd_apply": 2 * G * C * 4, "wm_bn_sync_bwd_sums": full, "wm_bn_sync_bwd_apply": 7 * G * C * 4,
    }
    assert set(minimum) == set(SHAPED)
    for name, need in minimum.items():
        assert call(lib, name, workspace_bytes=need - 1) == EWORKSPACE, name
        assert call(lib, name, workspace_bytes=0) == EWORKSPACE, name
    # the wide (one thread per channel) forms ask for the same sizes, although they use none of it
    for name in ("wm_bn_train_fwd", "wm_bn_train_stats", "wm_bn_train_bwd", "wm_bn_sync_bwd_sums"):
        assert call(lib, name, **WIDE, workspace_bytes=wide - 1) == EWORKSPACE, name
    assert call(lib, "wm_bn_relu_maxpool_bwd", **WIDE_POOLED, workspace_bytes=full_bytes(512, 4096, 2) - 1) == EWORKSPACE
    assert call(lib, "wm_bn_eval_fwd", **WIDE, workspace_bytes=2 * 4096 * 4 - 1) == EWORKSPACE
    assert call(lib, "wm_bn_sync_fwd_apply", **WIDE, group_count=256, workspace_bytes=2 * 2 * 4096 * 4 - 1) == EWORKSPACE
    assert call(lib, "wm_bn_sync_bwd_apply", **WIDE, group_count=256, workspace_bytes=7 * 2 * 4096 * 4 - 1) == EWORKSPACE
    # a larger, narrow shape (layer4 of the ResNet-18 step)
    rows, C = 2 * 256 * 7 * 7, 512
    for name in ("wm_bn_train_fwd", "wm_bn_train_stats", "wm_bn_train_bwd", "wm_bn_sync_fwd_sums", "wm_bn_sync_bwd_sums"):
        assert call(lib, name, rows=rows, C=C, workspace_bytes=1634560 - 1) == EWORKSPACE, name


def test_statistics_slots_validation(lib):
    G, C = 2, 64
    # a slot count that is not positive, with slots given
    for name in ("wm_bn_train_fwd_from_stats", "wm_bn_train_bwd_from_stats"):
        for tiles in (0, -4):
            assert call(lib, name, stat_tiles=tiles) == EINVAL, name
            assert call(lib, name, stat_tiles=tiles, C=60, workspace_bytes=0) == EINVAL, name    # ahead of the shape check
    for name in SLOTS_OPTIONAL:
        for tiles in (0, -4):
            assert call(lib, name, stat_part=FAKE, stat_tiles=tiles) == EINVAL, name
            assert call(lib, name, stat_part=FAKE, stat_tiles=tiles, workspace_bytes=0) == EINVAL, name   # ahead of workspace
            assert call(lib, name, stat_part=FAKE, stat_tiles=tiles, C=60) == EUNSUPPORTED, name          # behind the shape
    # more than 512 slots per group are pre-reduced to 128 per group in the workspace: what suffices without is too small
    scratch = scratch_bytes(513, C, G)
    assert scratch == 2 * 128 * 2 * 64 * 4 and scratch_bytes(512, C, G) == 0
    for tiles in (513, 6272):
        for name, base in (("wm_bn_train_fwd_from_stats", 2 * G * C * 4), ("wm_bn_train_bwd_from_stats", 7 * G * C * 4)):
            assert call(lib, name, stat_tiles=tiles, workspace_bytes=base) == EWORKSPACE, name
            assert call(lib, name, stat_tiles=tiles, workspace_bytes=base + scratch - 1) == EWORKSPACE, name
        for name in SLOTS_OPTIONAL:   # (these two need only the pre-reduction scratch)
            assert call(lib, name, stat_part=FAKE, stat_tiles=tiles, workspace_bytes=0) == EWORKSPACE, name
            assert call(lib, name, stat_part=FAKE, stat_tiles=tiles, workspace_bytes=scratch - 1) == EWORKSPACE, name
    # with slots the full-size workspace is not asked for; without them it is (stat_tiles is then ignored)
    for name in SLOTS_OPTIONAL:
        assert call(lib, name, stat_tiles=0, workspace_bytes=full_bytes(1024, C, G) - 1) == EWORKSPACE, name


def test_sync_apply_group_count(lib):
    for name in ("wm_bn_sync_fwd_apply", "wm_bn_sync_bwd_apply"):
        for ws in (AMPLE, 0):   # ahead of the workspace check
            assert call(lib, name, group_count=511, workspace_bytes=ws) == EINVAL, name     # fewer than this rank's rows
            assert call(lib, name, group_count=0, workspace_bytes=ws) == EINVAL, name
            assert call(lib, name, group_count=1 << 31, workspace_bytes=ws) == EINVAL, name
        assert call(lib, name, group_count=511, C=60) == EUNSUPPORTED, name                  # behind the shape check
        assert call(lib, name, **WIDE, group_count=255) == EINVAL, name


def test_wide_shape_restrictions(lib):
    wide = full_bytes(512, 4096, 2)
    # the from-statistics backward has no wide form, and says so before it looks at the workspace
    for ws in (AMPLE, 0):
        assert call(lib, "wm_bn_train_bwd_from_stats", **WIDE, workspace_bytes=ws) == EUNSUPPORTED
    # the wide forward writes no ReLU bit mask; the workspace check precedes this one
    assert call(lib, "wm_bn_train_fwd", **WIDE, relu_mask=FAKE, workspace_bytes=wide) == EUNSUPPORTED
    assert call(lib, "wm_bn_train_fwd", **WIDE, relu_mask=FAKE) == EUNSUPPORTED
    assert call(lib, "wm_bn_train_fwd", **WIDE, relu_mask=FAKE, workspace_bytes=wide - 1) == EWORKSPACE
    # the wide backward has no pooled gradient source; again behind the workspace check
    assert call(lib, "wm_bn_relu_maxpool_bwd", **WIDE_POOLED, workspace_bytes=wide) == EUNSUPPORTED
    assert call(lib, "wm_bn_relu_maxpool_bwd", **WIDE_POOLED, ysel=None) == EUNSUPPORTED
    assert call(lib, "wm_bn_relu_maxpool_bwd", **WIDE_POOLED, workspace_bytes=wide - 1) == EWORKSPACE


def test_relu_mask_from_y_needs_gamma_and_beta(lib):
    # the mask is recomputed as bf16(y * scale + shift) > 0: without the output tensor, gamma and beta are required.
    # Checked behind the workspace size.
    need = {"wm_bn_train_bwd": full_bytes(1024, 64, 2), "wm_bn_sync_bwd_sums": full_bytes(1024, 64, 2),
            "wm_bn_sync_bwd_apply": 7 * 2 * 64 * 4}
    for name, ws in need.items():
        for missing in (dict(gamma=None), dict(beta=None), dict(gamma=None, beta=None)):
            assert call(lib, name, relu_from_y=1, **missing, workspace_bytes=ws) == EINVAL, name
            assert call(lib, name, relu_from_y=1, **missing, workspace_bytes=ws - 1) == EWORKSPACE, name
    # (wm_bn_sync_bwd_sums checks it ahead of choosing the wide form)
    assert call(lib, "wm_bn_sync_bwd_sums", **WIDE, relu_from_y=1, gamma=None) == EINVAL


def test_pooled_backward_groups_must_divide_the_pooled_rows(lib):
    # 1 image of 2 x 2 pixels in two groups: 4 rows split, the single pooled row does not
    assert call(lib, "wm_bn_relu_maxpool_bwd", N=1, H=2, W=2, G=2) == EUNSUPPORTED
    assert call(lib, "wm_bn_relu_maxpool_bwd", N=1, H=2, W=2, G=2, workspace_bytes=full_bytes(4, 64, 2) - 1) == EWORKSPACE
