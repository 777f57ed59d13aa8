"""Every C entry point of csrc/bn.hip against tests/kernel_check.py: bn_forward_ref / bn_backward_ref in float64, with the
derived yardstick of check() (tolerance tier) and with torch.equal on the lattice families (exact tier).

Tolerance tier: bf16 tensors (out, dy, dz) with FACTOR against the emulation that rounds where the kernel rounds; float32 sums
(dgamma, dbeta, sums) with F32_SUM_FACTOR and f32_sum_floor against the float32 restatement; save_mean, save_invstd, scale,
shift and the running statistics against the float32 restatement with F32_SUM_FACTOR as well -- they are functions of the
float32 block sums, whose whole error is summation-order noise, and the restatement (rows in order inside a block) is one
realisation of it, the kernel's (row lanes, then LDS) another: the case kernel_check.F32_SUM_FACTOR is defined for.  All
float32 tensors carry kernel_check.f32_stat_floor / f32_sum_floor as absolute term, on criteria 1 and 2 as well (floor_all):
on two or three rows the restatement often lands on the exact value and would ask the same of every other order.

Every output (and the workspace) lies inside a larger buffer filled with a sentinel; the margins are asserted untouched after
every call, so an overrun of a few elements fails an assertion here.  Shapes: the smallest that reach each path of the launch
arithmetic, which the tests mirror (kernel_check.bn_reduce_blocks, bn_chunk_pow2, bn_stream_grid) and assert."""

import kernel_check as kc
import pytest
import torch
from guarded import DEV, Guarded, finish, ok, stream

EUNSUPPORTED = -2
FAKE = 4096             # never dereferenced: the calls that take it fail validation first
EPS, MOM = 1e-5, 0.1
MOM_DYADIC = 0.125

# (rows / G, C): what each reaches is asserted in test_launch_arithmetic_of_the_shapes
SMALL = [(3, 8), (2, 64), (1367, 24), (530, 40), (523, 64), (37, 1032), (37, 2048)]
# the forward lattice needs rows / G even: the even shapes above and even neighbours of the odd ones (the ragged second block
# of 1367 x 24 and the ragged four-row trips of 523 x 64 exist only at odd counts and stay with the tolerance tier)
EXACT_FWD = [(2, 64), (530, 40), (4, 8), (1366, 24), (524, 64), (38, 1032), (38, 2048)]
# the backward lattice needs rows / G a power of two (s1 / M and s2 / M exact): the nearest powers of two that keep the path
# (85 row lanes and two blocks at C = 24; non-POW2 apply at C = 40; several four-row trips at C = 64; 129 lanes; one row per trip)
EXACT_BWD = [(2, 64), (4, 8), (2048, 24), (512, 40), (512, 64), (32, 1032), (32, 2048)]
GROUPS = [1, 2, 3]
WIDE_C, WIDE_RPG, WIDE_G = [2056, 4096, 16384], [2, 5, 33], [1, 2]
SLOT_T = [1, 3, 512, 513, 1000]


@pytest.fixture(scope="module")
def lib():
    from ssl_wafermap_amd import _lib

    if not _lib.LIB_PATH.exists():
        from importlib import import_module

        import_module("ssl_wafermap_amd.build").build(verbose=False)
    return _lib.load()


def dbf(t):
    return None if t is None else t.bfloat16().to(DEV).contiguous()


def df(t):
    return None if t is None else t.float().to(DEV).contiguous()


def ptr(t):
    return 0 if t is None else (t.ptr if isinstance(t, Guarded) else t.data_ptr())


def scratch_floats(t, g, c):
    return g * kc.BN_SLOTS_REDUCED * 2 * c if t > kc.BN_SLOTS_DIRECT else 0


def workspace(nbytes):
    return Guarded((max(int(nbytes), 256),), torch.uint8)


# ------------------------------------------------------------------------------------------------ entry points
def train_fwd(lib, b, g, eps, mom, relu, use_res, want_mask, affine=True, slots=None, calls=1, stats_only=False):
    """wm_bn_train_fwd / _from_stats / wm_bn_train_stats -> dict of CPU tensors"""
    rows, c = b["y"].shape
    y, res = dbf(b["y"]), dbf(b["residual"]) if use_res else None
    gamma, beta = (df(b["gamma"]), df(b["beta"])) if affine else (None, None)
    rm, rv = Guarded((c,), torch.float32, b["running_mean"]), Guarded((c,), torch.float32, b["running_var"])
    nbt = Guarded((1,), torch.int64, torch.tensor([5]))
    mean, invstd = Guarded((g, c), torch.float32), Guarded((g, c), torch.float32)
    out = None if stats_only else Guarded((rows, c), torch.bfloat16)
    mask = Guarded((rows, c // 8), torch.uint8) if want_mask else None
    scale, shift = (Guarded((g, c), torch.float32), Guarded((g, c), torch.float32)) if stats_only else (None, None)
    sl = df(slots)
    t = 0 if slots is None else slots.shape[1]
    if stats_only:
        ws = workspace(scratch_floats(t, g, c) * 4 if slots is not None else lib.wm_bn_workspace_bytes(rows, c, g))
    else:
        ws = workspace((2 * g * c + scratch_floats(t, g, c)) * 4 if slots is not None else lib.wm_bn_workspace_bytes(rows, c, g))
    for _ in range(calls):
        if stats_only:
            ok(lib, lib.wm_bn_train_stats(y.data_ptr(), ptr(gamma), ptr(beta), rm.ptr, rv.ptr, nbt.ptr, rows, c, g, eps, mom, mean.ptr,
                                          invstd.ptr, scale.ptr, shift.ptr, ptr(sl), t, ws.ptr, ws.t.numel(), stream()), "wm_bn_train_stats")
        elif slots is not None:
            ok(lib, lib.wm_bn_train_fwd_from_stats(y.data_ptr(), ptr(res), ptr(gamma), ptr(beta), rm.ptr, rv.ptr, nbt.ptr, rows, c, g, eps,
                                                   mom, relu, mean.ptr, invstd.ptr, out.ptr, ptr(mask), sl.data_ptr(), t, ws.ptr,
                                                   ws.t.numel(), stream()), "wm_bn_train_fwd_from_stats")
        else:
            ok(lib, lib.wm_bn_train_fwd(y.data_ptr(), ptr(res), ptr(gamma), ptr(beta), rm.ptr, rv.ptr, nbt.ptr, rows, c, g, eps, mom, relu,
                                        mean.ptr, invstd.ptr, out.ptr, ptr(mask), ws.ptr, ws.t.numel(), stream()), "wm_bn_train_fwd")
    finish("training forward")
    got = {"mean": mean.t, "invstd": invstd.t, "running_mean": rm.t, "running_var": rv.t, "nbt": nbt.t}
    if not stats_only:
        got["out"] = out.t
    if mask is not None:
        got["relu_mask"] = mask.t
    if stats_only:
        got.update(scale=scale.t, shift=shift.t)
    return {k: v.cpu() for k, v in got.items()}


def train_bwd(lib, b, g, mask_form, want_dz, accumulate, sync=None):
    """wm_bn_train_bwd (sync None) or wm_bn_sync_bwd_sums (sync "sums") / wm_bn_sync_bwd_apply (sync = (group_count, totals)).
    mask_form: None (form 0), "out" (out_relu), "y" (recomputed)."""
    rows, c = b["bn_y"].shape
    y, dout = dbf(b["bn_y"]), dbf(b["dout"])
    out_relu = dbf(b["relu_x"]) if mask_form == "out" else None
    gamma, beta, mean, invstd = df(b["gamma"]), df(b["beta"]), df(b["mean"]), df(b["invstd"])
    init = b["acc"] if accumulate else (None, None)
    dgamma, dbeta = Guarded((c,), torch.float32, init[0]), Guarded((c,), torch.float32, init[1])
    dy = Guarded((rows, c), torch.bfloat16)
    dz = Guarded((rows, c), torch.bfloat16) if want_dz else None
    from_y = 1 if mask_form == "y" else 0
    got = {}
    if sync is None:
        ws = workspace(lib.wm_bn_workspace_bytes(rows, c, g))
        ok(lib, lib.wm_bn_train_bwd(y.data_ptr(), dout.data_ptr(), ptr(out_relu), from_y, gamma.data_ptr(), beta.data_ptr(), mean.data_ptr(),
                                    invstd.data_ptr(), rows, c, g, dgamma.ptr, dbeta.ptr, int(accumulate), dy.ptr, ptr(dz), ws.ptr,
                                    ws.t.numel(), stream()), "wm_bn_train_bwd")
        got.update(dy=dy.t, dgamma=dgamma.t, dbeta=dbeta.t)
    elif sync == "sums":
        ws = workspace(lib.wm_bn_workspace_bytes(rows, c, g))
        sums = Guarded((g, 2, c), torch.float32)
        ok(lib, lib.wm_bn_sync_bwd_sums(y.data_ptr(), dout.data_ptr(), ptr(out_relu), from_y, gamma.data_ptr(), beta.data_ptr(),
                                        mean.data_ptr(), invstd.data_ptr(), rows, c, g, dgamma.ptr, dbeta.ptr, int(accumulate), sums.ptr,
                                        ws.ptr, ws.t.numel(), stream()), "wm_bn_sync_bwd_sums")
        got.update(sums=sums.t, dgamma=dgamma.t, dbeta=dbeta.t)
    else:
        count, totals = sync
        ws = workspace(7 * g * c * 4)
        tot = df(totals)
        ok(lib, lib.wm_bn_sync_bwd_apply(y.data_ptr(), dout.data_ptr(), ptr(out_relu), from_y, gamma.data_ptr(), beta.data_ptr(),
                                         mean.data_ptr(), invstd.data_ptr(), rows, c, g, count, tot.data_ptr(), dy.ptr, ptr(dz), ws.ptr,
                                         ws.t.numel(), stream()), "wm_bn_sync_bwd_apply")
        got.update(dy=dy.t)
    finish("training backward")
    if dz is not None and sync != "sums":
        got["dz"] = dz.t
    return {k: v.cpu() for k, v in got.items()}


# ------------------------------------------------------------------------------------------------ comparisons
def check_bf16(got, ref, emu, what, kern):
    """`kern` goes in front of the logged name: the worst ratio per kernel and tensor is read from the parity log"""
    return kc.check(got, ref, emu, f"[{kern}] {what}")


def check_f32(got, ref, emu, what, kern, floor=0.0, factor=kc.F32_SUM_FACTOR):
    return kc.check(got, ref, emu, f"[{kern}] {what}", factor=factor, abs_floor=floor, floor_all=True)


def big_value_factor(rpg, c):
    """The factor of the float32 statistics on the big_value family, wider than F32_SUM_FACTOR and derived from the launch
    arithmetic: next to one element of 1e4 every later addition of the channel's sum rounds at THAT magnitude, and bn_reduce
    has a chain of ceil(block rows / row lanes) + row lanes + blocks additions behind it -- sqrt(chain) roundings as a random
    walk.  The row-order restatement is no yardstick for this: bf16 inputs lie on a grid of 2^-9 and coarser from 0.5 up, so
    added one by one to an accumulator near 2e4 (float32 step 2^-9) nearly all of them add exactly.  Measured on the MI355X at
    530 x 40, G = 1 (chain 62): save_mean 4.7 roundings of the largest channel's magnitude, 1.18x the F32_SUM_FACTOR bound."""
    blocks = kc.bn_block_rows(rpg, c)
    chain = -(-max(b - a for a, b in blocks) // kc.bn_rpp(c)) + kc.bn_rpp(c) + len(blocks)
    return max(kc.F32_SUM_FACTOR, chain ** 0.5)


def equal(got, ref, what):
    got, ref = got.double(), ref.double()
    assert torch.equal(got, ref), f"{what}: {(got != ref).sum().item()} of {ref.numel()} differ, max {float((got - ref).abs().max()):.3g}"


def mask_of_stored(got):
    """relu_mask must be the stored output > 0, bit for bit"""
    assert torch.equal(got["relu_mask"], kc.bn_pack_mask(got["out"].float() > 0)), "relu_mask is not (stored out > 0)"


def forward_refs(b, g, eps, mom, relu, use_res, affine=True, slots=None, wide=False, calls=1):
    """(float64, emulation) of `calls` consecutive forward calls (the running statistics are carried along)"""
    res = b["residual"] if use_res else None
    gamma, beta = (b["gamma"], b["beta"]) if affine else (None, None)
    pair = []
    for emulate in (False, True):
        run = (b["running_mean"], b["running_var"])
        for _ in range(calls):
            r = kc.bn_forward_ref(b["y"], res, gamma, beta, g, eps, mom, relu, run, slots=slots, emulate=emulate, wide=wide and emulate)
            run = (r["running_mean"], r["running_var"])
        pair.append(r)
    return pair


def compare_forward(got, ref, emu, b, g, tag, kern, stats_only=False, factor=kc.F32_SUM_FACTOR):
    rows = b["y"].shape[0]
    m = rows // g
    if not stats_only:
        check_bf16(got["out"], ref["out"], emu["out"], f"{tag} out", kern)
    names = ("mean", "invstd", "running_mean", "running_var") + (("scale", "shift") if stats_only else ())
    y64 = b["y"].double()
    # one float32 rounding at the scale of what enters each statistic (kernel_check.f32_stat_floor)
    floors = {"mean": kc.f32_sum_floor(y64) / m,
              "running_mean": kc.f32_sum_floor(y64) / m + kc.f32_stat_floor(b["running_mean"]),
              "running_var": kc.f32_sum_floor(y64 * y64) / max(m - 1, 1) + kc.f32_stat_floor(b["running_var"])}
    for name in names:
        check_f32(got[name], ref[name], emu[name], f"{tag} {name}", kern, floors.get(name, kc.f32_stat_floor(ref[name])), factor)


def compare_backward(got, ref, emu, b, tag, kern, terms=None):
    check_bf16(got["dy"], ref["dy"], emu["dy"], f"{tag} dy", kern)
    if "dz" in got:
        check_bf16(got["dz"], ref["dz"], emu["dz"], f"{tag} dz", kern)
    if "dgamma" in got:
        dz, xh = terms
        check_f32(got["dgamma"], ref["dgamma"], emu["dgamma"], f"{tag} dgamma", kern, kc.f32_sum_floor(dz * xh))
        check_f32(got["dbeta"], ref["dbeta"], emu["dbeta"], f"{tag} dbeta", kern, kc.f32_sum_floor(dz))


def backward_terms(b, ref, g):
    """(dz, dz xhat) [rows, C] float64: the summed terms, for f32_sum_floor"""
    rows = b["bn_y"].shape[0]
    grp = torch.arange(rows) // (rows // g)
    dz = ref["dz"] if ref["dz"] is not None else b["dout"].double()
    return dz, (b["bn_y"].double() - b["mean"].double()[grp]) * b["invstd"].double()[grp]


# ------------------------------------------------------------------------------------------------ launch arithmetic
def test_launch_arithmetic_of_the_shapes():
    """What every narrow shape is there for, restated from reduce_blocks / launch_reduce / chunk_pow2 / stream_grid"""
    assert kc.bn_rpp(8) == 256 and 3 < 256                                        # fewer rows than the 256 row lanes
    assert kc.bn_rpp(24) == 85 and 85 * 3 == 255                                  # one idle thread
    assert kc.bn_block_rows(1367, 24) == [(0, 684), (684, 1367)]                  # two blocks, the second one row short
    assert not kc.bn_chunk_pow2(40) and 40 % 32 == 8 and kc.bn_chunk_pow2(64) and not kc.bn_chunk_pow2(24)
    rpp = kc.bn_rpp(64)
    assert rpp == 32 and kc.bn_block_rows(523, 64) == [(0, 262), (262, 523)] and 262 > 4 * rpp and 262 % (4 * rpp) != 0
    assert kc.bn_rpp(1032) == 1 and 1032 // 8 == 129 and kc.bn_rpp(2048) == 1 and not kc.bn_chunk_pow2(1032)
    items = 2 * 8200 * (512 // 8)
    cap = kc.BN_STREAM_BLOCKS * kc.BN_THREADS
    assert items > cap and kc.bn_chunk_pow2(512) and kc.bn_stream_grid(items) == kc.BN_STREAM_BLOCKS
    assert (0 >> 6) // 8200 == 0 and (cap >> 6) // 8200 == 1                      # thread 0: first trip group 0, second trip group 1
    assert -(-16500 // (kc.bn_rpp(512) * 16)) > 256 and kc.bn_reduce_blocks(16500, 512) == 256
    assert kc.bn_block_rows(16500, 512)[-1] == (16500, 16500)                     # (the last block of the capped grid is empty)
    assert kc.bn_prereduce_plan(512) == (1, 512) and kc.bn_prereduce_plan(513) == (8, 65) and 513 - 64 * 8 == 1
    assert kc.bn_prereduce_plan(1000) == (8, 125)
    for c in WIDE_C:
        assert all(kc.bn_wide(rpg * g, c, g) for rpg in WIDE_RPG for g in WIDE_G)
    assert not kc.bn_wide(2, 16392, 1) and not kc.bn_wide(65537, 2056, 1)


def test_unsupported_widths_are_refused(lib):
    """C = 16392 (above the wide limit) and C = 2056 with 65537 rows per group: validation only, fake pointers"""
    for rows, c in ((8, 16392), (65537, 2056)):
        big = 1 << 40
        calls = {
            "wm_bn_train_fwd": lambda: lib.wm_bn_train_fwd(FAKE, None, FAKE, FAKE, FAKE, FAKE, None, rows, c, 1, EPS, MOM, 1, FAKE, FAKE,
                                                           FAKE, None, FAKE, big, None),
            "wm_bn_eval_fwd": lambda: lib.wm_bn_eval_fwd(FAKE, None, FAKE, FAKE, FAKE, FAKE, rows, c, EPS, 1, FAKE, FAKE, big, None),
            "wm_bn_train_bwd": lambda: lib.wm_bn_train_bwd(FAKE, FAKE, None, 0, FAKE, FAKE, FAKE, FAKE, rows, c, 1, FAKE, FAKE, 0, FAKE,
                                                           None, FAKE, big, None),
            "wm_bn_sync_fwd_sums": lambda: lib.wm_bn_sync_fwd_sums(FAKE, rows, c, 1, None, 0, FAKE, FAKE, big, None),
            "wm_bn_sync_bwd_sums": lambda: lib.wm_bn_sync_bwd_sums(FAKE, FAKE, None, 0, FAKE, FAKE, FAKE, FAKE, rows, c, 1, FAKE, FAKE, 0,
                                                                   FAKE, FAKE, big, None),
        }
        for name, call in calls.items():
            assert call() == EUNSUPPORTED, (name, rows, c)


# ------------------------------------------------------------------------------------------------ wm_bn_train_fwd
@pytest.mark.gpu
@pytest.mark.parametrize("g", GROUPS)
@pytest.mark.parametrize("rpg,c", EXACT_FWD)
def test_train_fwd_exact(lib, rpg, c, g):
    """Lattice, eps = 0, dyadic momentum: out, relu_mask, save_mean, save_invstd and running_mean equal float64 bit for bit;
    running_var where rows / G - 1 is a power of two (else it has a rounding and belongs to the tolerance tier)."""
    b = kc.bn_forward_inputs("lattice", rpg * g, c, g, seed=rpg + c + g)
    for use_res, relu, affine in ((True, 1, True), (False, 0, False), (False, 1, True)):
        got = train_fwd(lib, b, g, 0.0, MOM_DYADIC, relu, use_res, want_mask=True, affine=affine, calls=2)
        ref, _ = forward_refs(b, g, 0.0, MOM_DYADIC, relu, use_res, affine, calls=2)
        assert torch.equal(ref["mean"], b["mean"].double()) and torch.equal(ref["invstd"], 1.0 / b["s"].double())
        assert torch.equal(ref["out"], ref["out"].float().bfloat16().double())                 # the lattice is bf16-exact
        for name in ("out", "mean", "invstd", "running_mean"):
            equal(got[name], ref[name], f"{name} res={use_res} relu={relu}")
        if (rpg - 1) & (rpg - 2) == 0:
            equal(got["running_var"], ref["running_var"], "running_var")
        assert torch.equal(got["relu_mask"], kc.bn_pack_mask(ref["relu_mask"]))
        mask_of_stored(got)
        assert int(got["nbt"]) == 5 + 2 * g


@pytest.mark.gpu
@pytest.mark.parametrize("family", kc.BN_FORWARD_FAMILIES[1:])
@pytest.mark.parametrize("g", GROUPS)
@pytest.mark.parametrize("rpg,c", SMALL)
def test_train_fwd(lib, rpg, c, g, family):
    b = kc.bn_forward_inputs(family, rpg * g, c, g, seed=rpg + c)
    tag = f"train_fwd {family} {rpg}x{c} G={g}"
    factor = big_value_factor(rpg, c) if family == "big_value" else kc.F32_SUM_FACTOR
    # residual + relu + mask, two consecutive calls (the running statistics move twice); then the bare form with NULL gamma / beta
    got = train_fwd(lib, b, g, EPS, MOM, 1, True, want_mask=True, calls=2)
    ref, emu = forward_refs(b, g, EPS, MOM, 1, True, calls=2)
    compare_forward(got, ref, emu, b, g, tag, "bn_reduce<0> / bn_fwd_finalize / bn_apply", factor=factor)
    mask_of_stored(got)
    assert int(got["nbt"]) == 5 + 2 * g
    got = train_fwd(lib, b, g, EPS, MOM, 0, False, want_mask=False, affine=False)
    ref, emu = forward_refs(b, g, EPS, MOM, 0, False, affine=False)
    compare_forward(got, ref, emu, b, g, tag + " bare", "bn_reduce<0> / bn_fwd_finalize / bn_apply", factor=factor)
    assert int(got["nbt"]) == 5 + g


@pytest.mark.gpu
@pytest.mark.parametrize("rpg,c,g", [(8200, 512, 2), (16500, 512, 1)])
def test_train_fwd_beyond_the_grid_caps(lib, rpg, c, g):
    """More 16-byte items than the apply grid's 2^20 threads (a thread's second trip lies in the other group), and more rows
    than 256 reduce blocks of 64 take (the blocks grow instead)."""
    b = kc.bn_forward_inputs("randn", rpg * g, c, g, seed=rpg)
    got = train_fwd(lib, b, g, EPS, MOM, 1, True, want_mask=True)
    ref, emu = forward_refs(b, g, EPS, MOM, 1, True)
    compare_forward(got, ref, emu, b, g, f"train_fwd randn {rpg}x{c} G={g}", "bn_reduce<0> / bn_fwd_finalize / bn_apply")
    mask_of_stored(got)


@pytest.mark.gpu
@pytest.mark.parametrize("g", WIDE_G)
@pytest.mark.parametrize("rpg", WIDE_RPG)
@pytest.mark.parametrize("c", WIDE_C)
def test_train_fwd_wide(lib, c, rpg, g):
    """bn_col_fwd.  Exact tier (rows / G even only): rsqrtf is an approximation the hardware documents to one float32 ulp, so
    save_invstd is held to one ulp of the exact power of two and out -- whose bf16 rounding absorbs that -- to equality."""
    for family in ("randn", "offset", "constant"):
        b = kc.bn_forward_inputs(family, rpg * g, c, g, seed=rpg + c)
        got = train_fwd(lib, b, g, EPS, MOM, 1, True, want_mask=False, calls=2)
        ref, emu = forward_refs(b, g, EPS, MOM, 1, True, wide=True, calls=2)
        compare_forward(got, ref, emu, b, g, f"train_fwd wide {family} {rpg}x{c} G={g}", "bn_col_fwd")
        assert int(got["nbt"]) == 5 + 2 * g
    if rpg % 2 == 0:
        b = kc.bn_forward_inputs("lattice", rpg * g, c, g, seed=c)
        got = train_fwd(lib, b, g, 0.0, MOM_DYADIC, 1, True, want_mask=False)
        ref, _ = forward_refs(b, g, 0.0, MOM_DYADIC, 1, True)
        for name in ("out", "mean", "running_mean"):
            equal(got[name], ref[name], name)
        assert bool(((got["invstd"].double() - ref["invstd"]).abs() <= 2.0 ** -23 * ref["invstd"]).all())


# ------------------------------------------------------------------------------------------------ slots
def forward_slots(b, g, t, seed):
    y = b["y"].double()
    return kc.bn_row_slots(y, y * y, g, t, seed)


@pytest.mark.gpu
@pytest.mark.parametrize("t", SLOT_T)
@pytest.mark.parametrize("g", [1, 3])
def test_train_stats_and_fwd_from_stats_with_slots(lib, t, g):
    """The statistics come from [G][T][2][C] slots: read directly up to 512 per group, pre-reduced by stats_prereduce beyond
    (513: R = 8, 65 output slots, the last made of one slot).  Reference: the double sum of the same float32 slots."""
    rpg, c = 530, 40
    for family in ("randn", "offset", "lattice"):
        lat = family == "lattice"
        eps, mom = (0.0, MOM_DYADIC) if lat else (EPS, MOM)
        b = kc.bn_forward_inputs(family, rpg * g, c, g, seed=t)
        slots = forward_slots(b, g, t, seed=t + g)
        assert t < 4 or bool((slots[:, :, 0].abs().sum(-1) == 0).any()) or lat, "some slots should be empty"
        ref, emu = forward_refs(b, g, eps, mom, 1, True, slots=slots)
        got_s = train_fwd(lib, b, g, eps, mom, 1, False, False, slots=slots, stats_only=True)
        got_f = train_fwd(lib, b, g, eps, mom, 1, True, True, slots=slots)
        mask_of_stored(got_f)
        assert int(got_s["nbt"]) == 5 + g and int(got_f["nbt"]) == 5 + g
        if lat:
            for name in ("mean", "invstd", "running_mean", "scale", "shift"):
                equal(got_s[name], ref[name], f"stats {name} T={t}")
            for name in ("out", "mean", "invstd", "running_mean"):
                equal(got_f[name], ref[name], f"from_stats {name} T={t}")
        else:
            compare_forward(got_s, ref, emu, b, g, f"train_stats {family} T={t} G={g}", "stats_prereduce / bn_fwd_finalize", stats_only=True)
            compare_forward(got_f, ref, emu, b, g, f"fwd_from_stats {family} T={t} G={g}", "stats_prereduce / bn_fwd_finalize / bn_apply")


@pytest.mark.gpu
def test_train_fwd_from_stats_at_a_wide_width(lib):
    """With slots the finalize + apply kernels serve any width (no bn_col_fwd): C = 2056, 65 finalize blocks with 8 valid
    channels in the last, 257 lanes per row"""
    rpg, c, g, t = 34, 2056, 2, 3
    for family in ("randn", "lattice"):
        lat = family == "lattice"
        eps, mom = (0.0, MOM_DYADIC) if lat else (EPS, MOM)
        b = kc.bn_forward_inputs(family, rpg * g, c, g, seed=3)
        slots = forward_slots(b, g, t, seed=5)
        got = train_fwd(lib, b, g, eps, mom, 1, True, True, slots=slots)
        ref, emu = forward_refs(b, g, eps, mom, 1, True, slots=slots)
        mask_of_stored(got)
        if lat:
            for name in ("out", "mean", "invstd", "running_mean"):
                equal(got[name], ref[name], name)
        else:
            compare_forward(got, ref, emu, b, g, f"fwd_from_stats wide {family}", "bn_fwd_finalize / bn_apply at C = 2056")


# ------------------------------------------------------------------------------------------------ eval
@pytest.mark.gpu
@pytest.mark.parametrize("rows,c", [(3, 8), (530, 40), (523, 64), (37, 1032)] + [(r, c) for c in WIDE_C for r in WIDE_RPG])
def test_eval_fwd_and_scale_shift(lib, rows, c):
    """Against float64 on the given running statistics; every fourth channel has a running variance of 0 (invstd = eps^-1/2)"""
    b = kc.bn_forward_inputs("randn", rows, c, 1, seed=rows)
    b["running_var"][::4] = 0.0
    y, res = dbf(b["y"]), dbf(b["residual"])
    gamma, beta, rm, rv = df(b["gamma"]), df(b["beta"]), df(b["running_mean"]), df(b["running_var"])
    for use_res, relu, affine in ((True, 1, True), (False, 0, False)):
        ga, be = (gamma, beta) if affine else (None, None)
        out, ws = Guarded((rows, c), torch.bfloat16), workspace(2 * c * 4)
        scale, shift = Guarded((c,), torch.float32), Guarded((c,), torch.float32)
        ok(lib, lib.wm_bn_eval_fwd(y.data_ptr(), ptr(res if use_res else None), ptr(ga), ptr(be), rm.data_ptr(), rv.data_ptr(), rows, c, EPS,
                                   relu, out.ptr, ws.ptr, ws.t.numel(), stream()), "wm_bn_eval_fwd")
        ok(lib, lib.wm_bn_eval_scale_shift(ptr(ga), ptr(be), rm.data_ptr(), rv.data_ptr(), c, EPS, scale.ptr, shift.ptr, stream()),
           "wm_bn_eval_scale_shift")
        finish("eval forward")
        args = (b["y"], b["residual"] if use_res else None, b["gamma"] if affine else None, b["beta"] if affine else None,
                b["running_mean"], b["running_var"], EPS, relu)
        ref, emu = kc.bn_eval_ref(*args), kc.bn_eval_ref(*args, emulate=True)
        tag = f"eval {rows}x{c} res={use_res}"
        check_bf16(out.t.cpu(), ref["out"], emu["out"], tag + " out", "bn_eval_params / bn_apply")
        # one float32 rounding each: the float32 restatement's own error is the yardstick (FACTOR)
        kc.check(scale.t.cpu(), ref["scale"], emu["scale"], f"[bn_eval_params] {tag} scale")
        kc.check(shift.t.cpu(), ref["shift"], emu["shift"], f"[bn_eval_params] {tag} shift")
        assert torch.equal(rm.cpu(), b["running_mean"]) and torch.equal(rv.cpu(), b["running_var"])    # eval leaves them alone


# ------------------------------------------------------------------------------------------------ wm_bn_train_bwd
BWD_FORMS = [(None, False, False), (None, False, True), ("out", True, True), ("out", False, False), ("y", True, False), ("y", False, True)]


def backward_case(lib, b, g, mask_form, want_dz, accumulate, tag, kern, exact, wide=False):
    got = train_bwd(lib, b, g, mask_form, want_dz, accumulate)
    kw = dict(out_relu=b["relu_x"] if mask_form == "out" else None, remask=mask_form == "y", want_dz=True,
              accumulate_into=b["acc"] if accumulate else None)
    args = (b["bn_y"], b["dout"], b["gamma"], b["beta"], b["mean"], b["invstd"], g)
    ref = kc.bn_backward_ref(*args, **kw)
    tag = f"{tag} mask={mask_form} dz={want_dz} acc={accumulate}"
    if exact:
        kc.bn_lattice_exact(ref["pre"])
        equal(got["dy"], kc.bf(ref["dy"]), tag + " dy")
        if want_dz:
            equal(got["dz"], ref["dz"], tag + " dz")
        equal(got["dgamma"], ref["dgamma"], tag + " dgamma")
        equal(got["dbeta"], ref["dbeta"], tag + " dbeta")
    else:
        emu = kc.bn_backward_ref(*args, emulate=True, wide=wide, **kw)
        compare_backward(got, ref, emu, b, tag, kern, backward_terms(b, ref, g))


@pytest.mark.gpu
@pytest.mark.parametrize("g", GROUPS)
@pytest.mark.parametrize("rpg,c", EXACT_BWD)
def test_train_bwd_exact(lib, rpg, c, g):
    b = kc.bn_backward_inputs("lattice", rpg * g, c, g, seed=rpg + c + g)
    assert bool((b["relu_x"] == 0).any())                               # > 0 and >= 0 differ on this data
    for mask_form, want_dz, accumulate in BWD_FORMS:
        backward_case(lib, b, g, mask_form, want_dz, accumulate, f"train_bwd lattice {rpg}x{c} G={g}", "", exact=True)


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["randn", "offset"])
@pytest.mark.parametrize("g", GROUPS)
@pytest.mark.parametrize("rpg,c", SMALL)
def test_train_bwd(lib, rpg, c, g, family):
    b = kc.bn_backward_inputs(family, rpg * g, c, g, seed=rpg + c)
    for mask_form, want_dz, accumulate in BWD_FORMS:
        if mask_form == "y":
            if family == "offset":      # its pre-activations are spread around zero: a recomputed mask would hang on roundings
                continue
            assert kc.bn_preact_margin(b) > 8 * kc.BF16_ULP
        backward_case(lib, b, g, mask_form, want_dz, accumulate, f"train_bwd {family} {rpg}x{c} G={g}",
                      "bn_reduce<1> / bn_bwd_finalize / bn_bwd_apply", exact=False)


@pytest.mark.gpu
@pytest.mark.parametrize("rpg,c,g", [(8200, 512, 2), (16500, 512, 1)])
def test_train_bwd_beyond_the_grid_caps(lib, rpg, c, g):
    b = kc.bn_backward_inputs("randn", rpg * g, c, g, seed=rpg)
    backward_case(lib, b, g, "out", True, False, f"train_bwd randn {rpg}x{c} G={g}", "bn_reduce<1> / bn_bwd_finalize / bn_bwd_apply",
                  exact=False)


@pytest.mark.gpu
@pytest.mark.parametrize("g", WIDE_G)
@pytest.mark.parametrize("rpg", WIDE_RPG)
@pytest.mark.parametrize("c", WIDE_C)
def test_train_bwd_wide(lib, c, rpg, g):
    """bn_col_bwd: float32 sums in row order; the lattice tier where rows / G is a power of two"""
    b = kc.bn_backward_inputs("randn", rpg * g, c, g, seed=rpg + c)
    assert kc.bn_preact_margin(b) > 8 * kc.BF16_ULP
    for mask_form, want_dz, accumulate in ((None, False, True), ("out", True, False), ("y", True, True)):
        backward_case(lib, b, g, mask_form, want_dz, accumulate, f"train_bwd wide randn {rpg}x{c} G={g}", "bn_col_bwd", exact=False, wide=True)
    if rpg & (rpg - 1) == 0:
        b = kc.bn_backward_inputs("lattice", rpg * g, c, g, seed=c)
        for mask_form, want_dz, accumulate in ((None, False, True), ("out", True, False), ("y", True, True)):
            backward_case(lib, b, g, mask_form, want_dz, accumulate, f"train_bwd wide lattice {rpg}x{c} G={g}", "", exact=True)


# ------------------------------------------------------------------------------------------------ wm_bn_train_bwd_from_stats
@pytest.mark.gpu
@pytest.mark.parametrize("t", SLOT_T)
@pytest.mark.parametrize("g", [1, 3])
def test_train_bwd_from_stats(lib, t, g):
    """The slots hold (sum g, sum g (y - mean)) of a row partition; the finalize scales the second by invstd."""
    rpg, c = 512, 40
    for family in ("randn", "offset", "lattice"):
        b = kc.bn_backward_inputs(family, rpg * g, c, g, seed=t)
        grp = torch.arange(rpg * g) // rpg
        gr = b["dout"].double()
        slots = kc.bn_row_slots(gr, gr * (b["bn_y"].double() - b["mean"].double()[grp]), g, t, seed=t + g)
        for accumulate in (False, True):
            y, gd = dbf(b["bn_y"]), dbf(b["dout"])
            gamma, beta, mean, invstd, sl = df(b["gamma"]), df(b["beta"]), df(b["mean"]), df(b["invstd"]), df(slots)
            init = b["acc"] if accumulate else (None, None)
            dgamma, dbeta = Guarded((c,), torch.float32, init[0]), Guarded((c,), torch.float32, init[1])
            dy, ws = Guarded((rpg * g, c), torch.bfloat16), workspace((7 * g * c + scratch_floats(t, g, c)) * 4)
            ok(lib, lib.wm_bn_train_bwd_from_stats(y.data_ptr(), gd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), mean.data_ptr(),
                                                   invstd.data_ptr(), rpg * g, c, g, dgamma.ptr, dbeta.ptr, int(accumulate), dy.ptr,
                                                   sl.data_ptr(), t, ws.ptr, ws.t.numel(), stream()), "wm_bn_train_bwd_from_stats")
            finish("backward from slots")
            got = {"dy": dy.t.cpu(), "dgamma": dgamma.t.cpu(), "dbeta": dbeta.t.cpu()}
            kw = dict(fx_slots=slots, accumulate_into=b["acc"] if accumulate else None)
            args = (b["bn_y"], b["dout"], b["gamma"], b["beta"], b["mean"], b["invstd"], g)
            ref = kc.bn_backward_ref(*args, **kw)
            tag = f"bwd_from_stats {family} T={t} G={g} acc={accumulate}"
            if family == "lattice":
                kc.bn_lattice_exact(ref["pre"])
                equal(got["dy"], kc.bf(ref["dy"]), tag + " dy")
                equal(got["dgamma"], ref["dgamma"], tag + " dgamma")
                equal(got["dbeta"], ref["dbeta"], tag + " dbeta")
            else:
                emu = kc.bn_backward_ref(*args, emulate=True, **kw)
                compare_backward(got, ref, emu, b, tag, "stats_prereduce / bn_bwd_finalize(fx) / bn_bwd_apply<0>", backward_terms(b, ref, g))


# ------------------------------------------------------------------------------------------------ synchronised form
def split_ranks(t, g):
    """rows [G * 2 * rl, C] in (group, rank, row) order -> the two ranks' rows [G * rl, C]"""
    c = t.shape[1]
    v = t.reshape(g, 2, -1, c)
    return [v[:, r].reshape(-1, c).contiguous() for r in range(2)]


def join_ranks(parts, g):
    c = parts[0].shape[1]
    return torch.stack([p.reshape(g, -1, c) for p in parts], 1).reshape(-1, c)


def sync_fwd_sums(lib, y, g):
    rows, c = y.shape
    sums, ws = Guarded((g, 2, c), torch.float32), workspace(lib.wm_bn_workspace_bytes(rows, c, g))
    yd = dbf(y)
    ok(lib, lib.wm_bn_sync_fwd_sums(yd.data_ptr(), rows, c, g, None, 0, sums.ptr, ws.ptr, ws.t.numel(), stream()), "wm_bn_sync_fwd_sums")
    finish("sync forward sums")
    return sums.t.cpu()


def sync_fwd_apply(lib, b, y, res, g, count, totals, eps, mom):
    rows, c = y.shape
    yd, rd, gamma, beta, tot = dbf(y), dbf(res), df(b["gamma"]), df(b["beta"]), df(totals)
    rm, rv = Guarded((c,), torch.float32, b["running_mean"]), Guarded((c,), torch.float32, b["running_var"])
    nbt = Guarded((1,), torch.int64, torch.tensor([5]))
    mean, invstd, out = Guarded((g, c), torch.float32), Guarded((g, c), torch.float32), Guarded((rows, c), torch.bfloat16)
    ws = workspace(2 * g * c * 4)
    ok(lib, lib.wm_bn_sync_fwd_apply(yd.data_ptr(), rd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), rm.ptr, rv.ptr, nbt.ptr, rows, c, g,
                                     count, eps, mom, 1, mean.ptr, invstd.ptr, out.ptr, tot.data_ptr(), ws.ptr, ws.t.numel(), stream()),
       "wm_bn_sync_fwd_apply")
    finish("sync forward apply")
    assert int(nbt.t.cpu()) == 5 + g
    return {"out": out.t.cpu(), "mean": mean.t.cpu(), "invstd": invstd.t.cpu(), "running_mean": rm.t.cpu(), "running_var": rv.t.cpu()}


# (rows per rank and group, C); the lattice twin of each has a power of two as the two ranks' total (the backward's s / M)
SYNC_SHAPES = [(37, 24), (262, 64), (20, 1032)] + [(rl, c) for c in WIDE_C for rl in WIDE_RPG]
SYNC_EXACT = [(32, 24), (256, 64), (16, 1032)] + [(rl, c) for c in WIDE_C for rl in (2, 4, 32)]


@pytest.mark.gpu
@pytest.mark.parametrize("g", [1, 2])
@pytest.mark.parametrize("idx", range(len(SYNC_SHAPES)))
def test_sync_forward_of_two_ranks(lib, idx, g):
    """Two ranks = the two halves of every group of one batch, in one process: sums on each, added on the host, apply on each
    with group_count = the total.  The joined result against the BatchNorm of the whole batch."""
    for family, (rl, c) in (("randn", SYNC_SHAPES[idx]), ("offset", SYNC_SHAPES[idx]), ("lattice", SYNC_EXACT[idx])):
        lat = family == "lattice"
        eps, mom = (0.0, MOM_DYADIC) if lat else (EPS, MOM)
        b = kc.bn_forward_inputs(family, 2 * rl * g, c, g, seed=rl + c)
        ys, rs = split_ranks(b["y"], g), split_ranks(b["residual"], g)
        sums = [sync_fwd_sums(lib, y, g) for y in ys]
        totals = sums[0] + sums[1]
        got = [sync_fwd_apply(lib, b, ys[r], rs[r], g, 2 * rl, totals, eps, mom) for r in range(2)]
        for name in ("mean", "invstd", "running_mean", "running_var"):
            assert torch.equal(got[0][name], got[1][name]), name                 # both ranks hold the same statistics
        whole = dict(got[0], out=join_ranks([got[0]["out"], got[1]["out"]], g))
        ref = kc.bn_forward_ref(b["y"], b["residual"], b["gamma"], b["beta"], g, eps, mom, 1, (b["running_mean"], b["running_var"]))
        tag = f"sync fwd {family} 2x{rl}x{c} G={g}"
        wide = kc.bn_wide(rl * g, c, g)
        kern = "bn_col_sums<0>" if wide else "bn_reduce<0> / bn_sums_finalize"
        # the emulated ranks: their float32 totals (narrow: block sums; wide: a double sum rounded once), added in float32
        esum = [kc.bn_forward_ref(y, None, None, None, g, eps, mom, 0, emulate=not wide)["sums"].float() for y in ys]
        eslots = (esum[0] + esum[1]).unsqueeze(1)
        emu = kc.bn_forward_ref(b["y"], b["residual"], b["gamma"], b["beta"], g, eps, mom, 1, (b["running_mean"], b["running_var"]),
                                slots=eslots, emulate=True)
        if lat:
            for name in ("out", "mean", "invstd", "running_mean"):
                equal(whole[name], ref[name], f"{tag} {name}")
            equal(totals, ref["sums"], f"{tag} sums")
        else:
            for r in range(2):
                y64 = ys[r].double()
                r64 = torch.stack([y64.reshape(g, rl, c).sum(1), (y64 * y64).reshape(g, rl, c).sum(1)], 1)
                check_f32(sums[r], r64, esum[r], f"{tag} rank {r} sums", kern, kc.f32_sum_floor(y64 * y64))
            compare_forward(whole, ref, emu, b, g, tag, f"{kern} / bn_fwd_finalize / bn_apply (sync)")


@pytest.mark.gpu
@pytest.mark.parametrize("g", [1, 2])
@pytest.mark.parametrize("idx", range(len(SYNC_SHAPES)))
def test_sync_backward_of_two_ranks(lib, idx, g):
    for family, (rl, c) in (("randn", SYNC_SHAPES[idx]), ("lattice", SYNC_EXACT[idx])):
        lat = family == "lattice"
        b = kc.bn_backward_inputs(family, 2 * rl * g, c, g, seed=rl + c)
        assert lat or kc.bn_preact_margin(b) > 8 * kc.BF16_ULP
        wide = kc.bn_wide(rl * g, c, g)
        kern = "bn_col_sums<1>" if wide else "bn_reduce<1> / bn_sums_finalize"
        for mask_form in ("out", "y"):
            ranks = []
            for r in range(2):
                br = dict(b)
                for key in ("bn_y", "dout", "relu_x"):
                    br[key] = split_ranks(b[key], g)[r]
                ranks.append(br)
            local = [train_bwd(lib, br, g, mask_form, False, False, sync="sums") for br in ranks]
            totals = local[0]["sums"] + local[1]["sums"]
            applied = [train_bwd(lib, br, g, mask_form, True, False, sync=(2 * rl, totals)) for br in ranks]
            got = {"dy": join_ranks([a["dy"] for a in applied], g), "dz": join_ranks([a["dz"] for a in applied], g),
                   "dgamma": local[0]["dgamma"] + local[1]["dgamma"], "dbeta": local[0]["dbeta"] + local[1]["dbeta"]}
            kw = dict(out_relu=b["relu_x"] if mask_form == "out" else None, remask=mask_form == "y")
            args = (b["bn_y"], b["dout"], b["gamma"], b["beta"], b["mean"], b["invstd"], g)
            ref = kc.bn_backward_ref(*args, **kw)
            tag = f"sync bwd {family} 2x{rl}x{c} G={g} mask={mask_form}"
            if lat:
                kc.bn_lattice_exact(ref["pre"])
                equal(got["dy"], kc.bf(ref["dy"]), tag + " dy")
                for name in ("dz", "dgamma", "dbeta"):
                    equal(got[name], ref[name], f"{tag} {name}")
                equal(totals, ref["sums"], tag + " sums")
            else:
                emu = kc.bn_backward_ref(*args, emulate=True, **kw)
                terms = backward_terms(b, ref, g)
                compare_backward(got, ref, emu, b, tag, f"{kern} / bn_bwd_finalize / bn_bwd_apply<1> (sync)", terms)
                check_f32(totals, ref["sums"], emu["sums"], tag + " sums", kern, kc.f32_sum_floor(terms[1]))


# ------------------------------------------------------------------------------------------------ wm_add_bf16
@pytest.mark.gpu
@pytest.mark.parametrize("n", [8, 8 * (2 ** 20 + 3)])
def test_add_bf16(lib, n):
    """An IEEE float32 add of two bf16 values followed by one rounding is deterministic: equality.  The second size is three
    16-byte items past the grid cap of 2^20 threads."""
    assert n == 8 or n // 8 > kc.BN_STREAM_BLOCKS * kc.BN_THREADS
    gen = torch.Generator().manual_seed(n)
    a, b = torch.randn(n, generator=gen).bfloat16(), (torch.randn(n, generator=gen) * 3).bfloat16()
    out = Guarded((n,), torch.bfloat16)
    ad, bd = a.to(DEV), b.to(DEV)
    ok(lib, lib.wm_add_bf16(ad.data_ptr(), bd.data_ptr(), n, out.ptr, stream()), "wm_add_bf16")
    finish("wm_add_bf16")
    assert torch.equal(out.t.cpu(), (a.float() + b.float()).bfloat16())
