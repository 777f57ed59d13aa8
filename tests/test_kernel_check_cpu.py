"""The criteria of tests/kernel_check.py have teeth: proved on the CPU, without a kernel.

For every input family the GPU tests use, `check` is fed
  (a) an honest result: the emulation with every value moved by a few float32 ulp before each bf16 rounding
      (kernel_check.jitter), so its rounding events are independent of the yardstick's -- it must pass;
  (b) deliberately wrong computations, each of which the single criterion max |err| <= rel * max |ref| of
      tests/test_gpu_vit.py::_close accepts on unit-scale randn inputs -- each must fail at least one criterion.
A seeded error that passed would mean the inputs are too tame; the remedy is other inputs, never a wider bound."""
import kernel_check as kc
import pytest
import torch


def _reject(got, ref, emul, what):
    rows, finite = kc.verdict(got, ref, emul)
    line = ", ".join(f"{c}: {m:.3g} vs {b:.3g}" for c, m, b in rows)
    print(f"{what}: {line}")
    assert not finite or any(m > b for _, m, b in rows), f"seeded error accepted -- {what}: {line}"


def _accept(got, ref, emul, what):
    rows, finite = kc.verdict(got, ref, emul)
    line = ", ".join(f"{c}: {m:.3g} vs {b:.3g}" for c, m, b in rows)
    print(f"{what}: {line}")
    assert finite and all(m <= b for _, m, b in rows), f"honest result rejected -- {what}: {line}"


# ---------------------------------------------------------------------------------------------------- attention
ATT_SHAPES = [(2, 37, 2, 64), (1, 197, 2, 64), (1, 250, 2, 32)]


@pytest.mark.parametrize("family", kc.ATTENTION_FAMILIES)
@pytest.mark.parametrize("b,s,h,hd", ATT_SHAPES)
def test_attention_honest_result_passes(family, b, s, h, hd):
    scale = hd ** -0.5
    qkv, do = kc.attention_inputs(family, b, s, h, hd, seed=s)
    ref = kc.attention_ref(qkv, scale, do)
    emul = kc.attention_ref(qkv, scale, do, emulate=True)
    with kc.jitter(1):
        got = kc.attention_ref(qkv, scale, do, emulate=True)
    _accept(got[0], ref[0], emul[0], f"out {family} S={s}")
    _accept(got[2], ref[2], emul[2], f"dqkv {family} S={s}")
    _accept(kc.attention_lse_f32(qkv, scale) * (1 + 2.0 ** -24), ref[1], kc.attention_lse_f32(qkv, scale), f"lse {family} S={s}")


@pytest.mark.parametrize("family", kc.ATTENTION_FAMILIES)
@pytest.mark.parametrize("b,s,h,hd", ATT_SHAPES)
@pytest.mark.parametrize("error,tensor", [("noscale", 0), ("nodelta", 2), ("bwd_noscale", 2), ("lse_m", 1)])
def test_attention_seeded_errors_fail(family, b, s, h, hd, error, tensor):
    scale = hd ** -0.5
    qkv, do = kc.attention_inputs(family, b, s, h, hd, seed=s)
    ref = kc.attention_ref(qkv, scale, do)
    emul = kc.attention_ref(qkv, scale, do, emulate=True)
    bad = kc.attention_ref(qkv, scale, do, emulate=True, seed_error=error)
    yard = kc.attention_lse_f32(qkv, scale) if tensor == 1 else emul[tensor]
    _reject(bad[tensor], ref[tensor], yard, f"{error} {family} S={s}")


@pytest.mark.parametrize("family", ["randn", "zero_query", "v_offset", "offset-80"])
def test_attention_unmasked_padding_fails(family):
    """S = 250 in a 256-slot tile: the six padded key slots (logit 0, value 0) join the softmax.  On unit randn the old
    criterion scores 0.0121 against its bound 0.015.  (With logits near +80 or of spread 16 a logit-0 slot carries no
    weight a bf16 result could show: those families cannot see this error and are not asked to.)"""
    b, s, h, hd = 1, 250, 2, 64
    scale = hd ** -0.5
    qkv, do = kc.attention_inputs(family, b, s, h, hd, seed=s)
    ref = kc.attention_ref(qkv, scale)
    emul = kc.attention_ref(qkv, scale, emulate=True)
    bad = kc.attention_ref(qkv, scale, emulate=True, seed_error="pad6")
    if family == "randn":
        old = float((bad[0] - ref[0]).abs().max() / ref[0].abs().max())
        assert old <= 1.5e-2, old  # the criterion this pull request replaces accepted it
    _reject(bad[0], ref[0], emul[0], f"pad6 {family}")


# ---------------------------------------------------------------------------------------------------- LayerNorm
LN_SHAPES = [(130, 768), (37, 192)]


@pytest.mark.parametrize("family", kc.LN_FAMILIES)
@pytest.mark.parametrize("rows,c", LN_SHAPES)
@pytest.mark.parametrize("eps", [1e-6, 1e-5])
def test_layer_norm_honest_result_passes(family, rows, c, eps):
    x, gamma, beta, dy, dres = kc.layer_norm_inputs(family, rows, c, seed=rows)
    for skip in (None, dres):
        ref = kc.layer_norm_ref(x, gamma, beta, eps, dy, skip)
        emul = kc.layer_norm_ref(x, gamma, beta, eps, dy, skip, emulate=True)
        with kc.jitter(2):
            got = kc.layer_norm_ref(x, gamma, beta, eps, dy, skip, emulate=True)
        _accept(got[0], ref[0], emul[0], f"y {family}")
        _accept(got[1], ref[1], emul[1], f"dx {family}")
    dg, db = kc.layer_norm_param_grads_f32(x, dy, eps)
    _accept(dg * (1 + 2.0 ** -24), ref[2], dg, f"dgamma {family}")
    _accept(db * (1 + 2.0 ** -24), ref[3], db, f"dbeta {family}")
    if family == "constant":
        assert torch.equal(emul[0], kc.bf(beta.double()).expand(rows, c))


@pytest.mark.parametrize("family", ["randn", "tight", "mean300", "big_row"])
@pytest.mark.parametrize("rows,c", LN_SHAPES)
def test_layer_norm_statistics_without_the_last_piece_fail(family, rows, c):
    """The last 8 columns left out of mean and variance: 0.0065 on the old criterion at 130 x 768 (bound 0.01)."""
    x, gamma, beta, dy, _ = kc.layer_norm_inputs(family, rows, c, seed=rows)
    ref = kc.layer_norm_ref(x, gamma, beta, 1e-6, dy)
    emul = kc.layer_norm_ref(x, gamma, beta, 1e-6, dy, emulate=True)
    bad = kc.layer_norm_ref(x, gamma, beta, 1e-6, dy, emulate=True, seed_error="last8")
    if family == "randn" and c == 768:
        assert float((bad[0] - ref[0]).abs().max() / ref[0].abs().max()) <= 1e-2
    _reject(bad[0], ref[0], emul[0], f"last8 y {family} {rows}x{c}")


@pytest.mark.parametrize("rows,c", LN_SHAPES)
@pytest.mark.parametrize("eps,error", [(1e-6, "eps0"), (1e-6, "eps1e-5"), (1e-6, "eps1e-3"), (1e-5, "eps0"), (1e-5, "eps1e-3")])
def test_layer_norm_wrong_eps_fails_on_tight_rows(rows, c, eps, error):
    """eps is invisible on unit-scale rows (1e-7 .. 1e-4 on the old criterion, bound 0.01); on rows of spread ~1e-3 it
    decides the result.  Both eps values the GPU tests pass are covered, so a hard-coded one shows."""
    x, gamma, beta, dy, _ = kc.layer_norm_inputs("tight", rows, c, seed=rows)
    ref = kc.layer_norm_ref(x, gamma, beta, eps, dy)
    emul = kc.layer_norm_ref(x, gamma, beta, eps, dy, emulate=True)
    bad = kc.layer_norm_ref(x, gamma, beta, eps, dy, emulate=True, seed_error=error)
    _reject(bad[0], ref[0], emul[0], f"{error} (asked {eps:g}) y")
    _reject(bad[1], ref[1], emul[1], f"{error} (asked {eps:g}) dx")
    xr, gr, br, dyr, _ = kc.layer_norm_inputs("randn", rows, c, seed=rows)
    r2 = kc.layer_norm_ref(xr, gr, br, eps, dyr)
    b2 = kc.layer_norm_ref(xr, gr, br, eps, dyr, emulate=True, seed_error=error)
    assert float((b2[0] - r2[0]).abs().max() / r2[0].abs().max()) <= 1e-2  # the old inputs and criterion accepted it


@pytest.mark.parametrize("family", ["randn", "tight", "mean300", "big_row"])
@pytest.mark.parametrize("rows,c", LN_SHAPES)
def test_layer_norm_dx_without_mean_of_dy_fails(family, rows, c):
    x, gamma, beta, dy, dres = kc.layer_norm_inputs(family, rows, c, seed=rows)
    dy = kc.bf(dy + 3.0)   # (the GPU tests' gradient for the parameter sums: column mean not zero)
    ref = kc.layer_norm_ref(x, gamma, beta, 1e-6, dy)
    emul = kc.layer_norm_ref(x, gamma, beta, 1e-6, dy, emulate=True)
    bad = kc.layer_norm_ref(x, gamma, beta, 1e-6, dy, emulate=True, seed_error="no_mean_dy")
    _reject(bad[1], ref[1], emul[1], f"no_mean_dy {family}")


# ---------------------------------------------------------------------------------------------------- bias / act
@pytest.mark.parametrize("act", [0, 1, 2, 3])
@pytest.mark.parametrize("res", [False, True])
def test_bias_act_honest_result_passes_and_short_dbias_fails(act, res):
    rows, c = 264, 64
    g = torch.Generator().manual_seed(act)
    x = kc.act_grid(rows, c, seed=act)
    bias = torch.randn(c, generator=g) * 0.3
    r = kc.bf(torch.randn(rows, c, generator=g)) if res else None
    dy = kc.bf(torch.randn(rows, c, generator=g) + 3.0)
    ref = kc.bias_act_ref(x, bias, act, r, dy)
    emul = kc.bias_act_ref(x, bias, act, r, dy, emulate=True)
    with kc.jitter(3):
        got = kc.bias_act_ref(x, bias, act, r, dy, emulate=True)
    _accept(got[0], ref[0], emul[0], f"y act={act}")
    _accept(got[1], ref[1], emul[1], f"dx act={act}")
    yard = kc.colsum_f32(emul[1])
    _accept(yard * (1 + 2.0 ** -24), emul[2], yard, f"dbias act={act}")
    bad = kc.bias_act_ref(x, bias, act, r, dy, emulate=True, seed_error="rows-1")
    _reject(bad[2], emul[2], yard, f"dbias over rows-1 rows, act={act}")
    if act == 2:  # ReLU gradient at exactly 0 is 0, as torch
        z = torch.zeros(8, 8)
        assert torch.equal(kc.bias_act_ref(z, None, 2, None, torch.ones(8, 8))[1], torch.zeros(8, 8, dtype=torch.float64))


def test_gelu_and_mish_match_torch_float64():
    v = torch.linspace(-12, 12, 4001, dtype=torch.float64).requires_grad_(True)
    for act, fn in ((1, torch.nn.functional.gelu), (3, torch.nn.functional.mish)):
        y = fn(v)
        (gr,) = torch.autograd.grad(y.sum(), v)
        torch.testing.assert_close(kc._act64(v.detach(), act), y.detach(), rtol=1e-12, atol=1e-14)   # (torch's own 1 + erf cancels in the tail)
        torch.testing.assert_close(kc._act_grad64(v.detach(), act), gr, rtol=1e-10, atol=1e-14)


# ---------------------------------------------------------------------------------------------------- references
def test_float64_references_match_autograd():
    """The closed-form float64 gradients the GPU tests compare with are what autograd gives."""
    qkv, do = kc.attention_inputs("randn", 2, 19, 2, 32, seed=0)
    x = qkv.double().requires_grad_(True)
    q, k, v = (x[:, :, j].transpose(1, 2) for j in range(3))
    out = (((q @ k.transpose(-2, -1)) * 0.3).softmax(-1) @ v).transpose(1, 2)
    out.backward(do.double())
    ref = kc.attention_ref(qkv, 0.3, do)
    torch.testing.assert_close(ref[0], out.detach(), rtol=1e-12, atol=1e-14)
    torch.testing.assert_close(ref[2], x.grad, rtol=1e-11, atol=1e-13)
    torch.testing.assert_close(ref[1], torch.logsumexp((q @ k.transpose(-2, -1)) * 0.3, -1).detach(), rtol=1e-12, atol=1e-14)
    xl, gamma, beta, dy, dres = kc.layer_norm_inputs("randn", 9, 24, seed=1)
    t = [u.double().requires_grad_(True) for u in (xl, gamma, beta)]
    y = torch.nn.functional.layer_norm(t[0], (24,), t[1], t[2], 1e-5)
    (y * dy.double()).sum().backward()
    r = kc.layer_norm_ref(xl, gamma, beta, 1e-5, dy, dres)
    torch.testing.assert_close(r[0], y.detach(), rtol=1e-12, atol=1e-14)
    torch.testing.assert_close(r[1], t[0].grad + dres.double(), rtol=1e-10, atol=1e-12)
    torch.testing.assert_close(r[2], t[1].grad, rtol=1e-10, atol=1e-12)
    torch.testing.assert_close(r[3], t[2].grad, rtol=1e-10, atol=1e-12)
    g = torch.Generator().manual_seed(2)
    xm, res, dym = (kc.bf(torch.randn(11, 16, generator=g)) for _ in range(3))
    w1, w2 = kc.bf(torch.randn(32, 16, generator=g) * 0.3), kc.bf(torch.randn(16, 32, generator=g) * 0.3)
    b1, b2 = torch.randn(32, generator=g) * 0.1, torch.randn(16, generator=g) * 0.1
    tt = [u.double().requires_grad_(True) for u in (xm, w1, b1, w2, b2)]
    F = torch.nn.functional
    ym = F.linear(F.gelu(F.linear(tt[0], tt[1], tt[2])), tt[3], tt[4]) + res.double()
    ym.backward(dym.double())
    rm = kc.mlp_ref(xm, w1, b1, w2, b2, res, dym)
    torch.testing.assert_close(rm["y"], ym.detach(), rtol=1e-12, atol=1e-14)
    for name, u in zip(("dx", "dw1", "db1", "dw2", "db2"), tt):
        torch.testing.assert_close(rm[name], u.grad, rtol=1e-10, atol=1e-12)
