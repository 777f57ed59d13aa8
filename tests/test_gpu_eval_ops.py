"""GPU checks of the evaluation kernels (csrc/evalops.hip, WM_ACT_MISH in csrc/transformer.hip): multi-label AUROC against
sklearn, Mish against torch in float64, dropout's mask statistics and determinism, and one training step of the two-layer
probe against a float64 torch replica."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F
from sklearn.metrics import roc_auc_score

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16_REL = 2.0 ** -8   # 2x the bf16 rounding level (half an ulp is 2^-9 relative)


def _sk_auc(s, y):
    """Per-label sklearn AUC of float64 scores / 0-1 targets [rows, L]; 0 for a single-class label."""
    out = []
    for l in range(y.shape[1]):
        yl = y[:, l]
        out.append(roc_auc_score(yl, s[:, l]) if 0 < yl.sum() < len(yl) else 0.0)
    return np.array(out)


def _targets(rows, L, g):
    y = (torch.rand(rows, L, generator=g) < torch.linspace(0.05, 0.6, L)).to(torch.int8)
    return y


@pytest.mark.parametrize("rows", [1, 97, 5703, 26609])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("tied", [False, True])
def test_auroc_equals_sklearn_on_probabilities(rows, dtype, tied):
    from ssl_wafermap_amd.evalops import multilabel_auroc_per_label

    g = torch.Generator().manual_seed(rows + 7 * tied)
    L = 8
    if tied:   # a few levels: most pairs tie
        s = torch.randint(0, 5, (rows, L), generator=g).float() / 4
    else:      # float32 sigmoid of logits, the values the probes' AUROC ranks
        s = torch.sigmoid(2 * torch.randn(rows, L, generator=g))
    s = s.to(dtype)
    y = _targets(rows, L, g)
    if rows == 1:   # every label is single-class
        with pytest.warns(UserWarning, match="one class"):
            auc, npos = multilabel_auroc_per_label(s.to(DEV), y.to(DEV))
    else:
        auc, npos = multilabel_auroc_per_label(s.to(DEV), y.to(DEV), warn=False)
    ref = _sk_auc(s.double().numpy(), y.numpy())
    assert auc.dtype == torch.float64 and auc.shape == (L,)
    assert torch.equal(npos, y.long().sum(0))
    assert np.abs(auc.numpy() - ref).max() <= 1e-12, (auc.numpy(), ref)


def test_auroc_single_class_labels_are_zero_and_in_the_macro_mean():
    from ssl_wafermap_amd.models import multilabel_auroc

    g = torch.Generator().manual_seed(5)
    s = torch.rand(200, 4, generator=g)
    y = _targets(200, 4, g)
    y[:, 1] = 0   # no positives
    y[:, 2] = 1   # no negatives
    with pytest.warns(UserWarning, match="one class"):
        per = multilabel_auroc(s.to(DEV), y.to(DEV), average=None)
    assert per[1] == 0.0 and per[2] == 0.0
    ref = _sk_auc(s.double().numpy(), y.numpy())
    assert np.abs(per.numpy() - ref).max() <= 1e-12
    with pytest.warns(UserWarning):
        macro = multilabel_auroc(s.to(DEV), y.to(DEV))
    assert macro == pytest.approx(ref.mean(), abs=1e-12)


def test_auroc_two_calls_give_the_same_bits():
    from ssl_wafermap_amd.evalops import multilabel_auroc_per_label

    g = torch.Generator().manual_seed(11)
    s = torch.randn(26609, 8, generator=g).to(torch.bfloat16).to(DEV)
    y = _targets(26609, 8, g).to(DEV)
    a, _ = multilabel_auroc_per_label(s, y)
    b, _ = multilabel_auroc_per_label(s, y)
    assert torch.equal(a, b)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_auroc_of_logits_ranks_the_sigmoid(dtype):
    from ssl_wafermap_amd.evalops import multilabel_auroc_per_label

    g = torch.Generator().manual_seed(3)
    z = (6 * torch.randn(5703, 8, generator=g)).to(dtype)   # many saturate to 1.0f after the sigmoid: ties there
    z[:40, 0] = 30.0
    y = _targets(5703, 8, g)
    auc, _ = multilabel_auroc_per_label(z.to(DEV), y.to(DEV))
    # torch's float32 sigmoid on the device, where torchmetrics computes it in the reference's runs (the CPU sigmoid rounds
    # differently in the last bit, and near 1.0f a bit decides a tie)
    ref = _sk_auc(torch.sigmoid(z.float().to(DEV)).cpu().double().numpy(), y.numpy())
    assert np.abs(auc.numpy() - ref).max() <= 1e-6


# ------------------------------------------------------------------------------------ Mish
def _mish64(v):
    return v * torch.tanh(F.softplus(v, threshold=20))


def test_mish_forward_and_backward_match_torch_float64():
    from ssl_wafermap_amd import nn as hnn
    from ssl_wafermap_amd import vit_ops

    g = torch.Generator().manual_seed(0)
    rows, C = 1000, 256
    x = (4 * torch.randn(rows, C, generator=g)).to(torch.bfloat16)
    x[0, :16] = torch.tensor([25.0, 20.5, 19.5, -25.0, 0.0, -0.5, 1e-3, -30.0, 50.0, -5.0, 3.0, 8.0, -1.2, 0.7, 21.0, -19.0])
    bias = (0.5 * torch.randn(C, generator=g)).float()
    dy = torch.randn(rows, C, generator=g).to(torch.bfloat16)

    xd = x.to(DEV).requires_grad_(True)
    bd = bias.to(DEV).requires_grad_(True)
    y = vit_ops.bias_act(xd, bd, vit_ops.ACT_MISH)
    y.backward(dy.to(DEV))

    v = (x.double() + bias.double()).requires_grad_(True)
    ref = _mish64(v)
    ref.backward(dy.double())
    err_y = (y.detach().cpu().double() - ref.detach()).abs()
    assert (err_y <= BF16_REL * ref.detach().abs() + 1e-30).all(), float((err_y / ref.detach().abs().clamp_min(1e-30)).max())
    dx_ref = v.grad
    err_dx = (xd.grad.cpu().double() - dx_ref).abs()
    # (plus the float32 cancellation in mish'(v) near its zero at v = -1.19, times |dy|)
    assert (err_dx <= BF16_REL * dx_ref.abs() + 1e-6 * dy.double().abs()).all()
    # the bias gradient is the column sum of the bf16-rounded dx
    db_ref = dx_ref.sum(0)
    assert ((bd.grad.cpu().double() - db_ref).abs() <= BF16_REL * dx_ref.abs().sum(0) + 1e-6).all()

    # the module: Mish without a bias
    xm = x.to(DEV).requires_grad_(True)
    ym = hnn.Mish()(xm)
    ym.backward(dy.to(DEV))
    vm = x.double().requires_grad_(True)
    rm = _mish64(vm)
    rm.backward(dy.double())
    assert ((ym.detach().cpu().double() - rm.detach()).abs() <= BF16_REL * rm.detach().abs() + 1e-30).all()
    assert ((xm.grad.cpu().double() - vm.grad).abs() <= BF16_REL * vm.grad.abs() + 1e-6 * dy.double().abs()).all()


# ------------------------------------------------------------------------------------ dropout
def test_dropout_eval_and_p0_are_the_identity():
    from ssl_wafermap_amd import nn as hnn

    x = torch.randn(64, 256, device=DEV).to(torch.bfloat16)
    assert hnn.Dropout(0.5).eval()(x) is x
    assert hnn.Dropout(0.0).train()(x) is x


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("p", [0.1, 0.5, 0.9])
def test_dropout_mask_statistics_values_and_gradient(dtype, p):
    from oracle.augment import rand01
    from ssl_wafermap_amd.evalops import dropout

    n = 1 << 22
    x = (torch.randn(n, device=DEV) + 4.0).to(dtype)   # no zeros: kept <=> non-zero output
    xr = x.clone().requires_grad_(True)
    y = dropout(xr, p, 1234)
    kept = y != 0
    frac = float(kept.double().mean())
    sigma = (p * (1 - p) / n) ** 0.5
    assert abs(frac - (1 - p)) <= 4 * sigma, (frac, 1 - p)
    # the counter RNG of the augmentation kernel: rand01(seed, i) >= p
    assert torch.equal(kept.cpu(), torch.from_numpy(rand01(1234, n) >= np.float32(p)))
    scale = np.float32(1.0) / np.float32(1.0 - np.float32(p))
    want = (x[kept].float() * float(scale)).to(dtype)
    assert torch.equal(y[kept], want)
    assert torch.allclose(y[kept].double(), x[kept].double() / (1 - p), rtol=2.0 ** -7 if dtype == torch.bfloat16 else 1e-6)
    y.backward(torch.ones_like(y))
    assert torch.equal(xr.grad != 0, kept)
    assert torch.equal(xr.grad[kept], torch.full_like(xr.grad[kept], float(scale)).to(dtype))


def test_dropout_p1_gives_zeros_and_seeds_control_the_mask():
    from ssl_wafermap_amd import nn as hnn
    from ssl_wafermap_amd.evalops import dropout

    x = torch.randn(1000, 256, device=DEV).to(torch.bfloat16)
    assert not dropout(x, 1.0, 9).any()
    a, b, c = dropout(x, 0.5, 7), dropout(x, 0.5, 7), dropout(x, 0.5, 8)
    assert torch.equal(a, b)
    assert not torch.equal(a != 0, c != 0)

    d = hnn.Dropout(0.5).train()
    torch.manual_seed(42)
    y1 = d(x)
    s1 = d.last_seed
    y2 = d(x)
    assert d.last_seed != s1 and not torch.equal(y1, y2)   # a new seed per forward pass
    torch.manual_seed(42)
    assert torch.equal(d(x), y1) and d.last_seed == s1


# ------------------------------------------------------------------------------------ two-layer probe
def test_two_layer_probe_step_matches_float64_replica():
    from oracle.augment import rand01
    from ssl_wafermap_amd.models import TwoLayerMultilabelClassifier

    torch.manual_seed(0)
    B, Fdim, C = 300, 64, 8
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, Fdim, generator=g)
    y = (torch.rand(B, C, generator=g) < 0.3).long()
    pw = (1 - y.float().mean(0)) / y.float().mean(0)
    model = TwoLayerMultilabelClassifier(Fdim, C, pos_weight=pw).to(DEV).train()
    params = {k: p.detach().cpu().clone() for k, p in model.named_parameters()}
    logits = model(x.to(DEV))
    loss = model.criterion(logits, y.to(DEV).float())
    loss.backward()
    seed = model.model[2].last_seed
    mask = torch.from_numpy(rand01(seed, B * 256) >= np.float32(0.5)).view(B, 256).double()

    # replica: the kernel's bf16 operands (features and weights), everything else float64
    P = {k: (v.to(torch.bfloat16).double() if k.endswith("weight") else v.double()).requires_grad_(True)
         for k, v in params.items()}
    h = x.to(torch.bfloat16).double() @ P["model.0.weight"].T + P["model.0.bias"]
    a = _mish64(h) * mask * 2.0
    z = a @ P["model.3.weight"].T + P["model.3.bias"]
    ref = F.binary_cross_entropy_with_logits(z, y.double(), pos_weight=pw.double())
    ref.backward()
    assert abs(float(loss) - float(ref)) <= 1e-2 * abs(float(ref))
    for k, p in model.named_parameters():
        gr = P[k].grad
        rel = float((p.grad.cpu().double() - gr).norm() / gr.norm())
        assert rel <= 3e-2, (k, rel)
