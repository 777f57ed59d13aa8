"""GPU checks of the model-inspection kernels (csrc/interpret.hip) and their Python layer (interpret.py,
VisionTransformer.get_last_selfattention / get_intermediate_layers): attention probabilities, dino's attention-mass
mask and EigenCAM, each against a float64 restatement kept in this file, then end to end on golden wafers, and the
figure script.  Bounds are about 2x the error measured on an MI355X; the measured value is stated next to each."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = Path(__file__).resolve().parent.parent
FIXTURE = ROOT / "tests/golden/wm811k_train_1_split.npz"


def _measure(name, value):
    print(f"MEASURE {name} {value:.3e}")


# ------------------------------------------------------------------------------------------ float64 restatements
def probs_ref(qkv, b, s, h, scale):
    """softmax(scale q k^T) in float64 of qkv [b*s, 3*h*hd] -> [b, h, s, s]."""
    hd = qkv.shape[1] // (3 * h)
    t = qkv.double().reshape(b, s, 3, h, hd).permute(2, 0, 3, 1, 4)
    return torch.softmax((t[0] @ t[1].transpose(-1, -2)) * scale, dim=-1)


def mass_mask_ref(a, t):
    """visualize_attention.py: stable ascending sort, normalised cumsum, > 1 - t, scattered back.  a [rows, n] float64
    -> (mask bool, cum float64), both in the original order."""
    val, idx = torch.sort(a, dim=-1, stable=True)
    cum_sorted = torch.cumsum(val / val.sum(-1, keepdim=True), dim=-1)
    cum = torch.empty_like(cum_sorted).scatter_(-1, idx, cum_sorted)
    return cum > (1 - t), cum


def eigencam_ref(act, size):
    """pytorch_grad_cam get_2d_projection + BaseCAM + scale_cam_image in float64 (numpy SVD), with this project's sign
    rule, torch bilinear resize.  act float64 [N, C, H, W] (NaN allowed) -> ([N, size, size], leading eigengap
    lambda1 / lambda2 per image)."""
    a = np.nan_to_num(act.detach().cpu().double().numpy(), nan=0.0)
    n, c, h, w = a.shape
    maps, gaps = [], []
    for x in a:
        flat = x.reshape(c, h * w)
        A = flat.T - flat.T.mean(axis=0)
        _, sv, vt = np.linalg.svd(A, full_matrices=False)
        gaps.append(sv[0] ** 2 / max(sv[1] ** 2, 1e-300) if len(sv) > 1 else np.inf)
        if sv[0] == 0:
            maps.append(np.zeros((size, size)))
            continue
        p = A @ vt[0]
        if p @ flat.sum(axis=0) < 0:
            p = -p
        p = np.maximum(p, 0).reshape(h, w)
        p = p - p.min()
        p = p / (1e-7 + p.max())
        r = F.interpolate(torch.from_numpy(p)[None, None], size=(size, size), mode="bilinear",
                          align_corners=False)[0, 0].numpy()
        r = r - r.min()
        maps.append(r / (1e-7 + r.max()))
    return torch.from_numpy(np.stack(maps)), np.array(gaps)


def vit_last_attn_ref(vit, images):
    """float64 restatement from oracle.vit pieces on the model's weights: blocks[:-1], last norm1 + qkv, softmax."""
    from oracle import vit as ovit

    sd = {k: v.detach().double() for k, v in vit.state_dict().items()}
    x = images.double()
    p = vit.patch_embed.patch_size
    heads = vit.blocks[0].attn.num_heads
    t = F.conv2d(x, sd["patch_embed.proj.weight"], sd["patch_embed.proj.bias"], stride=p).flatten(2).transpose(1, 2)
    n = t.shape[0]
    t = torch.cat([sd["cls_token"].expand(n, -1, -1), t], dim=1) + ovit.pos_embed_for(sd["pos_embed"], x.shape[-1] // p)
    last = len(vit.blocks) - 1
    for i in range(last):
        t = ovit.block(t, sd, f"blocks.{i}", heads)
    c = t.shape[-1]
    hn = F.layer_norm(t, (c,), sd[f"blocks.{last}.norm1.weight"], sd[f"blocks.{last}.norm1.bias"], 1e-6)
    qkv = F.linear(hn, sd[f"blocks.{last}.attn.qkv.weight"], sd[f"blocks.{last}.attn.qkv.bias"])
    return probs_ref(qkv.reshape(n * t.shape[1], -1), n, t.shape[1], heads, (c // heads) ** -0.5)


def vit_layers_ref(vit, images, n_last):
    from oracle import vit as ovit

    sd = {k: v.detach().double() for k, v in vit.state_dict().items()}
    x = images.double()
    p = vit.patch_embed.patch_size
    heads = vit.blocks[0].attn.num_heads
    t = F.conv2d(x, sd["patch_embed.proj.weight"], sd["patch_embed.proj.bias"], stride=p).flatten(2).transpose(1, 2)
    t = torch.cat([sd["cls_token"].expand(t.shape[0], -1, -1), t], dim=1) + ovit.pos_embed_for(sd["pos_embed"],
                                                                                                x.shape[-1] // p)
    out = []
    for i in range(len(vit.blocks)):
        t = ovit.block(t, sd, f"blocks.{i}", heads)
        if len(vit.blocks) - i <= n_last:
            out.append(F.layer_norm(t, (t.shape[-1],), sd["norm.weight"], sd["norm.bias"], 1e-6))
    return out


# ------------------------------------------------------------------------------------------ inputs
def golden_images(n, size, start=0):
    """Inference images (resize, grey, normalise) of golden wafers start..start+n-1: bf16 channels_last."""
    from ssl_wafermap_amd.data import WaferStore
    from ssl_wafermap_amd.transforms import augment_views, get_inference_transforms, sample_view_params

    store, labels = WaferStore.load(FIXTURE)
    sub = WaferStore([store.wafer(i) for i in range(start, start + n)], device=DEV)
    params = sample_view_params(get_inference_transforms((size, size)), np.arange(n), sub.heights_np, sub.widths_np,
                                np.random.default_rng(0))
    return augment_views(sub, params, img_size=size, out_size=size, fmt="nhwc_bf16")


def make_vit(kind, seed=0, qk_gain=5.0):
    """Randomly initialised ViT whose qkv weights are scaled up so that the attention rows are peaked (dino's init gives
    nearly uniform rows at random weights, where argmax comparisons mean nothing)."""
    from ssl_wafermap_amd.models import vit_small, vit_tiny

    torch.manual_seed(seed)
    vit = (vit_small if kind == "small" else vit_tiny)(patch_size=16).to(DEV).eval()
    with torch.no_grad():
        for blk in vit.blocks:
            blk.attn.qkv.weight.mul_(qk_gain)
    return vit


def make_resnet(seed=0):
    from ssl_wafermap_amd.models import ResNet18

    torch.manual_seed(seed)
    return ResNet18().to(DEV).eval()


def rand_qkv(b, s, h, hd, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(b * s, 3 * h * hd, generator=g) * 1.5).to(dtype).to(DEV)


# ------------------------------------------------------------------------------------------ 1. attention kernel
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("hd", [64, 32])
@pytest.mark.parametrize("s", [1, 37, 197, 256])
@pytest.mark.parametrize("b", [1, 8, 64])
def test_attention_probs_against_float64(b, s, hd, dtype):
    from ssl_wafermap_amd.interpret import attention_probs

    h = 6 if hd == 64 else 4
    scale = hd ** -0.5
    qkv = rand_qkv(b, s, h, hd, dtype, seed=b * 1000 + s + hd)
    p = attention_probs(qkv, b, s, h, scale)
    assert p.shape == (b, h, s, s) and p.dtype == torch.float32
    ref = probs_ref(qkv, b, s, h, scale)
    err = (p.double() - ref).abs().max().item()
    _measure(f"probs_abs_err[{dtype},hd{hd},S{s},B{b}]", err)
    assert err <= 2.5e-6, err   # measured <= 1.2e-6 (both dtypes)
    rs = (p.double().sum(-1) - 1).abs().max().item()
    assert rs <= 1e-5, rs
    cls = attention_probs(qkv, b, s, h, scale, cls_only=True)
    assert cls.shape == (b, h, 1, s)
    assert torch.equal(cls[:, :, 0], p[:, :, 0])


@pytest.mark.parametrize("hd", [64, 32])
@pytest.mark.parametrize("s", [37, 197])
def test_attention_probs_times_v_matches_forward_kernel(s, hd):
    """P V in float64 against vit_ops.attention on the same qkv: the forward kernel multiplies bf16-rounded
    unnormalised probabilities with V and stores bf16, so the two differ by bf16 rounding."""
    from ssl_wafermap_amd import precision, vit_ops
    from ssl_wafermap_amd.interpret import attention_probs

    b, h = 8, 6 if hd == 64 else 4
    scale = hd ** -0.5
    for dtype in (torch.bfloat16, torch.float32):
        qkv = rand_qkv(b, s, h, hd, dtype, seed=s + hd)
        p = attention_probs(qkv, b, s, h, scale).double()
        v = qkv.double().reshape(b, s, 3, h, hd)[:, :, 2].permute(0, 2, 1, 3)
        pv = (p @ v).permute(0, 2, 1, 3).reshape(b * s, h * hd)
        with torch.no_grad(), precision.precision("bf16" if dtype == torch.bfloat16 else "float32"):
            out = vit_ops.attention(qkv, b, s, h, scale, head_dim=hd).double()
        mag = ((p.abs() @ v.abs()).permute(0, 2, 1, 3).reshape(b * s, h * hd))
        rel = ((out - pv).abs() / (mag + 1e-30)).max().item()
        _measure(f"pv_vs_forward[{dtype},hd{hd},S{s}]", rel)
        # bf16: output rounding 2^-9 plus the forward's bf16 probabilities 2^-9; measured <= 5.0e-3
        # float32 preset: measured <= 1.7e-6
        assert rel <= (1e-2 if dtype == torch.bfloat16 else 3.5e-6), rel


# ------------------------------------------------------------------------------------------ 2. get_last_selfattention
@pytest.mark.parametrize("kind", ["tiny", "small"])
@pytest.mark.parametrize("size", [224, 96])
def test_get_last_selfattention_against_float64(kind, size):
    from ssl_wafermap_amd import precision

    vit = make_vit(kind)
    x = golden_images(8, size)
    ref = vit_last_attn_ref(vit, x)
    with precision.precision("float32"):
        p32 = vit.get_last_selfattention(x)
    heads = vit.blocks[0].attn.num_heads
    t = (size // 16) ** 2 + 1
    assert p32.shape == (8, heads, t, t) and p32.dtype == torch.float32
    e32 = (p32.double() - ref).abs().max().item()
    _measure(f"last_attn_f32[{kind},{size}]", e32)
    assert e32 <= (1.2e-4 if kind == "small" else 5e-6), e32   # measured: small <= 5.8e-5, tiny <= 2.4e-6
    p16 = vit.get_last_selfattention(x)
    e16 = (p16.double() - ref).abs().max().item()
    _measure(f"last_attn_bf16[{kind},{size}]", e16)
    # bf16 activations through 11 blocks of peaked attention (absolute error of a probability): measured small <= 0.38,
    # tiny <= 0.028
    assert e16 <= (0.75 if kind == "small" else 0.06), e16
    # per-head argmax of the class-token row: equal wherever the oracle's top two patches are further apart than the
    # bf16 error seen on this input
    r = ref[:, :, 0, 1:]
    top2 = r.topk(2, dim=-1)
    clear = (top2.values[..., 0] - top2.values[..., 1]) > e16
    agree = p16[:, :, 0, 1:].argmax(-1) == r.argmax(-1)
    _measure(f"last_attn_argmax_clear_fraction[{kind},{size}]", clear.float().mean().item())
    assert bool(agree[clear].all())
    assert bool(clear.float().mean() >= 0.15)   # measured >= 0.21 of the (image, head) rows


# ------------------------------------------------------------------------------------------ 3. get_intermediate_layers
@pytest.mark.parametrize("prec", ["bf16", "float32"])
def test_get_intermediate_layers(prec):
    from ssl_wafermap_amd import precision

    vit = make_vit("small", qk_gain=1.0)
    x = golden_images(4, 224)
    with torch.no_grad(), precision.precision(prec):
        last = vit.get_intermediate_layers(x, 1)
        feat = vit(x)
        four = vit.get_intermediate_layers(x, 4)
    assert len(last) == 1 and last[0].shape == (4, 197, 384)
    # LayerNorm is one row per wave, independent of the row count: the class rows of the whole-token norm are the
    # forward's bits
    assert torch.equal(last[0][:, 0], feat.reshape(4, 384))
    ref = vit_layers_ref(vit, x, 4)
    assert len(four) == 4
    for i, (got, want) in enumerate(zip(four, ref)):
        rel = ((got.double() - want).abs().max() / want.abs().max()).item()
        _measure(f"intermediate_{prec}[{i}]", rel)
        assert rel <= (5e-2 if prec == "bf16" else 3e-6), rel   # measured bf16 <= 2.1e-2, float32 <= 1.5e-6
    assert torch.equal(four[-1], last[0])


# ------------------------------------------------------------------------------------------ 4. mass mask
@pytest.mark.parametrize("t", [0.1, 0.6, 0.9])
@pytest.mark.parametrize("n", [36, 196, 256])
@pytest.mark.parametrize("ties", [False, True])
def test_mass_mask_against_stable_sort(t, n, ties):
    from ssl_wafermap_amd.interpret import attention_mass_mask

    g = torch.Generator().manual_seed(n + int(10 * t) + 7 * ties)
    rows = 48
    if ties:   # few distinct levels: many exact ties
        a = torch.randint(0, 6, (rows, n), generator=g).float() / 8
        a[0] = 0.25   # a whole row of equal values
    else:
        a = torch.softmax(torch.randn(rows, n, generator=g) * 3, dim=-1)
    cls = torch.cat([torch.full((rows, 1), 0.5), a], dim=1).to(DEV)   # column 0 (the class token) is left out
    got = attention_mass_mask(cls, t).cpu()
    assert got.shape == (rows, n) and got.dtype == torch.bool
    want, cum = mass_mask_ref(a.double(), t)
    far = (cum - (1 - t)).abs() >= 1e-6
    assert torch.equal(got[far], want[far])
    assert bool(far.float().mean() > 0.9)
    assert torch.equal(attention_mass_mask(cls, t).cpu(), got)


# ------------------------------------------------------------------------------------------ 5. EigenCAM kernel
def planted(n, c, h, w, seed):
    """Activations with a planted leading component: rank-one spatial pattern x channel loading, plus noise."""
    g = torch.Generator().manual_seed(seed)
    pat = torch.randn(n, 1, h, w, generator=g)
    load = torch.randn(n, c, 1, 1, generator=g).abs() + 0.5
    return 3.0 * pat * load + 0.3 * torch.randn(n, c, h, w, generator=g) + 1.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("hw", [(3, 3), (7, 7), (8, 8)])
def test_eigencam_kernel_planted(hw, dtype):
    from ssl_wafermap_amd.interpret import eigencam_maps

    h, w = hw
    act = planted(6, 512, h, w, seed=h).to(dtype)
    ref, gaps = eigencam_ref(act.double(), 224)
    _measure(f"eigencam_planted_min_gap[{h}x{w}]", float(gaps.min()))
    assert gaps.min() >= 1.5
    got = eigencam_maps(act.to(DEV).contiguous(memory_format=torch.channels_last), 224)
    assert got.shape == (6, 224, 224) and got.dtype == torch.float32
    err = (got.double().cpu() - ref).abs().max().item()
    _measure(f"eigencam_planted_err[{dtype},{h}x{w}]", err)
    assert err <= 1e-7, err   # measured <= 3.0e-8 (float32 output rounding); smallest gap 4.4e3
    assert torch.equal(eigencam_maps(act.to(DEV).contiguous(memory_format=torch.channels_last), 224), got)


def test_eigencam_kernel_zero_nan_and_layouts():
    from ssl_wafermap_amd.interpret import eigencam_maps

    act = planted(4, 96, 7, 7, seed=3)
    act[0] = 0.0                      # lambda1 = 0 -> zeros
    act[1, 5, 2, 3] = float("nan")    # NaN -> 0
    act[1, :, 0, 0] = float("nan")
    act[2] = 2.5                      # constant: centred to zero -> zeros
    ref, _ = eigencam_ref(act, 7)
    got = eigencam_maps(act.to(DEV), None).cpu()   # default size: the activation grid; NCHW memory is accepted too
    assert got.shape == (4, 7, 7)
    assert torch.equal(got[0], torch.zeros(7, 7)) and torch.equal(got[2], torch.zeros(7, 7))
    assert bool(torch.isfinite(got).all())
    err = (got.double() - ref).abs().max().item()
    _measure("eigencam_nan_err", err)
    assert err <= 1e-7, err   # measured 2.9e-8


def test_eigencam_kernel_real_layer4():
    """Layer4 activations of golden wafers (random-init ResNet-18): real spectra, eigengaps recorded."""
    from ssl_wafermap_amd.interpret import eigencam_maps

    net = make_resnet()
    x = golden_images(32, 224)
    with torch.no_grad():
        act = net.forward_features(x)
    ref, gaps = eigencam_ref(act.double(), 224)
    _measure("layer4_gap_min", float(gaps.min()))
    _measure("layer4_gap_median", float(np.median(gaps)))
    for a in (act, act.float().contiguous(memory_format=torch.channels_last)):
        got = eigencam_maps(a, 224).double().cpu()
        err = (got - ref).abs().max().item()
        _measure(f"eigencam_layer4_err[{a.dtype}]", err)
        assert err <= 1e-7, err   # measured <= 3.0e-8 at eigengaps lambda1 / lambda2 from 1.22 (median 2.0)


# ------------------------------------------------------------------------------------------ 6. end to end
def test_eigencam_end_to_end():
    from ssl_wafermap_amd.interpret import eigencam

    net = make_resnet(1)
    net.train()
    x = golden_images(16, 224, start=100)
    cams = eigencam(net, x)
    assert net.training   # mode restored
    assert cams.shape == (16, 224, 224)
    net.eval()
    with torch.no_grad():
        act = net.forward_features(x)
    ref, _ = eigencam_ref(act.double(), 224)
    err = (cams.double().cpu() - ref).abs().max().item()
    _measure("eigencam_e2e_err", err)
    assert err <= 1e-7, err   # measured 3.0e-8
    assert torch.equal(eigencam(net, x), cams)
    assert eigencam(net, x, target_size=(64, 96)).shape == (16, 64, 96)


def test_attention_maps_end_to_end():
    from ssl_wafermap_amd.interpret import attention_maps

    vit = make_vit("small", seed=2)
    x = golden_images(8, 224, start=200)
    with torch.no_grad():
        qkv, n, seq = vit.last_qkv(x)
    ref = probs_ref(qkv, n, seq, 6, 64 ** -0.5)[:, :, 0]   # float64 [N, H, S] of the same qkv
    maps = attention_maps(vit, x, upsample=False)
    assert maps.shape == (8, 6, 14, 14)
    err = (maps.double() - ref[:, :, 1:].reshape(8, 6, 14, 14)).abs().max().item()
    _measure("attention_maps_err", err)
    assert err <= 4e-7, err   # measured 1.8e-7
    up = attention_maps(vit, x)
    assert up.shape == (8, 6, 224, 224)
    assert torch.equal(up, maps.repeat_interleave(16, 2).repeat_interleave(16, 3))
    assert torch.equal(attention_maps(vit, x), up)
    for t in (0.1, 0.6, 0.9):
        m = attention_maps(vit, x, threshold=t, upsample=False).cpu()
        assert m.dtype == torch.bool and m.shape == (8, 6, 14, 14)
        want, cum = mass_mask_ref(ref[:, :, 1:].reshape(48, 196).cpu(), t)
        far = (cum - (1 - t)).abs() >= 1e-5   # the probabilities carry ~1e-6 of error (above)
        assert torch.equal(m.reshape(48, 196)[far], want[far])
    mu = attention_maps(vit, x, threshold=0.6)
    assert mu.shape == (8, 6, 224, 224) and mu.dtype == torch.bool


def test_get_last_selfattention_cls_row_matches_maps():
    from ssl_wafermap_amd.interpret import attention_maps

    vit = make_vit("tiny", seed=3)
    x = golden_images(4, 96)
    full = vit.get_last_selfattention(x)
    maps = attention_maps(vit, x, upsample=False)
    assert torch.equal(full[:, :, 0, 1:].reshape(maps.shape), maps)


# ------------------------------------------------------------------------------------------ 7. script
def test_attention_figures_script(tmp_path):
    spec = importlib.util.spec_from_file_location("attention_figures_amd", ROOT / "scripts/attention_figures_amd.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    res = mod.main(["--data", str(FIXTURE), "--failure-types", "Scratch", "Edge-Loc", "--per-type", "2",
                    "--threshold", "0.6", "--out", str(tmp_path)])
    shapes = {"images": (4, 224, 224), "labels": (4,), "attention": (4, 6, 224, 224), "attention_mask": (4, 6, 224, 224),
              "eigencam": (4, 224, 224)}
    for k, shp in shapes.items():
        arr = np.load(tmp_path / f"{k}.npy")
        assert arr.shape == shp, (k, arr.shape)
        assert np.array_equal(arr, res[k])
    assert np.load(tmp_path / "attention_mask.npy").dtype == bool
    assert list(np.load(tmp_path / "labels.npy")) == [7, 7, 2, 2]
    cams = np.load(tmp_path / "eigencam.npy")
    assert cams.min() >= 0 and cams.max() <= 1
