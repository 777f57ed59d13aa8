"""GPU: north_star's floating-point tolerance -- whole-step loss within 1e-4 relative and embeddings within 1e-3 cosine
of the reference's float32 CPU path -- met under the float32 ("parity") precision preset, for the three steps the
reference runs: SimCLR ResNet-18 at bs 64 (scripts/WM811k_benchmark.py:236-248), DINO ViT-Tiny (:578-588) and MAE
ViT-S/16 (:902-947).

Why a preset: profiles/r04_error_budget_bf16.md (tools/error_budget.py) splits the bf16 preset's loss error by stage --
it is the bf16 storage of the inter-layer activations (every active stage adds +-1e-5 .. 1e-4, signs mixed), the same
distance torch's own bf16 autocast of the oracle code lands at (profiles/r04_bf16_gradient_noise.md); the bf16 tests
(test_gpu_stability.py, test_gpu_ops.py, test_gpu_vit.py) therefore assert bounds of a few 1e-4.  Here the same modules,
weights and inputs run with float32 activations (csrc/f32path.hip) and the contract's own numbers are asserted."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from parity_log import parity

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


# ------------------------------------------------------------------------------------------------ kernels vs torch
@pytest.mark.parametrize("n,c,h,k,r,stride,pad", [(3, 3, 20, 64, 7, 2, 3), (2, 64, 14, 128, 3, 2, 1), (2, 128, 9, 128, 3, 1, 1),
                                                  (2, 64, 8, 128, 1, 2, 0), (5, 37, 6, 70, 3, 1, 1)])
def test_f32_conv_matches_torch(n, c, h, k, r, stride, pad):
    # (hand-set 2e-6 against float32 torch; the derived bounds, exact lattices and ragged tiles of the same kernel are in
    # tests/test_gpu_f32_kernels.py::test_conv_lattice_is_exact / test_conv_forward_and_backward_through_every_epilogue)
    from ssl_wafermap_amd import f32path

    g = torch.Generator().manual_seed(n * 100 + c)
    x, w = torch.randn(n, c, h, h, generator=g), torch.randn(k, c, r, r, generator=g) * (c * r * r) ** -0.5
    b, res_shape = torch.randn(k, generator=g), None
    ref = F.conv2d(x, w, b, stride, pad)
    res = torch.randn(ref.shape, generator=g)
    got = f32path.conv2d(x.to(DEV), w.to(DEV), stride, pad, bias=b.to(DEV), act=f32path.ACT_GELU, residual=res.to(DEV))
    want = F.gelu(ref) + res
    parity(f"float32 conv {c}->{k} {r}x{r}/{stride} + bias + GELU + residual vs torch (max abs / max ref)",
           float((got.cpu() - want).abs().max() / want.abs().max()), 2e-6)


def test_f32_batchnorm_layernorm_pool_attention_match_torch():
    # (one shape per op against float32 torch with hand-set tolerances; per entry point, against float64 with derived bounds, ties
    # in the pooling windows and the edge shapes: tests/test_gpu_f32_kernels.py)
    from ssl_wafermap_amd import f32path

    g = torch.Generator().manual_seed(0)
    x = torch.randn(8, 64, 6, 6, generator=g) * 2 + 0.7
    gamma, beta = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.1
    rm, rv, nb = torch.zeros(64), torch.ones(64), torch.tensor(0)
    res = torch.randn(8, 64, 6, 6, generator=g)
    parts = [F.relu(F.batch_norm(p, rm, rv, gamma, beta, True, 0.1, 1e-5) + r) for p, r in zip(x.chunk(2), res.chunk(2))]
    drm, drv, dnb = torch.zeros(64, device=DEV), torch.ones(64, device=DEV), torch.tensor(0, device=DEV)
    got = f32path.batch_norm(x.to(DEV), gamma.to(DEV), beta.to(DEV), drm, drv, True, res.to(DEV), True, 1e-5, 0.1, 2, dnb)
    parity("float32 BatchNorm (2 groups, residual, ReLU) vs torch (max abs)", float((got.cpu() - torch.cat(parts)).abs().max()), 5e-6)
    torch.testing.assert_close(drm.cpu(), rm, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(drv.cpu(), rv, rtol=1e-5, atol=1e-6)
    assert int(dnb) == 2
    ev = f32path.batch_norm(x.to(DEV), gamma.to(DEV), beta.to(DEV), drm, drv, False)
    torch.testing.assert_close(ev.cpu(), F.batch_norm(x, rm, rv, gamma, beta, False, 0.1, 1e-5), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(f32path.max_pool3x3s2(x.to(DEV)).cpu(), F.max_pool2d(x, 3, 2, 1))
    torch.testing.assert_close(f32path.global_avg_pool(x.to(DEV)).cpu(), x.mean((2, 3)), rtol=1e-5, atol=1e-6)
    t = torch.randn(50, 192, generator=g) * 3 + 1
    lw, lb = torch.rand(192, generator=g) + 0.5, torch.randn(192, generator=g)
    torch.testing.assert_close(f32path.layer_norm(t.to(DEV), lw.to(DEV), lb.to(DEV), 1e-6).cpu(),
                               F.layer_norm(t, (192,), lw, lb, 1e-6), rtol=1e-5, atol=1e-5)
    for hd, heads, s in ((64, 3, 37), (32, 16, 50), (64, 6, 197)):
        qkv = torch.randn(2 * s, 3 * heads * hd, generator=g)
        q, k, v = qkv.reshape(2, s, 3, heads, hd).permute(2, 0, 3, 1, 4)
        ref = ((q @ k.transpose(-2, -1)) * hd ** -0.5).softmax(-1) @ v
        ref = ref.transpose(1, 2).reshape(2 * s, heads * hd)
        got = f32path.attention(qkv.to(DEV), 2, s, heads, None, hd)
        parity(f"float32 attention {heads} x {hd}, {s} tokens vs torch (max abs)", float((got.cpu() - ref).abs().max()), 5e-6)


# ------------------------------------------------------------------------------------------------ SimCLR
def test_simclr_bs64_step_under_the_float32_preset_meets_the_contract():
    """SimCLR ResNet-18, 64 wafers, two 224 x 224 views, identical weights and augmentation decisions: loss <= 1e-4
    relative, backbone embeddings and projections <= 1e-3 (1 - cosine, worst row) against the float32 oracle."""
    from oracle import resnet as orn
    from ssl_wafermap_amd import precision
    from ssl_wafermap_amd.data import WaferMapDataset
    from ssl_wafermap_amd.data.synthetic import synthetic_wafers
    from ssl_wafermap_amd.models import SimCLR
    from ssl_wafermap_amd.transforms import BaseViewTransform, augment_views

    B = 64
    for seed in (3, 4):
        wafers, labels = synthetic_wafers(128, seed=seed)
        ds = WaferMapDataset(wafers, labels, transform=BaseViewTransform(), device=DEV)
        torch.manual_seed(0)
        model = SimCLR(None, 9, batch_size=B, max_epochs=150).to(DEV).train()
        sd = {k: v.detach().float().cpu().clone() for k, v in model.state_dict().items()}
        params = ds.transform.sample(ds.store, np.arange(B), np.random.default_rng(seed))
        v = augment_views(ds.store, params[0], fmt="nchw_f32", n_slots=2 * B)     # float32, bit-exact vs oracle/augment.py
        got = {}
        hooks = [model.backbone.register_forward_hook(lambda m, a, o: got.__setitem__("f", o.detach().float().cpu())),
                 model.projection_head.register_forward_hook(lambda m, a, o: got.__setitem__("z", o.detach().float().cpu()))]
        with precision.precision("float32"):
            loss = model.training_step(((v[:B], v[B:]), None), 0)
        for h in hooks:
            h.remove()
        vc = v.cpu()
        ref, (f0, f1, z0, z1) = orn.simclr_loss(vc[:B], vc[B:], sd, 0.5, True)
        parity(f"SimCLR bs 64 whole-step loss, float32 preset vs float32 oracle (relative), seed {seed}", _rel(loss.detach(), ref), 1e-4)
        cf = 1 - F.cosine_similarity(got["f"], torch.cat([f0, f1]), dim=1)
        cz = 1 - F.cosine_similarity(got["z"], torch.cat([z0, z1]), dim=1)
        parity(f"SimCLR bs 64 backbone embeddings, float32 preset (1 - cosine, worst row), seed {seed}", float(cf.max()), 1e-3)
        parity(f"SimCLR bs 64 projections, float32 preset (1 - cosine, worst row), seed {seed}", float(cz.max()), 1e-3)


def test_resnet18_small_images_projections_under_the_float32_preset():
    """The configuration of test_gpu_ops.py::test_resnet18_forward_backward_matches_oracle (bs 32 of 64 x 64, last BN gains
    0.5) where the bf16 preset's projections sit at 1.45e-3: <= 1e-3 cosine and <= 1e-4 on the loss in float32."""
    from oracle import resnet as orn
    from ssl_wafermap_amd import ops, precision
    from ssl_wafermap_amd.heads import SimCLRProjectionHead
    from ssl_wafermap_amd.loss import NTXentLoss, stacked_views
    from ssl_wafermap_amd.models import create_model

    torch.manual_seed(0)
    backbone, head = create_model("resnet18", num_classes=0), SimCLRProjectionHead(512, 512, 128)
    for m in backbone.modules():
        if hasattr(m, "bn2"):
            torch.nn.init.constant_(m.bn2.weight, 0.5)
    sd = {"backbone." + k: v.clone() for k, v in backbone.state_dict().items()}
    sd.update({"projection_head." + k: v.clone() for k, v in head.state_dict().items()})
    g = torch.Generator().manual_seed(1)
    lut = torch.tensor([-1.5366, 0.1790, 1.8811])
    x0 = lut[torch.randint(0, 3, (32, 1, 64, 64), generator=g)].expand(-1, 3, -1, -1).contiguous()
    x1 = lut[torch.randint(0, 3, (32, 1, 64, 64), generator=g)].expand(-1, 3, -1, -1).contiguous()
    ref, (f0, f1, z0, z1) = orn.simclr_loss(x0, x1, {k: v.clone() for k, v in sd.items()}, 0.5, True)
    backbone.to(DEV).train()
    head.to(DEV).train()
    with precision.precision("float32"), ops.bn_groups(2):
        f = backbone(torch.cat([x0, x1]).to(DEV))
        z = head(f)
        loss = NTXentLoss(0.5)(*stacked_views(z.contiguous(), 32))
    cz = 1 - F.cosine_similarity(z.float().cpu(), torch.cat([z0, z1]), dim=1)
    parity("ResNet-18 + SimCLR head projections, bs 32 of 64x64, float32 preset (1 - cosine, worst row)", float(cz.max()), 1e-3)
    parity("ResNet-18 + head + NT-Xent loss, bs 32 of 64x64, float32 preset (relative)", _rel(loss.detach(), ref), 1e-4)


def test_simclr_optimiser_steps_under_the_float32_preset_stay_within_float32_noise_of_a_float64_run():
    """The whole SimCLR step (scripts/WM811k_benchmark.py:242-255: two-view forward, NT-Xent, backward, SGD with momentum and
    weight decay) under the float32 preset, at three successive points of a training run (bs 32, identical augmentation
    decisions).  The yardstick is the oracle run in FLOAT64: once the zero-initialised residual BatchNorm scales leave zero
    (after the first update) the float32 gradient of this network is itself only good to ~1e-2 -- torch's own float32 autograd
    differs from its float64 autograd by 0.2-1 % per tensor at IDENTICAL parameters on steps 2 and 3
    (profiles/r04_error_budget_bf16.md, "float32 gradient noise") -- so two float32 implementations cannot be held to 1e-5
    of each other along a free-running trajectory.  Each step therefore starts from the float64 run's parameters (rounded),
    and asserts: the loss within 1e-5 of float64; the whole gradient no further from float64 than 3x the float32 oracle's
    own distance; every tensor of step 1 (where float32 is still well conditioned) within 1e-3 of the float32 oracle; and
    the fused SGD update, fed its own gradients and momentum, within 1e-6 of the oracle's update rule."""
    from oracle import resnet as orn
    from ssl_wafermap_amd import ops, precision
    from ssl_wafermap_amd.data import WaferMapDataset
    from ssl_wafermap_amd.data.synthetic import synthetic_wafers
    from ssl_wafermap_amd.models import SimCLR
    from ssl_wafermap_amd.transforms import BaseViewTransform, augment_views

    B, steps = 32, 3
    wafers, labels = synthetic_wafers(128, seed=7)
    ds = WaferMapDataset(wafers, labels, transform=BaseViewTransform(), device=DEV)
    torch.manual_seed(0)
    model = SimCLR(None, 9, batch_size=B, max_epochs=150, log_rep_std=False).to(DEV).train()
    (opt,), _ = model.configure_optimizers()
    lr = opt.param_groups[0]["lr"]
    names = [k for k, _ in model.named_parameters()]
    sd64 = {k: v.detach().double().cpu().clone() for k, v in model.state_dict().items()}
    for k in names:
        sd64[k].requires_grad_(True)
    bufs64, bufs_own = {}, {}
    rng = np.random.default_rng(5)

    def flat(gs):
        return torch.cat([gs[k].reshape(-1).double() for k in names])

    worst_loss = worst_ratio = worst_update = worst_first = 0.0
    report = []
    for i in range(steps):
        idx = (np.arange(B) + i * B) % len(ds)
        params = ds.transform.sample(ds.store, idx, rng)
        v = augment_views(ds.store, params[0], fmt="nchw_f32", n_slots=2 * B)
        vc = v.cpu()
        # float64 run: the yardstick, and the parameters every float32 evaluation of this step starts from
        for k in names:
            sd64[k].grad = None
        l64, _ = orn.simclr_loss(vc[:B].double(), vc[B:].double(), sd64, 0.5, True)
        l64.backward()
        g64 = {k: sd64[k].grad for k in names}
        # float32 oracle at those parameters
        sd32 = {k: t.detach().float().clone() for k, t in sd64.items()}
        for k in names:
            sd32[k].requires_grad_(True)
        l32, _ = orn.simclr_loss(vc[:B], vc[B:], sd32, 0.5, True)
        l32.backward()
        g32 = {k: sd32[k].grad for k in names}
        # the HIP float32 preset at those parameters
        with torch.no_grad():
            for k, p_ in model.named_parameters():
                p_.copy_(sd32[k].detach().to(DEV))
        ops.bump_weight_epoch()
        opt.zero_grad()
        with precision.precision("float32"):
            loss = model.training_step(((v[:B], v[B:]), None), i)
            loss.backward()
        gh = {k: p_.grad.detach().float().cpu() for k, p_ in model.named_parameters()}
        f64 = flat(g64)
        e_hip = float((flat(gh) - f64).norm() / f64.norm())
        e_ora = float((flat(g32) - f64).norm() / f64.norm())
        report.append((i + 1, _rel(loss.detach(), l64.detach()), e_hip, e_ora))
        worst_loss = max(worst_loss, _rel(loss.detach(), l64.detach()))
        worst_ratio = max(worst_ratio, e_hip / (3 * e_ora + 1e-6))
        if i == 0:
            for k in names:
                if float(g32[k].norm()) > 1e-12:
                    worst_first = max(worst_first, float((gh[k] - g32[k]).norm() / g32[k].norm()))
        # the fused SGD update against the oracle's rule on the same (own) gradients and momentum
        own = {k: sd32[k].detach().clone() for k in names}
        opt.step()
        orn.sgd_step(own, gh, bufs_own, lr=lr)
        for k, p_ in model.named_parameters():
            worst_update = max(worst_update, float((p_.detach().float().cpu() - own[k]).abs().max()
                                                   / own[k].abs().max().clamp_min(1e-12)))
        with torch.no_grad():
            orn.sgd_step({k: sd64[k] for k in names}, g64, bufs64, lr=lr)
    torch.cuda.synchronize()
    for r in report:
        print("step %d: loss vs float64 %.2e; gradient vs float64: HIP float32 %.2e, torch float32 %.2e" % r)
    parity("SimCLR bs 32, three training states, float32 preset: loss vs float64 oracle (relative, worst step)", worst_loss, 1e-5)
    parity("SimCLR bs 32, float32 preset: step-1 parameter gradients vs float32 oracle (relative L2, worst tensor)", worst_first, 1e-3)
    parity("SimCLR bs 32, float32 preset: gradient distance to float64 / (3 x the float32 oracle's distance), worst step",
           worst_ratio, 1.0)
    parity("SimCLR bs 32, float32 preset: fused SGD update vs the oracle's rule (relative max, worst tensor and step)",
           worst_update, 1e-6)


# ------------------------------------------------------------------------------------------------ DINO ViT-Tiny
def test_dino_vit_tiny_step_under_the_float32_preset_meets_the_contract():
    """BASELINE.json configs[2]'s model at full depth (12 blocks), 8 wafers, 2 x 224 + 2 x 96 crops -- the step of
    test_gpu_vit.py::test_dino_training_step_matches_oracle_and_learns[vit_tiny] (bf16 preset: 2.1e-4 .. 3.4e-4)."""
    from oracle import vit as ov
    from ssl_wafermap_amd import ops, precision
    from ssl_wafermap_amd.models import DINOViT

    torch.manual_seed(0)
    model = DINOViT(None, 9, batch_size=8, max_epochs=10, log_rep_std=False, backbone="vit_tiny")
    with torch.no_grad():
        for p_ in model.backbone.parameters():
            if p_.dim() == 1:
                p_.add_(torch.randn_like(p_) * 0.05)
    model.teacher_backbone = copy.deepcopy(model.backbone)
    for p_ in model.teacher_backbone.parameters():
        p_.requires_grad = False
    model = model.to(DEV).train()
    b, nh = 8, 3
    g = torch.Generator().manual_seed(11)
    views = [torch.randn(b, 3, 224, 224, generator=g) for _ in range(2)] + [torch.randn(b, 3, 96, 96, generator=g) for _ in range(2)]
    vd = [v.to(DEV) for v in views]
    sd = {k: v.detach().clone().float() for k, v in model.state_dict().items()}
    s_bb = {k[len("backbone."):]: v.clone() for k, v in sd.items() if k.startswith("backbone.")}
    s_hd = {k[len("head."):]: v.clone() for k, v in sd.items() if k.startswith("head.")}
    t_bb = {k[len("teacher_backbone."):]: v.clone() for k, v in sd.items() if k.startswith("teacher_backbone.")}
    t_hd = {k[len("teacher_head."):]: v.clone() for k, v in sd.items() if k.startswith("teacher_head.")}
    fl = lambda d: {k: v for k, v in d.items() if v.is_floating_point() and "running" not in k}
    ov.update_momentum(s_bb, t_bb, 0.99)
    ov.update_momentum(fl(s_hd), fl(t_hd), 0.99)
    with torch.no_grad():
        t_out = [ov.dino_head(ov.vit_features(v, t_bb, nh), t_hd, training=True) for v in vd[:2]]
        s_out = [ov.dino_head(ov.vit_features(v, s_bb, nh), s_hd, training=True) for v in vd]
        ref, _ = ov.dino_loss(t_out, s_out, torch.zeros(1, 1, 2048, device=DEV), 0.04, 0.1)
    got = {}
    h = model.backbone.norm.register_forward_hook(lambda m, a, o: got.__setitem__("y", o.detach().float()))
    with precision.precision("float32"):
        loss = model.training_step(([ops.to_nhwc_bf16(v) for v in vd], None), 0)
    h.remove()
    parity("DINO ViT-Tiny (12 blocks) whole-step loss, float32 preset vs float32 oracle (relative)", _rel(loss.detach(), ref), 1e-4)
    with torch.no_grad():
        feats = torch.cat([ov.vit_features(torch.cat(vd[:2]), s_bb, nh), ov.vit_features(torch.cat(vd[2:]), s_bb, nh)])
    c = 1 - F.cosine_similarity(got["y"], feats, dim=1)
    parity("DINO ViT-Tiny class-token features, float32 preset (1 - cosine, worst row)", float(c.max()), 1e-3)
    with precision.precision("float32"), pytest.raises(NotImplementedError):
        model.training_step(([ops.to_nhwc_bf16(v) for v in vd], None), 0).backward()   # the transformer ops are forward-only and say so


# ------------------------------------------------------------------------------------------------ MAE ViT-S/16
def test_mae_vit_small_16_step_under_the_float32_preset_meets_the_contract():
    """BASELINE.json configs[3]'s model (ViT-S/16 encoder on 49 of 197 tokens, the reference's 512 / 16 decoder): the step of
    test_gpu_vit.py::test_mae_training_step_matches_oracle_and_learns[vit_small_16] (bf16 preset: 3.3e-4)."""
    from oracle import vit as ov
    from ssl_wafermap_amd import ops, precision
    from ssl_wafermap_amd.models import MAE
    from ssl_wafermap_amd.utils import get_at_index, patchify, random_token_mask

    torch.manual_seed(0)
    model = MAE(None, 9, batch_size=8, log_rep_std=False, backbone="vit_small_16")
    with torch.no_grad():
        model.mask_token.normal_(std=0.02)
        for p_ in model.parameters():
            if p_.dim() == 1:
                p_.add_(torch.randn_like(p_) * 0.02)
    model = model.to(DEV).train()
    b, seq, ps = 8, 197, 16
    g = torch.Generator().manual_seed(4)
    images = torch.randn(b, 3, 224, 224, generator=g).to(DEV)
    keep, mask = random_token_mask((b, seq), 0.75, generator=g)
    keep, mask = keep.to(DEV), mask.to(DEV)
    sd = {k: v.detach().clone().float() for k, v in model.state_dict().items()}
    with torch.no_grad():
        ref = ov.mae_loss(images, sd, keep, mask, enc_heads=6)
        enc_ref = ov.mae_encode(images, sd, keep, 6)
    with precision.precision("float32"):
        x_enc = model.forward_encoder(ops.to_nhwc_bf16(images), keep)
        pred = model.forward_decoder(x_enc, keep, mask)
        target = get_at_index(patchify(ops.to_nhwc_bf16(images), ps), mask - 1)
        loss = model.criterion(pred, target)
    parity("MAE ViT-S/16 whole-step loss, float32 preset vs float32 oracle (relative)", _rel(loss.detach(), ref), 1e-4)
    c = 1 - F.cosine_similarity(x_enc.float().reshape(-1, 384), enc_ref.reshape(-1, 384), dim=1)
    parity("MAE ViT-S/16 encoder tokens, float32 preset (1 - cosine, worst token)", float(c.max()), 1e-3)


# ------------------------------------------------------------------------------------------------ embeddings + kNN-top1, end to end
def test_real_wafer_embeddings_and_knn_top1_match_the_reference_path_end_to_end():
    """north_star: "matching the reference's CPU-path embeddings / kNN-top1 within 1e-3 cosine".  The reference's evaluation
    chain on its OWN wafers (tests/golden/wm811k_train_1_split.npz, 623 maps of data/processed/WM811K/train_1_split):
    get_inference_transforms (src/ssl_wafermap/transforms/augmentations.py:335-357) -> backbone in eval mode ->
    F.normalize -> feature bank / knn_predict with k 5, t 0.1 (src/ssl_wafermap/models/knn.py:67-98), on identical weights:
    oracle (numpy transforms + torch CPU float32) against the HIP path -- embeddings <= 1e-3 cosine and every decided top-1
    prediction identical under the float32 preset (measured 2.4e-7, 0 of 223 differ) AND under the bf16 production preset
    (4.6e-6, 0 of 223)."""
    from conftest import GOLDEN
    from oracle import augment as oa
    from oracle import knn as ok
    from oracle import resnet as orn
    from ssl_wafermap_amd import functional as Fh
    from ssl_wafermap_amd import precision
    from ssl_wafermap_amd.data import WaferStore
    from ssl_wafermap_amd.models import SimCLR
    from ssl_wafermap_amd.transforms import augment_views, get_inference_transforms, sample_view_params
    from ssl_wafermap_amd.utils.benchmarking import knn_predict

    store, labels = WaferStore.load(GOLDEN / "wm811k_train_1_split.npz", device=torch.device(DEV))
    n = store.n
    assert n == 623
    labels = torch.from_numpy(np.asarray(labels).astype(np.int64))
    torch.manual_seed(0)
    model = SimCLR(None, 9, batch_size=64).to(DEV).eval()
    with torch.no_grad():   # eval mode uses the running statistics: give them non-trivial values
        for m in model.backbone.modules():
            if hasattr(m, "running_mean"):
                m.running_mean.normal_(0, 0.1)
                m.running_var.uniform_(0.5, 1.5)
            if hasattr(m, "bn2"):
                torch.nn.init.normal_(m.bn2.weight, 0.5, 0.1)
    sd = {k[len("backbone."):]: v.detach().float().cpu().clone() for k, v in model.state_dict().items() if k.startswith("backbone.")}
    spec = get_inference_transforms()
    params = sample_view_params(spec, np.arange(n), store.heights_np, store.widths_np, np.random.default_rng(0))
    x = augment_views(store, params, fmt="nchw_f32")                       # [623, 3, 224, 224] float32
    # the oracle's own transform of the same wafers (numpy): the kernel's output must BE it
    off = store.offsets_np
    for i in (0, 17, 311, 622):
        w = store.bytes_np[off[i]:off[i] + int(store.heights_np[i]) * int(store.widths_np[i])].reshape(store.heights_np[i], store.widths_np[i])
        assert np.array_equal(x[i].cpu().numpy(), oa.augment_view(w, oa.ViewDecision()))
    with torch.no_grad():
        ref = torch.cat([orn.resnet18_features(x[i:i + 89].cpu(), sd, training=False) for i in range(0, n, 89)])
        with precision.precision("float32"):
            got32 = torch.cat([model.backbone(x[i:i + 89]).float() for i in range(0, n, 89)]).cpu()
        got16 = torch.cat([model.backbone(x[i:i + 89]).float() for i in range(0, n, 89)]).cpu()
    c32 = 1 - F.cosine_similarity(got32, ref, dim=1)
    c16 = 1 - F.cosine_similarity(got16, ref, dim=1)
    parity("real wafers, eval-mode ResNet-18 embeddings, float32 preset vs reference path (1 - cosine, worst wafer)", float(c32.max()), 1e-3)
    parity("real wafers, eval-mode ResNet-18 embeddings, bf16 preset vs reference path (1 - cosine, worst wafer)", float(c16.max()), 1e-3)
    # kNN: the first 400 wafers are the bank, the other 223 the queries
    nb = 400
    bank_r, q_r = F.normalize(ref[:nb], dim=1), F.normalize(ref[nb:], dim=1)
    pred_ref = ok.knn_predict(q_r, bank_r.t().contiguous(), labels[:nb], 9, 5, 0.1)[:, 0]
    scores = ok.knn_scores(*ok.knn_topk(q_r, bank_r.t().contiguous(), 5), labels[:nb], 9, 0.1)
    top2 = scores.topk(2, dim=1).values
    decided = (top2[:, 0] - top2[:, 1]) > 1e-3 * top2[:, 0]

    def hip_top1(feats):
        f = Fh.l2_normalize(feats.to(DEV).contiguous())
        return knn_predict(f[nb:], f[:nb].t(), labels[:nb].to(DEV), 9, 5, 0.1)[:, 0].cpu()

    p32, p16 = hip_top1(got32), hip_top1(got16)
    assert float(decided.float().mean()) > 0.9
    assert torch.equal(p32[decided], pred_ref[decided]), int((p32[decided] != pred_ref[decided]).sum())
    parity("real wafers, kNN top-1 (k 5, t 0.1) float32 preset vs reference path: fraction of ALL queries that differ",
           float((p32 != pred_ref).float().mean()), 0.01)
    parity("real wafers, kNN top-1 bf16 preset vs reference path: fraction of all queries that differ",
           float((p16 != pred_ref).float().mean()), 0.02,
           note="measured 0 of 223 (embeddings 4.6e-6 cosine): the production preset meets the embedding / kNN-top1 contract on real wafers too")
