#!/usr/bin/env python3
"""Report figures of model inspection on MI355X: the reference's notebooks/2.0-Figures-DINO-attention.ipynb (DINO
ViT-S/16 self-attention of the class token, per head) and notebooks/2.0-Figures-GradCAM.ipynb (EigenCAM of a ResNet-18
SSL backbone's layer4) on the HIP path (ssl_wafermap_amd.interpret).

    python scripts/attention_figures_amd.py [--dino-ckpt PATH] [--resnet-ckpt PATH] [--resnet-model FastSiam]
                                            [--data tests/golden/wm811k_train_1_split.npz | wafers.pkl.xz]
                                            [--failure-types Scratch Edge-Loc] [--per-type 1] [--threshold 0.6]
                                            [--out DIR]

What the notebooks do, and where it is here:
  DINO-attention  model.backbone.get_last_selfattention(img)[0, :, 0, 1:], reshape to the patch grid, nearest upsample
                  by the patch size, plt.imshow(cmap="Reds", norm=PowerNorm(gamma=2))
                                                    -> interpret.attention_maps(backbone, images[, threshold])
  GradCAM         EigenCAM(backbone, [backbone.layer4[-1]])(img), show_cam_on_image (cv2.applyColorMap)
                                                    -> interpret.eigencam(backbone, images), matplotlib colormap overlay
Wafers are chosen by failure type (the first --per-type wafers of each, in file order).  Without a checkpoint the
model keeps its random initialisation.  Outputs under --out: images.npy [N, S, S] (the grey inference image),
labels.npy, attention.npy [N, H, S, S] float32, attention_mask.npy [N, H, S, S] bool (with --threshold), eigencam.npy
[N, S, S] float32; PNGs as well when matplotlib imports.
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

FIXTURE = ROOT / "tests/golden/wm811k_train_1_split.npz"
# WM-811K failureType <-> failureCode of the reference's processed data (src/ssl_wafermap/models/knn.py:244-254)
FAILURE_TYPES = ["Center", "Donut", "Edge-Loc", "Edge-Ring", "Loc", "Near-full", "Random", "Scratch", "none"]


def load_wafers(path):
    """(WaferStore on the host, failure codes) from a store .npz or a reference *.pkl.xz (data/ingest.py)."""
    from ssl_wafermap_amd.data import WaferStore
    from ssl_wafermap_amd.data.ingest import read_wafer_pickle

    path = Path(path)
    if path.suffix == ".npz":
        store, labels = WaferStore.load(path)
    else:
        store, labels = read_wafer_pickle(path)
    if labels is None:
        raise ValueError(f"{path}: no failure labels")
    return store, np.asarray(labels).astype(np.int64)


def select(labels: np.ndarray, types, per_type: int) -> np.ndarray:
    idx = []
    for t in types:
        if t not in FAILURE_TYPES:
            raise ValueError(f"unknown failure type {t!r} (have {FAILURE_TYPES})")
        hits = np.flatnonzero(labels == FAILURE_TYPES.index(t))[:per_type]
        idx.extend(int(i) for i in hits)
    if not idx:
        raise ValueError(f"no wafer of the failure types {list(types)}")
    return np.array(idx, dtype=np.int64)


def inference_images(store, idx, size, device):
    """Inference transform (resize, grey, normalise) of the selected wafers: bf16 channels_last [N, 3, size, size]."""
    import torch

    from ssl_wafermap_amd.data import WaferStore
    from ssl_wafermap_amd.transforms import augment_views, get_inference_transforms, sample_view_params

    sub = WaferStore([store.wafer(int(i)) for i in idx], device=device)
    params = sample_view_params(get_inference_transforms((size, size)), np.arange(len(idx)), sub.heights_np,
                                sub.widths_np, np.random.default_rng(0))
    x = augment_views(sub, params, img_size=size, out_size=size, fmt="nhwc_bf16")
    return x.to(torch.device(device))


def _pngs(out: Path, images, names, attn, cams):
    try:
        import matplotlib

        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
        from matplotlib import colors
    except ImportError:
        return False
    for i, name in enumerate(names):
        heads = attn.shape[1]
        fig, axes = plt.subplots(1, heads + 1, figsize=(2.2 * (heads + 1), 2.4))
        axes[0].imshow(images[i], cmap="gray")
        axes[0].set_title(name)
        for h in range(heads):
            axes[h + 1].imshow(attn[i, h], cmap="Reds", norm=colors.PowerNorm(gamma=2))
            axes[h + 1].set_title(f"head {h}")
        for a in axes:
            a.axis("off")
        fig.savefig(out / f"attention_{i:03d}_{name}.png", dpi=120, bbox_inches="tight")
        plt.close(fig)
        # show_cam_on_image: 0.5 heat map + 0.5 image, the heat map from a matplotlib colormap instead of cv2.applyColorMap
        grey = (images[i] - images[i].min()) / max(float(np.ptp(images[i])), 1e-12)
        heat = plt.get_cmap("jet")(cams[i])[..., :3]
        overlay = 0.5 * heat + 0.5 * grey[..., None]
        plt.imsave(out / f"eigencam_{i:03d}_{name}.png", np.clip(overlay / overlay.max(), 0, 1))
    return True


def main(argv=None) -> dict:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--dino-ckpt", default=None, help="Lightning-layout checkpoint of DINOViT (random weights if absent)")
    ap.add_argument("--resnet-ckpt", default=None, help="Lightning-layout checkpoint of --resnet-model")
    ap.add_argument("--resnet-model", default="FastSiam", help="model class of the ResNet-18 checkpoint")
    ap.add_argument("--data", default=str(FIXTURE), help="WaferStore .npz or a reference *.pkl.xz with failure labels")
    ap.add_argument("--failure-types", nargs="+", default=["Scratch", "Edge-Loc"])
    ap.add_argument("--per-type", type=int, default=1)
    ap.add_argument("--img-size", type=int, default=224)
    ap.add_argument("--threshold", type=float, default=None, help="dino's attention-mass mask threshold")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default="attention_figures")
    args = ap.parse_args(argv)

    import torch

    from ssl_wafermap_amd import interpret
    from ssl_wafermap_amd import models as zoo
    from ssl_wafermap_amd.utils.checkpoint import load_checkpoint

    dev = torch.device("cuda:0")
    torch.manual_seed(args.seed)
    store, labels = load_wafers(args.data)
    idx = select(labels, args.failure_types, args.per_type)
    x = inference_images(store, idx, args.img_size, dev)

    dino = zoo.DINOViT(None, 9, batch_norm=False).to(dev)
    if args.dino_ckpt:
        load_checkpoint(dino, args.dino_ckpt)
    resnet = getattr(zoo, args.resnet_model)(None, 9).to(dev)
    if args.resnet_ckpt:
        load_checkpoint(resnet, args.resnet_ckpt)

    attn = interpret.attention_maps(dino.backbone, x)
    cams = interpret.eigencam(resnet.backbone, x)
    out = Path(args.out)
    out.mkdir(parents=True, exist_ok=True)
    images = x[:, 0].float().cpu().numpy()
    result = {"images": images, "labels": labels[idx], "attention": attn.cpu().numpy(), "eigencam": cams.cpu().numpy()}
    if args.threshold is not None:
        result["attention_mask"] = interpret.attention_maps(dino.backbone, x, threshold=args.threshold).cpu().numpy()
    for k, v in result.items():
        np.save(out / f"{k}.npy", v)
    names = [FAILURE_TYPES[int(labels[i])] for i in idx]
    pngs = _pngs(out, images, names, result["attention"], result["eigencam"])
    print(f"{len(idx)} wafers ({', '.join(names)}) -> {out}: " + ", ".join(f"{k}{list(v.shape)}" for k, v in result.items())
          + (" + PNGs" if pngs else " (matplotlib not available: no PNGs)"))
    return result


if __name__ == "__main__":
    main()
