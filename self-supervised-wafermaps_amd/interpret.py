"""Model inspection on the HIP kernels (csrc/interpret.hip): the self-attention maps and EigenCAM of the reference's
report figures (notebooks/2.0-Figures-DINO-attention.ipynb, notebooks/2.0-Figures-GradCAM.ipynb).

    p = attention_probs(qkv, batch, seq, heads, scale)          # float32 [B, H, S, S] (cls_only: [B, H, 1, S])
    maps = attention_maps(vit, images)                          # float32 [N, H, S, S]: class-token row, upsampled
    masks = attention_maps(vit, images, threshold=0.6)          # bool, dino's attention-mass mask
    cams = eigencam(resnet, images)                             # float32 [N, S, S] in [0, 1]

Inference only: nothing here has a backward pass.  No CPU fallback: CPU tensors raise WaferHipError.

EigenCAM's sign rule: the leading singular vector has no sign of its own (LAPACK's, and so pytorch_grad_cam's, is
arbitrary).  Here the projection is flipped so that it correlates non-negatively with the per-position channel sums of
the uncentred activations, which makes the strongly activated positions the hot spots.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple, Union

import torch

from . import _lib
from ._lib import check, dtype_code, ptr, require_gpu, stream_ptr

MAX_SEQ = 256       # tokens per image (attention kernels)
MAX_CAM_HW = 64     # layer4 positions per image (EigenCAM)


def _nhwc(images: torch.Tensor) -> torch.Tensor:
    from . import ops

    return ops.to_nhwc_bf16(images)


def attention_probs(qkv: torch.Tensor, batch: int, seq: int, heads: int, scale: float,
                    cls_only: bool = False) -> torch.Tensor:
    """softmax(scale q k^T) per head of qkv [batch * seq, 3 * heads * head_dim] (the qkv Linear's output, bf16 or
    float32; head_dim 64 or 32, seq <= 256) -> float32 [batch, heads, seq, seq], or [batch, heads, 1, seq] with only
    the class-token row when cls_only."""
    batch, seq, heads = int(batch), int(seq), int(heads)
    if qkv.dim() != 2 or batch <= 0 or seq <= 0 or heads <= 0 or qkv.shape[0] != batch * seq \
            or qkv.shape[1] % (3 * heads) != 0:
        raise ValueError(f"attention_probs: qkv {tuple(qkv.shape)} is not [B*S, 3*H*head_dim] for B={batch} S={seq} "
                         f"H={heads}")
    hd = qkv.shape[1] // (3 * heads)
    if hd not in (32, 64):
        raise ValueError(f"attention_probs: head_dim {hd} (the kernels take 64 or 32)")
    if seq > MAX_SEQ:
        raise ValueError(f"attention_probs: {seq} tokens (at most {MAX_SEQ})")
    if qkv.dtype not in (torch.bfloat16, torch.float32):
        raise _lib.WaferHipError(f"attention_probs: unsupported dtype {qkv.dtype}")
    qkv = qkv.detach().contiguous()
    require_gpu(qkv)
    rows = 1 if cls_only else seq
    out = torch.empty((batch, heads, rows, seq), dtype=torch.float32, device=qkv.device)
    check(_lib.load().wm_attention_probs(ptr(qkv), dtype_code(qkv), batch, seq, heads, hd, float(scale), int(bool(cls_only)),
                                         ptr(out), stream_ptr()), "wm_attention_probs")
    return out


def attention_mass_mask(cls_rows: torch.Tensor, threshold: float) -> torch.Tensor:
    """dino visualize_attention.py's --threshold mask of class-token rows [..., S] (float32, column 0 = the class token
    itself, which is left out): per row, patch i is kept when the patches at or below it in a stable ascending sort hold
    more than 1 - threshold of the row's patch mass.  Returns bool [..., S - 1]."""
    if cls_rows.dim() < 1 or cls_rows.shape[-1] < 2 or cls_rows.shape[-1] - 1 > MAX_SEQ:
        raise ValueError(f"attention_mass_mask: rows {tuple(cls_rows.shape)} (need 2..{MAX_SEQ + 1} columns)")
    threshold = float(threshold)
    if not 0.0 <= threshold <= 1.0:
        raise ValueError(f"attention_mass_mask: threshold {threshold} outside [0, 1]")
    a = cls_rows.detach().float().contiguous()
    require_gpu(a)
    s = a.shape[-1]
    rows = a.numel() // s
    keep = torch.empty(a.shape[:-1] + (s - 1,), dtype=torch.uint8, device=a.device)
    if rows == 0:
        return keep.bool()
    # entries 1..S-1 of each row: the pointer one float in, the row pitch S
    check(_lib.load().wm_attention_mass_mask(ptr(a) + 4, rows, s - 1, s, threshold, ptr(keep), stream_ptr()),
          "wm_attention_mass_mask")
    return keep.bool()


def _check_images(images: torch.Tensor, patch: int = 1) -> int:
    if images.dim() != 4 or images.shape[1] != 3:
        raise ValueError(f"expected images [N, 3, S, S], got {tuple(images.shape)}")
    s = images.shape[-1]
    if images.shape[-2] != s:
        raise ValueError(f"images must be square, got {images.shape[-2]} x {s}")
    if s % patch != 0:
        raise ValueError(f"image size {s} is not a multiple of the patch size {patch}")
    return s


def attention_maps(vit, images: torch.Tensor, threshold: Optional[float] = None,
                   upsample: bool = True) -> torch.Tensor:
    """Class-token attention of the last block of a VisionTransformer, per head, over the patch grid: float32
    [N, H, g, g] (g = S / patch), or with `upsample` the notebook's nearest upsample by the patch size, [N, H, S, S].
    With `threshold` the boolean attention-mass masks (attention_mass_mask) in the same shape."""
    p = vit.patch_embed.patch_size
    s = _check_images(images, p)
    g = s // p
    if g * g + 1 > MAX_SEQ:
        raise ValueError(f"attention_maps: {g * g + 1} tokens at {s}x{s} (at most {MAX_SEQ})")
    if not images.is_cuda:
        raise _lib.WaferHipError("attention_maps: images must be device tensors (no CPU fallback)")
    attn = vit.blocks[-1].attn
    with torch.no_grad():
        qkv, n, seq = vit.last_qkv(images)
        cls = attention_probs(qkv, n, seq, attn.num_heads, attn.scale, cls_only=True)[:, :, 0]   # [N, H, S]
        if threshold is not None:
            out = attention_mass_mask(cls, threshold).reshape(n, -1, g, g)
        else:
            out = cls[:, :, 1:].reshape(n, -1, g, g)
        if upsample:
            out = out.repeat_interleave(p, dim=2).repeat_interleave(p, dim=3)
    return out


def eigencam_maps(act: torch.Tensor, target_size: Union[int, Tuple[int, int], None] = None) -> torch.Tensor:
    """EigenCAM of activations [N, C, H, W] (bf16 or float32; H * W <= 64) -> float32 [N, out_h, out_w] in [0, 1]
    (target_size: int, (out_h, out_w) or None for H x W)."""
    if act.dim() != 4:
        raise ValueError(f"eigencam: activations {tuple(act.shape)} are not [N, C, H, W]")
    n, c, h, w = act.shape
    if h * w > MAX_CAM_HW:
        raise ValueError(f"eigencam: {h}x{w} = {h * w} positions per image (at most {MAX_CAM_HW}: inputs up to 256^2)")
    if target_size is None:
        oh, ow = h, w
    elif isinstance(target_size, int):
        oh = ow = target_size
    else:
        oh, ow = (int(v) for v in target_size)
    if not (0 < oh <= 4096 and 0 < ow <= 4096):
        raise ValueError(f"eigencam: target size {oh}x{ow}")
    if act.dtype not in (torch.bfloat16, torch.float32):
        act = act.float()
    a = act.detach().contiguous(memory_format=torch.channels_last)
    if not a.is_cuda:
        raise _lib.WaferHipError("eigencam: activations must be device tensors (no CPU fallback)")
    out = torch.empty((n, oh, ow), dtype=torch.float32, device=a.device)
    if n == 0:
        return out
    check(_lib.load().wm_eigencam(ptr(a), dtype_code(a), n, c, h, w, oh, ow, ptr(out), stream_ptr()), "wm_eigencam")
    return out


def eigencam(backbone, images: torch.Tensor, target_size: Union[int, Sequence[int], None] = None) -> torch.Tensor:
    """pytorch_grad_cam.EigenCAM(model, target_layers=[backbone.layer4[-1]]) of a ResNet-18 backbone: forward_features in
    eval mode without gradients, then eigencam_maps.  Returns float32 [N, S, S] for square images [N, 3, S, S] (the
    default target size is the input size, as pytorch_grad_cam's), in [0, 1].  The backbone's train / eval mode is
    restored afterwards."""
    s = _check_images(images)
    # layer4 of ResNet-18: stride 32 (conv1 / max-pool / layers 2-4 each halve, rounding up)
    h4 = s
    for _ in range(5):
        h4 = (h4 + 1) // 2
    if h4 * h4 > MAX_CAM_HW:
        raise ValueError(f"eigencam: {s}x{s} images give a {h4}x{h4} layer4 map (at most {MAX_CAM_HW} positions)")
    if not images.is_cuda:
        raise _lib.WaferHipError("eigencam: images must be device tensors (no CPU fallback)")
    was_training = backbone.training
    backbone.eval()
    try:
        with torch.no_grad():
            act = backbone.forward_features(_nhwc(images))
    finally:
        backbone.train(was_training)
    return eigencam_maps(act, s if target_size is None else target_size)
