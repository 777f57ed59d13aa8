"""Checkpoints in the layout of Lightning's `.ckpt` files, which the reference's evaluation scripts read
(scripts/MixedWM38_evals.py:873-903 `load_from_checkpoint`, scripts/WM811k_linear_probe.py:227
`model.load_state_dict(torch.load(path)["state_dict"])`): a dict with "state_dict" (module keys, CPU tensors),
"epoch" and "global_step".  Other top-level keys a Lightning file carries (optimizer_states, callbacks,
hyper_parameters, ...) are ignored when loading."""
from __future__ import annotations

import os
import pickle
from pathlib import Path

import torch


def save_checkpoint(model: torch.nn.Module, path: os.PathLike, epoch: int, global_step: int) -> Path:
    """Write {"state_dict", "epoch", "global_step"} for `model` to `path` (parent directories created)."""
    path = Path(path)
    path.parent.mkdir(parents=True, exist_ok=True)
    state = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    torch.save({"state_dict": state, "epoch": int(epoch), "global_step": int(global_step)}, path)
    return path


def load_checkpoint(model: torch.nn.Module, path: os.PathLike, strict: bool = True) -> dict:
    """Load `path`'s ["state_dict"] into `model` (torch.load with weights_only=True: no code is unpickled).  Returns
    the whole checkpoint dict.  A file that needs a class the safe loader does not allow fails with that class named."""
    try:
        ckpt = torch.load(Path(path), map_location="cpu", weights_only=True)
    except pickle.UnpicklingError as e:
        raise pickle.UnpicklingError(f"{path}: not loadable with weights_only=True -- {e}") from e
    if not isinstance(ckpt, dict) or "state_dict" not in ckpt:
        raise KeyError(f"{path}: no 'state_dict' entry (not a Lightning-layout checkpoint)")
    model.load_state_dict(ckpt["state_dict"], strict=strict)
    return ckpt
