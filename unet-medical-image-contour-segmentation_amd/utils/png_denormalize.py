"""Stage 4 of seg_main.py on the device: utils/png_denormalize.py (crop the letterbox, PIL LANCZOS back to the original
size), csrc/seg_pipeline.hip.

    unletterbox(canvas, width, height, lut=None) -> uint8 [B, height, width]     png_denormalize.py:_process_single_image

`lut` maps each canvas byte before the resample: None = identity (a grey mask, as the reference reads it), or e.g.
CLASS_TO_GREY to resample a class map as predict.py:mask_to_image would have drawn it (0 / 128 / 255)."""
from __future__ import annotations

import numpy as np
import torch

from .. import ops
from .png_normalize import TARGET, _IDENTITY, device_lut, letterbox_geometry, resample_into, resample_plan

CLASS_TO_GREY = np.zeros(256, np.uint8)
CLASS_TO_GREY[1], CLASS_TO_GREY[2] = 128, 255


def unletterbox(canvas: torch.Tensor, width: int, height: int, lut=None, target: int = TARGET) -> torch.Tensor:
    ops._require_gpu(canvas, "canvas")
    squeeze = canvas.dim() == 2
    src = (canvas.unsqueeze(0) if squeeze else canvas).contiguous()
    if tuple(src.shape[1:]) != (target, target):
        raise RuntimeError(f"canvas must be {target}x{target}, got {tuple(src.shape[1:])}")
    nw, nh, px, py = letterbox_geometry(width, height, target)     # png_denormalize.py:740-751 (same offsets)
    out = torch.empty(src.shape[0], height, width, dtype=torch.uint8, device=src.device)
    lut_t = device_lut(_IDENTITY if lut is None else lut, src.device)
    resample_into(src, (px, py, nw, nh), resample_plan(nw, nh, width, height, src.device), lut_t, out, (0, 0))
    return out.squeeze(0) if squeeze else out
