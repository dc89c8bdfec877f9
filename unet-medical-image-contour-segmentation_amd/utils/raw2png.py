"""Stage 1 of seg_main.py on the device: utils/raw2png.py (window / level of a 16-bit RAW to uint8).

    read_raw(path, width, height) -> np.uint16 [H, W]             raw2png.py:_read_16bit_raw (wrong size refused)
    window_bounds(window_width, window_length) -> (mn, mx)         raw2png.py:_apply_windowing:906-907
    window_level(raw, window_width, window_length) -> uint8        raw2png.py:_apply_windowing (csrc/seg_pipeline.hip)

`raw` is a GPU tensor of any shape holding uint16 codes (torch.uint16, or int16 / uint16 bits reinterpreted).  The result is
bit-exact with the reference's numpy 1.26 arithmetic: trunc(float64(clip(x, mn, mx) - mn) / float64(mx - mn) * 255)."""
from __future__ import annotations

import os

import numpy as np
import torch

from .. import ops
from .._lib import LIB


def read_raw(path: str, width: int, height: int) -> np.ndarray:
    """Little-endian uint16 [height][width]; a file of any other size is refused (the reference's reshape raises)."""
    size = os.path.getsize(path)
    if size != 2 * width * height:
        raise ValueError(f"{path}: {size} bytes, expected {2 * width * height} for {width}x{height} uint16")
    return np.fromfile(path, dtype="<u2").reshape(height, width)


def window_bounds(window_width: int, window_length: int):
    ww, wl = int(window_width), int(window_length)
    if ww < 2:
        raise ValueError(f"window width {ww} < 2: the window is empty (the reference divides 0 by 0)")
    return wl - ww // 2, wl + ww // 2


def window_level(raw: torch.Tensor, window_width: int, window_length: int) -> torch.Tensor:
    ops._require_gpu(raw, "raw")
    window_bounds(window_width, window_length)
    if raw.element_size() != 2 or raw.is_floating_point():
        raise RuntimeError(f"raw must hold 16-bit integer codes, got {raw.dtype}")
    src = raw.contiguous()
    out = torch.empty(src.shape, dtype=torch.uint8, device=src.device)
    LIB.call("uh_window_u16", src.data_ptr(), src.numel(), int(window_length), int(window_width), out.data_ptr(), ops._stream())
    return out
