"""The dataset's rotate + rescale at scale < 1 on the device (csrc/data_rescale.hip, `uh_batch_rescale_u8`): what
BasicDataset does with Pillow (/root/reference/utils/data_loading.py:66-70, 100-121), byte for byte:

    image = _rescaled(_quarter_turn(img, t), s, BICUBIC)     Resample.c ImagingResample, 8-bit, two passes
    mask  = _rescaled(_quarter_turn(mask, t), s, NEAREST)    Geometry.c ImagingScaleAffine

    rescaled_size(h, w, scale) -> (out_h, out_w)              data_loading.py:66-70 (int() of each side, PIL's (w, h) order)
    nearest_index(in_size, out_size) -> int32 [out_size]      ImagingScaleAffine's running double sum
    RescalePlan / rescale_plan(Hr, Wr, out_h, out_w, device)  both filters' tables on the device, cached per geometry
    batch_rescale(image_u8, mask_u8, turns, scale)            uint8 device batches -> rotated, rescaled uint8 device batches

The tables are host work in float64 done once per (size, scale); the kernels only index, multiply and add."""
from __future__ import annotations

from functools import lru_cache

import numpy as np
import torch

from .. import ops
from .._lib import LIB
from .png_normalize import PRECISION_BITS, resample_coeffs

RB_TX = 64                       # output columns per horizontal workgroup (csrc/data_rescale.hip)


def rescaled_size(h: int, w: int, scale: float):
    """(out_h, out_w) of `_rescaled` on an h x w image; refuses an empty result like the reference's assert."""
    out_w, out_h = int(scale * w), int(scale * h)
    if min(out_w, out_h) <= 0:
        raise ValueError("Scale is too small, resized images would have no pixel")
    return out_h, out_w


@lru_cache(maxsize=256)
def nearest_index(in_size: int, out_size: int) -> np.ndarray:
    """Source index of every output pixel of Pillow's NEAREST resize along one axis: `a0 = in / out; xo = a0 * 0.5;
    idx[x] = int(xo); xo += a0` in double precision, the accumulation of ImagingScaleAffine (neither floor((x + 0.5) * a0)
    nor a fixed-point form gives the same indices for every size)."""
    a0 = float(in_size) / out_size
    xo = a0 * 0.5
    idx = np.empty(out_size, np.int32)
    for x in range(out_size):
        idx[x] = -1 if xo < 0.0 else int(xo)
        xo += a0
    if idx.min() < 0 or idx.max() >= in_size:
        raise ValueError(f"nearest_index({in_size}, {out_size}): index outside the source")
    return idx


def _identity_coeffs(n: int):
    bounds = np.stack([np.arange(n, dtype=np.int32), np.ones(n, np.int32)], 1)
    return bounds, np.full((n, 1), 1 << PRECISION_BITS, np.int32)


def _span(bounds: np.ndarray) -> int:
    """Widest source window any RB_TX consecutive output columns (one horizontal workgroup) read."""
    n = bounds.shape[0]
    first = np.arange(0, n, RB_TX)
    last = np.minimum(first + RB_TX, n) - 1
    return int((bounds[last, 0] + bounds[last, 1] - bounds[first, 0]).max())


class RescalePlan:
    """Image.resize((out_w, out_h), BICUBIC / NEAREST) of an Hr x Wr (rotated) image: a pass whose size does not change is
    the identity (Pillow skips it), the horizontal pass covers only the rows the vertical pass reads."""

    def __init__(self, Hr: int, Wr: int, out_h: int, out_w: int, device):
        self.Hr, self.Wr, self.out_h, self.out_w = Hr, Wr, out_h, out_w
        hb, hc = resample_coeffs(Wr, out_w, "bicubic") if out_w != Wr else _identity_coeffs(out_w)
        vb, vc = resample_coeffs(Hr, out_h, "bicubic") if out_h != Hr else _identity_coeffs(out_h)
        vb = vb.copy()
        self.row0 = int(vb[0, 0])
        self.nrows = int(vb[-1, 0] + vb[-1, 1]) - self.row0
        vb[:, 0] -= self.row0
        self.kh, self.kv = hc.shape[1], vc.shape[1]
        self.span = _span(hb)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(device)
        self.hb, self.hc, self.vb, self.vc = t(hb), t(hc), t(vb), t(vc)
        self.xi, self.yi = t(nearest_index(Wr, out_w)), t(nearest_index(Hr, out_h))


_PLANS = {}


def rescale_plan(Hr: int, Wr: int, out_h: int, out_w: int, device) -> RescalePlan:
    key = (torch.device(device), Hr, Wr, out_h, out_w)
    if key not in _PLANS:
        _PLANS[key] = RescalePlan(Hr, Wr, out_h, out_w, key[0])
    return _PLANS[key]


def batch_rescale(image_u8, mask_u8, turns_d, odd: int, scale: float):
    """uint8 DEVICE batches [B,H,W,C] (C = 1 or 3) / [B,H,W] (either may be None), turns_d a DEVICE int32 [B] table or None,
    odd = 1 when every item turns an odd number of times -> (image [B,Ho,Wo,C], mask [B,Ho,Wo]) rotated and rescaled."""
    src = image_u8 if image_u8 is not None else mask_u8
    ops._require_gpu(src, "image_u8 / mask_u8")
    B, H, W = src.shape[:3]
    C = int(image_u8.shape[3]) if image_u8 is not None else 1
    Hr, Wr = (W, H) if odd else (H, W)
    out_h, out_w = rescaled_size(Hr, Wr, scale)
    plan = rescale_plan(Hr, Wr, out_h, out_w, src.device)
    img_o = msk_o = ws = None
    nbytes = 0
    if image_u8 is not None:
        img_o = torch.empty((B, out_h, out_w, C), dtype=torch.uint8, device=src.device)
        nbytes = LIB.query("uh_batch_rescale_ws_bytes", B, C, plan.nrows, out_w)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=src.device)
    if mask_u8 is not None:
        msk_o = torch.empty((B, out_h, out_w), dtype=torch.uint8, device=src.device)
    ptr = lambda t: None if t is None else t.data_ptr()
    LIB.call("uh_batch_rescale_u8", ptr(image_u8), C, ptr(mask_u8), ptr(turns_d), odd, B, H, W, plan.hb.data_ptr(),
             plan.hc.data_ptr(), plan.kh, plan.span, out_w, plan.vb.data_ptr(), plan.vc.data_ptr(), plan.kv, out_h, plan.row0,
             plan.nrows, plan.xi.data_ptr(), plan.yi.data_ptr(), ptr(img_o), ptr(msk_o), ptr(ws), nbytes, ops._stream())
    return img_o, msk_o
