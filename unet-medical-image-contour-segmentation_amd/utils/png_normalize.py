"""Stage 2 of seg_main.py on the device: utils/png_normalize.py (letterbox to 512 x 512 with PIL LANCZOS).

    letterbox_geometry(width, height, target=512) -> (nw, nh, px, py)       png_normalize.py:536-556
    lanczos_coeffs(in_size, out_size) -> (bounds [out][2], coef [out][k])   Pillow Resample.c precompute_coeffs +
                                                                            normalize_coeffs_8bpc (LANCZOS, 8-bit)
    resample_coeffs(in_size, out_size, filter)                              the same for 'lanczos' or 'bicubic' (the
                                                                            dataset rescale, utils/data_rescale.py)
    ResamplePlan(in_w, in_h, out_w, out_h)                                  both passes' tables, on the device, cached
    letterbox(images) -> uint8 [B, 512, 512]                                png_normalize.py:_process_single_image

The tables are host work in float64 (libm sin, as Pillow's C code) done once per geometry; csrc/seg_pipeline.hip only
multiplies and adds the 22-bit integer weights, so the result is Pillow's byte for byte."""
from __future__ import annotations

import math
from functools import lru_cache

import numpy as np
import torch

from .. import ops
from .._lib import LIB

TARGET = 512
PRECISION_BITS = 22
_IDENTITY = np.arange(256, dtype=np.uint8)


def letterbox_geometry(width: int, height: int, target: int = TARGET):
    if width <= 0 or height <= 0:
        raise ValueError(f"bad image size {width}x{height}")
    if width >= height:
        nw, nh = target, int(height * (target / width))
    else:
        nw, nh = int(width * (target / height)), target
    if nw <= 0 or nh <= 0:
        raise ValueError(f"{width}x{height} letterboxes to {nw}x{nh}: an empty image (PIL refuses it too)")
    return nw, nh, (target - nw) // 2, (target - nh) // 2


def _sinc(x: float) -> float:
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x: float) -> float:
    if -3.0 <= x < 3.0:
        return _sinc(x) * _sinc(x / 3)
    return 0.0


def _bicubic(x: float) -> float:
    """Resample.c bicubic_filter, a = -0.5."""
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


FILTERS = {"lanczos": (_lanczos, 3.0), "bicubic": (_bicubic, 2.0)}     # Resample.c: filter function, support


@lru_cache(maxsize=256)
def resample_coeffs(in_size: int, out_size: int, filter: str = "lanczos"):
    """-> (bounds int32 [out][2] = {xmin, taps}, coef int32 [out][ksize]) for the box (0, in_size): Resample.c
    precompute_coeffs + normalize_coeffs_8bpc with `filter` ('lanczos' or 'bicubic')."""
    fn, fsupport = FILTERS[filter]
    scale = float(in_size) / out_size
    filterscale = max(scale, 1.0)
    support = fsupport * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    coef = np.zeros((out_size, ksize), np.int32)
    ss = 1.0 / filterscale
    one = float(1 << PRECISION_BITS)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        k = [fn((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for w in k:
            ww += w
        if ww != 0.0:
            k = [w / ww for w in k]
        coef[xx, :xmax] = [int(-0.5 + w * one) if w < 0 else int(0.5 + w * one) for w in k]
        bounds[xx] = (xmin, xmax)
    return bounds, coef


@lru_cache(maxsize=64)
def lanczos_coeffs(in_size: int, out_size: int):
    """-> (bounds int32 [out][2] = {xmin, taps}, coef int32 [out][ksize]) for the box (0, in_size)."""
    return resample_coeffs(in_size, out_size, "lanczos")


def _identity_coeffs(n: int):
    bounds = np.stack([np.arange(n, dtype=np.int32), np.ones(n, np.int32)], 1)
    return bounds, np.full((n, 1), 1 << PRECISION_BITS, np.int32)


class ResamplePlan:
    """Image.resize((out_w, out_h), LANCZOS) of an in_w x in_h image (Resample.c ImagingResampleInner): a pass whose size
    does not change is the identity (Pillow skips it), the horizontal pass covers only the rows the vertical pass reads."""

    def __init__(self, in_w: int, in_h: int, out_w: int, out_h: int, device):
        self.in_w, self.in_h, self.out_w, self.out_h = in_w, in_h, out_w, out_h
        hb, hc = lanczos_coeffs(in_w, out_w) if out_w != in_w else _identity_coeffs(out_w)
        vb, vc = lanczos_coeffs(in_h, out_h) if out_h != in_h else _identity_coeffs(out_h)
        vb = vb.copy()
        self.row0 = int(vb[0, 0])
        self.nrows = int(vb[-1, 0] + vb[-1, 1]) - self.row0
        vb[:, 0] -= self.row0
        self.kh, self.kv = hc.shape[1], vc.shape[1]
        if self.kh > 128:
            raise ValueError(f"{in_w} -> {out_w} needs a {self.kh}-tap filter; the kernel holds at most 128")
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        self.hb, self.hc, self.vb, self.vc = t(hb), t(hc), t(vb), t(vc)


_PLANS = {}
_LUTS = {}


def resample_plan(in_w, in_h, out_w, out_h, device) -> ResamplePlan:
    key = (torch.device(device), in_w, in_h, out_w, out_h)
    if key not in _PLANS:
        _PLANS[key] = ResamplePlan(in_w, in_h, out_w, out_h, key[0])
    return _PLANS[key]


def device_lut(values, device) -> torch.Tensor:
    key = (torch.device(device), bytes(np.asarray(values, np.uint8)))
    if key not in _LUTS:
        _LUTS[key] = torch.from_numpy(np.asarray(values, np.uint8).copy()).to(device)
    return _LUTS[key]


def resample_into(src: torch.Tensor, box, plan: ResamplePlan, lut: torch.Tensor, dst: torch.Tensor, place=(0, 0)):
    """dst[:, py:py+out_h, px:px+out_w] = LANCZOS resize of src[:, y:y+h, x:x+w] through lut; the rest of dst = 0."""
    ops._require_gpu(src, "src")
    ops._require_gpu(dst, "dst")
    if src.dtype != torch.uint8 or dst.dtype != torch.uint8 or src.dim() != 3 or dst.dim() != 3:
        raise RuntimeError("resample_into takes uint8 [B,H,W] tensors")
    if not (src.is_contiguous() and dst.is_contiguous()) or src.shape[0] != dst.shape[0]:
        raise RuntimeError("resample_into: contiguous tensors of one batch size")
    B, Hs, Ws = src.shape
    _, Hd, Wd = dst.shape
    x, y, w, h = box
    if (w, h) != (plan.in_w, plan.in_h):
        raise RuntimeError(f"box {w}x{h} does not match the plan's {plan.in_w}x{plan.in_h}")
    nbytes = LIB.query("uh_resample_ws_bytes", B, plan.nrows, plan.out_w)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=src.device)
    LIB.call("uh_resample_lanczos_u8", src.data_ptr(), B, Hs, Ws, x, y, w, h, lut.data_ptr(), plan.hb.data_ptr(),
             plan.hc.data_ptr(), plan.kh, plan.out_w, plan.vb.data_ptr(), plan.vc.data_ptr(), plan.kv, plan.out_h, plan.row0,
             plan.nrows, dst.data_ptr(), Hd, Wd, place[0], place[1], ws.data_ptr(), nbytes, ops._stream())
    return dst


def letterbox(images: torch.Tensor, target: int = TARGET) -> torch.Tensor:
    """uint8 [B,H,W] (or [H,W]) on the GPU -> the 512 x 512 canvases png_normalize.py writes."""
    ops._require_gpu(images, "images")
    squeeze = images.dim() == 2
    src = (images.unsqueeze(0) if squeeze else images).contiguous()
    B, H, W = src.shape
    nw, nh, px, py = letterbox_geometry(W, H, target)
    out = torch.empty(B, target, target, dtype=torch.uint8, device=src.device)
    resample_into(src, (0, 0, W, H), resample_plan(W, H, nw, nh, src.device), device_lut(_IDENTITY, src.device), out, (px, py))
    return out.squeeze(0) if squeeze else out
