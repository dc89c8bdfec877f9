"""Host restatement of what BasicDataset does at scale < 1 with Pillow (data_loading.py:66-70, 100-121), written from
Pillow's C sources, independent of the package:

    bicubic_coeffs(in_size, out_size)    Resample.c precompute_coeffs (bicubic_filter, a = -0.5, support 2) +
                                         normalize_coeffs_8bpc (22-bit taps)
    resample_bicubic_u8(img, out_w, out_h)  ImagingResampleInner for 8-bit images: horizontal pass over the rows the
                                         vertical pass reads, clip8 to uint8, vertical pass; a pass whose size does not
                                         change is skipped; every channel uses the same taps
    nearest_map(in_size, out_size)       Geometry.c ImagingScaleAffine: xo = a0 / 2; idx = int(xo); xo += a0 (double)
    resize_nearest_u8(img, out_w, out_h)
    quarter_turn(arr, t)                 Image.transpose(ROTATE_90 * t): t quarter turns counter-clockwise
    dataset_rescale(img, mask, t, s)     (_rescaled(_quarter_turn(img, t), s, BICUBIC), ... NEAREST)
"""
import math
from functools import lru_cache

import numpy as np

PRECISION_BITS = 22


def _bicubic(x):
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


@lru_cache(maxsize=None)
def bicubic_coeffs(in_size, out_size):
    scale = filterscale = float(in_size) / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    kk = np.zeros((out_size, ksize), np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        ss = 1.0 / filterscale
        xmin = int(center - support + 0.5)
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > in_size:
            xmax = in_size
        xmax -= xmin
        k = []
        ww = 0.0
        for x in range(xmax):
            w = _bicubic((x + xmin - center + 0.5) * ss)
            k.append(w)
            ww += w
        for x in range(xmax):
            if ww != 0.0:
                k[x] /= ww
        for x in range(xmax):
            v = k[x] * (1 << PRECISION_BITS)
            kk[xx, x] = int(-0.5 + v) if k[x] < 0 else int(0.5 + v)
        bounds[xx] = (xmin, xmax)
    return bounds, kk


def _clip8(acc):
    return np.where(acc >= (256 << PRECISION_BITS), 255, np.where(acc <= 0, 0, acc >> PRECISION_BITS)).astype(np.uint8)


def _pass(a, bounds, kk, axis):
    """One 8bpc pass along `axis` of an int64 [H, W, C] array."""
    a = np.moveaxis(a, axis, 0)
    n = a.shape[0]
    j = np.arange(kk.shape[1])
    idx = np.minimum(bounds[:, :1] + j[None, :], n - 1)                     # [out, k] (taps past xmax weigh 0)
    w = np.where(j[None, :] < bounds[:, 1:2], kk, 0).astype(np.int64)
    acc = np.full((bounds.shape[0],) + a.shape[1:], 1 << (PRECISION_BITS - 1), np.int64)
    for t in range(kk.shape[1]):
        acc += a[idx[:, t]] * w[:, t, None, None]
    return np.moveaxis(_clip8(acc).astype(np.int64), 0, axis)


def resample_bicubic_u8(img, out_w, out_h):
    a = img[..., None] if img.ndim == 2 else img
    H, W = a.shape[:2]
    a = a.astype(np.int64)
    vb, vk = bicubic_coeffs(H, out_h)
    if out_w != W:
        first, last = int(vb[0, 0]), int(vb[-1, 0] + vb[-1, 1])
        hb, hk = bicubic_coeffs(W, out_w)
        a = _pass(a[first:last], hb, hk, 1)
        vb = vb.copy()
        vb[:, 0] -= first
    if out_h != H:
        a = _pass(a, vb, vk, 0)
    a = a.astype(np.uint8)
    return a[..., 0] if img.ndim == 2 else a


@lru_cache(maxsize=None)
def nearest_map(in_size, out_size):
    a0 = float(in_size) / out_size
    xo = a0 * 0.5
    out = []
    for _ in range(out_size):
        out.append(-1 if xo < 0.0 else int(xo))
        xo += a0
    return np.array(out, np.int64)


def resize_nearest_u8(img, out_w, out_h):
    H, W = img.shape[:2]
    return img[nearest_map(H, out_h)][:, nearest_map(W, out_w)]


def quarter_turn(arr, t):
    return np.ascontiguousarray(np.rot90(arr, t % 4, axes=(0, 1)))


def dataset_rescale(img, mask, turns, scale):
    img, mask = quarter_turn(img, turns), quarter_turn(mask, turns)
    H, W = img.shape[:2]
    ow, oh = int(scale * W), int(scale * H)
    assert min(ow, oh) > 0
    return resample_bicubic_u8(img, ow, oh), resize_nearest_u8(mask, ow, oh)
