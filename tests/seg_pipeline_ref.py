"""CPU restatements of the reference's seg_main.py stages, for the tests (not product code):

    window_ref       raw2png.py:_apply_windowing with numpy 1.26's arithmetic, restated without np.clip on uint16
    resize_ref       Pillow Resample.c LANCZOS for mode L (precompute_coeffs, normalize_coeffs_8bpc, both 8-bit passes)
    letterbox_ref / unletterbox_ref   png_normalize.py / png_denormalize.py on top of resize_ref
    contours_ref     OpenCV icvFetchContour (CHAIN_APPROX_SIMPLE) on the raster-first pixel of every external
                     8-connected component, list in reverse discovery order (cvInsertNodeIntoTree)
"""
from __future__ import annotations

import math

import numpy as np

# ------------------------------------------------------------------ stage 1
def window_ref(raw: np.ndarray, window_width: int, window_length: int) -> np.ndarray:
    if window_width < 2:
        raise ValueError("empty window")
    mn = window_length - window_width // 2
    mx = window_length + window_width // 2
    c = np.minimum(np.maximum(raw.astype(np.int64), mn), mx)
    return ((c - mn).astype(np.float64) / np.float64(mx - mn) * 255.0).astype(np.uint8)


# ------------------------------------------------------------------ Pillow LANCZOS, 8 bits
def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x):
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


def coeffs_ref(in_size, in0, in1, out_size):
    scale = float(in1 - in0) / out_size
    fs = max(scale, 1.0)
    support = 3.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int64)
    kk = np.zeros((out_size, ksize), np.int64)
    for xx in range(out_size):
        center = in0 + (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [_lanczos((x + xmin - center + 0.5) * (1.0 / fs)) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        kk[xx, :xmax] = [int(-0.5 + v * (1 << 22)) if v < 0 else int(0.5 + v * (1 << 22)) for v in w]
        bounds[xx] = (xmin, xmax)
    return bounds, kk


def _clip8(acc):
    return np.clip(acc >> 22, 0, 255).astype(np.uint8)


def resize_ref(img: np.ndarray, size) -> np.ndarray:
    """Image.fromarray(img, 'L').resize(size, Image.LANCZOS), restated."""
    H, W = img.shape
    ow, oh = size
    if (ow, oh) == (W, H):
        return img.copy()
    hb, hk = coeffs_ref(W, 0.0, W, ow)
    vb, vk = coeffs_ref(H, 0.0, H, oh)
    src = img.astype(np.int64)
    y0, y1 = int(vb[0, 0]), int(vb[-1, 0] + vb[-1, 1])
    if ow != W:
        rows = src[y0:y1]
        tmp = np.full((rows.shape[0], ow), 1 << 21, np.int64)
        for xx in range(ow):
            xmin, n = hb[xx]
            tmp[:, xx] += rows[:, xmin:xmin + n] @ hk[xx, :n]
        src = _clip8(tmp).astype(np.int64)
        vb = vb.copy()
        vb[:, 0] -= y0
    if oh == H:
        return src.astype(np.uint8)
    out = np.full((oh, src.shape[1]), 1 << 21, np.int64)
    for yy in range(oh):
        ymin, n = vb[yy]
        out[yy] += vk[yy, :n] @ src[ymin:ymin + n]
    return _clip8(out)


def geometry_ref(W, H, target=512):
    if W >= H:
        nw, nh = target, int(H * (target / W))
    else:
        nw, nh = int(W * (target / H)), target
    if nw == 0 or nh == 0:
        raise ValueError("empty letterbox")
    return nw, nh, (target - nw) // 2, (target - nh) // 2


def letterbox_ref(img, target=512):
    H, W = img.shape
    nw, nh, px, py = geometry_ref(W, H, target)
    out = np.zeros((target, target), np.uint8)
    out[py:py + nh, px:px + nw] = resize_ref(img, (nw, nh))
    return out


def unletterbox_ref(canvas, W, H, target=512):
    nw, nh, px, py = geometry_ref(W, H, target)
    return resize_ref(np.ascontiguousarray(canvas[py:py + nh, px:px + nw]), (W, H))


# ------------------------------------------------------------------ stage 5
_DX = (1, 1, 0, -1, -1, -1, 0, 1)
_DY = (0, -1, -1, -1, 0, 1, 1, 1)


def contours_ref(binary: np.ndarray):
    """cv2.findContours(binary, RETR_EXTERNAL, CHAIN_APPROX_SIMPLE), squeezed to int32 [n, 2], restated."""
    from scipy import ndimage
    f = np.pad(np.asarray(binary) != 0, 1)
    H, W = binary.shape
    bg, _ = ndimage.label(~f, structure=[[0, 1, 0], [1, 1, 1], [0, 1, 0]])
    outside = bg == bg[0, 0]                                       # background 4-connected to the frame
    lab, n = ndimage.label(f, structure=np.ones((3, 3), int))
    if n == 0:
        return []
    flat = lab.ravel()
    _, first = np.unique(flat, return_index=True)
    starts = sorted(int(p) for p, l in zip(first, _) if l != 0)
    PW = W + 2
    out = []
    for p in starts:
        y, x = divmod(p, PW)
        if not outside[y, x - 1]:
            continue
        out.append(_trace(f, x, y))
    return [np.asarray(c, np.int32).reshape(-1, 2) - 1 for c in reversed(out)]


def _trace(f, x0, y0):
    s = 4
    while True:
        s = (s - 1) & 7
        if f[y0 + _DY[s], x0 + _DX[s]] or s == 4:
            break
    if s == 4 and not f[y0 + _DY[4], x0 + _DX[4]]:
        return [(x0, y0)]
    x1, y1 = x0 + _DX[s], y0 + _DY[s]
    prev_s = s ^ 4
    x3, y3 = x0, y0
    pts = []
    while True:
        for k in range(1, 9):
            t = (s + k) & 7
            if f[y3 + _DY[t], x3 + _DX[t]]:
                break
        s = t
        if s != prev_s:
            pts.append((x3, y3))
            prev_s = s
        x4, y4 = x3 + _DX[s], y3 + _DY[s]
        if (x4, y4) == (x0, y0) and (x3, y3) == (x1, y1):
            return pts
        x3, y3 = x4, y4
        s = (s + 4) & 7
