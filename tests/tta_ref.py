"""numpy restatement of test-time augmentation, written from the definitions of DESIGN.md section 3 "Test-time augmentation",
not from the package: the yardstick of tests/test_tta_cpu.py and tests/test_gpu_tta.py.

A view is v = 4 t + 2 fy + fx, "flip, then transpose":
    t = 0: view[i][j] = x[H-1-i if fy else i][W-1-j if fx else j]         (H x W)
    t = 1: view[i][j] = x[H-1-j if fy else j][W-1-i if fx else i]         (W x H)
A mode is a set of views."""
import numpy as np

MODE_VIEWS = {"hflip": (0, 1), "flips": (0, 1, 2, 3), "rot4": (0, 3, 5, 6), "d4": (0, 1, 2, 3, 4, 5, 6, 7)}
Q = float(1 << 24)


def mode_views(mode):
    return MODE_VIEWS[mode]


def view_ref(a, v):
    """View v of an array whose first two axes are (H, W)."""
    if v & 2:
        a = a[::-1]
    if v & 1:
        a = a[:, ::-1]
    if v & 4:
        a = np.swapaxes(a, 0, 1)
    return np.ascontiguousarray(a)


def position_ref(v, H, W, y, x):
    """Where source pixel (y, x) lies in view v."""
    yy = H - 1 - y if v & 2 else y
    xx = W - 1 - x if v & 1 else x
    return (xx, yy) if v & 4 else (yy, xx)


def views_ref(x, mode):
    """x [B,H,W,C] -> (views0 [K0*B,H,W,C], views1 [K1*B,W,H,C]), view-major in ascending v (an empty array when K = 0)."""
    B, H, W, C = x.shape
    v0 = [view_ref(x[b], v) for v in mode_views(mode) if v < 4 for b in range(B)]
    v1 = [view_ref(x[b], v) for v in mode_views(mode) if v >= 4 for b in range(B)]
    a0 = np.stack(v0) if v0 else np.zeros((0, H, W, C), x.dtype)
    a1 = np.stack(v1) if v1 else np.zeros((0, W, H, C), x.dtype)
    return a0, a1


def compose_table(H, W):
    """The position map of every view on an H x W grid, as a tuple: (view shape, flat target of every source pixel)."""
    maps = {}
    for v in range(8):
        shape = (W, H) if v & 4 else (H, W)
        maps[v] = (shape, tuple(position_ref(v, H, W, y, x) for y in range(H) for x in range(W)))
    return maps


def probabilities64(logits):
    """float64 softmax over the last axis (one class: the sigmoid)."""
    l = logits.astype(np.float64)
    if l.shape[-1] == 1:
        return 1.0 / (1.0 + np.exp(-l))
    e = np.exp(l - l.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def merge_ref(logits0, logits1, mode, size):
    """logits0 [K0*B,H,W,NC], logits1 [K1*B,W,H,NC] (or None) -> S64 [B,H,W,NC] = sum over the views of p64 * 2^24 at the
    position of every source pixel, unrounded."""
    H, W = size
    views = mode_views(mode)
    k0 = sum(1 for v in views if v < 4)
    B = logits0.shape[0] // k0
    NC = logits0.shape[-1]
    S = np.zeros((B, H, W, NC), np.float64)
    yy, xx = np.mgrid[0:H, 0:W]
    i0 = i1 = 0
    for v in views:
        fy = H - 1 - yy if v & 2 else yy
        fx = W - 1 - xx if v & 1 else xx
        if v & 4:
            p = probabilities64(logits1[i1 * B:(i1 + 1) * B])
            S += p[:, fx, fy] * Q
            i1 += 1
        else:
            p = probabilities64(logits0[i0 * B:(i0 + 1) * B])
            S += p[:, fy, fx] * Q
            i0 += 1
    return S
