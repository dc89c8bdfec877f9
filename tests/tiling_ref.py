"""numpy / Python-integer restatement of tiled prediction, written from the definitions of DESIGN.md section 3 "Tiled
prediction", not from the package: the yardstick of tests/test_tiling_cpu.py and tests/test_gpu_tiling.py.

Per axis of length L with tile size `size` and `overlap`: tile length t = min(size, L); L <= size: one tile at 0; otherwise
stride S = size - overlap, n = ceil((L - size) / S) + 1 tiles at o_k = min(k S, L - size).  Position i of a tile weighs
w(i) = max(1, min(i + 1, t - i, overlap)).  The merged sum of an image pixel is the sum over the tiles that hold it of
wy wx q, q the tile's quantised value there; den is the sum of wy wx."""
import numpy as np

Q = 1 << 24


def origins(L, size, overlap):
    if L <= size:
        return [0]
    S = size - overlap
    n = -((L - size) // -S) + 1
    return [min(k * S, L - size) for k in range(n)]


def count_formula(L, size, overlap):
    if L <= size:
        return 1
    S = size - overlap
    return (L - size + S - 1) // S + 1


def weights(t, overlap):
    return np.asarray([max(1, min(i + 1, t - i, overlap)) for i in range(t)], dtype=np.uint64)


def grid(H, W, size, overlap):
    oy, ox = origins(H, size, overlap), origins(W, size, overlap)
    return len(oy), len(ox), min(size, H), min(size, W), oy, ox


def gather_ref(x, size, overlap):
    """x [B,H,W,C] -> tiles [B*ny*nx,th,tw,C] by slicing, image-major then row-major over the grid."""
    B, H, W, _ = x.shape
    _, _, th, tw, oy, ox = grid(H, W, size, overlap)
    return np.stack([x[b, y:y + th, xx:xx + tw] for b in range(B) for y in oy for xx in ox])


def merge_ref(q, size_hw, size, overlap):
    """q [B*ny*nx,th,tw,NC] non-negative integers (or float64 for an unrounded reference) -> (sums [B,H,W,NC], den [B,H,W]):
    uint64 sums for integer q, float64 for float q."""
    H, W = size_hw
    ny, nx, th, tw, oy, ox = grid(H, W, size, overlap)
    B = q.shape[0] // (ny * nx)
    NC = q.shape[-1]
    exact = np.issubdtype(q.dtype, np.integer)
    sums = np.zeros((B, H, W, NC), np.uint64 if exact else np.float64)
    den = np.zeros((B, H, W), np.uint64)
    w = np.outer(weights(th, overlap), weights(tw, overlap)).astype(np.uint64)
    n = 0
    for b in range(B):
        for y in oy:
            for x in ox:
                t = q[n].astype(np.uint64) if exact else q[n]
                sums[b, y:y + th, x:x + tw] += (w if exact else w.astype(np.float64))[..., None] * t
                den[b, y:y + th, x:x + tw] += w
                n += 1
    return sums, den


def classes_ref(sums, den, views):
    """The first maximum of the sums; one class: 2 sum > den views 2^24 (Python integers: no overflow to think about)."""
    if sums.shape[-1] == 1:
        s = sums[..., 0].astype(object)
        return (2 * s > den.astype(object) * (views * Q)).astype(np.uint8)
    return sums.argmax(-1).astype(np.uint8)                              # numpy: the first maximum


def probs_ref(sums, den, views):
    """(float)((double) sum / ((double) den views 2^24)); every operand is exact in float64."""
    unit = den.astype(np.float64) * float(views) * float(Q)
    return (sums.astype(np.float64) / unit[..., None]).astype(np.float32)


def probabilities64(logits):
    """float64 softmax over the last axis (one class: the sigmoid)."""
    l = logits.astype(np.float64)
    if l.shape[-1] == 1:
        return 1.0 / (1.0 + np.exp(-l))
    e = np.exp(l - l.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)
