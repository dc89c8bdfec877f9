"""numpy / Python-integer restatement of patch training's crop, written from the definitions of DESIGN.md section 3 "Patch
training", not from the package (only the Philox block function is shared: utils.augment.philox4x32_10, itself pinned by
tests/augment_ref.py): the yardstick of tests/test_crop_cpu.py and tests/test_gpu_crop.py.

For dataset item `index` in 0-based epoch `epoch` under `seed`: r0..r3 = Philox4x32-10 with key (seed & 2^32 - 1, seed >> 32)
and counter (index, epoch, 4, 0).  With ny = H - size + 1, nx = W - size + 1, n the number of pixels whose label is in
`classes` (only 0..63 can be), T = rint(fg 2^32):
    foreground, iff n > 0 and r0 < T:  k = (r1 n) >> 32, (py, px) the k-th such pixel in raster order, jy = (r2 size) >> 32,
                                       jx = (r3 size) >> 32, oy = clamp(py - jy, 0, ny - 1), ox = clamp(px - jx, 0, nx - 1)
    uniform, otherwise:                oy = (r2 ny) >> 32, ox = (r3 nx) >> 32"""
import numpy as np

CROP_DRAW = 4


def words(seed, epoch, indices):
    """uint32 [n,4]."""
    from unet_amd.utils.augment import philox4x32_10
    idx = np.asarray(list(indices), dtype=np.int64).reshape(-1)
    ctr = np.zeros((idx.size, 4), np.uint32)
    ctr[:, 0] = idx
    ctr[:, 1] = int(epoch)
    ctr[:, 2] = CROP_DRAW
    key = np.array([int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF], np.uint32)
    return philox4x32_10(ctr, key)


def threshold(fg):
    return int(np.rint(float(fg) * 4294967296.0))


def class_mask(classes):
    m = 0
    for c in classes:
        assert 0 <= int(c) <= 63
        m |= 1 << int(c)
    return m


def foreground(labels, mask):
    """Raster-order flat indices of the pixels whose label v lies in 0..63 with bit v of `mask` set."""
    lab = np.asarray(labels).astype(np.int64).reshape(-1)
    ok = (lab >= 0) & (lab < 64)
    bits = np.array([(int(mask) >> v) & 1 for v in range(64)], dtype=bool)
    hit = np.zeros(lab.shape, dtype=bool)
    hit[ok] = bits[lab[ok]]
    return np.flatnonzero(hit)


def select(labels, r, size, mask, T):
    """-> (oy, ox, n, picked): picked = (py, px) on the foreground branch, None on the uniform one.  Python integers."""
    H, W = np.asarray(labels).shape
    assert H >= size and W >= size
    r0, r1, r2, r3 = (int(v) for v in r)
    ny, nx = H - size + 1, W - size + 1
    fg = foreground(labels, mask)
    n = int(fg.size)
    if n > 0 and r0 < int(T):
        k = (r1 * n) >> 32
        py, px = divmod(int(fg[k]), W)
        jy, jx = (r2 * size) >> 32, (r3 * size) >> 32
        return min(max(py - jy, 0), ny - 1), min(max(px - jx, 0), nx - 1), n, (py, px)
    return (r2 * ny) >> 32, (r3 * nx) >> 32, n, None


def crop(image, labels, oy, ox, size):
    """image [C,H,W] (or None), labels [H,W] -> the slices."""
    return (None if image is None else image[:, oy:oy + size, ox:ox + size]), labels[oy:oy + size, ox:ox + size]
