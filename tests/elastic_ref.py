"""numpy restatement of the elastic deformation (csrc/augment.hip: uh_batch_augment_elastic; utils/augment.py:
elastic_table, elastic_weights), written from DESIGN.md section 3 "Elastic deformation", not from the package: the Q20
weight table, the control draws (Philox in Python integers and Box-Muller in float64 from tests/augment_ref.py), the
integer B-spline field, and the sampling from the warped Q16 position q'.  The photometry, the bf16 rounding, the affine
walk and the parameter draws are augment_ref's.

The sampler below asserts that every source index it forms lies inside the image, whatever the control table holds."""
import math

import numpy as np

import augment_ref as AR

Q16, Q20 = 1 << 16, 1 << 20
D_MAX = (1 << 22) - 1                                   # control values are clamped to |d| < 2^22 on load


def grid_shape(H, W, grid):
    """(GH, GW): ceil(n / grid) + 3 control points per axis, point k at (k - 1) grid."""
    return (H + grid - 1) // grid + 3, (W + grid - 1) // grid + 3


def basis(t):
    """The uniform cubic B-spline basis (B0, B1, B2, B3) at t in [0, 1), float64."""
    return ((1 - t) ** 3 / 6, (3 * t ** 3 - 6 * t ** 2 + 4) / 6, (-3 * t ** 3 + 3 * t ** 2 + 3 * t + 1) / 6, t ** 3 / 6)


def weights(grid):
    """[grid][4] Python integers: the basis at (n + 0.5) / grid times 2^20, rounded; the first largest entry of a row
    takes what the row lacks to 2^20."""
    rows = []
    for n in range(grid):
        w = [int(np.rint(b * Q20)) for b in basis((n + 0.5) / grid)]
        w[w.index(max(w))] += Q20 - sum(w)
        rows.append(w)
    return rows


def control_item(grid, sigma, p, seed, epoch, index, noise_key, H, W):
    """int64 [GH, GW, 2]: one item's control displacements in Q16 pixels.  Deformed when word 0 of draw 3 (key = the
    seed, counter (index, epoch, 3, 0)) gives u < p; control point q = ky GW + kx takes normals 2 (q & 1) and
    2 (q & 1) + 1 of the block with the item's noise key and counter (q >> 1, 0, 0, 2)."""
    GH, GW = grid_shape(H, W, grid)
    on = AR.unit(AR.philox((index, epoch, 3, 0), (seed & AR.M32, (seed >> 32) & AR.M32))[0]) < p
    if not on:
        return np.zeros((GH, GW, 2), np.int64)
    n = GH * GW
    words = np.array([AR.philox((j, 0, 0, 2), noise_key) for j in range((n + 1) // 2)], dtype=np.uint64)
    z = AR.normals(words, 2 * n, np.float64).reshape(n, 2)
    return np.rint(np.clip(z, -2.0, 2.0) * sigma * Q16).astype(np.int64).reshape(GH, GW, 2)


def field_q16(control, grid, H, W, wts=None):
    """The integer field (dx, dy), int64 [H, W] each, in Q16 pixels at every OUTPUT pixel:
    r_k = (sum_j w[nx][j] d[cy + k][cx + j] + 2^19) >> 20,  displacement = (sum_k w[ny][k] r_k + 2^19) >> 20."""
    w = np.array(weights(grid) if wts is None else wts, np.int64)
    d = np.clip(np.asarray(control).astype(np.int64), -D_MAX, D_MAX)
    assert d.shape == grid_shape(H, W, grid) + (2,)
    x, y = np.arange(W), np.arange(H)
    cx, nx, cy, ny = x // grid, x % grid, y // grid, y % grid
    half = np.int64(1 << 19)
    out = []
    for c in (0, 1):
        # rows[ky, x] = the row pass of control row ky at column x
        rows = (sum(w[nx, j][None, :] * d[:, cx + j, c] for j in range(4)) + half) >> np.int64(20)
        out.append((sum(w[ny, k][:, None] * rows[cy + k, :] for k in range(4)) + half) >> np.int64(20))
    return out[0], out[1]


def field_f64(control, grid, H, W):
    """The same spline at the pixel centres in float64 from the exact basis, in Q16 pixels (the yardstick of the integer
    field's error bound)."""
    d = np.clip(np.asarray(control).astype(np.float64), -D_MAX, D_MAX)
    x, y = np.arange(W), np.arange(H)
    bx = np.stack(basis((x % grid + 0.5) / grid))                     # [4, W]
    by = np.stack(basis((y % grid + 0.5) / grid))                     # [4, H]
    cx, cy = x // grid, y // grid
    out = []
    for c in (0, 1):
        rows = sum(bx[j][None, :] * d[:, cx + j, c] for j in range(4))
        out.append(sum(by[k][:, None] * rows[cy + k, :] for k in range(4)))
    return out[0], out[1]


def field_error_bound(d_max):
    """Q16 units between field_q16 and the exact spline: a weight row's errors sum to 0 and their magnitudes to
    at most 3 (three roundings of 1/2 and the adjusted entry's 3/2), so a pass errs by at most 3 D 2^-20 plus its own
    rounding of 1/2; the second pass carries the first one's error through a convex combination."""
    return 1.0 + 6.0 * float(d_max) / Q20


def warped_q16(m_q32, control, grid, H, W):
    qx, qy = AR.coords_q16(m_q32, H, W)
    dx, dy = field_q16(control, grid, H, W)
    return qx + dx, qy + dy


def _gather(plane, jy, jx):
    H, W = plane.shape[:2]
    iy, ix = np.clip(jy, 0, H - 1), np.clip(jx, 0, W - 1)
    assert iy.min() >= 0 and iy.max() < H and ix.min() >= 0 and ix.max() < W          # every source index is inside
    return plane[iy, ix]


def labels_from(lab, qx, qy, fill_mode=False, fill_label=1):
    """The label of the pixel that contains the position (qx, qy) (Q16 centre coordinates)."""
    H, W = lab.shape
    lx, ly = qx >> np.int64(16), qy >> np.int64(16)
    out = _gather(lab, ly, lx)
    if fill_mode:
        out = np.where((lx >= 0) & (lx < W) & (ly >= 0) & (ly < H), out, np.int64(fill_label))
    return out


def bilinear_from(img, qx, qy, fill_mode=False, fill_image=0.0):
    """img float32 [H, W, C] sampled at (qx, qy): 16-bit weights, top = p00 + wx (p01 - p00), bot = p10 + wx (p11 - p10),
    v = top + wy (bot - top), one fp32 rounding each; a zero weight takes the pixel itself."""
    img = np.asarray(img, np.float32)
    H, W, _ = img.shape
    ux, uy = qx - np.int64(32768), qy - np.int64(32768)
    ix, iy = ux >> np.int64(16), uy >> np.int64(16)
    fx, fy = ux & np.int64(0xFFFF), uy & np.int64(0xFFFF)
    wx = (fx.astype(np.float32) * np.float32(2.0 ** -16))[..., None]
    wy = (fy.astype(np.float32) * np.float32(2.0 ** -16))[..., None]

    def tap(jy, jx):
        p = _gather(img, jy, jx)
        if fill_mode:
            inside = (jx >= 0) & (jx < W) & (jy >= 0) & (jy < H)
            p = np.where(inside[..., None], p, np.float32(fill_image))
        return p.astype(np.float32)

    p00, p01, p10, p11 = tap(iy, ix), tap(iy, ix + 1), tap(iy + 1, ix), tap(iy + 1, ix + 1)
    zx, zy = (fx == 0)[..., None], (fy == 0)[..., None]
    top = np.where(zx, p00, p00 + wx * (p01 - p00)).astype(np.float32)
    bot = np.where(zx, p10, p10 + wx * (p11 - p10)).astype(np.float32)
    return np.where(zy, top, top + wy * (bot - top)).astype(np.float32)


def augment_item(img, lab, row, control, grid, border="clamp", fill_image=0.0, fill_label=1, dtype=np.float32, bf16=False):
    """One item through the elastic stage: augment_ref.augment_item with q replaced by q' = q + field."""
    fill = border == "fill"
    ref = img if img is not None else lab
    H, W = ref.shape[0], ref.shape[1]
    qx, qy = warped_q16(row["m"], control, grid, H, W)
    out_i = out_l = None
    if img is not None:
        v = bilinear_from(img, qx, qy, fill, fill_image)
        out_i = AR.photometry(v, row["gamma"], row["contrast"], row["brightness"], row["noise_std"], row["key"], dtype)
        if bf16:
            out_i = AR.round_bf16(np.asarray(out_i, np.float32))
    if lab is not None:
        out_l = labels_from(lab, qx, qy, fill, fill_label)
    return out_i, out_l


def jacobian_det(dx, dy):
    """Forward-difference determinant of the map (x + dx, y + dy) (dx, dy in pixels, [H, W]) on the [H-1, W-1] interior."""
    a = 1.0 + (dx[:-1, 1:] - dx[:-1, :-1])
    b = dx[1:, :-1] - dx[:-1, :-1]
    c = dy[:-1, 1:] - dy[:-1, :-1]
    d = 1.0 + (dy[1:, :-1] - dy[:-1, :-1])
    return a * d - b * c


def no_fold_slack(sigma, grid):
    """What the integer formats take from det >= 1 - 8 sigma / grid: each field value is within eps =
    field_error_bound 2^-16 px of the spline through the QUANTISED controls, whose neighbours differ by at most
    4 sigma + 2^-16 px; a difference entry moves by 2 eps, the determinant by (2 + 4 r) 2 eps + 2 (2 eps)^2 <= 8 eps + 8 eps^2."""
    eps = field_error_bound(math.floor(2.0 * sigma * Q16 + 0.5)) / Q16
    return 2.0 * 2.0 ** -16 / grid + 8.0 * eps + 8.0 * eps * eps
