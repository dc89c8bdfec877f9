"""numpy restatement of the training augmentation (csrc/augment.hip + utils/augment.py), written from DESIGN.md section 3
"Training augmentation", not from the package: Philox4x32-10 in Python integers, the parameter draws, the Q32 matrix, the
integer coordinate walk, the fp32 interpolation in the documented order (np.float32 operations, one rounding each), the
nearest labels and the photometry.

`augment(...)` computes the photometry in `dtype`: np.float32 restates the device's contrast / brightness / clamp bit for
bit (plain IEEE operations); np.float64 is the yardstick's exact side for gamma (powf) and noise (logf / cosf / sinf),
which no two libms evaluate alike."""
import math

import numpy as np

M32 = 0xFFFFFFFF
TWO32 = 4294967296.0


def philox(counter, key):
    """Philox4x32-10 on Python integers: (c0, c1, c2, c3), (k0, k1) -> four 32-bit words."""
    c0, c1, c2, c3 = (int(c) & M32 for c in counter)
    k0, k1 = (int(k) & M32 for k in key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def unit(word):
    return (word + 0.5) / TWO32


def draw_item(cfg, seed, epoch, index, H, W):
    """One item's drawn values: counter (index, epoch, draw, 0), key (seed low word, seed high word).  `cfg` is any
    object with the AugmentConfig fields."""
    key = (seed & M32, (seed >> 32) & M32)
    d0, d1, d2 = (philox((index, epoch, d, 0), key) for d in range(3))
    sym = lambda w: 2.0 * unit(w) - 1.0
    return {
        "hflip": unit(d0[0]) < cfg.p_hflip, "vflip": unit(d0[1]) < cfg.p_vflip,
        "theta_deg": sym(d0[2]) * cfg.rotate_deg if cfg.rotate_deg else 0.0,
        "scale": 1.0 + sym(d0[3]) * cfg.scale if cfg.scale else 1.0,
        "tx": sym(d1[0]) * (cfg.translate * W) if cfg.translate else 0.0,
        "ty": sym(d1[1]) * (cfg.translate * H) if cfg.translate else 0.0,
        "brightness": sym(d1[2]) * cfg.brightness if cfg.brightness else 0.0,
        "contrast": 1.0 + sym(d1[3]) * cfg.contrast if cfg.contrast else 1.0,
        "gamma": math.exp(sym(d2[0]) * math.log1p(cfg.gamma)) if cfg.gamma else 1.0,
        "noise_std": float(cfg.noise_std), "key": (d2[1], d2[2]),
    }


def matrix(d, H, W):
    """The unquantised inverse map [2, 3] in pixel-centre coordinates: source = A (out - centre - t) + centre with
    A = F R(-theta) / s."""
    fx, fy = (-1.0 if d["hflip"] else 1.0), (-1.0 if d["vflip"] else 1.0)
    th = math.radians(d["theta_deg"])
    cs, sn = (math.cos(th), math.sin(th)) if d["theta_deg"] != 0 else (1.0, 0.0)
    s = d["scale"]
    a00, a01, a10, a11 = fx * cs / s, fx * sn / s, -fy * sn / s, fy * cs / s
    cx, cy = W / 2.0, H / 2.0
    px, py = cx + d["tx"], cy + d["ty"]
    return np.array([[a00, a01, cx - (a00 * px + a01 * py)], [a10, a11, cy - (a10 * px + a11 * py)]], np.float64)


def q32(m):
    return [int(np.rint(v * TWO32)) for v in np.asarray(m, np.float64).reshape(6)]


def coords_q16(m_q32, H, W):
    """Q16 source centre coordinates (qx, qy), int64 [H, W]:  (m0 (2x+1) + m1 (2y+1) + 2 m2 + 2^16) >> 17."""
    x2 = (2 * np.arange(W, dtype=np.int64) + 1)[None, :]
    y2 = (2 * np.arange(H, dtype=np.int64) + 1)[:, None]
    q = []
    for a, b, c in (m_q32[0:3], m_q32[3:6]):
        s = np.int64(a) * x2 + np.int64(b) * y2 + np.int64(2 * c)
        q.append((s + np.int64(65536)) >> np.int64(17))
    return q[0], q[1]


def labels_nearest(lab, m_q32, fill_mode=False, fill_label=1):
    """lab int64 [H, W] -> the label of the pixel that contains the source position (floor of the centre coordinate)."""
    H, W = lab.shape
    qx, qy = coords_q16(m_q32, H, W)
    lx, ly = qx >> np.int64(16), qy >> np.int64(16)
    out = lab[np.clip(ly, 0, H - 1), np.clip(lx, 0, W - 1)]
    if fill_mode:
        out = np.where((lx >= 0) & (lx < W) & (ly >= 0) & (ly < H), out, np.int64(fill_label))
    return out


def bilinear_f32(img, m_q32, fill_mode=False, fill_image=0.0):
    """img float32 [H, W, C] -> float32 [H, W, C]: top = p00 + wx (p01 - p00), bot = p10 + wx (p11 - p10),
    v = top + wy (bot - top), every operation rounded to fp32 once; a zero weight takes the pixel itself."""
    img = np.asarray(img, np.float32)
    H, W, _ = img.shape
    qx, qy = coords_q16(m_q32, H, W)
    ux, uy = qx - np.int64(32768), qy - np.int64(32768)
    ix, iy = ux >> np.int64(16), uy >> np.int64(16)
    fx, fy = ux & np.int64(0xFFFF), uy & np.int64(0xFFFF)
    wx = (fx.astype(np.float32) * np.float32(2.0 ** -16))[..., None]
    wy = (fy.astype(np.float32) * np.float32(2.0 ** -16))[..., None]

    def tap(jy, jx):
        p = img[np.clip(jy, 0, H - 1), np.clip(jx, 0, W - 1)]
        if fill_mode:
            inside = (jx >= 0) & (jx < W) & (jy >= 0) & (jy < H)
            p = np.where(inside[..., None], p, np.float32(fill_image))
        return p.astype(np.float32)

    p00, p01, p10, p11 = tap(iy, ix), tap(iy, ix + 1), tap(iy + 1, ix), tap(iy + 1, ix + 1)
    zx, zy = (fx == 0)[..., None], (fy == 0)[..., None]
    top = np.where(zx, p00, p00 + wx * (p01 - p00)).astype(np.float32)
    bot = np.where(zx, p10, p10 + wx * (p11 - p10)).astype(np.float32)
    return np.where(zy, top, top + wy * (bot - top)).astype(np.float32)


def noise_words(key, n_elements):
    """uint32 [ceil(n / 4), 4]: block j has counter (j, 0, 0, 1)."""
    return np.array([philox((j, 0, 0, 1), key) for j in range((n_elements + 3) // 4)], dtype=np.uint64)


def normals(words, n_elements, dtype=np.float64):
    """Normal number of every element e = 0 .. n-1: block e >> 2, number e & 3; words (0, 1) and (2, 3) are Box-Muller
    pairs, radius from u = (r + 0.5) 2^-32, angle 2 pi r 2^-32, cosine first, then sine.  Evaluated in `dtype`."""
    t = dtype
    w = words.astype(t)
    z = np.empty((words.shape[0], 4), t)
    for p in (0, 2):
        u = (w[:, p] + t(0.5)) * t(2.0 ** -32)
        v = w[:, p + 1] * t(2.0 ** -32)
        rad = np.sqrt(t(-2.0) * np.log(u))
        ang = t(2.0 * math.pi) * v
        z[:, p], z[:, p + 1] = rad * np.cos(ang), rad * np.sin(ang)
    return z.reshape(-1)[:n_elements]


def photometry(v, gamma, contrast, brightness, noise_std, key, dtype=np.float64, z=None):
    """v [H, W, C] after the geometry -> gamma, contrast about 0.5, brightness, noise, clamp, in this order, in `dtype`;
    the scalars are the fp32 values of the parameter table; neutral stages are skipped (all neutral: v unchanged)."""
    t = dtype
    g, c, b, s = (np.float32(p) for p in (gamma, contrast, brightness, noise_std))
    if g == 1 and c == 1 and b == 0 and s == 0:
        return v
    x = np.asarray(v, np.float32).astype(t)
    if g != 1:
        x = np.power(np.clip(x, t(0), t(1)), t(g))
    if c != 1:
        x = (x - t(0.5)) * t(c) + t(0.5)
    if b != 0:
        x = x + t(b)
    if s != 0:
        n = x.size
        zz = normals(noise_words(key, n), n, t) if z is None else z
        x = x + t(s) * zz.reshape(x.shape).astype(t)
    return np.clip(x, t(0), t(1))


def augment_item(img, lab, row, border="clamp", fill_image=0.0, fill_label=1, dtype=np.float32, bf16=False):
    """One item through the whole stage.  img float32 [H, W, C] (bf16 inputs already widened) or None, lab int64 [H, W] or
    None, row: {'m': six Q32 ints, 'gamma', 'contrast', 'brightness', 'noise_std', 'key'}.  Returns (image in `dtype`, or
    rounded to bf16 and widened when bf16=True; labels)."""
    fill = border == "fill"
    out_i = out_l = None
    if img is not None:
        v = bilinear_f32(img, row["m"], fill, fill_image)
        out_i = photometry(v, row["gamma"], row["contrast"], row["brightness"], row["noise_std"], row["key"], dtype)
        if bf16:
            out_i = round_bf16(np.asarray(out_i, np.float32))
    if lab is not None:
        out_l = labels_nearest(lab, row["m"], fill, fill_label)
    return out_i, out_l


def round_bf16(x):
    """fp32 -> bf16 (round to nearest even) -> fp32, finite inputs."""
    b = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    b = (b + np.uint64(0x7FFF) + ((b >> np.uint64(16)) & np.uint64(1))) & np.uint64(0xFFFF0000)
    return b.astype(np.uint32).view(np.float32)
