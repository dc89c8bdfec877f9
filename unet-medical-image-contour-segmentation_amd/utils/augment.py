"""Seeded training augmentation on the device (csrc/augment.hip, `uh_batch_augment`; DESIGN.md section 3 "Training
augmentation").  The reference has none beyond the x4 quarter turns of BasicDataset; this stage is off unless asked for.

    cfg = AugmentConfig.parse("flip,rotate=15,scale=0.1,translate=0.05,brightness=0.1,contrast=0.1,gamma=0.2,noise=0.01")
    aug = BatchAugment(cfg, seed=0)
    batch = aug(batch, epoch, indices)          # device batch {'image' [B,C,H,W], 'mask' [B,H,W]} -> a new one, same layout
    DeviceBatchLoader(ds, 8, shuffle=True, seed=0, augment=aug)

Per item the host draws a flip pair, a rotation, an isotropic scale, a translation, a brightness shift, a contrast factor, a
gamma and a noise key from Philox4x32-10 keyed by the seed with counter (dataset index, epoch, draw, 0): an item's
augmentation depends on (seed, epoch, index) only -- not on the batch size, the position in the batch, the shuffle order
or thread timing.  The geometry becomes ONE inverse affine map per item, handed to the kernel as six int64 Q32 numbers;
the kernel walks it in integer arithmetic, so tests/augment_ref.py restates the whole stage in numpy bit for bit.

Draws (u = (r + 0.5) 2^-32 in (0, 1) from word r; s(u) = 2u - 1):
    draw 0: word 0 hflip (u < p_hflip), word 1 vflip, word 2 rotation s(u) rotate_deg, word 3 scale 1 + s(u) scale
    draw 1: word 0 / 1 translation s(u) translate W / H pixels, word 2 brightness s(u) brightness, word 3 contrast 1 + s(u) contrast
    draw 2: word 0 gamma exp(s(u) ln(1 + gamma)), words 1 / 2 the noise key; noise_std is not drawn
A range of 0 gives the neutral value exactly, and the all-neutral configuration is the identity: the kernel skips every
neutral stage and returns the input bits.  There is no CPU fallback.

Elastic deformation (`uh_batch_augment_elastic`; DESIGN.md section 3 "Elastic deformation") is a second, optional record:

    aug = BatchAugment(cfg, seed=0, elastic=ElasticConfig.parse("grid=64,sigma=4"))

Per item the host draws a displacement (dx, dy) for every point of a control grid of spacing `grid` pixels: normals from
the item's noise key with counter (block, 0, 0, 2), clamped to +-2 and scaled by `sigma`, in Q16 pixels; draw 3, word 0
decides whether the item is deformed at all (u < p).  The kernel evaluates the cubic B-spline through those points in
integer arithmetic from a Q20 weight table (`elastic_weights`) and adds it to the affine walk's source position."""
from __future__ import annotations

import dataclasses
import math
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

BORDERS = ("clamp", "fill")
# include/unet_hip.h: uh_augment_params (72 bytes)
PARAMS_DTYPE = np.dtype([("m", "<i8", (6,)), ("gamma", "<f4"), ("contrast", "<f4"), ("brightness", "<f4"),
                         ("noise_std", "<f4"), ("key", "<u4", (2,))])
Q32 = float(1 << 32)
# what a bare `--augment` means: mild values for a few hundred grey-scale scans -- both flips (with the dataset's quarter
# turns: the whole dihedral group), +-10 degrees, +-10 % size, +-5 % shift, +-0.05 brightness, +-10 % contrast, gamma in
# [1/1.1, 1.1], noise of 0.01 (2.5 grey levels of 255)
PRESETS = {"default": "flip,rotate=10,scale=0.1,translate=0.05,brightness=0.05,contrast=0.1,gamma=0.1,noise=0.01"}
# what a bare `--elastic` means: control points every 64 pixels, displaced by N(0, 4^2) pixels clamped to +-8
ELASTIC_PRESETS = {"default": "grid=64,sigma=4"}
Q16, Q20 = 1 << 16, 1 << 20

_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


def philox4x32_10(counter, key) -> np.ndarray:
    """Philox4x32-10 (Salmon et al., SC'11): counter [..., 4] and key [..., 2] uint32 words -> [..., 4] uint32."""
    c = np.asarray(counter, dtype=np.uint64) & 0xFFFFFFFF
    k = np.asarray(key, dtype=np.uint64) & 0xFFFFFFFF
    c0, c1, c2, c3 = (c[..., i].copy() for i in range(4))
    k0, k1 = k[..., 0].copy(), k[..., 1].copy()
    mask = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c0, np.uint64(_M1) * c2          # 32 x 32 -> 64 bits, exact in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & mask, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & mask
        k0, k1 = (k0 + np.uint64(_W0)) & mask, (k1 + np.uint64(_W1)) & mask
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


_FLOAT_KEYS = {"rotate": "rotate_deg", "scale": "scale", "translate": "translate", "brightness": "brightness",
               "contrast": "contrast", "gamma": "gamma", "noise": "noise_std", "hflip": "p_hflip", "vflip": "p_vflip",
               "fill_image": "fill_image"}


@dataclasses.dataclass(frozen=True)
class AugmentConfig:
    """Ranges of the per-item draws.  Every default is neutral: AugmentConfig() is the identity."""
    p_hflip: float = 0.0          # probability of a left-right flip
    p_vflip: float = 0.0          # probability of an up-down flip
    rotate_deg: float = 0.0       # rotation drawn from [-rotate_deg, rotate_deg] degrees
    scale: float = 0.0            # isotropic scale drawn from [1 - scale, 1 + scale]
    translate: float = 0.0        # shift drawn from [-translate, translate] x (width, height)
    brightness: float = 0.0       # additive shift drawn from [-brightness, brightness]
    contrast: float = 0.0         # factor about 0.5 drawn from [1 - contrast, 1 + contrast]
    gamma: float = 0.0            # exponent drawn log-uniformly from [1 / (1 + gamma), 1 + gamma]
    noise_std: float = 0.0        # sigma of the additive Gaussian noise
    border: str = "clamp"         # 'clamp': source coordinates clamped to the image; 'fill': constants outside it
    fill_image: float = 0.0
    fill_label: int = 1           # class 1 = the background grey 128

    def __post_init__(self):
        if self.border not in BORDERS:
            raise ValueError(f"AugmentConfig: border is one of {BORDERS}, not {self.border!r}")
        if not (0 <= self.p_hflip <= 1 and 0 <= self.p_vflip <= 1):
            raise ValueError("AugmentConfig: flip probabilities lie in [0, 1]")
        if not (0 <= self.scale < 1 and 0 <= self.contrast <= 1 and 0 <= self.translate <= 1):
            raise ValueError("AugmentConfig: scale in [0, 1), contrast and translate in [0, 1]")
        if min(self.rotate_deg, self.brightness, self.gamma, self.noise_std) < 0 or self.rotate_deg > 180:
            raise ValueError("AugmentConfig: rotate (<= 180), brightness, gamma and noise are not negative")

    @property
    def is_identity(self) -> bool:
        return not any((self.p_hflip, self.p_vflip, self.rotate_deg, self.scale, self.translate, self.brightness,
                        self.contrast, self.gamma, self.noise_std))

    @classmethod
    def parse(cls, spec: str) -> "AugmentConfig":
        """'flip,rotate=15,scale=0.1,...' -> config.  Keys: flip[=p] (both flips, p = 0.5), hflip[=p], vflip[=p], rotate
        (degrees), scale, translate, brightness, contrast, gamma, noise, border=clamp|fill, fill_image, fill_label; a preset
        name (PRESETS) stands for its spec; 'none' or '' is the identity.  Later keys win; unknown keys raise."""
        vals: Dict[str, object] = {}
        for tok in (t.strip() for t in PRESETS.get(spec.strip(), spec).split(",")):
            if not tok or tok == "none":
                continue
            name, eq, val = (s.strip() for s in tok.partition("="))
            if name in PRESETS and not eq:
                vals.update(dataclasses.asdict(cls.parse(PRESETS[name])))
            elif name in ("flip", "hflip", "vflip"):
                p = float(val) if eq else 0.5
                for f in (("p_hflip", "p_vflip") if name == "flip" else ("p_" + name,)):
                    vals[f] = p
            elif name in _FLOAT_KEYS and eq:
                vals[_FLOAT_KEYS[name]] = float(val)
            elif name == "fill_label" and eq:
                vals["fill_label"] = int(val)
            elif name == "border" and eq:
                vals["border"] = val
            else:
                raise ValueError(f"AugmentConfig.parse: unknown or valueless key {tok!r} in {spec!r}")
        return cls(**vals)

    def spec(self) -> str:
        """The canonical spec: AugmentConfig.parse(cfg.spec()) == cfg."""
        out = [f"{key}={getattr(self, field)!r}" for key, field in _FLOAT_KEYS.items() if key != "fill_image"]
        return ",".join(out + [f"border={self.border}", f"fill_image={self.fill_image!r}", f"fill_label={self.fill_label}"])


@dataclasses.dataclass(frozen=True)
class ElasticConfig:
    """The elastic deformation of an item: a cubic B-spline displacement field over a control grid.  The default is the
    identity (sigma = 0).  8 sigma < grid is required: the draws are clamped to +-2 sigma, so no entry of the field's
    Jacobian passes r = 4 sigma / grid and det(I + J) >= 1 - 2 r > 0: the warp never folds."""
    grid: int = 64                # control-point spacing in pixels: a multiple of 16 in [16, 256]
    sigma: float = 0.0            # standard deviation of a control displacement in pixels
    p: float = 1.0                # probability that an item is deformed at all

    def __post_init__(self):
        if isinstance(self.grid, bool) or int(self.grid) != self.grid or not 16 <= self.grid <= 256 or self.grid % 16:
            raise ValueError(f"ElasticConfig: grid is a multiple of 16 in [16, 256], not {self.grid!r}")
        if not (math.isfinite(self.sigma) and self.sigma >= 0 and 0 <= self.p <= 1):
            raise ValueError("ElasticConfig: sigma is finite and not negative, p lies in [0, 1]")
        if not 8 * self.sigma < self.grid:
            raise ValueError(f"ElasticConfig: 8 sigma < grid keeps the warp from folding; sigma={self.sigma!r}, grid={self.grid}")

    @property
    def is_identity(self) -> bool:
        return self.sigma == 0 or self.p == 0

    @classmethod
    def parse(cls, spec: str) -> "ElasticConfig":
        """'grid=64,sigma=4[,p=0.5]' -> config; a preset name (ELASTIC_PRESETS) stands for its spec; 'none' or '' is the
        identity.  Later keys win; unknown keys raise."""
        vals: Dict[str, object] = {}
        for tok in (t.strip() for t in ELASTIC_PRESETS.get(spec.strip(), spec).split(",")):
            if not tok or tok == "none":
                continue
            name, eq, val = (s.strip() for s in tok.partition("="))
            if name in ELASTIC_PRESETS and not eq:
                vals.update(dataclasses.asdict(cls.parse(ELASTIC_PRESETS[name])))
            elif name == "grid" and eq:
                vals["grid"] = int(val)
            elif name in ("sigma", "p") and eq:
                vals[name] = float(val)
            else:
                raise ValueError(f"ElasticConfig.parse: unknown or valueless key {tok!r} in {spec!r}")
        return cls(**vals)

    def spec(self) -> str:
        """The canonical spec: ElasticConfig.parse(cfg.spec()) == cfg."""
        return f"grid={self.grid},sigma={self.sigma!r},p={self.p!r}"


def elastic_grid_shape(size: Tuple[int, int], grid: int) -> Tuple[int, int]:
    """(GH, GW) of the control table of an H x W image: ceil(n / grid) + 3 points per axis, point k at (k - 1) grid."""
    return -(-int(size[0]) // grid) + 3, -(-int(size[1]) // grid) + 3


def elastic_weights(grid: int) -> np.ndarray:
    """int32 [grid, 4]: the uniform cubic B-spline basis at t = (n + 0.5) / grid with denominator 2^20, rounded from
    float64; the (first) largest entry of each row is adjusted so that the row sums to exactly 2^20.  Both axes use it."""
    ElasticConfig(grid=grid)                                       # a multiple of 16 in [16, 256], or ValueError
    t = (np.arange(int(grid), dtype=np.float64) + 0.5) / float(grid)
    basis = np.stack([(1.0 - t) ** 3 / 6.0, (3.0 * t ** 3 - 6.0 * t ** 2 + 4.0) / 6.0,
                      (-3.0 * t ** 3 + 3.0 * t ** 2 + 3.0 * t + 1.0) / 6.0, t ** 3 / 6.0], axis=1)
    w = np.rint(basis * float(Q20)).astype(np.int64)
    rows = np.arange(w.shape[0])
    w[rows, np.argmax(w, axis=1)] += Q20 - w.sum(axis=1)
    return w.astype(np.int32)


def _unit(words: np.ndarray) -> np.ndarray:
    return (words.astype(np.float64) + 0.5) / Q32


def affine_matrix(hflip, vflip, theta_deg, scale, tx, ty, height: int, width: int) -> np.ndarray:
    """The inverse map [2, 3] (float64) in pixel-centre coordinates, pixel i covering [i, i + 1): the forward transform is
    flip, then rotation by theta, then scale, then a shift by (tx, ty) pixels, all about the image centre; its inverse takes
    the output centre (x + 0.5, y + 0.5) to the source centre  F R(-theta) (out - centre - t) / scale + centre."""
    fx, fy = (-1.0 if hflip else 1.0), (-1.0 if vflip else 1.0)
    th = math.radians(float(theta_deg))
    cs, sn = (math.cos(th), math.sin(th)) if theta_deg != 0 else (1.0, 0.0)
    a = np.array([[fx * cs, fx * sn], [-fy * sn, fy * cs]], np.float64) / float(scale)
    cx, cy = width / 2.0, height / 2.0
    off = np.array([cx, cy]) - a @ np.array([cx + float(tx), cy + float(ty)])
    return np.concatenate([a, off[:, None]], axis=1)


def matrix_q32(matrix: np.ndarray) -> np.ndarray:
    """[2, 3] float64 -> six int64 Q32 numbers (m00 m01 m02 m10 m11 m12), rounded to nearest."""
    return np.rint(np.asarray(matrix, np.float64).reshape(6) * Q32).astype(np.int64)


class BatchAugment:
    """config + seed -> the per-item parameter table (host, pure) and the augmented device batch (`uh_batch_augment`).
    `elastic`: an ElasticConfig or its spec; unless it is absent or the identity, every item also gets a control table
    (`elastic_table`) and the launch is `uh_batch_augment_elastic`."""

    def __init__(self, config: AugmentConfig, seed: int, elastic: Optional[ElasticConfig] = None):
        if isinstance(config, str):
            config = AugmentConfig.parse(config)
        if isinstance(elastic, str):
            elastic = ElasticConfig.parse(elastic)
        self.config, self.seed, self.elastic = config, int(seed), elastic
        self.key = np.array([self.seed & 0xFFFFFFFF, (self.seed >> 32) & 0xFFFFFFFF], np.uint32)

    def _draw_words(self, epoch: int, idx: np.ndarray, n_draws: int) -> np.ndarray:
        """Philox words [n, n_draws, 4] of draws 0 .. n_draws - 1: key = the seed, counter (index, epoch, draw, 0)."""
        ctr = np.zeros((idx.size, n_draws, 4), np.uint32)
        ctr[:, :, 0] = idx[:, None]
        ctr[:, :, 1] = int(epoch)
        ctr[:, :, 2] = np.arange(n_draws)[None, :]
        return philox4x32_10(ctr, self.key)

    def draws(self, epoch: int, indices: Sequence[int], size: Tuple[int, int]) -> Dict[str, np.ndarray]:
        """The drawn values of every item (float64 / bool arrays over `indices`), before the matrix is composed."""
        cfg, (H, W) = self.config, size
        idx = np.asarray(list(indices), dtype=np.int64).reshape(-1)
        if idx.size and (idx.min() < 0 or idx.max() >= 1 << 32) or not 0 <= int(epoch) < 1 << 32:
            raise ValueError("BatchAugment: indices and epoch are 32-bit counters")
        words = self._draw_words(epoch, idx, 3)                    # [n, 3 draws, 4 words]
        u = _unit(words)
        s = 2.0 * u - 1.0
        ranged = lambda r, v, neutral: neutral + v * r if r else np.full(idx.size, neutral, np.float64)
        return {"hflip": u[:, 0, 0] < cfg.p_hflip, "vflip": u[:, 0, 1] < cfg.p_vflip,
                "theta_deg": ranged(cfg.rotate_deg, s[:, 0, 2], 0.0), "scale": ranged(cfg.scale, s[:, 0, 3], 1.0),
                "tx": ranged(cfg.translate * W, s[:, 1, 0], 0.0), "ty": ranged(cfg.translate * H, s[:, 1, 1], 0.0),
                "brightness": ranged(cfg.brightness, s[:, 1, 2], 0.0), "contrast": ranged(cfg.contrast, s[:, 1, 3], 1.0),
                "gamma": np.exp(s[:, 2, 0] * math.log1p(cfg.gamma)) if cfg.gamma else np.ones(idx.size),
                "key": words[:, 2, 1:3]}

    def params(self, epoch: int, indices: Sequence[int], size: Tuple[int, int]) -> np.ndarray:
        """The host table for dataset items `indices` of an H x W batch (size = (H, W)): a PARAMS_DTYPE array, row i for
        indices[i] -- the Q32 matrix, the photometric scalars as fp32 and the noise key.  A pure function of
        (config, seed, epoch, index, size)."""
        H, W = int(size[0]), int(size[1])
        d = self.draws(epoch, indices, (H, W))
        n = d["gamma"].size
        table = np.zeros(n, PARAMS_DTYPE)
        for i in range(n):
            table["m"][i] = matrix_q32(affine_matrix(d["hflip"][i], d["vflip"][i], d["theta_deg"][i], d["scale"][i],
                                                     d["tx"][i], d["ty"][i], H, W))
        table["gamma"], table["contrast"], table["brightness"] = d["gamma"], d["contrast"], d["brightness"]
        table["noise_std"] = self.config.noise_std
        table["key"] = d["key"]
        return table

    def elastic_table(self, epoch: int, indices: Sequence[int], size: Tuple[int, int]) -> np.ndarray:
        """int32 [n, GH, GW, 2]: the (dx, dy) control displacements of dataset items `indices` in Q16 pixels, GW =
        ceil(W / grid) + 3 and GH likewise.  Word 0 of draw 3 decides whether an item is deformed (u < p; otherwise its row is
        zero).  Control point q = ky GW + kx takes normals 2 (q & 1) (dx) and 2 (q & 1) + 1 (dy) of the Philox block with
        the item's noise key and counter (q >> 1, 0, 0, 2) -- the noise stage uses last word 1 -- by Box-Muller in float64
        (radius from u = (r + 0.5) 2^-32, angle 2 pi r 2^-32, cosine first), clamped to [-2, 2]: d = rint(z sigma 2^16).
        A pure function of (config, seed, epoch, index, size)."""
        el = self.elastic if self.elastic is not None else ElasticConfig()
        GH, GW = elastic_grid_shape(size, el.grid)
        key = self.draws(epoch, indices, (int(size[0]), int(size[1])))["key"]                   # validates the counters
        idx = np.asarray(list(indices), dtype=np.int64).reshape(-1)
        n, blocks = idx.size, (GH * GW + 1) // 2
        on = _unit(self._draw_words(epoch, idx, 4)[:, 3, 0]) < el.p
        ctr = np.zeros((n, blocks, 4), np.uint32)
        ctr[:, :, 0] = np.arange(blocks)[None, :]
        ctr[:, :, 3] = 2
        w = philox4x32_10(ctr, key[:, None, :]).astype(np.float64).reshape(n, blocks, 2, 2)     # [.., pair, (radius, angle)]
        u, v = (w[..., 0] + 0.5) * 2.0 ** -32, w[..., 1] * 2.0 ** -32
        rad, ang = np.sqrt(-2.0 * np.log(u)), (2.0 * math.pi) * v
        z = np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=-1).reshape(n, 2 * blocks, 2)[:, :GH * GW]
        d = np.rint(np.clip(z, -2.0, 2.0) * float(el.sigma) * float(Q16)).astype(np.int32)
        d[~on] = 0
        return d.reshape(n, GH, GW, 2)

    def __call__(self, batch, epoch: int, indices: Sequence[int]):
        """Device batch {'image': [B,C,H,W] fp32 / bf16 (any strides; channels_last is free), 'mask': int64 [B,H,W]} ->
        a new batch in the same layout (logical NCHW, channels_last memory).  Either entry may be absent."""
        ref = batch.get("image") if batch.get("image") is not None else batch.get("mask")
        if ref is None:
            raise ValueError("BatchAugment: the batch holds neither 'image' nor 'mask'")
        if len(indices) != ref.shape[0]:
            raise ValueError(f"BatchAugment: {len(indices)} indices for a batch of {ref.shape[0]}")
        cfg, size = self.config, (ref.shape[-2], ref.shape[-1])
        elastic = self.elastic is not None and not self.elastic.is_identity
        return _launch(batch, lambda: self.params(epoch, indices, size),
                       (lambda: self.elastic_table(epoch, indices, size)) if elastic else None,
                       self.elastic.grid if elastic else 0, cfg.border, cfg.fill_image, cfg.fill_label)


_WEIGHTS = {}                     # (grid, device) -> the device copy of elastic_weights(grid)


def augment_with_control(batch, params: np.ndarray, control, grid: int, border: str = "clamp", fill_image: float = 0.0,
                         fill_label: int = 1):
    """`uh_batch_augment_elastic` with explicit tables: `params` a PARAMS_DTYPE array [B], `control` int32 [B, GH, GW, 2]
    (numpy or torch) in Q16 pixels for control spacing `grid`; control=None is the plain `uh_batch_augment` launch of the
    same rows.  The batch and the result are laid out as in BatchAugment.__call__.  There is no CPU fallback."""
    return _launch(batch, lambda: params, None if control is None else (lambda: control), int(grid), border, fill_image,
                   fill_label)


def _launch(batch, params, control, grid: int, border: str, fill_image: float, fill_label: int):
    """One launch over a device batch: `uh_batch_augment`, or `uh_batch_augment_elastic` when `control` is given.  `params`
    and `control` are called for their tables once the batch has been checked."""
    import torch
    from .. import ops
    from .._lib import LIB
    image, mask = batch.get("image"), batch.get("mask")
    ref = image if image is not None else mask
    if ref is None:
        raise ValueError("BatchAugment: the batch holds neither 'image' nor 'mask'")
    for t in (image, mask):
        if t is not None:
            ops._require_gpu(t, "BatchAugment batch")
    B, H, W = ref.shape[0], ref.shape[-2], ref.shape[-1]
    C, nhwc, out, labels = 1, None, None, None
    if image is not None:
        if image.dim() != 4 or not 1 <= image.shape[1] <= 4:
            raise ValueError(f"BatchAugment: image batch {tuple(image.shape)} is not [B, 1..4, H, W]")
        C = image.shape[1]
        nhwc = image.permute(0, 2, 3, 1).contiguous()
        out = torch.empty_like(nhwc)
    if mask is not None:
        if mask.dtype != torch.int64 or tuple(mask.shape) != (B, H, W):
            raise TypeError(f"BatchAugment: mask batch must be int64 [B, H, W], got {mask.dtype} {tuple(mask.shape)}")
        mask = mask.contiguous()
        labels = torch.empty_like(mask)
    if border not in BORDERS:
        raise ValueError(f"BatchAugment: border is one of {BORDERS}, not {border!r}")
    if control is not None:
        ElasticConfig(grid=grid)                                   # a multiple of 16 in [16, 256], or ValueError
    table = np.ascontiguousarray(params(), PARAMS_DTYPE)
    if table.shape != (B,):
        raise ValueError(f"BatchAugment: {table.shape} parameter rows for a batch of {B}")
    tail = (B, H, W, C, ops._dt(nhwc) if nhwc is not None else 0, BORDERS.index(border), float(fill_image), int(fill_label))
    with torch.cuda.device(ref.device):
        stream = torch.cuda.current_stream()
        t_d = torch.from_numpy(table.view(np.uint8).reshape(B, PARAMS_DTYPE.itemsize)).to(ref.device)
        if control is None:
            LIB.call("uh_batch_augment", ops._p(nhwc), C, ops._p(mask), t_d.data_ptr(), ops._p(out), C, ops._p(labels),
                     *tail, stream.cuda_stream)
        else:
            c_d = torch.as_tensor(control())
            want = (B,) + elastic_grid_shape((H, W), grid) + (2,)
            if c_d.dtype != torch.int32 or tuple(c_d.shape) != want:
                raise TypeError(f"BatchAugment: control table must be int32 {want}, got {c_d.dtype} {tuple(c_d.shape)}")
            c_d = c_d.to(ref.device).contiguous()
            w_d = _WEIGHTS.get((grid, ref.device))
            if w_d is None:
                w_d = _WEIGHTS[(grid, ref.device)] = torch.from_numpy(elastic_weights(grid)).to(ref.device)
            LIB.call("uh_batch_augment_elastic", ops._p(nhwc), C, ops._p(mask), t_d.data_ptr(), c_d.data_ptr(), w_d.data_ptr(),
                     grid, ops._p(out), C, ops._p(labels), *tail, stream.cuda_stream)
            c_d.record_stream(stream)
        t_d.record_stream(stream)
    res = dict(batch)
    if out is not None:
        res["image"] = out.permute(0, 3, 1, 2)
    if labels is not None:
        res["mask"] = labels
    return res
