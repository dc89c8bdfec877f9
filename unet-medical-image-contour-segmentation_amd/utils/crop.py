"""Patch training: one seeded, foreground-aware square crop per item and epoch, chosen and cut on the device (csrc/crop.hip,
`uh_crop_select` / `uh_crop_gather`; DESIGN.md section 3 "Patch training").  Off unless asked for.

    cfg = CropConfig.parse("256,fg=0.7,classes=1+2")
    crop = BatchCrop(cfg, seed=0, n_classes=3)
    batch = crop(items, epoch, indices)         # prepared device items of ANY sizes -> {'image' [B,C,256,256], 'mask' [B,256,256]}
    DeviceBatchLoader(ds, 8, shuffle=True, seed=0, crop=crop)

The crop is taken from the prepared item -- what ds[i] returns: image [C,H,W], labels [H,W] -- before any augmentation.  Per
item the host draws four words r0..r3 from Philox4x32-10 keyed by the seed with counter (dataset index, epoch, 4, 0): draw 4
of the scheme of utils/augment.py, whose own draws are 0..3, so the two streams are independent under one seed and a crop
depends on (seed, epoch, index) only.  Everything after the draw is integer arithmetic (tests/crop_ref.py restates it in numpy
bit for bit).  With ny = H - size + 1, nx = W - size + 1, n the number of pixels whose label is in `classes` and
T = rint(fg 2^32):
    foreground branch, iff n > 0 and r0 < T:  k = (r1 n) >> 32, (py, px) the k-th such pixel in raster order,
        jy = (r2 size) >> 32, jx = (r3 size) >> 32, oy = clamp(py - jy, 0, ny - 1), ox = clamp(px - jx, 0, nx - 1)
        -- the chosen pixel lies inside the crop, at a uniform position unless the border clamps it;
    uniform branch, otherwise:                oy = (r2 ny) >> 32, ox = (r3 nx) >> 32.
An item smaller than the crop is an error that names it: there is no padding.  There is no CPU fallback."""
from __future__ import annotations

import dataclasses
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from .augment import philox4x32_10

MIN_SIZE, SIZE_STEP, MAX_SIDE = 16, 16, 16384
MAX_CLASS = 63                            # the class set is a 64-bit mask in the library
DEFAULT_SIZE, DEFAULT_FG = 256, 0.5
DEFAULT_SPEC = f"{DEFAULT_SIZE},fg={DEFAULT_FG!r}"          # a bare --crop
CROP_DRAW = 4                             # utils/augment.py owns draws 0..3
# include/unet_hip.h: uh_crop_item (48 bytes)
ITEM_DTYPE = np.dtype([("image", "<u8"), ("labels", "<u8"), ("H", "<i4"), ("W", "<i4"), ("ld", "<i4"), ("reserved", "<i4"),
                       ("r", "<u4", (4,))])


def _is_int(v) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


@dataclasses.dataclass(frozen=True)
class CropConfig:
    """size: the crop's side, a multiple of 16 from 16 up; fg: the probability of the foreground branch, in [0, 1]; classes: the
    label values that count as foreground, distinct ids in 0..63, or None for the class `evaluate` scores (for_head)."""
    size: int = DEFAULT_SIZE
    fg: float = DEFAULT_FG
    classes: Optional[Tuple[int, ...]] = None

    def __post_init__(self):
        if not _is_int(self.size) or not MIN_SIZE <= self.size <= MAX_SIDE or self.size % SIZE_STEP:
            raise ValueError(f"crop size must be a multiple of {SIZE_STEP} in [{MIN_SIZE}, {MAX_SIDE}], got {self.size!r}")
        object.__setattr__(self, "size", int(self.size))
        if isinstance(self.fg, bool) or not isinstance(self.fg, (int, float)) or not 0.0 <= float(self.fg) <= 1.0:
            raise ValueError(f"crop fg must be a number in [0, 1], got {self.fg!r}")
        object.__setattr__(self, "fg", float(self.fg))
        if self.classes is not None:
            try:
                cls = tuple(self.classes)
            except TypeError:
                raise ValueError(f"crop classes must be a sequence of label values, got {self.classes!r}") from None
            if not cls or not all(_is_int(c) and 0 <= c <= MAX_CLASS for c in cls) or len(set(cls)) != len(cls):
                raise ValueError(f"crop classes must be distinct label values in 0..{MAX_CLASS}, got {self.classes!r}")
            object.__setattr__(self, "classes", tuple(sorted(int(c) for c in cls)))

    @classmethod
    def parse(cls, spec: str) -> "CropConfig":
        """'256', '256,fg=0.7', '256,fg=0.7,classes=1+2'; '' is the bare flag's '256,fg=0.5'.  ValueError names the token."""
        if not isinstance(spec, str):
            raise ValueError(f"a crop spec is a string like {DEFAULT_SPEC!r}, got {spec!r}")
        parts = [t.strip() for t in spec.split(",")]
        if parts == [""]:
            return cls()
        if not parts[0].isdigit():
            raise ValueError(f"bad crop spec {spec!r}: size {parts[0]!r} is not a whole number")
        vals: Dict[str, object] = {"size": int(parts[0])}
        for tok in parts[1:]:
            key, eq, val = (s.strip() for s in tok.partition("="))
            if key not in ("fg", "classes") or not eq or not val:
                raise ValueError(f"bad crop spec {spec!r}: {tok!r} is not fg=P or classes=a+b")
            if key in vals:
                raise ValueError(f"bad crop spec {spec!r}: {key} is given twice ({tok!r})")
            try:
                vals[key] = float(val) if key == "fg" else tuple(int(v) for v in val.split("+"))
            except ValueError:
                raise ValueError(f"bad crop spec {spec!r}: {tok!r} does not parse") from None
        try:
            return cls(**vals)
        except ValueError as e:
            raise ValueError(f"bad crop spec {spec!r}: {e}") from None

    def spec(self) -> str:
        """The canonical spec: CropConfig.parse(cfg.spec()) == cfg."""
        return f"{self.size},fg={self.fg!r}" + (",classes=" + "+".join(str(c) for c in self.classes) if self.classes else "")

    def for_head(self, n_classes: int) -> "CropConfig":
        """The config with its classes resolved against a head of `n_classes` outputs: None becomes the class evaluate scores
        (utils.surface_loss.default_classes: 2 for three classes and more, 1 for the binary head; a 2-class head must say);
        given classes must be labels the head's data holds (below n_classes; the binary head trains on the labels 0..2)."""
        from .surface_loss import default_classes
        n_classes = int(n_classes)
        if n_classes < 1:
            raise ValueError(f"crop: a head has at least one class, got {n_classes}")
        if self.classes is None:
            try:
                return dataclasses.replace(self, classes=default_classes(n_classes))
            except ValueError:
                raise ValueError("crop: a 2-class head has no default class; pass classes=") from None
        top = 3 if n_classes == 1 else n_classes
        if max(self.classes) >= top:
            raise ValueError(f"crop: classes {'+'.join(str(c) for c in self.classes)} do not fit a head of {n_classes} "
                             f"class{'es' if n_classes > 1 else ''} (labels 0..{top - 1})")
        return self

    @property
    def class_mask(self) -> int:
        if self.classes is None:
            raise ValueError("crop: classes are unresolved; call for_head(n_classes)")
        mask = 0
        for c in self.classes:
            mask |= 1 << c
        return mask

    @property
    def threshold(self) -> int:
        """T = rint(fg 2^32), in [0, 2^32]."""
        return int(np.rint(self.fg * 4294967296.0))


def crop_config(crop) -> Optional[CropConfig]:
    """A CropConfig, a spec string or None -> CropConfig or None."""
    if crop is None or isinstance(crop, CropConfig):
        return crop
    if isinstance(crop, str):
        return CropConfig.parse(crop)
    raise ValueError(f"crop is a CropConfig, a spec string like {DEFAULT_SPEC!r} or None, got {crop!r}")


class BatchCrop:
    """config + seed + head -> the per-item words (host, pure) and the crop batch (`uh_crop_select`, `uh_crop_gather`)."""

    def __init__(self, config, seed: int, n_classes: int):
        self.config = crop_config(config).for_head(n_classes)
        self.seed, self.n_classes = int(seed), int(n_classes)
        self.key = np.array([self.seed & 0xFFFFFFFF, (self.seed >> 32) & 0xFFFFFFFF], np.uint32)
        self.last_origins = None          # device int32 [B,2] = (oy, ox) of the last call

    def words(self, epoch: int, indices: Sequence[int]) -> np.ndarray:
        """uint32 [n,4]: r0..r3 of dataset items `indices` in 0-based epoch `epoch` -- key = the seed's low / high words,
        counter (index, epoch, 4, 0)."""
        idx = np.asarray(list(indices), dtype=np.int64).reshape(-1)
        if idx.size and (idx.min() < 0 or idx.max() >= 1 << 32) or not 0 <= int(epoch) < 1 << 32:
            raise ValueError("BatchCrop: indices and epoch are 32-bit counters")
        ctr = np.zeros((idx.size, 4), np.uint32)
        ctr[:, 0], ctr[:, 1], ctr[:, 2] = idx, int(epoch), CROP_DRAW
        return philox4x32_10(ctr, self.key)

    def __call__(self, items: Sequence[Dict], epoch: int, indices: Sequence[int]):
        """items: prepared device items {'image': [C,H,W] fp32 / bf16, 'mask': int64 [H,W]} of any sizes, one per index ->
        {'image': [B,C,size,size] in the items' dtype (channels_last memory), 'mask': int64 [B,size,size]}."""
        from .. import ops
        indices = [int(i) for i in indices]
        if len(items) != len(indices) or not items:
            raise ValueError(f"BatchCrop: {len(indices)} indices for {len(items)} items")
        size = self.config.size
        for it, i in zip(items, indices):
            shape = tuple(it["mask"].shape)
            if len(shape) != 2 or min(shape) < size:
                raise ValueError(f"BatchCrop: item {i} is {shape[0]} x {shape[1] if len(shape) > 1 else '?'}, smaller than the "
                                 f"{size} x {size} crop (there is no padding)")
        words = self.words(epoch, indices)
        masks = [it["mask"] for it in items]
        origins, _ = ops.crop_select(masks, words, size, self.config.class_mask, self.config.threshold)
        image, mask = ops.crop_gather([it["image"] for it in items], masks, origins, size)
        self.last_origins = origins
        return {"image": image, "mask": mask}


def item_table(images, labels, words=None):
    """The uh_crop_item table (an ITEM_DTYPE array) of device images [C,H,W] (or None) and int64 labels [H,W] (or None), plus
    the tensors whose memory it points to (views made contiguous here): keep them until the launch is enqueued."""
    import torch
    n = len(labels) if labels is not None else len(images)
    table = np.zeros(n, ITEM_DTYPE)
    keep: List = []
    for b in range(n):
        if labels is not None:
            m = labels[b]
            if m.dtype != torch.int64 or m.dim() != 2:
                raise TypeError(f"crop: labels must be int64 [H, W], got {m.dtype} {tuple(m.shape)} in row {b}")
            m = m.contiguous()
            keep.append(m)
            table["labels"][b], table["H"][b], table["W"][b] = m.data_ptr(), m.shape[0], m.shape[1]
        if images is not None:
            x = images[b]
            if x.dim() != 3:
                raise TypeError(f"crop: an image is [C, H, W], got {tuple(x.shape)} in row {b}")
            v = x.permute(1, 2, 0)                                     # NHWC view; a pixel's channels must be consecutive
            H, W, C = v.shape
            if labels is not None and (H, W) != tuple(labels[b].shape):
                raise ValueError(f"crop: image {H} x {W} and labels {tuple(labels[b].shape)} differ in row {b}")
            ld = v.stride(1) if W > 1 else C
            if (C > 1 and v.stride(2) != 1) or ld < C or (H > 1 and v.stride(0) != W * ld):
                v, ld = v.contiguous(), C
            keep.append(v)
            table["image"][b], table["H"][b], table["W"][b], table["ld"][b] = v.data_ptr(), H, W, ld
    if words is not None:
        w = np.asarray(words, dtype=np.uint32)
        if w.shape != (n, 4):
            raise ValueError(f"crop: {w.shape} words for {n} rows; expected ({n}, 4)")
        table["r"] = w
    return table, keep
