"""Device-resident dataset cache: decode every training file once, keep the decoded bytes on the GPU and cut every later batch
from them with one launch (csrc/cache.hip, `uh_cache_gather_u8`; DESIGN.md section 3 "Dataset cache").  Off unless asked for.

    cache = DatasetCache(ds)                        # decodes len(ds.ids) image / mask pairs, uploads them into one arena
    raw = cache.gather([5, 2, 7])                   # what collate_raw returns for these items, as device tensors
    DeviceBatchLoader(ds, 8, shuffle=True, seed=0, cache=cache)        # the same batches, bit for bit, with no decode

BasicDataset serves a file as four items, one per quarter turn, and every one of them is a fresh decode of the same PNG pair:
e epochs decode a file 4 e times.  The cache keeps one ENTRY per file -- `ds.raw_item(e * views, host_rescale=False)`: the decoded
uint8 image and mask, unrotated and unrescaled -- and item `index` is entry `index // views` with `turns = index % views`, the
turns and the dataset's scale going to prepare_batch_device as they do from collate_raw.  Nothing downstream changes.

The arena is one torch.uint8 tensor laid out by `plan_entries`: an image is followed by its mask, every start is 16-byte
aligned and every entry is padded to a multiple of 16 bytes, which is what the gather kernel's 16-byte loads need.  The sizes
come from the files' headers (Pillow opens a file without decoding it), so a dataset over the limit is refused before a pixel
is decoded or a byte allocated.  The build decodes in `workers` threads and uploads through two pinned staging buffers of
bounded size: the host never holds the dataset.  The cache is all or nothing, and it does not watch the files."""
from __future__ import annotations

import time
from collections import deque
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

from .data_loading import QUARTER_TURNS

ALIGN = 16                              # csrc/cache.hip reads whole aligned 16-byte units
STAGE_BYTES = 32 << 20                  # one pinned staging buffer (two are used); grows to the largest entry if that is larger
# Pillow modes that np.asarray turns into uint8, and the channels they give
_MODE_CHANNELS = {"L": 1, "P": 1, "LA": 2, "PA": 2, "RGB": 3, "YCbCr": 3, "LAB": 3, "HSV": 3, "RGBA": 4, "RGBX": 4, "CMYK": 4}


class DatasetCacheTooLarge(ValueError):
    """The dataset's decoded bytes exceed the cache's limit."""


def _round_up(n: int) -> int:
    return (int(n) + ALIGN - 1) // ALIGN * ALIGN


def plan_entries(shapes: Sequence[Tuple[int, int, int]]) -> Tuple[List[int], List[int], int]:
    """The arena layout of entries with decoded shapes (H, W, C): -> (image_offsets, mask_offsets, total_bytes).  Entry e's image
    (H W C bytes) is followed by its mask (H W bytes); every start is a multiple of 16 and every entry takes a multiple of 16 bytes."""
    image_offsets, mask_offsets, off = [], [], 0
    for shape in shapes:
        H, W, C = (int(v) for v in shape)
        if H < 1 or W < 1 or C < 1:
            raise ValueError(f"plan_entries: bad shape {tuple(shape)!r}")
        image_offsets.append(off)
        off += _round_up(H * W * C)
        mask_offsets.append(off)
        off += _round_up(H * W)
    return image_offsets, mask_offsets, off


def entry_of(index: int, augment: bool) -> Tuple[int, int]:
    """Dataset item `index` -> (entry, turns): the file it comes from and the quarter turns the device stage applies."""
    views = QUARTER_TURNS if augment else 1
    return int(index) // views, int(index) % views


def _header_shape(path) -> Tuple[Tuple[int, ...], str]:
    """(the shape np.asarray(load_image(path)) will have, its dtype name) without decoding the pixels."""
    from PIL import Image
    suffix = path.suffix
    if suffix == ".npy":
        a = np.load(path, mmap_mode="r")
        return tuple(a.shape), str(a.dtype)
    if suffix in {".pt", ".pth"}:
        a = torch.load(path)
        return tuple(a.shape), str(a.dtype).replace("torch.", "")
    with Image.open(path) as im:
        w, h = im.size
        c = _MODE_CHANNELS.get(im.mode)
        if c is None:
            return (h, w), im.mode                      # 1, I, I;16, F: not 8-bit
        return ((h, w) if c == 1 else (h, w, c)), "uint8"


class DatasetCache:
    """The decoded files of `ds` (a BasicDataset) in one device arena.  `workers` decode threads (a count, never the machine's
    CPU count); `limit_bytes` None = half of the device memory that is free when the build starts.  A dataset over the limit
    raises DatasetCacheTooLarge before anything is decoded or allocated; one that does not decode to 8 bits raises raw_item's
    TypeError.  Attributes: nbytes (the arena), entries (files), build_seconds, decodes (load_image calls made), limit_bytes."""

    def __init__(self, ds, device=None, workers: int = 8, limit_bytes=None):
        if not torch.cuda.is_available():
            raise RuntimeError("DatasetCache needs a GPU (the host path is BasicDataset.__getitem__)")
        if not all(hasattr(ds, a) for a in ("raw_item", "ids", "augment", "_only", "images_dir", "mask_dir", "mask_suffix")):
            raise ValueError("DatasetCache caches a BasicDataset (raw_item, ids, augment and the folders)")
        if int(workers) < 1:
            raise ValueError("DatasetCache: workers must be positive")
        t0 = time.perf_counter()
        self.ds = ds
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.views = QUARTER_TURNS if ds.augment else 1
        self.entries = len(ds.ids)
        self.decodes = 0
        self._arena = None
        if limit_bytes is None:
            limit_bytes = torch.cuda.mem_get_info(self.device)[0] // 2
        self.limit_bytes = int(limit_bytes)
        # the paths, resolved once, and the headers: sizes before a pixel is decoded
        self._raw_shapes: List[Tuple[int, ...]] = []
        for stem in ds.ids:
            ishape, idt = _header_shape(ds._only(ds.images_dir, stem, "image"))
            mshape, mdt = _header_shape(ds._only(ds.mask_dir, stem + ds.mask_suffix, "mask"))
            if idt != "uint8" or mdt != "uint8":
                raise TypeError(f"DatasetCache: {stem} does not decode to 8-bit pixels ({idt}, {mdt}); such a dataset is not cached")
            if len(ishape) not in (2, 3) or (len(ishape) == 3 and not 1 <= ishape[2] <= 4) or tuple(mshape) != tuple(ishape[:2]):
                raise ValueError(f"DatasetCache: {stem} has an image of shape {ishape} and a mask of shape {mshape}")
            self._raw_shapes.append(tuple(ishape))
        self.shapes = [s if len(s) == 3 else s + (1,) for s in self._raw_shapes]
        self._image_off, self._mask_off, self.nbytes = plan_entries(self.shapes)
        if self.nbytes > self.limit_bytes:
            raise DatasetCacheTooLarge(f"DatasetCache: the dataset decodes to {self.nbytes} bytes ({self.entries} files), over the "
                                       f"limit of {self.limit_bytes} bytes")
        self.scale = 1.0
        self._build(int(workers))
        self.build_seconds = time.perf_counter() - t0

    # ------------------------------------------------------------------------------------------------------------ build
    def _decode(self, e: int) -> Dict:
        it = self.ds.raw_item(e * self.views, host_rescale=False)          # two load_image calls: image and mask
        if tuple(it["image_u8"].shape) != self._raw_shapes[e] or tuple(it["mask_u8"].shape) != self._raw_shapes[e][:2]:
            raise ValueError(f"DatasetCache: {self.ds.ids[e]} decodes to {tuple(it['image_u8'].shape)} / {tuple(it['mask_u8'].shape)}, "
                             f"its header said {self._raw_shapes[e]}")
        return it

    def _build(self, workers: int) -> None:
        from concurrent.futures import ThreadPoolExecutor
        dev = self.device
        spans = [self._mask_off[e] + _round_up(s[0] * s[1]) - self._image_off[e] for e, s in enumerate(self.shapes)]
        stage_bytes = max(STAGE_BYTES, max(spans))
        with torch.cuda.device(dev):
            arena = torch.empty(self.nbytes, dtype=torch.uint8, device=dev)
            if arena.data_ptr() % ALIGN:
                raise RuntimeError("DatasetCache: the arena is not 16-byte aligned")
            stages = [torch.empty(stage_bytes, dtype=torch.uint8, pin_memory=True) for _ in range(2)]
            done = [None, None]                                            # the event behind each staging buffer's last upload
            stream = torch.cuda.current_stream(dev)
            cur, base, fill = 0, 0, 0

            def flush():
                nonlocal cur, base, fill
                if fill:
                    arena[base:base + fill].copy_(stages[cur][:fill], non_blocking=True)
                    done[cur] = torch.cuda.Event()
                    done[cur].record(stream)
                    cur ^= 1
                    if done[cur] is not None:
                        done[cur].synchronize()                            # the buffer about to be refilled has been read
                base, fill = base + fill, 0

            scales = set()
            with ThreadPoolExecutor(workers) as pool:
                pending = deque()
                nxt = 0
                for e in range(self.entries):
                    while nxt < self.entries and len(pending) < 2 * workers:        # a bounded window of decoded entries
                        pending.append(pool.submit(self._decode, nxt))
                        nxt += 1
                    it = pending.popleft().result()
                    self.decodes += 2
                    if fill + spans[e] > stage_bytes:
                        flush()
                    host = stages[cur].numpy()
                    H, W, C = self.shapes[e]
                    io, mo = self._image_off[e] - base, self._mask_off[e] - base
                    host[io:io + H * W * C] = it["image_u8"].reshape(-1)
                    host[io + H * W * C:mo] = 0
                    host[mo:mo + H * W] = it["mask_u8"].reshape(-1)
                    host[mo + H * W:io + spans[e]] = 0
                    fill = io + spans[e]
                    scales.add(float(it.get("scale", 1.0)))
                flush()
            torch.cuda.synchronize(dev)
        if len(scales) > 1:
            raise ValueError("DatasetCache: the items of a dataset must have one scale")
        self.scale = scales.pop()
        self._arena = arena
        # one pair of views per entry, made once: a batch's row table is a list lookup
        self._rows = [(arena[self._image_off[e]:self._image_off[e] + s[0] * s[1] * s[2]],
                       arena[self._mask_off[e]:self._mask_off[e] + s[0] * s[1]]) for e, s in enumerate(self.shapes)]

    def close(self) -> None:
        """Give the arena back; gather raises afterwards."""
        self._arena = None
        self._rows = None

    # ----------------------------------------------------------------------------------------------------------- batches
    def _entries_of(self, indices) -> Tuple[List[int], List[int]]:
        if self._arena is None:
            raise RuntimeError("DatasetCache: the cache is closed")
        idx = [int(i) for i in indices]
        n = self.entries * self.views
        if not idx or any(not 0 <= i < n for i in idx):
            raise IndexError(f"DatasetCache: indices must be a non-empty list of items of a dataset of {n}")
        pairs = [entry_of(i, self.views > 1) for i in idx]
        return [e for e, _ in pairs], [t for _, t in pairs]

    def _gather(self, ents: List[int], turns: List[int]) -> Dict:
        from .. import ops
        shape = self.shapes[ents[0]]
        if any(self.shapes[e] != shape for e in ents):
            raise ValueError("collate_raw: the items of a batch must have one decoded size")
        if shape[0] != shape[1] and len({t & 1 for t in turns}) > 1:
            raise ValueError("collate_raw: non-square images rotated by odd and even quarter turns do not stack")
        H, W, C = shape
        image, mask = ops.cache_gather([self._rows[e] for e in ents], H * W * C, H * W)
        B = len(ents)
        return {"image_u8": image.view(B, H, W, C), "mask_u8": mask.view(B, H, W), "turns": torch.tensor(turns, dtype=torch.int32),
                "scale": self.scale}

    def gather(self, indices) -> Dict:
        """What collate_raw returns for the raw items `indices`, on the device: {'image_u8' [B,H,W,C], 'mask_u8' [B,H,W], 'turns'
        int32 [B] (host), 'scale'}.  collate_raw's rules and messages: one decoded shape, one turn parity unless square."""
        return self._gather(*self._entries_of(indices))

    def gather_groups(self, indices) -> Dict:
        """DeviceBatchLoader._collate_groups for the crop path: {'groups': [(positions in the batch, collated group)]}, the items
        grouped by decoded shape, turn parity (unless square) and scale, in order of first appearance."""
        ents, turns = self._entries_of(indices)
        groups: Dict = {}
        for pos, (e, t) in enumerate(zip(ents, turns)):
            shape = self._raw_shapes[e]
            parity = (t & 1) if shape[0] != shape[1] else 0
            groups.setdefault((shape, parity, self.scale), []).append(pos)
        return {"groups": [(pos, self._gather([ents[p] for p in pos], [turns[p] for p in pos])) for pos in groups.values()]}


__all__ = ["DatasetCache", "DatasetCacheTooLarge", "plan_entries", "entry_of", "ALIGN"]
