"""Sliding-window tiling: how an image is cut into tiles of one fixed shape and how the tiles' predictions are weighted
when they are put back (DESIGN.md section 3 "Tiled prediction").  Pure Python, no GPU; csrc/tiling.hip restates the same
rules in C (uh_tile_grid answers them without a launch) and tests/test_tiling_cpu.py holds the two against each other.

Per axis of length L, with tile size `size` and `overlap`:
    tile length  t = min(size, L)                      -- no padding, ever
    L <= size:   one tile at origin 0
    otherwise:   stride S = size - overlap, n = ceil((L - size) / S) + 1 tiles at o_k = min(k S, L - size)
The origins increase strictly, the first is 0 and the last tile ends at L; only the last origin is ever clamped, so a
position lies in at most 3 tiles of an axis (two of the regular sequence, because S >= size / 2, and the clamped one).
Position i of a tile of length t has the weight w(i) = max(1, min(i + 1, t - i, overlap)): a tent that is 1 at the border,
where the network saw zero padding instead of the image, and `overlap` in the middle.  A tile's weight at a pixel is
wy * wx <= 512 * 512 = 2^18.  The origin rule is NOT mirror-symmetric (the clamped tile is always the last one), so the
tiled prediction of a flipped image is not the flipped tiled prediction."""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Tuple, Union

MIN_SIZE, MAX_SIZE, SIZE_STEP = 16, 1024, 16
DEFAULT_SIZE, DEFAULT_OVERLAP = 512, 128
DEFAULT_SPEC = f"{DEFAULT_SIZE},overlap={DEFAULT_OVERLAP}"        # a bare --tile


def _is_int(v) -> bool:
    return isinstance(v, int) and not isinstance(v, bool)


@dataclass(frozen=True)
class TileConfig:
    """size: tile side, a multiple of 16 in [16, 1024]; overlap: 0 <= overlap <= size // 2.  ValueError for anything else."""
    size: int = DEFAULT_SIZE
    overlap: int = DEFAULT_OVERLAP

    def __post_init__(self):
        size, overlap = self.size, self.overlap
        if not _is_int(size) or not MIN_SIZE <= size <= MAX_SIZE or size % SIZE_STEP:
            raise ValueError(f"tile size must be a multiple of {SIZE_STEP} in [{MIN_SIZE}, {MAX_SIZE}], got {size!r}")
        if not _is_int(overlap) or not 0 <= overlap <= size // 2:
            raise ValueError(f"tile overlap must be an integer in [0, size // 2 = {size // 2}], got {overlap!r}")

    @property
    def spec(self) -> str:
        return f"{self.size},overlap={self.overlap}"


def parse_tile_spec(spec: str) -> TileConfig:
    """"512" (overlap 128, reduced to size // 2 for a size below 256), "512,overlap=64"; "" means "512,overlap=128"."""
    if not isinstance(spec, str):
        raise ValueError(f"a tile spec is a string like {DEFAULT_SPEC!r}, got {spec!r}")
    text = spec.strip()
    if not text:
        return TileConfig()
    head, sep, tail = text.partition(",")
    if not head.strip().isdigit():
        raise ValueError(f"bad tile spec {spec!r}: expected SIZE or SIZE,overlap=N")
    size = int(head)
    if not sep:
        if not MIN_SIZE <= size <= MAX_SIZE or size % SIZE_STEP:
            return TileConfig(size, 0)                          # raises with the size's message
        return TileConfig(size, min(DEFAULT_OVERLAP, size // 2))
    key, eq, val = tail.partition("=")
    if key.strip() != "overlap" or not eq or not val.strip().isdigit():
        raise ValueError(f"bad tile spec {spec!r}: expected SIZE or SIZE,overlap=N")
    return TileConfig(size, int(val))


def tile_config(tile: Union[TileConfig, str, None]) -> Optional[TileConfig]:
    """A TileConfig, a spec string or None -> TileConfig or None."""
    if tile is None:
        return None
    if isinstance(tile, TileConfig):
        return tile
    if isinstance(tile, str):
        return parse_tile_spec(tile)
    raise ValueError(f"tile is a TileConfig, a spec string like {DEFAULT_SPEC!r} or None, got {tile!r}")


def axis_origins(L: int, cfg: TileConfig) -> List[int]:
    if not _is_int(L) or L < 1:
        raise ValueError(f"an axis has a positive integer length, got {L!r}")
    if L <= cfg.size:
        return [0]
    S = cfg.size - cfg.overlap
    n = -(-(L - cfg.size) // S) + 1
    return [min(k * S, L - cfg.size) for k in range(n)]


def axis_weights(t: int, cfg: TileConfig) -> List[int]:
    """w(i) for i in 0..t-1 of a tile of length t."""
    return [max(1, min(i + 1, t - i, cfg.overlap)) for i in range(t)]


def tile_grid(H: int, W: int, cfg: TileConfig) -> Tuple[int, int, int, int, List[int], List[int]]:
    """(ny, nx, th, tw, oy, ox): the counts, the tile shape and the origins per axis of an H x W image."""
    oy, ox = axis_origins(H, cfg), axis_origins(W, cfg)
    return len(oy), len(ox), min(cfg.size, H), min(cfg.size, W), oy, ox


def tile_shape(H: int, W: int, cfg: TileConfig) -> Tuple[int, int]:
    return min(cfg.size, H), min(cfg.size, W)


def tile_count(H: int, W: int, cfg: TileConfig) -> int:
    ny, nx = tile_grid(H, W, cfg)[:2]
    return ny * nx
