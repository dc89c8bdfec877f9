"""Test-time augmentation: the eight poses of the square (the dihedral group D4) as views of an image, and the named
subgroups that predict / evaluate average over (DESIGN.md section 3 "Test-time augmentation").  Pure Python, no GPU.

A view is v = 4 t + 2 fy + fx, applied to an H x W image x as "flip, then transpose":
    t = 0: the view is H x W,  view[i][j] = x[H-1-i if fy else i][W-1-j if fx else j]
    t = 1: the view is W x H,  view[i][j] = x[H-1-j if fy else j][W-1-i if fx else i]
so a source pixel (y, x) lies in view v at (yy, xx) for t = 0 and at (xx, yy) for t = 1, with yy = H-1-y if fy else y and
xx = W-1-x if fx else x.  A mode is a set of views stored as a bit mask over v.  Only a set that is closed under composition
(a subgroup) makes the averaged prediction of a posed image the posed prediction of the image, so nothing else is taken."""
from __future__ import annotations

from typing import List, Tuple

MODES = {
    "hflip": 0x03,      # {0, 1}
    "flips": 0x0F,      # {0, 1, 2, 3}
    "rot4": 0x69,       # {0, 3, 5, 6}: the four quarter turns, the poses BasicDataset serves (rotation_idx = idx % 4)
    "d4": 0xFF,         # {0 .. 7}
}
DEFAULT_MODE = "d4"     # a bare --tta


def tta_mask(mode) -> int:
    """Bit mask over v of a named mode (or of a mask that is one of the four); ValueError for anything else."""
    if isinstance(mode, str):
        if mode in MODES:
            return MODES[mode]
    elif isinstance(mode, int) and not isinstance(mode, bool) and mode in MODES.values():
        return mode
    raise ValueError(f"unknown test-time augmentation mode {mode!r}: one of {', '.join(MODES)} (a closed set of views)")


def tta_view_list(mode) -> List[int]:
    mask = tta_mask(mode)
    return [v for v in range(8) if mask >> v & 1]


def tta_counts(mode) -> Tuple[int, int]:
    """(K0, K1): how many views of the mode keep the image's shape, how many transpose it."""
    views = tta_view_list(mode)
    return sum(1 for v in views if v < 4), sum(1 for v in views if v >= 4)


def _check_view(v: int) -> int:
    if not isinstance(v, int) or not 0 <= v < 8:
        raise ValueError(f"a view is an integer 0..7, got {v!r}")
    return v


def tta_view_shape(v: int, H: int, W: int) -> Tuple[int, int]:
    return (W, H) if _check_view(v) & 4 else (H, W)


def tta_source_position(v: int, H: int, W: int, y: int, x: int) -> Tuple[int, int]:
    """Where the source pixel (y, x) of an H x W image lies in its view v."""
    _check_view(v)
    if not (0 <= y < H and 0 <= x < W):
        raise ValueError(f"pixel ({y}, {x}) is outside a {H} x {W} image")
    yy = H - 1 - y if v & 2 else y
    xx = W - 1 - x if v & 1 else x
    return (xx, yy) if v & 4 else (yy, xx)


def tta_forward_views(mode, H: int, W: int) -> int:
    """Views of one source image that share a forward launch: all of them when the image is square (one view shape), the
    larger of K0 and K1 otherwise (the H x W views and the W x H views are two launches)."""
    k0, k1 = tta_counts(mode)
    return k0 + k1 if H == W else max(k0, k1)
