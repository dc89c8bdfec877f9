"""CPU check of the pixel-pass launch plan (csrc/uh_launch.h: uh_pixel_pass, the one plan behind the BatchNorm + ReLU, pool-tail,
max-pool, bilinear x2 and 1x1 entry points): the host query uh_pixel_pass_plan answers without a GPU, and must answer what the
entry points decided each for themselves before they shared the plan -- grid_for (bn.hip), bf_grid (bn_fused.hip) and pu_grid
(pool_up.hip) at 4096 workgroups, ct_grid (convt_1x1.hip) at 8192, and the hoist condition -- restated here.

A grid-stride kernel gives the same bits at any grid, so a wrong grid or a needlessly dropped hoist would show only as lost
speed on the device; a wrongly GRANTED hoist corrupts results, but only once the grid is capped."""
import ctypes

import pytest

from test_conv_plan_cpu import LEVELS, SIZES

CHANNELS = [3, 8, 12, 24, 64, 128, 256, 512, 1024]
CAPS = [256 * 16, 256 * 32]


def _clamped_grid(total, cap):
    """grid_for / bf_grid / pu_grid (cap 4096) and ct_grid (cap 8192), as each file spelled it."""
    g = (total + 255) // 256
    if g > cap:
        g = cap
    if g < 1:
        g = 1
    return g


def _pinned_plan(items, C, bf16, aligned, cap):
    """The vector ladder of the entry points before the shared plan -> [vec, hoist, grid]."""
    VEC = 8 if bf16 else 4
    if aligned and C % VEC == 0:                                   # uh_vec_ok of every tensor of the call
        G = C // VEC
        g = _clamped_grid(items * G, cap)
        return [VEC, int((g * 256) % G == 0), g]
    return [1, 0, _clamped_grid(items * C, cap)]                   # the scalar kernels have no hoisted form


@pytest.fixture(scope="module")
def lib():
    import unet_amd  # noqa: F401
    from unet_amd._lib import LIB
    LIB.load()
    return LIB


def _plan(lib, items, C, dt, aligned, cap):
    out = (ctypes.c_int64 * 3)()
    assert lib.query("uh_pixel_pass_plan", items, C, dt, aligned, cap, ctypes.addressof(out)) == 0
    return list(out)


def _items():
    """Pixel counts of the six image sizes at levels 0..5 for B = 1..8, and the quartered counts (2x2 windows)."""
    hw = sorted({(H >> k, W >> k) for H, W in SIZES for k in LEVELS})
    pixels = {B * h * w for B in range(1, 9) for h, w in hw}
    return sorted(pixels | {B * (h // 2) * (w // 2) for B in range(1, 9) for h, w in hw if h >= 2 and w >= 2})


def test_plan_query_matches_the_pinned_rules_and_reaches_every_outcome(lib):
    seen = set()
    for dt in (0, 1):
        for aligned in (0, 1):
            for C in CHANNELS:
                for items in _items():
                    for cap in CAPS:
                        want = _pinned_plan(items, C, dt == 1, aligned, cap)
                        assert _plan(lib, items, C, dt, aligned, cap) == want, (dt, aligned, C, items, cap)
                        vec, hoist, grid = want
                        seen.add("scalar" if vec == 1 else "hoist" if hoist else "vector at the cap" if grid == cap else "vector below the cap")
    assert seen == {"scalar", "hoist", "vector at the cap", "vector below the cap"}


def test_a_capped_grid_hoists_only_where_the_stride_keeps_the_channel_group(lib):
    # 360 448 pixels x 3 groups of 8 bf16 channels: 4096 x 256 threads stride by 1 048 576 = 1 mod 3 -- every thread changes its group
    assert _plan(lib, 2 * 512 * 352, 24, 1, 1, 4096) == [8, 0, 4096]
    # 8 groups: the same stride is a multiple of 8
    assert _plan(lib, 2 * 256 * 272, 64, 1, 1, 4096) == [8, 1, 4096]
    # the windows of the first extent fit below the cap: one element per thread, hoisted
    assert _plan(lib, 2 * 256 * 176, 24, 1, 1, 4096) == [8, 1, 1056]
    # unaligned tensors, or a channel count that is no multiple of 16 bytes, take the scalar form and never hoist
    assert _plan(lib, 120, 64, 1, 0, 4096) == [1, 0, 30]
    assert _plan(lib, 120, 12, 1, 1, 4096) == [1, 0, 6]
    assert _plan(lib, 120, 12, 0, 1, 4096) == [4, 0, 2]


def test_plan_query_refuses_bad_arguments(lib):
    out = (ctypes.c_int64 * 3)()
    assert lib.query("uh_pixel_pass_plan", 0, 64, 1, 1, 4096, ctypes.addressof(out)) < 0
    assert lib.query("uh_pixel_pass_plan", 120, 0, 1, 1, 4096, ctypes.addressof(out)) < 0
    assert lib.query("uh_pixel_pass_plan", 120, 64, 7, 1, 4096, ctypes.addressof(out)) < 0
    assert lib.query("uh_pixel_pass_plan", 120, 64, 1, 1, 0, ctypes.addressof(out)) < 0
    assert lib.query("uh_pixel_pass_plan", 120, 64, 1, 1, 4096, None) < 0
