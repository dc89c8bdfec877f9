"""CPU checks of the 3x3 launch plans (csrc/conv3x3.hip: fwd_plan for forward / backward-data, wgrad_plan for backward-weights):
the host queries built on them answer without a GPU.  (a) uh_conv3x3_fwd_kernel against the selection rules as predict.py restated
them before the library exported them; (b) uh_conv3x3_dgrad_bnsum_rows and uh_conv3x3_wgrad_ws_bytes against the values the
library answered before the plans (tests/golden/conv3x3_plan_parent.json); (c) BatchPredictor.launch_lengths against the lengths
DESIGN.md section 3 records; (d) uh_conv3x3_wgrad_plan against the backward-weights rules as the dispatch held them before
wgrad_plan, restated here, and against the workspace sizes of (b)."""
import ctypes
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# B = 1..8 in fp32 and bf16, six image sizes at pyramid levels 0-5, the 3x3 conv channel pairs of UNet and UNet_S (either
# up-sampling) and of BASELINE config 4 (UNetDepth(3, 4, True, widths=(64, ..., 2048)))
SIZES = [(512, 512), (512, 384), (1000, 999), (700, 300), (1024, 1024), (62, 62)]
LEVELS = range(6)
PAIRS = [(1, 16), (1, 64), (3, 64), (16, 16), (16, 32), (32, 16), (32, 32), (32, 64), (64, 32), (64, 64), (64, 128), (128, 64),
         (128, 128), (128, 256), (256, 128), (256, 256), (256, 512), (512, 256), (512, 512), (512, 1024), (1024, 512),
         (1024, 1024), (2048, 1024)]


def _grid():
    hw = sorted({(H >> k, W >> k) for H, W in SIZES for k in LEVELS})
    return [(dt, B, h, w, cin, cout) for dt in (0, 1) for B in range(1, 9) for h, w in hw for cin, cout in PAIRS]


def _pinned_code(B, h, w, cin, cout, bf16):
    """The forward-kernel rules of BatchPredictor._conv3x3_variant (predict.py), kept verbatim as the expectation."""
    es = 2 if bf16 else 4
    if cout % 64 or cin % (64 // es):
        return 0
    if B * h * w * max(cin, cout) * es >= (1 << 31) - 4096:
        return 5                                                   # past the 2 GiB buffer window: the older kernel
    ntile = B * ((h + 15) // 16) * ((w + 15) // 16)
    if cout % 128 == 0 and ntile * (cout // 128) >= 512:
        return 1                                                   # 128-channel slabs
    if bf16 and cin == 64:
        return 2                                                   # register-resident filter
    nchunk = cin // 32
    if bf16 and cin % 32 == 0 and ntile * (cout // 64) <= 256 and nchunk >= 8 and nchunk % 2 == 0:
        return 3                                                   # K split over the two halves of the workgroup
    return 4


@pytest.fixture(scope="module")
def lib():
    import unet_amd  # noqa: F401
    from unet_amd._lib import LIB
    LIB.load()
    return LIB


def test_channel_pairs_are_those_of_the_models():
    import torch
    import unet_amd
    models = [unet_amd.UNet(1, 3, False), unet_amd.UNet(1, 3, True), unet_amd.UNet_S(1, 3, False), unet_amd.UNet_S(1, 3, True),
              unet_amd.UNetDepth(3, 4, True, widths=(64, 128, 256, 512, 1024, 2048))]
    pairs = {(m.in_channels, m.out_channels) for model in models for m in model.modules()
             if isinstance(m, torch.nn.Conv2d) and tuple(m.kernel_size) == (3, 3)}
    assert sorted(pairs) == PAIRS


def test_fwd_kernel_query_matches_the_pinned_rules(lib):
    seen = set()
    for dt, B, h, w, cin, cout in _grid():
        want = _pinned_code(B, h, w, cin, cout, dt == 1)
        got = lib.query("uh_conv3x3_fwd_kernel", B, h, w, cin, 0, cout, dt)
        assert got == want, (dt, B, h, w, cin, cout)
        # the filter may be packed fragment-major exactly when the LDS-DMA kernel (codes 1-4) runs the call
        assert lib.query("uh_conv3x3_wfrag_ok", B, h, w, cin, 0, cout, cin, 0, cout, dt) == (1 <= want <= 4)
        seen.add(got)
    assert seen == {0, 1, 2, 3, 4, 5}
    assert lib.query("uh_conv3x3_fwd_kernel", 8, 1024, 1024, 128, 0, 128, 1) == 5
    assert lib.query("uh_conv3x3_fwd_kernel", 1, 512 >> 4, 512 >> 4, 512, 0, 512, 1) == 3


def test_fwd_kernel_query_refuses_bad_arguments(lib):
    assert lib.query("uh_conv3x3_fwd_kernel", 0, 16, 16, 64, 0, 64, 1) < 0
    assert lib.query("uh_conv3x3_fwd_kernel", 1, 16, 16, 64, 0, 64, 7) < 0


def test_bnsum_rows_and_wgrad_workspace_unchanged(lib):
    with open(os.path.join(ROOT, "tests", "golden", "conv3x3_plan_parent.json")) as f:
        table = json.load(f)["table"]
    grid = _grid()
    assert len(table) * 8 == len(grid)
    for dt, B, h, w, cin, cout in grid:
        rows, ws = table[f"{dt},{h},{w},{cin},{cout}"]
        assert lib.query("uh_conv3x3_dgrad_bnsum_rows", B, h, w, cout, cin, cout, cin, cin, dt) == rows[B - 1], (dt, B, h, w, cin, cout)
        assert lib.query("uh_conv3x3_wgrad_ws_bytes", B, h, w, cin, cout, dt) == ws[B - 1], (dt, B, h, w, cin, cout)


def _pinned_wgrad_plan(B, h, w, c0, c1, cout, bf16, narrow):
    """The backward-weights rules of conv3x3_wgrad_dispatch as it stood before wgrad_plan (kind / nwr / nsplit, the 2 GiB test, the
    stem ladder, slab16, the reduce launches), for dense pitches and aligned pointers -> the eight words of uh_conv3x3_wgrad_plan."""
    es = 2 if bf16 else 4
    cin = c0 + c1
    n = cout * 9 * cin
    if c0 % 64 == 0 and cin % 64 == 0 and cout % 64 == 0:          # (the dense pitches of such counts are multiples of 16 bytes)
        ntile = B * ((w + 15) // 16) * ((h + 7) // 8)
        lim = (1 << 31) - 4096
        dma = bf16 and B * h * w * max(c0, c1) * 2 < lim and B * h * w * cout * 2 < lim
        nwr = 4 if dma and not narrow and cout % 128 == 0 else 2
        ctiles = (cin // 64) * (cout // (32 * nwr))
        want = -(-(256 if nwr == 4 else 512) // ctiles)
        nsplit = 1 if want < 1 else min(want, ntile)
        code, grid, threads = (4 if not dma else 6 if nwr == 4 else 5), (nsplit, ctiles), 128 * nwr
        slab16 = dma and os.environ.get("UH_WGRAD_SLAB_F32", "")[:1] != "1"
    elif cin <= 4 and c1 == 0:
        nsplit = min(1024, B * ((w + 15) // 16) * ((h + 15) // 16))
        dy_ok = (cout * es) % 16 == 0
        if bf16 and cout == 64 and dy_ok:
            code, grid = 3, (nsplit, cin)
        elif cout % (16 // es) == 0 and dy_ok:
            code, grid = 2, (nsplit, 1)
        else:
            code, grid = 1, (nsplit, (cout + 63) // 64)
        threads, slab16 = 256, False
    else:
        return [0, 0, cout * 9, 1, 256, 0, 0, 0]                     # the generic kernel: no slabs, no reduce
    if slab16:
        lanes = 32 if nsplit >= 256 else 16 if nsplit >= 128 else 8 if nsplit >= 64 else 4
        reduce, blocks = 4, ((n // 2 >> 2) + 256 // lanes - 1) // (256 // lanes)
    elif n % 4:
        reduce, blocks = 1, (n + 255) // 256
    else:
        reduce, blocks = 2, (n // 4 + 63) // 64
    return [code, nsplit, grid[0], grid[1], threads, int(slab16), reduce, blocks]


def _wgrad_plan(lib, B, h, w, c0, c1, cout, dt, narrow):
    out = (ctypes.c_int64 * 8)()
    assert lib.query("uh_conv3x3_wgrad_plan", B, h, w, c0, c1, cout, dt, narrow, ctypes.addressof(out)) == 0
    return list(out)


def test_wgrad_plan_query_matches_the_pinned_rules_and_the_workspace_sizes(lib):
    seen = set()
    for dt, B, h, w, cin, cout in _grid():
        plans = [_wgrad_plan(lib, B, h, w, cin, 0, cout, dt, 0)]
        assert plans[0] == _pinned_wgrad_plan(B, h, w, cin, 0, cout, dt == 1, False), (dt, B, h, w, cin, cout)
        if dt == 1 and plans[0][0] >= 4:                             # a narrow call is computed as its padded MFMA shape
            plans.append(_wgrad_plan(lib, B, h, w, cin, 0, cout, dt, 1))
            assert plans[1] == _pinned_wgrad_plan(B, h, w, cin, 0, cout, True, True), (dt, B, h, w, cin, cout)
        # the workspace: the larger of the plans a bf16 call can take (alignment and family are unknown when it is sized)
        assert lib.query("uh_conv3x3_wgrad_ws_bytes", B, h, w, cin, cout, dt) == max(p[1] for p in plans) * cout * 9 * cin * 4 + 16
        seen.update((dt, p[0]) for p in plans)
    # codes 1, 2 and 4-on-bf16 lie outside the models' grid: the fp32 stems without / with 16-byte output rows, and a bf16 tensor
    # past the 2 GiB window of a buffer descriptor
    for dt, B, h, w, cin, cout, code in [(0, 2, 20, 20, 3, 6, 1), (0, 2, 20, 20, 3, 64, 2), (1, 8, 1024, 1024, 128, 128, 4)]:
        got = _wgrad_plan(lib, B, h, w, cin, 0, cout, dt, 0)
        assert got == _pinned_wgrad_plan(B, h, w, cin, 0, cout, dt == 1, False) and got[0] == code, (dt, B, h, w, cin, cout)
        seen.add((dt, got[0]))
    assert {code for _, code in seen} == {0, 1, 2, 3, 4, 5, 6}
    assert (1, 4) in seen and (0, 4) in seen
    # two sources: the MFMA rules take both counts, the stem kernels take one source only
    assert _wgrad_plan(lib, 2, 17, 23, 64, 64, 64, 1, 0) == _pinned_wgrad_plan(2, 17, 23, 64, 64, 64, True, False)
    assert _wgrad_plan(lib, 2, 17, 23, 64, 64, 64, 1, 0)[0] == 5
    assert _wgrad_plan(lib, 2, 12, 14, 2, 2, 16, 0, 0)[0] == 0
    assert _wgrad_plan(lib, 2, 12, 14, 96, 32, 64, 1, 0)[0] == 0


def test_wgrad_plan_query_refuses_bad_arguments(lib):
    out = (ctypes.c_int64 * 8)()
    assert lib.query("uh_conv3x3_wgrad_plan", 0, 16, 16, 64, 0, 64, 1, 0, ctypes.addressof(out)) < 0
    assert lib.query("uh_conv3x3_wgrad_plan", 1, 16, 16, 64, 0, 64, 7, 0, ctypes.addressof(out)) < 0
    assert lib.query("uh_conv3x3_wgrad_plan", 1, 16, 16, 64, 0, 64, 1, 0, None) < 0


@pytest.mark.parametrize("ctor,args,want", [
    ("UNet_S", (1, 3, False), [8, 8, 2, 7]),
    ("UNet_S", (1, 3, True), [8, 8, 2, 7]),
    ("UNet_SA", (1, 3), [8, 8, 2, 7]),
    ("UNet", (1, 3), [1, 1, 1, 1]),
])
def test_launch_lengths_at_batch_8(lib, ctor, args, want):
    """profiles/predict_bench_line.json's sizes (H x W); the longest launch of each, bf16, batch 8."""
    import unet_amd
    from unet_amd.predict import LaunchPlanner
    p = LaunchPlanner(getattr(unet_amd, ctor)(*args), 8, True)          # no device: launch_lengths only asks the library
    got = [p.launch_lengths(H, W) for H, W in ((512, 512), (384, 512), (999, 1000), (700, 300))]
    assert got == [list(range(1, n + 1)) for n in want]
