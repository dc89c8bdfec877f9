"""CPU checks of the 3x3 forward / backward-data launch plan (csrc/conv3x3.hip: fwd_plan): the host queries built on it answer
without a GPU.  (a) uh_conv3x3_fwd_kernel against the selection rules as predict.py restated them before the library exported
them; (b) uh_conv3x3_dgrad_bnsum_rows and uh_conv3x3_wgrad_ws_bytes against the values the library answered before the plan
(tests/golden/conv3x3_plan_parent.json); (c) BatchPredictor.launch_lengths against the lengths DESIGN.md section 3 records."""
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


@pytest.mark.parametrize("ctor,args,want", [
    ("UNet_S", (1, 3, False), [8, 8, 2, 7]),
    ("UNet_S", (1, 3, True), [8, 8, 2, 7]),
    ("UNet_SA", (1, 3), [8, 8, 2, 7]),
    ("UNet", (1, 3), [1, 1, 1, 1]),
])
def test_launch_lengths_at_batch_8(lib, ctor, args, want):
    """profiles/predict_bench_line.json's sizes (H x W); the longest launch of each, bf16, batch 8."""
    import unet_amd
    from unet_amd.predict import BatchPredictor
    p = object.__new__(BatchPredictor)          # no device: launch_lengths only asks the library
    p.model, p.batch, p.amp, p._lengths, p._layer_levels = getattr(unet_amd, ctor)(*args), 8, True, {}, None
    got = [p.launch_lengths(H, W) for H, W in ((512, 512), (384, 512), (999, 1000), (700, 300))]
    assert got == [list(range(1, n + 1)) for n in want]
