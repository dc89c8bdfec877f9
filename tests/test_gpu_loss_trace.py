"""The loss side asks of the C ABI exactly what it asked at the commit tests/golden/loss_call_trace_parent.json was recorded at
(ed0d3f5, before the loss nodes moved into losses.py and shared their plumbing and the kernels their head helpers): the same
launches with the same arguments in the same order, and bit-identical terms and gradients of the logits.  The cases and the
record's format are those of tests/golden/make_loss_call_trace.py, which this file replays."""
import importlib.util
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

_spec = importlib.util.spec_from_file_location("make_loss_call_trace", os.path.join(GOLDEN, "make_loss_call_trace.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

with open(os.path.join(GOLDEN, "loss_call_trace_parent.json")) as _f:
    PARENT = json.load(_f)

# Every loss entry point of include/unet_hip.h that launches: the record must hold each at least once, so that a case which falls
# off its branch fails instead of passing trivially.  (uh_surface_border_i64, the border masks as a tensor, has no caller among the
# package's public names: tests/test_gpu_surface_loss.py holds it.)
REQUIRED = ["uh_bce_dice_sums", "uh_bce_dice_grad", "uh_ce_dice_sums", "uh_ce_dice_grad", "uh_dice_sums", "uh_dice_from_sums",
            "uh_boundary_loss", "uh_boundary_loss_mask", "uh_seg_loss_binary_finish", "uh_seg_loss_binary_fused",
            "uh_seg_loss_multiclass_finish", "uh_surface_dist_map", "uh_surface_loss_sums", "uh_surface_loss_grad",
            "uh_focal_tversky_sums", "uh_focal_tversky_finish", "uh_focal_tversky_grad", "uh_distill_sums", "uh_distill_finish",
            "uh_distill_grad"]
# (entry point, index of ncls among its arguments) -> the heads the record must reach
HEADS = {("uh_ce_dice_sums", 3): {2, 3, 8}, ("uh_ce_dice_grad", 3): {2, 3, 8},
         ("uh_focal_tversky_sums", 4): {1, 2, 3, 4, 8}, ("uh_focal_tversky_grad", 4): {1, 2, 3, 4, 8},
         ("uh_surface_loss_sums", 5): {1, 3, 4, 8}, ("uh_surface_loss_grad", 5): {1, 3, 4, 8},
         ("uh_distill_sums", 3): {1, 2, 3, 4, 8}, ("uh_distill_grad", 3): {1, 2, 3, 4, 8}}


def test_the_parent_record_reaches_every_branch():
    assert sorted(PARENT["cases"]) == sorted(rec.CASES) and PARENT["extent"] == [list(s) for s in rec.SHAPES.values()]
    rows = [r for c in PARENT["cases"].values() for r in c["rows"]]
    names = {r[0] for r in rows}
    assert not [n for n in REQUIRED if n not in names]
    for (name, i), heads in HEADS.items():
        assert {r[1 + i] for r in rows if r[0] == name} >= heads, name
    assert {r[7] for r in rows if r[0] == "uh_focal_tversky_sums"} == set(rec.GAMMAS)
    # the three shapes, by pixel count, through a sums pass and a gradient pass of the shared launch code
    pixels = sorted(B * H * W for B, H, W in rec.SHAPES.values())
    assert sorted({r[4] for r in rows if r[0] == "uh_focal_tversky_grad"}) == pixels
    assert sorted({r[3] for r in rows if r[0] == "uh_distill_sums"}) == pixels
    assert sorted({r[5] for r in rows if r[0] == "uh_bce_dice_grad"}) == pixels
    # the data-parallel form: the mean over twice the pixels
    assert {r[6] / r[3] for r in rows if r[0] == "uh_ce_dice_grad"} == {1.0, 2.0}
    # no loss value or gradient is among the digests the two recording runs disagreed on
    assert PARENT["dropped_digests"] == []
    for name, c in PARENT["cases"].items():
        assert c["digests"], name
        if not name.startswith("functions."):
            assert any(k.endswith(".loss") for k in c["digests"]) and any(k.endswith(".grad") for k in c["digests"]), name


@pytest.mark.parametrize("case", sorted(rec.CASES))
def test_launch_record_and_results_equal_the_parents(case):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    want = PARENT["cases"][case]
    rows, digests = rec.run_case(case)
    for i, (a, b) in enumerate(zip(rows, want["rows"])):
        assert a == b, f"launch {i}: {a} != parent's {b}"
    assert len(rows) == len(want["rows"])
    assert want["digests"] and set(want["digests"]) == set(digests)
    differ = [k for k, v in want["digests"].items() if digests[k] != v]
    assert not differ, differ
