"""The conv + BatchNorm + ReLU nodes of ops.py ask of the C ABI exactly what they asked at the commit
tests/golden/ops_call_trace_parent.json was recorded at (9ea1231, before the nodes shared their BatchNorm plumbing): the same
launches with the same arguments in the same order on the same streams, and bit-identical results.  The cases and the record's
format are those of tests/golden/make_ops_call_trace.py, which this file replays."""
import importlib.util
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

_spec = importlib.util.spec_from_file_location("make_ops_call_trace", os.path.join(GOLDEN, "make_ops_call_trace.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

with open(os.path.join(GOLDEN, "ops_call_trace_parent.json")) as _f:
    PARENT = json.load(_f)

# entry points the record must hold at least once, so that a case which falls off its branch fails instead of passing trivially
REQUIRED = ["uh_stem_stats", "uh_bn_relu_pool_apply", "uh_bn_relu_upsample2x_fwd", "uh_bn_relu_head_fwd", "uh_conv3x3_dgrad_bnsum",
            "uh_conv3x3_fwd_narrow", "uh_conv3x3_wgrad_narrow", "uh_bn_finalize_ld", "uh_unpack_dw3x3", "uh_conv3x3_fwd_affine_relu",
            "uh_conv3x3_fwd_affine_relu_plan", "uh_conv3x3_fwd_narrow_plan", "uh_bn_bwd_finalize"]
# ... and these with a NULL partials pointer (argument index in include/unet_hip.h): the SyncBN form
REQUIRED_NULL_PARTIALS = {"uh_bn_relu_bwd_apply": 8, "uh_bn_relu_pool_bwd_apply": 10, "uh_bn_relu_head_bwd_apply": 8}


def test_the_parent_record_reaches_every_branch():
    assert sorted(PARENT["cases"]) == sorted(rec.CASES) and tuple(PARENT["extent"]) == rec.EXTENT
    rows = [r for c in PARENT["cases"].values() for r in c["rows"]]
    names = {r[0] for r in rows}
    assert not [n for n in REQUIRED if n not in names]
    for name, i in REQUIRED_NULL_PARTIALS.items():
        assert any(r[0] == name and r[1 + i] == 0 for r in rows), name
    assert any(r[-1] == 1 for r in PARENT["cases"]["a"]["rows"] if r[0] == "uh_conv3x3_wgrad"), "no side-stream backward-weights"
    for name, c in PARENT["cases"].items():
        if name == "g":          # the eval forwards: outputs only
            assert len(c["digests"]) == 6
            continue
        assert "loss" in c["digests"] and "logits" in c["digests"], name
        assert "flat_g" in c["digests"] or any(k.startswith("grad.") and k.endswith("double_conv.0.weight") for k in c["digests"]), name


@pytest.mark.parametrize("case", sorted(rec.CASES))
def test_launch_record_and_results_equal_the_parents(case):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    want = PARENT["cases"][case]
    rows, digests = rec.run_case(case)
    for i, (a, b) in enumerate(zip(rows, want["rows"])):
        assert a == b, f"launch {i}: {a} != parent's {b}"
    assert len(rows) == len(want["rows"])
    assert want["digests"] and set(want["digests"]) <= set(digests)
    differ = [k for k, v in want["digests"].items() if digests[k] != v]
    assert not differ, differ


def test_backward_through_an_eval_mode_layer_names_the_reason():
    import unet_amd
    dev = torch.device("cuda:0")
    block = unet_amd.DoubleConv(64, 64).to(dev).eval()
    x = torch.randn(1, 64, 8, 8, device=dev, requires_grad=True)
    with pytest.raises(RuntimeError, match="backward through eval-mode BatchNorm is not part of the train path"):
        block(x).sum().backward()
