"""The inference routes -- BatchPredictor (plain, batch-invariant, test-time augmentation, tiled, ensembles), evaluate() and
ContourPipeline -- ask of the C ABI exactly what they asked at the commit tests/golden/predict_call_trace_parent.json was recorded
at (9d4a175, before views, tiles and members were composed in one place; the six cases from before ensembles existed still
equal their record of 5c34f76): the same launches with the same arguments in the
same order on the same streams, the same stage names in `events`, the same `graph_replays` and `launch_lengths`, and
bit-identical results.  The cases and the record's format are those of tests/golden/make_predict_call_trace.py, which this file
replays."""
import importlib.util
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

_spec = importlib.util.spec_from_file_location("make_predict_call_trace", os.path.join(GOLDEN, "make_predict_call_trace.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

PARENT = rec.load(os.path.join(GOLDEN, "predict_call_trace_parent.json"))      # (every launch spelled out again)

# entry points the record must hold at least once, so that a case which falls off its route fails instead of passing trivially
REQUIRED = ["uh_tta_views", "uh_tta_merge", "uh_tile_gather", "uh_tile_merge", "uh_predict_prepare_u8", "uh_batch_prepare",
            "uh_logits_to_classes_u8", "uh_postprocess_masks", "uh_classes_to_grey_u8", "uh_contours_emit", "uh_ensemble_add",
            "uh_ensemble_finish"]


def test_the_parent_record_reaches_every_route():
    cases = PARENT["cases"]
    assert sorted(cases) == sorted(rec.CASES) and not PARENT["dropped_digests"]
    names = {r[0] for c in cases.values() for r in c["rows"]}
    assert not [n for n in REQUIRED if n not in names]
    assert any(n.startswith("uh_conv3x3_") and n.endswith("_plan") for n in names), "no pinned-plan conv entry point"
    replays = [f["graph_replays"] for f in (cases["p1"]["facts"], cases["p2"]["facts"], cases["p3"]["facts"],
                                            cases["p4"]["facts"]["plain"], cases["p4"]["facts"]["flips"])]
    assert all(n > 0 for n in replays), replays
    # the ensemble routes replay their members' graphs too (p5 without views has groups of 2 and 3 at batch 4: no full launch)
    replays = {c: sum(f["graph_replays"] for tag, f in cases[c]["facts"].items() if tag != "levels") for c in ("p5", "p6")}
    assert all(n > 0 for n in replays.values()), replays
    assert cases["p5"]["facts"]["d4"]["graph_replays"] > 0
    assert all(cases["p6"]["facts"][t]["graph_replays"] > 0 for t in ("plain", "flips"))
    # the plain route cut a batch: more launches (one uh_predict_prepare_u8 each) than planned batches, three passes over the images
    p1 = cases["p1"]
    launches = [r[4] for r in p1["rows"] if r[0] == "uh_predict_prepare_u8"]
    planned = p1["facts"]["planned_batches"]
    assert 4 not in p1["facts"]["launch_lengths"]["48x64"] and 4 in planned
    assert len(launches) > 3 * len(planned) and sum(launches) == 3 * sum(planned)
    p2 = [r[4] for r in cases["p2"]["rows"] if r[0] == "uh_predict_prepare_u8"]
    assert p2 == 3 * cases["p2"]["facts"]["planned_batches"]                     # batch-invariant: one launch per planned batch
    # the class maps are not constant, every evaluate and pipeline result is there, and the full pipeline batch is graphed (stream 1)
    assert max(p1["facts"]["levels"]) >= 2 and max(cases["p3"]["facts"]["levels"]) == 3 and max(cases["p4"]["facts"]["levels"]) >= 2
    assert max(cases["p5"]["facts"]["levels"]) >= 2 and max(cases["p6"]["facts"]["levels"]) >= 2
    assert len(cases["e1"]["digests"]) == 16 and len(set(cases["e1"]["digests"].values())) > 8
    assert len(cases["e2"]["digests"]) == 16 and len(set(cases["e2"]["digests"].values())) > 8
    assert len(cases["s1"]["digests"]) == 30
    assert any(r[-1] == 1 for r in cases["s1"]["rows"] if r[0] == "uh_conv1x1_fwd")
    for tag in ("default", "invariant"):
        assert cases["s1"]["facts"][tag]["events"][:7] == ["window", "letterbox", "forward", "argmax", "postprocess", "unletterbox",
                                                          "contours"]


@pytest.mark.parametrize("case", sorted(rec.CASES))
def test_launch_record_and_results_equal_the_parents(case):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    want = PARENT["cases"][case]
    got = rec.run_case(case)
    for i, (a, b) in enumerate(zip(got["rows"], want["rows"])):
        assert a == b, f"launch {i}: {a} != parent's {b}"
    assert len(got["rows"]) == len(want["rows"])
    assert got["facts"] == want["facts"]                       # stage names in order, graph_replays, launch_lengths
    assert want["digests"] and set(want["digests"]) == set(got["digests"])
    differ = [k for k, v in want["digests"].items() if got["digests"][k] != v]
    assert not differ, differ
