"""The pixel passes compute bit for bit what they computed at the commit tests/golden/pixel_pass_forms_parent.json was recorded
at (9bd533e, before their entry points shared one launch plan), in every launch form: scalar, 16-byte channel groups with and
without hoisted coefficients, grids below and at the cap, every rung of the class / lanes-per-pixel ladder.  The cases and the
record's format are those of tests/golden/make_pixel_pass_forms.py, which this file replays.
Eight digests of the record are newer: `up`, `up_dx` and `up_dx_ptr` of flat.fp32.c3 and flat.bf16.c64.unaligned and `up_dx`, `up_dx_ptr`
of flat.bf16.c12 -- the one-channel forms of the bilinear pair, which were given the arithmetic of the 16-byte forms (they differed from
them by a bf16 ulp now and then: tests/test_gpu_exact_pixel.py) and were recorded again, twice, with every other digest unchanged.

Beside the replay, every case asks uh_pixel_pass_plan for the form its calls take and requires the one it was chosen for, so
that a shape which falls off its branch fails instead of passing trivially (host only: that part needs no GPU)."""
import ctypes
import importlib.util
import json
import os

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

_spec = importlib.util.spec_from_file_location("make_pixel_pass_forms", os.path.join(GOLDEN, "make_pixel_pass_forms.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

with open(os.path.join(GOLDEN, "pixel_pass_forms_parent.json")) as _f:
    PARENT = json.load(_f)


def test_the_parent_record_holds_every_case_and_dropped_nothing_element_wise():
    assert sorted(PARENT["cases"]) == sorted(rec.CASES)
    assert all(PARENT["cases"][name] for name in rec.CASES)
    assert not [d for d in PARENT["dropped_digests"] if not rec.reduced(d.split(":", 1)[1])]


@pytest.mark.parametrize("case", sorted(rec.CASES))
def test_every_case_takes_the_form_it_was_chosen_for(case):
    import unet_amd  # noqa: F401
    from unet_amd._lib import LIB
    for want in rec.CASES[case][2]:
        out = (ctypes.c_int64 * 3)()
        assert LIB.query("uh_pixel_pass_plan", want["items"], want["C"], want["dt"], want["aligned"], want["cap"], ctypes.addressof(out)) == 0
        vec, hoist, grid = out
        form = "scalar" if vec == 1 else "hoist" if hoist else "vector"
        assert vec in (1, 8 if want["dt"] == rec.BF16 else 4) and (vec > 1 or not hoist)
        assert grid <= want["cap"]
        assert form + ("_capped" if grid == want["cap"] else "") == want["form"], (want, list(out))


def test_the_cases_reach_every_form():
    forms = {p["form"] for _, _, plans in rec.CASES.values() for p in plans}
    assert forms == {"scalar", "vector", "hoist", "vector_capped", "hoist_capped"}
    names = set(rec.CASES)
    for dt in ("bf16", "fp32"):
        assert {f"head.{dt}.lpp{lpp}.ncls{n}" for lpp in (8, 16) for n in (1, 3, 4)} <= names
        assert any(k.startswith(f"c11.{dt}.") and k.endswith(".ncls8") for k in names)


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(rec.CASES))
def test_results_equal_the_parents(case):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    want = PARENT["cases"][case]
    got = rec.run_case(case)
    assert want and set(want) <= set(got)
    differ = [k for k, v in want.items() if got[k] != v]
    assert not differ, differ
