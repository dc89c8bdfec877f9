"""CPU companion of tests/test_gpu_bn_stats.py: the references, conditions and bounds of tests/bn_stats_cases.py, proved without a GPU.

Part A (finalize and eval coefficients on synthetic rows):
  * the exact rational reference is what float64 torch.nn.BatchNorm2d computes on a pixel population with those rows;
  * the dyadic family meets every condition at every shape the GPU file runs, and a float64 restatement of bn_finalize_kernel then
    equals the expected outputs bit for bit; on the general family the restatement stays inside the derived bounds, and the double
    term of every bound is below 1/16 of the float32 rounding next to it (asserted in general_bounds);
  * each seeded mistake of finalize_restated breaks the comparison of at least the case made for it.
Part B (the rows of the conv kernels): every case meets the integer conditions of its producer's arithmetic, a float32 restatement
of each producer stays inside the derived bound, and each planted error moves some channel outside it."""
from fractions import Fraction as Fr

import numpy as np
import pytest
import torch

import bn_stats_cases as BC

F = np.float32
KEYS = ("scale", "shift", "mean", "rstd", "m2_out", "running_mean", "running_var")


def test_round_f32():
    rng = np.random.default_rng(1)
    for x in rng.standard_normal(200) * 10.0 ** rng.uniform(-5, 5, 200):
        assert BC.round_f32(Fr(float(x))) == F(x)
    # a tie that a trip through float64 would break the wrong way: 1 + 2^-24 + 2^-60 lies above the midpoint of 1 and 1 + 2^-23
    x = Fr(1) + Fr(1, 2 ** 24) + Fr(1, 2 ** 60)
    assert F(float(x)) == F(1) and BC.round_f32(x) == np.nextafter(F(1), F(2))
    assert BC.round_f32(Fr(1) + Fr(1, 2 ** 24)) == F(1) and BC.round_f32(-(Fr(1) + Fr(3, 2 ** 24))) == -(F(1) + F(2.0 ** -22))


def _bits(a):
    return np.asarray(a, F).view(np.uint32)


def _differs_dyadic(got, want):
    return [k for k in KEYS if not np.array_equal(_bits(got[k]), _bits(want[k]))]


def _differs_general(got, val, tol):
    return [k for k in KEYS if not bool((np.abs(got[k].astype(np.float64) - val[k]) <= tol[k]).all())]


@pytest.mark.parametrize("case", BC.FIN_CASES, ids=lambda c: c.name)
def test_finalize_dyadic_family(case):
    inp = BC.dyadic_rows(case)
    ex = BC.finalize_exact(inp)
    BC.assert_dyadic_conditions(inp, ex)
    dead = inp["counts"] == 0
    assert np.isnan(inp["mean"][dead]).all() and np.isnan(inp["m2"][dead]).all() and not np.isnan(inp["mean"][~dead]).any()
    buf = BC.pack_stats(inp, case.ldc)
    assert buf.shape == (case.nslab * (2 * case.ldc + 1),) and np.array_equal(buf[case.nslab * 2 * case.ldc:], inp["counts"])
    if case.ldc > case.C:
        assert np.isnan(buf[:case.nslab * 2 * case.ldc].reshape(case.nslab, 2, case.ldc)[:, :, case.C:]).all()
    if case.dead == "tail":
        assert inp["n_pass"] == inp["counts"][:BC.BNF_FAST].sum()                     # the kernel skips its walk
    if case.dead == "head":
        assert inp["counts"][:BC.BNF_FAST].sum() == 0
    want = BC.dyadic_expected(inp, ex)
    assert _differs_dyadic(BC.finalize_restated(inp, case.nslab), want) == []
    for c in range(case.C):
        if c % 5 == 4 and inp["eps"] > 0:
            assert want["m2_out"][c] == 0 and want["rstd"][c] == 256


@pytest.mark.parametrize("case", BC.FIN_CASES, ids=lambda c: c.name)
def test_finalize_general_family(case):
    inp = BC.general_rows(case)
    ex = BC.finalize_exact(inp)
    val, tol = BC.general_bounds(inp, ex, case.nslab)                                 # (asserts that the double term is negligible)
    assert _differs_general(BC.finalize_restated(inp, case.nslab), val, tol) == []
    for k in ("mean", "m2_out", "rstd", "scale"):                                      # a few units of float32 rounding, no more
        assert bool((tol[k] <= 2.2 * BC.U * np.abs(val[k])).all()), k
    if not (inp["counts"][0] == 0) and case.C >= 2:
        c = 1                                                                          # mean 1e4, standard deviation 0.1
        assert abs(val["mean"][c]) > 9e3 and val["m2_out"][c] / float(ex[c]["N"]) < 0.1


@pytest.mark.parametrize("name", ["rows65-scattered", "rows1025-none", "syncbn-world8-counted", "C3-ldc64-rows65"])
@pytest.mark.parametrize("family", sorted(BC.FAMILIES))
def test_exact_reference_is_batchnorm(name, family):
    """finalize_exact + the formulas of general_bounds against float64 torch.nn.BatchNorm2d in training mode on pixels that have
    exactly those rows: a relative 1e-11 (float64 on both sides; the large-mean channel cancels by 1e10 in torch's variance, so
    its variance is compared at 1e-4 there)."""
    case = BC.FIN_BY_NAME[name]
    inp = BC.FAMILIES[family](case)
    ex = BC.finalize_exact(inp)
    for c in range(min(case.C, 4)):
        x, dropped = BC.expand_pixels(inp, c)
        bn = torch.nn.BatchNorm2d(1, eps=float(inp["eps"]), momentum=float(inp["momentum"])).double()
        with torch.no_grad():
            bn.running_mean.fill_(float(inp["running_mean"][c]))
            bn.running_var.fill_(float(inp["running_var"][c]))
        bn.train()
        xt = torch.from_numpy(x).view(1, 1, -1, 1)
        bn(xt)
        n = len(x)
        assert n == ex[c]["N"]
        mean, M2 = float(ex[c]["mean"]), float(ex[c]["M2"]) - dropped
        mom = float(inp["momentum"])
        rel_var = 1e-4 if abs(mean) > 1e3 else 1e-11
        assert abs(float(xt.mean()) - mean) <= 1e-11 * max(abs(mean), 1e-3)
        assert abs(float(xt.var(unbiased=False)) * n - M2) <= rel_var * M2 + 1e-300
        assert abs(float(bn.running_mean) - ((1 - mom) * float(inp["running_mean"][c]) + mom * mean)) <= 1e-11 * (abs(mean) + 1)
        want_rv = (1 - mom) * float(inp["running_var"][c]) + mom * M2 / (n - 1)
        assert abs(float(bn.running_var) - want_rv) <= rel_var * want_rv
        assert int(bn.num_batches_tracked) == 1


# the seeded mistakes, and the cases that are there to catch each
MISTAKES = {
    "dead_rows_counted": ("rows65-scattered", "rows2500-head", "rows2-first_dead"),
    "no_walk": ("rows1025-none", "rows2500-head", "rows2048-scattered"),
    "walk_skips_partial": ("rows1025-none", "rows2500-none", "rows2500-head"),
    "n_ignored": ("n_twice-rows65", "n_one-rows1025", "syncbn-world2-twice"),
    "biased_running": ("rows2-none", "rows65-scattered", "syncbn-world8-counted"),
    "pivot_dead_row": ("rows2-first_dead", "rows2500-first_dead"),
    "eps_outside": ("rows65-scattered", "C130-rows65"),
}


@pytest.mark.parametrize("mistake,name", [(m, n) for m, names in MISTAKES.items() for n in names])
def test_finalize_seeded_mistakes_are_caught(mistake, name):
    case = BC.FIN_BY_NAME[name]
    inp = BC.dyadic_rows(case)
    ex = BC.finalize_exact(inp)
    assert _differs_dyadic(BC.finalize_restated(inp, case.nslab, mistake), BC.dyadic_expected(inp, ex)) != [], "dyadic family"
    inp = BC.general_rows(case)
    ex = BC.finalize_exact(inp)
    val, tol = BC.general_bounds(inp, ex, case.nslab)
    assert _differs_general(BC.finalize_restated(inp, case.nslab, mistake), val, tol) != [], "general family"


def test_a_wrong_last_bit_is_caught():
    """One unit in the last place of any output of any channel fails the dyadic comparison (it is an equality of bit patterns)."""
    case = BC.FIN_BY_NAME["rows65-scattered"]
    inp = BC.dyadic_rows(case)
    want = BC.dyadic_expected(inp, BC.finalize_exact(inp))
    for k in KEYS:
        got = {q: v.copy() for q, v in want.items()}
        got[k][case.C - 1] = np.nextafter(got[k][case.C - 1], F(np.inf))
        assert _differs_dyadic(got, want) == [k]


@pytest.mark.parametrize("C", BC.EVAL_C)
def test_eval_coeffs_families(C):
    inp = BC.eval_inputs(C, "dyadic")
    scale, shift, ts, tsh = BC.eval_expected(inp, "dyadic")                            # (asserts exactness)
    assert not ts.any() and not tsh.any() and len(set(np.abs(scale / inp["gamma"]))) == (4 if C > 1 else 1)
    inp = BC.eval_inputs(C, "general")
    scale, shift, ts, tsh = BC.eval_expected(inp, "general")
    with np.errstate(all="ignore"):
        sc = (inp["gamma"] / np.sqrt(inp["running_var"] + inp["eps"])).astype(F)      # float32 throughout, as the kernel
        sh = inp["beta"] - inp["running_mean"] * sc
    assert sc.dtype == F and sh.dtype == F
    assert bool((np.abs(sc - scale) <= ts).all()) and bool((np.abs(sh - shift) <= tsh).all())
    # discrimination: eps left out, or added behind the root, is outside the bound
    bad = (inp["gamma"] / np.sqrt(inp["running_var"])).astype(F)
    assert not bool((np.abs(bad - scale) <= ts).all())


# ------------------------------------------------------------------------------------------------ B. the rows of the conv kernels
def _rows_setup(shape, family, bf16, code):
    c = BC.family_case(shape, family)
    plan = BC.rows_plan(shape, bf16, code)
    y, y_ext = BC.stored(c.y, bf16), BC.stored(c.y_ext, bf16)
    tol = BC.row_bounds(y, y_ext, shape[:3], plan, BC.v2_lanes(shape[5], bf16))
    return c, plan, y, y_ext, tol


def _restated_rows(y, y_ext, shape3, plan, bf16, Cout, use_pivot=True):
    n_r, _, _ = BC.row_counts(shape3, plan["lanes"])
    if plan["producer"] in ("mfma", "stem_v3"):
        S1, S2, pv = BC.restate_pivot(y, BC.pivots(y_ext, shape3, plan), plan["lanes"], plan["producer"], use_pivot)
        return (n_r,) + BC.finish_pivot(S1, S2, pv, n_r, plan["producer"])
    return (n_r,) + BC.restate_two_pass(y, shape3, plan["producer"], BC.v2_lanes(Cout, bf16))


def _outside(rows, want, tol):
    mean, m2 = BC.merge_rows(*rows)
    return bool((np.abs(mean - want[0]) > tol[0]).any()) or bool((np.abs(m2 - want[1]) > tol[1]).any())


def test_rows_cases_cover_every_producer_and_form():
    import test_gpu_exact as G
    assert [c[:3] for c in BC.ROWS_CASES[:BC.N_FWD_CASES]] == G.FWD_CASES
    assert all(c[3] == G.FAMILIES for c in BC.ROWS_CASES[:BC.N_FWD_CASES])
    seen ={(BC.rows_plan(s, bf16, code)["producer"], code) for s, fam, bf16, code in BC.rows_params()}
    assert seen == {("tile_stats", 0), ("stem_v1", 0), ("stem_v2", 0), ("stem_v3", 0), ("mfma", 1), ("mfma", 2), ("mfma", 3), ("mfma", 4)}
    flat = {(BC.rows_plan(s, bf16, code)["producer"], code) for s, fam, bf16, code in BC.rows_params() if fam == "flat"}
    assert flat == seen                                                               # a bit-exact row for every arithmetic and form
    big = [s for s, _, _, _ in BC.rows_params() if s[1] * s[2] > 128 * 128]
    assert set(big) == {(1, 448, 448, 64, 0, 64)}
    plan = BC.rows_plan((1, 448, 448, 64, 0, 64), True, 2)
    assert plan["lanes"] == 512 < plan["ntile"] == 784                                 # rows of two tiles and rows of one
    assert BC.rows_plan(BC.CHAIN_SHAPE, False, 0) == dict(producer="stem_v2", lanes=1089, ntile=1089)
    assert BC.rows_plan(BC.CHAIN_SHAPE, True, 0) == dict(producer="stem_v3", lanes=1024, ntile=1089)


@pytest.mark.parametrize("shape,family,bf16,code", BC.rows_params() + BC.chain_params(), ids=BC.rows_id)
def test_rows_bounds_hold_and_discriminate(shape, family, bf16, code):
    """For every case of the GPU file: the reference rows merge to the moments of the whole tensor; a float32 restatement of the
    producer is inside the derived bound; each planted error is outside it for some channel."""
    c, plan, y, y_ext, (tol_mean, tol_m2, cond) = _rows_setup(shape, family, bf16, code)
    shape3, lanes = shape[:3], plan["lanes"]
    want = BC.whole_moments(y)
    tol = (tol_mean, tol_m2)
    ref = BC.reference_rows(y, lanes)
    n_r, k_r, per_tile = BC.row_counts(shape3, lanes)
    assert np.array_equal(ref[0], n_r) and n_r.sum() == shape[0] * shape[1] * shape[2] and k_r.sum() == plan["ntile"]
    mean, m2 = BC.merge_rows(*ref)
    assert bool((np.abs(mean - want[0]) <= 1e-12 * (1 + np.abs(want[0]))).all()) and bool((np.abs(m2 - want[1]) <= 1e-11 * want[1] + 1e-9).all())
    assert not _outside(ref, want, tol)
    # the producer in float32
    got = _restated_rows(y, y_ext, shape3, plan, bf16, shape[5])
    gm, g2 = BC.merge_rows(*got)
    assert bool((np.abs(gm - want[0]) <= tol_mean).all()) and bool((np.abs(g2 - want[1]) <= tol_m2).all()), \
        (float((np.abs(gm - want[0]) / tol_mean).max()), float((np.abs(g2 - want[1]) / np.maximum(tol_m2, 1e-300)).max()))
    if family == "flat":
        em, e2 = BC.flat_rows_exact(y, shape3, plan, y_ext)
        assert np.array_equal(got[1].astype(F), em) and np.array_equal(got[2].astype(F), e2)
    # planted errors: one pixel of a partial border tile (the last partial tile; the last tile where all are full) dropped / twice
    T, M = BC.to_tiles(y)
    partial = np.flatnonzero((per_tile < 256) & (per_tile > 1))                        # (a one-pixel tile would lose its row)
    t = int(partial[-1]) if len(partial) else len(per_tile) - 1
    px = int(np.flatnonzero(M[t])[-1])
    for times in (0.0, 2.0):
        wt = M.astype(np.float64)
        wt[t, px] = times
        assert _outside(BC.reference_rows(y, lanes, wt), want, tol), f"pixel counted {times:.0f} times"
    # a row taken from the neighbouring channel, or from the other half of a PERM2 pair (channels c and c ^ 4)
    C = shape[5]
    for name, perm in (("neighbour", np.arange(C) ^ 1), ("PERM2 half", np.arange(C) ^ 4)):
        if perm.max() < C:
            moved = (ref[0], ref[1].copy(), ref[2].copy())
            moved[1][0], moved[2][0] = ref[1][0][perm], ref[2][0][perm]                # row 0 alone
            assert _outside(moved, want, tol), name
    # the moments of the unrounded accumulator
    if bf16:
        y_acc = BC.stored(c.y, False)
        if not np.array_equal(y_acc, y):
            assert _outside(BC.reference_rows(y_acc, lanes), want, tol), "unrounded accumulator"
        else:
            assert family != "wide"                                                    # the wide family does round in bf16
    if family == "flat_large":
        plain = _restated_rows(y, y_ext, shape3, plan, bf16, C, use_pivot=False)
        assert _outside(plain, want, tol), "plain sums without a pivot"
        assert float(np.abs(want[0]).min()) > 100 and float((want[1] / n_r.sum()).max()) < 40
