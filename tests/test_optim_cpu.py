"""CPU proof that tests/test_gpu_optim.py is as sharp as it claims, at every case it runs (the lists are tests/optim_cases.py's):
(a) a numpy float32 restatement of the statements of csrc/optim.hip, every operation rounded on its own, stays within K / 2 of
the float64 reference where the kernels are given K, and reaches the floor below the normal range where the case is built to;
(b) the integer gradients sum exactly in float32 in any order, the restated sum of squares meets half its bound on the random
ones, and the probes see a dropped and a doubled element; (c) oracle/step_ref.py, given stock torch's doubles, equals
torch.optim.RMSprop with clip_grad_norm_ in float64, and the float32 clip coefficient is step_ref.clip_coef within two roundings;
(d) uh_grad_sumsq and uh_rmsprop_step refuse bad arguments before any launch; (e) each seeded mistake, applied to the
restatement, breaks a bound at the cases named here."""
import numpy as np
import pytest
import torch

import optim_cases as K
from exact_inputs import require_exact_sum
from oracle import step_ref as S

F = np.float32
_name = lambda c: c.name      # noqa: E731


def _run(case, mistake=None, at=None):
    x, h = K.step_inputs(case), K.HYPERS[case.hyper]
    ref = K.step_reference(x, K.coef32(case.norm, case.max_norm), h)           # the reference keeps the right coefficient
    got = K.step_f32(x, K.coef32(case.norm, case.max_norm, mistake), h, mistake, at)
    return x, ref, got, K.step_units(got, x, ref, h)


# ------------------------------------------------------------------------------------------------ (a) the restatement
def test_the_constants_are_what_the_docstrings_derive():
    assert (K.K_S, K.K_B, K.K_P) == (19, 10, 8) and (K.SHARP_S, K.SHARP_B) == (2.01, 2.01) and K.SUMSQ_ULPS == 17
    for h in K.HYPERS.values():                                   # 1.f - alpha is exact: the double of the rounded alpha is it
        a = F(h["alpha"])
        assert float(F(1) - a) == 1.0 - float(a)
    assert F(1.0 - 0.99) != F(1) - F(0.99)                        # ... and is not stock torch's 1 - alpha rounded once
    assert K.grid(K.ONE_SWEEP, K.STEP_MAXBLK) == 4096 == (K.ONE_SWEEP // 4) // 256 and K.grid(K.WRAP, K.STEP_MAXBLK) == 4096
    assert K.grid(2 ** 21, K.SUMSQ_MAXBLK) == 2048 == (2 ** 21 // 4) // 256 and K.grid(1, K.SUMSQ_MAXBLK) == 1


@pytest.mark.parametrize("case", K.STEP_CASES, ids=_name)
def test_step_restatement_stays_within_half_the_bounds(case):
    x, ref, got, units = _run(case)
    print(f"{case.name}: {K.fmt_units(units)}")
    assert not K.step_breaks(units, K.K_S / 2, K.K_B / 2, K.K_P / 2), units
    if case.max_norm == 0.0 or case.norm is None or case.name.startswith("far_below"):
        assert got["g"].tobytes() == x["g"].tobytes()             # coef = 1: the gradient keeps its bits


@pytest.mark.parametrize("case", K.SHARP_CASES, ids=_name)
def test_sharp_cases_have_the_roundings_that_were_counted(case):
    """wd = 0, mu = 0, coef = 1, sq = buf = 0: sq' = fl(fl((1 - alpha) g) g), two roundings, 2 u sq'; buf' = g / fl(fl(sqrt(sq')) +
    eps): half of sq's two, the root, the sum, the quotient, 4 u |q| = 2 u of the magnitude 2 |q|.  The restatement has exactly
    these roundings, so it is held to the counted bounds themselves, not to half of them."""
    x, ref, got, units = _run(case)
    assert got["g"].tobytes() == x["g"].tobytes()
    assert units["s"] <= K.SHARP_S and units["b"] <= K.SHARP_B and units["p"] <= K.K_P / 2, units
    assert np.array_equal(ref["mag_s"], ref["s"]) and np.allclose(ref["mag_b"], 2 * np.abs(ref["b"]), rtol=1e-12)


def test_the_tiny_case_reaches_the_floor():
    """sq' is about 1e-42: its float32 error is a fraction of 2^-149, far above K_S u sq', and inside the floor of 5."""
    case = K.CASE_BY_NAME["tiny"]
    x, ref, got, units = _run(case)
    err = np.abs(got["s"] - ref["s"])
    assert float(ref["s"].max()) < 2.0 ** -126 and float(ref["s"].min()) > 0
    assert float(err.max()) > 100 * K.K_S * K.U * float(ref["mag_s"].max()) and float(err.max()) <= K.DENORM
    assert units["s"] == 0.0 and bool((got["b"] != 0).all())


def test_zero_gradient_on_zero_state_stays_zero():
    case = K.CASE_BY_NAME["gzero-plain"]
    x, ref, got, _ = _run(case)
    dead = (x["g"] == 0)
    assert int(dead.sum()) >= case.n // 2
    for k in "sb":
        assert bool((got[k][dead] == 0).all()) and bool((ref[k][dead] == 0).all())
    assert got["p"][dead].tobytes() == x["p"][dead].tobytes()
    x, ref, got, _ = _run(K.CASE_BY_NAME["gzero-ema"])            # with weight decay ge = 0 only where p = 0 too
    dead = (x["g"] == 0) & (x["p"] == 0)
    assert int(dead.sum()) >= case.n // 4 and bool((got["b"][dead] == 0).all()) and bool(np.isfinite(got["b"]).all())


def test_ordinary_inputs_cancel_in_the_effective_gradient():
    """g coef + wd p cancels to a small part of A somewhere (wd = 1e-2): the bounds are in A for that reason."""
    case = K.CASE_BY_NAME["wrap"]
    x, h = K.step_inputs(case), K.hyper32(K.HYPERS[case.hyper])
    gc, wdp = x["g"].astype(np.float64) * float(K.coef32(case.norm, case.max_norm)), h["wd"] * x["p"].astype(np.float64)
    assert float((np.abs(gc + wdp) / (np.abs(gc) + np.abs(wdp))).min()) < 1e-4


# ------------------------------------------------------------------------------------------------ (b) the sum of squares
@pytest.mark.parametrize("n", K.SUMSQ_SIZES)
def test_integer_gradients_sum_exactly_in_float32(n):
    g = K.integer_gradient(n)
    terms = torch.from_numpy(g).double() ** 2
    nb = K.grid(n, K.SUMSQ_MAXBLK)
    # a workgroup's elements: every 256-thread stretch of 4-element groups it visits, and the tail (block 0); bounded by all
    # the elements of ceil(n / 4 / threads) sweeps of one workgroup plus the tail
    per_group = (-(-(n // 4) // (nb * 256)) * 1024 + 3) * 9
    assert per_group < 2 ** 24
    require_exact_sum(terms.reshape(1, -1)[:, :min(n, 2 ** 20)], 1.0, 1, "g^2")      # integers; any 2^20 of them stay below 2^24
    norm, partials = K.sumsq_f32(g)
    assert float(partials.max()) <= per_group and np.array_equal(partials, np.round(partials))
    assert float(partials.astype(np.float64).sum()) == float(terms.sum())
    assert norm == K.exact_norm(g)
    assert K.sumsq_f32(g, "dropped_tail")[0] != norm and K.sumsq_f32(g, "double")[0] != norm


@pytest.mark.parametrize("n", K.SUMSQ_SIZES)
def test_probes_see_a_dropped_and_a_doubled_element(n):
    idx = K.probe_indices(n)
    assert 0 in idx and n - 1 in idx and set(range(n // 4 * 4, n)) <= set(idx)
    if n == 2 ** 21 + 7:
        assert {1023, 2 ** 21, 2 ** 21 + 3, 2 ** 21 + 4, 2 ** 21 + 5, 2 ** 21 + 6} <= set(idx)
    if n == 2 ** 21:
        assert idx == [0, 1023, n - 1]
    for i in idx:
        g = np.zeros(n, F)
        g[i] = 3
        assert K.sumsq_f32(g)[0] == F(3)
    g = np.zeros(n, F)
    g[-1] = 3
    assert K.sumsq_f32(g, "dropped_tail")[0] == 0
    g = np.zeros(n, F)
    g[K.double_index(n)] = 3
    assert K.sumsq_f32(g, "double")[0] == F(np.sqrt(18.0))
    assert K.double_index(n) == (2 ** 21 if n > 2 ** 21 else n // 4 * 4 if n % 4 else n - 1)


@pytest.mark.parametrize("n,scale", K.SUMSQ_RANDOM)
def test_restated_sum_of_squares_meets_half_its_bound(n, scale):
    g = K.random_gradient(n, scale)
    want = K.norm64(g)
    got = float(K.sumsq_f32(g)[0])
    units = abs(got - want) / (K.U * want)
    print(f"n {n} scale {scale:g}: {units:.2f} u of the norm (bound {K.norm_bound(want) / (K.U * want):.1f})")
    assert abs(got - want) <= K.norm_bound(want, 0.5)
    assert float((g.astype(np.float64) ** 2)[g != 0].min()) > 2.0 ** -126 * 2 ** 24 or n * K.DENORM < K.U * want ** 2      # no floor needed


def test_squares_that_overflow_give_an_infinite_norm():
    with np.errstate(over="ignore"):
        assert np.isinf(K.sumsq_f32(np.full(4099, 3e19, F))[0]) and np.isinf(K.sumsq_f32(np.full(4099, 1e19, F))[0])
        assert np.isfinite(F(1e19) * F(1e19))                     # at 1e19 the sum overflows, not the square


# ------------------------------------------------------------------------------------------------ (c) stock torch
@pytest.mark.parametrize("name,hyper,state,gscale,max_norm", K.STOCK_CASES, ids=[c[0] for c in K.STOCK_CASES])
def test_the_oracle_given_torchs_doubles_is_stock_torch(name, hyper, state, gscale, max_norm):
    """Both are float64; torch orders the products of addcmul / addcdiv its own way: 16 float64 roundings of room."""
    x, h = K.stock_inputs(name, state, gscale), K.HYPERS[hyper]
    stock, mine = K.stock_torch_step(x, max_norm, h), K.oracle_step_doubles(x, max_norm, h)
    assert (K.real_norm32(x["g"]) > max_norm) == (gscale == 1.0)  # one clipped, one not
    ref = K.step_reference(x, K.coef32(K.real_norm32(x["g"]), max_norm), h)
    mags = {"g": np.abs(stock["g"]), "s": ref["mag_s"], "b": ref["mag_b"], "p": np.abs(stock["p"]) + 1e-300}
    for k in "gsbp":
        assert bool((np.abs(stock[k] - mine[k]) <= 16 * 2.0 ** -53 * mags[k]).all()), k
    # the primary reference against stock torch: what the float32 hyper-parameters and 1.f - alpha cost, in the bounds' units
    d = K.stock_distance({k: ref[k] for k in "gsbp"}, x, stock, ref, h)
    print(f"{name}: float64 reference to stock torch, relative to the magnitudes: " + ", ".join(f"{k} {v:.2e}" for k, v in d.items()))
    assert max(d.values()) <= K.OP_TOL / 2
    if state == "first":
        # sq' = (1 - alpha) ge^2: the whole difference of the two 1 - alpha lands in it, and the rounding of wd and of coef
        want = 1 - float(F(1) - F(0.99)) / (1 - 0.99)
        assert abs(want - 9.54e-7) < 1e-9 and 0.5 * want < d["s"] < 1.5 * want


@pytest.mark.parametrize("norm,max_norm", [(c.norm, c.max_norm) for c in K.STEP_CASES if c.n == 1025 and c.hyper == "ema"])
def test_the_float32_coefficient_is_the_oracles_within_two_roundings(norm, max_norm):
    got = float(K.coef32(norm, max_norm))
    if norm is None or max_norm == 0.0:
        assert got == 1.0
        return
    want = float(S.clip_coef(torch.tensor(float(F(norm)), dtype=torch.float64), float(F(max_norm))))
    # the sum and the quotient round once each; 1e-6f for 1e-6 moves the sum by 3e-14 / norm relatively
    assert abs(got - want) <= (2 * K.U + 3e-14 / norm + 1e-12) * want
    if norm == max_norm == 1.0:
        assert got == float(F(1) / (F(1) + F(1e-6))) < 1.0          # at max_norm the gradient IS scaled, as torch has it


# ------------------------------------------------------------------------------------------------ (d) refused arguments
def test_bad_arguments_are_refused_before_any_launch():
    """Every check sits in front of the launches: no GPU is touched (the pointers are never followed)."""
    import unet_amd  # noqa: F401
    from unet_amd._lib import LIB
    LIB.load()
    P, Q, R, T = 4096, 1 << 20, 1 << 21, 1 << 22                  # non-null, 16-byte aligned stand-in pointers
    need = LIB.query("uh_optim_ws_bytes", 1024)
    assert need >= K.SUMSQ_MAXBLK * 4
    for args in ((None, 8, Q, R, need), (P, 8, None, R, need), (P, 8, Q, None, need), (P, 0, Q, R, need), (P, -4, Q, R, need)):
        with pytest.raises(RuntimeError, match="uh_grad_sumsq: bad args"):
            LIB.call("uh_grad_sumsq", *args, None)
    with pytest.raises(RuntimeError, match="16-byte"):
        LIB.call("uh_grad_sumsq", P + 4, 8, Q, R, need, None)
    for short in (0, need - 1):
        with pytest.raises(RuntimeError, match="workspace too small"):
            LIB.call("uh_grad_sumsq", P, 8, Q, R, short, None)
    hyper = (1.0, 1e-5, 0.99, 1e-8, 1e-8, 0.999)
    good = [P, Q, R, T]
    for k in range(4):
        ptrs = list(good)
        ptrs[k] = None
        with pytest.raises(RuntimeError, match="uh_rmsprop_step: bad args"):
            LIB.call("uh_rmsprop_step", *ptrs, 8, None, *hyper, None)
        ptrs[k] = good[k] + 4
        with pytest.raises(RuntimeError, match="16-byte"):
            LIB.call("uh_rmsprop_step", *ptrs, 8, None, *hyper, None)
    for n in (0, -1):
        with pytest.raises(RuntimeError, match="uh_rmsprop_step: bad args"):
            LIB.call("uh_rmsprop_step", *good, n, None, *hyper, None)
    with pytest.raises(RuntimeError, match="uh_swap_f32"):
        LIB.call("uh_swap_f32", None, Q, 8, None)


# ------------------------------------------------------------------------------------------------ (e) seeded mistakes
# mistake -> (the cases where it must break a bound, the outputs of which at least one must miss)
MISTAKE_CASES = {
    "eps_inside_sqrt": (["n4099-reference", "n4099-ema", "first-plain", "wide-reference", "n7-ema"], "b"),
    "old_second_moment": (["n4099-reference", "n4099-ema", "first-ema", "large-plain", "n7-ema"], "b"),
    "decay_scaled_too": (["n4099-ema", "far_above-ema", "max_norm_half-ema", "n5-ema"], "sb"),
    "no_weight_decay": (["n4099-ema", "first-ema", "max_norm_zero-ema", "n3-ema"], "sb"),
    "one_minus_alpha_from_double": (["sharp-n7", "sharp-n4099"], "sb"),
    "lr_times_quotient": (["n4099-reference", "n4099-ema", "n1-ema", "wrap"], "p"),
    "g_left_unscaled": (["n4099-reference", "at_max_norm-ema", "just_below-reference", "just_above-ema", "n1-plain"], "g"),
    "coef_without_1e-6": (["at_max_norm-reference", "at_max_norm-ema", "just_below-ema", "n4099-ema", "max_norm_half-reference"], "g"),
    "dropped_tail": (["n1-reference", "n3-ema", "n5-plain", "n1025-ema", "n4099-reference", "wrap"], "gsbp"),
    "double": (["wrap", "wrap-first"], "gsb"),
}


def test_every_mistake_of_the_list_has_its_cases():
    assert sorted(MISTAKE_CASES) == sorted(K.STEP_MISTAKES) and len(K.STEP_MISTAKES) == 10


@pytest.mark.parametrize("mistake", K.STEP_MISTAKES)
def test_a_seeded_mistake_breaks_a_bound(mistake):
    names, outputs = MISTAKE_CASES[mistake]
    for name in names:
        case = K.CASE_BY_NAME[name]
        sharp = case in K.SHARP_CASES
        at = K.STEP_MAXBLK * 1024 if mistake == "double" else None          # the first element of the second sweep
        _, _, _, units = _run(case, mistake, at)
        ks, kb = (K.SHARP_S, K.SHARP_B) if sharp else (K.K_S, K.K_B)
        broken = K.step_breaks(units, ks, kb)
        print(f"{mistake} at {name}: {K.fmt_units(units)} -> breaks {broken}")
        assert set(broken) & set(outputs), (mistake, name, units)
        assert not K.step_breaks(_run(case)[3], ks, kb)             # and the right statements do not


def test_one_minus_alpha_from_double_is_inside_the_general_bounds():
    """Why the sharp cases exist: the 16 u between the two 1 - alpha fit into K_S = 19 and K_B = 10 (half of them reach buf), so the
    general bounds cannot say which of the two the kernel forms.  The counted bounds of the sharp cases can."""
    _, _, _, units = _run(K.CASE_BY_NAME["first-plain"], "one_minus_alpha_from_double")
    assert not K.step_breaks(units) and units["s"] > K.K_S / 2
    _, _, _, units = _run(K.CASE_BY_NAME["sharp-n4099"], "one_minus_alpha_from_double")
    assert units["s"] > 4 * K.SHARP_S and units["b"] > K.SHARP_B        # 15.6 u in sq', half of it in the quotient
