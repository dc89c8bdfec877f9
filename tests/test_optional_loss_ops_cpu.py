"""CPU proof that tests/test_gpu_optional_loss_ops.py is as sharp as it claims, at every case it runs (the lists are
tests/optional_loss_cases.py's): (a) the shapes reach what they are named for, by the launch formulas; (b) the saturated family is
exact in float32 and its expected sums are the restatement's, bit for bit; (c) the closed-form gradients equal autograd at the small
shapes; (d) a float32 torch restatement of each kernel's arithmetic stays within R where the kernels are given 2 R; (e) each seeded
mistake in the restatement breaks a bound or an equality at the case it is aimed at.

The same mistake in a kernel fails these assertions of tests/test_gpu_optional_loss_ops.py:

  seeded mistake                          GPU assertion it fails
  --------------------------------------  --------------------------------------------------------------------------------------
  last pixel of the ragged tail dropped   test_saturated_*: torch.equal on the sums (every pixel counts in W, P_c, T_c / agree;
                                          n - 1 is a special index); test_*_against_float64: the NaN pre-fill of that element
  pixel at grid * 256 counted twice       test_saturated_* at grid_wrap and above_cap: torch.equal on the sums (F, TP, kd, S move by
                                          one special pixel's term; the counts by one)
  1 - p_t for u                           test_focal_sums_finish_and_gradient_against_float64 at the easy cases (scale 0.0): F column
  class index off by one                  test_surface_value_and_gradient_against_float64 (every multi-class case); the focal
                                          count columns T_c (equalities)
  |K| replaced by C                       surface: value and gradient bounds at C != K; focal: the gradient bound with classes (1,)
  gscale left out                         every gradient test at gscale 0.5 and 65536
  phi's sign at a border pixel            test_distance_maps_at_grid_wrap_bit_for_bit (-0.0 against +0.0 is one bit)
  T^2 for T in the kd gradient            test_distill_sums_finish_and_gradient_against_float64 at every T != 1
  an out-of-head label given weight       the W column (an equality) of test_focal_* and of test_saturated_focal_*; the mask -1
                                          divided by truncation (class 0 under mask_div 2): W and T_0 of the saturated one-channel head"""
import numpy as np
import pytest
import torch

import distill_ref as DR
import focal_tversky_ref as FR
import optional_loss_cases as K
import surface_loss_ref as SR

_ids = lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else None      # noqa: E731


def _f32_of(sums64):
    return torch.tensor(sums64, dtype=torch.float64).float()


# ------------------------------------------------------------------------------------------------ (a) shapes
def test_the_shapes_reach_what_they_are_named_for():
    facts = K.launch_facts()
    assert set(facts) == set(K.SHAPES) and all(facts.values())
    n = K.npix("grid_wrap")
    sp = K.special_indices(n)
    assert {0, 255, 256, 2047, 2048, 4096 * 256 - 1, 4096 * 256, 513 * 256, n - 1} <= set(sp)
    assert K.special_indices(3) == [0, 2] and K.special_indices(3330)[-1] == 3329
    assert K.rows(K.npix("above_cap")) * 256 in K.special_indices(K.npix("above_cap"))


def test_the_saturated_family_is_exact_in_float32():
    assert K.sat_conditions()
    assert all(float(np.log2(w)) == round(float(np.log2(w))) for C in (2, 3, 4, 8) for w in K.sat_weights(C))
    assert all(float(a * 4) == round(a * 4) for pr in K.SAT_PRICES for a in pr)


# ------------------------------------------------------------------------------------------------ (b) saturated = restatement
@pytest.mark.parametrize("shape", list(K.SHAPES))
def test_saturated_focal_sums_are_the_restatements_bit_for_bit(shape):
    for ncls in K.SAT_HEADS[shape]:
        logits, mask, div, w, sums = K.sat_focal_case(shape, ncls)
        for gamma in K.SAT_GAMMAS if shape in K.SMALL else K.SAT_GAMMAS[2:]:
            own, g = K.focal_f32(logits, mask, div, ncls, w, gamma, 0.5, 0.5, (1,))
            assert own.double().tolist() == sums, (ncls, gamma, own.tolist(), sums)
            assert bool(torch.isfinite(g).all())


@pytest.mark.parametrize("shape", list(K.SHAPES))
def test_saturated_distill_sums_are_the_restatements_bit_for_bit(shape):
    for ncls in K.SAT_HEADS[shape]:
        z, v, sums = K.sat_distill_case(shape, ncls)
        own, g = K.distill_f32(z, v, ncls, K.SAT_T, float(z.shape[0]), 1.0)
        assert own.double().tolist() == sums and sums[0] == 128.0 * len(K.special_indices(z.shape[0]))
        # the gradient is 0 where the two agree and -+ w T / n on the two classes where they do not
        assert sorted(set((g * z.shape[0] / K.SAT_T).flatten().tolist())) in ([-1.0, 0.0, 1.0], [-1.0, 1.0])


@pytest.mark.parametrize("shape", list(K.SHAPES))
def test_saturated_surface_value_is_the_restatements_bit_for_bit(shape):
    n = K.npix(shape)
    for ncls, classes in K.SAT_SURFACE[shape]:
        logits, labels, phi, S = K.sat_surface_case(shape, ncls, classes)
        got, _ = K.surface_f32(logits, phi, ncls, classes, float(n), K.SURFACE_W)
        assert got == K.surface_finish64(S, float(n), len(classes), K.SURFACE_W), (ncls, classes, got, S)
    assert S != 0.0 or shape == "sub_wave"


# ------------------------------------------------------------------------------------------------ (c) closed forms = autograd
@pytest.mark.parametrize("case", [c for c in K.FOCAL_CASES if c[0] in K.SMALL], ids=_ids)
def test_focal_closed_form_equals_autograd(case):
    shape, scale, ncls, gamma = case
    ref = K.focal_ref_cached(*case)
    for alpha, beta, cls, gs in K.focal_grad_settings(shape)[:2]:
        g, M, _ = K.focal_grad64(ref, alpha, beta, cls, None)
        cl = FR.closed_form_gradient(ref["z"], ref["t"], ref["w"], gamma, alpha, beta, cls)
        ag = FR.autograd_gradient(ref["z"], ref["t"], ref["w"], gamma, alpha, beta, cls)
        assert float((cl - ag).abs().max()) <= 1e-12 * max(1.0, float(ag.abs().max()))
        # focal_grad64 is handed the sums rounded to float32, as the kernel is: it differs by that rounding alone, one unit at most
        assert float(((g - cl).abs() / (K.U * M)).max()) <= 1.0


@pytest.mark.parametrize("case", [c for c in K.DISTILL_CASES if c[0] in K.SMALL], ids=_ids)
def test_distill_closed_form_equals_autograd(case):
    shape, scale, ncls, teacher = case
    z, v = (K.head_form(t, ncls) for t in K.distill_inputs(*case))
    ref = K.distill_ref_cached(*case)
    T, n = ref["T"], ref["n"]
    kd, agree = DR.loss_terms(z, v, T)
    assert abs(float(kd) - T * T / n * ref["sums"][0]) <= 1e-12 * max(1.0, abs(float(kd))) + 1e-13 * ref["A"] / n
    assert round(float(agree) * n) == ref["sums"][1]
    g, _, _ = K.distill_grad64(ref, n, 1.0, None)
    ag = DR.autograd_gradient(z, v, T)
    assert float((g - ag).abs().max()) <= 1e-12 * T / n


@pytest.mark.parametrize("case", [c for c in K.SURFACE_CASES if c[0] in K.SMALL], ids=_ids)
def test_surface_closed_form_equals_autograd(case):
    shape, scale, ncls, classes = case
    B, H, W = K.SHAPES[shape]
    ref = K.surface_ref_cached(*case)
    logits = K.surface_inputs(shape, scale, ncls)
    bchw = (logits.reshape(B, H, W, 1) if ncls == 1 else logits.reshape(B, H, W, ncls)).permute(0, 3, 1, 2).double().requires_grad_()
    v = SR.surface_loss(bchw, K.surface_labels(shape, ncls == 1), ncls, classes)
    (ag,) = torch.autograd.grad(v, bchw)
    ag = ag.permute(0, 2, 3, 1).reshape(ref["p"].shape)
    g, M, _ = K.surface_grad64(ref, float(ref["n"]), 1.0, None)
    assert abs(float(v.detach()) - K.surface_value64(ref, float(ref["n"]))) <= 1e-12 * ref["A"] / ref["n"]
    assert float((g - ag).abs().max()) <= 1e-12 * max(1e-30, float(ag.abs().max()))


# ------------------------------------------------------------------------------------------------ (d) the restatement within R
WORST = {}


def _note(name, v):
    WORST[name] = max(WORST.get(name, 0.0), v)
    return v


@pytest.mark.parametrize("case", K.FOCAL_CASES + K.FOCAL_SUMS_ONLY, ids=_ids)
def test_focal_restatement_stays_within_r(case):
    shape, scale, ncls, gamma = case
    logits, mask, div = K.focal_inputs(shape, scale, ncls)
    ref = K.focal_ref_cached(*case)
    C = ref["C"]
    own, _ = K.focal_f32(logits, mask, div, ncls, ref["w"], gamma)
    units = K.L.check_sums(own, ref, K.FOCAL_COUNTS(C), K.SUMS_FRAC_RESTATEMENT)
    print(f"{case}: sums worst column {_note('focal sums', units):.2f} u S64 beyond its slack")
    if case in K.FOCAL_SUMS_ONLY:
        return
    worst = 0.0
    for alpha, beta, cls, gs in K.focal_grad_settings(shape):
        g64, M, slack = K.focal_grad64(ref, alpha, beta, cls, gs)
        _, g = K.focal_f32(logits, mask, div, ncls, ref["w"], gamma, alpha, beta, cls, gs, sums=_f32_of(ref["sums"]))
        worst = max(worst, K.grad_units(g, K.pick(g64, ncls), K.pick(M, ncls), K.pick(slack, ncls), gs))
    print(f"{case}: worst gradient element {_note('focal grad', worst):.2f} units of u M (R = {K.R_FOCAL_GRAD})")
    assert worst <= K.R_FOCAL_GRAD


@pytest.mark.parametrize("case", K.DISTILL_CASES + K.DISTILL_SUMS_ONLY, ids=_ids)
def test_distill_restatement_stays_within_r(case):
    shape, scale, ncls, teacher = case
    z, v = K.distill_inputs(*case)
    ref = K.distill_ref_cached(*case)
    n, T = ref["n"], ref["T"]
    own, _ = K.distill_f32(z, v, ncls, T, float(n), K.KD_W)
    assert float(own[1]) == ref["sums"][1]
    units = K.kd_sum_units(own[0], ref)
    print(f"{case}: kd sum {float(own[0]):.9g} (float64 {ref['sums'][0]:.9g}), {_note('kd sum', units):.2f} units of u A (R = {K.R_KD_SUM})")
    assert units <= K.R_KD_SUM
    if case in K.DISTILL_SUMS_ONLY:
        return
    worst = 0.0
    for world, gs in K.distill_grad_settings(shape):
        g64, M, slack = K.distill_grad64(ref, float(n * world), K.KD_W, gs)
        _, g = K.distill_f32(z, v, ncls, T, float(n * world), K.KD_W, gs)
        worst = max(worst, K.grad_units(g, K.pick(g64, ncls), K.pick(M, ncls), K.pick(slack, ncls), gs))
    print(f"{case}: worst gradient element {_note('kd grad', worst):.2f} units of u M (R = {K.R_DISTILL_GRAD})")
    assert worst <= K.R_DISTILL_GRAD


@pytest.mark.parametrize("case", K.SURFACE_CASES + K.SURFACE_SUMS_ONLY, ids=_ids)
def test_surface_restatement_stays_within_r(case):
    shape, scale, ncls, classes = case
    logits = K.surface_inputs(shape, scale, ncls)
    phi = K.surface_phi(shape, classes, ncls == 1)
    ref = K.surface_ref_cached(*case)
    n = ref["n"]
    (v, wv), _ = K.surface_f32(logits, phi, ncls, classes, float(n), K.SURFACE_W)
    units = K.surface_value_units(v, ref, float(n))
    print(f"{case}: value {v:.9g} (float64 {K.surface_value64(ref, float(n)):.9g}), {_note('surface value', units):.2f} units of u sum |p phi| (R = {K.R_SURFACE_VALUE})")
    assert units <= K.R_SURFACE_VALUE and wv == float(np.float32(K.SURFACE_W) * np.float32(v))
    if case in K.SURFACE_SUMS_ONLY:
        return
    worst = 0.0
    for world, gs in K.surface_grad_settings(shape):
        g64, M, slack = K.surface_grad64(ref, float(n * world), K.SURFACE_W, gs)
        _, g = K.surface_f32(logits, phi, ncls, classes, float(n * world), K.SURFACE_W, gs)
        worst = max(worst, K.grad_units(g, g64, M, slack, gs))
    R = K.surface_grad_r(ncls)[0]
    print(f"{case}: worst gradient element {_note('surface grad' + (' binary' if ncls == 1 else ''), worst):.2f} units of u M (R = {R})")
    assert worst <= R


def test_zz_the_worst_of_the_restatement_sits_in_the_upper_half_of_r():
    """R is the NEXT power of two above the worst: not a looser one.  (Runs after the cases above; alone it has nothing to check.)"""
    print(WORST)
    for name, R in (("focal grad", K.R_FOCAL_GRAD), ("kd grad", K.R_DISTILL_GRAD), ("surface grad", K.R_SURFACE_GRAD),
                    ("surface grad binary", K.R_SURFACE_GRAD_BINARY),
                    ("kd sum", K.R_KD_SUM), ("surface value", K.R_SURFACE_VALUE)):
        if name in WORST:
            assert R / 2 < WORST[name] <= R or (R == 1 and WORST[name] <= 1), (name, WORST[name], R)


# ------------------------------------------------------------------------------------------------ (e) seeded mistakes
def _focal_breaks(case, mistake, alpha=0.3, beta=0.7, cls=None, gs=None, **kw):
    """(a sums column or equality breaks, a gradient element breaks) with the kernels' 2 R."""
    shape, scale, ncls, gamma = case
    logits, mask, div = K.focal_inputs(shape, scale, ncls)
    ref = K.focal_ref_cached(*case)
    own, _ = K.focal_f32(logits, mask, div, ncls, ref["w"], gamma, mistake=mistake, **kw)
    g64, M, slack = K.focal_grad64(ref, alpha, beta, cls, gs)
    _, g = K.focal_f32(logits, mask, div, ncls, ref["w"], gamma, alpha, beta, cls, gs, sums=_f32_of(ref["sums"]), mistake=mistake, **kw)
    units = K.grad_units(g, K.pick(g64, ncls), K.pick(M, ncls), K.pick(slack, ncls), gs)
    return (not K.L.sums_hold(own, ref, K.FOCAL_COUNTS(ref["C"]))), units > K.K_FOCAL_GRAD


def _distill_breaks(case, mistake, world=1, gs=None, **kw):
    shape, scale, ncls, teacher = case
    z, v = K.distill_inputs(*case)
    ref = K.distill_ref_cached(*case)
    n, T = ref["n"], ref["T"]
    own, g = K.distill_f32(z, v, ncls, T, float(n * world), K.KD_W, gs, mistake=mistake, **kw)
    g64, M, slack = K.distill_grad64(ref, float(n * world), K.KD_W, gs)
    sums_break = float(own[1]) != ref["sums"][1] or abs(float(own[0]) - ref["sums"][0]) > K.kd_sum_bound(ref, K.K_KD_SUM)
    return sums_break, K.grad_units(g, K.pick(g64, ncls), K.pick(M, ncls), K.pick(slack, ncls), gs) > K.K_DISTILL_GRAD


def _surface_breaks(case, mistake, world=1, gs=None, **kw):
    shape, scale, ncls, classes = case
    logits = K.surface_inputs(shape, scale, ncls)
    phi = K.surface_phi(shape, classes, ncls == 1)
    ref = K.surface_ref_cached(*case)
    nm = float(ref["n"] * world)
    (v, _), g = K.surface_f32(logits, phi, ncls, classes, nm, K.SURFACE_W, gs, mistake=mistake, **kw)
    g64, M, slack = K.surface_grad64(ref, nm, K.SURFACE_W, gs)
    return abs(v - K.surface_value64(ref, nm)) > K.surface_value_bound(ref, nm, K.K_SURFACE_VALUE), K.grad_units(g, g64, M, slack, gs) > K.surface_grad_r(ncls)[1]


F_CASE, F_HARD = ("two_blocks", 10.0, 3, 2.0), ("two_blocks", 10.0, 3, 1.5)
D_CASE = ("two_blocks", 10.0, 3, "free")
S_CASE, S_BIN = ("two_blocks", 10.0, 3, (2,)), ("two_blocks", 10.0, 1, (1,))


def test_the_unmistaken_restatement_breaks_nothing():
    assert _focal_breaks(F_CASE, None) == (False, False) and _focal_breaks(F_HARD, None, 0.5, 0.5, (1,), 0.5) == (False, False)
    assert _distill_breaks(D_CASE, None) == (False, False) and _distill_breaks(D_CASE, None, 2, 0.5) == (False, False)
    assert _surface_breaks(S_CASE, None) == (False, False) and _surface_breaks(S_BIN, None, 2, 0.5) == (False, False)


def test_a_dropped_tail_pixel_breaks_an_equality_and_its_own_gradient():
    assert _focal_breaks(F_CASE, "tail") == (True, True)                    # the count columns are equalities
    assert _distill_breaks(D_CASE, "tail")[1]
    assert _surface_breaks(S_CASE, "tail")[1] and _surface_breaks(S_BIN, "tail")[1]
    # ... and at 10^6 pixels, where no rounding bound can see one pixel, the saturated family does
    for shape in ("grid_wrap", "above_cap"):
        z, v, sums = K.sat_distill_case(shape, 3)
        own, _ = K.distill_f32(z, v, 3, K.SAT_T, float(z.shape[0]), 1.0, mistake="tail")
        assert own.double().tolist() != sums
        logits, labels, phi, S = K.sat_surface_case(shape, 3, (2,))
        n = float(K.npix(shape))
        assert K.surface_f32(logits, phi, 3, (2,), n, 0.5, mistake="tail")[0] != K.surface_finish64(S, n, 1, 0.5)


@pytest.mark.parametrize("shape", ["grid_wrap", "above_cap"])
def test_a_pixel_counted_twice_where_the_grid_goes_round_breaks_the_exact_sums(shape):
    n = K.npix(shape)
    at = K.grid(n) * 256
    assert at in K.special_indices(n)
    logits, mask, div, w, sums = K.sat_focal_case(shape, 3)
    own, _ = K.focal_f32(logits, mask, div, 3, w, 1.5, mistake="twice", twice_at=at)
    assert own[0].item() != sums[0] and own[1].item() != sums[1]            # F (a disagreeing pixel) and W (every pixel)
    z, v, ksums = K.sat_distill_case(shape, 3)
    own, _ = K.distill_f32(z, v, 3, K.SAT_T, float(n), 1.0, mistake="twice", twice_at=at)
    assert own[0].item() == ksums[0] + 128.0
    logits, labels, phi, S = K.sat_surface_case(shape, 3, (2,))
    got = K.surface_f32(logits, phi, 3, (2,), float(n), 0.5, mistake="twice", twice_at=at)[0]
    assert (got != K.surface_finish64(S, float(n), 1, 0.5)) == (float(phi.reshape(1, -1)[0, at]) != 0.0)
    assert float(phi.reshape(1, -1)[0, at]) != 0.0
    # the general family cannot: one pixel of 10^6 is inside any rounding bound
    case = ("grid_wrap", 1.0, 3, "near")
    zz, vv = K.distill_inputs(*case)
    ref = K.distill_ref_cached(*case)
    own, _ = K.distill_f32(zz, vv, 3, ref["T"], float(ref["n"]), K.KD_W, mistake="twice", twice_at=at)
    assert float(own[1]) != ref["sums"][1]                                   # ... but for the count column


def test_one_minus_p_t_for_u_breaks_the_f_column_of_easy_pixels():
    for case in K.FOCAL_EASY:
        assert _focal_breaks(case, None) == (False, False) and _focal_breaks(case, "one_minus_pt")[0], case
    # neither the norm the older test holds the gradient to nor the per-element bound sees it in a mixed batch (see the finding in
    # optional_loss_cases)
    assert _focal_breaks(F_CASE, "one_minus_pt") == (False, False)
    shape, scale, ncls, gamma = F_CASE
    logits, mask, div = K.focal_inputs(shape, scale, ncls)
    ref = K.focal_ref_cached(*F_CASE)
    g64, _, _ = K.focal_grad64(ref, 0.3, 0.7, None, None)
    _, g = K.focal_f32(logits, mask, div, ncls, ref["w"], gamma, 0.3, 0.7, None, None, sums=_f32_of(ref["sums"]), mistake="one_minus_pt")
    assert float((g.double() - g64).norm() / g64.norm()) <= 2e-5


def test_a_class_index_off_by_one_breaks_counts_value_and_gradient():
    assert _focal_breaks(F_CASE, "label_off_by_one") == (True, True)
    assert _surface_breaks(S_CASE, "class_off_by_one") == (True, True)


def test_c_for_the_number_of_selected_classes_breaks_value_and_gradient():
    assert _surface_breaks(S_CASE, "k_is_c") == (True, True)
    assert _focal_breaks(F_CASE, "k_is_c", 0.5, 0.5, (1,))[1]


def test_gscale_left_out_breaks_every_gradient():
    for gs in (0.5, 65536.0):
        assert _focal_breaks(F_CASE, "no_gscale", gs=gs)[1] and _distill_breaks(D_CASE, "no_gscale", gs=gs)[1]
        assert _surface_breaks(S_CASE, "no_gscale", gs=gs)[1] and _surface_breaks(S_BIN, "no_gscale", gs=gs)[1]


def test_phi_with_the_wrong_sign_of_zero_on_the_border_differs_in_its_bits():
    labels = K.surface_labels("two_blocks", False)
    want = SR.phi_maps(labels, (2, 1), binary=False)
    assert np.array_equal(K.phi_port(labels, (2, 1), False).view(np.int32), want.view(np.int32))
    wrong = K.phi_port(labels, (2, 1), False, mistake="border_sign")
    assert np.array_equal(wrong, want) and not np.array_equal(wrong.view(np.int32), want.view(np.int32))


def test_t_squared_in_the_kd_gradient_breaks_it():
    assert K.KD_T[3] != 1.0 and _distill_breaks(D_CASE, "t_squared")[1]


def test_a_label_outside_the_head_given_weight_breaks_w():
    logits, mask, div = K.focal_inputs(*F_CASE[:3])
    t = torch.div(mask, div, rounding_mode="floor")
    assert int(((t < 0) | (t >= 3)).sum()) > 50
    assert _focal_breaks(F_CASE, "weight_outside")[0]
    lg, mk, dv, w, sums = K.sat_focal_case("two_blocks", 3)
    own, _ = K.focal_f32(lg, mk, dv, 3, w, 2.0, mistake="weight_outside")
    assert own[1].item() != sums[1]
    # the mask -1 under mask_div 2: `//` makes it -1, a truncating division class 0 (uh_mask_quot did that before this file)
    lg, mk, dv, w, sums = K.sat_focal_case("two_blocks", 1)
    assert dv == 2 and int((mk == -1).sum()) == 1
    own, _ = K.focal_f32(lg, mk, dv, 1, w, 2.0, mistake="trunc_div")
    assert own[1].item() == sums[1] + w[0] and own[2 + 4].item() == sums[2 + 4] + 1


def test_the_reference_keeps_todays_values_for_labels_inside_the_head():
    """focal_tversky_ref's extension: a label outside the head has a zero indicator row and no weight, and still counts in P_c."""
    g = torch.Generator().manual_seed(3)
    z = torch.randn(50, 3, generator=g, dtype=torch.float64)
    t = torch.randint(0, 3, (50,), generator=g)
    w = (0.5, 1.25, 2.0)
    tau = torch.nn.functional.one_hot(t, 3).double()
    assert torch.equal(FR.indicators(t, 3)[0], tau)
    base = [float(v) for v in FR.loss_terms(z, t, w, 2.0, 0.3, 0.7)]
    zz = torch.cat([z, torch.randn(7, 3, generator=g, dtype=torch.float64)])
    tt = torch.cat([t, torch.tensor([3, -1, 255, 3, 3, -7, 2 ** 40])])
    more = [float(v) for v in FR.loss_terms(zz, tt, w, 2.0, 0.3, 0.7)]
    assert more[1] == base[1] and more[2] != base[2]                         # focal unchanged; P_c grew, so Tversky moved
    ag = FR.autograd_gradient(zz, tt, w, 2.0, 0.3, 0.7)
    cl = FR.closed_form_gradient(zz, tt, w, 2.0, 0.3, 0.7)
    assert float((ag - cl).abs().max()) <= 1e-12 and float(ag[50:].abs().max()) > 0
