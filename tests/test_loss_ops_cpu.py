"""CPU proof that tests/test_gpu_loss_ops.py is as sharp as it claims, at every case it runs (the lists are tests/loss_cases.py's):
(a) a float32 torch restatement of the closed forms of csrc/loss.hip stays inside the bounds with room to spare -- sums within half
their bound, every gradient element within K = 8 units of 2^-24 * M where the kernels are given 16; (b) the boundary cases meet the
sensitivity condition (one miscounted pixel moves the loss by four tolerances or more) and a Python port of the kernel's neighbour
logic gives the oracle's counts on all 588 small geometries; (c) each seeded mistake, applied to the restatement or to the port --
a dropped tail element, n for n_mean, the sign of ka, one class's Dice sums left out, mask_div ignored, an edge pixel's neighbour
taken across the interior run, >= for > at 0.5 -- breaks a bound."""
import pytest
import torch

import loss_cases as K

_ids = lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else None      # noqa: E731


def _f32_of(sums64):
    return torch.tensor(sums64, dtype=torch.float64).float()


def _within(got, ref, counts, frac):
    """Sums inside their bound with `frac` of the accumulation budget (count columns: equal)."""
    return K.sums_hold(got, ref, counts, frac)


# ------------------------------------------------------------------------------------------------ (a) the restatement
@pytest.mark.parametrize("case", K.BINARY_CASES, ids=_ids)
def test_binary_restatement_stays_within_half_the_bounds(case):
    shape, scale, div, soft = case
    logits, mask = K.binary_inputs(*case)
    ref = K.binary_ref_cached(*case)
    n = ref["n"]
    own, _ = K.binary_f32(logits, mask, None if soft else div, n, 1.0, 1.0)
    assert _within(own, ref, () if soft else (3,), 0.5), (own.tolist(), ref["sums"])
    worst = 0.0
    for world, (w_bce, w_dice), gs in K.grad_settings(shape):
        g64, M = K.binary_grad64(ref, n * world, w_bce, w_dice, gs)
        _, g = K.binary_f32(logits, mask, None if soft else div, n * world, w_bce, w_dice, gs, sums=_f32_of(ref["sums"]))
        worst = max(worst, K.grad_units(g, g64, M, gs))
    print(f"{case}: worst gradient element {worst:.2f} units of 2^-24 M")
    assert worst <= K.K_RESTATEMENT


@pytest.mark.parametrize("case", K.MULTICLASS_CASES, ids=_ids)
def test_multiclass_restatement_stays_within_half_the_bounds(case):
    shape, scale, C, labels = case
    logits, mask = K.multiclass_inputs(*case)
    ref = K.multiclass_ref_cached(*case)
    n = ref["n"]
    assert (int((mask == C - 1).sum()) == 0) == (labels == "absent")
    if labels == "all" and shape != "sub_wave":
        assert all(c > 0 for c in ref["sums"][1 + 2 * C:])
    own, _ = K.multiclass_f32(logits, mask, n, 1.0, 1.0)
    assert _within(own, ref, tuple(range(1 + 2 * C, 1 + 3 * C)), 0.5), (own.tolist(), ref["sums"])
    worst = 0.0
    for world, (w_ce, w_dice), gs in K.grad_settings(shape):
        g64, M = K.multiclass_grad64(ref, n * world, w_ce, w_dice, gs)
        _, g = K.multiclass_f32(logits, mask, n * world, w_ce, w_dice, gs, sums=_f32_of(ref["sums"]))
        worst = max(worst, K.grad_units(g, g64, M, gs))
    print(f"{case}: worst gradient element {worst:.2f} units of 2^-24 M")
    assert worst <= K.K_RESTATEMENT


def test_the_cases_of_the_autograd_nodes():
    """SegLossBinaryFn runs the (2,37,45) case at s = 1 with mask // 2 as the boundary target, SegLossMulticlassFn a case of its
    own: the restatement meets the bounds there and the boundary term is sensitive to one pixel."""
    logits, mask = K.binary_inputs("two_blocks", 1.0, 2)
    assert float(logits.abs().max()) <= 10
    target = (mask // 2).float()
    K.assert_boundary_condition(logits, target, 5, 3.0, K.boundary_oracle(logits, target, 5, 3.0))
    (B, H, W, C, ew, wt, w_b), logits, mask = K.multiclass_node_case()
    ref = K.multiclass_ref(logits, mask)
    own, g = K.multiclass_f32(logits, mask, ref["n"], 1.0, 1.0)
    assert _within(own, ref, tuple(range(1 + 2 * C, 1 + 3 * C)), 0.5)
    g64, M = K.multiclass_grad64(ref, ref["n"], 1.0, 1.0, None)
    assert K.grad_units(g, g64, M, None) <= K.K_RESTATEMENT
    K.assert_boundary_condition(logits, mask.float(), ew, wt, K.boundary_oracle(logits, mask.float(), ew, wt))
    assert K.port_counts(logits, mask.float(), ew) == K.oracle_counts(logits, mask.float(), ew)


def test_the_special_binary_cases():
    logits, mask, d = K.wide_mask_case()
    ref = K.binary_ref(logits, mask // d)
    own, g = K.binary_f32(logits, mask, d, 4, 1.0, 1.0)
    assert _within(own, ref, (3,), 0.5)
    g64, M = K.binary_grad64(ref, 4, 1.0, 1.0, None)
    assert K.grad_units(g, g64, M, None) <= K.K_RESTATEMENT
    wrapped = (mask.to(torch.int32).to(torch.int64) // d)                     # what a 32-bit read of the mask would give
    assert not torch.equal(wrapped, mask // d)
    # S == 0: float64 keeps sigmoid(-200) = 1e-87, float32 has 0: the Dice term is 0 within its bound either way
    logits, mask = K.empty_sets_case()
    ref = K.binary_ref(logits, mask)
    own, g = K.binary_f32(logits, mask, 2, logits.numel(), 1.0, 1.0)
    assert float(own[2]) == 0.0 and float(own[3]) == 0.0 and 0 < ref["sums"][2] < 1e-80
    assert abs(ref["dice"]) <= K.DICE_ABS and bool(torch.isfinite(g).all())
    g64, M = K.binary_grad64(ref, logits.numel(), 1.0, 1.0, None)
    assert K.grad_units(g, g64, M, None) <= K.K_RESTATEMENT


def test_dice_integer_cases_are_exact_in_float32():
    for ngroups, group_len in K.DICE_LAYOUTS[:-1]:
        x, t, sums = K.dice_integer_inputs(ngroups, group_len)
        assert float(sums.max()) < 2 ** 24 and torch.equal(sums.float().double(), sums)
        assert float(sums[0].abs().max()) == 0.0 and float(sums[-1].min()) >= (0 if group_len == 1 else 1)
        f = torch.stack([(x.float() * t.float()).sum(1), x.float().sum(1), t.float().sum(1)], 1)
        assert torch.equal(f.double(), sums)
    assert [K.dice_bpg(g, n) for g, n in K.DICE_LAYOUTS] == [1, 1, 1, 2, 4, 1]
    assert 4300 * 2 > K.DICE_WS_ROWS >= 4300 and K.dice_bpg(8449, 1) * 8449 > K.DICE_WS_ROWS


# ------------------------------------------------------------------------------------------------ (b) boundary
def test_boundary_sweep_port_matches_the_oracle_and_is_sensitive():
    assert len(K.SWEEP) == 588
    smallest = 1e9
    for B, H, W, ew in K.SWEEP:
        pred, target = K.boundary_sweep_case(B, H, W, ew)
        want = K.boundary_oracle(pred, target, ew, K.SWEEP_EDGE_WEIGHT)
        counts, sizes = K.oracle_counts(pred, target, ew)
        assert K.port_counts(pred, target, ew) == (counts, sizes), (B, H, W, ew)
        smallest = min(smallest, K.assert_boundary_condition(pred, target, ew, K.SWEEP_EDGE_WEIGHT, want))
    print(f"smallest relative change of the loss for one miscounted pixel: {smallest:.3e} ({smallest / K.BOUNDARY_TOL:.0f} tolerances)")


@pytest.mark.parametrize("name", list(K.BOUNDARY_MID))
def test_boundary_mid_cases_meet_the_condition(name):
    B, H, W, ew, wt, C, kind = K.BOUNDARY_MID[name]
    pred, target = K.boundary_mid_case(name)
    want = K.boundary_oracle(pred, target, ew, wt)
    counts, sizes = K.oracle_counts(pred, target, ew)
    assert K.port_counts(pred, target, ew) == (counts, sizes)
    s = K.assert_boundary_condition(pred, target, ew, wt, want)
    print(f"{name}: loss {want:.9g}, counts {counts}, one pixel moves it by {s:.3e} ({s / K.BOUNDARY_TOL:.0f} tolerances)")
    assert wt <= 3


# ------------------------------------------------------------------------------------------------ (c) seeded mistakes
MISTAKE_CASES = [("sub_wave", 1.0), ("two_blocks", 1.0), ("two_blocks", 10.0)]


def _binary_breaks(shape, scale, mistake, world=1):
    logits, mask = K.binary_inputs(shape, scale, 2)
    ref = K.binary_ref_cached(shape, scale, 2)
    n = ref["n"]
    own, _ = K.binary_f32(logits, mask, 2, n * world, 1.0, 1.0, mistake=mistake)
    g64, M = K.binary_grad64(ref, n * world, 1.0, 1.0, None)
    _, g = K.binary_f32(logits, mask, 2, n * world, 1.0, 1.0, sums=_f32_of(ref["sums"]), mistake=mistake)
    return (not _within(own, ref, (3,), 1.0)), K.grad_units(g, g64, M, None) > K.K_GRAD


def _multiclass_breaks(shape, scale, C, mistake, world=1):
    logits, mask = K.multiclass_inputs(shape, scale, C, "all")
    ref = K.multiclass_ref_cached(shape, scale, C, "all")
    n = ref["n"]
    own, _ = K.multiclass_f32(logits, mask, n * world, 1.0, 1.0, mistake=mistake)
    g64, M = K.multiclass_grad64(ref, n * world, 1.0, 1.0, None)
    _, g = K.multiclass_f32(logits, mask, n * world, 1.0, 1.0, sums=_f32_of(ref["sums"]), mistake=mistake)
    return (not _within(own, ref, tuple(range(1 + 2 * C, 1 + 3 * C)), 1.0)), K.grad_units(g, g64, M, None) > K.K_GRAD


@pytest.mark.parametrize("shape,scale", MISTAKE_CASES)
def test_seeded_mistakes_break_the_binary_bounds(shape, scale):
    assert _binary_breaks(shape, scale, None) == (False, False) and _binary_breaks(shape, scale, None, world=2) == (False, False)
    sums_break, grad_break = _binary_breaks(shape, scale, "tail")
    assert sums_break and grad_break                       # a dropped element shows in the sums AND in its own gradient
    assert _binary_breaks(shape, scale, "n_for_n_mean", world=2)[1]
    assert _binary_breaks(shape, scale, "ka_sign")[1]
    assert all(_binary_breaks(shape, scale, "mask_div"))


@pytest.mark.parametrize("shape", ["second_sweep", "grid_wrap"])
def test_a_dropped_tail_element_shows_at_the_large_shapes_too(shape):
    """One term of 10^6 is inside the sums' relative bound unless its column is a count; the element's own gradient is not."""
    scale = 1.0 if shape == "second_sweep" else 10.0
    logits, mask = K.binary_inputs(shape, scale, 2)
    ref = K.binary_ref_cached(shape, scale, 2)
    n = ref["n"]
    g64, M = K.binary_grad64(ref, n, 1.0, 1.0, None)
    _, g = K.binary_f32(logits, mask, 2, n, 1.0, 1.0, sums=_f32_of(ref["sums"]), mistake="tail")
    assert abs(float(g64.flatten()[-1])) > K.grad_bound(M, None) and K.grad_units(g, g64, M, None) > K.K_GRAD


@pytest.mark.parametrize("C", [2, 3, 8])
@pytest.mark.parametrize("shape,scale", MISTAKE_CASES[1:])
def test_seeded_mistakes_break_the_multiclass_bounds(shape, scale, C):
    assert _multiclass_breaks(shape, scale, C, None) == (False, False)
    assert all(_multiclass_breaks(shape, scale, C, "tail"))
    assert _multiclass_breaks(shape, scale, C, "n_for_n_mean", world=2)[1]
    assert _multiclass_breaks(shape, scale, C, "ka_sign")[1]
    assert all(_multiclass_breaks(shape, scale, C, "class_left_out"))


@pytest.mark.parametrize("name", ["seams", "one_row_interior", "channel_1_of_4"])
@pytest.mark.parametrize("mistake", ["across_interior", "ge"])
def test_seeded_mistakes_break_the_boundary_bound(name, mistake):
    B, H, W, ew, wt, C, kind = K.BOUNDARY_MID[name]
    pred, target = K.boundary_mid_case(name)
    want = K.boundary_oracle(pred, target, ew, wt)
    right = K.loss_from_counts(*K.port_counts(pred, target, ew), wt)
    wrong = K.loss_from_counts(*K.port_counts(pred, target, ew, mistake), wt)
    assert abs(right - want) <= K.BOUNDARY_TOL * abs(want) / 4
    assert abs(wrong - want) > K.BOUNDARY_TOL * abs(want), (wrong, want)


def test_the_sweep_catches_a_neighbour_taken_across_the_interior():
    """... in the geometries that have an interior with an edge band around it, not only at the mid sizes."""
    caught = 0
    for B, H, W, ew in K.SWEEP:
        if ew == 0 or 2 * ew >= H or 2 * ew >= W:
            continue
        pred, target = K.boundary_sweep_case(B, H, W, ew)
        want = K.boundary_oracle(pred, target, ew, K.SWEEP_EDGE_WEIGHT)
        wrong = K.loss_from_counts(*K.port_counts(pred, target, ew, "across_interior"), K.SWEEP_EDGE_WEIGHT)
        caught += abs(wrong - want) > K.BOUNDARY_TOL * abs(want)
    assert caught >= 20, caught
