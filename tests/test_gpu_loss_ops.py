"""The default training loss (csrc/loss.hip) on the MI355X, entry point by entry point, against float64: uh_bce_dice_sums / _grad,
uh_ce_dice_sums / _grad, the two finishes, uh_dice_sums / uh_dice_from_sums, uh_boundary_loss / _mask and the fused binary call,
through LIB.call, and once per family through losses.SegLossBinaryFn (fused and separate), SegLossMulticlassFn and DiceCoeffFn.
Cases, references and bounds are tests/loss_cases.py's; tests/test_loss_ops_cpu.py shows on the CPU that float32 arithmetic meets the
bounds with half the room to spare and that a seeded mistake breaks them.

References.  oracle/losses_ref.py in float64 on the CPU (bce_with_logits_mean, cross_entropy_mean, dice_coeff, dice_loss,
multiclass_dice_coeff) and torch autograd on those; boundary_loss: the same oracle on float32 tensors, whose constants
(clamp(1e-6, 1 - 1e-6), 1 - p) are float32 by definition.

Shapes.  (1,1,3): less than a wave.  (2,37,45) = 3330: two blocks of the sums pass's 2048 stride, ragged tail.  (2,517,511): 258
partial rows, so the finishing block's column sum takes a second sweep.  (1,1031,1021) = 1 052 651 elements (pixels for C = 2):
the gradient kernels' grid of 4096 blocks goes round.  Logits N(0,1) * s, s in {1, 10, 100}: at 100 sigmoid and softmax saturate and
expf returns denormals and 0.

Bounds, fixed before any kernel ran.  With u = 2^-24:
  * sums.  Every column is a sum of non-negative terms (the BCE term is |x| [sign disagrees] + log1p(e), the CE term lse - x_t >= 0,
    the others are probabilities and 0/1 targets), so errors do not cancel into a larger relative one.  A thread adds at most 8
    terms up to 2^21 elements (8 u), then 6 shuffle levels (6 u), 3 LDS adds and the store of the double finish (2 u); with 8 u
    presumed for the element's own expf / log1pf / division:  |got - S64| <= 24 u S64 + n 2^-126, the floor being what terms below
    the normal range can lose.  Columns that are counts (sum t, the per-class label counts) are equal.
    Finding (softmax columns only): float32 rounds x_c - max(x) before expf, so a term exp(x_c - max) carries |x_c - max| u on top
    of expf's own error: 23 u at p = 1e-10, 87 u at the edge of the normal range.  A column of 10^3 pixels is made of terms near
    the maximum and does not notice; the 3-pixel case at s = 10 and 100 consists of such tails alone and the float32 restatement
    already sits at 16.5 u there.  The kernel's arithmetic is the natural one (the exact difference would need a second float), so
    the bound of these columns carries the term  u sum_i p_ic |x_ic - max_i|  computed from the float64 terms (loss_cases
    .multiclass_ref, "slack"): 104 u S at the very most, 6.2e-6 S, inside the project's op-by-op 2e-5.
  * loss terms.  BCE / CE mean: the sums bound and 2 u (1 / n_mean, the product).  dice_loss = 1 - ratio cancels: absolutely
    2 (24 u) + 4 u.  total: the sum of its terms' bounds and one ulp of the total.
  * gradients, per element, not by a norm:  |got - g64| <= K u M |gscale|,  M = |w_bce| / n_mean + |w_dice| (|ka| + |kb|) / 4
    (binary: s (1 - s) <= 1/4),  M = |w_ce| / n_mean + |w_dice| (|ka| + |kb|)  (multi-class), ka and kb from the float64 sums.
    K = 16 was fixed as four times what a float32 restatement of the closed forms showed against float64 (3.9); the CPU
    companion re-measures the restatement at every case (3.46 binary, 4.84 multi-class at most) and requires <= 8, so the kernels
    have twice the restatement's room at the least.
  * boundary_loss: relative 2e-5 against the float32 oracle, the bound fixture G7 is held to; for every case the CPU side
    asserts that +-1 in any of the oracle's six counts moves the loss by at least 4 tolerances, so the comparison cannot hide one
    miscounted pixel.
    Finding, fixed in loss.hip: the oracle's per-pixel BCE at logit(1e-6), target 0 is 2^-20 in float32 ((1 - t) x - logsigmoid(x)
    is one ulp of x), the kernel's max(x, 0) - x t + log1p(e) gave 1e-6.  Where every dilated pixel agrees the whole loss is that
    term, ~5e-7, and was 4.6 % off (33 of the sweep's 588 geometries have such a loss); boundary_region_loss now forms the four pixel
    terms in the oracle's order.  Where any pixel disagrees the change is below one ulp of the loss.
  * dice_coeff: on small integers every sum is an exact integer below 2^24: torch.equal.  On random probabilities value and
    backward are held to the op-by-op 2e-5.
"Two calls return the same bits" and "each half batch, given the whole batch's sums, gives the whole gradient" are equalities.
Not reached: boundary_count_kernel<int64_t> (chosen from 2^31 - 2^18 pixels on; no case here is larger than 1 052 651) and the NaN
flag of the fused call (test_gpu_parity.py holds it).

Measured on the MI355X (worst over all cases; the tests print each):
  binary       sums 1.27 u S64 (bound 24), gradient 3.46 units of u M (bound 16; the float32 restatement 3.46);
               through SegLossBinaryFn, fused and separate alike, 1.66
  multi-class  sums 1.83 u S64 beyond the slack (bound 24), gradient 4.84 units at C = 8, s = 10 (bound 16; the restatement 4.84); through
               SegLossMulticlassFn 1.67
  dice_coeff   integer sums equal; random probabilities: value 5.2e-8, backward 7.6e-8 (bound 2e-5)
  boundary     588 geometries x {float, mask, fused}: 2.4e-7 relative (bound 2e-5), the three forms the same bits; mid sizes 1.5e-7;
               one miscounted pixel would move the mid-size cases by 2.2e-4 to 5.7e-4, the small ones by 1.7e-2 or more"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import loss_cases as K
from oracle import losses_ref as L

pytestmark = pytest.mark.gpu

_ids = lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else None      # noqa: E731
EINVAL = -1


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    return torch.device("cuda:0")


def _lib():
    import unet_amd  # noqa: F401
    from unet_amd import losses
    from unet_amd._lib import LIB
    return losses, LIB


def _p(t):
    return None if t is None else t.data_ptr()


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _gs(gscale, dev):
    return None if gscale is None else torch.tensor([gscale], dtype=torch.float32, device=dev)


def _f32_sums(ref, dev):
    """The float64 sums, each rounded once to float32: the gradient kernels are tested apart from the sums kernels."""
    return torch.tensor(ref["sums"], dtype=torch.float64).float().to(dev)


# ------------------------------------------------------------------------------------------------ the C ABI, one call each
def binary_sums(lg, mk, div, tf):
    losses, LIB = _lib()
    sums = torch.empty(4, dtype=torch.float32, device=lg.device)
    ws = losses.loss_workspace(lg.device)
    LIB.call("uh_bce_dice_sums", lg.data_ptr(), _p(mk), int(div), _p(tf), lg.numel(), sums.data_ptr(), ws.data_ptr(), ws.numel(), None)
    return sums


def binary_finish(sums, n_mean):
    _, LIB = _lib()
    out = torch.empty(4, dtype=torch.float32, device=sums.device)
    LIB.call("uh_seg_loss_binary_finish", sums.data_ptr(), float(n_mean), None, 0.0, out.data_ptr(), None)
    return out.cpu()


def binary_grad(lg, mk, div, tf, sums, n_mean, w_bce, w_dice, gscale):
    _, LIB = _lib()
    dl = torch.full_like(lg, float("nan"))
    gs = _gs(gscale, lg.device)
    LIB.call("uh_bce_dice_grad", lg.data_ptr(), _p(mk), int(div), _p(tf), lg.numel(), sums.data_ptr(), float(n_mean), float(w_bce),
             float(w_dice), _p(gs), dl.data_ptr(), None)
    return dl


def multiclass_sums(lg, mk):
    losses, LIB = _lib()
    C = lg.shape[-1]
    sums = torch.empty(1 + 3 * C, dtype=torch.float32, device=lg.device)
    ws = losses.loss_workspace(lg.device)
    LIB.call("uh_ce_dice_sums", lg.data_ptr(), mk.data_ptr(), mk.numel(), C, sums.data_ptr(), ws.data_ptr(), ws.numel(), None)
    return sums


def multiclass_finish(sums, C, n_mean):
    _, LIB = _lib()
    out = torch.empty(4, dtype=torch.float32, device=sums.device)
    LIB.call("uh_seg_loss_multiclass_finish", sums.data_ptr(), C, float(n_mean), None, 0.0, out.data_ptr(), None)
    return out.cpu()


def multiclass_grad(lg, mk, sums, n_mean, w_ce, w_dice, gscale):
    _, LIB = _lib()
    dl = torch.full_like(lg, float("nan"))
    gs = _gs(gscale, lg.device)
    LIB.call("uh_ce_dice_grad", lg.data_ptr(), mk.data_ptr(), mk.numel(), lg.shape[-1], sums.data_ptr(), float(n_mean), float(w_ce),
             float(w_dice), _p(gs), dl.data_ptr(), None)
    return dl


def _check_terms(out, mean64, sum64, dice64, n, n_mean, what):
    """out = {total, mean, dice_loss, boundary = 0} of a finish call against float64.  Returns the errors as fractions of the bounds."""
    total, mean, dice, bnd = (float(v) for v in out)
    b_mean = K.mean_bound(sum64, n, n_mean)
    want_mean = mean64 * n / n_mean
    assert bnd == 0.0
    e_mean, e_dice, e_total = abs(mean - want_mean), abs(dice - dice64), abs(total - (want_mean + dice64))
    print(f"  {what}: mean {mean:.9g} off {e_mean:.3e} (bound {b_mean:.3e}); dice_loss {dice:.9g} off {e_dice:.3e} (bound {K.DICE_ABS:.3e}); "
          f"total {total:.9g} off {e_total:.3e}")
    assert e_mean <= b_mean and e_dice <= K.DICE_ABS
    assert e_total <= K.total_bound([b_mean, K.DICE_ABS], total)
    return e_mean / b_mean, e_dice / K.DICE_ABS


# ------------------------------------------------------------------------------------------------ binary: sums, terms, gradient
@pytest.mark.parametrize("case", K.BINARY_CASES, ids=_ids)
def test_binary_sums_terms_and_gradient_against_float64(case):
    shape, scale, div, soft = case
    dev = _dev()
    logits, m = K.binary_inputs(*case)
    ref = K.binary_ref_cached(*case)
    n = ref["n"]
    lg = logits.to(dev)
    mk, tf = (None, m.to(dev)) if soft else (m.to(dev), None)
    sums = binary_sums(lg, mk, div, tf)
    assert torch.equal(_bits(sums), _bits(binary_sums(lg, mk, div, tf)))                       # two calls, the same bits
    units = K.check_sums(sums.cpu(), ref, () if soft else (3,))
    print(f"{case}: sums {sums.cpu().tolist()}; worst column {units:.2f} units of 2^-24 S64 (bound {K.SUM_ULPS})")
    for world in (1, 2):
        _check_terms(binary_finish(sums, n * world), ref["bce"], ref["sums"][0], ref["dice"], n, n * world, f"n_mean = {world} n")
    handed = _f32_sums(ref, dev)
    worst = 0.0
    for world, (w_bce, w_dice), gs in K.grad_settings(shape):
        g64, M = K.binary_grad64(ref, n * world, w_bce, w_dice, gs)
        g = binary_grad(lg, mk, div, tf, handed, n * world, w_bce, w_dice, gs)
        got = K.grad_units(g.cpu(), g64, M, gs)
        worst = max(worst, got)
        assert got <= K.K_GRAD, (world, w_bce, w_dice, gs, got)
    print(f"{case}: worst gradient element {worst:.2f} units of 2^-24 M |gscale| (bound {K.K_GRAD})")
    g = binary_grad(lg, mk, div, tf, handed, n, 0.3, 0.7, 0.5)
    assert torch.equal(_bits(g), _bits(binary_grad(lg, mk, div, tf, handed, n, 0.3, 0.7, 0.5)))


def test_binary_mask_elements_past_31_bits_take_the_64_bit_division():
    dev = _dev()
    logits, mask, d = K.wide_mask_case()
    ref = K.binary_ref(logits, mask // d)
    lg, mk = logits.to(dev), mask.to(dev)
    sums = binary_sums(lg, mk, d, None)
    print(f"sums {sums.cpu().tolist()} against {ref['sums']}")
    K.check_sums(sums.cpu(), ref, (3,))
    g64, M = K.binary_grad64(ref, 4, 1.0, 1.0, None)
    assert K.grad_units(binary_grad(lg, mk, d, None, _f32_sums(ref, dev), 4, 1.0, 1.0, None).cpu(), g64, M, None) <= K.K_GRAD


def test_binary_empty_sets_give_dice_loss_zero_and_a_finite_gradient():
    """S == 0 (every sigmoid underflows to 0, no target set): the ratio is (0 + eps) / (0 + eps) and ka = kb = 0."""
    dev = _dev()
    logits, mask = K.empty_sets_case()
    ref = K.binary_ref(logits, mask)
    n = ref["n"]
    lg, mk = logits.to(dev), mask.to(dev)
    sums = binary_sums(lg, mk, 2, None)
    assert sums.cpu().tolist()[1:] == [0.0, 0.0, 0.0]
    K.check_sums(sums.cpu(), ref, (3,))
    out = binary_finish(sums, n)
    assert float(out[2]) == 0.0 and bool(torch.isfinite(out).all())
    for w in K.WEIGHTS:
        g = binary_grad(lg, mk, 2, None, sums, n, *w, None).cpu()
        g64, M = K.binary_grad64(ref, n, *w, None)
        assert bool(torch.isfinite(g).all()) and K.grad_units(g, g64, M, None) <= K.K_GRAD


def test_binary_half_batches_with_the_whole_sums_give_the_whole_gradient():
    """What a data-parallel rank computes: its own half of the logits, the sums and the element count of the global batch."""
    dev = _dev()
    logits, mask = K.binary_inputs("two_blocks", 10.0, 2)
    lg, mk = logits.to(dev), mask.to(dev)
    sums = binary_sums(lg, mk, 2, None)
    whole = binary_grad(lg, mk, 2, None, sums, lg.numel(), 1.0, 1.0, 0.5)
    halves = [binary_grad(lg[b:b + 1].contiguous(), mk[b:b + 1].contiguous(), 2, None, sums, lg.numel(), 1.0, 1.0, 0.5) for b in range(2)]
    assert float(whole.abs().max()) > 0 and torch.equal(_bits(torch.cat(halves)), _bits(whole))


@pytest.mark.parametrize("fuse", [True, False], ids=["fused", "separate"])
def test_seg_loss_binary_fn_against_float64(fuse):
    """The node train_step uses: every term, the total with the boundary term in it, and the gradient that backward() returns
    from the kernel's own sums."""
    losses, _ = _lib()
    dev = _dev()
    ew, wt, w_b = 5, 3.0, 0.25
    logits, mask = K.binary_inputs("two_blocks", 1.0, 2)
    ref = K.binary_ref_cached("two_blocks", 1.0, 2)
    n = ref["n"]
    assert float(logits.abs().max()) <= 10                                  # boundary_loss reads the logits as they are
    target = (mask // 2).float()
    bnd64 = K.boundary_oracle(logits, target, ew, wt)
    K.assert_boundary_condition(logits, target, ew, wt, bnd64)
    default = losses.FUSE_LOSS
    try:
        losses.FUSE_LOSS = fuse
        lg = logits.to(dev).requires_grad_()
        total, bce, dice, bnd, nan_flag = losses.SegLossBinaryFn.apply(lg, mask.to(dev), 2, w_b, ew, wt, None, 1)
        assert (nan_flag is not None) == fuse
        total.backward()
        total, bce, dice, bnd = (v.detach() for v in (total, bce, dice, bnd))
    finally:
        losses.FUSE_LOSS = default
    b_mean = K.mean_bound(ref["sums"][0], n, n)
    b_bnd = K.BOUNDARY_TOL * abs(bnd64)
    want = ref["bce"] + ref["dice"] + w_b * bnd64
    errs = (abs(float(bce) - ref["bce"]), abs(float(dice) - ref["dice"]), abs(float(bnd) - bnd64), abs(float(total) - want))
    print(f"fuse {fuse}: bce {float(bce):.9g} dice {float(dice):.9g} boundary {float(bnd):.9g} total {float(total):.9g}; off by {errs}")
    assert errs[0] <= b_mean and errs[1] <= K.DICE_ABS and errs[2] <= b_bnd
    assert errs[3] <= K.total_bound([b_mean, K.DICE_ABS, w_b * b_bnd], float(total))
    g64, M = K.binary_grad64(ref, n, 1.0, 1.0, None)
    units = K.grad_units(lg.grad.cpu(), g64, M, None)
    print(f"fuse {fuse}: worst gradient element {units:.2f} units of 2^-24 M")
    assert units <= K.K_GRAD


# ------------------------------------------------------------------------------------------------ multi-class
@pytest.mark.parametrize("case", K.MULTICLASS_CASES, ids=_ids)
def test_multiclass_sums_terms_and_gradient_against_float64(case):
    shape, scale, C, labels = case
    dev = _dev()
    logits, mask = K.multiclass_inputs(*case)
    ref = K.multiclass_ref_cached(*case)
    n = ref["n"]
    assert (int((mask == C - 1).sum()) == 0) == (labels == "absent")
    lg, mk = logits.to(dev), mask.to(dev)
    sums = multiclass_sums(lg, mk)
    assert torch.equal(_bits(sums), _bits(multiclass_sums(lg, mk)))
    units = K.check_sums(sums.cpu(), ref, tuple(range(1 + 2 * C, 1 + 3 * C)))
    print(f"{case}: worst sums column {units:.2f} units of 2^-24 S64 beyond its slack (bound {K.SUM_ULPS})")
    for world in (1, 2):
        _check_terms(multiclass_finish(sums, C, n * world), ref["ce"], ref["sums"][0], ref["dice"], n, n * world, f"n_mean = {world} n")
    handed = _f32_sums(ref, dev)
    worst = 0.0
    for world, (w_ce, w_dice), gs in K.grad_settings(shape):
        g64, M = K.multiclass_grad64(ref, n * world, w_ce, w_dice, gs)
        got = K.grad_units(multiclass_grad(lg, mk, handed, n * world, w_ce, w_dice, gs).cpu(), g64, M, gs)
        worst = max(worst, got)
        assert got <= K.K_GRAD, (world, w_ce, w_dice, gs, got)
    print(f"{case}: worst gradient element {worst:.2f} units of 2^-24 M |gscale| (bound {K.K_GRAD})")
    g = multiclass_grad(lg, mk, handed, n, 0.3, 0.7, 0.5)
    assert torch.equal(_bits(g), _bits(multiclass_grad(lg, mk, handed, n, 0.3, 0.7, 0.5)))


@pytest.mark.parametrize("C", [2, 3, 8])
def test_multiclass_half_batches_with_the_whole_sums_give_the_whole_gradient(C):
    dev = _dev()
    logits, mask = K.multiclass_inputs("two_blocks", 10.0, C, "all")
    lg, mk = logits.to(dev), mask.to(dev)
    sums = multiclass_sums(lg, mk)
    whole = multiclass_grad(lg, mk, sums, mk.numel(), 1.0, 1.0, 0.5)
    halves = [multiclass_grad(lg[b:b + 1].contiguous(), mk[b:b + 1].contiguous(), sums, mk.numel(), 1.0, 1.0, 0.5) for b in range(2)]
    assert float(whole.abs().max()) > 0 and torch.equal(_bits(torch.cat(halves)), _bits(whole))


def test_seg_loss_multiclass_fn_against_float64():
    """The multi-class node with its boundary term: channel 1 of the NHWC logits, pstride = C, bstride = H W C."""
    losses, _ = _lib()
    dev = _dev()
    (B, H, W, C, ew, wt, w_b), logits, mask = K.multiclass_node_case()
    ref = K.multiclass_ref(logits, mask)
    n = ref["n"]
    bnd64 = K.boundary_oracle(logits, mask.float(), ew, wt)
    K.assert_boundary_condition(logits, mask.float(), ew, wt, bnd64)
    lg = logits.to(dev).requires_grad_()
    out = losses.SegLossMulticlassFn.apply(lg, mask.to(dev), w_b, ew, wt, None, 1)
    out[0].backward()
    total, ce, dice, bnd = (float(v) for v in out.detach().cpu())
    b_mean = K.mean_bound(ref["sums"][0], n, n)
    b_bnd = K.BOUNDARY_TOL * abs(bnd64)
    errs = (abs(ce - ref["ce"]), abs(dice - ref["dice"]), abs(bnd - bnd64), abs(total - (ref["ce"] + ref["dice"] + w_b * bnd64)))
    print(f"ce {ce:.9g} dice {dice:.9g} boundary {bnd:.9g} total {total:.9g}; off by {errs}")
    assert errs[0] <= b_mean and errs[1] <= K.DICE_ABS and errs[2] <= b_bnd
    assert errs[3] <= K.total_bound([b_mean, K.DICE_ABS, w_b * b_bnd], total)
    g64, M = K.multiclass_grad64(ref, n, 1.0, 1.0, None)
    units = K.grad_units(lg.grad.cpu(), g64, M, None)
    print(f"worst gradient element {units:.2f} units of 2^-24 M")
    assert units <= K.K_GRAD


def test_multiclass_entry_points_refuse_1_and_9_classes_with_an_error_code():
    """Called from the CPU side with stand-in pointers: the check sits in front of the launch, nothing is followed."""
    _, LIB = _lib()
    dll = LIB.load()
    P = 4096
    big = LIB.query("uh_loss_ws_bytes", 100)
    for ncls in (1, 9):
        assert dll.uh_ce_dice_sums(P, P, 100, ncls, P, P, big, None) == EINVAL
        assert dll.uh_ce_dice_grad(P, P, 100, ncls, P, 100.0, 1.0, 1.0, None, P, None) == EINVAL
        assert dll.uh_seg_loss_multiclass_finish(P, ncls, 100.0, None, 0.0, P, None) == EINVAL
    assert dll.uh_ce_dice_sums(P, P, 100, 3, P, P, big - 1, None) == EINVAL


# ------------------------------------------------------------------------------------------------ dice_coeff
@pytest.mark.parametrize("ngroups,group_len", K.DICE_LAYOUTS)
def test_dice_sums_of_small_integers_are_exact(ngroups, group_len):
    losses, LIB = _lib()
    dev = _dev()
    x, t, want = K.dice_integer_inputs(ngroups, group_len)
    xf, tf = x.to(dev).float(), t.to(dev).float()
    sums = torch.empty(ngroups * 3, dtype=torch.float32, device=dev)
    ws = losses.loss_workspace(dev)
    assert ws.numel() // 16 == K.DICE_WS_ROWS
    LIB.call("uh_dice_sums", xf.data_ptr(), tf.data_ptr(), ngroups, group_len, sums.data_ptr(), ws.data_ptr(), ws.numel(), None)
    assert torch.equal(sums.cpu().double().view(ngroups, 3), want)
    out = torch.empty(2, dtype=torch.float32, device=dev)
    LIB.call("uh_dice_from_sums", sums.data_ptr(), ngroups, 1e-6, out.data_ptr(), None)
    LIB.call("uh_dice_from_sums", sums.data_ptr(), 1, 1e-6, out[1:].data_ptr(), None)            # group 0 alone: all zero
    want_v = K.dice_from_sums64(want)
    got, first = (float(v) for v in out.cpu())
    print(f"{ngroups} groups of {group_len} (blocks per group {K.dice_bpg(ngroups, group_len)}): dice {got:.9g}, off by {abs(got - want_v) / want_v:.3e}")
    assert abs(got - want_v) <= K.OP_TOL * want_v
    assert first == 1.0                                                                        # an all-zero group scores 1


def test_dice_sums_refuses_more_groups_than_the_workspace_holds():
    _, LIB = _lib()
    dll = LIB.load()
    P = 4096
    big = LIB.query("uh_loss_ws_bytes", 100)
    assert big // 16 == K.DICE_WS_ROWS
    assert dll.uh_dice_sums(P, P, K.DICE_WS_ROWS + 1, 1, P, P, big, None) == EINVAL
    assert b"workspace" in dll.uh_last_error()


@pytest.mark.parametrize("rbf", [True, False])
@pytest.mark.parametrize("shape", [(2, 37, 45), (3, 64, 65)], ids=_ids)
def test_dice_coeff_fn_value_and_backward_against_float64(shape, rbf):
    losses, _ = _lib()
    dev = _dev()
    g = torch.Generator().manual_seed(shape[1] + rbf)
    x = torch.rand(shape, generator=g)
    t = torch.randint(0, 2, shape, generator=g).float()
    x64 = x.double().requires_grad_()
    want = L.dice_coeff(x64, t.double(), reduce_batch_first=rbf)
    want.backward()
    ngroups = 1 if rbf else shape[0]
    xg = x.to(dev).requires_grad_()
    got = losses.DiceCoeffFn.apply(xg, t.to(dev), ngroups, x.numel() // ngroups, 1e-6)
    got.backward()
    got, want = got.detach(), want.detach()
    rel = abs(float(got) - float(want)) / float(want)
    rel_g = float((xg.grad.cpu().double() - x64.grad).abs().max() / x64.grad.abs().max())
    print(f"{shape} reduce_batch_first {rbf}: dice {float(got):.9g}, relative error {rel:.3e}; gradient, worst element over the largest {rel_g:.3e}")
    assert rel <= K.OP_TOL and rel_g <= K.OP_TOL


# ------------------------------------------------------------------------------------------------ boundary_loss
def _boundary(pred, pstride, bstride, target, B, H, W, ew, wt, out):
    losses, LIB = _lib()
    ws = losses.loss_workspace(pred.device)
    LIB.call("uh_boundary_loss", pred.data_ptr(), pstride, bstride, target.data_ptr(), B, H, W, ew, wt, 1e-6, out.data_ptr(),
             ws.data_ptr(), ws.numel(), None)


def _boundary_mask(pred, mask, div, B, H, W, ew, wt, out):
    losses, LIB = _lib()
    ws = losses.loss_workspace(pred.device)
    LIB.call("uh_boundary_loss_mask", pred.data_ptr(), 1, H * W, mask.data_ptr(), div, B, H, W, ew, wt, 1e-6, out.data_ptr(),
             ws.data_ptr(), ws.numel(), None)


def _boundary_fused(pred, mask, div, B, H, W, ew, wt):
    """The boundary term (out[3]) of the fused binary call."""
    _, LIB = _lib()
    dev = pred.device
    sums, out = torch.empty(4, dtype=torch.float32, device=dev), torch.empty(5, dtype=torch.float32, device=dev)
    ws = torch.empty(LIB.query("uh_seg_loss_fused_ws_bytes"), dtype=torch.uint8, device=dev)
    LIB.call("uh_seg_loss_binary_fused", pred.data_ptr(), mask.data_ptr(), div, B, H, W, ew, wt, 1e-6, 1.0, float(B * H * W),
             sums.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(), None)
    return out[3:4]


@pytest.mark.parametrize("B", [1, 2])
def test_boundary_sweep_of_small_geometries(B):
    """H, W in 1..7, edge width 0..5: an interior one pixel wide or high, 2 ew >= H or W, ew >= H, ew = 0.  Probabilities in
    {0.25, 0.75}, targets in {0, 128, 255}; the float form, the mask form on {0, 255} and the fused call's term."""
    dev = _dev()
    cases = [c for c in K.SWEEP if c[0] == B]
    assert len(cases) == 294
    wt = K.SWEEP_EDGE_WEIGHT
    got = torch.full((len(cases), 3), float("nan"), dtype=torch.float32, device=dev)
    want = []
    for i, (_, H, W, ew) in enumerate(cases):
        pred, target = K.boundary_sweep_case(B, H, W, ew)
        w = K.boundary_oracle(pred, target, ew, wt)
        K.assert_boundary_condition(pred, target, ew, wt, w)
        want.append(w)
        p, t = pred.to(dev), target.to(dev)
        mask = (t == 255).long() * 255
        _boundary(p, 1, H * W, t, B, H, W, ew, wt, got[i, 0:1])
        _boundary_mask(p, mask, 1, B, H, W, ew, wt, got[i, 1:2])
        got[i, 2:3].copy_(_boundary_fused(p, mask, 1, B, H, W, ew, wt))
    got = got.cpu().double()
    want = torch.tensor(want, dtype=torch.float64)
    rel = (got - want[:, None]).abs() / want[:, None].abs()
    i = int(rel.max(1).values.argmax())
    print(f"B {B}: worst relative error {float(rel.max()):.3e} at H, W, ew = {cases[i][1:]} (got {got[i].tolist()}, oracle {float(want[i]):.9g})")
    assert bool((rel <= K.BOUNDARY_TOL).all()), [(cases[j], got[j].tolist(), float(want[j])) for j in torch.nonzero(rel.max(1).values > K.BOUNDARY_TOL).flatten().tolist()[:8]]
    assert torch.equal(got[:, 0], got[:, 1]) and torch.equal(got[:, 0], got[:, 2])


@pytest.mark.parametrize("name", list(K.BOUNDARY_MID))
def test_boundary_where_region_runs_cross_block_seams(name):
    dev = _dev()
    B, H, W, ew, wt, C, kind = K.BOUNDARY_MID[name]
    pred, target = K.boundary_mid_case(name)
    want = K.boundary_oracle(pred, target, ew, wt)
    K.assert_boundary_condition(pred, target, ew, wt, want)
    p, t = pred.to(dev), target.to(dev)
    out = torch.full((3,), float("nan"), dtype=torch.float32, device=dev)
    if C == 1:
        mask = (t == 255).long() * 255
        _boundary(p, 1, H * W, t, B, H, W, ew, wt, out[0:1])
        _boundary_mask(p, mask, 1, B, H, W, ew, wt, out[1:2])
        out[2:3].copy_(_boundary_fused(p, mask, 1, B, H, W, ew, wt))
    else:
        ch1 = p[..., 1]
        assert ch1.data_ptr() == p.data_ptr() + 4 and ch1.stride() == (H * W * C, W * C, C)
        _boundary(ch1, C, H * W * C, t, B, H, W, ew, wt, out[0:1])
        out[1:].copy_(out[0:1].expand(2))
    got = out.cpu().double()
    rel = float(((got - want).abs() / abs(want)).max())
    print(f"{name}: got {got.tolist()}, oracle {want:.9g}, relative error {rel:.3e}")
    assert rel <= K.BOUNDARY_TOL
    assert float(got[0]) == float(got[1]) == float(got[2])
