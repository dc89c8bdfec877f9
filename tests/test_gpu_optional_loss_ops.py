"""The three optional training losses on the MI355X, entry point by entry point, against float64 per element:
uh_focal_tversky_sums / _finish / _grad (csrc/focal_loss.hip), uh_distill_sums / _finish / _grad (csrc/distill_loss.hip),
uh_surface_loss_sums / _grad with rebuild 0 and 1 and uh_surface_dist_map (csrc/surface_loss.hip), each through LIB.call, and once
per family through losses.FocalTverskyLossFn, SurfaceLossFn and DistillLossFn.  Cases, references, bounds and the constants R / 2 R are
tests/optional_loss_cases.py's (its docstring derives the bounds); tests/test_optional_loss_ops_cpu.py shows on the CPU that a float32
restatement stays within R and that each seeded mistake breaks an assertion made here.

What is new against test_gpu_focal_loss.py, test_gpu_surface_loss.py and test_gpu_distill.py (which stay as they are):
  * size: 528 374, 1 052 651 and 2 105 302 pixels -- the second sweep of column_sum_256 and sl_finish_kernel, the gradient and map
    grids going round past 4096 * 256 pixels, the row cap of 1024;
  * the saturated family: every sum an exact integer combination, compared with torch.equal, the finished values bit for bit, at
    all five shapes, the disagreeing pixels on the indices where a grid walk can slip;
  * gradients per element, |got - g64| <= |gscale| (K u M_x + slack_x), fed the float64 sums rounded once to float32, NaN pre-filled;
  * values against the absolute sum of the terms that were added (kd, surface);
  * surface heads 2, 5, 8, the 16-byte row path at NC = 8, the dword fallback of NC = 4 and 8 for pointers off the 16-byte grid;
    labels outside the focal head; teacher = student + 1e-3 N(0,1).
"Two calls return the same bits" and "each half batch, given the whole batch's sums / pixel count, gives the whole gradient" are
equalities, at second_sweep.  Not reached: pixel counts past 2^31 (the 64-bit index arithmetic of every walk).

Kernel change (csrc/uh_loss_reduce.h, uh_mask_quot): a mask outside [0, 2^31) took the truncating 64-bit division, so the mask -1
under mask_div 2 became class 0 and was given weight, where `//` of the reference makes it -1, a label outside the head.  Read from
the code while the out-of-head cases were written (it never ran on the device in that form); the quotient is now floored, as
the label quotient of surface_loss.hip always was.  The case that holds it: the saturated one-channel focal head, whose W and T_0 are equalities
(test_saturated_focal_sums_are_exact_and_the_finish_bit_for_bit).  Masks in [0, 2^31) take the same instructions as before.

Measured on the MI355X (worst over all cases; the tests print each next to its bound; no bound was exceeded):
  saturated      every focal column, both distillation columns and the surface value equal at all five shapes, the finishes bit for bit
  focal          sums 1.75 u S64 beyond the slack (bound 24; W and the T_c equal), gradient 3.80 units of u M (bound 8; the float32
                 restatement 3.80); through FocalTverskyLossFn 2.30
  distillation   kd sum 1.22 units of u A (bound 4; the restatement 1.22), agree equal, gradient 3.80 units (bound 8; the restatement
                 3.77); through DistillLossFn 2.94
  surface        value 0.00 units of u sum |p phi| beyond the slack and the store (bound 2: the sum is formed in double), gradient
                 8.10 units at C = 8, K = 1, s = 1 (bound 32; the restatement 8.10), sigmoid head 5.93 (bound 16; the restatement
                 5.93: sg (1 - sg) stays inside the absolute bound); the dword path of NC = 4 and 8 the aligned bits; maps at
                 1 052 651 pixels bit for bit; through SurfaceLossFn 5.64 (sigmoid) and 1.74"""
import ctypes

import numpy as np
import pytest
import torch

import optional_loss_cases as K

pytestmark = pytest.mark.gpu

_ids = lambda v: "-".join(map(str, v)).replace(" ", "") if isinstance(v, tuple) else None      # noqa: E731
_DEV = {}


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    return torch.device("cuda:0")


def _lib():
    import unet_amd  # noqa: F401
    from unet_amd import losses
    from unet_amd._lib import LIB
    return losses, LIB


def _up(key, *tensors):
    """Inputs are uploaded once per case."""
    if key not in _DEV:
        dev = _dev()
        _DEV[key] = tuple((torch.from_numpy(t) if isinstance(t, np.ndarray) else t).to(dev).contiguous() for t in tensors)
    return _DEV[key]


def _p(t):
    return None if t is None else t.data_ptr()


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _gs(gscale, dev):
    return None if gscale is None else torch.tensor([gscale], dtype=torch.float32, device=dev)


def _f32(values, dev):
    """float64 values, each rounded once to float32: the gradient and finish kernels are tested apart from the sums kernels."""
    return torch.tensor(values, dtype=torch.float64).float().to(dev)


def _ints(v):
    return (ctypes.c_int * len(v))(*v)


def _floats(v):
    return (ctypes.c_float * len(v))(*v)


# ------------------------------------------------------------------------------------------------ the C ABI, one call each
def focal_sums(lg, mk, div, ncls, w, gamma):
    losses, LIB = _lib()
    sums = torch.full((LIB.query("uh_focal_tversky_nsums", ncls),), float("nan"), dtype=torch.float32, device=lg.device)
    ws = losses.loss_workspace(lg.device)
    LIB.call("uh_focal_tversky_sums", lg.data_ptr(), mk.data_ptr(), int(div), mk.numel(), ncls, _floats(w), float(gamma), sums.data_ptr(),
             ws.data_ptr(), ws.numel(), None)
    return sums


def focal_finish(sums, ncls, alpha, beta, cls):
    _, LIB = _lib()
    out = torch.full((3,), float("nan"), dtype=torch.float32, device=sums.device)
    LIB.call("uh_focal_tversky_finish", sums.data_ptr(), ncls, float(alpha), float(beta), _ints(cls), len(cls), out.data_ptr(), None)
    return out.cpu()


def focal_grad(lg, mk, div, ncls, w, gamma, alpha, beta, cls, sums, gscale):
    _, LIB = _lib()
    dl = torch.full_like(lg, float("nan"))
    gs = _gs(gscale, lg.device)
    LIB.call("uh_focal_tversky_grad", lg.data_ptr(), mk.data_ptr(), int(div), mk.numel(), ncls, _floats(w), float(gamma), float(alpha),
             float(beta), _ints(cls), len(cls), sums.data_ptr(), _p(gs), dl.data_ptr(), None)
    return dl


def distill_sums(z, v, ncls, T):
    losses, LIB = _lib()
    sums = torch.full((2,), float("nan"), dtype=torch.float32, device=z.device)
    ws = losses.loss_workspace(z.device)
    LIB.call("uh_distill_sums", z.data_ptr(), v.data_ptr(), z.shape[0], ncls, float(T), sums.data_ptr(), ws.data_ptr(), ws.numel(), None)
    return sums


def distill_finish(sums, n_mean, T, w):
    _, LIB = _lib()
    out = torch.full((3,), float("nan"), dtype=torch.float32, device=sums.device)
    LIB.call("uh_distill_finish", sums.data_ptr(), float(n_mean), float(T), float(w), out.data_ptr(), None)
    return out.cpu()


def distill_grad(z, v, ncls, n_mean, T, w, gscale):
    _, LIB = _lib()
    dl = torch.full_like(z, float("nan"))
    gs = _gs(gscale, z.device)
    LIB.call("uh_distill_grad", z.data_ptr(), v.data_ptr(), z.shape[0], ncls, float(n_mean), float(T), float(w), _p(gs), dl.data_ptr(), None)
    return dl


def surface_ws(shape, K_sel, dev, fill=None):
    _, LIB = _lib()
    B, H, W = shape
    ws = torch.empty(LIB.query("uh_surface_loss_ws_bytes", B, H, W, K_sel), dtype=torch.uint8, device=dev)
    if fill is not None:
        ws.fill_(fill)
    return ws


def surface_sums(lg, mk, ncls, classes, n_mean, w, ws):
    """mk: int64 [B,H,W]; lg: a tensor or view of B H W ncls floats.  Returns {surface, w surface}; the distances stay in ws."""
    _, LIB = _lib()
    B, H, W = mk.shape
    out = torch.full((2,), float("nan"), dtype=torch.float32, device=mk.device)
    LIB.call("uh_surface_loss_sums", lg.data_ptr(), mk.data_ptr(), 2 if ncls == 1 else 1, _ints(classes), len(classes), ncls, B, H, W,
             float(n_mean), float(w), out.data_ptr(), ws.data_ptr(), ws.numel(), None)
    return out


def surface_grad(lg, mk, ncls, classes, n_mean, w, gscale, ws, rebuild, dl=None):
    _, LIB = _lib()
    B, H, W = mk.shape
    if dl is None:
        dl = torch.full_like(lg, float("nan"))
    gs = _gs(gscale, mk.device)
    LIB.call("uh_surface_loss_grad", lg.data_ptr(), mk.data_ptr(), 2 if ncls == 1 else 1, _ints(classes), len(classes), ncls, B, H, W,
             float(n_mean), float(w), _p(gs), dl.data_ptr(), int(rebuild), ws.data_ptr(), ws.numel(), None)
    return dl


def surface_map(mk, classes, binary):
    _, LIB = _lib()
    B, H, W = mk.shape
    phi = torch.full((len(classes), B, H, W), float("nan"), dtype=torch.float32, device=mk.device)
    ws = surface_ws((B, H, W), len(classes), mk.device)
    LIB.call("uh_surface_dist_map", mk.data_ptr(), 2 if binary else 1, _ints(classes), len(classes), phi.data_ptr(), B, H, W,
             ws.data_ptr(), ws.numel(), None)
    return phi


# ------------------------------------------------------------------------------------------------ the saturated family: exact
@pytest.mark.parametrize("shape", list(K.SHAPES))
def test_saturated_focal_sums_are_exact_and_the_finish_bit_for_bit(shape):
    dev = _dev()
    assert K.sat_conditions()
    for ncls in K.SAT_HEADS[shape]:
        logits, mask, div, w, sums64 = K.sat_focal_case(shape, ncls)
        lg, mk = _up(("satf", shape, ncls), logits, mask)
        C = 2 if ncls == 1 else ncls
        want = torch.tensor(sums64, dtype=torch.float64).float()
        for gamma in K.SAT_GAMMAS if shape in K.SMALL else K.SAT_GAMMAS[2:]:
            sums = focal_sums(lg, mk, div, ncls, w, gamma)
            assert torch.equal(sums.cpu(), want), (ncls, gamma, sums.cpu().tolist(), sums64)
        for (alpha, beta), cls in zip(K.SAT_PRICES, ((1,), tuple(range(1, C)))):
            out = focal_finish(sums, ncls, alpha, beta, cls)
            assert out.tolist() == K.focal_finish64(sums64, C, alpha, beta, cls), (ncls, alpha, beta, out.tolist())
        print(f"{shape} head {ncls}: F {sums64[0]:.0f} W {sums64[1]} of {mask.numel()} pixels, {len(K.special_indices(mask.numel()))} disagree: equal")


@pytest.mark.parametrize("shape", list(K.SHAPES))
def test_saturated_distill_sums_are_exact_and_the_finish_bit_for_bit(shape):
    _dev()
    for ncls in K.SAT_HEADS[shape]:
        z, v, sums64 = K.sat_distill_case(shape, ncls)
        zg, vg = _up(("satd", shape, ncls), z, v)
        n = z.shape[0]
        sums = distill_sums(zg, vg, ncls, K.SAT_T)
        assert sums.cpu().double().tolist() == sums64, (ncls, sums.cpu().tolist(), sums64)
        for world in (1, 2):
            out = distill_finish(sums, n * world, K.SAT_T, 0.75)
            assert out.tolist() == K.distill_finish64(sums64, float(n * world), K.SAT_T, 0.75), (ncls, world, out.tolist())
        if shape != "above_cap":
            # p - q is 0 where the two agree and -+1 on the two classes where they do not: -+ float(w T / n_mean) exactly
            g = distill_grad(zg, vg, ncls, n, K.SAT_T, 0.5, None).cpu()
            want = ((z > 0).double() - (v > 0).double()) * float(np.float32(0.5 * K.SAT_T / n))
            assert torch.equal(g.double(), want), ncls
        print(f"{shape} head {ncls}: sums {sums64} of {n} pixels: equal")


@pytest.mark.parametrize("shape", list(K.SHAPES))
def test_saturated_surface_value_is_exact(shape):
    dev = _dev()
    B, H, W = K.SHAPES[shape]
    n = B * H * W
    for ncls, classes in K.SAT_SURFACE[shape]:
        logits, labels, phi, S = K.sat_surface_case(shape, ncls, classes)
        lg, mk = _up(("sats", shape, ncls, classes), logits, labels)
        ws = surface_ws((B, H, W), len(classes), dev)
        for world in (1, 2):
            out = surface_sums(lg, mk, ncls, classes, n * world, K.SURFACE_W, ws).cpu()
            assert out.tolist() == K.surface_finish64(S, float(n * world), len(classes), K.SURFACE_W), (ncls, classes, out.tolist(), S)
        print(f"{shape} head {ncls} classes {classes}: sum of phi over the sure pixels {S!r}: equal")


# ------------------------------------------------------------------------------------------------ focal + Tversky
@pytest.mark.parametrize("case", K.FOCAL_CASES + K.FOCAL_SUMS_ONLY, ids=_ids)
def test_focal_sums_finish_and_gradient_against_float64(case):
    shape, scale, ncls, gamma = case
    dev = _dev()
    logits, mask, div = K.focal_inputs(shape, scale, ncls)
    ref = K.focal_ref_cached(*case)
    C, w = ref["C"], ref["w"]
    lg, mk = _up(("focal", shape, scale, ncls), logits, mask)
    sums = focal_sums(lg, mk, div, ncls, w, gamma)
    units = K.L.check_sums(sums.cpu(), ref, K.FOCAL_COUNTS(C))
    print(f"{case}: sums worst column {units:.2f} units of 2^-24 S64 beyond its slack (bound {K.L.SUM_ULPS}); W and the counts equal")
    if case in K.FOCAL_SUMS_ONLY:
        return
    handed = _f32(ref["sums"], dev)
    worst = 0.0
    for alpha, beta, cls, gs in K.focal_grad_settings(shape):
        cl = tuple(range(1, C)) if cls is None else cls
        out = focal_finish(handed, ncls, alpha, beta, cl)
        want = K.focal_finish64(handed.cpu().tolist(), C, alpha, beta, cl, rounded=False)
        for got, v in zip(out.tolist(), want):
            assert abs(got - v) <= K.finish_bound(v), (got, v)
        g64, M, slack = K.focal_grad64(ref, alpha, beta, cls, gs)
        g = focal_grad(lg, mk, div, ncls, w, gamma, alpha, beta, cl, handed, gs).cpu()
        got = K.grad_units(g, K.pick(g64, ncls), K.pick(M, ncls), K.pick(slack, ncls), gs)
        worst = max(worst, got)
        assert got <= K.K_FOCAL_GRAD, (alpha, beta, cls, gs, got)
    print(f"{case}: worst gradient element {worst:.2f} units of 2^-24 M |gscale| (bound {K.K_FOCAL_GRAD}, the restatement's {K.R_FOCAL_GRAD})")


# ------------------------------------------------------------------------------------------------ distillation
@pytest.mark.parametrize("case", K.DISTILL_CASES + K.DISTILL_SUMS_ONLY, ids=_ids)
def test_distill_sums_finish_and_gradient_against_float64(case):
    shape, scale, ncls, teacher = case
    dev = _dev()
    z, v = K.distill_inputs(*case)
    ref = K.distill_ref_cached(*case)
    n, T = ref["n"], ref["T"]
    zg, vg = _up(("kd",) + case, z, v)
    sums = distill_sums(zg, vg, ncls, T).cpu()
    assert float(sums[1]) == ref["sums"][1]
    units = K.kd_sum_units(sums[0], ref)
    print(f"{case}: kd sum {float(sums[0]):.9g} (float64 {ref['sums'][0]:.9g}): {units:.2f} units of 2^-24 A (bound {K.K_KD_SUM}, the "
          f"restatement's {K.R_KD_SUM}); agree equal")
    assert abs(float(sums[0]) - ref["sums"][0]) <= K.kd_sum_bound(ref, K.K_KD_SUM)
    if case in K.DISTILL_SUMS_ONLY:
        return
    handed = _f32(ref["sums"], dev)
    worst = 0.0
    for world, gs in K.distill_grad_settings(shape):
        out = distill_finish(handed, n * world, T, K.KD_W)
        for got, want in zip(out.tolist(), K.distill_finish64(handed.cpu().tolist(), float(n * world), T, K.KD_W, rounded=False)):
            assert abs(got - want) <= K.finish_bound(want, 0.0), (got, want)
        g64, M, slack = K.distill_grad64(ref, float(n * world), K.KD_W, gs)
        g = distill_grad(zg, vg, ncls, n * world, T, K.KD_W, gs).cpu()
        got = K.grad_units(g, K.pick(g64, ncls), K.pick(M, ncls), K.pick(slack, ncls), gs)
        worst = max(worst, got)
        assert got <= K.K_DISTILL_GRAD, (world, gs, got)
    print(f"{case}: worst gradient element {worst:.2f} units of 2^-24 M |gscale| (bound {K.K_DISTILL_GRAD}, the restatement's {K.R_DISTILL_GRAD})")


# ------------------------------------------------------------------------------------------------ surface
@pytest.mark.parametrize("case", K.SURFACE_CASES + K.SURFACE_SUMS_ONLY, ids=_ids)
def test_surface_value_and_gradient_against_float64(case):
    shape, scale, ncls, classes = case
    dev = _dev()
    B, H, W = K.SHAPES[shape]
    ref = K.surface_ref_cached(*case)
    n = ref["n"]
    lg, mk = _up(("sl", shape, scale, ncls), K.surface_inputs(shape, scale, ncls), K.surface_labels(shape, ncls == 1))
    ws = surface_ws((B, H, W), len(classes), dev)
    out = surface_sums(lg, mk, ncls, classes, n, K.SURFACE_W, ws).cpu()
    v = float(out[0])
    units = K.surface_value_units(v, ref, float(n))
    print(f"{case}: value {v:.9g} (float64 {K.surface_value64(ref, float(n)):.9g}): {units:.2f} units of 2^-24 sum |p phi| beyond the slack "
          f"(bound {K.K_SURFACE_VALUE}, the restatement's {K.R_SURFACE_VALUE})")
    assert abs(v - K.surface_value64(ref, float(n))) <= K.surface_value_bound(ref, float(n), K.K_SURFACE_VALUE)
    assert float(out[1]) == float(np.float32(K.SURFACE_W) * np.float32(v))
    if case in K.SURFACE_SUMS_ONLY:
        return
    R, K2 = K.surface_grad_r(ncls)
    worst = 0.0
    for i, (world, gs) in enumerate(K.surface_grad_settings(shape)):
        g64, M, slack = K.surface_grad64(ref, float(n * world), K.SURFACE_W, gs)
        kept = surface_grad(lg, mk, ncls, classes, n * world, K.SURFACE_W, gs, ws, rebuild=0)       # the distances of the value pass
        got = K.grad_units(kept.cpu(), g64, M, slack, gs)
        worst = max(worst, got)
        assert got <= K2, (world, gs, got)
        if i == 0:                                                                                 # ... and formed again, in a fresh workspace
            again = surface_grad(lg, mk, ncls, classes, n * world, K.SURFACE_W, gs, surface_ws((B, H, W), len(classes), dev, fill=0xA5), rebuild=1)
            assert torch.equal(_bits(again), _bits(kept))
    print(f"{case}: worst gradient element {worst:.2f} units of 2^-24 M |gscale| (bound {K2}, the restatement's {R})")


@pytest.mark.parametrize("binary,classes", [(False, (2,)), (False, (1, 2)), (True, (1,))], ids=["c2", "c12", "binary"])
def test_distance_maps_at_grid_wrap_bit_for_bit(binary, classes):
    """sl_map_kernel's grid goes round past 1 048 576 pixels; a border pixel is -0.0, so the comparison is of bits."""
    _dev()
    (mk,) = _up(("labels", "grid_wrap"), K.surface_labels("grid_wrap", binary))
    want = K.surface_phi("grid_wrap", classes, binary)
    got = surface_map(mk, classes, binary).cpu().numpy()
    assert got.shape == want.shape and np.array_equal(got.view(np.int32), want.view(np.int32))
    assert int((want.view(np.int32) == np.int32(-2 ** 31)).sum()) > 100                            # -0.0 on the borders


@pytest.mark.parametrize("ncls,classes", [(4, (1, 2, 3)), (8, (2,)), (8, (1, 2))], ids=_ids)
def test_surface_rows_off_the_16_byte_grid_give_the_aligned_bits(ncls, classes):
    """NC = 4 and 8 move a pixel's row as 16-byte vectors where logits and dlogits are 16-byte aligned and as dwords otherwise:
    one float off the grid (a slice of a larger buffer) gives the same bits, and the floats around the output slice stay."""
    dev = _dev()
    shape = "two_blocks"
    B, H, W = K.SHAPES[shape]
    n = B * H * W
    logits = K.surface_inputs(shape, 10.0, ncls)
    (mk,) = _up(("labels", shape), K.surface_labels(shape, False))
    m = n * ncls
    buf = torch.zeros(m + 8, dtype=torch.float32, device=dev)
    results = []
    for off, oo in ((4, 4), (1, 1), (4, 1), (3, 2)):          # aligned; both one float off; the output alone; both off, differently
        src = buf[off:off + m]
        src.copy_(logits.reshape(-1).to(dev))
        assert (src.data_ptr() % 16 == 0) == (off == 4)
        ws = surface_ws((B, H, W), len(classes), dev)
        value = surface_sums(src, mk, ncls, classes, n, K.SURFACE_W, ws)
        outbuf = torch.full((m + 8,), 12345.0, dtype=torch.float32, device=dev)
        surface_grad(src, mk, ncls, classes, n, K.SURFACE_W, 0.5, ws, rebuild=0, dl=outbuf[oo:oo + m])
        guard = torch.cat([outbuf[:oo], outbuf[oo + m:]]).cpu()
        assert bool((guard == 12345.0).all()), (off, guard.tolist())
        results.append((_bits(value).cpu(), _bits(outbuf[oo:oo + m]).cpu()))
    assert bool(torch.isfinite(results[0][1].view(torch.float32)).all()) and float(results[0][1].view(torch.float32).abs().max()) > 0
    for v, g in results[1:]:
        assert torch.equal(v, results[0][0]) and torch.equal(g, results[0][1])
    ref = K.surface_ref_cached(shape, 10.0, ncls, classes)
    g64, M, slack = K.surface_grad64(ref, float(n), K.SURFACE_W, 0.5)
    units = K.grad_units(results[1][1].view(torch.float32).reshape(n, ncls), g64, M, slack, 0.5)
    print(f"head {ncls} classes {classes}: the dword path's worst gradient element {units:.2f} units (bound {K.K_SURFACE_GRAD})")
    assert units <= K.K_SURFACE_GRAD


# ------------------------------------------------------------------------------------------------ same bits, half batches
def test_two_calls_give_the_same_bits_and_half_batches_the_whole_gradient_at_second_sweep():
    """What a data-parallel rank computes: its own half of the pixels with the sums (focal), the pixel count (distillation) or
    the mean's pixel count (surface: the maps are per image) of the whole batch."""
    dev = _dev()
    shape = "second_sweep"
    B, H, W = K.SHAPES[shape]
    n = B * H * W
    h = n // 2
    # focal
    case = (shape, 10.0, 3, 2.0)
    logits, mask, div = K.focal_inputs(*case[:3])
    ref = K.focal_ref_cached(*case)
    lg, mk = _up(("focal",) + case[:3], logits, mask)
    sums = focal_sums(lg, mk, div, 3, ref["w"], 2.0)
    assert torch.equal(_bits(sums), _bits(focal_sums(lg, mk, div, 3, ref["w"], 2.0)))
    run = lambda a, b: focal_grad(lg[a:b], mk[a:b], div, 3, ref["w"], 2.0, 0.3, 0.7, (1, 2), sums, 0.5)      # noqa: E731
    whole = run(0, n)
    assert float(whole.abs().max()) > 0 and torch.equal(_bits(whole), _bits(run(0, n)))
    assert torch.equal(_bits(torch.cat([run(0, h), run(h, n)])), _bits(whole))
    # distillation
    case = (shape, 10.0, 3, "free")
    zg, vg = _up(("kd",) + case, *K.distill_inputs(*case))
    T = K.KD_T[3]
    assert torch.equal(_bits(distill_sums(zg, vg, 3, T)), _bits(distill_sums(zg, vg, 3, T)))
    run = lambda a, b: distill_grad(zg[a:b], vg[a:b], 3, n, T, K.KD_W, 0.5)                                  # noqa: E731
    whole = run(0, n)
    assert float(whole.abs().max()) > 0 and torch.equal(_bits(whole), _bits(run(0, n)))
    assert torch.equal(_bits(torch.cat([run(0, h), run(h, n)])), _bits(whole))
    # surface
    for ncls, classes, scale in ((3, (2,), 10.0), (1, (1,), 1.0)):
        lg, mk = _up(("sl", shape, scale, ncls), K.surface_inputs(shape, scale, ncls), K.surface_labels(shape, ncls == 1))
        ws = surface_ws((B, H, W), 1, dev)
        value = surface_sums(lg, mk, ncls, classes, n, K.SURFACE_W, ws)
        whole = surface_grad(lg, mk, ncls, classes, n, K.SURFACE_W, 0.5, ws, rebuild=0)
        assert torch.equal(_bits(value), _bits(surface_sums(lg, mk, ncls, classes, n, K.SURFACE_W, ws)))
        assert float(whole.abs().max()) > 0
        assert torch.equal(_bits(whole), _bits(surface_grad(lg, mk, ncls, classes, n, K.SURFACE_W, 0.5, ws, rebuild=1)))
        hw = surface_ws((1, H, W), 1, dev)
        halves = [surface_grad(lg[a:b], mk[i:i + 1], ncls, classes, n, K.SURFACE_W, 0.5, hw, rebuild=1) for i, (a, b) in enumerate(((0, h), (h, n)))]
        assert torch.equal(_bits(torch.cat(halves)), _bits(whole))


# ------------------------------------------------------------------------------------------------ the autograd nodes
def test_focal_tversky_loss_fn_against_float64():
    losses, _ = _lib()
    dev = _dev()
    case = ("two_blocks", 10.0, 3, 1.5)
    B, H, W = K.SHAPES[case[0]]
    logits, mask, div = K.focal_inputs(*case[:3])
    ref = K.focal_ref_cached(*case)
    lg = logits.reshape(B, H, W, 3).to(dev).requires_grad_()
    total, focal, tversky = losses.FocalTverskyLossFn.apply(lg, mask.reshape(B, H, W).to(dev), div, ref["w"], 1.5, 0.3, 0.7, (1, 2))
    total.backward()
    want = K.focal_finish64(ref["sums"], 3, 0.3, 0.7, (1, 2), rounded=False)
    # the node's own sums: F within 24 u and its slack of F64, relative to W exactly; each Tversky index moves by at most the
    # relative error of TP and P (24 u and the slack, twice)
    rel = [K.L.sums_bound(s, ref["n"], sl) / abs(s) if s > 0 else 0.0 for s, sl in zip(ref["sums"], ref["slack"])]
    b_focal = want[1] * rel[0] + K.finish_bound(want[1])
    b_tv = 2 * max(rel[2:2 + 6]) + K.finish_bound(want[2])
    total, focal, tversky = (t.detach() for t in (total, focal, tversky))
    errs = [abs(float(a) - b) for a, b in zip((total, focal, tversky), want)]
    print(f"total {float(total):.9g} focal {float(focal):.9g} tversky {float(tversky):.9g}: off by {errs} (bounds {b_focal + b_tv:.3e} {b_focal:.3e} {b_tv:.3e})")
    assert errs[1] <= b_focal and errs[2] <= b_tv and errs[0] <= b_focal + b_tv + K.ulp32(want[0])
    g64, M, slack = K.focal_grad64(ref, 0.3, 0.7, (1, 2), None)
    units = K.grad_units(lg.grad.reshape(-1, 3).cpu(), g64, M, slack, None)
    print(f"worst gradient element {units:.2f} units of 2^-24 M (bound {K.K_FOCAL_GRAD})")
    assert units <= K.K_FOCAL_GRAD


def test_distill_loss_fn_against_float64():
    losses, _ = _lib()
    dev = _dev()
    case = ("two_blocks", 10.0, 3, "free")
    B, H, W = K.SHAPES[case[0]]
    z, v = K.distill_inputs(*case)
    ref = K.distill_ref_cached(*case)
    n, T = ref["n"], ref["T"]
    zg = z.reshape(B, H, W, 3).to(dev).requires_grad_()
    weighted, kd, agree = losses.DistillLossFn.apply(zg, v.reshape(B, H, W, 3).to(dev), T, K.KD_W)
    weighted.backward()
    weighted, kd, agree = (t.detach() for t in (weighted, kd, agree))
    want = K.distill_finish64(ref["sums"], float(n), T, K.KD_W, rounded=False)
    bound = T * T / n * K.kd_sum_bound(ref, K.K_KD_SUM)
    print(f"w kd {float(weighted):.9g} kd {float(kd):.9g} agree {float(agree):.9g}; kd off by {abs(float(kd) - want[1]):.3e} (bound {bound:.3e})")
    assert abs(float(kd) - want[1]) <= bound + K.finish_bound(want[1], 0.0)
    assert abs(float(weighted) - want[0]) <= K.KD_W * bound + K.finish_bound(want[0], 0.0)
    assert abs(float(agree) - want[2]) <= K.finish_bound(want[2], 0.0)
    g64, M, slack = K.distill_grad64(ref, float(n), K.KD_W, None)
    units = K.grad_units(zg.grad.reshape(-1, 3).cpu(), g64, M, slack, None)
    print(f"worst gradient element {units:.2f} units of 2^-24 M (bound {K.K_DISTILL_GRAD})")
    assert units <= K.K_DISTILL_GRAD


@pytest.mark.parametrize("ncls,classes", [(1, (1,)), (3, (1, 2))], ids=_ids)
def test_surface_loss_fn_against_float64(ncls, classes):
    losses, _ = _lib()
    dev = _dev()
    shape = "two_blocks"
    B, H, W = K.SHAPES[shape]
    ref = K.surface_ref_cached(shape, 10.0, ncls, classes)
    n = ref["n"]
    logits = K.surface_inputs(shape, 10.0, ncls)
    lg = (logits.reshape(B, H, W) if ncls == 1 else logits.reshape(B, H, W, ncls)).to(dev).requires_grad_()
    labels = torch.from_numpy(K.surface_labels(shape, ncls == 1)).to(dev)
    weighted, value = losses.SurfaceLossFn.apply(lg, labels, 2 if ncls == 1 else 1, classes, K.SURFACE_W)
    weighted.backward()
    weighted, value = weighted.detach(), value.detach()
    err = abs(float(value) - K.surface_value64(ref, float(n)))
    print(f"value {float(value):.9g}, off by {err:.3e} (bound {K.surface_value_bound(ref, float(n), K.K_SURFACE_VALUE):.3e})")
    assert err <= K.surface_value_bound(ref, float(n), K.K_SURFACE_VALUE)
    assert float(weighted) == float(np.float32(K.SURFACE_W) * np.float32(float(value)))
    g64, M, slack = K.surface_grad64(ref, float(n), K.SURFACE_W, None)
    units = K.grad_units(lg.grad.reshape(g64.shape).cpu(), g64, M, slack, None)
    print(f"worst gradient element {units:.2f} units of 2^-24 M (bound {K.surface_grad_r(ncls)[1]})")
    assert units <= K.surface_grad_r(ncls)[1]
