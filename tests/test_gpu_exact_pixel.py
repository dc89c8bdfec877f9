"""Bit-exact GPU tests of the pixel passes and of the recomputed stem, through the C ABI: BatchNorm + ReLU apply / backward
(csrc/bn.hip), the pool and head tails (bn_fused.hip), max-pool (pool_up.hip) and the four uh_stem_* entry points (stem_mfma.hip).

These kernels are per-channel affine maps, masks, 2x2 maxima and sums.  On the "dyadic" family of tests/exact_inputs.py -- small
integers in the tensors, a few bits times a power of two in every per-channel coefficient, the coefficient tuple distinct per
channel -- each has ONE right answer: every product is exact in fp32 and every sum is order-free (the condition is asserted on the
float64 terms where the case is built), element-wise bf16 outputs are one rounding of the exact value.  Every comparison is
E.assert_same or torch.equal against float64 references made with stock torch autograd on the CPU; none has a tolerance, except
the stem's statistics rows, which hold quotients: their bound is derived at test_stem_statistics_rows.
tests/test_exact_inputs_cpu.py shows on the CPU that the conditions hold at every shape used here and that a dropped pixel, a >= in
the ReLU mask, the last maximum for the first, another channel group's coefficients, a missing rounding of the stem's y or dy, or a
result passed through fp16 each change a compared value.

Second half: every pixel pass called with every tensor living as a CHANNEL SLICE of a wider buffer (pixel pitch != channel
count, as ops.py calls them on concat buffers) must equal the dense call value for value, leave the rest of its output buffers
untouched, and take the scalar form where the slice is off the 16-byte grid.  The bilinear pair is not dyadic and gets this check only.

Each case asks uh_pixel_pass_plan for the launch form its calls take and requires the one it was chosen for."""
import contextlib
import ctypes
import os

import pytest
import torch

import exact_inputs as E

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
CAP = 4096
CANARY = 77.0                                   # exact in bf16; no result of a case equals it everywhere


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    return torch.device("cuda:0")


def _name(dtype):
    return "bf16" if dtype == BF16 else "fp32"


def _dt(dtype):
    return 1 if dtype == BF16 else 0


def _vec(dtype):
    return 8 if dtype == BF16 else 4


def _st():
    return torch.cuda.current_stream().cuda_stream


def plan_form(items, C, dtype, aligned=True):
    """The launch form uh_pixel_pass_plan answers: scalar | vector | hoist, + "_capped" where the grid is the cap.  Host only."""
    import unet_amd  # noqa: F401
    from unet_amd._lib import LIB
    out = (ctypes.c_int64 * 3)()
    assert LIB.query("uh_pixel_pass_plan", items, C, _dt(dtype), 1 if aligned else 0, CAP, ctypes.addressof(out)) == 0
    vec, hoist, grid = out
    assert vec in (1, _vec(dtype)) and (vec > 1 or not hoist) and grid <= CAP
    return ("scalar" if vec == 1 else "hoist" if hoist else "vector") + ("_capped" if grid == CAP else "")


# ------------------------------------------------------------------------------------------------ buffers with a pixel pitch
class Layout:
    """Where a [B,H,W,C] tensor lives: channels off .. off + C of a buffer of `total` channels (None: dense).  The rest of the
    buffer holds CANARY."""

    def __init__(self, total=None, off=0):
        self.total, self.off = total, off

    def __repr__(self):
        return "dense" if self.total is None else f"{self.off}of{self.total}"

    def aligned(self, C, dtype):
        total = C if self.total is None else self.total
        return C % _vec(dtype) == 0 and total % _vec(dtype) == 0 and self.off % _vec(dtype) == 0


DENSE = Layout()


class Slot:
    """One tensor of a call: .view [B,H,W,C] (what the kernel reads or writes), .ld its pixel pitch, .ptr."""

    def __init__(self, shape, dtype, dev, lay, src=None):
        B, H, W, C = shape
        total = C if lay.total is None else lay.total
        self.buf = torch.full((B, H, W, total), CANARY, dtype=dtype, device=dev)
        self.view = self.buf[..., lay.off:lay.off + C]
        self.ld, self.C, self.off = total, C, lay.off
        if src is not None:
            self.view.copy_(src)
            assert torch.equal(self.view.float().cpu(), src.float().cpu())            # the values are exact in this dtype
        self.ptr = self.view.data_ptr()
        assert self.ptr == self.buf.data_ptr() + lay.off * self.buf.element_size()

    def result(self):
        """The written channels on the CPU, dense; the other channels must still hold the canary."""
        rest = torch.cat([self.buf[..., :self.off], self.buf[..., self.off + self.C:]], -1)
        assert bool((rest == CANARY).all()), "a pitched call wrote outside its channel slice"
        return self.view.contiguous().cpu()


def _in(t_nchw, dtype, dev, lay):
    return Slot(tuple(E.nhwc(t_nchw).shape), dtype, dev, lay, E.nhwc(t_nchw))


def _out(shape, dtype, dev, lay):
    return Slot(shape, dtype, dev, lay)


def _f32(v, dev):
    return v.float().to(dev).contiguous()


def _coeffs(c, dev):
    return [_f32(v, dev) for v in c.coeffs()]


def _sum_rows(part, nblk, C):
    """Partial rows [nblk][2][C] summed in float64 on the host -> (sum1, sum2): exact integers times the quantum."""
    p = part.cpu().double().view(nblk, 2, C).sum(0)
    return p[0], p[1]


def _exact_only(res, npix):
    """The in-kernel finalize divides by the pixel count: its dy is kept where that is a power of two (1 / n exact), else dropped --
    at the other extents its dgamma and dbeta alone are compared."""
    return res if E.is_pow2(npix) else {k: v for k, v in res.items() if not k.endswith("dy_own")}


def _want(ref_nchw, dtype):
    return E.expected(E.nhwc(ref_nchw), dtype)


# ------------------------------------------------------------------------------------------------ the calls
def run_bn(c, dtype, dev, lay):
    """uh_bn_relu_apply, uh_bn_relu_bwd_reduce, uh_bn_bwd_finalize, uh_bn_relu_bwd_apply in the SyncBN form (ready sums, nblk = 0,
    explicit n_total) and in the in-kernel-finalize form (nblk > 0, n_total = 0), every tensor in layout `lay`."""
    from unet_amd._lib import LIB
    B, H, W, C = c.shape
    n, dt, st = c.npix, _dt(dtype), _st()
    y, dz = _in(c.y, dtype, dev, lay), _in(c.dz, dtype, dev, lay)
    sc, sh, mu, rs = _coeffs(c, dev)
    z, dy, dy_own = (_out((B, H, W, C), dtype, dev, lay) for _ in range(3))
    LIB.call("uh_bn_relu_apply", y.ptr, y.ld, sc.data_ptr(), sh.data_ptr(), z.ptr, z.ld, n, C, dt, st)
    nblk = LIB.query("uh_bn_bwd_nblk", n, C)
    part = torch.full((nblk * 2 * C,), float("nan"), dtype=F32, device=dev)
    LIB.call("uh_bn_relu_bwd_reduce", dz.ptr, dz.ld, y.ptr, y.ld, sc.data_ptr(), sh.data_ptr(), mu.data_ptr(), rs.data_ptr(),
             part.data_ptr(), n, C, dt, st)
    fin_dg, fin_db, own_dg, own_db = (torch.full((C,), float("nan"), dtype=F32, device=dev) for _ in range(4))
    LIB.call("uh_bn_bwd_finalize", part.data_ptr(), nblk, C, fin_dg.data_ptr(), fin_db.data_ptr(), st)
    dg, db = _f32(c.dgamma, dev), _f32(c.dbeta, dev)
    LIB.call("uh_bn_relu_bwd_apply", dz.ptr, dz.ld, y.ptr, y.ld, sc.data_ptr(), sh.data_ptr(), mu.data_ptr(), rs.data_ptr(),
             None, 0, dg.data_ptr(), db.data_ptr(), dy.ptr, dy.ld, n, E.N_TOTAL, C, dt, st)
    LIB.call("uh_bn_relu_bwd_apply", dz.ptr, dz.ld, y.ptr, y.ld, sc.data_ptr(), sh.data_ptr(), mu.data_ptr(), rs.data_ptr(),
             part.data_ptr(), nblk, own_dg.data_ptr(), own_db.data_ptr(), dy_own.ptr, dy_own.ld, n, 0, C, dt, st)
    torch.cuda.synchronize()
    s1, s2 = _sum_rows(part, nblk, C)
    return _exact_only(dict(z=z.result(), sum1=s1, sum2=s2, fin_dgamma=fin_dg.cpu(), fin_dbeta=fin_db.cpu(), own_dgamma=own_dg.cpu(),
                            own_dbeta=own_db.cpu(), dy=dy.result(), dy_own=dy_own.result(), given_unchanged=torch.stack([dg, db]).cpu()), n)


def run_maxpool(c, dtype, dev, lay):
    """uh_maxpool2_fwd and uh_maxpool2_bwd (with and without dskip) on x = the stored z of a PoolTailCase."""
    from unet_amd._lib import LIB
    B, H, W, C = c.shape
    dt, st = _dt(dtype), _st()
    r = c.refs(dtype)
    x, dpool, dskip = _in(r["zq"], dtype, dev, lay), _in(c.dpool, dtype, dev, lay), _in(c.dskip, dtype, dev, lay)
    pooled = _out((B, H // 2, W // 2, C), dtype, dev, lay)
    dx, dx0 = _out((B, H, W, C), dtype, dev, lay), _out((B, H, W, C), dtype, dev, lay)
    LIB.call("uh_maxpool2_fwd", x.ptr, x.ld, pooled.ptr, pooled.ld, B, H, W, C, dt, st)
    LIB.call("uh_maxpool2_bwd", x.ptr, x.ld, dpool.ptr, dpool.ld, dskip.ptr, dskip.ld, dx.ptr, dx.ld, B, H, W, C, dt, st)
    LIB.call("uh_maxpool2_bwd", x.ptr, x.ld, dpool.ptr, dpool.ld, None, 0, dx0.ptr, dx0.ld, B, H, W, C, dt, st)
    torch.cuda.synchronize()
    return dict(pooled=pooled.result(), dx=dx.result(), dx_noskip=dx0.result())


def run_pool_tail(c, dtype, dev, lay):
    """uh_bn_relu_pool_apply, then with and without dskip: uh_bn_relu_pool_bwd_reduce, uh_bn_bwd_finalize and
    uh_bn_relu_pool_bwd_apply in both forms.  A case without sums runs the forward and the SyncBN apply only."""
    from unet_amd._lib import LIB
    B, H, W, C = c.shape
    n, dt, st = c.npix, _dt(dtype), _st()
    assert LIB.query("uh_bn_relu_pool_ok", B, H, W, C, dt) == 1
    y, dpool, dskip = _in(c.y, dtype, dev, lay), _in(c.dpool, dtype, dev, lay), _in(c.dskip, dtype, dev, lay)
    sc, sh, mu, rs = _coeffs(c, dev)
    co = (sc.data_ptr(), sh.data_ptr(), mu.data_ptr(), rs.data_ptr())
    z, pooled = _out((B, H, W, C), dtype, dev, lay), _out((B, H // 2, W // 2, C), dtype, dev, lay)
    LIB.call("uh_bn_relu_pool_apply", y.ptr, y.ld, sc.data_ptr(), sh.data_ptr(), z.ptr, z.ld, pooled.ptr, pooled.ld, B, H, W, C, dt, st)
    res = dict(z=z, pooled=pooled)
    dg, db = _f32(c.dgamma, dev), _f32(c.dbeta, dev)
    nblk = LIB.query("uh_bn_bwd_nblk", n, C)
    for tag, sk in (("skip.", (dskip.ptr, dskip.ld)), ("noskip.", (None, 0))):
        if tag == "noskip." and not c.sums:
            continue
        dy = _out((B, H, W, C), dtype, dev, lay)
        LIB.call("uh_bn_relu_pool_bwd_apply", *sk, dpool.ptr, dpool.ld, y.ptr, y.ld, *co, None, 0, dg.data_ptr(), db.data_ptr(),
                 dy.ptr, dy.ld, B, H, W, E.N_TOTAL, C, dt, st)
        res[tag + "dy"] = dy
        if not c.sums:
            continue
        part = torch.full((nblk * 2 * C,), float("nan"), dtype=F32, device=dev)
        LIB.call("uh_bn_relu_pool_bwd_reduce", *sk, dpool.ptr, dpool.ld, y.ptr, y.ld, *co, part.data_ptr(), B, H, W, C, dt, st)
        fin_dg, fin_db, own_dg, own_db = (torch.full((C,), float("nan"), dtype=F32, device=dev) for _ in range(4))
        LIB.call("uh_bn_bwd_finalize", part.data_ptr(), nblk, C, fin_dg.data_ptr(), fin_db.data_ptr(), st)
        dy_own = _out((B, H, W, C), dtype, dev, lay)
        LIB.call("uh_bn_relu_pool_bwd_apply", *sk, dpool.ptr, dpool.ld, y.ptr, y.ld, *co, part.data_ptr(), nblk, own_dg.data_ptr(),
                 own_db.data_ptr(), dy_own.ptr, dy_own.ld, B, H, W, 0, C, dt, st)
        res.update({tag + "part": part, tag + "fin_dgamma": fin_dg, tag + "fin_dbeta": fin_db, tag + "own_dgamma": own_dg,
                    tag + "own_dbeta": own_db, tag + "dy_own": dy_own})
    torch.cuda.synchronize()
    out = {}
    for k, v in res.items():
        if isinstance(v, Slot):
            out[k] = v.result()
        elif k.endswith("part"):
            out[k[:-4] + "sum1"], out[k[:-4] + "sum2"] = _sum_rows(v, nblk, C)
        else:
            out[k] = v.cpu()
    return _exact_only(out, n)


def run_head(c, dtype, dev, lay):
    """uh_bn_relu_head_fwd, uh_bn_relu_head_bwd_reduce, uh_bn_bwd_finalize, uh_bn_relu_head_bwd_apply in both forms; y and dy in
    layout `lay` (logits and dlogits are dense fp32 by the ABI)."""
    from unet_amd._lib import LIB
    B, H, W, C = c.shape
    n, ncls, dt, st = c.npix, c.ncls, _dt(dtype), _st()
    assert LIB.query("uh_bn_relu_head_ok", C, ncls, dt) == 1
    y = _in(c.y, dtype, dev, lay)
    sc, sh, mu, rs = _coeffs(c, dev)
    co = (sc.data_ptr(), sh.data_ptr(), mu.data_ptr(), rs.data_ptr())
    w, b = _f32(c.head_w.view(ncls, C), dev), _f32(c.head_b, dev)
    dl = E.nhwc(c.dlogits).to(dev).contiguous()
    logits = torch.full((B, H, W, ncls), float("nan"), dtype=F32, device=dev)
    LIB.call("uh_bn_relu_head_fwd", y.ptr, y.ld, sc.data_ptr(), sh.data_ptr(), w.data_ptr(), b.data_ptr(), logits.data_ptr(), n, C, ncls, dt, st)
    nblk = LIB.query("uh_bn_bwd_nblk", n, C)
    wsb = LIB.query("uh_bn_relu_head_bwd_ws_bytes", n, C, ncls)
    ws = torch.empty(wsb // 4 + 1, dtype=F32, device=dev)
    part = torch.full((nblk * 2 * C,), float("nan"), dtype=F32, device=dev)
    dhw, dhb = torch.full((ncls, C), float("nan"), dtype=F32, device=dev), torch.full((ncls,), float("nan"), dtype=F32, device=dev)
    LIB.call("uh_bn_relu_head_bwd_reduce", dl.data_ptr(), w.data_ptr(), y.ptr, y.ld, *co, part.data_ptr(), dhw.data_ptr(), dhb.data_ptr(),
             ws.data_ptr(), wsb, n, C, ncls, dt, st)
    fin_dg, fin_db, own_dg, own_db = (torch.full((C,), float("nan"), dtype=F32, device=dev) for _ in range(4))
    LIB.call("uh_bn_bwd_finalize", part.data_ptr(), nblk, C, fin_dg.data_ptr(), fin_db.data_ptr(), st)
    dg, db = _f32(c.dgamma, dev), _f32(c.dbeta, dev)
    dy, dy_own = _out((B, H, W, C), dtype, dev, lay), _out((B, H, W, C), dtype, dev, lay)
    LIB.call("uh_bn_relu_head_bwd_apply", dl.data_ptr(), w.data_ptr(), y.ptr, y.ld, *co, None, 0, dg.data_ptr(), db.data_ptr(),
             dy.ptr, dy.ld, n, E.N_TOTAL, C, ncls, dt, st)
    LIB.call("uh_bn_relu_head_bwd_apply", dl.data_ptr(), w.data_ptr(), y.ptr, y.ld, *co, part.data_ptr(), nblk, own_dg.data_ptr(),
             own_db.data_ptr(), dy_own.ptr, dy_own.ld, n, 0, C, ncls, dt, st)
    torch.cuda.synchronize()
    s1, s2 = _sum_rows(part, nblk, C)
    return _exact_only(dict(logits=logits.cpu(), sum1=s1, sum2=s2, dhead_w=dhw.cpu(), dhead_b=dhb.cpu(), fin_dgamma=fin_dg.cpu(),
                            fin_dbeta=fin_db.cpu(), own_dgamma=own_dg.cpu(), own_dbeta=own_db.cpu(), dy=dy.result(),
                            dy_own=dy_own.result()), n)


def _check_bn_backward(got, ref, c, dtype, tag=""):
    """The parts every BatchNorm backward shares: summed partial rows, both finalizes, dy in the SyncBN form everywhere and in the
    in-kernel-finalize form where the pixel count is a power of two (1 / n is then exact)."""
    for k in ("sum1", "sum2"):
        E.assert_same(got[tag + k], ref[k], f"{tag}partial rows summed in float64: {k}")
    for own in ("fin_", "own_"):
        E.assert_same(got[tag + own + "dgamma"], ref["sum2"].float(), f"{tag}{own}dgamma")
        E.assert_same(got[tag + own + "dbeta"], ref["sum1"].float(), f"{tag}{own}dbeta")
    E.assert_same(got[tag + "dy"], _want(ref["dy"], dtype), f"{tag}dy, SyncBN form (n_total = {E.N_TOTAL})")
    if ref.get("own_dy") is not None:
        assert E.is_pow2(c.npix)
        E.assert_same(got[tag + "dy_own"], _want(ref["own_dy"], dtype), f"{tag}dy, in-kernel finalize (n = {c.npix})")


# ------------------------------------------------------------------------------------------------ cases
# (B, H, W, C, dtype) -> the launch form at B*H*W items (the pixel walks) and at B*H*W/4 items (the window walks)
FORMS = {
    (2, 6, 10, 3, BF16): ("scalar", "scalar"), (2, 6, 10, 12, BF16): ("scalar", "scalar"), (2, 6, 10, 24, BF16): ("vector", "vector"),
    (2, 6, 10, 64, BF16): ("hoist", "hoist"), (2, 6, 10, 3, F32): ("scalar", "scalar"), (2, 6, 10, 12, F32): ("vector", "vector"),
    (2, 6, 10, 24, F32): ("hoist", "vector"), (2, 6, 10, 64, F32): ("hoist", "hoist"),
    (1, 5, 5, 3, BF16): ("scalar", "scalar"), (1, 5, 5, 3, F32): ("scalar", "scalar"),
    (2, 2, 2, 512, BF16): ("hoist", "hoist"), (2, 2, 2, 512, F32): ("hoist", "hoist"),
    (2, 8, 16, 24, BF16): ("hoist", "vector"), (2, 8, 16, 24, F32): ("hoist", "vector"),         # 256 pixels: 1 / n is exact
    (2, 512, 352, 24, BF16): ("vector_capped", "hoist"), (2, 256, 272, 64, BF16): ("hoist_capped", "hoist"),
    (2, 1024, 704, 24, BF16): ("vector_capped", "vector_capped"),
}
# dz of the case: wide integers, or -- where the sums of a large extent, or a dy built on the case's own sums, need it -- ternary
NARROW = {(2, 8, 16, 24): ("ternary", 0.5), (2, 512, 352, 24): ("ternary", 0.25), (2, 256, 272, 64): ("ternary", 0.25),
          (2, 1024, 704, 24): ("ternary", 0.25)}
ELEMENTWISE_ONLY = {(2, 1024, 704, 24)}         # the pool tail's capped form: its sums would need a far sparser dz than its dy


def _case_args(shape):
    return (*shape, *NARROW.get(shape, ("wide", 1.0)))


def _pool_case(shape):
    return E.pool_tail_case(*_case_args(shape), shape not in ELEMENTWISE_ONLY)


def _params(keep):
    keys = sorted((k for k in FORMS if keep(k)), key=lambda k: (k[:4], k[4] == BF16))
    return [pytest.param(k[:4], k[4], id=f"{'x'.join(map(str, k[:4]))}-{_name(k[4])}") for k in keys]


def _pool_tail_ok(k):
    B, H, W, C, dtype = k
    return H % 2 == 0 and W % 2 == 0 and C % _vec(dtype) == 0


BN_PARAMS = _params(lambda k: k[:4] not in ELEMENTWISE_ONLY)
MAXPOOL_PARAMS = _params(lambda k: k[:4] not in ELEMENTWISE_ONLY and k[0] * k[1] * k[2] < 200000)
POOL_TAIL_PARAMS = _params(_pool_tail_ok)
# the head tail: 8 and 16 lanes per pixel (C = lanes * 16 bytes), 1, 3 and 4 classes; and 256 pixels for the in-kernel finalize
HEAD_CASES = [((2, 6, 10, lpp * _vec(dt)), ncls, dt, "wide") for dt in (F32, BF16) for lpp in (8, 16) for ncls in (1, 3, 4)] + \
             [((2, 8, 16, 8 * _vec(dt)), 3, dt, "ternary") for dt in (F32, BF16)]
HEAD_PARAMS = [pytest.param(shape, ncls, dt, fam, id=f"{'x'.join(map(str, shape))}-ncls{ncls}-{_name(dt)}") for shape, ncls, dt, fam in HEAD_CASES]


def test_the_cases_reach_every_launch_form():
    """scalar, vector, hoist and the two capped forms, asked of uh_pixel_pass_plan for the very extents the tests run."""
    seen = set()
    for (B, H, W, C, dtype), (at_n, at_nw) in FORMS.items():
        n = B * H * W
        assert plan_form(n, C, dtype) == at_n, (B, H, W, C, dtype)
        assert plan_form(max(n // 4, 1), C, dtype) == at_nw, (B, H, W, C, dtype)
        seen |= {at_n, at_nw}
    assert seen == {"scalar", "vector", "hoist", "vector_capped", "hoist_capped"}
    assert {k[:4] for k in FORMS if k[:4] in ELEMENTWISE_ONLY} == ELEMENTWISE_ONLY
    assert any(E.is_pow2(k[0] * k[1] * k[2]) and k[0] * k[1] * k[2] >= 256 for k in FORMS)


# ------------------------------------------------------------------------------------------------ pixel passes, bit for bit
@pytest.mark.parametrize("shape,dtype", BN_PARAMS)
def test_bn_relu_passes_bit_exact(shape, dtype):
    dev = _dev()
    B, H, W, C = shape
    assert plan_form(B * H * W, C, dtype) == FORMS[(*shape, dtype)][0]
    c = E.bn_case(*_case_args(shape))
    got = run_bn(c, dtype, dev, DENSE)
    E.assert_same(got["z"], _want(c.z, dtype), "z")
    _check_bn_backward(got, dict(sum1=c.sum1, sum2=c.sum2, dy=c.dy, own_dy=c.own_dy), c, dtype)
    E.assert_same(got["given_unchanged"], torch.stack([c.dgamma, c.dbeta]).float(), "the SyncBN form must only read dgamma / dbeta")


@pytest.mark.parametrize("shape,dtype", MAXPOOL_PARAMS)
def test_maxpool_bit_exact(shape, dtype):
    """Forward, and backward to the FIRST maximum with and without a skip gradient; odd extents included."""
    dev = _dev()
    B, H, W, C = shape
    f_n, f_nw = FORMS[(*shape, dtype)]
    assert plan_form(B * H * W, C, dtype) == f_n and plan_form(max(B * H * W // 4, 1), C, dtype) == f_nw
    c = _pool_case(shape)
    got, r, r0 = run_maxpool(c, dtype, dev, DENSE), c.refs(dtype, True), c.refs(dtype, False)
    E.assert_same(got["pooled"], _want(r["pooled"], dtype), "pooled")
    E.assert_same(got["dx"], _want(r["dz"], dtype), "dx = dskip + route(dy)")
    E.assert_same(got["dx_noskip"], _want(r0["dz"], dtype), "dx = route(dy)")


@pytest.mark.parametrize("shape,dtype", POOL_TAIL_PARAMS)
def test_pool_tail_bit_exact(shape, dtype):
    dev = _dev()
    B, H, W, C = shape
    assert plan_form(B * H * W // 4, C, dtype) == FORMS[(*shape, dtype)][1]
    sums = shape not in ELEMENTWISE_ONLY
    c = _pool_case(shape)
    got = run_pool_tail(c, dtype, dev, DENSE)
    r = c.refs(dtype, True)
    E.assert_same(got["z"], _want(c.z, dtype), "z")
    E.assert_same(got["pooled"], _want(r["pooled"], dtype), "pooled")
    if not sums:
        E.assert_same(got["skip.dy"], _want(r["dy"], dtype), "dy, SyncBN form")
        return
    for tag, skip in (("skip.", True), ("noskip.", False)):
        _check_bn_backward(got, c.refs(dtype, skip), c, dtype, tag)


@pytest.mark.parametrize("shape,ncls,dtype,w_family", HEAD_PARAMS)
def test_head_tail_bit_exact(shape, ncls, dtype, w_family):
    dev = _dev()
    c = E.head_tail_case(*shape, ncls, w_family)
    got, r = run_head(c, dtype, dev, DENSE), c.refs(dtype)
    E.assert_same(got["logits"], E.nhwc(r["logits"]).float(), "logits")
    E.assert_same(got["dhead_w"], r["dhead_w"].float(), "dhead_w")
    E.assert_same(got["dhead_b"], r["dhead_b"].float(), "dhead_b")
    _check_bn_backward(got, r, c, dtype)


# ------------------------------------------------------------------------------------------------ pitched calls equal dense calls
def _layouts(C, dtype):
    lays = [Layout(2 * C, 0), Layout(2 * C, C)]
    if C == 24 and dtype == BF16:
        lays.append(Layout(36, 12))             # 24 bytes into a pixel: no 16-byte pieces
    if C == 3:
        lays.append(Layout(5, 0))
    return lays


PITCH_CASES = [((2, 6, 10, C), dt) for dt in (F32, BF16) for C in (3, 12, 24, 64)] + [((2, 256, 272, 64), BF16)]
PITCH_PARAMS = [pytest.param(shape, dt, id=f"{'x'.join(map(str, shape))}-{_name(dt)}") for shape, dt in PITCH_CASES]


def _same_results(a, b, what):
    assert sorted(a) == sorted(b)
    for k in sorted(a):
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), f"{what}: {k} differs from the dense call: {E.mismatches(a[k], b[k])}"


def _pitched_form(shape, dtype, lay, items):
    C = shape[3]
    form = plan_form(items, C, dtype, lay.aligned(C, dtype))
    if not lay.aligned(C, dtype):
        assert form.startswith("scalar"), (shape, dtype, lay, form)
    return form


@pytest.mark.parametrize("shape,dtype", PITCH_PARAMS)
def test_pitched_bn_and_pool_calls_equal_dense_calls(shape, dtype):
    """BatchNorm apply / backward, max-pool and (where the shape has one) the pool tail.  The exact family: reduced outputs must be
    equal too, whatever launch form the pitch selects."""
    dev = _dev()
    B, H, W, C = shape
    cb, cp = E.bn_case(*_case_args(shape)), _pool_case(shape)
    dense_bn, dense_mp = run_bn(cb, dtype, dev, DENSE), run_maxpool(cp, dtype, dev, DENSE)
    tail = _pool_tail_ok((*shape, dtype))
    dense_pt = run_pool_tail(cp, dtype, dev, DENSE) if tail else None
    forms = set()
    for lay in _layouts(C, dtype):
        forms.add(_pitched_form(shape, dtype, lay, B * H * W))
        _same_results(run_bn(cb, dtype, dev, lay), dense_bn, f"BatchNorm passes, {lay}")
        _same_results(run_maxpool(cp, dtype, dev, lay), dense_mp, f"max-pool, {lay}")
        if tail and lay.aligned(C, dtype):      # (the fused tail exists in 16-byte pieces only)
            _same_results(run_pool_tail(cp, dtype, dev, lay), dense_pt, f"pool tail, {lay}")
    if C == 24 and dtype == BF16:
        assert forms == {"vector", "scalar"}
    if shape == (2, 256, 272, 64):
        assert forms == {"hoist_capped"}


PITCH_HEAD_CASES = [((2, 6, 10, 8 * _vec(dt)), 3, dt, "wide") for dt in (F32, BF16)] + [((2, 256, 272, 64), 4, BF16, "ternary")]


@pytest.mark.parametrize("shape,ncls,dtype,w_family", [pytest.param(*v, id=f"{'x'.join(map(str, v[0]))}-ncls{v[1]}-{_name(v[2])}") for v in PITCH_HEAD_CASES])
def test_pitched_head_tail_calls_equal_dense_calls(shape, ncls, dtype, w_family):
    dev = _dev()
    C = shape[3]
    c = E.head_tail_case(*shape, ncls, w_family)
    dense = run_head(c, dtype, dev, DENSE)
    for lay in (Layout(2 * C, 0), Layout(2 * C, C)):
        _same_results(run_head(c, dtype, dev, lay), dense, f"head tail, {lay}")


@contextlib.contextmanager
def _env(key, value):
    before = os.environ.get(key)
    os.environ[key] = value
    try:
        yield
    finally:
        if before is None:
            os.environ.pop(key, None)
        else:
            os.environ[key] = before


def run_upsample(shape, dtype, dev, lay, seed):
    """uh_upsample2x_fwd, uh_upsample2x_bwd in both of its strip forms, and uh_bn_relu_upsample2x_fwd where the layout allows it,
    into (2H + 1) x (2W + 1) with one padding row on top and one padding column on the right.  Seeded, not dyadic."""
    from unet_amd._lib import LIB
    B, H, W, C = shape
    dt, st = _dt(dtype), _st()
    Ho, Wo, pt, pl = 2 * H + 1, 2 * W + 1, 1, 0
    g = torch.Generator().manual_seed(seed)
    x = Slot(shape, dtype, dev, lay, torch.randn(shape, generator=g).to(dtype))
    dup = Slot((B, Ho, Wo, C), dtype, dev, lay, torch.randn(B, Ho, Wo, C, generator=g).to(dtype))
    sc, sh = (torch.rand(C, generator=g) + 0.5).to(dev), (torch.randn(C, generator=g) * 0.3).to(dev)
    up, dx, dx_ptr = _out((B, Ho, Wo, C), dtype, dev, lay), _out(shape, dtype, dev, lay), _out(shape, dtype, dev, lay)
    LIB.call("uh_upsample2x_fwd", x.ptr, x.ld, up.ptr, up.ld, B, H, W, C, Ho, Wo, pt, pl, dt, st)
    LIB.call("uh_upsample2x_bwd", dup.ptr, dup.ld, dx.ptr, dx.ld, B, H, W, C, Ho, Wo, pt, pl, dt, st)
    with _env("UH_UP_BWD_PTR", "1"):
        LIB.call("uh_upsample2x_bwd", dup.ptr, dup.ld, dx_ptr.ptr, dx_ptr.ld, B, H, W, C, Ho, Wo, pt, pl, dt, st)
    res = dict(up=up, dx=dx, dx_ptr=dx_ptr)
    if lay.aligned(C, dtype) and LIB.query("uh_bn_relu_upsample2x_ok", B, H, W, C, Ho, Wo, dt) == 1:
        bn_up = _out((B, Ho, Wo, C), dtype, dev, lay)
        LIB.call("uh_bn_relu_upsample2x_fwd", x.ptr, x.ld, sc.data_ptr(), sh.data_ptr(), bn_up.ptr, bn_up.ld, B, H, W, C, Ho, Wo, pt, pl, dt, st)
        res["bn_up"] = bn_up
    torch.cuda.synchronize()
    return {k: v.result() for k, v in res.items()}


UP_PITCH_PARAMS = [pytest.param(shape, dt, lay, id=f"{'x'.join(map(str, shape))}-{_name(dt)}-{lay}")
                   for shape, dt in PITCH_CASES for lay in _layouts(shape[3], dt)]


@pytest.mark.parametrize("shape,dtype,lay", UP_PITCH_PARAMS)
def test_pitched_upsample_calls_equal_dense_calls(shape, dtype, lay):
    """uh_upsample2x_fwd, uh_upsample2x_bwd (both UH_UP_BWD_PTR forms) and uh_bn_relu_upsample2x_fwd on channel slices against the
    dense calls.

    [2x6x10x24-bf16-12of36] is the one id where the pitched and the dense call run DIFFERENT kernels: the slice is off the 16-byte
    grid, so it takes the one-channel forms where the dense call takes the 16-byte forms (every other id compares a kernel with
    itself at another pitch).  It found the two forms rounding differently, by one bf16 ulp on 3 of 13 104 values of `up` and 2 of
    2 880 of `dx`: the one-channel forward kernel left the contraction of its weights and blends to the compiler, and the one-channel
    backward was the gather kernel, which adds (wy * wx) * dy where the strip kernel adds wy * (sum over columns of wx * dy).  The
    one-channel forms now use the arithmetic of the 16-byte forms (csrc/pool_up.hip)."""
    dev = _dev()
    C = shape[3]
    dense = run_upsample(shape, dtype, dev, DENSE, 5 + C)
    assert bool((dense["up"] != 0).any()) and ("bn_up" in dense) == (C % _vec(dtype) == 0)
    got = run_upsample(shape, dtype, dev, lay, 5 + C)
    assert ("bn_up" in got) == lay.aligned(C, dtype)
    differ = {k: E.mismatches(got[k], dense[k]) for k in sorted(got) if not torch.equal(got[k], dense[k])}
    assert not differ, f"bilinear x2, {lay}: " + "; ".join(f"{k}: {v}" for k, v in differ.items())


# ------------------------------------------------------------------------------------------------ the recomputed stem
# (B, H, W): one full tile; partial tiles on both edges with a 1-pixel-wide tile column (pivot at (8, 8)); a first tile of fewer
# than 9 rows (pivot at (0, 0)); 33 x 33 = 1089 tiles on 1024 workgroups: workgroups 0 .. 64 take a second tile (the persistent
# loop, the halo prefetch, have_pivot in the statistics, the zeroed tail of the counts), 1-pixel tiles on both far edges
STEM_SHAPES = [(1, 16, 16), (3, 19, 33), (2, 7, 40), (1, 513, 513)]
STEM_PARAMS = [pytest.param(s, fam, id=f"{'x'.join(map(str, s))}-{fam}") for s in STEM_SHAPES for fam in ("ternary", "wide")]
TILE = 16


def _tiles(B, H, W):
    return B * ((H + TILE - 1) // TILE) * ((W + TILE - 1) // TILE)


def _stem_w(c, dev):
    from unet_amd import ops
    wf, _ = ops.pack_w3x3(c.w.to(dev), BF16, False)
    return wf


def run_stem(c, dev, x_lay, zlay):
    """uh_stem_bn_relu_fwd, uh_stem_bn_relu_bwd_reduce + uh_bn_bwd_finalize, uh_stem_bn_relu_bwd_wgrad (given integer dgamma / dbeta,
    n_total a power of two).  x in x_lay (its channel 0 is the image), z and dz in zlay."""
    from unet_amd._lib import LIB
    B, H, W = c.shape
    st, dt, C = _st(), 1, E.STEM_C
    wf = _stem_w(c, dev)
    x, dz = _in(c.x, BF16, dev, x_lay), _in(c.dz, BF16, dev, zlay)
    z = _out((B, H, W, C), BF16, dev, zlay)
    sc, sh, mu, rs = _coeffs(c, dev)
    LIB.call("uh_stem_bn_relu_fwd", x.ptr, 1, x.ld, wf.data_ptr(), sc.data_ptr(), sh.data_ptr(), z.ptr, z.ld, B, H, W, dt, st)
    nblk = LIB.query("uh_stem_nblk", B, H, W)
    part = torch.full((nblk * 2 * C,), float("nan"), dtype=F32, device=dev)
    LIB.call("uh_stem_bn_relu_bwd_reduce", dz.ptr, dz.ld, x.ptr, 1, x.ld, wf.data_ptr(), sc.data_ptr(), sh.data_ptr(), mu.data_ptr(),
             rs.data_ptr(), part.data_ptr(), B, H, W, dt, st)
    fin_dg, fin_db = torch.full((C,), float("nan"), dtype=F32, device=dev), torch.full((C,), float("nan"), dtype=F32, device=dev)
    LIB.call("uh_bn_bwd_finalize", part.data_ptr(), nblk, C, fin_dg.data_ptr(), fin_db.data_ptr(), st)
    wsc, wsh, wmu, wrs = [_f32(v, dev) for v in c.wg_coeffs()]
    dg, db = _f32(c.dgamma, dev), _f32(c.dbeta, dev)
    wsb = LIB.query("uh_stem_bwd_wgrad_ws_bytes", B, H, W, 1)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    dw = torch.full((C * 9,), float("nan"), dtype=F32, device=dev)
    LIB.call("uh_stem_bn_relu_bwd_wgrad", dz.ptr, dz.ld, x.ptr, 1, x.ld, wf.data_ptr(), wsc.data_ptr(), wsh.data_ptr(), wmu.data_ptr(),
             wrs.data_ptr(), dg.data_ptr(), db.data_ptr(), E.N_TOTAL, dw.data_ptr(), ws.data_ptr(), wsb, B, H, W, dt, st)
    torch.cuda.synchronize()
    s1, s2 = _sum_rows(part, nblk, C)
    return dict(z=z.result(), sum1=s1, sum2=s2, fin_dgamma=fin_dg.cpu(), fin_dbeta=fin_db.cpu(), dw=dw.cpu().view(C, 1, 3, 3))


@pytest.mark.parametrize("shape,family", STEM_PARAMS)
def test_stem_bit_exact(shape, family):
    from unet_amd._lib import LIB
    dev = _dev()
    B, H, W = shape
    nblk = LIB.query("uh_stem_nblk", B, H, W)
    if shape == (1, 513, 513):
        assert nblk == 1024 < _tiles(B, H, W) == 1089
    else:
        assert nblk == _tiles(B, H, W)
    c = E.stem_case(*shape, family)
    got = run_stem(c, dev, DENSE, DENSE)
    E.assert_same(got["z"], _want(c.z, BF16), "z")
    E.assert_same(got["sum1"], c.sum1, "partial rows summed in float64: sum m")
    E.assert_same(got["sum2"], c.sum2, "partial rows summed in float64: sum m xhat")
    E.assert_same(got["fin_dgamma"], c.sum2.float(), "dgamma")
    E.assert_same(got["fin_dbeta"], c.sum1.float(), "dbeta")
    E.assert_same(got["dw"], c.dw.float(), "dw (Cout, 1, r, s)")
    if shape == (3, 19, 33):
        # x as channel 0 of a 3-channel image, z and dz as the upper half of a 128-channel buffer (16-byte aligned, as the ABI asks)
        pitched = run_stem(c, dev, Layout(3, 0), Layout(128, 64))
        _same_results(pitched, got, "stem with ldx = 3, ldz = lddz = 128")


@pytest.mark.parametrize("shape,family", STEM_PARAMS)
def test_stem_statistics_rows(shape, family):
    """uh_stem_stats writes per workgroup r a row {mean_r, M2_r} and a pixel count n_r.  The counts are exact.  The rows hold
    quotients, so the merged mean and M2 get a bound, derived from the arithmetic of one row (u = 2^-24, Y = max |y|, p = the
    row's pivot, one of its y; d = y - p, |d| <= 2 Y):
      * s1 = sum d is an exact integer: n_r * 2 Y < 2^24 (asserted).  mean_r = fl(p + fl(s1 / n_r)): two roundings of values of at
        most 2 Y and Y: |error| <= 3 u Y.  The merged mean is a convex combination: the same bound, below the 16 u Y = 2^-20 Y asked.
      * s2 = sum d^2.  Each d^2 is an integer below 2^24 (asserted: (2 Y)^2 < 2^24), so the first add of a lane is exact.  A term
        then passes k - 1 roundings in its lane (k = 4 pixels per lane and tile the workgroup walks), 4 in the 16-lane row sum, 2
        across the waves, and M2_r = fl(s2 - fl(fl(s1 s1) / n_r)) adds 3, each at most u times a partial result <= sum d^2 <=
        n_r (2 Y)^2 (s1^2 / n_r <= sum d^2, Cauchy): |error of M2_r| <= (k + 8) u n_r 4 Y^2.
      * the merge in float64 adds n_r (mean_r - mean)^2: with |mean_r - mean| <= 2 Y and the 3 u Y above, 12 u n_r Y^2 more.
    Summed over the rows: u Y^2 sum_r n_r (4 k_r + 44).  It is asserted to stay below the 2^-18 n Y^2 asked (k = 4 for a row of
    one tile gives 60 u; the 65 two-tile rows of the largest shape have k = 8, 76 u, on an eighth of the pixels), and is far
    below the effect of one dropped pixel, about M2 / n."""
    from unet_amd._lib import LIB
    dev = _dev()
    B, H, W = shape
    c = E.stem_case(*shape, family)
    ntile, nblk, C = _tiles(B, H, W), LIB.query("uh_stem_nblk", B, H, W), E.STEM_C
    assert LIB.query("uh_conv3x3_stat_slabs", B, H, W, 1, C, 1) == ntile
    x = _in(c.x, BF16, dev, DENSE)
    stats = torch.full((ntile * (2 * C + 2),), float("nan"), dtype=F32, device=dev)
    LIB.call("uh_stem_stats", x.ptr, 1, x.ld, _stem_w(c, dev).data_ptr(), stats.data_ptr(), B, H, W, 1, _st())
    torch.cuda.synchronize()
    stats = stats.cpu()
    rows, counts = stats[:ntile * 2 * C].view(ntile, 2, C).double(), stats[ntile * 2 * C:ntile * 2 * C + ntile]
    # the pixel count of every tile, tiles walked in (image, tile row, tile column) order, tile t by workgroup t mod nblk
    ty, tx = (H + TILE - 1) // TILE, (W + TILE - 1) // TILE
    vy = torch.tensor([min(TILE, H - i * TILE) for i in range(ty)])
    vx = torch.tensor([min(TILE, W - i * TILE) for i in range(tx)])
    per_tile = (vy[:, None] * vx[None, :]).flatten().repeat(B).float()
    want_counts, k_lane = torch.zeros(ntile), torch.zeros(ntile)
    for first in range(0, ntile, nblk):
        seg = per_tile[first:first + nblk]
        want_counts[:len(seg)] += seg
        k_lane[:len(seg)] += 4
    assert torch.equal(counts, want_counts), "per-row pixel counts"
    assert float(counts.sum()) == B * H * W and bool((counts[nblk:] == 0).all())
    yq = c.yq                                                          # [B, 64, H, W] float64: what the kernel rounds y to
    Y, n = float(yq.abs().max()), B * H * W
    assert (2 * Y) ** 2 < E.F32_INT and float(counts.max()) * 2 * Y < E.F32_INT
    live = counts > 0
    nr = counts[live].double()[:, None]
    mean_r, m2_r = rows[live, 0], rows[live, 1]
    mean = (nr * mean_r).sum(0) / n
    m2 = m2_r.sum(0) + (nr * (mean_r - mean) ** 2).sum(0)
    u = 2.0 ** -24
    tol_mean = 3 * u * Y
    tol_m2 = u * Y * Y * float((counts[live].double() * (4 * k_lane[live].double() + 44)).sum())
    assert tol_mean <= 2.0 ** -20 * Y and tol_m2 <= 2.0 ** -18 * n * Y * Y
    want_mean = yq.mean((0, 2, 3))
    want_m2 = ((yq - want_mean.view(1, -1, 1, 1)) ** 2).sum((0, 2, 3))
    err_mean, err_m2 = float((mean - want_mean).abs().max()), float((m2 - want_m2).abs().max())
    print(f"stem statistics {shape} {family}: mean error {err_mean:.3e} (bound {tol_mean:.3e}), M2 error {err_m2:.3e} (bound {tol_m2:.3e}), "
          f"M2 / n = {float(want_m2.max()) / n:.3e}")
    assert err_mean <= tol_mean and err_m2 <= tol_m2
