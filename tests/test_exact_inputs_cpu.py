"""CPU proof that tests/test_gpu_exact.py is as sharp as it claims: (a) every input family meets its condition at every shape the GPU
file runs (the case lists are imported from there, the cases are built by the same code, which asserts the conditions); (b) float32
arithmetic gives the float64 reference bit for bit on these families, up to K = 18 432; (c) a pure-torch stand-in for a kernel
(float32 F.conv2d, optionally rounded to bf16) passes the comparator, and the same stand-in with ONE product removed at one output,
with one partial sum rounded to bf16, or with one border pixel's halo taken as non-zero fails it, at the right index."""
import pytest
import torch
import torch.nn.functional as F

import exact_inputs as E
import test_gpu_exact as G

F32, BF16 = torch.float32, torch.bfloat16
SHAPE = (2, 17, 23, 64, 64, 64)              # partial tiles on both edges, two sources; a shape of every GPU group


def _bf16_holds(*ts):
    return all(torch.equal(t.bfloat16().float(), t) for t in ts)


def test_the_cases_cover_every_form_and_every_plan():
    assert {c for _, c32, c16 in G.FWD_CASES for c in (c32, c16) if c is not None} == {0, 1, 2, 3, 4}
    assert {code for code, _, _, _ in G.WGRAD_CASES} == {0, 1, 2, 3, 4, 5, 6}
    assert {(dt, code) for _, dt, code in ((p.values[0], p.values[2], p.values[3]) for p in G.AFFINE_PARAMS)} >= {(BF16, 2), (BF16, 4)}
    assert {mfma for _, mfma in G.CONVT_CASES} == {False, True}


@pytest.mark.parametrize("shape", [s for s, _, _ in G.FWD_CASES], ids=lambda s: "x".join(map(str, s)))
def test_forward_families_meet_their_conditions(shape):
    for fam in G.FAMILIES:
        c = E.Conv3x3Case(shape, fam)         # asserts |reference| <= 256 (ternary) or 225 K < 2^24 (wide) on y and dx
        assert _bf16_holds(c.x, c.w, c.dy)
        lim = E.BF16_INT if fam == "ternary" else E.F32_INT - 1
        assert float(c.y.abs().max()) <= lim and float(c.dx.abs().max()) <= lim
        assert bool((c.y != 0).any()) and bool((c.dx != 0).any())


@pytest.mark.parametrize("code,dtype,shape,fams", G.WGRAD_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_backward_weights_families_meet_their_conditions(code, dtype, shape, fams):
    for fam in fams:
        c = E.WgradCase(shape, fam, G.wgrad_ref_dtype(shape))
        assert _bf16_holds(c.x, c.dy) and bool((c.dw != 0).any())
        if code >= 5:                         # block-scaled fp16 slabs: every subset sum of an element is below 2048
            assert fam == "slab" and c.nnz < 2048 and float(c.x.abs().max()) == 1.0


def test_split_conv_transpose_and_head_families_meet_their_conditions():
    for shape in G.SPLIT_SHAPES:
        for role in E.SPLIT_ROLES:
            c = E.SplitCase(shape, role)      # asserts the non-zero counts along every contraction
            twelve = {"x": c.x, "w": c.w, "dy": c.dy}
            for name, t in twelve.items():
                assert (float(t.abs().max()) > 1.0) == (name == role)
            hi = twelve[role].bfloat16().float()
            assert not torch.equal(hi, twelve[role]) and _bf16_holds(twelve[role] - hi)      # needs a low part, and two parts hold it
    for shape, _ in G.CONVT_CASES:
        for fam in G.FAMILIES:
            c = E.ConvTCase(shape, fam)
            assert _bf16_holds(c.x, c.wt, c.dy, c.bias) and torch.equal(c.bias, c.bias.round())
            if shape[4] > 2 * shape[1]:                             # the padding (bottom row first) holds zeros, not the bias
                assert bool((c.y[:, :, -1] == 0).all()) and bool((c.bias != 0).any())
    for shape in G.CONVT_SPLIT_SHAPES:
        for role in E.SPLIT_ROLES:
            E.ConvTCase(shape, "split_" + role)
    for ncls in (1, 4):
        for fam in G.FAMILIES:
            c = E.OutConvCase(G.OUTCONV_SHAPE, ncls, fam)
            assert _bf16_holds(c.x, c.w, c.dy, c.bias)


@pytest.mark.parametrize("shape", [SHAPE, (1, 16, 16, 1024, 0, 64), (1, 8, 8, 2048, 0, 64)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("family", G.FAMILIES)
def test_float32_equals_float64_on_the_families(family, shape):
    """Up to K = 9 * 2048 = 18 432: the float32 reference IS the float64 one, so either may serve."""
    a, b = E.Conv3x3Case(shape, family, torch.float64), E.Conv3x3Case(shape, family, torch.float32)
    assert torch.equal(a.x, b.x) and torch.equal(a.w, b.w)
    assert torch.equal(a.y.float(), b.y) and torch.equal(a.dx.float(), b.dx)
    assert torch.equal(b.y.double(), a.y) and torch.equal(b.dx.double(), a.dx)


@pytest.mark.parametrize("shape,family", [(SHAPE, "wide"), (SHAPE, "slab"), ((2, 160, 160, 64, 0, 64), "slab")])
def test_float32_equals_float64_for_backward_weights(shape, family):
    a, b = E.WgradCase(shape, family, torch.float64), E.WgradCase(shape, family, torch.float32)
    assert torch.equal(a.dy, b.dy) and torch.equal(b.dw.double(), a.dw)


# ------------------------------------------------------------------------------------------------ the comparator and injected faults
def _standin(x, w, dtype):
    """What a correct kernel computes: float32 accumulation, one rounding when it stores bf16.  NHWC."""
    y = E.nhwc(F.conv2d(x, w, padding=1))
    return y.bfloat16() if dtype == BF16 else y


def _first_nonzero_product(c):
    """(b, o, h, w), (i, r, s) of a product x * w that is not zero, at an interior pixel."""
    b, h, w_, o = 1, 5, 7, 3
    for i in range(c.x.shape[1]):
        for r in range(3):
            for s in range(3):
                if float(c.x[b, i, h + r - 1, w_ + s - 1] * c.w[o, i, r, s]) != 0.0:
                    return (b, o, h, w_), (i, r, s)
    raise AssertionError("no non-zero product")


@pytest.mark.parametrize("dtype", [F32, BF16], ids=G._name)
@pytest.mark.parametrize("family", G.FAMILIES)
def test_the_stand_in_passes(family, dtype):
    c = E.conv3x3_case(SHAPE, family)
    assert E.mismatches(_standin(c.x, c.w, dtype), E.expected(E.nhwc(c.y), dtype)) is None


@pytest.mark.parametrize("family,dtype", [("ternary", F32), ("ternary", BF16), ("wide", F32)])
def test_one_product_removed_at_one_output_fails(family, dtype):
    """Ternary: every non-zero product moves an integer of magnitude <= 256 by one, in fp32 and in bf16.  Wide in fp32 likewise; wide
    in bf16 shows a dropped product only where it crosses a rounding step of the output, so that pair is not claimed."""
    c = E.conv3x3_case(SHAPE, family)
    (b, o, h, w_), (i, r, s) = _first_nonzero_product(c)
    y = F.conv2d(c.x, c.w, padding=1)
    y[b, o, h, w_] -= c.x[b, i, h + r - 1, w_ + s - 1] * c.w[o, i, r, s]
    got = E.nhwc(y).bfloat16() if dtype == BF16 else E.nhwc(y)
    msg = E.mismatches(got, E.expected(E.nhwc(c.y), dtype))
    assert msg is not None and msg.startswith("1 of ") and "(b, h, w, c)" in msg and f"({b}, {h}, {w_}, {o})" in msg, msg
    with pytest.raises(AssertionError, match="1 of "):
        E.assert_same(got, E.expected(E.nhwc(c.y), dtype), "forward")


def test_one_partial_sum_rounded_to_bf16_fails():
    """Wide family: the partial sum over the first source (576 products of variance 80^2: sd 1 920) is rounded to bf16 before the second
    source is added.  In fp32 the result changes wherever that partial sum is no bf16 number: an integer in [256 * 2^k, 512 * 2^k) is
    one with probability 2^-(k+1), which over a normal of that sd leaves 0.11 + 0.10/2 + 0.19/4 + 0.31/8 + 0.25/16 + .. = 0.26
    unchanged -- asserted as "over 70 % change".  A bf16 result changes where the error crosses a rounding step of the output."""
    c = E.conv3x3_case(SHAPE, "wide")
    C0 = SHAPE[3]
    p0 = F.conv2d(c.x[:, :C0], c.w[:, :C0], padding=1)
    p1 = F.conv2d(c.x[:, C0:], c.w[:, C0:], padding=1)
    assert torch.equal((p0 + p1).double(), c.y)
    every = E.nhwc(p0.bfloat16().float() + p1)                          # the fault at EVERY output
    want = E.nhwc(c.y)
    changed32 = every != want.float()
    assert torch.equal(changed32, E.nhwc(p0.bfloat16().float() != p0))
    assert float(changed32.float().mean()) > 0.7
    changed16 = every.bfloat16() != E.to_bf16(want)
    assert bool(changed16.any())
    for dtype, changed in ((F32, changed32), (BF16, changed16)):
        at = tuple(changed.nonzero()[0].tolist())
        got = want.float().clone()
        got[at] = every[at]                                             # the fault at ONE output
        got = got.bfloat16() if dtype == BF16 else got
        msg = E.mismatches(got, E.expected(want, dtype))
        assert msg is not None and msg.startswith("1 of ") and str(at) in msg, msg


@pytest.mark.parametrize("dtype", [F32, BF16], ids=G._name)
@pytest.mark.parametrize("family", G.FAMILIES)
def test_one_border_pixel_with_a_non_zero_halo_fails(family, dtype):
    """The row above the image read as the image's last row (a wrapped halo) at ONE pixel of the top border."""
    c = E.conv3x3_case(SHAPE, family)
    b, w0, H = 0, 9, SHAPE[1]
    extra = torch.einsum("ois,is->o", c.w[:, :, 0, :], c.x[b, :, H - 1, w0 - 1:w0 + 2])
    assert bool((extra != 0).any())
    y = F.conv2d(c.x, c.w, padding=1)
    y[b, :, 0, w0] += extra
    got = E.nhwc(y).bfloat16() if dtype == BF16 else E.nhwc(y)
    msg = E.mismatches(got, E.expected(E.nhwc(c.y), dtype))
    assert msg is not None and f"({b}, 0, {w0}, " in msg, msg
    bad = (got != E.expected(E.nhwc(c.y), dtype)).nonzero()
    assert bool((bad[:, :3] == torch.tensor([b, 0, w0])).all())         # nothing but that pixel
    if family == "ternary" or dtype == F32:
        assert len(bad) == int((extra != 0).sum())                      # every channel whose halo term is non-zero


def test_the_comparator_counts_a_nan_and_refuses_another_dtype():
    a = torch.zeros(1, 2, 2, 4)
    b = a.clone()
    b[0, 1, 0, 2] = float("nan")
    assert E.mismatches(a, a.clone()) is None and E.mismatches(-a, a) is None      # values: -0 == +0
    assert "(0, 1, 0, 2)" in E.mismatches(b, a)
    with pytest.raises(AssertionError):
        E.mismatches(a.bfloat16(), a)


# ================================================================================================ the dyadic family (pixel passes)
# tests/test_gpu_exact_pixel.py: (a) every case class meets its conditions at every shape that file runs (the builders assert them on
# the float64 terms; here they are built, and the inputs are shown to be exact in bf16); (b) float32 sums in two orders give the
# float64 sums; (c) each mutation of the reference a subtly wrong kernel would amount to changes a compared value.
import test_gpu_exact_pixel as P  # noqa: E402

PIXEL_SHAPES = sorted({k[:4] for k in P.FORMS})
SMALL = (2, 6, 10, 24)


def _ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else None


def _dy(m, y, scale, mean, rstd, dgamma, dbeta, n):
    v = E._cv
    return v(scale) * (m - v(dbeta) / n - (y - v(mean)) * v(rstd) * v(dgamma) / n)


def _differs(a, b):
    return E.mismatches(a, b) is not None


@pytest.mark.parametrize("shape", [s for s in PIXEL_SHAPES if s not in P.ELEMENTWISE_ONLY], ids=_ids)
def test_bn_cases_meet_their_conditions(shape):
    c = E.bn_case(*P._case_args(shape))              # asserts: distinct coefficient tuples, order-free sums, every term of dy exact
    assert _bf16_holds(c.y, c.dz, *(v.float() for v in c.coeffs()), c.dgamma.float(), c.dbeta.float())
    assert (c.own_dy is not None) == E.is_pow2(c.npix)
    assert E.N_TOTAL != c.npix and E.is_pow2(E.N_TOTAL)
    for v in (c.z, c.dy, c.sum1, c.sum2):
        assert torch.equal(v.float().double(), v)    # fp32 holds the exact value: bf16 is ONE rounding of it


@pytest.mark.parametrize("shape", PIXEL_SHAPES, ids=_ids)
def test_pool_tail_cases_meet_their_conditions(shape):
    c = P._pool_case(shape)
    assert c.sums == (shape not in P.ELEMENTWISE_ONLY)
    assert _bf16_holds(c.y, c.dskip, c.dpool)
    dtypes = [dt for dt in (F32, BF16) if (*shape, dt) in P.FORMS]
    for dt in dtypes:
        for skip in ((True, False) if c.sums else (True,)):
            r = c.refs(dt, skip)                     # asserts: ties and all-zero windows, |dz| exact in bf16, sums, dy
            assert torch.equal(E.expected(r["dz"], dt).double(), r["dz"])
            assert ("own_dy" in r) == (c.sums and E.is_pow2(c.npix))
            assert torch.equal(r["zq"], c.z)         # z <= 4 * 15 + 4 in quarters: bf16 stores it exactly, the maxima are the same


@pytest.mark.parametrize("shape,ncls,dtype,w_family", P.HEAD_CASES + P.PITCH_HEAD_CASES[-1:], ids=lambda v: _ids(v) if isinstance(v, tuple) else str(v).replace("torch.", ""))
def test_head_tail_cases_meet_their_conditions(shape, ncls, dtype, w_family):
    c = E.head_tail_case(*shape, ncls, w_family)
    assert _bf16_holds(c.y, c.head_w, c.head_b, c.dlogits)
    r = c.refs(dtype)                                # asserts: logits, dhead_w, the sums and dy exact; |dz| exact in bf16
    assert ("own_dy" in r) == E.is_pow2(c.npix)
    assert bool((r["logits"] != 0).any()) and bool((r["dhead_w"] != 0).any())
    assert torch.equal(r["zq"], c.z)                 # (quarters up to 64: the stored activation is exact in bf16 too)


@pytest.mark.parametrize("shape", P.STEM_SHAPES, ids=_ids)
@pytest.mark.parametrize("family", ["ternary", "wide"])
def test_stem_cases_meet_their_conditions(family, shape):
    c = E.stem_case(*shape, family)                  # asserts: y exact, the rounding of y exercised (wide), sums, dy terms, dw budget
    assert _bf16_holds(c.x, c.w, c.dz)
    assert float(c.y.abs().max()) <= (9 if family == "ternary" else 2025)
    assert E.is_pow2(E.N_TOTAL) and torch.equal(c.dgamma, c.dgamma.round()) and torch.equal(c.dbeta, c.dbeta.round())
    if c.npix < 4096:
        assert bool((c.dgamma != 0).any()) and bool((c.dbeta != 0).any())      # the small shapes keep the xhat term of dy
    if family == "wide" and bool((c.dgamma != 0).any()):
        assert _differs(c.dyq, c.dy)                 # ... and the rounding of dy
    assert torch.equal(c.dw.float().double(), c.dw)
    if shape == (1, 513, 513):
        assert P._tiles(*shape) == 1089


def test_float32_sums_in_any_order_equal_the_float64_sums():
    c = E.bn_case(*P._case_args(SMALL))
    xhat = (c.y.double() - E._cv(c.mean)) * E._cv(c.rstd)
    for terms, want in ((c.m, c.sum1), (c.m * xhat, c.sum2)):
        t = terms.float().permute(1, 0, 2, 3).reshape(terms.shape[1], -1)
        fwd, rev = torch.zeros(t.shape[0]), torch.zeros(t.shape[0])
        for i in range(t.shape[1]):                  # serial float32 accumulation, first to last and last to first
            fwd += t[:, i]
            rev += t[:, t.shape[1] - 1 - i]
        assert torch.equal(fwd.double(), want) and torch.equal(rev.double(), want) and torch.equal(t.sum(1).double(), want)


def _mutations(y, dz, coeffs, dgamma, dbeta, n, dtypes):
    """Shared by the four case classes: y, dz float64 NCHW.  Each wrong reference changes a compared value."""
    scale, shift, mean, rstd = coeffs
    z, m = E.relu_and_mask(y, scale, shift, dz)
    xhat = (y - E._cv(mean)) * E._cv(rstd)
    sum1, sum2 = m.sum((0, 2, 3)), (m * xhat).sum((0, 2, 3))
    dy = _dy(m, y, scale, mean, rstd, dgamma, dbeta, n)
    # one pixel dropped from a sum
    at = tuple((m * xhat != 0).nonzero()[0].tolist())
    drop1, drop2 = sum1.clone(), sum2.clone()
    drop1[at[1]] -= m[at]
    drop2[at[1]] -= (m * xhat)[at]
    assert _differs(drop1, sum1) and _differs(drop2, sum2)
    assert _differs(drop1.float(), sum1.float()) and _differs(drop2.float(), sum2.float())          # ... and in the finalized fp32 values
    # >= in place of > in the mask: torch's ReLU passes nothing at z == 0
    t = y * E._cv(scale) + E._cv(shift)
    m_ge = dz * (t >= 0)
    assert bool(((t == 0) & (dz != 0)).any()) and _differs(m_ge, m)
    assert _differs(m_ge.sum((0, 2, 3)), sum1)
    for dt in dtypes:
        assert _differs(E.expected(_dy(m_ge, y, scale, mean, rstd, dgamma, dbeta, n), dt), E.expected(dy, dt))
    # channel c computed with channel c + 8's coefficients (a hoisted coefficient group that is not the thread's own)
    C = y.shape[1]
    roll = (torch.arange(C) + 8) % C
    z_w = torch.relu(y * E._cv(scale[roll]) + E._cv(shift[roll]))
    m_w = E.relu_and_mask(y, scale[roll], shift[roll], dz)[1]
    for dt in dtypes:
        assert _differs(E.expected(z_w, dt), E.expected(z, dt))
        assert _differs(E.expected(_dy(m, y, scale[roll], mean[roll], rstd[roll], dgamma, dbeta, n), dt), E.expected(dy, dt))
    assert _differs(m_w.sum((0, 2, 3)), sum1)
    assert _differs((m * (y - E._cv(mean[roll])) * E._cv(rstd[roll])).sum((0, 2, 3)), sum2)
    # an element-wise result passed through fp16 (11 bits): dy holds 1 / (16 n) steps
    if F32 in dtypes:
        assert _differs(dy.float().half().float(), dy.float())
    return z, m, dy


def test_bn_case_mutations_fail():
    c = E.bn_case(*P._case_args(SMALL))
    z, m, dy = _mutations(c.y.double(), c.dz.double(), c.coeffs(), c.dgamma, c.dbeta, E.N_TOTAL, (F32, BF16))
    assert torch.equal(z, c.z) and torch.equal(m, c.m) and torch.equal(dy, c.dy)
    # the SyncBN form must use n_total, not the pixel count
    assert _differs(E.expected(_dy(m, c.y.double(), c.scale, c.mean, c.rstd, c.dgamma, c.dbeta, c.npix), F32), E.expected(c.dy, F32))


def _one_hot_route(zq, dpool, last):
    """route(dpool) to the first (torch's rule) or to the LAST maximum of each 2x2 window, without autograd."""
    B, C, H, W = zq.shape
    win = F.unfold(zq, 2, stride=2).view(B, C, 4, -1)
    eq = win == win.max(2, keepdim=True).values
    if last:
        eq = eq.flip(2)
    hot = eq & (eq.double().cumsum(2) == 1)
    if last:
        hot = hot.flip(2)
    g = hot.double() * dpool.reshape(B, C, 1, -1)
    out = torch.zeros_like(zq)
    out[:, :, :H // 2 * 2, :W // 2 * 2] = F.fold(g.view(B, C * 4, -1), (H // 2 * 2, W // 2 * 2), 2, stride=2)
    return out


@pytest.mark.parametrize("dtype", [F32, BF16], ids=G._name)
def test_pool_tail_case_mutations_fail(dtype):
    c = P._pool_case(SMALL)
    r = c.refs(dtype, True)
    z, m, dy = _mutations(c.y.double(), r["dz"], c.coeffs(), c.dgamma, c.dbeta, E.N_TOTAL, (dtype,))
    assert torch.equal(m, r["m"]) and torch.equal(dy, r["dy"])
    # the last maximum in place of the first: torch's own routing is the first
    dpool = c.dpool.double()
    assert torch.equal(_one_hot_route(r["zq"], dpool, False), r["route"])
    last = _one_hot_route(r["zq"], dpool, True)
    assert _differs(last, r["route"])
    dz_last = last + c.dskip.double()
    assert _differs(E.expected(dz_last, dtype), E.expected(r["dz"], dtype))                         # uh_maxpool2_bwd's dx
    m_last = E.relu_and_mask(c.y.double(), c.scale, c.shift, dz_last)[1]
    # (tied positive maxima share y, hence the mask and xhat: the per-channel SUMS cannot see which one was taken -- dx and dy do)
    assert not _differs(m_last.sum((0, 2, 3)), r["sum1"])
    assert _differs(E.expected(_dy(m_last, c.y.double(), c.scale, c.mean, c.rstd, c.dgamma, c.dbeta, E.N_TOTAL), dtype), E.expected(r["dy"], dtype))
    # the odd extent of the stand-alone max-pool: the last row and column get the skip gradient only
    odd = P._pool_case((1, 5, 5, 3)).refs(dtype, False)
    assert bool((odd["dz"][:, :, 4] == 0).all()) and bool((odd["dz"][:, :, :, 4] == 0).all()) and bool((odd["dz"] != 0).any())


@pytest.mark.parametrize("dtype", [F32, BF16], ids=G._name)
def test_head_tail_case_mutations_fail(dtype):
    C = 8 * P._vec(dtype)
    c = E.head_tail_case(2, 6, 10, C, 3, "wide")
    r = c.refs(dtype)
    z, m, dy = _mutations(c.y.double(), r["dz"], c.coeffs(), c.dgamma, c.dbeta, E.N_TOTAL, (dtype,))
    assert torch.equal(m, r["m"]) and torch.equal(dy, r["dy"])
    w, dl = c.head_w.double(), c.dlogits.double()
    # one pixel dropped from the head's sums
    at = tuple((r["zq"] != 0).nonzero()[0].tolist())
    dhw = r["dhead_w"].clone()
    dhw[:, at[1]] -= dl[at[0], :, at[2], at[3]] * r["zq"][at]
    assert _differs(dhw.float(), r["dhead_w"].float())
    dhb = r["dhead_b"] - dl[0, :, 0, 0]
    assert _differs(dhb.float(), r["dhead_b"].float())
    # channel c with channel c + 8's coefficients, seen through the logits
    roll = (torch.arange(C) + 8) % C
    z_w = E.expected(torch.relu(c.y.double() * E._cv(c.scale[roll]) + E._cv(c.shift[roll])), dtype).double()
    assert _differs(F.conv2d(z_w, w, c.head_b.double()).float(), r["logits"].float())
    # one product dropped from one logit
    lg = r["logits"].clone()
    lg[at[0], :, at[2], at[3]] -= w[:, at[1], 0, 0] * r["zq"][at]
    assert bool((w[:, at[1], 0, 0] != 0).any()) and _differs(lg.float(), r["logits"].float())


@pytest.mark.parametrize("family", ["ternary", "wide"])
def test_stem_case_mutations_fail(family):
    shape = (2, 7, 40)
    c = E.stem_case(*shape, family)
    assert bool((c.dgamma != 0).any())
    z, m, dy = _mutations(c.yq, c.dz.double(), c.coeffs(), c.dgamma, c.dbeta, E.N_TOTAL, (BF16,))
    assert torch.equal(z, c.z) and torch.equal(m, c.m)
    x = c.x.double()
    # one pixel dropped from the filter gradient
    at = tuple((c.dyq != 0).nonzero()[0].tolist())
    hole = c.dyq.clone()
    hole[at] = 0
    assert _differs(E.stem_dw(hole, x).float(), c.dw.float())
    # >= in the mask and channel c + 8's coefficients, seen through dw
    ws, wsh, wm, wr = c.wg_coeffs()
    t = c.yq * E._cv(ws) + E._cv(wsh)
    m_ge = c.dz.double() * (t >= 0)
    roll = (torch.arange(E.STEM_C) + 8) % E.STEM_C
    mw = E.relu_and_mask(c.yq, ws, wsh, c.dz.double())[1]
    for wrong in (_dy(m_ge, c.yq, ws, wm, wr, c.dgamma, c.dbeta, E.N_TOTAL), _dy(mw, c.yq, ws[roll], wm[roll], wr[roll], c.dgamma, c.dbeta, E.N_TOTAL)):
        assert _differs(E.stem_dw(E.to_bf16(wrong).double(), x).float(), c.dw.float())
    if family == "wide":
        # y not rounded to bf16 before BatchNorm
        z_raw = torch.relu(c.y * E._cv(c.scale) + E._cv(c.shift))
        assert _differs(E.to_bf16(z_raw), E.to_bf16(c.z))
        m_raw = E.relu_and_mask(c.y, c.scale, c.shift, c.dz.double())[1]
        assert _differs((m_raw * (c.y - E._cv(c.mean)) * E._cv(c.rstd)).sum((0, 2, 3)), c.sum2)
        # dy not rounded to bf16 before the contraction
        assert _differs(E.stem_dw(c.dy, x).float(), c.dw.float())
        # dy passed through fp16 on its way to bf16 (a double rounding)
        assert _differs(E.stem_dw(c.dy.float().half().float().bfloat16().double(), x).float(), c.dw.float())


# ================================================================================================ spatial attention
# tests/test_gpu_exact_spatial_attention.py: (a) the launch forms its cases were chosen for are what uh_spatial_attn_plan answers, and
# the query follows the rule restated here; (b) SaFwdCase and SaBwdCase meet their conditions at every shape that file runs; (c)
# float32 sums in a shuffled order give the float64 values; (d) each mutation of the reference changes a compared value.
import test_gpu_exact_spatial_attention as S  # noqa: E402

SA_SHAPES = sorted({(*S.SHAPE, f[1]) for f in S.FORMS} | {(2, *hw, S.GEOMETRY_C) for hw in S.GEOMETRY} | {(*S.SHAPE, S.PITCH_C)})
SA_TWO_STEPS = sorted({(C, V * G) for _, C, form, (V, G, steps) in S.FORMS if steps == 2})      # (C, channels of the first step)


def test_spatial_attention_plan_query_and_the_forms_of_the_cases():
    import ctypes
    import unet_amd  # noqa: F401
    from unet_amd._lib import LIB
    assert len(S.check_forms()) == 12 and SA_TWO_STEPS == [(70, 64), (260, 256), (520, 512)]
    for dt in (F32, BF16):
        vec = 8 if dt == BF16 else 4
        for aligned in (True, False):
            for C in list(range(1, 132)) + [255, 256, 257, 260, 264, 511, 512, 513, 520, 1024, 4100]:
                V = vec if aligned and C % vec == 0 else 1
                nv = -(-C // V)
                G = 1
                while G < nv and G < 64:
                    G *= 2
                assert S.plan(C, dt, aligned) == (V, G, -(-nv // G)), (dt, aligned, C)
    out = (ctypes.c_int64 * 3)()
    assert LIB.query("uh_spatial_attn_plan", 0, 0, 1, ctypes.addressof(out)) < 0
    assert LIB.query("uh_spatial_attn_plan", 8, 7, 1, ctypes.addressof(out)) < 0
    assert LIB.query("uh_spatial_attn_plan", 8, 0, 1, None) < 0


@pytest.mark.parametrize("shape", SA_SHAPES, ids=_ids)
def test_spatial_attention_cases_meet_their_conditions(shape):
    B, H, W, C = shape
    for k in S.KS:
        c = E.sa_fwd_case(*shape, k)                 # asserts: the plants, 90 % of the map unsaturated, the accumulator exact or bounded
        assert _bf16_holds(c.x) and float(c.x.abs().max()) <= E.WIDE_MAX
        taps = c.w * 2.0 ** c.shift
        assert torch.equal(taps, taps.round()) and float(taps.abs().max()) == k * k and len(torch.unique(c.w)) == 2 * k * k
        assert c.exact_acc == E.is_pow2(C) and c.unsaturated >= 0.9 and c.acc_units <= E.SA_ACC_UNITS
        assert torch.equal(torch.max(c.x, dim=1).indices, c.amax) and torch.equal(torch.max(c.x, dim=1).values.double(), c.max)
        if c.exact_acc and c.npix > 100:
            assert float(c.a64.min()) < 0.1 and float(c.a64.max()) > 0.9          # the exact cases walk the sigmoid's range
        for mode in ("gate", "map"):
            b = E.sa_bwd_case(*shape, k, mode)       # asserts: |d| <= 256, g_s exact, g_pool / dw / dx order-free, dx32 == dx64 where C = 2^n
            assert set(b.a.unique().tolist()) <= set(E.SA_A_VALUES) and int(b.amax.max()) == C - 1 and int(b.amax.min()) == 0
            assert _bf16_holds(b.x, b.pool.float()) and (b.dy is None or _bf16_holds(b.dy))
            for v in (b.gs, b.gpool, b.dw):
                assert torch.equal(v.float().double(), v)
            if C > 1 and not E.is_pow2(C) and b.npix > 100:
                assert _differs(b.dx.double(), b.dx64)                             # ... and the roundings are exercised elsewhere


@pytest.mark.parametrize("k", S.KS)
def test_spatial_attention_big_case_reaches_the_second_round(k):
    B, H, W, C = S.BIG
    c = S.big_case(k)
    tile = E.sa_tile_of(B, H, W)
    assert E.sa_tiles(B, H, W) == 1032 == int(tile.max()) + 1 and B * H * W < 150000
    assert bool((c.a == 0.5).all()) and 0.03 < float((c.ga != 0).float().mean()) < 0.1
    for t in range(E.SA_DW_BLOCKS, 1032):
        assert bool((c.gs[tile == t] != 0).any())
    # one tile past the 1024th dropped, and the whole second round dropped
    for keep in (tile != 1030, tile < E.SA_DW_BLOCKS):
        assert _differs(E.sa_dw(c.gs * keep, c.pool, k).float(), c.dw.float())


def _serial32(terms, dim, g):
    """float32 accumulation of `terms` along `dim`, one term at a time, in a seeded shuffled order."""
    t = terms.float().movedim(dim, 0)
    assert torch.equal(t.double(), terms.movedim(dim, 0).double())
    acc = torch.zeros_like(t[0])
    for i in torch.randperm(t.shape[0], generator=g).tolist():
        acc = acc + t[i]
    return acc.double()


@pytest.mark.parametrize("k", S.KS)
def test_spatial_attention_float32_in_a_shuffled_order_equals_float64(k):
    g = torch.Generator().manual_seed(5)
    B, H, W = S.SHAPE
    P = k // 2
    c = E.sa_fwd_case(B, H, W, 260, k)
    assert torch.equal(_serial32(c.x, 1, g), c.x.double().sum(1))
    c = E.sa_fwd_case(B, H, W, 8, k)
    terms = F.unfold(c.pool, k, padding=P) * c.w.view(1, -1, 1)                     # [B, 2 k^2, H W]
    assert torch.equal(_serial32(terms, 1, g).view(B, H, W), E.sa_logits(c.pool, c.w))
    b = E.sa_bwd_case(B, H, W, 260, k, "gate")
    assert torch.equal(_serial32(b.x.double() * b.dy.double(), 1, g), b.d)
    for ch in (0, 1):
        terms = F.unfold(b.gs.unsqueeze(1), k, padding=P) * b.w[0, ch].flip(0, 1).reshape(1, -1, 1)
        assert torch.equal(_serial32(terms, 1, g).view(B, H, W), b.gpool[:, ch])
    terms = (F.unfold(b.pool, k, padding=P) * b.gs.view(B, 1, -1)).permute(1, 0, 2).reshape(2 * k * k, -1)
    assert torch.equal(_serial32(terms, 1, g).view(1, 2, k, k), b.dw)


def _rel(a, ref):
    return float(((a - ref).abs() / ref).max())


def _stacked(t):
    """[B,C,H,W] -> [1,C,B*H,W]: the images one below the other, as they lie in memory."""
    B, C, H, W = t.shape
    return t.permute(1, 0, 2, 3).reshape(1, C, B * H, W)


@pytest.mark.parametrize("k", S.KS)
@pytest.mark.parametrize("hw", S.GEOMETRY, ids=_ids)
def test_a_halo_that_reads_the_other_image_fails(hw, k):
    """pool, g_s and the workspace are contiguous over the batch: a halo without the image border's test reads the neighbouring
    image's rows.  At every extent of the geometry test that moves the map beyond its tolerance, and g_pool and dw exactly."""
    H, W = hw
    c = E.sa_fwd_case(2, H, W, S.GEOMETRY_C, k)
    wrong = torch.sigmoid(E.sa_logits(_stacked(c.pool), c.w)).view(2, H, W)
    assert _rel(wrong, c.a64) > 1000 * 8 * S.U
    for mode in ("gate", "map"):
        b = E.sa_bwd_case(2, H, W, S.GEOMETRY_C, k, mode)
        assert _differs(E.sa_gpool(_stacked(b.gs.unsqueeze(1))[:, 0], b.w).view(2, 2, H, W).transpose(0, 1).float(), b.gpool.float())
        assert _differs(E.sa_dw(_stacked(b.gs.unsqueeze(1))[:, 0], _stacked(b.pool), k).float(), b.dw.float())


@pytest.mark.parametrize("k", S.KS)
def test_spatial_attention_case_mutations_fail(k):
    B, H, W = S.SHAPE
    C = 8
    P = k // 2
    c = E.sa_fwd_case(B, H, W, C, k)
    xd = c.x.double()
    # a halo column dropped at the tile seam: the tile that starts at column 32 misses column 31
    seam = E.SA_TW
    right = (torch.arange(W) >= seam).view(1, 1, W)
    cut = c.pool.clone()
    cut[..., seam - 1] = 0
    wrong = torch.where(right, torch.sigmoid(E.sa_logits(cut, c.w)), c.a64)
    assert _rel(wrong, c.a64) > 1000 * 8 * S.U and torch.equal(wrong[..., :seam], c.a64[..., :seam])
    # the last maximum instead of the first; a maximum started at 0
    assert _differs(E.sa_last_max(xd).int(), c.amax.int()) and bool((c.amax <= E.sa_last_max(xd)).all())
    assert _differs(c.max.clamp_min(0).float(), c.max.float())
    wrong = torch.sigmoid(E.sa_logits(torch.stack([c.mean32.double(), c.max.clamp_min(0)], 1), c.w))
    assert _rel(wrong, c.a64) > 1000 * 8 * S.U
    # y rounded twice through bf16 (the map, then the product), and an fp32 y passed through bf16
    a32 = c.a64.float()
    x = E.nhwc(c.x)
    twice = (x * a32.bfloat16().float().unsqueeze(-1)).bfloat16()
    assert _differs(twice, E.sa_gate(x, a32, BF16)) and _differs(E.sa_gate(x, a32, F32).bfloat16().float(), E.sa_gate(x, a32, F32))
    for mode in ("gate", "map"):
        b = E.sa_bwd_case(B, H, W, C, k, mode)
        # the same seam in the backward: g_pool right of the seam misses g_s of column 31, dw of that tile misses pool's column 31
        gs_cut, pool_cut = b.gs.clone(), b.pool.clone()
        gs_cut[..., seam - 1] = 0
        pool_cut[..., seam - 1] = 0
        assert _differs(torch.where(right.unsqueeze(1), E.sa_gpool(gs_cut, b.w), b.gpool).float(), b.gpool.float())
        assert _differs((E.sa_dw(b.gs * right, pool_cut, k) + E.sa_dw(b.gs * ~right, b.pool, k)).float(), b.dw.float())
        # correlation instead of transposed correlation
        corr = F.conv2d(b.gs.unsqueeze(1), b.w.transpose(0, 1), padding=P)
        assert _differs(corr.float(), b.gpool.float())
        for dt in (F32, BF16):
            want = b.dx.bfloat16() if dt == BF16 else b.dx
            assert _differs(E.expected(E.sa_dx64(b.dya, corr, b.amax, C), dt), want)
            # g_avg not divided by C
            undivided = E.sa_dx32(b.dya, b.gpool, b.amax, C, divide=False)
            assert _differs(undivided.bfloat16() if dt == BF16 else undivided, want)
            # the max's gradient on another channel
            other = E.sa_dx32(b.dya, b.gpool, (b.amax + 1) % C, C)
            assert _differs(other.bfloat16() if dt == BF16 else other, want)
        # a for a (1 - a)
        gs_a = b.d * b.a
        assert _differs(gs_a.float(), b.gs.float()) and _differs(E.sa_dw(gs_a, b.pool, k).float(), b.dw.float())
        # one pixel dropped from dw
        hole = b.gs.clone()
        hole[tuple((b.gs != 0).nonzero()[0].tolist())] = 0
        assert _differs(E.sa_dw(hole, b.pool, k).float(), b.dw.float())


@pytest.mark.parametrize("C,first", SA_TWO_STEPS)
def test_a_channel_of_the_second_step_dropped_fails(C, first):
    """The forms whose lanes take a second step: the first channel past the first step left out of the channel sum, of the maximum
    and of sum_c x dy."""
    c = E.sa_fwd_case(*S.SHAPE, C, 7)
    assert first < C and _differs(E.sa_mean32(c.x, drop=first), c.mean32)
    head = c.x[:, :first].double()
    assert _differs(E.sa_first_max(head)[0].float(), c.max.float()) and _differs(E.sa_first_max(head)[1].int(), c.amax.int())
    b = E.sa_bwd_case(*S.SHAPE, C, 7, "gate")
    d = b.d - b.x[:, first].double() * b.dy[:, first].double()
    assert _differs((d * b.a * (1 - b.a)).float(), b.gs.float())
    assert bool((b.amax >= first).any())             # the max's gradient lands in the second step too
