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
