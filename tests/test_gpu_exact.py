"""Bit-exact GPU tests of the matrix-pipe kernels: 3x3 conv forward / backward-data in each of its forms, the fused inference
epilogue, backward-weights in each of its plans, the bf16x3 split products, the transposed convolution and the 1x1 head, through the
same ops wrappers and C ABI calls as test_gpu_ops.py.

The inputs come from tests/exact_inputs.py: integers chosen so that every product and partial sum is exact in fp32, hence the result
does not depend on the order of summation and must equal the float64 reference BIT FOR BIT, in fp32 and (after the one rounding of
the store) in bf16.  No comparison here has a tolerance: each is torch.equal, and each condition on the inputs is an assert on the
reference or on the contraction length (made where the case is built, exact_inputs.*Case).  tests/test_exact_inputs_cpu.py shows on
the CPU that the families meet their conditions at these shapes and that a dropped product, a 16-bit intermediate or a non-zero halo
fails the comparison.

Where a kernel rounds by design the inputs are narrowed, never the comparison:
  * backward-weights plans 5 and 6 (bf16) hand their per-split partial sums to the reduce kernel as block-scaled fp16 (11 bits and a
    power-of-two scale per workgroup block): integers survive while every partial is below 2048, so those plans get a dense +-1 x
    and a ternary dy with fewer than 2048 non-zeros per output channel (asserted), which bounds every subset sum;
  * bf16x3 drops the low x low product: one operand of each product is ternary, so that term is zero.
The pixel passes (BatchNorm + ReLU apply / backward, the pool and head tails, max-pool) and the recomputed stem (uh_stem_*) are
held to float64 in the same way, on the dyadic family, by test_gpu_exact_pixel.py, which also calls them with pixel pitches.
The BatchNorm statistics of the conv epilogue (divisions) are held row by row by test_gpu_bn_stats.py: the rows every forward form
here writes (counts exactly, moments within bounds derived from each producer's arithmetic, bit for bit on a family made for it),
uh_bn_finalize and uh_bn_eval_coeffs on synthetic rows, and the chain against float64 BatchNorm2d; the recomputed stem's rows
(uh_stem_stats) in test_gpu_exact_pixel.py.  Not covered here or there: the backward rows of uh_conv3x3_dgrad_bnsum
(test_gpu_bnsum.py), the bilinear pair (weights that are no dyadic numbers:
test_gpu_ops.py, and pitched against dense calls in test_gpu_exact_pixel.py), the narrow entry points (held bit for bit to the
padded form there), tensors past 2 GiB (forward code 5, test_gpu_large.py), the optimizer (held to float64, one step and twenty
chained, by test_gpu_ema.py).  The default loss (csrc/loss.hip) is held to float64 op by op, with derived bounds, by
test_gpu_loss_ops.py."""
import ctypes

import pytest
import torch

import exact_inputs as E

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
FAMILIES = ("ternary", "wide")


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    return torch.device("cuda:0")


def _name(dtype):
    return "bf16" if dtype == BF16 else "fp32"


def _to(t, dtype, dev):
    """NCHW float32 (CPU) -> dense NHWC on the device; the families' values are exact in either dtype."""
    g = E.nhwc(t).to(dev, dtype)
    assert torch.equal(g.float().cpu(), E.nhwc(t))
    return g


# ------------------------------------------------------------------------------------------------ 3x3 forward / backward-data
# (B, H, W, C0, C1, Cout) -> the answer of uh_conv3x3_fwd_kernel for the forward call in (fp32, bf16); None: not run in that dtype.
# 0 = generic or stem, 1 = 128-channel slabs, 2 = register-resident filter (bf16), 3 = K split (bf16), 4 = streaming filter.
FWD_CASES = [
    ((2, 12, 14, 8, 8, 16), 0, 0),           # generic, two sources
    ((3, 19, 33, 1, 0, 64), 0, 0),           # stem, one channel
    ((2, 20, 20, 3, 0, 64), 0, 0),           # stem, three channels
    ((2, 120, 120, 32, 0, 512), 1, 1),       # 128 tiles x 4 slabs of 128 channels, partial tiles on both edges
    ((2, 17, 23, 64, 0, 64), 4, 2),          # partial tiles on both edges
    ((1, 16, 16, 256, 0, 64), 4, 3),         # one tile, 8 K-chunks: 4 + 4
    ((2, 20, 37, 256, 256, 128), 4, 3),      # two sources, partial tiles
    ((2, 17, 23, 64, 64, 64), 4, 4),         # two sources
    ((1, 40, 24, 128, 128, 128), 4, 3),
    ((1, 16, 16, 1024, 0, 64), 4, 3),        # deep K: 9 216 products per output
    ((1, 448, 448, 64, 0, 64), None, 2),     # 784 tiles on 512 persistent workgroups: the halo buffers go round
]
FWD_PARAMS = [pytest.param(shape, fam, dt, code, id=f"{'x'.join(map(str, shape))}-{fam}-{_name(dt)}-code{code}")
              for shape, c32, c16 in FWD_CASES for fam in FAMILIES for dt, code in ((F32, c32), (BF16, c16)) if code is not None]


@pytest.mark.parametrize("shape,family,dtype,code", FWD_PARAMS)
def test_conv3x3_fwd_and_dgrad_bit_exact(shape, family, dtype, code):
    """Forward (with the BatchNorm statistics epilogue on, as training runs it) and backward-data, row-major and -- where the
    LDS-DMA kernel takes the call -- fragment-major filter packs, against the float64 reference."""
    from unet_amd import ops
    from unet_amd._lib import LIB
    dev = _dev()
    B, H, W, C0, C1, Cout = shape
    Cin = C0 + C1
    dt = 1 if dtype == BF16 else 0
    assert LIB.query("uh_conv3x3_fwd_kernel", B, H, W, C0, C1, Cout, dt) == code
    c = E.conv3x3_case(shape, family)                                  # (asserts the family's conditions on these tensors)
    x0 = _to(c.x[:, :C0], dtype, dev)
    x1 = _to(c.x[:, C0:], dtype, dev) if C1 else None
    dyg = _to(c.dy, dtype, dev)
    want_y, want_dx = E.expected(E.nhwc(c.y), dtype), E.expected(E.nhwc(c.dx), dtype)
    ok_f = ops.wfrag_ok(B, H, W, C0, C1, Cout, C0, C1, Cout, dt)
    ok_d = ops.wfrag_ok(B, H, W, Cout, 0, Cin, Cout, 0, Cin, dt)
    assert ok_f == (code >= 1)
    wg = c.w.to(dev)
    wf, wd = ops.pack_w3x3(wg, dtype, True)
    y, _, _ = ops.conv3x3_fwd(x0, x1, wf, Cout, True)
    E.assert_same(y, want_y, "forward, row-major pack")
    dx, _, _ = ops.conv3x3_fwd(dyg, None, wd, Cin, False)
    E.assert_same(dx, want_dx, "backward-data, row-major pack")
    if C1:                                                             # the two sources as channel slices of one buffer (pixel pitch Cin)
        xg = _to(c.x, dtype, dev)
        ys, _, _ = ops.conv3x3_fwd(xg[..., :C0], xg[..., C0:], wf, Cout, True)
        E.assert_same(ys, want_y, "forward, sources with a pixel pitch of C0 + C1")
    if ok_f or ok_d:
        wf2, wd2 = ops.pack_w3x3(wg, dtype, True, None, ok_f, ok_d)
        if ok_f:
            y2, _, _ = ops.conv3x3_fwd(x0, x1, wf2, Cout, True, None, True)
            E.assert_same(y2, want_y, "forward, fragment-major pack")
        if ok_d:
            dx2, _, _ = ops.conv3x3_fwd(dyg, None, wd2, Cin, False, None, True)
            E.assert_same(dx2, want_dx, "backward-data, fragment-major pack")


# ------------------------------------------------------------------------------------------------ inference epilogue
AFFINE_PARAMS = [pytest.param(shape, fam, dt, code, id=f"{'x'.join(map(str, shape))}-{fam}-{_name(dt)}-code{code}")
                 for shape, dt, code in (((2, 17, 23, 64, 0, 64), BF16, 2), ((2, 17, 23, 64, 64, 64), BF16, 4),
                                         ((2, 17, 23, 64, 64, 64), F32, 4))
                 for fam in FAMILIES]


@pytest.mark.parametrize("shape,family,dtype,code", AFFINE_PARAMS)
def test_conv3x3_affine_relu_epilogue_bit_exact(shape, family, dtype, code):
    """z = max(conv * scale + shift, 0) with scales 2^-3 .. 2^1 and shifts that are multiples of 1/8 (both signs): the product with
    a power of two and the sum are multiples of 1/8 below (2 * 225 K + 4): exact in fp32 while eight times that is below 2^24
    (asserted), however the epilogue fuses them; bf16 stores one rounding of that."""
    from unet_amd import ops
    from unet_amd._lib import LIB
    dev = _dev()
    B, H, W, C0, C1, Cout = shape
    dt = 1 if dtype == BF16 else 0
    assert LIB.query("uh_conv3x3_fwd_kernel", B, H, W, C0, C1, Cout, dt) == code
    c = E.conv3x3_case(shape, family)
    assert (2 * 225 * 9 * (C0 + C1) + 4) * 8 < E.F32_INT               # in eighths: |acc| * largest scale + |shift|
    g = torch.Generator().manual_seed(B + H + C0 + C1)
    scale = 2.0 ** torch.randint(-3, 2, (Cout,), generator=g).float()
    shift = torch.randint(-32, 33, (Cout,), generator=g).float() / 8
    assert bool((shift > 0).any()) and bool((shift < 0).any())
    ref = torch.relu(E.nhwc(c.y) * scale.double() + shift.double())
    assert float(ref.max()) * 8 < E.F32_INT and bool((ref == 0).any()) and bool((ref > 0).any())
    want = E.expected(ref, dtype)
    x0 = _to(c.x[:, :C0], dtype, dev)
    x1 = _to(c.x[:, C0:], dtype, dev) if C1 else None
    sc, sh = scale.to(dev), shift.to(dev)
    ok_f = ops.wfrag_ok(B, H, W, C0, C1, Cout, C0, C1, Cout, dt)
    for frag in ([False, True] if ok_f else [False]):
        wf, _ = ops.pack_w3x3(c.w.to(dev), dtype, False, None, frag, False)
        z = torch.empty(B, H, W, Cout, dtype=dtype, device=dev)
        LIB.call("uh_conv3x3_fwd_affine_relu", x0.data_ptr(), C0, C0, ops._p(x1), C1, C1, wf.data_ptr(), z.data_ptr(), Cout, Cout,
                 sc.data_ptr(), sh.data_ptr(), B, H, W, ops.conv_flags(dt, frag), ops._stream())
        E.assert_same(z, want, f"affine + ReLU epilogue, {'fragment' if frag else 'row'}-major pack")


# ------------------------------------------------------------------------------------------------ backward-weights
# (answer of uh_conv3x3_wgrad_plan, dtype, shape, families).  "wide": [-15, 15] in both operands, exact while the fp32 partial results
# stay fp32 (plans 0-4).  "slab": dense +-1 x, ternary dy with < 2048 non-zeros per output channel -- exact through the block-scaled
# fp16 slabs of plans 5 and 6 as well.  The last shape has 512 pixel ranges: the slab reduce adds 512 partial results per element.
WGRAD_CASES = [
    (0, BF16, (2, 12, 14, 8, 8, 16), ("wide", "slab")),
    (0, F32, (2, 12, 14, 8, 8, 16), ("wide", "slab")),
    (1, F32, (2, 20, 20, 3, 0, 6), ("wide", "slab")),
    (2, F32, (2, 20, 20, 3, 0, 64), ("wide", "slab")),
    (3, BF16, (3, 19, 33, 1, 0, 64), ("wide", "slab")),
    (4, F32, (2, 17, 23, 64, 64, 64), ("wide", "slab")),
    (5, BF16, (2, 17, 23, 64, 64, 64), ("slab",)),
    (6, BF16, (1, 16, 16, 128, 0, 256), ("slab",)),
    (5, BF16, (4, 320, 320, 64, 0, 64), ("slab",)),
]
# the float64 backward-weights reference of the last shape alone takes longer than the rest of this file: float32 there, exact
# because every subset sum is an integer below 2048 (asserted), and test_exact_inputs_cpu.py holds float32 == float64 for the family
WGRAD_REF32 = {(4, 320, 320, 64, 0, 64)}
WGRAD_PARAMS = [pytest.param(code, dt, shape, fam, id=f"plan{code}-{_name(dt)}-{'x'.join(map(str, shape))}-{fam}")
                for code, dt, shape, fams in WGRAD_CASES for fam in fams]


def wgrad_ref_dtype(shape):
    return torch.float32 if shape in WGRAD_REF32 else torch.float64


@pytest.mark.parametrize("code,dtype,shape,family", WGRAD_PARAMS)
def test_conv3x3_wgrad_bit_exact(code, dtype, shape, family):
    from unet_amd import ops
    from unet_amd._lib import LIB
    dev = _dev()
    B, H, W, C0, C1, Cout = shape
    Cin = C0 + C1
    dt = 1 if dtype == BF16 else 0
    plan = (ctypes.c_int64 * 8)()
    LIB.call("uh_conv3x3_wgrad_plan", B, H, W, C0, C1, Cout, dt, 0, ctypes.addressof(plan))
    assert plan[0] == code, list(plan)
    assert (plan[5] == 1) == (code >= 5), list(plan)                   # the fp16 slabs are the ones the "slab" family is made for
    c = E.wgrad_case(shape, family, wgrad_ref_dtype(shape))
    x0 = _to(c.x[:, :C0], dtype, dev)
    x1 = _to(c.x[:, C0:], dtype, dev) if C1 else None
    dwk = torch.full((Cout * 9 * Cin,), float("nan"), dtype=torch.float32, device=dev)
    ops.conv3x3_wgrad(_to(c.dy, dtype, dev), x0, x1, dwk)
    E.assert_same(dwk.view(Cout, 3, 3, Cin), c.dw.permute(0, 2, 3, 1).contiguous().float(), "backward-weights (Cout, r, s, Cin)")


# ------------------------------------------------------------------------------------------------ bf16x3 split products
SPLIT_SHAPES = [(2, 17, 23, 64, 64, 64), (2, 8, 8, 512, 0, 512)]
SPLIT_PARAMS = [pytest.param(shape, role, id=f"{'x'.join(map(str, shape))}-12bit-{role}") for shape in SPLIT_SHAPES for role in E.SPLIT_ROLES]


@pytest.mark.parametrize("shape,role", SPLIT_PARAMS)
def test_conv3x3_bf16x3_bit_exact(shape, role):
    """fp32 tensors, products w*x ~= wh*xh + wh*xl + wl*xh on the bf16 matrix pipe (UH_F32X3): forward, backward-data and
    backward-weights (split=True).  The dropped wl*xl term is the kernels' deliberate rounding: in every product here one operand is
    ternary, so its low part and that term are zero, and the three products kept are the exact product (see exact_inputs.SplitCase
    for which pair each role exercises)."""
    from unet_amd import ops
    from unet_amd._lib import LIB, UH_F32X3
    dev = _dev()
    B, H, W, C0, C1, Cout = shape
    Cin = C0 + C1
    assert LIB.query("uh_conv3x3_fwd_kernel", B, H, W, C0, C1, Cout, UH_F32X3) == 4
    plan = (ctypes.c_int64 * 8)()
    LIB.call("uh_conv3x3_wgrad_plan", B, H, W, C0, C1, Cout, UH_F32X3, 0, ctypes.addressof(plan))
    assert plan[0] == 4, list(plan)
    c = E.split_case(shape, role)
    x0 = _to(c.x[:, :C0], F32, dev)
    x1 = _to(c.x[:, C0:], F32, dev) if C1 else None
    dyg = _to(c.dy, F32, dev)
    wf, wd = ops.pack_w3x3(c.w.to(dev), F32, True, UH_F32X3)
    y, _, _ = ops.conv3x3_fwd(x0, x1, wf, Cout, True, UH_F32X3)
    E.assert_same(y, E.nhwc(c.y).float(), "bf16x3 forward")
    dx, _, _ = ops.conv3x3_fwd(dyg, None, wd, Cin, False, UH_F32X3)
    E.assert_same(dx, E.nhwc(c.dx).float(), "bf16x3 backward-data")
    dwk = torch.full((Cout * 9 * Cin,), float("nan"), dtype=torch.float32, device=dev)
    ops.conv3x3_wgrad(dyg, x0, x1, dwk, split=True)
    E.assert_same(dwk.view(Cout, 3, 3, Cin), c.dw.permute(0, 2, 3, 1).contiguous().float(), "bf16x3 backward-weights (Cout, r, s, Cin)")


# ------------------------------------------------------------------------------------------------ transposed convolution
# (B, h, w, Cin, Ho, Wo) -> Cin // 2 channels; does the MFMA path (csrc/convt_mfma.hip) take it, or the plain one (convt_1x1.hip)
CONVT_CASES = [
    ((2, 8, 9, 16, 17, 19), False),          # padded by one row and one column
    ((2, 16, 16, 128, 32, 32), True),        # exact extent
    ((2, 8, 8, 64, 17, 19), True),           # padded by 1 row, 3 columns: uneven left / right
    ((2, 16, 24, 512, 32, 48), True),        # deep K
]
CONVT_PARAMS = [pytest.param(shape, mfma, fam, dt, id=f"{'x'.join(map(str, shape))}-{fam}-{_name(dt)}")
                for shape, mfma in CONVT_CASES for fam in FAMILIES for dt in (F32, BF16)]
CONVT_SPLIT_SHAPES = [(2, 16, 16, 128, 32, 32), (2, 8, 8, 64, 17, 19)]
CONVT_SPLIT_PARAMS = [pytest.param(shape, "split_" + role, id=f"{'x'.join(map(str, shape))}-12bit-{role}")
                      for shape in CONVT_SPLIT_SHAPES for role in E.SPLIT_ROLES]


def _convt_run(c, dtype, dev):
    from unet_amd import ops
    B, h, w, Cin, Ho, Wo = c.shape
    xg = _to(c.x, dtype, dev).requires_grad_(True)
    wg, bg = c.wt.to(dev).requires_grad_(True), c.bias.to(dev).requires_grad_(True)
    y = ops.ConvTranspose2x2PadFn.apply(xg, wg, bg, Ho, Wo)
    y.backward(_to(c.dy, dtype, dev))
    E.assert_same(y.detach(), E.expected(E.nhwc(c.y), dtype), "forward")
    E.assert_same(xg.grad, E.expected(E.nhwc(c.dx), dtype), "backward-data")
    E.assert_same(wg.grad, c.dw.float(), "backward-weights (Cin, Cout, r, s)")
    E.assert_same(bg.grad, c.db.float(), "bias gradient")


@pytest.mark.parametrize("shape,mfma,family,dtype", CONVT_PARAMS)
def test_conv_transpose_bit_exact(shape, mfma, family, dtype):
    """ConvTranspose2d(k = 2, s = 2) + integer bias + padding to (Ho, Wo), forward and backward, on the MFMA and on the plain path."""
    from unet_amd._lib import LIB
    dev = _dev()
    B, h, w, Cin, Ho, Wo = shape
    assert bool(LIB.query("uh_convt2x2_mfma_ok", B, h, w, Cin, Cin // 2, Ho, Wo, 1 if dtype == BF16 else 0)) == mfma
    _convt_run(E.convt_case(shape, family), dtype, dev)


@pytest.mark.parametrize("shape,family", CONVT_SPLIT_PARAMS)
def test_conv_transpose_bf16x3_bit_exact(shape, family):
    """The same under ops.step_state(fp32_mode="bf16x3") (both operands split in registers, low x low dropped): 12-bit integers in
    one of x, weight, dy and dense +-1 in the other two, so each product has at most one low part."""
    from unet_amd import ops
    from unet_amd._lib import LIB, UH_F32X3
    dev = _dev()
    B, h, w, Cin, Ho, Wo = shape
    assert LIB.query("uh_convt2x2_mfma_ok", B, h, w, Cin, Cin // 2, Ho, Wo, UH_F32X3) == 1      # (bf16x3 exists on the MFMA path only)
    with ops.step_state(fp32_mode="bf16x3"):
        _convt_run(E.convt_case(shape, family), F32, dev)


# ------------------------------------------------------------------------------------------------ 1x1 head
OUTCONV_SHAPE = (2, 33, 20, 64)              # test_gpu_ops.test_outconv_1x1's


@pytest.mark.parametrize("dtype", [F32, BF16], ids=_name)
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("ncls", [1, 4])
def test_outconv_1x1_bit_exact(ncls, family, dtype):
    from unet_amd import ops
    dev = _dev()
    c = E.outconv_case(OUTCONV_SHAPE, ncls, family)
    xg = _to(c.x, dtype, dev).requires_grad_(True)
    wg, bg = c.w.to(dev).requires_grad_(True), c.bias.to(dev).requires_grad_(True)
    y = ops.OutConv1x1Fn.apply(xg, wg, bg)
    y.backward(E.nhwc(c.dy).to(dev))
    assert y.dtype == F32
    E.assert_same(y.detach(), E.nhwc(c.y).float(), "logits")
    E.assert_same(xg.grad, E.expected(E.nhwc(c.dx), dtype), "backward-data")
    E.assert_same(wg.grad, c.dw.float(), "backward-weights (class, Cin, 1, 1)")
    E.assert_same(bg.grad, c.db.float(), "bias gradient")
