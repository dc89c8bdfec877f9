"""Inputs on which the matrix-pipe kernels have ONE right answer, and the comparator that holds them to it.  CPU only.

The conv / transposed-conv / 1x1 kernels accumulate in fp32.  Where every product and every partial sum is an integer (or an
integer times one fixed power of two) below 2^24, fp32 addition is exact in ANY order, so the result equals the float64 reference
bit for bit: no tolerance, and a missing, doubled or misplaced term, or an intermediate kept in fewer bits, changes the output.

The pixel passes (BatchNorm + ReLU, the pool and head tails, max-pool) and the recomputed stem have their own "dyadic" family and
case classes in the second half of this file; the spatial-attention kernels have theirs (SaFwdCase, SaBwdCase) at its end.

Families (all values are exact in bf16, so one set of inputs serves the fp32 and the bf16 kernels):
  ternary  {-1, 0, +1}; for a contraction of length K the densities obey p_a * p_b <= 1100 / K, which keeps the outputs (integers)
           within +-256: bf16 stores them exactly.  `require_bf16_exact` asserts that on the reference -- a condition on the inputs.
           Every non-zero term is visible in the output bits.
  wide     integers in [-15, 15]: every partial sum is below 225 K < 2^24 (`require_wide_k`), the fp32 accumulator is exact, and a
           bf16 result is ONE round-to-nearest-even of the exact value (`to_bf16`).  An intermediate that passes through 16 bits, or a
           sum formed in less than fp32, shows here.
  split    for the bf16x3 products w*x ~= wh*xh + wh*xl + wl*xh: one operand holds integers of up to 12 bits (they need the high AND
           the low bf16 part), the other is ternary (its low part is zero), so the three products kept are the exact product and the
           dropped low*low term is zero.  `require_split` bounds the partial sums.
"""
import functools

import torch
import torch.nn.functional as F

F32_INT = 1 << 24              # integers up to here are exact in fp32, whatever the order they were added in
BF16_INT = 256                 # ... and up to here in bf16 (8 significant bits)
TERNARY_BUDGET = 1100          # expected non-zero products per output: sd = sqrt(1100) = 33, five sd = 166 < 256
WIDE_MAX = 15
SPLIT_MAX = 2047               # 11 bits and a sign


def ternary_density(K):
    """p_a * p_b for a contraction of length K."""
    return min(1.0, TERNARY_BUDGET / K)


def ternary(shape, p, g):
    sign = torch.randint(0, 2, shape, generator=g) * 2 - 1
    keep = torch.rand(shape, generator=g) < p
    return (sign * keep).float()


def wide(shape, g):
    return torch.randint(-WIDE_MAX, WIDE_MAX + 1, shape, generator=g).float()


def split_ints(shape, g):
    v = torch.randint(-SPLIT_MAX, SPLIT_MAX + 1, shape, generator=g).float()
    assert bool((v.bfloat16().float() != v).any()), "the operand must need its low bf16 part"
    assert torch.equal(v.bfloat16().float() + (v - v.bfloat16().float()).bfloat16().float(), v)      # high + low IS the value
    return v


def require_wide_k(K):
    assert WIDE_MAX * WIDE_MAX * K < F32_INT, f"wide family: 225 * {K} reaches 2^24"


def require_bf16_exact(ref):
    m = float(ref.abs().max())
    assert m <= BF16_INT, f"ternary family: max |reference| = {m} > 256, bf16 would round it"


def require_split(nnz_along_k):
    """nnz_along_k: the largest count of non-zeros of the TERNARY operand inside one contraction.  The 12-bit operand enters as its
    high part (at most 2048 after rounding) and its low part (at most 4), both into the same accumulator: 4096 per term bounds
    every partial sum whatever the order -- stricter than 2047 per term, which bounds the finished sum only."""
    n = int(nnz_along_k)
    assert SPLIT_MAX * n < F32_INT and 4096 * n < F32_INT, f"split family: {n} non-zeros along K"


def nnz_per_filter(w):
    """[Cout, Cin, kh, kw] -> the largest non-zero count of one output channel's filter."""
    return int((w != 0).sum(dim=(1, 2, 3)).max())


def nnz_per_window(x, k=3):
    """[B, C, H, W] -> the largest non-zero count inside one k x k x C window."""
    cnt = (x != 0).sum(dim=1, keepdim=True).float()
    return int(F.conv2d(cnt, torch.ones(1, 1, k, k), padding=k // 2).max())


def to_bf16(ref):
    """What a kernel that holds the exact value in fp32 stores in bf16: one round-to-nearest-even."""
    assert float(ref.abs().max()) < F32_INT
    return ref.float().bfloat16()


def expected(ref, dtype):
    return to_bf16(ref) if dtype == torch.bfloat16 else ref.float()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


# ------------------------------------------------------------------------------------------------ comparator
_NAMES = {4: "bhwc"}


def mismatches(got, want, limit=6):
    """None when got == want value for value (torch.equal), else the diagnosis: count and the first indices with got / want."""
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    if torch.equal(got, want):
        return None
    bad = ~(got == want)                                       # (a NaN counts)
    idx = bad.nonzero()
    names = _NAMES.get(got.dim(), "")
    lines = [f"{int(bad.sum())} of {bad.numel()} values differ; first at " + (f"({', '.join(names)})" if names else "index") + ":"]
    for i in idx[:limit].tolist():
        lines.append(f"  {tuple(i)}: got {float(got[tuple(i)])!r}, want {float(want[tuple(i)])!r}")
    return "\n".join(lines)


def assert_same(got, want, what=""):
    msg = mismatches(got, want)
    assert msg is None, f"{what}: {msg}"


# ------------------------------------------------------------------------------------------------ cases (inputs + references)
def _seed(*v):
    s = 7
    for k in v:
        s = (s * 1000003 + int(k)) % (1 << 31)
    return s


class Conv3x3Case:
    """x [B,Cin,H,W], w [Cout,Cin,3,3], dy [B,Cout,H,W] (float32 holding the family's values) and the references y = conv(x, w),
    dx = the gradient of x under dy, in `ref_dtype`.  Conditions of the family are asserted here, on these very tensors."""

    def __init__(self, shape, family, ref_dtype=torch.float64):
        B, H, W, C0, C1, Cout = shape
        Cin = C0 + C1
        Kf, Kd = 9 * Cin, 9 * Cout
        g = torch.Generator().manual_seed(_seed(*shape, family == "wide"))
        if family == "ternary":
            pw = ternary_density(max(Kf, Kd)) ** 0.5
            self.w = ternary((Cout, Cin, 3, 3), pw, g)
            self.x = ternary((B, Cin, H, W), ternary_density(Kf) / pw, g)
            self.dy = ternary((B, Cout, H, W), min(1.0, ternary_density(Kd) / pw), g)
        elif family == "wide":
            require_wide_k(Kf)
            require_wide_k(Kd)
            self.w, self.x, self.dy = wide((Cout, Cin, 3, 3), g), wide((B, Cin, H, W), g), wide((B, Cout, H, W), g)
        else:
            raise ValueError(family)
        self.shape, self.family = shape, family
        self.y = F.conv2d(self.x.to(ref_dtype), self.w.to(ref_dtype), padding=1)
        self.dx = F.conv_transpose2d(self.dy.to(ref_dtype), self.w.to(ref_dtype), padding=1)
        if family == "ternary":
            require_bf16_exact(self.y)
            require_bf16_exact(self.dx)
        else:
            assert float(self.y.abs().max()) < F32_INT and float(self.dx.abs().max()) < F32_INT


@functools.lru_cache(maxsize=2)
def conv3x3_case(shape, family, ref_dtype=torch.float64):
    return Conv3x3Case(shape, family, ref_dtype)


def _dw_ref(x, dy, ref_dtype):
    Cout, Cin = dy.shape[1], x.shape[1]
    w0 = torch.zeros(Cout, Cin, 3, 3, dtype=ref_dtype, requires_grad=True)
    (dw,) = torch.autograd.grad(F.conv2d(x.to(ref_dtype), w0, padding=1), [w0], dy.to(ref_dtype))
    return dw


class WgradCase:
    """x, dy and dw = the filter gradient.  family "wide": both in [-15, 15], every partial sum below 225 * B*H*W < 2^24.
    family "slab": x dense +-1, dy ternary with about 1024 non-zeros per output channel -- asserted below 2048, which bounds EVERY
    subset sum of one filter element, so the partial results survive the 11 bits of a block-scaled fp16 slab."""

    def __init__(self, shape, family, ref_dtype=torch.float64):
        B, H, W, C0, C1, Cout = shape
        Cin, n = C0 + C1, B * H * W
        g = torch.Generator().manual_seed(_seed(*shape, 11, family == "wide"))
        if family == "wide":
            require_wide_k(n)
            self.x, self.dy = wide((B, Cin, H, W), g), wide((B, Cout, H, W), g)
        elif family == "slab":
            self.x = ternary((B, Cin, H, W), 1.0, g)
            self.dy = ternary((B, Cout, H, W), min(1.0, 1024.0 / n), g)
            self.nnz = int((self.dy != 0).sum(dim=(0, 2, 3)).max())
            assert self.nnz < 2048, f"slab family: {self.nnz} non-zeros of dy in one output channel"
        else:
            raise ValueError(family)
        self.shape, self.family = shape, family
        self.dw = _dw_ref(self.x, self.dy, ref_dtype)
        assert float(self.dw.abs().max()) < (2048 if family == "slab" else F32_INT)


@functools.lru_cache(maxsize=2)
def wgrad_case(shape, family, ref_dtype=torch.float64):
    return WgradCase(shape, family, ref_dtype)


SPLIT_ROLES = ("x", "w", "dy")          # which tensor holds the 12-bit integers; the other two are ternary


def _split_operands(role, shapes, p, g):
    return [split_ints(shp, g) if name == role else ternary(shp, p, g) for name, shp in zip(SPLIT_ROLES, shapes)]


class SplitCase:
    """bf16x3 on the 3x3 conv: ONE of x, w, dy holds 12-bit integers, the other two are ternary (half of them non-zero), so every
    product the three kernels form has at most one operand with a low part:
        role   forward y = w * x       backward-data dx = w^T * dy     backward-weights dw = dy * x
        "x"    wh*xh + wh*xl           (ternary)                       dyh*xh + dyh*xl
        "w"    wh*xh + wl*xh           wh*dyh + wl*dyh                 (ternary)
        "dy"   (ternary)               wh*dyh + wh*dyl                 dyh*xh + dyl*xh
    Each contraction's count of ternary non-zeros is asserted (require_split)."""

    def __init__(self, shape, role, ref_dtype=torch.float64):
        B, H, W, C0, C1, Cout = shape
        Cin = C0 + C1
        g = torch.Generator().manual_seed(_seed(*shape, 23, SPLIT_ROLES.index(role)))
        self.x, self.w, self.dy = _split_operands(role, [(B, Cin, H, W), (Cout, Cin, 3, 3), (B, Cout, H, W)], 0.5, g)
        x, w, dy = self.x, self.w, self.dy

        def per_channel(t):
            return int((t != 0).sum(dim=(0, 2, 3)).max())

        # the ternary partner's non-zeros inside one contraction, per kernel (a ternary x ternary contraction is bounded by its length)
        counts = {"x": (nnz_per_filter(w), None, per_channel(dy)),
                  "w": (nnz_per_window(x), nnz_per_window(dy), None),
                  "dy": (None, nnz_per_filter(w.transpose(0, 1)), per_channel(x))}[role]
        for n in counts:
            if n is not None:
                require_split(n)
        assert max(9 * Cin, 9 * Cout, B * H * W) < F32_INT
        self.shape, self.role = shape, role
        self.y = F.conv2d(x.to(ref_dtype), w.to(ref_dtype), padding=1)
        self.dx = F.conv_transpose2d(dy.to(ref_dtype), w.to(ref_dtype), padding=1)
        self.dw = _dw_ref(x, dy, ref_dtype)
        for t in (self.y, self.dx, self.dw):
            assert float(t.abs().max()) < F32_INT


@functools.lru_cache(maxsize=2)
def split_case(shape, role, ref_dtype=torch.float64):
    return SplitCase(shape, role, ref_dtype)


class ConvTCase:
    """ConvTranspose2d(Cin, Cin // 2, 2, stride=2) + bias, padded to Ho x Wo.  family "ternary" / "wide" as above (K = Cin forward,
    4 * Cout backward-data, B*h*w backward-weights); "split_x" / "split_w" / "split_dy" as SplitCase's roles with dense +-1 ternaries.
    The bias holds integers."""

    def __init__(self, shape, family, ref_dtype=torch.float64):
        B, h, w, Cin, Ho, Wo = shape
        Cout = Cin // 2
        g = torch.Generator().manual_seed(_seed(*shape, 31, len(family), ord(family[-1])))
        npx = B * h * w
        shapes = [(B, Cin, h, w), (Cin, Cout, 2, 2), (B, Cout, Ho, Wo)]
        if family == "ternary":
            self.wt = ternary(shapes[1], 1.0, g)
            self.x = ternary(shapes[0], ternary_density(Cin), g)
            self.dy = ternary(shapes[2], ternary_density(4 * Cout), g)
            self.bias = torch.randint(-8, 9, (Cout,), generator=g).float()
        elif family == "wide":
            require_wide_k(max(Cin, 4 * Cout, 4 * npx))
            self.x, self.wt, self.dy = wide(shapes[0], g), wide(shapes[1], g), wide(shapes[2], g)
            self.bias = wide((Cout,), g)
        elif family.startswith("split_"):
            self.x, self.wt, self.dy = _split_operands(family[6:], shapes, 1.0, g)
            self.bias = split_ints((Cout,), g)
            require_split(max(Cin, 4 * Cout, 4 * npx) + 1)          # every contraction, the bias (forward) / all of dy (bias gradient) included
        else:
            raise ValueError(family)
        self.shape, self.family = shape, family
        xd = self.x.to(ref_dtype).requires_grad_(True)
        wd = self.wt.to(ref_dtype).requires_grad_(True)
        bd = self.bias.to(ref_dtype).requires_grad_(True)
        up = F.conv_transpose2d(xd, wd, bd, stride=2)
        dY, dX = Ho - up.shape[2], Wo - up.shape[3]
        y = F.pad(up, [dX // 2, dX - dX // 2, dY // 2, dY - dY // 2])
        self.y = y.detach()
        self.dx, self.dw, self.db = torch.autograd.grad(y, [xd, wd, bd], self.dy.to(ref_dtype))
        if family == "ternary":
            require_bf16_exact(self.y)
            require_bf16_exact(self.dx)
        for t in (self.y, self.dx, self.dw, self.db):
            assert float(t.abs().max()) < F32_INT


@functools.lru_cache(maxsize=2)
def convt_case(shape, family, ref_dtype=torch.float64):
    return ConvTCase(shape, family, ref_dtype)


class OutConvCase:
    """Conv2d(C, ncls, 1) + integer bias: x [B,C,H,W], w [ncls,C,1,1], dy [B,ncls,H,W]; K = C forward, ncls backward-data, B*H*W for
    the weight and bias gradients (fp32 results)."""

    def __init__(self, shape, ncls, family, ref_dtype=torch.float64):
        B, H, W, C = shape
        g = torch.Generator().manual_seed(_seed(*shape, ncls, 41, family == "wide"))
        if family == "ternary":
            p = ternary_density(C)
            self.x, self.w, self.dy = ternary((B, C, H, W), p, g), ternary((ncls, C, 1, 1), 1.0, g), ternary((B, ncls, H, W), 1.0, g)
            self.bias = torch.randint(-8, 9, (ncls,), generator=g).float()
        elif family == "wide":
            require_wide_k(max(C + 1, ncls, B * H * W))
            self.x, self.w, self.dy = wide((B, C, H, W), g), wide((ncls, C, 1, 1), g), wide((B, ncls, H, W), g)
            self.bias = wide((ncls,), g)
        else:
            raise ValueError(family)
        xd = self.x.to(ref_dtype).requires_grad_(True)
        wd = self.w.to(ref_dtype).requires_grad_(True)
        bd = self.bias.to(ref_dtype).requires_grad_(True)
        y = F.conv2d(xd, wd, bd)
        self.y = y.detach()
        self.dx, self.dw, self.db = torch.autograd.grad(y, [xd, wd, bd], self.dy.to(ref_dtype))
        if family == "ternary":
            require_bf16_exact(self.y)
            require_bf16_exact(self.dx)
        for t in (self.y, self.dx, self.dw, self.db):
            assert float(t.abs().max()) < F32_INT


@functools.lru_cache(maxsize=2)
def outconv_case(shape, ncls, family, ref_dtype=torch.float64):
    return OutConvCase(shape, ncls, family, ref_dtype)


# ------------------------------------------------------------------------------------------------ the dyadic family (pixel passes)
# BatchNorm + ReLU apply / backward, the pool and head tails, max-pool and the recomputed stem are per-channel affine maps, masks,
# 2x2 maxima and sums.  Tensors hold small integers, the per-channel coefficients are dyadic (a few bits times a power of two), so
# every product is exact in fp32 and every term of a sum is a multiple of ONE power-of-two quantum q: while sum |terms| / q stays
# below 2^24 (`require_exact_sum`, asserted on the float64 terms of the very case) every partial sum, in any order and through any
# fused multiply-add, is exact -- the kernel's result has one right value.  Element-wise bf16 outputs are one rounding of it.
SCALE_MAGS = (0.25, 0.5, 1.0, 2.0, 4.0)
RSTDS = (0.5, 1.0, 2.0)
HALVES = 17                    # shift and mean: k / 2 for k in -8 .. 8
N_TOTAL = 1024                 # the SyncBN form's pixel count: a power of two that is no case's own pixel count


def require_exact_sum(terms, q, dim, what=""):
    """terms: the float64 terms of a reduction over `dim` (for an element-wise result: every term a kernel may form for one element,
    stacked along `dim`).  All are multiples of the power-of-two quantum q, and per output element sum |terms| / q < 2^24: every
    partial sum, in any order and through any fused multiply-add, is then a multiple of q below 2^24 q -- exact in fp32."""
    t = terms / q
    assert torch.equal(t, t.round()), f"{what}: a term is no multiple of {q}"
    m = float(t.abs().sum(dim=dim).max())
    assert m < F32_INT, f"{what}: sum |terms| / q = {m} reaches 2^24"
    return m


def dyadic_coeffs(C, g, narrow=False):
    """-> scale, shift, mean, rstd (float64 [C]), the tuple distinct for every channel (drawn without replacement from the whole
    set, asserted): a kernel that computes a channel with another channel's coefficients changes the output.
    scale in +-{1/4, 1/2, 1, 2, 4}, shift and mean multiples of 1/2 in [-4, 4], rstd in {1/2, 1, 2};
    narrow: scale in +-{1, 2}, rstd in {1, 2}, mean an integer (coarser quanta for the long sums of the stem)."""
    mags = (1.0, 2.0) if narrow else SCALE_MAGS
    rstds = (1.0, 2.0) if narrow else RSTDS
    nmean = 9 if narrow else HALVES
    radix = (len(mags), 2, HALVES, nmean, len(rstds))
    total = 1
    for r in radix:
        total *= r
    assert C <= total
    idx = torch.randperm(total, generator=g)[:C]
    digits = []
    for r in radix:
        digits.append(idx % r)
        idx = idx // r
    scale = torch.tensor(mags, dtype=torch.float64)[digits[0]] * (digits[1].double() * 2 - 1)
    shift = (digits[2].double() - 8) / 2
    mean = (digits[3].double() - 4) if narrow else (digits[3].double() - 8) / 2
    rstd = torch.tensor(rstds, dtype=torch.float64)[digits[4]]
    tup = torch.stack([scale, shift, mean, rstd], 1)
    assert len(torch.unique(tup, dim=0)) == C, "the coefficient tuples must be distinct per channel"
    assert bool((scale < 0).any()) or C < 4
    return scale, shift, mean, rstd


def _cv(v):
    """[C] -> [1, C, 1, 1]"""
    return v.view(1, -1, 1, 1)


def relu_and_mask(y, scale, shift, dz):
    """z = relu(y * scale + shift) and m = the gradient torch's ReLU passes for dz (0 where z == 0), float64 NCHW."""
    t = (y * _cv(scale) + _cv(shift)).requires_grad_(True)
    z = torch.relu(t)
    (m,) = torch.autograd.grad(z, [t], dz)
    return z.detach(), m


def bn_sums(m, y, mean, rstd, what):
    """-> xhat, sum m, sum m xhat (float64), the two sums exact in fp32 in any order (asserted)."""
    xhat = (y - _cv(mean)) * _cv(rstd)
    require_exact_sum(m, 1.0, (0, 2, 3), what + ": sum m")
    require_exact_sum(m * xhat, 0.25, (0, 2, 3), what + ": sum m xhat")       # (y - mean) in halves, rstd >= 1/2
    return xhat, m.sum((0, 2, 3)), (m * xhat).sum((0, 2, 3))


def bn_dy(m, y, scale, mean, rstd, dgamma, dbeta, n, q_sums, what):
    """dy = scale (m - dbeta / n - xhat dgamma / n) in float64.  q_sums: the quantum of dgamma and dbeta.  Every term a kernel may
    form on the way -- scale m, scale dbeta / n, scale rstd dgamma / n times y and times mean -- is a multiple of
    q = q_sums / (16 n) (scale >= 1/4, rstd >= 1/2, mean in halves), and their absolute sum stays below 2^24 q (asserted): whatever the
    grouping (the kernels use a m + (b y + k), k = -scale dbeta / n - b mean), fp32 holds every intermediate exactly."""
    q = q_sums / (16.0 * n)
    b = _cv(scale * rstd * dgamma / n)
    terms = torch.stack([(_cv(scale) * m).abs(), (_cv(scale * dbeta / n)).abs().expand_as(m), (b * y).abs(), (b * _cv(mean)).abs().expand_as(m)])
    require_exact_sum(terms, q, 0, what + ": dy")
    xhat = (y - _cv(mean)) * _cv(rstd)
    return _cv(scale) * (m - _cv(dbeta) / n - xhat * _cv(dgamma) / n)


def given_sums(C, g, unit=1.0):
    """dgamma, dbeta of the SyncBN form: integers (times `unit`) in [-3, 3]."""
    return (torch.randint(-3, 4, (C,), generator=g).double() * unit, torch.randint(-3, 4, (C,), generator=g).double() * unit)


def is_pow2(n):
    return n > 0 and n & (n - 1) == 0


class BnCase:
    """BatchNorm + ReLU on [B,C,H,W] (NCHW float64 references; the inputs are exact in bf16):
        z = relu(y scale + shift);  m = dz [z > 0] (torch's ReLU gradient: 0 at z == 0, and many z are exactly 0 here);
        sum1 = sum m, sum2 = sum m xhat, xhat = (y - mean) rstd;
        dy = scale (m - dbeta / n - xhat dgamma / n) with GIVEN integer dgamma, dbeta and n = N_TOTAL (the SyncBN form), and --
        `own_dy`, where the pixel count is a power of two -- with dgamma = sum2, dbeta = sum1, n = the pixel count.
    dz: "wide" integers, or "ternary" of density p_dz where the sums of a large extent need it."""

    def __init__(self, B, H, W, C, dz_family="wide", p_dz=1.0):
        g = torch.Generator().manual_seed(_seed(B, H, W, C, 53, dz_family == "wide"))
        self.shape, self.npix = (B, H, W, C), B * H * W
        self.y = wide((B, C, H, W), g)
        self.dz = wide((B, C, H, W), g) if dz_family == "wide" else ternary((B, C, H, W), p_dz, g)
        self.scale, self.shift, self.mean, self.rstd = dyadic_coeffs(C, g)
        self.dgamma, self.dbeta = given_sums(C, g)
        y, dz = self.y.double(), self.dz.double()
        self.z, self.m = relu_and_mask(y, self.scale, self.shift, dz)
        assert bool((self.z == 0).any()) and bool((self.z > 0).any())
        _, self.sum1, self.sum2 = bn_sums(self.m, y, self.mean, self.rstd, "BnCase")
        self.dy = bn_dy(self.m, y, self.scale, self.mean, self.rstd, self.dgamma, self.dbeta, N_TOTAL, 1.0, "BnCase, given sums")
        self.own_dy = None
        if is_pow2(self.npix):
            self.own_dy = bn_dy(self.m, y, self.scale, self.mean, self.rstd, self.sum2, self.sum1, self.npix, 0.25, "BnCase, own sums")

    def coeffs(self):
        return self.scale, self.shift, self.mean, self.rstd


@functools.lru_cache(maxsize=4)
def bn_case(B, H, W, C, dz_family="wide", p_dz=1.0):
    return BnCase(B, H, W, C, dz_family, p_dz)


def first_max_route(zq, dpool):
    """pooled = MaxPool2d(2) of zq and the gradient of zq under dpool: torch routes it to the FIRST maximum of a window in
    (0,0), (0,1), (1,0), (1,1) order; rows / columns past 2 floor(H / 2) get nothing."""
    zl = zq.clone().requires_grad_(True)
    pooled = F.max_pool2d(zl, 2)
    (route,) = torch.autograd.grad(pooled, [zl], dpool)
    return pooled.detach(), route


class PoolTailCase:
    """BnCase with z also max-pooled 2x2.  Backward takes dskip (optional) plus dpool routed to the first maximum of the window:
    dz = dskip + route(dpool), never stored by the fused kernels.  z holds quarters in [0, 64]: ties are common, all-zero windows
    included (asserted).  The STORED z decides the maximum, so the references round it to the tensor dtype first (quarters up to 64
    are exact in bf16: the rounding of z itself is exercised by the stem's wide family): `refs(dtype, skip)`.  Also serves uh_maxpool2_fwd / _bwd on their own (x = the stored z; H and W
    may then be odd).  sums=False: element-wise outputs only (an extent whose sums would need narrower inputs than its dy)."""

    def __init__(self, B, H, W, C, dz_family="wide", p_dz=1.0, sums=True):
        g = torch.Generator().manual_seed(_seed(B, H, W, C, 59, dz_family == "wide"))
        self.shape, self.npix, self.sums = (B, H, W, C), B * H * W, sums
        draw = (lambda shp: wide(shp, g)) if dz_family == "wide" else (lambda shp: ternary(shp, p_dz, g))
        self.y = wide((B, C, H, W), g)
        self.dskip, self.dpool = draw((B, C, H, W)), draw((B, C, H // 2, W // 2))
        self.scale, self.shift, self.mean, self.rstd = dyadic_coeffs(C, g)
        if self.npix < 200 and not is_pow2(self.npix) and C >= 2:
            # two means that are halves but NO bf16 numbers (nine bits): the bf16 reduce kernel sums m (y - pivot) around pivot =
            # mean rounded to bf16 and corrects by (mean - pivot) sum m afterwards -- with every mean a bf16 number that term is 0.
            # (small extents only, and none whose own sums feed an exact dy: |xhat| grows tenfold, and with it the sums; the conditions
            # are asserted as everywhere)
            self.mean[0], self.mean[1] = 128.5, -200.5
            assert not torch.equal(self.mean.float().bfloat16().double(), self.mean)
        self.dgamma, self.dbeta = given_sums(C, g)
        self.z, _ = relu_and_mask(self.y.double(), self.scale, self.shift, torch.zeros(B, C, H, W, dtype=torch.float64))
        self._refs = {}

    def coeffs(self):
        return self.scale, self.shift, self.mean, self.rstd

    def refs(self, dtype, skip=True):
        """-> dict(zq, pooled, route, dz, m, sum1, sum2, dy[, own_dy]) in float64; zq = z as stored in `dtype`."""
        key = (dtype, skip)
        if key in self._refs:
            return self._refs[key]
        y = self.y.double()
        zq = expected(self.z, dtype).double()
        pooled, route = first_max_route(zq, self.dpool.double())
        win = F.unfold(zq, 2, stride=2)                                       # [B, C * 4, windows]
        win = win.view(zq.shape[0], zq.shape[1], 4, -1)
        ties = (win == win.max(2, keepdim=True).values).sum(2)
        if win.numel() >= 400:                                                # (the few windows of a tiny extent need not hold one)
            assert bool((ties > 1).any()) and bool((win.max(2).values == 0).any()), "the case must hold ties and all-zero windows"
        dz = route + (self.dskip.double() if skip else 0.0)
        assert float(dz.abs().max()) <= BF16_INT                              # dz = round_T(dskip + dpool): nothing to round
        _, m = relu_and_mask(y, self.scale, self.shift, dz)
        r = dict(zq=zq, pooled=pooled, route=route, dz=dz, m=m)
        if self.sums:
            _, r["sum1"], r["sum2"] = bn_sums(m, y, self.mean, self.rstd, "PoolTailCase")
        r["dy"] = bn_dy(m, y, self.scale, self.mean, self.rstd, self.dgamma, self.dbeta, N_TOTAL, 1.0, "PoolTailCase, given sums")
        if self.sums and is_pow2(self.npix):
            r["own_dy"] = bn_dy(m, y, self.scale, self.mean, self.rstd, r["sum2"], r["sum1"], self.npix, 0.25, "PoolTailCase, own sums")
        self._refs[key] = r
        return r


@functools.lru_cache(maxsize=4)
def pool_tail_case(B, H, W, C, dz_family="wide", p_dz=1.0, sums=True):
    return PoolTailCase(B, H, W, C, dz_family, p_dz, sums)


class HeadTailCase:
    """BnCase followed by the 1x1 head: logits = head_w . zq + bias (fp32) with zq = z as it would have been stored in the tensor
    dtype, never written.  Backward takes dlogits: dz = dlogits . head_w, and yields dhead_w = sum dlogits (x) zq, dhead_b = sum dlogits
    beside the BatchNorm sums and dy.  head_w, bias: wide integers; dlogits: dense +-1, so |dz| <= 15 ncls is exact in bf16 (the
    kernels round dz to the tensor dtype as the unfused path stores it: nothing to round here, asserted).  w_family "ternary": a
    head_w in {-1, 0, 1}, where the sums are to be used as dgamma / dbeta of an exact dy (the in-kernel finalize)."""

    def __init__(self, B, H, W, C, ncls, w_family="wide"):
        g = torch.Generator().manual_seed(_seed(B, H, W, C, ncls, 61, w_family == "wide"))
        self.shape, self.ncls, self.npix = (B, H, W, C), ncls, B * H * W
        self.y = wide((B, C, H, W), g)
        self.head_w = wide((ncls, C, 1, 1), g) if w_family == "wide" else ternary((ncls, C, 1, 1), 0.5, g)
        self.head_b = wide((ncls,), g)
        self.dlogits = ternary((B, ncls, H, W), 1.0, g)
        self.scale, self.shift, self.mean, self.rstd = dyadic_coeffs(C, g)
        self.dgamma, self.dbeta = given_sums(C, g)
        self.z, _ = relu_and_mask(self.y.double(), self.scale, self.shift, torch.zeros(B, C, H, W, dtype=torch.float64))
        self._refs = {}

    def coeffs(self):
        return self.scale, self.shift, self.mean, self.rstd

    def refs(self, dtype):
        if dtype in self._refs:
            return self._refs[dtype]
        y, w, b, dl = self.y.double(), self.head_w.double(), self.head_b.double(), self.dlogits.double()
        zq = expected(self.z, dtype).double().requires_grad_(True)
        wl, bl = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
        logits = F.conv2d(zq, wl, bl)
        dz, dhw, dhb = torch.autograd.grad(logits, [zq, wl, bl], dl)
        zq = zq.detach()
        # logits: C products zq w and the bias, in quarters; dhead_w: one product per pixel, in quarters; dhead_b: +-1 per pixel
        require_exact_sum(torch.cat([zq.unsqueeze(1) * w.view(1, -1, zq.shape[1], 1, 1), b.view(1, -1, 1, 1, 1).expand(zq.shape[0], -1, 1, *zq.shape[2:])], 2),
                          0.25, 2, "HeadTailCase: logits")
        require_exact_sum(dl.unsqueeze(2) * zq.unsqueeze(1), 0.25, (0, 3, 4), "HeadTailCase: dhead_w")
        assert self.npix < F32_INT and float(dz.abs().max()) <= BF16_INT
        _, m = relu_and_mask(y, self.scale, self.shift, dz)
        _, sum1, sum2 = bn_sums(m, y, self.mean, self.rstd, "HeadTailCase")
        r = dict(zq=zq, logits=logits.detach(), dz=dz, m=m, dhead_w=dhw.view(self.ncls, -1), dhead_b=dhb, sum1=sum1, sum2=sum2)
        r["dy"] = bn_dy(m, y, self.scale, self.mean, self.rstd, self.dgamma, self.dbeta, N_TOTAL, 1.0, "HeadTailCase, given sums")
        if is_pow2(self.npix):
            r["own_dy"] = bn_dy(m, y, self.scale, self.mean, self.rstd, sum2, sum1, self.npix, 0.25, "HeadTailCase, own sums")
        self._refs[dtype] = r
        return r


@functools.lru_cache(maxsize=4)
def head_tail_case(B, H, W, C, ncls, w_family="wide"):
    return HeadTailCase(B, H, W, C, ncls, w_family)


STEM_C = 64
STEM_UNIT = 256.0              # dgamma, dbeta of the stem: integers that are multiples of N_TOTAL / 4, so dgamma / n is in quarters


def stem_dy(m, yq, scale, mean, rstd, dgamma, dbeta, n):
    """The stem's dy = scale (m - dbeta / n - xhat dgamma / n), float64, BEFORE its rounding to bf16; the terms checked as in bn_dy
    with the narrow coefficients' quanta: scale, rstd >= 1, mean an integer, dgamma / n and dbeta / n in quarters -> q = 1/4."""
    b = _cv(scale * rstd * dgamma / n)
    terms = torch.stack([(_cv(scale) * m).abs(), (_cv(scale * dbeta / n)).abs().expand_as(m), (b * yq).abs(), (b * _cv(mean)).abs().expand_as(m)])
    require_exact_sum(terms, 0.25, 0, "StemCase: dy")
    xhat = (yq - _cv(mean)) * _cv(rstd)
    return _cv(scale) * (m - _cv(dbeta) / n - xhat * _cv(dgamma) / n)


def stem_dw(dyq, x):
    """dw [64, 1, 3, 3] = sum over pixels of dyq (x) x (the filter gradient of a padded 3x3 conv), float64."""
    w0 = torch.zeros(STEM_C, 1, 3, 3, dtype=torch.float64, requires_grad=True)
    (dw,) = torch.autograd.grad(F.conv2d(x, w0, padding=1), [w0], dyq)
    return dw


class StemCase:
    """The recomputed stem: x [B,1,H,W] and w [64,1,3,3] hold integers, y = conv(x, w) is exact in fp32 and the kernel rounds it to
    bf16 BY DESIGN (as the stored path stores it): yq = to_bf16(y), the reference rounds in the same place.  Then as BnCase on yq;
    dy is rounded to bf16 before dw = sum dy (x) x, again by design and again in the reference.
      "ternary"  x, w in {-1, 0, 1}: |y| <= 9, no rounding occurs; dz wide, the full coefficient set for z and the sums.
      "wide"     x, w in [-15, 15]: |y| up to 2025, the rounding of y is exercised; dz ternary.
    The sums run over every pixel of the image, so the inputs are narrowed with the pixel count until the conditions hold
    (asserted, never assumed): dz gets sparser, and the backward-weights half uses the narrow coefficient set (dyadic_coeffs) with
    dgamma, dbeta multiples of STEM_UNIT = N_TOTAL / 4 -- dy is then in quarters, and sum |dyq x| * 4 < 2^24 per filter element.
    Where even that fails dgamma, dbeta shrink to one unit, then (the wide family on a large image: |xhat| ~ 500 on every pixel) to 0:
    dy = scale m is then as sparse as dz; the small shapes keep the xhat term."""

    def __init__(self, B, H, W, family):
        g = torch.Generator().manual_seed(_seed(B, H, W, 67, family == "wide"))
        self.shape, self.family, self.npix = (B, H, W), family, B * H * W
        n = self.npix
        if family == "ternary":
            self.x, self.w = ternary((B, 1, H, W), 0.75, g), ternary((STEM_C, 1, 3, 3), 0.75, g)
            self.dz = wide((B, STEM_C, H, W), g) if n <= 4096 else ternary((B, STEM_C, H, W), min(1.0, 65536.0 / n), g)
        elif family == "wide":
            self.x, self.w = wide((B, 1, H, W), g), wide((STEM_C, 1, 3, 3), g)
            self.dz = ternary((B, STEM_C, H, W), min(1.0, 1024.0 / n), g)
        else:
            raise ValueError(family)
        x, w, dz = self.x.double(), self.w.double(), self.dz.double()
        self.y = F.conv2d(x, w, padding=1)
        assert float(self.y.abs().max()) < F32_INT
        self.yq = to_bf16(self.y).double()
        if family == "ternary":
            assert torch.equal(self.yq, self.y)
        else:
            # |y| has a standard deviation of 3 * 80: about a third lies past 256, where every second integer or more is rounded
            assert float((self.yq != self.y).double().mean()) > 0.1, "the wide family must exercise the rounding of y"
        # forward and the BatchNorm sums: the full coefficient set
        self.scale, self.shift, self.mean, self.rstd = dyadic_coeffs(STEM_C, g)
        self.z, self.m = relu_and_mask(self.yq, self.scale, self.shift, dz)
        assert bool((self.z > 0).any()) and (family == "wide" or bool((self.z == 0).any()))
        _, self.sum1, self.sum2 = bn_sums(self.m, self.yq, self.mean, self.rstd, "StemCase")
        # backward-weights: the narrow set
        self.wg_scale, self.wg_shift, self.wg_mean, self.wg_rstd = dyadic_coeffs(STEM_C, g, narrow=True)
        self.dgamma, self.dbeta = given_sums(STEM_C, g, STEM_UNIT)
        _, mw = relu_and_mask(self.yq, self.wg_scale, self.wg_shift, dz)
        for attempt in (0, 1, 2):
            self.dy = stem_dy(mw, self.yq, self.wg_scale, self.wg_mean, self.wg_rstd, self.dgamma, self.dbeta, N_TOTAL)
            self.dyq = to_bf16(self.dy).double()
            xw = F.unfold(x, 3, padding=1).view(B, 1, 9, H, W)                # the nine shifted images
            budget = float(torch.einsum("bchw,bkhw->ck", self.dyq.abs() * 4, xw[:, 0].abs()).max())
            if budget < F32_INT:
                break
            assert attempt < 2, f"StemCase: sum |dyq x| * 4 = {budget} reaches 2^24 even with dy = scale m"
            if attempt == 0:                                                  # one unit at the most, then none
                self.dgamma, self.dbeta = self.dgamma.sign() * STEM_UNIT, self.dbeta.sign() * STEM_UNIT
            else:
                self.dgamma, self.dbeta = torch.zeros(STEM_C, dtype=torch.float64), torch.zeros(STEM_C, dtype=torch.float64)
        t = self.dyq * 4
        assert torch.equal(t, t.round())
        self.dw = stem_dw(self.dyq, x)
        assert bool((self.dw != 0).any())

    def coeffs(self):
        return self.scale, self.shift, self.mean, self.rstd

    def wg_coeffs(self):
        return self.wg_scale, self.wg_shift, self.wg_mean, self.wg_rstd


@functools.lru_cache(maxsize=4)
def stem_case(B, H, W, family):
    return StemCase(B, H, W, family)


# ------------------------------------------------------------------------------------------------ spatial attention
# csrc/spatial_attn.hip: channel mean / max / first maximal channel, a k x k correlation of those two maps under a sigmoid, the gate
# y = x a, and their backward.  x holds wide integers and w is dyadic (the integers +-1 .. +-k^2, each once, times a power of two:
# every tap distinct), so the maximum, its channel, the channel sum, every correlation of the backward and the filter gradient have
# ONE right value; the mean is one float32 division of an exact sum.  Only the map itself holds an expf and a division.
SA_TH, SA_TW, SA_DW_BLOCKS = 8, 32, 1024       # the LDS tile of the k x k passes; the most workgroups the filter gradient is dealt to
SA_A_VALUES = (0.125, 0.25, 0.5, 0.75, 0.875)  # the synthetic map of the backward cases: a, 1 - a and a (1 - a) are exact in a few bits
SA_Q_GS = 1.0 / 64                             # quantum of g_s = d a (1 - a) with an integer d
SA_Q_W = 1.0 / 64                              # quantum of the backward cases' w
SA_D_MAX = 256                                 # |sum_c x dy| of the gate's backward: g_s then needs 9 + 6 bits
SA_ACC_UNITS = 4.0                             # the most an inexact accumulator of the map may be off, in units of 2^-24 (SaFwdCase)
SA_PLANTS = 7                               # pixel p holds plant p % 7: none, tie of two, tie of three, all equal, all negative, all zero, none


def sa_taps(k, g):
    """[1,2,k,k] float64: the integers 1 .. k^2 and their negatives, each once, in a seeded order (six bits and a sign at k = 7)."""
    kk = k * k
    v = torch.cat([torch.arange(1, kk + 1), -torch.arange(1, kk + 1)]).double()
    w = v[torch.randperm(2 * kk, generator=g)].view(1, 2, k, k)
    assert len(torch.unique(w)) == 2 * kk
    return w


def sa_first_max(x):
    """x [B,C,H,W] (no NaN) -> the channel maximum [B,H,W] and the FIRST channel that holds it (int64), without relying on how a
    library breaks ties."""
    m = x.max(dim=1, keepdim=True).values
    first = ((x == m).cumsum(1) == 0).sum(1)
    return m[:, 0], first


def sa_last_max(x):
    m = x.max(dim=1, keepdim=True).values
    return x.shape[1] - 1 - ((x == m).flip(1).cumsum(1) == 0).sum(1)


def sa_mean32(x, drop=None):
    """The kernel's mean: the exact integer channel sum divided ONCE in float32 by float(C).  drop: a channel left out (a mutant)."""
    C = x.shape[1]
    s = x.double().sum(1)
    if drop is not None:
        s = s - x[:, drop].double()
    assert float(s.abs().max()) < F32_INT
    return s.float() / torch.tensor(float(C), dtype=torch.float32)


def sa_logits(pool, w):
    """pool [B,2,H,W], w [1,2,k,k] (float64) -> [B,H,W]: the k x k correlation with zero padding k // 2."""
    return F.conv2d(pool, w, padding=w.shape[-1] // 2)[:, 0]


def sa_gate(x_nhwc, a, dtype):
    """y = x a: ONE float32 product (x is exact in float32, a is the float32 map [B,H,W]) rounded once to the tensor dtype."""
    y = x_nhwc.float() * a.float().unsqueeze(-1)
    return y.bfloat16() if dtype == torch.bfloat16 else y


def sa_tile_of(B, H, W):
    """[B,H,W] int64: the index of the SA_TH x SA_TW tile a pixel lies in, in the order the filter gradient deals them out."""
    ty, tx = (H + SA_TH - 1) // SA_TH, (W + SA_TW - 1) // SA_TW
    t = (torch.arange(H) // SA_TH).view(1, H, 1) * tx + (torch.arange(W) // SA_TW).view(1, 1, W)
    return t + torch.arange(B).view(B, 1, 1) * (ty * tx)


def sa_tiles(B, H, W):
    return B * ((H + SA_TH - 1) // SA_TH) * ((W + SA_TW - 1) // SA_TW)


class SaFwdCase:
    """uh_spatial_attn_fwd on x [B,C,H,W] of wide integers with planted pixels (SA_PLANTS) and w = sa_taps * 2^-shift.
    Exact, float32: mean (sa_mean32), max, amax (the first maximal channel).  pool = [mean, max] as float64 [B,2,H,W].
    a64 = sigmoid(correlation) in float64 on that pool; the shift is the smallest that leaves 90 % of the pixels of a64 inside
    (0.02, 0.98) (asserted).  Where C is a power of two the mean is exact and every term of the correlation is a multiple of
    2^-shift / C with an absolute sum below 2^24 of them (asserted): the kernel's accumulator is then exact in any order and its map
    differs from a64 by its sigmoid alone.  For other C the mean is a rounded quotient and the accumulator rounds: the GPU test forms
    the float64 map from the pool the kernel returned (checked bit for bit first) through `a_from_pool`, and the shift grows until
    2 k^2 max_p sum |w| |pool| <= SA_ACC_UNITS: the accumulator's 2 k^2 roundings, each at most 2^-24 of a partial sum that never
    exceeds sum |w| |pool|, then move the map's argument by at most 4 * 2^-24 -- and a by no more, relatively (d ln a = (1 - a) dz).
    That map is flat (|z| < 0.05); the wide range of the sigmoid is the business of the power-of-two cases, and the map kernel
    never sees C."""

    def __init__(self, B, H, W, C, k):
        g = torch.Generator().manual_seed(_seed(B, H, W, C, k, 71))
        self.shape, self.k, self.npix = (B, H, W, C), k, B * H * W
        x = wide((B, C, H, W), g)
        plant = (torch.arange(self.npix).view(B, 1, H, W) % SA_PLANTS).expand(B, C, H, W)
        ch = torch.arange(C).view(1, C, 1, 1).expand(B, C, H, W)
        x = torch.where((plant == 1) | (plant == 2) | (plant == 6), x.clamp(max=WIDE_MAX - 1), x)      # the planted channels alone hold the maximum
        x = torch.where((plant == 6) & (ch == C - 1), torch.tensor(float(WIDE_MAX)), x)
        if C >= 2:
            x = torch.where((plant == 1) & ((ch == C // 3) | (ch == C - 1)), torch.tensor(float(WIDE_MAX)), x)
        if C >= 3:
            x = torch.where((plant == 2) & ((ch == C // 4) | (ch == C // 2) | (ch == C - 1)), torch.tensor(float(WIDE_MAX)), x)
        x = torch.where(plant == 3, wide((B, 1, H, W), g).expand(B, C, H, W), x)
        x = torch.where(plant == 4, -1.0 - wide((B, C, H, W), g).abs().clamp(max=WIDE_MAX - 1), x)
        x = torch.where(plant == 5, torch.zeros(()), x)
        self.x = x.contiguous()
        xd = self.x.double()
        self.max, self.amax = sa_first_max(xd)
        self.mean32 = sa_mean32(self.x)
        self.pool = torch.stack([self.mean32.double(), self.max], 1)
        if self.npix >= 2 * SA_PLANTS:
            ties = (xd == self.max.unsqueeze(1)).sum(1)
            assert bool((ties == 2).any()) or C < 3
            assert bool((ties == 3).any()) or C < 4
            assert bool((self.max < 0).any()) and bool(((xd == 0).all(1)).any()) and bool((ties == C).any())
            assert bool((self.amax == 0).any()) and (C < 4 or bool((self.amax == C // 4).any())) and bool((self.amax == C - 1).any())
        taps = sa_taps(k, g)
        self.exact_acc = is_pow2(C)
        for shift in range(0, 40):
            self.w = taps * 2.0 ** -shift
            self.a64 = torch.sigmoid(sa_logits(self.pool, self.w))
            self.unsaturated = float(((self.a64 > 0.02) & (self.a64 < 0.98)).double().mean())
            # the roundings of an accumulator that is NOT exact: 2 k^2 additions, each off by at most 2^-24 of a partial sum, and no
            # partial sum exceeds sum |w| |pool|
            self.acc_units = 0.0 if self.exact_acc else 2 * k * k * float(sa_logits(self.pool.abs(), self.w.abs()).max())
            if self.unsaturated >= 0.9 and self.acc_units <= SA_ACC_UNITS:
                break
        assert self.unsaturated >= 0.9, f"SaFwdCase: only {self.unsaturated:.2f} of the map lies inside (0.02, 0.98)"
        assert self.acc_units <= SA_ACC_UNITS
        self.shift = shift
        if self.exact_acc:
            assert torch.equal(self.mean32.double(), xd.mean(1))
            # per pixel sum |w| |pool| = the correlation of the absolute values: ONE stacked term whose size is the sum of all 2 k^2
            q = 2.0 ** -shift / C
            assert torch.equal(self.pool / (1.0 / C), (self.pool / (1.0 / C)).round())
            require_exact_sum(sa_logits(self.pool.abs(), self.w.abs()).unsqueeze(0), q, 0, "SaFwdCase: the correlation")

    def a_from_pool(self, pool_bhw2):
        """float64 map from a float32 pool [B,H,W,2] as the kernel returned it."""
        return torch.sigmoid(sa_logits(pool_bhw2.double().permute(0, 3, 1, 2), self.w))


@functools.lru_cache(maxsize=64)
def sa_fwd_case(B, H, W, C, k):
    return SaFwdCase(B, H, W, C, k)


def sa_gpool(gs, w):
    """g_pool [B,2,H,W] = the transposed correlation of g_s [B,H,W] with w [1,2,k,k]: the adjoint of sa_logits."""
    return F.conv_transpose2d(gs.unsqueeze(1), w, padding=w.shape[-1] // 2)


def sa_dw(gs, pool, k):
    """dw [1,2,k,k] = sum_p g_s[p] pool[p + (r - P, s - P)]: the filter gradient of sa_logits, by stock autograd."""
    w0 = torch.zeros(1, 2, k, k, dtype=torch.float64, requires_grad=True)
    (dw,) = torch.autograd.grad(F.conv2d(pool, w0, padding=k // 2), [w0], gs.unsqueeze(1))
    return dw


def sa_dx64(dya, gpool, amax, C):
    """dx = dy a + g_avg / C + [c == amax] g_max in float64; dya [B,C,H,W] or None (the map's backward)."""
    hot = torch.arange(C).view(1, C, 1, 1) == amax.unsqueeze(1)
    base = gpool[:, 0:1] / C + hot * gpool[:, 1:2]
    return base if dya is None else dya + base


def sa_dx32(dya, gpool, amax, C, divide=True):
    """The kernel's last three operations in float32, everything before them in float64: g_avg / C is one division, dy a + that one
    rounding (dy a is exact, so a fused multiply-add gives the same bits), + g_max at the argmax channel one more.  -> float32."""
    gavg = gpool[:, 0:1].float()
    if divide:
        gavg = gavg / torch.tensor(float(C), dtype=torch.float32)
    t = gavg.expand(-1, C, -1, -1) if dya is None else dya.float() + gavg
    hot = torch.arange(C).view(1, C, 1, 1) == amax.unsqueeze(1)
    return torch.where(hot, t + gpool[:, 1:2].float(), t)


class SaBwdCase:
    """uh_spatial_attn_bwd with SYNTHETIC forward results (the call takes pool, amax and a as inputs): a from SA_A_VALUES, pool
    integers in [-7, 7], amax any channel (0 and C - 1 forced), x wide, w = sa_taps / 64.
      mode "gate": dy ternary of a density that keeps d = sum_c x dy within +-256 (asserted); mode "map": d = ga, ternary per pixel.
      g_s = d a (1 - a): an integer of 9 bits times 64ths -- exact.  g_pool and dw: every term a multiple of 2^-12 resp. 2^-6 with an
      absolute sum below 2^24 of them (asserted with require_exact_sum on the sums of absolute terms): exact in any order.
      dx: sa_dx32, asserted equal to pure float64 where C is a power of two (every value is then exact).
    p: density of dy / ga (None: 24 / C for the gate, 1/2 for the map); a_half: a = 1/2 everywhere; plant_tiles: force a non-zero ga
    into every tile from that index on (the filter gradient's second round)."""

    def __init__(self, B, H, W, C, k, mode, p=None, a_half=False, plant_tiles=None):
        assert mode in ("gate", "map")
        g = torch.Generator().manual_seed(_seed(B, H, W, C, k, 73, mode == "gate"))
        self.shape, self.k, self.mode, self.npix = (B, H, W, C), k, mode, B * H * W
        P = k // 2
        self.a = torch.tensor(SA_A_VALUES, dtype=torch.float64)[torch.randint(0, len(SA_A_VALUES), (B, H, W), generator=g)]
        if a_half:
            self.a = torch.full((B, H, W), 0.5, dtype=torch.float64)
        self.pool = torch.randint(-7, 8, (B, 2, H, W), generator=g).double()
        self.amax = torch.randint(0, C, (B, H, W), generator=g)
        self.amax.view(-1)[0] = C - 1
        self.amax.view(-1)[-1] = 0
        self.w = sa_taps(k, g) * SA_Q_W
        self.x = wide((B, C, H, W), g)
        if mode == "gate":
            self.dy = ternary((B, C, H, W), min(1.0, 24.0 / C) if p is None else p, g)
            self.ga = None
            terms = self.x.double() * self.dy.double()
            require_exact_sum(terms, 1.0, 1, "SaBwdCase: sum_c x dy")
            self.d = terms.sum(1)
            assert float(self.d.abs().max()) <= SA_D_MAX, f"SaBwdCase: |sum_c x dy| = {float(self.d.abs().max())} > {SA_D_MAX}"
            dya = self.dy.double() * self.a.unsqueeze(1)
        else:
            self.dy = None
            self.ga = ternary((B, H, W), 0.5 if p is None else p, g)
            if plant_tiles is not None:
                tile = sa_tile_of(B, H, W)
                for t in range(plant_tiles, sa_tiles(B, H, W)):
                    at = (tile == t).nonzero()[0]
                    self.ga[tuple(at.tolist())] = 1.0 if t % 2 else -1.0
            self.d = self.ga.double()
            dya = None
        assert bool((self.d != 0).any())
        self.gs = self.d * self.a * (1 - self.a)
        assert torch.equal(self.gs / SA_Q_GS, (self.gs / SA_Q_GS).round()) and torch.equal(self.gs.float().double(), self.gs)
        assert torch.equal(self.w / SA_Q_W, (self.w / SA_Q_W).round())
        # the sums of absolute terms, formed as the same contractions of the absolute values: one stacked term each
        require_exact_sum(sa_gpool(self.gs.abs(), self.w.abs()).unsqueeze(0), SA_Q_GS * SA_Q_W, 0, "SaBwdCase: g_pool")
        require_exact_sum(sa_dw(self.gs.abs(), self.pool.abs(), k).unsqueeze(0), SA_Q_GS, 0, "SaBwdCase: dw")
        self.gpool = sa_gpool(self.gs, self.w)
        self.dw = sa_dw(self.gs, self.pool, k)
        assert bool((self.dw != 0).any()) and bool((self.gpool != 0).any())
        self.dx64 = sa_dx64(dya, self.gpool, self.amax, C)
        self.dx = sa_dx32(dya, self.gpool, self.amax, C)
        self.dya = dya
        if is_pow2(C):
            terms = [self.gpool[:, 0:1].expand(-1, C, -1, -1) / C, self.gpool[:, 1:2].expand(-1, C, -1, -1)]
            if dya is not None:
                terms.append(dya)
            require_exact_sum(torch.stack(terms), SA_Q_GS * SA_Q_W / C, 0, "SaBwdCase: dx")
            assert torch.equal(self.dx.double(), self.dx64), "the float32 restatement of dx must BE float64 where C is a power of two"

    def ws(self):
        """The workspace as the kernel leaves it: g_pool [npix][2], then g_s [npix]; float32."""
        return torch.cat([self.gpool.permute(0, 2, 3, 1).reshape(-1), self.gs.reshape(-1)]).float()


@functools.lru_cache(maxsize=128)
def sa_bwd_case(B, H, W, C, k, mode, p=None, a_half=False, plant_tiles=None):
    return SaBwdCase(B, H, W, C, k, mode, p, a_half, plant_tiles)
