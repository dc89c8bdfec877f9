"""Inputs on which the matrix-pipe kernels have ONE right answer, and the comparator that holds them to it.  CPU only.

The conv / transposed-conv / 1x1 kernels accumulate in fp32.  Where every product and every partial sum is an integer (or an
integer times one fixed power of two) below 2^24, fp32 addition is exact in ANY order, so the result equals the float64 reference
bit for bit: no tolerance, and a missing, doubled or misplaced term, or an intermediate kept in fewer bits, changes the output.

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
