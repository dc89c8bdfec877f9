"""Cases, exact references, derived bounds, a float64 restatement and seeded mistakes shared by tests/test_gpu_bn_stats.py (the forward
BatchNorm statistics chain on the MI355X: uh_bn_finalize, uh_bn_finalize_ld, uh_bn_eval_coeffs and the statistics rows of the conv
kernels) and tests/test_bn_stats_cpu.py (the CPU proof that the references agree with float64 torch, that every family meets its
conditions at every shape and that each seeded mistake breaks a comparison).  Nothing here needs a GPU.

The buffer of csrc/bn.hip: [nslab][2][ldc] floats = per row (mean, M2) of the pixels the row covers, then [nslab] pixel counts.  Rows
with a zero count are dead: here they hold NaN.  Columns c >= C of a row (ldc > C) hold NaN as well.

Reference of the finalize (finalize_exact): the merge in exact rational arithmetic over the float32 row values,
    N = sum n_i,  mean = sum n_i m_i / N,  M2 = sum M2_i + sum n_i (m_i - mean)^2        (equal to p + A / N, S + Q - A^2 / N for any p),
then n = the caller's n (or N where it passes 0), var = M2 / n, unb = M2 / (n - 1) (var where n <= 1).

Two families of rows.
  "dyadic": every quantity is a dyadic rational with few bits, so that the kernel's double sums are exact in any order, its fp32
      products are exact (fp contraction cannot change a bit) and every output has one right answer: see dyadic_rows, which asserts
      each condition on the Fraction terms.  var + eps is 4, 1 or 1/4 (constant channels: eps = 2^-16 alone), so rstd is a power of two.
  "general": random fp32 rows, bounds derived in general_bounds.
"""
import collections
import math
import zlib
from fractions import Fraction as Fr

import numpy as np

F = np.float32
U = 2.0 ** -24                        # relative error of one rounding to float32
EPS64 = 2.0 ** -53                    # relative error of one rounding to float64
BNF_FAST = 1024                       # rows in the finalize's first batch (bn.hip: BNF_RL * BNF_MAXI)
CANARY = 12345.5
CANARY_NBT = 7777777


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def fr(x):
    """A float (float32 or float64 value) as an exact Fraction."""
    return Fr(float(x))


def is_f32(x):
    """Is the Fraction x a float32 number (normal range)?"""
    return x == 0 or fr(F(float(x))) == x and Fr(float(x)) == x


def round_f32(x):
    """The Fraction x rounded once to float32, to nearest even (normal range asserted): no trip through float64."""
    if x == 0:
        return F(0)
    a = abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length()          # 2^(e-1) < a < 2^(e+1)
    if Fr(2) ** e > a:
        e -= 1
    assert Fr(2) ** e <= a < Fr(2) ** (e + 1) and -126 <= e <= 127
    q = a / Fr(2) ** (e - 23)                                           # in [2^23, 2^24)
    fl = q.numerator // q.denominator
    rem = q - fl
    if rem > Fr(1, 2) or (rem == Fr(1, 2) and fl % 2 == 1):
        fl += 1
    v = Fr(fl) * Fr(2) ** (e - 23)
    out = F(float(v))
    assert fr(out) == v
    return out if x > 0 else F(-out)


def exact_in_double(x):
    return Fr(float(x)) == x


# ------------------------------------------------------------------------------------------------ finalize: the cases
FinCase = collections.namedtuple("FinCase", "name nslab C ldc dead n_mode eps momentum null")
NSLABS = (1, 2, 63, 64, 65, 1023, 1024, 1025, 2048, 2500)
CHANNELS = (1, 3, 4, 5, 64, 130)
PITCHED = ((3, 64), (16, 64), (67, 128))
N_MODES = ("counted", "zero", "twice", "one")
OPTIONAL = ("running_mean", "running_var", "num_batches_tracked", "m2_out")
EPS_DYADIC = 2.0 ** -16


def _fin(name, nslab, C, ldc=None, dead="none", n_mode="counted", eps=None, momentum=None, null=None):
    return FinCase(name, nslab, C, ldc if ldc is not None else C, dead, n_mode, eps, momentum, null)


FIN_CASES = (
    [_fin(f"rows{r}-{d}", r, 5, dead=d) for r in NSLABS for d in ("none", "scattered") if not (d == "scattered" and r == 1)] +
    [_fin(f"rows{r}-first_dead", r, 5, dead="first") for r in (2, 65, 1025, 2500)] +
    [_fin(f"rows{r}-{d}", r, 5, dead=d) for r in (1025, 2048, 2500) for d in ("tail", "head")] +
    [_fin(f"C{c}-rows{r}", r, c, dead="scattered") for c in CHANNELS for r in (65, 1025)] +
    [_fin(f"C{c}-ldc{l}-rows{r}", r, c, ldc=l, dead="scattered") for c, l in PITCHED for r in (2, 65, 1025)] +
    [_fin(f"n_{m}-rows{r}", r, 5, dead="scattered", n_mode=m) for m in N_MODES[1:] for r in (1, 65, 1025, 2500)
     if not (r == 1 and m != "one")] +
    [_fin("one_pixel", 1, 3, n_mode="one")] +
    [_fin(f"syncbn-world{w}-{m}", w, 64, n_mode=m) for w in (2, 8) for m in ("counted", "twice")] +
    [_fin(f"null-{p}", 65, 5, dead="scattered", null=p) for p in OPTIONAL] +
    [_fin("eps0", 65, 5, dead="scattered", eps=0.0), _fin("momentum_half", 65, 5, dead="scattered", momentum=0.5)])
FIN_BY_NAME = {c.name: c for c in FIN_CASES}
assert len(FIN_BY_NAME) == len(FIN_CASES)
NBT_CASES = ("C1-rows65", "C130-rows65", "C130-rows1025")


def dead_mask(case, rng):
    n, d = case.nslab, case.dead
    m = np.zeros(n, bool)
    if d == "scattered":
        m = rng.random(n) < 0.3
        if n > 1:
            m[0], m[n - 1] = False, True                               # the first row stays the pivot; the last row is dead
        if n > 3:
            m[n // 2] = True
    elif d == "first":
        m[0] = True
        if n > 4:
            m[3] = True
    elif d == "tail":
        m[BNF_FAST:] = True
    elif d == "head":
        m[:BNF_FAST] = True
    assert not m.all()
    return m


def _counts(case, rng, dead, total_pow2):
    """Pixel counts: 1 .. 256 per live row (what a 16 x 16 tile holds); dyadic family: rows come in (a, b) pairs with the same
    count (dyadic_rows gives them opposite offsets), and one or two rows without a partner absorb what is missing to a power of two."""
    n = case.nslab
    live = np.flatnonzero(~dead)
    cnt = np.zeros(n, np.int64)
    if not total_pow2:
        cnt[live] = rng.integers(1, 257, len(live))
        if case.name == "one_pixel":
            cnt[live] = 1
        return cnt, None
    if case.name == "one_pixel":
        cnt[live] = 1
        return cnt, np.zeros((0, 2), np.int64)
    nabs = 1 if len(live) % 2 == 1 else 2
    body, absorb = live[nabs:], live[:nabs]                    # (the rows behind the first 1024 are pairs: they carry offsets)
    pairs = body.reshape(-1, 2)
    c = rng.integers(1, 257, len(pairs))
    cnt[pairs[:, 0]], cnt[pairs[:, 1]] = c, c
    used = int(cnt.sum())
    total = 1 << max(4, (used + nabs).bit_length())
    rest = total - used
    if nabs == 1:
        cnt[absorb[0]] = rest
    else:
        cnt[absorb[0]] = rest // 4 * 3
        cnt[absorb[1]] = rest - rest // 4 * 3
    assert int(cnt.sum()) == total and total & (total - 1) == 0 and total < 2 ** 24 and (cnt[live] > 0).all()
    return cnt, pairs


def n_param(case, N):
    """-> (the n the caller passes, the n the kernel divides by)."""
    return {"counted": (N, N), "zero": (0, N), "twice": (2 * N, 2 * N), "one": (1, 1)}[case.n_mode]


def _top_bits(x, bits):
    """The largest Fraction <= x (x > 0) with `bits` significant bits."""
    e = x.numerator.bit_length() - x.denominator.bit_length()
    if Fr(2) ** e > x:
        e -= 1
    q = Fr(2) ** (e - bits + 1)
    return (x / q).numerator // (x / q).denominator * q


def _sums_exact_in_double(terms):
    """Sufficient for a double sum to be exact in ANY order: every term is a multiple of q = 2^-g and sum |terms| < 2^53 q."""
    g = max(t.denominator for t in terms)
    assert g & (g - 1) == 0
    return sum(abs(t) for t in terms) * g < 2 ** 53


def dyadic_rows(case):
    """-> inputs dict of the dyadic family (see the module docstring).  Per channel c: base mean b_c (a multiple of 1/16), the live
    rows' means b_c + k / 16 with k in -4 .. 4 and sum n_i k_i = 0 (pairs of equal counts and opposite k), so mean = b_c exactly and
    B = sum n_i (m_i - mean)^2 is a multiple of 2^-8; sum M2_i = n (T_c - eps) - B with T_c in (4, 1, 1/4), split over the live rows
    in float32 pieces.  Every fifth channel (c % 5 == 4) is constant: k = 0 and M2 = 0, so M2 = 0 and rstd = 1 / sqrt(eps) = 256."""
    rng = np.random.default_rng(_seed("dyadic", case.name))
    nslab, C = case.nslab, case.C
    eps = EPS_DYADIC if case.eps is None else case.eps
    mom = 0.25 if case.momentum is None else case.momentum
    dead = dead_mask(case, rng)
    cnt, pairs = _counts(case, rng, dead, True)
    live = np.flatnonzero(~dead)
    N = int(cnt.sum())
    n_pass, n_eff = n_param(case, N)
    mean = np.full((nslab, C), np.nan, F)
    m2 = np.full((nslab, C), np.nan, F)
    for c in range(C):
        T = (Fr(4), Fr(1), Fr(1, 4))[c % 3]
        const = c % 5 == 4 and eps > 0
        base = Fr(int(rng.integers(-128, 129)), 16)
        k = np.zeros(nslab, np.int64)
        if not const and case.n_mode != "one" and len(pairs):
            kk = rng.integers(-4, 5, len(pairs))
            k[pairs[:, 0]], k[pairs[:, 1]] = kk, -kk
        assert int((cnt * k).sum()) == 0
        for i in live:
            mean[i, c] = F(float(base + Fr(int(k[i]), 16)))
        Bq = sum(Fr(int(cnt[i])) * Fr(int(k[i]), 16) ** 2 for i in live)
        rest = Fr(0) if const else Fr(n_eff) * (T - fr(F(eps))) - Bq
        assert rest >= 0
        if not const:
            avg = rest / len(live)
            for j, i in enumerate(live):
                left = len(live) - j
                if left <= 3:
                    piece = _top_bits(rest, 24) if rest > 0 else Fr(0)
                else:
                    piece = min(rest, _top_bits(avg * Fr(int(rng.integers(1, 97)), 64), 12))
                m2[i, c] = F(float(piece))
                assert fr(m2[i, c]) == piece
                rest -= piece
            assert rest == 0, "the M2 of the channel does not split into float32 rows"
        else:
            m2[live, c] = 0
    g = rng.integers(-32, 33, C)
    g[g == 0] = 8
    inputs = dict(mean=mean, m2=m2, counts=cnt.astype(F), n_pass=n_pass, n_eff=n_eff, eps=F(eps), momentum=F(mom),
                  gamma=(g / 8).astype(F), beta=(rng.integers(-32, 33, C) / 8).astype(F),
                  running_mean=(rng.integers(-64, 65, C) / 16).astype(F), running_var=(rng.integers(1, 65, C) / 16).astype(F))
    return inputs


def general_rows(case):
    """Random fp32 rows.  Channel c has the population (mu, sd) of GENERAL[c % 4] -- one of them mean 1e4, standard deviation 0.1 --
    unless the first row is dead: then the kernel's pivot is 0, Q = sum n_i m_i^2 and M2 = S + Q - A^2 / N cancels in double by
    (mu / sd)^2, which the derived bound would have to carry; those cases keep |mu| / sd <= 10 (general_bounds asserts that the
    double term is negligible, whatever the case)."""
    rng = np.random.default_rng(_seed("general", case.name))
    nslab, C = case.nslab, case.C
    dead = dead_mask(case, rng)
    cnt, _ = _counts(case, rng, dead, False)
    table = GENERAL_PIVOT0 if dead[0] else GENERAL
    mean = np.full((nslab, C), np.nan, F)
    m2 = np.full((nslab, C), np.nan, F)
    live = ~dead
    nl = int(live.sum())
    for c in range(C):
        mu, sd = table[c % 4]
        mean[live, c] = (mu + sd * rng.standard_normal(nl) / np.sqrt(cnt[live])).astype(F)
        m2[live, c] = (sd * sd * (cnt[live] - 1) * (0.5 + rng.random(nl))).astype(F)
    N = int(cnt.sum())
    n_pass, n_eff = n_param(case, N)
    return dict(mean=mean, m2=m2, counts=cnt.astype(F), n_pass=n_pass, n_eff=n_eff, eps=F(1e-5 if case.eps is None else case.eps),
                momentum=F(0.1 if case.momentum is None else case.momentum),
                gamma=(rng.random(C) + 0.5).astype(F) * np.where(rng.random(C) < 0.25, -1, 1).astype(F),
                beta=(rng.standard_normal(C) * 0.2).astype(F), running_mean=(rng.standard_normal(C) * 0.1).astype(F),
                running_var=(rng.random(C) + 0.5).astype(F))


GENERAL = ((0.3, 1.0), (1.0e4, 0.1), (-7.0, 3.0), (250.0, 0.5))
GENERAL_PIVOT0 = ((0.3, 1.0), (1.0, 0.1), (-7.0, 3.0), (2.5, 0.5))
FAMILIES = {"dyadic": dyadic_rows, "general": general_rows}


def pack_stats(inp, ldc):
    """-> the float32 buffer [nslab][2][ldc] | [nslab] of bn.hip; columns >= C hold NaN."""
    mean, m2 = inp["mean"], inp["m2"]
    nslab, C = mean.shape
    rows = np.full((nslab, 2, ldc), np.nan, F)
    rows[:, 0, :C], rows[:, 1, :C] = mean, m2
    return np.concatenate([rows.reshape(-1), inp["counts"]])


# ------------------------------------------------------------------------------------------------ finalize: exact reference
def finalize_exact(inp):
    """Per channel the exact N, mean, M2 (Fractions), and the magnitudes of the kernel's own sums about ITS pivot (the first row's
    mean, 0 when that row is dead): SA = sum |n_i d_i|, S = sum M2_i, Q = sum n_i d_i^2, A."""
    mean, m2, cnt = inp["mean"], inp["m2"], inp["counts"]
    nslab, C = mean.shape
    live = [i for i in range(nslab) if cnt[i] > 0]
    ns = [Fr(int(cnt[i])) for i in live]
    N = sum(ns)
    out = []
    for c in range(C):
        ms = [fr(mean[i, c]) for i in live]
        m2s = [fr(m2[i, c]) for i in live]
        mu = sum(n * m for n, m in zip(ns, ms)) / N
        M2 = sum(m2s) + sum(n * (m - mu) ** 2 for n, m in zip(ns, ms))
        piv = fr(mean[0, c]) if cnt[0] > 0 else Fr(0)
        d = [m - piv for m in ms]
        A = sum(n * x for n, x in zip(ns, d))
        out.append(dict(N=N, mean=mu, M2=M2, piv=piv, A=A, SA=sum(abs(n * x) for n, x in zip(ns, d)), S=sum(m2s),
                        Q=sum(n * x * x for n, x in zip(ns, d)), terms=(ns, d, m2s)))
    return out


def assert_dyadic_conditions(inp, ex):
    """The conditions under which the kernel's arithmetic on the dyadic family is exact: double sums in any order, the quotients by
    powers of two, and every fp32 product and sum of the coefficient and running-statistics lines."""
    n_eff = inp["n_eff"]
    assert n_eff & (n_eff - 1) == 0
    eps, mom = fr(inp["eps"]), fr(inp["momentum"])
    assert is_f32(1 - mom)
    for c, e in enumerate(ex):
        ns, d, m2s = e["terms"]
        N = e["N"]
        assert N.denominator == 1 and N.numerator & (N.numerator - 1) == 0
        assert _sums_exact_in_double([n * x for n, x in zip(ns, d)]) and _sums_exact_in_double(m2s)
        assert _sums_exact_in_double([n * x * x for n, x in zip(ns, d)])
        assert all(exact_in_double(n * x) for n, x in zip(ns, d))                    # (nf * d, the first factor of the fma)
        A, S, Q = e["A"], e["S"], e["Q"]
        for v in (A * A, A * A / N, S + Q, S + Q - A * A / N, A / N, e["piv"] + A / N):
            assert exact_in_double(v)
        assert e["mean"] == e["piv"] + A / N and e["M2"] == S + Q - A * A / N and e["M2"] >= 0
        var = e["M2"] / n_eff
        assert exact_in_double(var) and var + eps in (Fr(4), Fr(1), Fr(1, 4), eps) and var + eps > 0
        r2 = 1 / (var + eps)
        rt = Fr(math.isqrt(r2.numerator), math.isqrt(r2.denominator))
        assert rt * rt == r2 and is_f32(rt)                                           # rstd is a power of two
        g, b = fr(inp["gamma"][c]), fr(inp["beta"][c])
        assert is_f32(e["mean"]) and is_f32(e["M2"]) and is_f32(g * rt) and is_f32(e["mean"] * g * rt)
        assert is_f32(b - e["mean"] * g * rt)
        rm = fr(inp["running_mean"][c])
        assert is_f32((1 - mom) * rm) and is_f32(mom * e["mean"]) and is_f32((1 - mom) * rm + mom * e["mean"])
        assert is_f32((1 - mom) * fr(inp["running_var"][c]))                          # (mom is a power of two: mom * unb is exact)
        assert mom.numerator == 1 and mom.denominator & (mom.denominator - 1) == 0


def unbiased_f32(M2, n_eff):
    """(float)(m2 / (n - 1)) as the kernel forms it: IEEE float64 division of the exact double m2, then one rounding to float32;
    var where n <= 1."""
    m2 = float(M2)
    assert Fr(m2) == M2
    return F(m2 / (n_eff - 1.0)) if n_eff > 1 else F(m2 / n_eff)


def dyadic_expected(inp, ex):
    """The one right answer of every output on the dyadic family (float32 arrays)."""
    n_eff, eps, mom = inp["n_eff"], fr(inp["eps"]), fr(inp["momentum"])
    C = len(ex)
    out = {k: np.zeros(C, F) for k in ("scale", "shift", "mean", "rstd", "m2_out", "running_mean", "running_var")}
    for c, e in enumerate(ex):
        r2 = 1 / (e["M2"] / n_eff + eps)
        rt = Fr(math.isqrt(r2.numerator), math.isqrt(r2.denominator))
        g, b = fr(inp["gamma"][c]), fr(inp["beta"][c])
        out["mean"][c], out["m2_out"][c], out["rstd"][c] = round_f32(e["mean"]), round_f32(e["M2"]), round_f32(rt)
        out["scale"][c] = round_f32(g * rt)
        out["shift"][c] = round_f32(b - e["mean"] * g * rt)
        out["running_mean"][c] = round_f32((1 - mom) * fr(inp["running_mean"][c]) + mom * e["mean"])
        unb = unbiased_f32(e["M2"], n_eff)
        out["running_var"][c] = round_f32((1 - mom) * fr(inp["running_var"][c]) + mom * fr(unb))
    return out


def general_bounds(inp, ex, nslab):
    """float64 values of the exact results and, per channel, the bound on each output of bn_finalize_kernel.  u = 2^-24, e = 2^-53.

    The merge in double.  A term of a sum passes at most L = 16 nb + 8 additions (nb = batches of 1024 rows: 16 per thread and batch,
    4 shuffle levels, 2 LDS adds, each block_sums result added once more), so |dA| <= L e SA, |dS| <= L e S, |dQ| <= (L + 2) e Q
    (the product nf * d and the fma round too).  mean = piv + A / N: |dmean| <= (L + 2) e (SA / N + |mean|) =: dbl_mean.
    A^2 / N: |d| <= 2 |A| |dA| / N + 2 e A^2 / N <= (2 L + 2) e Q  (|A| <= SA and SA^2 <= N Q by Cauchy-Schwarz), so
    |dM2| <= e ((L + 2) S + (3 L + 6) Q) <= (3 L + 6) e (S + Q) =: dbl_m2.   Both are asserted below to be under 1/16 of the one
    float32 rounding next to them: the merge is exact as far as float32 can see.
      mean_o  = fl32(mean):                         u |mean| + dbl_mean                                              =: e_mean
      m2_o    = fl32(m2):                           u M2 + dbl_m2
      rstd    = fl32(1 / sqrt(m2 / n + eps)):       u rstd + rstd (dbl_m2 / n) / (2 (var + eps)) + 4 e rstd          =: e_rstd
      scale   = fl32(g rstd):                       |g| e_rstd + u |g rstd|                                          =: e_scale
      shift   = fl32(bt - fl32(mean_o scale)) or fl32(fma(-mean_o, scale, bt)), as the compiler pleases: the error of the exact
                product mean_o scale is |mean| e_scale + |scale| e_mean + e_mean e_scale; the uncontracted form rounds the product
                (u |mean scale|) and both round the result (u (|bt| + |mean scale|) covers it): the bound of the uncontracted
                form covers both.
      running = fl32(fl32(om r) + fl32(mom x)) with om = fl32(1 - mom), or either product fused into the sum: four roundings at most
                (om, two products, the sum), each of at most u (|r| + |mom x|) up to second order, plus mom times the error of x:
                4 u (|r| + |mom x|) (1 + 2^-16) + mom e_x covers every contraction.  x = mean_o, or fl32(m2 / (n - 1)) with
                e_x = u unb + dbl_m2 / (n - 1) + 2 e unb.
    The formulas themselves are coefficient_bounds (part C carries the row bounds of part B through the same ones)."""
    n_eff, eps, mom = inp["n_eff"], float(inp["eps"]), float(inp["momentum"])
    nb = (nslab + BNF_FAST - 1) // BNF_FAST
    L = 16 * nb + 8
    C = len(ex)
    val = {k: np.zeros(C) for k in ("scale", "shift", "mean", "rstd", "m2_out", "running_mean", "running_var")}
    tol = {k: np.zeros(C) for k in val}
    for c, e in enumerate(ex):
        N, mean, M2 = float(e["N"]), float(e["mean"]), float(e["M2"])
        SA, S, Q = float(e["SA"]), float(e["S"]), float(e["Q"])
        dbl_mean = (L + 2) * EPS64 * (SA / N + abs(mean))
        dbl_m2 = (3 * L + 6) * EPS64 * (S + Q)
        assert dbl_mean <= U * abs(mean) / 16 and dbl_m2 <= U * M2 / 16, (c, dbl_mean, mean, dbl_m2, M2)
        v, t = coefficient_bounds(mean, M2, n_eff, dbl_mean, dbl_m2, float(inp["gamma"][c]), float(inp["beta"][c]),
                                  float(inp["running_mean"][c]), float(inp["running_var"][c]), mom, eps)
        for k in val:
            val[k][c], tol[k][c] = v[k], t[k]
    return val, tol


# ------------------------------------------------------------------------------------------------ finalize: float64 restatement
def finalize_restated(inp, nslab, mistake=None):
    """bn_finalize_kernel restated in numpy: the one-pass merge about the pivot in float64 (rows in index order), the roundings to
    float32 where the kernel rounds, products and sums of the last lines in float32 without contraction.  `mistake` seeds one error:
      "dead_rows_counted"   rows with a zero count are merged as well (their NaN with a zero weight)
      "no_walk"             the rows behind the first 1024 are never read
      "walk_skips_partial"  the last, partial batch behind the first 1024 is dropped
      "n_ignored"           the variance is taken over the counted total, not the caller's n
      "biased_running"      running_var takes the biased variance
      "pivot_dead_row"      the pivot is the first row's mean even when that row is dead
      "eps_outside"         rstd = 1 / (sqrt(var) + eps)"""
    mean, m2, cnt = inp["mean"].astype(np.float64), inp["m2"].astype(np.float64), inp["counts"].astype(np.float64)
    C = mean.shape[1]
    rows = nslab
    if mistake == "no_walk":
        rows = min(nslab, BNF_FAST)
    if mistake == "walk_skips_partial" and nslab > BNF_FAST:
        rows = nslab // BNF_FAST * BNF_FAST
    out = {k: np.zeros(C, F) for k in ("scale", "shift", "mean", "rstd", "m2_out", "running_mean", "running_var")}
    mom, eps = F(inp["momentum"]), F(inp["eps"])
    with np.errstate(all="ignore"):
        for c in range(C):
            piv = mean[0, c] if (cnt[0] > 0 or mistake == "pivot_dead_row") else 0.0
            N = A = S = Q = 0.0
            for i in range(rows):
                if cnt[i] > 0 or mistake == "dead_rows_counted":
                    d = mean[i, c] - piv
                    N += cnt[i]
                    A += cnt[i] * d
                    S += m2[i, c]
                    Q += cnt[i] * d * d
            mu = piv + A / N if N > 0 else 0.0
            M2 = S + Q - A * A / N if N > 0 else 0.0
            if M2 < 0:
                M2 = 0.0
            n = float(inp["n_pass"]) if (inp["n_pass"] > 0 and mistake != "n_ignored") else N
            var = M2 / n
            rstd = F(1.0 / (np.sqrt(var) + float(eps))) if mistake == "eps_outside" else F(1.0 / np.sqrt(var + float(eps)))
            sc = F(inp["gamma"][c] * rstd)
            out["scale"][c], out["rstd"][c], out["mean"][c], out["m2_out"][c] = sc, rstd, F(mu), F(M2)
            out["shift"][c] = F(inp["beta"][c] - F(F(mu) * sc))
            om = F(F(1) - mom)
            out["running_mean"][c] = F(F(om * inp["running_mean"][c]) + F(mom * F(mu)))
            unb = M2 / (n - 1.0) if (n > 1.0 and mistake != "biased_running") else var
            out["running_var"][c] = F(F(om * inp["running_var"][c]) + F(mom * F(unb)))
    return out


def expand_pixels(inp, c):
    """A population of float64 pixel values per live row whose (count, mean, M2) are the row's, for channel c: n - 2 values at the
    mean and a symmetric pair mean +- sqrt(M2 / 2) (one value where n = 1: M2 must be 0; then the row's M2 is dropped, which the
    caller accounts for).  -> (values, sum of the M2 dropped)."""
    vals, dropped = [], 0.0
    for i in range(len(inp["counts"])):
        n = int(inp["counts"][i])
        if n == 0:
            continue
        m, q = float(inp["mean"][i, c]), float(inp["m2"][i, c])
        if n == 1:
            vals.append(np.array([m]))
            dropped += q
        else:
            a = math.sqrt(q / 2)
            vals.append(np.concatenate([np.full(n - 2, m), [m - a, m + a]]))
    return np.concatenate(vals), dropped


# ------------------------------------------------------------------------------------------------ eval coefficients
EVAL_C = (1, 255, 256, 257)


def eval_inputs(C, family):
    """uh_bn_eval_coeffs.  dyadic: rv + eps in (4, 1, 1/4, 1/16) with eps = 2^-16, gamma and beta multiples of 1/8, running_mean
    multiples of 1/16: sqrt, the quotient by a power of two, the product and the difference are exact (asserted in eval_expected)."""
    rng = np.random.default_rng(_seed("eval", C, family))
    if family == "dyadic":
        eps = F(EPS_DYADIC)
        T = np.array([4.0, 1.0, 0.25, 0.0625])[rng.integers(0, 4, C)]
        rv = (T - float(eps)).astype(F)
        assert np.array_equal(rv.astype(np.float64) + float(eps), T)
        g = rng.integers(-32, 33, C)
        g[g == 0] = 8
        return dict(gamma=(g / 8).astype(F), beta=(rng.integers(-32, 33, C) / 8).astype(F),
                    running_mean=(rng.integers(-64, 65, C) / 16).astype(F), running_var=rv, eps=eps)
    return dict(gamma=((rng.random(C) + 0.5) * np.where(rng.random(C) < 0.25, -1, 1)).astype(F), beta=(rng.standard_normal(C) * 0.2).astype(F),
                running_mean=(rng.standard_normal(C) * np.where(rng.random(C) < 0.2, 100.0, 0.1)).astype(F),
                running_var=(10.0 ** rng.uniform(-4, 3, C)).astype(F), eps=F(1e-5))


def eval_expected(inp, family):
    """-> (scale, shift, tol_scale, tol_shift) in float64.  The kernel: sc = g / sqrtf(rv + eps), shift = b - rm * sc, all float32.
    Bound (general family): rv + eps rounds (relative u, u / 2 after the root), sqrtf rounds (u), the division rounds (u) -- both
    correctly rounded in this build (no fast-math flag): |dscale| <= 2.5 u |scale| (1 + 2^-20).  shift: |rm| |dscale| for the exact
    product, u |rm scale| for its rounding (absent where the compiler fuses it) and u (|b| + |rm scale|) (1 + 2^-20) for the result:
    covers both forms.  dyadic family: both tolerances are zero."""
    g, b, rm, rv = (inp[k].astype(np.float64) for k in ("gamma", "beta", "running_mean", "running_var"))
    eps = float(inp["eps"])
    scale = g / np.sqrt(rv + eps)
    shift = b - rm * scale
    if family == "dyadic":
        for v in (scale, rm * scale, shift):
            assert np.array_equal(v.astype(F).astype(np.float64), v)
        return scale, shift, np.zeros_like(scale), np.zeros_like(scale)
    ts = 2.5 * U * np.abs(scale) * (1 + 2.0 ** -20)
    return scale, shift, ts, np.abs(rm) * ts + U * np.abs(rm * scale) + U * (np.abs(b) + np.abs(rm * scale)) * (1 + 2.0 ** -20)


# ================================================================================================ B. the rows of the conv kernels
# Every forward form writes, per row r, {mean_r, M2_r} of the STORED y over the pixels of the tiles the row covers (tile t belongs to
# row t mod lanes; tiles in (image, tile row, tile column) order), and the pixel count n_r; rows lanes .. ntile - 1 get a zero count.
TILE = 16
CUS = 256                             # the persistent kernels size their grid for this many compute units (conv3x3.hip: lanes_for)


def tile_grid(B, H, W):
    return (H + TILE - 1) // TILE, (W + TILE - 1) // TILE


def rows_plan(shape, bf16, code):
    """What conv3x3.hip's fwd_plan decides for a dense, 16-byte aligned call, restated: the statistics producer and the number of
    live rows.  code = the answer of uh_conv3x3_fwd_kernel (asserted by the GPU test).  Producers:
      "mfma"        conv3x3_fwd_mfma_v2 (codes 1-4): pivot-shifted sums, one row per workgroup lane
      "stem_v3"     conv3x3_fwd_stem_v3 (bf16, Cin <= 4, Cout = 64): pivot-shifted sums in registers, min(tiles, 1024) rows
      "stem_v2"     conv3x3_fwd_stem_v2 (Cin <= 4, Cout a multiple of the 16-byte piece): two passes, one row per tile
      "stem_v1"     conv3x3_fwd_stem (Cin <= 4, any Cout): two passes, one row per tile
      "tile_stats"  conv3x3_fwd_generic + tile_stats_kernel: two passes, one row per tile"""
    B, H, W, C0, C1, Cout = shape
    ty, tx = tile_grid(B, H, W)
    ntile = B * ty * tx
    es = 2 if bf16 else 4

    def lanes_for(per_cu, slabs):
        gx = ((per_cu * CUS + slabs - 1) // slabs + 7) & ~7
        return min(gx, ntile)
    if code == 0:
        if C0 + C1 > 4 or C1:
            return dict(producer="tile_stats", lanes=ntile, ntile=ntile)
        if bf16 and Cout == 64:
            return dict(producer="stem_v3", lanes=min(ntile, 1024), ntile=ntile)
        return dict(producer="stem_v2" if Cout % (16 // es) == 0 else "stem_v1", lanes=ntile, ntile=ntile)
    lanes = {1: lambda: lanes_for(2, Cout // 128), 2: lambda: lanes_for(2, Cout // 64), 3: lambda: ntile,
             4: lambda: lanes_for(3, Cout // 64)}[code]()
    return dict(producer="mfma", lanes=lanes, ntile=ntile)


def to_tiles(y):
    """[B, H, W, C] float64 -> (T [ntile, 256, C] with zeros outside the image, M [ntile, 256] bool); pixel index = 16 row + column."""
    B, H, W, C = y.shape
    ty, tx = tile_grid(B, H, W)
    P = np.zeros((B, ty * TILE, tx * TILE, C))
    P[:, :H, :W] = y
    m = np.zeros((B, ty * TILE, tx * TILE), bool)
    m[:, :H, :W] = True
    T = P.reshape(B, ty, TILE, tx, TILE, C).transpose(0, 1, 3, 2, 4, 5).reshape(B * ty * tx, TILE * TILE, C)
    M = m.reshape(B, ty, TILE, tx, TILE).transpose(0, 1, 3, 2, 4).reshape(B * ty * tx, TILE * TILE)
    return T, M


def tile_origin(shape3, t):
    B, H, W = shape3
    ty, tx = tile_grid(B, H, W)
    b, r = divmod(t, ty * tx)
    return b, (r // tx) * TILE, (r % tx) * TILE


def row_counts(shape3, lanes):
    """-> (n_r float64 [lanes], k_r = tiles per row [lanes], per-tile pixel counts [ntile])."""
    B, H, W = shape3
    ty, tx = tile_grid(B, H, W)
    vy = np.minimum(TILE, H - np.arange(ty) * TILE)
    vx = np.minimum(TILE, W - np.arange(tx) * TILE)
    per_tile = np.tile((vy[:, None] * vx[None, :]).reshape(-1), B).astype(np.float64)
    n_r, k_r = np.zeros(lanes), np.zeros(lanes, np.int64)
    for first in range(0, len(per_tile), lanes):
        seg = per_tile[first:first + lanes]
        n_r[:len(seg)] += seg
        k_r[:len(seg)] += 1
    return n_r, k_r, per_tile


def _row_sum(per_tile_values, lanes):
    """[ntile, ...] -> [lanes, ...]: the float64 sum over the tiles of each row."""
    out = np.zeros((lanes,) + per_tile_values.shape[1:])
    for first in range(0, len(per_tile_values), lanes):
        seg = per_tile_values[first:first + lanes]
        out[:len(seg)] += seg
    return out


def reference_rows(y, lanes, weight=None):
    """The exact rows of the stored y [B, H, W, C] (float64): n_r, mean_r, M2_r (two passes in float64; on these families every value
    is an integer and the sums are exact).  `weight` [ntile, 256]: how often each pixel counts (the planted errors: 0 or 2)."""
    T, M = to_tiles(y)
    wt = M.astype(np.float64) if weight is None else weight
    n_r = _row_sum(wt.sum(1), lanes)
    s1 = _row_sum((T * wt[:, :, None]).sum(1), lanes)
    mean_r = s1 / n_r[:, None]
    R = np.arange(len(T)) % lanes
    d = (T - mean_r[R][:, None, :]) * np.sqrt(wt)[:, :, None]
    return n_r, mean_r, _row_sum((d * d).sum(1), lanes)


def merge_rows(n_r, mean_r, m2_r):
    """Rows -> per-channel (mean, M2), merged in float64 (as tests/test_gpu_exact_pixel.py::test_stem_statistics_rows does)."""
    n = n_r.sum()
    mean = (n_r[:, None] * mean_r).sum(0) / n
    return mean, m2_r.sum(0) + (n_r[:, None] * (mean_r - mean) ** 2).sum(0)


def whole_moments(y):
    mean = y.mean((0, 1, 2))
    return mean, ((y - mean) ** 2).sum((0, 1, 2))


def pivots(y_ext, shape3, plan):
    """The pivot of every live row and channel [lanes, C], from the stored y extended by the two virtual rows below the image
    (y_ext [B, H + 2, W, C]): one value of the row's FIRST tile (origin y0, x0; vy x vx valid pixels),
      mfma:    pixel (y0 + 2, x0 + 8), column x0 where vx <= 8 -- on a tile under three rows high that is a pixel below the image,
               whose accumulator the kernel forms from the zero-filled halo like any other;
      stem_v3: pixel (y0 + 8, x0 + 8) where vy > 8 and vx > 8, else (y0, x0)."""
    B, H, W = shape3
    out = np.zeros((plan["lanes"], y_ext.shape[-1]))
    for r in range(plan["lanes"]):
        b, y0, x0 = tile_origin(shape3, r)
        vy, vx = min(TILE, H - y0), min(TILE, W - x0)
        if plan["producer"] == "mfma":
            out[r] = y_ext[b, y0 + 2, x0 + (8 if vx > 8 else 0)]
        else:
            out[r] = y_ext[b, y0 + 8, x0 + 8] if (vy > 8 and vx > 8) else y_ext[b, y0, x0]
    return out


F32_INT = float(1 << 24)
SECOND = 1 + 2.0 ** -16               # covers the second-order terms of at most 300 roundings: (1 + u)^300 - 1 <= 300 u (1 + 2^-16)


def row_bounds(y, y_ext, shape3, plan, v2_lanes=32):
    """-> (tol_mean [C], tol_m2 [C], table of conditions): the bound on the merged mean and M2 of the rows one producer writes,
    from its arithmetic.  u = 2^-24; y is an integer tensor; per row r and channel: n = n_r, k = k_r tiles.

    Pivot-shifted form (mfma; stem_v3 in brackets).  p = the row's pivot (pivots()), d = y - p: integers, exact while |d| < 2^24
    (asserted).  S1 = sum d, S2 = sum d^2 =: D, A1 = sum |d|.
      * partial sums.  A lane adds its 16 [8 k] pixels in turn, the first onto zero: 15 [8 k - 1] roundings; 4 adds of the 16-lane
        row sum [3 shuffle levels]; k - 1 adds of the tile sums onto the workgroup's [3 adds over the waves]: R = 18 + k [8 k + 5]
        roundings at most on the way of a term, each at most u times a partial sum of magnitudes.  While A1 < 2^24 every partial
        sum of S1 is an exact integer: dS1 = 0, else dS1 = R u A1; while D < 2^24 the same for S2 (d^2 < 2^24): dS2 = 0, else R u D.
      * mean_r = fl(p + fl(S1 fl(1 / n))) [fl(p + fl(S1 / n))], the product possibly fused: e_r = dS1 / n + 2 u |S1 / n| + u |mean_r|.
      * M2_r = max(fl(S2 - fl(fl(S1 S1) fl(1 / n))), 0) [.. / n], possibly fused: eM_r = dS2 + 3 u S1^2 / n + 2 |S1| dS1 / n + u M2_r.
        (The clamp moves a negative result towards the true M2_r >= 0.)
    Two passes (stem_v1, stem_v2, tile_stats).  s = sum y: exact while sum |y| < 2^24 (asserted).  mu = fl(s / n) (stem_v2:
    fl(s fl(1 / n))): e_r = 2 u |mean_r|.  Second pass: d = fl(y - mu), d^2 (fused or not), added over `inner` pixels in a thread
    and `outer` partial results in turn: R2 = inner - 1 + outer - 1 roundings (stem_v1: 64 pixels per wave, 4 waves; stem_v2: 8
    pixels per lane, 256 / GB lanes; tile_stats: 256 pixels, one thread); sum (y - mu)^2 = M2_r + n (mu - mean_r)^2 exactly, so
      eM_r = (3 + R2) u (M2_r + n e_r^2) + n e_r^2.
    Merge in float64 (merge_rows): mean = sum n_r mean_r / n moves by at most sum n_r e_r / n; M2 = sum M2_r + sum n_r (mean_r - mean)^2
    by at most sum (eM_r + 2 n_r |mean_r - mean| e_r + n_r e_r^2) (the first-order effect of the merged mean's own shift is zero:
    sum n_r (mean_r - mean) = 0).  Every term carries the factor SECOND for what is of second order."""
    lanes, prod = plan["lanes"], plan["producer"]
    n_r, k_r, _ = row_counts(shape3, lanes)
    _, mean_r, m2_r = reference_rows(y, lanes)
    mean, _ = merge_rows(n_r, mean_r, m2_r)
    n = n_r[:, None]
    cond = {}
    if prod in ("mfma", "stem_v3"):
        p = pivots(y_ext, shape3, plan)
        T, M = to_tiles(y)
        R_of = np.arange(len(T)) % lanes
        d = (T - p[R_of][:, None, :]) * M[:, :, None]
        assert float(np.abs(d).max()) < F32_INT and float(np.abs(y_ext).max()) < F32_INT
        S1, A1, D = _row_sum(d.sum(1), lanes), _row_sum(np.abs(d).sum(1), lanes), _row_sum((d * d).sum(1), lanes)
        R = (18 + k_r if prod == "mfma" else 8 * k_r + 5)[:, None].astype(np.float64)
        dS1 = np.where(A1 < F32_INT, 0.0, R * U * A1)
        dS2 = np.where(D < F32_INT, 0.0, R * U * D)
        e_r = dS1 / n + 2 * U * np.abs(S1 / n) + U * np.abs(mean_r)
        eM_r = dS2 + 3 * U * S1 * S1 / n + 2 * np.abs(S1) * dS1 / n + U * m2_r
        cond = dict(S1_exact=bool((A1 < F32_INT).all()), S2_exact=bool((D < F32_INT).all()), S1sq_max=float((S1 * S1).max()),
                    D_max=float(D.max()))
    else:
        T, M = to_tiles(y)
        assert float(_row_sum(np.abs(T).sum(1), lanes).max()) < F32_INT, "the first pass of a tile is not exact"
        inner, outer = {"stem_v1": (64, 4), "stem_v2": (8, v2_lanes), "tile_stats": (256, 1)}[prod]
        R2 = inner - 1 + outer - 1
        e_r = 2 * U * np.abs(mean_r)
        eM_r = (3 + R2) * U * (m2_r + n * e_r ** 2) + n * e_r ** 2
    tol_mean = SECOND * (n * e_r).sum(0) / n_r.sum()
    tol_m2 = SECOND * (eM_r + 2 * n * np.abs(mean_r - mean) * e_r + n * e_r ** 2).sum(0)
    return tol_mean, tol_m2, cond


def v2_lanes(Cout, bf16):
    """conv3x3_fwd_stem_v2: pixel lanes per channel group = 256 / GB with GB = min(Cout / V, 8), V = 16 bytes of channels."""
    V = 8 if bf16 else 4
    return 256 // max(1, min(Cout // V, 8))                            # (only read for the stem_v2 producer: Cout % V == 0)


# ---- float32 restatements of the producers (the CPU proof that the bounds hold for arithmetic of that shape)
def _tree(v, axis):
    """Pairwise float32 sum along an axis of power-of-two length."""
    v = np.moveaxis(v, axis, 0)
    while v.shape[0] > 1:
        v = (v[0::2] + v[1::2]).astype(F)
    return v[0]


def _seq(v, axis):
    """Float32 sum along an axis, in index order."""
    v = np.moveaxis(v, axis, 0)
    s = v[0].astype(F)
    for i in range(1, v.shape[0]):
        s = (s + v[i]).astype(F)
    return s


def restate_pivot(y, p, lanes, producer, use_pivot=True):
    """mfma: lane = a column of the tile, its 16 rows in turn, the 16 lanes by a tree, the tiles of a row in turn.  stem_v3: thread =
    pixels pl + 32 j of every tile of the row in turn, the 32 threads by a tree (3 shuffle levels, then the waves in turn).
    use_pivot=False: the plain sums (p = 0), the last planted error."""
    T, M = to_tiles(y)
    ntile, _, C = T.shape
    R_of = np.arange(ntile) % lanes
    pv = (p if use_pivot else np.zeros_like(p)).astype(F)
    d = ((T.astype(F) - pv[R_of][:, None, :]) * M[:, :, None]).astype(F)
    dd = (d * d).astype(F)
    rows = int(np.ceil(ntile / lanes))
    pad = rows * lanes - ntile

    def by_row(v):                                                     # [ntile, ...] -> [rows-of-tiles, lanes, ...], absent tiles zero
        return np.concatenate([v, np.zeros((pad,) + v.shape[1:], F)]).reshape((rows, lanes) + v.shape[1:])
    out = []
    for v in (d, dd):
        if producer == "mfma":
            t = _tree(_seq(v.reshape(ntile, TILE, TILE, C), 1), 1)     # [ntile, C]
            out.append(_seq(by_row(t), 0))
        else:
            th = np.moveaxis(by_row(v.reshape(ntile, 8, 32, C)), 2, 1) # [k, j, lanes, pl, C]
            acc = _seq(th.reshape(rows * 8, lanes, 32, C), 0)          # one accumulator: tile by tile, j in turn: [lanes, pl, C]
            acc = acc.reshape(lanes, 4, 8, C)                          # pl = 8 wave + lane bits
            out.append(_seq(_tree(acc, 2), 1))
    S1, S2 = out
    return S1, S2, pv


def finish_pivot(S1, S2, pv, n_r, producer):
    n = n_r.astype(F)[:, None]
    if producer == "mfma":
        inv = (F(1) / n).astype(F)
        mean = (pv + (S1 * inv).astype(F)).astype(F)
        m2 = np.maximum((S2 - ((S1 * S1).astype(F) * inv).astype(F)).astype(F), F(0))
    else:
        mean = (pv + (S1 / n).astype(F)).astype(F)
        m2 = np.maximum((S2 - ((S1 * S1).astype(F) / n).astype(F)).astype(F), F(0))
    return mean.astype(np.float64), m2.astype(np.float64)


def restate_two_pass(y, shape3, producer, lanes32=32):
    """stem_v1: wave w adds rows 4 w .. 4 w + 3 of the tile in turn, the four waves in turn.  stem_v2: lane pl adds pixels
    pl + j PL, then the PL lanes in turn; mu = s * fl(1 / n).  tile_stats: one thread, row-major."""
    T, M = to_tiles(y)
    ntile, _, C = T.shape
    _, _, per_tile = row_counts(shape3, ntile)
    n = per_tile.astype(F)[:, None]

    def total(v):
        if producer == "stem_v1":
            return _seq(_seq(v.reshape(ntile, 4, 64, C), 2), 1)
        if producer == "stem_v2":
            return _seq(_seq(v.reshape(ntile, 256 // lanes32, lanes32, C), 1), 1)
        return _seq(v, 1)
    s = total((T * M[:, :, None]).astype(F))
    mu = (s * (F(1) / n).astype(F)).astype(F) if producer == "stem_v2" else (s / n).astype(F)
    d = ((T.astype(F) - mu[:, None, :]).astype(F) * M[:, :, None]).astype(F)
    m2 = total((d * d).astype(F))
    return mu.astype(np.float64), m2.astype(np.float64)


# ---- the families of part B
RowsCase = collections.namedtuple("RowsCase", "shape family x w y y_ext")


def _conv_ext(x, w):
    """y [B, C, H, W] and y_ext [B, C, H + 2, W] in float64: the conv of the zero-extended image, two rows below the image included."""
    import torch
    import torch.nn.functional as TF
    ye = TF.conv2d(TF.pad(x.double(), (0, 0, 0, 3)), w.double(), padding=1)[:, :, :x.shape[2] + 2]
    return ye[:, :, :x.shape[2]].contiguous(), ye.contiguous()


def flat_case(shape, large):
    """Channels that are nearly flat: x = m_ci + a pattern in -2 .. 2 whose sum over every full 16 x 16 tile is zero, filters with
    three +-1 (fewer where Cin < 3) on the CENTRE tap only, so y_c = sum +-x_ci pixel by pixel: |y - mean| <= 6 in every channel,
    and the sum of y over a full tile is 256 times an integer.  On full tiles the rows are then EXACT in every producer (asserted
    where it is used: flat_rows_exact).  large: m_ci in 500 .. 1500 (fp32 only), the large-mean case of the plain-sum mistake."""
    import torch
    B, H, W, C0, C1, Cout = shape
    Cin = C0 + C1
    g = torch.Generator().manual_seed(_seed("flat", shape, large) % (1 << 31))
    ty, tx = tile_grid(B, H, W)
    vals = torch.cat([torch.tensor([-2.0, -1.0, 0.0, 1.0, 2.0]).repeat(51), torch.zeros(1)])
    idx = torch.rand(B, Cin, ty, tx, 256, generator=g).argsort(-1)
    pat = vals[idx].view(B, Cin, ty, tx, TILE, TILE).permute(0, 1, 2, 4, 3, 5).reshape(B, Cin, ty * TILE, tx * TILE)[:, :, :H, :W]
    m = torch.randint(500, 1501, (Cin,), generator=g).float() if large else torch.randint(-2, 3, (Cin,), generator=g).float()
    x = (pat + m.view(1, Cin, 1, 1)).contiguous()
    w = torch.zeros(Cout, Cin, 3, 3)
    k = min(3, Cin)
    for co in range(Cout):
        ci = torch.randperm(Cin, generator=g)[:k]
        w[co, ci, 1, 1] = (torch.randint(0, 2, (k,), generator=g) * 2 - 1).float()
    y, ye = _conv_ext(x, w)
    mean = y.mean((0, 2, 3), keepdim=True)
    assert float((y - mean).abs().max()) <= 6.5 and float(y.abs().max()) < (256 if not large else F32_INT)
    return RowsCase(shape, "flat_large" if large else "flat", x, w, y, ye)


def family_case(shape, family):
    """ternary / wide: the tensors of exact_inputs.conv3x3_case (its conditions asserted there); flat / flat_large: flat_case."""
    if family in ("flat", "flat_large"):
        return flat_case(shape, family == "flat_large")
    import exact_inputs as E
    c = E.conv3x3_case(shape, family)
    y, ye = _conv_ext(c.x, c.w)
    assert bool((y == c.y).all())
    return RowsCase(shape, family, c.x, c.w, y, ye)


def stored(t_nchw, bf16):
    """NCHW float64 reference -> NHWC float64 of what the kernel stores (bf16: one rounding to nearest even)."""
    import torch
    t = t_nchw.permute(0, 2, 3, 1).contiguous()
    return (t.float().bfloat16().double() if bf16 else t.float().double()).numpy()


def flat_rows_exact(y, shape3, plan, y_ext):
    """The conditions under which a row of the flat family has ONE right answer, whatever the pivot and the order: every row covers
    full tiles only and a power-of-two pixel count; pivot forms: every partial sum of S1 and S2 and S1^2 are integers below 2^24,
    so mean_r = p + S1 / n and M2_r = S2 - S1^2 / n round once, from exact operands, fused or not; two passes: mu is an integer, so
    d = y - mu and d^2 are integers and their sum is below 2^24.  -> (mean_r, M2_r) as float32, both exactly representable."""
    lanes = plan["lanes"]
    B, H, W = shape3
    assert H % TILE == 0 and W % TILE == 0
    n_r, mean_r, m2_r = reference_rows(y, lanes)
    assert all(int(v) & (int(v) - 1) == 0 for v in n_r)
    if plan["producer"] in ("mfma", "stem_v3"):
        p = pivots(y_ext, shape3, plan)
        T, M = to_tiles(y)
        d = T - p[np.arange(len(T)) % lanes][:, None, :]
        S1, A1, D = _row_sum(d.sum(1), lanes), _row_sum(np.abs(d).sum(1), lanes), _row_sum((d * d).sum(1), lanes)
        assert float(A1.max()) < F32_INT and float(D.max()) < F32_INT and float((S1 * S1).max()) < F32_INT
    else:
        assert bool((mean_r == np.round(mean_r)).all()) and float(m2_r.max()) < F32_INT
    assert np.array_equal(mean_r.astype(F).astype(np.float64), mean_r) and np.array_equal(m2_r.astype(F).astype(np.float64), m2_r)
    return mean_r.astype(F), m2_r.astype(F)


# ================================================================================================ C. the chain
def coefficient_bounds(mean, M2, n_eff, d_mean, d_m2, gamma, beta, rm, rv, mom, eps):
    """Part A's formulas (general_bounds) for one channel, with d_mean and d_m2 the errors of the merged mean and M2 BEFORE the
    finalize rounds them to float32: part B's row bounds plus the double term.  dvar = d_m2 / n, drstd = rstd^3 dvar / 2 =
    rstd (d_m2 / n) / (2 (var + eps)).  -> ({name: value}, {name: bound})."""
    var = M2 / n_eff
    rstd = 1.0 / math.sqrt(var + eps)
    e_mean = U * abs(mean) + d_mean
    e_rstd = U * rstd + rstd * (d_m2 / n_eff) / (2 * (var + eps)) + 4 * EPS64 * rstd
    e_scale = abs(gamma) * e_rstd + U * abs(gamma * rstd)
    ms = abs(mean * gamma * rstd)
    unb = M2 / (n_eff - 1) if n_eff > 1 else var
    e_unb = U * unb + d_m2 / max(n_eff - 1, 1) + 2 * EPS64 * unb
    val = dict(mean=mean, m2_out=M2, rstd=rstd, scale=gamma * rstd, shift=beta - mean * gamma * rstd,
               running_mean=(1 - mom) * rm + mom * mean, running_var=(1 - mom) * rv + mom * unb)
    tol = dict(mean=e_mean, m2_out=U * M2 + d_m2, rstd=e_rstd, scale=e_scale,
               shift=abs(mean) * e_scale + abs(gamma * rstd) * e_mean + e_mean * e_scale + U * ms + U * (abs(beta) + ms) * SECOND,
               running_mean=4 * U * (abs(rm) + abs(mom * mean)) * SECOND + mom * e_mean,
               running_var=4 * U * (abs(rv) + abs(mom * unb)) * SECOND + mom * e_unb)
    return val, tol


CHAIN_SHAPE = (1, 513, 513, 1, 0, 64)


# ================================================================================================ the cases of parts B and C
# (B, H, W, C0, C1, Cout), the answer of uh_conv3x3_fwd_kernel in fp32 and in bf16 (None: not run), the families.
# The first block is tests/test_gpu_exact.py's FWD_CASES (the CPU companion asserts that it still is).
ROWS_CASES = [
    ((2, 12, 14, 8, 8, 16), 0, 0, ("ternary", "wide")),           # generic + tile_stats_kernel, two sources
    ((3, 19, 33, 1, 0, 64), 0, 0, ("ternary", "wide")),           # fp32 conv3x3_fwd_stem_v2, bf16 conv3x3_fwd_stem_v3
    ((2, 20, 20, 3, 0, 64), 0, 0, ("ternary", "wide")),
    ((2, 120, 120, 32, 0, 512), 1, 1, ("ternary", "wide")),
    ((2, 17, 23, 64, 0, 64), 4, 2, ("ternary", "wide")),
    ((1, 16, 16, 256, 0, 64), 4, 3, ("ternary", "wide")),
    ((2, 20, 37, 256, 256, 128), 4, 3, ("ternary", "wide")),
    ((2, 17, 23, 64, 64, 64), 4, 4, ("ternary", "wide")),
    ((1, 40, 24, 128, 128, 128), 4, 3, ("ternary", "wide")),
    ((1, 16, 16, 1024, 0, 64), 4, 3, ("ternary", "wide")),
    ((1, 448, 448, 64, 0, 64), None, 2, ("ternary", "wide")),     # 784 tiles on 512 rows
    # added here
    ((2, 20, 20, 3, 0, 6), 0, 0, ("ternary", "wide")),            # conv3x3_fwd_stem: Cout off the 16-byte grid
    ((2, 20, 20, 3, 0, 16), None, 0, ("ternary", "wide")),        # conv3x3_fwd_stem_v2 in bf16: one channel group pair, 128 pixel lanes
    ((2, 17, 23, 64, 0, 64), 4, None, ("flat_large",)),           # mean in the thousands, |y - mean| <= 6
    # full tiles, one per row: the flat family's rows are exact
    ((1, 16, 16, 8, 8, 16), 0, 0, ("flat",)),
    ((1, 16, 16, 3, 0, 6), 0, None, ("flat",)),
    ((1, 16, 32, 3, 0, 64), 0, 0, ("flat",)),
    ((1, 16, 16, 64, 0, 64), 4, 2, ("flat",)),
    ((1, 16, 16, 256, 0, 64), None, 3, ("flat",)),
    ((2, 128, 128, 32, 0, 512), None, 1, ("flat",)),
]
N_FWD_CASES = 11


def rows_params():
    return [(shape, fam, bf16, code) for shape, c32, c16, fams in ROWS_CASES for fam in fams for bf16, code in ((False, c32), (True, c16))
            if code is not None]


def chain_params():
    return [(CHAIN_SHAPE, "ternary", False, 0), (CHAIN_SHAPE, "ternary", True, 0)]


def rows_id(v):
    if isinstance(v, tuple):
        return "x".join(map(str, v))
    return {True: "bf16", False: "fp32"}.get(v, str(v)) if isinstance(v, bool) else str(v)
