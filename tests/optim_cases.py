"""Cases, float64 references, bounds, float32 restatements and seeded mistakes shared by tests/test_gpu_optim.py (the kernels of
csrc/optim.hip on the MI355X, through the C ABI and through FusedRMSprop) and tests/test_optim_cpu.py (the CPU proof that float32
arithmetic meets the bounds with half the room to spare and that each seeded mistake breaks one).  Nothing here needs a GPU.

References.  Primary (the one the bounds refer to): oracle/step_ref.py's rmsprop_update in float64 on the values the kernel
receives -- p, g, sq, buf as float32, every hyper-parameter rounded to float32 first (the C ABI takes float), 1 - alpha therefore
the float32 1.f - alpha (exact for alpha in [1/2, 1], so the double 1 - alpha of the rounded alpha is the same number).  The clip
coefficient is ONE float32 scalar, fminf(max_norm / (norm + 1e-6f), 1.f): coef32 restates it, g' = g * coef32 is an equality that
pins it, and the CPU companion holds it to step_ref.clip_coef in float64 (two roundings).  Second: stock torch.optim.RMSprop with
clip_grad_norm_ in float64 with the Python doubles (stock_torch_step); step_ref with the same doubles (oracle_step_doubles)
equals it, which validates the oracle's restatement.

Bounds are derived in the docstring of tests/test_gpu_optim.py."""
import collections
import zlib

import numpy as np
import torch

from oracle import step_ref as S

F = np.float32
U = 2.0 ** -24                        # the relative error of one float32 rounding
DENORM = 2.0 ** -149                  # what one rounding below the normal range may lose, absolutely
OP_TOL = 2e-5                         # the project's op-by-op bound (the distance to stock torch is held to it)
# Units of u times the magnitudes of step_reference(), fixed before any kernel ran: four times the worst of the float32
# restatement over every case below (sq 4.63, buf 2.33, p 1.77), rounded up; the CPU companion requires the restatement <= K / 2.
K_S, K_B, K_P = 19, 10, 8
# The first step without weight decay, momentum and clipping has no cancellation and few roundings: counted, not measured
# (2 u and the second-order terms; see the docstring of tests/test_gpu_optim.py).
SHARP_S, SHARP_B = 2.01, 2.01
FLOOR_S = 5 * DENORM
SUMSQ_ULPS = 17                       # of u * S64: 8 (a thread's terms) + 6 (shuffle levels) + 3 (LDS adds); n <= 2^22 + 7
SUMSQ_MAXBLK, STEP_MAXBLK = 2048, 4096

HYPERS = {
    "reference": dict(lr=1e-5, alpha=0.99, eps=1e-8, wd=1e-8, mu=0.999),        # the reference's train.py
    "ema": dict(lr=1e-3, alpha=0.99, eps=1e-8, wd=1e-2, mu=0.9),                # tests/test_gpu_ema.py
    "plain": dict(lr=1e-3, alpha=0.99, eps=1e-8, wd=0.0, mu=0.0),
}


def hyper32(h):
    """The values the kernel receives: each rounded to float32, as Python doubles."""
    return {k: float(F(v)) for k, v in h.items()}


def _seed(*key):
    return zlib.crc32(repr(key).encode())


# ------------------------------------------------------------------------------------------------ the step: cases
StepCase = collections.namedtuple("StepCase", "name n hyper state norm max_norm")
SIZES = (1, 3, 4, 5, 7, 1023, 1024, 1025, 4099)
ONE_SWEEP, WRAP = 2 ** 22, 2 ** 22 + 7       # exactly 4096 workgroups of 256 x 4 elements; the loop goes round and the tail runs
STATES = ("ordinary", "first", "gzero", "wide", "large")
BELOW_ONE, ABOVE_ONE = float(np.nextafter(F(1), F(0))), float(np.nextafter(F(1), F(2)))

STEP_CASES = (
    [StepCase(f"n{n}-{h}", n, h, "ordinary", 7.5, 1.0) for n in SIZES for h in HYPERS] +
    [StepCase(f"{st}-{h}", 4099, h, st, 7.5, 1.0) for st in STATES[1:] for h in HYPERS] +
    [StepCase("tiny", 4099, "plain", "tiny", 0.25, 1.0)] +
    [StepCase(f"{name}-{h}", 1025, h, "ordinary", norm, mx) for h in ("reference", "ema") for name, norm, mx in (
        ("far_below", 1e-3, 1.0), ("far_above", 1e4, 1.0), ("at_max_norm", 1.0, 1.0), ("just_below", BELOW_ONE, 1.0),
        ("just_above", ABOVE_ONE, 1.0), ("max_norm_half", 3.0, 0.5), ("max_norm_zero", 7.5, 0.0), ("norm_null", None, 1.0))] +
    [StepCase("one_sweep", ONE_SWEEP, "ema", "ordinary", 7.5, 1.0), StepCase("wrap", WRAP, "ema", "ordinary", 7.5, 1.0),
     StepCase("wrap-first", WRAP, "reference", "first", 0.25, 1.0)])
# no weight decay, no momentum, no clipping, first step: ge = g exactly and sq' = fl(fl((1 - alpha) g) g)
SHARP_CASES = [StepCase(f"sharp-n{n}", n, "plain", "first", None, 0.0) for n in (7, 4099)]
NONFINITE = [(norm, mx) for norm in (float("nan"), float("inf")) for mx in (1.0, 0.0)]
CASE_BY_NAME = {c.name: c for c in STEP_CASES + SHARP_CASES}
assert len(CASE_BY_NAME) == len(STEP_CASES) + len(SHARP_CASES)


def step_inputs(case):
    """{"p", "g", "s", "b"}: float32 arrays of case.n elements.
    ordinary: p ~ N(0,1), g ~ 0.1 N(0,1), sq ~ 0.01 U(0,1), buf ~ 0.1 N(0,1).   first: sq = buf = 0.
    gzero: a first step with g = 0 on every other element and p = 0 on every fourth (there ge = 0 and the quotient is 0 / eps).
    wide: |g| = 10^U(-20, 0); sq = U(0,1) g^2 on the odd elements, 0 on the even ones.   large: g ~ 1e3 N(0,1), sq ~ 1e6 U(0,1).
    tiny: |g| in [1e-20, 2e-20), sq = buf = 0 -- with wd = 0 the new sq is about 1e-42, below the normal range."""
    n, r = case.n, np.random.default_rng(_seed(case.name))
    p = r.standard_normal(n, dtype=F)
    g = r.standard_normal(n, dtype=F) * F(0.1)
    s = r.random(n, dtype=F) * F(0.01)
    b = r.standard_normal(n, dtype=F) * F(0.1)
    st = case.state
    if st in ("first", "gzero", "tiny"):
        s, b = np.zeros(n, F), np.zeros(n, F)
    if st == "gzero":
        g[::2] = 0
        p[::4] = 0
    elif st == "wide":
        g = (np.sign(g) * F(10.0) ** (r.random(n, dtype=F) * F(-20.0))).astype(F)
        s = (r.random(n, dtype=F) * g * g).astype(F)
        s[::2] = 0
    elif st == "large":
        g, s = g * F(1e4), s * F(1e8)
    elif st == "tiny":
        g = (np.sign(g) * F(1e-20) * (F(1) + r.random(n, dtype=F))).astype(F)
    else:
        assert st in ("ordinary", "first")
    return {"p": p, "g": g, "s": s, "b": b}


def coef32(norm, max_norm, mistake=None):
    """The kernel's own statement of the clip coefficient, in float32.  norm None: total_norm == NULL."""
    if norm is None or not max_norm > 0:
        return F(1)
    with np.errstate(divide="ignore"):
        den = F(norm) if mistake == "coef_without_1e-6" else F(norm) + F(1e-6)
        return np.minimum(F(max_norm) / den, F(1))


def step_reference(x, coef, hyper):
    """The primary reference: float64 on the float32 inputs and the float32-rounded hyper-parameters.  Returns float64 arrays:
    g, s, b, p (the outputs), the magnitudes mag_s, mag_b the bounds are relative to, and floor_b."""
    h = hyper32(hyper)
    t = {k: torch.from_numpy(x[k]).double() for k in "pgsb"}
    gc = t["g"] * float(coef)
    p2, s2, b2 = S.rmsprop_update(t["p"], gc, t["s"], t["b"], h["lr"], alpha=h["alpha"], eps=h["eps"], weight_decay=h["wd"],
                                  momentum=h["mu"])
    wdp = h["wd"] * t["p"]
    A = gc.abs() + wdp.abs()
    den = s2.sqrt() + h["eps"]
    q = (gc + wdp) / den
    out = {"g": gc, "s": s2, "b": b2, "p": p2,
           "mag_s": h["alpha"] * t["s"] + (1 - h["alpha"]) * A * A,
           "mag_b": (h["mu"] * t["b"]).abs() + q.abs() + A / den,
           "floor_b": DENORM * (2 + 2 / den)}
    return {k: v.numpy() for k, v in out.items()}


def step_f32(x, coef, hyper, mistake=None, at=None):
    """The statements of rmsprop_update in csrc/optim.hip in numpy float32, every operation rounded on its own (the kernel may
    contract products and sums into FMAs, which only removes roundings).  mistake: one of STEP_MISTAKES; `at`: the element that
    "double" updates twice."""
    h = {k: F(v) for k, v in hyper.items()}
    one = F(1)
    coef = F(coef)

    def update(p, g, s, b):
        one_m = F(1.0 - float(hyper["alpha"])) if mistake == "one_minus_alpha_from_double" else one - h["alpha"]
        gc = g * coef
        wdp = h["wd"] * p
        if mistake == "decay_scaled_too":
            ge = (g + wdp) * coef
        elif mistake == "no_weight_decay":
            ge = gc
        else:
            ge = gc + wdp
        s2 = h["alpha"] * s + one_m * ge * ge
        if mistake == "eps_inside_sqrt":
            den = np.sqrt(s2 + h["eps"])
        elif mistake == "old_second_moment":
            den = np.sqrt(s) + h["eps"]
        else:
            den = np.sqrt(s2) + h["eps"]
        q = ge / den
        b2 = h["mu"] * b + q
        p2 = p - h["lr"] * (q if mistake == "lr_times_quotient" else b2)
        return p2, (g if mistake == "g_left_unscaled" else gc), s2, b2

    with np.errstate(under="ignore"):
        out = [a.astype(F) for a in update(x["p"], x["g"], x["s"], x["b"])]
        if mistake == "dropped_tail":
            for a, k in zip(out, "pgsb"):
                a[-1] = x[k][-1]
        if mistake == "double":
            again = update(*(a[at:at + 1] for a in out))
            for a, v in zip(out, again):
                a[at] = v[0]
    assert all(a.dtype == F for a in out)
    return dict(zip("pgsb", out))


STEP_MISTAKES = ("eps_inside_sqrt", "old_second_moment", "decay_scaled_too", "no_weight_decay", "one_minus_alpha_from_double",
                 "lr_times_quotient", "g_left_unscaled", "coef_without_1e-6", "dropped_tail", "double")


def _units(err, mag, floor):
    """The worst of (err - floor) / (u mag); an error above the floor where the magnitude is 0 counts as infinite."""
    excess = np.maximum(err - floor, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        u = np.where(mag > 0, excess / (U * mag), np.where(excess > 0, np.inf, 0.0))
    return float(u.max())


def step_units(got, x, ref, hyper):
    """got: the four float32 outputs.  -> {"g": elements that differ from g * coef, "s", "b", "p": worst units}.  p is held to
    p - lr b' with the b' that was returned (one product, one difference; the product may lose 2^-149)."""
    for k in "pgsb":
        assert got[k].dtype == F and got[k].shape == x[k].shape and bool(np.isfinite(got[k]).all()), k
    h = hyper32(hyper)
    lrb = h["lr"] * got["b"].astype(np.float64)
    p64 = x["p"].astype(np.float64)
    return {"g": int((got["g"].view(np.int32) != ref["g"].astype(F).view(np.int32)).sum()),
            "s": _units(np.abs(got["s"] - ref["s"]), ref["mag_s"], FLOOR_S),
            "b": _units(np.abs(got["b"] - ref["b"]), ref["mag_b"], ref["floor_b"]),
            "p": _units(np.abs(got["p"] - (p64 - lrb)), np.abs(p64) + np.abs(lrb), DENORM)}


def step_breaks(units, ks=K_S, kb=K_B, kp=K_P):
    """The names of the outputs that miss their bound."""
    return [k for k, lim in (("g", 0), ("s", ks), ("b", kb), ("p", kp)) if units[k] > lim]


def check_step(got, x, ref, hyper, ks=K_S, kb=K_B, kp=K_P, what=""):
    units = step_units(got, x, ref, hyper)
    assert not step_breaks(units, ks, kb, kp), f"{what}: {units} against g == , sq {ks}, buf {kb}, p {kp}"
    return units


def fmt_units(units):
    return f"g {units['g']} differ, sq {units['s']:.2f}, buf {units['b']:.2f}, p {units['p']:.2f} units"


# ------------------------------------------------------------------------------------------------ stock torch
def real_norm32(g):
    """What uh_grad_sumsq returns for g, up to its own error: the float64 norm rounded once."""
    return float(F(np.sqrt(float((g.astype(np.float64) ** 2).sum()))))


def stock_torch_step(x, max_norm, hyper):
    """clip_grad_norm_ + torch.optim.RMSprop(momentum > 0, centered=False) in float64 with the Python doubles.  The norm is
    the gradient's own.  -> float64 arrays g, s, b, p."""
    p = torch.nn.Parameter(torch.from_numpy(x["p"]).double())
    opt = torch.optim.RMSprop([p], lr=hyper["lr"], alpha=hyper["alpha"], eps=hyper["eps"], weight_decay=hyper["wd"],
                              momentum=hyper["mu"], centered=False)
    assert hyper["mu"] > 0
    opt.state[p] = {"step": torch.tensor(0.0), "square_avg": torch.from_numpy(x["s"]).double(),
                    "momentum_buffer": torch.from_numpy(x["b"]).double()}
    p.grad = torch.from_numpy(x["g"]).double()
    if max_norm:
        torch.nn.utils.clip_grad_norm_([p], max_norm)
    opt.step()
    st = opt.state[p]
    return {"g": p.grad.numpy().copy(), "s": st["square_avg"].numpy().copy(), "b": st["momentum_buffer"].numpy().copy(),
            "p": p.detach().numpy().copy()}


def oracle_step_doubles(x, max_norm, hyper):
    """oracle/step_ref.py with the same doubles as stock torch."""
    t = {k: torch.from_numpy(x[k]).double() for k in "pgsb"}
    g = t["g"]
    if max_norm:
        g = g * S.clip_coef(g.norm(), max_norm)
    p2, s2, b2 = S.rmsprop_update(t["p"], g, t["s"], t["b"], hyper["lr"], alpha=hyper["alpha"], eps=hyper["eps"],
                                  weight_decay=hyper["wd"], momentum=hyper["mu"])
    return {"g": g.numpy(), "s": s2.numpy(), "b": b2.numpy(), "p": p2.numpy()}


# (name, hyper, state, gradient scale, max_norm): clipped and not, ordinary and first step
STOCK_CASES = [(f"{st}-{h}-x{gs:g}", h, st, gs, 1.0) for h in ("reference", "ema") for st in ("ordinary", "first") for gs in (1.0, 0.01)]


def stock_inputs(name, state, gscale):
    x = step_inputs(StepCase("stock-" + name, 4099, None, state, None, None))
    x["g"] = x["g"] * F(gscale)
    return x


def stock_distance(got, x, stock, ref, hyper):
    """Per element, relative to the magnitudes of the bounds: {"g", "s", "b", "p"} -> the worst |got - stock| / magnitude."""
    h = hyper32(hyper)
    mags = {"g": np.abs(ref["g"]), "s": ref["mag_s"], "b": ref["mag_b"],
            "p": np.abs(x["p"].astype(np.float64)) + np.abs(h["lr"] * ref["b"])}
    out = {}
    for k in "gsbp":
        err, m = np.abs(got[k].astype(np.float64) - stock[k]), mags[k]
        assert bool((err[m == 0] == 0).all()), k
        out[k] = float((err[m > 0] / m[m > 0]).max()) if bool((m > 0).any()) else 0.0
    return out


# ------------------------------------------------------------------------------------------------ the sum of squares
SUMSQ_SIZES = (1, 3, 4, 5, 1023, 1024, 1025, 4099, 2 ** 21, 2 ** 21 + 7)      # 2^21: exactly 2048 workgroups; + 7: second sweep, tail
SUMSQ_RANDOM = [(n, sc) for n in (3, 4099, 2 ** 21 + 7, WRAP) for sc in (1e-3, 1.0, 1e3)]


def grid(n, cap):
    return min(max((n // 4 + 255) // 256, 1), cap)


def integer_gradient(n):
    """Integers in [-3, 3]; the last element and the one at double_index(n) are 3: dropping the one or counting the other twice
    then moves the norm by 9 / (2 norm), six float32 ulps at the largest size."""
    g = np.random.default_rng(_seed("int", n)).integers(-3, 4, n).astype(F)
    for i in (n - 1, double_index(n)):
        g[i] = 3
    return g


def exact_norm(g):
    """The kernel's own two roundings of an exact integer sum: the double square root, then the float."""
    s = int((g.astype(np.int64) ** 2).sum())
    return F(np.sqrt(np.float64(s)))


def probe_indices(n):
    """0, the last element, every element of the tail, the last element of the first workgroup's first sweep, the first and the
    last element of the second sweep."""
    threads, n4 = grid(n, SUMSQ_MAXBLK) * 256, n // 4
    idx = {0, n - 1} | set(range(4 * n4, n))
    if n > 1023:
        idx.add(1023)
    if n4 > threads:
        idx |= {4 * threads, min(8 * threads, 4 * n4) - 1}
    return sorted(idx)


def sumsq_f32(g, mistake=None):
    """grad_sumsq_kernel + grad_norm_finish_kernel in numpy: the kernel's loop structure, every float32 operation rounded on its
    own.  -> (norm as float32, the float32 per-workgroup partials).  mistake: None | "dropped_tail" | "double" (the first element
    of the second sweep -- of the tail where there is no second sweep -- is counted twice)."""
    n = g.size
    if mistake == "dropped_tail":
        g = g.copy()
        g[-1] = 0
    nb = grid(n, SUMSQ_MAXBLK)
    T, n4 = nb * 256, n // 4
    sweeps = -(-n4 // T)
    grp = np.zeros((max(sweeps, 1) * T, 4), F)
    grp[:n4] = g[:4 * n4].reshape(n4, 4)
    acc = np.zeros(T, F)
    for k in range(sweeps):
        sq = grp[k * T:(k + 1) * T] ** 2
        acc = acc + (((sq[:, 0] + sq[:, 1]) + sq[:, 2]) + sq[:, 3])
    tail = g[4 * n4:]
    acc[:tail.size] += tail * tail
    if mistake == "double":
        i = double_index(n)
        acc[(i // 4) % T if i < 4 * n4 else i - 4 * n4] += g[i] * g[i]
    v = acc.reshape(nb, 4, 64)
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, :, lanes ^ o]
    red = v[:, :, 0]
    partials = ((red[:, 0] + red[:, 1]) + red[:, 2]) + red[:, 3]
    assert partials.dtype == F
    return F(np.sqrt(partials.astype(np.float64).sum())), partials


def double_index(n):
    """The element the mistake "double" counts twice: the first of the second sweep, of the tail where there is no second sweep,
    else the last."""
    threads = grid(n, SUMSQ_MAXBLK) * 256
    return 4 * threads if 4 * threads < n else min(n // 4 * 4, n - 1)


def norm_bound(norm64, frac=1.0):
    """SUMSQ_ULPS u on the sum is half of it on the root; the double finish and root (2^-50 at most), then the float rounding."""
    return (frac * SUMSQ_ULPS / 2 + 1) * U * norm64 + 2.0 ** -50 * norm64


def random_gradient(n, scale):
    return np.random.default_rng(_seed("rand", n, scale)).standard_normal(n, dtype=F) * F(scale)


def norm64(g):
    return float(np.sqrt((g.astype(np.float64) ** 2).sum()))


# ------------------------------------------------------------------------------------------------ FusedRMSprop
TOY_SHAPES = [(7, 5), (13,), (1,), (8, 3, 3, 3), (4,)]          # the fourth in channels_last
# fresh F / stale S over the optimizer's slices in the order of its flat buffer
PATTERNS = ("FFFFF", "SFFFF", "FFFFS", "FFSFF", "FSFSF", "FSSFF")
