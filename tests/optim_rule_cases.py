"""Cases, float64 references, bounds, float32 restatements and seeded mistakes of the AdamW and SGD rules of the fused optimizer
pass (csrc/optim.hip: uh_adamw_step[_ema], uh_sgd_step[_ema]; train.FusedAdamW, train.FusedSGD), shared by
tests/test_gpu_optim_rules.py (the kernels on the MI355X) and tests/test_optim_rules_cpu.py (the CPU proof that float32 arithmetic
meets the bounds with half the room to spare and that each seeded mistake breaks one).  Nothing here needs a GPU.  The machinery
-- sizes, states, the clip coefficient, the unit count -- is tests/optim_cases.py's, which holds the RMSprop rule the same way.

References.  Primary (the one the bounds refer to): the rule in float64 on the float32 buffers, every hyper-parameter rounded to
float32 first (the C ABI takes float); 1 - beta the exact double difference of the rounded beta, which the float32 1.f - beta also
yields for beta in [1/2, 1); the bias corrections bc_i = 1 - beta_i^t, t = steps + 1, in double from the rounded betas.  The clip
coefficient is optim_cases.coef32, ONE float32 scalar.  Second: stock torch.optim.AdamW / torch.optim.SGD behind clip_grad_norm_ in
float64 with the Python doubles (stock_adamw_step, stock_sgd_step); the primary reference with the same doubles equals it to 1e-12.

AdamW, with gc = g coef:   m' = b1 m + (1 - b1) gc,   v' = b2 v + (1 - b2) gc^2,
                           p' = p (1 - lr wd) - (lr / bc1) m' / (sqrt(v') / sqrt(bc2) + eps)
SGD, with ge = gc + wd p:  b' = mu b + ge,   d = nesterov ? ge + mu b' : b',   p' = p - lr d

Bounds, per element, in units of u = 2^-24 of a magnitude taken from the float64 reference, plus what roundings below the normal
range may lose (2^-149 each):
  g' = g coef                                    equal bits
  AdamW m':  K_M u (|b1 m| + |(1 - b1) gc|)      + 3 * 2^-149                    (gc, b1 m, (1 - b1) gc)
  AdamW v':  K_V u (b2 v + (1 - b2) gc^2)        + 4 * 2^-149                    (gc, (1 - b2) gc, its product with gc, b2 v)
  AdamW p':  K_PA u (|p| + (lr / bc1) (|b1 m| + |(1 - b1) gc|) / den64)          + 2^-149 (3 + 3 (lr / bc1) / den64)
             den64 = sqrt(v'64) / sqrt(bc2) + eps; the floor: lr wd p, the quotient, its product, and m's three over den64
  SGD b':    K_BS u (|mu b| + |gc| + |wd p|)     + 3 * 2^-149
  SGD p':    against p - lr d formed from the kernel's own b' (d = b', or ge64 + mu b'):
             K_PS u (|p| + lr (|gc| + |wd p| + |mu b'|))                        + 4 * 2^-149
Each K is four times the worst of the numpy float32 restatement below (every operation rounded on its own; the kernel may contract
products and sums into FMAs, which only removes roundings) over every case, rounded up; the restatement's worst values, measured on
the CPU before any kernel ran:  m' 2.42, v' 3.62, AdamW p' 4.67, SGD b' 2.77, SGD p' 2.73.
The sharp cases (first step, zero state, wd = 0, no clipping, p = 0) are counted, not measured: see SHARP_*."""
import collections

import numpy as np
import torch

import optim_cases as K

F = K.F
U, DENORM, OP_TOL = K.U, K.DENORM, K.OP_TOL
# four times the restatement's worst over every case (2.42, 3.62, 4.67; 2.77, 2.73), rounded up; fixed before any kernel ran
K_M, K_V, K_PA = 10, 15, 19
K_BS, K_PS = 12, 11
FLOOR_M, FLOOR_V, FLOOR_BS, FLOOR_PS = 3 * DENORM, 4 * DENORM, 3 * DENORM, 4 * DENORM
# First step, zero state, wd = 0, no clipping, p = 0: m' = fl((1 - b1) g) is ONE rounding, v' = fl(fl((1 - b2) g) g) two, and
# p' = -fl(step fl(m' / den)), den = fl(fl(fl(sqrt v') rbc2) + eps): m' 1, v' 2 halved by the root 1, the root 1, rbc2 1, the product
# 1, the sum 1, the quotient 1, step 1, the product 1: nine roundings of |p'|, which is the whole magnitude.  With 0.01 for the
# second-order terms.  In exact arithmetic m' / bc1 = g and v' / bc2 = g^2 there, so p' = -lr g / (|g| + eps): a t that is off by
# one, a missing or a misplaced bias correction moves p' by far more (the mistakes below).
SHARP_M, SHARP_V, SHARP_P = 1.01, 2.01, 9.05

ADAMW_HYPERS = {
    "torch": dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.01),          # torch's defaults (OptimConfig's)
    "strong": dict(lr=0.1, b1=0.5, b2=0.9, eps=1e-6, wd=0.5),             # lr wd = 0.05: where the decay is applied shows
    "plain": dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.0),
}
SGD_HYPERS = {
    "nnunet": dict(lr=1e-2, wd=3e-5, mu=0.99, nesterov=True),             # OptimConfig's defaults
    "heavy": dict(lr=1e-2, wd=1e-2, mu=0.9, nesterov=False),
    "vanilla": dict(lr=1e-2, wd=0.0, mu=0.0, nesterov=False),
}
COUNTERS = (0, 1, 9, 999, 99999)           # steps[0] before the step; at the last b1^t has underflowed and bc1 = 1
CLIPS = (("far_below", 1e-3, 1.0), ("far_above", 1e4, 1.0), ("at_max_norm", 1.0, 1.0), ("just_below", K.BELOW_ONE, 1.0),
         ("just_above", K.ABOVE_ONE, 1.0), ("max_norm_half", 3.0, 0.5), ("max_norm_zero", 7.5, 0.0), ("norm_null", None, 1.0))
STATES = K.STATES + ("pzero",)             # pzero: ordinary with p = 0 on every third element: the update is the whole magnitude

RuleCase = collections.namedtuple("RuleCase", "name n hyper state norm max_norm steps")

ADAMW_CASES = (
    [RuleCase(f"n{n}-{h}", n, h, "ordinary", 7.5, 1.0, 9) for n in K.SIZES for h in ("torch", "strong")] +
    [RuleCase(f"{st}-{h}", 4099, h, st, 7.5, 1.0, 0 if st in ("first", "gzero") else 9) for st in STATES[1:] for h in ("torch", "strong")] +
    [RuleCase(f"t{t}-{h}", 1025, h, "pzero", 0.25, 1.0, t) for t in COUNTERS for h in ("torch", "strong")] +
    [RuleCase(f"{name}-torch", 1025, "torch", "ordinary", norm, mx, 9) for name, norm, mx in CLIPS] +
    [RuleCase("wrap", K.WRAP, "torch", "ordinary", 7.5, 1.0, 999)])
ADAMW_SHARP = [RuleCase(f"sharp-n{n}", n, "plain", "sharp", None, 0.0, 0) for n in (7, 4099)]
SGD_CASES = (
    [RuleCase(f"n{n}-{h}", n, h, "ordinary", 7.5, 1.0, None) for n in K.SIZES for h in SGD_HYPERS] +
    [RuleCase(f"{st}-{h}", 4099, h, st, 7.5, 1.0, None) for st in STATES[1:] for h in SGD_HYPERS] +
    [RuleCase(f"{name}-nnunet", 1025, "nnunet", "ordinary", norm, mx, None) for name, norm, mx in CLIPS] +
    [RuleCase("wrap", K.WRAP, "nnunet", "ordinary", 7.5, 1.0, None)])
NONFINITE = K.NONFINITE


def inputs(case, rule):
    """{"p", "g", "m", "v"} (adamw) or {"p", "g", "b"} (sgd): float32 arrays of case.n elements, optim_cases.step_inputs' states:
    m and b ~ 0.1 N(0,1), v ~ 0.01 U(0,1) (0 on a first step; see there for gzero, wide, large).  sharp: a first step with p = 0."""
    base = {"pzero": "ordinary", "sharp": "first"}.get(case.state, case.state)
    x = K.step_inputs(K.StepCase(f"{rule}-{case.name}", case.n, None, base, None, None))
    if case.state == "pzero":
        x["p"][::3] = 0
    if case.state == "sharp":
        x["p"][:] = 0
    return {"p": x["p"], "g": x["g"], "m": x["b"], "v": x["s"]} if rule == "adamw" else {"p": x["p"], "g": x["g"], "b": x["b"]}


def hyper32(h):
    """The values the kernel receives: each number rounded to float32, as Python doubles (nesterov stays a bool)."""
    return {k: (v if isinstance(v, bool) else float(F(v))) for k, v in h.items()}


def bias_corrections(b1, b2, steps):
    """bc1, bc2 in double from the given betas and t = steps + 1."""
    t = int(steps) + 1
    return 1.0 - float(b1) ** t, 1.0 - float(b2) ** t


# ------------------------------------------------------------------------------------------------ AdamW
def adamw_reference(x, coef, hyper, steps, rounded=True):
    """The primary reference.  -> float64 arrays g, m, v, p, the magnitudes mag_m, mag_v, mag_p, floor_p, and vhat = v' / bc2."""
    h = hyper32(hyper) if rounded else dict(hyper)
    p, g, m, v = (x[k].astype(np.float64) for k in "pgmv")
    bc1, bc2 = bias_corrections(h["b1"], h["b2"], steps)
    gc = g * float(coef)
    m2 = h["b1"] * m + (1 - h["b1"]) * gc
    v2 = h["b2"] * v + (1 - h["b2"]) * gc * gc
    den = np.sqrt(v2) / np.sqrt(bc2) + h["eps"]
    step = h["lr"] / bc1
    p2 = p * (1 - h["lr"] * h["wd"]) - step * m2 / den
    mag_m = np.abs(h["b1"] * m) + np.abs((1 - h["b1"]) * gc)
    return {"g": gc, "m": m2, "v": v2, "p": p2, "mag_m": mag_m, "mag_v": h["b2"] * v + (1 - h["b2"]) * gc * gc,
            "mag_p": np.abs(p) + step * mag_m / den, "floor_p": DENORM * (3 + 3 * step / den), "vhat": v2 / bc2, "bc2": bc2}


def adamw_f32(x, coef, hyper, steps, mistake=None, at=None):
    """adamw_kernel's statements in numpy float32, every operation rounded on its own.  mistake: one of ADAMW_MISTAKES."""
    h = {k: F(v) for k, v in hyper.items()}
    one, coef = F(1), F(coef)
    t = int(steps) + (0 if mistake == "t_not_t_plus_1" else 1)
    with np.errstate(divide="ignore", under="ignore", over="ignore"):
        if mistake == "bc_in_float32":
            bc1, bc2 = one - np.power(h["b1"], F(t)), one - np.power(h["b2"], F(t))
            step, rbc2 = h["lr"] / bc1, one / np.sqrt(bc2)
        elif mistake == "no_bias_correction":
            step, rbc2 = h["lr"], one
        else:
            bc1, bc2 = 1.0 - float(h["b1"]) ** t, 1.0 - float(h["b2"]) ** t
            step, rbc2 = F(np.float64(h["lr"]) / bc1), F(1.0 / np.sqrt(np.float64(bc2)))
    lrwd = h["lr"] * h["wd"]
    assert all(isinstance(s, np.float32) for s in (step, rbc2, lrwd))

    def update(p, g, m, v):
        gc = g * coef
        gm = gc + h["wd"] * p if mistake == "l2_decay" else gc
        m2 = h["b1"] * m + (one - h["b1"]) * gm
        v2 = h["b2"] * v + (one - h["b2"]) * gm * gm
        root = np.sqrt(v if mistake == "old_second_moment" else v2)
        if mistake == "eps_inside_root":
            den = np.sqrt(v2 + h["eps"]) * rbc2
        elif mistake == "eps_before_bc":
            den = (root + h["eps"]) * rbc2
        else:
            den = root * rbc2 + h["eps"]
        if mistake == "l2_decay":
            p2 = p - step * (m2 / den)
        elif mistake == "decay_on_updated":
            pu = p - step * (m2 / den)
            p2 = pu - lrwd * pu
        else:
            p2 = (p - lrwd * p) - step * (m2 / den)
        return p2, (g if mistake == "g_left_unscaled" else gc), m2, v2

    with np.errstate(under="ignore", over="ignore", invalid="ignore", divide="ignore"):
        out = [a.astype(F) for a in update(x["p"], x["g"], x["m"], x["v"])]
        if mistake == "dropped_tail":
            for a, k in zip(out, "pgmv"):
                a[-1] = x[k][-1]
        if mistake == "double":
            again = update(*(a[at:at + 1] for a in out))
            for a, v in zip(out, again):
                a[at] = v[0]
    assert all(a.dtype == F for a in out)
    return dict(zip("pgmv", out))


ADAMW_MISTAKES = ("l2_decay", "no_bias_correction", "t_not_t_plus_1", "bc_in_float32", "eps_inside_root", "eps_before_bc",
                  "decay_on_updated", "old_second_moment", "g_left_unscaled", "dropped_tail", "double")


def _units(got, want, mag, floor):
    """optim_cases._units; a value that is not finite counts as infinitely far."""
    if not bool(np.isfinite(got).all()):
        return float("inf")
    return K._units(np.abs(got - want), mag, floor)


def _g_differs(got, ref):
    return int((got["g"].view(np.int32) != ref["g"].astype(F).view(np.int32)).sum())


def adamw_units(got, x, ref):
    for k in "pgmv":
        assert got[k].dtype == F and got[k].shape == x[k].shape, k
    return {"g": _g_differs(got, ref), "m": _units(got["m"], ref["m"], ref["mag_m"], FLOOR_M),
            "v": _units(got["v"], ref["v"], ref["mag_v"], FLOOR_V), "p": _units(got["p"], ref["p"], ref["mag_p"], ref["floor_p"])}


def adamw_breaks(units, km=K_M, kv=K_V, kp=K_PA):
    return [k for k, lim in (("g", 0), ("m", km), ("v", kv), ("p", kp)) if units[k] > lim]


def check_adamw(got, x, ref, km=K_M, kv=K_V, kp=K_PA, what=""):
    units = adamw_units(got, x, ref)
    assert not adamw_breaks(units, km, kv, kp), f"{what}: {units} against g == , m {km}, v {kv}, p {kp}"
    return units


def fmt_adamw(units):
    return f"g {units['g']} differ, m {units['m']:.2f}, v {units['v']:.2f}, p {units['p']:.2f} units"


# ------------------------------------------------------------------------------------------------ SGD
def sgd_reference(x, coef, hyper, rounded=True):
    """The primary reference.  -> float64 arrays g, b, p, ge (= gc + wd p), and the magnitude mag_b."""
    h = hyper32(hyper) if rounded else dict(hyper)
    p, g, b = (x[k].astype(np.float64) for k in "pgb")
    gc = g * float(coef)
    ge = gc + h["wd"] * p
    b2 = h["mu"] * b + ge
    d = ge + h["mu"] * b2 if h["nesterov"] else b2
    return {"g": gc, "b": b2, "p": p - h["lr"] * d, "ge": ge, "mag_b": np.abs(h["mu"] * b) + np.abs(gc) + np.abs(h["wd"] * p),
            "mag_ge": np.abs(gc) + np.abs(h["wd"] * p)}


def sgd_f32(x, coef, hyper, mistake=None, at=None):
    """sgd_update's statements in numpy float32, every operation rounded on its own.  mistake: one of SGD_MISTAKES."""
    h = {k: (v if isinstance(v, bool) else F(v)) for k, v in hyper.items()}
    coef = F(coef)
    nesterov = h["nesterov"] and mistake != "plain_for_nesterov"

    def update(p, g, b):
        gc = g * coef
        ge = (g + h["wd"] * p) * coef if mistake == "decay_scaled_too" else gc + h["wd"] * p
        b2 = h["mu"] * b + ((F(1) - h["mu"]) * ge if mistake == "dampened" else ge)
        d = (ge + h["mu"] * (b if mistake == "nesterov_from_old_buffer" else b2)) if nesterov else b2
        return p - h["lr"] * d, gc, b2

    with np.errstate(under="ignore"):
        out = [a.astype(F) for a in update(x["p"], x["g"], x["b"])]
        if mistake == "dropped_tail":
            for a, k in zip(out, "pgb"):
                a[-1] = x[k][-1]
        if mistake == "double":
            again = update(*(a[at:at + 1] for a in out))
            for a, v in zip(out, again):
                a[at] = v[0]
    assert all(a.dtype == F for a in out)
    return dict(zip("pgb", out))


SGD_MISTAKES = ("nesterov_from_old_buffer", "plain_for_nesterov", "decay_scaled_too", "dampened", "dropped_tail", "double")


def sgd_units(got, x, ref, hyper):
    """b' against the reference; p' against p - lr d with d formed from the b' that was returned."""
    for k in "pgb":
        assert got[k].dtype == F and got[k].shape == x[k].shape, k
    h = hyper32(hyper)
    p64, b_got = x["p"].astype(np.float64), got["b"].astype(np.float64)
    d = ref["ge"] + h["mu"] * b_got if h["nesterov"] else b_got
    mag_d = ref["mag_ge"] + np.abs(h["mu"] * b_got) if h["nesterov"] else np.abs(b_got)
    return {"g": _g_differs(got, ref), "b": _units(got["b"], ref["b"], ref["mag_b"], FLOOR_BS),
            "p": _units(got["p"], p64 - h["lr"] * d, np.abs(p64) + h["lr"] * mag_d, FLOOR_PS)}


def sgd_breaks(units, kb=K_BS, kp=K_PS):
    return [k for k, lim in (("g", 0), ("b", kb), ("p", kp)) if units[k] > lim]


def check_sgd(got, x, ref, hyper, what=""):
    units = sgd_units(got, x, ref, hyper)
    assert not sgd_breaks(units), f"{what}: {units} against g == , b {K_BS}, p {K_PS}"
    return units


def fmt_sgd(units):
    return f"g {units['g']} differ, b {units['b']:.2f}, p {units['p']:.2f} units"


# ------------------------------------------------------------------------------------------------ stock torch
def _clipped(p, x, max_norm):
    p.grad = torch.from_numpy(x["g"]).double()
    if max_norm:
        torch.nn.utils.clip_grad_norm_([p], max_norm)


def stock_adamw_step(x, max_norm, hyper, steps):
    """clip_grad_norm_ + torch.optim.AdamW(amsgrad=False) in float64 with the Python doubles, the norm the gradient's own, the
    state that of `steps` earlier steps.  -> float64 arrays g, m, v, p and vhat = v' / bc2."""
    p = torch.nn.Parameter(torch.from_numpy(x["p"]).double())
    opt = torch.optim.AdamW([p], lr=hyper["lr"], betas=(hyper["b1"], hyper["b2"]), eps=hyper["eps"], weight_decay=hyper["wd"],
                            amsgrad=False, foreach=False)
    opt.state[p] = {"step": torch.tensor(float(steps)), "exp_avg": torch.from_numpy(x["m"]).double(),
                    "exp_avg_sq": torch.from_numpy(x["v"]).double()}
    _clipped(p, x, max_norm)
    opt.step()
    st = opt.state[p]
    assert float(st["step"]) == steps + 1
    v = st["exp_avg_sq"].numpy().copy()
    return {"g": p.grad.numpy().copy(), "m": st["exp_avg"].numpy().copy(), "v": v, "p": p.detach().numpy().copy(),
            "vhat": v / bias_corrections(hyper["b1"], hyper["b2"], steps)[1]}


def stock_sgd_step(x, max_norm, hyper):
    """clip_grad_norm_ + torch.optim.SGD(dampening=0) in float64 with the Python doubles.  -> float64 arrays g, b, p."""
    p = torch.nn.Parameter(torch.from_numpy(x["p"]).double())
    opt = torch.optim.SGD([p], lr=hyper["lr"], momentum=hyper["mu"], dampening=0, weight_decay=hyper["wd"],
                          nesterov=hyper["nesterov"], foreach=False)
    assert hyper["mu"] > 0
    opt.state[p] = {"momentum_buffer": torch.from_numpy(x["b"]).double()}
    _clipped(p, x, max_norm)
    opt.step()
    return {"g": p.grad.numpy().copy(), "b": opt.state[p]["momentum_buffer"].numpy().copy(), "p": p.detach().numpy().copy()}


def clip_coef_doubles(g, max_norm):
    """clip_grad_norm_'s coefficient in float64 (oracle/step_ref.py's clip_coef)."""
    return float(K.S.clip_coef(torch.from_numpy(g).double().norm(), max_norm)) if max_norm else 1.0


# (name, hyper, state, gradient scale, max_norm, steps): clipped and not, ordinary and first step
STOCK_ADAMW = [(f"{st}-{h}-x{gs:g}", h, st, gs, 1.0, 0 if st == "first" else 9) for h in ("torch", "strong")
               for st in ("ordinary", "first") for gs in (1.0, 0.01)]
STOCK_SGD = [(f"{st}-{h}-x{gs:g}", h, st, gs, 1.0, None) for h in ("nnunet", "heavy") for st in ("ordinary", "first") for gs in (1.0, 0.01)]


def stock_inputs(rule, name, state, gscale):
    x = inputs(RuleCase("stock-" + name, 4099, None, state, None, None, None), rule)
    x["g"] = x["g"] * F(gscale)
    return x


def distance(got, want, mag):
    """The worst |got - want| / mag over the elements; where the magnitude is 0 the two must agree."""
    err = np.abs(np.asarray(got, np.float64) - want)
    assert bool((err[mag == 0] == 0).all())
    return float((err[mag > 0] / mag[mag > 0]).max()) if bool((mag > 0).any()) else 0.0


def stock_adamw_distance(got, stock, ref):
    """{"m", "vhat", "p"} -> the kernel's distance to stock torch relative to the bounds' magnitudes.  The raw v' is not held:
    float32(0.999) makes 1.f - b2 differ from 0.001 by 1.29e-5 relative, which v' / bc2 cancels (bc2 shifts with it)."""
    return {"m": distance(got["m"], stock["m"], ref["mag_m"]),
            "vhat": distance(got["v"].astype(np.float64) / ref["bc2"], stock["vhat"], ref["mag_v"] / ref["bc2"]),
            "p": distance(got["p"], stock["p"], ref["mag_p"])}


def stock_sgd_distance(got, x, stock, ref, hyper):
    h = hyper32(hyper)
    return {"b": distance(got["b"], stock["b"], ref["mag_b"]),
            "p": distance(got["p"], stock["p"], np.abs(x["p"].astype(np.float64)) + h["lr"] * (ref["mag_b"] + ref["mag_ge"]))}


# ------------------------------------------------------------------------------------------------ the average
def ema_c32(decay, warmup, t):
    """c = 1 - d_t in float32 as the kernels form it (tests/test_gpu_ema.py)."""
    d = F(decay)
    if warmup > 0:
        tf = F(t)
        d = np.minimum(d, (F(1) + tf) / (F(warmup) + tf))
    return F(1) - F(d)


def ema_within_bound(e_got, e_prev, p_new, c):
    """tests/test_gpu_ema.py's bound: three float32 roundings of values of magnitude at most 2 max(|p|, |e|): 6 u of that."""
    e, p = e_prev.astype(np.float64), p_new.astype(np.float64)
    return bool((np.abs(e_got - (e + np.float64(c) * (p - e))) <= 6 * U * np.maximum(np.abs(p), np.abs(e))).all())
