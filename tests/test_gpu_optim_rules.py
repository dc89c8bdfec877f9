"""The AdamW and SGD rules of the fused optimizer pass (csrc/optim.hip) on the MI355X, op by op against float64: uh_adamw_step,
uh_sgd_step and their _ema forms through LIB.call; FusedAdamW / FusedSGD (train.py) with padding, strided views, stale slices, runs
and the device step counter; the state round trip; GraphedTrainStepper(optimizer="adamw"); the one-rank RCCL step.  Cases,
references and bounds are tests/optim_rule_cases.py's (derived in its docstring); tests/test_optim_rules_cpu.py shows on the CPU that
float32 arithmetic meets the bounds with half the room to spare and that each of 11 + 6 seeded mistakes breaks one.
tests/test_gpu_optim_rules_cli.py runs the command line.

Bounds, per element, fixed before any kernel ran (u = 2^-24; the float32 restatement's worst in brackets):
  g' = g coef   equal bits;
  AdamW   m' 10 u (|b1 m| + |(1 - b1) gc|) [2.42],  v' 15 u (b2 v + (1 - b2) gc^2) [3.62],
          p' 19 u (|p| + (lr / bc1) (|b1 m| + |(1 - b1) gc|) / (sqrt(v'64) / sqrt(bc2) + eps)) [4.67];
  SGD     b' 12 u (|mu b| + |gc| + |wd p|) [2.77],  p' 11 u (|p| + lr |d|) against p - lr d from the kernel's own b' [2.73];
  sharp first step (zero state, wd = 0, no clipping, p = 0), counted: m' 1.01, v' 2.01, p' 9.05 units;
  the distance to stock torch.optim.AdamW / SGD in float64 with the Python doubles: 2e-5 of the same magnitudes on p', m', b' and
  on v' / bc2 (the raw v' is not held: float32(0.999) moves 1 - b2 by 1.29e-5 relative, and bc2 moves with it);
  the average of the _ema forms: tests/test_gpu_ema.py's 6 u max(|p'|, |e|).

Measured on the MI355X (worst over the cases; the tests print each):
  AdamW, C ABI   g' equal everywhere; m' 2.41 units ("large"; bound 10), v' 3.61 ("wide"; bound 15), p' 4.40 (t = 2, the "strong"
                 hyper-parameters; bound 19); the 2^22 + 7 case at t = 1000: 2.23 / 2.30 / 2.70.
  sharp cases    m' 0.95, v' 1.88, p' 3.23 units (counted bounds 1.01, 2.01, 9.05): step = lr / bc1 and 1 / sqrt(bc2) are what
                 the double formation gives, and division and square root behave as correctly rounded ones.
  SGD, C ABI     g' equal everywhere; b' 2.76 units ("large"; bound 12), p' 2.00 (bound 11); 2^22 + 7: 2.64 / 2.00.
  stock torch    AdamW: v' / bc2 1.29e-5 on an ordinary state at t = 10 (float32(0.999): bc2 moves by that much and beta2 v does
                 not), p' 5.5e-6 (half of it, through the root), m' 3.0e-7; on a first step v' / bc2 3.1e-7 while the raw v' sits
                 at 1.32e-5.  With betas 0.5 / 0.9 everything is below 5e-7.  SGD: b' 1.8e-7, p' 6.9e-8.  Bound 2e-5.
  _ema forms     p, g and the state bit-identical to the plain forms at every size; the average inside 6 u.
  FusedAdamW     m' 1.53, v' 3.00, p' 1.67 units over seven steps and six fresh / stale patterns, with and without the average;
  FusedSGD       b' 1.60, p' 0.98; every equality (stale slices, zeroed stale gradients, padding lanes, the parameters' own views,
                 the counters of applied and of aborted steps) held."""
import os
import socket

import numpy as np
import pytest
import torch

import optim_cases as K
import optim_rule_cases as R

pytestmark = pytest.mark.gpu

F = np.float32
SENTINEL, TAIL = 1.0e18, 8
_name = lambda c: c.name      # noqa: E731
KEYS = {"adamw": "pgmv", "sgd": "pgb"}
EMA = (0.999, 10)                               # decay, warmup of the _ema calls


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    return torch.device("cuda", torch.cuda.current_device())


def _lib():
    import unet_amd  # noqa: F401
    from unet_amd._lib import LIB
    return LIB


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _up(a):
    t = torch.full((a.size + TAIL,), SENTINEL, dtype=torch.float32)
    t[:a.size] = torch.from_numpy(a)
    return t.to(_dev())


def _down(t, n):
    h = t.cpu()
    assert bool((h[n:] == SENTINEL).all()), "the kernel wrote behind n"
    return h[:n].numpy()


def _same_bits(a, b):
    return a.tobytes() == b.tobytes()


def _counter(value):
    return torch.tensor([int(value)], dtype=torch.int32, device=_dev())


def run_rule(rule, x, norm, max_norm, hyper, steps=None, ema=None, updates=0):
    """uh_<rule>_step (ema None) or uh_<rule>_step_ema (ema: the float32 array of the average) on copies of x.  norm: a float
    (passed as a device scalar), None (NULL) or a device tensor.  -> the outputs, "e" among them with ema, and the two counters
    as they are after the call ("steps", "updates": the pass itself must not tick)."""
    keys, n = KEYS[rule], x["p"].size
    d = {k: _up(x[k]) for k in keys}
    nd = norm if torch.is_tensor(norm) else (None if norm is None else torch.tensor([norm], dtype=torch.float32, device=_dev()))
    np_ = None if nd is None else nd.data_ptr()
    sc, uc = _counter(steps or 0), _counter(updates)
    bufs = [d[k].data_ptr() for k in keys]
    tail = []
    if ema is not None:
        d["e"] = _up(ema)
        bufs.append(d["e"].data_ptr())
        tail = [EMA[0], EMA[1], uc.data_ptr()]
    if rule == "adamw":
        args = [np_, float(max_norm), hyper["lr"], hyper["b1"], hyper["b2"], hyper["eps"], hyper["wd"], sc.data_ptr()]
    else:
        args = [np_, float(max_norm), hyper["lr"], hyper["wd"], hyper["mu"], int(hyper["nesterov"])]
    _lib().call(f"uh_{rule}_step" + ("_ema" if ema is not None else ""), *bufs, n, *args, *tail, _stream())
    torch.cuda.synchronize()
    out = {k: _down(d[k], n) for k in d}
    out["steps"], out["updates"] = int(sc.item()), int(uc.item())
    return out


def run_sumsq(g):
    LIB = _lib()
    gd = _up(g)
    out = torch.full((1,), -1.0, dtype=torch.float32, device=_dev())
    ws = torch.empty(LIB.query("uh_optim_ws_bytes", g.size), dtype=torch.uint8, device=_dev())
    LIB.call("uh_grad_sumsq", gd.data_ptr(), g.size, out.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
    torch.cuda.synchronize()
    return out


# ------------------------------------------------------------------------------------------------ the step, C ABI
@pytest.mark.parametrize("case", R.ADAMW_CASES, ids=_name)
def test_adamw_step_against_float64(case):
    x, h = R.inputs(case, "adamw"), R.ADAMW_HYPERS[case.hyper]
    coef = K.coef32(case.norm, case.max_norm)
    ref = R.adamw_reference(x, coef, h, case.steps)
    got = run_rule("adamw", x, case.norm, case.max_norm, h, case.steps)
    units = R.adamw_units(got, x, ref)
    print(f"{case.name}: coef {float(coef):.9g}, t {case.steps + 1}: {R.fmt_adamw(units)}")
    R.check_adamw(got, x, ref, what=case.name)
    assert got["steps"] == case.steps                               # the pass reads the counter and leaves it
    if case.max_norm == 0.0 or case.norm is None or case.name.startswith(("far_below", "t")):
        assert coef == 1
    assert _same_bits(got["g"], x["g"]) == (coef == 1)
    if case.state == "gzero":                                       # a first step without a gradient: 0 / eps = 0, only the decay moves p
        dead = x["g"] == 0
        assert not got["m"][dead].any() and not got["v"][dead].any()
        assert _same_bits(got["p"][dead & (x["p"] == 0)], x["p"][dead & (x["p"] == 0)])


@pytest.mark.parametrize("case", R.ADAMW_SHARP, ids=_name)
def test_adamw_sharp_first_step_says_how_the_bias_corrections_are_formed(case):
    x, h = R.inputs(case, "adamw"), R.ADAMW_HYPERS[case.hyper]
    ref = R.adamw_reference(x, F(1), h, 0)
    got = run_rule("adamw", x, case.norm, case.max_norm, h, 0)
    units = R.adamw_units(got, x, ref)
    print(f"{case.name}: {R.fmt_adamw(units)} (counted bounds {R.SHARP_M}, {R.SHARP_V}, {R.SHARP_P})")
    R.check_adamw(got, x, ref, km=R.SHARP_M, kv=R.SHARP_V, kp=R.SHARP_P, what=case.name)
    assert _same_bits(got["g"], x["g"])
    # m' / bc1 = g and v' / bc2 = g^2: the first update is -lr g / (|g| + eps), whatever the betas
    g64 = x["g"].astype(np.float64)
    hh = R.hyper32(h)
    want = -hh["lr"] * g64 / (np.abs(g64) + hh["eps"])
    assert bool((np.abs(got["p"] - want) <= (R.SHARP_P + 0.01) * R.U * np.abs(want)).all())       # (0.01: the reference's own doubles)


@pytest.mark.parametrize("case", R.SGD_CASES, ids=_name)
def test_sgd_step_against_float64(case):
    x, h = R.inputs(case, "sgd"), R.SGD_HYPERS[case.hyper]
    coef = K.coef32(case.norm, case.max_norm)
    ref = R.sgd_reference(x, coef, h)
    got = run_rule("sgd", x, case.norm, case.max_norm, h)
    units = R.sgd_units(got, x, ref, h)
    print(f"{case.name}: coef {float(coef):.9g}: {R.fmt_sgd(units)}")
    R.check_sgd(got, x, ref, h, what=case.name)
    if case.max_norm == 0.0 or case.norm is None or case.name.startswith("far_below"):
        assert coef == 1
    assert _same_bits(got["g"], x["g"]) == (coef == 1)
    if case.state in ("first", "gzero") and h["wd"] == 0 and coef == 1 and not h["nesterov"]:
        assert _same_bits(got["b"], x["g"])                         # torch's first step: the buffer IS the gradient


@pytest.mark.parametrize("rule", ["adamw", "sgd"])
@pytest.mark.parametrize("norm,max_norm", R.NONFINITE, ids=lambda v: str(v))
def test_non_finite_norm_leaves_every_buffer_and_both_counters_untouched(rule, norm, max_norm):
    h = R.ADAMW_HYPERS["torch"] if rule == "adamw" else R.SGD_HYPERS["nnunet"]
    for n in (5, 1025):
        x = R.inputs(R.RuleCase(f"nonfinite-{n}", n, None, "ordinary", norm, max_norm, 9), rule)
        e = np.random.default_rng(n).standard_normal(n, dtype=F)
        for ema in (None, e):
            got = run_rule(rule, x, norm, max_norm, h, steps=9, ema=ema, updates=4)
            for k in KEYS[rule]:
                assert _same_bits(got[k], x[k]), (k, n)
            assert ema is None or _same_bits(got["e"], e)
            assert (got["steps"], got["updates"]) == (9, 4)
        # ... and the tick behind them does not count the step either
        nd = torch.tensor([norm], dtype=torch.float32, device=_dev())
        for start in (9, 4):
            c = _counter(start)
            _lib().call("uh_ema_tick", c.data_ptr(), nd.data_ptr(), _stream())
            assert int(c.item()) == start


@pytest.mark.parametrize("name,hyper,state,gscale,max_norm,steps", R.STOCK_ADAMW, ids=[c[0] for c in R.STOCK_ADAMW])
def test_adamw_distance_to_stock_torch(name, hyper, state, gscale, max_norm, steps):
    x, h = R.stock_inputs("adamw", name, state, gscale), R.ADAMW_HYPERS[hyper]
    norm = run_sumsq(x["g"])
    got = run_rule("adamw", x, norm, max_norm, h, steps)
    stock = R.stock_adamw_step(x, max_norm, h, steps)
    ref = R.adamw_reference(x, K.coef32(float(norm.item()), max_norm), h, steps)
    d = R.stock_adamw_distance(got, stock, ref)
    raw = R.distance(got["v"], stock["v"], ref["mag_v"])
    print(f"{name}: to stock torch: " + ", ".join(f"{k} {v:.2e}" for k, v in d.items()) + f"; raw v' {raw:.2e} (not held)")
    assert max(d.values()) <= R.OP_TOL
    R.check_adamw(got, x, ref, what=name)


@pytest.mark.parametrize("name,hyper,state,gscale,max_norm,steps", R.STOCK_SGD, ids=[c[0] for c in R.STOCK_SGD])
def test_sgd_distance_to_stock_torch(name, hyper, state, gscale, max_norm, steps):
    x, h = R.stock_inputs("sgd", name, state, gscale), R.SGD_HYPERS[hyper]
    norm = run_sumsq(x["g"])
    got = run_rule("sgd", x, norm, max_norm, h)
    stock = R.stock_sgd_step(x, max_norm, h)
    ref = R.sgd_reference(x, K.coef32(float(norm.item()), max_norm), h)
    d = R.stock_sgd_distance(got, x, stock, ref, h)
    print(f"{name}: to stock torch: " + ", ".join(f"{k} {v:.2e}" for k, v in d.items()))
    assert max(d.values()) <= R.OP_TOL
    R.check_sgd(got, x, ref, h, what=name)


def test_hyper_parameter_ranges_and_alignment_are_refused():
    LIB = _lib()
    n = 8
    b = [torch.zeros(n + 4, dtype=torch.float32, device=_dev()) for _ in range(5)]
    c = _counter(0)
    ptr = [t.data_ptr() for t in b]
    ok_a = [None, 1.0, 1e-3, 0.9, 0.999, 1e-8, 0.01, c.data_ptr()]
    ok_s = [None, 1.0, 1e-2, 3e-5, 0.99, 1]
    LIB.call("uh_adamw_step", *ptr[:4], n, *ok_a, _stream())
    LIB.call("uh_sgd_step", *ptr[:3], n, *ok_s, _stream())
    bad_a = [(3, 1.0), (3, -0.1), (4, 1.0), (5, -1e-8), (6, -0.01), (2, -1e-3), (7, None)]
    for i, v in bad_a:
        args = list(ok_a)
        args[i] = v
        with pytest.raises(RuntimeError, match="uh_adamw_step"):
            LIB.call("uh_adamw_step", *ptr[:4], n, *args, _stream())
    for i, v in [(2, -1e-2), (3, -1.0), (4, -0.5), (5, 2)]:
        args = list(ok_s)
        args[i] = v
        with pytest.raises(RuntimeError, match="uh_sgd_step"):
            LIB.call("uh_sgd_step", *ptr[:3], n, *args, _stream())
    with pytest.raises(RuntimeError, match="nesterov"):
        LIB.call("uh_sgd_step", *ptr[:3], n, None, 1.0, 1e-2, 0.0, 0.0, 1, _stream())
    for k in range(4):                                              # one buffer off by a float: not 16-byte aligned
        p = list(ptr[:4])
        p[k] += 4
        with pytest.raises(RuntimeError, match="aligned"):
            LIB.call("uh_adamw_step", *p, n, *ok_a, _stream())
        if k < 3:
            with pytest.raises(RuntimeError, match="aligned"):
                LIB.call("uh_sgd_step", *p[:3], n, *ok_s, _stream())
    with pytest.raises(RuntimeError, match="bad args"):
        LIB.call("uh_adamw_step", ptr[0], None, ptr[2], ptr[3], n, *ok_a, _stream())
    with pytest.raises(RuntimeError, match="decay"):
        LIB.call("uh_sgd_step_ema", *ptr[:4], n, *ok_s, 1.0, 0, c.data_ptr(), _stream())
    with pytest.raises(RuntimeError, match="bad args"):
        LIB.call("uh_adamw_step_ema", *ptr[:5], n, *ok_a, 0.9, 0, None, _stream())
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the _ema forms
@pytest.mark.parametrize("rule", ["adamw", "sgd"])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 4099, K.WRAP])
def test_ema_form_is_bit_identical_and_its_average_is_held(rule, n):
    h = R.ADAMW_HYPERS["torch"] if rule == "adamw" else R.SGD_HYPERS["nnunet"]
    for norm, updates in ((0.25, 3), (7.5, 8991)):                   # below max_norm = 1 and above; inside the warm-up and behind it
        x = R.inputs(R.RuleCase(f"ema-{n}-{norm}", n, None, "ordinary", norm, 1.0, 9), rule)
        e = np.random.default_rng(n).standard_normal(n, dtype=F)
        plain = run_rule(rule, x, norm, 1.0, h, steps=9)
        avg = run_rule(rule, x, norm, 1.0, h, steps=9, ema=e, updates=updates)
        for k in KEYS[rule]:
            assert _same_bits(plain[k], avg[k]), (k, n, norm)
        assert (avg["steps"], avg["updates"]) == (9, updates)       # the pass does not tick
        assert not _same_bits(avg["e"], e)
        assert R.ema_within_bound(avg["e"], e, avg["p"], R.ema_c32(EMA[0], EMA[1], updates)), (n, norm)
    assert R.ema_c32(EMA[0], EMA[1], 8991) == F(1) - F(0.999) and R.ema_c32(EMA[0], EMA[1], 3) == F(1) - F(4) / F(13)


# ------------------------------------------------------------------------------------------------ FusedAdamW / FusedSGD
EMA_DECAY = 0.9


def _toy(rule, ema, **kw):
    """Five parameters (optim_cases.TOY_SHAPES, the 4-D one channels_last) under a FusedAdamW / FusedSGD."""
    import unet_amd
    g = torch.Generator().manual_seed(5)
    params = []
    for shape in K.TOY_SHAPES:
        t = torch.randn(shape, generator=g).to(_dev())
        if len(shape) == 4:
            t = t.contiguous(memory_format=torch.channels_last)
        params.append(torch.nn.Parameter(t))
    assert params[3].stride() == (27, 1, 9, 3)
    common = dict(ema_decay=EMA_DECAY if ema else None, ema_warmup=0, **kw)
    if rule == "adamw":
        opt = unet_amd.FusedAdamW(params, lr=1e-3, betas=(0.9, 0.999), weight_decay=0.01, **common)
    else:
        opt = unet_amd.FusedSGD(params, lr=1e-2, momentum=0.9, nesterov=True, weight_decay=1e-2, **common)
    assert isinstance(opt, unet_amd.FusedOptimizer) and not isinstance(opt, unet_amd.FusedRMSprop)
    assert [tuple(p.shape) for p in opt.params] == K.TOY_SHAPES[::-1] and opt.total == 276
    assert opt.slices == [(0, 4), (4, 216), (220, 1), (224, 13), (240, 35)]
    return opt, params


def _memory_order(t, p):
    flat = torch.empty(p.numel(), dtype=t.dtype, device=t.device)
    torch.as_strided(flat, p.shape, p.stride()).copy_(t)
    return flat


def _flat_buffers(opt):
    torch.cuda.synchronize()
    out = {"p": opt.flat_p, "g": opt.flat_g}
    out.update({"m": opt.flat_m, "v": opt.flat_v} if opt.KIND == "adamw" else {"b": opt.flat_buf})
    if opt.flat_ema is not None:
        out["e"] = opt.flat_ema
    return {k: v.cpu().numpy().copy() for k, v in out.items()}


def _hyper(opt):
    g = opt.param_groups[0]
    if opt.KIND == "adamw":
        return dict(lr=g["lr"], b1=g["beta1"], b2=g["beta2"], eps=g["eps"], wd=g["weight_decay"])
    return dict(lr=g["lr"], wd=g["weight_decay"], mu=g["momentum"], nesterov=g["nesterov"])


def _gradients(opt, kind, seed):
    r = torch.Generator().manual_seed(seed)
    if kind == "integers":
        return [(torch.randint(1, 4, p.shape, generator=r) * (2 * torch.randint(0, 2, p.shape, generator=r) - 1)).float()
                for p in opt.params]
    return [torch.randn(p.shape, generator=r) * kind for p in opt.params]


def _step(opt, pattern, grads, worst, steps_before):
    """One backward and step with the slices of `pattern` fresh, checked against a reference formed from a snapshot of the flat
    buffers (errors do not chain).  -> the norm."""
    rule, keys = opt.KIND, KEYS[opt.KIND]
    fresh = [c == "F" for c in pattern]
    opt.zero_grad()
    sum((p * g.to(p.device)).sum() for p, g, f in zip(opt.params, grads, fresh) if f).backward()
    before = _flat_buffers(opt)
    mem = [_memory_order(g, p).numpy() for p, g in zip(opt.params, grads)]
    for (o, n), m, f in zip(opt.slices, mem, fresh):
        if f:
            assert _same_bits(before["g"][o:o + n], m)
    h = _hyper(opt)
    norm = float(opt.step().item())
    after = _flat_buffers(opt)
    gf = np.concatenate([m for m, f in zip(mem, fresh) if f])
    if all(float(v) == round(float(v)) for v in gf):
        assert F(norm) == K.exact_norm(gf), (norm, pattern)
    else:
        assert abs(norm - K.norm64(gf)) <= K.norm_bound(K.norm64(gf)), (norm, K.norm64(gf), pattern)
    coef = K.coef32(norm, opt.gradient_clipping)
    pad = np.ones(opt.total, bool)
    for i, ((o, n), p, m, f) in enumerate(zip(opt.slices, opt.params, mem, fresh)):
        pad[o:o + n] = False
        if not f:
            for k in before:
                if k == "g":
                    assert not after["g"][o:o + n].any(), (pattern, i)
                else:
                    assert _same_bits(after[k][o:o + n], before[k][o:o + n]), (pattern, i, k)
            continue
        x = {k: before[k][o:o + n] for k in keys if k != "g"}
        x["g"] = m
        got = {k: after[k][o:o + n] for k in keys}
        if rule == "adamw":                                         # the optimizer's t, also for a slice that was stale before
            units = R.check_adamw(got, x, R.adamw_reference(x, coef, h, steps_before), what=f"{pattern} slice {i}")
        else:
            units = R.check_sgd(got, x, R.sgd_reference(x, coef, h), h, what=f"{pattern} slice {i}")
        for k in units:
            if k != "g":
                worst[k] = max(worst.get(k, 0.0), units[k])
        assert _same_bits(_memory_order(p.detach(), p).cpu().numpy(), got["p"]), (pattern, i)
        if "e" in before:
            assert R.ema_within_bound(after["e"][o:o + n], before["e"][o:o + n], got["p"], F(1) - F(EMA_DECAY)), (pattern, i)
    for k in after:
        assert not after[k][pad].any(), f"padding lanes of flat {k} after {pattern}"
    assert int(pad.sum()) == 276 - 269
    return norm


def _count(opt):
    return None if opt.step_count is None else int(opt.step_count.item())


@pytest.mark.parametrize("ema", [False, True], ids=["plain", "ema"])
@pytest.mark.parametrize("rule", ["adamw", "sgd"])
def test_fused_optimizer_steps_and_stale_patterns(rule, ema):
    opt, _ = _toy(rule, ema)
    assert _count(opt) == (0 if rule == "adamw" else None)
    assert (opt.step_count is None) == (rule == "sgd") and (opt.ema_updates is None) == (not ema)
    worst, norms = {}, []
    kinds = [1.0, "integers", 0.01, 1.0, "integers", 0.01]            # clipped (norm ~ 16), exact, not clipped (~ 0.16)
    for k, (pattern, kind) in enumerate(zip(K.PATTERNS, kinds)):
        norms.append(_step(opt, pattern, _gradients(opt, kind, 100 + k), worst, k))
        assert _count(opt) in (None, k + 1)                         # one per applied step, stale slices or not
        assert not ema or int(opt.ema_updates.item()) == k + 1
    assert norms[0] > 1 > norms[2]
    # a changed lr is used by the next step (the seventh), and the p bound can tell: with the old one it breaks
    opt.param_groups[0]["lr"] = opt.param_groups[0]["lr"] / 2
    before = _flat_buffers(opt)
    grads = _gradients(opt, 1.0, 200)
    norm = _step(opt, "FFFFF", grads, worst, 6)
    after = _flat_buffers(opt)
    o, n = opt.slices[1]
    keys = KEYS[rule]
    x = {k: before[k][o:o + n] for k in keys if k != "g"}
    x["g"] = _memory_order(grads[1], opt.params[1]).numpy()
    got = {k: after[k][o:o + n] for k in keys}
    old = dict(_hyper(opt), lr=_hyper(opt)["lr"] * 2)
    if rule == "adamw":
        assert R.adamw_breaks(R.adamw_units(got, x, R.adamw_reference(x, K.coef32(norm, 1.0), old, 6))) == ["p"]
    else:
        assert R.sgd_breaks(R.sgd_units(got, x, R.sgd_reference(x, K.coef32(norm, 1.0), old), old)) == ["p"]
    assert _count(opt) in (None, 7)
    # an aborted step (no backward since the last one; a NaN gradient) applies nothing and counts nothing
    with pytest.raises(RuntimeError, match=type(opt).__name__):
        opt.step()
    snap = [t.clone() for t in opt.state_tensors()]
    opt.zero_grad()
    bad = torch.ones_like(opt.params[0])
    bad.view(-1)[0] = float("nan")
    sum((p * (bad if i == 0 else torch.ones_like(p))).sum() for i, p in enumerate(opt.params)).backward()
    assert not np.isfinite(float(opt.step().item()))
    torch.cuda.synchronize()
    for t, s in zip(opt.state_tensors(), snap):
        assert torch.equal(t.view(torch.int32), s.view(torch.int32))
    assert _count(opt) in (None, 7)
    print(f"Fused{rule} ({'ema' if ema else 'plain'}): worst " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()) + " units")
    opt.close()


@pytest.mark.parametrize("rule", ["adamw", "sgd"])
def test_second_gradient_before_step_is_refused_by_name(rule):
    opt, params = _toy(rule, False)
    opt.zero_grad()
    (params[0] * 2).sum().backward()
    with pytest.raises(RuntimeError, match=f"{type(opt).__name__}: a second gradient"):
        (params[0] * 3).sum().backward()
    opt.close()


# ------------------------------------------------------------------------------------------------ state round trip
@pytest.mark.parametrize("ema", [False, True], ids=["plain", "ema"])
@pytest.mark.parametrize("rule", ["adamw", "sgd"])
def test_state_dict_round_trip_is_bit_identical(rule, ema):
    import unet_amd

    def steps(opt, first, count):
        for k in range(first, first + count):
            if k == 2:
                opt.param_groups[0]["lr"] *= 0.5                     # a changed lr travels with the state
            opt.zero_grad()
            sum((p * g.to(p.device)).sum() for p, g in zip(opt.params, _gradients(opt, 1.0, 400 + k))).backward()
            opt.step()

    whole, _ = _toy(rule, ema)
    steps(whole, 0, 5)
    want = _flat_buffers(whole)
    want_count = _count(whole)
    whole.close()
    first, _ = _toy(rule, ema)
    steps(first, 0, 3)
    state = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in first.state_dict().items()}
    p_saved = first.flat_p.clone()
    steps(first, 3, 1)                                               # the state is a copy: later steps do not reach it
    first.close()
    own = {"adamw": {"exp_avg", "exp_avg_sq", "step"}, "sgd": {"momentum_buffer"}}[rule]
    assert set(state) == {"kind", "ema", "ema_updates", "layout", "total", "hyper"} | own and state["kind"] == rule
    assert rule == "sgd" or state["step"] == 3
    assert state["ema_updates"] == (3 if ema else 0) and (state["ema"] is not None) == ema
    second, _ = _toy(rule, ema)                                       # (the same seeded initial values: overwritten next)
    with torch.no_grad():
        second.flat_p.copy_(p_saved)
    second.load_state_dict(state)
    assert second.param_groups[0]["lr"] == first.param_groups[0]["lr"] and _count(second) == (3 if rule == "adamw" else None)
    steps(second, 3, 2)
    got = _flat_buffers(second)
    assert sorted(got) == sorted(want) and _count(second) == want_count
    for k in want:
        assert _same_bits(got[k], want[k]), k
    # a state of another kind is refused, naming both; an RMSprop state has no "kind" and counts as another
    other_rule = "sgd" if rule == "adamw" else "adamw"
    other, _ = _toy(other_rule, ema)
    with pytest.raises(ValueError, match=f"(?s)'{rule}'.*'{other_rule}'"):
        other.load_state_dict(state)
    other.close()
    g = torch.Generator().manual_seed(5)
    rms = unet_amd.FusedRMSprop([torch.nn.Parameter(torch.randn(s, generator=g).to(_dev())) for s in K.TOY_SHAPES],
                                ema_decay=EMA_DECAY if ema else None, ema_warmup=0)
    with pytest.raises(ValueError, match=f"(?s)'{rule}'.*'rmsprop'"):
        rms.load_state_dict(state)
    rms_state = rms.state_dict()
    assert "kind" not in rms_state and set(rms_state) == {"square_avg", "momentum_buffer", "ema", "ema_updates", "layout", "total", "hyper"}
    with pytest.raises(ValueError, match=f"(?s)'rmsprop'.*'{rule}'"):
        second.load_state_dict(rms_state)
    rms.close()
    second.close()


# ------------------------------------------------------------------------------------------------ steppers
def _batches(n, size=64, first_seed=20):
    import unet_amd
    return [tuple(t.to(_dev()) for t in unet_amd.ellipse_batch(2, size, seed=first_seed + i)) for i in range(n)]


def _model(classes, seed=0):
    import unet_amd
    torch.manual_seed(seed)
    return unet_amd.UNet_T(1, classes).to(memory_format=torch.channels_last).to(_dev())


def _opt_state(st):
    torch.cuda.synchronize()
    return [t.clone() for t in st.optimizer.state_tensors()]


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_train_stepper_builds_the_optimizer_of_the_config():
    import unet_amd
    st = unet_amd.TrainStepper(_model(1), lr=1e-3, amp=False)
    assert type(st.optimizer) is unet_amd.FusedRMSprop and st.optim_config is None
    assert {k: st.optimizer.param_groups[0][k] for k in ("lr", "alpha", "eps", "weight_decay", "momentum")} == \
        dict(lr=1e-3, alpha=0.99, eps=1e-8, weight_decay=1e-8, momentum=0.999)
    assert len(st.optimizer.state_tensors()) == 3
    st.close()
    st = unet_amd.TrainStepper(_model(1), lr=1e-3, amp=False, optimizer="adamw,wd=0.05", gradient_clipping=2.0, ema="0.9")
    o = st.optimizer
    assert type(o) is unet_amd.FusedAdamW and st.optim_config == unet_amd.OptimConfig("adamw", wd=0.05)
    assert (o.param_groups[0]["lr"], o.param_groups[0]["weight_decay"], o.gradient_clipping) == (1e-3, 0.05, 2.0)
    assert len(o.state_tensors()) == 6 and o.state_tensors()[-2] is o.step_count and o.state_tensors()[-1] is o.ema_updates
    st.close()
    st = unet_amd.TrainStepper(_model(1), lr=1e-2, amp=False, optimizer=unet_amd.OptimConfig("sgd", momentum=0.9, nesterov=False))
    assert type(st.optimizer) is unet_amd.FusedSGD and st.optimizer.param_groups[0]["nesterov"] is False
    assert st.optimizer.step_count is None and len(st.optimizer.state_tensors()) == 2
    st.close()
    st = unet_amd.TrainStepper(_model(1), lr=1e-3, amp=False, weight_decay=0.5, optimizer="rmsprop,momentum=0.9")
    assert type(st.optimizer) is unet_amd.FusedRMSprop                  # the config is authoritative: not the stepper's weight_decay
    assert (st.optimizer.param_groups[0]["momentum"], st.optimizer.param_groups[0]["weight_decay"]) == (0.9, 1e-8)
    st.close()
    with pytest.raises(ValueError, match="adam"):
        unet_amd.TrainStepper(_model(1), optimizer="adam")


def test_graph_replays_adamw_with_their_own_step_number():
    import unet_amd
    data = _batches(3)
    eager = unet_amd.TrainStepper(_model(1), lr=1e-3, amp=False, optimizer="adamw")
    trail_eager = []
    for im, mk in data:
        eager.step(im, mk)
        trail_eager.append(_opt_state(eager))
    eager.close()
    st = unet_amd.GraphedTrainStepper(_model(1), lr=1e-3, amp=False, optimizer="adamw")
    assert type(st.optimizer) is unet_amd.FusedAdamW
    start = _opt_state(st)
    st._capture(*data[0])
    _same(_opt_state(st), start)                                     # the capture's warm-up steps do not count ...
    counts = [int(st.optimizer.step_count.item())]
    assert not st.optimizer.flat_m.any() and not st.optimizer.flat_v.any()           # ... and leave no moment behind
    for (im, mk), want in zip(data, trail_eager):
        st.step(im, mk)
        _same(_opt_state(st), want)                                  # each replay is the eager step with the same t, bit for bit
        counts.append(int(st.optimizer.step_count.item()))
    assert counts == [0, 1, 2, 3]
    st.close()


# ------------------------------------------------------------------------------------------------ data parallel, one rank
def _rccl_one_rank_adamw_worker(rank, world, port, q):
    try:
        import torch.distributed as dist
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        os.environ["UH_DP_FORCE_SYNC"] = "1"          # run the collectives although the group has one rank
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        dev = torch.device("cuda:0")
        torch.cuda.set_device(dev)
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
        import unet_amd
        torch.manual_seed(0)
        model = unet_amd.UNet_S(1, 1, bilinear=True).to(memory_format=torch.channels_last).to(dev)
        stepper = unet_amd.TrainStepper(model, lr=1e-4, amp=True, wgrad_stream=True, optimizer="adamw")
        sync = stepper.optimizer.sync
        assert sync is not None and sync.active and dist.get_backend() == "nccl"
        im, mk = unet_amd.ellipse_batch(4, 96, seed=3)
        for _ in range(3):
            t = stepper.step(im.to(dev), mk.to(dev))
        torch.cuda.synchronize()
        q.put((rank, "ok", stepper.optimizer.flat_p.cpu().numpy(), float(t["loss"]), len(sync.buckets),
               int(stepper.optimizer.step_count.item())))
        dist.destroy_process_group()
    except Exception:  # pragma: no cover
        import traceback
        q.put((rank, traceback.format_exc()))


def test_adamw_runs_over_rccl_with_one_rank():
    """tests/test_gpu_dp.py's one-rank check of the real backend with optimizer="adamw": every collective is the identity, so
    three steps leave the parameters bit-identical to a plain single-process run."""
    import torch.multiprocessing as mp
    import unet_amd
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = unet_amd.UNet_S(1, 1, bilinear=True).to(memory_format=torch.channels_last).to(dev)
    st = unet_amd.TrainStepper(model, lr=1e-4, amp=True, wgrad_stream=True, optimizer="adamw")
    im, mk = unet_amd.ellipse_batch(4, 96, seed=3)
    for _ in range(3):
        t = st.step(im.to(dev), mk.to(dev))
    torch.cuda.synchronize()
    ref_p, ref_loss = st.optimizer.flat_p.cpu(), float(t["loss"])
    st.optimizer.close()
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    proc = ctx.Process(target=_rccl_one_rank_adamw_worker, args=(0, 1, port, q))
    proc.start()
    try:
        res = q.get(timeout=300)
        proc.join(timeout=60)
    finally:
        if proc.is_alive():               # a rank that hangs must not outlive the test (it holds the GPU)
            proc.kill()
            proc.join(timeout=10)
    assert res[1] == "ok", res
    _, _, p, loss, nbuckets, count = res
    assert nbuckets >= 1 and count == 3
    assert loss == ref_loss and torch.equal(torch.from_numpy(p), ref_p)
