"""The optimizer pass (csrc/optim.hip) on the MI355X, op by op against float64: uh_grad_sumsq, uh_rmsprop_step and uh_swap_f32
through LIB.call, and FusedRMSprop.step (train.py) with its padding, strided views, stale slices and runs.  Cases, references and
bounds are tests/optim_cases.py's; tests/test_optim_cpu.py shows on the CPU that float32 arithmetic meets the bounds with half the
room to spare and that each of ten seeded mistakes breaks one.  tests/test_gpu_ema.py shows that uh_rmsprop_step_ema writes the same
bits to p / g / sq / buf as uh_rmsprop_step, so what is pinned here is pinned for both.

References.  Primary: oracle/step_ref.py's rmsprop_update in float64 on the values the kernel receives -- float32 buffers, every
hyper-parameter rounded to float32 (the C ABI takes float), 1 - alpha the float32 1.f - alpha = 0.00999999046 (exact, so the double
1 - alpha of the rounded alpha is the same number), and the clip coefficient the ONE float32 scalar fminf(max_norm / (norm + 1e-6f),
1.f), which the equality g' = g * coef pins and the CPU companion holds to step_ref.clip_coef within two roundings.
Second: stock torch.optim.RMSprop(momentum > 0, centered=False) behind clip_grad_norm_ in float64 with the Python doubles
(alpha = 0.99, value = 1 - alpha = 0.01).  The kernel is HELD to the primary reference and its distance to stock torch is held to
the project's op-by-op 2e-5 per element and recorded: the two 1 - alpha differ by 9.5e-7 relative (9.3e-7 against a float32 stock
torch, which rounds the double 1 - alpha once), 16 u.  On a first step sq' = (1 - alpha) ge^2 takes all of it and the quotient
half; on later steps it fades with alpha.  Neither is "right"; the sharp cases below are what says which one the kernel forms.

Bounds, per element, never a norm over the vector, fixed before any kernel ran.  u = 2^-24, everything from the float64 reference,
A = |g coef| + |wd p| the magnitude that feeds ge = g coef + wd p (which cancels: to 1e-5 of A on ordinary inputs with wd = 1e-2),
q = ge / (sqrt(sq') + eps):
  * g' = g coef: one float32 product, nothing to contract: equal bits.  coef = 1 (max_norm <= 0, total_norm NULL, a norm below
    max_norm): the bits of g itself.
  * sq':  |got - s64| <= K_S u (alpha sq + (1 - alpha) A^2) + 5 * 2^-149
  * buf': |got - b64| <= K_B u (|mu buf| + |q| + A / (sqrt(s64) + eps)) + 2^-149 (2 + 2 / (sqrt(s64) + eps))
  * p' apart from buf', as the loss gradients are apart from the sums: with the kernel's own float32 b',
          |got - (p - lr b')| <= K_P u (|p| + |lr b'|) + 2^-149.
    K_S, K_B, K_P = 19, 10, 8: four times the worst of a numpy float32 restatement of the statements, every operation rounded on
    its own, over every case (4.63, 2.33, 1.77), rounded up.  The kernel may contract into FMAs, which removes roundings.
    Division and square root are presumed correctly rounded (-O3, no fast-math); the sharp cases would show if they were not.
  * The floors: what a rounding below the normal range may lose, 2^-149 each.  sq': g coef, wd p (each moves ge, and sq' by
    2 (1 - alpha) |ge| < 1 times as much while ge is that small), (1 - alpha) ge, its product with ge, alpha sq: 5; the sums
    of two such numbers are exact.  buf': the two in ge, divided by the denominator; mu buf and the quotient: 2; what sq' lost
    moves its root by at most sqrt(5 * 2^-149) = 8e-23, 8e-15 of eps.  p': the product lr b'.  The case "tiny" (wd = 0,
    |g| ~ 1e-20, sq = 0: sq' ~ 1e-42) lives on the floor: its error is 1e5 times K_S u sq'.
  * Sharp cases (wd = 0, mu = 0, no clipping, sq = buf = 0), counted, not measured: sq' = fl(fl((1 - alpha) g) g) has two
    roundings, 2 u sq'; buf' = g / fl(fl(sqrt(sq')) + eps) half of those, the root, the sum and the quotient, 4 u |q|, which is 2 u
    of the magnitude 2 |q|; both with 0.01 for the second-order terms.  Stock torch's 1 - alpha would sit at 16 and 4 units there,
    and inside K_S and K_B anywhere else.
  * uh_grad_sumsq.  Integers in [-3, 3]: every thread's and workgroup's partial is an integer below 2^24, the finish is in double:
    the norm equals float32(sqrt(float64(S))).  One 3.0 anywhere: exactly 3.  Random N(0,1) x {1e-3, 1, 1e3}, all terms
    non-negative: at n = 2^22 + 7 (2^20 + 1 groups of four over 2^19 threads) a thread adds at most 3 groups and a tail element:
    the square 1, the three adds inside a group 3, the adds to the accumulator 3 + 1: 8; six shuffle levels 6; three LDS adds
    3: 17 u of S64, half of that for the root, 1 for the float rounding (the double finish and root: 2^-50):
          |got - norm64| <= 9.5 u norm64.
    A gradient whose squares, or their sum, overflow float32 gives +inf, and the step behind it leaves every buffer untouched.
  * FusedRMSprop: each step's reference is formed from a snapshot of the flat buffers, so errors do not chain and the bounds above
    hold unchanged; stale slices, padding lanes and gradient_clipping=None are equalities.

Measured on the MI355X (worst over the cases; the tests print each):
  step, C ABI    g' equal everywhere; sq' 4.63 units at the first step (bound 19; the float32 restatement 4.63), buf' 2.30 at
                 n = 2^22 (bound 10; the restatement 2.33), p' 1.00 (bound 8; the restatement 1.77: the kernel forms p - lr b' as
                 one FMA).  The 2^22 and 2^22 + 7 cases: 3.52 / 2.30 / 1.00 and 3.19 / 2.21 / 1.00.  "tiny": sq' inside the floor.
  sharp cases    sq' 1.81, buf' 1.39 units (counted bounds 2.01): the kernel forms the float32 1.f - alpha, and its division and
                 square root behave as correctly rounded ones.
  stock torch    largest on the first step: sq' 1.23e-6 (20.7 u) of its magnitude, buf' 3.2e-7 (5.4 u), p' 6.0e-7 (10.1 u, where
                 |p| is small and lr b' is the magnitude), g' 9.2e-8 (the float32 coefficient); on an ordinary state sq' 6.5e-7,
                 buf' 2.6e-7.  Bound 2e-5.  Cause: 1.f - alpha against the double 1 - alpha, 9.5e-7, plus the kernel's own roundings.
  sum of squares integers equal at every size (the double square root gave the correctly rounded value each time), every probe
                 exactly 3; random gradients 0.50 u of the norm at most (bound 9.5); overflow: +inf and an untouched step.
  FusedRMSprop   sq' 3.19, buf' 1.31, p' 0.97 units over seven steps and six fresh / stale patterns, with and without the average;
                 every equality (stale slices, zeroed stale gradients, padding lanes, the parameters' own views, no clipping) held."""
import numpy as np
import pytest
import torch

import optim_cases as K

pytestmark = pytest.mark.gpu

F = np.float32
SENTINEL, TAIL = 1.0e18, 8                     # behind the n elements (its square is finite: a read past n shows in the norm)
_name = lambda c: c.name      # noqa: E731


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
    """A device buffer of a.size + TAIL floats: the array, then the sentinel."""
    t = torch.full((a.size + TAIL,), SENTINEL, dtype=torch.float32)
    t[:a.size] = torch.from_numpy(a)
    return t.to(_dev())


def _down(t, n):
    """-> the first n elements as a numpy array; the sentinel behind them must have survived."""
    h = t.cpu()
    assert bool((h[n:] == SENTINEL).all()), "the kernel wrote behind n"
    return h[:n].numpy()


def _norm_dev(norm):
    return None if norm is None else torch.tensor([norm], dtype=torch.float32, device=_dev())


def run_step(x, norm, max_norm, hyper):
    """uh_rmsprop_step on copies of x["p" "g" "s" "b"]; norm: a float (passed as a device scalar), None (NULL) or a device tensor."""
    n = x["p"].size
    d = {k: _up(x[k]) for k in "pgsb"}
    nd = norm if torch.is_tensor(norm) else _norm_dev(norm)
    _lib().call("uh_rmsprop_step", d["p"].data_ptr(), d["g"].data_ptr(), d["s"].data_ptr(), d["b"].data_ptr(), n,
                None if nd is None else nd.data_ptr(), float(max_norm), hyper["lr"], hyper["alpha"], hyper["eps"], hyper["wd"],
                hyper["mu"], _stream())
    torch.cuda.synchronize()
    return {k: _down(d[k], n) for k in "pgsb"}


def run_sumsq(g):
    """uh_grad_sumsq -> the 1-element device tensor."""
    LIB = _lib()
    n = g.size
    gd = _up(g)
    out = torch.full((1,), -1.0, dtype=torch.float32, device=_dev())
    ws = torch.empty(LIB.query("uh_optim_ws_bytes", n), dtype=torch.uint8, device=_dev())
    LIB.call("uh_grad_sumsq", gd.data_ptr(), n, out.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
    torch.cuda.synchronize()
    return out


def _same_bits(a, b):
    return a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------ the step, C ABI
@pytest.mark.parametrize("case", K.STEP_CASES, ids=_name)
def test_step_against_float64(case):
    x, h = K.step_inputs(case), K.HYPERS[case.hyper]
    coef = K.coef32(case.norm, case.max_norm)
    ref = K.step_reference(x, coef, h)
    got = run_step(x, case.norm, case.max_norm, h)
    units = K.step_units(got, x, ref, h)
    print(f"{case.name}: coef {float(coef):.9g}: {K.fmt_units(units)}")
    K.check_step(got, x, ref, h, what=case.name)
    if case.max_norm == 0.0 or case.norm is None or case.name.startswith("far_below"):
        assert coef == 1
    assert _same_bits(got["g"], x["g"]) == (coef == 1)              # coef = 1: the gradient keeps its bits
    if case.state == "gzero":                                       # 0 / eps = 0: nothing moves, nothing becomes NaN
        dead = (x["g"] == 0) & ((x["p"] == 0) | (h["wd"] == 0))
        assert int(dead.sum()) >= case.n // 8
        assert not got["s"][dead].any() and not got["b"][dead].any() and _same_bits(got["p"][dead], x["p"][dead])


@pytest.mark.parametrize("case", K.SHARP_CASES, ids=_name)
def test_sharp_first_step_says_which_one_minus_alpha(case):
    x, h = K.step_inputs(case), K.HYPERS[case.hyper]
    ref = K.step_reference(x, F(1), h)
    got = run_step(x, case.norm, case.max_norm, h)
    units = K.step_units(got, x, ref, h)
    print(f"{case.name}: {K.fmt_units(units)} (counted bounds {K.SHARP_S}, {K.SHARP_B})")
    K.check_step(got, x, ref, h, ks=K.SHARP_S, kb=K.SHARP_B, what=case.name)
    assert _same_bits(got["g"], x["g"])


@pytest.mark.parametrize("norm,max_norm", K.NONFINITE, ids=lambda v: str(v))
def test_non_finite_norm_leaves_every_buffer_untouched(norm, max_norm):
    for n in (5, 1025):
        x = K.step_inputs(K.StepCase(f"nonfinite-{n}", n, "ema", "ordinary", norm, max_norm))
        got = run_step(x, norm, max_norm, K.HYPERS["ema"])
        for k in "pgsb":
            assert _same_bits(got[k], x[k]), (k, n)


@pytest.mark.parametrize("name,hyper,state,gscale,max_norm", K.STOCK_CASES, ids=[c[0] for c in K.STOCK_CASES])
def test_distance_to_stock_torch(name, hyper, state, gscale, max_norm):
    """uh_grad_sumsq + uh_rmsprop_step against clip_grad_norm_ + torch.optim.RMSprop in float64 with the Python doubles."""
    x, h = K.stock_inputs(name, state, gscale), K.HYPERS[hyper]
    norm = run_sumsq(x["g"])
    got = run_step(x, norm, max_norm, h)
    stock = K.stock_torch_step(x, max_norm, h)
    ref = K.step_reference(x, K.coef32(float(norm.item()), max_norm), h)
    d = K.stock_distance(got, x, stock, ref, h)
    print(f"{name}: to stock torch, relative to the bounds' magnitudes: " + ", ".join(f"{k} {v:.2e} ({v / K.U:.1f} u)" for k, v in d.items()))
    assert max(d.values()) <= K.OP_TOL
    K.check_step(got, x, ref, h, what=name)                         # and to the primary reference, with the kernel's own norm
    if state == "first":
        assert d["s"] > 8e-7                                        # the 1 - alpha rounding is there, whole


# ------------------------------------------------------------------------------------------------ swap
@pytest.mark.parametrize("n", K.SIZES + (K.ONE_SWEEP, K.WRAP))
def test_swap_is_an_exact_exchange(n):
    r = np.random.default_rng(n)
    a, b = r.standard_normal(n, dtype=F), r.standard_normal(n, dtype=F)
    a[0], b[-1] = F("nan"), F("-inf")                               # bits, not values
    da, db = _up(a), _up(b)
    _lib().call("uh_swap_f32", da.data_ptr(), db.data_ptr(), n, _stream())
    torch.cuda.synchronize()
    assert _same_bits(_down(da, n), b) and _same_bits(_down(db, n), a)


# ------------------------------------------------------------------------------------------------ the sum of squares
@pytest.mark.parametrize("n", K.SUMSQ_SIZES)
def test_sumsq_of_small_integers_is_exact(n):
    g = K.integer_gradient(n)
    got = run_sumsq(g).cpu().numpy()[0]
    assert got == K.exact_norm(g), (float(got), float(K.exact_norm(g)))


@pytest.mark.parametrize("n", K.SUMSQ_SIZES)
def test_sumsq_sees_every_position(n):
    LIB = _lib()
    gd = _up(np.zeros(n, F))
    out = torch.full((1,), -1.0, dtype=torch.float32, device=_dev())
    ws = torch.empty(LIB.query("uh_optim_ws_bytes", n), dtype=torch.uint8, device=_dev())
    for i in K.probe_indices(n):
        gd[i] = 3.0
        LIB.call("uh_grad_sumsq", gd.data_ptr(), n, out.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
        assert float(out.item()) == 3.0, (n, i)
        gd[i] = 0.0
    LIB.call("uh_grad_sumsq", gd.data_ptr(), n, out.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
    assert float(out.item()) == 0.0                                 # all zero, the sentinel behind n unread


@pytest.mark.parametrize("n,scale", K.SUMSQ_RANDOM)
def test_sumsq_of_random_gradients_against_float64(n, scale):
    g = K.random_gradient(n, scale)
    want = K.norm64(g)
    got = float(run_sumsq(g).item())
    print(f"n {n} scale {scale:g}: off by {abs(got - want) / (K.U * want):.2f} u of the norm (bound {K.norm_bound(want) / (K.U * want):.1f})")
    assert abs(got - want) <= K.norm_bound(want)


@pytest.mark.parametrize("value", [3e19, 1e19])
def test_overflowing_squares_give_an_infinite_norm_and_no_step(value):
    """3e19: every square is infinite; 1e19: the squares are finite, a thread's sum of four is not."""
    x = K.step_inputs(K.StepCase("overflow", 4099, "ema", "ordinary", None, 1.0))
    x["g"] = np.full(4099, value, F)
    norm = run_sumsq(x["g"])
    assert float(norm.item()) == float("inf")
    got = run_step(x, norm, 1.0, K.HYPERS["ema"])
    for k in "pgsb":
        assert _same_bits(got[k], x[k]), k


# ------------------------------------------------------------------------------------------------ FusedRMSprop
EMA_DECAY = 0.9


def _toy(ema, **kw):
    """Five parameters (optim_cases.TOY_SHAPES, the 4-D one channels_last) under a FusedRMSprop with the EMA tests' hyper-parameters."""
    import unet_amd
    g = torch.Generator().manual_seed(5)
    params = []
    for shape in K.TOY_SHAPES:
        t = torch.randn(shape, generator=g).to(_dev())
        if len(shape) == 4:
            t = t.contiguous(memory_format=torch.channels_last)
        params.append(torch.nn.Parameter(t))
    assert params[3].stride() == (27, 1, 9, 3)
    opt = unet_amd.FusedRMSprop(params, lr=1e-3, weight_decay=1e-2, momentum=0.9, ema_decay=EMA_DECAY if ema else None,
                                ema_warmup=0, **kw)
    assert [tuple(p.shape) for p in opt.params] == K.TOY_SHAPES[::-1] and opt.total == 276
    assert opt.slices == [(0, 4), (4, 216), (220, 1), (224, 13), (240, 35)]
    return opt


def _memory_order(t, p):
    """The elements of t (shaped like the parameter p, on any device) in the order p keeps them in memory."""
    flat = torch.empty(p.numel(), dtype=t.dtype, device=t.device)
    torch.as_strided(flat, p.shape, p.stride()).copy_(t)
    return flat


def _flat_buffers(opt):
    torch.cuda.synchronize()
    out = {"p": opt.flat_p, "g": opt.flat_g, "s": opt.flat_sq, "b": opt.flat_buf}
    if opt.flat_ema is not None:
        out["e"] = opt.flat_ema
    return {k: v.cpu().numpy().copy() for k, v in out.items()}


def _hyper(opt):
    g = opt.param_groups[0]
    return dict(lr=g["lr"], alpha=g["alpha"], eps=g["eps"], wd=g["weight_decay"], mu=g["momentum"])


def _gradients(opt, kind, seed):
    """One gradient per slice, on the CPU, shaped like the parameter."""
    r = torch.Generator().manual_seed(seed)
    if kind == "integers":                                          # +-{1, 2, 3}: a one-element slice never gets a zero gradient
        return [(torch.randint(1, 4, p.shape, generator=r) * (2 * torch.randint(0, 2, p.shape, generator=r) - 1)).float()
                for p in opt.params]
    return [torch.randn(p.shape, generator=r) * kind for p in opt.params]


def _step(opt, pattern, grads, worst):
    """One backward and step with the slices of `pattern` fresh; every check of the issue's list.  -> the norm."""
    fresh = [c == "F" for c in pattern]
    opt.zero_grad()
    sum((p * g.to(p.device)).sum() for p, g, f in zip(opt.params, grads, fresh) if f).backward()
    before = _flat_buffers(opt)
    mem = [_memory_order(g, p).numpy() for p, g in zip(opt.params, grads)]
    for (o, n), m, f in zip(opt.slices, mem, fresh):
        if f:
            assert _same_bits(before["g"][o:o + n], m)              # the gradient arrived, in the parameter's memory order
    h = _hyper(opt)
    norm = float(opt.step().item())
    after = _flat_buffers(opt)
    # the norm: over the fresh gradients only
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
        x = {k: before[k][o:o + n] for k in "psb"}
        x["g"] = m
        ref = K.step_reference(x, coef, h)
        got = {k: after[k][o:o + n] for k in "pgsb"}
        units = K.check_step(got, x, ref, h, what=f"{pattern} slice {i}")
        for k in "sbp":
            worst[k] = max(worst.get(k, 0.0), units[k])
        # read through the parameter itself: the same values, in its own memory order
        assert _same_bits(_memory_order(p.detach(), p).cpu().numpy(), got["p"]), (pattern, i)
        if "e" in before:
            c = float(F(1) - F(EMA_DECAY))
            e, pn = before["e"][o:o + n].astype(np.float64), got["p"].astype(np.float64)
            bound = 6 * K.U * np.maximum(np.abs(pn), np.abs(e))    # tests/test_gpu_ema.py derives it
            assert bool((np.abs(after["e"][o:o + n] - (e + c * (pn - e))) <= bound).all()), (pattern, i)
    for k in after:
        assert not after[k][pad].any(), f"padding lanes of flat {k} after {pattern}"
    assert int(pad.sum()) == 276 - 269
    return norm


@pytest.mark.parametrize("ema", [False, True], ids=["plain", "ema"])
def test_fused_rmsprop_steps_and_stale_patterns(ema):
    opt = _toy(ema)
    worst = {}
    kinds = [1.0, "integers", 0.01, 1.0, "integers", 0.01]            # clipped (norm ~ 16), exact, not clipped (~ 0.16)
    norms = []
    for k, (pattern, kind) in enumerate(zip(K.PATTERNS, kinds)):
        if k > 0:                                                   # behind the all-fresh first step: a stale slice holds a
            before = _flat_buffers(opt)                             # state and, if it was fresh last time, that scaled gradient
            for (o, n), c, last in zip(opt.slices, pattern, K.PATTERNS[k - 1]):
                assert c == "F" or all(before[b][o:o + n].any() for b in ("sb" if last == "S" else "gsb")), (pattern, o)
        norms.append(_step(opt, pattern, _gradients(opt, kind, 100 + k), worst))
    assert norms[0] > 1 > norms[2]
    # a changed lr is used by the next step, and the p bound can tell: with the old one it breaks
    opt.param_groups[0]["lr"] = 5e-4
    before = _flat_buffers(opt)
    grads = _gradients(opt, 1.0, 200)
    norm = _step(opt, "FFFFF", grads, worst)
    after = _flat_buffers(opt)
    o, n = opt.slices[1]
    x = {k: before[k][o:o + n] for k in "psb"}
    x["g"] = _memory_order(grads[1], opt.params[1]).numpy()
    old = dict(_hyper(opt), lr=1e-3)
    units = K.step_units({k: after[k][o:o + n] for k in "pgsb"}, x, K.step_reference(x, K.coef32(norm, 1.0), old), old)
    assert K.step_breaks(units) == ["p"], units
    print(f"FusedRMSprop ({'ema' if ema else 'plain'}): worst sq {worst['s']:.2f}, buf {worst['b']:.2f}, p {worst['p']:.2f} units")
    opt.close()


def test_fused_rmsprop_without_clipping_leaves_the_gradient():
    opt = _toy(False, gradient_clipping=None)
    assert opt.gradient_clipping == 0.0
    worst = {}
    for k, pattern in enumerate(("FFFFF", "FSFSF")):
        grads = _gradients(opt, 1.0, 300 + k)
        norm = _step(opt, pattern, grads, worst)
        assert norm > 1                                             # clipping would have scaled
        after = _flat_buffers(opt)["g"]
        for (o, n), p, g, c in zip(opt.slices, opt.params, grads, pattern):
            want = _memory_order(g, p).numpy() if c == "F" else np.zeros(n, F)
            assert _same_bits(after[o:o + n], want), (pattern, o)
    opt.close()
