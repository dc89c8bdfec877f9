"""The forward BatchNorm statistics chain on the GPU, held to float64 row by row: the rows the conv kernels write, uh_bn_finalize /
uh_bn_finalize_ld over them, uh_bn_eval_coeffs, and the chain conv -> rows -> ops._bn_train_coefficients against float64
torch.nn.BatchNorm2d.  Cases, references and bounds come from tests/bn_stats_cases.py; tests/test_bn_stats_cpu.py proves on the CPU
that the families meet their conditions at these shapes and that the planted errors are caught.

No assert here carries a tolerance that is not zero or derived in the text beside it (or in the docstring of the function of
bn_stats_cases.py it comes from), and every derived bound is printed with the error it was compared to.  Where a kernel rounds by
design the inputs are narrowed, never the comparison."""
import numpy as np
import pytest
import torch

import bn_stats_cases as BC

pytestmark = pytest.mark.gpu

F = np.float32
PAD = 8                                      # canary floats on both sides of every per-channel output array
OUT_KEYS = ("scale", "shift", "mean", "rstd", "m2_out", "running_mean", "running_var")


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    return torch.device("cuda:0")


def _bits(a):
    return np.asarray(a, F).view(np.uint32)


# ------------------------------------------------------------------------------------------------ A. the finalize, called directly
class Guarded:
    """A per-channel array of exactly C floats with PAD canaries on both sides; the kernel gets the address of the C floats."""

    def __init__(self, C, dev, init=None):
        host = np.full(C + 2 * PAD, BC.CANARY, F)
        host[PAD:PAD + C] = np.nan if init is None else init
        self.C, self.t = C, torch.from_numpy(host).to(dev)

    @property
    def ptr(self):
        return self.t.data_ptr() + 4 * PAD

    def result(self, what):
        host = self.t.cpu().numpy()
        assert (host[:PAD] == BC.CANARY).all() and (host[PAD + self.C:] == BC.CANARY).all(), f"{what}: written outside its {self.C} entries"
        return host[PAD:PAD + self.C].copy()


def run_finalize(case, inp, dev, calls=1):
    """uh_bn_finalize (ldc == C) or uh_bn_finalize_ld on the packed rows.  -> dict of float32 arrays (+ "nbt")."""
    from unet_amd import ops
    from unet_amd._lib import LIB
    C = case.C
    stats = torch.from_numpy(BC.pack_stats(inp, case.ldc)).to(dev)
    gamma, beta = torch.from_numpy(inp["gamma"]).to(dev), torch.from_numpy(inp["beta"]).to(dev)
    out = {k: Guarded(C, dev) for k in ("scale", "shift", "mean", "rstd")}
    opt = {"running_mean": Guarded(C, dev, inp["running_mean"]), "running_var": Guarded(C, dev, inp["running_var"]),
           "m2_out": Guarded(C, dev)}
    nbt = torch.tensor([BC.CANARY_NBT - 1, 41, BC.CANARY_NBT + 1], dtype=torch.int64, device=dev)
    ptr = {k: (None if case.null == k else v.ptr) for k, v in opt.items()}
    nbt_ptr = None if case.null == "num_batches_tracked" else nbt.data_ptr() + 8
    head = ("uh_bn_finalize", stats.data_ptr(), case.nslab) if case.ldc == C else ("uh_bn_finalize_ld", stats.data_ptr(), case.nslab, case.ldc)
    for _ in range(calls):
        LIB.call(*head, C, int(inp["n_pass"]), gamma.data_ptr(), beta.data_ptr(), ptr["running_mean"], ptr["running_var"], nbt_ptr,
                 float(inp["momentum"]), float(inp["eps"]), out["scale"].ptr, out["shift"].ptr, out["mean"].ptr, out["rstd"].ptr,
                 ptr["m2_out"], ops._stream())
    torch.cuda.synchronize()
    got = {k: v.result(k) for k, v in {**out, **opt}.items()}
    got["nbt"] = nbt.cpu().tolist()
    assert np.array_equal(stats.cpu().numpy().view(np.uint32), BC.pack_stats(inp, case.ldc).view(np.uint32)), "the rows were written to"
    return got


def _check_untouched(case, inp, got):
    """What a null pointer leaves alone, and num_batches_tracked: 41 -> 42 between its two canaries."""
    assert got["nbt"] == [BC.CANARY_NBT - 1, 41 if case.null == "num_batches_tracked" else 42, BC.CANARY_NBT + 1]
    for k in ("running_mean", "running_var"):
        if case.null == k:
            assert np.array_equal(_bits(got[k]), _bits(inp[k])), f"{k}: changed though its pointer was null"
    if case.null == "m2_out":
        assert np.isnan(got["m2_out"]).all()


@pytest.mark.parametrize("case", BC.FIN_CASES, ids=lambda c: c.name)
def test_finalize_dyadic_rows_bit_exact(case):
    """Every output of bn_finalize_kernel on the dyadic family, bit for bit (conditions: bn_stats_cases.assert_dyadic_conditions).
    running_var holds the one quotient that is no power-of-two division, m2 / (n - 1): it is compared with IEEE float64 division
    rounded to float32 (the device's double division is correctly rounded: measured on the first run of this test, no case
    differs), so this comparison has no allowance either."""
    dev = _dev()
    inp = BC.dyadic_rows(case)
    ex = BC.finalize_exact(inp)
    BC.assert_dyadic_conditions(inp, ex)
    want = BC.dyadic_expected(inp, ex)
    got = run_finalize(case, inp, dev)
    _check_untouched(case, inp, got)
    for k in OUT_KEYS:
        if case.null == k:
            continue
        bad = np.flatnonzero(_bits(got[k]) != _bits(want[k]))
        assert len(bad) == 0, f"{k}: channels {bad[:8].tolist()} got {got[k][bad[:8]].tolist()} want {want[k][bad[:8]].tolist()}"
    again = run_finalize(case, inp, dev)
    for k in OUT_KEYS:
        assert np.array_equal(_bits(got[k]), _bits(again[k])), f"{k}: two calls on the same inputs differ"


@pytest.mark.parametrize("case", BC.FIN_CASES, ids=lambda c: c.name)
def test_finalize_general_rows_within_derived_bounds(case):
    """Random fp32 rows (one channel in four with mean 1e4 and standard deviation 0.1), momentum 0.1, eps 1e-5: per channel every
    output within the bound bn_stats_cases.general_bounds derives from the kernel's operations -- a few float32 roundings, the
    double term shown negligible there; shift and the running updates bounded for both contractions."""
    dev = _dev()
    inp = BC.general_rows(case)
    ex = BC.finalize_exact(inp)
    val, tol = BC.general_bounds(inp, ex, case.nslab)
    got = run_finalize(case, inp, dev)
    _check_untouched(case, inp, got)
    lines, failed = [], []
    for k in OUT_KEYS:
        if case.null == k:
            continue
        err = np.abs(got[k].astype(np.float64) - val[k])
        ratio = np.where(tol[k] > 0, err / np.where(tol[k] > 0, tol[k], 1), np.where(err > 0, np.inf, 0))
        c = int(np.argmax(ratio))
        lines.append(f"{k}: error {err[c]:.3e} (bound {tol[k][c]:.3e}) at channel {c}")
        if not bool((err <= tol[k]).all()):
            failed.append(k)
    print(f"finalize {case.name}: " + "; ".join(lines))
    assert failed == [], failed
    again = run_finalize(case, inp, dev)
    for k in OUT_KEYS:
        assert np.array_equal(_bits(got[k]), _bits(again[k])), f"{k}: two calls on the same inputs differ"


@pytest.mark.parametrize("name", BC.NBT_CASES)
def test_num_batches_tracked_rises_by_one_per_call(name):
    """One block (C = 1) and many (C = 130: 33 blocks, of which only block 0 may count), with and without the walk."""
    dev = _dev()
    case = BC.FIN_BY_NAME[name]
    inp = BC.dyadic_rows(case)
    for calls in (1, 2, 5):
        got = run_finalize(case, inp, dev, calls)
        assert got["nbt"] == [BC.CANARY_NBT - 1, 41 + calls, BC.CANARY_NBT + 1]


# ------------------------------------------------------------------------------------------------ A. the eval coefficients
@pytest.mark.parametrize("family", ["dyadic", "general"])
@pytest.mark.parametrize("C", BC.EVAL_C)
def test_eval_coeffs(C, family):
    """uh_bn_eval_coeffs: bit for bit on the dyadic family (tolerance zero), within the bound of bn_stats_cases.eval_expected
    against float64 gamma / sqrt(rv + eps) on random running statistics; C around the block of 256, canaries past C."""
    from unet_amd import ops
    from unet_amd._lib import LIB
    dev = _dev()
    inp = BC.eval_inputs(C, family)
    scale, shift, ts, tsh = BC.eval_expected(inp, family)
    t = {k: torch.from_numpy(inp[k]).to(dev) for k in ("gamma", "beta", "running_mean", "running_var")}
    sc, sh = Guarded(C, dev), Guarded(C, dev)
    LIB.call("uh_bn_eval_coeffs", t["gamma"].data_ptr(), t["beta"].data_ptr(), t["running_mean"].data_ptr(), t["running_var"].data_ptr(),
             float(inp["eps"]), C, sc.ptr, sh.ptr, ops._stream())
    torch.cuda.synchronize()
    gs, gh = sc.result("scale").astype(np.float64), sh.result("shift").astype(np.float64)
    es, eh = np.abs(gs - scale), np.abs(gh - shift)
    i, j = int(np.argmax(es - ts)), int(np.argmax(eh - tsh))
    print(f"eval coefficients C={C} {family}: scale error {es[i]:.3e} (bound {ts[i]:.3e}), shift error {eh[j]:.3e} (bound {tsh[j]:.3e})")
    assert bool((es <= ts).all()) and bool((eh <= tsh).all())


# ------------------------------------------------------------------------------------------------ B. the rows every forward form writes
def _nhwc(t, bf16, dev):
    """NCHW float32 (CPU) -> dense NHWC on the device; the families' values are exact in either dtype."""
    import exact_inputs as E
    g = E.nhwc(t).to(dev, torch.bfloat16 if bf16 else torch.float32)
    assert torch.equal(g.float().cpu(), E.nhwc(t))
    return g


def split_rows(stats, nslab, C):
    """The buffer a forward call filled -> (rows [nslab, 2, C] float64, counts [nslab] float64), on the host."""
    s = stats.cpu().numpy()
    return s[:nslab * 2 * C].reshape(nslab, 2, C).astype(np.float64), s[nslab * 2 * C:nslab * 2 * C + nslab].astype(np.float64)


def check_rows(label, stats, nslab, y, y_ext, shape, plan, tol, family):
    """Counts exactly; merged moments per channel within the derived bound; flat family: the rows bit for bit.
    -> (mean error, M2 error) as multiples of their bounds, worst channel."""
    B, H, W, _, _, C = shape
    lanes = plan["lanes"]
    assert nslab == plan["ntile"]
    rows, counts = split_rows(stats, nslab, C)
    n_r, _, _ = BC.row_counts((B, H, W), lanes)
    assert np.array_equal(counts[:lanes], n_r), f"{label}: per-row pixel counts"
    assert not counts[lanes:].any(), f"{label}: rows behind the live ones must have a zero count"
    assert int((counts > 0).sum()) == lanes and counts.sum() == B * H * W
    mean, m2 = BC.merge_rows(n_r, rows[:lanes, 0], rows[:lanes, 1])
    want_mean, want_m2 = BC.whole_moments(y)
    tol_mean, tol_m2, _ = tol
    em, e2 = np.abs(mean - want_mean), np.abs(m2 - want_m2)
    i, j = int(np.argmax(em - tol_mean)), int(np.argmax(e2 - tol_m2))
    print(f"rows {BC.rows_id(shape)} {family} {label} [{plan['producer']}, {lanes} rows]: mean error {em[i]:.3e} (bound {tol_mean[i]:.3e}), "
          f"M2 error {e2[j]:.3e} (bound {tol_m2[j]:.3e}), M2 / n = {want_m2[j] / (B * H * W):.3e}")
    assert bool((em <= tol_mean).all()), f"{label}: mean of channels {np.flatnonzero(em > tol_mean)[:8].tolist()}"
    assert bool((e2 <= tol_m2).all()), f"{label}: M2 of channels {np.flatnonzero(e2 > tol_m2)[:8].tolist()}"
    if family == "flat":
        want_rm, want_r2 = BC.flat_rows_exact(y, (B, H, W), plan, y_ext)                # (asserts the conditions)
        got_rm, got_r2 = rows[:lanes, 0].astype(F), rows[:lanes, 1].astype(F)
        assert np.array_equal(_bits(got_rm), _bits(want_rm)), f"{label}: row means {np.argwhere(got_rm != want_rm)[:4].tolist()}"
        assert np.array_equal(_bits(got_r2), _bits(want_r2)), f"{label}: row M2 {np.argwhere(got_r2 != want_r2)[:4].tolist()}"


def forward_launches(c, shape, bf16, code, dev):
    """The forward launches of test_gpu_exact.py::test_conv3x3_fwd_and_dgrad_bit_exact, statistics kept: row-major pack, the two
    sources as slices of one buffer, the fragment-major pack where the LDS-DMA kernel takes the call.  Yields (label, y, stats, nslab)."""
    from unet_amd import ops
    B, H, W, C0, C1, Cout = shape
    dtype, dt = (torch.bfloat16, 1) if bf16 else (torch.float32, 0)
    x0 = _nhwc(c.x[:, :C0], bf16, dev)
    x1 = _nhwc(c.x[:, C0:], bf16, dev) if C1 else None
    ok_f = ops.wfrag_ok(B, H, W, C0, C1, Cout, C0, C1, Cout, dt)
    assert ok_f == (code >= 1)
    wg = c.w.to(dev)
    wf, _ = ops.pack_w3x3(wg, dtype, False)
    yield ("row-major pack",) + tuple(ops.conv3x3_fwd(x0, x1, wf, Cout, True))
    if C1:
        xg = _nhwc(c.x, bf16, dev)
        yield ("sources with a pixel pitch of C0 + C1",) + tuple(ops.conv3x3_fwd(xg[..., :C0], xg[..., C0:], wf, Cout, True))
    if ok_f:
        wf2, _ = ops.pack_w3x3(wg, dtype, False, None, True, False)
        yield ("fragment-major pack",) + tuple(ops.conv3x3_fwd(x0, x1, wf2, Cout, True, None, True))


@pytest.mark.parametrize("shape,family,bf16,code", BC.rows_params(), ids=BC.rows_id)
def test_conv_statistics_rows(shape, family, bf16, code):
    """The statistics rows of every forward form (the launches of test_gpu_exact.py, the stem kernels off the 16-byte grid and in
    bf16 added), per row and per channel.

    Exact: the count of every live row is the pixel count of the tiles it covers (tile t on row t mod lanes), the rows behind have
    a zero count, the counts sum to B H W and the live rows are as many as the plan says (bn_stats_cases.rows_plan).

    Moments: y is an exact integer tensor; the rows are merged in float64 on the host and the merged mean and M2 of EVERY channel
    lie within the bound bn_stats_cases.row_bounds derives from the producer's arithmetic -- for the pivot-shifted form d = y - p
    (p is known: one pixel of the row's first tile), S1 = sum d and S2 = sum d^2 in fp32 lanes with R roundings on the way of a
    term (none while the integer partial sums stay below 2^24, which is tested on the reference per row and channel), mean =
    p + S1 (1 / n), M2 = max(S2 - S1^2 (1 / n), 0); for the per-tile kernels the two-pass form.  The derivation is that function's
    docstring; tests/test_bn_stats_cpu.py shows for each case that a float32 restatement of the producer meets the bound and that
    a dropped or doubled border pixel, a row from the neighbouring channel or the other PERM2 half, the unrounded accumulator and
    plain sums without a pivot do not.

    The flat family (full tiles, one per row, |y - mean| <= 6): every row has one right answer (bn_stats_cases.flat_rows_exact) and
    is compared bit for bit."""
    import exact_inputs as E
    from unet_amd._lib import LIB
    dev = _dev()
    B, H, W, C0, C1, Cout = shape
    assert LIB.query("uh_conv3x3_fwd_kernel", B, H, W, C0, C1, Cout, 1 if bf16 else 0) == code
    c = BC.family_case(shape, family)
    plan = BC.rows_plan(shape, bf16, code)
    y, y_ext = BC.stored(c.y, bf16), BC.stored(c.y_ext, bf16)
    tol = BC.row_bounds(y, y_ext, (B, H, W), plan, BC.v2_lanes(Cout, bf16))
    want_y = E.expected(E.nhwc(c.y), torch.bfloat16 if bf16 else torch.float32)
    for label, yg, stats, nslab in forward_launches(c, shape, bf16, code, dev):
        torch.cuda.synchronize()
        E.assert_same(yg, want_y, f"forward, {label}")
        check_rows(f"{'bf16' if bf16 else 'fp32'}, {label}", stats, nslab, y, y_ext, shape, plan, tol, family)


# ------------------------------------------------------------------------------------------------ C. the chain
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_chain_rows_to_coefficients_against_batchnorm(bf16):
    """conv -> its own rows -> ops._bn_train_coefficients, against float64 torch.nn.BatchNorm2d in training mode on the exact stored
    y.  fp32: conv3x3_fwd_stem_v2, 1089 per-tile rows, so the finalize walks behind its first 1024 on real rows; bf16:
    conv3x3_fwd_stem_v3, 1024 rows of which 65 cover two tiles, and the walk is skipped.

    Bound: part B's bound on the merged mean and M2 (row_bounds: the exact merge of the rows the conv wrote is that close to the
    moments of y), plus the double-precision term of the finalize's own merge (general_bounds, from S, Q, SA of these rows about the
    first row's mean), carried through the formulas of part A (coefficient_bounds): dvar = dM2 / n, drstd = rstd^3 dvar / 2,
    dscale = |gamma| drstd + u |scale|, shift and the running updates as derived there for either contraction."""
    import exact_inputs as E
    from unet_amd import ops
    from unet_amd._lib import LIB
    dev = _dev()
    shape = BC.CHAIN_SHAPE
    B, H, W, C0, C1, C = shape
    n = B * H * W
    assert LIB.query("uh_conv3x3_fwd_kernel", B, H, W, C0, C1, C, 1 if bf16 else 0) == 0
    c = BC.family_case(shape, "ternary")
    plan = BC.rows_plan(shape, bf16, 0)
    assert plan["lanes"] == (1024 if bf16 else 1089) and plan["ntile"] == 1089 > BC.BNF_FAST
    y, y_ext = BC.stored(c.y, bf16), BC.stored(c.y_ext, bf16)
    tol = BC.row_bounds(y, y_ext, (B, H, W), plan, BC.v2_lanes(C, bf16))
    label, yg, stats, nslab = next(forward_launches(c, shape, bf16, 0, dev))
    torch.cuda.synchronize()
    E.assert_same(yg, E.expected(E.nhwc(c.y), torch.bfloat16 if bf16 else torch.float32), "forward")
    check_rows(f"{'bf16' if bf16 else 'fp32'}, {label}", stats, nslab, y, y_ext, shape, plan, tol, "ternary")
    rng = np.random.default_rng(513)
    host = dict(gamma=(rng.random(C) + 0.5).astype(F), beta=(rng.standard_normal(C) * 0.2).astype(F),
                running_mean=(rng.standard_normal(C) * 0.1).astype(F), running_var=(rng.random(C) + 0.5).astype(F))
    t = {k: torch.from_numpy(v.copy()).to(dev) for k, v in host.items()}
    nbt = torch.tensor(7, dtype=torch.int64, device=dev)
    o = ops.ConvBnOpts(running_mean=t["running_mean"], running_var=t["running_var"], num_batches_tracked=nbt)
    coef, n_total = ops._bn_train_coefficients(stats, nslab, C, n, t["gamma"], t["beta"], o)
    torch.cuda.synchronize()
    assert n_total == n and int(nbt) == 8
    got = dict(zip(("scale", "shift", "mean", "rstd"), (v.cpu().numpy().astype(np.float64) for v in ops.coef_views(coef))))
    got["running_mean"], got["running_var"] = t["running_mean"].cpu().numpy().astype(np.float64), t["running_var"].cpu().numpy().astype(np.float64)
    # the reference: torch's own module in float64
    eps, mom = float(F(o.eps)), float(F(o.momentum))                                   # the values the kernel receives (the C ABI takes float)
    bn = torch.nn.BatchNorm2d(C, eps=eps, momentum=mom).double()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(host["gamma"]))
        bn.bias.copy_(torch.from_numpy(host["beta"]))
        bn.running_mean.copy_(torch.from_numpy(host["running_mean"]))
        bn.running_var.copy_(torch.from_numpy(host["running_var"]))
    bn.train()
    yt = torch.from_numpy(y).permute(0, 3, 1, 2).contiguous()
    with torch.no_grad():
        z = bn(yt)
    var, mean = torch.var_mean(yt, dim=(0, 2, 3), unbiased=False)
    rstd = 1.0 / torch.sqrt(var + eps)
    want = dict(mean=mean, rstd=rstd, scale=bn.weight * rstd, shift=bn.bias - mean * bn.weight * rstd, running_mean=bn.running_mean,
                running_var=bn.running_var)
    want = {k: v.detach().numpy() for k, v in want.items()}
    # Two float64 evaluations of the same sums over n terms differ by at most n 2^-53 relative, whatever their order: that much is
    # allowed between the module's output and y scale + shift with these coefficients, and between coefficient_bounds' values and torch's
    ref_tol = n * BC.EPS64
    lin = yt * torch.from_numpy(want["scale"]).view(1, C, 1, 1) + torch.from_numpy(want["shift"]).view(1, C, 1, 1)
    assert float((z - lin).abs().max()) <= ref_tol * (1 + float(z.abs().max()))
    assert int(bn.num_batches_tracked) == 1
    # the double term of the finalize's merge, from the rows it was given
    rows, counts = split_rows(stats, nslab, C)
    live = counts > 0
    nr, mr, m2r = counts[live][:, None], rows[live, 0], rows[live, 1]
    d = mr - rows[0, 0]
    L = 16 * ((nslab + BC.BNF_FAST - 1) // BC.BNF_FAST) + 8
    dbl_mean = (L + 2) * BC.EPS64 * ((nr * np.abs(d)).sum(0) / n + np.abs(want["mean"]))
    dbl_m2 = (3 * L + 6) * BC.EPS64 * (m2r.sum(0) + (nr * d * d).sum(0))
    M2 = want_m2 = BC.whole_moments(y)[1]
    worst = {}
    for ch in range(C):
        val, bound = BC.coefficient_bounds(float(want["mean"][ch]), float(M2[ch]), n, tol[0][ch] + dbl_mean[ch], tol[1][ch] + dbl_m2[ch],
                                           float(host["gamma"][ch]), float(host["beta"][ch]), float(host["running_mean"][ch]),
                                           float(host["running_var"][ch]), mom, eps)
        for k in got:
            assert abs(val[k] - want[k][ch]) <= ref_tol * (1 + abs(val[k])), (k, ch)    # coefficient_bounds' values are torch's
            err = abs(got[k][ch] - want[k][ch])
            if k not in worst or err / bound[k] > worst[k][0] / worst[k][1]:
                worst[k] = (err, bound[k], ch)
    print(f"chain {'bf16' if bf16 else 'fp32'}: " + "; ".join(f"{k}: error {e:.3e} (bound {b:.3e}) at channel {ch}" for k, (e, b, ch) in worst.items()))
    bad = [k for k, (e, b, _) in worst.items() if e > b]
    assert bad == [], bad
