"""Bit-exact GPU tests of the spatial-attention kernels (csrc/spatial_attn.hip) through the C ABI: uh_spatial_attn_fwd and
uh_spatial_attn_bwd in every launch form, across tile seams and image borders, past the filter gradient's 1024 workgroups, on
channel slices of wider buffers, and on the argmax rule's special values.

The cases are SaFwdCase and SaBwdCase of tests/exact_inputs.py: wide integers in x, a dyadic w with every tap distinct, and -- for the
backward, which takes the forward's results as inputs -- a synthetic map from {1/8 .. 7/8}, an integer pool and any argmax channel.
On them the channel maximum, its first channel, the mean (one float32 division of an exact sum), y (one product, one rounding),
g_s, g_pool, dw and dx each have ONE right value, from float64 stock torch; they are compared with E.assert_same / torch.equal.
tests/test_exact_inputs_cpu.py shows on the CPU that the conditions hold at every shape used here and that a dropped halo column,
the other image's rows in a halo, the last maximum, a maximum started at 0, a correlation for the transposed one, a missing
division by C, a for a (1 - a), a dropped tile past the 1024th, a dropped channel of a second step and a doubly rounded y each
change a compared value.

The map a is the one value with a tolerance: it holds an expf and a division.  Where C is a power of two the kernel's accumulator
is exact (asserted on the case), so a differs from sigmoid in float64 by uh_sigmoid alone: expf within one ulp (2 * 2^-24 of e,
(1 - a) of that on a), 1 + e and the division half an ulp each: 4 * 2^-24 at the most.  For other C the float64 map is formed from
the pool the kernel itself returned (compared bit for bit first), and the case scales w until the accumulator's roundings are
worth at most another 4 * 2^-24 (SaFwdCase).  The relative error is asserted against A_BOUND = twice the largest value measured
over every case of this file on an MI355X, and never above 8 * 2^-24, the budget tests/loss_cases.py gives a transcendental and
its roundings.  Measured over the 54 forward calls of this file: 2.000 * 2^-24 at the most (bf16, C = 520, k = 3: one float32
ulp of a map value just below 1/2; 1.0 to 1.9 on the power-of-two cases, whose maps run from 0.001 to 0.998), so A_BOUND = 4 * 2^-24.

Every case asks uh_spatial_attn_plan for the launch form its calls take and requires the one it was chosen for."""
import ctypes

import pytest
import torch

import exact_inputs as E
from test_gpu_exact_pixel import BF16, CANARY, DENSE, F32, Layout, Slot, _dev, _dt, _name, _st, _vec

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
A_MEASURED = 2.0 * U                             # largest relative error of the map over all cases, measured on an MI355X
A_BOUND = min(2 * A_MEASURED, 8 * U)
TAIL = 64                                        # canary elements behind every fp32 / int32 buffer a call writes
INT_CANARY = -77
SHAPE = (2, 9, 33)                               # two tile rows and two tile columns, one row and one column wide
KS = (3, 7)

# dtype, C, form, what uh_spatial_attn_plan must answer (V, G, steps)
FORMS = [
    (F32, 1, "scalar, one lane", (1, 1, 1)), (F32, 3, "scalar, grouped", (1, 4, 1)), (F32, 6, "scalar, grouped", (1, 8, 1)),
    (F32, 70, "scalar, two steps", (1, 64, 2)), (F32, 4, "vector, one lane", (4, 1, 1)), (F32, 24, "vector, grouped", (4, 8, 1)),
    (F32, 260, "vector, two steps", (4, 64, 2)),
    (BF16, 1, "scalar, one lane", (1, 1, 1)), (BF16, 12, "scalar, grouped", (1, 16, 1)), (BF16, 70, "scalar, two steps", (1, 64, 2)),
    (BF16, 8, "vector, one lane", (8, 1, 1)), (BF16, 24, "vector, grouped", (8, 4, 1)), (BF16, 520, "vector, two steps", (8, 64, 2)),
]
FORM_NAMES = {"scalar, one lane", "scalar, grouped", "scalar, two steps", "vector, one lane", "vector, grouped", "vector, two steps"}
GEOMETRY = [(1, 1), (2, 3), (7, 31), (8, 32), (9, 33), (17, 65)]
GEOMETRY_C = 8
BIG = (3, 9, 5473, 1)                            # 3 * 2 * 172 = 1032 tiles of 8 x 32 on 1024 workgroups, 147 771 pixels
PITCH_C = 24


def plan(C, dtype, aligned=True):
    """(V, G, steps) of uh_spatial_attn_plan.  Host only."""
    import unet_amd  # noqa: F401
    from unet_amd._lib import LIB
    out = (ctypes.c_int64 * 3)()
    assert LIB.query("uh_spatial_attn_plan", C, _dt(dtype), 1 if aligned else 0, ctypes.addressof(out)) == 0
    return tuple(out)


def form_of(C, dtype, aligned=True):
    V, G, steps = plan(C, dtype, aligned)
    assert V in (1, _vec(dtype)) and G in (1, 2, 4, 8, 16, 32, 64) and G * steps * V >= C > G * (steps - 1) * V
    return ("scalar" if V == 1 else "vector") + (", two steps" if steps == 2 else ", grouped" if G > 1 else ", one lane" if steps == 1 else ", many steps")


def check_forms():
    """Every form of FORMS is what the query answers, and the list reaches all six in both dtypes (where the dtype has it)."""
    seen = set()
    for dtype, C, form, want in FORMS:
        assert plan(C, dtype) == want and form_of(C, dtype) == form, (dtype, C, plan(C, dtype))
        V, G, steps = want
        if form == "vector, grouped":
            assert G * V > C                                         # idle lanes
        if form == "scalar, two steps":
            assert 0 < C - G * V < G * V                             # the second step is ragged: some lanes live, some not
        if form == "vector, two steps":
            assert C - G * V == V                                    # ... one live lane
        seen.add((dtype, form))
    assert seen == {(dt, f) for dt in (F32, BF16) for f in FORM_NAMES}
    return seen


class Tail:
    """A flat buffer a call writes n elements of, with TAIL canaries behind them."""

    def __init__(self, n, dev, dtype=F32):
        self.n, self.canary = n, INT_CANARY if dtype == torch.int32 else CANARY
        self.buf = torch.full((n + TAIL,), self.canary, dtype=dtype, device=dev)
        self.ptr = self.buf.data_ptr()

    def head(self, written=None):
        """The first n elements on the CPU; everything behind `written` (default n) must still hold the canary."""
        written = self.n if written is None else written
        assert bool((self.buf[written:] == self.canary).all()), "a call wrote past the end of a buffer"
        return self.buf[:self.n].cpu()


def _in(t_nchw, dtype, dev, lay):
    src = E.nhwc(t_nchw)
    return Slot(tuple(src.shape), dtype, dev, lay, src)


# ------------------------------------------------------------------------------------------------ the calls
def run_fwd(c, dtype, dev, xl=DENSE, yl=DENSE):
    from unet_amd._lib import LIB
    B, H, W, C = c.shape
    n = c.npix
    x, y = _in(c.x, dtype, dev, xl), Slot((B, H, W, C), dtype, dev, yl)
    w = c.w.float().to(dev).contiguous()
    pool, amax, a = Tail(2 * n, dev), Tail(n, dev, torch.int32), Tail(n, dev)
    LIB.call("uh_spatial_attn_fwd", x.ptr, x.ld, w.data_ptr(), c.k, pool.ptr, amax.ptr, a.ptr, y.ptr, y.ld, B, H, W, C, _dt(dtype), _st())
    torch.cuda.synchronize()
    assert torch.equal(x.result().float(), E.nhwc(c.x))              # the input and the rest of its buffer are as they were
    return dict(pool=pool.head().view(B, H, W, 2), amax=amax.head().view(B, H, W), a=a.head().view(B, H, W), y=y.result())


def check_fwd(c, got, dtype, what):
    """-> the largest relative error of the map."""
    E.assert_same(got["pool"][..., 1], c.max.float(), f"{what}: channel maximum")
    E.assert_same(got["amax"], c.amax.int(), f"{what}: first maximal channel")
    E.assert_same(got["pool"][..., 0], c.mean32, f"{what}: channel mean (exact sum / float(C), once)")
    ref = c.a64 if c.exact_acc else c.a_from_pool(got["pool"])
    err = float(((got["a"].double() - ref).abs() / ref).max())
    print(f"map error {what}: {err / U:.3f} * 2^-24 (bound {A_BOUND / U:.3f}, accumulator {c.acc_units:.2f})")
    assert err <= A_BOUND, f"{what}: the map is off by {err / U:.3f} * 2^-24 relatively"
    E.assert_same(got["y"], E.sa_gate(E.nhwc(c.x), got["a"], dtype), f"{what}: y = x a, rounded once")
    return err


def run_bwd(c, dtype, dev, xl=DENSE, dyl=DENSE, dxl=DENSE, extra_rows=0):
    from unet_amd._lib import LIB
    B, H, W, C = c.shape
    n, k = c.npix, c.k
    gate = c.mode == "gate"
    x = _in(c.x, dtype, dev, xl) if gate else None
    dy = _in(c.dy, dtype, dev, dyl) if gate else None
    ga = None if gate else c.ga.float().to(dev).contiguous()
    w = c.w.float().to(dev).contiguous()
    pool, amax, a = E.nhwc(c.pool).float().to(dev).contiguous(), c.amax.int().to(dev).contiguous(), c.a.float().to(dev).contiguous()
    dx = Slot((B, H, W, C), dtype, dev, dxl)
    need = LIB.query("uh_spatial_attn_dw_nblk", B, H, W)
    assert need == min(E.sa_tiles(B, H, W), E.SA_DW_BLOCKS)
    rows = need + extra_rows
    ws, dw, part = Tail(3 * n, dev), Tail(2 * k * k, dev), Tail(rows * 2 * k * k, dev)
    LIB.call("uh_spatial_attn_bwd", dy.ptr if gate else None, dy.ld if gate else 0, None if gate else ga.data_ptr(),
             x.ptr if gate else None, x.ld if gate else 0, w.data_ptr(), k, pool.data_ptr(), amax.data_ptr(), a.data_ptr(), ws.ptr,
             dx.ptr, dx.ld, dw.ptr, part.ptr, rows, B, H, W, C, _dt(dtype), _st())
    torch.cuda.synchronize()
    if gate:
        assert torch.equal(x.result().float(), E.nhwc(c.x)) and torch.equal(dy.result().float(), E.nhwc(c.dy))
    assert torch.equal(pool.cpu(), E.nhwc(c.pool).float()) and torch.equal(amax.cpu(), c.amax.int()) and torch.equal(a.cpu(), c.a.float())
    rows_written = part.head(need * 2 * k * k)[:need * 2 * k * k].view(need, 2 * k * k)
    return dict(ws=ws.head(), dw=dw.head().view(1, 2, k, k), dx=dx.result(), part_sum=rows_written.double().sum(0).view(1, 2, k, k))


def check_bwd(c, got, dtype, what):
    n = c.npix
    E.assert_same(got["ws"][2 * n:], c.gs.reshape(-1).float(), f"{what}: g_s as the kernel left it")
    E.assert_same(got["ws"][:2 * n], c.ws()[:2 * n], f"{what}: g_pool as the kernel left it")
    E.assert_same(got["part_sum"], c.dw, f"{what}: partial rows summed in float64")
    E.assert_same(got["dw"], c.dw.float(), f"{what}: dw")
    want = E.nhwc(c.dx)
    E.assert_same(got["dx"], want.bfloat16() if dtype == BF16 else want, f"{what}: dx")


# ------------------------------------------------------------------------------------------------ every launch form
FORM_PARAMS = [pytest.param(dt, C, k, id=f"{_name(dt)}-C{C}-k{k}") for dt, C, _, _ in FORMS for k in KS]


def test_the_cases_reach_every_launch_form():
    check_forms()


@pytest.mark.parametrize("dtype,C,k", FORM_PARAMS)
def test_forward_in_every_form(dtype, C, k):
    dev = _dev()
    assert (dtype, C, form_of(C, dtype)) in {f[:3] for f in FORMS}
    c = E.sa_fwd_case(*SHAPE, C, k)
    check_fwd(c, run_fwd(c, dtype, dev), dtype, f"{_name(dtype)} C={C} k={k}")


@pytest.mark.parametrize("mode", ["gate", "map"])
@pytest.mark.parametrize("dtype,C,k", FORM_PARAMS)
def test_backward_in_every_form(dtype, C, k, mode):
    dev = _dev()
    assert (dtype, C, form_of(C, dtype)) in {f[:3] for f in FORMS}
    c = E.sa_bwd_case(*SHAPE, C, k, mode)
    check_bwd(c, run_bwd(c, dtype, dev), dtype, f"{_name(dtype)} C={C} k={k} {mode}")


# ------------------------------------------------------------------------------------------------ tile seams and image borders
@pytest.mark.parametrize("dtype", [F32, BF16], ids=_name)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("hw", GEOMETRY, ids=lambda v: "x".join(map(str, v)))
def test_geometry(hw, k, dtype):
    """One pixel; an image smaller than the halo; one tile short of, equal to and one past a tile in both directions; 3 x 3 tiles,
    the middle one with a neighbour on every side.  B = 2: the second image's rows lie where a halo that forgets the image border
    would read (tests/test_exact_inputs_cpu.py shows that such a halo changes a compared value at each of these extents)."""
    dev = _dev()
    C = GEOMETRY_C
    assert plan(C, dtype) == ((8, 1, 1) if dtype == BF16 else (4, 2, 1))
    c = E.sa_fwd_case(2, *hw, C, k)
    assert c.exact_acc
    what = f"{_name(dtype)} {hw[0]}x{hw[1]} k={k}"
    check_fwd(c, run_fwd(c, dtype, dev), dtype, what)
    for mode in ("gate", "map"):
        cb = E.sa_bwd_case(2, *hw, C, k, mode)
        check_bwd(cb, run_bwd(cb, dtype, dev), dtype, f"{what} {mode}")


# ------------------------------------------------------------------------------------------------ the filter gradient's second round
def big_case(k):
    return E.sa_bwd_case(*BIG, k, "map", 1.0 / 16, True, E.SA_DW_BLOCKS)


@pytest.mark.parametrize("k", KS)
def test_filter_gradient_past_1024_tiles(k):
    """1032 tiles on 1024 workgroups: workgroups 0 .. 7 take a second tile.  Map mode, a = 1/2, a sparse ternary ga with a non-zero
    planted in every tile past the 1024th (asserted on the reference); dw, like everything else, bit for bit -- also with more rows of
    dw_partials than the call needs, which it must neither write nor read."""
    from unet_amd._lib import LIB
    dev = _dev()
    B, H, W, C = BIG
    tiles = E.sa_tiles(B, H, W)
    assert LIB.query("uh_spatial_attn_dw_nblk", B, H, W) == E.SA_DW_BLOCKS == 1024 < tiles == 1032
    assert form_of(C, F32) == "scalar, one lane"
    c = big_case(k)
    tile = E.sa_tile_of(B, H, W)
    for t in range(E.SA_DW_BLOCKS, tiles):
        assert bool((c.gs[tile == t] != 0).any()), f"tile {t} holds no gradient"
    for extra in (0, 5):
        check_bwd(c, run_bwd(c, F32, dev, extra_rows=extra), F32, f"fp32 1032 tiles k={k}, {extra} spare rows")


# ------------------------------------------------------------------------------------------------ pitched calls equal dense calls
def pitch_layouts(dtype):
    """An aligned slice, and one off the 16-byte grid (12 bytes resp. 24 bytes into a pixel whose pitch is no 16-byte multiple)."""
    return [Layout(2 * PITCH_C, PITCH_C), Layout(30, 3) if dtype == F32 else Layout(36, 12)]


def _same(a, b, what):
    assert sorted(a) == sorted(b)
    for key in sorted(a):
        assert a[key].dtype == b[key].dtype and torch.equal(a[key], b[key]), f"{what}: {key} differs from the dense call: {E.mismatches(a[key], b[key])}"


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("dtype", [F32, BF16], ids=_name)
def test_pitched_calls_equal_dense_calls(dtype, k):
    """x, y, dy, dx each in turn, then all together, as a channel slice of a wider buffer: value for value the dense call's results
    (the map included: it is the same kernel on the same pool), the rest of the buffer untouched (Slot.result), nothing written past
    pool, amax, a, ws, dw or dw_partials (Tail.head).  Off the 16-byte grid the query must answer the scalar form."""
    dev = _dev()
    C = PITCH_C
    cf, cg, cm = E.sa_fwd_case(*SHAPE, C, k), E.sa_bwd_case(*SHAPE, C, k, "gate"), E.sa_bwd_case(*SHAPE, C, k, "map")
    dense_f, dense_g, dense_m = run_fwd(cf, dtype, dev), run_bwd(cg, dtype, dev), run_bwd(cm, dtype, dev)
    check_fwd(cf, dense_f, dtype, f"{_name(dtype)} C={C} k={k} dense")
    check_bwd(cg, dense_g, dtype, "dense gate")
    check_bwd(cm, dense_m, dtype, "dense map")
    assert plan(C, dtype)[0] == _vec(dtype)
    lays = pitch_layouts(dtype)
    assert [lay.aligned(C, dtype) for lay in lays] == [True, False]
    for lay in lays:
        V = plan(C, dtype, lay.aligned(C, dtype))[0]
        assert V == (_vec(dtype) if lay.aligned(C, dtype) else 1)
        for placed in ({"x"}, {"y"}, {"dy"}, {"dx"}, {"x", "y", "dy", "dx"}):
            at = {t: lay if t in placed else DENSE for t in ("x", "y", "dy", "dx")}
            tag = f"{'+'.join(sorted(placed))} at {lay}"
            if placed & {"x", "y"}:
                _same(run_fwd(cf, dtype, dev, at["x"], at["y"]), dense_f, f"forward, {tag}")
            if placed & {"x", "dy", "dx"}:
                _same(run_bwd(cg, dtype, dev, at["x"], at["dy"], at["dx"]), dense_g, f"gate backward, {tag}")
            if "dx" in placed:
                _same(run_bwd(cm, dtype, dev, dxl=at["dx"]), dense_m, f"map backward, {tag}")


# ------------------------------------------------------------------------------------------------ the argmax rule
def argmax_pixels(C):
    """[1, 7, C] float32, one pixel per rule of sa_better: a NaN after a larger number, two NaNs, all -inf, all negative, -0.0 before
    0.0, 0.0 before -0.0, and a lone maximum in the last channel.  The channels of interest sit in different lanes and steps."""
    nan, inf = float("nan"), float("inf")
    g = torch.Generator().manual_seed(E._seed(C, 79))
    px = -1.0 - E.wide((7, C), g).abs()                              # negative fillers, -1 .. -16
    lo, mid, hi = 0, C // 2, C - 1
    px[0, lo], px[0, hi] = 9.0, nan
    px[1, mid], px[1, hi] = nan, nan
    px[2, :] = -inf
    px[4, mid], px[4, hi] = -0.0, 0.0
    px[5, mid], px[5, hi] = 0.0, -0.0
    px[6, hi] = 3.0
    return px.view(1, 7, C)


@pytest.mark.parametrize("dtype,C", [pytest.param(dt, C, id=f"{_name(dt)}-C{C}") for dt, C, _, _ in FORMS if C > 1])
def test_argmax_rule_on_special_values(dtype, C):
    """amax is the index torch.max(dim) gives on the CPU and the maximum is the same value (NaN for NaN; the sign of a zero is not
    compared).  The kernel starts from (0, no channel): an all-negative or all -inf pixel shows a start at 0."""
    from unet_amd._lib import LIB
    dev = _dev()
    assert (dtype, C, form_of(C, dtype)) in {f[:3] for f in FORMS}
    px = argmax_pixels(C)
    want = torch.max(px.bfloat16().float() if dtype == BF16 else px, dim=2)
    assert want.indices.view(-1).tolist()[:3] == [C - 1, C // 2, 0] and want.indices.view(-1).tolist()[4:] == [C // 2, C // 2, C - 1]
    assert float(want.values.view(-1)[3]) < 0
    n = px.shape[1]
    x = px.to(dtype).view(1, 1, n, C).to(dev).contiguous()
    y = torch.empty_like(x)
    w = (E.sa_taps(3, torch.Generator().manual_seed(1)) / 128).float().to(dev)
    pool, amax, a = Tail(2 * n, dev), Tail(n, dev, torch.int32), Tail(n, dev)
    LIB.call("uh_spatial_attn_fwd", x.data_ptr(), C, w.data_ptr(), 3, pool.ptr, amax.ptr, a.ptr, y.data_ptr(), C, 1, 1, n, C, _dt(dtype), _st())
    torch.cuda.synchronize()
    got_max, got_idx = pool.head().view(n, 2)[:, 1], amax.head()
    a.head()
    assert got_idx.tolist() == want.indices.view(-1).tolist(), (got_idx.tolist(), want.indices.view(-1).tolist())
    assert torch.equal(got_max.isnan(), want.values.view(-1).isnan())
    assert torch.equal(got_max.nan_to_num(nan=0.0), want.values.view(-1).nan_to_num(nan=0.0))      # (-inf stays -inf; -0.0 == 0.0)
