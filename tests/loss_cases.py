"""Cases, float64 references, bounds and float32 restatements shared by tests/test_gpu_loss_ops.py (the kernels of csrc/loss.hip on
the MI355X) and tests/test_loss_ops_cpu.py (the CPU proof that the bounds are met by float32 arithmetic and broken by a mistake).

References.  BCE / CE mean, dice_coeff, dice_loss, multiclass_dice_coeff: oracle/losses_ref.py evaluated in float64 on the CPU, and
torch autograd on those functions for the gradients (the weights, n / n_mean and gscale enter linearly and are applied in float64).
boundary_loss: the same oracle on float32 CPU tensors (its constants are float32 by definition).

Bounds (derived in the docstring of tests/test_gpu_loss_ops.py): sums_bound, mean_bound, DICE_ABS, total_bound, grad_bound."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import losses_ref as L

U = 2.0 ** -24                       # half an ulp of 1.0f: the relative error of one float32 rounding
SUM_ULPS = 24                        # 8 (element) + 8 (a thread's adds) + 6 (shuffles) + 2 (LDS adds and the float store)
TINY = 2.0 ** -126                   # a term below the normal range loses at most this much, absolutely
DICE_ABS = 2 * SUM_ULPS * U + 4 * U
K_GRAD = 16                          # units of 2^-24 * M per gradient element (kernels); the float32 restatement must stay <= 8
K_RESTATEMENT = 8
BOUNDARY_TOL = 2e-5                  # relative, against the float32 oracle: the bound fixture G7 is held to
OP_TOL = 2e-5                        # the project's op-by-op bound (dice_coeff on random probabilities)

SHAPES = {
    "sub_wave": (1, 1, 3),           # fewer elements than a wave
    "two_blocks": (2, 37, 45),       # 3330: two blocks of the 2048 stride, ragged tail
    "second_sweep": (2, 517, 511),   # 258 partial rows: the finishing block's column sum takes a second sweep
    "grid_wrap": (1, 1031, 1021),    # 1 052 651 > 4096 * 256: the gradient kernels' grid goes round (514 partial rows)
}
SMALL = ("sub_wave", "two_blocks")
SCALES = (1.0, 10.0, 100.0)
WEIGHTS = ((1.0, 1.0), (1.0, 0.0), (0.0, 1.0), (0.3, 0.7))
GSCALES = (None, 0.5, 65536.0)
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def ulp32(v):
    return float(np.spacing(np.float32(abs(float(v)))))


# ------------------------------------------------------------------------------------------------ bounds
def sums_bound(s64, n, slack=0.0, frac=1.0):
    """slack: what the rounding of the inputs' difference x - max(x) costs a softmax column (see multiclass_ref); frac scales the
    accumulation budget alone (the CPU companion holds the restatement to half of it)."""
    return frac * SUM_ULPS * U * abs(float(s64)) + slack + n * TINY


def mean_bound(sum64, n, n_mean):
    """The BCE / CE mean: the sum's bound, the rounding of 1 / n_mean and of the product."""
    return sums_bound(sum64, n) / n_mean + 2 * U * abs(float(sum64)) / n_mean


def total_bound(parts, total):
    """parts: the bounds of the terms that were added."""
    return sum(parts) + ulp32(total)


def grad_bound(M, gscale):
    return K_GRAD * U * M * abs(1.0 if gscale is None else gscale)


def dice_k(inter, ssum, eps=1e-6):
    """(ka, kb) of d(1 - dice) / dp = ka * t + kb, from float64 sums (only their size enters the gradient bound's M)."""
    if ssum == 0:
        return 0.0, 0.0
    den = ssum + eps
    return -2.0 / den, (2.0 * inter + eps) / (den * den)


# ------------------------------------------------------------------------------------------------ binary cases
def binary_inputs(shape, scale, mask_div=2, soft=False):
    """fp32 logits [B,H,W] = N(0,1) * scale and an int64 mask with mask // mask_div in {0, 1} (soft: float targets in [0, 1])."""
    def make():
        B, H, W = SHAPES[shape]
        g = torch.Generator().manual_seed(11 + 1000 * mask_div + int(scale) + 7 * B * H + (500 if soft else 0))
        logits = torch.randn((B, H, W), generator=g) * scale
        # (a draw of 10^6 can hold an exact 0, where max(x, 0) and |x| of the oracle's BCE have their kinks and autograd returns
        # a subgradient of each piece, not the derivative of the sum)
        logits = torch.where(logits == 0, torch.full_like(logits, 0.5 * scale), logits)
        if soft:
            return logits, torch.rand((B, H, W), generator=g)
        return logits, torch.randint(0, 2 * mask_div, (B, H, W), generator=g)
    return _cached(("bin", shape, scale, mask_div, soft), make)


def wide_mask_case():
    """Four elements, two of them >= 2^31 (the 64-bit division of uh_mask_quot), divisor 2^31 - 1: targets 1, 0, 1, 1."""
    d = 2 ** 31 - 1
    logits = torch.tensor([[[0.75, -1.5, 2.25, -0.5]]])
    mask = torch.tensor([[[2 ** 31, 5, 2 ** 31 - 1, 2 ** 32 - 3]]], dtype=torch.int64)
    assert (mask // d).flatten().tolist() == [1, 0, 1, 1]
    return logits, mask, d


def empty_sets_case():
    """S == 0: sigmoid(-200) is 0 in float32 and no target is set."""
    B, H, W = SHAPES["two_blocks"]
    return torch.full((B, H, W), -200.0), torch.zeros((B, H, W), dtype=torch.int64)


def binary_ref(logits, target):
    """float64: sums {sum BCE, sum s t, sum s, sum t}, the two loss terms and their gradients d bce_mean / dx, d dice_loss / dx."""
    x = logits.double().requires_grad_()
    t = target.double()
    n = x.numel()
    bce = L.bce_with_logits_mean(x, t)
    s = torch.sigmoid(x)
    dice = L.dice_loss(s, t)
    g_bce, = torch.autograd.grad(bce, x, retain_graph=True)
    g_dice, = torch.autograd.grad(dice, x)
    sd = s.detach()
    sums = [float(bce.detach()) * n, float((sd * t).sum()), float(sd.sum()), float(t.sum())]
    assert not bool((logits == 0).any())
    ka, kb = dice_k(sums[1], sums[2] + sums[3])
    return {"n": n, "sums": sums, "bce": float(bce.detach()), "dice": float(dice.detach()), "g_bce": g_bce, "g_dice": g_dice, "ka": ka, "kb": kb}


def binary_ref_cached(shape, scale, mask_div=2, soft=False):
    def make():
        logits, m = binary_inputs(shape, scale, mask_div, soft)
        return binary_ref(logits, m if soft else m // mask_div)
    return _cached(("binref", shape, scale, mask_div, soft), make)


def binary_grad64(ref, n_mean, w_bce, w_dice, gscale):
    """(gradient, M): d [w_bce * sum BCE / n_mean + w_dice * dice_loss] / dx * gscale, and the bound's scale M."""
    gs = 1.0 if gscale is None else gscale
    g = gs * (w_bce * (ref["n"] / n_mean) * ref["g_bce"] + w_dice * ref["g_dice"])
    M = abs(w_bce) / n_mean + abs(w_dice) * (abs(ref["ka"]) + abs(ref["kb"])) / 4
    return g, M


# ------------------------------------------------------------------------------------------------ multi-class cases
def multiclass_inputs(shape, scale, C, labels="absent"):
    """fp32 NHWC logits [B,H,W,C] and int64 labels; "absent": the last class never occurs."""
    def make():
        B, H, W = SHAPES[shape]
        g = torch.Generator().manual_seed(5 + 1000 * C + int(scale) + 7 * B * H)
        logits = torch.randn((B, H, W, C), generator=g) * scale
        mask = torch.randint(0, C - 1 if labels == "absent" else C, (B, H, W), generator=g)
        return logits, mask
    return _cached(("mc", shape, scale, C, labels), make)


def multiclass_ref(logits, mask):
    """float64: sums {sum CE, sum p_c t_c, sum p_c, count_c}, CE mean, dice_loss and their gradients (NHWC)."""
    C = logits.shape[-1]
    x = logits.double().requires_grad_()
    bchw = x.permute(0, 3, 1, 2)
    onehot = F.one_hot(mask, C).permute(0, 3, 1, 2).double()
    ce = L.cross_entropy_mean(bchw, mask)
    p = torch.softmax(bchw, dim=1)
    dice = L.dice_loss(p, onehot, multiclass=True)
    g_ce, = torch.autograd.grad(ce, x, retain_graph=True)
    g_dice, = torch.autograd.grad(dice, x)
    pd = p.detach()
    npix = mask.numel()
    # both the kernel and float64 start from the float32 logits, but float32 rounds x_c - max(x) (relative 2^-24), so exp of it
    # is off by |x_c - max(x)| * 2^-24 relatively: nothing for the terms that make up a large sum, up to 104 units for a term at
    # the edge of underflow.  The weighted sum of that, from the float64 terms, is added to a softmax column's bound.
    xd = bchw.detach()
    dist = (xd - xd.max(1, keepdim=True).values).abs()
    slack = [0.0] + (U * (pd * onehot * dist).sum((0, 2, 3))).tolist() + (U * (pd * dist).sum((0, 2, 3))).tolist() + [0.0] * C
    sums = [float(ce.detach()) * npix] + (pd * onehot).sum((0, 2, 3)).tolist() + pd.sum((0, 2, 3)).tolist() + onehot.sum((0, 2, 3)).tolist()
    ka, kb = dice_k(sum(sums[1:1 + C]), sum(sums[1 + C:]))
    return {"n": npix, "C": C, "sums": sums, "slack": slack, "ce": float(ce.detach()), "dice": float(dice.detach()), "g_ce": g_ce, "g_dice": g_dice, "ka": ka, "kb": kb}


def multiclass_node_case():
    """SegLossMulticlassFn with its boundary term: (B, H, W, C, edge width, edge weight, w_boundary), N(0,1) logits that
    boundary_loss reads as they are (|v| <= 10), labels 0..3 (as float targets none of them is 255)."""
    def make():
        B, H, W, C = 3, 33, 47, 4
        g = torch.Generator().manual_seed(3347)
        logits = torch.randn((B, H, W, C), generator=g)
        mask = torch.randint(0, C, (B, H, W), generator=g)
        assert float(logits.abs().max()) <= 10
        return (B, H, W, C, 5, 3.0, 0.25), logits, mask
    return _cached("mcnode", make)


def multiclass_ref_cached(shape, scale, C, labels="absent"):
    return _cached(("mcref", shape, scale, C, labels), lambda: multiclass_ref(*multiclass_inputs(shape, scale, C, labels)))


def multiclass_grad64(ref, n_mean, w_ce, w_dice, gscale):
    gs = 1.0 if gscale is None else gscale
    g = gs * (w_ce * (ref["n"] / n_mean) * ref["g_ce"] + w_dice * ref["g_dice"])
    M = abs(w_ce) / n_mean + abs(w_dice) * (abs(ref["ka"]) + abs(ref["kb"]))
    return g, M


# ------------------------------------------------------------------------------------------------ comparisons
def check_sums(got, ref, counts=(), frac=1.0):
    """got: float32 sums (CPU); ref: a *_ref dictionary.  Columns in `counts` are equalities.  Returns the worst error, less the
    column's slack, in units of 2^-24 * S64 (the budget is SUM_ULPS of them)."""
    worst = 0.0
    n, slack = ref["n"], ref.get("slack")
    for k, want in enumerate(ref["sums"]):
        have = float(got[k])
        if k in counts:
            assert have == want, f"count column {k}: {have} != {want}"
            continue
        err, sl = abs(have - want), slack[k] if slack else 0.0
        bound = sums_bound(want, n, sl, frac)
        assert err <= bound, f"sums column {k}: {have!r} vs {want!r}: off by {err:.3e}, bound {bound:.3e}"
        if abs(want) > 1e-20:                                   # (below that the absolute floor is the bound that counts)
            worst = max(worst, max(err - sl, 0.0) / (U * abs(want)))
    return worst


def sums_hold(got, ref, counts=(), frac=1.0):
    try:
        check_sums(got, ref, counts, frac)
    except AssertionError:
        return False
    return True


def grad_units(got, g64, M, gscale):
    """The worst element of |got - g64| in units of 2^-24 * M * |gscale| (the bound is K_GRAD of them)."""
    gs = abs(1.0 if gscale is None else gscale)
    assert got.shape == g64.shape and bool(torch.isfinite(got).all())
    return float((got.double() - g64).abs().max()) / (U * M * gs)


# ------------------------------------------------------------------------------------------------ float32 restatements
def _f32(v):
    return torch.tensor(float(v), dtype=torch.float32)


def _dice_k32(I2, S, mistake):
    eps = _f32(1e-6)
    if float(S) == 0.0:
        return _f32(0.0), _f32(0.0)
    den = S + eps
    ka = _f32(-2.0) / den
    return (-ka if mistake == "ka_sign" else ka), (I2 + eps) / (den * den)


def binary_f32(logits, mask, mask_div, n_mean, w_bce, w_dice, gscale=None, sums=None, mistake=None):
    """The closed forms of the binary path in float32 torch.  Returns (sums [4], gradient).  mask: int64, or float targets with
    mask_div None.  mistake: None | "tail" | "n_for_n_mean" | "ka_sign" | "mask_div"."""
    x = logits.float().reshape(-1)
    if mask_div is None:
        t = mask.float().reshape(-1)
    else:
        t = (mask if mistake == "mask_div" else mask // mask_div).float().reshape(-1)
    n = x.numel()
    e = torch.exp(-x.abs())
    s = torch.where(x >= 0, 1 / (1 + e), e / (1 + e))
    terms = torch.stack([x.clamp_min(0) - x * t + torch.log1p(e), s * t, s, t])
    if mistake == "tail":
        terms = terms[:, :-1]
    own = terms.sum(1)
    sm = own if sums is None else sums.float()
    ka, kb = _dice_k32(2 * sm[1], sm[2] + sm[3], mistake)
    inv_n = _f32(1.0 / (n if mistake == "n_for_n_mean" else n_mean))
    g = _f32(w_bce) * (s - t) * inv_n + _f32(w_dice) * (ka * t + kb) * s * (1 - s)
    if gscale is not None:
        g = _f32(gscale) * g
    if mistake == "tail":
        g[-1] = 0.0
    return own, g.reshape(logits.shape)


def multiclass_f32(logits, mask, n_mean, w_ce, w_dice, gscale=None, sums=None, mistake=None):
    """The closed forms of the multi-class path in float32 torch.  Returns (sums [1 + 3 C], gradient NHWC).
    mistake: None | "tail" | "n_for_n_mean" | "ka_sign" | "class_left_out"."""
    C = logits.shape[-1]
    x = logits.float().reshape(-1, C)
    t = mask.reshape(-1)
    n = t.numel()
    xl = x - x.max(1, keepdim=True).values
    ex = torch.exp(xl)
    den = ex.sum(1)
    p = ex * (1 / den)[:, None]
    oh = F.one_hot(t, C).float()
    ce = torch.log(den) - xl.gather(1, t[:, None]).squeeze(1)
    cut = slice(None, -1) if mistake == "tail" else slice(None)
    own = torch.cat([ce[cut].sum().reshape(1), (p * oh)[cut].sum(0), p[cut].sum(0), oh[cut].sum(0)])
    if mistake == "class_left_out":
        own = own.clone()
        own[[C, 2 * C, 3 * C]] = 0.0
    sm = own if sums is None else sums.float().clone()
    if mistake == "class_left_out":
        sm[[C, 2 * C, 3 * C]] = 0.0
    ka, kb = _dice_k32(2 * sm[1:1 + C].sum(), sm[1 + C:].sum(), mistake)
    inv_n = _f32(1.0 / (n if mistake == "n_for_n_mean" else n_mean))
    gd = ka * oh + kb
    dot = (p * gd).sum(1, keepdim=True)
    g = _f32(w_ce) * (p - oh) * inv_n + _f32(w_dice) * p * (gd - dot)
    if gscale is not None:
        g = _f32(gscale) * g
    if mistake == "tail":
        g[-1] = 0.0
    return own, g.reshape(logits.shape)


# ------------------------------------------------------------------------------------------------ dice_coeff cases
DICE_LAYOUTS = [(3, 1), (3, 255), (2, 4096), (2, 4097), (2, 12289), (4300, 4097)]      # (ngroups, group_len)
DICE_WS_ROWS = 8448                                                                    # partial rows the workspace holds


def dice_bpg(ngroups, group_len):
    """Blocks per group the entry point settles on (documented behaviour: halved until the rows fit the workspace)."""
    bpg = max(1, (group_len + 4095) // 4096)
    while bpg > 1 and ngroups * bpg > DICE_WS_ROWS:
        bpg >>= 1
    return bpg


def dice_integer_inputs(ngroups, group_len):
    """x in {0..3}, t in {0, 1}: every sum is an integer below 2^24, the same in any order.  Group 0 is all zero where there
    is more than one group."""
    def make():
        g = torch.Generator().manual_seed(ngroups * 31 + group_len)
        x = torch.randint(0, 4, (ngroups, group_len), generator=g, dtype=torch.int8)
        t = torch.randint(0, 2, (ngroups, group_len), generator=g, dtype=torch.int8)
        x[0] = 0
        t[0] = 0
        assert 3 * group_len < 2 ** 24
        xl, tl = x.long(), t.long()
        sums = torch.stack([(xl * tl).sum(1), xl.sum(1), tl.sum(1)], 1).double()
        return x, t, sums
    return _cached(("dice", ngroups, group_len), make)


def dice_from_sums64(sums, eps=1e-6):
    inter = 2.0 * sums[:, 0]
    sets = sums[:, 1] + sums[:, 2]
    sets = torch.where(sets == 0, inter, sets)
    return float(((inter + eps) / (sets + eps)).mean())


# ------------------------------------------------------------------------------------------------ boundary cases
SWEEP = [(B, H, W, ew) for B in (1, 2) for H in range(1, 8) for W in range(1, 8) for ew in range(6)]
SWEEP_EDGE_WEIGHT = 2.0


def boundary_sweep_case(B, H, W, ew):
    g = torch.Generator().manual_seed(((B * 8 + H) * 8 + W) * 8 + ew)
    pred = torch.where(torch.rand((B, H, W), generator=g) < 0.5, 0.25, 0.75).float()
    target = torch.tensor([0.0, 128.0, 255.0])[torch.randint(0, 3, (B, H, W), generator=g)]
    return pred, target


# name -> (B, H, W, edge width, edge weight, channels, kind)
BOUNDARY_MID = {
    "seams": (2, 37, 45, 5, 3.0, 1, "prob"),            # region runs cross the seam between the two blocks
    "one_row_interior": (1, 3, 1031, 1, 1.0, 1, "prob"),
    "channel_1_of_4": (3, 33, 47, 5, 3.0, 4, "prob"),
    "sigmoid": (2, 37, 45, 5, 3.0, 1, "logit"),
}


def boundary_mid_case(name):
    """pred [B,H,W] (or [B,H,W,C], the loss reads channel 1) and float targets in {0, 128, 255}.  "prob": values in
    {0.25, 0.5, 0.75} (0.5 itself is not above the threshold); "logit": N(0,1) * 8 pushed off |v| < 1e-3."""
    def make():
        B, H, W, ew, wt, C, kind = BOUNDARY_MID[name]
        g = torch.Generator().manual_seed(B * 1000 + H * W + C)
        shape = (B, H, W) if C == 1 else (B, H, W, C)
        if kind == "prob":
            pred = torch.tensor([0.25, 0.5, 0.75])[torch.randint(0, 3, shape, generator=g)]
        else:
            v = torch.randn(shape, generator=g) * 8
            pred = torch.where(v.abs() < 1e-3, torch.full_like(v, 1e-3), v)
            assert float(pred.abs().max()) > 10 and float(pred.abs().min()) >= 1e-3      # sigmoid(v) > 0.5 sits on no rounding
        target = torch.tensor([0.0, 128.0, 255.0])[torch.randint(0, 3, (B, H, W), generator=g)]
        return pred.float().contiguous(), target
    return _cached(("bmid", name), make)


def boundary_oracle(pred, target, ew, wt):
    """The float32 oracle.  pred [B,H,W] or NHWC [B,H,W,C]."""
    p = pred.float()
    if p.dim() == 4:
        p = p.permute(0, 3, 1, 2)
    return float(L.boundary_loss(p, target, edge_width=ew, edge_weight=wt))


def _thresholded(pred, target):
    p = pred.float()
    if p.dim() == 4:
        p = p[..., 1]
    if bool(p.min() < -10) or bool(p.max() > 10):
        p = torch.sigmoid(p)
    return p, (target == 255).float()


def oracle_counts(pred, target, ew):
    """The oracle's own counts [inter, psum, tsum] x [interior, edge] and the two region sizes, by its own region code."""
    p, t = _thresholded(pred, target)
    B, H, W = p.shape
    em = L.edge_mask(B, H, W, ew)
    counts, sizes = [], []
    for region in (~em, em):
        if not bool(region.any()):
            counts += [0, 0, 0]
            sizes.append(0)
            continue
        n = int(region.sum()) // B
        pb = L._dilate3_gather_order((p[region].reshape(B, n) > 0.5).float())
        tb = L._dilate3_gather_order((t[region].reshape(B, n) > 0.5).float())
        counts += [int((pb * tb).sum()), int(pb.sum()), int(tb.sum())]
        sizes.append(B * n)
    return counts, sizes


def region_loss_from_counts(inter, psum, tsum, N, smooth=1e-6):
    """The oracle's region formula as a function of its counts: float64 arithmetic on the oracle's four float32 pixel terms."""
    if N <= 0:
        return 0.0
    iou = (inter + smooth) / (psum + tsum - inter + smooth)
    n11, n10, n01, n00 = inter, psum - inter, tsum - inter, N - psum - tsum + inter
    return (1 - iou) + 0.5 * (n11 * _pixel_bce(1, 1) + n10 * _pixel_bce(1, 0) + n01 * _pixel_bce(0, 1) + n00 * _pixel_bce(0, 0)) / N


def _pixel_bce(pb, tb):
    """One pixel's BCE as the oracle forms it, in float32: about 13.8 where the dilated maps disagree; 2^-20 (not 1e-6: the
    float32 difference x - logsigmoid(x) at x = -13.8 is one ulp of x) where both are 0, 1e-6 where both are 1."""
    def make():
        q = torch.tensor([float(pb)]).clamp(1e-6, 1 - 1e-6).clamp(1e-12, 1 - 1e-12)
        return float(F.binary_cross_entropy_with_logits(torch.log(q / (1 - q)), torch.tensor([float(tb)]), reduction="sum"))
    return _cached(("pixel_bce", pb, tb), make)


def loss_from_counts(counts, sizes, wt):
    return (region_loss_from_counts(*counts[:3], sizes[0]) + wt * region_loss_from_counts(*counts[3:], sizes[1])) / (1 + wt)


def _valid(c, N):
    inter, psum, tsum = c
    return 0 <= inter <= min(psum, tsum) and max(psum, tsum) <= N and N - psum - tsum + inter >= 0


def boundary_sensitivity(counts, sizes, wt):
    """The smallest relative change of the loss over every admissible +-1 of one of the oracle's six counts."""
    base = loss_from_counts(counts, sizes, wt)
    smallest = math.inf
    for k in range(6):
        for d in (-1, 1):
            c = list(counts)
            c[k] += d
            if sizes[k // 3] == 0 or not _valid(c[3 * (k // 3):3 * (k // 3) + 3], sizes[k // 3]):
                continue
            smallest = min(smallest, abs(loss_from_counts(c, sizes, wt) - base) / abs(base))
    return base, smallest


def assert_boundary_condition(pred, target, ew, wt, want):
    """One miscounted pixel moves the loss by at least 4 tolerances; the count formula reproduces the oracle's value."""
    counts, sizes = oracle_counts(pred, target, ew)
    base, smallest = boundary_sensitivity(counts, sizes, wt)
    assert abs(base - want) <= 2e-6 * abs(want), (base, want)
    assert smallest >= 4 * BOUNDARY_TOL, (smallest, counts, sizes)
    return smallest


def port_counts(pred, target, ew, mistake=None):
    """A Python port of the neighbour logic (every pixel finds the previous / next pixel of its own region analytically).
    mistake: None | "across_interior" (an edge pixel's neighbour taken across the interior run) | "ge" (>= for > at 0.5)."""
    p, t = _thresholded(pred, target)
    B, H, W = p.shape
    pbin = (p >= 0.5 if mistake == "ge" else p > 0.5).reshape(B, -1).tolist()
    tbin = (t > 0.5).reshape(B, -1).tolist()
    empty = ew > 0 and (2 * ew >= H or 2 * ew >= W)

    def is_edge(h, w):
        return ew != 0 and (h < ew or h >= H - ew or w < ew or w >= W - ew)

    def prev(h, w, edge):
        if not edge:
            if w - 1 >= ew:
                return h * W + w - 1
            return (h - 1) * W + W - ew - 1 if h - 1 >= ew else -1
        ph, pw = (h, w - 1) if w > 0 else (h - 1, W - 1)
        if ph < 0:
            return -1
        if not empty and not is_edge(ph, pw) and mistake != "across_interior":
            pw = ew - 1
        return ph * W + pw

    def nxt(h, w, edge):
        if not edge:
            if w + 1 < W - ew:
                return h * W + w + 1
            return (h + 1) * W + ew if h + 1 < H - ew else -1
        nh, nw = (h, w + 1) if w + 1 < W else (h + 1, 0)
        if nh >= H:
            return -1
        if not empty and not is_edge(nh, nw) and mistake != "across_interior":
            nw = W - ew
        return nh * W + nw

    counts = [0] * 6
    for h in range(H):
        for w in range(W):
            edge = False if ew == 0 else (True if empty else is_edge(h, w))
            nb = [r for r in (h * W + w, prev(h, w, edge), nxt(h, w, edge)) if r >= 0]
            o = 3 if edge else 0
            for b in range(B):
                pd = any(pbin[b][r] for r in nb)
                td = any(tbin[b][r] for r in nb)
                counts[o] += pd and td
                counts[o + 1] += pd
                counts[o + 2] += td
    n_int = 0 if empty else (H * W if ew == 0 else (H - 2 * ew) * (W - 2 * ew))
    return counts, [B * n_int, B * (H * W - n_int)]


# ------------------------------------------------------------------------------------------------ the case lists both files run
# (shape, scale, mask_div, soft targets)
BINARY_CASES = ([(sh, s, 2, False) for sh in SMALL for s in SCALES] +
                [("two_blocks", 10.0, 1, False), ("two_blocks", 10.0, 3, False), ("two_blocks", 1.0, 2, True),
                 ("two_blocks", 100.0, 2, True), ("second_sweep", 1.0, 2, False), ("second_sweep", 100.0, 2, False),
                 ("grid_wrap", 10.0, 2, False)])
# (n_mean / n, (w_bce, w_dice), gscale): the whole grid on the small shapes, two corners of it on the large ones
GRAD_GRID = [(world, w, gs) for world in (1, 2) for w in WEIGHTS for gs in GSCALES]
GRAD_CORNERS = [(1, (1.0, 1.0), None), (2, (0.3, 0.7), 0.5)]
# (shape, scale, classes, labels)
MULTICLASS_CASES = ([("two_blocks", s, C, lab) for C in range(2, 9) for s in SCALES for lab in ("absent", "all")] +
                    [("sub_wave", s, C, "absent") for C in (2, 5, 8) for s in SCALES] +
                    [("second_sweep", 10.0, 2, "all"), ("grid_wrap", 1.0, 2, "all")])


def grad_settings(shape):
    return GRAD_GRID if shape in SMALL else GRAD_CORNERS
