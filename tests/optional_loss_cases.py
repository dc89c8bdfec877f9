"""Cases, float64 references, bounds and float32 restatements shared by tests/test_gpu_optional_loss_ops.py (the kernels of
csrc/focal_loss.hip, csrc/surface_loss.hip and csrc/distill_loss.hip on the MI355X) and tests/test_optional_loss_ops_cpu.py (the CPU
proof that float32 arithmetic meets the bounds and that a seeded mistake breaks them).  The pattern is tests/loss_cases.py's.

Shapes and what each reaches (asserted by launch_facts() from the launch formulas, so a change of the constants fails on the CPU):
sub_wave (1,1,3); two_blocks (2,37,45) = 3330, two partial rows and a ragged tail; second_sweep (2,517,511): 258 rows, so
column_sum_256 and sl_finish_kernel sweep twice; grid_wrap (1,1031,1021) = 1 052 651 > 4096 * 256: 514 rows and the gradient / map
grids go round; above_cap (2,1031,1021): 1028 rows asked for, LOSS_MAXBLK = 1024 given (sums passes only).

References.  focal_tversky_ref, distill_ref, surface_loss_ref in float64 on the CPU; their closed-form gradients, which
test_optional_loss_ops_cpu.py shows equal to autograd at the two small shapes.

The saturated family is exact.  Logits are one-hot at +-SAT_HALF (the one-channel head: +-2 SAT_HALF against its implied 0), for
distillation times SAT_T = 2, so every shifted and scaled logit is 0 or -128 and expf(-128) = 0 in float32: every probability is 0 or
1 and log1pf(rest) = 0.  With class weights that are powers of two every focal column is a small integer combination (F = 128 sum of
w_t over the disagreeing pixels), both distillation columns are (128 #disagree, #agree), and the surface value is the sum of phi over
the pixels whose sure class is selected: float32 values that are 0 or multiples of 2^-23 not below 1, whose absolute sum stays
below 2^30, so every partial sum is exact in double in any order.  The disagreeing / selected pixels sit on special_indices(n).

Bounds, with u = 2^-24 (derived here, before any kernel ran; k and K are NOT chosen: R is the next power of two above the worst a
float32 torch restatement of the kernel's arithmetic shows against float64 over every case, the kernels get 2 R):
  * sums columns of non-negative terms (focal F, TP_c, P_c): loss_cases.sums_bound, 24 u S64 + slack + n 2^-126.  The slack is
    what the rounding of x_c - max(x) costs expf (u |x_c - max| relatively, loss_cases.multiclass_ref) and, for F, what
    u^gamma = exp2(gamma log2 u) adds: gamma (|log2 u| + d_u) u relatively, d_u the p-weighted |x_c - max| of the classes in u.
    Counts (T_c, agree) and W (weights are multiples of 1/4 and W 4 < 2^24) are equalities.
  * the kd sum cancels (q_c (a_c - b_c) against the log1p difference):  |got - S64| <= k u A + slack + n 2^-126 with
    A = sum_x [sum_c q_c (|a_c| + |b_c|) + |l1p_t| + |l1p_s|]  and  slack = u sum_x sum_c [q_c |a_c| (|a_c - b_c| + 1) + p_c |b_c|]
    (expf of the rounded a_c moves q_c by q_c |a_c| u, and the same through log1p).
  * the surface value is a signed sum formed in double from float32 probabilities:
    |got - v64| <= (k u sum |p_c phi_c| + u sum p_c |x_c - max| |phi_c|) / (n_mean K) + u |v64| (the float store).
  * finishes (focal, distillation) are double arithmetic on float32 sums and one float store: given the float64 sums rounded to
    float32, |got - f64(those)| <= half an ulp of the value + 2^-40 of the largest term.
  * gradients, per element:  |got - g64| <= |gscale| (K u M_x + slack_x), M_x from the float64 pieces of that pixel:
      focal         M = |w_t s / W| + 2 max_c |g_c|;  slack = u [|w_t s / W| |tau_k - p_k| (gamma (|log2 u| + d_u) + e_k) +
                    2 p_k |x_k - max| max_c |g_c|], e_k = d_u for k = t, |x_k - max| otherwise
      surface       M = scale p_k (|phi_k| + |dot|), slack = u scale p_k (|x_k - max| (|phi_k| + |dot|) + sum_c p_c |x_c - max| |phi_c|)
                    plus 2^-126 scale (|phi_k| + |dot|) for a p_k below the normal range; binary: M = scale |phi| / 4
                    Finding, on the CPU, before any kernel ran: with K >= 2 selected classes phi_c < 0 inside one class is > 0 for the
                    others, dot cancels and |dot| in M no longer covers the roundings of its K products (the restatement sat at
                    290 units).  The arithmetic is the natural float32 one, so the bound carries (K + 3) u scale p_k sum_c p_c |phi_c|
                    for K >= 2 (each product: expf, the reciprocal, p = x inv and its own rounding; K - 1 additions).
      distillation  M = w T / n_mean (p_k |a_k| <= 1/e: the rounded difference costs a bounded absolute amount, inside K)
    Every element also has the floor 2^-126 (a product below the normal range).
  R / 2 R (the restatement's worst on the CPU in brackets; test_optional_loss_ops_cpu.py re-measures it at every case, requires <= R
  and requires R to be the next power of two above it):  focal gradient 4 / 8 (3.80); surface gradient, softmax heads 16 / 32
  (8.10), sigmoid head 8 / 16 (5.93); distillation gradient 4 / 8 (3.77); kd sum 2 / 4 (1.22); surface value 1 / 2 (0.00: the
  sum is formed in double).  Sums columns of non-negative terms keep loss_cases.SUM_ULPS = 24, the restatement half of it (2.00).
  Finding, on the CPU: the float64 reference's -log p_t = logsumexp(z) - z_t keeps no digit below 1e-16 |z|, where the kernel's
  log1p form does (F = 1.2e-36 against a reference of 0.0 at three sure pixels); focal_ref forms it as log1p(rest) + (max - z_t).
  Finding, on the CPU: u formed as 1 - p_t does NOT leave the per-element gradient bound (M carries the factor u^gamma itself and
  the Tversky part, the elements carry tau_k - p_k <= u on top), nor the F column of a mixed batch; it leaves the F column where
  the batch is made of easy pixels alone (FOCAL_EASY)."""
import numpy as np
import torch

import distill_ref as DR
import focal_tversky_ref as FR
import loss_cases as L
import surface_loss_ref as SR

U = L.U
TINY = L.TINY
ulp32 = L.ulp32

# R: ceiling of the float32 restatement (next power of two above its worst over every case); the kernels are held to 2 R
# (measured worst of the restatement in the comment)
R_FOCAL_GRAD, K_FOCAL_GRAD = 4, 8                    # 3.80
R_SURFACE_GRAD, K_SURFACE_GRAD = 16, 32              # 8.10, softmax heads (C = 8, K = 1, s = 1; every other case is below 6.5)
R_SURFACE_GRAD_BINARY, K_SURFACE_GRAD_BINARY = 8, 16 # 5.93: sg (1 - sg) at sg near 1 costs u / 2 absolutely, against M = |phi| / 4
R_DISTILL_GRAD, K_DISTILL_GRAD = 4, 8                # 3.77
R_KD_SUM, K_KD_SUM = 2, 4                            # 1.22
R_SURFACE_VALUE, K_SURFACE_VALUE = 1, 2              # 0.00: the sum is formed in double; the slack and the store cover the rest
SUMS_FRAC_RESTATEMENT = 0.5              # of loss_cases.SUM_ULPS, as tests/test_loss_ops_cpu.py holds its restatement

SHAPES = dict(L.SHAPES, above_cap=(2, 1031, 1021))
SMALL = L.SMALL
SCALES = L.SCALES
ROW_STRIDE, ROW_CAP = 2048, 1024         # loss_nblk: (n + 2047) / 2048 rows, at most LOSS_MAXBLK
GRID_CAP, BLOCK = 4096, 256              # uh_flat_grid(n, UH_GRID_CAP): (n + 255) / 256 blocks, at most 256 * 16
SWEEP = 256                              # rows one sweep of column_sum_256 / sl_finish_kernel takes
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def npix(shape):
    B, H, W = SHAPES[shape]
    return B * H * W


def rows_asked(n):
    return (n + ROW_STRIDE - 1) // ROW_STRIDE


def rows(n):
    return max(1, min(ROW_CAP, rows_asked(n)))


def grid(n):
    return max(1, min(GRID_CAP, (n + BLOCK - 1) // BLOCK))


def launch_facts():
    """What each shape reaches, from the launch formulas."""
    n = {k: npix(k) for k in SHAPES}
    facts = {
        "sub_wave": n["sub_wave"] == 3 and n["sub_wave"] < 64,
        "two_blocks": n["two_blocks"] == 3330 and rows(n["two_blocks"]) == 2 and n["two_blocks"] % ROW_STRIDE != 0,
        "second_sweep": n["second_sweep"] == 528374 and rows(n["second_sweep"]) == 258 > SWEEP and grid(n["second_sweep"]) * BLOCK >= n["second_sweep"],
        "grid_wrap": n["grid_wrap"] == 1052651 > GRID_CAP * BLOCK == 1048576 and rows(n["grid_wrap"]) == 514 and grid(n["grid_wrap"]) == GRID_CAP,
        "above_cap": n["above_cap"] == 2105302 and rows_asked(n["above_cap"]) == 1028 > ROW_CAP == rows(n["above_cap"]),
    }
    assert all(facts.values()), facts
    return facts


launch_facts()


def special_indices(n):
    """Where a walk can slip: the first block's and first row's ends, the seam where the sums pass (rows * 256) and the gradient
    pass (grid * 256) start their second trip, the first index of the last partial row, the last pixel."""
    r, g = rows(n), grid(n)
    want = [0, 255, 256, 2047, 2048, g * BLOCK - 1, g * BLOCK, r * BLOCK - 1, r * BLOCK, (r - 1) * BLOCK, n - 1]
    return sorted({i for i in want if 0 <= i < n})


def _gen(*key):
    """A seeded generator per case (the hash of a tuple of numbers is not salted: the same draw in every process)."""
    return torch.Generator().manual_seed(abs(hash(tuple(float(k) if not isinstance(k, str) else sum(map(ord, k)) for k in key))) % (2 ** 31))


def _f32(v):
    return torch.tensor(float(v), dtype=torch.float32)


def two_class(z):
    return torch.stack([torch.zeros_like(z), z], dim=1)


def head_form(logits, ncls):
    """[n] (one-channel head) or [n, C] logits -> [n, C] with C = 2 on (0, z) for the one-channel head."""
    return two_class(logits) if ncls == 1 else logits


def _dist(z):
    return (z - z.max(1, keepdim=True).values).abs()


# ================================================================================================ the saturated family
SAT_HALF = 64.0
SAT_T = 2.0
SAT_GAMMAS = (0.0, 2.0, 1.5)
SAT_PRICES = ((0.5, 0.5), (0.25, 0.75))           # dyadic: every product of the Tversky finish is exact


def sat_weights(C):
    return tuple(2.0 ** (c % 3 - 1) for c in range(C))


def sat_logits(hot, ncls, half):
    if ncls == 1:
        return torch.where(hot == 1, 2 * half, -2 * half).float()
    return torch.where(torch.nn.functional.one_hot(hot, ncls).bool(), half, -half).float()


def sat_conditions():
    """expf(-128) is 0 in float32 and log1pf(0) is 0: asserted on the CPU."""
    e = torch.exp(torch.tensor([-2 * SAT_HALF, -2 * SAT_HALF * SAT_T / SAT_T], dtype=torch.float32))
    assert e.tolist() == [0.0, 0.0] and float(torch.log1p(e[0])) == 0.0
    assert float(torch.exp2(torch.tensor(1.5) * torch.log2(torch.tensor(1.0)))) == 1.0
    return True


def _sat_hot(shape, ncls, what):
    n = npix(shape)
    C = 2 if ncls == 1 else ncls
    g = _gen("sat", what, shape, ncls)
    hot = torch.randint(0, C, (n,), generator=g)
    other = (hot + 1 + torch.randint(0, C - 1, (n,), generator=g)) % C
    sp = torch.tensor(special_indices(n))
    return n, C, g, hot, other, sp


def sat_focal_case(shape, ncls):
    """(logits, mask, mask_div, weights, sums64 [2 + 3 C] as exact float64): the prediction is sure everywhere, the label
    disagrees on the special indices, and (beyond a wave) three pixels carry labels outside the head, one of them the mask -1."""
    def make():
        n, C, g, hot, other, sp = _sat_hot(shape, ncls, "focal")
        t = hot.clone()
        t[sp] = other[sp]
        if n > 64:
            t[1], t[n // 2 + 1] = C, 255
        w = sat_weights(C)
        mask, div = (2 * t + torch.randint(0, 2, (n,), generator=g), 2) if ncls == 1 else (t, 1)
        if n > 64:
            # -1 // mask_div is -1 (outside the head) for either divisor; a truncating division would make it class 0 under 2
            mask[n // 2 + 2], t[n // 2 + 2] = -1, -1
        tau, inside = FR.indicators(t, C)
        wt = torch.tensor(w, dtype=torch.float64)[torch.where(inside, t, torch.zeros_like(t))] * inside
        p = torch.nn.functional.one_hot(hot, C).double()
        F = 2 * SAT_HALF * float((wt * (t != hot)).sum())
        sums = [F, float(wt.sum())] + (p * tau).sum(0).tolist() + p.sum(0).tolist() + tau.sum(0).tolist()
        assert all(float(np.float32(s)) == s and s * 4 < 2 ** 24 for s in sums) and F > 0
        return sat_logits(hot, ncls, SAT_HALF), mask, div, w, sums
    return _cached(("satf", shape, ncls), make)


def finish_bound(v, largest=1.0):
    """A finish is double arithmetic on float32 sums and one float store: half an ulp of the value and 2^-40 of the largest term."""
    return 0.5 * ulp32(v) + 2.0 ** -40 * max(abs(v), largest)


def focal_finish64(sums, C, alpha, beta, cls, rounded=True):
    """ft_finish_kernel's double arithmetic in its order -> (total, focal, tversky), rounded to float32 values or not."""
    F, W = float(sums[0]), float(sums[1])
    focal = F / W if W > 0 else 0.0
    tv = 0.0
    for c in range(C):
        if c in cls:
            TP, P, T = float(sums[2 + c]), float(sums[2 + C + c]), float(sums[2 + 2 * C + c])
            tv += 1.0 - (TP + 1e-6) / ((1.0 - alpha - beta) * TP + alpha * P + beta * T + 1e-6)
    tv /= float(len(cls))
    return [float(np.float32(v)) if rounded else v for v in (focal + tv, focal, tv)]


def sat_distill_case(shape, ncls):
    """(student, teacher, sums64 = [128 #disagree, #agree]); T = SAT_T."""
    def make():
        n, C, g, hot, other, sp = _sat_hot(shape, ncls, "kd")
        ht = hot.clone()
        ht[sp] = other[sp]
        sums = [2 * SAT_HALF * len(sp), float(n - len(sp))]
        return sat_logits(hot, ncls, SAT_HALF * SAT_T), sat_logits(ht, ncls, SAT_HALF * SAT_T), sums
    return _cached(("satd", shape, ncls), make)


def distill_finish64(sums, n_mean, T, w, rounded=True):
    kd = T * T / n_mean * float(sums[0])
    return [float(np.float32(v)) if rounded else v for v in (w * kd, kd, float(sums[1]) / n_mean)]


def surface_labels(shape, binary):
    """int64 [B,H,W]: class 2 on a few ellipses, a random mix of 0 and 1 elsewhere (binary: {0, 1} elsewhere, the target mask // 2)."""
    def make():
        B, H, W = SHAPES[shape]
        rng = np.random.default_rng(B * 1000 + H + W)
        return SR.blob_labels(rng, B, H, W, cls=2, others=(0, 1))
    return _cached(("sllab", shape), make)


def surface_phi(shape, classes, binary):
    return _cached(("phi", shape, tuple(classes), binary), lambda: SR.phi_maps(surface_labels(shape, binary), classes, binary=binary))


def sat_surface_case(shape, ncls, classes):
    """(logits, labels [B,H,W], phi [K,B,H,W] float32, S64): the sure class is random everywhere and the first selected class on
    the special indices; S64 = sum of phi_k where the sure class is classes[k] (binary: where the sigmoid is 1), exact."""
    def make():
        n, C, g, hot, other, sp = _sat_hot(shape, ncls, "sl")
        hot[sp] = 1 if ncls == 1 else classes[0]
        phi = surface_phi(shape, classes, ncls == 1)
        ph = torch.from_numpy(phi).double().reshape(len(classes), n)
        S, A = 0.0, 0.0
        for k, c in enumerate(classes):
            sel = hot == (1 if ncls == 1 else c)
            S += float(ph[k][sel].sum())
            A += float(ph[k][sel].abs().sum())
        nz = ph[ph != 0].abs()
        assert A < 2 ** 30 and (nz.numel() == 0 or float(nz.min()) >= 1.0)          # multiples of 2^-23 below 2^30: 53 bits
        assert bool((ph * 2 ** 23 == (ph * 2 ** 23).round()).all())
        return sat_logits(hot, ncls, SAT_HALF), surface_labels(shape, ncls == 1), phi, S
    return _cached(("sats", shape, ncls, tuple(classes)), make)


def surface_finish64(S, n_mean, K, w):
    v = float(np.float32(S * (1.0 / (n_mean * float(K)))))
    return [v, float(np.float32(np.float32(w) * np.float32(v)))]


SAT_HEADS = {s: ((1, 2, 3, 4, 8) if s in SMALL else (1, 3)) for s in SHAPES}
SAT_SURFACE = {s: ([(1, (1,)), (2, (1,)), (3, (2,)), (3, (1, 2)), (4, (1, 2, 3)), (5, (2, 4)), (8, (2,)), (8, tuple(range(1, 8)))]
                   if s in SMALL else [(1, (1,)), (3, (2,))]) for s in SHAPES}


# ================================================================================================ focal + Tversky
FOCAL_GAMMAS = (0.0, 1.0, 2.0, 1.5)
FOCAL_CASES = ([("two_blocks", s, C, FOCAL_GAMMAS[(i + j) % 4]) for i, C in enumerate((1, 2, 3, 4, 8)) for j, s in enumerate(SCALES)] +
               [("sub_wave", s, C, FOCAL_GAMMAS[(i + j + 1) % 4]) for i, C in enumerate((1, 3, 8)) for j, s in enumerate(SCALES)] +
               [("two_blocks", 10.0, 3, 1.5), ("two_blocks", 10.0, 3, 2.0),
                ("second_sweep", 10.0, 3, 2.0), ("second_sweep", 1.0, 1, 1.5), ("grid_wrap", 1.0, 3, 1.5), ("grid_wrap", 10.0, 1, 2.0)])
# scale 0.0 stands for the easy family: every pixel is classified right with a margin of 12 to 15 (u between 3e-7 and 2e-5), so the
# F column is made of easy terms alone and u formed as 1 - p_t (absolute error u / 2) is far outside its bound
FOCAL_EASY = [("sub_wave", 0.0, 3, 2.0), ("two_blocks", 0.0, 3, 2.0), ("sub_wave", 0.0, 1, 1.5)]
FOCAL_CASES = FOCAL_CASES + FOCAL_EASY
FOCAL_SUMS_ONLY = [("above_cap", 1.0, 3, 2.0), ("above_cap", 10.0, 1, 1.5)]
# (alpha, beta, Tversky classes or None for 1..C-1, gscale)
FOCAL_GRAD_SMALL = [(0.3, 0.7, None, None), (0.5, 0.5, (1,), 0.5), (0.3, 0.7, None, 65536.0)]
FOCAL_GRAD_LARGE = [(0.3, 0.7, None, 0.5)]


def focal_grad_settings(shape):
    return FOCAL_GRAD_SMALL if shape in SMALL else FOCAL_GRAD_LARGE


def focal_weights(C):
    return tuple(0.5 + 0.75 * c for c in range(C))          # multiples of 1/4


def focal_inputs(shape, scale, ncls):
    """(logits [n] or [n, C] float32, mask int64 [n], mask_div).  Beyond a wave 3 % of the labels lie outside the head."""
    def make():
        n = npix(shape)
        C = 2 if ncls == 1 else ncls
        g = _gen("focal", shape, scale, ncls)
        logits = torch.randn((n,) if ncls == 1 else (n, ncls), generator=g) * scale
        t = torch.randint(0, C, (n,), generator=g)
        if scale == 0.0:
            margin = 12 + 3 * torch.rand(n, generator=g)
            sure = torch.nn.functional.one_hot(t, C) * margin[:, None]
            noise = 0.5 * torch.randn((n, ncls), generator=g)
            logits = (2 * t - 1) * margin + noise[:, 0] if ncls == 1 else sure + noise
        elif n > 64:
            out = torch.tensor([C, 255] + ([-1] if ncls > 1 else []))[torch.randint(0, 2 + (ncls > 1), (n,), generator=g)]
            t = torch.where(torch.rand(n, generator=g) < 0.03, out, t)
        if ncls == 1:
            return logits, 2 * t + torch.randint(0, 2, (n,), generator=g), 2
        return logits, t, 1
    return _cached(("fin", shape, scale, ncls), make)


def focal_ref(logits, mask, div, ncls, gamma, w=None):
    """float64: the sums {F, W, TP_c, P_c, T_c}, their slack, and the per-pixel pieces the gradient's bound is made of."""
    z = head_form(logits, ncls).double()
    t = torch.div(mask, div, rounding_mode="floor")
    n, C = z.shape
    w = focal_weights(C) if w is None else w
    p, tau, log_u, _, wt = FR._pieces(z, t, w)
    # -log p_t as log1p(sum of the non-maximal exponentials) + (max - z_t): z_t - logsumexp(z) keeps no digit of it once it is
    # below 1e-16 of |z|, and the kernel's float32 log1p form does
    zm = z.max(1, keepdim=True).values
    top = torch.nn.functional.one_hot(DR.first_argmax(z), C).bool()
    nlp = (torch.log1p(torch.exp(z - zm).masked_fill(top, 0.0).sum(1)) + ((zm - z) * tau).sum(1)) * tau.sum(1)
    mod = torch.exp(gamma * log_u)
    u = log_u.exp()
    dist = _dist(z)
    du = ((p * (1 - tau) * dist).sum(1) / u.clamp_min(1e-300)).clamp_max(1e4)
    powslack = gamma * (log_u.abs() / np.log(2.0) + du)
    fterm = wt * mod * nlp
    sums = [float(fterm.sum()), float(wt.sum())] + (p * tau).sum(0).tolist() + p.sum(0).tolist() + tau.sum(0).tolist()
    slack = [U * float((fterm * (powslack + du)).sum()), 0.0] + (U * (p * tau * dist).sum(0)).tolist() + (U * (p * dist).sum(0)).tolist() + [0.0] * C
    assert float(np.float32(sums[1])) == sums[1] and sums[1] * 4 < 2 ** 24 and all(v * 4 == round(v * 4) for v in w)
    return {"n": n, "C": C, "w": w, "gamma": gamma, "sums": sums, "slack": slack, "z": z, "t": t,
            "pieces": (p, tau, u, log_u, nlp, wt, mod, dist, du, powslack)}


def focal_ref_cached(shape, scale, ncls, gamma):
    return _cached(("fref", shape, scale, ncls, gamma), lambda: focal_ref(*focal_inputs(shape, scale, ncls), ncls, gamma))


FOCAL_COUNTS = lambda C: (1,) + tuple(range(2 + 2 * C, 2 + 3 * C))      # noqa: E731   W and the T_c


def focal_grad64(ref, alpha, beta, cls, gscale, sums=None):
    """(g64 [n, C], bound [n, C] without K: (M, slack)) from the float64 closed forms, with the float64 sums rounded to float32
    (what the gradient kernel is handed)."""
    p, tau, u, log_u, nlp, wt, mod, dist, du, powslack = ref["pieces"]
    C, gamma = ref["C"], ref["gamma"]
    cls = tuple(range(1, C)) if cls is None else cls
    sm = torch.tensor(ref["sums"] if sums is None else sums, dtype=torch.float64).float().double()
    W, TP, P, T = sm[1], sm[2:2 + C], sm[2 + C:2 + 2 * C], sm[2 + 2 * C:]
    N, D = TP + FR.EPS, (1.0 - alpha - beta) * TP + alpha * P + beta * T + FR.EPS
    ind = torch.zeros(C, dtype=torch.float64)
    ind[list(cls)] = 1.0 / len(cls)
    ga, gb = -ind * (D - N * (1.0 - beta)) / (D * D), ind * N * alpha / (D * D)
    gsel = torch.where(tau.bool(), ga, gb)
    if gamma == 0:
        s = -torch.ones_like(u)
    else:
        q = (p * tau).sum(1)
        r = torch.where(u > 0, -nlp / torch.where(u > 0, u, torch.ones_like(u)), -torch.ones_like(u))
        s = gamma * mod * q * r - mod
    fk = wt / W * s
    tmp = tau * u[:, None] - (1.0 - tau) * p
    gs = 1.0 if gscale is None else gscale
    g = gs * (fk[:, None] * tmp + p * (gsel - (p * gsel).sum(1, keepdim=True)))
    gmax = float(torch.cat([ga, gb]).abs().max())
    M = (fk.abs() + 2 * gmax)[:, None].expand_as(p)
    ek = torch.where(tau.bool(), du[:, None], dist)
    slack = U * (fk.abs()[:, None] * tmp.abs() * (powslack[:, None] + ek) + 2 * gmax * p * dist)
    return g, M, slack


def grad_units(got, g64, M, slack, gscale):
    """The worst element of (|got - g64| / |gscale| - slack) / (u M): the bound is K of these units."""
    gs = abs(1.0 if gscale is None else gscale)
    assert got.shape == g64.shape and bool(torch.isfinite(got).all()), (got.shape, g64.shape)
    over = ((got.double() - g64).abs() / gs - slack - TINY).clamp_min(0)       # (a product below the normal range loses 2^-126 at most)
    units = torch.where(M > 0, over / (U * M.clamp_min(1e-300)), torch.where(over > 0, torch.full_like(over, float("inf")), over))
    return float(units.max())


def focal_f32(logits, mask, div, ncls, w, gamma, alpha=0.5, beta=0.5, cls=None, gscale=None, sums=None, mistake=None, twice_at=None):
    """ft_pixel, ft_sums_kernel and ft_grad_kernel in float32 torch.  Returns (sums [2 + 3 C], gradient [n] or [n, C]).
    mistake: None | "tail" | "twice" | "one_minus_pt" | "label_off_by_one" | "k_is_c" | "no_gscale" | "weight_outside" | "trunc_div"."""
    z = head_form(logits.float(), ncls)
    n, C = z.shape
    t = torch.div(mask, div, rounding_mode="trunc" if mistake == "trunc_div" else "floor")
    if mistake == "label_off_by_one":
        t = t + 1
    inside = (t >= 0) & (t < C)
    tc = torch.where(inside, t, torch.zeros_like(t))
    tau = torch.nn.functional.one_hot(tc, C).bool() & inside[:, None]
    wv = torch.tensor(w, dtype=torch.float32)
    wt = torch.where(inside, wv[tc], wv[t % C] if mistake == "weight_outside" else torch.zeros(()))
    m = z.max(1, keepdim=True).values
    am = torch.nn.functional.one_hot(DR.first_argmax(z), C).bool()
    x = torch.exp(z - m)
    rest = torch.where(am, torch.zeros(()), x).sum(1)
    su = torch.where(tau, torch.zeros(()), x).sum(1)
    zt = torch.where(inside, z.gather(1, tc[:, None]).squeeze(1), m.squeeze(1))
    inv = 1 / (1 + rest)
    p = x * inv[:, None]
    q = torch.where(tau, p, torch.zeros(())).sum(1)
    u = 1 - q if mistake == "one_minus_pt" else su * inv
    nlp = torch.log1p(rest) - (zt - m.squeeze(1))
    g32 = _f32(gamma)
    pw = {0.0: torch.ones_like(u), 1.0: u, 2.0: u * u}.get(float(gamma))
    if pw is None:
        pw = torch.exp2(g32 * torch.log2(u))
    tf = tau.float()
    cols = torch.cat([(wt * (pw * nlp))[:, None], wt[:, None], p * tf, p, tf], 1)
    if mistake == "tail":
        cols = cols[:-1]
    own = cols.sum(0)
    if mistake == "twice":
        own = own + cols[twice_at]
    sm = (own if sums is None else sums.float()).double()
    cls = tuple(range(1, C)) if cls is None else cls
    TP, P, T = sm[2:2 + C], sm[2 + C:2 + 2 * C], sm[2 + 2 * C:]
    N, D = TP + 1e-6, (1.0 - alpha - beta) * TP + alpha * P + beta * T + 1e-6
    ind = torch.zeros(C, dtype=torch.float64)
    ind[list(cls)] = 1.0 / (C if mistake == "k_is_c" else len(cls))
    ga, gb = (-ind * (D - N * (1.0 - beta)) / (D * D)).float(), (ind * N * alpha / (D * D)).float()
    inv_w = (1.0 / sm[1] if sm[1] > 0 else sm[1] * 0).float()
    if gamma == 0:
        s = -torch.ones_like(u)
    else:
        r = torch.where(u > 0, -nlp / torch.where(u > 0, u, torch.ones_like(u)), -torch.ones_like(u))
        s = pw * (g32 * q * r - 1)
    fk = wt * inv_w * s
    gsel = torch.where(tau, ga, gb)
    dot = (p * gsel).sum(1, keepdim=True)
    tmp = torch.where(tau, u[:, None], -p)
    g = fk[:, None] * tmp + p * (gsel - dot)
    if gscale is not None and mistake != "no_gscale":
        g = _f32(gscale) * g
    if mistake == "tail":
        g[-1] = 0.0
    return own, (g[:, 1] if ncls == 1 else g)


def pick(g, ncls):
    """The one-channel head's gradient is the second column of the two-class form."""
    return g[:, 1] if ncls == 1 else g


# ================================================================================================ distillation
KD_T = {1: 2.0, 2: 1.0, 3: 3.0, 4: 2.0, 8: 0.7}                # 3 and 0.7: 1 / T is no power of two
KD_W = 0.75
# (shape, scale, ncls, teacher): "free" = independent N(0,1) * scale; "near" = student + 1e-3 N(0,1) (the cancelling regime)
DISTILL_CASES = ([("two_blocks", s, C, "free") for C in (1, 2, 3, 4, 8) for s in SCALES] +
                 [("two_blocks", s, C, "near") for C in (1, 3, 8) for s in (1.0, 100.0)] +
                 [("sub_wave", s, C, "free") for C in (1, 3, 8) for s in SCALES] +
                 [("second_sweep", 10.0, 3, "free"), ("second_sweep", 1.0, 1, "near"), ("grid_wrap", 1.0, 3, "near"), ("grid_wrap", 10.0, 1, "free")])
DISTILL_SUMS_ONLY = [("above_cap", 1.0, 3, "free"), ("above_cap", 10.0, 1, "near")]
DISTILL_GRAD_SMALL = [(1, None), (2, 0.5), (1, 65536.0)]      # (n_mean / n, gscale)
DISTILL_GRAD_LARGE = [(2, 0.5)]


def distill_grad_settings(shape):
    return DISTILL_GRAD_SMALL if shape in SMALL else DISTILL_GRAD_LARGE


def distill_inputs(shape, scale, ncls, teacher):
    def make():
        n = npix(shape)
        g = _gen("kd", shape, scale, ncls, teacher)
        z = torch.randn((n,) if ncls == 1 else (n, ncls), generator=g) * scale
        v = torch.randn(z.shape, generator=g) * scale if teacher == "free" else z + 1e-3 * torch.randn(z.shape, generator=g)
        return z, v
    return _cached(("kin", shape, scale, ncls, teacher), make)


def distill_ref(z32, v32, ncls, T):
    """float64: sums {sum KL, sum agree}, the absolute sum A of the terms the kernel adds, the slack, p and q."""
    z, v = head_form(z32, ncls).double(), head_form(v32, ncls).double()
    n = z.shape[0]
    a, b = (v - v.max(1, keepdim=True).values) / T, (z - z.max(1, keepdim=True).values) / T
    l1t, l1s = torch.logsumexp(a, 1), torch.logsumexp(b, 1)
    q, p = torch.exp(a - l1t[:, None]), torch.exp(b - l1s[:, None])
    kl = (q * (a - b)).sum(1) - (l1t - l1s)
    A = float(((q * (a.abs() + b.abs())).sum(1) + l1t.abs() + l1s.abs()).sum())
    slack = U * float((q * a.abs() * ((a - b).abs() + 1) + p * b.abs()).sum())
    agree = float((DR.first_argmax(z) == DR.first_argmax(v)).sum())
    return {"n": n, "T": T, "sums": [float(kl.sum()), agree], "A": A, "slack": slack, "p": p, "q": q}


def distill_ref_cached(shape, scale, ncls, teacher):
    return _cached(("kref", shape, scale, ncls, teacher), lambda: distill_ref(*distill_inputs(shape, scale, ncls, teacher), ncls, KD_T[ncls]))


def kd_sum_bound(ref, k):
    return k * U * ref["A"] + ref["slack"] + ref["n"] * TINY


def kd_sum_units(got, ref):
    return max(abs(float(got) - ref["sums"][0]) - ref["slack"] - ref["n"] * TINY, 0.0) / (U * ref["A"]) if ref["A"] > 0 else 0.0


def distill_grad64(ref, n_mean, w, gscale):
    gs = 1.0 if gscale is None else gscale
    M = w * ref["T"] / n_mean
    return gs * M * (ref["p"] - ref["q"]), torch.full_like(ref["p"], M), torch.zeros_like(ref["p"])


def _kd_side32(z, inv_t):
    m = z.max(1, keepdim=True).values
    am = torch.nn.functional.one_hot(DR.first_argmax(z), z.shape[1]).bool()
    a = (z - m) * inv_t
    x = torch.exp(a)
    rest = torch.where(am, torch.zeros(()), x).sum(1)
    inv = 1 / (1 + rest)
    return a, x * inv[:, None], torch.log1p(rest), am


def distill_f32(z32, v32, ncls, T, n_mean, w, gscale=None, mistake=None, twice_at=None):
    """kd_side, kd_sums_kernel and kd_grad_kernel in float32 torch.  Returns (sums [2], gradient).
    mistake: None | "tail" | "twice" | "t_squared" | "no_gscale"."""
    z, v = head_form(z32.float(), ncls), head_form(v32.float(), ncls)
    inv_t = _f32(1.0 / T)
    sa, sp, sl, sam = _kd_side32(z, inv_t)
    ta, tp, tl, tam = _kd_side32(v, inv_t)
    kl = (tp * (ta - sa)).sum(1) - (tl - sl)
    cols = torch.stack([kl, (sam == tam).all(1).float()], 1)
    if mistake == "tail":
        cols = cols[:-1]
    own = cols.sum(0)
    if mistake == "twice":
        own = own + cols[twice_at]
    coef = _f32(w * (T * T if mistake == "t_squared" else T) / n_mean)
    k = coef if gscale is None or mistake == "no_gscale" else _f32(gscale) * coef
    d = sp - tp
    others = torch.where(sam, torch.zeros(()), d).sum(1, keepdim=True)
    g = k * torch.where(sam, -others, d)
    if mistake == "tail":
        g[-1] = 0.0
    return own, (g[:, 1] if ncls == 1 else g)


# ================================================================================================ surface loss
SURFACE_W = 0.5
# (shape, scale, ncls, classes)
SURFACE_CASES = ([("two_blocks", s, C, cls) for (C, cls) in SAT_SURFACE["two_blocks"] for s in ((10.0,) if C in (4, 5) else SCALES)] +
                 [("sub_wave", 10.0, C, cls) for (C, cls) in [(1, (1,)), (3, (2,)), (8, (1, 2))]] +
                 [("second_sweep", 10.0, 3, (2,)), ("second_sweep", 1.0, 1, (1,)), ("grid_wrap", 1.0, 3, (2,)), ("grid_wrap", 100.0, 1, (1,))])
SURFACE_SUMS_ONLY = [("above_cap", 1.0, 3, (2,)), ("above_cap", 10.0, 1, (1,))]
SURFACE_GRAD_SMALL = [(1, None), (2, 0.5), (1, 65536.0)]      # (n_mean / n, gscale)
SURFACE_GRAD_LARGE = [(2, 0.5)]


def surface_grad_r(ncls):
    """(R, 2 R) of the surface gradient for a head."""
    return (R_SURFACE_GRAD_BINARY, K_SURFACE_GRAD_BINARY) if ncls == 1 else (R_SURFACE_GRAD, K_SURFACE_GRAD)


def surface_grad_settings(shape):
    return SURFACE_GRAD_SMALL if shape in SMALL else SURFACE_GRAD_LARGE


def surface_inputs(shape, scale, ncls):
    """float32 logits [n] or NHWC-flat [n, C]."""
    def make():
        n = npix(shape)
        g = _gen("sl", shape, scale, ncls)
        return torch.randn((n,) if ncls == 1 else (n, ncls), generator=g) * scale
    return _cached(("sin", shape, scale, ncls), make)


def surface_ref(logits, phi, ncls, classes):
    """float64 pieces: p [n, C] (binary: sigma [n]), phik [n, C] (phi of a selected class in its channel, 0 elsewhere), the sum S,
    the absolute sum and the slack of the value."""
    K = len(classes)
    ph = torch.from_numpy(phi).double().reshape(K, -1)
    z = logits.double()
    n = z.shape[0]
    if ncls == 1:
        p = torch.sigmoid(z)
        terms = p * ph[0]
        return {"n": n, "K": 1, "ncls": 1, "p": p, "phik": ph[0], "S": float(terms.sum()), "A": float(terms.abs().sum()), "slack": 0.0}
    p = torch.softmax(z, 1)
    phik = torch.zeros_like(z)
    for k, c in enumerate(classes):
        phik[:, c] = ph[k]
    dist = _dist(z)
    terms = p * phik
    return {"n": n, "K": K, "ncls": ncls, "p": p, "phik": phik, "dist": dist, "S": float(terms.sum()), "A": float(terms.abs().sum()),
            "slack": U * float((terms.abs() * dist).sum())}


def surface_ref_cached(shape, scale, ncls, classes):
    return _cached(("sref", shape, scale, ncls, tuple(classes)),
                   lambda: surface_ref(surface_inputs(shape, scale, ncls), surface_phi(shape, classes, ncls == 1), ncls, classes))


def surface_value64(ref, n_mean):
    return ref["S"] / (n_mean * ref["K"])


def surface_value_bound(ref, n_mean, k):
    return (k * U * ref["A"] + ref["slack"]) / (n_mean * ref["K"]) + U * abs(surface_value64(ref, n_mean))


def surface_value_units(got, ref, n_mean):
    d = n_mean * ref["K"]
    over = max(abs(float(got) - surface_value64(ref, n_mean)) - ref["slack"] / d - U * abs(surface_value64(ref, n_mean)), 0.0)
    return over * d / (U * ref["A"]) if ref["A"] > 0 else (0.0 if over == 0 else float("inf"))


def surface_grad64(ref, n_mean, w, gscale):
    gs = 1.0 if gscale is None else gscale
    scale = w / (n_mean * ref["K"])
    p, phik = ref["p"], ref["phik"]
    if ref["ncls"] == 1:
        return gs * scale * phik * p * (1 - p), scale * phik.abs() / 4, torch.zeros_like(p)
    dot = (p * phik).sum(1, keepdim=True)
    reach = phik.abs() + dot.abs()
    M = scale * p * reach
    slack = U * scale * p * (ref["dist"] * reach + (p * ref["dist"] * phik.abs()).sum(1, keepdim=True)) + TINY * scale * reach
    if ref["K"] > 1:
        # Several selected classes: phi_c < 0 inside one class is > 0 for the others, so dot cancels while every one of its K
        # products carries expf, the reciprocal, p = x inv and its own rounding (4 u) and the sum K - 1 additions.  |dot| in M
        # does not cover that; the float32 arithmetic is the natural one, so the bound carries (K + 3) u sum_c p_c |phi_c|.
        slack = slack + (ref["K"] + 3) * U * scale * p * (p * phik.abs()).sum(1, keepdim=True)
    return gs * scale * p * (phik - dot), M, slack


def phi_port(labels, classes, binary, mistake=None):
    """sl_phi over the reference's border and distance: -r inside, +r outside, a border pixel -0.0.  mistake "border_sign":
    the border pixels +0.0."""
    q = np.asarray(labels) // 2 if binary else np.asarray(labels)
    out = SR.phi_maps(labels, classes, binary=binary).copy()
    if mistake == "border_sign":
        for k, c in enumerate(classes):
            out[k][(q == c) & (out[k] == 0)] = 0.0
    return out


def surface_f32(logits, phi, ncls, classes, n_mean, w, gscale=None, mistake=None, twice_at=None):
    """sl_softmax / sl_sigmoid, sl_sums_kernel + sl_finish_kernel and sl_grad_kernel in torch.  Returns ([value, w value], gradient).
    mistake: None | "tail" | "twice" | "class_off_by_one" | "k_is_c" | "no_gscale"."""
    K = len(classes)
    ph = torch.from_numpy(phi).float().reshape(K, -1)
    x = logits.float()
    Kd = ncls if mistake == "k_is_c" else K
    scale = _f32(w / (n_mean * Kd))
    gs = scale if gscale is None or mistake == "no_gscale" else _f32(gscale) * scale
    if ncls == 1:
        e = torch.exp(-x.abs())
        sg = torch.where(x >= 0, 1 / (1 + e), e / (1 + e))
        terms = sg.double() * ph[0].double()
        g = gs * (ph[0] * (sg * (1 - sg)))
    else:
        ex = torch.exp(x - x.max(1, keepdim=True).values)
        p = ex * (1 / ex.sum(1))[:, None]
        phk = torch.zeros_like(x)
        for k, c in enumerate(classes):
            phk[:, (c - 1) if mistake == "class_off_by_one" else c] = ph[k]
        terms = (p.double() * phk.double()).sum(1)
        dot = (p * phk).sum(1, keepdim=True)
        g = gs * (p * (phk - dot))
    if mistake == "tail":
        terms = terms[:-1]
        g[-1] = 0.0
    S = terms.sum()
    if mistake == "twice":
        S = S + terms[twice_at]
    v = (S * (1.0 / (n_mean * Kd))).float()
    return [float(v), float(_f32(w) * v)], g
