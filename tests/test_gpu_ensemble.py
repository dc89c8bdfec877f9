"""Checkpoint ensembles on the MI355X (DESIGN.md section 3 "Ensembles"): uh_ensemble_add against the integer sums the two merges
export, uh_ensemble_finish against the host's integer arithmetic on the kernel's own accumulator, the independence of the member
order, BatchPredictor(Ensemble(...)) and evaluate(Ensemble(...)) against the members run one by one, and the command lines.
Only the comparison with float64 (test 4) has a tolerance."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tta_ref as R  # noqa: E402
from test_gpu_tta import _image, _loader, _model  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1), (5, 7), (33, 31), (64, 48)]          # tails, odd pitches, more than one workgroup
BATCHES = (1, 3)
CLASSES = (1, 2, 3, 4, 7)
WEIGHTS = ([1, 1], [1, 2, 1], [3, 1, 1, 2, 1])
Q = 1 << 24


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _logits(rng, B, H, W, NC, dtype, dev):
    """Seeded N(0, 2^2) logits rounded to `dtype`: (numpy float32 NHWC, the NCHW tensor over NHWC memory a head returns)."""
    t = torch.from_numpy((2.0 * rng.standard_normal((B, H, W, NC))).astype(np.float32)).to(dtype)
    return t.float().numpy(), t.to(dev).permute(0, 3, 1, 2)


def _members(rng, n, B, H, W, NC, dtype, dev):
    return [_logits(rng, B, H, W, NC, dtype, dev) for _ in range(n)]


def _i64(t):
    return t.cpu().numpy().astype(np.int64)


def _dirty(B, H, W, NC, dev):
    return torch.full((B, H, W, NC), -1, dtype=torch.int64, device=dev)              # every byte 0xFF


def _add_all(ops, srcs, weights, dev, dirty=False):
    """ensemble_add over the members; dirty: the first member is assigned to a pre-filled accumulator through the entry point's
    `first` argument, as ops.ensemble_add does for a new one."""
    from unet_amd._lib import LIB
    acc = None
    for k, (s, w) in enumerate(zip(srcs, weights)):
        if k == 0 and dirty:
            v = s if s.dtype in (torch.int32, torch.int64) else s.permute(0, 2, 3, 1)
            assert v.is_contiguous()
            B, H, W, NC = v.shape
            acc = _dirty(B, H, W, NC, dev)
            kind = {torch.float32: 0, torch.bfloat16: 1, torch.int32: 3, torch.int64: 4}[v.dtype]
            LIB.call("uh_ensemble_add", v.data_ptr(), kind, B * H * W, NC, w, 1, acc.data_ptr(), None)
            torch.cuda.synchronize()
        else:
            acc = ops.ensemble_add(s, w, acc)
    return acc


# ------------------------------------------------------------------ 1. the integer part of add
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("H,W", SHAPES)
def test_add_of_logits_is_the_shared_quantiser(H, W, dtype):
    """acc == sum_m w_m q_m with q_m what uh_tile_merge returns at overlap 0 (every tent weight 1, den 1: the bare quantiser)."""
    from unet_amd import ops
    dev = _dev()
    rng = np.random.default_rng(H * 100 + W)
    for B in BATCHES:
        for NC in CLASSES:
            for weights in WEIGHTS:
                mem = _members(rng, len(weights), B, H, W, NC, dtype, dev)
                want = np.zeros((B, H, W, NC), np.int64)
                for (_, t), w in zip(mem, weights):
                    q = ops.tile_merge(t, "1024,overlap=0", (H, W), sums=True)
                    assert int(q.den.min()) == int(q.den.max()) == 1
                    want += w * _i64(q.sums)
                acc = _add_all(ops, [t for _, t in mem], weights, dev)
                assert acc.dtype == torch.int64 and tuple(acc.shape) == (B, H, W, NC)
                np.testing.assert_array_equal(_i64(acc), want, err_msg=f"{B} {NC} {weights}")
                np.testing.assert_array_equal(_i64(_add_all(ops, [t for _, t in mem], weights, dev, dirty=True)), want)


@pytest.mark.parametrize("H,W", SHAPES)
def test_add_of_view_sums(H, W):
    from unet_amd import ops
    from test_gpu_tta import _logits as view_logits
    dev = _dev()
    rng = np.random.default_rng(H * 100 + W + 1)
    for B in BATCHES:
        for NC in CLASSES:
            for weights, mode in zip(WEIGHTS, ("hflip", "d4", "hflip")):
                srcs = []
                for _ in weights:
                    (_, l0), (_, l1) = view_logits(rng, mode, B, H, W, NC, torch.bfloat16)
                    m = ops.tta_merge(l0.to(dev).permute(0, 3, 1, 2), None if l1 is None else l1.to(dev).permute(0, 3, 1, 2), mode,
                                      (H, W), sums=True)
                    assert m.sums.dtype == torch.int32
                    srcs.append(m.sums)
                want = sum(w * _i64(s) for s, w in zip(srcs, weights))
                np.testing.assert_array_equal(_i64(_add_all(ops, srcs, weights, dev)), want, err_msg=f"{B} {NC} {mode}")
                np.testing.assert_array_equal(_i64(_add_all(ops, srcs, weights, dev, dirty=True)), want)


def test_add_of_tile_sums():
    import unet_amd
    from unet_amd import ops
    dev = _dev()
    H, W, cfg = 64, 48, "32,overlap=8"
    ny, nx, th, tw, _, _ = unet_amd.tile_grid(H, W, unet_amd.TileConfig(32, 8))
    rng = np.random.default_rng(6448)
    for B in BATCHES:
        for NC in CLASSES:
            for weights in WEIGHTS:
                srcs = []
                for _ in weights:
                    _, t = _logits(rng, B * ny * nx, th, tw, NC, torch.float32, dev)
                    m = ops.tile_merge(t, cfg, (H, W), sums=True)
                    assert m.sums.dtype == torch.int64 and int(m.den.max()) > 1
                    srcs.append(m.sums)
                want = sum(w * _i64(s) for s, w in zip(srcs, weights))
                np.testing.assert_array_equal(_i64(_add_all(ops, srcs, weights, dev)), want, err_msg=f"{B} {NC} {weights}")
                np.testing.assert_array_equal(_i64(_add_all(ops, srcs, weights, dev, dirty=True)), want)


def _offset(t):
    """The same values in the same layout, one element into a fresh buffer: aligned to the element and no further."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    out = buf[1:].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 != 0 and out.is_contiguous()
    return out


@pytest.mark.parametrize("NC", CLASSES)
def test_bases_off_the_16_byte_grid_give_the_same_bytes(NC):
    """The element-by-element forms (a source or an accumulator that is not 16-byte aligned) against the wide ones."""
    from unet_amd import ops
    dev = _dev()
    rng = np.random.default_rng(NC + 40)
    B, H, W = 2, 33, 31
    weights = [2, 1, 3]
    for dtype in (torch.float32, torch.bfloat16, torch.int32, torch.int64):
        if dtype in (torch.int32, torch.int64):
            srcs = [torch.from_numpy(rng.integers(0, 1 << 27, (B, H, W, NC))).to(dev).to(dtype) for _ in weights]
            shifted = [_offset(s) for s in srcs]
        else:
            srcs = [t for _, t in _members(rng, 3, B, H, W, NC, dtype, dev)]
            shifted = [_offset(t.permute(0, 2, 3, 1)).permute(0, 3, 1, 2) for t in srcs]
        want = _add_all(ops, srcs, weights, dev)
        acc = _offset(_dirty(B, H, W, NC, dev))
        for k, (s, w) in enumerate(zip(shifted, weights)):
            if k == 0:
                from unet_amd._lib import LIB
                v = s if s.dtype in (torch.int32, torch.int64) else s.permute(0, 2, 3, 1)
                kind = {torch.float32: 0, torch.bfloat16: 1, torch.int32: 3, torch.int64: 4}[v.dtype]
                LIB.call("uh_ensemble_add", v.data_ptr(), kind, B * H * W, NC, w, 1, acc.data_ptr(), None)
            else:
                assert ops.ensemble_add(s, w, acc) is acc
        assert torch.equal(acc, want), dtype
        a = ops.ensemble_finish(want, 6, probs=True, confidence=True)
        b = ops.ensemble_finish(acc, 6, probs=True, confidence=True)
        assert torch.equal(a.classes, b.classes) and torch.equal(a.probs, b.probs) and torch.equal(a.confidence, b.confidence)


# ------------------------------------------------------------------ 2. the integer part of finish
def _finish_ref(acc, den, views, total):
    """classes, probs, confidence from the accumulator on the host, in Python / numpy integers."""
    B, H, W, NC = acc.shape
    d = np.ones((B, H, W), np.int64) if den is None else den.astype(np.int64)
    T = d * (views * total * Q)
    probs = (acc.astype(np.float64) / T[..., None].astype(np.float64)).astype(np.float32)
    if NC == 1:
        a = acc[..., 0]
        classes = (2 * a > T).astype(np.uint8)
        m = np.minimum(a, T)
        conf = ((255 * np.maximum(m, T - m)) // T).astype(np.uint8)
    else:
        classes = acc.argmax(-1).astype(np.uint8)                                    # numpy: the first maximum
        s = acc.sum(-1)
        conf = np.where(s > 0, (255 * acc.max(-1)) // np.maximum(s, 1), 0).astype(np.uint8)
    return classes, probs, conf


def _check_finish(ops, acc, total, views, den):
    got = ops.ensemble_finish(acc, total, views=views, den=den, probs=True, confidence=True)
    want_c, want_p, want_f = _finish_ref(_i64(acc), None if den is None else _i64(den), views, total)
    np.testing.assert_array_equal(got.classes.cpu().numpy(), want_c)
    assert got.probs.cpu().numpy().tobytes() == want_p.tobytes()
    np.testing.assert_array_equal(got.confidence.cpu().numpy(), want_f)
    only = ops.ensemble_finish(acc, total, views=views, den=den)
    assert only.probs is None and only.confidence is None and torch.equal(only.classes, got.classes)
    assert torch.equal(ops.ensemble_finish(acc, total, views=views, den=den, probs=True).probs, got.probs)
    assert torch.equal(ops.ensemble_finish(acc, total, views=views, den=den, confidence=True).confidence, got.confidence)
    return got


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("H,W", SHAPES)
def test_finish_integer_part(H, W, dtype):
    from unet_amd import ops
    from test_gpu_tta import _logits as view_logits
    dev = _dev()
    rng = np.random.default_rng(H * 100 + W + 2)
    for B in BATCHES:
        for NC in CLASSES:
            for weights in WEIGHTS:
                total = sum(weights)
                mem = _members(rng, len(weights), B, H, W, NC, dtype, dev)
                acc = _add_all(ops, [t for _, t in mem], weights, dev)
                got = _check_finish(ops, acc, total, 1, None)
                a = _i64(acc)
                if NC > 1:
                    assert np.abs(a.sum(-1) - total * Q).max() <= total * 2 * NC     # the members' roundings
                    assert int(got.confidence.min()) >= 255 // NC
                den = torch.from_numpy(rng.integers(1, 5, (B, H, W)).astype(np.int32)).to(dev)
                _check_finish(ops, acc * den[..., None].long(), total, 1, den)       # den given
                srcs = []
                for _ in weights:                                                    # views = 8: the sums of d4
                    (_, l0), (_, l1) = view_logits(rng, "d4", B, H, W, NC, dtype)
                    srcs.append(ops.tta_merge(l0.to(dev).permute(0, 3, 1, 2), l1.to(dev).permute(0, 3, 1, 2), "d4", (H, W),
                                              sums=True).sums)
                acc8 = _add_all(ops, srcs, weights, dev)
                _check_finish(ops, acc8, total, 8, None)
                _check_finish(ops, acc8 * den[..., None].long(), total, 8, den)


def test_finish_at_the_ends_of_the_range():
    """Hand-made accumulators: ties take the first maximum, an empty pixel has confidence 0, the one-class rule at T / 2, and
    sums near 2^59 (den views total_weight near 2^35, where 255 acc leaves 64 bits) against Python's integers."""
    from unet_amd import ops
    dev = _dev()
    acc = torch.tensor([[5, 5, 1], [0, 0, 0], [1, 7, 7], [0, 0, 9]], dtype=torch.int64, device=dev).view(1, 1, 4, 3)
    got = ops.ensemble_finish(acc, 1, confidence=True)
    assert got.classes.flatten().tolist() == [0, 0, 1, 2]
    assert got.confidence.flatten().tolist() == [255 * 5 // 11, 0, 255 * 7 // 15, 255]
    total, views = 3, 2
    T = views * total * Q
    vals = [0, 1, T // 2 - 1, T // 2, T // 2 + 1, T - 1, T, T + 5]
    one = torch.tensor(vals, dtype=torch.int64, device=dev).view(1, 1, len(vals), 1)
    got = ops.ensemble_finish(one, total, views=views, confidence=True)
    assert got.classes.flatten().tolist() == [int(2 * v > T) for v in vals]
    assert got.confidence.flatten().tolist() == [255 * max(min(v, T), T - min(v, T)) // T for v in vals]
    den_v, views, total = (1 << 22) - 3, 8, 1024
    T = den_v * views * total * Q                                                    # just below 2^59
    rows = [[T - 7, 5, 2], [T // 3, T // 3 + 1, T // 3], [T // 2, T // 2 - 1, 1], [1, T // 255, T - T // 255 - 1]]
    big = torch.tensor(rows, dtype=torch.int64, device=dev).view(1, 1, len(rows), 3)
    den = torch.full((1, 1, len(rows)), den_v, dtype=torch.int32, device=dev)
    got = ops.ensemble_finish(big, total, views=views, den=den, probs=True, confidence=True)
    assert got.confidence.flatten().tolist() == [255 * max(r) // sum(r) for r in rows]
    assert got.classes.flatten().tolist() == [r.index(max(r)) for r in rows]
    want_p = np.asarray([[np.float32(np.float64(v) / np.float64(T)) for v in r] for r in rows], np.float32)
    assert got.probs.cpu().numpy().tobytes() == want_p.tobytes()
    half = torch.tensor([T // 2, T // 2 + 1, T - 1, 3], dtype=torch.int64, device=dev).view(1, 1, 4, 1)
    got = ops.ensemble_finish(half, total, views=views, den=den, confidence=True)
    assert got.classes.flatten().tolist() == [0, 1, 1, 0]
    assert got.confidence.flatten().tolist() == [255 * max(v, T - v) // T for v in (T // 2, T // 2 + 1, T - 1, 3)]


# ------------------------------------------------------------------ 3. the member order
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_member_order_changes_nothing(dtype):
    from unet_amd import ops
    dev = _dev()
    rng = np.random.default_rng(3)
    for H, W in SHAPES:
        for NC in CLASSES:
            weights = [3, 1, 1, 2, 1]
            mem = [t for _, t in _members(rng, 5, 3, H, W, NC, dtype, dev)]
            ref = None
            for perm in ([0, 1, 2, 3, 4], [4, 3, 2, 1, 0], [2, 0, 4, 1, 3]):
                acc = _add_all(ops, [mem[i] for i in perm], [weights[i] for i in perm], dev)
                m = ops.ensemble_finish(acc, sum(weights), probs=True, confidence=True)
                got = (acc, m.classes, m.probs, m.confidence)
                if ref is None:
                    ref = got
                for a, b in zip(ref, got):
                    assert torch.equal(a, b), (H, W, NC, perm)


# ------------------------------------------------------------------ 4. against float64
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("NC", CLASSES)
def test_add_against_float64(NC, dtype):
    """|acc - S64| <= W (1 + 2 E), S64 = sum_m w_m p64_m 2^24, W the total weight, E the error of torch's own fp32 softmax on these
    logits in units of 2^-24 (measured here on the device): the derivation of test_gpu_tta.py::test_merge_against_float64 with a
    member in place of a view -- 1 covers the rounding of q, half a unit per unit of weight, with slack for the rounding of S64;
    2 E because two correct fp32 softmaxes may err in opposite directions.  The classes equal the float64 rule wherever the
    float64 top-two gap (one class: the distance to T / 2) exceeds twice that; at most 0.1 % of the pixels may be left out.
    Measured (MI355X, over NC and both dtypes): E 1.43 - 2.92, largest |acc - S64| 6.17 - 14.27 (bound at W = 8, E = 1.43: 30.9),
    at most 18 of 49572 pixels left out (bf16, one class); the table is in DESIGN.md section 3 "Ensembles"."""
    from unet_amd import ops
    dev = _dev()
    rng = np.random.default_rng(NC)
    worst_E = worst_dev = 0.0
    pixels = left_out = 0
    for H, W in SHAPES:
        for B in BATCHES:
            for weights in WEIGHTS:
                total = sum(weights)
                mem = _members(rng, len(weights), B, H, W, NC, dtype, dev)
                E = 0.0
                S64 = np.zeros((B, H, W, NC), np.float64)
                for (n, t), w in zip(mem, weights):
                    lf = t.permute(0, 2, 3, 1).float()
                    p32 = torch.sigmoid(lf) if NC == 1 else torch.softmax(lf, -1)
                    p64 = R.probabilities64(n)
                    E = max(E, float(np.abs(p32.cpu().numpy().astype(np.float64) * Q - p64 * Q).max()))
                    S64 += w * p64 * Q
                acc = _add_all(ops, [t for _, t in mem], weights, dev)
                got = ops.ensemble_finish(acc, total).classes.cpu().numpy()
                deviation = float(np.abs(_i64(acc).astype(np.float64) - S64).max())
                worst_E, worst_dev = max(worst_E, E), max(worst_dev, deviation)
                bound = total * (1 + 2 * E)
                assert deviation <= bound, (H, W, B, weights, deviation, bound, E)
                if NC == 1:
                    gap = np.abs(S64[..., 0] - total * (Q >> 1))
                    want = (S64[..., 0] > total * (Q >> 1)).astype(np.uint8)
                else:
                    top = np.sort(S64, axis=-1)
                    gap = top[..., -1] - top[..., -2]
                    want = S64.argmax(-1).astype(np.uint8)
                decided = gap > 2 * bound
                assert np.array_equal(got[decided], want[decided]), (H, W, B, weights)
                pixels += decided.size
                left_out += int((~decided).sum())
    print(f"ensemble add vs float64, NC={NC} {dtype}: E = {worst_E:.3f}, largest |acc - S64| = {worst_dev:.3f} (units of 2^-24); "
          f"{left_out} of {pixels} pixels left out")
    assert left_out <= 0.001 * pixels


# ------------------------------------------------------------------ 5. end to end
SIZES = ((40, 48), (33, 31))
_MODELS = {}


def _trio(dev, classes=3):
    """Three small random-init members (a seed each), built once; in eval mode whatever the last test left them in."""
    if classes not in _MODELS:
        _MODELS[classes] = [_model("UNet_T", classes, bil, dev, seed=s) for bil, s in ((True, 3), (False, 11), (True, 23))]
    return [m.to(dev).eval() for m in _MODELS[classes]]


def _prepared(img, dev):
    """What uh_predict_prepare_u8 makes of a uint8 image, as the network's input."""
    x = (img.astype(np.float32) / np.float32(255.0))[None, None]
    return torch.from_numpy(x).to(dev).contiguous(memory_format=torch.channels_last)


def _own_logits(model, x, amp):
    from unet_amd.inference import eval_forward
    return eval_forward(model, x, amp, plan_images=1).clone()


@pytest.mark.parametrize("amp", [True, False])
def test_predictor_is_order_and_batch_independent_and_equals_the_members(amp):
    import unet_amd
    from unet_amd import ops
    dev = _dev()
    a, b, c = _trio(dev)
    weights = [1, 2, 1]
    images = [_image(20 + k, H, W) for k in range(4) for H, W in SIZES]               # (f) mixed sizes in one call
    p = unet_amd.BatchPredictor(unet_amd.Ensemble([a, b, c], weights), batch=8, postprocess=False, amp=amp, batch_invariant=True)
    (cls, conf), prob = p.masks_and_confidence(images, grey=False), p.probabilities(images)
    assert all(r.shape == im.shape and r.dtype == np.uint8 for r, im in zip(cls, images))
    assert all(r.shape == im.shape and r.dtype == np.uint8 for r, im in zip(conf, images))
    assert any(len(np.unique(r)) > 1 for r in cls), "a constant prediction compares nothing"
    grey = p(images)
    for g, r in zip(grey, cls):
        np.testing.assert_array_equal(g, np.asarray([0, 128, 255], np.uint8)[r])
    # (a) member order and batch
    q = unet_amd.BatchPredictor(unet_amd.Ensemble([c, a, b], [1, 1, 2]), batch=8, postprocess=False, amp=amp, batch_invariant=True)
    others = [q.masks_and_confidence(images, grey=False) + (q.probabilities(images),)]
    for batch in (1, 3):
        r = unet_amd.BatchPredictor(unet_amd.Ensemble([a, b, c], weights), batch=batch, postprocess=False, amp=amp,
                                    batch_invariant=True)
        others.append(r.masks_and_confidence(images, grey=False) + (None,))          # (one pass each: nothing is captured)
    for oc, of, op in others:
        for k in range(len(images)):
            assert oc[k].tobytes() == cls[k].tobytes() and of[k].tobytes() == conf[k].tobytes()
            assert op is None or op[k].tobytes() == prob[k].tobytes()
    # (b) the members one by one
    for k, img in enumerate(images):
        x = _prepared(img, dev)
        acc = None
        for m, w in zip((a, b, c), weights):
            acc = ops.ensemble_add(_own_logits(m, x, amp), w, acc)
        want = ops.ensemble_finish(acc, sum(weights), probs=True, confidence=True)
        np.testing.assert_array_equal(cls[k], want.classes[0].cpu().numpy(), err_msg=str(k))
        assert prob[k].tobytes() == want.probs[0].permute(2, 0, 1).contiguous().cpu().numpy().tobytes()
        np.testing.assert_array_equal(conf[k], want.confidence[0].cpu().numpy())


@pytest.mark.parametrize("amp", [True, False])
def test_an_ensemble_of_one_is_the_bare_model(amp):
    import unet_amd
    dev = _dev()
    a = _trio(dev)[0]
    images = [_image(30 + k, H, W) for k in range(2) for H, W in SIZES]
    bare = unet_amd.BatchPredictor(a, batch=8, postprocess=False, amp=amp, batch_invariant=True)
    solo = unet_amd.BatchPredictor(unet_amd.Ensemble([a]), batch=8, postprocess=False, amp=amp, batch_invariant=True)
    assert solo.ensemble is None and solo.model is a
    want = [unet_amd.predict_img(a, im, dev) for im in images] if amp else None
    for x, y in zip(bare.classes(images), solo.classes(images)):
        assert x.tobytes() == y.tobytes()
    if want is not None:                                                              # today's path: predict_img's argmax of the logits
        for x, w in zip(bare.classes(images), want):
            np.testing.assert_array_equal(x, w.astype(np.uint8))
    with pytest.raises(RuntimeError, match="ensemble"):
        solo.confidence(images)
    with pytest.raises(RuntimeError, match="tta"):
        solo.probabilities(images)


@pytest.mark.parametrize("amp", [True, False])
def test_predictor_under_tta_and_tiling_adds_the_members_own_sums(amp):
    import unet_amd
    from unet_amd import ops
    dev = _dev()
    members, weights = _trio(dev), [1, 2, 1]
    H, W = 64, 48
    images = [_image(40 + k, H, W) for k in range(2)]
    ens = unet_amd.Ensemble(members, weights)
    # tta = "flips": the members' view sums
    p = unet_amd.BatchPredictor(ens, batch=8, postprocess=False, amp=amp, batch_invariant=True, tta="flips")
    cls, prob = p.classes(images), p.probabilities(images)
    for k, img in enumerate(images):
        x = _prepared(img, dev)
        v0, _ = ops.tta_views(x, "flips")
        acc = None
        for m, w in zip(members, weights):
            l0 = torch.cat([_own_logits(m, v0[i:i + 1], amp) for i in range(4)])
            acc = ops.ensemble_add(ops.tta_merge(l0, None, "flips", (H, W), sums=True).sums, w, acc)
        want = ops.ensemble_finish(acc, sum(weights), views=4, probs=True)
        np.testing.assert_array_equal(cls[k], want.classes[0].cpu().numpy(), err_msg=f"tta {k}")
        assert prob[k].tobytes() == want.probs[0].permute(2, 0, 1).contiguous().cpu().numpy().tobytes()
    # tile = "32,overlap=8": the members' tile sums and the shared den
    cfg = "32,overlap=8"
    t = unet_amd.BatchPredictor(ens, batch=8, postprocess=False, amp=amp, batch_invariant=True, tile=cfg)
    cls, conf = t.classes(images), t.confidence(images)
    swapped = unet_amd.BatchPredictor(unet_amd.Ensemble(members[::-1], weights[::-1]), batch=3, postprocess=False, amp=amp,
                                      batch_invariant=True, tile=cfg)
    for k, img in enumerate(images):
        tiles = ops.tile_gather(_prepared(img, dev), cfg)
        acc = den = None
        for m, w in zip(members, weights):
            logits = torch.cat([_own_logits(m, tiles[i:i + 1], amp) for i in range(tiles.shape[0])])
            merged = ops.tile_merge(logits, cfg, (H, W), sums=True)
            den = merged.den
            acc = ops.ensemble_add(merged.sums, w, acc)
        want = ops.ensemble_finish(acc, sum(weights), den=den, confidence=True)
        np.testing.assert_array_equal(cls[k], want.classes[0].cpu().numpy(), err_msg=f"tile {k}")
        np.testing.assert_array_equal(conf[k], want.confidence[0].cpu().numpy())
    for x, y in zip(cls, swapped.classes(images)):
        assert x.tobytes() == y.tobytes()
    # both: the sums of the views feed the tile merge
    both = unet_amd.BatchPredictor(ens, batch=8, postprocess=False, amp=amp, batch_invariant=True, tile=cfg, tta="flips")
    cls = both.classes(images)
    tiles = ops.tile_gather(_prepared(images[0], dev), cfg)
    acc = den = None
    for m, w in zip(members, weights):
        sums = []
        for i in range(tiles.shape[0]):
            v0, _ = ops.tta_views(tiles[i:i + 1], "flips")
            l0 = torch.cat([_own_logits(m, v0[j:j + 1], amp) for j in range(4)])
            sums.append(ops.tta_merge(l0, None, "flips", (32, 32), sums=True).sums)
        merged = ops.tile_merge(torch.cat(sums), cfg, (H, W), 4, sums=True)
        den = merged.den
        acc = ops.ensemble_add(merged.sums, w, acc)
    np.testing.assert_array_equal(cls[0], ops.ensemble_finish(acc, sum(weights), views=4, den=den).classes[0].cpu().numpy())


def test_mixed_architectures_share_an_ensemble():
    import unet_amd
    dev = _dev()
    t = _model("UNet_T", 3, True, dev, seed=5)
    s = _model("UNet_S", 3, False, dev, seed=7)
    images = [_image(50 + k, H, W) for k in range(2) for H, W in SIZES]
    p = unet_amd.BatchPredictor(unet_amd.Ensemble([t, s], [2, 1]), batch=8, postprocess=False, batch_invariant=True)
    q = unet_amd.BatchPredictor(unet_amd.Ensemble([s, t], [1, 2]), batch=3, postprocess=False, batch_invariant=True)
    assert len(p._members) == 2 and p._members[0].planner is not p._members[1].planner
    for x, y in zip(p.classes(images), q.classes(images)):
        assert x.tobytes() == y.tobytes()
    for x, y in zip(p.confidence(images), q.confidence(images)):
        assert x.tobytes() == y.tobytes()
    assert any(len(np.unique(r)) > 1 for r in p.classes(images))
    again = p.classes(images)                                                        # full batches seen before: graphs replay
    for x, y in zip(again, q.classes(images)):
        assert x.tobytes() == y.tobytes()
    with pytest.raises(ValueError, match="head"):
        unet_amd.Ensemble([t, _model("UNet_T", 1, True, dev)])


# ------------------------------------------------------------------ 6. evaluate
@pytest.mark.parametrize("classes", [3, 1])
def test_evaluate_scores_the_ensembles_masks_in_any_member_order(classes, tmp_path):
    import unet_amd
    from PIL import Image
    from unet_amd import ops
    dev = _dev()
    a, b, c = _trio(dev, classes)
    loader = _loader()
    res = [tuple(float(v) for v in unet_amd.evaluate(unet_amd.Ensemble(ms, ws), loader, dev, True, postprocess=False))
           for ms, ws in (([a, b, c], [1, 2, 1]), ([c, a, b], [1, 1, 2]), ([b, c, a], [2, 1, 1]))]
    assert res[0] == res[1] == res[2], res
    assert 0.0 < res[0][0] < 1.0, "a degenerate prediction compares nothing"
    assert all(m.training for m in (a, b, c))                                         # evaluate leaves the members in train mode
    for m in (a, b, c):
        m.eval()
    # the masks it scores: the finish over the members' own logits, read back from the dump
    dump = tmp_path / "pred"
    got = unet_amd.evaluate(unet_amd.Ensemble([a, b, c], [1, 2, 1]), loader, dev, True, epoch_pred_dir=str(dump), postprocess=False)
    assert tuple(float(v) for v in got) == res[0]
    for m in (a, b, c):
        m.eval()
    lut =np.asarray([0, 255], np.uint8) if classes == 1 else np.asarray([0, 128, 255], np.uint8)
    dice = 0.0
    for k, batch in enumerate(loader, 1):
        x = batch["image"].to(device=dev, dtype=torch.float32, memory_format=torch.channels_last)
        acc = None
        for m, w in zip((a, b, c), (1, 2, 1)):
            acc = ops.ensemble_add(_own_logits(m, x, True), w, acc)
        want = ops.ensemble_finish(acc, 4).classes
        for i in range(x.shape[0]):
            np.testing.assert_array_equal(np.asarray(Image.open(dump / f"pred_batch{k}_sample{i}.png")), lut[want[i].cpu().numpy()])
        true = batch["mask"].to(dev)
        if classes == 1:
            dice += float(unet_amd.dice_coeff(want.float(), torch.div(true, 2, rounding_mode="floor").float(), reduce_batch_first=False))
        else:
            dice += float(unet_amd.dice_coeff((want == 2).float(), (true == 2).float(), reduce_batch_first=False))
    assert abs(dice / len(loader) - res[0][0]) <= 1e-6
    for m in (a, b, c):
        m.eval()
    # tta and tiling go through the same helper
    t0 = unet_amd.evaluate(unet_amd.Ensemble([a, b, c]), loader, dev, True, postprocess=False, tta="flips", tile="32,overlap=8")
    t1 = unet_amd.evaluate(unet_amd.Ensemble([c, b, a]), loader, dev, True, postprocess=True, tta="flips", tile="32,overlap=8")
    assert float(t0[0]) == float(t1[0])
    one = unet_amd.evaluate(unet_amd.Ensemble([a]), loader, dev, True, postprocess=False)
    bare = unet_amd.evaluate(a, loader, dev, True, postprocess=False)
    assert tuple(float(v) for v in one) == tuple(float(v) for v in bare)
    for m in (a, b, c):
        m.eval()


# ------------------------------------------------------------------ 7. the command lines
def _run_cli(module, args, cwd):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, "-m", module] + args, capture_output=True, text=True, timeout=300, cwd=str(cwd), env=env)


def test_predict_cli_writes_masks_and_confidence(tmp_path):
    import unet_amd
    from PIL import Image
    dev = _dev()
    a, b, _ = _trio(dev)
    pa = unet_amd.save_checkpoint(a.cpu(), str(tmp_path / "a.pth"), mask_values=[0, 128, 255])
    pb = unet_amd.save_checkpoint(b.cpu(), str(tmp_path / "b.pth"), mask_values=[0, 128, 255])
    a.to(dev), b.to(dev)
    src = tmp_path / "in"
    src.mkdir()
    files = {"a.png": (40, 48), "b.png": (33, 31), "c.png": (40, 48)}
    images = {}
    for k, (name, (H, W)) in enumerate(files.items()):
        images[name] = _image(60 + k, H, W)
        Image.fromarray(images[name]).save(src / name)
    out, conf = tmp_path / "out", tmp_path / "conf"
    r = _run_cli("unet_amd.predict", ["-m", pa, pb + ",w=2", "--arch", "UNet_T", "-i", str(src), "-o", str(out), "--no-postprocess",
                                      "--confidence-dir", str(conf)], tmp_path)
    assert r.returncode == 0, r.stderr[-4000:]
    p = unet_amd.BatchPredictor(unet_amd.Ensemble([a, b], [1, 2]), postprocess=False, batch_invariant=True)
    want, want_conf = p.masks_and_confidence([images[n] for n in files])
    assert sorted(os.listdir(out)) == sorted(files)
    assert sorted(os.listdir(conf)) == sorted(n[:-4] + "_conf.png" for n in files)
    for n, w, c in zip(files, want, want_conf):
        np.testing.assert_array_equal(np.asarray(Image.open(out / n)), w, err_msg=n)
        np.testing.assert_array_equal(np.asarray(Image.open(conf / (n[:-4] + "_conf.png"))), c, err_msg=n)
    assert any(len(np.unique(w)) > 1 for w in want) and any(len(np.unique(c)) > 1 for c in want_conf)


def test_evaluate_cli_lists_the_members(tmp_path):
    import unet_amd
    from PIL import Image
    from unet_amd.utils.distill import teacher_sha256
    dev = _dev()
    a, b, _ = _trio(dev)
    pa = unet_amd.save_checkpoint(a.cpu(), str(tmp_path / "a.pth"), mask_values=[0, 128, 255])
    pb = unet_amd.save_checkpoint(b.cpu(), str(tmp_path / "b.pth"), mask_values=[0, 128, 255])
    a.to(dev), b.to(dev)
    for sub in ("imgs/val", "masks/val"):
        os.makedirs(tmp_path / "data" / sub)
    grey = np.array([0, 128, 255], np.uint8)
    for k, batch in enumerate(_loader(n=2, H=48, W=48)):                              # square: the loader's quarter turns keep the size
        for i in range(2):
            Image.fromarray((batch["image"][i, 0].numpy() * 255).astype(np.uint8)).save(tmp_path / "data" / "imgs" / "val" / f"s{k}{i}.png")
            Image.fromarray(grey[batch["mask"][i].numpy()]).save(tmp_path / "data" / "masks" / "val" / f"s{k}{i}_mask.png")
    js = tmp_path / "r.json"
    r = _run_cli("unet_amd.evaluate", ["-m", pa, pb + ",w=2", "--arch", "UNet_T", "--data-root", str(tmp_path / "data"), "-b", "2",
                                       "-s", "1", "--no-metrics", "--json", str(js)], tmp_path)
    assert r.returncode == 0, r.stderr[-4000:]
    rep = json.loads(js.read_text())
    assert rep["members"] == [{"path": pa, "arch": "UNet_T", "weight": 1, "sha256": teacher_sha256(pa)},
                              {"path": pb, "arch": "UNet_T", "weight": 2, "sha256": teacher_sha256(pb)}]
    assert 0.0 <= rep["dice"]["mean"] <= 1.0
