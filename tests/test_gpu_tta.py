"""Test-time augmentation on the MI355X (DESIGN.md section 3 "Test-time augmentation"): uh_tta_views and uh_tta_merge against the
numpy restatement tests/tta_ref.py, the exact equivariance of BatchPredictor(tta=...) and evaluate(tta=...) under every pose of
a mode, and the command line.  Only the comparison with float64 (test 3) has a tolerance."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tta_ref as R  # noqa: E402
from conftest import randomize_bn_  # noqa: E402

pytestmark = pytest.mark.gpu
MODES = ("hflip", "flips", "rot4", "d4")
SHAPES = [(1, 1), (1, 33), (33, 1), (31, 32), (37, 50), (64, 64), (70, 33)]          # (H, W): edges of the 32- and 16-pixel tiles
Q = 1 << 24


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _nchw(a, dev, dtype=None):
    """numpy NHWC -> the logical NCHW tensor over NHWC memory that the network's head returns."""
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    if dtype is not None:
        t = t.to(dtype)
    return t.permute(0, 3, 1, 2)


# ------------------------------------------------------------------ 1. views are exact
@pytest.mark.parametrize("H,W", SHAPES)
def test_views_are_exact(H, W):
    from unet_amd import ops
    dev = _dev()
    rng = np.random.default_rng(H * 100 + W)
    for B in (1, 3):
        for C in (1, 3):
            x = rng.standard_normal((B, H, W, C)).astype(np.float32)
            for layout in ("nhwc", "nchw"):
                t = _nchw(x, dev) if layout == "nhwc" else torch.from_numpy(np.ascontiguousarray(x.transpose(0, 3, 1, 2))).to(dev)
                for mode in MODES:
                    want0, want1 = R.views_ref(x, mode)
                    got0, got1 = ops.tta_views(t, mode)
                    assert tuple(got0.shape) == (want0.shape[0], C, H, W)
                    assert got0.permute(0, 2, 3, 1).is_contiguous()
                    assert got0.permute(0, 2, 3, 1).cpu().numpy().tobytes() == want0.tobytes(), (B, C, mode)
                    if want1.shape[0] == 0:
                        assert got1 is None
                    else:
                        assert tuple(got1.shape) == (want1.shape[0], C, W, H)
                        assert got1.permute(0, 2, 3, 1).cpu().numpy().tobytes() == want1.tobytes(), (B, C, mode)
                        if H == W:
                            joint = ops.tta_joint_views(got0, got1)
                            assert torch.equal(joint, torch.cat([got0, got1]))


# ------------------------------------------------------------------ 2. / 3. the merge
def _logits(rng, mode, B, H, W, NC, dtype):
    """Seeded N(0, 2^2) logits of every view, as the exact float values of `dtype`: (numpy float32 pair, torch pair)."""
    views = R.mode_views(mode)
    k0, k1 = sum(v < 4 for v in views), sum(v >= 4 for v in views)
    out = []
    for n, h, w in ((k0 * B, H, W), (k1 * B, W, H)):
        if n == 0:
            out.append((None, None))
            continue
        t = torch.from_numpy((2.0 * rng.standard_normal((n, h, w, NC))).astype(np.float32)).to(dtype)
        out.append((t.float().numpy(), t))
    return out


def _classes_from_sums(sums, V):
    if sums.shape[-1] == 1:
        return (sums[..., 0] > V * (Q >> 1)).astype(np.uint8)
    return sums.argmax(-1).astype(np.uint8)                             # numpy: the first maximum


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("H,W", SHAPES)
def test_merge_integer_part(H, W, dtype):
    """classes = first maximum of the kernel's own sums, probs = sums / (V 2^24), both exactly; every pixel sums to about V 2^24."""
    from unet_amd import ops
    dev = _dev()
    rng = np.random.default_rng(H * 100 + W)
    for B in (1, 3):
        for NC in (1, 2, 3, 4, 7):
            for mode in MODES:
                V = len(R.mode_views(mode))
                (_, l0), (_, l1) = _logits(rng, mode, B, H, W, NC, dtype)
                m = ops.tta_merge(l0.to(dev).permute(0, 3, 1, 2), None if l1 is None else l1.to(dev).permute(0, 3, 1, 2), mode,
                                  (H, W), sums=True, probs=True)
                sums = m.sums.cpu().numpy().astype(np.int64)
                assert sums.shape == (B, H, W, NC) and m.classes.shape == (B, H, W) and m.classes.dtype == torch.uint8
                assert sums.min() >= 0 and sums.max() <= V * Q
                if NC > 1:
                    # per view: NC roundings of q and of the quotient (half a unit each), NC - 1 roundings of the denominator
                    assert np.abs(sums.sum(-1) - V * Q).max() <= V * 2 * NC
                np.testing.assert_array_equal(m.classes.cpu().numpy(), _classes_from_sums(sums, V), err_msg=f"{B} {NC} {mode}")
                want_p = (sums.astype(np.float64) / (V * Q)).astype(np.float32)
                assert m.probs.cpu().numpy().tobytes() == want_p.tobytes(), (B, NC, mode)
                only = ops.tta_merge(l0.to(dev).permute(0, 3, 1, 2), None if l1 is None else l1.to(dev).permute(0, 3, 1, 2),
                                     mode, (H, W))
                assert only.sums is None and only.probs is None and torch.equal(only.classes, m.classes)


def test_merge_takes_square_views_as_one_batch():
    from unet_amd import ops
    dev = _dev()
    rng = np.random.default_rng(0)
    for mode in ("rot4", "d4"):
        (_, l0), (_, l1) = _logits(rng, mode, 2, 33, 33, 3, torch.bfloat16)
        a, b = l0.to(dev).permute(0, 3, 1, 2), l1.to(dev).permute(0, 3, 1, 2)
        two = ops.tta_merge(a, b, mode, (33, 33), sums=True)
        one = ops.tta_merge(torch.cat([a, b]), None, mode, (33, 33), sums=True)
        assert torch.equal(two.sums, one.sums) and torch.equal(two.classes, one.classes)
    with pytest.raises(RuntimeError):
        ops.tta_merge(a[:6], None, "d4", (33, 33))                      # six entries are not the eight views of whole images


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("NC", [1, 2, 3, 4, 7])
def test_merge_against_float64(NC, dtype):
    """|sums - S64| <= V (1 + 2 E), E = the error of torch's own fp32 softmax on these logits, in units of 2^-24 (measured here
    on the device): 1 covers the rounding of q, half a unit per view, with slack for the rounding of S64; 2 E because two correct
    fp32 softmaxes may err in opposite directions.  The classes equal the float64 argmax wherever the float64 top-two gap exceeds
    twice that; at most 0.1 % of the pixels may be left out.
    Measured (MI355X, over NC and both dtypes): E 1.43 - 2.94, largest |sums - S64| 5.04 - 6.13 (bound at V = 8, E = 1.43: 30.9),
    at most 16 of 74520 pixels left out; the table is in DESIGN.md section 3."""
    from unet_amd import ops
    dev = _dev()
    rng = np.random.default_rng(NC)
    B = 2
    worst_E = worst_dev = 0.0
    pixels = left_out = 0
    for H, W in SHAPES:
        for mode in MODES:
            V = len(R.mode_views(mode))
            (n0, l0), (n1, l1) = _logits(rng, mode, B, H, W, NC, dtype)
            E = 0.0
            for n, l in ((n0, l0), (n1, l1)):
                if l is None:
                    continue
                lf = l.to(dev).float()
                p32 = torch.sigmoid(lf) if NC == 1 else torch.softmax(lf, -1)
                E = max(E, float(np.abs(p32.cpu().numpy().astype(np.float64) * Q - R.probabilities64(n) * Q).max()))
            S64 = R.merge_ref(n0, n1, mode, (H, W))
            m = ops.tta_merge(l0.to(dev).permute(0, 3, 1, 2), None if l1 is None else l1.to(dev).permute(0, 3, 1, 2), mode, (H, W),
                              sums=True)
            sums = m.sums.cpu().numpy().astype(np.float64)
            deviation = float(np.abs(sums - S64).max())
            worst_E, worst_dev = max(worst_E, E), max(worst_dev, deviation)
            bound = V * (1 + 2 * E)
            assert deviation <= bound, (H, W, mode, deviation, bound, E)
            if NC == 1:
                gap = np.abs(S64[..., 0] - V * (Q >> 1))
                want = (S64[..., 0] > V * (Q >> 1)).astype(np.uint8)
            else:
                top = np.sort(S64, axis=-1)
                gap = top[..., -1] - top[..., -2]
                want = S64.argmax(-1).astype(np.uint8)
            decided = gap > 2 * bound
            got = m.classes.cpu().numpy()
            assert np.array_equal(got[decided], want[decided]), (H, W, mode)
            pixels += decided.size
            left_out += int((~decided).sum())
    print(f"tta merge vs float64, NC={NC} {dtype}: E = {worst_E:.3f}, largest |sums - S64| = {worst_dev:.3f} (units of 2^-24); "
          f"{left_out} of {pixels} pixels left out")
    assert left_out <= 0.001 * pixels


# ------------------------------------------------------------------ 4. exact equivariance, end to end
def _image(seed, H, W):
    """A seeded uint8 image with structure at several scales (so that the classes of a random network vary)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    img = 90 + 70 * np.sin(yy / 5.0 + seed) * np.cos(xx / 7.0) + 40 * ((yy - H / 3) ** 2 + (xx - W / 2) ** 2 < (min(H, W) / 3) ** 2)
    return np.clip(img + rng.normal(0, 12, (H, W)), 2, 255).astype(np.uint8)


def _model(arch, classes, bilinear, dev, seed=3):
    import unet_amd
    torch.manual_seed(seed)
    model = getattr(unet_amd, arch)(1, classes, bilinear)
    randomize_bn_(model, seed + 1)
    model = model.to(dev).eval()
    x = torch.from_numpy(_image(0, 48, 40).astype(np.float32) / 255.0)[None, None].to(dev)
    with torch.no_grad():                                               # the classes compete: a constant map compares nothing
        y = model(x).float()
        centre = y.mean(dim=(0, 2, 3)) if classes > 1 else (y.amax(dim=(0, 2, 3)) + y.amin(dim=(0, 2, 3))) / 2
        model.outc.conv.bias.sub_(centre)
    return model


def _check_equivariance(p, x, mode):
    poses = [R.view_ref(x, h) for h in R.mode_views(mode)]
    cls = p.classes([x] + poses)
    prob = p.probabilities([x] + poses)
    assert cls[0].shape == x.shape and prob[0].dtype == np.float32 and prob[0].shape[1:] == x.shape
    for h, c, q in zip(R.mode_views(mode), cls[1:], prob[1:]):
        np.testing.assert_array_equal(c, R.view_ref(cls[0], h), err_msg=f"classes, pose {h}")
        want = R.view_ref(prob[0].transpose(1, 2, 0), h).transpose(2, 0, 1)
        assert q.shape == want.shape and q.tobytes() == np.ascontiguousarray(want).tobytes(), f"probabilities, pose {h}"
    V = len(R.mode_views(mode))
    assert np.array_equal(prob[0] * (V * Q), np.round(prob[0] * (V * Q)))                 # multiples of 2^-24 / V
    return cls[0]


EQUIVARIANCE = [(arch, bil, H, W, mode)
                for arch, bil, sizes in (("UNet_T", True, ((48, 40), (37, 50))), ("UNet_T", False, ((48, 40), (37, 50))),
                                         ("UNet_SA", True, ((48, 40),)))
                for H, W in sizes for mode in (("d4", "rot4", "flips") if (H, W) == (37, 50) else ("d4", "rot4"))]


@pytest.mark.parametrize("batch_invariant", [True, False])
@pytest.mark.parametrize("amp", [True, False])
@pytest.mark.parametrize("arch,bilinear,H,W,mode", EQUIVARIANCE)
def test_prediction_of_a_posed_image_is_the_posed_prediction(arch, bilinear, H, W, mode, amp, batch_invariant):
    import unet_amd
    dev = _dev()
    model = _model(arch, 3, bilinear, dev)
    p = unet_amd.BatchPredictor(model, batch=8, postprocess=False, amp=amp, batch_invariant=batch_invariant, tta=mode)
    cls = _check_equivariance(p, _image(1, H, W), mode)
    assert len(np.unique(cls)) > 1, "a constant prediction compares nothing"
    grey = p([_image(1, H, W)])[0]
    np.testing.assert_array_equal(grey, np.asarray([0, 128, 255], np.uint8)[cls])


def test_mixed_sizes_share_a_call():
    """[x, h1 x, another size, h2 x] with batch 8: the grouping and the two-shape path together."""
    import unet_amd
    dev = _dev()
    model = _model("UNet_T", 3, True, dev)
    p = unet_amd.BatchPredictor(model, batch=8, postprocess=False, tta="d4")
    x, other = _image(2, 37, 50), _image(3, 48, 48)
    cls = p.classes([x, R.view_ref(x, 5), other, R.view_ref(x, 2), R.view_ref(other, 6), x, x])
    np.testing.assert_array_equal(cls[1], R.view_ref(cls[0], 5))
    np.testing.assert_array_equal(cls[3], R.view_ref(cls[0], 2))
    np.testing.assert_array_equal(cls[4], R.view_ref(cls[2], 6))
    np.testing.assert_array_equal(cls[5], cls[0])
    np.testing.assert_array_equal(cls[6], cls[0])
    alone = unet_amd.BatchPredictor(model, batch=1, postprocess=False, tta="d4")          # eight launches of one view
    np.testing.assert_array_equal(alone.classes([x])[0], cls[0])
    np.testing.assert_array_equal(alone.classes([other])[0], cls[2])
    with pytest.raises(RuntimeError, match="tta"):
        unet_amd.BatchPredictor(model, postprocess=False).probabilities([x])
    with pytest.raises(ValueError):
        unet_amd.BatchPredictor(model, tta="rot8")


# ------------------------------------------------------------------ 5. no hidden coupling
@pytest.mark.parametrize("amp", [True, False])
def test_predictor_equals_views_run_one_by_one(amp):
    import unet_amd
    from unet_amd import ops
    dev = _dev()
    model = _model("UNet_T", 3, False, dev)
    H, W = 37, 50
    img = _image(4, H, W)
    x = (img.astype(np.float32) / np.float32(255.0))[None, :, :, None]                    # what uh_predict_prepare_u8 makes of it
    views0, views1 = R.views_ref(x, "d4")
    logits = []
    for views in (views0, views1):
        outs = []
        for k in range(views.shape[0]):                                                   # every view in a launch of its own
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp), ops.plan_images(1):
                outs.append(model(_nchw(views[k:k + 1], dev)).clone())
        logits.append(torch.cat(outs))
    merged = ops.tta_merge(logits[0], logits[1], "d4", (H, W), probs=True)
    p = unet_amd.BatchPredictor(model, postprocess=False, amp=amp, tta="d4")
    np.testing.assert_array_equal(p.classes([img])[0], merged.classes[0].cpu().numpy())
    assert p.probabilities([img])[0].tobytes() == merged.probs[0].permute(2, 0, 1).contiguous().cpu().numpy().tobytes()
    assert len(np.unique(merged.classes.cpu().numpy())) > 1


# ------------------------------------------------------------------ 6. evaluate
def _loader(h=None, n=6, H=40, W=48):
    """3 batches x 2 images; with `h` the images and masks are both posed by that view."""
    batches = []
    for s in range(0, n, 2):
        imgs, masks = [], []
        for i in (s, s + 1):
            rng = np.random.default_rng(50 + i)
            yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
            r = ((yy - H * rng.uniform(0.4, 0.6)) / (H * rng.uniform(0.25, 0.4))) ** 2 + \
                ((xx - W * rng.uniform(0.4, 0.6)) / (W * rng.uniform(0.25, 0.4))) ** 2
            mask = np.where(r < 0.5, 2, np.where(r < 1.0, 1, 0)).astype(np.int64)
            img = np.clip(mask / 2.0 * 0.6 + 0.2 + rng.normal(0, 0.05, (H, W)), 0, 1).astype(np.float32)
            if h is not None:
                img, mask = R.view_ref(img, h), R.view_ref(mask, h)
            imgs.append(img[None])
            masks.append(mask)
        batches.append({"image": torch.from_numpy(np.stack(imgs)), "mask": torch.from_numpy(np.stack(masks))})
    return batches


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


@pytest.mark.parametrize("classes", [3, 1])
@pytest.mark.parametrize("h", [5, 2])
def test_evaluate_scores_a_posed_set_alike(classes, h):
    import unet_amd
    dev = _dev()
    model = _model("UNet_T", classes, True, dev, seed=classes + 5)
    res = []
    for loader in (_loader(), _loader(h)):
        acc = unet_amd.ContourMetrics()
        dice = unet_amd.evaluate(model, loader, dev, True, postprocess=False, metrics=acc, tta="d4")
        res.append(([float(v) for v in dice], acc.result()["raw"]))
    (d0, m0), (d1, m1) = res
    assert np.allclose(d0, d1, rtol=0, atol=1e-6), (d0, d1)
    assert 0.0 < d0[0] < 1.0, "a degenerate prediction compares nothing"
    assert m0["n"] == m1["n"] == 6
    assert _same(m0["per_image"]["iou"], m1["per_image"]["iou"]) and _same(m0["per_image"]["hd"], m1["per_image"]["hd"])
    assert _same(m0["per_image"]["undefined"], m1["per_image"]["undefined"])
    # with post-processing and dumps the merged classes flow through the same statements
    a = unet_amd.evaluate(model, _loader(), dev, True, postprocess=True, tta="d4")
    assert abs(float(a[0]) - d0[0]) <= 1e-6


def test_evaluate_scores_the_merged_classes():
    """A head bias that puts class 2 on top everywhere: evaluate(tta='d4') returns the Dice of the all-2 map."""
    import unet_amd
    dev = _dev()
    model = _model("UNet_T", 3, True, dev)
    with torch.no_grad():
        model.outc.conv.bias.copy_(torch.tensor([0.0, 0.0, 200.0]))
    loader = _loader()
    want = sum(float(unet_amd.dice_coeff(torch.ones(2, 40, 48, device=dev), (b["mask"].to(dev) == 2).float(),
                                         reduce_batch_first=False)) for b in loader) / 3
    got = unet_amd.evaluate(model, loader, dev, True, postprocess=False, tta="d4")
    assert abs(float(got[0]) - want) <= 1e-6 and 0.1 < want < 0.9
    with torch.no_grad():
        model.outc.conv.bias.copy_(torch.tensor([200.0, 0.0, 0.0]))
    none = unet_amd.evaluate(model, loader, dev, True, postprocess=False, tta="d4")
    assert float(none[0]) < 1e-3
    with pytest.raises(ValueError):
        unet_amd.evaluate(model, loader, dev, True, tta="rot8")


# ------------------------------------------------------------------ 7. the command line
def test_cli_writes_what_the_predictor_returns(tmp_path):
    import unet_amd
    from PIL import Image
    from test_gpu_predict_cli import _cli
    dev = _dev()
    model = _model("UNet_T", 3, False, dev)
    wpath = unet_amd.save_checkpoint(model.cpu(), str(tmp_path / "w.pth"), mask_values=[0, 128, 255])
    model = model.to(dev)
    src = tmp_path / "in"
    src.mkdir()
    files = {"a.png": (48, 40), "b.png": (37, 50), "c.png": (48, 40)}
    images = {}
    for k, (name, (H, W)) in enumerate(files.items()):
        images[name] = _image(10 + k, H, W)
        Image.fromarray(images[name]).save(src / name)
    out = tmp_path / "out"
    r = _cli(["-m", wpath, "--arch", "UNet_T", "-i", str(src), "-o", str(out), "--no-postprocess", "--tta", "d4"], tmp_path)
    assert r.returncode == 0, r.stderr[-4000:]
    p = unet_amd.BatchPredictor(model, postprocess=False, batch_invariant=True, tta="d4")
    want = p([images[n] for n in files])
    assert sorted(os.listdir(out)) == sorted(files)
    for n, w in zip(files, want):
        np.testing.assert_array_equal(np.asarray(Image.open(out / n)), w, err_msg=n)
    assert any(len(np.unique(w)) > 1 for w in want)
    bad = _cli(["-m", wpath, "-i", str(src), "--tta", "rot8"], tmp_path)
    assert bad.returncode == 2
