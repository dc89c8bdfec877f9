"""Contour metrics on the MI355X (csrc/contour_metrics.hip) against the scipy / numpy restatement tests/contour_metrics_ref.py:
the border and the exact squared distance transform as integer arrays, the record of uh_contour_metrics field by field,
determinism and batch invariance, evaluate(metrics=...) against the PNG dumps of the same run, and the two command lines.

Bounds.  Integer fields and HD are compared for equality (HD = sqrt of the same integer in fp64, correctly rounded on both
sides).  HD95 and ASSD: relative 1e-12 -- both sides work in fp64 from identical integers, the finish is a handful of
correctly rounded operations plus a sum of n <= a few thousand terms (n * 2^-53 ~ 1e-12 in the worst ordering, far less in
practice), and linear interpolation is continuous in the index, so a one-ulp difference in 0.95 (n - 1) moves the value by
no more than that."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import contour_metrics_ref as R
from conftest import ROOT

pytestmark = pytest.mark.gpu

SIZES = [(512, 512), (300, 700), (700, 300), (100, 37), (1000, 999), (1, 1), (1, 513), (513, 1)]
REL = 1e-12


def _kinds(rng, H, W):
    single = np.zeros((H, W), bool)
    single[int(rng.integers(0, H)), int(rng.integers(0, W))] = True
    yy, xx = np.indices((H, W))
    return {"blob": R.blob_mask(rng, H, W), "single": single, "full": np.ones((H, W), bool),
            "checkerboard": (yy + xx) % 2 == 0, "empty": np.zeros((H, W), bool)}


def _batches(H, W, seed):
    """B = 1: every kind of mask alone; B = 8: all of them in one batch, the empty image among non-empty ones."""
    rng = np.random.default_rng(seed)
    k = _kinds(rng, H, W)
    for name, m in k.items():
        yield name, m[None]
    yield "batch8", np.stack([k["blob"], k["single"], k["full"], k["checkerboard"], k["empty"]] +
                             [R.blob_mask(rng, H, W) for _ in range(3)])


def _class_map(rng, masks, cls=2):
    """uint8 class maps whose class `cls` is `masks`; the rest is a mix of the other values."""
    other = rng.choice(np.array([v for v in (0, 1, 3) if v != cls], np.uint8), masks.shape)
    return np.where(masks, np.uint8(cls), other)


@pytest.mark.parametrize("H,W", SIZES)
def test_border_and_edt_equal_the_restatement(H, W):
    from unet_amd import ops
    rng = np.random.default_rng(H * 7 + W)
    for name, masks in _batches(H, W, seed=H + 3 * W):
        cm = torch.from_numpy(_class_map(rng, masks)).cuda()
        got_b = ops.mask_border(cm, 2).cpu().numpy()
        want_b = np.stack([R.border(m) for m in masks])
        assert got_b.dtype == np.uint8 and np.array_equal(got_b, want_b.astype(np.uint8)), (name, H, W)
        # the transform of the border (what the metric uses) and of the mask itself (dense features: the checkerboard)
        for feat in (want_b, masks):
            f = torch.from_numpy(feat.astype(np.uint8) * 255).cuda()
            got = ops.edt_sq(f).cpu().numpy()
            want = np.stack([R.edt_sq(m) for m in feat])
            assert got.dtype == np.int64 and np.array_equal(got, want), (name, H, W, np.abs(got - want).max())


def _pairs(H, W, B, seed):
    rng = np.random.default_rng(seed)
    P = np.stack([R.blob_mask(rng, H, W) for _ in range(B)])
    T = np.stack([R.blob_mask(rng, H, W) for _ in range(B)])
    return P, T


def _records(P, T, cls_pred=2, cls_true=2):
    from unet_amd import ops
    from unet_amd.utils.contour_metrics import decode_records
    rng = np.random.default_rng(5)
    rec = ops.contour_metrics(torch.from_numpy(_class_map(rng, P, cls_pred)).cuda(),
                              torch.from_numpy(_class_map(rng, T, cls_true)).cuda(), cls_pred, cls_true)
    assert rec.dtype == torch.float64 and rec.shape == (P.shape[0], 12)
    return rec, {k: v.cpu().numpy() for k, v in decode_records(rec).items()}


INT_KEYS = ("n_pred", "n_true", "n_inter", "n_union", "n_border_pred", "n_border_true", "n", "max_d2", "undefined")


def _check_image(got, i, want, P, T):
    for k in INT_KEYS:
        assert int(got[k][i]) == want[k], (k, i, int(got[k][i]), want[k])
    if want["undefined"]:
        assert all(math.isnan(got[k][i]) for k in ("hd", "hd95", "assd")) and got["iou"][i] == 0.0
        return
    assert got["hd"][i] == np.sqrt(np.float64(want["max_d2"])) == want["hd"], (i, got["hd"][i], want["hd"])
    assert got["iou"][i] == want["iou"]
    for k in ("hd95", "assd"):
        print(f"image {i} {k}: device {got[k][i]!r} numpy {want[k]!r} rel {abs(got[k][i] - want[k]) / max(want[k], 1e-300):.3e}")
        assert abs(got[k][i] - want[k]) <= REL * abs(want[k]), (k, i, got[k][i], want[k])
    if want["n"]:
        d2 = np.sort(R.distances_sq(P, T))
        assert abs(got["sum_dist"][i] - np.sqrt(d2.astype(np.float64)).sum()) <= REL * got["sum_dist"][i]
        assert d2[0] <= got["d2_lo"][i] <= got["d2_hi"][i] <= d2[-1] and 0.0 <= got["weight"][i] < 1.0
        a, b, g = math.sqrt(got["d2_lo"][i]), math.sqrt(got["d2_hi"][i]), got["weight"][i]
        assert abs((a + (b - a) * g) - want["hd95"]) <= 2 * REL * want["hd95"]


@pytest.mark.parametrize("H,W", [(512, 512), (300, 700), (100, 37), (1000, 999)])
def test_records_equal_the_restatement(H, W):
    P, T = _pairs(H, W, 8, seed=H + W)
    want = [R.image_metrics(p, t) for p, t in zip(P, T)]
    assert not any(m["undefined"] for m in want) and all(m["n"] > 0 for m in want)    # the condition of the random set
    _, got = _records(P, T)
    for i, m in enumerate(want):
        _check_image(got, i, m, P[i], T[i])


def test_hand_made_cases_every_field():
    H, W = 64, 48
    E = np.zeros((H, W), bool)
    sq = np.zeros((H, W), bool)
    sq[10:30, 10:30] = True
    sh = np.zeros((H, W), bool)
    sh[13:33, 14:34] = True
    one, other = E.copy(), E.copy()
    one[3, 4], other[10, 28] = True, True
    edge = E.copy()
    edge[0:20, 0:9] = True
    P = np.stack([E, E, sq, sq, sq, one, edge, np.ones((H, W), bool)])
    T = np.stack([E, sq, E, sq, sh, other, sq, sq])
    _, got = _records(P, T, cls_pred=1, cls_true=2)
    want = [R.image_metrics(p, t) for p, t in zip(P, T)]
    assert [m["undefined"] for m in want] == [0, 1, 1, 0, 0, 0, 0, 0]
    for i, m in enumerate(want):
        _check_image(got, i, m, P[i], T[i])
    assert (got["hd"][0], got["hd95"][0], got["assd"][0], got["iou"][0], got["n"][0]) == (0.0, 0.0, 0.0, 1.0, 0)
    assert (got["hd"][3], got["hd95"][3], got["assd"][3], got["iou"][3]) == (0.0, 0.0, 0.0, 1.0)
    assert got["hd"][4] == 5.0 and got["hd"][5] == got["hd95"][5] == got["assd"][5] == 25.0
    from unet_amd import contour_metrics
    m = contour_metrics(torch.from_numpy(P.astype(np.int64) * 2).cuda(), torch.from_numpy(T.astype(np.int64) * 2).cuda(),
                        cls=2, spacing=0.5)
    assert m["undefined"].tolist() == [False, True, True, False, False, False, False, False]
    assert float(m["hd"][4]) == 2.5 and float(m["iou"][3]) == 1.0 and m["hd"].dtype == torch.float64


def test_deterministic_and_batch_invariant():
    P, T = _pairs(300, 700, 8, seed=9)
    P[5] = False                                                     # an undefined image inside the batch
    T[6] = False
    P[6] = False                                                     # and a both-empty one
    a, _ = _records(P, T)
    b, _ = _records(P, T)
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    for i in range(8):
        alone, _ = _records(P[i:i + 1], T[i:i + 1])
        assert torch.equal(alone.view(torch.int64)[0], a.view(torch.int64)[i]), i


# ------------------------------------------------------------------------------------------------ evaluate()
def _parent_evaluate(net, batches, device, amp, postprocess=True):
    """evaluate() as it was before the `metrics` keyword, without the PNG dumps: the loop restated."""
    from unet_amd import ops
    from unet_amd.utils.dice_score import dice_coeff
    from unet_amd.utils.post_process import postprocess_mask
    with torch.inference_mode():
        net.eval()
        n = 0
        dice_score = torch.zeros((), dtype=torch.float32, device=device)
        dice_post = torch.zeros((), dtype=torch.float32, device=device)
        min_dice = torch.full((), 10.0, dtype=torch.float32, device=device)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
            for batch in batches:
                n += 1
                image = batch["image"].to(device=device, dtype=torch.float32, memory_format=torch.channels_last)
                mask_true = batch["mask"].to(device=device, dtype=torch.float32)
                mask_pred = net(image)
                if net.n_classes == 1:
                    mask_true = torch.div(mask_true, 2, rounding_mode="floor")
                    pred = ops.threshold_mask(mask_pred.squeeze(1))
                    d = dice_coeff(pred, mask_true, reduce_batch_first=False)
                    cur = d
                    if postprocess:
                        processed = (postprocess_mask((pred * 255).to(torch.uint8)) // 255).float()
                        dp = dice_coeff(processed, mask_true, reduce_batch_first=False)
                        dice_post += dp
                        cur = torch.minimum(d, dp)
                else:
                    idx = ops.argmax_classes(mask_pred)
                    true_c = (mask_true == 2).float()
                    d = dice_coeff((idx == 2).float(), true_c, reduce_batch_first=False)
                    cur = d
                    if postprocess:
                        processed = postprocess_mask(idx.to(torch.uint8))
                        dice_post += dice_coeff((processed == 2).float(), true_c, reduce_batch_first=False)
                dice_score += d
                min_dice = torch.minimum(min_dice, cur.float())
        net.train()
        if not postprocess:
            dice_post = dice_score
        return dice_score / max(n, 1), dice_post / max(n, 1), min_dice


def _same_bits(a, b):
    return all(torch.equal(x.float().cpu().view(torch.int32), y.float().cpu().view(torch.int32)) for x, y in zip(a, b))


def _close_sets(got, want):
    """Set figures: a mean of non-negative per-image values that are each within REL of numpy's is within REL of numpy's mean;
    the second REL covers the rounding of the two sums, which run in different orders."""
    for k in ("hd", "hd95", "hd_max", "assd", "iou"):
        if math.isnan(want[k]):
            assert math.isnan(got[k]), k
        else:
            assert abs(got[k] - want[k]) <= 2 * REL * abs(want[k]), (k, got[k], want[k])
    assert got["n"] == want["n"] and got["n_undefined"] == want["n_undefined"]


@pytest.mark.parametrize("classes", [3, 1])
def test_evaluate_with_and_without_metrics(tmp_path, monkeypatch, classes):
    import unet_amd
    from unet_amd import ContourMetrics, ellipse_batch, ops
    dev = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(3)
    model = unet_amd.UNet_T(1, classes, bilinear=True).to(memory_format=torch.channels_last).to(dev)
    images, masks = ellipse_batch(6, 192, seed=11)
    batches = [{"image": images[i:i + 2], "mask": masks[i:i + 2]} for i in range(0, 6, 2)]
    calls = []
    real = ops.contour_metrics
    monkeypatch.setattr(ops, "contour_metrics", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    want = _parent_evaluate(model, batches, dev, True)
    off = unet_amd.evaluate(model, batches, dev, True)
    assert _same_bits(off, want) and not calls                       # metrics=None: the parent's bits, no new launch
    acc = ContourMetrics()
    on = unet_amd.evaluate(model, batches, dev, True, str(tmp_path / "pred"), metrics=acc)
    assert _same_bits(on, want) and len(on) == 3 and len(calls) == 2 * len(batches)
    res = acc.result()
    # the restatement on the masks that the same run dumped, decoded back from the PNGs
    raw, post = [], []
    fg = 255                                                          # class 2 (multi-class) / class 1 (binary) are coded 255
    for k, batch in enumerate(batches, start=1):
        for i in range(2):
            T = (batch["mask"][i].numpy() == 2) if classes > 1 else (batch["mask"][i].numpy() // 2 == 1)
            p_raw = np.asarray(Image.open(tmp_path / "pred" / f"pred_batch{k}_sample{i}.png")) == fg
            p_post = np.asarray(Image.open(tmp_path / "pred" / "postprocessed" / f"pred_batch{k}_sample{i}.png")) == fg
            raw.append(R.image_metrics(p_raw, T))
            post.append(R.image_metrics(p_post, T))
    _close_sets(res["raw"], R.set_metrics(raw))
    _close_sets(res["post"], R.set_metrics(post))
    for name, rows in (("raw", raw), ("post", post)):
        per = res[name]["per_image"]
        assert per["undefined"].tolist() == [bool(m["undefined"]) for m in rows]
        for k in ("hd", "hd95", "assd", "iou"):
            w = np.array([m[k] for m in rows])
            assert np.array_equal(np.isnan(per[k]), np.isnan(w))
            ok = ~np.isnan(w)
            assert (np.abs(per[k][ok] - w[ok]) <= REL * np.abs(w[ok])).all(), (name, k)
    calls.clear()
    no_post = ContourMetrics()
    unet_amd.evaluate(model, batches, dev, True, postprocess=False, metrics=no_post)
    assert len(calls) == len(batches) and no_post.result()["post"]["n"] == 0 and no_post.result()["raw"]["n"] == 6


# ------------------------------------------------------------------------------------------------ the command lines
def _png_tree(root, n_train, n_val, size, seed):
    from unet_amd import ellipse_batch
    imgs, masks = ellipse_batch(n_train + n_val, size, seed=seed)
    grey = np.array([0, 128, 255], np.uint8)
    for i in range(n_train + n_val):
        split = "train" if i < n_train else "val"
        for d in ("imgs", "masks"):
            os.makedirs(os.path.join(root, d, split), exist_ok=True)
        Image.fromarray((imgs[i, 0].numpy() * 255).astype(np.uint8)).save(os.path.join(root, "imgs", split, f"p{i:03d}.png"))
        Image.fromarray(grey[masks[i].numpy()]).save(os.path.join(root, "masks", split, f"p{i:03d}_mask.png"))


def _run(module, cwd, args, limit=300):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, "-m", module] + args, capture_output=True, text=True,
                       timeout=limit + 30, cwd=str(cwd), env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    return r


def test_evaluate_command_line(tmp_path):
    import unet_amd
    from unet_amd.evaluate_cli import report
    from unet_amd.utils.data_loading import BasicDataset, DeviceBatchLoader
    data = tmp_path / "data"
    _png_tree(str(data), 0, 12, 256, seed=21)
    torch.manual_seed(5)
    model = unet_amd.UNet_T(1, 3, bilinear=False)
    ckpt = str(tmp_path / "m.pth")
    unet_amd.save_checkpoint(model, ckpt, mask_values=[0, 128, 255])
    out = tmp_path / "out.json"
    args = ["-m", ckpt, "--data-root", str(data), "--arch", "UNet_T", "-b", "4", "-s", "0.5", "--workers", "4", "--spacing", "0.25"]
    r = _run("unet_amd.evaluate", tmp_path, args + ["--json", str(out)])
    assert "Validation Dice score" in r.stderr and "Validation contour metrics" in r.stderr and "HD95" in r.stderr
    got = json.loads(out.read_text())
    dev = torch.device("cuda", torch.cuda.current_device())
    model = model.to(memory_format=torch.channels_last).to(dev)
    val = BasicDataset(str(data / "imgs" / "val"), str(data / "masks" / "val"), 0.5)
    acc = unet_amd.ContourMetrics(spacing=0.25)
    dice = unet_amd.evaluate(model, DeviceBatchLoader(val, 4, shuffle=False, drop_last=True, workers=4, device=dev), dev, True,
                             metrics=acc)
    want = json.loads(json.dumps(report(tuple(float(v) for v in dice), acc.result())))
    assert got == want
    assert got["metrics"]["raw"]["n"] == 48 and len(got["metrics"]["raw"]["per_image"]["hd"]) == 48
    quiet = _run("unet_amd.evaluate", tmp_path, args + ["--no-metrics"])
    assert "Validation Dice score" in quiet.stderr and "contour metrics" not in quiet.stderr and "HD95" not in quiet.stderr


def test_train_command_line_metrics_flag(tmp_path):
    data = tmp_path / "data"
    _png_tree(str(data), 3, 2, 128, seed=7)
    args = ["-e", "1", "-b", "2", "-s", "0.5", "-c", "3", "--seed", "0", "--model", "UNet_T", "--data-root", str(data),
            "--workers", "4"]
    on = _run("unet_amd.train", tmp_path, args + ["--metrics"])
    lines = on.stderr.splitlines()
    dice_at = [i for i, ln in enumerate(lines) if "Validation Dice score" in ln]
    assert len(dice_at) == 1 and "Validation contour metrics" in lines[dice_at[0] + 1] and "HD95" in lines[dice_at[0] + 1]
    off = _run("unet_amd.train", tmp_path, args)
    assert "Validation Dice score" in off.stderr and "images/s" in off.stderr and "contour metrics" not in off.stderr
