"""Tiled prediction on the MI355X (DESIGN.md section 3 "Tiled prediction"): uh_tile_gather and uh_tile_merge against the numpy
restatement tests/tiling_ref.py, BatchPredictor(tile=...) and evaluate(tile=...) against hand compositions of the same calls,
and the one-tile case against the untiled path.  Only the comparison with float64 (test 3) has a tolerance."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tiling_ref as R  # noqa: E402
from conftest import randomize_bn_  # noqa: E402

pytestmark = pytest.mark.gpu
# (H, W, size, overlap): edge tiles; three tiles deep per axis; zero overlap; an image smaller than the tile; a clamped last tile
SHAPES = [(37, 53, 16, 4), (47, 31, 16, 8), (33, 33, 16, 0), (40, 48, 64, 16), (63, 95, 32, 16)]
CLASSES = (1, 2, 3, 4, 7)
Q = 1 << 24


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _cfg(size, overlap):
    from unet_amd.utils.tiling import TileConfig
    return TileConfig(size, overlap)


def _nchw(a, dev, dtype=None):
    """numpy NHWC -> the logical NCHW tensor over NHWC memory that the network takes and its head returns."""
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    if dtype is not None:
        t = t.to(dtype)
    return t.permute(0, 3, 1, 2)


# ------------------------------------------------------------------ 1. the gather is exact
@pytest.mark.parametrize("H,W,size,overlap", SHAPES)
def test_gather_is_exact(H, W, size, overlap):
    from unet_amd import ops
    dev = _dev()
    rng = np.random.default_rng(H * 100 + W)
    B = 2
    for C in (1, 3):
        x = rng.standard_normal((B, H, W, C)).astype(np.float32)
        want = R.gather_ref(x, size, overlap)
        for layout in ("nhwc", "nchw"):
            t = _nchw(x, dev) if layout == "nhwc" else torch.from_numpy(np.ascontiguousarray(x.transpose(0, 3, 1, 2))).to(dev)
            got = ops.tile_gather(t, _cfg(size, overlap))
            assert tuple(got.shape) == (want.shape[0], C, want.shape[1], want.shape[2])
            assert got.permute(0, 2, 3, 1).is_contiguous()
            assert got.permute(0, 2, 3, 1).cpu().numpy().tobytes() == want.tobytes(), (C, layout)
        spec = ops.tile_gather(_nchw(x, dev), f"{size},overlap={overlap}")                 # the spec string is taken too
        assert torch.equal(spec, got)
        # an image row that does not start on 16 bytes: the float-by-float read of the 16-byte kernel
        odd = ops.tile_gather(_nchw(x, dev)[1:], _cfg(size, overlap))
        assert odd.permute(0, 2, 3, 1).cpu().numpy().tobytes() == R.gather_ref(x[1:], size, overlap).tobytes()


def test_gather_of_rows_that_are_no_multiple_of_16_bytes():
    """An image narrower than the tile: tile rows of 31 and 93 floats, the float-by-float kernel."""
    from unet_amd import ops
    dev = _dev()
    rng = np.random.default_rng(7)
    for C in (1, 3):
        x = rng.standard_normal((2, 70, 31, C)).astype(np.float32)
        got = ops.tile_gather(_nchw(x, dev), _cfg(32, 8))
        assert got.permute(0, 2, 3, 1).cpu().numpy().tobytes() == R.gather_ref(x, 32, 8).tobytes(), C


# ------------------------------------------------------------------ 2. the merge of integer sums is exact
@pytest.mark.parametrize("V", [1, 8])
@pytest.mark.parametrize("H,W,size,overlap", SHAPES)
def test_merge_of_integer_sums_is_exact(H, W, size, overlap, V):
    from unet_amd import ops
    dev = _dev()
    rng = np.random.default_rng(H * 100 + W + V)
    ny, nx, th, tw, _, _ = R.grid(H, W, size, overlap)
    B = 2
    for NC in CLASSES:
        q = rng.integers(0, (1 << 27) * V, (B * ny * nx, th, tw, NC), dtype=np.int64).astype(np.int32)
        q[0, 0, 0, :] = (1 << 27) * V - 1                                                  # the largest value allowed
        want_s, want_d = R.merge_ref(q, (H, W), size, overlap)
        m = ops.tile_merge(torch.from_numpy(q).to(dev), _cfg(size, overlap), (H, W), V, sums=True, probs=True)
        assert m.sums.dtype == torch.int64 and m.den.dtype == torch.int32 and m.classes.dtype == torch.uint8
        assert m.sums.cpu().numpy().astype(np.uint64).tobytes() == want_s.tobytes(), NC
        assert m.den.cpu().numpy().astype(np.uint64).tobytes() == want_d.tobytes(), NC
        np.testing.assert_array_equal(m.classes.cpu().numpy(), R.classes_ref(want_s, want_d, V), err_msg=f"NC={NC}")
        assert m.probs.cpu().numpy().tobytes() == R.probs_ref(want_s, want_d, V).tobytes(), NC
        only = ops.tile_merge(torch.from_numpy(q).to(dev), _cfg(size, overlap), (H, W), V)
        assert only.sums is None and only.den is None and only.probs is None and torch.equal(only.classes, m.classes)
    assert int(want_d.max()) <= 9 * max(1, overlap) ** 2 and int(want_d.min()) >= 1


def test_merge_breaks_ties_like_the_argmax():
    """Equal sums: the first maximum; one class exactly at the threshold: class 0."""
    from unet_amd import ops
    dev = _dev()
    H, W, size, overlap = 37, 53, 16, 4
    ny, nx, th, tw, _, _ = R.grid(H, W, size, overlap)
    for NC in (2, 3, 4, 7):
        q = np.full((ny * nx, th, tw, NC), 5, np.int32)
        q[..., 0] = 3                                                                      # classes 1 .. NC-1 tie on top
        m = ops.tile_merge(torch.from_numpy(q).to(dev), _cfg(size, overlap), (H, W), 1)
        assert int(m.classes.min()) == int(m.classes.max()) == 1
    half = np.full((ny * nx, th, tw, 1), Q // 2, np.int32)
    assert int(ops.tile_merge(torch.from_numpy(half).to(dev), _cfg(size, overlap), (H, W), 1).classes.max()) == 0
    assert int(ops.tile_merge(torch.from_numpy(half + 1).to(dev), _cfg(size, overlap), (H, W), 1).classes.min()) == 1


# ------------------------------------------------------------------ 3. the merge of logits against float64
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("NC", CLASSES)
def test_merge_of_logits_against_float64(NC, dtype):
    """|sums - S64| <= den (1 + 2 E) per pixel, E = the error of torch's own fp32 softmax / sigmoid on these logits against
    float64, in units of 2^-24, measured here on the device: a tile's q is within 1/2 + E' of its float64 value for a correct
    fp32 softmax of error E', the weights add up to den, and two correct softmaxes may err in opposite directions (2 E; the 1
    leaves half a unit per weight for the rounding of S64 itself).  The classes equal the float64 ones wherever the float64
    top-two gap exceeds twice that bound; at most 0.5 % of the pixels of a case may be left out.
    Measured on the MI355X (over the five shapes): E 1.43 - 2.88, largest |sums - S64| / den 1.43 - 3.84 against bounds of
    3.9 - 6.8; fp32 leaves no pixel out, bf16 at most 10 of 3840 (0.26 %, NC = 7; exact ties of repeated bf16 values in singly
    covered pixels).  The table is in DESIGN.md section 3 "Tiled prediction"."""
    from unet_amd import ops
    dev = _dev()
    rng = np.random.default_rng(NC)
    B = 2
    for H, W, size, overlap in SHAPES:
        ny, nx, th, tw, _, _ = R.grid(H, W, size, overlap)
        t = torch.from_numpy((2.0 * rng.standard_normal((B * ny * nx, th, tw, NC))).astype(np.float32)).to(dtype)
        exact = t.float().numpy()                                                          # the logits' exact values
        p64 = R.probabilities64(exact)
        lf = t.to(dev).float()
        p32 = torch.sigmoid(lf) if NC == 1 else torch.softmax(lf, -1)
        E = float(np.abs(p32.cpu().numpy().astype(np.float64) * Q - p64 * Q).max())
        S64, den = R.merge_ref(p64 * Q, (H, W), size, overlap)
        m = ops.tile_merge(t.to(dev).permute(0, 3, 1, 2), _cfg(size, overlap), (H, W), sums=True)
        assert m.den.cpu().numpy().astype(np.uint64).tobytes() == den.tobytes()
        sums = m.sums.cpu().numpy().astype(np.float64)
        bound = den.astype(np.float64) * (1 + 2 * E)
        excess = np.abs(sums - S64) / bound[..., None]
        if NC == 1:
            gap = np.abs(S64[..., 0] - den.astype(np.float64) * (Q >> 1))
            want = (S64[..., 0] > den.astype(np.float64) * (Q >> 1)).astype(np.uint8)
        else:
            top = np.sort(S64, axis=-1)
            gap = top[..., -1] - top[..., -2]
            want = S64.argmax(-1).astype(np.uint8)
        decided = gap > 2 * bound
        left_out = int((~decided).sum())
        print(f"tile merge vs float64, NC={NC} {dtype} {(H, W, size, overlap)}: E = {E:.3f}, largest |sums - S64| / den = "
              f"{float((np.abs(sums - S64) / den[..., None]).max()):.3f} (units of 2^-24; bound {1 + 2 * E:.3f}); "
              f"{left_out} of {decided.size} pixels left out")
        assert float(excess.max()) <= 1.0, (H, W, size, overlap, float(excess.max()), E)
        got = m.classes.cpu().numpy()
        assert np.array_equal(got[decided], want[decided]), (H, W, size, overlap)
        assert left_out <= 0.005 * decided.size, (H, W, size, overlap, left_out, decided.size)


# ------------------------------------------------------------------ networks and images
def _image(seed, H, W):
    """A seeded uint8 image with structure at several scales (so that the classes of a random network vary)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    img = 90 + 70 * np.sin(yy / 5.0 + seed) * np.cos(xx / 7.0) + 40 * ((yy - H / 3) ** 2 + (xx - W / 2) ** 2 < (min(H, W) / 3) ** 2)
    return np.clip(img + rng.normal(0, 12, (H, W)), 2, 255).astype(np.uint8)


_MODELS = {}


def _model(arch, bilinear, dev, classes=3, seed=3):
    """Seeded random weights, non-trivial BatchNorm running statistics, a head bias that lets the classes compete."""
    key = (arch, bilinear, classes, seed)
    if key not in _MODELS:
        import unet_amd
        torch.manual_seed(seed)
        model = getattr(unet_amd, arch)(1, classes, bilinear)
        randomize_bn_(model, seed + 1)
        model = model.to(dev).eval()
        x = torch.from_numpy(_image(0, 48, 40).astype(np.float32) / 255.0)[None, None].to(dev)
        with torch.no_grad():
            y = model(x).float()
            centre = y.mean(dim=(0, 2, 3)) if classes > 1 else (y.amax(dim=(0, 2, 3)) + y.amin(dim=(0, 2, 3))) / 2
            model.outc.conv.bias.sub_(centre)
        _MODELS[key] = model
    return _MODELS[key].eval()


def _prepared(img):
    """What uh_predict_prepare_u8 makes of a uint8 image (it holds bytes > 1): float32 [1,H,W,1]."""
    return (img.astype(np.float32) / np.float32(255.0))[None, :, :, None]


def _one_by_one(model, tiles, amp, dev):
    """numpy tiles [N,th,tw,1] -> the logits of every tile from a launch of its own under the pinned plan."""
    from unet_amd import ops
    outs = []
    for k in range(tiles.shape[0]):
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp), ops.plan_images(1):
            outs.append(model(_nchw(tiles[k:k + 1], dev)).clone())
    return torch.cat(outs)


def _loader(images, masks, per_batch=2):
    return [{"image": torch.from_numpy(np.stack([_prepared(i)[0, :, :, 0][None] for i in images[s:s + per_batch]])),
             "mask": torch.from_numpy(np.stack(masks[s:s + per_batch]))} for s in range(0, len(images), per_batch)]


def _mask(seed, H, W):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    r = ((yy - H * rng.uniform(0.4, 0.6)) / (H * 0.35)) ** 2 + ((xx - W * rng.uniform(0.4, 0.6)) / (W * 0.35)) ** 2
    return np.where(r < 0.5, 2, np.where(r < 1.0, 1, 0)).astype(np.int64)


def _dump(path):
    return {os.path.relpath(os.path.join(d, f), path): open(os.path.join(d, f), "rb").read()
            for d, _, files in os.walk(path) for f in files}


# ------------------------------------------------------------------ 4. one tile means untiled
@pytest.mark.parametrize("amp", [True, False])
def test_one_tile_is_the_untiled_path(amp, tmp_path):
    import unet_amd
    dev = _dev()
    model = _model("UNet_S", False, dev)
    images = [_image(1, 40, 48), _image(2, 64, 64), _image(3, 40, 48)]
    plain = unet_amd.BatchPredictor(model, postprocess=False, amp=amp)
    tiled = unet_amd.BatchPredictor(model, postprocess=False, amp=amp, tile="64,overlap=16")
    for a, b in zip(plain(images), tiled(images)):
        np.testing.assert_array_equal(a, b)
    want = plain.classes(images)
    for a, b in zip(want, tiled.classes(images)):
        np.testing.assert_array_equal(a, b)
    assert any(len(np.unique(c)) > 1 for c in want), "a constant prediction compares nothing"
    post = unet_amd.BatchPredictor(model, postprocess=True, amp=amp, min_area=20, tile=unet_amd.TileConfig(64, 16))
    for a, b in zip(unet_amd.BatchPredictor(model, postprocess=True, amp=amp, min_area=20)(images), post(images)):
        np.testing.assert_array_equal(a, b)
    for k, (H, W) in enumerate(((40, 48), (64, 64))):
        imgs = [_image(10 + i, H, W) for i in range(4)]
        loader = _loader(imgs, [_mask(20 + i, H, W) for i in range(4)])
        a = unet_amd.evaluate(model, loader, dev, amp, str(tmp_path / f"plain{k}"), postprocess=True)
        b = unet_amd.evaluate(model, loader, dev, amp, str(tmp_path / f"tiled{k}"), postprocess=True, tile="64,overlap=16")
        assert [float(v) for v in a] == [float(v) for v in b]
        da, db = _dump(tmp_path / f"plain{k}"), _dump(tmp_path / f"tiled{k}")
        assert len(da) == 8 and da == db                                                   # raw and post-processed, 4 images


# ------------------------------------------------------------------ 5. the plumbing against a hand composition
@pytest.mark.parametrize("amp", [True, False])
@pytest.mark.parametrize("arch,bilinear", [("UNet_S", False), ("UNet_T", True)])
def test_predictor_equals_tiles_run_one_by_one(arch, bilinear, amp):
    import unet_amd
    from unet_amd import ops
    dev = _dev()
    model = _model(arch, bilinear, dev)
    cfg = _cfg(32, 8)
    images = [_image(4, 70, 90), _image(5, 47, 31)]
    want = []
    for img in images:
        tiles = R.gather_ref(_prepared(img), cfg.size, cfg.overlap)
        merged = ops.tile_merge(_one_by_one(model, tiles, amp, dev), cfg, img.shape, probs=True)
        want.append((merged.classes[0].cpu().numpy(), merged.probs[0].permute(2, 0, 1).contiguous().cpu().numpy()))
    assert len(np.unique(want[0][0])) > 1, "a constant prediction compares nothing"
    for batch_invariant in (True, False):
        for batch in (1, 3, 8):
            p = unet_amd.BatchPredictor(model, batch=batch, postprocess=False, amp=amp, batch_invariant=batch_invariant, tile=cfg)
            for calls in ([images], [[images[0]], [images[1]]]):                           # one call; each image alone
                cls = [c for call in calls for c in p.classes(call)]
                prob = [q for call in calls for q in p.probabilities(call)]
                for (wc, wp), c, q in zip(want, cls, prob):
                    np.testing.assert_array_equal(c, wc, err_msg=f"batch={batch} invariant={batch_invariant}")
                    assert q.dtype == np.float32 and q.shape == wp.shape and q.tobytes() == wp.tobytes(), (batch, batch_invariant)
            grey = p(images)
            for (wc, _), g in zip(want, grey):
                np.testing.assert_array_equal(g, np.asarray([0, 128, 255], np.uint8)[wc])


def test_pool_fills_the_launches():
    """Tiles of images of different sizes that share a tile shape go through full forward steps: 12 + 6 tiles, batch 4."""
    import unet_amd
    dev = _dev()
    model = _model("UNet_S", False, dev)
    p = unet_amd.BatchPredictor(model, batch=4, postprocess=False, tile=_cfg(32, 8), batch_invariant=True)
    seen = []
    forward = p._forward_cut
    p._forward_cut = lambda x, size, m: (seen.append((x.shape[0], tuple(size))), forward(x, size, m))[1]
    images = [_image(6, 70, 90), _image(7, 50, 70)]                                        # 3 x 4 and 2 x 3 tiles of 32 x 32
    both = p.classes(images)
    assert seen == [(4, (32, 32))] * 4 + [(2, (32, 32))]
    for img, c in zip(images, both):
        np.testing.assert_array_equal(p.classes([img])[0], c)


# ------------------------------------------------------------------ 6. with test-time augmentation
@pytest.mark.parametrize("mode", ["flips", "d4"])
def test_predictor_with_tta_equals_the_hand_composition(mode):
    import unet_amd
    from unet_amd import ops
    from unet_amd.utils.tta import tta_counts
    dev = _dev()
    model = _model("UNet_S", False, dev)
    cfg = _cfg(32, 8)
    img = _image(8, 48, 80)
    k0, k1 = tta_counts(mode)
    tiles = R.gather_ref(_prepared(img), cfg.size, cfg.overlap)
    sums = []
    for k in range(tiles.shape[0]):
        v0, v1 = ops.tta_views(_nchw(tiles[k:k + 1], dev), mode)
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16), ops.plan_images(1):
            l0 = torch.cat([model(v0[i:i + 1]).clone() for i in range(k0)])
            l1 = torch.cat([model(v1[i:i + 1]).clone() for i in range(k1)]) if k1 else None
        sums.append(ops.tta_merge(l0, l1, mode, (32, 32), sums=True).sums)
    merged = ops.tile_merge(torch.cat(sums), cfg, img.shape, k0 + k1, probs=True)
    assert len(np.unique(merged.classes.cpu().numpy())) > 1
    for batch in (8, 3):
        p = unet_amd.BatchPredictor(model, batch=batch, postprocess=False, tta=mode, tile=cfg)
        np.testing.assert_array_equal(p.classes([img])[0], merged.classes[0].cpu().numpy())
        assert p.probabilities([img])[0].tobytes() == merged.probs[0].permute(2, 0, 1).contiguous().cpu().numpy().tobytes()


# ------------------------------------------------------------------ 7. evaluate
@pytest.mark.parametrize("tta", [None, "flips"])
def test_evaluate_scores_the_tiled_prediction(tta):
    import unet_amd
    dev = _dev()
    model = _model("UNet_S", False, dev)
    cfg = _cfg(32, 8)
    H, W = 48, 80
    images = [_image(30 + i, H, W) for i in range(4)]
    masks = [_mask(40 + i, H, W) for i in range(4)]
    loader = _loader(images, masks)
    p = unet_amd.BatchPredictor(model, postprocess=False, tta=tta, tile=cfg, batch_invariant=True)
    cls = p.classes(images)
    total = torch.zeros((), dtype=torch.float32, device=dev)
    low = torch.full((), 10.0, dtype=torch.float32, device=dev)
    for s in range(0, 4, 2):
        pred = torch.from_numpy(np.stack(cls[s:s + 2])).to(dev)
        true = torch.from_numpy(np.stack(masks[s:s + 2])).to(dev)
        d = unet_amd.dice_coeff((pred == 2).float(), (true == 2).float(), reduce_batch_first=False)
        total += d
        low = torch.minimum(low, d.float())
    want = [float(total / 2), float(total / 2), float(low)]
    got = unet_amd.evaluate(model, loader, dev, True, postprocess=False, tta=tta, tile=cfg)
    assert [float(v) for v in got] == want
    assert 0.0 < want[0] < 1.0, "a degenerate prediction compares nothing"
    today = unet_amd.evaluate(model, loader, dev, True, postprocess=False, tta=tta)
    none = unet_amd.evaluate(model, loader, dev, True, postprocess=False, tta=tta, tile=None)
    assert [float(v) for v in today] == [float(v) for v in none]
    with pytest.raises(ValueError):
        unet_amd.evaluate(model, loader, dev, True, tile="24")


# ------------------------------------------------------------------ 8. the command lines
def test_predict_cli_writes_what_the_predictor_returns(tmp_path):
    import unet_amd
    from PIL import Image
    from test_gpu_predict_cli import _cli
    dev = _dev()
    model = _model("UNet_T", False, dev)
    wpath = unet_amd.save_checkpoint(model.cpu(), str(tmp_path / "w.pth"), mask_values=[0, 128, 255])
    model = model.to(dev)
    src = tmp_path / "in"
    src.mkdir()
    files = {"a.png": (70, 90), "b.png": (47, 31), "c.png": (50, 70), "d.png": (20, 24)}
    images = {}
    for k, (name, (H, W)) in enumerate(files.items()):
        images[name] = _image(60 + k, H, W)
        Image.fromarray(images[name]).save(src / name)
    out = tmp_path / "out"
    r = _cli(["-m", wpath, "--arch", "UNet_T", "-i", str(src), "-o", str(out), "--no-postprocess", "-b", "3",
              "--tile", "32,overlap=8"], tmp_path)
    assert r.returncode == 0, r.stderr[-4000:]
    p = unet_amd.BatchPredictor(model, batch=3, postprocess=False, batch_invariant=True, tile="32,overlap=8")
    want = p([images[n] for n in files])
    assert sorted(os.listdir(out)) == sorted(files)
    for n, w in zip(files, want):
        np.testing.assert_array_equal(np.asarray(Image.open(out / n)), w, err_msg=n)
    assert any(len(np.unique(w)) > 1 for w in want)


def test_evaluate_cli_records_the_spec(tmp_path):
    import json
    import unet_amd
    from PIL import Image
    from unet_amd.evaluate_cli import main
    dev = _dev()
    model = _model("UNet_T", False, dev)
    wpath = unet_amd.save_checkpoint(model.cpu(), str(tmp_path / "w.pth"), mask_values=[0, 128, 255])
    model.to(dev)
    data = tmp_path / "data"
    for d in ("imgs", "masks"):
        os.makedirs(data / d / "val")
    for i in range(2):
        Image.fromarray(_image(70 + i, 80, 80)).save(data / "imgs" / "val" / f"p{i}.png")
        Image.fromarray(np.asarray([0, 128, 255], np.uint8)[_mask(80 + i, 80, 80)]).save(data / "masks" / "val" / f"p{i}_mask.png")
    out = tmp_path / "out.json"
    rc = main(["-m", wpath, "--data-root", str(data), "--arch", "UNet_T", "-b", "2", "-s", "1.0", "--workers", "2", "--no-metrics",
               "--tile", "32,overlap=8", "--tta", "flips", "--json", str(out)])
    assert rc == 0
    rep = json.loads(out.read_text())
    assert rep["tile"] == "32,overlap=8" and rep["tta"] == "flips"
    assert 0.0 <= rep["dice"]["min"] <= rep["dice"]["mean"] <= 1.0
