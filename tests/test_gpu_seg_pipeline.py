"""RAW -> contour pipeline (seg_main.py) on the MI355X: window / level, the two PIL-exact resamples, the contour tracer and
the whole pipeline against the host composition of the reference's stages (numpy, PIL, predict_img, postprocess_mask,
the contour restatement of tests/seg_pipeline_ref.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import seg_pipeline_ref as R  # noqa: E402
from conftest import load_golden  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G18 = [(700, 300), (300, 700), (512, 384), (512, 512), (100, 37), (1000, 999)]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _pil_letterbox(a):
    H, W = a.shape
    nw, nh, px, py = R.geometry_ref(W, H)
    c = Image.new("L", (512, 512), 0)
    c.paste(Image.fromarray(a, mode="L").resize((nw, nh), Image.LANCZOS), (px, py))
    return np.asarray(c)


def _pil_unletterbox(canvas, W, H):
    nw, nh, px, py = R.geometry_ref(W, H)
    return np.asarray(Image.fromarray(canvas, mode="L").crop((px, py, px + nw, py + nh)).resize((W, H), Image.LANCZOS))


# ------------------------------------------------------------------ stage 1
@pytest.mark.parametrize("wl,ww", [(40, 400), (1000, 400), (1000, 401), (32768, 65535), (1000, 2)])
def test_window_level_all_codes(wl, ww):
    import unet_amd
    dev = _dev()
    x = np.arange(65536, dtype=np.uint16)
    got = unet_amd.window_level(torch.from_numpy(x.view(np.int16)).to(dev), ww, wl).cpu().numpy()
    np.testing.assert_array_equal(got, R.window_ref(x, ww, wl))
    odd = unet_amd.window_level(torch.from_numpy(x[:1237].view(np.int16)).to(dev), ww, wl).cpu().numpy()   # scalar tail
    np.testing.assert_array_equal(odd, R.window_ref(x[:1237], ww, wl))


def test_window_level_refuses_empty_window():
    import unet_amd
    dev = _dev()
    with pytest.raises(ValueError):
        unet_amd.window_level(torch.zeros(8, dtype=torch.int16, device=dev), 1, 40)


# ------------------------------------------------------------------ stages 2 and 4
@pytest.mark.parametrize("W,H", G18)
def test_letterbox_and_unletterbox_match_g18_and_pil(W, H):
    import unet_amd
    from unet_amd.utils.png_denormalize import unletterbox
    dev = _dev()
    g = load_golden(f"g18_{W}x{H}")
    got = unet_amd.letterbox(torch.from_numpy(g["image"]).to(dev)).cpu().numpy()
    np.testing.assert_array_equal(got, g["normalized"])
    np.testing.assert_array_equal(got, _pil_letterbox(g["image"]))
    for k in ("3", "2"):
        back = unletterbox(torch.from_numpy(g["mask" + k]).to(dev), W, H).cpu().numpy()
        np.testing.assert_array_equal(back, g["denorm" + k])


@pytest.mark.parametrize("W,H", [(2048, 1536), (1536, 2048), (4000, 3000)])
def test_letterbox_round_trip_large_against_pil(W, H):
    import unet_amd
    from unet_amd.utils.png_denormalize import CLASS_TO_GREY, unletterbox
    dev = _dev()
    rng = np.random.default_rng(W + H)
    imgs = (rng.random((2, H, W)) * 256).astype(np.uint8)
    got = unet_amd.letterbox(torch.from_numpy(imgs).to(dev)).cpu().numpy()
    for b in range(2):
        np.testing.assert_array_equal(got[b], _pil_letterbox(imgs[b]))
    cls = rng.integers(0, 3, (2, 512, 512)).astype(np.uint8)
    back = unletterbox(torch.from_numpy(cls).to(dev), W, H, lut=CLASS_TO_GREY).cpu().numpy()
    for b in range(2):
        np.testing.assert_array_equal(back[b], _pil_unletterbox(CLASS_TO_GREY[cls[b]], W, H))


def test_letterbox_mixed_batch():
    import unet_amd
    dev = _dev()
    rng = np.random.default_rng(7)
    imgs = np.stack([np.zeros((300, 700), np.uint8), np.full((300, 700), 255, np.uint8),
                     (rng.random((300, 700)) * 256).astype(np.uint8), (rng.random((300, 700)) < 0.5).astype(np.uint8)])
    got = unet_amd.letterbox(torch.from_numpy(imgs).to(dev)).cpu().numpy()
    for b in range(len(imgs)):
        np.testing.assert_array_equal(got[b], _pil_letterbox(imgs[b]))


# ------------------------------------------------------------------ stage 5
HAND = []


def _hand_cases():
    a = np.zeros((5, 6), np.uint8); a[2, 3] = 255; HAND.append(a)
    a = np.zeros((5, 6), np.uint8); a[1, 1:5] = 255; HAND.append(a)
    a = np.zeros((6, 5), np.uint8); a[1:5, 2] = 255; HAND.append(a)
    a = np.zeros((7, 8), np.uint8); a[1:5, 2:7] = 255; HAND.append(a)
    a = np.zeros((7, 7), np.uint8); a[1:6, 1] = 255; a[5, 1:5] = 255; HAND.append(a)
    a = np.zeros((6, 6), np.uint8)
    for i in range(4):
        a[1 + i, 1 + i] = 255
    HAND.append(a)
    a = np.zeros((6, 8), np.uint8); a[2:5, 1:4] = 255; a[3, 4:7] = 255; HAND.append(a)
    a = np.zeros((11, 11), np.uint8); a[1:10, 1:10] = 255; a[3:8, 3:8] = 0; a[5, 5] = 255; HAND.append(a)
    a = np.zeros((8, 12), np.uint8); a[1:3, 1:3] = 255; a[4:6, 7:10] = 255; HAND.append(a)
    a = np.zeros((6, 7), np.uint8); a[0:2, 0:2] = 255; a[4:6, 5:7] = 255; HAND.append(a)
    HAND.append(np.full((3, 4), 200, np.uint8))
    HAND.append(np.full((4, 4), 127, np.uint8))                        # not > 127: empty


_hand_cases()


@pytest.mark.parametrize("i", range(len(HAND)))
def test_external_contours_hand_cases(i):
    import unet_amd
    dev = _dev()
    got = unet_amd.external_contours(torch.from_numpy(HAND[i]).to(dev))
    want = R.contours_ref(HAND[i] > 127)
    assert [c.tolist() for c in got] == [c.tolist() for c in want]
    assert all(c.dtype == np.int32 and c.ndim == 2 and c.shape[1] == 2 for c in got)


def _blobs(rng, H, W, n):
    yy, xx = np.mgrid[0:H, 0:W]
    m = np.zeros((H, W), np.uint8)
    for _ in range(n):
        cx, cy = rng.uniform(-0.05, 1.05) * W, rng.uniform(-0.05, 1.05) * H
        rx, ry = rng.uniform(0.01, 0.25) * W, rng.uniform(0.01, 0.25) * H
        inside = ((xx - cx) / rx) ** 2 + ((yy - cy) / ry) ** 2 < 1
        m[inside] = 255 if rng.random() < 0.75 else 0
    m[rng.random((H, W)) < 0.002] ^= 255                               # isolated pixels, pinholes, spurs
    return m


@pytest.mark.parametrize("H,W", [(37, 61), (300, 700), (1536, 2048)])
def test_external_contours_random_blobs_batch(H, W):
    import unet_amd
    dev = _dev()
    rng = np.random.default_rng(H * W)
    masks = np.stack([_blobs(rng, H, W, 12) for _ in range(8)])
    masks[3] = 0                                                       # an empty image inside the batch
    t = torch.from_numpy(masks).to(dev)
    got = unet_amd.external_contours(t)
    again = unet_amd.external_contours(t)
    assert got[3] == []
    for b in range(8):
        want = R.contours_ref(masks[b] > 127)
        assert len(got[b]) == len(want), f"image {b}"
        for c, w in zip(got[b], want):
            np.testing.assert_array_equal(c, w)
        assert len(again[b]) == len(got[b]) and all((x == y).all() for x, y in zip(again[b], got[b]))


# ------------------------------------------------------------------ end to end
def _phantoms(rng, n, H, W):
    """CT-like 16-bit scans: air around an elliptic body (~1000), an inner organ (~1060) and a bright bone (~1600)."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.empty((n, H, W), np.uint16)
    for i in range(n):
        img = rng.normal(30, 8, (H, W))
        cx, cy = W * rng.uniform(0.4, 0.6), H * rng.uniform(0.4, 0.6)
        rx, ry = W * rng.uniform(0.25, 0.4), H * rng.uniform(0.25, 0.4)
        img[((xx - cx) / rx) ** 2 + ((yy - cy) / ry) ** 2 < 1] = 1000 + rng.normal(0, 10, (H, W))[
            ((xx - cx) / rx) ** 2 + ((yy - cy) / ry) ** 2 < 1]
        img[((xx - cx) / (rx / 3)) ** 2 + ((yy - cy - ry / 3) / (ry / 4)) ** 2 < 1] += 600
        out[i] = np.clip(img, 0, 65535).astype(np.uint16)
    return out


class _IntensityStub(torch.nn.Module):
    """Logits that follow the input's intensity: class 2 where the pixel is bright, 1 in between, 0 for air."""

    def forward(self, x):
        return torch.cat([0.2 - x, 0.15 - (x - 0.2).abs(), x - 0.3], dim=1) * 8.0


def _host_composition(model, raw, ww, wl, dev):
    import unet_amd
    H, W = raw.shape
    canvas = _pil_letterbox(R.window_ref(raw, ww, wl))
    cls = unet_amd.postprocess_mask(unet_amd.predict_img(model, canvas, dev))
    grey = _pil_unletterbox(np.asarray(unet_amd.mask_to_image(cls)), W, H)
    return canvas, cls, grey, R.contours_ref(grey > 127)


@pytest.mark.parametrize("H,W,B", [(300, 700, 3), (1536, 2048, 8)])
def test_pipeline_stub_model_equals_host_composition(H, W, B):
    import unet_amd
    dev = _dev()
    rng = np.random.default_rng(H + W)
    raws = _phantoms(rng, B, H, W)
    model = _IntensityStub().to(dev)
    pipe = unet_amd.ContourPipeline(model, W, H, 400, 1040, batch=B)
    out = pipe.run_batch(raws)
    nonempty = 0
    for b in range(B):
        canvas, cls, grey, want = _host_composition(model, raws[b], 400, 1040, dev)
        np.testing.assert_array_equal(out["canvas"][b].cpu().numpy(), canvas)
        np.testing.assert_array_equal(out["classes"][b].cpu().numpy(), cls)
        np.testing.assert_array_equal(out["grey"][b].cpu().numpy(), grey)
        assert [c.tolist() for c in out["contours"][b]] == [c.tolist() for c in want]
        nonempty += len(want) > 0
    assert nonempty == B
    js = pipe(raws, [f"s{b}" for b in range(B)])
    assert all(j is not None and j["imageWidth"] == W and j["imageHeight"] == H for j in js)


def test_pipeline_unet_graphed_and_partial_batch():
    import unet_amd
    dev = _dev()
    torch.manual_seed(3)
    model = unet_amd.UNet(1, 3, bilinear=False).to(dev)
    rng = np.random.default_rng(11)
    raws = _phantoms(rng, 5, 300, 400)
    pipe = unet_amd.ContourPipeline(model, 400, 300, 400, 1040, batch=4)
    for s in (0, 4):                                                   # a full (graphed) batch, then a partial one
        out = pipe.run_batch(raws[s:s + 4])
        for b in range(out["canvas"].shape[0]):
            canvas, cls, grey, want = _host_composition(model, raws[s + b], 400, 1040, dev)
            np.testing.assert_array_equal(out["canvas"][b].cpu().numpy(), canvas)
            np.testing.assert_array_equal(out["argmax"][b].cpu().numpy(), unet_amd.predict_img(model, canvas, dev))
            np.testing.assert_array_equal(out["classes"][b].cpu().numpy(), cls)
            np.testing.assert_array_equal(out["grey"][b].cpu().numpy(), grey)
            assert [c.tolist() for c in out["contours"][b]] == [c.tolist() for c in want]
    assert pipe._graph is not None


def test_cli_on_a_directory(tmp_path):
    import unet_amd
    _dev()
    torch.manual_seed(4)
    model = unet_amd.UNet(1, 3, bilinear=False)
    wpath = unet_amd.save_checkpoint(model, str(tmp_path / "w.pth"), mask_values=[0, 1, 2])
    rng = np.random.default_rng(5)
    raws = _phantoms(rng, 3, 120, 160)
    d = tmp_path / "raw"
    d.mkdir()
    for i in range(3):
        raws[i].astype("<u2").tofile(d / f"scan{i}.raw")
    np.zeros(10, "<u2").tofile(d / "bad.raw")                           # wrong size: skipped, the others written
    out = tmp_path / "out"
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "unet_amd.seg_main", "--input-raw", str(d), "-o", str(out), "--width", "160",
                        "--height", "120", "-ww", "400", "-wl", "1040", "-m", wpath, "--keep-stages"],
                       capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "bad.raw" in r.stderr
    sizes = json.load(open(out / "2_normalized_png" / "original_sizes.json"))
    assert sorted(sizes) == ["scan0.png", "scan1.png", "scan2.png"]
    for i in range(3):
        win = np.asarray(Image.open(out / "1_raw_png" / f"scan{i}.png"))
        np.testing.assert_array_equal(win, R.window_ref(raws[i], 400, 1040))
        np.testing.assert_array_equal(np.asarray(Image.open(out / "2_normalized_png" / f"scan{i}.png")), _pil_letterbox(win))
        grey = np.asarray(Image.open(out / "4_denormalized_masks" / f"scan{i}.png"))
        want = R.contours_ref(grey > 127)
        jp = out / "5_json_results" / f"scan{i}.json"
        assert jp.exists() == bool(want)
        if want:
            d5 = json.load(open(jp, encoding="utf-8"))
            assert [s["points"] for s in d5["shapes"]] == [c.tolist() for c in want]
