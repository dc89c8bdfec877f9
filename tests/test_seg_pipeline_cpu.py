"""RAW -> contour pipeline (seg_main.py), host side: the restatements against G18 and live PIL, the window formula, the
hand-derived contours, the JSON layout, the CLI and the refusals.  GPU side: test_gpu_seg_pipeline.py."""
import json
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import seg_pipeline_ref as R  # noqa: E402
from conftest import load_golden  # noqa: E402

G18 = [(700, 300), (300, 700), (512, 384), (512, 512), (100, 37), (1000, 999)]


# ------------------------------------------------------------------ letterbox geometry and LANCZOS
@pytest.mark.parametrize("W,H", G18)
def test_geometry_and_restatement_reproduce_g18(W, H):
    import unet_amd
    g = load_golden(f"g18_{W}x{H}")
    assert unet_amd.letterbox_geometry(W, H) == R.geometry_ref(W, H)
    assert json.loads(str(g["sizes_json"]))[f"g18_{W}x{H}.png"] == {"width": W, "height": H}
    np.testing.assert_array_equal(R.letterbox_ref(g["image"]), g["normalized"])
    np.testing.assert_array_equal(R.unletterbox_ref(g["mask3"], W, H), g["denorm3"])
    np.testing.assert_array_equal(R.unletterbox_ref(g["mask2"], W, H), g["denorm2"])


@pytest.mark.parametrize("src,dst", [((700, 300), (512, 219)), ((40, 96), (213, 512)), ((2048, 1536), (512, 384)),
                                     ((512, 384), (2048, 1536)), ((50, 50), (512, 512)), ((4000, 3000), (512, 384))])
def test_lanczos_restatement_matches_live_pil(src, dst):
    rng = np.random.default_rng(src[0] + dst[1])
    a = (rng.random(src[::-1]) * 256).astype(np.uint8)
    pil = np.asarray(Image.fromarray(a, mode="L").resize(dst, Image.LANCZOS))
    np.testing.assert_array_equal(R.resize_ref(a, dst), pil)


@pytest.mark.parametrize("n_in,n_out", [(700, 512), (96, 512), (4000, 512), (219, 300), (512, 512), (37, 100)])
def test_package_coefficient_tables_equal_restatement(n_in, n_out):
    from unet_amd.utils.png_normalize import lanczos_coeffs
    b, k = lanczos_coeffs(n_in, n_out)
    rb, rk = R.coeffs_ref(n_in, 0.0, n_in, n_out)
    np.testing.assert_array_equal(b, rb)
    np.testing.assert_array_equal(k, rk)
    assert lanczos_coeffs(n_in, n_out)[1] is k                      # cached per geometry


def test_downscale_from_4000_needs_more_than_six_taps():
    from unet_amd.utils.png_normalize import lanczos_coeffs
    b, _ = lanczos_coeffs(4000, 512)
    assert b[:, 1].max() >= 25


def test_zero_size_letterbox_is_refused():
    import unet_amd
    with pytest.raises(ValueError):
        unet_amd.letterbox_geometry(2000, 1)
    with pytest.raises(ValueError):
        R.geometry_ref(2000, 1)
    with pytest.raises(ValueError):
        Image.new("L", (2000, 1)).resize((512, 0), Image.LANCZOS)


# ------------------------------------------------------------------ window / level
@pytest.mark.parametrize("wl,ww", [(40, 400), (1000, 400), (1000, 401), (32768, 65535), (1000, 2)])
def test_window_formula_matches_reference_arithmetic(wl, ww):
    x = np.arange(65536, dtype=np.uint16)
    mn, mx = wl - ww // 2, wl + ww // 2
    # the reference's float64 arithmetic, element by element in Python (numpy 1.26 semantics, no uint16 np.clip)
    want = np.array([int(float(min(max(int(v), mn), mx) - mn) / float(mx - mn) * 255.0) for v in x[::97]], np.uint8)
    np.testing.assert_array_equal(R.window_ref(x, ww, wl)[::97], want)
    if mn >= 0 and mx <= 65535:
        np.testing.assert_array_equal(R.window_ref(x, ww, wl), ((np.clip(x, mn, mx) - mn) / (mx - mn) * 255).astype(np.uint8))


def test_window_refusals(tmp_path):
    from unet_amd.utils.raw2png import read_raw, window_bounds
    with pytest.raises(ValueError):
        window_bounds(1, 100)
    with pytest.raises(ValueError):
        window_bounds(0, 100)
    assert window_bounds(400, 40) == (-160, 240)
    p = tmp_path / "a.raw"
    np.arange(12, dtype="<u2").tofile(p)
    assert read_raw(str(p), 4, 3).tolist() == np.arange(12).reshape(3, 4).tolist()
    with pytest.raises(ValueError):
        read_raw(str(p), 5, 3)


# ------------------------------------------------------------------ contours: hand-derived answers
def _c(img):
    return [c.tolist() for c in R.contours_ref(np.asarray(img, np.uint8))]


def test_contour_single_pixel_and_runs():
    a = np.zeros((5, 6), np.uint8)
    a[2, 3] = 1
    assert _c(a) == [[[3, 2]]]
    a = np.zeros((5, 6), np.uint8)
    a[1, 1:5] = 1
    assert _c(a) == [[[1, 1], [4, 1]]]
    a = np.zeros((6, 5), np.uint8)
    a[1:5, 2] = 1
    assert _c(a) == [[[2, 1], [2, 4]]]


def test_contour_rectangle_l_shape_and_diagonal():
    a = np.zeros((7, 8), np.uint8)
    a[1:5, 2:7] = 1
    assert _c(a) == [[[2, 1], [2, 4], [6, 4], [6, 1]]]               # counter-clockwise on screen, down the left side
    a = np.zeros((7, 7), np.uint8)
    a[1:6, 1] = 1
    a[5, 1:5] = 1
    assert _c(a) == [[[1, 1], [1, 5], [4, 5], [2, 5], [1, 4]]]      # coming back, the inner corner is cut diagonally
    a = np.zeros((6, 6), np.uint8)
    for i in range(4):
        a[1 + i, 1 + i] = 1
    assert _c(a) == [[[1, 1], [4, 4]]]


def test_contour_spur_visited_twice():
    a = np.zeros((6, 8), np.uint8)
    a[2:5, 1:4] = 1
    a[3, 4:7] = 1                                                   # one-pixel-wide spur to the east
    c = _c(a)[0]
    assert c[0] == [1, 2] and c.count([6, 3]) == 1
    assert c.count([4, 3]) == 2                                     # the spur's base is passed going out and back


def test_contour_ring_with_island_and_two_blobs_order():
    a = np.zeros((11, 11), np.uint8)
    a[1:10, 1:10] = 1
    a[3:8, 3:8] = 0
    a[5, 5] = 1                                                     # island inside the hole: not external
    assert _c(a) == [[[1, 1], [1, 9], [9, 9], [9, 1]]]
    b = np.zeros((8, 12), np.uint8)
    b[1:3, 1:3] = 1
    b[4:6, 7:10] = 1
    assert _c(b) == [[[7, 4], [7, 5], [9, 5], [9, 4]], [[1, 1], [1, 2], [2, 2], [2, 1]]]   # last found comes first


def test_contour_blobs_touching_every_edge_and_empty():
    a = np.zeros((6, 7), np.uint8)
    a[0:2, 0:2] = 1
    a[4:6, 5:7] = 1
    assert _c(a) == [[[5, 4], [5, 5], [6, 5], [6, 4]], [[0, 0], [0, 1], [1, 1], [1, 0]]]
    assert _c(np.ones((3, 4), np.uint8)) == [[[0, 0], [0, 2], [3, 2], [3, 0]]]
    assert _c(np.zeros((4, 4), np.uint8)) == []


# ------------------------------------------------------------------ JSON and CLI
def test_contour_json_layout():
    from unet_amd.utils.mask2polygon import contour_json, json_text
    assert contour_json([], "x", 10, 20) is None
    d = contour_json([np.array([[1, 2], [3, 4]], np.int32)], "scan_01", 700, 300)
    assert list(d) == ["version", "imagePath", "imageData", "flags", "shapes", "imageWidth", "imageHeight"]
    assert list(d["shapes"][0]) == ["label", "labelIndex", "points", "shape_type", "description", "mask", "group_id", "flags"]
    want = ('{\n  "version": "1.0.2.799",\n  "imagePath": "scan_01",\n  "imageData": null,\n  "flags": {},\n  "shapes": [\n'
            '    {\n      "label": 1,\n      "labelIndex": 0,\n      "points": [\n        [\n          1,\n          2\n'
            '        ],\n        [\n          3,\n          4\n        ]\n      ],\n      "shape_type": "polygon",\n'
            '      "description": "",\n      "mask": null,\n      "group_id": null,\n      "flags": {}\n    }\n  ],\n'
            '  "imageWidth": 700,\n  "imageHeight": 300\n}')
    assert json_text(d) == want


def test_cli_parsing_and_aliases():
    from unet_amd.seg_main import build_parser
    a = build_parser().parse_args(["--input-raw", "d", "--width", "2048", "--height", "1536", "-ww", "400", "-wl", "40",
                                   "-m", "w.pth"])
    assert (a.output_root, a.window_width, a.window_length, a.model, a.keep_stages) == ("seg_results", 400, 40, "w.pth", False)
    b = build_parser().parse_args(["--input-raw", "d", "-o", "r", "--width", "5", "--height", "6", "--window-width", "3",
                                   "--window-length", "-7", "--model", "m.pth", "--keep-stages"])
    assert (b.output_root, b.window_width, b.window_length, b.keep_stages) == ("r", 3, -7, True)
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--input-raw", "d", "--width", "5", "--height", "6", "-ww", "3", "-m", "m.pth"])


def test_device_entry_points_refuse_cpu_tensors():
    import unet_amd
    from unet_amd.utils.png_denormalize import unletterbox
    with pytest.raises(RuntimeError, match="GPU"):
        unet_amd.window_level(torch.zeros(4, 4, dtype=torch.int16), 400, 40)
    with pytest.raises(RuntimeError, match="GPU"):
        unet_amd.letterbox(torch.zeros(30, 40, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="GPU"):
        unletterbox(torch.zeros(512, 512, dtype=torch.uint8), 40, 30)
    with pytest.raises(RuntimeError, match="GPU"):
        unet_amd.external_contours(torch.zeros(30, 40, dtype=torch.uint8))


def test_pipeline_refuses_bad_windows_and_geometry():
    import unet_amd
    with pytest.raises(ValueError):
        unet_amd.ContourPipeline(torch.nn.Identity(), 64, 64, 1, 40)
    with pytest.raises(ValueError):
        unet_amd.ContourPipeline(torch.nn.Identity(), 4000, 1, 400, 40)
