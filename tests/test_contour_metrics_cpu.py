"""Contour metrics, host side: known answers of the scipy / numpy restatement (tests/contour_metrics_ref.py) that the GPU
tests use as their yardstick, its transform against an O(N^2) brute force, the ContourMetrics reduction arithmetic (alone and
over gloo at two ranks), the `python -m unet_amd.evaluate` parser and its refusals, and the new C-ABI symbols."""
import ctypes
import math
import os
import socket

import numpy as np
import pytest
import torch
from PIL import Image

import contour_metrics_ref as R


# ------------------------------------------------------------------------------------------------ known answers
def _square(H, W, y0, x0, side):
    m = np.zeros((H, W), bool)
    m[y0:y0 + side, x0:x0 + side] = True
    return m


def test_shifted_squares_give_hd_5():
    P, T = _square(64, 64, 10, 10, 20), _square(64, 64, 13, 14, 20)
    m = R.image_metrics(P, T)
    assert m["hd"] == 5.0 and m["max_d2"] == 25 and m["undefined"] == 0
    assert m["n"] == m["n_border_pred"] + m["n_border_true"] == 2 * (4 * 20 - 4)
    assert m["iou"] == (17 * 16) / (2 * 400 - 17 * 16)
    assert 0.0 < m["assd"] <= m["hd95"] <= m["hd"]


def test_mask_against_itself_is_all_zero():
    P = R.blob_mask(np.random.default_rng(0), 80, 60)
    m = R.image_metrics(P, P)
    assert (m["hd"], m["hd95"], m["assd"], m["iou"], m["max_d2"]) == (0.0, 0.0, 0.0, 1.0, 0)


def test_single_pixels_give_their_euclidean_distance():
    P, T = np.zeros((20, 30), bool), np.zeros((20, 30), bool)
    P[3, 4], T[10, 28] = True, True
    m = R.image_metrics(P, T)
    want = math.sqrt(7 ** 2 + 24 ** 2)
    assert m["hd"] == m["hd95"] == m["assd"] == want == 25.0 and m["n"] == 2 and m["iou"] == 0.0


def test_image_edge_pixels_are_border():
    M = np.zeros((8, 9), bool)
    M[0:5, 0:6] = True                                  # touches the top and the left edge
    b = R.border(M)
    assert b[0, 0:6].all() and b[0:5, 0].all() and b[4, 0:6].all() and b[0:5, 5].all()
    assert not b[1:4, 1:5].any() and b.sum() == 6 * 5 - 3 * 4
    full = np.ones((5, 7), bool)
    assert R.border(full).sum() == 5 * 7 - 3 * 5        # a full image: its frame


def test_empty_cases():
    E, M = np.zeros((16, 16), bool), _square(16, 16, 4, 4, 5)
    both = R.image_metrics(E, E)
    assert (both["hd"], both["hd95"], both["assd"], both["iou"], both["undefined"], both["n"]) == (0.0, 0.0, 0.0, 1.0, 0, 0)
    for P, T in ((E, M), (M, E)):
        one = R.image_metrics(P, T)
        assert math.isnan(one["hd"]) and math.isnan(one["hd95"]) and math.isnan(one["assd"])
        assert one["iou"] == 0.0 and one["undefined"] == 1
    s = R.set_metrics([R.image_metrics(E, M), R.image_metrics(M, M), R.image_metrics(E, E)])
    assert s["n"] == 3 and s["n_undefined"] == 1 and s["hd"] == 0.0 and s["iou"] == (0.0 + 1.0 + 1.0) / 3
    assert (R.edt_sq(E) == R.NO_FEATURE).all()


def test_restatement_edt_equals_brute_force():
    rng = np.random.default_rng(3)
    for feat in (rng.random((100, 37)) < 0.01, R.border(R.blob_mask(rng, 100, 37)), np.zeros((100, 37), bool)):
        assert np.array_equal(R.edt_sq(feat), R.edt_sq_brute(feat))
    one = np.zeros((100, 37), bool)
    one[99, 0] = True
    assert R.edt_sq(one)[0, 36] == 99 ** 2 + 36 ** 2


# ------------------------------------------------------------------------------------------------ the accumulator
def make_records(rows):
    """A float64 [B,12] record table (uh_contour_record rows) from image_metrics-style dicts."""
    from unet_amd.utils.contour_metrics import FLOAT_FIELDS, INT_FIELDS
    rec = torch.zeros(len(rows), 12, dtype=torch.float64)
    ints = rec.view(torch.int32)
    for i, m in enumerate(rows):
        for k, name in enumerate(INT_FIELDS):
            ints[i, k] = int(m.get(name, 0))
        for k, name in enumerate(FLOAT_FIELDS):
            rec[i, 6 + k] = float(m.get(name, 0.0))
    return rec


_NAN = float("nan")
_ROWS = [dict(hd=5.0, hd95=4.5, assd=2.0, iou=0.5, undefined=0, n=10),
         dict(hd=_NAN, hd95=_NAN, assd=_NAN, iou=0.0, undefined=1),
         dict(hd=1.0, hd95=1.0, assd=0.25, iou=0.75, undefined=0, n=7),
         dict(hd=0.0, hd95=0.0, assd=0.0, iou=1.0, undefined=0),
         dict(hd=9.0, hd95=8.0, assd=3.5, iou=0.25, undefined=0, n=4)]


def _check_set(got, rows, spacing):
    want = R.set_metrics(rows, spacing)
    for k in ("hd", "hd95", "hd_max", "assd", "iou"):
        assert got[k] == pytest.approx(want[k], rel=1e-12, abs=0), k
    assert got["n"] == want["n"] and got["n_undefined"] == want["n_undefined"]


def test_accumulator_arithmetic():
    from unet_amd import ContourMetrics
    acc = ContourMetrics(spacing=0.5)
    acc.update(make_records(_ROWS[:2]), "raw")
    acc.update(make_records(_ROWS[2:]), "raw")
    acc.update(make_records(_ROWS[3:]), "post")
    res = acc.result()
    _check_set(res["raw"], _ROWS, 0.5)
    _check_set(res["post"], _ROWS[3:], 0.5)
    assert res["raw"]["hd"] == (5.0 + 1.0 + 0.0 + 9.0) / 4 * 0.5 and res["raw"]["hd_max"] == 4.5 and res["raw"]["n_undefined"] == 1
    per = res["raw"]["per_image"]
    assert per["hd"].shape == (5,) and np.isnan(per["hd"][1]) and per["hd"][4] == 4.5 and per["iou"][2] == 0.75
    assert per["undefined"].tolist() == [False, True, False, False, False]
    empty = ContourMetrics().result()
    assert empty["raw"]["n"] == 0 and math.isnan(empty["raw"]["hd"]) and empty["post"]["n"] == 0
    only_undefined = ContourMetrics()
    only_undefined.update(make_records(_ROWS[1:2]))
    r = only_undefined.result()["raw"]
    assert r["n"] == 1 and r["n_undefined"] == 1 and math.isnan(r["hd"]) and math.isnan(r["hd_max"]) and r["iou"] == 0.0
    with pytest.raises(ValueError):
        acc.update(make_records(_ROWS[:1]), "other")
    with pytest.raises(RuntimeError):
        acc.update(torch.zeros(2, 11, dtype=torch.float64))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _gloo_worker(rank, world, port, q):
    try:
        import torch.distributed as dist
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from unet_amd import ContourMetrics
        mine = _ROWS[:2] if rank == 0 else _ROWS[2:]
        acc = ContourMetrics(spacing=2.0)
        acc.update(make_records(mine), "raw")
        if rank == 1:
            acc.update(make_records(_ROWS[4:]), "post")          # rank 0 holds no post-processed record at all
        acc.all_reduce(None)
        res = acc.result()
        _check_set(res["raw"], _ROWS, 2.0)
        _check_set(res["post"], _ROWS[4:], 2.0)
        assert len(res["raw"]["per_image"]["hd"]) == len(mine)   # the per-image arrays stay the rank's own
        dist.destroy_process_group()
        q.put((rank, "ok"))
    except Exception as e:  # pragma: no cover
        q.put((rank, repr(e)))


def test_accumulator_all_reduce_gloo_world2():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gloo_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=30)
    assert all(r[1] == "ok" for r in res), res


# ------------------------------------------------------------------------------------------------ the command lines
def test_evaluate_cli_defaults():
    from unet_amd.evaluate_cli import get_args
    a = get_args(["-m", "w.pth", "--data-root", "d"])
    assert (a.model, a.data_root, a.split, a.arch, a.classes, a.bilinear, a.batch_size, a.scale) == \
        ("w.pth", "d", "val", "UNet_S", 3, False, 8, 0.5)
    assert (a.postprocess, a.amp, a.metrics, a.spacing, a.pred_dir, a.workers, a.json) == (True, True, True, 1.0, None, 8, None)
    b = get_args(["-m", "w.pth", "--data-root", "d", "--split", "test", "--arch", "UNet_SA", "-c", "1", "--bilinear", "-b", "2",
                  "-s", "1", "--no-postprocess", "--no-amp", "--no-metrics", "--spacing", "0.7", "--pred-dir", "p",
                  "--workers", "3", "--json", "o.json"])
    assert (b.split, b.arch, b.classes, b.bilinear, b.batch_size, b.scale, b.postprocess, b.amp, b.metrics, b.spacing,
            b.pred_dir, b.workers, b.json) == ("test", "UNet_SA", 1, True, 2, 1.0, False, False, False, 0.7, "p", 3, "o.json")
    for bad in ([], ["-m", "w.pth"], ["--data-root", "d"], ["-m", "w.pth", "--data-root", "d", "--arch", "VGG"]):
        with pytest.raises(SystemExit) as e:
            get_args(bad)
        assert e.value.code == 2
    from unet_amd.train_cli import get_args as train_args
    assert train_args([]).metrics is False and train_args(["--metrics"]).metrics is True


def _tiny_split(root, n, size=32):
    rng = np.random.default_rng(1)
    for d in ("imgs", "masks"):
        os.makedirs(os.path.join(root, d, "val"), exist_ok=True)
    for i in range(n):
        Image.fromarray(rng.integers(0, 256, (size, size), dtype=np.uint8)).save(os.path.join(root, "imgs", "val", f"p{i}.png"))
        Image.fromarray(rng.choice(np.array([0, 128, 255], np.uint8), (size, size))).save(
            os.path.join(root, "masks", "val", f"p{i}_mask.png"))


def test_evaluate_cli_exit_statuses(tmp_path, caplog, monkeypatch):
    import unet_amd
    from unet_amd.evaluate import main as via_evaluate
    from unet_amd.evaluate_cli import main
    good = str(tmp_path / "good.pth")
    torch.save(unet_amd.UNet_T(1, 3).state_dict(), good)
    data = str(tmp_path / "data")
    _tiny_split(data, 2)
    with caplog.at_level("ERROR"):
        assert main(["-m", good, "--data-root", str(tmp_path / "absent")]) == 1
        assert "does not exist" in caplog.text
        caplog.clear()
        assert main(["-m", good, "--data-root", data, "--split", "test"]) == 1          # a split that is not there
        os.makedirs(tmp_path / "hollow" / "imgs" / "val")
        os.makedirs(tmp_path / "hollow" / "masks" / "val")
        caplog.clear()
        assert main(["-m", good, "--data-root", str(tmp_path / "hollow"), "--arch", "UNet_T"]) == 1   # an empty split
        assert "No usable image" in caplog.text
        caplog.clear()
        assert main(["-m", good, "--data-root", data, "--arch", "UNet_T", "-b", "16"]) == 1   # 2 x 4 items < one batch
        assert "fewer than one batch" in caplog.text
        caplog.clear()
        assert main(["-m", str(tmp_path / "absent.pth"), "--data-root", data, "--arch", "UNet_T"]) == 1
        assert main(["-m", good, "--data-root", data, "--arch", "UNet"]) == 1           # another network's checkpoint
        assert "Failed to load" in caplog.text
        caplog.clear()
        monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
        assert main(["-m", good, "--data-root", data, "--arch", "UNet_T", "-b", "4"]) == 2     # all checks pass: no device
        assert "no GPU" in caplog.text
        assert via_evaluate(["-m", good, "--data-root", data, "--arch", "UNet_T", "-b", "4"]) == 2


# ------------------------------------------------------------------------------------------------ the C ABI
NEW_SYMBOLS = ("uh_mask_border_u8", "uh_edt_sq_ws_bytes", "uh_edt_sq_u8", "uh_contour_metrics_ws_bytes", "uh_contour_metrics")


def test_new_symbols_declared_and_exported():
    import unet_amd  # noqa: F401
    from unet_amd._lib import LIB, LIB_PATH, parse_header
    protos = parse_header()
    dll = ctypes.CDLL(LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in protos, f"{name} is not declared in include/unet_hip.h"
        assert hasattr(dll, name), f"{name} is not exported"
    assert protos["uh_contour_metrics"][1] == ["ptr", "ptr", "int", "int", "ptr", "int", "int", "int", "ptr", "size_t", "uh_stream"]
    assert LIB.query("uh_contour_metrics_ws_bytes", 8, 512, 512) >= 8 * ((511 ** 2 + 511 ** 2 + 1) * 4)
    assert LIB.query("uh_contour_metrics_ws_bytes", 1, 1, 1) >= 4
    assert LIB.query("uh_edt_sq_ws_bytes", 8, 512, 512) > 0
    assert LIB.query("uh_edt_sq_ws_bytes", 1, 2, 5000) >= 2 * 5000 * 4            # a row wider than LDS holds: searched in memory
    assert LIB.query("uh_contour_metrics_ws_bytes", 0, 512, 512) == 0


def test_new_entry_points_refuse_bad_arguments():
    import unet_amd  # noqa: F401
    from unet_amd._lib import LIB
    LIB.load()
    with pytest.raises(RuntimeError, match="uh_mask_border_u8"):
        LIB.call("uh_mask_border_u8", None, 2, None, 1, 8, 8, None)
    with pytest.raises(RuntimeError, match="uh_mask_border_u8"):
        LIB.call("uh_mask_border_u8", 16, 2, 16, 1, 0, 8, None)
    with pytest.raises(RuntimeError, match="uh_edt_sq_u8"):
        LIB.call("uh_edt_sq_u8", None, None, 1, 8, 8, None, 0, None)
    with pytest.raises(RuntimeError, match="uh_edt_sq_u8"):
        LIB.call("uh_edt_sq_u8", 16, 16, -1, 8, 8, 16, 1024, None)
    with pytest.raises(RuntimeError, match="uh_edt_sq_u8"):
        LIB.call("uh_edt_sq_u8", 16, 16, 1, 8, 40000, 16, 1 << 30, None)        # beyond the 31-bit distance range
    with pytest.raises(RuntimeError, match="uh_contour_metrics"):
        LIB.call("uh_contour_metrics", None, None, 2, 2, None, 1, 8, 8, None, 0, None)
    with pytest.raises(RuntimeError, match="uh_contour_metrics"):
        LIB.call("uh_contour_metrics", 16, 16, 2, 2, 16, 1, 8, 0, 16, 1024, None)
    with pytest.raises(RuntimeError, match=r"uh_contour_metrics.*workspace"):
        LIB.call("uh_contour_metrics", 16, 16, 2, 2, 16, 1, 8, 8, 16, 8, None)  # too small a workspace: said before any launch


def test_ops_refuse_host_tensors():
    from unet_amd import contour_metrics, ops
    m = torch.zeros(1, 8, 8, dtype=torch.uint8)
    for call in (lambda: ops.mask_border(m, 2), lambda: ops.edt_sq(m), lambda: ops.contour_metrics(m, m, 2, 2),
                 lambda: contour_metrics(m, m)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
