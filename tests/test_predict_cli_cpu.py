"""CPU checks of the prediction command line: the restatements of tests/predict_ref.py against fixture G19 (recorded from
the reference's own predict.py / evaluate.py functions), the package's tables, path rules and directory walk against the
restatements, the batch planner's properties, argument parsing and the refusals that happen before a device is needed,
the ordered PNG writer, and the C ABI of csrc/predict_io.hip (exports and argument checks; no launch without a GPU)."""
import ctypes
import json
import logging
import os
import sys
import types

import numpy as np
import pytest
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import predict_ref as R  # noqa: E402
from conftest import load_golden  # noqa: E402


@pytest.fixture(scope="module")
def g19():
    r = load_golden("g19_predict_cli")
    return r, json.loads(str(r["meta_json"]))


def _touch_tree(root, names):
    for rel in names:
        p = os.path.join(root, rel)
        os.makedirs(os.path.dirname(p), exist_ok=True)
        open(p, "wb").close()


# ------------------------------------------------------------------ 1. restatements == G19, package == restatements
def test_output_paths_reproduce_g19(g19):
    from unet_amd import predict_cli
    _, meta = g19
    assert "not OpenCV" in meta["postprocess_mask"]
    for (output, f), want in zip(meta["path_cases"], meta["output_paths"]):
        assert R.output_path_ref(output, f) == want
        assert predict_cli.output_path(output, f) == want
    assert meta["output_dirs_created"] == ["out", "out/deep"]


def test_directory_walk_reproduces_g19(g19, tmp_path):
    from unet_amd import predict_cli
    _, meta = g19
    _touch_tree(str(tmp_path), meta["tree"])
    found = R.walk_ref(str(tmp_path))
    assert sorted(os.path.relpath(f, tmp_path) for f in found) == meta["walk_found_sorted"]
    assert predict_cli.discover(str(tmp_path)) == found                # same files in the same (os.walk) order
    assert "b.PNG" in meta["walk_found_sorted"] and "sub/h.Jpg" in meta["walk_found_sorted"]
    assert "f.png.bak" not in meta["walk_found_sorted"] and "png" not in meta["walk_found_sorted"]
    empty = tmp_path / "none"
    empty.mkdir()
    assert R.walk_ref(str(empty)) == meta["walk_empty"] == predict_cli.discover(str(empty)) == []


def test_grey_tables_reproduce_g19(g19):
    from unet_amd import predict
    r, _ = g19
    codes = np.arange(256).reshape(16, 16)
    for key, dt in (("mask_to_image_u8", np.uint8), ("mask_to_image_i64", np.int64)):
        np.testing.assert_array_equal(R.grey_classes_ref(codes.astype(dt)), r[key])
        np.testing.assert_array_equal(np.asarray(predict.mask_to_image(codes.astype(dt))), r[key])
    np.testing.assert_array_equal(predict.GREY_CLASSES, R.table_ref(R.grey_classes_ref))
    np.testing.assert_array_equal(predict.GREY_POSTPROCESSED, R.table_ref(R.grey_postprocessed_ref))
    np.testing.assert_array_equal(predict.GREY_BINARY, R.table_ref(R.grey_binary_ref))
    assert list(predict.GREY_CLASSES[:4]) == [0, 128, 255, 0] and predict.GREY_CLASSES[3:].max() == 0
    assert list(predict.GREY_POSTPROCESSED[:4]) == [0, 0, 255, 0]      # evaluate.py:160-163: class 1 -> 0
    assert list(predict.GREY_BINARY[:4]) == [0, 255, 0, 0]


@pytest.mark.parametrize("n_classes", [3, 1])
@pytest.mark.parametrize("postprocess", [True, False])
def test_evaluate_dump_naming_and_coding_reproduce_g19(g19, n_classes, postprocess):
    r, meta = g19
    tag = f"eval_c{n_classes}_{'pp' if postprocess else 'raw'}"
    want = {k[len(tag) + 6:]: v for k, v in r.items() if k.startswith(tag + ".file.")}
    got = R.evaluate_dump_ref(r[tag + ".raw"], r[tag + ".post"], n_classes, postprocess)
    assert sorted(got) == sorted(want) == meta[tag]["files"]
    assert meta[tag]["dirs"] == (["postprocessed"] if postprocess else [])
    assert "pred_batch1_sample0.png" in got and "pred_batch0_sample0.png" not in got       # the counter starts at 1
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    levels = set(np.unique(np.concatenate([v.ravel() for k, v in want.items() if not k.startswith("postprocessed")])))
    assert levels == ({0, 128, 255} if n_classes == 3 else {0, 255})
    if postprocess and n_classes == 3:
        post = np.concatenate([v.ravel() for k, v in want.items() if k.startswith("postprocessed")])
        assert set(np.unique(post)) == {0, 255}


# ------------------------------------------------------------------ 2. the planner
def _check_plan(sizes, batch, window=None):
    from unet_amd.predict import plan_batches
    plan = plan_batches(sizes, batch, window)
    seen = []
    for size, members in plan:
        assert 1 <= len(members) <= batch
        assert all(tuple(sizes[i]) == tuple(size) for i in members)
        assert members == sorted(members)
        seen.extend(members)
    assert sorted(seen) == list(range(len(sizes))) and len(seen) == len(set(seen))
    return plan


def test_planner_properties_on_random_lists():
    rng = np.random.default_rng(0)
    pool = [(512, 512), (384, 512), (999, 1000), (700, 300), (1, 1)]
    for trial in range(300):
        n = int(rng.integers(0, 60))
        sizes = [pool[int(k)] for k in rng.integers(0, int(rng.integers(1, len(pool) + 1)), n)]
        batch = int(rng.integers(1, 10))
        plan = _check_plan(sizes, batch)
        for size in set(sizes):                                        # without a window only the last batch of a size is partial
            lens = [len(m) for s, m in plan if s == size]
            assert all(v == batch for v in lens[:-1])
        window = int(rng.integers(1, 40))
        plan = _check_plan(sizes, batch, window)
        # no item waits for an index more than max(window, batch) past its own
        released = {}
        for step, (_, members) in enumerate(plan):
            for i in members:
                released[i] = max(members)
        assert all(released[i] - i <= max(window, batch) for i in released)


def test_write_order_is_discovery_order_with_duplicate_stems(tmp_path):
    """Batches finish in size order, files are committed in input order: the later input wins a shared output path."""
    from unet_amd.predict import plan_batches
    from unet_amd.predict_cli import output_path
    from unet_amd.utils.png_writer import OrderedPngWriter
    rng = np.random.default_rng(3)
    for trial in range(5):
        n = 40
        stems = [f"s{int(k)}" for k in rng.integers(0, 12, n)]
        files = [os.path.join("in", f"d{i % 3}", stems[i] + (".jpg" if i % 2 else ".png")) for i in range(n)]
        sizes = [[(8, 8), (5, 7), (3, 3)][int(k)] for k in rng.integers(0, 3, n)]
        out = tmp_path / f"o{trial}"
        out.mkdir()
        w = OrderedPngWriter(workers=4)
        plan = plan_batches(sizes, 4)
        for _, members in reversed(plan):                              # any completion order
            for i in members:
                if i % 11 == 5:
                    w.skip(i)                                          # an input that failed to decode
                else:
                    w.submit(i, output_path(str(out), files[i]), np.full(sizes[i], i, np.uint8))
        written = w.close()
        order = [i for i in range(n) if i % 11 != 5]
        assert written == [output_path(str(out), files[i]) for i in order]
        winners = {}
        for i in order:
            winners[output_path(str(out), files[i])] = i
        assert sorted(os.listdir(out)) == sorted(os.path.basename(p) for p in winners)
        for p, i in winners.items():
            a = np.asarray(Image.open(p))
            assert a.shape == sizes[i] and (a == i).all() and Image.open(p).mode == "L"


def test_writer_reports_a_failed_write(tmp_path):
    from unet_amd.utils.png_writer import OrderedPngWriter
    w = OrderedPngWriter(workers=2)
    w.submit(0, tmp_path / "missing_dir" / "a.png", np.zeros((2, 2), np.uint8))
    with pytest.raises(OSError):
        w.close()


# ------------------------------------------------------------------ 3. arguments and early refusals
def test_reference_flags_and_defaults():
    from unet_amd.predict_cli import get_args
    a = get_args(["-m", "w.pth", "-i", "x.png"])
    assert (a.model, a.input, a.output, a.viz, a.no_save, a.postprocess) == ("w.pth", "x.png", None, False, False, True)
    assert (a.arch, a.classes, a.bilinear, a.amp, a.batch_size, a.workers) == ("UNet", 3, False, True, 8, 8)
    b = get_args(["--model", "w.pth", "--input", "d", "--output", "o", "--viz", "--no-save", "--postprocess"])
    assert (b.output, b.viz, b.no_save, b.postprocess) == ("o", True, True, True)
    c = get_args(["-m", "w.pth", "-i", "d", "-o", "o", "-v", "-n", "-p", "--no-postprocess", "--arch", "UNet_SA", "-c", "4",
                  "--bilinear", "--no-amp", "-b", "3", "--workers", "2"])
    assert (c.postprocess, c.arch, c.classes, c.bilinear, c.amp, c.batch_size, c.workers) == (False, "UNet_SA", 4, True, False, 3, 2)
    for bad in ([], ["-m", "w.pth"], ["-i", "x.png"], ["-m", "w.pth", "-i", "x", "--arch", "VGG"]):
        with pytest.raises(SystemExit) as e:
            get_args(bad)
        assert e.value.code == 2


def _png(path):
    Image.fromarray(np.zeros((8, 8), np.uint8)).save(path)
    return str(path)


def test_refusals_before_the_device(tmp_path, caplog, monkeypatch):
    import torch
    import unet_amd
    from unet_amd.predict_cli import main
    img = _png(tmp_path / "x.png")
    with caplog.at_level(logging.ERROR):
        assert main(["-m", "model.pt", "-i", img]) == 1
        assert "TorchScript" in caplog.text and "model.pt" in caplog.text
        caplog.clear()
        assert main(["-m", "model.onnx", "-i", img]) == 1
        assert "Unsupported model format" in caplog.text and "model.onnx" in caplog.text
        caplog.clear()
        assert main(["-m", "w.pth", "-i", str(tmp_path / "nope.png")]) == 1
        assert "does not exist" in caplog.text
        caplog.clear()
        empty = tmp_path / "empty"
        empty.mkdir()
        (empty / "readme.txt").write_text("no image here")
        assert main(["-m", "w.pth", "-i", str(empty)]) == 1
        assert "No image file" in caplog.text
        caplog.clear()
        assert main(["-m", str(tmp_path / "absent.pth"), "-i", img]) == 1
        assert "Failed to load the model" in caplog.text
        caplog.clear()
        wrong = unet_amd.save_checkpoint(unet_amd.UNet_T(1, 3), str(tmp_path / "t.pth"), mask_values=[0, 1, 2])
        assert main(["-m", wrong, "-i", img]) == 1                    # a UNet_T checkpoint into the default UNet
        assert "Failed to load the model" in caplog.text
        caplog.clear()
        assert main(["-m", wrong, "-i", img, "--arch", "UNet_T", "-c", "1"]) == 1
        assert "evaluate" in caplog.text
        caplog.clear()
        # --viz where matplotlib cannot be imported: said so, exit 1, before the model is even read
        monkeypatch.setitem(sys.modules, "matplotlib", None)
        monkeypatch.setitem(sys.modules, "matplotlib.pyplot", None)
        assert main(["-m", str(tmp_path / "absent.pth"), "-i", img, "--viz"]) == 1
        assert "matplotlib" in caplog.text and "Failed to load" not in caplog.text
        caplog.clear()
        monkeypatch.delitem(sys.modules, "matplotlib")
        monkeypatch.delitem(sys.modules, "matplotlib.pyplot")
        if not torch.cuda.is_available():                              # everything checks out, then: no device, status 2
            assert main(["-m", wrong, "-i", img, "--arch", "UNet_T"]) == 2
            assert "no GPU" in caplog.text
    assert np.asarray(Image.open(img)).max() == 0                      # nothing was written over the input


def test_checkpoint_mask_values_are_dropped(tmp_path):
    import torch
    import unet_amd
    m = unet_amd.UNet_T(1, 3)
    path = unet_amd.save_checkpoint(m, str(tmp_path / "w.pth"), mask_values=[0, 128, 255])
    assert "mask_values" in torch.load(path, map_location="cpu", weights_only=True)
    assert unet_amd.load_checkpoint(unet_amd.UNet_T(1, 3), path) == [0, 128, 255]       # popped, then load_state_dict succeeds


def test_predict_module_hooks_the_cli():
    import unet_amd
    from unet_amd import predict, predict_cli
    assert predict.main.__doc__ and "predict_cli" in predict.main.__doc__
    assert callable(predict_cli.main) and unet_amd.BatchPredictor is predict.BatchPredictor
    with pytest.raises(ValueError, match="evaluate"):
        unet_amd.BatchPredictor(unet_amd.UNet_T(1, 1, True))
    with pytest.raises(ValueError):
        unet_amd.BatchPredictor(unet_amd.UNet_T(1, 3, True), batch=0)
    from unet_amd.train_cli import get_args
    assert get_args([]).pred_dir is None and get_args(["--pred-dir", "p"]).pred_dir == "p"


# ------------------------------------------------------------------ 4. the C ABI
def test_predict_io_symbols_exported_and_arguments_checked():
    import unet_amd  # noqa: F401
    from unet_amd._lib import LIB, LIB_PATH
    dll = ctypes.CDLL(LIB_PATH)
    for name in ("uh_predict_prepare_u8", "uh_logits_to_classes_u8", "uh_classes_to_grey_u8"):
        assert hasattr(dll, name), f"{name} is not exported"
        assert name in LIB.protos
    LIB.load()
    p = 4096                                                           # a non-null pointer that is never dereferenced
    with pytest.raises(RuntimeError, match="uh_predict_prepare_u8.*null pointer"):
        LIB.call("uh_predict_prepare_u8", None, p, p, 1, 8, 8, None)
    with pytest.raises(RuntimeError, match="uh_predict_prepare_u8.*null pointer"):
        LIB.call("uh_predict_prepare_u8", p, p, None, 1, 8, 8, None)
    for B, H, W in ((0, 8, 8), (1, -8, 8), (1, 8, -1)):
        with pytest.raises(RuntimeError, match="uh_predict_prepare_u8.*bad sizes"):
            LIB.call("uh_predict_prepare_u8", p, p, p, B, H, W, None)
    with pytest.raises(RuntimeError, match="uh_logits_to_classes_u8.*null pointer"):
        LIB.call("uh_logits_to_classes_u8", None, 64, 3, 0, p, None)
    with pytest.raises(RuntimeError, match="uh_logits_to_classes_u8.*null pointer"):
        LIB.call("uh_logits_to_classes_u8", p, 64, 3, 0, None, None)
    with pytest.raises(RuntimeError, match="uh_logits_to_classes_u8.*bad sizes"):
        LIB.call("uh_logits_to_classes_u8", p, -64, 3, 0, p, None)
    with pytest.raises(RuntimeError, match="uh_logits_to_classes_u8.*bad sizes"):
        LIB.call("uh_logits_to_classes_u8", p, 64, 0, 0, p, None)
    with pytest.raises(RuntimeError, match="uh_logits_to_classes_u8.*dtype"):
        LIB.call("uh_logits_to_classes_u8", p, 64, 3, 7, p, None)
    with pytest.raises(RuntimeError, match="uh_classes_to_grey_u8.*null pointer"):
        LIB.call("uh_classes_to_grey_u8", p, p, None, 64, None)
    with pytest.raises(RuntimeError, match="uh_classes_to_grey_u8.*bad size"):
        LIB.call("uh_classes_to_grey_u8", p, p, p, -1, None)
