"""`python -m unet_amd.predict`, BatchPredictor and evaluate's PNG dumps on the MI355X: the three byte stages of
csrc/predict_io.hip against numpy / torch over every code, BatchPredictor against the one-image composition
mask_to_image(postprocess_mask(predict_img(...))) on mixed sizes and batch lengths, the command line as a subprocess,
and evaluate(epoch_pred_dir=...) / train --pred-dir against the restatements of tests/predict_ref.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import predict_ref as R  # noqa: E402
from conftest import ROOT  # noqa: E402

pytestmark = pytest.mark.gpu
SIZES = [(512, 512), (384, 512), (999, 1000), (700, 300)]              # (H, W): 512x512, 512x384, 1000x999, 300x700


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


# ------------------------------------------------------------------ item 5: uh_predict_prepare_u8
def _prepare_ref(img):
    """data_loading.py:86-87 + predict.py:20 for one decoded grey image."""
    a = img[np.newaxis, ...]
    if (a > 1).any():
        a = a.astype(np.float32) / 255.0
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.float32).numpy()


@pytest.mark.parametrize("H,W", [(70, 90), (1, 1), (999, 1000), (16, 16), (3, 5)])
def test_prepare_is_numpy_bit_for_bit_and_per_image(H, W):
    from unet_amd import ops
    dev = _dev()
    rng = np.random.default_rng(H * 1000 + W)
    n = H * W
    ordinary = (np.arange(n) % 256).astype(np.uint8)                   # every code where the image is large enough
    rng.shuffle(ordinary)
    if n == 1:
        ordinary[0] = 37
    zeros = np.zeros(n, np.uint8)
    binary = rng.integers(0, 2, n, dtype=np.uint8)
    binary[n // 2] = 1                                                 # 0/1 only: NOT divided
    one_two = rng.integers(0, 2, n, dtype=np.uint8)
    one_two[n - 1] = 2                                                 # a single 2, in the last byte: divided
    batch = np.stack([ordinary, zeros, binary, one_two, binary, ordinary]).reshape(6, H, W)
    got = ops.predict_prepare_u8(torch.from_numpy(batch).to(dev))
    assert got.shape == (6, 1, H, W) and got.dtype == torch.float32
    got = got.cpu().numpy()
    for b in range(6):
        want = _prepare_ref(batch[b])
        assert got[b].tobytes() == want.tobytes(), f"image {b}"
    assert got[2].max() == 1.0 and got[3].max() == np.float32(2) / np.float32(255)
    if n >= 256:
        codes = np.arange(256, dtype=np.uint8)
        assert np.array_equal(np.unique(got[0]), codes.astype(np.float32) / np.float32(255.0))


def test_prepare_unaligned_views():
    """A batch that starts at an odd byte takes the scalar path: same bytes."""
    from unet_amd._lib import LIB
    dev = _dev()
    rng = np.random.default_rng(5)
    H, W, B = 33, 47, 3
    base = torch.from_numpy(rng.integers(0, 256, B * H * W + 3, dtype=np.uint8)).to(dev)
    img = base[3:]
    out = torch.empty(B * H * W + 1, dtype=torch.float32, device=dev)
    flags = torch.empty(B, dtype=torch.int32, device=dev)
    LIB.call("uh_predict_prepare_u8", img.data_ptr(), out[1:].data_ptr(), flags.data_ptr(), B, H, W,
             torch.cuda.current_stream().cuda_stream)
    want = img.cpu().numpy().astype(np.float32) / 255.0
    assert out[1:].cpu().numpy().tobytes() == want.tobytes()


# ------------------------------------------------------------------ item 6: classes and grey
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [2, 3, 4, 6])
@pytest.mark.parametrize("B,H,W", [(2, 37, 53), (1, 1, 1), (3, 64, 64), (1, 5, 3)])
def test_logits_to_classes_equals_torch_argmax(dtype, C, B, H, W):
    from unet_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(C * 100 + H)
    nhwc = torch.randn(B, H, W, C, generator=g)
    flat = nhwc.view(-1, C)
    n = flat.shape[0]
    for p in range(0, n, 3):                                           # planted ties, every pair of classes in turn
        a, b = p % C, (p // 3 + 1) % C
        flat[p, a] = flat[p, b] = flat[p].max() + (p % 2)
    for p in range(1, n, 7):                                           # planted NaNs: one, several, all
        flat[p, p % C] = float("nan")
        if p % 2:
            flat[p, (p + 1) % C] = float("nan")
    if n > 4:
        flat[4, :] = float("nan")
    nhwc = nhwc.to(dtype)
    want = torch.argmax(nhwc.permute(0, 3, 1, 2), dim=1).to(torch.uint8)
    for logits in (nhwc.to(dev).permute(0, 3, 1, 2),                   # the head's layout: NHWC memory, NCHW shape
                   nhwc.permute(0, 3, 1, 2).contiguous().to(dev)):     # NCHW memory
        got = ops.logits_to_classes_u8(logits)
        assert got.dtype == torch.uint8 and got.shape == (B, H, W)
        assert torch.equal(got.cpu(), want)
    if dtype == torch.float32:
        assert torch.equal(ops.argmax_classes(nhwc.to(dev).permute(0, 3, 1, 2)).cpu().to(torch.uint8), want)


@pytest.mark.parametrize("fn", [R.grey_classes_ref, R.grey_postprocessed_ref, R.grey_binary_ref])
def test_classes_to_grey_all_codes_in_and_out_of_place(fn):
    from unet_amd import ops, predict
    dev = _dev()
    table = {R.grey_classes_ref: predict.GREY_CLASSES, R.grey_postprocessed_ref: predict.GREY_POSTPROCESSED,
             R.grey_binary_ref: predict.GREY_BINARY}[fn]
    lut = torch.from_numpy(table.copy()).to(dev)
    rng = np.random.default_rng(1)
    for n in (256, 100003, 5, 4096):
        codes = rng.integers(0, 256, n, dtype=np.uint8)
        codes[:min(n, 256)] = np.arange(min(n, 256))
        want = fn(codes)
        t = torch.from_numpy(codes).to(dev)
        out = ops.classes_to_grey_u8(t, lut)
        assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(t.cpu().numpy(), codes)
        view = t[1:].contiguous() if n < 10 else t[1:]                 # an unaligned start: the scalar path
        assert np.array_equal(ops.classes_to_grey_u8(view, lut).cpu().numpy(), want[1:])
        assert ops.classes_to_grey_u8(t, lut, out=t) is t              # in place
        assert np.array_equal(t.cpu().numpy(), want)


# ------------------------------------------------------------------ item 7: BatchPredictor
def _phantom(rng, H, W):
    """8-bit CT-like slice: dark noisy air, an elliptic body, a bright inner region."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    img = rng.normal(20, 6, (H, W))
    cx, cy = W * rng.uniform(0.4, 0.6), H * rng.uniform(0.4, 0.6)
    rx, ry = W * rng.uniform(0.3, 0.4), H * rng.uniform(0.3, 0.4)
    body = ((xx - cx) / rx) ** 2 + ((yy - cy) / ry) ** 2 < 1
    img[body] = 110 + rng.normal(0, 8, int(body.sum()))
    img[((xx - cx) / (rx / 3)) ** 2 + ((yy - cy - ry / 3) / (ry / 4)) ** 2 < 1] += 90
    return np.clip(img, 0, 255).astype(np.uint8)


def _mixed_images(seed, counts=(9, 5, 3, 8)):
    rng = np.random.default_rng(seed)
    imgs = [_phantom(rng, H, W) for (H, W), n in zip(SIZES, counts) for _ in range(n)]
    order = rng.permutation(len(imgs))
    return [imgs[i] for i in order]


class _IntensityStub(torch.nn.Module):
    """Logits that follow the input's intensity: class 2 where the pixel is bright, 1 in between, 0 for air."""
    n_channels, n_classes = 1, 3

    def forward(self, x):
        return torch.cat([0.2 - x, 0.15 - (x - 0.2).abs(), x - 0.3], dim=1) * 8.0


def _randomize_bn(model, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
                m.weight.copy_(torch.rand(m.num_features, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.num_features, generator=g) * 0.1)


def _balance_head(model, img, dev):
    """A randomly initialised network tends to put one class on top everywhere; moving the head's bias by the mean logit of
    each class on one image makes the three classes compete, so that the class maps compared below are not constant."""
    x = torch.from_numpy(img.astype(np.float32) / 255.0)[None, None].to(dev)
    with torch.no_grad():
        y = model(x).float()
        if y.shape[1] == 1:
            # binary head: the middle of the logit range, not the mean -- the mean sits on the flat background and leaves its
            # logits within 1e-7 of zero, where fp32 sigmoid(x) > 0.5 (evaluate.py:60-62) and x > 0 (uh_threshold_mask) part
            centre = (y.amax(dim=(0, 2, 3)) + y.amin(dim=(0, 2, 3))) / 2
        else:
            centre = y.mean(dim=(0, 2, 3))
        model.outc.conv.bias.sub_(centre)


def _alone(model, img, dev, postprocess=True):
    import unet_amd
    cls = unet_amd.predict_img(model, img, dev)
    if postprocess:
        cls = unet_amd.postprocess_mask(cls)
    return np.asarray(unet_amd.mask_to_image(cls))


def _check_predictor(model, images, dev, postprocess=True, batches=(8, 1, 3), graphs=True):
    import unet_amd
    want = [_alone(model, im, dev, postprocess) for im in images]
    for batch in batches:
        p = unet_amd.BatchPredictor(model, batch=batch, postprocess=postprocess)
        got = p(images)
        assert len(got) == len(images)
        for i, (g, w) in enumerate(zip(got, want)):
            assert g.dtype == np.uint8 and g.shape == images[i].shape
            np.testing.assert_array_equal(g, w, err_msg=f"batch={batch} image {i} {images[i].shape}")
        again = p(images)                                              # graphs are captured by now
        for g, w in zip(again, want):
            np.testing.assert_array_equal(g, w)
        if graphs:                                                     # the list holds full batches of a repeated size
            assert p.graph_replays > 0 and len(p._graphs) <= p.MAX_GRAPHS
    return want


def test_batch_predictor_stub_model_masks_are_not_empty():
    import unet_amd
    dev = _dev()
    images = _mixed_images(3)
    model = _IntensityStub().to(dev)
    want = _check_predictor(model, images, dev)
    assert all((w == 255).sum() >= 15000 for w in want), "post-processed masks must not be empty"
    assert all(set(np.unique(w)) <= {0, 255} for w in want)
    raw = _check_predictor(model, images, dev, postprocess=False, batches=(8,))
    assert all(set(np.unique(w)) == {0, 128, 255} for w in raw)
    p = unet_amd.BatchPredictor(model, batch=8)
    cls = p.classes(images[:5])
    for c, im in zip(cls, images[:5]):
        np.testing.assert_array_equal(c, unet_amd.postprocess_mask(unet_amd.predict_img(model, im, dev)))
    pil = p([Image.fromarray(im) for im in images[:3]])                # PIL "L" images are taken too
    for a, w in zip(pil, want[:3]):
        np.testing.assert_array_equal(a, w)


@pytest.mark.parametrize("arch,bilinear", [("UNet_S", False), ("UNet_S", True), ("UNet_SA", False)])
def test_batch_predictor_equals_one_image_composition(arch, bilinear):
    import unet_amd
    dev = _dev()
    torch.manual_seed(7)
    model = getattr(unet_amd, arch)(1, 3, bilinear=bilinear)
    _randomize_bn(model, 21)
    model = model.to(dev).eval()
    images = _mixed_images(11)
    _balance_head(model, images[0], dev)
    want = _check_predictor(model, images, dev, postprocess=False)
    assert all(len(np.unique(w)) == 3 for w in want), "a constant prediction compares nothing"
    _check_predictor(model, images[:12], dev, postprocess=True, batches=(8, 3), graphs=False)


def test_batch_predictor_keeps_few_graphs_and_refuses_binary_heads():
    import unet_amd
    dev = _dev()
    model = _IntensityStub().to(dev)
    p = unet_amd.BatchPredictor(model, batch=1, postprocess=False)
    rng = np.random.default_rng(0)
    sizes = [(40 + 8 * k, 64) for k in range(7)]
    images = [rng.integers(0, 256, s, dtype=np.uint8) for s in sizes] * 3
    got = p(images)
    assert len(p._graphs) == p.MAX_GRAPHS and p.graph_replays >= 7
    for g, im in zip(got, images):
        np.testing.assert_array_equal(g, _alone(model, im, dev, postprocess=False))
    with pytest.raises(ValueError, match="evaluate"):
        unet_amd.BatchPredictor(unet_amd.UNet_T(1, 1, True))


# ------------------------------------------------------------------ item 8: the command line
def _cli(args, cwd, timeout=300):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, "-m", "unet_amd.predict"] + args, capture_output=True, text=True, timeout=timeout,
                          cwd=str(cwd), env=env)


def _tree(root, seed):
    """Mixed sizes, a sub-directory with a duplicate stem, a .jpg, an upper-case suffix and one truncated file."""
    rng = np.random.default_rng(seed)
    files = {"a.png": (96, 128), "b.png": (96, 128), "c.PNG": (80, 80), "photo.jpg": (64, 112), "sub/a.png": (80, 80),
             "sub/deep/d.jpeg": (96, 128), "e.png": (70, 90)}
    for rel, (H, W) in files.items():
        os.makedirs(os.path.dirname(os.path.join(root, rel)), exist_ok=True)
        Image.fromarray(_phantom(rng, H, W)).save(os.path.join(root, rel))
    with open(os.path.join(root, "broken.png"), "wb") as f:
        f.write(open(os.path.join(root, "a.png"), "rb").read()[:60])
    with open(os.path.join(root, "notes.txt"), "w") as f:
        f.write("not an image")
    return files


def _model_file(tmp_path, arch="UNet_T"):
    import unet_amd
    torch.manual_seed(5)
    model = getattr(unet_amd, arch)(1, 3, bilinear=False)
    _randomize_bn(model, 9)
    dev = torch.device("cuda:0")
    _balance_head(model.to(dev).eval(), _phantom(np.random.default_rng(1), 96, 128), dev)     # class maps that are not constant
    model = model.cpu()
    path = unet_amd.save_checkpoint(model, str(tmp_path / "w.pth"), mask_values=[0, 128, 255])
    return model, path


def test_cli_on_a_tree(tmp_path):
    dev = _dev()
    model, wpath = _model_file(tmp_path)
    model = model.to(dev).eval()
    src = tmp_path / "in"
    _tree(str(src), 2)
    out = tmp_path / "out"
    common = ["-m", wpath, "--arch", "UNet_T", "-b", "2", "--workers", "3", "--no-postprocess"]
    r = _cli(common + ["-i", str(src), "-o", str(out)], tmp_path)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "broken.png" in r.stderr and "notes.txt" not in r.stderr
    found = R.walk_ref(str(src))
    assert len(found) == 8
    winners = {}
    for f in found:                                                    # the later file in discovery order wins a shared stem
        if not f.endswith("broken.png"):
            winners[R.output_path_ref(str(out), f)] = f
    assert sorted(os.listdir(out)) == sorted(os.path.basename(p) for p in winners)
    assert len(winners) == 6                                           # a.png and sub/a.png share one
    nonconstant = 0
    for path, f in winners.items():
        want = _alone(model, np.asarray(Image.open(f).convert("L")), dev, postprocess=False)
        got = np.asarray(Image.open(path))
        np.testing.assert_array_equal(got, want, err_msg=f)
        nonconstant += len(np.unique(want)) > 1
    assert nonconstant > 0
    # --no-save writes nothing
    before = sorted(os.listdir(out))
    out2 = tmp_path / "out2"
    r = _cli(common + ["-i", str(src), "-o", str(out2), "-n"], tmp_path)
    assert r.returncode == 0, r.stderr[-4000:]
    assert not out2.exists() and sorted(os.listdir(out)) == before
    # without -o the mask lands beside the input (and a PNG input is overwritten by its mask)
    single = tmp_path / "single"
    single.mkdir()
    jpg = np.asarray(Image.open(src / "photo.jpg").convert("L"))
    Image.open(src / "photo.jpg").save(single / "photo.jpg")
    png_in = np.asarray(Image.open(src / "e.png"))
    Image.fromarray(png_in).save(single / "e.png")
    r = _cli(common + ["-i", str(single)], tmp_path)
    assert r.returncode == 0, r.stderr[-4000:]
    assert sorted(os.listdir(single)) == ["e.png", "photo.jpg", "photo.png"]
    jpg = np.asarray(Image.open(single / "photo.jpg").convert("L"))
    np.testing.assert_array_equal(np.asarray(Image.open(single / "photo.png")), _alone(model, jpg, dev, postprocess=False))
    np.testing.assert_array_equal(np.asarray(Image.open(single / "e.png")), _alone(model, png_in, dev, postprocess=False))


def test_cli_default_flags_postprocess_a_single_file(tmp_path):
    """The defaults: UNet(1, 3, bilinear=False), post-processing on, batch 8; one file given by name."""
    import unet_amd
    dev = _dev()
    torch.manual_seed(2)
    model = unet_amd.UNet(1, 3, bilinear=False)
    wpath = unet_amd.save_checkpoint(model, str(tmp_path / "w.pth"), mask_values=[0, 128, 255])
    rng = np.random.default_rng(8)
    img = _phantom(rng, 200, 232)
    Image.fromarray(img).save(tmp_path / "scan.png")
    out = tmp_path / "o"
    r = _cli(["-m", wpath, "-i", str(tmp_path / "scan.png"), "-o", str(out)], tmp_path)
    assert r.returncode == 0, r.stderr[-4000:]
    want = _alone(model.to(dev).eval(), img, dev, postprocess=True)
    np.testing.assert_array_equal(np.asarray(Image.open(out / "scan.png")), want)


# ------------------------------------------------------------------ item 9: evaluate(epoch_pred_dir=...) and train --pred-dir
def _read_tree(root):
    files = {}
    for d, _, names in os.walk(root):
        for n in names:
            p = os.path.join(d, n)
            files[os.path.relpath(p, root)] = np.asarray(Image.open(p))
    return files


@pytest.mark.parametrize("classes,postprocess", [(3, True), (1, True), (3, False), (1, False)])
def test_evaluate_writes_the_reference_files(tmp_path, classes, postprocess):
    import unet_amd
    dev = _dev()
    torch.manual_seed(classes)
    model = unet_amd.UNet_T(1, classes, bilinear=True)
    _randomize_bn(model, 4)
    model = model.to(dev)
    imgs, masks = unet_amd.ellipse_batch(6, 160, seed=3)
    _balance_head(model.eval(), (imgs[0, 0].numpy() * 255).astype(np.uint8), dev)          # predictions that are not constant
    batches = [{"image": imgs[s:s + 2], "mask": masks[s:s + 2]} for s in (0, 2, 4)]
    plain = unet_amd.evaluate(model, batches, dev, True, None, postprocess)
    dumped = unet_amd.evaluate(model, batches, dev, True, str(tmp_path / "pred"), postprocess)
    for a, b in zip(plain, dumped):
        assert torch.equal(a, b)
    raw, post = [], []
    model.eval()
    for b in batches:
        x = b["image"].to(device=dev, dtype=torch.float32, memory_format=torch.channels_last)
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=True):
            logits = model(x).float().cpu()
        if classes == 1:
            r = (torch.sigmoid(logits.squeeze(1)) > 0.5).numpy().astype(np.uint8)                # evaluate.py:60-62
            p = [unet_amd.postprocess_mask(m * 255) // 255 for m in r]                           # evaluate.py:71-78
        else:
            r = logits.argmax(dim=1).numpy().astype(np.uint8)
            p = [unet_amd.postprocess_mask(m) for m in r]
        raw.append(r)
        post.append(p)
    want = R.evaluate_dump_ref(raw, post, classes, postprocess)
    got = _read_tree(str(tmp_path / "pred"))
    assert sorted(got) == sorted(want)
    assert len(got) == (12 if postprocess else 6) and "pred_batch1_sample0.png" in got and "pred_batch3_sample1.png" in got
    assert os.path.isdir(tmp_path / "pred" / "postprocessed") == postprocess
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    assert any(len(np.unique(v)) > 1 for v in want.values())


def test_train_pred_dir_writes_epochs_and_leaves_the_weights_alone(tmp_path):
    from test_gpu_train_cli import _png_tree, _run_cli
    _dev()
    data = tmp_path / "data"
    _png_tree(str(data), 3, 2, 128, seed=7)
    args = ["-e", "1", "-b", "2", "-s", "0.5", "-c", "3", "--seed", "0", "--model", "UNet_T", "--data-root", str(data),
            "--workers", "4"]
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir()
    b.mkdir()
    _run_cli(a, args)
    _run_cli(b, args + ["--pred-dir", str(b / "predictions")])
    assert not (a / "predictions").exists()
    ep = b / "predictions" / "epoch_1"
    names = sorted(n for n in os.listdir(ep) if n.endswith(".png"))
    # 8 validation items (2 files x 4 quarter turns), batch 2, drop_last: 4 batches of 2
    assert names == sorted(f"pred_batch{k}_sample{i}.png" for k in range(1, 5) for i in range(2))
    assert sorted(os.listdir(ep / "postprocessed")) == names
    for n in names:
        assert np.asarray(Image.open(ep / n)).shape == (64, 64)
        assert set(np.unique(np.asarray(Image.open(ep / "postprocessed" / n)))) <= {0, 255}
    sa = torch.load(a / "model_epoch1.pth", map_location="cpu", weights_only=True)
    sb = torch.load(b / "model_epoch1.pth", map_location="cpu", weights_only=True)
    assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
