"""Patch training on the MI355X (DESIGN.md section 3 "Patch training"), bit for bit against the numpy restatement
tests/crop_ref.py: uh_crop_select over mixed-size label planes, every rank of a plane, the border clamps; uh_crop_gather
against numpy slicing; DeviceBatchLoader(crop=...) against ds[i] sliced at the reference origin; `python -m unet_amd.train
--crop --tile` with --save-state / --resume as child processes.  No tolerances anywhere."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import crop_ref as R  # noqa: E402

from conftest import ROOT  # noqa: E402

pytestmark = pytest.mark.gpu

PLANES = ((16, 16), (17, 23), (37, 53), (64, 64), (100, 257), (300, 700))   # 300 x 700: 821 chunks, no multiple of 256 or 64
NEVER = np.array([0, 3, -1, 64, 255, 66], np.int64)                          # in neither mask; 66 = 64 + 2 must not wrap
ONE_BIT, TWO_BIT = 1 << 2, (1 << 1) | (1 << 2)
FULL = 0xFFFFFFFF
WORDS = np.array([[0, 0, 0, 0], [FULL, FULL, FULL, FULL], [(1 << 31) - 1, FULL, 0, FULL], [1 << 31, 0, FULL, 0],
                  [0x12345678, 0x9ABCDEF0, 0x0F1E2D3C, 0xC3D2E1F0], [7, 0x80000000, 0x7FFFFFFF, 0x80000001]], np.uint32)


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _variants(rng, H, W):
    """The label planes of one size: n = 0, n = 1 at the first and at the last pixel, n = H W, a sparse random set (values 1
    and 2: the one-bit mask counts fewer than the two-bit one).  Everything else holds values that never count."""
    back = lambda: NEVER[rng.integers(0, NEVER.size, (H, W))]
    none, first, last, sparse = back(), back(), back(), back()
    first[0, 0] = 2
    last[H - 1, W - 1] = 2
    hit = rng.random((H, W)) < 0.01
    hit[rng.integers(0, H), rng.integers(0, W)] = True
    sparse[hit] = rng.integers(1, 3, int(hit.sum()))
    return [none, first, last, np.full((H, W), 2, np.int64), sparse]


@pytest.fixture(scope="module")
def planes():
    rng = np.random.default_rng(20)
    host = [v for H, W in PLANES for v in _variants(rng, H, W)]
    return host, [torch.from_numpy(v).to(_dev()) for v in host]


@pytest.mark.parametrize("mask", [ONE_BIT, TWO_BIT])
@pytest.mark.parametrize("threshold", [0, 1 << 31, 1 << 32])
def test_select_matches_the_reference_on_mixed_sizes(planes, mask, threshold):
    from unet_amd import ops
    host, dev = planes
    rows = [(p, w) for p in range(len(host)) for w in range(len(WORDS))]       # 30 planes x 6 word rows in ONE call
    words = np.stack([WORDS[w] for _, w in rows])
    origins, counts = ops.crop_select([dev[p] for p, _ in rows], words, 16, mask, threshold)
    origins, counts = origins.cpu().numpy(), counts.cpu().numpy()
    branches = set()
    for i, (p, w) in enumerate(rows):
        oy, ox, n, picked = R.select(host[p], WORDS[w], 16, mask, threshold)
        assert (int(origins[i, 0]), int(origins[i, 1]), int(counts[i])) == (oy, ox, n), (host[p].shape, p % 5, w)
        branches.add(picked is not None)
    assert branches == ({False} if threshold == 0 else {False, True})


def test_select_finds_every_rank():
    """One 24 x 40 plane, B = n rows aliasing it, r1 = ceil(k 2^32 / n): row k lands on foreground pixel k.  The pixels lie where
    no border clamps (py <= 8, px <= 24 for size 16) and r2 = r3 = 0, so the origin IS the pixel."""
    from unet_amd import ops
    rng = np.random.default_rng(21)
    lab = np.zeros((24, 40), np.int64)
    at = rng.choice(9 * 25, 50, replace=False)
    lab[at // 25, at % 25] = 2
    fg = np.flatnonzero(lab.reshape(-1) == 2)
    n = int(fg.size)
    assert n == 50
    words = np.zeros((n, 4), np.uint32)
    words[:, 1] = [-((-k << 32) // n) for k in range(n)]
    d = torch.from_numpy(lab).to(_dev())
    origins, counts = ops.crop_select([d] * n, words, 16, ONE_BIT, 1 << 32)
    origins = origins.cpu().numpy()
    assert np.array_equal(counts.cpu().numpy(), np.full(n, n))
    for k in range(n):
        assert (int(origins[k, 0]), int(origins[k, 1])) == divmod(int(fg[k]), 40), k
        assert R.select(lab, words[k], 16, ONE_BIT, 1 << 32)[3] == divmod(int(fg[k]), 40)
    words[1:, 1] -= 1                                                             # one below the first word of rank k: rank k - 1
    origins = ops.crop_select([d] * n, words, 16, ONE_BIT, 1 << 32)[0].cpu().numpy()
    for k in range(1, n):
        assert (int(origins[k, 0]), int(origins[k, 1])) == divmod(int(fg[k - 1]), 40), k


def test_select_clamps_at_the_borders():
    from unet_amd import ops
    H, W, size = 40, 56, 32
    corners = ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1))
    host = []
    for py, px in corners:
        lab = np.ones((H, W), np.int64)
        lab[py, px] = 2
        host.append(lab)
    dev = [torch.from_numpy(v).to(_dev()) for v in host]
    jitter = ((0, 0), (FULL, FULL), (0, FULL), (FULL, 0))
    rows = [(c, j) for c in range(4) for j in range(4)]
    words = np.array([[0, 0, jitter[j][0], jitter[j][1]] for _, j in rows], np.uint32)
    origins = ops.crop_select([dev[c] for c, _ in rows], words, size, ONE_BIT, 1 << 32)[0].cpu().numpy()
    for i, (c, j) in enumerate(rows):
        oy, ox, n, picked = R.select(host[c], words[i], size, ONE_BIT, 1 << 32)
        assert n == 1 and picked == corners[c]
        assert (int(origins[i, 0]), int(origins[i, 1])) == (oy, ox), (corners[c], jitter[j])
        assert 0 <= oy <= H - size and 0 <= ox <= W - size and oy <= corners[c][0] < oy + size and ox <= corners[c][1] < ox + size
    assert {tuple(o) for o in origins.tolist()} == {(0, 0), (0, W - size), (H - size, 0), (H - size, W - size)}


# -------------------------------------------------------------------------------------------------------------- gather
def _bytes(t):
    t = t.contiguous().cpu()
    return (t.view(torch.int16) if t.dtype == torch.bfloat16 else t).numpy().tobytes()


GATHER_SIZES = ((16, 16), (17, 23), (37, 53), (40, 56), (33, 70))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("size,pad_in,pad_out", [(16, 0, 0), (16, 1, 0), (16, 0, 1), (32, 0, 0), (32, 2, 1)])
def test_gather_matches_numpy_slicing(dtype, C, size, pad_in, pad_out):
    """Origins: 0, the largest, odd ox, and out of range on every side (equal to their clamp).  pad_in / pad_out: the pixel
    strides ld_in = C + pad_in, ld_out = C + pad_out."""
    from unet_amd import ops
    g = torch.Generator().manual_seed(22)
    shapes = [s for s in GATHER_SIZES if min(s) >= size]
    asked = ((0, 0), (10 ** 6, 10 ** 6), (1, 3), (-5, 10 ** 6), (10 ** 6, -1), (0, 1), (2, 5))
    images, labels, origin, want = [], [], [], []
    for i, (H, W) in enumerate(shapes * 2):
        wide = torch.randn(H, W, C + pad_in, generator=g).to(dtype).to(_dev())
        images.append(wide[..., :C].permute(2, 0, 1))                            # [C,H,W], pixel stride C + pad_in
        labels.append(torch.randint(-3, 70, (H, W), generator=g).to(_dev()))
        origin.append(asked[i % len(asked)])
        want.append((min(max(origin[-1][0], 0), H - size), min(max(origin[-1][1], 0), W - size)))
    assert any(w[1] % 2 for w in want)
    o = torch.tensor(origin, dtype=torch.int32, device=_dev())
    image, mask = ops.crop_gather(images, labels, o, size, ld_out=C + pad_out)
    assert image.shape == (len(images), C, size, size) and image.dtype == dtype and mask.shape == (len(images), size, size)
    assert image.permute(0, 2, 3, 1).stride() == (size * size * (C + pad_out), size * (C + pad_out), C + pad_out, 1)
    for b, (oy, ox) in enumerate(want):
        ri, rl = R.crop(images[b], labels[b], oy, ox, size)
        assert _bytes(image[b]) == _bytes(ri), (b, shapes[b % len(shapes)], origin[b])
        assert _bytes(mask[b]) == _bytes(rl), (b, shapes[b % len(shapes)], origin[b])
    only_image, none = ops.crop_gather(images, None, o, size, ld_out=C + pad_out)
    assert none is None and _bytes(only_image) == _bytes(image)
    none, only_mask = ops.crop_gather(None, labels, o, size)
    assert none is None and _bytes(only_mask) == _bytes(mask)


# -------------------------------------------------------------------------------------------------------------- loader
FILE_SIZES = ((40, 56), (64, 48), (33, 70), (48, 48), (56, 40), (70, 36))           # H x W of the six training files


def _write_pair(root, split, name, H, W, rng, contour=True):
    for d in ("imgs", "masks"):
        os.makedirs(os.path.join(root, d, split), exist_ok=True)
    Image.fromarray(rng.integers(2, 256, (H, W)).astype(np.uint8)).save(os.path.join(root, "imgs", split, name + ".png"))
    grey = np.where(rng.random((H, W)) < 0.5, 0, 128).astype(np.uint8)
    if contour:                                                                      # a thin class-2 line: under 3 % of the pixels
        grey[rng.integers(0, H), W // 4: W // 2] = 255
    Image.fromarray(grey).save(os.path.join(root, "masks", split, name + "_mask.png"))


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("crop_data"))
    rng = np.random.default_rng(23)
    for i, (H, W) in enumerate(FILE_SIZES):
        _write_pair(root, "train", f"t{i}", H, W, rng, contour=i != 3)               # one file without foreground: n = 0
    for i in range(2):
        _write_pair(root, "val", f"v{i}", 48, 48, rng)
    return root


def _train_set(folder, scale, augment=True):
    from unet_amd import BasicDataset
    return BasicDataset(os.path.join(folder, "imgs", "train"), os.path.join(folder, "masks", "train"), scale, augment=augment)


def _serve(loader, epochs):
    """{(epoch, index): (image, mask)} on the host, and the batches as served."""
    out, served = {}, []
    for e in range(epochs):
        batches = list(loader)
        for idx, batch in zip(loader.batches_of(loader.orders[e]), batches):
            assert batch["image"].shape[0] == len(idx) == batch["mask"].shape[0]
            for j, i in enumerate(idx):
                assert (e, i) not in out
                out[(e, i)] = (batch["image"][j].cpu(), batch["mask"][j].cpu())
            served.append((e, idx, batch))
    return out, served


@pytest.mark.parametrize("scale,size", [(1.0, 32), (0.5, 16)])
def test_loader_crops_equal_sliced_items(folder, scale, size):
    from unet_amd import BatchCrop
    from unet_amd.utils.data_loading import DeviceBatchLoader
    ds = _train_set(folder, scale)
    items = [ds[i] for i in range(len(ds))]
    assert len(items) == 24 and len({tuple(it["mask"].shape) for it in items}) > 4
    crop = BatchCrop(f"{size},fg=0.75", seed=5, n_classes=3)
    one, _ = _serve(DeviceBatchLoader(ds, 1, shuffle=True, seed=100, workers=4, crop=crop), 2)
    three, _ = _serve(DeviceBatchLoader(ds, 3, shuffle=True, seed=200, workers=4, crop=crop), 2)
    branches, origins = set(), {}
    for e in range(2):
        words = R.words(5, e, range(len(ds)))
        for i, it in enumerate(items):
            oy, ox, n, picked = R.select(it["mask"].numpy(), words[i], size, 1 << 2, R.threshold(0.75))
            ri, rl = R.crop(it["image"], it["mask"], oy, ox, size)
            for got in (one[(e, i)], three[(e, i)]):
                assert got[0].dtype == torch.float32 and got[1].dtype == torch.int64
                assert _bytes(got[0]) == _bytes(ri) and _bytes(got[1]) == _bytes(rl), (e, i, oy, ox)
            branches.add(picked is not None)
            origins[(e, i)] = (oy, ox)
    assert branches == {False, True}
    assert sum(origins[(0, i)] != origins[(1, i)] for i in range(len(ds))) > len(ds) // 2       # two epochs differ
    assert crop.last_origins.dtype == torch.int32 and crop.last_origins.is_cuda and crop.last_origins.shape[1] == 2


def test_loader_crops_then_augments(folder):
    from unet_amd import BatchAugment, BatchCrop
    from unet_amd.utils.data_loading import DeviceBatchLoader
    ds = _train_set(folder, 1.0)
    crop, aug = BatchCrop("32", seed=9, n_classes=3), BatchAugment("flip,rotate=10,brightness=0.1", seed=9)
    _, plain = _serve(DeviceBatchLoader(ds, 3, shuffle=True, seed=9, workers=4, crop=crop), 1)
    _, both = _serve(DeviceBatchLoader(ds, 3, shuffle=True, seed=9, workers=4, crop=crop, augment=aug), 1)
    assert len(plain) == len(both) == 8
    changed = 0
    for (e, idx, batch), (e2, idx2, got) in zip(plain, both):
        assert (e, idx) == (e2, idx2)
        want = aug(batch, e, idx)
        assert got["image"].is_contiguous(memory_format=torch.channels_last) or got["image"].shape[1] == 1
        assert _bytes(got["image"]) == _bytes(want["image"]) and _bytes(got["mask"]) == _bytes(want["mask"])
        changed += _bytes(got["image"]) != _bytes(batch["image"])
    assert changed == len(plain)


def test_loader_without_crop_still_refuses_mixed_sizes(folder):
    from unet_amd.utils.data_loading import DeviceBatchLoader
    from unet_amd import BatchCrop
    ds = _train_set(folder, 1.0, augment=False)
    first = next(iter(DeviceBatchLoader(ds, 3, shuffle=False, workers=2, crop=BatchCrop("32", seed=0, n_classes=3))))
    assert first["image"].shape == (3, 1, 32, 32) and first["mask"].shape == (3, 32, 32)    # the same three files, cropped
    with pytest.raises(ValueError, match="one decoded size"):
        list(DeviceBatchLoader(ds, 3, shuffle=False, workers=2))


def test_batch_crop_names_an_item_that_is_too_small(folder):
    from unet_amd import BatchCrop
    from unet_amd.utils.data_loading import DeviceBatchLoader
    ds = _train_set(folder, 1.0, augment=False)
    small = [i for i in range(len(ds)) if min(ds[i]["mask"].shape) < 48]
    with pytest.raises(ValueError, match=r"item (%s) is .* smaller than the 48 x 48 crop" % "|".join(map(str, small))):
        list(DeviceBatchLoader(ds, 1, shuffle=False, workers=2, crop=BatchCrop("48", seed=0, n_classes=3)))


# ---------------------------------------------------------------------------------------------------------- command line
CLI = ["--model", "UNet_T", "-b", "3", "-s", "1", "--seed", "0", "--workers", "4", "--crop", "32", "--tile", "32,overlap=8"]


def _run_cli(cwd, args, timeout=300):
    os.makedirs(cwd, exist_ok=True)
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "unet_amd.train"] + args, capture_output=True, text=True, timeout=timeout,
                       cwd=str(cwd), env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    return r


@pytest.fixture(scope="module")
def runs(tmp_path_factory, folder):
    """A: two epochs in one go.  B: one epoch, then --resume up to the second.  Same folder, same options."""
    top = tmp_path_factory.mktemp("crop_cli")
    base = CLI + ["--data-root", folder]
    a, b = top / "a", top / "b"
    log_a = _run_cli(a, base + ["-e", "2", "--save-state", "--checkpoint-dir", str(a / "ck")]).stderr
    _run_cli(b, base + ["-e", "1", "--save-state", "--checkpoint-dir", str(b / "ck")])
    log_b2 = _run_cli(b, base + ["-e", "2", "--resume", str(b / "ck" / "train_state.pth"), "--checkpoint-dir", str(b / "ck")]).stderr
    return {"a": a, "b": b, "log_a": log_a, "log_b2": log_b2}


def _load(path):
    return torch.load(path, map_location="cpu", weights_only=True)


def test_cli_completes_and_logs_the_crop(runs):
    assert "Training crops (seed 0): 32,fg=0.5,classes=2" in runs["log_a"]
    assert "Training crops (seed 0): 32,fg=0.5,classes=2" in runs["log_b2"]
    assert runs["log_a"].count("Validation Dice score") == 2 and "Epoch 2/2: loss" in runs["log_a"]
    state = _load(runs["a"] / "ck" / "train_state.pth")
    assert state["args"]["crop"] == "32,fg=0.5" and state["args"]["tile"] == "32,overlap=8"
    assert "crop_seed" not in state and state["loader_seed"] == 0 and state["epoch"] == 2 and state["global_step"] == 16


def test_cli_resumed_run_ends_where_the_uninterrupted_run_ends(runs):
    want, got = _load(runs["a"] / "model_epoch2.pth"), _load(runs["b"] / "model_epoch2.pth")
    assert list(want) == list(got)
    for k in want:
        assert torch.equal(want[k], got[k]), k
    first = _load(runs["b"] / "model_epoch1.pth")
    assert any(not torch.equal(first[k], got[k]) for k in first)
    assert "Resumed after epoch 1 (global step 8" in runs["log_b2"] and "Epoch 1/2" not in runs["log_b2"]


def test_cli_tile_reaches_evaluate(runs, folder):
    """The last evaluation of the loop runs on the final weights: its logged Dice is evaluate(tile=...) on model_epoch2.pth."""
    import unet_amd
    from unet_amd.utils.data_loading import DeviceBatchLoader
    logged = re.findall(r"Validation Dice score: (\S+)  postprocessed: (\S+)  min: (\S+)", runs["log_a"])
    assert len(logged) == 2
    model = unet_amd.UNet_T(n_channels=1, n_classes=3, bilinear=False)
    model.load_state_dict(_load(runs["a"] / "model_epoch2.pth"))
    model = model.to(memory_format=torch.channels_last).to(_dev())
    val = unet_amd.BasicDataset(os.path.join(folder, "imgs", "val"), os.path.join(folder, "masks", "val"), 1.0)
    loader = DeviceBatchLoader(val, 3, shuffle=False, drop_last=True, workers=4, device=_dev())
    dice = unet_amd.evaluate(model, loader, _dev(), True, tile="32,overlap=8")
    assert tuple(repr(float(v)) for v in dice) == logged[-1]
