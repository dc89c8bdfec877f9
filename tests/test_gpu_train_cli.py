"""The training command line and its device input path on the MI355X: uh_batch_rescale_u8 against live Pillow (bytes), the
whole prepare_batch_device(..., scale=s) against stacking ds[i], DeviceBatchLoader, and the CLI run as a subprocess whose
final state_dict is bit-identical to an in-process loop fed with the host-path items in the loader's order."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import ROOT, load_golden
from test_data_loading_cpu import _write_tree

pytestmark = pytest.mark.gpu

_OPS = {1: Image.ROTATE_90, 2: Image.ROTATE_180, 3: Image.ROTATE_270}


def _pil(img, mask, t, s):
    pi, pm = Image.fromarray(img), Image.fromarray(mask)
    if t:
        pi, pm = pi.transpose(_OPS[t]), pm.transpose(_OPS[t])
    size = (int(s * pi.size[0]), int(s * pi.size[1]))
    return np.asarray(pi.resize(size, Image.BICUBIC)), np.asarray(pm.resize(size, Image.NEAREST))


def test_g12_items_at_half_scale(tmp_path):
    from unet_amd.utils.data_loading import BasicDataset, collate_raw, prepare_batch_device
    r = load_golden("g12_data_loading")
    _write_tree(tmp_path, r)
    ds = BasicDataset(str(tmp_path / "imgs"), str(tmp_path / "masks"), 0.5, augment=True)
    for n in ds.ids:
        base = ds.ids.index(n) * 4
        for rots in ((0, 2), (1, 3)):
            b = collate_raw([ds.raw_item(base + t, host_rescale=False) for t in rots])
            assert b["scale"] == 0.5
            for dt in (torch.float32, torch.bfloat16):
                out = prepare_batch_device(b["image_u8"], b["mask_u8"], b["turns"], device="cuda", dtype=dt,
                                           scale=b["scale"])
                want_i = torch.stack([ds[base + t]["image"] for t in rots])
                want_m = torch.stack([ds[base + t]["mask"] for t in rots])
                assert torch.equal(out["image"].cpu(), want_i.to(dt)), (n, rots, dt)
                assert torch.equal(out["mask"].cpu(), want_m), (n, rots)
                for k, t in enumerate(rots):
                    assert np.array_equal(out["image"][k].float().cpu().numpy(),
                                          torch.from_numpy(r[f"s0.5.{n}.r{t}.image"]).to(dt).float().numpy())


@pytest.mark.parametrize("H,W,C", [(1024, 768, 1), (768, 1024, 3), (512, 512, 3), (1000, 1000, 1), (257, 130, 1),
                                   (63, 17, 3), (7, 9, 1)])
def test_rescale_equals_pillow(H, W, C):
    from oracle import data_prep_ref as R
    from unet_amd.utils.data_loading import prepare_batch_device
    from unet_amd.utils.data_rescale import batch_rescale
    rng = np.random.default_rng(H * 3 + W + C)
    B = 4
    img = rng.integers(0, 256, (B, H, W, C), dtype=np.uint8)
    img[2] = rng.integers(0, 2, (H, W, C), dtype=np.uint8)             # a 0/1 image: its rescale decides the /255 rule
    mask = rng.choice(np.array([0, 128, 255, 7], np.uint8), (B, H, W))
    turn_sets = ([0, 1, 2, 3],) if H == W else ([0, 2, 2, 0], [1, 3, 1, 3])
    for s in (0.5, 0.25, 0.37, 0.8):
        if int(s * min(H, W)) == 0:
            continue
        for turns in turn_sets:
            pil = [_pil(img[b] if C > 1 else img[b, ..., 0], mask[b], turns[b], s) for b in range(B)]
            odd = 1 if (H != W and turns[0] & 1) else 0
            t_d = torch.tensor(turns, dtype=torch.int32, device="cuda")
            gi, gm = batch_rescale(torch.from_numpy(img).cuda(), torch.from_numpy(mask).cuda(), t_d, odd, s)
            gi, gm = gi.cpu().numpy(), gm.cpu().numpy()
            for b in range(B):
                wi = pil[b][0] if C > 1 else pil[b][0][..., None]
                assert np.array_equal(gi[b], wi), ("bicubic", H, W, C, s, turns[b])
                assert np.array_equal(gm[b], pil[b][1]), ("nearest", H, W, C, s, turns[b])
            want_i, want_m = R.prepare_batch([p[0] for p in pil], np.stack([p[1] for p in pil]))
            for dt in (torch.float32, torch.bfloat16):
                out = prepare_batch_device(torch.from_numpy(img), torch.from_numpy(mask), turns, device="cuda", dtype=dt,
                                           scale=s)
                assert torch.equal(out["image"].cpu(), torch.from_numpy(want_i).to(dt)), (H, W, C, s, turns, dt)
                assert np.array_equal(out["mask"].cpu().numpy(), want_m)


def _png_tree(root, n_train, n_val, size, seed):
    """imgs/{train,val}, masks/{train,val}: ellipse phantoms as 8-bit PNGs, masks coded 0 / 128 / 255."""
    from unet_amd import ellipse_batch
    imgs, masks = ellipse_batch(n_train + n_val, size, seed=seed)
    grey = np.array([0, 128, 255], np.uint8)
    for i in range(n_train + n_val):
        split = "train" if i < n_train else "val"
        for d in ("imgs", "masks"):
            os.makedirs(os.path.join(root, d, split), exist_ok=True)
        Image.fromarray((imgs[i, 0].numpy() * 255).astype(np.uint8)).save(os.path.join(root, "imgs", split, f"p{i:03d}.png"))
        Image.fromarray(grey[masks[i].numpy()]).save(os.path.join(root, "masks", split, f"p{i:03d}_mask.png"))


def test_loader_batches_equal_host_items(tmp_path):
    from unet_amd.utils.data_loading import BasicDataset, DeviceBatchLoader
    _png_tree(str(tmp_path), 3, 0, 96, seed=5)
    ds = BasicDataset(str(tmp_path / "imgs" / "train"), str(tmp_path / "masks" / "train"), 0.5)
    loader = DeviceBatchLoader(ds, 5, shuffle=True, drop_last=False, seed=11, workers=3)
    for epoch in range(2):
        got = list(loader)
        idx = loader.batches_of(loader.orders[epoch])
        assert loader.orders[epoch] == loader.epoch_order(epoch) and len(got) == len(idx) == 3
        for batch, ids in zip(got, idx):
            assert torch.equal(batch["image"].cpu(), torch.stack([ds[i]["image"] for i in ids]))
            assert torch.equal(batch["mask"].cpu(), torch.stack([ds[i]["mask"] for i in ids]))
            assert batch["image"].is_contiguous(memory_format=torch.channels_last)


def test_loader_falls_back_for_float_images(tmp_path, caplog):
    from unet_amd.utils.data_loading import BasicDataset, DeviceBatchLoader
    rng = np.random.default_rng(0)
    for d in ("imgs", "masks"):
        os.makedirs(tmp_path / d)
    for i in range(2):
        np.save(tmp_path / "imgs" / f"f{i}.npy", rng.random((20, 20), dtype=np.float32))
        Image.fromarray(rng.choice(np.array([0, 128, 255], np.uint8), (20, 20))).save(tmp_path / "masks" / f"f{i}_mask.png")
    ds = BasicDataset(str(tmp_path / "imgs"), str(tmp_path / "masks"), 0.5)
    loader = DeviceBatchLoader(ds, 2, shuffle=False, workers=2)
    with caplog.at_level("INFO"):
        got = list(loader)
    assert loader.host_items and caplog.text.count("serving ds[i]") == 1
    for batch, ids in zip(got, loader.batches_of(loader.orders[0])):
        assert torch.equal(batch["image"].cpu(), torch.stack([ds[i]["image"] for i in ids]))


def _run_cli(cwd, args, timeout=300):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "unet_amd.train"] + args, capture_output=True, text=True, timeout=timeout,
                       cwd=str(cwd), env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    return r


def _replay(data, model_name, classes, bilinear, epochs, batch, seed, lr=1e-5):
    """The CLI's loop in process, fed with the HOST-path items (ds[i]) in the loader's order."""
    import unet_amd
    from unet_amd.evaluate import evaluate
    from unet_amd.train import TrainStepper, cosine_warm_restarts_lr
    from unet_amd.train_cli import eval_due
    from unet_amd.utils.data_loading import BasicDataset, DeviceBatchLoader
    dev = torch.device("cuda", torch.cuda.current_device())
    train = BasicDataset(str(data / "imgs" / "train"), str(data / "masks" / "train"), 0.5)
    val = BasicDataset(str(data / "imgs" / "val"), str(data / "masks" / "val"), 0.5)
    torch.manual_seed(seed)
    model = getattr(unet_amd, model_name)(n_channels=1, n_classes=classes, bilinear=bilinear)
    model = model.to(memory_format=torch.channels_last).to(dev)
    stepper = TrainStepper(model, lr=lr, amp=True)
    order = DeviceBatchLoader(train, batch, shuffle=True, drop_last=False, seed=seed)
    n = len(train)
    stack = lambda ds, ids: {"image": torch.stack([ds[i]["image"] for i in ids]),
                             "mask": torch.stack([ds[i]["mask"] for i in ids])}
    val_batches = [stack(val, ids) for ids in DeviceBatchLoader(val, batch, drop_last=True).batches_of(list(range(len(val))))]
    gs, evals = 0, 0
    for epoch in range(epochs):
        for ids in order.batches_of(order.epoch_order(epoch)):
            b = stack(train, ids)
            stepper.step(b["image"].to(dev, torch.float32, memory_format=torch.channels_last), b["mask"].to(dev))
            gs += 1
            if eval_due(gs, n, batch):
                score, _, _ = evaluate(model, val_batches, dev, True)
                stepper.optimizer.param_groups[0]["lr"] = cosine_warm_restarts_lr(lr, float(score))
                evals += 1
    torch.cuda.synchronize()
    stepper.close()
    return {k: v.detach().cpu() for k, v in model.state_dict().items()}, evals


@pytest.mark.parametrize("classes,bilinear", [(3, False), (1, True)])
def test_cli_equals_host_path_loop(tmp_path, classes, bilinear):
    import unet_amd
    data = tmp_path / "data"
    _png_tree(str(data), 3, 2, 128, seed=7)
    args = ["-e", "2", "-b", "2", "-s", "0.5", "-c", str(classes), "--seed", "0", "--model", "UNet_T",
            "--data-root", str(data), "--workers", "4"] + (["--bilinear"] if bilinear else [])
    r = _run_cli(tmp_path, args)
    assert "images/s" in r.stderr and "Validation Dice score" in r.stderr
    sd = torch.load(tmp_path / "model_epoch2.pth", map_location="cpu", weights_only=True)
    assert "mask_values" not in sd
    m = unet_amd.UNet_T(1, classes, bilinear=bilinear)
    m.load_state_dict(sd)
    want, evals = _replay(data, "UNet_T", classes, bilinear, 2, 2, 0)
    assert evals == 2                                               # 12 items, batch 2: after steps 6 and 12
    assert list(sd) == list(want)
    for k in want:
        assert torch.equal(sd[k], want[k]), k


def test_checkpoint_and_resume(tmp_path):
    import unet_amd
    data = tmp_path / "data"
    _png_tree(str(data), 2, 1, 64, seed=3)
    _run_cli(tmp_path, ["-e", "10", "-b", "4", "-s", "0.5", "-c", "3", "--model", "UNet_T", "--seed", "1",
                        "--data-root", str(data), "--checkpoint-dir", str(tmp_path / "ck")])
    files = sorted(os.listdir(tmp_path / "ck"))
    assert files == ["checkpoint_epoch10.pth"]
    ck = torch.load(tmp_path / "ck" / "checkpoint_epoch10.pth", map_location="cpu", weights_only=True)
    assert ck["mask_values"] == [0, 128, 255, 0, 128, 255]                 # train.mask_values + val.mask_values
    final = torch.load(tmp_path / "model_epoch10.pth", map_location="cpu", weights_only=True)
    assert all(torch.equal(final[k], ck[k]) for k in final)
    r = _run_cli(tmp_path, ["-e", "1", "-b", "4", "-s", "0.5", "-c", "3", "--model", "UNet_T", "--seed", "1",
                            "--data-root", str(data), "-f", str(tmp_path / "ck" / "checkpoint_epoch10.pth")])
    assert "Model loaded from" in r.stderr
    resumed = torch.load(tmp_path / "model_epoch1.pth", map_location="cpu", weights_only=True)
    fresh = unet_amd.UNet_T(1, 3)
    # one more epoch from the checkpoint: the weights moved on from it, and are not a fresh start
    assert not torch.equal(resumed["inc.double_conv.0.weight"], ck["inc.double_conv.0.weight"])
    d_ck = (resumed["inc.double_conv.0.weight"] - ck["inc.double_conv.0.weight"]).abs().max()
    d_fresh = (resumed["inc.double_conv.0.weight"] - fresh.state_dict()["inc.double_conv.0.weight"]).abs().max()
    assert d_ck < d_fresh
