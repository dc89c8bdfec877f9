"""Training augmentation on the MI355X (csrc/augment.hip through BatchAugment): the device against the numpy restatement
bit for bit (geometry, contrast, brightness), exact properties (identity, flips, repeatability, batch invariance), gamma
and noise against float64 with torch's CPU float32 as the yardstick, the augmented DeviceBatchLoader and the command line.

Measured on one MI355X (max |error| against float64; the yardstick is torch's CPU float32 evaluation of the same formula):
gamma: device 5.88e-08, CPU float32 3.46e-08, ratio 1.70 (allowed 4; the bound in force was the 2^-22 floor, 2.38e-07);
noise: device 1.03e-05, CPU float32 1.03e-05, ratio 1.00 (bound 4.13e-05; both are the fp32 rounding of the angle)."""
import logging
import os
import sys

import numpy as np
import pytest
import torch

import augment_ref as AR
from test_gpu_train_cli import _png_tree

pytestmark = pytest.mark.gpu

GEOMETRY = "flip,rotate=25,scale=0.2,translate=0.1"


def _batch(B, C, H, W, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    img = torch.rand(B, H, W, C, generator=g).to(dtype)
    lab = torch.randint(0, 3, (B, H, W), generator=g)
    return {"image": img.cuda().permute(0, 3, 1, 2), "mask": lab.cuda()}, img.float().numpy(), lab.numpy()


def _nhwc(out):
    return out["image"].permute(0, 2, 3, 1).float().cpu().numpy()


def _row(table, b):
    r = {k: table[b][k] for k in ("gamma", "contrast", "brightness", "noise_std")}
    r["m"], r["key"] = table["m"][b].tolist(), tuple(int(k) for k in table["key"][b])
    return r


@pytest.mark.parametrize("border", ["clamp", "fill"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("H,W", [(100, 37), (512, 512), (999, 1000)])
def test_device_equals_restatement_bit_for_bit(H, W, C, dtype, border):
    from unet_amd import AugmentConfig, BatchAugment
    cfg = AugmentConfig.parse(GEOMETRY + f",contrast=0.3,brightness=0.2,border={border},fill_image=0.25,fill_label=1")
    aug = BatchAugment(cfg, seed=H * 1000 + W)
    idx = [3, 0, 17, 8, 5]
    batch, img, lab = _batch(5, C, H, W, dtype, H + W + C)
    out = aug(batch, 1, idx)
    assert out["image"].dtype == dtype and out["image"].shape == batch["image"].shape
    assert out["image"].is_contiguous(memory_format=torch.channels_last) or C == 1
    got_i, got_l = _nhwc(out), out["mask"].cpu().numpy()
    table = aug.params(1, idx, (H, W))
    assert len({table[b].tobytes() for b in range(5)}) == 5                    # five different parameter rows
    for b in range(5):
        want_i, want_l = AR.augment_item(img[b], lab[b], _row(table, b), border, 0.25, 1, np.float32,
                                         bf16=dtype == torch.bfloat16)
        assert got_i[b].tobytes() == np.asarray(want_i, np.float32).tobytes(), (b, np.abs(got_i[b] - want_i).max())
        assert np.array_equal(got_l[b], want_l), b


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_neutral_config_returns_the_input_bits(dtype):
    from unet_amd import AugmentConfig, BatchAugment
    batch, _, _ = _batch(3, 3, 100, 37, dtype, 1)
    out = BatchAugment(AugmentConfig(), 7)(batch, 4, [9, 1, 2])
    assert torch.equal(out["image"], batch["image"]) and torch.equal(out["mask"], batch["mask"])
    assert out["image"].data_ptr() != batch["image"].data_ptr()


def test_flip_only_equals_torch_flip():
    from unet_amd import AugmentConfig, BatchAugment
    batch, _, _ = _batch(8, 1, 96, 130, torch.float32, 2)
    aug = BatchAugment(AugmentConfig.parse("flip"), 11)
    idx = list(range(8))
    out = aug(batch, 0, idx)
    d = aug.draws(0, idx, (96, 130))
    seen = set()
    for b in range(8):
        dims = [k for k, on in ((-1, d["hflip"][b]), (-2, d["vflip"][b])) if on]
        seen.add(tuple(dims))
        assert torch.equal(out["image"][b], torch.flip(batch["image"][b], dims) if dims else batch["image"][b]), b
        assert torch.equal(out["mask"][b], torch.flip(batch["mask"][b], dims) if dims else batch["mask"][b]), b
    assert len(seen) >= 3


def test_repeatable_and_independent_of_the_batch():
    from unet_amd import AugmentConfig, BatchAugment
    cfg = AugmentConfig.parse("flip,rotate=15,scale=0.1,translate=0.05,brightness=0.1,contrast=0.1,gamma=0.2,noise=0.01")
    aug = BatchAugment(cfg, 3)
    batch, _, _ = _batch(8, 3, 120, 200, torch.float32, 3)
    idx = [4, 9, 1, 0, 30, 2, 7, 5]
    a, b = aug(batch, 2, idx), BatchAugment(cfg, 3)(batch, 2, idx)
    assert torch.equal(a["image"], b["image"]) and torch.equal(a["mask"], b["mask"])          # two runs, identical bytes
    for pos in range(8):                                                                       # alone = inside the batch
        one = aug({"image": batch["image"][pos:pos + 1], "mask": batch["mask"][pos:pos + 1]}, 2, [idx[pos]])
        assert torch.equal(one["image"][0], a["image"][pos]) and torch.equal(one["mask"][0], a["mask"][pos]), pos
    perm = [7, 3, 0, 5, 1, 6, 2, 4]                                                            # at any position
    p = aug({"image": batch["image"][perm], "mask": batch["mask"][perm]}, 2, [idx[k] for k in perm])
    assert torch.equal(p["image"], a["image"][perm]) and torch.equal(p["mask"], a["mask"][perm])
    assert not torch.equal(aug(batch, 3, idx)["image"], a["image"])                            # another epoch differs
    img_only, lab_only = aug({"image": batch["image"]}, 2, idx), aug({"mask": batch["mask"]}, 2, idx)
    assert torch.equal(img_only["image"], a["image"]) and torch.equal(lab_only["mask"], a["mask"])


def _yardstick(device_err, cpu32_err, what):
    """tests/yardstick.py's manner: the device's error against float64 is held to 4 x the error of torch's CPU float32
    evaluation of the same formula (two libms, a few ulp each), with a floor of 2^-22 (one fp32 ulp at 0.25)."""
    bound = max(4.0 * cpu32_err, 2.0 ** -22)
    print(f"{what}: device max|err| {device_err:.3e}, torch CPU float32 {cpu32_err:.3e}, "
          f"ratio {device_err / max(cpu32_err, 1e-300):.2f}, bound {bound:.3e}")
    assert device_err <= bound, (what, device_err, bound)


def test_gamma_against_float64():
    from unet_amd import AugmentConfig, BatchAugment
    aug = BatchAugment(AugmentConfig.parse("gamma=0.5"), 21)
    batch, img, _ = _batch(4, 1, 256, 256, torch.float32, 4)
    idx = [0, 1, 2, 3]
    table = aug.params(0, idx, (256, 256))
    assert (table["gamma"] != 1).all()
    got = _nhwc(aug(batch, 0, idx)).astype(np.float64)
    exact = np.stack([AR.photometry(img[b], table["gamma"][b], 1.0, 0.0, 0.0, None, np.float64) for b in range(4)])
    x = torch.from_numpy(img)                                                         # the same formula in CPU float32
    cpu32 = torch.stack([torch.pow(x[b].clamp(0, 1), torch.tensor(table["gamma"][b])).clamp(0, 1) for b in range(4)])
    assert cpu32.dtype == torch.float32
    _yardstick(float(np.abs(got - exact).max()), float(np.abs(cpu32.double().numpy() - exact).max()), "gamma")


def test_noise_against_float64_and_its_moments():
    from unet_amd import AugmentConfig, BatchAugment
    sigma = 0.05
    aug = BatchAugment(AugmentConfig.parse(f"noise={sigma}"), 33)
    H = W = 1024                                                                       # N = 2^20 pixels
    x = torch.full((1, 1, H, W), 0.5, device="cuda")                                   # clamp never bites: 10 sigma to spare
    out = aug({"image": x}, 0, [5])["image"]
    table = aug.params(0, [5], (H, W))
    s32 = table["noise_std"][0]
    z_dev = ((out.cpu().double().numpy().reshape(-1) - 0.5) / float(s32))
    n = z_dev.size
    words = AR.noise_words(tuple(int(k) for k in table["key"][0]), n)
    z64 = AR.normals(words, n, np.float64)
    # torch's CPU float32 evaluation of the same formula from the same words
    w = torch.from_numpy(words.astype(np.int64)).to(torch.float32)
    u, v = (w[:, 0::2] + 0.5) * 2.0 ** -32, w[:, 1::2] * 2.0 ** -32
    rad, ang = torch.sqrt(-2.0 * torch.log(u)), 6.283185307179586 * v
    z32 = torch.stack([rad * torch.cos(ang), rad * torch.sin(ang)], -1).reshape(-1)[:n]
    out32 = (torch.full((n,), 0.5) + torch.tensor(s32) * z32).clamp(0, 1)          # ... through the fp32 output, as the device
    assert out32.dtype == torch.float32
    z_cpu = (out32.double().numpy() - 0.5) / float(s32)
    _yardstick(float(np.abs(z_dev - z64).max()), float(np.abs(z_cpu - z64).max()), "noise")
    assert abs(z_dev.mean()) <= 5 / np.sqrt(n), z_dev.mean()
    assert abs(z_dev.var() - 1) <= 5 * np.sqrt(2 / n), z_dev.var()


def _stack(ds, ids):
    return torch.stack([ds[i]["image"] for i in ids]), torch.stack([ds[i]["mask"] for i in ids])


def test_augmented_loader(tmp_path):
    from unet_amd import AugmentConfig, BatchAugment
    from unet_amd.utils.data_loading import BasicDataset, DeviceBatchLoader, collate_raw, prepare_batch_device
    _png_tree(str(tmp_path), 3, 0, 96, seed=5)
    ds = BasicDataset(str(tmp_path / "imgs" / "train"), str(tmp_path / "masks" / "train"), 0.5)
    cfg = AugmentConfig.parse("default")
    loaders = [DeviceBatchLoader(ds, 5, shuffle=True, drop_last=False, seed=11, workers=3, augment=BatchAugment(cfg, 11))
               for _ in range(2)]
    by_hand = BatchAugment(cfg, 11)
    epochs = []
    for epoch in range(2):
        got = list(loaders[0])
        again = list(loaders[1])                                         # a second loader with the same seed
        idx = loaders[0].batches_of(loaders[0].orders[epoch])
        assert len(got) == len(again) == len(idx) == 3
        for batch, rep, ids in zip(got, again, idx):
            raw = collate_raw([ds.raw_item(i, host_rescale=False) for i in ids])
            plain = prepare_batch_device(raw["image_u8"], raw["mask_u8"], raw["turns"], device="cuda", scale=raw["scale"])
            want = by_hand(plain, epoch, ids)
            assert torch.equal(batch["image"], want["image"]) and torch.equal(batch["mask"], want["mask"])
            assert torch.equal(batch["image"], rep["image"]) and torch.equal(batch["mask"], rep["mask"])
            assert not torch.equal(batch["image"], plain["image"])
            assert batch["image"].is_contiguous(memory_format=torch.channels_last)
        epochs.append({i: batch["image"][k].cpu() for batch, ids in zip(got, idx) for k, i in enumerate(ids)})
    assert all(not torch.equal(epochs[0][i], epochs[1][i]) for i in epochs[0])          # epoch 1 differs from epoch 0
    # augment=None yields what it yields today
    loader = DeviceBatchLoader(ds, 5, shuffle=True, drop_last=False, seed=11, workers=3, augment=None)
    for batch, ids in zip(list(loader), loader.batches_of(loader.epoch_order(0))):
        wi, wm = _stack(ds, ids)
        assert torch.equal(batch["image"].cpu(), wi) and torch.equal(batch["mask"].cpu(), wm)


def test_loader_augments_the_host_item_fallback(tmp_path):
    from PIL import Image
    from unet_amd import AugmentConfig, BatchAugment
    from unet_amd.utils.data_loading import BasicDataset, DeviceBatchLoader
    rng = np.random.default_rng(0)
    for d in ("imgs", "masks"):
        os.makedirs(tmp_path / d)
    for i in range(2):
        np.save(tmp_path / "imgs" / f"f{i}.npy", rng.random((20, 20), dtype=np.float32))
        Image.fromarray(rng.choice(np.array([0, 128, 255], np.uint8), (20, 20))).save(tmp_path / "masks" / f"f{i}_mask.png")
    ds = BasicDataset(str(tmp_path / "imgs"), str(tmp_path / "masks"), 0.5)
    aug = BatchAugment(AugmentConfig.parse("flip,rotate=20,brightness=0.1"), 2)
    loader = DeviceBatchLoader(ds, 3, shuffle=False, workers=2, augment=aug)
    got = list(loader)
    assert loader.host_items
    for batch, ids in zip(got, loader.batches_of(loader.orders[0])):
        wi, wm = _stack(ds, ids)
        want = aug({"image": wi.cuda(), "mask": wm.cuda()}, 0, ids)
        assert torch.equal(batch["image"], want["image"]) and torch.equal(batch["mask"], want["mask"])
        assert not torch.equal(batch["image"].cpu(), wi)


def test_command_line_trains_with_augment_and_validates_without(tmp_path, monkeypatch, caplog):
    import unet_amd  # noqa: F401
    from unet_amd import train_cli
    from unet_amd.utils.data_loading import BasicDataset
    data = tmp_path / "data"
    _png_tree(str(data), 3, 2, 128, seed=7)
    monkeypatch.chdir(tmp_path)
    ev = sys.modules["unet_amd.evaluate"]
    real, seen = ev.evaluate, {}

    def spy(net, loader, *a, **k):
        if "first" not in seen:
            seen["augment"] = loader.augment
            seen["first"] = {key: v.cpu() for key, v in next(iter(loader)).items()}
        return real(net, loader, *a, **k)

    monkeypatch.setattr(ev, "evaluate", spy)
    with caplog.at_level(logging.INFO):
        rc = train_cli.main(["--augment", "-e", "1", "-b", "2", "-s", "0.5", "-c", "3", "--seed", "0", "--model", "UNet_T",
                             "--data-root", str(data), "--workers", "4", "--checkpoint-dir", str(tmp_path / "ck")])
    assert rc == 0 and (tmp_path / "model_epoch1.pth").exists()
    assert caplog.text.count("Training augmentation (seed 0): ") == 1 and "rotate=10.0" in caplog.text
    loss = float(caplog.text.split("loss (total) ")[1].split(",")[0])
    assert np.isfinite(loss) and loss > 0
    sd = torch.load(tmp_path / "model_epoch1.pth", map_location="cpu", weights_only=True)
    assert all(torch.isfinite(v).all() for v in sd.values() if v.is_floating_point())
    val = BasicDataset(str(data / "imgs" / "val"), str(data / "masks" / "val"), 0.5)
    wi, wm = _stack(val, [0, 1])
    assert seen["augment"] is None
    assert torch.equal(seen["first"]["image"], wi) and torch.equal(seen["first"]["mask"], wm)
