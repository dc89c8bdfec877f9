"""Elastic deformation on the MI355X (csrc/augment.hip: uh_batch_augment_elastic, through BatchAugment and
augment_with_control): the device against the numpy restatement (tests/elastic_ref.py) bit for bit, exact properties (zero
and constant fields against uh_batch_augment, batch invariance, repeatability, the identity record), the loader and the
command line."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import augment_ref as AR
import elastic_ref as ER
from test_gpu_augment import GEOMETRY, _batch, _nhwc, _row
from test_gpu_train_cli import ROOT, _png_tree

pytestmark = pytest.mark.gpu

PHOTO = "contrast=0.3,brightness=0.2"


@pytest.mark.parametrize("affine", [GEOMETRY, "none"], ids=["affine", "identity"])
@pytest.mark.parametrize("border", ["clamp", "fill"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("grid", [16, 64])
@pytest.mark.parametrize("H,W", [(100, 37), (96, 130)])
def test_device_equals_restatement_bit_for_bit(H, W, grid, C, dtype, border, affine):
    from unet_amd import AugmentConfig, BatchAugment, ElasticConfig
    cfg = AugmentConfig.parse(f"{affine},{PHOTO},border={border},fill_image=0.25,fill_label=1")
    aug = BatchAugment(cfg, seed=H * 1000 + W, elastic=ElasticConfig(grid=grid, sigma=grid / 10))
    idx = [3, 0, 17, 8, 5]
    batch, img, lab = _batch(5, C, H, W, dtype, H + W + C)
    out = aug(batch, 1, idx)
    assert out["image"].dtype == dtype and out["image"].shape == batch["image"].shape
    got_i, got_l = _nhwc(out), out["mask"].cpu().numpy()
    table, control = aug.params(1, idx, (H, W)), aug.elastic_table(1, idx, (H, W))
    assert len({control[b].tobytes() for b in range(5)}) == 5 and control.any(axis=(1, 2, 3)).all()      # five different tables
    moved = 0
    for b in range(5):
        want_i, want_l = ER.augment_item(img[b], lab[b], _row(table, b), control[b], grid, border, 0.25, 1, np.float32,
                                         bf16=dtype == torch.bfloat16)
        assert got_i[b].tobytes() == np.asarray(want_i, np.float32).tobytes(), (b, np.abs(got_i[b] - want_i).max())
        assert np.array_equal(got_l[b], want_l), b
        moved += int((want_l != AR.labels_nearest(lab[b], _row(table, b)["m"], border == "fill", 1)).sum())
    assert moved > 0                                                          # the field does move labels


def _geometry_rows(B, H, W, border="fill", seed=9, epoch=0):
    from unet_amd import AugmentConfig, BatchAugment
    cfg = AugmentConfig.parse(f"{GEOMETRY},{PHOTO},border={border},fill_image=0.25")
    return BatchAugment(cfg, seed).params(epoch, list(range(B)), (H, W))


@pytest.mark.parametrize("grid", [16, 64])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_zero_field_equals_the_affine_launch(grid, dtype):
    from unet_amd.utils.augment import augment_with_control
    B, H, W = 4, 100, 150
    batch, _, _ = _batch(B, 3, H, W, dtype, 6)
    for border in ("clamp", "fill"):
        rows = _geometry_rows(B, H, W, border)
        zero = np.zeros((B,) + ER.grid_shape(H, W, grid) + (2,), np.int32)
        got = augment_with_control(batch, rows, zero, grid, border, 0.25, 1)
        want = augment_with_control(batch, rows, None, grid, border, 0.25, 1)          # uh_batch_augment
        assert torch.equal(got["image"], want["image"]) and torch.equal(got["mask"], want["mask"])
        assert not torch.equal(want["image"], batch["image"])


@pytest.mark.parametrize("grid", [16, 64])
def test_constant_field_equals_shifted_offsets(grid):
    from unet_amd.utils.augment import augment_with_control
    B, H, W = 4, 100, 150
    batch, _, _ = _batch(B, 1, H, W, torch.float32, 7)
    rows = _geometry_rows(B, H, W)
    control = np.empty((B,) + ER.grid_shape(H, W, grid) + (2,), np.int32)
    control[..., 0], control[..., 1] = 3 << 16, -(2 << 16)                            # (+3, -2) whole pixels
    shifted = rows.copy()
    shifted["m"][:, 2] += 3 << 32
    shifted["m"][:, 5] -= 2 << 32
    got = augment_with_control(batch, rows, control, grid, "fill", 0.25, 1)
    want = augment_with_control(batch, shifted, None, grid, "fill", 0.25, 1)
    assert torch.equal(got["image"], want["image"]) and torch.equal(got["mask"], want["mask"])
    plain = augment_with_control(batch, rows, None, grid, "fill", 0.25, 1)
    assert not torch.equal(got["image"], plain["image"]) and not torch.equal(got["mask"], plain["mask"])


def _elastic_aug(seed=3, spec="grid=32,sigma=3"):
    from unet_amd import AugmentConfig, BatchAugment
    cfg = AugmentConfig.parse("flip,rotate=15,scale=0.1,translate=0.05,brightness=0.1,contrast=0.1,gamma=0.2,noise=0.01")
    return BatchAugment(cfg, seed, elastic=spec)


def test_repeatable_and_independent_of_the_batch():
    aug = _elastic_aug()
    batch, _, _ = _batch(8, 3, 120, 200, torch.float32, 3)
    idx = [4, 9, 1, 0, 30, 2, 7, 5]
    a, b = aug(batch, 2, idx), _elastic_aug()(batch, 2, idx)
    assert torch.equal(a["image"], b["image"]) and torch.equal(a["mask"], b["mask"])          # two calls, identical bytes
    for pos in range(8):                                                                       # alone = inside the batch
        one = aug({"image": batch["image"][pos:pos + 1], "mask": batch["mask"][pos:pos + 1]}, 2, [idx[pos]])
        assert torch.equal(one["image"][0], a["image"][pos]) and torch.equal(one["mask"][0], a["mask"][pos]), pos
    perm = [7, 3, 0, 5, 1, 6, 2, 4]                                                            # at any position
    p = aug({"image": batch["image"][perm], "mask": batch["mask"][perm]}, 2, [idx[k] for k in perm])
    assert torch.equal(p["image"], a["image"][perm]) and torch.equal(p["mask"], a["mask"][perm])
    assert not torch.equal(aug(batch, 3, idx)["mask"], a["mask"])                              # another epoch differs
    plain = _elastic_aug(spec="none")(batch, 2, idx)                                           # and the field is not nothing
    assert not torch.equal(plain["mask"], a["mask"]) and not torch.equal(plain["image"], a["image"])
    img_only, lab_only = aug({"image": batch["image"]}, 2, idx), aug({"mask": batch["mask"]}, 2, idx)
    assert torch.equal(img_only["image"], a["image"]) and torch.equal(lab_only["mask"], a["mask"])


def test_identity_record_is_the_plain_call():
    from unet_amd import BatchAugment, ElasticConfig
    batch, _, _ = _batch(4, 3, 100, 37, torch.bfloat16, 1)
    idx = [9, 1, 2, 6]
    plain = _elastic_aug(spec=None)
    want = BatchAugment(plain.config, plain.seed)(batch, 4, idx)
    for el in (ElasticConfig(sigma=0), ElasticConfig(grid=32, sigma=3, p=0), None):
        got = BatchAugment(plain.config, plain.seed, elastic=el)(batch, 4, idx)
        assert torch.equal(got["image"], want["image"]) and torch.equal(got["mask"], want["mask"])


def test_bad_tables_are_refused():
    from unet_amd.utils.augment import augment_with_control
    batch, _, _ = _batch(2, 1, 40, 40, torch.float32, 1)
    rows = _geometry_rows(2, 40, 40)
    with pytest.raises(TypeError, match="control table"):
        augment_with_control(batch, rows, np.zeros((2, 5, 5, 2), np.int32), 16, "clamp", 0.0, 1)       # GH = GW = 6
    with pytest.raises(ValueError):
        augment_with_control(batch, rows, np.zeros((2, 6, 6, 2), np.int32), 24, "clamp", 0.0, 1)


def test_elastic_loader_serves_the_same_bytes_per_index_in_any_order(tmp_path):
    from unet_amd.utils.data_loading import BasicDataset, DeviceBatchLoader
    _png_tree(str(tmp_path), 3, 0, 96, seed=5)
    ds = BasicDataset(str(tmp_path / "imgs" / "train"), str(tmp_path / "masks" / "train"), 0.5)
    served = []
    for shuffle in (True, False):
        loader = DeviceBatchLoader(ds, 5, shuffle=shuffle, drop_last=False, seed=11, workers=3,
                                   augment=_elastic_aug(11, "grid=16,sigma=1.5"))
        got = list(loader)
        ids = loader.batches_of(loader.orders[0])
        served.append({i: (b["image"][k].cpu(), b["mask"][k].cpu()) for b, idx in zip(got, ids) for k, i in enumerate(idx)})
    assert served[0].keys() == served[1].keys() == set(range(len(ds)))
    assert loader.orders[0] == list(range(len(ds)))
    for i in served[0]:
        assert torch.equal(served[0][i][0], served[1][i][0]) and torch.equal(served[0][i][1], served[1][i][1]), i
    plain = DeviceBatchLoader(ds, 5, shuffle=False, seed=11, workers=3, augment=_elastic_aug(11, "none"))
    first = next(iter(plain))
    assert not torch.equal(first["mask"][0].cpu(), served[1][0][1])


def _train(cwd, data, extra, limit=240):
    """One `python -m unet_amd.train` run in a fresh child process under its own time limit; returns the saved weights."""
    os.makedirs(cwd)
    args = ["-e", "1", "-b", "2", "-s", "0.5", "-c", "3", "--seed", "0", "--model", "UNet_T", "--data-root", str(data),
            "--workers", "4", "--checkpoint-dir", str(cwd / "ck")] + extra
    r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, "-m", "unet_amd.train"] + args, capture_output=True,
                       text=True, timeout=limit + 30, cwd=str(cwd), env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, r.stderr[-4000:]
    return torch.load(cwd / "model_epoch1.pth", map_location="cpu", weights_only=True), r.stderr


def test_command_line_trains_with_elastic(tmp_path):
    data = tmp_path / "data"
    _png_tree(str(data), 3, 2, 128, seed=7)
    a, log = _train(tmp_path / "a", data, ["--augment", "--elastic"])
    assert log.count("Training augmentation (seed 0): ") == 1 and "; elastic grid=64,sigma=4.0,p=1.0" in log
    b, _ = _train(tmp_path / "b", data, ["--augment", "--elastic"])
    c, log_c = _train(tmp_path / "c", data, ["--augment"])
    assert "elastic" not in log_c
    assert a.keys() == b.keys() == c.keys()
    assert all(torch.equal(a[k], b[k]) for k in a)                                   # the same seed: identical weights
    assert all(torch.isfinite(v).all() for v in a.values() if v.is_floating_point())
    assert any(not torch.equal(a[k], c[k]) for k in a)                               # without --elastic: other weights
