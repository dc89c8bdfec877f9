"""The training command line (train_cli.py) and the dataset rescale it moves to the device, host side: the Pillow
restatements of tests/resize_ref.py against live Pillow, the package's tables against the restatements, the reference's
flags and defaults, the evaluation / checkpoint cadence against a literal restatement of train.py:161-216, the loader's
order, raw_item(host_rescale=False), and the refusal to train without a GPU."""
import numpy as np
import pytest
import torch
from PIL import Image

import resize_ref as RR
from conftest import load_golden
from test_data_loading_cpu import _write_tree

SCALES = (0.5, 0.25, 0.3, 0.37, 0.7, 0.8)
SMALL = list(range(1, 64))
LARGE = [(64, 65), (100, 129), (255, 256), (333, 500), (512, 511), (767, 1024), (1100, 999)]
_OPS = {1: Image.ROTATE_90, 2: Image.ROTATE_180, 3: Image.ROTATE_270}


def _pil_rescale(img, mask, turns, scale):
    pi, pm = Image.fromarray(img), Image.fromarray(mask)
    if turns:
        pi, pm = pi.transpose(_OPS[turns]), pm.transpose(_OPS[turns])
    size = (int(scale * pi.size[0]), int(scale * pi.size[1]))
    if min(size) <= 0:
        return None
    return np.asarray(pi.resize(size, Image.BICUBIC)), np.asarray(pm.resize(size, Image.NEAREST))


def _check_pair(rng, h, w, C):
    img = rng.integers(0, 256, (h, w) if C == 1 else (h, w, 3), dtype=np.uint8)
    mask = rng.integers(0, 256, (h, w), dtype=np.uint8)
    for s in SCALES:
        for t in range(4):
            want = _pil_rescale(img, mask, t, s)
            if want is None:
                continue
            got = RR.dataset_rescale(img, mask, t, s)
            assert np.array_equal(got[0], want[0]), ("bicubic", h, w, C, s, t)
            assert np.array_equal(got[1], want[1]), ("nearest", h, w, C, s, t)


@pytest.mark.parametrize("C", [1, 3])
def test_restatement_equals_pillow_small(C):
    """Every size below 64 (as height, against a second size as width), six scales, four turns."""
    rng = np.random.default_rng(C)
    for h in SMALL:
        _check_pair(rng, h, 1 + (h * 37) % 63, C)


@pytest.mark.parametrize("h,w", LARGE)
def test_restatement_equals_pillow_large(h, w):
    rng = np.random.default_rng(h * 7 + w)
    for C in (1, 3):
        _check_pair(rng, h, w, C)


def test_nearest_maps_equal_pillow_coordinates():
    """Pillow's own NEAREST index maps: resize an 'I' image whose pixels hold their own column."""
    from unet_amd.utils.data_rescale import nearest_index
    for n in list(range(1, 200)) + list(range(200, 1101, 7)) + [1024, 1100]:
        coords = Image.fromarray(np.arange(n, dtype=np.int32)[None, :], mode="I")
        for s in SCALES:
            m = int(s * n)
            if m <= 0:
                continue
            want = np.asarray(coords.resize((m, 1), Image.NEAREST))[0].astype(np.int64)
            assert np.array_equal(RR.nearest_map(n, m), want), (n, s)
            assert np.array_equal(nearest_index(n, m), want), (n, s)


def test_nearest_is_not_the_closed_form():
    """The reason the maps are tabulated on the host: floor((x + 0.5) * in / out) differs for some sizes."""
    diff = 0
    for n in range(1, 1101):
        for s in SCALES:
            m = int(s * n)
            if m > 0:
                closed = np.floor((np.arange(m) + 0.5) * n / m).astype(np.int64)
                diff += not np.array_equal(closed, RR.nearest_map(n, m))
    assert diff > 0


def test_package_tables_equal_restatement():
    from unet_amd.utils.png_normalize import resample_coeffs
    for n in list(range(1, 64)) + [100, 257, 512, 767, 1024, 1100]:
        for s in SCALES:
            m = int(s * n)
            if m <= 0:
                continue
            b, k = resample_coeffs(n, m, "bicubic")
            rb, rk = RR.bicubic_coeffs(n, m)
            np.testing.assert_array_equal(b, rb)
            np.testing.assert_array_equal(k, rk)


@pytest.mark.parametrize("n_in,n_out", [(700, 512), (96, 512), (4000, 512), (219, 300), (512, 512), (37, 100)])
def test_lanczos_tables_unchanged(n_in, n_out):
    import seg_pipeline_ref as SR
    from unet_amd.utils.png_normalize import lanczos_coeffs, resample_coeffs
    rb, rk = SR.coeffs_ref(n_in, 0.0, n_in, n_out)
    for b, k in (lanczos_coeffs(n_in, n_out), resample_coeffs(n_in, n_out, "lanczos")):
        np.testing.assert_array_equal(b, rb)
        np.testing.assert_array_equal(k, rk)


def test_rescale_plan_span_covers_every_workgroup():
    """`span` bounds the source window of every 64-column horizontal tile (the kernel's LDS window)."""
    from unet_amd.utils.data_rescale import _span
    from unet_amd.utils.png_normalize import resample_coeffs
    for n, m in ((1024, 512), (1100, 275), (768, 614), (63, 15), (5, 1)):
        b, _ = resample_coeffs(n, m, "bicubic")
        span = _span(b)
        for c0 in range(0, m, 64):
            c1 = min(c0 + 64, m) - 1
            assert b[c1, 0] + b[c1, 1] - b[c0, 0] <= span
            assert (b[c0:c1 + 1, 0] >= b[c0, 0]).all() and (b[c0:c1 + 1, 0] + b[c0:c1 + 1, 1] <= b[c1, 0] + b[c1, 1]).all()


# ------------------------------------------------------------------------------------------------ the command line
def test_reference_flags_and_defaults():
    from unet_amd.train_cli import get_args
    a = get_args([])
    assert (a.epochs, a.batch_size, a.lr, a.load, a.scale, a.val, a.amp, a.bilinear, a.classes) == \
        (5, 1, 1e-5, False, 0.5, 10.0, True, False, 3)
    assert (a.model, a.data_root, a.checkpoint_dir, a.workers, a.seed) == \
        ("UNet_S", "data/data-without-black-shadow", "./checkpoints", 8, None)
    b = get_args(["-e", "7", "-b", "4", "-l", "3e-4", "-f", "m.pth", "-s", "0.25", "-v", "20", "--amp", "--bilinear",
                  "-c", "1"])
    assert (b.epochs, b.batch_size, b.lr, b.load, b.scale, b.val, b.amp, b.bilinear, b.classes) == \
        (7, 4, 3e-4, "m.pth", 0.25, 20.0, True, True, 1)
    c = get_args(["--epochs", "2", "--batch-size", "3", "--learning-rate", "1e-3", "--load", "x", "--scale", "1",
                  "--validation", "5", "--classes", "2", "--no-amp", "--model", "UNet_SA", "--seed", "4", "--workers", "2"])
    assert (c.epochs, c.batch_size, c.lr, c.load, c.scale, c.val, c.amp, c.classes, c.model, c.seed, c.workers) == \
        (2, 3, 1e-3, "x", 1.0, 5.0, False, 2, "UNet_SA", 4, 2)
    with pytest.raises(SystemExit):
        get_args(["--model", "UNetPlusPlus"])
    from unet_amd.train import get_args as via_train
    assert vars(via_train([])) == vars(a)


def _reference_cadence(n_train, batch_size, epochs):
    """train.py:90-216, the loop with its data and model taken out."""
    evals, ckpts = [], []
    global_step = 0
    batches = [min(batch_size, n_train - i) for i in range(0, n_train, batch_size)]     # DataLoader(drop_last=False)
    for epoch in range(1, epochs + 1):
        for _ in batches:
            global_step += 1
            division_step = n_train // batch_size
            if division_step > 0:
                if global_step % division_step == 0:
                    evals.append((epoch, global_step))
        factor = 5
        if epoch > epochs * 0.5:
            if epoch % factor == 0:
                ckpts.append(epoch)
    return evals, ckpts


def test_cadence_matches_reference_loop():
    from unet_amd.train_cli import cadence
    for n_train in (1, 2, 3, 7, 8, 9, 16, 33, 100):
        for b in (1, 2, 3, 4, 8, 16, 200):
            for epochs in (1, 2, 5, 9, 10, 11, 20):
                evals, ckpts = _reference_cadence(n_train, b, epochs)
                got = cadence(n_train, b, epochs)
                assert got["eval_steps"] == evals, (n_train, b, epochs)
                assert got["checkpoint_epochs"] == ckpts, (n_train, b, epochs)
    # the cases the reference's wording hides: mid-epoch and twice per epoch, never when n_train < batch
    assert cadence(9, 4, 1)["eval_steps"] == [(1, 2)]
    assert cadence(5, 2, 1)["eval_steps"] == [(1, 2)] and cadence(5, 2, 2)["eval_steps"] == [(1, 2), (2, 4), (2, 6)]
    assert cadence(3, 4, 3)["eval_steps"] == []
    assert cadence(8, 2, 10)["checkpoint_epochs"] == [10] and cadence(8, 2, 20)["checkpoint_epochs"] == [15, 20]


def _tree(tmp_path):
    r = load_golden("g12_data_loading")
    _write_tree(tmp_path, r)
    return r


def test_loader_order_is_seeded_and_drops_last(tmp_path):
    from unet_amd.utils.data_loading import BasicDataset, DeviceBatchLoader
    _tree(tmp_path)
    ds = BasicDataset(str(tmp_path / "imgs"), str(tmp_path / "masks"), 0.5, augment=True)
    n = len(ds)
    a = DeviceBatchLoader(ds, 5, shuffle=True, drop_last=False, seed=3)
    b = DeviceBatchLoader(ds, 5, shuffle=True, drop_last=False, seed=3)
    c = DeviceBatchLoader(ds, 5, shuffle=True, drop_last=False, seed=4)
    for e in range(3):
        assert a.epoch_order(e) == b.epoch_order(e) and sorted(a.epoch_order(e)) == list(range(n))
    assert a.epoch_order(0) != a.epoch_order(1) and a.epoch_order(0) != c.epoch_order(0)
    sizes = [len(x) for x in a.batches_of(a.epoch_order(0))]
    assert sizes == [5] * (n // 5) + ([n % 5] if n % 5 else []) and len(a) == len(sizes)
    v = DeviceBatchLoader(ds, 5, shuffle=False, drop_last=True)
    assert v.epoch_order(0) == v.epoch_order(7) == list(range(n))
    vb = v.batches_of(v.epoch_order(0))
    assert [len(x) for x in vb] == [5] * (n // 5) and len(v) == n // 5 and sum(vb, []) == list(range(n // 5 * 5))
    unseeded = DeviceBatchLoader(ds, 5, shuffle=True)
    assert unseeded.epoch_order(0) == unseeded.epoch_order(0)                 # one draw per loader, fixed afterwards


@pytest.mark.parametrize("scale", [0.5, 0.37])
def test_raw_items_without_host_rescale(tmp_path, scale):
    """raw_item(host_rescale=False) hands over decoded bytes + turns + scale; the restated rescale then the oracle's
    arithmetic give the reference's item (ds[i]).  The default keeps rescaling on the host."""
    from oracle import data_prep_ref as R
    from unet_amd.utils.data_loading import BasicDataset, collate_raw
    r = _tree(tmp_path)
    ds = BasicDataset(str(tmp_path / "imgs"), str(tmp_path / "masks"), scale, augment=True)
    for i in range(len(ds)):
        raw = ds.raw_item(i, host_rescale=False)
        n = ds.ids[i // 4]
        assert np.array_equal(raw["image_u8"], r[f"raw.{n}.img"]) and raw["turns"] == i % 4 and raw["scale"] == scale
        img, mask = RR.dataset_rescale(raw["image_u8"], raw["mask_u8"], raw["turns"], raw["scale"])
        want_i, want_m = R.prepare_item(img, mask, 0)
        item = ds[i]
        assert np.array_equal(want_i, item["image"].numpy()) and np.array_equal(want_m, item["mask"].numpy())
        if scale == 0.5:
            assert np.array_equal(want_i, r[f"s0.5.{n}.r{i % 4}.image"])           # the reference's own items (G12)
        host = ds.raw_item(i)
        assert host["turns"] == 0 and host["scale"] == 1.0 and np.array_equal(host["image_u8"], img)
    b = collate_raw([ds.raw_item(0, host_rescale=False), ds.raw_item(2, host_rescale=False)], pin=False)
    assert b["scale"] == scale and b["turns"].tolist() == [0, 2]
    with pytest.raises(ValueError):
        collate_raw([ds.raw_item(0, host_rescale=False), ds.raw_item(2)], pin=False)     # two scales in one batch


def test_main_refuses_a_machine_without_gpu(tmp_path, monkeypatch, caplog):
    from unet_amd import train_cli
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    rc = train_cli.main(["-e", "1", "--data-root", str(tmp_path)])
    assert rc != 0
    assert "no GPU" in caplog.text
    assert not (tmp_path / "model_epoch1.pth").exists()


def test_device_rescale_has_no_cpu_fallback():
    from unet_amd.utils.data_loading import prepare_batch_device
    u8 = torch.zeros(2, 8, 12, 1, dtype=torch.uint8)
    with pytest.raises(RuntimeError):
        prepare_batch_device(u8, torch.zeros(2, 8, 12, dtype=torch.uint8), device="cpu", scale=0.5)
    with pytest.raises(ValueError):
        prepare_batch_device(torch.zeros(2, 8, 12, 2, dtype=torch.uint8), torch.zeros(2, 8, 12, dtype=torch.uint8),
                             device="cuda", scale=0.5)
    from unet_amd.utils.data_rescale import rescaled_size
    assert rescaled_size(1024, 768, 0.5) == (512, 384) and rescaled_size(7, 5, 0.37) == (2, 1)
    with pytest.raises(ValueError):
        rescaled_size(3, 7, 0.25)
