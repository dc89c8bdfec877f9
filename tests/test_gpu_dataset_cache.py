"""The device-resident dataset cache on the MI355X (csrc/cache.hip, utils/dataset_cache.py, DeviceBatchLoader(cache=...),
`train --cache`): the gather kernel against numpy with canaries round its outputs, its error codes, the cached loader against
the uncached one bit for bit, one decode per file, the limits, and the command line in child processes."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu

ROWS_PER_LAUNCH = 32            # csrc/cache.hip: CACHE_ROWS (test_rows_per_launch_is_what_the_source_says)
CANARY, GUARD = 0xA5, 64
SHAPES = [(5, 7, 1), (16, 16, 1), (33, 31, 3), (64, 48, 4)]
ENTRIES = 5
ORDERS = {1: [2], 3: [3, 1, 1], ROWS_PER_LAUNCH + 1: [ENTRIES - 1 - (i % ENTRIES) for i in range(ROWS_PER_LAUNCH + 1)]}
UH_EINVAL = -1


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _call(table, B, image_bytes, mask_bytes, image_out, mask_out):
    """uh_cache_gather_u8 through the C ABI: the return code, not an exception."""
    from unet_amd._lib import LIB
    return LIB.query("uh_cache_gather_u8", None if table is None else table.ctypes.data, B, image_bytes, mask_bytes, image_out,
                     mask_out, _stream())


def _guarded(nbytes):
    """A device buffer of `nbytes` with GUARD canary bytes on each side, inside a larger canary-filled allocation."""
    whole = torch.full((GUARD + nbytes + GUARD,), CANARY, dtype=torch.uint8, device=_dev())
    assert whole.data_ptr() % 16 == 0
    return whole, whole.data_ptr() + GUARD


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "x".join(map(str, s)))
def arena(request):
    """ENTRIES random entries of one shape in a plan_entries arena whose padding holds a value no entry byte is compared with."""
    from unet_amd import plan_entries
    H, W, C = request.param
    rng = np.random.default_rng(H * 1000 + W)
    io, mo, total = plan_entries([request.param] * ENTRIES)
    host = np.full(total, 0x3C, np.uint8)
    images = [rng.integers(0, 256, H * W * C, dtype=np.uint8) for _ in range(ENTRIES)]
    masks = [rng.integers(0, 256, H * W, dtype=np.uint8) for _ in range(ENTRIES)]
    for e in range(ENTRIES):
        host[io[e]:io[e] + H * W * C] = images[e]
        host[mo[e]:mo[e] + H * W] = masks[e]
    dev = torch.from_numpy(host).to(_dev())
    assert dev.data_ptr() % 16 == 0
    return {"dev": dev, "io": io, "mo": mo, "images": images, "masks": masks, "ib": H * W * C, "mb": H * W}


def test_rows_per_launch_is_what_the_source_says():
    src = open(os.path.join(ROOT, "unet-medical-image-contour-segmentation_amd", "csrc", "cache.hip")).read()
    assert f"constexpr int CACHE_ROWS = {ROWS_PER_LAUNCH};" in src


@pytest.mark.parametrize("form", ["both", "image", "mask"])
@pytest.mark.parametrize("B", sorted(ORDERS))
def test_gather_kernel_against_numpy_with_canaries(arena, B, form):
    order = ORDERS[B]
    base = arena["dev"].data_ptr()
    want_i, want_m = form != "mask", form != "image"
    table = np.zeros((B, 2), np.uint64)
    for b, e in enumerate(order):
        table[b, 0] = base + arena["io"][e] if want_i else 0            # a row's pointer for a null output may be null
        table[b, 1] = base + arena["mo"][e] if want_m else 0
    ib, mb = arena["ib"], arena["mb"]
    img, img_p = _guarded(B * ib)
    msk, msk_p = _guarded(B * mb)
    rc = _call(table, B, ib, mb, img_p if want_i else None, msk_p if want_m else None)
    torch.cuda.synchronize()
    assert rc == 0
    img, msk = img.cpu().numpy(), msk.cpu().numpy()
    for got, want, n, data in ((img, want_i, ib, arena["images"]), (msk, want_m, mb, arena["masks"])):
        assert (got[:GUARD] == CANARY).all() and (got[GUARD + B * n:] == CANARY).all(), "a canary was written"
        if want:
            assert np.array_equal(got[GUARD:GUARD + B * n], np.concatenate([data[e] for e in order]))
        else:
            assert (got == CANARY).all(), "an output that was not asked for was written"


def test_every_einval_case_returns_the_code_and_launches_nothing(arena):
    from unet_amd._lib import LIB
    base = arena["dev"].data_ptr()
    ib, mb = arena["ib"], arena["mb"]
    B = 3
    good = np.array([[base + arena["io"][e], base + arena["mo"][e]] for e in (0, 1, 2)], np.uint64)

    def rows(r, c, v):
        t = good.copy()
        t[r, c] = v
        return t

    img, ip = _guarded(B * ib + 16)
    msk, mp = _guarded(B * mb + 16)
    cases = {
        "items null": (None, B, ib, mb, ip, mp),
        "both outputs null": (good, B, ib, mb, None, None),
        "B = 0": (good, 0, ib, mb, ip, mp),
        "B < 0": (good, -1, ib, mb, ip, mp),
        "zero image length": (good, B, 0, mb, ip, mp),
        "zero mask length": (good, B, ib, 0, ip, mp),
        "zero image length, image only": (good, B, 0, mb, ip, None),
        "misaligned image_out": (good, B, ib, mb, ip + 8, mp),
        "misaligned mask_out": (good, B, ib, mb, ip, mp + 1),
        "null image row": (rows(1, 0, 0), B, ib, mb, ip, mp),
        "null mask row": (rows(2, 1, 0), B, ib, mb, ip, mp),
        "misaligned image row": (rows(0, 0, int(good[0, 0]) + 4), B, ib, mb, ip, mp),
        "misaligned mask row": (rows(2, 1, int(good[2, 1]) + 8), B, ib, mb, ip, mp),
    }
    for name, args in cases.items():
        assert _call(*args) == UH_EINVAL, name
        assert b"uh_cache_gather_u8" in LIB.query("uh_last_error"), name
    torch.cuda.synchronize()
    assert bool((img == CANARY).all()) and bool((msk == CANARY).all()), "a refused call wrote to an output"
    # the null forms the header allows are not errors
    assert _call(rows(1, 1, 0), B, ib, 0, ip, None) == 0 and _call(rows(1, 0, 0), B, 0, mb, None, mp) == 0
    torch.cuda.synchronize()


def test_ops_wrapper_names_the_argument(arena):
    from unet_amd import ops
    ib, mb = arena["ib"], arena["mb"]
    dev = arena["dev"]
    pair = lambda e: (dev[arena["io"][e]:arena["io"][e] + ib], dev[arena["mo"][e]:arena["mo"][e] + mb])
    image, mask = ops.cache_gather([pair(4), pair(0), pair(4)], ib, mb)
    assert tuple(image.shape) == (3, ib) and tuple(mask.shape) == (3, mb)
    assert np.array_equal(image.cpu().numpy(), np.stack([arena["images"][e] for e in (4, 0, 4)]))
    assert np.array_equal(mask.cpu().numpy(), np.stack([arena["masks"][e] for e in (4, 0, 4)]))
    image, mask = ops.cache_gather([(None, pair(1)[1])], ib, mb, want_image=False)
    assert image is None and np.array_equal(mask.cpu().numpy()[0], arena["masks"][1])
    with pytest.raises(RuntimeError, match=r"rows\[0\] image"):
        ops.cache_gather([(pair(0)[0].cpu(), pair(0)[1])], ib, mb)
    with pytest.raises(RuntimeError, match=r"rows\[1\] mask"):
        ops.cache_gather([pair(0), (pair(1)[0], dev[0:2 * mb:2])], ib, mb)
    with pytest.raises(RuntimeError, match="image_bytes"):
        ops.cache_gather([pair(0)], ib + 1, mb)
    with pytest.raises(ValueError):
        ops.cache_gather([], ib, mb)
    with pytest.raises(ValueError):
        ops.cache_gather([pair(0)], ib, mb, want_image=False, want_mask=False)


# ------------------------------------------------------------------------------------------------------------ folders
def _write_pairs(top, sizes, channels=1, bits=8, seed=0):
    """imgs/ and masks/ under `top`: one random PNG pair per (H, W) of `sizes`, masks coded 0 / 128 / 255."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    grey = np.array([0, 128, 255], np.uint8)
    os.makedirs(os.path.join(top, "imgs"))
    os.makedirs(os.path.join(top, "masks"))
    for i, (H, W) in enumerate(sizes):
        if bits == 16:
            pixels = rng.integers(0, 65536, (H, W), dtype=np.uint16)
        else:
            pixels = rng.integers(0, 256, (H, W) if channels == 1 else (H, W, channels), dtype=np.uint8)
        Image.fromarray(pixels).save(os.path.join(top, "imgs", f"p{i:02d}.png"))
        Image.fromarray(grey[rng.integers(0, 3, (H, W))]).save(os.path.join(top, "masks", f"p{i:02d}_mask.png"))
    return top


def _dataset(top, scale=1.0, augment=True):
    from unet_amd import BasicDataset
    return BasicDataset(os.path.join(top, "imgs"), os.path.join(top, "masks"), scale, augment=augment)


@pytest.fixture(scope="module")
def folders(tmp_path_factory):
    top = tmp_path_factory.mktemp("dataset_cache")
    return {"grey": _write_pairs(str(top / "grey"), [(32, 32)] * 6, seed=1),
            "rgb": _write_pairs(str(top / "rgb"), [(24, 40)] * 6, channels=3, seed=2),
            "mixed": _write_pairs(str(top / "mixed"), [(48, 40), (64, 64), (48, 40), (64, 64), (64, 64), (48, 40)], seed=3),
            "deep": _write_pairs(str(top / "deep"), [(32, 32)] * 3, bits=16, seed=4)}


def _assert_same_epochs(plain, cached, epochs=3):
    batches = 0
    for _ in range(epochs):
        a, b = list(plain), list(cached)
        assert len(a) == len(b) == len(plain)
        for x, y in zip(a, b):
            assert x["image"].dtype == y["image"].dtype and x["image"].shape == y["image"].shape
            assert torch.equal(x["image"], y["image"]) and torch.equal(x["mask"], y["mask"])
            batches += 1
    assert plain.orders == cached.orders and len(cached.orders) == epochs
    return batches


@pytest.mark.parametrize("scale", [1.0, 0.5])
@pytest.mark.parametrize("folder", ["grey", "rgb"])
def test_cached_loader_is_the_uncached_loader_bit_for_bit(folders, folder, scale):
    from unet_amd import DatasetCache
    from unet_amd.utils.data_loading import DeviceBatchLoader
    ds = _dataset(folders[folder], scale, augment=(folder == "grey"))       # non-square items stack without quarter turns only
    cache = DatasetCache(ds, workers=4)
    assert cache.entries == 6 and cache.decodes == 12 and cache.nbytes == 6 * (2048 if folder == "grey" else 2880 + 960)
    kw = dict(batch_size=4, shuffle=True, seed=11, workers=4)
    assert _assert_same_epochs(DeviceBatchLoader(ds, **kw), DeviceBatchLoader(ds, cache=cache, **kw)) == 3 * (6 if folder == "grey" else 2)
    raw = cache.gather([1, 0])
    assert raw["image_u8"].is_cuda and tuple(raw["image_u8"].shape) == ((2, 32, 32, 1) if folder == "grey" else (2, 24, 40, 3))
    assert raw["turns"].tolist() == ([1, 0] if folder == "grey" else [0, 0]) and raw["scale"] == scale
    cache.close()
    with pytest.raises(RuntimeError, match="closed"):
        cache.gather([0])


def test_cached_loader_with_augment_and_elastic(folders):
    from unet_amd import BatchAugment
    from unet_amd.utils.data_loading import DeviceBatchLoader
    ds = _dataset(folders["grey"])
    kw = dict(batch_size=4, shuffle=True, seed=5, workers=4)
    plain = DeviceBatchLoader(ds, augment=BatchAugment("default", 5, elastic="grid=16,sigma=1"), **kw)
    cached = DeviceBatchLoader(ds, augment=BatchAugment("default", 5, elastic="grid=16,sigma=1"), cache=True, **kw)
    assert cached.cache is not None and cached.cache.ds is ds
    _assert_same_epochs(plain, cached)


@pytest.mark.parametrize("scale", [1.0, 0.5])
def test_cached_loader_with_crop_on_mixed_sizes(folders, scale):
    from unet_amd import BatchCrop
    from unet_amd.utils.data_loading import DeviceBatchLoader
    ds = _dataset(folders["mixed"], scale)
    kw = dict(batch_size=4, shuffle=True, seed=7, workers=4)
    plain = DeviceBatchLoader(ds, crop=BatchCrop("16", 7, 3), **kw)
    cached = DeviceBatchLoader(ds, crop=BatchCrop("16", 7, 3), cache=True, **kw)
    _assert_same_epochs(plain, cached)
    shapes = cached.cache.shapes                                              # decoded, whatever the scale
    a, b = shapes.index((48, 40, 1)), shapes.index((64, 64, 1))
    groups = cached.cache.gather_groups([4 * a, 4 * b, 4 * a + 1, 4 * b + 1, 4 * a + 2])["groups"]
    assert [pos for pos, _ in groups] == [[0, 4], [1, 3], [2]]              # 48x40 even turns, 64x64, 48x40 odd turn
    assert [tuple(g["image_u8"].shape) for _, g in groups] == [(2, 48, 40, 1), (2, 64, 64, 1), (1, 48, 40, 1)]


def test_refusals(folders):
    from unet_amd import DatasetCache
    from unet_amd.utils.data_loading import DeviceBatchLoader
    mixed, grey = _dataset(folders["mixed"]), _dataset(folders["grey"])
    said = []
    for cache in (None, True):
        with pytest.raises(ValueError) as e:
            list(DeviceBatchLoader(mixed, batch_size=len(mixed), workers=4, cache=cache))
        said.append(str(e.value))
    assert said[0] == said[1] == "collate_raw: the items of a batch must have one decoded size"
    rgb = _dataset(folders["rgb"])                                        # augment=True: odd and even turns of 24x40 in one batch
    said = []
    for cache in (None, True):
        with pytest.raises(ValueError) as e:
            list(DeviceBatchLoader(rgb, batch_size=4, workers=4, cache=cache))
        said.append(str(e.value))
    assert said[0] == said[1] and "odd and even quarter turns" in said[0]
    cache = DatasetCache(grey, workers=2)
    with pytest.raises(ValueError, match="host_rescale"):
        DeviceBatchLoader(grey, 4, host_rescale=True, cache=cache)
    with pytest.raises(ValueError, match="another dataset"):
        DeviceBatchLoader(_dataset(folders["grey"]), 4, cache=cache)
    with pytest.raises(ValueError, match="DatasetCache"):
        DeviceBatchLoader(grey, 4, cache="yes")


def test_one_decode_per_file(folders, monkeypatch):
    from unet_amd import DatasetCache
    from unet_amd.utils import data_loading
    from unet_amd.utils.data_loading import DeviceBatchLoader
    ds = _dataset(folders["grey"])
    files, calls = len(ds.ids), []
    real = data_loading.load_image

    def counted(path):
        calls.append(path)
        return real(path)

    monkeypatch.setattr(data_loading, "load_image", counted)
    cache = DatasetCache(ds, workers=4)
    assert len(calls) == 2 * files == cache.decodes
    kw = dict(batch_size=4, shuffle=True, seed=3, workers=4)
    cached = DeviceBatchLoader(ds, cache=cache, **kw)
    for _ in range(3):
        assert len(list(cached)) == 6
    assert len(calls) == 2 * files
    plain = DeviceBatchLoader(ds, **kw)
    for _ in range(3):
        assert len(list(plain)) == 6
    assert len(calls) - 2 * files == 2 * 4 * 3 * files
    assert cache.build_seconds > 0 and cache.entries == files


def test_limits(folders):
    from unet_amd import DatasetCache, DatasetCacheTooLarge
    from unet_amd.utils.data_loading import DeviceBatchLoader
    grey = _dataset(folders["grey"])
    with pytest.raises(DatasetCacheTooLarge) as e:
        DatasetCache(grey, limit_bytes=1024)
    assert isinstance(e.value, ValueError) and "1024" in str(e.value) and str(6 * 2048) in str(e.value)
    assert DatasetCache(grey, limit_bytes=6 * 2048).nbytes == 6 * 2048
    assert 0 < DatasetCache(grey).limit_bytes <= torch.cuda.mem_get_info()[1] // 2        # half of what is free
    deep = _dataset(folders["deep"])
    with pytest.raises(TypeError, match="8-bit"):
        DatasetCache(deep)
    kw = dict(batch_size=4, shuffle=True, seed=1, workers=4)
    plain, cached = DeviceBatchLoader(deep, **kw), DeviceBatchLoader(deep, cache=True, **kw)
    assert cached.cache is None and cached.host_items
    _assert_same_epochs(plain, cached, epochs=1)


# ------------------------------------------------------------------------------------------------------- command line
COMMON = ["-b", "2", "-s", "1", "--model", "UNet_T", "--seed", "0", "--workers", "4"]


def _run_cli(cwd, args, timeout=300):
    os.makedirs(cwd, exist_ok=True)
    r = subprocess.run([sys.executable, "-m", "unet_amd.train"] + args, capture_output=True, text=True, timeout=timeout,
                       cwd=str(cwd), env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, r.stderr[-4000:]
    return r.stderr


def _load(path):
    return torch.load(path, map_location="cpu", weights_only=True)


def _assert_same_weights(a, b):
    want, got = _load(a), _load(b)
    assert list(want) == list(got)
    for k in want:
        assert torch.equal(want[k], got[k]), k


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    from PIL import Image
    top = tmp_path_factory.mktemp("dataset_cache_cli")
    rng = np.random.default_rng(9)
    grey = np.array([0, 128, 255], np.uint8)
    for split, n in (("train", 6), ("val", 2)):
        for d in ("imgs", "masks"):
            os.makedirs(top / "data" / d / split)
        for i in range(n):
            Image.fromarray(rng.integers(0, 256, (32, 32), dtype=np.uint8)).save(top / "data" / "imgs" / split / f"p{i}.png")
            Image.fromarray(grey[rng.integers(0, 3, (32, 32))]).save(top / "data" / "masks" / split / f"p{i}_mask.png")
    base = COMMON + ["--data-root", str(top / "data")]
    logs = {"plain": _run_cli(top / "plain", base + ["-e", "2"]),
            "cache": _run_cli(top / "cache", base + ["-e", "2", "--cache"]),
            "small": _run_cli(top / "small", base + ["-e", "2", "--cache", "limit=0.000001"])}
    _run_cli(top / "resumed", base + ["-e", "1", "--save-state", "--checkpoint-dir", str(top / "resumed" / "ck")])
    logs["resumed"] = _run_cli(top / "resumed", base + ["-e", "2", "--cache", "--resume", str(top / "resumed" / "ck" / "train_state.pth"),
                                                        "--checkpoint-dir", str(top / "resumed" / "ck")])
    return top, logs


def test_cli_cache_does_not_change_the_weights(cli):
    top, logs = cli
    _assert_same_weights(top / "plain" / "model_epoch2.pth", top / "cache" / "model_epoch2.pth")
    first = _load(top / "resumed" / "model_epoch1.pth")
    assert any(not torch.equal(v, _load(top / "plain" / "model_epoch2.pth")[k]) for k, v in first.items())
    assert "Dataset cache (training): 6 files" in logs["cache"] and "Dataset cache (validation): 2 files" in logs["cache"]
    assert "MiB on the device, built in" in logs["cache"] and "Dataset cache" not in logs["plain"]


def test_cli_resume_takes_a_run_with_or_without_the_cache(cli):
    top, logs = cli
    _assert_same_weights(top / "plain" / "model_epoch2.pth", top / "resumed" / "model_epoch2.pth")
    assert "Resumed after epoch 1" in logs["resumed"] and "Dataset cache (training): 6 files" in logs["resumed"]
    assert "cache" not in _load(top / "resumed" / "ck" / "train_state.pth")["args"]


def test_cli_set_over_the_limit_is_served_uncached_with_a_warning(cli):
    top, logs = cli
    _assert_same_weights(top / "plain" / "model_epoch2.pth", top / "small" / "model_epoch2.pth")
    for what in ("training", "validation"):
        assert f"WARNING: Dataset cache ({what}): not cached" in logs["small"]
    assert "over the limit of 1073 bytes" in logs["small"] and "MiB on the device" not in logs["small"]
