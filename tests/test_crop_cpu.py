"""CPU checks of patch training (DESIGN.md section 3 "Patch training"): CropConfig and its spec parser, the per-item words
against the numpy restatement tests/crop_ref.py, properties of that restatement itself, the argument checks of the library's
entry points (host-only: they return before any launch) and the command line's record of --crop / --tile."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import crop_ref as R  # noqa: E402

from conftest import GOLDEN  # noqa: E402


# ------------------------------------------------------------------------------------------------------------- config
def test_config_parse_and_spec_round_trip():
    import unet_amd
    from unet_amd.utils.crop import DEFAULT_SPEC, CropConfig, crop_config
    assert unet_amd.CropConfig is CropConfig
    assert CropConfig() == CropConfig(256, 0.5, None) == CropConfig.parse("") == CropConfig.parse("256") == CropConfig.parse(DEFAULT_SPEC)
    assert DEFAULT_SPEC == "256,fg=0.5" == CropConfig().spec()
    cfg = CropConfig.parse("256,fg=0.7,classes=1+2")
    assert cfg == CropConfig(256, 0.7, (1, 2)) and cfg.spec() == "256,fg=0.7,classes=1+2"
    assert CropConfig.parse(" 64 , classes = 2+1 , fg = 1 ").spec() == "64,fg=1.0,classes=1+2"        # canonical: sorted, repr
    for spec in ("16", "32,fg=0", "48,fg=1", "512,fg=0.25,classes=0", "16384,classes=63+0+5"):
        cfg = CropConfig.parse(spec)
        assert CropConfig.parse(cfg.spec()) == cfg and CropConfig.parse(cfg.spec()).spec() == cfg.spec()
    assert crop_config(None) is None and crop_config("32") == CropConfig(32) == crop_config(CropConfig(32))
    assert CropConfig(32, 1).threshold == 1 << 32 and CropConfig(32, 0).threshold == 0 and CropConfig(32, 0.5).threshold == 1 << 31
    assert CropConfig(32, 0.7).threshold == int(np.rint(0.7 * 2.0 ** 32)) == R.threshold(0.7)
    assert CropConfig(32, 0.5, (1, 2)).class_mask == 6 == R.class_mask((1, 2))


@pytest.mark.parametrize("spec,token", [
    ("24", "24"), ("8", "8"), ("0", "0"), ("16400", "16400"), ("-32", "-32"), ("32.0", "32.0"), ("abc", "abc"),
    ("32,fg=1.5", "1.5"), ("32,fg=-0.1", "-0.1"), ("32,fg=x", "fg=x"), ("32,fg=", "fg="), ("32,fg", "fg"), ("32,fg=nan", "nan"),
    ("32,classes=64", "64"), ("32,classes=-1", "-1"), ("32,classes=1+1", "1, 1"), ("32,classes=a", "classes=a"),
    ("32,classes=", "classes="), ("32,classes=1+", "classes=1+"), ("32,overlap=8", "overlap=8"), ("32,fg=0.5,fg=0.5", "fg=0.5"),
    ("32,", "''"), ("32;fg=1", "32;fg=1")])
def test_parse_errors_name_the_token(spec, token):
    from unet_amd.utils.crop import CropConfig
    with pytest.raises(ValueError) as e:
        CropConfig.parse(spec)
    assert token in str(e.value), str(e.value)


def test_config_refusals():
    from unet_amd.utils.crop import CropConfig, crop_config
    for size in (24, 8, 0, -16, 16400, 32.0, "32", True, None):
        with pytest.raises(ValueError, match="size"):
            CropConfig(size)
    for fg in (1.5, -0.1, float("nan"), "0.5", None, True):
        with pytest.raises(ValueError, match="fg"):
            CropConfig(32, fg)
    for classes in ((64,), (-1,), (1, 1), (), (1.5,), 2, ("1",)):
        with pytest.raises(ValueError, match="classes"):
            CropConfig(32, 0.5, classes)
    for spec in (None, 32):
        with pytest.raises(ValueError):
            CropConfig.parse(spec)
    with pytest.raises(ValueError):
        crop_config(32)
    with pytest.raises(ValueError, match="unresolved"):
        CropConfig(32).class_mask


def test_class_defaults_per_head():
    from unet_amd.utils.crop import BatchCrop, CropConfig
    from unet_amd.utils.surface_loss import default_classes
    for n in (3, 4, 7):
        assert CropConfig(32).for_head(n).classes == (2,) == default_classes(n)
    assert CropConfig(32).for_head(1).classes == (1,) == default_classes(1)
    with pytest.raises(ValueError, match="2-class head"):
        CropConfig(32).for_head(2)
    assert CropConfig(32, 0.5, (1,)).for_head(2).classes == (1,)
    assert CropConfig(32, 0.5, (0, 1)).for_head(2).classes == (0, 1)
    assert CropConfig(32, 0.5, (1, 2)).for_head(3).classes == (1, 2)
    assert CropConfig(32, 0.5, (2,)).for_head(1).classes == (2,)                    # the binary head trains on the labels 0..2
    for classes, n in (((3,), 3), ((2,), 2), ((1, 5), 4), ((3,), 1)):
        with pytest.raises(ValueError, match="do not fit"):
            CropConfig(32, 0.5, classes).for_head(n)
    assert BatchCrop("32,fg=0.25", seed=7, n_classes=3).config == CropConfig(32, 0.25, (2,))
    with pytest.raises(ValueError):
        BatchCrop("32", seed=7, n_classes=2)


# -------------------------------------------------------------------------------------------------------------- words
def test_words_equal_the_reference():
    from unet_amd.utils.crop import BatchCrop
    for seed in (0, 1, 12345, (1 << 40) + 17, (1 << 62) - 1):
        crop = BatchCrop("32", seed, 3)
        for epoch in (0, 1, 7, (1 << 32) - 1):
            idx = [0, 1, 2, 3, 100, 65536, (1 << 32) - 1]
            w = crop.words(epoch, idx)
            assert w.dtype == np.uint32 and w.shape == (len(idx), 4)
            assert np.array_equal(w, R.words(seed, epoch, idx))
    crop = BatchCrop("32", 5, 3)
    assert np.array_equal(crop.words(2, [9, 3])[1], crop.words(2, [3])[0])                         # a row depends on its index only
    assert not np.array_equal(crop.words(0, [3]), crop.words(1, [3]))
    assert crop.words(0, []).shape == (0, 4)
    for epoch, idx in ((-1, [0]), (1 << 32, [0]), (0, [-1]), (0, [1 << 32])):
        with pytest.raises(ValueError, match="32-bit"):
            crop.words(epoch, idx)


def test_words_are_draw_4_of_the_augmenter_scheme():
    """Counter (index, epoch, 4, 0) under the augmenter's key: its own draws 0..3 stay its own."""
    from unet_amd.utils.augment import BatchAugment
    from unet_amd.utils.crop import BatchCrop
    aug, crop = BatchAugment("flip", seed=11), BatchCrop("32", 11, 3)
    idx = np.array([0, 5, 77], np.int64)
    five = aug._draw_words(3, idx, 5)
    assert np.array_equal(five[:, 4], crop.words(3, idx))
    for d in range(4):
        assert not np.array_equal(five[:, d], crop.words(3, idx))


def test_augment_draws_are_the_parents():
    """BatchAugment.draws is what it was before the crop stream existed: recorded from the parent commit."""
    from unet_amd.utils.augment import BatchAugment
    g = dict(np.load(os.path.join(GOLDEN, "augment_draws_parent.npz"), allow_pickle=False))
    spec = "flip,rotate=15,scale=0.1,translate=0.05,brightness=0.1,contrast=0.1,gamma=0.2,noise=0.01"
    for seed, epoch in ((0, 0), (3, 2), ((1 << 40) + 9, 5)):
        d = BatchAugment(spec, seed=seed).draws(epoch, [0, 1, 2, 17, 4000], (96, 128))
        for k, v in d.items():
            want = g[f"s{seed}_e{epoch}_{k}"]
            assert v.dtype == want.dtype and np.array_equal(v, want), (seed, epoch, k)


# ------------------------------------------------------------------------------------- properties of the reference itself
def _plane(rng, H, W, density):
    lab = rng.integers(0, 2, (H, W)).astype(np.int64)
    lab[rng.random((H, W)) < density] = 2
    return lab


def test_reference_fg_one_puts_the_picked_pixel_inside_every_crop():
    rng = np.random.default_rng(0)
    uniform_pos = 0
    for H, W, size in ((16, 16, 16), (40, 56, 32), (33, 70, 16), (64, 48, 48)):
        lab = _plane(rng, H, W, 0.02)
        lab[0, 0] = lab[H - 1, W - 1] = 2
        for r in rng.integers(0, 1 << 32, (200, 4), dtype=np.uint64):
            oy, ox, n, picked = R.select(lab, r, size, 1 << 2, 1 << 32)
            assert n == int((lab == 2).sum()) and picked is not None
            py, px = picked
            assert lab[py, px] == 2 and oy <= py < oy + size and ox <= px < ox + size
            assert 0 <= oy <= H - size and 0 <= ox <= W - size
            jy, jx = (int(r[2]) * size) >> 32, (int(r[3]) * size) >> 32
            uniform_pos += (py - oy, px - ox) == (jy, jx)                            # unless the border clamps it
    assert uniform_pos > 0


def test_reference_fg_zero_or_no_foreground_takes_the_uniform_branch():
    rng = np.random.default_rng(1)
    H, W, size = 40, 56, 32
    lab = _plane(rng, H, W, 0.05)
    empty = np.where(lab == 2, 1, lab)
    for r in rng.integers(0, 1 << 32, (100, 4), dtype=np.uint64):
        want = ((int(r[2]) * (H - size + 1)) >> 32, (int(r[3]) * (W - size + 1)) >> 32)
        oy, ox, n, picked = R.select(lab, r, size, 1 << 2, 0)                       # fg = 0: r0 < 0 never holds
        assert (oy, ox) == want and picked is None and n > 0
        oy, ox, n, picked = R.select(empty, r, size, 1 << 2, 1 << 32)               # n = 0
        assert (oy, ox) == want and picked is None and n == 0
    r = np.array([1 << 31, 0, 0xFFFFFFFF, 0xFFFFFFFF], np.uint64)
    assert R.select(lab, r, size, 1 << 2, 1 << 31)[3] is None                       # r0 < T is strict
    r[0] -= 1
    assert R.select(lab, r, size, 1 << 2, 1 << 31)[3] is not None
    assert R.select(empty, r, size, 1 << 2, 0)[:2] == (H - size, W - size)          # the last origin is reachable, never passed


def test_reference_rank_extremes_and_label_range():
    rng = np.random.default_rng(2)
    lab = _plane(rng, 37, 53, 0.03)
    fg = np.flatnonzero(lab.reshape(-1) == 2)
    first, last = divmod(int(fg[0]), 53), divmod(int(fg[-1]), 53)
    assert R.select(lab, (0, 0, 5, 5), 16, 1 << 2, 1 << 32)[3] == first
    assert R.select(lab, (0, 0xFFFFFFFF, 5, 5), 16, 1 << 2, 1 << 32)[3] == last
    n = fg.size
    for k in range(n):                                                               # r1 = ceil(k 2^32 / n) is the first word of rank k
        r1 = -((-k << 32) // n)
        assert R.select(lab, (0, r1, 0, 0), 16, 1 << 2, 1 << 32)[3] == divmod(int(fg[k]), 53)
    odd = lab.copy()
    odd[0, :4] = (-1, 64, 255, 66)                                                   # 66 = 64 + 2: no wrap onto bit 2
    assert np.array_equal(R.foreground(odd, (1 << 64) - 1), np.flatnonzero((odd.reshape(-1) >= 0) & (odd.reshape(-1) < 64)))
    assert R.select(odd, (0, 0, 0, 0), 16, 1 << 2, 1 << 32)[2] == int((odd == 2).sum())
    assert np.array_equal(R.foreground(lab, 0b110), np.flatnonzero(lab.reshape(-1) >= 1))


# --------------------------------------------------------------------------------------------- the library's refusals
def test_entry_points_declared_and_exported():
    import unet_amd  # noqa: F401
    from unet_amd._lib import LIB, LIB_PATH
    from unet_amd.utils.crop import ITEM_DTYPE
    dll = ctypes.CDLL(LIB_PATH)
    for name in ("uh_crop_select_ws_bytes", "uh_crop_select", "uh_crop_gather"):
        assert name in LIB.protos, f"{name} is not declared in include/unet_hip.h"
        assert hasattr(dll, name), f"{name} is not exported"
    assert LIB.protos["uh_crop_select_ws_bytes"] == ("size_t", ["int"])
    assert LIB.protos["uh_crop_select"][1] == ["ptr", "int", "int", "uint64_t", "uint64_t", "ptr", "ptr", "ptr", "size_t", "uh_stream"]
    assert LIB.protos["uh_crop_gather"][1] == ["ptr"] + ["int"] * 4 + ["ptr", "ptr", "int", "ptr", "uh_stream"]
    assert ITEM_DTYPE.itemsize == 48
    assert LIB.query("uh_crop_select_ws_bytes", 0) == 0 and LIB.query("uh_crop_select_ws_bytes", -3) == 0
    assert LIB.query("uh_crop_select_ws_bytes", 8) == 8 * LIB.query("uh_crop_select_ws_bytes", 1) > 0


def test_arguments_are_checked_before_any_launch():
    import unet_amd  # noqa: F401
    from unet_amd._lib import LIB
    from unet_amd.utils.crop import ITEM_DTYPE
    LIB.load()
    p = 4096                                                            # a non-null pointer that is never dereferenced
    F32, BF16 = 0, 1
    need = LIB.query("uh_crop_select_ws_bytes", 2)

    def table(B=2, **kw):
        t = np.zeros(max(B, 1), ITEM_DTYPE)
        t["image"], t["labels"], t["H"], t["W"], t["ld"] = p, p, 40, 56, 1
        for k, v in kw.items():
            t[k][-1] = v                                           # the last row is the odd one: every row is looked at
        return t

    def select(t=None, B=2, size=32, mask=4, T=1 << 31, origin=p, count=p, ws=p, ws_bytes=need, items=True):
        t = table(B) if t is None else t
        LIB.call("uh_crop_select", t.ctypes.data if items else None, B, size, mask, T, origin, count, ws, ws_bytes, None)

    def gather(t=None, B=2, C=1, dt=F32, size=32, origin=p, image_out=p, ld_out=None, labels_out=p, items=True):
        t = table(B) if t is None else t
        LIB.call("uh_crop_gather", t.ctypes.data if items else None, B, C, dt, size, origin, image_out, C if ld_out is None else ld_out,
                 labels_out, None)

    for fn, name in ((select, "uh_crop_select"), (gather, "uh_crop_gather")):
        with pytest.raises(RuntimeError, match=name + ".*null pointer"):
            fn(items=False)
        with pytest.raises(RuntimeError, match=name + ".*null pointer"):
            fn(origin=None)
        with pytest.raises(RuntimeError, match=name + ".*null pointer"):
            fn(t=table(labels=0))
        with pytest.raises(RuntimeError, match=name + ".*misaligned"):
            fn(origin=p + 2)
        with pytest.raises(RuntimeError, match=name + ".*misaligned"):
            fn(t=table(labels=p + 4))
        for size in (0, 8, 24, -16, 16400, 100):
            with pytest.raises(RuntimeError, match=name + ".*bad size"):
                fn(size=size)
        for B in (0, -1):
            with pytest.raises(RuntimeError, match=name + ".*bad batch"):
                fn(B=B)
        for kw in (dict(H=16385), dict(W=16385), dict(H=0), dict(W=-4)):
            with pytest.raises(RuntimeError, match=name + ".*bad sizes"):
                fn(t=table(**kw))
        for kw in (dict(H=31), dict(W=31)):
            with pytest.raises(RuntimeError, match=name + ".*row 1 is smaller than the crop"):
                fn(t=table(**kw))
        with pytest.raises(RuntimeError, match=name + ".*row 0 is smaller than the crop"):
            fn(size=48)
    with pytest.raises(RuntimeError, match="uh_crop_select.*null pointer"):
        select(ws=None)
    with pytest.raises(RuntimeError, match="uh_crop_select.*misaligned"):
        select(count=p + 1)
    with pytest.raises(RuntimeError, match="uh_crop_select.*misaligned"):
        select(ws=p + 2)
    with pytest.raises(RuntimeError, match="uh_crop_select.*fg_threshold"):
        select(T=(1 << 32) + 1)
    with pytest.raises(RuntimeError, match="uh_crop_select.*fg_threshold"):
        select(T=(1 << 64) - 1)
    with pytest.raises(RuntimeError, match="uh_crop_select.*workspace too small"):
        select(ws_bytes=need - 1)
    with pytest.raises(RuntimeError, match="uh_crop_select.*workspace too small"):
        select(ws_bytes=0)
    with pytest.raises(RuntimeError, match="uh_crop_gather.*null pointer"):
        gather(image_out=None, labels_out=None)                         # no output at all
    with pytest.raises(RuntimeError, match="uh_crop_gather.*null pointer"):
        gather(t=table(image=0))
    for C in (0, 5, -1):
        with pytest.raises(RuntimeError, match="uh_crop_gather.*bad channels"):
            gather(C=C)
    with pytest.raises(RuntimeError, match="uh_crop_gather.*bad pixel stride"):
        gather(C=3, t=table(ld=2))                                      # ld < C in the last row (the others hold 1: refused too)
    with pytest.raises(RuntimeError, match="uh_crop_gather.*bad pixel stride"):
        t = table()
        t["ld"] = 3
        gather(C=3, t=t, ld_out=2)
    for dt in (2, 3, -1):
        with pytest.raises(RuntimeError, match="uh_crop_gather.*bad dtype"):
            gather(dt=dt)
    with pytest.raises(RuntimeError, match="uh_crop_gather.*misaligned"):
        gather(image_out=p + 2)                                         # fp32 at an odd half-word
    with pytest.raises(RuntimeError, match="uh_crop_gather.*misaligned"):
        gather(image_out=p + 1, dt=BF16)
    with pytest.raises(RuntimeError, match="uh_crop_gather.*misaligned"):
        gather(labels_out=p + 4)
    with pytest.raises(RuntimeError, match="uh_crop_gather.*misaligned"):
        gather(t=table(image=p + 2))
    with pytest.raises(RuntimeError, match="uh_crop_gather.*misaligned"):
        gather(t=table(image=p + 1), dt=BF16)


def test_no_cpu_fallback():
    import torch
    import unet_amd
    from unet_amd import ops
    lab = torch.zeros(40, 56, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.crop_select([lab], np.zeros((1, 4), np.uint32), 32, 4, 1 << 31)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.crop_gather([torch.zeros(1, 40, 56)], [lab], torch.zeros(1, 2, dtype=torch.int32), 32)
    crop = unet_amd.BatchCrop("32", 0, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        crop([{"image": torch.zeros(1, 40, 56), "mask": lab}], 0, [0])
    with pytest.raises(ValueError, match="item 7 is 40 x 56, smaller than the 64 x 64 crop"):
        unet_amd.BatchCrop("64", 0, 3)([{"image": torch.zeros(1, 40, 56), "mask": lab}], 0, [7])


def test_loader_takes_the_keyword():
    import inspect
    from unet_amd.utils.data_loading import DeviceBatchLoader
    assert inspect.signature(DeviceBatchLoader.__init__).parameters["crop"].default is None
    assert DeviceBatchLoader([0] * 4, 2).crop is None


# ------------------------------------------------------------------------------------------------------- command line
BASE = ["--model", "UNet_T", "-c", "3", "-b", "3"]


def test_command_line_parses_the_flags(capsys):
    from unet_amd import train_cli
    from unet_amd.utils.crop import CropConfig
    assert train_cli.get_args(BASE).crop is None and train_cli.get_args(BASE).tile is None
    assert train_cli.get_args(BASE + ["--crop"]).crop == CropConfig(256, 0.5)
    assert train_cli.get_args(["--crop"] + BASE).crop == CropConfig(256, 0.5)
    assert train_cli.get_args(BASE + ["--crop", "32,classes=2+1"]).crop == CropConfig(32, 0.5, (1, 2))
    assert train_cli.get_args(BASE + ["--tile"]).tile == "512,overlap=128"
    assert train_cli.get_args(BASE + ["--tile", "32,overlap=8"]).tile == "32,overlap=8"
    assert train_cli.get_args(BASE + ["--tile", "64"]).tile == "64,overlap=32"
    for flag, bad in (("--crop", "24"), ("--crop", "32,fg=2"), ("--crop", "32,classes=64"), ("--tile", "24"), ("--tile", "64,overlap=33")):
        with pytest.raises(SystemExit) as e:
            train_cli.get_args(BASE + [flag, bad])
        assert e.value.code == 2
    capsys.readouterr()
    with pytest.raises(SystemExit):
        train_cli.build_parser().parse_args(["--help"])
    out = capsys.readouterr().out
    assert "--crop" in out and "--tile" in out


def test_run_record_holds_the_canonical_crop_and_tile_specs():
    from unet_amd.train_cli import RECORDED, get_args, run_record
    assert ("crop", "--crop") in RECORDED and ("tile", "--tile") in RECORDED
    rec = run_record(get_args(BASE + ["--crop", " 32 , classes=2+1, fg=1", "--tile", "64"]))
    assert rec["crop"] == "32,fg=1.0,classes=1+2" and rec["tile"] == "64,overlap=32"
    assert sorted(rec) == sorted(k for k, _ in RECORDED)
    bare = run_record(get_args(BASE + ["--crop", "--tile"]))
    assert bare["crop"] == "256,fg=0.5" and bare["tile"] == "512,overlap=128"
    off = run_record(get_args(BASE))
    assert off["crop"] is None and off["tile"] is None


def _state(tmp_path, argv, drop=()):
    import torch
    from unet_amd.train_cli import get_args, run_record
    record = run_record(get_args(BASE + list(argv)))
    for k in drop:
        del record[k]
    path = str(tmp_path / "train_state.pth")
    torch.save({"format": 1, "model": {}, "optimizer": {}, "epoch": 1, "global_step": 4, "lr": 1e-5, "loader_seed": 0,
                "augment_seed": None, "args": record}, path)
    return path


def test_resume_refuses_a_differing_crop_or_tile(tmp_path):
    from unet_amd.train_cli import get_args, load_resume_state
    path = _state(tmp_path, ["--crop", "32,fg=0.5", "--tile", "32,overlap=8"])
    same = ["--crop", "32", "--tile", "32,overlap=8"]
    assert load_resume_state(get_args(BASE + ["-e", "2", "--resume", path] + same))["epoch"] == 1
    for argv, flag in ((["--crop", "32,fg=0.6", "--tile", "32,overlap=8"], "--crop"), (["--crop", "48", "--tile", "32,overlap=8"], "--crop"),
                       (["--tile", "32,overlap=8"], "--crop"), (["--crop", "32", "--tile", "32,overlap=4"], "--tile"),
                       (["--crop", "32"], "--tile")):
        with pytest.raises(ValueError) as e:
            load_resume_state(get_args(BASE + ["-e", "2", "--resume", path] + argv))
        assert flag in str(e.value), str(e.value)


def test_resume_reads_a_state_without_the_keys_as_off(tmp_path):
    from unet_amd.train_cli import get_args, load_resume_state
    path = _state(tmp_path, [], drop=("crop", "tile"))                     # a state file written before the options existed
    assert load_resume_state(get_args(BASE + ["-e", "2", "--resume", path]))["epoch"] == 1
    with pytest.raises(ValueError, match="--crop"):
        load_resume_state(get_args(BASE + ["-e", "2", "--resume", path, "--crop", "32"]))
    with pytest.raises(ValueError, match="--tile"):
        load_resume_state(get_args(BASE + ["-e", "2", "--resume", path, "--tile"]))


def test_a_crop_that_does_not_fit_the_head_ends_with_status_2(caplog):
    from unet_amd import train_cli
    assert train_cli.main(["--model", "UNet_T", "-c", "3", "--crop", "32,classes=3"]) == 2
    assert "--crop" in caplog.text and "do not fit" in caplog.text
    caplog.clear()
    assert train_cli.main(["--model", "UNet_T", "-c", "2", "--crop", "32"]) == 2
    assert "--crop" in caplog.text and "2-class head" in caplog.text
