"""Training augmentation, host side (utils/augment.py) and its numpy restatement (tests/augment_ref.py): Philox known
answers, the parameter draws as a pure function of (seed, epoch, index), the exact identity and flip tables, the restated
geometry against torch's float64 grid_sample within a bound derived from the fixed-point formats, and spec parsing."""
import dataclasses

import numpy as np
import pytest
import torch

import augment_ref as AR

# Philox4x32-10 known answers (counter, key, output)
KAT = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
       ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
       ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
SPEC = "flip,rotate=15,scale=0.1,translate=0.05,brightness=0.1,contrast=0.1,gamma=0.2,noise=0.01"


def _hex(words):
    return " ".join(f"{int(w):08x}" for w in words)


@pytest.mark.parametrize("counter,key,want", KAT)
def test_philox_known_answers(counter, key, want):
    from unet_amd.utils.augment import philox4x32_10
    assert _hex(AR.philox(counter, key)) == want
    assert _hex(philox4x32_10(np.array(counter, np.uint32), np.array(key, np.uint32))) == want
    # the vectorised form, a batch of counters against one key
    many = philox4x32_10(np.array([counter, (1, 2, 3, 4)], np.uint32), np.array(key, np.uint32))
    assert _hex(many[0]) == want and _hex(many[1]) == _hex(AR.philox((1, 2, 3, 4), key))


def _rows_equal(a, b):
    return a.tobytes() == b.tobytes()


def test_params_are_a_pure_function_of_seed_epoch_index():
    from unet_amd import AugmentConfig, BatchAugment
    cfg = AugmentConfig.parse(SPEC)
    aug = BatchAugment(cfg, seed=1234567890123)
    idx = [7, 0, 3, 11, 4, 9, 2, 40]
    full = aug.params(2, idx, (96, 128))
    assert full.dtype.itemsize == 72 and full.shape == (8,)
    assert _rows_equal(full, BatchAugment(cfg, 1234567890123).params(2, idx, (96, 128)))      # no hidden state
    perm = [5, 2, 7, 0, 1, 6, 3, 4]
    assert _rows_equal(aug.params(2, [idx[p] for p in perm], (96, 128)), full[perm])          # permuting permutes the rows
    assert _rows_equal(np.concatenate([aug.params(2, idx[:3], (96, 128)), aug.params(2, idx[3:], (96, 128))]), full)
    for k, i in enumerate(idx):                                                                # alone = inside a batch
        assert _rows_equal(aug.params(2, [i], (96, 128)), full[k:k + 1])
    assert not _rows_equal(aug.params(3, idx, (96, 128)), full)                                # another epoch
    assert not _rows_equal(BatchAugment(cfg, 5).params(2, idx, (96, 128)), full)               # another seed
    assert len({aug.params(2, [i], (96, 128)).tobytes() for i in range(50)}) == 50             # another item


def test_package_draws_equal_the_restatement():
    from unet_amd import AugmentConfig, BatchAugment
    cfg = AugmentConfig.parse(SPEC + ",border=fill")
    seed = (77 << 32) + 5
    aug = BatchAugment(cfg, seed)
    for epoch, H, W in ((0, 100, 37), (3, 512, 512)):
        idx = list(range(0, 60, 7))
        table = aug.params(epoch, idx, (H, W))
        for row, i in zip(table, idx):
            d = AR.draw_item(cfg, seed, epoch, i, H, W)
            assert row["m"].tolist() == AR.q32(AR.matrix(d, H, W))
            assert (row["gamma"], row["contrast"], row["brightness"], row["noise_std"]) == \
                tuple(np.float32(d[k]) for k in ("gamma", "contrast", "brightness", "noise_std"))
            assert tuple(int(k) for k in row["key"]) == d["key"]


def test_draws_stay_inside_their_ranges():
    from unet_amd import AugmentConfig, BatchAugment
    cfg = AugmentConfig.parse(SPEC)
    H, W = 200, 300
    d = BatchAugment(cfg, 9).draws(1, range(4000), (H, W))
    assert np.abs(d["theta_deg"]).max() <= 15 and np.abs(d["theta_deg"]).max() > 14
    assert d["scale"].min() >= 0.9 and d["scale"].max() <= 1.1 and d["scale"].max() - d["scale"].min() > 0.19
    assert np.abs(d["tx"]).max() <= 0.05 * W and np.abs(d["ty"]).max() <= 0.05 * H and np.abs(d["tx"]).max() > 0.045 * W
    assert np.abs(d["brightness"]).max() <= 0.1 and np.abs(d["contrast"] - 1).max() <= 0.1
    assert d["gamma"].min() >= 1 / 1.2 and d["gamma"].max() <= 1.2 and d["gamma"].min() < 0.85 and d["gamma"].max() > 1.18
    for flips in (d["hflip"], d["vflip"]):
        assert 0.45 < flips.mean() < 0.55                         # p = 0.5 over 4000 draws: 6 sigma is 0.047
    assert abs(np.log(d["gamma"]).mean()) < 0.02                  # log-uniform: symmetric in the exponent
    table = BatchAugment(cfg, 9).params(1, range(64), (H, W))
    assert (table["noise_std"] == np.float32(0.01)).all() and np.abs(table["m"]).max() < 1 << 48


def test_neutral_config_is_the_exact_identity():
    from unet_amd import AugmentConfig, BatchAugment
    cfg = AugmentConfig()
    assert cfg.is_identity and AugmentConfig.parse("") == cfg and AugmentConfig.parse("none") == cfg
    t = BatchAugment(cfg, 3).params(5, range(16), (37, 100))
    one = 1 << 32
    assert (t["m"] == np.array([one, 0, 0, 0, one, 0])).all()
    assert (t["gamma"] == 1).all() and (t["contrast"] == 1).all() and (t["brightness"] == 0).all() and (t["noise_std"] == 0).all()
    assert not np.signbit(t["brightness"]).any()
    # and the restated walk with that table is the identity gather
    img = np.random.default_rng(0).random((37, 100, 3), dtype=np.float32)
    lab = np.random.default_rng(1).integers(0, 3, (37, 100))
    row = {k: t[0][k] for k in ("gamma", "contrast", "brightness", "noise_std", "key")}
    row["m"] = t["m"][0].tolist()
    oi, ol = AR.augment_item(img, lab, row)
    assert oi.tobytes() == img.tobytes() and np.array_equal(ol, lab)


def test_flip_only_configs_give_unit_entries_and_integer_offsets():
    from unet_amd import AugmentConfig, BatchAugment
    H, W = 37, 100
    one = 1 << 32
    both = BatchAugment(AugmentConfig(p_hflip=1.0, p_vflip=1.0), 0).params(0, range(4), (H, W))
    assert (both["m"] == np.array([-one, 0, W * one, 0, -one, H * one])).all()
    h = BatchAugment(AugmentConfig(p_hflip=1.0), 0).params(0, range(4), (H, W))
    assert (h["m"] == np.array([-one, 0, W * one, 0, one, 0])).all()
    mixed = BatchAugment(AugmentConfig.parse("flip"), 0).params(0, range(64), (H, W))["m"]
    assert set(np.unique(np.abs(mixed[:, [0, 4]]))) == {one} and (mixed[:, [1, 3]] == 0).all()
    assert (mixed[:, [2, 5]] % one == 0).all()
    assert {(int(r[0] < 0), int(r[4] < 0)) for r in mixed} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    # the restated walk is torch.flip, bit for bit
    img = np.random.default_rng(2).random((H, W, 2), dtype=np.float32)
    lab = np.random.default_rng(3).integers(0, 3, (H, W))
    assert AR.bilinear_f32(img, both["m"][0].tolist()).tobytes() == img[::-1, ::-1].tobytes()
    assert np.array_equal(AR.labels_nearest(lab, h["m"][0].tolist()), lab[:, ::-1])


# ------------------------------------------------------------------------------ the restatement against grid_sample
# The allowed difference, from the formats (not tuned).  Coordinates: a Q32 matrix entry is off by at most 2^-33, it
# multiplies a centre coordinate of at most 2048, two entries and the offset per axis: 2 * 2048 * 2^-33 + 2^-33 < 2^-21;
# the rounding to Q16 adds 2^-17: below 2^-16 px per axis for sizes up to 2048.  Values: the bilinear surface changes by
# at most (largest neighbour difference <= 1) per pixel along each axis, so 2 axes * 2^-16 = 2^-15; the fp32 evaluation
# adds 3 roundings per interpolation of at most 2^-25 each (values in [0, 1]), two levels deep: 6 * 2^-25 = 3 * 2^-24.
COORD_BOUND = 2.0 ** -16
VALUE_BOUND = 2.0 ** -15 * 1.0 + 3 * 2.0 ** -24


def _grid_sample64(img, m, mode, fill=0.0):
    """torch's float64 bilinear sampling of img [H, W, C] at the UNQUANTISED map m [2, 3] (pixel-centre coordinates)."""
    H, W, _ = img.shape
    xc, yc = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    sx = m[0, 0] * xc + m[0, 1] * yc + m[0, 2]
    sy = m[1, 0] * xc + m[1, 1] * yc + m[1, 2]
    grid = torch.from_numpy(np.stack([2 * sx / W - 1, 2 * sy / H - 1], -1))[None]       # align_corners=False
    t = torch.from_numpy(img.astype(np.float64) - fill).permute(2, 0, 1)[None]
    out = torch.nn.functional.grid_sample(t, grid, mode="bilinear", padding_mode=mode, align_corners=False)
    return out[0].permute(1, 2, 0).numpy() + fill, sx, sy


@pytest.mark.parametrize("H,W,C", [(100, 37, 1), (64, 64, 3), (301, 517, 2), (2048, 96, 1)])
@pytest.mark.parametrize("border", ["clamp", "fill"])
def test_restatement_against_float64_grid_sample(H, W, C, border):
    from unet_amd import AugmentConfig
    cfg = AugmentConfig.parse("flip,rotate=30,scale=0.25,translate=0.1")
    rng = np.random.default_rng(H * 31 + W)
    img = rng.random((H, W, C), dtype=np.float32)
    lab = rng.integers(0, 3, (H, W))
    fill = 0.25 if border == "fill" else 0.0
    worst, outside = 0.0, 0
    for index in range(4):
        d = AR.draw_item(cfg, 42, 1, index, H, W)
        m = AR.matrix(d, H, W)
        mq = AR.q32(m)
        want, sx, sy = _grid_sample64(img, m, "border" if border == "clamp" else "zeros", fill)
        got = AR.bilinear_f32(img, mq, border == "fill", fill)
        qx, qy = AR.coords_q16(mq, H, W)
        assert np.abs(qx / 65536.0 - sx).max() < COORD_BOUND and np.abs(qy / 65536.0 - sy).max() < COORD_BOUND
        err = float(np.abs(got.astype(np.float64) - want).max())
        worst = max(worst, err)
        assert err <= VALUE_BOUND, (index, err, VALUE_BOUND)
        # labels: the nearest-pixel gather of the restated integer coordinates (ties at half pixels are this design's rule)
        lx, ly = qx >> 16, qy >> 16
        inside = (lx >= 0) & (lx < W) & (ly >= 0) & (ly < H)
        gathered = lab[np.clip(ly, 0, H - 1), np.clip(lx, 0, W - 1)]
        if border == "fill":
            gathered = np.where(inside, gathered, 1)
        assert np.array_equal(AR.labels_nearest(lab, mq, border == "fill", 1), gathered)
        outside += int((~inside).sum())
    assert outside > 0                                               # the case does reach past the border
    print(f"restatement vs float64 grid_sample {H}x{W}x{C} {border}: max |diff| {worst:.3e} (bound {VALUE_BOUND:.3e})")


def test_restated_noise_and_photometry_order():
    """Box-Muller from the documented words, and the stage order gamma -> contrast -> brightness -> noise -> clamp."""
    key = (123, 456)
    w = AR.noise_words(key, 10)
    assert w.shape == (3, 4) and tuple(int(x) for x in w[1]) == AR.philox((1, 0, 0, 1), key)
    z = AR.normals(w, 10)
    u, v = (float(w[1, 2]) + 0.5) / 2 ** 32, float(w[1, 3]) / 2 ** 32
    assert z[6] == np.sqrt(-2 * np.log(u)) * np.cos(2 * np.pi * v) and z[7] == np.sqrt(-2 * np.log(u)) * np.sin(2 * np.pi * v)
    big = AR.normals(AR.noise_words(key, 1 << 14), 1 << 14)
    n = big.size
    assert abs(big.mean()) <= 5 / np.sqrt(n) and abs(big.var() - 1) <= 5 * np.sqrt(2 / n)
    x = np.array([[[0.25], [0.81]]], np.float32)
    got = AR.photometry(x, 0.5, 1.5, 0.125, 0.0, key)
    want = np.clip((np.sqrt(x.astype(np.float64)) - 0.5) * 1.5 + 0.5 + 0.125, 0, 1)
    assert np.allclose(got, want, rtol=0, atol=1e-15)
    assert AR.photometry(x, 1.0, 1.0, 0.0, 0.0, key) is x            # all neutral: untouched, not even clamped


# ----------------------------------------------------------------------------------------------------------- parsing
def test_parse_round_trips_and_rejects_unknown_keys():
    from unet_amd import AugmentConfig
    c = AugmentConfig.parse(SPEC)
    assert dataclasses.asdict(c) == dict(p_hflip=0.5, p_vflip=0.5, rotate_deg=15.0, scale=0.1, translate=0.05, brightness=0.1,
                                         contrast=0.1, gamma=0.2, noise_std=0.01, border="clamp", fill_image=0.0, fill_label=1)
    for cfg in (c, AugmentConfig(), AugmentConfig.parse("default"),
                AugmentConfig.parse("hflip=0.25,rotate=7.5,border=fill,fill_image=0.5,fill_label=0")):
        assert AugmentConfig.parse(cfg.spec()) == cfg
    d = AugmentConfig.parse("default")
    assert not d.is_identity and d == AugmentConfig.parse(" default ") and d.border == "clamp"
    assert AugmentConfig.parse("default,rotate=0").rotate_deg == 0 and AugmentConfig.parse("default,rotate=0").scale == d.scale
    assert AugmentConfig.parse("vflip").p_vflip == 0.5 and AugmentConfig.parse("vflip").p_hflip == 0
    for bad in ("shear=3", "rotate", "flip,blur=1", "border=wrap", "rotate=-1", "hflip=2", "scale=abc"):
        with pytest.raises(ValueError):
            AugmentConfig.parse(bad)


def test_command_line_flag():
    from unet_amd.train_cli import build_parser
    p = build_parser()
    assert p.parse_args([]).augment is None                                         # off by default
    assert p.parse_args(["--augment"]).augment == "default"
    assert p.parse_args(["--augment", "flip,rotate=5"]).augment == "flip,rotate=5"
    assert p.parse_args(["--augment", "-e", "1"]).augment == "default" and p.parse_args(["--augment", "-e", "1"]).epochs == 1


def test_no_cpu_fallback():
    from unet_amd import AugmentConfig, BatchAugment
    aug = BatchAugment(AugmentConfig.parse("flip"), 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        aug({"image": torch.rand(2, 1, 8, 8), "mask": torch.zeros(2, 8, 8, dtype=torch.int64)}, 0, [0, 1])


def test_loader_takes_an_augmenter_and_defaults_to_none():
    from unet_amd import AugmentConfig, BatchAugment
    from unet_amd.utils.data_loading import DeviceBatchLoader
    ds = list(range(10))
    assert DeviceBatchLoader(ds, 4).augment is None
    aug = BatchAugment(AugmentConfig.parse("default"), 1)
    assert DeviceBatchLoader(ds, 4, augment=aug).augment is aug
