"""Elastic deformation, host side (utils/augment.py: ElasticConfig, elastic_table, elastic_weights) and its numpy
restatement (tests/elastic_ref.py): the tables against the restatement, the table as a pure function of (seed, epoch,
index), exact reproduction of constants, the integer field against a float64 evaluation of the same spline within the
bound DESIGN.md derives, the no-fold condition, the restated sampler's address guard, spec parsing and the command line."""
import dataclasses

import numpy as np
import pytest
import torch

import augment_ref as AR
import elastic_ref as ER

INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1


def _aug(spec="grid=32,sigma=3", seed=1234567890123, base="flip,rotate=15,noise=0.01"):
    from unet_amd import AugmentConfig, BatchAugment, ElasticConfig
    return BatchAugment(AugmentConfig.parse(base), seed, elastic=ElasticConfig.parse(spec))


@pytest.mark.parametrize("grid", [16, 32, 64, 256])
def test_weights_equal_the_restatement_and_rows_sum_to_one(grid):
    from unet_amd.utils.augment import elastic_weights
    w = elastic_weights(grid)
    assert w.dtype == np.int32 and w.shape == (grid, 4)
    assert w.tolist() == ER.weights(grid)
    assert (w.astype(np.int64).sum(axis=1) == 1 << 20).all() and (w >= 0).all()
    assert np.abs(w - w[::-1, ::-1]).max() <= 2       # B_j(t) = B_{3-j}(1 - t), up to the adjustment
    for bad in (0, 8, 24, 272):
        with pytest.raises(ValueError):
            elastic_weights(bad)


def test_table_equals_the_restatement():
    seed = (77 << 32) + 5
    for spec, epoch, H, W in (("grid=16,sigma=1.5", 0, 100, 37), ("grid=64,sigma=4", 3, 96, 130), ("grid=32,sigma=3,p=0.5", 2, 64, 64)):
        aug = _aug(spec, seed)
        el = aug.elastic
        idx = list(range(0, 60, 7))
        table = aug.elastic_table(epoch, idx, (H, W))
        assert table.dtype == np.int32 and table.shape == (len(idx),) + ER.grid_shape(H, W, el.grid) + (2,)
        keys = aug.draws(epoch, idx, (H, W))["key"]
        for row, i, key in zip(table, idx, keys):
            want = ER.control_item(el.grid, el.sigma, el.p, seed, epoch, i, tuple(int(k) for k in key), H, W)
            assert np.array_equal(row, want), (spec, i)
            assert tuple(int(k) for k in key) == AR.draw_item(aug.config, seed, epoch, i, H, W)["key"]
        assert np.abs(table).max() <= round(2 * el.sigma * 65536) and np.abs(table).max() > 1.5 * el.sigma * 65536
        if el.p < 1:
            zero = [not row.any() for row in table]
            assert any(zero) and not all(zero)


def test_table_is_a_pure_function_of_seed_epoch_index():
    from unet_amd import BatchAugment
    aug = _aug()
    idx = [7, 0, 3, 11, 4, 9, 2, 40]
    size = (96, 128)
    full = aug.elastic_table(2, idx, size)
    assert np.array_equal(full, _aug().elastic_table(2, idx, size))                            # no hidden state
    perm = [5, 2, 7, 0, 1, 6, 3, 4]
    assert np.array_equal(aug.elastic_table(2, [idx[p] for p in perm], size), full[perm])      # permuting permutes the rows
    for k, i in enumerate(idx):                                                                # alone = inside a batch
        assert np.array_equal(aug.elastic_table(2, [i], size), full[k:k + 1])
    assert not np.array_equal(aug.elastic_table(3, idx, size), full)                           # another epoch
    assert not np.array_equal(_aug(seed=5).elastic_table(2, idx, size), full)                  # another seed
    assert len({aug.elastic_table(2, [i], size).tobytes() for i in range(50)}) == 50           # another item
    assert not _aug("grid=32,sigma=3,p=0").elastic_table(2, idx, size).any()                   # p = 0: zeros
    assert not BatchAugment(aug.config, aug.seed).elastic_table(2, idx, size).any()            # no elastic record: zeros
    # the affine and photometric draws do not move when the elastic record is added
    assert aug.params(2, idx, size).tobytes() == BatchAugment(aug.config, aug.seed).params(2, idx, size).tobytes()
    assert aug.params(2, idx, size).tobytes() == BatchAugment(aug.config, aug.seed, elastic=None).params(2, idx, size).tobytes()


@pytest.mark.parametrize("grid", [16, 64])
def test_constant_field_is_reproduced_exactly(grid):
    H, W = 100, 37
    GH, GW = ER.grid_shape(H, W, grid)
    for c in ((3 << 16, -2 << 16), (12345, -1), (ER.D_MAX, -ER.D_MAX)):
        dx, dy = ER.field_q16(np.broadcast_to(np.array(c, np.int64), (GH, GW, 2)), grid, H, W)
        assert (dx == c[0]).all() and (dy == c[1]).all()


@pytest.mark.parametrize("spec,H,W", [("grid=16,sigma=1.9", 100, 37), ("grid=64,sigma=7.9", 96, 130), ("grid=256,sigma=31", 300, 520)])
def test_integer_field_against_float64(spec, H, W):
    aug = _aug(spec, 11)
    worst = 0.0
    for control in aug.elastic_table(1, range(6), (H, W)):
        bound = ER.field_error_bound(np.abs(control).max()) + 1e-6               # + float64's own rounding, far below
        for got, want in zip(ER.field_q16(control, aug.elastic.grid, H, W), ER.field_f64(control, aug.elastic.grid, H, W)):
            err = float(np.abs(got - want).max())
            worst = max(worst, err)
            assert err <= bound, (spec, err, bound)
    print(f"integer field vs float64 spline, {spec} {H}x{W}: max |diff| {worst:.3f} Q16 units (bound {bound:.3f})")


def test_no_fold():
    from unet_amd import AugmentConfig, BatchAugment, ElasticConfig
    el = ElasticConfig(grid=32, sigma=3.9)
    H, W = 96, 128
    floor = 1.0 - 8.0 * el.sigma / el.grid - ER.no_fold_slack(el.sigma, el.grid)
    assert floor > 0
    worst = 1.0
    for seed in range(200):
        control = BatchAugment(AugmentConfig(), seed, elastic=el).elastic_table(0, [seed % 7], (H, W))[0]
        dx, dy = ER.field_q16(control, el.grid, H, W)
        det = ER.jacobian_det(dx / 65536.0, dy / 65536.0)
        worst = min(worst, float(det.min()))
        assert det.min() >= floor and det.min() > 0, (seed, det.min(), floor)
    print(f"no-fold, grid=32 sigma=3.9, 200 seeds: min det {worst:.4f} (floor {floor:.4f})")
    for bad in (dict(grid=32, sigma=4), dict(grid=16, sigma=2.0), dict(grid=24, sigma=1), dict(grid=272, sigma=1),
                dict(grid=32, sigma=-1), dict(grid=32, sigma=1, p=1.5)):
        with pytest.raises(ValueError):
            ElasticConfig(**bad)
    with pytest.raises(ValueError):
        ElasticConfig.parse("grid=32,sigma=4")


@pytest.mark.parametrize("border", ["clamp", "fill"])
def test_restated_sampler_guards_its_addresses_and_zero_field_is_the_affine_stage(border):
    from unet_amd import AugmentConfig, BatchAugment
    H, W, grid = 100, 37, 16
    rng = np.random.default_rng(4)
    img = rng.random((H, W, 3), dtype=np.float32)
    lab = rng.integers(0, 3, (H, W))
    cfg = AugmentConfig.parse(f"flip,rotate=25,scale=0.2,translate=0.1,contrast=0.3,border={border},fill_image=0.25")
    t = BatchAugment(cfg, 3).params(1, [5], (H, W))[0]
    row = {k: t[k] for k in ("gamma", "contrast", "brightness", "noise_std")}
    row["m"], row["key"] = t["m"].tolist(), tuple(int(k) for k in t["key"])
    shape = ER.grid_shape(H, W, grid) + (2,)
    zero_i, zero_l = ER.augment_item(img, lab, row, np.zeros(shape, np.int64), grid, border, 0.25, 1)
    want_i, want_l = AR.augment_item(img, lab, row, border, 0.25, 1)
    assert zero_i.tobytes() == want_i.tobytes() and np.array_equal(zero_l, want_l)
    # the extremes of int32 in every pattern: the index asserts of the restated walk hold, the output is finite
    extremes = rng.choice(np.array([INT32_MIN, INT32_MAX, 0], np.int64), shape)
    for control in (np.full(shape, INT32_MIN, np.int64), np.full(shape, INT32_MAX, np.int64), extremes):
        oi, ol = ER.augment_item(img, lab, row, control, grid, border, 0.25, 1)
        assert np.isfinite(oi).all() and ol.min() >= 0 and ol.max() <= 2
        dx, dy = ER.field_q16(control, grid, H, W)
        assert max(np.abs(dx).max(), np.abs(dy).max()) <= ER.D_MAX


def test_parse_round_trips_and_rejects_unknown_keys():
    from unet_amd import ElasticConfig
    from unet_amd.utils.augment import ELASTIC_PRESETS
    assert ELASTIC_PRESETS["default"] == "grid=64,sigma=4"
    d = ElasticConfig.parse("default")
    assert dataclasses.asdict(d) == dict(grid=64, sigma=4.0, p=1.0) and not d.is_identity
    assert dataclasses.is_dataclass(d) and d == ElasticConfig.parse(" default ")
    with pytest.raises(dataclasses.FrozenInstanceError):
        d.sigma = 1.0
    for cfg in (d, ElasticConfig(), ElasticConfig.parse("grid=16,sigma=1.25,p=0.5"), ElasticConfig.parse("default,sigma=2")):
        assert ElasticConfig.parse(cfg.spec()) == cfg
    assert ElasticConfig().is_identity and ElasticConfig.parse("") == ElasticConfig() and ElasticConfig.parse("none") == ElasticConfig()
    assert ElasticConfig(sigma=0).is_identity and ElasticConfig(sigma=3, p=0).is_identity and ElasticConfig().p == 1
    assert ElasticConfig.parse("default,sigma=2").grid == 64
    for bad in ("shear=3", "sigma", "grid=64,blur=1", "grid=abc", "grid=20,sigma=1", "grid=64,sigma=8", "p=2", "grid=64.5"):
        with pytest.raises(ValueError):
            ElasticConfig.parse(bad)


def test_command_line_flag():
    from unet_amd.train_cli import build_parser
    p = build_parser()
    assert p.parse_args([]).elastic is None                                           # off by default
    assert p.parse_args(["--elastic"]).elastic == "default"
    assert p.parse_args(["--elastic", "grid=32,sigma=2"]).elastic == "grid=32,sigma=2"
    a = p.parse_args(["--elastic", "--augment", "-e", "1"])
    assert a.elastic == "default" and a.augment == "default" and a.epochs == 1
    assert p.parse_args(["--augment"]).elastic is None


def test_bad_spec_fails_before_anything_is_loaded(tmp_path, monkeypatch):
    from unet_amd import train_cli
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    with pytest.raises(ValueError, match="8 sigma < grid"):
        train_cli.main(["--elastic", "grid=32,sigma=4", "--data-root", str(tmp_path / "missing")])


def test_batch_augment_takes_the_record_or_its_spec():
    from unet_amd import AugmentConfig, BatchAugment, ElasticConfig
    cfg = AugmentConfig.parse("default")
    assert BatchAugment(cfg, 1).elastic is None
    assert BatchAugment(cfg, 1, elastic="default").elastic == ElasticConfig(grid=64, sigma=4.0)
    assert BatchAugment(cfg, 1, "grid=16,sigma=1").elastic == ElasticConfig(grid=16, sigma=1.0)


def test_no_cpu_fallback():
    from unet_amd.utils.augment import augment_with_control
    batch = {"image": torch.rand(2, 1, 8, 8), "mask": torch.zeros(2, 8, 8, dtype=torch.int64)}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _aug("grid=16,sigma=1")(batch, 0, [0, 1])
    table = _aug().params(0, [0, 1], (8, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        augment_with_control(batch, table, np.zeros((2, 4, 4, 2), np.int32), 16, "clamp", 0.0, 1)
