"""CPU checks of test-time augmentation (DESIGN.md section 3 "Test-time augmentation"): the view algebra of utils/tta.py against
the numpy restatement tests/tta_ref.py, the closure of every mode, BatchPredictor's grouping arithmetic, the command lines and
the argument checks of the two C entry points (host-only: they return before any launch)."""
import ctypes
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tta_ref as R  # noqa: E402

MODES = ("hflip", "flips", "rot4", "d4")
GRIDS = ((1, 1), (1, 4), (3, 5))


def _labels(H, W):
    return np.arange(H * W, dtype=np.int64).reshape(H, W)


def _key(a):
    return (a.shape, a.tobytes())


def test_the_four_masks():
    import unet_amd
    want = {"hflip": {0, 1}, "flips": {0, 1, 2, 3}, "rot4": {0, 3, 5, 6}, "d4": set(range(8))}
    for mode, views in want.items():
        mask = unet_amd.tta_mask(mode)
        assert {v for v in range(8) if mask >> v & 1} == views == set(R.mode_views(mode))
        assert unet_amd.tta_mask(mask) == mask                          # a mask that is one of the four is taken too
    from unet_amd.utils import tta
    assert tta.DEFAULT_MODE == "d4"
    assert [tta.tta_counts(m) for m in MODES] == [(2, 0), (4, 0), (2, 2), (4, 4)]
    for bad in ("rot", "", None, "D4", 0, (1 << 0) | (1 << 5), 0x1FF, True, 1.0):
        with pytest.raises(ValueError):
            unet_amd.tta_mask(bad)


def _closed(views, H=3, W=5):
    """Closed under composition and inverse, by brute force over what the views do to an H x W grid of distinct labels."""
    L = _labels(H, W)
    images = {_key(R.view_ref(L, v)) for v in views}
    for g, h in itertools.product(views, views):
        if _key(R.view_ref(R.view_ref(L, h), g)) not in images:
            return False
    return all(any(_key(R.view_ref(R.view_ref(L, h), k)) == _key(L) for k in views) for h in views)


def test_every_mode_is_a_subgroup_and_other_sets_are_refused():
    import unet_amd
    for mode in MODES:
        assert _closed(R.mode_views(mode)), mode
    assert not _closed((0, 5)) and not _closed((0, 4, 5)) and not _closed((1, 2))
    closed = [s for n in range(1, 9) for s in itertools.combinations(range(8), n) if _closed(s)]
    assert len(closed) == 10                                            # D4 has ten subgroups; the modes are four of them
    for s in closed + [(0, 5)]:
        mask = sum(1 << v for v in s)
        if mask in (0x03, 0x0F, 0x69, 0xFF):
            assert unet_amd.tta_mask(mask) == mask
        else:
            with pytest.raises(ValueError):
                unet_amd.tta_mask(mask)


@pytest.mark.parametrize("H,W", GRIDS)
def test_source_position_inverts_the_views(H, W):
    import unet_amd
    L = _labels(H, W)
    for v in range(8):
        view = R.view_ref(L, v)
        assert unet_amd.tta_view_shape(v, H, W) == view.shape
        for y in range(H):
            for x in range(W):
                pos = unet_amd.tta_source_position(v, H, W, y, x)
                assert pos == R.position_ref(v, H, W, y, x)
                assert view[pos] == L[y, x], (v, y, x)
    with pytest.raises(ValueError):
        unet_amd.tta_source_position(8, H, W, 0, 0)
    with pytest.raises(ValueError):
        unet_amd.tta_source_position(0, H, W, H, 0)
    with pytest.raises(ValueError):
        unet_amd.tta_view_shape(-1, H, W)


@pytest.mark.parametrize("H,W", GRIDS)
@pytest.mark.parametrize("mode", MODES)
def test_views_of_a_posed_image_are_the_views_of_the_image(mode, H, W):
    """The premise of the equivariance claim: for h in the mode, {g (h x)} = {g x} as multisets."""
    x = np.random.default_rng(H * 10 + W).integers(0, 256, (1, H, W, 2)).astype(np.float32)
    want = sorted(_key(a) for part in R.views_ref(x, mode) for a in part)
    for h in R.mode_views(mode):
        hx = R.view_ref(x[0], h)[None]
        got = sorted(_key(a) for part in R.views_ref(hx, mode) for a in part)
        assert got == want, (mode, h)


def test_merge_ref_is_equivariant_and_normalised():
    """The restatement itself: S64 of a posed image is the posed S64, and the sums of a pixel add up to V * 2^24."""
    rng = np.random.default_rng(3)
    H, W, NC = 3, 5, 3

    def net(views):                                                     # any per-pixel map commutes with the poses
        return np.concatenate([views * 1.5, views[..., ::-1] - 0.5, np.abs(views)], axis=-1)[..., :NC]

    x = rng.normal(0, 2, (2, H, W, 1))
    for mode in MODES:
        v0, v1 = R.views_ref(x, mode)
        S = R.merge_ref(net(v0), net(v1), mode, (H, W))
        assert np.allclose(S.sum(-1), len(R.mode_views(mode)) * R.Q, rtol=1e-12)
        for h in R.mode_views(mode):
            hx = np.stack([R.view_ref(x[b], h) for b in range(2)])
            w0, w1 = R.views_ref(hx, mode)
            Sh = R.merge_ref(net(w0), net(w1), mode, hx.shape[1:3])
            for b in range(2):
                np.testing.assert_allclose(Sh[b], R.view_ref(S[b], h), rtol=1e-13)


def _predictor(batch, tta):
    import unet_amd
    from unet_amd.predict import LaunchPlanner
    return LaunchPlanner(None, batch, True, tta=unet_amd.tta_mask(tta))          # no device, no model: the grouping is arithmetic


def test_grouping_arithmetic_under_tta():
    """-b stays the number of images per forward launch: a launch carries every view of a square image."""
    assert _predictor(8, "d4").tta_group(64, 64) == 1
    assert _predictor(8, "flips").tta_group(64, 64) == 2
    assert _predictor(3, "d4").tta_group(64, 64) == 1
    assert _predictor(8, "hflip").tta_group(64, 64) == 4
    assert _predictor(8, "rot4").tta_group(64, 64) == 2
    assert _predictor(16, "d4").tta_group(64, 64) == 2
    # H != W: the H x W views and the W x H views are two launches, of the larger count
    assert _predictor(8, "d4").tta_group(40, 48) == 2
    assert _predictor(8, "rot4").tta_group(40, 48) == 4
    assert _predictor(8, "flips").tta_group(40, 48) == 2
    assert _predictor(3, "d4").tta_group(40, 48) == 1


def test_constructors_take_the_keyword():
    import inspect
    import unet_amd
    from unet_amd.predict import BatchPredictor
    assert inspect.signature(BatchPredictor.__init__).parameters["tta"].default is None
    assert inspect.signature(unet_amd.evaluate).parameters["tta"].default is None
    p = object.__new__(BatchPredictor)
    p.tta = p.tile = None
    with pytest.raises(RuntimeError, match="tta"):
        p.probabilities([])


def test_command_lines_parse_the_flag(capsys):
    from unet_amd import evaluate_cli, predict_cli
    pred = ["-m", "m.pth", "-i", "x.png"]
    ev = ["-m", "m.pth", "--data-root", "d"]
    for cli, base in ((predict_cli, pred), (evaluate_cli, ev)):
        assert cli.get_args(base).tta is None
        assert cli.get_args(base + ["--tta"]).tta == "d4"
        assert cli.get_args(["--tta"] + base).tta == "d4"
        for mode in MODES:
            assert cli.get_args(base + ["--tta", mode]).tta == mode
        with pytest.raises(SystemExit) as e:
            cli.get_args(base + ["--tta", "rot8"])
        assert e.value.code == 2
        capsys.readouterr()
        with pytest.raises(SystemExit):
            cli.build_parser().parse_args(["--help"])
        assert "--tta" in capsys.readouterr().out
    rep = evaluate_cli.report((0.5, 0.25, 0.125), None, "rot4")
    assert rep["tta"] == "rot4" and "tta" not in evaluate_cli.report((0.5, 0.25, 0.125), None)


def test_no_cpu_fallback():
    import torch
    import unet_amd  # noqa: F401
    from unet_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.tta_views(torch.zeros(1, 1, 4, 4), "d4")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.tta_merge(torch.zeros(8, 3, 4, 4), None, "d4", (4, 4))
    with pytest.raises(ValueError):
        ops.tta_views(torch.zeros(1, 1, 4, 4), "rot8")


def test_symbols_declared_exported_and_arguments_checked():
    import unet_amd  # noqa: F401
    from unet_amd._lib import LIB, LIB_PATH
    dll = ctypes.CDLL(LIB_PATH)
    for name in ("uh_tta_views", "uh_tta_merge"):
        assert name in LIB.protos, f"{name} is not declared in include/unet_hip.h"
        assert hasattr(dll, name), f"{name} is not exported"
    assert LIB.protos["uh_tta_views"][1] == ["ptr"] * 3 + ["int"] * 5 + ["uh_stream"]
    assert LIB.protos["uh_tta_merge"][1] == ["ptr"] * 2 + ["int"] * 6 + ["ptr"] * 3 + ["uh_stream"]
    LIB.load()
    p = 4096                                                            # a non-null pointer that is never dereferenced
    with pytest.raises(RuntimeError, match="uh_tta_views.*null pointer"):
        LIB.call("uh_tta_views", None, p, p, 1, 8, 8, 1, 0xFF, None)
    with pytest.raises(RuntimeError, match="uh_tta_views.*null pointer"):
        LIB.call("uh_tta_views", p, None, p, 1, 8, 8, 1, 0xFF, None)
    with pytest.raises(RuntimeError, match="uh_tta_views.*null pointer"):
        LIB.call("uh_tta_views", p, p, None, 1, 8, 8, 1, 0x69, None)    # rot4 has transposed views
    for mask in (0, 0x21, 0x100, 0x0E, -1):
        with pytest.raises(RuntimeError, match="uh_tta_views.*bad mask"):
            LIB.call("uh_tta_views", p, p, p, 1, 8, 8, 1, mask, None)
        with pytest.raises(RuntimeError, match="uh_tta_merge.*bad mask"):
            LIB.call("uh_tta_merge", p, p, 0, 1, 8, 8, 3, mask, None, p, None, None)
    for B, H, W, C in ((0, 8, 8, 1), (1, 0, 8, 1), (1, 8, -1, 1), (1, 8, 8, 0), (1, 8, 8, 9), (65536, 8, 8, 1)):
        with pytest.raises(RuntimeError, match="uh_tta_views.*bad sizes"):
            LIB.call("uh_tta_views", p, p, p, B, H, W, C, 0xFF, None)
    with pytest.raises(RuntimeError, match="uh_tta_views.*misaligned"):
        LIB.call("uh_tta_views", p + 2, p, p, 1, 8, 8, 1, 0xFF, None)
    with pytest.raises(RuntimeError, match="uh_tta_merge.*null pointer"):
        LIB.call("uh_tta_merge", None, p, 0, 1, 8, 8, 3, 0xFF, None, p, None, None)
    with pytest.raises(RuntimeError, match="uh_tta_merge.*null pointer"):
        LIB.call("uh_tta_merge", p, None, 0, 1, 8, 8, 3, 0xFF, None, p, None, None)
    with pytest.raises(RuntimeError, match="uh_tta_merge.*null pointer"):
        LIB.call("uh_tta_merge", p, p, 0, 1, 8, 8, 3, 0xFF, None, None, None, None)      # no output at all
    with pytest.raises(RuntimeError, match="uh_tta_merge.*dtype"):
        LIB.call("uh_tta_merge", p, p, 7, 1, 8, 8, 3, 0xFF, None, p, None, None)
    for NC in (0, -1, 257):
        with pytest.raises(RuntimeError, match="uh_tta_merge.*bad sizes"):
            LIB.call("uh_tta_merge", p, p, 0, 1, 8, 8, NC, 0xFF, None, p, None, None)
    with pytest.raises(RuntimeError, match="uh_tta_merge.*misaligned"):
        LIB.call("uh_tta_merge", p + 2, p, 0, 1, 8, 8, 3, 0xFF, None, p, None, None)     # fp32 logits at an odd half-word
    with pytest.raises(RuntimeError, match="uh_tta_merge.*misaligned"):
        LIB.call("uh_tta_merge", p + 1, p, 1, 1, 8, 8, 3, 0xFF, None, p, None, None)
    with pytest.raises(RuntimeError, match="uh_tta_merge.*misaligned"):
        LIB.call("uh_tta_merge", p, p, 1, 1, 8, 8, 3, 0xFF, p + 2, p, None, None)
