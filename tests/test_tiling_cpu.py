"""CPU checks of tiled prediction (DESIGN.md section 3 "Tiled prediction"): the geometry of utils/tiling.py against its stated
properties, against the numpy restatement tests/tiling_ref.py and against the library's host query uh_tile_grid; the refusals of
TileConfig and the spec parser; the command lines; the argument checks of the launch entry points (host-only: they return
before any launch)."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tiling_ref as R  # noqa: E402

SIZES = (16, 32, 64)
LENGTHS = range(1, 201)


def _configs():
    for size in SIZES:
        for overlap in range(0, size // 2 + 1):
            yield size, overlap


def test_geometry_sweep():
    from unet_amd.utils.tiling import TileConfig, axis_origins, tile_grid, tile_shape
    for size, overlap in _configs():
        cfg = TileConfig(size, overlap)
        for L in LENGTHS:
            o = axis_origins(L, cfg)
            t = min(size, L)
            assert o == R.origins(L, size, overlap)
            assert o[0] == 0 and o[-1] + t == L                                     # the first is 0, the last ends at L
            assert all(0 <= k and k + t <= L for k in o)                            # every tile lies inside [0, L)
            assert all(a < b for a, b in zip(o, o[1:]))                             # strictly increasing
            cover = np.zeros(L, np.int64)
            for k in o:
                cover[k:k + t] += 1
            assert cover.min() >= 1 and cover.max() <= 3, (L, size, overlap)        # the union is [0, L); at most 3 deep
            if L <= size:
                assert o == [0] and t == L
            else:
                assert len(o) == math.ceil((L - size) / (size - overlap)) + 1 == R.count_formula(L, size, overlap)
    cfg = TileConfig(32, 8)
    assert tile_grid(70, 90, cfg) == (3, 4, 32, 32, [0, 24, 38], [0, 24, 48, 58])      # worked by hand: S = 24
    assert tile_shape(20, 90, cfg) == (20, 32) and tile_grid(20, 31, cfg) == (1, 1, 20, 31, [0], [0])


def test_weights_are_positive_and_symmetric():
    from unet_amd.utils.tiling import TileConfig, axis_weights
    for size, overlap in _configs():
        cfg = TileConfig(size, overlap)
        for t in (1, 2, 5, size - 1, size):
            w = axis_weights(t, cfg)
            assert len(w) == t and min(w) >= 1 and max(w) <= max(1, overlap)
            assert w == w[::-1]
            assert w == [int(v) for v in R.weights(t, overlap)]
            if overlap == 0:
                assert set(w) == {1}
    assert axis_weights(16, TileConfig(16, 4)) == [1, 2, 3, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 3, 2, 1]
    assert 512 * 512 == 1 << 18                                                     # the largest weight of a tile pixel


def _c_grid(dll, H, W, size, overlap):
    ny, nx, th, tw = (ctypes.c_int() for _ in range(4))
    rc = dll.uh_tile_grid(H, W, size, overlap, ctypes.byref(ny), ctypes.byref(nx), ctypes.byref(th), ctypes.byref(tw), None, None)
    assert rc == 0
    oy, ox = (ctypes.c_int * ny.value)(), (ctypes.c_int * nx.value)()
    assert dll.uh_tile_grid(H, W, size, overlap, None, None, None, None, oy, ox) == 0
    return ny.value, nx.value, th.value, tw.value, list(oy), list(ox)


def test_library_answers_the_same_grid():
    import unet_amd  # noqa: F401
    from unet_amd._lib import LIB
    from unet_amd.utils.tiling import TileConfig, tile_grid
    assert "uh_tile_grid" in LIB.protos, "uh_tile_grid is not declared in include/unet_hip.h"
    assert LIB.protos["uh_tile_grid"][1] == ["int"] * 4 + ["ptr"] * 6
    dll = LIB.load()
    for size, overlap in _configs():
        cfg = TileConfig(size, overlap)
        for L in LENGTHS:
            M = 200 - L + 1                                                         # the other axis sweeps the other way
            assert _c_grid(dll, L, M, size, overlap) == tile_grid(L, M, cfg), (L, M, size, overlap)
    assert _c_grid(dll, 4096, 3000, 512, 128) == tile_grid(4096, 3000, TileConfig())
    for size, overlap in ((24, 0), (2048, 0), (0, 0), (-16, 0), (64, 33), (64, -1), (1040, 8)):
        assert dll.uh_tile_grid(100, 100, size, overlap, None, None, None, None, None, None) == -1      # UH_EINVAL
    assert dll.uh_tile_grid(0, 100, 64, 16, None, None, None, None, None, None) == -1
    assert dll.uh_tile_grid(100, -1, 64, 16, None, None, None, None, None, None) == -1


def test_config_and_spec_refusals():
    import unet_amd
    from unet_amd.utils.tiling import DEFAULT_SPEC, TileConfig, parse_tile_spec, tile_config
    assert TileConfig() == TileConfig(512, 128) == parse_tile_spec("") == parse_tile_spec("512") == parse_tile_spec(DEFAULT_SPEC)
    assert parse_tile_spec("512,overlap=64") == TileConfig(512, 64) and parse_tile_spec(" 64 , overlap = 0 ") == TileConfig(64, 0)
    assert TileConfig(512, 64).spec == "512,overlap=64" and unet_amd.TileConfig is TileConfig
    assert tile_config(None) is None and tile_config("64,overlap=8") == TileConfig(64, 8) == tile_config(TileConfig(64, 8))
    for size, overlap in ((24, 0), (2048, 0), (64, 33), (64, -1), (-64, 0), (0, 0), (8, 0), (64.0, 0), (64, 1.5), ("64", 0),
                          (True, 0), (1040, 0)):
        with pytest.raises(ValueError):
            TileConfig(size, overlap)
    for size in SIZES:
        with pytest.raises(ValueError):
            TileConfig(size, size // 2 + 1)
        TileConfig(size, size // 2)
    for spec in ("24", "2048", "64,overlap=33", "-64", "64,overlap=-1", "garbage", "64,", "64,overlap", "64,overlap=",
                 "64,stride=8", "64;8", "64,overlap=8,overlap=8", "6 4", "0x40", "64.0", None, 64):
        with pytest.raises(ValueError):
            parse_tile_spec(spec)
    with pytest.raises(ValueError):
        tile_config(64)


def test_constructors_take_the_keyword():
    import inspect
    import unet_amd
    from unet_amd.predict import BatchPredictor
    assert inspect.signature(BatchPredictor.__init__).parameters["tile"].default is None
    assert inspect.signature(unet_amd.evaluate).parameters["tile"].default is None
    p = object.__new__(BatchPredictor)
    p.tta = p.tile = None
    with pytest.raises(RuntimeError, match="tile"):
        p.probabilities([])
    from unet_amd.predict import LaunchPlanner
    assert LaunchPlanner(None, 8, True, tta=unet_amd.tta_mask("flips")).tile_chunk(32, 32) == 2      # under tta the group counts tiles
    assert LaunchPlanner(None, 8, True).tile_chunk(32, 32) == 8


def test_command_lines_parse_the_flag(capsys):
    from unet_amd import evaluate_cli, predict_cli
    pred = ["-m", "m.pth", "-i", "x.png"]
    ev = ["-m", "m.pth", "--data-root", "d"]
    for cli, base in ((predict_cli, pred), (evaluate_cli, ev)):
        assert cli.get_args(base).tile is None
        assert cli.get_args(base + ["--tile"]).tile == "512,overlap=128"
        assert cli.get_args(["--tile"] + base).tile == "512,overlap=128"
        assert cli.get_args(base + ["--tile", "512"]).tile == "512,overlap=128"
        assert cli.get_args(base + ["--tile", "512,overlap=64"]).tile == "512,overlap=64"
        assert cli.get_args(base + ["--tile", "64,overlap=0", "--tta", "flips"]).tta == "flips"
        for bad in ("24", "2048", "64,overlap=33", "garbage"):
            with pytest.raises(SystemExit) as e:
                cli.get_args(base + ["--tile", bad])
            assert e.value.code == 2
        capsys.readouterr()
        with pytest.raises(SystemExit):
            cli.build_parser().parse_args(["--help"])
        assert "--tile" in capsys.readouterr().out
    rep = evaluate_cli.report((0.5, 0.25, 0.125), None, "flips", "512,overlap=64")
    assert rep["tile"] == "512,overlap=64" and rep["tta"] == "flips"
    assert "tile" not in evaluate_cli.report((0.5, 0.25, 0.125), None)


def test_no_cpu_fallback():
    import torch
    import unet_amd  # noqa: F401
    from unet_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.tile_gather(torch.zeros(1, 1, 40, 40), "16,overlap=4")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.tile_merge(torch.zeros(9, 3, 16, 16), "16,overlap=4", (40, 40))
    with pytest.raises(ValueError):
        ops.tile_gather(torch.zeros(1, 1, 40, 40), "24")
    with pytest.raises(ValueError):
        ops.tile_merge(torch.zeros(9, 3, 16, 16), "16,overlap=4", (40, 40), views=3)


def test_symbols_declared_exported_and_arguments_checked():
    import unet_amd  # noqa: F401
    from unet_amd._lib import LIB, LIB_PATH
    dll = ctypes.CDLL(LIB_PATH)
    for name in ("uh_tile_grid", "uh_tile_gather", "uh_tile_merge"):
        assert name in LIB.protos, f"{name} is not declared in include/unet_hip.h"
        assert hasattr(dll, name), f"{name} is not exported"
    assert LIB.protos["uh_tile_gather"][1] == ["ptr"] * 2 + ["int"] * 6 + ["uh_stream"]
    assert LIB.protos["uh_tile_merge"][1] == ["ptr"] + ["int"] * 8 + ["ptr"] * 4 + ["uh_stream"]
    LIB.load()
    p = 4096                                                            # a non-null pointer that is never dereferenced
    F32, BF16, SUMS = 0, 1, 3

    def gather(x=p, tiles=p, B=1, H=40, W=40, C=1, size=16, overlap=4):
        LIB.call("uh_tile_gather", x, tiles, B, H, W, C, size, overlap, None)

    def merge(src=p, kind=F32, views=1, B=1, H=40, W=40, NC=3, size=16, overlap=4, sums=None, den=None, classes=p, probs=None):
        LIB.call("uh_tile_merge", src, kind, views, B, H, W, NC, size, overlap, sums, den, classes, probs, None)

    for fn, name in ((gather, "uh_tile_gather"), (merge, "uh_tile_merge")):
        for size, overlap in ((24, 0), (2048, 0), (0, 0), (-16, 0), (64, 33), (64, -1)):
            with pytest.raises(RuntimeError, match=name + ".*bad config"):
                fn(size=size, overlap=overlap)
        for kw in (dict(B=0), dict(H=0), dict(W=-1), dict(B=65536)):
            with pytest.raises(RuntimeError, match=name + ".*bad sizes"):
                fn(**kw)
    with pytest.raises(RuntimeError, match="uh_tile_gather.*null pointer"):
        gather(x=None)
    with pytest.raises(RuntimeError, match="uh_tile_gather.*null pointer"):
        gather(tiles=None)
    for C in (0, 9):
        with pytest.raises(RuntimeError, match="uh_tile_gather.*bad sizes"):
            gather(C=C)
    with pytest.raises(RuntimeError, match="uh_tile_gather.*misaligned"):
        gather(x=p + 2)
    with pytest.raises(RuntimeError, match="uh_tile_gather.*misaligned"):
        gather(tiles=p + 1)
    with pytest.raises(RuntimeError, match="uh_tile_merge.*null pointer"):
        merge(src=None)
    with pytest.raises(RuntimeError, match="uh_tile_merge.*null pointer"):
        merge(classes=None)                                             # no output at all
    for kind in (2, 4, -1, 0x100):
        with pytest.raises(RuntimeError, match="uh_tile_merge.*bad kind"):
            merge(kind=kind)
    for views in (0, 3, 5, 16, -1):
        with pytest.raises(RuntimeError, match="uh_tile_merge.*bad views"):
            merge(kind=SUMS, views=views)
    with pytest.raises(RuntimeError, match="uh_tile_merge.*bad views"):
        merge(kind=F32, views=8)                                        # logits are one view
    for NC in (0, -1, 257):
        with pytest.raises(RuntimeError, match="uh_tile_merge.*bad sizes"):
            merge(NC=NC)
    with pytest.raises(RuntimeError, match="uh_tile_merge.*misaligned"):
        merge(src=p + 2)                                                # fp32 logits at an odd half-word
    with pytest.raises(RuntimeError, match="uh_tile_merge.*misaligned"):
        merge(src=p + 1, kind=BF16)
    with pytest.raises(RuntimeError, match="uh_tile_merge.*misaligned"):
        merge(src=p + 2, kind=SUMS)
    with pytest.raises(RuntimeError, match="uh_tile_merge.*misaligned"):
        merge(sums=p + 4)                                               # 64-bit sums
    with pytest.raises(RuntimeError, match="uh_tile_merge.*misaligned"):
        merge(den=p + 2)
    with pytest.raises(RuntimeError, match="uh_tile_merge.*misaligned"):
        merge(probs=p + 2)
