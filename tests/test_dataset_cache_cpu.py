"""The host side of the dataset cache (utils/dataset_cache.py, csrc/cache.hip): the arena layout, the item -> (entry, turns) map,
the --cache option and the build wiring.  No GPU."""
import os

import pytest

from conftest import ROOT

SHAPES = [(5, 7, 1), (33, 31, 3), (16, 16, 1)]


def _bytes(shape):
    H, W, C = shape
    return H * W * C, H * W


def test_plan_entries_hand_computed_case():
    from unet_amd import plan_entries
    io, mo, total = plan_entries(SHAPES)
    # (5,7,1): 35 -> 48 + 35 -> 48;  (33,31,3): 3069 -> 3072 + 1023 -> 1024;  (16,16,1): 256 + 256
    assert io == [0, 96, 4192]
    assert mo == [48, 3168, 4448]
    assert total == 48 + 48 + 3072 + 1024 + 256 + 256 == 4704


@pytest.mark.parametrize("shapes", [SHAPES, SHAPES[::-1], [(1, 1, 1)], [(64, 48, 4), (5, 7, 1), (5, 7, 1), (17, 1, 2)]])
def test_plan_entries_alignment_padding_and_no_overlap(shapes):
    from unet_amd import plan_entries
    io, mo, total = plan_entries(shapes)
    assert len(io) == len(mo) == len(shapes)
    assert all(o % 16 == 0 for o in io + mo) and total % 16 == 0
    spans = []
    for s, i, m in zip(shapes, io, mo):
        ib, mb = _bytes(s)
        spans += [(i, i + -(-ib // 16) * 16), (m, m + -(-mb // 16) * 16)]       # every entry padded to a multiple of 16
    assert spans[0][0] == 0 and spans[-1][1] == total
    for (a0, a1), (b0, b1) in zip(spans, spans[1:]):
        assert a1 == b0 and a0 < a1                                                 # image, mask, image, ...: dense, disjoint
    assert plan_entries([]) == ([], [], 0)
    with pytest.raises(ValueError):
        plan_entries([(0, 4, 1)])


def test_index_to_entry_and_turns():
    from unet_amd.utils.dataset_cache import entry_of
    from unet_amd.utils.data_loading import QUARTER_TURNS
    assert QUARTER_TURNS == 4
    assert [entry_of(i, True) for i in range(9)] == [(0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (1, 1), (1, 2), (1, 3), (2, 0)]
    assert [entry_of(i, False) for i in range(4)] == [(0, 0), (1, 0), (2, 0), (3, 0)]


def test_cache_option_parses_and_is_not_a_determining_argument():
    from unet_amd import train_cli
    assert train_cli.get_args([]).cache is None
    assert train_cli.get_args(["--cache"]).cache == train_cli.CacheSpec(None)
    assert train_cli.get_args(["--cache", "limit=0.5"]).cache == train_cli.CacheSpec(1 << 29)
    assert train_cli.get_args(["--cache", "limit=0.000001"]).cache.limit_bytes == 1073
    assert "cache" not in dict(train_cli.RECORDED)
    with_cache, without = train_cli.get_args(["--cache"]), train_cli.get_args([])
    assert train_cli.run_record(with_cache) == train_cli.run_record(without)
    assert "--cache [limit=GiB]" in train_cli.__doc__


@pytest.mark.parametrize("spec", ["limit", "limit=", "limit=x", "limit=0", "limit=-1", "limit=inf", "size=1", "0.5"])
def test_bad_cache_spec_exits_with_status_2(spec, capsys):
    from unet_amd import train_cli
    with pytest.raises(SystemExit) as e:
        train_cli.get_args(["--cache", spec])
    assert e.value.code == 2 and "--cache" in capsys.readouterr().err


def test_source_is_built_and_declared():
    import importlib.util
    spec = importlib.util.spec_from_file_location("_uh_build_cache_test",
                                                  os.path.join(ROOT, "unet-medical-image-contour-segmentation_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    assert "cache.hip" in build.SOURCES and os.path.isfile(os.path.join(build.CSRC, "cache.hip"))
    from unet_amd._lib import parse_header
    ret, args = parse_header()["uh_cache_gather_u8"]
    assert ret == "int" and args == ["ptr", "int", "size_t", "size_t", "ptr", "ptr", "uh_stream"]
    text = open(os.path.join(ROOT, "include", "unet_hip.h")).read()
    assert "typedef struct uh_cache_item" in text and "rounded up to 16" in text.lower()


def test_loader_refuses_a_cache_it_cannot_use():
    from unet_amd.utils.data_loading import DeviceBatchLoader
    ds = list(range(4))
    with pytest.raises(ValueError, match="host_rescale"):
        DeviceBatchLoader(ds, 2, host_rescale=True, cache=object())
    with pytest.raises(ValueError, match="DatasetCache"):
        DeviceBatchLoader(ds, 2, cache="yes")
    assert DeviceBatchLoader(ds, 2).cache is None
