"""CPU checks of checkpoint ensembles (DESIGN.md section 3 "Ensembles"): the refusals of the Ensemble container, the member
spec parser and its globs, both command-line parsers with one and with several -m items, and the argument checks of the two
launch entry points (host-only: they return before any launch)."""
import ctypes
import os

import pytest
import torch


def _net(arch="UNet_T", classes=3, bilinear=True):
    import unet_amd
    return getattr(unet_amd, arch)(1, classes, bilinear)


# ------------------------------------------------------------------ 1. the container
def test_ensemble_holds_members_and_weights():
    import unet_amd
    from unet_amd.utils.ensemble import Ensemble, single_model
    assert unet_amd.Ensemble is Ensemble
    a, b, c = _net(), _net("UNet_S", 3, False), _net("UNet_T", 3, False)            # architectures and upsampling may differ
    e = Ensemble([a, b, c])
    assert e.members == [a, b, c] and e.weights == [1, 1, 1] and e.total_weight == 3 and len(e) == 3
    assert (e.n_channels, e.n_classes) == (1, 3)
    assert not isinstance(e, torch.nn.Module)
    assert e.train() is e and all(m.training for m in e.members)
    assert e.eval() is e and not any(m.training for m in e.members)
    w = Ensemble([a, b], weights=[255, 2])
    assert w.weights == [255, 2] and w.total_weight == 257
    assert single_model(a) is a and single_model(Ensemble([a])) is a and single_model(Ensemble([a], [7])) is a
    assert single_model(e) is None


def test_ensemble_refusals():
    from unet_amd.utils.ensemble import Ensemble
    a = _net()
    with pytest.raises(ValueError, match="at least one"):
        Ensemble([])
    with pytest.raises(ValueError, match="head of 1 outputs"):
        Ensemble([a, _net(classes=1)])
    with pytest.raises(ValueError, match="head of 4 outputs"):
        Ensemble([a, a, _net(classes=4)])
    odd = _net()
    odd.n_channels = 3
    with pytest.raises(ValueError, match="input channels"):
        Ensemble([a, odd])
    with pytest.raises(ValueError, match="not"):
        Ensemble([a, torch.nn.Conv2d(1, 3, 1)])                                     # no n_classes: not one of the networks
    for bad in ([0, 1], [1, 256], [1, -1], [1, 1.0], [1, True], [1, "2"]):
        with pytest.raises(ValueError, match="weight"):
            Ensemble([a, a], weights=bad)
    with pytest.raises(ValueError, match="2 members"):
        Ensemble([a, a], weights=[1])
    with pytest.raises(ValueError, match="1024"):
        Ensemble([a] * 5, weights=[255, 255, 255, 255, 5])                          # 1025
    assert Ensemble([a] * 5, weights=[255, 255, 255, 255, 4]).total_weight == 1024


# ------------------------------------------------------------------ 2. member specs
def test_member_spec_parser():
    from unet_amd.utils.ensemble import MemberSpec, is_plain_single, parse_member_spec
    assert parse_member_spec("a.pth") == MemberSpec("a.pth", None, 1)
    assert parse_member_spec("a.pth,arch=UNet_S") == MemberSpec("a.pth", "UNet_S", 1)
    assert parse_member_spec("a.pth,w=2") == MemberSpec("a.pth", None, 2)
    assert parse_member_spec(" runs/*/m.pth , w = 255 , arch = UNet_T ") == MemberSpec("runs/*/m.pth", "UNet_T", 255)
    for bad in ("", ",w=2", "arch=UNet", "w=2", "a.pth,", "a.pth,w", "a.pth,w=", "a.pth,T=2", "a.pth,weight=2", "a.pth,w=0",
                "a.pth,w=256", "a.pth,w=1.5", "a.pth,w=-1", "a.pth,w=2,w=2", "a.pth,arch=VGG", "a.pth,arch=UNet,arch=UNet", None, 3):
        with pytest.raises(ValueError):
            parse_member_spec(bad)
    assert is_plain_single(["a.pth"]) and not is_plain_single(["a.pth", "b.pth"])
    assert not is_plain_single(["a.pth,w=2"]) and not is_plain_single(["ck/*.pth"])


def test_globs_expand_in_sorted_order(tmp_path):
    from unet_amd.utils.ensemble import MemberSpec, expand_member_specs
    for name in ("checkpoint_epoch10.pth", "checkpoint_epoch5.pth", "other.txt"):
        (tmp_path / name).write_bytes(b"")
    pattern = str(tmp_path / "checkpoint_epoch*.pth")
    got = expand_member_specs([pattern + ",w=3,arch=UNet_S", "plain.pth"])
    assert got == [MemberSpec(str(tmp_path / "checkpoint_epoch10.pth"), "UNet_S", 3),
                   MemberSpec(str(tmp_path / "checkpoint_epoch5.pth"), "UNet_S", 3), MemberSpec("plain.pth", None, 1)]
    with pytest.raises(ValueError, match="matches no file"):
        expand_member_specs([str(tmp_path / "nothing*.pth")])


def test_load_reads_upsampling_off_the_checkpoint_and_refuses_mismatches(tmp_path):
    import unet_amd
    from unet_amd.utils import distill, ensemble
    from unet_amd.utils.ensemble import Ensemble
    assert ensemble.teacher_shape is distill.teacher_shape                          # the helper is shared, not copied
    torch.manual_seed(0)
    a = unet_amd.save_checkpoint(_net("UNet_T", 3, True), str(tmp_path / "a.pth"), mask_values=[0, 1, 2])
    b = unet_amd.save_checkpoint(_net("UNet_T", 3, False), str(tmp_path / "b.pth"), mask_values=[0, 1, 2])
    s = unet_amd.save_checkpoint(_net("UNet_S", 3, False), str(tmp_path / "s.pth"), mask_values=[0, 1, 2])
    one = unet_amd.save_checkpoint(_net("UNet_T", 1, True), str(tmp_path / "one.pth"))
    e = Ensemble.load([a, b + ",w=2", s + ",arch=UNet_S"], 1, 3, "UNet_T", "cpu")
    assert [type(m).__name__ for m in e.members] == ["UNet_T", "UNet_T", "UNet_S"] and e.weights == [1, 2, 1]
    assert [m.bilinear for m in e.members] == [True, False, False]
    assert not any(m.training for m in e.members)
    assert [r["path"] for r in e.records] == [a, b, s] and [r["arch"] for r in e.records] == ["UNet_T", "UNet_T", "UNet_S"]
    assert e.records[1]["weight"] == 2 and e.records[0]["sha256"] == distill.teacher_sha256(a)
    g = Ensemble.load([str(tmp_path / "[ab].pth")], 1, 3, "UNet_T", "cpu")
    assert [r["path"] for r in g.records] == [a, b]
    with pytest.raises(ValueError, match="head of 1 outputs"):
        Ensemble.load([a, one], 1, 3, "UNet_T", "cpu")
    with pytest.raises(ValueError, match="does not hold a UNet_S"):
        Ensemble.load([a + ",arch=UNet_S"], 1, 3, "UNet_T", "cpu")
    with pytest.raises(ValueError, match="does not exist"):
        Ensemble.load([str(tmp_path / "absent.pth")], 1, 3, "UNet_T", "cpu")


# ------------------------------------------------------------------ 3. command lines
def test_command_lines_take_one_or_several_models(capsys):
    from unet_amd import evaluate_cli, predict_cli
    pred = ["-i", "x.png"]
    ev = ["--data-root", "d"]
    for cli, rest in ((predict_cli, pred), (evaluate_cli, ev)):
        one = cli.get_args(["-m", "m.pth"] + rest)
        assert one.model == "m.pth" and one.members == ["m.pth"]                    # one -m: the string it has always been
        many = cli.get_args(["-m", "a.pth", "b.pth,w=2", "ck/*.pth,arch=UNet_T"] + rest)
        assert many.members == ["a.pth", "b.pth,w=2", "ck/*.pth,arch=UNet_T"] and many.model == many.members
        assert cli.get_args(rest + ["--model", "a.pth", "b.pth"]).members == ["a.pth", "b.pth"]
        for bad in (["-m"], ["-m", "a.pth", "b.pth,w=0"], ["-m", "a.pth,arch=VGG"], ["-m", "a.pth,scale=2"]):
            with pytest.raises(SystemExit) as e:
                cli.get_args(bad + rest)
            assert e.value.code == 2
        capsys.readouterr()
    assert predict_cli.get_args(["-m", "m.pth"] + pred).confidence_dir is None
    assert predict_cli.get_args(["-m", "a.pth", "b.pth", "--confidence-dir", "c"] + pred).confidence_dir == "c"
    assert predict_cli.confidence_path("c", "in/sub/a.jpg") == os.path.join("c", "a_conf.png")
    members = [{"path": "a.pth", "arch": "UNet", "bilinear": False, "weight": 2, "sha256": "00"}]
    rep = evaluate_cli.report((0.5, 0.25, 0.125), None, members=members)
    assert rep["members"] == [{"path": "a.pth", "arch": "UNet", "weight": 2, "sha256": "00"}]
    assert "members" not in evaluate_cli.report((0.5, 0.25, 0.125), None)


def test_predict_refuses_bad_members_before_the_device(tmp_path, caplog):
    import logging
    import numpy as np
    from PIL import Image
    import unet_amd
    from unet_amd.predict_cli import main
    img = str(tmp_path / "x.png")
    Image.fromarray(np.zeros((8, 8), np.uint8)).save(img)
    a = unet_amd.save_checkpoint(_net("UNet_T", 3, True), str(tmp_path / "a.pth"))
    with caplog.at_level(logging.ERROR):
        assert main(["-m", a, "model.pt", "-i", img]) == 1
        assert "TorchScript" in caplog.text
        caplog.clear()
        assert main(["-m", a, str(tmp_path / "absent.pth"), "-i", img, "--arch", "UNet_T"]) == 1
        assert "Failed to load the model" in caplog.text and "does not exist" in caplog.text
        caplog.clear()
        assert main(["-m", a, "-i", img, "--arch", "UNet_T", "--bilinear", "--confidence-dir", str(tmp_path / "c")]) == 1
        assert "--confidence-dir needs an ensemble" in caplog.text


def test_constructors_and_no_cpu_fallback():
    from unet_amd import ops
    from unet_amd.predict import BatchPredictor
    p = object.__new__(BatchPredictor)
    p.tta = p.tile = p.ensemble = None
    with pytest.raises(RuntimeError, match="ensemble"):
        p.confidence([])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ensemble_add(torch.zeros(1, 3, 4, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ensemble_finish(torch.zeros(1, 4, 4, 3, dtype=torch.int64), 2)


# ------------------------------------------------------------------ 4. the entry points check their arguments
def test_symbols_declared_exported_and_arguments_checked():
    import unet_amd  # noqa: F401
    from unet_amd import ops
    from unet_amd._lib import LIB, LIB_PATH
    dll = ctypes.CDLL(LIB_PATH)
    for name in ("uh_ensemble_add", "uh_ensemble_finish"):
        assert name in LIB.protos, f"{name} is not declared in include/unet_hip.h"
        assert hasattr(dll, name), f"{name} is not exported"
    assert LIB.protos["uh_ensemble_add"][1] == ["ptr", "int", "int64_t", "int", "unsigned", "int", "ptr", "uh_stream"]
    assert LIB.protos["uh_ensemble_finish"][1] == ["ptr", "ptr", "int", "unsigned", "int64_t", "int", "ptr", "ptr", "ptr", "uh_stream"]
    assert (ops.UH_TILE_SUMS_I32, ops.UH_ENS_SUMS_U64) == (3, 4)
    LIB.load()
    p = 4096                                                            # a non-null pointer that is never dereferenced
    F32, BF16, S32, S64 = 0, 1, 3, 4

    def add(src=p, kind=F32, npix=10, NC=3, weight=1, first=1, acc=p):
        LIB.call("uh_ensemble_add", src, kind, npix, NC, weight, first, acc, None)

    def finish(acc=p, den=None, views=1, total=2, npix=10, NC=3, classes=p, probs=None, confidence=None):
        LIB.call("uh_ensemble_finish", acc, den, views, total, npix, NC, classes, probs, confidence, None)

    for fn, name in ((add, "uh_ensemble_add"), (finish, "uh_ensemble_finish")):
        for NC in (0, -1, 257):
            with pytest.raises(RuntimeError, match=name + ".*bad sizes"):
                fn(NC=NC)
        for npix in (0, -5):
            with pytest.raises(RuntimeError, match=name + ".*bad sizes"):
                fn(npix=npix)
        with pytest.raises(RuntimeError, match=name + ".*null pointer"):
            fn(acc=None)
        with pytest.raises(RuntimeError, match=name + ".*misaligned"):
            fn(acc=p + 4)                                               # 64-bit sums
    with pytest.raises(RuntimeError, match="uh_ensemble_add.*null pointer"):
        add(src=None)
    for weight in (0, 1025, 1 << 20):
        with pytest.raises(RuntimeError, match="uh_ensemble_add.*bad weight"):
            add(weight=weight)
    for kind in (2, 5, -1, 0x100):
        with pytest.raises(RuntimeError, match="uh_ensemble_add.*bad kind"):
            add(kind=kind)
    with pytest.raises(RuntimeError, match="uh_ensemble_add.*misaligned"):
        add(src=p + 2)                                                  # fp32 logits at an odd half-word
    with pytest.raises(RuntimeError, match="uh_ensemble_add.*misaligned"):
        add(src=p + 1, kind=BF16)
    with pytest.raises(RuntimeError, match="uh_ensemble_add.*misaligned"):
        add(src=p + 2, kind=S32)
    with pytest.raises(RuntimeError, match="uh_ensemble_add.*misaligned"):
        add(src=p + 4, kind=S64)
    for views in (0, 3, 5, 16, -1):
        with pytest.raises(RuntimeError, match="uh_ensemble_finish.*bad views"):
            finish(views=views)
    for total in (0, 1025):
        with pytest.raises(RuntimeError, match="uh_ensemble_finish.*bad total_weight"):
            finish(total=total)
    with pytest.raises(RuntimeError, match="uh_ensemble_finish.*null pointer"):
        finish(classes=None)                                            # no output at all
    with pytest.raises(RuntimeError, match="uh_ensemble_finish.*misaligned"):
        finish(den=p + 2)
    with pytest.raises(RuntimeError, match="uh_ensemble_finish.*misaligned"):
        finish(probs=p + 2)
