"""CPU checks of knowledge distillation (DESIGN.md section 3 "Distillation"): the float64 restatement the GPU tests compare against
(tests/distill_ref.py) agrees with its own closed-form gradient and with the sigmoid statement of the one-channel head,
DistillConfig parses and refuses what it should, the C ABI refuses bad arguments without touching a GPU, and --distill takes
part in the --resume record with the digest of the teacher file."""
import hashlib
import logging

import pytest
import torch

import distill_ref as R


def _inputs(C, scale, n=257, seed=0):
    g = torch.Generator().manual_seed(seed + 13 * C)
    z = torch.randn(n, C, generator=g, dtype=torch.float64) * scale
    v = torch.randn(n, C, generator=g, dtype=torch.float64) * scale
    return z, v


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("C", [2, 3, 8])
@pytest.mark.parametrize("T", [0.5, 1.0, 2.0, 4.0])
@pytest.mark.parametrize("scale", [1.0, 10.0, 100.0])
def test_closed_form_gradient_is_autograd(C, T, scale):
    z, v = _inputs(C, scale)
    auto = R.autograd_gradient(z, v, T)
    closed = R.closed_form_gradient(z, v, T)
    assert torch.isfinite(auto).all() and torch.isfinite(closed).all()
    assert float((auto - closed).norm() / closed.norm()) <= 1e-12


@pytest.mark.parametrize("T", [0.5, 1.0, 2.0, 4.0])
def test_one_channel_form_is_the_two_class_form(T):
    """sigmoid statement of the one-channel head against the two-class softmax on the logits (0, z) and (0, v)."""
    g = torch.Generator().manual_seed(5)
    z = torch.randn(300, generator=g, dtype=torch.float64) * 4
    v = torch.randn(300, generator=g, dtype=torch.float64) * 4
    kd, agree = R.loss_terms(R.two_class_logits(z), R.two_class_logits(v), T)
    ls = torch.nn.functional.logsigmoid
    q1, q0 = torch.sigmoid(v / T), torch.sigmoid(-v / T)
    kl = q1 * (ls(v / T) - ls(z / T)) + q0 * (ls(-v / T) - ls(-z / T))
    assert torch.allclose(kd, T * T * kl.mean(), rtol=1e-12, atol=0)
    assert float(agree) == float(((z > 0) == (v > 0)).double().mean())
    # and the one-channel gradient is d kd / d z_1 of the two-class form: T / n (sigmoid(z / T) - sigmoid(v / T))
    closed = R.closed_form_gradient(R.two_class_logits(z), R.two_class_logits(v), T)[:, 1]
    want = T / 300 * (torch.sigmoid(z / T) - q1)
    assert float((closed - want).norm() / want.norm()) <= 1e-12
    zz = z.clone().requires_grad_(True)
    R.loss_terms(R.two_class_logits(zz), R.two_class_logits(v), T)[0].backward()
    assert float((zz.grad - closed).norm() / closed.norm()) <= 1e-12


@pytest.mark.parametrize("C", [2, 3, 8])
@pytest.mark.parametrize("scale", [1.0, 10.0, 100.0])
def test_kd_of_equal_logits_is_zero_and_kd_is_never_negative(C, scale):
    z, v = _inputs(C, scale)
    for T in (0.5, 1.0, 2.0, 4.0):
        kd, agree = R.loss_terms(z, z.clone(), T)
        assert float(kd) == 0.0 and float(agree) == 1.0
        assert float(R.closed_form_gradient(z, z.clone(), T).abs().max()) == 0.0
        kd, agree = R.loss_terms(z, v, T)
        assert float(kd) >= 0.0 and 0.0 <= float(agree) <= 1.0
        # Gibbs, pixel by pixel
        q, p = torch.softmax(v / T, 1), torch.softmax(z / T, 1)
        per_pixel = torch.where(q > 0, q * (torch.log_softmax(v / T, 1) - torch.log_softmax(z / T, 1)), torch.zeros_like(q)).sum(1)
        assert float(per_pixel.min()) >= -1e-15 and torch.isfinite(p).all()


def test_first_argmax_takes_the_first_of_equal_maxima():
    z = torch.tensor([[1.0, 1.0, 0.0], [0.0, 2.0, 2.0], [3.0, 1.0, 3.0], [0.0, 0.0, 0.0]], dtype=torch.float64)
    assert R.first_argmax(z).tolist() == [0, 1, 0, 0]
    # the one-channel head at z = 0: (0, 0), the first maximum is class 0
    assert R.first_argmax(R.two_class_logits(torch.tensor([0.0, -1.0, 1.0]))).tolist() == [0, 0, 1]


@pytest.mark.parametrize("C", [2, 3, 8])
def test_the_t_squared_factor_keeps_the_gradient_magnitude_across_temperatures(C):
    """The gradient of the bare KL falls as 1 / T^2; with the T^2 factor its norm stays within a factor 2 over T in {1, 2, 4} on
    N(0,1) logits (Hinton et al., section 2), so that w means the same at every temperature."""
    z, v = _inputs(C, 1.0)
    norms = [float(R.closed_form_gradient(z, v, T).norm()) for T in (1.0, 2.0, 4.0)]
    print(f"C {C}: gradient norms at T = 1, 2, 4: {norms}")
    assert max(norms) <= 2.0 * min(norms), norms
    bare = [n / (T * T) for n, T in zip(norms, (1.0, 2.0, 4.0))]
    assert max(bare) > 2.0 * min(bare)                                   # without the factor it does not


# ------------------------------------------------------------------------------------------------ DistillConfig
@pytest.mark.parametrize("spec,want", [
    ("teacher.pth", ("teacher.pth", "UNet", 2.0, 1.0)),
    ("runs/a b/model_epoch50_ema.pth,arch=UNet_S", ("runs/a b/model_epoch50_ema.pth", "UNet_S", 2.0, 1.0)),
    (" t.pth , w=0.5, T=4 ,arch=UNet_SA", ("t.pth", "UNet_SA", 4.0, 0.5)),
    ("/abs/checkpoint_epoch10.pth,T=1,arch=UNet_T", ("/abs/checkpoint_epoch10.pth", "UNet_T", 1.0, 1.0)),
    ("name=with=equals.pth,T=0.5", ("name=with=equals.pth", "UNet", 0.5, 1.0)),
])
def test_distill_config_parse_and_spec_round_trip(spec, want):
    import unet_amd
    cfg = unet_amd.DistillConfig.parse(spec)
    assert (cfg.teacher, cfg.arch, cfg.T, cfg.w) == want
    assert unet_amd.DistillConfig.parse(cfg.spec()) == cfg
    assert unet_amd.DistillConfig.of(spec) == cfg and unet_amd.DistillConfig.of(cfg) is cfg and unet_amd.DistillConfig.of(None) is None


def test_distill_config_defaults_are_the_bare_path():
    import unet_amd
    from unet_amd.train_cli import get_args
    assert unet_amd.DistillConfig("t.pth") == unet_amd.DistillConfig.parse("t.pth") == unet_amd.DistillConfig("t.pth", "UNet", 2.0, 1.0)
    assert unet_amd.DistillConfig("t.pth").spec() == "t.pth,arch=UNet,T=2.0,w=1.0"
    assert get_args(["--distill", "t.pth"]).distill == unet_amd.DistillConfig("t.pth") and get_args([]).distill is None
    assert get_args(["--distill", "t.pth,arch=UNet_S,T=3"]).distill == unet_amd.DistillConfig("t.pth", arch="UNet_S", T=3)
    with pytest.raises(TypeError):
        unet_amd.DistillConfig.of(3)


@pytest.mark.parametrize("bad,names", [
    ("", "path is missing"), (",T=2", "path is missing"), ("T=2", "path is missing"), ("arch=UNet,t.pth", "path is missing"),
    ("a,b.pth", "'b.pth'"), ("a,b.pth,T=2", "comma"),                     # a comma in the path
    ("t.pth,arch=ResNet", "arch"), ("t.pth,arch=unet", "arch"), ("t.pth,arch=", "arch="),
    ("t.pth,T=0", "temperature"), ("t.pth,T=-1", "temperature"), ("t.pth,T=inf", "temperature"), ("t.pth,T=nan", "temperature"),
    ("t.pth,T=hot", "temperature"), ("t.pth,w=-1", "weight"), ("t.pth,w=0", "weight"), ("t.pth,w=nan", "weight"),
    ("t.pth,w=x", "weight"), ("t.pth,T=1,T=2", "twice"), ("t.pth,arch=UNet,arch=UNet", "twice"), ("t.pth,w=1,w=1", "twice"),
    ("t.pth,tau=2", "'tau=2'"), ("t.pth,T", "'T'"), ("t.pth,,T=2", "''"),
])
def test_distill_config_refuses_a_malformed_spec_and_names_the_fault(bad, names):
    import unet_amd
    with pytest.raises(ValueError, match=names):
        unet_amd.DistillConfig.parse(bad)


def test_distill_config_refuses_bad_fields():
    import unet_amd
    with pytest.raises(ValueError, match="comma"):
        unet_amd.DistillConfig("a,b.pth")
    with pytest.raises(ValueError, match="arch"):
        unet_amd.DistillConfig("t.pth", arch="VGG")
    with pytest.raises(ValueError, match="temperature"):
        unet_amd.DistillConfig("t.pth", T=0)
    with pytest.raises(ValueError, match="weight"):
        unet_amd.DistillConfig("t.pth", w=-1)
    with pytest.raises(ValueError, match="teacher"):
        unet_amd.DistillConfig("")


# ------------------------------------------------------------------------------------------------ the C ABI
NAMES = ("uh_distill_nsums", "uh_distill_sums", "uh_distill_finish", "uh_distill_grad")


def test_header_declares_the_entry_points():
    import ctypes
    import unet_amd  # noqa: F401
    from unet_amd._lib import LIB_PATH, parse_header
    protos = parse_header()
    assert protos["uh_distill_nsums"] == ("int", [])
    assert protos["uh_distill_sums"] == ("int", ["ptr", "ptr", "int64_t", "int", "double", "ptr", "ptr", "size_t", "uh_stream"])
    assert protos["uh_distill_finish"] == ("int", ["ptr", "double", "double", "double", "ptr", "uh_stream"])
    assert protos["uh_distill_grad"] == ("int", ["ptr", "ptr", "int64_t", "int", "double", "double", "double", "ptr", "ptr", "uh_stream"])
    dll = ctypes.CDLL(LIB_PATH)
    for name in NAMES:
        assert hasattr(dll, name), f"{name} is not exported"
    # the loss it stands beside keeps its signatures
    assert protos["uh_focal_tversky_nsums"] == ("int", ["int"])
    assert protos["uh_ce_dice_sums"] == ("int", ["ptr", "ptr", "int64_t", "int", "ptr", "ptr", "size_t", "uh_stream"])


def test_the_source_is_built_into_the_one_library():
    import importlib.util
    import os
    import unet_amd
    spec = importlib.util.spec_from_file_location("_uh_build", os.path.join(os.path.dirname(unet_amd.__file__), "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    assert "distill_loss.hip" in build.SOURCES and os.path.isfile(os.path.join(build.CSRC, "distill_loss.hip"))


def test_bad_arguments_return_an_error_code_before_any_launch():
    """Every check sits in front of the launch: no GPU is touched (the device pointers are never followed)."""
    import unet_amd  # noqa: F401
    from unet_amd._lib import LIB
    LIB.load()
    P = 4096                                                            # a non-null stand-in for a device pointer
    big = LIB.query("uh_loss_ws_bytes", 100)
    nan, inf = float("nan"), float("inf")
    assert LIB.query("uh_distill_nsums") == 2

    def sums(student=P, teacher=P, npix=100, ncls=3, T=2.0, out=P, ws=P, ws_bytes=big):
        LIB.call("uh_distill_sums", student, teacher, npix, ncls, T, out, ws, ws_bytes, None)

    def finish(s=P, n_mean=100.0, T=2.0, w=1.0, out=P):
        LIB.call("uh_distill_finish", s, n_mean, T, w, out, None)

    def grad(student=P, teacher=P, npix=100, ncls=3, n_mean=100.0, T=2.0, w=1.0, dl=P):
        LIB.call("uh_distill_grad", student, teacher, npix, ncls, n_mean, T, w, None, dl, None)

    for call in (sums, grad):
        for ncls in (0, 9, -1):
            with pytest.raises(RuntimeError, match="classes, got"):
                call(ncls=ncls)
        for kw in ({"student": None}, {"teacher": None}, {"npix": 0}, {"npix": -5}):
            with pytest.raises(RuntimeError, match="bad args"):
                call(**kw)
    for call in (sums, finish, grad):
        for T in (0.0, -1.0, nan, inf):
            with pytest.raises(RuntimeError, match="temperature"):
                call(T=T)
    for call in (finish, grad):
        for w in (0.0, -1.0, nan, inf):
            with pytest.raises(RuntimeError, match="weight"):
                call(w=w)
        for n in (0.0, -3.0, nan, inf):
            with pytest.raises(RuntimeError, match="n_mean"):
                call(n_mean=n)
    with pytest.raises(RuntimeError, match="workspace too small"):
        sums(ws_bytes=big - 1)
    with pytest.raises(RuntimeError, match="bad args"):
        sums(out=None)
    with pytest.raises(RuntimeError, match="bad args"):
        sums(ws=None)
    with pytest.raises(RuntimeError, match="bad args"):
        grad(dl=None)
    with pytest.raises(RuntimeError, match="null"):
        finish(out=None)
    with pytest.raises(RuntimeError, match="null"):
        finish(s=None)


# ------------------------------------------------------------------------------------------------ the command line
BASE = ["--model", "UNet_T", "-c", "3", "-b", "4", "-s", "0.5"]


def _teacher_file(path, n_classes=3, arch="UNet_T", bilinear=False, seed=0):
    """A checkpoint of a freshly initialised network in the wire format of checkpoint.py, written on the CPU."""
    import unet_amd
    torch.manual_seed(seed)
    model = getattr(unet_amd, arch)(1, n_classes, bilinear=bilinear)
    return unet_amd.save_checkpoint(model, str(path), mask_values=[0, 1, 2])


def _state_file(path, argv=(), drop=(), change=None):
    """A hand-made --save-state file for BASE + argv; `drop`: keys taken out of its argument record, `change`: keys replaced."""
    from unet_amd.train_cli import get_args, run_record
    record = run_record(get_args(BASE + list(argv)))
    for k in drop:
        del record[k]
    record.update(change or {})
    state = {"format": 1, "model": {"w": torch.zeros(2)},
             "optimizer": {"square_avg": torch.zeros(4), "momentum_buffer": torch.zeros(4), "ema": None, "ema_updates": 0,
                           "layout": [[0, 2, [2]]], "total": 4, "hyper": {"lr": 1e-5}},
             "epoch": 1, "global_step": 2, "lr": 1e-5, "loader_seed": 1, "augment_seed": None, "args": record}
    torch.save(state, path)
    return str(path)


def test_run_record_holds_the_canonical_spec_and_the_digest_of_the_teacher_file(tmp_path):
    from unet_amd.train_cli import RECORDED, get_args, run_record
    assert ("distill", "--distill") in RECORDED
    teacher = _teacher_file(tmp_path / "teacher.pth")
    rec = run_record(get_args(BASE + ["--distill", f"{teacher}, T=4,arch=UNet_T"]))
    assert rec["distill"] == f"{teacher},arch=UNet_T,T=4.0,w=1.0"
    assert rec["distill_sha256"] == hashlib.sha256(open(teacher, "rb").read()).hexdigest()
    off = run_record(get_args(BASE))
    assert off["distill"] is None and off["distill_sha256"] is None
    assert sorted(rec) == sorted(k for k, _ in RECORDED) == sorted(off)
    with pytest.raises(ValueError, match="cannot be read"):
        run_record(get_args(BASE + ["--distill", str(tmp_path / "gone.pth")]))


@pytest.mark.parametrize("spec", ["t.pth,T=0", "t.pth,w=-1", "t.pth,arch=ResNet", "a,b.pth", "t.pth,T=1,T=2", ""])
def test_a_malformed_distill_spec_exits_with_status_2(capsys, spec):
    from unet_amd.train_cli import main
    with pytest.raises(SystemExit) as e:
        main(BASE + ["--distill", spec])
    assert e.value.code == 2 and "--distill" in capsys.readouterr().err


def test_a_missing_teacher_file_exits_with_status_2(tmp_path, caplog):
    from unet_amd.train_cli import main
    with caplog.at_level(logging.ERROR):
        assert main(BASE + ["--distill", str(tmp_path / "no_such_teacher.pth")]) == 2
    assert "--distill" in caplog.text and "does not exist" in caplog.text and "no_such_teacher.pth" in caplog.text
    assert "no GPU" not in caplog.text                               # refused for the argument, before a GPU is looked for


def test_a_file_that_is_no_checkpoint_exits_with_status_2(tmp_path, caplog):
    from unet_amd.train_cli import main
    junk = tmp_path / "junk.pth"
    junk.write_bytes(b"not a checkpoint")
    with caplog.at_level(logging.ERROR):
        assert main(BASE + ["--distill", str(junk)]) == 2
    assert "--distill" in caplog.text and "not a checkpoint" in caplog.text and "no GPU" not in caplog.text


@pytest.mark.parametrize("teacher_classes,student_classes", [(1, 3), (3, 1), (3, 2)])
def test_a_teacher_with_another_head_exits_with_status_2(tmp_path, caplog, teacher_classes, student_classes):
    from unet_amd.train_cli import main
    teacher = _teacher_file(tmp_path / "teacher.pth", n_classes=teacher_classes)
    with caplog.at_level(logging.ERROR):
        assert main(["--model", "UNet_T", "-b", "4", "-c", str(student_classes), "--distill", f"{teacher},arch=UNet_T"]) == 2
    assert "--distill" in caplog.text and "no GPU" not in caplog.text
    assert f"head of {teacher_classes} outputs" in caplog.text and f"one of {student_classes}" in caplog.text      # both sides


def test_the_teacher_shape_is_read_from_the_checkpoint_keys(tmp_path):
    from unet_amd.utils.distill import check_teacher, teacher_shape
    conv = _teacher_file(tmp_path / "convt.pth", n_classes=3, bilinear=False)
    bil = _teacher_file(tmp_path / "bilinear.pth", n_classes=1, arch="UNet_S", bilinear=True)
    assert teacher_shape(conv) == {"n_channels": 1, "n_classes": 3, "bilinear": False}
    assert teacher_shape(bil) == {"n_channels": 1, "n_classes": 1, "bilinear": True}
    assert check_teacher(f"{bil},arch=UNet_S", 1, 1)["bilinear"] is True
    with pytest.raises(ValueError, match="takes 1 input channels, the student 3"):
        check_teacher(conv, 3, 3)


def test_resume_refuses_a_differing_spec_and_a_differing_digest(tmp_path, caplog):
    from unet_amd.train_cli import get_args, load_resume_state, main
    teacher = _teacher_file(tmp_path / "teacher.pth")
    spec = f"{teacher},arch=UNet_T"
    cases = [((), ["--distill", spec]),                                               # saved without, resumed with
             (["--distill", spec], []),                                               # saved with, resumed without
             (["--distill", spec], ["--distill", spec + ",T=4"]),                     # another temperature
             (["--distill", spec], ["--distill", spec + ",w=0.5"])]                   # another weight
    for i, (saved, now) in enumerate(cases):
        path = _state_file(tmp_path / f"state{i}.pth", saved)
        args = BASE + now + ["--resume", path]
        with pytest.raises(ValueError, match=r"\-\-distill"):
            load_resume_state(get_args(args))
        caplog.clear()
        with caplog.at_level(logging.ERROR):
            assert main(args) == 2
        assert "--distill" in caplog.text
    # the same spec, another file behind the path: the digest differs
    path = _state_file(tmp_path / "state_digest.pth", ["--distill", spec])
    _teacher_file(teacher, seed=1)                                                    # retrained teacher, same name
    args = BASE + ["--distill", spec, "--resume", path]
    with pytest.raises(ValueError, match="SHA-256"):
        load_resume_state(get_args(args))
    caplog.clear()
    with caplog.at_level(logging.ERROR):
        assert main(args) == 2
    assert "SHA-256" in caplog.text and "distill_sha256" in caplog.text


def test_resume_accepts_the_same_spec_and_digest_and_a_state_from_before_the_option(tmp_path):
    from unet_amd.train_cli import get_args, load_resume_state
    teacher = _teacher_file(tmp_path / "teacher.pth")
    spec = f"{teacher},arch=UNet_T,T=2"
    same = _state_file(tmp_path / "a.pth", ["--distill", spec])
    assert load_resume_state(get_args(BASE + ["--distill", f"{teacher},T=2.0,arch=UNet_T,w=1", "--resume", same]))["epoch"] == 1
    old = _state_file(tmp_path / "b.pth", drop=("distill", "distill_sha256"))        # written before the keys existed: read as None
    assert load_resume_state(get_args(BASE + ["--resume", old]))["epoch"] == 1
    with pytest.raises(ValueError, match=r"\-\-distill"):
        load_resume_state(get_args(BASE + ["--distill", spec, "--resume", old]))
