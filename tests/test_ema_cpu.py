"""CPU checks of the averaged weights and the resumable training state (DESIGN.md section 3 "Averaged weights and resumable
state"): EmaConfig, the three new C-ABI entry points as the header declares them and as they refuse bad arguments, and the
--ema / --save-state / --resume argument handling, which answers before a GPU is looked for."""
import ctypes
import logging

import pytest
import torch


# ------------------------------------------------------------------------------------------------ EmaConfig
@pytest.mark.parametrize("spec,decay,warmup", [("0.999,warmup=10", 0.999, 10), ("0.9", 0.9, 10), ("0.99, warmup=0", 0.99, 0),
                                               ("0.5,warmup=3", 0.5, 3)])
def test_ema_config_parse_and_spec_round_trip(spec, decay, warmup):
    import unet_amd
    cfg = unet_amd.EmaConfig.parse(spec)
    assert (cfg.decay, cfg.warmup) == (decay, warmup)
    assert unet_amd.EmaConfig.parse(cfg.spec()) == cfg
    assert unet_amd.EmaConfig.of(spec) == cfg and unet_amd.EmaConfig.of(cfg) is cfg and unet_amd.EmaConfig.of(None) is None


def test_ema_config_defaults_are_the_bare_flag():
    import unet_amd
    from unet_amd.train_cli import EMA_BARE, get_args
    assert unet_amd.EmaConfig() == unet_amd.EmaConfig.parse(EMA_BARE) == unet_amd.EmaConfig(0.999, 10)
    assert get_args(["--ema"]).ema == unet_amd.EmaConfig() and get_args([]).ema is None
    assert get_args(["--ema", "0.9,warmup=0"]).ema == unet_amd.EmaConfig(0.9, 0)


@pytest.mark.parametrize("decay", [0.0, 1.0, -0.1, 1.5, float("nan")])
def test_ema_config_rejects_decay_outside_the_open_interval(decay):
    import unet_amd
    with pytest.raises(ValueError, match="decay"):
        unet_amd.EmaConfig(decay, 10)
    with pytest.raises(ValueError, match="decay"):
        unet_amd.EmaConfig.parse(f"{decay!r},warmup=10")


def test_ema_config_rejects_a_negative_warmup_and_unknown_keys():
    import unet_amd
    with pytest.raises(ValueError, match="warmup"):
        unet_amd.EmaConfig(0.9, -1)
    with pytest.raises(ValueError, match="warmup"):
        unet_amd.EmaConfig.parse("0.9,warmup=-1")
    for bad in ("", "warmup=3", "0.9,warm=3", "0.9,warmup", "0.9,warmup=2,warmup=3", "0.9,warmup=1.5", "abc"):
        with pytest.raises(ValueError):
            unet_amd.EmaConfig.parse(bad)
    with pytest.raises(SystemExit):
        from unet_amd.train_cli import get_args
        get_args(["--ema", "1.5"])


# ------------------------------------------------------------------------------------------------ the C ABI
def test_header_declares_the_three_prototypes():
    import unet_amd  # noqa: F401
    from unet_amd._lib import LIB_PATH, parse_header
    protos = parse_header()
    assert protos["uh_rmsprop_step_ema"] == ("int", ["ptr"] * 5 + ["int64_t", "ptr"] + ["float"] * 7 + ["int", "ptr", "uh_stream"])
    assert protos["uh_ema_tick"] == ("int", ["ptr", "ptr", "uh_stream"])
    assert protos["uh_swap_f32"] == ("int", ["ptr", "ptr", "int64_t", "uh_stream"])
    # the pass it extends keeps its signature
    assert protos["uh_rmsprop_step"] == ("int", ["ptr"] * 4 + ["int64_t", "ptr"] + ["float"] * 6 + ["uh_stream"])
    dll = ctypes.CDLL(LIB_PATH)
    for name in ("uh_rmsprop_step_ema", "uh_ema_tick", "uh_swap_f32"):
        assert hasattr(dll, name), f"{name} is not exported"


def test_bad_arguments_raise_before_any_launch():
    """Every check sits in front of the launch: no GPU is touched (the pointers are never followed)."""
    import unet_amd  # noqa: F401
    from unet_amd._lib import LIB
    LIB.load()
    P, Q = 4096, 1 << 20                                          # non-null, 16-byte aligned stand-in pointers
    ok = (1.0, 1e-5, 0.99, 1e-8, 1e-8, 0.999)
    with pytest.raises(RuntimeError, match="uh_rmsprop_step_ema"):
        LIB.call("uh_rmsprop_step_ema", P, P, P, P, None, 8, None, *ok, 0.999, 10, P, None)          # no average
    with pytest.raises(RuntimeError, match="uh_rmsprop_step_ema"):
        LIB.call("uh_rmsprop_step_ema", P, P, P, P, Q, 8, None, *ok, 0.999, 10, None, None)          # no counter
    with pytest.raises(RuntimeError, match="16-byte"):
        LIB.call("uh_rmsprop_step_ema", P, P, P, P, Q + 4, 8, None, *ok, 0.999, 10, P, None)
    for decay, warmup in ((0.0, 10), (1.0, 10), (0.9, -1)):
        with pytest.raises(RuntimeError, match="decay"):
            LIB.call("uh_rmsprop_step_ema", P, P, P, P, Q, 8, None, *ok, decay, warmup, P, None)
    with pytest.raises(RuntimeError, match="uh_ema_tick"):
        LIB.call("uh_ema_tick", None, None, None)
    with pytest.raises(RuntimeError, match="uh_swap_f32"):
        LIB.call("uh_swap_f32", P, Q, 0, None)
    with pytest.raises(RuntimeError, match="16-byte"):
        LIB.call("uh_swap_f32", P, Q + 8, 16, None)
    with pytest.raises(RuntimeError, match="overlap"):
        LIB.call("uh_swap_f32", P, P + 16, 16, None)


# ------------------------------------------------------------------------------------------------ the command line
def _state_file(path, **changed):
    """A hand-made --save-state file for `--model UNet_T -c 3 -b 4 -s 0.5 -l 1e-5`, bf16, no options; `changed` overrides
    entries of its argument record."""
    from unet_amd.train_cli import get_args, run_record
    record = run_record(get_args(["--model", "UNet_T", "-c", "3", "-b", "4", "-s", "0.5"]))
    record.update(changed)
    state = {"format": 1, "model": {"w": torch.zeros(2)},
             "optimizer": {"square_avg": torch.zeros(4), "momentum_buffer": torch.zeros(4), "ema": None, "ema_updates": 0,
                           "layout": [[0, 2, [2]]], "total": 4, "hyper": {"lr": 1e-5}},
             "epoch": 1, "global_step": 2, "lr": 1e-5, "loader_seed": 1, "augment_seed": None, "args": record}
    torch.save(state, path)
    return str(path)


BASE = ["--model", "UNet_T", "-c", "3", "-b", "4", "-s", "0.5"]


def test_run_record_holds_the_determining_arguments_in_canonical_form():
    from unet_amd.train_cli import RECORDED, get_args, run_record
    rec = run_record(get_args(BASE + ["--augment", "flip", "--elastic", "grid=16,sigma=1", "--ema", "0.9,warmup=0",
                                      "--surface-loss", "0.5,classes=1+2", "--bilinear", "--no-amp"]))
    assert sorted(rec) == sorted(k for k, _ in RECORDED)
    assert (rec["model"], rec["classes"], rec["bilinear"], rec["batch_size"], rec["scale"], rec["amp"], rec["lr"]) == \
        ("UNet_T", 3, True, 4, 0.5, False, 1e-5)
    assert rec["ema"] == "0.9,warmup=0" and rec["elastic"] == "grid=16,sigma=1.0,p=1.0" and rec["surface"] == "0.5,ramp=0.0,classes=1+2"
    assert rec["augment"] == run_record(get_args(BASE + ["--augment", "hflip=0.5,vflip=0.5"]))["augment"]
    off = run_record(get_args(BASE))
    assert off["augment"] is off["elastic"] is off["surface"] is off["ema"] is None


def test_resume_accepts_the_run_that_wrote_the_state(tmp_path):
    from unet_amd.train_cli import get_args, load_resume_state
    path = _state_file(tmp_path / "train_state.pth")
    state = load_resume_state(get_args(BASE + ["--resume", path, "-e", "7", "--seed", "3"]))      # -e and --seed are free
    assert state["epoch"] == 1 and state["global_step"] == 2
    assert load_resume_state(get_args(BASE)) is None


def test_load_with_resume_fails(tmp_path, caplog):
    from unet_amd.train_cli import get_args, load_resume_state, main
    path = _state_file(tmp_path / "train_state.pth")
    with pytest.raises(ValueError, match="--load"):
        load_resume_state(get_args(BASE + ["--resume", path, "-f", "weights.pth"]))
    with caplog.at_level(logging.ERROR):
        assert main(BASE + ["--resume", path, "-f", "weights.pth"]) == 2
    assert "--load" in caplog.text and "--resume" in caplog.text


@pytest.mark.parametrize("argv,name", [(["-c", "2"], "--classes"), (["--model", "UNet_S"], "--model"), (["--bilinear"], "--bilinear"),
                                       (["-b", "2"], "--batch-size"), (["-s", "0.25"], "--scale"), (["--no-amp"], "--amp"),
                                       (["-l", "1e-4"], "--learning-rate"), (["--augment"], "--augment"),
                                       (["--elastic"], "--elastic"), (["--surface-loss"], "--surface-loss"), (["--ema"], "--ema")])
def test_resume_refuses_a_changed_determining_argument(tmp_path, caplog, argv, name):
    from unet_amd.train_cli import get_args, load_resume_state, main
    path = _state_file(tmp_path / "train_state.pth")
    args = BASE + argv + ["--resume", path]                         # (a later option wins in argparse)
    with pytest.raises(ValueError, match=name.replace("-", r"\-")):
        load_resume_state(get_args(args))
    with caplog.at_level(logging.ERROR):
        assert main(args) == 2
    assert name in caplog.text


def test_resume_names_classes_when_the_record_differs(tmp_path, caplog):
    """The state was saved by a 2-class run; the command line asks for 3."""
    from unet_amd.train_cli import main
    path = _state_file(tmp_path / "train_state.pth", classes=2)
    with caplog.at_level(logging.ERROR):
        assert main(BASE + ["--resume", path]) == 2
    assert "--classes" in caplog.text and "classes" in caplog.text and "2" in caplog.text and "3" in caplog.text
    assert "no GPU" not in caplog.text                               # refused for the argument, before a GPU is looked for


def test_resume_refuses_a_state_with_no_epoch_left(tmp_path, caplog):
    """The hand-made state was saved after epoch 1: -e 1 leaves nothing to train (and would label the final files wrongly)."""
    from unet_amd.train_cli import get_args, load_resume_state, main
    path = _state_file(tmp_path / "train_state.pth")
    with pytest.raises(ValueError, match="no epoch is left"):
        load_resume_state(get_args(BASE + ["--resume", path, "-e", "1"]))
    with caplog.at_level(logging.ERROR):
        assert main(BASE + ["--resume", path, "-e", "1"]) == 2
    assert "--epochs" in caplog.text
    assert load_resume_state(get_args(BASE + ["--resume", path, "-e", "2"]))["epoch"] == 1


def test_resume_refuses_a_file_that_is_no_training_state(tmp_path):
    from unet_amd.train_cli import get_args, load_resume_state
    path = tmp_path / "weights.pth"
    torch.save({"w": torch.zeros(2)}, path)
    with pytest.raises(ValueError, match="not a training state"):
        load_resume_state(get_args(BASE + ["--resume", str(path)]))
