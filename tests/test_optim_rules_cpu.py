"""The CPU side of the AdamW and SGD rules of the fused optimizer pass: OptimConfig's grammar, --optimizer, the run record and
--resume's refusal, the four new entry points in header and binding, and the proof that goes with tests/test_gpu_optim_rules.py:
numpy float32 restatements of the kernels' statements meet every bound of tests/optim_rule_cases.py with half the room to spare,
each seeded mistake breaks at least one, and the float64 reference equals stock torch.optim.AdamW / SGD.  No test needs a GPU."""
import logging
import re

import numpy as np
import pytest
import torch

import optim_cases as K
import optim_rule_cases as R

F = np.float32
BASE = ["--model", "UNet_T", "-c", "3", "-b", "4", "-s", "0.5"]


# ------------------------------------------------------------------------------------------------ OptimConfig
def test_defaults_of_each_rule():
    from unet_amd import OptimConfig
    a, s, r = OptimConfig.parse("adamw"), OptimConfig.parse("sgd"), OptimConfig.parse("rmsprop")
    assert (a.rule, a.betas, a.eps, a.wd) == ("adamw", (0.9, 0.999), 1e-8, 0.01) and a.momentum is a.alpha is a.nesterov is None
    assert (s.rule, s.momentum, s.nesterov, s.wd) == ("sgd", 0.99, True, 3e-5) and s.betas is s.eps is s.alpha is None
    assert (r.rule, r.alpha, r.eps, r.momentum, r.wd) == ("rmsprop", 0.99, 1e-8, 0.999, 1e-8) and r.betas is r.nesterov is None
    assert OptimConfig() == r and OptimConfig("adamw") == a and OptimConfig("sgd") == s
    assert OptimConfig.of(None) is None and OptimConfig.of(a) is a and OptimConfig.of("sgd") == s
    with pytest.raises(TypeError):
        OptimConfig.of(3)


@pytest.mark.parametrize("spec,canonical", [
    ("adamw", "adamw,betas=0.9/0.999,eps=1e-08,wd=0.01"),
    (" adamw , wd=0.05 , betas=0.8/0.99 ", "adamw,betas=0.8/0.99,eps=1e-08,wd=0.05"),
    ("adamw,eps=1e-6,wd=0", "adamw,betas=0.9/0.999,eps=1e-06,wd=0.0"),
    ("sgd", "sgd,momentum=0.99,nesterov,wd=3e-05"),
    ("sgd,plain,momentum=0.9", "sgd,momentum=0.9,plain,wd=3e-05"),
    ("sgd,momentum=0,plain,wd=0", "sgd,momentum=0.0,plain,wd=0.0"),
    ("sgd,nesterov", "sgd,momentum=0.99,nesterov,wd=3e-05"),
    ("rmsprop", "rmsprop,alpha=0.99,eps=1e-08,momentum=0.999,wd=1e-08"),
    ("rmsprop,momentum=0,alpha=0.9", "rmsprop,alpha=0.9,eps=1e-08,momentum=0.0,wd=1e-08"),
])
def test_spec_is_canonical_and_round_trips(spec, canonical):
    from unet_amd import OptimConfig
    cfg = OptimConfig.parse(spec)
    assert cfg.spec() == canonical
    assert OptimConfig.parse(cfg.spec()) == cfg and OptimConfig.parse(canonical).spec() == canonical


@pytest.mark.parametrize("spec,token", [
    ("adam", "adam"), ("", "''"), ("lion,wd=1", "lion"),                                 # an unknown rule
    ("adamw,wd=0.1,wd=0.2", "wd=0.2"), ("sgd,nesterov,plain", "plain"),                 # a key given twice
    ("adamw,momentum=0.9", "momentum=0.9"), ("sgd,betas=0.9/0.99", "betas=0.9/0.99"),    # a key of another rule
    ("rmsprop,nesterov", "nesterov"), ("sgd,alpha=0.9", "alpha=0.9"), ("adamw,lr=1e-3", "lr=1e-3"),
    ("adamw,betas=1/0.9", "betas=1/0.9"), ("adamw,betas=0.9/1.0", "betas=0.9/1.0"),      # betas outside [0, 1)
    ("adamw,betas=-0.1/0.9", "betas=-0.1/0.9"), ("adamw,betas=0.9", "betas=0.9"), ("adamw,betas=a/b", "betas=a/b"),
    ("adamw,eps=-1e-8", "eps=-1e-8"), ("adamw,wd=-1", "wd=-1"), ("sgd,wd=-0.1", "wd=-0.1"),      # negative values
    ("sgd,momentum=-0.5", "momentum=-0.5"), ("rmsprop,momentum=-1", "momentum=-1"), ("rmsprop,eps=-1", "eps=-1"),
    ("sgd,momentum=0", "momentum=0"), ("sgd,momentum=0,nesterov", "momentum=0"),         # nesterov without momentum
    ("adamw,wd", "wd"), ("adamw,wd=", "wd="), ("adamw,eps=tiny", "eps=tiny"), ("sgd,wd=nan", "wd=nan"),
])
def test_parse_names_the_token_that_is_wrong(spec, token):
    from unet_amd import OptimConfig
    with pytest.raises(ValueError, match=re.escape(token)):
        OptimConfig.parse(spec)


def test_constructor_checks_what_parse_checks():
    from unet_amd import OptimConfig
    for kw in (dict(rule="adamw", betas=(0.9, 1.0)), dict(rule="adamw", momentum=0.9), dict(rule="sgd", momentum=0.0),
               dict(rule="sgd", wd=-1.0), dict(rule="adam"), dict(rule="rmsprop", alpha=1.5), dict(rule="adamw", eps=float("inf"))):
        with pytest.raises(ValueError):
            OptimConfig(**kw)
    assert OptimConfig("sgd", momentum=0.0, nesterov=False).spec() == "sgd,momentum=0.0,plain,wd=3e-05"


# ------------------------------------------------------------------------------------------------ command line
def test_optimizer_flag_through_get_args(capsys):
    from unet_amd import OptimConfig
    from unet_amd.train import get_args
    assert get_args(BASE).optimizer is None
    args = get_args(BASE + ["--optimizer", "adamw,wd=0.05"])
    assert args.optimizer == OptimConfig("adamw", wd=0.05) and args.lr == 1e-5
    assert get_args(BASE + ["--optimizer", "sgd,plain", "-l", "0.01"]).optimizer.nesterov is False
    for bad in ("adam", "adamw,betas=1/1", "sgd,momentum=0"):
        with pytest.raises(SystemExit) as e:
            get_args(BASE + ["--optimizer", bad])
        assert e.value.code == 2
        assert "--optimizer" in capsys.readouterr().err


def test_run_record_has_the_key_on_and_off():
    from unet_amd.train_cli import RECORDED, get_args, run_record
    assert ("optimizer", "--optimizer") in RECORDED
    on = run_record(get_args(BASE + ["--optimizer", "sgd,momentum=0.9"]))
    off = run_record(get_args(BASE))
    assert sorted(on) == sorted(k for k, _ in RECORDED) == sorted(off)
    assert on["optimizer"] == "sgd,momentum=0.9,nesterov,wd=3e-05" and off["optimizer"] is None
    assert {k: v for k, v in on.items() if k != "optimizer"} == {k: v for k, v in off.items() if k != "optimizer"}


def _state_file(path, drop=(), **changed):
    """A hand-made --save-state file as tests/test_ema_cpu.py builds it; `changed` overrides entries of its argument record,
    `drop` removes some (a state written before the key existed)."""
    from unet_amd.train_cli import get_args, run_record
    record = run_record(get_args(BASE))
    record.update(changed)
    for k in drop:
        del record[k]
    state = {"format": 1, "model": {"w": torch.zeros(2)},
             "optimizer": {"square_avg": torch.zeros(4), "momentum_buffer": torch.zeros(4), "ema": None, "ema_updates": 0,
                           "layout": [[0, 2, [2]]], "total": 4, "hyper": {"lr": 1e-5}},
             "epoch": 1, "global_step": 2, "lr": 1e-5, "loader_seed": 1, "augment_seed": None, "args": record}
    torch.save(state, path)
    return str(path)


def test_resume_refuses_another_optimizer_and_accepts_an_old_record(tmp_path, caplog):
    from unet_amd.train_cli import get_args, load_resume_state, main
    old = _state_file(tmp_path / "old.pth", drop=("optimizer",))                 # written before the option existed
    assert load_resume_state(get_args(BASE + ["--resume", old]))["epoch"] == 1
    with pytest.raises(ValueError, match=r"\-\-optimizer"):
        load_resume_state(get_args(BASE + ["--resume", old, "--optimizer", "adamw"]))
    adamw = _state_file(tmp_path / "adamw.pth", optimizer="adamw,betas=0.9/0.999,eps=1e-08,wd=0.01")
    assert load_resume_state(get_args(BASE + ["--resume", adamw, "--optimizer", "adamw"]))["epoch"] == 1
    for argv in ([], ["--optimizer", "sgd"], ["--optimizer", "adamw,wd=0.1"]):
        with pytest.raises(ValueError, match=r"\-\-optimizer"):
            load_resume_state(get_args(BASE + ["--resume", adamw] + argv))
        with caplog.at_level(logging.ERROR):
            assert main(BASE + ["--resume", adamw] + argv) == 2
        assert "--optimizer" in caplog.text and "no GPU" not in caplog.text
        caplog.clear()


# ------------------------------------------------------------------------------------------------ header and binding
ARGS = {"uh_adamw_step": 14, "uh_adamw_step_ema": 18, "uh_sgd_step": 11, "uh_sgd_step_ema": 15}


def test_the_four_entry_points_are_in_header_and_binding():
    import unet_amd  # noqa: F401
    from unet_amd._lib import HEADER, LIB, parse_header
    text = open(HEADER).read()
    protos = parse_header()
    for name, count in ARGS.items():
        assert re.search(rf"\bint {name}\(", text), name
        assert name in protos and name in LIB.protos, name
        ret, types = LIB.protos[name]
        assert ret == "int" and len(types) == count and types[-1] == "uh_stream", (name, types)
        assert types[:3] == ["ptr"] * 3
    # beside the RMSprop pair: the same conventions, the state streams and the step counter in between
    assert len(protos["uh_adamw_step"][1]) == len(protos["uh_rmsprop_step"][1]) + 1
    assert len(protos["uh_sgd_step"][1]) == len(protos["uh_rmsprop_step"][1]) - 2
    for rule in ("adamw", "sgd"):
        assert len(protos[f"uh_{rule}_step_ema"][1]) - len(protos[f"uh_{rule}_step"][1]) == 4          # ema, decay, warmup, updates
    LIB.load()                                                        # every symbol of the header resolves in the library


# ------------------------------------------------------------------------------------------------ the restatements meet the bounds
def _adamw(case, **kw):
    x, h = R.inputs(case, "adamw"), R.ADAMW_HYPERS[case.hyper]
    coef = K.coef32(case.norm, case.max_norm)
    ref = R.adamw_reference(x, coef, h, case.steps)
    return x, ref, R.adamw_units(R.adamw_f32(x, coef, h, case.steps, **kw), x, ref)


def _sgd(case, **kw):
    x, h = R.inputs(case, "sgd"), R.SGD_HYPERS[case.hyper]
    coef = K.coef32(case.norm, case.max_norm)
    ref = R.sgd_reference(x, coef, h)
    return x, ref, R.sgd_units(R.sgd_f32(x, coef, h, **kw), x, ref, h)


def _sharp(case):
    return (R.SHARP_M, R.SHARP_V, R.SHARP_P) if case.state == "sharp" else ()


def test_float32_restatements_meet_every_bound_at_half():
    worst = {}
    for case in R.ADAMW_CASES:
        _, _, units = _adamw(case)
        assert not R.adamw_breaks(units, R.K_M / 2, R.K_V / 2, R.K_PA / 2), (case.name, units)
        for k in "mvp":
            worst["adamw " + k] = max(worst.get("adamw " + k, 0.0), units[k])
    for case in R.ADAMW_SHARP:                                      # counted bounds: met whole, not at half
        _, _, units = _adamw(case)
        assert not R.adamw_breaks(units, *_sharp(case)), (case.name, units)
    for case in R.SGD_CASES:
        _, _, units = _sgd(case)
        assert not R.sgd_breaks(units, R.K_BS / 2, R.K_PS / 2), (case.name, units)
        for k in "bp":
            worst["sgd " + k] = max(worst.get("sgd " + k, 0.0), units[k])
    print("the float32 restatements' worst units: " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    # the constants are four times these, rounded up
    for k, const in (("adamw m", R.K_M), ("adamw v", R.K_V), ("adamw p", R.K_PA), ("sgd b", R.K_BS), ("sgd p", R.K_PS)):
        assert const == int(np.ceil(4 * worst[k])), (k, worst[k], const)


@pytest.mark.parametrize("mistake", R.ADAMW_MISTAKES)
def test_each_adamw_mistake_breaks_a_bound(mistake):
    broken = {}
    for case in R.ADAMW_CASES + R.ADAMW_SHARP:
        if case.n > 4099:
            continue
        _, _, units = _adamw(case, mistake=mistake, at=case.n // 2)
        hit = R.adamw_breaks(units, *_sharp(case))
        if hit:
            broken[case.name] = hit
    print(f"{mistake}: breaks {len(broken)} cases, e.g. {list(broken.items())[:3]}")
    assert broken
    if mistake in ("no_bias_correction", "t_not_t_plus_1"):
        assert all(c.name in broken for c in R.ADAMW_SHARP)         # the sharp first step sees both


@pytest.mark.parametrize("mistake", R.SGD_MISTAKES)
def test_each_sgd_mistake_breaks_a_bound(mistake):
    broken = {}
    for case in R.SGD_CASES:
        if case.n > 4099:
            continue
        _, _, units = _sgd(case, mistake=mistake, at=case.n // 2)
        hit = R.sgd_breaks(units)
        if hit:
            broken[case.name] = hit
    print(f"{mistake}: breaks {len(broken)} cases, e.g. {list(broken.items())[:3]}")
    assert broken


def test_one_minus_beta_and_the_raw_second_moment():
    """1.f - b is exact for the float32 betas (Sterbenz), so the double difference of the rounded beta is what the kernel forms;
    and float32(0.999) moves 1 - b2 by 1.29e-5 relative, which is why the raw v' is not held to stock torch but v' / bc2 is."""
    for b in (0.9, 0.999, 0.5):
        assert float(F(1) - F(b)) == 1.0 - float(F(b))
    rel = abs((1.0 - float(F(0.999))) - 0.001) / 0.001
    print(f"1.f - float32(0.999) against 0.001: {rel:.3e} relative")
    assert 1.2e-5 < rel < 1.4e-5
    for t in (0, 1, 9, 999, 99999):                                   # ... and bc2 shifts with it: v' / bc2 stays inside OP_TOL
        bc2_32, bc2_64 = R.bias_corrections(0.0, float(F(0.999)), t)[1], R.bias_corrections(0.0, 0.999, t)[1]
        assert abs(bc2_32 - bc2_64) / bc2_64 <= rel * 1.001
    assert R.bias_corrections(float(F(0.9)), float(F(0.999)), 99999)[0] == 1.0            # b1^t has underflowed


# ------------------------------------------------------------------------------------------------ the reference is stock torch
@pytest.mark.parametrize("name,hyper,state,gscale,max_norm,steps", R.STOCK_ADAMW, ids=[c[0] for c in R.STOCK_ADAMW])
def test_adamw_reference_with_doubles_equals_stock_torch(name, hyper, state, gscale, max_norm, steps):
    x, h = R.stock_inputs("adamw", name, state, gscale), R.ADAMW_HYPERS[hyper]
    stock = R.stock_adamw_step(x, max_norm, h, steps)
    ref = R.adamw_reference(x, R.clip_coef_doubles(x["g"], max_norm), h, steps, rounded=False)
    for k, mag in (("g", np.abs(ref["g"])), ("m", ref["mag_m"]), ("v", ref["mag_v"]), ("p", ref["mag_p"]),
                   ("vhat", ref["mag_v"] / ref["bc2"])):
        assert R.distance(ref[k], stock[k], mag) <= 1e-12, k
    # and the float32 restatement's distance to it, relative to the bounds' magnitudes: inside the project's 2e-5
    coef = K.coef32(K.real_norm32(x["g"]), max_norm)
    d = R.stock_adamw_distance(R.adamw_f32(x, coef, h, steps), stock, R.adamw_reference(x, coef, h, steps))
    print(f"{name}: float32 restatement to stock torch: " + ", ".join(f"{k} {v:.2e}" for k, v in d.items()))
    assert max(d.values()) <= R.OP_TOL


@pytest.mark.parametrize("name,hyper,state,gscale,max_norm,steps", R.STOCK_SGD, ids=[c[0] for c in R.STOCK_SGD])
def test_sgd_reference_with_doubles_equals_stock_torch(name, hyper, state, gscale, max_norm, steps):
    x, h = R.stock_inputs("sgd", name, state, gscale), R.SGD_HYPERS[hyper]
    stock = R.stock_sgd_step(x, max_norm, h)
    ref = R.sgd_reference(x, R.clip_coef_doubles(x["g"], max_norm), h, rounded=False)
    for k, mag in (("g", np.abs(ref["g"])), ("b", ref["mag_b"]), ("p", np.abs(ref["p"]) + h["lr"] * ref["mag_b"])):
        assert R.distance(ref[k], stock[k], mag) <= 1e-12, k
    coef = K.coef32(K.real_norm32(x["g"]), max_norm)
    d = R.stock_sgd_distance(R.sgd_f32(x, coef, h), x, stock, R.sgd_reference(x, coef, h), h)
    print(f"{name}: float32 restatement to stock torch: " + ", ".join(f"{k} {v:.2e}" for k, v in d.items()))
    assert max(d.values()) <= R.OP_TOL
