"""`python -m unet_amd.train --optimizer ...` as child processes on the MI355X, on the synthetic tiny dataset and the shape of
tests/test_gpu_train_resume.py: under AdamW and under SGD, with --ema, a run interrupted after its first epoch and resumed from
train_state.pth ends bit for bit where the uninterrupted run ends; a differing --optimizer on resume ends with status 2; and
without the option the state file holds exactly the optimizer keys it held before the option existed."""
import os
import subprocess
import sys

import pytest
import torch

from conftest import ROOT
from test_gpu_train_resume import COMMON, _files, _load, _png_tree, _run_cli

pytestmark = pytest.mark.gpu

OPTIONS = ["--ema", "0.9,warmup=0", "-l", "1e-3"]
SPECS = {"adamw": "adamw", "sgd": "sgd,momentum=0.9"}


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    top = tmp_path_factory.mktemp("optim_cli")
    _png_tree(str(top / "data"), 8, 4, 96, seed=3)
    return top


@pytest.fixture(scope="module", params=sorted(SPECS))
def runs(request, data):
    """A: two epochs in one go.  B: one epoch, then --resume up to the second.  Same data, same options."""
    rule = request.param
    base = COMMON + OPTIONS + ["--optimizer", SPECS[rule], "--data-root", str(data / "data")]
    a, b = data / f"{rule}_a", data / f"{rule}_b"
    log_a = _run_cli(a, base + ["-e", "2", "--save-state", "--checkpoint-dir", str(a / "ck")]).stderr
    _run_cli(b, base + ["-e", "1", "--save-state", "--checkpoint-dir", str(b / "ck")])
    log_b2 = _run_cli(b, base + ["-e", "2", "--resume", str(b / "ck" / "train_state.pth"), "--checkpoint-dir", str(b / "ck")]).stderr
    return {"rule": rule, "base": base, "a": a, "b": b, "log_a": log_a, "log_b2": log_b2}


def test_resumed_run_ends_where_the_uninterrupted_run_ends(runs):
    for name in ("model_epoch2.pth", "model_epoch2_ema.pth"):
        want, got = _load(runs["a"] / name), _load(runs["b"] / name)
        assert list(want) == list(got)
        for k in want:
            assert torch.equal(want[k], got[k]), (runs["rule"], name, k)
    first, second = _load(runs["b"] / "model_epoch1.pth"), _load(runs["b"] / "model_epoch2.pth")
    assert any(not torch.equal(first[k], second[k]) for k in first)
    assert "Resumed after epoch 1 (global step 8" in runs["log_b2"] and "Epoch 1/2" not in runs["log_b2"]


def test_log_names_the_canonical_spec_and_the_state_holds_the_rule(runs):
    from unet_amd import OptimConfig
    canonical = OptimConfig.parse(SPECS[runs["rule"]]).spec()
    for log in (runs["log_a"], runs["log_b2"]):
        assert log.count(f"Optimizer: {canonical}") == 1
    state = _load(runs["a"] / "ck" / "train_state.pth")
    assert state["args"]["optimizer"] == canonical and state["epoch"] == 2 and state["global_step"] == 16
    opt = state["optimizer"]
    assert opt["kind"] == runs["rule"] and opt["ema_updates"] == 16 and opt["ema"] is not None
    if runs["rule"] == "adamw":
        assert opt["step"] == 16 and set(opt) >= {"exp_avg", "exp_avg_sq"} and "momentum_buffer" not in opt
        assert opt["exp_avg"].abs().sum() > 0 and opt["exp_avg_sq"].min() >= 0
    else:
        assert "step" not in opt and "square_avg" not in opt and opt["momentum_buffer"].abs().sum() > 0
        assert opt["hyper"]["momentum"] == 0.9 and opt["hyper"]["nesterov"] is True


def test_resume_with_another_optimizer_ends_with_status_2(runs):
    env = dict(os.environ, PYTHONPATH=ROOT)
    other = "sgd" if runs["rule"] == "adamw" else "adamw"
    base = [a for a in runs["base"] if a != SPECS[runs["rule"]] and a != "--optimizer"]
    for extra in (["--optimizer", other],):          # (the other refusals: tests/test_optim_rules_cpu.py, without a child process)
        r = subprocess.run([sys.executable, "-m", "unet_amd.train"] + base + extra +
                           ["-e", "2", "--resume", str(runs["b"] / "ck" / "train_state.pth")],
                           capture_output=True, text=True, timeout=300, cwd=str(runs["b"]), env=env)
        assert r.returncode == 2 and "--optimizer" in r.stderr, r.stderr[-2000:]


def test_without_the_option_the_state_file_is_what_it_was(data):
    c = data / "c"
    log = _run_cli(c, COMMON + ["--data-root", str(data / "data"), "-e", "1", "--save-state", "--checkpoint-dir", str(c / "ck")]).stderr
    assert "Optimizer:" not in log
    assert _files(c) == ["ck/train_state.pth", "model_epoch1.pth"]
    state = _load(c / "ck" / "train_state.pth")
    assert set(state["optimizer"]) == {"square_avg", "momentum_buffer", "ema", "ema_updates", "layout", "total", "hyper"}
    assert set(state["optimizer"]["hyper"]) == {"lr", "alpha", "eps", "weight_decay", "momentum", "gradient_clipping", "ema_decay",
                                                "ema_warmup"}
    assert state["args"]["optimizer"] is None
