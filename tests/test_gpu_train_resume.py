"""`python -m unet_amd.train --save-state / --resume / --ema` as child processes on the MI355X: a run interrupted after its first
epoch and resumed from train_state.pth ends bit for bit where the uninterrupted run ends -- live weights, averaged weights
and the log of the second epoch -- and a run without the new options leaves none of the new files behind."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import ROOT

pytestmark = pytest.mark.gpu

COMMON = ["--model", "UNet_T", "-b", "4", "-s", "0.5", "--seed", "1", "--workers", "4"]
OPTIONS = ["--augment", "--elastic", "grid=16,sigma=1", "--ema", "0.9,warmup=0"]


def _png_tree(root, n_train, n_val, size, seed):
    """imgs/{train,val}, masks/{train,val}: ellipse phantoms as 8-bit PNGs, masks coded 0 / 128 / 255."""
    from unet_amd import ellipse_batch
    imgs, masks = ellipse_batch(n_train + n_val, size, seed=seed)
    grey = np.array([0, 128, 255], np.uint8)
    for i in range(n_train + n_val):
        split = "train" if i < n_train else "val"
        for d in ("imgs", "masks"):
            os.makedirs(os.path.join(root, d, split), exist_ok=True)
        Image.fromarray((imgs[i, 0].numpy() * 255).astype(np.uint8)).save(os.path.join(root, "imgs", split, f"p{i:03d}.png"))
        Image.fromarray(grey[masks[i].numpy()]).save(os.path.join(root, "masks", split, f"p{i:03d}_mask.png"))


def _run_cli(cwd, args, timeout=300):
    os.makedirs(cwd, exist_ok=True)
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "unet_amd.train"] + args, capture_output=True, text=True, timeout=timeout,
                       cwd=str(cwd), env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    return r


def _files(top):
    return sorted(os.path.relpath(os.path.join(d, f), top) for d, _, fs in os.walk(top) for f in fs)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """A: two epochs in one go.  B: one epoch, then --resume up to the second.  Same data, same options."""
    top = tmp_path_factory.mktemp("resume")
    data = top / "data"
    _png_tree(str(data), 8, 4, 96, seed=3)
    base = COMMON + OPTIONS + ["--data-root", str(data)]
    a, b = top / "a", top / "b"
    log_a = _run_cli(a, base + ["-e", "2", "--save-state", "--checkpoint-dir", str(a / "ck")]).stderr
    log_b1 = _run_cli(b, base + ["-e", "1", "--save-state", "--checkpoint-dir", str(b / "ck")]).stderr
    log_b2 = _run_cli(b, base + ["-e", "2", "--resume", str(b / "ck" / "train_state.pth"), "--checkpoint-dir", str(b / "ck")]).stderr
    return {"top": top, "data": data, "a": a, "b": b, "log_a": log_a, "log_b1": log_b1, "log_b2": log_b2}


def _load(path):
    return torch.load(path, map_location="cpu", weights_only=True)


def test_resumed_run_ends_where_the_uninterrupted_run_ends(runs):
    for name in ("model_epoch2.pth", "model_epoch2_ema.pth"):
        want, got = _load(runs["a"] / name), _load(runs["b"] / name)
        assert list(want) == list(got)
        for k in want:
            assert torch.equal(want[k], got[k]), (name, k)
    # the interrupted run's first epoch is the uninterrupted run's first epoch
    first = _load(runs["b"] / "model_epoch1.pth")
    assert any(not torch.equal(first[k], _load(runs["b"] / "model_epoch2.pth")[k]) for k in first)
    assert "Training state loaded from" in runs["log_b2"] and "Resumed after epoch 1 (global step 8" in runs["log_b2"]
    assert "Epoch 1/2" not in runs["log_b2"]


def test_averaged_model_loads_like_any_checkpoint_and_differs_from_the_live_one(runs):
    import unet_amd
    live, avg = _load(runs["a"] / "model_epoch2.pth"), _load(runs["a"] / "model_epoch2_ema.pth")
    model = unet_amd.UNet_T(1, 3)
    assert unet_amd.load_checkpoint(model, str(runs["a"] / "model_epoch2_ema.pth")) is None
    for k, v in model.state_dict().items():
        assert torch.equal(v, avg[k]), k
    assert list(live) == list(avg)
    weights = [k for k in live if k.endswith(".weight")]
    assert weights and all(not torch.equal(live[k], avg[k]) for k in weights)
    for k in live:                                                   # BatchNorm statistics are the live ones, not averaged
        if "running_" in k or "num_batches_tracked" in k:
            assert torch.equal(live[k], avg[k]), k


def _epoch2(log):
    """The deterministic part of the second epoch's log: its evaluation line and loss / Dice / lr of its epoch line."""
    lines = log.splitlines()
    at = max(i for i, l in enumerate(lines) if "Epoch 1/2" in l or "Resumed after epoch 1" in l)
    dice = [l for l in lines[at:] if "Validation Dice score (EMA):" in l]
    epoch = [re.search(r"Epoch 2/2: loss \(total\) \S+, Dice \(EMA\) .*?, lr \S+,", l) for l in lines[at:] if "Epoch 2/2: loss" in l]
    assert len(dice) == 1 and len(epoch) == 1 and epoch[0] is not None, log[-3000:]
    return dice[0], epoch[0].group(0)


def test_second_epoch_logs_match(runs):
    assert _epoch2(runs["log_a"]) == _epoch2(runs["log_b2"])
    assert runs["log_a"].count("Validation Dice score (EMA):") == 2                # one evaluation per cadence point, not two
    assert runs["log_a"].count("Validation Dice score") == 2


def test_state_file_holds_what_a_resume_needs(runs):
    assert _files(runs["a"] / "ck") == ["train_state.pth"]                         # no checkpoint is due at 2 epochs; no .tmp stays
    state = _load(runs["a"] / "ck" / "train_state.pth")
    assert state["epoch"] == 2 and state["global_step"] == 16 and state["loader_seed"] == 1 and state["augment_seed"] == 1
    assert state["args"]["ema"] == "0.9,warmup=0" and state["args"]["classes"] == 3 and state["args"]["model"] == "UNet_T"
    assert state["optimizer"]["ema_updates"] == 16 and state["optimizer"]["ema"] is not None
    live = _load(runs["a"] / "model_epoch2.pth")
    for k in live:
        assert torch.equal(state["model"][k], live[k]), k


def test_resume_refuses_another_head_with_status_2(runs):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "unet_amd.train"] + COMMON + OPTIONS +
                       ["--data-root", str(runs["data"]), "-e", "2", "-c", "2", "--resume", str(runs["b"] / "ck" / "train_state.pth")],
                       capture_output=True, text=True, timeout=300, cwd=str(runs["top"]), env=env)
    assert r.returncode == 2 and "--classes" in r.stderr


def test_without_the_options_no_new_file_appears(runs):
    c = runs["top"] / "c"
    _run_cli(c, COMMON + ["--data-root", str(runs["data"]), "-e", "1", "--checkpoint-dir", str(c / "ck")])
    files = _files(c)
    assert files == ["model_epoch1.pth"], files
    assert not any("train_state" in f or "_ema" in f for f in files)
