"""bench.py --gpus N must start N ranks itself when no torch.distributed environment is present (missing #1).
Without a GPU the ranks stop at the "needs an MI355X" check -- after the launcher has given each of them its RANK /
WORLD_SIZE, which is what is checked here; the full 2-rank flow runs in tests/test_gpu_bench_ranks.py on the GPU box."""
import os
import subprocess
import sys

from conftest import ROOT


def _run(args, env_extra=None, timeout=300):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True,
                          timeout=timeout)


def test_gpus_flag_spawns_that_many_ranks():
    import torch
    if torch.cuda.is_available():
        import pytest
        pytest.skip("CPU-side check of the launcher (the GPU flow has its own test)")
    r = _run(["--gpus", "2", "--backend", "gloo", "--share-gpu", "--steps", "1", "--warmup", "0"])
    assert r.returncode != 0
    assert "rank 0/2" in r.stderr and "rank 1/2" in r.stderr, r.stderr[-2000:]


def test_gpus_must_match_world_size():
    r = _run(["--gpus", "4"], {"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and "WORLD_SIZE=2" in r.stderr


def test_more_ranks_than_devices_is_refused():
    import torch
    if torch.cuda.device_count() >= 2:
        import pytest
        pytest.skip("machine has several GPUs")
    r = _run(["--gpus", "2"])
    assert r.returncode != 0 and "--share-gpu" in r.stderr


def test_plain_run_leaves_every_extra_leg_to_full(monkeypatch):
    """`bench.py --steps K --warmup W` times the steps and nothing else; --full turns every leg on again and the --no-* options
    still switch single legs off there."""
    import bench
    legs = ("no_strong_leg", "no_kernel_profile", "no_b4_leg", "no_sustained", "no_inference", "no_cpu_baseline")
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert a.steps == 7 and a.warmup == 2 and not a.full and a.dump_outputs is None
    assert all(getattr(a, k) for k in legs)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--no-sustained", "--dump-outputs", "out"])
    a = bench.parse()
    assert a.full and a.no_sustained and a.dump_outputs == "out"
    assert not any(getattr(a, k) for k in legs if k != "no_sustained")


def test_dump_outputs_writes_float32_and_samples_large_tensors_the_same_way(tmp_path):
    import numpy as np
    import torch
    import bench
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Conv2d(1, 4, 3), torch.nn.BatchNorm2d(4))
    big = torch.randn(9 << 20)                                         # 36 MiB of float32: above the 32 MiB share of logits
    terms = {"loss": torch.tensor(1.5, dtype=torch.bfloat16), "logits": big, "grad_norm": torch.tensor(0.25)}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), terms, model)
    got = {f: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert set(got) == {"loss.npy", "logits.npy", "grad_norm.npy", "parameters.npy", "bn_running_stats.npy"}
    assert all(v.dtype == np.float32 for v in got.values())
    assert float(got["loss.npy"]) == 1.5 and got["parameters.npy"].size == sum(p.numel() for p in model.parameters())
    assert got["logits.npy"].size == (32 << 20) // 4 and np.isin(got["logits.npy"][:100], big.numpy()).all()
    assert np.array_equal(got["logits.npy"], np.load(tmp_path / "b" / "logits.npy"))     # a fixed sample
