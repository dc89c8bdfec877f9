"""Benchmark of the three update rules of the fused optimizer pass (csrc/optim.hip): RMSprop, AdamW and SGD.  Prints one JSON line
and writes it to profiles/optim_bench.json.

    python optim_bench.py [--iters 30] [--batch 8] [--size 512] [--steps 20] [--warmup 5] [--rounds 3]
                          [--out profiles/optim_bench.json]

Two things, alternated in one process (the protocol of ema_bench.py):
  - device time of uh_rmsprop_step, uh_adamw_step and uh_sgd_step, each with its _ema form, over the parameter count of
    UNet(1,1,bilinear): "cold" times single calls, each just behind a 512 MiB write to another buffer (larger than the last-level
    cache: what a train step offers the optimizer), the six kernels taking turns call by call; "back to back" times 10 calls
    between two events, the kernels taking turns sample block by sample block (--rounds blocks each).  The byte model: RMSprop and
    AdamW move 8 fp32 streams (p, g and two states, read and written), SGD 6, the _ema forms 2 more each.  Nobody had measured
    the new kernels, so the same run records the ratio of each cold median to RMSprop's AND RMSprop's own max / median spread: an
    AdamW ratio above 1 + that spread, or an SGD ratio above 6/8 + that spread, wants an explanation (DESIGN.md section 3
    "Optimizers"); the per-thread double power of the bias corrections is the first suspect;
  - train-step images/s of UNet(1,1,bilinear) in bf16 at batch 8 under each rule, the three steppers alternating, --rounds windows
    of --steps steps each after --warmup steps, a device synchronise closing every window.  Reported, gated on nothing."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from ema_bench import cold_samples, device_samples, spread  # noqa: E402

STREAMS = {"rmsprop": 8, "adamw": 8, "sgd": 6}          # fp32 streams of the plain pass; the _ema forms move 2 more


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--steps", type=int, default=20, help="train steps per timed window")
    ap.add_argument("--warmup", type=int, default=5, help="untimed steps per stepper before the first window")
    ap.add_argument("--rounds", type=int, default=3, help="blocks and windows per rule, alternated")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("optim_bench.py needs an MI355X")
    import unet_amd
    from unet_amd._lib import LIB
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B, H, W = args.batch, args.size, args.size
    ema = unet_amd.EmaConfig()
    specs = {"rmsprop": None, "adamw": unet_amd.OptimConfig("adamw"), "sgd": unet_amd.OptimConfig("sgd")}
    out = {"metric": "optim_bench", "device": torch.cuda.get_device_name(0), "iters": args.iters,
           "specs": {k: (v.spec() if v is not None else "default (rmsprop)") for k, v in specs.items()}, "ema": ema.spec()}
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(0)

    # ---- (a) the six passes alone, over the flat length of the full model
    n = sum((p.numel() + 3) // 4 * 4 for p in unet_amd.UNet(1, 1, bilinear=True).parameters())
    p, gr, s1, s2, avg = (torch.randn(n, generator=g).to(dev) * s for s in (1.0, 1e-3, 0.0, 0.0, 1.0))
    norm = torch.tensor([0.5], dtype=torch.float32, device=dev)
    updates = torch.zeros(1, dtype=torch.int32, device=dev)
    steps = torch.full((1,), 1000, dtype=torch.int32, device=dev)
    ptr = [t.data_ptr() for t in (p, gr, s1, s2)]
    tail = (float(ema.decay), int(ema.warmup), updates.data_ptr())
    rms = (norm.data_ptr(), 1.0, 1e-5, 0.99, 1e-8, 1e-8, 0.999)
    adw = (norm.data_ptr(), 1.0, 1e-5, 0.9, 0.999, 1e-8, 0.01, steps.data_ptr())
    sgd = (norm.data_ptr(), 1.0, 1e-5, 3e-5, 0.99, 1)
    fns = {
        "rmsprop": lambda: LIB.call("uh_rmsprop_step", *ptr, n, *rms, st),
        "rmsprop_ema": lambda: LIB.call("uh_rmsprop_step_ema", *ptr, avg.data_ptr(), n, *rms, *tail, st),
        "adamw": lambda: LIB.call("uh_adamw_step", *ptr, n, *adw, st),
        "adamw_ema": lambda: LIB.call("uh_adamw_step_ema", *ptr, avg.data_ptr(), n, *adw, *tail, st),
        "sgd": lambda: LIB.call("uh_sgd_step", *ptr[:3], n, *sgd, st),
        "sgd_ema": lambda: LIB.call("uh_sgd_step_ema", *ptr[:3], avg.data_ptr(), n, *sgd, *tail, st),
    }
    nbytes = {name: (STREAMS[name.split("_")[0]] + (2 if name.endswith("_ema") else 0)) * 4 * n for name in fns}
    samples = {name: [] for name in fns}
    blocks = {name: [] for name in fns}
    for _ in range(args.rounds):
        for name, fn in fns.items():
            ts = device_samples(fn, args.iters)
            samples[name] += ts
            blocks[name].append(statistics.median(ts))
    evict = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
    cold = cold_samples(fns, args.iters, evict)

    def table(ts):
        t = {name: dict(spread(v), bytes=nbytes[name], byte_model_over_rmsprop=nbytes[name] / nbytes["rmsprop"]) for name, v in ts.items()}
        base = t["rmsprop"]
        for name, row in t.items():
            row["over_rmsprop"] = row["median"] / base["median"]
            row["GBps"] = row["bytes"] / row["median"] / 1e6
        return {"ms": t, "rmsprop_max_over_median": base["max"] / base["median"],
                "rmsprop_spread": (base["max"] - base["min"]) / base["median"]}

    kern = {"elements": n, "cold": dict(table(cold), evict_bytes=evict.numel()),
            "back_to_back": dict(table(samples), block_medians_ms=blocks)}
    c = kern["cold"]
    room = c["rmsprop_max_over_median"] - 1.0
    c["adamw_within_rmsprop_spread"] = c["ms"]["adamw"]["over_rmsprop"] <= 1.0 + room
    c["sgd_within_byte_model_plus_spread"] = c["ms"]["sgd"]["over_rmsprop"] <= 6 / 8 + room
    out["kernel"] = kern
    del p, gr, s1, s2, avg, evict

    # ---- (b) the train step under each rule, the steppers alternating in one process
    images = torch.rand(B, 1, H, W, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
    labels = torch.randint(0, 3, (B, H, W), generator=g).to(dev)
    steppers = {}
    for name, spec in specs.items():
        torch.manual_seed(0)
        model = unet_amd.UNet(1, 1, bilinear=True).to(memory_format=torch.channels_last).to(dev)
        steppers[name] = unet_amd.TrainStepper(model, amp=True, optimizer=spec)

    def window(stepper, count):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(count):
            stepper.step(images, labels)
        torch.cuda.synchronize()
        return B * count / (time.perf_counter() - t0)

    for s in steppers.values():
        window(s, args.warmup)
    rates = {name: [] for name in steppers}
    for _ in range(args.rounds):
        for name in steppers:
            rates[name].append(window(steppers[name], args.steps))
    step = {"model": "UNet(1,1,bilinear=True)", "dtype": "bf16", "batch": B, "size": f"{H}x{W}",
            "steps_per_window": args.steps, "rounds": args.rounds}
    for name in steppers:
        step[name + "_img_s"] = dict(spread(rates[name]), all=[round(r, 1) for r in rates[name]])
    for name in ("adamw", "sgd"):
        step[name + "_over_rmsprop"] = step[name + "_img_s"]["median"] / step["rmsprop_img_s"]["median"]
    step["rmsprop_spread"] = (step["rmsprop_img_s"]["max"] - step["rmsprop_img_s"]["min"]) / step["rmsprop_img_s"]["median"]
    out["train_step"] = step
    for s in steppers.values():
        s.close()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
