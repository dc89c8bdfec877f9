"""Benchmark of the averaged weights (EMA) kept inside the optimizer pass (csrc/optim.hip).  Prints one JSON line and writes it
to profiles/ema_bench.json.

    python ema_bench.py [--iters 30] [--batch 8] [--size 512] [--steps 20] [--warmup 5] [--rounds 3]
                        [--out profiles/ema_bench.json]

Three things, alternated in one process:
  - device time (events around 10 back-to-back calls, warm-up, median of --iters samples with min / max) of uh_rmsprop_step
    and of uh_rmsprop_step_ema over the parameter count of UNet(1,1,bilinear), the two kernels taking turns sample block by
    sample block (--rounds blocks each).  The plain pass moves 8 fp32 streams, the averaging pass 10: the byte model says
    1.25 x.  The ratio is read against the spread of the plain pass's own repeated timings.  Back to back, part of either
    pass's working set (4 or 5 buffers of 69 MB) is still in the 256 MiB last-level cache when the next call starts, which
    no train step offers the optimizer; "cold" therefore times single calls, each just after a 512 MiB write to another
    buffer, the two kernels taking turns call by call;
  - train-step images/s of UNet(1,1,bilinear) in bf16 at batch 8 with and without ema, the two steppers alternating, --rounds
    windows of --steps steps each after --warmup steps, a device synchronise closing every window;
  - the cost of one TrainStepper.averaged() round trip (swap in, swap out; nothing evaluated inside), host wall time around
    a device synchronise, and the device time of one uh_swap_f32."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def device_samples(fn, iters, warmup=3, inner=10):
    """Milliseconds per call: `iters` samples of `inner` back-to-back calls between two events."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) / inner)
    return ts


def cold_samples(fns, iters, evict, warmup=3):
    """{name: [ms]}: single calls, each behind a write over `evict` (larger than the last-level cache), taking turns."""
    out = {name: [] for name in fns}
    for i in range(warmup + iters):
        for name, fn in fns.items():
            evict.fill_(i & 1)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= warmup:
                out[name].append(e0.elapsed_time(e1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--steps", type=int, default=20, help="train steps per timed window")
    ap.add_argument("--warmup", type=int, default=5, help="untimed steps per stepper before the first window")
    ap.add_argument("--rounds", type=int, default=3, help="plain / ema blocks and windows, alternated")
    ap.add_argument("--ema", default="0.999,warmup=10")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ema_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ema_bench.py needs an MI355X")
    import unet_amd
    from unet_amd._lib import LIB
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B, H, W = args.batch, args.size, args.size
    cfg = unet_amd.EmaConfig.parse(args.ema)
    out = {"metric": "ema_bench", "device": torch.cuda.get_device_name(0), "iters": args.iters, "ema": cfg.spec()}
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(0)

    # ---- (a) the two optimizer passes alone, over the flat length of the full model
    n = sum((p.numel() + 3) // 4 * 4 for p in unet_amd.UNet(1, 1, bilinear=True).parameters())
    p, gr, sq, buf, ema = (torch.randn(n, generator=g).to(dev) * s for s in (1.0, 1e-3, 0.0, 0.0, 1.0))
    norm = torch.tensor([0.5], dtype=torch.float32, device=dev)
    updates = torch.zeros(1, dtype=torch.int32, device=dev)
    hyper = (1.0, 1e-5, 0.99, 1e-8, 1e-8, 0.999)

    def plain():
        LIB.call("uh_rmsprop_step", p.data_ptr(), gr.data_ptr(), sq.data_ptr(), buf.data_ptr(), n, norm.data_ptr(), *hyper, st)

    def averaging():
        LIB.call("uh_rmsprop_step_ema", p.data_ptr(), gr.data_ptr(), sq.data_ptr(), buf.data_ptr(), ema.data_ptr(), n,
                 norm.data_ptr(), *hyper, float(cfg.decay), int(cfg.warmup), updates.data_ptr(), st)

    def swap():
        LIB.call("uh_swap_f32", p.data_ptr(), ema.data_ptr(), n, st)

    samples = {"plain": [], "ema": []}
    blocks = {"plain": [], "ema": []}
    for _ in range(args.rounds):
        for name, fn in (("plain", plain), ("ema", averaging)):
            ts = device_samples(fn, args.iters)
            samples[name] += ts
            blocks[name].append(statistics.median(ts))
    kern = {"elements": n, "bytes_plain": 8 * 4 * n, "bytes_ema": 10 * 4 * n,
            "rmsprop_step_ms": spread(samples["plain"]), "rmsprop_step_ema_ms": spread(samples["ema"]),
            "rmsprop_step_block_medians_ms": blocks["plain"], "rmsprop_step_ema_block_medians_ms": blocks["ema"],
            "swap_f32_ms": spread(device_samples(swap, args.iters))}
    kern["ema_over_plain"] = kern["rmsprop_step_ema_ms"]["median"] / kern["rmsprop_step_ms"]["median"]
    kern["byte_model_ratio"] = 1.25
    kern["plain_spread"] = (kern["rmsprop_step_ms"]["max"] - kern["rmsprop_step_ms"]["min"]) / kern["rmsprop_step_ms"]["median"]
    kern["plain_GBps"] = kern["bytes_plain"] / kern["rmsprop_step_ms"]["median"] / 1e6
    kern["ema_GBps"] = kern["bytes_ema"] / kern["rmsprop_step_ema_ms"]["median"] / 1e6
    evict = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
    cold = cold_samples({"plain": plain, "ema": averaging}, args.iters, evict)
    kern["cold"] = {"evict_bytes": evict.numel(), "rmsprop_step_ms": spread(cold["plain"]), "rmsprop_step_ema_ms": spread(cold["ema"])}
    kern["cold"]["ema_over_plain"] = kern["cold"]["rmsprop_step_ema_ms"]["median"] / kern["cold"]["rmsprop_step_ms"]["median"]
    kern["cold"]["plain_spread"] = (kern["cold"]["rmsprop_step_ms"]["max"] - kern["cold"]["rmsprop_step_ms"]["min"]) \
        / kern["cold"]["rmsprop_step_ms"]["median"]
    out["kernel"] = kern
    del p, gr, sq, buf, ema, evict

    # ---- (b) the train step without and with the average, alternating in one process
    images = torch.rand(B, 1, H, W, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
    labels = torch.randint(0, 3, (B, H, W), generator=g).to(dev)
    steppers = {}
    for name, spec in (("off", None), ("on", cfg)):
        torch.manual_seed(0)
        model = unet_amd.UNet(1, 1, bilinear=True).to(memory_format=torch.channels_last).to(dev)
        steppers[name] = unet_amd.TrainStepper(model, amp=True, ema=spec)

    def window(stepper, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            stepper.step(images, labels)
        torch.cuda.synchronize()
        return B * steps / (time.perf_counter() - t0)

    for s in steppers.values():
        window(s, args.warmup)
    rates = {"off": [], "on": []}
    for _ in range(args.rounds):
        for name in ("off", "on"):
            rates[name].append(window(steppers[name], args.steps))
    step = {"model": "UNet(1,1,bilinear=True)", "dtype": "bf16", "batch": B, "size": f"{H}x{W}",
            "steps_per_window": args.steps, "rounds": args.rounds,
            "off_img_s": spread(rates["off"]), "off_img_s_all": [round(r, 1) for r in rates["off"]],
            "on_img_s": spread(rates["on"]), "on_img_s_all": [round(r, 1) for r in rates["on"]]}
    step["on_over_off"] = step["on_img_s"]["median"] / step["off_img_s"]["median"]
    step["off_spread"] = (step["off_img_s"]["max"] - step["off_img_s"]["min"]) / step["off_img_s"]["median"]
    step["ms_per_step_added"] = 1e3 * B * (1.0 / step["on_img_s"]["median"] - 1.0 / step["off_img_s"]["median"])
    out["train_step"] = step

    # ---- (c) one averaged() round trip on the stepper that keeps an average
    on = steppers["on"]
    trips = []
    for i in range(args.iters + 3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with on.averaged():
            pass
        torch.cuda.synchronize()
        if i >= 3:
            trips.append(1e3 * (time.perf_counter() - t0))
    out["averaged_round_trip_ms"] = spread(trips)
    for s in steppers.values():
        s.close()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
