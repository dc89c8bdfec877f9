"""Benchmark of the surface loss (csrc/surface_loss.hip).  Prints one JSON line and writes it to
profiles/surface_loss_bench.json.

    python surface_loss_bench.py [--iters 30] [--batch 8] [--size 512] [--steps 20] [--warmup 5] [--rounds 3]
                                 [--out profiles/surface_loss_bench.json]

  - device time (events around 10 back-to-back calls, warm-up, median of --iters samples with min / max) at 8 x 1 x 512^2
    (binary head, K = 1) and 8 x 3 x 512^2 (softmax head, K = 1 and K = 2) of
      the map build    uh_surface_dist_map: border + distance transform + fp32 map (the public helper), and
      loss + gradient  uh_surface_loss_sums (border + distance transform + value) followed by uh_surface_loss_grad,
    on blob labels (a few filled ellipses per image, the shape of the dataset's contours);
  - train-step images/s of UNet(1,1,bilinear) in bf16 at batch 8 with the term off and on (weight 0.1), one process, the two
    steppers alternating, --rounds windows of --steps steps each after --warmup steps, a device synchronise closing every
    window.  The cost of the term is read against the spread of the option-off windows."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def device_ms(fn, iters, warmup=3, inner=10):
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
    return spread(ts)


def blob_labels(rng, B, H, W):
    """int64 [B,H,W]: class 2 on three filled ellipses per image, a random mix of 0 and 1 elsewhere."""
    yy, xx = np.indices((H, W))
    out = rng.integers(0, 2, (B, H, W)).astype(np.int64)
    for b in range(B):
        for _ in range(3):
            cy, cx = rng.uniform(0.2, 0.8) * H, rng.uniform(0.2, 0.8) * W
            ry, rx = rng.uniform(0.05, 0.25) * H, rng.uniform(0.05, 0.25) * W
            out[b][((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0] = 2
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--steps", type=int, default=20, help="train steps per timed window")
    ap.add_argument("--warmup", type=int, default=5, help="untimed steps per stepper before the first window")
    ap.add_argument("--rounds", type=int, default=3, help="off / on windows, alternated")
    ap.add_argument("--weight", type=float, default=0.1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surface_loss_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("surface_loss_bench.py needs an MI355X")
    import unet_amd
    from unet_amd._lib import LIB
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B, H, W = args.batch, args.size, args.size
    out = {"metric": "surface_loss_device_ms", "device": torch.cuda.get_device_name(0), "iters": args.iters,
           "batch": B, "size": f"{H}x{W}"}
    rng = np.random.default_rng(0)
    labels = torch.from_numpy(blob_labels(rng, B, H, W)).to(dev)
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(0)

    # ---- the kernels alone
    kern = {}
    for name, ncls, cls in (("binary_8x1", 1, (1,)), ("softmax_8x3_k1", 3, (2,)), ("softmax_8x3_k2", 3, (1, 2))):
        K, div = len(cls), 2 if ncls == 1 else 1
        shape = (B, H, W) if ncls == 1 else (B, H, W, ncls)
        logits = (torch.randn(shape, generator=g) * 3).to(dev)
        arr = (ctypes.c_int * K)(*cls)
        ws = torch.empty(LIB.query("uh_surface_loss_ws_bytes", B, H, W, K), dtype=torch.uint8, device=dev)
        phi = torch.empty(K, B, H, W, dtype=torch.float32, device=dev)
        val = torch.empty(2, dtype=torch.float32, device=dev)
        dl = torch.empty_like(logits)
        n_mean = float(B * H * W)

        def build():
            LIB.call("uh_surface_dist_map", labels.data_ptr(), div, arr, K, phi.data_ptr(), B, H, W, ws.data_ptr(), ws.numel(), st)

        def loss_grad():
            LIB.call("uh_surface_loss_sums", logits.data_ptr(), labels.data_ptr(), div, arr, K, ncls, B, H, W, n_mean, 1.0,
                     val.data_ptr(), ws.data_ptr(), ws.numel(), st)
            LIB.call("uh_surface_loss_grad", logits.data_ptr(), labels.data_ptr(), div, arr, K, ncls, B, H, W, n_mean, 1.0, None,
                     dl.data_ptr(), 0, ws.data_ptr(), ws.numel(), st)

        def grad_only():
            LIB.call("uh_surface_loss_grad", logits.data_ptr(), labels.data_ptr(), div, arr, K, ncls, B, H, W, n_mean, 1.0, None,
                     dl.data_ptr(), 0, ws.data_ptr(), ws.numel(), st)

        kern[name] = {"ncls": ncls, "classes": list(cls), "distance_maps": K * B, "workspace_bytes": ws.numel(),
                      "map_build_ms": device_ms(build, args.iters), "loss_plus_grad_ms": device_ms(loss_grad, args.iters),
                      "grad_alone_ms": device_ms(grad_only, args.iters)}
    out["kernel"] = kern

    # ---- the train step with the term off and on, alternating in one process
    images = torch.rand(B, 1, H, W, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
    steppers = {}
    for name, w in (("off", 0.0), ("on", args.weight)):
        torch.manual_seed(0)
        model = unet_amd.UNet(1, 1, bilinear=True).to(memory_format=torch.channels_last).to(dev)
        steppers[name] = unet_amd.TrainStepper(model, amp=True, surface_weight=w)

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
    step = {"model": "UNet(1,1,bilinear=True)", "dtype": "bf16", "batch": B, "size": f"{H}x{W}", "weight": args.weight,
            "steps_per_window": args.steps, "rounds": args.rounds,
            "off_img_s": spread(rates["off"]), "off_img_s_all": [round(r, 1) for r in rates["off"]],
            "on_img_s": spread(rates["on"]), "on_img_s_all": [round(r, 1) for r in rates["on"]]}
    step["on_over_off"] = step["on_img_s"]["median"] / step["off_img_s"]["median"]
    step["off_spread"] = (step["off_img_s"]["max"] - step["off_img_s"]["min"]) / step["off_img_s"]["median"]
    step["ms_per_step_added"] = 1e3 * B * (1.0 / step["on_img_s"]["median"] - 1.0 / step["off_img_s"]["median"])
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
