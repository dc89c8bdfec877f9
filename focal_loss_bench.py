"""Benchmark of the focal + Tversky loss (csrc/focal_loss.hip).  Prints one JSON line and writes it to
profiles/focal_loss_bench.json.

    python focal_loss_bench.py [--iters 10] [--passes 3] [--batch 8] [--size 512] [--steps 20] [--warmup 5] [--rounds 3]
                               [--out profiles/focal_loss_bench.json]

  - device time (events around 10 back-to-back calls, warm-up, median with min / max of --passes x --iters samples) of
      uh_focal_tversky_sums  beside  uh_ce_dice_sums / uh_bce_dice_sums   (each: one pass over the logits + its column sums)
      uh_focal_tversky_grad  beside  uh_ce_dice_grad / uh_bce_dice_grad
    at 8 x 512^2 x 3 (softmax head) and 8 x 512^2 x 1 (one-channel head), gamma = 2 and gamma = 0.5 (the exp2 / log2 path), the
    old and the new launches alternated in one process (--passes times old, new, old, new, ...).  The new kernels move the
    bytes of the pair they replace; `new_over_old` is the ratio of the medians;
  - train-step images/s of UNet(1,3,bilinear) in bf16 at batch 8 with the option off and on ("focal=2,tversky=0.3/0.7"), one
    process, the two steppers alternating, --rounds windows of --steps steps each after --warmup steps, a device synchronise
    closing every window.  The difference is read against the spread of the option-off windows."""
import argparse
import ctypes
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10, help="samples per launch and pass")
    ap.add_argument("--passes", type=int, default=3, help="alternations of the old and the new launches")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--steps", type=int, default=20, help="train steps per timed window")
    ap.add_argument("--warmup", type=int, default=5, help="untimed steps per stepper before the first window")
    ap.add_argument("--rounds", type=int, default=3, help="off / on windows, alternated")
    ap.add_argument("--loss", default="focal=2,tversky=0.3/0.7")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "focal_loss_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("focal_loss_bench.py needs an MI355X")
    import unet_amd
    from unet_amd._lib import LIB
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B, H, W = args.batch, args.size, args.size
    n = B * H * W
    out = {"metric": "focal_loss_device_ms", "device": torch.cuda.get_device_name(0), "iters": args.iters, "passes": args.passes,
           "batch": B, "size": f"{H}x{W}"}
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(0)
    labels = torch.randint(0, 3, (B, H, W), generator=g).to(dev)
    ws = torch.empty(LIB.query("uh_loss_ws_bytes", n), dtype=torch.uint8, device=dev)

    # ---- the kernels beside the pair they replace
    kern = {}
    for name, ncls in (("softmax_8x3", 3), ("one_channel_8x1", 1)):
        C = 2 if ncls == 1 else ncls
        div = 2 if ncls == 1 else 1
        logits = (torch.randn((B, H, W) if ncls == 1 else (B, H, W, ncls), generator=g) * 3).to(dev)
        dl = torch.empty_like(logits)
        w = (ctypes.c_float * C)(*([1.0] * C))
        cls = (ctypes.c_int * (C - 1))(*range(1, C))
        s_new = torch.empty(2 + 3 * C, dtype=torch.float32, device=dev)
        s_old = torch.empty(4 if ncls == 1 else 1 + 3 * ncls, dtype=torch.float32, device=dev)
        lp, mp, dp = logits.data_ptr(), labels.data_ptr(), dl.data_ptr()

        def old_sums():
            if ncls == 1:
                LIB.call("uh_bce_dice_sums", lp, mp, 2, None, n, s_old.data_ptr(), ws.data_ptr(), ws.numel(), st)
            else:
                LIB.call("uh_ce_dice_sums", lp, mp, n, ncls, s_old.data_ptr(), ws.data_ptr(), ws.numel(), st)

        def old_grad():
            if ncls == 1:
                LIB.call("uh_bce_dice_grad", lp, mp, 2, None, n, s_old.data_ptr(), float(n), 1.0, 1.0, None, dp, st)
            else:
                LIB.call("uh_ce_dice_grad", lp, mp, n, ncls, s_old.data_ptr(), float(n), 1.0, 1.0, None, dp, st)

        def new_sums(gamma):
            return lambda: LIB.call("uh_focal_tversky_sums", lp, mp, div, n, ncls, w, gamma, s_new.data_ptr(), ws.data_ptr(),
                                    ws.numel(), st)

        def new_grad(gamma):
            return lambda: LIB.call("uh_focal_tversky_grad", lp, mp, div, n, ncls, w, gamma, 0.3, 0.7, cls, C - 1, s_new.data_ptr(),
                                    None, dp, st)

        launches = {"old_sums": old_sums, "new_sums_gamma2": new_sums(2.0), "new_sums_gamma0.5": new_sums(0.5),
                    "old_grad": old_grad, "new_grad_gamma2": new_grad(2.0), "new_grad_gamma0.5": new_grad(0.5)}
        old_sums()
        new_sums(2.0)()                                               # the gradient launches read sums
        samples = {k: [] for k in launches}
        for _ in range(args.passes):
            for k, fn in launches.items():
                samples[k] += device_samples(fn, args.iters)
        res = {k + "_ms": spread(v) for k, v in samples.items()}
        res["bytes_read_sums"] = n * (4 * ncls + 8)
        res["bytes_moved_grad"] = n * (8 * ncls + 8)
        for what in ("sums", "grad"):
            for gm in ("gamma2", "gamma0.5"):
                res[f"{what}_{gm}_new_over_old"] = res[f"new_{what}_{gm}_ms"]["median"] / res[f"old_{what}_ms"]["median"]
        kern[name] = res
    out["kernel"] = kern

    # ---- the train step with the option off and on, alternating in one process
    images = torch.rand(B, 1, H, W, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
    steppers = {}
    for name, loss in (("off", None), ("on", args.loss)):
        torch.manual_seed(0)
        model = unet_amd.UNet(1, 3, bilinear=True).to(memory_format=torch.channels_last).to(dev)
        steppers[name] = unet_amd.TrainStepper(model, amp=True, loss=loss)

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
    step = {"model": "UNet(1,3,bilinear=True)", "dtype": "bf16", "batch": B, "size": f"{H}x{W}", "loss": args.loss,
            "steps_per_window": args.steps, "rounds": args.rounds,
            "off_img_s": spread(rates["off"]), "off_img_s_all": [round(r, 1) for r in rates["off"]],
            "on_img_s": spread(rates["on"]), "on_img_s_all": [round(r, 1) for r in rates["on"]]}
    step["on_over_off"] = step["on_img_s"]["median"] / step["off_img_s"]["median"]
    step["off_spread"] = (step["off_img_s"]["max"] - step["off_img_s"]["min"]) / step["off_img_s"]["median"]
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
