"""Benchmark of the contour metrics (csrc/contour_metrics.hip).  Prints one JSON line and writes it to
profiles/contour_metrics_bench.json.

    python metrics_bench.py [--iters 20] [--reps 5] [--val-batches 6] [--out profiles/contour_metrics_bench.json]

Masks: a filled body per image (the phantoms of pipeline_bench.py as class maps), 8 x 512^2 and 2 x 1024^2, class 2.
  - device time (events, median of --iters, with min / max) of uh_contour_metrics, of uh_edt_sq_u8 alone, of
    uh_mask_border_u8 alone and of the post-processing stage on the same batch;
  - the same batches through the scipy restatement on the host (tests/contour_metrics_ref.py), 16 threads;
  - evaluate() over a synthetic validation set: the loop as it was before the `metrics` keyword (restated below) against
    evaluate(metrics=None), alternating, --reps wall-clock repetitions each, and evaluate() with an accumulator."""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def body_masks(rng, n, H, W):
    """Class maps {0,1,2}: a filled body (class 2) on background 1, and a second map whose body is a little off."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    out = np.ones((2, n, H, W), np.uint8)
    for i in range(n):
        cx, cy = W * rng.uniform(0.4, 0.6), H * rng.uniform(0.4, 0.6)
        rx, ry = W * rng.uniform(0.25, 0.4), H * rng.uniform(0.25, 0.4)
        out[0, i][((xx - cx) / rx) ** 2 + ((yy - cy) / ry) ** 2 < 1] = 2
        cx, cy, rx, ry = cx + rng.uniform(-6, 6), cy + rng.uniform(-6, 6), rx * rng.uniform(0.95, 1.05), ry * rng.uniform(0.95, 1.05)
        out[1, i][((xx - cx) / rx) ** 2 + ((yy - cy) / ry) ** 2 < 1] = 2
        out[1, i][int(H * 0.05):int(H * 0.05) + 3, int(W * 0.9):int(W * 0.9) + 3] = 2          # a far-away speck
    return out[0], out[1]


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def device_ms(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return spread(ts)


def parent_evaluate(net, batches, device, amp):
    """evaluate(postprocess=True) as it was before the `metrics` keyword (multi-class branch, no PNG dumps)."""
    from unet_amd import ops
    from unet_amd.utils.dice_score import dice_coeff
    from unet_amd.utils.post_process import postprocess_mask
    with torch.inference_mode():
        net.eval()
        n = 0
        dice_score = torch.zeros((), dtype=torch.float32, device=device)
        dice_post = torch.zeros((), dtype=torch.float32, device=device)
        min_dice = torch.full((), 10.0, dtype=torch.float32, device=device)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
            for batch in batches:
                n += 1
                image = batch["image"].to(device=device, dtype=torch.float32, memory_format=torch.channels_last)
                mask_true = batch["mask"].to(device=device, dtype=torch.float32)
                idx = ops.argmax_classes(net(image))
                true_c = (mask_true == 2).float()
                d = dice_coeff((idx == 2).float(), true_c, reduce_batch_first=False)
                processed = postprocess_mask(idx.to(torch.uint8))
                dice_post += dice_coeff((processed == 2).float(), true_c, reduce_batch_first=False)
                dice_score += d
                min_dice = torch.minimum(min_dice, d.float())
        net.train()
        return dice_score / max(n, 1), dice_post / max(n, 1), min_dice


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    [float(v) for v in out]                      # the caller's host read of the three figures
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--val-batches", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contour_metrics_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("metrics_bench.py needs an MI355X")
    import contour_metrics_ref as R
    import unet_amd
    from unet_amd import ops
    dev = torch.device("cuda:0")
    out = {"metric": "contour_metrics_device_ms", "device": torch.cuda.get_device_name(0), "iters": args.iters, "sizes": []}
    for B, H, W in ((8, 512, 512), (2, 1024, 1024)):
        P, T = body_masks(np.random.default_rng(H + B), B, H, W)
        p, t = torch.from_numpy(P).to(dev), torch.from_numpy(T).to(dev)
        border = ops.mask_border(t, 2)
        res = {"batch": B, "size": f"{H}x{W}",
               "contour_metrics_ms": device_ms(lambda: ops.contour_metrics(p, t, 2, 2), args.iters),
               "edt_sq_ms": device_ms(lambda: ops.edt_sq(border), args.iters),
               "mask_border_ms": device_ms(lambda: ops.mask_border(t, 2), args.iters),
               "postprocess_ms": device_ms(lambda: unet_amd.postprocess_mask(p), args.iters)}
        with ThreadPoolExecutor(max_workers=16) as pool:
            host = []
            for _ in range(3):
                t0 = time.perf_counter()
                rows = list(pool.map(lambda i: R.image_metrics(P[i] == 2, T[i] == 2), range(B)))
                host.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        for i in range(B):
            R.image_metrics(P[i] == 2, T[i] == 2)
        res["host_scipy_one_thread_ms"] = (time.perf_counter() - t0) * 1e3
        res["host_scipy_16_threads_ms"] = spread(host)
        res["host_over_device"] = res["host_scipy_16_threads_ms"]["median"] / res["contour_metrics_ms"]["median"]
        got = unet_amd.utils.contour_metrics.decode_records(ops.contour_metrics(p, t, 2, 2))
        res["hd_equal_to_host"] = bool(all(float(got["hd"][i]) == rows[i]["hd"] for i in range(B)))
        res["mean_hd95"] = float(got["hd95"].mean())
        out["sizes"].append(res)
    # evaluate(): a synthetic validation set, the loop before the keyword against metrics=None, alternating
    torch.manual_seed(0)
    model = unet_amd.UNet_S(1, 3, bilinear=False).to(memory_format=torch.channels_last).to(dev)
    images, masks = unet_amd.ellipse_batch(8 * args.val_batches, 512, seed=4)
    batches = [{"image": images[i:i + 8].to(dev), "mask": masks[i:i + 8].to(dev)} for i in range(0, images.shape[0], 8)]
    for _ in range(2):
        parent_evaluate(model, batches, dev, True)
        unet_amd.evaluate(model, batches, dev, True)
        unet_amd.evaluate(model, batches, dev, True, metrics=unet_amd.ContourMetrics())
    parent, new, on = [], [], []
    for _ in range(args.reps):
        parent.append(wall_ms(lambda: parent_evaluate(model, batches, dev, True)))
        new.append(wall_ms(lambda: unet_amd.evaluate(model, batches, dev, True)))

    def with_acc():
        acc = unet_amd.ContourMetrics()
        r = unet_amd.evaluate(model, batches, dev, True, metrics=acc)
        acc.result()
        return r
    for _ in range(args.reps):
        on.append(wall_ms(with_acc))
    ev = {"model": "UNet_S(1,3)", "batches": len(batches), "batch": 8, "size": "512x512", "amp": True,
          "parent_loop_ms": spread(parent), "metrics_none_ms": spread(new), "with_accumulator_ms": spread(on)}
    ev["metrics_none_median_inside_parent_spread"] = bool(ev["parent_loop_ms"]["min"] <= ev["metrics_none_ms"]["median"]
                                                          <= ev["parent_loop_ms"]["max"])
    ev["accumulator_cost_ms_per_batch"] = (ev["with_accumulator_ms"]["median"] - ev["metrics_none_ms"]["median"]) / len(batches)
    out["evaluate"] = ev
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
