"""Benchmark of folder prediction (predict.py on the device).  Prints one JSON line.

    python predict_bench.py [--reps 5] [--per-size 16] [--cli-images 64]

For UNet_S(1,3) and UNet(1,3) (bf16, transposed-conv upscaling), on synthetic phantoms held in memory:
  (a) the per-image loop a user of the package writes without BatchPredictor:
      mask_to_image(postprocess_mask(predict_img(model, img, device))) for every image;
  (b) unet_amd.BatchPredictor(model, batch=8) on the same list;
  (c) unet_amd.BatchPredictor(model, batch=8, batch_invariant=True): every batch one launch under the pinned plan;
on two workloads: 8 x 512x512 (one size, one batch) and a shuffled mixed set (512x512, 512x384, 1000x999, 300x700,
`--per-size` of each).  The legs run in this process on the same images, alternating, `--reps` times after a warm-up pass
over every shape; a leg's time is a host clock around work that ends in a device synchronise (all legs end with their
results on the host).  Reported: images/s from the median repetition, the min-max spread, and the ratios (b)/(a), (c)/(b).
Then the device time of every stage of one 8 x 512x512 batch from events on the stream (both predictors), and the command line end to
end on a temporary folder (`python -m unet_amd.predict`, decode and PNG encode included; process start-up and model load
are inside the figure and are also reported apart)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

SIZES = [(512, 512), (384, 512), (999, 1000), (700, 300)]          # (H, W)


def phantom(rng, H, W):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    img = rng.normal(20, 6, (H, W)).astype(np.float32)
    cx, cy = W * rng.uniform(0.4, 0.6), H * rng.uniform(0.4, 0.6)
    rx, ry = W * rng.uniform(0.3, 0.4), H * rng.uniform(0.3, 0.4)
    body = ((xx - cx) / rx) ** 2 + ((yy - cy) / ry) ** 2 < 1
    img[body] = 110 + rng.normal(0, 8, int(body.sum()))
    img[((xx - cx) / (rx / 3)) ** 2 + ((yy - cy - ry / 3) / (ry / 4)) ** 2 < 1] += 90
    return np.clip(img, 0, 255).astype(np.uint8)


def balance_head(model, img, dev):
    """A fresh network puts one class on top everywhere and post-processing then has nothing to do; centring the head's
    logits on one phantom makes the class maps (and so the post-processing load) non-trivial."""
    x = torch.from_numpy(img.astype(np.float32) / 255.0)[None, None].to(dev)
    with torch.no_grad():
        model.outc.conv.bias.sub_(model(x).float().mean(dim=(0, 2, 3)))


def per_image_loop(unet_amd, model, images, dev):
    return [np.asarray(unet_amd.mask_to_image(unet_amd.postprocess_mask(unet_amd.predict_img(model, im, dev)))) for im in images]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def rates(n, times):
    r = sorted(n / t for t in times)
    return {"images_per_s": statistics.median(r), "min": r[0], "max": r[-1], "reps": len(r)}


def run_model(name, reps, per_size):
    import unet_amd
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = getattr(unet_amd, name)(1, 3, bilinear=False).to(dev).eval()
    rng = np.random.default_rng(1)
    one = [phantom(rng, 512, 512) for _ in range(8)]
    mixed = [phantom(rng, H, W) for (H, W) in SIZES for _ in range(per_size)]
    mixed = [mixed[i] for i in rng.permutation(len(mixed))]
    balance_head(model, one[0], dev)
    res = {"model": f"{name}(1,3)", "rows": []}
    for label, images in (("8x512x512", one), (f"mixed_{per_size}_each_of_4_sizes", mixed)):
        predictor = unet_amd.BatchPredictor(model, batch=8)
        invariant = unet_amd.BatchPredictor(model, batch=8, batch_invariant=True)
        ref = per_image_loop(unet_amd, model, images, dev)            # warm-up of every shape, all legs
        predictor(images)
        got = predictor(images)                                        # second pass: graphs captured
        invariant(images)
        got_c = invariant(images)
        same = all(np.array_equal(a, b) for a, b in zip(ref, got))
        same_c = all(np.array_equal(a, b) for a, b in zip(ref, got_c))
        ta, tb, tc = [], [], []
        for _ in range(reps):                                          # alternating
            ta.append(timed(lambda: per_image_loop(unet_amd, model, images, dev))[0])
            tb.append(timed(lambda: predictor(images))[0])
            tc.append(timed(lambda: invariant(images))[0])
        a, b, c = rates(len(images), ta), rates(len(images), tb), rates(len(images), tc)
        row = {"workload": label, "images": len(images), "per_image_loop": a, "batch_predictor": b,
               "batch_predictor_invariant": c, "ratio_b_over_a": b["images_per_s"] / a["images_per_s"],
               "ratio_c_over_b": c["images_per_s"] / b["images_per_s"], "outputs_equal": same, "outputs_equal_invariant": same_c,
               "foreground_share": float(np.mean([(g == 255).mean() for g in got])), "graph_replays": predictor.graph_replays,
               "graph_replays_invariant": invariant.graph_replays,
               "launch_lengths": {f"{h}x{w}": v for (h, w), v in predictor.planner.lengths.items()},
               "launch_lengths_invariant": {f"{h}x{w}": v for (h, w), v in invariant.planner.lengths.items()}}
        if label == "8x512x512":
            for key, pr in (("stage_ms_per_8_images", predictor), ("stage_ms_per_8_images_invariant", invariant)):
                pr.events = []
                for _ in range(reps):
                    pr(images)
                torch.cuda.synchronize()
                st = {}
                for stage, e0, e1 in pr.events:
                    st[stage] = st.get(stage, 0.0) + e0.elapsed_time(e1) / reps
                pr.events = None
                row[key] = st
        res["rows"].append(row)
    return res


def run_cli(n_images, reps):
    import unet_amd
    from PIL import Image
    torch.manual_seed(0)
    out = {"images": n_images, "model": "UNet_S(1,3)", "batch_size": 8, "workers": 8}
    rng = np.random.default_rng(2)
    with tempfile.TemporaryDirectory() as td:
        src, dst = os.path.join(td, "in"), os.path.join(td, "out")
        os.makedirs(src)
        for i in range(n_images):
            H, W = SIZES[i % len(SIZES)]
            Image.fromarray(phantom(rng, H, W)).save(os.path.join(src, f"p{i:04d}.png"))
        model = unet_amd.UNet_S(1, 3, bilinear=False)
        wpath = unet_amd.save_checkpoint(model, os.path.join(td, "w.pth"), mask_values=[0, 128, 255])
        one = os.path.join(td, "one")
        os.makedirs(one)
        Image.fromarray(phantom(rng, 64, 64)).save(os.path.join(one, "tiny.png"))
        env = dict(os.environ, PYTHONPATH=ROOT)
        base = [sys.executable, "-m", "unet_amd.predict", "-m", wpath, "--arch", "UNet_S"]

        def call(args):
            t0 = time.perf_counter()
            r = subprocess.run(base + args, capture_output=True, text=True, env=env, cwd=td, timeout=600)
            if r.returncode != 0:
                raise RuntimeError("predict CLI failed:\n" + r.stderr[-2000:])
            return time.perf_counter() - t0

        call(["-i", one, "-o", dst])                                   # warm-up of the file cache and code objects
        full = [call(["-i", src, "-o", dst]) for _ in range(reps)]
        startup = [call(["-i", one, "-o", dst]) for _ in range(reps)]  # start-up, model load and one 64x64 image
        out["written"] = len([f for f in os.listdir(dst) if f.startswith("p")])
    out["end_to_end"] = rates(n_images, full)
    out["startup_s"] = statistics.median(startup)
    out["images_per_s_beyond_startup"] = n_images / max(statistics.median(full) - statistics.median(startup), 1e-9)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--per-size", type=int, default=16)
    ap.add_argument("--cli-images", type=int, default=64, help="0: leave the command-line leg out")
    ap.add_argument("--models", default="UNet_S,UNet")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("predict_bench.py needs an MI355X")
    out = {"metric": "predict_images_per_s", "device": torch.cuda.get_device_name(0), "amp": "bf16", "postprocess": True,
           "results": [run_model(m, args.reps, args.per_size) for m in args.models.split(",")]}
    if args.cli_images > 0:
        out["cli"] = run_cli(args.cli_images, max(2, args.reps // 2))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
