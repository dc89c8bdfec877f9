"""Benchmark of the RAW -> contour pipeline (seg_main.py on the device, unet_amd.ContourPipeline).  Prints one JSON line.

    python pipeline_bench.py [--batch 8] [--iters 10] [--sizes 2048x1536,512x512]

Per size: RAW -> JSON images/s with UNet(1,3,bilinear=False) inference (bf16, graphed) and without it (the forward
replaced by a three-op stub), the device time of every stage from events, the RAW file read and the JSON write timed
apart, and in the same run the host composition of the reference's stages: numpy window, PIL letterbox, the same
device forward + argmax + post-processing, PIL de-letterbox.  The host contour step is the Python restatement of
OpenCV's tracer (tests/seg_pipeline_ref.py), NOT OpenCV, and is reported separately."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def phantoms(rng, n, H, W):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    out = np.empty((n, H, W), np.uint16)
    for i in range(n):
        img = rng.normal(30, 8, (H, W)).astype(np.float32)
        cx, cy = W * rng.uniform(0.4, 0.6), H * rng.uniform(0.4, 0.6)
        rx, ry = W * rng.uniform(0.25, 0.4), H * rng.uniform(0.25, 0.4)
        body = ((xx - cx) / rx) ** 2 + ((yy - cy) / ry) ** 2 < 1
        img[body] = 1000 + rng.normal(0, 10, int(body.sum()))
        img[((xx - cx) / (rx / 3)) ** 2 + ((yy - cy - ry / 3) / (ry / 4)) ** 2 < 1] += 600
        out[i] = np.clip(img, 0, 65535).astype(np.uint16)
    return out


class Stub(torch.nn.Module):
    def forward(self, x):
        return torch.cat([0.2 - x, 0.15 - (x - 0.2).abs(), x - 0.3], dim=1) * 8.0


def run_size(W, H, B, iters, ww, wl, model):
    import unet_amd
    from unet_amd.utils.mask2polygon import contour_json, write_json
    from unet_amd.utils.raw2png import read_raw
    import seg_pipeline_ref as R
    from PIL import Image
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(W * H)
    raws = phantoms(rng, B, H, W)
    res = {"size": f"{W}x{H}", "batch": B}
    with tempfile.TemporaryDirectory() as td:
        for i in range(B):
            raws[i].astype("<u2").tofile(os.path.join(td, f"s{i}.raw"))
        t0 = time.perf_counter()
        for _ in range(iters):
            batch = np.stack([read_raw(os.path.join(td, f"s{i}.raw"), W, H) for i in range(B)])
        res["raw_read_ms_per_batch"] = (time.perf_counter() - t0) * 1e3 / iters
        for label, m in (("with_inference", model), ("without_inference", Stub().to(dev))):
            pipe = unet_amd.ContourPipeline(m, W, H, ww, wl, batch=B)
            for _ in range(3):
                pipe(batch, [f"s{i}" for i in range(B)])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                js = pipe(batch, [f"s{i}" for i in range(B)])
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / iters
            res[f"{label}_images_per_s"] = B / dt
            res[f"{label}_ms_per_batch"] = dt * 1e3
            if label == "with_inference":
                pipe.events = []
                for _ in range(iters):
                    pipe.run_batch(batch)
                torch.cuda.synchronize()
                st = {}
                for name, e0, e1 in pipe.events:
                    st[name] = st.get(name, 0.0) + e0.elapsed_time(e1) / iters
                pipe.events = None
                res["stage_ms_per_batch"] = st
                res["non_inference_device_ms"] = sum(v for k, v in st.items() if k not in ("forward", "argmax"))
                res["contours_per_image"] = [0 if j is None else len(j["shapes"]) for j in js]
                t0 = time.perf_counter()
                for _ in range(iters):
                    for i, j in enumerate(js):
                        if j is not None:
                            write_json(os.path.join(td, f"s{i}.json"), j)
                res["json_write_ms_per_batch"] = (time.perf_counter() - t0) * 1e3 / iters
                pipe_model = pipe
    # host composition (one pass over the batch; the host stages dominate)
    host = {"window_numpy": 0.0, "letterbox_pil": 0.0, "device_predict": 0.0, "unletterbox_pil": 0.0}
    t = time.perf_counter
    a = t(); wins = [R.window_ref(raws[i], ww, wl) for i in range(B)]; host["window_numpy"] = t() - a
    a = t()
    canv = []
    for w in wins:
        nw, nh, px, py = R.geometry_ref(W, H)
        c = Image.new("L", (512, 512), 0)
        c.paste(Image.fromarray(w, mode="L").resize((nw, nh), Image.LANCZOS), (px, py))
        canv.append(np.asarray(c))
    host["letterbox_pil"] = t() - a
    torch.cuda.synchronize()
    a = t()
    ct = torch.from_numpy(np.stack(canv)).to(dev)
    logits = pipe_model._forward(ct)
    cls = unet_amd.postprocess_mask(unet_amd.ops.argmax_classes(logits).to(torch.uint8)).cpu().numpy()
    host["device_predict"] = t() - a
    a = t()
    greys = []
    nw, nh, px, py = R.geometry_ref(W, H)
    for c in cls:
        g = np.asarray(unet_amd.mask_to_image(c))
        greys.append(np.asarray(Image.fromarray(g, mode="L").crop((px, py, px + nw, py + nh)).resize((W, H), Image.LANCZOS)))
    host["unletterbox_pil"] = t() - a
    a = t()
    for g in greys:
        R.contours_ref(g > 127)
    contour_s = t() - a
    res["host_composition_ms_per_batch"] = {k: v * 1e3 for k, v in host.items()}
    res["host_composition_images_per_s_excluding_contours"] = B / sum(host.values())
    res["host_contours_python_restatement_not_opencv_ms_per_batch"] = contour_s * 1e3
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--sizes", default="2048x1536,512x512")
    ap.add_argument("--ww", type=int, default=400)
    ap.add_argument("--wl", type=int, default=1040)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("pipeline_bench.py needs an MI355X")
    import unet_amd
    torch.manual_seed(0)
    model = unet_amd.UNet(1, 3, bilinear=False).to("cuda:0")
    out = {"metric": "raw_to_json_images_per_s", "device": torch.cuda.get_device_name(0), "results": []}
    for s in args.sizes.split(","):
        W, H = (int(v) for v in s.split("x"))
        out["results"].append(run_size(W, H, args.batch, args.iters, args.ww, args.wl, model))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
