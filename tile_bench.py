"""Benchmark of tiled prediction (csrc/tiling.hip).  Prints one JSON line and writes it to profiles/tile_bench.json.

    python tile_bench.py [--iters 20] [--rounds 5] [--per-size 16] [--legs kernels,mixed,large] [--out profiles/tile_bench.json]

Everything runs in one process on warmed shapes, in --rounds rounds that alternate the candidates; reported is the median
(min - max) of the rounds.
  kernels  device events around uh_tile_gather and uh_tile_merge for two 2048 x 2048 images, tiles of 512 with overlap 128
           (50 tiles), one image channel, NC = 3, fp32 logits (what the network's head returns), beside a torch device copy that
           moves the same number of bytes and beside the same result composed from torch ops: slices and a cat for the gather;
           per tile a softmax times the weight plane, added into the image by slicing, then an argmax, for the merge;
  mixed    predict_bench.py's mixed set (--per-size images of each of 512x512, 384x512, 999x1000, 700x300, shuffled) through
           BatchPredictor(batch=8, batch_invariant=True) with tile off and with tile="512", UNet_S(1,3) and UNet(1,3), bf16:
           images/s from a host clock around whole calls (they end with the masks on the host);
  large    one 2048 x 2048 and one 4096 x 4096 image through UNet(1,3), whole against tile="512": seconds per image from the
           same host clock, and torch.cuda.max_memory_allocated of a fresh predictor's first (un-graphed) call."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

SIZES = [(512, 512), (384, 512), (999, 1000), (700, 300)]          # (H, W): predict_bench.py's mixed set


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def device_ms(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def alternate(fns, iters, rounds):
    """{name: spread of per-call device ms} over `rounds` rounds that run every candidate in turn."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            ts[k].append(device_ms(fn, iters))
    return {k: spread(v) for k, v in ts.items()}


def host_rounds(runs, rounds, warm=2):
    """{name: [seconds per call]} from a host clock around calls that end in a synchronise, the candidates alternating."""
    for fn in runs.values():
        for _ in range(warm):
            fn()
    ts = {k: [] for k in runs}
    for _ in range(rounds):
        for k, fn in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts[k].append(time.perf_counter() - t0)
    return ts


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
    x = torch.from_numpy(img.astype(np.float32) / 255.0)[None, None].to(dev)
    with torch.no_grad():
        model.outc.conv.bias.sub_(model(x).float().mean(dim=(0, 2, 3)))


# ------------------------------------------------------------------ the kernels' torch-op compositions
def torch_gather(x_nhwc, th, tw, oy, ox):
    return torch.cat([x_nhwc[b:b + 1, y:y + th, x:x + tw] for b in range(x_nhwc.shape[0]) for y in oy for x in ox])


def torch_merge(logits_nhwc, B, H, W, th, tw, oy, ox, wplane):
    """logits [B ny nx, th, tw, NC] -> uint8 classes: per tile softmax x weight added into the image by slicing, then argmax
    (the normalisation by the summed weights does not change the argmax)."""
    acc = torch.zeros(B, H, W, logits_nhwc.shape[-1], dtype=torch.float32, device=logits_nhwc.device)
    n = 0
    for b in range(B):
        for y in oy:
            for x in ox:
                acc[b, y:y + th, x:x + tw] += torch.softmax(logits_nhwc[n].float(), -1) * wplane
                n += 1
    return acc.argmax(-1).to(torch.uint8)


def leg_kernels(args, dev):
    from unet_amd import ops
    from unet_amd.utils.tiling import TileConfig, axis_weights, tile_grid
    cfg = TileConfig(512, 128)
    B, H, W, C, NC = 2, 2048, 2048, 1, 3
    ny, nx, th, tw, oy, ox = tile_grid(H, W, cfg)
    N = B * ny * nx
    g = torch.Generator(device="cpu").manual_seed(0)
    x = torch.rand(B, H, W, C, generator=g).to(dev).permute(0, 3, 1, 2)
    xn = x.permute(0, 2, 3, 1)
    logits = (2.0 * torch.randn(N, th, tw, NC, generator=g)).to(dev)
    ln = logits.permute(0, 3, 1, 2)
    wplane = (torch.tensor(axis_weights(th, cfg), dtype=torch.float32)[:, None] *
              torch.tensor(axis_weights(tw, cfg), dtype=torch.float32)[None, :]).to(dev)[..., None]
    gather_bytes = 2 * 4 * C * N * th * tw                         # every tile element read once and written once
    merge_bytes = 4 * NC * N * th * tw + B * H * W                 # every tile logit read once, one class byte per pixel
    src_g = torch.empty(gather_bytes // 2, dtype=torch.uint8, device=dev)
    dst_g = torch.empty_like(src_g)
    src_m = torch.empty(merge_bytes // 2, dtype=torch.uint8, device=dev)
    dst_m = torch.empty_like(src_m)
    t = alternate({"gather": lambda: ops.tile_gather(x, cfg),
                   "gather_torch": lambda: torch_gather(xn, th, tw, oy, ox),
                   "gather_copy": lambda: dst_g.copy_(src_g),
                   "merge": lambda: ops.tile_merge(ln, cfg, (H, W)),
                   "merge_torch": lambda: torch_merge(logits, B, H, W, th, tw, oy, ox, wplane),
                   "merge_copy": lambda: dst_m.copy_(src_m)}, args.iters, args.rounds)
    same_g = bool(torch.equal(ops.tile_gather(x, cfg).permute(0, 2, 3, 1), torch_gather(xn, th, tw, oy, ox)))
    same_m = float((ops.tile_merge(ln, cfg, (H, W)).classes == torch_merge(logits, B, H, W, th, tw, oy, ox, wplane)).float().mean())
    gbs = lambda nbytes, ms: nbytes / (ms * 1e-3) / 1e9
    return {"shape": {"B": B, "H": H, "W": W, "C": C, "NC": NC, "tile": cfg.spec, "tiles": N, "logits": "fp32"},
            "gather_ms": t["gather"], "gather_bytes": gather_bytes, "gather_GBps": gbs(gather_bytes, t["gather"]["median"]),
            "gather_copy_ms": t["gather_copy"], "gather_copy_GBps": gbs(gather_bytes, t["gather_copy"]["median"]),
            "gather_torch_ops_ms": t["gather_torch"], "gather_torch_over_kernel": t["gather_torch"]["median"] / t["gather"]["median"],
            "gather_faster_beyond_spread": bool(t["gather"]["max"] < t["gather_torch"]["min"]),
            "gather_equal_to_torch_ops": same_g,
            "merge_ms": t["merge"], "merge_bytes": merge_bytes, "merge_GBps": gbs(merge_bytes, t["merge"]["median"]),
            "merge_copy_ms": t["merge_copy"], "merge_copy_GBps": gbs(merge_bytes, t["merge_copy"]["median"]),
            "merge_torch_ops_ms": t["merge_torch"], "merge_torch_over_kernel": t["merge_torch"]["median"] / t["merge"]["median"],
            "merge_faster_beyond_spread": bool(t["merge"]["max"] < t["merge_torch"]["min"]),
            "classes_equal_to_torch_ops_fraction": same_m}


def leg_mixed(args, dev):
    import unet_amd
    rows = []
    for name in args.models.split(","):
        torch.manual_seed(0)
        model = getattr(unet_amd, name)(1, 3, bilinear=False).to(dev).eval()
        rng = np.random.default_rng(1)
        one = [phantom(rng, 512, 512) for _ in range(8)]              # (drawn first, as predict_bench.py does)
        mixed = [phantom(rng, H, W) for (H, W) in SIZES for _ in range(args.per_size)]
        mixed = [mixed[i] for i in rng.permutation(len(mixed))]
        balance_head(model, one[0], dev)
        off = unet_amd.BatchPredictor(model, batch=8, batch_invariant=True)
        on = unet_amd.BatchPredictor(model, batch=8, batch_invariant=True, tile="512")
        ts = host_rounds({"off": lambda: off(mixed), "tile_512": lambda: on(mixed)}, args.rounds)
        a, b = off(mixed), on(mixed)
        agree = float(np.mean([(u == v).mean() for u, v in zip(a, b)]))
        r = {k: spread([len(mixed) / t for t in v]) for k, v in ts.items()}
        rows.append({"model": f"{name}(1,3)", "workload": f"mixed_{args.per_size}_each_of_4_sizes", "images": len(mixed),
                     "images_per_s": r, "tile_over_off": r["tile_512"]["median"] / r["off"]["median"],
                     "gain_beyond_spread": bool(r["tile_512"]["min"] > r["off"]["max"]),
                     "graph_replays": {"off": off.graph_replays, "tile_512": on.graph_replays},
                     "graphs_kept": {"off": len(off._graphs), "tile_512": len(on._graphs)},
                     "mask_agreement_with_untiled": agree})
        del off, on, model
        torch.cuda.empty_cache()
    return rows


def leg_large(args, dev):
    import unet_amd
    torch.manual_seed(0)
    model = unet_amd.UNet(1, 3, bilinear=False).to(dev).eval()
    rng = np.random.default_rng(3)
    balance_head(model, phantom(rng, 512, 512), dev)
    rows = []
    for side in (2048, 4096):
        img = phantom(rng, side, side)
        row = {"model": "UNet(1,3)", "size": f"{side}x{side}"}
        masks = {}
        for key, tile in (("whole", None), ("tile_512", "512")):
            try:
                # memory first, on a fresh predictor: its first call runs un-graphed (a replayed graph's activations live in
                # the graph's pool, which max_memory_allocated does not see)
                p = unet_amd.BatchPredictor(model, batch=8, batch_invariant=True, tile=tile)
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats()
                p([img])
                torch.cuda.synchronize()
                peak = torch.cuda.max_memory_allocated() / 2 ** 20
                ts = host_rounds({key: lambda: masks.__setitem__(key, p([img])[0])}, args.rounds)[key]
                row[key] = {"seconds": spread(ts), "first_call_max_memory_allocated_MiB": peak, "graph_replays": p.graph_replays}
                del p
            except RuntimeError as e:                                  # (an image that does not fit is a result too)
                row[key] = {"error": str(e)[:300]}
            torch.cuda.empty_cache()
        if "whole" in masks and "tile_512" in masks:
            row["mask_agreement_with_untiled"] = float((masks["whole"] == masks["tile_512"]).mean())
            row["whole_over_tile_seconds"] = row["whole"]["seconds"]["median"] / row["tile_512"]["seconds"]["median"]
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--per-size", type=int, default=16)
    ap.add_argument("--models", default="UNet_S,UNet")
    ap.add_argument("--legs", default="kernels,mixed,large")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tile_bench.json"))
    args = ap.parse_args()
    if args.rounds < 5:
        sys.exit("tile_bench.py reports the spread of at least 5 alternated rounds")
    if not torch.cuda.is_available():
        sys.exit("tile_bench.py needs an MI355X")
    dev = torch.device("cuda:0")
    out = {"metric": "tile_bench", "device": torch.cuda.get_device_name(0), "iters": args.iters, "rounds": args.rounds, "amp": "bf16"}
    legs = args.legs.split(",")
    if "kernels" in legs:
        out["kernels"] = leg_kernels(args, dev)
    if "mixed" in legs:
        out["mixed"] = leg_mixed(args, dev)
    if "large" in legs:
        out["large"] = leg_large(args, dev)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
