"""Benchmark of test-time augmentation (csrc/tta.hip).  Prints one JSON line and writes it to profiles/tta_bench.json.

    python tta_bench.py [--iters 20] [--rounds 5] [--images 64] [--out profiles/tta_bench.json]

Everything runs in one process on warmed shapes, timed with device events (the end-to-end part: a host clock around work that
ends in a synchronise), in --rounds rounds that alternate the candidates:
  - kernel time of uh_tta_views and uh_tta_merge at B = 8, 512 x 512, one image channel, NC = 3, bf16 logits, modes d4 and
    flips, as bytes moved over time -- (1 + V) 4 C H W B for the views, V NC 2 H W B + H W B for the merge -- beside a torch
    device copy that moves the same number of bytes, timed in the same rounds;
  - the merge against the same result composed from torch ops on the same tensors: per view a softmax, an inverse flip or
    transpose and an add, then an argmax;
  - BatchPredictor images/s at 512 x 512, UNet(1, 3), batch 8, with tta off, flips and d4, and the same launches with the two
    kernels replaced by their torch-op compositions; rate_off / (V rate_tta) is the cost of TTA beyond its V forwards."""
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


def pose(a, v):
    """View v of an NHWC batch with torch ops."""
    dims = [d for d, on in ((1, v & 2), (2, v & 1)) if on]
    if dims:
        a = a.flip(dims)
    return a.transpose(1, 2) if v & 4 else a


def unpose(a, v):
    """A view's NHWC tensor back on the source grid."""
    if v & 4:
        a = a.transpose(1, 2)
    dims = [d for d, on in ((1, v & 2), (2, v & 1)) if on]
    return a.flip(dims) if dims else a


def torch_views(x_nhwc, views):
    v0 = torch.cat([pose(x_nhwc, v).contiguous() for v in views if v < 4])
    v1 = [pose(x_nhwc, v).contiguous() for v in views if v >= 4]
    return v0, torch.cat(v1) if v1 else None


def torch_merge(l0, l1, views, B):
    """logits NHWC per shape -> uint8 classes: softmax, inverse pose and add per view, then argmax."""
    acc = None
    i0 = i1 = 0
    for v in views:
        if v & 4:
            l, i1 = l1[i1 * B:(i1 + 1) * B], i1 + 1
        else:
            l, i0 = l0[i0 * B:(i0 + 1) * B], i0 + 1
        p = unpose(torch.softmax(l.float(), -1), v)
        acc = p.contiguous() if acc is None else acc.add_(p)
    return acc.argmax(-1).to(torch.uint8)


def torch_launch(p, arrays, views):
    """BatchPredictor._launch under test-time augmentation with the two kernels replaced by their torch-op compositions."""
    from unet_amd import ops
    H, W = arrays[0].shape
    B = len(arrays)
    img = p._upload(arrays, H, W)
    x = torch.empty(B, 1, H, W, dtype=torch.float32, device=p.device, memory_format=torch.channels_last)
    ops.predict_prepare_u8(img, x, p._flags)
    v0, v1 = torch_views(x.permute(0, 2, 3, 1), views)
    if v1 is not None and H == W:
        n0 = v0.shape[0]
        logits = p._forward_cut(torch.cat([v0, v1]).permute(0, 3, 1, 2), (H, W), p._members[0]).permute(0, 2, 3, 1)
        l0, l1 = logits[:n0], logits[n0:]
    else:
        l0 = p._forward_cut(v0.permute(0, 3, 1, 2), (H, W), p._members[0]).permute(0, 2, 3, 1)
        l1 = p._forward_cut(v1.permute(0, 3, 1, 2), (W, H), p._members[0]).permute(0, 2, 3, 1) if v1 is not None else None
    return p._deliver(torch_merge(l0, l1, views, B), True)


def phantoms(n, H, W, seed=0):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    out = []
    for _ in range(n):
        img = rng.normal(20, 6, (H, W)).astype(np.float32)
        cx, cy, rx, ry = W * rng.uniform(0.4, 0.6), H * rng.uniform(0.4, 0.6), W * rng.uniform(0.3, 0.4), H * rng.uniform(0.3, 0.4)
        body = ((xx - cx) / rx) ** 2 + ((yy - cy) / ry) ** 2 < 1
        img[body] += 100
        out.append(np.clip(img, 0, 255).astype(np.uint8))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tta_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tta_bench.py needs an MI355X")
    import unet_amd
    from unet_amd import ops
    from unet_amd.utils.tta import tta_view_list
    dev = torch.device("cuda:0")
    B, H, W, C, NC = 8, 512, 512, 1, 3
    out = {"metric": "tta_device_ms", "device": torch.cuda.get_device_name(0), "iters": args.iters, "rounds": args.rounds,
           "shape": {"B": B, "H": H, "W": W, "C": C, "NC": NC, "logits": "bf16"}, "kernels": {}}
    g = torch.Generator(device="cpu").manual_seed(0)
    x = torch.rand(B, H, W, C, generator=g).to(dev).permute(0, 3, 1, 2)
    for mode in ("d4", "flips"):
        views = tta_view_list(mode)
        V = len(views)
        k0 = sum(v < 4 for v in views)
        logits = (2.0 * torch.randn(V * B, H, W, NC, generator=g)).to(torch.bfloat16).to(dev)
        l0, l1 = logits[:k0 * B].permute(0, 3, 1, 2), (logits[k0 * B:].permute(0, 3, 1, 2) if V > k0 else None)
        views_bytes = (1 + V) * 4 * C * H * W * B
        merge_bytes = V * NC * 2 * H * W * B + H * W * B
        src_v = torch.empty(views_bytes // 2, dtype=torch.uint8, device=dev)
        dst_v = torch.empty_like(src_v)
        src_m = torch.empty(merge_bytes // 2, dtype=torch.uint8, device=dev)
        dst_m = torch.empty_like(src_m)
        l0n = l0.permute(0, 2, 3, 1)
        l1n = None if l1 is None else l1.permute(0, 2, 3, 1)
        xn = x.permute(0, 2, 3, 1)
        t = alternate({"views": lambda: ops.tta_views(x, mode),
                       "views_torch": lambda: torch_views(xn, views),
                       "views_copy": lambda: dst_v.copy_(src_v),
                       "merge": lambda: ops.tta_merge(l0, l1, mode, (H, W)),
                       "merge_torch": lambda: torch_merge(l0n, l1n, views, B),
                       "merge_copy": lambda: dst_m.copy_(src_m)}, args.iters, args.rounds)
        same = float((ops.tta_merge(l0, l1, mode, (H, W)).classes == torch_merge(l0n, l1n, views, B)).float().mean())
        gbs = lambda nbytes, ms: nbytes / (ms * 1e-3) / 1e9
        out["kernels"][mode] = {
            "views_ms": t["views"], "views_bytes": views_bytes, "views_GBps": gbs(views_bytes, t["views"]["median"]),
            "views_copy_ms": t["views_copy"], "views_copy_GBps": gbs(views_bytes, t["views_copy"]["median"]),
            "views_torch_ops_ms": t["views_torch"],
            "views_torch_over_kernel": t["views_torch"]["median"] / t["views"]["median"],
            "merge_ms": t["merge"], "merge_bytes": merge_bytes, "merge_GBps": gbs(merge_bytes, t["merge"]["median"]),
            "merge_copy_ms": t["merge_copy"], "merge_copy_GBps": gbs(merge_bytes, t["merge_copy"]["median"]),
            "merge_torch_ops_ms": t["merge_torch"],
            "merge_torch_over_kernel": t["merge_torch"]["median"] / t["merge"]["median"],
            "merge_faster_beyond_spread": bool(t["merge"]["max"] < t["merge_torch"]["min"]),
            "classes_equal_to_torch_ops_fraction": same}
        del logits, l0, l1, src_v, dst_v, src_m, dst_m
    # end to end: BatchPredictor, UNet(1, 3), 512 x 512, batch 8
    torch.manual_seed(0)
    model = unet_amd.UNet(1, 3, bilinear=False)
    images = phantoms(args.images, H, W)
    preds = {"off": unet_amd.BatchPredictor(model, batch=8, batch_invariant=True)}
    runs = {"off": lambda: preds["off"](images)}
    for mode in ("flips", "d4"):
        preds[mode] = unet_amd.BatchPredictor(model, batch=8, batch_invariant=True, tta=mode)
        preds[mode + "_torch"] = unet_amd.BatchPredictor(model, batch=8, batch_invariant=True, tta=mode)
        runs[mode] = lambda m=mode: preds[m](images)

        def composed(m=mode):
            p, views = preds[m + "_torch"], tta_view_list(m)
            g = p.tta_group(H, W)
            return [torch_launch(p, images[s:s + g], views) for s in range(0, len(images), g)]
        runs[mode + "_torch"] = composed
    for fn in runs.values():
        for _ in range(2):
            fn()
    rates = {k: [] for k in runs}
    for _ in range(args.rounds):
        for k, fn in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            rates[k].append(len(images) / (time.perf_counter() - t0))
    e2e = {"model": "UNet(1,3)", "size": f"{H}x{W}", "batch": 8, "images": len(images), "amp": True, "batch_invariant": True,
           "images_per_s": {k: spread(v) for k, v in rates.items()}}
    off = e2e["images_per_s"]["off"]["median"]
    for mode in ("flips", "d4"):
        V = len(tta_view_list(mode))
        e2e[mode + "_cost_beyond_forwards"] = off / (V * e2e["images_per_s"][mode]["median"])
        e2e[mode + "_torch_ops_cost_beyond_forwards"] = off / (V * e2e["images_per_s"][mode + "_torch"]["median"])
        e2e[mode + "_over_torch_ops"] = e2e["images_per_s"][mode]["median"] / e2e["images_per_s"][mode + "_torch"]["median"]
    out["end_to_end"] = e2e
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
