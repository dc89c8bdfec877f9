"""Benchmark of patch training (csrc/crop.hip).  Prints one JSON line and writes it to profiles/crop_bench.json.

    python crop_bench.py [--iters 20] [--rounds 5] [--files 16] [--legs select,gather,loader] [--out profiles/crop_bench.json]

Everything runs in one process on warmed shapes, in --rounds rounds that alternate the candidates; reported is the median
(min - max) of the rounds.  No thresholds are set here.
  select   device events around back-to-back ops.crop_select calls on 8 int64 label planes of 512 x 512, 2048 x 2048 and
           4096 x 4096 (a thin class-2 ring, under 1 % of the pixels; every row on the foreground branch), beside a torch
           device copy of the same label bytes and beside the same origins composed from torch ops: per plane isin, nonzero
           and an index with the rank (its nonzero synchronises with the host: the events then bracket that wait as well);
  gather   ops.crop_gather of 8 crops of 512 x 512 out of 2048 x 2048 items (one fp32 channel + int64 labels) beside a copy
           of its output bytes and beside slice + stack;
  loader   DeviceBatchLoader over --files PNG pairs of 2048 x 2048 with crop 512 (decode threads, device prepare, select,
           gather): images/s of whole epochs from a host clock, beside the images/s of TrainStepper(UNet_S(1,3), bf16) alone
           on one resident 8 x 512 x 512 batch -- and which of the two bounds the loop."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

CLASS = 2
MASK = 1 << CLASS
ALWAYS = 1 << 32


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


def ring_labels(rng, H, W):
    """int64 [H,W]: 0 outside, 1 inside an ellipse, a ring of class 2 about three pixels wide between them."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    cx, cy = W * rng.uniform(0.4, 0.6), H * rng.uniform(0.4, 0.6)
    rx, ry = W * rng.uniform(0.25, 0.35), H * rng.uniform(0.25, 0.35)
    d = np.sqrt(((xx - cx) / rx) ** 2 + ((yy - cy) / ry) ** 2)
    lab = (d < 1).astype(np.int64)
    lab[np.abs(d - 1) * min(rx, ry) < 1.5] = CLASS
    return lab


def torch_select(labels, words, size, classes):
    """The foreground branch of every plane composed from torch ops -> origins on the host (nonzero synchronises)."""
    out = []
    for lab, r in zip(labels, words):
        H, W = lab.shape
        at = torch.isin(lab, classes).flatten().nonzero()
        n = at.shape[0]
        p = int(at[(int(r[1]) * n) >> 32])
        py, px = divmod(p, W)
        jy, jx = (int(r[2]) * size) >> 32, (int(r[3]) * size) >> 32
        out.append((min(max(py - jy, 0), H - size), min(max(px - jx, 0), W - size)))
    return out


def leg_select(args, dev):
    from unet_amd import ops
    rng = np.random.default_rng(0)
    classes = torch.tensor([CLASS], device=dev)
    rows = []
    for side, size in ((512, 256), (2048, 512), (4096, 512)):
        labels = [torch.from_numpy(ring_labels(rng, side, side)).to(dev) for _ in range(8)]
        words = rng.integers(0, 1 << 32, (8, 4), dtype=np.uint64).astype(np.uint32)
        nbytes = 8 * side * side * 8
        src = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        iters = max(2, args.iters // (4 if side == 4096 else 1))
        t = alternate({"select": lambda: ops.crop_select(labels, words, size, MASK, ALWAYS),
                       "copy": lambda: dst.copy_(src),
                       "torch": lambda: torch_select(labels, words, size, classes)}, iters, args.rounds)
        origins, counts = ops.crop_select(labels, words, size, MASK, ALWAYS)
        same = origins.cpu().tolist() == [list(o) for o in torch_select(labels, words, size, classes)]
        gbs = lambda ms: nbytes / (ms * 1e-3) / 1e9
        rows.append({"shape": f"8 x {side} x {side} int64", "crop": size, "label_bytes": nbytes,
                     "foreground_fraction": float(counts.sum().item()) / (8 * side * side),
                     "select_ms": t["select"], "select_GBps_of_labels_read_once": gbs(t["select"]["median"]),
                     "copy_ms": t["copy"], "copy_GBps_read_plus_write": 2 * gbs(t["copy"]["median"]),
                     "select_over_copy": t["select"]["median"] / t["copy"]["median"],
                     "torch_ops_ms": t["torch"], "torch_over_kernel": t["torch"]["median"] / t["select"]["median"],
                     "select_faster_beyond_spread": bool(t["select"]["max"] < t["torch"]["min"]),
                     "origins_equal_to_torch_ops": bool(same)})
        del labels, src, dst
        torch.cuda.empty_cache()
    return rows


def leg_gather(args, dev):
    from unet_amd import ops
    rng = np.random.default_rng(1)
    g = torch.Generator().manual_seed(1)
    side, size, B = 2048, 512, 8
    images = [torch.rand(side, side, 1, generator=g).to(dev).permute(2, 0, 1) for _ in range(B)]
    labels = [torch.from_numpy(ring_labels(rng, side, side)).to(dev) for _ in range(B)]
    at = [(int(rng.integers(0, side - size + 1)), int(rng.integers(0, side - size + 1))) for _ in range(B)]
    origins = torch.tensor(at, dtype=torch.int32, device=dev)
    nbytes = B * size * size * (4 + 8)
    src = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)

    def composed():
        return (torch.stack([x[:, oy:oy + size, ox:ox + size] for x, (oy, ox) in zip(images, at)]),
                torch.stack([m[oy:oy + size, ox:ox + size] for m, (oy, ox) in zip(labels, at)]))

    t = alternate({"gather": lambda: ops.crop_gather(images, labels, origins, size), "copy": lambda: dst.copy_(src),
                   "torch": composed}, args.iters, args.rounds)
    a, b = ops.crop_gather(images, labels, origins, size), composed()
    gbs = lambda ms: 2 * nbytes / (ms * 1e-3) / 1e9
    return {"shape": f"{B} crops of {size} x {size} from {side} x {side}, 1 fp32 channel + int64 labels", "output_bytes": nbytes,
            "gather_ms": t["gather"], "gather_GBps_read_plus_write": gbs(t["gather"]["median"]),
            "copy_ms": t["copy"], "copy_GBps_read_plus_write": gbs(t["copy"]["median"]),
            "gather_over_copy": t["gather"]["median"] / t["copy"]["median"],
            "torch_ops_ms": t["torch"], "torch_over_kernel": t["torch"]["median"] / t["gather"]["median"],
            "gather_faster_beyond_spread": bool(t["gather"]["max"] < t["torch"]["min"]),
            "equal_to_torch_ops": bool(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]))}


def leg_loader(args, dev):
    import unet_amd
    from PIL import Image
    from unet_amd.utils.data_loading import DeviceBatchLoader
    rng = np.random.default_rng(2)
    side, size, B = 2048, 512, 8
    grey = np.array([0, 128, 255], np.uint8)
    with tempfile.TemporaryDirectory() as top:
        for d in ("imgs", "masks"):
            os.makedirs(os.path.join(top, d))
        for i in range(args.files):
            lab = ring_labels(rng, side, side)
            img = np.clip(40 + 80 * lab + rng.normal(0, 10, lab.shape), 0, 255).astype(np.uint8)
            Image.fromarray(img).save(os.path.join(top, "imgs", f"p{i:03d}.png"))
            Image.fromarray(grey[lab]).save(os.path.join(top, "masks", f"p{i:03d}_mask.png"))
        ds = unet_amd.BasicDataset(os.path.join(top, "imgs"), os.path.join(top, "masks"), 1.0)
        loader = DeviceBatchLoader(ds, B, shuffle=True, seed=0, workers=args.workers, device=dev,
                                   crop=unet_amd.BatchCrop(f"{size}", seed=0, n_classes=3))

        def epoch():
            n = 0
            for batch in loader:
                n += batch["image"].shape[0]
            torch.cuda.synchronize()
            return n

        epoch()
        rates = []
        for _ in range(args.rounds):
            t0 = time.perf_counter()
            n = epoch()
            rates.append(n / (time.perf_counter() - t0))
        batch = next(iter(loader))
    torch.manual_seed(0)
    model = unet_amd.UNet_S(1, 3, bilinear=False).to(memory_format=torch.channels_last).to(dev)
    stepper = unet_amd.TrainStepper(model, lr=1e-5, amp=True)
    images, masks = batch["image"], batch["mask"]
    step = alternate({"step": lambda: stepper.step(images, masks)}, max(5, args.iters // 2), args.rounds)["step"]
    stepper.close()
    step_rate = {"median": B / (step["median"] * 1e-3), "min": B / (step["max"] * 1e-3), "max": B / (step["min"] * 1e-3)}
    r = spread(rates)
    return {"files": args.files, "items_per_epoch": len(ds), "source": f"{side} x {side} 8-bit PNG pairs", "crop": size, "batch": B,
            "workers": args.workers, "host_cpus": os.cpu_count(), "loader_images_per_s": r,
            "train_step": "TrainStepper(UNet_S(1,3), bf16) on one resident 8 x 1 x 512 x 512 batch", "step_ms": step,
            "step_images_per_s": step_rate, "loader_over_step": r["median"] / step_rate["median"],
            "bound_by": "loader (PNG decode)" if r["max"] < step_rate["min"] else ("train step" if r["min"] > step_rate["max"] else "neither beyond the spread")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--files", type=int, default=16)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--legs", default="select,gather,loader")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crop_bench.json"))
    args = ap.parse_args()
    if args.rounds < 5:
        sys.exit("crop_bench.py reports the spread of at least 5 alternated rounds")
    if not torch.cuda.is_available():
        sys.exit("crop_bench.py needs an MI355X")
    dev = torch.device("cuda:0")
    out = {"metric": "crop_bench", "device": torch.cuda.get_device_name(0), "iters": args.iters, "rounds": args.rounds}
    legs = args.legs.split(",")
    if "select" in legs:
        out["select"] = leg_select(args, dev)
    if "gather" in legs:
        out["gather"] = leg_gather(args, dev)
    if "loader" in legs:
        out["loader"] = leg_loader(args, dev)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
