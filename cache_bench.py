"""Benchmark of the device-resident dataset cache (utils/dataset_cache.py, csrc/cache.hip).  Prints one JSON line and writes it
to profiles/cache_bench.json.

    python cache_bench.py [--pairs 64] [--size 1024] [--batch 8] [--scale 0.5] [--epochs 3] [--rounds 2] [--iters 30] [--workers 8]

Everything is measured in ONE process, the two sides of every comparison alternated, every run listed beside its median:
    gather      uh_cache_gather_u8 (image + mask of 8 items, one launch) against ONE device-to-device copy of the same number of
                bytes, at 8 x 1024^2 and 8 x 512^2: single calls between device events, each behind a write over a buffer larger
                than the last-level cache, taking turns (ema_bench.cold_samples).  over_copy = median / median; the copy's own
                max / median says what a ratio near 1 is worth.
    loader      DeviceBatchLoader alone, cached and uncached, on train_bench.py's dataset (64 PNG pairs at 1024^2, -s 0.5, x4
                views = 256 items, batch 8): images/s of one epoch, a host clock round an epoch that ends in a synchronise.
                build_seconds, nbytes and decodes are the cache's own.  enqueue_ms_per_batch is the host time the cached
                loader takes to issue a batch (no synchronise inside the window).
    epoch       train_cli.run_training, cached (what --cache does: both sets) and uncached, for UNet(1,1,bilinear) and UNet_S(1,3),
                bf16, beside TrainStepper alone on the same batches already on the device: epoch_over_step for each, the uncached
                spread (max - min) / median, and break_even_epochs = build_seconds / (uncached epoch time - cached epoch time).
                step_enqueue_ms_per_batch is the host time one step takes to issue.
An epoch's images/s counts the training images over the epoch's wall time without its evaluation; a run's first epoch is a warm-up."""
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

from ema_bench import cold_samples, spread  # noqa: E402
from train_bench import write_tree  # noqa: E402


def rates(xs):
    return dict(spread(xs), all=[round(x, 1) for x in xs], spread=(max(xs) - min(xs)) / statistics.median(xs))


def gather_vs_copy(dev, batch, sizes, iters):
    from unet_amd import plan_entries
    from unet_amd._lib import LIB
    out = {}
    evict = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    for size in sizes:
        n = 2 * batch                                                     # entries in the arena; the batch takes every other one
        io, mo, total = plan_entries([(size, size, 1)] * n)
        arena = torch.randint(0, 256, (total,), dtype=torch.uint8, device=dev)
        order = [(7 * i + 3) % n for i in range(batch)]
        table = np.array([[arena.data_ptr() + io[e], arena.data_ptr() + mo[e]] for e in order], np.uint64)
        ib = mb = size * size
        image = torch.empty(batch * ib, dtype=torch.uint8, device=dev)
        mask = torch.empty(batch * mb, dtype=torch.uint8, device=dev)
        src = arena[:batch * (ib + mb)]
        dst = torch.empty_like(src)
        fns = {"gather": lambda: LIB.call("uh_cache_gather_u8", table.ctypes.data, batch, ib, mb, image.data_ptr(), mask.data_ptr(), stream),
               "copy": lambda: dst.copy_(src)}
        ms = cold_samples(fns, iters, evict)
        nbytes = batch * (ib + mb)
        row = {name: dict(spread(v), GBps=2 * nbytes / statistics.median(v) / 1e6) for name, v in ms.items()}
        out[f"{batch}x{size}x{size}"] = dict(row, bytes=nbytes, over_copy=row["gather"]["median"] / row["copy"]["median"],
                                             gather_max_over_median=row["gather"]["max"] / row["gather"]["median"],
                                             copy_max_over_median=row["copy"]["max"] / row["copy"]["median"])
        want = torch.cat([arena[io[e]:io[e] + ib] for e in order])
        assert torch.equal(image, want), "the timed gather is not the copy it is compared with"
    out["evict_bytes"] = evict.numel()
    return out


def epoch_rate(loader):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = sum(b["image"].shape[0] for b in loader)
    torch.cuda.synchronize()
    return n / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--scale", type=float, default=0.5)
    ap.add_argument("--epochs", type=int, default=3, help="epochs per run; the first is a warm-up")
    ap.add_argument("--rounds", type=int, default=2, help="cached / uncached runs, alternated")
    ap.add_argument("--iters", type=int, default=30, help="cold samples per side of the gather comparison")
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cache_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("cache_bench.py needs an MI355X")
    import unet_amd
    from unet_amd import DatasetCache
    from unet_amd.train import TrainStepper
    from unet_amd.train_cli import CacheSpec, build_model, run_training
    from unet_amd.utils.data_loading import BasicDataset, DeviceBatchLoader
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    out = {"device": torch.cuda.get_device_name(0), "batch": args.batch, "source": f"{args.size}x{args.size}", "scale": args.scale,
           "pairs": args.pairs, "workers": args.workers, "dtype": "bf16"}
    out["gather"] = gather_vs_copy(dev, args.batch, (args.size, args.size // 2), args.iters)
    with tempfile.TemporaryDirectory() as tmp:
        write_tree(tmp, args.pairs, max(1, args.pairs // 4), args.size)
        train = BasicDataset(os.path.join(tmp, "imgs", "train"), os.path.join(tmp, "masks", "train"), args.scale)
        val = BasicDataset(os.path.join(tmp, "imgs", "val"), os.path.join(tmp, "masks", "val"), args.scale)
        out["n_train"], out["n_val"] = len(train), len(val)
        cache = DatasetCache(train, device=dev, workers=args.workers)
        out["cache"] = {"build_seconds": cache.build_seconds, "nbytes": cache.nbytes, "entries": cache.entries, "decodes": cache.decodes}

        def loader(cached):
            return DeviceBatchLoader(train, args.batch, shuffle=True, drop_last=False, seed=0, workers=args.workers, device=dev,
                                     cache=cache if cached else None)

        # the loaders alone
        lds = {"cached": loader(True), "uncached": loader(False)}
        got = {k: [] for k in lds}
        for r in range(args.rounds + 2):
            for k, ld in lds.items():
                rate = epoch_rate(ld)
                if r:                                                     # every loader's first epoch is a warm-up
                    got[k].append(rate)
        ld = lds["cached"]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        nb = sum(1 for _ in ld)
        enqueue = (time.perf_counter() - t0) / nb
        torch.cuda.synchronize()
        out["loader"] = {"cached_img_s": rates(got["cached"]), "uncached_img_s": rates(got["uncached"]),
                         "cached_over_uncached": statistics.median(got["cached"]) / statistics.median(got["uncached"]),
                         "cached_enqueue_ms_per_batch": enqueue * 1e3}

        # the epoch loop, beside the step alone
        models = {"UNet(1,1,bilinear)": lambda: unet_amd.UNet(1, 1, bilinear=True), "UNet_S(1,3)": lambda: build_model("UNet_S", 3, False)}
        out["epoch"] = {}
        for name, make in models.items():
            def fresh_model():
                torch.manual_seed(0)
                return make().to(memory_format=torch.channels_last).to(dev)

            batches = list(loader(True))
            stepper = TrainStepper(fresh_model(), lr=1e-5, amp=True)
            for b in batches[:3]:
                stepper.step(b["image"], b["mask"])
            torch.cuda.synchronize()
            step_rates, step_enqueue = [], []
            for _ in range(3):
                t0 = time.perf_counter()
                for b in batches:
                    stepper.step(b["image"], b["mask"])
                t1 = time.perf_counter()
                torch.cuda.synchronize()
                step_rates.append(sum(b["image"].shape[0] for b in batches) / (time.perf_counter() - t0))
                step_enqueue.append((t1 - t0) / len(batches))
            stepper.close()
            del batches, stepper

            def loop(cached):
                hist = run_training(fresh_model(), dev, train, val, epochs=args.epochs, batch_size=args.batch, learning_rate=1e-5,
                                    amp=True, checkpoint_dir=None, workers=args.workers, train_loader=loader(cached),
                                    cache=CacheSpec() if cached else None)
                return [h["img_s"] for h in hist[1:]]

            runs = {"cached": [], "uncached": []}
            for _ in range(args.rounds):
                runs["uncached"] += loop(False)
                runs["cached"] += loop(True)
            step = statistics.median(step_rates)
            c, u = statistics.median(runs["cached"]), statistics.median(runs["uncached"])
            gain = len(train) / u - len(train) / c                        # seconds per epoch
            out["epoch"][name] = {
                "step_img_s": dict(spread(step_rates), all=[round(r, 1) for r in step_rates]),
                "step_enqueue_ms_per_batch": statistics.median(step_enqueue) * 1e3,
                "cached_img_s": rates(runs["cached"]), "uncached_img_s": rates(runs["uncached"]),
                "cached_epoch_over_step": c / step, "uncached_epoch_over_step": u / step, "cached_over_uncached": c / u,
                "cached_exceeds_uncached_by_more_than_its_spread": c > max(runs["uncached"]),
                "epoch_seconds_saved": gain,
                "break_even_epochs": cache.build_seconds / gain if gain > 0 else None}
        cache.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
