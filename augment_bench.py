"""Benchmark of the training augmentation (csrc/augment.hip).  Prints one JSON line and writes it to
profiles/augment_bench.json.

    python augment_bench.py [--iters 50] [--pairs 64] [--size 1024] [--batch 8] [--scale 0.5] [--epochs 3] [--rounds 2]
                            [--workers 8] [--out profiles/augment_bench.json]

  - device time (events around 20 back-to-back launches, warm-up, median of --iters samples with min / max) of uh_batch_augment on one 8 x 1 x 512^2 fp32 batch
    (image + labels) for two configurations: the geometric part alone, and every stage (gamma, contrast, brightness, noise);
    the achieved bytes/s over the 2 (4 C + 8) bytes per pixel the stage has to move; the identity table for scale (a copy
    through the same kernel); and the same batch's uh_batch_prepare (from device-resident uint8 bytes);
  - the epoch loop of train_bench.py (UNet(1,1,bilinear), bf16, batch 8, --pairs PNG pairs at --size^2, scale 0.5) with and
    without the preset `--augment`, alternating in one process, `--rounds` runs each, the first epoch of every run a warm-up.
    The cost of augmentation is read against the spread of the un-augmented loop's own repeats."""
import argparse
import json
import os
import statistics
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

GEOMETRY = "flip,rotate=10,scale=0.1,translate=0.05"


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def device_us(fn, iters, warmup=5, inner=20):
    """Microseconds per call: `iters` samples of `inner` back-to-back calls between two events (a launch of some tens of
    microseconds alone between two events would measure the events)."""
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
        ts.append(e0.elapsed_time(e1) * 1e3 / inner)
    return spread(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--scale", type=float, default=0.5)
    ap.add_argument("--epochs", type=int, default=3, help="epochs per run; the first is a warm-up")
    ap.add_argument("--rounds", type=int, default=2, help="plain / augmented runs, alternated")
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("augment_bench.py needs an MI355X")
    import unet_amd
    from train_bench import write_tree
    from unet_amd import AugmentConfig, BatchAugment
    from unet_amd.train_cli import run_training
    from unet_amd.utils.data_loading import BasicDataset, DeviceBatchLoader, prepare_batch_device
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    out = {"metric": "batch_augment_device_us", "device": torch.cuda.get_device_name(0), "iters": args.iters}

    # ---- the kernel alone: 8 x 1 x 512^2 fp32, image + labels
    B, C, H, W = 8, 1, 512, 512
    g = torch.Generator().manual_seed(0)
    u8 = torch.randint(0, 256, (B, H, W, C), dtype=torch.uint8, generator=g).to(dev)
    m8 = torch.tensor([0, 128, 255], dtype=torch.uint8)[torch.randint(0, 3, (B, H, W), generator=g)].to(dev)
    batch = prepare_batch_device(u8, m8, None, device=dev)
    idx = list(range(B))
    nbytes = 2 * (4 * C + 8) * B * H * W
    kern = {"batch": B, "channels": C, "size": f"{H}x{W}", "dtype": "fp32", "bytes_moved": nbytes}
    for name, spec in (("identity", "none"), ("geometry", GEOMETRY), ("all_stages", "default")):
        aug = BatchAugment(AugmentConfig.parse(spec), 0)
        table = torch.from_numpy(aug.params(0, idx, (H, W)).view("uint8").reshape(B, -1).copy()).to(dev)
        nhwc = batch["image"].permute(0, 2, 3, 1).contiguous()
        o_i, o_l = torch.empty_like(nhwc), torch.empty_like(batch["mask"])
        from unet_amd._lib import LIB

        def launch():           # the launch alone: no table upload, no allocation
            LIB.call("uh_batch_augment", nhwc.data_ptr(), C, batch["mask"].data_ptr(), table.data_ptr(), o_i.data_ptr(), C,
                     o_l.data_ptr(), B, H, W, C, 0, 0, 0.0, 1, torch.cuda.current_stream().cuda_stream)
        t = device_us(launch, args.iters)
        kern[name + "_us"] = t
        kern[name + "_tb_s"] = nbytes / (t["median"] * 1e-6) / 1e12
        kern[name + "_call_us"] = device_us(lambda: aug(batch, 0, idx), args.iters)      # with the table upload and the allocations
    kern["prepare_us"] = device_us(lambda: prepare_batch_device(u8, m8, None, device=dev), args.iters)
    out["kernel"] = kern

    # ---- the epoch loop with and without --augment
    with tempfile.TemporaryDirectory() as tmp:
        write_tree(tmp, args.pairs, max(1, args.pairs // 4), args.size)
        train = BasicDataset(os.path.join(tmp, "imgs", "train"), os.path.join(tmp, "masks", "train"), args.scale)
        val = BasicDataset(os.path.join(tmp, "imgs", "val"), os.path.join(tmp, "masks", "val"), args.scale)

        def loop(spec):
            torch.manual_seed(0)
            model = unet_amd.UNet(1, 1, bilinear=True).to(memory_format=torch.channels_last).to(dev)
            loader = DeviceBatchLoader(train, args.batch, shuffle=True, drop_last=False, seed=0, workers=args.workers, device=dev)
            hist = run_training(model, dev, train, val, epochs=args.epochs, batch_size=args.batch, learning_rate=1e-5, amp=True,
                                checkpoint_dir=None, train_loader=loader, augment=spec)
            return [h["img_s"] for h in hist[1:]]

        plain, augmented = [], []
        for _ in range(args.rounds):
            plain += loop(None)
            augmented += loop("default")
        ep = {"model": "UNet(1,1,bilinear=True)", "dtype": "bf16", "batch": args.batch, "source": f"{args.size}x{args.size}",
              "scale": args.scale, "pairs": args.pairs, "n_train": len(train), "workers": args.workers,
              "plain_img_s": spread(plain), "plain_img_s_all": [round(r, 1) for r in plain],
              "augment_img_s": spread(augmented), "augment_img_s_all": [round(r, 1) for r in augmented]}
        ep["augment_over_plain"] = ep["augment_img_s"]["median"] / ep["plain_img_s"]["median"]
        ep["plain_spread"] = (ep["plain_img_s"]["max"] - ep["plain_img_s"]["min"]) / ep["plain_img_s"]["median"]
        ep["augment_median_inside_plain_spread"] = bool(ep["plain_img_s"]["min"] <= ep["augment_img_s"]["median"]
                                                        <= ep["plain_img_s"]["max"])
        out["epoch_loop"] = ep
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
