"""Benchmark of the training command line's epoch loop (python -m unet_amd.train) on a folder of PNGs.  Prints one JSON line.

    python train_bench.py [--pairs 64] [--size 1024] [--batch 8] [--scale 0.5] [--epochs 3] [--rounds 2] [--workers 8]

Writes a seeded synthetic dataset to a temp dir (`--pairs` 1024^2 PNG pairs from ellipse_batch, masks coded 0/128/255,
plus a quarter as many validation pairs) and trains UNet(1, 1, bilinear=True) in bf16 at batch 8, scale 0.5 (-> 512^2),
x4 augmentation on, through train_cli.run_training.  Every run's first epoch is a warm-up; the others are timed.
    epoch_img_s               the loop with DeviceBatchLoader: decode threads, rotate + rescale on the device
    host_rescale_epoch_img_s  the same loop with Pillow rescaling in the decode threads (raw_item's default path);
                              the two alternate, `--rounds` times each, in one process
    step_img_s                TrainStepper alone on the same batches already on the device (the ceiling)
    rescale_us_per_batch      uh_batch_rescale_u8 on one B x 1024^2 batch (device events), prepare_us_per_batch the
                              whole prepare_batch_device (rescale + /255 + remap) from device-resident uint8 bytes
    loader_img_s / host_loader_img_s  the two loaders alone (no training), decode_ms_per_item one raw_item on one thread
An epoch's images/s counts the training images over the epoch's wall time without its evaluation."""
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


def write_tree(root, n_train, n_val, size, seed=0):
    from PIL import Image
    from unet_amd import ellipse_batch
    grey = np.array([0, 128, 255], np.uint8)
    for split, n, s in (("train", n_train, seed), ("val", n_val, seed + 1)):
        for d in ("imgs", "masks"):
            os.makedirs(os.path.join(root, d, split), exist_ok=True)
        for c in range(0, n, 8):
            k = min(8, n - c)
            imgs, masks = ellipse_batch(k, size, seed=s * 1000 + c)
            for i in range(k):
                stem = f"s{c + i:04d}"
                Image.fromarray((imgs[i, 0].numpy() * 255).astype(np.uint8)).save(os.path.join(root, "imgs", split, stem + ".png"))
                Image.fromarray(grey[masks[i].numpy()]).save(os.path.join(root, "masks", split, stem + "_mask.png"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--scale", type=float, default=0.5)
    ap.add_argument("--epochs", type=int, default=3, help="epochs per run; the first is a warm-up")
    ap.add_argument("--rounds", type=int, default=2, help="device / host runs, alternated")
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("train_bench.py needs a GPU")
    import unet_amd
    from unet_amd.train import TrainStepper
    from unet_amd.train_cli import run_training
    from unet_amd.utils.data_loading import BasicDataset, DeviceBatchLoader, collate_raw, prepare_batch_device
    from unet_amd.utils.data_rescale import batch_rescale
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    out = {"model": "UNet(1,1,bilinear=True)", "dtype": "bf16", "batch": args.batch, "source": f"{args.size}x{args.size}",
           "scale": args.scale, "pairs": args.pairs, "workers": args.workers, "device": torch.cuda.get_device_name(0)}
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.perf_counter()
        write_tree(tmp, args.pairs, max(1, args.pairs // 4), args.size)
        out["dataset_write_s"] = round(time.perf_counter() - t0, 1)
        train = BasicDataset(os.path.join(tmp, "imgs", "train"), os.path.join(tmp, "masks", "train"), args.scale)
        val = BasicDataset(os.path.join(tmp, "imgs", "val"), os.path.join(tmp, "masks", "val"), args.scale)
        out["n_train"], out["n_val"] = len(train), len(val)

        def fresh_model():
            torch.manual_seed(0)
            return unet_amd.UNet(1, 1, bilinear=True).to(memory_format=torch.channels_last).to(dev)

        def loader(host):
            return DeviceBatchLoader(train, args.batch, shuffle=True, drop_last=False, seed=0, workers=args.workers,
                                     device=dev, host_rescale=host)

        # the ceiling: TrainStepper alone on the same batches, already on the device (a fresh model, as every run below)
        batches = list(loader(False))
        stepper = TrainStepper(fresh_model(), lr=1e-5, amp=True)
        for b in batches[:3]:
            stepper.step(b["image"], b["mask"])
        torch.cuda.synchronize()
        rates = []
        for _ in range(3):
            t0 = time.perf_counter()
            for b in batches:
                stepper.step(b["image"], b["mask"])
            torch.cuda.synchronize()
            rates.append(sum(b["image"].shape[0] for b in batches) / (time.perf_counter() - t0))
        stepper.close()
        del batches, stepper
        out["step_img_s"] = round(float(np.median(rates)), 1)

        def loop(host):
            hist = run_training(fresh_model(), dev, train, val, epochs=args.epochs, batch_size=args.batch, learning_rate=1e-5,
                                amp=True, checkpoint_dir=None, train_loader=loader(host))
            return [h["img_s"] for h in hist[1:]]

        dev_rates, host_rates = [], []
        for _ in range(args.rounds):
            dev_rates += loop(False)
            host_rates += loop(True)
        out["epoch_img_s"] = round(float(np.median(dev_rates)), 1)
        out["epoch_img_s_all"] = [round(r, 1) for r in dev_rates]
        out["host_rescale_epoch_img_s"] = round(float(np.median(host_rates)), 1)
        out["host_rescale_epoch_img_s_all"] = [round(r, 1) for r in host_rates]

        # the loaders alone
        for key, host in (("loader_img_s", False), ("host_loader_img_s", True)):
            ld = loader(host)
            list(ld)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = sum(b["image"].shape[0] for b in ld)
            torch.cuda.synchronize()
            out[key] = round(n / (time.perf_counter() - t0), 1)
        t0 = time.perf_counter()
        for i in range(8):
            train.raw_item(i, host_rescale=False)
        out["decode_ms_per_item"] = round((time.perf_counter() - t0) / 8 * 1e3, 2)
        t0 = time.perf_counter()
        for i in range(8):
            train.raw_item(i)
        out["host_rescale_ms_per_item"] = round((time.perf_counter() - t0) / 8 * 1e3, 2)

        out["epoch_over_step"] = round(out["epoch_img_s"] / out["step_img_s"], 3)
        out["host_over_step"] = round(out["host_rescale_epoch_img_s"] / out["step_img_s"], 3)

        # the rescale kernel alone, on one batch of raw bytes already on the device
        raw = collate_raw([train.raw_item(i, host_rescale=False) for i in range(0, 4 * args.batch, 4)])   # turns 0
        img_d, msk_d = raw["image_u8"].cuda(), raw["mask_u8"].cuda()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        reps = 50
        for _ in range(5):
            batch_rescale(img_d, msk_d, None, 0, args.scale)
        ev[0].record()
        for _ in range(reps):
            batch_rescale(img_d, msk_d, None, 0, args.scale)
        ev[1].record()
        for _ in range(reps):
            prepare_batch_device(img_d, msk_d, None, device=dev, scale=args.scale)
        ev[2].record()
        torch.cuda.synchronize()
        out["rescale_us_per_batch"] = round(ev[0].elapsed_time(ev[1]) / reps * 1e3, 1)
        out["prepare_us_per_batch"] = round(ev[1].elapsed_time(ev[2]) / reps * 1e3, 1)
        B, H, W = msk_d.shape
        Ho, Wo = int(args.scale * H), int(args.scale * W)
        out["rescale_hbm_bytes"] = int(2 * B * H * W + 2 * B * Ho * Wo)       # the bytes read and written, intermediate excluded
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
