"""Benchmark of the elastic deformation kernel (csrc/augment.hip: uh_batch_augment_elastic) beside the affine launch it
extends.  Prints one JSON line and writes it to profiles/elastic_bench.json.

    python elastic_bench.py [--iters 50] [--out profiles/elastic_bench.json]

Device time of one launch on an 8 x 1 x 512^2 fp32 batch (image + labels), geometry only (no photometric stage), for
uh_batch_augment and for uh_batch_augment_elastic at control spacings 64 (sigma 4), 16 (sigma 1) and 256 (sigma 16).  The
legs ALTERNATE in one process: every round takes one sample of each leg (events around 20 back-to-back launches), so
drift of the shared machine lands on all of them alike; the figures are the median, min and max of --iters rounds, and
the ratio of each elastic leg to the affine launch of the same run."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from augment_bench import GEOMETRY, spread  # noqa: E402

INNER = 20


def sample_us(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(INNER):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / INNER


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "elastic_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("elastic_bench.py needs an MI355X")
    from unet_amd import AugmentConfig, BatchAugment, ElasticConfig
    from unet_amd._lib import LIB
    from unet_amd.utils.augment import elastic_weights
    from unet_amd.utils.data_loading import prepare_batch_device
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B, C, H, W = 8, 1, 512, 512
    g = torch.Generator().manual_seed(0)
    u8 = torch.randint(0, 256, (B, H, W, C), dtype=torch.uint8, generator=g).to(dev)
    m8 = torch.tensor([0, 128, 255], dtype=torch.uint8)[torch.randint(0, 3, (B, H, W), generator=g)].to(dev)
    batch = prepare_batch_device(u8, m8, None, device=dev)
    nhwc, mask = batch["image"].permute(0, 2, 3, 1).contiguous(), batch["mask"]
    o_i, o_l = torch.empty_like(nhwc), torch.empty_like(mask)
    idx = list(range(B))
    cfg = AugmentConfig.parse(GEOMETRY)
    rows = torch.from_numpy(BatchAugment(cfg, 0).params(0, idx, (H, W)).view("uint8").reshape(B, -1).copy()).to(dev)
    stream = torch.cuda.current_stream().cuda_stream

    def affine():           # the launch alone: no table upload, no allocation
        LIB.call("uh_batch_augment", nhwc.data_ptr(), C, mask.data_ptr(), rows.data_ptr(), o_i.data_ptr(), C, o_l.data_ptr(),
                 B, H, W, C, 0, 0, 0.0, 1, stream)

    def elastic(grid, sigma):
        el = ElasticConfig(grid=grid, sigma=sigma)
        control = torch.from_numpy(BatchAugment(cfg, 0, elastic=el).elastic_table(0, idx, (H, W))).to(dev)
        weights = torch.from_numpy(elastic_weights(grid)).to(dev)

        def launch():
            LIB.call("uh_batch_augment_elastic", nhwc.data_ptr(), C, mask.data_ptr(), rows.data_ptr(), control.data_ptr(),
                     weights.data_ptr(), grid, o_i.data_ptr(), C, o_l.data_ptr(), B, H, W, C, 0, 0, 0.0, 1, stream)
        launch.keep = (control, weights)
        return launch

    legs = {"affine": affine, "elastic_grid64": elastic(64, 4.0), "elastic_grid16": elastic(16, 1.0),
            "elastic_grid256": elastic(256, 16.0)}
    for fn in legs.values():                                    # warm-up: code objects, caches
        for _ in range(5 * INNER):
            fn()
    torch.cuda.synchronize()
    samples = {name: [] for name in legs}
    for _ in range(args.iters):
        for name, fn in legs.items():
            samples[name].append(sample_us(fn))
    nbytes = 2 * (4 * C + 8) * B * H * W
    out = {"metric": "batch_augment_elastic_device_us", "device": torch.cuda.get_device_name(0), "iters": args.iters,
           "inner_launches": INNER, "batch": B, "channels": C, "size": f"{H}x{W}", "dtype": "fp32", "geometry": GEOMETRY,
           "bytes_moved": nbytes}
    for name, ts in samples.items():
        out[name + "_us"] = spread(ts)
        out[name + "_tb_s"] = nbytes / (out[name + "_us"]["median"] * 1e-6) / 1e12
        if name != "affine":
            out[name + "_over_affine"] = out[name + "_us"]["median"] / out["affine_us"]["median"]
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
