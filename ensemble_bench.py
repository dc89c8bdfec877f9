"""Benchmark of checkpoint ensembles (csrc/ensemble.hip).  Prints one JSON line and writes it to profiles/ensemble_bench.json.

    python ensemble_bench.py [--iters 20] [--images 64] [--rounds 5] [--out profiles/ensemble_bench.json]

Everything runs in one process on warmed shapes:
  - kernel time of uh_ensemble_add (accumulating, first = 0) for its source kinds -- bf16 and fp32 logits, the uint32 sums of
    uh_tta_merge, the uint64 sums of uh_tile_merge -- and of uh_ensemble_finish (classes alone, and all three outputs) at
    B = 8, 512 x 512, NC = 3, as bytes moved over time, beside a torch device-to-device copy that moves the same number of
    bytes: single calls, each behind a write over a buffer larger than the last-level cache, the candidates taking turns
    (ema_bench.cold_samples, as optim_bench.py);
  - BatchPredictor images/s at 512 x 512, batch 8, with an Ensemble of 1, 2, 3 and 5 UNet_S(1, 3) members against M separate
    one-model predictors run over the same images one after the other (what a user could do before), in --rounds rounds that
    alternate the candidates (a host clock around work that ends in a synchronise), and the device time of the stages of the
    three-member ensemble."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
from ema_bench import cold_samples, spread  # noqa: E402
from tta_bench import phantoms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ensemble_bench.py needs an MI355X")
    import unet_amd
    from unet_amd import ops
    from unet_amd._lib import LIB, UH_BF16, UH_F32
    dev = torch.device("cuda:0")
    B, H, W, NC = 8, 512, 512, 3
    npix = B * H * W
    out = {"metric": "ensemble_device_ms", "device": torch.cuda.get_device_name(0), "iters": args.iters, "rounds": args.rounds,
           "shape": {"B": B, "H": H, "W": W, "NC": NC}}

    # ---- (a) the two kernels against a copy of the bytes they move
    g = torch.Generator(device="cpu").manual_seed(0)
    logits = 2.0 * torch.randn(B, H, W, NC, generator=g)
    srcs = {"add_bf16": (logits.to(torch.bfloat16).to(dev), UH_BF16, 2), "add_f32": (logits.to(dev), UH_F32, 4),
            "add_u32": (torch.randint(0, 1 << 27, (B, H, W, NC), generator=g, dtype=torch.int32).to(dev), ops.UH_TILE_SUMS_I32, 4),
            "add_u64": (torch.randint(0, 1 << 48, (B, H, W, NC), generator=g, dtype=torch.int64).to(dev), ops.UH_ENS_SUMS_U64, 8)}
    acc = ops.ensemble_add(srcs["add_bf16"][0].permute(0, 3, 1, 2), 1)
    classes = torch.empty(B, H, W, dtype=torch.uint8, device=dev)
    conf = torch.empty(B, H, W, dtype=torch.uint8, device=dev)
    probs = torch.empty(B, H, W, NC, dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    fns, nbytes = {}, {}
    for name, (t, kind, esize) in srcs.items():
        fns[name] = lambda t=t, kind=kind: LIB.call("uh_ensemble_add", t.data_ptr(), kind, npix, NC, 2, 0, acc.data_ptr(), stream)
        nbytes[name] = npix * NC * (esize + 16)                        # the source, the sums read and written
    fns["finish_classes"] = lambda: LIB.call("uh_ensemble_finish", acc.data_ptr(), None, 1, 4, npix, NC, classes.data_ptr(), None, None,
                                             stream)
    nbytes["finish_classes"] = npix * (NC * 8 + 1)
    fns["finish_all"] = lambda: LIB.call("uh_ensemble_finish", acc.data_ptr(), None, 1, 4, npix, NC, classes.data_ptr(),
                                         probs.data_ptr(), conf.data_ptr(), stream)
    nbytes["finish_all"] = npix * (NC * 8 + 1 + NC * 4 + 1)
    for name in list(nbytes):
        src = torch.empty(nbytes[name] // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        fns[name + "_copy"] = lambda s=src, d=dst: d.copy_(s)
    evict = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
    cold = cold_samples(fns, args.iters, evict)
    kern = {"evict_bytes": evict.numel()}
    for name, nb in nbytes.items():
        k, c = spread(cold[name]), spread(cold[name + "_copy"])
        kern[name] = {"ms": k, "bytes": nb, "GBps": nb / k["median"] / 1e6, "copy_ms": c, "copy_GBps": nb / c["median"] / 1e6,
                      "over_copy": k["median"] / c["median"]}
    out["kernels"] = kern
    del evict, fns, srcs, acc, probs

    # ---- (b) BatchPredictor: an ensemble of M members against M separate one-model passes
    images = phantoms(args.images, H, W)
    models = []
    for s in range(5):
        torch.manual_seed(s)
        models.append(unet_amd.UNet_S(1, 3, bilinear=False))
    solo = [unet_amd.BatchPredictor(m, batch=8, batch_invariant=True) for m in models]
    runs = {}
    for M in (1, 2, 3, 5):
        p = unet_amd.BatchPredictor(unet_amd.Ensemble(models[:M]), batch=8, batch_invariant=True)
        runs[f"ensemble_{M}"] = lambda p=p: p(images)
        runs[f"separate_{M}"] = lambda M=M: [q(images) for q in solo[:M]]
        if M == 3:
            staged = p
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
    e2e = {"model": "UNet_S(1,3)", "size": f"{H}x{W}", "batch": 8, "images": len(images), "amp": True, "batch_invariant": True,
           "images_per_s": {k: spread(v) for k, v in rates.items()}}
    for M in (1, 2, 3, 5):
        e2e[f"ensemble_over_separate_{M}"] = e2e["images_per_s"][f"ensemble_{M}"]["median"] / e2e["images_per_s"][f"separate_{M}"]["median"]
    staged.events = []
    t0 = time.perf_counter()
    staged(images)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    stages = {}
    for name, e0, e1 in staged.events:
        stages[name] = stages.get(name, 0.0) + e0.elapsed_time(e1)
    staged.events = None
    e2e["stages_ms_ensemble_3"] = dict(stages, wall=wall * 1e3)
    out["end_to_end"] = e2e
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
