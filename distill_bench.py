"""Benchmark of knowledge distillation (csrc/distill_loss.hip, utils/distill.py).  Prints one JSON line and writes it to
profiles/distill_bench.json.

    python distill_bench.py [--iters 10] [--passes 3] [--batch 8] [--size 512] [--steps 20] [--warmup 5] [--rounds 3]
                            [--out profiles/distill_bench.json]

  - device time (events around 10 back-to-back calls, warm-up, median with min / max of --passes x --iters samples) of
      uh_distill_sums + uh_distill_finish   (one pass over both logit tensors, 8 C bytes a pixel, + column sums + finish)
      uh_distill_grad                       (one pass, reads 8 C and writes 4 C bytes a pixel)
    at 8 x 512^2 x 3 (softmax head) and 8 x 512^2 x 1 (one-channel head), beside the CE / BCE + Dice launches of the default
    loss and beside a device-to-device copy that moves the same bytes (half read, half written); the legs alternate in one
    process (--passes times a, b, c, ...).  `over_copy` is the ratio of the medians;
  - the teacher's forward alone: UNet(1,3,bilinear) in bf16 at batch 8, Distiller.teacher_logits (the batch-invariant eval
    forward), device time per call;
  - train-step images/s of a UNet_T and a UNet_S student (bf16, batch 8) with the option off and on against that teacher, one
    process, the steppers alternating, --rounds windows of --steps steps each after --warmup steps, a device synchronise closing
    every window.  `on_predicted_img_s` is the off step plus the teacher's forward alone: what the step with the option costs
    beyond it is the kd launches and the host's share."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def device_samples(fn, iters, warmup=3, inner=10):
    """Milliseconds per call: `iters` samples of `inner` back-to-back calls between two events."""
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
        ts.append(e0.elapsed_time(e1) / inner)
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10, help="samples per launch and pass")
    ap.add_argument("--passes", type=int, default=3, help="alternations of the legs")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--steps", type=int, default=20, help="train steps per timed window")
    ap.add_argument("--warmup", type=int, default=5, help="untimed steps per stepper before the first window")
    ap.add_argument("--rounds", type=int, default=3, help="off / on windows, alternated")
    ap.add_argument("--temperature", type=float, default=2.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distill_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("distill_bench.py needs an MI355X")
    import unet_amd
    from unet_amd._lib import LIB
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B, H, W = args.batch, args.size, args.size
    n = B * H * W
    T = float(args.temperature)
    out = {"metric": "distill_device_ms", "device": torch.cuda.get_device_name(0), "iters": args.iters, "passes": args.passes,
           "batch": B, "size": f"{H}x{W}", "temperature": T}
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(0)
    labels = torch.randint(0, 3, (B, H, W), generator=g).to(dev)
    ws = torch.empty(LIB.query("uh_loss_ws_bytes", n), dtype=torch.uint8, device=dev)

    # ---- the kd launches beside the default loss's and beside a copy of their own bytes
    kern = {}
    for name, ncls in (("softmax_8x3", 3), ("one_channel_8x1", 1)):
        dims = (B, H, W) if ncls == 1 else (B, H, W, ncls)
        student = (torch.randn(dims, generator=g) * 3).to(dev)
        teacher = (torch.randn(dims, generator=g) * 3).to(dev)
        dl = torch.empty_like(student)
        s_kd = torch.empty(LIB.query("uh_distill_nsums"), dtype=torch.float32, device=dev)
        o_kd = torch.empty(3, dtype=torch.float32, device=dev)
        s_old = torch.empty(4 if ncls == 1 else 1 + 3 * ncls, dtype=torch.float32, device=dev)
        zp, vp, mp, dp = student.data_ptr(), teacher.data_ptr(), labels.data_ptr(), dl.data_ptr()
        bytes_sums, bytes_grad = n * 8 * ncls, n * 12 * ncls
        # a copy moves its size twice (read + write): sources of half the pass's bytes
        c_sums = (torch.empty(bytes_sums // 2, dtype=torch.uint8, device=dev), torch.empty(bytes_sums // 2, dtype=torch.uint8, device=dev))
        c_grad = (torch.empty(bytes_grad // 2, dtype=torch.uint8, device=dev), torch.empty(bytes_grad // 2, dtype=torch.uint8, device=dev))

        def kd_sums():
            LIB.call("uh_distill_sums", zp, vp, n, ncls, T, s_kd.data_ptr(), ws.data_ptr(), ws.numel(), st)
            LIB.call("uh_distill_finish", s_kd.data_ptr(), float(n), T, 1.0, o_kd.data_ptr(), st)

        def kd_grad():
            LIB.call("uh_distill_grad", zp, vp, n, ncls, float(n), T, 1.0, None, dp, st)

        def old_sums():
            if ncls == 1:
                LIB.call("uh_bce_dice_sums", zp, mp, 2, None, n, s_old.data_ptr(), ws.data_ptr(), ws.numel(), st)
            else:
                LIB.call("uh_ce_dice_sums", zp, mp, n, ncls, s_old.data_ptr(), ws.data_ptr(), ws.numel(), st)

        def old_grad():
            if ncls == 1:
                LIB.call("uh_bce_dice_grad", zp, mp, 2, None, n, s_old.data_ptr(), float(n), 1.0, 1.0, None, dp, st)
            else:
                LIB.call("uh_ce_dice_grad", zp, mp, n, ncls, s_old.data_ptr(), float(n), 1.0, 1.0, None, dp, st)

        launches = {"kd_sums_finish": kd_sums, "copy_sums_bytes": lambda: c_sums[1].copy_(c_sums[0]), "default_sums": old_sums,
                    "kd_grad": kd_grad, "copy_grad_bytes": lambda: c_grad[1].copy_(c_grad[0]), "default_grad": old_grad}
        old_sums()                                                    # the default gradient launch reads its sums
        samples = {k: [] for k in launches}
        for _ in range(args.passes):
            for k, fn in launches.items():
                samples[k] += device_samples(fn, args.iters)
        res = {k + "_ms": spread(v) for k, v in samples.items()}
        res["bytes_sums"], res["bytes_grad"] = bytes_sums, bytes_grad
        for what, leg in (("sums", "kd_sums_finish"), ("grad", "kd_grad")):
            med = res[leg + "_ms"]["median"]
            res[f"kd_{what}_over_copy"] = med / res[f"copy_{what}_bytes_ms"]["median"]
            res[f"kd_{what}_over_default"] = med / res[f"default_{what}_ms"]["median"]
            res[f"kd_{what}_GB_s"] = res[f"bytes_{what}"] / med / 1e6
        kern[name] = res
    out["kernel"] = kern

    # ---- the teacher's forward alone, then the train step with the option off and on, alternating in one process
    images = torch.rand(B, 1, H, W, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
    with tempfile.TemporaryDirectory() as tmp:
        torch.manual_seed(1)
        path = unet_amd.save_checkpoint(unet_amd.UNet(1, 3, bilinear=True), os.path.join(tmp, "teacher.pth"))
        distiller = unet_amd.Distiller(unet_amd.DistillConfig(path, arch="UNet", T=T), 1, 3, dev, amp=True)
    fwd = []
    for _ in range(args.passes):
        fwd += device_samples(lambda: distiller.teacher_logits(images), args.iters, inner=3)
    out["teacher_forward"] = {"model": "UNet(1,3,bilinear=True)", "dtype": "bf16", "batch": B, "size": f"{H}x{W}", "ms": spread(fwd)}

    def window(stepper, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            stepper.step(images, labels)
        torch.cuda.synchronize()
        return B * steps / (time.perf_counter() - t0)

    out["train_step"] = {}
    for arch in ("UNet_T", "UNet_S"):
        steppers = {}
        for name, distill in (("off", None), ("on", distiller)):
            torch.manual_seed(0)
            model = getattr(unet_amd, arch)(1, 3, bilinear=True).to(memory_format=torch.channels_last).to(dev)
            steppers[name] = unet_amd.TrainStepper(model, amp=True, distill=distill)
        for s in steppers.values():
            window(s, args.warmup)
        rates = {"off": [], "on": []}
        for _ in range(args.rounds):
            for name in ("off", "on"):
                rates[name].append(window(steppers[name], args.steps))
        step = {"student": f"{arch}(1,3,bilinear=True)", "teacher": "UNet(1,3,bilinear=True)", "dtype": "bf16", "batch": B,
                "size": f"{H}x{W}", "steps_per_window": args.steps, "rounds": args.rounds,
                "off_img_s": spread(rates["off"]), "off_img_s_all": [round(r, 1) for r in rates["off"]],
                "on_img_s": spread(rates["on"]), "on_img_s_all": [round(r, 1) for r in rates["on"]]}
        off_ms, on_ms = 1e3 * B / step["off_img_s"]["median"], 1e3 * B / step["on_img_s"]["median"]
        step["off_step_ms"], step["on_step_ms"] = off_ms, on_ms
        step["on_predicted_img_s"] = 1e3 * B / (off_ms + out["teacher_forward"]["ms"]["median"])
        step["on_beyond_teacher_ms"] = on_ms - off_ms - out["teacher_forward"]["ms"]["median"]
        step["off_spread"] = (step["off_img_s"]["max"] - step["off_img_s"]["min"]) / step["off_img_s"]["median"]
        out["train_step"][arch] = step
        for s in steppers.values():
            s.close()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
