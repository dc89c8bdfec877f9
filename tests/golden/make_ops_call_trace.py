#!/usr/bin/env python3
"""Record what the conv + BatchNorm + ReLU nodes of ops.py ask of the C ABI: every LIB.call launch of a set of small
forward/backward cases, and sha256 digests of their results.  tests/test_gpu_ops_trace.py replays the same cases (it imports
CASES / run_case from this file) and requires the record of tests/golden/ops_call_trace_parent.json, row for row.

One row per launch: the entry-point name, then its arguments typed by LIB.protos -- integers and floats as they are, every
pointer as 0 / 1 (null / non-null), the stream as 0 / 1 (the stream that was current when the case began / another one, so
backward-weights on the side stream shows).  Needs an MI355X.  To renew the fixture, at the commit whose behaviour is to be
kept:

    python tests/golden/make_ops_call_trace.py record run1.json
    python tests/golden/make_ops_call_trace.py record run2.json
    python tests/golden/make_ops_call_trace.py merge run1.json run2.json tests/golden/ops_call_trace_parent.json

`merge` refuses two runs whose launch records differ and keeps only the digests both runs agree on (the rest are named
under "dropped_digests")."""
import contextlib
import hashlib
import json
import os
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# The whole network at batch 2 (test_gpu_fused_tails.py runs it at 64 x 96).  The parent's record at 32 x 48 reaches every branch the
# test names -- all three fused tails, the fused BatchNorm-backward sums, the narrow and the plan entry points -- so the smaller one it is.
EXTENT = (32, 48)


@contextlib.contextmanager
def recording(rows):
    """Wrap LIB.call for the length of a case."""
    from unet_amd._lib import LIB
    main = torch.cuda.current_stream().cuda_stream or 0
    had = LIB.__dict__.get("call")
    inner = LIB.call

    def call(name, *args):
        row = [name]
        for t, a in zip(LIB.protos[name][1], args):
            if t == "ptr":
                row.append(1 if a else 0)
            elif t == "uh_stream":
                row.append(0 if (a or 0) == main else 1)
            else:
                row.append(float(a) if t in ("float", "double") else int(a))
        rows.append(row)
        return inner(name, *args)

    LIB.call = call
    try:
        yield
    finally:
        if had is None:
            del LIB.call
        else:
            LIB.call = had


def _batch(B, C, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, C, H, W, generator=g), torch.randint(0, 3, (B, H, W), generator=g)


def _buffers(model):
    return {"buf." + k: v for k, v in model.state_dict().items() if "running" in k or "num_batches" in k}


def _stepper_case(H, W, freeze=False, sync_bn=False):
    """(a) / (f) / (h): the bilinear full-width UNet, channels_last weights, bf16, two TrainStepper steps."""
    import unet_amd
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = unet_amd.UNet(1, 1, bilinear=True).to(memory_format=torch.channels_last).to(dev)
    if freeze:
        model.down2.maxpool_conv[1].double_conv[3].weight.requires_grad_(False)
        model.up1.conv.double_conv[1].weight.requires_grad_(False)
    im, mk = _batch(2, 1, H, W, 11)
    im, mk = im.to(dev), mk.to(dev)
    stepper = unet_amd.TrainStepper(model, amp=True, wgrad_stream=True, sync_bn=sync_bn)
    try:
        assert (stepper.sync_bn is not None) == sync_bn
        for _ in range(2):
            t = stepper.step(im, mk, global_batch=2 if sync_bn else None)
        torch.cuda.synchronize()
        out = {"logits": t["logits"], "loss": t["loss"].detach(), "flat_g": stepper.optimizer.flat_g.clone(),
               "flat_p": stepper.optimizer.flat_p.clone()}
        out.update({k: v.clone() for k, v in _buffers(model).items()})
        return out
    finally:
        stepper.close()


def case_a(H, W):
    return _stepper_case(H, W)


def case_f(H, W):
    return _stepper_case(H, W, freeze=True)


def case_h(H, W):
    """(a) under SyncBN with a one-rank process group (UH_DP_FORCE_SYNC=1), initialised in-process from a file store."""
    import torch.distributed as dist
    assert not dist.is_initialized()
    before = os.environ.get("UH_DP_FORCE_SYNC")
    os.environ["UH_DP_FORCE_SYNC"] = "1"
    with tempfile.TemporaryDirectory() as tmp:
        dist.init_process_group("gloo", store=dist.FileStore(os.path.join(tmp, "store"), 1), rank=0, world_size=1)
        try:
            return _stepper_case(H, W, sync_bn=True)
        finally:
            dist.destroy_process_group()
            if before is None:
                os.environ.pop("UH_DP_FORCE_SYNC", None)
            else:
                os.environ["UH_DP_FORCE_SYNC"] = before


def _plain_case(model, x, cot, amp):
    """One forward + plain backward() in training mode."""
    dev = torch.device("cuda:0")
    model = model.to(dev).train()
    x, cot = x.to(dev), cot.to(dev)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
        out = model(x)
    loss = (out.float() * cot).sum()
    loss.backward()
    torch.cuda.synchronize()
    res = {"logits": out.detach(), "loss": loss.detach()}
    res.update({"grad." + k: p.grad for k, p in model.named_parameters()})
    res.update(_buffers(model))
    return res


def _convt_case(H, W, mode):
    import unet_amd
    from unet_amd import ops
    torch.manual_seed(1)
    model = unet_amd.UNet(3, 2, bilinear=False)
    g = torch.Generator().manual_seed(12)
    x, cot = torch.randn(2, 3, H, W, generator=g), torch.randn(2, 2, H, W, generator=g)
    with ops.step_state(fp32_mode=mode):
        return _plain_case(model, x, cot, False)


def case_b(H, W):
    return _convt_case(H, W, "exact")


def case_c(H, W):
    return _convt_case(H, W, "bf16x3")


def _tiny_case(H, W, amp):
    import unet_amd
    torch.manual_seed(2)
    model = unet_amd.UNet_T(3, 2, bilinear=True)
    g = torch.Generator().manual_seed(13)
    x, cot = torch.randn(2, 3, H, W, generator=g), torch.randn(2, 2, H, W, generator=g)
    return _plain_case(model, x, cot, amp)


def case_d_bf16(H, W):
    return _tiny_case(H, W, True)


def case_d_fp32(H, W):
    return _tiny_case(H, W, False)


def case_e(H, W):
    from unet_amd import ops
    before, ops.NARROW_IO = ops.NARROW_IO, False
    try:
        return _tiny_case(H, W, True)
    finally:
        ops.NARROW_IO = before


def case_g(H, W):
    """Eval forward at batch 3, with and without plan_images(1): (a)'s model in bf16, UNet_T in bf16 and fp32."""
    import unet_amd
    from unet_amd import ops
    dev = torch.device("cuda:0")
    res = {}
    x1, _ = _batch(3, 1, H, W, 14)
    x3 = torch.randn(3, 3, H, W, generator=torch.Generator().manual_seed(15))
    torch.manual_seed(0)
    full = unet_amd.UNet(1, 1, bilinear=True).to(memory_format=torch.channels_last).to(dev).eval()
    torch.manual_seed(2)
    tiny = unet_amd.UNet_T(3, 2, bilinear=True).to(dev).eval()
    for name, model, x, amp in (("unet_bf16", full, x1, True), ("unet_t_bf16", tiny, x3, True), ("unet_t_fp32", tiny, x3, False)):
        for plan in (0, 1):
            with torch.no_grad(), ops.plan_images(plan), torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
                res[f"{name}.plan{plan}"] = model(x.to(dev))
    torch.cuda.synchronize()
    return res


CASES = {"a": case_a, "b": case_b, "c": case_c, "d_bf16": case_d_bf16, "d_fp32": case_d_fp32, "e": case_e, "f": case_f,
         "g": case_g, "h": case_h}


def digest(t):
    raw = t.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()
    return hashlib.sha256(raw).hexdigest()


def run_case(name, extent=EXTENT):
    """-> (rows, {result name: sha256})"""
    from unet_amd import ops
    rows = []
    assert ops.STEP == ops.StepState(), "a case must start from the default step state: nothing may be left installed"
    with recording(rows):
        res = CASES[name](*extent)
    assert ops.STEP == ops.StepState(), f"case {name} left a step state installed"
    return rows, {k: digest(v) for k, v in sorted(res.items()) if v is not None}


def dump(doc, path):
    """Compact: one line per launch."""
    with open(path, "w") as f:
        f.write('{"extent": %s, "dropped_digests": %s, "cases": {\n' % (json.dumps(doc["extent"]), json.dumps(doc.get("dropped_digests", []))))
        for i, (name, case) in enumerate(doc["cases"].items()):
            f.write('"%s": {"digests": %s, "rows": [\n' % (name, json.dumps(case["digests"], separators=(",", ":"))))
            f.write(",\n".join(json.dumps(r, separators=(",", ":")) for r in case["rows"]))
            f.write("\n]}%s\n" % ("," if i + 1 < len(doc["cases"]) else ""))
        f.write("}}\n")


def main(argv):
    if argv[0] == "record":
        import time
        extent = (int(argv[2]), int(argv[3])) if len(argv) > 2 else EXTENT
        doc = {"extent": list(extent), "cases": {}}
        for name in CASES:
            t0 = time.time()
            rows, digests = run_case(name, extent)
            doc["cases"][name] = {"digests": digests, "rows": rows}
            print(f"case {name}: {len(rows)} launches, {len(digests)} digests, {time.time() - t0:.1f} s", flush=True)
        dump(doc, argv[1])
    elif argv[0] == "merge":
        a, b = (json.load(open(p)) for p in argv[1:3])
        dropped = []
        for name, ca in a["cases"].items():
            cb = b["cases"][name]
            if ca["rows"] != cb["rows"]:
                raise SystemExit(f"case {name}: the two runs launched different records")
            for k in list(ca["digests"]):
                if ca["digests"][k] != cb["digests"].get(k):
                    dropped.append(f"{name}:{k}")
                    del ca["digests"][k]
        a["dropped_digests"] = dropped
        dump(a, argv[3])
        print(f"merged: {sum(len(c['rows']) for c in a['cases'].values())} launches, dropped digests: {dropped}")
    else:
        raise SystemExit(__doc__)


if __name__ == "__main__":
    main(sys.argv[1:])
