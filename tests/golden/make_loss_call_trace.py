#!/usr/bin/env python3
"""Record what the loss side asks of the C ABI: every LIB.call launch of a set of small loss cases (value and backward), and
sha256 digests of every term and of the logits' gradient.  tests/test_gpu_loss_trace.py replays the same cases (it imports CASES /
run_case from this file) and requires the record of tests/golden/loss_call_trace_parent.json, row for row.

The record's format, `recording`, `digest`, `dump` and the `merge` rule are those of make_ops_call_trace.py beside this file.
The losses are driven through the package's public names only (seg_loss with its options, surface_loss / surface_distance_map,
focal_tversky_loss, distill_loss, dice_coeff / dice_loss, boundary_loss), so the same file records at any commit that has them.
Needs an MI355X.  To renew the fixture, at the commit whose behaviour is to be kept:

    python tests/golden/make_loss_call_trace.py record run1.json
    python tests/golden/make_loss_call_trace.py record run2.json
    python tests/golden/make_loss_call_trace.py merge run1.json run2.json tests/golden/loss_call_trace_parent.json

The shapes are the smallest that reach each branch of the launch code the loss kernels share.  Their first pass leaves one row of
partial sums per block of 2048 pixels, at most 1024 rows; the column sum behind it is one workgroup of 256 threads; the gradient
kernels run a flat grid capped at 4096 blocks of 256 threads:

    2 x 24 x 40      1 920 pixels     one partial row
    3 x 96 x 120     34 560 pixels    17 rows
    2 x 727 x 727    1 057 058 pixels 517 rows: above 256, the column sum takes a second sweep; above 4096 * 256 = 1 048 576
                                      pixels, the capped gradient grid goes round
(the 1024-row cap needs more than 2 097 152 pixels: tests/test_gpu_optional_loss_ops.py holds it)."""
import importlib.util
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

_spec = importlib.util.spec_from_file_location("make_ops_call_trace", os.path.join(HERE, "make_ops_call_trace.py"))
_ops_rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_ops_rec)
recording, digest, dump = _ops_rec.recording, _ops_rec.digest, _ops_rec.dump

SHAPES = {"s0": (2, 24, 40), "s1": (3, 96, 120), "big": (2, 727, 727)}
TEACHER = "teacher.pth"          # DistillConfig wants a path; seg_loss / distill_loss never open it
GAMMAS = (0.0, 1.0, 2.0, 1.5)    # the three multiplication forms of u^gamma and the exp2 one


def _identity(t):
    return t


def _inputs(shape, head, seed, dtype=torch.float32):
    """Logits [B,head,H,W] as a model returns them (a leaf that takes the gradient), the dataset's labels ({0,1,2} for the
    one-channel head, class ids otherwise) and a teacher's logits, on the device."""
    B, H, W = shape
    g = torch.Generator().manual_seed(1000 * seed + head)
    z = (3.0 * torch.randn(B, head, H, W, generator=g)).to(dtype)
    v = (3.0 * torch.randn(B, head, H, W, generator=g)).to(dtype)
    mk = torch.randint(0, 3 if head == 1 else head, (B, H, W), generator=g)
    dev = torch.device("cuda:0")
    return z.to(dev).requires_grad_(True), mk.to(dev), v.to(dev)


def _weights(head):
    return tuple(1.0 + 0.25 * i for i in range(2 if head == 1 else head))


def _surface_classes(head):
    return {1: None, 3: None, 4: (1, 2, 3), 8: (2, 5)}[head]


def _seg(res, tag, z, mk, head, **kw):
    """seg_loss + backward twice over: the single-process form, and with an identity reduction at world = 2 (the unfused,
    data-parallel launch sequence).  Every term and the logits' gradient join `res`."""
    import unet_amd
    for form, extra in (("one", {}), ("dp", {"reduce_sums": _identity, "world": 2})):
        z.grad = None
        terms = unet_amd.seg_loss(z, mk, head, **kw, **extra)
        terms["loss"].backward()
        for k, v in terms.items():
            res[f"{tag}.{form}.{k}"] = v.detach().clone()
        res[f"{tag}.{form}.grad"] = z.grad.clone()


def _distill(w=0.7):
    import unet_amd
    return unet_amd.DistillConfig(TEACHER, T=2.0, w=w)


def case_pair(shape, heads, seed=1):
    """The default loss: the BCE + Dice + boundary node (head 1), the CE + Dice node (2, 3, 8; head 3 once more with the
    boundary term on)."""
    res = {}
    for head in heads:
        z, mk, _ = _inputs(shape, head, seed)
        _seg(res, f"h{head}", z, mk, head)
        if head == 3:
            _seg(res, "h3.boundary", z, mk, head, boundary_weight=0.25)
        if head == 1:
            _seg(res, "h1.noboundary", z, mk, head, boundary_weight=0.0)
    return res


def case_focal(shape, heads, seed=2, gammas=GAMMAS):
    import unet_amd
    res = {}
    for head in heads:
        z, mk, _ = _inputs(shape, head, seed)
        for gamma in gammas:
            cfg = unet_amd.LossConfig(gamma=gamma, weights=_weights(head))
            _seg(res, f"h{head}.g{gamma}", z, mk, head, loss=cfg)
    return res


def case_surface(shape, heads, seed=3):
    res = {}
    for head in heads:
        z, mk, _ = _inputs(shape, head, seed)
        _seg(res, f"h{head}", z, mk, head, surface_weight=0.5, surface_classes=_surface_classes(head))
    return res


def case_distill(shape, heads, seed=4):
    res = {}
    for head in heads:
        z, mk, v = _inputs(shape, head, seed)
        _seg(res, f"h{head}", z, mk, head, distill=_distill(), teacher_logits=v)
    return res


def case_all_on(shape, heads=(1, 3), seed=5):
    """Every option at once, and bf16 logits (what the model returns under autocast) through the default node."""
    res = {}
    for head in heads:
        z, mk, v = _inputs(shape, head, seed)
        _seg(res, f"h{head}", z, mk, head, loss="focal=2", surface_weight=0.5, distill=_distill(), teacher_logits=v)
        z, mk, v = _inputs(shape, head, seed, torch.bfloat16)
        _seg(res, f"h{head}.bf16", z, mk, head)
        _seg(res, f"h{head}.bf16.all", z, mk, head, loss="focal=2", surface_weight=0.5, distill=_distill(0.25), teacher_logits=v)
    return res


def case_functions(shape, heads=(1, 3), seed=6):
    """The loss functions next to seg_loss, each with its backward where it has one."""
    import unet_amd
    res = {}

    def run(tag, fn, z):
        z.grad = None
        out = fn()
        out.backward()
        res[tag], res[tag + ".grad"] = out.detach().clone(), z.grad.clone()

    for head in heads:
        z, mk, v = _inputs(shape, head, seed)
        run(f"h{head}.surface", lambda: unet_amd.surface_loss(z, mk, head), z)
        run(f"h{head}.focal", lambda: unet_amd.focal_tversky_loss(z, mk, head, "focal=1.5,tversky=0.5/0.5"), z)
        run(f"h{head}.distill", lambda: unet_amd.distill_loss(z, v, head, _distill()), z)
        if head == 1:
            run("h1.squeezed.focal", lambda: unet_amd.focal_tversky_loss(z.squeeze(1), mk, 1, "focal=2"), z)
            res["h1.map"] = unet_amd.surface_distance_map(mk, (1,), binary=True)
            p, t = torch.sigmoid(z.squeeze(1)), (mk // 2).float()
            res["h1.boundary"] = unet_amd.boundary_loss(z.detach(), t, 51, 15.0)
        else:
            res[f"h{head}.map"] = unet_amd.surface_distance_map(mk[0], (0, 2))
            p = torch.softmax(z, dim=1)
            t = torch.nn.functional.one_hot(mk, head).permute(0, 3, 1, 2).float()
            res[f"h{head}.boundary"] = unet_amd.boundary_loss(z.detach(), mk.float(), 51, 7.0)
        run(f"h{head}.dice_loss", lambda: unet_amd.dice_loss(p, t, multiclass=head > 1), z)
        res[f"h{head}.dice_coeff"] = unet_amd.dice_coeff(p.detach().flatten(0, -3), t.flatten(0, -3)).clone()
    return res


def _small(name):
    s = SHAPES[name]
    return {f"pair.{name}": lambda: case_pair(s, (1, 2, 3, 8)),
            f"focal.{name}": lambda: case_focal(s, (1, 2, 3, 4, 8)),
            f"surface.{name}": lambda: case_surface(s, (1, 3, 4, 8)),
            f"distill.{name}": lambda: case_distill(s, (1, 2, 3, 4, 8)),
            f"all_on.{name}": lambda: case_all_on(s),
            f"functions.{name}": lambda: case_functions(s)}


CASES = {**_small("s0"), **_small("s1"),
         "pair.big": lambda: case_pair(SHAPES["big"], (1, 3)),
         "focal.big": lambda: case_focal(SHAPES["big"], (1, 3), gammas=(2.0, 1.5)),
         "surface.big": lambda: case_surface(SHAPES["big"], (1, 3)),
         "distill.big": lambda: case_distill(SHAPES["big"], (1, 3))}


def run_case(name):
    """-> (rows, {result name: sha256})"""
    rows = []
    with recording(rows):
        res = CASES[name]()
        torch.cuda.synchronize()
    return rows, {k: digest(v) for k, v in sorted(res.items()) if v is not None}


def main(argv):
    if argv[0] == "record":
        import time
        doc = {"extent": [list(s) for s in SHAPES.values()], "cases": {}}
        for name in CASES:
            t0 = time.time()
            rows, digests = run_case(name)
            doc["cases"][name] = {"digests": digests, "rows": rows}
            print(f"case {name}: {len(rows)} launches, {len(digests)} digests, {time.time() - t0:.1f} s", flush=True)
        dump(doc, argv[1])
    elif argv[0] == "merge":
        _ops_rec.main(argv)
    else:
        raise SystemExit(__doc__)


if __name__ == "__main__":
    main(sys.argv[1:])
