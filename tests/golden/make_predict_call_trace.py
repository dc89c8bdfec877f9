#!/usr/bin/env python3
"""Record what the inference routes ask of the C ABI and of themselves: every LIB.call launch of BatchPredictor (plain,
batch-invariant, test-time augmentation, tiled, an ensemble untiled and tiled), evaluate() of one network and of an ensemble, and
ContourPipeline on small seeded cases, the stage names their
`events` collect, `graph_replays`, `launch_lengths`, and sha256 digests of everything they return.
tests/test_gpu_predict_trace.py replays the same cases (it imports CASES / run_case from this file) and requires the record of
tests/golden/predict_call_trace_parent.json, row for row.

The rows are those of tests/golden/make_ops_call_trace.py (its `recording` is reused: pointers as 0 / 1, the stream as 0 / 1 for
the stream that was current when the case began / another one, so warm-up and capture of a graph show).  The cases call public
API only, so this file runs unchanged on both sides of a change to the host code.  Needs an MI355X.  To renew the fixture, at
the commit whose behaviour is to be kept:

    python tests/golden/make_predict_call_trace.py record run1.json
    python tests/golden/make_predict_call_trace.py record run2.json
    python tests/golden/make_predict_call_trace.py merge run1.json run2.json tests/golden/predict_call_trace_parent.json

`merge` refuses two runs whose launch records, stage names, replay counts or launch lengths differ and keeps only the digests
both runs agree on (the rest are named under "dropped_digests").  The files hold every different launch once (`dump`); `load`
spells the record out again, launch by launch."""
import hashlib
import importlib.util
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

_spec = importlib.util.spec_from_file_location("make_ops_call_trace", os.path.join(HERE, "make_ops_call_trace.py"))
ops_trace = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ops_trace)
recording = ops_trace.recording

MIN_AREA = 40                      # the default 15000 would blank every mask of these sizes


def digest(v):
    if isinstance(v, torch.Tensor):
        v = v.detach().float().cpu().numpy() if v.dtype == torch.bfloat16 else v.detach().cpu().numpy()
    if isinstance(v, np.ndarray):
        v = np.ascontiguousarray(v)
        return hashlib.sha256(f"{v.dtype}{v.shape}".encode() + v.tobytes()).hexdigest()
    return hashlib.sha256(json.dumps(v, sort_keys=True).encode()).hexdigest()


def _image(seed, H, W):
    """A seeded uint8 image with structure at several scales, so that the classes of a random network vary."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    img = 90 + 70 * np.sin(yy / 5.0 + seed) * np.cos(xx / 7.0) + 40 * ((yy - H / 3) ** 2 + (xx - W / 2) ** 2 < (min(H, W) / 3) ** 2)
    return np.clip(img + rng.normal(0, 12, (H, W)), 2, 255).astype(np.uint8)


def _mask(seed, H, W):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    r = ((yy - H * rng.uniform(0.4, 0.6)) / (H * 0.35)) ** 2 + ((xx - W * rng.uniform(0.4, 0.6)) / (W * 0.35)) ** 2
    return np.where(r < 0.5, 2, np.where(r < 1.0, 1, 0)).astype(np.int64)


def _model(classes=3, seed=3):
    """UNet(1, classes) with seeded weights, non-trivial BatchNorm running statistics and a head bias that lets the classes
    compete.  Built before the recording starts."""
    import unet_amd
    dev = torch.device("cuda:0")
    torch.manual_seed(seed)
    model = unet_amd.UNet(1, classes)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.2)
                m.running_mean.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(m.bias.shape, generator=g) + 0.5)
        model = model.to(dev).eval()
        x = torch.from_numpy(_image(0, 48, 64).astype(np.float32) / 255.0)[None, None].to(dev)
        y = model(x).float()
        centre = y.mean(dim=(0, 2, 3)) if classes > 1 else (y.amax(dim=(0, 2, 3)) + y.amin(dim=(0, 2, 3))) / 2
        model.outc.conv.bias.sub_(centre)
    torch.cuda.synchronize()
    return model


def _images(counts, seed):
    """[(H, W), n] -> the images in a fixed shuffled order."""
    sizes = [s for s, n in counts for _ in range(n)]
    images = [_image(10 * seed + k, H, W) for k, (H, W) in enumerate(sizes)]
    return [images[i] for i in np.random.default_rng(seed).permutation(len(images))]


def _lengths(p, sizes):
    return {f"{H}x{W}": list(p.launch_lengths(H, W)) for H, W in sizes}


def _stages(obj):
    return [e[0] for e in obj.events]


def _levels(res):
    """How many different bytes every uint8 result holds: a record of constant masks would compare little."""
    return [int(len(np.unique(a))) for _, a in sorted(res.items()) if a.dtype == np.uint8]


# A case is (prepare, run): prepare() builds the model and the inputs, run(state) is what is recorded -> (results, facts).
# ------------------------------------------------------------------------------------------ BatchPredictor
P1_IMAGES = [((48, 64), 5), ((32, 32), 3), ((64, 48), 1)]


def _plain(batch_invariant):
    def prepare():
        return _model(), _images(P1_IMAGES, 1)

    def run(state):
        import unet_amd
        from unet_amd.predict import plan_batches
        model, images = state
        p = unet_amd.BatchPredictor(model, batch=4, min_area=MIN_AREA, batch_invariant=batch_invariant)
        p.events = []
        first, second = p(images), p(images)                              # the second call replays graphs
        res = {f"first.{i}": a for i, a in enumerate(first)}
        res.update({f"second.{i}": a for i, a in enumerate(second)})
        res.update({f"classes.{i}": a for i, a in enumerate(p.classes(images))})
        planned = [len(m) for _, m in plan_batches([im.shape for im in images], 4)]
        return res, {"events": _stages(p), "graph_replays": p.graph_replays, "planned_batches": planned, "levels": _levels(res),
                     "launch_lengths": _lengths(p, [s for s, _ in P1_IMAGES])}
    return prepare, run


def _tta():
    def prepare():
        return _model(), _images([((48, 48), 2), ((32, 48), 2)], 3)

    def run(state):
        import unet_amd
        model, images = state
        p = unet_amd.BatchPredictor(model, batch=8, min_area=MIN_AREA, batch_invariant=True, tta="d4")
        p.events = []
        res = {}
        for name, fn in (("call", p), ("classes", p.classes), ("probabilities", p.probabilities)):
            res.update({f"{name}.{i}": a for i, a in enumerate(fn(images))})
        raw = unet_amd.BatchPredictor(model, batch=8, postprocess=False, batch_invariant=True, tta="d4")
        res.update({f"raw.{i}": a for i, a in enumerate(raw.classes(images))})
        return res, {"events": _stages(p), "graph_replays": p.graph_replays, "levels": _levels(res),
                     "launch_lengths": _lengths(p, [(48, 48), (32, 48), (48, 32)])}
    return prepare, run


def _tiled():
    def prepare():
        return _model(), [_image(40 + k, H, W) for k, (H, W) in enumerate([(48, 80), (64, 64), (32, 32), (48, 80)])]

    def run(state):
        import unet_amd
        model, images = state
        res, facts = {}, {}
        for tag, tta in (("plain", None), ("flips", "flips")):
            p = unet_amd.BatchPredictor(model, batch=4, min_area=MIN_AREA, tile="32,overlap=8", tta=tta)
            p.events = []
            res.update({f"{tag}.call.{i}": a for i, a in enumerate(p(images))})
            res.update({f"{tag}.probabilities.{i}": a for i, a in enumerate(p.probabilities(images))})
            facts[tag] = {"events": _stages(p), "graph_replays": p.graph_replays, "launch_lengths": _lengths(p, [(32, 32)])}
        facts["levels"] = _levels(res)
        return res, facts
    return prepare, run


ENSEMBLE_SEEDS, ENSEMBLE_WEIGHTS = (3, 5), [2, 1]


def _members(classes=3):
    import unet_amd
    return unet_amd.Ensemble([_model(classes, seed=s) for s in ENSEMBLE_SEEDS], weights=ENSEMBLE_WEIGHTS)


def _ensemble():
    def prepare():
        return _members(), _images([((48, 48), 2), ((32, 48), 3)], 5)

    def run(state):
        import unet_amd
        ens, images = state
        res, facts = {}, {}
        for tag, tta in (("plain", None), ("d4", "d4")):
            p = unet_amd.BatchPredictor(ens, batch=4, min_area=MIN_AREA, batch_invariant=True, tta=tta)
            p.events = []
            first, second = p(images), p(images)                          # the second call replays graphs
            masks, confidence = p.masks_and_confidence(images)
            for name, got in (("first", first), ("second", second), ("classes", p.classes(images)),
                              ("probabilities", p.probabilities(images)), ("masks", masks), ("confidence", confidence)):
                res.update({f"{tag}.{name}.{i}": a for i, a in enumerate(got)})
            facts[tag] = {"events": _stages(p), "graph_replays": p.graph_replays,
                          "launch_lengths": _lengths(p, [(48, 48), (32, 48), (48, 32)])}
        facts["levels"] = _levels(res)
        return res, facts
    return prepare, run


def _ensemble_tiled():
    def prepare():
        return _members(), _tiled()[0]()[1]

    def run(state):
        import unet_amd
        ens, images = state
        res, facts = {}, {}
        for tag, tta in (("plain", None), ("flips", "flips")):
            p = unet_amd.BatchPredictor(ens, batch=4, min_area=MIN_AREA, tile="32,overlap=8", tta=tta)
            p.events = []
            for name, fn in (("call", p), ("probabilities", p.probabilities), ("confidence", p.confidence)):
                res.update({f"{tag}.{name}.{i}": a for i, a in enumerate(fn(images))})
            facts[tag] = {"events": _stages(p), "graph_replays": p.graph_replays, "launch_lengths": _lengths(p, [(32, 32)])}
        facts["levels"] = _levels(res)
        return res, facts
    return prepare, run


# ------------------------------------------------------------------------------------------ evaluate
def _evaluate(build=_model):
    """`build(classes)`: the network (or the ensemble) that is scored."""
    def prepare():
        images = [_image(60 + k, 48, 64) for k in range(4)]
        masks = [_mask(70 + k, 48, 64) for k in range(4)]
        loader = [{"image": torch.from_numpy(np.stack([(i.astype(np.float32) / np.float32(255.0))[None] for i in images[s:s + 2]])),
                   "mask": torch.from_numpy(np.stack(masks[s:s + 2]))} for s in (0, 2)]
        return {3: build(3), 1: build(1)}, loader

    def run(state):
        import unet_amd
        models, loader = state
        dev = torch.device("cuda:0")
        res = {}
        for classes, model in models.items():
            for tta in (None, "rot4"):
                for tile in (None, "32,overlap=8"):
                    for post in (True, False):
                        got = unet_amd.evaluate(model, loader, dev, True, postprocess=post, tta=tta, tile=tile)
                        res[f"nc{classes}.tta_{tta}.tile_{tile is not None}.post_{post}"] = torch.stack([v.float() for v in got])
        return res, {}
    return prepare, run


# ------------------------------------------------------------------------------------------ ContourPipeline
def _raws(n, H, W, seed):
    """CT-like 16-bit scans: air around an elliptic body (~1000), an inner organ and a bright bone."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.empty((n, H, W), np.uint16)
    for i in range(n):
        img = rng.normal(30, 8, (H, W))
        cx, cy = W * rng.uniform(0.4, 0.6), H * rng.uniform(0.4, 0.6)
        rx, ry = W * rng.uniform(0.25, 0.4), H * rng.uniform(0.25, 0.4)
        body = ((xx - cx) / rx) ** 2 + ((yy - cy) / ry) ** 2 < 1
        img[body] = 1000 + rng.normal(0, 10, (H, W))[body]
        img[((xx - cx) / (rx / 3)) ** 2 + ((yy - cy - ry / 3) / (ry / 4)) ** 2 < 1] += 600
        out[i] = np.clip(img, 0, 65535).astype(np.uint16)
    return out


def _pipeline():
    def prepare():
        return _model(), _raws(3, 120, 160, 5)

    def run(state):
        import unet_amd
        model, raws = state
        res, facts = {}, {}
        for tag, invariant in (("default", False), ("invariant", True)):
            pipe = unet_amd.ContourPipeline(model, 160, 120, 400, 1040, batch=2, min_area=MIN_AREA, batch_invariant=invariant)
            pipe.events = []
            for part, s in (("full", slice(0, 2)), ("partial", slice(2, 3))):
                out = pipe.run_batch(raws[s])
                for k in ("window", "canvas", "logits", "argmax", "classes", "grey"):
                    res[f"{tag}.{part}.{k}"] = out[k].clone()
                res[f"{tag}.{part}.contours"] = [[np.asarray(c).tolist() for c in cs] for cs in out["contours"]]
            res[f"{tag}.json"] = pipe(raws)                                # the full batch replays its graph
            facts[tag] = {"events": _stages(pipe)}
        return res, facts
    return prepare, run


CASES = {"p1": _plain(False), "p2": _plain(True), "p3": _tta(), "p4": _tiled(), "p5": _ensemble(), "p6": _ensemble_tiled(),
         "e1": _evaluate(), "e2": _evaluate(_members), "s1": _pipeline()}


def run_case(name):
    """-> {"rows": launches, "digests": {result name: sha256}, "facts": stage names, replay counts, launch lengths}"""
    prepare, run = CASES[name]
    state = prepare()
    rows = []
    with recording(rows):
        res, facts = run(state)
        torch.cuda.synchronize()
    return {"rows": rows, "digests": {k: digest(v) for k, v in sorted(res.items())}, "facts": facts}


LAYERS = ("uh_conv", "uh_pack_", "uh_maxpool", "uh_upsample", "uh_bn_", "uh_sa_")    # what a network forward launches


def dump(doc, path):
    """Lossless and compact: every different launch once ("rows", one per line), every different run of network-layer launches
    once ("blocks": a forward of one shape), and per case the sequence "launches": n >= 0 is rows[n], n < 0 is blocks[-n - 1]."""
    rows, blocks, cases = {}, {}, {}
    for name, case in doc["cases"].items():
        seq, run = [], []
        for r in case["rows"] + [None]:
            if r is not None and r[0].startswith(LAYERS):
                run.append(rows.setdefault(json.dumps(r, separators=(",", ":")), len(rows)))
                continue
            if run:
                seq.append(-1 - blocks.setdefault(tuple(run), len(blocks)))
                run = []
            if r is not None:
                seq.append(rows.setdefault(json.dumps(r, separators=(",", ":")), len(rows)))
        cases[name] = '"%s": {"facts": %s,\n"digests": %s,\n"launches": %s}' % (
            name, json.dumps(case["facts"], separators=(",", ":")), json.dumps(case["digests"], separators=(",", ":")),
            json.dumps(seq, separators=(",", ":")))
    with open(path, "w") as f:
        f.write('{"dropped_digests": %s, "rows": [\n%s\n],\n' % (json.dumps(doc.get("dropped_digests", [])), ",\n".join(rows)))
        f.write('"blocks": [\n%s\n],\n' % ",\n".join(json.dumps(list(b), separators=(",", ":")) for b in blocks))
        f.write('"cases": {\n%s\n}}\n' % ",\n".join(cases.values()))


def load(path):
    """The document `dump` wrote, with every case's "rows" spelled out again."""
    with open(path) as f:
        doc = json.load(f)
    rows, blocks = doc.pop("rows"), doc.pop("blocks")
    for case in doc["cases"].values():
        case["rows"] = [rows[i] for n in case.pop("launches") for i in ([n] if n >= 0 else blocks[-n - 1])]
    return doc


def main(argv):
    if argv[0] == "record":
        import time
        doc = {"cases": {}}
        for name in CASES:
            t0 = time.time()
            doc["cases"][name] = run_case(name)
            print(f"case {name}: {len(doc['cases'][name]['rows'])} launches, {len(doc['cases'][name]['digests'])} digests, "
                  f"{time.time() - t0:.1f} s", flush=True)
        dump(doc, argv[1])
    elif argv[0] == "merge":
        a, b = (load(p) for p in argv[1:3])
        dropped = []
        for name, ca in a["cases"].items():
            cb = b["cases"][name]
            if ca["rows"] != cb["rows"] or ca["facts"] != cb["facts"]:
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
