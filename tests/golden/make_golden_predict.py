"""Generate fixture G19 (file handling of predict.py, PNG dumps of evaluate.py) under tests/golden/ by running the
REFERENCE's own functions: predict.get_output_path, predict.process_directory (on a tiny tree this script builds),
predict.mask_to_image, and evaluate.evaluate(..., epoch_pred_dir=...) on the CPU with a stub network, for the binary and
the 3-class branch, with and without post-processing.

    python tests/golden/make_golden_predict.py PATH_TO_REFERENCE_CHECKOUT

The reference imports cv2 (utils/post_process.py) and matplotlib (utils/utils.py); stand-in modules are put into
sys.modules before the import, and utils.post_process.postprocess_mask is replaced by this repository's scipy restatement
(oracle/post_process_ref.py).  The fixture therefore pins file names, batch counters and grey codings, NOT OpenCV; its
metadata says so.  Nothing of the reference is copied: its functions are imported and run, their results recorded."""
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch
from PIL import Image

OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))

TREE = ["a.png", "b.PNG", "c.jpg", "d.JPEG", "e.jpeg", "notes.txt", "f.png.bak", "g.bmp", "sub/a.png", "sub/h.Jpg",
        "sub/deeper/i.png", "sub/deeper/readme.md", "png", "j.tiff"]
PATH_CASES = [(None, "imgs/a.png"), (None, "/abs/dir/b.jpg"), (None, "c.jpeg"), ("out", "imgs/a.png"), ("out", "imgs/sub/a.png"),
              ("out/deep", "x/y/z.tar.png"), (None, "x/y/z.tar.png"), ("out", "noext"), (None, "dir.d/e.PNG")]


class Stub(torch.nn.Module):
    """Logits decided by the input's intensity (0 / 0.5 / 1 -> class 0 / 1 / 2; binary: 1 -> foreground)."""

    def __init__(self, n_classes):
        super().__init__()
        self.n_classes = n_classes

    def forward(self, x):
        if self.n_classes == 1:
            return (x - 0.75) * 8.0
        return torch.cat([0.25 - x, 0.2 - (x - 0.5).abs(), x - 0.75], dim=1) * 8.0


def batches(seed):
    """Two batches of two 160x160 items: a disc of class 2 large enough to survive min_area = 15000, class-1 patches, noise
    specks that the opening removes, and one item without any foreground."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:160, 0:160]
    out = []
    for k in range(2):
        imgs, masks = [], []
        for i in range(2):
            cls = np.zeros((160, 160), np.int64)
            cls[20:60, 10 + 30 * i:150] = 1
            if (k, i) != (1, 1):
                cls[(xx - 80 - 3 * k) ** 2 + (yy - 82 + 2 * i) ** 2 < 74 ** 2] = 2
                cls[(xx - 90) ** 2 + (yy - 80) ** 2 < 9 ** 2] = 1                    # a hole the post-processing fills
            for _ in range(12):
                y, x = rng.integers(0, 158, 2)
                cls[y:y + 2, x:x + 1] = 2
            imgs.append(cls.astype(np.float32)[None] / 2.0)
            masks.append(np.roll(cls, 3, axis=1))
        out.append({"image": torch.from_numpy(np.stack(imgs)), "mask": torch.from_numpy(np.stack(masks))})
    return out


def main(ref):
    sys.path.insert(0, ref)
    sys.path.insert(0, ROOT)
    from oracle import post_process_ref
    cv2 = types.ModuleType("cv2")
    plt = types.ModuleType("matplotlib.pyplot")
    mpl = types.ModuleType("matplotlib")
    mpl.pyplot = plt
    sys.modules.update({"cv2": cv2, "matplotlib": mpl, "matplotlib.pyplot": plt})
    import utils.post_process as ref_post                                   # the reference's module, cv2 stand-in inside
    ref_post.postprocess_mask = post_process_ref.postprocess_mask
    import predict as ref_predict
    import evaluate as ref_evaluate
    ref_evaluate.postprocess_mask = post_process_ref.postprocess_mask
    rec = {}
    meta = {"reference_functions": ["predict.get_output_path", "predict.process_directory", "predict.mask_to_image",
                                    "evaluate.evaluate"],
            "postprocess_mask": "oracle/post_process_ref.py (scipy restatement) injected for cv2: the fixture pins file names, "
                                "batch counters and grey codings, not OpenCV",
            "stand_in_modules": ["cv2", "matplotlib", "matplotlib.pyplot"], "tree": TREE, "path_cases": PATH_CASES}
    with tempfile.TemporaryDirectory() as td:
        cwd = os.getcwd()
        os.chdir(td)
        try:
            # get_output_path (it creates args.output as a side effect)
            paths = []
            for output, f in PATH_CASES:
                paths.append(ref_predict.get_output_path(types.SimpleNamespace(output=output), f))
            meta["output_paths"] = paths
            meta["output_dirs_created"] = sorted(d for d in ("out", "out/deep") if os.path.isdir(d))
            # process_directory
            for rel in TREE:
                p = os.path.join("tree", rel)
                os.makedirs(os.path.dirname(p), exist_ok=True)
                open(p, "wb").close()
            found = ref_predict.process_directory("tree")
            meta["walk_found_sorted"] = sorted(os.path.relpath(f, "tree") for f in found)
            meta["walk_empty"] = ref_predict.process_directory("out")
            # mask_to_image on every code, as uint8 and as the int64 predict_img returns
            codes = np.arange(256).reshape(16, 16)
            rec["mask_to_image_u8"] = np.asarray(ref_predict.mask_to_image(codes.astype(np.uint8)))
            rec["mask_to_image_i64"] = np.asarray(ref_predict.mask_to_image(codes.astype(np.int64)))
            # evaluate's dumps
            for n_classes in (3, 1):
                for postprocess in (True, False):
                    tag = f"eval_c{n_classes}_{'pp' if postprocess else 'raw'}"
                    net = Stub(n_classes)
                    data = batches(19)
                    with torch.no_grad():
                        logits = [net(b["image"]) for b in data]
                    if n_classes == 1:
                        raw = [(torch.sigmoid(l.squeeze(1)) > 0.5).numpy().astype(np.uint8) for l in logits]
                        post = [np.stack([post_process_ref.postprocess_mask(m * 255) // 255 for m in r]) for r in raw]
                    else:
                        raw = [l.argmax(dim=1).numpy().astype(np.uint8) for l in logits]
                        post = [np.stack([post_process_ref.postprocess_mask(m) for m in r]) for r in raw]
                    d = os.path.join("pred", tag)
                    os.makedirs(d)
                    scores = ref_evaluate.evaluate(net, [dict(b) for b in data], torch.device("cpu"), False, d, postprocess)
                    names = []
                    for root, _, files in os.walk(d):
                        for f in files:
                            rel = os.path.relpath(os.path.join(root, f), d)
                            names.append(rel)
                            rec[f"{tag}.file.{rel}"] = np.asarray(Image.open(os.path.join(root, f)))
                    meta[tag] = {"files": sorted(names), "dirs": sorted(x for x in os.listdir(d) if os.path.isdir(os.path.join(d, x))),
                                 "scores": [float(s) for s in scores]}
                    rec[f"{tag}.raw"] = np.stack(raw)
                    rec[f"{tag}.post"] = np.stack(post)
        finally:
            os.chdir(cwd)
    rec["meta_json"] = np.array(json.dumps(meta))
    path = os.path.join(OUT, "g19_predict_cli.npz")
    np.savez_compressed(path, **rec)
    print(path, os.path.getsize(path))
    print(json.dumps(meta, indent=1)[:3000])


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
