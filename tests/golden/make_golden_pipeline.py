"""Generate fixture set G18 (letterbox / de-letterbox of seg_main.py) under tests/golden/ by running the REFERENCE's own
PngNormalizer and PngDenormalizer classes (utils/png_normalize.py, utils/png_denormalize.py: they import only PIL).

    python tests/golden/make_golden_pipeline.py PATH_TO_REFERENCE_CHECKOUT

Inputs are seeded synthetic grey PNGs (smooth shapes plus mild noise, so the files stay small) at 700x300, 300x700,
512x384 (the horizontal pass is skipped), 512x512 (PIL's copy path), 100x37 (upscale) and 1000x999; masks are synthetic
{0,128,255} and {0,255} 512x512 canvases.  One g18_<W>x<H>.npz per size: image, normalized, mask3, mask2, denorm3,
denorm2, plus the sizes JSON text the normalizer wrote (sizes_json)."""
import json
import os
import sys
import tempfile

import numpy as np
from PIL import Image

SIZES = [(700, 300), (300, 700), (512, 384), (512, 512), (100, 37), (1000, 999)]
OUT = os.path.dirname(os.path.abspath(__file__))


def synth_image(W, H, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    img = 40 + 60 * xx / max(W - 1, 1) + 30 * yy / max(H - 1, 1)
    for _ in range(4):
        cx, cy = rng.uniform(0, W), rng.uniform(0, H)
        rx, ry = rng.uniform(0.1, 0.4) * W, rng.uniform(0.1, 0.4) * H
        img += rng.uniform(40, 120) * ((((xx - cx) / rx) ** 2 + ((yy - cy) / ry) ** 2) < 1)
    img += rng.integers(0, 4, (H, W))
    return np.clip(img, 0, 255).astype(np.uint8)


def synth_mask(seed, levels):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:512, 0:512].astype(np.float64)
    m = np.full((512, 512), levels[0], np.uint8)
    for lv in levels[1:]:
        for _ in range(2):
            cx, cy, r = rng.uniform(100, 412), rng.uniform(100, 412), rng.uniform(40, 150)
            m[((xx - cx) ** 2 + (yy - cy) ** 2) < r * r] = lv
    return m


def main(ref):
    sys.path.insert(0, os.path.join(ref, "utils"))
    from png_normalize import PngNormalizer          # the reference's classes, imported at run time (nothing is copied)
    from png_denormalize import PngDenormalizer
    with tempfile.TemporaryDirectory() as td:
        d = {k: os.path.join(td, k) for k in ("in", "norm", "m3", "m2", "d3", "d2")}
        for p in d.values():
            os.makedirs(p)
        imgs = {}
        for i, (W, H) in enumerate(SIZES):
            name = f"g18_{W}x{H}.png"
            imgs[name] = synth_image(W, H, 100 + i)
            Image.fromarray(imgs[name], mode="L").save(os.path.join(d["in"], name))
            Image.fromarray(synth_mask(200 + i, (0, 128, 255)), mode="L").save(os.path.join(d["m3"], name))
            Image.fromarray(synth_mask(300 + i, (0, 255)), mode="L").save(os.path.join(d["m2"], name))
        PngNormalizer(d["in"], d["norm"]).normalize()
        sizes_path = os.path.join(d["norm"], "original_sizes.json")
        PngDenormalizer(d["m3"], d["d3"], sizes_path).denormalize()
        PngDenormalizer(d["m2"], d["d2"], sizes_path).denormalize()
        sizes_text = open(sizes_path, encoding="utf-8").read()
        rd = lambda k, n: np.asarray(Image.open(os.path.join(d[k], n)))
        for name, img in imgs.items():
            path = os.path.join(OUT, name.replace(".png", ".npz"))
            np.savez_compressed(path, image=img, normalized=rd("norm", name), mask3=rd("m3", name), mask2=rd("m2", name),
                                denorm3=rd("d3", name), denorm2=rd("d2", name), sizes_json=np.array(sizes_text))
            print(path, os.path.getsize(path), json.loads(sizes_text)[name])


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
