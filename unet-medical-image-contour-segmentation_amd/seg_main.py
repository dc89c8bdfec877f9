"""The reference's shipped pipeline, seg_main.py: 16-bit RAW scans -> body-contour polygons in LabelMe JSON, with every
pixel stage on the device and one stream from the RAW upload to the contour points.

    stage 1  utils/raw2png.py         window / level                      uh_window_u16
    stage 2  utils/png_normalize.py   letterbox to 512 x 512 (LANCZOS)     uh_resample_lanczos_u8
    stage 3  predict.py               predict_img + postprocess_mask       eval forward (GraphedForward for full batches),
                                                                           uh_argmax_classes, uh_postprocess_masks
    stage 4  utils/png_denormalize.py crop + LANCZOS to the original size  uh_resample_lanczos_u8 (class -> grey table)
    stage 5  utils/mask2polygon.py    external contours -> JSON            uh_contours_count / uh_contours_emit

    ContourPipeline(model, width, height, window_width, window_length, batch=8, postprocess=True, batch_invariant=False)
    python -m unet_amd.seg_main --input-raw DIR -o ROOT --width W --height H -ww WW -wl WL -m model.pth [--keep-stages]
                                [--batch-invariant]

The reference chains five scripts by subprocess with a PNG encode / decode between them; the intermediate images here
stay on the device unless --keep-stages asks for the reference's directories 1-4 (pixel-identical, the PNG encoders
differ).  The _contour_overlay.png drawing of mask2polygon.py and TorchScript .pt models are not covered."""
from __future__ import annotations

import argparse
import json
import logging
import os
import sys
from typing import Dict, List, Optional

import numpy as np
import torch

from . import ops
from .inference import GraphedForward, eval_forward, timed_stage
from .utils.mask2polygon import contour_json, external_contours, write_json
from .utils.png_denormalize import CLASS_TO_GREY
from .utils.png_normalize import TARGET, _IDENTITY, device_lut, letterbox_geometry, resample_into, resample_plan
from .utils.post_process import _run as _postprocess_run
from .utils.raw2png import read_raw, window_bounds, window_level
from ._lib import LIB

class ContourPipeline:
    """`pipe(raws)` -> one LabelMe dict (or None: no contour) per RAW image.  raws: uint16 [B,H,W] (numpy or a GPU tensor;
    int16 bits accepted).  `pipe.run_batch(raws)` also returns the intermediate device tensors ("logits" is the forward's
    output buffer, which a graphed batch overwrites on its next run).
    `batch_invariant=False`: every launch takes its own kernels, so logits (by ~1e-4; a tie may flip a class) depend on
    `batch`.  True: the forward runs under ops.plan_images(1) and an image's logits are, bit for bit, those it gets alone."""

    def __init__(self, model: torch.nn.Module, width: int, height: int, window_width: int, window_length: int,
                 batch: int = 8, postprocess: bool = True, device=None, amp: bool = True, min_area: int = 15000,
                 morph_kernel_size: int = 3, batch_invariant: bool = False):
        window_bounds(window_width, window_length)                      # refuses WW < 2
        self.geometry = letterbox_geometry(width, height)                # refuses an empty letterbox
        if batch < 1:
            raise ValueError("batch must be >= 1")
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if self.device.type != "cuda":
            raise RuntimeError("ContourPipeline needs an MI355X: the HIP path has no CPU fallback")
        self.model = model.to(self.device).eval()
        self.width, self.height = int(width), int(height)
        self.ww, self.wl = int(window_width), int(window_length)
        self.batch, self.postprocess, self.amp = int(batch), bool(postprocess), amp
        self.min_area, self.ksize = int(min_area), int(morph_kernel_size)
        self.batch_invariant = bool(batch_invariant)
        nw, nh, px, py = self.geometry
        self._plan_in = resample_plan(self.width, self.height, nw, nh, self.device)
        self._plan_out = resample_plan(nw, nh, self.width, self.height, self.device)
        self._lut_id = device_lut(_IDENTITY, self.device)
        self._lut_cls = device_lut(CLASS_TO_GREY, self.device)
        self._graph: Optional[GraphedForward] = None
        self._flags = torch.empty(self.batch, dtype=torch.int32, device=self.device)
        self.events = None                    # set to a list to collect (stage, start event, end event) per batch

    # ---------------------------------------------------------------- stages
    def _mark(self, name, fn, *a):
        return timed_stage(self.events, name, fn, *a)

    def _to_device(self, raws):
        if isinstance(raws, np.ndarray):
            a = np.ascontiguousarray(raws)
            if a.dtype not in (np.uint16, np.int16):
                raise RuntimeError(f"RAW batch must be 16-bit, got {a.dtype}")
            t = torch.from_numpy(a.view(np.int16))
            t = (t.pin_memory() if torch.cuda.is_available() else t).to(self.device, non_blocking=True)
        else:
            t = raws
            ops._require_gpu(t, "raws")
        if t.dim() == 2:
            t = t.unsqueeze(0)
        if tuple(t.shape[1:]) != (self.height, self.width):
            raise RuntimeError(f"RAW batch is {tuple(t.shape[1:])}, the pipeline was built for {(self.height, self.width)}")
        return t.contiguous()

    def _letterbox(self, img):
        nw, nh, px, py = self.geometry
        out = torch.empty(img.shape[0], TARGET, TARGET, dtype=torch.uint8, device=self.device)
        return resample_into(img, (0, 0, self.width, self.height), self._plan_in, self._lut_id, out, (px, py))

    def _forward(self, canvas):
        B = canvas.shape[0]
        x = torch.empty(B, 1, TARGET, TARGET, dtype=torch.float32, device=self.device, memory_format=torch.channels_last)
        flags = self._flags if B <= self._flags.numel() else torch.empty(B, dtype=torch.int32, device=self.device)
        # predict.py:19 preprocess: float32 / 255 when the image holds a byte > 1 (decided per image), channels_last
        LIB.call("uh_batch_prepare", canvas.data_ptr(), 1, None, None, 0, x.data_ptr(), 1, None, flags.data_ptr(), B, TARGET,
                 TARGET, 0, ops._stream())
        plan = 1 if self.batch_invariant else 0
        if B == self.batch:
            if self._graph is None:
                self._graph = GraphedForward(self.model, x, amp=self.amp, plan_images=plan)
            return self._graph(x)
        return eval_forward(self.model, x, self.amp, plan)

    def _unletterbox(self, classes):
        nw, nh, px, py = self.geometry
        out = torch.empty(classes.shape[0], self.height, self.width, dtype=torch.uint8, device=self.device)
        return resample_into(classes, (px, py, nw, nh), self._plan_out, self._lut_cls, out, (0, 0))

    def run_batch(self, raws) -> Dict[str, object]:
        raw = self._to_device(raws)
        win = self._mark("window", window_level, raw, self.ww, self.wl)
        canvas = self._mark("letterbox", self._letterbox, win)
        logits = self._mark("forward", self._forward, canvas)
        idx = self._mark("argmax", ops.argmax_classes, logits)
        classes = idx.to(torch.uint8)
        if self.postprocess:
            classes = self._mark("postprocess", _postprocess_run, classes, self.min_area, self.ksize)
        grey = self._mark("unletterbox", self._unletterbox, classes)
        contours = self._mark("contours", external_contours, grey)
        return {"window": win, "canvas": canvas, "logits": logits, "argmax": idx, "classes": classes, "grey": grey, "contours": contours}

    def __call__(self, raws, stems: Optional[List[str]] = None):
        res = []
        n = raws.shape[0] if raws.ndim == 3 else 1
        stems = stems or [str(i) for i in range(n)]
        for s in range(0, n, self.batch):
            out = self.run_batch(raws[s:s + self.batch])
            for stem, cont in zip(stems[s:s + self.batch], out["contours"]):
                res.append(contour_json(cont, stem, self.width, self.height))
        return res


# -------------------------------------------------------------------- CLI (seg_main.py:169-230)
def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="RAW -> contour JSON pipeline on the MI355X (seg_main.py)")
    p.add_argument("--input-raw", required=True, help="RAW file or directory of .raw files")
    p.add_argument("--output-root", "-o", default="seg_results", help="output root directory")
    p.add_argument("--width", type=int, required=True, help="RAW width")
    p.add_argument("--height", type=int, required=True, help="RAW height")
    p.add_argument("--window-width", "-ww", type=int, required=True, help="window width")
    p.add_argument("--window-length", "-wl", type=int, required=True, help="window level")
    p.add_argument("--model", "-m", required=True, help="model weights (.pth state_dict, UNet(1, 3, bilinear=False))")
    p.add_argument("--batch", type=int, default=8, help="images per device batch")
    p.add_argument("--keep-stages", action="store_true", help="also write the reference's directories 1-4")
    p.add_argument("--batch-invariant", action="store_true",
                   help="pin every layer to the kernel one image gets: the results do not depend on --batch")
    return p


def list_raws(path: str) -> List[str]:
    if os.path.isfile(path):
        return [path] if path.lower().endswith(".raw") else []
    return sorted(os.path.join(path, f) for f in os.listdir(path)
                  if os.path.isfile(os.path.join(path, f)) and f.lower().endswith(".raw"))


def _save_png(path, arr):
    from PIL import Image
    Image.fromarray(np.ascontiguousarray(arr), mode="L").save(path)


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(asctime)s - %(levelname)s - %(message)s")
    from .checkpoint import load_checkpoint
    from .unet import UNet
    root = args.output_root
    dirs = {k: os.path.join(root, v) for k, v in (("raw_png", "1_raw_png"), ("normalized_png", "2_normalized_png"),
                                                  ("pred_masks", "3_pred_masks"), ("denormalized_masks", "4_denormalized_masks"),
                                                  ("json_results", "5_json_results"))}
    for k, d in dirs.items():
        if args.keep_stages or k == "json_results":
            os.makedirs(d, exist_ok=True)
    model = UNet(n_channels=1, n_classes=3, bilinear=False)
    load_checkpoint(model, args.model)                                  # mask_values dropped (predict.py:106-109)
    pipe = ContourPipeline(model, args.width, args.height, args.window_width, args.window_length, batch=args.batch,
                           batch_invariant=args.batch_invariant)
    stems, raws = [], []
    for f in list_raws(args.input_raw):
        try:
            raws.append(read_raw(f, args.width, args.height))
            stems.append(os.path.splitext(os.path.basename(f))[0])
        except ValueError as e:
            logging.error("skipped: %s", e)                           # raw2png.py:899-901: the file fails, the run goes on
    if not raws:
        logging.error("no RAW file of the stated size under %s", args.input_raw)
        return 1
    sizes, written = {}, 0
    batch = np.stack(raws)
    for s in range(0, len(raws), pipe.batch):
        out = pipe.run_batch(batch[s:s + pipe.batch])
        if args.keep_stages:
            host = {k: out[k].cpu().numpy() for k in ("window", "canvas", "classes", "grey")}
        for i, stem in enumerate(stems[s:s + pipe.batch]):
            d = contour_json(out["contours"][i], stem, args.width, args.height)
            if args.keep_stages:
                _save_png(os.path.join(dirs["raw_png"], stem + ".png"), host["window"][i])
                _save_png(os.path.join(dirs["normalized_png"], stem + ".png"), host["canvas"][i])
                _save_png(os.path.join(dirs["pred_masks"], stem + ".png"), CLASS_TO_GREY[host["classes"][i]])
                _save_png(os.path.join(dirs["denormalized_masks"], stem + ".png"), host["grey"][i])
                sizes[stem + ".png"] = {"width": args.width, "height": args.height}
            if d is None:
                logging.warning("no contour: %s", stem)               # mask2polygon.py:331-333
                continue
            write_json(os.path.join(dirs["json_results"], stem + ".json"), d)
            written += 1
    if args.keep_stages:
        with open(os.path.join(dirs["normalized_png"], "original_sizes.json"), "w", encoding="utf-8") as f:
            json.dump(sizes, f, ensure_ascii=False, indent=2)
    logging.info("%d of %d images written to %s", written, len(stems), dirs["json_results"])
    return 0


if __name__ == "__main__":
    sys.exit(main())
