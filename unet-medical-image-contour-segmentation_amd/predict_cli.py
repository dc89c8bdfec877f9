"""The reference's prediction command line, /root/reference/predict.py:31-152, on the HIP path:

    python -m unet_amd.predict -m model.pth [MEMBER ...] -i FILE_OR_DIR [-o OUT] [-n] [-v] [--no-postprocess]
                               [--arch UNet] [-c 3] [--bilinear] [--no-amp] [-b 8] [--workers 8] [--no-batch-invariant]
                               [--tta [hflip|flips|rot4|d4]] [--tile [SIZE[,overlap=N]]] [--confidence-dir DIR]

Every image is predicted at its own size (scale 1).  The images of a folder are decoded by a thread pool, grouped by size,
run through BatchPredictor in batches (prepare, eval forward, classes, post-processing and grey coding on the device, one
upload and one download per batch) and encoded to PNG by the same pool while the next batch runs.  The forward is
batch-invariant (BatchPredictor(batch_invariant=True)): a batch is one launch and every image gets the bits it gets alone;
--no-batch-invariant cuts the batches instead, to the same files.  --tta averages the prediction over the views of a mode
(utils/tta.py; a bare --tta means d4): -b stays the number of images per forward launch, views included.  --tile predicts
every image as overlapping tiles of one shape (utils/tiling.py; a bare --tile means 512,overlap=128): the images are grouped
by tile shape instead of size, the tiles of a group share full forward launches of -b tiles, and the overlap is blended.
Several -m items, or one with a key or a glob (PATH[,arch=A][,w=N], utils/ensemble.py), make an ensemble: the members'
probabilities are added as integers with their weights before the argmax; --arch is the architecture of a member without
arch=, and bilinear vs transposed-conv upsampling is read off each checkpoint.  --confidence-dir DIR also writes
<stem>_conf.png, floor(255 max / sum) of the summed probabilities per pixel.  One plain -m x.pth runs the one-model path.

Reference behaviour that is kept, awkward parts included:
  - predict.py:33-38  the flags -m, -i (both required), -o, -v, -n, and -p, a store_true whose default is already True;
                      --no-postprocess is the way to turn it off here;
  - predict.py:61-68  a directory is walked recursively (os.walk order) for .png / .jpg / .jpeg, case-insensitive;
  - predict.py:76-84  a missing input path or a directory without images: an error message and exit status 1;
  - predict.py:93-98  .pt (TorchScript) models: REFUSED here with exit status 1, no TorchScript path exists on this port;
  - predict.py:99-109 .pth: UNet(n_channels=1, n_classes=3, bilinear=False) by default (--arch / --classes / --bilinear
                      select another network), a `mask_values` key is dropped before load_state_dict;
  - predict.py:110-116 any other suffix, or a checkpoint that does not load: exit status 1;
  - predict.py:122    every image is opened and converted to "L";
  - predict.py:43-49  without -o the mask is written next to the input as <stem>.png, which overwrites a PNG input; with
                      -o every mask goes flat into that directory as <stem>.png, so equal stems of different sub-directories
                      collide and the later one in discovery order wins.  Files are written in discovery order whatever
                      order the size groups finished in, so the winner is the reference's;
  - predict.py:146-147 a file that fails is logged with its name and skipped, the others are written, exit status 0;
  - predict.py:141-144 --viz needs matplotlib, imported lazily: where it is absent the command says so and exits 1 before
                      any prediction is made.  The figure is a plain image / mask pair, not utils.plot_img_and_mask.
There is no CPU fallback: without a GPU the command exits with status 2 (after the argument, input and model checks)."""
from __future__ import annotations

import argparse
import logging
import os
import sys
from collections import deque
from concurrent.futures import ThreadPoolExecutor
from typing import List, Optional

import numpy as np

ARCHS = ("UNet", "UNet_S", "UNet_T", "UNet_SA")
EXTENSIONS = (".png", ".jpg", ".jpeg")


class _MembersAction(argparse.Action):
    """-m SPEC [SPEC ...]: `members` holds the specs; `model` stays the string it has always been for one -m item and is the
    list for several."""

    def __call__(self, parser, namespace, values, option_string=None):
        from .utils.ensemble import parse_member_spec
        for v in values:
            try:
                parse_member_spec(v)
            except ValueError as e:
                parser.error(f"argument {option_string}: {e}")
        namespace.members = list(values)
        namespace.model = values[0] if len(values) == 1 else list(values)


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Predict multi-class masks for an image or a directory of images")
    # the reference's flags, short forms and defaults (predict.py:31-40)
    p.add_argument("--model", "-m", required=True, nargs="+", action=_MembersAction, metavar="MODEL",
                   help="Model weights (.pth state_dict); several items, each PATH[,arch=A][,w=N] (PATH may be a glob), make "
                        "an ensemble")
    p.add_argument("--input", "-i", required=True, help="Input image file or directory (walked recursively)")
    p.add_argument("--output", "-o", help="Output directory (default: <stem>.png next to each input, overwriting a PNG input)")
    p.add_argument("--viz", "-v", action="store_true", default=False, help="Show each result (needs matplotlib)")
    p.add_argument("--no-save", "-n", action="store_true", default=False, help="Do not write the masks")
    p.add_argument("--postprocess", "-p", action="store_true", default=True, help="Apply post-processing (the default)")
    # additions; the defaults are what predict.py hard-codes
    p.add_argument("--no-postprocess", dest="postprocess", action="store_false", help="Write the raw argmax classes")
    p.add_argument("--arch", choices=ARCHS, default="UNet", help="Network (predict.py:107 builds UNet)")
    p.add_argument("--classes", "-c", type=int, default=3, help="Number of classes")
    p.add_argument("--bilinear", action="store_true", default=False, help="Bilinear upsampling")
    p.add_argument("--no-amp", dest="amp", action="store_false", default=True, help="Run the forward in fp32 (default: bf16 autocast)")
    p.add_argument("--batch-size", "-b", dest="batch_size", type=int, default=8, help="Images of one size per device batch")
    p.add_argument("--workers", type=int, default=8, help="Decode / encode threads")
    p.add_argument("--batch-invariant", dest="batch_invariant", action="store_true", default=True,
                   help="Pin every layer of a batch to the kernel one image gets, so that full batches run as one launch "
                        "(the default; the masks are the same either way)")
    p.add_argument("--no-batch-invariant", dest="batch_invariant", action="store_false",
                   help="Cut every batch into launches in which each layer gets one image's kernel by itself")
    from .utils.tta import DEFAULT_MODE, MODES
    p.add_argument("--tta", nargs="?", const=DEFAULT_MODE, default=None, choices=tuple(MODES),
                   help="Test-time augmentation: average the prediction over these views (a bare --tta: d4; default: off)")
    from .utils.tiling import DEFAULT_SPEC, parse_tile_spec

    def tile_spec(text):
        try:
            return parse_tile_spec(text).spec
        except ValueError as e:
            raise argparse.ArgumentTypeError(str(e))

    p.add_argument("--tile", nargs="?", const=DEFAULT_SPEC, default=None, type=tile_spec, metavar="SPEC",
                   help="Sliding-window prediction: cut every image into tiles of SIZE[,overlap=N] pixels and blend the overlap "
                        f"(a bare --tile: {DEFAULT_SPEC}; default: off)")
    p.add_argument("--confidence-dir", default=None, metavar="DIR",
                   help="Ensembles: also write <stem>_conf.png there, floor(255 max / sum) of the summed probabilities")
    return p


def get_args(argv=None) -> argparse.Namespace:
    return build_parser().parse_args(argv)


def output_path(output: Optional[str], input_file: str) -> str:
    """predict.py:43-49."""
    base_name = os.path.splitext(os.path.basename(input_file))[0]
    if output is None:
        return os.path.join(os.path.dirname(input_file), f"{base_name}.png")
    return os.path.join(output, f"{base_name}.png")


def discover(input_dir: str) -> List[str]:
    """predict.py:61-68: every .png / .jpg / .jpeg under input_dir, in os.walk order."""
    image_files = []
    for root, _, files in os.walk(input_dir):
        for file in files:
            if file.lower().endswith(EXTENSIONS):
                image_files.append(os.path.join(root, file))
    return image_files


def decode(path: str) -> np.ndarray:
    """predict.py:122: Image.open(path).convert('L'), as a uint8 [H,W] array."""
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("L"))


def _show(plt, path, img, grey):
    fig, ax = plt.subplots(1, 2)
    ax[0].set_title(os.path.basename(path))
    ax[0].imshow(img, cmap="gray")
    ax[1].set_title("mask")
    ax[1].imshow(grey, cmap="gray", vmin=0, vmax=255)
    plt.show()


def confidence_path(confidence_dir: str, input_file: str) -> str:
    return os.path.join(confidence_dir, os.path.splitext(os.path.basename(input_file))[0] + "_conf.png")


def run(predictor, files: List[str], output: Optional[str], save: bool, workers: int, show=None, window: Optional[int] = None,
        confidence_dir: Optional[str] = None):
    """Predicts `files` and writes the masks (and, with `confidence_dir`, an ensemble's confidence maps, from the same pass).
    -> (written paths in write order, failed input paths)."""
    from .predict import BatchPlanner
    from .utils.png_writer import OrderedPngWriter
    workers = max(1, int(workers))
    failed: List[str] = []
    planner = BatchPlanner(predictor.batch, window if window is not None else 16 * predictor.batch)
    tile = getattr(predictor, "tile", None)
    if tile is not None:
        from .utils.tiling import tile_shape
    held = {}
    with ThreadPoolExecutor(max_workers=workers, thread_name_prefix="predict-io") as pool:
        writer = OrderedPngWriter(pool=pool)
        conf_writer = OrderedPngWriter(pool=pool) if confidence_dir is not None else None

        def finish(members):
            imgs = [held.pop(i) for i in members]
            if conf_writer is not None:
                out, conf = predictor.masks_and_confidence(imgs)
                for k, i in enumerate(members):
                    conf_writer.submit(i, confidence_path(confidence_dir, files[i]), conf[k])
            else:
                out = predictor(imgs) if tile is not None else predictor.run_batch(imgs)     # (tiled: sizes are mixed)
            for k, i in enumerate(members):
                if save:
                    writer.submit(i, output_path(output, files[i]), out[k])
                else:
                    writer.skip(i)
                if show is not None:
                    show(files[i], imgs[k], out[k])

        ahead = max(2 * predictor.batch, 2 * workers)             # decodes in flight beyond the one being waited for
        pending = deque()
        nxt = 0
        for i in range(len(files)):
            while nxt < len(files) and len(pending) < ahead:
                pending.append(pool.submit(decode, files[nxt]))
                nxt += 1
            fut = pending.popleft()
            logging.info("Predicting image %s", files[i])
            try:
                img = fut.result()
            except Exception as e:                                # predict.py:146-147: logged with its name, the run goes on
                logging.error("Error while processing image %s: %s", files[i], e)
                failed.append(files[i])
                writer.skip(i)
                if conf_writer is not None:
                    conf_writer.skip(i)
                continue
            held[i] = img
            for _, members in planner.add(i, img.shape if tile is None else tile_shape(img.shape[0], img.shape[1], tile)):
                finish(members)
        for _, members in planner.flush():
            finish(members)
        written = writer.close()
        if conf_writer is not None:
            conf_writer.close()
    return written, failed


def main(argv=None) -> int:
    args = get_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(levelname)s: %(message)s")
    # input (predict.py:76-86)
    if os.path.isdir(args.input):
        in_files = discover(args.input)
        logging.info("Found %d image files in the directory", len(in_files))
        if not in_files:
            logging.error("No image file found in directory %s", args.input)
            return 1
    else:
        if not os.path.isfile(args.input):
            logging.error("Input file does not exist: %s", args.input)
            return 1
        in_files = [args.input]
    if args.batch_size < 1 or args.workers < 1:
        logging.error("--batch-size and --workers must be at least 1")
        return 1
    # model format (predict.py:93-116); checked before anything touches the device
    from .utils.ensemble import is_plain_single, parse_member_spec
    plain = is_plain_single(args.members)                             # one bare path: the one-model statements below
    for path in (parse_member_spec(m).path for m in args.members):
        if path.endswith(".pt"):
            logging.error("TorchScript models (.pt) are not supported: %s. This port runs .pth state_dicts through its HIP "
                          "kernels; there is no TorchScript path.", path)
            return 1
        if not path.endswith(".pth"):
            logging.error("Unsupported model format: %s (only .pth state_dicts are supported)", path)
            return 1
    plt = None
    if args.viz:
        try:
            import matplotlib.pyplot as plt                        # lazily: the package does not depend on it
        except ImportError:
            logging.error("--viz needs matplotlib, which is not installed; nothing was predicted")
            return 1
    import torch
    from .checkpoint import load_checkpoint
    from .train_cli import build_model
    try:
        if args.classes < 2:
            raise ValueError("predict.py takes argmax(dim=1): it needs a multi-class head (--classes >= 2); binary models "
                             "are scored and dumped by unet_amd.evaluate(..., epoch_pred_dir=...)")
        if plain:
            model = build_model(args.arch, args.classes, args.bilinear)
            load_checkpoint(model, args.model, device="cpu")          # mask_values dropped (predict.py:106-108)
            model.eval()
        else:
            from .utils.ensemble import Ensemble
            model = Ensemble.load(args.members, 1, args.classes, args.arch, "cpu")
        if args.confidence_dir is not None and len(getattr(model, "members", ())) < 2:
            raise ValueError("--confidence-dir needs an ensemble of two or more members")
    except Exception as e:
        logging.error("Failed to load the model %s: %s", args.model, e)
        return 1
    if plain:
        logging.info("Model loaded: %s, %d classes, %s upscaling", args.arch, args.classes,
                     "bilinear" if args.bilinear else "transposed conv")
    else:
        for r in model.records:
            logging.info("Member loaded: %s, %s, %s upscaling, weight %d", r["path"], r["arch"],
                         "bilinear" if r["bilinear"] else "transposed conv", r["weight"])
    if not torch.cuda.is_available():
        logging.error("predict: no GPU found. This port predicts on the MI355X through its HIP kernels and has no CPU path.")
        return 2
    from .predict import BatchPredictor
    device = torch.device("cuda", torch.cuda.current_device())
    logging.info("Using device %s", device)
    predictor = BatchPredictor(model, batch=args.batch_size, postprocess=args.postprocess, amp=args.amp, device=device,
                               batch_invariant=args.batch_invariant, tta=args.tta, tile=args.tile)
    if args.output is not None and not args.no_save:
        os.makedirs(args.output, exist_ok=True)                       # predict.py:48
    if args.confidence_dir is not None:
        os.makedirs(args.confidence_dir, exist_ok=True)
    show = (lambda path, img, grey: _show(plt, path, img, grey)) if plt is not None else None
    written, failed = run(predictor, in_files, args.output, not args.no_save, args.workers, show,
                          **({"confidence_dir": args.confidence_dir} if args.confidence_dir is not None else {}))
    logging.info("%d of %d images predicted, %d masks written%s", len(in_files) - len(failed), len(in_files), len(written),
                 f", {len(failed)} failed" if failed else "")
    return 0


if __name__ == "__main__":
    sys.exit(main())
