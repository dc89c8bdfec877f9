"""Scores a checkpoint on a data split without training (the reference reaches evaluate.py from its train loop only):

    python -m unet_amd.evaluate -m CKPT [MEMBER ...] --data-root DIR [--split val] [--arch UNet_S|UNet|UNet_T|UNet_SA] [-c 3] [--bilinear]
                                [-b 8] [-s 0.5] [--no-postprocess] [--no-amp] [--no-metrics] [--spacing 1.0]
                                [--pred-dir DIR] [--workers 8] [--json OUT] [--tta [hflip|flips|rot4|d4]]
                                [--tile [SIZE[,overlap=N]]]

It reads DIR/imgs/SPLIT and DIR/masks/SPLIT through the loader the train command builds for validation (BasicDataset with
its x4 quarter-turn augmentation, in order, drop_last=True: a trailing partial batch is not scored), loads the checkpoint
through checkpoint.py (a `mask_values` key is dropped) and runs evaluate().  It prints the Dice trio -- mean, post-processed,
minimum -- and, unless --no-metrics, the contour metrics HD95 / HD / ASSD / IoU of the raw and the post-processed masks
(utils/contour_metrics.py).  --spacing is the isotropic pixel pitch the distances are reported in.  --pred-dir writes the
predictions as grey-coded PNGs, as evaluate(epoch_pred_dir=...) does.  --json writes the set results and the per-image table.
--tta scores the prediction averaged over the views of a mode (utils/tta.py; a bare --tta means d4) and records it in --json.
--tile scores the sliding-window prediction (utils/tiling.py; a bare --tile means 512,overlap=128) and records its spec in --json.
Several -m items, or one with a key or a glob (PATH[,arch=A][,w=N], utils/ensemble.py), score the ensemble of those checkpoints;
--json then lists the members: path, arch, weight and the SHA-256 of the file.  One plain -m CKPT is scored as ever.
Exit status 1: a missing directory, an empty split (or one shorter than a batch), a checkpoint that does not load.  There is
no CPU fallback: without a GPU the command exits with status 2, after those checks."""
from __future__ import annotations

import argparse
import json
import logging
import math
import os
import sys

ARCHS = ("UNet_S", "UNet", "UNet_T", "UNet_SA")


def build_parser() -> argparse.ArgumentParser:
    from .predict_cli import _MembersAction
    p = argparse.ArgumentParser(description="Score a checkpoint on a validation split: Dice and contour-distance metrics")
    p.add_argument("--model", "-m", required=True, nargs="+", action=_MembersAction, metavar="CKPT",
                   help="Checkpoint (.pth state_dict); several items, each PATH[,arch=A][,w=N] (PATH may be a glob), are scored "
                        "as an ensemble")
    p.add_argument("--data-root", required=True, help="Directory holding imgs/SPLIT and masks/SPLIT")
    p.add_argument("--split", default="val", help="Sub-directory of imgs/ and masks/ that is scored")
    p.add_argument("--arch", choices=ARCHS, default="UNet_S", help="Network (the train command's default)")
    p.add_argument("--classes", "-c", type=int, default=3, help="Number of classes")
    p.add_argument("--bilinear", action="store_true", default=False, help="Bilinear upsampling")
    p.add_argument("--batch-size", "-b", dest="batch_size", type=int, default=8, help="Images per batch")
    p.add_argument("--scale", "-s", type=float, default=0.5, help="Downscaling factor of the images")
    p.add_argument("--no-postprocess", dest="postprocess", action="store_false", default=True, help="Score the raw masks only")
    p.add_argument("--no-amp", dest="amp", action="store_false", default=True, help="Run the forward in fp32 (default: bf16 autocast)")
    p.add_argument("--no-metrics", dest="metrics", action="store_false", default=True, help="Print the Dice trio only")
    p.add_argument("--spacing", type=float, default=1.0, help="Isotropic pixel pitch; multiplies the reported distances")
    p.add_argument("--pred-dir", default=None, help="Write the predictions there as grey-coded PNGs (default: off)")
    p.add_argument("--workers", type=int, default=8, help="Decode threads")
    p.add_argument("--json", default=None, metavar="OUT", help="Write the set results and the per-image table to OUT")
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
    return p


def get_args(argv=None) -> argparse.Namespace:
    return build_parser().parse_args(argv)


def _plain(v):
    """JSON without NaN literals: an undefined distance is null."""
    if isinstance(v, float):
        return v if math.isfinite(v) else None
    if isinstance(v, dict):
        return {k: _plain(x) for k, x in v.items()}
    if hasattr(v, "tolist"):
        return _plain(v.tolist())
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    return v


def report(dice, contour, tta=None, tile=None, members=None) -> dict:
    """What --json writes: {"dice": {...}, "metrics": {"raw": {...}, "post": {...}} or null}, "tta": mode under --tta,
    "tile": spec under --tile and "members": [{"path", "arch", "weight", "sha256"}] for an ensemble."""
    out = {"dice": {"mean": float(dice[0]), "postprocessed": float(dice[1]), "min": float(dice[2])}, "metrics": None}
    if members is not None:
        out["members"] = [{k: r[k] for k in ("path", "arch", "weight", "sha256")} for r in members]
    if tta is not None:
        out["tta"] = tta
    if tile is not None:
        out["tile"] = tile
    if contour is not None:
        out["metrics"] = _plain(contour)
    return out


def main(argv=None) -> int:
    args = get_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(levelname)s: %(message)s")
    images_dir = os.path.join(args.data_root, "imgs", args.split)
    masks_dir = os.path.join(args.data_root, "masks", args.split)
    for d in (images_dir, masks_dir):
        if not os.path.isdir(d):
            logging.error("Directory does not exist: %s", d)
            return 1
    if args.batch_size < 1 or args.workers < 1 or not 0 < args.scale <= 1 or not args.spacing > 0:
        logging.error("--batch-size and --workers must be at least 1, --scale in (0, 1], --spacing positive")
        return 1
    from .utils.ensemble import is_plain_single
    plain = is_plain_single(args.members)                             # one bare path: the one-model statements below
    if plain and not os.path.isfile(args.model):
        logging.error("Checkpoint does not exist: %s", args.model)
        return 1
    import torch
    from .checkpoint import load_checkpoint
    from .train_cli import build_model
    from .utils.data_loading import BasicDataset
    try:
        val_set = BasicDataset(images_dir, masks_dir, args.scale)
    except Exception as e:
        logging.error("No usable image / mask pair in %s: %s", images_dir, e)
        return 1
    if len(val_set) // args.batch_size == 0:
        logging.error("The split holds %d items, fewer than one batch of %d (drop_last=True): nothing to score", len(val_set),
                      args.batch_size)
        return 1
    try:
        if plain:
            model = build_model(args.arch, args.classes, args.bilinear)
            model = model.to(memory_format=torch.channels_last)
            load_checkpoint(model, args.model, device="cpu")
        else:
            from .utils.ensemble import Ensemble
            model = Ensemble.load(args.members, 1, args.classes, args.arch, "cpu")
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
        logging.error("evaluate: no GPU found. This port evaluates on the MI355X through its HIP kernels and has no CPU path.")
        return 2
    from .evaluate import evaluate
    from .utils.contour_metrics import ContourMetrics, format_line
    from .utils.data_loading import DeviceBatchLoader
    device = torch.device("cuda", torch.cuda.current_device())
    logging.info("Using device %s", device)
    model.to(device=device)
    loader = DeviceBatchLoader(val_set, args.batch_size, shuffle=False, drop_last=True, workers=args.workers, device=device)
    acc = ContourMetrics(spacing=args.spacing) if args.metrics else None
    dice = evaluate(model, loader, device, args.amp, args.pred_dir, postprocess=args.postprocess, metrics=acc, tta=args.tta, tile=args.tile)
    dice = tuple(float(v) for v in dice)
    logging.info("Validation Dice score: %s  postprocessed: %s  min: %s", *dice)
    contour = None
    if acc is not None:
        contour = acc.result()
        logging.info(format_line(contour, args.postprocess))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(report(dice, contour, args.tta, args.tile, None if plain else model.records), f, indent=1)
        logging.info("Results written to %s", args.json)
    return 0


if __name__ == "__main__":
    sys.exit(main())
