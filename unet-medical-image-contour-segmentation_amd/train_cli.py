"""The reference's training command line, /root/reference/train.py:223-309, on the HIP path:

    python -m unet_amd.train -e 5 -b 1 -l 1e-5 -s 0.5 -c 3 [--bilinear] [-f model.pth] [--no-amp]
                             [--model UNet_S] [--data-root DIR] [--checkpoint-dir DIR] [--workers 8] [--seed N]
                             [--pred-dir DIR] [--metrics] [--augment [SPEC]] [--elastic [SPEC]] [--surface-loss [SPEC]]
                             [--loss [SPEC]] [--ema [DECAY[,warmup=N]]] [--save-state] [--resume STATE]
                             [--crop [SPEC]] [--tile [SPEC]] [--distill SPEC] [--optimizer SPEC] [--cache [limit=GiB]]

It reads data_root/{imgs,masks}/{train,val} (BasicDataset, x4 quarter-turn augmentation) and runs the epoch loop of
train.py:29-220, restated literally ("reproduced, not fixed"):
  - train batches shuffled, the last one partial (shuffle=True, drop_last=False); validation in order, drop_last=True;
  - one TrainStepper step per batch (the NaN check raises as train.py:149-151);
  - evaluate(..., postprocess=True) whenever global_step % (n_train // batch_size) == 0, never when that divisor is 0
    (train.py:174-187: it can fall mid-epoch or more than once per epoch), then lr = cosine_warm_restarts_lr(lr, dice);
  - checkpoint_dir/checkpoint_epoch{E}.pth when E > epochs / 2 and E % 5 == 0, with mask_values = train + val
    (train.py:208-216); model_epoch{epochs}.pth, a plain state_dict, in the working directory (train.py:220);
  - --pred-dir DIR (default: off) passes DIR/epoch_{epoch} to evaluate as train.py:99-100 does with ./predictions: the
    validation predictions of every evaluation are written there as grey-coded PNGs (evaluate.py:88-105, 146-164);
  - --metrics (default: off) also scores every evaluation's masks with the contour metrics (utils/contour_metrics.py) and
    logs one line with HD95 / HD / ASSD / IoU, raw and post-processed, after the "Validation Dice score" line;
  - --augment [SPEC] (default: off) passes every TRAINING batch through the seeded device augmentation of utils/augment.py
    (csrc/augment.hip): flips, rotation, scale, shift, brightness, contrast, gamma, noise, drawn per (seed, epoch, item);
    bare --augment is the preset 'default', SPEC is e.g. "flip,rotate=15,scale=0.1,noise=0.01".  Validation is never augmented;
  - --elastic [SPEC] (default: off) adds a smooth elastic deformation to the same launch: random displacements on a coarse
    control grid, cubic B-spline interpolation, image and labels warped together, drawn per (seed, epoch, item); bare
    --elastic is the preset 'default' ("grid=64,sigma=4"), SPEC is "grid=G,sigma=S[,p=P]" with 8 S < G.  It works with or
    without --augment (without it the affine map is the identity).  Validation is never deformed;
  - --surface-loss [W[,ramp=R][,classes=a+b]] (default: off) adds the distance-weighted surface loss (utils/surface_loss.py,
    csrc/surface_loss.hip) to every training step, its distance maps rebuilt on the device from the step's own (augmented)
    labels.  The weight of epoch e (1-based) is min(1, W + R (e - 1)); bare --surface-loss is "0.01,ramp=0.01"; classes default
    to the one evaluate scores.  One log line per epoch gives the weight, the epoch line the summed term;
  - --loss [focal=G[,weights=w0+w1+..][,tversky=A/B][,classes=a+b]] (default: off; bare: "focal=2,tversky=0.3/0.7") replaces the
    CE + Dice pair of every training step by the class-weighted focal + Tversky loss (utils/focal_loss.py, csrc/focal_loss.hip):
    G the focusing exponent, one weight per class of the head (two for -c 1), A / B the prices of false positives / false
    negatives, classes the Tversky subset (default 1..C-1).  The boundary and surface terms stay on top.  A spec that does not
    fit --classes ends the command with status 2 before anything is loaded; the epoch line reports the summed terms;
  - --ema [DECAY[,warmup=N]] (default: off; bare: "0.999,warmup=10") keeps an exponential moving average of the parameters
    inside the optimizer pass (train.EmaConfig, csrc/optim.hip).  Every evaluation of the loop then runs ONCE, on the
    averaged weights (TrainStepper.averaged()): its Dice is what the log prints, marked "(EMA)", and what the learning-rate
    rule receives.  checkpoint_epoch{E}.pth and model_epoch{E}.pth keep the live weights; checkpoint_epoch{E}_ema.pth and
    model_epoch{E}_ema.pth are written beside them in the same wire format (predict, evaluate and seg_main load them as
    they are).  BatchNorm running statistics are the live ones in both;
  - --crop [SIZE[,fg=P][,classes=a+b]] (default: off; bare: "256,fg=0.5") is patch training (utils/crop.py, csrc/crop.hip): every
    TRAINING item gives one SIZE x SIZE crop per epoch, drawn per (seed, epoch, item) and, with probability P, placed so that
    it holds a pixel of the given classes (default: the class evaluate scores).  The training images may then differ in
    size; each must be at least SIZE x SIZE after --scale.  The crop comes before --augment / --elastic.  Validation is
    untouched: whole images, one size per batch.  A spec that does not fit --classes ends the command with status 2;
  - --tile [SIZE[,overlap=N]] (default: off; bare: "512,overlap=128") runs every in-loop evaluation as the sliding-window
    prediction of utils/tiling.py (evaluate(tile=...)): what validates a patch-trained network on images larger than its crops;
  - --distill PATH[,arch=UNet|UNet_S|UNet_T|UNet_SA][,T=t][,w=W] (default: off; arch UNet, T 2, w 1) is knowledge distillation
    (utils/distill.py, csrc/distill_loss.hip): PATH is the checkpoint of a trained network of architecture `arch` with the
    same head (a model_epoch{E}.pth, *_ema.pth or checkpoint_epoch{E}.pth file; no comma in the path).  Every training step
    runs that frozen teacher on its own (cropped, augmented) images and adds W T^2 KL(softmax(teacher / T) || softmax(student /
    T)) to the loss, on top of whichever loss the step runs.  A malformed spec, a missing file or a teacher whose head differs
    from --classes ends the command with status 2 before a dataset or a GPU is touched.  One log line per epoch gives the
    mean term and the mean share of pixels on which student and teacher pick the same class.  Validation, checkpoints and
    the saved model hold the student alone; --save-state records the spec and the SHA-256 of the teacher file;
  - --optimizer SPEC (default: off, the reference's RMSprop) chooses the update rule of the fused optimizer pass
    (train.OptimConfig, csrc/optim.hip): "adamw[,betas=B1/B2][,eps=E][,wd=W]" (defaults 0.9/0.999, 1e-8, 0.01: torch's),
    "sgd[,momentum=M][,nesterov|plain][,wd=W]" (defaults 0.99, nesterov, 3e-5: nnU-Net's) or "rmsprop[,alpha=A][,eps=E]
    [,momentum=M][,wd=W]" (defaults: the reference's values).  The learning rate stays -l and the loop's schedule drives it under
    every rule; gradient clipping, --ema, --save-state and --resume work as with the default.  A malformed spec ends the
    command with status 2; one log line names the canonical spec;
  - --cache [limit=GiB] (default: off) keeps the decoded training and validation files on the device (utils/dataset_cache.py,
    csrc/cache.hip): every file is decoded once, before the first epoch, and every batch of every epoch -- the in-loop
    evaluations' too -- is cut from that arena with one launch instead of being decoded again.  The batches are the same bits,
    so it is NOT a determining argument: it is not recorded by --save-state and --resume takes a run with or without it.
    limit is the most a set may take, in GiB (default: half of the device memory that is free).  One log line per set gives
    its files, MiB and build seconds; a set that is over the limit or does not decode to 8 bits is served as without the
    option, with a warning that says why.  A malformed spec ends the command with status 2;
  - --save-state writes checkpoint_dir/train_state.pth at the end of every epoch (a temporary file renamed over it): model
    and optimizer state (the rule's buffers and step count, the moving average and its update count), epoch, global step, lr, the
    loader's and the augmenter's seeds, and a record of the arguments that determine the run (RECORDED);
  - --resume STATE restores all of that and continues with the epoch after the saved one up to -e: the run is bit for bit
    the run that was never interrupted.  A determining argument that differs from the record ends the command with
    status 2 and a message naming it, and so does a state whose epoch is not below -e (nothing is left to train); -f together
    with --resume is an error;
  - --load drops mask_values (train.py:275-280); -v is accepted and unused, as in the reference.
Input batches come from DeviceBatchLoader: decode threads, pinned collation, rotation + BICUBIC / NEAREST rescale + /255
+ label remap on the device (csrc/data_rescale.hip, csrc/data_prep.hip), bit-identical to stacking ds[i].
--amp (the default) is the project's bf16 path; --no-amp trains in fp32.  There is no CPU fallback: without a GPU the
command exits with status 2."""
from __future__ import annotations

import argparse
import contextlib
import logging
import math
import os
import sys
import time
from pathlib import Path
from typing import Dict, List, NamedTuple, Optional, Tuple

import torch

from .train import EmaConfig, OptimConfig
from .utils.focal_loss import LOSS_BARE, LossConfig

MODELS = ("UNet_S", "UNet", "UNet_T", "UNet_SA")


class SurfaceSpec(NamedTuple):
    """--surface-loss: the weight of epoch 1, its growth per epoch, the selected classes (None: the class evaluate scores)."""
    weight: float
    ramp: float = 0.0
    classes: Optional[Tuple[int, ...]] = None


SURFACE_BARE = "0.01,ramp=0.01"
EMA_BARE = EmaConfig().spec()            # "0.999,warmup=10"
CROP_BARE = "256,fg=0.5"
TILE_BARE = "512,overlap=128"
STATE_FILE = "train_state.pth"
# the arguments that determine a run, as --save-state records and --resume compares them: (record key, command-line name)
RECORDED = (("model", "--model"), ("classes", "--classes"), ("bilinear", "--bilinear"), ("batch_size", "--batch-size"),
            ("scale", "--scale"), ("amp", "--amp / --no-amp"), ("lr", "--learning-rate"), ("augment", "--augment"),
            ("elastic", "--elastic"), ("surface", "--surface-loss"), ("ema", "--ema"), ("loss", "--loss"),
            ("crop", "--crop"), ("tile", "--tile"), ("distill", "--distill"),
            ("distill_sha256", "--distill (the SHA-256 of the teacher file)"), ("optimizer", "--optimizer"))


def parse_surface_spec(text: str) -> SurfaceSpec:
    """"W[,ramp=R][,classes=a+b]" -> SurfaceSpec; ValueError names what is wrong."""
    parts = [t.strip() for t in str(text).split(",")]
    if not parts or not parts[0]:
        raise ValueError("the weight is missing")
    try:
        weight = float(parts[0])
    except ValueError:
        raise ValueError(f"weight {parts[0]!r} is not a number") from None
    if not math.isfinite(weight) or weight < 0.0:
        raise ValueError(f"weight {parts[0]!r} must be finite and >= 0")
    ramp, classes, seen = 0.0, None, set()
    for tok in parts[1:]:
        key, eq, val = tok.partition("=")
        if not eq or not val or key not in ("ramp", "classes"):
            raise ValueError(f"{tok!r} is not ramp=R or classes=a+b")
        if key in seen:
            raise ValueError(f"{key} is given twice")
        seen.add(key)
        try:
            if key == "ramp":
                ramp = float(val)
            else:
                classes = tuple(int(v) for v in val.split("+"))
        except ValueError:
            raise ValueError(f"{tok!r} does not parse") from None
    if not math.isfinite(ramp) or ramp < 0.0:
        raise ValueError("ramp must be finite and >= 0")
    if classes is not None and (min(classes) < 0 or len(set(classes)) != len(classes)):
        raise ValueError("classes must be distinct ids >= 0")
    return SurfaceSpec(weight, ramp, classes)


def _surface_arg(text: str) -> SurfaceSpec:
    try:
        return parse_surface_spec(text)
    except ValueError as e:
        raise argparse.ArgumentTypeError(f"bad --surface-loss {text!r}: {e}") from None


def surface_weight_at(spec: SurfaceSpec, epoch: int) -> float:
    """The surface weight of epoch `epoch` (1-based): min(1, W + R (epoch - 1))."""
    return min(1.0, spec.weight + spec.ramp * (int(epoch) - 1))


def surface_spec_text(spec: Optional[SurfaceSpec]) -> Optional[str]:
    """The canonical spec of a SurfaceSpec (None stays None): parse_surface_spec(text) == spec."""
    if spec is None:
        return None
    return f"{spec.weight!r},ramp={spec.ramp!r}" + (",classes=" + "+".join(str(c) for c in spec.classes) if spec.classes else "")


def _ema_arg(text: str):
    try:
        return EmaConfig.parse(text)
    except ValueError as e:
        raise argparse.ArgumentTypeError(f"bad --ema {text!r}: {e}") from None


def _optimizer_arg(text: str):
    try:
        return OptimConfig.parse(text)
    except ValueError as e:
        raise argparse.ArgumentTypeError(f"bad --optimizer {text!r}: {e}") from None


def _loss_arg(text: str):
    try:
        return LossConfig.parse(text)
    except ValueError as e:
        raise argparse.ArgumentTypeError(f"bad --loss {text!r}: {e}") from None


def _crop_arg(text: str):
    from .utils.crop import CropConfig
    try:
        return CropConfig.parse(text)
    except ValueError as e:
        raise argparse.ArgumentTypeError(f"bad --crop {text!r}: {e}") from None


class CacheSpec(NamedTuple):
    """--cache: the most one dataset's cache may take, in bytes (None: half of the free device memory)."""
    limit_bytes: Optional[int] = None


def parse_cache_spec(text: str) -> CacheSpec:
    """"" or "limit=GiB" -> CacheSpec; ValueError names what is wrong."""
    text = str(text).strip()
    if not text:
        return CacheSpec()
    key, eq, val = (t.strip() for t in text.partition("="))
    if key != "limit" or not eq or not val:
        raise ValueError(f"{text!r} is not limit=GiB")
    try:
        gib = float(val)
    except ValueError:
        raise ValueError(f"limit {val!r} is not a number") from None
    if not math.isfinite(gib) or gib <= 0.0:
        raise ValueError(f"limit {val!r} must be finite and > 0")
    return CacheSpec(int(gib * (1 << 30)))


def _cache_arg(text: str) -> CacheSpec:
    try:
        return parse_cache_spec(text)
    except ValueError as e:
        raise argparse.ArgumentTypeError(f"bad --cache {text!r}: {e}") from None


def build_cache(ds, what: str, spec: CacheSpec, device, workers: int, log=None):
    """The DatasetCache of `ds` under --cache, logged in one line, or None -- with a warning naming the reason -- for a set that is
    over the limit or does not decode to 8 bits: that set is then served through the uncached path."""
    from .utils.dataset_cache import DatasetCache, DatasetCacheTooLarge
    try:
        cache = DatasetCache(ds, device=device, workers=workers, limit_bytes=spec.limit_bytes)
    except (DatasetCacheTooLarge, TypeError) as e:
        logging.warning(f"Dataset cache ({what}): not cached, served through the decode threads: {e}")
        return None
    if log:
        log(f"Dataset cache ({what}): {cache.entries} files, {cache.nbytes / (1 << 20):.1f} MiB on the device, built in "
            f"{cache.build_seconds:.2f} s")
    return cache


def _distill_arg(text: str):
    from .utils.distill import DistillConfig
    try:
        return DistillConfig.parse(text)
    except ValueError as e:
        raise argparse.ArgumentTypeError(f"bad --distill {text!r}: {e}") from None


def _tile_arg(text: str) -> str:
    from .utils.tiling import parse_tile_spec
    try:
        return parse_tile_spec(text).spec
    except ValueError as e:
        raise argparse.ArgumentTypeError(f"bad --tile {text!r}: {e}") from None


def run_record(args: argparse.Namespace) -> Dict:
    """The arguments that determine what a run computes (RECORDED), specs in their canonical form, None for an option that is
    off.  With --distill the record also holds the SHA-256 of the teacher file's bytes.  ValueError for a spec that does not
    parse or a teacher file that cannot be read."""
    from .utils.augment import AugmentConfig, ElasticConfig
    distill = getattr(args, "distill", None)
    optimizer = getattr(args, "optimizer", None)
    if distill is not None:
        from .utils.distill import teacher_sha256
    return {"model": args.model, "classes": int(args.classes), "bilinear": bool(args.bilinear),
            "batch_size": int(args.batch_size), "scale": float(args.scale), "amp": bool(args.amp), "lr": float(args.lr),
            "augment": AugmentConfig.parse(args.augment).spec() if args.augment is not None else None,
            "elastic": ElasticConfig.parse(args.elastic).spec() if args.elastic is not None else None,
            "surface": surface_spec_text(args.surface_loss),
            "ema": args.ema.spec() if args.ema is not None else None,
            "loss": args.loss.spec() if getattr(args, "loss", None) is not None else None,
            "crop": args.crop.spec() if getattr(args, "crop", None) is not None else None,
            "tile": getattr(args, "tile", None),
            "distill": distill.spec() if distill is not None else None,
            "distill_sha256": teacher_sha256(distill.teacher) if distill is not None else None,
            "optimizer": optimizer.spec() if optimizer is not None else None}


def load_resume_state(args: argparse.Namespace) -> Optional[Dict]:
    """--resume: the saved state, read on the CPU and checked against this command line; None without the option.
    ValueError names the argument that is wrong -- before a GPU, a dataset or a model is touched."""
    if not args.resume:
        return None
    if args.load:
        raise ValueError("--load / -f cannot be combined with --resume (the state file carries the weights)")
    state = torch.load(args.resume, map_location="cpu", weights_only=True)
    missing = [k for k in ("model", "optimizer", "epoch", "global_step", "lr", "loader_seed", "augment_seed", "args")
               if not isinstance(state, dict) or k not in state]
    if missing:
        raise ValueError(f"--resume {args.resume}: not a training state (no {', '.join(missing)})")
    if int(state["epoch"]) >= args.epochs:
        raise ValueError(f"--resume {args.resume}: the state was saved after epoch {int(state['epoch'])} and --epochs / -e is "
                         f"{args.epochs}: no epoch is left to train")
    now = run_record(args)
    for key, flag in RECORDED:
        if state["args"].get(key) != now[key]:
            raise ValueError(f"--resume {args.resume}: {flag} ({key}) is {now[key]!r} on the command line, but the state was "
                             f"saved by a run with {state['args'].get(key)!r}")
    return state


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Train the UNet on images and target masks")
    # the reference's flags, short forms and defaults (train.py:223-236)
    p.add_argument("--epochs", "-e", metavar="E", type=int, default=5, help="Number of epochs")
    p.add_argument("--batch-size", "-b", dest="batch_size", metavar="B", type=int, default=1, help="Batch size")
    p.add_argument("--learning-rate", "-l", metavar="LR", type=float, default=1e-5, help="Learning rate", dest="lr")
    p.add_argument("--load", "-f", type=str, default=False, help="Load model from a .pth file")
    p.add_argument("--scale", "-s", type=float, default=0.5, help="Downscaling factor of the images")
    p.add_argument("--validation", "-v", dest="val", type=float, default=10.0,
                   help="Percent of the data that is used as validation (0-100); accepted and unused, as in the reference")
    p.add_argument("--amp", action="store_true", default=True, help="Use mixed precision (bf16; the default)")
    p.add_argument("--bilinear", action="store_true", default=False, help="Use bilinear upsampling")
    p.add_argument("--classes", "-c", type=int, default=3, help="Number of classes")
    # additions
    p.add_argument("--no-amp", dest="amp", action="store_false", help="Train in fp32")
    p.add_argument("--model", choices=MODELS, default="UNet_S", help="Network (train.py:253 uses UNet_S)")
    p.add_argument("--data-root", default="data/data-without-black-shadow",
                   help="Directory holding imgs/{train,val} and masks/{train,val}")
    p.add_argument("--checkpoint-dir", default="./checkpoints", help="Where checkpoint_epoch{E}.pth files go")
    p.add_argument("--workers", type=int, default=8, help="Decode threads per loader")
    p.add_argument("--seed", type=int, default=None, help="Seeds model init and shuffling (default: unseeded)")
    p.add_argument("--pred-dir", default=None,
                   help="Write the validation predictions of every evaluation to DIR/epoch_{epoch} as PNGs (default: off)")
    p.add_argument("--metrics", action="store_true", default=False,
                   help="Log HD95 / HD / ASSD / IoU of every evaluation after its Dice line (default: off)")
    p.add_argument("--augment", nargs="?", const="default", default=None, metavar="SPEC",
                   help="Augment the training batches on the device: a preset name or e.g. 'flip,rotate=15,scale=0.1,"
                        "translate=0.05,brightness=0.1,contrast=0.1,gamma=0.2,noise=0.01' (bare flag: 'default'; default: off)")
    p.add_argument("--elastic", nargs="?", const="default", default=None, metavar="SPEC",
                   help="Deform the training batches elastically on the device: a preset name or 'grid=64,sigma=4[,p=1]' "
                        "(control spacing and displacement sigma in pixels, 8 sigma < grid; bare flag: 'default'; default: off)")
    p.add_argument("--surface-loss", dest="surface_loss", nargs="?", const=SURFACE_BARE, default=None, type=_surface_arg,
                   metavar="W[,ramp=R][,classes=a+b]",
                   help="Add W * surface loss (distance to the true contour, maps built on the device each step); the weight of "
                        f"epoch e is min(1, W + R (e - 1)) (bare flag: '{SURFACE_BARE}'; default: off)")
    p.add_argument("--loss", nargs="?", const=LOSS_BARE, default=None, type=_loss_arg,
                   metavar="focal=G[,weights=w0+w1+..][,tversky=A/B][,classes=a+b]",
                   help="Replace the CE + Dice pair by the class-weighted focal + Tversky loss: focusing exponent G, one weight per "
                        f"class, false-positive / false-negative prices A / B over the given classes (bare flag: '{LOSS_BARE}'; "
                        "default: off)")
    p.add_argument("--ema", nargs="?", const=EMA_BARE, default=None, type=_ema_arg, metavar="DECAY[,warmup=N]",
                   help="Keep an exponential moving average of the weights in the optimizer pass; evaluations run on it and "
                        f"*_ema.pth files are written beside the usual ones (bare flag: '{EMA_BARE}'; default: off)")
    p.add_argument("--crop", nargs="?", const=CROP_BARE, default=None, type=_crop_arg, metavar="SIZE[,fg=P][,classes=a+b]",
                   help="Patch training: one seeded SIZE x SIZE crop per training item and epoch, cut on the device; with "
                        "probability P it holds a pixel of the given classes (default: the class evaluate scores).  The training "
                        f"images may differ in size (bare flag: '{CROP_BARE}'; default: off)")
    p.add_argument("--tile", nargs="?", const=TILE_BARE, default=None, type=_tile_arg, metavar="SIZE[,overlap=N]",
                   help="Run the in-loop evaluations as the sliding-window prediction: tiles of SIZE pixels, overlap blended "
                        f"(bare flag: '{TILE_BARE}'; default: off)")
    p.add_argument("--distill", default=None, type=_distill_arg, metavar="PATH[,arch=NAME][,T=t][,w=W]",
                   help="Knowledge distillation: add W * T^2 * KL(teacher || student) at temperature T against the frozen network of "
                        "architecture NAME (UNet, UNet_S, UNet_T, UNet_SA; default UNet) loaded from the checkpoint PATH "
                        "(defaults: T=2, w=1; default: off)")
    p.add_argument("--optimizer", default=None, type=_optimizer_arg, metavar="RULE[,key=value ...]",
                   help="The update rule of the fused optimizer pass: 'adamw[,betas=B1/B2][,eps=E][,wd=W]', "
                        "'sgd[,momentum=M][,nesterov|plain][,wd=W]' or 'rmsprop[,alpha=A][,eps=E][,momentum=M][,wd=W]'; the learning "
                        "rate stays -l (default: off, the reference's RMSprop)")
    p.add_argument("--cache", nargs="?", const=CacheSpec(), default=None, type=_cache_arg, metavar="limit=GiB",
                   help="Decode every training and validation file once and keep the pixels on the device; every batch is cut "
                        "from there.  limit: the most one set may take, in GiB (default: half of the free device memory).  The "
                        "batches are the same bits, so --resume takes a run with or without it (default: off)")
    p.add_argument("--save-state", dest="save_state", action="store_true", default=False,
                   help=f"Write checkpoint_dir/{STATE_FILE} after every epoch: everything --resume needs (default: off)")
    p.add_argument("--resume", default=None, metavar="STATE",
                   help="Continue the run a --save-state file was written by, bit for bit, with the epoch after the saved one")
    return p


def get_args(argv=None) -> argparse.Namespace:
    return build_parser().parse_args(argv)


# ------------------------------------------------------------------------------------- cadence (train.py:161-216)
def eval_due(global_step: int, n_train: int, batch_size: int) -> bool:
    division_step = n_train // batch_size
    return division_step > 0 and global_step % division_step == 0


def checkpoint_due(epoch: int, epochs: int) -> bool:
    return epoch > epochs * 0.5 and epoch % 5 == 0


def cadence(n_train: int, batch_size: int, epochs: int) -> Dict[str, List]:
    """{'eval_steps': [(epoch, global_step)] at which evaluate runs, 'checkpoint_epochs': [E]} of the loop below
    (steps per epoch: ceil(n_train / batch_size), the last batch partial)."""
    steps = math.ceil(n_train / batch_size)
    evals, gs = [], 0
    for epoch in range(1, epochs + 1):
        for _ in range(steps):
            gs += 1
            if eval_due(gs, n_train, batch_size):
                evals.append((epoch, gs))
    return {"eval_steps": evals, "checkpoint_epochs": [e for e in range(1, epochs + 1) if checkpoint_due(e, epochs)]}


def build_model(name: str, n_classes: int, bilinear: bool):
    from . import unet
    return getattr(unet, name)(n_channels=1, n_classes=n_classes, bilinear=bilinear)


def run_training(model, device, train_set, val_set, *, epochs: int, batch_size: int, learning_rate: float, amp: bool,
                 checkpoint_dir: str = "./checkpoints", seed: Optional[int] = None, workers: int = 8,
                 train_loader=None, log=None, pred_dir: Optional[str] = None, metrics: bool = False,
                 augment=None, surface: Optional[SurfaceSpec] = None, elastic=None, ema=None, save_state: bool = False,
                 resume: Optional[Dict] = None, record: Optional[Dict] = None, loss=None, crop=None, tile=None,
                 distill=None, optimizer=None, cache: Optional[CacheSpec] = None) -> List[Dict]:
    """The epoch loop of train.py:29-220 over directory datasets.  Returns one record per epoch: the summed loss, the
    last evaluation's three Dice figures (None in an epoch without one), the lr, the training images/s of the epoch (train
    images over the epoch's wall time without its evaluations) and the seconds spent evaluating.
    `augment`: an AugmentConfig, a spec string or a BatchAugment for the TRAIN loader (a config is seeded with the loader's
    seed: `seed`, or the loader's own draw when unseeded); the validation loader never gets one.
    `elastic`: an ElasticConfig or a spec string, added to that augmenter; alone, it deforms over the identity affine map.
    `surface`: a SurfaceSpec; every epoch's steps run with surface_weight_at(surface, epoch), and the record gains the weight
    and the summed term.
    `ema`: an EmaConfig or a spec string; every evaluation then runs inside stepper.averaged() (once, on the averaged
    weights: that Dice is logged, marked "(EMA)", and drives the lr), every checkpoint gets a *_ema.pth twin, and the last
    record returned carries the averaged model as "ema_state_dict" (TrainStepper.ema_state_dict(), on the CPU).
    `loss`: a LossConfig or a spec string; every step runs the focal + Tversky node in place of the CE + Dice pair, and the record
    gains the summed "focal" and "tversky" terms.
    `crop`: a CropConfig, a spec string or a BatchCrop for the TRAIN loader (a config is seeded with the loader's seed, which
    is the saved one on resume: the state file needs no key for it); the validation loader never gets one.
    `tile`: a TileConfig or a spec string, passed to every evaluation of the loop.
    `distill`: a DistillConfig, a spec string or a Distiller; every step adds the distillation term against the frozen teacher, the
    record gains the epoch's mean "kd" and "kd_agree", and one line per epoch logs them.  Evaluations and checkpoints hold the
    student alone.
    `optimizer`: an OptimConfig or a spec string: the rule of the fused optimizer pass (None: RMSprop as ever); one line logs it.
    `cache`: a CacheSpec: both loaders are served from a DatasetCache of their set (build_cache; a set that cannot be cached is
    served as without it).  The batches are the same bits, so nothing of it is recorded.
    `save_state`: write checkpoint_dir/train_state.pth after every epoch, holding `record` (run_record) as its "args".
    `resume`: such a state (load_resume_state); the model must already hold its weights.  Optimizer state, lr, counters
    and the seeds are restored and the loop continues with the epoch after the saved one: only those epochs are returned."""
    from .evaluate import evaluate
    from .checkpoint import save_checkpoint
    from .train import TrainStepper, cosine_warm_restarts_lr
    from .utils.data_loading import DeviceBatchLoader
    n_train = len(train_set)
    if train_loader is None:
        train_loader = DeviceBatchLoader(train_set, batch_size, shuffle=True, drop_last=False,
                                         seed=seed if resume is None else resume["loader_seed"], workers=workers, device=device)
    elif resume is not None:
        train_loader.seed = int(resume["loader_seed"])
    built = []                                                               # the caches of this call, closed at its end
    if cache is not None and train_loader.cache is None and not train_loader.host_rescale:
        train_loader.cache = build_cache(train_set, "training", cache, device, workers, log)
        built.append(train_loader.cache)
    if crop is not None:
        from .utils.crop import BatchCrop
        if not isinstance(crop, BatchCrop):
            crop = BatchCrop(crop, train_loader.seed, model.n_classes)
        train_loader.crop = crop
        if log:
            log(f"Training crops (seed {crop.seed}): {crop.config.spec()}")
    if augment is not None or elastic is not None:
        from .utils.augment import AugmentConfig, BatchAugment
        if isinstance(augment, BatchAugment):
            if elastic is not None:
                raise ValueError("run_training: a BatchAugment carries its own elastic configuration")
        else:
            aug_seed = train_loader.seed if resume is None or resume["augment_seed"] is None else resume["augment_seed"]
            augment = BatchAugment(augment if augment is not None else AugmentConfig(), aug_seed, elastic=elastic)
        train_loader.augment = augment
        if log:
            log(f"Training augmentation (seed {augment.seed}): {augment.config.spec()}"
                + (f"; elastic {augment.elastic.spec()}" if augment.elastic is not None else ""))
    if cache is not None:
        built.append(build_cache(val_set, "validation", cache, device, workers, log))
    val_loader = DeviceBatchLoader(val_set, batch_size, shuffle=False, drop_last=True, workers=workers, device=device,
                                   cache=built[-1] if cache is not None else None)
    stepper = TrainStepper(model, lr=learning_rate, amp=amp, surface_classes=surface.classes if surface is not None else None,
                           ema=ema, loss=loss, **({} if distill is None else {"distill": distill}),
                           **({} if optimizer is None else {"optimizer": optimizer}))
    if stepper.optim_config is not None and log:
        log(f"Optimizer: {stepper.optim_config.spec()}")
    if stepper.distill is not None and log:
        log(f"Distillation: teacher {stepper.distill.config.spec()}")
    lr = learning_rate
    global_step = 0
    first_epoch = 1
    if resume is not None:
        stepper.optimizer.load_state_dict(resume["optimizer"])
        lr = float(resume["lr"])
        stepper.optimizer.param_groups[0]["lr"] = lr
        global_step = int(resume["global_step"])
        first_epoch = int(resume["epoch"]) + 1
        train_loader.epoch = int(resume["epoch"])          # the loader's 0-based epoch is also the augmenter's
        if log:
            log(f"Resumed after epoch {resume['epoch']} (global step {global_step}, lr {lr:.6g})")
    tag = " (EMA)" if stepper.ema is not None else ""
    tile_kw = {"tile": tile} if tile is not None else {}
    mask_values = train_set.mask_values + val_set.mask_values
    history = []
    for epoch in range(first_epoch, epochs + 1):
        model.train()
        losses, surfaces, focals, tverskys, kds, agrees = [], [], [], [], [], []
        if surface is not None:
            stepper.surface_weight = surface_weight_at(surface, epoch)
            if log:
                log(f"Epoch {epoch}/{epochs}: surface loss weight {stepper.surface_weight:.6g}")
        dice = (None, None, None)
        eval_s = 0.0
        seen = 0
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        for batch in train_loader:
            images, true_masks = batch["image"], batch["mask"]
            terms = stepper.step(images, true_masks)
            losses.append(terms["loss"].detach())
            if "surface" in terms:
                surfaces.append(terms["surface"].detach())
            if "focal" in terms:
                focals.append(terms["focal"].detach())
                tverskys.append(terms["tversky"].detach())
            if "kd" in terms:
                kds.append(terms["kd"].detach())
                agrees.append(terms["kd_agree"].detach())
            seen += images.shape[0]
            global_step += 1
            if eval_due(global_step, n_train, batch_size):
                torch.cuda.synchronize(device)
                te = time.perf_counter()
                epoch_pred_dir = os.path.join(pred_dir, f"epoch_{epoch}") if pred_dir else None  # train.py:99-100
                acc = None
                if metrics:
                    from .utils.contour_metrics import ContourMetrics, format_line
                    acc = ContourMetrics()
                with (stepper.averaged() if stepper.ema is not None else contextlib.nullcontext()):
                    val_score, val_post, val_min = evaluate(model, val_loader, device, amp, epoch_pred_dir, metrics=acc, **tile_kw)  # postprocess=True
                lr = cosine_warm_restarts_lr(learning_rate, float(val_score))                    # scheduler.step(val_score)
                stepper.optimizer.param_groups[0]["lr"] = lr
                dice = (float(val_score), float(val_post), float(val_min))
                eval_s += time.perf_counter() - te
                if log:
                    log(f"Validation Dice score{tag}: {dice[0]}  postprocessed: {dice[1]}  min: {dice[2]}")
                if acc is not None:
                    contour = acc.result()
                    if log:
                        log(format_line(contour))
        torch.cuda.synchronize(device)
        wall = time.perf_counter() - t0
        epoch_loss = 0.0
        for v in torch.stack(losses).float().cpu().tolist() if losses else []:
            epoch_loss += v                                                                      # loss.item() summed
        rec = {"epoch": epoch, "loss": epoch_loss, "val_dice": dice[0], "val_dice_post": dice[1], "val_dice_min": dice[2],
               "lr": lr, "images": seen, "img_s": seen / max(wall - eval_s, 1e-9), "eval_s": eval_s}
        if surface is not None:
            rec["surface_weight"] = stepper.surface_weight
            rec["surface"] = float(torch.stack(surfaces).double().sum().item()) if surfaces else 0.0
        if stepper.loss is not None:
            rec["focal"] = float(torch.stack(focals).double().sum().item()) if focals else 0.0
            rec["tversky"] = float(torch.stack(tverskys).double().sum().item()) if tverskys else 0.0
        if stepper.distill is not None:
            rec["kd"] = float(torch.stack(kds).double().mean().item()) if kds else 0.0
            rec["kd_agree"] = float(torch.stack(agrees).double().mean().item()) if agrees else 0.0
            if log:
                log(f"Epoch {epoch}/{epochs}: distillation kd (mean) {rec['kd']:.6g}, agreement with the teacher (mean) "
                    f"{rec['kd_agree']:.4f}")
        if checkpoint_dir is not None and checkpoint_due(epoch, epochs):
            path = os.path.join(checkpoint_dir, f"checkpoint_epoch{epoch}.pth")
            save_checkpoint(model, path, mask_values=mask_values)
            rec["checkpoint"] = path
            if stepper.ema is not None:
                save_checkpoint(model, path[:-len(".pth")] + "_ema.pth", mask_values=mask_values,
                                state_dict=stepper.ema_state_dict())
        if save_state and checkpoint_dir is not None:
            rec["state"] = _write_state(os.path.join(checkpoint_dir, STATE_FILE), model, stepper, epoch, global_step, lr,
                                        train_loader.seed, augment.seed if augment is not None else None, record)
        history.append(rec)
        if log:
            log(f"Epoch {epoch}/{epochs}: loss (total) {epoch_loss:.6g}, Dice{tag} {dice[0]} / post {dice[1]} / min {dice[2]}, "
                f"lr {lr:.6g}, {rec['img_s']:.1f} images/s ({seen} images, evaluation {eval_s:.2f} s)"
                + (f", surface (summed) {rec['surface']:.6g} at weight {rec['surface_weight']:.6g}" if "surface" in rec else "")
                + (f", focal (summed) {rec['focal']:.6g}, tversky (summed) {rec['tversky']:.6g}" if "focal" in rec else "")
                + (f", checkpoint {rec['checkpoint']}" if "checkpoint" in rec else ""))
    if stepper.ema is not None and history:
        history[-1]["ema_state_dict"] = stepper.ema_state_dict()
    stepper.close()
    for c in built:
        if c is not None:
            c.close()
    return history


def _write_state(path: str, model, stepper, epoch: int, global_step: int, lr: float, loader_seed: int,
                 augment_seed: Optional[int], record: Optional[Dict]) -> str:
    """--save-state: everything --resume needs, written beside `path` and renamed over it (a reader never sees half a file)."""
    cpu = lambda v: v.detach().cpu() if torch.is_tensor(v) else v
    state = {"format": 1, "model": {k: cpu(v) for k, v in model.state_dict().items()},
             "optimizer": {k: cpu(v) for k, v in stepper.optimizer.state_dict().items()},
             "epoch": int(epoch), "global_step": int(global_step), "lr": float(lr), "loader_seed": int(loader_seed),
             "augment_seed": int(augment_seed) if augment_seed is not None else None, "args": dict(record or {})}
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    tmp = path + ".tmp"
    torch.save(state, tmp)
    os.replace(tmp, path)
    return path


def main(argv=None) -> int:
    args = get_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(levelname)s: %(message)s")
    try:
        if args.loss is not None:
            try:
                args.loss.for_head(args.classes)                              # against the head, before anything is loaded
            except ValueError as e:
                raise ValueError(f"--loss: {e}") from None
        if args.crop is not None:
            try:
                args.crop.for_head(args.classes)                              # likewise
            except ValueError as e:
                raise ValueError(f"--crop: {e}") from None
        if args.distill is not None:
            from .utils.distill import check_teacher
            try:
                check_teacher(args.distill, 1, args.classes)                  # the file and its head, likewise (build_model: 1 channel)
            except ValueError as e:
                raise ValueError(f"--distill: {e}") from None
        resume = load_resume_state(args)                                      # a refused --resume needs no GPU to say so
        record = run_record(args) if (args.save_state or resume is not None) else None
    except ValueError as e:
        logging.error(f"train: {e}")
        return 2
    if not torch.cuda.is_available():
        logging.error("train: no GPU found. This port trains on the MI355X through its HIP kernels and has no CPU path.")
        return 2
    from .checkpoint import load_checkpoint
    from .utils.data_loading import BasicDataset
    device = torch.device("cuda", torch.cuda.current_device())
    logging.info(f"Using device {device}")
    root = Path(args.data_root)
    augment = None
    if args.augment is not None:
        from .utils.augment import AugmentConfig
        augment = AugmentConfig.parse(args.augment)                           # a bad spec fails before anything is loaded
    elastic = None
    if args.elastic is not None:
        from .utils.augment import ElasticConfig
        elastic = ElasticConfig.parse(args.elastic)                           # likewise
    if args.surface_loss is not None:
        from .utils.surface_loss import head_classes
        try:
            head_classes(args.classes, args.surface_loss.classes)             # against the head, before anything is loaded
        except ValueError as e:
            logging.error(f"train: --surface-loss: {e}")
            return 2
    train_set = BasicDataset(root / "imgs" / "train", root / "masks" / "train", args.scale)
    val_set = BasicDataset(root / "imgs" / "val", root / "masks" / "val", args.scale)
    if args.seed is not None:
        torch.manual_seed(args.seed)
    model = build_model(args.model, args.classes, args.bilinear)
    model = model.to(memory_format=torch.channels_last)
    logging.info(f"Network: {args.model}, {model.n_channels} input channels, {model.n_classes} output channels (classes), "
                 f"{'bilinear' if args.bilinear else 'transposed conv'} upscaling")
    if args.load:
        load_checkpoint(model, args.load, device="cpu")                       # mask_values dropped (train.py:275-280)
        logging.info(f"Model loaded from {args.load}")
    if resume is not None:
        model.load_state_dict(resume["model"])
        logging.info(f"Training state loaded from {args.resume}")
    model.to(device=device)
    n_train, n_val = len(train_set), len(val_set)
    logging.info(f"Starting training: epochs {args.epochs}, batch size {args.batch_size}, learning rate {args.lr}, "
                 f"training items {n_train}, validation items {n_val}, scale {args.scale}, "
                 f"{'bf16 autocast' if args.amp else 'fp32'}, checkpoints in {args.checkpoint_dir}")
    history = run_training(model, device, train_set, val_set, epochs=args.epochs, batch_size=args.batch_size,
                           learning_rate=args.lr, amp=args.amp, checkpoint_dir=args.checkpoint_dir, seed=args.seed,
                           workers=args.workers, log=logging.info, pred_dir=args.pred_dir, metrics=args.metrics,
                           augment=augment, surface=args.surface_loss, elastic=elastic, ema=args.ema,
                           save_state=args.save_state, resume=resume, record=record, loss=args.loss,
                           crop=args.crop, tile=args.tile, distill=args.distill, optimizer=args.optimizer, cache=args.cache)
    path = f"model_epoch{args.epochs}.pth"
    torch.save({k: v.detach().cpu() for k, v in model.state_dict().items()}, path)                # train.py:220
    logging.info(f"Model saved to {path}")
    if args.ema is not None:
        path = f"model_epoch{args.epochs}_ema.pth"
        torch.save(history[-1]["ema_state_dict"], path)
        logging.info(f"Averaged model saved to {path}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
