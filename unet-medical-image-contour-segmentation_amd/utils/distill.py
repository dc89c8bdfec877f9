"""Knowledge distillation (Hinton et al.; csrc/distill_loss.hip; the reference has no counterpart; DESIGN.md section 3
"Distillation"): a small network is trained on the labels and also on the temperature-softened class probabilities of a trained
large one.  Student logits z, teacher logits v, a head of C classes, n pixels:

    q = softmax(v / T),  p = softmax(z / T)
    kd    = T^2 / n  sum_x sum_c q_c (log q_c - log p_c)
    agree = 1 / n  sum_x [argmax z = argmax v]                   (a logged diagnostic, no gradient)
    loss += w kd

The one-channel head is the two-class case on the logits (0, z) and (0, v).

    DistillConfig                                                teacher file, its architecture, T, w; parse / spec / of
    distill_loss(student_logits, teacher_logits, n_classes, config)   -> 0-dim tensor with gradient (to the student only)
    Distiller(config, n_channels, n_classes, device, amp)        the frozen teacher: teacher_logits(images)

seg_loss / train_step / TrainStepper take them as `distill=`: the term is added on top of whatever loss the step runs.  The
command line's --distill SPEC builds it."""
from __future__ import annotations

import dataclasses
import hashlib
import math
import os
from typing import Dict, Optional, Union

import torch

ARCHS = ("UNet", "UNet_S", "UNet_T", "UNet_SA")


def _num(text: str, what: str) -> float:
    try:
        return float(text)
    except ValueError:
        raise ValueError(f"DistillConfig.parse: {what} {text!r} is not a number") from None


@dataclasses.dataclass(frozen=True)
class DistillConfig:
    """The distillation term: `teacher` the checkpoint file of the trained network (a live, *_ema or checkpoint_epoch file; no
    comma in the path), `arch` its architecture, T > 0 the temperature both sides are softened with, w > 0 the weight of the
    term.  The defaults are the bare path."""
    teacher: str
    arch: str = "UNet"
    T: float = 2.0
    w: float = 1.0

    def __post_init__(self):
        def number(v):
            return isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v)
        path = os.fspath(self.teacher) if isinstance(self.teacher, os.PathLike) else self.teacher
        if not isinstance(path, str) or not path.strip():
            raise ValueError(f"DistillConfig: the teacher is the path of a checkpoint file, not {self.teacher!r}")
        if "," in path:
            raise ValueError(f"DistillConfig: the teacher path may not contain a comma: {path!r}")
        if self.arch not in ARCHS:
            raise ValueError(f"DistillConfig: arch is one of {', '.join(ARCHS)}, not {self.arch!r}")
        if not (number(self.T) and self.T > 0):
            raise ValueError(f"DistillConfig: the temperature (T=) is a finite number > 0, not {self.T!r}")
        if not (number(self.w) and self.w > 0):
            raise ValueError(f"DistillConfig: the weight (w=) is a finite number > 0, not {self.w!r}")
        object.__setattr__(self, "teacher", path.strip())
        object.__setattr__(self, "T", float(self.T))
        object.__setattr__(self, "w", float(self.w))

    @classmethod
    def parse(cls, spec: str) -> "DistillConfig":
        """'PATH[,arch=UNet|UNet_S|UNet_T|UNet_SA][,T=t][,w=W]' -> config, e.g. 'model_epoch50_ema.pth,arch=UNet,T=2'; the path is
        the first token, a key that is left out keeps its default.  ValueError names what is wrong."""
        parts = [t.strip() for t in str(spec).split(",")]
        if not parts[0]:
            raise ValueError(f"DistillConfig.parse: the teacher path is missing in {spec!r}")
        if "=" in parts[0] and parts[0].partition("=")[0] in ("arch", "T", "w"):
            raise ValueError(f"DistillConfig.parse: the teacher path is missing in {spec!r} (it is the first token)")
        kw = {}
        for tok in parts[1:]:
            key, eq, val = (t.strip() for t in tok.partition("="))
            if key not in ("arch", "T", "w") or not eq or not val:
                raise ValueError(f"DistillConfig.parse: {tok!r} is not arch=NAME, T=t or w=W in {spec!r} (the path is the first "
                                 "token and may not contain a comma)")
            if key in kw:
                raise ValueError(f"DistillConfig.parse: {key} is given twice in {spec!r}")
            kw[key] = val if key == "arch" else _num(val, "the temperature (T)" if key == "T" else "the weight (w)")
        return cls(parts[0], **kw)

    def spec(self) -> str:
        """The canonical spec: DistillConfig.parse(cfg.spec()) == cfg."""
        return f"{self.teacher},arch={self.arch},T={self.T!r},w={self.w!r}"

    @classmethod
    def of(cls, distill: Union[None, str, "DistillConfig"]) -> Optional["DistillConfig"]:
        """None, a spec string or a config -> None or a config."""
        if distill is None or isinstance(distill, cls):
            return distill
        if isinstance(distill, str):
            return cls.parse(distill)
        raise TypeError(f"distill is a DistillConfig or a spec string, not {type(distill).__name__}")


def teacher_sha256(path: str) -> str:
    """SHA-256 of the teacher file's bytes (what --save-state records beside the spec); ValueError when it cannot be read."""
    h = hashlib.sha256()
    try:
        with open(path, "rb") as f:
            for block in iter(lambda: f.read(1 << 20), b""):
                h.update(block)
    except OSError as e:
        raise ValueError(f"the teacher file {path!r} cannot be read: {e.strerror or e}") from None
    return h.hexdigest()


def _load_state(path: str, what: str = "teacher") -> Dict[str, torch.Tensor]:
    if not os.path.isfile(path):
        raise ValueError(f"the {what} file {path!r} does not exist")
    try:
        try:
            state = torch.load(path, map_location="cpu", weights_only=True)
        except Exception:
            state = torch.load(path, map_location="cpu", weights_only=False)
    except Exception as e:
        raise ValueError(f"the {what} file {path!r} is not a checkpoint: {e}") from None
    if not isinstance(state, dict) or "outc.conv.weight" not in state or "inc.double_conv.0.weight" not in state:
        raise ValueError(f"the {what} file {path!r} is not a checkpoint of this project's networks (no inc / outc weights)")
    return state


def teacher_shape(path: str, what: str = "teacher") -> Dict:
    """What the checkpoint's keys say about the teacher, read on the CPU: {'n_channels', 'n_classes', 'bilinear'} -- input
    channels of the stem, outputs of the head, and bilinear (no transposed-conv weights) vs transposed-conv upsampling.
    `what` names the file's role in the error text (utils/ensemble.py reads its members through this)."""
    state = _load_state(path, what)
    return {"n_channels": int(state["inc.double_conv.0.weight"].shape[1]), "n_classes": int(state["outc.conv.weight"].shape[0]),
            "bilinear": not any(k.endswith(".up.weight") for k in state)}


def check_teacher(config, n_channels: int, n_classes: int) -> Dict:
    """The teacher file of `config` against the student's input channels and head, without a GPU; -> teacher_shape(path).
    ValueError names both sides of a mismatch."""
    cfg = DistillConfig.of(config)
    shape = teacher_shape(cfg.teacher)
    if shape["n_classes"] != int(n_classes):
        raise ValueError(f"the teacher {cfg.teacher!r} has a head of {shape['n_classes']} outputs, the student one of {int(n_classes)}: "
                         "distillation compares the two heads class by class")
    if shape["n_channels"] != int(n_channels):
        raise ValueError(f"the teacher {cfg.teacher!r} takes {shape['n_channels']} input channels, the student {int(n_channels)}: both "
                         "see the same images")
    return shape


def distill_terms(student_logits: torch.Tensor, teacher_logits: torch.Tensor, n_classes: int, config, *, reduce_sums=None,
                  world: float = 1):
    """(w * kd, kd, agree) of student and teacher logits [B,n_classes,H,W] (or [B,H,W] for the one-channel head) as the models
    return them.  Only the first carries gradient, and only to the student."""
    from .. import losses
    cfg = DistillConfig.of(config)
    if cfg is None:
        raise ValueError("distill_loss needs a DistillConfig or a spec string")
    if tuple(student_logits.shape) != tuple(teacher_logits.shape):
        raise ValueError(f"distill_loss: student logits {tuple(student_logits.shape)} and teacher logits {tuple(teacher_logits.shape)} "
                         "differ in shape")
    s, _ = losses.head_layout(student_logits, n_classes, "distill_loss")
    t, _ = losses.head_layout(teacher_logits, n_classes, "distill_loss")
    return losses.DistillLossFn.apply(s, t, cfg.T, cfg.w, reduce_sums, world)


def distill_loss(student_logits: torch.Tensor, teacher_logits: torch.Tensor, n_classes: int, config) -> torch.Tensor:
    """w * kd as a 0-dim tensor; its gradient reaches the student's logits only.  `config`: a DistillConfig or a spec string."""
    return distill_terms(student_logits, teacher_logits, n_classes, config)[0]


class Distiller:
    """The frozen teacher of a distilling run.  Built with train_cli.build_model(config.arch, ...), bilinear vs transposed-conv
    upsampling read off the checkpoint's keys, loaded with checkpoint.load_checkpoint (live, *_ema and checkpoint_epoch files
    alike), in eval() with requires_grad_(False): it is in no optimizer, no flat buffer, no moving average and no checkpoint
    of the student's, its BatchNorm running statistics never move, and under data parallel every rank holds its own copy
    that no collective touches.  A head or input-channel mismatch with the student raises ValueError naming both sides."""

    def __init__(self, config, n_channels: int, n_classes: int, device, amp: bool = True):
        from ..checkpoint import load_checkpoint
        from ..train_cli import build_model
        self.config = DistillConfig.of(config)
        if self.config is None:
            raise ValueError("Distiller needs a DistillConfig or a spec string")
        shape = check_teacher(self.config, n_channels, n_classes)
        self.amp = bool(amp)
        self.device = torch.device(device)
        model = build_model(self.config.arch, int(n_classes), shape["bilinear"])
        if model.n_channels != int(n_channels):
            raise ValueError(f"the teacher architecture {self.config.arch} takes {model.n_channels} input channels, the student "
                             f"{int(n_channels)}")
        try:
            load_checkpoint(model, self.config.teacher, device="cpu")
        except RuntimeError as e:
            raise ValueError(f"the teacher file {self.config.teacher!r} does not hold a {self.config.arch}"
                             f"{' (bilinear)' if shape['bilinear'] else ''}: {e}") from None
        model = model.to(memory_format=torch.channels_last).to(device=self.device)
        model.eval()
        model.requires_grad_(False)
        self.teacher = model

    def teacher_logits(self, images: torch.Tensor) -> torch.Tensor:
        """The teacher's logits for `images`, each item computed bit for bit as it is alone (the batch-invariant eval forward),
        without autograd.  The step record of a surrounding training step (ops.STEP) is set aside for the call and is back,
        unchanged, when it returns: the teacher's logits depend on the item and the teacher alone."""
        from .. import ops
        from ..inference import eval_forward
        with ops.step_state(**ops.StepState()._asdict()):
            return eval_forward(self.teacher, images, self.amp, plan_images=1)
