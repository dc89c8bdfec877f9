"""Class-weighted focal + Tversky loss for imbalanced classes (csrc/focal_loss.hip; the reference has no counterpart;
DESIGN.md section 3 "Focal / Tversky loss").  For a head of C classes with softmax p, labels t, n pixels:

    u        = sum_{c != t} p_c                                  (1 - p_t, formed without the cancellation)
    focal    = sum_x w_t u^gamma (-log p_t) / sum_x w_t          (Lin et al.; gamma = 0: the weighted cross-entropy)
    TI_c     = (TP_c + eps) / ((1 - alpha - beta) TP_c + alpha P_c + beta T_c + eps),  eps = 1e-6
    tversky  = 1 / |K| sum_{c in K} (1 - TI_c)                   (Salehi et al.; alpha = beta = 0.5: the per-class Dice)
    loss     = focal + tversky

The one-channel head is the two-class case on the logits (0, z): labels mask // 2, K = {1}, two weights.

    LossConfig                                                   gamma, weights, alpha / beta, classes; parse / spec / of
    focal_tversky_loss(logits, true_masks, n_classes, config)   -> 0-dim tensor with gradient, next to surface_loss

seg_loss / train_step / TrainStepper take the config as `loss=`: it replaces the CE + Dice pair, the boundary and surface terms
stay on top.  The command line's --loss [SPEC] builds it."""
from __future__ import annotations

import dataclasses
import math
from typing import Optional, Tuple, Union

import torch


def _num(text: str, what: str) -> float:
    try:
        v = float(text)
    except ValueError:
        raise ValueError(f"LossConfig.parse: {what} {text!r} is not a number") from None
    return v


@dataclasses.dataclass(frozen=True)
class LossConfig:
    """The focal + Tversky loss that replaces the CE + Dice pair.  gamma >= 0 is the focusing exponent; weights (None: all 1)
    one per class of the head, each > 0 (two for the one-channel head: background, foreground); alpha / beta >= 0 with
    alpha + beta > 0 price false positives / false negatives; classes (None: 1..C-1) the Tversky subset.  The defaults are the
    bare --loss flag."""
    gamma: float = 2.0
    weights: Optional[Tuple[float, ...]] = None
    alpha: float = 0.3
    beta: float = 0.7
    classes: Optional[Tuple[int, ...]] = None

    def __post_init__(self):
        def number(v):
            return isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v)
        if not (number(self.gamma) and self.gamma >= 0):
            raise ValueError(f"LossConfig: gamma (focal=) is a finite number >= 0, not {self.gamma!r}")
        if not (number(self.alpha) and number(self.beta) and self.alpha >= 0 and self.beta >= 0 and self.alpha + self.beta > 0):
            raise ValueError(f"LossConfig: alpha and beta (tversky=) are finite and >= 0 with alpha + beta > 0, not "
                             f"{self.alpha!r} / {self.beta!r}")
        if self.weights is not None:
            w = tuple(self.weights)
            if not 2 <= len(w) <= 8 or not all(number(v) and v > 0 for v in w):
                raise ValueError(f"LossConfig: weights are 2 to 8 finite numbers > 0, not {self.weights!r}")
            object.__setattr__(self, "weights", tuple(float(v) for v in w))
        if self.classes is not None:
            c = tuple(self.classes)
            if not c or not all(isinstance(v, int) and not isinstance(v, bool) and 0 <= v < 8 for v in c) or len(set(c)) != len(c):
                raise ValueError(f"LossConfig: classes are distinct ids in [0, 8), not {self.classes!r}")
            object.__setattr__(self, "classes", c)
        object.__setattr__(self, "gamma", float(self.gamma))
        object.__setattr__(self, "alpha", float(self.alpha))
        object.__setattr__(self, "beta", float(self.beta))

    @classmethod
    def parse(cls, spec: str) -> "LossConfig":
        """'focal=G[,weights=w0+w1+..][,tversky=A/B][,classes=a+b]' -> config, e.g. 'focal=2,tversky=0.3/0.7'; a key that is left
        out keeps its default.  ValueError names what is wrong."""
        vals = {}
        parts = [t.strip() for t in str(spec).split(",")]
        if not any(parts):
            raise ValueError(f"LossConfig.parse: focal=G is missing in {spec!r}")
        for tok in parts:
            key, eq, val = (t.strip() for t in tok.partition("="))
            if key not in ("focal", "weights", "tversky", "classes") or not eq or not val:
                raise ValueError(f"LossConfig.parse: {tok!r} is not focal=G, weights=w0+w1+.., tversky=A/B or classes=a+b in {spec!r}")
            if key in vals:
                raise ValueError(f"LossConfig.parse: {key} is given twice in {spec!r}")
            if key == "focal":
                vals[key] = _num(val, "focal (gamma)")
            elif key == "weights":
                vals[key] = tuple(_num(v, "weight") for v in val.split("+"))
            elif key == "tversky":
                a, slash, b = val.partition("/")
                if not slash:
                    raise ValueError(f"LossConfig.parse: tversky {val!r} is not A/B")
                vals[key] = (_num(a, "tversky alpha"), _num(b, "tversky beta"))
            else:
                try:
                    vals[key] = tuple(int(v) for v in val.split("+"))
                except ValueError:
                    raise ValueError(f"LossConfig.parse: classes {val!r} are not integers joined by +") from None
        if "focal" not in vals:
            raise ValueError(f"LossConfig.parse: focal=G is missing in {spec!r}")
        kw = {"gamma": vals["focal"]}
        if "weights" in vals:
            kw["weights"] = vals["weights"]
        if "tversky" in vals:
            kw["alpha"], kw["beta"] = vals["tversky"]
        if "classes" in vals:
            kw["classes"] = vals["classes"]
        return cls(**kw)

    def spec(self) -> str:
        """The canonical spec: LossConfig.parse(cfg.spec()) == cfg."""
        return (f"focal={self.gamma!r}"
                + ("" if self.weights is None else ",weights=" + "+".join(repr(v) for v in self.weights))
                + f",tversky={self.alpha!r}/{self.beta!r}"
                + ("" if self.classes is None else ",classes=" + "+".join(str(c) for c in self.classes)))

    @classmethod
    def of(cls, loss: Union[None, str, "LossConfig"]) -> Optional["LossConfig"]:
        """None, a spec string or a config -> None or a config."""
        if loss is None or isinstance(loss, cls):
            return loss
        if isinstance(loss, str):
            return cls.parse(loss)
        raise TypeError(f"loss is a LossConfig or a spec string, not {type(loss).__name__}")

    def for_head(self, n_classes: int) -> Tuple[Tuple[float, ...], Tuple[int, ...]]:
        """(weights, classes) of this config on a head of `n_classes` outputs (1: the one-channel head, two classes); ValueError
        when the number of weights or a class does not fit the head."""
        from .. import losses
        return losses.focal_head(n_classes, self.weights, self.classes)


LOSS_BARE = "focal=2,tversky=0.3/0.7"


def focal_tversky_terms(logits: torch.Tensor, true_masks: torch.Tensor, n_classes: int, config, *, reduce_sums=None, world: float = 1):
    """(total, focal, tversky) of logits [B,n_classes,H,W] (or [B,H,W] for the one-channel head) as the model returns them and
    int labels [B,H,W] with the dataset's values (NOT yet // 2 for the one-channel head).  Only `total` carries gradient."""
    from .. import losses
    cfg = LossConfig.of(config)
    if cfg is None:
        raise ValueError("focal_tversky_loss needs a LossConfig or a spec string")
    w, cls = cfg.for_head(n_classes)
    lg, mask_div = losses.head_layout(logits, n_classes, "focal_tversky_loss")
    return losses.FocalTverskyLossFn.apply(lg, true_masks, mask_div, w, cfg.gamma, cfg.alpha, cfg.beta, cls, reduce_sums, world)


def focal_tversky_loss(logits: torch.Tensor, true_masks: torch.Tensor, n_classes: int, config) -> torch.Tensor:
    """The focal + Tversky loss as a 0-dim tensor; its gradient reaches the logits.  `config`: a LossConfig or a spec string."""
    return focal_tversky_terms(logits, true_masks, n_classes, config)[0]
