"""The distance-weighted surface loss of Kervadec et al. on the device (csrc/surface_loss.hip; the reference has no
counterpart; DESIGN.md section 3 "Surface loss").  Per image b and selected class c:

    T_c           (label == c) for a multi-class head; (label // 2 == 1) for the binary head, the target BCE uses
    S(T), D_T[x]  border and exact squared distance as the contour metrics define them (utils/contour_metrics.py)
    phi_c[b,y,x]  s * float32(sqrt(float64(D_T[x]))), s = -1 inside T_c, +1 outside; -0.0 on the border pixels; +0.0 everywhere
                  in an image without the class, which then has no gradient for it
    surface       1 / (n_mean K) * sum_b sum_x sum_{c in C} p_c(x) phi_c(x), p = sigmoid or softmax, K = |C|

    surface_distance_map(labels, classes, binary=False)   -> fp32 [K,B,H,W] maps, on the device
    surface_loss(logits, labels, n_classes, classes=None)  -> 0-dim tensor with gradient, next to boundary_loss

The maps are rebuilt from the labels of every call: a step that augments its labels on the device gets the maps of the
labels it trains on.  The default class is the one `evaluate` scores: the foreground of a binary head, class 2 otherwise."""
from __future__ import annotations

from typing import Optional, Tuple

import torch


def default_classes(n_classes: int) -> Tuple[int, ...]:
    """The class `evaluate` scores: the foreground (target value 1) of a binary head, class 2 for n_classes >= 3."""
    if n_classes == 1:
        return (1,)
    if n_classes >= 3:
        return (2,)
    raise ValueError("surface loss: a 2-class head has no default class; pass classes=")


def head_classes(n_classes: int, classes=None) -> Tuple[int, ...]:
    """`classes` checked against the head.  The binary head has one map, the foreground's."""
    from .. import losses
    if classes is None:
        return default_classes(n_classes)
    if n_classes == 1:
        cls = losses.surface_classes(classes)
        if cls != (1,):
            raise ValueError(f"surface loss: the binary head has one class, the foreground (1); got {cls}")
        return cls
    return losses.surface_classes(classes, n_classes)


def surface_distance_map(labels: torch.Tensor, classes, *, binary: bool = False) -> torch.Tensor:
    """Signed distance maps fp32 [K,B,H,W] of int labels [B,H,W] (or [H,W]) on the GPU, one per class id in `classes`.
    binary=True: the labels are the dataset's {0,1,2} and class c means (label // 2 == c), the binary head's target."""
    from .. import losses
    if labels.dim() == 2:
        labels = labels.unsqueeze(0)
    return losses.surface_dist_map(labels, classes, 2 if binary else 1)


def surface_loss(logits: torch.Tensor, labels: torch.Tensor, n_classes: int, classes=None) -> torch.Tensor:
    """logits [B,n_classes,H,W] (or [B,H,W] for the binary head) as the model returns them, labels int [B,H,W] with the
    dataset's values (NOT yet // 2).  Returns the surface term; its gradient reaches the logits."""
    from .. import losses
    cls = head_classes(n_classes, classes)
    lg, mask_div = losses.head_layout(logits, n_classes, "surface_loss")
    weighted, _ = losses.SurfaceLossFn.apply(lg, labels, mask_div, cls, 1.0, None, 1)
    return weighted
