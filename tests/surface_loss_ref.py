"""scipy / torch-float64 restatement of the surface loss (DESIGN.md section 3 "Surface loss"), the yardstick of
csrc/surface_loss.hip -- the role tests/contour_metrics_ref.py plays for the contour metrics, whose border and exact squared
distance it reuses.  Per image b and selected class c of int labels [B,H,W]:

    T_c           (label == c); binary head: (label // 2 == c), c = 1
    phi_c[b]      s * float32(sqrt(float64(D_T))), s = -1 inside T_c, +1 outside (so the border pixels are -0.0);
                  all +0.0 when T_c is empty in image b
    surface       1 / (n_mean K) * sum_b sum_x sum_{c in C} p_c(x) phi_c(x), p = sigmoid(z) or softmax(z)_c, in float64
    binary        dL/dz   = g w / n_mean * phi * sigma (1 - sigma)
    multi-class   dL/dz_k = g w / (n_mean K) * p_k * (phi_k [k in C] - sum_{c in C} p_c phi_c)"""
import numpy as np
import torch

from contour_metrics_ref import blob_mask, border, edt_sq


def default_classes(n_classes):
    return (1,) if n_classes == 1 else (2,)


def phi_image(T):
    """float32 [H,W] signed distance map of one boolean target."""
    T = np.asarray(T, bool)
    if not T.any():
        return np.zeros(T.shape, np.float32)
    d2 = edt_sq(border(T))
    phi = np.sqrt(d2.astype(np.float64)).astype(np.float32)
    return np.where(T, -phi, phi)


def phi_maps(labels, classes, binary=False):
    """float32 [K,B,H,W] of int labels [B,H,W]."""
    labels = np.asarray(labels)
    q = labels // 2 if binary else labels
    return np.stack([np.stack([phi_image(q[b] == c) for b in range(q.shape[0])]) for c in classes])


def probabilities(logits, n_classes):
    """float64 [B,C,H,W] logits -> p; the binary head keeps its one channel."""
    return torch.sigmoid(logits) if n_classes == 1 else torch.softmax(logits, dim=1)


def surface_loss(logits, labels, n_classes, classes=None, n_mean=None):
    """logits: torch [B,n_classes,H,W] (computed in float64; autograd reaches them); labels: int array [B,H,W] with the
    dataset's values.  n_mean: the pixel count of the mean (default B H W)."""
    classes = default_classes(n_classes) if classes is None else tuple(classes)
    z = logits.double()
    phi = torch.from_numpy(phi_maps(labels, classes, binary=n_classes == 1)).double()
    p = probabilities(z, n_classes)
    n_mean = float(z.shape[0] * z.shape[2] * z.shape[3]) if n_mean is None else float(n_mean)
    total = z.new_zeros(())
    for k, c in enumerate(classes):
        total = total + (p[:, 0 if n_classes == 1 else c] * phi[k]).sum()
    return total / (n_mean * len(classes))


def closed_form_grad(logits, labels, n_classes, classes=None, n_mean=None, g=1.0, w=1.0):
    """The gradient formulas of the contract, float64 [B,C,H,W]."""
    classes = default_classes(n_classes) if classes is None else tuple(classes)
    z = logits.detach().double()
    phi = torch.from_numpy(phi_maps(labels, classes, binary=n_classes == 1)).double()
    n_mean = float(z.shape[0] * z.shape[2] * z.shape[3]) if n_mean is None else float(n_mean)
    p = probabilities(z, n_classes)
    if n_classes == 1:
        return (g * w / n_mean) * phi[0].unsqueeze(1) * p * (1 - p)
    phik = torch.zeros_like(z)
    for k, c in enumerate(classes):
        phik[:, c] = phi[k]
    dot = (p * phik).sum(dim=1, keepdim=True)                     # phik is 0 outside C
    return (g * w / (n_mean * len(classes))) * p * (phik - dot)


class ClosedFormSurface(torch.autograd.Function):
    """surface_loss with closed_form_grad as its backward: gradcheck compares the formulas with finite differences."""

    @staticmethod
    def forward(ctx, logits, labels, n_classes, classes):
        ctx.save_for_backward(logits)
        ctx.meta = (labels, n_classes, classes)
        return surface_loss(logits.detach(), labels, n_classes, classes)

    @staticmethod
    def backward(ctx, g):
        (logits,) = ctx.saved_tensors
        labels, n_classes, classes = ctx.meta
        return closed_form_grad(logits, labels, n_classes, classes) * g, None, None, None


def blob_labels(rng, B, H, W, cls=2, others=(0, 1)):
    """int64 [B,H,W]: class `cls` on a blob_mask, a random mix of `others` elsewhere."""
    masks = np.stack([blob_mask(rng, H, W) for _ in range(B)])
    rest = rng.choice(np.asarray(others, np.int64), masks.shape)
    return np.where(masks, np.int64(cls), rest)
