"""The loss side of the train step over the C ABI (include/unet_hip.h): the torch.autograd.Function nodes of the default loss
(BCE / CE + Dice + boundary), the Dice metric and the optional terms (surface, focal + Tversky, distillation), with the plumbing
they share.  Every node reads: prologue (the helpers below), its own launches, epilogue.

Node layout: logits [B,H,W] for the one-channel head (its target is mask // mask_div, mask_div = 2) or NHWC [B,H,W,C] for a
softmax head (mask_div = 1), int64 labels [B,H,W].  head_layout() takes the model's [B,n_classes,H,W] there.
Everything here requires GPU tensors: there is no CPU fallback."""
from __future__ import annotations

import ctypes
import math
import os
from typing import Optional, Tuple

import torch
from torch.autograd import Function

from .ops import LIB, _p, _require_gpu, _stream


# ----------------------------------------------------------------------------- what the nodes share
def _logits32(logits: torch.Tensor, what: str = "logits") -> torch.Tensor:
    _require_gpu(logits, what)
    return logits.float().contiguous()


def _label_batch(mask: torch.Tensor) -> torch.Tensor:
    _require_gpu(mask, "labels")
    if mask.dim() != 3:
        raise RuntimeError(f"labels are [B,H,W], got {tuple(mask.shape)}")
    mk = mask.contiguous()
    return mk if mk.dtype == torch.int64 else mk.long()


def _head_of(lg: torch.Tensor, labels_shape, who: str) -> int:
    """ncls of node-layout logits checked against the labels' [B,H,W]: 1 for [B,H,W], C for [B,H,W,C]."""
    if lg.dim() not in (3, 4) or tuple(lg.shape[:3]) != tuple(labels_shape):
        raise RuntimeError(f"{who} expects logits [B,H,W] or [B,H,W,C] matching labels {tuple(labels_shape)}, got {tuple(lg.shape)}")
    ncls = 1 if lg.dim() == 3 else int(lg.shape[-1])
    if ncls == 1 and lg.dim() == 4:
        raise RuntimeError(f"{who}: the one-channel head passes its logits as [B,H,W]")
    return ncls


def _seed_grad(g: torch.Tensor) -> torch.Tensor:
    """The upstream gradient of a scalar term as the kernels read it: fp32 [1] on the device."""
    g0 = g.reshape(1)
    if g0.dtype != torch.float32 or not g0.is_contiguous():
        g0 = g0.contiguous().float()
    return g0


def _grad_out(dl: torch.Tensor, shape, dtype) -> torch.Tensor:
    dl = dl.view(shape)
    return dl if dtype == torch.float32 else dl.to(dtype)


def _c_array(ctype, values):
    return (ctype * len(values))(*values)


def head_layout(logits: torch.Tensor, n_classes: int, who: str = "seg_loss") -> Tuple[torch.Tensor, int]:
    """Model-layout logits [B,n_classes,H,W] (or [B,H,W] for the one-channel head) -> (node-layout logits, mask_div)."""
    if n_classes == 1:
        return (logits.squeeze(1) if logits.dim() == 4 else logits), 2
    if logits.dim() != 4 or logits.shape[1] != n_classes:
        raise ValueError(f"{who} expects logits [B,{n_classes},H,W], got {tuple(logits.shape)}")
    return logits.permute(0, 2, 3, 1), 1


# ----------------------------------------------------------------------------- the default loss, Dice, boundary
def loss_workspace(device) -> torch.Tensor:
    return torch.empty(LIB.query("uh_loss_ws_bytes", 1), dtype=torch.uint8, device=device)


def boundary_loss_value(pred: torch.Tensor, pstride: int, bstride: int, target: torch.Tensor, B: int, H: int, W: int,
                        edge_width: int, edge_weight: float, smooth: float = 1e-6) -> torch.Tensor:
    _require_gpu(pred, "prediction")
    _require_gpu(target, "target")
    out = torch.empty(1, dtype=torch.float32, device=pred.device)
    ws = loss_workspace(pred.device)
    LIB.call("uh_boundary_loss", pred.data_ptr(), pstride, bstride, target.data_ptr(), B, H, W, int(edge_width),
             float(edge_weight), float(smooth), out.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
    return out


def boundary_loss_mask_value(logits: torch.Tensor, mask: torch.Tensor, mask_div: int, edge_width: int, edge_weight: float,
                             smooth: float = 1e-6) -> torch.Tensor:
    """boundary_loss(logits, (mask // mask_div).float(), edge_width, edge_weight) of train.py:134 for logits [B,H,W]: the kernel
    divides the int64 mask itself.  A value without gradient, fp32 [1]."""
    _require_gpu(logits, "logits")
    lg = logits.detach().float().contiguous()
    mk = mask.contiguous()
    if mk.dtype != torch.int64:
        mk = mk.long()
    if mk.dim() != 3 or tuple(lg.shape) != tuple(mk.shape):
        raise RuntimeError(f"boundary loss expects logits and mask [B,H,W], got {tuple(logits.shape)} and {tuple(mask.shape)}")
    B, H, W = mk.shape
    out = torch.empty(1, dtype=torch.float32, device=lg.device)
    ws = loss_workspace(lg.device)
    LIB.call("uh_boundary_loss_mask", lg.data_ptr(), 1, H * W, mk.data_ptr(), int(mask_div), B, H, W, int(edge_width),
             float(edge_weight), float(smooth), out.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
    return out


# Single-process binary loss as three launches (uh_seg_loss_binary_fused) instead of six + glue; False: the separate calls
# (what data-parallel runs use anyway: their sums are all-reduced between the calls).  The two are bit-identical (tests).
FUSE_LOSS = os.environ.get("UH_FUSE_LOSS", "1") != "0"
_LOSS_WS = {}


def _fused_loss_workspace(device) -> torch.Tensor:
    """One workspace per device for the fused loss (its three launches run back to back on one stream; a second stream
    using the loss concurrently on the same device is not a supported pattern of the train step)."""
    key = (device.type, device.index, torch.cuda.current_stream(device).cuda_stream)
    ws = _LOSS_WS.get(key)
    if ws is None:
        ws = _LOSS_WS[key] = torch.empty(LIB.query("uh_seg_loss_fused_ws_bytes"), dtype=torch.uint8, device=device)
    return ws


class SegLossBinaryFn(Function):
    """train.py:119-134 in one node: t = mask // mask_div; BCEWithLogits(mean) + dice_loss(sigmoid) +
    w_boundary * boundary_loss(logits, t, 51, 15).  Returns (total, bce, dice, boundary, nan_flag) as 0-dim tensors; only
    `total` carries gradient (boundary_loss is constant w.r.t. the logits); nan_flag (float 0/1, or None when
    the separate kernels ran) is train.py:149's isnan(loss) without a kernel of its own.
    `reduce_sums` (optional callable) all-reduces the 4 partial sums across data-parallel ranks so the
    Dice ratio and the BCE mean are those of the GLOBAL batch."""

    @staticmethod
    def forward(ctx, logits, mask, mask_div: int, w_boundary: float, edge_width: int, edge_weight: float,
                reduce_sums=None, world: int = 1):
        lg = _logits32(logits)
        if mask.dim() != 3 or lg.numel() != mask.numel():
            raise RuntimeError(f"binary seg loss expects mask [B,H,W] matching the logits, got {tuple(mask.shape)} "
                               f"vs {tuple(logits.shape)}")
        mk = _label_batch(mask)
        B, H, W = mk.shape
        n = lg.numel()
        dev = lg.device
        sums = torch.empty(4, dtype=torch.float32, device=dev)
        out = torch.empty(5, dtype=torch.float32, device=dev)
        fused = FUSE_LOSS and reduce_sums is None
        if fused:
            ws = _fused_loss_workspace(dev)
            LIB.call("uh_seg_loss_binary_fused", lg.data_ptr(), mk.data_ptr(), int(mask_div), B, H, W, int(edge_width),
                     float(edge_weight), 1e-6, float(w_boundary), float(round(n * world)), sums.data_ptr(), out.data_ptr(),
                     ws.data_ptr(), ws.numel(), _stream())
        else:
            ws = loss_workspace(dev)
            LIB.call("uh_bce_dice_sums", lg.data_ptr(), mk.data_ptr(), int(mask_div), None, n, sums.data_ptr(),
                     ws.data_ptr(), ws.numel(), _stream())
            if reduce_sums is not None:
                reduce_sums(sums)
            bl = None
            if w_boundary != 0.0:
                # boundary_loss(logits, (mask // mask_div).float(), 51, 15), train.py:134 -- the kernel divides the int64 mask itself
                bl = torch.empty(1, dtype=torch.float32, device=dev)
                LIB.call("uh_boundary_loss_mask", lg.data_ptr(), 1, H * W, mk.data_ptr(), int(mask_div), B, H, W, int(edge_width),
                         float(edge_weight), 1e-6, bl.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
            LIB.call("uh_seg_loss_binary_finish", sums.data_ptr(), float(round(n * world)), _p(bl), float(w_boundary),
                     out.data_ptr(), _stream())
        ctx.save_for_backward(lg, mk, sums)
        ctx.meta = (int(mask_div), n, world, logits.shape, logits.dtype)
        ctx.set_materialize_grads(False)
        total, bce, dice, bnd = out[0], out[1], out[2], out[3]
        nan_flag = out[4:5] if fused else None
        ctx.mark_non_differentiable(bce, dice, bnd)
        if nan_flag is not None:
            ctx.mark_non_differentiable(nan_flag)
        return total, bce, dice, bnd, nan_flag

    @staticmethod
    def backward(ctx, g_total, *_unused):
        lg, mk, sums = ctx.saved_tensors
        mask_div, n, world, shape, dtype = ctx.meta
        if g_total is None:
            return (None,) * 8
        g0 = _seed_grad(g_total)                  # only the total carries gradient
        dl = torch.empty_like(lg)
        LIB.call("uh_bce_dice_grad", lg.data_ptr(), mk.data_ptr(), mask_div, None, n, sums.data_ptr(),
                 float(round(n * world)), 1.0, 1.0, g0.data_ptr(), dl.data_ptr(), _stream())
        return (_grad_out(dl, shape, dtype),) + (None,) * 7


class SegLossMulticlassFn(Function):
    """train.py:136-142: CrossEntropyLoss + dice_loss(softmax, one_hot, multiclass=True) on NHWC
    fp32 logits [B,H,W,C] (+ optional w_boundary * boundary_loss on channel 1, train.py:143-147)."""

    @staticmethod
    def forward(ctx, logits_nhwc, mask, w_boundary: float, edge_width: int, edge_weight: float,
                reduce_sums=None, world: int = 1):
        lg = _logits32(logits_nhwc)
        B, H, W, C = lg.shape
        npix = B * H * W
        mk = _label_batch(mask)
        dev = lg.device
        sums = torch.empty(1 + 3 * C, dtype=torch.float32, device=dev)
        ws = loss_workspace(dev)
        LIB.call("uh_ce_dice_sums", lg.data_ptr(), mk.data_ptr(), npix, C, sums.data_ptr(), ws.data_ptr(),
                 ws.numel(), _stream())
        if reduce_sums is not None:
            reduce_sums(sums)
        bl = None
        if w_boundary != 0.0:
            # 4-D path of boundary_loss.py:20-23: channel 1 of the logits, target = mask as float
            bl = boundary_loss_value(lg[..., 1], C, H * W * C, mk.float(), B, H, W, edge_width, edge_weight)
        out = torch.empty(4, dtype=torch.float32, device=dev)
        LIB.call("uh_seg_loss_multiclass_finish", sums.data_ptr(), C, float(round(npix * world)), _p(bl),
                 float(w_boundary), out.data_ptr(), _stream())
        ctx.save_for_backward(lg, mk, sums)
        ctx.meta = (npix, C, world, logits_nhwc.shape, logits_nhwc.dtype)
        return out

    @staticmethod
    def backward(ctx, gout):
        lg, mk, sums = ctx.saved_tensors
        npix, C, world, shape, dtype = ctx.meta
        g0 = _seed_grad(gout[0:1])
        dl = torch.empty_like(lg)
        LIB.call("uh_ce_dice_grad", lg.data_ptr(), mk.data_ptr(), npix, C, sums.data_ptr(), float(round(npix * world)),
                 1.0, 1.0, g0.data_ptr(), dl.data_ptr(), _stream())
        return (_grad_out(dl, shape, dtype),) + (None,) * 6


class DiceCoeffFn(Function):
    """dice_coeff (dice_score.py:5-25) over `ngroups` groups of `group_len` elements."""

    @staticmethod
    def forward(ctx, x, t, ngroups: int, group_len: int, eps: float):
        xf = _logits32(x, "input")
        tf = t.float().contiguous()
        dev = xf.device
        sums = torch.empty(ngroups * 3, dtype=torch.float32, device=dev)
        ws = loss_workspace(dev)
        LIB.call("uh_dice_sums", xf.data_ptr(), tf.data_ptr(), ngroups, group_len, sums.data_ptr(), ws.data_ptr(),
                 ws.numel(), _stream())
        out = torch.empty(1, dtype=torch.float32, device=dev)
        LIB.call("uh_dice_from_sums", sums.data_ptr(), ngroups, float(eps), out.data_ptr(), _stream())
        ctx.save_for_backward(tf, sums)
        ctx.meta = (ngroups, group_len, eps, x.shape, x.dtype)
        return out.view(())

    @staticmethod
    def backward(ctx, g):
        tf, sums = ctx.saved_tensors
        ngroups, group_len, eps, shape, dtype = ctx.meta
        s = sums.view(ngroups, 3)
        inter2 = 2 * s[:, 0]
        sets = s[:, 1] + s[:, 2]
        live = sets != 0
        den = sets + eps
        ka = torch.where(live, 2.0 / den, torch.zeros_like(den))
        kb = torch.where(live, -(inter2 + eps) / (den * den), torch.zeros_like(den))
        dx = (ka[:, None] * tf.view(ngroups, group_len) + kb[:, None]) * (g / ngroups)
        return dx.view(shape).to(dtype), None, None, None, None


# ----------------------------------------------------------------------------- surface loss (csrc/surface_loss.hip)
SURFACE_MAX_CLASSES = 8
_SURFACE_WS = {}


class _SurfaceWorkspace:
    """One workspace per (shape, K, device, stream): it carries the squared distances from the value to the gradient of the same
    step.  `generation` counts the value passes that wrote it: a backward that finds another generation than its forward's
    (two losses of one shape in flight) has the distances formed again instead of reading someone else's."""

    def __init__(self, nbytes: int, device):
        self.buf = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=device)
        self.generation = 0


def _surface_workspace(B: int, H: int, W: int, K: int, device) -> _SurfaceWorkspace:
    key = (B, H, W, K, device.type, device.index, torch.cuda.current_stream(device).cuda_stream)
    ws = _SURFACE_WS.get(key)
    if ws is None:
        ws = _SURFACE_WS[key] = _SurfaceWorkspace(LIB.query("uh_surface_loss_ws_bytes", B, H, W, K), device)
    return ws


def surface_classes(classes, n_classes: Optional[int] = None) -> Tuple[int, ...]:
    """The selected classes as a checked tuple of distinct ids (below n_classes where a head is given)."""
    try:
        cls = tuple(int(c) for c in classes)
    except TypeError:
        cls = (int(classes),)
    if not 1 <= len(cls) <= SURFACE_MAX_CLASSES:
        raise ValueError(f"surface loss: 1 to {SURFACE_MAX_CLASSES} classes, got {cls}")
    if len(set(cls)) != len(cls) or min(cls) < 0 or (n_classes is not None and max(cls) >= n_classes):
        raise ValueError(f"surface loss: classes {cls} must be distinct ids in [0, {n_classes if n_classes is not None else 'inf'})")
    return cls


def surface_border(mask: torch.Tensor, classes, mask_div: int = 1) -> torch.Tensor:
    """uint8 [K,B,H,W]: 1 on the border of (mask // mask_div == classes[k]), straight from the int64 labels."""
    cls = surface_classes(classes)
    mk = _label_batch(mask)
    B, H, W = mk.shape
    out = torch.empty(len(cls), B, H, W, dtype=torch.uint8, device=mk.device)
    LIB.call("uh_surface_border_i64", mk.data_ptr(), int(mask_div), _c_array(ctypes.c_int, cls), len(cls), out.data_ptr(), B, H, W,
             _stream())
    return out


def surface_dist_map(mask: torch.Tensor, classes, mask_div: int = 1) -> torch.Tensor:
    """fp32 [K,B,H,W]: the signed distance of every pixel to the contour of (mask // mask_div == classes[k]) in its image,
    negative inside, -0.0 on the border pixels, +0.0 everywhere in an image without the class."""
    cls = surface_classes(classes)
    mk = _label_batch(mask)
    B, H, W = mk.shape
    ws = _surface_workspace(B, H, W, len(cls), mk.device)
    ws.generation += 1                                             # the distances in the workspace are no longer a loss's
    out = torch.empty(len(cls), B, H, W, dtype=torch.float32, device=mk.device)
    LIB.call("uh_surface_dist_map", mk.data_ptr(), int(mask_div), _c_array(ctypes.c_int, cls), len(cls), out.data_ptr(), B, H, W,
             ws.buf.data_ptr(), ws.buf.numel(), _stream())
    return out


class SurfaceLossFn(Function):
    """The surface loss of DESIGN.md section 3 in one node: logits [B,H,W] (ncls = 1, sigmoid; target mask // mask_div) or NHWC
    [B,H,W,C] (softmax), int64 labels [B,H,W], `classes` a tuple of distinct ids.  Returns (w * surface, surface) as 0-dim
    tensors; the first carries the gradient, the second is the logged term.  `reduce_sums` sums the pair over data-parallel ranks
    (the value is normalised by the GLOBAL pixel count n * world; the gradient needs no collective).  Nothing is read back."""

    @staticmethod
    def forward(ctx, logits, mask, mask_div: int, classes, weight: float, reduce_sums=None, world: float = 1):
        lg = _logits32(logits)
        mk = _label_batch(mask)
        B, H, W = mk.shape
        ncls = _head_of(lg, mk.shape, "surface loss")
        cls = surface_classes(classes, ncls if ncls > 1 else None)         # sigmoid head: the id is a value of mask // mask_div
        if ncls == 1 and len(cls) != 1:
            raise ValueError(f"surface loss: the sigmoid head has one map, got classes {cls}")
        n_mean = float(round(B * H * W * world))
        ws = _surface_workspace(B, H, W, len(cls), lg.device)
        out = torch.empty(2, dtype=torch.float32, device=lg.device)
        ws.generation += 1
        LIB.call("uh_surface_loss_sums", lg.data_ptr(), mk.data_ptr(), int(mask_div), _c_array(ctypes.c_int, cls), len(cls), ncls,
                 B, H, W, n_mean, float(weight), out.data_ptr(), ws.buf.data_ptr(), ws.buf.numel(), _stream())
        if reduce_sums is not None:
            reduce_sums(out)
        ctx.save_for_backward(lg, mk)
        ctx.meta = (int(mask_div), cls, ncls, n_mean, float(weight), ws, ws.generation, logits.shape, logits.dtype)
        ctx.set_materialize_grads(False)
        value, weighted = out[0], out[1]
        ctx.mark_non_differentiable(value)
        return weighted, value

    @staticmethod
    def backward(ctx, g_weighted, *_unused):
        if g_weighted is None:
            return (None,) * 7
        lg, mk = ctx.saved_tensors
        mask_div, cls, ncls, n_mean, weight, ws, generation, shape, dtype = ctx.meta
        B, H, W = mk.shape
        g0 = _seed_grad(g_weighted)
        rebuild = ws.generation != generation
        if rebuild:
            ws.generation += 1
        dl = torch.empty_like(lg)
        LIB.call("uh_surface_loss_grad", lg.data_ptr(), mk.data_ptr(), mask_div, _c_array(ctypes.c_int, cls), len(cls), ncls, B, H, W,
                 n_mean, weight, g0.data_ptr(), dl.data_ptr(), int(rebuild), ws.buf.data_ptr(), ws.buf.numel(), _stream())
        return (_grad_out(dl, shape, dtype),) + (None,) * 6


# ----------------------------------------------------------------------------- focal + Tversky loss (csrc/focal_loss.hip)
FOCAL_MAX_CLASSES = 8


def focal_head(n_classes: int, weights=None, classes=None) -> Tuple[Tuple[float, ...], Tuple[int, ...]]:
    """Class weights and Tversky classes checked against a head: `n_classes` = 1 (the one-channel head: two classes, labels
    mask // 2) or 2..8.  Defaults: all weights 1, classes 1..C-1."""
    if isinstance(n_classes, bool) or int(n_classes) != n_classes or not 1 <= n_classes <= FOCAL_MAX_CLASSES:
        raise ValueError(f"focal / Tversky loss: heads of 1 to {FOCAL_MAX_CLASSES} classes, got {n_classes!r}")
    C = 2 if n_classes == 1 else int(n_classes)
    w = (1.0,) * C if weights is None else tuple(float(v) for v in weights)
    if len(w) != C:
        raise ValueError(f"focal / Tversky loss: {len(w)} class weights for a head of {C} classes"
                         + (" (the one-channel head has two: background, foreground)" if n_classes == 1 else ""))
    if not all(math.isfinite(v) and v > 0.0 for v in w):
        raise ValueError(f"focal / Tversky loss: class weights must be finite and > 0, got {w}")
    cls = tuple(range(1, C)) if classes is None else tuple(int(c) for c in classes)
    if not cls or len(set(cls)) != len(cls) or min(cls) < 0 or max(cls) >= C:
        raise ValueError(f"focal / Tversky loss: classes {cls} must be distinct ids in [0, {C})")
    return w, cls


class FocalTverskyLossFn(Function):
    """The focal + Tversky loss of DESIGN.md section 3 in one node: logits [B,H,W] (the one-channel head: two classes on the
    logits (0, z), labels mask // mask_div) or NHWC [B,H,W,C] (softmax), int64 labels [B,H,W]; `weights` one per class (two for
    the one-channel head), `classes` the Tversky subset.  Returns (total, focal, tversky) as 0-dim tensors; only `total` carries
    gradient.  `reduce_sums` sums the 2 + 3 C partial sums over data-parallel ranks between the two passes: value and gradient
    are then those of the GLOBAL batch (`world` is accepted for symmetry with the other loss nodes: the focal term is
    normalised by the reduced sum of weights, not by a pixel count).  Nothing is read back."""

    @staticmethod
    def forward(ctx, logits, mask, mask_div: int, weights, gamma: float, alpha: float, beta: float, classes,
                reduce_sums=None, world: float = 1):
        lg = _logits32(logits)
        mk = _label_batch(mask)
        ncls = _head_of(lg, mk.shape, "focal / Tversky loss")
        w, cls = focal_head(ncls, weights, classes)
        gamma, alpha, beta = float(gamma), float(alpha), float(beta)
        if not (math.isfinite(gamma) and gamma >= 0.0):
            raise ValueError(f"focal / Tversky loss: gamma must be finite and >= 0, got {gamma}")
        if not (math.isfinite(alpha) and math.isfinite(beta) and alpha >= 0.0 and beta >= 0.0 and alpha + beta > 0.0):
            raise ValueError(f"focal / Tversky loss: alpha and beta must be finite and >= 0 with alpha + beta > 0, got {alpha}, {beta}")
        npix = mk.numel()
        dev = lg.device
        sums = torch.empty(LIB.query("uh_focal_tversky_nsums", ncls), dtype=torch.float32, device=dev)
        ws = loss_workspace(dev)
        LIB.call("uh_focal_tversky_sums", lg.data_ptr(), mk.data_ptr(), int(mask_div), npix, ncls, _c_array(ctypes.c_float, w), gamma,
                 sums.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
        if reduce_sums is not None:
            reduce_sums(sums)
        out = torch.empty(3, dtype=torch.float32, device=dev)
        LIB.call("uh_focal_tversky_finish", sums.data_ptr(), ncls, alpha, beta, _c_array(ctypes.c_int, cls), len(cls), out.data_ptr(),
                 _stream())
        ctx.save_for_backward(lg, mk, sums)
        ctx.meta = (int(mask_div), npix, ncls, w, gamma, alpha, beta, cls, logits.shape, logits.dtype)
        ctx.set_materialize_grads(False)
        total, focal, tversky = out[0], out[1], out[2]
        ctx.mark_non_differentiable(focal, tversky)
        return total, focal, tversky

    @staticmethod
    def backward(ctx, g_total, *_unused):
        if g_total is None:
            return (None,) * 10
        lg, mk, sums = ctx.saved_tensors
        mask_div, npix, ncls, w, gamma, alpha, beta, cls, shape, dtype = ctx.meta
        g0 = _seed_grad(g_total)
        dl = torch.empty_like(lg)
        LIB.call("uh_focal_tversky_grad", lg.data_ptr(), mk.data_ptr(), mask_div, npix, ncls, _c_array(ctypes.c_float, w), gamma,
                 alpha, beta, _c_array(ctypes.c_int, cls), len(cls), sums.data_ptr(), g0.data_ptr(), dl.data_ptr(), _stream())
        return (_grad_out(dl, shape, dtype),) + (None,) * 9


# ----------------------------------------------------------------------------- knowledge distillation (csrc/distill_loss.hip)
DISTILL_MAX_CLASSES = 8


class DistillLossFn(Function):
    """The distillation term of DESIGN.md section 3 in one node: student and teacher logits of the same shape, [B,H,W] (the
    one-channel head: two classes on the logits (0, z)) or NHWC [B,H,W,C] (softmax), temperature T > 0, weight w > 0.  Returns
    (w * kd, kd, agree) as 0-dim tensors; only the first carries gradient, and only to the student: the teacher's logits are
    detached.  `reduce_sums` sums the two partial sums over data-parallel ranks between the two passes; value and agreement are
    then those of the GLOBAL batch, n_mean = round(B H W world), and the gradient needs no collective.  Nothing is read back."""

    @staticmethod
    def forward(ctx, student_logits, teacher_logits, T: float, w: float, reduce_sums=None, world: float = 1):
        _require_gpu(student_logits, "student logits")
        _require_gpu(teacher_logits, "teacher logits")
        if student_logits.dim() not in (3, 4) or tuple(student_logits.shape) != tuple(teacher_logits.shape):
            raise RuntimeError(f"distillation expects student and teacher logits of one shape, [B,H,W] or [B,H,W,C], got "
                               f"{tuple(student_logits.shape)} and {tuple(teacher_logits.shape)}")
        ncls = _head_of(student_logits, student_logits.shape[:3], "distillation")
        if not 1 <= ncls <= DISTILL_MAX_CLASSES:
            raise ValueError(f"distillation: heads of 1 to {DISTILL_MAX_CLASSES} classes, got {ncls}")
        T, w = float(T), float(w)
        if not (math.isfinite(T) and T > 0.0):
            raise ValueError(f"distillation: the temperature must be finite and > 0, got {T}")
        if not (math.isfinite(w) and w > 0.0):
            raise ValueError(f"distillation: the weight must be finite and > 0, got {w}")
        lg = _logits32(student_logits.detach(), "student logits")
        tl = _logits32(teacher_logits.detach(), "teacher logits")
        B, H, W = lg.shape[:3]
        npix = B * H * W
        n_mean = float(round(npix * world))
        dev = lg.device
        sums = torch.empty(LIB.query("uh_distill_nsums"), dtype=torch.float32, device=dev)
        ws = loss_workspace(dev)
        LIB.call("uh_distill_sums", lg.data_ptr(), tl.data_ptr(), npix, ncls, T, sums.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
        if reduce_sums is not None:
            reduce_sums(sums)
        out = torch.empty(3, dtype=torch.float32, device=dev)
        LIB.call("uh_distill_finish", sums.data_ptr(), n_mean, T, w, out.data_ptr(), _stream())
        ctx.save_for_backward(lg, tl)
        ctx.meta = (npix, ncls, n_mean, T, w, student_logits.shape, student_logits.dtype)
        ctx.set_materialize_grads(False)
        weighted, kd, agree = out[0], out[1], out[2]
        ctx.mark_non_differentiable(kd, agree)
        return weighted, kd, agree

    @staticmethod
    def backward(ctx, g_weighted, *_unused):
        if g_weighted is None:
            return (None,) * 6
        lg, tl = ctx.saved_tensors
        npix, ncls, n_mean, T, w, shape, dtype = ctx.meta
        g0 = _seed_grad(g_weighted)
        dl = torch.empty_like(lg)
        LIB.call("uh_distill_grad", lg.data_ptr(), tl.data_ptr(), npix, ncls, n_mean, T, w, g0.data_ptr(), dl.data_ptr(), _stream())
        return (_grad_out(dl, shape, dtype),) + (None,) * 5
