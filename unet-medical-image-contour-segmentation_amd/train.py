"""The optimizer step of /root/reference/train.py:113-159 on the HIP path.

    seg_loss(...)     loss assembly of train.py:118-142 over the nodes of losses.py: the base node (BCE / CE + Dice, or
                      focal + Tversky), then the surface term, then the distillation term
    FusedRMSprop      clip_grad_norm_(1.0) + RMSprop(lr, weight_decay=1e-8, momentum=0.999) of
                      train.py:80-81,157-158 as two passes over one flat fp32 buffer; optionally an exponential moving
                      average of the parameters in the same pass (EmaConfig), and state_dict / load_state_dict
    FusedAdamW, FusedSGD   the same pass (FusedOptimizer) under torch.optim.AdamW's and torch.optim.SGD's (Nesterov) rule,
                      chosen with OptimConfig / TrainStepper(optimizer=...) / --optimizer
    train_step(...)   zero_grad -> forward (autocast) -> loss -> NaN check -> backward -> clip -> step
    TrainStepper      model + optimizer (+ data-parallel sync) bundle used by bench.py
    train_model(...)  the epoch loop of train.py:29-220 on a user-supplied iterable of batches
    main(argv)        `python -m unet_amd.train`: the reference's command line over a data directory (train_cli.py)
A reference-style loop with torch.optim.RMSprop / clip_grad_norm_ on `model.parameters()` also
works unchanged: the modules are ordinary nn.Modules.
"""
from __future__ import annotations

import contextlib
import dataclasses
import math
import os
import weakref
from typing import Dict, Iterable, Optional, Union

import torch
import torch.nn as nn

from . import dp as dpmod
from . import losses
from . import ops
from ._lib import LIB


# ----------------------------------------------------------------------------------- loss
def _add_term(terms: Dict[str, torch.Tensor], weighted: torch.Tensor, **reported) -> None:
    """total += weighted; `reported` joins the terms.  The fused loss's NaN flag was formed without the new term and is dropped:
    train_step tests the new total itself."""
    terms["loss"] = terms["loss"] + weighted
    terms.update(reported)
    terms.pop("nan_flag", None)


def _pair_terms(lg: torch.Tensor, true_masks: torch.Tensor, mask_div: int, boundary_weight, reduce_sums, world):
    """The default base node: BCE + Dice + 0.25 boundary for the one-channel head (train.py:119-134), CE + Dice otherwise
    (train.py:136-142; its boundary term, train.py:143-147, is commented out: weight 0)."""
    if lg.dim() == 3:
        w_b = 0.25 if boundary_weight is None else boundary_weight
        total, bce, dice, bnd, nan_flag = losses.SegLossBinaryFn.apply(lg, true_masks, mask_div, w_b, 51, 15.0, reduce_sums, world)
        terms = {"loss": total, "bce": bce, "dice": dice, "boundary": bnd}
        if nan_flag is not None:
            terms["nan_flag"] = nan_flag          # float 0 / 1 written by the loss's finishing block (train.py:149)
        return terms
    w_b = 0.0 if boundary_weight is None else boundary_weight
    out = losses.SegLossMulticlassFn.apply(lg, true_masks, w_b, 51, 7.0, reduce_sums, world)
    return {"loss": out[0], "ce": out[1].detach(), "dice": out[2].detach(), "boundary": out[3].detach()}


def _focal_tversky_terms(masks_pred: torch.Tensor, true_masks: torch.Tensor, n_classes: int, loss, boundary_weight, reduce_sums,
                         world) -> Dict[str, torch.Tensor]:
    """The base node with `loss` (a LossConfig): focal + tversky (DESIGN.md section 3 "Focal / Tversky loss") in place of the
    CE + Dice pair, + w_b * boundary_loss as the pair has it (a value without gradient, per rank)."""
    from .utils.focal_loss import focal_tversky_terms
    w_b = (0.25 if n_classes == 1 else 0.0) if boundary_weight is None else float(boundary_weight)
    total, focal, tversky = focal_tversky_terms(masks_pred, true_masks, n_classes, loss, reduce_sums=reduce_sums, world=world)
    terms = {"loss": total, "focal": focal, "tversky": tversky}
    if w_b == 0.0:
        terms["boundary"] = torch.zeros((), dtype=torch.float32, device=total.device)
        return terms
    lg, mask_div = losses.head_layout(masks_pred.detach(), n_classes)
    if n_classes == 1:
        bnd = losses.boundary_loss_mask_value(lg, true_masks, mask_div, 51, 15.0)[0]                               # train.py:134
    else:
        lg = lg.float().contiguous()
        B, H, W, C = lg.shape
        bnd = losses.boundary_loss_value(lg[..., 1], C, H * W * C, true_masks.float(), B, H, W, 51, 7.0)[0]
    terms["loss"] = total + w_b * bnd
    terms["boundary"] = bnd
    return terms


def seg_loss(masks_pred: torch.Tensor, true_masks: torch.Tensor, n_classes: int, *, reduce_sums=None, world: float = 1,
             boundary_weight: Optional[float] = None, surface_weight: float = 0.0, surface_classes=None,
             loss=None, distill=None, teacher_logits: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """train.py:118-142.  masks_pred: logits [B,n_classes,H,W] (as returned by the model);
    true_masks: int64 [B,H,W] with the dataset's values {0,1,2,..} (NOT yet // 2).
    surface_weight != 0 adds surface_weight * surface loss over `surface_classes` (default: the class evaluate scores) and the
    term "surface"; with 0 nothing else is launched and the result is what it is without the option.
    loss (a utils.focal_loss.LossConfig or its spec string; default None: the code path, the launches and the results are what
    they are without the option): the class-weighted focal + Tversky node replaces the CE + Dice pair, and the terms carry
    "focal" and "tversky" in place of "ce" / "bce" and "dice"; the boundary and surface terms stay on top.
    distill (a utils.distill.DistillConfig or its spec string; default None: nothing is launched, allocated or imported for it)
    with teacher_logits (the teacher's logits for the same images, shaped like masks_pred): adds w * kd after the surface term,
    and the terms carry "kd" and "kd_agree"."""
    if loss is None:
        lg, mask_div = losses.head_layout(masks_pred, n_classes)
        terms = _pair_terms(lg, true_masks, mask_div, boundary_weight, reduce_sums, world)
    else:
        terms = _focal_tversky_terms(masks_pred, true_masks, n_classes, loss, boundary_weight, reduce_sums, world)
        # (the surface term's view of masks_pred is made behind the focal node, which has one of its own: autograd sums the
        # nodes' gradients in the reverse order of their views, and three fp32 summands do not commute)
        lg, mask_div = losses.head_layout(masks_pred, n_classes)
    if surface_weight:
        # DESIGN.md section 3 "Surface loss"
        from .utils.surface_loss import head_classes
        weighted, value = losses.SurfaceLossFn.apply(lg, true_masks, mask_div, head_classes(n_classes, surface_classes),
                                                     float(surface_weight), reduce_sums, world)
        _add_term(terms, weighted, surface=value)
    if distill is not None:
        # DESIGN.md section 3 "Distillation"
        from .utils.distill import distill_terms
        if teacher_logits is None:
            raise ValueError("seg_loss: distill=... needs teacher_logits (Distiller.teacher_logits(images))")
        weighted, kd, agree = distill_terms(masks_pred, teacher_logits, n_classes, distill, reduce_sums=reduce_sums, world=world)
        _add_term(terms, weighted, kd=kd, kd_agree=agree)
    return terms


# ----------------------------------------------------------------------------------- optimizer
@dataclasses.dataclass(frozen=True)
class EmaConfig:
    """The exponential moving average of the parameters kept by the fused optimizer: e <- e + (1 - d_t) (p - e) after every
    update, d_t = min(decay, (1 + t) / (warmup + t)) at the t-th update (0-based) when warmup > 0, else decay.  The
    average starts as a copy of the parameters, so it needs no bias correction; the warm-up lets it follow the fast first
    updates instead of holding on to the initialisation for 1 / (1 - decay) steps."""
    decay: float = 0.999
    warmup: int = 10

    def __post_init__(self):
        if not (isinstance(self.decay, (int, float)) and not isinstance(self.decay, bool) and 0.0 < float(self.decay) < 1.0):
            raise ValueError(f"EmaConfig: decay lies in (0, 1), not {self.decay!r}")
        if isinstance(self.warmup, bool) or int(self.warmup) != self.warmup or self.warmup < 0:
            raise ValueError(f"EmaConfig: warmup is an integer >= 0, not {self.warmup!r}")

    @classmethod
    def parse(cls, spec: str) -> "EmaConfig":
        """'DECAY[,warmup=N]' -> config, e.g. '0.999,warmup=10'; ValueError names what is wrong."""
        parts = [t.strip() for t in str(spec).split(",")]
        if not parts[0]:
            raise ValueError(f"EmaConfig.parse: the decay is missing in {spec!r}")
        try:
            vals = {"decay": float(parts[0])}
        except ValueError:
            raise ValueError(f"EmaConfig.parse: decay {parts[0]!r} is not a number") from None
        for tok in parts[1:]:
            name, eq, val = (t.strip() for t in tok.partition("="))
            if name != "warmup" or not eq or "warmup" in vals:
                raise ValueError(f"EmaConfig.parse: {tok!r} is not warmup=N (once) in {spec!r}")
            try:
                vals["warmup"] = int(val)
            except ValueError:
                raise ValueError(f"EmaConfig.parse: warmup {val!r} is not an integer") from None
        return cls(**vals)

    def spec(self) -> str:
        """The canonical spec: EmaConfig.parse(cfg.spec()) == cfg."""
        return f"{float(self.decay)!r},warmup={int(self.warmup)}"

    @classmethod
    def of(cls, ema: Union[None, str, "EmaConfig"]) -> Optional["EmaConfig"]:
        """None, a spec string or a config -> None or a config."""
        if ema is None or isinstance(ema, cls):
            return ema
        if isinstance(ema, str):
            return cls.parse(ema)
        raise TypeError(f"ema is an EmaConfig or a spec string, not {type(ema).__name__}")


_OPTIM_RULES = {      # rule -> its keys and their defaults (adamw: torch's, sgd: nnU-Net's, rmsprop: the reference's train.py)
    "adamw": dict(betas=(0.9, 0.999), eps=1e-8, wd=0.01),
    "sgd": dict(momentum=0.99, nesterov=True, wd=3e-5),
    "rmsprop": dict(alpha=0.99, eps=1e-8, momentum=0.999, wd=1e-8),
}


@dataclasses.dataclass(frozen=True)
class OptimConfig:
    """The update rule of the fused optimizer pass and its hyper-parameters (TrainStepper(optimizer=...), --optimizer):
        adamw[,betas=B1/B2][,eps=E][,wd=W]                      torch.optim.AdamW, defaults 0.9/0.999, 1e-8, 0.01
        sgd[,momentum=M][,nesterov|plain][,wd=W]                torch.optim.SGD(dampening=0), defaults 0.99, nesterov, 3e-5
        rmsprop[,alpha=A][,eps=E][,momentum=M][,wd=W]           torch.optim.RMSprop, defaults 0.99, 1e-8, 0.999, 1e-8
    A field that does not belong to the rule is None.  The learning rate is not part of it: it stays the stepper's `lr`, a
    kernel argument read from param_groups[0]["lr"] at every step."""
    rule: str = "rmsprop"
    betas: Optional[tuple] = None
    eps: Optional[float] = None
    wd: Optional[float] = None
    momentum: Optional[float] = None
    alpha: Optional[float] = None
    nesterov: Optional[bool] = None

    def __post_init__(self):
        if self.rule not in _OPTIM_RULES:
            raise ValueError(f"OptimConfig: the rule is one of {', '.join(_OPTIM_RULES)}, not {self.rule!r}")
        own = _OPTIM_RULES[self.rule]
        for k in ("betas", "eps", "wd", "momentum", "alpha", "nesterov"):
            v = getattr(self, k)
            if k not in own:
                if v is not None:
                    raise ValueError(f"OptimConfig: {k} does not belong to {self.rule}")
                continue
            object.__setattr__(self, k, self._checked(k, own[k] if v is None else v))
        if self.nesterov and self.momentum == 0.0:
            raise ValueError("OptimConfig: nesterov needs momentum > 0 (momentum=0 is plain SGD)")

    @staticmethod
    def _checked(k: str, v):
        """The value of key k in its canonical type; ValueError says what it should have been."""
        if k == "betas":
            try:
                b = (float(v[0]), float(v[1])) if len(v) == 2 else None
            except (TypeError, ValueError):
                b = None
            if b is None or not all(0.0 <= x < 1.0 for x in b):
                raise ValueError(f"OptimConfig: betas are two numbers in [0, 1), not {v!r}")
            return b
        if k == "nesterov":
            return bool(v)
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not (0.0 <= float(v) < math.inf) or (k == "alpha" and v > 1.0):
            raise ValueError(f"OptimConfig: {k} is a number " + ("in [0, 1]" if k == "alpha" else ">= 0") + f", not {v!r}")
        return float(v)

    @classmethod
    def parse(cls, spec: str) -> "OptimConfig":
        """'RULE[,key=value ...]' -> config, e.g. 'adamw,betas=0.9/0.99,wd=0.05' or 'sgd,momentum=0.9,plain'; ValueError names
        the token that is wrong."""
        parts = [t.strip() for t in str(spec).split(",")]
        rule = parts[0]
        if rule not in _OPTIM_RULES:
            raise ValueError(f"OptimConfig.parse: the rule {rule!r} in {spec!r} is none of {', '.join(_OPTIM_RULES)}")
        own, vals, toks = _OPTIM_RULES[rule], {}, {}
        for tok in parts[1:]:
            name, eq, val = (t.strip() for t in tok.partition("="))
            if name in ("nesterov", "plain") and not eq:
                name, val = "nesterov", name == "nesterov"
            elif not eq or not val:
                raise ValueError(f"OptimConfig.parse: {tok!r} is not key=value in {spec!r}")
            if name not in own:
                raise ValueError(f"OptimConfig.parse: {tok!r} does not belong to {rule} (its keys: {', '.join(own)}) in {spec!r}")
            if name in vals:
                raise ValueError(f"OptimConfig.parse: {tok!r} gives {name} a second time in {spec!r}")
            try:
                if name == "betas":
                    b1, slash, b2 = val.partition("/")
                    if not slash:
                        raise ValueError
                    val = (float(b1), float(b2))
                elif name != "nesterov":
                    val = float(val)
            except ValueError:
                raise ValueError(f"OptimConfig.parse: {tok!r} is not " + ("betas=B1/B2" if name == "betas" else f"{name}=NUMBER")
                                 + f" in {spec!r}") from None
            try:
                vals[name] = cls._checked(name, val)
            except ValueError as e:
                raise ValueError(f"OptimConfig.parse: {tok!r} in {spec!r}: {e}") from None
            toks[name] = tok
        if vals.get("nesterov", own.get("nesterov")) and vals.get("momentum") == 0.0:
            raise ValueError(f"OptimConfig.parse: {toks['momentum']!r} in {spec!r}: nesterov needs momentum > 0 "
                             "(say 'plain' for SGD without momentum)")
        return cls(rule=rule, **vals)

    def spec(self) -> str:
        """The canonical spec, every key of the rule spelled out: OptimConfig.parse(cfg.spec()) == cfg."""
        out = [self.rule]
        for k in sorted(_OPTIM_RULES[self.rule]):
            v = getattr(self, k)
            if k == "betas":
                out.append(f"betas={v[0]!r}/{v[1]!r}")
            elif k == "nesterov":
                out.append("nesterov" if v else "plain")
            else:
                out.append(f"{k}={v!r}")
        return ",".join(out)

    @classmethod
    def of(cls, optimizer: Union[None, str, "OptimConfig"]) -> Optional["OptimConfig"]:
        """None, a spec string or a config -> None or a config."""
        if optimizer is None or isinstance(optimizer, cls):
            return optimizer
        if isinstance(optimizer, str):
            return cls.parse(optimizer)
        raise TypeError(f"optimizer is an OptimConfig or a spec string, not {type(optimizer).__name__}")


class FusedOptimizer:
    """clip_grad_norm_ + one update rule over ONE flat buffer: everything of the fused pass that is not the rule.  The rules
    are the subclasses FusedRMSprop, FusedAdamW and FusedSGD; each owns its state buffers and launches its own kernel.

    Every parameter is re-pointed at a view of `flat_p` (values preserved, strides preserved, so
    channels_last weights stay channels_last); gradients are gathered into `flat_g` by
    post-accumulate hooks in backward-ready order, which is also the bucket order of the
    data-parallel all-reduce.

    ema_decay (default None: off -- nothing is allocated and the launches are what they are without the option): keep an
    exponential moving average of the parameters in `flat_ema`, laid out like `flat_p` and initialised to a copy of it,
    updated inside the same pass (the rule's _ema entry point) with the decay of EmaConfig(ema_decay, ema_warmup) at update
    number `ema_updates` (a device int32[1], advanced once per applied step by uh_ema_tick: a step skipped for a non-finite
    gradient norm does not count).  A parameter skipped as stale (no gradient this step) keeps its average untouched, like
    the rest of its state.  Data parallel: the average is a function of parameters that are identical on every rank, so
    every rank keeps the same one without communication.  swap_ema() exchanges the parameters and their average in place."""

    KIND = None                  # the "kind" of state_dict()
    HYPER = ()                   # the keys of param_groups[0] beside "lr"

    def __init__(self, params: Iterable[nn.Parameter], defaults: Dict, gradient_clipping: float = 1.0,
                 process_group=None, bucket_bytes: int = 8 << 20, ema_decay: Optional[float] = None, ema_warmup: int = EmaConfig.warmup):
        name = type(self).__name__
        plist = [p for p in params if p.requires_grad]
        if not plist:
            raise ValueError(f"{name} got no parameters")
        dev = plist[0].device
        if dev.type != "cuda":
            raise RuntimeError(f"{name} needs parameters on the GPU (no CPU fallback)")
        self.params = list(reversed(plist))          # backward produces gradients roughly in this order
        self.defaults = dict(defaults)
        self.param_groups = [dict(self.defaults, params=self.params)]
        self.gradient_clipping = float(gradient_clipping) if gradient_clipping else 0.0
        slices, off = [], 0
        for p in self.params:
            n = p.numel()
            slices.append((off, n))
            off += (n + 3) // 4 * 4                  # keep every slice 16-byte aligned
        self.total = off
        self.slices = slices
        self.flat_p = torch.zeros(off, dtype=torch.float32, device=dev)
        self.flat_g = torch.zeros(off, dtype=torch.float32, device=dev)
        self._alloc_state(off, dev)
        self.norm = torch.zeros(1, dtype=torch.float32, device=dev)
        self.ws = torch.empty(LIB.query("uh_optim_ws_bytes", off), dtype=torch.uint8, device=dev)
        self._index = {}
        self._grad_keys = []
        self._hooks = []
        self._closed = False
        # one backward per step: which slices of flat_g hold THIS step's gradient (reset by zero_grad / step)
        self._fresh = [False] * len(self.params)
        self._stale_verified = None                  # data parallel: the fresh / stale pattern of the last step (agreed on the first)
        self._probe, self._probe_code = None, None
        with torch.no_grad():
            for i, (p, (o, n)) in enumerate(zip(self.params, slices)):
                if p.dtype != torch.float32:
                    raise RuntimeError(f"{name} expects fp32 master parameters")
                if not _is_dense(p):
                    raise RuntimeError("parameters must be dense (contiguous or channels_last)")
                # a parameter belongs to ONE FusedOptimizer: a stale owner's hook would steal the gradient (it fires first,
                # copies p.grad into its dead buffer and clears it), so an earlier owner is closed here (take-over)
                prev = getattr(p, "_uh_owner", None)
                prev = prev() if prev is not None else None
                if prev is not None and prev is not self:
                    prev.close()
                view = torch.as_strided(self.flat_p, p.shape, p.stride(), o)
                view.copy_(p)
                p.data = view
                self._index[id(p)] = i
                p._uh_owner = weakref.ref(self)
                # backward kernels write this parameter's gradient straight into the flat buffer (ops.GRAD_DST)
                ops.GRAD_DST[view.data_ptr()] = (torch.as_strided(self.flat_g, p.shape, p.stride(), o),
                                                 _weak_callback(self, i))
                self._grad_keys.append(view.data_ptr())
                # the hook holds the optimizer weakly (a bound method would keep it -- and its four flat buffers --
                # alive for as long as the parameter lives) and its handle is kept so that close() can remove it
                self._hooks.append(p.register_post_accumulate_grad_hook(_weak_grad_hook(self)))
        self.sync = None
        if dpmod.sync_enabled(process_group):
            self.sync = dpmod.BucketedGradSync(self.flat_g, slices, bucket_bytes, process_group)
        self.ema = EmaConfig(float(ema_decay), ema_warmup) if ema_decay is not None else None
        self.flat_ema = self.ema_updates = None
        if self.ema is not None:
            self.flat_ema = self.flat_p.clone()
            self.ema_updates = torch.zeros(1, dtype=torch.int32, device=dev)

    def close(self):
        """Detach from the parameters: hooks removed, in-place gradient destinations unregistered.  The parameters keep
        their current values (they stay views of this optimizer's flat buffer until someone re-points them)."""
        if getattr(self, "_closed", True):
            return
        self._closed = True
        for h in self._hooks:
            h.remove()
        self._hooks = []
        for k in self._grad_keys:
            ent = ops.GRAD_DST.get(k)
            if ent is not None and ent[0].untyped_storage().data_ptr() == self.flat_g.untyped_storage().data_ptr():
                ops.GRAD_DST.pop(k, None)
        self._grad_keys = []
        for p in self.params:
            ref = getattr(p, "_uh_owner", None)
            if ref is not None and ref() in (self, None):
                p._uh_owner = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _mark(self, i: int, event=None):
        if self._fresh[i]:
            raise RuntimeError(f"{type(self).__name__}: a second gradient for the same parameter arrived before step(): the backward "
                               "kernels overwrite the flat gradient buffer, so gradient accumulation over several "
                               "backward() calls is not supported (call zero_grad() + step() once per backward)")
        self._fresh[i] = True
        if self.sync is not None:
            self.sync.mark_ready(i, event)

    def _written(self, i: int, event=None):
        if not self._closed:
            self._mark(i, event)

    def _on_grad(self, p: torch.Tensor):
        if self._closed:
            return
        i = self._index[id(p)]
        o, n = self.slices[i]
        g = p.grad
        if g is None:            # written in place by the backward kernel (ops.GRAD_DST); readiness came via _written
            return
        torch.as_strided(self.flat_g, p.shape, p.stride(), o).copy_(g)     # parameters without an in-place writer
        p.grad = None
        self._mark(i)

    def zero_grad(self, set_to_none: bool = True):
        for p in self.params:
            p.grad = None
        self._fresh = [False] * len(self.params)

    def abort_step(self):
        """Drop the gradients of the current backward without applying them (NaN loss, train.py:149-151): the side
        stream and any gradient all-reduce already in flight are drained so that the next step starts clean."""
        if ops.STEP.wgrad_stream is not None:
            torch.cuda.current_stream().wait_stream(ops.STEP.wgrad_stream)
        if self.sync is not None:
            self.sync.wait()
        self._fresh = [False] * len(self.params)

    @staticmethod
    def _pattern_code(pattern) -> float:
        """A small integer (exact in fp32, its square times the world size too) that names a fresh / stale pattern."""
        return float(1 + sum((i + 1) * 7919 for i, f in enumerate(pattern) if f) % 4093)

    def pattern_probe(self) -> Optional[torch.Tensor]:
        """Data parallel: [c, c^2] of the pattern the LAST step ran with (device tensor, rewritten only when the pattern changes).
        train_step appends it to the NaN-flag all-reduce every rank issues every step anyway: sum(c^2) * world == sum(c)^2 iff
        every rank had the same pattern."""
        if self.sync is None or self._stale_verified is None:
            return None
        code = self._pattern_code(self._stale_verified)
        if self._probe is None or self._probe_code != code:
            self._probe = torch.tensor([code, code * code], dtype=torch.float32, device=self.flat_g.device)
            self._probe_code = code
        return self._probe

    def _check_stale_pattern(self):
        """Data parallel: "skip a parameter that got no gradient" is only what torch.optim + DDP do when EVERY rank skips it
        (behind DDP's all-reduce .grad is non-None on every rank).  A parameter that is fresh on one rank and stale on another
        would be updated on one replica only, silently.  The pattern is therefore compared across the ranks on the first
        step (one tiny all-reduce + host read, once).  Afterwards it MAY change -- freezing or unfreezing layers mid-run is
        legal with torch.optim + DDP -- as long as it changes on every rank alike: each step's pattern rides, as a checksum, in
        the NEXT step's NaN-flag all-reduce (pattern_probe; a collective every rank issues every step, so nobody can be left
        waiting), and a mismatch raises on all ranks together, one step late.  U-Net uses every parameter on every step."""
        pattern = tuple(self._fresh)
        if self._stale_verified is None:
            import torch.distributed as dist
            bits = torch.tensor([1.0 if f else 0.0 for f in pattern], dtype=torch.float32, device=self.flat_g.device)
            both = torch.stack([bits, -bits])
            dist.all_reduce(both, op=dist.ReduceOp.MAX, group=self.sync.group)     # max(bits), -min(bits)
            if bool((both[0] != -both[1]).any().item()):
                # (every rank takes this branch: the buckets are drained and the step is abandoned before anyone raises)
                self.sync.wait()
                self._fresh = [False] * len(self.params)
                raise RuntimeError(f"{type(self).__name__} (data parallel): a parameter received a gradient on some ranks and none on "
                                   "others; the replicas would diverge (give every rank the same set of trainable / used "
                                   "parameters)")
        self._stale_verified = pattern

    def check_probe(self, s1: float, s2: float, world: int):
        """Host side of pattern_probe: s1 = sum of the ranks' codes, s2 = sum of their squares (read with the NaN flag)."""
        if abs(s2 * world - s1 * s1) > 0.5:
            self.abort_step()
            raise RuntimeError(f"{type(self).__name__} (data parallel): in the previous step the set of parameters that received gradients "
                               "differed between the ranks; the replicas have diverged by one update (give every rank the same "
                               "set of trainable / used parameters)")

    @torch.no_grad()
    def step(self):
        if self._closed:
            raise RuntimeError(f"{type(self).__name__}.step() after close() (another {type(self).__name__} took the parameters over)")
        ops.flush_slabs()
        if ops.STEP.wgrad_stream is not None:
            torch.cuda.current_stream().wait_stream(ops.STEP.wgrad_stream)     # weight gradients written on the side stream
        # A parameter that received no gradient this step is SKIPPED, as torch.optim skips parameters whose .grad is None
        # (an unused or frozen parameter must not drift under weight decay / momentum): its slice of the flat gradient is
        # zeroed -- so that it adds nothing to the clipping norm and a data-parallel peer that did produce a gradient still
        # meets a matching all-reduce -- and the update runs over the contiguous runs of fresh slices only.
        stale = [i for i, f in enumerate(self._fresh) if not f]
        if stale and len(stale) == len(self._fresh):
            raise RuntimeError(f"{type(self).__name__}.step() without a backward pass since the last step / zero_grad")
        runs = [(0, self.total)]
        if stale:
            for i in stale:
                o, n = self.slices[i]
                self.flat_g[o:o + n].zero_()
                if self.sync is not None:
                    self.sync.mark_ready(i)
            runs, start = [], None
            for i, (o, n) in enumerate(self.slices):
                end = o + (n + 3) // 4 * 4
                if self._fresh[i]:
                    if start is None:
                        start = o
                    last = end
                elif start is not None:
                    runs.append((start, last - start))
                    start = None
            if start is not None:
                runs.append((start, last - start))
        if self.sync is not None:
            # (behind the stale slices' mark_ready: every bucket has been issued -- in index order on every rank -- so the
            # comparison's own all-reduce sits at the same place in every rank's sequence of collectives)
            self._check_stale_pattern()
        self._fresh = [False] * len(self.params)
        if self.sync is not None:
            self.sync.wait()
        g = self.param_groups[0]
        st = torch.cuda.current_stream().cuda_stream
        LIB.call("uh_grad_sumsq", self.flat_g.data_ptr(), self.total, self.norm.data_ptr(), self.ws.data_ptr(),
                 self.ws.numel(), st)
        for o, n in runs:
            self._launch(o, n, g, st)
        # behind every run's launch: all of them read the same step and update numbers
        for counter in self.counters():
            LIB.call("uh_ema_tick", counter.data_ptr(), self.norm.data_ptr(), st)
        ops.WEIGHT_EPOCH += 1        # parameters changed behind torch's version counters (see ops.packed_w3x3_cached)
        return self.norm

    # ---- what a rule provides
    def _alloc_state(self, total: int, dev):
        """Allocate the rule's zeroed state buffers (and its step counter, if it has one)."""
        raise NotImplementedError

    def _launch(self, o: int, n: int, g: Dict, st: int):
        """Enqueue the rule's kernel (its _ema form when self.ema is set) over the n floats at offset o of the flat buffers."""
        raise NotImplementedError

    def _rule_state(self) -> Dict[str, torch.Tensor]:
        """state_dict key -> the rule's flat state buffer, in the order of the kernel's arguments."""
        raise NotImplementedError

    step_count = None            # a device int32[1] of applied steps where the rule needs one (FusedAdamW)

    def counters(self):
        """The device int32[1] counters uh_ema_tick advances once per applied step."""
        return [c for c in (self.step_count, self.ema_updates) if c is not None]

    def state_tensors(self):
        """Every device tensor a step changes beside the gradient: the parameters, the rule's buffers, the moving average and
        the counters.  What a snapshot has to cover (GraphedTrainStepper's capture warm-up)."""
        out = [self.flat_p] + list(self._rule_state().values())
        if self.ema is not None:
            out.append(self.flat_ema)
        return out + self.counters()

    def _ema_args(self):
        return float(self.ema.decay), int(self.ema.warmup), self.ema_updates.data_ptr()

    @torch.no_grad()
    def swap_ema(self):
        """Exchange the parameters and their moving average in place (uh_swap_f32: exact, no third buffer): the model then
        computes with the averaged weights, and a second call puts everything back bit for bit.  The packed-filter and
        folded BatchNorm caches are keyed on ops.WEIGHT_EPOCH (ops.packed_w3x3_cached, ops.bn_eval_coeffs_cached,
        ops.ConvWeightPack), which is bumped."""
        if self.ema is None:
            raise RuntimeError(f"{type(self).__name__}.swap_ema() without ema_decay")
        LIB.call("uh_swap_f32", self.flat_p.data_ptr(), self.flat_ema.data_ptr(), self.total,
                 torch.cuda.current_stream().cuda_stream)
        ops.WEIGHT_EPOCH += 1

    def _layout(self):
        return [[int(o), int(n), [int(d) for d in p.shape]] for p, (o, n) in zip(self.params, self.slices)]

    def state_dict(self) -> Dict:
        """The state a resumed run needs beside the parameters themselves (they travel in the model's state_dict): clones of
        the rule's buffers (RMSprop: square_avg, momentum_buffer; AdamW: exp_avg, exp_avg_sq and the step count; SGD:
        momentum_buffer), the moving average and its update count (None / 0 without one), the slice layout they are laid out
        by, and the hyper-parameters (the current lr among them).  AdamW and SGD states also say their "kind"; an RMSprop
        state has no such key."""
        g = self.param_groups[0]
        hyper = {k: (g[k] if isinstance(g[k], bool) else float(g[k])) for k in ("lr",) + self.HYPER}
        hyper["gradient_clipping"] = self.gradient_clipping
        hyper["ema_decay"] = float(self.ema.decay) if self.ema is not None else None
        hyper["ema_warmup"] = int(self.ema.warmup) if self.ema is not None else None
        out = {} if self.KIND == "rmsprop" else {"kind": self.KIND}
        out.update((k, v.detach().clone()) for k, v in self._rule_state().items())
        if self.step_count is not None:
            out["step"] = int(self.step_count.item())
        out.update({"ema": self.flat_ema.detach().clone() if self.ema is not None else None,
                    "ema_updates": int(self.ema_updates.item()) if self.ema is not None else 0,
                    "layout": self._layout(), "total": int(self.total), "hyper": hyper})
        return out

    @torch.no_grad()
    def load_state_dict(self, state: Dict):
        """Restore what state_dict() returned.  ValueError when the slice layout differs (another model, another parameter
        order), when the state and this optimizer disagree about keeping a moving average, or when they keep it with another
        decay or warm-up (the average is part of the run: it is not continued under other settings silently), or when the
        state was written by another rule (a state without "kind" is RMSprop's)."""
        name = type(self).__name__
        kind = state.get("kind", "rmsprop")
        if kind != self.KIND:
            raise ValueError(f"{name}.load_state_dict: the state is an optimizer state of kind {kind!r}, this optimizer's is "
                             f"{self.KIND!r}")
        layout = [[int(o), int(n), [int(d) for d in shape]] for o, n, shape in state["layout"]]
        if layout != self._layout() or int(state["total"]) != self.total:
            raise ValueError(f"{name}.load_state_dict: the state's slice layout is not this optimizer's "
                             f"({len(layout)} slices over {int(state['total'])} floats against {len(self.slices)} over {self.total})")
        if (state.get("ema") is not None) != (self.ema is not None):
            raise ValueError(f"{name}.load_state_dict: the state " + ("has" if state.get("ema") is not None else "lacks")
                             + " a moving average and this optimizer " + ("keeps one" if self.ema is not None else "keeps none"))
        hyper = dict(state["hyper"])
        if self.ema is not None:
            saved = EmaConfig(float(hyper["ema_decay"]), int(hyper["ema_warmup"]))
            if saved != self.ema:
                raise ValueError(f"{name}.load_state_dict: the state's moving average was kept with {saved.spec()!r}, "
                                 f"this optimizer keeps one with {self.ema.spec()!r}")
            self.flat_ema.copy_(state["ema"])
            self.ema_updates.fill_(int(state["ema_updates"]))
        for k, buf in self._rule_state().items():
            buf.copy_(state[k])
        if self.step_count is not None:
            self.step_count.fill_(int(state["step"]))
        for k in ("lr",) + self.HYPER:
            self.param_groups[0][k] = hyper[k] if isinstance(hyper[k], bool) else float(hyper[k])
        self.gradient_clipping = float(hyper["gradient_clipping"])
        ops.WEIGHT_EPOCH += 1

    def grad_of(self, p: torch.Tensor) -> torch.Tensor:
        """The (clipped, after step()) gradient of `p` as stored in the flat buffer."""
        o, n = self.slices[self._index[id(p)]]
        return torch.as_strided(self.flat_g, p.shape, p.stride(), o)


class FusedRMSprop(FusedOptimizer):
    """clip_grad_norm_ + torch.optim.RMSprop(momentum > 0, centered=False) over ONE flat buffer (FusedOptimizer): the
    reference's optimizer and the default.  State: `flat_sq` (square_avg) and `flat_buf` (momentum_buffer);
    uh_rmsprop_step / uh_rmsprop_step_ema."""

    KIND = "rmsprop"
    HYPER = ("alpha", "eps", "weight_decay", "momentum")

    def __init__(self, params: Iterable[nn.Parameter], lr: float = 1e-5, alpha: float = 0.99, eps: float = 1e-8,
                 weight_decay: float = 1e-8, momentum: float = 0.999, gradient_clipping: float = 1.0,
                 process_group=None, bucket_bytes: int = 8 << 20, ema_decay: Optional[float] = None, ema_warmup: int = EmaConfig.warmup):
        super().__init__(params, dict(lr=lr, alpha=alpha, eps=eps, weight_decay=weight_decay, momentum=momentum),
                         gradient_clipping, process_group, bucket_bytes, ema_decay, ema_warmup)

    def _alloc_state(self, total, dev):
        self.flat_sq = torch.zeros(total, dtype=torch.float32, device=dev)
        self.flat_buf = torch.zeros(total, dtype=torch.float32, device=dev)

    def _rule_state(self):
        return {"square_avg": self.flat_sq, "momentum_buffer": self.flat_buf}

    def _launch(self, o, n, g, st):
        if self.ema is None:
            LIB.call("uh_rmsprop_step", self.flat_p[o:].data_ptr(), self.flat_g[o:].data_ptr(), self.flat_sq[o:].data_ptr(),
                     self.flat_buf[o:].data_ptr(), n, self.norm.data_ptr(), self.gradient_clipping, float(g["lr"]),
                     float(g["alpha"]), float(g["eps"]), float(g["weight_decay"]), float(g["momentum"]), st)
        else:
            LIB.call("uh_rmsprop_step_ema", self.flat_p[o:].data_ptr(), self.flat_g[o:].data_ptr(),
                     self.flat_sq[o:].data_ptr(), self.flat_buf[o:].data_ptr(), self.flat_ema[o:].data_ptr(), n,
                     self.norm.data_ptr(), self.gradient_clipping, float(g["lr"]), float(g["alpha"]), float(g["eps"]),
                     float(g["weight_decay"]), float(g["momentum"]), *self._ema_args(), st)


class FusedAdamW(FusedOptimizer):
    """clip_grad_norm_ + torch.optim.AdamW(amsgrad=False, maximize=False) over ONE flat buffer (FusedOptimizer).  State:
    `flat_m` (exp_avg), `flat_v` (exp_avg_sq) and `step_count`, a device int32[1] of the steps applied so far: the kernel
    reads it for the bias corrections 1 - beta^t, t = step_count + 1 (uh_adamw_step / uh_adamw_step_ema), and uh_ema_tick
    advances it once per applied step -- on the device, so that a step replayed from a captured graph uses its own t.  A step
    skipped for a non-finite gradient norm does not count.

    The counter is ONE per optimizer, where torch keeps one per parameter: a parameter skipped as stale (no gradient this
    step) keeps exp_avg, exp_avg_sq and its value untouched, as in torch, but when it gets a gradient again its bias
    corrections use the optimizer's t, not the number of updates it has itself received.  The U-Nets use every parameter on
    every step, so for them the two agree."""

    KIND = "adamw"
    HYPER = ("beta1", "beta2", "eps", "weight_decay")

    def __init__(self, params: Iterable[nn.Parameter], lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.01, gradient_clipping: float = 1.0, process_group=None, bucket_bytes: int = 8 << 20,
                 ema_decay: Optional[float] = None, ema_warmup: int = EmaConfig.warmup):
        cfg = OptimConfig("adamw", betas=betas, eps=eps, wd=weight_decay)           # (the range checks)
        super().__init__(params, dict(lr=lr, beta1=cfg.betas[0], beta2=cfg.betas[1], eps=cfg.eps, weight_decay=cfg.wd),
                         gradient_clipping, process_group, bucket_bytes, ema_decay, ema_warmup)

    def _alloc_state(self, total, dev):
        self.flat_m = torch.zeros(total, dtype=torch.float32, device=dev)
        self.flat_v = torch.zeros(total, dtype=torch.float32, device=dev)
        self.step_count = torch.zeros(1, dtype=torch.int32, device=dev)

    def _rule_state(self):
        return {"exp_avg": self.flat_m, "exp_avg_sq": self.flat_v}

    def _launch(self, o, n, g, st):
        args = (self.flat_p[o:].data_ptr(), self.flat_g[o:].data_ptr(), self.flat_m[o:].data_ptr(), self.flat_v[o:].data_ptr())
        hyper = (self.norm.data_ptr(), self.gradient_clipping, float(g["lr"]), float(g["beta1"]), float(g["beta2"]),
                 float(g["eps"]), float(g["weight_decay"]), self.step_count.data_ptr())
        if self.ema is None:
            LIB.call("uh_adamw_step", *args, n, *hyper, st)
        else:
            LIB.call("uh_adamw_step_ema", *args, self.flat_ema[o:].data_ptr(), n, *hyper, *self._ema_args(), st)


class FusedSGD(FusedOptimizer):
    """clip_grad_norm_ + torch.optim.SGD(dampening=0) over ONE flat buffer (FusedOptimizer), Nesterov momentum by default.
    State: `flat_buf` (momentum_buffer), zero-initialised -- with dampening 0 that gives torch's first step, which is why
    dampening is not offered; no step counter (uh_sgd_step / uh_sgd_step_ema).  momentum=0 is plain SGD."""

    KIND = "sgd"
    HYPER = ("momentum", "weight_decay", "nesterov")

    def __init__(self, params: Iterable[nn.Parameter], lr: float = 1e-2, momentum: float = 0.99, nesterov: bool = True,
                 weight_decay: float = 3e-5, gradient_clipping: float = 1.0, process_group=None, bucket_bytes: int = 8 << 20,
                 ema_decay: Optional[float] = None, ema_warmup: int = EmaConfig.warmup):
        cfg = OptimConfig("sgd", momentum=momentum, nesterov=nesterov, wd=weight_decay)          # (the range checks)
        super().__init__(params, dict(lr=lr, momentum=cfg.momentum, weight_decay=cfg.wd, nesterov=cfg.nesterov),
                         gradient_clipping, process_group, bucket_bytes, ema_decay, ema_warmup)

    def _alloc_state(self, total, dev):
        self.flat_buf = torch.zeros(total, dtype=torch.float32, device=dev)

    def _rule_state(self):
        return {"momentum_buffer": self.flat_buf}

    def _launch(self, o, n, g, st):
        args = (self.flat_p[o:].data_ptr(), self.flat_g[o:].data_ptr(), self.flat_buf[o:].data_ptr())
        hyper = (self.norm.data_ptr(), self.gradient_clipping, float(g["lr"]), float(g["weight_decay"]), float(g["momentum"]),
                 int(bool(g["nesterov"])))
        if self.ema is None:
            LIB.call("uh_sgd_step", *args, n, *hyper, st)
        else:
            LIB.call("uh_sgd_step_ema", *args, self.flat_ema[o:].data_ptr(), n, *hyper, *self._ema_args(), st)


def build_optimizer(config: OptimConfig, params, lr: float, **common) -> FusedOptimizer:
    """The optimizer of a config (authoritative for the rule's hyper-parameters; lr and `common` -- gradient_clipping,
    process_group, ema_decay, ema_warmup -- come from the caller)."""
    if config.rule == "adamw":
        return FusedAdamW(params, lr=lr, betas=config.betas, eps=config.eps, weight_decay=config.wd, **common)
    if config.rule == "sgd":
        return FusedSGD(params, lr=lr, momentum=config.momentum, nesterov=config.nesterov, weight_decay=config.wd, **common)
    return FusedRMSprop(params, lr=lr, alpha=config.alpha, eps=config.eps, weight_decay=config.wd, momentum=config.momentum,
                        **common)


def _weak_grad_hook(opt: "FusedOptimizer"):
    ref = weakref.ref(opt)

    def hook(p):
        o = ref()
        if o is not None:
            o._on_grad(p)
    return hook


def _weak_callback(opt: "FusedOptimizer", i: int):
    ref = weakref.ref(opt)

    def cb(event=None):
        o = ref()
        if o is not None:
            o._written(i, event)
    return cb


def _is_dense(p: torch.Tensor) -> bool:
    sizes_strides = sorted(((st, sz) for sz, st in zip(p.shape, p.stride()) if sz > 1))
    expect = 1
    for st, sz in sizes_strides:
        if st != expect:
            return False
        expect *= sz
    return True


# ----------------------------------------------------------------------------------- one step
_ONES = {}
_PINNED = {}


def _one_like(loss: torch.Tensor) -> torch.Tensor:
    key = (loss.device, loss.dtype, tuple(loss.shape))
    t = _ONES.get(key)
    if t is None:
        t = _ONES[key] = torch.ones(loss.shape, dtype=loss.dtype, device=loss.device)
    return t


def _pinned_flag(device, n: int = 1) -> torch.Tensor:
    """Pinned floats the NaN flag (and, data parallel, the pattern probe) are copied into (one buffer per device: it is read
    back before the next step writes it)."""
    t = _PINNED.get(device)
    if t is None:
        t = _PINNED[device] = torch.zeros(4, dtype=torch.float32).pin_memory()
    return t[:n]


def train_step(model: nn.Module, optimizer, images: torch.Tensor, true_masks: torch.Tensor, *, amp: bool = True,
               gradient_clipping: float = 1.0, reduce_sums=None, world: int = 1, check_nan: bool = True,
               boundary_weight: Optional[float] = None, cc_loss: bool = False, surface_weight: float = 0.0,
               surface_classes=None, loss=None, distill=None) -> Dict[str, torch.Tensor]:
    """Statement sequence of train.py:113-159.  `optimizer` is a FusedOptimizer (clipping fused into
    its step) or any torch.optim optimizer (then clip_grad_norm_ is applied as in the reference).
    surface_weight / surface_classes: the surface term of seg_loss (0: off, the step is what it is without the option).
    loss: the focal + Tversky configuration of seg_loss (None: off, likewise).
    distill: a utils.distill.Distiller (None: off, likewise): its frozen teacher's eval forward runs on this step's images --
    as they arrive here, augmented and cropped -- before the student's forward, and seg_loss adds w * kd."""
    assert images.shape[1] == model.n_channels, \
        f"Network has been defined with {model.n_channels} input channels, but loaded images have " \
        f"{images.shape[1]} channels. Please check that the images are loaded correctly."   # train.py:108-111
    teacher_logits = None if distill is None else distill.teacher_logits(images)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
        masks_pred = model(images)
        terms = seg_loss(masks_pred, true_masks, model.n_classes, reduce_sums=reduce_sums, world=world,
                         boundary_weight=boundary_weight, surface_weight=surface_weight, surface_classes=surface_classes,
                         loss=loss, distill=None if distill is None else distill.config, teacher_logits=teacher_logits)
    if cc_loss and model.n_classes == 1:
        # the block train.py:124-132 keeps commented out (BASELINE config 5 turns it on): a Python float, no gradient.
        # sigmoid(x) > 0.5 <=> x > 0, so the 0/1 threshold mask stands in for the probabilities.  The masks stay on the
        # device (uh_cc_loss_device); only the resulting scalar is read back, which waits for the forward like the
        # reference's .cpu() does.
        from .utils.connected_component_loss import connected_component_loss
        cc = connected_component_loss(ops.threshold_mask(masks_pred.detach().squeeze(1)), edge_distance=50, min_area=1000,
                                      penalty_weight=0.1)
        terms["cc"] = torch.tensor(cc, device=masks_pred.device)
        terms["loss"] = terms["loss"] + cc
    loss = terms["loss"]
    nan_flag = terms.pop("nan_flag", None)       # (not one of the reported terms)
    nan_host = nan_event = None
    if check_nan:
        # train.py:149-151 raises before backward().  Reading the flag right here would stall the host until the
        # forward has drained and leave the GPU idle while backward is being enqueued, so the flag travels to pinned
        # memory asynchronously and is read after backward has been ENQUEUED, still before the optimizer step: a NaN
        # loss raises the same error and never reaches the parameters.
        flag = nan_flag
        if flag is None or cc_loss:
            flag = torch.isnan(loss.detach()).reshape(1).float()
        probe = None
        if reduce_sums is not None:
            # data parallel: boundary_loss (and so the loss value) is per rank; every rank must take the SAME decision, or
            # the ranks that continue hang at their next collective while one has raised.  The same all-reduce carries the
            # checksum of the previous step's fresh / stale gradient pattern (FusedOptimizer.pattern_probe).
            probe = optimizer.pattern_probe() if isinstance(optimizer, FusedOptimizer) else None
            if probe is not None:
                flag = torch.cat([flag.reshape(1), probe])
            flag = reduce_sums(flag)
        nan_host = _pinned_flag(loss.device, flag.numel())
        nan_host.copy_(flag, non_blocking=True)
        nan_event = torch.cuda.Event()
        nan_event.record()
    optimizer.zero_grad(set_to_none=True)
    # (the seed gradient is a cached constant: loss.backward() alone launches a fill kernel for it every step)
    loss.backward(gradient=_one_like(loss))
    ops.flush_slabs()            # the backward-weights reductions that waited for one batched launch (ops.SlabBatch)
    if nan_event is not None:
        nan_event.synchronize()
        host = nan_host.tolist()
        if len(host) == 3:
            optimizer.check_probe(host[1], host[2], optimizer.sync.world)     # (`world` may be a ragged shard's gb / lb: the group's size counts)
        if host[0] > 0:
            if isinstance(optimizer, FusedOptimizer):
                optimizer.abort_step()
            raise RuntimeError("Fatal: NaN loss detected!")                                   # train.py:149-151
    if isinstance(optimizer, FusedOptimizer):
        terms["grad_norm"] = optimizer.step()
    else:
        terms["grad_norm"] = torch.nn.utils.clip_grad_norm_(model.parameters(), gradient_clipping)
        optimizer.step()
    terms["logits"] = masks_pred.detach()
    return terms


class TrainStepper:
    """Model + fused optimizer (FusedRMSprop unless `optimizer` names another rule) (+ RCCL gradient sync when
    torch.distributed is initialised)."""

    def __init__(self, model: nn.Module, lr: float = 1e-5, weight_decay: float = 1e-8, momentum: float = 0.999,
                 gradient_clipping: float = 1.0, amp: bool = True, process_group=None, check_nan: bool = True,
                 wgrad_stream: Optional[bool] = None, cc_loss: bool = False, sync_bn: bool = False, fp32_mode: str = "exact",
                 surface_weight: float = 0.0, surface_classes=None, ema: Union[None, str, EmaConfig] = None, loss=None,
                 distill=None, optimizer: Union[None, str, OptimConfig] = None):
        self.model = model
        # optimizer: an OptimConfig or a spec string ("adamw", "sgd,momentum=0.9", ...): the update rule of the fused pass and
        # its hyper-parameters, for which the config is authoritative (`weight_decay` and `momentum` above are RMSprop's and are
        # not read then); `lr` and `gradient_clipping` stay this constructor's.  None (default): FusedRMSprop as ever.
        self.optim_config = OptimConfig.of(optimizer)
        # distill: a utils.distill.Distiller, DistillConfig or spec string: every step adds w * kd against the frozen teacher's
        # logits for the step's images.  The teacher is an object beside the model: it is in no optimizer, flat buffer, moving
        # average, state_dict or checkpoint, and no collective touches it (every rank holds its own copy).  A config or spec
        # builds the Distiller here, on the model's device, with this stepper's amp.  None (default): nothing is imported,
        # allocated or launched for it.
        self.distill = None
        if distill is not None:
            from .utils.distill import Distiller
            if not isinstance(distill, Distiller):
                distill = Distiller(distill, model.n_channels, model.n_classes, next(model.parameters()).device, amp)
            elif distill.teacher.n_classes != model.n_classes or distill.teacher.n_channels != model.n_channels:
                raise ValueError(f"TrainStepper: the teacher has {distill.teacher.n_channels} input channels and a head of "
                                 f"{distill.teacher.n_classes} outputs, the student {model.n_channels} and {model.n_classes}")
            self.distill = distill
        # loss: a utils.focal_loss.LossConfig or its spec string: the focal + Tversky node replaces the CE + Dice pair of every
        # step, checked against the model's head here.  None (default): the step is what it is without the option.
        self.loss = None
        if loss is not None:
            from .utils.focal_loss import LossConfig
            self.loss = LossConfig.of(loss)
            self.loss.for_head(model.n_classes)
        # ema: an EmaConfig or a spec string ("0.999,warmup=10"): the optimizer keeps a moving average of the parameters
        # (FusedOptimizer), averaged() computes with it.  None (default): nothing is allocated or launched for it.
        self.ema = EmaConfig.of(ema)
        self._averaged = False
        # the surface term of seg_loss; a plain attribute: the epoch loop may change the weight between steps (0 = off)
        self.surface_weight = float(surface_weight)
        self.surface_classes = surface_classes
        # wgrad_stream: backward-weights kernels (and their slab reductions) on a stream of their own, beside the BatchNorm /
        # pool / upsample backward kernels of the layers that follow.  True / False force it; None (default) decides per step
        # (`_side_for`): ON for bf16 steps of at least 2^20 pixels per process.  Round 2 measured one stream 2-3 % faster and
        # turned it off; with round 4's kernels (bf16 slabs, rotated backward-weights loop) it is the other way round on the
        # GPU-bound bf16 configurations -- batch 8: 872.2 -> 884.9 images/s (+1.5 %), batch 4 +2.2 %, batch 32 +1 %, config 4
        # +1.1 %, transposed-conv variant +0.8 %, three interleaved rounds each -- while exact fp32 loses 3 % and batch 2
        # (host-bound: two more stream switches per layer) 7-20 % (DESIGN.md "Measured (round 4)").  UH_SIDE_STREAM=0 / 1
        # overrides the automatic choice.
        # (kept on the instance and installed in ops.STEP for the duration of step() only: another live stepper keeps its own
        # choice, and nothing of this one is left behind between steps or after close())
        self._side_auto = wgrad_stream is None
        env = os.environ.get("UH_SIDE_STREAM")
        if self._side_auto and env in ("0", "1"):
            wgrad_stream, self._side_auto = (env == "1"), False
        want = wgrad_stream is None or bool(wgrad_stream)
        # (a high-priority stream: 897.6 vs 894.9 images/s on the default priority, 893.2 on a low one, 884.8 on one stream --
        # scratch/r4_prio_probe.py, three interleaved rounds)
        self.wgrad_stream = torch.cuda.Stream(priority=-1) if (want and torch.cuda.is_available()) else None
        self.amp = amp
        self.check_nan = check_nan
        if fp32_mode not in ("exact", "bf16x3"):
            raise ValueError("fp32_mode must be 'exact' or 'bf16x3'")
        self.fp32_mode = fp32_mode          # how fp32 activations are convolved (ops.StepState.fp32_mode); irrelevant under amp
        self.cc_loss = cc_loss
        self.group = process_group
        self.world = dpmod.world_size(process_group)
        self.reduce_sums = dpmod.make_sum_reducer(process_group)
        # sync_bn: BatchNorm statistics (forward) and their backward sums over the GLOBAL batch -> the data-parallel step
        # reproduces the single-process step on the concatenated batch (SURVEY.md 8e option 2); default = per-rank
        # statistics like stock DDP.  One all_gather (2C+1 floats) + one all_reduce (2C floats) per BatchNorm layer.
        # Its collectives run on the GRADIENT group by default.  UH_SYNCBN_OWN_GROUP=1 gives them a process group of their own
        # (on the gradient group they queue, inside RCCL's one stream per communicator, behind bucket all-reduces; with the
        # opt-in side stream for backward-weights those wait for side-stream events, and the critical-path BatchNorm backward
        # would stall behind work it does not depend on).  Opt-in because two communicators issuing collectives concurrently
        # from one process is the pattern RCCL deadlocks on when the ranks enqueue them in different orders, and no N > 1
        # RCCL box has run it yet; because dist.new_group is a collective over the WHOLE default group (a stepper built on a
        # sub-group must be constructed by every rank of the job); and because the extra communicator has to be destroyed
        # (close()).  UH_DP_FORCE_SYNC=1 turns SyncBN on in a ONE-rank group too, so that both communicators are exercised
        # against the real backend on a one-GPU box (tests/test_gpu_dp.py).
        self.sync_bn = None
        self.bn_group = None
        if sync_bn and dpmod.sync_enabled(process_group):
            import torch.distributed as dist
            group = process_group
            if os.environ.get("UH_SYNCBN_OWN_GROUP") == "1":
                ranks = dist.get_process_group_ranks(process_group) if process_group is not None else list(range(dist.get_world_size()))
                self.bn_group = group = dist.new_group(ranks=ranks)
            self.sync_bn = (group, self.world)
        common = dict(gradient_clipping=gradient_clipping, process_group=process_group,
                      **({} if self.ema is None else {"ema_decay": self.ema.decay, "ema_warmup": self.ema.warmup}))
        if self.optim_config is None:
            self.optimizer = FusedRMSprop(model.parameters(), lr=lr, weight_decay=weight_decay, momentum=momentum, **common)
        else:
            self.optimizer = build_optimizer(self.optim_config, model.parameters(), lr, **common)
        self._pack = None
        # the closing reductions of backward-weights wait for one batched launch behind the backward pass; data parallel: for
        # one launch per gradient bucket, so that the bucket's all-reduce still starts under the rest of the backward pass
        sync = self.optimizer.sync
        self._slabs = ops.SlabBatch(flush_bytes=None if sync is None else 8 << 20)

    def close(self):
        """Release what the stepper owns outside torch's garbage collection: the optimizer's hooks and, when SyncBN runs on
        a process group of its own (UH_SYNCBN_OWN_GROUP=1), that communicator."""
        opt = getattr(self, "optimizer", None)
        if opt is not None:
            opt.close()
        grp, self.bn_group = getattr(self, "bn_group", None), None
        if grp is not None:
            import torch.distributed as dist
            self.sync_bn = None
            if dist.is_initialized():
                dist.destroy_process_group(grp)

    def __del__(self):
        try:
            if getattr(self, "bn_group", None) is not None:
                self.close()
        except Exception:
            pass

    @contextlib.contextmanager
    def averaged(self):
        """`with stepper.averaged(): evaluate(model, ...)` -- inside the block the model's parameters ARE the moving average
        (swapped in place, FusedOptimizer.swap_ema), on leaving it the live ones are back bit for bit, also after an exception.
        BatchNorm running statistics are shared with the live model and not averaged: they are already a moving average
        (momentum 0.1) of the statistics of recent batches.  Nesting the block or calling step() inside it raises
        RuntimeError: an update applied to the swapped buffers would train the average."""
        if self.ema is None:
            raise RuntimeError("TrainStepper.averaged() needs ema=...")
        if self._averaged:
            raise RuntimeError("TrainStepper.averaged() is already active (it does not nest)")
        self.optimizer.swap_ema()
        self._averaged = True
        try:
            yield self.model
        finally:
            self.optimizer.swap_ema()
            self._averaged = False

    def _refuse_averaged(self):
        if self._averaged:
            raise RuntimeError("TrainStepper.step() inside averaged(): the model holds the averaged weights")

    def ema_state_dict(self) -> Dict[str, torch.Tensor]:
        """The model's state_dict on the CPU in the checkpoint wire format (checkpoint.py), with the averaged parameters in
        place of the live ones and the live buffers (BatchNorm running statistics: see averaged())."""
        if self.ema is None:
            raise RuntimeError("TrainStepper.ema_state_dict() needs ema=...")
        opt = self.optimizer
        src = opt.flat_p if self._averaged else opt.flat_ema          # (inside averaged() the model holds the average)
        base, size = opt.flat_p.data_ptr(), opt.flat_p.numel() * 4
        out = {}
        for k, v in self.model.state_dict().items():
            off = v.data_ptr() - base
            if 0 <= off < size and v.dtype == torch.float32:
                v = torch.as_strided(src, v.shape, v.stride(), off // 4)
            out[k] = v.detach().to("cpu", copy=True)
        return out

    SIDE_MIN_PIXELS = 1 << 20

    def _side_for(self, images):
        """The stream backward-weights runs on in the step over `images` (None: the launch stream)."""
        if self.wgrad_stream is None or not self._side_auto:
            return self.wgrad_stream
        if self.sync_bn is not None and self.bn_group is None:
            # SyncBN's collectives share the gradient communicator (one RCCL stream): a BatchNorm-backward all_reduce on the critical
            # path would queue behind bucket all-reduces that wait for side-stream events.  Unmeasured over RCCL with more than
            # one rank (one-GPU boxes), so the automatic choice stays on the safe side: one stream.  UH_SYNCBN_OWN_GROUP=1 (a
            # communicator of its own) or an explicit wgrad_stream=True keep the side stream.
            return None
        big = images.is_cuda and images.shape[0] * images.shape[-2] * images.shape[-1] >= self.SIDE_MIN_PIXELS
        return self.wgrad_stream if (self.amp and big) else None

    @contextlib.contextmanager
    def _step_state(self, images, sync_bn, global_batch: Optional[int] = None):
        """Everything the autograd nodes read besides their arguments, installed (ops.step_state) for the step over `images`
        and gone again behind it, also when the step raises.  `sync_bn`: the (group, world) pair of the step or None.
        Yields the `world` the loss is normalised by."""
        self.model.train()
        side = self._side_for(images)
        world, batch = self.world, None
        if sync_bn is not None:
            lb = int(images.shape[0])
            gb = int(global_batch) if global_batch is not None else dpmod.global_batch(lb, self.group, images.device)
            batch = (gb, lb)
            world = gb / lb               # ragged shards: the loss is normalised by the GLOBAL pixel count n * gb / lb
        # one launch packs every 3x3 filter (bf16/fp32 KRSC + backward-data layout) for this step's forward/backward
        dt = torch.bfloat16 if self.amp else getattr(self.model, "compute_dtype", torch.float32)
        if self._pack is None or self._pack.dtype != dt:
            ws = [m.weight for m in self.model.modules() if isinstance(m, nn.Conv2d) and m.kernel_size == (3, 3)]
            self._pack = ops.ConvWeightPack(ws, dt) if ws and all(w.is_cuda for w in ws) else None
        if self._pack is not None:
            self._pack.refresh()
        self._slabs.reset()
        with ops.step_state(wgrad_stream=side, sync_bn=sync_bn, sync_bn_batch=batch, weight_pack=self._pack,
                            slab_batch=self._slabs if side is None else None, fp32_mode=self.fp32_mode):
            yield world

    def step(self, images, true_masks, global_batch: Optional[int] = None):
        """One optimizer step (train.py:113-159).  `global_batch` (data parallel with sync_bn): the sum of the ranks' batch
        sizes when the caller knows it (equal shards: world * B) -- otherwise it is all-reduced here, which costs a blocking
        host read per step."""
        self._refuse_averaged()
        with self._step_state(images, self.sync_bn, global_batch) as world:
            return train_step(self.model, self.optimizer, images, true_masks, amp=self.amp,
                              reduce_sums=self.reduce_sums, world=world, check_nan=self.check_nan, cc_loss=self.cc_loss,
                              surface_weight=self.surface_weight, surface_classes=self.surface_classes,
                              loss=self.loss, distill=self.distill)


class GraphedTrainStepper(TrainStepper):
    """TrainStepper whose whole step (forward, loss, backward, clip + update) is captured once into a HIP graph and
    replayed per batch: for launch-bound models (UNet_S / UNet_T: ~500 small kernels per step) the host no longer paces
    the GPU.  Fixed batch shape; re-captured when the learning rate changes (it is a kernel argument); single process
    only.  A NaN loss is detected after the replay (the fused optimizer kernel has skipped the update: non-finite norm).
    With `ema` the captured graph holds the averaging launches and the update counter's tick; the decay of the warm-up is
    computed on the device from that counter, so every replay uses its own.  Likewise with optimizer="adamw": the step number
    of the bias corrections is FusedAdamW.step_count on the device, ticked inside the graph."""

    def __init__(self, model: nn.Module, *args, warmup: int = 2, **kw):
        kw.setdefault("wgrad_stream", False)         # one stream unless asked for: the graph is for launch-bound small models
        self._refuse_uncaptured(distill=kw.get("distill"))          # (before a teacher is built for it)
        super().__init__(model, *args, **kw)
        if self.world != 1:
            raise RuntimeError("GraphedTrainStepper is single-process; use TrainStepper with torch.distributed")
        if self.cc_loss:
            raise RuntimeError("connected_component_loss returns a Python float (a device read-back every step): not capturable")
        self._refuse_uncaptured(self.surface_weight, self.loss, self.distill)
        self._warmup = max(1, warmup)
        self._graph = None
        self._key = None

    @staticmethod
    def _refuse_uncaptured(surface_weight=0.0, loss=None, distill=None):
        for on, what, off in ((bool(surface_weight), "the surface loss", "surface_weight must be 0"),
                              (loss is not None, "the focal / Tversky loss", "loss must be None"),
                              (distill is not None, "distillation", "distill must be None")):
            if on:
                raise RuntimeError(f"GraphedTrainStepper does not capture {what} ({off}): use TrainStepper")

    def _eager_step(self, images, masks):
        with self._step_state(images, None):         # (single process: per-rank BatchNorm statistics, world = self.world)
            return train_step(self.model, self.optimizer, images, masks, amp=self.amp, reduce_sums=self.reduce_sums,
                              world=self.world, check_nan=False)

    def _capture(self, images, masks):
        opt = self.optimizer
        # the warm-up steps the capture protocol needs must not count as training: snapshot, warm up, restore
        snap_model = {k: v.clone() for k, v in self.model.state_dict().items()}
        snap_opt = [t.clone() for t in opt.state_tensors()]          # parameters, the rule's state, the average, the counters
        self._im = images.detach().clone(memory_format=torch.preserve_format)
        self._mk = masks.detach().clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(self._warmup):
                self._eager_step(self._im, self._mk)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        with torch.no_grad():
            for t, snap in zip(opt.state_tensors(), snap_opt):
                t.copy_(snap)
            for k, v in self.model.state_dict().items():
                if v.data_ptr() < opt.flat_p.data_ptr() or v.data_ptr() >= opt.flat_p.data_ptr() + opt.flat_p.numel() * 4:
                    v.copy_(snap_model[k])                    # buffers (running statistics, num_batches_tracked)
        self._graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self._graph):
            terms = self._eager_step(self._im, self._mk)
            self._nan = torch.isnan(terms["loss"].detach()).reshape(1)
        self._terms = terms
        self._key = (tuple(images.shape), tuple(masks.shape), float(opt.param_groups[0]["lr"]))

    def step(self, images, true_masks):
        self._refuse_uncaptured(self.surface_weight, self.loss, self.distill)
        self._refuse_averaged()
        key = (tuple(images.shape), tuple(true_masks.shape), float(self.optimizer.param_groups[0]["lr"]))
        if self._graph is None or key != self._key:
            self._capture(images, true_masks)
        self._im.copy_(images)
        self._mk.copy_(true_masks)
        self._graph.replay()
        ops.WEIGHT_EPOCH += 1
        if self.check_nan and bool(self._nan.item()):
            raise RuntimeError("Fatal: NaN loss detected!")                                   # train.py:149-151
        return self._terms


# ----------------------------------------------------------------------------------- epoch loop
def cosine_warm_restarts_lr(base_lr: float, epoch_arg: float, T_0: int = 4, T_mult: int = 2, eta_min: float = 1e-7):
    """CosineAnnealingWarmRestarts.step(epoch) closed form; train.py:187 passes the Dice score as
    `epoch` -- reproduced, not fixed."""
    e = float(epoch_arg)
    if e >= T_0:
        n = int(math.log(e / T_0 * (T_mult - 1) + 1, T_mult)) if T_mult > 1 else int(e // T_0)
        T_cur = e - T_0 * (T_mult ** n - 1) / (T_mult - 1) if T_mult > 1 else e % T_0
        T_i = T_0 * T_mult ** n
    else:
        T_cur, T_i = e, T_0
    return eta_min + (base_lr - eta_min) * (1 + math.cos(math.pi * T_cur / T_i)) / 2


def train_model(model, device, train_batches, val_batches=None, epochs: int = 5, learning_rate: float = 1e-5,
                amp: bool = True, weight_decay: float = 1e-8, momentum: float = 0.999,
                gradient_clipping: float = 1.0, log=None):
    """Epoch loop of train.py:29-220 over in-memory iterables of {'image','mask'} batches (the
    reference's directory dataset / checkpoint cadence / tqdm are outside the hot-path scope)."""
    from .evaluate import evaluate
    stepper = TrainStepper(model, lr=learning_rate, weight_decay=weight_decay, momentum=momentum,
                           gradient_clipping=gradient_clipping, amp=amp)
    history = []
    for epoch in range(1, epochs + 1):
        epoch_loss = 0.0
        for batch in train_batches:
            images = batch["image"].to(device=device, dtype=torch.float32, memory_format=torch.channels_last)
            true_masks = batch["mask"].to(device=device, dtype=torch.long)
            terms = stepper.step(images, true_masks)
            epoch_loss += terms["loss"].item()                                                # train.py:163
        rec = {"epoch": epoch, "loss": epoch_loss}
        if val_batches is not None:
            val_score, _, min_score = evaluate(model, val_batches, device, amp)          # train.py:186 (postprocess=True)
            lr = cosine_warm_restarts_lr(learning_rate, float(val_score))                     # train.py:187
            stepper.optimizer.param_groups[0]["lr"] = lr
            rec.update(val_dice=float(val_score), min_dice=float(min_score), lr=lr)
        history.append(rec)
        if log:
            log(rec)
    return history


# ----------------------------------------------------------------------------------- command line
def get_args(argv=None):
    """The reference's train.py flags (train_cli.py)."""
    from .train_cli import get_args as _get_args
    return _get_args(argv)


def main(argv=None) -> int:
    """`python -m unet_amd.train ...`: the reference's train.py command line (train_cli.py)."""
    from .train_cli import main as _main
    return _main(argv)


if __name__ == "__main__":
    import sys
    sys.exit(main())
