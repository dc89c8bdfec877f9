"""Torch-side plumbing over the C ABI (include/unet_hip.h): tensor descriptors -> raw pointers,
and the torch.autograd.Function nodes that put the HIP kernels behind the reference's nn.Module
surface.  Activations travel between nodes as pixel-dense NHWC tensors [B,H,W,C] whose pixel
stride may exceed C (channel slices of a wider buffer); the user-facing modules expose them as
logical NCHW views.  Everything here requires GPU tensors: there is no CPU fallback."""
from __future__ import annotations

import contextlib
import ctypes
import os
from typing import NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch
from torch.autograd import Function

from ._lib import LIB, UH_BF16, UH_F32, UH_F32X3, UH_WFRAG, UH_WFRAG_D

BN_EPS_DEFAULT = 1e-5

# optional per-launch timing (bench.py): (kernel family, algorithmic FLOPs, start event, end event, tag) with
# tag = (direction, B, H, W, input channels, output channels) on the 3x3 conv launches, None elsewhere
PROFILE_ON = False
PROFILE = []


def _variant(Cin_split, Cout, esize):
    ck = 64 // esize
    ok = all(c % ck == 0 for c in Cin_split if c) and Cout % 64 == 0
    if ok:
        return "mfma"
    return "stem" if sum(Cin_split) <= 4 else "generic"


class _Timed:
    def __init__(self, name, flops, tag=None):
        self.name, self.flops, self.tag = name, flops, tag

    def __enter__(self):
        if PROFILE_ON:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e1 = torch.cuda.Event(enable_timing=True)
            self.e0.record()
        return self

    def __exit__(self, *a):
        if PROFILE_ON:
            self.e1.record()
            PROFILE.append((self.name, self.flops, self.e0, self.e1, self.tag))


# ----------------------------------------------------------------------------- helpers
def _require_gpu(t: torch.Tensor, what: str = "tensor"):
    if not t.is_cuda:
        raise RuntimeError(f"{what} is on {t.device}: the HIP path needs GPU tensors (no CPU fallback exists)")


def _dt(t: torch.Tensor) -> int:
    if t.dtype == torch.bfloat16:
        return UH_BF16
    if t.dtype == torch.float32:
        return UH_F32
    raise RuntimeError(f"unsupported activation dtype {t.dtype} (float32 / bfloat16 only)")


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def compute_dtype(default: torch.dtype = torch.float32) -> torch.dtype:
    """bf16 inside torch.autocast (train.py:116 wraps the forward in autocast), else `default`."""
    if torch.is_autocast_enabled():
        return torch.bfloat16
    return default


def pixel_ld(t: torch.Tensor) -> int:
    """Pixel stride (elements) of an NHWC tensor [B,H,W,C]."""
    B, H, W, C = t.shape
    if W > 1:
        return t.stride(2)
    if H > 1:
        return t.stride(1)
    if B > 1:
        return t.stride(0)
    return max(C, 1)


def pixel_ld_or0(t: Optional[torch.Tensor]) -> int:
    return 0 if t is None else pixel_ld(t)          # (an absent second source)


def is_pixel_dense(t: torch.Tensor) -> bool:
    B, H, W, C = t.shape
    if C > 1 and t.stride(3) != 1:
        return False
    ld = pixel_ld(t)
    if ld < C:
        return False
    if W > 1 and t.stride(2) != ld:
        return False
    if H > 1 and t.stride(1) != W * ld:
        return False
    if B > 1 and t.stride(0) != H * W * ld:
        return False
    return True


def dense_nhwc(t: torch.Tensor) -> torch.Tensor:
    """Return `t` ([B,H,W,C]) if it can be walked with one pixel stride, else a packed copy."""
    return t if is_pixel_dense(t) else t.contiguous()


def grad_like(dz: torch.Tensor, ref: torch.Tensor) -> torch.Tensor:
    """An incoming NHWC gradient in `ref`'s dtype, walkable with one pixel stride."""
    return dense_nhwc(dz if dz.dtype == ref.dtype else dz.to(ref.dtype))


def to_nhwc(x: torch.Tensor, dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """Logical NCHW tensor (any memory format) -> pixel-dense NHWC view/copy in `dtype`."""
    _require_gpu(x, "input")
    v = x.permute(0, 2, 3, 1)
    if dtype is not None and v.dtype != dtype:
        v = v.to(dtype)
    return dense_nhwc(v)


def to_nchw(x: torch.Tensor) -> torch.Tensor:
    return x.permute(0, 3, 1, 2)


def _empty_like_param(p: torch.Tensor) -> torch.Tensor:
    return torch.empty_strided(p.shape, p.stride(), dtype=torch.float32, device=p.device)


class StepState(NamedTuple):
    """What one training step tells the autograd nodes besides their arguments.  TrainStepper installs a record for the duration
    of a step (step_state); between steps, and for every call outside a stepper, the defaults hold.
    `wgrad_stream`: a second HIP stream for backward-weights -- it only feeds the optimizer, so it can run beside the
    backward-data conv and the HBM-bound BatchNorm-backward kernels of the layers that follow.
    `sync_bn`: (process group, world size) when BatchNorm statistics are to be those of the GLOBAL batch of a data-parallel job
    (TrainStepper(sync_bn=True)); None = per-rank statistics (what stock DDP does).  `sync_bn_batch`: (global batch, local
    batch) of the step under sync_bn; None = equal shards.  `weight_pack`: the ConvWeightPack of the model being trained
    (ConvBnReluFn packs per layer on a miss).  `slab_batch`: the step's SlabBatch; None = every backward-weights call reduces
    its own slabs at once.  `fp32_mode`: how fp32 activations are convolved: "exact" = fp32 MFMA (157 TFLOP/s peak, the parity
    path); "bf16x3" = products on the bf16 matrix pipe with hi/lo splits of both operands (forward / backward-data 3x3 convs
    of MFMA-aligned layers; ~1e-5 relative, backward-weights stays exact).  TrainStepper(fp32_mode=...) / bench.py --bf16x3."""
    wgrad_stream: Optional[torch.cuda.Stream] = None
    sync_bn: Optional[tuple] = None
    sync_bn_batch: Optional[Tuple[int, int]] = None
    weight_pack: Optional[ConvWeightPack] = None
    slab_batch: Optional[SlabBatch] = None
    fp32_mode: str = "exact"


STEP = StepState()


@contextlib.contextmanager
def step_state(**fields):
    """Install STEP._replace(**fields) for the block; the record that was there on entry is back on leaving it, also after an
    exception.  Each reader takes its field when its call is enqueued: a graph captured inside the block keeps what was read."""
    global STEP
    if fields.get("fp32_mode", "exact") not in ("exact", "bf16x3"):
        raise ValueError("fp32_mode must be 'exact' or 'bf16x3'")
    unknown = set(fields) - set(StepState._fields)
    if unknown:
        raise TypeError(f"step_state: no such field: {', '.join(sorted(unknown))}")
    prev, STEP = STEP, STEP._replace(**fields)
    try:
        yield
    finally:
        STEP = prev


# FusedRMSprop registers, per parameter storage, the view of its flat gradient buffer that the backward kernels
# should write into directly (no gather copy afterwards).  Keyed by data_ptr of the parameter.
GRAD_DST = {}


def _grad_buffer(p: torch.Tensor, wanted: bool = True):
    """-> (buffer to write the gradient of `p` into, completion callback or None).  With a callback the gradient is
    final in the optimizer's flat buffer: the autograd node returns None for it (no AccumulateGrad clone).
    `wanted=False` (autograd does not need this gradient: a frozen parameter): scratch memory, no callback -- the
    optimizer must see the parameter as one that received no gradient (torch.optim skips those)."""
    ent = GRAD_DST.get(p.data_ptr()) if wanted else None
    if ent is not None and ent[0].shape == p.shape and ent[0].stride() == p.stride():
        return ent
    return _empty_like_param(p), None


def _is_krsc_dense(w: torch.Tensor) -> bool:
    O, I, kh, kw = w.shape
    return w.stride() == (kh * kw * I, 1, kw * I, I)


# ----------------------------------------------------------------------------- raw op wrappers
def conv_dt(x: torch.Tensor, C0: int, C1: int, Cout: int, need_dx: bool) -> int:
    """dtype code for the 3x3 conv calls of one layer (pack + forward + backward-data use the SAME code)."""
    if x.dtype == torch.float32 and STEP.fp32_mode == "bf16x3":
        Cin = C0 + C1
        if Cin > 4 and C0 % 16 == 0 and C1 % 16 == 0 and Cout % 64 == 0 and (not need_dx or Cin % 64 == 0):
            return UH_F32X3
    return _dt(x)


# Use fragment-major filter packs (UH_WFRAG) wherever the LDS-DMA MFMA kernel runs (False: KRSC everywhere, for A/B runs).
WFRAG = True


def conv_flags(cdt: int, frag: bool) -> int:
    """dtype code of a conv call + the flag that says its filter pack is fragment-major."""
    return cdt | (UH_WFRAG if frag else 0)


# Plan length of the eval forward (0 = off).  Under `with plan_images(1):` the eval-mode Conv->BN->ReLU and the transposed
# convolution take, for a batch of B images, the kernel form ONE image of that size gets (uh_conv3x3_fwd_affine_relu_plan,
# uh_convt2x2_mfma_ok_plan), so every image comes out bit for bit as it does alone, whatever B.  The choice is made on the
# host when the call is enqueued: a graph captured under it keeps it.  Training-mode layers do not read it.
PLAN_IMAGES = 0


@contextlib.contextmanager
def plan_images(n: int = 1):
    """Pin the kernel choice of the eval forward to that of a launch of `n` images (0: the launch's own choice)."""
    global PLAN_IMAGES
    n = int(n)
    if n < 0:
        raise ValueError("plan_images: the plan length must be >= 0")
    prev, PLAN_IMAGES = PLAN_IMAGES, n
    try:
        yield
    finally:
        PLAN_IMAGES = prev


def wfrag_ok(B: int, H: int, W: int, C0: int, C1: int, Cout: int, ld0: int, ld1: int, ldy: int, dt: int,
             plan: int = 0) -> bool:
    """May the filter of this conv call be packed fragment-major?  (dt: UH_F32 / UH_BF16; bf16x3 packs are KRSC.)
    `plan`: the call runs under the pinned plan of that length."""
    if not WFRAG or dt not in (UH_F32, UH_BF16):
        return False
    if plan:
        return bool(LIB.query("uh_conv3x3_wfrag_ok_plan", B, plan, H, W, C0, C1, Cout, ld0, ld1, ldy, dt))
    return bool(LIB.query("uh_conv3x3_wfrag_ok", B, H, W, C0, C1, Cout, ld0, ld1, ldy, dt))


def pack_w3x3(weight: torch.Tensor, dtype: torch.dtype, need_dgrad: bool, dt_code: Optional[int] = None,
              frag_f: bool = False, frag_d: bool = False):
    """-> (forward pack, backward-data pack or None); frag_f / frag_d: fragment-major instead of KRSC (the conv call that
    consumes the pack must then pass wfrag=True)."""
    O, I = weight.shape[0], weight.shape[1]
    w32 = weight if weight.dtype == torch.float32 else weight.float()
    wf = torch.empty(O * 9 * I, dtype=dtype, device=weight.device)
    wd = torch.empty(O * 9 * I, dtype=dtype, device=weight.device) if need_dgrad else None
    sO, sI, sH, sW = w32.stride()
    if dt_code is None:
        dt_code = UH_BF16 if dtype == torch.bfloat16 else UH_F32
    flags = (UH_WFRAG if frag_f else 0) | (UH_WFRAG_D if (frag_d and need_dgrad) else 0)
    LIB.call("uh_pack_w3x3", w32.data_ptr(), sO, sI, sH, sW, O, I, wf.data_ptr(), _p(wd), dt_code | flags, _stream())
    return wf, wd


# Bumped by every optimizer step that writes parameters through raw pointers (FusedRMSprop): such writes do not touch
# torch's version counters, and the inference path caches packed filters per parameter.
WEIGHT_EPOCH = 0


def packed_w3x3_cached(weight: torch.Tensor, dtype: torch.dtype, frag: bool = False) -> torch.Tensor:
    """Filter pack (KRSC, or fragment-major with frag=True) for the inference forward, cached on the parameter until it
    changes."""
    try:
        version = weight._version
    except RuntimeError:                      # a temporary created under torch.inference_mode (zero-padded small-width filter)
        return pack_w3x3(weight, dtype, False, frag_f=frag)[0]
    key = (weight.data_ptr(), version, WEIGHT_EPOCH, dtype, tuple(weight.stride()), frag)
    hit = getattr(weight, "_uh_packed", None)
    if hit is not None and hit[0] == key:
        return hit[1]
    wf, _ = pack_w3x3(weight, dtype, False, frag_f=frag)
    try:
        weight._uh_packed = (key, wf)
    except AttributeError:
        pass
    return wf


# Bumped whenever a training-mode forward rewrites BatchNorm running statistics through raw pointers (no torch version
# bump): the inference path caches the eval-mode scale / shift per BatchNorm until then.
BN_STATS_EPOCH = 0


def bn_eval_coeffs_cached(gamma, beta, running_mean, running_var, eps: float, C: int, Cp: int):
    """-> (scale, shift) fp32 views of Cp entries each, the first C real: eval-mode BatchNorm (evaluate.py:30, predict.py:17)
    folded to one multiply-add, cached on the gamma parameter until a parameter or a running statistic changes."""
    try:
        key = (gamma.data_ptr(), beta.data_ptr(), running_mean.data_ptr(), running_var.data_ptr(), gamma._version,
               beta._version, running_mean._version, running_var._version, WEIGHT_EPOCH, BN_STATS_EPOCH, float(eps), C, Cp)
    except RuntimeError:                      # inference tensors carry no version counter
        key = None
    hit = getattr(gamma, "_uh_bn_eval", None) if key is not None else None
    if hit is not None and hit[0] == key:
        return hit[1][:Cp], hit[1][Cp:]
    g32 = gamma if gamma.dtype == torch.float32 else gamma.float()
    b32 = beta if beta.dtype == torch.float32 else beta.float()
    coef = torch.empty(2 * Cp, dtype=torch.float32, device=gamma.device)
    LIB.call("uh_bn_eval_coeffs", g32.data_ptr(), b32.data_ptr(), running_mean.data_ptr(), running_var.data_ptr(), float(eps),
             C, coef.data_ptr(), coef[Cp:].data_ptr(), _stream())
    if key is not None:
        try:
            gamma._uh_bn_eval = (key, coef)
        except AttributeError:
            pass
    return coef[:Cp], coef[Cp:]


class ConvWeightPack:
    """Packed (KRSC forward + flipped/transposed backward-data) copies of ALL 3x3 filters of a model, refreshed by one
    kernel launch per train step (TrainStepper) instead of one launch per layer inside the forward."""

    def __init__(self, weights, dtype: torch.dtype):
        self.weights = [w for w in weights if w.dim() == 4 and w.shape[2:] == (3, 3) and w.dtype == torch.float32 and w.is_cuda]
        self.dtype = dtype
        self.epoch = -1
        self._build()

    def _build(self):
        dev = self.weights[0].device
        rows, off, toff = [], 0, 0
        self.offsets = []
        ck = 32 if self.dtype == torch.bfloat16 else 16          # channels per 64-byte K chunk
        self.frags = []
        for w in self.weights:
            O, I = w.shape[0], w.shape[1]
            sO, sI, sH, sW = w.stride()
            # fragment-major copies where the LDS-DMA MFMA kernel will consume them (uh_conv3x3_wfrag_ok's channel rules;
            # the caller of lookup() states what its conv call needs and packs for itself when that differs)
            ff = WFRAG and O % 64 == 0 and I % ck == 0
            fd = WFRAG and I % 64 == 0 and O % ck == 0
            self.frags.append((ff, fd))
            rows.append([w.data_ptr(), sO, sI, sH, sW, O, I, off, toff, (1 if ff else 0) | (2 if fd else 0)])
            self.offsets.append(off)
            off += O * 9 * I
            toff += ((O + 31) // 32) * ((I + 31) // 32) * 9
        self.total = off
        self.ntiles = toff
        self.table = torch.tensor(rows, dtype=torch.int64).to(dev)
        self.ptrs = [w.data_ptr() for w in self.weights]
        self.strides = [tuple(w.stride()) for w in self.weights]
        self.wf = torch.empty(self.total, dtype=self.dtype, device=dev)
        self.wd = torch.empty(self.total, dtype=self.dtype, device=dev)
        self.versions = [None] * len(self.weights)
        self.index = {p: i for i, p in enumerate(self.ptrs)}

    def refresh(self):
        if any(w.data_ptr() != p or tuple(w.stride()) != st for w, p, st in zip(self.weights, self.ptrs, self.strides)):
            self._build()                       # a parameter was re-allocated (.to(), load with assign=True, ...)
        LIB.call("uh_pack_w3x3_batched", self.table.data_ptr(), len(self.weights), self.ntiles, self.wf.data_ptr(),
                 self.wd.data_ptr(), UH_BF16 if self.dtype == torch.bfloat16 else UH_F32, _stream())
        self.versions = [w._version for w in self.weights]
        self.epoch = WEIGHT_EPOCH

    def lookup(self, weight: torch.Tensor, dtype: torch.dtype, frag_f: bool = False, frag_d: bool = False):
        """-> (w_fwd, w_dgrad) views if the pack holds the CURRENT value of `weight` in `dtype` in the layouts the caller's
        conv calls need (frag_f / frag_d: fragment-major forward / backward-data copy), else None."""
        if STEP.fp32_mode != "exact" and dtype == torch.float32:
            return None                          # bf16x3 layers pack their own [hi | lo] copies
        i = self.index.get(weight.data_ptr())
        if i is None or dtype != self.dtype or self.epoch != WEIGHT_EPOCH or self.versions[i] != weight._version \
                or self.strides[i] != tuple(weight.stride()) or self.frags[i] != (bool(frag_f), bool(frag_d)):
            return None
        n = weight.shape[0] * 9 * weight.shape[1]
        o = self.offsets[i]
        return self.wf[o:o + n], self.wd[o:o + n]


def conv3x3_fwd(x0: torch.Tensor, x1: Optional[torch.Tensor], w_packed: torch.Tensor, Cout: int,
                want_stats: bool, dt_code: Optional[int] = None, wfrag: bool = False):
    B, H, W, C0 = x0.shape
    C1 = 0 if x1 is None else x1.shape[3]
    dt = _dt(x0) if dt_code is None else dt_code
    y = torch.empty((B, H, W, Cout), dtype=x0.dtype, device=x0.device)
    stats, nslab = None, 0
    if want_stats:
        nslab = LIB.query("uh_conv3x3_stat_slabs", B, H, W, C0 + C1, Cout, dt)
        stats = torch.empty(nslab * (2 * Cout + 2), dtype=torch.float32, device=x0.device)
    name = "conv3x3_fwd_" + _variant((C0, C1), Cout, x0.element_size())
    with _Timed(name, 2.0 * B * H * W * Cout * 9 * (C0 + C1), ("fwd" if want_stats else "dgrad", B, H, W, C0 + C1, Cout)):
        LIB.call("uh_conv3x3_fwd", x0.data_ptr(), C0, pixel_ld(x0), _p(x1), C1, pixel_ld_or0(x1),
                 w_packed.data_ptr(), y.data_ptr(), Cout, Cout, _p(stats), B, H, W, conv_flags(dt, wfrag), _stream())
    return y, stats, nslab


class SlabBatch:
    """Backward-weights reductions that wait for ONE launch (uh_conv3x3_wgrad_partials + uh_slab_reduce_batched).  A conv layer's
    filter gradient only feeds the optimizer, so its closing reduction over the pixel splits -- one 8-14 us launch per layer, in
    the middle of the backward stream -- is queued here instead, with the callback that tells the optimizer (and the gradient
    all-reduce) that the parameter's gradient is final, and flush() runs them all.  The partial results live in workspaces this
    object owns, one per destination (they are written in one step and read at the flush of the same step).
    `flush_bytes`: flush as soon as that many bytes of gradients are pending (data parallel: one bucket's worth, so that the
    bucket's all-reduce can start under the rest of the backward pass); None: only when asked (TrainStepper: after backward)."""

    def __init__(self, flush_bytes: Optional[int] = None):
        self.flush_bytes = flush_bytes
        self.arena = {}                      # one workspace per destination, kept between steps (up to ~37 MB each: close() frees them)
        self.rows, self.callbacks = [], []
        self.pending_bytes = 0
        self._tables = {}                    # row set -> (device table, rows, blocks); data parallel flushes one set per bucket

    def workspace(self, key, nbytes: int, device) -> torch.Tensor:
        ws = self.arena.get(key)
        if ws is None or ws.numel() < nbytes or ws.device != device:
            ws = self.arena[key] = torch.empty(nbytes, dtype=torch.uint8, device=device)
            self._tables.clear()             # a table holds workspace addresses
        return ws

    def add(self, desc, callback):
        self.rows.append(tuple(desc))
        self.callbacks.append(callback)
        self.pending_bytes += 4 * int(desc[2])
        if self.flush_bytes is not None and self.pending_bytes >= self.flush_bytes:
            self.flush()

    def reset(self):
        self.rows, self.callbacks, self.pending_bytes = [], [], 0

    def close(self):
        """Drop the workspaces and the device tables (the next use allocates them again)."""
        self.reset()
        self.arena.clear()
        self._tables.clear()

    def flush(self):
        if not self.rows:
            return
        key = tuple(self.rows)
        entry = self._tables.get(key)
        if entry is None:
            # (same layers, same buffers every step: a table is uploaded once per row set -- through pinned memory, without
            # blocking the host in the middle of backward -- and a captured graph replays with it)
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("SlabBatch: the reduction table would be built (allocation + host-to-device copy) during graph "
                                   "capture; run one eager step first")
            tab, off = [], 0
            for r in self.rows:
                tab.append([r[0], r[1], r[2], r[3], r[4], r[5], off, r[7]])
                off += r[6]
            dev = next(iter(self.arena.values())).device
            host = torch.tensor(tab, dtype=torch.int64).pin_memory()
            entry = self._tables[key] = (host.to(dev, non_blocking=True), len(tab), off, host)     # (host kept until the copy has run)
        table, nrows, blocks = entry[:3]
        with _Timed("slab_reduce_batched", 0.0):
            LIB.call("uh_slab_reduce_batched", table.data_ptr(), nrows, blocks, _stream())
        cbs = self.callbacks
        self.reset()
        for cb in cbs:
            if cb is not None:
                cb(None)


# Queue the closing reductions in STEP.slab_batch.  OFF by default -- measured (round 4, one MI355X, config 2, three interleaved rounds, bf16 slabs): 873.1 images/s with the
# per-layer launches, 872.2 with one batched launch behind the backward pass (B=4: 763.0 / 762.2).  The eighteen launches it
# removes are bandwidth-bound (37 MB each at 5.5 TB/s), not latency-bound, and a layer's slabs are read back from the Infinity
# Cache when the reduction runs at once, from HBM when it runs a millisecond later.  UH_DEFER_SLABS=1 turns it on.
DEFER_SLABS = os.environ.get("UH_DEFER_SLABS", "0") == "1"


def flush_slabs():
    if STEP.slab_batch is not None:
        STEP.slab_batch.flush()


def conv3x3_wgrad(dy: torch.Tensor, x0: torch.Tensor, x1: Optional[torch.Tensor], out_krsc: torch.Tensor,
                  split: bool = False, defer_cb=None) -> bool:
    """dW (fp32 KRSC) of a 3x3 conv.  `defer_cb` (a callable taking one argument): the caller allows the closing reduction to be
    queued in STEP.slab_batch; the callback then fires when it has run.  -> True when the result (and the callback) were deferred."""
    B, H, W, Cout = dy.shape
    C0 = x0.shape[3]
    C1 = 0 if x1 is None else x1.shape[3]
    dt = _dt(dy)
    nbytes = LIB.query("uh_conv3x3_wgrad_ws_bytes", B, H, W, C0 + C1, Cout, dt)
    if split and dt == UH_F32 and C0 % 64 == 0 and C1 % 64 == 0 and Cout % 64 == 0:
        dt = UH_F32X3                          # bf16x3 products (STEP.fp32_mode); same workspace as the fp32 plan
    name = "conv3x3_wgrad_" + ("mfma" if (C0 % 64 == 0 and C1 % 64 == 0 and Cout % 64 == 0) else
                                ("stem" if C0 + C1 <= 4 else "generic"))
    batch = STEP.slab_batch if (defer_cb is not None and DEFER_SLABS and name == "conv3x3_wgrad_mfma") else None
    timed = _Timed(name, 2.0 * B * H * W * Cout * 9 * (C0 + C1), ("wgrad", B, H, W, C0 + C1, Cout))
    if batch is not None:
        ws = batch.workspace(out_krsc.data_ptr(), nbytes, dy.device)
        desc = (ctypes.c_int64 * 8)()
        with timed:
            LIB.call("uh_conv3x3_wgrad_partials", dy.data_ptr(), pixel_ld(dy), x0.data_ptr(), C0, pixel_ld(x0), _p(x1), C1,
                     pixel_ld_or0(x1), out_krsc.data_ptr(), Cout, ws.data_ptr(), nbytes, B, H, W, dt,
                     ctypes.addressof(desc), _stream())
        if desc[3] == 0:                       # a path without slabs: the gradient is final
            return False
        batch.add(list(desc), defer_cb)
        return True
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dy.device)
    with timed:
        LIB.call("uh_conv3x3_wgrad", dy.data_ptr(), pixel_ld(dy), x0.data_ptr(), C0, pixel_ld(x0), _p(x1), C1,
                 pixel_ld_or0(x1), out_krsc.data_ptr(), Cout, ws.data_ptr(), nbytes, B, H, W, dt, _stream())
    return False


def bench_double_conv(B: int, H: int, W: int, Cin: int, Cout: int, dtype: torch.dtype, iters: int = 20):
    """Time the conv kernels of one DoubleConv(Cin -> Cout -> Cout) in isolation: preallocated buffers, the C ABI
    called back to back (`iters` launches between two HIP events on the launch stream, so the figure is kernel
    time, not Python time).  Returns ms and TFLOP/s per kernel; bench.py reports it for the layer the north-star's
    MFMA target is quoted on (the 256-channel DoubleConv)."""
    dev = torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator(device="cpu").manual_seed(0)
    # forward inputs are (BatchNorm -> ReLU) outputs in the network: half zeros, like here (what the operands toggle decides
    # the clock the chip holds under MFMA load); `dyv`, the gradient operand, is dense
    x = torch.relu(torch.randn(B, H, W, Cin, generator=g)).to(dev, dtype)
    h = torch.relu(torch.randn(B, H, W, Cout, generator=g)).to(dev, dtype)
    dyv = torch.randn(B, H, W, Cout, generator=g).to(dev, dtype)
    w1 = (torch.randn(Cout, Cin, 3, 3, generator=g) / (3 * Cin ** 0.5)).to(dev)
    w2 = (torch.randn(Cout, Cout, 3, 3, generator=g) / (3 * Cout ** 0.5)).to(dev)
    dt = _dt(x)
    fr = {"f1": wfrag_ok(B, H, W, Cin, 0, Cout, Cin, 0, Cout, dt), "d1": wfrag_ok(B, H, W, Cout, 0, Cin, Cout, 0, Cin, dt),
          "f2": wfrag_ok(B, H, W, Cout, 0, Cout, Cout, 0, Cout, dt)}
    w1f, w1d = pack_w3x3(w1, dtype, True, frag_f=fr["f1"], frag_d=fr["d1"])
    w2f, w2d = pack_w3x3(w2, dtype, True, frag_f=fr["f2"], frag_d=fr["f2"])
    yo = torch.empty(B, H, W, Cout, dtype=dtype, device=dev)
    xo = torch.empty(B, H, W, Cin, dtype=dtype, device=dev)
    nslab = LIB.query("uh_conv3x3_stat_slabs", B, H, W, Cin, Cout, dt)
    stats = torch.empty(nslab * (2 * Cout + 2), dtype=torch.float32, device=dev)
    dw = torch.empty(Cout * 9 * Cout, dtype=torch.float32, device=dev)
    wsb = max(LIB.query("uh_conv3x3_wgrad_ws_bytes", B, H, W, Cout, Cout, dt),
              LIB.query("uh_conv3x3_wgrad_ws_bytes", B, H, W, Cin, Cout, dt))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    st = _stream()

    def fwd(src, cin, wp, dst, cout, stat, frag=False):
        LIB.call("uh_conv3x3_fwd", src.data_ptr(), cin, cin, None, 0, 0, wp.data_ptr(), dst.data_ptr(), cout, cout,
                 _p(stat), B, H, W, conv_flags(dt, frag), st)

    def wgrad(dy, src, cin):
        LIB.call("uh_conv3x3_wgrad", dy.data_ptr(), Cout, src.data_ptr(), cin, cin, None, 0, 0, dw.data_ptr(), Cout,
                 ws.data_ptr(), wsb, B, H, W, dt, st)

    def timeit(fn, flops):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / iters
        return {"ms": round(ms, 4), "tflops": round(flops / (ms * 1e-3) / 1e12, 1)}

    f1 = 2.0 * B * H * W * Cout * 9 * Cin
    f2 = 2.0 * B * H * W * Cout * 9 * Cout
    out = {
        "shape": f"B{B} {H}x{W} {Cin}->{Cout}->{Cout} {str(dtype)[6:]}",
        "fwd_conv1": timeit(lambda: fwd(x, Cin, w1f, yo, Cout, stats, fr["f1"]), f1),
        "fwd_conv2": timeit(lambda: fwd(h, Cout, w2f, yo, Cout, stats, fr["f2"]), f2),
        "dgrad_conv2": timeit(lambda: fwd(dyv, Cout, w2d, yo, Cout, None, fr["f2"]), f2),
        "dgrad_conv1": timeit(lambda: fwd(dyv, Cout, w1d, xo, Cin, None, fr["d1"]), f1),
        "wgrad_conv2": timeit(lambda: wgrad(dyv, h, Cout), f2),
        "wgrad_conv1": timeit(lambda: wgrad(dyv, x, Cin), f1),
    }
    tot_f = 3 * f2 + 3 * f1
    tot_ms = sum(v["ms"] for k, v in out.items() if isinstance(v, dict))
    out["all_six"] = {"ms": round(tot_ms, 4), "tflops": round(tot_f / (tot_ms * 1e-3) / 1e12, 1)}
    return out


# ----------------------------------------------------------------------------- conv + BN + ReLU
def coef_views(coef: torch.Tensor):
    """-> (scale, shift, mean, rstd): the four per-channel views of a [scale | shift | mean | rstd] buffer."""
    C = coef.numel() // 4
    return coef[:C], coef[C:2 * C], coef[2 * C:3 * C], coef[3 * C:]


def _sync_bn_forward(coef, m2, n_local, Cout, g32, b32, o, nbt_ptr):
    """Merge the per-rank (count, mean, M2) rows into the global-batch statistics: one all_gather of 2C+1 floats per
    layer, then the same uh_bn_finalize over `world` rows (Chan merge in double), which also updates the running
    statistics with the global unbiased variance.  Returns the global pixel count."""
    import torch.distributed as dist
    group, world = STEP.sync_bn
    dev = coef.device
    mean = coef_views(coef)[2]
    row = torch.cat([mean, m2, torch.full((1,), float(n_local), dtype=torch.float32, device=dev)])
    gathered = torch.empty(world * (2 * Cout + 1), dtype=torch.float32, device=dev)
    dist.all_gather(list(gathered.view(world, 2 * Cout + 1).unbind(0)), row, group=group)
    g2 = gathered.view(world, 2 * Cout + 1)
    stats = torch.empty(world * (2 * Cout + 2), dtype=torch.float32, device=dev)
    stats[:world * 2 * Cout].view(world, 2 * Cout).copy_(g2[:, :2 * Cout])
    stats[world * 2 * Cout:world * 2 * Cout + world].copy_(g2[:, 2 * Cout])
    # the global pixel count: this rank's count scaled by global batch / local batch (TrainStepper all-reduces the batch
    # sizes once per step, so ragged shards -- the last batch of an epoch -- get the right variance denominator)
    gb, lb = STEP.sync_bn_batch if STEP.sync_bn_batch is not None else (world, 1)
    n_total = int(n_local) * gb // lb
    LIB.call("uh_bn_finalize", stats.data_ptr(), world, Cout, n_total, g32.data_ptr(), b32.data_ptr(), _p(o.running_mean),
             _p(o.running_var), nbt_ptr, float(o.momentum), float(o.eps), *[v.data_ptr() for v in coef_views(coef)], None, _stream())
    return n_total


def _bn_train_coefficients(stats, nslab, Cout, n, gamma, beta, o, ldc: Optional[int] = None):
    """Per-channel [scale | shift | mean | rstd] from the conv kernels' statistics rows (+ running statistics /
    num_batches_tracked update, + the cross-rank merge under SyncBN; `o`: the layer's ConvBnOpts).  `ldc`: the rows are that many channels wide and only
    the first Cout count (small-width layers: the conv is computed for the padded layer; uh_bn_finalize_ld).
    -> (coef, n_total)"""
    global BN_STATS_EPOCH
    BN_STATS_EPOCH += 1                       # running statistics are about to change under torch's feet
    dev = stats.device
    coef = torch.empty(4 * Cout, dtype=torch.float32, device=dev)
    out = [v.data_ptr() for v in coef_views(coef)]
    g32 = gamma if gamma.dtype == torch.float32 else gamma.float()
    b32 = beta if beta.dtype == torch.float32 else beta.float()
    nbt = o.num_batches_tracked
    fused_nbt = nbt is not None and nbt.is_cuda and nbt.dtype == torch.int64
    nbt_ptr = nbt.data_ptr() if fused_nbt else None
    rows = ("uh_bn_finalize", stats.data_ptr(), nslab) if ldc is None else ("uh_bn_finalize_ld", stats.data_ptr(), nslab, ldc)
    # (SyncBN: this call only forms the local mean / M2; the merge below updates the running statistics)
    m2 = None if STEP.sync_bn is None else torch.empty(Cout, dtype=torch.float32, device=dev)
    running = (_p(o.running_mean), _p(o.running_var), nbt_ptr) if STEP.sync_bn is None else (None, None, None)
    LIB.call(*rows, Cout, n, g32.data_ptr(), b32.data_ptr(), *running, float(o.momentum), float(o.eps), *out, _p(m2), _stream())
    n_total = n if STEP.sync_bn is None else _sync_bn_forward(coef, m2, n, Cout, g32, b32, o, nbt_ptr)
    if nbt is not None and not fused_nbt:
        nbt.add_(1)
    return coef, n_total


def _bn_global_sums(dgamma, dbeta, C, sync_bn):
    """SyncBN: the parameter gradients stay LOCAL sums (the gradient all-reduce SUMS them like every other gradient: the loss
    is already normalised by the global batch); the dx formula needs the GLOBAL sums.  -> (sum for gamma, sum for beta)"""
    import torch.distributed as dist
    glob = torch.cat([dgamma.reshape(-1), dbeta.reshape(-1)])
    dist.all_reduce(glob, op=dist.ReduceOp.SUM, group=sync_bn[0])
    return glob[:C], glob[C:]


def _bn_backward_finish(partials, nblk, C, dgamma, dbeta, sync_bn, n_total, apply):
    """Close BatchNorm backward over `nblk` rows of partial sums: `apply(part_ptr, nb, dg_ptr, db_ptr, n_total)` finishes the
    per-channel sums itself (local statistics), or is handed the global ones and the global pixel count (SyncBN)."""
    if sync_bn is None:
        apply(partials.data_ptr(), nblk, dgamma.data_ptr(), dbeta.data_ptr(), 0)
        return
    LIB.call("uh_bn_bwd_finalize", partials.data_ptr(), nblk, C, dgamma.data_ptr(), dbeta.data_ptr(), _stream())
    sums_g, sums_b = _bn_global_sums(dgamma, dbeta, C, sync_bn)
    apply(None, 0, sums_g.data_ptr(), sums_b.data_ptr(), n_total)


def _bn_param_grads(bufs, wanted):
    """`bufs`: the (buffer, callback) pairs _grad_buffer gave for gamma and beta.  Fires the callbacks -> what autograd gets
    for each: the buffer, or None when the gradient is final in the optimizer's flat buffer or nobody asked for it."""
    out = []
    for (grad, cb), want in zip(bufs, wanted):
        if cb is not None:
            cb()
            grad = None
        out.append(grad if want else None)
    return out


def _unpack_dw3x3(dwk, dweight):
    """KRSC scratch gradient -> the (strided) gradient buffer of a [Cout, Cin, 3, 3] parameter."""
    sO, sI, sH, sW = dweight.stride()
    LIB.call("uh_unpack_dw3x3", dwk.data_ptr(), dweight.data_ptr(), sO, sI, sH, sW, dweight.shape[0], dweight.shape[1], _stream())


def _grads_for(inputs, **grads):
    """backward's answer: one entry per forward input, in order, None where no gradient was named."""
    return tuple(grads.get(k) for k in inputs)


# Fuse BatchNorm + ReLU of a DoubleConv's last conv with its consumer (csrc/bn_fused.hip) in training: TAIL_POOL where the
# activation is skip connection + max-pool input (every encoder level), TAIL_HEAD where it only feeds the 1x1 OutConv.
# False: the separate kernels (A/B measurements; the tests compare both).
FUSE_TAILS = True
TAIL_NONE, TAIL_POOL, TAIL_HEAD, TAIL_UP = 0, 1, 2, 3


def pool_tail_ok(x0: torch.Tensor, Cout: int) -> bool:
    B, H, W, _ = x0.shape
    return bool(FUSE_TAILS and LIB.query("uh_bn_relu_pool_ok", B, H, W, Cout, _dt(x0)))


FUSE_UP_TAIL = os.environ.get("UH_FUSE_UP_TAIL", "1") != "0"      # (A/B switch of the up-sampling tail alone)


def up_tail_ok(x0: torch.Tensor, Cout: int, Ho: int, Wo: int) -> bool:
    """May (BatchNorm -> ReLU -> nn.Upsample(2, bilinear) -> F.pad to Ho x Wo) run as one kernel behind this layer's conv?"""
    B, H, W, _ = x0.shape
    return bool(FUSE_TAILS and FUSE_UP_TAIL and LIB.query("uh_bn_relu_upsample2x_ok", B, H, W, Cout, Ho, Wo, _dt(x0)))


def head_tail_ok(x0: torch.Tensor, Cout: int, head_weight: torch.Tensor) -> bool:
    return bool(FUSE_TAILS and head_weight.shape[1] == Cout and tuple(head_weight.shape[2:]) == (1, 1) and
                LIB.query("uh_bn_relu_head_ok", Cout, head_weight.shape[0], _dt(x0)))


# ---- BatchNorm-backward sums formed by the NEXT conv's backward-data.  Inside a DoubleConv the
# gradient of the activation between the two convs is produced by the second conv's backward-data and read back at once by
# uh_bn_relu_bwd_reduce (that tensor + the first conv's raw output).  uh_conv3x3_dgrad_bnsum forms the two per-channel sums in the
# conv epilogue instead -- accumulators still in registers, one read of the raw output -- and the reduce pass is not launched
# (8 of the 12 plain BatchNorm layers of the bilinear UNet).  UH_FUSE_BNSUM=0 turns it off.
FUSE_BNSUM = os.environ.get("UH_FUSE_BNSUM", "1") != "0"
# Layers (image height x channels of the tensor whose BatchNorm sums are formed, e.g. "32x512,512x64") that keep the separate
# reduce pass although the fusion is on -- per-layer A/B runs and the default exclusion list.
BNSUM_OFF = {tuple(int(v) for v in k.split("x")) for k in os.environ.get("UH_BNSUM_OFF", "").split(",") if k}


class BnSumLink:
    """What ties the two ConvBnReluFn nodes of a DoubleConv together for that fusion: the first layer publishes its raw conv
    output and BatchNorm coefficients in forward; the second layer's backward leaves the partial sums (and the gradient tensor
    they belong to); the first layer's backward uses them if the gradient it receives IS that tensor (autograd hands over the
    same storage when the activation had no other consumer), else it runs the reduce pass as before."""
    __slots__ = ("y", "coef", "dz", "dz_version", "partials", "rows")

    def __init__(self):
        self.y = self.coef = self.dz = self.partials = None
        self.rows = 0
        self.dz_version = -1


class ConvBnOpts(NamedTuple):
    """What a ConvBnReluFn / ConvBnReluNarrowFn call carries besides the tensors that can receive a gradient.
    `tail` (training only): TAIL_POOL -> the node returns (z, maxpool2(z)) (unet_parts.py:32 on top), the backward takes (dskip,
    dpool) and never materialises their sum; TAIL_HEAD -> returns the fp32 logits of the 1x1 OutConv (the node's head_w
    [ncls,Cout,1,1], head_b; unet_parts.py:103) and z is never written; TAIL_UP (up_size = (Ho, Wo)) -> returns the bilinear
    x2 up-sampling of z zero-padded to Ho x Wo (unet_parts.py:70,80,85-88: z's only reader) and z is never written.
    `bnsum_pub` / `bnsum_use` (BnSumLink): this layer is the first / the second conv of a DoubleConv whose
    BatchNorm-backward sums may be formed by the second conv's backward-data.  `c0_true`: see ConvBnReluNarrowFn."""
    running_mean: Optional[torch.Tensor] = None
    running_var: Optional[torch.Tensor] = None
    num_batches_tracked: Optional[torch.Tensor] = None
    training: bool = True
    momentum: float = 0.1
    eps: float = BN_EPS_DEFAULT
    tail: int = TAIL_NONE
    up_size: Optional[Tuple[int, int]] = None
    bnsum_pub: Optional[BnSumLink] = None
    bnsum_use: Optional[BnSumLink] = None
    c0_true: Optional[int] = None


def _conv_bn_relu_eval(x0, x1, weight, gamma, beta, o: ConvBnOpts):
    """inference (model.eval(): evaluate.py:30, predict.py:17): running statistics -> per-channel scale/shift, applied with
    the ReLU inside the conv epilogue (under plan_images: in the pinned kernel form); nothing is kept for a backward pass."""
    B, H, W, C0 = x0.shape
    C1 = 0 if x1 is None else x1.shape[3]
    Cout = weight.shape[0]
    cdt = conv_dt(x0, C0, C1, Cout, False)
    plan = PLAN_IMAGES
    frag = wfrag_ok(B, H, W, C0, C1, Cout, pixel_ld(x0), pixel_ld_or0(x1), Cout, cdt, plan)
    wf = pack_w3x3(weight, x0.dtype, False, cdt)[0] if cdt == UH_F32X3 else packed_w3x3_cached(weight, x0.dtype, frag)
    scale, shift = bn_eval_coeffs_cached(gamma, beta, o.running_mean, o.running_var, o.eps, Cout, Cout)
    z = torch.empty(B, H, W, Cout, dtype=x0.dtype, device=x0.device)
    name, images = ("uh_conv3x3_fwd_affine_relu_plan", (B, plan)) if plan else ("uh_conv3x3_fwd_affine_relu", (B,))
    LIB.call(name, x0.data_ptr(), C0, pixel_ld(x0), _p(x1), C1, pixel_ld_or0(x1), wf.data_ptr(), z.data_ptr(), Cout, Cout,
             scale.data_ptr(), shift.data_ptr(), *images, H, W, conv_flags(cdt, frag), _stream())
    return z


_CBR_INPUTS = ("x0", "x1", "weight", "gamma", "beta", "head_w", "head_b", "opts")
_EVAL_BACKWARD = "backward through eval-mode BatchNorm is not part of the train path"


class ConvBnReluFn(Function):
    """(nn.Conv2d(3x3, pad 1, no bias) -> nn.BatchNorm2d -> nn.ReLU) of unet_parts.py:15-17 / 18-20 as
    one autograd node.  Inputs: x0 (+ optional x1 = second half of the channel concat of
    unet_parts.py:95, never materialised), the reference-layout parameters, the 1x1 head's parameters (TAIL_HEAD, else
    None) and the options record with the BN buffers (ConvBnOpts)."""

    @staticmethod
    def forward(ctx, x0, x1, weight, gamma, beta, head_w, head_b, opts: ConvBnOpts):
        _require_gpu(x0, "activation")
        x0 = dense_nhwc(x0)
        x1 = None if x1 is None else dense_nhwc(x1)
        training, tail = opts.training, opts.tail
        B, H, W, C0 = x0.shape
        C1 = 0 if x1 is None else x1.shape[3]
        Cout, Cin = weight.shape[0], weight.shape[1]
        if Cin != C0 + C1:
            raise RuntimeError(f"conv expects {Cin} input channels, got {C0}+{C1}")
        ctx.training = training
        if not training:
            if tail != TAIL_NONE:
                raise RuntimeError("ConvBnReluFn: fused tails are a training-mode path")
            return _conv_bn_relu_eval(x0, x1, weight, gamma, beta, opts)
        need_dx = any(ctx.needs_input_grad[:2])
        cdt = conv_dt(x0, C0, C1, Cout, need_dx)
        # fragment-major filter packs where the LDS-DMA MFMA kernel runs (forward: this call; backward-data: the conv of dy
        # [B,H,W,Cout] with the transposed filter into dx [B,H,W,Cin])
        frag_f = wfrag_ok(B, H, W, C0, C1, Cout, pixel_ld(x0), pixel_ld_or0(x1), Cout, cdt)
        frag_d = need_dx and wfrag_ok(B, H, W, Cout, 0, Cin, Cout, 0, Cin, cdt)
        pack = STEP.weight_pack
        hit = pack.lookup(weight, x0.dtype, frag_f, frag_d) if (pack is not None and cdt != UH_F32X3) else None
        wf, wd = hit if hit is not None else pack_w3x3(weight, x0.dtype, need_dx, cdt, frag_f, frag_d)
        ctx.cdt, ctx.frag_d = cdt, frag_d
        dev = x0.device
        n = B * H * W
        y, stats, nslab = conv3x3_fwd(x0, x1, wf, Cout, True, cdt, frag_f)
        coef, n_total = _bn_train_coefficients(stats, nslab, Cout, n, gamma, beta, opts)
        scale, shift, mean, rstd = coef_views(coef)
        ctx.bn_params = (gamma, beta)
        ctx.dims = (B, H, W, C0, C1, Cout)
        ctx.n_total = n_total
        ctx.sync_bn = STEP.sync_bn               # (None = per-rank statistics; a one-rank group under UH_DP_FORCE_SYNC still runs the collectives)
        ctx.tail = tail
        ctx.bnsum_pub = ctx.bnsum_use = None
        if FUSE_BNSUM and x0.dtype == torch.bfloat16 and cdt == UH_BF16:
            bnsum_pub, bnsum_use = opts.bnsum_pub, opts.bnsum_use
            if bnsum_pub is not None and tail == TAIL_NONE:
                bnsum_pub.y, bnsum_pub.coef = y, coef
                bnsum_pub.partials = bnsum_pub.dz = None      # (left over when a previous backward never reached this layer)
                ctx.bnsum_pub = bnsum_pub
            if bnsum_use is not None and bnsum_use.y is not None and x1 is None:
                ctx.bnsum_use = bnsum_use
        saved = [x0, x1, y, coef, wd, weight]
        if tail == TAIL_HEAD:
            ncls = head_w.shape[0]
            hw2 = head_w.reshape(ncls, Cout).contiguous().float()
            hb2 = head_b.contiguous().float()
            logits = torch.empty((B, H, W, ncls), dtype=torch.float32, device=dev)
            LIB.call("uh_bn_relu_head_fwd", y.data_ptr(), Cout, scale.data_ptr(), shift.data_ptr(), hw2.data_ptr(),
                     hb2.data_ptr(), logits.data_ptr(), n, Cout, ncls, _dt(y), _stream())
            saved.append(hw2)
            ctx.head_params = (head_w, head_b)
            out = logits
        elif tail == TAIL_UP:
            Ho, Wo = opts.up_size
            pt, pl = _pad_geometry(H, W, Ho, Wo)
            u = torch.empty((B, Ho, Wo, Cout), dtype=y.dtype, device=dev)
            LIB.call("uh_bn_relu_upsample2x_fwd", y.data_ptr(), Cout, scale.data_ptr(), shift.data_ptr(), u.data_ptr(), Cout,
                     B, H, W, Cout, Ho, Wo, pt, pl, _dt(y), _stream())
            ctx.up = (Ho, Wo, pt, pl)
            out = u
        elif tail == TAIL_POOL:
            z = torch.empty_like(y)
            pooled = torch.empty((B, H // 2, W // 2, Cout), dtype=y.dtype, device=dev)
            LIB.call("uh_bn_relu_pool_apply", y.data_ptr(), Cout, scale.data_ptr(), shift.data_ptr(), z.data_ptr(), Cout,
                     pooled.data_ptr(), Cout, B, H, W, Cout, _dt(y), _stream())
            ctx.set_materialize_grads(False)
            out = (z, pooled)
        else:
            out = torch.empty_like(y)
            LIB.call("uh_bn_relu_apply", y.data_ptr(), Cout, scale.data_ptr(), shift.data_ptr(), out.data_ptr(), Cout,
                     n, Cout, _dt(y), _stream())
        ctx.save_for_backward(*saved)
        return out

    @staticmethod
    def backward(ctx, *grads):
        if not ctx.training:
            raise RuntimeError(_EVAL_BACKWARD)
        need = dict(zip(_CBR_INPUTS, ctx.needs_input_grad))
        tail = ctx.tail
        x0, x1, y, coef, wd, weight, *hw2 = ctx.saved_tensors          # (hw2: the head tail's fp32 [ncls, Cout] filter)
        B, H, W, C0, C1, Cout = ctx.dims
        Cin = C0 + C1
        n = B * H * W
        dev = y.device
        scale, shift, mean, rstd = coef_views(coef)
        dt = _dt(y)
        nblk = LIB.query("uh_bn_bwd_nblk", n, Cout)
        partials = torch.empty(nblk * 2 * Cout, dtype=torch.float32, device=dev)
        bn_args = (y.data_ptr(), Cout, scale.data_ptr(), shift.data_ptr(), mean.data_ptr(), rstd.data_ptr())
        dhead = (None, None)
        # The gradient of z: a tensor (no tail), dlogits . head_w (head tail) or dskip + route(dpool) (pool tail) -- the
        # last two are rebuilt inside both BatchNorm passes instead of being stored.  The reduce pass writes the per-block
        # sums, `apply(...)` finishes (or is handed) the per-channel sums and writes dy.
        if tail == TAIL_HEAD:
            dl = grads[0].float().contiguous()
            hw2, = hw2
            ncls = hw2.shape[0]
            head_w, head_b = ctx.head_params
            (dwb, cb_hw), (dbb, cb_hb) = _grad_buffer(head_w, need["head_w"]), _grad_buffer(head_b, need["head_b"])
            direct = cb_hw is not None and cb_hb is not None and dwb.stride(0) == Cout and dwb.stride(1) == 1 and \
                dbb.is_contiguous() and dwb.dtype == torch.float32 and dbb.dtype == torch.float32
            dhw = dwb if direct else torch.empty((ncls, Cout), dtype=torch.float32, device=dev)
            dhb = dbb if direct else torch.empty(ncls, dtype=torch.float32, device=dev)
            nbytes = LIB.query("uh_bn_relu_head_bwd_ws_bytes", n, Cout, ncls)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            LIB.call("uh_bn_relu_head_bwd_reduce", dl.data_ptr(), hw2.data_ptr(), *bn_args, partials.data_ptr(),
                     dhw.data_ptr(), dhb.data_ptr(), ws.data_ptr(), nbytes, n, Cout, ncls, dt, _stream())
            if direct:
                cb_hw()
                cb_hb()

            def apply(part_ptr, nb, dg_ptr, db_ptr, n_total):
                LIB.call("uh_bn_relu_head_bwd_apply", dl.data_ptr(), hw2.data_ptr(), *bn_args, part_ptr, nb, dg_ptr, db_ptr,
                         dy.data_ptr(), Cout, n, n_total, Cout, ncls, dt, _stream())
            dhead = (None, None) if direct else (dhw.view(head_w.shape) if need["head_w"] else None,
                                                 dhb if need["head_b"] else None)
        elif tail == TAIL_POOL and grads[1] is not None:
            dskip, dpool = grads
            dskip, dpool = None if dskip is None else grad_like(dskip, y), grad_like(dpool, y)
            sk = (_p(dskip), pixel_ld_or0(dskip), dpool.data_ptr(), pixel_ld(dpool))
            LIB.call("uh_bn_relu_pool_bwd_reduce", *sk, *bn_args, partials.data_ptr(), B, H, W, Cout, dt, _stream())

            def apply(part_ptr, nb, dg_ptr, db_ptr, n_total):
                LIB.call("uh_bn_relu_pool_bwd_apply", *sk, *bn_args, part_ptr, nb, dg_ptr, db_ptr, dy.data_ptr(), Cout,
                         B, H, W, n_total, Cout, dt, _stream())
        else:
            dz = grads[0]
            if dz is None:          # pool tail whose outputs were both unused
                return _grads_for(_CBR_INPUTS)
            dz = grad_like(dz, y)
            if tail == TAIL_UP:     # the gradient arrives for the up-sampled tensor: transpose of the interpolation first
                Ho, Wo, pt, pl = ctx.up
                du, dz = dz, torch.empty((B, H, W, Cout), dtype=y.dtype, device=dev)
                LIB.call("uh_upsample2x_bwd", du.data_ptr(), pixel_ld(du), dz.data_ptr(), Cout, B, H, W, Cout, Ho, Wo, pt, pl,
                         dt, _stream())
            link = ctx.bnsum_pub
            if link is not None:
                # the sums came with the gradient (uh_conv3x3_dgrad_bnsum in the consumer's backward) -- if this IS that gradient
                # (same storage, same extent, and not written since the sums were formed: a tensor hook or an in-place
                # accumulation that edits the gradient keeps the storage and bumps the version counter)
                if link.partials is not None and link.dz is not None and dz.data_ptr() == link.dz.data_ptr() and \
                        dz.shape == link.dz.shape and dz.stride() == link.dz.stride() and dz._version == link.dz_version:
                    partials, nblk = link.partials, link.rows
                else:
                    link = None
                ctx.bnsum_pub.partials = ctx.bnsum_pub.dz = ctx.bnsum_pub.y = ctx.bnsum_pub.coef = None
            if link is None:
                LIB.call("uh_bn_relu_bwd_reduce", dz.data_ptr(), pixel_ld(dz), *bn_args, partials.data_ptr(), n, Cout, dt, _stream())

            def apply(part_ptr, nb, dg_ptr, db_ptr, n_total):
                LIB.call("uh_bn_relu_bwd_apply", dz.data_ptr(), pixel_ld(dz), *bn_args, part_ptr, nb, dg_ptr, db_ptr,
                         dy.data_ptr(), Cout, n, n_total, Cout, dt, _stream())
        bn_wanted = (need["gamma"], need["beta"])
        bn_bufs = [_grad_buffer(p, w) for p, w in zip(ctx.bn_params, bn_wanted)]
        dy = torch.empty_like(y)
        _bn_backward_finish(partials, nblk, Cout, bn_bufs[0][0], bn_bufs[1][0], ctx.sync_bn, ctx.n_total, apply)
        # backward-data first: it is the only consumer on the critical path (the next layer's BatchNorm backward waits
        # for it).  Backward-weights then goes to the side stream BEHIND it, so that it runs beside the HBM-bound
        # kernels of the layers that follow (BatchNorm backward, pool / upsample backward) instead of beside this
        # layer's own MFMA-bound backward-data.
        dx0 = dx1 = None
        if wd is not None and (need["x0"] or need["x1"]):
            use, rows = ctx.bnsum_use, 0
            if use is not None and use.y is not None and use.y.shape == (B, H, W, Cin) and use.y.is_contiguous() and \
                    (H, Cin) not in BNSUM_OFF:
                rows = LIB.query("uh_conv3x3_dgrad_bnsum_rows", B, H, W, Cout, Cin, Cout, Cin, Cin, ctx.cdt)
            if rows > 0:
                # backward-data + the BatchNorm-backward sums of the layer in front (its reduce pass is not launched)
                dx = torch.empty((B, H, W, Cin), dtype=dy.dtype, device=dev)
                bsum = torch.empty(rows * 2 * Cin, dtype=torch.float32, device=dev)
                # (a kernel family of its own in bench.py's profile: the same MFMA work as plain backward-data plus a read of
                # `use.y` and the sums -- its time is not comparable with the plain launches')
                with _Timed("conv3x3_dgrad_bnsum_mfma", 2.0 * B * H * W * Cin * 9 * Cout, ("dgrad", B, H, W, Cout, Cin)):
                    LIB.call("uh_conv3x3_dgrad_bnsum", dy.data_ptr(), Cout, Cout, wd.data_ptr(), dx.data_ptr(), Cin, Cin,
                             use.y.data_ptr(), Cin, use.coef.data_ptr(), bsum.data_ptr(), B, H, W,
                             conv_flags(ctx.cdt, ctx.frag_d), _stream())
                use.partials, use.rows, use.dz, use.dz_version = bsum, rows, dx, dx._version
            else:
                dx, _, _ = conv3x3_fwd(dy, None, wd, Cin, False, ctx.cdt, ctx.frag_d)
            dx0 = dx[..., :C0] if need["x0"] else None
            dx1 = dx[..., C0:] if (x1 is not None and need["x1"]) else None
        # weight gradient: straight into the parameter's layout when that IS KRSC (channels_last weights)
        dweight = side_done = None
        split = ctx.cdt == UH_F32X3
        if need["weight"]:
            dweight, cb_w = _grad_buffer(weight)
            side = STEP.wgrad_stream
            if cb_w is not None and side is not None and _is_krsc_dense(weight):
                ev = torch.cuda.Event()
                ev.record()                         # dy (and this layer's backward-data) are enqueued before this point
                side.wait_event(ev)
                with torch.cuda.stream(side):
                    conv3x3_wgrad(dy, x0, x1, dweight, split)
                    side_done = torch.cuda.Event()
                    side_done.record()              # the gradient all-reduce of this parameter's bucket waits for THIS
                for t_ in (dy, x0, x1):
                    if t_ is not None:
                        t_.record_stream(side)      # the caching allocator must not recycle them under the side stream
            elif _is_krsc_dense(weight):
                # (straight into the optimizer's flat buffer: the closing reduction may wait for the batched launch, and the
                # "gradient ready" callback with it)
                if conv3x3_wgrad(dy, x0, x1, dweight, split, cb_w):
                    cb_w = None
                    dweight = None
            else:
                dwk = torch.empty(Cout * 9 * Cin, dtype=torch.float32, device=dev)
                conv3x3_wgrad(dy, x0, x1, dwk, split)
                _unpack_dw3x3(dwk, dweight)
            if cb_w is not None:
                cb_w(side_done)
                dweight = None
        dgamma, dbeta = _bn_param_grads(bn_bufs, bn_wanted)
        return _grads_for(_CBR_INPUTS, x0=dx0, x1=dx1, weight=dweight, gamma=dgamma, beta=dbeta, head_w=dhead[0], head_b=dhead[1])


# ----------------------------------------------------------------------------- the stem, output recomputed
# The first layer of the network (inc.double_conv.0-2: Conv2d(Cin <= 4 -> 64) -> BatchNorm2d -> ReLU) with its conv output
# RECOMPUTED by every consumer instead of stored (csrc/conv3x3.hip, stem_bn_bwd_v3): 9 multiply-adds per element against four HBM
# passes over the largest tensor of the model.  bf16 training, single-channel images by default (STEM_RECOMPUTE_MAX_CIN).
STEM_RECOMPUTE = os.environ.get("UH_STEM_RECOMPUTE", "1") != "0"
STEM_RECOMPUTE_MAX_CIN = 1


def stem_recompute_ok(x0: torch.Tensor, Cin: int, Cout: int) -> bool:
    return bool(STEM_RECOMPUTE and x0.dtype == torch.bfloat16 and Cin <= STEM_RECOMPUTE_MAX_CIN and x0.shape[-1] == Cin and
                LIB.query("uh_stem_ok", Cin, Cout, UH_BF16) and x0.shape[0] * x0.shape[1] * x0.shape[2] < 2 ** 31)


class StemConvBnReluFn(Function):
    """(Conv2d(1 -> 64, 3x3, pad 1, no bias) -> BatchNorm2d -> ReLU) of unet_parts.py:15-17 for the network's first
    layer in training: the conv output is never written; statistics, the activation, the BatchNorm-backward sums and the
    filter gradient are each computed from the IMAGE (uh_stem_*).  The image gets no gradient."""

    @staticmethod
    def forward(ctx, x0, weight, gamma, beta, running_mean, running_var, num_batches_tracked, momentum: float, eps: float):
        _require_gpu(x0, "image")
        x0 = dense_nhwc(x0)
        B, H, W, Cin = x0.shape
        Cout = weight.shape[0]
        if weight.shape[1] != Cin or not stem_recompute_ok(x0, Cin, Cout):
            raise RuntimeError("StemConvBnReluFn: bf16 single-channel image into 64 output channels only")
        dev = x0.device
        hit = STEP.weight_pack.lookup(weight, x0.dtype, False, False) if STEP.weight_pack is not None else None
        wf = hit[0] if hit is not None else pack_w3x3(weight, x0.dtype, False)[0]
        n = B * H * W
        nslab = LIB.query("uh_conv3x3_stat_slabs", B, H, W, Cin, Cout, UH_BF16)
        stats = torch.empty(nslab * (2 * Cout + 2), dtype=torch.float32, device=dev)
        with _Timed("conv3x3_fwd_stem", 2.0 * n * Cout * 9 * Cin):
            LIB.call("uh_stem_stats", x0.data_ptr(), Cin, pixel_ld(x0), wf.data_ptr(), stats.data_ptr(), B, H, W, UH_BF16, _stream())
        coef, n_total = _bn_train_coefficients(stats, nslab, Cout, n, gamma, beta, ConvBnOpts(
            running_mean, running_var, num_batches_tracked, momentum=momentum, eps=eps))
        z = torch.empty((B, H, W, Cout), dtype=x0.dtype, device=dev)
        with _Timed("conv3x3_fwd_stem", 2.0 * n * Cout * 9 * Cin):
            LIB.call("uh_stem_bn_relu_fwd", x0.data_ptr(), Cin, pixel_ld(x0), wf.data_ptr(), coef.data_ptr(), coef[Cout:].data_ptr(),
                     z.data_ptr(), Cout, B, H, W, UH_BF16, _stream())
        ctx.save_for_backward(x0, coef, wf, weight)
        ctx.bn_params = (gamma, beta)
        ctx.dims = (B, H, W, Cin, Cout)
        ctx.n_total = n_total
        ctx.sync_bn = STEP.sync_bn               # (None = per-rank statistics; a one-rank group under UH_DP_FORCE_SYNC still runs the collectives)
        return z

    @staticmethod
    def backward(ctx, dz):
        x0, coef, wf, weight = ctx.saved_tensors
        B, H, W, Cin, Cout = ctx.dims
        dev = x0.device
        dz = grad_like(dz, x0)
        scale, shift, mean, rstd = coef_views(coef)
        args = (dz.data_ptr(), pixel_ld(dz), x0.data_ptr(), Cin, pixel_ld(x0), wf.data_ptr(), scale.data_ptr(), shift.data_ptr(),
                mean.data_ptr(), rstd.data_ptr())
        nblk = LIB.query("uh_stem_nblk", B, H, W)
        partials = torch.empty(nblk * 2 * Cout, dtype=torch.float32, device=dev)
        LIB.call("uh_stem_bn_relu_bwd_reduce", *args, partials.data_ptr(), B, H, W, UH_BF16, _stream())
        bn_wanted = ctx.needs_input_grad[2:4]
        bn_bufs = [_grad_buffer(p, w) for p, w in zip(ctx.bn_params, bn_wanted)]
        sums_g, sums_b = bn_bufs[0][0], bn_bufs[1][0]
        # (this node always finalizes first: the sums are an argument of its backward-weights kernel)
        LIB.call("uh_bn_bwd_finalize", partials.data_ptr(), nblk, Cout, sums_g.data_ptr(), sums_b.data_ptr(), _stream())
        if ctx.sync_bn is not None:
            sums_g, sums_b = _bn_global_sums(sums_g, sums_b, Cout, ctx.sync_bn)
        dweight = None
        if ctx.needs_input_grad[1]:
            dweight, cb_w = _grad_buffer(weight)
            nbytes = LIB.query("uh_stem_bwd_wgrad_ws_bytes", B, H, W, Cin)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            direct = _is_krsc_dense(weight)
            dwk = dweight if direct else torch.empty(Cout * 9 * Cin, dtype=torch.float32, device=dev)
            with _Timed("conv3x3_wgrad_stem", 2.0 * B * H * W * Cout * 9 * Cin):
                LIB.call("uh_stem_bn_relu_bwd_wgrad", *args, sums_g.data_ptr(), sums_b.data_ptr(), ctx.n_total, dwk.data_ptr(),
                         ws.data_ptr(), nbytes, B, H, W, UH_BF16, _stream())
            if not direct:
                _unpack_dw3x3(dwk, dweight)
            if cb_w is not None:
                cb_w(None)
                dweight = None
        dgamma, dbeta = _bn_param_grads(bn_bufs, bn_wanted)
        return None, dweight, dgamma, dbeta, None, None, None, None, None


# ----------------------------------------------------------------------------- small-width conv + BN + ReLU
# Small-width layers keep their activations at the real channel count in HBM (False: 64-channel zero-padded tensors, the
# first implementation -- kept for A/B measurements and as the path for channel counts that are not 16-byte multiples).
NARROW_IO = True


def _rup64(c: int) -> int:
    return (c + 63) // 64 * 64


def narrow_ok(x0: torch.Tensor, x1: Optional[torch.Tensor], Cout: int) -> bool:
    """Can this layer run on the narrow-tensor conv entry points?  (every stored channel count a multiple of one
    16-byte piece, 16-byte aligned pixel rows)"""
    vec = 16 // x0.element_size()
    for t in (x0, x1):
        if t is None:
            continue
        if t.shape[-1] % vec or (pixel_ld(t) * t.element_size()) % 16 or t.data_ptr() % 16:
            return False
    return Cout % vec == 0


def _narrow_dims(x0, x1, Cout):
    """-> stored channels of both sources, then the 64-aligned counts the layer is computed at (sources, output)."""
    C0m, C1m = x0.shape[3], 0 if x1 is None else x1.shape[3]
    return C0m, C1m, _rup64(C0m), _rup64(C1m) if C1m else 0, _rup64(Cout)


def _narrow_fwd(x0, x1, wf, out, stats, scale, shift, cdt, plan=0):
    """uh_conv3x3_fwd_narrow(_plan) of a small-width layer into `out`: statistics rows (training) or the eval-mode scale /
    shift + ReLU in the epilogue."""
    B, H, W, Cout = out.shape
    C0m, C1m, Cp0, Cp1, Cop = _narrow_dims(x0, x1, Cout)
    name, images = ("uh_conv3x3_fwd_narrow_plan", (B, plan)) if plan else ("uh_conv3x3_fwd_narrow", (B,))
    with _Timed("conv3x3_fwd_narrow", 2.0 * B * H * W * Cop * 9 * (Cp0 + Cp1)):
        LIB.call(name, x0.data_ptr(), Cp0, C0m, pixel_ld(x0), _p(x1), Cp1, C1m, pixel_ld_or0(x1), wf.data_ptr(),
                 out.data_ptr(), Cout, Cop, Cout, _p(stats), _p(scale), _p(shift), *images, H, W, cdt, _stream())


def _conv_bn_relu_narrow_eval(x0, x1, wf, cdt, Cout, gamma, beta, o: ConvBnOpts):
    B, H, W, _ = x0.shape
    # scale / shift are read in 16-byte pieces for every padded channel group: Cop entries, the first Cout real
    scale, shift = bn_eval_coeffs_cached(gamma, beta, o.running_mean, o.running_var, o.eps, Cout, _rup64(Cout))
    z = torch.empty(B, H, W, Cout, dtype=x0.dtype, device=x0.device)
    _narrow_fwd(x0, x1, wf, z, None, scale, shift, cdt, PLAN_IMAGES)
    return z


_NARROW_INPUTS = ("x0", "x1", "weight", "gamma", "beta", "opts")


class ConvBnReluNarrowFn(Function):
    """(Conv2d 3x3 -> BatchNorm2d -> ReLU) of unet_parts.py:15-20 for the small-width models (UNet_S / UNet_T,
    unet_model.py:52-126): COMPUTED as the next 64-aligned layer -- zero filters / unit gamma in the padding, so the
    MFMA kernels of the full-width UNet apply -- while every activation in HBM (x, raw conv output, z and their
    gradients) keeps its real channel count: the conv kernels read channels beyond the stored count as zeros and never
    write them (uh_conv3x3_fwd_narrow / uh_conv3x3_wgrad_narrow).  `opts.c0_true`: x0 may itself carry zero channels up to
    a 16-byte piece (the 1- or 3-channel input image); only its first c0_true channels meet filter taps."""

    @staticmethod
    def forward(ctx, x0, x1, weight, gamma, beta, opts: ConvBnOpts):
        _require_gpu(x0, "activation")
        x0 = dense_nhwc(x0)
        x1 = None if x1 is None else dense_nhwc(x1)
        training, c0_true = opts.training, opts.c0_true
        B, H, W, _ = x0.shape
        Cout, Cin = weight.shape[0], weight.shape[1]
        C0m, C1m, Cp0, Cp1, Cop = _narrow_dims(x0, x1, Cout)
        if Cin != c0_true + C1m or c0_true > C0m:
            raise RuntimeError(f"conv expects {Cin} input channels, got {c0_true}+{C1m}")
        if not narrow_ok(x0, x1, Cout):
            raise RuntimeError("narrow conv: stored channel counts / strides must be multiples of 16 bytes")
        Cinp, dev, single = Cp0 + Cp1, x0.device, x1 is None
        want_wd = (training and ctx.needs_input_grad[0], training and not single and ctx.needs_input_grad[1])
        cdt = conv_dt(x0, Cp0, Cp1, Cop, any(want_wd))
        w32 = weight if weight.dtype == torch.float32 else weight.float()
        wd0 = wd1 = None
        if cdt == UH_F32X3:
            # bf16x3 packs are [hi | lo] pairs, so the per-source backward-data filters cannot be row blocks of one pack:
            # pad with torch, pack per source
            with torch.no_grad():
                wp = torch.zeros(Cop, Cinp, 3, 3, dtype=torch.float32, device=dev)
                wp[:Cout, :c0_true] = w32[:, :c0_true]
                if C1m:
                    wp[:Cout, Cp0:Cp0 + C1m] = w32[:, c0_true:]
            wf, wd0 = pack_w3x3(wp, x0.dtype, want_wd[0] and single, cdt)
            if training and not single:
                wd0 = pack_w3x3(wp[:, :Cp0], x0.dtype, True, cdt)[1] if want_wd[0] else None
                wd1 = pack_w3x3(wp[:, Cp0:], x0.dtype, True, cdt)[1] if want_wd[1] else None
        else:
            # one launch: zero-padded forward pack + backward-data pack whose row blocks are the per-source filters
            wf = torch.empty(Cop * 9 * Cinp, dtype=x0.dtype, device=dev)
            wd = torch.empty(Cop * 9 * Cinp, dtype=x0.dtype, device=dev) if any(want_wd) else None
            sO, sI, sH, sW = w32.stride()
            LIB.call("uh_pack_w3x3_padded", w32.data_ptr(), sO, sI, sH, sW, Cout, c0_true, C1m, Cop, Cp0, Cp1, wf.data_ptr(),
                     _p(wd), cdt, _stream())
            if wd is not None:
                wd0 = wd[:Cp0 * 9 * Cop] if want_wd[0] else None
                wd1 = wd[Cp0 * 9 * Cop:] if want_wd[1] else None
        ctx.training = training
        if not training:
            return _conv_bn_relu_narrow_eval(x0, x1, wf, cdt, Cout, gamma, beta, opts)
        n = B * H * W
        y = torch.empty(B, H, W, Cout, dtype=x0.dtype, device=dev)
        nslab = LIB.query("uh_conv3x3_stat_slabs", B, H, W, Cinp, Cop, cdt)
        stats = torch.empty(nslab * (2 * Cop + 2), dtype=torch.float32, device=dev)
        _narrow_fwd(x0, x1, wf, y, stats, None, None, cdt)
        # statistics rows are Cop channels wide (the conv is computed for the padded layer); only the Cout real ones count
        coef, n_total = _bn_train_coefficients(stats, nslab, Cout, n, gamma, beta, opts, ldc=Cop)
        scale, shift, _, _ = coef_views(coef)
        z = torch.empty_like(y)
        LIB.call("uh_bn_relu_apply", y.data_ptr(), Cout, scale.data_ptr(), shift.data_ptr(), z.data_ptr(), Cout, n, Cout,
                 _dt(y), _stream())
        ctx.save_for_backward(x0, x1, y, coef, wd0, wd1, weight)
        ctx.bn_params = (gamma, beta)
        ctx.dims = (B, H, W, Cout, c0_true)
        ctx.cdt = cdt
        ctx.n_total = n_total
        ctx.sync_bn = STEP.sync_bn               # (None = per-rank statistics; a one-rank group under UH_DP_FORCE_SYNC still runs the collectives)
        return z

    @staticmethod
    def backward(ctx, dz):
        if not ctx.training:
            raise RuntimeError(_EVAL_BACKWARD)
        need = dict(zip(_NARROW_INPUTS, ctx.needs_input_grad))
        x0, x1, y, coef, wd0, wd1, weight = ctx.saved_tensors
        B, H, W, Cout, c0_true = ctx.dims
        C0m, C1m, Cp0, Cp1, Cop = _narrow_dims(x0, x1, Cout)
        Cinp = Cp0 + Cp1
        n = B * H * W
        dev = y.device
        dz = grad_like(dz, y)
        scale, shift, mean, rstd = coef_views(coef)
        dt = _dt(y)
        nblk = LIB.query("uh_bn_bwd_nblk", n, Cout)
        partials = torch.empty(nblk * 2 * Cout, dtype=torch.float32, device=dev)
        bn_args = (dz.data_ptr(), pixel_ld(dz), y.data_ptr(), Cout, scale.data_ptr(), shift.data_ptr(), mean.data_ptr(), rstd.data_ptr())
        LIB.call("uh_bn_relu_bwd_reduce", *bn_args, partials.data_ptr(), n, Cout, dt, _stream())
        bn_wanted = (need["gamma"], need["beta"])
        bn_bufs = [_grad_buffer(p, w) for p, w in zip(ctx.bn_params, bn_wanted)]
        dy = torch.empty_like(y)

        def apply(part_ptr, nb, dg_ptr, db_ptr, n_total):
            LIB.call("uh_bn_relu_bwd_apply", *bn_args, part_ptr, nb, dg_ptr, db_ptr, dy.data_ptr(), Cout, n, n_total, Cout, dt,
                     _stream())
        _bn_backward_finish(partials, nblk, Cout, bn_bufs[0][0], bn_bufs[1][0], ctx.sync_bn, ctx.n_total, apply)
        # backward-data: the padded layer's transposed conv, once per source, each writing its own narrow dx
        dx = [None, None]
        for i, (wd, Cp, Cm) in enumerate(((wd0, Cp0, C0m), (wd1, Cp1, C1m))):
            if wd is None or not ctx.needs_input_grad[i]:
                continue
            dx[i] = torch.empty(B, H, W, Cm, dtype=y.dtype, device=dev)
            with _Timed("conv3x3_fwd_narrow", 2.0 * n * Cop * 9 * Cp):
                LIB.call("uh_conv3x3_fwd_narrow", dy.data_ptr(), Cop, Cout, Cout, None, 0, 0, 0, wd.data_ptr(),
                         dx[i].data_ptr(), Cm, Cp, Cm, None, None, None, B, H, W, ctx.cdt, _stream())
        dweight = None
        if need["weight"]:
            wdt = UH_F32X3 if (ctx.cdt == UH_F32X3) else dt
            nbytes = LIB.query("uh_conv3x3_wgrad_ws_bytes", B, H, W, Cinp, Cop, dt)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            dwk = torch.empty(Cop, 3, 3, Cinp, dtype=torch.float32, device=dev)
            with _Timed("conv3x3_wgrad_narrow", 2.0 * n * Cop * 9 * Cinp):
                LIB.call("uh_conv3x3_wgrad_narrow", dy.data_ptr(), Cout, Cop, Cout, x0.data_ptr(), Cp0, C0m, pixel_ld(x0),
                         _p(x1), Cp1, C1m, pixel_ld_or0(x1), dwk.data_ptr(), ws.data_ptr(), nbytes,
                         B, H, W, wdt, _stream())
            dweight, cb_w = _grad_buffer(weight)
            dweight[:, :c0_true].copy_(dwk[:Cout, :, :, :c0_true].permute(0, 3, 1, 2))
            if C1m:
                dweight[:, c0_true:].copy_(dwk[:Cout, :, :, Cp0:Cp0 + C1m].permute(0, 3, 1, 2))
            if cb_w is not None:
                cb_w()
                dweight = None
        dgamma, dbeta = _bn_param_grads(bn_bufs, bn_wanted)
        return _grads_for(_NARROW_INPUTS, x0=dx[0], x1=dx[1], weight=dweight, gamma=dgamma, beta=dbeta)


# ----------------------------------------------------------------------------- max-pool
def _maxpool_fwd(x):
    B, H, W, C = x.shape
    y = torch.empty((B, H // 2, W // 2, C), dtype=x.dtype, device=x.device)
    LIB.call("uh_maxpool2_fwd", x.data_ptr(), pixel_ld(x), y.data_ptr(), C, B, H, W, C, _dt(x), _stream())
    return y


def _maxpool_bwd(x, dy, dskip):
    B, H, W, C = x.shape
    dx = torch.empty((B, H, W, C), dtype=x.dtype, device=x.device)
    dy = dense_nhwc(dy if dy.dtype == x.dtype else dy.to(x.dtype))
    if dskip is not None:
        dskip = dense_nhwc(dskip if dskip.dtype == x.dtype else dskip.to(x.dtype))
    LIB.call("uh_maxpool2_bwd", x.data_ptr(), pixel_ld(x), dy.data_ptr(), pixel_ld(dy), _p(dskip),
             0 if dskip is None else pixel_ld(dskip), dx.data_ptr(), C, B, H, W, C, _dt(x), _stream())
    return dx


class MaxPool2Fn(Function):
    """nn.MaxPool2d(2) (unet_parts.py:32)."""

    @staticmethod
    def forward(ctx, x):
        _require_gpu(x, "activation")
        x = dense_nhwc(x)
        ctx.save_for_backward(x)
        return _maxpool_fwd(x)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        return _maxpool_bwd(x, dy, None)


class PoolSplitFn(Function):
    """x -> (x as the skip connection, maxpool(x)).  One node so that the backward adds the skip
    gradient and routes the pooled gradient in a single pass (unet_model.py:28-32 uses every
    encoder output twice)."""

    @staticmethod
    def forward(ctx, x):
        _require_gpu(x, "activation")
        x = dense_nhwc(x)
        ctx.save_for_backward(x)
        ctx.set_materialize_grads(False)
        return x.view_as(x), _maxpool_fwd(x)

    @staticmethod
    def backward(ctx, dskip, dpool):
        (x,) = ctx.saved_tensors
        if dpool is None:
            return dskip
        return _maxpool_bwd(x, dpool, dskip)


# ----------------------------------------------------------------------------- upsample / convT (+ pad)
def _pad_geometry(h, w, Ho, Wo):
    """F.pad(x1, [dX//2, dX-dX//2, dY//2, dY-dY//2]) of unet_parts.py:85-88 (Python floor division)."""
    dY, dX = Ho - 2 * h, Wo - 2 * w
    return dY // 2, dX // 2


class UpsampleBilinearPadFn(Function):
    """nn.Upsample(scale_factor=2, mode='bilinear', align_corners=True) + F.pad (unet_parts.py:70,85-88)."""

    @staticmethod
    def forward(ctx, x, Ho: int, Wo: int):
        _require_gpu(x, "activation")
        x = dense_nhwc(x)
        B, h, w, C = x.shape
        pt, pl = _pad_geometry(h, w, Ho, Wo)
        y = torch.empty((B, Ho, Wo, C), dtype=x.dtype, device=x.device)
        LIB.call("uh_upsample2x_fwd", x.data_ptr(), pixel_ld(x), y.data_ptr(), C, B, h, w, C, Ho, Wo, pt, pl,
                 _dt(x), _stream())
        ctx.geom = (B, h, w, C, Ho, Wo, pt, pl)
        return y

    @staticmethod
    def backward(ctx, dy):
        B, h, w, C, Ho, Wo, pt, pl = ctx.geom
        dy = dense_nhwc(dy)
        dx = torch.empty((B, h, w, C), dtype=dy.dtype, device=dy.device)
        LIB.call("uh_upsample2x_bwd", dy.data_ptr(), pixel_ld(dy), dx.data_ptr(), C, B, h, w, C, Ho, Wo, pt, pl,
                 _dt(dy), _stream())
        return dx, None, None


class ConvTranspose2x2PadFn(Function):
    """nn.ConvTranspose2d(Cin, Cin//2, 2, stride=2) + F.pad (unet_parts.py:73,85-88).  MFMA GEMMs over pixels
    (csrc/convt_mfma.hip) when the shape qualifies, else the LDS-tiled SIMT kernels of csrc/convt_1x1.hip."""

    @staticmethod
    def forward(ctx, x, weight, bias, Ho: int, Wo: int, training: bool = True):
        _require_gpu(x, "activation")
        x = dense_nhwc(x)
        B, h, w, Cin = x.shape
        Cout = weight.shape[1]
        wc = weight.contiguous().float()
        bc = bias.contiguous().float()
        pt, pl = _pad_geometry(h, w, Ho, Wo)
        y = torch.empty((B, Ho, Wo, Cout), dtype=x.dtype, device=x.device)
        dt = _dt(x)
        if PLAN_IMAGES and not training:      # eval forward under plan_images: the choice one image gets
            mfma = bool(LIB.query("uh_convt2x2_mfma_ok_plan", B, PLAN_IMAGES, h, w, Cin, Cout, Ho, Wo, dt))
        else:
            mfma = bool(LIB.query("uh_convt2x2_mfma_ok", B, h, w, Cin, Cout, Ho, Wo, dt))
        if mfma and dt == UH_F32 and STEP.fp32_mode == "bf16x3":
            dt = UH_F32X3                    # split products on the bf16 matrix pipe (both operands split in registers)
        wd = None
        if mfma:
            wf = torch.empty(Cin * Cout * 4, dtype=x.dtype, device=x.device)
            wd = torch.empty(Cin * Cout * 4, dtype=x.dtype, device=x.device)
            LIB.call("uh_convt2x2_pack", wc.data_ptr(), Cin, Cout, wf.data_ptr(), wd.data_ptr(), dt, _stream())
            with _Timed("convt2x2_fwd_mfma", 2.0 * B * h * w * Cin * 4 * Cout):
                LIB.call("uh_convt2x2_fwd_mfma", x.data_ptr(), pixel_ld(x), wf.data_ptr(), bc.data_ptr(), y.data_ptr(), Cout,
                         B, h, w, Cin, Cout, Ho, Wo, pt, pl, dt, _stream())
        else:
            LIB.call("uh_convt2x2_fwd", x.data_ptr(), pixel_ld(x), wc.data_ptr(), bc.data_ptr(), y.data_ptr(), Cout,
                     B, h, w, Cin, Cout, Ho, Wo, pt, pl, dt, _stream())
        ctx.save_for_backward(x, wc, wd)
        ctx.geom = (B, h, w, Cin, Cout, Ho, Wo, pt, pl)
        ctx.dt = dt
        return y

    @staticmethod
    def backward(ctx, dy):
        x, wc, wd = ctx.saved_tensors
        B, h, w, Cin, Cout, Ho, Wo, pt, pl = ctx.geom
        dy = dense_nhwc(dy if dy.dtype == x.dtype else dy.to(x.dtype))
        dt = ctx.dt
        mfma = wd is not None
        # dy usually is the [.., C:] half of the gradient of the concatenated tensor (pixel stride 2 x Cout): the MFMA kernels address
        # it through a 2 GiB buffer window that uh_convt2x2_mfma_ok sized for the PACKED tensor -- pack it when the strided walk
        # would pass that window (32 x 512 x 512 x 64 bf16 channels inside a 128-channel gradient: bench.py's global-batch-32 leg)
        if mfma and dy.shape[0] * dy.shape[1] * dy.shape[2] * pixel_ld(dy) * dy.element_size() >= (1 << 31) - 4096:
            dy = dy.contiguous()
        flops = 2.0 * B * h * w * Cin * 4 * Cout
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty((B, h, w, Cin), dtype=x.dtype, device=x.device)
            if mfma:
                with _Timed("convt2x2_dgrad_mfma", flops):
                    LIB.call("uh_convt2x2_dgrad_mfma", dy.data_ptr(), pixel_ld(dy), wd.data_ptr(), dx.data_ptr(), Cin, B, h, w,
                             Cin, Cout, Ho, Wo, pt, pl, dt, _stream())
            else:
                LIB.call("uh_convt2x2_dgrad", dy.data_ptr(), pixel_ld(dy), wc.data_ptr(), dx.data_ptr(), Cin, B, h, w,
                         Cin, Cout, Ho, Wo, pt, pl, dt, _stream())
        dw = torch.empty((Cin, Cout, 2, 2), dtype=torch.float32, device=x.device)
        db = torch.empty(Cout, dtype=torch.float32, device=x.device)
        if mfma:
            nbytes = LIB.query("uh_convt2x2_wgrad_mfma_ws_bytes", B, h, w, Cin, Cout, dt)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
            with _Timed("convt2x2_wgrad_mfma", flops):
                LIB.call("uh_convt2x2_wgrad_mfma", dy.data_ptr(), pixel_ld(dy), x.data_ptr(), pixel_ld(x), dw.data_ptr(),
                         db.data_ptr(), ws.data_ptr(), nbytes, B, h, w, Cin, Cout, Ho, Wo, pt, pl, dt, _stream())
        else:
            nbytes = LIB.query("uh_convt2x2_wgrad_ws_bytes", B, h, w, Cin, Cout)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
            LIB.call("uh_convt2x2_wgrad", dy.data_ptr(), pixel_ld(dy), x.data_ptr(), pixel_ld(x), dw.data_ptr(),
                     db.data_ptr(), ws.data_ptr(), nbytes, B, h, w, Cin, Cout, Ho, Wo, pt, pl, dt, _stream())
        return dx, dw, db, None, None, None


# ----------------------------------------------------------------------------- spatial attention
def _sa_weight(weight: torch.Tensor):
    k = int(weight.shape[-1])
    if tuple(weight.shape) != (1, 2, k, k) or k not in (3, 7):
        raise RuntimeError(f"SpatialAttention weight must be [1, 2, k, k] with k in (3, 7), got {tuple(weight.shape)}")
    return weight.detach().float().contiguous(), k


def _sa_forward(ctx, x, weight, gate: bool):
    _require_gpu(x, "activation")
    x = dense_nhwc(x)
    B, H, W, C = x.shape
    wc, k = _sa_weight(weight)
    npix = B * H * W
    pool = torch.empty((npix, 2), dtype=torch.float32, device=x.device)
    amax = torch.empty(npix, dtype=torch.int32, device=x.device)
    a = torch.empty((B, H, W, 1), dtype=torch.float32, device=x.device)
    y = torch.empty((B, H, W, C), dtype=x.dtype, device=x.device) if gate else None
    LIB.call("uh_spatial_attn_fwd", x.data_ptr(), pixel_ld(x), wc.data_ptr(), k, pool.data_ptr(), amax.data_ptr(),
             a.data_ptr(), _p(y), C, B, H, W, C, _dt(x), _stream())
    ctx.save_for_backward(x if gate else None, wc, pool, amax, a)
    ctx.geom = (B, H, W, C, k, tuple(weight.shape), x.dtype)
    return y if gate else a


def _sa_backward(ctx, dy, ga):
    x, wc, pool, amax, a = ctx.saved_tensors
    B, H, W, C, k, wshape, dtype = ctx.geom
    if dy is not None:
        dy = dense_nhwc(dy if dy.dtype == dtype else dy.to(dtype))
    else:
        ga = ga.float().contiguous()
    dev = pool.device
    ws = torch.empty(3 * B * H * W, dtype=torch.float32, device=dev)
    dx = torch.empty((B, H, W, C), dtype=dtype, device=dev)
    dw = torch.empty(wshape, dtype=torch.float32, device=dev)
    nblk = LIB.query("uh_spatial_attn_dw_nblk", B, H, W)
    part = torch.empty((nblk, 2 * k * k), dtype=torch.float32, device=dev)
    LIB.call("uh_spatial_attn_bwd", _p(dy), 0 if dy is None else pixel_ld(dy), _p(ga), _p(x), 0 if x is None else pixel_ld(x),
             wc.data_ptr(), k, pool.data_ptr(), amax.data_ptr(), a.data_ptr(), ws.data_ptr(), dx.data_ptr(), C, dw.data_ptr(),
             part.data_ptr(), nblk, B, H, W, C, UH_BF16 if dtype == torch.bfloat16 else UH_F32, _stream())
    return dx, dw


class SpatialAttnMapFn(Function):
    """SpatialAttention.forward (unet_parts.py:50-60): x [B,H,W,C] -> a = sigmoid(conv_kxk([mean_c x, max_c x])) as fp32
    [B,H,W,1].  The max's gradient goes to the FIRST maximal channel, as torch.max(dim=1) routes it."""

    @staticmethod
    def forward(ctx, x, weight):
        return _sa_forward(ctx, x, weight, gate=False)

    @staticmethod
    def backward(ctx, ga):
        return _sa_backward(ctx, None, ga)


class SpatialAttnGateFn(Function):
    """The gated skip of Up(use_attention=True) (unet_parts.py:91-92): y = x * SpatialAttention(x), one node (the map
    never leaves the kernels as a tensor of the graph); y is rounded once to x's dtype."""

    @staticmethod
    def forward(ctx, x, weight):
        return _sa_forward(ctx, x, weight, gate=True)

    @staticmethod
    def backward(ctx, dy):
        return _sa_backward(ctx, dy, None)


# ----------------------------------------------------------------------------- OutConv
class OutConv1x1Fn(Function):
    """nn.Conv2d(Cin, n_classes, kernel_size=1) with bias (unet_parts.py:103); logits are fp32."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        _require_gpu(x, "activation")
        x = dense_nhwc(x)
        B, H, W, Cin = x.shape
        ncls = weight.shape[0]
        w2 = weight.reshape(ncls, Cin).contiguous().float()
        b2 = bias.contiguous().float()
        logits = torch.empty((B, H, W, ncls), dtype=torch.float32, device=x.device)
        LIB.call("uh_conv1x1_fwd", x.data_ptr(), pixel_ld(x), w2.data_ptr(), b2.data_ptr(), logits.data_ptr(),
                 B * H * W, Cin, ncls, _dt(x), _stream())
        ctx.save_for_backward(x, w2)
        ctx.wshape = tuple(weight.shape)
        ctx.params = (weight, bias)
        return logits

    @staticmethod
    def backward(ctx, dl):
        x, w2 = ctx.saved_tensors
        B, H, W, Cin = x.shape
        ncls = w2.shape[0]
        n = B * H * W
        dl = dl.float().contiguous()
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty((B, H, W, Cin), dtype=x.dtype, device=x.device)
            LIB.call("uh_conv1x1_dgrad", dl.data_ptr(), w2.data_ptr(), dx.data_ptr(), Cin, n, Cin, ncls, _dt(x), _stream())
        nbytes = LIB.query("uh_conv1x1_wgrad_ws_bytes", n, Cin, ncls)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        # straight into the optimizer's flat gradient buffer when the parameter is registered there (FusedRMSprop) and its
        # [n_classes][Cin] plane is dense -- a 1x1 filter has the same memory order in contiguous and channels_last layout
        weight, bias = ctx.params
        (dwb, cb_w), (dbb, cb_b) = _grad_buffer(weight, ctx.needs_input_grad[1]), _grad_buffer(bias, ctx.needs_input_grad[2])
        direct = cb_w is not None and cb_b is not None and dwb.stride(0) == Cin and dwb.stride(1) == 1 and \
            dbb.is_contiguous() and dwb.dtype == torch.float32 and dbb.dtype == torch.float32
        if direct:
            dw, db = dwb, dbb
        else:
            dw = torch.empty((ncls, Cin), dtype=torch.float32, device=x.device)
            db = torch.empty(ncls, dtype=torch.float32, device=x.device)
        LIB.call("uh_conv1x1_wgrad", dl.data_ptr(), x.data_ptr(), pixel_ld(x), dw.data_ptr(), db.data_ptr(),
                 ws.data_ptr(), nbytes, n, Cin, ncls, _dt(x), _stream())
        if direct:
            cb_w()
            cb_b()
            return dx, None, None
        return dx, dw.view(ctx.wshape) if ctx.needs_input_grad[1] else None, db if ctx.needs_input_grad[2] else None


# ----------------------------------------------------------------------------- inference masks
def argmax_classes(mask_pred: torch.Tensor) -> torch.Tensor:
    """`mask_pred.argmax(dim=1)` of predict.py:27 / evaluate.py:111 for logits [B,C,H,W] -> int64 [B,H,W]."""
    _require_gpu(mask_pred, "logits")
    if mask_pred.dim() != 4:
        raise RuntimeError(f"argmax_classes expects [B,C,H,W] logits, got {tuple(mask_pred.shape)}")
    B, C, H, W = mask_pred.shape
    v = mask_pred.permute(0, 2, 3, 1)
    if v.dtype != torch.float32 or not v.is_contiguous():
        v = v.float().contiguous()
    out = torch.empty(B, H, W, dtype=torch.int64, device=v.device)
    LIB.call("uh_argmax_classes", v.data_ptr(), B * H * W, C, out.data_ptr(), _stream())
    return out


def threshold_mask(logits: torch.Tensor) -> torch.Tensor:
    """`(torch.sigmoid(logits) > 0.5).float()` of evaluate.py:60-62, computed as logits > 0."""
    _require_gpu(logits, "logits")
    v = logits if (logits.dtype == torch.float32 and logits.is_contiguous()) else logits.float().contiguous()
    out = torch.empty(v.shape, dtype=torch.float32, device=v.device)
    LIB.call("uh_threshold_mask", v.data_ptr(), v.numel(), out.data_ptr(), _stream())
    return out


# ----------------------------------------------------------------------------- predict.py byte stages (csrc/predict_io.hip)
def predict_prepare_u8(img_u8: torch.Tensor, out: Optional[torch.Tensor] = None, flags: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 [B,H,W] decoded grey images -> float32 [B,1,H,W]: `/ 255` for every image that holds a byte > 1, the raw
    0.0 / 1.0 otherwise (data_loading.py:86-87 decided per image, on the device)."""
    _require_gpu(img_u8, "images")
    if img_u8.dtype != torch.uint8 or img_u8.dim() != 3 or not img_u8.is_contiguous():
        raise RuntimeError(f"predict_prepare_u8 takes a contiguous uint8 [B,H,W] batch, got {img_u8.dtype} {tuple(img_u8.shape)}")
    B, H, W = img_u8.shape
    if out is None:
        out = torch.empty(B, 1, H, W, dtype=torch.float32, device=img_u8.device)
    if flags is None:
        flags = torch.empty(B, dtype=torch.int32, device=img_u8.device)
    if out.dtype != torch.float32 or out.numel() != B * H * W or not out.is_contiguous() or flags.numel() < B:
        raise RuntimeError("predict_prepare_u8: output must be a contiguous float32 [B,1,H,W] and flags an int32 [B]")
    LIB.call("uh_predict_prepare_u8", img_u8.data_ptr(), out.data_ptr(), flags.data_ptr(), B, H, W, _stream())
    return out


def logits_to_classes_u8(mask_pred: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`mask_pred.argmax(dim=1)` as uint8 [B,H,W] for logits [B,C,H,W] (fp32 or bf16; read through their NHWC view); the
    int64 map of argmax_classes is not materialised."""
    _require_gpu(mask_pred, "logits")
    if mask_pred.dim() != 4 or mask_pred.shape[1] > 256:
        raise RuntimeError(f"logits_to_classes_u8 expects [B,C<=256,H,W] logits, got {tuple(mask_pred.shape)}")
    B, C, H, W = mask_pred.shape
    v = mask_pred.permute(0, 2, 3, 1)
    if v.dtype not in (torch.float32, torch.bfloat16):
        v = v.float()
    if not v.is_contiguous():
        v = v.contiguous()
    if out is None:
        out = torch.empty(B, H, W, dtype=torch.uint8, device=v.device)
    if out.dtype != torch.uint8 or out.numel() != B * H * W or not out.is_contiguous():
        raise RuntimeError("logits_to_classes_u8: output must be a contiguous uint8 [B,H,W]")
    LIB.call("uh_logits_to_classes_u8", v.data_ptr(), B * H * W, C, _dt(v), out.data_ptr(), _stream())
    return out


def classes_to_grey_u8(classes: torch.Tensor, lut: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = lut[classes] for a uint8 tensor and a 256-entry device table; `out=classes` recodes in place."""
    _require_gpu(classes, "classes")
    _require_gpu(lut, "lut")
    if classes.dtype != torch.uint8 or not classes.is_contiguous():
        raise RuntimeError("classes_to_grey_u8 takes a contiguous uint8 tensor")
    if lut.dtype != torch.uint8 or lut.numel() != 256 or not lut.is_contiguous():
        raise RuntimeError("classes_to_grey_u8: the table is a contiguous uint8 [256]")
    if out is None:
        out = torch.empty_like(classes)
    if out.dtype != torch.uint8 or out.shape != classes.shape or not out.is_contiguous():
        raise RuntimeError("classes_to_grey_u8: output must be a contiguous uint8 tensor of the input's shape")
    LIB.call("uh_classes_to_grey_u8", classes.data_ptr(), out.data_ptr(), lut.data_ptr(), classes.numel(), _stream())
    return out


# ----------------------------------------------------------------------------- test-time augmentation (csrc/tta.hip)
class TtaMerged(NamedTuple):
    classes: torch.Tensor                     # uint8 [B,H,W]
    sums: Optional[torch.Tensor]              # int32 [B,H,W,NC]: the integer sums of the quantised probabilities (< 2^28)
    probs: Optional[torch.Tensor]             # float32 [B,H,W,NC] = sums / (V * 2^24)


def tta_views(x: torch.Tensor, mode) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """The views of a batch of images [B,C,H,W] (fp32, read through its NHWC view) under a mode of utils/tta.py ->
    (views0 [K0*B,C,H,W], views1 [K1*B,C,W,H] or None), view-major, both channels-last: what the network takes.  The two are
    slices of one buffer, views1 right behind views0."""
    from .utils.tta import tta_counts, tta_mask
    mask = tta_mask(mode)
    _require_gpu(x, "images")
    if x.dim() != 4:
        raise RuntimeError(f"tta_views expects [B,C,H,W] images, got {tuple(x.shape)}")
    B, C, H, W = x.shape
    v = x.permute(0, 2, 3, 1)
    if v.dtype != torch.float32:
        v = v.float()
    if not v.is_contiguous():
        v = v.contiguous()
    k0, k1 = tta_counts(mask)
    per = B * H * W * C
    buf = torch.empty((k0 + k1) * per, dtype=torch.float32, device=x.device)
    views0 = buf[:k0 * per].view(k0 * B, H, W, C)
    views1 = buf[k0 * per:].view(k1 * B, W, H, C) if k1 else None
    LIB.call("uh_tta_views", v.data_ptr(), views0.data_ptr(), _p(views1), B, H, W, C, mask, _stream())
    return views0.permute(0, 3, 1, 2), None if views1 is None else views1.permute(0, 3, 1, 2)


def tta_joint_views(views0: torch.Tensor, views1: torch.Tensor) -> torch.Tensor:
    """The two results of tta_views for SQUARE images as the one batch [(K0+K1)*B,C,H,W] they are in memory."""
    if views0.shape[1:] != views1.shape[1:] or views0.shape[2] != views0.shape[3]:
        raise RuntimeError("tta_joint_views: the views have two shapes")
    n0, n1 = views0.shape[0], views1.shape[0]
    a = views0.permute(0, 2, 3, 1)
    if views1.data_ptr() != a.data_ptr() + a.numel() * a.element_size():
        raise RuntimeError("tta_joint_views takes the pair tta_views returned")
    return torch.as_strided(a, (n0 + n1,) + tuple(a.shape[1:]), a.stride(), a.storage_offset()).permute(0, 3, 1, 2)


def tta_merge(logits0: torch.Tensor, logits1: Optional[torch.Tensor], mode, size: Tuple[int, int], *, sums: bool = False,
              probs: bool = False) -> TtaMerged:
    """Merges the logits of the views of tta_views back onto the source grid `size` = (H, W): logits0 [K0*B,NC,H,W], logits1
    [K1*B,NC,W,H] (fp32 or bf16, read through their NHWC view).  logits1 = None with a mode that has transposed views: the
    images are square and logits0 holds all (K0+K1)*B views.  -> TtaMerged(classes, sums or None, probs or None)."""
    from .utils.tta import tta_counts, tta_mask
    mask = tta_mask(mode)
    k0, k1 = tta_counts(mask)
    H, W = int(size[0]), int(size[1])
    _require_gpu(logits0, "logits")
    if logits0.dim() != 4 or tuple(logits0.shape[2:]) != (H, W) or logits0.shape[1] > 256:
        raise RuntimeError(f"tta_merge expects [N,C<=256,{H},{W}] logits of the untransposed views, got {tuple(logits0.shape)}")
    NC = logits0.shape[1]

    def nhwc(t):
        v = t.permute(0, 2, 3, 1)
        if v.dtype not in (torch.float32, torch.bfloat16):
            v = v.float()
        return v if v.is_contiguous() else v.contiguous()

    v0 = nhwc(logits0)
    v1 = None
    if k1 and logits1 is None:
        if H != W or v0.shape[0] % (k0 + k1):
            raise RuntimeError(f"tta_merge: {tuple(logits0.shape)} cannot hold every view of square images in this mode")
        B = v0.shape[0] // (k0 + k1)
        v0, v1 = v0[:k0 * B], v0[k0 * B:]
    else:
        if v0.shape[0] % k0:
            raise RuntimeError(f"tta_merge: {v0.shape[0]} untransposed views do not divide by {k0}")
        B = v0.shape[0] // k0
        if k1:
            _require_gpu(logits1, "logits")
            if tuple(logits1.shape) != (k1 * B, NC, W, H) or logits1.dtype != logits0.dtype:
                raise RuntimeError(f"tta_merge expects [{k1 * B},{NC},{W},{H}] logits of the transposed views in "
                                   f"{logits0.dtype}, got {tuple(logits1.shape)} {logits1.dtype}")
            v1 = nhwc(logits1)
    dev = v0.device
    classes = torch.empty(B, H, W, dtype=torch.uint8, device=dev)
    s = torch.empty(B, H, W, NC, dtype=torch.int32, device=dev) if sums else None
    p = torch.empty(B, H, W, NC, dtype=torch.float32, device=dev) if probs else None
    LIB.call("uh_tta_merge", v0.data_ptr(), _p(v1), _dt(v0), B, H, W, NC, mask, _p(s), classes.data_ptr(), _p(p), _stream())
    return TtaMerged(classes, s, p)


# ----------------------------------------------------------------------------- tiled prediction (csrc/tiling.hip)
UH_TILE_SUMS_I32 = 3                          # include/unet_hip.h: the int32 sums of uh_tta_merge as the source of uh_tile_merge


class TileMerged(NamedTuple):
    classes: torch.Tensor                     # uint8 [B,H,W]
    sums: Optional[torch.Tensor]              # int64 [B,H,W,NC]: the weighted integer sums (< 2^49; uint64 in the library)
    den: Optional[torch.Tensor]               # int32 [B,H,W]: the sum of the covering tiles' weights (< 2^22; uint32 in the library)
    probs: Optional[torch.Tensor]             # float32 [B,H,W,NC] = sums / (den * views * 2^24)


def tile_gather(x: torch.Tensor, cfg) -> torch.Tensor:
    """The tiles of a batch of images [B,C,H,W] (fp32, read through its NHWC view) under a TileConfig / spec of utils/tiling.py
    -> [B*ny*nx,C,th,tw], image-major then row-major over the grid, channels-last: what the network takes.  A pure copy."""
    from .utils.tiling import tile_config, tile_grid
    cfg = tile_config(cfg)
    if cfg is None:
        raise ValueError("tile_gather needs a tile config")
    _require_gpu(x, "images")
    if x.dim() != 4:
        raise RuntimeError(f"tile_gather expects [B,C,H,W] images, got {tuple(x.shape)}")
    B, C, H, W = x.shape
    v = x.permute(0, 2, 3, 1)
    if v.dtype != torch.float32:
        v = v.float()
    if not v.is_contiguous():
        v = v.contiguous()
    ny, nx, th, tw, _, _ = tile_grid(H, W, cfg)
    tiles = torch.empty(B * ny * nx, th, tw, C, dtype=torch.float32, device=x.device)
    LIB.call("uh_tile_gather", v.data_ptr(), tiles.data_ptr(), B, H, W, C, cfg.size, cfg.overlap, _stream())
    return tiles.permute(0, 3, 1, 2)


def tile_merge(src: torch.Tensor, cfg, size: Tuple[int, int], views: int = 1, *, sums: bool = False, probs: bool = False) -> TileMerged:
    """Merges the results of the tiles of tile_gather back onto the image grid `size` = (H, W).  src: the tiles' logits
    [B*ny*nx,NC,th,tw] (fp32 or bf16, read through their NHWC view; views = 1), or the int32 sums of tta_merge(sums=True) for
    every tile, [B*ny*nx,th,tw,NC] as TtaMerged.sums holds them, with `views` the number of views they add up.
    -> TileMerged(classes, sums or None, den or None, probs or None); den comes with sums."""
    from .utils.tiling import tile_config, tile_grid
    cfg = tile_config(cfg)
    if cfg is None:
        raise ValueError("tile_merge needs a tile config")
    H, W = int(size[0]), int(size[1])
    ny, nx, th, tw, _, _ = tile_grid(H, W, cfg)
    if views not in (1, 2, 4, 8):
        raise ValueError(f"tile_merge: views is 1, 2, 4 or 8, got {views!r}")
    _require_gpu(src, "tile results")
    if src.dim() != 4:
        raise RuntimeError(f"tile_merge expects 4-d tile results, got {tuple(src.shape)}")
    if src.dtype == torch.int32:
        if tuple(src.shape[1:3]) != (th, tw) or src.shape[3] > 256:
            raise RuntimeError(f"tile_merge expects [N,{th},{tw},NC<=256] int32 sums, got {tuple(src.shape)}")
        v, kind = src, UH_TILE_SUMS_I32
    else:
        if views != 1:
            raise ValueError("tile_merge: logits are one view (views = 1); pass the sums of tta_merge for more")
        if tuple(src.shape[2:]) != (th, tw) or src.shape[1] > 256:
            raise RuntimeError(f"tile_merge expects [N,C<=256,{th},{tw}] logits, got {tuple(src.shape)}")
        v = src.permute(0, 2, 3, 1)
        if v.dtype not in (torch.float32, torch.bfloat16):
            v = v.float()
        kind = _dt(v)
    if not v.is_contiguous():
        v = v.contiguous()
    N, NC = v.shape[0], v.shape[3]
    if N == 0 or N % (ny * nx):
        raise RuntimeError(f"tile_merge: {N} tiles are not whole {H} x {W} images of {ny} x {nx} tiles")
    B = N // (ny * nx)
    dev = v.device
    classes = torch.empty(B, H, W, dtype=torch.uint8, device=dev)
    s = torch.empty(B, H, W, NC, dtype=torch.int64, device=dev) if sums else None
    d = torch.empty(B, H, W, dtype=torch.int32, device=dev) if sums else None
    p = torch.empty(B, H, W, NC, dtype=torch.float32, device=dev) if probs else None
    LIB.call("uh_tile_merge", v.data_ptr(), kind, int(views), B, H, W, NC, cfg.size, cfg.overlap, _p(s), _p(d), classes.data_ptr(),
             _p(p), _stream())
    return TileMerged(classes, s, d, p)


# ----------------------------------------------------------------------------- checkpoint ensembles (csrc/ensemble.hip)
UH_ENS_SUMS_U64 = 4                           # include/unet_hip.h: the uint64 sums of uh_tile_merge as the source of uh_ensemble_add


class EnsembleMerged(NamedTuple):
    classes: torch.Tensor                     # uint8 [B,H,W]
    probs: Optional[torch.Tensor]             # float32 [B,H,W,NC] = acc / (den * views * 2^24 * total_weight)
    confidence: Optional[torch.Tensor]        # uint8 [B,H,W] = floor(255 * max_c acc / sum_c acc)


def ensemble_add(src: torch.Tensor, weight: int = 1, acc: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Adds one member's result, `weight` times, into the accumulator int64 [B,H,W,NC] (uint64 in the library) and returns it;
    acc = None: a new accumulator that the member is assigned to (no memset).  src: the member's logits [B,NC,H,W] (fp32 or
    bf16, read through their NHWC view and quantised as tta_merge / tile_merge quantise), the int32 sums [B,H,W,NC] of
    tta_merge(sums=True), or the int64 sums [B,H,W,NC] of tile_merge(sums=True)."""
    _require_gpu(src, "member results")
    if isinstance(weight, bool) or not isinstance(weight, int) or not 1 <= weight <= 1024:
        raise ValueError(f"ensemble_add: weight is an integer in 1..1024, got {weight!r}")
    if src.dim() != 4:
        raise RuntimeError(f"ensemble_add expects 4-d member results, got {tuple(src.shape)}")
    if src.dtype in (torch.int32, torch.int64):
        v, kind = src, UH_TILE_SUMS_I32 if src.dtype == torch.int32 else UH_ENS_SUMS_U64
    else:
        v = src.permute(0, 2, 3, 1)
        if v.dtype not in (torch.float32, torch.bfloat16):
            v = v.float()
        kind = _dt(v)
    if not v.is_contiguous():
        v = v.contiguous()
    B, H, W, NC = v.shape
    if NC > 256 or v.numel() == 0:
        raise RuntimeError(f"ensemble_add expects 1..256 classes and at least one pixel, got {tuple(src.shape)}")
    first = acc is None
    if first:
        acc = torch.empty(B, H, W, NC, dtype=torch.int64, device=v.device)
    elif acc.dtype != torch.int64 or tuple(acc.shape) != (B, H, W, NC) or not acc.is_contiguous() or acc.device != v.device:
        raise RuntimeError(f"ensemble_add: the accumulator must be a contiguous int64 [{B},{H},{W},{NC}] on the member's device")
    LIB.call("uh_ensemble_add", v.data_ptr(), kind, B * H * W, NC, weight, 1 if first else 0, acc.data_ptr(), _stream())
    return acc


def ensemble_finish(acc: torch.Tensor, total_weight: int, *, views: int = 1, den: Optional[torch.Tensor] = None, probs: bool = False,
                    confidence: bool = False) -> EnsembleMerged:
    """The accumulator of ensemble_add over members of `total_weight` in all -> EnsembleMerged(classes, probs or None, confidence
    or None).  views: the views every member's sums add up (1, 2, 4 or 8); den: the int32 [B,H,W] weights of tile_merge (the
    same for every member), None for untiled members."""
    _require_gpu(acc, "accumulator")
    if views not in (1, 2, 4, 8):
        raise ValueError(f"ensemble_finish: views is 1, 2, 4 or 8, got {views!r}")
    if isinstance(total_weight, bool) or not isinstance(total_weight, int) or not 1 <= total_weight <= 1024:
        raise ValueError(f"ensemble_finish: total_weight is an integer in 1..1024, got {total_weight!r}")
    if acc.dtype != torch.int64 or acc.dim() != 4 or not acc.is_contiguous() or acc.shape[3] > 256 or acc.numel() == 0:
        raise RuntimeError(f"ensemble_finish expects a contiguous int64 [B,H,W,NC<=256] accumulator, got {acc.dtype} {tuple(acc.shape)}")
    B, H, W, NC = acc.shape
    if den is not None:
        _require_gpu(den, "den")
        if den.dtype != torch.int32 or tuple(den.shape) != (B, H, W) or not den.is_contiguous():
            raise RuntimeError(f"ensemble_finish: den must be a contiguous int32 [{B},{H},{W}]")
    dev = acc.device
    classes = torch.empty(B, H, W, dtype=torch.uint8, device=dev)
    p = torch.empty(B, H, W, NC, dtype=torch.float32, device=dev) if probs else None
    c = torch.empty(B, H, W, dtype=torch.uint8, device=dev) if confidence else None
    LIB.call("uh_ensemble_finish", acc.data_ptr(), _p(den), int(views), total_weight, B * H * W, NC, classes.data_ptr(), _p(p), _p(c),
             _stream())
    return EnsembleMerged(classes, p, c)


# ----------------------------------------------------------------------------- patch training (csrc/crop.hip)
def crop_select(labels: Sequence[torch.Tensor], words, size: int, class_mask: int, threshold: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The crop origins of utils/crop.py for int64 label planes [H,W] of any sizes: words uint32 [B,4] (r0..r3 per plane),
    class_mask bit v set for every label value v that counts, threshold = rint(fg 2^32).
    -> (origins int32 [B,2] = (oy, ox), counts int32 [B] = the counted pixels), both on the device."""
    from .utils.crop import item_table
    labels = list(labels)
    if not labels:
        raise ValueError("crop_select needs at least one label plane")
    for m in labels:
        _require_gpu(m, "labels")
    if not 0 <= int(class_mask) < 1 << 64 or not 0 <= int(threshold) <= 1 << 32:
        raise ValueError(f"crop_select: class_mask is a 64-bit mask and threshold lies in [0, 2^32], got {class_mask!r}, {threshold!r}")
    table, keep = item_table(None, labels, words)
    B, dev = len(labels), labels[0].device
    with torch.cuda.device(dev):
        origins = torch.empty(B, 2, dtype=torch.int32, device=dev)
        counts = torch.empty(B, dtype=torch.int32, device=dev)
        ws_bytes = LIB.query("uh_crop_select_ws_bytes", B)
        ws = torch.empty(ws_bytes // 4, dtype=torch.int32, device=dev)
        LIB.call("uh_crop_select", table.ctypes.data, B, int(size), int(class_mask), int(threshold), origins.data_ptr(),
                 counts.data_ptr(), ws.data_ptr(), ws_bytes, _stream())
    del keep
    return origins, counts


def crop_gather(images: Optional[Sequence[torch.Tensor]], labels: Optional[Sequence[torch.Tensor]], origins: torch.Tensor,
                size: int, ld_out: Optional[int] = None) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
    """[oy, oy + size) x [ox, ox + size) of every item: images [C,H,W] (fp32 or bf16, one dtype and C, read through their NHWC
    views; a pixel stride above C is taken as it is) and / or int64 labels [H,W], origins int32 [B,2] on the device (clamped
    into the item as they are loaded).  -> (image [B,C,size,size], channels_last memory with pixel stride ld_out (default C),
    or None; labels int64 [B,size,size] or None).  A pure copy."""
    from .utils.crop import item_table
    images = list(images) if images is not None else None
    labels = list(labels) if labels is not None else None
    ref = images if images is not None else labels
    if not ref or (images is not None and labels is not None and len(images) != len(labels)):
        raise ValueError("crop_gather needs images and / or labels, one of each per item")
    for t in (images or []) + (labels or []) + [origins]:
        _require_gpu(t, "crop source")
    B, dev = len(ref), ref[0].device
    if origins.dtype != torch.int32 or tuple(origins.shape) != (B, 2) or not origins.is_contiguous():
        raise RuntimeError(f"crop_gather expects contiguous int32 [{B},2] origins, got {origins.dtype} {tuple(origins.shape)}")
    C, dt, out, lab = 1, UH_F32, None, None
    if images is not None:
        C = images[0].shape[0]
        if any(x.dtype != images[0].dtype or x.shape[0] != C for x in images):
            raise RuntimeError("crop_gather: the images of a batch have one dtype and one channel count")
        dt = _dt(images[0])
    table, keep = item_table(images, labels)
    size = int(size)
    ld_out = C if ld_out is None else int(ld_out)
    with torch.cuda.device(dev):
        if images is not None:
            out = (torch.empty if ld_out == C else torch.zeros)((B, size, size, max(ld_out, 1)), dtype=images[0].dtype, device=dev)
        if labels is not None:
            lab = torch.empty((B, size, size), dtype=torch.int64, device=dev)
        LIB.call("uh_crop_gather", table.ctypes.data, B, C, dt, size, origins.data_ptr(), _p(out), ld_out, _p(lab), _stream())
    del keep
    return (out[..., :C].permute(0, 3, 1, 2) if out is not None else None), lab


# ----------------------------------------------------------------------------- dataset cache (csrc/cache.hip)
def cache_gather(rows, image_bytes: int, mask_bytes: int, want_image: bool = True,
                 want_mask: bool = True) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
    """One batch cut from cached entries: rows = one (image, mask) pair per batch item, contiguous uint8 device tensors whose
    storage starts 16-byte aligned and is readable up to the length rounded up to 16 (utils/dataset_cache.py pads its arena so);
    rows may repeat.  -> (uint8 [B, image_bytes] or None, uint8 [B, mask_bytes] or None): the first image_bytes / mask_bytes bytes
    of every row's tensors, in one launch per 32 rows.  A side that is not wanted may be None in the rows.  A pure copy."""
    rows = list(rows)
    if not rows:
        raise ValueError("cache_gather needs at least one row")
    if not (want_image or want_mask):
        raise ValueError("cache_gather: want_image and want_mask are both False")
    image_bytes, mask_bytes = int(image_bytes), int(mask_bytes)
    table = np.zeros((len(rows), 2), dtype=np.uint64)                    # include/unet_hip.h: uh_cache_item (16 bytes)
    dev = None
    for b, row in enumerate(rows):
        if len(row) != 2:
            raise ValueError(f"cache_gather: rows[{b}] is not an (image, mask) pair")
        for col, (t, want, need, what) in enumerate(zip(row, (want_image, want_mask), (image_bytes, mask_bytes), ("image", "mask"))):
            if not want:
                continue
            if t is None:
                raise RuntimeError(f"cache_gather: rows[{b}] has no {what}")
            _require_gpu(t, f"rows[{b}] {what}")
            if t.dtype != torch.uint8 or not t.is_contiguous():
                raise RuntimeError(f"cache_gather: rows[{b}] {what} must be a contiguous uint8 tensor, got {t.dtype} {tuple(t.shape)}")
            if need < 1 or t.numel() < need:
                raise RuntimeError(f"cache_gather: {what}_bytes={need} does not fit rows[{b}] {what} of {t.numel()} bytes")
            if dev is None:
                dev = t.device
            elif t.device != dev:
                raise RuntimeError(f"cache_gather: rows[{b}] {what} is on {t.device}, the first row on {dev}")
            table[b, col] = t.data_ptr()
    B = len(rows)
    with torch.cuda.device(dev):
        image = torch.empty((B, image_bytes), dtype=torch.uint8, device=dev) if want_image else None
        mask = torch.empty((B, mask_bytes), dtype=torch.uint8, device=dev) if want_mask else None
        LIB.call("uh_cache_gather_u8", table.ctypes.data, B, image_bytes, mask_bytes, _p(image), _p(mask), _stream())
    return image, mask


# ----------------------------------------------------------------------------- contour metrics (csrc/contour_metrics.hip)
CONTOUR_RECORD_DOUBLES = 12         # uh_contour_record: 12 x uint32 (= 6 doubles wide), then 6 x double
_EDT_WS = {}
_CONTOUR_WS = {}


def _u8_batch(t: torch.Tensor, what: str) -> Tuple[int, int, int]:
    _require_gpu(t, what)
    if t.dtype != torch.uint8 or t.dim() != 3 or not t.is_contiguous():
        raise RuntimeError(f"{what} must be a contiguous uint8 [B,H,W] tensor, got {t.dtype} {tuple(t.shape)}")
    return tuple(t.shape)


def _cached_ws(cache: dict, query: str, B: int, H: int, W: int, device) -> torch.Tensor:
    key = (B, H, W, device)
    ws = cache.get(key)
    if ws is None:
        ws = cache[key] = torch.empty(max(LIB.query(query, B, H, W), 256), dtype=torch.uint8, device=device)
    return ws


def mask_border(mask_u8: torch.Tensor, cls: int) -> torch.Tensor:
    """uint8 [B,H,W]: 1 on the pixels of (mask == cls) that have one of their four edge neighbours outside it (outside the
    image counts as outside), 0 elsewhere."""
    B, H, W = _u8_batch(mask_u8, "mask")
    out = torch.empty_like(mask_u8)
    LIB.call("uh_mask_border_u8", mask_u8.data_ptr(), int(cls), out.data_ptr(), B, H, W, _stream())
    return out


def edt_sq(feature_u8: torch.Tensor) -> torch.Tensor:
    """Exact squared Euclidean distance of every pixel to the nearest non-zero pixel of its image: uint8 [B,H,W] ->
    int64 [B,H,W] (4294967295 everywhere in an image without a non-zero pixel)."""
    B, H, W = _u8_batch(feature_u8, "feature")
    ws = _cached_ws(_EDT_WS, "uh_edt_sq_ws_bytes", B, H, W, feature_u8.device)
    out = torch.empty(B, H, W, dtype=torch.int32, device=feature_u8.device)
    LIB.call("uh_edt_sq_u8", feature_u8.data_ptr(), out.data_ptr(), B, H, W, ws.data_ptr(), ws.numel(), _stream())
    return out.to(torch.int64) & 0xFFFFFFFF                         # torch has no arithmetic on uint32


def contour_metrics(pred_u8: torch.Tensor, true_u8: torch.Tensor, cls_pred: int, cls_true: int) -> torch.Tensor:
    """HD / HD95 / ASSD / IoU of (pred == cls_pred) against (true == cls_true) per image: the uh_contour_record table as a
    float64 [B,12] tensor.  Columns 6..11 are weight, sum_dist, hd, hd95, assd, iou; `.view(torch.int32)[:, :12]` are the
    integer fields (include/unet_hip.h).  Nothing is read back to the host."""
    B, H, W = _u8_batch(pred_u8, "pred")
    if _u8_batch(true_u8, "true") != (B, H, W) or true_u8.device != pred_u8.device:
        raise RuntimeError(f"contour_metrics: pred {tuple(pred_u8.shape)} and true {tuple(true_u8.shape)} differ")
    ws = _cached_ws(_CONTOUR_WS, "uh_contour_metrics_ws_bytes", B, H, W, pred_u8.device)
    rec = torch.empty(B, CONTOUR_RECORD_DOUBLES, dtype=torch.float64, device=pred_u8.device)
    LIB.call("uh_contour_metrics", pred_u8.data_ptr(), true_u8.data_ptr(), int(cls_pred), int(cls_true), rec.data_ptr(), B, H, W,
             ws.data_ptr(), ws.numel(), _stream())
    return rec


# ----------------------------------------------------------------------------- losses (losses.py)
# The loss nodes live in losses.py and the package names them there.  The loss tests as they stood before the move say
# ops.<name> and have to keep passing as they are, so those names still resolve: looked up in losses.py on demand (nothing of
# it is imported here at import time).  Functions and classes only; the FUSE_LOSS switch, which callers assign, is
# losses.FUSE_LOSS alone: a forwarded copy would take the assignment and change nothing.
_MOVED_TO_LOSSES = ("loss_workspace", "boundary_loss_value", "boundary_loss_mask_value", "SegLossBinaryFn", "SegLossMulticlassFn",
                    "DiceCoeffFn", "surface_classes", "surface_border", "surface_dist_map", "SurfaceLossFn", "focal_head",
                    "FocalTverskyLossFn", "DistillLossFn")


def __getattr__(name):
    if name in _MOVED_TO_LOSSES:
        from . import losses
        return getattr(losses, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
