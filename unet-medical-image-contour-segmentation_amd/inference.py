"""Low-latency inference: the eval-mode forward (predict.py:15-29 / evaluate.py:43-54) captured once into a HIP graph and
replayed.  At batch 1 the ~60 kernels of a forward take less GPU time than their launches take on the host; the graph
removes the host from the loop.  Fixed input shape/dtype per instance (like any graph capture).

`forward_step` and `finish_group` are the one statement of how a prediction is composed of test-time augmentation views, tiles
and ensemble members (the table in DESIGN.md section 3); BatchPredictor and evaluate() both walk it, each with its own forward."""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

from . import ops


def eval_forward(model: torch.nn.Module, x: torch.Tensor, amp: bool, plan_images: int = 0) -> torch.Tensor:
    """`model(x)` without autograd, under bf16 autocast when `amp`, and under ops.plan_images(plan_images) when that is > 0
    (0 leaves a plan that is already active in force)."""
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
        if plan_images:
            with ops.plan_images(plan_images):
                return model(x)
        return model(x)


def timed_stage(events, name, fn, *a, **kw):
    """`fn(*a, **kw)`; when `events` is a list, (name, start event, end event) on the current stream is appended to it."""
    if events is None:
        return fn(*a, **kw)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn(*a, **kw)
    e1.record()
    events.append((name, e0, e1))
    return r


# ------------------------------------------------------------------------------------------ views, tiles, members
class Prediction(NamedTuple):
    classes: torch.Tensor                     # uint8 [B,H,W]
    probs: Optional[torch.Tensor]             # float32 [B,H,W,NC], where asked for
    confidence: Optional[torch.Tensor]        # uint8 [B,H,W], where asked for (ensembles)


def view_count(tta) -> int:
    """The views that the sums of a prediction under the mask `tta` add up per image (None: 1)."""
    if tta is None:
        return 1
    from .utils.tta import tta_counts
    return sum(tta_counts(tta))


def _unmarked(name, fn, *a, **kw):
    return fn(*a, **kw)


def forward_step(x: torch.Tensor, forwards, tta, last: bool = False, probs: bool = False, mark=_unmarked):
    """One forward step on a prepared batch or a chunk of tiles [n,C,h,w]: yields one result per member, in order.
    `forwards`: per member a callable (inputs [k,C,h',w'], (h', w')) -> logits [k,NC,h',w'] that outlive the member's next call.
    `tta`: the mask of utils/tta.py or None.  The views are built once for all members; a member's forward runs on `x`, on the
    joint views of a square shape or on the two view batches, and ops.tta_merge follows where there are views.
    `last`: nothing merges after this step (one member, untiled), so the result under `tta` is the TtaMerged record with the
    classes (and `probs`); otherwise it is the int32 view sums.  Without `tta` it is the logits either way.
    A generator: a member's launches are made when its result is asked for, so a caller that consumes each result before it
    takes the next (finish_group's ensemble_add) launches member by member."""
    h, w = int(x.shape[-2]), int(x.shape[-1])

    def forward(f, v, size):
        out = mark("forward", f, v, size)
        if tuple(out.shape[-2:]) != size:                              # predict.py:26 is dead at scale 1
            raise RuntimeError(f"the network returned {tuple(out.shape[-2:])} for a {size} input")
        return out

    if tta is None:
        for f in forwards:
            yield forward(f, x, (h, w))
        return
    v0, v1 = mark("views", ops.tta_views, x, tta)
    for f in forwards:
        if v1 is not None and h == w:                                  # one view shape: one forward
            l0, l1 = forward(f, ops.tta_joint_views(v0, v1), (h, w)), None
        else:
            l0 = forward(f, v0, (h, w))
            l1 = forward(f, v1, (w, h)) if v1 is not None else None
        merged = mark("merge", ops.tta_merge, l0, l1, tta, (h, w), sums=not last, probs=last and probs)
        yield merged if last else merged.sums


def finish_group(results, weights, tile, size, tta, probs: bool = False, confidence: bool = False, mark=_unmarked) -> Prediction:
    """The members' results for a group of equally sized images -> Prediction.  `results`: what forward_step yielded per member
    (for tiled images: for every tile of the group, steps concatenated), taken one at a time.  `weights`: the members' integer
    weights, None for one model.  `tile`: the TileConfig, None for whole images; `size`: (H, W) of the images.
    Tiled results go through ops.tile_merge; with `weights` every member's logits, view sums or tile sums go through
    ops.ensemble_add and one ops.ensemble_finish follows.  The last of these writes `classes` / `probs` / `confidence`; one model's
    untiled result under `tta` already holds them, its plain logits -- also those of an image that is one tile -- go through
    ops.logits_to_classes_u8."""
    if weights is None and tile is None:                               # nothing merges here
        (src,) = results
        if tta is not None:
            return Prediction(src.classes, src.probs, None)
        return Prediction(mark("classes", ops.logits_to_classes_u8, src), None, None)
    views = view_count(tta)

    def tile_merge(src, **kw):
        return mark("tile_merge", ops.tile_merge, src, tile, size, views, **kw)

    if weights is not None:
        acc = den = None
        for src, weight in zip(results, weights):
            if tile is not None:
                merged = tile_merge(src, sums=True)
                src, den = merged.sums, merged.den                     # (the tiles' weights `den` are the same for all members)
            acc = mark("ensemble_add", ops.ensemble_add, src, weight, acc)
        return Prediction(*mark("ensemble_finish", ops.ensemble_finish, acc, sum(weights), views=views, den=den, probs=probs,
                                confidence=confidence))
    (src,) = results
    if probs:
        merged = tile_merge(src, probs=True)
        return Prediction(merged.classes, merged.probs, None)
    from .utils.tiling import tile_count
    if tta is None and tile_count(size[0], size[1], tile) == 1:
        return Prediction(mark("classes", ops.logits_to_classes_u8, src), None, None)   # the tile is the image: as untiled
    return Prediction(tile_merge(src).classes, None, None)


class GraphedForward:
    """`g = GraphedForward(model, example_images); logits = g(images)` -- same result as `model.eval()(images)`.
    The returned tensor is the graph's static output buffer: copy it if it must survive the next call.
    `plan_images` > 0: warm-up and capture run under ops.plan_images(plan_images) -- the kernel choice is made on the host
    while the graph is captured, so the replays keep it (1: every image is computed bit for bit as it is alone).  Outside
    an instance built with it, an ops.plan_images block that is active at construction time is captured just the same."""

    def __init__(self, model: torch.nn.Module, example: torch.Tensor, amp: bool = True, warmup: int = 3, plan_images: int = 0):
        if not example.is_cuda:
            raise RuntimeError("GraphedForward needs GPU tensors (no CPU fallback exists)")
        self.model = model.eval()
        self.amp = amp
        self.plan_images = int(plan_images)
        self.static_in = example.detach().clone(memory_format=torch.preserve_format)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                      # warm-up off the default stream: filter packs, allocator pools
            for _ in range(max(1, warmup)):
                eval_forward(self.model, self.static_in, self.amp, self.plan_images)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.static_out = eval_forward(self.model, self.static_in, self.amp, self.plan_images)

    def __call__(self, images: torch.Tensor) -> torch.Tensor:
        if images.shape != self.static_in.shape:
            raise RuntimeError(f"captured for input shape {tuple(self.static_in.shape)}, got {tuple(images.shape)}")
        self.static_in.copy_(images)
        self.graph.replay()
        return self.static_out
