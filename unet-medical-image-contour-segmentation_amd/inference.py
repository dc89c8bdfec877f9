"""Low-latency inference: the eval-mode forward (predict.py:15-29 / evaluate.py:43-54) captured once into a HIP graph and
replayed.  At batch 1 the ~60 kernels of a forward take less GPU time than their launches take on the host; the graph
removes the host from the loop.  Fixed input shape/dtype per instance (like any graph capture)."""
from __future__ import annotations

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
