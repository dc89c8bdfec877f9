"""Inference of /root/reference/predict.py on the HIP path.

    predict_img(model, full_img, device) -> np.ndarray[H, W] of class indices        predict.py:15-29
    mask_to_image(mask) -> PIL.Image (0 / 128 / 255 grey levels)                      predict.py:52-58
    preprocess_image(pil_img, scale=1.0) -> float32 [C, H, W]                         data_loading.py:65-91 (image branch)
    BatchPredictor(model, batch=8, postprocess=True, batch_invariant=False, tta=None, tile=None)(images) -> [uint8 [H, W] grey]
                                                                                      predict.py:120-135 for a list of images
    python -m unet_amd.predict -m model.pth -i DIR [-o OUT]                           predict.py:31-152 (predict_cli.py)

predict_img is the reference's one-image call: the forward runs the eval-mode kernels (BatchNorm running statistics folded
into per-channel scale/shift), argmax is `uh_argmax_classes`.  BatchPredictor is the same computation for a list of images
of mixed sizes: grouped by size, batched, with the byte stages of csrc/predict_io.hip around the forward (`uh_predict_prepare_u8`,
`uh_logits_to_classes_u8`, `uh_classes_to_grey_u8`), `uh_postprocess_masks` between them and one upload and one download per
batch.  Its result for an image is, pixel for pixel, mask_to_image(postprocess_mask(predict_img(model, image, device))).
"""
from __future__ import annotations

from collections import OrderedDict, deque
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from . import ops
from .inference import GraphedForward, eval_forward, finish_group, forward_step, timed_stage


def _table(pairs) -> np.ndarray:
    t = np.zeros(256, np.uint8)                  # np.zeros_like(mask): a code the reference does not name stays 0
    for k, v in pairs:
        t[k] = v
    return t


GREY_CLASSES = _table([(0, 0), (1, 128), (2, 255)])        # predict.py:52-58, evaluate.py:150-154
GREY_POSTPROCESSED = _table([(0, 0), (2, 255)])            # evaluate.py:160-163: the post-processed multi-class map, 1 -> 0
GREY_BINARY = _table([(0, 0), (1, 255)])                   # evaluate.py:96-97 (pred * 255) and :103-105


def preprocess_image(pil_img, scale: float = 1.0) -> np.ndarray:
    """Image branch of BasicDataset.preprocess (data_loading.py:65-91); ndarrays are taken as already-decoded images."""
    from .utils.data_loading import BasicDataset
    if isinstance(pil_img, np.ndarray):
        if scale != 1.0:
            raise ValueError("scale != 1 needs a PIL image")
        img = pil_img[np.newaxis, ...] if pil_img.ndim == 2 else pil_img.transpose((2, 0, 1))
        return img.astype(np.float32) / 255.0 if (img > 1).any() else img
    return BasicDataset.preprocess(None, pil_img, scale, is_mask=False)


def predict_img(model, full_img, device):
    model.eval()
    img = torch.from_numpy(np.ascontiguousarray(preprocess_image(full_img, 1.0)))
    img = img.unsqueeze(0).to(device=device, dtype=torch.float32, memory_format=torch.channels_last)
    if hasattr(full_img, "size") and not isinstance(full_img, np.ndarray):
        out_hw = (full_img.size[1], full_img.size[0])
    else:
        out_hw = tuple(np.asarray(full_img).shape[:2])
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=True):
        mask_pred = model(img)
        if tuple(mask_pred.shape[-2:]) != tuple(out_hw):
            # predict.py:26; never taken with scale=1 (the UNet output has the input's size, unet_parts.py:85-88)
            mask_pred = F.interpolate(mask_pred.float(), out_hw, mode="bilinear")
        idx = ops.argmax_classes(mask_pred).squeeze(0)
    return idx.cpu().numpy()


def mask_to_image(mask: np.ndarray):
    from PIL import Image
    vis = np.zeros_like(mask, dtype=np.uint8)
    vis[mask == 1] = 128
    vis[mask == 2] = 255
    return Image.fromarray(vis)


# ------------------------------------------------------------------------------------------ batches of one size
class BatchPlanner:
    """Groups a stream of (index, (H, W)) into batches of one size.  `add` returns the batches that became full; `flush`
    the partial ones, in order of their oldest member.  No item is held back for more than `window` later indices: once
    the stream has moved that far past the oldest waiting item, its group is released partial, so that a rare size at the
    start of a folder does not keep every later result waiting in memory (results are written in index order)."""

    def __init__(self, batch: int, window: Optional[int] = None):
        if batch < 1:
            raise ValueError("batch must be >= 1")
        self.batch = int(batch)
        self.window = max(int(window), self.batch) if window is not None else None
        self._groups: "OrderedDict[Tuple[int, int], List[int]]" = OrderedDict()

    def add(self, index: int, size: Tuple[int, int]) -> List[Tuple[Tuple[int, int], List[int]]]:
        size = (int(size[0]), int(size[1]))
        g = self._groups.setdefault(size, [])
        g.append(index)
        out = []
        if len(g) == self.batch:
            out.append((size, self._groups.pop(size)))
        while self.window is not None and self._groups:
            oldest = min(self._groups, key=lambda k: self._groups[k][0])
            if index - self._groups[oldest][0] < self.window:
                break
            out.append((oldest, self._groups.pop(oldest)))
        return out

    def flush(self) -> List[Tuple[Tuple[int, int], List[int]]]:
        out = sorted(self._groups.items(), key=lambda kv: kv[1][0])
        self._groups = OrderedDict()
        return out


def plan_batches(sizes: Sequence[Tuple[int, int]], batch: int, window: Optional[int] = None):
    """[( (H, W), [indices] )] covering every index of `sizes` once, each batch of one size and at most `batch` long."""
    planner = BatchPlanner(batch, window)
    out = []
    for i, s in enumerate(sizes):
        out.extend(planner.add(i, s))
    out.extend(planner.flush())
    return out


def _as_grey_array(img) -> np.ndarray:
    a = img if isinstance(img, np.ndarray) else np.asarray(img)
    if a.dtype != np.uint8 or a.ndim != 2:
        raise ValueError(f"BatchPredictor takes decoded 8-bit grey images (PIL 'L' or uint8 [H,W]), got {a.dtype} {a.shape}")
    return a


class LaunchPlanner:
    """The launch arithmetic of BatchPredictor: which launch lengths an image size allows, how a batch is cut into them, and
    how many source images or tiles make a launch group.  It touches no tensor and no device; it only asks LIB.query.

    The result for an image does not depend on its neighbours or on `batch`: every kernel of the eval forward computes a
    pixel from that image's data in a fixed order.  WHICH kernel runs, however, is chosen per launch in two places, and
    the alternatives sum in different orders (logits differ by ~1e-4, a few argmax ties flip):
      - the transposed convolution takes its MFMA GEMM only when B*h*w of its input is a multiple of 32 pixels (bf16; 16 in
        fp32) and the SIMT kernel otherwise (uh_convt2x2_mfma_ok): 62 x 62 alone is not, eight of them are;
      - conv3x3_fwd_dispatch splits the contraction over the two halves of a workgroup when a layer with 256+ input channels
        has at most 256 (tile, 64-channel slab) pairs, and moves to 128-channel slabs from 512 (tile, slab) pairs: a
        700 x 300 image has 18 tiles at the level of up1 (256 -> 128 channels), so 7 images split K and 8 do not.
    `launch_lengths` asks the library for both choices (uh_convt2x2_mfma_ok, uh_conv3x3_fwd_kernel) and only forms
    launches in which every layer gets the kernel it gets for one image; a batch is cut into the fewest such launches,
    down to one image per launch where nothing longer qualifies.

    `batch_invariant=True` lifts the cutting: the forward runs under ops.plan_images(1), which pins every layer of a launch
    to the kernel one image gets (uh_conv3x3_fwd_affine_relu_plan, uh_convt2x2_mfma_ok_plan), so a launch of any length
    gives every image the bits it gets alone.  `launch_lengths` then asks the pinned queries and returns every B up to
    `batch` that no real-B limit (a tensor past the 2 GiB window: another kernel) excludes.  The masks are those of the
    default mode; only the number of launches differs."""

    def __init__(self, model: torch.nn.Module, batch: int, amp: bool, batch_invariant: bool = False, tta=None):
        self.model, self.batch, self.amp = model, int(batch), bool(amp)
        self.batch_invariant, self.tta = bool(batch_invariant), tta
        self.lengths: Dict[Tuple[int, int], List[int]] = {}           # (H, W) -> launch_lengths(H, W)

    def _layers(self):
        """(kind, module, pyramid levels it may sit at) for the layers whose kernel choice can depend on B."""
        depth = getattr(self.model, "depth", None)
        if depth is None:
            depth = sum(1 for n, _ in self.model.named_children() if n.startswith("down"))
        out = []
        for name, m in self.model.named_modules():
            is_t = isinstance(m, torch.nn.ConvTranspose2d)
            if not is_t and not (isinstance(m, torch.nn.Conv2d) and tuple(m.kernel_size) == (3, 3)):
                continue
            top = name.split(".")[0]
            if top == "inc":
                levels = [0]
            elif top.startswith("down") and top[4:].isdigit():
                levels = [int(top[4:])]
            elif top.startswith("up") and top[2:].isdigit():
                # block j works at level depth - j; its transposed convolution reads the level below
                levels = [depth - int(top[2:]) + (1 if is_t else 0)]
            else:
                levels = list(range(0, depth + 1))                 # unknown place: every level is checked
            out.append(("convt" if is_t else "conv", m, levels))
        return out

    def launch_lengths(self, H: int, W: int) -> List[int]:
        """The launch lengths B <= batch at which an H x W image is computed by the kernels it gets alone (1 always is)."""
        key = (int(H), int(W))
        if key not in self.lengths:
            from ._lib import LIB, UH_BF16, UH_F32
            dt = UH_BF16 if self.amp else UH_F32
            pin = 1 if self.batch_invariant else 0
            layers = self._layers()                                    # walked once per new size: the lengths are kept

            def choice(B, kind, m, k):
                h, w = H >> k, W >> k
                if h < 1 or w < 1:
                    return 0
                if kind == "convt":
                    if pin and B > 1:
                        return LIB.query("uh_convt2x2_mfma_ok_plan", B, pin, h, w, m.in_channels, m.out_channels, H >> (k - 1),
                                         W >> (k - 1), dt)
                    return LIB.query("uh_convt2x2_mfma_ok", B, h, w, m.in_channels, m.out_channels, H >> (k - 1), W >> (k - 1), dt)
                if pin and B > 1:
                    # the summation class of the kernel the pinned call runs: equal to one image's unless a real-B limit moved it
                    code = LIB.query("uh_conv3x3_fwd_kernel_plan", B, pin, h, w, m.in_channels, 0, m.out_channels, dt)
                    return LIB.query("uh_conv3x3_fwd_sum_class", code)
                code = LIB.query("uh_conv3x3_fwd_kernel", B, h, w, m.in_channels, 0, m.out_channels, dt)
                return LIB.query("uh_conv3x3_fwd_sum_class", code) if pin else code

            self.lengths[key] = [B for B in range(1, self.batch + 1)
                                 if all(choice(B, kind, m, k) == choice(1, kind, m, k)
                                        for kind, m, levels in layers for k in levels if k >= (1 if kind == "convt" else 0))]
        return self.lengths[key]

    def cut(self, n: int, H: int, W: int) -> List[int]:
        """`n` images of H x W as the fewest launches launch_lengths allows: each piece the longest that still fits."""
        lengths = self.launch_lengths(H, W)
        pieces = []
        while n:
            pieces.append(max(v for v in lengths if v <= n))
            n -= pieces[-1]
        return pieces

    def tta_group(self, H: int, W: int) -> int:
        """Source images of one size per launch group: `batch` is the number of images per forward launch, and a launch
        carries every view of a square image, the larger of the two view shapes' counts otherwise."""
        from .utils.tta import tta_forward_views
        return max(1, self.batch // tta_forward_views(self.tta, H, W))

    def tile_chunk(self, th: int, tw: int) -> int:
        """Tiles of one shape per forward step: `batch`, or under test-time augmentation what tta_group allows (it counts
        tiles here: `batch` stays the number of network inputs per forward launch)."""
        return self.batch if self.tta is None else self.tta_group(th, tw)


class _Member:
    """What a network of the predictor keeps to itself: the network, its weight in an ensemble (None: it runs alone), its
    launch arithmetic and its graph cache."""

    def __init__(self, model: torch.nn.Module, weight: Optional[int], batch: int, amp: bool, batch_invariant: bool, tta):
        self.model, self.weight = model, weight
        self.planner = LaunchPlanner(model, batch, amp, batch_invariant, tta)
        self._graphs: "OrderedDict[Tuple[int, int, int], object]" = OrderedDict()
        self._seen = set()


class BatchPredictor:
    """`predictor(images)` -> one uint8 [H,W] grey-coded mask per image, in input order: what
    mask_to_image(postprocess_mask(predict_img(model, image, device))) returns for that image (mask_to_image(predict_img(...))
    with postprocess=False).  `predictor.classes(images)` returns the class maps instead.  Images may have mixed sizes; they
    are grouped by (H, W) and run up to `batch` at a time.  A full batch of a size that has been seen before replays a
    captured graph (at most MAX_GRAPHS are kept per network, least recently used first out); everything else runs un-graphed.
    A batch is cut into launches of the lengths `launch_lengths` allows, all lengths under `batch_invariant=True` (LaunchPlanner).

    Three options compose (inference.forward_step and inference.finish_group; DESIGN.md section 3 "How a prediction is composed"):
      `tta`    a mode of utils/tta.py ("hflip", "flips", "rot4", "d4"): every image is predicted in each view of the mode and the
               views' quantised probabilities are added before the argmax (uh_tta_views, the forward, uh_tta_merge);
      `tile`   a utils.tiling.TileConfig or its spec, "512,overlap=128": every image is cut into tiles of one shape,
               (min(size, H), min(size, W)), after the prepare of the WHOLE image (uh_tile_gather), and uh_tile_merge adds the
               tiles' quantised probabilities, weighted by a tent over the overlap;
      `model`  may be a utils.ensemble.Ensemble: every member runs its forward on the same staged tensor, cut by its own
               LaunchPlanner and replaying its own graph cache, and uh_ensemble_add adds the members' sums by their weights.
    Upload, prepare, views and gather run once per group, whatever the number of members (M) and views (V):

      tta  tile  members   per forward step                                     per image group
      -    -     1         forward                                              logits_to_classes_u8
      yes  -     1         views, forward(s), tta_merge: classes / probs        -
      any  -     M         views once; per member forward (+ tta_merge: sums)   per member ensemble_add; ensemble_finish(V)
      -    yes   1         forward, the logits kept                             tile_merge: classes / probs (*)
      yes  yes   1         views, forward(s), tta_merge: sums                   tile_merge(V): classes / probs
      any  yes   M         views once; per member as the two rows above         per member tile_merge: sums, ensemble_add;
                                                                                ensemble_finish(V, den)
      (*) the classes of an image that is one tile: logits_to_classes_u8, the untiled statement

    Everything after the quantiser is an integer sum and the last rung takes the first maximum, so the masks depend on no order
    of views, tiles or members.  Post-processing and grey coding run on the whole-image class map as ever.
    Untiled, a launch group is a cut piece of the batch for one plain model and `tta_group` source images otherwise: `batch`
    stays the number of network inputs per forward launch, the view batches are cut by `launch_lengths` and replay graphs like
    any batch, so every view gets the logits it gets alone and the prediction of a posed image is exactly the posed prediction.
    Tiled, the tiles of all images of a call that share a tile shape are pooled, whatever the images' sizes, and forwarded
    `tile_chunk` at a time, so every forward step but the last of a tile shape is full and device memory holds `batch` tiles of
    activations plus the results of the images in flight.  An image that fits in one tile is that tile and, without `tta`, gets
    the bits of the untiled path; the tile origins are not mirror-symmetric, so under `tile` a posed image is NOT promised the
    posed prediction.
    `probabilities(images)` returns the averaged probabilities of any row but the first, `confidence(images)` floor(255 max / sum)
    of an ensemble's summed probabilities per pixel.  A bare module, or an Ensemble of one member, runs the one-model rows."""

    MAX_GRAPHS = 4
    tta = tile = ensemble = None              # what a predictor has that was built with none of them

    def __init__(self, model: torch.nn.Module, batch: int = 8, postprocess: bool = True, amp: bool = True, device=None,
                 min_area: int = 15000, morph_kernel_size: int = 3, batch_invariant: bool = False, tta=None, tile=None):
        if batch < 1:
            raise ValueError("batch must be >= 1")
        self.batch_invariant = bool(batch_invariant)
        if tta is not None:
            from .utils.tta import tta_mask
            tta = tta_mask(tta)                                          # ValueError for anything but the four modes
        self.tta = tta
        if tile is not None:
            from .utils.tiling import tile_config
            tile = tile_config(tile)                                     # ValueError for a bad size, overlap or spec
        self.tile = tile
        if getattr(model, "n_classes", None) == 1:
            # predict.py:27 takes argmax(dim=1) of a one-channel tensor: all zeros.  Not reproduced.
            raise ValueError("BatchPredictor needs a multi-class head: predict.py's argmax over one channel is all zeros. "
                             "Binary (n_classes == 1) models are scored and dumped by unet_amd.evaluate(..., epoch_pred_dir=...)")
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if self.device.type != "cuda":
            raise RuntimeError("BatchPredictor needs an MI355X: the HIP path has no CPU fallback")
        from .utils.ensemble import single_model
        solo = single_model(model)
        self.ensemble = model.to(self.device).eval() if solo is None else None     # None: one network, the one-model rows
        self.model = solo.to(self.device).eval() if solo is not None else self.ensemble
        self.batch, self.postprocess, self.amp = int(batch), bool(postprocess), bool(amp)
        self.min_area, self.ksize = int(min_area), int(morph_kernel_size)
        self._lut = torch.from_numpy(GREY_CLASSES.copy()).to(self.device)
        self._flags = torch.empty(self.batch, dtype=torch.int32, device=self.device)
        nets = [(self.model, None)] if solo is not None else zip(self.ensemble.members, self.ensemble.weights)
        self._members = [_Member(m, w, self.batch, self.amp, self.batch_invariant, self.tta) for m, w in nets]
        self.planner = self._members[0].planner
        self._pin_in: Optional[torch.Tensor] = None
        self._pin_out: Optional[torch.Tensor] = None
        self._upload_done = torch.cuda.Event()                        # recorded behind every upload out of _pin_in
        self.events = None                    # set to a list to collect (stage, start event, end event) per batch
        self.graph_replays = 0

    # ---------------------------------------------------------------- stages
    def _mark(self, name, fn, *a, **kw):
        return timed_stage(self.events, name, fn, *a, **kw)

    def launch_lengths(self, H: int, W: int) -> List[int]:
        return self.planner.launch_lengths(H, W)

    @property
    def _graphs(self):
        """The graph cache of the first network (the only one of a bare model): kept by the member, read here as `planner` is."""
        return self._members[0]._graphs

    def tta_group(self, H: int, W: int) -> int:
        return min(m.planner.tta_group(H, W) for m in self._members)

    def tile_chunk(self, th: int, tw: int) -> int:
        return min(m.planner.tile_chunk(th, tw) for m in self._members)

    def _pinned(self, which: str, nbytes: int) -> torch.Tensor:
        buf = getattr(self, which)
        if buf is None or buf.numel() < nbytes:
            buf = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
            setattr(self, which, buf)
        return buf[:nbytes]

    def _upload(self, arrays: List[np.ndarray], H: int, W: int) -> torch.Tensor:
        B = len(arrays)
        stage = self._pinned("_pin_in", B * H * W).view(B, H, W)
        host = stage.numpy()
        for i, a in enumerate(arrays):
            host[i] = a
        dev = torch.empty(B, H, W, dtype=torch.uint8, device=self.device)
        dev.copy_(stage, non_blocking=True)
        return dev

    def _stage(self, arrays: List[np.ndarray]) -> torch.Tensor:
        """Equally sized uint8 [H,W] images -> the network's input float32 [B,1,H,W], channels_last, on the device."""
        H, W = arrays[0].shape
        B = len(arrays)
        self._upload_done.synchronize()            # the pinned staging buffer is free once the previous upload has left it
        img = self._mark("upload", self._upload, arrays, H, W)
        self._upload_done.record()
        x = torch.empty(B, 1, H, W, dtype=torch.float32, device=self.device, memory_format=torch.channels_last)
        flags = self._flags if B <= self._flags.numel() else torch.empty(B, dtype=torch.int32, device=self.device)
        self._mark("prepare", ops.predict_prepare_u8, img, x, flags)
        return x

    def _forward(self, x: torch.Tensor, size: Tuple[int, int], m: _Member) -> torch.Tensor:
        """One launch of the network of `m`, through its planner and graph cache."""
        full = m.planner.launch_lengths(*size)[-1]                     # the longest launch this size allows
        size = (x.shape[0],) + tuple(size)
        if x.shape[0] == full and size in m._seen:
            g = m._graphs.pop(size, None)
            if g is None:
                while len(m._graphs) >= self.MAX_GRAPHS:
                    m._graphs.popitem(last=False)                     # least recently used
                g = GraphedForward(m.model, x, amp=self.amp, plan_images=1 if self.batch_invariant else 0)
            m._graphs[size] = g
            self.graph_replays += 1
            return g(x)
        if x.shape[0] == full:
            m._seen.add(size)
        return eval_forward(m.model, x, self.amp, plan_images=1 if self.batch_invariant else 0)

    def run_batch(self, arrays: List[np.ndarray], grey: bool = True, probs: bool = False, conf: bool = False) -> np.ndarray:
        """One batch of equally sized uint8 [H,W] images -> uint8 [B,H,W] on the host (grey-coded, or class indices), in as
        few launches as launch_lengths allows; or (probs; under `tta`, `tile` or an ensemble) float32 [B,NC,H,W]; or (conf; an
        ensemble) uint8 [B,2,H,W], the masks and the confidence maps."""
        H, W = arrays[0].shape
        if self.tile is not None:
            return np.stack(self._run_tiled(arrays, grey, probs, conf))
        if self.ensemble is None and self.tta is None:
            groups = self.planner.cut(len(arrays), H, W)               # one plain model: a group is a launch
        else:
            g = self.batch if self.tta is None else self.tta_group(H, W)
            groups = [min(g, len(arrays) - s) for s in range(0, len(arrays), g)]
        more = {k: True for k, v in (("probs", probs), ("conf", conf)) if v}     # masks alone are _launch(arrays, grey), as ever
        out, s = [], 0
        for b in groups:
            out.append(self._launch(arrays[s:s + b], grey, **more))
            s += b
        return out[0] if len(out) == 1 else np.concatenate(out)

    def _forwards(self):
        """Per member the forward that inference.forward_step calls: _forward_cut through that member's planner and graphs."""
        return [lambda x, size, m=m: self._forward_cut(x, size, m) for m in self._members]

    def _launch(self, arrays: List[np.ndarray], grey: bool, probs: bool = False, conf: bool = False) -> np.ndarray:
        """One launch group of equally sized images: stage, forward step, finish, deliver."""
        with torch.cuda.device(self.device):
            results = forward_step(self._stage(arrays), self._forwards(), self.tta, last=self.ensemble is None, probs=probs,
                                   mark=self._mark)
            return self._finish(results, None, arrays[0].shape, grey, probs, conf)

    def _finish(self, results, tile, size: Tuple[int, int], grey: bool, probs: bool, conf: bool) -> np.ndarray:
        """The members' results for a group of images -> uint8 [B,H,W] on the host, (probs) float32 [B,NC,H,W], or (conf; an
        ensemble) uint8 [B,2,H,W]: the masks and the confidence maps."""
        weights = None if self.ensemble is None else [m.weight for m in self._members]
        out = finish_group(results, weights, tile, size, self.tta, probs=probs, confidence=conf, mark=self._mark)
        if probs:
            return out.probs.permute(0, 3, 1, 2).cpu().numpy()
        masks = self._deliver(out.classes, grey)
        if conf:
            return np.stack([masks, out.confidence.cpu().numpy()], axis=1)
        return masks

    def _deliver(self, cls: torch.Tensor, grey: bool) -> np.ndarray:
        """Class maps uint8 [B,H,W] on the device -> post-processed, grey-coded, on the host."""
        B, H, W = cls.shape
        if self.postprocess:
            from .utils.post_process import _run as _postprocess_run
            cls = self._mark("postprocess", _postprocess_run, cls, self.min_area, self.ksize)
        if grey:
            self._mark("grey", ops.classes_to_grey_u8, cls, self._lut, cls)
        out = self._pinned("_pin_out", B * H * W).view(B, H, W)
        self._mark("download", out.copy_, cls, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        return out.numpy().copy()

    def _forward_cut(self, x: torch.Tensor, size: Tuple[int, int], m: _Member) -> torch.Tensor:
        """_forward for a batch of any length (views, tiles), in as few launches as launch_lengths allows."""
        cut = m.planner.cut(x.shape[0], *size)
        if len(cut) == 1:
            return self._forward(x, size, m)
        return torch.cat([self._forward(part, size, m).clone() for part in x.split(cut)])   # (a replayed graph returns its static buffer)

    # ---------------------------------------------------------------- tiled prediction
    def _prepare_tiles(self, arrays: List[np.ndarray]) -> torch.Tensor:
        """Equally sized images -> their tiles [B*ny*nx,1,th,tw] on the device; the prepare sees the WHOLE images."""
        with torch.cuda.device(self.device):
            return self._mark("gather", ops.tile_gather, self._stage(arrays), self.tile)

    def _tile_forward(self, tiles: torch.Tensor, shape: Tuple[int, int]) -> torch.Tensor:
        """One forward step of the tiled flow, in a tensor that outlives the next step: the logits [n,NC,th,tw] of the tiles,
        or under test-time augmentation the int32 sums [n,th,tw,NC] over their views; for an ensemble the members' side by
        side in dimension 1, [n,M,...]."""
        with torch.cuda.device(self.device):
            out = list(forward_step(tiles, self._forwards(), self.tta, mark=self._mark))
            if self.ensemble is not None:
                return torch.stack(out, dim=1)                          # (copies: a replayed graph returns its static buffer)
            return out[0].clone() if self.tta is None else out[0]      # (the same; the view sums are a fresh tensor)

    def _tile_finish(self, src: torch.Tensor, H: int, W: int, grey: bool, probs: bool, conf: bool = False) -> np.ndarray:
        """The results of _tile_forward for every tile of a batch of H x W images -> what _finish returns."""
        with torch.cuda.device(self.device):
            return self._finish([src] if self.ensemble is None else src.unbind(1), self.tile, (H, W), grey, probs, conf)

    def _run_tiled(self, arrays: List[np.ndarray], grey: bool, probs: bool = False, conf: bool = False) -> List[np.ndarray]:
        """Images of any sizes -> their results in input order.  The tiles of all images that share a tile shape are pooled:
        same-size images (up to `batch`) share an upload, a prepare, a gather and a merge; the pool forwards `tile_chunk`
        tiles at a time, so every forward step but the last of a tile shape is full, and an image is merged and delivered
        as soon as its last tile is through."""
        from .utils.tiling import tile_shape
        result: List[Optional[np.ndarray]] = [None] * len(arrays)
        by_shape: "OrderedDict[Tuple[int, int], List[int]]" = OrderedDict()
        for i, a in enumerate(arrays):
            by_shape.setdefault(tile_shape(a.shape[0], a.shape[1], self.tile), []).append(i)
        for shape, members in by_shape.items():
            chunk = self.tile_chunk(*shape)
            waiting: Optional[torch.Tensor] = None                     # tiles not yet forwarded
            done: List[torch.Tensor] = []                              # results of forwarded tiles, in order
            n_done = 0
            records = deque()                                          # (image indices, H, W, tiles) in tile order

            def advance(final: bool):
                nonlocal waiting, done, n_done
                while waiting is not None and (waiting.shape[0] >= chunk or final):
                    part, rest = waiting[:chunk], waiting[chunk:]
                    waiting = rest if rest.shape[0] else None
                    done.append(self._tile_forward(part, shape))
                    n_done += part.shape[0]
                    while records and records[0][3] <= n_done:
                        idx, H, W, n = records.popleft()
                        have = done[0] if len(done) == 1 else torch.cat(done)
                        done = [have[n:]] if have.shape[0] > n else []
                        n_done -= n
                        out = self._tile_finish(have[:n], H, W, grey, probs, conf)
                        for k, i in enumerate(idx):
                            result[i] = np.ascontiguousarray(out[k])

            for _, group in plan_batches([arrays[i].shape for i in members], self.batch):
                idx = [members[k] for k in group]
                tiles = self._prepare_tiles([arrays[i] for i in idx])
                records.append((idx, arrays[idx[0]].shape[0], arrays[idx[0]].shape[1], tiles.shape[0]))
                waiting = tiles if waiting is None else torch.cat([waiting, tiles])
                advance(False)
            advance(True)
        return result

    def _run(self, images, grey: bool, probs: bool = False, conf: bool = False) -> List[np.ndarray]:
        arrays = [_as_grey_array(im) for im in images]
        if self.tile is not None:
            return self._run_tiled(arrays, grey, probs, conf)
        result: List[Optional[np.ndarray]] = [None] * len(arrays)
        for _, members in plan_batches([a.shape for a in arrays], self.batch):
            out = self.run_batch([arrays[i] for i in members], grey, probs, conf)
            for k, i in enumerate(members):
                result[i] = np.ascontiguousarray(out[k])
        return result

    def __call__(self, images) -> List[np.ndarray]:
        return self._run(images, True)

    def classes(self, images) -> List[np.ndarray]:
        return self._run(images, False)

    def probabilities(self, images) -> List[np.ndarray]:
        """float32 [NC,H,W] per image: the mean over the views of the softmax probabilities (multiples of 2^-24 / V); under
        `tile` the weighted mean over the covering tiles (and their views), (float)(sum / (den V 2^24)); for an ensemble the
        weighted mean over its members of either, or of the members' plain probabilities, (float)(sum / (den V 2^24 weights))."""
        if self.tta is None and self.tile is None and self.ensemble is None:
            raise RuntimeError("probabilities() returns the mean over the views of test-time augmentation (tta=...) or over the "
                               "covering tiles of tiled prediction (tile=...): build the predictor with one of them")
        return self._run(images, False, probs=True)

    def masks_and_confidence(self, images, grey: bool = True) -> Tuple[List[np.ndarray], List[np.ndarray]]:
        """(what predictor(images) returns, what confidence(images) returns) from one pass over the images."""
        if self.ensemble is None:
            raise RuntimeError("confidence() measures how far the members of an ensemble agree: build the predictor with a "
                               "utils.ensemble.Ensemble of two or more members")
        both = self._run(images, grey, conf=True)
        return [np.ascontiguousarray(b[0]) for b in both], [np.ascontiguousarray(b[1]) for b in both]

    def confidence(self, images) -> List[np.ndarray]:
        """uint8 [H,W] per image: floor(255 max_c s_c / sum_c s_c) of the ensemble's summed probabilities s (255: every
        member puts everything on one class), formed in integers on the device (uh_ensemble_finish)."""
        return self.masks_and_confidence(images)[1]


def main(argv=None) -> int:
    """`python -m unet_amd.predict ...`: the reference's predict.py command line (predict_cli.py)."""
    from .predict_cli import main as _main
    return _main(argv)


if __name__ == "__main__":
    import sys
    sys.exit(main())
