"""Validation metric of /root/reference/evaluate.py:12-171: eval-mode forward (running statistics folded into the conv
epilogue), device-side masks, raw Dice and -- with postprocess=True -- the Dice after utils/post_process.postprocess_mask,
which here runs on the device for the whole batch (the reference copies every image to the host for OpenCV).  With
epoch_pred_dir the predictions are also written as grey-coded PNGs (evaluate.py:35-40, 88-105, 146-164): the coding is one
table pass per batch on the device (uh_classes_to_grey_u8), the files are encoded and written by a background writer, and
evaluate returns once they are on disk.  Without it nothing of that runs.  With `metrics` (a utils.contour_metrics.ContourMetrics)
the scored masks of every batch also go through uh_contour_metrics (HD / HD95 / ASSD / IoU); the records stay on the device
until the accumulator's result() is read.  Without it nothing of that runs either.
With `tta` (a mode of utils/tta.py) the prediction that is scored is the average over the views of the mode: the views are built on
the device (uh_tta_views), run through the batch-invariant forward and merged (uh_tta_merge); everything after the argmax /
threshold runs on the merged classes unchanged.  Without it nothing of that runs.
With `tile` (a utils.tiling.TileConfig or its spec) a batch whose images are larger than one tile is cut into tiles on the device
(uh_tile_gather), the tiles run through the batch-invariant forward a batch at a time and uh_tile_merge puts the class map
back together (with `tta`: per tile the views, the forward and uh_tta_merge, then the tile merge of the integer sums); a batch
whose images fit in one tile takes the statements it takes without `tile`.  Without it nothing of that runs.
`python -m unet_amd.evaluate -m CKPT --data-root DIR` scores a checkpoint without training (evaluate_cli.py)."""
from __future__ import annotations

import torch

from . import ops
from .inference import finish_group, forward_step
from .utils.dice_score import dice_coeff
from .utils.post_process import postprocess_mask
from .utils.tta import tta_mask


class _PredDump:
    """pred_batch{k}_sample{i}.png under epoch_pred_dir, k counting from 1, and the same names under postprocessed/ when
    post-processing is on (evaluate.py:35-40, 88-105, 146-164)."""

    def __init__(self, epoch_pred_dir, postprocess: bool, device):
        import os
        from .predict import GREY_BINARY, GREY_CLASSES, GREY_POSTPROCESSED
        from .utils.png_writer import OrderedPngWriter
        self.dir = os.fspath(epoch_pred_dir)
        self.post_dir = os.path.join(self.dir, "postprocessed") if postprocess else None
        os.makedirs(self.post_dir if postprocess else self.dir, exist_ok=True)
        self.luts = {k: torch.from_numpy(v.copy()).to(device) for k, v in
                     (("classes", GREY_CLASSES), ("postprocessed", GREY_POSTPROCESSED), ("binary", GREY_BINARY))}
        self.writer = OrderedPngWriter()
        self.order = 0

    def add(self, batch_index: int, raw_u8, raw_table: str, post_u8=None, post_table=None):
        import os
        grey = [(self.dir, ops.classes_to_grey_u8(raw_u8.contiguous(), self.luts[raw_table]))]
        if post_u8 is not None:
            grey.append((self.post_dir, ops.classes_to_grey_u8(post_u8.contiguous(), self.luts[post_table])))
        host = [(d, g.cpu().numpy()) for d, g in grey]
        for i in range(raw_u8.shape[0]):
            for d, g in host:                      # the raw file, then its post-processed twin, as the reference writes them
                self.writer.submit(self.order, os.path.join(d, f"pred_batch{batch_index}_sample{i}.png"), g[i])
                self.order += 1

    def close(self):
        self.writer.close()


def _pieces(net, n):
    """The forward evaluate gives inference.forward_step (inside evaluate's autocast): `net` on pieces of `n` inputs -- each view
    of a batch is a launch of its own, of the batch's length -- under the pinned plan of one image."""
    def forward(x, size):
        with ops.plan_images(1):
            out = [net(x[s:s + n]) for s in range(0, x.shape[0], n)]
        return out[0] if len(out) == 1 else torch.cat(out)
    return forward


def _tile_results(net, tiles, B, tta):
    """What one network gives for every tile of a batch, the tiles going through forward_step `B` at a time (under `tta` each
    such chunk with views of its own).  A member's tiles all go through before the next member's."""
    return torch.cat([r for s in range(0, tiles.shape[0], B)
                      for r in forward_step(tiles[s:s + B], [_pieces(net, min(B, tiles.shape[0] - s))], tta)])


@torch.inference_mode()
def evaluate(net, dataloader, device, amp, epoch_pred_dir=None, postprocess=True, process_group=None, metrics=None, tta=None,
             tile=None):
    """evaluate.py:12-171.  `postprocess=True` is the reference's default (evaluate.py:13): the second return value is then
    the Dice after post-processing and the minimum is taken over min(raw, post-processed) per batch (evaluate.py:85).
    Batches are consumed lazily; under torch.distributed (every rank evaluating its shard of the validation set) the Dice
    sums and batch counts are all-reduced so that every rank returns the metric of the whole set.  `metrics`: an accumulator
    that is updated with the contour-metric records of the raw and (postprocess=True) the post-processed masks of every
    batch, P and T being exactly the masks whose Dice is taken, and all-reduced where the Dice sums are; the return value
    is the same 3-tuple either way.  `tta`: "hflip", "flips", "rot4" or "d4" -- the masks that are scored, post-processed,
    measured and dumped are those of the prediction averaged over these views (None: one forward, as the reference).
    `tile`: a TileConfig or a spec like "512,overlap=128" -- images larger than one tile are predicted tile by tile and merged
    with the overlap blended (None: whole images).
    `net` may be a utils.ensemble.Ensemble: the masks that are scored are then the first maximum of the members' integer sums
    (uh_ensemble_add, uh_ensemble_finish), under `tta` and `tile` as well; an Ensemble of one member is scored as that member."""
    from .utils.ensemble import Ensemble, single_model
    ens = net if isinstance(net, Ensemble) and single_model(net) is None else None
    whole = net                                                      # what goes back into train mode at the end
    if ens is None:
        net = single_model(net)
    members, weights = ([net], None) if ens is None else (ens.members, ens.weights)
    if tta is not None:
        tta = tta_mask(tta)
    if tile is not None:
        from .utils.tiling import tile_config, tile_count
        tile = tile_config(tile)
    net.eval()
    num_val_batches = 0
    dice_score = torch.zeros((), dtype=torch.float32, device=device)
    dice_post = torch.zeros((), dtype=torch.float32, device=device)
    min_dice = torch.full((), 10.0, dtype=torch.float32, device=device)
    dump = _PredDump(epoch_pred_dir, postprocess, device) if epoch_pred_dir is not None else None
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
        for batch in dataloader:
            num_val_batches += 1
            image, mask_true = batch["image"], batch["mask"]
            image = image.to(device=device, dtype=torch.float32, memory_format=torch.channels_last)
            mask_true = mask_true.to(device=device, dtype=torch.float32)
            tiled = tile is not None and tile_count(image.shape[2], image.shape[3], tile) > 1
            plain = tta is None and not tiled and ens is None
            if plain:
                mask_pred = net(image)
            else:                                                      # the ladder of inference.py, uint8 [B,H,W] classes
                B, size = image.shape[0], tuple(image.shape[2:])
                if tiled:
                    tiles = ops.tile_gather(image, tile)
                    results = (_tile_results(m, tiles, B, tta) for m in members)
                else:
                    results = forward_step(image, [_pieces(m, B) for m in members], tta, last=ens is None)
                merged = finish_group(results, weights, tile if tiled else None, size, tta).classes
            if net.n_classes == 1:
                mask_true = torch.div(mask_true, 2, rounding_mode="floor")                      # evaluate.py:56
                assert mask_true.min() >= 0 and mask_true.max() <= 1, "True mask indices should be in [0, 1]"
                if plain:
                    pred = ops.threshold_mask(mask_pred.squeeze(1))    # sigmoid(x) > 0.5  <=>  x > 0   (evaluate.py:60-62)
                else:
                    pred = merged.float()                              # the averaged (or blended) sigmoid > 0.5
                d = dice_coeff(pred, mask_true, reduce_batch_first=False)
                cur = d
                if postprocess:
                    # evaluate.py:71-78 literally: the binary mask goes in coded {0,255}, postprocess_mask looks for class 2
                    # (finds none) and `processed // 255` is the prediction that is scored
                    coded = (pred * 255).to(torch.uint8)
                    processed_u8 = postprocess_mask(coded) // 255
                    processed = processed_u8.float()
                    dp = dice_coeff(processed, mask_true, reduce_batch_first=False)
                    dice_post += dp
                    cur = torch.minimum(d, dp)                                                  # evaluate.py:85
                if metrics is not None:
                    true_u8 = mask_true.to(torch.uint8).contiguous()
                    metrics.update(ops.contour_metrics(pred.to(torch.uint8).contiguous(), true_u8, 1, 1), "raw")
                    if postprocess:
                        metrics.update(ops.contour_metrics(processed_u8.contiguous(), true_u8, 1, 1), "post")
                if dump is not None:                                                            # evaluate.py:88-105
                    dump.add(num_val_batches, pred.to(torch.uint8), "binary", processed_u8 if postprocess else None, "binary")
            else:
                idx = ops.argmax_classes(mask_pred) if plain else merged.long()   # evaluate.py:111
                true_c = (mask_true == 2).float()
                d = dice_coeff((idx == 2).float(), true_c, reduce_batch_first=False)
                cur = d
                if postprocess:
                    processed = postprocess_mask(idx.to(torch.uint8))                           # evaluate.py:125-134
                    dice_post += dice_coeff((processed == 2).float(), true_c, reduce_batch_first=False)
                if metrics is not None:
                    true_u8 = mask_true.to(torch.uint8).contiguous()
                    metrics.update(ops.contour_metrics(idx.to(torch.uint8).contiguous(), true_u8, 2, 2), "raw")
                    if postprocess:
                        metrics.update(ops.contour_metrics(processed.contiguous(), true_u8, 2, 2), "post")
                if dump is not None:                                                            # evaluate.py:146-164
                    dump.add(num_val_batches, idx.to(torch.uint8), "classes", processed if postprocess else None,
                             "postprocessed")
            dice_score += d
            min_dice = torch.minimum(min_dice, cur.float())
    whole.train()
    if dump is not None:
        dump.close()                                            # every file is on disk before the metric is returned
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size(process_group) > 1:
        acc = torch.stack([dice_score, dice_post, torch.tensor(float(num_val_batches), device=device)])
        dist.all_reduce(acc, op=dist.ReduceOp.SUM, group=process_group)
        dist.all_reduce(min_dice, op=dist.ReduceOp.MIN, group=process_group)
        dice_score, dice_post, n = acc[0], acc[1], acc[2].clamp_min(1.0)
        if metrics is not None:
            metrics.all_reduce(process_group)
    else:
        n = max(num_val_batches, 1)
    if not postprocess:
        dice_post = dice_score                                                                  # evaluate.py:168-169
    return dice_score / n, dice_post / n, min_dice


def main(argv=None) -> int:
    """`python -m unet_amd.evaluate ...`: scores a checkpoint on a validation split (evaluate_cli.py)."""
    from .evaluate_cli import main as _main
    return _main(argv)


if __name__ == "__main__":
    import sys
    sys.exit(main())
