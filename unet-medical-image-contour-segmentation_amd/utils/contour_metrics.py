"""Contour-distance metrics on the device (csrc/contour_metrics.hip; the reference has no counterpart): Hausdorff distance,
its 95th percentile, average symmetric surface distance and IoU of a predicted mask P against the truth T.

    border S(M)   pixels of M with one of their four edge neighbours outside M (outside the image counts as outside)
    D_M[x]        min over q in S(M) of |x - q|^2, an exact integer in pixel units
    R             sqrt(D_T[p]) for p in S(P) together with sqrt(D_P[q]) for q in S(T): one multiset
    HD = max R, HD95 = numpy.percentile(R, 95), ASSD = mean R, IoU = |P & T| / |P | T|
    both masks empty: HD = HD95 = ASSD = 0, IoU = 1; exactly one empty: the distances are nan ("undefined"), IoU = 0

    contour_metrics(pred, true, cls=2, spacing=1.0)  -> dict of per-image tensors, on the device
    ContourMetrics(spacing=1.0)                      accumulator over the batches of an evaluation:
        .update(records, which="raw" | "post")       appends a record table of ops.contour_metrics; nothing is read back
        .all_reduce(group)                           every rank gets the sums, counts, maximum and n_undefined of the set
        .result()                                    the single host read -> {"raw": {...}, "post": {...}}

Set means of the distances run over the defined images, hd_max is their maximum; the IoU mean runs over every image.
`spacing` is isotropic (one pixel pitch for both axes) and multiplies the reported distances on the host: the kernels stay
in integer pixel units."""
from __future__ import annotations

from typing import Dict, List, Optional

import torch

INT_FIELDS = ("n_pred", "n_true", "n_inter", "n_union", "n_border_pred", "n_border_true", "n", "max_d2", "d2_lo", "d2_hi",
              "undefined", "reserved")
FLOAT_FIELDS = ("weight", "sum_dist", "hd", "hd95", "assd", "iou")
WHICH = ("raw", "post")
_HD, _HD95, _ASSD, _IOU = 8, 9, 10, 11               # float64 columns of a record row
_UNDEFINED = 10                                       # int32 column
_NSUM = 6                                             # sum hd, sum hd95, sum assd, sum iou, images, undefined images


def decode_records(records: torch.Tensor) -> Dict[str, torch.Tensor]:
    """The fields of a float64 [B,12] record table (uh_contour_record rows) by name; integers as int64."""
    if records.dtype != torch.float64 or records.dim() != 2 or records.shape[1] != 12:
        raise RuntimeError(f"a record table is float64 [B,12], got {records.dtype} {tuple(records.shape)}")
    ints = records.contiguous().view(torch.int32)[:, :12].to(torch.int64) & 0xFFFFFFFF
    out = {name: ints[:, i] for i, name in enumerate(INT_FIELDS) if name != "reserved"}
    out.update({name: records[:, 6 + i] for i, name in enumerate(FLOAT_FIELDS)})
    return out


def _as_u8_batch(t: torch.Tensor) -> torch.Tensor:
    if t.dim() == 2:
        t = t.unsqueeze(0)
    if t.dim() != 3:
        raise RuntimeError(f"masks are [H,W] or [B,H,W], got {tuple(t.shape)}")
    return t.to(torch.uint8).contiguous()


def contour_metrics(pred: torch.Tensor, true: torch.Tensor, cls: int = 2, spacing: float = 1.0) -> Dict[str, torch.Tensor]:
    """Per-image metrics of (pred == cls) against (true == cls) for class maps [H,W] or [B,H,W] on the GPU (any dtype that
    holds the class values exactly).  -> {"hd", "hd95", "assd", "iou": float64 [B]; "undefined": bool [B]; the integer
    fields of the record: int64 [B]}."""
    from .. import ops
    rec = decode_records(ops.contour_metrics(_as_u8_batch(pred), _as_u8_batch(true), cls, cls))
    for k in ("hd", "hd95", "assd"):
        rec[k] = rec[k] * float(spacing)
    rec["undefined"] = rec["undefined"] != 0
    del rec["weight"], rec["sum_dist"]
    return rec


def _set_sums(records: torch.Tensor):
    """-> (float64 [6] sums, float64 [] maximum HD) of a record table, on its device."""
    undefined = records.view(torch.int32)[:, _UNDEFINED] != 0
    zero = torch.zeros((), dtype=torch.float64, device=records.device)
    dist = torch.where(undefined[:, None], zero, records[:, _HD:_ASSD + 1])
    sums = torch.cat([dist.sum(0), records[:, _IOU].sum(0, keepdim=True),
                      torch.full((1,), float(records.shape[0]), dtype=torch.float64, device=records.device),
                      undefined.sum(0, keepdim=True).to(torch.float64)])
    hd_max = torch.where(undefined, zero - float("inf"), records[:, _HD]).amax() if records.shape[0] else zero - float("inf")
    return sums, hd_max


class ContourMetrics:
    def __init__(self, spacing: float = 1.0):
        self.spacing = float(spacing)
        self._records: Dict[str, List[torch.Tensor]] = {w: [] for w in WHICH}
        self._reduced: Optional[Dict[str, tuple]] = None

    def update(self, records: torch.Tensor, which: str = "raw") -> None:
        if which not in WHICH:
            raise ValueError(f"which is 'raw' or 'post', got {which!r}")
        if records.dtype != torch.float64 or records.dim() != 2 or records.shape[1] != 12:
            raise RuntimeError(f"a record table is float64 [B,12], got {records.dtype} {tuple(records.shape)}")
        self._records[which].append(records.detach())
        self._reduced = None

    def _table(self, which: str, device=None) -> torch.Tensor:
        recs = self._records[which]
        if recs:
            return torch.cat(recs).contiguous()
        return torch.zeros(0, 12, dtype=torch.float64, device=device)

    def _device(self):
        for w in WHICH:
            if self._records[w]:
                return self._records[w][0].device
        return torch.device("cpu")

    def all_reduce(self, group=None) -> None:
        """Sums, counts and n_undefined are added and the maximum is taken over the ranks of `group`: result() then gives the
        set figures of the concatenated set on every rank (the per-image arrays stay this rank's own)."""
        import torch.distributed as dist
        device = self._device()
        local = {w: _set_sums(self._table(w, device)) for w in WHICH}
        sums = torch.stack([local[w][0] for w in WHICH])
        maxs = torch.stack([local[w][1] for w in WHICH])
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
            dist.all_reduce(sums, op=dist.ReduceOp.SUM, group=group)
            dist.all_reduce(maxs, op=dist.ReduceOp.MAX, group=group)
        self._reduced = {w: (sums[i], maxs[i]) for i, w in enumerate(WHICH)}

    def result(self) -> Dict[str, Dict]:
        device = self._device()
        tables = {w: self._table(w, device) for w in WHICH}
        reduced = self._reduced or {w: _set_sums(tables[w]) for w in WHICH}
        # one tensor, one copy to the host
        flat = torch.cat([t.reshape(-1) for t in tables.values()] +
                         [torch.cat([reduced[w][0], reduced[w][1].reshape(1)]) for w in WHICH]).cpu()
        out, at = {}, 0
        host = {}
        for w in WHICH:
            n = tables[w].shape[0]
            host[w] = flat[at:at + n * 12].reshape(n, 12)
            at += n * 12
        for w in WHICH:
            stats = flat[at:at + _NSUM + 1].tolist()
            at += _NSUM + 1
            images, undefined = int(stats[4]), int(stats[5])
            defined = images - undefined
            mean = lambda s: s / defined * self.spacing if defined else float("nan")   # noqa: E731
            fields = decode_records(host[w])
            per_image = {k: (fields[k] * self.spacing).numpy() for k in ("hd", "hd95", "assd")}
            per_image["iou"] = fields["iou"].numpy()
            per_image["undefined"] = (fields["undefined"] != 0).numpy()
            out[w] = {"hd95": mean(stats[1]), "hd": mean(stats[0]), "hd_max": stats[6] * self.spacing if defined else float("nan"),
                      "assd": mean(stats[2]), "iou": stats[3] / images if images else float("nan"),
                      "n": images, "n_undefined": undefined, "per_image": per_image}
        return out


def format_line(result: Dict[str, Dict], postprocess: bool = True) -> str:
    """One log line: HD95 / HD / ASSD / IoU of the raw and, where scored, the post-processed masks."""
    def part(name, r):
        return (f"{name} HD95 {r['hd95']:.4g}  HD {r['hd']:.4g} (max {r['hd_max']:.4g})  ASSD {r['assd']:.4g}  IoU {r['iou']:.4g}"
                f"  [{r['n']} images, {r['n_undefined']} undefined]")
    line = "Validation contour metrics: " + part("raw", result["raw"])
    if postprocess and result["post"]["n"]:
        line += "  |  " + part("postprocessed", result["post"])
    return line
