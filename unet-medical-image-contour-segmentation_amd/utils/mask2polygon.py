"""Stage 5 of seg_main.py on the device: utils/mask2polygon.py (grey > 127, external contours, LabelMe JSON).

    external_contours(grey) -> [[np.int32 [n, 2], ...] per image]   cv2.findContours(RETR_EXTERNAL, CHAIN_APPROX_SIMPLE)
                                                                    + squeeze(axis=1)   (mask2polygon.py:325-329)
    contour_json(contours, stem, width, height) -> dict | None      mask2polygon.py:336-359 (None: no contour, no file)
    json_text(d) -> str                                             json.dump(..., ensure_ascii=False, indent=2)

The contours are traced on the device (csrc/seg_pipeline.hip: union-find labels, one wave per contour); only the point
counts and the points come back.  PARITY UNPINNED against OpenCV (not installed): the tests hold a literal restatement
of OpenCV's icvFetchContour and hand-derived answers."""
from __future__ import annotations

import json

import numpy as np
import torch

from .. import ops
from .._lib import LIB


def external_contours(grey: torch.Tensor):
    ops._require_gpu(grey, "grey")
    squeeze = grey.dim() == 2
    g = (grey.unsqueeze(0) if squeeze else grey)
    if g.dim() != 3 or g.dtype != torch.uint8:
        raise RuntimeError(f"grey must be uint8 [H,W] or [B,H,W], got {g.dtype} {tuple(grey.shape)}")
    g = g.contiguous()
    B, H, W = g.shape
    dev = g.device
    nbytes = LIB.query("uh_contours_ws_bytes", B, H, W)
    if nbytes == 0:
        raise RuntimeError(f"uh_contours_ws_bytes refused {B}x{H}x{W}")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    info = torch.zeros(3 + 2 * B + 1, dtype=torch.int32, device=dev)
    npts = torch.empty(LIB.query("uh_contours_max", B, H, W), dtype=torch.int32, device=dev)
    st = ops._stream()
    LIB.call("uh_contours_count", g.data_ptr(), B, H, W, ws.data_ptr(), nbytes, info.data_ptr(), npts.data_ptr(), st)
    info_h = info.cpu().numpy()
    total_c, total_p = int(info_h[0]), int(info_h[1])
    pts = torch.empty(max(total_p, 1), 2, dtype=torch.int32, device=dev)
    LIB.call("uh_contours_emit", ws.data_ptr(), nbytes, B, H, W, info.data_ptr(), npts.data_ptr(), pts.data_ptr(), total_p, st)
    info_h = info.cpu().numpy()
    if info_h[2] != 0:
        raise RuntimeError(f"contour tracer reported an inconsistent walk (flags {int(info_h[2])})")
    counts = npts[:total_c].cpu().numpy()
    pts_h = pts[:total_p].cpu().numpy()
    ncont = info_h[3:3 + B]
    out, c, p = [], 0, 0
    for b in range(B):
        lst = []
        for _ in range(int(ncont[b])):
            n = int(counts[c])
            lst.append(pts_h[p:p + n])
            c += 1
            p += n
        out.append(lst)
    return out[0] if squeeze else out


def contour_json(contours, stem: str, width: int, height: int):
    if not contours:
        return None                                                 # mask2polygon.py:331-333: warning, no JSON
    return {
        "version": "1.0.2.799",
        "imagePath": stem,
        "imageData": None,
        "flags": {},
        "shapes": [{"label": 1, "labelIndex": 0, "points": np.asarray(c).tolist(), "shape_type": "polygon",
                    "description": "", "mask": None, "group_id": None, "flags": {}} for c in contours],
        "imageWidth": int(width),
        "imageHeight": int(height),
    }


def json_text(d) -> str:
    return json.dumps(d, ensure_ascii=False, indent=2)


def write_json(path: str, d) -> None:
    with open(path, "w", encoding="utf-8") as f:
        json.dump(d, f, ensure_ascii=False, indent=2)
