"""scipy / numpy restatement of the contour-metric definitions (DESIGN.md section 3 "Contour metrics"), the yardstick of
csrc/contour_metrics.hip -- the role tests/resize_ref.py plays for the rescale.  Per image, P and T boolean H x W masks:

    border S(M)   M & ~binary_erosion(M, 4-neighbourhood, border_value=0)
    D_M[x]        min over q in S(M) of |x - q|^2 as an exact integer (distance_transform_edt's indices, recomputed as
                  dy^2 + dx^2); 0xFFFFFFFF everywhere when S(M) is empty
    R             sqrt(D_T[p]) for p in S(P) together with sqrt(D_P[q]) for q in S(T)
    HD = max R, HD95 = numpy.percentile(R, 95), ASSD = mean R, IoU = |P & T| / |P | T|
    both empty: HD = HD95 = ASSD = 0, IoU = 1, n = 0;  exactly one empty: nan, undefined, IoU = 0, n = 0."""
import numpy as np
from scipy import ndimage

NO_FEATURE = 0xFFFFFFFF
_CROSS = ndimage.generate_binary_structure(2, 1)


def border(mask):
    mask = np.asarray(mask, bool)
    return mask & ~ndimage.binary_erosion(mask, _CROSS, border_value=0)


def edt_sq(feature):
    """Exact squared distance to the nearest True pixel of `feature`, int64 [H,W]."""
    feature = np.asarray(feature, bool)
    if not feature.any():
        return np.full(feature.shape, NO_FEATURE, np.int64)
    idx = ndimage.distance_transform_edt(~feature, return_distances=False, return_indices=True)
    yy, xx = np.indices(feature.shape)
    dy, dx = idx[0].astype(np.int64) - yy, idx[1].astype(np.int64) - xx
    return dy * dy + dx * dx


def edt_sq_brute(feature):
    feature = np.asarray(feature, bool)
    if not feature.any():
        return np.full(feature.shape, NO_FEATURE, np.int64)
    fy, fx = np.nonzero(feature)
    yy, xx = np.indices(feature.shape)
    d = (yy[..., None] - fy) ** 2 + (xx[..., None] - fx) ** 2
    return d.min(-1).astype(np.int64)


def distances_sq(P, T):
    """The multiset R as squared integers (unsorted): D_T at S(P), then D_P at S(T)."""
    sp, st = border(P), border(T)
    return np.concatenate([edt_sq(st)[sp], edt_sq(sp)[st]])


def image_metrics(P, T):
    P, T = np.asarray(P, bool), np.asarray(T, bool)
    sp, st = border(P), border(T)
    out = {"n_pred": int(P.sum()), "n_true": int(T.sum()), "n_inter": int((P & T).sum()), "n_union": int((P | T).sum()),
           "n_border_pred": int(sp.sum()), "n_border_true": int(st.sum())}
    if not P.any() and not T.any():
        out.update(n=0, max_d2=0, undefined=0, hd=0.0, hd95=0.0, assd=0.0, iou=1.0)
        return out
    if not P.any() or not T.any():
        out.update(n=0, max_d2=0, undefined=1, hd=float("nan"), hd95=float("nan"), assd=float("nan"), iou=0.0)
        return out
    d2 = distances_sq(P, T)
    r = np.sqrt(d2.astype(np.float64))
    out.update(n=int(d2.size), max_d2=int(d2.max()), undefined=0, hd=float(r.max()), hd95=float(np.percentile(r, 95)),
               assd=float(r.mean()), iou=out["n_inter"] / out["n_union"])
    return out


def set_metrics(per_image, spacing=1.0):
    """Set figures of a list of image_metrics dicts: distance means over the defined images, IoU over all of them."""
    ok = [m for m in per_image if not m["undefined"]]
    mean = lambda k: float(np.mean([m[k] for m in ok])) * spacing if ok else float("nan")   # noqa: E731
    return {"hd95": mean("hd95"), "hd": mean("hd"), "hd_max": max(m["hd"] for m in ok) * spacing if ok else float("nan"),
            "assd": mean("assd"), "iou": float(np.mean([m["iou"] for m in per_image])) if per_image else float("nan"),
            "n": len(per_image), "n_undefined": len(per_image) - len(ok)}


def blob_mask(rng, H, W, blobs=3, fill=0.25):
    """A random mask of a few filled ellipses (never empty: the first one is centred inside the image)."""
    yy, xx = np.indices((H, W))
    m = np.zeros((H, W), bool)
    for k in range(blobs):
        cy, cx = rng.uniform(0.2, 0.8) * H, rng.uniform(0.2, 0.8) * W
        ry, rx = max(1.0, rng.uniform(0.05, fill) * H), max(1.0, rng.uniform(0.05, fill) * W)
        m |= ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
    m[int(H * 0.5), int(W * 0.5)] = True
    return m
