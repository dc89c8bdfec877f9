#!/usr/bin/env python3
"""Record what the pixel passes of the C ABI compute -- BatchNorm + ReLU apply / backward, the pool and head tails, max-pool,
bilinear x2, the 1x1 OutConv -- in every launch form their host side can choose: scalar, 16-byte channel groups with and
without hoisted coefficients, grids below and at the cap, every rung of the class / lanes-per-pixel ladder.
tests/test_gpu_pixel_pass_forms.py replays the same cases (it imports CASES / run_case from this file) and requires the sha256
digests of tests/golden/pixel_pass_forms_parent.json.

Only C-ABI entry points are called, on seeded inputs; every output is digested, for the reduce entry points the partial rows
and the per-channel sums behind them.  Needs an MI355X.  To renew the fixture, at the commit whose behaviour is to be kept:

    python tests/golden/make_pixel_pass_forms.py record run1.json
    python tests/golden/make_pixel_pass_forms.py record run2.json
    python tests/golden/make_pixel_pass_forms.py merge run1.json run2.json tests/golden/pixel_pass_forms_parent.json

`merge` refuses two runs that differ in their cases, in the names of their digests or in the digest of an element-wise
output; of the reduced outputs (partial rows, per-channel and filter sums) it keeps the digests both runs agree on and names
the rest under "dropped_digests"."""
import contextlib
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

F32, BF16 = 0, 1
CAP, CAP_1X1 = 4096, 8192                       # workgroups: the BatchNorm / pool / upsample passes, the 1x1 conv
B, H, W = 2, 6, 10                              # the small extent: 120 pixels, 30 windows
# outputs behind a reduction: merge may drop one of these where two runs disagree, never an element-wise output
REDUCED = ("partials", "dgamma", "dbeta", "dhead_w", "dhead_b", "c11_dw", "c11_dbias")


def _vec(dt):
    return 8 if dt == BF16 else 4


def _name(dt):
    return "bf16" if dt == BF16 else "fp32"


class Call:
    """Seeded device tensors and LIB.call on the current stream."""

    def __init__(self, dt, seed):
        from unet_amd._lib import LIB
        self.lib, self.dt, self.seed = LIB, dt, seed
        self.dev = torch.device("cuda:0")
        self.tt = torch.bfloat16 if dt == BF16 else torch.float32
        self.st = torch.cuda.current_stream().cuda_stream

    def vals(self, n, lo=-1.0, hi=1.0, dtype=None, off=0):
        """n values in [lo, hi) from an integer hash of (seed, draw, index): the same on every machine.  off: the tensor
        starts `off` elements behind a 16-byte boundary."""
        self.seed += 1
        i = torch.arange(n, device=self.dev, dtype=torch.int64)
        h = ((i % 65521) ** 2 * 31 + i * 2654435761 + self.seed * 40503) % 65521
        v = (h.to(torch.float32) / 65521.0) * (hi - lo) + lo
        out = self.empty(n, dtype, off)
        out.copy_(v)
        return out

    def empty(self, n, dtype=None, off=0):
        buf = torch.zeros(n + off, device=self.dev, dtype=dtype or self.tt)
        return buf[off:]

    def f32(self, n, lo=-1.0, hi=1.0):
        return self.vals(n, lo, hi, torch.float32)

    def coeffs(self, C):
        """scale, shift, mean, rstd"""
        return self.f32(C, 0.5, 1.5), self.f32(C, -0.3, 0.3), self.f32(C, -0.2, 0.2), self.f32(C, 0.5, 1.5)

    def call(self, name, *args):
        self.lib.call(name, *[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args], self.dt, self.st)

    def nblk(self, npix, C):
        return self.lib.query("uh_bn_bwd_nblk", npix, C)


@contextlib.contextmanager
def _env(key, value):
    before = os.environ.get(key)
    os.environ[key] = value
    try:
        yield
    finally:
        if before is None:
            os.environ.pop(key, None)
        else:
            os.environ[key] = before


def _bn_bwd(c, res, tag, dz, y, co, n, C, out_off=0):
    """uh_bn_relu_bwd_reduce / uh_bn_bwd_finalize / uh_bn_relu_bwd_apply, the last one also in its SyncBN form."""
    scale, shift, mean, rstd = co
    nblk = c.nblk(n, C)
    part, dg, db, dg2, db2 = c.empty(nblk * 2 * C, torch.float32), *(c.empty(C, torch.float32) for _ in range(4))
    dy, dy2 = c.empty(n * C, off=out_off), c.empty(n * C, off=out_off)
    c.call("uh_bn_relu_bwd_reduce", dz, C, y, C, scale, shift, mean, rstd, part, n, C)
    c.lib.call("uh_bn_bwd_finalize", part.data_ptr(), nblk, C, dg2.data_ptr(), db2.data_ptr(), c.st)
    c.call("uh_bn_relu_bwd_apply", dz, C, y, C, scale, shift, mean, rstd, part, nblk, dg, db, dy, C, n, 0, C)
    c.call("uh_bn_relu_bwd_apply", dz, C, y, C, scale, shift, mean, rstd, None, 0, dg, db, dy2, C, n, 2 * n, C)
    res.update({tag + "partials": part, tag + "fin.dgamma": dg2, tag + "fin.dbeta": db2, tag + "dgamma": dg, tag + "dbeta": db,
                tag + "dy": dy, tag + "dy_ntotal": dy2})


def case_flat(C, dt, out_off=0):
    """BatchNorm apply / backward, max-pool, bilinear x2 and the 1x1 backward-data on 120 pixels.  out_off: the OUTPUT of every
    call starts that many elements behind a 16-byte boundary (the scalar form of a channel count that has a vector form)."""
    c = Call(dt, 100 * C + dt)
    n, res = B * H * W, {}
    y, dz, co = c.vals(n * C), c.vals(n * C), c.coeffs(C)
    z = c.empty(n * C, off=out_off)
    c.call("uh_bn_relu_apply", y, C, co[0], co[1], z, C, n, C)
    res["z"] = z
    _bn_bwd(c, res, "bn.", dz, y, co, n, C, out_off)
    # max-pool of z, its backward with and without a skip gradient
    nw = n // 4
    pooled, dpool, dskip = c.empty(nw * C, off=out_off), c.vals(nw * C), c.vals(n * C)
    dx, dx0 = c.empty(n * C, off=out_off), c.empty(n * C, off=out_off)
    c.call("uh_maxpool2_fwd", z, C, pooled, C, B, H, W, C)
    c.call("uh_maxpool2_bwd", z, C, dpool, C, dskip, C, dx, C, B, H, W, C)
    c.call("uh_maxpool2_bwd", z, C, dpool, C, None, 0, dx0, C, B, H, W, C)
    res.update({"pooled": pooled, "pool_dx": dx, "pool_dx_noskip": dx0})
    # bilinear x2 into 13 x 21 (one padding row on top, one padding column on the right), alone and behind BatchNorm + ReLU
    Ho, Wo, pt, pl = 2 * H + 1, 2 * W + 1, 1, 0
    no = B * Ho * Wo
    up, dup, up_dx, up_dx_ptr, up_dx_h1 = c.empty(no * C, off=out_off), c.vals(no * C), *(c.empty(n * C, off=out_off) for _ in range(3))
    c.call("uh_upsample2x_fwd", z, C, up, C, B, H, W, C, Ho, Wo, pt, pl)
    res["up"] = up
    if C % _vec(dt) == 0 and not out_off:
        bn_up = c.empty(no * C)
        c.call("uh_bn_relu_upsample2x_fwd", y, C, co[0], co[1], bn_up, C, B, H, W, C, Ho, Wo, pt, pl)
        res["bn_up"] = bn_up
    c.call("uh_upsample2x_bwd", dup, C, up_dx, C, B, H, W, C, Ho, Wo, pt, pl)
    with _env("UH_UP_BWD_PTR", "1"):             # the pointer form of the strip kernel
        c.call("uh_upsample2x_bwd", dup, C, up_dx_ptr, C, B, H, W, C, Ho, Wo, pt, pl)
    c.call("uh_upsample2x_bwd", dup, C, up_dx_h1, C, B * H, 1, W, C, 2, 2 * W, 0, 0)      # one-row maps: the gather kernel
    res.update({"up_dx": up_dx, "up_dx_ptr": up_dx_ptr, "up_dx_h1": up_dx_h1})
    ncls = 3
    dl, w, c11_dx = c.f32(n * ncls), c.f32(ncls * C), c.empty(n * C, off=out_off)
    c.call("uh_conv1x1_dgrad", dl, w, c11_dx, C, n, C, ncls)
    res["c11_dx"] = c11_dx
    return res


def _pool_tail(c, res, tag, Bc, Hc, Wc, C, y, co, dskip, dpool, reduce=True):
    scale, shift, mean, rstd = co
    n = Bc * Hc * Wc
    sk = (dskip, C if dskip is not None else 0, dpool, C)
    dg, db, dy = c.empty(C, torch.float32), c.empty(C, torch.float32), c.empty(n * C)
    if reduce:
        nblk = c.nblk(n, C)
        part = c.empty(nblk * 2 * C, torch.float32)
        c.call("uh_bn_relu_pool_bwd_reduce", *sk, y, C, scale, shift, mean, rstd, part, Bc, Hc, Wc, C)
        res[tag + "partials"] = part
    else:                                        # the SyncBN form: the sums are given
        nblk, part = 0, None
        dg.copy_(c.f32(C))
        db.copy_(c.f32(C))
    c.call("uh_bn_relu_pool_bwd_apply", *sk, y, C, scale, shift, mean, rstd, part, nblk, dg, db, dy, C, Bc, Hc, Wc, 0, C)
    res.update({tag + "dgamma": dg, tag + "dbeta": db, tag + "dy": dy})


def case_pool(C, dt):
    """The pool tail on 30 windows: vector form only."""
    c = Call(dt, 200 * C + dt)
    n, res = B * H * W, {}
    y, co, dskip, dpool = c.vals(n * C), c.coeffs(C), c.vals(n * C), c.vals(n // 4 * C)
    z, pooled = c.empty(n * C), c.empty(n // 4 * C)
    c.call("uh_bn_relu_pool_apply", y, C, co[0], co[1], z, C, pooled, C, B, H, W, C)
    res.update({"z": z, "pooled": pooled})
    _pool_tail(c, res, "skip.", B, H, W, C, y, co, dskip, dpool)
    _pool_tail(c, res, "noskip.", B, H, W, C, y, co, None, dpool)
    return res


def _c11(c, res, n, C, ncls, x, w, b, dl):
    lg, dw, dbias = c.empty(n * ncls, torch.float32), c.empty(ncls * C, torch.float32), c.empty(ncls, torch.float32)
    wsb = c.lib.query("uh_conv1x1_wgrad_ws_bytes", n, C, ncls)
    ws = c.empty(wsb // 4 + 1, torch.float32)
    c.call("uh_conv1x1_fwd", x, C, w, b, lg, n, C, ncls)
    c.call("uh_conv1x1_wgrad", dl, x, C, dw, dbias, ws, wsb, n, C, ncls)
    res.update({"c11_logits": lg, "c11_dw": dw, "c11_dbias": dbias})


def case_head(lpp, ncls, dt):
    """The head tail and the 1x1 forward / weight gradient on 120 pixels: C = lpp 16-byte groups."""
    C = lpp * _vec(dt)
    c = Call(dt, 1000 * lpp + 10 * ncls + dt)
    n, res = B * H * W, {}
    y, co, w, b, dl = c.vals(n * C), c.coeffs(C), c.f32(ncls * C), c.f32(ncls), c.f32(n * ncls)
    scale, shift, mean, rstd = co
    lg = c.empty(n * ncls, torch.float32)
    c.call("uh_bn_relu_head_fwd", y, C, scale, shift, w, b, lg, n, C, ncls)
    nblk = c.nblk(n, C)
    wsb = c.lib.query("uh_bn_relu_head_bwd_ws_bytes", n, C, ncls)
    part, ws = c.empty(nblk * 2 * C, torch.float32), c.empty(wsb // 4 + 1, torch.float32)
    dhw, dhb, dg, db, dy = c.empty(ncls * C, torch.float32), c.empty(ncls, torch.float32), c.empty(C, torch.float32), c.empty(C, torch.float32), c.empty(n * C)
    c.call("uh_bn_relu_head_bwd_reduce", dl, w, y, C, scale, shift, mean, rstd, part, dhw, dhb, ws, wsb, n, C, ncls)
    c.call("uh_bn_relu_head_bwd_apply", dl, w, y, C, scale, shift, mean, rstd, part, nblk, dg, db, dy, C, n, 0, C, ncls)
    res.update({"logits": lg, "partials": part, "dhead_w": dhw, "dhead_b": dhb, "dgamma": dg, "dbeta": db, "dy": dy})
    _c11(c, res, n, C, ncls, y, w, b, dl)
    return res


def case_c11(C, ncls, dt):
    """The 1x1 conv alone: class counts and channel counts outside the head shape."""
    c = Call(dt, 3000 + 10 * C + ncls + 5 * dt)
    n, res = B * H * W, {}
    _c11(c, res, n, C, ncls, c.vals(n * C), c.f32(ncls * C), c.f32(ncls), c.f32(n * ncls))
    return res


def case_capped(Bc, Hc, Wc, C, dt=BF16):
    """More channel groups than 4096 workgroups of 256 threads: the grid-stride walk of the BatchNorm passes, and the pool tail
    of the same extent."""
    c = Call(dt, Hc + Wc + C)
    n, res = Bc * Hc * Wc, {}
    y, dz, co, dpool = c.vals(n * C), c.vals(n * C), c.coeffs(C), c.vals(n // 4 * C)
    z, z2, pooled = c.empty(n * C), c.empty(n * C), c.empty(n // 4 * C)
    c.call("uh_bn_relu_apply", y, C, co[0], co[1], z, C, n, C)
    _bn_bwd(c, res, "bn.", dz, y, co, n, C)
    c.call("uh_bn_relu_pool_apply", y, C, co[0], co[1], z2, C, pooled, C, Bc, Hc, Wc, C)
    res.update({"z": z, "pool.z": z2, "pool.pooled": pooled})
    _pool_tail(c, res, "pool.", Bc, Hc, Wc, C, y, co, dz, dpool)
    return res


def case_capped_pool(Bc, Hc, Wc, C, dt=BF16):
    """The pool tail where the WINDOWS outnumber the capped grid's threads."""
    c = Call(dt, Hc + Wc + C + 1)
    n, res = Bc * Hc * Wc, {}
    y, co, dskip, dpool = c.vals(n * C), c.coeffs(C), c.vals(n * C), c.vals(n // 4 * C)
    z, pooled = c.empty(n * C), c.empty(n // 4 * C)
    c.call("uh_bn_relu_pool_apply", y, C, co[0], co[1], z, C, pooled, C, Bc, Hc, Wc, C)
    res.update({"z": z, "pooled": pooled})
    _pool_tail(c, res, "", Bc, Hc, Wc, C, y, co, dskip, dpool, reduce=False)
    return res


def _plan(items, C, dt, form, aligned=1, cap=CAP):
    """What uh_pixel_pass_plan must answer for a call of the case: form = scalar | hoist | vector (no hoist), + "_capped" where the
    grid is the cap."""
    return {"items": items, "C": C, "dt": dt, "aligned": aligned, "cap": cap, "form": form}


def _cases():
    """name -> (function, arguments, the plans the case must take)"""
    n, nw = B * H * W, B * H * W // 4
    # the forms by the rules the entry points held before they shared one plan: 16-byte groups where C is a multiple of 8 bf16 / 4
    # fp32; hoisted coefficients where 256 x workgroups is a multiple of the group count
    flat = {(3, BF16): ("scalar", "scalar"), (12, BF16): ("scalar", "scalar"), (24, BF16): ("vector", "vector"),
            (64, BF16): ("hoist", "hoist"), (3, F32): ("scalar", "scalar"), (12, F32): ("vector", "vector"),
            (24, F32): ("hoist", "vector"), (64, F32): ("hoist", "hoist")}          # at 120 pixels, at 30 windows
    pool = {(24, BF16): "vector", (64, BF16): "hoist", (24, F32): "vector", (64, F32): "hoist"}
    cases = {}
    for (C, dt), (at_n, at_nw) in flat.items():
        cases[f"flat.{_name(dt)}.c{C}"] = (case_flat, (C, dt), [_plan(n, C, dt, at_n), _plan(nw, C, dt, at_nw),
                                                               _plan(n, C, dt, at_n, cap=CAP_1X1)])
    cases["flat.bf16.c64.unaligned"] = (case_flat, (64, BF16, 1), [_plan(n, 64, BF16, "scalar", aligned=0)])
    for (C, dt), form in pool.items():
        cases[f"pool.{_name(dt)}.c{C}"] = (case_pool, (C, dt), [_plan(nw, C, dt, form)])
    for dt in (BF16, F32):
        for lpp in (8, 16):
            for ncls in (1, 3, 4):
                cases[f"head.{_name(dt)}.lpp{lpp}.ncls{ncls}"] = (case_head, (lpp, ncls, dt), [])
        for C, ncls in ((8 * _vec(dt), 8), (24, 3), (24, 5), (3, 2)):
            cases[f"c11.{_name(dt)}.c{C}.ncls{ncls}"] = (case_c11, (C, ncls, dt), [])
    # 360 448 pixels x 3 groups > 4096 x 256 threads and 1 048 576 mod 3 != 0: a thread changes its channel group as it strides
    # (the windows of this extent, a quarter as many, still fit below the cap: one group per thread, hoisted)
    cases["capped.c24"] = (case_capped, (2, 512, 352, 24), [_plan(2 * 512 * 352, 24, BF16, "vector_capped"),
                                                            _plan(2 * 512 * 352 // 4, 24, BF16, "hoist")])
    # 139 264 pixels x 8 groups: capped, and a thread keeps its group
    cases["capped.c64"] = (case_capped, (2, 256, 272, 64), [_plan(2 * 256 * 272, 64, BF16, "hoist_capped"),
                                                            _plan(2 * 256 * 272 // 4, 64, BF16, "hoist")])
    # ... and the pool tail at four times the extent, where its windows are what the pixels are above
    cases["capped_pool.c24"] = (case_capped_pool, (2, 1024, 704, 24), [_plan(2 * 1024 * 704 // 4, 24, BF16, "vector_capped")])
    return cases


CASES = _cases()


def digest(t):
    raw = t.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()
    return hashlib.sha256(raw).hexdigest()


def run_case(name):
    """-> {result name: sha256}"""
    fn, args, _ = CASES[name]
    res = fn(*args)
    torch.cuda.synchronize()
    return {k: digest(v) for k, v in sorted(res.items())}


def reduced(key):
    return key.rsplit(".", 1)[-1] in REDUCED


def dump(doc, path):
    """Compact: one line per case."""
    with open(path, "w") as f:
        f.write('{"dropped_digests": %s, "cases": {\n' % json.dumps(doc.get("dropped_digests", [])))
        f.write(",\n".join('"%s": %s' % (name, json.dumps(d, separators=(",", ":"))) for name, d in doc["cases"].items()))
        f.write("\n}}\n")


def main(argv):
    if argv and argv[0] == "record":
        import time
        doc = {"cases": {}}
        for name in CASES:
            t0 = time.time()
            doc["cases"][name] = run_case(name)
            print(f"case {name}: {len(doc['cases'][name])} digests, {time.time() - t0:.2f} s", flush=True)
        dump(doc, argv[1])
    elif argv and argv[0] == "merge":
        a, b = (json.load(open(p)) for p in argv[1:3])
        if list(a["cases"]) != list(b["cases"]):
            raise SystemExit("the two runs hold different cases")
        dropped = []
        for name, da in a["cases"].items():
            db = b["cases"][name]
            if sorted(da) != sorted(db):
                raise SystemExit(f"case {name}: the two runs digested different results")
            for k in list(da):
                if da[k] != db[k]:
                    if not reduced(k):
                        raise SystemExit(f"case {name}: the element-wise output {k} differs between the two runs")
                    dropped.append(f"{name}:{k}")
                    del da[k]
        a["dropped_digests"] = dropped
        dump(a, argv[3])
        print(f"merged: {sum(len(d) for d in a['cases'].values())} digests in {len(a['cases'])} cases, dropped digests: {dropped}")
    else:
        raise SystemExit(__doc__)


if __name__ == "__main__":
    main(sys.argv[1:])
