"""The batch-invariant eval forward on the device: under the pinned plan (uh_conv3x3_fwd_affine_relu_plan with plan_B = 1,
uh_convt2x2_mfma_ok_plan, ops.plan_images(1)) an image of a batch gets, bit for bit, what it gets in a launch of its own -- at
the level of one layer, of the whole network (eager and graphed), of BatchPredictor, of ContourPipeline and of the predict
command line.  Every assertion is on bits of activations / logits; inputs and weights are seeded."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT

pytestmark = pytest.mark.gpu

BF16, F32 = 1, 0
SIZES = [(512, 512), (300, 700), (1000, 999)]
# (level, C0, C1, Cout) of every 3x3 conv of UNet(1, 3) and UNet_S(1, 3) (transposed-convolution up-sampling) whose contraction
# is long enough for the K split (256+ input channels)
LAYERS = [(2, 256, 0, 256), (2, 256, 256, 256), (3, 256, 0, 512), (3, 512, 0, 512), (3, 512, 512, 512), (4, 512, 0, 1024),
          (4, 1024, 0, 1024), (3, 128, 128, 128), (4, 256, 0, 256)]


def _lib():
    import unet_amd  # noqa: F401
    from unet_amd._lib import LIB
    LIB.load()
    return LIB


def _conv_shapes():
    """(h, w, C0, C1, Cout): every layer shape above that gets the K split (code 3) for ONE image at one of SIZES, plus one
    shape each whose single image gets 128-channel slabs (1), the register-resident filter (2) and the streaming form (4)."""
    lib = _lib()
    out = []
    for H, W in SIZES:
        for k, C0, C1, Cout in LAYERS:
            s = (H >> k, W >> k, C0, C1, Cout)
            if lib.query("uh_conv3x3_fwd_kernel", 1, s[0], s[1], C0, C1, Cout, BF16) == 3 and s not in out:
                out.append(s)
    # (256 x 256, 64 -> 128: the register-resident filter alone, 128-channel slabs from two images on)
    extra = [(368, 368, 64, 0, 128), (256, 256, 64, 0, 128), (64, 64, 128, 0, 128)]
    assert [lib.query("uh_conv3x3_fwd_kernel", 1, h, w, c0, c1, co, BF16) for h, w, c0, c1, co in extra] == [1, 2, 4]
    return out + extra


CONV_SHAPES = _conv_shapes()


def test_the_shape_list_covers_what_it_says():
    lib = _lib()
    codes = [lib.query("uh_conv3x3_fwd_kernel", 1, h, w, c0, c1, co, BF16) for h, w, c0, c1, co in CONV_SHAPES]
    assert codes.count(3) == len(CONV_SHAPES) - 3 >= 20 and set(codes) == {1, 2, 3, 4}
    assert any(c1 for _, _, _, c1, _ in CONV_SHAPES) and any(h % 16 or w % 16 for h, w, *_ in CONV_SHAPES)
    # pinned, the K split runs far past its own threshold of 256 (tile, slab) pairs
    assert max(8 * ((h + 15) // 16) * ((w + 15) // 16) * (co // 64) for (h, w, _, _, co), c in zip(CONV_SHAPES, codes) if c == 3) >= 2048


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    return torch.device("cuda:0")


class _Layer:
    """One eval-mode Conv -> scale/shift -> ReLU layer with seeded data (scale 1, shift 0: the conv itself meets the bound)."""

    def __init__(self, B, h, w, C0, C1, Cout, dtype, dev):
        from unet_amd import ops
        self.ops, self.dims, self.dtype, self.dev = ops, (h, w, C0, C1, Cout), dtype, dev
        Cin = C0 + C1
        g = torch.Generator().manual_seed(h * 1000 + w * 10 + Cin + Cout)
        x = torch.randn(B, h, w, Cin, generator=g)
        wt = torch.randn(Cout, Cin, 3, 3, generator=g) / (3.0 * Cin ** 0.5)
        if dtype == torch.bfloat16:          # compare like with like: the oracle sees the bf16-rounded operands
            x, wt = x.bfloat16().float(), wt.bfloat16().float()
        self.x = x.to(dev, dtype)
        self.w = wt.to(dev)
        self.packs = {False: ops.pack_w3x3(self.w, dtype, False)[0]}
        self.scale = torch.ones(Cout, device=dev)
        self.shift = torch.zeros(Cout, device=dev)
        self.dt = ops._dt(self.x)

    def run(self, lo, hi, plan=None):
        """Images lo..hi-1 in one launch: plan None = uh_conv3x3_fwd_affine_relu, else the pinned entry point."""
        ops = self.ops
        from unet_amd._lib import LIB, UH_WFRAG
        h, w, C0, C1, Cout = self.dims
        x = self.x[lo:hi]
        B = hi - lo
        x0 = x[..., :C0]
        x1 = x[..., C0:] if C1 else None
        ld = C0 + C1
        frag = ops.wfrag_ok(B, h, w, C0, C1, Cout, ld, ld if C1 else 0, Cout, self.dt, plan or 0)
        if frag and True not in self.packs:
            self.packs[True] = ops.pack_w3x3(self.w, self.dtype, False, frag_f=True)[0]
        z = torch.empty(B, h, w, Cout, dtype=self.dtype, device=self.dev)
        args = (x0.data_ptr(), C0, ld, ops._p(x1), C1, ld if C1 else 0, self.packs[frag].data_ptr(), z.data_ptr(), Cout, Cout,
                self.scale.data_ptr(), self.shift.data_ptr(), B)
        tail = (h, w, self.dt | (UH_WFRAG if frag else 0), ops._stream())
        if plan is None:
            LIB.call("uh_conv3x3_fwd_affine_relu", *args, *tail)
        else:
            LIB.call("uh_conv3x3_fwd_affine_relu_plan", *args, plan, *tail)
        return z

    def code(self, B, plan=0):
        h, w, C0, C1, Cout = self.dims
        return _lib().query("uh_conv3x3_fwd_kernel_plan", B, plan, h, w, C0, C1, Cout, self.dt)

    def fp64(self, i):
        """relu(conv) of image i in fp64 (im2col + one matrix product, on the device)."""
        h, w, C0, C1, Cout = self.dims
        cols = F.unfold(self.x[i:i + 1].permute(0, 3, 1, 2).double(), 3, padding=1)          # [1, Cin * 9, h * w]
        y = self.w.double().reshape(Cout, -1) @ cols[0]
        return y.clamp_(min=0).reshape(Cout, h, w).permute(1, 2, 0)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("h,w,C0,C1,Cout", CONV_SHAPES)
def test_pinned_conv_gives_every_image_its_own_bits(dtype, h, w, C0, C1, Cout):
    dev = _dev()
    B = 8
    L = _Layer(B, h, w, C0, C1, Cout, dtype, dev)
    one, got, own = L.code(1), L.code(B, 1), L.code(B)
    z = L.run(0, B, plan=1)
    err = ref_max = 0.0
    for i in range(B):
        alone = L.run(i, i + 1)
        assert torch.equal(z[i], alone[0]), f"image {i}: codes alone / pinned / unpinned = {one} / {got} / {own}"
        ref = L.fp64(i)
        err = max(err, float((z[i].double() - ref).abs().max()))
        ref_max = max(ref_max, float(ref.abs().max()))
    # the bound of tests/test_gpu_ops.py::test_conv3x3_k_split_inside_the_workgroup against fp64
    tol = 4e-5 if dtype == torch.float32 else 1e-2
    print(f"codes alone/pinned/unpinned {one}/{got}/{own}  rel err vs fp64 {err / ref_max:.3e} (bound {tol:g})")
    assert err / ref_max < tol, f"{err / ref_max:.3e}"
    # plan_B = 0 is the unpinned call
    assert torch.equal(L.run(0, B, plan=0), L.run(0, B))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("h,w,C0,C1,Cout", CONV_SHAPES)
def test_forms_of_one_summation_class_give_the_same_bits(dtype, h, w, C0, C1, Cout):
    """Image 0 through every form the plan can be made to choose: alone under plan lengths 1..64, and inside unpinned
    launches of 2, 4 and 8 images.  Forms the library exports as one class must agree to the bit; for the others the
    difference is printed (DESIGN.md section 3 records it) and nothing is asserted."""
    dev = _dev()
    lib = _lib()
    L = _Layer(8, h, w, C0, C1, Cout, dtype, dev)
    outs = {}
    for plan in (1, 2, 4, 8, 16, 64):
        outs.setdefault(L.code(1, plan), L.run(0, 1, plan=plan)[0])
    for B in (2, 4, 8):
        outs.setdefault(L.code(B), L.run(0, B)[0])
    codes = sorted(outs)
    for a in codes:
        for b in codes:
            if a < b:
                if lib.query("uh_conv3x3_fwd_sum_class", a) == lib.query("uh_conv3x3_fwd_sum_class", b):
                    assert torch.equal(outs[a], outs[b]), f"codes {a} and {b} are exported as one class"
                else:
                    d = (outs[a].float() - outs[b].float()).abs().max()
                    print(f"codes {a} vs {b}: max |diff| {float(d):.3e} of max {float(outs[a].float().abs().max()):.3e}")
    print(f"forms seen: {codes}")


# ------------------------------------------------------------------------------------------ transposed convolution
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("h,w,pad", [(62, 62, 0), (64, 64, 0), (37, 87, 1)])
def test_pinned_transposed_convolution(dtype, h, w, pad):
    """62 x 62: one image is not a multiple of 32 pixels, eight are -- pinned, the batch stays on the SIMT kernel; 64 x 64
    qualifies alone and keeps the MFMA GEMM.  pad: an odd skip size (F.pad of unet_parts.py:85-88)."""
    from unet_amd import ops
    dev = _dev()
    lib = _lib()
    B, Cin, Cout = 8, 128, 64
    Ho, Wo = 2 * h + pad, 2 * w + pad
    dt = BF16 if dtype == torch.bfloat16 else F32
    alone_choice = lib.query("uh_convt2x2_mfma_ok", 1, h, w, Cin, Cout, Ho, Wo, dt)
    assert lib.query("uh_convt2x2_mfma_ok_plan", B, 1, h, w, Cin, Cout, Ho, Wo, dt) == alone_choice
    assert alone_choice == (1 if (h * w) % (32 if dt == BF16 else 16) == 0 else 0)
    if (h, w) == (62, 62):
        assert lib.query("uh_convt2x2_mfma_ok", B, h, w, Cin, Cout, Ho, Wo, dt) == 1       # unpinned, the batch would change kernels
    g = torch.Generator().manual_seed(h + w)
    x = torch.randn(B, h, w, Cin, generator=g).to(dev, dtype)
    wt = (torch.randn(Cin, Cout, 2, 2, generator=g) / Cin ** 0.5).to(dev)
    bias = torch.randn(Cout, generator=g).to(dev)
    with torch.no_grad():
        with ops.plan_images(1):
            y = ops.ConvTranspose2x2PadFn.apply(x, wt, bias, Ho, Wo, False)
        for i in range(B):
            assert torch.equal(y[i], ops.ConvTranspose2x2PadFn.apply(x[i:i + 1], wt, bias, Ho, Wo, False)[0]), i
        # a training-mode call does not read the switch
        with ops.plan_images(1):
            yt = ops.ConvTranspose2x2PadFn.apply(x, wt, bias, Ho, Wo, True)
        assert torch.equal(yt, ops.ConvTranspose2x2PadFn.apply(x, wt, bias, Ho, Wo))


# ------------------------------------------------------------------------------------------ whole network
def _randomize_bn(model, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
                m.weight.copy_(torch.rand(m.num_features, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.num_features, generator=g) * 0.1)


def _model(arch, bilinear, dev, seed=7):
    import unet_amd
    torch.manual_seed(seed)
    model = getattr(unet_amd, arch)(1, 3, bilinear=bilinear)
    _randomize_bn(model, 21)
    return model.to(dev).eval()


def _fwd(model, x):
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        return model(x)


@pytest.mark.parametrize("H,W", [(512, 512), (512, 384), (300, 700), (1000, 999)])
@pytest.mark.parametrize("arch,bilinear", [("UNet", False), ("UNet", True), ("UNet_S", False), ("UNet_SA", False)])
def test_whole_network_logits_do_not_depend_on_the_batch(arch, bilinear, H, W):
    from unet_amd import ops
    from unet_amd.inference import GraphedForward
    dev = _dev()
    model = _model(arch, bilinear, dev)
    g = torch.Generator().manual_seed(H + W)
    x = torch.rand(8, 1, H, W, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
    alone = [_fwd(model, x[i:i + 1])[0].clone() for i in range(8)]
    assert all(bool(torch.isfinite(a).all()) for a in alone) and float(alone[0].float().std()) > 0
    for B in (3, 8):
        with ops.plan_images(1):
            eager = _fwd(model, x[:B])
        graphed = GraphedForward(model, x[:B], amp=True, plan_images=1)(x[:B])
        for i in range(B):
            assert torch.equal(eager[i], alone[i]), f"eager, batch {B}, image {i}"
            assert torch.equal(graphed[i], alone[i]), f"graphed, batch {B}, image {i}"
    assert ops.PLAN_IMAGES == 0


# ------------------------------------------------------------------------------------------ BatchPredictor
def _phantom(rng, H, W):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    img = rng.normal(20, 6, (H, W))
    cx, cy = W * rng.uniform(0.4, 0.6), H * rng.uniform(0.4, 0.6)
    rx, ry = W * rng.uniform(0.3, 0.4), H * rng.uniform(0.3, 0.4)
    body = ((xx - cx) / rx) ** 2 + ((yy - cy) / ry) ** 2 < 1
    img[body] = 110 + rng.normal(0, 8, int(body.sum()))
    img[((xx - cx) / (rx / 3)) ** 2 + ((yy - cy - ry / 3) / (ry / 4)) ** 2 < 1] += 90
    return np.clip(img, 0, 255).astype(np.uint8)


def _balance_head(model, img, dev):
    """Moves the head's bias by the mean logit of each class on one image, so that the three classes compete."""
    x = torch.from_numpy(img.astype(np.float32) / 255.0)[None, None].to(dev)
    with torch.no_grad():
        model.outc.conv.bias.sub_(model(x).float().mean(dim=(0, 2, 3)))


def _count_launches(p):
    calls = []
    inner = p._launch

    def wrapped(arrays, grey):
        calls.append(len(arrays))
        return inner(arrays, grey)

    p._launch = wrapped
    return calls


def test_batch_predictor_batch_invariant_runs_full_batches():
    import unet_amd
    from unet_amd.predict import plan_batches
    dev = _dev()
    model = _model("UNet", False, dev)
    rng = np.random.default_rng(5)
    images = [_phantom(rng, H, W) for (H, W), n in (((512, 512), 17), ((300, 180), 9), ((62 * 16, 64), 3)) for _ in range(n)]
    images = [images[i] for i in rng.permutation(len(images))]
    _balance_head(model, images[0], dev)
    planned = plan_batches([im.shape for im in images], 8)
    on = unet_amd.BatchPredictor(model, batch=8, postprocess=False, batch_invariant=True)
    off = unet_amd.BatchPredictor(model, batch=8, postprocess=False)
    calls_on, calls_off = _count_launches(on), _count_launches(off)
    got, want = on(images), off(images)
    assert any(len(np.unique(w)) == 3 for w in want), "a constant prediction compares nothing"
    for i, (a, b) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(a, b, err_msg=f"image {i} {images[i].shape}")
    # one launch per planned batch; the default mode cuts them (512 x 512: the full UNet runs one image per launch)
    assert calls_on == [len(m) for _, m in planned]
    assert off.launch_lengths(512, 512) == [1] and on.launch_lengths(512, 512) == list(range(1, 9))
    assert sum(calls_off) == len(images) and len(calls_off) >= 17 + 2 > len(calls_on)
    assert on.graph_replays > 0                    # 512 x 512 comes in two full batches: the second replays a graph
    again = on(images)
    for a, b in zip(again, want):
        np.testing.assert_array_equal(a, b)


# ------------------------------------------------------------------------------------------ ContourPipeline
def _raw_phantoms(rng, n, H, W):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.empty((n, H, W), np.uint16)
    for i in range(n):
        img = rng.normal(30, 8, (H, W))
        cx, cy = W * rng.uniform(0.4, 0.6), H * rng.uniform(0.4, 0.6)
        rx, ry = W * rng.uniform(0.25, 0.4), H * rng.uniform(0.25, 0.4)
        body = ((xx - cx) / rx) ** 2 + ((yy - cy) / ry) ** 2 < 1
        img[body] = 1000 + rng.normal(0, 10, (H, W))[body]
        img[((xx - cx) / (rx / 3)) ** 2 + ((yy - cy - ry / 3) / (ry / 4)) ** 2 < 1] += 600
        out[i] = np.clip(img, 0, 65535).astype(np.uint16)
    return out


def test_contour_pipeline_batch_invariant():
    import unet_amd
    dev = _dev()
    model = _model("UNet", False, dev, seed=3)
    raws = _raw_phantoms(np.random.default_rng(11), 8, 300, 400)
    big = unet_amd.ContourPipeline(model, 400, 300, 400, 1040, batch=8, batch_invariant=True)
    small = unet_amd.ContourPipeline(model, 400, 300, 400, 1040, batch=1, batch_invariant=True)
    out = big.run_batch(raws)
    assert big._graph is not None
    logits = out["logits"].clone()
    assert logits.shape[0] == 8 and float(logits.float().std()) > 0
    for i in range(8):
        o1 = small.run_batch(raws[i:i + 1])
        assert torch.equal(o1["logits"][0], logits[i]), f"image {i}"
        assert torch.equal(o1["grey"][0], out["grey"][i])
        assert [c.tolist() for c in o1["contours"][0]] == [c.tolist() for c in out["contours"][i]]


# ------------------------------------------------------------------------------------------ command line
def test_cli_writes_the_same_files_either_way(tmp_path):
    import unet_amd
    from PIL import Image
    dev = _dev()
    model = _model("UNet", False, dev, seed=5)
    _balance_head(model, _phantom(np.random.default_rng(1), 96, 128), dev)
    wpath = unet_amd.save_checkpoint(model.cpu(), str(tmp_path / "w.pth"), mask_values=[0, 128, 255])
    src = tmp_path / "in"
    os.makedirs(src)
    rng = np.random.default_rng(2)
    for k in range(11):
        H, W = ((96, 128), (80, 80), (70, 90))[k % 3]
        Image.fromarray(_phantom(rng, H, W)).save(src / f"im{k:02d}.png")
    outs = {}
    for name, flags in (("on", []), ("off", ["--no-batch-invariant"])):
        out = tmp_path / name
        r = subprocess.run([sys.executable, "-m", "unet_amd.predict", "-m", wpath, "-i", str(src), "-o", str(out), "--no-postprocess"]
                           + flags, capture_output=True, text=True, timeout=300, cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=ROOT))
        assert r.returncode == 0, r.stderr[-2000:]
        outs[name] = {f: open(out / f, "rb").read() for f in sorted(os.listdir(out))}
    assert sorted(outs["on"]) == [f"im{k:02d}.png" for k in range(11)]
    assert outs["on"] == outs["off"]
    assert any(len(np.unique(np.asarray(Image.open(tmp_path / "on" / f)))) == 3 for f in outs["on"])
