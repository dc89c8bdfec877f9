"""Op-level GPU parity (through the C ABI wrappers in ops.py) against fp64 stock-PyTorch CPU maths:
conv3x3 forward / backward-data / backward-weights over a sweep of shapes that exercise every kernel
variant (MFMA NB=2/4, stem, generic; two-source inputs; partial tiles; odd sizes).  The bounds here are fractions of a tensor's
largest value on Gaussian inputs; test_gpu_exact.py holds each kernel form and backward-weights plan, one asserted case per
answer of uh_conv3x3_fwd_kernel / uh_conv3x3_wgrad_plan, to the float64 reference bit for bit on integer inputs."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    return torch.device("cuda:0")


def _nhwc(t, dtype, dev):
    return t.permute(0, 2, 3, 1).contiguous().to(dev, dtype)


SHAPES = [
    # B, H, W, C0, C1, Cout
    (2, 32, 32, 64, 0, 128),
    (2, 64, 64, 64, 0, 64),
    (1, 16, 16, 128, 0, 256),
    (2, 17, 23, 64, 64, 64),
    (1, 40, 24, 128, 128, 128),
    (2, 8, 8, 512, 0, 512),
    (3, 19, 33, 1, 0, 64),
    (2, 20, 20, 3, 0, 64),
    (2, 12, 14, 8, 8, 16),
    (1, 4, 4, 64, 0, 128),
    (2, 2, 2, 128, 0, 128),
]


# More tiles than persistent workgroups (768 for 64-channel slabs, 512 for 128-channel ones; backward-weights: 512 pixel
# ranges): every workgroup walks SEVERAL tiles, Chan-merges its BatchNorm moments across them and prefetches the next
# tile's halo under the last K-chunk -- the code path bench.py times at 512x512.
SHAPES_MULTITILE = [
    (1, 448, 448, 64, 0, 64),        # 784 tiles > 768 workgroups (NBW = 1), 2 K-chunks per tile
    (2, 320, 336, 64, 0, 128),       # 840 tiles x 1 slab > 512 workgroups (NBW = 2)
    (1, 448, 448, 64, 64, 64),       # two-source K loop across tiles (the decoder's virtual concat)
    (3, 250, 333, 128, 0, 64),       # odd sizes: partial tiles on both edges, 1008 tiles
    (4, 320, 320, 64, 0, 64),        # 1 600 tiles on 512 workgroups of the register-resident-filter form: 3-4 tiles each, so its
                                     # three halo buffers (the DMA a whole tile ahead) go round more than once
    (2, 333, 250, 64, 0, 64),        # the same with partial tiles on both edges (672 tiles: 1-2 each, border and interior mixed)
]


# Deep K and many tiles at once: the 1024- and 2048-channel two-source K loops of up1.0 (config 2)
# and of config 4's up1 on maps large enough that every persistent workgroup walks several tiles -- 32 / 64 K-chunks per
# tile with the double-buffered halo DMA wrapping from the last chunk of one tile to chunk 0 of the next, and
# backward-weights with its pixel-range split over (Cin/64) x (Cout/128) channel tiles.
SHAPES_DEEPK_MULTITILE = [
    (1, 160, 160, 512, 512, 512),    # K = 9 216 (up1.0): 100 tiles x 4 slabs
    (1, 96, 96, 1024, 1024, 1024),   # K = 18 432 (config 4's up1 at reduced extent): 36 tiles x 8 slabs
]


# Few tiles, long contraction (the 32 x 32 level of a small batch): in bf16 the forward / backward-data kernel splits the K-chunks
# over the two halves of an 8-wave workgroup (KS = 2) and adds the two accumulator sets in LDS; fp32 takes the ordinary form.
SHAPES_KSPLIT = [
    (4, 32, 32, 512, 0, 512),        # down4 at BASELINE config 3's 4 images per GPU: 16 tiles x 8 slabs, 16 chunks
    (8, 32, 32, 512, 0, 512),        # ... and at config 2's batch: 256 workgroups, the limit
    (2, 20, 37, 256, 256, 128),      # two sources, partial tiles on both edges
    (1, 16, 16, 1024, 0, 64),        # 32 chunks, one tile, one slab
    (3, 16, 16, 320, 0, 64),         # 10 chunks (5 + 5)
    (1, 16, 16, 288, 0, 64),         # 9 chunks: odd, stays unsplit
]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,H,W,C0,C1,Cout", SHAPES_KSPLIT)
def test_conv3x3_k_split_inside_the_workgroup(dtype, B, H, W, C0, C1, Cout):
    _conv_case(dtype, B, H, W, C0, C1, Cout, tol_f32=4e-5)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,H,W,C0,C1,Cout", SHAPES_MULTITILE)
def test_conv3x3_multitile_fwd_stats_dgrad_wgrad(dtype, B, H, W, C0, C1, Cout):
    _conv_case(dtype, B, H, W, C0, C1, Cout)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,H,W,C0,C1,Cout", SHAPES_DEEPK_MULTITILE)
def test_conv3x3_deep_k_multitile_fwd_stats_dgrad_wgrad(dtype, B, H, W, C0, C1, Cout):
    # fp32 accumulation over K = 9 216 / 18 432 products against fp64: the round-off bound grows like sqrt(K)
    _conv_case(dtype, B, H, W, C0, C1, Cout, tol_f32=6e-5)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,H,W,C0,C1,Cout", SHAPES)
def test_conv3x3_fwd_dgrad_wgrad(dtype, B, H, W, C0, C1, Cout):
    _conv_case(dtype, B, H, W, C0, C1, Cout)


def _conv_case(dtype, B, H, W, C0, C1, Cout, tol_f32=2e-5):
    from unet_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(B * 1000 + H * 10 + C0 + Cout)
    Cin = C0 + C1
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (3.0 * Cin ** 0.5)
    dy = torch.randn(B, Cout, H, W, generator=g)
    if dtype == torch.bfloat16:          # compare like with like: the oracle sees the bf16-rounded operands
        x, w, dy = x.bfloat16().float(), w.bfloat16().float(), dy.bfloat16().float()
    xd = x.double().requires_grad_(True)
    wd = w.double().requires_grad_(True)
    yref = F.conv2d(xd, wd, padding=1)
    dxref, dwref = torch.autograd.grad(yref, [xd, wd], dy.double())

    xg = _nhwc(x, dtype, dev)
    x0 = xg[..., :C0]
    x1 = xg[..., C0:] if C1 else None
    wf, wdg = ops.pack_w3x3(w.to(dev), dtype, True)
    y, stats, nslab = ops.conv3x3_fwd(x0, x1, wf, Cout, True)
    tol = tol_f32 if dtype == torch.float32 else 1e-2
    # fragment-major filter packs (UH_WFRAG), wherever the LDS-DMA MFMA kernel takes the call: bit-identical results
    dtc = ops._dt(xg)
    ok_f = ops.wfrag_ok(B, H, W, C0, C1, Cout, ops.pixel_ld(x0), 0 if x1 is None else ops.pixel_ld(x1), Cout, dtc)
    ok_d = ops.wfrag_ok(B, H, W, Cout, 0, Cin, Cout, 0, Cin, dtc)
    if ok_f or ok_d:
        wf2, wd2 = ops.pack_w3x3(w.to(dev), dtype, True, None, ok_f, ok_d)
        if ok_f:
            y2, st2, _ = ops.conv3x3_fwd(x0, x1, wf2, Cout, True, None, True)
            assert torch.equal(y2, y)
            c1, c2 = stats[nslab * 2 * Cout:nslab * 2 * Cout + nslab], st2[nslab * 2 * Cout:nslab * 2 * Cout + nslab]
            assert torch.equal(c1, c2)                  # pixel counts; rows with a zero count hold nothing
            live = c1 > 0
            assert torch.equal(st2[:nslab * 2 * Cout].view(nslab, 2 * Cout)[live], stats[:nslab * 2 * Cout].view(nslab, 2 * Cout)[live])
        if ok_d:
            dyg_ = _nhwc(dy, dtype, dev)
            dxa, _, _ = ops.conv3x3_fwd(dyg_, None, wdg, Cin, False)
            dxb, _, _ = ops.conv3x3_fwd(dyg_, None, wd2, Cin, False, None, True)
            assert torch.equal(dxa, dxb)

    def rel(a, b):
        return float((a.double().cpu() - b).abs().max() / b.abs().max())

    yn = y.permute(0, 3, 1, 2)
    assert rel(yn, yref.detach()) < tol, f"fwd {rel(yn, yref.detach()):.3e}"
    # BatchNorm statistics from the conv epilogue: per-slab (mean, M2) of the STORED y + pixel counts
    st = stats[:nslab * 2 * Cout].view(nslab, 2, Cout).double().cpu()
    cnt = stats[nslab * 2 * Cout:nslab * 2 * Cout + nslab].double().cpu()
    assert float(cnt.sum()) == B * H * W
    live = cnt > 0                      # a kernel may use fewer slabs than the buffer holds: zero-count rows are unused
    st, cnt = st[live], cnt[live]
    ys = y.double().cpu().reshape(-1, Cout)
    mean = (st[:, 0] * cnt[:, None]).sum(0) / cnt.sum()
    m2 = (st[:, 1] + cnt[:, None] * (st[:, 0] - mean[None]) ** 2).sum(0)
    assert float((mean - ys.mean(0)).abs().max()) <= 1e-5 * float(ys.abs().max()) + 1e-7
    assert float((m2 - ((ys - ys.mean(0)) ** 2).sum(0)).abs().max()) <= 1e-4 * float(((ys - ys.mean(0)) ** 2).sum(0).max())

    dyg = _nhwc(dy, dtype, dev)
    dx, _, _ = ops.conv3x3_fwd(dyg, None, wdg, Cin, False)
    assert rel(dx.permute(0, 3, 1, 2), dxref) < tol, f"dgrad {rel(dx.permute(0, 3, 1, 2), dxref):.3e}"

    dwk = torch.empty(Cout * 9 * Cin, dtype=torch.float32, device=dev)
    ops.conv3x3_wgrad(dyg, x0, x1, dwk)
    dwn = dwk.view(Cout, 3, 3, Cin).permute(0, 3, 1, 2)
    assert rel(dwn, dwref) < _wgrad_tol(dtype), f"wgrad {rel(dwn, dwref):.3e}"


def _wgrad_tol(dtype):
    # inputs are exact in both; fp32: only the accumulation order differs.  bf16: the per-split partial sums travel to the reduce
    # kernel as block-scaled fp16 (conv3x3_wgrad_mfma_v2<.., SLAB16>: 2^-12 per partial) and are added in fp32; the reference's
    # autocast backward rounds the TOTAL to bf16, 2^-9 = 2e-3 of each element
    return 2e-5 if dtype == torch.float32 else 1e-3


# One smallest shape per backward-weights kernel (the codes of uh_conv3x3_wgrad_plan; code 4 on bf16, a tensor past 2 GiB, is
# test_gpu_large.py's)
WGRAD_PLAN_CASES = [
    pytest.param(0, torch.bfloat16, (2, 12, 14, 8, 8, 16), id="0-generic-bf16"),
    pytest.param(0, torch.float32, (2, 12, 14, 8, 8, 16), id="0-generic-fp32"),
    pytest.param(1, torch.float32, (2, 20, 20, 3, 0, 6), id="1-stem-fp32"),
    pytest.param(2, torch.float32, (2, 20, 20, 3, 0, 64), id="2-stem_v2-fp32"),
    pytest.param(3, torch.bfloat16, (3, 19, 33, 1, 0, 64), id="3-stem_v3-bf16"),
    pytest.param(4, torch.float32, (2, 17, 23, 64, 64, 64), id="4-mfma-fp32"),
    pytest.param(5, torch.bfloat16, (2, 17, 23, 64, 64, 64), id="5-dma64-bf16"),
    pytest.param(6, torch.bfloat16, (1, 16, 16, 128, 0, 256), id="6-dma128-bf16"),
]


@pytest.mark.parametrize("code,dtype,shape", WGRAD_PLAN_CASES)
def test_conv3x3_wgrad_takes_the_planned_kernel_and_defers_to_the_same_bits(code, dtype, shape):
    """uh_conv3x3_wgrad_plan names the kernel; uh_conv3x3_wgrad meets the float64 gradient within _conv_case's bounds; and, where
    the kernel leaves slabs, uh_conv3x3_wgrad_partials + uh_slab_reduce_batched give the bits of the call that reduces at once."""
    import ctypes
    from unet_amd import ops
    from unet_amd._lib import LIB
    dev = _dev()
    B, H, W, C0, C1, Cout = shape
    Cin = C0 + C1
    g = torch.Generator().manual_seed(B * 1000 + H * 10 + C0 + Cout)
    x = torch.randn(B, Cin, H, W, generator=g)
    dy = torch.randn(B, Cout, H, W, generator=g)
    if dtype == torch.bfloat16:
        x, dy = x.bfloat16().float(), dy.bfloat16().float()
    wd = torch.zeros(Cout, Cin, 3, 3, dtype=torch.float64, requires_grad=True)
    (dwref,) = torch.autograd.grad(F.conv2d(x.double(), wd, padding=1), [wd], dy.double())
    x0 = _nhwc(x[:, :C0], dtype, dev)                            # dense pitches, as the query assumes
    x1 = _nhwc(x[:, C0:], dtype, dev) if C1 else None
    dyg = _nhwc(dy, dtype, dev)
    dt = ops._dt(dyg)
    plan = (ctypes.c_int64 * 8)()
    LIB.call("uh_conv3x3_wgrad_plan", B, H, W, C0, C1, Cout, dt, 0, ctypes.addressof(plan))
    assert plan[0] == code, list(plan)

    dwk = torch.empty(Cout * 9 * Cin, dtype=torch.float32, device=dev)
    ops.conv3x3_wgrad(dyg, x0, x1, dwk)
    err = float((dwk.view(Cout, 3, 3, Cin).permute(0, 3, 1, 2).double().cpu() - dwref).abs().max() / dwref.abs().max())
    assert err < _wgrad_tol(dtype), f"wgrad {err:.3e}"
    if plan[1] == 0:
        return                                                   # no slabs, nothing to defer
    nbytes = LIB.query("uh_conv3x3_wgrad_ws_bytes", B, H, W, Cin, Cout, dt)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    dw2 = torch.full_like(dwk, float("nan"))
    desc = (ctypes.c_int64 * 8)()
    LIB.call("uh_conv3x3_wgrad_partials", dyg.data_ptr(), Cout, x0.data_ptr(), C0, C0, ops._p(x1), C1, C1, dw2.data_ptr(), Cout,
             ws.data_ptr(), nbytes, B, H, W, dt, ctypes.addressof(desc), ops._stream())
    if desc[3]:                                                  # (a result that is no multiple of 4 floats is reduced at once)
        assert [desc[3], desc[4], desc[6]] == [plan[1], plan[5], plan[7]], (list(desc), list(plan))
        table = torch.tensor([[desc[0], desc[1], desc[2], desc[3], desc[4], desc[5], 0, desc[7]]], dtype=torch.int64, device=dev)
        LIB.call("uh_slab_reduce_batched", table.data_ptr(), 1, desc[6], ops._stream())
    else:
        assert plan[6] == 1, list(plan)
    assert torch.equal(dw2, dwk)


@pytest.mark.parametrize("dtype,noise", [(torch.float32, 1e-3), (torch.bfloat16, 0.25)])
@pytest.mark.parametrize("H,W", [(64, 64), (160, 48), (7, 9)])
def test_conv3x3_stats_of_near_constant_channels_with_a_corner_outlier(dtype, noise, H, W):
    """the BatchNorm statistics are pivot-shifted sums; a pivot taken at the image corner would be the one
    atypical value of a channel that is flat everywhere else (medical backgrounds) and M2 = S2 - S1^2 / n would cancel.
    Centre-tap filters make every output channel a scaled copy of an input channel = level 5 +- noise, except ONE huge
    value at pixel (0,0) of image 0; the merged (mean, M2) must match fp64 moments of the stored y."""
    from unet_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(H * 100 + W)
    B, C = 2, 64
    x = 5.0 + noise * torch.randn(B, C, H, W, generator=g)
    x[0, :, 0, 0] = 3000.0
    w = torch.zeros(C, C, 3, 3)
    w[torch.arange(C), torch.arange(C), 1, 1] = 1.0 + torch.arange(C) / 64.0
    if dtype == torch.bfloat16:
        x, w = x.bfloat16().float(), w.bfloat16().float()
    xg = _nhwc(x, dtype, dev)
    wf, _ = ops.pack_w3x3(w.to(dev), dtype, False)
    y, stats, nslab = ops.conv3x3_fwd(xg, None, wf, C, True)
    st = stats[:nslab * 2 * C].view(nslab, 2, C).double().cpu()
    cnt = stats[nslab * 2 * C:nslab * 2 * C + nslab].double().cpu()
    live = cnt > 0
    st, cnt = st[live], cnt[live]
    mean = (st[:, 0] * cnt[:, None]).sum(0) / cnt.sum()
    m2 = (st[:, 1] + cnt[:, None] * (st[:, 0] - mean[None]) ** 2).sum(0)
    ys = y.double().cpu().reshape(-1, C)
    # the outlier dominates the true moments; what must survive is the flat part, so compare the moments of everything BUT
    # the outlier pixel, recovered from the merged ones (exact algebra in double) -- a cancelled S2 - S1^2/n shows up here
    n = float(cnt.sum())
    o = ys[0]                                                     # pixel (0,0) of image 0
    mean_r = (mean * n - o) / (n - 1)
    m2_r = m2 - (o - mean) ** 2 * n / (n - 1)
    rest = ys[1:]
    want_mean, want_m2 = rest.mean(0), ((rest - rest.mean(0)) ** 2).sum(0)
    assert float(((mean_r - want_mean).abs() / want_mean.abs()).max()) < 1e-5
    # removing the outlier's (o - mean)^2 ~ 1e7 from M2 in double leaves fp32 round-off of the kernel's own sums: the flat
    # part's M2 is ~ n * noise^2 * gain^2; allow the kernel's fp32 accumulation (1e-6 of the outlier term) on top of 2 %
    slack = 2e-2 * want_m2 + 2e-6 * (o - mean) ** 2
    assert bool(((m2_r - want_m2).abs() <= slack).all()), float(((m2_r - want_m2).abs() / slack).max())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_conv3x3_strided_slices(dtype):
    """inputs / outputs that are channel slices of wider buffers (pixel stride > C)."""
    from unet_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(3)
    B, H, W, C, Cout = 2, 20, 28, 64, 64
    wide = torch.randn(B, H, W, 3 * C, generator=g)
    if dtype == torch.bfloat16:
        wide = wide.bfloat16().float()
    w = torch.randn(Cout, C, 3, 3, generator=g) / 24.0
    if dtype == torch.bfloat16:
        w = w.bfloat16().float()
    xs = wide[..., C:2 * C]
    yref = F.conv2d(xs.permute(0, 3, 1, 2).double(), w.double(), padding=1)
    wg = wide.to(dev, dtype)
    wf, _ = ops.pack_w3x3(w.to(dev), dtype, False)
    y, _, _ = ops.conv3x3_fwd(wg[..., C:2 * C], None, wf, Cout, False)
    e = float((y.permute(0, 3, 1, 2).double().cpu() - yref).abs().max() / yref.abs().max())
    assert e < (2e-5 if dtype == torch.float32 else 1e-2), e


# ------------------------------------------------------------------------------------------------
# pooling / upsampling / BatchNorm / 1x1 / ConvTranspose / optimizer, each against fp64 torch on CPU
# ------------------------------------------------------------------------------------------------
def _rel(a, b):
    b = b.double()
    return float((a.double().cpu() - b).abs().max() / b.abs().max().clamp_min(1e-30))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,h,w,C,Ho,Wo", [(2, 32, 32, 64, 64, 64), (2, 12, 19, 64, 25, 39), (1, 8, 9, 8, 17, 19),
                                           (2, 1, 1, 16, 2, 2), (1, 5, 7, 3, 10, 14), (2, 4, 4, 512, 8, 8),
                                           (1, 40, 33, 16, 81, 67), (8, 64, 64, 64, 128, 128), (2, 2, 2, 8, 4, 4),
                                           (1, 3, 2, 8, 7, 5), (4, 128, 96, 64, 256, 192), (1, 2, 9, 8, 4, 18),
                                           (1, 6, 7, 24, 12, 14), (2, 5, 3, 48, 13, 9), (1, 7, 7, 40, 14, 14)])   # channel groups not a power of two
def test_upsample_bilinear_pad(dtype, B, h, w, C, Ho, Wo):
    from unet_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(h * 100 + w)
    x = torch.randn(B, C, h, w, generator=g)
    cot = torch.randn(B, C, Ho, Wo, generator=g)
    if dtype == torch.bfloat16:
        x, cot = x.bfloat16().float(), cot.bfloat16().float()
    xd = x.double().requires_grad_(True)
    up = F.interpolate(xd, scale_factor=2, mode="bilinear", align_corners=True)
    dY, dX = Ho - up.shape[2], Wo - up.shape[3]
    ref = F.pad(up, [dX // 2, dX - dX // 2, dY // 2, dY - dY // 2])
    (dxref,) = torch.autograd.grad(ref, xd, cot.double())
    xg = _nhwc(x, dtype, dev).requires_grad_(True)
    y = ops.UpsampleBilinearPadFn.apply(xg, Ho, Wo)
    y.backward(_nhwc(cot, dtype, dev))
    # fp32: the interpolation weights are formed in fp32 like torch's float kernels (src = scale*dst, error ~ 6e-8*size)
    # while the reference here is fp64
    tol = max(4e-6, 1.5e-7 * max(Ho, Wo)) if dtype == torch.float32 else 8e-3
    assert _rel(y.permute(0, 3, 1, 2), ref.detach()) < tol
    assert _rel(xg.grad.permute(0, 3, 1, 2), dxref) < tol


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,h,w,C,Ho,Wo", [(2, 32, 32, 64, 64, 64), (2, 12, 19, 64, 25, 39), (1, 8, 9, 8, 17, 19), (2, 2, 2, 8, 4, 4),
                                           (1, 40, 33, 16, 81, 67), (4, 64, 48, 64, 128, 96), (1, 6, 7, 24, 12, 14)])
def test_upsample_backward_buffer_and_pointer_forms_agree(dtype, B, h, w, C, Ho, Wo, monkeypatch):
    """The strip form of the bilinear backward reads dy through a buffer descriptor (unused columns / rows get out-of-range offsets
    and read zeros) for tensors below 1 GiB and through clamped pointers + selects above: the two must be bit-identical, padding
    included, and a NaN / Inf in an output pixel must reach exactly the inputs that pixel is interpolated from in both."""
    from unet_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(7 * h + w)
    cot = torch.randn(B, Ho, Wo, C, generator=g)
    if C >= 8:
        cot[0, Ho // 2, Wo // 2, 3] = float("nan")
        cot[B - 1, Ho // 3, Wo // 3, 5] = float("inf")
    dy = cot.to(dtype).to(dev)
    pt, pl = (Ho - 2 * h) // 2, (Wo - 2 * w) // 2
    out = []
    for force in ("0", "1"):
        monkeypatch.setenv("UH_UP_BWD_PTR", force)
        dx = torch.full((B, h, w, C), 7.0, dtype=dtype, device=dev)
        ops.LIB.call("uh_upsample2x_bwd", dy.data_ptr(), C, dx.data_ptr(), C, B, h, w, C, Ho, Wo, pt, pl, ops._dt(dy), ops._stream())
        torch.cuda.synchronize()
        out.append(dx.cpu())
    a, b = out
    assert torch.equal(torch.isnan(a), torch.isnan(b))
    assert torch.equal(torch.nan_to_num(a.float(), nan=0.0, posinf=1e30, neginf=-1e30), torch.nan_to_num(b.float(), nan=0.0, posinf=1e30, neginf=-1e30))
    if C >= 8:
        # the NaN stays inside the 2 x 2 inputs of its output pixel (and its channel)
        bad = torch.isnan(a[0].float())
        assert bad.any() and bad.sum() <= 4 and bad[..., 3].sum() == bad.sum()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,H,W,C", [(2, 64, 64, 64), (2, 15, 19, 8), (1, 6, 6, 3), (2, 8, 8, 512)])
def test_maxpool_and_poolsplit(dtype, B, H, W, C):
    from unet_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(H + W + C)
    x = torch.relu(torch.randn(B, C, H, W, generator=g))       # post-ReLU like the real input: ties at 0
    if dtype == torch.bfloat16:
        x = x.bfloat16().float()
    cot = torch.randn(B, C, H // 2, W // 2, generator=g)
    skipcot = torch.randn(B, C, H, W, generator=g)
    if dtype == torch.bfloat16:
        cot, skipcot = cot.bfloat16().float(), skipcot.bfloat16().float()
    xd = x.double().requires_grad_(True)
    ref = F.max_pool2d(xd, 2)
    (dxref,) = torch.autograd.grad(ref, xd, cot.double())
    xg = _nhwc(x, dtype, dev).requires_grad_(True)
    y = ops.MaxPool2Fn.apply(xg)
    y.backward(_nhwc(cot, dtype, dev))
    assert _rel(y.permute(0, 3, 1, 2), ref.detach()) == 0.0
    # ties between equal positive values are measure-zero for fp32 randn; for bf16 they exist and the
    # first-maximum rule must match torch's
    assert _rel(xg.grad.permute(0, 3, 1, 2), dxref) == 0.0
    xg2 = _nhwc(x, dtype, dev).requires_grad_(True)
    skip, pooled = ops.PoolSplitFn.apply(xg2)
    (skip * _nhwc(skipcot, dtype, dev)).sum().backward(retain_graph=True)
    pooled.backward(_nhwc(cot, dtype, dev))
    want = dxref + skipcot.double()
    # PoolSplit's backward is called once per output use by autograd; gradients accumulate to the same sum
    assert _rel(xg2.grad.permute(0, 3, 1, 2), want) < (1e-6 if dtype == torch.float32 else 1e-2)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("ncls", [1, 4])
def test_outconv_1x1(dtype, ncls):
    from unet_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(ncls)
    B, H, W, C = 2, 33, 20, 64
    x = torch.randn(B, C, H, W, generator=g)
    wt = torch.randn(ncls, C, 1, 1, generator=g) / 8
    bias = torch.randn(ncls, generator=g)
    cot = torch.randn(B, ncls, H, W, generator=g)
    if dtype == torch.bfloat16:
        x = x.bfloat16().float()
    xd, wd, bd = x.double().requires_grad_(True), wt.double().requires_grad_(True), bias.double().requires_grad_(True)
    ref = F.conv2d(xd, wd, bd)
    dxr, dwr, dbr = torch.autograd.grad(ref, [xd, wd, bd], cot.double())
    xg = _nhwc(x, dtype, dev).requires_grad_(True)
    wg, bg = wt.to(dev).requires_grad_(True), bias.to(dev).requires_grad_(True)
    y = ops.OutConv1x1Fn.apply(xg, wg, bg)
    y.backward(cot.permute(0, 2, 3, 1).contiguous().to(dev))
    assert y.dtype == torch.float32
    assert _rel(y.permute(0, 3, 1, 2), ref.detach()) < 2e-6
    assert _rel(xg.grad.permute(0, 3, 1, 2), dxr) < (2e-6 if dtype == torch.float32 else 8e-3)
    assert _rel(wg.grad, dwr) < 2e-5 and _rel(bg.grad, dbr) < 2e-5


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,h,w,Cin,Ho,Wo", [(2, 8, 8, 64, 16, 16), (2, 8, 9, 16, 17, 19), (1, 4, 4, 128, 8, 8),
                                             # MFMA GEMM path (csrc/convt_mfma.hip): exact / padded / partial tiles / deep K
                                             (2, 16, 16, 128, 32, 32), (1, 32, 32, 64, 64, 64), (2, 8, 8, 64, 17, 19),
                                             (4, 32, 32, 256, 64, 64), (2, 16, 24, 512, 32, 48), (3, 8, 12, 192, 16, 24)])
def test_conv_transpose_pad(dtype, B, h, w, Cin, Ho, Wo):
    from unet_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(Cin)
    Cout = Cin // 2
    x = torch.randn(B, Cin, h, w, generator=g)
    wt = torch.randn(Cin, Cout, 2, 2, generator=g) / (Cin ** 0.5)
    bias = torch.randn(Cout, generator=g)
    cot = torch.randn(B, Cout, Ho, Wo, generator=g)
    if dtype == torch.bfloat16:          # like with like: the MFMA path multiplies bf16 weights (what autocast does too)
        x, cot, wt = x.bfloat16().float(), cot.bfloat16().float(), wt.bfloat16().float()
    xd, wd, bd = x.double().requires_grad_(True), wt.double().requires_grad_(True), bias.double().requires_grad_(True)
    up = F.conv_transpose2d(xd, wd, bd, stride=2)
    dY, dX = Ho - up.shape[2], Wo - up.shape[3]
    ref = F.pad(up, [dX // 2, dX - dX // 2, dY // 2, dY - dY // 2])
    dxr, dwr, dbr = torch.autograd.grad(ref, [xd, wd, bd], cot.double())
    xg = _nhwc(x, dtype, dev).requires_grad_(True)
    wg, bg = wt.to(dev).requires_grad_(True), bias.to(dev).requires_grad_(True)
    y = ops.ConvTranspose2x2PadFn.apply(xg, wg, bg, Ho, Wo)
    y.backward(_nhwc(cot, dtype, dev))
    tol = 5e-6 if dtype == torch.float32 else 8e-3
    assert _rel(y.permute(0, 3, 1, 2), ref.detach()) < tol
    assert _rel(xg.grad.permute(0, 3, 1, 2), dxr) < tol
    assert _rel(wg.grad, dwr) < 2e-5 and _rel(bg.grad, dbr) < 2e-5


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,H,W,C", [(2, 64, 64, 64), (2, 9, 11, 24), (4, 32, 32, 256), (1, 5, 5, 3)])
def test_bn_relu_forward_backward(dtype, B, H, W, C):
    """conv-free check of the BN kernels: statistics come from the generic tile-stats path of a 1-tap-like
    identity conv is not available, so drive uh_bn_* directly with exact statistics of a random y."""
    from unet_amd import ops
    from unet_amd._lib import LIB
    dev = _dev()
    g = torch.Generator().manual_seed(C)
    y = torch.randn(B, C, H, W, generator=g) * 2 + 5.0           # large mean: the hard case for the variance
    dz = torch.randn(B, C, H, W, generator=g)
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.randn(C, generator=g) * 0.1 - 2.5 * gamma      # puts the ReLU threshold inside the data
    if dtype == torch.bfloat16:
        y, dz = y.bfloat16().float(), dz.bfloat16().float()
    yd = y.double().requires_grad_(True)
    gd, bd = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    zr = F.relu(F.batch_norm(yd, None, None, gd, bd, True, 0.1, 1e-5))
    dyr, dgr, dbr = torch.autograd.grad(zr, [yd, gd, bd], dz.double())
    n = B * H * W
    yg, dzg = _nhwc(y, dtype, dev), _nhwc(dz, dtype, dev)
    mean = y.double().mean((0, 2, 3))
    var = y.double().var((0, 2, 3), unbiased=False)
    rstd = (1.0 / torch.sqrt(var + 1e-5))
    scale = (gamma.double() * rstd).float().to(dev)
    shift = (beta.double() - mean * gamma.double() * rstd).float().to(dev)
    meang, rstdg = mean.float().to(dev), rstd.float().to(dev)
    z = torch.empty_like(yg)
    dtc = 1 if dtype == torch.bfloat16 else 0
    st = torch.cuda.current_stream().cuda_stream
    LIB.call("uh_bn_relu_apply", yg.data_ptr(), C, scale.data_ptr(), shift.data_ptr(), z.data_ptr(), C, n, C, dtc, st)
    assert _rel(z.permute(0, 3, 1, 2), zr.detach()) < (2e-6 if dtype == torch.float32 else 8e-3)
    nblk = LIB.query("uh_bn_bwd_nblk", n, C)
    part = torch.empty(nblk * 2 * C, dtype=torch.float32, device=dev)
    LIB.call("uh_bn_relu_bwd_reduce", dzg.data_ptr(), C, yg.data_ptr(), C, scale.data_ptr(), shift.data_ptr(),
             meang.data_ptr(), rstdg.data_ptr(), part.data_ptr(), n, C, dtc, st)
    dgam = torch.empty(C, dtype=torch.float32, device=dev)
    dbet = torch.empty(C, dtype=torch.float32, device=dev)
    dy = torch.empty_like(yg)
    LIB.call("uh_bn_relu_bwd_apply", dzg.data_ptr(), C, yg.data_ptr(), C, scale.data_ptr(), shift.data_ptr(),
             meang.data_ptr(), rstdg.data_ptr(), part.data_ptr(), nblk, dgam.data_ptr(), dbet.data_ptr(), dy.data_ptr(), C,
             n, 0, C, dtc, st)
    tol = 2e-5 if dtype == torch.float32 else 1e-2
    assert _rel(dgam, dgr) < 2e-5 and _rel(dbet, dbr) < 2e-5
    assert _rel(dy.permute(0, 3, 1, 2), dyr) < tol
    # the split form used by SyncBN: finalize alone, then apply with ready sums (nblk = 0) and an explicit n
    dg2, db2, dy2 = torch.empty_like(dgam), torch.empty_like(dbet), torch.empty_like(dy)
    LIB.call("uh_bn_bwd_finalize", part.data_ptr(), nblk, C, dg2.data_ptr(), db2.data_ptr(), st)
    LIB.call("uh_bn_relu_bwd_apply", dzg.data_ptr(), C, yg.data_ptr(), C, scale.data_ptr(), shift.data_ptr(),
             meang.data_ptr(), rstdg.data_ptr(), None, 0, dg2.data_ptr(), db2.data_ptr(), dy2.data_ptr(), C, n, n, C, dtc, st)
    assert torch.equal(dg2, dgam) and torch.equal(db2, dbet) and torch.equal(dy2, dy)


def test_bn_relu_apply_bf16_is_fma_relu_one_rounding():
    """What uh_bn_relu_apply stores in bf16 is fma(y, scale, shift), then the ReLU, then ONE rounding: within 2**-8 (one bf16
    rounding) of the largest value.  33 x 17 pixels: partial rows."""
    from unet_amd._lib import LIB, UH_BF16
    dev = _dev()
    B, H, W, C = 2, 33, 17, 64
    g = torch.Generator().manual_seed(B * 7 + H + C)
    y = torch.randn(B, H, W, C, generator=g).to(dev, torch.bfloat16)
    scale = (torch.rand(C, generator=g) + 0.5).to(dev)
    shift = (torch.randn(C, generator=g) * 0.3).to(dev)
    z = torch.empty_like(y)
    LIB.call("uh_bn_relu_apply", y.data_ptr(), C, scale.data_ptr(), shift.data_ptr(), z.data_ptr(), C, B * H * W, C, UH_BF16,
             torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    want = torch.relu(torch.addcmul(shift, y.float(), scale)).to(torch.bfloat16)
    assert float((z.float() - want.float()).abs().max()) <= 2 ** -8 * float(want.float().abs().max())


def test_rmsprop_clip_flat():
    from unet_amd._lib import LIB
    from oracle import step_ref as S
    dev = _dev()
    g = torch.Generator().manual_seed(9)
    n = 100003
    p, gr = torch.randn(n, generator=g), torch.randn(n, generator=g) * 0.01
    sq, buf = torch.rand(n, generator=g) * 1e-4, torch.randn(n, generator=g) * 0.1
    norm = gr.double().norm().float()
    coef = S.clip_coef(norm, 1.0)
    pr, sqr, bufr = S.rmsprop_update(p.double(), (gr * coef).double(), sq.double(), buf.double(), 1e-3)
    pg, gg, sg, bg = [t.to(dev).clone() for t in (p, gr, sq, buf)]
    pad = (n + 3) // 4 * 4

    def padded(t):
        o = torch.zeros(pad, device=dev)
        o[:n] = t
        return o
    pg, gg, sg, bg = map(padded, (pg, gg, sg, bg))
    nrm = torch.zeros(1, device=dev)
    ws = torch.empty(LIB.query("uh_optim_ws_bytes", pad), dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    LIB.call("uh_grad_sumsq", gg.data_ptr(), pad, nrm.data_ptr(), ws.data_ptr(), ws.numel(), st)
    LIB.call("uh_rmsprop_step", pg.data_ptr(), gg.data_ptr(), sg.data_ptr(), bg.data_ptr(), pad, nrm.data_ptr(), 1.0, 1e-3,
             0.99, 1e-8, 1e-8, 0.999, st)
    assert abs(float(nrm) - float(norm)) < 1e-6 * float(norm)
    assert _rel(pg[:n], pr) < 1e-6 and _rel(sg[:n], sqr) < 1e-5 and _rel(bg[:n], bufr) < 1e-5
    assert _rel(gg[:n], (gr * coef).double()) < 1e-6


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_batched_weight_pack_matches_per_layer(dtype):
    """uh_pack_w3x3_batched (one launch for every 3x3 filter of a model) == uh_pack_w3x3 per layer, for contiguous and
    channels_last parameters, and the cache notices parameter updates."""
    from unet_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(4)
    shapes = [(64, 1), (64, 64), (128, 64), (16, 24), (8, 3), (256, 128), (128, 512), (512, 1024), (72, 40), (96, 160)]      # odd entries channels_last: whole 32 x 32 tiles take the 16-byte form, (96, 160) mixes both forms
    ws = []
    for k, (o, i) in enumerate(shapes):
        w = torch.randn(o, i, 3, 3, generator=g).to(dev)
        if k % 2:
            w = w.contiguous(memory_format=torch.channels_last)
        ws.append(w)
    pack = ops.ConvWeightPack(ws, dtype)
    pack.refresh()
    nfrag = 0
    for w, fr in zip(ws, pack.frags):
        # every layer is packed in the layouts the pack chose (fragment-major where the MFMA kernel will consume it);
        # asking for another layout is a miss
        hit = pack.lookup(w, dtype, *fr)
        assert hit is not None
        wf, wd = ops.pack_w3x3(w, dtype, True, None, *fr)
        assert torch.equal(hit[0], wf) and torch.equal(hit[1], wd)
        assert pack.lookup(w, dtype, not fr[0], fr[1]) is None
        nfrag += int(fr[0]) + int(fr[1])
        if fr[0]:                 # a fragment-major pack is a permutation of the KRSC pack
            kr = ops.pack_w3x3(w, dtype, False)[0]
            assert torch.equal(torch.sort(wf.float())[0], torch.sort(kr.float())[0]) and not torch.equal(wf, kr)
    assert nfrag > 0
    fr0, fr2 = pack.frags[0], pack.frags[2]
    assert pack.lookup(ws[0], torch.float32 if dtype == torch.bfloat16 else torch.bfloat16, *fr0) is None
    ws[2].mul_(2.0)                                   # torch-side update: version counter moves -> miss until refreshed
    assert pack.lookup(ws[2], dtype, *fr2) is None
    pack.refresh()
    wf, wd = ops.pack_w3x3(ws[2], dtype, True, None, *fr2)
    hit = pack.lookup(ws[2], dtype, *fr2)
    assert torch.equal(hit[0], wf) and torch.equal(hit[1], wd)
    ops.WEIGHT_EPOCH += 1                             # raw-pointer optimizer update -> every entry is stale
    assert pack.lookup(ws[0], dtype, *fr0) is None


@pytest.mark.parametrize("B,H,W,C0,C1,Cout", [(2, 32, 32, 64, 0, 128), (2, 17, 23, 64, 64, 64), (1, 40, 24, 128, 128, 128),
                                               (2, 8, 8, 512, 0, 512), (1, 448, 448, 64, 0, 64), (8, 64, 64, 16, 0, 64)])
def test_conv3x3_bf16x3_split_products(B, H, W, C0, C1, Cout):
    """fp32 tensors, products on the bf16 matrix pipe (UH_F32X3): w*x ~= wh*xh + wh*xl + wl*xh.  Forward, the fused
    inference epilogue and backward-data against fp64; the error budget is ~2^-17 per product (1e-5), asserted at 1e-4."""
    from unet_amd import ops
    from unet_amd._lib import LIB, UH_F32X3
    dev = _dev()
    g = torch.Generator().manual_seed(B + H + C0 + Cout)
    Cin = C0 + C1
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (3.0 * Cin ** 0.5)
    dy = torch.randn(B, Cout, H, W, generator=g)
    xd, wd_ = x.double().requires_grad_(True), w.double()
    yref = F.conv2d(xd, wd_, padding=1)
    (dxref,) = torch.autograd.grad(yref, xd, dy.double())
    xg = _nhwc(x, torch.float32, dev)
    x0, x1 = xg[..., :C0], (xg[..., C0:] if C1 else None)
    need_dx = Cin % 64 == 0
    wf, wdg = ops.pack_w3x3(w.to(dev), torch.float32, need_dx, UH_F32X3)
    y, stats, nslab = ops.conv3x3_fwd(x0, x1, wf, Cout, True, UH_F32X3)
    rel = lambda a, b: float((a.double().cpu() - b).abs().max() / b.abs().max())
    e = rel(y.permute(0, 3, 1, 2), yref.detach())
    assert e < 1e-4, f"fwd {e:.3e}"
    yx, _, _ = ops.conv3x3_fwd(x0, x1, ops.pack_w3x3(w.to(dev), torch.float32, False)[0], Cout, False)      # exact fp32 MFMA
    assert rel(y.permute(0, 3, 1, 2), yx.permute(0, 3, 1, 2).double().cpu()) < 1e-4
    st = stats[:nslab * 2 * Cout].view(nslab, 2, Cout).double().cpu()
    cnt = stats[nslab * 2 * Cout:nslab * 2 * Cout + nslab].double().cpu()
    live = cnt > 0
    mean = (st[live, 0] * cnt[live, None]).sum(0) / cnt.sum()
    assert float((mean - y.double().cpu().reshape(-1, Cout).mean(0)).abs().max()) < 1e-5 * float(y.abs().max()) + 1e-7
    if need_dx:
        dx, _, _ = ops.conv3x3_fwd(_nhwc(dy, torch.float32, dev), None, wdg, Cin, False, UH_F32X3)
        e = rel(dx.permute(0, 3, 1, 2), dxref)
        assert e < 1e-4, f"dgrad {e:.3e}"
    sc, sh = (torch.rand(Cout, generator=g) + 0.5).to(dev), (torch.randn(Cout, generator=g) * 0.3).to(dev)
    z = torch.empty(B, H, W, Cout, dtype=torch.float32, device=dev)
    LIB.call("uh_conv3x3_fwd_affine_relu", x0.data_ptr(), C0, ops.pixel_ld(x0), None if x1 is None else x1.data_ptr(), C1,
             0 if x1 is None else ops.pixel_ld(x1), wf.data_ptr(), z.data_ptr(), Cout, Cout, sc.data_ptr(), sh.data_ptr(),
             B, H, W, UH_F32X3, torch.cuda.current_stream().cuda_stream)
    zref = F.relu(yref.detach() * sc.double().cpu()[None, :, None, None] + sh.double().cpu()[None, :, None, None])
    assert rel(z.permute(0, 3, 1, 2), zref) < 1e-4


def test_bf16x3_rejects_unaligned_shapes():
    from unet_amd import ops
    from unet_amd._lib import UH_F32X3
    dev = _dev()
    x = torch.randn(1, 8, 8, 24, device=dev)
    w = torch.randn(16, 24, 3, 3, device=dev)
    wf, _ = ops.pack_w3x3(w, torch.float32, False, UH_F32X3)
    with pytest.raises(RuntimeError, match="bf16x3"):
        ops.conv3x3_fwd(x, None, wf, 16, False, UH_F32X3)


@pytest.mark.parametrize("B,H,W,C0,C1,Cout", [(2, 32, 32, 64, 0, 128), (2, 17, 23, 64, 64, 64), (1, 40, 24, 128, 128, 128), (2, 8, 8, 512, 0, 512)])
def test_conv3x3_wgrad_bf16x3(B, H, W, C0, C1, Cout):
    """backward-weights with bf16x3 split products (fp32 dy and x, v_mfma_f32_32x32x8_bf16 x3) against fp64."""
    from unet_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(B + H + C0 + Cout + 1)
    Cin = C0 + C1
    x = torch.randn(B, Cin, H, W, generator=g)
    dy = torch.randn(B, Cout, H, W, generator=g)
    wd_ = torch.zeros(Cout, Cin, 3, 3, dtype=torch.float64, requires_grad=True)
    (dwref,) = torch.autograd.grad(F.conv2d(x.double(), wd_, padding=1), wd_, dy.double())
    xg = _nhwc(x, torch.float32, dev)
    x0, x1 = xg[..., :C0], (xg[..., C0:] if C1 else None)
    dwk = torch.empty(Cout * 9 * Cin, dtype=torch.float32, device=dev)
    ops.conv3x3_wgrad(_nhwc(dy, torch.float32, dev), x0, x1, dwk, split=True)
    got = dwk.view(Cout, 3, 3, Cin).permute(0, 3, 1, 2).double().cpu()
    e = float((got - dwref).abs().max() / dwref.abs().max())
    assert e < 1e-4, f"wgrad bf16x3 {e:.3e}"
    dwx = torch.empty_like(dwk)
    ops.conv3x3_wgrad(_nhwc(dy, torch.float32, dev), x0, x1, dwx)                  # exact fp32 MFMA
    assert float((dwk - dwx).abs().max() / dwx.abs().max()) < 1e-4


@pytest.mark.parametrize("B,h,w,Cin,Ho,Wo", [(2, 16, 16, 128, 32, 32), (2, 8, 8, 64, 17, 19), (4, 32, 32, 256, 64, 64)])
def test_conv_transpose_bf16x3(B, h, w, Cin, Ho, Wo):
    """ConvTranspose2d k2 s2 in fp32 with bf16x3 split products (ops.step_state(fp32_mode=...)) against fp64."""
    from unet_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(Cin + 5)
    Cout = Cin // 2
    x = torch.randn(B, Cin, h, w, generator=g)
    wt = torch.randn(Cin, Cout, 2, 2, generator=g) / (Cin ** 0.5)
    bias = torch.randn(Cout, generator=g)
    cot = torch.randn(B, Cout, Ho, Wo, generator=g)
    xd, wd, bd = x.double().requires_grad_(True), wt.double().requires_grad_(True), bias.double().requires_grad_(True)
    up = F.conv_transpose2d(xd, wd, bd, stride=2)
    dY, dX = Ho - up.shape[2], Wo - up.shape[3]
    ref = F.pad(up, [dX // 2, dX - dX // 2, dY // 2, dY - dY // 2])
    dxr, dwr, dbr = torch.autograd.grad(ref, [xd, wd, bd], cot.double())
    with ops.step_state(fp32_mode="bf16x3"):
        xg = _nhwc(x, torch.float32, dev).requires_grad_(True)
        wg, bg = wt.to(dev).requires_grad_(True), bias.to(dev).requires_grad_(True)
        y = ops.ConvTranspose2x2PadFn.apply(xg, wg, bg, Ho, Wo)
        y.backward(_nhwc(cot, torch.float32, dev))
    assert _rel(y.permute(0, 3, 1, 2), ref.detach()) < 1e-4
    assert _rel(xg.grad.permute(0, 3, 1, 2), dxr) < 1e-4
    assert _rel(wg.grad, dwr) < 1e-4 and _rel(bg.grad, dbr) < 2e-5


# ------------------------------------------------------------------------------------------------
# small-width layers (UNet_S / UNet_T): narrow tensors in HBM, arithmetic padded to 64 channels
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,H,W,C0,C1,Cout", [(2, 20, 28, 3, 0, 16), (2, 17, 23, 16, 16, 32), (1, 24, 24, 32, 0, 16),
                                              (2, 16, 16, 64, 64, 32), (2, 12, 12, 128, 0, 8), (1, 9, 7, 1, 0, 8),
                                              (2, 33, 18, 8, 8, 8), (1, 16, 16, 32, 32, 64)])
def test_small_width_narrow_tensors(dtype, B, H, W, C0, C1, Cout):
    """ConvBnReluNarrowFn (tensors at their real channel count, uh_conv3x3_*_narrow) against (a) the zero-padded 64-channel
    formulation on the ordinary entry points -- same arithmetic, so the forward must agree BIT FOR BIT -- and (b) fp64
    stock-PyTorch maths of conv -> BatchNorm(train) -> ReLU."""
    import torch.nn as nn
    from unet_amd import ops
    from unet_amd.unet import unet_parts
    dev = _dev()
    g = torch.Generator().manual_seed(B + H * 7 + C0 * 13 + C1 * 17 + Cout)
    Cin = C0 + C1
    conv = nn.Conv2d(Cin, Cout, 3, padding=1, bias=False)
    bn = nn.BatchNorm2d(Cout)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(Cout, Cin, 3, 3, generator=g) / (3.0 * Cin ** 0.5))
        bn.weight.copy_(torch.rand(Cout, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(Cout, generator=g) * 0.2)
    x = torch.randn(B, H, W, Cin, generator=g)
    gz = torch.randn(B, H, W, Cout, generator=g)
    if dtype == torch.bfloat16:
        x = x.bfloat16().float()
    conv, bn = conv.to(dev), bn.to(dev)

    def run(narrow, training=True):
        ops.NARROW_IO = narrow
        try:
            bn.running_mean.zero_(); bn.running_var.fill_(1.0); bn.num_batches_tracked.zero_()
            x0 = x[..., :C0].to(dev, dtype).contiguous().requires_grad_(True)
            x1 = x[..., C0:].to(dev, dtype).contiguous().requires_grad_(True) if C1 else None
            z = unet_parts._conv_bn_relu(x0, x1, conv, bn, training)
            if not training:
                return z.detach().float().cpu()
            ins = [t for t in (x0, x1, conv.weight, bn.weight, bn.bias) if t is not None]
            grads = torch.autograd.grad((z.float() * gz.to(dev)).sum(), ins)
            out = [z.detach()] + list(grads) + [bn.running_mean.clone(), bn.running_var.clone()]
            assert int(bn.num_batches_tracked) == 1
            return [t.float().cpu() for t in out]
        finally:
            ops.NARROW_IO = True

    nar, pad = run(True), run(False)
    assert nar[0].shape == (B, H, W, Cout)
    stem = Cin <= 4          # the padded formulation of an image layer runs on the (non-MFMA) stem kernels: same maths,
    ftol = 1e-5 if dtype == torch.float32 else 2e-2     # another summation order

    def same(a, b, what):
        if stem:
            e = float((a - b).abs().max() / (b.abs().max() + 1e-12))
            assert e < ftol, f"{what}: {e:.3e}"
        else:
            assert torch.equal(a, b), f"{what} differs from the padded formulation"

    same(nar[0], pad[0], "forward")
    same(nar[-2], pad[-2], "running_mean")
    same(nar[-1], pad[-1], "running_var")
    for a, b, name in zip(nar[1:-2], pad[1:-2], ["dx0", "dx1", "dW", "dgamma", "dbeta"] if C1 else ["dx0", "dW", "dgamma", "dbeta"]):
        assert a.shape == b.shape, name
        e = float((a - b).abs().max() / (b.abs().max() + 1e-12))
        assert e < (1e-4 if dtype == torch.float32 else 2e-2), f"{name}: {e:.3e}"
    # inference form (running statistics, fused scale/shift/ReLU epilogue)
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(Cout, generator=g) * 0.1); bn.running_var.copy_(torch.rand(Cout, generator=g) + 0.5)
        rm, rv = bn.running_mean.clone(), bn.running_var.clone()

        def run_eval(narrow):
            ops.NARROW_IO = narrow
            try:
                bn.running_mean.copy_(rm); bn.running_var.copy_(rv)
                x0 = x[..., :C0].to(dev, dtype).contiguous()
                x1 = x[..., C0:].to(dev, dtype).contiguous() if C1 else None
                return unet_parts._conv_bn_relu(x0, x1, conv, bn, False).float().cpu()
            finally:
                ops.NARROW_IO = True
        ze_n, ze_p = run_eval(True), run_eval(False)
        same(ze_n, ze_p, "eval forward")
        assert torch.equal(bn.running_mean, rm) and torch.equal(bn.running_var, rv)

    if dtype == torch.float32:
        xd = x.permute(0, 3, 1, 2).double().requires_grad_(True)
        wd = conv.weight.detach().double().cpu().requires_grad_(True)
        gd = bn.weight.detach().double().cpu().requires_grad_(True)
        bd = bn.bias.detach().double().cpu().requires_grad_(True)
        zr = F.relu(F.batch_norm(F.conv2d(xd, wd, padding=1), None, None, gd, bd, True, 0.1, bn.eps))
        ref = torch.autograd.grad((zr * gz.permute(0, 3, 1, 2).double()).sum(), [xd, wd, gd, bd])
        assert _rel(nar[0].permute(0, 3, 1, 2), zr.detach()) < 1e-4
        dx = torch.cat([nar[1], nar[2]], dim=-1) if C1 else nar[1]
        k = 3 if C1 else 2
        assert _rel(dx.permute(0, 3, 1, 2), ref[0]) < 2e-4
        assert _rel(nar[k], ref[1]) < 2e-4
        assert _rel(nar[k + 1], ref[2]) < 2e-4 and _rel(nar[k + 2], ref[3]) < 2e-4
        ze_ref = F.relu(F.batch_norm(F.conv2d(xd.detach(), wd.detach(), padding=1), rm.double().cpu(), rv.double().cpu(),
                                     gd.detach(), bd.detach(), False, 0.1, bn.eps))
        assert _rel(ze_n.permute(0, 3, 1, 2), ze_ref) < 1e-4


def test_narrow_entry_points_reject_bad_arguments():
    from unet_amd import ops
    from unet_amd._lib import LIB, UH_BF16
    dev = _dev()
    x = torch.zeros(1, 8, 8, 16, dtype=torch.bfloat16, device=dev)
    w = torch.zeros(64 * 9 * 64, dtype=torch.bfloat16, device=dev)
    y = torch.zeros(1, 8, 8, 16, dtype=torch.bfloat16, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    with pytest.raises(RuntimeError):      # valid count not a multiple of a 16-byte piece
        LIB.call("uh_conv3x3_fwd_narrow", x.data_ptr(), 64, 12, 16, None, 0, 0, 0, w.data_ptr(), y.data_ptr(), 16, 64, 16,
                 None, None, None, 1, 8, 8, UH_BF16, st)
    with pytest.raises(RuntimeError):      # padded count not on the MFMA path
        LIB.call("uh_conv3x3_fwd_narrow", x.data_ptr(), 48, 16, 16, None, 0, 0, 0, w.data_ptr(), y.data_ptr(), 16, 64, 16,
                 None, None, None, 1, 8, 8, UH_BF16, st)
    with pytest.raises(RuntimeError):      # valid > padded
        LIB.call("uh_conv3x3_fwd_narrow", x.data_ptr(), 64, 128, 16, None, 0, 0, 0, w.data_ptr(), y.data_ptr(), 16, 64, 16,
                 None, None, None, 1, 8, 8, UH_BF16, st)


def _wgrad_errors(x, dy, dev):
    """rms error of uh_conv3x3_wgrad (bf16 tensors) against fp64, rms error of the fp64 total rounded to bf16 -- what the
    reference's autocast backward hands to the optimizer (train.py:116; the conv's weight is a bf16 copy) -- and the largest error
    relative to the largest element."""
    from unet_amd import ops
    B, Cin, H, W = x.shape
    Cout = dy.shape[1]
    wd = torch.zeros(Cout, Cin, 3, 3, dtype=torch.float64, requires_grad=True)
    (dwref,) = torch.autograd.grad(F.conv2d(x.double(), wd, padding=1), [wd], dy.double())
    dwk = torch.empty(Cout * 9 * Cin, dtype=torch.float32, device=dev)
    ops.conv3x3_wgrad(_nhwc(dy, torch.bfloat16, dev), _nhwc(x, torch.bfloat16, dev), None, dwk)
    ours = dwk.view(Cout, 3, 3, Cin).permute(0, 3, 1, 2).double().cpu()
    e_ours = float((ours - dwref).pow(2).mean().sqrt())
    e_ref = float((dwref.float().bfloat16().double() - dwref).pow(2).mean().sqrt())
    return e_ours, e_ref, float((ours - dwref).abs().max() / dwref.abs().max())


@pytest.mark.parametrize("B,H,W,Cin,Cout", [(2, 128, 128, 128, 256), (2, 256, 256, 64, 64), (4, 32, 32, 512, 512), (2, 128, 128, 128, 128),
                                            (2, 120, 136, 64, 128)])
def test_16_bit_slabs_are_more_precise_than_the_reference_rounding_of_the_total(B, H, W, Cin, Cout):
    """The per-split partial sums of bf16 backward-weights travel to the reduce kernel as block-scaled fp16 pairs (SLAB16) and are
    added in fp32 (the shapes take the reduce kernel through its 8, 32, 4, 16 and 32 split-lane blocks: 64, 512, 8, 128, 256 splits;
    the last one with border tiles).  The reference's autocast backward returns the filter gradient in bf16, i.e. it rounds the TOTAL.  On
    i.i.d. gradients the partials, added in quadrature, are about as large as the total, and fp16 carries three more bits than
    bf16: the error against fp64 stays far below that single rounding of the total."""
    dev = _dev()
    g = torch.Generator().manual_seed(B + H + Cin + Cout)
    x = torch.relu(torch.randn(B, Cin, H, W, generator=g)).bfloat16().float()           # activations as the layer sees them: half zeros
    dy = torch.randn(B, Cout, H, W, generator=g).bfloat16().float()
    e_ours, e_ref, worst = _wgrad_errors(x, dy, dev)
    assert e_ours <= 0.25 * e_ref, (e_ours, e_ref)
    assert worst <= 5e-4, worst


@pytest.mark.parametrize("B,H,W,Cin,Cout", [(2, 256, 256, 64, 64), (8, 256, 256, 64, 128), (2, 128, 128, 128, 256), (4, 64, 64, 256, 512)])
@pytest.mark.parametrize("noise", [0.0, 0.3])
def test_16_bit_slabs_with_a_gradient_whose_sign_follows_image_regions(B, H, W, Cin, Cout, noise):
    """i.i.d. gradients hide the hard case.  Here dy is +a inside a centred disc and -a' outside, zero-sum per
    channel over the batch (what BatchNorm backward hands down), x is a ReLU'd activation with a large mean: a pixel tile lies
    inside one region, so every per-split partial sum is ~10 x larger than the total in quadrature, whatever the order of the
    tiles (contiguous ranges and strided tiles measured alike, scratch/r5_slab_structured.py).  Round 4's bf16 partials put the
    result 8-13 x above the reference's single bf16 rounding of the total on these inputs; block-scaled fp16 must stay within
    1.6 x of it (measured 1.0-1.5), and fp32 slabs (UH_WGRAD_SLAB_F32=1) remain for anyone who wants the partials exact."""
    dev = _dev()
    g = torch.Generator().manual_seed(B + H + Cin + Cout)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    disc = (((yy - H / 2) ** 2 + (xx - W / 2) ** 2) < (0.3 * min(H, W)) ** 2).float()
    sign = disc - (1 - disc) * disc.mean() / (1 - disc.mean())
    amp = torch.rand(1, Cout, 1, 1, generator=g) + 0.5
    dy = sign[None, None] * amp + noise * torch.randn(B, Cout, H, W, generator=g)
    dy = dy - dy.mean(dim=(0, 2, 3), keepdim=True)
    x = torch.relu(torch.randn(B, Cin, H, W, generator=g) + 1.5)
    e_ours, e_ref, worst = _wgrad_errors(x.bfloat16().float(), dy.bfloat16().float(), dev)
    assert e_ours <= 1.6 * e_ref, (e_ours, e_ref, e_ours / e_ref)
    assert worst <= 6e-3, worst
