"""GPU tests of the spatial-attention kernels (csrc/spatial_attn.hip) and UNet_SA: the map and the fused skip gate against
fp64 CPU torch over channel counts, odd extents, both filter sizes and a strided gradient; the bf16 path by the yardstick
of tests/yardstick.py; fixture set G17 (the reference's SpatialAttention, Up(use_attention=True), UNet_SA); graph capture,
determinism and the benchmarked 8 x 1 x 512^2 bf16 shape."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from conftest import load_golden
from test_gpu_parity import T, _dev, check, run_block
from test_spatial_attention_cpu import sa_map_ref
from yardstick import Collector, l2

pytestmark = pytest.mark.gpu


def tied_input(b, c, h, w, seed):
    """ReLU-like activations with all-zero pixels and maxima held by two channels (the lower one takes the gradient)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.relu(torch.randn(b, c, h, w, generator=g))
    x[:, :, ::4, ::3] = 0.0
    if c >= 6:
        x[:, 2, 1::2, ::2] = 7.0
        x[:, 5, 1::2, ::2] = 7.0
    return x


def rel_l2(a, b):
    return float((a.detach().double().cpu() - b.detach().double().cpu()).norm() / b.detach().double().cpu().norm().clamp_min(1e-300))


def _ref64(x, w, cot, gate):
    """fp64 CPU torch: gate -> (y = x * map, dx, dw) for the cotangent of y; map -> (map, dx, dw) for the cotangent of the map."""
    xr = x.double().requires_grad_(True)
    wr = w.double().requires_grad_(True)
    a = sa_map_ref(xr, wr)
    out = xr * a if gate else a
    out.backward(cot.double())
    return out.detach(), xr.grad, wr.grad, a.detach()


@pytest.mark.parametrize("k", [3, 7])
@pytest.mark.parametrize("hw", [(15, 19), (1, 1)])
@pytest.mark.parametrize("C", [1, 16, 24, 64, 128])
def test_kernels_vs_fp64_fp32(C, hw, k):
    import unet_amd
    from unet_amd import ops
    dev = _dev()
    H, W = hw
    B = 2
    x = tied_input(B, C, H, W, seed=C * 100 + H + k)
    g = torch.Generator().manual_seed(7 + C + k)
    w = torch.randn(1, 2, k, k, generator=g) * 0.5
    cot_y = torch.randn(B, C, H, W, generator=g)
    cot_a = torch.randn(B, 1, H, W, generator=g)
    xn = x.permute(0, 2, 3, 1).contiguous().to(dev)
    wd = w.to(dev).requires_grad_(True)

    # fused gate; its gradient arrives as the skip half of a concat gradient (pixel stride 2C)
    y_ref, dx_ref, dw_ref, a_ref = _ref64(x, w, cot_y, gate=True)
    xg = xn.clone().requires_grad_(True)
    y = ops.SpatialAttnGateFn.apply(xg, wd)
    wide = torch.cat([cot_y.permute(0, 2, 3, 1), torch.zeros(B, H, W, C)], dim=-1).to(dev)
    dy = wide[..., :C]
    assert ops.pixel_ld(dy) == 2 * C
    y.backward(dy)
    assert rel_l2(y.permute(0, 3, 1, 2), y_ref) <= 1e-5
    assert rel_l2(xg.grad.permute(0, 3, 1, 2), dx_ref) <= 1e-5
    assert rel_l2(wd.grad, dw_ref) <= 1e-4

    # standalone map (its backward takes the map's gradient directly)
    a_ref2, dxa_ref, dwa_ref, _ = _ref64(x, w, cot_a, gate=False)
    wd.grad = None
    xa = xn.clone().requires_grad_(True)
    a = ops.SpatialAttnMapFn.apply(xa, wd)
    a.backward(cot_a.permute(0, 2, 3, 1).to(dev))
    assert rel_l2(a.permute(0, 3, 1, 2), a_ref2) <= 1e-5
    assert rel_l2(xa.grad.permute(0, 3, 1, 2), dxa_ref) <= 1e-5
    assert rel_l2(wd.grad, dwa_ref) <= 1e-4
    if C >= 6 and H > 1:
        # tied pixels: the max's gradient lands on channel 2 (the first maximum), never on channel 5
        gx = xa.grad.permute(0, 3, 1, 2).double().cpu()
        tied = (slice(None), slice(1, None, 2), slice(0, None, 2))
        d_first = gx[:, 2][tied] - dxa_ref[:, 2][tied]
        d_second = gx[:, 5][tied] - dxa_ref[:, 5][tied]
        scale = float(dxa_ref.abs().max())
        assert float(d_first.abs().max()) <= 1e-5 * scale and float(d_second.abs().max()) <= 1e-5 * scale
        assert float((dxa_ref[:, 2][tied] - dxa_ref[:, 5][tied]).abs().max()) > 1e-3 * scale     # the case is exercised


@pytest.mark.parametrize("C,k", [(16, 7), (64, 7), (128, 3)])
def test_gate_bf16_by_the_yardstick(C, k):
    """bf16 gate against the fp32 CPU graph on the same (bf16-representable) inputs, held to the reference's own bf16 error
    (the same graph under torch.autocast('cpu', bfloat16))."""
    from unet_amd import ops
    dev = _dev()
    B, H, W = 2, 33, 47
    x = tied_input(B, C, H, W, seed=900 + C).bfloat16().float()
    g = torch.Generator().manual_seed(901 + C)
    w = torch.randn(1, 2, k, k, generator=g) * 0.5
    cot = torch.randn(B, C, H, W, generator=g).bfloat16().float()
    sa = nn.Module()
    sa.conv1 = nn.Conv2d(2, 1, k, padding=k // 2, bias=False)
    with torch.no_grad():
        sa.conv1.weight.copy_(w)
    legs = {}
    for tag, amp in (("ref32", False), ("ref16", True)):
        sa.zero_grad(set_to_none=True)
        xr = (x.bfloat16() if amp else x).clone().requires_grad_(True)
        with torch.autocast("cpu", dtype=torch.bfloat16, enabled=amp):
            pooled = torch.cat([xr.mean(dim=1, keepdim=True), xr.max(dim=1, keepdim=True)[0]], dim=1)
            y = xr * torch.sigmoid(sa.conv1(pooled))
        y.float().backward(cot)
        legs[tag] = (y.detach().float(), xr.grad.float(), sa.conv1.weight.grad.clone())
    xg = x.permute(0, 2, 3, 1).contiguous().bfloat16().to(dev).requires_grad_(True)
    wd = w.to(dev).requires_grad_(True)
    y = ops.SpatialAttnGateFn.apply(xg, wd)
    y.backward(cot.permute(0, 2, 3, 1).bfloat16().to(dev))
    c = Collector(f"spatial-attention gate C={C} k={k}")
    c.tensor("y", y.permute(0, 3, 1, 2).float(), legs["ref32"][0], legs["ref16"][0])
    c.tensor("dx", xg.grad.permute(0, 3, 1, 2).float(), legs["ref32"][1], legs["ref16"][1])
    c.tensor("dw", wd.grad, legs["ref32"][2], legs["ref16"][2])
    c.done()


def test_backward_is_bit_identical_between_runs():
    from unet_amd import ops
    dev = _dev()
    x = tied_input(4, 32, 97, 131, seed=3).permute(0, 2, 3, 1).contiguous().to(dev)
    w = (torch.randn(1, 2, 7, 7) * 0.3).to(dev).requires_grad_(True)
    cot = torch.randn(4, 97, 131, 32).to(dev)
    out = []
    for _ in range(2):
        w.grad = None
        xg = x.clone().requires_grad_(True)
        ops.SpatialAttnGateFn.apply(xg, w).backward(cot)
        out.append((xg.grad.clone(), w.grad.clone()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


@pytest.mark.parametrize("k", [7, 3])
def test_spatial_attention_golden(k):
    import unet_amd
    run_block(unet_amd.SpatialAttention(k), load_golden(f"g17_sa_k{k}"), _dev(), 1)


@pytest.mark.parametrize("name,bilinear", [("g17_up_sa_bilinear_16_8", True), ("g17_up_sa_bilinear_16_8_oddpad", True),
                                           ("g17_up_sa_convt_16_8", False), ("g17_up_sa_convt_16_8_oddpad", False)])
def test_attention_up_golden(name, bilinear):
    import unet_amd
    run_block(unet_amd.AttentionUp(16, 8, bilinear), load_golden(name), _dev(), 2)


def test_unet_sa_default_model_trajectory():
    """G17: UNet_SA(1, 3, bilinear=False), seeded init, 3 fp32 steps with CE + multiclass Dice; the tolerances of G16's
    UNet_S trajectory (test_gpu_parity.py::_run_traj)."""
    import unet_amd
    dev = _dev()
    r = load_golden("g17_unet_sa_convt_3class")
    lr = 1e-5
    torch.manual_seed(0)
    model = unet_amd.UNet_SA(1, 3, False)
    for (k, v), want, scale in zip(model.state_dict().items(), r["sd0_sums"], r["sd0_abs_sums"]):
        assert abs(float(v.double().sum()) - want) <= 1e-9 * max(scale, 1.0), k
    model = model.to(dev)
    stepper = unet_amd.TrainStepper(model, lr=lr, amp=False)
    for s in range(3):
        im, mk = T(r[f"s{s}.images"], dev), T(r[f"s{s}.masks"], dev)
        model.train()
        terms = unet_amd.train_step(model, stepper.optimizer, im, mk, amp=False)
        tl = 1e-3 if s == 0 else 2e-2
        check(terms["logits"], r[f"s{s}.logits"], tl, f"logits s{s}")
        for q in ("loss", "dice", "ce"):
            check(terms[q], r[f"s{s}.{q}"], 1e-4 if s == 0 else 3e-3, f"{q} s{s}")
        check(terms["grad_norm"], r[f"s{s}.grad_norm"], 1e-3 if s == 0 else 3e-2, f"grad_norm s{s}")
        if s == 0:
            named = dict(model.named_parameters())
            for k, n2 in zip([str(n) for n in r["grad_names"]], r["grad_l2"]):
                g = stepper.optimizer.grad_of(named[k])
                if "s0.grad." + k in r:
                    check(g, r["s0.grad." + k], 2e-2, "grad " + k, l2=True)
                assert abs(float(g.double().norm()) - n2) <= 2e-2 * n2, k
    sd = model.state_dict()
    for k, n2, tot in zip([str(n) for n in r["sd3_names"]], r["sd3_l2"], r["sd3_sums"]):
        v = sd[k]
        if "num_batches" in k:
            assert int(v) == int(r["sd3." + k]) if "sd3." + k in r else int(v) == 3
            continue
        if "sd3." + k in r:
            check(v, r["sd3." + k], 5e-3, "final " + k, atol=0.0 if "running" in k else 150 * lr)
        assert abs(float(v.double().norm()) - n2) <= 5e-3 * n2 + 150 * lr * np.sqrt(v.numel()), k


def test_unet_sa_bf16_step0_by_the_yardstick():
    """G17: UNet_SA(1,1,bilinear=True) step 0 under bf16 against the reference's fp32 result, held to the reference's own
    bf16 error (its autocast('cpu', bfloat16) result in the same fixture)."""
    import unet_amd
    from yardstick import FACTOR, FACTOR_LOOSE
    dev = _dev()
    r = load_golden("g17_bf16_unet_sa_bilinear_64")
    torch.manual_seed(0)
    model = unet_amd.UNet_SA(1, 1, bilinear=True).to(dev)
    stepper = unet_amd.TrainStepper(model, amp=True)
    terms = stepper.step(T(r["images"], dev), T(r["masks"], dev))
    c = Collector("UNet_SA 64x64")
    for q in ("bce", "dice", "grad_norm"):
        c.scalar(q, float(terms[q].detach()), r[f"ref32.s0.{q}"], r[f"ref16.s0.{q}"])
    c.scalar("bce + dice", float((terms["bce"] + terms["dice"]).detach()), r["ref32.s0.bce"] + r["ref32.s0.dice"],
             r["ref16.s0.bce"] + r["ref16.s0.dice"])
    c.tensor("logits", terms["logits"].float(), r["ref32.s0.logits"], r["ref16.s0.logits"])
    _boundary_is_that_of_the_logits(terms, T(r["masks"]))
    names = [str(k) for k in r["grad_names"]]
    own = dict(zip(names, r["grad_l2.diff"] / r["grad_l2.ref32"]))
    n32 = dict(zip(names, r["grad_l2.ref32"]))
    for k, p in model.named_parameters():
        g = stepper.optimizer.grad_of(p)
        factor = FACTOR if p.numel() >= 1024 else FACTOR_LOOSE
        if "ref32.grad." + k in r:
            c.add("grad " + k, l2(g, r["ref32.grad." + k]), float(own[k]), factor=factor)
        else:      # large tensors: only their norms are stored -- the norm's relative error is a lower bound of the L2 error
            c.add("grad-norm " + k, abs(float(g.double().norm()) - n32[k]) / n32[k], float(own[k]), factor=factor)
    c.done()


def _boundary_is_that_of_the_logits(terms, masks):
    """The boundary term (weight 0.25 in the loss) thresholds the raw logits at 0.5 (boundary_loss.py:28, :88-96: at
    initialisation no logit leaves [-10, 10], so no sigmoid is applied): a pixel whose logit sits next to 0.5 flips its
    whole count under ANY rounding, so this piecewise-constant term carries no precision yardstick (the reference's own
    bf16 lands on its fp32 value by luck in G17, 1 % away on other draws).  It must be exactly the boundary loss of the
    logits the HIP step computed -- whose precision the yardstick judges."""
    from oracle import losses_ref as L
    logits = terms["logits"].detach().float().cpu()
    want = float(L.boundary_loss(logits.squeeze(1), (masks // 2).float(), edge_width=51, edge_weight=15))
    assert abs(float(terms["boundary"].detach()) - want) <= 1e-4 * abs(want), (float(terms["boundary"]), want)
    total = terms["bce"] + terms["dice"] + 0.25 * terms["boundary"]
    assert abs(float(terms["loss"].detach()) - float(total.detach())) <= 1e-5 * abs(float(total.detach()))


def test_graphed_forward_equals_eager_eval():
    import unet_amd
    dev = _dev()
    torch.manual_seed(5)
    model = unet_amd.UNet_SA(1, 1, bilinear=True).to(dev)
    im, _ = unet_amd.ellipse_batch(2, 96, seed=8)
    im = im.to(dev)
    model.eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        eager = model(im).clone()
    gf = unet_amd.GraphedForward(model, im, amp=True)
    out = gf(im)
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


@pytest.mark.parametrize("bilinear,amp", [(False, False), (True, True)])
def test_graph_captured_step_matches_eager(bilinear, amp):
    import unet_amd
    dev = _dev()
    im, mk = unet_amd.ellipse_batch(2, 64, seed=4)
    im2, mk2 = unet_amd.ellipse_batch(2, 64, seed=5)
    res = []
    for cls in (unet_amd.TrainStepper, unet_amd.GraphedTrainStepper):
        torch.manual_seed(0)
        model = unet_amd.UNet_SA(1, 1, bilinear=bilinear).to(dev)
        st = cls(model, lr=1e-4, amp=amp)
        for a, b in ((im, mk), (im2, mk2)):
            t = st.step(a.to(dev), b.to(dev))
        torch.cuda.synchronize()
        res.append((float(t["loss"].detach()), {k: v.clone() for k, v in model.state_dict().items()}))
    assert res[0][0] == res[1][0]
    for k, v in res[0][1].items():
        assert torch.equal(v, res[1][1][k]), k


class _NNUNetSA(nn.Module):
    """UNet_SA as a stock torch.nn graph (oracle/nn_ref.NNUNet's blocks, a SpatialAttention holder per decoder block):
    the CPU yardstick of the benchmarked shape, which no fixture holds."""

    def __init__(self, bilinear):
        super().__init__()
        from oracle.nn_ref import NNUNet
        self.net = NNUNet(1, 1, bilinear, (16, 32, 64, 128, 256))
        for j in range(1, 5):
            att = nn.Module()
            att.conv1 = nn.Conv2d(2, 1, 7, padding=3, bias=False)
            getattr(self.net, f"up{j}").attention = att
        self.n_classes = 1

    def forward(self, x):
        import torch.nn.functional as F
        net = self.net
        skips = [net.inc.double_conv(x)]
        for k in range(1, 5):
            d = getattr(net, f"down{k}").maxpool_conv
            skips.append(d[1].double_conv(d[0](skips[-1])))
        y = skips[-1]
        for j in range(1, 5):
            blk, skip = getattr(net, f"up{j}"), skips[4 - j]
            y = blk.up(y)
            dy, dx = skip.shape[2] - y.shape[2], skip.shape[3] - y.shape[3]
            y = F.pad(y, [dx // 2, dx - dx // 2, dy // 2, dy - dy // 2])
            pooled = torch.cat([skip.mean(dim=1, keepdim=True), skip.max(dim=1, keepdim=True)[0]], dim=1)
            skip = skip * torch.sigmoid(blk.attention.conv1(pooled))
            y = blk.conv.double_conv(torch.cat([skip, y], dim=1))
        return net.outc.conv(y)


def test_unet_sa_bf16_512_three_steps():
    """The benchmarked shape (B=8, 1x512x512, bf16): three steps stay finite; the step-0 loss sits within the yardstick of
    the CPU torch.nn graph (fp32 vs its own bf16 autocast result, forward only)."""
    import unet_amd
    dev = _dev()
    torch.manual_seed(2)
    model = unet_amd.UNet_SA(1, 1, bilinear=True)
    ref = _NNUNetSA(True)
    ref.net.load_state_dict({k: v for k, v in model.state_dict().items()})
    im, mk = unet_amd.ellipse_batch(8, 512, seed=21)
    from oracle import step_ref as S
    smooth = {}
    for tag, amp in (("ref32", False), ("ref16", True)):
        ref.train()
        with torch.no_grad(), torch.autocast("cpu", dtype=torch.bfloat16, enabled=amp):
            logits = ref(im)
        terms = S.seg_loss(logits.float(), mk, 1)
        smooth[tag] = float(terms["bce"] + terms["dice"])
    model = model.to(dev)
    st = unet_amd.TrainStepper(model, amp=True)
    for s in range(3):
        t = st.step(im.to(dev), mk.to(dev))
        assert np.isfinite(float(t["loss"].detach())) and bool(torch.isfinite(t["grad_norm"]).item())
        if s == 0:
            t0 = {k: v.detach().clone() for k, v in t.items() if torch.is_tensor(v)}
    assert all(torch.isfinite(v).all() for v in model.state_dict().values() if v.is_floating_point())
    c = Collector("UNet_SA 8x512x512")
    c.scalar("loss s0 (bce + dice)", float(t0["bce"] + t0["dice"]), smooth["ref32"], smooth["ref16"])
    c.done()
    _boundary_is_that_of_the_logits(t0, mk)
