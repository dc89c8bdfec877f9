"""The focal + Tversky loss on the MI355X (csrc/focal_loss.hip) against the torch-float64 restatement tests/focal_tversky_ref.py:
value and gradient of every head, finiteness where the probabilities underflow, determinism, the data-parallel sums, agreement
with today's CE / BCE kernels, the wiring into seg_loss / train_step, the graph-captured stepper's refusal and the C ABI's.

Shapes.  B=2, H=37, W=45: 3330 pixels are two blocks of the sums pass's 2048-element grid stride with a ragged tail;
B=1, H=1, W=3: fewer elements than a wave.  Labels: the last class never occurs (T_c = 0); the larger shape also runs with every
class present.  Logits N(0,1) * s, s in {1, 10, 100}: at 100 p_t underflows and u reaches 0 and 1.

Bounds.  total, focal, tversky: relative error <= 2e-5; gradient: relative L2 <= 2e-5 -- the bound the project holds every fp32
kernel to op by op (an fp32 torch restatement of the formulas measures 1e-7 to 3e-7 on these inputs; the kernels 4e-7 at most).  "Same bits" and the
half-batch gradients are equalities.  loss - focal - tversky against the other terms: total is one rounding of focal + tversky
and the boundary term joins by one fp32 addition (0.25 * boundary is exact), so within one ulp of the loss."""
import ctypes

import numpy as np
import pytest
import torch

import focal_tversky_ref as R

pytestmark = pytest.mark.gpu

TOL = 2e-5
SHAPES = {"two_blocks": (2, 37, 45), "sub_wave": (1, 1, 3)}
PRICES = [(0.5, 0.5), (0.3, 0.7)]
_CACHE = {}
SEED = 1          # a draw in which no term of the reference is 0 (see test_value_and_gradient_against_float64)


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _weights(C):
    return tuple(0.5 + 0.75 * c for c in range(C))


def _inputs(C, scale, shape, labels="absent"):
    """fp32 logits ([B,H,W] for C = 1, NHWC otherwise) and the int64 mask a head of C outputs is trained on, on the CPU, once.
    C = 1: dataset values {0,1,2}, the label is mask // 2.  labels = "absent": the last class never occurs."""
    key = (C, scale, shape, labels)
    if key not in _CACHE:
        B, H, W = SHAPES[shape]
        g = torch.Generator().manual_seed(SEED + 1000 * C + int(scale) + B * H)
        logits = torch.randn((B, H, W) if C == 1 else (B, H, W, C), generator=g) * scale
        if C == 1:
            mask = torch.randint(0, 2 if labels == "absent" else 3, (B, H, W), generator=g)
        else:
            mask = torch.randint(0, C - 1 if labels == "absent" else C, (B, H, W), generator=g)
        _CACHE[key] = (logits, mask)
    return _CACHE[key]


def _ref_form(C, logits, mask):
    """(z [n, classes], t [n], weights, Tversky classes) of the restatement for a head of C outputs."""
    if C == 1:
        return R.two_class_logits(logits.double()), (mask // 2).reshape(-1), _weights(2), (1,)
    return logits.double().reshape(-1, C), mask.reshape(-1), _weights(C), None


def _gpu(C, logits, mask, gamma, alpha, beta, weights=None, reduce_sums=None):
    from unet_amd import losses
    z = logits.cuda().requires_grad_()
    w = weights if weights is not None else _weights(2 if C == 1 else C)
    cls = (1,) if C == 1 else tuple(range(1, C))
    total, focal, tversky = losses.FocalTverskyLossFn.apply(z, mask.cuda(), 2 if C == 1 else 1, w, gamma, alpha, beta, cls, reduce_sums)
    total.backward()
    return (total.detach(), focal.detach(), tversky.detach()), z.grad


# ------------------------------------------------------------------------------------------------ value and gradient
@pytest.mark.parametrize("scale", [1.0, 10.0, 100.0])
@pytest.mark.parametrize("gamma", [0.0, 0.5, 2.0])
@pytest.mark.parametrize("C", [1, 2, 3, 8])
def test_value_and_gradient_against_float64(C, gamma, scale):
    worst = 0.0
    for shape, labels in (("two_blocks", "absent"), ("sub_wave", "absent"), ("two_blocks", "all")):
        logits, mask = _inputs(C, scale, shape, labels)
        z, t, w, cls = _ref_form(C, logits, mask)
        if labels == "absent":
            assert int((t == z.shape[1] - 1).sum()) == 0                       # T_c = 0 for the last class
        for alpha, beta in PRICES:
            want = [float(v) for v in R.loss_terms(z, t, w, gamma, alpha, beta, cls)]
            # (three pixels at s = 100 can all be easy: focal and tversky are then exactly 0 in float64 and a relative error says
            # nothing; SEED is a draw where that does not happen)
            assert min(abs(x) for x in want) > 1e-12, want
            want_g = R.closed_form_gradient(z, t, w, gamma, alpha, beta, cls)
            want_g = want_g[:, 1].reshape(logits.shape) if C == 1 else want_g.reshape(logits.shape)
            got, g = _gpu(C, logits, mask, gamma, alpha, beta)
            assert all(v.dtype == torch.float32 and v.dim() == 0 for v in got) and g.shape == logits.shape
            assert all(torch.isfinite(v).item() for v in got) and torch.isfinite(g).all()      # also at s = 100
            rel = [abs(float(v) - x) / abs(x) for v, x in zip(got, want)]
            rel_g = float((g.cpu().double() - want_g).norm() / want_g.norm())
            print(f"C {C} gamma {gamma} s {scale} {shape}/{labels} a/b {alpha}/{beta}: total {float(got[0]):.9g} focal {float(got[1]):.9g} "
                  f"tversky {float(got[2]):.9g}; relative errors {rel[0]:.3e} {rel[1]:.3e} {rel[2]:.3e}; gradient relative L2 {rel_g:.3e}")
            worst = max(worst, rel_g, *rel)
            assert max(rel) <= TOL, rel
            assert rel_g <= TOL, rel_g
    print(f"worst {worst:.3e}")


@pytest.mark.parametrize("gamma", [1.0, 1.5])
def test_the_other_exponent_paths(gamma):
    """gamma = 1 (a multiplication) and a gamma that takes exp2(gamma log2 u), on the 3-class head."""
    logits, mask = _inputs(3, 10.0, "two_blocks", "all")
    z, t, w, cls = _ref_form(3, logits, mask)
    want = [float(v) for v in R.loss_terms(z, t, w, gamma, 0.3, 0.7, cls)]
    want_g = R.closed_form_gradient(z, t, w, gamma, 0.3, 0.7, cls).reshape(logits.shape)
    got, g = _gpu(3, logits, mask, gamma, 0.3, 0.7)
    rel = [abs(float(v) - x) / abs(x) for v, x in zip(got, want)]
    rel_g = float((g.cpu().double() - want_g).norm() / want_g.norm())
    print(f"gamma {gamma}: relative errors {rel}; gradient relative L2 {rel_g:.3e}")
    assert max(rel) <= TOL and rel_g <= TOL


# ------------------------------------------------------------------------------------------------ reproducibility
@pytest.mark.parametrize("C", [1, 3, 8])
def test_two_calls_return_the_same_bits(C):
    logits, mask = _inputs(C, 10.0, "two_blocks", "all")
    v0, g0 = _gpu(C, logits, mask, 0.5, 0.3, 0.7)
    v1, g1 = _gpu(C, logits, mask, 0.5, 0.3, 0.7)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(v0, v1)) and torch.equal(_bits(g0), _bits(g1))


@pytest.mark.parametrize("C", [1, 3, 8])
@pytest.mark.parametrize("gamma", [0.0, 0.5, 2.0])
def test_half_batches_with_the_whole_sums_give_the_whole_gradient(C, gamma):
    """What a data-parallel rank computes: its own half of the logits, the sums of the global batch."""
    logits, mask = _inputs(C, 10.0, "two_blocks", "all")
    seen = []
    whole_v, whole_g = _gpu(C, logits, mask, gamma, 0.3, 0.7, reduce_sums=lambda s: seen.append(s.clone()))
    assert len(seen) == 1 and seen[0].numel() == 2 + 3 * (2 if C == 1 else C)
    halves = [_gpu(C, logits[b:b + 1], mask[b:b + 1], gamma, 0.3, 0.7, reduce_sums=lambda s: s.copy_(seen[0])) for b in range(2)]
    assert float(whole_g.abs().max()) > 0
    assert torch.equal(_bits(torch.cat([h[1] for h in halves])), _bits(whole_g))
    for v, _ in halves:                                                             # ... and the value is the global batch's
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(v, whole_v))


# ------------------------------------------------------------------------------------------------ today's kernels
@pytest.mark.parametrize("C", [1, 2, 3, 8])
def test_gamma_zero_unit_weights_agree_with_todays_cross_entropy(C):
    """focal(gamma = 0, w = 1) is the CE / BCE mean of uh_ce_dice_sums / uh_bce_dice_sums; today's gradient with its Dice part
    switched off (w_dice = 0) is the restatement's focal-only gradient, and so is the new gradient less the Tversky part."""
    import unet_amd
    from unet_amd import losses
    from unet_amd._lib import LIB
    logits, mask = _inputs(C, 1.0, "two_blocks", "all")
    ones = (1.0,) * (2 if C == 1 else C)
    (_, focal, _), g_new = _gpu(C, logits, mask, 0.0, 0.3, 0.7, weights=ones)
    bchw = logits.cuda().unsqueeze(1) if C == 1 else logits.cuda().permute(0, 3, 1, 2)
    terms = unet_amd.seg_loss(bchw, mask.cuda(), C)
    today = float(terms["bce" if C == 1 else "ce"])
    print(f"C {C}: focal {float(focal):.9g}, today's CE {today:.9g}, relative difference {abs(float(focal) - today) / today:.3e}")
    assert abs(float(focal) - today) <= TOL * today
    # today's gradient stream, CE part only
    lg, mk = logits.cuda().contiguous(), mask.cuda()
    n = mk.numel()
    dl = torch.empty_like(lg)
    ws = losses.loss_workspace(lg.device)
    if C == 1:
        sums = torch.empty(4, dtype=torch.float32, device=lg.device)
        LIB.call("uh_bce_dice_sums", lg.data_ptr(), mk.data_ptr(), 2, None, n, sums.data_ptr(), ws.data_ptr(), ws.numel(), None)
        LIB.call("uh_bce_dice_grad", lg.data_ptr(), mk.data_ptr(), 2, None, n, sums.data_ptr(), float(n), 1.0, 0.0, None, dl.data_ptr(), None)
    else:
        sums = torch.empty(1 + 3 * C, dtype=torch.float32, device=lg.device)
        LIB.call("uh_ce_dice_sums", lg.data_ptr(), mk.data_ptr(), n, C, sums.data_ptr(), ws.data_ptr(), ws.numel(), None)
        LIB.call("uh_ce_dice_grad", lg.data_ptr(), mk.data_ptr(), n, C, sums.data_ptr(), float(n), 1.0, 0.0, None, dl.data_ptr(), None)
    torch.cuda.synchronize()
    z, t, _, cls = _ref_form(C, logits, mask)
    pick = (lambda g: g[:, 1].reshape(logits.shape)) if C == 1 else (lambda g: g.reshape(logits.shape))
    want = pick(R.focal_gradient(z, t, ones, 0.0))
    tv = pick(R.tversky_gradient(z, t, 0.3, 0.7, cls))
    rel_today = float((dl.cpu().double() - want).norm() / want.norm())
    rel_new = float((g_new.cpu().double() - tv - want).norm() / want.norm())
    print(f"C {C}: today's CE gradient against the focal-only restatement {rel_today:.3e}; the new one less Tversky {rel_new:.3e}")
    assert rel_today <= TOL and rel_new <= TOL


# ------------------------------------------------------------------------------------------------ wiring
@pytest.mark.parametrize("n_classes", [1, 3])
def test_seg_loss_wiring(n_classes):
    import unet_amd
    B, H, W = 2, 32, 32
    g = torch.Generator().manual_seed(n_classes)
    logits = (torch.randn(B, n_classes, H, W, generator=g) * 3).cuda()
    labels = torch.randint(0, 3, (B, H, W), generator=g).cuda()
    off = unet_amd.seg_loss(logits, labels, n_classes)
    none = unet_amd.seg_loss(logits, labels, n_classes, loss=None)
    assert list(none) == list(off) and "focal" not in none
    for k in off:
        assert torch.equal(_bits(none[k]), _bits(off[k])), k                         # loss=None: today's bits
    cfg = unet_amd.LossConfig(gamma=2.0, weights=(0.5, 2.0) if n_classes == 1 else (0.5, 1.0, 4.0))
    on = unet_amd.seg_loss(logits, labels, n_classes, loss=cfg)
    assert set(on) == {"loss", "focal", "tversky", "boundary"}
    assert torch.equal(_bits(unet_amd.seg_loss(logits, labels, n_classes, loss=cfg.spec())["loss"]), _bits(on["loss"]))
    alone = unet_amd.focal_tversky_loss(logits, labels, n_classes, cfg)
    loss, focal, tversky, bnd = (float(on[k]) for k in ("loss", "focal", "tversky", "boundary"))
    w_b = 0.25 if n_classes == 1 else 0.0
    assert torch.equal(_bits(on["boundary"]), _bits(off["boundary"]))               # the boundary term is the pair's
    assert abs(float(alone) - (focal + tversky)) <= float(np.spacing(np.float32(abs(float(alone)))))
    ulp = float(np.spacing(np.float32(abs(loss))))
    print(f"n_classes {n_classes}: loss {loss:.9g} = focal {focal:.9g} + tversky {tversky:.9g} + {w_b} * {bnd:.9g}; off by "
          f"{abs(loss - focal - tversky - w_b * bnd):.3e}, ulp {ulp:.3e}")
    assert focal > 0 and tversky > 0 and (bnd > 0) == (n_classes == 1)
    assert abs((loss - focal - tversky) - w_b * bnd) <= ulp
    # the surface term keeps working on top
    both = unet_amd.seg_loss(logits, labels, n_classes, loss=cfg, surface_weight=0.5)
    assert set(both) == set(on) | {"surface"}
    surface = unet_amd.surface_loss(logits, labels, n_classes)
    assert torch.equal(_bits(both["surface"]), _bits(surface))
    assert abs(float(both["loss"]) - (loss + 0.5 * float(surface))) <= 2 * float(np.spacing(np.float32(abs(float(both["loss"])))))
    # and the gradient reaches the logits through every term
    z = logits.clone().requires_grad_()
    unet_amd.seg_loss(z, labels, n_classes, loss=cfg)["loss"].backward()
    assert torch.isfinite(z.grad).all() and float(z.grad.abs().max()) > 0


@pytest.mark.parametrize("n_classes", [1, 3])
def test_one_train_step_with_the_option(n_classes):
    import unet_amd
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = unet_amd.UNet_T(1, n_classes, bilinear=True).to(dev)
    opt = unet_amd.FusedRMSprop(model.parameters())
    g = torch.Generator().manual_seed(1)
    images = torch.rand(2, 1, 32, 32, generator=g).to(dev)
    masks = torch.randint(0, 3, (2, 32, 32), generator=g).to(dev)
    model.train()
    before = opt.flat_p.clone()
    terms = unet_amd.train_step(model, opt, images, masks, amp=False, loss=unet_amd.LossConfig())
    assert "focal" in terms and "tversky" in terms and not ({"ce", "bce", "dice"} & set(terms))
    for k in ("loss", "focal", "tversky", "grad_norm"):
        assert torch.isfinite(terms[k]).all(), k
    assert float(terms["grad_norm"]) > 0 and not torch.equal(opt.flat_p, before)
    opt.close()


def test_the_stepper_takes_the_option_and_the_graph_stepper_refuses():
    import unet_amd
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = unet_amd.UNet_T(1, 3, bilinear=True).to(dev)
    with pytest.raises(RuntimeError, match="focal"):
        unet_amd.GraphedTrainStepper(model, amp=False, loss="focal=2")
    with pytest.raises(ValueError, match="class weights"):
        unet_amd.TrainStepper(model, amp=False, loss="focal=2,weights=1+2")         # two weights, three classes
    images = torch.rand(2, 1, 32, 32, device=dev)
    masks = torch.randint(0, 3, (2, 32, 32), device=dev)
    stepper = unet_amd.TrainStepper(model, amp=True, loss="focal=2,tversky=0.3/0.7")
    assert stepper.loss == unet_amd.LossConfig()
    terms = stepper.step(images, masks)
    assert torch.isfinite(terms["focal"]).item() and torch.isfinite(terms["tversky"]).item() and torch.isfinite(terms["loss"]).item()
    stepper.close()
    plain = unet_amd.TrainStepper(model, amp=False)
    assert plain.loss is None and "focal" not in plain.step(images, masks)
    plain.close()


# ------------------------------------------------------------------------------------------------ the C ABI
def test_each_entry_point_refuses_bad_arguments_with_an_error_code():
    """Called from the CPU side with stand-in pointers: the checks sit in front of the launches, nothing is followed."""
    import unet_amd  # noqa: F401
    from unet_amd._lib import LIB
    dll = LIB.load()
    P = 4096
    big = LIB.query("uh_loss_ws_bytes", 100)
    w3, bad_w = (ctypes.c_float * 3)(1, 1, 1), (ctypes.c_float * 3)(1, 0, 1)
    k2, bad_k = (ctypes.c_int * 2)(1, 2), (ctypes.c_int * 2)(1, 3)
    assert dll.uh_focal_tversky_sums(P, P, 1, 100, 3, bad_w, 2.0, P, P, big, None) == -1
    assert dll.uh_focal_tversky_sums(P, P, 1, 100, 3, w3, -1.0, P, P, big, None) == -1
    assert dll.uh_focal_tversky_sums(P, P, 1, 100, 9, w3, 2.0, P, P, big, None) == -1
    assert dll.uh_focal_tversky_sums(P, P, 1, 100, 3, w3, 2.0, P, P, big - 1, None) == -1
    assert dll.uh_focal_tversky_finish(P, 3, 0.0, 0.0, k2, 2, P, None) == -1
    assert dll.uh_focal_tversky_finish(P, 3, 0.3, 0.7, bad_k, 2, P, None) == -1
    assert dll.uh_focal_tversky_finish(P, 0, 0.3, 0.7, k2, 2, P, None) == -1
    assert dll.uh_focal_tversky_grad(P, P, 1, 100, 3, bad_w, 2.0, 0.3, 0.7, k2, 2, P, None, P, None) == -1
    assert dll.uh_focal_tversky_grad(P, P, 1, 100, 3, w3, 2.0, 0.3, 0.7, bad_k, 2, P, None, P, None) == -1
    assert dll.uh_focal_tversky_grad(P, P, 1, 100, 3, w3, 2.0, -0.3, 0.7, k2, 2, P, None, P, None) == -1
    assert b"alpha" in dll.uh_last_error()
