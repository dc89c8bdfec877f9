"""The surface loss on the MI355X (csrc/surface_loss.hip) against the scipy / torch-float64 restatement tests/surface_loss_ref.py:
the signed distance maps bit for bit, value and gradient of both heads, determinism, batch independence (what the data-parallel
path relies on), two losses of one shape in flight (the workspace's rebuild path), the wiring into seg_loss / train_step, and the graph-captured stepper's refusal.

Bounds.  The maps are float32(sqrt(float64(exact integer))) on both sides: compared as bits.  Value: relative error <= 2e-5;
gradient: relative L2 <= 2e-5 -- the bound the project holds every fp32 kernel to op by op.  "Same bits" and "batch
independence" are equalities.  loss - w * surface against the option-off loss: one fp32 addition, so within one ulp of the
sum (its rounding error is at most half an ulp; w = 0.5 makes w * surface exact)."""
import numpy as np
import pytest
import torch

import surface_loss_ref as R

pytestmark = pytest.mark.gpu

TOL = 2e-5


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ maps
def _map_cases():
    rng = np.random.default_rng(11)
    one = R.blob_labels(rng, 1, 1, 1)                              # a single pixel: all of it the class
    small = R.blob_labels(rng, 2, 3, 5)
    small[1] = 2                                                   # an image that is entirely the class
    odd = R.blob_labels(rng, 3, 37, 100)
    odd[1] = rng.integers(0, 2, (37, 100))                         # an image without class 2
    sq = R.blob_labels(rng, 2, 64, 64)
    binary = R.blob_labels(rng, 2, 64, 64, cls=2, others=(0,))     # labels in {0, 2}: the binary head's data
    return [("1x1", one, (2,), False), ("full", small, (2,), False), ("full_k2", small, (2, 0), False),
            ("absent", odd, (2,), False), ("absent_k2", odd, (1, 2), False), ("square_k2", sq, (0, 2), False),
            ("binary", binary, (1,), True), ("binary_of_three", sq, (1,), True)]


@pytest.mark.parametrize("name,labels,classes,binary", _map_cases(), ids=[c[0] for c in _map_cases()])
def test_distance_maps_equal_the_restatement_bit_for_bit(name, labels, classes, binary):
    import unet_amd
    want = torch.from_numpy(R.phi_maps(labels, classes, binary=binary))
    got = unet_amd.surface_distance_map(torch.from_numpy(labels).cuda(), classes, binary=binary)
    assert got.dtype == torch.float32 and tuple(got.shape) == (len(classes),) + labels.shape
    assert torch.equal(_bits(got).cpu(), _bits(want)), (name, float((got.cpu() - want).abs().max()))
    if name == "absent":
        assert not _bits(got[0, 1]).any()                          # +0.0 everywhere
    if name == "full":
        assert (got[0, 1] <= 0).all() and (got[0, 1, 1:-1, 1:-1] < 0).all()


def test_border_comes_straight_from_the_int64_labels():
    import contour_metrics_ref as C
    from unet_amd import losses
    rng = np.random.default_rng(2)
    labels = R.blob_labels(rng, 2, 37, 100)
    got = losses.surface_border(torch.from_numpy(labels).cuda(), (2, 1)).cpu().numpy()
    want = np.stack([np.stack([C.border(labels[b] == c) for b in range(2)]) for c in (2, 1)]).astype(np.uint8)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    got2 = losses.surface_border(torch.from_numpy(labels).cuda(), (1,), mask_div=2).cpu().numpy()
    assert np.array_equal(got2[0], np.stack([C.border(labels[b] // 2 == 1) for b in range(2)]).astype(np.uint8))


# ------------------------------------------------------------------------------------------------ value and gradient
LOSS_CASES = [("binary", 1, None, (2, 33, 47)), ("c3_default", 3, None, (2, 33, 47)), ("c3_12", 3, (1, 2), (2, 33, 47)),
              ("c4", 4, None, (1, 17, 130))]
_CACHE = {}


def _case(name):
    """Inputs and the float64 reference of a case, computed once and shared."""
    if name not in _CACHE:
        _, n_classes, classes, (B, H, W) = next(c for c in LOSS_CASES if c[0] == name)
        rng = np.random.default_rng(len(name) + 7 * n_classes)
        labels = R.blob_labels(rng, B, H, W)
        g = torch.Generator().manual_seed(B * H + W + n_classes)
        logits = torch.randn(B, n_classes, H, W, generator=g) * 3
        z = logits.double().requires_grad_()
        value = R.surface_loss(z, labels, n_classes, classes)
        (grad,) = torch.autograd.grad(value, z)
        _CACHE[name] = (n_classes, classes, labels, logits, float(value.detach()), grad)
    return _CACHE[name]


def _run(logits, labels, n_classes, classes):
    import unet_amd
    z = logits.cuda().requires_grad_()
    v = unet_amd.surface_loss(z, torch.from_numpy(labels).cuda(), n_classes, classes)
    v.backward()
    return v.detach(), z.grad


@pytest.mark.parametrize("name", [c[0] for c in LOSS_CASES])
def test_value_and_gradient_against_float64(name):
    n_classes, classes, labels, logits, want_v, want_g = _case(name)
    v, g = _run(logits, labels, n_classes, classes)
    assert v.dtype == torch.float32 and v.dim() == 0 and g.shape == logits.shape
    rel_v = abs(float(v) - want_v) / abs(want_v)
    rel_g = float((g.cpu().double() - want_g).norm() / want_g.norm())
    print(f"{name}: value {float(v):.9g} (float64 {want_v:.9g}), relative error {rel_v:.3e}; gradient relative L2 {rel_g:.3e}")
    assert rel_v <= TOL, rel_v
    assert rel_g <= TOL, rel_g


@pytest.mark.parametrize("name", ["binary", "c3_12"])
def test_two_calls_return_the_same_bits(name):
    n_classes, classes, labels, logits, _, _ = _case(name)
    v0, g0 = _run(logits, labels, n_classes, classes)
    v1, g1 = _run(logits, labels, n_classes, classes)
    assert torch.equal(_bits(v0), _bits(v1)) and torch.equal(_bits(g0), _bits(g1))


@pytest.mark.parametrize("n_classes,classes", [(1, (1,)), (3, (1, 2))])
def test_gradient_of_a_batch_is_that_of_its_halves(n_classes, classes):
    """Each half is computed with the n_mean of the whole batch (world = 2), as a data-parallel rank would."""
    from unet_amd import losses
    rng = np.random.default_rng(4)
    B, H, W = 4, 24, 40
    labels = torch.from_numpy(R.blob_labels(rng, B, H, W)).cuda()
    g = torch.Generator().manual_seed(9)
    logits = (torch.randn(B, n_classes, H, W, generator=g) * 3).cuda()

    def grad(lo, hi, world):
        z = logits[lo:hi].clone().requires_grad_()
        lg = z.squeeze(1) if n_classes == 1 else z.permute(0, 2, 3, 1)
        weighted, _ = losses.SurfaceLossFn.apply(lg, labels[lo:hi], 2 if n_classes == 1 else 1, classes, 1.0, None, world)
        weighted.backward()
        return z.grad

    whole = grad(0, 4, 1)
    halves = torch.cat([grad(0, 2, 2), grad(2, 4, 2)])
    assert float(whole.abs().max()) > 0
    assert torch.equal(_bits(whole), _bits(halves))


@pytest.mark.parametrize("n_classes,classes", [(1, (1,)), (3, (1, 2)), (4, (2,))])
def test_two_losses_of_one_shape_in_flight_keep_their_own_distances(n_classes, classes):
    """Forward A, forward B (other labels, same shape: the same workspace), then backward A and backward B.  B's forward wrote
    its distances over A's, so A's backward forms them again (rebuild), and that in turn makes B's do so: each gradient is
    bit for bit the one computed alone."""
    from unet_amd import losses
    B, H, W = 2, 24, 40
    div = 2 if n_classes == 1 else 1
    labels = [torch.from_numpy(R.blob_labels(np.random.default_rng(s), B, H, W)).cuda() for s in (21, 22)]
    assert not torch.equal(labels[0], labels[1])
    g = torch.Generator().manual_seed(5)
    logits = [(torch.randn(B, n_classes, H, W, generator=g) * 3).cuda() for _ in range(2)]

    def forward(i):
        z = logits[i].clone().requires_grad_()
        lg = z.squeeze(1) if n_classes == 1 else z.permute(0, 2, 3, 1)
        weighted, _ = losses.SurfaceLossFn.apply(lg, labels[i], div, classes, 1.0)
        return z, weighted

    alone = []
    for i in range(2):
        z, weighted = forward(i)
        weighted.backward()
        alone.append(z.grad)
    assert float(alone[0].abs().max()) > 0 and not torch.equal(alone[0], alone[1])
    (za, wa), (zb, wb) = forward(0), forward(1)
    wa.backward()
    wb.backward()
    assert torch.equal(_bits(za.grad), _bits(alone[0]))
    assert torch.equal(_bits(zb.grad), _bits(alone[1]))
    # ... and with the distance-map helper using the workspace between a forward and its backward
    za, wa = forward(0)
    losses.surface_dist_map(labels[1], classes, div)
    wa.backward()
    assert torch.equal(_bits(za.grad), _bits(alone[0]))


# ------------------------------------------------------------------------------------------------ wiring
@pytest.mark.parametrize("n_classes", [1, 3])
def test_seg_loss_wiring(n_classes):
    import unet_amd
    rng = np.random.default_rng(6)
    B, H, W = 2, 32, 32
    labels = torch.from_numpy(R.blob_labels(rng, B, H, W)).cuda()
    g = torch.Generator().manual_seed(n_classes)
    logits = (torch.randn(B, n_classes, H, W, generator=g) * 3).cuda()
    off = unet_amd.seg_loss(logits, labels, n_classes)
    zero = unet_amd.seg_loss(logits, labels, n_classes, surface_weight=0.0, surface_classes=None)
    assert list(zero) == list(off) and "surface" not in zero
    for k in off:
        assert torch.equal(_bits(zero[k]), _bits(off[k])), k
    w = 0.5
    on = unet_amd.seg_loss(logits, labels, n_classes, surface_weight=w)
    assert set(on) - {"surface"} == set(off) - {"nan_flag"} and "surface" in on
    alone = unet_amd.surface_loss(logits, labels, n_classes)
    assert torch.equal(_bits(on["surface"]), _bits(alone))
    loss, surface, base = float(on["loss"]), float(on["surface"]), float(off["loss"])
    ulp = float(np.spacing(np.float32(abs(loss))))
    print(f"n_classes {n_classes}: loss {loss:.9g} = {base:.9g} + {w} * {surface:.9g}; off by {abs(loss - w * surface - base):.3e}, ulp {ulp:.3e}")
    assert surface != 0.0 and abs((loss - w * surface) - base) <= ulp
    for k in set(off) - {"loss", "nan_flag"}:
        assert torch.equal(_bits(on[k]), _bits(off[k])), k


def _flat_gradient(surface_weight):
    import unet_amd
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = unet_amd.UNet_T(1, 3, bilinear=True).to(dev)
    opt = unet_amd.FusedRMSprop(model.parameters())
    g = torch.Generator().manual_seed(1)
    images = torch.rand(2, 1, 32, 32, generator=g).to(dev)
    masks = torch.from_numpy(R.blob_labels(np.random.default_rng(1), 2, 32, 32)).to(dev)
    model.train()
    terms = unet_amd.train_step(model, opt, images, masks, amp=False, surface_weight=surface_weight)
    flat = opt.flat_g.clone()
    opt.close()
    return terms, flat


def test_one_train_step_with_the_term():
    off, g_off = _flat_gradient(0.0)
    on, g_on = _flat_gradient(0.1)
    assert "surface" in on and "surface" not in off
    for k in ("loss", "ce", "dice", "surface", "grad_norm"):
        assert torch.isfinite(on[k]).all(), k
    assert torch.isfinite(g_on).all() and not torch.equal(g_on, g_off)


def test_stepper_attribute_and_the_graph_stepper_refuses():
    import unet_amd
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = unet_amd.UNet_T(1, 1, bilinear=True).to(dev)
    with pytest.raises(RuntimeError, match="surface"):
        unet_amd.GraphedTrainStepper(model, amp=False, surface_weight=0.1)
    graphed = unet_amd.GraphedTrainStepper(model, amp=False)
    graphed.surface_weight = 0.1                                   # ... and when the weight is switched on later
    images = torch.rand(2, 1, 32, 32, device=dev)
    masks = torch.from_numpy(R.blob_labels(np.random.default_rng(1), 2, 32, 32)).to(dev)
    with pytest.raises(RuntimeError, match="surface"):
        graphed.step(images, masks)
    graphed.close()
    stepper = unet_amd.TrainStepper(model, amp=False)
    assert stepper.surface_weight == 0.0 and "surface" not in stepper.step(images, masks)
    stepper.surface_weight = 0.25                                  # a plain attribute: the epoch loop changes it between steps
    terms = stepper.step(images, masks)
    assert torch.isfinite(terms["surface"]).item() and torch.isfinite(terms["loss"]).item()
    stepper.close()
