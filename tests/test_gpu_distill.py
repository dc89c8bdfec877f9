"""Knowledge distillation on the MI355X (csrc/distill_loss.hip) against the torch-float64 restatement tests/distill_ref.py: value,
agreement and gradient of every head, finiteness where the probabilities underflow, the exact zero of equal logits,
determinism, the data-parallel sums, gradient scaling, bf16 logits, the wiring into seg_loss / train_step / TrainStepper, the
frozen teacher, the batch-invariant teacher forward, the step record, and the refusals.

Shapes (those of the focal tests).  B=2, H=37, W=45: 3330 pixels are two blocks of the sums pass's 2048-element grid stride with
a ragged tail; B=1, H=1, W=3: fewer elements than a wave.  Student and teacher logits are independent N(0,1) * s draws,
s in {1, 10, 100}: at 100 and T = 0.5 the softened probabilities underflow to 0.

Bounds.  kd: relative error <= 2e-5; gradient: relative L2 <= 2e-5 -- the bound the project holds every fp32 loss kernel to (an
fp32 torch restatement of the kernel's form measures at most 1.0e-6 in the value and under 5e-7 in the gradient on these draws).
At T = 4 the value of the 3-pixel shape is lost to cancellation in fp32 itself (1.6e-5 for C = 1, s = 1): T = 4 is held to the
gradient bound and to finiteness only.  agree is an equality: the count over n, rounded once to fp32.  "Same bits", the exact
zero, the half-batch gradients and the power-of-two gradient scale are equalities.
Measured on an MI355X, worst case over every case of test_value_and_gradient_against_float64 (it prints each figure and a line
"worst" per head and scale): value 8.7e-7 (C = 8, s = 1, the 3-pixel shape), gradient 5.5e-7."""
import ctypes

import numpy as np
import pytest
import torch

import distill_ref as R

pytestmark = pytest.mark.gpu

TOL = 2e-5
SHAPES = {"two_blocks": (2, 37, 45), "sub_wave": (1, 1, 3)}
HEADS = [1, 2, 3, 8]
_CACHE = {}
SEED = 3


def _bits(t):
    return t.detach().contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _inputs(C, scale, shape):
    """fp32 student and teacher logits ([B,H,W] for C = 1, NHWC otherwise), independent draws, on the CPU, once."""
    key = (C, scale, shape)
    if key not in _CACHE:
        B, H, W = SHAPES[shape]
        g = torch.Generator().manual_seed(SEED + 1000 * C + int(scale) + B * H)
        dims = (B, H, W) if C == 1 else (B, H, W, C)
        _CACHE[key] = (torch.randn(dims, generator=g) * scale, torch.randn(dims, generator=g) * scale)
    return _CACHE[key]


def _ref_form(C, logits):
    return R.two_class_logits(logits.double()) if C == 1 else logits.double().reshape(-1, C)


def _ref(C, z, v, T, w=1.0):
    """(kd, agree as the fp32 the kernel must return, w * d kd / dz shaped like z) of the restatement."""
    zz, vv = _ref_form(C, z), _ref_form(C, v)
    kd, agree = R.loss_terms(zz, vv, T)
    n = zz.shape[0]
    count = int((R.first_argmax(zz) == R.first_argmax(vv)).sum())
    assert float(agree) == count / n
    g = w * R.closed_form_gradient(zz, vv, T)
    g = g[:, 1].reshape(z.shape) if C == 1 else g.reshape(z.shape)
    return float(kd), np.float32(count / n), g


def _gpu(z, v, T, w=1.0, reduce_sums=None, world=1, seed_grad=None):
    from unet_amd import losses
    zz = z.cuda().requires_grad_()
    vv = v.cuda().requires_grad_()                                    # asks for a gradient: it must not get one
    weighted, kd, agree = losses.DistillLossFn.apply(zz, vv, T, w, reduce_sums, world)
    assert weighted.requires_grad and not kd.requires_grad and not agree.requires_grad
    if seed_grad is None:
        weighted.backward()
    else:
        weighted.backward(gradient=torch.tensor(seed_grad, device="cuda"))
    assert vv.grad is None
    return (weighted.detach(), kd.detach(), agree.detach()), zz.grad


# ------------------------------------------------------------------------------------------------ value and gradient
@pytest.mark.parametrize("scale", [1.0, 10.0, 100.0])
@pytest.mark.parametrize("C", HEADS)
def test_value_and_gradient_against_float64(C, scale):
    worst_v = worst_g = 0.0
    for shape in SHAPES:
        z, v = _inputs(C, scale, shape)
        for T in (0.5, 1.0, 2.0, 4.0):
            for w in (1.0, 0.75):
                want_kd, want_agree, want_g = _ref(C, z, v, T, w)
                assert want_kd > 1e-12 and float(want_g.norm()) > 0
                (weighted, kd, agree), g = _gpu(z, v, T, w)
                assert all(t.dtype == torch.float32 and t.dim() == 0 for t in (weighted, kd, agree)) and g.shape == z.shape
                assert all(torch.isfinite(t).item() for t in (weighted, kd, agree)) and torch.isfinite(g).all()   # also at s = 100
                rel = abs(float(kd) - want_kd) / want_kd
                rel_w = abs(float(weighted) - w * want_kd) / (w * want_kd)
                rel_g = float((g.cpu().double() - want_g).norm() / want_g.norm())
                print(f"C {C} s {scale} {shape} T {T} w {w}: kd {float(kd):.9g} (float64 {want_kd:.9g}) relative error {rel:.3e}, "
                      f"weighted {rel_w:.3e}; agree {float(agree):.9g}; gradient relative L2 {rel_g:.3e}")
                assert np.float32(float(agree)) == want_agree, (float(agree), want_agree)
                assert rel_g <= TOL, rel_g
                worst_g = max(worst_g, rel_g)
                if T != 4.0:                                          # (T = 4: the gradient and finiteness only, see above)
                    assert rel <= TOL and rel_w <= TOL, (rel, rel_w)
                    worst_v = max(worst_v, rel, rel_w)
    print(f"worst: value {worst_v:.3e}, gradient {worst_g:.3e}")


@pytest.mark.parametrize("C", HEADS)
def test_everything_is_finite_where_the_probabilities_underflow(C):
    for shape in SHAPES:
        z, v = _inputs(C, 100.0, shape)
        for T in (0.5, 1.0, 2.0, 4.0):
            out, g = _gpu(z, v, T)
            assert all(torch.isfinite(t).item() for t in out) and torch.isfinite(g).all(), (shape, T)
            assert float(out[1]) > 0 and 0.0 <= float(out[2]) <= 1.0
    # logits of magnitude 100 exactly, opposite on the two sides: every q_c but one is 0
    dims = (1, 4, 5) if C == 1 else (1, 4, 5, C)
    z = torch.full(dims, 100.0)
    if C > 1:
        z[..., 1:] = -100.0
    out, g = _gpu(z, -z, 0.5)
    assert all(torch.isfinite(t).item() for t in out) and torch.isfinite(g).all()
    assert float(out[2]) == 0.0 and float(out[1]) > 0


# ------------------------------------------------------------------------------------------------ exact zero, same bits
@pytest.mark.parametrize("scale", [1.0, 100.0])
@pytest.mark.parametrize("C", HEADS)
def test_a_teacher_equal_to_the_student_gives_exact_zeros(C, scale):
    for shape in SHAPES:
        z, _ = _inputs(C, scale, shape)
        for T in (0.5, 2.0, 3.0, 4.0):                                           # (1 / 3: a scale that is no power of two)
            (weighted, kd, agree), g = _gpu(z, z.clone(), T, 0.75)
            assert int(_bits(kd)) == 0 and int(_bits(weighted)) == 0            # the bits of +0.0
            assert not bool((_bits(g) != 0).any())                              # every element +0.0
            assert float(agree) == 1.0


@pytest.mark.parametrize("C", [1, 3, 8])
def test_two_calls_return_the_same_bits(C):
    z, v = _inputs(C, 10.0, "two_blocks")
    v0, g0 = _gpu(z, v, 2.0)
    v1, g1 = _gpu(z, v, 2.0)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(v0, v1)) and torch.equal(_bits(g0), _bits(g1))


# ------------------------------------------------------------------------------------------------ data parallel, scaling, dtypes
@pytest.mark.parametrize("C", [1, 3, 8])
def test_half_batches_with_the_summed_sums_give_the_whole_gradient(C):
    """What a rank of a two-rank run computes: its own half of both tensors, the two ranks' sums added, world = 2."""
    z, v = _inputs(C, 10.0, "two_blocks")
    whole_v, whole_g = _gpu(z, v, 2.0, 0.75)
    own = []
    for b in range(2):
        _gpu(z[b:b + 1], v[b:b + 1], 2.0, 0.75, reduce_sums=lambda s: own.append(s.clone()), world=2)
    assert len(own) == 2 and all(s.numel() == 2 and s.dtype == torch.float32 for s in own)
    halves = [_gpu(z[b:b + 1], v[b:b + 1], 2.0, 0.75, reduce_sums=lambda s, b=b: s.add_(own[1 - b]), world=2) for b in range(2)]
    assert float(whole_g.abs().max()) > 0
    assert torch.equal(_bits(torch.cat([h[1] for h in halves])), _bits(whole_g))
    for (weighted, kd, agree), _ in halves:                                    # ... and the value is the global batch's
        assert abs(float(kd) - float(whole_v[1])) <= TOL * float(whole_v[1])
        assert abs(float(weighted) - float(whole_v[0])) <= TOL * float(whole_v[0])
        assert float(agree) == float(whole_v[2])                               # (counts below 2^24 add exactly)
    # a rank alone with world = 2 and no reducer: its own sums over the global pixel count
    alone, g_alone = _gpu(z[:1], v[:1], 2.0, 0.75, world=2)
    assert torch.equal(_bits(g_alone), _bits(halves[0][1]))
    npix = 2 * 37 * 45
    assert abs(float(alone[1]) - 2.0 * 2.0 / npix * float(own[0][0])) <= TOL * float(alone[1])          # T^2 / n_mean * sum KL


@pytest.mark.parametrize("C", [1, 3])
def test_the_seed_gradient_scales_the_gradient_exactly(C):
    z, v = _inputs(C, 10.0, "two_blocks")
    _, g1 = _gpu(z, v, 2.0)
    for k in (4.0, 0.25, -2.0):
        _, gk = _gpu(z, v, 2.0, seed_grad=k)
        assert torch.equal(_bits(gk), _bits(g1 * k)), k


@pytest.mark.parametrize("C", [1, 3])
def test_bf16_logits_give_the_fp32_result_of_their_upcast(C):
    z, v = _inputs(C, 10.0, "two_blocks")
    zb, vb = z.bfloat16(), v.bfloat16()
    for s, t in ((zb, vb), (zb, vb.float()), (zb.float(), vb)):
        want, want_g = _gpu(s.float(), t.float(), 2.0)
        got, g = _gpu(s, t, 2.0)
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(got, want))
        assert g.dtype == s.dtype and torch.equal(_bits(g), _bits(want_g.to(s.dtype)))


# ------------------------------------------------------------------------------------------------ wiring
@pytest.mark.parametrize("n_classes", [1, 3])
def test_seg_loss_wiring(n_classes):
    import unet_amd
    B, H, W = 2, 32, 32
    g = torch.Generator().manual_seed(n_classes)
    logits = (torch.randn(B, n_classes, H, W, generator=g) * 3).cuda()
    teacher = (torch.randn(B, n_classes, H, W, generator=g) * 3).cuda()
    labels = torch.randint(0, 3, (B, H, W), generator=g).cuda()
    off = unet_amd.seg_loss(logits, labels, n_classes)
    none = unet_amd.seg_loss(logits, labels, n_classes, distill=None, teacher_logits=None)
    assert list(none) == list(off) and "kd" not in none
    for k in off:
        assert torch.equal(_bits(none[k]), _bits(off[k])), k                         # distill=None: today's bits
    cfg = unet_amd.DistillConfig("unused.pth", T=2.0, w=0.5)
    on = unet_amd.seg_loss(logits, labels, n_classes, distill=cfg, teacher_logits=teacher)
    assert set(on) == (set(off) - {"nan_flag"}) | {"kd", "kd_agree"}
    assert torch.equal(_bits(unet_amd.seg_loss(logits, labels, n_classes, distill=cfg.spec(), teacher_logits=teacher)["loss"]),
                       _bits(on["loss"]))
    alone = unet_amd.distill_loss(logits, teacher, n_classes, cfg)
    loss, kd, agree = float(on["loss"]), float(on["kd"]), float(on["kd_agree"])
    ulp = float(np.spacing(np.float32(abs(loss))))
    print(f"n_classes {n_classes}: loss {loss:.9g} = {float(off['loss']):.9g} + 0.5 * kd {kd:.9g}; off by "
          f"{abs((loss - float(off['loss'])) - 0.5 * kd):.3e}, ulp {ulp:.3e}; agree {agree:.6f}")
    assert kd > 0 and 0.0 < agree < 1.0 and float(alone) == 0.5 * kd
    assert abs((loss - float(off["loss"])) - 0.5 * kd) <= ulp
    for k in off:
        if k not in ("loss", "nan_flag"):
            assert torch.equal(_bits(on[k]), _bits(off[k])), k                       # the other terms are untouched
    with pytest.raises(ValueError, match="teacher_logits"):
        unet_amd.seg_loss(logits, labels, n_classes, distill=cfg)
    # the student logits' gradient is the sum of the two nodes' gradients; the teacher's logits get none
    grads = []
    for fn in (lambda z: unet_amd.seg_loss(z, labels, n_classes, distill=cfg, teacher_logits=teacher)["loss"],
               lambda z: unet_amd.seg_loss(z, labels, n_classes)["loss"],
               lambda z: unet_amd.distill_loss(z, teacher, n_classes, cfg)):
        z = logits.clone().requires_grad_()
        fn(z).backward()
        grads.append(z.grad)
    assert float(grads[2].abs().max()) > 0
    assert torch.equal(_bits(grads[0]), _bits(grads[1] + grads[2]))
    # on top of the focal / Tversky loss and the surface term
    both = unet_amd.seg_loss(logits, labels, n_classes, loss="focal=2", surface_weight=0.5, distill=cfg, teacher_logits=teacher)
    assert {"focal", "tversky", "surface", "kd", "kd_agree"} <= set(both) and torch.equal(_bits(both["kd"]), _bits(on["kd"]))


def _teacher_file(path, n_classes, seed, arch="UNet_T", bilinear=True):
    import unet_amd
    from conftest import randomize_bn_
    torch.manual_seed(seed)
    model = getattr(unet_amd, arch)(1, n_classes, bilinear=bilinear)
    randomize_bn_(model, seed)                                         # running statistics that are not the initial 0 / 1
    return unet_amd.save_checkpoint(model, str(path), mask_values=[0, 1, 2])


@pytest.mark.parametrize("n_classes", [1, 3])
def test_one_train_step_moves_the_student_and_nothing_of_the_teacher(tmp_path, n_classes):
    import unet_amd
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = unet_amd.UNet_T(1, n_classes, bilinear=True).to(dev)
    cfg = unet_amd.DistillConfig(_teacher_file(tmp_path / "teacher.pth", n_classes, seed=7), arch="UNet_T", T=2.0, w=1.0)
    distiller = unet_amd.Distiller(cfg, 1, n_classes, dev, amp=False)
    teacher = distiller.teacher
    assert not teacher.training and not any(p.requires_grad for p in teacher.parameters())
    assert isinstance(teacher, unet_amd.UNet_T) and teacher.bilinear                # read off the checkpoint's keys
    frozen = {k: v.clone() for k, v in teacher.state_dict().items()}
    keys = list(model.state_dict())
    opt = unet_amd.FusedRMSprop(model.parameters())
    g = torch.Generator().manual_seed(1)
    images = torch.rand(2, 1, 32, 48, generator=g).to(dev)
    masks = torch.randint(0, 3, (2, 32, 48), generator=g).to(dev)
    model.train()
    before = opt.flat_p.clone()
    terms = unet_amd.train_step(model, opt, images, masks, amp=False, distill=distiller)
    for k in ("loss", "kd", "kd_agree", "grad_norm"):
        assert torch.isfinite(terms[k]).all(), k
    assert float(terms["kd"]) > 0 and 0.0 <= float(terms["kd_agree"]) <= 1.0
    assert float(terms["grad_norm"]) > 0 and not torch.equal(opt.flat_p, before)     # the parameters move
    after = teacher.state_dict()
    assert list(after) == list(frozen)
    for k, v in frozen.items():                                                      # parameters and BatchNorm buffers alike
        assert torch.equal(after[k], v) and (not v.is_floating_point() or torch.equal(_bits(after[k]), _bits(v))), k
    assert all(p.grad is None for p in teacher.parameters()) and not teacher.training
    assert list(model.state_dict()) == keys and not any("teacher" in k for k in keys)
    lo, hi = opt.flat_p.data_ptr(), opt.flat_p.data_ptr() + opt.flat_p.numel() * 4
    assert not any(lo <= p.data_ptr() < hi for p in teacher.parameters())            # no teacher in the flat buffer
    opt.close()


def test_a_teacher_with_another_head_is_refused_naming_both_sides(tmp_path):
    import unet_amd
    path = _teacher_file(tmp_path / "teacher.pth", 3, seed=7)
    with pytest.raises(ValueError, match="head of 3 outputs, the student one of 1"):
        unet_amd.Distiller(unet_amd.DistillConfig(path, arch="UNet_T"), 1, 1, "cuda:0")
    with pytest.raises(ValueError, match="takes 1 input channels, the student 3"):
        unet_amd.Distiller(unet_amd.DistillConfig(path, arch="UNet_T"), 3, 3, "cuda:0")
    with pytest.raises(ValueError, match="does not hold a UNet_S"):
        unet_amd.Distiller(unet_amd.DistillConfig(path, arch="UNet_S"), 1, 3, "cuda:0")


@pytest.mark.parametrize("amp", [True, False])
def test_the_teacher_logits_of_an_item_do_not_depend_on_the_batch(tmp_path, amp):
    import unet_amd
    dev = torch.device("cuda:0")
    cfg = unet_amd.DistillConfig(_teacher_file(tmp_path / "teacher.pth", 3, seed=7, bilinear=False), arch="UNet_T")
    distiller = unet_amd.Distiller(cfg, 1, 3, dev, amp=amp)
    assert not distiller.teacher.bilinear
    x = torch.rand(3, 1, 32, 48, generator=torch.Generator().manual_seed(2)).to(dev)
    whole = distiller.teacher_logits(x)
    assert whole.shape == (3, 3, 32, 48) and not whole.requires_grad and torch.isfinite(whole).all()
    for i in range(3):
        assert torch.equal(_bits(whole[i:i + 1].float()), _bits(distiller.teacher_logits(x[i:i + 1]).float())), i


def _plain_step(seed=0):
    """One fp32 TrainStepper step without the option on a freshly seeded UNet_T: (loss bits, parameter bits)."""
    import unet_amd
    dev = torch.device("cuda:0")
    torch.manual_seed(seed)
    model = unet_amd.UNet_T(1, 3, bilinear=True).to(dev)
    g = torch.Generator().manual_seed(4)
    images = torch.rand(2, 1, 32, 48, generator=g).to(dev)
    masks = torch.randint(0, 3, (2, 32, 48), generator=g).to(dev)
    stepper = unet_amd.TrainStepper(model, amp=False)
    assert stepper.distill is None
    terms = stepper.step(images, masks)
    assert "kd" not in terms
    out = (_bits(terms["loss"]).clone(), _bits(stepper.optimizer.flat_p).clone())
    stepper.close()
    return out, (images, masks)


def test_the_step_record_is_untouched_and_nothing_leaks_between_steppers(tmp_path):
    import unet_amd
    from unet_amd import ops
    dev = torch.device("cuda:0")
    default = ops.StepState()
    assert ops.STEP == default
    first, (images, masks) = _plain_step()
    torch.manual_seed(5)
    student = unet_amd.UNet_T(1, 3, bilinear=True).to(dev)
    spec = _teacher_file(tmp_path / "teacher.pth", 3, seed=7) + ",arch=UNet_T,T=2,w=1"
    stepper = unet_amd.TrainStepper(student, amp=True, distill=spec)                 # a spec: the stepper builds the Distiller
    assert isinstance(stepper.distill, unet_amd.Distiller) and stepper.distill.amp is True
    seen = []
    inner = stepper.distill.teacher_logits

    def watched(x):
        before = ops.STEP
        inside = []
        fwd = stepper.distill.teacher.forward
        stepper.distill.teacher.forward = lambda *a, **k: (inside.append(ops.STEP), fwd(*a, **k))[1]
        try:
            out = inner(x)
        finally:
            del stepper.distill.teacher.forward
        seen.append((before, inside[0], ops.STEP))
        return out

    stepper.distill.teacher_logits = watched
    teacher_before = {k: v.clone() for k, v in stepper.distill.teacher.state_dict().items()}
    for _ in range(2):
        terms = stepper.step(images, masks)
        assert torch.isfinite(terms["loss"]).item() and torch.isfinite(terms["kd"]).item()
    assert len(seen) == 2
    for before, inside, after in seen:
        assert after is before and before.weight_pack is not None                    # the step's record, as it was
        assert inside == default                                                     # the teacher runs under the defaults
    for k, v in stepper.distill.teacher.state_dict().items():
        assert torch.equal(v, teacher_before[k]), k
    assert not any(p is q for p in stepper.distill.teacher.parameters() for g in stepper.optimizer.param_groups for q in g["params"])
    stepper.close()
    assert ops.STEP == default
    second, _ = _plain_step()
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])


def test_the_epoch_loop_logs_the_term_and_saves_the_student_alone(tmp_path):
    """run_training (what `python -m unet_amd.train --distill ...` calls) in process, two epochs over five tiny phantoms."""
    import os
    from PIL import Image
    import unet_amd
    from unet_amd.train_cli import STATE_FILE, get_args, run_record, run_training
    from unet_amd.utils.data_loading import BasicDataset
    imgs, masks = unet_amd.ellipse_batch(5, 64, seed=3)
    grey = np.array([0, 128, 255], np.uint8)
    for i in range(5):
        split = "train" if i < 3 else "val"
        for d in ("imgs", "masks"):
            os.makedirs(tmp_path / d / split, exist_ok=True)
        Image.fromarray((imgs[i, 0].numpy() * 255).astype(np.uint8)).save(tmp_path / "imgs" / split / f"p{i}.png")
        Image.fromarray(grey[masks[i].numpy()]).save(tmp_path / "masks" / split / f"p{i}_mask.png")
    sets = [BasicDataset(str(tmp_path / "imgs" / s), str(tmp_path / "masks" / s), 1.0) for s in ("train", "val")]
    spec = _teacher_file(tmp_path / "teacher.pth", 3, seed=7) + ",arch=UNet_T,T=2,w=0.5"
    args = get_args(["--model", "UNet_T", "-c", "3", "-b", "2", "-s", "1.0", "--bilinear", "--distill", spec, "--save-state"])
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = unet_amd.UNet_T(1, 3, bilinear=True).to(memory_format=torch.channels_last).to(dev)
    keys = list(model.state_dict())
    lines = []
    history = run_training(model, dev, sets[0], sets[1], epochs=2, batch_size=2, learning_rate=1e-5, amp=True,
                           checkpoint_dir=str(tmp_path / "ckpt"), seed=1, workers=2, log=lines.append, distill=args.distill,
                           save_state=True, record=run_record(args))
    assert len(history) == 2
    for rec in history:
        assert np.isfinite(rec["loss"]) and np.isfinite(rec["kd"]) and rec["kd"] > 0 and 0.0 <= rec["kd_agree"] <= 1.0
    assert sum("distillation kd (mean)" in l for l in lines) == 2 and any(l.startswith("Distillation: teacher") for l in lines)
    state = torch.load(tmp_path / "ckpt" / STATE_FILE, map_location="cpu", weights_only=True)
    assert list(state["model"]) == keys                                              # the student alone
    assert state["args"]["distill"] == args.distill.spec() and len(state["args"]["distill_sha256"]) == 64
    # without the option the records carry no such keys
    torch.manual_seed(0)
    plain = unet_amd.UNet_T(1, 3, bilinear=True).to(memory_format=torch.channels_last).to(dev)
    off = run_training(plain, dev, sets[0], sets[1], epochs=1, batch_size=2, learning_rate=1e-5, amp=True, checkpoint_dir=None,
                       seed=1, workers=2)
    assert "kd" not in off[0] and "kd_agree" not in off[0]


# ------------------------------------------------------------------------------------------------ refusals
def test_the_graph_stepper_refuses_the_option(tmp_path):
    import unet_amd
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = unet_amd.UNet_T(1, 3, bilinear=True).to(dev)
    spec = _teacher_file(tmp_path / "teacher.pth", 3, seed=7) + ",arch=UNet_T"
    with pytest.raises(RuntimeError, match="distillation"):
        unet_amd.GraphedTrainStepper(model, amp=False, distill=spec)
    with pytest.raises(ValueError, match="head of 3 outputs, the student one of 1"):
        unet_amd.TrainStepper(unet_amd.UNet_T(1, 1, bilinear=True).to(dev), amp=False, distill=spec)


def test_each_entry_point_refuses_bad_arguments_with_an_error_code():
    """Called from the CPU side with stand-in pointers: the checks sit in front of the launches, nothing is followed."""
    import unet_amd  # noqa: F401
    from unet_amd._lib import LIB
    dll = LIB.load()
    P = 4096
    big = LIB.query("uh_loss_ws_bytes", 100)
    assert dll.uh_distill_nsums() == 2
    assert dll.uh_distill_sums(P, P, 100, 9, 2.0, P, P, big, None) == -1
    assert dll.uh_distill_sums(P, P, 100, 3, 0.0, P, P, big, None) == -1
    assert dll.uh_distill_sums(P, P, 0, 3, 2.0, P, P, big, None) == -1
    assert dll.uh_distill_sums(P, None, 100, 3, 2.0, P, P, big, None) == -1
    assert dll.uh_distill_sums(P, P, 100, 3, 2.0, P, P, big - 1, None) == -1
    assert dll.uh_distill_finish(P, 0.0, 2.0, 1.0, P, None) == -1
    assert dll.uh_distill_finish(P, 100.0, float("nan"), 1.0, P, None) == -1
    assert dll.uh_distill_finish(P, 100.0, 2.0, -1.0, P, None) == -1
    assert dll.uh_distill_finish(None, 100.0, 2.0, 1.0, P, None) == -1
    assert dll.uh_distill_grad(P, P, 100, 0, 100.0, 2.0, 1.0, None, P, None) == -1
    assert dll.uh_distill_grad(P, P, 100, 3, 100.0, 2.0, 1.0, None, None, None) == -1
    assert dll.uh_distill_grad(P, P, 100, 3, float("inf"), 2.0, 1.0, None, P, None) == -1
    assert dll.uh_distill_grad(P, P, 100, 3, 100.0, 2.0, 0.0, None, P, None) == -1
    assert b"weight" in dll.uh_last_error()
