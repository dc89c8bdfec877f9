"""CPU checks of the surface loss (DESIGN.md section 3 "Surface loss"): the restatement tests/surface_loss_ref.py against a brute
force distance and against finite differences, the --surface-loss command-line option, and the C ABI's new entry points."""
import ctypes

import numpy as np
import pytest
import torch

import contour_metrics_ref as C
import surface_loss_ref as R


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("H,W", [(7, 9), (16, 5)])
def test_phi_agrees_with_the_brute_force_distance(H, W):
    rng = np.random.default_rng(H * 31 + W)
    for _ in range(4):
        T = C.blob_mask(rng, H, W)
        d2 = C.edt_sq_brute(C.border(T))
        want = np.sqrt(d2.astype(np.float64)).astype(np.float32)
        got = R.phi_image(T)
        assert got.dtype == np.float32 and np.array_equal(np.abs(got), want)
        assert (got[T] <= 0).all() and (got[~T] > 0).all()
        assert np.signbit(got[C.border(T)]).all() and (got[C.border(T)] == 0).all()      # border pixels are -0.0


def test_empty_class_is_all_zero_and_a_full_class_is_non_positive():
    labels = np.zeros((2, 6, 8), np.int64)
    labels[1] = 2
    phi = R.phi_maps(labels, (2,))
    assert phi.shape == (1, 2, 6, 8) and phi.dtype == np.float32
    assert (phi[0, 0] == 0).all() and not np.signbit(phi[0, 0]).any()                    # class absent: +0.0 everywhere
    full = phi[0, 1]
    assert (full <= 0).all()
    frame = np.ones((6, 8), bool)
    frame[1:-1, 1:-1] = False
    assert np.array_equal(full == 0, frame)                                              # its zeros lie on the image frame
    # the binary head's target is label // 2
    assert np.array_equal(R.phi_maps(labels, (1,), binary=True), phi)


@pytest.mark.parametrize("n_classes,classes", [(1, None), (3, None), (3, (1, 2)), (3, (0,))])
def test_closed_form_gradients_pass_gradcheck(n_classes, classes):
    rng = np.random.default_rng(5)
    B, H, W = 2, 5, 4
    labels = R.blob_labels(rng, B, H, W)
    g = torch.Generator().manual_seed(3)
    z = (torch.randn(B, n_classes, H, W, generator=g, dtype=torch.float64) * 3).requires_grad_()
    assert torch.autograd.gradcheck(lambda t: R.ClosedFormSurface.apply(t, labels, n_classes, classes), (z,), eps=1e-6, atol=1e-8)
    (auto,) = torch.autograd.grad(R.surface_loss(z, labels, n_classes, classes), z)
    closed = R.closed_form_grad(z, labels, n_classes, classes)
    assert torch.allclose(auto, closed, rtol=1e-12, atol=1e-15)
    # n_mean, the upstream gradient and the weight scale it linearly
    scaled = R.closed_form_grad(z, labels, n_classes, classes, n_mean=4 * B * H * W, g=0.5, w=3.0)
    assert torch.allclose(scaled, closed * (0.5 * 3.0 / 4), rtol=1e-12, atol=1e-18)


# ------------------------------------------------------------------------------------------------ the command line
def test_surface_weight_at_ramps_and_saturates():
    from unet_amd.train_cli import SurfaceSpec, surface_weight_at
    spec = SurfaceSpec(0.01, 0.01)
    assert surface_weight_at(spec, 1) == 0.01
    assert surface_weight_at(spec, 3) == pytest.approx(0.03, rel=1e-12)
    assert surface_weight_at(spec, 1000) == 1.0
    assert surface_weight_at(SurfaceSpec(0.05), 7) == 0.05
    assert surface_weight_at(SurfaceSpec(0.0, 0.5), 2) == 0.5


def test_surface_loss_flag_parses():
    from unet_amd.train_cli import SurfaceSpec, get_args
    assert get_args([]).surface_loss is None
    assert get_args(["--surface-loss"]).surface_loss == SurfaceSpec(0.01, 0.01, None)
    assert get_args(["--surface-loss", "0.05"]).surface_loss == SurfaceSpec(0.05, 0.0, None)
    assert get_args(["--surface-loss", "0.02,ramp=0.1,classes=1+2"]).surface_loss == SurfaceSpec(0.02, 0.1, (1, 2))
    assert get_args(["--surface-loss", "0.5,classes=2", "-e", "3"]).surface_loss == SurfaceSpec(0.5, 0.0, (2,))
    # the flag before another option stays bare
    a = get_args(["--surface-loss", "--metrics"])
    assert a.surface_loss == SurfaceSpec(0.01, 0.01, None) and a.metrics


@pytest.mark.parametrize("spec", ["x", "", "-0.1", "nan", "0.1,ramp", "0.1,ramp=", "0.1,ramp=-1", "0.1,slope=2", "0.1,classes=a",
                                  "0.1,classes=1+1", "0.1,classes=-1", "0.1,ramp=0.1,ramp=0.2", "ramp=0.1"])
def test_malformed_surface_specs_are_argparse_errors(spec, capsys):
    from unet_amd.train_cli import get_args
    with pytest.raises(SystemExit) as e:
        get_args(["--surface-loss=" + spec])
    assert e.value.code == 2
    # the parser's own message, not argparse's "unrecognized arguments" for an option it does not know
    assert f"bad --surface-loss {spec!r}: " in capsys.readouterr().err


def test_classes_are_checked_against_the_head():
    from unet_amd.utils.surface_loss import default_classes, head_classes
    assert default_classes(1) == (1,) and default_classes(3) == (2,) and default_classes(4) == (2,)
    assert head_classes(3, (1, 2)) == (1, 2) and head_classes(1, None) == (1,) and head_classes(1, (1,)) == (1,)
    for n, cls in ((3, (3,)), (3, ()), (3, (1, 1)), (1, (2,)), (2, None), (4, (-1,))):
        with pytest.raises(ValueError):
            head_classes(n, cls)


# ------------------------------------------------------------------------------------------------ the C ABI
NEW_SYMBOLS = ("uh_surface_loss_ws_bytes", "uh_surface_border_i64", "uh_surface_dist_map", "uh_surface_loss_sums",
               "uh_surface_loss_grad")


def test_new_header_symbols_are_exported():
    import unet_amd  # noqa: F401
    from unet_amd._lib import LIB, LIB_PATH, parse_header
    protos = parse_header()
    dll = ctypes.CDLL(LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in protos, f"{name} is not declared in include/unet_hip.h"
        assert hasattr(dll, name), f"{name} is not exported"
    LIB.load()
    # D (4 bytes) + border (1 byte) per map pixel at least; nothing for a shape the entry points refuse
    assert LIB.query("uh_surface_loss_ws_bytes", 8, 512, 512, 3) >= 5 * 3 * 8 * 512 * 512
    assert LIB.query("uh_surface_loss_ws_bytes", 8, 512, 512, 0) == 0 and LIB.query("uh_surface_loss_ws_bytes", 0, 4, 4, 1) == 0
    assert LIB.query("uh_surface_loss_ws_bytes", 1, 1, 8192, 1) > LIB.query("uh_surface_loss_ws_bytes", 1, 2, 4096, 1)   # the EDT's wide rows


def test_bad_arguments_raise_instead_of_crashing():
    """Every check sits in front of the first launch: no GPU is touched (the pointers are never followed)."""
    import unet_amd  # noqa: F401
    from unet_amd._lib import LIB
    LIB.load()
    one, two = (ctypes.c_int * 1)(2), (ctypes.c_int * 2)(1, 1)
    P, WS = 4096, 1 << 20                                          # a non-null, 16-byte aligned stand-in pointer
    with pytest.raises(RuntimeError, match="null pointer"):
        LIB.call("uh_surface_border_i64", None, 1, one, 1, P, 1, 4, 4, None)
    with pytest.raises(RuntimeError, match="null pointer"):
        LIB.call("uh_surface_dist_map", P, 1, None, 1, P, 1, 4, 4, P, WS, None)
    with pytest.raises(RuntimeError, match="null pointer"):
        LIB.call("uh_surface_loss_sums", None, P, 1, one, 1, 3, 1, 4, 4, 16.0, 1.0, P, P, WS, None)
    with pytest.raises(RuntimeError, match="null pointer"):
        LIB.call("uh_surface_loss_grad", P, P, 1, one, 1, 3, 1, 4, 4, 16.0, 1.0, None, None, 0, P, WS, None)
    with pytest.raises(RuntimeError, match="selected classes"):     # K < 1
        LIB.call("uh_surface_dist_map", P, 1, one, 0, P, 1, 4, 4, P, WS, None)
    with pytest.raises(RuntimeError, match="selected classes"):
        LIB.call("uh_surface_loss_sums", P, P, 1, one, 9, 3, 1, 4, 4, 16.0, 1.0, P, P, WS, None)
    with pytest.raises(RuntimeError, match=r"class id 2 is outside \[0, 2\)"):
        LIB.call("uh_surface_loss_sums", P, P, 1, one, 1, 2, 1, 4, 4, 16.0, 1.0, P, P, WS, None)
    with pytest.raises(RuntimeError, match="outside"):
        LIB.call("uh_surface_border_i64", P, 1, (ctypes.c_int * 1)(-1), 1, P, 1, 4, 4, None)
    # the sigmoid head: one map, its id a value of mask // mask_div (1, the foreground), not a channel below ncls
    with pytest.raises(RuntimeError, match="workspace 16 <"):
        LIB.call("uh_surface_loss_sums", P, P, 2, (ctypes.c_int * 1)(1), 1, 1, 1, 4, 4, 16.0, 1.0, P, P, 16, None)
    with pytest.raises(RuntimeError, match="workspace 16 <"):
        LIB.call("uh_surface_loss_grad", P, P, 2, (ctypes.c_int * 1)(1), 1, 1, 1, 4, 4, 16.0, 1.0, None, P, 0, P, 16, None)
    with pytest.raises(RuntimeError, match="sigmoid head has one map"):
        LIB.call("uh_surface_loss_sums", P, P, 2, (ctypes.c_int * 2)(0, 1), 2, 1, 1, 4, 4, 16.0, 1.0, P, P, WS, None)
    with pytest.raises(RuntimeError, match="selected twice"):
        LIB.call("uh_surface_loss_grad", P, P, 1, two, 2, 3, 1, 4, 4, 16.0, 1.0, None, P, 0, P, WS, None)
    with pytest.raises(RuntimeError, match="1 .sigmoid. to 8"):     # ncls > 8
        LIB.call("uh_surface_loss_sums", P, P, 1, one, 1, 9, 1, 4, 4, 16.0, 1.0, P, P, WS, None)
    with pytest.raises(RuntimeError, match="1 .sigmoid. to 8"):
        LIB.call("uh_surface_loss_grad", P, P, 1, one, 1, 0, 1, 4, 4, 16.0, 1.0, None, P, 0, P, WS, None)
    with pytest.raises(RuntimeError, match="limited to 32768"):     # the EDT's own size limits
        LIB.call("uh_surface_dist_map", P, 1, one, 1, P, 1, 4, 32769, P, WS, None)
    with pytest.raises(RuntimeError, match="65535"):
        LIB.call("uh_surface_dist_map", P, 1, two, 2, P, 40000, 4, 4, P, WS, None)
    with pytest.raises(RuntimeError, match="mask_div"):
        LIB.call("uh_surface_dist_map", P, 0, one, 1, P, 1, 4, 4, P, WS, None)
    with pytest.raises(RuntimeError, match="n_mean"):
        LIB.call("uh_surface_loss_sums", P, P, 1, one, 1, 3, 1, 4, 4, 0.0, 1.0, P, P, WS, None)
    with pytest.raises(RuntimeError, match="workspace 16 <"):
        LIB.call("uh_surface_loss_grad", P, P, 1, one, 1, 3, 1, 4, 4, 16.0, 1.0, None, P, 0, P, 16, None)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        LIB.call("uh_surface_dist_map", P, 1, one, 1, P, 1, 4, 4, P + 4, WS, None)


def test_python_surface_has_no_cpu_fallback_and_the_graph_stepper_signature():
    import inspect
    import unet_amd
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        unet_amd.surface_distance_map(torch.zeros(1, 4, 4, dtype=torch.int64), (2,))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        unet_amd.surface_loss(torch.zeros(1, 3, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64), 3)
    for fn in (unet_amd.seg_loss, unet_amd.train_step, unet_amd.TrainStepper.__init__):
        params = inspect.signature(fn).parameters
        assert params["surface_weight"].default == 0.0 and params["surface_classes"].default is None


def test_the_shared_head_check_refuses_a_one_channel_head_with_a_channel_axis():
    """One head check for the surface, focal and distillation nodes: [B,H,W] is the one-channel head, [B,H,W,C] a softmax head of
    C >= 2, and [B,H,W,1] is refused for all three (the surface node used to read it as the one-channel head)."""
    from unet_amd import losses
    assert losses._head_of(torch.zeros(2, 4, 5), (2, 4, 5), "surface loss") == 1
    assert losses._head_of(torch.zeros(2, 4, 5, 3), (2, 4, 5), "surface loss") == 3
    for who in ("surface loss", "focal / Tversky loss", "distillation"):
        with pytest.raises(RuntimeError, match=f"{who}: the one-channel head passes its logits as \\[B,H,W\\]"):
            losses._head_of(torch.zeros(2, 4, 5, 1), (2, 4, 5), who)
    with pytest.raises(RuntimeError, match="surface loss expects logits \\[B,H,W\\] or \\[B,H,W,C\\] matching labels"):
        losses._head_of(torch.zeros(2, 4, 6), (2, 4, 5), "surface loss")
