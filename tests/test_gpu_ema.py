"""The averaged weights (EMA) of the optimizer pass on the MI355X (DESIGN.md section 3 "Averaged weights and resumable state"):
uh_rmsprop_step_ema against uh_rmsprop_step bit for bit and against a float64 restatement of the average, the update
counter, the exact swap behind TrainStepper.averaged(), the captured graph, and the optimizer's state_dict round trip.

The bound of the average.  e' = e + c (p - e) is three fp32 roundings (the difference, the product, the sum), each of a
value of magnitude at most 2 M with M = max(|p|, |e|) and c <= 1, so each costs at most 2^-24 * 2 M: 6 * 2^-24 * M in all
(contracting the product and the sum into one FMA only removes a rounding).  The restatement takes the kernel's own fp32
p_new and e_prev and forms d_t and c = 1 - d_t in float32 as the kernel does: rounding 0.999 to fp32 alone moves c by
2e-5 relative, far more than the bound.  Chained over k steps the error obeys err' <= d err + bound, so it never passes
k bounds; the chained test allows 20 for its 20 steps."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
HYPER = dict(lr=1e-3, alpha=0.99, eps=1e-8, wd=1e-2, mu=0.9)
GRID_CAP_N = 4 * 256 * 4096 + 7          # one element group more than 256 x 16 workgroups of 256 threads hold: the loop wraps


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _inputs(n, seed, norm):
    """p, g, sq >= 0, buf, ema (n floats, padded allocation) and the 1-element norm."""
    g = torch.Generator().manual_seed(seed)
    dev = _dev()
    t = {"p": torch.randn(n, generator=g), "g": torch.randn(n, generator=g) * 0.1, "sq": torch.rand(n, generator=g) * 0.01,
         "buf": torch.randn(n, generator=g) * 0.1, "ema": torch.randn(n, generator=g)}
    out = {k: v.to(dev) for k, v in t.items()}
    out["norm"] = torch.tensor([norm], dtype=torch.float32, device=dev)
    return out


def _plain(t, n, max_norm=1.0):
    from unet_amd._lib import LIB
    LIB.call("uh_rmsprop_step", t["p"].data_ptr(), t["g"].data_ptr(), t["sq"].data_ptr(), t["buf"].data_ptr(), n,
             t["norm"].data_ptr(), max_norm, HYPER["lr"], HYPER["alpha"], HYPER["eps"], HYPER["wd"], HYPER["mu"],
             torch.cuda.current_stream().cuda_stream)


def _with_ema(t, n, decay, warmup, updates, max_norm=1.0):
    from unet_amd._lib import LIB
    LIB.call("uh_rmsprop_step_ema", t["p"].data_ptr(), t["g"].data_ptr(), t["sq"].data_ptr(), t["buf"].data_ptr(),
             t["ema"].data_ptr(), n, t["norm"].data_ptr(), max_norm, HYPER["lr"], HYPER["alpha"], HYPER["eps"], HYPER["wd"],
             HYPER["mu"], decay, warmup, updates.data_ptr(), torch.cuda.current_stream().cuda_stream)


def _c32(decay, warmup, t):
    """c = 1 - d_t in float32, d_t = warmup > 0 ? min(decay, (1 + t) / (warmup + t)) : decay -- the kernel's statements."""
    d = np.float32(decay)
    if warmup > 0:
        tf = np.float32(t)
        d = np.minimum(d, (np.float32(1) + tf) / (np.float32(warmup) + tf))
    return np.float32(1) - np.float32(d)


def _ema_ref(e_prev, p_new, c):
    e, p = np.asarray(e_prev, np.float64), np.asarray(p_new, np.float64)
    return e + np.float64(c) * (p - e)


def _bound(p_new, e_prev):
    return 6 * U * np.maximum(np.abs(np.asarray(p_new, np.float64)), np.abs(np.asarray(e_prev, np.float64)))


# ------------------------------------------------------------------------------------------------ 1. parameter path unchanged
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 4099, GRID_CAP_N])
def test_parameter_path_is_bit_identical_to_the_plain_step(n):
    for norm in (0.25, 7.5):                                         # below max_norm = 1 (no clipping) and above it
        a, b = _inputs(n, n % 1000 + 1, norm), _inputs(n, n % 1000 + 1, norm)
        before = a["g"].clone()
        updates = torch.tensor([3], dtype=torch.int32, device=_dev())
        _plain(a, n)
        _with_ema(b, n, 0.999, 10, updates)
        torch.cuda.synchronize()
        for k in ("p", "g", "sq", "buf"):
            assert torch.equal(a[k], b[k]), (k, n, norm)
        assert not torch.equal(a["ema"], b["ema"]) and int(updates.item()) == 3       # the average moved; the pass does not tick
        assert torch.equal(a["g"], before) == (norm < 1.0)          # the clip rescaled the gradient only above max_norm


# ------------------------------------------------------------------------------------------------ 2. EMA arithmetic, one step
@pytest.mark.parametrize("warmup,t", [(0, 0), (0, 5), (10, 0), (10, 1), (10, 9), (10, 8991)])
def test_ema_of_one_step_against_float64(warmup, t):
    n = 4099
    x = _inputs(n, 77 + t % 50 + warmup, 0.5)
    e_prev = x["ema"].cpu().numpy()
    updates = torch.tensor([t], dtype=torch.int32, device=_dev())
    _with_ema(x, n, 0.999, warmup, updates)
    torch.cuda.synchronize()
    p_new, got = x["p"].cpu().numpy(), x["ema"].cpu().numpy().astype(np.float64)
    c = _c32(0.999, warmup, t)
    err = np.abs(got - _ema_ref(e_prev, p_new, c))
    bound = _bound(p_new, e_prev)
    print(f"warmup {warmup} t {t}: c = {float(c):.9g}, worst error / bound = {float((err / bound).max()):.3f}")
    assert (err <= bound).all()
    if warmup == 10 and t == 8991:
        assert c == np.float32(1) - np.float32(0.999)               # the update at which the warm-up reaches the decay ...
        assert _c32(0.999, 10, 8989) > c                            # ... and not before (8991 / 9000 at t = 8990 rounds onto it)
    if warmup == 10 and t == 0:
        assert c == np.float32(1) - np.float32(0.1)


# ------------------------------------------------------------------------------------------------ toy optimizer
def _toy(ema_decay=0.99, lr=1e-2, **kw):
    """Two parameters of 7 x 5 and 13 elements under a FusedRMSprop; backward(ga, gb) delivers those as their gradients."""
    import unet_amd
    g = torch.Generator().manual_seed(5)
    a = torch.nn.Parameter(torch.randn(7, 5, generator=g).to(_dev()))
    b = torch.nn.Parameter(torch.randn(13, generator=g).to(_dev()))
    opt = unet_amd.FusedRMSprop([a, b], lr=lr, ema_decay=ema_decay, **kw)
    return a, b, opt


def _backward(opt, pairs):
    opt.zero_grad()
    sum((p * g).sum() for p, g in pairs).backward()


def _state(opt):
    torch.cuda.synchronize()
    return {"p": opt.flat_p.clone(), "sq": opt.flat_sq.clone(), "buf": opt.flat_buf.clone(), "ema": opt.flat_ema.clone(),
            "updates": int(opt.ema_updates.item())}


# ------------------------------------------------------------------------------------------------ 3. chained
def test_twenty_chained_steps_against_float64():
    a, b, opt = _toy(ema_decay=0.99)
    assert opt.ema.warmup == 10 and int(opt.ema_updates.item()) == 0 and torch.equal(opt.flat_ema, opt.flat_p)
    g = torch.Generator().manual_seed(9)
    ref = opt.flat_ema.cpu().numpy().astype(np.float64)
    for k in range(1, 21):
        e_prev = opt.flat_ema.cpu().numpy()
        _backward(opt, [(a, torch.randn(a.shape, generator=g).to(_dev())), (b, torch.randn(b.shape, generator=g).to(_dev()))])
        opt.step()
        s = _state(opt)
        assert s["updates"] == k
        p_new = s["p"].cpu().numpy()
        ref = _ema_ref(ref, p_new, _c32(0.99, 10, k - 1))
        err = np.abs(s["ema"].cpu().numpy().astype(np.float64) - ref)
        assert (err <= 20 * _bound(p_new, e_prev)).all(), (k, float(err.max()))
    assert not torch.equal(opt.flat_ema, opt.flat_p)


# ------------------------------------------------------------------------------------------------ 4. fixed point and skip
def test_zero_lr_is_a_fixed_point_and_a_nan_gradient_skips_everything():
    a, b, opt = _toy(lr=0.0)
    g = torch.Generator().manual_seed(2)
    for k in range(5):
        _backward(opt, [(a, torch.randn(a.shape, generator=g).to(_dev())), (b, torch.randn(b.shape, generator=g).to(_dev()))])
        opt.step()
        s = _state(opt)
        assert torch.equal(s["ema"], s["p"]) and s["updates"] == k + 1
    a, b, opt = _toy(lr=1e-2)
    _backward(opt, [(a, torch.ones_like(a)), (b, torch.ones_like(b))])
    opt.step()                                                       # a first step: every buffer holds something
    before = _state(opt)
    bad = torch.ones_like(b)
    bad[3] = float("nan")
    _backward(opt, [(a, torch.ones_like(a)), (b, bad)])
    opt.step()
    after = _state(opt)
    assert not torch.isfinite(opt.norm).item()
    for k in ("p", "sq", "buf", "ema"):
        assert torch.equal(before[k].view(torch.int32), after[k].view(torch.int32)), k
    assert after["updates"] == before["updates"] == 1


# ------------------------------------------------------------------------------------------------ 5. stale slice
def test_a_parameter_without_a_gradient_keeps_its_average():
    a, b, opt = _toy(lr=1e-2, ema_decay=0.5, ema_warmup=0)
    _backward(opt, [(a, torch.ones_like(a)), (b, torch.ones_like(b))])
    opt.step()
    before = _state(opt)
    _backward(opt, [(a, torch.ones_like(a))])                        # b gets no gradient in this step
    opt.step()
    after = _state(opt)
    ia, ib = opt._index[id(a)], opt._index[id(b)]
    (oa, na), (ob, nb) = opt.slices[ia], opt.slices[ib]
    for k in ("p", "sq", "buf", "ema"):
        assert torch.equal(before[k][ob:ob + nb], after[k][ob:ob + nb]), k
    assert not torch.equal(before["ema"][oa:oa + na], after["ema"][oa:oa + na])
    assert not torch.equal(before["p"][oa:oa + na], after["p"][oa:oa + na])
    assert after["updates"] == before["updates"] + 1 == 2


# ------------------------------------------------------------------------------------------------ steppers
def _batches(n, size=64, first_seed=20):
    import unet_amd
    return [tuple(t.to(_dev()) for t in unet_amd.ellipse_batch(2, size, seed=first_seed + i)) for i in range(n)]


def _model(classes, seed=0):
    import unet_amd
    torch.manual_seed(seed)
    return unet_amd.UNet_T(1, classes).to(memory_format=torch.channels_last).to(_dev())


def _eval_logits(model, images, amp):
    model.eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
        return model(images).float().clone()


def _opt_state(st):
    torch.cuda.synchronize()
    o = st.optimizer
    out = {"p": o.flat_p.clone(), "sq": o.flat_sq.clone(), "buf": o.flat_buf.clone()}
    if o.ema is not None:
        out.update(ema=o.flat_ema.clone(), updates=int(o.ema_updates.item()))
    return out


def _same(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k], k


# ------------------------------------------------------------------------------------------------ 6. swap is exact and noticed
def test_swap_is_exact_and_noticed():
    import unet_amd
    data = _batches(6)
    probe = data[0][0]
    res = []
    for swapping in (False, True):
        model = _model(3)
        st = unet_amd.TrainStepper(model, lr=1e-3, ema="0.9,warmup=0")
        for k, (im, mk) in enumerate(data, 1):
            st.step(im, mk)
            if swapping and k in (2, 4):
                live = _eval_logits(model, probe, True)
                with st.averaged():
                    avg = _eval_logits(model, probe, True)
                    with pytest.raises(RuntimeError, match="averaged"):
                        st.step(im, mk)
                    with pytest.raises(RuntimeError, match="nest"):
                        with st.averaged():
                            pass
                assert not torch.equal(avg, live)
                assert torch.equal(_eval_logits(model, probe, True), live)                  # and back again
                fresh = unet_amd.UNet_T(1, 3)
                fresh.load_state_dict(st.ema_state_dict())
                fresh = fresh.to(memory_format=torch.channels_last).to(_dev())
                assert torch.equal(_eval_logits(fresh, probe, True), avg), "a stale packed filter or folded BatchNorm was used"
        res.append((_opt_state(st), {k: v.clone() for k, v in model.state_dict().items()}))
        st.close()
    _same(res[0][0], res[1][0])
    _same(res[0][1], res[1][1])
    assert res[0][0]["updates"] == 6


def test_averaged_restores_the_live_weights_after_an_exception():
    import unet_amd
    model = _model(3)
    st = unet_amd.TrainStepper(model, lr=1e-3, ema="0.9,warmup=0")
    st.step(*_batches(1)[0])
    before = _opt_state(st)
    with pytest.raises(KeyError):
        with st.averaged():
            assert torch.equal(st.optimizer.flat_p, before["ema"]) and torch.equal(st.optimizer.flat_ema, before["p"])
            raise KeyError("inside")
    _same(_opt_state(st), before)
    with st.averaged():                                              # usable again
        pass
    with pytest.raises(RuntimeError, match="ema"):
        unet_amd.TrainStepper(_model(3, seed=1)).averaged().__enter__()
    st.close()


# ------------------------------------------------------------------------------------------------ 7. no EMA equals today
def test_the_option_changes_only_the_extra_buffer():
    import unet_amd
    data = _batches(4)
    res = []
    for ema in (None, "0.99"):
        model = _model(3)
        st = unet_amd.TrainStepper(model, lr=1e-3, ema=ema)
        assert (st.optimizer.flat_ema is None) == (ema is None) and (st.optimizer.ema_updates is None) == (ema is None)
        for im, mk in data:
            st.step(im, mk)
        res.append(_opt_state(st))
        st.close()
    for k in ("p", "sq", "buf"):
        assert torch.equal(res[0][k], res[1][k]), k
    assert "ema" not in res[0] and res[1]["updates"] == 4


# ------------------------------------------------------------------------------------------------ 8. graph
def test_graph_replays_average_with_their_own_decay():
    import unet_amd
    data = _batches(3)
    model = _model(1)
    eager = unet_amd.TrainStepper(model, lr=1e-3, amp=False, ema="0.99")
    for im, mk in data:
        eager.step(im, mk)
    want = _opt_state(eager)
    eager.close()
    model = _model(1)
    st = unet_amd.GraphedTrainStepper(model, lr=1e-3, amp=False, ema="0.99")
    start = _opt_state(st)
    st._capture(*data[0])
    after_capture = _opt_state(st)
    _same(after_capture, start)                                      # the capture's warm-up steps do not count
    assert after_capture["updates"] == 0
    trail = [after_capture]
    for im, mk in data:
        st.step(im, mk)
        trail.append(_opt_state(st))
    _same(trail[-1], want)
    assert [s["updates"] for s in trail] == [0, 1, 2, 3]
    # each replay used the decay of its own update number: d_0 = 1/10, d_1 = 2/11, d_2 = 3/12, not the d_0 of the capture
    for t in (1, 2):
        e_prev, p_new = trail[t]["ema"].cpu().numpy(), trail[t + 1]["p"].cpu().numpy()
        got = trail[t + 1]["ema"].cpu().numpy().astype(np.float64)
        assert (np.abs(got - _ema_ref(e_prev, p_new, _c32(0.99, 10, t))) <= _bound(p_new, e_prev)).all()
        frozen = np.abs(got - _ema_ref(e_prev, p_new, _c32(0.99, 10, 0)))
        assert (frozen > _bound(p_new, e_prev)).any(), "the warm-up decay is frozen in the graph"
    st.close()


# ------------------------------------------------------------------------------------------------ 9. state round trip
def test_state_dict_round_trip_resumes_bit_for_bit():
    import unet_amd
    data = _batches(6)

    def run(st, chunk, first):
        for k, (im, mk) in enumerate(chunk, first):
            if k == 3:
                st.optimizer.param_groups[0]["lr"] = 5e-4            # a changed lr travels with the state
            st.step(im, mk)

    model = _model(3)
    whole = unet_amd.TrainStepper(model, lr=1e-3, ema="0.9,warmup=10")
    run(whole, data, 1)
    want = (_opt_state(whole), {k: v.clone() for k, v in model.state_dict().items()})
    whole.close()

    model = _model(3)
    first = unet_amd.TrainStepper(model, lr=1e-3, ema="0.9,warmup=10")
    run(first, data[:3], 1)
    torch.cuda.synchronize()
    sd_model = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    sd_opt = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in first.optimizer.state_dict().items()}
    first.step(*data[3])                                             # the state is a copy: later steps do not reach it
    first.close()
    assert sd_opt["ema_updates"] == 3 and sd_opt["hyper"]["lr"] == 5e-4 and sd_opt["hyper"]["ema_decay"] == 0.9

    model = unet_amd.UNet_T(1, 3)                                    # other initial weights
    model.load_state_dict(sd_model)
    model = model.to(memory_format=torch.channels_last).to(_dev())
    second = unet_amd.TrainStepper(model, lr=1e-3, ema="0.9,warmup=10")
    second.optimizer.load_state_dict(sd_opt)
    assert second.optimizer.param_groups[0]["lr"] == 5e-4
    run(second, data[3:], 4)
    _same(_opt_state(second), want[0])
    _same({k: v.clone() for k, v in model.state_dict().items()}, want[1])
    second.close()

    other = unet_amd.TrainStepper(_model(1), lr=1e-3, ema="0.9,warmup=10")
    with pytest.raises(ValueError, match="layout"):
        other.optimizer.load_state_dict(sd_opt)
    other.close()
    slower = unet_amd.TrainStepper(_model(3), lr=1e-3, ema="0.99,warmup=10")      # the same layout, another decay
    with pytest.raises(ValueError, match="0.99"):
        slower.optimizer.load_state_dict(sd_opt)
    assert slower.optimizer.ema == slower.ema == unet_amd.EmaConfig(0.99, 10)
    slower.close()
    plain = unet_amd.TrainStepper(_model(3), lr=1e-3)
    with pytest.raises(ValueError, match="moving average"):
        plain.optimizer.load_state_dict(sd_opt)
    plain.close()
