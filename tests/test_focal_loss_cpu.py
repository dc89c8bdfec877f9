"""CPU checks of the focal + Tversky loss (DESIGN.md section 3 "Focal / Tversky loss"): the float64 restatement the GPU tests
compare against (tests/focal_tversky_ref.py) agrees with the terms it generalises and with its own closed-form gradient,
LossConfig parses and refuses what it should, the C ABI refuses bad arguments without touching a GPU, and --loss takes part in
the --resume record."""
import logging

import pytest
import torch
import torch.nn.functional as F

import focal_tversky_ref as R


def _inputs(C, scale, n=257, seed=0):
    g = torch.Generator().manual_seed(seed + 13 * C)
    z = torch.randn(n, C, generator=g, dtype=torch.float64) * scale
    t = torch.randint(0, C - 1, (n,), generator=g) if C > 2 else torch.randint(0, 2, (n,), generator=g)
    w = [0.5 + 0.75 * c for c in range(C)]
    return z, t, w


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("C", [2, 3, 8])
@pytest.mark.parametrize("scale", [1.0, 10.0])
def test_gamma_zero_is_the_weighted_cross_entropy(C, scale):
    z, t, w = _inputs(C, scale)
    want = F.cross_entropy(z, t, weight=torch.tensor(w, dtype=torch.float64))
    assert torch.allclose(R.focal_term(z, t, w, 0.0), want, rtol=1e-13, atol=0)
    assert torch.allclose(R.focal_term(z, t, [1.0] * C, 0.0), F.cross_entropy(z, t), rtol=1e-13, atol=0)


@pytest.mark.parametrize("C", [2, 3, 8])
def test_equal_prices_are_the_per_class_dice(C):
    z, t, _ = _inputs(C, 3.0)
    p = torch.softmax(z, dim=1)
    tau = F.one_hot(t, C).double()
    TP, P, T = (p * tau).sum(0), p.sum(0), tau.sum(0)
    dice = (2 * TP + 2 * R.EPS) / (P + T + 2 * R.EPS)
    want = (1 - dice[1:]).mean()
    assert torch.allclose(R.tversky_term(z, t, 0.5, 0.5), want, rtol=1e-13, atol=0)


@pytest.mark.parametrize("C", [2, 3, 8])
@pytest.mark.parametrize("gamma", [0.0, 0.5, 2.0])
@pytest.mark.parametrize("scale", [1.0, 10.0, 100.0])
def test_closed_form_gradient_is_autograd(C, gamma, scale):
    z, t, w = _inputs(C, scale)
    for alpha, beta in ((0.5, 0.5), (0.3, 0.7)):
        auto = R.autograd_gradient(z, t, w, gamma, alpha, beta)
        closed = R.closed_form_gradient(z, t, w, gamma, alpha, beta)
        assert torch.isfinite(auto).all() and torch.isfinite(closed).all()
        assert float((auto - closed).norm() / auto.norm()) <= 1e-12


@pytest.mark.parametrize("gamma", [0.0, 0.5, 2.0])
def test_one_channel_form_is_the_two_class_form(gamma):
    """sigmoid statement of the one-channel head against the two-class softmax on the logits (0, z)."""
    g = torch.Generator().manual_seed(5)
    z = torch.randn(300, generator=g, dtype=torch.float64) * 4
    t = torch.randint(0, 2, (300,), generator=g)
    w = [0.7, 2.5]
    total, focal, tversky = R.loss_terms(R.two_class_logits(z), t, w, gamma, 0.3, 0.7, classes=(1,))
    p1 = torch.sigmoid(z)
    pt = torch.where(t == 1, p1, torch.sigmoid(-z))
    wt = torch.tensor(w, dtype=torch.float64)[t]
    nlp = F.softplus(torch.where(t == 1, -z, z))                       # -log sigmoid(+-z)
    focal_s = (wt * torch.sigmoid(torch.where(t == 1, -z, z)) ** gamma * nlp).sum() / wt.sum()
    tf = t.double()
    TP, P, T = (p1 * tf).sum(), p1.sum(), tf.sum()
    tv_s = 1 - (TP + R.EPS) / (0.0 * TP + 0.3 * P + 0.7 * T + R.EPS)
    assert torch.allclose(focal, focal_s, rtol=1e-12, atol=0) and torch.allclose(tversky, tv_s, rtol=1e-12, atol=0)
    assert torch.allclose(total, focal_s + tv_s, rtol=1e-12, atol=0)
    assert pt.min() > 0
    # and the one-channel gradient is dL/dz_1 of the two-class form
    zz = z.clone().requires_grad_(True)
    R.loss_terms(R.two_class_logits(zz), t, w, gamma, 0.3, 0.7, classes=(1,))[0].backward()
    closed = R.closed_form_gradient(R.two_class_logits(z), t, w, gamma, 0.3, 0.7, classes=(1,))[:, 1]
    assert float((zz.grad - closed).norm() / closed.norm()) <= 1e-12


# ------------------------------------------------------------------------------------------------ LossConfig
@pytest.mark.parametrize("spec,want", [
    ("focal=2,tversky=0.3/0.7", (2.0, None, 0.3, 0.7, None)),
    ("focal=0", (0.0, None, 0.3, 0.7, None)),
    ("focal=0.5, weights=1+2+3.5, tversky=0.5/0.5, classes=1+2", (0.5, (1.0, 2.0, 3.5), 0.5, 0.5, (1, 2))),
    ("classes=1,focal=1,weights=0.25+4", (1.0, (0.25, 4.0), 0.3, 0.7, (1,))),
])
def test_loss_config_parse_and_spec_round_trip(spec, want):
    import unet_amd
    cfg = unet_amd.LossConfig.parse(spec)
    assert (cfg.gamma, cfg.weights, cfg.alpha, cfg.beta, cfg.classes) == want
    assert unet_amd.LossConfig.parse(cfg.spec()) == cfg
    assert unet_amd.LossConfig.of(spec) == cfg and unet_amd.LossConfig.of(cfg) is cfg and unet_amd.LossConfig.of(None) is None


def test_loss_config_defaults_are_the_bare_flag():
    import unet_amd
    from unet_amd.train_cli import get_args
    from unet_amd.utils.focal_loss import LOSS_BARE
    assert LOSS_BARE == "focal=2,tversky=0.3/0.7"
    assert unet_amd.LossConfig() == unet_amd.LossConfig.parse(LOSS_BARE) == unet_amd.LossConfig(2.0, None, 0.3, 0.7, None)
    assert get_args(["--loss"]).loss == unet_amd.LossConfig() and get_args([]).loss is None
    assert get_args(["--loss", "focal=0.5,classes=2"]).loss == unet_amd.LossConfig(gamma=0.5, classes=(2,))


@pytest.mark.parametrize("bad,names", [
    ("", "focal"), ("tversky=0.3/0.7", "focal"), ("focal", "focal"), ("focal=", "focal"), ("focal=abc", "focal"),
    ("focal=-1", "gamma"), ("focal=inf", "gamma"), ("focal=nan", "gamma"), ("focal=1,focal=2", "twice"),
    ("focal=2,gamma=3", "gamma=3"), ("focal=2,weights=1", "weights"), ("focal=2,weights=1+0", "weights"),
    ("focal=2,weights=1+-2", "weights"), ("focal=2,weights=1+x", "weight"), ("focal=2,weights=1+2+3+4+5+6+7+8+9", "weights"),
    ("focal=2,tversky=0.3", "A/B"), ("focal=2,tversky=0/0", "alpha"), ("focal=2,tversky=-0.1/0.7", "alpha"),
    ("focal=2,tversky=a/b", "alpha"), ("focal=2,classes=1+1", "classes"), ("focal=2,classes=-1", "classes"),
    ("focal=2,classes=1.5", "classes"), ("focal=2,classes=8", "classes"), ("focal=2,,tversky=0.3/0.7", "''"),
])
def test_loss_config_refuses_a_malformed_spec_and_names_the_fault(bad, names):
    import unet_amd
    with pytest.raises(ValueError, match=names):
        unet_amd.LossConfig.parse(bad)


def test_loss_config_is_checked_against_the_head():
    import unet_amd
    cfg = unet_amd.LossConfig.parse("focal=2,weights=1+2+3")
    assert cfg.for_head(3) == ((1.0, 2.0, 3.0), (1, 2))
    assert unet_amd.LossConfig().for_head(1) == ((1.0, 1.0), (1,))
    assert unet_amd.LossConfig().for_head(8)[1] == (1, 2, 3, 4, 5, 6, 7)
    with pytest.raises(ValueError, match="3 class weights"):
        cfg.for_head(1)
    with pytest.raises(ValueError, match="3 class weights"):
        cfg.for_head(4)
    with pytest.raises(ValueError, match="classes"):
        unet_amd.LossConfig(classes=(3,)).for_head(3)
    with pytest.raises(ValueError, match="classes"):
        unet_amd.LossConfig(classes=(2,)).for_head(1)
    with pytest.raises(ValueError, match="heads"):
        unet_amd.LossConfig().for_head(9)
    with pytest.raises(TypeError):
        unet_amd.LossConfig.of(3)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_header_declares_the_entry_points():
    import ctypes
    import unet_amd  # noqa: F401
    from unet_amd._lib import LIB_PATH, parse_header
    protos = parse_header()
    assert protos["uh_focal_tversky_nsums"] == ("int", ["int"])
    assert protos["uh_focal_tversky_sums"] == ("int", ["ptr", "ptr", "int", "int64_t", "int", "ptr", "float", "ptr", "ptr", "size_t", "uh_stream"])
    assert protos["uh_focal_tversky_finish"] == ("int", ["ptr", "int", "double", "double", "ptr", "int", "ptr", "uh_stream"])
    assert protos["uh_focal_tversky_grad"] == ("int", ["ptr", "ptr", "int", "int64_t", "int", "ptr", "float", "double", "double", "ptr", "int",
                                                       "ptr", "ptr", "ptr", "uh_stream"])
    dll = ctypes.CDLL(LIB_PATH)
    for name in ("uh_focal_tversky_nsums", "uh_focal_tversky_sums", "uh_focal_tversky_finish", "uh_focal_tversky_grad"):
        assert hasattr(dll, name), f"{name} is not exported"
    # the pair it stands beside keeps its signatures
    assert protos["uh_ce_dice_sums"] == ("int", ["ptr", "ptr", "int64_t", "int", "ptr", "ptr", "size_t", "uh_stream"])


def test_bad_arguments_return_an_error_code_before_any_launch():
    """Every check sits in front of the launch: no GPU is touched (the device pointers are never followed)."""
    import ctypes
    import unet_amd  # noqa: F401
    from unet_amd._lib import LIB
    LIB.load()
    P = 4096                                                            # a non-null stand-in for a device pointer
    big = LIB.query("uh_loss_ws_bytes", 100)
    fl = lambda *v: (ctypes.c_float * len(v))(*v)
    it = lambda *v: (ctypes.c_int * len(v))(*v)
    assert [LIB.query("uh_focal_tversky_nsums", n) for n in (0, 1, 2, 3, 8, 9)] == [0, 8, 8, 11, 26, 0]

    def sums(ncls=3, weights=fl(1, 1, 1), gamma=2.0, logits=P, ws_bytes=big, mask_div=1, npix=100):
        LIB.call("uh_focal_tversky_sums", logits, P, mask_div, npix, ncls, weights, gamma, P, P, ws_bytes, None)

    def finish(ncls=3, alpha=0.3, beta=0.7, classes=it(1, 2), K=2, out=P):
        LIB.call("uh_focal_tversky_finish", P, ncls, alpha, beta, classes, K, out, None)

    def grad(ncls=3, weights=fl(1, 1, 1), gamma=2.0, alpha=0.3, beta=0.7, classes=it(1, 2), K=2, dl=P):
        LIB.call("uh_focal_tversky_grad", P, P, 1, 100, ncls, weights, gamma, alpha, beta, classes, K, P, None, dl, None)

    for call in (sums, grad):
        with pytest.raises(RuntimeError, match="weight"):
            call(weights=fl(1, 0, 1))
        with pytest.raises(RuntimeError, match="weight"):
            call(weights=fl(1, -2, 1))
        with pytest.raises(RuntimeError, match="weight"):
            call(weights=fl(1, float("nan"), 1))
        with pytest.raises(RuntimeError, match="weights"):
            call(weights=None)
        with pytest.raises(RuntimeError, match="gamma"):
            call(gamma=-0.5)
        with pytest.raises(RuntimeError, match="gamma"):
            call(gamma=float("nan"))
        for ncls in (0, 9, -1):
            with pytest.raises(RuntimeError, match="classes, got"):
                call(ncls=ncls)
    with pytest.raises(RuntimeError, match="workspace too small"):
        sums(ws_bytes=big - 1)
    with pytest.raises(RuntimeError, match="bad args"):
        sums(logits=None)
    with pytest.raises(RuntimeError, match="bad args"):
        sums(npix=0)
    with pytest.raises(RuntimeError, match="mask_div"):
        sums(mask_div=0)
    with pytest.raises(RuntimeError, match="bad args"):
        grad(dl=None)
    for call in (finish, grad):
        with pytest.raises(RuntimeError, match="alpha"):
            call(alpha=0.0, beta=0.0)
        with pytest.raises(RuntimeError, match="alpha"):
            call(alpha=-0.1)
        with pytest.raises(RuntimeError, match="alpha"):
            call(beta=float("nan"))
        with pytest.raises(RuntimeError, match="outside the head"):
            call(classes=it(1, 3))
        with pytest.raises(RuntimeError, match="outside the head"):
            call(ncls=1, classes=it(2), K=1)
        with pytest.raises(RuntimeError, match="twice"):
            call(classes=it(2, 2))
        with pytest.raises(RuntimeError, match="Tversky classes"):
            call(K=0)
        with pytest.raises(RuntimeError, match="Tversky classes"):
            call(classes=None)
        for ncls in (0, 9):
            with pytest.raises(RuntimeError, match="classes, got"):
                call(ncls=ncls)
    with pytest.raises(RuntimeError, match="null"):
        finish(out=None)


# ------------------------------------------------------------------------------------------------ the command line
BASE = ["--model", "UNet_T", "-c", "3", "-b", "4", "-s", "0.5"]


def _state_file(path, argv=(), drop=()):
    """A hand-made --save-state file for BASE + argv; `drop`: keys taken out of its argument record."""
    from unet_amd.train_cli import get_args, run_record
    record = run_record(get_args(BASE + list(argv)))
    for k in drop:
        del record[k]
    state = {"format": 1, "model": {"w": torch.zeros(2)},
             "optimizer": {"square_avg": torch.zeros(4), "momentum_buffer": torch.zeros(4), "ema": None, "ema_updates": 0,
                           "layout": [[0, 2, [2]]], "total": 4, "hyper": {"lr": 1e-5}},
             "epoch": 1, "global_step": 2, "lr": 1e-5, "loader_seed": 1, "augment_seed": None, "args": record}
    torch.save(state, path)
    return str(path)


def test_run_record_holds_the_canonical_loss_spec():
    from unet_amd.train_cli import RECORDED, get_args, run_record
    assert ("loss", "--loss") in RECORDED
    rec = run_record(get_args(BASE + ["--loss", "focal=1, weights=1+2+4,classes=2"]))
    assert rec["loss"] == "focal=1.0,weights=1.0+2.0+4.0,tversky=0.3/0.7,classes=2"
    assert run_record(get_args(BASE + ["--loss"]))["loss"] == "focal=2.0,tversky=0.3/0.7"
    assert run_record(get_args(BASE))["loss"] is None
    assert sorted(rec) == sorted(k for k, _ in RECORDED)


def test_a_malformed_loss_spec_exits_with_status_2(capsys):
    from unet_amd.train_cli import main
    with pytest.raises(SystemExit) as e:
        main(BASE + ["--loss", "focal=-1"])
    assert e.value.code == 2 and "--loss" in capsys.readouterr().err


@pytest.mark.parametrize("argv,says", [(["-c", "3", "--loss", "focal=2,weights=1+2"], "2 class weights"),
                                       (["-c", "1", "--loss", "focal=2,weights=1+2+3"], "3 class weights"),
                                       (["-c", "3", "--loss", "focal=2,classes=3"], "classes")])
def test_a_loss_spec_that_does_not_fit_the_head_exits_with_status_2(caplog, argv, says):
    from unet_amd.train_cli import main
    with caplog.at_level(logging.ERROR):
        assert main(["--model", "UNet_T", "-b", "4"] + argv) == 2
    assert "--loss" in caplog.text and says in caplog.text
    assert "no GPU" not in caplog.text                               # refused for the argument, before a GPU is looked for


@pytest.mark.parametrize("saved,now", [((), ["--loss"]), (["--loss"], []), (["--loss"], ["--loss", "focal=2,tversky=0.5/0.5"])])
def test_resume_refuses_a_differing_loss(tmp_path, caplog, saved, now):
    from unet_amd.train_cli import get_args, load_resume_state, main
    path = _state_file(tmp_path / "train_state.pth", saved)
    args = BASE + now + ["--resume", path]
    with pytest.raises(ValueError, match=r"\-\-loss"):
        load_resume_state(get_args(args))
    with caplog.at_level(logging.ERROR):
        assert main(args) == 2
    assert "--loss" in caplog.text


def test_resume_accepts_the_same_loss_and_a_state_from_before_the_option(tmp_path):
    from unet_amd.train_cli import get_args, load_resume_state
    same = _state_file(tmp_path / "a.pth", ["--loss", "focal=2,tversky=0.3/0.7"])
    assert load_resume_state(get_args(BASE + ["--loss", "--resume", same]))["epoch"] == 1
    old = _state_file(tmp_path / "b.pth", drop=("loss",))              # written before the key existed: reads as None
    assert load_resume_state(get_args(BASE + ["--resume", old]))["epoch"] == 1
    with pytest.raises(ValueError, match=r"\-\-loss"):
        load_resume_state(get_args(BASE + ["--loss", "--resume", old]))
