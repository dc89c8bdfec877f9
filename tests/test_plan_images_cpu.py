"""CPU checks of the pinned launch plan (csrc/conv3x3.hip: fwd_plan's plan_B; csrc/convt_mfma.hip: uh_convt2x2_mfma_ok_plan) and of
the switches built on it: ops.plan_images, BatchPredictor(batch_invariant=True).launch_lengths and the command-line flags.  The
queries are host-only, so nothing here needs a GPU.  The grid is the one of tests/test_conv_plan_cpu.py."""
import pytest

from test_conv_plan_cpu import _grid

LARGE = 5


@pytest.fixture(scope="module")
def lib():
    import unet_amd  # noqa: F401
    from unet_amd._lib import LIB
    LIB.load()
    return LIB


def test_sum_classes(lib):
    """Codes 1, 2 and 4 are exported as one class (same K-chunk order, same MFMA, same epilogue); 0, 3 and 5 stand alone."""
    cls = [lib.query("uh_conv3x3_fwd_sum_class", k) for k in range(6)]
    assert cls[1] == cls[2] == cls[4]
    assert len({cls[0], cls[1], cls[3], cls[5]}) == 4
    assert lib.query("uh_conv3x3_fwd_sum_class", -1) < 0
    assert lib.query("uh_conv3x3_fwd_sum_class", 6) < 0


def test_pinned_kernel_is_the_one_image_kernel(lib):
    same = lambda a, b: lib.query("uh_conv3x3_fwd_sum_class", a) == lib.query("uh_conv3x3_fwd_sum_class", b)
    pinned_ksplit_past_its_threshold = large = 0
    for dt, B, h, w, cin, cout in _grid():
        own = lib.query("uh_conv3x3_fwd_kernel", B, h, w, cin, 0, cout, dt)
        one = lib.query("uh_conv3x3_fwd_kernel", 1, h, w, cin, 0, cout, dt)
        got = lib.query("uh_conv3x3_fwd_kernel_plan", B, 1, h, w, cin, 0, cout, dt)
        if own == LARGE:
            assert got == LARGE, (dt, B, h, w, cin, cout)            # the real B is past the 2 GiB window
            large += 1
        else:
            assert got == one or same(got, one), (dt, B, h, w, cin, cout, got, one)
            assert got == one or got == own, (dt, B, h, w, cin, cout, got, one, own)     # never a third form
        pinned_ksplit_past_its_threshold += got == 3 and own != 3
        # plan_B = 0 is the unpinned plan
        assert lib.query("uh_conv3x3_fwd_kernel_plan", B, 0, h, w, cin, 0, cout, dt) == own, (dt, B, h, w, cin, cout)
        # the filter may be packed fragment-major exactly when codes 1-4 run the pinned call
        assert lib.query("uh_conv3x3_wfrag_ok_plan", B, 1, h, w, cin, 0, cout, cin, 0, cout, dt) == (1 <= got <= 4)
        assert lib.query("uh_conv3x3_wfrag_ok_plan", B, 0, h, w, cin, 0, cout, cin, 0, cout, dt) == (1 <= own <= 4)
    assert pinned_ksplit_past_its_threshold > 0 and large > 0
    # UNet at 8 x 512 x 512, level 2 (128 x 128, 256 -> 256): 512 tiles x 4 slabs, K split all the same
    assert lib.query("uh_conv3x3_fwd_kernel", 8, 128, 128, 256, 0, 256, 1) == 1
    assert lib.query("uh_conv3x3_fwd_kernel_plan", 8, 1, 128, 128, 256, 0, 256, 1) == 3
    # a plan longer than the launch: one image under the plan of eight
    assert lib.query("uh_conv3x3_fwd_kernel_plan", 1, 8, 128, 128, 256, 0, 256, 1) == 1


def test_pinned_queries_refuse_bad_arguments(lib):
    assert lib.query("uh_conv3x3_fwd_kernel_plan", 0, 1, 16, 16, 64, 0, 64, 1) < 0
    assert lib.query("uh_conv3x3_fwd_kernel_plan", 1, -1, 16, 16, 64, 0, 64, 1) < 0
    assert lib.query("uh_conv3x3_fwd_kernel_plan", 1, 1, 16, 16, 64, 0, 64, 7) < 0
    assert lib.query("uh_conv3x3_fwd_kernel_plan", 1, 1, 16, 0, 64, 0, 64, 1) < 0
    assert lib.query("uh_conv3x3_wfrag_ok_plan", 1, -1, 16, 16, 64, 0, 64, 64, 0, 64, 1) == 0
    # the pinned calls check the plan length before they touch a pointer
    assert lib.query("uh_conv3x3_fwd_affine_relu_plan", None, 64, 64, None, 0, 0, None, None, 64, 64, None, None, 1, -1, 16, 16, 1,
                     None) < 0
    assert lib.query("uh_conv3x3_fwd_narrow_plan", None, 64, 16, 16, None, 0, 0, 0, None, None, 16, 64, 16, None, None, None, 1, -1,
                     16, 16, 1, None) < 0


def test_pinned_transposed_convolution_choice(lib):
    ok = lambda B, h, w, dt=1: lib.query("uh_convt2x2_mfma_ok", B, h, w, 128, 64, 2 * h, 2 * w, dt)
    okp = lambda B, p, h, w, dt=1: lib.query("uh_convt2x2_mfma_ok_plan", B, p, h, w, 128, 64, 2 * h, 2 * w, dt)
    # 62 x 62 = 3844 pixels: not a multiple of 32 alone, eight of them are -- pinned: the SIMT kernel for the whole batch
    assert ok(1, 62, 62) == 0 and ok(8, 62, 62) == 1
    assert okp(8, 1, 62, 62) == 0 and okp(8, 0, 62, 62) == 1
    # an image that qualifies alone keeps the GEMM at every B
    for B in range(1, 9):
        assert ok(1, 64, 64) == 1 and okp(B, 1, 64, 64) == 1
        for h, w in ((62, 62), (64, 64), (37, 87), (125, 124)):
            for dt in (0, 1):
                assert okp(B, 1, h, w, dt) == ok(1, h, w, dt)
                assert okp(B, 0, h, w, dt) == ok(B, h, w, dt)
    assert okp(0, 1, 64, 64) == 0 and okp(1, -1, 64, 64) == 0
    # a real-B limit still counts: the output of 64 images of 1024 x 1024 x 64 bf16 channels passes 2 GiB
    assert ok(1, 512, 512) == 1 and okp(64, 1, 512, 512) == 0


def test_plan_images_switch():
    import unet_amd  # noqa: F401
    from unet_amd import ops
    assert ops.PLAN_IMAGES == 0
    with ops.plan_images(1):
        assert ops.PLAN_IMAGES == 1
        with ops.plan_images(0):
            assert ops.PLAN_IMAGES == 0
        assert ops.PLAN_IMAGES == 1
    assert ops.PLAN_IMAGES == 0
    with pytest.raises(ValueError):
        with ops.plan_images(-1):
            pass
    with pytest.raises(RuntimeError):
        with ops.plan_images(1):
            raise RuntimeError("inside")
    assert ops.PLAN_IMAGES == 0


SIZES = ((512, 512), (384, 512), (999, 1000), (700, 300))


def _predictor(ctor, args, **kw):
    import unet_amd
    from unet_amd.predict import LaunchPlanner
    return LaunchPlanner(getattr(unet_amd, ctor)(*args), 8, True, **kw)          # no device: launch_lengths only asks the library


@pytest.mark.parametrize("ctor,args,off", [
    ("UNet", (1, 3), [1, 1, 1, 1]),
    ("UNet_S", (1, 3, False), [8, 8, 2, 7]),
    ("UNet_S", (1, 3, True), [8, 8, 2, 7]),
    ("UNet_SA", (1, 3), [8, 8, 2, 7]),
])
def test_launch_lengths_batch_invariant(lib, ctor, args, off):
    p = _predictor(ctor, args, batch_invariant=True)
    assert [p.launch_lengths(H, W) for H, W in SIZES] == [list(range(1, 9))] * 4
    # off, and constructed with the default: the lengths tests/test_conv_plan_cpu.py pins
    for attrs in ({"batch_invariant": False}, {}):
        p = _predictor(ctor, args, **attrs)
        assert [p.launch_lengths(H, W) for H, W in SIZES] == [list(range(1, n + 1)) for n in off]


def test_launch_lengths_keep_the_real_batch_limits(lib):
    """The last Up block of UNet reads 128 channels at level 0: at 1024 x 1024 in bf16 that is 2^28 bytes per image, so eight
    images reach the 2 GiB window (another kernel, code 5) and the pinned plan stops at seven."""
    p = _predictor("UNet", (1, 3), batch_invariant=True)
    p.batch = 10
    assert p.launch_lengths(1024, 1024) == list(range(1, 8))


def test_command_lines_parse_the_flags(capsys):
    from unet_amd import predict_cli, seg_main
    base = ["-m", "m.pth", "-i", "x.png"]
    assert predict_cli.get_args(base).batch_invariant is True
    assert predict_cli.get_args(base + ["--no-batch-invariant"]).batch_invariant is False
    assert predict_cli.get_args(base + ["--batch-invariant"]).batch_invariant is True
    seg = ["--input-raw", "d", "--width", "4", "--height", "4", "-ww", "2", "-wl", "1", "-m", "m.pth"]
    assert seg_main.build_parser().parse_args(seg).batch_invariant is False
    assert seg_main.build_parser().parse_args(seg + ["--batch-invariant"]).batch_invariant is True
    for parser, flag in ((predict_cli.build_parser(), "--no-batch-invariant"), (seg_main.build_parser(), "--batch-invariant")):
        with pytest.raises(SystemExit):
            parser.parse_args(["--help"])
        assert flag in capsys.readouterr().out


def test_constructors_take_the_keyword():
    import inspect
    from unet_amd.inference import GraphedForward
    from unet_amd.predict import BatchPredictor
    from unet_amd.seg_main import ContourPipeline
    assert inspect.signature(BatchPredictor.__init__).parameters["batch_invariant"].default is False
    assert inspect.signature(ContourPipeline.__init__).parameters["batch_invariant"].default is False
    assert inspect.signature(GraphedForward.__init__).parameters["plan_images"].default == 0


@pytest.mark.parametrize("lengths", [[1], [1, 2, 7], [1, 3], [1, 3, 5, 7], [1, 2, 3, 5, 6, 7], list(range(1, 9))])
def test_cut_is_the_greedy_split(lengths):
    """LaunchPlanner.cut: every piece an allowed length, the pieces sum to n, each the largest length that fits what is left."""
    from unet_amd.predict import LaunchPlanner
    p = LaunchPlanner(None, 8, True)
    p.lengths[(48, 64)] = lengths                  # the public cache: no model and no library are asked
    for n in range(1, 21):
        pieces = p.cut(n, 48, 64)
        assert sum(pieces) == n and all(b in lengths for b in pieces)
        left = n
        for b in pieces:
            assert b == max(v for v in lengths if v <= left)
            left -= b
    assert p.cut(0, 48, 64) == []
