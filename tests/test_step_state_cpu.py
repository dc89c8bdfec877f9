"""CPU checks of ops.StepState / ops.step_state: the one record a training step installs for the autograd nodes (side stream,
SyncBN group and batch, filter pack, slab batch, fp32 mode) and the context manager that installs and restores it.  Nothing
here calls the library or needs a GPU."""
import pytest
import torch

FIELDS = ("wgrad_stream", "sync_bn", "sync_bn_batch", "weight_pack", "slab_batch", "fp32_mode")


@pytest.fixture()
def ops():
    import unet_amd  # noqa: F401
    from unet_amd import ops
    assert ops.STEP == ops.StepState()
    yield ops
    assert ops.STEP == ops.StepState()


def test_defaults(ops):
    s = ops.StepState()
    assert s._fields == FIELDS
    assert s == (None, None, None, None, None, "exact")
    assert all(getattr(s, f) is None for f in FIELDS[:-1]) and s.fp32_mode == "exact"


def test_installs_what_it_is_given_and_restores(ops):
    before, stream, pack = ops.STEP, object(), object()
    with ops.step_state(wgrad_stream=stream, weight_pack=pack, sync_bn_batch=(4, 2)):
        assert ops.STEP == ops.StepState(wgrad_stream=stream, weight_pack=pack, sync_bn_batch=(4, 2))
        assert ops.STEP.wgrad_stream is stream and ops.STEP.weight_pack is pack
    assert ops.STEP is before
    with ops.step_state():                       # no field: the record that is there stays
        assert ops.STEP == before
    assert ops.STEP is before


def test_restores_after_an_exception(ops):
    before = ops.STEP
    with pytest.raises(RuntimeError, match="inside"):
        with ops.step_state(fp32_mode="bf16x3", slab_batch=object()):
            assert ops.STEP.fp32_mode == "bf16x3"
            raise RuntimeError("inside")
    assert ops.STEP is before


def test_nested_blocks_restore_in_order(ops):
    stream = object()
    with ops.step_state(wgrad_stream=stream):
        outer = ops.STEP
        assert outer == ops.StepState(wgrad_stream=stream)
        with ops.step_state(fp32_mode="bf16x3"):
            assert ops.STEP == ops.StepState(wgrad_stream=stream, fp32_mode="bf16x3")      # the inner block keeps the outer's fields
        assert ops.STEP is outer
    assert ops.STEP == ops.StepState()


def test_refuses_unknown_fields_and_modes(ops):
    with pytest.raises(TypeError):
        with ops.step_state(wgrad_strem=None):
            pass
    for mode in ("fast", "", None, "BF16X3"):
        with pytest.raises(ValueError):
            with ops.step_state(fp32_mode=mode):
                pass
    with pytest.raises(ValueError):              # nothing of a refused call is installed, the valid fields included
        with ops.step_state(wgrad_stream=object(), fp32_mode="tf32"):
            pass


def test_conv_dt_reads_the_installed_mode(ops):
    from unet_amd._lib import UH_BF16, UH_F32, UH_F32X3
    x = torch.zeros(1, 4, 4, 64)
    assert ops.conv_dt(x, 64, 0, 64, True) == UH_F32
    with ops.step_state(fp32_mode="bf16x3"):
        assert ops.conv_dt(x, 64, 0, 64, True) == UH_F32X3
        assert ops.conv_dt(x.bfloat16(), 64, 0, 64, True) == UH_BF16        # bf16 activations are not split
        assert ops.conv_dt(x, 3, 0, 64, False) == UH_F32                    # the stem is not MFMA-aligned
    assert ops.conv_dt(x, 64, 0, 64, True) == UH_F32


def test_the_loose_globals_are_gone(ops):
    assert not any(hasattr(ops, n) for n in ("WGRAD_STREAM", "SYNC_BN", "SYNC_BN_BATCH", "WEIGHT_PACK", "SLAB_BATCH", "FP32_MODE"))
