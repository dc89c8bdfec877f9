"""CPU checks of UNet_SA / SpatialAttention / AttentionUp (fixture set G17, tests/golden/make_golden_sa.py): the module tree
has the reference's state_dict layout and initialisation order, the C ABI declares the spatial-attention entry points, the
product path refuses CPU tensors, and the torch restatement of the attention map that the GPU tests compare against is
pinned to the reference's own SpatialAttention."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden


def sa_map_ref(x, w):
    """SpatialAttention.forward (unet_parts.py:50-60) in stock torch: x [B,C,H,W], w [1,2,k,k] -> [B,1,H,W]."""
    k = w.shape[-1]
    pooled = torch.cat([x.mean(dim=1, keepdim=True), x.max(dim=1, keepdim=True)[0]], dim=1)
    return torch.sigmoid(F.conv2d(pooled, w, padding=k // 2))


def test_unet_sa_state_dict_matches_g17():
    import unet_amd
    r = load_golden("g17_unet_sa_convt_3class")
    sd = unet_amd.UNet_SA(1, 3, False).state_dict()
    assert list(sd) == [str(n) for n in r["sd0_names"]]
    for (k, v), shape in zip(sd.items(), r["sd0_shapes"]):
        assert ",".join(str(d) for d in v.shape) == str(shape), k
    assert [k for k in sd if "attention" in k] == [f"up{j}.attention.conv1.weight" for j in range(1, 5)]
    assert tuple(sd["up1.attention.conv1.weight"].shape) == (1, 2, 7, 7)


def test_unet_sa_seeded_init_matches_g17():
    """torch.manual_seed(0) + ctor gives the reference's initial weights: parameters are created in its order
    (up, conv, attention inside every decoder block)."""
    import unet_amd
    r = load_golden("g17_unet_sa_convt_3class")
    torch.manual_seed(0)
    sd = unet_amd.UNet_SA(1, 3, False).state_dict()
    for (k, v), want, scale in zip(sd.items(), r["sd0_sums"], r["sd0_abs_sums"]):
        assert abs(float(v.double().sum()) - want) <= 1e-9 * max(scale, 1.0), k
        assert abs(float(v.double().abs().sum()) - scale) <= 1e-9 * max(scale, 1.0), k


def test_unet_sa_bilinear_keys_match_g17_bf16_fixture():
    import unet_amd
    r = load_golden("g17_bf16_unet_sa_bilinear_64")
    names = [k for k, p in unet_amd.UNet_SA(1, 1, True).named_parameters()]
    assert names == [str(n) for n in r["grad_names"]]


def test_attention_up_and_module_surface():
    import unet_amd
    for bilinear in (True, False):
        m = unet_amd.AttentionUp(16, 8, bilinear)
        plain = unet_amd.Up(16, 8, bilinear)
        keys = list(m.state_dict())
        assert keys == list(plain.state_dict()) + ["attention.conv1.weight"]
        assert m.use_attention is True and isinstance(m.attention, unet_amd.SpatialAttention)
        r = load_golden(f"g17_up_sa_{'bilinear' if bilinear else 'convt'}_16_8")
        assert keys == [k[4:] for k in r if k.startswith("sd0.")]
    for k in (3, 7):
        sa = unet_amd.SpatialAttention(k)
        assert tuple(sa.conv1.weight.shape) == (1, 2, k, k) and sa.conv1.bias is None
        assert sa.conv1.padding == (k // 2, k // 2)
    with pytest.raises(AssertionError):
        unet_amd.SpatialAttention(5)
    with pytest.raises(NotImplementedError, match="AttentionUp"):
        unet_amd.Up(16, 8, True, use_attention=True)
    with pytest.raises(NotImplementedError):
        unet_amd.UNet_SA(1, 1).use_checkpointing()


def test_cpu_tensors_are_refused():
    import unet_amd
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        unet_amd.SpatialAttention()(torch.rand(2, 8, 16, 16))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        unet_amd.AttentionUp(16, 8, True)(torch.rand(1, 8, 8, 8), torch.rand(1, 8, 16, 16))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        unet_amd.UNet_SA(1, 1)(torch.rand(1, 1, 32, 32))


def test_spatial_attention_prototypes_parse():
    import unet_amd  # noqa: F401
    from unet_amd._lib import LIB, parse_header
    protos = parse_header()
    assert protos["uh_spatial_attn_dw_nblk"] == ("int", ["int", "int", "int"])
    ret, fwd = protos["uh_spatial_attn_fwd"]
    assert ret == "int" and len(fwd) == 15 and fwd[-1] == "uh_stream" and fwd[3] == "int"
    ret, bwd = protos["uh_spatial_attn_bwd"]
    assert ret == "int" and len(bwd) == 22 and bwd[-1] == "uh_stream" and bwd.count("ptr") == 11
    LIB.load()
    assert LIB.query("uh_spatial_attn_dw_nblk", 8, 512, 512) == 1024
    assert LIB.query("uh_spatial_attn_dw_nblk", 1, 1, 1) == 1
    assert protos["uh_spatial_attn_plan"] == ("int", ["int", "int", "int", "ptr"])
    out = (ctypes.c_int64 * 3)()
    assert LIB.query("uh_spatial_attn_plan", 64, 1, 1, ctypes.addressof(out)) == 0 and list(out) == [8, 8, 1]
    assert LIB.query("uh_spatial_attn_plan", 64, 1, 0, ctypes.addressof(out)) == 0 and list(out) == [1, 64, 1]
    # shape checks run on the host before anything is enqueued
    with pytest.raises(RuntimeError, match="k is 3 or 7"):
        LIB.call("uh_spatial_attn_fwd", 16, 8, 16, 5, 16, 16, 16, None, 8, 1, 4, 4, 8, 0, None)
    with pytest.raises(RuntimeError, match="exactly one"):
        LIB.call("uh_spatial_attn_bwd", None, 0, None, None, 0, 16, 7, 16, 16, 16, 16, 16, 8, 16, 16, 1, 1, 4, 4, 8, 0, None)


@pytest.mark.parametrize("k", [7, 3])
def test_torch_restatement_pinned_to_g17(k):
    """sa_map_ref (what the GPU tests compare the kernels with, in fp64) against the reference's SpatialAttention in G17,
    including the gradient routing of the max to the FIRST maximal channel on tied pixels."""
    r = load_golden(f"g17_sa_k{k}")
    w = torch.from_numpy(r["sd0.conv1.weight"]).double().requires_grad_(True)
    x = torch.from_numpy(r["x0"]).double().requires_grad_(True)
    y = sa_map_ref(x, w)
    y.backward(torch.from_numpy(r["cot"]).double())
    np.testing.assert_allclose(y.detach().numpy(), r["y"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(x.grad.numpy(), r["dx0"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(w.grad.numpy(), r["grad.conv1.weight"], rtol=1e-5, atol=1e-5)
    assert ((r["x0"] == r["x0"].max(axis=1, keepdims=True)).sum(axis=1) > 1).any(), "the fixture holds tied maxima"
