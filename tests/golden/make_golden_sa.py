#!/usr/bin/env python3
"""Generate fixture set G17 (spatial attention) under tests/golden/ by running the REFERENCE's own modules.

Run in the build container only (like make_golden.py, it imports the reference's modules at run time; nothing is copied):

    python tests/golden/make_golden_sa.py

G17:
  g17_sa_k7 / g17_sa_k3            SpatialAttention(k) forward + backward on ReLU inputs with all-zero pixels and tied maxima
  g17_up_sa_{bilinear,convt}_16_8  Up(16, 8, bilinear, use_attention=True) forward + backward, plus the odd-padding forms
  g17_unet_sa_convt_3class         UNet_SA(1,3,bilinear=False) 3-step trajectory at 2x1x64x64, seeded init (the shape of G16)
  g17_bf16_unet_sa_bilinear_64     UNet_SA(1,1,bilinear=True) step 0 in fp32 and under autocast('cpu', bf16) (the shape of G15)
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import (module_fwd_bwd, npy, randomize_bn, ref_train_steps_amp, save,  # noqa: E402
                         synth_batch)
from unet.unet_parts import SpatialAttention, Up  # noqa: E402  (the reference's, on make_golden's path)
from unet.unet_model import UNet_SA              # noqa: E402


SMALL = 1 << 12          # tensors of at most this many elements are stored whole in the trajectory fixture


def tied_relu_input(g, b, c, h, w):
    """ReLU output with the cases the max's gradient routing depends on: pixels where every channel is 0, and pixels whose
    maximum is held by two channels (the gradient goes to the lower one)."""
    x = torch.relu(torch.randn(b, c, h, w, generator=g))
    x[:, :, ::4, ::3] = 0.0
    if c >= 6:
        x[:, 2, 1::2, ::2] = 9.0
        x[:, 5, 1::2, ::2] = 9.0
    return x


def g17_spatial_attention():
    g = torch.Generator().manual_seed(170)
    for k, c in ((7, 24), (3, 16)):
        torch.manual_seed(171 + k)
        m = SpatialAttention(k)
        module_fwd_bwd(m, [tied_relu_input(g, 2, c, 15, 19)], f"g17_sa_k{k}")


def g17_up_attention():
    g = torch.Generator().manual_seed(172)
    cases = (("g17_up_sa_bilinear_16_8", True, (8, 8, 8), (8, 16, 16)),
             ("g17_up_sa_bilinear_16_8_oddpad", True, (8, 8, 9), (8, 17, 19)),
             ("g17_up_sa_convt_16_8", False, (16, 8, 8), (8, 16, 16)),
             ("g17_up_sa_convt_16_8_oddpad", False, (16, 8, 9), (8, 17, 19)))
    for i, (name, bilinear, s1, s2) in enumerate(cases):
        torch.manual_seed(173 + i)
        m = Up(16, 8, bilinear=bilinear, use_attention=True)
        randomize_bn(m, 177 + i)
        x1 = torch.randn(2, *s1, generator=g)
        x2 = tied_relu_input(g, 2, *s2)
        module_fwd_bwd(m, [x1, x2], name)


def g17_unet_sa_trajectory():
    """UNet_SA(1, 3, bilinear=False), CE + multiclass Dice, 3 fp32 steps; weights = torch.manual_seed(0) + ctor (not stored;
    per-tensor sums are), as G16 does for UNet_S."""
    torch.manual_seed(0)
    m = UNet_SA(1, 3, bilinear=False)
    init = {k: v.detach().clone() for k, v in m.state_dict().items()}
    batches = [synth_batch(1700 + s, 2, 1, 64, 64, nmask=3) for s in range(3)]
    full = ref_train_steps_amp(m, batches, 3, False)
    # under 1 MiB: every logit and scalar, the gradients / final values of the small tensors, L2 norms and sums of all
    rec = {k: v for k, v in full.items() if not (k.startswith("s0.grad.") or k.startswith("sd3.")) or v.size <= SMALL}
    grads = {k[len("s0.grad."):]: v for k, v in full.items() if k.startswith("s0.grad.")}
    rec["grad_names"] = np.array(list(grads))
    rec["grad_l2"] = np.array([np.linalg.norm(v.astype(np.float64)) for v in grads.values()])
    final = {k[len("sd3."):]: v for k, v in full.items() if k.startswith("sd3.")}
    rec["sd3_names"] = np.array(list(final))
    rec["sd3_sums"] = np.array([float(v.astype(np.float64).sum()) for v in final.values()])
    rec["sd3_l2"] = np.array([np.linalg.norm(v.astype(np.float64)) for v in final.values()])
    rec["sd0_names"] = np.array(list(init))
    rec["sd0_shapes"] = np.array([",".join(str(d) for d in v.shape) for v in init.values()])
    rec["sd0_sums"] = np.array([float(v.double().sum()) for v in init.values()])
    rec["sd0_abs_sums"] = np.array([float(v.double().abs().sum()) for v in init.values()])
    for s, (im, mk) in enumerate(batches):
        rec[f"s{s}.images"], rec[f"s{s}.masks"] = npy(im), npy(mk)
    save("g17_unet_sa_convt_3class", **rec)


def g17_bf16_unet_sa():
    """UNet_SA(1,1,bilinear=True) (torch.manual_seed(0) + ctor) on 2x1x64x64, step 0, fp32 and bf16 autocast: logits, loss
    terms, gradient norm, per-tensor gradient L2 norms and (bf16 - fp32) differences, gradients of tensors <= 2^15 elements."""
    g = torch.Generator().manual_seed(1701)
    images = torch.rand(2, 1, 64, 64, generator=g)
    masks = torch.randint(0, 3, (2, 64, 64), generator=g)
    rec = {"images": npy(images), "masks": npy(masks)}
    grads = {}
    for tag, amp in (("ref32", False), ("ref16", True)):
        torch.manual_seed(0)
        m = UNet_SA(1, 1, bilinear=True)
        r = ref_train_steps_amp(m, [(images, masks)], 1, amp)
        grads[tag] = {k[8:]: v for k, v in r.items() if k.startswith("s0.grad.")}
        rec.update({tag + "." + k: v for k, v in r.items() if k.startswith("s0.") and not k.startswith("s0.grad.")})
    names = list(grads["ref32"])
    rec["grad_names"] = np.array(names)
    rec["grad_l2.ref32"] = np.array([np.linalg.norm(grads["ref32"][k].astype(np.float64)) for k in names])
    rec["grad_l2.ref16"] = np.array([np.linalg.norm(grads["ref16"][k].astype(np.float64)) for k in names])
    rec["grad_l2.diff"] = np.array([np.linalg.norm(grads["ref16"][k].astype(np.float64) - grads["ref32"][k]) for k in names])
    for k in names:
        if grads["ref32"][k].size <= 1 << 15:
            rec["ref32.grad." + k], rec["ref16.grad." + k] = grads["ref32"][k], grads["ref16"][k]
    rec["note"] = np.array("UNet_SA(1,1,True): torch.manual_seed(0) + ctor; data Generator(1701): rand(2,1,64,64), randint(0,3); "
                           "gradients are AFTER clip_grad_norm_(1.0)")
    save("g17_bf16_unet_sa_bilinear_64", **rec)


if __name__ == "__main__":
    g17_spatial_attention()
    g17_up_attention()
    g17_unet_sa_trajectory()
    g17_bf16_unet_sa()
