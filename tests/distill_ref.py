"""Torch-float64 restatement of the distillation term (DESIGN.md section 3 "Distillation"): the value as plain tensor arithmetic
that autograd differentiates, and the closed-form gradient the kernels implement.  Student logits z and teacher logits v are
[n, C] (any leading shape flattened by the caller).  The one-channel head is `two_class_logits(z)`: logits (0, z).

    q = softmax(v / T),  p = softmax(z / T)
    kd    = T^2 / n  sum_x sum_c q_c (log q_c - log p_c)
    agree = 1 / n  sum_x [argmax_c z = argmax_c v]                (first maximum)
    d kd / d z_k = T / n (p_k - q_k)"""
import torch


def two_class_logits(z):
    """[n] one-channel logits -> [n, 2] logits (0, z): p_1 = sigmoid(z), p_0 = sigmoid(-z)."""
    z = z.reshape(-1)
    return torch.stack([torch.zeros_like(z), z], dim=1)


def first_argmax(z):
    """Index of the first maximum of every row (torch.argmax leaves the choice among equal maxima open)."""
    C = z.shape[1]
    is_max = z == z.max(dim=1, keepdim=True).values
    idx = torch.arange(C, device=z.device).expand_as(z)
    return torch.where(is_max, idx, torch.full_like(idx, C)).min(dim=1).values


def loss_terms(z, v, T, n=None):
    """(kd, agree) as float64 0-dim tensors; kd is differentiable w.r.t. z when z is float64 and requires grad.  `n`: the pixel
    count of the mean (default: the rows of z).  Log-probabilities come from log_softmax, never from the log of a rounded
    probability; q_c = 0 contributes 0."""
    z, v = z.double(), v.double()
    n = z.shape[0] if n is None else n
    log_q = torch.log_softmax(v / T, dim=1)
    log_p = torch.log_softmax(z / T, dim=1)
    q = log_q.exp()
    kl = torch.where(q > 0, q * (log_q - log_p), torch.zeros_like(q)).sum()
    agree = (first_argmax(z) == first_argmax(v)).double().sum() / n
    return T * T / n * kl, agree


def autograd_gradient(z, v, T, n=None):
    zz = z.detach().double().requires_grad_(True)
    loss_terms(zz, v, T, n)[0].backward()
    return zz.grad


def closed_form_gradient(z, v, T, n=None):
    """d kd / d z_k = T / n (p_k - q_k)."""
    z, v = z.double(), v.double()
    n = z.shape[0] if n is None else n
    return T / n * (torch.softmax(z / T, dim=1) - torch.softmax(v / T, dim=1))
