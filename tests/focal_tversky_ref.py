"""Torch-float64 restatement of the focal + Tversky loss (DESIGN.md section 3 "Focal / Tversky loss"): the value as plain tensor
arithmetic that autograd differentiates, and the closed-form gradient the kernels implement.  Logits are [n, C] (any leading
shape flattened by the caller), labels int [n].  The one-channel head is `two_class_logits(z)`: logits (0, z).
A label outside [0, C) matches no class (what ft_pixel of csrc/focal_loss.hip documents): its indicator row tau is zero, its weight
w_t is 0 -- the pixel adds nothing to F, W, TP or T -- and it still counts in P_c = sum p_c."""
import torch

EPS = 1e-6


def two_class_logits(z):
    """[n] one-channel logits -> [n, 2] logits (0, z): p_1 = sigmoid(z), p_0 = sigmoid(-z)."""
    z = z.reshape(-1)
    return torch.stack([torch.zeros_like(z), z], dim=1)


def default_classes(C):
    return tuple(range(1, C))


def indicators(t, C):
    """(tau [n, C] float64, inside [n] bool): one_hot(t) for labels in [0, C), a zero row for a label outside the head."""
    t = t.long()
    inside = (t >= 0) & (t < C)
    tau = torch.nn.functional.one_hot(torch.where(inside, t, torch.zeros_like(t)), C).double() * inside[:, None].double()
    return tau, inside


def _pieces(z, t, w):
    z = z.double()
    C = z.shape[1]
    w = torch.as_tensor(w, dtype=torch.float64, device=z.device)
    logp = z - torch.logsumexp(z, dim=1, keepdim=True)              # log p_t = z_t - logsumexp, never log of a rounded p
    p = logp.exp()
    tau, inside = indicators(t, C)
    # u = sum_{c != t} p_c, never 1 - p_t; in log space, so that autograd stays finite where u underflows to 0 (outside the
    # head nothing is left out: u = 1)
    log_u = torch.logsumexp(z.masked_fill(tau.bool(), float("-inf")), dim=1) - torch.logsumexp(z, dim=1)
    nlp = -(logp * tau).sum(dim=1)
    wt = w[torch.where(inside, t.long(), torch.zeros_like(t.long()))] * inside.double()
    return p, tau, log_u, nlp, wt


def focal_term(z, t, w, gamma):
    p, tau, log_u, nlp, wt = _pieces(z, t, w)
    mod = torch.exp(gamma * log_u)                                  # u^gamma; gamma = 0: 1, also at u = 0
    return (wt * mod * nlp).sum() / wt.sum()


def tversky_term(z, t, alpha, beta, classes=None):
    z = z.double()
    C = z.shape[1]
    p = torch.softmax(z, dim=1)
    tau, _ = indicators(t, C)
    TP, P, T = (p * tau).sum(dim=0), p.sum(dim=0), tau.sum(dim=0)
    TI = (TP + EPS) / ((1.0 - alpha - beta) * TP + alpha * P + beta * T + EPS)
    K = list(default_classes(C) if classes is None else classes)
    return (1.0 - TI[K]).sum() / len(K)


def loss_terms(z, t, w, gamma, alpha, beta, classes=None):
    """(total, focal, tversky) as float64 0-dim tensors; differentiable w.r.t. z when z is float64 and requires grad."""
    f = focal_term(z, t, w, gamma)
    tv = tversky_term(z, t, alpha, beta, classes)
    return f + tv, f, tv


def autograd_gradient(z, t, w, gamma, alpha, beta, classes=None, focal=True, tversky=True):
    zz = z.detach().double().requires_grad_(True)
    total = zz.sum() * 0.0
    if focal:
        total = total + focal_term(zz, t, w, gamma)
    if tversky:
        total = total + tversky_term(zz, t, alpha, beta, classes)
    total.backward()
    return zz.grad


def focal_gradient(z, t, w, gamma):
    """dL/dz_k = w_t / W s (tau_k - p_k), s = gamma u^gamma q r - u^gamma, q = p_t, r = log(q) / u (-1 at u = 0)."""
    p, tau, log_u, nlp, wt = _pieces(z, t, w)
    u = log_u.exp()
    if gamma == 0:
        s = -torch.ones_like(u)
    else:
        q = (p * tau).sum(dim=1)
        r = torch.where(u > 0, -nlp / torch.where(u > 0, u, torch.ones_like(u)), -torch.ones_like(u))
        mod = torch.exp(gamma * log_u)
        s = gamma * mod * q * r - mod
    return (wt / wt.sum() * s)[:, None] * (tau * u[:, None] - (1.0 - tau) * p)          # tau_k - p_k; 1 - p_t is u


def tversky_gradient(z, t, alpha, beta, classes=None):
    """g_c = -[c in K] / |K| (tau_c D_c - N_c ((1 - alpha - beta) tau_c + alpha)) / D_c^2; dL/dz_k = p_k (g_k - sum_c p_c g_c)."""
    z = z.double()
    C = z.shape[1]
    p = torch.softmax(z, dim=1)
    tau, _ = indicators(t, C)
    TP, P, T = (p * tau).sum(dim=0), p.sum(dim=0), tau.sum(dim=0)
    N = TP + EPS
    D = (1.0 - alpha - beta) * TP + alpha * P + beta * T + EPS
    K = list(default_classes(C) if classes is None else classes)
    ind = torch.zeros(C, dtype=torch.float64, device=z.device)
    ind[K] = 1.0 / len(K)
    g = -ind * (tau * D - N * ((1.0 - alpha - beta) * tau + alpha)) / (D * D)
    return p * (g - (p * g).sum(dim=1, keepdim=True))


def closed_form_gradient(z, t, w, gamma, alpha, beta, classes=None):
    return focal_gradient(z, t, w, gamma) + tversky_gradient(z, t, alpha, beta, classes)
