"""Float64 restatement of the ICT trainer's three kernels (csrc/ict.hip): the batch assembly that mixes and the
two consistency losses whose target is a mixture of two teacher rows, with their gradients with respect to the student's logits
written out by hand.  Shared by test_cpu_ict.py, which checks the restatement against float64 autograd and finite differences, and
test_gpu_ict.py, which runs the kernels against it.

Conventions: logits are [N, C, H, W]; ``perm`` is a sequence of N integers and the mix is a GATHER -- sample i's partner is
``perm[i]``; an entry outside [0, N) counts as i (``clean_perm``).  ``c0`` and ``c1`` are the two float32 coefficients the step block
holds, taken as exact in float64 (``coefficients``).  eps = 1e-16, means as in pixel_ref.py.
"""
from __future__ import annotations

import numpy as np
import torch

F64 = torch.float64
EPS = 1e-16


def coefficients(lam: float):
    """(c0, c1) as the host stages them: float32(lam) and float32(1 - lam), the subtraction in double; returned as Python floats."""
    lam = float(lam)
    return float(np.float32(lam)), float(np.float32(1.0 - lam))


def clean_perm(perm, n: int):
    """The permutation with every entry outside [0, n) replaced by its own index, and the number of such entries."""
    out = [int(p) if 0 <= int(p) < n else i for i, p in enumerate(perm)]
    return out, sum(1 for i, p in enumerate(perm) if not 0 <= int(p) < n)


def mix_rows(b: torch.Tensor, perm, c0: float, c1: float) -> torch.Tensor:
    """c0 * b_i + c1 * b_perm[i] in float64."""
    idx, _ = clean_perm(perm, b.shape[0])
    b64 = b.to(F64)
    return c0 * b64 + c1 * b64[torch.tensor(idx, dtype=torch.long)]


def cat_mixed(a: torch.Tensor, b: torch.Tensor, perm, c0: float, c1: float) -> torch.Tensor:
    """[a | mix(b)] in float64."""
    return torch.cat([a.to(F64), mix_rows(b, perm, c0, c1)])


def cat_mixed_bound(b: torch.Tensor, perm, c0: float, c1: float) -> torch.Tensor:
    """3 * 2^-24 * (|c0 x| + |c1 y|) per mixed element: three roundings, or two with a fused multiply-add."""
    idx, _ = clean_perm(perm, b.shape[0])
    b64 = b.to(F64)
    return 3.0 * 2.0 ** -24 * ((c0 * b64).abs() + (c1 * b64[torch.tensor(idx, dtype=torch.long)]).abs())


def target(b64: torch.Tensor, perm, c0: float, c1: float) -> torch.Tensor:
    """q = c0 * softmax(b_i) + c1 * softmax(b_perm[i]) at the same pixel, detached."""
    return mix_rows(b64.detach().to(F64).softmax(1), perm, c0, c1)


def mse_expr(a64: torch.Tensor, b64: torch.Tensor, perm, c0: float, c1: float) -> torch.Tensor:
    """mean over N*C*H*W of (softmax(a) - q)^2."""
    return ((a64.softmax(1) - target(b64, perm, c0, c1)) ** 2).mean()


def klcons_expr(a64: torch.Tensor, b64: torch.Tensor, perm, c0: float, c1: float) -> torch.Tensor:
    """mean_pix sum_c -q_c log((p_c + eps) / (q_c + eps)), p = softmax(a)."""
    p, q = a64.softmax(1), target(b64, perm, c0, c1)
    return (-q * torch.log((p + EPS) / (q + EPS))).sum(1).mean()


EXPR = {"mse": mse_expr, "klcons": klcons_expr}


def loss_and_grad(kernel: str, a: torch.Tensor, b: torch.Tensor, perm, c0: float, c1: float):
    """(loss, d loss / d a) in float64, the gradient by hand: d/da_c = p_c (g_c - <g, p>) / npix through the softmax Jacobian with
    g = 2 (p - q) / C (mse) or -q / (p + eps) (klcons).  Nothing flows to b."""
    a64, b64 = a.detach().to(F64), b.detach().to(F64)
    p, q = a64.softmax(1), target(b64, perm, c0, c1)
    n, c, h, w = p.shape
    if kernel == "mse":
        loss = ((p - q) ** 2).mean()
        g = 2.0 * (p - q) / c
    else:
        loss = (-q * torch.log((p + EPS) / (q + EPS))).sum(1).mean()
        g = -q / (p + EPS)
    return loss, p * (g - (g * p).sum(1, keepdim=True)) / (n * h * w)


def autograd_loss_and_grad(kernel: str, a: torch.Tensor, b: torch.Tensor, perm, c0: float, c1: float):
    """The same pair by float64 autograd of the expression: the check of ``loss_and_grad``."""
    a64 = a.detach().to(F64).clone().requires_grad_(True)
    loss = EXPR[kernel](a64, b.detach().to(F64), perm, c0, c1)
    loss.backward()
    return loss.detach(), a64.grad


def draws(seed: int, ub: int, mix_alpha: float):
    """(lam, perm) of one iteration as the semantics state them: numpy's global generator seeded with ``seed``, the Beta draw, then
    the permutation.  The caller's generator state is put back."""
    state = np.random.get_state()
    try:
        np.random.seed(seed)
        lam = float(np.random.beta(mix_alpha, mix_alpha))
        perm = [int(p) for p in np.random.permutation(ub)]
    finally:
        np.random.set_state(state)
    return lam, perm
