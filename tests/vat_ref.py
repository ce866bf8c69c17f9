"""Reference restatement of virtual adversarial training for the tests, written from the description of the
four steps and evaluated with torch autograd on the CPU in whatever dtype the inputs have (float64 for the reference values,
float32 to measure how far a float32 evaluation lands from them):

1. ``pred = model(x, tracked=True)`` without autograd;
2. ``d = l2_normalize(d0)``, per sample over every other axis (``d0`` is injected: the tests do not share a random generator);
3. ``ip`` times ``adv = KL(model(x + xi d, tracked=False), pred)``, ``d = l2_normalize(d adv / d d)``;
4. ``lds = KL(model(x + eps prop_eps d, tracked=False), pred)``, with autograd down to the model's parameters.

``model(x, tracked) -> logits`` is any callable; ``tracked=False`` asks for batch statistics that leave the running statistics and
the batch counter alone.  ``KL(a, b) = mean_pixels sum_c -t log((p + 1e-16) / (t + 1e-16))`` with ``p = softmax(a)``, ``t = softmax(b)``
detached.  Also here: Philox4x32-10 and the Box-Muller map of ``miseg_normal_fill`` in Python integers / numpy.
"""
from __future__ import annotations

from typing import Callable, Sequence, Union

import numpy as np
import torch
from torch import Tensor

KL_EPS = 1e-16


def l2_normalize(d: Tensor) -> Tensor:
    norm = d.reshape(d.shape[0], -1).pow(2).sum(1).sqrt()
    return d / norm.view(-1, *([1] * (d.dim() - 1)))


def kl_logits(logits: Tensor, target_logits: Tensor) -> Tensor:
    p, t = logits.softmax(1), target_logits.detach().softmax(1)
    return (-t * torch.log((p + KL_EPS) / (t + KL_EPS))).sum(1).mean()


def vat(model: Callable[[Tensor, bool], Tensor], x: Tensor, d0: Tensor, xi: float = 10.0, eps: Union[float, Tensor] = 1.0,
        prop_eps: float = 0.25, ip: int = 1) -> dict:
    """{'pred': clean logits, 'd': [the direction after step 2 and after every iteration], 'r_adv', 'x_adv', 'lds'}; ``lds`` carries
    the graph of step 4 (``lds.backward()`` gives the parameter gradients)."""
    assert ip >= 1 and d0.shape == x.shape
    with torch.no_grad():
        pred = model(x, True)
    d = l2_normalize(d0.to(x.dtype))
    ds = [d]
    for _ in range(ip):
        d = d.detach().clone().requires_grad_()
        adv = kl_logits(model(x + xi * d, False), pred)
        (g,) = torch.autograd.grad(adv, d)
        d = l2_normalize(g)
        ds.append(d)
    if torch.is_tensor(eps):
        assert eps.shape == (x.shape[0],)
        radius = eps.to(x.dtype).view(-1, *([1] * (x.dim() - 1))) * prop_eps
    else:
        radius = float(eps) * prop_eps
    r_adv = (d * radius).detach()
    lds = kl_logits(model(x + r_adv, False), pred)
    return {"pred": pred, "d": ds, "r_adv": r_adv, "x_adv": x + r_adv, "lds": lds}


class _RoundBF16(torch.autograd.Function):
    """A bf16 rounding point in ANY float dtype: the value is rounded to bf16 going forward and kept in its own dtype; going backward
    the gradient is rounded too where the kernels store it in bf16 (``grad=True``: activations), and passed through for a weight
    operand or the image (``grad=False``: their gradients stay fp32 on the device)."""

    @staticmethod
    def forward(ctx, x, grad):
        ctx.round_grad = grad
        return x.bfloat16().to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return (g.bfloat16().to(g.dtype) if ctx.round_grad else g), None


def unet_bf16_rounded(sd: dict, x: Tensor) -> Tensor:
    """The U-Net in training mode on batch statistics (nothing is tracked) with the bf16 kernels' rounding points -- the image and
    every weight operand rounded to bf16, exact products accumulated in the evaluation's dtype, batch statistics from the un-rounded
    accumulators, the raw convolution output, every stored activation and their gradients rounded to bf16, logits unrounded --
    restated from the description of oracle.unet.unet_forward_bf16_autograd so that it also runs in float64 (the oracle's roundings
    return float32).  In float32 it is that function."""
    import torch.nn.functional as F
    r = _RoundBF16.apply

    def cbr(t, ck, bk):
        acc = F.conv2d(t, r(sd[f"{ck}.weight"], False), None, 1, 1)
        mean = acc.mean((0, 2, 3), keepdim=True)
        var = acc.var((0, 2, 3), unbiased=False, keepdim=True)
        scale = sd[f"{bk}.weight"].view(1, -1, 1, 1) * torch.rsqrt(var + 1e-5)
        shift = sd[f"{bk}.bias"].view(1, -1, 1, 1) - mean * scale
        return r(F.relu(r(acc, True) * scale + shift), True)

    def block(name, t):
        return cbr(cbr(t, f"{name}.conv.0", f"{name}.conv.1"), f"{name}.conv.3", f"{name}.conv.4")

    def pool(t):
        return F.max_pool2d(t, 2, 2)
    e1 = block("Conv1", r(x, False))
    e2 = block("Conv2", pool(e1))
    e3 = block("Conv3", pool(e2))
    e4 = block("Conv4", pool(e3))
    d = block("Conv5", pool(e4))
    for lvl, skip in ((5, e4), (4, e3), (3, e2), (2, e1)):
        u = cbr(F.interpolate(d, scale_factor=2, mode="nearest"), f"Up{lvl}.up.1", f"Up{lvl}.up.2")
        d = block(f"Up_conv{lvl}", torch.cat((skip, u), 1))
    return F.conv2d(d, sd["DeConv_1x1.weight"], sd["DeConv_1x1.bias"])


def oracle_model(sd: dict, bf16: bool = False) -> Callable[[Tensor, bool], Tensor]:
    """The oracle U-Net over the state dict ``sd`` in training mode: ``tracked`` passes move the running statistics in ``sd``.
    ``bf16``: ``unet_bf16_rounded`` (it never tracks: the comparison does not look at the running statistics)."""
    from oracle import unet as OU

    def run(x: Tensor, tracked: bool) -> Tensor:
        if bf16:
            return unet_bf16_rounded(sd, x)
        return OU.unet_forward(sd, x, True, tracked)[0]
    return run


def rel_l2(got: Tensor, ref: Tensor) -> float:
    return float((got.double() - ref.double()).norm() / ref.double().norm())


def rel_l2_per_sample(got: Tensor, ref: Tensor) -> float:
    """Worst sample's relative L2 distance."""
    return max(rel_l2(got[i], ref[i]) for i in range(ref.shape[0]))


# ---------------------------------------------------------------------------------------------------------------- the generator
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(counter: Sequence[int], key: Sequence[int]) -> tuple:
    """Philox4x32 with ten rounds (Salmon et al., SC'11) on Python integers."""
    c0, c1, c2, c3 = (int(v) & MASK for v in counter)
    k0, k1 = (int(v) & MASK for v in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & MASK, p1 & MASK, ((p0 >> 32) ^ c3 ^ k1) & MASK, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def philox_words(seed: int, offset: int, n: int) -> np.ndarray:
    """uint32 words of elements [offset, offset + n): element j is word j & 3 of the block with counter (lo32(j >> 2), hi32(j >> 2),
    0, 0) and key (lo32(seed), hi32(seed))."""
    seed &= (1 << 64) - 1
    out, cache = np.empty(n, dtype=np.uint32), {}
    for i in range(n):
        j = offset + i
        b = j >> 2
        if b not in cache:
            cache = {b: philox4x32_10((b & MASK, b >> 32, 0, 0), (seed & MASK, seed >> 32))}
        out[i] = cache[b][j & 3]
    return out


def normals_from_words(words: np.ndarray, offset: int) -> np.ndarray:
    """float64 Box-Muller values of ``miseg_normal_fill``'s map for elements [offset, offset + n), given their words and those of
    their pair partners: ``words`` must cover whole blocks of four (offset and n multiples of 4)."""
    assert offset % 4 == 0 and words.size % 4 == 0
    w = words.reshape(-1, 2, 2).astype(np.int64)
    u1 = ((w[:, :, 0] >> 8) + 1) * 2.0 ** -24
    u2 = (w[:, :, 1] >> 8) * 2.0 ** -24
    rad, ang = np.sqrt(-2.0 * np.log(u1)), 2.0 * np.pi * u2
    return np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=-1).reshape(-1)
