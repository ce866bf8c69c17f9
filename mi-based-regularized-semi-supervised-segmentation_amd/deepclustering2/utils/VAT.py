"""Virtual adversarial training (ref whl:deepclustering2/utils/VAT.py: ``_disable_tracking_bn_stats``, ``_l2_normalize``, ``VATLoss``).

``VATLoss(xi, eps, prop_eps, ip, distance_func)(model, x) -> (lds, (x + r_adv).detach(), r_adv.detach())`` with the reference's four
steps:

1. ``pred = model(x)`` without autograd, in the model's current mode (training: the BatchNorm running statistics move);
2. ``d = l2_normalize(randn_like(x))``, per sample over all of C x H x W;
3. ``ip`` times ``adv = KL(model(x + xi d), pred)``, ``d = l2_normalize(d adv / d d)``;
4. ``lds = KL(model(x + eps prop_eps d), pred)``, the pass that carries the gradient to the parameters.

Steps 3 and 4 run with the BatchNorm tracking switched off (``unet_ops.bn_untracked``): batch statistics, running statistics and
batch counter untouched.  What differs from the wheel, on purpose:

* the model returns LOGITS (the U-Net of this repository does; the wheel's models return a list of simplexes and the class reads
  ``[0]`` -- a list or tuple is still accepted and its first entry taken).  The distance is the wheel's ``KL_div`` on the two
  softmaxes, ``mean_pixels sum_c -t log((p + 1e-16) / (t + 1e-16))``, ``t = softmax(pred)`` detached -- one fused kernel
  (``ops.softmax_kl_consistency`` without flips);
* step 3 differentiates with respect to the PERTURBED IMAGE ``x + xi d`` instead of ``d``: the two gradients differ by the positive
  factor ``xi``, which the normalisation removes;
* the direction pass computes data gradients only (``unet_ops.data_grad_only``).  The wheel's ``adv_distance.backward()`` also
  leaves the direction pass's parameter gradients in every ``param.grad``, where a later ``backward`` adds to them unless the caller
  clears them in between.  Here ``forward`` leaves ``param.grad`` and the flat gradient buffer untouched;
* the random direction comes from the library's counter-based generator (``ops.normal_fill``: Philox4x32-10 + Box-Muller, seeded per
  call), not from torch's;
* a direction of zero or non-finite norm does not produce NaN: the sample gets no perturbation and a device flag is raised through
  ``miseg_amd.checks`` (at once, or with the iteration's report inside a ``checks.deferred`` block, where the guarded Adam skips
  the update).  The wheel fails its ``allclose(norm, 1)`` assertion there.
"""
from __future__ import annotations

from typing import Optional, Union

import torch
from torch import Tensor, nn

from deepclustering2.loss import KL_div

__all__ = ["VATLoss", "_l2_normalize"]


def _l2_normalize(d: Tensor) -> Tensor:
    """``d / ||d||_2`` per sample over every other axis (ref VAT.py:24-29); a new tensor.  On the GPU one library call
    (``ops.l2_perturb``), whose flag for a zero / non-finite norm is checked like the reference's assertion."""
    if d.is_cuda:
        from miseg_amd import checks, ops
        ones = ops.cached_const(("ones", str(d.device), d.shape[0]), lambda: torch.ones(d.shape[0], dtype=torch.float32, device=d.device))
        _, _, out, flag = ops.l2_perturb(d.float(), None, ones, want_d=True)
        checks.require_zero(flag.view(()), AssertionError, "_l2_normalize: a sample's norm is zero or not finite")
        return out.view_as(d)
    norm = d.reshape(d.shape[0], -1).norm(dim=1).view(d.shape[0], *([1] * (d.dim() - 1)))
    return d / norm


class VATLoss(nn.Module):
    def __init__(self, xi: float = 10.0, eps: Union[float, Tensor] = 1.0, prop_eps: float = 0.25, ip: int = 1, distance_func=None):
        super().__init__()
        if int(ip) != ip or int(ip) < 1:
            raise ValueError(f"VATLoss: ip must be an integer >= 1, given {ip!r} (the reference would normalise the random direction only "
                             "and never look at the model)")
        if not isinstance(eps, (float, int, Tensor)):
            raise NotImplementedError(f"eps should be tensor or float, given {eps}.")
        if distance_func is None:
            distance_func = KL_div(verbose=False)
        if not (isinstance(distance_func, KL_div) and distance_func.supports_fused()):
            raise NotImplementedError("VATLoss: the distance is KL_div(reduction='mean', eps=1e-16) without class weights (the fused kernel)")
        self.xi, self.eps, self.prop_eps, self.ip = float(xi), eps, float(prop_eps), int(ip)
        self.distance_func = distance_func

    # ---- per-sample scale vectors [N] on the device
    def _scales(self, x: Tensor):
        from miseg_amd import ops
        n, dev = x.shape[0], x.device
        xi = ops.cached_const(("vat_scale", str(dev), n, self.xi), lambda: torch.full((n,), self.xi, dtype=torch.float32, device=dev))
        if isinstance(self.eps, Tensor):
            if self.eps.numel() != n or self.eps.dim() > 1:
                raise ValueError(f"VATLoss: a tensor eps holds one value per sample, shape [{n}]; given {tuple(self.eps.shape)}")
            radius = (self.eps.detach().to(device=dev, dtype=torch.float32).reshape(n) * self.prop_eps).contiguous()
        else:
            value = float(self.eps) * self.prop_eps
            radius = ops.cached_const(("vat_scale", str(dev), n, value), lambda: torch.full((n,), value, dtype=torch.float32, device=dev))
        return xi, radius

    @staticmethod
    def _logits(out) -> Tensor:
        return out[0] if isinstance(out, (list, tuple)) else out

    def forward(self, model, x: Tensor, *, d0: Optional[Tensor] = None, seed: Optional[int] = None, record: Optional[dict] = None):
        """The wheel's ``forward(model, x)``; the rest is keyword-only.  ``d0``: the initial direction instead of a random one (tests);
        ``seed``: of the random one (default: drawn from Python's ``random``); ``record``: a dict that receives ``pred`` (the clean
        logits), ``d`` (the normalised direction after the initial normalisation and after every iteration) and ``r_adv``."""
        from miseg_amd import checks, ops, unet_ops
        if x.dim() < 2 or x.dtype != torch.float32:
            raise ValueError(f"VATLoss: x is a float32 batch, given {tuple(x.shape)} {x.dtype}")
        xi, radius = self._scales(x)
        x = x.detach().contiguous()
        with unet_ops.bn_float_statistics():
            return self._forward(model, x, xi, radius, d0, seed, record)

    def _forward(self, model, x, xi, radius, d0, seed, record):
        # every pass of the loss -- the clean one too -- on the float batch statistics: the direction is a difference of two passes
        from miseg_amd import checks, ops, unet_ops
        with torch.no_grad():
            pred = self._logits(model(x)).detach()
        if d0 is None:
            if seed is None:
                import random
                seed = random.getrandbits(63)
            g = ops.normal_fill(torch.empty_like(x), seed)
        else:
            if d0.shape != x.shape:
                raise ValueError(f"VATLoss: d0 has the shape of x, given {tuple(d0.shape)} for {tuple(x.shape)}")
            g = d0.detach().to(device=x.device, dtype=torch.float32).contiguous()
        want_d = record is not None
        if want_d:
            record["pred"], record["d"] = pred, []
        flag = None
        with unet_ops.bn_untracked():
            for _ in range(self.ip):
                x_hat, _, d, flag = ops.l2_perturb(g, x, xi, want_d=want_d, flag=flag)
                if want_d:
                    record["d"].append(d)
                x_hat.requires_grad_()
                with unet_ops.data_grad_only():
                    adv = ops.softmax_kl_consistency(self._logits(model(x_hat)), pred, None)
                (g,) = torch.autograd.grad(adv, x_hat)
                g = g.contiguous()
            x_adv, r_adv, d, flag = ops.l2_perturb(g, x, radius, want_r=True, want_d=want_d, flag=flag)
            if want_d:
                record["d"].append(d)
                record["r_adv"] = r_adv
            checks.require_zero(flag.view(()), AssertionError, "VATLoss: a perturbation direction has zero or non-finite norm (the "
                                "reference's allclose(norm, 1) assertion); that sample was left unperturbed")
            lds = ops.softmax_kl_consistency(self._logits(model(x_adv)), pred, None)
        return lds, x_adv.detach(), r_adv.detach()
