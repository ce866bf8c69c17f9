"""Virtual adversarial training (csrc/vat.hip): the per-sample L2 perturbation and the counter-based normal generator."""
from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor

from .._cabi import query
from .._rt import _need_gpu, _ptr, _stream, _ws
from ..stepio import zero_counter
from ._pkg import call


def l2_perturb(g: Tensor, x: Optional[Tensor], scale: Tensor, want_r: bool = False, want_d: bool = False, flag: Optional[Tensor] = None):
    """Per sample ``d = g / ||g||_2`` (over everything but dim 0), ``r = scale[n] * d``, ``out = x + r`` in one library call
    (``miseg_l2_perturb``; the norm is a fixed-order double sum).  Returns ``(out, r, d, flag)`` -- ``out`` is None without ``x``, ``r``
    / ``d`` unless wanted; ``flag`` = int32 device counter of samples whose norm is zero or not finite (they get d = r = 0: no NaN)."""
    _need_gpu(g, x, scale, flag)
    g = g.contiguous()
    n, m = g.shape[0], g.numel() // max(g.shape[0], 1)
    assert g.dtype == torch.float32 and scale.dtype == torch.float32 and scale.is_contiguous() and scale.numel() == n, (g.dtype, scale.shape)
    if x is not None:
        x = x.contiguous()
        assert x.dtype == torch.float32 and x.shape == g.shape, (x.shape, g.shape)
    assert x is not None or want_r or want_d
    out = torch.empty_like(g) if x is not None else None
    r = torch.empty_like(g) if want_r else None
    d = torch.empty_like(g) if want_d else None
    if flag is None:
        flag = zero_counter(g.device, (1,))
    ws = _ws(query("miseg_l2_perturb_ws_bytes", n, m), g.device)
    call("miseg_l2_perturb", _stream(), _ptr(g), _ptr(x), _ptr(scale), n, m, _ptr(out), _ptr(r), _ptr(d), _ptr(flag), _ptr(ws), ws.numel())
    return out, r, d, flag


def _as_i64(v: int) -> int:
    v = int(v) & 0xFFFFFFFFFFFFFFFF
    return v - (1 << 64) if v >= (1 << 63) else v


def normal_fill(out: Tensor, seed: int, offset: int = 0) -> Tensor:
    """Fill the contiguous fp32 tensor ``out`` with standard normals: element i depends on ``(seed, offset + i)`` only (Philox4x32-10 +
    Box-Muller, ``miseg_normal_fill``) -- ``normal_fill(a, s, 0)`` over n elements equals two fills of k and n - k at offsets 0 and k."""
    _need_gpu(out)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() > 0
    call("miseg_normal_fill", _stream(), _as_i64(seed), int(offset), _ptr(out), out.numel())
    return out


def philox_words(n: int, seed: int, offset: int = 0, device="cuda") -> Tensor:
    """The 32-bit words under ``normal_fill``'s elements [offset, offset + n), as int32 bit patterns (``miseg_philox_fill``)."""
    out = torch.empty(int(n), dtype=torch.int32, device=device)
    call("miseg_philox_fill", _stream(), _as_i64(seed), int(offset), _ptr(out), out.numel())
    return out
