"""Batch assembly (csrc/batch.hip, affine.hip, ict.hip, uamt.hip): per-sample flips, the affine warp, the network's input batches in one launch, and
``split_rows`` -- the split of the logits whose backward assembles the batch gradient in place, with the protocol
(``_split_part_of``, ``_scaled_grad``) by which a loss kernel writes its part's rows itself."""
from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor

from .. import _cabi, checks, unet_ops
from .._rt import _DT, _need_gpu, _ptr, _stream, empty_nhwc, fill_zero
from ..stepio import zero_counter
from ._pkg import call


def _flip_raw(x: Tensor, flips: Tensor) -> Tensor:
    _need_gpu(x, flips)
    if x.element_size() not in (2, 4, 8):
        raise ValueError("flip: element size must be 2, 4 or 8 bytes")
    out = torch.empty_like(x)
    n, c, h, w = x.shape
    ist = torch.tensor(x.stride(), dtype=torch.int64)   # host arrays, read on the host side of the C call
    ost = torch.tensor(out.stride(), dtype=torch.int64)
    call("miseg_flip", _stream(), _ptr(x), _ptr(out), n, c, h, w, ist.data_ptr(), ost.data_ptr(), x.element_size(), _ptr(flips))
    return out


class _Flip(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: Tensor, flips: Tensor):
        ctx.save_for_backward(flips)
        return _flip_raw(x, flips)

    @staticmethod
    def backward(ctx, g: Tensor):
        (flips,) = ctx.saved_tensors
        return _flip_raw(g, flips), None  # a flip is its own inverse


def flip(x: Tensor, flips: Tensor) -> Tensor:
    """Per-sample H/W flip of an [N,C,H,W]-shaped tensor (any strides; 2/4/8-byte elements), bit-exact."""
    return _Flip.apply(x, flips) if x.requires_grad else _flip_raw(x, flips)


# ------------------------------------------------------------------------------------------ affine warp (csrc/affine.hip)
_AFFINE_MODES = {"bilinear": 0, "nearest": 1}
AFFINE_MAX_REACH = 8


def affine_inverse(theta: Tensor) -> Tensor:
    """The [N, 2, 3] matrices of the inverse maps: ``[[A | t], [0 0 1]]`` inverted on the host in float64, as float32 on the CPU."""
    t = theta.detach().to("cpu", torch.float64)
    full = torch.zeros(t.shape[0], 3, 3, dtype=torch.float64)
    full[:, :2] = t
    full[:, 2, 2] = 1.0
    try:
        inv = torch.linalg.inv(full)
    except RuntimeError as e:                # torch.linalg.LinAlgError is one
        raise ValueError(f"affine_warp: inverse=True needs invertible matrices ({e})") from None
    return inv[:, :2].to(torch.float32).contiguous()


def affine_reach(theta: Tensor, h: int, w: int) -> int:
    """The ``reach`` that ``miseg_affine_warp_bwd`` needs for these matrices on an ``h`` x ``w`` image (include/miseg_hip.h), from a host
    copy in float64: ceil(largest row sum of |A^-1|) + 1 over the batch, A the linear part in pixels, or ``max(h, w) - 1`` (the whole
    image) if that is smaller.  A singular matrix, or one so large that the forward's fp32 source points stray by a quarter of a pixel
    of the pre-image (|theta| row sums ~1e3 at 2048 pixels), counts as needing the whole image.  The result may exceed
    ``AFFINE_MAX_REACH``: the caller decides what to do then."""
    t = theta.detach().to("cpu", torch.float64)
    h, w = int(h), int(w)
    both = h > 1 and w > 1
    a00 = t[:, 0, 0] if w > 1 else torch.ones_like(t[:, 0, 0])
    a11 = t[:, 1, 1] if h > 1 else torch.ones_like(t[:, 0, 0])
    a01 = t[:, 0, 1] * ((w - 1) / (h - 1)) if both else torch.zeros_like(a00)
    a10 = t[:, 1, 0] * ((h - 1) / (w - 1)) if both else torch.zeros_like(a00)
    det = (a00 * a11 - a01 * a10).abs()
    rowsum = torch.maximum(a11.abs() + a01.abs(), a10.abs() + a00.abs()) / det
    stray = rowsum * 2.0 ** -21 * (t.abs().sum(2).amax(1) + 1.0) * max(h, w)
    need = torch.where(torch.isfinite(rowsum) & (stray <= 0.25), torch.ceil(rowsum) + 1.0, torch.full_like(rowsum, float("inf")))
    return int(max(1.0, min(float(need.max()), float(max(h, w) - 1))))


class _AffineWarp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: Tensor, theta: Tensor, mode: int, channels_last: bool, reach: Optional[int]):
        n, c, h, w = x.shape
        y = torch.empty_like(x)
        call("miseg_affine_warp_fwd", _stream(), _ptr(x), _ptr(theta), n, c, h, w, int(channels_last), mode, _ptr(y))
        ctx.save_for_backward(theta)
        ctx.meta = (n, c, h, w, mode, channels_last, reach)
        return y

    @staticmethod
    def backward(ctx, g: Tensor):
        (theta,) = ctx.saved_tensors
        n, c, h, w, mode, channels_last, reach = ctx.meta
        g = g.float().contiguous(memory_format=torch.channels_last if channels_last else torch.contiguous_format)
        gx = torch.empty_like(g)
        call("miseg_affine_warp_bwd", _stream(), _ptr(g), _ptr(theta), n, c, h, w, int(channels_last), mode, reach, _ptr(gx))
        return gx, None, None, None, None


def affine_warp(x: Tensor, theta: Tensor, mode: str = "bilinear", inverse: bool = False, reach: Optional[int] = None) -> Tensor:
    """``F.grid_sample(x, F.affine_grid(theta, x.shape, align_corners=True), mode, "zeros", align_corners=True)`` for a GPU fp32
    ``x`` [N, C, H, W], contiguous or channels_last (the output has the input's memory format), without the grid; the backward is
    the exact adjoint as a gather, bit-reproducible (include/miseg_hip.h, miseg_affine_warp_fwd / _bwd).  ``theta`` [N, 2, 3] on the
    CPU (uploaded) or on the device; no gradient flows to it.  ``inverse``: warp by the inverse maps (``affine_inverse``; a device
    ``theta`` is read back for it).  ``reach``: the backward's search radius in pixels, 1..8; ``None`` computes it from the host copy
    of the matrices (``affine_reach``) and takes 8 for a device ``theta``, whose matrices the caller then vouches for.  Raises
    ``ValueError`` for anything the kernels do not take, and for matrices whose gradient they cannot cover when ``x`` requires one."""
    if not isinstance(x, Tensor) or not isinstance(theta, Tensor):
        raise ValueError("affine_warp: x and theta must be tensors")
    if not x.is_cuda:
        raise ValueError("affine_warp: x must be a GPU tensor (AffineTensorTransform takes CPU tensors through torch)")
    if x.dtype != torch.float32 or x.dim() != 4 or x.numel() == 0:
        raise ValueError(f"affine_warp: x must be a non-empty fp32 [N, C, H, W] tensor, got {x.dtype} {tuple(x.shape)}")
    if mode not in _AFFINE_MODES:
        raise ValueError(f"affine_warp: mode must be one of {sorted(_AFFINE_MODES)}, got {mode!r}")
    if theta.requires_grad:
        raise ValueError("affine_warp: no gradient with respect to theta; pass theta.detach()")
    n, c, h, w = x.shape
    if tuple(theta.shape) != (n, 2, 3) or not theta.is_floating_point():
        raise ValueError(f"affine_warp: theta must be a floating-point [{n}, 2, 3] tensor, got {tuple(theta.shape)}")
    if x.is_contiguous():
        channels_last = False
    elif x.is_contiguous(memory_format=torch.channels_last):
        channels_last = True
    else:
        raise ValueError("affine_warp: x must be contiguous or channels_last")
    if _cabi.lib().miseg_affine_warp_supported(c, h, w, int(channels_last), _AFFINE_MODES[mode]) < 0 or x.numel() >= 2 ** 31:
        raise ValueError(f"affine_warp: the kernels take 1 <= H, W <= 2048 and fewer than 2^31 elements, got {tuple(x.shape)}")
    if reach is not None and not (isinstance(reach, int) and 1 <= reach <= AFFINE_MAX_REACH):
        raise ValueError(f"affine_warp: reach must be an integer in 1..{AFFINE_MAX_REACH}, got {reach!r}")
    needs_grad = x.requires_grad and torch.is_grad_enabled()
    host = affine_inverse(theta) if inverse else (theta.detach() if not theta.is_cuda else None)
    if host is not None:
        need = affine_reach(host, h, w)
        if needs_grad and need > (AFFINE_MAX_REACH if reach is None else reach):
            raise ValueError(f"affine_warp: the backward would have to search {need} pixels around each pre-image for these matrices, "
                             f"more than {'the limit of 8' if reach is None else f'reach={reach}'}; use torch's grid_sample for them")
        reach = min(need, AFFINE_MAX_REACH) if reach is None else reach
        theta = host
    elif reach is None:
        reach = AFFINE_MAX_REACH
    theta = theta.detach().to(device=x.device, dtype=torch.float32).contiguous()
    return _AffineWarp.apply(x, theta, _AFFINE_MODES[mode], channels_last, int(reach))


# ------------------------------------------------------------------------------------------ split with a layout-preserving backward
_SPLIT_MEMCPY = False   # True: assemble slice gradients with hipMemcpy (slower on a busy device)


class _SplitHolder:
    """Shared by the parts of one ``split_rows``: the batch gradient buffer that the split's backward returns.  A loss kernel whose
    input IS a part writes its scaled gradient straight into that part's rows (``_scaled_grad``: one launch, where autograd would
    multiply into a temporary and the split's backward would copy it over); the backward then only zero-fills the parts without a loss."""
    __slots__ = ("meta", "sizes", "out", "filled")

    def __init__(self, x: Tensor, sizes):
        cl = x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last)
        self.meta, self.sizes, self.out = (tuple(x.shape), x.dtype, x.device, cl), list(sizes), None
        self.filled = set()       # parts whose rows a loss kernel's backward has written in this backward pass

    def buffer(self) -> Tensor:
        if self.out is None:
            shape, dtype, device, cl = self.meta
            self.out = torch.empty(shape, dtype=dtype, device=device, memory_format=torch.channels_last if cl else torch.contiguous_format)
        return self.out

    def rows(self, idx: int) -> Tensor:
        return self.buffer().narrow(0, sum(self.sizes[:idx]), self.sizes[idx])


def _split_part_of(given: Tensor, used: Tensor):
    """(holder, index) if ``used`` -- the tensor the kernel read -- is, unconverted, a part of a split_rows."""
    tag = getattr(given, "_miseg_split", None)
    if tag is None or used.data_ptr() != given.data_ptr() or used.dtype != torch.float32:
        return None
    return tag


def _scaled_grad(part, grad: Tensor, g: Tensor) -> Tensor:
    """``grad * g`` for a 0-d upstream gradient ``g``; for a part of a split_rows, written into the part's rows of the batch
    gradient by one library launch (scale read from device memory) and returned as that view.  Where another loss's backward has
    written those rows already in this pass (two losses on one part: the supervised and the cross term of ``cps``), the product is
    ADDED to them -- two library launches -- and None is returned: autograd holds the rows as the first loss's gradient, whichever
    of the two ran first.  Precondition: every gradient of such a part comes through this function (or ``output_local_mi``'s backward,
    which adds into the rows the same way).  A further consumer that hands autograd an ORDINARY tensor for the part would let it form
    ``rows + tensor`` in a new buffer, possibly before a later in-place addition, which would then be lost; no shipped trainer has one."""
    if part is not None and g.dim() == 0 and g.dtype == torch.float32 and g.is_cuda and grad.dtype == torch.float32 and grad.numel() % 4 == 0:
        holder, idx = part
        dst = holder.rows(idx)
        # (the launch stores 16-byte vectors: rows that start off such a boundary -- odd map sizes -- take the torch product below)
        if dst.dtype == grad.dtype and dst.shape == grad.shape and dst.stride() == grad.stride() and dst.data_ptr() % 16 == 0 and \
                grad.data_ptr() % 16 == 0:
            if idx in holder.filled:
                scaled = torch.empty_like(grad)
                call("miseg_assemble_rows", _stream(), _ptr(scaled), _ptr(grad), _ptr(g), grad.numel(), None, None, 0, None, None, 0)
                call("miseg_axpy", _stream(), 0, _ptr(scaled), _ptr(dst), grad.numel())
                return None
            call("miseg_assemble_rows", _stream(), _ptr(dst), _ptr(grad), _ptr(g), grad.numel(), None, None, 0, None, None, 0)
            holder.filled.add(idx)
            return dst
    return grad * g


class _SplitRows(torch.autograd.Function):
    """``torch.split(x, sizes, dim=0)`` whose backward assembles the gradient directly in x's memory format.

    The logits leave the network as one NHWC batch [labeled | unlabeled | flipped unlabeled] and are split for the losses
    (ref semi_seg/epocher.py:150-152).  Autograd's own split backward concatenates the per-part gradients, and a part without a
    loss (the detached UDA branch) arrives as NCHW zeros: the concatenation then comes out NCHW and the next kernel's NHWC view
    of it is a 4-channel transposing copy -- measured 1.35 ms per step for 50 MB.  Here: one NHWC buffer; parts whose loss kernel
    wrote its rows already (``_scaled_grad``) cost nothing, absent parts are zero-filled, anything else is copied in."""

    @staticmethod
    def forward(ctx, x: Tensor, holder, *sizes: int):
        ctx.sizes = sizes
        ctx.set_materialize_grads(False)    # a part without a loss stays None (materialised it would be NCHW zeros: a transposing copy)
        ctx.meta = (x.shape, x.dtype, x.device, x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last))
        outs, o = [], 0
        for n in sizes:
            outs.append(x.narrow(0, o, n))
            o += n
        ctx.holder = holder
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        shape, dtype, device, cl = ctx.meta
        holder = ctx.holder
        if holder is not None:
            out, holder.out = holder.buffer(), None
            holder.filled = set()
        else:
            out = torch.empty(shape, dtype=dtype, device=device, memory_format=torch.channels_last if cl else torch.contiguous_format)
        o = 0
        for n, g in zip(ctx.sizes, grads):
            part = out.narrow(0, o, n)
            if g is None:
                if part.is_cuda and n and part.data_ptr() % 16 == 0:     # (the library's fill wants a 16-byte boundary)
                    fill_zero(part)
                else:
                    part.zero_()
            elif g.data_ptr() == part.data_ptr() and g.shape == part.shape and g.stride() == part.stride():
                pass                              # its loss kernel's backward wrote these rows (_scaled_grad)
            elif _SPLIT_MEMCPY:
                part.copy_(g)
            else:
                torch.mul(g, 1.0, out=part)   # an elementwise kernel: copy_ of two dense tensors is a hipMemcpyDtoD, seen at 1.5 ms for 16 MB
            o += n
        return (out,) + (None,) * (len(ctx.sizes) + 1)


def split_rows(x: Tensor, sizes) -> tuple:
    holder = _SplitHolder(x, [int(n) for n in sizes]) if x.is_cuda and x.requires_grad else None
    outs = _SplitRows.apply(x, holder, *[int(n) for n in sizes])
    if holder is not None:
        for i, t in enumerate(outs):
            t._miseg_split = (holder, i)
    return outs


def _cat_operands(a: Tensor, b: Tensor, flips: Tensor):
    """The checked, contiguous operands of the two batch-assembly launches: 4-byte [N,C,H,W] tensors of one type and map shape."""
    _need_gpu(a, b, flips)
    a, b = a.contiguous(), b.contiguous()
    assert a.dtype == b.dtype and a.shape[1:] == b.shape[1:] and a.element_size() == 4 and a.dim() == 4, (a.shape, b.shape, a.dtype)
    return a, b, a.shape[0], b.shape[0]


def cat_flip(a: Tensor, b: Tensor, flips: Tensor, stem_dtype=None) -> Tensor:
    """``torch.cat([a, b, flip(b)])`` along dim 0 in one launch (ref semi_seg/epocher.py:148-153: the network's input batch).
    ``stem_dtype`` (bfloat16 / float16, one-channel fp32 images): the same launch also writes the first convolution's operand -- the
    batch cast to that type and padded to one channel vector -- and hangs it on the result (``_miseg_stem``) for ``unet_ops.stem_input``."""
    a, b, na, nb = _cat_operands(a, b, flips)
    out = torch.empty((na + 2 * nb,) + tuple(a.shape[1:]), dtype=a.dtype, device=a.device)
    if stem_dtype in (torch.bfloat16, torch.float16) and a.dtype == torch.float32 and a.shape[1] == 1 and not unet_ops._STEM_KERNELS:      # (read when called: tests switch it)
        pad = empty_nhwc(na + 2 * nb, 8, a.shape[2], a.shape[3], stem_dtype, a.device)
        call("miseg_cat_flip_pad", _stream(), _ptr(a), na, _ptr(b), nb, a.shape[2], a.shape[3], _ptr(flips), _ptr(out), _DT[stem_dtype], _ptr(pad))
        out._miseg_stem = (stem_dtype, pad)
        return out
    call("miseg_cat_flip", _stream(), _ptr(a), na, _ptr(b), nb, a.shape[1], a.shape[2], a.shape[3], _ptr(flips), _ptr(out))
    return out


def cat_flipped(a: Tensor, b: Tensor, flips: Tensor) -> Tensor:
    """``torch.cat([a, flip(b)])`` along dim 0 in one launch: the Mean Teacher student's input batch (ref
    contrastyou/epocher/base_epocher.py:176-181); the teacher reads ``b`` itself."""
    a, b, na, nb = _cat_operands(a, b, flips)
    assert flips.dtype == torch.int32 and flips.numel() >= nb
    out = torch.empty((na + nb,) + tuple(a.shape[1:]), dtype=a.dtype, device=a.device)
    call("miseg_cat_flipped", _stream(), _ptr(a), na, _ptr(b), nb, a.shape[1], a.shape[2], a.shape[3], _ptr(flips), _ptr(out))
    return out


def cat_mixed(a: Tensor, b: Tensor, perm: Tensor, coef: Tensor, check_perm: bool = True) -> Tensor:
    """``torch.cat([a, coef[0] * b + coef[1] * b[perm]])`` along dim 0 in one launch: the ICT student's input batch (DESIGN.md section
    27); the teacher reads ``b`` itself.  fp32 [N,C,H,W]; ``perm`` int32 [Nb] and ``coef`` fp32 [2] on the device (the iteration's step
    block).  A ``perm[i]`` outside [0, Nb) mixes sample i with itself and is flagged; with ``check_perm`` the flag goes to
    ``checks.require_zero``: raised here, or at the iteration's fetch inside a ``checks.deferred`` block."""
    a, b, na, nb = _cat_operands(a, b, perm)
    _need_gpu(coef)
    assert a.dtype == torch.float32 and perm.dtype == torch.int32 and perm.numel() >= nb and perm.is_contiguous(), (a.dtype, perm.dtype, perm.shape)
    assert coef.dtype == torch.float32 and coef.numel() >= 2 and coef.is_contiguous(), (coef.dtype, coef.shape)
    out = torch.empty((na + nb,) + tuple(a.shape[1:]), dtype=a.dtype, device=a.device)
    bad = zero_counter(a.device, (1,))
    call("miseg_cat_mixed", _stream(), _ptr(a), na, _ptr(b), nb, a.shape[1], a.shape[2], a.shape[3], _ptr(perm), _ptr(coef), _ptr(out), _ptr(bad))
    if check_perm:
        checks.require_zero(bad, IndexError, f"cat_mixed: an entry of the permutation lies outside [0, {nb})")
    return out


def noise_add(x: Tensor, seed: Tensor, passes: int, sigma: float, clip: float) -> Tensor:
    """``stack([x + clamp(sigma * z[p], -clip, clip) for p in range(passes)])`` in one launch: the noisy copies the UA-MT teacher sees
    (DESIGN.md section 28).  ``x`` fp32, contiguous; ``seed`` int32 [2] on the device (the low and high word of the 64-bit seed, in the
    iteration's step block); element i of ``z[p]`` is ``normal_fill``'s standard normal for ``(seed, p * x.numel() + i)``.  ``sigma``
    and ``clip`` are constants of the call (and of a recorded tape)."""
    _need_gpu(x, seed)
    assert x.dtype == torch.float32 and x.is_contiguous() and x.numel() > 0, (x.dtype, x.shape, x.stride())
    assert seed.dtype == torch.int32 and seed.numel() >= 2 and seed.is_contiguous(), (seed.dtype, seed.shape)
    assert int(passes) >= 1 and float(sigma) >= 0.0 and float(clip) >= 0.0, (passes, sigma, clip)
    out = torch.empty((int(passes),) + tuple(x.shape), dtype=x.dtype, device=x.device)
    call("miseg_noise_add", _stream(), _ptr(x), x.numel(), int(passes), _ptr(seed), float(sigma), float(clip), _ptr(out))
    return out
