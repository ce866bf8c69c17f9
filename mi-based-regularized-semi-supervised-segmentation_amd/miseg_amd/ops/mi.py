"""Mutual-information losses (csrc/mi_local.hip, mi_local_loss.hip, mi_global.hip, mi_out.hip): the local MI of a probability pair
or of all sub-heads of a tap, the global MI, the local MI on the network output -- they share the loss epilogue ``_local_loss`` -- and
the arithmetic the local-MI contraction runs in."""
from __future__ import annotations

import os
from typing import List, Optional, Sequence, Tuple

import torch
from torch import Tensor

from .. import _cabi
from .._cabi import query
from .._rt import _need_gpu, _ptr, _stream, _ws, cached_const, empty_nhwc, fill_zero, logits_nhwc, windows_tensor
from ..stepio import scalar_out
from ._pkg import call, mi_planes
from .batch import _split_part_of       # the shared piece: output-level MI writes its gradients into the parts of a split_rows

MI_PRECISIONS = {"fp32": 0, "bf16x3": 1, "bf16": 2, "f16f8": 3}
_mi_precision = MI_PRECISIONS.get(os.environ.get("MISEG_MI_PRECISION", "fp32"), 0)     # rebound by set_mi_precision: read it HERE only


def set_mi_precision(mode: str) -> None:
    """Arithmetic of the local-MI contraction: 'fp32' (exact fp32 MFMA, default), 'bf16x3' (bf16 MFMA on hi/lo-split
    operands: fp32-class accuracy at 3/16 of the MFMA time), 'f16f8' (f16 hi x hi + both cross terms K-concatenated on the
    block-scaled fp8 pipe: the same accuracy class at 2/3 of bf16x3's matrix time; kernels that have no such form take bf16x3)
    or 'bf16' (plain bf16 operands)."""
    global _mi_precision
    _mi_precision = MI_PRECISIONS[mode]


def resolve_mi_precision(compute_dtype, requested: Optional[str] = None) -> str:
    """The local-MI arithmetic a trainer runs with: the ``MISEG_MI_PRECISION`` environment variable if set (an override for A/B
    runs), else the model's ``Arch.mi_precision`` config key, else by the U-Net's storage type -- exact fp32 MFMA for
    ``Arch.compute_dtype=float32`` (the parity mode), the f16 + fp8 split for bfloat16 / float16 (the benchmarked arithmetic)."""
    env = os.environ.get("MISEG_MI_PRECISION")
    mode = env or requested or ("fp32" if compute_dtype in (torch.float32, "float32", "fp32", None) else "f16f8")
    if mode not in MI_PRECISIONS:
        raise ValueError(f"mi_precision must be one of {sorted(MI_PRECISIONS)}, got {mode!r}")
    return mode


def mi_precision_code() -> int:
    """The current arithmetic as the kernels' argument (the launch tape's key reads it: a recorded step holds it as a constant)."""
    return _mi_precision


def mi_precision_name() -> str:
    return next(k for k, v in MI_PRECISIONS.items() if v == _mi_precision)


def colour_windows(windows: Sequence[Tuple[int, int, int, int]]) -> List[List[int]]:
    """Greedy colouring of overlapping windows into pairwise-disjoint groups (deterministic backward:
    each group is one launch with plain read-modify-write, groups run in stream order)."""
    groups: List[List[int]] = []
    for idx, (h0, h1, w0, w1) in enumerate(windows):
        for grp in groups:
            if all(h1 <= windows[j][0] or windows[j][1] <= h0 or w1 <= windows[j][2] or windows[j][3] <= w0 for j in grp):
                grp.append(idx)
                break
        else:
            groups.append([idx])
    return groups


def _int_windows(windows) -> list:
    return [tuple(int(v) for v in w) for w in windows]


def _pixels(windows, which=None) -> int:
    """Pixels covered by the windows (those with the indices ``which``), overlaps counted once per window."""
    return sum((h1 - h0) * (w1 - w0) for h0, h1, w0, w1 in (windows if which is None else (windows[i] for i in which)))


def _local_fwd(x: Tensor, y: Tensor, mask, pad: int, windows, win: Tensor, raw: Tensor, precision: Optional[int] = None) -> None:
    """raw[P][T][T][K][K] of one (x, y) pair: both contiguous [N,K,H,W] fp32 (possibly views into a larger tensor)."""
    n, k, h, w = x.shape
    p, t = len(windows), 2 * pad + 1
    ws = _ws(query("miseg_iic_local_joint_ws_bytes", n, k, h, w, pad, p), x.device)
    px = _pixels(windows)
    call("miseg_iic_local_joint_fwd", _stream(), _ptr(x), _ptr(y), _ptr(mask), n, k, h, w, pad, _ptr(win), p, _ptr(raw),
         _ptr(ws), ws.numel(), _mi_precision if precision is None else precision, work=(2.0 * k * k * t * t * n * px, 2.0 * n * k * px * 4),
         tag=f"iic_local_joint_fwd[p{pad}]")


def _is_whole(windows, h: int, w: int) -> bool:
    return len(windows) == 1 and tuple(windows[0]) == (0, h, 0, w)


def _local_bwd(x: Tensor, y: Tensor, mask, pad: int, windows, win: Tensor, grad_raw: Tensor, scale: Tensor, gx: Tensor,
               gy: Tensor) -> None:
    """gx, gy (same layout as x, y): overwritten for a single whole-image window, accumulated into otherwise (caller
    zero-fills).  Overlapping windows are split into disjoint colour groups, one launch each, in stream order."""
    n, k, h, w = x.shape
    whole = _is_whole(windows, h, w)
    bws = _ws(query("miseg_iic_local_bwd_ws_bytes", k, pad, len(windows)), x.device)
    tt = (2 * pad + 1) ** 2
    for grp in colour_windows(windows):
        if len(grp) == len(windows):
            gwin, ggrad, gscale = win, grad_raw, scale
        else:
            idx = cached_const(("idx", str(x.device), tuple(grp)), lambda: torch.tensor(grp, dtype=torch.long, device=x.device))
            gwin, ggrad, gscale = win[idx].contiguous(), grad_raw[idx].contiguous(), scale[idx].contiguous()
        px = _pixels(windows, grp)
        call("miseg_iic_local_bwd", _stream(), _ptr(x), _ptr(y), _ptr(mask), n, k, h, w, pad, _ptr(gwin), len(grp),
             _ptr(ggrad), _ptr(gscale), _ptr(gx), _ptr(gy), 0 if whole else 1, _mi_precision, _ptr(bws), bws.numel(),
             work=(4.0 * k * k * tt * n * px, 4.0 * n * k * px * 4), tag=f"iic_local_bwd[p{pad}]")


class _LocalMI(torch.autograd.Function):
    """loss[P] of IIDSegmentationLoss over P windows (ref: contrastyou/losses/iic_loss.py:107-149)."""

    @staticmethod
    def forward(ctx, x: Tensor, y: Tensor, mask: Optional[Tensor], pad: int, windows, lamda: float):
        _need_gpu(x, y, mask)
        x, y = x.contiguous().float(), y.contiguous().float()
        mask = None if mask is None else mask.contiguous().float()
        n, k, h, w = x.shape
        p = len(windows)
        dev = x.device
        win = windows_tensor(windows, dev)
        t = 2 * pad + 1
        raw = torch.empty(p, t, t, k, k, dtype=torch.float32, device=dev)
        _local_fwd(x, y, mask, pad, windows, win, raw)
        loss = scalar_out((p,), dev)
        grad_raw = torch.empty_like(raw)
        _local_loss(raw, k, pad, p, lamda, loss, grad_raw)
        ctx.save_for_backward(x, y, mask, grad_raw, win)
        ctx.pad, ctx.windows = pad, list(windows)
        ctx.raw = raw
        return loss

    @staticmethod
    def backward(ctx, gloss: Tensor):
        x, y, mask, grad_raw, win = ctx.saved_tensors
        n, k, h, w = x.shape
        whole = _is_whole(ctx.windows, h, w)
        gx, gy = (torch.empty_like(x), torch.empty_like(y)) if whole else (torch.zeros_like(x), torch.zeros_like(y))
        _local_bwd(x, y, mask, ctx.pad, ctx.windows, win, grad_raw, gloss.contiguous().float(), gx, gy)
        return gx, gy, None, None, None, None


# miseg_iic_local_loss_fwd gives each of its 16 waves 3 K^2 + 4 K floats of LDS and refuses above 156 KiB: K <= 28 fits
# (tests/test_gpu_mi_loss.py pins 28 accepted / 29 refused).  The joint forward and the backward take K up to 32.
LOCAL_LOSS_SINGLE_BLOCK_MAX_K = 28


def _local_loss(raw: Tensor, k: int, pad: int, p: int, lamda: float, loss: Tensor, grad_raw: Tensor) -> None:
    """Loss epilogue of the local MI (ref iic_loss.py:124-146).  pad >= 2: one block per (window, displacement) -- the single
    block per window needs ceil((2 pad + 1)^2 / 16) rounds on one CU while the IIC chain waits for it.  The same form whenever
    the single block cannot hold K (it has no such limit; the numbers of grad_raw are the same bits either way)."""
    if pad >= 2 or k > LOCAL_LOSS_SINGLE_BLOCK_MAX_K:
        ws = _ws(query("miseg_iic_local_loss_ws_bytes", pad, p), raw.device)
        call("miseg_iic_local_loss_fwd_ws", _stream(), _ptr(raw), k, pad, p, float(lamda), _ptr(loss), _ptr(grad_raw), _ptr(ws), ws.numel())
    else:
        call("miseg_iic_local_loss_fwd", _stream(), _ptr(raw), k, pad, p, float(lamda), _ptr(loss), _ptr(grad_raw))


class _LocalMIHeads(torch.autograd.Function):
    """All S sub-heads of one decoder tap in one node: probs[S, 2*UB, K, H, W] holds, per sub-head, the UB maps of the
    flipped features followed by the UB maps of the transformed image (ref semi_seg/epocher.py:264-272 evaluates the
    criterion once per sub-head on ``p[:ub], p[ub:]``).  loss[S][P]; the backward writes every sub-head's gradient
    straight into one gprob[S, 2*UB, K, H, W] buffer, so autograd never materialises per-slice zero-padded copies."""

    @staticmethod
    def forward(ctx, probs: Tensor, ub: int, mask: Optional[Tensor], pad: int, windows, lamda: float):
        _need_gpu(probs, mask)
        probs = probs.contiguous().float()
        mask = None if mask is None else mask.contiguous().float()
        s, n2, k, h, w = probs.shape
        if n2 != 2 * ub:
            raise _cabi.MisegError(f"local_mi_heads: probs holds {n2} maps per sub-head, expected 2*{ub}")
        p, t, dev = len(windows), 2 * pad + 1, probs.device
        win = windows_tensor(windows, dev)
        raw = torch.empty(s, p, t, t, k, k, dtype=torch.float32, device=dev)
        planes = None
        if mask is None:    # every sub-head in one launch
            ws = _ws(max(query("miseg_iic_local_joint_ws_bytes", ub, k, h, w, pad, p * s),
                         query("miseg_iic_local_joint_ws_bytes", ub, k, h, w, pad, p)), dev)   # batched launch | per-head fallback
            px = _pixels(windows)
            nplanes = query("miseg_iic_local_planes_bytes", s, ub, k, h, w, pad) if mi_planes() and _mi_precision == MI_PRECISIONS["f16f8"] else 0
            if nplanes > 0:
                # the joint forward also writes every probability out as the backward's operand images (f16 hi, two e4m3 planes,
                # pixel-major): the backward's source rows are then plain memory -> LDS copies, and this node keeps the planes, not probs
                planes = torch.empty(nplanes, dtype=torch.uint8, device=dev)
                call("miseg_iic_local_joint_fwd_heads_planes", _stream(), _ptr(probs), s, ub, k, h, w, pad, _ptr(win), p, _ptr(raw), _ptr(ws),
                     ws.numel(), _ptr(planes), nplanes, work=(2.0 * k * k * t * t * ub * px * s, 2.0 * ub * k * px * (4 + 4.4) * s),
                     tag=f"iic_local_joint_fwd[p{pad}]")
            else:
                call("miseg_iic_local_joint_fwd_heads", _stream(), _ptr(probs), s, ub, k, h, w, pad, _ptr(win), p, _ptr(raw), _ptr(ws), ws.numel(),
                     _mi_precision, work=(2.0 * k * k * t * t * ub * px * s, 2.0 * ub * k * px * 4 * s), tag=f"iic_local_joint_fwd[p{pad}]")
        else:
            for i in range(s):
                _local_fwd(probs[i, :ub], probs[i, ub:], mask, pad, windows, win, raw[i])
        loss = scalar_out((s, p), dev)
        grad_raw = torch.empty_like(raw)
        _local_loss(raw, k, pad, s * p, lamda, loss, grad_raw)
        ctx.save_for_backward(planes if planes is not None else probs, mask, grad_raw, win)
        ctx.pad, ctx.windows, ctx.ub, ctx.planes, ctx.shape = pad, list(windows), ub, planes is not None, tuple(probs.shape)
        return loss

    @staticmethod
    def backward(ctx, gloss: Tensor):
        probs, mask, grad_raw, win = ctx.saved_tensors
        s, _, k, h, w = ctx.shape
        ub = ctx.ub
        gprob = torch.empty(ctx.shape, dtype=torch.float32, device=probs.device)
        if not _is_whole(ctx.windows, h, w):
            fill_zero(gprob)
        scale = gloss.contiguous().float()
        if mask is None:
            whole = _is_whole(ctx.windows, h, w)
            tt = (2 * ctx.pad + 1) ** 2
            bws = _ws(query("miseg_iic_local_bwd_ws_bytes", k, ctx.pad, len(ctx.windows) * s), probs.device)   # >= the per-head size
            for grp in colour_windows(ctx.windows):
                if len(grp) == len(ctx.windows):
                    gwin, ggrad, gscale = win, grad_raw, scale
                else:
                    dev = probs.device
                    idx = cached_const(("idx32", str(dev), tuple(grp)), lambda: torch.tensor(grp, dtype=torch.int32, device=dev))
                    gwin = cached_const(("gwin", str(dev), tuple(ctx.windows), tuple(grp)), lambda: win[idx.long()].contiguous())
                    npw, per = len(ctx.windows), grad_raw[0, 0].numel()
                    ggrad = torch.empty((s, len(grp)) + tuple(grad_raw.shape[2:]), dtype=torch.float32, device=dev)
                    gscale = torch.empty((s, len(grp)), dtype=torch.float32, device=dev)
                    call("miseg_gather_rows", _stream(), _ptr(grad_raw), _ptr(ggrad), s, npw, len(grp), _ptr(idx), per)
                    call("miseg_gather_rows", _stream(), _ptr(scale), _ptr(gscale), s, npw, len(grp), _ptr(idx), 1)
                px = _pixels(ctx.windows, grp)
                if ctx.planes:
                    call("miseg_iic_local_bwd_heads_planes", _stream(), _ptr(probs), probs.numel(), s, ub, k, h, w, ctx.pad, _ptr(gwin), len(grp),
                         _ptr(ggrad), _ptr(gscale), _ptr(gprob), 0 if whole else 1, _ptr(bws), bws.numel(),
                         work=(4.0 * k * k * tt * ub * px * s, 2.0 * ub * k * px * (4.4 + 4) * s), tag=f"iic_local_bwd[p{ctx.pad}]")
                else:
                    call("miseg_iic_local_bwd_heads", _stream(), _ptr(probs), s, ub, k, h, w, ctx.pad, _ptr(gwin), len(grp), _ptr(ggrad),
                         _ptr(gscale), _ptr(gprob), 0 if whole else 1, _mi_precision, _ptr(bws), bws.numel(),
                         work=(4.0 * k * k * tt * ub * px * s, 4.0 * ub * k * px * 4 * s), tag=f"iic_local_bwd[p{ctx.pad}]")
        else:
            for i in range(s):
                _local_bwd(probs[i, :ub], probs[i, ub:], mask, ctx.pad, ctx.windows, win, grad_raw[i], scale[i], gprob[i, :ub],
                           gprob[i, ub:])
        return gprob, None, None, None, None, None


def local_mi_heads(probs: Tensor, ub: int, pad: int, windows, lamda: float = 1.0, mask: Optional[Tensor] = None) -> Tensor:
    """loss[S][P] for probs[S, 2*UB, K, H, W] (see _LocalMIHeads)."""
    return _LocalMIHeads.apply(probs, int(ub), mask, int(pad), _int_windows(windows), float(lamda))


def local_mi_losses(x: Tensor, y: Tensor, pad: int, windows, lamda: float = 1.0, mask: Optional[Tensor] = None) -> Tensor:
    return _LocalMI.apply(x, y, mask, int(pad), _int_windows(windows), float(lamda))


def local_mi_raw_joint(x: Tensor, y: Tensor, pad: int, windows, mask: Optional[Tensor] = None, precision: Optional[str] = None) -> Tensor:
    """raw[P][T][T][K][K] only (no autograd) -- exposed for parity tests of the contraction."""
    _need_gpu(x, y, mask)
    x, y = x.contiguous().float(), y.contiguous().float()
    k, t = x.shape[1], 2 * pad + 1
    raw = torch.empty(len(windows), t, t, k, k, dtype=torch.float32, device=x.device)
    _local_fwd(x, y, mask, pad, windows, windows_tensor(windows, x.device), raw, None if precision is None else MI_PRECISIONS[precision])
    return raw


# ------------------------------------------------------------------------------------------ global MI
def _global_outputs(s: int, k: int, dev):
    """(loss[S] in the iteration's arena, loss_no_lamb[S], joint[S,K,K]) of a global-MI forward."""
    loss = scalar_out((s,), dev)
    return loss, torch.empty_like(loss), torch.empty(s, k, k, dtype=torch.float32, device=dev)


class _GlobalMI(torch.autograd.Function):
    """IIDLoss for S sub-heads at once: x, y [S,N,K] -> (loss[S], loss_no_lamb[S], joint[S,K,K])."""

    @staticmethod
    def forward(ctx, x: Tensor, y: Tensor, lamb: float):
        _need_gpu(x, y)
        x, y = x.contiguous().float(), y.contiguous().float()
        s, n, k = x.shape
        loss, loss_nl, joint = _global_outputs(s, k, x.device)
        call("miseg_iic_global_fwd", _stream(), _ptr(x), _ptr(y), s, n, k, float(lamb), _ptr(loss), _ptr(loss_nl), _ptr(joint))
        ctx.save_for_backward(x, y)
        ctx.lamb = float(lamb)
        ctx.mark_non_differentiable(loss_nl, joint)
        ctx.set_materialize_grads(False)      # (autograd would fill zero gradients for the two non-differentiable outputs: two launches)
        return loss, loss_nl, joint

    @staticmethod
    def backward(ctx, gloss, _g1, _g2):
        if gloss is None:
            return None, None, None
        x, y = ctx.saved_tensors
        s, n, k = x.shape
        gx, gy = torch.empty_like(x), torch.empty_like(y)
        up = gloss.contiguous().float()
        call("miseg_iic_global_bwd", _stream(), _ptr(x), _ptr(y), s, n, k, ctx.lamb, _ptr(up), _ptr(gx), _ptr(gy))
        return gx, gy, None


def global_mi(x: Tensor, y: Tensor, lamb: float = 1.0):
    return _GlobalMI.apply(x, y, float(lamb))


class _GlobalMIPair(torch.autograd.Function):
    """IIDLoss for S sub-heads on prob[S, 2N, K] = [view 1 | view 2] along dim 1 (the layout the heads produce): the kernels read the
    two halves in place and write ONE gradient tensor -- no slice copies, no zero-filled halves added together by autograd."""

    @staticmethod
    def forward(ctx, prob: Tensor, lamb: float):
        _need_gpu(prob)
        prob = prob.contiguous().float()
        s, n2, k = prob.shape
        loss, loss_nl, joint = _global_outputs(s, k, prob.device)
        call("miseg_iic_global_fwd_pair", _stream(), _ptr(prob), s, n2 // 2, k, float(lamb), _ptr(loss), _ptr(loss_nl), _ptr(joint))
        ctx.save_for_backward(prob)
        ctx.lamb = float(lamb)
        ctx.mark_non_differentiable(loss_nl, joint)
        ctx.set_materialize_grads(False)      # (as in _GlobalMI)
        return loss, loss_nl, joint

    @staticmethod
    def backward(ctx, gloss, _g1, _g2):
        if gloss is None:
            return None, None
        prob, = ctx.saved_tensors
        s, n2, k = prob.shape
        gprob = torch.empty_like(prob)
        call("miseg_iic_global_bwd_pair", _stream(), _ptr(prob), s, n2 // 2, k, ctx.lamb, _ptr(gloss.contiguous().float()), _ptr(gprob))
        return gprob, None


def global_mi_pair(prob: Tensor, lamb: float = 1.0):
    """(loss[S], loss_no_lamb[S], joint[S,K,K]) of IIDLoss(prob[:, :N], prob[:, N:]) for prob[S, 2N, K]."""
    if prob.shape[1] % 2:
        raise _cabi.MisegError(f"global_mi_pair: prob holds {prob.shape[1]} rows per sub-head, expected an even number (two views)")
    return _GlobalMIPair.apply(prob, float(lamb))


class _GlobalJoint(torch.autograd.Function):
    """compute_joint (ref iic_loss.py:74-94) for S pairs at once: x, y [S,N,K] -> joint [S,K,K]."""

    @staticmethod
    def forward(ctx, x: Tensor, y: Tensor, symmetric: bool):
        _need_gpu(x, y)
        x, y = x.contiguous().float(), y.contiguous().float()
        s, n, k = x.shape
        joint = torch.empty(s, k, k, dtype=torch.float32, device=x.device)
        call("miseg_iic_global_joint_fwd", _stream(), _ptr(x), _ptr(y), s, n, k, int(bool(symmetric)), _ptr(joint))
        ctx.save_for_backward(x, y, joint)
        ctx.symmetric = bool(symmetric)
        return joint

    @staticmethod
    def backward(ctx, gjoint):
        x, y, joint = ctx.saved_tensors
        s, n, k = x.shape
        gx, gy = torch.empty_like(x), torch.empty_like(y)
        gjoint = gjoint.contiguous().float()
        call("miseg_iic_global_joint_bwd", _stream(), _ptr(x), _ptr(y), s, n, k, int(ctx.symmetric), _ptr(joint), _ptr(gjoint), _ptr(gx), _ptr(gy))
        return gx, gy, None


def global_joint(x: Tensor, y: Tensor, symmetric: bool = True) -> Tensor:
    return _GlobalJoint.apply(x, y, bool(symmetric))


# ------------------------------------------------------------------------------------------ local MI on the network output
def output_local_mi_supported(c: int, pad: int) -> bool:
    """Whether ``output_local_mi`` has a fused kernel for ``c`` classes and this padding (2 <= c <= 8, 0 <= pad <= 3)."""
    return int(_cabi.lib().miseg_iic_out_joint_ws_bytes(1, int(c), 1, 1, int(pad), 1)) >= 0


class _OutputLocalMI(torch.autograd.Function):
    """loss[P] of IIDSegmentationLoss over the P windows (ref contrastyou/losses/iic_loss.py:107-149, :152-189) on
    x = softmax(flip(b)), y = softmax(a), straight from the logits: the joint kernel computes both softmaxes in registers, the local-MI
    epilogue (``_local_loss``) turns the joint into the losses and d loss / d joint, the backward kernel goes from there to the logits
    of both sides.  Neither side is detached.

    Gradient hand-over (no add launch): when ``a`` is a part of a ``split_rows`` whose rows another loss kernel has already written --
    the consistency term, whose node is created after this one and therefore runs first in backward -- the kernel adds this term's
    gradient into those rows and the node returns no gradient for ``a``; ``b``'s gradient is written into its part's rows.  In any
    other order or layout the node returns fresh tensors and autograd adds as usual."""

    @staticmethod
    def forward(ctx, a: Tensor, b: Tensor, flips: Optional[Tensor], pad: int, windows, lamda: float):
        _need_gpu(a, b, flips)
        raw_a, raw_b = a, b
        a, b = logits_nhwc(a), logits_nhwc(b)
        if a.shape != b.shape:
            raise _cabi.MisegError(f"output_local_mi: logits {tuple(a.shape)} and {tuple(b.shape)} differ")
        n, c, h, w = a.shape
        if flips is not None and (flips.dtype != torch.int32 or flips.numel() < n):
            raise _cabi.MisegError("output_local_mi: flips must be int32 with one mask per sample")
        p, t, dev = len(windows), 2 * pad + 1, a.device
        win = windows_tensor(windows, dev)
        raw = torch.empty(p, t, t, c, c, dtype=torch.float32, device=dev)
        ws = _ws(query("miseg_iic_out_joint_ws_bytes", n, c, h, w, pad, p), dev)
        px = _pixels(windows)
        call("miseg_iic_out_joint_fwd", _stream(), _ptr(a), _ptr(b), _ptr(flips), n, c, h, w, pad, _ptr(win), p, _ptr(raw), _ptr(ws),
             ws.numel(), work=(2.0 * c * c * t * t * n * px, 2.0 * n * c * h * w * 4), tag=f"iic_out_joint_fwd[p{pad}]")
        loss = scalar_out((p,), dev)
        grad_raw = torch.empty_like(raw)
        _local_loss(raw, c, pad, p, lamda, loss, grad_raw)
        ctx.save_for_backward(a, b, flips, grad_raw, win)
        ctx.pad = pad
        ctx.parts = (_split_part_of(raw_a, a), _split_part_of(raw_b, b))
        ctx.set_materialize_grads(False)
        return loss

    @staticmethod
    def backward(ctx, gloss: Tensor):
        if gloss is None:
            return None, None, None, None, None, None
        a, b, flips, grad_raw, win = ctx.saved_tensors
        n, c, h, w = a.shape
        part_a, part_b = ctx.parts
        ga, gb, acc, ret_a, ret_b = None, None, 0, True, True
        if part_a is not None and part_a[1] in part_a[0].filled:
            cand = part_a[0].rows(part_a[1])
            if cand.shape == a.shape and cand.stride() == a.stride():
                ga, acc, ret_a = cand, 1, False              # += into the consistency gradient already there
        if ga is None:
            ga = empty_nhwc(n, c, h, w, torch.float32, a.device)
        if part_b is not None and part_b[1] not in part_b[0].filled:
            cand = part_b[0].rows(part_b[1])
            if cand.shape == b.shape and cand.stride() == b.stride():
                gb = cand
                part_b[0].filled.add(part_b[1])
        if gb is None:
            gb = empty_nhwc(n, c, h, w, torch.float32, b.device)
        t = 2 * ctx.pad + 1
        call("miseg_iic_out_bwd", _stream(), _ptr(a), _ptr(b), _ptr(flips), n, c, h, w, ctx.pad, _ptr(win), win.shape[0], _ptr(grad_raw),
             _ptr(gloss.contiguous().float()), _ptr(ga), _ptr(gb), acc,
             work=(4.0 * c * c * t * t * n * h * w, n * c * h * w * 4.0 * (4 + acc)), tag=f"iic_out_bwd[p{ctx.pad}]")
        return (ga if ret_a else None), (gb if ret_b else None), None, None, None, None


def output_local_mi(a: Tensor, b: Tensor, flips: Optional[Tensor], pad: int, windows, lamda: float = 1.0) -> Tensor:
    """loss[P] of ``IIDSegmentationSmallPathLoss(padding=pad)(softmax(flip(b)), softmax(a))`` per window (the reference averages them):
    a, b = [N, C, H, W] logits (fp32 NHWC read in place; others converted), ``flips`` the per-sample masks of ``b``'s flip
    (None: no flip), ``windows`` = [(h0, h1, w0, w1)] in the reference's patch order.  Only 2 <= C <= 8, 0 <= pad <= 3
    (``output_local_mi_supported``); the library refuses anything else."""
    return _OutputLocalMI.apply(a, b, flips, int(pad), _int_windows(windows), float(lamda))
