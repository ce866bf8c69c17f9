"""Cluster heads (csrc/heads_local.hip, heads_global.hip, heads_var.hip): S sub-heads of 1x1 convolution / Linear + softmax in one
launch, with the fused sample gather and flip replay; the ``_var`` heads are the mlp / normalize variants."""
from __future__ import annotations

import os
from typing import Optional

import torch
from torch import Tensor

from .._cabi import query
from .._rt import _DT, _GradJoin, _need_gpu, _ptr, _stream, _ws, as_nhwc, empty_nhwc, fill_zero, zeros_nhwc
from ..gradslot import stacked_grad_slot
from ..stepio import zero_counter
from ._pkg import call


def _stacked_grad(params, shape, device) -> Tensor:
    """Gradient buffer for a stacked [S, ...] head parameter: the flat-gradient slots themselves when the S parameters
    sit back to back there (gradslot.register_adjacent), else a fresh tensor."""
    slot = stacked_grad_slot(params) if params else None
    return slot.view(shape) if slot is not None else torch.empty(shape, dtype=torch.float32, device=device)


def _capture_params(ctx, *params) -> tuple:
    """The stacked head parameters as contiguous fp32; ``ctx.stacks`` keeps the module parameters each is a view of (``_param_grads``)."""
    ctx.stacks = tuple(getattr(t, "_miseg_stack_params", None) for t in params)
    return tuple(t.contiguous().float() for t in params)


def _param_grads(ctx, device, *shapes) -> tuple:
    """One gradient buffer per captured parameter, in their order (None where the shape is None: an absent second layer)."""
    return tuple(None if shape is None else _stacked_grad(stack, shape, device) for stack, shape in zip(ctx.stacks, shapes))


_HEAD_RECOMPUTE = os.environ.get("MISEG_HEAD_RECOMPUTE", "1") != "0"   # 0: the head backward reads the saved probabilities


class _LocalHead(torch.autograd.Function):
    """S x (1x1 conv + channel softmax) with fused sample gather + flip replay -> prob [S,M,K,H,W]."""

    @staticmethod
    def forward(ctx, feat: Tensor, w: Tensor, b: Tensor, src: Tensor, flips: Optional[Tensor], temperature: float):
        _need_gpu(feat, w, b, src, flips)
        feat = as_nhwc(feat)
        bsz, c, h, wd = feat.shape
        s, k, _ = w.shape
        m = src.numel()
        w, b = _capture_params(ctx, w, b)
        prob = torch.empty(s, m, k, h, wd, dtype=torch.float32, device=feat.device)
        viol = zero_counter(feat.device) if k <= 32 else None
        _LocalHead.last_violations = viol
        ctx.sink = getattr(feat, "_miseg_grad_sink", None)
        call("miseg_head_local_fwd", _stream(), _DT[feat.dtype], _ptr(feat), bsz, h, wd, c, _ptr(src), _ptr(flips), m, _ptr(w), _ptr(b),
             s, k, float(temperature), _ptr(prob), 2e-4, _ptr(viol), work=(2.0 * s * k * c * m * h * wd, (s * k * 4.0 + c * feat.element_size()) * m * h * wd),
             tag=f"head_local_fwd[c{c}]")
        # the shipped top tap: the backward computes the probabilities again from the features (bit-equal), so the node does not hold on
        # to them -- with the local-MI node keeping operand planes instead (see mi._LocalMIHeads) the fp32 tensor dies after the joint forward
        ctx.recompute = bool(_HEAD_RECOMPUTE and not _GradJoin.enabled and
                             query("miseg_head_local_bwd_recompute_supported", _DT[feat.dtype], c, s, k))
        ctx.save_for_backward(feat, w, src, flips, feat.new_empty(0) if ctx.recompute else prob, b)
        ctx.temperature = float(temperature)
        ctx.src_range = getattr(src, "_miseg_range", None)
        return prob

    @staticmethod
    def backward(ctx, gprob: Tensor):
        feat, w, src, flips, prob, b = ctx.saved_tensors
        bsz, c, h, wd = feat.shape
        s, k, _ = w.shape
        m = src.numel()
        gprob = gprob.contiguous().float()
        gfeat = None
        joined = None
        if ctx.needs_input_grad[0] and query("miseg_head_local_bwd_acc_supported", _DT[feat.dtype], c, s, k) and \
                (not _GradJoin.only or _GradJoin.only == str(c)):
            joined = _GradJoin.take(feat)
        if joined is not None:
            # the other consumer of this feature already wrote its input gradient: add ours to it in the kernel epilogue
            gsum, written, writer = joined
            cur = torch.cuda.current_stream(feat.device)
            cur.wait_event(written)
            gsum.record_stream(cur)
            gw, gb = _param_grads(ctx, feat.device, w.shape, (s, k))
            ws = _ws(query("miseg_head_local_bwd_ws_bytes", m, h, wd, c, s, k), feat.device)
            call("miseg_head_local_bwd_acc", _stream(), _DT[feat.dtype], _ptr(feat), bsz, h, wd, c, _ptr(src), _ptr(flips), m, _ptr(w), s, k,
                 ctx.temperature, _ptr(prob), _ptr(gprob), _ptr(gsum), _ptr(gw), _ptr(gb), _ptr(ws), ws.numel(),
                 work=(4.0 * s * k * c * m * h * wd, (3 * s * k * 4.0 + 3 * c * feat.element_size()) * m * h * wd), tag=f"head_local_bwd[c{c}]")
            if writer != cur:
                done = torch.cuda.Event()
                done.record(cur)
                writer.wait_event(done)       # whoever reads the joined gradient next does so on the writer's stream
            return None, gw, gb, None, None, None
        sink = ctx.sink if not _GradJoin.enabled else None
        compact, n0, n1 = False, 0, bsz
        if ctx.needs_input_grad[0]:
            rng = ctx.src_range
            if rng is not None and feat.dtype in (torch.bfloat16, torch.float16) and k == 20 and s == 5 and c in (16, 32) and 0 <= rng[0] <= rng[1] <= bsz:
                # the shipped kernels store (not accumulate) every pixel and channel of the rows in src = [start, stop) and touch no other
                if sink is not None and rng[0] < rng[1]:
                    # ... so a COMPACT gradient of those rows is all there is: the producing layer's BatchNorm backward adds it in its
                    # loaders (unet_ops._GradSink) -- no zero fill of the other rows, no add kernel over the whole batch
                    n0, n1 = rng
                    gfeat = torch.empty((n1 - n0, c, h, wd), dtype=feat.dtype, device=feat.device, memory_format=torch.channels_last)
                    compact = True
                else:
                    gfeat = torch.empty((bsz, c, h, wd), dtype=feat.dtype, device=feat.device, memory_format=torch.channels_last)
                    if rng[0] > 0:
                        fill_zero(gfeat[:rng[0]])
                    if rng[1] < bsz:
                        fill_zero(gfeat[rng[1]:])
            else:
                gfeat = fill_zero(empty_nhwc(bsz, c, h, wd, feat.dtype, feat.device))
        gw, gb = _param_grads(ctx, feat.device, w.shape, (s, k))
        ws = _ws(query("miseg_head_local_bwd_ws_bytes", m, h, wd, c, s, k), feat.device)
        work = (4.0 * s * k * c * m * h * wd, (3 * s * k * 4.0 + 2 * c * feat.element_size()) * m * h * wd)
        if ctx.recompute:
            # the kernel computes the probabilities again from the features (bit-equal to the forward's): it reads gprob only
            call("miseg_head_local_bwd_recompute", _stream(), _DT[feat.dtype], _ptr(feat), bsz, h, wd, c, _ptr(src), _ptr(flips), m, _ptr(w),
                 _ptr(b), s, k, ctx.temperature, _ptr(gprob), _ptr(gfeat), n0, _ptr(gw), _ptr(gb), _ptr(ws), ws.numel(),
                 work=(work[0] + 2.0 * s * k * c * m * h * wd, work[1] - s * k * 4.0 * m * h * wd), tag=f"head_local_bwd[c{c}]")
        elif compact:
            call("miseg_head_local_bwd_rows", _stream(), _DT[feat.dtype], _ptr(feat), bsz, h, wd, c, _ptr(src), _ptr(flips), m, _ptr(w), s, k,
                 ctx.temperature, _ptr(prob), _ptr(gprob), _ptr(gfeat), n0, _ptr(gw), _ptr(gb), _ptr(ws), ws.numel(), work=work,
                 tag=f"head_local_bwd[c{c}]")
        else:
            call("miseg_head_local_bwd", _stream(), _DT[feat.dtype], _ptr(feat), bsz, h, wd, c, _ptr(src), _ptr(flips), m, _ptr(w), s, k,
                 ctx.temperature, _ptr(prob), _ptr(gprob), _ptr(gfeat), _ptr(gw), _ptr(gb), _ptr(ws), ws.numel(), work=work,
                 tag=f"head_local_bwd[c{c}]")
        if gfeat is not None and sink is not None:
            sink.put(gfeat, n0, n1)          # handed to the producing layer's backward; autograd gets no gradient from this edge
            return None, gw, gb, None, None, None
        if gfeat is not None:
            _GradJoin.offer(feat, gfeat)     # a later consumer of the same feature (e.g. up_conv's pooled data gradient) may add into it
        return gfeat, gw, gb, None, None, None


def local_head(feat: Tensor, w: Tensor, b: Tensor, src: Tensor, flips: Optional[Tensor], temperature: float = 1.0) -> Tensor:
    """prob[S, M, K, H, W].  The kernel also counts the positions whose K probabilities do not sum to one; the count rides
    on the result (``_miseg_simplex`` = (axis, device counter, tensor version)) so that a later ``checks.assert_simplex`` of
    this very tensor costs nothing."""
    _LocalHead.last_violations = None
    prob = _LocalHead.apply(feat, w, b, src, flips, float(temperature))
    if _LocalHead.last_violations is not None:
        prob._miseg_simplex = (2, _LocalHead.last_violations, prob._version)
        _LocalHead.last_violations = None
    return prob


class _GlobalHead(torch.autograd.Function):
    """S x (global avg pool -> Linear -> softmax) -> prob [S,M,K]."""

    @staticmethod
    def forward(ctx, feat: Tensor, w: Tensor, b: Tensor, src: Tensor, temperature: float):
        _need_gpu(feat, w, b, src)
        feat = as_nhwc(feat)
        bsz, c, h, wd = feat.shape
        s, k, _ = w.shape
        m = src.numel()
        w, b = _capture_params(ctx, w, b)
        pooled = torch.empty(m, c, dtype=torch.float32, device=feat.device)
        prob = torch.empty(s, m, k, dtype=torch.float32, device=feat.device)
        call("miseg_head_global_fwd", _stream(), _DT[feat.dtype], _ptr(feat), bsz, h, wd, c, _ptr(src), m, _ptr(w), _ptr(b), s, k,
             float(temperature), _ptr(pooled), _ptr(prob))
        ctx.save_for_backward(w, src, pooled, prob)
        ctx.meta = (bsz, c, h, wd, feat.dtype, float(temperature))
        ctx.sink = getattr(feat, "_miseg_grad_sink", None)
        ctx.src_range = getattr(src, "_miseg_range", None)
        return prob

    @staticmethod
    def backward(ctx, gprob: Tensor):
        w, src, pooled, prob = ctx.saved_tensors
        bsz, c, h, wd, dtype, temperature = ctx.meta
        s, k, _ = w.shape
        m = src.numel()
        gprob = gprob.contiguous().float()
        gfeat, compact, n0, n1 = None, False, 0, bsz
        sink, rng = ctx.sink, ctx.src_range
        if ctx.needs_input_grad[0]:
            if sink is not None and rng is not None and 0 <= rng[0] < rng[1] <= bsz and rng[1] - rng[0] == m:
                # the kernel writes every element of the rows in src = [start, stop) and nothing else: a compact gradient (_LocalHead)
                n0, n1 = rng
                gfeat = empty_nhwc(n1 - n0, c, h, wd, dtype, w.device)
                compact = True
            else:
                gfeat = fill_zero(empty_nhwc(bsz, c, h, wd, dtype, w.device))
        gw, gb = _param_grads(ctx, w.device, w.shape, (s, k))
        dz = torch.empty(s * m * k, dtype=torch.float32, device=w.device)
        if compact:
            call("miseg_head_global_bwd_rows", _stream(), _DT[dtype], bsz, h, wd, c, _ptr(src), m, _ptr(w), s, k, temperature, _ptr(pooled),
                 _ptr(prob), _ptr(gprob), _ptr(gfeat), n0, _ptr(gw), _ptr(gb), _ptr(dz))
        else:
            call("miseg_head_global_bwd", _stream(), _DT[dtype], bsz, h, wd, c, _ptr(src), m, _ptr(w), s, k, temperature, _ptr(pooled),
                 _ptr(prob), _ptr(gprob), _ptr(gfeat), _ptr(gw), _ptr(gb), _ptr(dz))
        if gfeat is not None and sink is not None:
            sink.put(gfeat, n0, n1)
            return None, gw, gb, None, None
        return gfeat, gw, gb, None, None


def global_head(feat: Tensor, w: Tensor, b: Tensor, src: Tensor, temperature: float = 1.0) -> Tensor:
    return _GlobalHead.apply(feat, w, b, src, float(temperature))


# ------------------------------------------------------------------------------------------ head variants (mlp / normalize)
def _var_layers(feat: Tensor, w1: Tensor, w2: Optional[Tensor], b2: Optional[Tensor]):
    """(hid, w2, b2) as the ``_var`` nodes take them: ``hid`` = the hidden width, 0 for the single-layer head (``w2 is None``), whose
    second layer travels as two empty dummies."""
    if w2 is None:
        w2 = b2 = torch.empty(0, device=feat.device)
        return 0, w2, b2
    return int(w1.shape[1]), w2, b2


def _capture_var_params(ctx, w1, b1, w2, b2, hid: int) -> tuple:
    w1, b1, w2, b2 = _capture_params(ctx, w1, b1, w2, b2)
    return (w1, b1, w2, b2) if hid else (w1, b1, None, None)      # (the dummies of a single-layer head)


def _var_param_grads(ctx, device, w1, b1, w2, b2, hid: int) -> tuple:
    return _param_grads(ctx, device, w1.shape, b1.shape, w2.shape if hid else None, b2.shape if hid else None)


class _LocalHeadVar(torch.autograd.Function):
    """LocalClusterHead with head_type='mlp' and/or normalize=True (csrc/heads_var.hip) -> prob [S,M,K,H,W].
    hid == 0: single layer (w1 [S,K,C], b1 [S,K]; w2, b2 are dummies).  The backward recomputes the forward from the features."""

    @staticmethod
    def forward(ctx, feat, w1, b1, w2, b2, src, flips, temperature: float, normalize: bool, hid: int):
        _need_gpu(feat, w1, b1, src, flips)
        feat = as_nhwc(feat)
        bsz, c, h, wd = feat.shape
        s = w1.shape[0]
        k = (w2 if hid else w1).shape[1]
        m = src.numel()
        w1, b1, w2, b2 = _capture_var_params(ctx, w1, b1, w2, b2, hid)
        prob = torch.empty(s, m, k, h, wd, dtype=torch.float32, device=feat.device)
        call("miseg_head_local_var_fwd", _stream(), _DT[feat.dtype], _ptr(feat), bsz, h, wd, c, _ptr(src), _ptr(flips), m, _ptr(w1), _ptr(b1),
             hid, _ptr(w2), _ptr(b2), s, k, float(temperature), int(bool(normalize)), _ptr(prob))
        ctx.save_for_backward(feat, w1, b1, w2, b2, src, flips)
        ctx.cfg = (float(temperature), bool(normalize), int(hid), k)
        return prob

    @staticmethod
    def backward(ctx, gprob):
        feat, w1, b1, w2, b2, src, flips = ctx.saved_tensors
        temperature, normalize, hid, k = ctx.cfg
        bsz, c, h, wd = feat.shape
        s, m, dev = w1.shape[0], src.numel(), feat.device
        gprob = gprob.contiguous().float()
        gfeat = zeros_nhwc(bsz, c, h, wd, feat.dtype, dev) if ctx.needs_input_grad[0] else None
        gw1, gb1, gw2, gb2 = _var_param_grads(ctx, dev, w1, b1, w2, b2, hid)
        ws = _ws(query("miseg_head_local_var_bwd_ws_bytes", m, h, wd, c, hid, s, k), dev)
        call("miseg_head_local_var_bwd", _stream(), _DT[feat.dtype], _ptr(feat), bsz, h, wd, c, _ptr(src), _ptr(flips), m, _ptr(w1), _ptr(b1),
             hid, _ptr(w2), _ptr(b2), s, k, temperature, int(normalize), _ptr(gprob), _ptr(gfeat), _ptr(gw1), _ptr(gb1), _ptr(gw2), _ptr(gb2),
             _ptr(ws), ws.numel())
        return gfeat, gw1, gb1, gw2, gb2, None, None, None, None, None


def local_head_var(feat, w1, b1, w2, b2, src, flips, temperature=1.0, normalize=False) -> Tensor:
    """w2 is None for the single-layer head.  w1 [S,R,C] (R = hidden width or K), w2 [S,K,HID]."""
    hid, w2, b2 = _var_layers(feat, w1, w2, b2)
    return _LocalHeadVar.apply(feat, w1, b1, w2, b2, src, flips, float(temperature), bool(normalize), hid)


class _GlobalHeadVar(torch.autograd.Function):
    """ClusterHead with head_type='mlp' and/or normalize=True -> prob [S,M,K]."""

    @staticmethod
    def forward(ctx, feat, w1, b1, w2, b2, src, temperature: float, normalize: bool, hid: int):
        _need_gpu(feat, w1, b1, src)
        feat = as_nhwc(feat)
        bsz, c, h, wd = feat.shape
        s = w1.shape[0]
        k = (w2 if hid else w1).shape[1]
        m = src.numel()
        w1, b1, w2, b2 = _capture_var_params(ctx, w1, b1, w2, b2, hid)
        pooled = torch.empty(m, c, dtype=torch.float32, device=feat.device)
        prob = torch.empty(s, m, k, dtype=torch.float32, device=feat.device)
        call("miseg_head_global_var_fwd", _stream(), _DT[feat.dtype], _ptr(feat), bsz, h, wd, c, _ptr(src), m, _ptr(w1), _ptr(b1), hid, _ptr(w2),
             _ptr(b2), s, k, float(temperature), int(bool(normalize)), _ptr(pooled), _ptr(prob))
        ctx.save_for_backward(w1, b1, w2, b2, src, pooled)
        ctx.cfg = (float(temperature), bool(normalize), int(hid), k, bsz, c, h, wd, feat.dtype)
        return prob

    @staticmethod
    def backward(ctx, gprob):
        w1, b1, w2, b2, src, pooled = ctx.saved_tensors
        temperature, normalize, hid, k, bsz, c, h, wd, dtype = ctx.cfg
        s, m, dev = w1.shape[0], src.numel(), w1.device
        gprob = gprob.contiguous().float()
        gfeat = zeros_nhwc(bsz, c, h, wd, dtype, dev) if ctx.needs_input_grad[0] else None
        gw1, gb1, gw2, gb2 = _var_param_grads(ctx, dev, w1, b1, w2, b2, hid)
        dpool = torch.empty(s * m * c, dtype=torch.float32, device=dev)
        call("miseg_head_global_var_bwd", _stream(), _DT[dtype], bsz, h, wd, c, _ptr(src), m, _ptr(w1), _ptr(b1), hid, _ptr(w2), _ptr(b2), s, k,
             temperature, int(normalize), _ptr(pooled), _ptr(gprob), _ptr(gfeat), _ptr(gw1), _ptr(gb1), _ptr(gw2), _ptr(gb2), _ptr(dpool))
        return gfeat, gw1, gb1, gw2, gb2, None, None, None, None


def global_head_var(feat, w1, b1, w2, b2, src, temperature=1.0, normalize=False) -> Tensor:
    hid, w2, b2 = _var_layers(feat, w1, w2, b2)
    return _GlobalHeadVar.apply(feat, w1, b1, w2, b2, src, float(temperature), bool(normalize), hid)
