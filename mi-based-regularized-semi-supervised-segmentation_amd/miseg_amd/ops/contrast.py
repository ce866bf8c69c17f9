"""Contrastive pre-training (csrc/supcon.hip, contrast_decoder.hip, and the 3x3 convolutions of csrc/conv_*.hip for the decoder's
projection head): the supervised-contrastive loss, the pooled embedding and the layers of ``LocalProjectionHead``."""
from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor

from .. import _cabi
from .._cabi import query
from .._rt import _DT, _need_gpu, _ptr, _stream, _ws, as_nhwc, empty_nhwc
from ..stepio import scalar_out
from ..packcache import _pack
from ._pkg import call

_SUPCON_MAX_N, _SUPCON_MAX_D = 1024, 1024     # kSupMaxN / kSupMaxD of csrc/supcon.hip


def supcon_supported(n: int, d: int, views: int = 2) -> bool:
    """Whether ``supcon`` has a kernel for ``n`` = views x batch embedding rows of width ``d`` (the range of ``miseg_supcon``: at
    least two views of a non-empty batch, n <= 1024, d a multiple of 4 in 4..1024).  Pure host arithmetic."""
    n, d, views = int(n), int(d), int(views)
    return views >= 2 and n >= views and n % views == 0 and n <= _SUPCON_MAX_N and 4 <= d <= _SUPCON_MAX_D and d % 4 == 0


class _SupCon(torch.autograd.Function):
    @staticmethod
    def forward(ctx, e: Tensor, labels: Optional[Tensor], views: int, temperature: float, base_temperature: float):
        _need_gpu(e, labels)
        if e.dim() != 2:
            raise ValueError(f"supcon: embeddings must be [views * batch, dim], got {tuple(e.shape)}")
        e = e.contiguous().float()
        n, d = e.shape
        if labels is not None:
            labels = labels.contiguous().view(-1)
            if labels.dtype != torch.int32:
                labels = labels.to(torch.int32)
            if labels.numel() * views != n:
                raise ValueError("Num of labels does not match num of features")
        if not supcon_supported(n, d, views):
            raise _cabi.MisegError(f"miseg_supcon has no kernel for {n} rows of width {d} in {views} views (ops.supcon_supported)")
        dev = e.device
        loss = scalar_out((), dev)
        want_grad = ctx.needs_input_grad[0]
        ge = torch.empty_like(e) if want_grad else None
        ws = _ws(query("miseg_supcon_ws_bytes", n, d), dev)
        call("miseg_supcon", _stream(), _ptr(e), n, d, int(views), _ptr(labels), float(temperature), float(base_temperature), None,
             _ptr(loss), _ptr(ge), _ptr(ws), ws.numel())
        if want_grad:
            ctx.save_for_backward(ge)
        return loss

    @staticmethod
    def backward(ctx, g: Tensor):
        (ge,) = ctx.saved_tensors
        return ge * g, None, None, None, None


def supcon(e: Tensor, labels: Optional[Tensor] = None, views: int = 2, temperature: float = 0.07, base_temperature: float = 0.07) -> Tensor:
    """``SupConLoss(temperature, 'all', base_temperature)(stack(chunk(F.normalize(e, dim=1), views), 1), labels)`` from the RAW
    embeddings ``e`` [views * batch, dim] (view-major, as the projector returns them for ``cat([img, img_tf])``) in one library call
    that also leaves the gradient with respect to ``e``; ``labels`` int [batch], None = SimCLR.  Deterministic.  Shapes:
    ``supcon_supported``."""
    return _SupCon.apply(e, labels, int(views), float(temperature), float(base_temperature))


class _AvgPoolNHWC(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat: Tensor):
        _need_gpu(feat)
        feat = as_nhwc(feat)
        n, c, h, w = feat.shape
        pooled = torch.empty(n, c, dtype=torch.float32, device=feat.device)
        call("miseg_avgpool_fwd", _stream(), _DT[feat.dtype], _ptr(feat), n, h, w, c, _ptr(pooled))
        ctx.meta = (n, c, h, w, feat.dtype)
        return pooled

    @staticmethod
    def backward(ctx, g: Tensor):
        n, c, h, w, dtype = ctx.meta
        g = g.contiguous().float()
        gfeat = empty_nhwc(n, c, h, w, dtype, g.device)
        call("miseg_avgpool_bwd", _stream(), _DT[dtype], _ptr(g), n, h, w, c, _ptr(gfeat))
        return gfeat


def avgpool_nhwc(feature: Tensor) -> Tensor:
    """``Flatten()(nn.AdaptiveAvgPool2d((1, 1))(feature))`` on the network's channels_last feature map in its storage type (fp32,
    bf16, fp16) -> fp32 [N, C]; the backward broadcasts ``g / (H * W)`` into a feature gradient of the storage type."""
    return _AvgPoolNHWC.apply(feature)


# ------------------------------------------------------------------------------------------ LocalProjectionHead (contrastdecoder)
_CD_MAX_C = 1024          # kCdMaxC of csrc/contrast_decoder.hip


def conv3x3_bias_supported(cin: int, cout: int, dtype=torch.float32) -> bool:
    """Whether ``conv3x3_bias`` has kernels for a Conv2d(cin, cout, 3, 1, 1) on activations of ``dtype``: whole 16-byte channel
    vectors on both sides (the range of ``miseg_conv3x3_fwd`` / ``miseg_conv3x3_wgrad`` for a single full-resolution source)."""
    if dtype not in _DT:
        return False
    vec = 4 if dtype == torch.float32 else 8
    return int(cin) > 0 and int(cout) > 0 and int(cin) % vec == 0 and int(cout) % vec == 0


def bias_lrelu_supported(c: int) -> bool:
    """The channel range of ``miseg_bias_lrelu_fwd/bwd``: a multiple of 4, at most 1024."""
    return 0 < int(c) <= _CD_MAX_C and int(c) % 4 == 0


def bias_amaxpool_supported(n: int, c: int, h: int, w: int, output_size=(4, 4), partition_num=(1, 1), views: int = 1) -> bool:
    """The range of ``miseg_bias_amaxpool_fwd/bwd``.  Pure host arithmetic."""
    n, c, h, w, views = int(n), int(c), int(h), int(w), int(views)
    (oh, ow), (ph, pw) = (int(v) for v in output_size), (int(v) for v in partition_num)
    return (min(n, h, w, oh, ow, ph, pw, views) >= 1 and bias_lrelu_supported(c) and oh % ph == 0 and ow % pw == 0 and n % views == 0
            and h * w < 2 ** 31 and n * oh * ow < 2 ** 31)


class _Conv3x3Bias(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: Tensor, weight: Tensor):
        _need_gpu(x, weight)
        x = as_nhwc(x)
        n, cin, h, w = x.shape
        cout = weight.shape[0]
        if tuple(weight.shape[1:]) != (cin, 3, 3) or not conv3x3_bias_supported(cin, cout, x.dtype):
            raise _cabi.MisegError(f"conv3x3_bias has no kernel for a weight {tuple(weight.shape)} on {cin} channels of {x.dtype} "
                                   "(ops.conv3x3_bias_supported)")
        raw = empty_nhwc(n, cout, h, w, x.dtype, x.device)
        call("miseg_conv3x3_fwd", _stream(), _DT[x.dtype], _ptr(x), cin, 0, None, 0, 0, n, h, w, _ptr(_pack(weight, x.dtype, 0)), cout,
             _ptr(raw), None, work=(18.0 * cin * cout * n * h * w, float(x.element_size()) * n * h * w * (cin + cout)),
             tag=f"conv3x3_fwd[{h}x{w},{cin}->{cout}]")
        ctx.save_for_backward(x, weight)
        ctx.weight_ref = weight          # the Parameter object itself: the pack cache is keyed by it
        return raw

    @staticmethod
    def backward(ctx, graw: Tensor):
        x, weight = ctx.saved_tensors
        n, cin, h, w = x.shape
        cout, dtype, dev = weight.shape[0], x.dtype, x.device
        graw = as_nhwc(graw.to(dtype))
        gx = gw = None
        if ctx.needs_input_grad[1]:
            gw = torch.empty_like(weight)
            ws = _ws(query("miseg_conv3x3_wgrad_ws_bytes", n, h, w, cin, cout), dev)
            call("miseg_conv3x3_wgrad", _stream(), _DT[dtype], _ptr(x), cin, 0, None, 0, 0, n, h, w, _ptr(graw), cout, _ptr(gw), _ptr(ws), ws.numel(),
                 work=(18.0 * cin * cout * n * h * w, float(x.element_size()) * n * h * w * (cin + cout)), tag=f"conv3x3_wgrad[{h}x{w},{cin}->{cout}]")
        if ctx.needs_input_grad[0]:
            gx = empty_nhwc(n, cin, h, w, dtype, dev)
            call("miseg_conv3x3_fwd", _stream(), _DT[dtype], _ptr(graw), cout, 0, None, 0, 0, n, h, w, _ptr(_pack(ctx.weight_ref, dtype, 1, 0, cin)), cin,
                 _ptr(gx), None, work=(18.0 * cin * cout * n * h * w, float(x.element_size()) * n * h * w * (cin + cout)),
                 tag=f"conv3x3_dgrad[{h}x{w},{cout}->{cin}]")
        return gx, gw


def conv3x3_bias(x: Tensor, weight: Tensor) -> Tensor:
    """The convolution of a biased ``nn.Conv2d(cin, cout, 3, 1, 1)`` on a channels_last activation of fp32 / bf16 / fp16, WITHOUT its
    bias: the consumer (``bias_lrelu`` or ``bias_amaxpool``) adds it in the pass it makes anyway and owns its gradient.  Forward, data
    gradient (pack kind 1) and weight gradient are the MFMA kernels of csrc/conv_tiled.hip / conv_stream.hip / conv_wgrad.hip.  Shapes: ``conv3x3_bias_supported``."""
    return _Conv3x3Bias.apply(x, weight)


class _BiasLReLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, raw: Tensor, bias: Tensor, slope: float, inplace: bool):
        _need_gpu(raw, bias)
        raw = as_nhwc(raw)
        n, c, h, w = raw.shape
        if not bias_lrelu_supported(c) or bias.numel() != c:
            raise _cabi.MisegError(f"miseg_bias_lrelu_fwd has no kernel for {c} channels and a bias of {bias.numel()} (ops.bias_lrelu_supported)")
        bias = bias.contiguous().float()
        y = raw if inplace else torch.empty_like(raw)
        call("miseg_bias_lrelu_fwd", _stream(), _DT[raw.dtype], _ptr(raw), n, h, w, c, _ptr(bias), float(slope), _ptr(y),
             work=(0.0, 2.0 * raw.element_size() * raw.numel()), tag=f"bias_lrelu_fwd[{h}x{w},{c}]")
        if inplace:
            ctx.mark_dirty(raw)
        ctx.save_for_backward(y)
        ctx.slope = float(slope)
        return y

    @staticmethod
    def backward(ctx, gy: Tensor):
        (y,) = ctx.saved_tensors
        n, c, h, w = y.shape
        gy = as_nhwc(gy.to(y.dtype))
        gx = torch.empty_like(y) if ctx.needs_input_grad[0] else None
        gbias = torch.empty(c, dtype=torch.float32, device=y.device)
        ws = _ws(query("miseg_bias_lrelu_bwd_ws_bytes", _DT[y.dtype], n, h, w, c), y.device)
        call("miseg_bias_lrelu_bwd", _stream(), _DT[y.dtype], _ptr(y), _ptr(gy), n, h, w, c, ctx.slope, _ptr(gx), _ptr(gbias), _ptr(ws), ws.numel(),
             work=(0.0, 3.0 * y.element_size() * y.numel()), tag=f"bias_lrelu_bwd[{h}x{w},{c}]")
        return gx, gbias, None, None


def bias_lrelu(raw: Tensor, bias: Tensor, slope: float = 0.01, inplace: bool = False) -> Tensor:
    """``F.leaky_relu(raw + bias[None, :, None, None], slope)`` on a channels_last activation in its storage type (fp32 add and
    multiply, one rounding to the storage type); ``inplace`` overwrites ``raw``.  The backward reads the RESULT, as torch's in-place
    ``leaky_relu`` does, and returns the bias gradient as a fixed-order fp32 sum.  ``slope=1`` is the bare bias add."""
    return _BiasLReLU.apply(raw, bias, float(slope), bool(inplace))


class _BiasAMaxPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, raw: Tensor, bias: Optional[Tensor], oh: int, ow: int, ph: int, pw: int, views: int):
        _need_gpu(raw, bias)
        raw = as_nhwc(raw)
        n, c, h, w = raw.shape
        if not bias_amaxpool_supported(n, c, h, w, (oh, ow), (ph, pw), views) or (bias is not None and bias.numel() != c):
            raise _cabi.MisegError(f"miseg_bias_amaxpool_fwd has no kernel for {tuple(raw.shape)} -> ({oh}, {ow}) in ({ph}, {pw}) blocks of "
                                   f"{views} views (ops.bias_amaxpool_supported)")
        if bias is not None:
            bias = bias.contiguous().float()
        e = torch.empty(n * ph * pw, c * (oh // ph) * (ow // pw), dtype=torch.float32, device=raw.device)
        idx = torch.empty(n, oh, ow, c, dtype=torch.int32, device=raw.device)
        call("miseg_bias_amaxpool_fwd", _stream(), _DT[raw.dtype], _ptr(raw), n, h, w, c, _ptr(bias), oh, ow, ph, pw, views, _ptr(e), _ptr(idx),
             work=(0.0, float(raw.element_size()) * raw.numel()), tag=f"bias_amaxpool_fwd[{h}x{w},{c}]")
        ctx.save_for_backward(idx)
        ctx.meta = (n, c, h, w, oh, ow, ph, pw, views, raw.dtype, bias is not None)
        ctx.mark_non_differentiable(idx)
        return e, idx

    @staticmethod
    def backward(ctx, ge: Tensor, _gidx):
        (idx,) = ctx.saved_tensors
        n, c, h, w, oh, ow, ph, pw, views, dtype, has_bias = ctx.meta
        ge = ge.contiguous().float()
        graw = empty_nhwc(n, c, h, w, dtype, ge.device)
        gbias = torch.empty(c, dtype=torch.float32, device=ge.device) if has_bias and ctx.needs_input_grad[1] else None
        call("miseg_bias_amaxpool_bwd", _stream(), _DT[dtype], _ptr(ge), _ptr(idx), n, h, w, c, oh, ow, ph, pw, views, _ptr(graw), _ptr(gbias),
             work=(0.0, float(graw.element_size()) * graw.numel()), tag=f"bias_amaxpool_bwd[{h}x{w},{c}]")
        return graw, gbias, None, None, None, None, None


def bias_amaxpool(raw: Tensor, bias: Optional[Tensor], output_size=(4, 4), partition_num=(1, 1), views: int = 1, return_indices: bool = False):
    """``F.adaptive_max_pool2d(raw, output_size) + bias[None, :, None, None]`` on a channels_last activation in its storage type,
    returned as the fp32 rows ``cat_v(unfold_position(chunk_v, partition_num)[0].view(rows, -1))`` the contrastive loss reads
    ([N * PH * PW, C * OH/PH * OW/PW]; ``partition_num=(1, 1), views=1`` is ``[N, C * OH * OW]``, the contiguous NCHW result).  Ties
    take the first maximum in row-major order, a NaN wins.  The backward writes the whole gradient of ``raw`` (overlapping windows
    add in window order) and the bias gradient.  Shapes: ``bias_amaxpool_supported``."""
    (oh, ow), (ph, pw) = (int(v) for v in output_size), (int(v) for v in partition_num)
    e, idx = _BiasAMaxPool.apply(raw, bias, oh, ow, ph, pw, int(views))
    return (e, idx) if return_indices else e
