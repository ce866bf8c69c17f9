"""Autograd front-ends of the U-Net kernels: conv3x3 + BatchNorm(train/eval) + ReLU (+ fused 2x2
max-pool, + fused nearest-x2 upsample / skip concat on the input side) and the 1x1 logits head.

ref: contrastyou/arch/unet.py:10-40 (conv_block / up_conv), :61-64 (pools), :84,129 (DeConv_1x1),
:109-125 (torch.cat skips).  Activations are [N,C,H,W]-shaped torch tensors in channels_last memory
(= the NHWC layout of the kernels) of dtype float32 (exact mode) or bfloat16.
"""
from __future__ import annotations

import contextlib
import os

from typing import Optional, Tuple

import torch
from torch import Tensor

from . import _cabi, stepio
from ._cabi import call, query
from ._rt import _DT, _GradJoin, _need_gpu, _ptr, _stream, _ws, as_nhwc, empty_nhwc, wait_stream
from .gradslot import grad_slot
from .packcache import _pack, _pack_now
from .tape import keep

BN_EPS, BN_MOMENTUM = 1e-5, 0.1

# ---- switches (DESIGN.md, appendix "environment switches", and section 26 for the paths they select).  Module attributes, read when
# a layer runs: tests patch them.  SYNC_COUNTERS.enabled (MISEG_BN_FINISH, below) and _rt._GradJoin.enabled are the other two.
_WGRAD_SIDE = os.environ.get("MISEG_WGRAD_STREAM", "1") != "0"       # weight gradients on a side stream (_wgrad_fork); 0: the main stream
_GRAPH_STREAMS = os.environ.get("MISEG_GRAPH_STREAMS", "1") == "1"   # fork side streams inside a captured step too (side_streams_allowed)
_STEM_KERNELS = os.environ.get("MISEG_STEM_KERNELS", "1") != "0"     # the stem through its own kernels (_forward_plan); 0: the MFMA path
_STEM_DGRAD = os.environ.get("MISEG_STEM_DGRAD", "1") != "0"         # the image gradient through miseg_conv3x3_stem_dgrad; 0: the generic path
_BN_ACC = os.environ.get("MISEG_BN_ACC", "1") != "0"                 # forward statistics as fixed-point accumulators; 0: partial rows + finalize
_BN_ACC_BWD = os.environ.get("MISEG_BN_ACC_BWD", "0") == "1"         # the same for the backward's sums (measured slower: OFF)
_FUSE_UPS_DGRAD = True   # False: conv3x3 dgrad + miseg_sumpool2x2 as two launches
_DUAL_DGRAD = True       # concat layers: one data-gradient launch with two destinations (False: one launch per source)
_FUSE_BN_BWD = os.environ.get("MISEG_BN_FUSE", "0") == "1"           # BatchNorm backward folded into the convolutions (_backward_fused; measured slower: OFF)
# The statistics pass ALONE in the producing data-gradient kernel's epilogue (no loader transform): MISEG_BN_RED=1 (round-4 experiment)
_RED_ONLY = os.environ.get("MISEG_BN_RED", "0") == "1" and not _FUSE_BN_BWD
_STEM_MAX_W = 1022                  # the stem kernels keep whole image rows (+ halo) in 4 x 256 registers


def side_streams_allowed() -> bool:
    """May this code fork a side stream now?  Under hipGraph capture the fork/join (wait_stream both ways) is captured as graph
    dependencies; ``MISEG_GRAPH_STREAMS=0`` keeps a captured step on one stream."""
    return _GRAPH_STREAMS or not torch.cuda.is_current_stream_capturing()


def _epilogue_sums_allowed() -> bool:
    """May a data-gradient epilogue take the source layer's BatchNorm-backward sums?  With the folded backward (which includes the
    statistics pass in the producing data-gradient kernel's epilogue) or with that pass alone (``_RED_ONLY``)."""
    return _FUSE_BN_BWD or _RED_ONLY


# ---- weight gradients off the critical path
# In the U-Net backward only BN-backward -> dgrad feeds the next layer; a layer's wgrad (+ its split reduction) has no consumer
# before the optimiser.  It is launched on a side stream so the dgrad chain does not queue behind it and the two fill each
# other's tails.  Joined before anything reads the flat gradient buffer (FlatBuffers.collect, GradReducer._launch).
_wgrad_streams: dict = {}
_wgrad_dirty: set = set()


def wgrad_stream(device):
    st = _wgrad_streams.get(device)
    if st is None:
        st = _wgrad_streams[device] = torch.cuda.Stream(device=device)
    return st


def join_wgrad_streams() -> None:
    """Make the current stream wait for every outstanding side-stream wgrad.  Called with the weight-gradient stream itself current (the
    data-parallel reducer launches its collectives from it) there is nothing to wait for and the device stays marked: the backward
    pass's own stream still has to join when the pass ends."""
    for dev in list(_wgrad_dirty):
        cur = torch.cuda.current_stream(dev)
        if cur != _wgrad_streams[dev]:
            wait_stream(cur, _wgrad_streams[dev])
            _wgrad_dirty.discard(dev)


class _BnRec:
    """What a layer's CONSUMER needs to take the layer's BatchNorm-backward sums in the epilogue of its data-gradient kernel, and
    the hand-over of those sums.  Hangs off the activation tensor (``y._miseg_bn``); the consumer's backward fills ``parts`` and
    names the gradient tensor they belong to, the layer's backward uses them only if autograd hands it that very tensor, unmodified
    (another consumer of the activation -> autograd added the gradients into a new tensor -> the ordinary reduce runs)."""
    __slots__ = ("raw", "saved", "shape", "parts", "nparts", "for_grad", "for_version")

    def __init__(self):
        self.raw = self.saved = self.shape = self.parts = self.for_grad = None
        self.nparts = self.for_version = 0

    def offer(self, grad: Tensor, parts: Tensor, nparts: int) -> None:
        self.parts, self.nparts, self.for_grad, self.for_version = parts, nparts, grad, grad._version

    def take(self, grad: Optional[Tensor]):
        parts, nparts, mine = self.parts, self.nparts, self.for_grad is grad and grad is not None and grad._version == self.for_version
        self.parts = self.for_grad = None
        return (parts, nparts) if mine and parts is not None else (None, 0)


class _GradSink:
    """Side channel for a SECOND gradient of a layer's activation.  A tapped feature map feeds the next layer and a cluster head (ref
    semi_seg/epocher.py:258-273, the head sees the last 2 UB samples); autograd would add the two gradients with an elementwise kernel
    over the whole batch, behind a zero fill of the samples the head does not touch.  Instead the head's backward ``put``s its compact
    gradient (samples [n0, n1) only) here and returns no gradient; this layer's backward -- which autograd runs after every consumer
    of the activation, whatever they return -- ``take``s it and the BatchNorm-backward kernels add it in their loaders
    (``miseg_bn_relu_bwd_dual``)."""
    __slots__ = ("items",)

    def __init__(self):
        self.items = []

    def put(self, grad: Tensor, n0: int, n1: int) -> None:
        self.items.append((grad, int(n0), int(n1), torch.cuda.current_stream(grad.device)))

    def take(self):
        items, self.items = self.items, []
        return items


class _SyncCounters:
    """int32 counters for the "last block finishes" launches (miseg_conv3x3_bn_fwd, miseg_bn_relu_bwd_sync): zero when a launch
    starts, zero again when it ends.  One zero-filled array per device, handed out round-robin, so that launches which could overlap
    (different streams) never share a counter.
    OFF by default (``MISEG_BN_FINISH=1`` turns it on): it removes 44 of the step's ~300 launches, but the finishing block's serial
    tail (ticket atomic -> cache invalidate -> dependent loads of the partial rows from memory -> coefficients) costs more than the
    5 us finalize kernel plus its launch gap did: 8.54 ms/step (rows written through, no release fence) and 8.83 ms (release fence
    per block) against 8.03-8.10 ms with the separate finalize launches, same box, same run."""
    SLOTS = 256

    def __init__(self):
        self._pool, self._next = {}, 0
        self.enabled = os.environ.get("MISEG_BN_FINISH", "0") == "1"

    def take(self, device) -> Optional[Tensor]:
        if not self.enabled:
            return None
        pool = self._pool.get(device)
        if pool is None:
            pool = self._pool[device] = torch.zeros(self.SLOTS, dtype=torch.int32, device=device)
        self._next = (self._next + 1) % self.SLOTS
        return pool[self._next:self._next + 1]


SYNC_COUNTERS = _SyncCounters()


def loss_scale_of(model) -> float:
    """INITIAL loss scale of a model: 1 unless its activations are stored as IEEE half, whose range (6e-8 .. 65504) does not hold the
    per-pixel gradients of a mean over 48 x 256 x 256 positions (~3e-7).  ``MISEG_LOSS_SCALE`` overrides the default 2^14; the
    fused Adam divides it back out (``miseg_adam_step_scaled``), so the update equals the unscaled one up to rounding.  From there the
    scale is dynamic (``flat.LossScaler``: halved when the flat gradient holds an inf / NaN, that step skipped on the device)."""
    net = getattr(model, "module", model)
    if getattr(net, "compute_dtype", None) != torch.float16:
        return 1.0
    return float(os.environ.get("MISEG_LOSS_SCALE", 16384.0))


def vec_of(dtype) -> int:
    return 8 if dtype in (torch.bfloat16, torch.float16) else 4


# ---- gradients with respect to the input image, and forward passes that leave the running statistics alone (virtual adversarial
# training; saliency maps and adversarial evaluation need the first too)
# _STEM_DGRAD: the stem's data gradient through its own pixel-per-thread kernel (miseg_conv3x3_stem_dgrad); 0: the generic path (the
# streaming / tiled convolution over a dgrad-packed weight whose input channels are padded to one vector; channel 0 of its output).
_bn_untracked = False
_data_grad_only = False
_bn_float_stats = False


@contextlib.contextmanager
def _mode(flag: str):
    """Set the module-level mode ``flag`` for the duration of a ``with`` block."""
    prev, globals()[flag] = globals()[flag], True
    try:
        yield
    finally:
        globals()[flag] = prev


def bn_untracked():
    """Training-mode forwards inside this block normalise with the batch statistics and leave ``running_mean``, ``running_var`` and
    ``num_batches_tracked`` untouched (``track_running_stats`` switched off, as the wheel's ``_disable_tracking_bn_stats`` does): the
    BatchNorm kernels get null pointers for the three, which every forward variant -- accumulator, counter, finalize, stem -- takes as
    "do not track".  Outputs and ``saved`` coefficients are those of a tracked pass.  Evaluation-mode forwards are not affected."""
    return _mode("_bn_untracked")


def bn_float_statistics():
    """Training-mode forwards inside this block take their batch statistics from the float partial sums (one row per convolution
    block + ``miseg_bn_finalize``, or the last-block counter form), not from the fixed-point accumulators: the path ``MISEG_BN_ACC=0``
    selects, for these forwards only.  For computations that DIFFERENCE two forward passes of nearly the same input (VAT's direction at
    a small ``xi``): with the accumulators the direction after one iteration at ``xi = 0.1`` was measured 1.6e-3 from the float64
    reference, with the float sums 1.3e-4, where a float32 evaluation on the CPU lands at 9e-5."""
    return _mode("_bn_float_stats")


def data_grad_only():
    """Forwards inside this block build a graph whose backward DELIVERS data gradients only: no weight-gradient launch of the 3x3
    convolutions, no flat-gradient slot claimed or written, ``param.grad`` untouched, no weight-gradient side stream.  Two sums are
    still formed and dropped, into scratch: gamma's and beta's (the BatchNorm data gradient needs them anyway) and the 1x1 head's
    weight and bias sums, which its one backward kernel forms in the pass that writes the data gradient (68 multiply-adds per pixel).  The flag is read when the
    forward runs and travels in the node, so the backward may run after the block has been left (VAT's direction pass)."""
    return _mode("_data_grad_only")


class _StemSink:
    """Hand-over of the image gradient from the stem layer's backward to ``_StemInput``'s: the layer's input is the zero-padded
    channel vector [B,VEC,H,W] of the storage type, the image's gradient is fp32 [B,1,H,W] -- ``miseg_conv3x3_stem_dgrad`` writes that
    directly, so the layer returns no gradient for the padded operand and leaves the image's here."""
    __slots__ = ("grad", "image")

    def __init__(self):
        self.grad = self.image = None

    def take(self):
        g, self.grad = self.grad, None
        return g


class _StemInput(torch.autograd.Function):
    """``stem_input`` for an image that requires a gradient: the same operand (described or materialised), and a backward that returns
    the image's fp32 gradient -- the stem kernel's (through the sink) or, on the generic path, the real channels of the padded
    operand's gradient."""

    @staticmethod
    def forward(ctx, image: Tensor, dtype, sink: _StemSink):
        ctx.set_materialize_grads(False)
        ctx.sink, ctx.cin = sink, image.shape[1]
        op = _stem_operand(image.detach(), dtype)
        sink.image = getattr(op, "_miseg_stem_f32", None)
        return op

    @staticmethod
    def backward(ctx, g: Optional[Tensor]):
        gimage = ctx.sink.take()
        if gimage is None and g is not None:
            gimage = g[:, :ctx.cin].float().contiguous()
        return gimage, None, None


def stem_input(image: Tensor, dtype) -> Tensor:
    """fp32 [B,Cin,H,W] image -> [B,VEC,H,W] channels_last tensor of ``dtype`` (extra channels zero).  An image that requires a
    gradient gets it: through ``miseg_conv3x3_stem_dgrad`` for one channel, through the generic data-gradient path otherwise."""
    if image.requires_grad and torch.is_grad_enabled():
        sink = _StemSink()
        out = _StemInput.apply(image, dtype, sink)
        if sink.image is not None:             # the operand is only described (see _stem_operand): the description rides on the result
            out._miseg_stem_f32 = sink.image
        out._miseg_stem_sink = sink
        return out
    return _stem_operand(image, dtype)


def _stem_operand(image: Tensor, dtype) -> Tensor:
    _need_gpu(image)
    pre = getattr(image, "_miseg_stem", None)      # the launch that assembled the batch wrote this operand too (ops.cat_flip)
    if pre is not None and pre[0] == dtype and pre[1].shape[0] == image.shape[0]:
        return pre[1]
    b, cin, h, w = image.shape
    if _STEM_KERNELS and cin == 1 and w <= _STEM_MAX_W and image.dtype == torch.float32 and image.is_contiguous() and dtype in (torch.bfloat16, torch.float16):
        # the stem's own kernels read the fp32 image itself (and round it as they read): the padded operand is only DESCRIBED -- an
        # uninitialised tensor of its shape and type that carries the image; conv_bn_relu fills it in if it takes the MFMA path after all
        out = empty_nhwc(b, vec_of(dtype), h, w, dtype, image.device)
        out._miseg_stem_f32 = image
        return out
    image = as_nhwc(image.float())
    cp = vec_of(dtype)
    cp = ((cin + cp - 1) // cp) * cp
    out = empty_nhwc(b, cp, h, w, dtype, image.device)
    call("miseg_cast_pad", _stream(), _ptr(image), b * h * w, cin, _DT[dtype], _ptr(out), cp)
    return out


# ---- the forward plan: which statistics path a layer takes, decided before anything is launched or allocated
_EVAL, _COUNTER, _ACC, _ROWS = "eval", "counter", "acc", "rows"


def _forward_plan(training: bool, stem_ok: bool, counter_ok: bool, use_acc: bool, acc_supported: bool, io, acc_words: int):
    """-> (path, stem, acc): the statistics path, whether the stem kernels serve it, and the accumulator claimed from the step block.
      1. not training                                        eval:    stem_fwd | conv3x3_fwd; bn_eval_coeffs; bn_relu_fwd
      2. ``counter_ok`` (SYNC_COUNTERS.enabled and fusable)  counter: conv3x3_bn_fwd; bn_relu_fwd
      3. ``use_acc`` and (stem or fwd_acc_supported) and an accumulator could be had
                                                             acc:     stem_fwd | conv3x3_fwd_acc; bn_relu_fwd_acc
      4. otherwise                                           rows:    conv3x3_fwd + partial rows; bn_finalize; bn_relu_fwd
    The stem kernel hands its statistics to the accumulator only, so the counter and rows paths never take it (the packed MFMA path
    has statistics rows; the caller then materialises a described stem operand).  ``io`` is the current step block or None: its
    ``acc64`` claims room and is called at most once, only when row 3 is otherwise reached; it returns None when the block has no room
    left (-> rows).  Without a step block (stand-alone use of the layer) row 3 holds and ``acc`` is None: the caller zero-fills one.
    use_acc: 1 (default), the forward statistics leave the convolution as fixed-point atomic adds and the apply kernel finishes them
    itself (miseg_conv3x3_fwd_acc / miseg_bn_relu_fwd_acc): 22 launches fewer per step.  0: one partial row per block + miseg_bn_finalize.
    stem_ok: the stem (one image channel) through its own pixel-per-thread kernels reading the fp32 image, instead of the streaming
    MFMA convolution and the tiled weight gradient on a padded channel vector: the kernels themselves are on a par (50 vs 50 us forward,
    52 + 7 vs 59 + 10 us weight gradient -- the step's last kernel), the padded operand's 15 us launch becomes 4: -0.02 ms per step."""
    if not training:
        return _EVAL, stem_ok, None
    if counter_ok:
        return _COUNTER, False, None
    if use_acc and (stem_ok or acc_supported):
        if io is None:
            return _ACC, stem_ok, None
        acc = io.acc64(acc_words)
        if acc is not None:
            return _ACC, stem_ok, acc
    return _ROWS, False, None


class _ConvBNReLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x0: Tensor, x1: Optional[Tensor], weight: Tensor, gamma: Tensor, beta: Tensor, running_mean: Tensor,
                running_var: Tensor, nbt: Tensor, cfg: tuple):
        training, ups0, ups1, want_pool, rec, rec0, rec1, sink = cfg       # the values that are not tensors (conv_bn_relu)
        _need_gpu(x0, x1, weight)
        ctx.stem_sink = getattr(x0, "_miseg_stem_sink", None)      # stem_input's: the image itself wants a gradient
        ctx.data_only = _data_grad_only
        if training and _bn_untracked:       # frozen statistics: the kernels take null pointers as "do not track" (bn_untracked)
            running_mean = running_var = nbt = None
        use_acc = _BN_ACC and not _bn_float_stats      # (bn_float_statistics: the float partial sums for this forward)
        x0 = as_nhwc(x0)
        dtype, dev = x0.dtype, x0.device
        n, c0 = x0.shape[0], x0.shape[1]
        h, w = x0.shape[2] << ups0, x0.shape[3] << ups0
        c1 = 0
        if x1 is not None:
            x1 = as_nhwc(x1)
            c1 = x1.shape[1]
            assert x1.dtype == dtype and (x1.shape[2] << ups1, x1.shape[3] << ups1) == (h, w)
        cout = weight.shape[0]
        # the stem: one image channel read as a whole (zero-padded) channel vector; the weight keeps its own shape, the pack kernel pads
        assert weight.shape[1] == c0 + c1 or (x1 is None and weight.shape[1] < c0), (weight.shape, c0, c1)
        weight = weight.contiguous().float()
        # the stem (one image channel, padded to a channel vector): its own kernels, no matrix cores (miseg_conv3x3_stem_fwd / _wgrad)
        image = getattr(x0, "_miseg_stem_f32", None)       # stem_input's descriptor: x0 itself is uninitialised
        stem_ok = bool(_STEM_KERNELS and x1 is None and not ups0 and weight.shape[1] == 1 and c0 > 1 and w <= _STEM_MAX_W and
                       query("miseg_conv3x3_stem_supported", _DT[dtype], 1, c0, cout))
        counter_ok = bool(training and SYNC_COUNTERS.enabled and query("miseg_conv3x3_bn_fwd_fusable", _DT[dtype], c0 + c1, n, h, w, cout))
        acc_supported = bool(training and query("miseg_conv3x3_fwd_acc_supported", _DT[dtype], c0 + c1, n, h, w, cout))
        path, stem, acc = _forward_plan(training, stem_ok, counter_ok, use_acc, acc_supported, stepio.current(), 2 * cout + 2)   # sums + misfit count
        packed = None if stem else _pack(weight, dtype, 0, cin=c0 + c1)
        if image is not None and not stem:                                  # the MFMA path after all: materialise the padded operand
            call("miseg_cast_pad", _stream(), _ptr(image), n * h * w, 1, _DT[dtype], _ptr(x0), c0)
            image = None
        raw = empty_nhwc(n, cout, h, w, dtype, dev)
        saved = torch.empty(4 * cout, dtype=torch.float32, device=dev)
        if path == _ACC and acc is None:
            # the statistics leave the convolution as fixed-point atomic adds into one [2 C] accumulator that the step block's upload
            # zeroed; the apply kernel turns them into coefficients itself: no partial rows, no finalize launch
            # (stand-alone use of the layer: a zero fill)
            acc = torch.zeros(2 * cout + 2, dtype=torch.int64, device=dev)
        es = x0.element_size()
        work = (18.0 * (c0 + c1) * cout * n * h * w, float(es) * n * h * w * (c0 / (4 ** ups0) + c1 / (4 ** ups1) + cout))
        if stem:                      # (the eval and acc paths only)
            call("miseg_conv3x3_stem_fwd", _stream(), _DT[dtype], _ptr(image if image is not None else x0), int(image is not None), 1 if image is not None else c0,
                 n, h, w, _ptr(weight), 1, cout, _ptr(raw), _ptr(acc),
                 work=(18.0 * cout * n * h * w, float(es) * n * h * w * (c0 + cout)), tag=f"conv3x3_fwd[{h}x{w},{c0 + c1}->{cout}]")
        elif path == _ACC:
            call("miseg_conv3x3_fwd_acc", _stream(), _DT[dtype], _ptr(x0), c0, ups0, _ptr(x1), c1, ups1, n, h, w, _ptr(packed), cout, _ptr(raw),
                 _ptr(acc), work=work, tag=f"conv3x3_fwd[{h}x{w},{c0 + c1}->{cout}]")
        elif path == _COUNTER:        # the conv's last block turns the partial sums into `saved` / the running statistics itself
            # rows of the statistics matrix: one per block of the kernel that will serve this shape
            stats = torch.empty(query("miseg_conv3x3_stats_parts", _DT[dtype], c0 + c1, n, h, w) * 2 * cout, dtype=torch.float32, device=dev)
            call("miseg_conv3x3_bn_fwd", _stream(), _DT[dtype], _ptr(x0), c0, ups0, _ptr(x1), c1, ups1, n, h, w, _ptr(packed), cout, _ptr(raw),
                 _ptr(stats), _ptr(gamma), _ptr(beta), BN_EPS, BN_MOMENTUM, _ptr(running_mean), _ptr(running_var), _ptr(nbt), _ptr(saved),
                 _ptr(SYNC_COUNTERS.take(dev)), work=work, tag=f"conv3x3_fwd[{h}x{w},{c0 + c1}->{cout}]")
        else:                         # rows: one partial row per block of the kernel that will serve this shape; eval: no statistics
            parts = query("miseg_conv3x3_fwd_parts", _DT[dtype], c0 + c1, n, h, w, cout) if path == _ROWS else 0
            stats = torch.empty(parts * 2 * cout, dtype=torch.float32, device=dev) if path == _ROWS else None
            call("miseg_conv3x3_fwd", _stream(), _DT[dtype], _ptr(x0), c0, ups0, _ptr(x1), c1, ups1, n, h, w, _ptr(packed), cout, _ptr(raw),
                 _ptr(stats), work=work, tag=f"conv3x3_fwd[{h}x{w},{c0 + c1}->{cout}]")
        if path == _ROWS:
            call("miseg_bn_finalize", _stream(), _ptr(stats), parts, cout, n * h * w, _ptr(gamma), _ptr(beta), BN_EPS, BN_MOMENTUM,
                 _ptr(running_mean), _ptr(running_var), _ptr(nbt), _ptr(saved))
        elif path == _EVAL:
            call("miseg_bn_eval_coeffs", _stream(), cout, _ptr(gamma), _ptr(beta), BN_EPS, _ptr(running_mean), _ptr(running_var), _ptr(saved))
        y = empty_nhwc(n, cout, h, w, dtype, dev)
        pooled = empty_nhwc(n, cout, h // 2, w // 2, dtype, dev) if want_pool else None
        if path == _ACC:
            call("miseg_bn_relu_fwd_acc", _stream(), _DT[dtype], _ptr(raw), n, h, w, cout, _ptr(acc), _ptr(gamma), _ptr(beta), BN_EPS, BN_MOMENTUM,
                 _ptr(running_mean), _ptr(running_var), _ptr(nbt), _ptr(saved), _ptr(y), _ptr(pooled),
                 work=(0.0, float(es) * n * h * w * cout * (2.25 if want_pool else 2.0)), tag=f"bn_relu_fwd[{h}x{w},{cout}]")
        else:
            call("miseg_bn_relu_fwd", _stream(), _DT[dtype], _ptr(raw), n, h, w, cout, _ptr(saved), _ptr(y), _ptr(pooled),
                 work=(0.0, float(es) * n * h * w * cout * (2.25 if want_pool else 2.0)), tag=f"bn_relu_fwd[{h}x{w},{cout}]")
        ctx.save_for_backward(x0, x1, weight, gamma, raw, y, saved)
        ctx.param_refs = (weight, gamma, beta)   # the Parameter objects (flat-gradient slots hang off them)
        ctx.cfg = (training, ups0, ups1, want_pool, c0, c1, n, h, w, cout)
        ctx.stem, ctx.image = stem, (image if stem else None)
        if rec is not None:
            rec.raw, rec.saved, rec.shape = raw, saved, (n, cout, h, w)
        ctx.recs = (rec, rec0, rec1)
        ctx.sink = sink
        if want_pool:
            return y, pooled
        return y, None

    @staticmethod
    def backward(ctx, gy: Optional[Tensor], gpool: Optional[Tensor]):
        x0, x1, weight, gamma, raw, y, saved = ctx.saved_tensors
        training, ups0, ups1, want_pool, c0, c1, n, h, w, cout = ctx.cfg
        dtype, dev = raw.dtype, raw.device
        extras = ctx.sink.take() if ctx.sink is not None else []
        if gy is None and gpool is None and not extras:
            return _grads()
        cur = torch.cuda.current_stream(dev)
        for g2, _, _, st2 in extras:
            wait_stream(cur, st2)             # (autograd would have made the same wait before adding the two gradients)
            keep(g2, cur)
        extra = None
        if len(extras) == 1 and (gy is not None or gpool is not None) and extras[0][0].dtype == dtype:
            extra = extras[0]
        elif extras:                          # several heads on one tap, or a tap nothing else consumes: add them here, in torch
            gy = gy.clone() if gy is not None else torch.zeros((n, cout, h, w), dtype=dtype, device=dev, memory_format=torch.channels_last)
            for g2, a, b, _ in extras:
                gy[a:b] += g2.to(dtype)
        rec = ctx.recs[0]
        ext_parts, ext_nparts = rec.take(gy) if rec is not None else (None, 0)
        stem_grad = bool(ctx.needs_input_grad[0] and weight.shape[1] < c0)     # the gradient of the image behind a padded stem operand
        if _FUSE_BN_BWD and not want_pool and gpool is None and gy is not None and not stem_grad and _dgrads_fusable(ctx, dtype):
            return _ConvBNReLU._backward_fused(ctx, gy, ext_parts, ext_nparts)
        gy = None if gy is None else as_nhwc(gy.to(dtype))
        gpool = None if gpool is None else as_nhwc(gpool.to(dtype))
        graw = empty_nhwc(n, cout, h, w, dtype, dev)
        want_w, want_g, want_b, ggamma, gbeta = _param_grads(ctx, cout, dev)
        ws = _ws(query("miseg_bn_bwd_ws_bytes", n, h, w, cout), dev)
        # ---- BatchNorm backward: one decision, one launch
        use_ext = ext_parts is not None and not extras and gpool is None and gy is not None and not want_pool and dtype != torch.float16
        bacc = None
        # _BN_ACC_BWD: the backward's sums through two fixed-point tiers (miseg_bn_relu_bwd_dual_acc).  Built and measured, OFF: the
        # reduce kernel's blocks all finish together, so their atomics arrive as one burst on a few lines (+8 us per launch) and the
        # apply prologue costs 5 us -- more than the finalize launch they replace (6 us + a launch boundary).  DESIGN.md section 10.
        if not use_ext and _BN_ACC_BWD and not SYNC_COUNTERS.enabled and query("miseg_bn_relu_bwd_acc_supported", _DT[dtype], n, h, w, cout):
            # the reduce kernel adds its sums into a zeroed two-tier fixed-point accumulator, the apply kernel finishes them: no finalize launch
            io = stepio.current()
            bacc = io.acc64(4 * cout + 2) if io is not None else torch.zeros(4 * cout + 2, dtype=torch.int64, device=dev)   # (None: block full -> finalize path)
        g2, n0, n1 = (as_nhwc(extra[0]), extra[1], extra[2]) if extra is not None else (None, 0, 0)
        if use_ext:
            # the data-gradient kernel that wrote gy has summed dz and dz * xhat per block in its epilogue: finalize + apply only
            call("miseg_bn_relu_bwd_ext", _stream(), _DT[dtype], _ptr(raw), _ptr(gy), n, h, w, cout, _ptr(gamma), _ptr(saved), int(training),
                 _ptr(graw), _ptr(ggamma), _ptr(gbeta), _ptr(ext_parts), ext_nparts, _ptr(ws), ws.numel(),
                 work=(0.0, float(raw.element_size()) * n * h * w * cout * 3.0), tag=f"bn_relu_bwd[{h}x{w},{cout}]")
        elif bacc is not None:
            call("miseg_bn_relu_bwd_dual_acc", _stream(), _DT[dtype], _ptr(raw), _ptr(gy), _ptr(gpool), _ptr(g2), n0, n1, n, h, w, cout, _ptr(gamma),
                 _ptr(saved), int(training), _ptr(graw), _ptr(ggamma), _ptr(gbeta), _ptr(ws), ws.numel(), _ptr(bacc),
                 work=(0.0, float(raw.element_size()) * n * h * w * cout * 5.0), tag=f"bn_relu_bwd[{h}x{w},{cout}]")
        elif extra is not None:
            call("miseg_bn_relu_bwd_dual", _stream(), _DT[dtype], _ptr(raw), _ptr(gy), _ptr(gpool), _ptr(g2), n0, n1, n, h, w, cout, _ptr(gamma),
                 _ptr(saved), int(training), _ptr(graw), _ptr(ggamma), _ptr(gbeta), _ptr(ws), ws.numel(),
                 work=(0.0, float(raw.element_size()) * n * h * w * cout * 5.0), tag=f"bn_relu_bwd[{h}x{w},{cout}]")
        else:
            call("miseg_bn_relu_bwd_sync", _stream(), _DT[dtype], _ptr(raw), _ptr(y), _ptr(gy), _ptr(gpool), n, h, w, cout, _ptr(gamma), _ptr(saved),
                 int(training), _ptr(graw), _ptr(ggamma), _ptr(gbeta), _ptr(ws), ws.numel(), _ptr(SYNC_COUNTERS.take(dev)),
                 work=(0.0, float(raw.element_size()) * n * h * w * cout * 5.0), tag=f"bn_relu_bwd[{h}x{w},{cout}]")
        gw = None
        if want_w:
            stem_wg = bool(ctx.stem and not _FUSE_BN_BWD)
            # the stem's weight has fewer input channels than the channel vector its activation was padded to: the kernel computes the
            # padded gradient, a slice of it is the parameter's
            padded = weight.shape[1] != c0 + c1 and not stem_wg

            def launch(stream_handle, gw, gw_full, ws2):
                if stem_wg:      # the last kernel of the backward pass: a pixel-per-thread kernel, gw [cout][1][3][3] written directly
                    img = ctx.image
                    call("miseg_conv3x3_stem_wgrad", stream_handle, _DT[dtype], _ptr(img if img is not None else x0), int(img is not None),
                         1 if img is not None else c0, n, h, w, _ptr(graw), cout, _ptr(gw), _ptr(ws2), ws2.numel(),
                         work=(18.0 * cout * n * h * w, float(raw.element_size()) * n * h * w * (c0 + cout)), tag=f"conv3x3_wgrad[{h}x{w},{c0 + c1}->{cout}]")
                    return
                call("miseg_conv3x3_wgrad", stream_handle, _DT[dtype], _ptr(x0), c0, ups0, _ptr(x1), c1, ups1, n, h, w, _ptr(graw), cout, _ptr(gw_full),
                     _ptr(ws2), ws2.numel(), work=(18.0 * (c0 + c1) * cout * n * h * w, float(raw.element_size()) * n * h * w * (c0 + c1 + cout)),
                     tag=f"conv3x3_wgrad[{h}x{w},{c0 + c1}->{cout}]")
                if gw_full is not gw:
                    call("miseg_conv3x3_wgrad_slice", stream_handle, _ptr(gw_full), cout, c0 + c1, weight.shape[1], _ptr(gw))
            gw = _wgrad_fork(ctx.param_refs[0], weight, dev, (graw, x0, x1, ctx.image), launch, c0 + c1 if padded else None,
                             query("miseg_conv3x3_stem_wgrad_ws_bytes", cout) if stem_wg else query("miseg_conv3x3_wgrad_ws_bytes", n, h, w, c0 + c1, cout))
        g0, g1 = _data_grads(ctx, graw, x0, x1, weight, stem_grad)
        return _grads(g0, g1, gw, ggamma if want_g else None, gbeta if want_b else None)

    @staticmethod
    def _backward_fused(ctx, gy_in: Tensor, ext_parts: Optional[Tensor], ext_nparts: int):
        x0, x1, weight, gamma, raw, y, saved = ctx.saved_tensors
        training, ups0, ups1, want_pool, c0, c1, n, h, w, cout = ctx.cfg
        dtype, dev, es = raw.dtype, raw.device, raw.element_size()
        gy = as_nhwc(gy_in.to(dtype))
        want_w, want_g, want_b, ggamma, gbeta = _param_grads(ctx, cout, dev)
        coef = torch.empty(6 * cout, dtype=torch.float32, device=dev)
        if ext_parts is not None:       # the consumer's data-gradient kernel already summed dz and dz * xhat per block: finalize only
            call("miseg_bn_relu_bwd_stats", _stream(), _DT[dtype], None, None, n, h, w, cout, _ptr(gamma), _ptr(saved), int(training), _ptr(coef),
                 _ptr(ggamma), _ptr(gbeta), _ptr(ext_parts), ext_nparts, None, 0)
        else:
            ws = _ws(query("miseg_bn_bwd_ws_bytes", n, h, w, cout), dev)
            call("miseg_bn_relu_bwd_stats", _stream(), _DT[dtype], _ptr(raw), _ptr(gy), n, h, w, cout, _ptr(gamma), _ptr(saved), int(training),
                 _ptr(coef), _ptr(ggamma), _ptr(gbeta), None, 0, _ptr(ws), ws.numel(),
                 work=(0.0, float(es) * n * h * w * cout * 2.0), tag=f"bn_relu_bwd[{h}x{w},{cout}]")
        gw = None
        if want_w:
            def launch(stream_handle, gw, gw_full, ws2):
                call("miseg_conv3x3_wgrad_bn", stream_handle, _DT[dtype], _ptr(x0), c0, ups0, _ptr(x1), c1, ups1, n, h, w, _ptr(raw), _ptr(gy), _ptr(coef),
                     cout, _ptr(gw), _ptr(ws2), ws2.numel(),
                     work=(18.0 * (c0 + c1) * cout * n * h * w, float(es) * n * h * w * (c0 + c1 + 2 * cout)), tag=f"conv3x3_wgrad[{h}x{w},{c0 + c1}->{cout}]")
            gw = _wgrad_fork(ctx.param_refs[0], weight, dev, (raw, gy, coef, x0, x1), launch, None, query("miseg_conv3x3_wgrad_ws_bytes", n, h, w, c0 + c1, cout))
        g0, g1 = _source_grads(ctx, x0, x1, _dgrad_folded, raw, gy, coef, weight)
        return _grads(g0, g1, gw, ggamma if want_g else None, gbeta if want_b else None)


def _grads(g0=None, g1=None, gw=None, ggamma=None, gbeta=None):
    """What a backward of ``_ConvBNReLU`` returns: the five gradients, and None for every other argument of ``forward``."""
    return (g0, g1, gw, ggamma, gbeta) + _NO_GRADS


_NO_GRADS = (None,) * (_ConvBNReLU.forward.__code__.co_argcount - 1 - 5)      # (ctx; x0, x1, weight, gamma, beta)


def _param_grads(ctx, cout: int, dev):
    """-> (want_w, want_g, want_b, ggamma, gbeta): which parameter gradients the backward delivers, and where gamma's and beta's sums
    go.  Written in place when the flat gradient buffer has an open slot -- only for a parameter whose gradient is wanted: a
    data-gradient-only pass (data_grad_only) neither claims nor writes a slot, its sums land in scratch and are dropped."""
    _, pg, pb = ctx.param_refs
    want_g, want_b, want_w = (ctx.needs_input_grad[i] and not ctx.data_only for i in (3, 4, 2))
    ggamma, gbeta = grad_slot(pg) if want_g else None, grad_slot(pb) if want_b else None
    if ggamma is None:
        ggamma = torch.empty(cout, dtype=torch.float32, device=dev)
    if gbeta is None:
        gbeta = torch.empty(cout, dtype=torch.float32, device=dev)
    return want_w, want_g, want_b, ggamma, gbeta


def _wgrad_fork(pw, weight: Tensor, dev, operands, launch, padded_cin: Optional[int], ws_bytes: int) -> Tensor:
    """The weight gradient of one layer, on the side stream when its result lands in the flat buffer (nothing on this stream touches it
    again): ``launch(stream_handle, gw, gw_full, ws)`` issues the kernels that read ``operands``; -> ``gw``.  ``padded_cin``: the kernel
    writes a gradient of that many input channels into ``gw_full``, a scratch tensor (None: ``gw_full`` is ``gw``)."""
    gw = grad_slot(pw)
    side = None
    if gw is None:
        gw = torch.empty_like(weight)
        _second_user_waits(pw, dev)
    elif _WGRAD_SIDE and side_streams_allowed():
        side = wgrad_stream(dev)
    # the workspace comes from the current stream's pool and is handed to the side stream like the operands
    ws = _ws(ws_bytes, dev)
    gw_full = gw if padded_cin is None else torch.empty((weight.shape[0], padded_cin, 3, 3), dtype=torch.float32, device=dev)
    if side is None:
        launch(_stream(), gw, gw_full, ws)
        return gw
    if not _wgrad_dirty:          # first side-stream wgrad of this backward pass: join when the pass ends, so that
        # param.grad (which already aliases the flat slot) is safe to touch from the main stream as soon as
        # backward() returns -- gradient accumulation, clip_grad_norm_, inspection -- not only after collect()
        torch.autograd.Variable._execution_engine.queue_callback(join_wgrad_streams)
    wait_stream(side, torch.cuda.current_stream(dev))        # the operands are produced on the current stream
    for t in operands:            # keep their memory from being recycled under the side stream
        keep(t, side)
    keep(ws, side)
    if gw_full is not gw:
        keep(gw_full, side)
    _wgrad_dirty.add(dev)
    # launched on the side stream by HANDLE (entering the `torch.cuda.stream` context costs 15-20 us of host time, 22 times per
    # backward pass)
    if _cabi.TIMER is not None:       # the per-kernel timer records its events on torch's current stream
        with torch.cuda.stream(side):
            launch(_stream(), gw, gw_full, ws)
    else:
        launch(side.cuda_stream, gw, gw_full, ws)
    return gw


def _data_grads(ctx, graw: Tensor, x0: Tensor, x1: Optional[Tensor], weight: Tensor, stem_grad: bool):
    """The data gradients (g0, g1) of the three-pass backward from ``graw``: both sources of a concat in one launch, the image behind a
    padded stem operand, or one launch per source (``_dgrad_plain``)."""
    training, ups0, ups1, want_pool, c0, c1, n, h, w, cout = ctx.cfg
    dtype, dev = graw.dtype, graw.device
    if _DUAL_DGRAD and x1 is not None and ctx.needs_input_grad[0] and ctx.needs_input_grad[1] and not ups0 and not ups1 and \
            c0 % 16 == 0 and c1 % 4 == 0 and not _GradJoin.enabled and not _epilogue_sums_allowed():
        # concat of two full-resolution sources: both data gradients in ONE launch (graw read once, twice the blocks)
        packed = _pack(weight, dtype, 1, 0, c0 + c1)
        g0, g1 = empty_nhwc(n, c0, h, w, dtype, dev), empty_nhwc(n, c1, h, w, dtype, dev)
        call("miseg_conv3x3_dgrad_dual", _stream(), _DT[dtype], _ptr(graw), cout, n, h, w, _ptr(packed), c0, _ptr(g0), c1, _ptr(g1),
             work=(18.0 * (c0 + c1) * cout * n * h * w, float(graw.element_size()) * n * h * w * (c0 + c1 + cout)),
             tag=f"conv3x3_dgrad[{h}x{w},{cout}->{c0}+{c1}]")
        return g0, g1
    if stem_grad:
        sink = ctx.stem_sink
        if sink is not None and _STEM_DGRAD and weight.shape[1] == 1 and query("miseg_conv3x3_stem_dgrad_supported", _DT[dtype], cout, w):
            # one image channel: the stem's own kernel writes the fp32 image gradient; it reaches the image through the sink
            sink.grad = stem_dgrad(graw, weight)
            return None, None
        # the generic path; the padded channels' gradients are computed and dropped (stem_input's backward keeps the real ones)
        return stem_dgrad_generic(graw, weight, c0), None
    return _source_grads(ctx, x0, x1, _dgrad_plain, graw, weight)


def _source_grads(ctx, x0: Tensor, x1: Optional[Tensor], one, *operands):
    """(g0, g1) = ``one(cfg, *operands, cb, cs, ups, xs, src_rec)`` for each source that wants a gradient: its channel range in the
    weight, its upsampling, the source tensor and the source layer's hand-over record."""
    training, ups0, ups1, want_pool, c0, c1, n, h, w, cout = ctx.cfg
    rec, rec0, rec1 = ctx.recs
    grads = [None, None]
    for s, (cb, cs, ups, xs, src_rec) in enumerate(((0, c0, ups0, x0, rec0), (c0, c1, ups1, x1, rec1))):
        if xs is not None and ctx.needs_input_grad[s]:
            grads[s] = one(ctx.cfg, *operands, cb, cs, ups, xs, src_rec)
    return grads


def _dgrad_plain(cfg, graw: Tensor, weight: Tensor, cb: int, cs: int, ups: int, xs: Tensor, src_rec: Optional[_BnRec]) -> Optional[Tensor]:
    """One source's data gradient from ``graw`` (the three-pass backward)."""
    n, h, w, cout = cfg[6:10]
    dtype, dev, es = graw.dtype, graw.device, graw.element_size()
    packed = _pack(weight, dtype, 1, cb, cs)
    if ups and _FUSE_UPS_DGRAD and query("miseg_conv3x3_fwd_sumpool_supported", _DT[dtype], cout, n, h, w, cs):
        # the source was read through the x2 upsample: its gradient is the 2x2 sum-pool of the data gradient -- pooled in the
        # convolution's epilogue, the full-resolution gradient (4x the bytes) never exists
        joined = _GradJoin.take(xs) if query("miseg_conv3x3_fwd_sumpool_acc_supported", _DT[dtype], cout, n, h, w) else None
        if joined is not None:
            # the source is also a local-MI tap and its head's backward has already written its gradient: add ours into it
            gsum, written, writer = joined
            cur_s = torch.cuda.current_stream(dev)
            cur_s.wait_event(written)
            gsum.record_stream(cur_s)
            call("miseg_conv3x3_fwd_sumpool_acc", _stream(), _DT[dtype], _ptr(graw), cout, n, h, w, _ptr(packed), cs, _ptr(gsum),
                 work=(18.0 * cs * cout * n * h * w, float(es) * n * h * w * (cs / 2 + cout)),
                 tag=f"conv3x3_dgrad[{h}x{w},{cout}->{cs}]")
            if writer != cur_s:
                done = torch.cuda.Event()
                done.record(cur_s)
                writer.wait_event(done)
            return None
        glow = empty_nhwc(n, cs, h // 2, w // 2, dtype, dev)
        call("miseg_conv3x3_fwd_sumpool", _stream(), _DT[dtype], _ptr(graw), cout, n, h, w, _ptr(packed), cs, _ptr(glow),
             work=(18.0 * cs * cout * n * h * w, float(es) * n * h * w * (cs / 4 + cout)),
             tag=f"conv3x3_dgrad[{h}x{w},{cout}->{cs}]")
        _GradJoin.offer(xs, glow)      # if the source is a tap whose head backward has yet to run, it adds into this tensor
        return glow
    gfull = empty_nhwc(n, cs, h, w, dtype, dev)
    red = _red_target(src_rec, ups, dtype, cout, n, h, w, cs)
    if red is not None:      # the source is a BatchNorm layer read at full resolution: its backward sums in this launch's epilogue
        parts, nparts = red
        call("miseg_conv3x3_dgrad_bn", _stream(), _DT[dtype], _ptr(graw), None, None, cout, n, h, w, _ptr(packed), cs, _ptr(gfull), 0,
             _ptr(src_rec.raw), _ptr(src_rec.saved), _ptr(parts),
             work=(18.0 * cs * cout * n * h * w, float(es) * n * h * w * (2 * cs + cout)), tag=f"conv3x3_dgrad[{h}x{w},{cout}->{cs}]")
        src_rec.offer(gfull, parts, nparts)
        return gfull
    call("miseg_conv3x3_fwd", _stream(), _DT[dtype], _ptr(graw), cout, 0, None, 0, 0, n, h, w, _ptr(packed), cs, _ptr(gfull), None,
         work=(18.0 * cs * cout * n * h * w, float(es) * n * h * w * (cs + cout)), tag=f"conv3x3_dgrad[{h}x{w},{cout}->{cs}]")
    return _sumpooled(gfull, cs, n, h, w) if ups else gfull


def _dgrad_folded(cfg, raw: Tensor, gy: Tensor, coef: Tensor, weight: Tensor, cb: int, cs: int, ups: int, xs: Tensor,
                  src_rec: Optional[_BnRec]) -> Tensor:
    """One source's data gradient with graw formed in the kernel's loader from ``raw``, ``gy`` and ``coef`` (the folded backward)."""
    n, h, w, cout = cfg[6:10]
    dtype, dev, es = raw.dtype, raw.device, raw.element_size()
    packed = _pack(weight, dtype, 1, cb, cs)
    flops = 18.0 * cs * cout * n * h * w
    if ups and query("miseg_conv3x3_dgrad_bn_supported", _DT[dtype], cout, n, h, w, cs, 1):
        glow = empty_nhwc(n, cs, h // 2, w // 2, dtype, dev)
        call("miseg_conv3x3_dgrad_bn", _stream(), _DT[dtype], _ptr(raw), _ptr(gy), _ptr(coef), cout, n, h, w, _ptr(packed), cs, _ptr(glow), 1,
             None, None, None, work=(flops, float(es) * n * h * w * (cs / 4 + 2 * cout)), tag=f"conv3x3_dgrad[{h}x{w},{cout}->{cs}]")
        return glow
    gfull = empty_nhwc(n, cs, h, w, dtype, dev)
    red = _red_target(src_rec, ups, dtype, cout, n, h, w, cs)
    if red is not None:
        parts, nparts = red
        call("miseg_conv3x3_dgrad_bn", _stream(), _DT[dtype], _ptr(raw), _ptr(gy), _ptr(coef), cout, n, h, w, _ptr(packed), cs, _ptr(gfull), 0,
             _ptr(src_rec.raw), _ptr(src_rec.saved), _ptr(parts), work=(flops, float(es) * n * h * w * (2 * cs + 2 * cout)),
             tag=f"conv3x3_dgrad[{h}x{w},{cout}->{cs}]")
        src_rec.offer(gfull, parts, nparts)
    else:
        call("miseg_conv3x3_dgrad_bn", _stream(), _DT[dtype], _ptr(raw), _ptr(gy), _ptr(coef), cout, n, h, w, _ptr(packed), cs, _ptr(gfull), 0,
             None, None, None, work=(flops, float(es) * n * h * w * (cs + 2 * cout)), tag=f"conv3x3_dgrad[{h}x{w},{cout}->{cs}]")
    return _sumpooled(gfull, cs, n, h, w) if ups else gfull


def _sumpooled(gfull: Tensor, cs: int, n: int, h: int, w: int) -> Tensor:
    """The gradient of a source read through the x2 upsample, from its full-resolution gradient: the 2x2 sums, as a launch of their own."""
    glow = empty_nhwc(n, cs, h // 2, w // 2, gfull.dtype, gfull.device)
    call("miseg_sumpool2x2", _stream(), _DT[gfull.dtype], _ptr(gfull), n, h, w, cs, _ptr(glow), 0)
    return glow


def stem_dgrad_supported(dtype, cout: int, w: int) -> bool:
    """Whether ``stem_dgrad`` has a kernel for this storage type, channel count and row length (``miseg_conv3x3_stem_dgrad_supported``)."""
    return dtype in _DT and bool(query("miseg_conv3x3_stem_dgrad_supported", _DT[dtype], int(cout), int(w)))


def stem_dgrad(graw: Tensor, weight: Tensor) -> Tensor:
    """Data gradient of the one-channel stem convolution: ``graw`` = NHWC [N,Cout,H,W] of the storage type (the gradient of the raw
    convolution output), ``weight`` = the fp32 master [Cout,1,3,3] -> fp32 [N,1,H,W] (``miseg_conv3x3_stem_dgrad``)."""
    _need_gpu(graw, weight)
    graw = as_nhwc(graw)
    n, cout, h, w = graw.shape
    assert weight.dtype == torch.float32 and tuple(weight.shape) == (cout, 1, 3, 3) and weight.is_contiguous(), (weight.shape, weight.dtype)
    out = torch.empty((n, 1, h, w), dtype=torch.float32, device=graw.device)
    ws = _ws(query("miseg_conv3x3_stem_dgrad_ws_bytes", cout), graw.device)
    call("miseg_conv3x3_stem_dgrad", _stream(), _DT[graw.dtype], _ptr(graw), n, h, w, cout, _ptr(weight), _ptr(out), _ptr(ws), ws.numel(),
         work=(18.0 * cout * n * h * w, float(n * h * w) * (graw.element_size() * cout + 4.0)), tag=f"conv3x3_stem_dgrad[{h}x{w},{cout}->1]")
    return out


def stem_dgrad_generic(graw: Tensor, weight: Tensor, cp: int) -> Tensor:
    """The stem's data gradient without its own kernel: ``weight`` (fp32 [Cout,Cin,3,3], Cin below one channel vector) with its input
    channels zero-padded to ``cp``, packed for the data gradient (kind 1), through the streaming / tiled convolution over ``graw``
    (NHWC [N,Cout,H,W] of the storage type) -> the gradient of the padded operand, NHWC [N,cp,H,W] of the storage type: channels
    [0, Cin) are the image's, the rest are zero.  Any width, any channel count the convolutions take."""
    n, cout, h, w = graw.shape
    cin = weight.shape[1]
    wpad = torch.zeros((cout, cp, 3, 3), dtype=torch.float32, device=graw.device)
    wpad[:, :cin] = weight
    gfull = empty_nhwc(n, cp, h, w, graw.dtype, graw.device)
    call("miseg_conv3x3_fwd", _stream(), _DT[graw.dtype], _ptr(graw), cout, 0, None, 0, 0, n, h, w, _ptr(_pack_now(wpad, graw.dtype, 1, 0, cp)), cp,
         _ptr(gfull), None, work=(18.0 * cp * cout * n * h * w, float(graw.element_size()) * n * h * w * (cp + cout)),
         tag=f"conv3x3_dgrad[{h}x{w},{cout}->{cp}]")
    return gfull


def _second_user_waits(pw, dev) -> None:
    """A weight used by two forward passes of one backward (VAT: the labeled and the perturbed pass): the first user's weight gradient
    went into the flat slot from the side stream, this user's goes into a tensor of its own and autograd ADDS it into that slot on the
    current stream -- which therefore has to see the side stream's launch first."""
    if getattr(pw, "_miseg_grad_slot", None) is not None and dev in _wgrad_dirty:
        wait_stream(torch.cuda.current_stream(dev), wgrad_stream(dev))


def _dgrads_fusable(ctx, dtype) -> bool:
    """Can every data-gradient launch of this layer's backward form graw in its loader?"""
    training, ups0, ups1, want_pool, c0, c1, n, h, w, cout = ctx.cfg
    if _GradJoin.enabled or cout % vec_of(dtype):
        return False
    return all(cs == 0 or query("miseg_conv3x3_dgrad_bn_supported", _DT[dtype], cout, n, h, w, cs, 0) for cs in (c0, c1))


def _red_target(src_rec: Optional[_BnRec], ups: int, dtype, cout: int, n: int, h: int, w: int, cs: int):
    """(parts, nparts) if this data-gradient launch can take the source layer's BatchNorm-backward sums in its epilogue."""
    if not _epilogue_sums_allowed() or src_rec is None or ups or src_rec.raw is None or src_rec.shape != (n, cs, h, w) or \
            src_rec.raw.dtype != dtype:
        return None
    nparts = query("miseg_conv3x3_dgrad_red_parts", _DT[dtype], cout, n, h, w, cs)
    if not nparts:
        return None
    return torch.empty(nparts * 2 * cs, dtype=torch.float32, device=src_rec.raw.device), nparts


def conv_bn_relu(x0: Tensor, x1: Optional[Tensor], weight: Tensor, gamma: Tensor, beta: Tensor, running_mean: Tensor,
                 running_var: Tensor, nbt: Tensor, training: bool, ups0: int = 0, ups1: int = 0,
                 want_pool: bool = False) -> Tuple[Tensor, Optional[Tensor]]:
    # BatchNorm backward folded into the convolutions around it (_FUSE_BN_BWD; layers without the fused pool): the statistics pass leaves
    # six coefficients per channel, the data- and weight-gradient kernels form graw in their loaders (no bn_bwd_apply pass, no graw
    # tensor), and a data-gradient launch whose output is the activation gradient of ANOTHER such layer takes that layer's statistics
    # pass in its epilogue (no bn_relu_bwd_reduce pass there).  OFF by default (MISEG_BN_FUSE=1 turns it on): measured slower,
    # DESIGN.md section 9.
    # the hand-over record exists only where it can be used: the opt-in fused backward, a layer without the fused pool (a pooled layer's
    # backward routes through the 2x2 windows and keeps its own reduce), a forward pass that records a graph
    rec = _BnRec() if (_epilogue_sums_allowed() and not want_pool and torch.is_grad_enabled()) else None
    rec0 = getattr(x0, "_miseg_bn", None) if not ups0 else None
    rec1 = getattr(x1, "_miseg_bn", None) if x1 is not None and not ups1 else None
    sink = _GradSink() if torch.is_grad_enabled() and not _FUSE_BN_BWD else None
    # the values that are not tensors travel as one object, so that autograd's `apply` and `needs_input_grad` see nine arguments
    y, pooled = _ConvBNReLU.apply(x0, x1, weight, gamma, beta, running_mean, running_var, nbt,
                                  (bool(training), int(ups0), int(ups1), bool(want_pool), rec, rec0, rec1, sink))
    if rec is not None and rec.raw is not None:
        y._miseg_bn = rec
    if sink is not None and y.requires_grad:
        y._miseg_grad_sink = sink
    return y, pooled


class _Conv1x1(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: Tensor, weight: Tensor, bias: Tensor):
        _need_gpu(x, weight, bias)
        x = as_nhwc(x)
        n, cin, h, w = x.shape
        cout = weight.shape[0]
        wf = weight.contiguous().float().view(cout, cin)
        bf = bias.contiguous().float()
        out = empty_nhwc(n, cout, h, w, torch.float32, x.device)
        call("miseg_conv1x1_fwd", _stream(), _DT[x.dtype], _ptr(x), n, h, w, cin, _ptr(wf), _ptr(bf), cout, _ptr(out))
        _GradJoin.clear()                # offers of an earlier backward pass that nobody took
        ctx.save_for_backward(x, wf)
        ctx.wshape = tuple(weight.shape)
        ctx.param_refs = (weight, bias)
        ctx.data_only = _data_grad_only
        return out

    @staticmethod
    def backward(ctx, gout: Tensor):
        x, wf = ctx.saved_tensors
        n, cin, h, w = x.shape
        cout = wf.shape[0]
        gout = as_nhwc(gout.float())
        gin = empty_nhwc(n, cin, h, w, x.dtype, x.device) if ctx.needs_input_grad[0] else None
        pw, pb = ctx.param_refs
        want_w, want_b = (ctx.needs_input_grad[i] and not ctx.data_only for i in (1, 2))     # (a data_grad_only pass: scratch, dropped)
        # written in place when the flat gradient buffer has an open slot
        gw, gb = grad_slot(pw) if want_w else None, grad_slot(pb) if want_b else None
        gw = gw.view(cout, cin) if gw is not None else torch.empty_like(wf)
        if gb is None:
            gb = torch.empty(cout, dtype=torch.float32, device=x.device)
        ws = _ws(query("miseg_conv1x1_bwd_ws_bytes", n, h, w, cin, cout), x.device)
        call("miseg_conv1x1_bwd", _stream(), _DT[x.dtype], _ptr(x), _ptr(gout), n, h, w, cin, _ptr(wf), cout, _ptr(gin), _ptr(gw), _ptr(gb),
             _ptr(ws), ws.numel())
        if gin is not None:
            _GradJoin.offer(x, gin)      # a tap's head backward may add its gradient of x into this tensor (ops._GradJoin)
        return gin, gw.view(ctx.wshape) if want_w else None, gb if want_b else None


def conv1x1(x: Tensor, weight: Tensor, bias: Tensor) -> Tensor:
    return _Conv1x1.apply(x, weight, bias)


def count_nonfinite(grad: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """Device float[1]: how many entries of the fp32 tensor ``grad`` are inf or NaN (``miseg_count_nonfinite``)."""
    _need_gpu(grad)
    assert grad.dtype == torch.float32 and grad.is_contiguous()
    if out is None:
        out = torch.empty(1, dtype=torch.float32, device=grad.device)
    call("miseg_count_nonfinite", _stream(), _ptr(grad), grad.numel(), _ptr(out))
    return out


def adam_step(param: Tensor, grad: Tensor, exp_avg: Tensor, exp_avg_sq: Tensor, hyper: Tensor, beta1: float, beta2: float,
              grad_scale: float = 1.0, guard: Optional[Tensor] = None) -> None:
    """Fused Adam on flat fp32 buffers; ``hyper`` = device fp32[4] (lr/bc1, 1/sqrt(bc2), eps, weight_decay); ``grad`` is read as
    grad / grad_scale (the static loss scale of the fp16 mode); ``guard`` = fp32 device flags, any non-zero / NaN one turns the launch
    into a no-op (a failed deferred check must not move the weights)."""
    _need_gpu(param, grad, exp_avg, exp_avg_sq, hyper)
    if guard is not None:
        _need_gpu(guard)
        assert guard.dtype == torch.float32 and guard.is_contiguous()
    # grad_scale == -1: the kernel reads 1 / loss scale from hyper[4] (the step block: a dynamic scale under a replayed launch tape)
    call("miseg_adam_step_guarded", _stream(), _ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), param.numel(), float(beta1),
         float(beta2), _ptr(hyper), float(grad_scale), _ptr(guard), 0 if guard is None else guard.numel())


def _flat_step_args(param: Tensor, grad: Tensor, states, hyper: Tensor, words: int, guard: Optional[Tensor]) -> None:
    _need_gpu(param, grad, hyper, *states)
    for t in (grad, *states):
        assert t.dtype == param.dtype == torch.float32 and t.numel() == param.numel() and t.is_contiguous() and param.is_contiguous()
    assert hyper.dtype == torch.float32 and hyper.is_contiguous() and hyper.numel() >= words
    if guard is not None:
        _need_gpu(guard)
        assert guard.dtype == torch.float32 and guard.is_contiguous()


def radam_step(param: Tensor, grad: Tensor, exp_avg: Tensor, exp_avg_sq: Tensor, hyper: Tensor, beta1: float, beta2: float,
               grad_scale: float = 1.0, guard: Optional[Tensor] = None) -> None:
    """The wheel's RAdam on flat fp32 buffers (``miseg_radam_step``); ``hyper`` = device fp32[5] (step size, rectified as 1 / 0, eps,
    weight decay x lr, 1 / loss scale); ``grad_scale`` and ``guard`` as ``adam_step``'s (-1: the kernel reads ``hyper[4]``)."""
    _flat_step_args(param, grad, (exp_avg, exp_avg_sq), hyper, 5, guard)
    call("miseg_radam_step", _stream(), _ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), param.numel(), float(beta1),
         float(beta2), _ptr(hyper), float(grad_scale), _ptr(guard), 0 if guard is None else guard.numel())


def adabound_step(param: Tensor, grad: Tensor, exp_avg: Tensor, exp_avg_sq: Tensor, max_exp_avg_sq: Optional[Tensor], hyper: Tensor,
                  beta1: float, beta2: float, decoupled: bool, grad_scale: float = 1.0, guard: Optional[Tensor] = None) -> None:
    """The wheel's AdaBound (``decoupled`` weight decay: AdaBoundW) on flat fp32 buffers (``miseg_adabound_step``); ``hyper`` = device
    fp32[6] (step size, lower bound, eps, weight decay, 1 / loss scale, upper bound); ``max_exp_avg_sq``: the amsbound variant's
    running maximum, or None."""
    states = (exp_avg, exp_avg_sq) if max_exp_avg_sq is None else (exp_avg, exp_avg_sq, max_exp_avg_sq)
    _flat_step_args(param, grad, states, hyper, 6, guard)
    call("miseg_adabound_step", _stream(), _ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), _ptr(max_exp_avg_sq), param.numel(),
         float(beta1), float(beta2), _ptr(hyper), int(bool(decoupled)), float(grad_scale), _ptr(guard),
         0 if guard is None else guard.numel())


def ema_update(teacher: Tensor, student: Tensor, coef: Tensor, guard: Optional[Tensor] = None) -> None:
    """Mean Teacher EMA on flat fp32 buffers laid out alike: ``teacher = (teacher * a + b * student) * d`` with ``coef`` = device
    fp32[3] (a, b, d) = (alpha, 1 - alpha, 1 - weight_decay), rounded as torch's eager ``mul_ / add_ / mul_`` (include/miseg_hip.h);
    ``guard``: the fused Adam's flags -- any non-zero / NaN one leaves the teacher untouched."""
    _need_gpu(teacher, student, coef)
    assert teacher.dtype == student.dtype == coef.dtype == torch.float32 and teacher.numel() == student.numel() and coef.numel() >= 3
    assert teacher.is_contiguous() and student.is_contiguous() and coef.is_contiguous()
    if guard is not None:
        _need_gpu(guard)
        assert guard.dtype == torch.float32 and guard.is_contiguous()
    call("miseg_ema_update", _stream(), _ptr(teacher), _ptr(student), teacher.numel(), _ptr(coef), _ptr(guard),
         0 if guard is None else guard.numel(), work=(0.0, 12.0 * teacher.numel()), tag="ema_update")
