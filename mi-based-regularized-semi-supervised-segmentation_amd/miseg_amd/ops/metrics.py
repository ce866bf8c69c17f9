"""Evaluation metrics on the device (csrc/metrics.hip, surface.hip, components.hip): Dice counts, surface distances, the largest
connected component."""
from __future__ import annotations

import os
from typing import Optional, Sequence

import torch
from torch import Tensor

from .. import components as host, stepio
from .._cabi import query
from .._rt import _need_gpu, _ptr, _stream, _ws, cached_const, logits_nhwc
from ._pkg import call


def argmax_dice(logits: Tensor, labels: Optional[Tensor], want_pred: bool = True, to_host: bool = False):
    """argmax over channels and per-sample per-class (intersection, union) int64 counts.  ``to_host``: inside a training iteration,
    write the counts into the iteration's read-back block (``stepio``) so that they travel with its scalars."""
    _need_gpu(logits, labels)
    logits = logits_nhwc(logits)
    n, c, h, w = logits.shape
    dev = logits.device
    pred = torch.empty(n, h, w, dtype=torch.int64, device=dev) if want_pred else None
    inter = uni = None
    if labels is not None:
        labels = labels.contiguous().view(n, h, w).long()
        io = stepio.CURRENT if to_host else None
        if io is not None and io.device == dev:          # the iteration's one device -> host copy carries them
            inter, uni = io.out("inter", (n, c), torch.int64), io.out("union", (n, c), torch.int64)
        else:
            inter = torch.empty(n, c, dtype=torch.int64, device=dev)
            uni = torch.empty(n, c, dtype=torch.int64, device=dev)
    call("miseg_argmax_dice", _stream(), _ptr(logits), _ptr(labels), n, h, w, c, _ptr(pred), _ptr(inter), _ptr(uni))
    return pred, inter, uni


def surface_stats(pred: Tensor, target: Tensor, classes: Sequence[int], q: float = 0.95, ws: Optional[Tensor] = None):
    """Surface-distance statistics of class-coded masks ``pred``, ``target`` ([N, H, W] integer device tensors, unit spacing) for the
    classes listed: ``stats`` int64 [N, len(classes), 2, 4] = (n, max_sq, qlo_sq, qhi_sq) per direction (0: border of pred -> border of
    target, 1: the converse) and ``sum_dist`` float64 [N, len(classes), 2] (include/miseg_hip.h, miseg_surface_stats).  One library
    call, no host sync; ``ws``: scratch to use instead of a fresh allocation (the library checks its size)."""
    _need_gpu(pred, target)
    if pred.shape != target.shape or pred.dim() != 3:
        raise ValueError(f"surface_stats: pred and target must both be [N, H, W], got {tuple(pred.shape)} and {tuple(target.shape)}")
    n, h, w = pred.shape
    if max(h, w) > 512:      # not a RuntimeError: InferenceEpocher ignores those (an absent class), and this must not pass for one
        raise ValueError(f"surface_stats: the kernel handles H, W <= 512, got {h} x {w}; MISEG_SURFACE_HOST=1 takes SurfaceMeter's scipy path")
    dev = pred.device
    pred, target = pred.contiguous().long(), target.contiguous().long()
    cls = tuple(int(c) for c in classes)
    cls_dev = cached_const(("surface_classes", str(dev), cls), lambda: torch.tensor(cls, dtype=torch.int32, device=dev))
    rows = n * len(cls) * 2
    block = torch.empty(rows * 5, dtype=torch.int64, device=dev)       # both outputs in one allocation: one copy brings them to the host
    stats, sum_dist = block[:rows * 4].view(n, len(cls), 2, 4), block[rows * 4:].view(torch.float64).view(n, len(cls), 2)
    stats._miseg_block = block
    if ws is None:
        ws = _ws(query("miseg_surface_stats_ws_bytes", n, h, w, len(cls)), dev)
    call("miseg_surface_stats", _stream(), _ptr(pred), _ptr(target), n, h, w, _ptr(cls_dev), len(cls), float(q), _ptr(stats),
         _ptr(sum_dist), _ptr(ws), ws.numel())
    return stats, sum_dist


def largest_component(pred: Tensor, classes: Sequence[int], volume: bool = False, connectivity: int = 1, fill: int = 0,
                      target: Optional[Tensor] = None, num_classes: Optional[int] = None, want_labels: bool = False,
                      ws: Optional[Tensor] = None, out: Optional[Tensor] = None):
    """Keep the largest connected component of each class in ``classes`` of the class-coded ``pred`` (int64 [N, H, W]); every other
    pixel of those classes becomes ``fill`` (include/miseg_hip.h, miseg_largest_component, has the definition: scipy.ndimage.label's,
    ties to the component with the first pixel).  ``volume``: the N slices are one 3-D unit instead of N 2-D ones; ``connectivity`` 1 =
    faces, 2 = the full neighbourhood.  Returns ``(out, stats)`` with ``stats`` int64 [U, len(classes), 3] = (components, pixels kept,
    pixels of the class); then ``labels`` (int32 [N, H, W], the first pixel index of the pixel's component, -1 elsewhere) if
    ``want_labels``; then ``(inter, uni)`` (int64 [N, num_classes], ``argmax_dice``'s counts of ``out`` against ``target``) if a target
    is given.  ``out`` may be ``pred`` itself.  One library call, no host sync.  CPU tensors, and every tensor with
    ``MISEG_COMPONENTS_HOST=1``, take the scipy twin (``miseg_amd.components``); ``MISEG_COMPONENTS_HOST=0`` refuses CPU tensors.
    Every bad argument is a ValueError, never a RuntimeError, which ``InferenceEpocher`` would take for an absent class."""
    mode = os.environ.get("MISEG_COMPONENTS_HOST")
    cls, fill, c = host.check_arguments(pred, classes, connectivity, fill, target, num_classes, out)
    if not pred.is_cuda or mode == "1":
        if not pred.is_cuda and mode == "0":
            raise ValueError("largest_component: CPU tensors with MISEG_COMPONENTS_HOST=0 (the host path is switched off)")
        return host.largest_component_host(pred, cls, volume, connectivity, fill, target, num_classes, want_labels, None, out)
    n, h, w = pred.shape
    dev = pred.device
    pred = pred.contiguous()
    rank = 3 if volume else 2
    cls_dev = cached_const(("component_classes", str(dev), cls), lambda: torch.tensor(cls, dtype=torch.int32, device=dev))
    out = torch.empty_like(pred) if out is None else out
    labels = torch.empty(n, h, w, dtype=torch.int32, device=dev) if want_labels else None
    stats = torch.empty(1 if volume else n, len(cls), 3, dtype=torch.int64, device=dev)
    inter = uni = None
    if target is not None:
        target = target.contiguous()
        block = torch.empty(2, n, c, dtype=torch.int64, device=dev)
        inter, uni = block[0], block[1]
    if ws is None:
        ws = _ws(query("miseg_largest_component_ws_bytes", n, h, w, len(cls), rank), dev)
    call("miseg_largest_component", _stream(), _ptr(pred), n, h, w, _ptr(cls_dev), len(cls), rank, int(connectivity), fill, _ptr(out),
         _ptr(labels), _ptr(stats), _ptr(target), c, _ptr(inter), _ptr(uni), _ptr(ws), ws.numel())
    return host.pack(out, stats, labels, None if target is None else (inter, uni))
