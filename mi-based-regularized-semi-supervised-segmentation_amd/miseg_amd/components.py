"""Host twin of ``ops.largest_component`` on ``scipy.ndimage.label``: same signature, same results (include/miseg_hip.h,
miseg_largest_component, has the definition).  It serves CPU tensors and, with ``MISEG_COMPONENTS_HOST=1``, GPU tensors too; the
argument checks are shared with the device path, which is why they live here."""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch
from torch import Tensor

MAX_SIDE = 2048
MAX_VALUE = 64           # class values, fill and the Dice class count live in [0, 64)


def check_arguments(pred: Tensor, classes: Sequence[int], connectivity, fill, target: Optional[Tensor], num_classes, out: Optional[Tensor]):
    """The checks of both paths; ValueError throughout (``InferenceEpocher`` swallows RuntimeError).  Returns (classes, fill, C)."""
    if not isinstance(pred, Tensor) or pred.dtype != torch.int64 or pred.dim() != 3:
        raise ValueError(f"largest_component: pred must be an int64 [N, H, W] tensor, got {getattr(pred, 'dtype', type(pred))} "
                         f"{tuple(getattr(pred, 'shape', ()))}")
    n, h, w = pred.shape
    if n < 1 or h < 1 or w < 1 or max(h, w) > MAX_SIDE or n * h * w >= 2 ** 31:
        raise ValueError(f"largest_component: needs N >= 1, 1 <= H, W <= {MAX_SIDE} and fewer than 2^31 pixels, got {n} x {h} x {w}")
    if connectivity not in (1, 2):
        raise ValueError(f"largest_component: connectivity must be 1 (faces) or 2 (full neighbourhood), got {connectivity!r}")
    cls = tuple(int(c) for c in classes)
    if not 1 <= len(cls) <= MAX_VALUE or any(not 0 <= c < MAX_VALUE for c in cls):
        raise ValueError(f"largest_component: classes must be 1 to {MAX_VALUE} values in [0, {MAX_VALUE}), got {cls}")
    if len(set(cls)) != len(cls):
        raise ValueError(f"largest_component: duplicate classes in {cls}")
    fill = int(fill)
    if not 0 <= fill < MAX_VALUE or fill in cls:
        raise ValueError(f"largest_component: fill must lie in [0, {MAX_VALUE}) and not be one of the classes, got {fill} with {cls}")
    c = 0
    if target is not None:
        if not isinstance(target, Tensor) or target.dtype != torch.int64 or target.shape != pred.shape or target.device != pred.device:
            raise ValueError("largest_component: target must be an int64 tensor of pred's shape on pred's device")
        if num_classes is None or not 1 <= int(num_classes) <= MAX_VALUE:
            raise ValueError(f"largest_component: a target needs num_classes in [1, {MAX_VALUE}], got {num_classes!r}")
        c = int(num_classes)
    if out is not None and (not isinstance(out, Tensor) or out.dtype != torch.int64 or out.shape != pred.shape or out.device != pred.device
                            or not out.is_contiguous()):
        raise ValueError("largest_component: out must be a contiguous int64 tensor of pred's shape on pred's device")
    return cls, fill, c


def pack(out, stats, labels, counts):
    """(out, stats), then labels when asked, then (inter, uni) when a target was given."""
    res = [out, stats]
    if labels is not None:
        res.append(labels)
    if counts is not None:
        res.append(counts)
    return tuple(res)


def largest_component_host(pred: Tensor, classes: Sequence[int], volume: bool = False, connectivity: int = 1, fill: int = 0,
                           target: Optional[Tensor] = None, num_classes: Optional[int] = None, want_labels: bool = False, ws=None,
                           out: Optional[Tensor] = None):
    """``ops.largest_component`` on the host: one ``scipy.ndimage.label`` per (unit, class).  The results live on pred's device."""
    from scipy.ndimage import generate_binary_structure, label
    cls, fill, c = check_arguments(pred, classes, connectivity, fill, target, num_classes, out)
    dev = pred.device
    p = pred.detach().cpu().numpy()
    n, h, w = p.shape
    units = [p] if volume else list(p)
    rank = 3 if volume else 2
    structure = generate_binary_structure(rank, 1 if connectivity == 1 else rank)
    cleaned = p.copy()
    cleaned_units = [cleaned] if volume else list(cleaned)
    lab_out = np.full(p.shape, -1, np.int32)
    lab_units = [lab_out] if volume else list(lab_out)
    stats = np.zeros((len(units), len(cls), 3), np.int64)
    for u, unit in enumerate(units):
        for k, value in enumerate(cls):
            lab, count = label(unit == value, structure=structure)
            if count == 0:
                continue
            sizes = np.bincount(lab.ravel())[1:]
            keep = int(np.argmax(sizes)) + 1
            stats[u, k] = (count, sizes[keep - 1], sizes.sum())
            cleaned_units[u][(lab != 0) & (lab != keep)] = fill
            ids, first = np.unique(lab.ravel(), return_index=True)       # first pixel (raster order) of every component
            table = np.full(count + 1, -1, np.int64)
            table[ids] = first
            lab_units[u][lab != 0] = table[lab[lab != 0]]
    counts = None
    if target is not None:
        t = target.detach().cpu().numpy()
        inter, uni = np.zeros((n, c), np.int64), np.zeros((n, c), np.int64)
        for b in range(n):
            o_in, t_in = (cleaned[b] >= 0) & (cleaned[b] < c), (t[b] >= 0) & (t[b] < c)
            uni[b] = np.bincount(cleaned[b][o_in], minlength=c) + np.bincount(t[b][t_in], minlength=c)
            inter[b] = np.bincount(cleaned[b][o_in & (cleaned[b] == t[b])], minlength=c)
        counts = (torch.from_numpy(inter).to(dev), torch.from_numpy(uni).to(dev))
    result = torch.from_numpy(cleaned).to(dev)
    if out is not None:
        out.copy_(result)
        result = out
    return pack(result, torch.from_numpy(stats).to(dev), torch.from_numpy(lab_out).to(dev) if want_labels else None, counts)
