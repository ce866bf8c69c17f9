"""Supervised contrastive loss (Khosla et al., arXiv:2004.11362; SimCLR, arXiv:2002.05709, without labels) with the surface of
ref ``contrastyou/losses/contrast_loss.py:11-100``: ``SupConLoss(temperature, contrast_mode, base_temperature)`` and
``forward(features [bsz, n_views, ...], labels=None, mask=None)``.

Two paths.  ``contrast_mode='all'`` without an explicit ``mask`` on the GPU runs ONE library call (``miseg_amd.ops.supcon``,
csrc/supcon.hip: normalisation, loss and the gradient, deterministic); everything else -- ``'one'``, an explicit (possibly asymmetric)
``mask``, CPU tensors, a shape outside ``ops.supcon_supported`` -- is composed from torch operations below.

The kernel L2-normalises its rows.  The pre-training epocher hands it the projector's RAW output through ``from_embeddings`` (the
reference's ``F.normalize`` -> ``chunk`` -> ``stack`` -> criterion, contrast_epocher.py:90-95, in one node).  ``forward`` takes the
unit-norm rows the reference's callers pass; normalising them again changes them by rounding only.  Rows that are NOT unit-norm give
the reference's value through the composition alone: pass an explicit ``mask`` or build the module with ``fused=False``.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor, nn

__all__ = ["SupConLoss"]


class SupConLoss(nn.Module):
    def __init__(self, temperature=0.07, contrast_mode="all", base_temperature=0.07, fused: bool = True):
        super().__init__()
        self.temperature = temperature
        self.contrast_mode = contrast_mode
        self.base_temperature = base_temperature
        self.fused = fused

    # ------------------------------------------------------------------ the reference's entry
    def forward(self, features: Tensor, labels=None, mask: Optional[Tensor] = None) -> Tensor:
        if features.dim() < 3:
            raise ValueError("`features` needs to be [bsz, n_views, ...],at least 3 dimensions are required")
        features = features.reshape(features.shape[0], features.shape[1], -1)
        bsz, views = features.shape[:2]
        if labels is not None and mask is not None:
            raise ValueError("Cannot define both `labels` and `mask`")
        if labels is not None:
            labels = self._label_tensor(labels, features.device)
            if labels.numel() != bsz:
                raise ValueError("Num of labels does not match num of features")
        if self.contrast_mode not in ("all", "one"):
            raise ValueError("Unknown mode: {}".format(self.contrast_mode))
        if mask is None and self._kernel_takes(features, views * bsz, features.shape[2], views):
            from miseg_amd import ops
            rows = features.transpose(0, 1).reshape(views * bsz, -1)      # view-major, the order of cat(unbind(features, 1))
            return ops.supcon(rows, labels, views, self.temperature, self.base_temperature)
        if mask is None:
            ids = torch.arange(bsz, device=features.device) if labels is None else labels
            mask = ids.view(-1, 1) == ids.view(1, -1)
        return self._composed(features, mask.to(features.device, torch.float32))

    # ------------------------------------------------------------------ the epocher's entry
    def from_embeddings(self, e: Tensor, labels=None, views: int = 2) -> Tensor:
        """The loss of ``forward(stack(chunk(F.normalize(e, dim=1), views), 1), labels)`` from the projector's raw, un-normalised
        ``e`` [views * bsz, dim] (rows ``v * bsz .. v * bsz + bsz - 1`` are view ``v``)."""
        if e.dim() != 2 or e.shape[0] % views != 0:
            raise ValueError(f"`e` needs to be [n_views * bsz, dim] with n_views = {views}, got {tuple(e.shape)}")
        bsz = e.shape[0] // views
        if labels is not None:
            labels = self._label_tensor(labels, e.device)
            if labels.numel() != bsz:
                raise ValueError("Num of labels does not match num of features")
        if self._kernel_takes(e, e.shape[0], e.shape[1], views):
            from miseg_amd import ops
            return ops.supcon(e, labels, views, self.temperature, self.base_temperature)
        unit = torch.nn.functional.normalize(e.float(), dim=1)
        return self.forward(torch.stack(torch.chunk(unit, views, dim=0), dim=1), labels=labels)

    # ------------------------------------------------------------------ helpers
    def _kernel_takes(self, t: Tensor, n: int, d: int, views: int) -> bool:
        if not (self.fused and self.contrast_mode == "all" and t.is_cuda):
            return False
        from miseg_amd import ops
        return ops.supcon_supported(n, d, views)

    @staticmethod
    def _label_tensor(labels, device) -> Tensor:
        if not torch.is_tensor(labels):
            labels = torch.tensor(list(labels), dtype=torch.int32)
        return labels.reshape(-1).to(device)

    def _composed(self, features: Tensor, mask: Tensor) -> Tensor:
        """torch composition; ``mask`` float [bsz, bsz], mask[i, j] = 1 where sample j is a positive of sample i."""
        bsz, views = features.shape[:2]
        contrast = features.transpose(0, 1).reshape(views * bsz, -1)
        anchors, repeats = (contrast, views) if self.contrast_mode == "all" else (features[:, 0], 1)
        sim = anchors @ contrast.t() / self.temperature
        sim = sim - sim.max(dim=1, keepdim=True).values.detach()         # stability only: the shift cancels in the log-probability
        # anchor a is row a of `contrast` in both modes: that column is the anchor itself and takes no part
        others = 1.0 - torch.eye(anchors.shape[0], contrast.shape[0], device=features.device, dtype=sim.dtype)
        positives = mask.to(sim.dtype).repeat(repeats, views) * others
        log_prob = sim - torch.log((torch.exp(sim) * others).sum(dim=1, keepdim=True) + 1e-16)
        per_anchor = (positives * log_prob).sum(dim=1) / positives.sum(dim=1)
        return -(self.temperature / self.base_temperature) * per_anchor.mean()
