from typing import Optional, Sequence, Tuple

import torch
from torch import nn

Model = nn.Module  # the reference's Model wrapper is not on the semi-supervised path


class ema_updater:
    """The Mean Teacher's exponential moving average (whl:deepclustering2/models/ema.py:96-131), same signature and schedule:
    ``alpha_k = min(1 - 1 / (k + 1), alpha)`` with ``k`` = this updater's call count (``justify_alpha``; so the first update copies
    the student), then ``t = t * alpha_k + (1 - alpha_k) * s`` and ``t = t * (1 - weight_decay)`` for every parameter; with
    ``update_bn`` the BatchNorm running statistics too.

    Underneath, the teacher's parameters live in one flat buffer laid out as the student's (``miseg_amd.flat.MirrorBuffers``) and
    the update is ONE kernel launch (``miseg_ema_update``) whose coefficients are read from device memory.  Split in two halves like
    the fused Adam: ``host_step`` advances the call count and returns the coefficients, ``apply`` launches the kernel on them (the
    Mean Teacher epocher stages them in the iteration's step block, so a replayed launch tape reads each step's alpha).  Unlike the
    wheel's updater, the call count is state: ``state_dict`` / ``load_state_dict`` carry it, so a resumed run continues the schedule.
    GPU only: models on the CPU raise, as every kernel entry does."""

    def __init__(self, alpha=0.999, justify_alpha=True, weight_decay=1e-5, update_bn=False) -> None:
        self._alpha = alpha
        self._weight_decay = weight_decay
        self._update_bn = update_bn
        self._justify_alpha = justify_alpha
        self._global_step = 0
        self._mirror = None           # the teacher's flat buffer (miseg_amd.flat.MirrorBuffers of the student's)
        self._mirror_of = None

    # ------------------------------------------------------------------ schedule
    def alpha_at(self, k: int) -> float:
        alpha = self._alpha
        if self._justify_alpha:
            alpha = min(1 - 1 / (k + 1), self._alpha)
        return alpha

    def host_step(self) -> Tuple[float, float, float]:
        """(alpha, 1 - alpha, 1 - weight_decay) of this call, in double as the wheel computes them; advances the call count."""
        alpha = self.alpha_at(self._global_step)
        self._global_step += 1
        return alpha, 1 - alpha, 1 - self._weight_decay if self._weight_decay > 0 else 1.0

    @property
    def global_step(self) -> int:
        return self._global_step

    def state_dict(self) -> dict:
        return {"global_step": self._global_step, "alpha": self._alpha, "justify_alpha": self._justify_alpha,
                "weight_decay": self._weight_decay, "update_bn": self._update_bn}

    def load_state_dict(self, state_dict: dict, strict: bool = True) -> None:
        self._global_step = int(state_dict["global_step"])

    # ------------------------------------------------------------------ device half
    def flats(self, ema_model: nn.Module, student_flat) -> "object":
        """The teacher's flat mirror of ``student_flat`` (``miseg_amd.flat.FlatBuffers``), built on first use and whenever either
        buffer moved."""
        from miseg_amd.flat import MirrorBuffers
        m = self._mirror
        if m is None or m.like is not student_flat or self._mirror_of is not ema_model:
            m = self._mirror = MirrorBuffers(list(ema_model.parameters()), student_flat)
            self._mirror_of = ema_model
        m.ensure()
        return m

    @torch.no_grad()
    def apply(self, ema_model: nn.Module, student_flat, coef: torch.Tensor, guard: Optional[torch.Tensor] = None) -> None:
        from miseg_amd import packcache, unet_ops
        mirror = self.flats(ema_model, student_flat)
        unet_ops.ema_update(mirror.flat_param, student_flat.flat_param, coef, guard)
        packcache.PACK_CACHE.invalidate()      # the teacher's masters changed: its packed operand copies are stale

    @torch.no_grad()
    def __call__(self, ema_model: nn.Module, student_model: nn.Module):
        from miseg_amd.ops import _need_gpu
        sp, tp = list(student_model.parameters()), list(ema_model.parameters())
        _need_gpu(*sp[:1], *tp[:1])
        student_flat = self._student_flat(sp)
        coef = torch.tensor(self.host_step(), dtype=torch.float32).to(sp[0].device, non_blocking=True)
        self.apply(ema_model, student_flat, coef)
        if self._update_bn:
            self._average_buffers(ema_model, student_model, coef)

    def _student_flat(self, sp: Sequence[nn.Parameter]):
        """The flat buffer the student's parameters live in (the fused Adam's), else one built for them here."""
        from miseg_amd.flat import FlatBuffers, owner_of
        owner = owner_of(list(sp))
        if owner is not None:
            return owner
        fb = getattr(self, "_own_flat", None)
        if fb is None or [id(p) for p in fb.given] != [id(p) for p in sp]:
            fb = self._own_flat = FlatBuffers(list(sp))
        fb.ensure()
        return fb

    @staticmethod
    def _average_buffers(ema_model: nn.Module, student_model: nn.Module, coef: torch.Tensor) -> None:
        from miseg_amd import unet_ops
        for (name, t), (_, s) in zip(ema_model.named_buffers(), student_model.named_buffers()):
            if ("running_mean" in name or "running_var" in name) and t.is_contiguous() and s.is_contiguous():
                unet_ops.ema_update(t, s, coef)
