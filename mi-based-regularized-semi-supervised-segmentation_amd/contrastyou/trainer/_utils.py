"""Cluster heads and the contrastive projection heads on the MI355X kernels (ref: contrastyou/trainer/_utils.py:44-93, :96-168).

``ClusterHead`` (global: avg-pool -> Linear -> softmax/T) and ``LocalClusterHead`` (per pixel:
1x1 conv -> channel softmax/T), each with ``num_subheads`` independent sub-heads, same constructor
arguments and the reference's state_dict keys (``_headers.<s>.<idx>.{weight,bias}``).  All sub-heads
of a head run in ONE fused launch.  ``forward(features)`` keeps the reference signature and returns a
list of per-sub-head probabilities; ``forward_gathered(features, src, flips)`` additionally fuses the
epocher's sample gather / flip replay / cat (semi_seg/epocher.py:258-273) into the same kernel.
``head_type='linear'`` with ``normalize=False`` (the shipped config, config/semi.yaml:45-55) runs on the tuned
kernels of csrc/heads_*.hip / heads_global.hip; ``head_type='mlp'`` and ``normalize=True`` (ref :106-126, :146-161) run on the
generic fused kernels of csrc/heads_var.hip (same gather / flip fusion, forward recomputed in the backward).

``ProjectionHead`` (contrastive pre-training: avg-pool -> Linear [-> LeakyReLU -> Linear]) pools the channels_last feature map with
``ops.avgpool_nhwc`` (csrc/contrast.hip); its one or two small ``nn.Linear`` layers stay on torch.  ``LocalProjectionHead`` (decoder
pre-training: 3x3 conv [-> LeakyReLU -> 3x3 conv] -> adaptive max-pool) runs on ``ops.conv3x3_bias`` / ``bias_lrelu`` / ``bias_amaxpool``.
"""
from __future__ import annotations

from typing import List, Optional

import torch
from torch import Tensor, nn

from miseg_amd import ops
from miseg_amd.gradslot import register_adjacent, stacked_param


class Flatten(nn.Module):
    def forward(self, features):
        return features.view(features.shape[0], -1)


class Identical(nn.Module):
    def forward(self, input):
        return input


class SoftmaxWithT(nn.Softmax):
    def __init__(self, dim, T: float = 0.1) -> None:
        super().__init__(dim)
        self._T = T


class Normalize(nn.Module):
    """Parameter-free place holder (ref _utils.py:26-33) so the Sequential indices -- hence the state_dict keys -- match."""

    def forward(self, input):
        return torch.nn.functional.normalize(input, p=2, dim=1)


class ProjectionHead(nn.Module):
    """ref _utils.py:44-65, same Sequential layout (state_dict keys ``_header.2.*`` and, for ``mlp``, ``_header.4.*``): global
    average pool -> Flatten -> Linear(input_dim, interm_dim) -> LeakyReLU(0.01) -> Linear(interm_dim, output_dim), or a single
    Linear(input_dim, output_dim) for ``head_type='linear'``.  The pool reads the network's NHWC feature map in its storage type
    and returns fp32 (``ops.avgpool_nhwc``; GPU only, like every kernel); the Linear layers are fp32 torch modules (2 x 32 x 256 x 256
    FLOPs at the bench shape).  The ``AdaptiveAvgPool2d`` / ``Flatten`` entries of the Sequential only hold the indices."""

    def __init__(self, input_dim, output_dim, interm_dim=256, head_type="mlp") -> None:
        super().__init__()
        assert head_type in ("mlp", "linear"), head_type
        if head_type == "mlp":
            tail = [nn.Linear(input_dim, interm_dim), nn.LeakyReLU(0.01, inplace=True), nn.Linear(interm_dim, output_dim)]
        else:
            tail = [nn.Linear(input_dim, output_dim)]
        self._header = nn.Sequential(nn.AdaptiveAvgPool2d((1, 1)), Flatten(), *tail)

    def forward(self, features: Tensor) -> Tensor:
        x = ops.avgpool_nhwc(features)
        for layer in list(self._header)[2:]:
            x = layer(x)
        return x


class LocalProjectionHead(nn.Module):
    """ref _utils.py:68-93, same constructor and Sequential layout (state_dict keys ``_projector.0.*`` and, for ``mlp``,
    ``_projector.2.*``): Conv2d(input_dim, 64, 3, 1, 1) -> LeakyReLU(0.01) -> Conv2d(64, 32, 3, 1, 1) -> adaptive_max_pool2d, or the
    first convolution and the pool alone for ``head_type='linear'``.  ``forward`` returns the pooled map [N, Cout, OH, OW] (fp32).

    ``embeddings`` returns what the decoder pre-training epocher feeds the contrastive loss,
    ``cat_v(unfold_position(chunk_v(forward(x)), partition_num)[0].view(rows, -1))``, written by the pool kernel itself.

    On the GPU the convolutions are the MFMA kernels (``ops.conv3x3_bias``), their biases ride in the passes behind them
    (``ops.bias_lrelu``, ``ops.bias_amaxpool``; csrc/contrast_decoder.hip) and the feature map stays in its storage type.  CPU tensors
    and shapes a kernel refuses run the torch composition of the same modules."""

    def __init__(self, input_dim, head_type="mlp", output_size=(4, 4)) -> None:
        super().__init__()
        assert head_type in ("mlp", "linear"), head_type
        self._output_size = tuple(int(v) for v in output_size)
        if head_type == "mlp":
            self._projector = nn.Sequential(nn.Conv2d(input_dim, 64, 3, 1, 1), nn.LeakyReLU(0.01, inplace=True), nn.Conv2d(64, 32, 3, 1, 1))
        else:
            self._projector = nn.Sequential(nn.Conv2d(input_dim, 64, 3, 1, 1))

    def _kernel_takes(self, features: Tensor, views: int, partition_num) -> bool:
        if not (features.is_cuda and features.dim() == 4 and features.dtype in (torch.float32, torch.bfloat16, torch.float16)):
            return False
        n, _, h, w = features.shape
        convs = [m for m in self._projector if isinstance(m, nn.Conv2d)]
        return all(ops.conv3x3_bias_supported(m.in_channels, m.out_channels, features.dtype) and ops.bias_lrelu_supported(m.out_channels)
                   for m in convs) and features.shape[1] == convs[0].in_channels and \
            ops.bias_amaxpool_supported(n, convs[-1].out_channels, h, w, self._output_size, partition_num, views)

    def _rows(self, features: Tensor, views: int, partition_num) -> Tensor:
        first = self._projector[0]
        raw = ops.conv3x3_bias(features, first.weight)
        if len(self._projector) == 1:
            return ops.bias_amaxpool(raw, first.bias, self._output_size, partition_num, views)
        hidden = ops.bias_lrelu(raw, first.bias, self._projector[1].negative_slope, inplace=True)
        last = self._projector[2]
        return ops.bias_amaxpool(ops.conv3x3_bias(hidden, last.weight), last.bias, self._output_size, partition_num, views)

    def _composed(self, features: Tensor) -> Tensor:
        out = self._projector(features.to(self._projector[0].weight.dtype))
        return torch.nn.functional.adaptive_max_pool2d(out, output_size=self._output_size)

    def forward(self, features: Tensor) -> Tensor:
        if not self._kernel_takes(features, 1, (1, 1)):
            return self._composed(features)
        rows = self._rows(features, 1, (1, 1))
        return rows.view(features.shape[0], -1, *self._output_size)

    def embeddings(self, features: Tensor, views: int = 2, partition_num=(2, 2)) -> Tensor:
        partition_num = tuple(int(v) for v in partition_num)
        if features.shape[0] % views != 0:
            raise ValueError(f"`features` needs to hold {views} views of a batch, got {features.shape[0]} samples")
        if self._output_size[0] % partition_num[0] or self._output_size[1] % partition_num[1]:
            raise ValueError(f"output_size {self._output_size} is not a multiple of partition_num {partition_num}")
        if self._kernel_takes(features, views, partition_num):
            return self._rows(features, views, partition_num)
        from contrastyou.epocher._utils import unfold_position
        blocks = [unfold_position(chunk, partition_num)[0] for chunk in torch.chunk(self._composed(features), views, dim=0)]
        return torch.cat([b.reshape(b.shape[0], -1) for b in blocks], dim=0)


_GLOBAL_HIDDEN = 128       # ref _utils.py:120: the pooled mlp head's hidden width is fixed


def _stack(layers, attr):
    return stacked_param([getattr(layer, attr) for layer in layers])


class _SubHeadParams:
    """The S sub-heads' parameters as stacked [S, ...] tensors (views of the flat buffers when the optimiser laid them out back
    to back): first layer, and second layer for head_type='mlp'."""

    def _register(self, first, second):
        self._first, self._second = first, second
        for layers in ((first,) if second is None else (first, second)):
            register_adjacent([layer.weight for layer in layers])
            register_adjacent([layer.bias for layer in layers])

    def _stacked(self):
        def flat2(w):       # conv weights [S, R, C, 1, 1] -> [S, R, C], keeping the flat-slot bookkeeping of the stack
            v = w.view(w.shape[0], w.shape[1], -1)
            if hasattr(w, "_miseg_stack_params"):
                v._miseg_stack_params = w._miseg_stack_params
            return v
        w1, b1 = flat2(_stack(self._first, "weight")), _stack(self._first, "bias")
        if self._second is None:
            return w1, b1, None, None
        return w1, b1, flat2(_stack(self._second, "weight")), _stack(self._second, "bias")


class ClusterHead(nn.Module, _SubHeadParams):
    def __init__(self, input_dim, num_clusters=5, num_subheads=10, head_type="linear", T=1, normalize=False) -> None:
        super().__init__()
        assert head_type in ("linear", "mlp"), head_type
        self._input_dim, self._num_clusters, self._num_subheads, self._T, self._normalize = \
            input_dim, num_clusters, num_subheads, T, normalize
        self._head_type = head_type
        tail = lambda: [Normalize() if normalize else Identical(), SoftmaxWithT(1, T=T)]  # noqa: E731
        if head_type == "linear":
            build = lambda: nn.Sequential(nn.AdaptiveAvgPool2d((1, 1)), Flatten(), nn.Linear(input_dim, num_clusters), *tail())  # noqa: E731
        else:
            build = lambda: nn.Sequential(nn.AdaptiveAvgPool2d((1, 1)), Flatten(), nn.Linear(input_dim, _GLOBAL_HIDDEN),  # noqa: E731
                                          nn.LeakyReLU(0.01, inplace=True), nn.Linear(_GLOBAL_HIDDEN, num_clusters), *tail())
        self._headers = nn.ModuleList([build() for _ in range(num_subheads)])
        self._register([h[2] for h in self._headers], [h[4] for h in self._headers] if head_type == "mlp" else None)

    def forward_gathered(self, features: Tensor, src: Tensor) -> Tensor:
        w1, b1, w2, b2 = self._stacked()
        if self._head_type == "linear" and not self._normalize:
            return ops.global_head(features, w1, b1, src, self._T)          # [S, M, K] -- the shipped, tuned kernels
        return ops.global_head_var(features, w1, b1, w2, b2, src, self._T, self._normalize)

    def forward(self, features: Tensor) -> List[Tensor]:
        src = torch.arange(features.shape[0], dtype=torch.int32, device=features.device)
        return list(self.forward_gathered(features, src))


class LocalClusterHead(nn.Module, _SubHeadParams):
    def __init__(self, input_dim, head_type="linear", num_clusters=10, num_subheads=10, T=1, interm_dim=64,
                 normalize=False) -> None:
        super().__init__()
        assert head_type in ("linear", "mlp"), head_type
        self._T, self._normalize, self._head_type = T, normalize, head_type
        tail = lambda: [Normalize() if normalize else Identical(), SoftmaxWithT(1, T=T)]  # noqa: E731
        if head_type == "linear":
            build = lambda: nn.Sequential(nn.Conv2d(input_dim, num_clusters, 1, 1, 0), *tail())  # noqa: E731
        else:
            build = lambda: nn.Sequential(nn.Conv2d(input_dim, interm_dim, 1, 1, 0), nn.LeakyReLU(0.01, inplace=True),  # noqa: E731
                                          nn.Conv2d(interm_dim, num_clusters, 1, 1, 0), *tail())
        self._headers = nn.ModuleList([build() for _ in range(num_subheads)])
        self._register([h[0] for h in self._headers], [h[2] for h in self._headers] if head_type == "mlp" else None)

    def forward_gathered(self, features: Tensor, src: Tensor, flips: Optional[Tensor]) -> Tensor:
        w1, b1, w2, b2 = self._stacked()
        if self._head_type == "linear" and not self._normalize:
            return ops.local_head(features, w1, b1, src, flips, self._T)      # [S, M, K, H, W] -- the shipped, tuned kernels
        return ops.local_head_var(features, w1, b1, w2, b2, src, flips, self._T, self._normalize)

    def forward(self, features: Tensor) -> List[Tensor]:
        src = torch.arange(features.shape[0], dtype=torch.int32, device=features.device)
        return list(self.forward_gathered(features, src, None))
