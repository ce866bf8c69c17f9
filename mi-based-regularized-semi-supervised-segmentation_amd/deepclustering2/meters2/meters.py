"""Per-epoch meters with the reference's names and summaries
(ref whl:deepclustering2/meters2/meter_interface.py:41-137, individual_meters/averagemeter.py:7-77,
individual_meters/general_dice_meter.py:18-188).

``SurfaceMeter`` (HD / HD95 / ASD) takes GPU tensors through the HIP surface-distance kernel.
``UniversalDice.add`` keeps the reference signature (class-coded ``pred``/``target`` tensors + group
names).  On GPU tensors the per-sample per-class intersection/union counts come from the fused HIP
argmax/Dice kernel when logits are supplied via ``add_logits``; integer counts are bit-exact either way.
"""
from __future__ import annotations

import os
from collections import OrderedDict, defaultdict
from typing import Dict, List, Union

import numpy as np
import torch
from torch import Tensor

from deepclustering2.utils import class2one_hot, iter_average, nice_dict, to_float


class MeterResultDict(dict):
    pass


class _Metric:
    def reset(self): ...
    def add(self, *a, **k): ...
    def summary(self) -> dict: ...
    def detailed_summary(self) -> dict: ...


class AverageValueMeter(_Metric):
    def __init__(self):
        self.reset()

    def reset(self):
        self.n, self.sum = 0, 0.0

    def add(self, value, n=1):
        self.sum += value
        self.n += n

    def value(self):
        return (np.nan if self.n == 0 else self.sum / self.n), np.nan

    def summary(self) -> dict:
        return MeterResultDict({"mean": self.value()[0]})

    def detailed_summary(self) -> dict:
        return MeterResultDict({"mean": self.value()[0], "val": self.value()[1]})


class MultipleAverageValueMeter(_Metric):
    def __init__(self) -> None:
        self._meter_dicts = defaultdict(AverageValueMeter)

    def reset(self):
        for v in self._meter_dicts.values():
            v.reset()

    def add(self, *_, **kwargs):
        for k, v in kwargs.items():
            self._meter_dicts[k].add(v)

    def summary(self) -> MeterResultDict:
        return MeterResultDict({k: v.summary()["mean"] for k, v in self._meter_dicts.items()})

    detailed_summary = summary


class UniversalDice(_Metric):
    """Per-group (patient) 3D Dice ``(2*I + 1e-6) / (U + 1e-6)``; DSC_mean over ``report_axises``."""

    def __init__(self, C=4, report_axises=None) -> None:
        assert report_axises is None or isinstance(report_axises, (list, tuple))
        self._C = C
        self._report_axis = list(range(C)) if report_axises is None else list(report_axises)
        assert max(self._report_axis) <= C
        self.reset()

    def reset(self):
        self._intersections, self._unions, self._group_names, self._n = [], [], [], 0

    def _names(self, batch: int, group_name) -> List[str]:
        if group_name is None:
            return [f"{self._n}_{i:03d}" for i in range(batch)]
        if isinstance(group_name, str):
            return [group_name] * batch
        assert len(group_name) == batch and isinstance(group_name[0], str)
        return list(group_name)

    def add_counts(self, inter: Tensor, union: Tensor, group_name=None):
        """Integer [B,C] intersection / union counts (e.g. from the HIP argmax/Dice kernel)."""
        self._intersections.append(inter.detach().to("cpu", torch.int64))
        self._unions.append(union.detach().to("cpu", torch.int64))
        self._group_names.extend(self._names(inter.shape[0], group_name))
        self._n += 1

    def add(self, pred: Tensor, target: Tensor, group_name: Union[str, List[str]] = None):
        assert pred.shape == target.shape, (pred.shape, target.shape)
        assert not pred.requires_grad and not target.requires_grad
        p, t = class2one_hot(pred, self._C), class2one_hot(target, self._C)
        dims = list(range(2, p.dim()))
        self.add_counts((p * t).sum(dims), (p + t).sum(dims), group_name)

    def value(self, **kwargs):
        if self._n == 0:
            return [np.nan] * self._C, [np.nan] * self._C
        inter, union = torch.cat(self._intersections, 0), torch.cat(self._unions, 0)
        names = np.asarray(self._group_names)
        rows = []
        for g in sorted(set(self._group_names)):
            idx = torch.from_numpy(names == g)
            rows.append((2 * inter[idx].sum(0) + 1e-6) / (union[idx].sum(0) + 1e-6))
        dice = torch.stack(rows, 0)
        return dice.mean(0), dice.std(0)

    def summary(self) -> dict:
        means, _ = self.value()
        rep = {f"DSC{i}": to_float(means[i]) for i in self._report_axis}
        rep["DSC_mean"] = iter_average(rep.values())
        return MeterResultDict(rep)

    def detailed_summary(self) -> dict:
        means, stds = self.value()
        rep = dict(self.summary())
        rep.update({f"DSC_std{i}": to_float(stds[i]) for i in self._report_axis})
        return MeterResultDict(rep)


def _surface_distances(result: np.ndarray, reference: np.ndarray, voxelspacing=None, connectivity: int = 1) -> np.ndarray:
    """Distances from the border voxels of ``result`` to the border of ``reference`` -- MedPy 0.4.0
    ``medpy.metric.binary.__surface_distances`` (requirement.txt:27; not installed here), restated on scipy.ndimage:
    borders = object XOR its erosion with the ``connectivity`` structuring element, Euclidean distance transform of the
    complement of the reference border.  Raises RuntimeError on an empty object, as MedPy does."""
    from scipy.ndimage import binary_erosion, distance_transform_edt, generate_binary_structure
    result = np.atleast_1d(np.asarray(result).astype(bool))
    reference = np.atleast_1d(np.asarray(reference).astype(bool))
    footprint = generate_binary_structure(result.ndim, connectivity)
    if 0 == np.count_nonzero(result):
        raise RuntimeError("The first supplied array does not contain any binary object.")
    if 0 == np.count_nonzero(reference):
        raise RuntimeError("The second supplied array does not contain any binary object.")
    result_border = result ^ binary_erosion(result, structure=footprint, iterations=1)
    reference_border = reference ^ binary_erosion(reference, structure=footprint, iterations=1)
    dt = distance_transform_edt(~reference_border, sampling=voxelspacing)
    return dt[result_border]


def hausdorff_distance(data1, data2, voxelspacing=None) -> float:
    """ref whl:deepclustering2/meters2/individual_meters/surface_distance.py:9-14."""
    hd1 = _surface_distances(data1, data2, voxelspacing, connectivity=1)
    hd2 = _surface_distances(data2, data1, voxelspacing, connectivity=1)
    return max(hd1.max(), hd2.max())


def mod_hausdorff_distance(data1, data2, voxelspacing=None, percentile=95) -> float:
    """The 95th-percentile Hausdorff distance (ref whl:.../surface_distance.py:17-24)."""
    hd1 = _surface_distances(data1, data2, voxelspacing, connectivity=1)
    hd2 = _surface_distances(data2, data1, voxelspacing, connectivity=1)
    return max(np.percentile(hd1, percentile), np.percentile(hd2, percentile))


def average_surface_distance(data1, data2, voxelspacing=None) -> float:
    """MedPy 0.4.0 ``assd`` (ref whl:.../surface_distance.py:27-29): the mean of the two directed mean surface distances."""
    asd1 = _surface_distances(data1, data2, voxelspacing, connectivity=1).mean()
    asd2 = _surface_distances(data2, data1, voxelspacing, connectivity=1).mean()
    return np.mean((asd1, asd2))


_SURFACE_PERCENTILE = 95


def _lerp_sqrt(n: int, qlo_sq: int, qhi_sq: int, q: float) -> float:
    """np.percentile(d, 100 q) of n ascending distances given the squares of its two neighbours in rank: numpy's linear method
    (virtual index v = (n - 1) q, fraction v - floor(v), and its two-sided lerp), in float64."""
    v = (n - 1) * q
    t = v - np.floor(v)
    a, b = np.sqrt(np.float64(qlo_sq)), np.sqrt(np.float64(qhi_sq))
    return float(b - (b - a) * (1 - t)) if t >= 0.5 else float(a + (b - a) * t)


class SurfaceMeter(_Metric):
    """Per-slice, per-class surface distance of class-coded masks (ref whl:.../surface_meter.py:20-145): ``hausdorff`` (HD),
    ``mod_hausdorff`` (MHD, the 95th percentile) or ``average_surface`` (ASD).  Device tensors with unit spacing go through one
    ``miseg_amd.ops.surface_stats`` call and one download per batch, and the host finishes in float64; CPU tensors, a
    ``voxelspacing`` and ``MISEG_SURFACE_HOST=1`` take the scipy restatement of MedPy above."""

    meter_choices = {"mod_hausdorff": mod_hausdorff_distance, "hausdorff": hausdorff_distance, "average_surface": average_surface_distance}
    abbr = {"mod_hausdorff": "MHD", "hausdorff": "HD", "average_surface": "ASD"}

    def __init__(self, C=4, report_axises=None, metername: str = "hausdorff") -> None:
        assert metername in self.meter_choices, metername
        assert report_axises is None or isinstance(report_axises, (list, tuple))
        self._C = C
        self._report_axis = list(report_axises) if report_axises is not None else list(range(C))
        assert max(self._report_axis) <= C
        self._surface_name = metername
        self._abbr = self.abbr[metername]
        self._surface_function = self.meter_choices[metername]
        self.reset()

    def reset(self):
        self._mhd, self._n = [], 0

    @staticmethod
    def on_device(pred: Tensor, target: Tensor, voxelspacing=None) -> bool:
        """GPU slices [N, H, W] with unit spacing, unless ``MISEG_SURFACE_HOST=1``."""
        return pred.is_cuda and target.is_cuda and pred.dim() == 3 and voxelspacing is None and os.environ.get("MISEG_SURFACE_HOST") != "1"

    @staticmethod
    def batch_stats(pred: Tensor, target: Tensor, classes):
        """Host copies (int64 [N, K, 2, 4], float64 [N, K, 2]) of ``ops.surface_stats`` for one batch: one launch, one download.
        Meters with the same ``report_axises`` may share them (``add(..., stats=)``)."""
        from miseg_amd import ops
        stats, sum_dist = ops.surface_stats(pred.detach(), target.detach(), classes, q=_SURFACE_PERCENTILE / 100)
        block = getattr(stats, "_miseg_block", None)      # both outputs in one allocation
        if block is None:
            return stats.cpu().numpy(), sum_dist.cpu().numpy()
        host = block.cpu()
        return host[:stats.numel()].view(stats.shape).numpy(), host[stats.numel():].view(torch.float64).view(sum_dist.shape).numpy()

    def _from_stats(self, stats: np.ndarray, sum_dist: np.ndarray) -> np.ndarray:
        if (stats[..., 0] == 0).any():          # as MedPy: an empty object on either side
            raise RuntimeError("A supplied array does not contain any binary object.")
        if self._surface_name == "hausdorff":
            return np.sqrt(stats[..., 1].max(-1).astype(np.float64))
        if self._surface_name == "average_surface":
            return (sum_dist / stats[..., 0]).sum(-1) / 2
        out = np.zeros(stats.shape[:2])
        for b in range(stats.shape[0]):
            for k in range(stats.shape[1]):
                out[b, k] = max(_lerp_sqrt(int(n), int(lo), int(hi), _SURFACE_PERCENTILE / 100) for n, _, lo, hi in stats[b, k])
        return out

    def add(self, pred: Tensor, target: Tensor, voxelspacing=None, stats=None):
        """``stats``: the ``batch_stats`` of this very batch and these ``report_axises``, to share one launch between meters."""
        assert pred.shape == target.shape, f"incompatible shape of `pred` and `target`, given {pred.shape} and {target.shape}."
        if self.on_device(pred, target, voxelspacing):
            out = self._from_stats(*(stats if stats is not None else self.batch_stats(pred, target, self._report_axis)))
        else:
            p = pred.detach().cpu().numpy()
            t = target.detach().cpu().numpy()
            out = np.zeros([p.shape[0], len(self._report_axis)])
            for b in range(p.shape[0]):
                for k, c in enumerate(self._report_axis):
                    out[b, k] = self._surface_function(p[b] == c, t[b] == c, voxelspacing)   # RuntimeError (empty class) aborts the batch
        self._mhd.append(out)
        self._n += 1

    def value(self, **kwargs):
        if self._n == 0:
            return [np.nan] * self._C, [np.nan] * self._C
        mhd = np.concatenate(self._mhd, axis=0)
        return mhd.mean(0), mhd.std(0)

    def summary(self) -> dict:
        means, _ = self.value()
        return MeterResultDict({f"{self._abbr}{i}": to_float(means[num]) for num, i in enumerate(self._report_axis)})

    def detailed_summary(self) -> dict:
        return self.summary()

    def get_plot_names(self) -> List[str]:
        return [f"{self._abbr}{i}" for i in self._report_axis]


class EpochResultDict(dict):
    def __repr__(self):
        return "".join(f"{k}: \n\t{nice_dict(v)}\n" for k, v in self.items())


class MeterInterface:
    def __init__(self) -> None:
        self._ind_meter_dicts: Dict[str, _Metric] = OrderedDict()
        self._group_dicts: Dict[str, List[str]] = OrderedDict()

    def __getitem__(self, meter_name: str) -> _Metric:
        return self._ind_meter_dicts[meter_name]

    def register_meter(self, name: str, meter: _Metric, group_name=None) -> None:
        assert isinstance(name, str) and isinstance(meter, _Metric), (name, meter)
        self._ind_meter_dicts[name] = meter
        if group_name is not None:
            self._group_dicts.setdefault(group_name, []).append(name)

    def delete_meter(self, name: str) -> None:
        del self._ind_meter_dicts[name]
        for names in self._group_dicts.values():
            if name in names:
                names.remove(name)

    @property
    def meter_names(self) -> List[str]:
        return list(self._ind_meter_dicts.keys())

    @property
    def meters(self):
        return self._ind_meter_dicts

    def tracking_status(self, group_name=None, detailed_summary=False) -> EpochResultDict:
        keys = self._group_dicts[group_name] if group_name else self.meter_names
        return EpochResultDict(**{k: (self.meters[k].detailed_summary() if detailed_summary else self.meters[k].summary())
                                  for k in keys})

    def add(self, meter_name, *args, **kwargs):
        self.meters[meter_name].add(*args, **kwargs)

    def reset(self) -> None:
        for v in self.meters.values():
            v.reset()
