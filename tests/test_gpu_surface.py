"""``miseg_surface_stats`` against the host references of tests/surface_ref.py, bit for bit in the integers; ``SurfaceMeter``'s
device path against its host path; ``InferenceEpocher`` with the three surface meters."""
import os
import sys

import numpy as np
import pytest
import torch

import surface_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mi-based-regularized-semi-supervised-segmentation_amd")
QS = (0.95, 0.0, 1.0, 0.5)


def ops():
    from miseg_amd import ops as _ops
    return _ops


def _dev(*arrays):
    return tuple(torch.from_numpy(np.array(a)).to(DEV) for a in arrays)


def _check(stats, sum_dist, want_stats, want_sums, what):
    """Integers: equal.  Sums: each square root is within 1 ulp and there are n additions in double -> (n + 2) * 2^-53 relative."""
    stats, sum_dist = stats.cpu(), sum_dist.cpu().numpy()
    assert torch.equal(stats, torch.from_numpy(want_stats)), (what, (stats.numpy() != want_stats).nonzero())
    bound = (want_stats[..., 0] + 2) * 2.0 ** -53 * want_sums
    err = np.abs(sum_dist - want_sums)
    assert (err <= bound).all(), (what, float(err.max()))


@pytest.mark.parametrize("classes", [(1, 2, 3), (1, 3)])
@pytest.mark.parametrize("shape", R.SHAPES)
def test_kernel_equals_the_reference_on_the_zoo(shape, classes):
    dist = R.zoo_distances(*shape, classes)
    for name, p, t in R.zoo(*shape):
        dp, dt = _dev(p, t)
        for q in QS:
            stats, sum_dist = ops().surface_stats(dp, dt, classes, q=q)
            assert stats.shape == (3, len(classes), 2, 4) and stats.dtype == torch.int64
            assert sum_dist.shape == (3, len(classes), 2) and sum_dist.dtype == torch.float64
            _check(stats, sum_dist, *R.stats_from(dist[name], 3, len(classes), q), (name, q))


def test_kernel_on_random_discs_256():
    p, t = R.discs(2, 256, seed=11)
    dist = R.distances_ref(p, t, (1, 2, 3))
    assert sum(v is not None for v in dist.values()) >= 8          # the seed leaves (nearly) every class in both masks
    dp, dt = _dev(p, t)
    for q in (0.95, 0.5):
        _check(*ops().surface_stats(dp, dt, (1, 2, 3), q=q), *R.stats_from(dist, 2, 3, q), q)


def test_kernel_two_pixels_in_opposite_corners_512():
    """max_sq = 2 * 511^2 = 522 242: more than 16 bits, and the column walk crosses the whole image."""
    p, t = np.zeros((1, 512, 512), np.int64), np.zeros((1, 512, 512), np.int64)
    p[0, 0, 0] = t[0, 511, 511] = 1
    stats, sum_dist = ops().surface_stats(*_dev(p, t), (1,), q=0.95)
    want = torch.tensor([1, 2 * 511 ** 2, 2 * 511 ** 2, 2 * 511 ** 2]).expand(1, 1, 2, 4)
    assert torch.equal(stats.cpu(), want)
    assert torch.equal(sum_dist.cpu(), torch.full((1, 1, 2), float(np.sqrt(np.float64(2 * 511 ** 2))), dtype=torch.float64))
    _check(stats, sum_dist, *R.stats_ref(p, t, (1,), 0.95), "512")


def test_two_calls_are_bit_identical():
    for p, t in ([R.discs(2, 256, seed=3)] + [(p, t) for n, p, t in R.zoo(37, 53) if n in ("rings", "checkerboard")]):
        dp, dt = _dev(p, t)
        a = ops().surface_stats(dp, dt, (1, 2, 3))
        b = ops().surface_stats(dp, dt, (1, 2, 3))
        assert torch.equal(a[0], b[0])
        assert torch.equal(a[1].view(torch.int64), b[1].view(torch.int64))


def test_bad_arguments_are_refused_and_launch_nothing():
    from miseg_amd._cabi import MisegError
    p, t = _dev(*R.zoo(24, 40)[6][1:])
    good = ops().surface_stats(p, t, (1, 2, 3))
    with pytest.raises(MisegError, match="workspace too small"):
        ops().surface_stats(p, t, (1, 2, 3), ws=torch.empty(256, dtype=torch.uint8, device=DEV))
    for q in (1.5, -0.1, float("nan")):
        with pytest.raises(MisegError, match="q must lie"):
            ops().surface_stats(p, t, (1, 2, 3), q=q)
    with pytest.raises(MisegError):
        ops().surface_stats(p.cpu(), t.cpu(), (1, 2, 3))
    wide = torch.zeros(1, 8, 520, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match="H, W <= 512"):          # not a RuntimeError, which InferenceEpocher would take for an absent class
        ops().surface_stats(wide, wide, (1,))
    torch.cuda.synchronize()                                       # nothing was launched: no deferred error, and the next call is sound
    again = ops().surface_stats(p, t, (1, 2, 3))
    assert torch.equal(good[0], again[0]) and torch.equal(good[1], again[1])


# ------------------------------------------------------------------------------------------ the meter
METERS = (("hausdorff", "HD"), ("mod_hausdorff", "MHD"), ("average_surface", "ASD"))


def _meter_cases():
    for shape in ((37, 53), (64, 64)):
        for name, p, t in R.zoo(*shape):
            if name in R.FULL:
                yield p, t, [1, 2, 3]
            elif name == "checkerboard":
                yield p, t, [1, 2]


@pytest.mark.parametrize("metername, abbr", METERS)
def test_meter_device_path_equals_host_path(metername, abbr, monkeypatch):
    from deepclustering2.meters2 import SurfaceMeter
    monkeypatch.delenv("MISEG_SURFACE_HOST", raising=False)
    for p, t, axes in _meter_cases():
        dev, host = (SurfaceMeter(C=4, report_axises=axes, metername=metername) for _ in range(2))
        dp, dt = _dev(p, t)
        dev.add(dp, dt)
        host.add(dp.cpu(), dt.cpu())
        got, want = dev._mhd[0], host._mhd[0]
        assert got.shape == want.shape == (3, len(axes)) and got.dtype == np.float64
        if metername == "hausdorff":
            assert np.array_equal(got, want)
        else:                                                      # n <= 4096 border pixels: (n + 2) * 2^-53 < 5e-13
            assert (np.abs(got - want) <= 1e-12 * np.abs(want)).all(), float(np.abs(got - want).max())
        assert dev.summary().keys() == host.summary().keys() and list(dev.summary()) == [f"{abbr}{i}" for i in axes]


def _count_calls(monkeypatch):
    calls, real = [], ops().surface_stats

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)

    monkeypatch.setattr(ops(), "surface_stats", counted)
    return calls


def test_meter_host_switch_and_voxelspacing_take_the_host_path(monkeypatch):
    from deepclustering2.meters2 import SurfaceMeter
    p, t = _dev(*R.zoo(24, 40)[6][1:])
    calls = _count_calls(monkeypatch)
    monkeypatch.delenv("MISEG_SURFACE_HOST", raising=False)
    dev = SurfaceMeter(C=4, report_axises=[1, 2, 3], metername="mod_hausdorff")
    dev.add(p, t)
    assert len(calls) == 1                                         # one launch per batch
    spaced = SurfaceMeter(C=4, report_axises=[1, 2, 3], metername="mod_hausdorff")
    spaced.add(p, t, voxelspacing=(1.0, 1.0))
    assert len(calls) == 1
    monkeypatch.setenv("MISEG_SURFACE_HOST", "1")
    host = SurfaceMeter(C=4, report_axises=[1, 2, 3], metername="mod_hausdorff")
    host.add(p, t)
    assert len(calls) == 1
    assert (np.abs(host._mhd[0] - dev._mhd[0]) <= 1e-12 * host._mhd[0]).all() and np.array_equal(host._mhd[0], spaced._mhd[0])


@pytest.mark.parametrize("metername, abbr", METERS)
def test_meter_absent_class_raises_on_the_device_path(metername, abbr, monkeypatch):
    from deepclustering2.meters2 import SurfaceMeter
    monkeypatch.delenv("MISEG_SURFACE_HOST", raising=False)
    calls = _count_calls(monkeypatch)
    zoo = {name: (p, t) for name, p, t in R.zoo(24, 40)}
    meter = SurfaceMeter(C=4, report_axises=[1, 2, 3], metername=metername)
    meter.add(*_dev(*zoo["rings"]))
    with pytest.raises(RuntimeError):
        meter.add(*_dev(*zoo["missing"]))
    assert len(calls) == 2 and meter._n == 1 and len(meter._mhd) == 1


# ------------------------------------------------------------------------------------------ InferenceEpocher
@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """The 64x64 synthetic set-up of test_gpu_cli.py's inference test: a tiny UNet, one epoch of `partial`, two batches."""
    sys.path.insert(0, PKG)
    from contrastyou.arch import UNet
    from deepclustering2.loss import KL_div
    from semi_seg.synthetic import SyntheticEval, SyntheticPairs
    from semi_seg.trainer import trainer_zoos
    cfg = {"Optim": {"name": "Adam", "lr": 1e-4, "weight_decay": 1e-5},
           "Trainer": {"feature_names": ["Conv5", "Up_conv3", "Up_conv2"], "feature_importance": [1, 0.5, 0.5], "max_epoch": 1}}
    tr = trainer_zoos["partial"](
        model=UNet(input_dim=1, num_classes=4), labeled_loader=iter(SyntheticPairs(2, 64, 4, seed=0)),
        unlabeled_loader=iter(SyntheticPairs(2, 64, 4, seed=1)), val_loader=SyntheticEval(1, 2, 64, 4, seed=2),
        test_loader=SyntheticEval(2, 3, 64, 4, seed=3), sup_criterion=KL_div(), configuration=cfg,
        save_dir=str(tmp_path_factory.mktemp("surface") / "run"), max_epoch=1, num_batches=2, device="cuda")
    tr.init()
    tr.start_training()
    return tr


def test_inference_reports_the_three_surface_metrics(trained, monkeypatch):
    monkeypatch.delenv("MISEG_SURFACE_HOST", raising=False)
    calls = _count_calls(monkeypatch)
    result, score = trained.inference(surface_metrics=("hausdorff", "mod_hausdorff", "average_surface"))
    assert 0.0 <= score <= 1.0 and list(result) == ["loss", "dice", "hd", "mhd", "asd"]
    for key, abbr in (("hd", "HD"), ("mhd", "MHD"), ("asd", "ASD")):
        assert list(result[key]) == [f"{abbr}{i}" for i in (1, 2, 3)]
    assert len(calls) == 2                                         # two batches, one shared launch each
    hd, mhd, asd = (np.array(list(result[k].values())) for k in ("hd", "mhd", "asd"))
    # this barely trained model leaves classes out of its predictions, so a batch may record nothing (NaN), as on the host path;
    # what is recorded is ordered: 0 <= ASD, MHD <= HD.  Values are compared in test_inference_epocher_device_equals_host.
    assert np.array_equal(np.isnan(hd), np.isnan(mhd)) and np.array_equal(np.isnan(hd), np.isnan(asd))
    ok = ~np.isnan(hd)
    assert (mhd[ok] <= hd[ok] + 1e-9).all() and (asd[ok] <= hd[ok] + 1e-9).all() and (asd[ok] >= 0).all()
    # the configuration names them too
    trained._config["Inference"] = {"surface_metrics": ["mod_hausdorff"]}
    try:
        result2, _ = trained.inference()
    finally:
        del trained._config["Inference"]
    assert list(result2) == ["loss", "dice", "mhd"]
    assert np.array_equal(list(result2["mhd"].values()), list(result["mhd"].values()), equal_nan=True)


def test_inference_default_report_is_the_parents(trained, monkeypatch):
    monkeypatch.delenv("MISEG_SURFACE_HOST", raising=False)
    calls = _count_calls(monkeypatch)
    result, _ = trained.inference()
    assert list(result) == ["loss", "dice", "hd"] and list(result["hd"]) == ["HD1", "HD2", "HD3"]
    assert list(result["dice"]) == ["DSC1", "DSC2", "DSC3", "DSC_mean"] and list(result["loss"]) == ["mean"]
    assert len(calls) == 2
    monkeypatch.setenv("MISEG_SURFACE_HOST", "1")
    host, _ = trained.inference()
    assert len(calls) == 2
    assert list(host) == list(result) and result["dice"] == host["dice"]
    assert np.array_equal(list(result["hd"].values()), list(host["hd"].values()), equal_nan=True)


class _Quantiser(torch.nn.Module):
    """Stands in for a trained network: logits that peak at the quartile of the blurred image, so that every class appears in every
    predicted slice as blobs -- the surface meters then record every batch."""
    num_classes = 4

    def forward(self, img):
        z = torch.nn.functional.avg_pool2d(img, 9, stride=1, padding=4, count_include_pad=False)
        lo, hi = z.amin((1, 2, 3), keepdim=True), z.amax((1, 2, 3), keepdim=True)
        centres = torch.tensor([0.125, 0.375, 0.625, 0.875], device=img.device).view(1, 4, 1, 1)
        return -((z - lo) / (hi - lo) - centres) ** 2 * 100


def test_inference_epocher_device_equals_host(tmp_path, monkeypatch):
    sys.path.insert(0, PKG)
    from deepclustering2.loss import KL_div
    from semi_seg.epocher import InferenceEpocher
    from semi_seg.synthetic import SyntheticEval

    def run():
        runner = InferenceEpocher(_Quantiser(), val_loader=SyntheticEval(2, 3, 64, 4, seed=3), sup_criterion=KL_div(), device="cuda",
                                  surface_metrics=("hausdorff", "mod_hausdorff", "average_surface"))
        runner.set_save_dir(str(tmp_path))
        result, _ = runner.run()
        return result, runner.meters

    monkeypatch.delenv("MISEG_SURFACE_HOST", raising=False)
    calls = _count_calls(monkeypatch)
    dev, dev_meters = run()
    assert len(calls) == 2 and all(dev_meters[k]._n == 2 for k in ("hd", "mhd", "asd"))      # both batches recorded, one launch each
    monkeypatch.setenv("MISEG_SURFACE_HOST", "1")
    host, host_meters = run()
    assert len(calls) == 2 and host_meters["hd"]._n == 2
    assert dev["hd"] == host["hd"] and np.isfinite(list(dev["hd"].values())).all() and min(dev["hd"].values()) > 1.0
    for key in ("mhd", "asd"):
        a, b = np.array(list(dev[key].values())), np.array(list(host[key].values()))
        assert np.isfinite(b).all() and (np.abs(a - b) <= 1e-12 * b).all(), (key, a, b)
