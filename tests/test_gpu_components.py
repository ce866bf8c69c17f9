"""``miseg_largest_component`` against the host reference of tests/component_ref.py (``scipy.ndimage.label`` + ``bincount``), bit for
bit: everything here is an integer, every comparison is ``torch.equal`` with a host result, never with the code under test."""
import os
import sys

import numpy as np
import pytest
import torch

import component_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mi-based-regularized-semi-supervised-segmentation_amd")
COMBOS = [(rank, conn) for rank in (2, 3) for conn in (1, 2)]


def ops():
    from miseg_amd import ops as _ops
    return _ops


@pytest.fixture(autouse=True)
def _device_path(monkeypatch):
    monkeypatch.delenv("MISEG_COMPONENTS_HOST", raising=False)


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def _check(got, want, what):
    """got = (out, stats, labels) of the op; want = (out, labels, stats) of the reference."""
    out, stats, labels = got
    assert out.dtype == torch.int64 and stats.dtype == torch.int64 and labels.dtype == torch.int32
    assert torch.equal(stats.cpu(), torch.from_numpy(want[2])), (what, "stats", stats.cpu().tolist(), want[2].tolist())
    assert torch.equal(labels.cpu(), torch.from_numpy(want[1])), (what, "labels", int((labels.cpu().numpy() != want[1]).sum()))
    assert torch.equal(out.cpu(), torch.from_numpy(want[0])), (what, "out", int((out.cpu().numpy() != want[0]).sum()))


@pytest.mark.parametrize("classes", R.CLASS_LISTS)
@pytest.mark.parametrize("shape", R.GPU_SHAPES)
def test_kernel_equals_the_reference_on_the_zoo(shape, classes):
    for name, p in R.zoo(*shape):
        dp = _dev(p)
        for rank, conn in COMBOS:
            got = ops().largest_component(dp, classes, volume=rank == 3, connectivity=conn, want_labels=True)
            assert got[1].shape == (1 if rank == 3 else 3, len(classes), 3)
            _check(got, R.zoo_ref(*shape, classes, rank, conn)[name], (name, rank, conn))
    assert torch.equal(dp.cpu(), torch.from_numpy(np.array(p)))        # the input is left alone


def test_kernel_on_the_long_spiral_512():
    """The long chain: one component of ~131 000 pixels that winds through every 64 x 64 tile of the slice 32 times."""
    p, length = R.spiral(512)
    want = R.keep_ref(p, (1,), 2, 1)
    assert want[2].tolist() == [[[2, length, length + 9]]] and not want[0][0, 255:258, 255:258].any()
    got = ops().largest_component(_dev(p), (1,), want_labels=True)
    _check(got, want, "spiral")
    assert int(got[0].sum()) == length


def test_kernel_on_random_discs_256():
    import surface_ref
    p, t = surface_ref.discs(2, 256, seed=11)
    for m in (p, t):
        for rank, conn in COMBOS:
            got = ops().largest_component(_dev(m), (1, 2, 3), volume=rank == 3, connectivity=conn, want_labels=True)
            _check(got, R.keep_ref(m, (1, 2, 3), rank, conn), (rank, conn))


def test_dice_counts_equal_the_meters():
    from deepclustering2.meters2 import UniversalDice
    zoo = dict(R.zoo(65, 130))
    for pname, tname in (("noise", "rings"), ("rings", "unlisted_value"), ("equal_discs", "equal_discs")):
        p, t = _dev(zoo[pname]), _dev(zoo[tname])
        t = torch.where(t == 5, torch.zeros_like(t), t)               # class2one_hot takes values in [0, C) only
        for rank, conn in COMBOS:
            out, stats, (inter, uni) = ops().largest_component(p, (1, 2, 3), volume=rank == 3, connectivity=conn, target=t, num_classes=4)
            assert torch.equal(out.cpu(), torch.from_numpy(R.zoo_ref(65, 130, (1, 2, 3), rank, conn)[pname][0]))
            meter = UniversalDice(4, report_axises=[1, 2, 3])
            meter.add(out.cpu(), t.cpu())
            assert inter.dtype == torch.int64 and inter.shape == (3, 4)
            assert torch.equal(inter.cpu(), meter._intersections[0]) and torch.equal(uni.cpu(), meter._unions[0]), (pname, rank, conn)
    # values outside [0, C) count in nothing: C = 2 with classes 2, 3 (and 5) in the maps
    p, t = _dev(zoo["unlisted_value"]), _dev(zoo["rings"])
    out, _, (inter, uni) = ops().largest_component(p, (1, 2, 3), target=t, num_classes=2)
    o, tt = out.cpu(), t.cpu()
    want_i = torch.stack([((o == c) & (tt == c)).sum((1, 2)) for c in range(2)], 1)
    want_u = torch.stack([(o == c).sum((1, 2)) + (tt == c).sum((1, 2)) for c in range(2)], 1)
    assert torch.equal(inter.cpu(), want_i) and torch.equal(uni.cpu(), want_u)


def test_out_may_alias_pred_and_fill_is_honoured():
    zoo = dict(R.zoo(65, 130))
    for name in ("noise", "checkerboard", "equal_discs"):
        for rank, conn in COMBOS:
            work = _dev(zoo[name])
            res = ops().largest_component(work, (1, 2), volume=rank == 3, connectivity=conn, fill=7, want_labels=True, out=work)
            assert res[0] is work
            _check(res, R.keep_ref(zoo[name], (1, 2), rank, conn, fill=7), (name, rank, conn))


def test_two_calls_are_bit_identical():
    zoo = dict(R.zoo(130, 67))
    for name in ("noise", "checkerboard"):
        p, t = _dev(zoo[name]), _dev(zoo["rings"])
        for rank, conn in COMBOS:
            a = ops().largest_component(p, (1, 2, 3), volume=rank == 3, connectivity=conn, target=t, num_classes=4, want_labels=True)
            b = ops().largest_component(p, (1, 2, 3), volume=rank == 3, connectivity=conn, target=t, num_classes=4, want_labels=True)
            for x, y in zip(a[:3] + a[3], b[:3] + b[3]):
                assert torch.equal(x, y), (name, rank, conn)


def test_device_equals_host_twin(monkeypatch):
    zoo = dict(R.zoo(37, 53))
    for name in ("noise", "rings", "across_slices", "unlisted_value"):
        p, t = _dev(zoo[name]), _dev(zoo["rings"])
        for rank, conn in COMBOS:
            kw = dict(volume=rank == 3, connectivity=conn, target=t, num_classes=4, want_labels=True)
            dev = ops().largest_component(p, (3, 1), **kw)
            host = ops().largest_component(p.cpu(), (3, 1), **{**kw, "target": t.cpu()})
            monkeypatch.setenv("MISEG_COMPONENTS_HOST", "1")
            forced = ops().largest_component(p, (3, 1), **kw)           # device tensors through the host path
            monkeypatch.delenv("MISEG_COMPONENTS_HOST")
            for x, y, z in zip(dev[:3] + dev[3], host[:3] + host[3], forced[:3] + forced[3]):
                assert x.is_cuda and not y.is_cuda and z.is_cuda and x.dtype == y.dtype == z.dtype
                assert torch.equal(x.cpu(), y) and torch.equal(z.cpu(), y), (name, rank, conn)


def test_bad_arguments_are_refused_and_launch_nothing():
    from miseg_amd._cabi import MisegError
    p = _dev(dict(R.zoo(24, 40))["rings"])
    good = ops().largest_component(p, (1, 2, 3))
    with pytest.raises(MisegError, match="workspace too small"):
        ops().largest_component(p, (1, 2, 3), ws=torch.empty(256, dtype=torch.uint8, device=DEV))
    for kwargs in ({"classes": (0, 1)}, {"classes": (1, 1)}, {"classes": (1,), "connectivity": 3}, {"classes": (64,)}):
        with pytest.raises(ValueError):
            ops().largest_component(p, **kwargs)
    with pytest.raises(ValueError, match="2048"):
        ops().largest_component(torch.zeros(1, 8, 2049, dtype=torch.int64, device=DEV), (1,))
    torch.cuda.synchronize()                                           # nothing was launched: the next call is sound
    again = ops().largest_component(p, (1, 2, 3))
    assert torch.equal(good[0], again[0]) and torch.equal(good[1], again[1])


# ------------------------------------------------------------------------------------------ InferenceEpocher
class _Decoder(torch.nn.Module):
    """Stands in for a trained network: the image holds the wanted prediction as class / 4, the logits peak at that class."""
    num_classes = 4

    def forward(self, img):
        centres = torch.arange(4, device=img.device, dtype=img.dtype).view(1, 4, 1, 1)
        return -((img * 4 - centres) ** 2) * 100


class _Loader:
    """Two batches of three 64 x 64 slices: per class one large rectangle and one stray pixel far from it; the target holds the
    rectangles, moved by a pixel."""

    def __init__(self):
        self.pred, self.target, self._batches = [], [], []
        for b in range(2):
            p, t = np.zeros((3, 64, 64), np.int64), np.zeros((3, 64, 64), np.int64)
            for s in range(3):
                d = b + s
                p[s, 5 + d:20 + d, 5:20], t[s, 6 + d:21 + d, 5:21] = 1, 1
                p[s, 5:20, 30 + d:50], t[s, 5:20, 31 + d:50] = 2, 2
                p[s, 30:50 - d, 10:40], t[s, 31:50 - d, 10:41] = 3, 3
                p[s, 60, 60 - d], p[s, 62, 2 + d], p[s, 1 + d, 62] = 1, 2, 3
            self.pred.append(p)
            self.target.append(t)
            names = [f"patient{b:03d}_00_{s:02d}" for s in range(3)]
            self._batches.append([[torch.from_numpy(p).float().unsqueeze(1) / 4, torch.from_numpy(t).unsqueeze(1)], names, ["0"] * 3,
                                  [f"patient{b:03d}_00"] * 3])

    def __len__(self):
        return len(self._batches)

    def __iter__(self):
        return iter(self._batches)


def _run_epocher(save_dir, **kwargs):
    sys.path.insert(0, PKG)
    from deepclustering2.loss import KL_div
    from semi_seg.epocher import InferenceEpocher
    loader = _Loader()
    runner = InferenceEpocher(_Decoder(), val_loader=loader, sup_criterion=KL_div(), device="cuda", **kwargs)
    runner.set_save_dir(str(save_dir))
    result, score = runner.run()
    return loader, result, score


def test_inference_epocher_keeps_the_largest_component(tmp_path):
    from PIL import Image

    from deepclustering2.meters2.meters import hausdorff_distance
    loader, plain, plain_score = _run_epocher(tmp_path / "plain")
    assert list(plain) == ["loss", "dice", "hd"] and not (tmp_path / "plain" / "pred_lcc").exists()
    assert sorted(os.listdir(tmp_path / "plain")) == ["gt", "img", "pred"]
    _, result, score = _run_epocher(tmp_path / "lcc", keep_largest=True)
    assert list(result) == ["loss", "dice", "hd", "dice_lcc", "hd_lcc"]
    for key in ("loss", "dice", "hd"):                                 # the old keys with the old values
        assert result[key] == plain[key], key
    assert score == plain_score == result["dice"]["DSC_mean"]
    assert list(result["dice_lcc"]) == list(result["dice"]) and list(result["hd_lcc"]) == list(result["hd"])
    assert all(result["dice_lcc"][k] >= result["dice"][k] for k in result["dice"])
    assert result["dice_lcc"]["DSC_mean"] > result["dice"]["DSC_mean"]
    cleaned = [R.keep_ref(p, (1, 2, 3), 2, 1)[0] for p in loader.pred]

    def host_hd(maps):                                                 # [6 slices, 3 classes] -> the meter's mean over slices
        return np.array([[hausdorff_distance(m[s] == c, t[s] == c) for c in (1, 2, 3)]
                         for m, t in zip(maps, loader.target) for s in range(3)]).mean(0)

    want, raw = host_hd(cleaned), host_hd(loader.pred)
    for k, c in enumerate((1, 2, 3)):
        assert result["hd_lcc"][f"HD{c}"] == want[k] and result["hd"][f"HD{c}"] == raw[k] and want[k] < raw[k], (c, want, raw)
    files = sorted(os.listdir(tmp_path / "lcc" / "pred_lcc"))
    assert files == sorted(os.listdir(tmp_path / "lcc" / "pred")) and len(files) == 6
    for b in range(2):
        for s in range(3):
            name = f"patient{b:03d}_00_{s:02d}.png"
            assert np.array_equal(np.asarray(Image.open(tmp_path / "lcc" / "pred_lcc" / name)), cleaned[b][s].astype(np.uint8))
            assert np.array_equal(np.asarray(Image.open(tmp_path / "lcc" / "pred" / name)), loader.pred[b][s].astype(np.uint8))


def test_inference_epocher_with_three_surface_meters_and_8_connectivity(tmp_path):
    _, result, _ = _run_epocher(tmp_path, keep_largest=True, component_connectivity=2,
                                surface_metrics=("hausdorff", "mod_hausdorff", "average_surface"))
    assert list(result) == ["loss", "dice", "hd", "mhd", "asd", "dice_lcc", "hd_lcc", "mhd_lcc", "asd_lcc"]
    for key in ("hd", "asd"):                                          # the stray pixel is the maximum and raises the mean
        assert all(result[key + "_lcc"][k] < result[key][k] for k in result[key]), key
    assert all(result["mhd_lcc"][k] <= result["mhd"][k] for k in result["mhd"])      # a percentile without the maximum is no larger


def test_trainer_inference_reaches_the_epocher(tmp_path, monkeypatch):
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
        test_loader=SyntheticEval(1, 2, 64, 4, seed=3), sup_criterion=KL_div(), configuration=cfg,
        save_dir=str(tmp_path / "run"), max_epoch=1, num_batches=2, device="cuda")
    tr.init()
    tr.to("cuda")
    tr._save_to("best.pth")                                            # an untrained checkpoint: inference only has to load one
    seen, real = [], ops().largest_component

    def recorded(*a, **k):
        seen.append(k.get("connectivity"))
        return real(*a, **k)

    monkeypatch.setattr(ops(), "largest_component", recorded)
    result, score = tr.inference()
    assert list(result) == ["loss", "dice", "hd"] and not seen and not (tmp_path / "run" / "pred_lcc").exists()
    result, score2 = tr.inference(keep_largest=True)
    assert list(result) == ["loss", "dice", "hd", "dice_lcc", "hd_lcc"] and seen == [1] and score2 == score
    assert len(os.listdir(tmp_path / "run" / "pred_lcc")) == 2
    tr._config["Inference"] = {"keep_largest_component": True, "component_connectivity": 2}
    try:
        result, _ = tr.inference()
        assert list(result) == ["loss", "dice", "hd", "dice_lcc", "hd_lcc"] and seen == [1, 2]
        result, _ = tr.inference(keep_largest=False)                   # the argument wins over the configuration
        assert list(result) == ["loss", "dice", "hd"] and seen == [1, 2]
    finally:
        del tr._config["Inference"]
