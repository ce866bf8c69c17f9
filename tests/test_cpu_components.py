"""Largest connected component, host side: the two references of tests/component_ref.py against each other, the host twin of
``ops.largest_component`` against the reference, the declaration of ``miseg_largest_component`` in the header, the binding and the
built library, and the argument checks that are made on the host before any launch."""
import ctypes
import re
import subprocess

import numpy as np
import pytest
import torch

import component_ref as R

COMBOS = [(rank, conn) for rank in (2, 3) for conn in (1, 2)]


def _same(a, b, what):
    for x, y, part in zip(a, b, ("out", "labels", "stats")):
        assert x.dtype == y.dtype and np.array_equal(x, y), (what, part)


@pytest.mark.parametrize("shape", R.CPU_SHAPES)
def test_label_reference_equals_flood_fill_on_the_zoo(shape):
    for rank, conn in COMBOS:
        for classes in R.CLASS_LISTS:
            ref = R.zoo_ref(*shape, classes, rank, conn)
            for name, p in R.zoo(*shape):
                _same(ref[name], R.keep_brute(p, classes, rank, conn), (name, rank, conn, classes))


@pytest.mark.parametrize("shape", R.CPU_SHAPES[:3])
def test_the_zoo_holds_what_it_says(shape):
    h, w = shape
    zoo = dict(R.zoo(h, w))
    assert len(zoo) == 13
    ref = {combo: R.zoo_ref(h, w, (1, 2, 3), *combo) for combo in COMBOS}
    for combo in COMBOS:
        out, labels, stats = ref[combo]["empty"]
        assert not out.any() and (labels == -1).all() and not stats.any()
        out, labels, stats = ref[combo]["full"]
        if combo[0] == 2:
            assert np.array_equal(out, zoo["full"]) and stats[..., 1].sum() == stats[..., 2].sum() == 3 * h * w
        else:                                                  # slices 0 and 2 hold class 1, slice 1 lies between: a tie, slice 0 stays
            assert np.array_equal(out[:2], zoo["full"][:2]) and not out[2].any() and stats[0, 0].tolist() == [2, h * w, 2 * h * w]
    # the checkerboard: every pixel its own component under 4-connectivity and all sizes tie, so the first pixel survives
    out, labels, stats = ref[2, 1]["checkerboard"]
    assert (stats[:, :2, 0].sum(1) == h * w).all() and (stats[:, :2, 1] == 1).all() and (out != 0).sum() == 6
    assert out[0, 0, 0] == 1 and out[0, 0, 1] == 2 and out[1, 0, 0] == 2 and out[1, 0, 1] == 1
    out, labels, stats = ref[2, 2]["checkerboard"]
    assert (stats[:, :2, 0] == 1).all() and np.array_equal(out, zoo["checkerboard"])
    # two equal discs: the earlier one stays; of the two squares the later, larger one
    out, labels, stats = ref[2, 1]["equal_discs"]
    assert (stats[:, 0, 0] == 2).all() and (stats[:, 0, 1] * 2 == stats[:, 0, 2]).all()
    ys = np.nonzero(out[0] == 1)[0]
    assert ys.max() < h // 2 + 1 and (out[:, 0:2, w - 2:w] == 0).all() and (out[:, h - 3:h, 0:3] == 2).all()
    # comb and serpentine: one component per slice whatever the connectivity
    for conn in (1, 2):
        assert (ref[2, conn]["comb"][2][:, 0, 0] == 1).all() and (ref[2, conn]["serpentine"][2][..., 0].max() == 1)
    # the diagonal: min(h, w) components under 4, one under 8
    assert (ref[2, 1]["diagonal"][2][:, 0, 0] == min(h, w)).all() and (ref[2, 2]["diagonal"][2][:, 0, 0] == 1).all()
    # across slices: separate for rank 2, joined face to face for rank 3, corner to corner only with the full neighbourhood
    assert ref[2, 1]["across_slices"][2][:, 0, 0].tolist() == [1, 2, 2]
    assert ref[3, 1]["across_slices"][2][0, 0].tolist() == [3, 15, 27] and ref[3, 2]["across_slices"][2][0, 0].tolist() == [2, 15, 27]
    assert (ref[2, 1]["absent"][2][0, 1] == 0).all() and (ref[2, 1]["absent"][2][2, 2] == 0).all()
    for combo in COMBOS:                                       # a value that is not listed is left alone, for either class list
        for classes in R.CLASS_LISTS:
            out = R.zoo_ref(h, w, classes, *combo)["unlisted_value"][0]
            keep = ~np.isin(zoo["unlisted_value"], classes)
            assert np.array_equal(out[keep], zoo["unlisted_value"][keep]) and (zoo["unlisted_value"] == 5).any()


@pytest.mark.parametrize("shape", R.CPU_SHAPES)
def test_host_twin_equals_the_reference(shape, monkeypatch):
    from miseg_amd import ops
    monkeypatch.delenv("MISEG_COMPONENTS_HOST", raising=False)
    for rank, conn in COMBOS:
        for classes in R.CLASS_LISTS:
            ref = R.zoo_ref(*shape, classes, rank, conn)
            for name, p in R.zoo(*shape):
                out, stats, labels = ops.largest_component(torch.from_numpy(p.copy()), classes, volume=rank == 3, connectivity=conn,
                                                           want_labels=True)
                _same(ref[name], (out.numpy(), labels.numpy(), stats.numpy()), (name, rank, conn, classes))


def test_host_twin_dice_counts_fill_and_aliasing():
    from deepclustering2.meters2 import UniversalDice
    from miseg_amd import ops
    zoo = dict(R.zoo(24, 40))
    pred, target = torch.from_numpy(zoo["noise"].copy()), torch.from_numpy(zoo["rings"].copy())
    out, stats, (inter, uni) = ops.largest_component(pred, (1, 2, 3), target=target, num_classes=4)
    meter = UniversalDice(4, report_axises=[1, 2, 3])
    meter.add(out, target)
    assert torch.equal(inter, meter._intersections[0]) and torch.equal(uni, meter._unions[0])
    # fill: what is dropped becomes the fill value; out may be pred
    ref = R.keep_ref(zoo["noise"], (1, 2), 2, 2, fill=7)
    work = pred.clone()
    res = ops.largest_component(work, (1, 2), connectivity=2, fill=7, out=work)
    assert res[0] is work and np.array_equal(work.numpy(), ref[0]) and np.array_equal(res[1].numpy(), ref[2])
    # a target value outside [0, C) counts in nothing
    bad = target.clone()
    bad[0, 0, :5] = 9
    _, _, (inter2, uni2) = ops.largest_component(pred, (1, 2, 3), target=bad, num_classes=4)
    o, t = out[0, 0, :5], target[0, 0, :5]
    assert int(uni.sum() - uni2.sum()) == 5 and int(inter.sum() - inter2.sum()) == int((o == t).sum())


def test_component_symbols_are_declared_and_exported():
    from miseg_amd import _cabi
    header = re.sub(r"/\*.*?\*/", " ", open(_cabi.HEADER).read(), flags=re.S)
    for name, nargs in (("miseg_largest_component", 19), ("miseg_largest_component_ws_bytes", 5)):
        m = re.search(r"\b%s\s*\(([^;{]*?)\)\s*;" % name, header, flags=re.S)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert len(_cabi.PROTOTYPES[name][1]) == nargs, name
    proto = _cabi.PROTOTYPES["miseg_largest_component"][1]
    assert proto[7] is ctypes.c_int and proto[8] is ctypes.c_int and proto[9] is ctypes.c_int64 and proto[14] is ctypes.c_int64
    assert _cabi.PROTOTYPES["miseg_largest_component_ws_bytes"][0] is ctypes.c_int64
    exported = subprocess.run(["nm", "-D", "--defined-only", _cabi.LIB_PATH], check=True, capture_output=True, text=True).stdout
    names = {line.split()[-1] for line in exported.splitlines() if line.strip()}
    assert {"miseg_largest_component", "miseg_largest_component_ws_bytes"} <= names
    assert _cabi.lib().miseg_version() >= 413


def test_workspace_query():
    from miseg_amd import _cabi
    q = _cabi.lib().miseg_largest_component_ws_bytes
    small, large = q(1, 8, 8, 1, 2), q(16, 256, 256, 3, 2)
    assert 0 < small < large and large >= 16 * 256 * 256 * 8
    assert q(1, 2048, 2048, 64, 3) > 0
    for bad in ((1, 4096, 8, 1, 2), (1, 8, 2049, 1, 2), (0, 8, 8, 1, 2), (1, 0, 8, 1, 2), (1, 8, 8, 0, 2), (1, 8, 8, 65, 2),
                (1, 8, 8, 1, 1), (1, 8, 8, 1, 4), (512, 2048, 2048, 1, 2)):
        assert q(*bad) == -1, bad                               # refused, not rounded


def test_entry_point_refuses_bad_arguments_before_any_launch():
    """Every case fails a host check that precedes the first launch, so the made-up addresses are never used."""
    from miseg_amd import _cabi
    from miseg_amd._cabi import MisegError
    ws_bytes = _cabi.lib().miseg_largest_component_ws_bytes(2, 16, 16, 3, 2)
    P = 4096                                                   # stands for "not null"
    good = dict(stream=None, pred=P, N=2, H=16, W=16, classes=P, K=3, rank=2, conn=1, fill=0, out=P, labels=None, stats=P, target=None,
                C=0, inter=None, uni=None, ws=P, ws_bytes=ws_bytes)
    cases = [({"pred": None}, "null pointer"), ({"classes": None}, "null pointer"), ({"out": None}, "null pointer"),
             ({"stats": None}, "null pointer"), ({"ws": None}, "null pointer"),
             ({"rank": 1}, "rank"), ({"rank": 4}, "rank"), ({"conn": 0}, "connectivity"), ({"conn": 3}, "connectivity"),
             ({"H": 4096}, "bad shape"), ({"W": 4096}, "bad shape"), ({"N": 0}, "bad shape"), ({"K": 0}, "bad shape"),
             ({"K": 65}, "bad shape"), ({"fill": 64}, "fill"), ({"fill": -1}, "fill"),
             ({"target": P, "C": 4}, "inter / uni"), ({"target": P, "inter": P, "uni": P, "C": 65}, "class count"),
             ({"target": P, "inter": P, "uni": P, "C": 0}, "class count"),
             ({"ws_bytes": ws_bytes - 1}, "workspace too small"), ({"ws_bytes": 0}, "workspace too small")]
    for change, message in cases:
        with pytest.raises(MisegError, match=message):
            _cabi.call("miseg_largest_component", *{**good, **change}.values())


def test_op_raises_value_errors(monkeypatch):
    from miseg_amd import ops
    pred = torch.zeros(2, 16, 16, dtype=torch.int64)
    monkeypatch.setenv("MISEG_COMPONENTS_HOST", "0")           # the host path switched off: CPU tensors are refused
    with pytest.raises(ValueError, match="CPU tensors"):
        ops.largest_component(pred, (1, 2, 3))
    monkeypatch.delenv("MISEG_COMPONENTS_HOST")
    for kwargs, message in (({"classes": (0, 1)}, "fill"), ({"classes": (1, 2), "fill": 2}, "fill"), ({"classes": (1, 2, 1)}, "duplicate"),
                            ({"classes": (1, 64)}, "classes"), ({"classes": (-1,)}, "classes"), ({"classes": ()}, "classes"),
                            ({"classes": (1,), "fill": 64}, "fill"), ({"classes": (1,), "connectivity": 0}, "connectivity"),
                            ({"classes": (1,), "connectivity": 3}, "connectivity"),
                            ({"classes": (1,), "target": pred}, "num_classes"),
                            ({"classes": (1,), "target": pred[:1], "num_classes": 4}, "target")):
        with pytest.raises(ValueError, match=message):
            ops.largest_component(pred, **kwargs)
    for bad in (pred.int(), pred.float(), pred[0], pred[None], torch.zeros(1, 8, 2049, dtype=torch.int64),
                torch.zeros(1, 2049, 8, dtype=torch.int64)):
        with pytest.raises(ValueError, match="largest_component"):
            ops.largest_component(bad, (1,))


class _Net(torch.nn.Module):
    num_classes = 4

    def forward(self, img):
        return img


def test_inference_epocher_default_meters_are_unchanged():
    from deepclustering2.loss import KL_div
    from deepclustering2.meters2 import MeterInterface
    from semi_seg.epocher import InferenceEpocher
    default = InferenceEpocher(_Net(), val_loader=[], sup_criterion=KL_div(), device="cpu")
    assert list(default._configure_meters(MeterInterface()).meters) == ["loss", "dice", "hd"]
    both = InferenceEpocher(_Net(), val_loader=[], sup_criterion=KL_div(), device="cpu", surface_metrics=("hausdorff", "average_surface"),
                            keep_largest=True, component_connectivity=2)
    assert list(both._configure_meters(MeterInterface()).meters) == ["loss", "dice", "hd", "asd", "dice_lcc", "hd_lcc", "asd_lcc"]
    with pytest.raises(AssertionError):
        InferenceEpocher(_Net(), val_loader=[], sup_criterion=KL_div(), device="cpu", keep_largest=True, component_connectivity=3)


def test_write_prediction_map(tmp_path):
    from PIL import Image

    from contrastyou.epocher._utils import write_prediction_map
    maps = torch.from_numpy(dict(R.zoo(24, 40))["rings"].copy())
    write_prediction_map(maps, str(tmp_path), ["a", "b", "c"], "pred_lcc")
    for m, f in zip(maps, "abc"):
        assert np.array_equal(np.asarray(Image.open(tmp_path / "pred_lcc" / f"{f}.png")), m.numpy().astype(np.uint8))
