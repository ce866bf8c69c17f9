"""Surface distances, host side: the two references of tests/surface_ref.py against each other, ``SurfaceMeter``'s three metrics on
CPU tensors against numpy, and the declaration of ``miseg_surface_stats`` in the header, the binding and the built library."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import surface_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = (1, 2, 3)


@pytest.mark.parametrize("shape", R.SHAPES)
def test_edt_reference_equals_brute_force_on_the_zoo(shape):
    for name, p, t in R.zoo(*shape):
        ref, brute = R.zoo_distances(*shape, CLASSES)[name], R.distances_brute(p, t, CLASSES)
        assert ref.keys() == brute.keys()
        for key in ref:
            assert (ref[key] is None) == (brute[key] is None), (name, key)
            if ref[key] is not None:
                assert np.array_equal(ref[key], brute[key]), (name, key)
        for q in (0.95, 0.0, 1.0, 0.5):
            a, b = R.stats_from(ref, 3, 3, q), R.stats_from(brute, 3, 3, q)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (name, q)


@pytest.mark.parametrize("shape", R.SHAPES)
def test_the_zoo_holds_what_it_says(shape):
    h, w = shape
    zoo = {name: (p, t) for name, p, t in R.zoo(h, w)}
    assert len(zoo) == 8
    for name in R.FULL:                                           # classes 1..3 in every slice of both masks
        for m in zoo[name]:
            assert all((m[b] == c).any() for b in range(3) for c in CLASSES), name
    stats, sums = R.stats_from(R.zoo_distances(h, w, CLASSES)["same"], 3, 3, 0.95)
    assert (stats[..., 0] > 0).all() and (stats[..., 1:] == 0).all() and (sums == 0).all()
    stats, _ = R.stats_from(R.zoo_distances(h, w, CLASSES)["missing"], 3, 3, 0.95)
    assert (stats[0, 1] == 0).all() and (stats[2, 2] == 0).all() and (stats[1, :, :, 0] > 0).all() and (stats[0, 0, :, 0] > 0).all()
    stats, _ = R.stats_from(R.zoo_distances(h, w, CLASSES)["full"], 3, 3, 0.95)
    assert (stats[:, 0, 0, 0] == 2 * (h + w) - 4).all() and (stats[:, 1:] == 0).all()       # the frame; classes 2, 3 absent from pred
    stats, _ = R.stats_from(R.zoo_distances(h, w, CLASSES)["checkerboard"], 3, 3, 0.95)
    assert stats[:, :2, :, 0].sum() == 3 * 2 * h * w                                         # every pixel is a border pixel
    stats, _ = R.stats_from(R.zoo_distances(h, w, CLASSES)["corners"], 3, 3, 1.0)
    assert (stats[..., 0] == 1).all() and stats[..., 1].max() == (h - 1) ** 2 + (w - 1) ** 2


def _directed(p, t):
    from deepclustering2.meters2.meters import _surface_distances
    return _surface_distances(p, t, None, 1), _surface_distances(t, p, None, 1)


@pytest.mark.parametrize("metername, abbr", [("mod_hausdorff", "MHD"), ("average_surface", "ASD"), ("hausdorff", "HD")])
def test_surface_meter_on_cpu_tensors(metername, abbr):
    from deepclustering2.meters2 import SurfaceMeter
    from deepclustering2.meters2.meters import hausdorff_distance
    meter = SurfaceMeter(C=4, report_axises=[1, 2, 3], metername=metername)
    assert meter.get_plot_names() == [f"{abbr}{i}" for i in (1, 2, 3)]
    want = []
    for shape in ((24, 40), (37, 53)):
        for name, p, t in R.zoo(*shape):
            if name not in R.FULL:
                continue
            meter.add(torch.from_numpy(p.copy()), torch.from_numpy(t.copy()))
            for b in range(3):
                row = []
                for c in CLASSES:
                    d0, d1 = _directed(p[b] == c, t[b] == c)
                    if metername == "mod_hausdorff":
                        row.append(max(np.percentile(d0, 95), np.percentile(d1, 95)))
                    elif metername == "average_surface":
                        row.append((d0.mean() + d1.mean()) / 2)
                    else:
                        row.append(hausdorff_distance(p[b] == c, t[b] == c))
                want.append(row)
    got, want = np.concatenate(meter._mhd, 0), np.asarray(want)
    assert got.shape == want.shape == (24, 3)
    if metername == "hausdorff":
        assert np.array_equal(got, want)                                    # unchanged, bit for bit
    else:
        assert np.abs(got - want).max() <= 1e-12, np.abs(got - want).max()
    summary = meter.summary()
    assert list(summary) == [f"{abbr}{i}" for i in (1, 2, 3)]
    assert abs(summary[f"{abbr}2"] - want[:, 1].mean()) <= 1e-12 and meter.detailed_summary() == summary


@pytest.mark.parametrize("metername", ["mod_hausdorff", "average_surface", "hausdorff"])
def test_an_absent_class_raises_and_records_nothing(metername):
    from deepclustering2.meters2 import SurfaceMeter
    meter = SurfaceMeter(C=4, report_axises=[1, 2, 3], metername=metername)
    zoo = {name: (p, t) for name, p, t in R.zoo(24, 40)}
    meter.add(*(torch.from_numpy(m.copy()) for m in zoo["rings"]))
    assert meter._n == 1
    with pytest.raises(RuntimeError):
        meter.add(*(torch.from_numpy(m.copy()) for m in zoo["missing"]))
    assert meter._n == 1 and len(meter._mhd) == 1


def test_unknown_meter_name_is_refused():
    from deepclustering2.meters2 import SurfaceMeter
    with pytest.raises(AssertionError):
        SurfaceMeter(C=4, metername="dice")


def test_numpy_percentile_from_its_two_neighbours():
    """The host half of the device path: numpy's linear percentile rebuilt from the squares of rank floor(v) and ceil(v)."""
    from deepclustering2.meters2.meters import _lerp_sqrt
    rng = np.random.default_rng(5)
    for n in (1, 2, 3, 7, 20, 21, 100, 4096):
        sq = np.sort(rng.integers(0, 5000, n))
        for q in (0.95, 0.5, 0.0, 1.0):
            v = (n - 1) * q
            got = _lerp_sqrt(n, sq[int(np.floor(v))], sq[int(np.ceil(v))], q)
            want = np.percentile(np.sqrt(sq.astype(np.float64)), 100 * q)
            assert abs(got - want) <= 1e-12 * max(want, 1.0), (n, q, got, want)


def test_surface_symbols_are_declared_and_exported():
    from miseg_amd import _cabi
    header = re.sub(r"/\*.*?\*/", " ", open(_cabi.HEADER).read(), flags=re.S)
    for name, nargs in (("miseg_surface_stats", 13), ("miseg_surface_stats_ws_bytes", 4)):
        m = re.search(r"\b%s\s*\(([^;{]*?)\)\s*;" % name, header, flags=re.S)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert len(_cabi.PROTOTYPES[name][1]) == nargs, name
    import ctypes
    assert _cabi.PROTOTYPES["miseg_surface_stats"][1][8] is ctypes.c_double and _cabi.PROTOTYPES["miseg_surface_stats_ws_bytes"][0] is ctypes.c_int64
    exported = subprocess.run(["nm", "-D", "--defined-only", _cabi.LIB_PATH], check=True, capture_output=True, text=True).stdout
    names = {line.split()[-1] for line in exported.splitlines() if line.strip()}
    assert {"miseg_surface_stats", "miseg_surface_stats_ws_bytes"} <= names


def test_library_version_and_workspace_query():
    from miseg_amd import _cabi
    lib = _cabi.lib()
    assert lib.miseg_version() >= 410
    small, large = lib.miseg_surface_stats_ws_bytes(1, 8, 8, 1), lib.miseg_surface_stats_ws_bytes(16, 256, 256, 3)
    assert 0 < small < large and large >= 16 * 3 * 2 * 256 * 256 * 6
    assert lib.miseg_surface_stats_ws_bytes(1, 513, 8, 1) < 0 and lib.miseg_surface_stats_ws_bytes(1, 8, 8, 0) < 0     # refused, not rounded
