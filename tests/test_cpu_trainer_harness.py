"""The comparison functions of tests/trainer_harness.py on tests/golden/entmin.npz -- a flat vector built to carry every fingerprint's
sample exactly, then one tensor scaled, then the offset table shifted by one element -- and its small pure helpers.  No device."""
import json

import numpy as np
import pytest
import torch

import synth
import trainer_harness as th


class _Param:
    """What the comparison functions ask of a parameter: its size (and, for the stub offset table, a name)."""

    def __init__(self, name, shape):
        self.name, self.shape = name, tuple(int(v) for v in shape)

    def numel(self):
        return int(np.prod(self.shape))


def _flat(g, prefix, shift=0):
    """Every ``<prefix>/<name>`` fingerprint of the fixture as noise of its ``shape`` carrying ``sample`` at ``synth.sample_index``, laid
    out one after the other (a gap of three elements between tensors); ``shift`` moves the offset table, not the data."""
    names = sorted({k[len(prefix) + 1:].split("#")[0] for k in g.files if k.startswith(prefix + "/")})
    rng = np.random.RandomState(0)
    named, offsets, parts, at = {}, {}, [rng.standard_normal(3)], 3
    for n in names:
        fp = synth.fp_unpack(g, f"{prefix}/{n}")
        p = _Param(n, fp["shape"])
        body = rng.standard_normal(p.numel())
        body[synth.sample_index(p.numel(), f"{prefix}/{n}")] = fp["sample"]
        named[n], offsets[n] = p, at + shift
        parts += [body, rng.standard_normal(3)]
        at += p.numel() + 3
    return np.concatenate(parts), named, lambda p: offsets[p.name]


@pytest.mark.parametrize("prefix,measure", [("grad_step1", th.sampled_rel_l2), ("param_after", th.sampled_max_abs)])
def test_exact_samples_give_zero_and_a_shifted_offset_table_does_not(golden, prefix, measure):
    g = golden("entmin")
    flat, named, offset_of = _flat(g, prefix)
    assert len(named) >= 4
    assert measure(g, prefix, flat, named, offset_of) == {n: 0.0 for n in named}
    assert measure(g, prefix, torch.from_numpy(flat), named, offset_of) == {n: 0.0 for n in named}
    _, _, shifted = _flat(g, prefix, shift=1)
    errs = measure(g, prefix, flat, named, shifted)
    assert sorted(errs) == sorted(named) and min(errs.values()) > 0.1, min(errs.values())


def test_one_scaled_tensor_shows_in_its_own_relative_error_only(golden):
    g = golden("entmin")
    flat, named, offset_of = _flat(g, "grad_step1")
    victim = sorted(named)[len(named) // 2]
    o = offset_of(named[victim])
    flat[o:o + named[victim].numel()] *= 1 + 1e-3
    errs = th.sampled_rel_l2(g, "grad_step1", flat, named, offset_of)
    assert abs(errs[victim] - 1e-3) < 1e-9, errs[victim]
    assert all(v == 0.0 for n, v in errs.items() if n != victim)


def test_one_scaled_tensor_shows_in_its_own_largest_distance_only(golden):
    g = golden("entmin")
    flat, named, offset_of = _flat(g, "param_after")
    victim = sorted(named)[len(named) // 2]
    o = offset_of(named[victim])
    flat[o:o + named[victim].numel()] *= 1 + 1e-3
    errs = th.sampled_max_abs(g, "param_after", flat, named, offset_of)
    largest = float(np.abs(synth.fp_unpack(g, f"param_after/{victim}")["sample"]).max())
    assert largest > 0 and abs(errs[victim] / largest - 1e-3) < 1e-9, (errs[victim], largest)
    assert all(v == 0.0 for n, v in errs.items() if n != victim)


def test_sampled_reads_the_fingerprints_entries():
    flat = np.arange(100000, dtype=np.float32)
    got = th.sampled(flat, 7, 90000, "some/tag")
    assert got.dtype == np.float64 and np.array_equal(got, 7.0 + synth.sample_index(90000, "some/tag"))
    assert np.array_equal(th.sampled(torch.from_numpy(flat), 2, 5, "t"), [2.0, 3.0, 4.0, 5.0, 6.0])


def test_meter_items_flattens_a_result():
    res = {"sup_loss": {"mean": 0.5}, "sup_dice": {"DSC_mean": np.float32(0.25), "DSC0": 1}, "lr": {}}
    got = th.meter_items(res)
    assert got == {"sup_loss/mean": 0.5, "sup_dice/DSC_mean": 0.25, "sup_dice/DSC0": 1.0}
    assert all(type(v) is float for v in got.values())


def test_golden_cfg_reads_the_cfg_entries(golden):
    g = golden("entmin")
    cfg = th.golden_cfg(g)
    assert cfg and sorted(cfg) == sorted(k[4:] for k in g.files if k.startswith("cfg/"))
    assert all(not isinstance(v, np.ndarray) for v in cfg.values())


def test_own_lines_removed_sorts_what_is_left():
    lines = ["_storage/tra_mi/0 :: float", "_model/w :: tensor float32 [2]", "_optimizer/loss_scaler/scale :: float", "_buffers/x :: int",
             "_storage/tra_minimum :: float"]
    assert th.own_lines_removed(lines, ("_storage/tra_mi/", "_optimizer/loss_scaler/")) == ["_buffers/x :: int", "_model/w :: tensor float32 [2]",
                                                                                         "_storage/tra_minimum :: float"]
    assert th.own_lines_removed(lines, ["_storage/tra_mi"]) == ["_buffers/x :: int", "_model/w :: tensor float32 [2]",
                                                               "_optimizer/loss_scaler/scale :: float"]
    assert th.own_lines_removed(lines, ()) == sorted(lines)


def test_error_dump_writes_prefix_tag_json_only_when_asked(tmp_path, monkeypatch):
    rows = {"b": 1.5, "a": {"loss": 2e-7}}
    monkeypatch.delenv("MISEG_ERROR_DUMP", raising=False)
    monkeypatch.chdir(tmp_path)
    th.error_dump("entmin", "golden_grad", rows)
    assert list(tmp_path.iterdir()) == []
    out = tmp_path / "errors" / "here"
    monkeypatch.setenv("MISEG_ERROR_DUMP", str(out))
    th.error_dump("entmin", "golden_grad", rows)
    th.error_dump("mi_local", "variants", rows, sort_keys=True)
    assert sorted(p.name for p in out.iterdir()) == ["entmin_golden_grad.json", "mi_local_variants.json"]
    assert (out / "entmin_golden_grad.json").read_text() == json.dumps(rows, indent=1)
    assert (out / "mi_local_variants.json").read_text() == json.dumps(rows, indent=1, sort_keys=True)


def test_reference_batches_yield_the_nested_structure_with_independent_clones():
    imgs = [torch.full((2, 1, 4, 4), float(i)) for i in range(3)]
    tgts = [torch.full((2, 1, 4, 4), i, dtype=torch.long) for i in range(3)]
    items = list(th.reference_batches(imgs, tgts, 2))
    assert len(items) == 3
    for i, ((first, second), names, partitions, groups) in enumerate(items):
        assert first[0] is imgs[i] and first[1] is tgts[i]
        assert torch.equal(second[0], imgs[i]) and torch.equal(second[1], tgts[i])
        assert second[0].data_ptr() != imgs[i].data_ptr() and second[1].data_ptr() != tgts[i].data_ptr()
        assert names == ["patient000_00_0", "patient001_00_1"] and partitions == ["0", "0"] and groups == ["patient000_00", "patient001_00"]
    items[0][0][1][0].add_(1.0)
    assert float(imgs[0].max()) == 0.0


def test_tape_assertions_take_their_counts_and_keys_from_the_caller():
    good = th.TapeInfo(replays=4, disabled=None, recorded=True, op_names=["miseg_adam_step"], n_ops=1)
    th.assert_replayed(good, 4)
    for bad in (None, good._replace(disabled="an ATen launch"), good._replace(recorded=False), good._replace(replays=3)):
        with pytest.raises(AssertionError):
            th.assert_replayed(bad, 4)
    a = {"param": torch.arange(4.0), "bn": [torch.ones(2), torch.zeros(2)], "meters": "{'lr': nan}", "skipped": torch.zeros(1)}
    b = {"param": torch.arange(4.0), "bn": [torch.ones(2), torch.zeros(2)], "meters": "{'lr': nan}", "skipped": torch.ones(1)}
    th.assert_same_state(a, b, ("param", "bn", "meters"))
    with pytest.raises(AssertionError):
        th.assert_same_state(a, b, ("param", "skipped"))
    b["bn"][1] = torch.full((2,), 1e-30)
    with pytest.raises(AssertionError):
        th.assert_same_state(a, b, ("bn",))
    with pytest.raises(AssertionError):
        th.assert_same_state(a, dict(b, meters="{'lr': 0.1}"), ("meters",))
