"""Structure of semi_seg/epocher.py and semi_seg/trainer.py that every trainer shares, on the CPU: the meter table (names and order
are the columns of storage.csv), what ``_record`` feeds, the one supervised-loss and the one consistency-loss function, and the two
refusals of the trainers.  Every expected name, order and message is a literal here."""
import types

import pytest
import torch

BASE = ["lr", "sup_loss", "reg_loss", "sup_dice"]
FEATURES = ["Conv5", "Up_conv3"]
METER_TABLE = {
    "EvalEpocher": ["loss", "dice"],
    "InferenceEpocher": ["loss", "dice", "hd", "asd", "dice_lcc", "hd_lcc", "asd_lcc"],
    "TrainEpocher": BASE,
    "UDATrainEpocher": BASE + ["uda"],
    "IICTrainEpocher": BASE + ["mi", "individual_mis"],
    "UDAIICEpocher": BASE + ["mi", "individual_mis", "uda", "iic_weight", "uda_weight"],
    "MeanTeacherEpocher": BASE + ["reg_weight"],
    "VATEpocher": BASE + ["reg_weight"],
    "MIDLTrainEpocher": BASE + ["uda", "mi"],
    "EntropyMinEpocher": BASE + ["entropy"],
    "PretrainEncoderEpocher": ["contrastive_loss", "lr"],
    "PretrainDecoderEpocher": ["contrastive_loss", "lr"],
}


def _bare(name):
    """An epocher with only what ``_configure_meters`` and ``_record`` read."""
    from deepclustering2.meters2 import MeterInterface
    from semi_seg import epocher as E
    ep = object.__new__(getattr(E, name))
    ep._model = types.SimpleNamespace(num_classes=4)
    ep._feature_position = list(FEATURES)
    ep._surface_metrics, ep._keep_largest = ("hausdorff", "average_surface"), True
    ep._iic_weight, ep._cons_weight, ep._reg_weight = 0.125, 5.0, 2.0
    ep.meters = ep._configure_meters(MeterInterface())
    return ep


@pytest.mark.parametrize("name", sorted(METER_TABLE))
def test_meter_names_and_order(name):
    from deepclustering2.meters2 import AverageValueMeter, MultipleAverageValueMeter, SurfaceMeter, UniversalDice
    meters = _bare(name).meters
    assert meters.meter_names == METER_TABLE[name]
    special = {"sup_dice": UniversalDice, "dice": UniversalDice, "dice_lcc": UniversalDice, "individual_mis": MultipleAverageValueMeter,
               "hd": SurfaceMeter, "asd": SurfaceMeter, "hd_lcc": SurfaceMeter, "asd_lcc": SurfaceMeter}
    for meter_name in meters.meter_names:
        assert type(meters[meter_name]) is special.get(meter_name, AverageValueMeter), meter_name
    for dice in ("sup_dice", "dice", "dice_lcc"):
        if dice in meters.meter_names:
            assert meters[dice]._C == 4 and meters[dice]._report_axis == [1, 2, 3]


HOST_KEYS = {      # the host values a trainer's iteration reports besides sup_loss and reg_loss -> the meter each one feeds
    "TrainEpocher": {}, "MeanTeacherEpocher": {}, "VATEpocher": {},
    "UDATrainEpocher": {"uda": "uda"},
    "IICTrainEpocher": {"mi": "mi"},
    "UDAIICEpocher": {"mi": "mi", "uda": "uda"},
    "MIDLTrainEpocher": {"uda": "uda", "mi": "mi"},
    "EntropyMinEpocher": {"entropy": "entropy"},
}


def _counts():
    return torch.tensor([[3, 1, 0, 2], [1, 1, 1, 1]]), torch.tensor([[9, 4, 2, 5], [4, 4, 4, 4]])


@pytest.mark.parametrize("name", sorted(HOST_KEYS))
def test_record_feeds_every_host_value_to_its_meter(name):
    ep = _bare(name)
    host = {"sup_loss": 0.75, "reg_loss": 0.5}
    host.update({key: 0.0625 * (i + 1) for i, key in enumerate(HOST_KEYS[name])})
    taps = name in ("IICTrainEpocher", "UDAIICEpocher")
    if taps:
        host.update({"mi/Conv5": 1.5, "mi/Up_conv3": 2.5})
    inter, union = _counts()
    ep._record(host, inter, union, ["p0", "p1"])
    fed = {"sup_loss": 0.75, "reg_loss": 0.5, **{meter: host[key] for key, meter in HOST_KEYS[name].items()}}
    for meter, value in fed.items():
        assert (ep.meters[meter].n, ep.meters[meter].sum) == (1, value), meter
    dice = ep.meters["sup_dice"]
    assert torch.equal(dice._intersections[0], inter) and torch.equal(dice._unions[0], union) and dice._group_names == ["p0", "p1"]
    if taps:
        assert ep.meters["individual_mis"].summary() == {"Conv5": 1.5, "Up_conv3": 2.5}
    if name == "UDAIICEpocher":           # constants of the instance, recorded with every iteration
        assert ep.meters["iic_weight"].summary() == {"mean": 0.125} and ep.meters["uda_weight"].summary() == {"mean": 5.0}
    # nothing else moved: lr and reg_weight are fed once per epoch by _run, not here
    untouched = set(ep.meters.meter_names) - set(fed) - {"sup_dice", "individual_mis", "iic_weight", "uda_weight"}
    assert all(ep.meters[meter].n == 0 for meter in untouched), untouched


@pytest.mark.parametrize("name", ["UDATrainEpocher", "MIDLTrainEpocher", "IICTrainEpocher", "EntropyMinEpocher"])
def test_record_leaves_optional_meters_alone_without_their_keys(name):
    ep = _bare(name)
    ep._record({"sup_loss": 0.75, "reg_loss": 0.5}, *_counts(), ["p0", "p1"])
    assert ep.meters["sup_loss"].n == ep.meters["reg_loss"].n == 1
    for meter in set(ep.meters.meter_names) - {"sup_loss", "reg_loss", "sup_dice", "individual_mis"}:
        assert ep.meters[meter].n == 0, meter
    if "individual_mis" in ep.meters.meter_names:
        assert ep.meters["individual_mis"].summary() == {}


def test_supervised_loss_unfused_is_the_reference_call_and_keeps_its_assertions():
    """8 pixels, 3 classes.  A ``KL_div`` without the fused kernel is called as the reference calls it, on softmax and one-hot.  A
    label outside [0, C) raises AssertionError.  ``disable_assert`` reaches the criterion alone -- it spares ``KL_div``'s own
    assertions (the evaluation's probabilities carry no graph) --; the label check is ``class2one_hot``'s and stays on in the
    evaluation too, as it was at each of the five call sites this function replaced."""
    from deepclustering2.loss import KL_div
    from deepclustering2.utils import class2one_hot
    from semi_seg.epocher import supervised_loss

    class Unfused(KL_div):
        def supports_fused(self):
            return False

    g = torch.Generator().manual_seed(0)
    logits = torch.randn(2, 3, 2, 2, generator=g).requires_grad_(True)
    labels = torch.tensor([[[0, 1], [2, 1]], [[2, 2], [0, 1]]])
    crit = Unfused(verbose=False)
    got = supervised_loss(crit, logits, labels, 3)
    want = crit(logits.softmax(1), class2one_hot(labels, 3))
    assert torch.equal(got, want) and got.requires_grad
    assert torch.equal(supervised_loss(crit, logits, labels, 3, disable_assert=True), want)
    bad = labels.clone()
    bad[0, 0, 0] = 3
    with pytest.raises(AssertionError):
        supervised_loss(crit, logits, bad, 3)
    with pytest.raises(AssertionError):
        supervised_loss(crit, logits, bad, 3, disable_assert=True)
    # what disable_assert does disable: KL_div insists on a graph behind the probabilities, and the evaluation has none
    with pytest.raises(AssertionError):
        supervised_loss(crit, logits.detach(), labels, 3)
    assert torch.equal(supervised_loss(crit, logits.detach(), labels, 3, disable_assert=True), want.detach())
    # a criterion that is no KL_div is called with the two operands and nothing else, unless the evaluation asks
    seen = []
    supervised_loss(lambda *a, **k: seen.append((len(a), k)) or a[0].sum(), logits, labels, 3)
    supervised_loss(lambda *a, **k: seen.append((len(a), k)) or a[0].sum(), logits, labels, 3, disable_assert=True)
    assert seen == [(2, {}), (2, {"disable_assert": True})]


def test_consistency_loss_fallback_calls_the_criterion_once_on_materialised_operands(monkeypatch):
    from miseg_amd import ops
    from semi_seg.epocher import consistency_loss

    def torch_flip(x, masks):       # bit 0: flip H, bit 1: flip W, per sample
        return torch.stack([s.flip([d + 1 for d in range(2) if int(m) >> d & 1]) for s, m in zip(x, masks)])

    monkeypatch.setattr(ops, "flip", torch_flip)
    g = torch.Generator().manual_seed(1)
    student = torch.randn(2, 3, 2, 4, generator=g).requires_grad_(True)
    other = torch.randn(2, 3, 2, 4, generator=g).requires_grad_(True)
    flips = torch.tensor([1, 2], dtype=torch.int32)
    calls = []

    def criterion(a, b):
        calls.append((a, b))
        return (a - b).abs().sum()

    out = consistency_loss(criterion, student, other, flips)
    assert len(calls) == 1
    a, b = calls[0]
    assert torch.equal(a, student.softmax(1)) and a.requires_grad
    assert torch.equal(b, torch_flip(other, flips).softmax(1)) and not b.requires_grad
    assert torch.equal(out, (a - b).abs().sum())


def test_pending_has_no_capture_leftovers():
    from semi_seg.epocher import _Pending
    assert not hasattr(_Pending, "drain") and not hasattr(_Pending, "set_static")
    assert hasattr(_Pending(), "_static")      # precompute's slot stays


FLOAT16 = {"vat": "Trainer.name=vat has no loss scaling in its direction pass: use Arch.compute_dtype float32 or bfloat16",
           "contrast": "Trainer.name=contrast has no loss scaling: use Arch.compute_dtype float32 or bfloat16",
           "contrastdecoder": "Trainer.name=contrastdecoder has no loss scaling: use Arch.compute_dtype float32 or bfloat16"}
MULTI_RANK = {"vat": "Trainer.name=vat runs in a single process: the gradient reducer's hooks would also fire in the direction pass",
              "contrast": "Trainer.name=contrast runs in a single process: a cross-rank contrastive loss needs an all-gather of the "
                          "embeddings, which is not implemented",
              "contrastdecoder": "Trainer.name=contrastdecoder runs in a single process: a cross-rank contrastive loss needs an all-gather "
                                 "of the embeddings, which is not implemented"}


@pytest.mark.parametrize("name", sorted(FLOAT16))
def test_trainer_refusals_keep_their_types_and_messages(name, monkeypatch):
    import torch.distributed as dist
    from semi_seg.trainer import trainer_zoos
    tr = object.__new__(trainer_zoos[name])
    for dtype in (torch.float32, torch.bfloat16):
        tr._model = types.SimpleNamespace(compute_dtype=dtype)
        tr._refuse_float16()
    tr._model = types.SimpleNamespace(compute_dtype=torch.float16)
    with pytest.raises(NotImplementedError) as err:
        tr._refuse_float16()
    assert str(err.value) == FLOAT16[name]
    assert tr.attach_data_parallel() is None            # a single process: nothing to attach, nothing refused
    monkeypatch.setattr(dist, "is_available", lambda: True)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 2)
    with pytest.raises(RuntimeError) as err:
        tr.attach_data_parallel()
    assert str(err.value) == MULTI_RANK[name]


def test_mean_teacher_evaluates_its_teacher_through_the_base_trainer():
    from semi_seg.trainer import MeanTeacherTrainer, SemiTrainer
    assert MeanTeacherTrainer._eval_epoch is SemiTrainer._eval_epoch
    tr = object.__new__(MeanTeacherTrainer)
    tr._model, tr._teacher_model = object(), object()
    assert tr._inference_model() is tr._teacher_model
