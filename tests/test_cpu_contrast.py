"""CPU side of the `contrast` trainer (``Trainer.name=contrast``): registration, the ``ContrastParameters``
defaults and their CLI overrides, the label generator, the torch composition of ``SupConLoss`` against the reference's recorded losses
and a float64 closed form, its ``ValueError``s, the projection head's key layout, the new entry points, ``Pretrained=`` and the trainer
built on the CPU."""
import os
import re

import pytest
import torch

import trainer_harness as th
from contrast_ref import closed_form, embeddings as _embeddings
from trainer_harness import PKG

SHIPPED = {"group_option": "partition", "extract_position": "Conv5", "ptype": "mlp", "output_dim": 256, "temperature": 0.07,
           "base_temperature": 0.07}


def _build(tmp_path, argv=()):
    from semi_seg.main import build_trainer
    return build_trainer(["Trainer.name=contrast", "Data.name=synthetic", "Trainer.device=cpu", f"Trainer.save_dir={tmp_path}/run",
                          "Trainer.max_epoch=2", "Trainer.num_batches=1", "Data.size=32", "LabeledData.batch_size=1",
                          "UnlabeledData.batch_size=2"] + list(argv))


# ------------------------------------------------------------------------------------------------ registration and configuration
def test_trainer_zoo_has_contrast_and_keeps_the_others():
    from semi_seg.trainer import ContrastTrainer, SemiTrainer, trainer_zoos
    assert trainer_zoos["contrast"] is ContrastTrainer and issubclass(ContrastTrainer, SemiTrainer)
    assert {"partial", "uda", "iic", "udaiic", "meanteacher", "midl", "entmin"} <= set(trainer_zoos)


def test_shipped_section_is_read_and_cli_overrides_reach_the_epocher(tmp_path):
    import yaml
    from semi_seg import epocher as E
    assert yaml.safe_load(open(os.path.join(PKG, "config", "contrast.yaml"))) == {"ContrastParameters": SHIPPED}
    tr = _build(tmp_path)
    assert tr._config["ContrastParameters"] == SHIPPED
    assert yaml.safe_load(open(tmp_path / "run" / "config.yaml"))["ContrastParameters"] == SHIPPED
    ep = tr._make_epocher()
    assert type(ep) is E.PretrainEncoderEpocher and ep._group_option == "partition" and ep._extract_position == "Conv5"
    from deepclustering2.meters2 import MeterInterface
    assert sorted(ep._configure_meters(MeterInterface()).meter_names) == ["contrastive_loss", "lr"]
    tr = _build(tmp_path / "b", ["ContrastParameters.group_option=both", "ContrastParameters.ptype=linear", "ContrastParameters.output_dim=64",
                                 "ContrastParameters.temperature=0.1", "ContrastParameters.extract_position=Conv4"])
    assert tr._config["ContrastParameters"] == {**SHIPPED, "group_option": "both", "ptype": "linear", "output_dim": 64, "temperature": 0.1,
                                                "extract_position": "Conv4"}
    assert tr._contrastive_criterion.temperature == 0.1 and tr._contrastive_criterion.base_temperature == 0.07
    assert sorted(tr._projector.state_dict()) == ["_header.2.bias", "_header.2.weight"]
    assert tuple(tr._projector.state_dict()["_header.2.weight"].shape) == (64, 128)
    ep = tr._make_epocher()
    assert ep._group_option == "both" and ep._extract_position == "Conv4"
    assert ep._label_generator._contrastive_on_patient and ep._label_generator._contrastive_on_partition


def test_semi_yaml_is_untouched_by_the_new_section():
    import yaml
    cfg = yaml.safe_load(open(os.path.join(PKG, "config", "semi.yaml")))
    assert "ContrastParameters" not in cfg and "Pretrained" not in cfg


# ------------------------------------------------------------------------------------------------ labels
def test_global_label_generator_hand_written_cases():
    from contrastyou.epocher._utils import GlobalLabelGenerator
    partitions = ["2", "0", "1", "0", "2"]
    patients = ["p2", "p1", "p1", "p2", "p2"]
    assert GlobalLabelGenerator(contrastive_on_patient=False, contrastive_on_partition=True)(partitions, patients) == [2, 0, 1, 0, 2]
    assert GlobalLabelGenerator(contrastive_on_patient=True, contrastive_on_partition=False)(partitions, patients) == [1, 0, 0, 1, 1]
    # both: "_p2_2", "_p1_0", "_p1_1", "_p2_0", "_p2_2" -> sorted unique: _p1_0 _p1_1 _p2_0 _p2_2
    assert GlobalLabelGenerator(contrastive_on_patient=True, contrastive_on_partition=True)(partitions, patients) == [3, 0, 1, 2, 3]
    assert GlobalLabelGenerator(False, False)(partitions, patients) == [0] * 5                 # every sample the same class
    assert GlobalLabelGenerator()(["10", "9"], ["a", "b"]) == [0, 1]                           # string order: "_10" < "_9"
    with pytest.raises(AssertionError):
        GlobalLabelGenerator()(["0"], ["a", "b"])


def test_epocher_group_options_select_the_generator_switches():
    from semi_seg.epocher import PretrainEncoderEpocher
    from contrastyou.arch import UNet
    net = UNet(1, 4)
    for opt, want in (("partition", (False, True)), ("patient", (True, False)), ("both", (True, True))):
        ep = PretrainEncoderEpocher(net, torch.nn.Identity(), None, iter(()), None, 1, 0, "cpu", opt, "Conv5")
        assert (ep._label_generator._contrastive_on_patient, ep._label_generator._contrastive_on_partition) == want
    with pytest.raises(AssertionError):
        PretrainEncoderEpocher(net, torch.nn.Identity(), None, iter(()), None, 1, 0, "cpu", "slice", "Conv5")


# ------------------------------------------------------------------------------------------------ the loss, composed
@pytest.mark.parametrize("b,d,views,labels,T", [(4, 64, 2, [0, 1, 0, 1], 0.07), (5, 32, 2, None, 0.5), (6, 16, 3, [0, 0, 1, 2, 1, 0], 0.07)])
def test_composition_matches_the_float64_closed_form(b, d, views, labels, T):
    """Labels, SimCLR and three views.  The SimCLR case runs at SimCLR's own temperature 0.5: at 0.07 the only positive of an anchor
    (its other view, cosine ~0.96) dominates the denominator, the loss is log(1 + ~1e-5) and fp32 -- the reference's included --
    resolves it to ~1e-3 relative only."""
    from contrastyou.losses.contrast_loss import SupConLoss
    e = _embeddings(b, d, views, seed=b)
    ref_loss, ref_grad = closed_form(e, labels, views, T, T)
    crit = SupConLoss(temperature=T, base_temperature=T)
    e64 = e.double().requires_grad_()
    unit = torch.nn.functional.normalize(e64, dim=1)
    loss = crit(torch.stack(torch.chunk(unit, views, 0), 1), labels=labels)
    loss.backward()
    assert abs(float(loss) - ref_loss) <= 1e-12 * abs(ref_loss)
    assert float((e64.grad - ref_grad).abs().max()) <= 1e-12 * float(ref_grad.abs().max())
    # from_embeddings on the CPU is the same composition behind F.normalize
    e32 = e.clone().requires_grad_()
    loss32 = crit.from_embeddings(e32, labels, views=views)
    loss32.backward()
    assert abs(float(loss32) - ref_loss) <= 1e-5 * abs(ref_loss)
    assert float((e32.grad.double() - ref_grad).abs().max()) <= 1e-5 * float(ref_grad.abs().max())


def test_composition_matches_the_reference_run(golden):
    """The reference's own first loss (tests/golden/contrast.npz) from its own raw embeddings of that iteration: the composition
    behind ``from_embeddings`` in fp32 (the reference's arithmetic: 1e-5 covers its rounding ten times over) and the float64 closed
    form.  Partitions 0 1 0 1 give labels 0 1 0 1: three positives and four negatives per anchor."""
    from contrastyou.epocher._utils import GlobalLabelGenerator
    from contrastyou.losses.contrast_loss import SupConLoss
    g = golden("contrast")
    labels = GlobalLabelGenerator(contrastive_on_partition=True)([str(p) for p in g["partitions"]], [str(p) for p in g["patients"]])
    assert labels == [int(v) for v in g["labels"]] == [0, 1, 0, 1]
    e = torch.from_numpy(g["embeddings_step1"])
    assert tuple(e.shape) == (8, 256) and g["loss"].shape == (3,)
    ref = float(g["loss"][0])
    assert abs(float(SupConLoss().from_embeddings(e, labels)) - ref) <= 1e-5 * abs(ref)
    assert abs(closed_form(e, labels, 2)[0] - ref) <= 1e-5 * abs(ref)
    for k in ("projector", "Conv5", "Conv1-4"):
        assert 0.0 < float(g[f"own_error/{k}"]) < 3e-2 / 4


def test_explicit_mask_one_mode_and_asymmetric_mask():
    from contrastyou.losses.contrast_loss import SupConLoss
    b, d, views = 5, 24, 2
    e = torch.nn.functional.normalize(_embeddings(b, d, views, seed=3).double(), dim=1)
    feats = torch.stack(torch.chunk(e, views, 0), 1)
    labels = [0, 1, 0, 2, 1]
    lab = torch.tensor(labels)
    mask = (lab.view(-1, 1) == lab.view(1, -1)).float()
    crit = SupConLoss(temperature=0.1, base_temperature=0.07)
    assert torch.equal(crit(feats, mask=mask), crit(feats, labels=labels))
    assert torch.equal(crit(feats, mask=torch.eye(b)), crit(feats))                      # SimCLR
    assert abs(float(crit(feats, labels=labels)) - closed_form(e, labels, views, 0.1, 0.07)[0]) < 1e-12
    # 'one': the anchors are view 0 only -- the mean of the first B per-anchor terms of 'all'
    one = SupConLoss(temperature=0.1, base_temperature=0.07, contrast_mode="one")(feats, labels=labels)
    n = views * b
    s = e @ e.t() / 0.1
    off = ~torch.eye(n, dtype=torch.bool)
    logp = s - torch.log((torch.exp(s) * off).sum(1, keepdim=True))
    lab2 = lab.repeat(views)
    pos = (lab2.view(-1, 1) == lab2.view(1, -1)) & off
    per_anchor = -(0.1 / 0.07) * (logp * pos).sum(1) / pos.sum(1)
    assert abs(float(one) - float(per_anchor[:b].mean())) < 1e-12
    # an asymmetric mask: sample 0 takes sample 1 as a positive, not the other way round
    asym = torch.eye(b)
    asym[0, 1] = 1.0
    got = crit(feats, mask=asym)
    pos_a = asym.bool().repeat(views, views) & off
    want = (-(0.1 / 0.07) * (logp * pos_a).sum(1) / pos_a.sum(1)).mean()
    assert abs(float(got) - float(want)) < 1e-12
    # features with trailing dimensions are flattened
    assert torch.equal(crit(feats.view(b, views, 4, 6), labels=labels), crit(feats, labels=labels))


def test_value_errors():
    from contrastyou.losses.contrast_loss import SupConLoss
    crit = SupConLoss()
    feats = torch.randn(4, 2, 8)
    with pytest.raises(ValueError, match="at least 3 dimensions"):
        crit(torch.randn(4, 8))
    with pytest.raises(ValueError, match="Cannot define both"):
        crit(feats, labels=[0, 1, 0, 1], mask=torch.eye(4))
    with pytest.raises(ValueError, match="Num of labels does not match"):
        crit(feats, labels=[0, 1, 0])
    with pytest.raises(ValueError, match="Unknown mode"):
        SupConLoss(contrast_mode="some")(feats)
    with pytest.raises(ValueError, match="Num of labels does not match"):
        crit.from_embeddings(torch.randn(8, 8), [0, 1, 0])
    with pytest.raises(ValueError):
        crit.from_embeddings(torch.randn(7, 8), None)


def test_supcon_supported_mirrors_the_kernels_range():
    from miseg_amd import ops
    assert all(ops.supcon_supported(n, d, 2) for n in (4, 6, 32, 512, 1024) for d in (64, 128, 256, 4, 1024))
    assert ops.supcon_supported(9, 64, 3) and ops.supcon_supported(2, 64, 2)
    assert not ops.supcon_supported(8, 64, 1) and not ops.supcon_supported(9, 64, 2) and not ops.supcon_supported(0, 64, 2)
    assert not ops.supcon_supported(1026, 64, 2) and not ops.supcon_supported(8, 66, 2) and not ops.supcon_supported(8, 2048, 2)
    src = open(os.path.join(PKG, "csrc", "supcon.hip")).read()
    assert "kSupMaxN = 1024, kSupMaxD = 1024" in src and (ops._SUPCON_MAX_N, ops._SUPCON_MAX_D) == (1024, 1024)


def test_library_exports_and_header_declares_the_new_entry_points():
    from miseg_amd import _cabi
    new = {"miseg_supcon": 13, "miseg_supcon_ws_bytes": 2, "miseg_avgpool_fwd": 8, "miseg_avgpool_bwd": 8}
    _, out = th.assert_entry_points(new)
    for name, nargs in new.items():
        assert len(_cabi.PROTOTYPES[name][1]) == nargs
    for name in ("f16_miseg_avgpool_fwd", "f16_miseg_avgpool_bwd"):                       # the IEEE-half twins of the pool
        assert re.search(r"\bT " + name + r"$", out, re.M)
    assert _cabi.lib().miseg_version() >= 408
    ws = _cabi.lib().miseg_supcon_ws_bytes
    assert ws(32, 256) == 4 * (32 * 256 + 32 * 32 + 2 * 32) and ws(8, 66) == -1 and ws(2048, 64) == -1 and ws(1, 64) == -1


# ------------------------------------------------------------------------------------------------ the head
def test_projection_head_state_dict_keys_and_gpu_only_forward():
    from contrastyou.trainer._utils import ProjectionHead
    from miseg_amd._cabi import MisegError
    mlp = ProjectionHead(256, 128)
    assert {k: tuple(v.shape) for k, v in mlp.state_dict().items()} == {
        "_header.2.weight": (256, 256), "_header.2.bias": (256,), "_header.4.weight": (128, 256), "_header.4.bias": (128,)}
    lin = ProjectionHead(64, 32, head_type="linear")
    assert {k: tuple(v.shape) for k, v in lin.state_dict().items()} == {"_header.2.weight": (32, 64), "_header.2.bias": (32,)}
    assert isinstance(mlp._header[3], torch.nn.LeakyReLU) and mlp._header[3].negative_slope == 0.01
    with pytest.raises(AssertionError):
        ProjectionHead(64, 32, head_type="conv")
    with pytest.raises(MisegError):                      # no CPU fallback
        mlp(torch.randn(2, 256, 4, 4))


# ------------------------------------------------------------------------------------------------ Pretrained=
def test_pretrained_resolution_and_refusal_with_checkpoint(tmp_path):
    from contrastyou.arch import UNet
    from semi_seg.main import _pretrained_file, build_trainer, load_pretrained
    src = UNet(1, 4)
    with torch.no_grad():
        for p in src.parameters():
            p.add_(1.0)
    run = tmp_path / "pre"
    run.mkdir()
    torch.save({"_model": src.state_dict(), "_optimizer": {"state": {}, "param_groups": []}, "_buffers": {"_cur_epoch": 7, "_start_epoch": 0,
                                                                                                     "_best_score": 0.5}}, run / "last.pth")
    assert _pretrained_file(run) == run / "last.pth" and _pretrained_file(run / "last.pth") == run / "last.pth"
    with pytest.raises(FileNotFoundError):
        _pretrained_file(tmp_path / "nothing")
    with pytest.raises(FileNotFoundError):
        _pretrained_file(tmp_path)                       # a directory without last.pth
    dst = UNet(1, 4)
    load_pretrained(dst, run)
    assert all(torch.equal(a, b) for a, b in zip(src.state_dict().values(), dst.state_dict().values()))
    bad = dict(src.state_dict())
    bad.pop("Conv1.conv.0.weight")
    torch.save({"_model": bad}, run / "partial.pth")
    with pytest.raises(RuntimeError):                    # strict
        load_pretrained(UNet(1, 4), run / "partial.pth")
    torch.save({"model": src.state_dict()}, run / "other.pth")
    with pytest.raises(KeyError):
        load_pretrained(UNet(1, 4), run / "other.pth")
    with pytest.raises(ValueError, match="Pretrained"):
        build_trainer(["Trainer.name=partial", f"Pretrained={run}", f"Checkpoint={run}", "Data.name=synthetic", "Trainer.device=cpu"])
    tr = build_trainer(["Trainer.name=partial", f"Pretrained={run}", "Data.name=synthetic", "Trainer.device=cpu", f"Trainer.save_dir={tmp_path}/ft",
                        "Data.size=32", "LabeledData.batch_size=1", "UnlabeledData.batch_size=1"])
    assert tr._start_epoch == 0 and tr._cur_epoch == 0 and tr._best_score == -1
    assert all(torch.equal(a, b) for a, b in zip(src.state_dict().values(), tr._model.state_dict().values()))


# ------------------------------------------------------------------------------------------------ the trainer on the CPU
def test_contrast_trainer_builds_on_the_cpu_with_exactly_the_encoder_and_projector_trainable(tmp_path):
    tr = _build(tmp_path)
    model = tr._model
    mine = {id(p) for p in tr._trainable()}
    want = [p for n, p in model.named_parameters() if n.startswith(("Conv1.", "Conv2.", "Conv3.", "Conv4.", "Conv5."))] + list(tr._projector.parameters())
    assert mine == {id(p) for p in want} and len(mine) == len(want) == 5 * 6 + 4
    assert all(p.requires_grad == n.startswith("Conv") for n, p in model.named_parameters())
    given = [p for g in tr._optimizer.param_groups for p in g["params"]]
    assert {id(p) for p in given} == mine
    ck = tr.state_dict()
    assert {"_model", "_projector", "_optimizer", "_scheduler", "_contrastive_criterion", "_storage", "_buffers"} <= set(ck)
    assert sorted(ck["_projector"]) == ["_header.2.bias", "_header.2.weight", "_header.4.bias", "_header.4.weight"]
    assert tr.attach_data_parallel() is None
    with pytest.raises(NotImplementedError, match="fine-tune"):
        tr._eval_epoch(loader=None)
    with pytest.raises(NotImplementedError, match="fine-tune"):
        tr.inference()
    tr4 = _build(tmp_path / "c4", ["ContrastParameters.extract_position=Conv3"])
    assert all(p.requires_grad == n.startswith(("Conv1.", "Conv2.", "Conv3.")) for n, p in tr4._model.named_parameters())
    assert len(list(tr4._trainable())) == 3 * 6 + 4
    with pytest.raises(NotImplementedError, match="loss scaling"):
        _build(tmp_path / "h", ["Arch.compute_dtype=float16"])


def test_encode_stops_at_the_position():
    """``UNet.encode`` calls the blocks up to ``util`` and nothing behind it (the blocks are stubbed: the kernels are GPU only)."""
    from contrastyou.arch import UNet
    net = UNet(1, 4)
    called = []
    for name in net.component_names:
        if name == "DeConv_1x1":
            continue
        getattr(net, name).forward = (lambda nm: lambda x: (called.append(nm), x[0] if isinstance(x, (tuple, list)) else x)[1])(name)
    x = torch.zeros(1, 1, 16, 16)
    net.encode(x, "Conv5")
    assert called == ["Conv1", "Conv2", "Conv3", "Conv4", "Conv5"]
    called.clear()
    net.encode(x, "Conv3")
    assert called == ["Conv1", "Conv2", "Conv3"]
    called.clear()
    net.encode(x, "Up_conv4")
    assert called == ["Conv1", "Conv2", "Conv3", "Conv4", "Conv5", "Up5", "Up_conv5", "Up4", "Up_conv4"]
    with pytest.raises(AssertionError):
        net.encode(x, "Conv6")
