"""CPU side of the `contrastdecoder` trainer (``Trainer.name=contrastdecoder``): registration, the
``ContrastDecoderParameters`` defaults and their overrides, ``LocalLabelGenerator`` and ``unfold_position`` against the reference's
recorded labels and hand-built cases, the pool kernel's row layout as ``unfold_position``, ``LocalProjectionHead``'s key layout and CPU
composition against float64, the reference's recorded loss from its recorded pooled output, the refusals and the new entry points."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import trainer_harness as th
from contrast_decoder_ref import GROUPS, embed_rows, golden_projector_state
from trainer_harness import PKG

SHIPPED = {"extract_position": "Up_conv3", "enable_grad_from": "Up5", "ptype": "mlp", "output_size": [4, 4], "partition_num": [2, 2],
           "temperature": 0.07, "base_temperature": 0.07}


def _build(tmp_path, argv=()):
    from semi_seg.main import build_trainer
    return build_trainer(["Trainer.name=contrastdecoder", "Data.name=synthetic", "Trainer.device=cpu", f"Trainer.save_dir={tmp_path}/run",
                          "Trainer.max_epoch=2", "Trainer.num_batches=1", "Data.size=32", "LabeledData.batch_size=1",
                          "UnlabeledData.batch_size=2"] + list(argv))


# ------------------------------------------------------------------------------------------------ registration and configuration
def test_trainer_zoo_has_contrastdecoder_and_keeps_the_others():
    from semi_seg.trainer import ContrastDecoderTrainer, ContrastTrainer, SemiTrainer, trainer_zoos
    assert trainer_zoos["contrastdecoder"] is ContrastDecoderTrainer and issubclass(ContrastDecoderTrainer, SemiTrainer)
    assert trainer_zoos["contrast"] is ContrastTrainer
    assert {"partial", "uda", "iic", "udaiic", "meanteacher", "midl", "entmin", "contrast"} <= set(trainer_zoos)


def test_shipped_section_is_read_and_overrides_reach_the_epocher(tmp_path):
    import yaml
    from semi_seg import epocher as E
    assert yaml.safe_load(open(os.path.join(PKG, "config", "contrast_decoder.yaml"))) == {"ContrastDecoderParameters": SHIPPED}
    tr = _build(tmp_path)
    assert tr._config["ContrastDecoderParameters"] == SHIPPED and "ContrastParameters" not in tr._config
    written = yaml.safe_load(open(tmp_path / "run" / "config.yaml"))
    assert written["ContrastDecoderParameters"] == SHIPPED and "ContrastParameters" not in written
    ep = tr._make_epocher()
    assert type(ep) is E.PretrainDecoderEpocher and ep._extract_position == "Up_conv3" and ep._partition_num == (2, 2)
    assert type(ep._label_generator).__name__ == "LocalLabelGenerator"
    from deepclustering2.meters2 import MeterInterface
    assert sorted(ep._configure_meters(MeterInterface()).meter_names) == ["contrastive_loss", "lr"]
    tr = _build(tmp_path / "b", ["ContrastDecoderParameters.ptype=linear", "ContrastDecoderParameters.temperature=0.1",
                                 "ContrastDecoderParameters.extract_position=Up_conv4", "ContrastDecoderParameters.enable_grad_from=Up_conv5"])
    assert tr._config["ContrastDecoderParameters"] == {**SHIPPED, "ptype": "linear", "temperature": 0.1, "extract_position": "Up_conv4",
                                                       "enable_grad_from": "Up_conv5"}
    assert tr._contrastive_criterion.temperature == 0.1 and tr._contrastive_criterion.base_temperature == 0.07
    assert sorted(tr._projector.state_dict()) == ["_projector.0.bias", "_projector.0.weight"]
    assert tuple(tr._projector.state_dict()["_projector.0.weight"].shape) == (64, 64, 3, 3)
    assert all(p.requires_grad == n.startswith(("Up_conv5.", "Up4.", "Up_conv4.")) for n, p in tr._model.named_parameters())
    with pytest.raises(ValueError, match="partition_num"):
        _build(tmp_path / "c", ["ContrastDecoderParameters.partition_num=[3,2]"])
    with pytest.raises(ValueError, match="extract_position"):
        _build(tmp_path / "d", ["ContrastDecoderParameters.extract_position=Up_conv9"])


def test_the_other_configuration_files_are_untouched():
    import yaml
    semi = yaml.safe_load(open(os.path.join(PKG, "config", "semi.yaml")))
    assert "ContrastDecoderParameters" not in semi and "ContrastParameters" not in semi
    contrast = yaml.safe_load(open(os.path.join(PKG, "config", "contrast.yaml")))
    assert contrast == {"ContrastParameters": {"group_option": "partition", "extract_position": "Conv5", "ptype": "mlp", "output_dim": 256,
                                               "temperature": 0.07, "base_temperature": 0.07}}


# ------------------------------------------------------------------------------------------------ labels and the unfold
def test_unfold_position_hand_built_case():
    from contrastyou.epocher._utils import unfold_position
    x = torch.arange(2 * 3 * 4 * 6, dtype=torch.float32).view(2, 3, 4, 6)
    blocks, flags = unfold_position(x, (2, 2))
    assert tuple(blocks.shape) == (8, 3, 2, 3)
    assert flags == [(0, 0)] * 2 + [(0, 3)] * 2 + [(2, 0)] * 2 + [(2, 3)] * 2
    assert torch.equal(blocks[0], x[0, :, 0:2, 0:3]) and torch.equal(blocks[3], x[1, :, 0:2, 3:6]) and torch.equal(blocks[6], x[0, :, 2:4, 3:6])
    blocks, flags = unfold_position(x, (4, 4))                       # a width the grid does not divide: blocks of 6 // 4 = 1 pixel, all six per row (the reference's arithmetic)
    assert tuple(blocks.shape) == (4 * 6 * 2, 3, 1, 1) and flags[-1] == (3, 5)
    blocks, flags = unfold_position(torch.zeros(1, 1, 5, 5), (2, 2))
    assert tuple(blocks.shape) == (4, 1, 2, 2) and flags == [(0, 0), (0, 2), (2, 0), (2, 2)]


@pytest.mark.parametrize("n,c,osz,part,views", [(4, 3, (4, 4), (2, 2), 2), (6, 2, (4, 6), (2, 3), 3), (3, 5, (4, 4), (1, 1), 1), (2, 4, (4, 4), (4, 4), 2)])
def test_kernel_row_layout_is_cat_of_unfold_position_over_the_views(n, c, osz, part, views):
    """The layout formula of ``miseg_bias_amaxpool_fwd`` (tests/contrast_decoder_ref.embed_rows) against the reference's function."""
    from contrastyou.epocher._utils import unfold_position
    pooled = torch.arange(n * c * osz[0] * osz[1], dtype=torch.float32).view(n, c, *osz)
    want = torch.cat([unfold_position(chunk, part)[0].reshape(part[0] * part[1] * (n // views), -1) for chunk in torch.chunk(pooled, views, dim=0)])
    assert torch.equal(embed_rows(pooled, part, views), want)
    if part == (1, 1) and views == 1:
        assert torch.equal(want, pooled.view(n, -1))


def test_local_label_generator_against_the_recorded_labels_and_by_hand(golden):
    from contrastyou.epocher._utils import LocalLabelGenerator, unfold_position
    g = golden("contrast_decoder")
    partitions, patients = [str(p) for p in g["partitions"]], [str(p) for p in g["patients"]]
    locations = unfold_position(torch.zeros(4, 1, 4, 4), (2, 2))[1]
    labels = LocalLabelGenerator()(partitions, patients, locations)
    assert labels == [int(v) for v in g["labels"]] and len(labels) == 16
    # samples 0 and 1 (patient001, partition 0) share a label in every block, 2 (partition 1) and 3 (patient002) stand alone
    assert all(labels[4 * k] == labels[4 * k + 1] and len({labels[4 * k], labels[4 * k + 2], labels[4 * k + 3]}) == 3 for k in range(4))
    assert len(set(labels)) == 12
    # by hand: keys "_<location>_<patient>_<partition>", ranked among the sorted unique keys
    got = LocalLabelGenerator()(["1", "0"], ["b", "a"], ["(0, 0)", "(0, 0)", "(0, 2)", "(0, 2)"])
    assert got == [1, 0, 3, 2]
    with pytest.raises(AssertionError):
        LocalLabelGenerator()(["0", "1"], ["a", "b"], ["x", "y", "z"])


def test_epocher_locations_equal_unfold_positions_flags():
    from contrastyou.arch import UNet
    from contrastyou.epocher._utils import unfold_position
    from contrastyou.trainer._utils import LocalProjectionHead
    from semi_seg.epocher import PretrainDecoderEpocher
    for osz, part in (((4, 4), (2, 2)), ((4, 4), (4, 4)), ((6, 4), (2, 1))):
        ep = PretrainDecoderEpocher(UNet(1, 4), LocalProjectionHead(32, output_size=osz), None, iter(()), None, 1, 0, "cpu", "Up_conv3", part)
        assert ep._locations(3) == unfold_position(torch.zeros(3, 1, *osz), part)[1]


# ------------------------------------------------------------------------------------------------ the head
@pytest.mark.parametrize("head_type", ["mlp", "linear"])
def test_local_projection_head_keys_and_cpu_composition_against_float64(head_type):
    from contrastyou.epocher._utils import unfold_position
    from contrastyou.trainer._utils import LocalProjectionHead
    torch.manual_seed(0)
    head = LocalProjectionHead(32, head_type=head_type)
    want = {"_projector.0.weight": (64, 32, 3, 3), "_projector.0.bias": (64,)}
    if head_type == "mlp":
        want.update({"_projector.2.weight": (32, 64, 3, 3), "_projector.2.bias": (32,)})
        assert isinstance(head._projector[1], torch.nn.LeakyReLU) and head._projector[1].negative_slope == 0.01
    assert {k: tuple(v.shape) for k, v in head.state_dict().items()} == want
    with pytest.raises(AssertionError):
        LocalProjectionHead(32, head_type="conv")
    ref = torch.nn.Sequential(*[torch.nn.Conv2d(32, 64, 3, 1, 1), torch.nn.LeakyReLU(0.01), torch.nn.Conv2d(64, 32, 3, 1, 1)][:3 if head_type == "mlp" else 1])
    ref.load_state_dict({k.replace("_projector.", ""): v for k, v in head.state_dict().items()})
    ref = ref.double()
    x = torch.randn(4, 32, 10, 7, generator=torch.Generator().manual_seed(1))
    out = head(x)
    out64 = F.adaptive_max_pool2d(ref(x.double()), (4, 4))
    assert tuple(out.shape) == tuple(out64.shape) and float((out.double() - out64).abs().max()) <= 1e-5 * float(out64.abs().max())
    rows = head.embeddings(x, views=2, partition_num=(2, 2))
    assert torch.equal(rows, torch.cat([unfold_position(c, (2, 2))[0].reshape(8, -1) for c in torch.chunk(out, 2)]))
    with pytest.raises(ValueError):
        head.embeddings(x[:3], views=2)
    with pytest.raises(ValueError):
        head.embeddings(x, views=2, partition_num=(3, 2))


def test_recorded_pooled_output_gives_the_recorded_loss(golden):
    """The reference's pooled projector output of iteration 1, unfolded, through ``SupConLoss.from_embeddings`` with the recorded labels:
    its recorded first loss (fp32 composition: 1e-5 covers its rounding)."""
    from contrastyou.epocher._utils import unfold_position
    from contrastyou.losses.contrast_loss import SupConLoss
    g = golden("contrast_decoder")
    pooled = torch.from_numpy(g["pooled_step1"])
    assert tuple(pooled.shape) == (8, 32, 4, 4) and g["loss"].shape == (3,) and g["masks"].shape == (3, 4)
    assert sorted(int(m) for m in g["masks"][0]) == [0, 1, 2, 3]
    rows = torch.cat([unfold_position(c, (2, 2))[0].reshape(16, -1) for c in torch.chunk(pooled, 2)])
    assert torch.equal(rows, embed_rows(pooled, (2, 2), 2))
    loss = SupConLoss().from_embeddings(rows, [int(v) for v in g["labels"]])
    assert abs(float(loss) - float(g["loss"][0])) <= 1e-5 * float(g["loss"][0])
    # the fixture's own record: 16 seeds x 4 groups of fp32 <-> float64 distances, the chosen seed among them, its arg-max margin above 2
    seeds = [int(s) for s in g["model_seeds"]]
    assert seeds == list(range(83, 99)) and int(g["cfg/model_seed"]) in seeds
    assert all(0.0 < float(g[f"own_error/{s}/{k}"]) < 3e-2 for s in seeds for k in GROUPS)
    assert float(g["pool_margin_min"]) > 2.0 and float(g["pool_gap_min"]) > 0.0
    state = golden_projector_state()
    assert {k: tuple(v.shape) for k, v in state.items()} == {"_projector.0.weight": (64, 32, 3, 3), "_projector.0.bias": (64,),
                                                             "_projector.2.weight": (32, 64, 3, 3), "_projector.2.bias": (32,)}


# ------------------------------------------------------------------------------------------------ the kernels' host side
def test_supported_mirrors():
    from miseg_amd import ops
    assert ops.bias_lrelu_supported(32) and ops.bias_lrelu_supported(1024) and ops.bias_lrelu_supported(4)
    assert not ops.bias_lrelu_supported(30) and not ops.bias_lrelu_supported(0) and not ops.bias_lrelu_supported(1028)
    assert ops.bias_amaxpool_supported(8, 32, 32, 32, (4, 4), (2, 2), 2) and ops.bias_amaxpool_supported(2, 32, 3, 5, (4, 4), (2, 2), 1)
    assert not ops.bias_amaxpool_supported(8, 32, 32, 32, (4, 4), (3, 2), 2) and not ops.bias_amaxpool_supported(7, 32, 32, 32, (4, 4), (2, 2), 2)
    assert not ops.bias_amaxpool_supported(8, 30, 32, 32, (4, 4), (2, 2), 2) and not ops.bias_amaxpool_supported(1, 32, 65536, 32768)
    assert ops.conv3x3_bias_supported(32, 64, torch.float32) and ops.conv3x3_bias_supported(64, 32, torch.bfloat16)
    assert ops.conv3x3_bias_supported(4, 4, torch.float32) and not ops.conv3x3_bias_supported(4, 8, torch.float16)
    assert not ops.conv3x3_bias_supported(30, 64, torch.float32) and not ops.conv3x3_bias_supported(32, 64, torch.float64)
    src = open(os.path.join(PKG, "csrc", "contrast_decoder.hip")).read()
    assert "kCdMaxC = 1024" in src and ops._CD_MAX_C == 1024


def test_library_exports_and_header_declares_the_new_entry_points():
    from miseg_amd import _cabi
    new = {"miseg_bias_lrelu_fwd": 10, "miseg_bias_lrelu_bwd_ws_bytes": 5, "miseg_bias_lrelu_bwd": 13, "miseg_bias_amaxpool_fwd": 15,
           "miseg_bias_amaxpool_bwd": 15}
    _, out = th.assert_entry_points(new)
    for name, nargs in new.items():
        assert len(_cabi.PROTOTYPES[name][1]) == nargs
        assert re.search(r"\bT f16_" + name + r"$", out, re.M)
    assert _cabi.lib().miseg_version() >= 409
    ws = _cabi.lib().miseg_bias_lrelu_bwd_ws_bytes
    assert ws(_cabi.F32, 4, 8, 8, 32) == 8 * 32 * 4 and ws(_cabi.BF16, 32, 128, 128, 32) == 1024 * 32 * 4 and ws(_cabi.F32, 4, 8, 8, 30) == -1


# ------------------------------------------------------------------------------------------------ the trainer on the CPU
def test_trainer_builds_with_exactly_the_decoder_blocks_and_projector_trainable_and_refuses(tmp_path):
    tr = _build(tmp_path)
    model = tr._model
    blocks = ("Up5.", "Up_conv5.", "Up4.", "Up_conv4.", "Up3.", "Up_conv3.")
    mine = {id(p) for p in tr._trainable()}
    want = [p for n, p in model.named_parameters() if n.startswith(blocks)] + list(tr._projector.parameters())
    assert mine == {id(p) for p in want} and len(mine) == len(want)
    assert all(p.requires_grad == n.startswith(blocks) for n, p in model.named_parameters())
    given = [p for g in tr._optimizer.param_groups for p in g["params"]]
    assert {id(p) for p in given} == mine
    ck = tr.state_dict()
    assert {"_model", "_projector", "_optimizer", "_scheduler", "_contrastive_criterion", "_storage", "_buffers"} <= set(ck)
    assert sorted(ck["_projector"]) == ["_projector.0.bias", "_projector.0.weight", "_projector.2.bias", "_projector.2.weight"]
    assert tr.attach_data_parallel() is None
    with pytest.raises(NotImplementedError, match="Trainer.name=contrastdecoder pre-trains the decoder"):
        tr._eval_epoch(loader=None)
    with pytest.raises(NotImplementedError, match="Trainer.name=contrastdecoder has no segmentation"):
        tr.inference()
    with pytest.raises(NotImplementedError, match="Trainer.name=contrastdecoder has no loss scaling"):
        _build(tmp_path / "h", ["Arch.compute_dtype=float16"])


def test_more_than_one_rank_is_refused(tmp_path, monkeypatch):
    import torch.distributed as dist
    tr = _build(tmp_path)
    monkeypatch.setattr(dist, "is_available", lambda: True)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 2)
    with pytest.raises(RuntimeError, match="Trainer.name=contrastdecoder runs in a single process"):
        tr.attach_data_parallel()


def test_loader_recipe_loses_its_total_freedom():
    """A loader whose dataset carries a ``Recipe`` gets the ``total_freedom=False`` copy: both views share the geometric transform."""
    from miseg_amd.slices import Recipe
    from semi_seg.augment import ACDCStrongTransforms
    from semi_seg.trainer import ContrastDecoderTrainer

    class Dataset:
        transform = ACDCStrongTransforms.pretrain

        def set_transform(self, t):
            self.transform = t

    class Loader:
        dataset = Dataset()

    assert ACDCStrongTransforms.pretrain.total_freedom
    tr = ContrastDecoderTrainer.__new__(ContrastDecoderTrainer)
    tr._unlabeled_loader = Loader()
    tr._use_shared_geometry()
    got = Loader.dataset.transform
    assert isinstance(got, Recipe) and not got.total_freedom and got.geo == ACDCStrongTransforms.pretrain.geo and got.twice
    assert ACDCStrongTransforms.pretrain.total_freedom                     # the shared preset itself is not edited
