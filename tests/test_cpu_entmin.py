"""CPU side of the `entmin` trainer (``Trainer.name=entmin``, the ``EntropyMinParameters`` section): registration, the section it
reads (CLI override included), the epocher it builds, the library's new entry point, the class-count query, the checkpoint tree and
``Entropy.supports_fused``."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mi-based-regularized-semi-supervised-segmentation_amd")
NEW = "miseg_softmax_entropy"
DISPATCH = (2, 3, 4, 5, 6, 8, 10, 16)          # MISEG_DISPATCH_C of csrc/losses.hip


def _config(argv=()):
    from deepclustering2.configparser import ConfigManger
    return ConfigManger(os.path.join(PKG, "config", "semi.yaml"), verbose=False, argv=list(argv))


def _trainer(cfg):
    from contrastyou.arch import UNet
    from deepclustering2.loss import KL_div
    from semi_seg.trainer import trainer_zoos
    tr = trainer_zoos["entmin"].__new__(trainer_zoos["entmin"])
    tr._config = cfg
    tr._model = UNet(**cfg["Arch"])
    tr._init()
    # what _make_epocher reads besides the section
    tr._optimizer, tr._labeled_loader, tr._unlabeled_loader, tr._sup_criterion = None, iter(()), iter(()), KL_div(verbose=False)
    tr._num_batches, tr._cur_epoch, tr._device = 1, 0, "cpu"
    return tr


def test_trainer_zoo_has_entmin_reading_its_section():
    import yaml
    from semi_seg import epocher as E
    from semi_seg.trainer import EntropyMinTrainer, SemiTrainer, trainer_zoos
    assert trainer_zoos["entmin"] is EntropyMinTrainer and issubclass(EntropyMinTrainer, SemiTrainer)
    assert {"partial", "uda", "iic", "udaiic", "meanteacher", "midl"} <= set(trainer_zoos)
    cfg = yaml.safe_load(open(os.path.join(PKG, "config", "semi.yaml")))
    assert cfg["EntropyMinParameters"] == {"weight": 0.00001}          # the shipped default stays
    tr = _trainer(cfg)
    assert tr._reg_weight == cfg["EntropyMinParameters"]["weight"] == 1e-5
    ep = tr._make_epocher()
    assert type(ep) is E.EntropyMinEpocher and issubclass(E.EntropyMinEpocher, E.TrainEpocher)
    assert ep._reg_weight == 1e-5
    from deepclustering2.meters2 import MeterInterface
    assert sorted(ep._configure_meters(MeterInterface()).meter_names) == ["entropy", "lr", "reg_loss", "sup_dice", "sup_loss"]
    assert getattr(ep.regularization, "_miseg_fused", False)
    # no module of its own on the trainer: the checkpoint tree stays the partial one
    assert not any(hasattr(v, "state_dict") for k, v in vars(tr).items() if k not in ("_model", "_sup_criterion"))


def test_cli_override_reaches_the_epocher():
    cfg = _config(["Trainer.name=entmin", "EntropyMinParameters.weight=0.5"]).config
    tr = _trainer(cfg)
    assert tr._reg_weight == 0.5
    assert tr._make_epocher()._reg_weight == 0.5


def test_library_exports_and_header_declares_the_new_entry_point():
    from miseg_amd import _cabi
    header = open(os.path.join(ROOT, "include", "miseg_hip.h")).read()
    assert re.search(r"\bint\s+" + NEW + r"\s*\(", header)
    assert NEW in _cabi.declared_symbols()
    restype, argtypes = _cabi.PROTOTYPES[NEW]
    assert len(argtypes) == 11                     # stream, logits, N, H, W, C, upstream, loss, glogits, ws, ws_bytes
    lib = os.path.join(PKG, "lib", "libmiseg_hip.so")
    assert os.path.exists(lib), "build() makes the library"
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT " + NEW + r"$", out, re.M)


def test_supported_class_counts_mirror_the_dispatch_list():
    from miseg_amd import ops
    assert [c for c in range(0, 40) if ops.softmax_entropy_supported(c)] == list(DISPATCH)
    # ... which is the list the library's source dispatches on
    src = open(os.path.join(PKG, "csrc", "losses.hip")).read()
    macro = src[src.index("#define MISEG_DISPATCH_C"):]
    macro = macro[:macro.index("default:")]
    assert tuple(int(m) for m in re.findall(r"case (\d+):", macro)) == DISPATCH


def test_checkpoint_key_tree_after_init_is_the_partial_trainers(golden, tmp_path):
    """No module of its own: ``trainer.state_dict()`` after ``init()`` has the partial trainer's key tree line for line (the REFERENCE
    partial trainer's, tests/golden/trainer_io.npz)."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import synth
    from test_cpu_host import _build_trainer
    tr = _build_trainer("entmin", tmp_path / "run")
    mine = sorted(synth.tree_lines(tr.state_dict()))
    assert mine == [str(x) for x in golden("trainer_io")["partial/tree_after_init"]]


def test_entropy_supports_fused_for_the_defaults_only():
    from deepclustering2.loss import Entropy
    assert Entropy().supports_fused() and Entropy(reduction="mean", eps=1e-16).supports_fused()
    assert not Entropy(reduction="sum").supports_fused()
    assert not Entropy(reduction="none").supports_fused()
    assert not Entropy(eps=1e-8).supports_fused()


def test_entropy_forward_is_unchanged():
    """``forward`` stays the wheel's expression."""
    import torch
    from deepclustering2.loss import Entropy
    p = torch.randn(3, 5, 7, 6, generator=torch.Generator().manual_seed(0)).softmax(1)
    ref = -(p * (p + 1e-16).log()).sum(1)
    assert torch.equal(Entropy()(p), ref.mean()) and torch.equal(Entropy(reduction="sum")(p), ref.sum())
    assert torch.equal(Entropy(reduction="none")(p), ref)
