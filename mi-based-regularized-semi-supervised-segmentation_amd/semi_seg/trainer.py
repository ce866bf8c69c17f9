"""The semi-supervised trainers behind ``Trainer.name`` (ref ``semi_seg/trainer.py:24-214``).

Drop-in surface: ``trainer_zoos = {partial, uda, iic, udaiic}`` (+ ``meanteacher``, the reference's ContrastTrainerMT, and ``midl`` and
``entmin``, the ``MIDLPaperParameters`` and ``EntropyMinParameters`` sections' trainers, ``vat``, virtual adversarial training on the
wheel's ``VATLoss``, ``ict``, interpolation consistency training on the Mean Teacher, ``uamt``, the uncertainty-aware Mean Teacher,
``cps``, cross pseudo supervision of two trainable networks, and ``contrast`` and ``contrastdecoder``, the encoder and decoder
stages of the reference's contrastive pre-training), the keyword-only constructor, ``init()``, ``start_training()``,
``inference(checkpoint)``, ``set_feature_positions`` and the attribute names the checkpoint tree is
keyed by (``_model``, ``_optimizer``, ``_scheduler``, ``_projector_wrappers``, ``_IIDSegWrapper``, ``_storage`` ...; the
tree itself is pinned by ``tests/golden/trainer_io.npz``).  Config sections are the ones of ``config/semi.yaml``.

Own structure: a trainer is (a) the config sections it reads in ``_init`` and (b) ONE ``_make_epocher`` that builds the
epoch object; the loop, evaluation, checkpointing and logging live once in ``SemiTrainer``.  Data-parallel runs (one
process per GPU, RCCL over xGMI) are part of the loop, not bolted on: ``attach_data_parallel`` gives the optimiser's flat
gradient buffer a ``miseg_amd.ddp.GradReducer``, every epocher is handed that reducer, every rank evaluates (identical
weights, identical scores) and only rank 0 writes ``last.pth`` / ``best.pth`` / ``storage.csv`` / TensorBoard.
"""
from __future__ import annotations

from itertools import chain
from pathlib import Path
from typing import Optional, Tuple

import torch
from torch import nn

from contrastyou import PROJECT_PATH
from deepclustering2 import optim
from deepclustering2.loss import KL_div
from deepclustering2.meters2 import EpochResultDict, StorageIncomeDict
from deepclustering2.schedulers import GradualWarmupScheduler
from deepclustering2.trainer import Trainer
from deepclustering2.type import T_loader, T_loss
from semi_seg import epocher as E
from semi_seg._utils import IICLossWrapper, ProjectorWrapper

__all__ = ["trainer_zoos"]

_CONSISTENCY = {"mse": nn.MSELoss, "kl": KL_div}   # UDARegCriterion.name (config/semi.yaml:31-33)
_COSINE_FLOOR = 1e-7                               # eta_min of the cosine phase (ref trainer.py:57-60)


def _consistency_section(section: dict) -> Tuple[nn.Module, float]:
    return _CONSISTENCY[section["name"]](), float(section["weight"])


def _checkpoint_file(checkpoint, default_dir) -> Path:
    """``None`` -> ``<save_dir>/best.pth``; a directory -> its ``best.pth``; a file must be a ``.pth``."""
    if checkpoint is None:
        return Path(default_dir) / "best.pth"
    path = Path(checkpoint)
    if path.is_dir():
        return path / "best.pth"
    if path.is_file() and path.suffix == ".pth":
        return path
    raise FileNotFoundError(path)


class SemiTrainer(Trainer):
    """``partial``: supervised KL on the labeled batch only (the unlabeled loader is drawn but unused)."""

    RUN_PATH = str(Path(PROJECT_PATH) / "semi_seg" / "runs")  # noqa
    feature_positions = ["Up_conv4", "Up_conv3"]
    SINGLE_PROCESS: Optional[str] = None     # why the trainer refuses data-parallel runs, worded after its ``NAME`` (None: it takes them)

    def __init__(self, *, model: nn.Module, labeled_loader: T_loader, unlabeled_loader: T_loader, val_loader: T_loader,
                 test_loader: T_loader, sup_criterion: T_loss, save_dir: str = "base", max_epoch: int = 100,
                 num_batches: int = 100, device: str = "cpu", configuration=None, **kwargs):
        super().__init__(model, save_dir, max_epoch, num_batches, device, configuration)
        self._labeled_loader, self._unlabeled_loader = labeled_loader, unlabeled_loader
        self._val_loader, self._test_loader = val_loader, test_loader
        self._sup_criterion = sup_criterion
        self._grad_reducer = None

    # ------------------------------------------------------------------ set-up
    def init(self) -> None:
        self._init()
        self._init_optimizer()
        self._init_scheduler(self._optimizer)

    def _init(self) -> None:
        section = self._config["Trainer"]
        # arithmetic of the local-MI contraction: Arch.mi_precision, else by Arch.compute_dtype (f16f8 for bfloat16 / float16)
        from miseg_amd import ops
        net = getattr(self._model, "module", self._model)
        ops.set_mi_precision(ops.resolve_mi_precision(getattr(net, "compute_dtype", None), getattr(net, "mi_precision", None)))
        self.set_feature_positions(section["feature_names"])
        raw = section["feature_importance"]
        assert isinstance(raw, list), type(raw)
        weights = [float(v) for v in raw]
        assert len(weights) == len(self.feature_positions), (weights, self.feature_positions)
        total = sum(weights)
        self._feature_importance = [v / total for v in weights]

    def _trainable(self):
        return self._model.parameters()

    def _init_optimizer(self) -> None:
        section = dict(self._config["Optim"])
        factory = optim.__dict__[section.pop("name")]        # ``Adam`` resolves to the fused flat-buffer HIP Adam
        self._optimizer = factory(params=self._trainable(), **section)

    def _init_scheduler(self, optimizer) -> None:
        section = self._config.get("Scheduler")
        if section is None:
            return
        warm = section["warmup_max"]
        cosine = torch.optim.lr_scheduler.CosineAnnealingLR(optimizer, T_max=self._config["Trainer"]["max_epoch"] - warm,
                                                            eta_min=_COSINE_FLOOR)
        self._scheduler = GradualWarmupScheduler(optimizer, section["multiplier"], total_epoch=warm, after_scheduler=cosine)

    @classmethod
    def set_feature_positions(cls, feature_positions) -> None:
        cls.feature_positions = feature_positions           # class-wide, as in the reference (trainer.py:127-129)

    def attach_data_parallel(self, num_buckets: int = 3):
        """One process per GPU: bucketed RCCL all-reduce of the flat gradient, launched from autograd hooks
        (``miseg_amd.ddp``).  No-op (returns None) when torch.distributed is not initialised or has a single rank.  A trainer with a
        ``SINGLE_PROCESS`` reason refuses a multi-rank run."""
        if self.SINGLE_PROCESS is not None:
            import torch.distributed as dist
            if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
                raise RuntimeError(f"Trainer.name={self.NAME} runs in a single process: {self.SINGLE_PROCESS}")
            return None
        from miseg_amd import ddp
        return ddp.attach(self, num_buckets=num_buckets)

    def _refuse_float16(self) -> None:
        """For the trainers that say in ``NO_FLOAT16`` what they lack for ``Arch.compute_dtype=float16``; called from their ``_init``."""
        if getattr(self._model, "compute_dtype", torch.float32) == torch.float16:
            raise NotImplementedError(f"Trainer.name={self.NAME} {self.NO_FLOAT16}: use Arch.compute_dtype float32 or bfloat16")

    # ------------------------------------------------------------------ one epoch
    def _epoch_args(self) -> dict:
        return dict(num_batches=self._num_batches, cur_epoch=self._cur_epoch, device=self._device,
                    feature_position=self.feature_positions, feature_importance=self._feature_importance)

    def _make_epocher(self):
        return E.TrainEpocher(self._model, self._optimizer, self._labeled_loader, self._unlabeled_loader, self._sup_criterion, 0,
                              **self._epoch_args())

    def _run_epoch(self, *args, **kwargs) -> EpochResultDict:
        epocher = self._make_epocher()
        epocher._reducer = self._grad_reducer
        return epocher.run()

    def _eval_epoch(self, *, loader: T_loader, **kwargs) -> Tuple[EpochResultDict, float]:
        return E.EvalEpocher(self._inference_model(), val_loader=loader, sup_criterion=self._sup_criterion, cur_epoch=self._cur_epoch,
                             device=self._device).run()

    # ------------------------------------------------------------------ the loop
    def _start_training(self) -> None:
        for epoch in range(self._start_epoch, self._max_epoch):
            self._cur_epoch = epoch
            trained = self.run_epoch()
            with torch.no_grad():
                validated, score = self.eval_epoch(loader=self._val_loader)
                tested, _ = self.eval_epoch(loader=self._test_loader)
            scheduler = getattr(self, "_scheduler", None)
            if scheduler is not None:
                scheduler.step()
            self._log_epoch(StorageIncomeDict(tra=trained, val=validated, test=tested), score)

    def _log_epoch(self, record: StorageIncomeDict, score: float) -> None:
        """History, TensorBoard, ``last.pth`` / ``best.pth``, ``storage.csv`` -- the writing rank only.  Every rank tracks
        ``_best_score`` so that all ranks agree on it if the writer role ever moves."""
        self._storage.put_from_dict(record, self._cur_epoch)
        if not self.is_writer:
            self._best_score = max(self._best_score, score)
            return
        self._writer.add_scalar_with_StorageDict(record, self._cur_epoch)
        self.save(score)
        self._storage.to_csv(self._save_dir)

    # ------------------------------------------------------------------ inference
    def _inference_model(self) -> nn.Module:
        """The network that validation, test and ``inference`` evaluate."""
        return self._model

    def inference(self, checkpoint=None, surface_metrics=None, keep_largest=None):  # noqa
        """``surface_metrics``: ``SurfaceMeter`` names to report (``hausdorff`` -> ``hd``, ``mod_hausdorff`` -> ``mhd``,
        ``average_surface`` -> ``asd``); None reads the optional ``Inference.surface_metrics`` of the configuration, whose default is
        the reference's ``("hausdorff",)``.  ``keep_largest``: also report the prediction with only the largest connected component
        of each foreground class kept (``InferenceEpocher``: the ``*_lcc`` meters and ``pred_lcc/``); None reads the optional
        ``Inference.keep_largest_component`` (default false) and ``Inference.component_connectivity`` (default 1).  The returned
        score is the raw prediction's DSC_mean either way."""
        if checkpoint is not None and not Path(checkpoint).exists():
            raise AssertionError(checkpoint)         # the reference asserts the path (semi_seg/trainer.py:112-115) before resolving it
        target = _checkpoint_file(checkpoint, self._save_dir)
        self.load_state_dict_from_path(str(target), strict=True)
        if surface_metrics is None:
            surface_metrics = (self._config.get("Inference") or {}).get("surface_metrics") or ("hausdorff",)
        if keep_largest is None:
            keep_largest = bool((self._config.get("Inference") or {}).get("keep_largest_component", False))
        connectivity = int((self._config.get("Inference") or {}).get("component_connectivity", 1))
        runner = E.InferenceEpocher(self._inference_model(), val_loader=self._test_loader, sup_criterion=self._sup_criterion,
                                    cur_epoch=self._cur_epoch, device=self._device, surface_metrics=tuple(surface_metrics),
                                    keep_largest=bool(keep_largest), component_connectivity=connectivity)
        runner.set_save_dir(self._save_dir)
        return runner.run()


class UDATrainer(SemiTrainer):
    """``uda``: + ``weight`` x consistency between f(flip(x)) and flip(f(x))."""

    def _init(self) -> None:
        super()._init()
        self._reg_criterion, self._reg_weight = _consistency_section(self._config["UDARegCriterion"])

    def _make_epocher(self):
        return E.UDATrainEpocher(self._model, self._optimizer, self._labeled_loader, self._unlabeled_loader, self._sup_criterion,
                                 reg_criterion=self._reg_criterion, reg_weight=self._reg_weight, **self._epoch_args())


class IICTrainer(SemiTrainer):
    """``iic``: + ``weight`` x importance-weighted IIC mutual information over the tapped features; the projector heads
    are trained with the network."""

    def _init(self) -> None:
        super()._init()
        section = self._config["IICRegParameters"]
        heads = ProjectorWrapper()
        heads.init_encoder(feature_names=self.feature_positions, **section["EncoderParams"])
        heads.init_decoder(feature_names=self.feature_positions, **section["DecoderParams"])
        self._projector_wrappers = heads
        self._IIDSegWrapper = IICLossWrapper(feature_names=self.feature_positions, **section["LossParams"])
        self._reg_weight = float(section["weight"])

    def _trainable(self):
        return chain(self._model.parameters(), self._projector_wrappers.parameters())

    def _make_epocher(self):
        return E.IICTrainEpocher(self._model, self._projector_wrappers, self._optimizer, self._labeled_loader, self._unlabeled_loader,
                                 self._sup_criterion, IIDSegCriterionWrapper=self._IIDSegWrapper, reg_weight=self._reg_weight,
                                 **self._epoch_args())


class UDAIICTrainer(IICTrainer):
    """``udaiic``: ``UDARegCriterion.weight`` x consistency + ``IICRegParameters.weight`` x IIC; the combined
    regulariser enters the loss with weight 1 (ref trainer.py:187-196, epocher.py:294-296)."""

    def _init(self) -> None:
        super()._init()
        self._iic_weight, self._reg_weight = self._reg_weight, 1.0
        self._reg_criterion, self._uda_weight = _consistency_section(self._config["UDARegCriterion"])

    def _make_epocher(self):
        return E.UDAIICEpocher(self._model, self._projector_wrappers, self._optimizer, self._labeled_loader, self._unlabeled_loader,
                               self._sup_criterion, self._reg_criterion, self._IIDSegWrapper, cons_weight=self._uda_weight,
                               iic_weight=self._iic_weight, **self._epoch_args())


class MeanTeacherTrainer(SemiTrainer):
    """``meanteacher``: the baseline of the paper's comparisons (ref contrastyou/trainer/contrast_trainer.py:235-262).  The student
    is trained with ``MeanTeacherParameters.weight`` x consistency (``name``: mse | kl) against a teacher -- a second ``UNet(**Arch)``
    with its own initialisation and no gradients -- that follows the student as an exponential moving average
    (``alpha``, ``weight_decay``; ``deepclustering2.models.ema_updater``).  Validation, test and ``inference`` evaluate the TEACHER
    (ref :261), so the best checkpoint is the teacher's best.  Checkpoints carry ``_teacher_model`` and ``_ema_updater``."""

    def _init(self) -> None:
        super()._init()
        from contrastyou.arch import UNet
        from deepclustering2.models import ema_updater
        section = self._teacher_section()
        self._reg_criterion, self._reg_weight = _consistency_section(section)
        self._teacher_model = UNet(**self._config["Arch"])
        for param in self._teacher_model.parameters():
            param.detach_()
            param.requires_grad_(False)
        self._teacher_model.train()
        self._ema_updater = ema_updater(alpha=float(section["alpha"]), justify_alpha=True, weight_decay=float(section["weight_decay"]),
                                        update_bn=False)

    def _teacher_section(self) -> dict:
        """The section with the consistency term (``name``, ``weight``) and the EMA (``alpha``, ``weight_decay``)."""
        return self._config["MeanTeacherParameters"]

    def _make_epocher(self):
        return E.MeanTeacherEpocher(self._model, self._teacher_model, self._optimizer, self._labeled_loader, self._unlabeled_loader,
                                    self._sup_criterion, reg_criterion=self._reg_criterion, reg_weight=self._reg_weight,
                                    ema_updater=self._ema_updater, **self._epoch_args())

    def _inference_model(self):
        return self._teacher_model


class ICTTrainer(MeanTeacherTrainer):
    """``ict``: interpolation consistency training (Verma et al. 2019, the "MixUp" row of the semi-supervised comparisons) -- a Mean
    Teacher whose student sees ``lam * u_i + (1 - lam) * u_perm[i]`` of two unlabeled images and is held, with ``ICTParameters.weight``
    x consistency (``name``: mse | kl), to the same mix of the teacher's two predictions; ``lam ~ Beta(mix_alpha, mix_alpha)`` and the
    permutation are drawn every iteration.  The section is optional: missing keys take the class's defaults.  Teacher, EMA
    (``alpha``, ``weight_decay``), checkpoint tree and evaluation are ``meanteacher``'s.  Semantics: DESIGN.md section 27."""

    DEFAULTS = dict(name="mse", weight=10.0, alpha=0.999, weight_decay=0.000001, mix_alpha=1.0)
    NAME = "ict"

    @classmethod
    def parameters(cls, configuration) -> dict:
        """``ICTParameters`` of a configuration over the defaults; unknown keys are an error, and so is ``mix_alpha <= 0``."""
        section = dict((configuration or {}).get("ICTParameters") or {})
        unknown = sorted(set(section) - set(cls.DEFAULTS))
        if unknown:
            raise KeyError(f"ICTParameters: unknown keys {unknown}; known: {sorted(cls.DEFAULTS)}")
        merged = {**cls.DEFAULTS, **section}
        if str(merged["name"]) not in _CONSISTENCY:
            raise KeyError(f"ICTParameters.name={merged['name']}: one of {sorted(_CONSISTENCY)}")
        if not float(merged["mix_alpha"]) > 0.0:
            raise ValueError(f"ICTParameters.mix_alpha={merged['mix_alpha']}: the Beta distribution needs a positive parameter")
        return dict(name=str(merged["name"]), weight=float(merged["weight"]), alpha=float(merged["alpha"]),
                    weight_decay=float(merged["weight_decay"]), mix_alpha=float(merged["mix_alpha"]))

    def _teacher_section(self) -> dict:
        params = self.parameters(self._config)
        self._mix_alpha = params.pop("mix_alpha")
        return params

    def _make_epocher(self):
        return E.ICTEpocher(self._model, self._teacher_model, self._optimizer, self._labeled_loader, self._unlabeled_loader,
                            self._sup_criterion, reg_criterion=self._reg_criterion, reg_weight=self._reg_weight,
                            ema_updater=self._ema_updater, mix_alpha=self._mix_alpha, **self._epoch_args())


class UAMTTrainer(MeanTeacherTrainer):
    """``uamt``: the uncertainty-aware Mean Teacher (Yu et al., MICCAI 2019) -- a Mean Teacher whose teacher sees the unlabeled batch
    under clipped Gaussian noise (``noise_sigma``, ``noise_clip``), runs ``passes`` more stochastic forwards for a per-pixel predictive
    entropy, and whose ``UAMTParameters.weight`` x squared-distance consistency counts only where that entropy lies below a threshold
    ramping from ``threshold_start`` to ``threshold_end`` (fractions of ``ln C``) over the run.  The section is optional: missing keys
    take the class's defaults.  Teacher, EMA (``alpha``, ``weight_decay``), checkpoint tree and evaluation are ``meanteacher``'s.
    Semantics: DESIGN.md section 28."""

    DEFAULTS = dict(name="mse", weight=0.1, alpha=0.99, weight_decay=0.000001, passes=8, noise_sigma=0.1, noise_clip=0.2,
                    threshold_start=0.75, threshold_end=1.0)
    NAME = "uamt"
    SINGLE_PROCESS = "the count of certain pixels would have to be all-reduced before the gradient is scaled"

    @classmethod
    def parameters(cls, configuration) -> dict:
        """``UAMTParameters`` of a configuration over the defaults.  ``KeyError``: an unknown key, a ``name`` other than mse (UA-MT
        defines no KL form); ``ValueError``: ``passes`` outside 1..32, a negative ``noise_sigma`` / ``noise_clip`` / threshold,
        ``threshold_start > threshold_end``."""
        section = dict((configuration or {}).get("UAMTParameters") or {})
        unknown = sorted(set(section) - set(cls.DEFAULTS))
        if unknown:
            raise KeyError(f"UAMTParameters: unknown keys {unknown}; known: {sorted(cls.DEFAULTS)}")
        merged = {**cls.DEFAULTS, **section}
        if str(merged["name"]) != "mse":
            raise KeyError(f"UAMTParameters.name={merged['name']}: mse (the masked term has no KL form)")
        out = dict(name="mse", weight=float(merged["weight"]), alpha=float(merged["alpha"]), weight_decay=float(merged["weight_decay"]),
                   passes=int(merged["passes"]), noise_sigma=float(merged["noise_sigma"]), noise_clip=float(merged["noise_clip"]),
                   threshold_start=float(merged["threshold_start"]), threshold_end=float(merged["threshold_end"]))
        if float(merged["passes"]) != out["passes"] or not 1 <= out["passes"] <= 32:
            raise ValueError(f"UAMTParameters.passes={merged['passes']}: a whole number in 1..32")
        if out["noise_sigma"] < 0.0 or out["noise_clip"] < 0.0:
            raise ValueError(f"UAMTParameters: noise_sigma={out['noise_sigma']} and noise_clip={out['noise_clip']} must not be negative")
        if out["threshold_start"] < 0.0 or out["threshold_end"] < 0.0 or out["threshold_start"] > out["threshold_end"]:
            raise ValueError(f"UAMTParameters: 0 <= threshold_start={out['threshold_start']} <= threshold_end={out['threshold_end']}")
        return out

    def _teacher_section(self) -> dict:
        params = self.parameters(self._config)
        self._uamt = {k: params.pop(k) for k in ("passes", "noise_sigma", "noise_clip", "threshold_start", "threshold_end")}
        return params

    def _make_epocher(self):
        return E.UAMTEpocher(self._model, self._teacher_model, self._optimizer, self._labeled_loader, self._unlabeled_loader,
                             self._sup_criterion, reg_criterion=self._reg_criterion, reg_weight=self._reg_weight,
                             ema_updater=self._ema_updater, k_total=self._max_epoch * self._num_batches, **self._uamt,
                             **self._epoch_args())


class CPSTrainer(SemiTrainer):
    """``cps``: cross pseudo supervision (Chen et al., CVPR 2021) -- two segmentation networks, ``_model`` (A) and ``_model_b`` (B, a
    second ``UNet(**Arch)`` with its own initialisation), trained together: each on the supervised loss of the labeled batch and, with
    ``CPSParameters.weight``, on the cross entropy against the OTHER network's hard prediction (over every image with ``on_labeled``,
    the paper's form; over the unlabeled ones only without).  Both networks' parameters sit in the one fused optimiser.  The section is
    optional: missing keys take the class's defaults.  Checkpoints carry ``_model_b``.  Validation, test and ``inference`` evaluate
    network A, as in the paper.  ``Pretrained=`` loads network A only: B keeps its own initialisation, the difference between the two
    being what the method feeds on.  Semantics: DESIGN.md section 30."""

    DEFAULTS = dict(weight=1.5, on_labeled=True)
    NAME = "cps"

    @classmethod
    def parameters(cls, configuration) -> dict:
        """``CPSParameters`` of a configuration over the defaults; an unknown key is a ``KeyError``, a negative weight a ``ValueError``."""
        section = dict((configuration or {}).get("CPSParameters") or {})
        unknown = sorted(set(section) - set(cls.DEFAULTS))
        if unknown:
            raise KeyError(f"CPSParameters: unknown keys {unknown}; known: {sorted(cls.DEFAULTS)}")
        merged = {**cls.DEFAULTS, **section}
        if not float(merged["weight"]) >= 0.0:
            raise ValueError(f"CPSParameters.weight={merged['weight']}: must not be negative")
        return dict(weight=float(merged["weight"]), on_labeled=bool(merged["on_labeled"]))

    def _init(self) -> None:
        super()._init()
        from contrastyou.arch import UNet
        params = self.parameters(self._config)
        self._reg_weight, self._on_labeled = params["weight"], params["on_labeled"]
        self._model_b = UNet(**self._config["Arch"])
        self._model_b.train()

    def _trainable(self):
        return chain(self._model.parameters(), self._model_b.parameters())

    def _make_epocher(self):
        return E.CPSEpocher(self._model, self._model_b, self._optimizer, self._labeled_loader, self._unlabeled_loader, self._sup_criterion,
                            reg_weight=self._reg_weight, on_labeled=self._on_labeled, **self._epoch_args())


class MIDLTrainer(UDATrainer):
    """``midl``: ``UDARegCriterion.weight`` x consistency + ``MIDLPaperParameters.iic_weight`` x the local mutual information of the
    network's output (``IIDSegmentationSmallPathLoss(padding, patch_size)`` on softmax(flip(f(x))) and softmax(f(flip(x)))); the
    combined regulariser enters the loss with weight 1, as udaiic's.  No new modules: the checkpoint tree is the ``uda`` trainer's, and
    validation, test and ``inference`` evaluate the model as for ``uda``.  Semantics: DESIGN.md section 12."""

    def _init(self) -> None:
        super()._init()
        section = self._config["MIDLPaperParameters"]
        self._uda_weight, self._reg_weight = self._reg_weight, 1.0
        self._iic_weight = float(section["iic_weight"])
        self._mi_padding, self._mi_patch_size = int(section["padding"]), int(section["patch_size"])

    def mi_criterion(self):
        """The MI term's criterion (the reference's class and its patch / step sizes); built where it is used, so that the trainer's
        checkpoint tree stays the ``uda`` one."""
        from contrastyou.losses.iic_loss import IIDSegmentationSmallPathLoss
        return IIDSegmentationSmallPathLoss(lamda=1.0, padding=self._mi_padding, patch_size=self._mi_patch_size)

    def _make_epocher(self):
        return E.MIDLTrainEpocher(self._model, self._optimizer, self._labeled_loader, self._unlabeled_loader, self._sup_criterion,
                                  self._reg_criterion, cons_weight=self._uda_weight, iic_weight=self._iic_weight,
                                  padding=self._mi_padding, patch_size=self._mi_patch_size, **self._epoch_args())


class EntropyMinTrainer(SemiTrainer):
    """``entmin``: + ``EntropyMinParameters.weight`` x the mean entropy of the prediction on the unlabeled batch
    (``Entropy()(softmax(flip(f(x))))``, one fused kernel).  No new modules -- the criterion is built inside the epocher --, so the
    checkpoint tree is the ``partial`` trainer's, and validation, test and ``inference`` are ``partial``'s.  Semantics: DESIGN.md
    section 13."""

    def _init(self) -> None:
        super()._init()
        self._reg_weight = float(self._config["EntropyMinParameters"]["weight"])

    def _make_epocher(self):
        return E.EntropyMinEpocher(self._model, self._optimizer, self._labeled_loader, self._unlabeled_loader, self._sup_criterion,
                                   reg_weight=self._reg_weight, **self._epoch_args())


class VATTrainer(SemiTrainer):
    """``vat``: + ``VATParameters.weight`` x the virtual adversarial loss of the unlabeled batch (``deepclustering2.utils.VAT.VATLoss``
    with ``xi``, ``eps``, ``prop_eps``, ``ip``: a clean pass, ``ip`` direction passes that end in the gradient with respect to the image,
    one perturbed pass).  The section is optional: missing keys take the class's defaults and ``weight`` 1.  No new modules -- the
    criterion is built inside the epocher --, so the checkpoint tree is the ``partial`` trainer's, and validation, test and
    ``inference`` are ``partial``'s.  ``Arch.compute_dtype=float16`` is refused (no loss scaling in the direction pass), and so are
    data-parallel runs.  Semantics: DESIGN.md section 23."""

    DEFAULTS = dict(weight=1.0, xi=10.0, eps=1.0, prop_eps=0.25, ip=1)
    NAME = "vat"
    NO_FLOAT16 = "has no loss scaling in its direction pass"
    SINGLE_PROCESS = "the gradient reducer's hooks would also fire in the direction pass"

    @classmethod
    def parameters(cls, configuration) -> dict:
        """``VATParameters`` of a configuration over the defaults; unknown keys are an error."""
        section = dict((configuration or {}).get("VATParameters") or {})
        unknown = sorted(set(section) - set(cls.DEFAULTS))
        if unknown:
            raise KeyError(f"VATParameters: unknown keys {unknown}; known: {sorted(cls.DEFAULTS)}")
        merged = {**cls.DEFAULTS, **section}
        return dict(weight=float(merged["weight"]), xi=float(merged["xi"]), eps=float(merged["eps"]), prop_eps=float(merged["prop_eps"]),
                    ip=int(merged["ip"]))

    def _init(self) -> None:
        super()._init()
        self._refuse_float16()
        params = self.parameters(self._config)
        self._reg_weight = params.pop("weight")
        self._vat_params = params

    def _make_epocher(self):
        return E.VATEpocher(self._model, self._optimizer, self._labeled_loader, self._unlabeled_loader, self._sup_criterion,
                            reg_weight=self._reg_weight, **self._vat_params, **self._epoch_args())


class ContrastTrainer(SemiTrainer):
    """``contrast``: contrastive pre-training of the encoder (the encoder stage of ref contrastyou/trainer/contrast_trainer.py:64-114;
    DESIGN.md section 14).  ``unlabeled_loader`` is the pre-training loader; the labeled, validation and test loaders are accepted and
    unused.  One epoch = one ``PretrainEncoderEpocher``, then the scheduler, the history / TensorBoard / ``storage.csv`` and
    ``last.pth``; nothing is evaluated and no ``best.pth`` is written.  Fine-tune from the result with any other trainer and
    ``Pretrained=<run dir | .pth>`` (semi_seg/main.py).

    Reads ``ContrastParameters`` (defaults: config/contrast.yaml, merged under the given configuration).  Only ``Conv1 ..
    extract_position`` and the projector are trained -- and only they are handed to the optimiser, so every other parameter stays bit
    for bit.  Checkpoints carry ``_model``, ``_projector``, ``_optimizer``, ``_scheduler``, ``_contrastive_criterion``, ``_storage``."""

    DEFAULTS = Path(PROJECT_PATH) / "config" / "contrast.yaml"
    SECTION = "ContrastParameters"
    NAME, STAGE = "contrast", "encoder"
    NO_FLOAT16 = "has no loss scaling"
    SINGLE_PROCESS = "a cross-rank contrastive loss needs an all-gather of the embeddings, which is not implemented"

    def __init__(self, *, configuration=None, **kwargs):
        import yaml
        shipped = yaml.safe_load(open(str(self.DEFAULTS)))[self.SECTION]
        configuration = dict(configuration or {})
        configuration[self.SECTION] = {**shipped, **(configuration.get(self.SECTION) or {})}
        super().__init__(configuration=configuration, **kwargs)

    def _init(self) -> None:
        super()._init()
        from contrastyou.arch import UNet
        from contrastyou.losses.contrast_loss import SupConLoss
        from contrastyou.trainer._utils import ProjectionHead
        section = self._config["ContrastParameters"]
        self._group_option, self._extract_position = str(section["group_option"]), str(section["extract_position"])
        assert self._group_option in ("partition", "patient", "both"), self._group_option
        if self._extract_position not in UNet.dimension_dict:
            raise ValueError(f"ContrastParameters.extract_position={self._extract_position}: one of {sorted(UNet.dimension_dict)}")
        self._refuse_float16()
        self._projector = ProjectionHead(input_dim=UNet.dimension_dict[self._extract_position], output_dim=int(section["output_dim"]),
                                         head_type=str(section["ptype"]))
        self._contrastive_criterion = SupConLoss(temperature=float(section["temperature"]),
                                                 base_temperature=float(section["base_temperature"]))
        self._model.disable_grad_all()
        self._model.enable_grad(from_="Conv1", util=self._extract_position)

    def _trainable(self):
        """The parameters of ``Conv1 .. extract_position`` and the projector's.  The reference hands Adam every parameter and relies on
        ``grad is None`` to skip the rest; the flat fused Adam zero-fills such slots and would still decay them."""
        blocks = self._model._range("Conv1", self._extract_position)
        return chain(*(getattr(self._model, name).parameters() for name in blocks), self._projector.parameters())

    def _make_epocher(self):
        return E.PretrainEncoderEpocher(self._model, self._projector, self._optimizer, self._unlabeled_loader, self._contrastive_criterion,
                                        num_batches=self._num_batches, cur_epoch=self._cur_epoch, device=self._device,
                                        group_option=self._group_option, extract_position=self._extract_position)

    def _run_epoch(self, *args, **kwargs) -> EpochResultDict:
        return self._make_epocher().run()

    def _start_training(self) -> None:
        for epoch in range(self._start_epoch, self._max_epoch):
            self._cur_epoch = epoch
            trained = self.run_epoch()
            scheduler = getattr(self, "_scheduler", None)
            if scheduler is not None:
                scheduler.step()
            record = StorageIncomeDict(tra=trained)
            self._storage.put_from_dict(record, self._cur_epoch)
            if self.is_writer:
                self._writer.add_scalar_with_StorageDict(record, self._cur_epoch)
                self._save_to("last.pth")
                self._storage.to_csv(self._save_dir)

    def _eval_epoch(self, *args, **kwargs):
        raise NotImplementedError(f"Trainer.name={self.NAME} pre-trains the {self.STAGE} and evaluates nothing: fine-tune with another trainer and "
                                  "Pretrained=<this run's directory>, and evaluate that")

    def inference(self, checkpoint=None):  # noqa
        raise NotImplementedError(f"Trainer.name={self.NAME} has no segmentation to infer: fine-tune with another trainer and "
                                  "Pretrained=<this run's directory>, and run inference on that")


class ContrastDecoderTrainer(ContrastTrainer):
    """``contrastdecoder``: contrastive pre-training of the decoder (the decoder stage of ref
    contrastyou/trainer/contrast_trainer.py:116-170), between ``contrast`` (``Pretrained=<its run>`` on the way
    in) and the fine-tune (``Pretrained=<this run>`` on the way out).  One epoch = one ``PretrainDecoderEpocher``; the loop, ``last.pth``
    and what is refused are ``ContrastTrainer``'s.

    Reads ``ContrastDecoderParameters`` (defaults: config/contrast_decoder.yaml, merged under the given configuration).  Gradients
    are enabled for ``enable_grad_from .. extract_position`` only, and only those blocks and the projector are handed to the
    optimiser; the encoder runs in train mode with frozen weights (its BatchNorm running statistics move, as in the reference).  The
    pre-training loader's recipe is replaced by its ``total_freedom=False`` copy: both views share the geometric transform."""

    DEFAULTS = Path(PROJECT_PATH) / "config" / "contrast_decoder.yaml"
    SECTION = "ContrastDecoderParameters"
    NAME, STAGE = "contrastdecoder", "decoder"

    def _init(self) -> None:
        SemiTrainer._init(self)
        from contrastyou.arch import UNet
        from contrastyou.losses.contrast_loss import SupConLoss
        from contrastyou.trainer._utils import LocalProjectionHead
        section = self._config[self.SECTION]
        self._extract_position, self._enable_grad_from = str(section["extract_position"]), str(section["enable_grad_from"])
        if self._extract_position not in UNet.dimension_dict:
            raise ValueError(f"{self.SECTION}.extract_position={self._extract_position}: one of {sorted(UNet.dimension_dict)}")
        names = list(self._model.component_names)
        if self._enable_grad_from not in names or names.index(self._enable_grad_from) > names.index(self._extract_position):
            raise ValueError(f"{self.SECTION}.enable_grad_from={self._enable_grad_from}: a block at or before {self._extract_position} in {names}")
        self._refuse_float16()
        self._output_size = tuple(int(v) for v in section["output_size"])
        self._partition_num = tuple(int(v) for v in section["partition_num"])
        if len(self._output_size) != 2 or len(self._partition_num) != 2 or any(o % p for o, p in zip(self._output_size, self._partition_num)):
            raise ValueError(f"{self.SECTION}: output_size {self._output_size} must be a multiple of partition_num {self._partition_num}")
        self._projector = LocalProjectionHead(input_dim=UNet.dimension_dict[self._extract_position], head_type=str(section["ptype"]),
                                              output_size=self._output_size)
        self._contrastive_criterion = SupConLoss(temperature=float(section["temperature"]),
                                                 base_temperature=float(section["base_temperature"]))
        self._model.disable_grad_all()
        self._model.enable_grad(from_=self._enable_grad_from, util=self._extract_position)
        self._use_shared_geometry()

    def _use_shared_geometry(self) -> None:
        """Give the pre-training loader's dataset the ``total_freedom=False`` copy of its recipe (ref contrast_trainer.py:136-138).
        Loaders without a recipe (the synthetic ones) yield what they yield."""
        import dataclasses
        dataset = getattr(self._unlabeled_loader, "dataset", None)
        recipe = getattr(dataset, "transform", None)
        if dataclasses.is_dataclass(recipe) and hasattr(recipe, "total_freedom") and hasattr(dataset, "set_transform"):
            dataset.set_transform(dataclasses.replace(recipe, total_freedom=False))

    def _trainable(self):
        """The parameters of ``enable_grad_from .. extract_position`` and the projector's (see ``ContrastTrainer._trainable``)."""
        blocks = self._model._range(self._enable_grad_from, self._extract_position)
        return chain(*(getattr(self._model, name).parameters() for name in blocks), self._projector.parameters())

    def _make_epocher(self):
        return E.PretrainDecoderEpocher(self._model, self._projector, self._optimizer, self._unlabeled_loader, self._contrastive_criterion,
                                        num_batches=self._num_batches, cur_epoch=self._cur_epoch, device=self._device,
                                        extract_position=self._extract_position, partition_num=self._partition_num)


trainer_zoos = {"partial": SemiTrainer, "uda": UDATrainer, "iic": IICTrainer, "udaiic": UDAIICTrainer, "meanteacher": MeanTeacherTrainer,
                "midl": MIDLTrainer, "entmin": EntropyMinTrainer, "vat": VATTrainer, "contrast": ContrastTrainer,
                "contrastdecoder": ContrastDecoderTrainer, "ict": ICTTrainer, "uamt": UAMTTrainer, "cps": CPSTrainer}
