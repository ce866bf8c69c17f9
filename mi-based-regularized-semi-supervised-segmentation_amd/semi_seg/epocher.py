"""Train / eval epochers of the semi-supervised segmentation step on the MI355X kernels.

Drop-in for ref ``semi_seg/epocher.py``: same classes, constructor signatures and meter names
(``lr, sup_loss, reg_loss, sup_dice{DSC1..,DSC_mean}, mi, individual_mis{<feature>}, uda, iic_weight,
uda_weight``).  One step = one U-Net forward on cat[labeled, unlabeled, flip(unlabeled)], supervised KL,
regulariser, one backward, Adam (ref :137-188).  What changed underneath:

* the per-sample ``clone().flip()`` Python loops (ref :148-149, :160-161, :264-266) became index math:
  decisions are still drawn from Python's ``random`` under ``FixRandomSeed(seed)`` in the reference's
  order, packed into an int32 bit-mask tensor and applied inside the consuming kernels;
* ``softmax -> one-hot -> KL`` (ref :165-166) and ``softmax, softmax -> MSE`` (ref :221-224) are single
  fused kernels with fused backward;
* slicing / chunking / cat of tapped features and the five sub-heads (ref :258-273) are one gather-fused
  launch per tap; the IIC losses run on the MFMA joint kernels;
* the ~7 ``.item()`` host syncs per iteration (ref :182-185, :225, :278-282) are ONE device-to-host copy
  of all meter scalars.
"""
from __future__ import annotations

import math
import os
import random
from typing import List, Optional, Tuple, Union

import numpy as np
import torch
from torch import Tensor, nn

from contrastyou.epocher._utils import preprocess_input_with_single_transformation  # noqa
from contrastyou.epocher._utils import preprocess_input_with_twice_transformation  # noqa
from contrastyou.epocher._utils import (GlobalLabelGenerator, LocalLabelGenerator, write_img_target, write_predict,
                                        write_prediction_map)
from contrastyou.helper import average_iter, weighted_average_iter
from contrastyou.trainer._utils import ClusterHead  # noqa
from deepclustering2.augment.tensor_augment import TensorRandomFlip
from deepclustering2.decorator import FixRandomSeed
from deepclustering2.epoch import _Epocher  # noqa
from deepclustering2.loss import Entropy, GeneralizedDiceLoss, KL_div
from deepclustering2.meters2 import (AverageValueMeter, EpochResultDict, MeterInterface, MultipleAverageValueMeter, SurfaceMeter,
                                     UniversalDice)
from deepclustering2.optim import get_lrs_from_optimizer
from deepclustering2.type import T_loader, T_loss, T_optim
from deepclustering2.utils import class2one_hot
from miseg_amd import checks, lazy, ops, packcache, stepio, unet_ops
from miseg_amd.lazy import LinearLoss
from miseg_amd.tape import keep as _keep
from semi_seg._utils import FeatureExtractor, IICLossWrapper, KLDiceLoss, ProjectorWrapper

_DEBUG_ASSERTS = os.environ.get("MISEG_ASSERTS", "0") == "1"
_READBACK_EARLY = os.environ.get("MISEG_READBACK_EARLY", "1") != "0"     # Dice counts + report launched before backward (0: after it, on the step's tail)
_GUARD_STEP = os.environ.get("MISEG_GUARD_STEP", "1") != "0"   # a failed deferred check turns the iteration's Adam launch into a no-op


def _fused(fn):
    fn._miseg_fused = True
    return fn


class _num_class_mixin:
    _model: nn.Module

    @property
    def num_classes(self):
        return self._model.num_classes


class _Pending:
    """Device scalars whose host values are fetched with a single synchronising copy per iteration; the deferred
    assertion flags of miseg_amd.checks ride in the same copy and are raised right after it."""

    def __init__(self):
        self._names: List[str] = []
        self._vals: List[Tensor] = []
        self.checks: list = []
        self._static = None

    def put(self, name: str, value) -> None:
        """value: a device scalar or a symbolic miseg_amd.lazy.LinearLoss (evaluated with all others at fetch time)."""
        self._names.append(name)
        self._vals.append(value.detach() if isinstance(value, (Tensor, LinearLoss)) else value)

    def precompute(self) -> Optional[Tensor]:
        """Evaluate everything recorded so far NOW (values and check flags: ``device_values``) and keep the result for the
        iteration's ``post`` / ``fetch``; returns the check flags (a view of that vector, None without checks) -- the optimiser
        launch is guarded with them.  Nothing may be ``put`` between this call and the post."""
        if self._static is None:
            if not self._vals and not self.checks:
                return None
            scalars = self.device_values()
            self._static = (self._names, scalars, list(self.checks))
            self._names, self._vals, self.checks[:] = [], [], []
        names, scalars, items = self._static
        return scalars[len(names):] if items else None

    def take_static(self):
        """(names, device vector, check items) of ``precompute``, removed."""
        st, self._static = self._static, None
        return st

    def device_values(self) -> Tensor:
        """float32 device vector: the put() values followed by the deferred-check flags (one launch: lazy.report)."""
        return lazy.report(self._vals, self.checks)

    def fetch(self) -> dict:
        if self._static is not None:      # values of a replayed step graph: one static device tensor, fixed names and checks
            names, scalars, items = self._static
            self._static = None
            host = scalars.tolist()
            out = dict(zip(names, host))
            checks.raise_failed(items, host[len(names):])
            return out
        if not self._vals and not self.checks:
            return {}
        host = self.device_values().tolist()
        out = dict(zip(self._names, host))
        items, self.checks[:] = list(self.checks), []
        self._names, self._vals = [], []
        checks.raise_failed(items, host[len(out):])
        return out

    def post(self, extras=()):
        """Start the asynchronous copy of this iteration's scalars (and deferred-check flags) into pinned host memory and
        return a ticket for ``wait``; ``extras`` (device tensors, e.g. the Dice counts) travel the same way and come back as
        the ticket's host tensors.  The training loop waits for iteration i's ticket only after iteration i+1 is enqueued,
        so the host never drains the GPU queue: a per-iteration ``fetch()`` left the first ~0.25 ms of every step's launches
        exposed."""
        if self._static is not None:
            names, scalars, items = self._static
            self._static = None
        elif not self._vals and not self.checks:
            names, scalars, items = [], None, []
        else:
            scalars = self.device_values()
            names, items = self._names, list(self.checks)
            self._names, self._vals, self.checks[:] = [], [], []
        payload = ([] if scalars is None else [scalars]) + list(extras)
        if not any(t.is_cuda for t in payload):
            return names, items, scalars, tuple(extras), None
        self._turn = getattr(self, "_turn", 0) ^ 1
        ring = self.__dict__.setdefault("_ring", {})
        host = []
        for i, t in enumerate(payload):
            buf = ring.get((self._turn, i))
            if buf is None or buf.shape != t.shape or buf.dtype != t.dtype:
                buf = ring[(self._turn, i)] = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
            buf.copy_(t.detach(), non_blocking=True)
            host.append(buf)
        done = torch.cuda.Event()
        done.record()
        if scalars is None:
            return names, items, None, tuple(host), done
        return names, items, host[0], tuple(host[1:]), done

    @staticmethod
    def wait(ticket):
        """(host values, host extras) of a ``post()`` ticket; raises the deferred assertions that rode along (same errors as
        ``fetch``).  The host tensors are ring buffers: consume them before the ticket after next is posted."""
        if isinstance(ticket, stepio.Ticket):     # the iteration's one read-back block (values | flags | [overflow count], Dice counts)
            fields = ticket.io.wait(ticket)
            vals = fields["scalars"].tolist()
            out = dict(zip(ticket.names, vals))
            for name, field in fields.items():        # what an epocher put into the block beside the standard fields (cps: "agree")
                if name not in ("scalars", "inter", "union", "nonfinite"):
                    out[name] = field.tolist()
            checks.raise_failed(ticket.items, vals[len(ticket.names):len(ticket.names) + len(ticket.items)])
            extras = [fields["inter"], fields["union"]]
            if "nonfinite" in fields:
                extras.append(fields["nonfinite"])
            elif ticket.nvals > len(ticket.names) + len(ticket.items):      # overflow count in the slot behind the flags
                extras.append(fields["scalars"][ticket.nvals - 1:ticket.nvals])
            return out, tuple(extras)
        names, items, host, extras, done = ticket
        if done is not None:
            done.synchronize()
        vals = host.tolist() if host is not None else []
        out = dict(zip(names, vals))
        checks.raise_failed(items, vals[len(names):])
        return out, extras


def supervised_loss(criterion: T_loss, logits: Tensor, labels: Tensor, num_classes: int, disable_assert: bool = False) -> Tensor:
    """``criterion(softmax(logits), one_hot(labels))`` (ref :165-166): one fused kernel where the criterion has it, else the
    reference's call on materialised operands.  ``disable_assert`` is the evaluation's (no autograd there for ``KL_div`` to insist on)."""
    if isinstance(criterion, KL_div) and criterion.supports_fused():
        return criterion.from_logits(logits, labels)
    if isinstance(criterion, (GeneralizedDiceLoss, KLDiceLoss)) and logits.is_cuda and criterion.supports_fused(logits.shape[1]) and \
            ops.softmax_dice_supported(logits.shape[1]):
        return criterion.from_logits(logits, labels)
    flags = {"disable_assert": True} if disable_assert else {}
    return criterion(logits.softmax(1), class2one_hot(labels, num_classes), **flags)


def consistency_loss(criterion: T_loss, student_tf_logits: Tensor, other_logits: Tensor, flips: Tensor):
    """``criterion(softmax(student(flip(u))), softmax(flip(other(u))).detach())`` (ref :221-224): flip, both softmaxes and the
    distance are one fused kernel for ``nn.MSELoss`` and the fused ``KL_div`` (``name: mse | kl``)."""
    if isinstance(criterion, nn.MSELoss):
        return LinearLoss.of(ops.softmax_mse(student_tf_logits, other_logits, flips))
    if isinstance(criterion, KL_div) and criterion.supports_fused():
        return LinearLoss.of(ops.softmax_kl_consistency(student_tf_logits, other_logits, flips))
    # any other criterion object: called as the reference calls it, on materialised operands
    return criterion(student_tf_logits.softmax(1), ops.flip(other_logits, flips).softmax(1).detach())


class EvalEpocher(_num_class_mixin, _Epocher):
    """Per-patient evaluation: KL loss + 3D Dice (ref :36-73).  A label outside [0, C) raises AssertionError at once, batch by batch
    (``ops.softmax_kl`` outside a ``checks.deferred`` block reads its flag where the loss is read anyway), as the reference's
    ``class2one_hot`` does; the inference epocher inherits this."""

    def __init__(self, model, val_loader: T_loader, sup_criterion: T_loss, cur_epoch=0, device="cpu") -> None:
        super().__init__(model, num_batches=len(val_loader), cur_epoch=cur_epoch, device=device)
        self._val_loader = val_loader
        self._sup_criterion = sup_criterion

    def _configure_meters(self, meters: MeterInterface) -> MeterInterface:
        meters.register_meter("loss", AverageValueMeter())
        meters.register_meter("dice", UniversalDice(self.num_classes, report_axises=list(range(1, self.num_classes))))
        return meters

    _WANT_PRED = False        # whether ``_after_batch`` needs the class map (it gets None without)

    @torch.no_grad()
    def _run(self, *args, **kwargs) -> Tuple[EpochResultDict, float]:
        self._model.eval()
        report_dict = EpochResultDict()
        for _, val_data in zip(self._indicator, self._val_loader):
            val_img, val_target, file_path, _, group = self._unzip_data(val_data, self._device)
            val_logits = self._model(val_img)
            labels = val_target.squeeze(1)
            val_loss = supervised_loss(self._sup_criterion, val_logits, labels, self.num_classes, disable_assert=True)
            pred, inter, union = ops.argmax_dice(val_logits, labels, want_pred=self._WANT_PRED)
            self.meters["loss"].add(val_loss.item())
            self.meters["dice"].add_counts(inter, union, group_name=group)
            self._after_batch(val_img, val_target, val_logits, pred, file_path, group)
            report_dict = self.meters.tracking_status()
            self._indicator.set_postfix_dict(report_dict)
        return report_dict, self.meters["dice"].summary()["DSC_mean"]

    def _after_batch(self, val_img, val_target, val_logits, pred, file_path, group) -> None:   # what an evaluation adds per batch
        pass

    @staticmethod
    def _unzip_data(data, device):
        return preprocess_input_with_single_transformation(data, device)


class InferenceEpocher(EvalEpocher):
    """Evaluation that also dumps image / ground truth / prediction PNGs and reports per-class surface distances
    (ref :76-107): ``surface_metrics`` lists ``SurfaceMeter`` names, registered as ``hd`` (hausdorff, the reference's one),
    ``mhd`` (mod_hausdorff) and ``asd`` (average_surface).  The argmax + Dice counts stay fused on the device and so do the surface
    statistics (one ``miseg_surface_stats`` launch per batch, shared by the meters); the PNG writes are host work, as in the reference.

    ``keep_largest`` (default off: every report, key and file is then what it is without it) adds the same measurements on the
    prediction with only the largest connected component of each foreground class kept, per slice (a loader batch need not be a
    whole patient, so not per volume): one ``ops.largest_component`` call per batch, which also returns the cleaned prediction's Dice
    counts.  The meters ``dice_lcc`` and ``hd_lcc`` / ``mhd_lcc`` / ``asd_lcc`` stand next to the raw prediction's, which stay, and
    the cleaned maps go to ``pred_lcc/``.  ``component_connectivity``: 1 = 4-neighbours, 2 = 8-neighbours."""

    SURFACE_METERS = {"hausdorff": "hd", "mod_hausdorff": "mhd", "average_surface": "asd"}

    def __init__(self, model, val_loader: T_loader, sup_criterion: T_loss, cur_epoch=0, device="cpu", surface_metrics=("hausdorff",),
                 keep_largest=False, component_connectivity=1) -> None:
        self._surface_metrics = tuple(surface_metrics)
        assert all(m in self.SURFACE_METERS for m in self._surface_metrics), surface_metrics
        assert component_connectivity in (1, 2), component_connectivity
        self._keep_largest, self._component_connectivity = bool(keep_largest), int(component_connectivity)
        super().__init__(model, val_loader, sup_criterion, cur_epoch=cur_epoch, device=device)

    def set_save_dir(self, save_dir):
        self._save_dir = save_dir

    def _configure_meters(self, meters: MeterInterface) -> MeterInterface:
        meters = super()._configure_meters(meters)
        for metername in self._surface_metrics:
            meters.register_meter(self.SURFACE_METERS[metername],
                                  SurfaceMeter(C=self.num_classes, report_axises=list(range(1, self.num_classes)), metername=metername))
        if self._keep_largest:
            meters.register_meter("dice_lcc", UniversalDice(self.num_classes, report_axises=list(range(1, self.num_classes))))
            for metername in self._surface_metrics:
                meters.register_meter(self.SURFACE_METERS[metername] + "_lcc",
                                      SurfaceMeter(C=self.num_classes, report_axises=list(range(1, self.num_classes)), metername=metername))
        return meters

    def _add_surface(self, pred, labels, suffix=""):
        shared = None                              # the batch's surface statistics: one launch for all the surface meters
        if len(self._surface_metrics) > 1 and SurfaceMeter.on_device(pred, labels):
            shared = SurfaceMeter.batch_stats(pred, labels, list(range(1, self.num_classes)))
        for metername in self._surface_metrics:
            try:                                   # ref: ExceptionIgnorer(RuntimeError) -- a class absent from a slice
                self.meters[self.SURFACE_METERS[metername] + suffix].add(pred, labels, stats=shared)
            except RuntimeError:
                pass

    _WANT_PRED = True

    def _after_batch(self, val_img, val_target, val_logits, pred, file_path, group) -> None:
        write_img_target(val_img, val_target, self._save_dir, file_path)
        write_predict(val_logits, self._save_dir, file_path)
        labels = val_target.squeeze(1)
        self._add_surface(pred, labels)
        if self._keep_largest:
            cleaned, _, (inter_lcc, union_lcc) = ops.largest_component(
                pred, list(range(1, self.num_classes)), volume=False, connectivity=self._component_connectivity, fill=0,
                target=labels.contiguous().long(), num_classes=self.num_classes)
            self.meters["dice_lcc"].add_counts(inter_lcc, union_lcc, group_name=group)
            self._add_surface(cleaned, labels, "_lcc")
            write_prediction_map(cleaned, self._save_dir, file_path, "pred_lcc")


class TrainEpocher(_num_class_mixin, _Epocher):
    """Supervised-only (``partial``) step (ref :110-197); the semi-supervised epochers add ``regularization``."""

    def __init__(self, model, optimizer: T_optim, labeled_loader: T_loader, unlabeled_loader: T_loader, sup_criterion: T_loss,
                 reg_weight: float, num_batches: int, cur_epoch=0, device="cpu", feature_position=None,
                 feature_importance=None) -> None:
        super().__init__(model, num_batches=num_batches, cur_epoch=cur_epoch, device=device)
        self._optimizer = optimizer
        self._labeled_loader, self._unlabeled_loader = labeled_loader, unlabeled_loader
        self._sup_criterion = sup_criterion
        self._reg_weight = reg_weight
        self._affine_transformer = TensorRandomFlip(axis=[1, 2], threshold=0.8)
        assert isinstance(feature_position, list) and isinstance(feature_position[0], str), feature_position
        assert isinstance(feature_importance, list) and isinstance(feature_importance[0], (int, float)), feature_importance
        self._feature_position, self._feature_importance = feature_position, feature_importance
        self._reducer = None  # set by miseg_amd.ddp.attach() for data-parallel runs

    # The meters a class ADDS, in the order of the report's columns.  ``_configure_meters`` registers those of the whole class chain,
    # base first; ``_record`` feeds each one whose name is a key of the iteration's host dict.  What is not a host value (the Dice
    # counts, ``lr``, the weights, the per-tap ``individual_mis``) is fed where it is known.
    METERS: Tuple[str, ...] = ("lr", "sup_loss", "reg_loss", "sup_dice")

    def _configure_meters(self, meters: MeterInterface) -> MeterInterface:
        for klass in reversed(type(self).__mro__):
            for name in vars(klass).get("METERS", ()):
                if name == "sup_dice":
                    meter = UniversalDice(self.num_classes, report_axises=list(range(1, self.num_classes)))
                else:
                    meter = MultipleAverageValueMeter() if name == "individual_mis" else AverageValueMeter()
                meters.register_meter(name, meter)
        return meters

    # ---- one optimisation step
    def _step(self, labeled_data, unlabeled_data):
        # host prelude: unpack the batches, draw the flip decisions (same draws, same order as the per-sample flips at ref :148-149)
        seed = random.randint(0, int(1e7))
        labeled_image, labeled_target, _, _, label_group = self._unzip_data(labeled_data, self._device)
        unlabeled_image, _unlabeled_target, *_ = self._unzip_data(unlabeled_data, self._device)
        self._batch_shapes = (tuple(labeled_image.shape), tuple(unlabeled_image.shape))
        flip_masks = self._draw_words(seed, len(unlabeled_image))
        self._seed = seed
        io = self._io_for(labeled_image.device)
        tape = self._step_tape
        if tape is not None and (self._reducer is None or self._reducer.flat.flat_grad.is_cuda):
            ticket = tape.step(io, labeled_image, labeled_target, unlabeled_image, flip_masks)
        else:
            ticket = self._run_step(io, labeled_image, labeled_target, unlabeled_image, flip_masks)
        return ticket, None, label_group

    def _draw_words(self, seed: int, ub: int) -> List[int]:
        """The iteration's host draws under ``FixRandomSeed(seed)``, as the int32 words the step block stages in its flips slot:
        [flips of the UB unlabeled samples | UB zeros] (the tf branch is never re-flipped)."""
        with FixRandomSeed(seed):
            decisions = self._affine_transformer.decisions(ub)
        return ops.flip_masks(list(decisions) + [[False, False]] * ub)

    _io = None
    _step_tape = None
    _TRAIN_FORWARDS = 1       # U-Net training forwards per iteration: the step block's BatchNorm accumulator room (stepio.block_bytes)
    _TAPE_DEFAULT = os.environ.get("MISEG_TAPE", "1") != "0"

    def _io_for(self, device) -> "stepio.StepIO":
        """The iteration's two host <-> device blocks (miseg_amd.stepio); with them, unless MISEG_TAPE=0, the launch tape that replays
        the iteration from one C call once it has run eagerly a few times (miseg_amd.tape.StepTape).  Both hang off the OPTIMISER,
        which outlives the per-epoch epocher objects (ref semi_seg/trainer.py:197-206 builds a new epocher every epoch): the tape
        recorded in the first epoch serves the later ones.  GPU only, like the kernels."""
        if torch.device(device).type != "cuda":
            from miseg_amd._cabi import MisegError
            raise MisegError("the train step runs on the GPU only (got CPU batches); there is no CPU fallback")
        io = self._io
        if io is None or io.device != torch.device(device):
            ctx = getattr(self._optimizer, "_miseg_step_ctx", None)
            size = stepio.block_bytes(self._TRAIN_FORWARDS)
            if ctx is None or ctx["io"].device != torch.device(device) or ctx["io"].param_bytes != size:
                if ctx is not None and ctx["tape"] is not None:
                    ctx["tape"].release()
                ctx = {"io": stepio.StepIO(device, param_bytes=size), "tape": None}
                try:
                    self._optimizer._miseg_step_ctx = ctx
                except AttributeError:
                    pass
            io = self._io = ctx["io"]
            self._step_ctx = ctx
            if ctx["tape"] is not None:
                ctx["tape"].ep = self
                self._step_tape = ctx["tape"]
            elif self._TAPE_DEFAULT and self._step_tape is None:
                self.enable_step_tape()
        return io

    def enable_step_tape(self, warmup: int = 3) -> None:
        """Replay the iteration from the library's launch tape after ``warmup`` eager iterations (one more runs eagerly while it is
        recorded).  In data-parallel runs the bucket all-reduces and the wait for them stay host calls between segments of the tape
        (miseg_amd.tape.host_call)."""
        from miseg_amd.tape import StepTape
        self.disable_step_tape()
        self._step_tape = StepTape(self, warmup=warmup)
        ctx = getattr(self, "_step_ctx", None)
        if ctx is not None:
            ctx["tape"] = self._step_tape

    def disable_step_tape(self) -> None:
        if self._step_tape is not None:
            self._step_tape.release()
        self._step_tape = None
        ctx = getattr(self, "_step_ctx", None)
        if ctx is not None:
            ctx["tape"] = None

    def _tape_signature(self):
        """What, besides shapes, decides the recorded launch list: the trainer kind and its loss coefficients (they are the constant
        gradients that seed backward)."""
        # ... and where the persistent state lives: a rebuilt flat buffer (FlatBuffers.build after the parameters moved) or moved
        # BatchNorm buffers would leave the recorded pointers dangling -- a changed address re-records instead
        opt = self._optimizer
        where = tuple((fb.flat_param.data_ptr(), fb.flat_grad.data_ptr()) for fb in getattr(opt, "_flats", []) if fb.flat_param is not None)
        where += tuple(t.data_ptr() for name in ("_m", "_vmax") for t in getattr(opt, name, []) if t is not None)
        buf = next(iter(self._model.buffers()), None)
        return (type(self).__name__, float(self._reg_weight), getattr(self, "_cons_weight", None), getattr(self, "_iic_weight", None),
                tuple(self._feature_importance), tuple(self._feature_position), self._criterion_signature(self._sup_criterion),
                type(getattr(self, "_reg_criterion", None)).__name__, where, None if buf is None else buf.data_ptr(), id(self._model))

    @staticmethod
    def _criterion_signature(criterion):
        """A criterion's type name and, where it has a ``signature()``, the constants its fused call bakes into the recorded launch
        (``GeneralizedDiceLoss`` / ``KLDiceLoss``: eps, pow, class weights, the two coefficients); ``KL_div`` has none."""
        name = type(criterion).__name__
        return (name, criterion.signature()) if hasattr(criterion, "signature") else name

    def _loss_scale(self) -> float:
        """Current loss scale: 1 unless the activations are IEEE half (BASELINE configs[4]); dynamic from its initial value."""
        scale = unet_ops.loss_scale_of(self._model)
        if scale == 1.0:
            return 1.0
        if not hasattr(self._optimizer, "grad_scale"):
            raise RuntimeError("Arch.compute_dtype=float16 needs a fused optimiser (Optim.name=Adam, RAdam, AdaBound or AdaBoundW), "
                               "which undoes the loss scale")
        if self._optimizer.loss_scaler is None:
            from miseg_amd.flat import LossScaler
            self._optimizer.loss_scaler = LossScaler(scale)
        return self._optimizer.loss_scaler.scale

    def _stage(self, io, flip_masks) -> int:
        """Host half of an iteration: the optimiser's step counter / scalars, the loss scale and the flip masks into the next pinned
        slot of the step block.  No device work (a replayed launch tape calls just this)."""
        rows = self._optimizer.host_step() if hasattr(self._optimizer, "host_step") else []
        scale = self._loss_scale()
        if hasattr(self._optimizer, "grad_scale"):
            self._optimizer.grad_scale = scale
        return io.stage(flip_masks, rows, scale)

    def _run_step(self, io, labeled_image: Tensor, labeled_target: Tensor, unlabeled_image: Tensor, flip_masks):
        """One eager iteration on the GPU: upload, forward, losses, backward, optimiser, read-back.  Returns the read-back ticket."""
        io.upload(self._stage(io, flip_masks))
        stepio.CURRENT = io
        try:
            self._device_step(labeled_image, labeled_target, unlabeled_image, io.flips())
            return self._post(io)
        finally:
            stepio.CURRENT = None

    def _after_replay(self) -> None:
        packcache.PACK_CACHE.invalidate()       # the replay ran Adam: eager users of the weights (evaluation) must re-pack

    def _post(self, io):
        """The iteration's report (if the guarded optimiser launch has not computed it already) and the one device -> host copy."""
        self._pending.precompute()
        st = self._pending.take_static()
        names, scalars, items = st if st is not None else ([], None, [])
        rep = getattr(io, "last_report", None)
        if scalars is not None and (rep is None or scalars.data_ptr() != rep.data_ptr()):
            # evaluated outside the read-back block (a value that does not live in the scalar arena): copy it in
            rep = io.out("scalars", (scalars.numel() + 1,), torch.float32)
            rep[:scalars.numel()].copy_(scalars)
        nvals = 0 if rep is None else rep.numel() - (0 if getattr(self._optimizer, "last_nonfinite", None) is not None and
                                                     self._optimizer.last_nonfinite.data_ptr() == rep[-1:].data_ptr() else 1)
        return io.post(names, items, nvals)

    def _before_forward(self, ub: int) -> None:   # hooks for epochers that start work while the network is still running
        pass

    def _after_forward(self) -> None:
        pass

    def _forward(self, batch: Tensor, ub: int) -> Tensor:
        """One training forward of the network, between the forward hooks; its simplex / NaN assertions are deferred to this
        iteration's fetch()."""
        with checks.deferred(self._pending.checks):
            self._before_forward(ub)
            try:
                return self._model(batch)
            finally:
                self._after_forward()

    def _assemble(self, labeled_image: Tensor, unlabeled_image: Tensor, flips: Tensor, keep_unflipped: bool) -> Tensor:
        """The network's batch, ``[labeled | unlabeled | flip(unlabeled)]`` or, without ``keep_unflipped``, ``[labeled |
        flip(unlabeled)]`` (ref :148-153: per-sample flips, stack, cat): one launch where the kernels take the operands."""
        if labeled_image.dtype == unlabeled_image.dtype == torch.float32 and labeled_image.dim() == 4 and \
                labeled_image.shape[1:] == unlabeled_image.shape[1:] and labeled_image.is_cuda:
            if not keep_unflipped:
                return ops.cat_flipped(labeled_image, unlabeled_image, flips)
            net = getattr(self._model, "module", self._model)
            return ops.cat_flip(labeled_image, unlabeled_image, flips,
                                stem_dtype=getattr(net, "compute_dtype", None) if getattr(net, "input_dim", None) == 1 else None)
        flipped = ops.flip(unlabeled_image, flips)
        return torch.cat([labeled_image, unlabeled_image, flipped] if keep_unflipped else [labeled_image, flipped], dim=0)

    def _device_step(self, labeled_image: Tensor, labeled_target: Tensor, unlabeled_image: Tensor, flips2: Tensor, seed: int = None):
        """Everything of the iteration that runs on the GPU between the upload and the read-back: forward, losses, backward,
        optimiser kernel, Dice counts.  No host synchronisation, no host->device traffic, and -- for the shipped trainers -- no launch
        outside the library (so the iteration can be replayed from the launch tape); the host half (``_stage``) has run."""
        seed = self._seed if seed is None else seed
        lb, ub = len(labeled_image), len(unlabeled_image)
        self._flips2 = flips2
        flips = flips2[:ub]
        batch = self._assemble(labeled_image, unlabeled_image, flips, keep_unflipped=True)
        unlabeled_image_tf = batch[lb + ub:]
        assert unlabeled_image_tf.shape == unlabeled_image.shape

        predict_logits = self._forward(batch, ub)
        label_logits, unlabel_logits, unlabel_tf_logits = ops.split_rows(predict_logits, [lb, ub, ub])
        labels = labeled_target.squeeze(1)
        with checks.deferred(self._pending.checks):
            sup_loss = supervised_loss(self._sup_criterion, label_logits, labels, self.num_classes)
            reg_fn = self.regularization
            fused = getattr(reg_fn, "_miseg_fused", False)
            reg_loss = reg_fn(
                unlabeled_tf_logits=unlabel_tf_logits,
                unlabeled_logits_tf=None if fused else ops.flip(unlabel_logits, flips),
                seed=seed, unlabeled_image=unlabeled_image, unlabeled_image_tf=unlabeled_image_tf,
                unlabeled_logits=unlabel_logits, flips=flips, num_unlabeled=ub,
            )
        return self._finish_step(sup_loss, reg_loss, label_logits, labels)

    def _finish_step(self, sup_loss, reg_loss, label_logits: Tensor, labels: Tensor, more_loss=None):
        """The iteration's tail: the total loss, the forward read-back, backward, the guarded optimiser launch.  Returns the Dice
        counts.  ``more_loss``: a term of the total that is neither reported as ``sup_loss`` nor weighted (a second network's
        supervised loss)."""
        total_loss = sup_loss + self._reg_weight * reg_loss
        if more_loss is not None:
            total_loss = total_loss + more_loss
        # Everything the read-back needs from the FORWARD pass is launched here, before backward: the Dice counts and the iteration's
        # report (meter values + the simplex / NaN flags that guard the update).  Issued after backward they sat behind the optimiser's
        # wait for the weight-gradient stream, i.e. on the step's tail (~19 us); here they run while the main stream waits for the IIC chain.
        def forward_readback():
            with torch.no_grad():
                self._pending.put("sup_loss", sup_loss)
                self._pending.put("reg_loss", reg_loss)
                dice = ops.argmax_dice(label_logits.detach(), labels, want_pred=False, to_host=True)
            return dice[1], dice[2], (self._pending.precompute() if _GUARD_STEP and hasattr(self._optimizer, "apply") else None)
        if _READBACK_EARLY:
            inter, union, guard = forward_readback()
        self._optimizer.zero_grad()
        if self._reducer is not None:
            self._reducer.prepare()
        # fp16 storage mode: backward is seeded with the loss scale; the fused Adam reads the gradients as grad / scale, counts their
        # non-finite entries and skips the update if there are any; the scale follows (flat.LossScaler, one iteration late)
        scale = self._loss_scale()
        if isinstance(total_loss, LinearLoss):
            total_loss.backward(scale)
        elif scale != 1.0:
            (total_loss * scale).backward()
        else:
            total_loss.backward()
        if self._reducer is not None:
            self._reducer.finish()
        io = stepio.CURRENT
        if not _READBACK_EARLY:
            inter, union, guard = forward_readback()
        if hasattr(self._optimizer, "apply"):
            # The report's flags guard the update on the device: the host raises a failed check one iteration late, but it has not moved
            # the weights (the reference raises before backward).
            self._optimizer.apply(guard=guard, io=io)
        else:
            self._optimizer.step()
        self._overflow = getattr(self._optimizer, "last_nonfinite", None)     # device float[1] in the fp16 mode, else None
        return inter, union

    def _run(self, *args, **kwargs) -> EpochResultDict:
        self.meters["lr"].add(get_lrs_from_optimizer(self._optimizer)[0])
        self._model.train()
        assert self._model.training, self._model.training
        report_dict = {}
        self._pending = _Pending()
        with FeatureExtractor(self._model, self._feature_position) as self._fextractor:
            for _, labeled_data, unlabeled_data in zip(self._indicator, self._labeled_loader, self._unlabeled_loader):
                self._after_step(*self._step(labeled_data, unlabeled_data))
                report_dict = self.meters.tracking_status()
                self._indicator.set_postfix_dict(report_dict)
            self._flush_records()
            report_dict = self.meters.tracking_status()
        return report_dict

    # The iteration's single host read-back (ref: the .item() calls of semi_seg/epocher.py:115-121) is taken one iteration
    # late: iteration i's scalars travel to pinned memory asynchronously and are recorded after iteration i+1 is enqueued, so
    # the GPU always has the next step queued.  Every iteration is still recorded (the last one by _flush_records), a NaN loss
    # or a failed deferred assertion raises one iteration later.  MISEG_DEFER_FETCH=0 restores the synchronous read-back.
    _DEFER_FETCH = os.environ.get("MISEG_DEFER_FETCH", "1") != "0"
    _inflight = None

    _overflow = None

    def _after_step(self, inter, union: Optional[Tensor], label_group) -> None:
        if isinstance(inter, stepio.Ticket):      # the GPU path: the read-back is already under way (_post)
            ticket = inter
        else:
            extras = (inter, union) if self._overflow is None else (inter, union, self._overflow)
            ticket = self._pending.post(extras)
        prev, self._inflight = self._inflight, (ticket, label_group)
        if not self._DEFER_FETCH:
            self._flush_records()
        elif prev is not None:
            self._record_ticket(*prev)

    def _flush_records(self) -> None:
        last, self._inflight = self._inflight, None
        if last is not None:
            self._record_ticket(*last)

    def _record_ticket(self, ticket, label_group) -> None:
        host, extras = self._pending.wait(ticket)
        inter, union = extras[0], extras[1]
        if len(extras) > 2:         # fp16 mode: the gradient's non-finite count -> the loss scale of the iterations still to be enqueued
            scaler = self._optimizer.loss_scaler
            before, bad = scaler.scale, float(extras[2][0])
            scaler.update(bad, getattr(ticket, "scale", None))
            if (bad != 0.0 or bad != bad) and hasattr(self._optimizer, "step_skipped"):
                self._optimizer.step_skipped()          # the device skipped that update: it does not count towards the bias corrections
            if scaler.scale < before:
                import warnings
                warnings.warn(f"fp16 gradient overflow: that optimiser step was skipped, loss scale {before:g} -> {scaler.scale:g}")
        self._record(host, inter.clone(), union.clone(), label_group)   # the meters keep them; the pinned ring is reused

    def _record(self, host: dict, inter: Tensor, union: Tensor, label_group) -> None:
        for name in self.meters.meter_names:
            if name in host:
                self.meters[name].add(host[name])
        self.meters["sup_dice"].add_counts(inter, union, group_name=label_group)

    @staticmethod
    def _unzip_data(data, device):
        (image, target), _, filename, partition, group = preprocess_input_with_twice_transformation(data, device)
        return image, target, filename, partition, group

    @_fused
    def regularization(self, *args, **kwargs):
        return LinearLoss([])      # symbolic zero (ref :194-197 returns a zero tensor): no kernel, reported as 0


class _uda_mixin:
    """The reported consistency term of ``uda``, ``midl`` and ``udaiic`` (``_reg_criterion`` is the epocher's)."""

    METERS = ("uda",)

    def _uda(self, unlabeled_tf_logits: Tensor, unlabeled_logits: Tensor, flips: Tensor):
        loss = consistency_loss(self._reg_criterion, unlabeled_tf_logits, unlabeled_logits, flips)
        self._pending.put("uda", loss)
        return loss


class UDATrainEpocher(_uda_mixin, TrainEpocher):
    """Consistency between f(flip(x)) and flip(f(x)).detach() (ref :200-226)."""

    def __init__(self, model, optimizer, labeled_loader, unlabeled_loader, sup_criterion, reg_criterion: T_loss, reg_weight: float,
                 num_batches: int, cur_epoch: int = 0, device="cpu", feature_position=None, feature_importance=None) -> None:
        super().__init__(model, optimizer, labeled_loader, unlabeled_loader, sup_criterion, reg_weight, num_batches, cur_epoch,
                         device, feature_position, feature_importance)
        self._reg_criterion = reg_criterion

    @_fused
    def regularization(self, unlabeled_tf_logits: Tensor, unlabeled_logits_tf: Tensor = None, seed=None, *args,
                       unlabeled_logits: Tensor = None, flips: Tensor = None, **kwargs):
        return self._uda(unlabeled_tf_logits, unlabeled_logits, flips)


class IICTrainEpocher(TrainEpocher):
    """Global (encoder taps) + local (decoder taps) IIC mutual information (ref :229-284)."""

    METERS = ("mi", "individual_mis")

    def __init__(self, model, projectors_wrapper: ProjectorWrapper, optimizer, labeled_loader, unlabeled_loader, sup_criterion,
                 IIDSegCriterionWrapper: IICLossWrapper, reg_weight: float, num_batches: int, cur_epoch: int = 0, device="cpu",
                 feature_position=None, feature_importance=None) -> None:
        super().__init__(model, optimizer, labeled_loader, unlabeled_loader, sup_criterion, reg_weight, num_batches, cur_epoch,
                         device, feature_position, feature_importance)
        assert projectors_wrapper.feature_names == self._feature_position
        self._projectors_wrapper = projectors_wrapper
        assert IIDSegCriterionWrapper.feature_names == self._feature_position
        self._IIDSegCriterionWrapper = IIDSegCriterionWrapper

    # ---- The IIC branch runs on its own HIP stream.  (1) Each tapped feature is turned into its MI loss the moment the
    # forward hook delivers it (FeatureExtractor.on_feature), so heads + joint of the Up_conv3 tap overlap the rest of the
    # decoder on the main stream; (2) autograd replays backward nodes on the stream of their forward op, so the
    # matrix-core-bound local-MI backward of the earlier taps overlaps the HBM-bound BatchNorm / weight-gradient kernels of
    # the later decoder blocks.  Backward runs the most recently created chain first, i.e. the last tap -- the one the main
    # stream has to wait for -- goes first.
    def _use_side_stream(self, dev) -> bool:
        if dev.type != "cuda" or os.environ.get("MISEG_IIC_STREAM", "1") != "1":
            return False
        # under hipGraph capture the fork/join (wait_stream both ways) is captured as graph dependencies
        return unet_ops.side_streams_allowed()

    def _side(self, dev):
        side = getattr(self, "_iic_stream", None)
        if side is None:
            side = self._iic_stream = torch.cuda.Stream(device=dev)
        red = getattr(self, "_reducer", None)
        if red is not None and side not in red.producer_streams:
            red.producer_streams.append(side)
            red.producer_streams.append(torch.cuda.current_stream(dev))
        return side

    def _before_forward(self, ub: int) -> None:
        self._early, self._ub_now = {}, ub
        fx = getattr(self, "_fextractor", None)
        if fx is not None and hasattr(fx, "on_feature") and self._use_side_stream(self._flips2.device):
            fx.on_feature = self._on_feature

    def _after_forward(self) -> None:
        fx = getattr(self, "_fextractor", None)
        if fx is not None and hasattr(fx, "on_feature"):
            fx.on_feature = None

    def _on_feature(self, name: str, feature: Tensor) -> None:
        idx = self._feature_position.index(name)
        projector, criterion = list(self._projectors_wrapper)[idx], list(self._IIDSegCriterionWrapper)[idx]
        main, side = torch.cuda.current_stream(feature.device), self._side(feature.device)
        ops.wait_stream(side, main)
        _keep(feature, side)
        with torch.cuda.stream(side):
            self._early[name] = self._tap_loss(feature, projector, criterion, self._flips2, self._ub_now)

    def _iic(self, flips: Tensor, ub: int):
        if not self._use_side_stream(flips.device):
            return self._iic_body(flips, ub)
        main, side = torch.cuda.current_stream(flips.device), self._side(flips.device)
        ops.wait_stream(side, main)
        with torch.cuda.stream(side):
            out = self._iic_body(flips, ub)
        ops.wait_stream(main, side)
        for t, _ in LinearLoss.of(out).terms:      # produced on `side`, read on `main`: keep the allocator informed
            _keep(t, main)
        return out

    def _tap_loss(self, feature: Tensor, projector, criterion, flips2: Tensor, ub: int):
        total = feature.shape[0]
        # last 2*UB samples of the tap: [features(unlabeled) | features(flip(unlabeled))]   (ref :258-259)
        src = ops.arange_i32(total - 2 * ub, total, feature.device)
        if isinstance(projector, ClusterHead):  # encoder tap: global pooling is flip-invariant (ref :261-262)
            probs = projector.forward_gathered(feature, src)                       # [S, 2UB, K]
            if _DEBUG_ASSERTS:
                from contrastyou.losses.iic_loss import simplex
                assert simplex(probs.flatten(0, 1))
            if probs.shape[1] != 2 * ub:
                raise RuntimeError(f"encoder tap: {probs.shape[1]} rows per sub-head, expected 2 x {ub}")
            per_head, _, _ = ops.global_mi_pair(probs, criterion.lamb)
            return LinearLoss.mean(per_head)
        # decoder tap: replay the flip on features(unlabeled) (ref :264-266), fused into the head
        probs = projector.forward_gathered(feature, src, flips2)  # [S, 2UB, K, H, W]
        if hasattr(criterion, "forward_heads"):   # all sub-heads as one autograd node (gradient lands in one buffer)
            return criterion.forward_heads(probs, ub, lazy=True)
        return average_iter([criterion(p[:ub], p[ub:]) for p in probs])

    def _iic_body(self, flips: Tensor, ub: int):
        flips2 = self._flips2 if getattr(self, "_flips2", None) is not None and len(self._flips2) == 2 * ub \
            else torch.cat([flips, torch.zeros_like(flips)])
        early = getattr(self, "_early", {})
        losses = []
        for name, feature, projector, criterion in zip(self._feature_position, self._fextractor, self._projectors_wrapper,
                                                       self._IIDSegCriterionWrapper):
            loss = early.pop(name, None)      # already launched from the forward hook (side stream)
            losses.append(loss if loss is not None else self._tap_loss(feature, projector, criterion, flips2, ub))
        reg_loss = weighted_average_iter(losses, self._feature_importance)
        self._pending.put("mi", -reg_loss)
        for name, v in zip(self._feature_position, losses):
            self._pending.put("mi/" + name, -v)
        return reg_loss

    @_fused
    def regularization(self, unlabeled_tf_logits: Tensor, unlabeled_logits_tf: Tensor = None, seed: int = None, *args,
                       flips: Tensor = None, num_unlabeled: int = None, **kwargs):
        return self._iic(flips, num_unlabeled if num_unlabeled is not None else len(unlabeled_tf_logits))

    def _record(self, host, inter, union, label_group):
        super()._record(host, inter, union, label_group)
        if "mi" in host:
            self.meters["individual_mis"].add(**{n: host["mi/" + n] for n in self._feature_position})


class UDAIICEpocher(_uda_mixin, IICTrainEpocher):
    """``cons_weight * UDA + iic_weight * IIC`` with reg_weight forced to 1 (ref :287-323)."""

    def __init__(self, model, projectors_wrapper: ProjectorWrapper, optimizer, labeled_loader, unlabeled_loader, sup_criterion,
                 reg_criterion: T_loss, IIDSegCriterion: T_loss, num_batches: int, cur_epoch: int = 0, device="cpu",
                 feature_position=None, feature_importance=None, cons_weight=1, iic_weight=0.1) -> None:
        super().__init__(model, projectors_wrapper, optimizer, labeled_loader, unlabeled_loader, sup_criterion, IIDSegCriterion,
                         1.0, num_batches, cur_epoch, device, feature_position, feature_importance)
        self._cons_weight, self._iic_weight = cons_weight, iic_weight
        self._reg_criterion = reg_criterion

    METERS = ("iic_weight", "uda_weight")

    @_fused
    def regularization(self, unlabeled_tf_logits: Tensor, unlabeled_logits_tf: Tensor = None, seed: int = None, *args,
                       unlabeled_logits: Tensor = None, flips: Tensor = None, num_unlabeled: int = None, **kwargs):
        iic_loss = self._iic(flips, num_unlabeled if num_unlabeled is not None else len(unlabeled_tf_logits))
        cons_loss = self._uda(unlabeled_tf_logits, unlabeled_logits, flips)
        return self._cons_weight * cons_loss + self._iic_weight * iic_loss

    def _record(self, host, inter, union, label_group):
        super()._record(host, inter, union, label_group)
        # host-side bookkeeping lives here, not in regularization(): that one is part of the captured device step
        self.meters["iic_weight"].add(self._iic_weight)
        self.meters["uda_weight"].add(self._cons_weight)


class MeanTeacherEpocher(TrainEpocher):
    """Mean Teacher (ref contrastyou/epocher/base_epocher.py:129-216, trainer contrast_trainer.py:235-262): a student trained on
    ``sup_loss + reg_weight * consistency(student(flip(u)), flip(teacher(u)))`` and a teacher that only runs forward and follows the
    student as an exponential moving average (``deepclustering2.models.ema_updater``).  One iteration:

    1. flip decisions of the unlabeled batch under ``FixRandomSeed(seed)`` (the ``semi_seg`` transformer, as the other epochers);
    2. the teacher's forward (train mode, no autograd) on the UNFLIPPED unlabeled batch: its own batch statistics, its own running
       statistics;
    3. the student's forward on ``[labeled | flip(unlabeled)]`` (one launch assembles it, ``ops.cat_flipped``);
    4. KL to the one-hot labels + ``reg_weight`` x the fused softmax-MSE (``name: kl``: the fused KL consistency) against the
       teacher's logits, flipped inside the loss kernel;
    5. backward, the guarded fused Adam on the student, then ONE ``miseg_ema_update`` launch over the teacher's flat buffer, guarded
       by the same flags: a skipped iteration moves neither network (the call count still advances, as the reference's does).

    The EMA's coefficients (alpha changes every step) ride in the step block, one row behind Adam's, so a replayed launch tape reads
    them; the block has accumulator room for both training forwards."""

    _TRAIN_FORWARDS = 2
    METERS = ("reg_weight",)

    def __init__(self, model, teacher_model, optimizer, labeled_loader: T_loader, unlabeled_loader: T_loader, sup_criterion: T_loss,
                 reg_criterion: T_loss, reg_weight: float, num_batches: int, cur_epoch=0, device="cpu", feature_position=None,
                 feature_importance=None, ema_updater=None) -> None:
        super().__init__(model, optimizer, labeled_loader, unlabeled_loader, sup_criterion, reg_weight, num_batches, cur_epoch,
                         device, feature_position, feature_importance)
        assert ema_updater is not None, "the Mean Teacher needs an ema_updater"
        self._teacher_model = teacher_model
        self._reg_criterion = reg_criterion
        self._ema_updater = ema_updater
        self._ema_row = None

    def _run(self, *args, **kwargs) -> EpochResultDict:
        self._teacher_model.train()
        self.meters["reg_weight"].add(self._reg_weight)
        return super()._run(*args, **kwargs)

    def _stage(self, io, flip_masks) -> int:
        """The fused optimiser's rows, then the EMA's (alpha, 1 - alpha, 1 - weight decay) of this call as one more row of the block."""
        if not hasattr(self._optimizer, "host_step"):
            raise RuntimeError("Trainer.name=meanteacher needs a fused optimiser (Optim.name: Adam, RAdam, AdaBound or AdaBoundW)")
        rows = self._optimizer.host_step()
        scale = self._loss_scale()
        self._optimizer.grad_scale = scale
        self._ema_row = len(rows)
        self._ema_updater.flats(self._teacher_model, self._optimizer.flat)     # the teacher's mirror of the student's flat buffer
        return io.stage(flip_masks, list(rows) + self._own_rows(), scale)

    def _own_rows(self) -> List[List[float]]:
        """The rows this epocher stages behind the optimiser's: the EMA's."""
        return [list(self._ema_updater.host_step()) + [0.0]]

    def _tape_signature(self):
        m = self._ema_updater._mirror
        buf = next(iter(self._teacher_model.buffers()), None)
        u = self._ema_updater
        return super()._tape_signature() + (id(self._teacher_model), None if m is None or m.flat_param is None else m.flat_param.data_ptr(),
                                            None if buf is None else buf.data_ptr(), u._alpha, u._justify_alpha, u._weight_decay, u._update_bn)

    def _device_step(self, labeled_image: Tensor, labeled_target: Tensor, unlabeled_image: Tensor, flips2: Tensor, seed: int = None):
        lb, ub = len(labeled_image), len(unlabeled_image)
        self._flips2 = flips2
        flips = flips2[:ub]
        batch = self._student_batch(labeled_image, unlabeled_image, flips)
        with checks.deferred(self._pending.checks):
            with torch.no_grad():          # the teacher: train mode, its own batch statistics, no autograd (ref :187-188)
                teacher_logits = self._teacher_forward(unlabeled_image)
            predict_logits = self._forward(batch, ub)
        label_logits, unlabel_tf_logits = ops.split_rows(predict_logits, [lb, ub])
        labels = labeled_target.squeeze(1)
        with checks.deferred(self._pending.checks):
            sup_loss = supervised_loss(self._sup_criterion, label_logits, labels, self.num_classes)
            reg_loss = self._consistency(unlabel_tf_logits, teacher_logits, flips)
        inter, union = self._finish_step(sup_loss, reg_loss, label_logits, labels)
        # the EMA after Adam (ref :205-206), guarded by the flags that guarded Adam
        self._ema_updater.apply(self._teacher_model, self._optimizer.flat, stepio.CURRENT.hyper(self._ema_row)[:3],
                                getattr(self._optimizer, "last_guard", None))
        return inter, union

    def _teacher_forward(self, unlabeled_image: Tensor) -> Tensor:
        """The teacher's logits the consistency term is held to: one tracked training forward on the unlabeled batch."""
        return self._teacher_model(unlabeled_image)

    def _student_batch(self, labeled_image: Tensor, unlabeled_image: Tensor, flips: Tensor) -> Tensor:
        """``[labeled | flip(unlabeled)]`` (ref :176-181)."""
        return self._assemble(labeled_image, unlabeled_image, flips, keep_unflipped=False)

    def _consistency(self, student_tf_logits: Tensor, teacher_logits: Tensor, flips: Tensor):
        """``reg_criterion(softmax(student(flip(u))), softmax(flip(teacher(u))).detach())`` (ref :193-194)."""
        return consistency_loss(self._reg_criterion, student_tf_logits, teacher_logits, flips)


def mix_consistency_loss(criterion: T_loss, student_logits: Tensor, teacher_logits: Tensor, perm: Tensor, coef: Tensor):
    """``criterion(softmax(student(m)), q)`` with ``q = coef[0] * softmax(teacher(u)) + coef[1] * softmax(teacher(u))[perm]`` detached:
    mixing, softmaxes and distance are one fused kernel for ``nn.MSELoss`` and the fused ``KL_div`` (``name: mse | kl``)."""
    if isinstance(criterion, nn.MSELoss):
        return LinearLoss.of(ops.softmax_mix_mse(student_logits, teacher_logits, perm, coef))
    if isinstance(criterion, KL_div) and criterion.supports_fused():
        return LinearLoss.of(ops.softmax_mix_kl_consistency(student_logits, teacher_logits, perm, coef))
    # any other criterion object: on materialised operands
    t = teacher_logits.detach().float().softmax(1)
    return criterion(student_logits.softmax(1), coef[0] * t + coef[1] * t[perm.long()])


class ICTEpocher(MeanTeacherEpocher):
    """``ict``: interpolation consistency training (Verma et al. 2019; ``ICTParameters``) -- the Mean Teacher
    iteration whose student sees a convex mix of two unlabeled images and is held to the same mix of the teacher's two predictions.
    What differs from ``MeanTeacherEpocher``, by the numbers of its iteration:

    1. the host draws, under ``FixRandomSeed(seed)`` and in this order, ``lam = float(numpy.random.beta(mix_alpha, mix_alpha))`` and
       ``perm = numpy.random.permutation(UB)``; no flips are drawn or applied.  ``perm`` travels in the step block's flips slot and
       ``(c0, c1) = (float32(lam), float32(1 - lam))`` in one more row behind the EMA's, so a replayed launch tape reads each
       iteration's values;
    3. the student's batch is ``[labeled | m]`` with ``m_i = c0 * u_i + c1 * u_perm[i]`` (one launch, ``ops.cat_mixed``);
    4. the consistency target at a pixel is ``c0 * softmax(t_i) + c1 * softmax(t_perm[i])`` of the teacher's logits ``t`` on the
       unmixed batch, mixed inside the loss kernel (``ops.softmax_mix_mse`` / ``ops.softmax_mix_kl_consistency``).

    The teacher's forward, backward, the guarded optimiser, the EMA and the meters are ``MeanTeacherEpocher``'s.  An index of the
    permutation outside the batch is one of the iteration's deferred checks (``IndexError`` at the fetch, the update skipped)."""

    def __init__(self, model, teacher_model, optimizer, labeled_loader: T_loader, unlabeled_loader: T_loader, sup_criterion: T_loss,
                 reg_criterion: T_loss, reg_weight: float, num_batches: int, cur_epoch=0, device="cpu", feature_position=None,
                 feature_importance=None, ema_updater=None, mix_alpha: float = 1.0) -> None:
        super().__init__(model, teacher_model, optimizer, labeled_loader, unlabeled_loader, sup_criterion, reg_criterion, reg_weight,
                         num_batches, cur_epoch, device, feature_position, feature_importance, ema_updater)
        if not float(mix_alpha) > 0.0:
            raise ValueError(f"ICTEpocher: mix_alpha must be positive, got {mix_alpha}")
        self._mix_alpha = float(mix_alpha)
        self._mix = (1.0, 0.0)

    @staticmethod
    def draw_mix(seed: int, ub: int, mix_alpha: float) -> Tuple[float, List[int]]:
        """``(lam, perm)`` of one iteration: under ``FixRandomSeed(seed)``, the Beta draw first, then the permutation."""
        with FixRandomSeed(seed):
            lam = float(np.random.beta(mix_alpha, mix_alpha))
            perm = np.random.permutation(ub)
        return lam, [int(p) for p in perm]

    def _draw_words(self, seed: int, ub: int) -> List[int]:
        lam, perm = self.draw_mix(seed, ub, self._mix_alpha)
        self._mix = (lam, 1.0 - lam)           # the subtraction in double; the block stores both as float32
        return perm

    def _own_rows(self) -> List[List[float]]:
        return super()._own_rows() + [[float(self._mix[0]), float(self._mix[1])]]

    def _coef(self) -> Tensor:
        return stepio.CURRENT.hyper(self._ema_row + 1)[:2]

    def _tape_signature(self):
        return super()._tape_signature() + (self._mix_alpha, self._criterion_signature(self._reg_criterion))

    def _student_batch(self, labeled_image: Tensor, unlabeled_image: Tensor, perm: Tensor) -> Tensor:
        """``[labeled | c0 * unlabeled + c1 * unlabeled[perm]]``: one launch where the kernel takes the operands."""
        coef = self._coef()
        if labeled_image.dtype == unlabeled_image.dtype == torch.float32 and labeled_image.dim() == 4 and \
                labeled_image.shape[1:] == unlabeled_image.shape[1:] and labeled_image.is_cuda:
            with checks.deferred(self._pending.checks):
                return ops.cat_mixed(labeled_image, unlabeled_image, perm, coef)
        wide = unlabeled_image.to(torch.promote_types(unlabeled_image.dtype, torch.float32))      # (16-bit images are mixed in fp32)
        mixed = coef[0] * wide + coef[1] * wide[perm.long()]
        return torch.cat([labeled_image, mixed.to(unlabeled_image.dtype)], dim=0)

    def _consistency(self, student_logits: Tensor, teacher_logits: Tensor, perm: Tensor):
        return mix_consistency_loss(self._reg_criterion, student_logits, teacher_logits, perm, self._coef())


def uamt_threshold(k: int, k_total: int, start: float, end: float, num_classes: int) -> float:
    """UA-MT's uncertainty threshold at iteration ``k`` of ``k_total``, in double: the fraction ``start + (end - start) *
    exp(-5 (1 - min(k / k_total, 1))^2)`` of the largest entropy ``ln(num_classes)``."""
    r = min(float(k) / float(max(int(k_total), 1)), 1.0)
    return (float(start) + (float(end) - float(start)) * math.exp(-5.0 * (1.0 - r) ** 2)) * math.log(float(num_classes))


class UAMTEpocher(MeanTeacherEpocher):
    """``uamt``: the uncertainty-aware Mean Teacher (Yu et al., MICCAI 2019; ``UAMTParameters``) -- the Mean
    Teacher iteration whose consistency term counts only where the teacher is certain.  What differs from ``MeanTeacherEpocher``, by
    the numbers of its iteration:

    1. no flips are drawn or applied; the host computes the threshold ``thr = uamt_threshold(k, k_total, ...)`` of iteration
       ``k = cur_epoch * num_batches + i``.  The flips slot of the step block holds UB zeros (the student's batch is the plain
       concatenation) and then the two 32-bit halves of the iteration's seed; ``thr`` is word 0 of one more row behind the EMA's;
    2. one launch (``ops.noise_add``) writes the ``1 + passes`` noisy copies ``x[p] = u + clamp(noise_sigma * z[p], +-noise_clip)``,
       the generator seeded from the device words.  The teacher's tracked forward sees ``x[0]``; ``passes`` more forwards under
       ``unet_ops.bn_untracked()`` see ``x[1..]`` and their softmaxes are summed (``ops.softmax_accum``): these move no BatchNorm
       buffer, so the evaluated teacher does not depend on ``passes``;
    3. the student's batch is ``[labeled | u]``, the unlabeled images clean;
    4. the consistency term is ``ops.softmax_umse``: the squared distance of the two softmaxes over the pixels whose predictive
       entropy lies below ``thr``, normalised by their count.

    Backward, the guarded optimiser, the EMA and the meters are ``MeanTeacherEpocher``'s; ``uncertainty`` (mean predictive entropy),
    ``certain`` (share of the pixels below the threshold) and ``threshold`` come on top.  Images must be fp32 4-D tensors: there is no
    torch composition to fall back on, it would freeze the seed under the launch tape."""

    METERS = ("uncertainty", "certain", "threshold")

    def __init__(self, model, teacher_model, optimizer, labeled_loader: T_loader, unlabeled_loader: T_loader, sup_criterion: T_loss,
                 reg_criterion: T_loss, reg_weight: float, num_batches: int, cur_epoch=0, device="cpu", feature_position=None,
                 feature_importance=None, ema_updater=None, passes: int = 8, noise_sigma: float = 0.1, noise_clip: float = 0.2,
                 threshold_start: float = 0.75, threshold_end: float = 1.0, k_total: Optional[int] = None) -> None:
        super().__init__(model, teacher_model, optimizer, labeled_loader, unlabeled_loader, sup_criterion, reg_criterion, reg_weight,
                         num_batches, cur_epoch, device, feature_position, feature_importance, ema_updater)
        if not isinstance(reg_criterion, nn.MSELoss):
            raise KeyError("UAMTEpocher: the masked consistency term is the squared distance (name: mse)")
        if not 1 <= int(passes) <= 32:
            raise ValueError(f"UAMTEpocher: passes must lie in 1..32, got {passes}")
        if float(noise_sigma) < 0.0 or float(noise_clip) < 0.0:
            raise ValueError(f"UAMTEpocher: noise_sigma and noise_clip must not be negative, got {noise_sigma}, {noise_clip}")
        if not 0.0 <= float(threshold_start) <= float(threshold_end):
            raise ValueError(f"UAMTEpocher: 0 <= threshold_start <= threshold_end, got {threshold_start}, {threshold_end}")
        self._passes, self._noise_sigma, self._noise_clip = int(passes), float(noise_sigma), float(noise_clip)
        self._threshold = (float(threshold_start), float(threshold_end))
        self._k_total = int(k_total) if k_total is not None else int(num_batches)
        self._TRAIN_FORWARDS = 2 + self._passes      # the step block's BatchNorm accumulator room (stepio.block_bytes)
        self._iteration = 0
        self._thr = 0.0
        self._thr_sent: List[float] = []             # thresholds of the iterations whose read-back is still under way
        self._acc = None

    def threshold_at(self, i: int) -> float:
        """The threshold of iteration ``i`` (from 0) of this epoch: a function of ``cur_epoch`` and ``i`` only."""
        return uamt_threshold(self._cur_epoch * self._num_batches + i, self._k_total, *self._threshold, self.num_classes)

    def _draw_words(self, seed: int, ub: int) -> List[int]:
        self._thr = self.threshold_at(self._iteration)
        self._iteration += 1
        self._thr_sent.append(self._thr)
        lo, hi = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
        return [0] * ub + [w - (1 << 32) if w >= (1 << 31) else w for w in (lo, hi)]

    def _own_rows(self) -> List[List[float]]:
        return super()._own_rows() + [[float(self._thr)]]

    def _thr_word(self) -> Tensor:
        return stepio.CURRENT.hyper(self._ema_row + 1)[:1]

    def _tape_signature(self):
        return super()._tape_signature() + (self._passes, self._noise_sigma, self._noise_clip) + self._threshold

    def _student_batch(self, labeled_image: Tensor, unlabeled_image: Tensor, flips: Tensor) -> Tensor:
        """``[labeled | unlabeled]``: the flips are zeros, ``_assemble``'s one launch is the plain concatenation."""
        for image in (labeled_image, unlabeled_image):
            if not (torch.is_tensor(image) and image.dtype == torch.float32 and image.dim() == 4 and image.is_cuda):
                raise TypeError(f"Trainer.name=uamt takes fp32 [N,C,H,W] image batches on the GPU, got "
                                f"{getattr(image, 'dtype', type(image))} {tuple(getattr(image, 'shape', ()))}")
        if labeled_image.shape[1:] != unlabeled_image.shape[1:]:
            raise TypeError(f"Trainer.name=uamt: labeled {tuple(labeled_image.shape)} and unlabeled {tuple(unlabeled_image.shape)} images differ")
        return self._assemble(labeled_image, unlabeled_image, flips, keep_unflipped=False)

    def _teacher_forward(self, unlabeled_image: Tensor) -> Tensor:
        ub = len(unlabeled_image)
        noisy = ops.noise_add(unlabeled_image.contiguous(), self._flips2[ub:ub + 2], 1 + self._passes, self._noise_sigma, self._noise_clip)
        teacher_logits = self._teacher_model(noisy[0])           # tracked, as MeanTeacherEpocher's
        acc = None
        with unet_ops.bn_untracked():
            for p in range(1, 1 + self._passes):
                acc = ops.softmax_accum(self._teacher_model(noisy[p]), acc)
        self._acc = acc
        return teacher_logits

    def _consistency(self, student_logits: Tensor, teacher_logits: Tensor, flips: Tensor):
        loss, _kept, stats = ops.softmax_umse(student_logits, teacher_logits, self._acc, self._thr_word(), self._passes)
        self._acc = None
        self._pending.put("certain", stats[0])
        self._pending.put("uncertainty", stats[1])
        return LinearLoss.of(loss)

    def _record(self, host: dict, inter: Tensor, union: Tensor, label_group) -> None:
        super()._record(host, inter, union, label_group)
        self.meters["threshold"].add(self._thr_sent.pop(0))       # records arrive in the order of the iterations


class CPSEpocher(TrainEpocher):
    """``cps``: cross pseudo supervision (Chen et al., CVPR 2021; ``CPSParameters``) -- two trainable networks
    with different initial weights, each held to the other's hard prediction.  One iteration:

    1. the seed is drawn as in every epocher (the host RNG stream stays aligned) and otherwise unused; no flips are drawn or applied,
       the flips slot of the step block holds UB zeros;
    2. ``x = [labeled | unlabeled]``, assembled once (one launch) and fed to both networks;
    3. two training forwards with autograd, ``a = model(x)`` and ``b = model_b(x)``: each in train mode with its own batch statistics
       and running statistics; the ``FeatureExtractor`` stays on ``model``;
    4. ``sup_a`` and ``sup_b``: the supervised criterion on each network's labeled rows;
    5. the cross term (``ops.softmax_cross_pseudo``, one launch) over all rows -- with ``on_labeled`` false over the unlabeled rows
       only --: ``cps_a = mean_px CE(a, argmax b)``, ``cps_b = mean_px CE(b, argmax a)``, labels detached, ``reg_loss = cps_a + cps_b``;
    6. ``sup_a + sup_b + reg_weight * reg_loss``, one backward, the guarded fused optimiser over BOTH networks' parameters (one flat
       buffer): a skipped iteration moves neither network.

    Meters beside ``TrainEpocher``'s: ``sup_loss`` is network A's, ``sup_loss_b`` network B's, ``agreement`` the exact share of the
    term's pixels where the two hard predictions coincide, ``reg_weight``; ``sup_dice`` is network A's.  The term has no
    data-dependent denominator, so data-parallel runs need nothing beyond the gradient all-reduce."""

    _TRAIN_FORWARDS = 2
    METERS = ("sup_loss_b", "agreement", "reg_weight")

    def __init__(self, model, model_b, optimizer, labeled_loader: T_loader, unlabeled_loader: T_loader, sup_criterion: T_loss,
                 reg_weight: float, num_batches: int, cur_epoch=0, device="cpu", feature_position=None, feature_importance=None,
                 on_labeled: bool = True) -> None:
        super().__init__(model, optimizer, labeled_loader, unlabeled_loader, sup_criterion, reg_weight, num_batches, cur_epoch, device,
                         feature_position, feature_importance)
        if float(reg_weight) < 0.0:
            raise ValueError(f"CPSEpocher: the weight of the cross term must not be negative, got {reg_weight}")
        self._model_b = model_b
        self._on_labeled = bool(on_labeled)
        self._pixels_sent: List[int] = []          # pixels of the cross term, of the iterations whose read-back is still under way

    def _run(self, *args, **kwargs) -> EpochResultDict:
        self._model_b.train()
        self.meters["reg_weight"].add(self._reg_weight)
        return super()._run(*args, **kwargs)

    def _draw_words(self, seed: int, ub: int) -> List[int]:
        (lb, _, h, w), _ = self._batch_shapes
        self._pixels_sent.append(((lb if self._on_labeled else 0) + ub) * h * w)
        return [0] * ub

    def _stage(self, io, flip_masks) -> int:
        if not hasattr(self._optimizer, "host_step"):
            raise RuntimeError("Trainer.name=cps needs a fused optimiser (Optim.name: Adam, RAdam, AdaBound or AdaBoundW)")
        return super()._stage(io, flip_masks)

    def _tape_signature(self):
        buf = next(iter(self._model_b.buffers()), None)
        return super()._tape_signature() + (id(self._model_b), None if buf is None else buf.data_ptr(), self._on_labeled)

    def _device_step(self, labeled_image: Tensor, labeled_target: Tensor, unlabeled_image: Tensor, flips2: Tensor, seed: int = None):
        lb, ub = len(labeled_image), len(unlabeled_image)
        self._flips2 = flips2
        batch = self._assemble(labeled_image, unlabeled_image, flips2[:ub], keep_unflipped=False)      # zero flips: the plain concatenation
        logits_a = self._forward(batch, ub)
        with checks.deferred(self._pending.checks):
            logits_b = self._model_b(batch)
        label_a, unlabel_a = ops.split_rows(logits_a, [lb, ub])
        label_b, unlabel_b = ops.split_rows(logits_b, [lb, ub])
        labels = labeled_target.squeeze(1)
        io = stepio.CURRENT
        with checks.deferred(self._pending.checks):
            sup_a = supervised_loss(self._sup_criterion, label_a, labels, self.num_classes)
            sup_b = supervised_loss(self._sup_criterion, label_b, labels, self.num_classes)
            # the count rides in the read-back block as the integer it is; the host divides it by the pixels (_record)
            count = None if io is None else io.out("agree", (1,), torch.int64)
            if self._on_labeled:
                cross, _ = ops.softmax_cross_pseudo((label_a, unlabel_a), (label_b, unlabel_b), count)
            else:
                cross, _ = ops.softmax_cross_pseudo(unlabel_a, unlabel_b, count)
        self._pending.put("sup_loss_b", sup_b)
        return self._finish_step(sup_a, LinearLoss.of(cross), label_a, labels, more_loss=sup_b)

    def _record(self, host: dict, inter: Tensor, union: Tensor, label_group) -> None:
        super()._record(host, inter, union, label_group)
        # ``agree``: the block's extra field, handed through by ``_Pending.wait``; records arrive in the order of the iterations
        self.meters["agreement"].add(int(host["agree"][0]) / self._pixels_sent.pop(0))


class MIDLTrainEpocher(UDATrainEpocher):
    """``midl``: the UDA iteration (same flips, same ``[labeled | unlabeled | flip(unlabeled)]`` forward, same supervised KL) whose
    regulariser adds the local mutual information of the network's OUTPUT (``MIDLPaperParameters``):

        x = softmax(flip(unlabeled_logits)), y = softmax(unlabeled_tf_logits)               (the IIC tap's order, ref :249-275)
        reg = cons_weight * UDA(y, x.detach()) + iic_weight * IIDSegmentationSmallPathLoss(padding, patch_size)(x, y)

    with reg_weight 1 (as udaiic, ref trainer.py:187-196).  Neither side of the MI term is detached.  The MI term is one library
    node (``ops.output_local_mi``: softmaxes in registers, the local-MI epilogue, a backward that ends on the logits and adds into
    the consistency gradient's rows); shapes outside its envelope (more than 8 classes, padding above 3) run the reference's
    composition -- torch softmax and this repo's generic ``IIDSegmentationSmallPathLoss`` -- eagerly: the launch tape then declines
    with its usual warning.  Meters: the base ones, ``uda`` and ``mi`` (= -MI loss, the sign ``IICTrainEpocher`` reports)."""

    METERS = ("mi",)

    def __init__(self, model, optimizer, labeled_loader, unlabeled_loader, sup_criterion, reg_criterion: T_loss, num_batches: int,
                 cur_epoch: int = 0, device="cpu", feature_position=None, feature_importance=None, cons_weight: float = 5.0,
                 iic_weight: float = 0.1, padding: int = 1, patch_size=1024) -> None:
        super().__init__(model, optimizer, labeled_loader, unlabeled_loader, sup_criterion, reg_criterion, 1.0, num_batches, cur_epoch,
                         device, feature_position, feature_importance)
        from contrastyou.losses.iic_loss import IIDSegmentationSmallPathLoss
        self._cons_weight, self._iic_weight = float(cons_weight), float(iic_weight)
        self._mi_criterion = IIDSegmentationSmallPathLoss(lamda=1.0, padding=int(padding), patch_size=patch_size)

    def windows(self, h: int, w: int):
        """The criterion's patches of an h x w map, (h0, h1, w0, w1) in the reference's order (patch_generator)."""
        from contrastyou.losses.iic_loss import _windows
        crit = self._mi_criterion
        return _windows(h, w, crit._patch_size, crit._step_size)

    def _mi(self, unlabeled_tf_logits: Tensor, unlabeled_logits: Tensor, flips: Tensor):
        crit = self._mi_criterion
        c, h, w = unlabeled_tf_logits.shape[1:]
        if ops.output_local_mi_supported(c, crit.padding):
            losses = ops.output_local_mi(unlabeled_tf_logits, unlabeled_logits, flips, crit.padding, self.windows(h, w), crit.lamda)
            checks.raise_if_nan(losses, "midl: a patch loss of the output MI is nan")
            return LinearLoss.mean(losses)
        # out of the fused envelope: the reference's composition on the generic local-MI kernels (eager; the tape declines)
        x = ops.flip(unlabeled_logits, flips).softmax(1)
        y = unlabeled_tf_logits.float().softmax(1)
        return crit(x.float(), y)

    @_fused
    def regularization(self, unlabeled_tf_logits: Tensor, unlabeled_logits_tf: Tensor = None, seed=None, *args,
                       unlabeled_logits: Tensor = None, flips: Tensor = None, **kwargs):
        # the MI node first: its backward then runs after the consistency term's and adds into the rows that one has written
        mi_loss = self._mi(unlabeled_tf_logits, unlabeled_logits, flips)
        cons_loss = self._uda(unlabeled_tf_logits, unlabeled_logits, flips)
        self._pending.put("mi", -mi_loss)
        return self._cons_weight * cons_loss + self._iic_weight * mi_loss

    def _tape_signature(self):
        crit = self._mi_criterion
        return super()._tape_signature() + (self._iic_weight, crit.padding, crit.lamda, tuple(crit._patch_size), tuple(crit._step_size))


class EntropyMinEpocher(TrainEpocher):
    """``entmin``: the ``partial`` iteration (same flips, same ``[labeled | unlabeled | flip(unlabeled)]`` forward, same supervised
    KL) whose regulariser is the entropy of the prediction on the unlabeled batch (``EntropyMinParameters``):

        reg   = Entropy(reduction="mean", eps=1e-16)(softmax(flip(unlabeled_logits)))  = mean_{n,h,w} -sum_c p_c log(p_c + 1e-16)
        total = sup_loss + reg_weight * reg                  (reg_weight = EntropyMinParameters.weight)

    The mean over pixels does not depend on the flip, so the fused kernel (``ops.softmax_entropy``) reads the ``unlabeled`` rows of
    the logits batch in place and writes its gradient into those rows of the batch gradient; the ``flip(unlabeled)`` rows get none
    (``split_rows``' backward zero-fills them).  A class count the kernel does not have (e.g. 7) runs the torch composition
    eagerly: the launch tape then declines with its usual warning.  Meters: the base ones plus ``entropy``, the unweighted value
    (``reg_loss`` reports the same number, as ``uda``'s does)."""

    METERS = ("entropy",)

    def __init__(self, model, optimizer, labeled_loader, unlabeled_loader, sup_criterion, reg_weight: float, num_batches: int,
                 cur_epoch: int = 0, device="cpu", feature_position=None, feature_importance=None) -> None:
        super().__init__(model, optimizer, labeled_loader, unlabeled_loader, sup_criterion, reg_weight, num_batches, cur_epoch,
                         device, feature_position, feature_importance)
        self._entropy_criterion = Entropy()

    @_fused
    def regularization(self, unlabeled_tf_logits: Tensor, unlabeled_logits_tf: Tensor = None, seed=None, *args,
                       unlabeled_logits: Tensor = None, flips: Tensor = None, **kwargs):
        crit = self._entropy_criterion
        if crit.supports_fused() and ops.softmax_entropy_supported(unlabeled_logits.shape[1]):
            loss = LinearLoss.of(crit.from_logits(unlabeled_logits))
        else:  # no kernel for this class count: the reference expression on materialised operands (eager; the tape declines)
            loss = crit(ops.flip(unlabeled_logits, flips).float().softmax(1))
        self._pending.put("entropy", loss)
        return loss


class VATEpocher(TrainEpocher):
    """``vat``: virtual adversarial training (``VATParameters``).  One iteration:

        sup   = KL(softmax(f(x_l)), onehot(y_l))          the labeled batch alone, as its own BatchNorm batch
        reg   = VATLoss(xi, eps, prop_eps, ip)(f, x_u)    deepclustering2.utils.VAT: clean pass, ``ip`` direction passes, perturbed pass
        total = sup + reg_weight * reg                    one backward, Adam

    ``3 + ip`` U-Net forwards per iteration: the labeled and the clean unlabeled pass move the BatchNorm running statistics (in that
    order), the direction and perturbed passes use batch statistics and leave them alone.  The passes of the loss take their batch
    statistics from float partial sums (``unet_ops.bn_float_statistics``), the labeled pass from the step block's accumulators.  The direction passes' backward computes
    data gradients only -- down to the image, through ``miseg_conv3x3_stem_dgrad`` -- and touches no ``param.grad``; the weights are
    used twice by the parameter backward (labeled and perturbed pass) and autograd adds the second gradient to the flat slot the
    first one wrote.  The unlabeled loader's flip decisions are drawn as in ``partial`` (the host random streams stay aligned) and not
    applied.  The random direction is the library generator's, seeded with the iteration's seed.  A direction of zero / non-finite
    norm raises a deferred check: the guarded Adam skips that update and the host raises one iteration later.

    The iteration runs eagerly: ``enable_step_tape`` is a no-op here.  A replayed launch tape repeats the recorded arguments, and
    ``miseg_normal_fill`` takes its seed by value: every replay would draw the recorded iteration's direction.  (The direction pass
    also scales the distance's gradient with one torch product, which the recording would refuse.)  Meters: the base ones plus
    ``reg_weight``."""

    _TAPE_DEFAULT = False
    METERS = ("reg_weight",)

    def __init__(self, model, optimizer, labeled_loader, unlabeled_loader, sup_criterion, reg_weight: float, num_batches: int,
                 cur_epoch: int = 0, device="cpu", feature_position=None, feature_importance=None, xi: float = 10.0, eps: float = 1.0,
                 prop_eps: float = 0.25, ip: int = 1) -> None:
        super().__init__(model, optimizer, labeled_loader, unlabeled_loader, sup_criterion, reg_weight, num_batches, cur_epoch,
                         device, feature_position, feature_importance)
        from deepclustering2.utils.VAT import VATLoss
        self._vat = VATLoss(xi=xi, eps=eps, prop_eps=prop_eps, ip=ip)

    def enable_step_tape(self, warmup: int = 3) -> None:
        """No-op: the ``vat`` iteration runs eagerly (class docstring)."""

    def _run(self, *args, **kwargs) -> EpochResultDict:
        self.meters["reg_weight"].add(self._reg_weight)
        return super()._run(*args, **kwargs)

    def _device_step(self, labeled_image: Tensor, labeled_target: Tensor, unlabeled_image: Tensor, flips2: Tensor, seed: int = None):
        seed = self._seed if seed is None else seed
        self._flips2 = flips2
        labels = labeled_target.squeeze(1)
        with checks.deferred(self._pending.checks):
            label_logits = self._forward(labeled_image, len(unlabeled_image))
            sup_loss = supervised_loss(self._sup_criterion, label_logits, labels, self.num_classes)
            lds, _, _ = self._vat(self._model, unlabeled_image, seed=seed)
        return self._finish_step(LinearLoss.of(sup_loss), LinearLoss.of(lds), label_logits, labels)


class PretrainEncoderEpocher(_Epocher):
    """``contrast``: contrastive pre-training of the encoder (ref contrastyou/epocher/contrast_epocher.py:21-113, DESIGN.md section
    14).  One iteration: unpack the two augmented views, ONE train-mode forward of ``cat([img, img_tf])`` up to ``extract_position``
    (BatchNorm sees the concatenated batch), the projection head, the supervised-contrastive loss of the raw embeddings with the
    labels of ``group_option`` (``SupConLoss.from_embeddings``: normalisation, loss and gradient in one library call), backward, Adam.
    The loss is read once per iteration -- before backward, so a NaN raises ``RuntimeError`` with the weights unmoved.  Eager: the
    launch tape does not record this epocher.  Meters: ``contrastive_loss``, ``lr``.

    Against the reference: the network stops at ``extract_position`` (``UNet.encode``; the reference runs the decoder and discards
    its output), and the optimiser holds the parameters of ``Conv1..extract_position`` and the projector only (the trainer's
    ``_trainable``)."""

    def __init__(self, model, projection_head: nn.Module, optimizer: T_optim, pretrain_loader: T_loader, contrastive_criterion: T_loss,
                 num_batches: int, cur_epoch=0, device="cpu", group_option: str = "partition", extract_position: str = "Conv5") -> None:
        assert isinstance(num_batches, int) and num_batches > 0, num_batches
        super().__init__(model, num_batches=num_batches, cur_epoch=cur_epoch, device=device)
        self._projection_head = projection_head
        self._optimizer = optimizer
        self._pretrain_loader = pretrain_loader
        self._contrastive_criterion = contrastive_criterion
        assert group_option in ("partition", "patient", "both"), group_option
        self._group_option = group_option
        self._label_generator = GlobalLabelGenerator(contrastive_on_patient=group_option in ("patient", "both"),
                                                     contrastive_on_partition=group_option in ("partition", "both"))
        net = getattr(model, "module", model)
        assert extract_position in net.component_names, extract_position
        self._extract_position = extract_position

    def to(self, device=torch.device("cpu")):
        super().to(device)
        self._projection_head.to(self._device)

    def _configure_meters(self, meters: MeterInterface) -> MeterInterface:
        meters.register_meter("contrastive_loss", AverageValueMeter())
        meters.register_meter("lr", AverageValueMeter())
        return meters

    def _loss(self, data) -> Tensor:
        """Forward half of an iteration: the contrastive loss of one batch of the loader (a 0-d tensor with its graph)."""
        (img, _), (img_tf, _), _filename, partition_list, group_list = preprocess_input_with_twice_transformation(data, self._device)
        net = getattr(self._model, "module", self._model)
        feature = net.encode(torch.cat([img, img_tf], dim=0), util=self._extract_position)
        embeddings = self._projection_head(feature)
        labels = self._label_generator(partition_list=list(partition_list), patient_list=list(group_list))
        return self._contrastive_criterion.from_embeddings(embeddings, labels)

    def _step(self, data) -> float:
        """One iteration; returns the loss value (the iteration's one host read, taken before backward)."""
        loss = self._loss(data)
        value = loss.item()
        if value != value:
            raise RuntimeError(f"contrastive loss is nan (epoch {self._cur_epoch})")
        self._optimizer.zero_grad()
        loss.backward()
        self._optimizer.step()
        return value

    def _run(self, *args, **kwargs) -> EpochResultDict:
        self._model.train()
        self._projection_head.train()
        assert self._model.training, self._model.training
        self.meters["lr"].add(get_lrs_from_optimizer(self._optimizer)[0])
        report_dict = {}
        for _, data in zip(self._indicator, self._pretrain_loader):
            self.meters["contrastive_loss"].add(self._step(data))
            report_dict = self.meters.tracking_status()
            self._indicator.set_postfix_dict(report_dict)
        return report_dict


class PretrainDecoderEpocher(PretrainEncoderEpocher):
    """``contrastdecoder``: contrastive pre-training of the decoder (ref contrastyou/epocher/contrast_epocher.py:116-176, DESIGN.md
    section 15).  One iteration: unpack the two views (same geometric transform, different colour jitter); draw a seed and, under
    ``FixRandomSeed(seed)``, one H/W flip mask per sample; ONE train-mode forward of ``cat([flip(img), img_ctf])`` up to
    ``extract_position``; flip the second half of the feature map with the same masks; ``LocalProjectionHead.embeddings`` (two
    convolutions, the adaptive max-pool and the 2x2 position unfold, the rows written by the pool kernel); the supervised-contrastive
    loss with the labels of ``LocalLabelGenerator`` (equal patient, partition and block position); backward, Adam.  Both flips are one
    ``ops.flip`` over all 2B samples with masks of zero for the half that stays.  The loss is read once per iteration, before backward.
    Eager: the launch tape does not record this epocher.  Meters: ``contrastive_loss``, ``lr``.

    Against the reference: the network stops at ``extract_position`` and the optimiser holds the parameters of ``enable_grad_from ..
    extract_position`` and the projector only (the trainer's ``_trainable``)."""

    def __init__(self, model, projection_head: nn.Module, optimizer: T_optim, pretrain_decoder_loader: T_loader, contrastive_criterion: T_loss,
                 num_batches: int, cur_epoch=0, device="cpu", extract_position: str = "Up_conv3", partition_num=(2, 2)) -> None:
        super().__init__(model, projection_head, optimizer, pretrain_decoder_loader, contrastive_criterion, num_batches, cur_epoch=cur_epoch,
                         device=device, group_option="both", extract_position=extract_position)
        self._label_generator = LocalLabelGenerator()
        self._transformer = TensorRandomFlip(axis=[1, 2], threshold=0.5)
        self._partition_num = tuple(int(v) for v in partition_num)
        self.last_flip_masks = None      # the masks of the latest iteration (tests compare them with the reference's draws)

    def _locations(self, batch: int):
        """``unfold_position``'s second result for one view of ``batch`` samples: the pixel offset of each row's block in the pooled map."""
        oh, ow = self._projection_head._output_size
        bh, bw = oh // self._partition_num[0], ow // self._partition_num[1]
        return [(top, left) for top in range(0, oh - bh + 1, bh) for left in range(0, ow - bw + 1, bw) for _ in range(batch)]

    def _loss(self, data) -> Tensor:
        (img, _), (img_ctf, _), _filename, partition_list, group_list = preprocess_input_with_twice_transformation(data, self._device)
        batch = img.shape[0]
        seed = random.randint(0, int(1e5))
        with FixRandomSeed(seed):
            masks = ops.flip_masks(self._transformer.decisions(batch))
        self.last_flip_masks = list(masks)
        still = [0] * batch
        net = getattr(self._model, "module", self._model)
        images = ops.flip(torch.cat([img, img_ctf], dim=0), torch.tensor(masks + still, dtype=torch.int32, device=img.device))
        feature = net.encode(images, util=self._extract_position)
        feature = ops.flip(feature, torch.tensor(still + masks, dtype=torch.int32, device=img.device))
        embeddings = self._projection_head.embeddings(feature, views=2, partition_num=self._partition_num)
        labels = self._label_generator(list(partition_list), list(group_list), self._locations(batch))
        return self._contrastive_criterion.from_embeddings(embeddings, labels)
