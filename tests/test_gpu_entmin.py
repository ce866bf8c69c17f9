"""GPU: the `entmin` trainer (``Trainer.name=entmin``) -- the fused softmax-entropy kernel against float64
autograd (plain and as a part of a split batch, every class count, peaked logits, the grid-stride path), determinism, refusals, the
composed fallback, the epocher against the reference's own run (tests/golden/entmin.npz), the step under the launch tape and the CLI."""
import os
import shutil
from functools import partial

import numpy as np
import pytest
import torch

import synth
import trainer_harness as th
from trainer_harness import DEV, FEATURES

pytestmark = pytest.mark.gpu
T = torch.from_numpy
CLASS_COUNTS = (2, 3, 4, 5, 6, 8, 10, 16)
_dump = partial(th.error_dump, "entmin")          # the numbers DESIGN.md section 13 quotes


def _logits(c, scale, shape=(3, 37, 53)):
    g = torch.Generator().manual_seed(1000 * c + int(scale))
    return torch.randn(shape[0], c, shape[1], shape[2], generator=g) * scale


def _reference(z):
    """float64 autograd on the CPU: Entropy(reduction='mean', eps=1e-16)(softmax(z, 1)) and its gradient."""
    z64 = z.double().requires_grad_()
    p = z64.softmax(1)
    loss = (-(p * (p + 1e-16).log()).sum(1)).mean()
    loss.backward()
    return float(loss), z64.grad


def _rel(got, ref):
    return float((got - ref).abs().max() / ref.abs().max())


def _nhwc(t):
    return t.to(DEV).contiguous(memory_format=torch.channels_last)


# ---------------------------------------------------------------------------------------------------------------- 1. the kernel
# Bounds: the specification's 1e-5 for a loss, and the same relative to the largest entry for the gradients.  A torch fp32 evaluation of
# the reference expression on the CPU is <= 1.5e-7 (loss) and <= 7e-7 (gradients) from float64 on these inputs, so the bounds leave the
# kernel more than ten times the reference's own error.  Achieved: DESIGN.md section 13.
LOSS_BOUND, GRAD_BOUND = 1e-5, 1e-5


@pytest.mark.parametrize("scale", [2.0, 12.0])
@pytest.mark.parametrize("c", CLASS_COUNTS)
def test_kernel_against_float64_plain_tensor(c, scale):
    """[3, C, 37, 53] (5883 pixels: no multiple of the block), ``randn * 2`` and the peaked ``randn * 12``."""
    from miseg_amd import ops
    z = _logits(c, scale)
    ref_loss, ref_grad = _reference(z)
    zd = _nhwc(z).requires_grad_()
    loss = ops.softmax_entropy(zd)
    loss.backward()
    err = {"value": ref_loss, "loss": abs(float(loss) - ref_loss) / abs(ref_loss), "grad": _rel(zd.grad.cpu().double(), ref_grad)}
    print("entmin plain", c, scale, err)
    _dump(f"kernel_plain_c{c}_s{int(scale)}", err)
    assert err["loss"] < LOSS_BOUND and err["grad"] < GRAD_BOUND, err


@pytest.mark.parametrize("scale", [2.0, 12.0])
@pytest.mark.parametrize("c", CLASS_COUNTS)
def test_kernel_against_float64_as_the_middle_part_of_a_split_batch(c, scale):
    """The trainer's arrangement: [first | middle | last] = one NHWC batch through ``split_rows``; the entropy reads the middle part
    and hands its rows of the batch gradient over (in place where the rows start on a 16-byte boundary -- C = 4, 8, 16 here --, through
    the split's copy otherwise), the first part's rows are what its own loss (a fused softmax-KL) wrote, the last part has no loss and
    comes out exactly zero."""
    from miseg_amd import ops
    from miseg_amd.lazy import LinearLoss
    z = _logits(c, scale)
    g = torch.Generator().manual_seed(c)
    first, last = torch.randn(2, c, 37, 53, generator=g), torch.randn(3, c, 37, 53, generator=g)
    labels = torch.randint(0, c, (2, 37, 53), generator=g)
    ref_loss, ref_grad = _reference(z)
    batch = _nhwc(torch.cat([first, z, last])).requires_grad_()
    pf, pm, pl = ops.split_rows(batch, [2, 3, 3])
    sup = ops.softmax_kl(pf, labels.to(DEV))
    ent = ops.softmax_entropy(pm)
    (LinearLoss.of(sup) + 0.5 * LinearLoss.of(ent)).backward()
    grad = batch.grad.cpu().double()
    # the first part alone: the same KL on a plain tensor
    fd = _nhwc(first).requires_grad_()
    ops.softmax_kl(fd, labels.to(DEV)).backward()
    err = {"value": ref_loss, "loss": abs(float(ent) - ref_loss) / abs(ref_loss), "grad": _rel(grad[2:5], 0.5 * ref_grad)}
    print("entmin split", c, scale, err)
    _dump(f"kernel_split_c{c}_s{int(scale)}", err)
    assert err["loss"] < LOSS_BOUND and err["grad"] < GRAD_BOUND, err
    assert torch.equal(batch.grad[5:], torch.zeros_like(batch.grad[5:]))
    assert torch.equal(batch.grad[:2], fd.grad)
    assert batch.grad.is_contiguous(memory_format=torch.channels_last)


def test_grid_stride_path_against_float64():
    """[1, 4, 768, 768]: 589824 pixels > 2048 blocks x 256 threads, every thread loops; 2304 > 2048 partials in the finish."""
    from miseg_amd import ops
    z = _logits(4, 2.0, shape=(1, 768, 768))
    ref_loss, ref_grad = _reference(z)
    zd = _nhwc(z).requires_grad_()
    loss = ops.softmax_entropy(zd)
    loss.backward()
    err = {"value": ref_loss, "loss": abs(float(loss) - ref_loss) / abs(ref_loss), "grad": _rel(zd.grad.cpu().double(), ref_grad)}
    print("entmin grid-stride", err)
    _dump("kernel_gridstride", err)
    assert err["loss"] < LOSS_BOUND and err["grad"] < GRAD_BOUND, err


def _raw_call(z, with_grad=True):
    from miseg_amd import _cabi
    n, c, h, w = z.shape
    loss = torch.full((1,), float("nan"), device=DEV)
    grad = torch.full_like(z, float("nan")) if with_grad else None
    ws = torch.empty(max(int(_cabi.lib().miseg_loss_ws_bytes(n, h, w)), 16), dtype=torch.uint8, device=DEV)
    _cabi.call("miseg_softmax_entropy", torch.cuda.current_stream().cuda_stream, z.data_ptr(), n, h, w, c, None, loss.data_ptr(),
               None if grad is None else grad.data_ptr(), ws.data_ptr(), ws.numel())
    return loss, grad


def test_two_calls_are_bit_identical_and_forward_only_gives_the_same_loss():
    z = _nhwc(_logits(4, 2.0, shape=(2, 300, 301)))
    l1, g1 = _raw_call(z)
    l2, g2 = _raw_call(z)
    l3, _ = _raw_call(z, with_grad=False)
    torch.cuda.synchronize()
    assert torch.equal(l1, l2) and torch.equal(g1, g2) and torch.equal(l1, l3)
    assert torch.isfinite(l1).all() and torch.isfinite(g1).all()


def test_upstream_scales_the_gradient_only():
    from miseg_amd import _cabi
    z = _nhwc(_logits(3, 2.0))
    n, c, h, w = z.shape
    l1, g1 = _raw_call(z)
    up = torch.tensor([0.25], device=DEV)
    loss, grad = torch.empty(1, device=DEV), torch.empty_like(z)
    ws = torch.empty(int(_cabi.lib().miseg_loss_ws_bytes(n, h, w)), dtype=torch.uint8, device=DEV)
    _cabi.call("miseg_softmax_entropy", torch.cuda.current_stream().cuda_stream, z.data_ptr(), n, h, w, c, up.data_ptr(), loss.data_ptr(),
               grad.data_ptr(), ws.data_ptr(), ws.numel())
    assert torch.equal(loss, l1)
    torch.testing.assert_close(grad, g1 * 0.25, rtol=2e-7, atol=0)


def test_unsupported_class_count_and_empty_batch_are_refused():
    """C = 7 and npix = 0: MisegError from the C ABI, nothing launched (the outputs keep their fill)."""
    from miseg_amd import _cabi, ops
    assert not ops.softmax_entropy_supported(7)
    z = _nhwc(torch.randn(1, 7, 8, 8))
    with pytest.raises(_cabi.MisegError, match="unsupported class count"):
        ops.softmax_entropy(z)
    loss, grad = torch.full((1,), 3.0, device=DEV), torch.full_like(z, 3.0)
    ws = torch.zeros(64, dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    with pytest.raises(_cabi.MisegError):
        _cabi.call("miseg_softmax_entropy", stream, z.data_ptr(), 1, 8, 8, 7, None, loss.data_ptr(), grad.data_ptr(), ws.data_ptr(), 64)
    z4 = _nhwc(torch.randn(1, 4, 8, 8))
    for n, h, w in ((0, 8, 8), (1, 0, 8), (1, 8, 0)):
        with pytest.raises(_cabi.MisegError):
            _cabi.call("miseg_softmax_entropy", stream, z4.data_ptr(), n, h, w, 4, None, loss.data_ptr(), None, ws.data_ptr(), 64)
    with pytest.raises(_cabi.MisegError):          # a workspace smaller than miseg_loss_ws_bytes
        _cabi.call("miseg_softmax_entropy", stream, z4.data_ptr(), 1, 64, 64, 4, None, loss.data_ptr(), None, ws.data_ptr(), 8)
    torch.cuda.synchronize()
    assert float(loss) == 3.0 and bool((grad == 3.0).all()) and not bool(ws.any())


def test_fallback_without_a_kernel_matches_float64():
    """C = 7: the epocher composes ``Entropy()(flip(logits).softmax(1))`` with torch and returns a tensor, not a LinearLoss."""
    from semi_seg.epocher import EntropyMinEpocher, _Pending
    from deepclustering2.loss import Entropy
    ep = EntropyMinEpocher.__new__(EntropyMinEpocher)
    ep._entropy_criterion, ep._pending = Entropy(), _Pending()
    for scale in (2.0, 12.0):
        z = _logits(7, scale)
        ref_loss, ref_grad = _reference(z)
        zd = z.to(DEV).requires_grad_()
        flips = torch.tensor([1, 2, 3], dtype=torch.int32, device=DEV)
        loss = ep.regularization(None, None, 0, unlabeled_logits=zd, flips=flips)
        assert isinstance(loss, torch.Tensor)
        loss.backward()
        err = {"loss": abs(float(loss) - ref_loss) / abs(ref_loss), "grad": _rel(zd.grad.cpu().double(), ref_grad)}
        _dump(f"fallback_s{int(scale)}", err)
        assert err["loss"] < LOSS_BOUND and err["grad"] < GRAD_BOUND, err
    assert ep._pending._names == ["entropy", "entropy"]


def test_fused_path_returns_a_linear_loss_and_reports_entropy():
    from miseg_amd.lazy import LinearLoss
    from semi_seg.epocher import EntropyMinEpocher, _Pending
    from deepclustering2.loss import Entropy
    ep = EntropyMinEpocher.__new__(EntropyMinEpocher)
    ep._entropy_criterion, ep._pending = Entropy(), _Pending()
    z = _logits(4, 2.0)
    loss = ep.regularization(None, None, 0, unlabeled_logits=_nhwc(z).requires_grad_(), flips=None)
    assert isinstance(loss, LinearLoss) and ep._pending._names == ["entropy"]
    assert abs(float(loss.value()) - _reference(z)[0]) < LOSS_BOUND * _reference(z)[0]


# ---------------------------------------------------------------------------------------------------------------- 2. the epocher
def _golden_run(g, monkeypatch):
    from deepclustering2.loss import KL_div
    from deepclustering2.optim import Adam
    from semi_seg import epocher as E
    cfg = th.golden_cfg(g)
    H, LB, UB, NB = int(cfg["H"]), int(cfg["LB"]), int(cfg["UB"]), int(cfg["NB"])
    model = th.unet("float32", int(cfg["model_seed"]))
    opt = Adam(model.parameters(), lr=float(cfg["lr"]), weight_decay=float(cfg["wd"]))
    lab = [(T(synth.uniform(f"entmin/lab{i}", (LB, 1, H, H))), T(synth.integers(f"entmin/tgt{i}", (LB, 1, H, H), 4))) for i in range(NB)]
    unl = [T(synth.uniform(f"entmin/unl{i}", (UB, 1, H, H))) for i in range(NB)]
    th.replay_seeds(monkeypatch, g["seeds"])
    with th.adam_gradients(monkeypatch) as grads:
        ep = E.EntropyMinEpocher(model, opt, th.reference_batches([a for a, _ in lab], [b for _, b in lab], LB),
                                 th.reference_batches(unl, [torch.zeros(UB, 1, H, H, dtype=torch.long)] * NB, UB), KL_div(verbose=False),
                                 float(cfg["weight"]), NB, 0, DEV, feature_position=FEATURES, feature_importance=th.IMPORTANCE)
        ep._TAPE_DEFAULT = False
        per_step = th.keep_records(ep)
        res = ep.run()
    return res, grads[0].cpu(), per_step, opt


def test_epocher_matches_the_reference_run(golden, monkeypatch):
    """fp32, tape off, 3 iterations against the reference's TrainEpocher with the wheel's Entropy as regulariser at weight 1
    (tests/golden/entmin.npz): step-1 gradients at the first-iteration bounds of test_gpu_step, per-step losses, the meter key set,
    the decoder tail after the last step."""
    g = golden("entmin")
    res, grad, per_step, opt = _golden_run(g, monkeypatch)
    named = dict(zip((str(n) for n in g["param_names"]), opt.flat.given))
    assert len(named) == len(opt.flat.given)
    worst = th.sampled_rel_l2(g, "grad_step1", grad, named, opt.flat.offset_of)
    tail = sorted(v for k, v in worst.items() if k.startswith(("Up_conv2", "DeConv")))
    print("entmin golden gradients: logits layer", max(v for k, v in worst.items() if k.startswith("DeConv")), "tail", tail[0],
          tail[len(tail) // 2], tail[-1], "all", max(worst.values()))
    _dump("golden_grad", worst)
    # the first-iteration bounds of test_gpu_step::test_step_gradients_match_reference; measured: logits layer 6.0e-6, last block
    # 5.3e-6 (tightest) / 3.3e-4 (median) / 1.8e-3 (worst), any tensor 4.7e-3.  The fixture's own fp32 error against a float64 run of
    # the reference is stored in it (own_error/*: 6.5e-6 / 3.7e-4 / 5.0e-4 / 1.4e-3; make_golden_entmin.py says how its seed was taken)
    assert max(v for k, v in worst.items() if k.startswith("DeConv")) < 2e-5, worst
    assert tail[len(tail) // 2] < 5e-3 and tail[0] < 1e-5 and tail[-1] < 1.5e-2, tail
    assert max(worst.values()) < 3e-2, worst
    assert len(per_step) == 3
    print("entmin golden steps:", per_step, list(g["sup_loss"]), list(g["entropy"]))
    np.testing.assert_allclose(per_step[0]["sup_loss"], g["sup_loss"][0], rtol=2e-5)
    np.testing.assert_allclose(per_step[0]["entropy"], g["entropy"][0], rtol=2e-5)
    np.testing.assert_allclose(per_step[0]["reg_loss"], g["entropy"][0], rtol=2e-5)
    np.testing.assert_allclose([s["sup_loss"] for s in per_step], g["sup_loss"], rtol=3e-3)
    np.testing.assert_allclose([s["entropy"] for s in per_step], g["entropy"], rtol=3e-3)
    assert [s["reg_loss"] for s in per_step] == [s["entropy"] for s in per_step]
    # the decoder tail after 3 Adam steps: near-zero gradients' signs move a weight by up to 2 lr per step
    last = {n: q for n, q in named.items() if n.startswith(("Up_conv2", "DeConv_1x1"))}
    for n, d in th.sampled_max_abs(g, "param_after", opt.flat.flat_param, last, opt.flat.offset_of).items():
        assert d <= 7.5e-3, (n, d)
    keys = [str(k) for k in g["meter_keys"]]
    got = th.meter_items(res)
    assert sorted(got) == sorted(keys), (sorted(got), sorted(keys))
    ref = dict(zip(keys, (float(v) for v in g["meter_values"])))
    np.testing.assert_allclose(got["sup_loss/mean"], ref["sup_loss/mean"], rtol=3e-3)
    np.testing.assert_allclose(got["entropy/mean"], ref["entropy/mean"], rtol=3e-3)
    np.testing.assert_allclose(got["reg_loss/mean"], ref["reg_loss/mean"], rtol=3e-3)


# ---------------------------------------------------------------------------------------------------------------- 3. the tape
def build(dtype="float32", num_batches=7, weight=1.0):
    from deepclustering2.loss import KL_div
    from deepclustering2.optim import Adam
    from semi_seg.epocher import EntropyMinEpocher
    from semi_seg.synthetic import SyntheticPairs
    model = th.unet(dtype, 41)
    opt = Adam(model.parameters(), lr=1e-3, weight_decay=1e-5)
    lab = SyntheticPairs(2, 64, 4, seed=0, device=DEV)
    unl = SyntheticPairs(2, 64, 4, seed=1, device=DEV)
    ep = EntropyMinEpocher(model, opt, iter(lab), iter(unl), KL_div(verbose=False), weight, num_batches, 0, DEV,
                           feature_position=FEATURES, feature_importance=th.IMPORTANCE)
    return ep, model, opt


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_entmin_tape_replay_equals_eager_steps(dtype):
    """2 eager + 1 recorded + 4 replayed iterations give the parameters, Adam's moments and the meters of 7 eager ones, bit for bit.
    The recorded iteration has no ATen launch (the tape would have been refused), one launch of the new entry point and no
    consistency kernel."""
    got, info = th.run_steps(lambda: build(dtype), 7, True)
    ref, _ = th.run_steps(lambda: build(dtype), 7, False)
    th.assert_replayed(info, 4)
    names = info.op_names
    assert names.count("miseg_softmax_entropy") == 1 and names.count("miseg_softmax_mse") == 0, names
    th.assert_same_state(got, ref, ("param", "m", "v", "meters"))
    assert "entropy" in got["meters"]


def test_changed_weight_rerecords_the_tape():
    ep, _, _ = build()
    sig = ep._tape_signature()
    assert ep._tape_signature() == sig
    ep._reg_weight = 0.5
    assert ep._tape_signature() != sig


# ---------------------------------------------------------------------------------------------------------------- 4. the CLI
_TINY = ["Trainer.device=cuda", "Trainer.max_epoch=2", "Trainer.num_batches=3", "Data.size=64", "LabeledData.batch_size=2",
         "UnlabeledData.batch_size=2"]


@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
def test_main_cli_runs_entmin(golden, dtype):
    """``python semi_seg/main.py Trainer.name=entmin EntropyMinParameters.weight=0.001``: two tiny epochs; config.yaml, last.pth and a
    storage CSV with an entropy column; the checkpoint's key tree is the partial trainer's (tests/golden/trainer_io.npz) plus the
    entropy history (and, in fp16, the loss scaler); inference() runs on it in a fresh process."""
    save = f"pytest_cli_entmin_{dtype}_{os.getpid()}"
    run_dir = th.run_dir(save)
    shutil.rmtree(run_dir, ignore_errors=True)
    try:
        th.run_main(["Trainer.name=entmin", "EntropyMinParameters.weight=0.001", f"Trainer.save_dir={save}", f"Arch.compute_dtype={dtype}"] + _TINY)
        files = set(os.listdir(run_dir))
        assert {"config.yaml", "last.pth", "storage.csv"} <= files, files
        header = open(os.path.join(run_dir, "storage.csv")).read().splitlines()[0].split(",")
        assert any(h.startswith("tra_entropy") for h in header), header
        import yaml
        cfg = yaml.safe_load(open(os.path.join(run_dir, "config.yaml")))
        assert cfg["EntropyMinParameters"]["weight"] == 0.001
        lines = th.checkpoint_tree(os.path.join(run_dir, "last.pth"))
        mine = th.own_lines_removed(lines, ("_storage/tra_entropy", "_optimizer/loss_scaler/"))
        assert any(l.startswith("_storage/tra_entropy") for l in lines)
        assert any(l.startswith("_optimizer/loss_scaler/") for l in lines) == (dtype == "float16")
        ref = sorted(str(x) for x in golden("trainer_io")["partial/tree_last_pth"])
        assert mine == ref, (sorted(set(mine) - set(ref))[:12], sorted(set(ref) - set(mine))[:12])
        score = th.run_inference(["Trainer.name=entmin", f"Trainer.save_dir={save}_inf", f"Arch.compute_dtype={dtype}"] + _TINY,
                                os.path.join(run_dir, "last.pth"))
        assert 0.0 <= score <= 1.0, score
    finally:
        shutil.rmtree(run_dir, ignore_errors=True)
        shutil.rmtree(run_dir + "_inf", ignore_errors=True)
