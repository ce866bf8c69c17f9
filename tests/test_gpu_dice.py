"""GPU: the Dice supervised loss (``SupCriterion.name=dice|kldice``) -- the fused ``miseg_softmax_dice`` against
float64 autograd (every class count, both powers, class weights, peaked logits, less than a wave, the grid-stride path, as the labeled
part of a split batch, with a KL part), determinism, bad labels, refusals; the ``partial`` epocher against the reference's own run with
the wheel's criterion (tests/golden/dice.npz), the step under the launch tape and the CLI."""
import os
import random
import shutil
from functools import partial

import numpy as np
import pytest
import torch

import dice_ref
import synth
import trainer_harness as th
from trainer_harness import DEV, FEATURES

pytestmark = pytest.mark.gpu
T = torch.from_numpy
CLASS_COUNTS = (2, 3, 4, 5, 6, 8, 10, 16)
# The project's bounds for a pixel loss (tests/test_gpu_entmin.py): the loss within 1e-5 relative, the gradient within 1e-5 of the
# reference gradient's largest entry.  A torch fp32 evaluation of the same expression is within 6e-8 (loss) and 5e-7 (gradient) of
# float64 on these inputs, so the bounds leave the kernel more than ten times the reference's own error.  Achieved: DESIGN.md section 25.
LOSS_BOUND, GRAD_BOUND = 1e-5, 1e-5


_dump = partial(th.error_dump, "dice")          # the numbers DESIGN.md section 25 quotes


def _nhwc(t):
    return t.to(DEV).contiguous(memory_format=torch.channels_last)


def _weight(c, weighted):
    return dice_ref.class_weights(c) if weighted else None


def _run(z, lab, check_labels=True, **kw):
    """ops.softmax_dice forward + backward on a plain NHWC tensor; ``kw`` as dice_ref.reference names them."""
    from miseg_amd import ops
    weight = kw.pop("weight", None)
    cw = None if weight is None else torch.tensor(weight, dtype=torch.float32, device=DEV)
    zd = _nhwc(z).requires_grad_()
    loss = ops.softmax_dice(zd, lab.to(DEV), class_weight=cw, check_labels=check_labels, **kw)
    loss.backward()
    return float(loss.detach()), zd.grad.cpu().double()


def _errors(got, ref):
    return {"value": ref[0], "loss": abs(got[0] - ref[0]) / abs(ref[0]), "grad": dice_ref.rel(got[1], ref[1])}


# ---------------------------------------------------------------------------------------------------------------- 1. the kernel
@pytest.mark.parametrize("scale", [2, 12])
@pytest.mark.parametrize("pw", [1, 2])
@pytest.mark.parametrize("c", CLASS_COUNTS)
def test_kernel_against_float64(c, pw, scale):
    """[3, C, 33, 31]: 1023 pixels per sample -- no multiple of the block or the wave, four blocks per sample with a ragged tail --,
    sample 0 labelled entirely with class 1, class 0 absent everywhere; ``randn * 2`` and the peaked ``randn * 12``; with and without
    class weights."""
    shape = (3, c, 33, 31)
    z, lab = dice_ref.logits(shape, scale), dice_ref.labels(shape)
    assert int((lab == 0).sum()) == 0 and bool((lab[0] == 1).all())
    for weighted in (False, True):
        w = _weight(c, weighted)
        ref = dice_ref.reference(z, lab, pw, 1e-8, w)
        err = _errors(_run(z, lab, pow=pw, weight=w), ref)
        print("dice kernel", c, pw, scale, weighted, err)
        _dump(f"kernel_c{c}_p{pw}_s{scale}_w{int(weighted)}", err)
        assert err["loss"] < LOSS_BOUND and err["grad"] < GRAD_BOUND, err


@pytest.mark.parametrize("pw", [1, 2])
def test_less_than_one_wave(pw):
    """[2, 16, 5, 7]: 35 pixels per sample."""
    shape = (2, 16, 5, 7)
    z, lab = dice_ref.logits(shape, 2), dice_ref.labels(shape)
    w = _weight(16, True)
    err = _errors(_run(z, lab, pow=pw, weight=w), dice_ref.reference(z, lab, pw, 1e-8, w))
    print("dice small", pw, err)
    _dump(f"kernel_small_p{pw}", err)
    assert err["loss"] < LOSS_BOUND and err["grad"] < GRAD_BOUND, err


def test_grid_stride_path_against_float64():
    """[1, 4, 192, 192]: 36864 pixels in one sample > the cap of 128 blocks per sample x 256 threads = 32768, so the first threads of
    every block loop in both pixel passes and the finish sums 128 partials per class."""
    from miseg_amd import _cabi
    shape = (1, 4, 192, 192)
    assert _cabi.lib().miseg_softmax_dice_ws_bytes(1, 192, 192, 4) == _cabi.lib().miseg_softmax_dice_ws_bytes(1, 128, 256, 4)   # capped
    z, lab = dice_ref.logits(shape, 2), dice_ref.labels(shape)
    lab[0, 100:] = torch.randint(1, 4, (92, 192), generator=torch.Generator().manual_seed(5))      # (sample 0 is all class 1 otherwise)
    for kw in (dict(pow=2), dict(pow=1, kl_weight=0.7, dice_weight=1.3)):
        err = _errors(_run(z, lab, **kw), dice_ref.reference(z, lab, eps=1e-8, **kw))
        print("dice grid-stride", kw, err)
        _dump(f"kernel_gridstride_p{kw['pow']}", err)
        assert err["loss"] < LOSS_BOUND and err["grad"] < GRAD_BOUND, err


@pytest.mark.parametrize("c", [3, 4, 16])
def test_labeled_part_of_a_split_batch(c):
    """The trainer's arrangement: [labeled | unlabeled | flipped] = one NHWC batch through ``split_rows([2, 3, 3])``; Dice reads the
    first part and writes its rows of the batch gradient (in place where they start on a 16-byte boundary, through the split's copy
    otherwise), a fused entropy the second, the third has no loss and comes out exactly zero."""
    from miseg_amd import ops
    from miseg_amd.lazy import LinearLoss
    shape = (2, c, 33, 31)
    z, lab = dice_ref.logits(shape, 2), dice_ref.labels(shape)
    g = torch.Generator().manual_seed(c)
    mid, last = torch.randn(3, c, 33, 31, generator=g), torch.randn(3, c, 33, 31, generator=g)
    ref = dice_ref.reference(z, lab, 2, 1e-8)
    batch = _nhwc(torch.cat([z, mid, last])).requires_grad_()
    pf, pm, pl = ops.split_rows(batch, [2, 3, 3])
    sup = ops.softmax_dice(pf, lab.to(DEV), pow=2)
    ent = ops.softmax_entropy(pm)
    (LinearLoss.of(sup) + 0.5 * LinearLoss.of(ent)).backward()
    md = _nhwc(mid).requires_grad_()
    (0.5 * LinearLoss.of(ops.softmax_entropy(md))).backward()      # the entropy alone
    err = _errors((float(sup.detach()), batch.grad[:2].cpu().double()), ref)
    print("dice split", c, err)
    _dump(f"kernel_split_c{c}", err)
    assert err["loss"] < LOSS_BOUND and err["grad"] < GRAD_BOUND, err
    assert torch.equal(batch.grad[2:5], md.grad)
    assert torch.equal(batch.grad[5:], torch.zeros_like(batch.grad[5:]))
    assert batch.grad.is_contiguous(memory_format=torch.channels_last)


@pytest.mark.parametrize("pw", [1, 2])
def test_kldice_against_float64(pw):
    """0.7 KL + 1.3 GDL against float64; with kl_weight 1 and dice_weight 0 the call is ``ops.softmax_kl`` within the bounds."""
    from miseg_amd import ops
    shape = (3, 4, 33, 31)
    w = _weight(4, True)
    for scale in (2, 12):
        z, lab = dice_ref.logits(shape, scale), dice_ref.labels(shape)
        kw = dict(pow=pw, kl_weight=0.7, dice_weight=1.3, weight=w)
        err = _errors(_run(z, lab, **kw), dice_ref.reference(z, lab, eps=1e-8, **kw))
        print("kldice", pw, scale, err)
        _dump(f"kernel_kldice_p{pw}_s{scale}", err)
        assert err["loss"] < LOSS_BOUND and err["grad"] < GRAD_BOUND, err
        zk = _nhwc(z).requires_grad_()
        kl = ops.softmax_kl(zk, lab.to(DEV))
        kl.backward()
        err = _errors(_run(z, lab, pow=pw, kl_weight=1.0, dice_weight=0.0), (float(kl), zk.grad.cpu().double()))
        assert err["loss"] < LOSS_BOUND and err["grad"] < GRAD_BOUND, err


def _raw_call(z, lab, with_grad=True, upstream=None, c=None, n=None, pw=1, ws_short=0, kl_weight=0.5):
    """The C entry point on NaN-prefilled outputs; returns (status message or None, loss, grad, bad)."""
    from miseg_amd import _cabi
    zn, zc, h, w = z.shape
    n, c = zn if n is None else n, zc if c is None else c
    loss = torch.full((1,), float("nan"), device=DEV)
    grad = torch.full_like(z, float("nan")) if with_grad else None
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    need = int(_cabi.lib().miseg_softmax_dice_ws_bytes(max(n, 1), h, w, zc))
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    msg = None
    try:
        _cabi.call("miseg_softmax_dice", torch.cuda.current_stream().cuda_stream, z.data_ptr(), lab.data_ptr(), n, h, w, c, pw, 1e-8, None,
                   kl_weight, 1.0, None if upstream is None else upstream.data_ptr(), loss.data_ptr(),
                   None if grad is None else grad.data_ptr(), bad.data_ptr(), ws.data_ptr(), need - ws_short)
    except _cabi.MisegError as ex:
        msg = str(ex)
    return msg, loss, grad, bad


def test_two_calls_are_bit_identical_and_forward_only_gives_the_same_loss():
    shape = (3, 5, 65, 67)
    z, lab = _nhwc(dice_ref.logits(shape, 2)), dice_ref.labels(shape).to(DEV)
    _, l1, g1, _ = _raw_call(z, lab)
    _, l2, g2, _ = _raw_call(z, lab)
    _, l3, _, _ = _raw_call(z, lab, with_grad=False)
    torch.cuda.synchronize()
    assert torch.equal(l1, l2) and torch.equal(g1, g2) and torch.equal(l1, l3)
    assert torch.isfinite(l1).all() and torch.isfinite(g1).all()


def test_upstream_scales_the_gradient_only():
    shape = (3, 3, 33, 31)
    z, lab = _nhwc(dice_ref.logits(shape, 2)), dice_ref.labels(shape).to(DEV)
    _, l1, g1, _ = _raw_call(z, lab)
    _, l2, g2, _ = _raw_call(z, lab, upstream=torch.tensor([0.25], device=DEV))
    assert torch.equal(l1, l2)
    torch.testing.assert_close(g2, g1 * 0.25, rtol=2e-7, atol=0)


@pytest.mark.parametrize("pw", [1, 2])
def test_bad_labels_are_flagged_and_left_out(pw):
    """C and -1 at five pixels of sample 1: the flag is set, loss and gradient are the float64 reference with those pixels' p and t
    zeroed, their gradient rows exactly 0; with ``check_labels`` the call raises outside a deferred block."""
    from miseg_amd import ops
    shape = (3, 4, 33, 31)
    z, lab = dice_ref.logits(shape, 2), dice_ref.labels(shape).clone()
    where = [(1, 0, 0), (1, 7, 30), (1, 16, 16), (1, 32, 1), (1, 32, 30)]
    for i, (n, h, w) in enumerate(where):
        lab[n, h, w] = 4 if i % 2 == 0 else -1
    bad = (lab < 0) | (lab >= 4)
    assert int(bad.sum()) == 5
    kw = dict(pow=pw, kl_weight=0.7, dice_weight=1.3)
    ref = dice_ref.reference(z, lab, eps=1e-8, bad=bad, **kw)
    got = _run(z, lab, check_labels=False, **kw)
    err = _errors(got, ref)
    print("dice bad labels", pw, err)
    _dump(f"kernel_badlabel_p{pw}", err)
    assert err["loss"] < LOSS_BOUND and err["grad"] < GRAD_BOUND, err
    for n, h, w in where:
        assert float(got[1][n, :, h, w].abs().max()) == 0.0
    _, _, _, flag = _raw_call(_nhwc(z), lab.to(DEV))
    assert int(flag) != 0
    _, _, _, flag = _raw_call(_nhwc(z), dice_ref.labels(shape).to(DEV))
    assert int(flag) == 0
    with pytest.raises(AssertionError, match="softmax_dice: a label lies outside"):
        ops.softmax_dice(_nhwc(z), lab.to(DEV), check_labels=True)


def test_refusals_launch_nothing():
    """C = 7, pow = 3, N = 0 and a workspace one byte short: MISEG_E_INVALID each, the NaN-prefilled outputs untouched."""
    from miseg_amd import _cabi, ops
    assert not ops.softmax_dice_supported(7)
    z7 = _nhwc(torch.randn(1, 7, 8, 8))
    lab = torch.ones(1, 8, 8, dtype=torch.long, device=DEV)
    with pytest.raises(_cabi.MisegError, match="unsupported class count"):
        ops.softmax_dice(z7, lab)
    z4 = _nhwc(torch.randn(1, 4, 8, 8))
    for what, (z, kw) in {"c7": (z7, {}), "pow3": (z4, dict(pw=3)), "n0": (z4, dict(n=0)), "ws": (z4, dict(ws_short=1))}.items():
        msg, loss, grad, flag = _raw_call(z, lab, **kw)
        torch.cuda.synchronize()
        assert msg is not None and "(-1)" in msg, (what, msg)
        assert bool(torch.isnan(loss).all()) and bool(torch.isnan(grad).all()) and int(flag) == 0, what
    msg, loss, grad, _ = _raw_call(z4, lab)
    assert msg is None and bool(torch.isfinite(loss).all()) and bool(torch.isfinite(grad).all())


def test_no_grad_is_forward_only_and_criteria_take_the_fused_path():
    """Under ``torch.no_grad()`` (evaluation) no gradient buffer is made; ``supervised_loss`` routes both criteria to the entry point
    (same bits as the direct call) and uploads the class weights once per criterion object."""
    from deepclustering2.loss import GeneralizedDiceLoss
    from miseg_amd import ops
    from semi_seg._utils import KLDiceLoss
    from semi_seg.epocher import supervised_loss
    shape = (3, 4, 33, 31)
    z, lab = _nhwc(dice_ref.logits(shape, 2)), dice_ref.labels(shape).to(DEV)
    w = _weight(4, True)
    crit = GeneralizedDiceLoss(pow=2, weight=w)
    cw = torch.tensor(w, device=DEV)
    with torch.no_grad():
        got = supervised_loss(crit, z, lab, 4, disable_assert=True)
        assert not got.requires_grad and torch.equal(got, ops.softmax_dice(z, lab, pow=2, class_weight=cw))
    zr = z.clone().requires_grad_()
    assert torch.equal(supervised_loss(crit, zr, lab, 4), got)
    assert crit.class_weight_on(z.device) is crit.class_weight_on(z.device)
    kd = KLDiceLoss(0.7, 1.3, GeneralizedDiceLoss(pow=2, weight=w))
    assert torch.equal(supervised_loss(kd, zr, lab, 4), ops.softmax_dice(z, lab, pow=2, class_weight=cw, kl_weight=0.7, dice_weight=1.3))
    # a criterion without a kernel keeps the materialised call
    z7 = torch.randn(1, 7, 8, 8, device=DEV, requires_grad=True)
    lab7 = torch.randint(0, 7, (1, 8, 8), device=DEV)
    ref7 = dice_ref.reference(z7.detach().cpu(), lab7.cpu())[0]
    assert abs(float(supervised_loss(GeneralizedDiceLoss(), z7, lab7, 7).detach()) - ref7) < LOSS_BOUND * ref7


# ---------------------------------------------------------------------------------------------------------------- 2. the epocher
def _golden_run(g, monkeypatch):
    from deepclustering2.optim import Adam
    from semi_seg import epocher as E
    from semi_seg._utils import build_sup_criterion
    cfg = th.golden_cfg(g)
    H, LB, UB, NB = int(cfg["H"]), int(cfg["LB"]), int(cfg["UB"]), int(cfg["NB"])
    model = th.unet("float32", int(cfg["model_seed"]))
    opt = Adam(model.parameters(), lr=float(cfg["lr"]), weight_decay=float(cfg["wd"]))
    lab = [(T(synth.uniform(f"dice/lab{i}", (LB, 1, H, H))), T(synth.integers(f"dice/tgt{i}", (LB, 1, H, H), 4))) for i in range(NB)]
    unl = [T(synth.uniform(f"dice/unl{i}", (UB, 1, H, H))) for i in range(NB)]
    th.replay_seeds(monkeypatch, g["seeds"])
    with th.adam_gradients(monkeypatch) as grads:
        crit = build_sup_criterion({"SupCriterion": {"name": "dice"}}, 4)
        ep = E.TrainEpocher(model, opt, th.reference_batches([a for a, _ in lab], [b for _, b in lab], LB),
                            th.reference_batches(unl, [torch.zeros(UB, 1, H, H, dtype=torch.long)] * NB, UB), crit, 0.0, NB, 0, DEV,
                            feature_position=FEATURES, feature_importance=th.IMPORTANCE)
        ep._TAPE_DEFAULT = False
        per_step = th.keep_records(ep)
        res = ep.run()
    return res, grads[0].cpu(), per_step, opt


def test_partial_epocher_with_dice_matches_the_reference_run(golden, monkeypatch):
    """fp32, tape off, 3 `partial` iterations against the reference's TrainEpocher given the wheel's GeneralizedDiceLoss
    (tests/golden/dice.npz): step-1 gradients at the first-iteration bounds of test_gpu_step, per-step sup_loss, the meter key set, the
    decoder tail after the last step."""
    g = golden("dice")
    res, grad, per_step, opt = _golden_run(g, monkeypatch)
    named = dict(zip((str(n) for n in g["param_names"]), opt.flat.given))
    assert len(named) == len(opt.flat.given)
    worst = th.sampled_rel_l2(g, "grad_step1", grad, named, opt.flat.offset_of)
    tail = sorted(v for k, v in worst.items() if k.startswith(("Up_conv2", "DeConv")))
    print("dice golden gradients: logits layer", max(v for k, v in worst.items() if k.startswith("DeConv")), "tail", tail[0],
          tail[len(tail) // 2], tail[-1], "all", max(worst.values()))
    _dump("golden_grad", worst)
    # the first-iteration bounds of test_gpu_step::test_step_gradients_match_reference, as test_gpu_entmin takes them over.  The
    # fixture's own fp32 error against a float64 run of the reference is stored in it (own_error/*; make_golden_dice.py)
    assert max(v for k, v in worst.items() if k.startswith("DeConv")) < 2e-5, worst
    assert tail[len(tail) // 2] < 5e-3 and tail[0] < 1e-5 and tail[-1] < 1.5e-2, tail
    assert max(worst.values()) < 3e-2, worst
    assert len(per_step) == 3
    print("dice golden steps:", per_step, list(g["sup_loss"]))
    np.testing.assert_allclose(per_step[0]["sup_loss"], g["sup_loss"][0], rtol=2e-5)
    np.testing.assert_allclose([s["sup_loss"] for s in per_step], g["sup_loss"], rtol=3e-3)
    last = {n: q for n, q in named.items() if n.startswith(("Up_conv2", "DeConv_1x1"))}
    for n, d in th.sampled_max_abs(g, "param_after", opt.flat.flat_param, last, opt.flat.offset_of).items():
        assert d <= 7.5e-3, (n, d)
    keys = [str(k) for k in g["meter_keys"]]
    got = th.meter_items(res)
    assert sorted(got) == sorted(keys), (sorted(got), sorted(keys))
    ref = dict(zip(keys, (float(v) for v in g["meter_values"])))
    np.testing.assert_allclose(got["sup_loss/mean"], ref["sup_loss/mean"], rtol=3e-3)


def test_without_the_section_the_first_step_is_the_softmax_kl_call(monkeypatch):
    """No ``SupCriterion`` section: the criterion is the plain KL_div and the step's ``sup_loss`` has the bits of ``ops.softmax_kl`` on
    the same logits (the parent commit's path)."""
    from deepclustering2.loss import KL_div
    from deepclustering2.optim import Adam
    from miseg_amd import ops
    from semi_seg import epocher as E
    from semi_seg._utils import build_sup_criterion
    from semi_seg.synthetic import SyntheticPairs
    crit = build_sup_criterion({}, 4)
    assert type(crit) is KL_div
    model = th.unet("float32", 41)
    opt = Adam(model.parameters(), lr=1e-3, weight_decay=1e-5)
    ep = E.TrainEpocher(model, opt, iter(SyntheticPairs(2, 64, 4, seed=0, device=DEV)), iter(SyntheticPairs(2, 64, 4, seed=1, device=DEV)),
                        crit, 0.0, 1, 0, DEV, feature_position=FEATURES, feature_importance=th.IMPORTANCE)
    ep._TAPE_DEFAULT = False
    seen, per_step = [], th.keep_records(ep)
    real = E.supervised_loss

    def spy(criterion, logits, labels, *a, **k):
        seen.append((criterion, logits.detach().clone(), labels.clone()))
        return real(criterion, logits, labels, *a, **k)

    monkeypatch.setattr(E, "supervised_loss", spy)
    random.seed(3)
    ep.run()
    assert len(seen) == 1 and seen[0][0] is crit and len(per_step) == 1
    direct = ops.softmax_kl(seen[0][1], seen[0][2])
    assert per_step[0]["sup_loss"] == float(direct), (per_step[0]["sup_loss"], float(direct))


# ---------------------------------------------------------------------------------------------------------------- 3. the tape
def build(name, dtype="float32", num_batches=7, **section):
    from deepclustering2.optim import Adam
    from semi_seg._utils import build_sup_criterion
    from semi_seg.epocher import TrainEpocher
    from semi_seg.synthetic import SyntheticPairs
    model = th.unet(dtype, 41)
    opt = Adam(model.parameters(), lr=1e-3, weight_decay=1e-5)
    lab = SyntheticPairs(2, 64, 4, seed=0, device=DEV)
    unl = SyntheticPairs(2, 64, 4, seed=1, device=DEV)
    crit = build_sup_criterion({"SupCriterion": {"name": name, **section}}, 4)
    ep = TrainEpocher(model, opt, iter(lab), iter(unl), crit, 0.0, num_batches, 0, DEV, feature_position=FEATURES,
                      feature_importance=th.IMPORTANCE)
    return ep, model, opt


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("name", ["dice", "kldice"])
def test_tape_replay_equals_eager_steps(name, dtype):
    """2 eager + 1 recorded + 4 replayed iterations give the parameters, Adam's moments and the meters of 7 eager ones, bit for bit.
    The recorded iteration has no ATen launch (the tape would have been refused), one launch of the new entry point and no softmax-KL."""
    section = dict(kl_weight=0.7, dice_weight=1.3, pow=2) if name == "kldice" else {}
    got, info = th.run_steps(lambda: build(name, dtype, **section), 7, True)
    ref, _ = th.run_steps(lambda: build(name, dtype, **section), 7, False)
    th.assert_replayed(info, 4)
    names = info.op_names
    assert names.count("miseg_softmax_dice") == 1 and names.count("miseg_softmax_kl") == 0, names
    th.assert_same_state(got, ref, ("param", "m", "v", "meters"))


def test_changed_dice_weight_rerecords_the_tape():
    ep, _, _ = build("kldice", dice_weight=1.0)
    sig = ep._tape_signature()
    assert ep._tape_signature() == sig
    ep._sup_criterion.dice_weight = 2.0
    assert ep._tape_signature() != sig


# ---------------------------------------------------------------------------------------------------------------- 4. the CLI
@pytest.mark.parametrize("trainer,name,epochs,dtype", [("udaiic", "kldice", 2, "bfloat16"), ("meanteacher", "dice", 1, "float16")])
def test_main_cli_runs_with_the_section(trainer, name, epochs, dtype):
    """``python semi_seg/main.py Trainer.name=<trainer> SupCriterion.name=<name>`` on synthetic data (bf16 storage, and fp16 with its
    loss scale): trains, validates with a finite loss, writes the section into config.yaml and the criterion's (small) subtree into
    the checkpoint."""
    save = f"pytest_cli_dice_{trainer}_{os.getpid()}"
    run_dir = th.run_dir(save)
    shutil.rmtree(run_dir, ignore_errors=True)
    try:
        th.run_main([f"Trainer.save_dir={save}", "Trainer.device=cuda", f"Trainer.max_epoch={epochs}", "Trainer.num_batches=3",
                     "Data.name=synthetic", "Data.size=64", "LabeledData.batch_size=2", "UnlabeledData.batch_size=2",
                     f"Trainer.name={trainer}", f"SupCriterion.name={name}", "SupCriterion.pow=2", f"Arch.compute_dtype={dtype}"])
        files = set(os.listdir(run_dir))
        assert {"config.yaml", "last.pth", "storage.csv"} <= files, files
        import yaml
        cfg = yaml.safe_load(open(os.path.join(run_dir, "config.yaml")))
        assert cfg["SupCriterion"] == {"name": name, "pow": 2}
        rows = open(os.path.join(run_dir, "storage.csv")).read().splitlines()
        header = rows[0].split(",")
        assert len(rows) == 1 + epochs
        cols = [i for i, h in enumerate(header) if h.startswith(("tra_sup_loss", "val_loss"))]
        assert any(header[i].startswith("tra_sup_loss") for i in cols) and any(header[i].startswith("val_loss") for i in cols), header
        for col in cols:
            assert all(np.isfinite(float(r.split(",")[col])) for r in rows[1:]), (header[col], rows)
        ck = torch.load(os.path.join(run_dir, "last.pth"), map_location="cpu", weights_only=False)
        assert ck["_sup_criterion"] == ({"kl_weight": 1.0, "dice_weight": 1.0} if name == "kldice" else {})
    finally:
        shutil.rmtree(run_dir, ignore_errors=True)
