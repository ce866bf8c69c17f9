"""GPU: contrastive encoder pre-training (``Trainer.name=contrast``) -- the fused SupCon kernel against float64
autograd of its closed form, determinism, refusals and the composed fallback, the NHWC average pool in every storage type, the
projection head against float64 autograd, the epocher against the reference's own run (tests/golden/contrast.npz), a bf16 step and the
CLI including fine-tuning from ``Pretrained=``."""
import os
import shutil
from functools import partial

import numpy as np
import pytest
import torch

import synth
import trainer_harness as th
from contrast_ref import closed_form, embeddings, golden_projector_state, golden_views, group_of
from oracle import unet as OU
from trainer_harness import DEV

pytestmark = pytest.mark.gpu


_dump = partial(th.error_dump, "contrast")          # the numbers DESIGN.md section 14 quotes


def _rel(got, ref):
    return float((got - ref).abs().max() / ref.abs().max())


# ---------------------------------------------------------------------------------------------------------------- 1. the kernel
# Bounds: 1e-5 relative for the loss and 1e-5 of the largest reference entry for the gradients -- the bounds of the other loss kernels.
# A torch fp32 evaluation of the same expression on the CPU is <= 8.7e-8 (loss) / <= 1.5e-6 (gradients, at B = 256; <= 1.2e-6 below) from
# float64 on these inputs, so the bounds leave the kernel about ten times the reference's own error.  The test prints that fp32 error next
# to the kernel's (measured: loss <= 1.7e-7, gradients <= 3.0e-6).
LOSS_BOUND, GRAD_BOUND = 1e-5, 1e-5
# (B, D, scale, classes): labels = sample index mod classes
LABELLED = [(2, 256, 1, 1), (3, 256, 1, 2), (5, 64, 1, 3), (16, 256, 1, 3), (16, 256, 30, 6), (37, 256, 1, 5), (256, 128, 1, 7)]


def _fp32_reference_error(e, labels, views, T, ref_loss, ref_grad):
    """The torch composition (the reference's arithmetic) in fp32 on the CPU against float64."""
    from contrastyou.losses.contrast_loss import SupConLoss
    x = e.clone().requires_grad_()
    loss = SupConLoss(temperature=T, base_temperature=T).from_embeddings(x, labels, views=views)
    loss.backward()
    return {"loss": abs(float(loss.detach()) - ref_loss) / abs(ref_loss), "grad": _rel(x.grad.double(), ref_grad)}


def _kernel_case(tag, e, labels, views, T=0.07):
    from miseg_amd import ops
    ref_loss, ref_grad = closed_form(e, labels, views, T, T)
    ed = e.to(DEV).requires_grad_()
    lab = None if labels is None else torch.tensor(labels, dtype=torch.int32, device=DEV)
    loss = ops.supcon(ed, lab, views, T, T)
    loss.backward()
    err = {"value": ref_loss, "loss": abs(float(loss.detach()) - ref_loss) / abs(ref_loss), "grad": _rel(ed.grad.cpu().double(), ref_grad),
           "torch_fp32": _fp32_reference_error(e, labels, views, T, ref_loss, ref_grad)}
    print("supcon", tag, err)
    _dump(f"kernel_{tag}", err)
    assert err["loss"] < LOSS_BOUND and err["grad"] < GRAD_BOUND, err


@pytest.mark.parametrize("b,d,scale,classes", LABELLED)
def test_kernel_against_float64_labelled(b, d, scale, classes):
    e = embeddings(b, d, 2, seed=1000 * b + d + classes, scale=float(scale))
    _kernel_case(f"b{b}_d{d}_s{scale}_c{classes}", e, [i % classes for i in range(b)], 2)


def test_kernel_against_float64_simclr():
    """``labels=None``: the only positive of an anchor is its other view.  Run at SimCLR's own temperature 0.5: at 0.07 that positive
    (cosine ~0.96) dominates the denominator, the loss is log(1 + ~1e-5), and fp32 -- the reference's evaluation included -- resolves
    such a value to ~1e-3 relative only; at 0.5 the loss is O(1) and the 1e-5 bound means what it means for the labelled cases."""
    _kernel_case("simclr_b16_d256", embeddings(16, 256, 2, seed=7), None, 2, T=0.5)


def test_kernel_against_float64_three_views():
    _kernel_case("v3_b5_d64", embeddings(5, 64, 3, seed=11), [0, 1, 2, 0, 1], 3)


def _raw_call(e, labels, views, with_grad=True, upstream=None, T=0.07, fill=float("nan"), n=None, d=None):
    from miseg_amd import _cabi
    n, d = (e.shape[0] if n is None else n), (e.shape[1] if d is None else d)
    loss = torch.full((1,), fill, device=DEV)
    grad = torch.full_like(e, fill) if with_grad else None
    nbytes = int(_cabi.lib().miseg_supcon_ws_bytes(n, d))
    ws = torch.zeros(max(nbytes, 1 << 16), dtype=torch.uint8, device=DEV)
    _cabi.call("miseg_supcon", torch.cuda.current_stream().cuda_stream, e.data_ptr(), n, d, views, None if labels is None else labels.data_ptr(),
               T, T, None if upstream is None else upstream.data_ptr(), loss.data_ptr(), None if grad is None else grad.data_ptr(),
               ws.data_ptr(), ws.numel())
    return loss, grad, ws


def test_upstream_scales_the_gradient_only():
    e = embeddings(16, 256, 2, seed=3).to(DEV)
    labels = torch.tensor([i % 3 for i in range(16)], dtype=torch.int32, device=DEV)
    ref_loss, ref_grad = closed_form(e.cpu(), labels.cpu().tolist(), 2)
    l1, g1, _ = _raw_call(e, labels, 2)
    l2, g2, _ = _raw_call(e, labels, 2, upstream=torch.tensor([0.25], device=DEV))
    assert torch.equal(l1, l2)
    err = {"loss": abs(float(l2) - ref_loss) / abs(ref_loss), "grad": _rel(g2.cpu().double(), 0.25 * ref_grad)}
    print("supcon upstream 0.25", err)
    _dump("kernel_upstream", err)
    assert err["loss"] < LOSS_BOUND and err["grad"] < GRAD_BOUND, err
    assert torch.equal(g2, g1 * 0.25)          # a power of two: the same bits, scaled


# ---------------------------------------------------------------------------------------------------------------- 2. determinism
@pytest.mark.parametrize("b,d", [(16, 256), (256, 128)])
def test_two_calls_are_bit_identical_and_forward_only_gives_the_same_loss(b, d):
    e = embeddings(b, d, 2, seed=5).to(DEV)
    labels = torch.tensor([i % 5 for i in range(b)], dtype=torch.int32, device=DEV)
    l1, g1, _ = _raw_call(e, labels, 2)
    l2, g2, _ = _raw_call(e, labels, 2)
    l3, _, _ = _raw_call(e, labels, 2, with_grad=False)
    torch.cuda.synchronize()
    assert torch.equal(l1, l2) and torch.equal(g1, g2) and torch.equal(l1, l3)
    assert torch.isfinite(l1).all() and torch.isfinite(g1).all()


# ---------------------------------------------------------------------------------------------------------------- 3. refusals
def test_refusals_launch_nothing_and_the_module_composes_instead():
    """V = 1, N not divisible by V, an unsupported D, an empty batch: MISEG_E_INVALID, the sentinel-filled outputs and the workspace are
    untouched.  ``SupConLoss`` on such a shape runs the torch composition, which meets the kernel's bounds."""
    from contrastyou.losses.contrast_loss import SupConLoss
    from miseg_amd import _cabi, ops
    e = embeddings(4, 64, 2, seed=1).to(DEV)                       # a valid [8, 64] buffer behind every refused call
    labels = torch.zeros(8, dtype=torch.int32, device=DEV)
    for views, n, d in ((1, 8, 64), (3, 8, 64), (2, 8, 66), (2, 8, 2048), (2, 0, 64), (2, 1026, 64)):
        assert not ops.supcon_supported(n, d, views)
        with pytest.raises(_cabi.MisegError):
            loss, grad, ws = _raw_call(e, labels, views, fill=3.0, n=n, d=d)
    # the call that raised returned nothing: repeat with the buffers in hand
    loss, grad = torch.full((1,), 3.0, device=DEV), torch.full_like(e, 3.0)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    for views, n, d in ((1, 8, 64), (3, 8, 64), (2, 8, 66), (2, 0, 64)):
        with pytest.raises(_cabi.MisegError):
            _cabi.call("miseg_supcon", stream, e.data_ptr(), n, d, views, labels.data_ptr(), 0.07, 0.07, None, loss.data_ptr(), grad.data_ptr(),
                       ws.data_ptr(), ws.numel())
    with pytest.raises(_cabi.MisegError):                          # a workspace smaller than miseg_supcon_ws_bytes
        _cabi.call("miseg_supcon", stream, e.data_ptr(), 8, 64, 2, labels.data_ptr(), 0.07, 0.07, None, loss.data_ptr(), grad.data_ptr(),
                   ws.data_ptr(), 64)
    torch.cuda.synchronize()
    assert float(loss) == 3.0 and bool((grad == 3.0).all()) and not bool(ws.any())
    with pytest.raises(_cabi.MisegError):
        ops.supcon(embeddings(4, 66, 2, seed=2).to(DEV), None, 2)
    # the module: D = 66 has no kernel -> composition, on the GPU, at the kernel's bounds
    x = embeddings(6, 66, 2, seed=2)
    lab = [0, 1, 2, 0, 1, 2]
    ref_loss, ref_grad = closed_form(x, lab, 2)
    xd = x.to(DEV).requires_grad_()
    loss = SupConLoss().from_embeddings(xd, lab)
    assert loss.grad_fn is not None and "SupCon" not in type(loss.grad_fn).__name__
    loss.backward()
    err = {"loss": abs(float(loss.detach()) - ref_loss) / abs(ref_loss), "grad": _rel(xd.grad.cpu().double(), ref_grad)}
    print("supcon composed fallback", err)
    _dump("fallback", err)
    assert err["loss"] < LOSS_BOUND and err["grad"] < GRAD_BOUND, err


def test_module_forward_on_unit_rows_runs_the_kernel():
    """``forward(features [B, V, D], labels)`` on unit-norm rows: the fused node, within the kernel's bounds of the closed form (the
    renormalisation of unit rows moves them by rounding only)."""
    from contrastyou.losses.contrast_loss import SupConLoss
    x = embeddings(16, 256, 2, seed=9)
    lab = [i % 3 for i in range(16)]
    ref_loss, _ = closed_form(x, lab, 2)
    unit = torch.nn.functional.normalize(x, dim=1).to(DEV)
    loss = SupConLoss()(torch.stack(torch.chunk(unit, 2, 0), 1).requires_grad_(), labels=lab)
    assert "SupCon" in type(loss.grad_fn).__name__
    assert abs(float(loss.detach()) - ref_loss) / abs(ref_loss) < LOSS_BOUND


# ---------------------------------------------------------------------------------------------------------------- 4. the pool
_STORAGE = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16}


def _ulp_distance(a, b):
    """Distance in units in the last place between two tensors of one floating type (same-sign finite values)."""
    it = torch.int32 if a.dtype == torch.float32 else torch.int16
    return (a.contiguous().view(it).to(torch.int64) - b.contiguous().view(it).to(torch.int64)).abs()


@pytest.mark.parametrize("dtype", list(_STORAGE))
@pytest.mark.parametrize("n,c,h,w", [(8, 256, 4, 4), (6, 256, 3, 5), (4, 128, 16, 16)])
def test_avgpool_forward_and_backward(n, c, h, w, dtype):
    from miseg_amd import ops
    dt = _STORAGE[dtype]
    g = torch.Generator().manual_seed(n * 1000 + h * 10 + w)
    feat = torch.randn(n, c, h, w, generator=g).to(dt)                      # the STORED values are the input of both sides
    ref = feat.double().mean(dim=(2, 3))
    torch_err = _rel(torch.nn.functional.adaptive_avg_pool2d(feat.float(), 1).flatten(1).double(), ref)
    fd = feat.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_()
    pooled = ops.avgpool_nhwc(fd)
    assert pooled.dtype == torch.float32 and tuple(pooled.shape) == (n, c)
    err = _rel(pooled.detach().cpu().double(), ref)
    gout = torch.randn(n, c, generator=g)
    pooled.backward(gout.to(DEV))
    grad = fd.grad
    assert grad.dtype == dt and grad.is_contiguous(memory_format=torch.channels_last) and tuple(grad.shape) == (n, c, h, w)
    want = (gout / float(h * w)).to(dt)                                        # fp32 division, one rounding to the storage type
    ulps = _ulp_distance(grad.cpu(), want.view(n, c, 1, 1).expand(n, c, h, w))
    row = {"torch_fp32_err": torch_err, "err": err, "bwd_max_ulp": int(ulps.max())}
    print("avgpool", (n, c, h, w), dtype, row)
    _dump(f"pool_{n}x{c}x{h}x{w}_{dtype}", row)
    # forward: 10 x the error of torch's own fp32 adaptive_avg_pool2d on the CPU on these inputs, both against the float64 mean
    assert err <= 10 * torch_err, row
    # backward: bit-exact where H * W is a power of two (the division is exact), within one unit in the last place otherwise
    assert int(ulps.max()) <= (0 if (h * w) & (h * w - 1) == 0 else 1), row
    assert torch.equal(grad[:, :, 0, 0].unsqueeze(-1).unsqueeze(-1).expand_as(grad), grad)      # one value per (sample, channel)


def test_avgpool_refuses_bad_shapes():
    from miseg_amd import _cabi
    stream = torch.cuda.current_stream().cuda_stream
    feat = torch.zeros(2 * 4 * 4 * 8, device=DEV)
    out = torch.full((2 * 8,), 3.0, device=DEV)
    for n, h, w, c, dt in ((2, 4, 4, 6, 0), (0, 4, 4, 8, 0), (2, 0, 4, 8, 0), (2, 4, 4, 8, 7)):
        with pytest.raises(_cabi.MisegError):
            _cabi.call("miseg_avgpool_fwd", stream, dt, feat.data_ptr(), n, h, w, c, out.data_ptr())
        with pytest.raises(_cabi.MisegError):
            _cabi.call("miseg_avgpool_bwd", stream, dt, out.data_ptr(), n, h, w, c, feat.data_ptr())
    torch.cuda.synchronize()
    assert bool((out == 3.0).all()) and not bool(feat.any())


# ---------------------------------------------------------------------------------------------------------------- 5. the head
HEAD_BOUND = 1e-5      # output and parameter gradients, relative to the largest entry


@pytest.mark.parametrize("head_type", ["mlp", "linear"])
def test_projection_head_against_float64_autograd(head_type):
    """An NHWC feature [8, 256, 4, 4] through ``ProjectionHead`` against float64 autograd of the reference's Sequential (average pool,
    Flatten, Linear [, LeakyReLU(0.01), Linear]) on the CPU with the same parameters."""
    from contrastyou.trainer._utils import ProjectionHead
    torch.manual_seed(0)
    head = ProjectionHead(256, 128, head_type=head_type)
    tail = [torch.nn.Linear(256, 256), torch.nn.LeakyReLU(0.01), torch.nn.Linear(256, 128)] if head_type == "mlp" else [torch.nn.Linear(256, 128)]
    ref = torch.nn.Sequential(torch.nn.AdaptiveAvgPool2d((1, 1)), torch.nn.Flatten(), *tail)
    ref.load_state_dict({k.replace("_header.", ""): v for k, v in head.state_dict().items()})
    ref = ref.double()
    g = torch.Generator().manual_seed(1)
    feat, probe = torch.randn(8, 256, 4, 4, generator=g), torch.randn(8, 128, generator=g)
    f64 = feat.double().requires_grad_()
    out64 = ref(f64)
    (out64 * probe.double()).sum().backward()
    head = head.to(DEV)
    fd = feat.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_()
    out = head(fd)
    (out * probe.to(DEV)).sum().backward()
    err = {"out": _rel(out.detach().cpu().double(), out64.detach()), "feature_grad": _rel(fd.grad.cpu().double(), f64.grad)}
    for (k, p), (_, q) in zip(head.named_parameters(), ref.named_parameters()):
        err[k] = _rel(p.grad.cpu().double(), q.grad)
    print("projection head", head_type, err)
    _dump(f"head_{head_type}", err)
    assert max(err.values()) < HEAD_BOUND, err


# ---------------------------------------------------------------------------------------------------------------- 6. the epocher
_RUNS = {}


def _golden_run(g, dtype="float32"):
    """The fixture's three iterations through ``PretrainEncoderEpocher``; computed once per dtype and shared (as plain data)."""
    if dtype in _RUNS:
        return _RUNS[dtype]
    from itertools import chain
    from contrastyou.arch import UNet
    from contrastyou.losses.contrast_loss import SupConLoss
    from contrastyou.trainer._utils import ProjectionHead
    from deepclustering2.optim import Adam
    from miseg_amd import unet_ops
    from semi_seg.epocher import PretrainEncoderEpocher
    cfg = {k[4:]: g[k].item() for k in g.files if k.startswith("cfg/")}
    H, B, NB = int(cfg["H"]), int(cfg["B"]), int(cfg["NB"])
    model = UNet(1, 4, compute_dtype=dtype)
    model.load_state_dict(OU.init_state(1, 4, seed=int(cfg["model_seed"])))
    projector = ProjectionHead(256, int(cfg["output_dim"]), head_type="mlp")
    projector.load_state_dict(golden_projector_state(int(cfg["output_dim"])))
    model, projector = model.to(DEV), projector.to(DEV)
    model.disable_grad_all()
    model.enable_grad("Conv1", "Conv5")
    initial = {k: v.detach().clone() for k, v in model.state_dict().items()}
    named = [(f"{blk}.{n}", p) for blk in model._range("Conv1", "Conv5") for n, p in getattr(model, blk).named_parameters()]
    named += list(projector.named_parameters())
    opt = Adam((p for _, p in named), lr=float(cfg["lr"]), weight_decay=float(cfg["wd"]))
    partitions, patients = [str(p) for p in g["partitions"]], [str(p) for p in g["patients"]]

    def loader():
        tgt = torch.zeros(B, 1, H, H, dtype=torch.long)
        for i in range(NB):
            a, b = golden_views(i, B, H)
            yield [[[a, tgt], [b, tgt.clone()]], [f"{p}_{j}" for j, p in enumerate(patients)], list(partitions), list(patients)]

    crit = SupConLoss()
    losses, labels_seen, fused = [], [], []
    inner = crit.from_embeddings

    def spy(e, labels=None, views=2):
        v = inner(e, labels, views)
        losses.append(float(v.detach()))
        labels_seen.append(list(labels))
        fused.append(type(v.grad_fn).__name__)
        return v

    crit.from_embeddings = spy
    grads, real_adam = [], unet_ops.adam_step

    def adam_spy(param, grad, *a, **k):
        grads.append(grad.detach().clone())
        return real_adam(param, grad, *a, **k)

    unet_ops.adam_step = adam_spy
    try:
        res = PretrainEncoderEpocher(model, projector, opt, loader(), crit, NB, 0, DEV, "partition", "Conv5").run()
    finally:
        unet_ops.adam_step = real_adam
        crit.from_embeddings = inner

    def sampled(flat, name, param, tag):
        return th.sampled(flat, opt.flat.offset_of(param), param.numel(), f"{tag}/{name}")

    now = model.state_dict()
    # plain data only: a model kept alive here would stay registered with the weight-pack cache for the rest of the session
    out = dict(res={k: dict(v) for k, v in res.items()}, losses=losses, labels=labels_seen, fused=fused, names=[n for n, _ in named],
               grad_step1={n: sampled(grads[0], n, p, "grad_step1") for n, p in named},
               grads_finite=[bool(torch.isfinite(x).all()) for x in grads],
               param_after={n: sampled(opt.flat.flat_param, n, p, "param_after") for n, p in named if n.startswith("Conv")},
               decoder_changed=[k for k, v in now.items() if not k.startswith("Conv") and not torch.equal(v, initial[k])],
               encoder_unmoved=[n for n, p in model.named_parameters() if n.startswith("Conv") and torch.equal(p.detach(), initial[n])],
               decoder_keys=sum(1 for k in now if not k.startswith("Conv")))
    _RUNS[dtype] = out
    del res, model, projector, opt, named, grads, now, initial, crit, inner, spy
    import gc
    gc.collect()
    return out


def test_epocher_matches_the_reference_run(golden):
    """fp32, 3 iterations against the reference's PretrainEncoderEpoch / ProjectionHead / SupConLoss (tests/golden/contrast.npz)."""
    g = golden("contrast")
    run = _golden_run(g)
    assert run["labels"] == [[int(v) for v in g["labels"]]] * 3
    assert all("SupCon" in f for f in run["fused"]), run["fused"]
    print("contrast golden losses:", run["losses"], list(g["loss"]))
    np.testing.assert_allclose(run["losses"], g["loss"], rtol=1e-3)
    assert abs(run["res"]["contrastive_loss"]["mean"] - float(np.mean(g["loss"]))) <= 1e-3 * float(np.mean(g["loss"]))
    assert sorted(run["res"]) == ["contrastive_loss", "lr"]
    # step-1 gradients, relative L2 per parameter group on the fingerprint samples: <= 4 x the fixture's own fp32 error against a float64
    # run of the reference, floored at 2e-5 (test_gpu_step's bound for the layer next to the loss), capped at 3e-2 (its any-tensor bound)
    assert run["names"] == [str(n) for n in g["param_names"]]
    num, den = {}, {}
    for n in run["names"]:
        got = run["grad_step1"][n]
        ref = synth.fp_unpack(g, f"grad_step1/{n}")["sample"].astype(np.float64)
        k = group_of(n)
        num[k] = num.get(k, 0.0) + float(((got - ref) ** 2).sum())
        den[k] = den.get(k, 0.0) + float((ref ** 2).sum())
    dist = {k: (num[k] / den[k]) ** 0.5 for k in num}
    bound = {k: min(max(4.0 * float(g[f"own_error/{k}"]), 2e-5), 3e-2) for k in dist}
    print("contrast golden gradients:", dist, "bounds", bound, "own error", {k: float(g[f"own_error/{k}"]) for k in dist})
    _dump("golden_grad", {"distance": dist, "bound": bound})
    assert sorted(dist) == ["Conv1-4", "Conv5", "projector"]
    assert all(dist[k] <= bound[k] for k in dist), (dist, bound)
    # after the three steps: the decoder (parameters and BatchNorm buffers) bit for bit where it started, every encoder parameter moved
    assert run["decoder_keys"] > 0 and run["decoder_changed"] == [] and run["encoder_unmoved"] == []
    # Adam moves a weight by at most lr per step; a near-zero gradient of the other sign moves it the other way: 2 x lr x 3 steps (+25 %)
    lr = float(g["cfg/lr"])
    assert len(run["param_after"]) == 30
    for n, got in run["param_after"].items():
        fp = synth.fp_unpack(g, f"param_after/{n}")
        assert np.abs(got - fp["sample"]).max() <= 7.5 * lr, (n, np.abs(got - fp["sample"]).max())


def test_kernel_on_the_reference_embeddings(golden):
    """The reference's own raw embeddings of iteration 1 and its own loss value."""
    from miseg_amd import ops
    g = golden("contrast")
    e = torch.from_numpy(g["embeddings_step1"]).to(DEV)
    loss = ops.supcon(e, torch.tensor(g["labels"], dtype=torch.int32, device=DEV), 2)
    assert abs(float(loss) - float(g["loss"][0])) <= LOSS_BOUND * float(g["loss"][0])


# ---------------------------------------------------------------------------------------------------------------- 7. bf16
def test_bf16_step_runs_with_finite_loss_and_gradients(golden):
    """``Arch.compute_dtype=bfloat16``: the same three iterations run, loss and every gradient finite.  The distance of the loss from the
    fp32 run is printed and recorded (MISEG_ERROR_DUMP), not asserted."""
    g = golden("contrast")
    run = _golden_run(g, "bfloat16")
    fp32 = _golden_run(g)
    assert len(run["losses"]) == 3 and all(np.isfinite(v) for v in run["losses"])
    assert len(run["grads_finite"]) == 3 and all(run["grads_finite"])
    assert all("SupCon" in f for f in run["fused"])
    row = {"bf16": run["losses"], "fp32": fp32["losses"], "relative": [abs(a - b) / abs(b) for a, b in zip(run["losses"], fp32["losses"])]}
    print("contrast bf16 against fp32 loss:", row)
    _dump("bf16_loss", row)


# ---------------------------------------------------------------------------------------------------------------- 8. the CLI
_TINY = ["Trainer.device=cuda", "Trainer.num_batches=2", "Data.name=synthetic", "Data.size=64", "LabeledData.batch_size=2", "UnlabeledData.batch_size=4"]

_FINE_TUNE = r"""
import os, sys, torch
from semi_seg.main import build_trainer
ck = torch.load(os.path.join(os.environ["CONTRAST_RUN"], "last.pth"), map_location="cpu", weights_only=False)
args = sys.argv[1:]
fresh = build_trainer([a for a in args if not a.startswith("Pretrained=")] + ["Trainer.save_dir=" + os.environ["CONTRAST_FT"] + "_fresh"])
tr = build_trainer(args + ["Trainer.save_dir=" + os.environ["CONTRAST_FT"]])
assert tr._start_epoch == 0 and tr._cur_epoch == 0, (tr._start_epoch, tr._cur_epoch)
sd, init = tr._model.state_dict(), fresh._model.state_dict()
enc = [k for k in sd if k.startswith("Conv")]
dec = [k for k in sd if not k.startswith("Conv")]
assert enc and dec
assert all(torch.equal(sd[k].cpu(), ck["_model"][k]) for k in sd)
assert all(torch.equal(sd[k].cpu(), init[k].cpu()) for k in dec)
assert any(not torch.equal(sd[k].cpu(), init[k].cpu()) for k in enc)
assert all(p.requires_grad for p in tr._model.parameters())
tr.start_training()
print("fine-tuned from epoch", tr._start_epoch, "to", tr._cur_epoch)
"""


def test_main_cli_pretrains_and_fine_tunes_from_pretrained():
    """``python semi_seg/main.py Trainer.name=contrast ... ContrastParameters.group_option=patient``: two tiny epochs; config.yaml with
    the section, last.pth with ``_projector``, no best.pth, storage.csv with a contrastive_loss column.  Then ``Trainer.name=partial
    Pretrained=<that dir>`` in a fresh process: starts at epoch 0, the model is the checkpoint's, the decoder is a fresh ``RandomSeed``
    initialisation (which the pre-training never touched), one tiny epoch trains."""
    import yaml
    save = f"pytest_cli_contrast_{os.getpid()}"
    run_dir = th.run_dir(save)
    ft = save + "_ft"
    try:
        shutil.rmtree(run_dir, ignore_errors=True)
        th.run_main(["Trainer.name=contrast", "ContrastParameters.group_option=patient", f"Trainer.save_dir={save}", "Trainer.max_epoch=2"] + _TINY)
        files = set(os.listdir(run_dir))
        assert {"config.yaml", "last.pth", "storage.csv"} <= files and "best.pth" not in files, files
        cfg = yaml.safe_load(open(os.path.join(run_dir, "config.yaml")))
        assert cfg["ContrastParameters"] == {"group_option": "patient", "extract_position": "Conv5", "ptype": "mlp", "output_dim": 256,
                                             "temperature": 0.07, "base_temperature": 0.07}
        lines = open(os.path.join(run_dir, "storage.csv")).read().splitlines()
        assert any("contrastive_loss" in h for h in lines[0].split(",")) and len(lines) == 3, lines[:1]
        ck = torch.load(os.path.join(run_dir, "last.pth"), map_location="cpu", weights_only=False)
        assert {"_model", "_projector", "_optimizer", "_scheduler", "_contrastive_criterion", "_storage", "_buffers"} <= set(ck)
        assert sorted(ck["_projector"]) == ["_header.2.bias", "_header.2.weight", "_header.4.bias", "_header.4.weight"]
        assert ck["_buffers"]["_cur_epoch"] == 1
        assert len(ck["_optimizer"]["param_groups"][0]["params"]) == 5 * 6 + 4           # the encoder's and the projector's only
        res = th.run_main(["Trainer.name=partial", f"Pretrained={run_dir}", "Trainer.max_epoch=1"] + _TINY, code=_FINE_TUNE,
                          env={"CONTRAST_RUN": run_dir, "CONTRAST_FT": ft})
        assert "fine-tuned from epoch 0 to 0" in res.stdout, res.stdout[-2000:] + res.stderr[-4000:]
        ck2 = torch.load(os.path.join(run_dir + "_ft", "last.pth"), map_location="cpu", weights_only=False)
        assert ck2["_buffers"]["_cur_epoch"] == 0 and "_projector" not in ck2
    finally:
        for d in (run_dir, run_dir + "_ft", run_dir + "_ft_fresh"):
            shutil.rmtree(d, ignore_errors=True)
