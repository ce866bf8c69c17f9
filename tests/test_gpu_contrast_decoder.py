"""GPU: contrastive decoder pre-training (``Trainer.name=contrastdecoder``) -- the bias + LeakyReLU and adaptive
max-pool kernels bit for bit against fp32 torch on the CPU computed from the stored inputs, their bias gradients against float64 sums,
determinism and refusals, ``LocalProjectionHead`` against float64 autograd, the epocher against the reference's own run
(tests/golden/contrast_decoder.npz), a bf16 run and the three-stage CLI chain."""
import os
import shutil
from functools import partial

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import synth
import trainer_harness as th
from contrast_decoder_ref import GROUPS, embed_rows, golden_projector_state, golden_views, group_of, pool_reference, same_bits
from oracle import unet as OU
from trainer_harness import DEV

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
SENTINEL = 3.0


_dump = partial(th.error_dump, "contrast_decoder")          # the numbers DESIGN.md section 15 quotes


def _rel(got, ref):
    return float((got - ref).abs().max() / ref.abs().max())


def _dt(dtype):
    from miseg_amd import _cabi
    return {torch.float32: _cabi.F32, torch.bfloat16: _cabi.BF16, torch.float16: _cabi.F16}[dtype]


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------------------------------------------- 1. bias + LeakyReLU
# [N, H, W, C].  The first four are the issue's; the last has more fp32 vectors than one stride of the capped grid (1024 blocks), so
# that the second of a thread's four loads in flight is a real one.
LRELU_SHAPES = [(1, 3, 3, 64), (2, 5, 7, 32), (3, 16, 16, 32), (4, 64, 64, 64), (8, 64, 64, 64)]
GBIAS_BOUND = 1e-5     # max |error| / max |reference|: the bound of the other reduction kernels


def _lrelu_inputs(shape, dtype, seed):
    """raw of ``dtype`` with exact zeros and entries where raw + bias == 0 (the bias is a multiple of 1/8, exact in every type)."""
    n, h, w, c = shape
    g = torch.Generator().manual_seed(seed)
    bias = torch.randint(-8, 9, (c,), generator=g).float() / 8
    raw = torch.randn(shape, generator=g).to(dtype)
    flat = raw.view(-1, c)
    rows = torch.arange(flat.shape[0])
    flat[rows[::3], (rows[::3] * 5) % c] = 0
    cancel = (rows[1::4] * 7) % c
    flat[rows[1::4], cancel] = (-bias[cancel]).to(dtype)
    return raw, bias


def _lrelu_reference(raw, bias, slope):
    v = raw.float() + bias.view(1, 1, 1, -1)
    return torch.where(v > 0, v, v * slope).to(raw.dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("shape", LRELU_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bias_lrelu_forward_and_gx_bit_exact_and_gbias(shape, dtype):
    from miseg_amd import _cabi
    n, h, w, c = shape
    raw, bias = _lrelu_inputs(shape, dtype, seed=sum(shape))
    g = torch.Generator().manual_seed(1 + sum(shape))
    gy = (torch.randn(shape, generator=g) + 0.5).to(dtype)            # mean 0.5: the channel sums do not cancel
    assert bool((raw == 0).any()) and bool(((raw.float() + bias.view(1, 1, 1, -1)) == 0).any())
    rows = []
    for slope in (0.01, 1.0):
        ref_y = _lrelu_reference(raw, bias, slope)
        terms = torch.where(ref_y.float() > 0, gy.float(), gy.float() * slope)
        ref_gx, ref_gb = terms.to(dtype), terms.double().sum(dim=(0, 1, 2))
        nbytes = int(_cabi.lib().miseg_bias_lrelu_bwd_ws_bytes(_dt(dtype), n, h, w, c))
        assert nbytes > 0
        for inplace in (False, True):
            x, b = raw.to(DEV), bias.to(DEV)
            y = x if inplace else torch.full_like(x, SENTINEL)
            _cabi.call("miseg_bias_lrelu_fwd", _stream(), _dt(dtype), x.data_ptr(), n, h, w, c, b.data_ptr(), slope, y.data_ptr())
            assert same_bits(y, ref_y), (slope, inplace)
            gyd = gy.to(DEV)
            gx = gyd if inplace else torch.full_like(gyd, SENTINEL)
            gb = torch.full((c,), SENTINEL, device=DEV)
            ws = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
            _cabi.call("miseg_bias_lrelu_bwd", _stream(), _dt(dtype), y.data_ptr(), gyd.data_ptr(), n, h, w, c, slope, gx.data_ptr(), gb.data_ptr(),
                       ws.data_ptr(), ws.numel())
            assert same_bits(gx, ref_gx), (slope, inplace)
            err = _rel(gb.cpu().double(), ref_gb)
            rows.append({"slope": slope, "inplace": inplace, "gbias": err})
            assert err <= GBIAS_BOUND, rows
    print("bias_lrelu", shape, dtype, rows)
    _dump(f"lrelu_{'x'.join(map(str, shape))}_{str(dtype).split('.')[-1]}", rows)


# ---------------------------------------------------------------------------------------------------------------- 2. adaptive max-pool
# (N, C, H, W), (OH, OW), (PH, PW), V
POOL_CASES = [((4, 32, 8, 8), (4, 4), (2, 2), 2), ((4, 32, 10, 7), (4, 4), (2, 2), 2), ((2, 32, 3, 5), (4, 4), (2, 2), 1),
              ((3, 64, 16, 16), (4, 4), (1, 1), 1), ((6, 32, 12, 12), (2, 2), (2, 2), 2), ((8, 32, 32, 32), (4, 4), (2, 2), 2)]


def _pool_call(raw, bias, osz, part, views, fill=SENTINEL):
    from miseg_amd import _cabi
    n, h, w, c = raw.shape
    rows, cols = n * part[0] * part[1], c * (osz[0] // part[0]) * (osz[1] // part[1])
    e = torch.full((rows, cols), fill, device=DEV)
    idx = torch.full((n, osz[0], osz[1], c), -7, dtype=torch.int32, device=DEV)
    _cabi.call("miseg_bias_amaxpool_fwd", _stream(), _dt(raw.dtype), raw.data_ptr(), n, h, w, c, None if bias is None else bias.data_ptr(),
               osz[0], osz[1], part[0], part[1], views, e.data_ptr(), idx.data_ptr())
    return e, idx


def _pool_bwd_call(ge, idx, shape, dtype, osz, part, views):
    from miseg_amd import _cabi
    n, h, w, c = shape
    graw = torch.full(shape, SENTINEL, dtype=dtype, device=DEV)
    gb = torch.full((c,), SENTINEL, device=DEV)
    _cabi.call("miseg_bias_amaxpool_bwd", _stream(), _dt(dtype), ge.data_ptr(), idx.data_ptr(), n, h, w, c, osz[0], osz[1], part[0], part[1], views,
               graw.data_ptr(), gb.data_ptr())
    return graw, gb


def _pool_check(raw, bias, osz, part, views, seed=0):
    """Forward values and indices, backward and bias gradient of one input against the CPU expression; returns (graw, ge, idx)."""
    ref_e, ref_idx, leaf = pool_reference(raw, bias, osz, part, views)
    e, idx = _pool_call(raw.to(DEV), bias.to(DEV), osz, part, views)
    assert same_bits(idx, ref_idx)
    assert same_bits(e, ref_e.detach())
    g = torch.Generator().manual_seed(seed)
    ge = torch.randn(ref_e.shape, generator=g) + 0.5
    ref_e.backward(ge)
    ref_graw = leaf.grad.permute(0, 2, 3, 1).contiguous().to(raw.dtype)
    graw, gb = _pool_bwd_call(ge.to(DEV), idx, tuple(raw.shape), raw.dtype, osz, part, views)
    assert same_bits(graw, ref_graw)
    n, h, w, c = raw.shape
    per_channel = ge.double().view(-1, c, (osz[0] // part[0]) * (osz[1] // part[1])).sum(dim=(0, 2))
    err = _rel(gb.cpu().double(), per_channel)
    assert err <= GBIAS_BOUND, err
    return graw.cpu(), ge, idx.cpu(), err


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("shape,osz,part,views", POOL_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_bias_amaxpool_forward_backward_bit_exact(shape, osz, part, views, dtype):
    n, c, h, w = shape
    g = torch.Generator().manual_seed(n * 1000 + h * 10 + w)
    raw = torch.randn(n, h, w, c, generator=g).to(dtype)
    bias = torch.randn(c, generator=g)
    planted = (h, w) == (10, 7)
    if planted:
        # rows [0, 3) and [2, 5) of the window grid share row 2, columns [0, 2) and [1, 4) share column 1: pixel (2, 0) is the maximum of
        # two windows in channel 0, pixel (2, 1) of four windows in channel 1
        raw[0, 2, 0, 0] = 100.0
        raw[0, 2, 1, 1] = 100.0
    graw, ge, idx, err = _pool_check(raw, bias, osz, part, views, seed=c + h)
    print("bias_amaxpool", shape, osz, part, views, dtype, {"gbias": err})
    _dump(f"pool_{'x'.join(map(str, shape))}_{str(dtype).split('.')[-1]}", {"gbias": err})
    if (part, views) == ((1, 1), 1):            # the contiguous NCHW tensor the reference module returns
        e, _ = _pool_call(raw.to(DEV), bias.to(DEV), osz, part, views)
        ref = F.adaptive_max_pool2d(raw.float().permute(0, 3, 1, 2), osz) + bias.view(1, -1, 1, 1)
        assert same_bits(e.view(n, c, *osz), ref.contiguous())
    if planted:
        rows = ge.view(views, part[0], part[1], n // views, c, osz[0] // part[0], osz[1] // part[1])   # [v, ph, pw, b, c, dh, dw]

        def at(oh, ow, ch):
            return rows[0, oh // 2, ow // 2, 0, ch, oh % 2, ow % 2]

        two = (at(0, 0, 0) + at(1, 0, 0)).to(dtype)
        four = (((at(0, 0, 1) + at(0, 1, 1)) + at(1, 0, 1)) + at(1, 1, 1)).to(dtype)
        assert idx[0, 0, 0, 0] == idx[0, 1, 0, 0] == 2 * w and idx[0, 0, 0, 1] == idx[0, 1, 1, 1] == 2 * w + 1
        assert same_bits(graw[0, 2, 0, 0], two) and same_bits(graw[0, 2, 1, 1], four)
        # nothing else of the sentinel-filled gradient survives in those windows: every other pixel of channel 0 in rows 0..4, column
        # 0 (which only those two windows contain) of sample 0 is exactly zero
        column = graw[0, 0:5, 0, 0].clone()
        column[2] = 0
        assert not bool(column.any())


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_bias_amaxpool_ties_take_the_first_index_and_a_nan_wins(dtype):
    osz, part, views = (4, 4), (2, 2), 2
    hh, ww = torch.meshgrid(torch.arange(12), torch.arange(10), indexing="ij")
    patches = ((hh // 2) * 3 + ww // 3).float()                                    # constant 2 x 3 patches: every window has ties
    raw = (patches.view(1, 12, 10, 1) * torch.ones(4, 1, 1, 32)).to(dtype).contiguous()
    raw[1] = 0.25                                                                   # a constant sample: index of the window's first pixel
    bias = torch.zeros(32)
    _, _, idx, _ = _pool_check(raw, bias, osz, part, views)
    assert int(idx[1, 0, 0, 0]) == 0 and int(idx[1, 3, 3, 5]) == 9 * 10 + 7          # rows [9, 12), columns [7, 10)
    g = torch.Generator().manual_seed(3)
    raw = torch.randn(4, 12, 10, 32, generator=g).to(dtype)
    raw[2, 7, 4, 9] = float("nan")                                                  # rows [6, 9) x columns [2, 5) and [5, 8): window (2, 1)
    ref_e, ref_idx, _ = pool_reference(raw, bias, osz, part, views)
    e, idx = _pool_call(raw.to(DEV), bias.to(DEV), osz, part, views)
    assert same_bits(idx, ref_idx) and same_bits(e, ref_e.detach())
    assert int(idx[2, 2, 1, 9]) == 7 * 10 + 4 and int(torch.isnan(e).sum()) == 1


# ---------------------------------------------------------------------------------------------------------------- 3. determinism, refusals
def test_two_calls_of_each_entry_point_are_bit_identical():
    from miseg_amd import _cabi
    shape, osz, part, views = (8, 33, 31, 32), (4, 4), (2, 2), 2
    n, h, w, c = shape
    g = torch.Generator().manual_seed(9)
    for dtype in DTYPES:
        raw, gy = torch.randn(shape, generator=g).to(dtype).to(DEV), (torch.randn(shape, generator=g) + 0.5).to(dtype).to(DEV)
        bias = torch.randn(c, generator=g).to(DEV)
        got = []
        for _ in range(2):
            y = torch.empty_like(raw)
            _cabi.call("miseg_bias_lrelu_fwd", _stream(), _dt(dtype), raw.data_ptr(), n, h, w, c, bias.data_ptr(), 0.01, y.data_ptr())
            gx, gb = torch.empty_like(raw), torch.empty(c, device=DEV)
            ws = torch.empty(int(_cabi.lib().miseg_bias_lrelu_bwd_ws_bytes(_dt(dtype), n, h, w, c)), dtype=torch.uint8, device=DEV)
            _cabi.call("miseg_bias_lrelu_bwd", _stream(), _dt(dtype), y.data_ptr(), gy.data_ptr(), n, h, w, c, 0.01, gx.data_ptr(), gb.data_ptr(),
                       ws.data_ptr(), ws.numel())
            e, idx = _pool_call(raw, bias, osz, part, views)
            graw, gb2 = _pool_bwd_call(e, idx, shape, dtype, osz, part, views)
            got.append((y, gx, gb, e, idx, graw, gb2))
        torch.cuda.synchronize()
        assert all(same_bits(a, b) for a, b in zip(*got)), dtype
        assert all(bool(torch.isfinite(t.float()).all()) for t in got[0])


def test_refusals_launch_nothing():
    """C = 30, an output size the partition does not divide, N not a multiple of V, a null pointer, a short workspace: MISEG_E_INVALID,
    the sentinel-filled outputs untouched, and ``miseg_last_error`` names the entry point."""
    from miseg_amd import _cabi, ops
    n, h, w, c = 4, 8, 8, 32
    raw = torch.randn(n, h, w, c, device=DEV)
    bias = torch.zeros(64, device=DEV)
    y, gx = torch.full_like(raw, SENTINEL), torch.full_like(raw, SENTINEL)
    gb = torch.full((64,), SENTINEL, device=DEV)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    e = torch.full((16, 128), SENTINEL, device=DEV)
    idx = torch.full((n, 4, 4, c), -7, dtype=torch.int32, device=DEV)
    dt, st = _cabi.F32, _stream()

    def refused(name, *args):
        with pytest.raises(_cabi.MisegError) as info:
            _cabi.call(name, st, dt, *args)
        assert name[len("miseg_"):] in str(info.value), str(info.value)

    assert not ops.bias_lrelu_supported(30) and not ops.bias_amaxpool_supported(n, 30, h, w, (4, 4), (2, 2), 2)
    assert not ops.bias_amaxpool_supported(n, c, h, w, (4, 4), (3, 2), 2) and not ops.bias_amaxpool_supported(n, c, h, w, (4, 4), (2, 2), 3)
    assert ops.bias_amaxpool_supported(n, c, h, w, (4, 4), (2, 2), 2) and ops.bias_lrelu_supported(c)
    refused("miseg_bias_lrelu_fwd", raw.data_ptr(), n, h, w, 30, bias.data_ptr(), 0.01, y.data_ptr())
    refused("miseg_bias_lrelu_fwd", None, n, h, w, c, bias.data_ptr(), 0.01, y.data_ptr())
    refused("miseg_bias_lrelu_bwd", raw.data_ptr(), raw.data_ptr(), n, h, w, 30, 0.01, gx.data_ptr(), gb.data_ptr(), ws.data_ptr(), ws.numel())
    refused("miseg_bias_lrelu_bwd", None, raw.data_ptr(), n, h, w, c, 0.01, gx.data_ptr(), gb.data_ptr(), ws.data_ptr(), ws.numel())
    need = int(_cabi.lib().miseg_bias_lrelu_bwd_ws_bytes(dt, n, h, w, c))
    assert need > 16 and int(_cabi.lib().miseg_bias_lrelu_bwd_ws_bytes(dt, n, h, w, 30)) == -1
    refused("miseg_bias_lrelu_bwd", raw.data_ptr(), raw.data_ptr(), n, h, w, c, 0.01, gx.data_ptr(), gb.data_ptr(), ws.data_ptr(), need - 16)
    for cc, osz, part, views in ((30, (4, 4), (2, 2), 2), (c, (4, 4), (3, 2), 2), (c, (4, 4), (2, 3), 2), (c, (4, 4), (2, 2), 3)):
        refused("miseg_bias_amaxpool_fwd", raw.data_ptr(), n, h, w, cc, bias.data_ptr(), osz[0], osz[1], part[0], part[1], views, e.data_ptr(), idx.data_ptr())
        refused("miseg_bias_amaxpool_bwd", e.data_ptr(), idx.data_ptr(), n, h, w, cc, osz[0], osz[1], part[0], part[1], views, gx.data_ptr(), gb.data_ptr())
    refused("miseg_bias_amaxpool_fwd", None, n, h, w, c, bias.data_ptr(), 4, 4, 2, 2, 2, e.data_ptr(), idx.data_ptr())
    refused("miseg_bias_amaxpool_bwd", e.data_ptr(), None, n, h, w, c, 4, 4, 2, 2, 2, gx.data_ptr(), gb.data_ptr())
    torch.cuda.synchronize()
    for t in (y, gx, gb, e):
        assert bool((t == SENTINEL).all())
    assert bool((idx == -7).all()) and not bool(ws.any())


# ---------------------------------------------------------------------------------------------------------------- 4. the module
HEAD_BOUND = 1e-5      # output, feature gradient and parameter gradients, relative to the largest entry (test_gpu_contrast's head bound)
MARGIN = 1e-4          # no LeakyReLU input and no top-two gap of a pooling window closer to a branch than this x the tensor's largest entry


def _reference_head(head, head_type):
    ref = torch.nn.Sequential(torch.nn.Conv2d(32, 64, 3, 1, 1), torch.nn.LeakyReLU(0.01), torch.nn.Conv2d(64, 32, 3, 1, 1)) if head_type == "mlp" \
        else torch.nn.Sequential(torch.nn.Conv2d(32, 64, 3, 1, 1))
    ref.load_state_dict({k.replace("_projector.", ""): v for k, v in head.state_dict().items()})
    return ref.double()


def _clear_of_branches(ref, feat64):
    """float64 on the CPU: every LeakyReLU input and every top-two gap of a 2 x 2 pooling window at least MARGIN x the largest entry."""
    with torch.no_grad():
        x = feat64
        for layer in ref:
            if isinstance(layer, torch.nn.LeakyReLU) and float(x.abs().min()) < MARGIN * float(x.abs().max()):
                return False
            x = layer(x)
        n, c, h, w = x.shape
        top = x.view(n, c, 4, h // 4, 4, w // 4).permute(0, 1, 2, 4, 3, 5).reshape(n, c, 4, 4, -1).topk(2, dim=-1).values
        return float((top[..., 0] - top[..., 1]).min()) >= MARGIN * float(x.abs().max())


@pytest.mark.parametrize("head_type", ["mlp", "linear"])
def test_local_projection_head_against_float64_autograd(head_type):
    """An NHWC fp32 feature [4, 32, 8, 8] through ``LocalProjectionHead`` against float64 autograd of the reference-shaped
    ``nn.Sequential`` + ``adaptive_max_pool2d``.  The input seed is the first, from 0, that keeps every branch MARGIN away in float64, so
    fp32 rounding cannot move one; ``embeddings()`` is ``unfold_position`` of ``forward()`` bit for bit."""
    from contrastyou.epocher._utils import unfold_position
    from contrastyou.trainer._utils import LocalProjectionHead
    torch.manual_seed(0)
    head = LocalProjectionHead(32, head_type=head_type)
    ref = _reference_head(head, head_type)
    for seed in range(5000):
        g = torch.Generator().manual_seed(seed)
        feat = torch.randn(4, 32, 8, 8, generator=g)
        if _clear_of_branches(ref, feat.double()):
            break
    else:
        raise AssertionError("no input seed below 5000 keeps the branches clear")
    cout = 32 if head_type == "mlp" else 64
    probe = torch.randn(4, cout, 4, 4, generator=g)
    f64 = feat.double().requires_grad_()
    out64 = F.adaptive_max_pool2d(ref(f64), (4, 4))
    (out64 * probe.double()).sum().backward()
    head = head.to(DEV)
    fd = feat.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_()
    out = head(fd)
    assert tuple(out.shape) == (4, cout, 4, 4) and "BiasAMaxPool" in type(out.grad_fn).__name__ + type(out.grad_fn.next_functions[0][0]).__name__
    (out * probe.to(DEV)).sum().backward()
    err = {"seed": seed, "out": _rel(out.detach().cpu().double(), out64.detach()), "feature_grad": _rel(fd.grad.cpu().double(), f64.grad)}
    for (k, p), (_, q) in zip(head.named_parameters(), ref.named_parameters()):
        err[k] = _rel(p.grad.cpu().double(), q.grad)
    print("local projection head", head_type, err)
    _dump(f"head_{head_type}", err)
    assert len(err) == (7 if head_type == "mlp" else 5)
    assert max(v for k, v in err.items() if k != "seed") < HEAD_BOUND, err
    with torch.no_grad():
        rows = head.embeddings(fd, views=2, partition_num=(2, 2))
        pooled = head(fd)
        want = torch.cat([unfold_position(chunk, (2, 2))[0].reshape(8, -1) for chunk in torch.chunk(pooled, 2, dim=0)])
    assert same_bits(rows, want)


# ---------------------------------------------------------------------------------------------------------------- 5. the epocher
_RUNS = {}
TRAINED = ("Up5.", "Up_conv5.", "Up4.", "Up_conv4.", "Up3.", "Up_conv3.")
UNTOUCHED = ("Up2.", "Up_conv2.", "DeConv_1x1.")


def _golden_run(g, dtype="float32"):
    """The fixture's three iterations through ``PretrainDecoderEpocher``; computed once per dtype and shared (as plain data)."""
    if dtype in _RUNS:
        return _RUNS[dtype]
    import random
    from contrastyou.arch import UNet
    from contrastyou.losses.contrast_loss import SupConLoss
    from contrastyou.trainer._utils import LocalProjectionHead
    from deepclustering2.optim import Adam
    from miseg_amd import unet_ops
    from semi_seg.epocher import PretrainDecoderEpocher
    cfg = {k[4:]: g[k].item() for k in g.files if k.startswith("cfg/")}
    H, B, NB = int(cfg["H"]), int(cfg["B"]), int(cfg["NB"])
    model = UNet(1, 4, compute_dtype=dtype)
    model.load_state_dict(OU.init_state(1, 4, seed=int(cfg["model_seed"])))
    projector = LocalProjectionHead(32, head_type="mlp", output_size=(4, 4))
    projector.load_state_dict(golden_projector_state())
    model, projector = model.to(DEV), projector.to(DEV)
    model.disable_grad_all()
    model.enable_grad(str(cfg["grad_from"]), str(cfg["position"]))
    initial = {k: v.detach().clone() for k, v in model.state_dict().items()}
    initial_projector = {k: v.detach().clone() for k, v in projector.state_dict().items()}
    named = [(f"{blk}.{n}", p) for blk in model._range(str(cfg["grad_from"]), str(cfg["position"])) for n, p in getattr(model, blk).named_parameters()]
    named += list(projector.named_parameters())
    opt = Adam((p for _, p in named), lr=float(cfg["lr"]), weight_decay=float(cfg["wd"]))
    partitions, patients = [str(p) for p in g["partitions"]], [str(p) for p in g["patients"]]

    def loader():
        tgt = torch.zeros(B, 1, H, H, dtype=torch.long)
        for i in range(NB):
            a, b = golden_views(i, B, H)
            yield [[[a, tgt], [b, tgt.clone()]], [f"{p}_{j}" for j, p in enumerate(patients)], list(partitions), list(patients)]

    crit = SupConLoss()
    losses, labels_seen, fused, masks, pooled = [], [], [], [], []
    inner = crit.from_embeddings
    ep = PretrainDecoderEpocher(model, projector, opt, loader(), crit, NB, 0, DEV, str(cfg["position"]), (2, 2))

    def spy(e, labels=None, views=2):
        v = inner(e, labels, views)
        losses.append(float(v.detach()))
        labels_seen.append(list(labels))
        fused.append(type(v.grad_fn).__name__ + "|" + type(e.grad_fn).__name__)
        masks.append(list(ep.last_flip_masks))
        pooled.append(e.detach().cpu().clone())
        return v

    crit.from_embeddings = spy
    grads, real_adam = [], unet_ops.adam_step

    def adam_spy(param, grad, *a, **k):
        grads.append(grad.detach().clone())
        return real_adam(param, grad, *a, **k)

    unet_ops.adam_step = adam_spy
    random.seed(int(cfg["py_seed"]))
    try:
        res = ep.run()
    finally:
        unet_ops.adam_step = real_adam
        crit.from_embeddings = inner

    def sampled(flat, name, param, tag):
        return th.sampled(flat, opt.flat.offset_of(param), param.numel(), f"{tag}/{name}")

    now, now_projector = model.state_dict(), projector.state_dict()
    # plain data only: a model kept alive here would stay registered with the weight-pack cache for the rest of the session
    out = dict(res={k: dict(v) for k, v in res.items()}, losses=losses, labels=labels_seen, fused=fused, masks=masks, rows_step1=pooled[0],
               names=[n for n, _ in named],
               grad_step1={n: sampled(grads[0], n, p, "grad_step1") for n, p in named},
               grads_finite=[bool(torch.isfinite(x).all()) for x in grads],
               param_after={n: sampled(opt.flat.flat_param, n, p, "param_after") for n, p in named},
               frozen_changed=[n for n, p in model.named_parameters() if not n.startswith(TRAINED) and not torch.equal(p.detach(), initial[n])],
               untouched_changed=[k for k, v in now.items() if k.startswith(UNTOUCHED) and not torch.equal(v, initial[k])],
               untouched_keys=sum(1 for k in now if k.startswith(UNTOUCHED)),
               trained_unmoved=[n for n, p in model.named_parameters() if n.startswith(TRAINED) and torch.equal(p.detach(), initial[n])]
               + [k for k, v in now_projector.items() if torch.equal(v, initial_projector[k])],
               encoder_running_mean_moved=[k for k, v in now.items() if k.startswith("Conv") and k.endswith("running_mean") and not torch.equal(v, initial[k])])
    _RUNS[dtype] = out
    del res, model, projector, opt, named, grads, now, initial, crit, inner, spy, ep
    import gc
    gc.collect()
    return out


def _group_distances(run, g):
    num, den = {}, {}
    for n in run["names"]:
        got = run["grad_step1"][n]
        ref = synth.fp_unpack(g, f"grad_step1/{n}")["sample"].astype(np.float64)
        k = group_of(n)
        num[k] = num.get(k, 0.0) + float(((got - ref) ** 2).sum())
        den[k] = den.get(k, 0.0) + float((ref ** 2).sum())
    return {k: (num[k] / den[k]) ** 0.5 for k in num}


def test_epocher_matches_the_reference_run(golden):
    """fp32, 3 iterations against the reference's PretrainDecoderEpoch / LocalProjectionHead / SupConLoss / LocalLabelGenerator
    (tests/golden/contrast_decoder.npz): the drawn masks, the labels, the pooled output of iteration 1, the losses, the step-1 gradients
    per parameter group, and what moved after the three steps."""
    g = golden("contrast_decoder")
    run = _golden_run(g)
    assert run["masks"] == [[int(m) for m in row] for row in g["masks"]]
    assert run["labels"] == [[int(v) for v in g["labels"]]] * 3
    assert all(f == "_SupConBackward|_BiasAMaxPoolBackward" for f in run["fused"]), run["fused"]
    want_rows = embed_rows(torch.from_numpy(g["pooled_step1"]), (2, 2), 2)
    # the pooled output of iteration 1: within 8 x the reference's own largest fp32 <-> float64 distance of the tensor that is pooled
    rows_err, rows_bound = float((run["rows_step1"].double() - want_rows.double()).abs().max()), 8.0 * float(g["conv_out_dist_max"])
    print("contrastdecoder golden losses:", run["losses"], list(g["loss"]), "pooled output of iteration 1:", rows_err, "bound", rows_bound)
    assert rows_err <= rows_bound
    np.testing.assert_allclose(run["losses"], g["loss"], rtol=1e-3)
    assert sorted(run["res"]) == ["contrastive_loss", "lr"]
    assert abs(run["res"]["contrastive_loss"]["mean"] - float(np.mean(g["loss"]))) <= 1e-3 * float(np.mean(g["loss"]))
    # step-1 gradients, relative L2 per parameter group on the fingerprint samples.  Bound per group: max(4 x the fixture seed's own fp32
    # error against float64, the largest own error among the generator's 16 model seeds, 2e-5), capped at 3e-2 -- what a flipped
    # LeakyReLU / arg-max branch costs in this configuration, measured on the reference alone (make_golden_contrast_decoder.py)
    assert run["names"] == [str(n) for n in g["param_names"]]
    dist = _group_distances(run, g)
    seed, seeds = int(g["cfg/model_seed"]), [int(s) for s in g["model_seeds"]]
    own = {k: float(g[f"own_error/{seed}/{k}"]) for k in GROUPS}
    worst = {k: max(float(g[f"own_error/{s}/{k}"]) for s in seeds) for k in GROUPS}
    bound = {k: min(max(4.0 * own[k], worst[k], 2e-5), 3e-2) for k in GROUPS}
    print("contrastdecoder golden gradients:", dist, "bounds", bound, "own error", own)
    _dump("golden_grad", {"distance": dist, "bound": bound, "own": own, "losses": run["losses"], "rows_step1": rows_err})
    assert sorted(dist) == sorted(GROUPS)
    assert all(dist[k] <= bound[k] for k in dist), (dist, bound)
    # after the three steps: the encoder's parameters and everything of Up2 / Up_conv2 / DeConv_1x1 (parameters and BatchNorm buffers) bit
    # for bit where they started; every parameter of Up5 .. Up_conv3 and of the projector moved; the frozen encoder's BatchNorm running
    # statistics moved (its forward is in train mode, as in the reference)
    assert run["frozen_changed"] == [] and run["untouched_keys"] > 0 and run["untouched_changed"] == []
    assert run["trained_unmoved"] == []
    assert run["encoder_running_mean_moved"]
    # Adam moves a weight by at most lr per step; a near-zero gradient of the other sign moves it the other way: 2 x lr x 3 steps (+25 %)
    lr = float(g["cfg/lr"])
    assert len(run["param_after"]) == len(run["names"])
    for n, got in run["param_after"].items():
        fp = synth.fp_unpack(g, f"param_after/{n}")
        assert np.abs(got - fp["sample"]).max() <= 7.5 * lr, (n, np.abs(got - fp["sample"]).max())


def test_bf16_run_is_finite(golden):
    """``Arch.compute_dtype=bfloat16``: the same three iterations run, loss and every gradient finite.  The distance from the fp32 run is
    printed and recorded (MISEG_ERROR_DUMP), not asserted."""
    g = golden("contrast_decoder")
    run = _golden_run(g, "bfloat16")
    fp32 = _golden_run(g)
    assert len(run["losses"]) == 3 and all(np.isfinite(v) for v in run["losses"])
    assert len(run["grads_finite"]) == 3 and all(run["grads_finite"])
    assert all(f == "_SupConBackward|_BiasAMaxPoolBackward" for f in run["fused"])
    assert run["masks"] == fp32["masks"]
    ref = {n: fp32["grad_step1"][n] for n in fp32["names"]}
    num = sum(float(((run["grad_step1"][n] - ref[n]) ** 2).sum()) for n in ref)
    den = sum(float((ref[n] ** 2).sum()) for n in ref)
    row = {"bf16": run["losses"], "fp32": fp32["losses"], "relative": [abs(a - b) / abs(b) for a, b in zip(run["losses"], fp32["losses"])],
           "grad_step1_relative_l2": (num / den) ** 0.5}
    print("contrastdecoder bf16 against fp32:", row)
    _dump("bf16", row)


# ---------------------------------------------------------------------------------------------------------------- 6. the CLI
_TINY = ["Trainer.device=cuda", "Trainer.num_batches=2", "Data.name=synthetic", "Data.size=64", "LabeledData.batch_size=2", "UnlabeledData.batch_size=4"]

_STAGE = r"""
import os, sys, torch
from semi_seg.main import build_trainer
before = torch.load(os.path.join(os.environ["STAGE_FROM"], "last.pth"), map_location="cpu", weights_only=False)["_model"]
tr = build_trainer(sys.argv[1:])
assert tr._start_epoch == 0 and tr._cur_epoch == 0, (tr._start_epoch, tr._cur_epoch)
sd = tr._model.state_dict()
assert all(torch.equal(sd[k].cpu(), before[k]) for k in sd), "the model is not the checkpoint's"
tr.start_training()
print("stage done: epochs", tr._start_epoch, "to", tr._cur_epoch)
"""


def test_main_cli_runs_the_three_stages():
    """``Trainer.name=contrast``, then ``Trainer.name=contrastdecoder Pretrained=<run 1>``, then ``Trainer.name=partial Pretrained=<run
    2>``, tiny epochs on synthetic data.  Run 2 starts from run 1's model (so its encoder is run 1's final one), writes config.yaml with
    its section, last.pth with ``_projector`` and storage.csv, no best.pth, and leaves the encoder's parameters and the last decoder
    blocks as it found them; run 3 starts at epoch 0 with run 2's ``Up_conv3`` weights."""
    import yaml
    save = f"pytest_cli_contrastdecoder_{os.getpid()}"
    r1, r2, r3 = (th.run_dir(f"{save}_{k}") for k in (1, 2, 3))
    try:
        for d in (r1, r2, r3):
            shutil.rmtree(d, ignore_errors=True)
        th.run_main(["Trainer.name=contrast", f"Trainer.save_dir={save}_1", "Trainer.max_epoch=1"] + _TINY)
        res = th.run_main(["Trainer.name=contrastdecoder", f"Pretrained={r1}", f"Trainer.save_dir={save}_2", "Trainer.max_epoch=2"] + _TINY,
                          code=_STAGE, env={"STAGE_FROM": r1})
        assert "stage done: epochs 0 to 1" in res.stdout, res.stdout[-2000:] + res.stderr[-4000:]
        files = set(os.listdir(r2))
        assert {"config.yaml", "last.pth", "storage.csv"} <= files and "best.pth" not in files, files
        cfg = yaml.safe_load(open(os.path.join(r2, "config.yaml")))
        assert cfg["ContrastDecoderParameters"] == {"extract_position": "Up_conv3", "enable_grad_from": "Up5", "ptype": "mlp", "output_size": [4, 4],
                                                    "partition_num": [2, 2], "temperature": 0.07, "base_temperature": 0.07}
        assert "ContrastParameters" not in cfg
        lines = open(os.path.join(r2, "storage.csv")).read().splitlines()
        assert any("contrastive_loss" in h for h in lines[0].split(",")) and len(lines) == 3, lines[:1]
        ck1 = torch.load(os.path.join(r1, "last.pth"), map_location="cpu", weights_only=False)
        ck2 = torch.load(os.path.join(r2, "last.pth"), map_location="cpu", weights_only=False)
        assert {"_model", "_projector", "_optimizer", "_scheduler", "_contrastive_criterion", "_storage", "_buffers"} <= set(ck2)
        assert sorted(ck2["_projector"]) == ["_projector.0.bias", "_projector.0.weight", "_projector.2.bias", "_projector.2.weight"]
        assert ck2["_buffers"]["_cur_epoch"] == 1
        trained = [k for k in ck2["_model"] if k.startswith(TRAINED) and not k.endswith(("running_mean", "running_var", "num_batches_tracked"))]
        assert len(ck2["_optimizer"]["param_groups"][0]["params"]) == len(trained) + 4        # Up5 .. Up_conv3 and the projector only
        m1, m2 = ck1["_model"], ck2["_model"]
        frozen = [k for k in m2 if not k.startswith(TRAINED) and not k.endswith(("running_mean", "running_var", "num_batches_tracked"))]
        assert frozen and all(torch.equal(m1[k], m2[k]) for k in frozen)
        assert all(torch.equal(m1[k], m2[k]) for k in m2 if k.startswith(UNTOUCHED))
        assert all(not torch.equal(m1[k], m2[k]) for k in trained)
        res = th.run_main(["Trainer.name=partial", f"Pretrained={r2}", f"Trainer.save_dir={save}_3", "Trainer.max_epoch=1"] + _TINY,
                          code=_STAGE, env={"STAGE_FROM": r2})
        assert "stage done: epochs 0 to 0" in res.stdout, res.stdout[-2000:] + res.stderr[-4000:]
        ck3 = torch.load(os.path.join(r3, "last.pth"), map_location="cpu", weights_only=False)
        assert ck3["_buffers"]["_cur_epoch"] == 0 and "_projector" not in ck3
    finally:
        for d in (r1, r2, r3):
            shutil.rmtree(d, ignore_errors=True)
