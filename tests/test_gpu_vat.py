"""GPU: virtual adversarial training (``Trainer.name=vat``) -- the stem's data-gradient kernel (integer-exact
against float64, and against the generic path), the frozen-statistics BatchNorm forward in every variant, the L2 perturbation and the
counter-based normal generator, ``VATLoss`` against the wheel's own run (tests/golden/vat.npz), the direction pass's lack of side
effects, the epocher against the same composition on the oracle, and the CLI."""
import os
import random
import shutil
import sys
from functools import partial

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import synth  # noqa: E402
import trainer_harness as th  # noqa: E402
import vat_ref  # noqa: E402
from oracle import losses as OL  # noqa: E402
from oracle import unet as OU  # noqa: E402
from trainer_harness import DEV, FEATURES  # noqa: E402

pytestmark = pytest.mark.gpu
T = torch.from_numpy
DTYPES = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16}
U24 = 2.0 ** -24          # half an ulp of float32, relative


_dump = partial(th.error_dump, "vat")          # the numbers DESIGN.md section 23 quotes


def _nhwc(t, dtype=None):
    t = t.to(DEV) if dtype is None else t.to(device=DEV, dtype=dtype)
    return t.contiguous(memory_format=torch.channels_last)


# ---------------------------------------------------------------------------------------------------------------- 1. the stem's data gradient
COUT = 16
STEM_SHAPES = [(3, 37, 53), (1, 5, 300), (2, 16, 1022)]      # odd, no multiple of the block; wider than one 256-lane chunk; the maximum width


def _integers(shape, seed):
    """graw in {-1, 0, 1} and w in {-1, 0, 1}: every product and every partial sum of the 144 terms is an integer of magnitude <= 144,
    exact in bf16 (8 significant bits), fp16 and fp32 -- in any order of summation."""
    g = torch.Generator().manual_seed(seed)
    n, h, w = shape
    return torch.randint(-1, 2, (n, COUT, h, w), generator=g).double(), torch.randint(-1, 2, (COUT, 1, 3, 3), generator=g).double()


def _generic(graw, weight):
    from miseg_amd import unet_ops
    return unet_ops.stem_dgrad_generic(graw, weight.to(DEV).float().contiguous(), unet_ops.vec_of(graw.dtype))


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("shape", STEM_SHAPES)
def test_stem_dgrad_is_integer_exact(shape, dtype):
    """``miseg_conv3x3_stem_dgrad`` on small integers equals float64 ``conv_transpose2d`` on the CPU bit for bit."""
    from miseg_amd import ops
    graw, w = _integers(shape, 100 + shape[2])
    ref = F.conv_transpose2d(graw, w, padding=1)
    assert ops.stem_dgrad_supported(DTYPES[dtype], COUT, shape[2])
    got = ops.stem_dgrad(_nhwc(graw, DTYPES[dtype]), w.float().to(DEV))
    assert got.dtype == torch.float32 and got.shape == ref.shape and got.is_contiguous()
    assert torch.equal(got.cpu().double(), ref)
    assert torch.equal(ops.stem_dgrad(_nhwc(graw, DTYPES[dtype]), w.float().to(DEV)), got)          # two calls, the same bits


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_rows_of_1023_pixels_are_refused_and_served_by_the_generic_path(dtype):
    """[1, 3, 1023]: one pixel more than the kernel's row registers hold.  The query says no, the entry point refuses without launching,
    and the generic path -- the streaming / tiled convolution over the dgrad-packed, channel-padded weight -- gives the exact integers
    (they are representable in the storage type) in channel 0 and zeros in the padded channels."""
    from miseg_amd import _cabi, ops
    shape = (1, 3, 1023)
    graw, w = _integers(shape, 7)
    ref = F.conv_transpose2d(graw, w, padding=1)
    assert not ops.stem_dgrad_supported(DTYPES[dtype], COUT, 1023) and ops.stem_dgrad_supported(DTYPES[dtype], COUT, 1022)
    gd = _nhwc(graw, DTYPES[dtype])
    with pytest.raises(_cabi.MisegError, match="stem_dgrad"):
        ops.stem_dgrad(gd, w.float().to(DEV))
    full = _generic(gd, w)
    assert full.dtype == DTYPES[dtype] and full.shape[1] == (4 if dtype == "float32" else 8)
    assert torch.equal(full[:, :1].cpu().double(), ref)
    assert not bool(full[:, 1:].any())


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_stem_dgrad_equals_the_generic_path_on_random_data(dtype):
    """Random ``graw`` (rounded to the storage type) and weights at [3, 37, 53].  Both paths multiply the same rounded operands exactly
    and add 144 products in fp32, in different orders; the generic path then rounds its result to the storage type.  So they differ by
    at most one rounding of the result to the storage type (half an ulp: 2^-8 of the value for bf16's 8 significant bits, 2^-11 for
    fp16's 11, nothing for fp32) plus, on either
    side, the error of a 144-term fp32 sum, 144 * 2^-24 * sum |terms|."""
    from miseg_amd import ops
    dt = DTYPES[dtype]
    g = torch.Generator().manual_seed(5)
    graw = torch.randn(3, COUT, 37, 53, generator=g).to(dt)
    w = torch.randn(COUT, 1, 3, 3, generator=g)
    got = ops.stem_dgrad(_nhwc(graw), w.to(DEV)).cpu().double()
    gen = _generic(_nhwc(graw), w)[:, :1].cpu().double()
    wr = w.to(dt).double()
    ref = F.conv_transpose2d(graw.double(), wr, padding=1)
    mag = F.conv_transpose2d(graw.double().abs(), wr.abs(), padding=1)
    sum_err = 144 * U24 * mag
    half_ulp = {"float32": 0.0, "bfloat16": 2.0 ** -8, "float16": 2.0 ** -11}[dtype]
    err = {"kernel_vs_float64": float(((got - ref).abs() / mag).max()), "generic_vs_float64": float(((gen - ref).abs() / mag).max()),
           "kernel_vs_generic": float(((got - gen).abs() / mag).max())}
    print("stem dgrad random", dtype, err)
    _dump(f"stem_dgrad_random_{dtype}", err)
    assert bool(((got - ref).abs() <= sum_err).all()), err
    assert bool(((got - gen).abs() <= half_ulp * ref.abs() + 2 * sum_err + (6e-8 if dtype == "float16" else 0.0)).all()), err


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("width", [48, 1023])
def test_image_gradient_through_the_stem_layer(dtype, width, monkeypatch):
    """``conv_bn_relu`` on ``stem_input(image)`` with an image that requires a gradient: the gradient reaches the image -- through the
    kernel at width 48, through the generic path at width 1023 and, with the switch off, at width 48 too -- and the two paths agree
    to the storage type's rounding (see the random-data test).  Asserted from the entry points that ran."""
    from miseg_amd import unet_ops
    dt = DTYPES[dtype]
    g = torch.Generator().manual_seed(3)
    image = torch.rand(2, 1, 6, width, generator=g).to(DEV)
    weight = (torch.randn(16, 1, 3, 3, generator=g) * 0.5).to(DEV).requires_grad_()
    gamma, beta = torch.ones(16, device=DEV).requires_grad_(), torch.zeros(16, device=DEV).requires_grad_()
    gy = _nhwc(torch.randn(2, 16, 6, width, generator=g), dt)
    seen = []
    real = unet_ops.call
    monkeypatch.setattr(unet_ops, "call", lambda name, *a, **k: (seen.append(name), real(name, *a, **k))[1])
    from miseg_amd import ops
    real_ops = ops.call
    monkeypatch.setattr(ops, "call", lambda name, *a, **k: (seen.append(name), real_ops(name, *a, **k))[1])

    def run(kernel):
        monkeypatch.setattr(unet_ops, "_STEM_DGRAD", kernel)
        del seen[:]
        img = image.clone().requires_grad_()
        rm, rv, nbt = torch.zeros(16, device=DEV), torch.ones(16, device=DEV), torch.zeros((), dtype=torch.long, device=DEV)
        y, _ = unet_ops.conv_bn_relu(unet_ops.stem_input(img, dt), None, weight, gamma, beta, rm, rv, nbt, True)
        (gi,) = torch.autograd.grad(y, img, gy)
        assert gi.shape == img.shape and gi.dtype == torch.float32
        return gi, list(seen)
    fast, names_fast = run(True)
    slow, names_slow = run(False)
    assert ("miseg_conv3x3_stem_dgrad" in names_fast) == (width <= 1022), names_fast
    assert "miseg_conv3x3_stem_dgrad" not in names_slow and "miseg_conv3x3_fwd" in names_slow, names_slow
    assert torch.isfinite(fast).all() and float(fast.abs().max()) > 0
    # one rounding of the result to the storage type and two 144-term fp32 sums (the random-data test has the exact bound): fp32
    # 2 * 144 * 2^-24 = 1.7e-5 of sum |terms|, itself a few times the largest entry; bf16 one ulp, 2^-7, of the largest entry
    tol = {"float32": 1e-4, "bfloat16": 2.0 ** -7}[dtype]
    assert float((fast - slow).abs().max()) <= tol * float(slow.abs().max()), float((fast - slow).abs().max() / slow.abs().max())


def test_three_channel_images_take_the_generic_data_gradient():
    """Images with more than one channel: the padded operand's gradient from the generic path, its real channels kept -- against
    float64 autograd on the CPU (fp32 storage; a 27-term sum per output feeds BatchNorm: 1e-4 of the largest entry)."""
    from miseg_amd import unet_ops
    g = torch.Generator().manual_seed(9)
    image = torch.rand(2, 3, 9, 20, generator=g)
    weight, gy = torch.randn(8, 3, 3, 3, generator=g) * 0.3, torch.randn(2, 8, 9, 20, generator=g)
    img64 = image.double().requires_grad_()
    raw = F.conv2d(img64, weight.double(), padding=1)
    y = F.relu(F.batch_norm(raw, None, None, torch.ones(8, dtype=torch.float64), torch.zeros(8, dtype=torch.float64), True, 0.1, 1e-5))
    (ref,) = torch.autograd.grad(y, img64, gy.double())
    img = image.to(DEV).requires_grad_()
    rm, rv, nbt = torch.zeros(8, device=DEV), torch.ones(8, device=DEV), torch.zeros((), dtype=torch.long, device=DEV)
    out, _ = unet_ops.conv_bn_relu(unet_ops.stem_input(img, torch.float32), None, weight.to(DEV).requires_grad_(), torch.ones(8, device=DEV),
                                   torch.zeros(8, device=DEV), rm, rv, nbt, True)
    (got,) = torch.autograd.grad(out, img, _nhwc(gy))
    assert got.shape == image.shape
    assert float((got.cpu().double() - ref).abs().max()) <= 1e-4 * float(ref.abs().max())


# ---------------------------------------------------------------------------------------------------------------- 2. frozen statistics
FWD_ENTRY = {"acc": "miseg_conv3x3_fwd_acc", "counter": "miseg_conv3x3_bn_fwd", "finalize": "miseg_bn_finalize", "stem": "miseg_conv3x3_stem_fwd"}


def _select(monkeypatch, variant):
    """Make ``conv_bn_relu`` take one forward variant: the accumulator (the default), the last-block counter, the finalize launch."""
    from miseg_amd import unet_ops
    monkeypatch.setattr(unet_ops, "_BN_ACC", variant in ("acc", "stem"))
    monkeypatch.setattr(unet_ops.SYNC_COUNTERS, "enabled", variant == "counter")


def _spy(monkeypatch):
    from miseg_amd import unet_ops
    seen, real = [], unet_ops.call
    monkeypatch.setattr(unet_ops, "call", lambda name, *a, **k: (seen.append(name), real(name, *a, **k))[1])
    return seen


# (the stem kernels serve 16-bit storage: an fp32 stem layer is the accumulator variant of the streaming convolution)
@pytest.mark.parametrize("variant,dtype", [(v, d) for v in ("acc", "counter", "finalize", "stem") for d in ("float32", "bfloat16")
                                           if (v, d) != ("stem", "float32")])
def test_untracked_layer_leaves_the_statistics_and_equals_a_tracked_pass(monkeypatch, variant, dtype):
    """One ``conv_bn_relu`` layer at [3, *, 32, 48] under ``bn_untracked()``: running mean, running variance and the batch counter keep
    their bits; output, pooled output and the ``saved`` coefficients equal a tracked pass on the same input bit for bit; the tracked
    pass does move the three.  Every forward variant; which one ran is read from the entry points called."""
    from miseg_amd import unet_ops
    dt = DTYPES[dtype]
    _select(monkeypatch, variant)
    seen = _spy(monkeypatch)
    g = torch.Generator().manual_seed(11)
    cin = 1 if variant == "stem" else 16
    x = torch.rand(3, cin, 32, 48, generator=g).to(DEV)
    weight = (torch.randn(16, cin, 3, 3, generator=g) * 0.2).to(DEV).requires_grad_()
    gamma, beta = (1 + 0.1 * torch.randn(16, generator=g)).to(DEV).requires_grad_(), (0.1 * torch.randn(16, generator=g)).to(DEV).requires_grad_()
    rm0, rv0 = torch.randn(16, generator=g).to(DEV), (1 + torch.rand(16, generator=g)).to(DEV)

    def run(untracked):
        rm, rv, nbt = rm0.clone(), rv0.clone(), torch.full((), 5, dtype=torch.long, device=DEV)
        x0 = unet_ops.stem_input(x, dt) if variant == "stem" else _nhwc(x, dt)
        del seen[:]
        if untracked:
            with unet_ops.bn_untracked():
                y, pooled = unet_ops.conv_bn_relu(x0, None, weight, gamma, beta, rm, rv, nbt, True, want_pool=True)
        else:
            y, pooled = unet_ops.conv_bn_relu(x0, None, weight, gamma, beta, rm, rv, nbt, True, want_pool=True)
        saved = y.grad_fn.saved_tensors[6]
        return y, pooled, saved, rm, rv, nbt, list(seen)
    yu, pu, su, rmu, rvu, nbtu, names_u = run(True)
    yt, pt, st, rmt, rvt, nbtt, names_t = run(False)
    assert FWD_ENTRY[variant] in names_u and names_u == names_t, (variant, names_u, names_t)
    if variant != "stem":
        assert "miseg_conv3x3_stem_fwd" not in names_u
    if variant in ("counter", "finalize"):
        assert "miseg_conv3x3_fwd_acc" not in names_u and "miseg_bn_relu_fwd_acc" not in names_u
    if variant == "counter":
        assert "miseg_bn_finalize" not in names_u
    assert torch.equal(rmu, rm0) and torch.equal(rvu, rv0) and int(nbtu) == 5
    assert torch.equal(yu, yt) and torch.equal(pu, pt) and torch.equal(su, st)
    assert not torch.equal(rmt, rm0) and not torch.equal(rvt, rv0) and int(nbtt) == 6
    assert torch.isfinite(su).all() and float(yu.float().abs().max()) > 0


def test_untracked_does_not_touch_evaluation_mode():
    from miseg_amd import unet_ops
    g = torch.Generator().manual_seed(2)
    x = _nhwc(torch.rand(2, 16, 8, 8, generator=g))
    weight = (torch.randn(16, 16, 3, 3, generator=g) * 0.2).to(DEV)
    rm, rv, nbt = torch.randn(16, generator=g).to(DEV), (1 + torch.rand(16, generator=g)).to(DEV), torch.zeros((), dtype=torch.long, device=DEV)
    args = (x, None, weight, torch.ones(16, device=DEV), torch.zeros(16, device=DEV), rm, rv, nbt, False)
    with unet_ops.bn_untracked():
        a, _ = unet_ops.conv_bn_relu(*args)
    b, _ = unet_ops.conv_bn_relu(*args)
    assert torch.equal(a, b) and int(nbt) == 0


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_float_statistics_context_selects_the_finalize_path(monkeypatch, dtype):
    """``bn_float_statistics()``: the layer's forward takes the float partial sums (``miseg_conv3x3_fwd`` + ``miseg_bn_finalize``)
    instead of the fixed-point accumulators, for the forwards inside the block only; ``VATLoss`` runs all its passes that way.  The
    two paths agree to the statistics' rounding (fp32 storage: 1e-5 of the largest output; bf16: one ulp, 2^-7)."""
    from miseg_amd import unet_ops
    seen = _spy(monkeypatch)
    g = torch.Generator().manual_seed(12)
    x = _nhwc(torch.rand(3, 16, 32, 48, generator=g), DTYPES[dtype])
    weight = (torch.randn(16, 16, 3, 3, generator=g) * 0.2).to(DEV)
    args = lambda: (x, None, weight, torch.ones(16, device=DEV), torch.zeros(16, device=DEV), torch.zeros(16, device=DEV),  # noqa: E731
                    torch.ones(16, device=DEV), torch.zeros((), dtype=torch.long, device=DEV), True)
    with unet_ops.bn_float_statistics():
        a, _ = unet_ops.conv_bn_relu(*args())
    inside = list(seen)
    del seen[:]
    b, _ = unet_ops.conv_bn_relu(*args())
    assert "miseg_bn_finalize" in inside and "miseg_conv3x3_fwd_acc" not in inside, inside
    assert "miseg_conv3x3_fwd_acc" in seen and "miseg_bn_finalize" not in seen, seen
    tol = 1e-5 if dtype == "float32" else 2.0 ** -7
    assert float((a.float() - b.float()).abs().max()) <= tol * float(b.float().abs().max())
    model = _unet(dtype, 13)
    del seen[:]
    from deepclustering2.utils.VAT import VATLoss
    VATLoss()(model, T(synth.uniform("vat/x", (3, 1, 32, 48))).to(DEV), seed=1)
    assert seen.count("miseg_bn_finalize") == 3 * 22 and "miseg_conv3x3_fwd_acc" not in seen and "miseg_bn_relu_fwd_acc" not in seen, sorted(set(seen))


def _unet(dtype, seed):
    return th.unet(dtype, seed).train()


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("variant", ["acc", "counter", "finalize"])
def test_untracked_unet_leaves_every_buffer_and_equals_a_tracked_pass(monkeypatch, variant, dtype):
    """The whole U-Net at [3, 1, 32, 48] in training mode: under ``bn_untracked()`` all 66 BatchNorm buffers keep their bits and the
    logits equal those of the tracked pass that follows, which moves every buffer.  In bf16 the default run also goes through the
    stem kernel."""
    from miseg_amd import unet_ops
    _select(monkeypatch, variant)
    seen = _spy(monkeypatch)
    model = _unet(dtype, 13)
    x = T(synth.uniform("vat/x", (3, 1, 32, 48))).to(DEV)
    before = {k: v.clone() for k, v in model.named_buffers()}
    with torch.no_grad(), unet_ops.bn_untracked():
        a = model(x)
    names = set(seen)
    assert FWD_ENTRY[variant] in names, (variant, sorted(names))
    assert ("miseg_conv3x3_stem_fwd" in names) == (variant == "acc" and dtype == "bfloat16"), sorted(names)
    for k, v in model.named_buffers():
        assert torch.equal(v, before[k]), k
    with torch.no_grad():
        b = model(x)
    assert torch.equal(a, b) and torch.isfinite(a).all()
    moved = [k for k, v in model.named_buffers() if not torch.equal(v, before[k])]
    assert len(moved) == len(before) == 66, (len(moved), len(before))


# ---------------------------------------------------------------------------------------------------------------- 3. l2_perturb
@pytest.mark.parametrize("m", [1, 1023, 48 * 48 + 1])
@pytest.mark.parametrize("n", [1, 3])
def test_l2_perturb_against_float64(n, m):
    """d = g / ||g||, r = scale * d, out = x + r per sample.  The norm is a double sum rounded once to fp32 (relative 2^-24), the
    division rounds once more, the product and the sum once each: |d - d64| <= 3 * 2^-24 |d64|, |r - r64| <= 4 * 2^-24 |r64|,
    |out - out64| <= 4 * 2^-24 |r64| + 2^-24 |out64| (half-ulp roundings; the first-order terms, doubled for the second order)."""
    from miseg_amd import ops
    gen = torch.Generator().manual_seed(10 * n + m)
    g, x = torch.randn(n, m, generator=gen) * 3, torch.rand(n, m, generator=gen)
    scale = torch.tensor([2.5, 0.25, 10.0][:n])
    out, r, d, flag = ops.l2_perturb(g.to(DEV), x.to(DEV), scale.to(DEV), want_r=True, want_d=True)
    out2, r2, d2, flag2 = ops.l2_perturb(g.to(DEV), x.to(DEV), scale.to(DEV), want_r=True, want_d=True)
    assert torch.equal(out, out2) and torch.equal(r, r2) and torch.equal(d, d2)          # two calls, the same bits
    assert int(flag) == 0 and int(flag2) == 0
    d64 = g.double() / g.double().norm(dim=1, keepdim=True)
    r64 = scale.double().view(-1, 1) * d64
    out64 = x.double() + r64
    assert bool(((d.cpu().double() - d64).abs() <= 2 * 3 * U24 * d64.abs()).all())
    assert bool(((r.cpu().double() - r64).abs() <= 2 * 4 * U24 * r64.abs()).all())
    assert bool(((out.cpu().double() - out64).abs() <= 2 * (4 * U24 * r64.abs() + U24 * out64.abs())).all())
    # the outputs are optional: the direction alone, and the perturbed tensor alone, are the same bits
    _, _, d3, _ = ops.l2_perturb(g.to(DEV), None, scale.to(DEV), want_d=True)
    out3, r3, d4, _ = ops.l2_perturb(g.to(DEV), x.to(DEV), scale.to(DEV))
    assert torch.equal(d3, d) and torch.equal(out3, out) and r3 is None and d4 is None


def test_l2_perturb_flags_a_zero_and_a_non_finite_sample_without_writing_nan():
    from miseg_amd import ops
    gen = torch.Generator().manual_seed(4)
    g, x = torch.randn(4, 1, 7, 9, generator=gen), torch.rand(4, 1, 7, 9, generator=gen)
    g[1] = 0.0
    g[3, 0, 2, 2] = float("inf")
    scale = torch.full((4,), 2.0)
    out, r, d, flag = ops.l2_perturb(g.to(DEV), x.to(DEV), scale.to(DEV), want_r=True, want_d=True)
    assert int(flag) == 2
    for t in (out, r, d):
        assert torch.isfinite(t).all()
    for bad in (1, 3):
        assert torch.equal(out[bad].cpu(), x[bad]) and not bool(r[bad].any()) and not bool(d[bad].any())
    for good in (0, 2):
        torch.testing.assert_close(d[good].cpu().double().norm(), torch.tensor(1.0, dtype=torch.float64), rtol=1e-6, atol=0)
    # a flag handed in is added to, not reset
    _, _, _, flag = ops.l2_perturb(g.to(DEV), None, scale.to(DEV), want_d=True, flag=flag)
    assert int(flag) == 4
    from deepclustering2.utils.VAT import _l2_normalize
    with pytest.raises(AssertionError, match="zero or not finite"):
        _l2_normalize(g.to(DEV))
    torch.testing.assert_close(_l2_normalize(g[:1].to(DEV)).cpu(), vat_ref.l2_normalize(g[:1]), rtol=1e-6, atol=0)


# ---------------------------------------------------------------------------------------------------------------- 4. normal_fill
N_DRAWS = 65536


def test_normal_fill_depends_on_seed_and_position_only():
    from miseg_amd import ops
    a = ops.normal_fill(torch.empty(N_DRAWS, device=DEV), 1234)
    assert torch.equal(ops.normal_fill(torch.empty(N_DRAWS, device=DEV), 1234), a)
    assert torch.equal(ops.normal_fill(torch.empty(4, 1, 128, 128, device=DEV), 1234).view(-1), a)      # the shape is not an input
    for k in (1, 2, 3, 1021, 40000):                 # the split need not fall on a block of four
        head, tail = torch.empty(k, device=DEV), torch.empty(N_DRAWS - k, device=DEV)
        ops.normal_fill(head, 1234, 0), ops.normal_fill(tail, 1234, k)
        assert torch.equal(torch.cat([head, tail]), a), k
    b = ops.normal_fill(torch.empty(N_DRAWS, device=DEV), 1235)
    assert not torch.equal(a, b) and float((a == b).float().mean()) < 0.01
    assert torch.isfinite(a).all()


@pytest.mark.parametrize("seed,offset", [(0, 0), (7, 3), ((1 << 40) + 12345, 5), (3, (1 << 34) + 2), (-1, 1)])
def test_philox_words_match_the_python_philox(seed, offset):
    """The 32-bit words under the normals against tests/vat_ref.py (itself pinned to the published known answers in
    test_cpu_vat.py): a seed above 2^32 reaches the second key word, an offset above 2^34 the second counter word."""
    from miseg_amd import ops
    got = ops.philox_words(70, seed, offset, DEV).cpu().numpy().view(np.uint32)
    assert np.array_equal(got, vat_ref.philox_words(seed, offset, 70))


def test_normals_follow_box_muller_of_the_words_and_have_the_moments():
    """u1 and u2 are exact in fp32; logf, sqrtf and the sine / cosine of an angle rounded to fp32 (|error| <= 2 pi 2^-24 = 3.7e-7 on an
    argument below 2 pi, times a radius below 5.8) leave each value within 2e-5 absolute of the float64 map.  Moments over n = 65536:
    |mean| < 5 / sqrt(n), |var - 1| < 5 sqrt(2 / n)."""
    from miseg_amd import ops
    z = ops.normal_fill(torch.empty(N_DRAWS, device=DEV), 99).cpu().double().numpy()
    ref = vat_ref.normals_from_words(vat_ref.philox_words(99, 0, 4096), 0)
    assert np.abs(z[:4096] - ref).max() <= 2e-5, np.abs(z[:4096] - ref).max()
    mean, var = z.mean(), z.var()
    print("normal_fill moments", mean, var)
    assert abs(mean) < 5 / np.sqrt(N_DRAWS) and abs(var - 1) < 5 * np.sqrt(2 / N_DRAWS), (mean, var)


# ---------------------------------------------------------------------------------------------------------------- 5. VATLoss
def _case(g, case):
    shape = tuple(int(v) for v in g["cfg/shape"])
    eps = g[f"{case}/eps"]
    return dict(x=T(synth.uniform("vat/x", shape)), d0=T(synth.normal("vat/d0", shape)), ip=int(g[f"{case}/ip"]),
                eps=float(eps) if eps.ndim == 0 else T(eps).float(), xi=float(g[f"{case}/xi"]), prop_eps=float(g["cfg/prop_eps"]))


def _run_vatloss(model, c):
    from deepclustering2.utils.VAT import VATLoss
    rec = {}
    crit = VATLoss(xi=c["xi"], eps=c["eps"].to(DEV) if torch.is_tensor(c["eps"]) else c["eps"], prop_eps=c["prop_eps"], ip=c["ip"])
    lds, x_adv, r_adv = crit(model, c["x"].to(DEV), d0=c["d0"].to(DEV), record=rec)
    return lds, x_adv, r_adv, rec


def _distances(lds, r_adv, rec, grads, ref):
    """The quantities of tests/golden/make_golden_vat.py::distances against ``ref`` (a dict with the golden file's entries)."""
    out = dict(pred=float((rec["pred"].softmax(1).cpu().double() - ref["pred"]).abs().max() / ref["pred"].abs().max()),
               r_adv=vat_ref.rel_l2_per_sample(r_adv.cpu(), ref["r_adv"]),
               lds=abs(float(lds) - float(ref["lds"])) / abs(float(ref["lds"])),
               grad_norms=max(abs(float(grads[n].double().norm()) - v) / v for n, v in ref["grad_norms"].items()))
    for i, d in enumerate(rec["d"]):
        out[f"d{i}"] = vat_ref.rel_l2_per_sample(d.cpu(), ref["d"][i])
    for n, v in ref["whole"].items():
        out[f"grad/{n}"] = vat_ref.rel_l2(grads[n].cpu(), v)
    return out


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_vatloss_matches_the_wheels_run(golden, case):
    """fp32 U-Net, ``d0`` injected, against what the wheel's ``VATLoss`` produced in float64 (tests/golden/vat.npz): the clean
    prediction, the direction after every normalisation (worst sample's relative L2), ``r_adv``, ``lds`` and the parameter gradients
    of ``lds.backward()`` (every tensor's norm, two whole tensors).

    Bounds.  Each is TEN times the distance at which a torch-float32 evaluation of tests/vat_ref.py lands from its float64 evaluation
    on these very inputs, measured on the CPU by make_golden_vat.py and stored in the file (``own_error/<case>/<quantity>``) -- the
    margin the entmin tests give a kernel over the reference's own error.  One iteration is as stable as a forward pass (directions
    2e-5); the second iteration of case b differentiates at x + 10 d1, where float32 itself lands 3 % from float64, so several of its
    bounds are too wide to fail; case c is case b at xi = 0.1, where float32 is stable over both iterations and the second iteration
    with a tensor ``eps`` is held to 1e-1 in the direction and 4e-4 in ``lds`` (DESIGN.md section 23 has all the columns)."""
    g = golden("vat")
    c = _case(g, case)
    model = _unet("float32", int(g["cfg/model_seed"]))
    lds, x_adv, r_adv, rec = _run_vatloss(model, c)
    assert all(p.grad is None for p in model.parameters())
    lds.backward()
    grads = {n: p.grad for n, p in model.named_parameters()}
    names = [str(n) for n in g[f"{case}/grad_names"]]
    assert sorted(names) == sorted(grads)
    ref = dict(pred=T(g[f"{case}/pred"]), r_adv=T(g[f"{case}/r_adv"]), lds=float(g[f"{case}/lds"]),
               d=[T(g[f"{case}/d{i}"]) for i in range(c["ip"] + 1)], grad_norms=dict(zip(names, (float(v) for v in g[f"{case}/grad_norms"]))),
               whole={str(n): T(g[f"{case}/grad/{n}"]) for n in g["whole"]})
    got = _distances(lds, r_adv, rec, grads, ref)
    own = {k: float(g[f"own_error/{case}/{k}"]) for k in got}
    print(f"vat golden {case}: achieved {got}\n  float32 restatement {own}")
    _dump(f"golden_{case}_float32", {"achieved": got, "float32_restatement": own})
    torch.testing.assert_close(x_adv, c["x"].to(DEV) + r_adv, rtol=0, atol=0)
    radius = (c["eps"] if torch.is_tensor(c["eps"]) else torch.full((3,), c["eps"])) * c["prop_eps"]
    torch.testing.assert_close(r_adv.reshape(3, -1).norm(dim=1).cpu(), radius, rtol=1e-5, atol=0)
    # the tracked pass moved the statistics once, the others not at all
    sd = model.state_dict()
    assert int(sd["Conv1.conv.1.num_batches_tracked"]) == 1
    np.testing.assert_allclose(sd["Conv1.conv.1.running_mean"].cpu().numpy(), g[f"{case}/bn/running_mean"], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(sd["Conv1.conv.1.running_var"].cpu().numpy(), g[f"{case}/bn/running_var"], rtol=1e-4)
    late = [k for k in got if got[k] >= 10 * own[k]]
    assert not late, {k: (got[k], 10 * own[k]) for k in late}


_BF16_REF = {}


def _bf16_reference(g, case):
    """float64 evaluation of the restatement with the bf16 kernels' rounding points (``vat_ref.unet_bf16_rounded``), once per case."""
    if case not in _BF16_REF:
        c = _case(g, case)
        sd = OU.init_state(1, 4, seed=int(g["cfg/model_seed"]))
        keys = OU.trainable_keys(sd)
        for k in sd:
            if sd[k].is_floating_point():
                sd[k] = sd[k].double()
        for k in keys:
            sd[k].requires_grad_()
        eps = c["eps"].double() if torch.is_tensor(c["eps"]) else c["eps"]
        res = vat_ref.vat(vat_ref.oracle_model(sd, bf16=True), c["x"].double(), c["d0"].double(), c["xi"], eps, c["prop_eps"], c["ip"])
        res["lds"].backward()
        whole = [str(n) for n in g["whole"]]
        _BF16_REF[case] = dict(pred=res["pred"].softmax(1), r_adv=res["r_adv"], lds=float(res["lds"].detach()), d=[d.detach() for d in res["d"]],
                               grad_norms={k: float(sd[k].grad.norm()) for k in keys}, whole={n: sd[n].grad.detach() for n in whole})
    return _BF16_REF[case]


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_vatloss_bf16_against_the_bf16_rounded_restatement(golden, case):
    """The same comparison in bf16 storage: the bf16 U-Net against a float64 evaluation of the restatement with the bf16 kernels'
    rounding points, bounds set the same way -- ten times the distance of that restatement's float32 evaluation from its float64 one
    (``own_error_bf16/<case>/<quantity>``, measured on the CPU by make_golden_vat.py).

    What these bounds can and cannot catch.  A randomly initialised 22-layer network amplifies bf16 rounding: the float32 and float64
    evaluations of the SAME rounded network already differ by 5e-2 in the clean probabilities, 20-50 % in the first direction and more
    than 100 % in the second (two unit vectors are at most 2 apart), on every model seed.  Ten times that is above 1 for every direction
    and most gradients, so those assertions cannot fail; they are kept because the issue sets them and the achieved figures are dumped.
    The quantities whose bound CAN fail are ``pred`` (0.46 of the largest probability) and ``lds`` (0.18 / 0.37 / 0.064).  Exact in
    any arithmetic, and asserted tightly: ``x_adv = x + r_adv`` bit for bit, every direction a unit vector, ``||r_adv|| = eps
    prop_eps`` per sample, a finite positive ``lds``, every parameter gradient finite and present."""
    g = golden("vat")
    c = _case(g, case)
    model = _unet("bfloat16", int(g["cfg/model_seed"]))
    lds, x_adv, r_adv, rec = _run_vatloss(model, c)
    assert all(p.grad is None for p in model.parameters())
    lds.backward()
    grads = {n: p.grad for n, p in model.named_parameters()}
    ref = _bf16_reference(g, case)
    assert sorted(ref["grad_norms"]) == sorted(grads)
    got = _distances(lds, r_adv, rec, grads, ref)
    own = {k: float(g[f"own_error_bf16/{case}/{k}"]) for k in got}
    print(f"vat bf16 {case}: achieved {got}\n  float32 bf16-rounded restatement {own}")
    _dump(f"golden_{case}_bfloat16", {"achieved": got, "float32_restatement": own})
    torch.testing.assert_close(x_adv, c["x"].to(DEV) + r_adv, rtol=0, atol=0)
    radius = (c["eps"] if torch.is_tensor(c["eps"]) else torch.full((3,), c["eps"])) * c["prop_eps"]
    torch.testing.assert_close(r_adv.reshape(3, -1).norm(dim=1).cpu(), radius, rtol=1e-5, atol=0)
    for d in rec["d"]:
        torch.testing.assert_close(d.reshape(3, -1).double().norm(dim=1).cpu(), torch.ones(3, dtype=torch.float64), rtol=1e-6, atol=0)
    assert float(lds) > 0 and all(torch.isfinite(v).all() and float(v.abs().max()) > 0 for v in grads.values())
    late = [k for k in got if got[k] >= 10 * own[k]]
    assert not late, {k: (got[k], 10 * own[k]) for k in late}


def test_vatloss_draws_its_direction_from_the_seed():
    """Without ``d0``: the same seed gives the same bits, another seed another direction, and the first recorded direction is the
    normalised ``normal_fill`` of that seed."""
    from deepclustering2.utils.VAT import VATLoss, _l2_normalize
    from miseg_amd import ops
    model = _unet("float32", 13)
    x = T(synth.uniform("vat/x", (3, 1, 32, 48))).to(DEV)
    state = {k: v.clone() for k, v in model.state_dict().items()}
    runs = []
    for seed in (5, 5, 6):
        model.load_state_dict(state)
        rec = {}
        lds, _, r = VATLoss()(model, x, seed=seed, record=rec)
        runs.append((lds.detach().clone(), r, rec["d"][0]))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert not torch.equal(runs[0][1], runs[2][1])
    assert torch.equal(runs[0][2], _l2_normalize(ops.normal_fill(torch.empty_like(x), 5)))


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_direction_pass_has_no_side_effects(dtype, monkeypatch):
    """After ``VATLoss.forward`` and before any ``backward``: every ``param.grad`` is None, the flat gradient buffer keeps its bits, no
    slot is claimed, no weight-gradient kernel ran and the side stream was not used -- while the direction pass did compute a data
    gradient down to the image.  Then ``sup + lds`` backward: the flat buffer holds the SUM of the two users of the weights."""
    from deepclustering2.optim import Adam
    from deepclustering2.utils.VAT import VATLoss
    from miseg_amd import ops, unet_ops
    model = _unet(dtype, 13)
    opt = Adam(model.parameters(), lr=1e-3, weight_decay=1e-5)
    opt.zero_grad()
    flat = opt.flat.flat_grad
    flat.copy_(torch.randn(flat.shape, generator=torch.Generator().manual_seed(1)).to(DEV))
    before = flat.clone()
    seen = []
    real_u, real_o = unet_ops.call, ops.call
    monkeypatch.setattr(unet_ops, "call", lambda name, *a, **k: (seen.append(name), real_u(name, *a, **k))[1])
    monkeypatch.setattr(ops, "call", lambda name, *a, **k: (seen.append(name), real_o(name, *a, **k))[1])
    unet_ops._wgrad_dirty.clear()
    x = T(synth.uniform("vat/x", (3, 1, 32, 48))).to(DEV)
    lds, _, _ = VATLoss(ip=2)(model, x, seed=3)
    torch.cuda.synchronize()
    assert all(p.grad is None for p in model.parameters())
    assert torch.equal(flat, before)
    assert not any(getattr(p, "_miseg_grad_claimed", False) for p in model.parameters())
    assert not unet_ops._wgrad_dirty
    assert not [n for n in seen if "wgrad" in n], sorted(set(seen))
    assert seen.count("miseg_conv3x3_stem_dgrad") == 2, seen.count("miseg_conv3x3_stem_dgrad")
    assert sum(n.startswith("miseg_bn_relu_bwd") for n in seen) == 2 * 22 and seen.count("miseg_conv1x1_bwd") == 2      # 22 layers, twice
    # the parameter backward: f(x_l) and the perturbed pass both use the weights; the flat buffer must hold the sum
    xl = T(synth.uniform("vat/xl", (2, 1, 32, 48))).to(DEV)
    labels = T(synth.integers("vat/yl", (2, 32, 48), 4)).to(DEV)
    model.load_state_dict(OU.init_state(1, 4, seed=13))
    opt.zero_grad()
    sup = ops.softmax_kl(model(xl), labels)
    lds, _, _ = VATLoss()(model, x, seed=3)
    (sup + lds).backward()
    both = {n: p.grad.detach().clone() for n, p in model.named_parameters()}
    # what the optimiser reads: after collect() every slot of the flat buffer holds its parameter's gradient
    opt.flat.collect()
    torch.cuda.synchronize()
    in_place = sum(p.grad.data_ptr() == p._miseg_grad_slot.data_ptr() for p in model.parameters())
    print("second users: gradients living in their flat slot", in_place, "of", len(both))
    for n, p in model.named_parameters():
        o = opt.flat.offset_of(p)
        assert torch.equal(opt.flat.flat_grad[o:o + p.numel()].view_as(p), both[n]), n
    model.load_state_dict(OU.init_state(1, 4, seed=13))
    opt.zero_grad()
    ops.softmax_kl(model(xl), labels).backward()
    first = {n: p.grad.detach().clone() for n, p in model.named_parameters()}
    opt.zero_grad()
    lds, _, _ = VATLoss()(model, x, seed=3)
    lds.backward()
    second = {n: p.grad.detach().clone() for n, p in model.named_parameters()}
    for n in both:
        torch.testing.assert_close(both[n], first[n] + second[n], rtol=1e-5, atol=1e-6 * float(both[n].abs().max()))
        assert float(second[n].abs().max()) > 0, n


# ---------------------------------------------------------------------------------------------------------------- 6. the epocher
EP = dict(H=32, W=48, LB=2, UB=3, NB=2, lr=1e-3, wd=1e-5, weight=1.0, model_seed=13)      # the bounds: tests/test_gpu_step.py's fp32 step


def _loaders():
    H, W, LB, UB, NB = (EP[k] for k in ("H", "W", "LB", "UB", "NB"))
    lab = [(T(synth.uniform(f"vat/ep/lab{i}", (LB, 1, H, W))), T(synth.integers(f"vat/ep/tgt{i}", (LB, 1, H, W), 4))) for i in range(NB)]
    unl = [T(synth.uniform(f"vat/ep/unl{i}", (UB, 1, H, W))) for i in range(NB)]
    return (lab, unl, th.reference_batches([a for a, _ in lab], [b for _, b in lab], LB),
            th.reference_batches(unl, [torch.zeros(UB, 1, H, W, dtype=torch.long)] * NB, UB))


def test_epocher_matches_the_same_composition_on_the_oracle(monkeypatch):
    """Two iterations of ``VATEpocher`` (fp32, LB = 2, UB = 3, 32 x 48) against the oracle U-Net composed the same way: labeled pass
    (tracked), ``vat_ref.vat`` on the unlabeled batch with the direction the library generator draws for the iteration's seed,
    ``sup + weight * lds``, one backward, the oracle's Adam.  Bounds: those of tests/test_gpu_step.py for the fp32 step -- first
    iteration sup_loss 2e-5 and reg_loss 2e-4 relative, Dice 2e-3; two-iteration means 3e-3 / 0.2 / 2e-2 (+5e-3); every weight within
    2.5 lr per step of its start, and moved the way the oracle moved it wherever that moved it by more than 1.2 lr."""
    from deepclustering2.loss import KL_div
    from deepclustering2.optim import Adam
    from miseg_amd import ops
    from semi_seg import epocher as E
    lab, unl, lab_loader, unl_loader = _loaders()
    model = _unet("float32", EP["model_seed"])
    opt = Adam(model.parameters(), lr=EP["lr"], weight_decay=EP["wd"])
    seeds = []
    real_randint = random.randint

    def spy(a, b):
        seeds.append(real_randint(a, b))
        return seeds[-1]
    monkeypatch.setattr(E.random, "randint", spy)
    ep = E.VATEpocher(model, opt, lab_loader, unl_loader, KL_div(verbose=False), EP["weight"], EP["NB"], 0, DEV, feature_position=FEATURES,
                      feature_importance=th.IMPORTANCE)
    per_step = th.keep_records(ep)
    random.seed(78)       # counting up from 77, the first host seed whose direction leaves the float32 oracle within 2e-5 of its float64
    res = ep.run()        # evaluation in iteration 1 (77: 1e-3, a ReLU mask apart); the criterion looks at the oracle alone
    assert ep._step_tape is None and len(seeds) == EP["NB"] and len(per_step) == EP["NB"]
    # ---- the oracle
    sd = OU.init_state(1, 4, seed=EP["model_seed"])
    keys = OU.trainable_keys(sd)
    m, v = [torch.zeros_like(sd[k]) for k in keys], [torch.zeros_like(sd[k]) for k in keys]
    dice = OL.DiceMeter(4, report_axis=[1, 2, 3])
    ref_steps = []
    for i in range(EP["NB"]):
        for k in keys:
            sd[k].requires_grad_(True)
            sd[k].grad = None
        d0 = ops.normal_fill(torch.empty(EP["UB"], 1, EP["H"], EP["W"], device=DEV), seeds[i]).cpu()
        logits = OU.unet_forward(sd, lab[i][0], True, True)[0]
        sup = OL.kl_div(logits.softmax(1), OL.class2one_hot(lab[i][1].squeeze(1), 4))
        out = vat_ref.vat(vat_ref.oracle_model(sd), unl[i], d0)
        (sup + EP["weight"] * out["lds"]).backward()
        ref_steps.append({"sup_loss": float(sup), "reg_loss": float(out["lds"])})
        dice.add(logits.max(1)[1], lab[i][1].squeeze(1), group_name=[f"patient{j:03d}_00" for j in range(EP["LB"])])
        with torch.no_grad():
            grads = [sd[k].grad for k in keys]
            for k in keys:
                sd[k].requires_grad_(False)
            OL.adam_step([sd[k] for k in keys], grads, m, v, i + 1, EP["lr"], weight_decay=EP["wd"])
    print("vat epocher:", per_step, ref_steps)
    _dump("epocher", {"got": per_step, "oracle": ref_steps})
    np.testing.assert_allclose(per_step[0]["sup_loss"], ref_steps[0]["sup_loss"], rtol=2e-5)
    np.testing.assert_allclose(per_step[0]["reg_loss"], ref_steps[0]["reg_loss"], rtol=2e-4, atol=1e-7)
    np.testing.assert_allclose(res["sup_loss"]["mean"], np.mean([s["sup_loss"] for s in ref_steps]), rtol=3e-3)
    np.testing.assert_allclose(res["reg_loss"]["mean"], np.mean([s["reg_loss"] for s in ref_steps]), rtol=0.2, atol=1e-7)
    assert res["reg_weight"]["mean"] == EP["weight"]
    assert set(res) == {"lr", "sup_loss", "reg_loss", "reg_weight", "sup_dice"}
    for k, val in dice.summary().items():
        np.testing.assert_allclose(res["sup_dice"][k], val, rtol=2e-2, atol=5e-3)
    init = OU.init_state(1, 4, seed=EP["model_seed"])
    agree = total = 0
    for k, val in model.state_dict().items():
        if not k.endswith(("weight", "bias")):
            continue
        mine = (val.detach().cpu().double() - init[k].double()).reshape(-1).numpy()
        ref_move = (sd[k].double() - init[k].double()).reshape(-1).numpy()
        sel = np.abs(ref_move) > 1.2 * EP["lr"]
        agree += int((np.sign(mine[sel]) == np.sign(ref_move[sel])).sum())
        total += int(sel.sum())
        assert np.abs(mine).max() <= 2.5 * EP["lr"] * EP["NB"], k
    assert total > 1000 and agree >= 0.97 * total, (agree, total)
    # the running statistics: two tracked passes per iteration (labeled, clean unlabeled), in that order
    got_sd = model.state_dict()
    assert int(got_sd["Conv1.conv.1.num_batches_tracked"]) == int(sd["Conv1.conv.1.num_batches_tracked"]) == 2 * EP["NB"]
    np.testing.assert_allclose(got_sd["Up_conv2.conv.4.running_mean"].cpu().numpy(), sd["Up_conv2.conv.4.running_mean"].numpy(), rtol=2e-2, atol=2e-3)


def test_zero_direction_skips_the_update_and_raises(monkeypatch):
    """A direction of zero norm: the deferred check rides with the iteration's report, the guarded Adam leaves the weights alone, and
    the host raises the reference's AssertionError at the read-back."""
    from deepclustering2.loss import KL_div
    from deepclustering2.optim import Adam
    from miseg_amd import ops
    from semi_seg import epocher as E
    _, _, lab_loader, unl_loader = _loaders()
    model = _unet("float32", EP["model_seed"])
    opt = Adam(model.parameters(), lr=EP["lr"], weight_decay=EP["wd"])
    monkeypatch.setattr(ops, "normal_fill", lambda out, seed, offset=0: out.zero_())
    ep = E.VATEpocher(model, opt, lab_loader, unl_loader, KL_div(verbose=False), 1.0, 1, 0, DEV, feature_position=FEATURES,
                      feature_importance=th.IMPORTANCE)
    opt.zero_grad()                                   # (builds the flat buffers)
    before = opt.flat.flat_param.detach().clone()
    with pytest.raises(AssertionError, match="zero or non-finite norm"):
        ep.run()
    assert torch.equal(opt.flat.flat_param, before)


# ---------------------------------------------------------------------------------------------------------------- 7. the CLI
def test_main_cli_runs_vat_and_its_checkpoint_is_the_partial_trainers(golden):
    """``python semi_seg/main.py Trainer.name=vat``: 2 epochs x 2 batches on the synthetic data (bf16), validation and test every
    epoch; config.yaml, last.pth, a storage CSV with a reg_weight column; the checkpoint's key tree is the partial trainer's plus that
    history.  In a fresh process the ``partial`` trainer runs inference on the vat checkpoint, and a ``vat`` trainer loads the
    checkpoint a ``partial`` trainer wrote (strict)."""
    save = f"pytest_cli_vat_{os.getpid()}"
    run_dir = th.run_dir(save)
    common = ["Trainer.device=cuda", "Trainer.max_epoch=2", "Trainer.num_batches=2", "Data.size=64", "LabeledData.batch_size=2",
              "UnlabeledData.batch_size=3", "Arch.compute_dtype=bfloat16"]
    shutil.rmtree(run_dir, ignore_errors=True)
    try:
        th.run_main(["Trainer.name=vat", "VATParameters.weight=0.5", f"Trainer.save_dir={save}"] + common)
        files = set(os.listdir(run_dir))
        assert {"config.yaml", "last.pth", "storage.csv"} <= files, files
        rows = open(os.path.join(run_dir, "storage.csv")).read().splitlines()
        header = rows[0].split(",")
        assert len(rows) == 3 and any(h.startswith("tra_reg_weight") for h in header) and any(h.startswith("val_") for h in header), header
        for row in rows[1:]:
            for k, val in zip(header, row.split(",")):
                if k.startswith("tra_") and val != "":
                    assert float(val) == float(val) and abs(float(val)) < 1e6, (k, val)
        import yaml
        cfg = yaml.safe_load(open(os.path.join(run_dir, "config.yaml")))
        assert cfg["VATParameters"] == {"weight": 0.5}           # what was given; the rest are the class's defaults
        lines = th.checkpoint_tree(os.path.join(run_dir, "last.pth"))
        mine = th.own_lines_removed(lines, ("_storage/tra_reg_weight",))
        assert any(l.startswith("_storage/tra_reg_weight") for l in lines)
        ref = sorted(str(x) for x in golden("trainer_io")["partial/tree_last_pth"])
        assert mine == ref, (sorted(set(mine) - set(ref))[:12], sorted(set(ref) - set(mine))[:12])
        code = ("import os, sys\n"
                "from semi_seg.main import build_trainer\n"
                "argv = sys.argv[1:]\n"
                "part = build_trainer(['Trainer.name=partial', 'Trainer.save_dir=' + os.environ['VAT_SAVE'] + '_partial'] + argv)\n"
                "res, score = part.inference(os.environ['VAT_CKPT'])\n"
                "assert 0.0 <= score <= 1.0, score\n"
                "part._save_to('last.pth')\n"
                "vat = build_trainer(['Trainer.name=vat', 'Trainer.save_dir=' + os.environ['VAT_SAVE'] + '_back'] + argv)\n"
                "vat.load_state_dict_from_path(os.path.join(str(part._save_dir), 'last.pth'), strict=True)\n"
                "res2, score2 = vat.inference(os.path.join(str(part._save_dir), 'last.pth'))\n"
                "assert score2 == score, (score, score2)\n"
                "print('inference', score)\n")
        res = th.run_main(common, code=code, env={"VAT_CKPT": os.path.join(run_dir, "last.pth"), "VAT_SAVE": save})
        assert "inference" in res.stdout, res.stdout[-2000:] + res.stderr[-4000:]
    finally:
        for suffix in ("", "_partial", "_back"):
            shutil.rmtree(run_dir + suffix, ignore_errors=True)
