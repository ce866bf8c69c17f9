"""The float64 references of tests/exact_ref.py against torch's own float64 autograd, and every integer input recipe of the GPU file
(test_gpu_exact_integers.py) inside the exact range at every shape it uses -- so a GPU case can never fail on its own precondition.
Runs anywhere (no GPU)."""
import pytest
import torch
import torch.nn.functional as F

import exact_ref as R

F64 = torch.float64
SRC_CASES = {
    # (n, h, w, c0, ups0, c1, ups1, cout)
    "plain_odd": (2, 7, 9, 3, 0, 0, 0, 4),
    "concat": (2, 6, 10, 3, 0, 5, 0, 4),
    "upsample": (2, 6, 10, 4, 1, 0, 0, 3),
    "upsample_concat": (3, 10, 6, 2, 1, 3, 0, 5),
    "both_upsampled": (1, 4, 6, 2, 1, 2, 1, 3),
}


def _sources(name):
    n, h, w, c0, ups0, c1, ups1, cout = SRC_CASES[name]
    x0 = R.ints(f"cpu/{name}/x0", (n, c0, h >> ups0, w >> ups0), -3, 3)
    x1 = R.ints(f"cpu/{name}/x1", (n, c1, h >> ups1, w >> ups1), -3, 3) if c1 else None
    wt = R.ints(f"cpu/{name}/w", (cout, c0 + c1, 3, 3), -2, 2)
    g = R.ints(f"cpu/{name}/g", (n, cout, h, w), -2, 2)
    return x0, ups0, x1, ups1, wt, g


@pytest.mark.parametrize("name", sorted(SRC_CASES))
def test_conv_dgrad_wgrad_references_equal_float64_autograd(name):
    x0, ups0, x1, ups1, wt, g = _sources(name)
    a0 = x0.clone().requires_grad_(True)
    a1 = x1.clone().requires_grad_(True) if x1 is not None else None
    aw = wt.clone().requires_grad_(True)
    up = lambda t, u: F.interpolate(t, scale_factor=2, mode="nearest") if u else t
    xin = up(a0, ups0) if a1 is None else torch.cat((up(a0, ups0), up(a1, ups1)), 1)
    out = F.conv2d(xin, aw, None, 1, 1)
    (out * g).sum().backward()
    # forward: against the definition itself (nine shifted products), not only against F.conv2d
    xp = F.pad(xin.detach(), (1, 1, 1, 1))
    h, w = out.shape[2:]
    direct = sum(torch.einsum("nihw,oi->nohw", xp[:, :, ky:ky + h, kx:kx + w], wt[:, :, ky, kx]) for ky in range(3) for kx in range(3))
    ref, s1, s2 = R.conv_ref(x0, ups0, x1, ups1, wt)
    assert torch.equal(ref, out.detach()) and torch.equal(ref, direct)
    assert torch.equal(s1, direct.sum((0, 2, 3))) and torch.equal(s2, (direct * direct).sum((0, 2, 3)))
    # data gradient: per-source slices; an upsampled source receives the 2 x 2 sums of its slice
    d = R.dgrad_ref(g, wt, x0.shape[1])
    c0 = x0.shape[1]
    chans = (slice(0, c0), slice(c0, None))
    for src, ups, grad in ((0, ups0, a0.grad), (1, ups1, None if a1 is None else a1.grad)):
        if grad is not None:
            assert torch.equal(d["pooled"][:, chans[src]] if ups else d["slices"][src], grad)
    assert torch.equal(torch.cat(d["slices"], 1), d["full"]) and (d["pooled"] is None) == bool(g.shape[2] % 2 or g.shape[3] % 2)
    # weight gradient, both formulations
    assert torch.equal(R.wgrad_ref(x0, ups0, x1, ups1, g), aw.grad)
    assert torch.equal(R.wgrad_ref(x0, ups0, x1, ups1, g, method="einsum"), aw.grad)


@pytest.mark.parametrize("name", ["c16_16_16", "gen_24_32", "gen_cat_32_32_32", "gen_up_64_32", "sub_tile_gen"])
def test_the_two_weight_gradient_formulations_agree_on_gpu_cases(name):
    x0, x1, g, gw, _ = R.wgrad_case(name)
    ups0 = R.WGRAD_CASES[name][4]
    assert torch.equal(gw, R.wgrad_ref(x0, ups0, x1, 0, g, method="einsum"))


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("pool,dual", [(False, False), (True, False), (True, True), (False, True)])
def test_bn_backward_reference_equals_float64_autograd_without_ties(training, pool, dual):
    n, c, h, w = 4, 5, 6, 8
    gen = torch.Generator().manual_seed(11)
    raw = torch.randn(n, c, h, w, dtype=F64, generator=gen).requires_grad_(True)      # continuous data: no ties, no exact zeros
    gamma = (1 + 0.3 * torch.randn(c, dtype=F64, generator=gen)).requires_grad_(True)
    beta = (0.2 * torch.randn(c, dtype=F64, generator=gen)).requires_grad_(True)
    rm, rv = 0.1 * torch.randn(c, dtype=F64, generator=gen), 1 + torch.rand(c, dtype=F64, generator=gen)
    gy = torch.randn(n, c, h, w, dtype=F64, generator=gen)
    gpool = torch.randn(n, c, h // 2, w // 2, dtype=F64, generator=gen) if pool else None
    gy2 = torch.randn(2, c, h, w, dtype=F64, generator=gen) if dual else None
    eps = 1e-5
    y = F.relu(F.batch_norm(raw, None if training else rm, None if training else rv, gamma, beta, training, 0.1, eps))
    obj = (y * gy).sum()
    if pool:
        obj = obj + (F.max_pool2d(y, 2, 2) * gpool).sum()
    if dual:
        obj = obj + (y[1:3] * gy2).sum()
    obj.backward()
    with torch.no_grad():
        mean = raw.mean((0, 2, 3)) if training else rm
        var = raw.var((0, 2, 3), unbiased=False) if training else rv
        invstd = (var + eps).rsqrt()
        scale = gamma * invstd
        saved = torch.stack((mean, invstd, scale, beta - mean * scale))
        ref = R.bn_bwd_ref(raw.detach(), gy, gpool, gy2, (1, 3), gamma.detach(), saved, training)
    torch.testing.assert_close(ref["graw"], raw.grad, rtol=1e-10, atol=1e-12)
    torch.testing.assert_close(ref["ggamma"], gamma.grad, rtol=1e-10, atol=1e-12)
    torch.testing.assert_close(ref["gbeta"], beta.grad, rtol=1e-10, atol=1e-12)
    coef = R.bwd_coef_ref(gamma.detach(), saved, ref["ggamma"], ref["gbeta"], n * h * w, training)
    v = lambda r: coef[r].view(1, -1, 1, 1)
    if not pool and not dual:       # the loader's form of the same tensor
        loaded = (ref["y"] > 0) * v(3) * gy + v(4) + v(5) * (raw.detach() - v(2))
        torch.testing.assert_close(loaded, raw.grad, rtol=1e-10, atol=1e-12)


def test_bn_backward_reference_routes_tied_maxima_like_max_pool2d():
    """On tied data (integers in {-2..2}, identity coefficients) the pooled gradient must land where torch's own max_pool2d backward
    puts it: the first maximum of each window in scan order; and a window of zeros passes nothing (y == 0 is masked)."""
    raw = R.ints("cpu/ties/raw", (3, 4, 8, 10), -2, 2)
    gpool = R.ints("cpu/ties/gpool", (3, 4, 4, 5), 1, 3)        # strictly positive: a misrouted gradient cannot cancel
    c = raw.shape[1]
    saved = torch.stack((torch.zeros(c, dtype=F64), torch.ones(c, dtype=F64), torch.ones(c, dtype=F64), torch.zeros(c, dtype=F64)))
    ref = R.bn_bwd_ref(raw, None, gpool, None, None, torch.ones(c, dtype=F64), saved, False)
    a = raw.clone().requires_grad_(True)
    (F.max_pool2d(F.relu(a), 2, 2) * gpool).sum().backward()
    assert torch.equal(ref["dz"], a.grad) and torch.equal(ref["graw"], a.grad)
    y = F.relu(raw)
    _, idx = F.max_pool2d(y, 2, 2, return_indices=True)
    win = y.unfold(2, 2, 2).unfold(3, 2, 2).reshape(3, 4, 4, 5, 4)                      # window corners in scan order
    first = (win == win.max(-1, keepdim=True).values).to(torch.int64).argmax(-1)       # argmax of a 0/1 tensor: the first 1
    hh, ww = torch.meshgrid(torch.arange(4), torch.arange(5), indexing="ij")
    assert torch.equal(idx, (2 * hh + first // 2) * 10 + 2 * ww + first % 2)
    assert int((win.max(-1).values == win.min(-1).values).sum()) >= 16                  # the data does hold fully tied windows (of 240)


def test_round_to_is_one_rounding_to_nearest_even():
    t = torch.tensor([257.0, 258.0, 259.0, 1.00390625, 1.01171875, -3.0, 2049.0, 2051.0], dtype=F64)
    assert R.round_to(t, torch.bfloat16).tolist() == [256.0, 258.0, 260.0, 1.0, 1.015625, -3.0, 2048.0, 2048.0]
    assert R.round_to(t, torch.float16).tolist()[-2:] == [2048.0, 2052.0]
    assert torch.equal(R.round_to(t, torch.float32), t)
    with pytest.raises(AssertionError):
        R.round_to(torch.tensor([1.0 + 2.0 ** -30], dtype=F64), torch.bfloat16)
    with pytest.raises(AssertionError):
        R.assert_exact_range(torch.tensor([257.0], dtype=F64), torch.bfloat16)
    with pytest.raises(AssertionError):
        R.assert_exact_range(torch.tensor([3.0], dtype=F64), torch.float32, abs_sum=2.0 ** 24)
    assert R.quantum_of(torch.tensor([0.75, 3.0], dtype=F64)) == 0.25


# ---- every recipe of the GPU file inside the exact range, at every shape and storage type it uses
@pytest.mark.parametrize("name", sorted(R.FWD_CASES))
def test_forward_recipes_are_in_range(name):
    for dtype in R.FWD_CASES[name][-1]:
        R.fwd_precondition(name, dtype)
    n, h, w, c0, ups0, c1, ups1, cout = R.FWD_CASES[name][:8]
    assert R.conv_streams(torch.bfloat16, c0 + c1, n, h, w) == name.startswith("stream")


@pytest.mark.parametrize("name", sorted(R.STATS_CASES))
def test_statistics_recipes_are_in_range(name):
    for dtype in R.STATS_CASES[name][-1]:
        R.stats_precondition(name, dtype)


@pytest.mark.parametrize("name", sorted(R.STEM_CASES))
def test_stem_recipes_are_in_range(name):
    for dtype in R.HALF:
        R.stem_precondition(name, dtype)


@pytest.mark.parametrize("table,name", [("dgrad", k) for k in sorted(R.DGRAD_CASES)] + [("dual", k) for k in sorted(R.DUAL_CASES)] +
                         [("sumpool", k) for k in sorted(R.SUMPOOL_CASES)])
def test_data_gradient_recipes_are_in_range(table, name):
    dtypes = R.HALF if table == "sumpool" else {"dgrad": R.DGRAD_CASES, "dual": R.DUAL_CASES}[table][name][-1]
    for dtype in dtypes:
        R.dgrad_precondition(table, name, dtype)
    if table == "sumpool":          # the accumulate form adds integers in {-8..8}
        _, _, ref, _ = R.dgrad_case(table, name)
        assert float(ref["pooled"].abs().max()) + 8 <= 256


@pytest.mark.parametrize("name", sorted(R.WGRAD_CASES))
def test_weight_gradient_recipes_are_in_range_and_in_their_split_class(name):
    R.wgrad_precondition(name)
    n, h, w, c0, ups0, c1, cout, _ = R.WGRAD_CASES[name]
    ntiles, per, splits = R.wgrad_splits(n, h, w, c0 + c1, cout)
    if name.startswith(("one_tile", "sub_tile")):
        assert ntiles == 1 and splits == 1
    elif name.startswith("few_tiles"):
        assert 1 < ntiles < 256 // per and splits == ntiles
    elif name.startswith("remainder"):
        assert ntiles > splits == 256 // per and ntiles % splits != 0
    elif name == "stream_c16":
        assert (ntiles, splits) == (1024, 256)
    if "c16" in name:
        assert R.wgrad_kernel(torch.bfloat16, c0 + c1, cout) == "c16"
    elif "gen" in name:
        assert R.wgrad_kernel(torch.bfloat16, c0 + c1, cout) == "general"


@pytest.mark.parametrize("shape", sorted(R.C1X1_SHAPES))
def test_logits_head_recipes_are_in_range(shape):
    for cout in R.C1X1_COUTS:
        x, wt, bias, gout, out, gin, gw, gb = R.c1x1_case(shape, cout)
        npix = x.shape[0] * x.shape[2] * x.shape[3]
        R.assert_exact_range(out, torch.float32, 16 * 4 + 5)
        R.assert_exact_range(gin, torch.bfloat16, cout * 4)
        R.assert_exact_range(gw, torch.float32, 4.0 * npix)
        R.assert_exact_range(gb, torch.float32, 2.0 * npix)
    assert (R.C1X1_SHAPES["ragged"][0] * 37 * 53) % 256 != 0 and 2 * 256 * 257 > 512 * 256


@pytest.mark.parametrize("name", sorted(R.BN_CASES))
def test_batchnorm_recipes_are_in_range(name):
    n, h, w, c, training, pool = R.BN_CASES[name]
    if training:
        assert (n * h * w) & (n * h * w - 1) == 0           # power-of-two pixel count: the two means are dyadic
    for variant in ("plain", "dual") + (("pool",) if pool else ()):
        for dtype in R.ALL:
            ref = R.bn_precondition(name, variant, dtype)
    y = ref["y"]
    assert float((y == 0).double().mean()) > 0.2            # many exact zeros ...
    if pool:
        win = y.unfold(2, 2, 2).unfold(3, 2, 2).reshape(n, c, h // 2, w // 2, 4)
        assert float(((win == win.max(-1, keepdim=True).values).sum(-1) > 1).double().mean()) > 0.4      # ... and tied maxima in nearly half of the windows


@pytest.mark.parametrize("name", sorted(R.DGRAD_BN_CASES))
def test_fused_batchnorm_data_gradient_recipes_are_in_range(name):
    for dtype in R.DGRAD_BN_CASES[name][-1]:
        ref = R.dgrad_bn_reference(name, dtype)
        if not R.DGRAD_BN_CASES[name][5]:
            assert ref["quantum"] >= 0.25 and torch.equal(ref["graw_loaded"], ref["bn"]["graw"])      # eval mode: nothing to round
            if "stream" not in name:
                R.dgrad_red_reference(name, dtype)          # (asserts the range of the epilogue reduce's sums)
    n, h, w, k, cs = R.DGRAD_BN_CASES[name][:5]
    assert R.conv_streams(torch.bfloat16, k, n, h, w) == ("stream" in name) and ("pool_" not in name or (cs > 32 and h % 2 == 0 and w % 2 == 0))


def test_every_built_tile_shape_has_a_case():
    """The tiled kernel is built with the shapes csrc/conv.h tiled_shape() can return and no others (tiled_shape_built): 14 for 16-bit
    storage, 4 for fp32.  A shape that went missing is a run-time error, so each one is selected by a plain case (forward, statistics or
    pooled table) and by a fused case (DGRAD_BN_CASES).  Shape = (fp32, channels per block, tile width, tile height, pooled)."""
    built = {(False, cot, tw, th, False) for cot in (16, 32) for tw in (16, 32) for th in (8, 16)}
    built |= {(False, 64, tw, 16, False) for tw in (16, 32)} | {(False, 64, tw, th, True) for tw in (16, 32) for th in (8, 16)}
    built |= {(True, cot, tw, 16, False) for cot in (16, 32) for tw in (16, 32)}
    shape = lambda d, h, w, cout, pool=False: (d == torch.float32,) + R.tiled_shape(d, h, w, cout, pool) + (pool,)
    plain, fused = set(), set()
    for n, h, w, c0, _, c1, _, cout, _, _, types in R.FWD_CASES.values():
        plain |= {shape(d, h, w, cout) for d in types if not R.conv_streams(d, c0 + c1, n, h, w)}
    for n, h, w, cin, cout, types in R.STATS_CASES.values():
        plain |= {shape(d, h, w, cout) for d in types if not R.conv_streams(d, cin, n, h, w)}
    for n, h, w, k, cs, _ in R.SUMPOOL_CASES.values():
        plain |= {shape(d, h, w, cs, True) for d in R.HALF if not R.conv_streams(d, k, n, h, w)}
    for name, (n, h, w, k, cs, _, types) in R.DGRAD_BN_CASES.items():
        fused |= {shape(d, h, w, cs) for d in types if not R.conv_streams(d, k, n, h, w)}
        fused |= {shape(d, h, w, cs, True) for d in types if "pool_" in name and d in R.HALF}
    assert plain == built and fused == built


def test_mover_loader_and_forward_recipes_are_in_range():
    """The recipes of the remaining GPU tests: sum-pool, axpy, cast-pad, the weight gradient's BatchNorm loader and its channel slice,
    and the BatchNorm forward."""
    for shape in R.SUMPOOL2X2_SHAPES:
        x, pre, want = R.sumpool2x2_case(shape)
        R.assert_exact_range(want + pre, torch.bfloat16, 40)
    for vec in (4, 8):
        for numel in R.axpy_sizes(vec):
            a, b = R.axpy_case(numel)
            R.assert_exact_range(a + b, torch.bfloat16)
        assert R.axpy_sizes(vec)[1] // vec > 8192 * 256
    for cin in (1, 3):
        img = R.cast_pad_case(cin)
        assert torch.equal(R.round_to(img, torch.float16), img) and not torch.equal(R.round_to(img, torch.bfloat16), img)
    for name in R.WGRAD_BN_NAMES:
        R.wgrad_bn_case(name)
    R.slice_case()
    for case in R.BN_FWD_CASES:
        for dtype in R.ALL:
            R.bn_fwd_case(case, dtype)
    n, h, w = R.C1X1_FWD_LOOPING
    assert n * h * w > 4096 * 256


@pytest.mark.parametrize("name", sorted(R.LOADER_CASES))
def test_batchnorm_loader_recipes_are_in_range(name):
    for dtype in R.LOADER_CASES[name][-1]:
        R.loader_precondition(name, dtype)
    kind, n, h, w, k = R.LOADER_CASES[name][:5]
    if kind == "dgrad":
        assert R.conv_streams(torch.bfloat16, k, n, h, w) == ("stream" in name)
