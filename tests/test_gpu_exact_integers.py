"""Integer-exact tests of the convolution, weight-gradient, logits-head and BatchNorm kernels (csrc/conv_*.hip, csrc/bn.hip).

The kernels are fed small integers (BatchNorm: dyadic coefficients).  Every operand is exact in bf16, IEEE half and fp32, every
product and partial sum is an integer below 2^24, so the fp32 accumulators hold them exactly in whatever order a kernel adds, and
the HIP result must EQUAL the float64 reference of tests/exact_ref.py at every element: a dropped, duplicated or misplaced pixel,
channel, tap, tile or split changes some integer.  Every comparison below is an equality; each case first asserts, on its reference,
the range precondition that makes equality the right demand (tests/test_cpu_exact_ref.py proves the same on a machine without a GPU).
Every call goes through the C ABI (miseg_amd._cabi); outputs are pre-filled with NaN so that an element nobody writes is seen.

Case -> kernel (csrc/conv_*.hip, csrc/bn.hip; the dispatch predicates are mirrored in exact_ref.py and asserted through the library's
own queries).  16-bit = bf16 and, through the -DMISEG_F16_BUILD twins, IEEE half.
  tiled_* / deep_* (H * W < 64^2)            conv3x3_kernel: 16-row tiles, 16 / 32 / 64-channel slices, 16-wide tiles at W < 32; fp32 always
  pt_remainder_64_64 (16-bit, 100 x 200)     conv3x3_pt_kernel: 8-row tiles, 273 tiles over 137 persistent blocks
  t16x16_* / t8x32_* / t8x16_* (and t16x32 in the fused table): one case per tile shape the library is built with (csrc/conv.h
                                             tiled_shape_built) that no case above selects.  Channels per block, tile width x height:
                                             16-bit  t16x16 (16 x 16, 20 x 20)   16 | 32 | 64, 16 x 16    conv3x3_kernel, 8 waves
                                                     t8x32 (64 x 64, 70 x 66)    16 | 32, 32 x 8          conv3x3_pt_kernel
                                                     t8x16 (256 x 16, 258 x 18)  16 | 32, 16 x 8          conv3x3_pt_kernel
                                             fp32    every size                  16 | 32, 16 | 32 x 16    conv3x3_kernel, 4 waves
                                             pooled (16-bit, Cs = 64): 64 on all four tiles (16-row: conv3x3_kernel, 8 waves; 8-row:
                                             conv3x3_pt_kernel)
  test_eight_row_tiles_under_the_conv_switches  MISEG_CONV_PERSISTENT=0: conv3x3_kernel, 4 waves, on the 8-row shapes (pooled too);
                                             MISEG_CONV_DEPTH=2: conv3x3_pt_kernel<.., DEPTH = 2> (not pooled); a fresh process each
  stream_* (16-bit, Cin <= 32, >= 512 tiles) conv3x3_stream_kernel: NV = 1..4, concat (DU) and upsampled loaders, ragged 250 x 230
  test_data_gradient / _concat_in_one_launch the same three kernels behind pack kind 1, channel slices, two destinations (C1 = 4, 16)
  test_pooled_data_gradient                  stream kernel POOL (+ accumulate), conv3x3_kernel POOL 64 slices, conv3x3_pt_kernel POOL
  statistics cases                           the three kernels' epilogue sums: partial rows and the 2^-20 fixed-point accumulator
  test_stem_kernels                          stem_conv_fwd_kernel, stem_wgrad_kernel + stem_wgrad_sum_kernel, slice_cin_kernel
  c16_* / *_c16 (16-bit)                     conv3x3_wgrad_bf16_c16_kernel;   gen_* / *_gen (16-bit): conv3x3_wgrad_bf16_kernel
  every weight-gradient case in fp32, f32_*  conv3x3_wgrad_kernel<float>;   all of them: wgrad_reduce_kernel
  one_tile / sub_tile / few_tiles / remainder  ntiles = 1, one split per tile, ntiles % splits != 0 (273 over 256, 105 over 64)
  test_weight_gradient_with_the_batchnorm_loader  the BNL = true instance of each weight-gradient kernel
  test_logits_head                           conv1x1_fwd_kernel / conv1x1_bwd_kernel<.., 16, 1|2|3|4|5|8> + sum_parts2_kernel
  test_bn_relu_forward                       bn_relu_fwd_pool_kernel (C / vector a power of two <= 32), bn_relu_fwd_kernel<POOL>
  test_bn_relu_backward                      bn_relu_bwd_reduce_kernel / bn_bwd_apply_kernel <POOL = 0 | 1> (+ gy2, + ACC),
                                             bn_bwd_finalize_kernel, the last-block finish (_sync)
  test_batchnorm_backward_folded_...         reduce + finalize -> bwd_coef; the BNL loaders of conv3x3_kernel and conv3x3_stream_kernel;
                                             evaluation-mode tiled cases: conv3x3_kernel<.., BNL, RED> in its forms BNL, RED and BNL + RED
                                             (4 waves) on every tile shape of 16-bit storage and of fp32, pool_* (16-bit): POOL + BNL
  test_batchnorm_loaders_with_nonzero_...    the BNL loaders of the stream, tiled and all three weight-gradient kernels with P, Q != 0
Not covered here: miseg_bn_relu_bwd_ext, the red_* epilogue of miseg_conv3x3_dgrad_bn on the streaming kernel and in training mode
(their sums are the ones checked above, taken in another kernel's epilogue), and everything that derives invstd through rsqrtf in a
kernel (miseg_bn_finalize, miseg_bn_relu_fwd_acc, miseg_conv3x3_bn_fwd): not exact by design.
"""
import os
import subprocess
import sys

import pytest
import torch

import exact_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64
NAN = float("nan")
# the library's own reading of the switch (csrc/conv.h tiled_persistent()): unset in the suite, set in the children of the last test
PERSISTENT = int(os.environ.get("MISEG_CONV_PERSISTENT", "1") or 0) != 0


def _abi():
    from miseg_amd import _cabi
    return _cabi


def DT(dtype):
    c = _abi()
    return {torch.float32: c.F32, torch.bfloat16: c.BF16, torch.float16: c.F16}[dtype]


def st():
    return torch.cuda.current_stream().cuda_stream


_LIVE = []


def ptr(t):
    """Device address of a tensor for the C ABI.  The tensor is kept alive until the test ends: a temporary handed over as
    `ptr(dev(...))` would otherwise go back to the allocator at once, and a later argument's upload could land in its memory before
    the kernel has run."""
    if t is None:
        return None
    _LIVE.append(t)
    return t.data_ptr()


@pytest.fixture(autouse=True)
def _release_operands():
    yield
    torch.cuda.synchronize()
    _LIVE.clear()


def dev(t64, dtype):
    """NCHW float64 (CPU) -> NHWC tensor [N][H][W][C] of the storage type on the device (exact: the values are small integers)."""
    return None if t64 is None else t64.permute(0, 2, 3, 1).contiguous().to(dtype).to(DEV)


def host(t):
    """NHWC device tensor -> NCHW float64 on the CPU."""
    return t.detach().cpu().to(F64).permute(0, 3, 1, 2)


def f32(t64):
    return t64.to(torch.float32).contiguous().to(DEV)


def nans(shape, dtype):
    return torch.full(tuple(shape), NAN, dtype=dtype, device=DEV)


def scratch(nbytes):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=DEV)


def pack(wt64, dtype, kind=0, ci_begin=0, ci_count=0, cin=None):
    from miseg_amd import packcache
    return packcache._pack_now(f32(wt64), dtype, kind, ci_begin, ci_count if kind else wt64.shape[1], cin=cin)


def pairs(table):
    """(case, storage type) pairs, case-major: the float64 reference of a case is computed once and shared by its storage types."""
    return [pytest.param(k, d, id=f"{k}-{str(d).replace('torch.', '')}") for k in sorted(table) for d in table[k][-1]]


def cdiv(a, b):
    return (a + b - 1) // b


def fixed(acc, scale):
    """int64 fixed-point accumulator entries -> float64 values."""
    return acc.cpu().to(F64) / scale


# =================================================================================================================== a. forward
@pytest.mark.parametrize("name,dtype", pairs(R.FWD_CASES))
def test_forward_convolution(name, dtype):
    """miseg_conv3x3_fwd on random integer inputs and weights: tiled (ragged, 64-channel slices, 16-wide deep tiles), persistent tiled
    (a block count that does not divide the tiles) and streaming kernels; concatenated and upsampled sources on both families."""
    c = _abi()
    n, h, w, c0, ups0, c1, ups1, cout = R.FWD_CASES[name][:8]
    R.fwd_precondition(name, dtype)
    x0, x1, wt, (ref, _, _), _ = R.fwd_case(name)
    dt, cin = DT(dtype), c0 + c1
    parts = c.query("miseg_conv3x3_stats_parts", dt, cin, n, h, w)
    if name.startswith("stream") and dtype != torch.float32:            # the streaming kernel: one row per persistent block
        assert parts == min(n * cdiv(h, 16) * cdiv(w, 32), 512)
    else:                                                               # one tile per row, of the shape the selection rule gives
        _, tw, th = R.tiled_shape(dtype, h, w, cout)
        assert th == (8 if dtype != torch.float32 and h * w >= 64 * 64 else 16) and tw == (32 if w >= 32 else 16)
        assert parts == n * cdiv(h, th) * cdiv(w, tw)
        blocks = c.query("miseg_conv3x3_fwd_parts", dt, cin, n, h, w, cout)
        assert blocks == R.fwd_parts(dtype, cin, n, h, w, cout, PERSISTENT)
        if name.startswith("pt_") and th == 8 and PERSISTENT:          # the persistent form: fewer blocks than tiles, not a divisor
            assert blocks < parts and parts % blocks != 0
    out = nans((n, h, w, cout), dtype)
    xd0, xd1 = dev(x0, dtype), dev(x1, dtype)
    c.call("miseg_conv3x3_fwd", st(), dt, ptr(xd0), c0, ups0, ptr(xd1), c1, ups1, n, h, w, ptr(pack(wt, dtype)), cout, ptr(out), None)
    assert torch.equal(host(out), ref)


@pytest.mark.parametrize("name,dtype", pairs(R.STATS_CASES))
def test_forward_convolution_batchnorm_statistics(name, dtype):
    """The BatchNorm statistics of the convolution's epilogue on a sparse integer input: the partial rows fp32[parts][2][Cout] of
    miseg_conv3x3_fwd, added in float64, and the 2^-20 fixed-point accumulator of miseg_conv3x3_fwd_acc must both equal the reference's
    per-channel sum and sum of squares exactly (whole-tensor sums below 2^24: every partial is exact whatever the block partition)."""
    c = _abi()
    n, h, w, cin, cout, _ = R.STATS_CASES[name]
    R.stats_precondition(name, dtype)
    x, wt, (ref, s1, s2) = R.stats_case(name)
    dt = DT(dtype)
    xd, pk = dev(x, dtype), pack(wt, dtype)
    parts = c.query("miseg_conv3x3_fwd_parts", dt, cin, n, h, w, cout)
    if not R.conv_streams(dtype, cin, n, h, w):
        assert parts == R.fwd_parts(dtype, cin, n, h, w, cout, PERSISTENT)
    if name.startswith("pt_") and dtype != torch.float32 and PERSISTENT:
        assert parts < c.query("miseg_conv3x3_stats_parts", dt, cin, n, h, w)
    out, stats = nans((n, h, w, cout), dtype), nans((parts, 2, cout), torch.float32)
    c.call("miseg_conv3x3_fwd", st(), dt, ptr(xd), cin, 0, None, 0, 0, n, h, w, ptr(pk), cout, ptr(out), ptr(stats))
    assert torch.equal(host(out), ref)
    tot = stats.cpu().to(F64).sum(0)
    assert torch.equal(tot[0], s1) and torch.equal(tot[1], s2)
    assert c.query("miseg_conv3x3_fwd_acc_supported", dt, cin, n, h, w, cout)
    out, acc = nans((n, h, w, cout), dtype), torch.zeros(2 * cout + 1, dtype=torch.int64, device=DEV)
    c.call("miseg_conv3x3_fwd_acc", st(), dt, ptr(xd), cin, 0, None, 0, 0, n, h, w, ptr(pk), cout, ptr(out), ptr(acc))
    assert torch.equal(host(out), ref)
    a = acc.cpu()
    assert torch.equal(a[:cout], (s1 * 2 ** 20).to(torch.int64)) and torch.equal(a[cout:2 * cout], (s2 * 2 ** 20).to(torch.int64))
    assert int(a[2 * cout]) == 0                                        # no block sum failed to fit


@pytest.mark.parametrize("dtype", R.HALF, ids=["bfloat16", "float16"])
@pytest.mark.parametrize("name", sorted(R.STEM_CASES))
def test_stem_kernels(name, dtype):
    """miseg_conv3x3_stem_fwd / _stem_wgrad on the padded 16-bit operand (x_f32 = 0) and on the fp32 image (x_f32 = 1): output,
    accumulator and weight gradient equal the reference AND the matrix-core path on the padded channel vector (miseg_conv3x3_fwd_acc
    with the padded pack, miseg_conv3x3_wgrad + miseg_conv3x3_wgrad_slice)."""
    c = _abi()
    n, h, w, cout = R.STEM_CASES[name]
    R.stem_precondition(name, dtype)
    img, wt, g, (ref, s1, s2), gw_ref = R.stem_case(name)
    dt = DT(dtype)
    xpad = dev(torch.cat((img, torch.zeros(n, 7, h, w, dtype=F64)), 1), dtype)
    ximg = f32(img.permute(0, 2, 3, 1))
    wd, gd = f32(wt), dev(g, dtype)
    want_acc = torch.cat(((s1 * 2 ** 20), (s2 * 2 ** 20), torch.zeros(1, dtype=F64))).to(torch.int64)
    assert c.query("miseg_conv3x3_stem_supported", dt, 1, 8, cout) and c.query("miseg_conv3x3_stem_supported", dt, 1, 1, cout)
    for x, x_f32, cp in ((xpad, 0, 8), (ximg, 1, 1)):
        out, acc = nans((n, h, w, cout), dtype), torch.zeros(2 * cout + 1, dtype=torch.int64, device=DEV)
        c.call("miseg_conv3x3_stem_fwd", st(), dt, ptr(x), x_f32, cp, n, h, w, ptr(wd), 1, cout, ptr(out), ptr(acc))
        assert torch.equal(host(out), ref) and torch.equal(acc.cpu(), want_acc)
        out = nans((n, h, w, cout), dtype)
        c.call("miseg_conv3x3_stem_fwd", st(), dt, ptr(x), x_f32, cp, n, h, w, ptr(wd), 1, cout, ptr(out), None)      # evaluation mode
        assert torch.equal(host(out), ref)
        ws = scratch(c.query("miseg_conv3x3_stem_wgrad_ws_bytes", cout))
        gw = nans((cout, 1, 3, 3), torch.float32)
        c.call("miseg_conv3x3_stem_wgrad", st(), dt, ptr(x), x_f32, cp, n, h, w, ptr(gd), cout, ptr(gw), ptr(ws), ws.numel())
        assert torch.equal(gw.cpu().to(F64), gw_ref)
    # the matrix-core path on the padded operand
    assert c.query("miseg_conv3x3_fwd_acc_supported", dt, 8, n, h, w, cout)
    out, acc = nans((n, h, w, cout), dtype), torch.zeros(2 * cout + 1, dtype=torch.int64, device=DEV)
    c.call("miseg_conv3x3_fwd_acc", st(), dt, ptr(xpad), 8, 0, None, 0, 0, n, h, w, ptr(pack(wt, dtype, cin=8)), cout, ptr(out), ptr(acc))
    assert torch.equal(host(out), ref) and torch.equal(acc.cpu(), want_acc)
    ws = scratch(c.query("miseg_conv3x3_wgrad_ws_bytes", n, h, w, 8, cout))
    gw_pad, gw = nans((cout, 8, 3, 3), torch.float32), nans((cout, 1, 3, 3), torch.float32)
    c.call("miseg_conv3x3_wgrad", st(), dt, ptr(xpad), 8, 0, None, 0, 0, n, h, w, ptr(gd), cout, ptr(gw_pad), ptr(ws), ws.numel())
    c.call("miseg_conv3x3_wgrad_slice", st(), ptr(gw_pad), cout, 8, 1, ptr(gw))
    assert torch.equal(gw_pad.cpu().to(F64), torch.cat((gw_ref, torch.zeros(cout, 7, 3, 3, dtype=F64)), 1))
    assert torch.equal(gw.cpu().to(F64), gw_ref)


# =================================================================================================================== b. data gradients
@pytest.mark.parametrize("name,dtype", pairs(R.DGRAD_CASES))
def test_data_gradient(name, dtype):
    """miseg_conv3x3_fwd with the mirrored pack (kind 1): the full input-channel range and the two ci_begin / ci_count slices of a
    concat, against float64 conv_transpose2d."""
    c = _abi()
    n, h, w, k, cin, c0 = R.DGRAD_CASES[name][:6]
    R.dgrad_precondition("dgrad", name, dtype)
    g, wt, ref, _ = R.dgrad_case("dgrad", name)
    dt, gd = DT(dtype), dev(g, dtype)
    slices = [(0, cin, ref["full"])] + ([(0, c0, ref["slices"][0]), (c0, cin - c0, ref["slices"][1])] if c0 else [])
    for cb, cs, want in slices:
        out = nans((n, h, w, cs), dtype)
        c.call("miseg_conv3x3_fwd", st(), dt, ptr(gd), k, 0, None, 0, 0, n, h, w, ptr(pack(wt, dtype, 1, cb, cs)), cs, ptr(out), None)
        assert torch.equal(host(out), want), (cb, cs)


@pytest.mark.parametrize("name,dtype", pairs(R.DUAL_CASES))
def test_data_gradient_of_a_concat_in_one_launch(name, dtype):
    """miseg_conv3x3_dgrad_dual: out0 and out1 against the reference's channel slices (C0 = 16, C1 in {4, 16}; streaming and tiled)."""
    c = _abi()
    n, h, w, k, c0, c1, _ = R.DUAL_CASES[name]
    R.dgrad_precondition("dual", name, dtype)
    g, wt, ref, _ = R.dgrad_case("dual", name)
    dt = DT(dtype)
    assert R.conv_streams(dtype, k, n, h, w) == name.startswith("stream")
    out0, out1 = nans((n, h, w, c0), dtype), nans((n, h, w, c1), dtype)
    c.call("miseg_conv3x3_dgrad_dual", st(), dt, ptr(dev(g, dtype)), k, n, h, w, ptr(pack(wt, dtype, 1, 0, c0 + c1)), c0, ptr(out0), c1, ptr(out1))
    assert torch.equal(host(out0), ref["slices"][0]) and torch.equal(host(out1), ref["slices"][1])


@pytest.mark.parametrize("dtype", R.HALF, ids=["bfloat16", "float16"])
@pytest.mark.parametrize("name", sorted(R.SUMPOOL_CASES))
def test_pooled_data_gradient(name, dtype):
    """miseg_conv3x3_fwd_sumpool (streaming shapes and the tiled kernel's 64-channel-slice form) against the 2 x 2 sums of the
    reference -- the four fp32 sums are added before the one rounding, and the pooled reference is in range --, and
    miseg_conv3x3_fwd_sumpool_acc on an integer pre-fill."""
    c = _abi()
    n, h, w, k, cs, with_acc = R.SUMPOOL_CASES[name]
    R.dgrad_precondition("sumpool", name, dtype)
    g, wt, ref, _ = R.dgrad_case("sumpool", name)
    dt, gd, pk = DT(dtype), dev(g, dtype), pack(wt, dtype, 1, 0, cs)
    assert c.query("miseg_conv3x3_fwd_sumpool_supported", dt, k, n, h, w, cs)
    assert R.conv_streams(dtype, k, n, h, w) == name.startswith("stream")
    out = nans((n, h // 2, w // 2, cs), dtype)
    c.call("miseg_conv3x3_fwd_sumpool", st(), dt, ptr(gd), k, n, h, w, ptr(pk), cs, ptr(out))
    assert torch.equal(host(out), ref["pooled"])
    assert bool(c.query("miseg_conv3x3_fwd_sumpool_acc_supported", dt, k, n, h, w)) == with_acc
    if with_acc:
        pre = R.ints(f"sumpool/{name}/pre", ref["pooled"].shape, -8, 8)
        R.assert_exact_range(ref["pooled"] + pre, dtype)
        inout = dev(pre, dtype)
        c.call("miseg_conv3x3_fwd_sumpool_acc", st(), dt, ptr(gd), k, n, h, w, ptr(pk), cs, ptr(inout))
        assert torch.equal(host(inout), ref["pooled"] + pre)


@pytest.mark.parametrize("dtype", R.ALL, ids=["float32", "bfloat16", "float16"])
def test_sumpool_axpy_and_cast_pad(dtype):
    """The small movers of the backward pass: miseg_sumpool2x2 (accumulate 0 and 1), miseg_axpy (incl. a size whose blocks loop) and
    miseg_cast_pad (Cin = 1 and 3 into one 16-byte channel vector)."""
    c = _abi()
    dt, vec = DT(dtype), 4 if dtype == torch.float32 else 8
    for n, h, w, ch in R.SUMPOOL2X2_SHAPES:
        x, pre, want = R.sumpool2x2_case((n, h, w, ch))
        R.assert_exact_range(want + pre, dtype, 40)
        out = nans((n, h // 2, w // 2, ch), dtype)
        c.call("miseg_sumpool2x2", st(), dt, ptr(dev(x, dtype)), n, h, w, ch, ptr(out), 0)
        assert torch.equal(host(out), want)
        out = dev(pre, dtype)
        c.call("miseg_sumpool2x2", st(), dt, ptr(dev(x, dtype)), n, h, w, ch, ptr(out), 1)
        assert torch.equal(host(out), want + pre)
    for numel in R.axpy_sizes(vec):                                     # one partial block; more vectors than the grid has threads
        a, b = R.axpy_case(numel)
        R.assert_exact_range(a + b, dtype)
        dst = b.to(dtype).to(DEV)
        c.call("miseg_axpy", st(), dt, ptr(a.to(dtype).to(DEV)), ptr(dst), numel)
        assert torch.equal(dst.cpu().to(F64), a + b)
    for cin in (1, 3):
        n, h, w = R.CAST_PAD_SHAPE
        img = R.cast_pad_case(cin)                                      # eighths: rounded by bf16, exact in half and fp32
        out = nans((n * h * w, vec), dtype)
        c.call("miseg_cast_pad", st(), ptr(f32(img)), n * h * w, cin, dt, ptr(out), vec)
        want = torch.cat((R.round_to(img, dtype), torch.zeros(n * h * w, vec - cin, dtype=F64)), 1)
        assert torch.equal(out.cpu().to(F64), want)


# =================================================================================================================== c. weight gradients
@pytest.mark.parametrize("name,dtype", pairs(R.WGRAD_CASES))
def test_weight_gradient(name, dtype):
    """miseg_conv3x3_wgrad called directly: the narrow and the general 16-bit kernel, the fp32 kernel and their reduce, on ragged
    shapes, concatenated and upsampled sources, and every class of the split arithmetic (one tile, one split per tile, a split count
    that does not divide the tiles).  gw must equal the float64 reference as fp32 integers."""
    c = _abi()
    n, h, w, c0, ups0, c1, cout, _ = R.WGRAD_CASES[name]
    R.wgrad_precondition(name)
    x0, x1, g, ref, _ = R.wgrad_case(name)
    dt, cin = DT(dtype), c0 + c1
    nbytes = c.query("miseg_conv3x3_wgrad_ws_bytes", n, h, w, cin, cout)
    assert nbytes == R.wgrad_splits(n, h, w, cin, cout)[2] * cdiv(cin, 32) * cdiv(cout, 32) * 32 * 288 * 4
    ws, gw = scratch(nbytes), nans((cout, cin, 3, 3), torch.float32)
    c.call("miseg_conv3x3_wgrad", st(), dt, ptr(dev(x0, dtype)), c0, ups0, ptr(dev(x1, dtype)), c1, 0, n, h, w, ptr(dev(g, dtype)), cout,
           ptr(gw), ptr(ws), ws.numel())
    assert torch.equal(gw.cpu().to(F64), ref)


@pytest.mark.parametrize("dtype", R.ALL, ids=["float32", "bfloat16", "float16"])
@pytest.mark.parametrize("name", R.WGRAD_BN_NAMES)
def test_weight_gradient_with_the_batchnorm_loader(name, dtype):
    """miseg_conv3x3_wgrad_bn (the opt-in loader form) with plain coefficients -- scale = 1, shift = 0, mean = 0, A = 1, P = Q = 0 --
    so that the loader's graw is the integer (raw > 0) * gy: the result must equal wgrad_ref on that gradient."""
    c = _abi()
    n, h, w, c0, ups0, c1, cout, _ = R.WGRAD_CASES[name]
    x0, x1, gy, _, _ = R.wgrad_case(name)
    raw, ref = R.wgrad_bn_case(name)                                    # (asserts the range of the reference)
    dt, cin = DT(dtype), c0 + c1
    coef = torch.zeros(6, cout, dtype=torch.float32)
    coef[0] = 1.0
    coef[3] = 1.0
    coef = coef.to(DEV)
    ws, gw = scratch(c.query("miseg_conv3x3_wgrad_ws_bytes", n, h, w, cin, cout)), nans((cout, cin, 3, 3), torch.float32)
    c.call("miseg_conv3x3_wgrad_bn", st(), dt, ptr(dev(x0, dtype)), c0, ups0, ptr(dev(x1, dtype)), c1, 0, n, h, w, ptr(dev(raw, dtype)),
           ptr(dev(gy, dtype)), ptr(coef), cout, ptr(gw), ptr(ws), ws.numel())
    assert torch.equal(gw.cpu().to(F64), ref)


@pytest.mark.parametrize("dtype", R.ALL, ids=["float32", "bfloat16", "float16"])
def test_weight_gradient_slice_keeps_three_of_eight_channels(dtype):
    """miseg_conv3x3_wgrad on an input with three real and five zero channels, then miseg_conv3x3_wgrad_slice keeping the first three:
    a wrong channel stride in the slice would mix the kept channels."""
    c = _abi()
    n, h, w, cin, cpad, cout = R.SLICE_CASE
    x, g, ref = R.slice_case()
    ws = scratch(c.query("miseg_conv3x3_wgrad_ws_bytes", n, h, w, cpad, cout))
    gw_pad, gw = nans((cout, cpad, 3, 3), torch.float32), nans((cout, cin, 3, 3), torch.float32)
    c.call("miseg_conv3x3_wgrad", st(), DT(dtype), ptr(dev(x, dtype)), cpad, 0, None, 0, 0, n, h, w, ptr(dev(g, dtype)), cout, ptr(gw_pad), ptr(ws),
           ws.numel())
    c.call("miseg_conv3x3_wgrad_slice", st(), ptr(gw_pad), cout, cpad, cin, ptr(gw))
    assert torch.equal(gw_pad.cpu().to(F64), ref) and torch.equal(gw.cpu().to(F64), ref[:, :cin])


@pytest.mark.parametrize("name,dtype", pairs(R.LOADER_CASES))
def test_batchnorm_loaders_with_nonzero_offsets(name, dtype):
    """miseg_conv3x3_dgrad_bn (streaming and tiled loaders, ragged sizes) and miseg_conv3x3_wgrad_bn (narrow, general and fp32 kernels)
    with integer coefficient rows whose P and Q are NOT zero: graw = [y > 0] * A * gy + P + Q * (raw - mean) is an integer, so the
    results are exact at any size -- and positions outside the image must stay zero, not P - Q * mean."""
    c = _abi()
    kind, n, h, w, k, other, _ = R.LOADER_CASES[name]
    R.loader_precondition(name, dtype)
    case = R.loader_case(name)
    dt = DT(dtype)
    rawd, gyd, coef = dev(case["raw"], dtype), dev(case["gy"], dtype), f32(case["coef"])
    if kind == "dgrad":
        assert c.query("miseg_conv3x3_dgrad_bn_supported", dt, k, n, h, w, other, 0)
        assert R.conv_streams(dtype, k, n, h, w) == ("stream" in name)
        out = nans((n, h, w, other), dtype)
        c.call("miseg_conv3x3_dgrad_bn", st(), dt, ptr(rawd), ptr(gyd), ptr(coef), k, n, h, w, ptr(pack(case["w"], dtype, 1, 0, other)), other,
               ptr(out), 0, None, None, None)
        assert torch.equal(host(out), case["gx"])
    else:
        ws, gw = scratch(c.query("miseg_conv3x3_wgrad_ws_bytes", n, h, w, other, k)), nans((k, other, 3, 3), torch.float32)
        c.call("miseg_conv3x3_wgrad_bn", st(), dt, ptr(dev(case["x"], dtype)), other, 0, None, 0, 0, n, h, w, ptr(rawd), ptr(gyd), ptr(coef), k,
               ptr(gw), ptr(ws), ws.numel())
        assert torch.equal(gw.cpu().to(F64), case["gw"])


# =================================================================================================================== d. logits head
@pytest.mark.parametrize("dtype", R.ALL, ids=["float32", "bfloat16", "float16"])
@pytest.mark.parametrize("shape", sorted(R.C1X1_SHAPES))
def test_logits_head(shape, dtype):
    """miseg_conv1x1_fwd / _bwd for every supported Cout with an integer bias, at a pixel count that is no multiple of 256 and at one
    above 512 * 256 (the backward's blocks loop; the forward's grid is capped at 4096 blocks and gets its own looping shape below):
    out, gin (stored in dt), gw and gbias are exact."""
    c = _abi()
    n, h, w = R.C1X1_SHAPES[shape]
    dt = DT(dtype)
    for cout in R.C1X1_COUTS:
        x, wt, bias, gout, out_ref, gin_ref, gw_ref, gb_ref = R.c1x1_case(shape, cout)
        R.assert_exact_range(gin_ref, dtype, cout * 4)
        xd, wd, bd = dev(x, dtype), f32(wt), f32(bias)
        out = nans((n, h, w, cout), torch.float32)
        c.call("miseg_conv1x1_fwd", st(), dt, ptr(xd), n, h, w, 16, ptr(wd), ptr(bd), cout, ptr(out))
        assert torch.equal(host(out), out_ref), cout
        ws = scratch(c.query("miseg_conv1x1_bwd_ws_bytes", n, h, w, 16, cout))
        gin, gw, gb = nans((n, h, w, 16), dtype), nans((cout, 16), torch.float32), nans((cout,), torch.float32)
        c.call("miseg_conv1x1_bwd", st(), dt, ptr(xd), ptr(dev(gout, torch.float32)), n, h, w, 16, ptr(wd), cout, ptr(gin), ptr(gw), ptr(gb),
               ptr(ws), ws.numel())
        assert torch.equal(host(gin), gin_ref) and torch.equal(gw.cpu().to(F64), gw_ref) and torch.equal(gb.cpu().to(F64), gb_ref), cout


@pytest.mark.parametrize("dtype", R.ALL, ids=["float32", "bfloat16", "float16"])
def test_logits_head_forward_blocks_loop(dtype):
    """miseg_conv1x1_fwd above 4096 * 256 pixels, where its grid-stride loop is entered a second time."""
    c = _abi()
    n, h, w = R.C1X1_FWD_LOOPING
    x = R.ints("c1x1/fwd_looping/x", (n, 16, h, w), -2, 2)
    xd = dev(x, dtype)
    for cout in R.C1X1_COUTS:
        wt, bias = R.ints(f"c1x1/{cout}/w", (cout, 16), -2, 2), R.ints(f"c1x1/{cout}/b", (cout,), -5, 5)
        out = nans((n, h, w, cout), torch.float32)
        c.call("miseg_conv1x1_fwd", st(), DT(dtype), ptr(xd), n, h, w, 16, ptr(f32(wt)), ptr(f32(bias)), cout, ptr(out))
        want = torch.einsum("nchw,oc->nohw", x, wt) + bias.view(1, -1, 1, 1)          # |.| <= 16 * 4 + 5: exact anywhere
        assert torch.equal(host(out), want), cout
        del out


def test_logits_head_refuses_six_and_seven_classes():
    """Cout = 6 and 7 have no kernel instance today (csrc/mi_out.hip accepts 2..8 classes): the entry points must refuse, not launch."""
    c = _abi()
    n, h, w = 1, 4, 4
    x = torch.zeros(n, h, w, 16, dtype=torch.bfloat16, device=DEV)
    for cout in (6, 7):
        wd, bd, out, gout = (torch.zeros(s, dtype=torch.float32, device=DEV) for s in ((cout, 16), (cout,), (n, h, w, cout), (n, h, w, cout)))
        with pytest.raises(c.MisegError, match="unsupported Cout"):
            c.call("miseg_conv1x1_fwd", st(), c.BF16, ptr(x), n, h, w, 16, ptr(wd), ptr(bd), cout, ptr(out))
        ws = scratch(c.query("miseg_conv1x1_bwd_ws_bytes", n, h, w, 16, cout))
        gin, gw, gb = torch.zeros_like(x), torch.zeros_like(wd), torch.zeros_like(bd)
        with pytest.raises(c.MisegError, match="unsupported Cout"):
            c.call("miseg_conv1x1_bwd", st(), c.BF16, ptr(x), ptr(gout), n, h, w, 16, ptr(wd), cout, ptr(gin), ptr(gw), ptr(gb), ptr(ws), ws.numel())


# =================================================================================================================== e. BatchNorm
@pytest.mark.parametrize("dtype", R.ALL, ids=["float32", "bfloat16", "float16"])
@pytest.mark.parametrize("n,h,w,ch,pool", R.BN_FWD_CASES)
def test_bn_relu_forward(n, h, w, ch, pool, dtype):
    """miseg_bn_relu_fwd with dyadic coefficients on integer raw values (negative ones and exact zeros included): y and the fused
    2 x 2 max-pool -- the coalesced pooled kernel (C / vector a power of two <= 32) and the generic one.  Odd sizes: y alone (the
    pooled form needs even H, W and must refuse otherwise)."""
    c = _abi()
    dt = DT(dtype)
    raw, saved, y_ref, p_ref = R.bn_fwd_case((n, h, w, ch, pool), dtype)        # (asserts range, exact zeros, a zero pre-activation)
    y = nans((n, h, w, ch), dtype)
    pooled = nans((n, h // 2, w // 2, ch), dtype)
    c.call("miseg_bn_relu_fwd", st(), dt, ptr(dev(raw, dtype)), n, h, w, ch, ptr(f32(saved)), ptr(y), ptr(pooled) if pool else None)
    assert torch.equal(host(y), y_ref)
    if pool:
        assert torch.equal(host(pooled), p_ref)
    else:
        with pytest.raises(c.MisegError, match="even H, W"):
            c.call("miseg_bn_relu_fwd", st(), dt, ptr(dev(raw, dtype)), n, h, w, ch, ptr(f32(saved)), ptr(y), ptr(pooled))


def _bn_check(got, ref, dtype, what):
    graw, ggamma, gbeta = got
    assert torch.equal(ggamma.cpu().to(F64), ref["ggamma"]), what
    assert torch.equal(gbeta.cpu().to(F64), ref["gbeta"]), what
    assert torch.equal(host(graw), R.round_to(ref["graw"], dtype)), what


@pytest.mark.parametrize("dtype", R.ALL, ids=["float32", "bfloat16", "float16"])
@pytest.mark.parametrize("name", sorted(R.BN_CASES))
def test_bn_relu_backward(name, dtype):
    """miseg_bn_relu_bwd, _sync, _dual and _dual_acc on integer gradients and raw values in {-2..2} -- most 2 x 2 windows hold tied
    maxima (the pooled gradient must go to the FIRST one in scan order) and many y are exactly 0 (masked) -- with a second gradient
    on a strict inner sample range.  ggamma and gbeta are exact; graw is the float64 reference rounded once to the storage type
    (training mode at power-of-two pixel counts: the two means are dyadic and every fp32 intermediate is exact).  _dual_acc: its
    accumulator reads back the exact totals in both fixed-point tiers with both misfit counters at 0."""
    c = _abi()
    n, h, w, ch, training, pool = R.BN_CASES[name]
    dt = DT(dtype)
    case = R.bn_case(name)
    rawd, gyd, gpd, gy2d = (dev(case[k], dtype) for k in ("raw", "gy", "gpool", "gy2"))
    gam, sav = f32(case["gamma"]), f32(case["saved"])
    n2 = case["n2"]
    assert 0 < n2[0] < n2[1] <= n and (n2[1] < n or n == 2)        # a strict inner range (two samples: the second one)
    ws = scratch(c.query("miseg_bn_bwd_ws_bytes", n, h, w, ch))
    yd = dev(R.bn_fwd_ref(case["raw"], case["saved"], False)[0], dtype)

    def outs():
        return nans((n, h, w, ch), dtype), nans((ch,), torch.float32), nans((ch,), torch.float32)

    ref_plain = R.bn_precondition(name, "plain", dtype)
    ref_main = R.bn_precondition(name, "pool", dtype) if pool else ref_plain
    ref_dual = R.bn_precondition(name, "dual", dtype)
    # two launches + finalize, with the pooled gradient where the layer has one
    o = outs()
    c.call("miseg_bn_relu_bwd", st(), dt, ptr(rawd), ptr(yd), ptr(gyd), ptr(gpd), n, h, w, ch, ptr(gam), ptr(sav), int(training), ptr(o[0]), ptr(o[1]),
           ptr(o[2]), ptr(ws), ws.numel())
    _bn_check(o, ref_main, dtype, "bwd")
    # the last reduce block finishes the statistics (twice: the counter must be back at zero); gy alone, then with the pooled gradient
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    for gp, ref in ((None, ref_plain), (gpd, ref_main)):
        o = outs()
        c.call("miseg_bn_relu_bwd_sync", st(), dt, ptr(rawd), ptr(yd), ptr(gyd), ptr(gp), n, h, w, ch, ptr(gam), ptr(sav), int(training), ptr(o[0]),
               ptr(o[1]), ptr(o[2]), ptr(ws), ws.numel(), ptr(counter))
        _bn_check(o, ref, dtype, "sync")
        assert int(counter) == 0
    if pool:        # the pooled gradient alone (gy = null)
        ref = R.bn_bwd_ref(case["raw"], None, case["gpool"], None, None, case["gamma"], case["saved"], training)
        o = outs()
        c.call("miseg_bn_relu_bwd", st(), dt, ptr(rawd), ptr(yd), None, ptr(gpd), n, h, w, ch, ptr(gam), ptr(sav), int(training), ptr(o[0]), ptr(o[1]),
               ptr(o[2]), ptr(ws), ws.numel())
        _bn_check(o, ref, dtype, "pool only")
    o = outs()
    c.call("miseg_bn_relu_bwd_dual", st(), dt, ptr(rawd), ptr(gyd), ptr(gpd), ptr(gy2d), n2[0], n2[1], n, h, w, ch, ptr(gam), ptr(sav), int(training),
           ptr(o[0]), ptr(o[1]), ptr(o[2]), ptr(ws), ws.numel())
    _bn_check(o, ref_dual, dtype, "dual")
    assert c.query("miseg_bn_relu_bwd_acc_supported", dt, n, h, w, ch)
    o, acc = outs(), torch.zeros(4 * ch + 2, dtype=torch.int64, device=DEV)
    c.call("miseg_bn_relu_bwd_dual_acc", st(), dt, ptr(rawd), ptr(gyd), ptr(gpd), ptr(gy2d), n2[0], n2[1], n, h, w, ch, ptr(gam), ptr(sav),
           int(training), ptr(o[0]), ptr(o[1]), ptr(o[2]), ptr(ws), ws.numel(), ptr(acc))
    _bn_check(o, ref_dual, dtype, "dual_acc")
    want = torch.cat((ref_dual["gbeta"], ref_dual["ggamma"]))
    assert int(acc[4 * ch]) == 0 and int(acc[4 * ch + 1]) == 0                                  # every block sum fitted both tiers
    assert torch.equal(fixed(acc[:2 * ch], 2.0 ** 40), want) and torch.equal(fixed(acc[2 * ch:4 * ch], 2.0 ** 12), want)


@pytest.mark.parametrize("name,dtype", pairs(R.DGRAD_BN_CASES))
def test_batchnorm_backward_folded_into_the_data_gradient(name, dtype):
    """miseg_bn_relu_bwd_stats, then miseg_conv3x3_dgrad_bn with and without gy.  bwd_coef must hold the six rows implied by the exact
    sums.  The loader (csrc/common.h bn_graw_vec, called from the tile loaders of csrc/conv_tiled.h, conv_stream.hip and conv_wgrad.hip) forms
    graw = [y > 0] * A * gy + P + Q * (raw - mean) in fp32 and PACKS it to the storage type before it reaches the matrix cores: one
    rounding in bf16 / half, none in fp32.  Evaluation mode (P = Q = 0): graw is a multiple of 1/4, nothing is rounded, the data
    gradient is exact.  Training mode: the reference rounds graw once at that same place (exact_ref.dgrad_bn_reference); the cases
    keep graw a multiple of 2^-10, so the fp32 accumulator still holds every partial sum exactly, and the stored gradient is the
    float64 one rounded once.  Without gy the kernel reads that same rounded graw as a plain tensor: same result."""
    c = _abi()
    n, h, w, k, cs, training, _ = R.DGRAD_BN_CASES[name]
    dt = DT(dtype)
    case, ref = R.dgrad_bn_case(name), R.dgrad_bn_reference(name, dtype)
    rawd, gyd, gam, sav = dev(case["raw"], dtype), dev(case["gy"], dtype), f32(case["gamma"]), f32(case["saved"])
    ws = scratch(c.query("miseg_bn_bwd_ws_bytes", n, h, w, k))
    coef, ggamma, gbeta = nans((6, k), torch.float32), nans((k,), torch.float32), nans((k,), torch.float32)
    c.call("miseg_bn_relu_bwd_stats", st(), dt, ptr(rawd), ptr(gyd), n, h, w, k, ptr(gam), ptr(sav), int(training), ptr(coef), ptr(ggamma), ptr(gbeta),
           None, 0, ptr(ws), ws.numel())
    assert torch.equal(ggamma.cpu().to(F64), ref["bn"]["ggamma"]) and torch.equal(gbeta.cpu().to(F64), ref["bn"]["gbeta"])
    assert torch.equal(coef.cpu().to(F64), ref["coef"])
    assert c.query("miseg_conv3x3_dgrad_bn_supported", dt, k, n, h, w, cs, 0)
    assert R.conv_streams(dtype, k, n, h, w) == ("stream" in name)
    pk, want = pack(case["w"], dtype, 1, 0, cs), R.round_to(ref["gx"], dtype)
    out = nans((n, h, w, cs), dtype)
    c.call("miseg_conv3x3_dgrad_bn", st(), dt, ptr(rawd), ptr(gyd), ptr(coef), k, n, h, w, ptr(pk), cs, ptr(out), 0, None, None, None)
    assert torch.equal(host(out), want)
    out = nans((n, h, w, cs), dtype)
    c.call("miseg_conv3x3_dgrad_bn", st(), dt, ptr(dev(ref["graw_loaded"], dtype)), None, None, k, n, h, w, ptr(pk), cs, ptr(out), 0, None, None, None)
    assert torch.equal(host(out), want)
    if "pool_" in name and dtype != torch.float32:      # the loader in front of the 2 x 2 sum-pooled epilogue: four exact fp32 sums, one rounding
        assert c.query("miseg_conv3x3_dgrad_bn_supported", dt, k, n, h, w, cs, 1)
        out = nans((n, h // 2, w // 2, cs), dtype)
        c.call("miseg_conv3x3_dgrad_bn", st(), dt, ptr(rawd), ptr(gyd), ptr(coef), k, n, h, w, ptr(pk), cs, ptr(out), 1, None, None, None)
        assert torch.equal(host(out), R.round_to(R.dgrad_ref(ref["graw_loaded"], case["w"])["pooled"], dtype))
    if training or "stream" in name:
        return
    # the epilogue reduce (evaluation-mode tiled cases: exact_ref.dgrad_red_reference), alone on the plain tensor and behind the loader:
    # the same gradient, and partial rows that add up to the exact sums of dz and dz * xhat of the layer that produced the Cs-channel tensor
    red = R.dgrad_red_reference(name, dtype)
    rows = c.query("miseg_conv3x3_dgrad_red_parts", dt, k, n, h, w, cs)
    _, tw, th = R.tiled_shape(dtype, h, w, cs)
    assert rows == n * cdiv(h, th) * cdiv(w, tw)
    rraw, rsaved = dev(red["raw"], dtype), f32(red["saved"])
    for src, gy_, coef_ in ((dev(ref["graw_loaded"], dtype), None, None), (rawd, gyd, coef)):
        out, parts = nans((n, h, w, cs), dtype), nans((rows, 2, cs), torch.float32)
        c.call("miseg_conv3x3_dgrad_bn", st(), dt, ptr(src), ptr(gy_), ptr(coef_), k, n, h, w, ptr(pk), cs, ptr(out), 0, ptr(rraw), ptr(rsaved), ptr(parts))
        assert torch.equal(host(out), want)
        tot = parts.cpu().to(F64).sum(0)
        assert torch.equal(tot[0], red["gbeta"]) and torch.equal(tot[1], red["ggamma"])


# =================================================================================================================== f. the switches
def _eight_row_cases():
    """The 16-bit cases of the forward, statistics and pooled tables that the tiled kernel serves with 8-row tiles."""
    eight = lambda d, cin, n, h, w, cout: not R.conv_streams(d, cin, n, h, w) and R.tiled_shape(d, h, w, cout)[2] == 8
    fwd = [(k, d) for k, v in sorted(R.FWD_CASES.items()) for d in v[-1] if d in R.HALF and eight(d, v[3] + v[5], v[0], v[1], v[2], v[7])]
    stats = [(k, d) for k, v in sorted(R.STATS_CASES.items()) for d in v[-1] if d in R.HALF and eight(d, v[3], v[0], v[1], v[2], v[4])]
    pooled = [(k, d) for k, v in sorted(R.SUMPOOL_CASES.items()) for d in R.HALF if eight(d, v[3], v[0], v[1], v[2], v[4])]
    return fwd, stats, pooled


def _switch_child():
    """Runs in a fresh process (the library reads its switches once): the 8-row cases through the test functions above."""
    fwd, stats, pooled = _eight_row_cases()
    for fn, cases in ((test_forward_convolution, fwd), (test_forward_convolution_batchnorm_statistics, stats), (test_pooled_data_gradient, pooled)):
        for name, dtype in cases:
            fn(name, dtype)
            torch.cuda.synchronize()
            _LIVE.clear()
    print(f"switch child ok: {len(fwd)} forward, {len(stats)} statistics, {len(pooled)} pooled cases")


CHILD = "import conftest, test_gpu_exact_integers as t; t._switch_child()"       # conftest: the import paths of the suite


def test_eight_row_tiles_under_the_conv_switches():
    """MISEG_CONV_PERSISTENT=0 (the 4-wave per-tile forms of the 8-row tiles) and MISEG_CONV_DEPTH=2 (two stages in flight in the
    persistent form, non-pooled): each in a fresh process, one after the other, the second only if the first passed; every 8-row
    forward, statistics and pooled case against the same float64 references, equality at every element."""
    fwd, stats, pooled = _eight_row_cases()
    shapes = {R.tiled_shape(d, *R.FWD_CASES[k][1:3], R.FWD_CASES[k][7])[:2] for k, d in fwd}
    assert shapes == {(16, 16), (16, 32), (32, 16), (32, 32)} and stats and len(pooled) >= 4       # both slice widths on both tile widths
    for switch in ("MISEG_CONV_PERSISTENT=0", "MISEG_CONV_DEPTH=2"):
        key, value = switch.split("=")
        env = {k: v for k, v in os.environ.items() if k not in ("MISEG_CONV_PERSISTENT", "MISEG_CONV_DEPTH")}
        env[key] = value
        res = subprocess.run([sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", CHILD], env=env,
                             cwd=os.path.dirname(os.path.abspath(__file__)), capture_output=True, text=True, timeout=300)
        assert res.returncode == 0 and "switch child ok" in res.stdout, switch + "\n" + res.stdout[-2000:] + res.stderr[-4000:]
