"""float64 references and integer input recipes for the bit-exact kernel tests (test_cpu_exact_ref.py, test_gpu_exact_integers.py).

The idea: feed the convolution / BatchNorm kernels small integers (or dyadic fractions).  Every operand is then exactly representable
in bf16, IEEE half and fp32, every product and every partial sum is an integer (a multiple of one power of two) below 2^24 of that
unit, so an fp32 accumulator holds it exactly IN WHATEVER ORDER the kernel adds, and the stored result is exact whenever it stays
inside the storage type's exact-integer range.  The HIP result must then equal the float64 reference bit for bit at every element:
no tolerance, no allowed share of bad elements.

Everything here is plain torch on the CPU, NCHW float64.  The case tables at the end are shared by the CPU test (which proves every
recipe inside the exact range at every shape) and the GPU test (which runs them).
"""
from __future__ import annotations

import functools

import numpy as np
import torch
import torch.nn.functional as F

import synth

F64 = torch.float64
# largest n such that every integer of magnitude <= n is representable: 8 / 11 / 24 significand bits
EXACT_INT = {torch.bfloat16: 256.0, torch.float16: 2048.0, torch.float32: 16777216.0}
ACC_LIMIT = 16777216.0      # the fp32 accumulator


# ----------------------------------------------------------------------------------------------------------------- inputs
def ints(tag: str, shape, lo: int, hi: int, density: float = 1.0) -> torch.Tensor:
    """Deterministic integers in [lo, hi] as a float64 tensor, seeded from the tag (as synth does); ``density`` = share of entries kept
    (the others are zero), for the cases that need small sums."""
    rs = np.random.RandomState(synth._seed("exact/" + tag))
    v = rs.randint(lo, hi + 1, size=tuple(shape)).astype(np.float64)
    if density < 1.0:
        v = v * (rs.random_sample(tuple(shape)) < density)
    return torch.from_numpy(v)


def pick(tag: str, shape, values) -> torch.Tensor:
    """Deterministic draws from a short list of values (the dyadic BatchNorm coefficients)."""
    rs = np.random.RandomState(synth._seed("exact/" + tag))
    return torch.tensor(values, dtype=F64)[torch.from_numpy(rs.randint(0, len(values), size=tuple(shape)))]


# ----------------------------------------------------------------------------------------------------------------- references
def cat_sources(x0, ups0, x1=None, ups1=0):
    """The convolution's input: channel concat of up to two sources, each optionally read through a nearest x2 upsample."""
    a = F.interpolate(x0, scale_factor=2, mode="nearest") if ups0 else x0
    if x1 is None:
        return a
    b = F.interpolate(x1, scale_factor=2, mode="nearest") if ups1 else x1
    return torch.cat((a, b), 1)


def conv_ref(x0, ups0, x1, ups1, w):
    """3 x 3 convolution, zero padding 1, in float64 -> (out, per-channel sum, per-channel sum of squares)."""
    out = F.conv2d(cat_sources(x0, ups0, x1, ups1).to(F64), w.to(F64), None, 1, 1)
    return out, out.sum((0, 2, 3)), (out * out).sum((0, 2, 3))


def dgrad_ref(g, w, c0=None):
    """Data gradient of the convolution with weight w [K][Cin][3][3] for the output gradient g [N][K][H][W]: float64 conv_transpose2d.
    Returns dict(full=[N][Cin][H][W], slices=(channels [0, c0), channels [c0, Cin)) of a concat, pooled=2 x 2 sums of `full` -- the
    gradient of a source that was read through the nearest x2 upsample; None for odd sizes)."""
    full = F.conv_transpose2d(g.to(F64), w.to(F64), None, 1, 1)
    c0 = full.shape[1] if c0 is None else c0
    h, wd = full.shape[2:]
    pooled = F.avg_pool2d(full, 2) * 4 if h % 2 == 0 and wd % 2 == 0 else None
    return dict(full=full, slices=(full[:, :c0], full[:, c0:]), pooled=pooled)


def wgrad_ref(x0, ups0, x1, ups1, g, method: str = "autograd"):
    """Weight gradient [K][Cin][3][3] of conv_ref for the output gradient g, two independent ways: float64 autograd of conv_ref, and
    nine shifted einsums over the zero-padded input."""
    xin = cat_sources(x0, ups0, x1, ups1).to(F64)
    g = g.to(F64)
    if method == "autograd":
        w = torch.zeros(g.shape[1], xin.shape[1], 3, 3, dtype=F64, requires_grad=True)
        (F.conv2d(xin, w, None, 1, 1) * g).sum().backward()
        return w.grad
    assert method == "einsum", method
    h, wd = xin.shape[2:]
    xp = F.pad(xin, (1, 1, 1, 1))
    gw = torch.empty(g.shape[1], xin.shape[1], 3, 3, dtype=F64)
    for ky in range(3):
        for kx in range(3):
            gw[:, :, ky, kx] = torch.einsum("nohw,nihw->oi", g, xp[:, :, ky:ky + h, kx:kx + wd])
    return gw


def make_saved(tag: str, c: int, invstds=(0.5, 1.0, 2.0), gammas=(0.5, 1.0, 2.0)):
    """BatchNorm coefficients that keep everything dyadic: integer mean, invstd and gamma powers of two.
    -> (gamma [C], saved [4][C] = mean | invstd | scale = gamma * invstd | shift = -mean * scale), float64."""
    mean = ints(tag + "/mean", (c,), -1, 1)
    invstd = pick(tag + "/invstd", (c,), invstds)
    gamma = pick(tag + "/gamma", (c,), gammas)
    scale = gamma * invstd
    return gamma, torch.stack((mean, invstd, scale, -mean * scale))


def bn_fwd_ref(raw, saved, pool: bool):
    """y = relu(raw * scale + shift) and its 2 x 2 max-pool, float64."""
    v = lambda r: saved[r].view(1, -1, 1, 1)
    y = F.relu(raw.to(F64) * v(2) + v(3))
    return y, (F.max_pool2d(y, 2, 2) if pool else None)


def bn_bwd_ref(raw, gy, gpool, gy2, n2_range, gamma, saved, training: bool):
    """BatchNorm + ReLU (+ 2 x 2 max-pool) backward in float64 -> dict(graw, ggamma, gbeta, dz, y).
    gy: gradient of y or None; gpool: gradient of the pooled output or None; gy2: a second gradient of y for samples
    [n2_range[0], n2_range[1]) or None."""
    raw = raw.to(F64)
    v = lambda r: saved[r].to(F64).view(1, -1, 1, 1)
    y = F.relu(raw * v(2) + v(3))
    g = torch.zeros_like(raw) if gy is None else gy.to(F64).clone()
    if gpool is not None:
        # the pooled gradient goes to the FIRST maximum of each window in scan order: torch's own rule -- max_pool2d's CPU kernel keeps
        # a candidate only if it is strictly greater than the running maximum, and so do its indices
        _, idx = F.max_pool2d(y, 2, 2, return_indices=True)
        n, c, h, w = raw.shape
        routed = torch.zeros(n, c, h * w, dtype=F64)
        routed.scatter_add_(2, idx.view(n, c, -1), gpool.to(F64).reshape(n, c, -1))
        g += routed.view(n, c, h, w)
    if gy2 is not None:
        g[n2_range[0]:n2_range[1]] += gy2.to(F64)
    dz = (y > 0).to(F64) * g
    xhat = (raw - v(0)) * v(1)
    gbeta, ggamma = dz.sum((0, 2, 3)), (dz * xhat).sum((0, 2, 3))
    count = raw.shape[0] * raw.shape[2] * raw.shape[3]
    m1 = (gbeta / count if training else torch.zeros_like(gbeta)).view(1, -1, 1, 1)
    m2 = (ggamma / count if training else torch.zeros_like(ggamma)).view(1, -1, 1, 1)
    graw = (gamma.to(F64) * saved[1].to(F64)).view(1, -1, 1, 1) * (dz - m1 - xhat * m2)
    return dict(graw=graw, ggamma=ggamma, gbeta=gbeta, dz=dz, y=y)


def bwd_coef_ref(gamma, saved, ggamma, gbeta, count: int, training: bool):
    """The six rows scale | shift | mean | A | P | Q with which a fused loader forms graw = [y > 0] * A * gy + P + Q * (raw - mean)."""
    a = gamma * saved[1]
    b = gbeta / count if training else torch.zeros_like(gbeta)
    c = ggamma / count if training else torch.zeros_like(ggamma)
    return torch.stack((saved[2], saved[3], saved[0], a, -(a * b), -(a * saved[1] * c)))


def round_to(t64: torch.Tensor, dtype) -> torch.Tensor:
    """One round-to-nearest-even into the storage type, returned as float64.  Goes through fp32: every value these tests round is
    exactly representable in fp32 (asserted), so this is a single rounding."""
    t32 = t64.to(torch.float32)
    assert torch.equal(t32.to(F64), t64), "value not representable in fp32: the rounding below would be a double rounding"
    return t32.to(dtype).to(F64)


def quantum_of(t64: torch.Tensor, lowest: int = -40) -> float:
    """The largest power of two every entry of t64 is a multiple of (1.0 for integers)."""
    q = 0
    while q > lowest and not bool(((t64 * 2.0 ** -q) == torch.round(t64 * 2.0 ** -q)).all()):
        q -= 1
    assert q > lowest, "not dyadic"
    return 2.0 ** q


def assert_exact_range(ref: torch.Tensor, dtype, abs_sum=None, quantum: float = 1.0) -> None:
    """The precondition of an exact comparison, asserted on the REFERENCE before anything touches the GPU: every stored value is a
    multiple of `quantum` of magnitude <= quantum * (256 | 2048 | 2^24) for bf16 | half | fp32, and -- for sums -- the worst-case
    accumulator magnitude `abs_sum` (the sum of |products| of the largest output) is below quantum * 2^24."""
    assert bool((ref / quantum == torch.round(ref / quantum)).all()), "reference is not a multiple of its quantum"
    peak = float(ref.abs().max()) / quantum
    assert peak <= EXACT_INT[dtype], (peak, dtype)
    if abs_sum is not None:
        assert float(abs_sum) / quantum < ACC_LIMIT, (float(abs_sum), quantum)


# ----------------------------------------------------------------------------------------------------------------- case tables
ALL = (torch.float32, torch.bfloat16, torch.float16)
HALF = (torch.bfloat16, torch.float16)


def conv_streams(dtype, cin, n, h, w) -> bool:
    """csrc/conv.h conv_streams(): the persistent streaming kernel serves 16-bit storage, <= 32 input channels, >= 512 16 x 32 tiles."""
    return dtype in HALF and cin <= 32 and w >= 32 and n * ((h + 15) // 16) * ((w + 31) // 32) >= 512


def tiled_shape(dtype, h, w, cout, pool=False):
    """csrc/conv.h tiled_shape(): (output channels per block, tile width, tile height) of a call the tiled kernel serves."""
    tw = 32 if w >= 32 else 16
    th = 8 if dtype in HALF and h * w >= 64 * 64 else 16
    if dtype in HALF:
        cot = 64 if pool else 16 if cout <= 16 else 32 if cout <= 32 or th == 8 else 64
    else:
        cot = 16 if cout <= 16 else 32
    return cot, tw, th


def fwd_parts(dtype, cin, n, h, w, cout, persistent=True):
    """csrc/conv_fwd.hip miseg_conv3x3_fwd_parts() for a call the tiled kernel serves: one statistics row per tile, or -- 16-bit 8-row
    tiles in the persistent form (conv.h pt_grid(): two blocks per CU over the output-channel slices) -- one per persistent block."""
    assert not conv_streams(dtype, cin, n, h, w)
    cot, tw, th = tiled_shape(dtype, h, w, cout)
    ntiles = n * ((h + th - 1) // th) * ((w + tw - 1) // tw)
    if th != 8 or not persistent:
        return ntiles
    target = max(1, 512 // ((cout + cot - 1) // cot))
    per = max(1, (ntiles + target - 1) // target)
    return (ntiles + per - 1) // per


def wgrad_splits(n, h, w, cin, cout):
    """csrc/conv_wgrad.hip wgrad_splits(): (8 x 32 tiles, blocks per split, splits)."""
    ntiles = n * ((h + 7) // 8) * ((w + 31) // 32)
    per = ((cin + 31) // 32) * ((cout + 31) // 32)
    return ntiles, per, min(max(1, 256 // per), ntiles)


def wgrad_kernel(dtype, cin, cout) -> str:
    """csrc/conv_wgrad.hip conv3x3_wgrad_impl(): which of the three weight-gradient kernels serves the layer."""
    if dtype == torch.float32:
        return "fp32"
    narrow = cout % 16 == 0 and (min(cin, cout) <= 16 or (cin == 32 and cout == 64))
    return "c16" if narrow or cout <= 16 else "general"


# forward convolution: name -> (n, h, w, c0, ups0, c1, ups1, cout, x range, w range, storage types); x in {-xr..xr}, w in {-wr..wr}
FWD_CASES = {
    "tiled_ragged_8_32": (3, 20, 36, 8, 0, 0, 0, 32, 2, 1, ALL),
    "tiled_ragged_24_32": (3, 50, 46, 24, 0, 0, 0, 32, 2, 1, ALL),
    "tiled_64_64": (3, 40, 70, 64, 0, 0, 0, 64, 2, 1, ALL),                     # 16-row tiles, 64-channel slices
    # 16-bit: 8-row tiles (H * W >= 64^2) in the persistent form, 32-channel slices; 273 tiles over 137 blocks: the last takes one
    "pt_remainder_64_64": (3, 100, 200, 64, 0, 0, 0, 64, 2, 1, HALF),
    "deep_256_256": (4, 16, 16, 256, 0, 0, 0, 256, 1, 1, ALL),                  # 16-row, 16-wide tiles, 64-channel slices
    "stream_16_16": (4, 256, 256, 16, 0, 0, 0, 16, 2, 1, ALL),                  # fp32: the tiled kernel at 512 tiles
    "stream_16_32": (4, 256, 256, 16, 0, 0, 0, 32, 2, 1, HALF),
    "stream_32_32": (4, 256, 256, 32, 0, 0, 0, 32, 2, 1, HALF),
    "stream_ragged_24_32": (6, 250, 230, 24, 0, 0, 0, 32, 2, 1, HALF),
    "stream_cat_16_16_16": (4, 256, 256, 16, 0, 16, 0, 16, 2, 1, HALF),
    "tiled_cat_16_16_16": (3, 20, 36, 16, 0, 16, 0, 16, 2, 1, ALL),
    "stream_cat_ragged_8_16_16": (6, 250, 230, 8, 0, 16, 0, 16, 2, 1, HALF),
    "tiled_cat_ragged_8_16_16": (3, 50, 46, 8, 0, 16, 0, 16, 2, 1, ALL),
    "stream_up_32_16": (4, 256, 256, 32, 1, 0, 0, 16, 2, 1, HALF),
    "tiled_up_32_16": (3, 20, 36, 32, 1, 0, 0, 16, 2, 1, ALL),
    "stream_up_16_cat_16_16": (4, 256, 256, 16, 1, 16, 0, 16, 2, 1, HALF),
    "tiled_up_16_cat_16_16": (3, 20, 36, 16, 1, 16, 0, 16, 2, 1, ALL),
    # one case per tile shape the library is built with and no case above selects (tiled_shape: channels per block, tile width x height;
    # fp32 always has 16-row tiles and at most 32 channels per block); Cin = 64: two channel chunks per tile, once per tile height
    "t16x16_8_8": (2, 16, 16, 8, 0, 0, 0, 8, 2, 1, ALL),                        # 16, 16 x 16; half a channel slice
    "t16x16_ragged_16_32": (2, 20, 20, 16, 0, 0, 0, 32, 2, 1, ALL),             # 32, 16 x 16
    "t16x16_ragged_64_64": (1, 20, 20, 64, 0, 0, 0, 64, 2, 1, ALL),             # 64, 16 x 16
    "t8x32_16_16": (2, 64, 64, 16, 0, 0, 0, 16, 2, 1, ALL),                     # 16-bit: 16, 32 x 8
    "t8x32_ragged_8_32": (2, 70, 66, 8, 0, 0, 0, 32, 2, 1, ALL),                # 16-bit: 32, 32 x 8 with edge tiles
    "t8x16_16_16": (1, 256, 16, 16, 0, 0, 0, 16, 2, 1, ALL),                    # 16-bit: 16, 16 x 8
    "t8x16_ragged_64_64": (2, 258, 18, 64, 0, 0, 0, 64, 2, 1, ALL),             # 16-bit: 32, 16 x 8, two slices
}


@functools.lru_cache(maxsize=4)
def fwd_case(name: str):
    """-> (x0, x1 or None, w, (out, sum, sumsq), worst-case accumulator magnitude) of a FWD_CASES entry."""
    n, h, w, c0, ups0, c1, ups1, cout, xr, wr, _ = FWD_CASES[name]
    x0 = ints(f"fwd/{name}/x0", (n, c0, h >> ups0, w >> ups0), -xr, xr)
    x1 = ints(f"fwd/{name}/x1", (n, c1, h >> ups1, w >> ups1), -xr, xr) if c1 else None
    wt = ints(f"fwd/{name}/w", (cout, c0 + c1, 3, 3), -wr, wr)
    return x0, x1, wt, conv_ref(x0, ups0, x1, ups1, wt), 9.0 * (c0 + c1) * xr * wr


# BatchNorm statistics of the forward convolution: sparse inputs (density 1/8, values {-1, 0, 1}), so that a channel's sum of squares
# over the WHOLE tensor stays below 2^24 -- every partial sum is then exact whatever the block partition.  (n, h, w, cin, cout, types)
STATS_CASES = {
    "stream_16_16": (4, 256, 256, 16, 16, ALL),
    "tiled_ragged_8_32": (3, 20, 36, 8, 32, ALL),
    "pt_remainder_64_64": (3, 100, 200, 64, 64, ALL),   # 16-bit: the persistent tiled kernel, one row per block of two tiles
    # the other tile shapes (FWD_CASES has the map from size to shape)
    "t16x16_8_8": (2, 16, 16, 8, 8, ALL),
    "t16x16_ragged_16_32": (2, 20, 20, 16, 32, ALL),
    "t16x16_ragged_16_64": (1, 20, 20, 16, 64, ALL),
    "t8x32_16_16": (2, 64, 64, 16, 16, ALL),
    "t8x16_16_16": (1, 256, 16, 16, 16, ALL),
    "t8x16_ragged_64_64": (2, 258, 18, 64, 64, ALL),
}


@functools.lru_cache(maxsize=4)
def stats_case(name: str):
    n, h, w, cin, cout, _ = STATS_CASES[name]
    x = ints(f"stats/{name}/x", (n, cin, h, w), -1, 1, density=0.125)
    wt = ints(f"stats/{name}/w", (cout, cin, 3, 3), -1, 1)
    return x, wt, conv_ref(x, 0, None, 0, wt)


# the stem: one image channel, (n, h, w, cout); image in {-2..2}, weights in {-1, 0, 1}
STEM_CASES = {"stream_16": (4, 256, 256, 16), "ragged_16": (3, 50, 46, 16), "odd_32": (5, 33, 20, 32)}


@functools.lru_cache(maxsize=4)
def stem_case(name: str):
    n, h, w, cout = STEM_CASES[name]
    img = ints(f"stem/{name}/x", (n, 1, h, w), -2, 2)
    wt = ints(f"stem/{name}/w", (cout, 1, 3, 3), -1, 1)
    g = ints(f"stem/{name}/g", (n, cout, h, w), -1, 1)
    return img, wt, g, conv_ref(img, 0, None, 0, wt), wgrad_ref(img, 0, None, 0, g)


# data gradient: the layer has weight [K][Cin][3][3]; g [N][K][H][W] in {-gr..gr} with `density`, w in {-1, 0, 1}.
# name -> (n, h, w, K, Cin, c0 (concat split of the input channels, or None), g range, density, storage types)
DGRAD_CASES = {
    "tiled_ragged_32_8": (3, 20, 36, 32, 8, None, 2, 1.0, ALL),
    "tiled_ragged_32_8p16": (3, 50, 46, 32, 24, 8, 2, 1.0, ALL),
    "tiled_64_64": (3, 40, 70, 64, 64, None, 2, 1.0, ALL),
    "deep_256_256": (4, 16, 16, 256, 256, None, 1, 1.0, ALL),
    "pt_remainder_64_64": (3, 100, 200, 64, 64, None, 2, 1.0, HALF),
    "stream_16_16p16": (4, 256, 256, 16, 32, 16, 2, 1.0, HALF),
    "stream_32_32": (4, 256, 256, 32, 32, None, 2, 1.0, HALF),
    "stream_ragged_32_8p16": (6, 250, 230, 32, 24, 8, 2, 1.0, HALF),
}
# miseg_conv3x3_dgrad_dual: C0 = 16, C1 in {4, 16}.  name -> (n, h, w, K, C0, C1, storage types)
DUAL_CASES = {
    "stream_16_16p16": (4, 256, 256, 16, 16, 16, HALF),
    "stream_16_16p4": (4, 256, 256, 16, 16, 4, HALF),
    "stream_ragged_32_16p4": (6, 250, 230, 32, 16, 4, HALF),
    "tiled_16_16p16": (3, 20, 36, 16, 16, 16, ALL),
    "tiled_ragged_32_16p4": (3, 50, 46, 32, 16, 4, ALL),
    "tiled_64_16p16": (3, 40, 70, 64, 16, 16, ALL),
}
# pooled data gradient (miseg_conv3x3_fwd_sumpool[_acc]): g in {-1, 0, 1} at density 1/2, so that the 2 x 2 SUMS stay inside bf16's 256.
# name -> (n, h, w, K, Cs, acc form too)
SUMPOOL_CASES = {
    "stream_16_32": (4, 256, 256, 16, 32, True),
    "stream_32_16": (4, 256, 256, 32, 16, True),
    "stream_ragged_16_32": (6, 250, 230, 16, 32, True),
    "tiled_64_64": (3, 20, 36, 64, 64, False),          # the tiled kernel's 64-channel-slice form (Cs > 32), 16-row tiles
    "tiled8_128_64": (2, 64, 70, 128, 64, False),       # ... 8-row tiles, ragged width
    "tiled16x16_ragged_64_64": (2, 20, 20, 64, 64, False),      # ... 16-wide 16-row tiles
    "tiled8x16_ragged_16_64": (1, 258, 18, 16, 64, False),      # ... 16-wide 8-row tiles
}


@functools.lru_cache(maxsize=4)
def dgrad_case(table: str, name: str):
    """-> (g, w, dgrad_ref(g, w, c0), worst-case accumulator magnitude)."""
    if table == "dgrad":
        n, h, w, k, cin, c0, gr, dens, _ = DGRAD_CASES[name]
    elif table == "dual":
        n, h, w, k, c0, c1, _ = DUAL_CASES[name]
        cin, gr, dens = c0 + c1, 2, 1.0
    else:
        n, h, w, k, cin, _ = SUMPOOL_CASES[name]
        c0, gr, dens = None, 1, 0.5
    g = ints(f"{table}/{name}/g", (n, k, h, w), -gr, gr, density=dens)
    wt = ints(f"{table}/{name}/w", (k, cin, 3, 3), -1, 1)
    return g, wt, dgrad_ref(g, wt, c0), 9.0 * k * gr * (4 if table == "sumpool" else 1)


# weight gradient: x in {-2..2}, g in {-1, 0, 1}.  name -> (n, h, w, c0, ups0, c1, cout, storage types)
WGRAD_CASES = {
    # narrow 16-bit kernel (conv3x3_wgrad_bf16_c16_kernel)
    "c16_16_16": (2, 64, 64, 16, 0, 0, 16, ALL),
    "c16_32_16": (2, 64, 64, 32, 0, 0, 16, HALF),
    "c16_16_32": (2, 40, 70, 16, 0, 0, 32, HALF),
    "c16_32_64": (2, 24, 40, 32, 0, 0, 64, HALF),
    # general 16-bit kernel (conv3x3_wgrad_bf16_kernel); fp32: conv3x3_wgrad_kernel<float>
    "gen_32_32": (3, 50, 46, 32, 0, 0, 32, ALL),
    "gen_64_64": (3, 40, 70, 64, 0, 0, 64, ALL),
    "gen_256_256": (4, 16, 16, 256, 0, 0, 256, ALL),
    "gen_24_32": (3, 50, 46, 24, 0, 0, 32, ALL),
    "gen_cat_32_32_32": (3, 20, 36, 32, 0, 32, 32, ALL),
    "gen_up_64_32": (3, 20, 36, 64, 1, 0, 32, ALL),
    "f32_8_32": (3, 20, 36, 8, 0, 0, 32, (torch.float32,)),
    # split arithmetic, one narrow (16 -> 16: one block per split, 256 splits) and one general (64 -> 64: four blocks, 64 splits) shape each
    "one_tile_c16": (1, 8, 32, 16, 0, 0, 16, ALL),
    "one_tile_gen": (1, 8, 32, 64, 0, 0, 64, ALL),
    "sub_tile_c16": (1, 5, 19, 16, 0, 0, 16, ALL),
    "sub_tile_gen": (1, 5, 19, 64, 0, 0, 64, ALL),
    "few_tiles_c16": (3, 20, 36, 16, 0, 0, 16, ALL),        # 18 tiles < 256 splits: one split per tile
    "few_tiles_gen": (3, 20, 36, 64, 0, 0, 64, ALL),        # 18 tiles < 64 splits
    "remainder_c16": (7, 100, 70, 16, 0, 0, 16, ALL),       # 7 * 13 * 3 = 273 tiles over 256 splits: 17 splits take a second tile
    "remainder_gen": (5, 50, 70, 64, 0, 0, 64, ALL),        # 5 * 7 * 3 = 105 tiles over 64 splits: 41 splits take a second tile
    "stream_c16": (4, 256, 256, 16, 0, 0, 16, HALF),        # the streaming layers' shape: 1 024 tiles over 256 splits
}


@functools.lru_cache(maxsize=4)
def wgrad_case(name: str):
    """-> (x0, x1 or None, g, wgrad_ref, worst-case accumulator magnitude)."""
    n, h, w, c0, ups0, c1, cout, _ = WGRAD_CASES[name]
    x0 = ints(f"wgrad/{name}/x0", (n, c0, h >> ups0, w >> ups0), -2, 2)
    x1 = ints(f"wgrad/{name}/x1", (n, c1, h, w), -2, 2) if c1 else None
    g = ints(f"wgrad/{name}/g", (n, cout, h, w), -1, 1)
    return x0, x1, g, wgrad_ref(x0, ups0, x1, 0, g), 2.0 * n * h * w


# 1 x 1 logits head: (n, h, w); in [N][16][H][W] in {-2..2}, w [Cout][16] in {-2..2}, integer bias, gout in {-2..2}
C1X1_SHAPES = {"ragged": (3, 37, 53), "looping": (2, 256, 257)}
C1X1_COUTS = (1, 2, 3, 4, 5, 8)
C1X1_FWD_LOOPING = (5, 512, 411)        # more than 4096 * 256 pixels: the forward kernel's blocks loop too (its grid is capped at 4096)


@functools.lru_cache(maxsize=4)
def c1x1_case(shape: str, cout: int):
    n, h, w = C1X1_SHAPES[shape]
    x = ints(f"c1x1/{shape}/x", (n, 16, h, w), -2, 2)
    wt = ints(f"c1x1/{cout}/w", (cout, 16), -2, 2)
    bias = ints(f"c1x1/{cout}/b", (cout,), -5, 5)
    gout = ints(f"c1x1/{shape}/{cout}/g", (n, cout, h, w), -2, 2)
    out = torch.einsum("nchw,oc->nohw", x, wt) + bias.view(1, -1, 1, 1)
    gin = torch.einsum("nohw,oc->nchw", gout, wt)
    gw = torch.einsum("nohw,nchw->oc", gout, x)
    return x, wt, bias, gout, out, gin, gw, gout.sum((0, 2, 3))


# BatchNorm + ReLU (+ max-pool) backward.  raw in {-2..2}: most 2 x 2 windows hold tied maxima, many y are exactly 0.
# name -> (n, h, w, C, training, pooled gradient too)
BN_CASES = {
    "train_16": (2, 32, 64, 16, True, True),
    "train_32": (2, 32, 64, 32, True, True),
    "train_64": (2, 32, 64, 64, True, True),
    "train_256": (2, 32, 64, 256, True, True),
    "train_deep_256": (4, 16, 16, 256, True, True),
    "train_four_16": (4, 32, 32, 16, True, True),
    "eval_odd_16": (3, 21, 37, 16, False, False),
    "eval_ragged_32": (3, 50, 46, 32, False, True),
    # 33 633 pixels x 256 channels: the reduce grid is at its 512-block cap, every thread makes several trips and the last trip of four
    # pixels is cut short by the end of the tensor
    "eval_ragged_wide_256": (3, 111, 101, 256, False, False),
}
BN_N2 = {2: (1, 2), 3: (1, 2), 4: (1, 3)}      # the second gradient's sample range: strictly inside the batch wherever it has three samples


@functools.lru_cache(maxsize=4)
def bn_case(name: str):
    """-> dict(raw, gy, gpool, gy2, n2, gamma, saved)."""
    n, h, w, c, training, pool = BN_CASES[name]
    gamma, saved = make_saved(f"bn/{name}", c)
    n2 = BN_N2[n]
    return dict(raw=ints(f"bn/{name}/raw", (n, c, h, w), -2, 2), gy=ints(f"bn/{name}/gy", (n, c, h, w), -1, 1),
                gpool=ints(f"bn/{name}/gpool", (n, c, h // 2, w // 2), -1, 1) if pool else None,
                gy2=ints(f"bn/{name}/gy2", (n2[1] - n2[0], c, h, w), -1, 1), n2=n2, gamma=gamma, saved=saved)


# miseg_bn_relu_bwd_stats + miseg_conv3x3_dgrad_bn (+ miseg_conv3x3_wgrad_bn).  name -> (n, h, w, K, Cs, training, storage types).
# Training mode: the pixel count is a power of two and gamma, invstd are in {1, 2}, so that graw is a multiple of 2^-10 (1 024 pixels:
# the two means are multiples of 2^-10) and the data gradient's sums of <= 144 of them stay exact in fp32 (asserted per case).
DGRAD_BN_CASES = {
    "eval_tiled_ragged": (3, 20, 36, 32, 16, False, ALL),
    "eval_stream_16": (4, 256, 256, 16, 16, False, HALF),
    "eval_stream_32_16": (4, 256, 256, 32, 16, False, HALF),
    "train_tiled": (1, 16, 64, 16, 16, True, ALL),
    "train_tiled_rows": (1, 32, 32, 16, 16, True, ALL),
    # the fused forms on every tile shape (Cs decides the channels per block; FWD_CASES has the map from size to shape).  pool_*: even
    # sizes and Cs = 64, so that 16-bit storage also has the pooled form (64 channels per block on that tile)
    "eval_t16x16_16_16": (2, 16, 16, 16, 16, False, ALL),
    "eval_t16x16_ragged_16_32": (2, 20, 20, 16, 32, False, ALL),
    "eval_pool_t16x16_64_64": (1, 16, 16, 64, 64, False, ALL),
    "eval_t16x32_8_32": (2, 32, 32, 8, 32, False, ALL),
    "eval_pool_t16x32_ragged_16_64": (1, 36, 40, 16, 64, False, ALL),
    "eval_t8x32_64_16": (1, 64, 64, 64, 16, False, ALL),
    "eval_pool_t8x32_ragged_8_64": (1, 70, 66, 8, 64, False, ALL),
    "eval_t8x16_16_16": (1, 256, 16, 16, 16, False, ALL),
    "eval_pool_t8x16_ragged_16_64": (1, 258, 18, 16, 64, False, ALL),
}


@functools.lru_cache(maxsize=4)
def dgrad_bn_case(name: str):
    n, h, w, k, cs, training, _ = DGRAD_BN_CASES[name]
    vals = (1.0, 2.0) if training else (0.5, 1.0, 2.0)
    gamma, saved = make_saved(f"dgbn/{name}", k, vals, vals)
    return dict(raw=ints(f"dgbn/{name}/raw", (n, k, h, w), -2, 2), gy=ints(f"dgbn/{name}/gy", (n, k, h, w), -1, 1),
                w=ints(f"dgbn/{name}/w", (k, cs, 3, 3), -1, 1), gamma=gamma, saved=saved)


# ----------------------------------------------------------------------------------------------------------------- preconditions
# One per table: what a case asserts on its reference before it touches the GPU (and what test_cpu_exact_ref.py proves for every
# case and storage type on a machine without one).
def fwd_precondition(name: str, dtype) -> None:
    _, _, _, (out, _, _), abs_sum = fwd_case(name)
    assert_exact_range(out, dtype, abs_sum)


def stats_precondition(name: str, dtype) -> None:
    x, wt, (out, s1, s2) = stats_case(name)
    assert_exact_range(out, dtype, 9.0 * x.shape[1])
    assert float(s2.max()) < ACC_LIMIT and float(out.abs().sum((0, 2, 3)).max()) < ACC_LIMIT       # whole-tensor sums: any partition is exact


def stem_precondition(name: str, dtype) -> None:
    img, wt, g, (out, s1, s2), gw = stem_case(name)
    assert_exact_range(out, dtype, 18.0)
    assert float(s2.max()) < ACC_LIMIT
    assert_exact_range(gw, torch.float32, 2.0 * g[:, 0].numel())


def dgrad_precondition(table: str, name: str, dtype) -> None:
    _, _, ref, abs_sum = dgrad_case(table, name)
    assert_exact_range(ref["pooled"] if table == "sumpool" else ref["full"], dtype, abs_sum)


def wgrad_precondition(name: str) -> None:
    _, _, _, gw, abs_sum = wgrad_case(name)
    assert_exact_range(gw, torch.float32, abs_sum)


def bn_reference(name: str, variant: str):
    """bn_bwd_ref of a BN_CASES entry; variant: "plain" (gy only) | "pool" (gy + gpool) | "dual" (gy [+ gpool] + gy2)."""
    c = bn_case(name)
    training = BN_CASES[name][4]
    gpool = c["gpool"] if variant in ("pool", "dual") else None
    gy2 = c["gy2"] if variant == "dual" else None
    return bn_bwd_ref(c["raw"], c["gy"], gpool, gy2, c["n2"], c["gamma"], c["saved"], training)


def bn_precondition(name: str, variant: str, dtype) -> dict:
    """Sums exact in fp32 whatever the partition (multiples of 1/2 whose absolute total is below 2^23), graw exactly representable in
    fp32 before its one rounding, y inside the storage type's range.  Returns the reference."""
    c = bn_case(name)
    ref = bn_reference(name, variant)
    if name == "eval_ragged_wide_256":
        npix = c["raw"].shape[0] * c["raw"].shape[2] * c["raw"].shape[3]
        assert npix > 512 * 64 and npix % 4 != 0
    xhat = (c["raw"] - c["saved"][0].view(1, -1, 1, 1)) * c["saved"][1].view(1, -1, 1, 1)
    assert_exact_range(ref["gbeta"], torch.float32, ref["dz"].abs().sum((0, 2, 3)).max())
    assert_exact_range(ref["ggamma"], torch.float32, (ref["dz"] * xhat).abs().sum((0, 2, 3)).max(), quantum=0.5)
    assert_exact_range(ref["y"], dtype, quantum=0.25)
    round_to(ref["graw"], dtype)            # (asserts fp32 representability)
    return ref


def dgrad_bn_reference(name: str, dtype):
    """-> dict(bn=bn_bwd_ref, coef=the six rows, graw_loaded=graw as the loader hands it to the matrix cores, gx=data gradient, gw=weight
    gradient of a 16-channel input x) for a DGRAD_BN_CASES entry.  The loader (csrc/common.h bn_graw_vec) forms graw in fp32 and packs
    it to the storage type: ONE rounding for bf16 / half, none for fp32."""
    n, h, w, k, cs, training, _ = DGRAD_BN_CASES[name]
    c = dgrad_bn_case(name)
    bn = bn_bwd_ref(c["raw"], c["gy"], None, None, None, c["gamma"], c["saved"], training)
    coef = bwd_coef_ref(c["gamma"], c["saved"], bn["ggamma"], bn["gbeta"], n * h * w, training)
    graw = round_to(bn["graw"], dtype)
    q = quantum_of(graw)
    gx = dgrad_ref(graw, c["w"])["full"]
    abs_sum = F.conv_transpose2d(graw.abs(), c["w"].abs(), None, 1, 1).max()
    assert_exact_range(gx, torch.float32, abs_sum, quantum=q)       # the fp32 accumulator holds every partial sum
    round_to(gx, dtype)
    return dict(bn=bn, coef=coef, graw_loaded=graw, gx=gx, quantum=q)


def dgrad_red_reference(name: str, dtype):
    """The epilogue reduce of miseg_conv3x3_dgrad_bn (csrc/conv_tiled.h, RED) for an evaluation-mode DGRAD_BN_CASES entry: the layer
    that produced the Cs-channel tensor whose gradient the launch writes has raw output `raw` and coefficients `saved`; the epilogue
    takes dz = [raw * scale + shift > 0] * (the gradient AS STORED) and sums dz and dz * xhat per channel.  Everything is a multiple of
    the gradient's quantum / 2 (invstd >= 1/2), and the whole-tensor absolute sums are asserted below 2^24 of it: any partition is exact.
    -> dict(raw, saved, gbeta, ggamma)."""
    n, h, w, k, cs, training, _ = DGRAD_BN_CASES[name]
    assert not training         # (training mode: the gradient is a multiple of 2^-10, whole-tensor sums would leave fp32's exact range)
    ref = dgrad_bn_reference(name, dtype)
    raw = ints(f"dgbn/{name}/red/raw", (n, cs, h, w), -2, 2)
    _, saved = make_saved(f"dgbn/{name}/red", cs)
    v = lambda r: saved[r].view(1, -1, 1, 1)
    dz = (raw * v(2) + v(3) > 0).to(F64) * round_to(ref["gx"], dtype)
    dev = dz * (raw - v(0))
    q = ref["quantum"]
    assert_exact_range(dz.sum((0, 2, 3)), torch.float32, dz.abs().sum((0, 2, 3)).max(), quantum=q)
    assert_exact_range(dev.sum((0, 2, 3)), torch.float32, dev.abs().sum((0, 2, 3)).max(), quantum=q)
    return dict(raw=raw, saved=saved, gbeta=dz.sum((0, 2, 3)), ggamma=dev.sum((0, 2, 3)) * saved[1])


# ---- recipes of the remaining GPU tests (kept here so that test_cpu_exact_ref.py proves them in range too)
SUMPOOL2X2_SHAPES = ((3, 20, 36, 24), (2, 6, 10, 16), (1, 2, 2, 8))


def sumpool2x2_case(shape):
    """-> (x, pre-fill, 2 x 2 sums of x)."""
    n, h, w, ch = shape
    x = ints(f"sumpool2x2/{h}/x", (n, ch, h, w), -8, 8)
    pre = ints(f"sumpool2x2/{h}/pre", (n, ch, h // 2, w // 2), -8, 8)
    return x, pre, F.avg_pool2d(x, 2) * 4


def axpy_sizes(vec: int):
    return vec * 37, vec * (8192 * 256 + 3)         # one partial block; more vectors than the elementwise grid (8192 blocks) has threads


def axpy_case(numel: int):
    return ints(f"axpy/{numel}/a", (numel,), -60, 60), ints(f"axpy/{numel}/b", (numel,), -60, 60)


CAST_PAD_SHAPE = (3, 50, 46)


def cast_pad_case(cin: int):
    """Eighths of magnitude <= 125: ten significant bits, rounded by bf16, exact in half and fp32."""
    n, h, w = CAST_PAD_SHAPE
    return ints(f"cast_pad/{cin}", (n * h * w, cin), -1000, 1000) / 8


WGRAD_BN_NAMES = ("c16_16_16", "gen_32_32", "gen_cat_32_32_32", "remainder_gen")


def wgrad_bn_case(name: str):
    """A WGRAD_CASES entry read as a BatchNorm layer's backward with plain coefficients (scale = 1, shift = 0, mean = 0, A = 1,
    P = Q = 0): -> (raw, reference weight gradient for g = (raw > 0) * gy, worst-case accumulator magnitude)."""
    x0, x1, gy, _, abs_sum = wgrad_case(name)
    raw = ints(f"wgrad_bn/{name}/raw", gy.shape, -2, 2)
    ref = wgrad_ref(x0, WGRAD_CASES[name][4], x1, 0, (raw > 0).to(F64) * gy)
    assert_exact_range(ref, torch.float32, abs_sum)
    return raw, ref


SLICE_CASE = (3, 20, 36, 3, 8, 16)      # (n, h, w, real input channels, padded to, Cout): miseg_conv3x3_wgrad_slice keeps 3 of 8


def slice_case():
    n, h, w, cin, cpad, cout = SLICE_CASE
    x = torch.cat((ints("slice/x", (n, cin, h, w), -2, 2), torch.zeros(n, cpad - cin, h, w, dtype=F64)), 1)
    g = ints("slice/g", (n, cout, h, w), -1, 1)
    gw = wgrad_ref(x, 0, None, 0, g)
    assert_exact_range(gw, torch.float32, 2.0 * n * h * w)
    assert bool((gw[:, :cin] != 0).any()) and not bool((gw[:, cin:] != 0).any())
    return x, g, gw


BN_FWD_CASES = ((3, 20, 36, 16, True), (2, 8, 12, 24, True), (2, 6, 10, 256, True), (3, 21, 37, 16, False))      # (n, h, w, C, pooled)


def bn_fwd_case(case, dtype):
    """-> (raw, saved, y, pooled or None); y inside the storage type's range, many exact zeros, some pre-activation exactly 0."""
    n, h, w, ch, pool = case
    gamma, saved = make_saved(f"bnfwd/{ch}", ch)
    raw = ints(f"bnfwd/{h}/{ch}/raw", (n, ch, h, w), -3, 3)
    y, pooled = bn_fwd_ref(raw, saved, pool)
    assert_exact_range(y, dtype, quantum=0.25)
    assert float((y == 0).double().mean()) > 0.2 and bool((raw * saved[2].view(1, -1, 1, 1) + saved[3].view(1, -1, 1, 1) == 0).any())
    return raw, saved, y, pooled


# The BatchNorm loaders of the data- and weight-gradient kernels with NON-ZERO offsets P, Q at any size: bwd_coef is an input of those
# entry points, so the test hands them integer rows of its own (A in {1, 2, 4}, P and Q in {-1, 0, 1}) instead of the ones a
# training-mode statistics pass would give.  graw = [y > 0] * A * gy + P + Q * (raw - mean) is then an integer of magnitude <= 8:
# nothing is rounded in any storage type, every sum is exact -- and a halo pixel that read P instead of zero would show.
# name -> (kind, n, h, w, K, other channels, storage types); kind "dgrad": K -> Cs data gradient, "wgrad": Cin -> K weight gradient
LOADER_CASES = {
    "dgrad_stream_16_16": ("dgrad", 4, 256, 256, 16, 16, HALF),
    "dgrad_stream_32_16": ("dgrad", 4, 256, 256, 32, 16, HALF),
    "dgrad_stream_ragged_32_32": ("dgrad", 6, 250, 230, 32, 32, HALF),
    "dgrad_tiled_ragged_32_16": ("dgrad", 3, 50, 46, 32, 16, ALL),
    "wgrad_c16_16_16": ("wgrad", 3, 50, 46, 16, 16, ALL),
    "wgrad_gen_32_32": ("wgrad", 3, 50, 46, 32, 32, ALL),
    "wgrad_gen_remainder_64_64": ("wgrad", 5, 50, 70, 64, 64, ALL),
}


@functools.lru_cache(maxsize=2)
def loader_case(name: str):
    """-> dict(raw, gy, coef [6][K], graw, and w + gx (dgrad) or x + gw (wgrad))."""
    kind, n, h, w, k, other, _ = LOADER_CASES[name]
    gamma, saved = make_saved(f"loader/{name}", k, (1.0, 2.0), (1.0, 2.0))
    a = gamma * saved[1]
    p, q = ints(f"loader/{name}/p", (k,), -1, 1), ints(f"loader/{name}/q", (k,), -1, 1)
    coef = torch.stack((saved[2], saved[3], saved[0], a, p, q))
    raw, gy = ints(f"loader/{name}/raw", (n, k, h, w), -2, 2), ints(f"loader/{name}/gy", (n, k, h, w), -1, 1)
    v = lambda t: t.view(1, -1, 1, 1)
    graw = (raw * v(saved[2]) + v(saved[3]) > 0).to(F64) * v(a) * gy + v(p) + v(q) * (raw - v(saved[0]))
    assert float(graw.abs().max()) <= 8 and bool((v(p) != 0).any()) and bool((v(q) != 0).any())
    out = dict(raw=raw, gy=gy, coef=coef, graw=graw)
    if kind == "dgrad":
        out["w"] = ints(f"loader/{name}/w", (k, other, 3, 3), -1, 1)
        out["gx"] = dgrad_ref(graw, out["w"])["full"]
        out["abs_sum"] = 9.0 * k * 8
    else:
        out["x"] = ints(f"loader/{name}/x", (n, other, h, w), -2, 2)
        out["gw"] = wgrad_ref(out["x"], 0, None, 0, graw)
        out["abs_sum"] = 16.0 * n * h * w
    return out


def loader_precondition(name: str, dtype) -> None:
    c = loader_case(name)
    assert_exact_range(c["graw"], dtype)
    if "gx" in c:
        assert_exact_range(c["gx"], dtype, c["abs_sum"])
    else:
        assert_exact_range(c["gw"], torch.float32, c["abs_sum"])
