"""Shared by tests/test_cpu_mi_local_plan.py and tests/test_gpu_mi_local_variants.py: the case table, shapes, windows, inputs and
float64 references of the local-MI contraction kernels of csrc/mi_local.hip -- joint_fwd_kernel<4,4> / <9,9> with 1 .. 7 sub-blocks per
dimension of D and the four staged tiles, joint_reduce_kernel, local_bwd2_kernel<4> / <9> (col2im by plain read-modify-write or by LDS
atomics), local_bwd_kernel<4> / <2> / <1> (gradient matrix in LDS or read from global memory) -- and of the plain-bf16 kernels
(precision "bf16").  Needs no GPU; tests/mi_loss_ref.py is the model.

Which kernel runs is decided from (K, pad) alone by plan_joint / plan_bwd (csrc/mi_local.h).  The library reports that decision through
miseg_iic_local_joint_plan / miseg_iic_local_bwd_plan (include/miseg_hip.h); ``joint_plan`` / ``bwd_plan`` below decode them, and the
table is checked against them, never against a copy of the arithmetic: test_cpu_mi_local_plan.py enumerates K = 1 .. 64, pad = 0 .. 7
and fails when a variant exists that no row of VARIANT_CASES reaches.

Shapes.  Per row a SMALL map (N = 2, H = 11, W = widest tile of the two plans + a ragged rest: 70 / 40 / 20) and, for K <= 32, a WALKING
map (N, K, 48, 70) with N the smallest count >= 6 at which a forward block takes a second item (N tr tc > G) and a backward block a
second (window, direction) key (2 sum_p N ceil(h_p / 4) ceil(w_p / WB) > 256).  Windows: the whole image, or two disjoint crops that
touch no border and start at no tile boundary, with a 0/1 mask and the per-window scales 0.5 and 2.

References, all float64 on oracle/iic.py: local_joint_raw per window on the masked maps; the whole loss by local_mi_from_raw; the
backward alone as autograd of sum_p scale[p] <G_p, local_joint_raw((x m)[win_p], (y m)[win_p])>.

Integer inputs (x, y in 0 .. 3, G in -3 .. 3, mask 0/1, scales 0.5 and 2, prefill in -4 .. 4): every product and partial sum is an
integer below 2^24 (``int_sum_bounds``), so fp32 kernels in any summation order, and bf16 operands, give the float64 result bit for bit.
"""
from __future__ import annotations

import functools
from collections import namedtuple

import torch

import synth
from oracle import iic as OI

F64, F32 = torch.float64, torch.float32
SCALES = (0.5, 2.0)
PRECISIONS = {"fp32": 0, "bf16": 2}

# ----------------------------------------------------------------------------------------------------------------- the table
# (name, K, pad).  The name states the variant the row is there for: forward <cap> sb<sub-blocks> <tile> | backward kind.
VARIANT_CASES = [
    ("f9_sb2_8x64__direct2_lds", 21, 3),
    ("f9_sb2_8x64_ragged__direct4_glb", 25, 3),
    ("f9_sb2_4x64__direct4_glb", 32, 3),
    ("f9_sb2_4x64__direct2_lds", 32, 2),
    ("f9_sb2_8x64__direct1_lds", 20, 4),
    ("f9_sb3_4x64__direct4_glb", 27, 5),
    ("f9_sb3_4x32__direct4_glb", 31, 6),
    ("f9_sb4_4x32__direct2_glb", 32, 7),
    ("f9_sb1_8x64__bwd2x9_atomic", 12, 3),
    # forward only (the backward takes K <= 32)
    ("f4_sb1_4x64", 40, 0),
    ("f9_sb1_4x64", 48, 1),
    ("f9_sb2_4x32", 64, 1),
    ("f9_sb4_4x32_k64", 64, 3),
    ("f9_sb5_4x32", 39, 7),
    ("f9_sb6_4x32", 49, 7),
    ("f9_sb6_4x16", 60, 6),
    ("f9_sb7_4x16", 58, 7),
    # controls: one row of each variant the suite already ran
    ("ctl_f9_sb1_8x64__bwd2x9_rmw", 20, 3),
    ("ctl_f4_sb1_8x64__bwd2x4_atomic", 8, 3),
    ("ctl_f4_sb1_8x64__bwd2x4_rmw", 5, 2),
    ("ctl_f9_sb1_8x64__direct4_lds", 29, 1),
]
BWD_CASES = [c for c in VARIANT_CASES if c[1] <= 32]
FWD_ONLY_CASES = [c for c in VARIANT_CASES if c[1] > 32]
BF16_CASES = [("bf16_rows_pad1", 20, 1), ("bf16_rows_pad3", 20, 3)]       # precision "bf16": px forward / rows backward with one product
HEADS_CASES = [("f9_sb2_8x64__direct2_lds", 21, 3), ("f9_sb2_4x64__direct2_lds", 32, 2)]    # an sb = 2 forward, a direct<2> backward
K_ENUM, PAD_ENUM = range(1, 65), range(0, 8)

JointPlan = namedtuple("JointPlan", "cap sb tps RB WB G")
BwdPlan = namedtuple("BwdPlan", "kind width g_in_lds plain_rmw WB")
ROWS, BWD2, DIRECT = 1, 2, 3


def _lib():
    from miseg_amd import _cabi
    return _cabi.lib()


def joint_plan(n, k, h, w, pad, p):
    """miseg_iic_local_joint_plan decoded, None where the forward refuses."""
    v = int(_lib().miseg_iic_local_joint_plan(n, k, h, w, pad, p))
    return None if v < 0 else JointPlan(v & 255, (v >> 8) & 255, (v >> 16) & 255, (v >> 24) & 255, (v >> 32) & 255, (v >> 40) & 0xffff)


def bwd_plan(n, k, h, w, pad, p, masked=False, precision="fp32"):
    """miseg_iic_local_bwd_plan decoded, None where the backward refuses."""
    v = int(_lib().miseg_iic_local_bwd_plan(n, k, h, w, pad, p, int(masked), PRECISIONS[precision]))
    return None if v < 0 else BwdPlan(v & 15, (v >> 4) & 15, (v >> 8) & 1, (v >> 9) & 1, (v >> 16) & 255)


def fwd_key(jp):
    return None if jp is None else (jp.cap, jp.sb, jp.RB, jp.WB)


def bwd_key(bp):
    return None if bp is None else (bp.kind, bp.width, bp.g_in_lds, bp.plain_rmw)


# ----------------------------------------------------------------------------------------------------------------- shapes, windows
def _plans(k, pad, n=2, h=11, w=70):
    return joint_plan(n, k, h, w, pad, 1), (bwd_plan(n, k, h, w, pad, 1) if k <= 32 else None)


def small_shape(k, pad):
    """(2, K, 11, W): at least two column tiles in the forward and in the backward, the last one ragged."""
    jp, bp = _plans(k, pad)
    wb = max(jp.WB, bp.WB if bp is not None else 0)
    return 2, k, 11, {16: 20, 32: 40}.get(wb, 70)


def windows(h, w, kind):
    if kind == "whole":
        return [(0, h, 0, w)]
    split = 37 if w >= 70 else w // 2
    return [(1, h - 2, 3, split), (2, h - 1, split + 4, w - 2)]


def fwd_items(n, h, w, wins, jp):
    """Items of the busiest window's slot (a block takes a second one when this exceeds G)."""
    return max(n * -(-(h1 - h0) // jp.RB) * -(-(w1 - w0) // jp.WB) for h0, h1, w0, w1 in wins)


def bwd_items(n, wins, bp):
    return 2 * sum(n * -(-(h1 - h0) // 4) * -(-(w1 - w0) // bp.WB) for h0, h1, w0, w1 in wins)


def walking_shape(k, pad):
    """(N, K, 48, 70) with the smallest N >= 6 at which both walking conditions hold on the whole-image window."""
    h, w = 48, 70
    for n in range(6, 64):
        jp, bp = joint_plan(n, k, h, w, pad, 1), bwd_plan(n, k, h, w, pad, 1)
        wins = windows(h, w, "whole")
        if fwd_items(n, h, w, wins, jp) > jp.G and bwd_items(n, wins, bp) > 256:
            return n, k, h, w
    raise AssertionError((k, pad))


def shape_of(k, pad, which):
    return small_shape(k, pad) if which == "small" else walking_shape(k, pad)


# ----------------------------------------------------------------------------------------------------------------- inputs
def _T(a):
    return torch.from_numpy(a)


@functools.lru_cache(maxsize=None)
def real_inputs(shape):
    """-> (x, y) fp32 peaked, correlated simplexes and the 0/1 mask [N,1,H,W]."""
    tag = "mi_local/real/" + "_".join(map(str, shape))
    x, y = synth.peaked_pair(tag, shape)
    return _T(x), _T(y), _T(synth.mask(tag + "/mask", (shape[0], 1) + tuple(shape[2:])))


@functools.lru_cache(maxsize=None)
def int_inputs(shape, pad, nwin):
    """-> dict(x, y in 0..3, mask 0/1, G [P,T,T,K,K] in -3..3, prefill_x / prefill_y in -4..4), fp32 tensors holding integers."""
    n, k, h, w = shape
    t = 2 * pad + 1
    tag = "mi_local/int/" + "_".join(map(str, shape)) + f"_p{pad}_w{nwin}"
    f = lambda name, shp, high, off=0: (_T(synth.integers(tag + name, shp, high)) - off).to(F32)
    return dict(x=f("/x", shape, 4), y=f("/y", shape, 4), mask=_T(synth.mask(tag + "/mask", (n, 1, h, w))),
                G=f("/G", (nwin, t, t, k, k), 7, 3), prefill_x=f("/px", shape, 9, 4), prefill_y=f("/py", shape, 9, 4))


def int_sum_bounds(shape, pad):
    """Largest |sum| an output of the integer runs can reach: raw joint N H W 9, backward T T K 9 (x 2 for the scale, + 4 prefill)."""
    n, k, h, w = shape
    t = 2 * pad + 1
    return n * h * w * 9, t * t * k * 9 * 2 + 4


# ----------------------------------------------------------------------------------------------------------------- references
def ref_joint(x, y, pad, wins, mask=None):
    """float64 raw[P][T][T][K][K] of (x m, y m) cropped to each window."""
    x, y = x.to(F64), y.to(F64)
    if mask is not None:
        x, y = x * mask.to(F64), y * mask.to(F64)
    return torch.stack([OI.local_joint_raw(x[:, :, h0:h1, w0:w1], y[:, :, h0:h1, w0:w1], pad) for h0, h1, w0, w1 in wins])


def ref_bwd(x, y, pad, wins, grad_raw, scales, mask=None):
    """float64 (gx, gy) of sum_p scale[p] <G_p, raw_p> through the crop, the zero padding and the mask."""
    x, y = x.detach().to(F64, copy=True).requires_grad_(True), y.detach().to(F64, copy=True).requires_grad_(True)
    raw = ref_joint(x, y, pad, wins, mask)
    s = torch.tensor(list(scales), dtype=F64).view(-1, 1, 1, 1, 1)
    gx, gy = torch.autograd.grad((raw * grad_raw.to(F64) * s).sum(), [x, y])
    return gx, gy


def ref_whole(x, y, pad, wins, scales, mask=None, dtype=F64, lamda=1.0):
    """The whole op in ``dtype``: dict(loss [P], gx, gy of sum_p scale[p] loss[p], grad_raw [P,T,T,K,K] = d loss[p] / d raw[p]), as float64."""
    x, y = x.detach().to(dtype, copy=True).requires_grad_(True), y.detach().to(dtype, copy=True).requires_grad_(True)   # never the cached inputs
    m = None if mask is None else mask.to(dtype)
    xm, ym = (x, y) if m is None else (x * m, y * m)
    raws = [OI.local_joint_raw(xm[:, :, h0:h1, w0:w1], ym[:, :, h0:h1, w0:w1], pad) for h0, h1, w0, w1 in wins]
    loss = torch.stack([OI.local_mi_from_raw(r, lamda) for r in raws])
    s = torch.tensor(list(scales), dtype=dtype)
    gx, gy = torch.autograd.grad((loss * s).sum(), [x, y])
    grad_raw = torch.stack([OI.local_mi_grad_wrt_raw(r.detach(), lamda) for r in raws])
    return dict(loss=loss.detach().to(F64), gx=gx.to(F64), gy=gy.to(F64), grad_raw=grad_raw.to(F64), raw=torch.stack(raws).detach().to(F64))


def scales_for(wins):
    return SCALES[:len(wins)] if len(wins) > 1 else (1.0,)


@functools.lru_cache(maxsize=None)
def real_reference(shape, pad, kind, fp32_too=True):
    """Shared float64 reference of the real-valued runs of one (shape, pad, window set): the whole op, plus the fp32 oracle's own loss.
    Computed once; treat as read-only."""
    x, y, mask = real_inputs(shape)
    wins = windows(shape[2], shape[3], kind)
    m = mask if kind == "crops" else None
    ref = ref_whole(x, y, pad, wins, scales_for(wins), m)
    if fp32_too:
        ref["loss_fp32"] = ref_whole(x, y, pad, wins, scales_for(wins), m, dtype=F32)["loss"]
    return ref


def to_bf16(t):
    """The rounding of f32_to_bf16_bits (csrc/common.h: __float2bfloat16, round to nearest even), back in fp32."""
    return t.to(torch.bfloat16).to(F32)
