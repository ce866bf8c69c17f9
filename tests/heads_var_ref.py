"""Shared by tests/test_cpu_heads_var.py and tests/test_gpu_heads_var.py: the case tables of the mlp / normalize cluster-head kernels
(csrc/heads_var.hip), their float64 reference, the same composition in fp32 on the CPU ("torch's own fp32 error", the convention of
test_gpu_contrast.py) and the Python mirror of the launch arithmetic (LDS bytes, blocks, chunks), in the style of contrast_ref.py,
dice_ref.py and exact_heads.py.

The reference is torch autograd over the oracle's composition (oracle/heads.py) in float64 on the CPU:
  local   1x1 conv [-> LeakyReLU(0.01) -> 1x1 conv] [-> F.normalize(dim=1, eps=1e-12)] -> softmax(. / T, dim=1)
  global  AdaptiveAvgPool2d(1) -> Flatten -> the same layers as Linear
on the gathered (``src``) and, for the local head, flipped (``oracle.losses.apply_flips``) features.  The features are the STORED values
(rounded to the storage type, then widened), the parameters fp32 values widened, the cotangent a fixed random tensor, so that the
comparison covers gfeat, gw1, gb1, gw2 and gb2.  Inputs are keyed draws of tests/golden/synth.py; the weights are scaled like a fresh
layer (1 / sqrt(fan-in)) so that the softmax is not saturated (asserted by the CPU test: the largest probability is below 0.9 on most
pixels).

Each shape is the smallest that reaches its branch; the CPU test computes the condition a case exists for from the shapes with the
formulas below and asserts it.
"""
from __future__ import annotations

import functools
from collections import OrderedDict

import torch

import synth
from oracle import heads as OH
from oracle import losses as OL

F64 = torch.float64
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
ALL = (F32, BF16, F16)
KVT = 64                      # kVT of heads_var.hip: pixels (local) or samples (global) per wave
LDS_LIMIT = 150 * 1024        # the refusal limit of every entry point
MAX_BLOCKS = 1024             # local_bwd_blocks' cap
NORM_EPS = 1e-12              # F.normalize's eps and kNormEps
CAP = 1e-4                    # the loosest fp32 gradient bound test_gpu_mi.py uses; 10 x the fp32-torch error never reaches it (CPU test)
OUTPUTS = ("prob", "gfeat", "gw1", "gb1", "gw2", "gb2")


def tname(dtype) -> str:
    return {F32: "f32", BF16: "bf16", F16: "f16"}[dtype]


def cdiv(a: int, b: int) -> int:
    return (a + b - 1) // b


# ----------------------------------------------------------------------------------------------------------------- launch arithmetic
def local_fwd_lds(c: int, hid: int, k: int) -> int:
    """local_fwd_lds(): also the global forward's request."""
    return (c + hid + k) * KVT * 4


def local_bwd_lds(c: int, hid: int, k: int) -> int:
    return (2 * c + 2 * hid + 2 * k) * KVT * 4


def global_bwd_lds(c: int, hid: int, k: int) -> int:
    """miseg_head_global_var_bwd: the local request without the feature-gradient columns."""
    return local_bwd_lds(c, hid, k) - c * KVT * 4


def local_chunks(m: int, h: int, w: int) -> int:
    return m * cdiv(h * w, KVT)


def local_bwd_blocks(m: int, h: int, w: int) -> int:
    return min(local_chunks(m, h, w), MAX_BLOCKS)


def part_floats(c: int, hid: int, k: int) -> int:
    r1 = hid if hid > 0 else k
    return r1 * c + r1 + (k * hid + k if hid > 0 else 0)


def local_bwd_ws_bytes(m: int, h: int, w: int, c: int, hid: int, s: int, k: int) -> int:
    return (local_bwd_blocks(m, h, w) + 1) * s * part_floats(c, hid, k) * 4


def feat_kernel_chunks(h: int, w: int, c: int) -> int:
    """gridDim.y of head_global_var_feat_kernel."""
    return max(1, min(32, cdiv(h * w * c, 256 * 8)))


# ----------------------------------------------------------------------------------------------------------------- the cases
def _case(B, M, C, HID, K, S, H, W, T, normalize, types, src, flips=None, fwd_only=False, zero=None):
    assert len(src) == M and len(set(src)) == M and all(0 <= i < B for i in src)
    assert flips is None or (len(flips) == M and all(0 <= f < 4 for f in flips))
    return dict(B=B, M=M, C=C, HID=HID, K=K, S=S, H=H, W=W, T=T, normalize=normalize, types=tuple(types), src=list(src),
                flips=None if flips is None else list(flips), fwd_only=fwd_only, zero=zero)


_STRIDE = dict(B=7, M=6, C=8, K=6, S=3, H=120, W=110, T=0.5, types=ALL, src=[5, 0, 6, 2, 1, 4], flips=[0, 1, 2, 3, 1, 0])
LOCAL_CASES = OrderedDict([
    # 6 x 207 = 1242 chunks against 1024 blocks: blocks 0..217 take a second chunk; 13200 mod 64 = 16: every sample ends on a partial chunk
    ("stride_mlp_norm", _case(HID=64, normalize=True, **_STRIDE)),
    ("stride_mlp", _case(HID=64, normalize=False, **_STRIDE)),
    ("stride_lin_norm", _case(HID=0, normalize=True, **_STRIDE)),
    # one partial chunk per sample; backward LDS 103 KiB
    ("upconv5", _case(3, 3, 128, 64, 10, 2, 7, 9, 1.0, True, ALL, [2, 0, 1], [3, 1, 2])),
    ("upconv2", _case(5, 4, 16, 64, 20, 5, 24, 20, 2.0, False, ALL, [4, 1, 0, 3], [1, 2, 3, 0])),
    # the variant kernels as a second implementation of the linear head
    ("plain", _case(3, 2, 16, 0, 6, 2, 9, 13, 0.5, False, (F32, F16), [2, 0], [2, 1])),
    # backward LDS exactly 150 x 1024 bytes; the forward-only companion has C + HID + K = 600
    ("lds_limit", _case(3, 2, 128, 128, 44, 1, 8, 8, 1.0, True, (F32, F16), [2, 0], [1, 2])),
    ("lds_limit_fwd", _case(3, 2, 280, 256, 64, 1, 8, 8, 1.0, True, (F32, BF16), [2, 0], [1, 2], fwd_only=True)),
    # logits that are exactly zero: the nrm <= eps branch.  "pixels": b1 = 0 and a handful of all-zero feature columns;
    # "subhead": w2 = b2 = 0 in sub-head 1.  bf16, not fp16: the gradient there is g / 1e-12, beyond fp16's range.
    ("zero_norm_lin", _case(3, 2, 8, 0, 6, 2, 5, 7, 1.0, True, (F32, BF16), [2, 0], [3, 0], zero="pixels")),
    ("zero_norm_mlp", _case(3, 2, 8, 64, 6, 2, 5, 7, 1.0, True, (F32, BF16), [2, 0], [3, 0], zero="subhead")),
])

_MLOOP = dict(B=151, M=150, C=32, K=6, S=2, H=3, W=1, T=1.0, normalize=True, types=ALL, src=[(7 * i + 3) % 151 for i in range(150)])
GLOBAL_CASES = OrderedDict([
    # forward LDS 98.5 KiB, backward 133 KiB; the feature kernel runs with 2 chunks
    ("conv5", _case(6, 5, 256, 128, 10, 3, 4, 4, 0.5, True, ALL, [4, 0, 5, 2, 1])),
    # three passes of 64 samples with a tail of 22; HW = 3 < the pool's four partial sums
    ("mloop_mlp", _case(HID=128, **_MLOOP)),
    ("mloop_lin", _case(HID=0, **_MLOOP)),
    # K at its limit, C no multiple of 64 (the pool's grid.y guard), a 1 x 1 map
    ("kmax", _case(4, 4, 70, 0, 64, 1, 1, 1, 0.5, True, (F32, F16), [3, 1, 0, 2])),
    # the feature kernel at its cap of 32 chunks (16 * 16 * 256 / 2048 = 32)
    ("featcap", _case(3, 2, 256, 128, 6, 2, 16, 16, 1.0, False, (F32, BF16), [2, 0])),
    ("zero_norm_lin", _case(5, 4, 8, 0, 6, 2, 2, 3, 1.0, True, (F32, BF16), [4, 0, 3, 1], zero="pixels")),
    ("zero_norm_mlp", _case(5, 4, 8, 128, 6, 2, 2, 3, 1.0, True, (F32, BF16), [4, 0, 3, 1], zero="subhead")),
])
TABLES = {"local": LOCAL_CASES, "global": GLOBAL_CASES}
# the cases that also run through LocalClusterHead / ClusterHead (the state-dict stacking on the path)
MODULE_CASES = [("local", "upconv5", F32), ("local", "upconv2", F16), ("local", "stride_lin_norm", BF16),
                ("global", "conv5", BF16), ("global", "mloop_lin", F32), ("global", "mloop_mlp", F16)]


def pairs(kind: str):
    return [(n, d) for n, c in TABLES[kind].items() for d in c["types"]]


def pair_ids(kind: str):
    return [f"{n}-{tname(d)}" for n, d in pairs(kind)]


# ----------------------------------------------------------------------------------------------------------------- inputs
def _T(a):
    return torch.from_numpy(a)


@functools.lru_cache(maxsize=None)
def inputs(kind: str, name: str):
    """-> dict(feat [B,C,H,W] fp32 (before the rounding to a storage type), w1 [S,R,C], b1 [S,R], w2 [S,K,HID] | None, b2, cot): fp32."""
    c = TABLES[kind][name]
    tag = f"heads_var/{kind}/{name}"
    B, M, C, HID, K, S, H, W = (c[k] for k in ("B", "M", "C", "HID", "K", "S", "H", "W"))
    r1 = HID if HID else K
    feat = _T(synth.normal(tag + "/feat", (B, C, H, W)))
    w1 = _T(synth.normal(tag + "/w1", (S, r1, C), scale=C ** -0.5))
    b1 = _T(synth.normal(tag + "/b1", (S, r1), scale=0.1))
    w2 = _T(synth.normal(tag + "/w2", (S, K, HID), scale=HID ** -0.5)) if HID else None
    b2 = _T(synth.normal(tag + "/b2", (S, K), scale=0.1)) if HID else None
    if c["zero"] == "pixels":
        b1 = torch.zeros_like(b1)
        if kind == "local":                      # a handful of all-zero feature columns in the rows that src names
            for i, (y, x) in zip(c["src"] + c["src"], [(0, 0), (H - 1, W - 1), (2, 3), (1, 5)]):
                feat[i, :, y, x] = 0
        else:                                    # a sample whose pooled feature is zero
            feat[c["src"][1]] = 0
    elif c["zero"] == "subhead":
        w2[1], b2[1] = 0, 0
    cot = _T(synth.normal(tag + "/cot", (S, M, K, H, W) if kind == "local" else (S, M, K)))
    return dict(feat=feat, w1=w1, b1=b1, w2=w2, b2=b2, cot=cot)


def stored_feat(kind: str, name: str, dtype):
    """The features as the kernel reads them: rounded once to the storage type."""
    return inputs(kind, name)["feat"].to(dtype)


def decisions(flips):
    """Flip codes (bit 0 = H, bit 1 = W) -> the oracle's [[flip_h, flip_w], ...]."""
    return [[bool(f & 1), bool(f & 2)] for f in flips]


def state_dict(kind: str, w1, b1, w2, b2):
    """Stacked parameters -> the reference module tree's keys (views: autograd reaches the stacked leaves)."""
    first, second = (0, 2) if kind == "local" else (2, 4)
    shape = (lambda w: w[..., None, None]) if kind == "local" else (lambda w: w)
    sd = OrderedDict()
    for s in range(w1.shape[0]):
        sd[f"_headers.{s}.{first}.weight"], sd[f"_headers.{s}.{first}.bias"] = shape(w1[s]), b1[s]
        if w2 is not None:
            sd[f"_headers.{s}.{second}.weight"], sd[f"_headers.{s}.{second}.bias"] = shape(w2[s]), b2[s]
    return sd


def compose(kind: str, case, feat, w1, b1, w2, b2):
    """The oracle's composition on the gathered, flipped features in the dtype of its arguments -> prob [S,M,K(,H,W)]."""
    x = feat[torch.tensor(case["src"])]
    if kind == "local":
        if case["flips"] is not None:
            x = OL.apply_flips(x, decisions(case["flips"]))
        outs = OH.local_cluster_head(state_dict(kind, w1, b1, w2, b2), x, case["T"], case["normalize"])
    else:
        outs = OH.cluster_head(state_dict(kind, w1, b1, w2, b2), x, case["T"], case["normalize"])
    return torch.stack(outs)


def evaluate(kind: str, case, feat, w1, b1, w2, b2, cot, fn=compose):
    """Forward + autograd of ``fn`` in the dtype of ``w1`` -> {prob, gfeat [B,C,H,W], gw1, gb1[, gw2, gb2]} (forward-only: prob)."""
    dt = w1.dtype
    leaves = OrderedDict((k, v.detach().to(dt).clone().requires_grad_(True))
                         for k, v in (("gfeat", feat), ("gw1", w1), ("gb1", b1), ("gw2", w2), ("gb2", b2)) if v is not None)
    prob = fn(kind, case, leaves["gfeat"], leaves["gw1"], leaves["gb1"], leaves.get("gw2"), leaves.get("gb2"))
    out = {"prob": prob.detach()}
    if not case["fwd_only"]:
        (prob * cot.to(dt)).sum().backward()
        out.update((k, v.grad) for k, v in leaves.items())
    return out


def rel(got, ref) -> float:
    """max |got - ref| / max |ref|: _rel of test_gpu_contrast.py."""
    return float((got.double() - ref).abs().max() / ref.abs().max())


@functools.lru_cache(maxsize=None)
def reference(kind: str, name: str, dtype):
    """-> dict(ref = the float64 outputs, fp32 = the fp32-torch outputs' errors against them, bound = min(10 x fp32 error, CAP) per
    output).  Computed once per (case, storage type) and shared; treat as read-only."""
    case, x = TABLES[kind][name], inputs(kind, name)
    feat = stored_feat(kind, name, dtype)
    wide = lambda t, d: None if t is None else t.to(d)     # noqa: E731
    ref = evaluate(kind, case, feat.to(F64), *(wide(x[k], F64) for k in ("w1", "b1", "w2", "b2")), x["cot"])
    low = evaluate(kind, case, feat.to(F32), *(x[k] for k in ("w1", "b1", "w2", "b2")), x["cot"])
    fp32 = {k: rel(low[k], ref[k]) for k in ref}
    return dict(ref=ref, fp32=fp32, bound={k: min(10.0 * v, CAP) for k, v in fp32.items()})


def half_ulp(ref, dtype):
    """Half a unit in the last place of the storage type at |ref| (float64, element-wise): 2^(floor(log2 |ref|) - p) with p = 8
    significand bits for bf16, 11 for fp16 (the exponent clamped at the type's smallest normal one); 0 for fp32, which is not rounded."""
    if dtype == F32:
        return torch.zeros_like(ref)
    p, emin = (8, -126) if dtype == BF16 else (11, -14)
    _, e = torch.frexp(ref.abs())                   # |ref| = m 2^e with m in [0.5, 1)
    return torch.ldexp(torch.ones_like(ref), (e - 1).clamp_min(emin) - p)


# ----------------------------------------------------------------------------------------------------------------- second evaluation
def compose_modules(kind: str, case, feat, w1, b1, w2, b2, raw_logits=False):
    """The same function from torch.nn modules given the same parameters, with a gather / flip of its own (index arithmetic, no
    apply_flips) and the normalisation written out: the independent float64 evaluation the CPU test holds the reference against.
    ``raw_logits``: the logits before the normalisation instead."""
    import torch.nn as nn
    K, HID, C = case["K"], case["HID"], case["C"]
    rows = []
    for m, i in enumerate(case["src"]):
        g = feat[i]
        f = case["flips"][m] if (kind == "local" and case["flips"] is not None) else 0
        if f & 1:
            g = g[:, torch.arange(case["H"] - 1, -1, -1)]
        if f & 2:
            g = g[:, :, torch.arange(case["W"] - 1, -1, -1)]
        rows.append(g)
    x = torch.stack(rows)
    outs = []
    for s in range(case["S"]):
        if kind == "local":
            l1 = nn.Conv2d(C, HID or K, 1).to(w1.dtype)
            l2 = nn.Conv2d(HID, K, 1).to(w1.dtype) if HID else None
            pre = []
        else:
            l1 = nn.Linear(C, HID or K).to(w1.dtype)
            l2 = nn.Linear(HID, K).to(w1.dtype) if HID else None
            pre = [nn.AdaptiveAvgPool2d((1, 1)), nn.Flatten()]
        del l1.weight, l1.bias                               # the caller's tensors stand in for the parameters: autograd reaches them
        l1.weight, l1.bias = w1[s].view(HID or K, C, *((1, 1) if kind == "local" else ())), b1[s]
        layers = pre + [l1]
        if HID:
            del l2.weight, l2.bias
            l2.weight, l2.bias = w2[s].view(K, HID, *((1, 1) if kind == "local" else ())), b2[s]
            layers += [nn.LeakyReLU(0.01), l2]
        z = nn.Sequential(*layers)(x)
        if raw_logits:                                       # before the normalisation and the softmax
            outs.append(z)
            continue
        if case["normalize"]:
            z = z / torch.linalg.vector_norm(z, dim=1, keepdim=True).clamp_min(NORM_EPS)     # its subgradient at 0 is 0, as in F.normalize
        outs.append(nn.Softmax(dim=1)(z / case["T"]))
    return torch.stack(outs)
