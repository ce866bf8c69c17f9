"""float64 references, dyadic input recipes and the dispatch mirror of the cluster-head tests (test_cpu_exact_heads.py,
test_gpu_exact_heads.py, test_gpu_heads_fp64.py), in the style of exact_ref.py.

The head backward kernels (csrc/heads_bwd.hip, csrc/heads_bwd_fused.h, csrc/heads_global.hip) take the probabilities and their gradient as INPUTS.  Their arithmetic is
dot = sum_k g p, dz = p (g - dot) / T, a hi + lo split of dz and of W into the 16-bit type, matrix-core sums in fp32 and one rounding
to the storage type.  On dyadic inputs every one of these steps is exact: p = j / den on the simplex, g and the features small integers,
W small integers (or multiples of 1/64), T a power of two.  Every product and partial sum is then a multiple of one power of two and
below 2^24 of it, so the fp32 accumulators hold it in whatever order a kernel adds, and the HIP result must EQUAL the float64 reference
at every element.  Everything here is plain torch / numpy on the CPU.

The denominators.  dz = p (g - dot) / T has the numerator j * i with j <= den and |i| <= 4 den (|g - dot| <= 4).  A 16-bit type with
t significand bits (bf16 8, half 11) splits dz into hi + lo; lo is non-zero only where j * i needs more than t bits.  With den = 8 the
numerator is at most 256, which bf16 holds in ONE piece: the lo plane -- and the matrix-core instructions that consume it -- would
never see a non-zero value; with den = 32 the same holds for half (numerators up to 4096 = 2^12 with few low bits set: measured share
of non-zero lo entries 0).  The 16-bit recipes therefore use den = 64 (bf16: numerators up to 2^14, hi + lo holds 16 bits) and den = 128
(half: up to 2^16, hi + lo holds 22 bits), with the mass of a pixel on three classes so that j is large; fp32, which has no split, keeps
den = 8.  The CPU test asserts the share of non-zero lo entries among the non-zero dz (LO_SHARE) for every 16-bit case of the "dz" recipe.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

import exact_ref as R
import synth

F64 = torch.float64
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
ALL, HALF = R.ALL, R.HALF
ACC_LIMIT = R.ACC_LIMIT
DEN = {F32: 8, BF16: 64, F16: 128}     # prob = j / DEN[storage type] in the "dz" recipe
LO_SHARE = 0.25                        # "dz" recipe: at least this share of the non-zero dz entries has a non-zero lo part
W_LO_SHARE = 0.4                       # "w" recipe: at least this share of the weights has a non-zero lo part
W_RANGE = {BF16: 1023, F16: 16383}     # "w" recipe: W = n / 64 with |n| <= this (10 bits > bf16's 8, 14 bits > half's 11)


def tname(dtype) -> str:
    return {F32: "float", BF16: "bf16", F16: "f16"}[dtype]


def cdiv(a: int, b: int) -> int:
    return (a + b - 1) // b


# ----------------------------------------------------------------------------------------------------------------- inputs
def simplex(tag: str, s: int, m: int, k: int, h: int, w: int, den: int, peaks: int = 3) -> torch.Tensor:
    """prob [S][M][K][H][W] float64: at every (sub-head, sample, pixel) `den` units are spread over `peaks` distinct classes (some may get
    none), every entry is j / den and the K entries sum to exactly 1."""
    rs = np.random.RandomState(synth._seed("exact_heads/" + tag))
    n, peaks = s * m * h * w, min(peaks, k)
    weights = np.arange(peaks, 0, -1, dtype=np.float64)
    counts = rs.multinomial(den, weights / weights.sum(), size=n).astype(np.float64)
    cls = np.argsort(rs.random_sample((n, k)), axis=1)[:, :peaks]
    p = np.zeros((n, k))
    np.put_along_axis(p, cls, counts, axis=1)
    return torch.from_numpy(p / den).view(s, m, h, w, k).permute(0, 1, 4, 2, 3).contiguous()


def pick_src(b: int, m: int):
    """M distinct rows out of [1, B - 1), not monotone: B = M + 2 leaves row 0 and row B - 1 untouched (the guard rows of the compact
    form with row0 = 1)."""
    assert b == m + 2
    rows = list(range(1, m + 1))
    out = []
    while rows:
        out.append(rows.pop())
        if rows:
            out.append(rows.pop(0))
    assert sorted(out) == list(range(1, m + 1)) and out != sorted(out)
    return out


def flip_sets(m: int):
    """Flip masks per sample such that a case sees all four masks: one assignment for M >= 4, two for smaller M."""
    a = [(i + 1) % 4 for i in range(m)]
    return (a,) if m >= 4 else (a, [(i + 3) % 4 for i in range(m)])


# ----------------------------------------------------------------------------------------------------------------- references
def gather_flip(feat, src, flips):
    """feat [B][C][H][W] -> [M][C][H][W]: sample m is row src[m], mirrored in H if flips[m] & 1 and in W if flips[m] & 2."""
    out = []
    for i, f in zip(src, flips):
        g = feat[i]
        dims = [d for d, on in ((1, f & 1), (2, f & 2)) if on]
        out.append(g.flip(dims) if dims else g)
    return torch.stack(out)


def dz_ref(prob, gprob, T: float, method: str = "formula"):
    """The gradient of the logits, dz = p (g - <g, p>) / T, over the class axis 2.  "autograd": float64 autograd through the softmax of
    logits that reproduce prob: q = p exp(u / T) / sum_k p exp(u / T) is softmax((log p + u) / T) and equals p at u = 0."""
    p, g = prob.to(F64), gprob.to(F64)
    if method == "formula":
        return p * (g - (g * p).sum(2, keepdim=True)) / T
    assert method == "autograd", method
    u = torch.zeros_like(p, requires_grad=True)
    q = p * torch.exp(u / T)
    ((q / q.sum(2, keepdim=True)) * g).sum().backward()
    return u.grad


def head_local_bwd_ref(feat, w, src, flips, T, prob, gprob, method: str = "einsum"):
    """Backward of S x (1 x 1 conv C -> K, softmax(. / T)) on the gathered, flipped features, float64.
    feat [B][C][H][W], w [S][K][C], prob / gprob [S][M][K][H][W] -> (gfeat [B][C][H][W], gw [S][K][C], gb [S][K]).  Rows of gfeat that
    are not in src are "untouched": zero here, whatever the caller left there on the device.
    "einsum": the sums written out.  "autograd": float64 autograd of sum g softmax((W f + b) / T) with the logits shifted so that the
    softmax is prob (see dz_ref): gather, flip, convolution and softmax all differentiated by torch."""
    feat, w, p, g = feat.to(F64), w.to(F64), prob.to(F64), gprob.to(F64)
    if method == "einsum":
        ft = gather_flip(feat, src, flips)
        dz = dz_ref(p, g, T)
        gw = torch.einsum("smkhw,mchw->skc", dz, ft)
        gb = dz.sum((1, 3, 4))
        gt = torch.einsum("skc,smkhw->mchw", w, dz)
        gfeat = torch.zeros_like(feat)
        for m, (i, f) in enumerate(zip(src, flips)):
            dims = [d for d, on in ((1, f & 1), (2, f & 2)) if on]
            gfeat[i] = gt[m].flip(dims) if dims else gt[m]          # a mirror is its own inverse
        return gfeat, gw, gb
    assert method == "autograd", method
    fa, wa = feat.clone().requires_grad_(True), w.clone().requires_grad_(True)
    ba = torch.zeros(w.shape[:2], dtype=F64, requires_grad=True)
    z = torch.einsum("skc,mchw->smkhw", wa, gather_flip(fa, src, flips)) + ba[:, None, :, None, None]
    q = p * torch.exp((z - z.detach()) / T)
    ((q / q.sum(2, keepdim=True)) * g).sum().backward()
    return fa.grad, wa.grad, ba.grad


def pool_ref(feat, src):
    """Global average pool of the gathered samples: [B][C][H][W] -> [M][C]."""
    return feat.to(F64)[list(src)].mean((2, 3))


def head_global_bwd_ref(pooled, w, src, HW: int, T, prob, gprob, method: str = "einsum"):
    """Backward of S x (Linear C -> K on the pooled feature, softmax(. / T)).  pooled [M][C], w [S][K][C], prob / gprob [S][M][K]
    -> (gvec [M][C], gw, gb): every pixel of row src[m] of gfeat receives gvec[m] (the average pool's backward), other rows are untouched."""
    assert len(set(src)) == len(src)
    pooled, w, p, g = pooled.to(F64), w.to(F64), prob.to(F64), gprob.to(F64)
    if method == "einsum":
        dz = dz_ref(p, g, T)
        return torch.einsum("skc,smk->mc", w, dz) / HW, torch.einsum("smk,mc->skc", dz, pooled), dz.sum(1)
    assert method == "autograd", method
    fa = pooled.clone()[:, :, None].repeat(1, 1, HW).requires_grad_(True)      # HW equal pixels: their mean is `pooled`
    wa = w.clone().requires_grad_(True)
    ba = torch.zeros(w.shape[:2], dtype=F64, requires_grad=True)
    z = torch.einsum("skc,mc->smk", wa, fa.mean(2)) + ba[:, None, :]
    q = p * torch.exp((z - z.detach()) / T)
    ((q / q.sum(2, keepdim=True)) * g).sum().backward()
    assert torch.equal(fa.grad, fa.grad[:, :, :1].expand_as(fa.grad))
    return fa.grad[:, :, 0], wa.grad, ba.grad


def split(t64, dtype):
    """The kernels' hi + lo split of an fp32 value into the 16-bit type -> (hi, lo) as float64."""
    v = t64.to(torch.float32)
    assert torch.equal(v.to(F64), t64)
    hi = v.to(dtype)
    lo = (v - hi.to(torch.float32)).to(dtype)
    return hi.to(F64), lo.to(F64)


# ----------------------------------------------------------------------------------------------------------------- dispatch mirror
def fwd_instance(dtype, c, s, k, h, w) -> str:
    """csrc/heads_fwd.hip miseg_head_local_fwd(): the kernel instance that serves a shape."""
    hw, t = h * w, tname(dtype)
    if dtype in HALF and k == 20 and c in (16, 32) and hw % 4 == 0 and s * k * c <= 3200:
        return f"head_local_fwd_mfma_kernel<{c}>[{t}]"
    if k <= 32:
        kpp = 4 * cdiv(k, 4)
        if hw % 4 == 0 and w % 4 == 0:
            return f"head_local_fwd_reg_kernel<{t},{kpp},4,{'true' if k == kpp else 'false'}>"
        return f"head_local_fwd_reg_kernel<{t},{kpp},1,false>"
    return f"head_local_fwd_kernel<{t}>"


def bwd_blocks(m, h, w) -> int:
    """head_w_blocks(): blocks (= partial vectors in the workspace) of the fused kernel."""
    return min(m * cdiv(h * w, 64), 768)


def bwd_ws_bytes(m, h, w, c, s, k) -> int:
    return (bwd_blocks(m, h, w) + 1) * (s * k * c + s * k) * 4


def bwd_wave_shape(dtype, c, s, k) -> bool:
    return dtype in HALF and k == 20 and c == 16 and s == 5


def bwd_instance(dtype, c, s, k, h, w, m) -> str:
    """csrc/heads_bwd.hip head_local_bwd_impl() and csrc/heads_bwd_fused.h launch_head_bwd_fused_t(): the kernel instance that serves a shape (h, w, m choose no instance, only how often a
    block or a wave loops: bwd_loops)."""
    t = tname(dtype)
    if bwd_wave_shape(dtype, c, s, k):
        return f"head_local_bwd_wave_kernel<16,false>[{t}]"
    ctm = 1 if c <= 16 else 2 if c <= 32 else 4 if c <= 64 else 8
    r = s * k
    if k == 20 and r <= 100 and dtype in HALF and c == 32:
        return f"head_local_bwd_fused_kernel<{t},2,25,true,true>"
    if k == 20 and r <= 100:
        return f"head_local_bwd_fused_kernel<{t},{ctm},25,true,false>"
    return f"head_local_bwd_fused_kernel<{t},{ctm},{28 if r <= 112 else 64},false,false>"


def bwd_loops(dtype, c, s, k, h, w, m) -> bool:
    """Does some block (fused kernel: 768 blocks at most) or some wave (wave kernel: 256 blocks of four waves at most) take a second chunk?"""
    chunks = m * cdiv(h * w, 64)
    return chunks > (4 * min(256, bwd_blocks(m, h, w)) if bwd_wave_shape(dtype, c, s, k) else 768)


def bwd_lds_bytes(c, s, k) -> int:
    """The LDS request of head_local_bwd_impl (refused above 150 KiB)."""
    r = s * k
    rp = cdiv(r, 16) * 16
    cp = cdiv(c, 16) * 16
    return max((rp * 65 + 64 * (c + 1) + rp * (c + 1) + 4 * max(s, 5) * 64) * 4, (2 * 128 * 72 + cp * 72 + 2 * cp * 136) * 2 + 4 * 5 * 64 * 4)


# ----------------------------------------------------------------------------------------------------------------- local backward cases
# name -> (storage types, C, S, K, M, H, W, options).  Options: den = one denominator for every type, fdens = share of non-zero features
# (the large maps: keeps sum |dz f| over all pixels below 2^24 lsb).
def _cases():
    t = {}

    def add(prefix, types, csk_list, shapes, **opt):
        for c, s, k in csk_list:
            for m, h, w in shapes:
                t[f"{prefix}_{c}x{s}x{k}_{m}x{h}x{w}"] = (tuple(types), c, s, k, m, h, w, opt)

    add("wave", HALF, [(16, 5, 20)], [(2, 6, 10), (3, 22, 36), (2, 37, 45)])
    add("wave", HALF, [(16, 5, 20)], [(4, 128, 136)], den=8, fdens=0.125)          # 1088 chunks > 4 * 256 waves
    add("bf", HALF, [(32, 5, 20), (32, 3, 20)], [(3, 22, 36), (2, 37, 45)])
    add("k20", (F32,), [(16, 5, 20), (32, 5, 20)], [(3, 22, 36)])
    add("k20", (F32,), [(16, 5, 20)], [(4, 112, 112)], fdens=0.125)                # 784 chunks > 768 blocks
    add("k20", HALF, [(16, 3, 20)], [(3, 22, 36)])
    add("k20", (F32, BF16), [(64, 5, 20), (128, 5, 20), (8, 1, 20)], [(3, 22, 36)])
    add("k20", ALL, [(24, 2, 20)], [(3, 22, 36)])
    add("rw28", (F32, BF16), [(8, 3, 6), (16, 5, 10), (32, 4, 28)], [(3, 10, 12)])
    add("rw28", ALL, [(12, 3, 7)], [(3, 10, 12)])
    add("rw28", (F32, BF16), [(8, 3, 6), (16, 5, 10), (32, 4, 28)], [(2, 37, 45)], fdens=0.5)      # few classes: |dz| is larger
    add("rw28", ALL, [(12, 3, 7)], [(2, 37, 45)], fdens=0.5)
    add("rw64", (F32, BF16), [(16, 5, 32), (32, 4, 64)], [(2, 22, 36)])
    add("rw64", ALL, [(16, 6, 20)], [(2, 22, 36)])
    return t


LOCAL_CASES = _cases()
# the instance family each name prefix must land on (asserted against bwd_instance by the CPU test)
FAMILY = {"wave": "head_local_bwd_wave_kernel<16,false>", "bf": ",25,true,true>", "k20": ",25,true,false>", "rw28": ",28,false,false>",
          "rw64": ",64,false,false>"}
TEMPS = (1.0, 0.5, 2.0)
# rows form (row0 > 0), accumulating form and gfeat = NULL: one shape of each of the first three instances
VARIANT_CASES = ("wave_16x5x20_3x22x36", "bf_32x5x20_3x22x36", "bf_32x3x20_2x37x45", "k20_16x5x20_3x22x36", "k20_24x2x20_3x22x36")
# the "w" recipe (W = n / 64 with a non-zero lo plane, dz within the 16-bit type): the two kernels that split W
W_RECIPE_CASES = ("wave_16x5x20_3x22x36", "wave_16x5x20_2x37x45", "bf_32x5x20_3x22x36", "bf_32x3x20_2x37x45")


def case_temperature(name: str) -> float:
    return TEMPS[sorted(LOCAL_CASES).index(name) % 3]


def local_pairs(names=None, types=None):
    """(case, storage type) pairs, case-major."""
    out = []
    for n in sorted(LOCAL_CASES) if names is None else names:
        out += [(n, d) for d in LOCAL_CASES[n][0] if types is None or d in types]
    return out


@functools.lru_cache(maxsize=2)
def local_case(name: str, dtype, recipe: str = "dz", flipset: int = 0):
    """-> dict(feat [B][C][H][W], w, prob, gprob, pre (integers the accumulating form finds in gfeat), src, flips, T, B, qdz, qw,
    gfeat, gw, gb (head_local_bwd_ref), and the worst-case accumulator magnitudes abs_gw, abs_gb, abs_gfeat, abs_dot)."""
    _, c, s, k, m, h, w, opt = LOCAL_CASES[name]
    b, T = m + 2, case_temperature(name)
    src, flips = pick_src(b, m), list(flip_sets(m)[flipset])
    tag = f"{name}/{recipe}"
    if recipe == "dz":
        den = opt.get("den", DEN[dtype])
        wt = R.ints(f"heads/{tag}/w", (s, k, c), -2, 2)
        qw = 1.0
    else:
        assert recipe == "w" and dtype in HALF
        den = 4                                                            # j * i <= 4 * 16: dz within 7 bits
        wt = R.ints(f"heads/{tag}/w/{tname(dtype)}", (s, k, c), -W_RANGE[dtype], W_RANGE[dtype]) / 64
        qw = 1.0 / 64
    feat = R.ints(f"heads/{tag}/f", (b, c, h, w), -4, 4, density=opt.get("fdens", 1.0))
    prob = simplex(f"{tag}/p/{den}", s, m, k, h, w, den)
    gprob = R.ints(f"heads/{tag}/g", (s, m, k, h, w), -2, 2)
    pre = R.ints(f"heads/{tag}/pre", (b, c, h, w), -8, 8)
    gfeat, gw, gb = head_local_bwd_ref(feat, wt, src, flips, T, prob, gprob)
    dz = dz_ref(prob, gprob, T).abs()
    return dict(feat=feat, w=wt, prob=prob, gprob=gprob, pre=pre, src=src, flips=flips, T=T, B=b, den=den, qdz=min(1.0, 1.0 / T) / den ** 2,
                qw=qw, gfeat=gfeat, gw=gw, gb=gb, abs_gw=float(torch.einsum("smkhw,mchw->skc", dz, gather_flip(feat, src, flips).abs()).max()),
                abs_gb=float(dz.sum((1, 3, 4)).max()), abs_gfeat=float(torch.einsum("skc,smkhw->mchw", wt.abs(), dz).max()),
                abs_dot=float((prob * gprob.abs()).sum(2).max()))


def local_precondition(name: str, dtype, recipe: str = "dz", flipset: int = 0) -> dict:
    """What makes equality the right demand, asserted on the reference: every sum below 2^24 of its lsb whatever the order, every
    operand exact in its type, the stored results one rounding away from values fp32 holds exactly.  Returns the case."""
    c = local_case(name, dtype, recipe, flipset)
    qdz, qw = c["qdz"], c["qw"]
    assert bool((c["prob"].sum(2) == 1).all()) and bool((c["prob"] >= 0).all())
    for t in (c["feat"], c["pre"]):
        R.assert_exact_range(t, dtype)
    for t in (c["prob"], c["gprob"], c["w"]):
        assert torch.equal(t.to(torch.float32).to(F64), t)
    R.assert_exact_range(c["gw"], F32, c["abs_gw"], quantum=qdz)
    R.assert_exact_range(c["gb"], F32, c["abs_gb"], quantum=qdz)
    R.assert_exact_range(c["gfeat"], F32, c["abs_gfeat"], quantum=qdz * qw)
    assert c["abs_dot"] * c["den"] < ACC_LIMIT
    R.assert_exact_range(c["gfeat"] + c["pre"], F32, c["abs_gfeat"] + 8.0, quantum=qdz * qw)      # the accumulating form's one fp32 add
    return c


# ----------------------------------------------------------------------------------------------------------------- global head cases
GLOBAL_CASES = {      # name -> (C, H = W, S, K, M); H * W a power of two: the mean and the pool's backward are exact
    "c32_8x8_s1k6_m3": (32, 8, 1, 6, 3),
    "c32_16x16_s1k6_m16": (32, 16, 1, 6, 16),
    "c48_8x8_s5k20_m3": (48, 8, 5, 20, 3),
    "c48_16x16_s5k20_m16": (48, 16, 5, 20, 16),
    "c256_8x8_s5k6_m16": (256, 8, 5, 6, 16),
    "c256_16x16_s1k20_m3": (256, 16, 1, 20, 3),
}


@functools.lru_cache(maxsize=2)
def global_case(name: str):
    """-> dict(feat [B][C][H][W], pooled [M][C], w, prob / gprob [S][M][K], src, T, B, gvec [M][C], gw, gb, magnitudes)."""
    c, h, s, k, m = GLOBAL_CASES[name]
    b, T, den = m + 2, TEMPS[sorted(GLOBAL_CASES).index(name) % 3], 8
    src = pick_src(b, m)
    feat = R.ints(f"gheads/{name}/f", (b, c, h, h), -4, 4)
    wt = R.ints(f"gheads/{name}/w", (s, k, c), -2, 2)
    prob = simplex(f"g/{name}/p", s, m, k, 1, 1, den)[:, :, :, 0, 0].contiguous()
    gprob = R.ints(f"gheads/{name}/g", (s, m, k), -2, 2)
    pooled = pool_ref(feat, src)
    gvec, gw, gb = head_global_bwd_ref(pooled, wt, src, h * h, T, prob, gprob)
    dz = dz_ref(prob, gprob, T).abs()
    return dict(feat=feat, pooled=pooled, w=wt, prob=prob, gprob=gprob, src=src, T=T, B=b, den=den, gvec=gvec, gw=gw, gb=gb,
                qdz=min(1.0, 1.0 / T) / den ** 2, abs_gw=float(torch.einsum("smk,mc->skc", dz, pooled.abs()).max()),
                abs_gb=float(dz.sum(1).max()), abs_gvec=float(torch.einsum("skc,smk->mc", wt.abs(), dz).max()))


def global_precondition(name: str, dtype) -> dict:
    c = global_case(name)
    hw = GLOBAL_CASES[name][1] ** 2
    assert hw & (hw - 1) == 0
    R.assert_exact_range(c["feat"], dtype)
    R.assert_exact_range(c["pooled"], F32, float(c["feat"].abs().sum((2, 3)).max()) / hw, quantum=1.0 / hw)      # integer sums, then / HW
    R.assert_exact_range(c["gw"], F32, c["abs_gw"], quantum=c["qdz"] / hw)
    R.assert_exact_range(c["gb"], F32, c["abs_gb"], quantum=c["qdz"])
    R.assert_exact_range(c["gvec"] * hw, F32, c["abs_gvec"], quantum=c["qdz"])               # the sum, before the exact division by HW
    R.round_to(c["gvec"], dtype)
    return c


# ----------------------------------------------------------------------------------------------------------------- forward cases (float64)
# name -> (storage types, C, S, K, M, H, W).  Not exact (exp): compared with float64 at the bounds of
# test_gpu_mi.py::test_local_head_forward_mfma_vs_float64.
FWD_REL, FWD_ABS, SIMPLEX_TOL = 1e-5, 2e-6, 2e-4


def _fwd_cases():
    t = {}
    for c in (16, 32):
        t[f"mfma{c}_s3_22x36"] = (HALF, c, 3, 20, 4, 22, 36)
    t["mfma16_s3_72x36"] = (HALF, 16, 3, 20, 4, 72, 36)                     # the largest map: three blocks of 1024 pixels, ragged
    for k in (4, 8, 12, 16, 24, 28, 32):
        t[f"reg4_exact_k{k}"] = (ALL, 8, 2, k, 3, 24, 44)                  # 1056 pixels: two blocks, the second nearly empty
    t["reg4_exact_k20_f32"] = ((F32,), 16, 5, 20, 3, 24, 44)
    for k in (6, 7, 10, 19):
        t[f"reg4_guard_k{k}"] = (ALL, 8, 2, k, 3, 24, 44)
    t["reg1_k10_37x45"] = (ALL, 8, 2, 10, 3, 37, 45)                        # W % 4 != 0, seven blocks of 256 pixels
    t["reg1_k10_9x10"] = (ALL, 8, 2, 10, 3, 9, 10)                          # W % 4 != 0, less than one block
    t["k20_off_mfma_7x9"] = (HALF, 16, 5, 20, 4, 7, 9)                      # H W % 4 != 0
    t["k20_off_mfma_c32_s6"] = (HALF, 32, 6, 20, 3, 24, 44)                 # S K C = 3840 > 3200
    for k in (33, 64):
        t[f"generic_k{k}"] = (ALL, 8, 2, k, 3, 13, 22)                     # 286 pixels: two blocks
    return t


FWD_CASES = _fwd_cases()
FWD_FAMILY = {"mfma16": "head_local_fwd_mfma_kernel<16>", "mfma32": "head_local_fwd_mfma_kernel<32>", "reg4_exact": ",4,true>",
              "reg4_guard": ",4,false>", "reg1": ",1,false>", "generic": "head_local_fwd_kernel<"}


def fwd_pairs():
    return [(n, d) for n in sorted(FWD_CASES) for d in FWD_CASES[n][0]]


def fwd_case(name: str, dtype):
    """-> dict(feat [B][C][H][W] rounded to the storage type, w, b, src, flips, T, ref [S][M][K][H][W] float64): the generator
    scales of test_local_head_forward_mfma_vs_float64 (weights 0.7 randn, T in {0.8, 1})."""
    _, c, s, k, m, h, w = FWD_CASES[name]
    gen = torch.Generator().manual_seed(synth._seed(f"exact_heads/fwd/{name}"))
    b = m + 1
    feat = torch.randn(b, c, h, w, generator=gen).to(dtype).to(F64)
    wt = (torch.randn(s, k, c, generator=gen) * 0.7).to(F64)
    bias = torch.randn(s, k, generator=gen).to(F64)
    src = list(range(b - 1, b - 1 - m, -1))
    src[0], src[-1] = src[-1], src[0]
    flips = [(3 + i) % 4 for i in range(m)]
    T = (0.8, 1.0)[sorted(FWD_CASES).index(name) % 2]
    z = torch.einsum("skc,mchw->smkhw", wt, gather_flip(feat, src, flips)) + bias[:, None, :, None, None]
    return dict(feat=feat, w=wt, b=bias, src=src, flips=flips, T=T, B=b, ref=torch.softmax(z / T, dim=2))
