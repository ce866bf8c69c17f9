"""Bit-exact tests of the cluster-head backward kernels (csrc/heads_bwd.hip, csrc/heads_bwd_fused.h, csrc/heads_global.hip) on dyadic data.

The backward kernels take prob and gprob as inputs: dot = sum g p, dz = p (g - dot) / T, a hi + lo 16-bit split of dz and W, fp32
matrix-core sums, one rounding to the storage type.  On the recipes of tests/exact_heads.py (p = j / den on the simplex, integer g and
features, W integers or n / 64, T in {1, 0.5, 2}) every step is exact, so gfeat, gw and gb must EQUAL the float64 reference at every
element in every storage type.  Every comparison below is torch.equal; each case first asserts, on its reference, the precondition that
makes equality the right demand (tests/test_cpu_exact_heads.py proves the same without a GPU).  Every call goes through the C ABI
(miseg_amd._cabi).  Outputs are pre-filled with NaN, the workspace with NaN bit patterns, the rows of gfeat outside src with a sentinel
that must survive bit for bit.  Every case runs all four flip masks (two flip assignments where M < 4), a non-monotone src that is a
strict subset of the batch, and T from the recipe.

Case -> kernel instance (the dispatch predicates of head_local_bwd_impl are mirrored by exact_heads.bwd_instance and asserted through
the library's own queries).  16-bit = bf16 and, through the -DMISEG_F16_BUILD twins, IEEE half.  Name = family_CxSxK_MxHxW.
  wave_16x5x20_*   16-bit   head_local_bwd_wave_kernel<16,false>: 2x6x10 less than one chunk, 3x22x36 ragged last chunk, 2x37x45 odd W
                            and HW, 4x128x136 1088 chunks > 4 * 256 waves (a wave takes a second chunk; sum_partials reads 256 of 768 slots)
  bf_32x5x20_*, bf_32x3x20_*  16-bit   head_local_bwd_fused_kernel<.,2,25,true,true> (dz and W^T as hi + lo planes on the 16-bit MFMA)
  k20_16x5x20_* fp32, k20_16x3x20_* 16-bit   fused<.,1,25,true,false>;  4x112x112: 784 chunks > 768 blocks (a block loops)
  k20_32x5x20_* fp32, k20_24x2x20_* all      fused<.,2,25,true,false>   (24: C % 16 != 0)
  k20_64x5x20_*, k20_128x5x20_* fp32 + bf16  fused<.,4,..> / fused<.,8,..>: the 64- and 128-channel taps
  k20_8x1x20_* fp32 + bf16                   fused<.,1,25,true,false> with C % 16 != 0 and one sub-head
  rw28_8x3x6_*, rw28_16x5x10_*, rw28_12x3x7_* (K odd: kmagic, C % 16 != 0), rw28_32x4x28_* (R = 112)   fused<.,1|2,28,false,false>
  rw64_16x5x32_* (R 160), rw64_32x4x64_* (R 256), rw64_16x6x20_* (K = 20 but R = 120)                  fused<.,1|2,64,false,false>
  test_local_head_backward_rows_acc_and_null        the first three instances through miseg_head_local_bwd_rows (row0 = 1, guard rows on
                                                    both sides), miseg_head_local_bwd_acc (gfeat preloaded with integers, the exact sum
                                                    rounded once) and gfeat = NULL (gw, gb unchanged)
  test_local_head_backward_with_split_weights       wave and BF kernels with W = n / 64 (non-zero W-lo plane, dz inside the 16-bit type)
  test_local_head_backward_refusals                 C % 4 != 0, S K > 256, a workspace one byte short, R = 256 with C = 128 (LDS)
  test_global_head_pool_and_backward                head_pool_kernel, head_global_bwd_kernel, head_global_bwd_feat_kernel (+ _rows)
  test_unknown_storage_type_is_refused_before_any_launch   dt = 7 through the entry points that used to launch their 16-bit kernels on it
sum_partials_kernel runs behind every local case.  The forward kernels are in test_gpu_heads_fp64.py (float64 comparison: they go through exp).
Not covered here: head_local_bwd_wave_kernel<16,true> (miseg_head_local_bwd_recompute) runs the softmax, so it is not exact by design;
test_gpu_mi.py::test_local_head_backward_recomputing_the_probabilities_is_bit_equal ties it bit for bit to the reading form above.
head_global_fwd_kernel (exp) is compared with the oracle in test_gpu_mi.py.  Of the fused kernel's (storage type, CTM, RW) grid the
table runs every CTM (1, 2, 4, 8) with RW = 25 and CTM 1 | 2 with RW = 28 and RW = 64; fused<.,4 | 8,28 | 64,..> (more than 32 channels
off the K = 20 path: no shipped tap) are the same code with another pair of constants and are not run.
IEEE half runs one case per kernel family (wave, BF, K = 20 CTM 1 | 2, RW 28, RW 64), not every CTM.
"""
import pytest
import torch

import exact_heads as E
import exact_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64
NAN = float("nan")
SENTINEL = -77.0        # exact in every storage type


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
    """Device address of a tensor for the C ABI; the tensor is kept alive until the test ends."""
    if t is None:
        return None
    _LIVE.append(t)
    return t.data_ptr()


@pytest.fixture(autouse=True)
def _release_operands():
    yield
    torch.cuda.synchronize()
    _LIVE.clear()


def nhwc(t64, dtype):
    return t64.permute(0, 2, 3, 1).contiguous().to(dtype).to(DEV)


def host(t):
    return t.detach().cpu().to(F64).permute(0, 3, 1, 2)


def f32(t64):
    return t64.to(torch.float32).contiguous().to(DEV)


def i32(values):
    return torch.tensor(list(values), dtype=torch.int32, device=DEV)


def nans(shape, dtype=torch.float32):
    return torch.full(tuple(shape), NAN, dtype=dtype, device=DEV)


def nan_bytes(nbytes):
    """A workspace whose every fp32 word is a NaN pattern: a partial vector that is read without having been written shows in gw / gb."""
    return torch.full((max(int(nbytes), 16),), 0xFF, dtype=torch.uint8, device=DEV)


def _ids(pairs):
    return [f"{n}-{E.tname(d)}" for n, d in pairs]


def run_local(name, dtype, c, form="plain"):
    """One call of the local head's backward on the case c -> (gfeat [B][C][H][W] float64 on the host or None, gw, gb).
    form: "plain" | "rows" (compact gradient, row0 = 1) | "acc" (gfeat preloaded with c["pre"]) | "null" (gfeat = NULL)."""
    abi = _abi()
    _, ch, s, k, m, h, w, _ = E.LOCAL_CASES[name]
    dt, b = DT(dtype), c["B"]
    nb = abi.query("miseg_head_local_bwd_ws_bytes", m, h, w, ch, s, k)
    assert nb == E.bwd_ws_bytes(m, h, w, ch, s, k)
    assert abi.query("miseg_head_local_bwd_recompute_supported", dt, ch, s, k) == int(E.bwd_wave_shape(dtype, ch, s, k))
    assert abi.query("miseg_head_local_bwd_acc_supported", dt, ch, s, k) == 1
    feat, wt, prob, gprob = nhwc(c["feat"], dtype), f32(c["w"]), f32(c["prob"]), f32(c["gprob"])
    src, flips = i32(c["src"]), i32(c["flips"])
    gfeat = torch.full((b, h, w, ch), SENTINEL, dtype=dtype, device=DEV)
    gfeat[src.long()] = nhwc(c["pre"], dtype)[src.long()] if form == "acc" else NAN
    gw, gb, ws = nans((s, k, ch)), nans((s, k)), nan_bytes(nb)
    head = (st(), dt, ptr(feat), b, h, w, ch, ptr(src), ptr(flips), m, ptr(wt), s, k, c["T"], ptr(prob), ptr(gprob))
    tail = (ptr(gw), ptr(gb), ptr(ws), nb)
    if form == "rows":
        abi.call("miseg_head_local_bwd_rows", *head, ptr(gfeat) + h * w * ch * gfeat.element_size(), 1, *tail)
    elif form == "acc":
        abi.call("miseg_head_local_bwd_acc", *head, ptr(gfeat), *tail)
    else:
        abi.call("miseg_head_local_bwd", *head, None if form == "null" else ptr(gfeat), *tail)
    return (None if form == "null" else host(gfeat)), gw.cpu().to(F64), gb.cpu().to(F64)


def expected_gfeat(c, dtype, acc=False):
    """Rows of src: the exact gradient (+ the preloaded integers) rounded once to the storage type; every other row: the sentinel."""
    exact = c["gfeat"] + c["pre"] if acc else c["gfeat"]
    out = torch.full_like(exact, SENTINEL)
    out[c["src"]] = R.round_to(exact, dtype)[c["src"]]
    return out


LOCAL_PAIRS = E.local_pairs()


@pytest.mark.parametrize("name,dtype", LOCAL_PAIRS, ids=_ids(LOCAL_PAIRS))
def test_local_head_backward(name, dtype):
    """miseg_head_local_bwd on the "dz" recipe: gfeat (rows of src; the other rows keep the sentinel), gw and gb equal the float64
    reference for every flip assignment of the case."""
    m = E.LOCAL_CASES[name][4]
    masks = set()
    for fs in range(len(E.flip_sets(m))):
        c = E.local_precondition(name, dtype, "dz", fs)
        masks |= set(c["flips"])
        gfeat, gw, gb = run_local(name, dtype, c)
        assert torch.equal(gw, c["gw"])
        assert torch.equal(gb, c["gb"])
        assert torch.equal(gfeat, expected_gfeat(c, dtype))
    assert masks == {0, 1, 2, 3}


VARIANT_PAIRS = E.local_pairs(E.VARIANT_CASES)


@pytest.mark.parametrize("name,dtype", VARIANT_PAIRS, ids=_ids(VARIANT_PAIRS))
def test_local_head_backward_rows_acc_and_null(name, dtype):
    """The wave kernel, the BF fused kernel and the K = 20 fused kernel through the three other entry points: the compact gradient
    with row0 = 1 (one guard row on either side keeps the sentinel), the accumulating form (gfeat holds integers; result = the exact
    sum rounded ONCE), and gfeat = NULL (the kernels skip the gfeat phase behind `if (gfeat)`; gw and gb are the same)."""
    c = E.local_precondition(name, dtype, "dz", 0)
    gfeat, gw, gb = run_local(name, dtype, c, "rows")
    assert torch.equal(gw, c["gw"]) and torch.equal(gb, c["gb"])
    assert torch.equal(gfeat, expected_gfeat(c, dtype))
    gfeat, gw, gb = run_local(name, dtype, c, "acc")
    assert torch.equal(gw, c["gw"]) and torch.equal(gb, c["gb"])
    assert torch.equal(gfeat, expected_gfeat(c, dtype, acc=True))
    gfeat, gw, gb = run_local(name, dtype, c, "null")
    assert gfeat is None and torch.equal(gw, c["gw"]) and torch.equal(gb, c["gb"])


W_PAIRS = E.local_pairs(E.W_RECIPE_CASES)


@pytest.mark.parametrize("name,dtype", W_PAIRS, ids=_ids(W_PAIRS))
def test_local_head_backward_with_split_weights(name, dtype):
    """The "w" recipe: W = n / 64 needs both planes of the kernels' W^T split, dz fits the 16-bit type (no lo x lo product exists)."""
    c = E.local_precondition(name, dtype, "w", 0)
    gfeat, gw, gb = run_local(name, dtype, c)
    assert torch.equal(gw, c["gw"]) and torch.equal(gb, c["gb"])
    assert torch.equal(gfeat, expected_gfeat(c, dtype))


def test_local_head_backward_refusals():
    """Shapes the entry point must refuse (MisegError) instead of launching: C % 4 != 0, S K > 256, a workspace one byte short,
    R = 256 with C = 128 (the LDS request).  Nothing is launched, so small buffers do."""
    abi = _abi()
    buf = torch.zeros(1 << 16, dtype=torch.float32, device=DEV)
    src, flips = i32([0]), i32([0])

    def call(dtype, ch, s, k, h=4, w=4, short=0):
        nb = E.bwd_ws_bytes(1, h, w, ch, s, k)
        abi.call("miseg_head_local_bwd", st(), DT(dtype), ptr(buf), 1, h, w, ch, ptr(src), ptr(flips), 1, ptr(buf), s, k, 1.0, ptr(buf), ptr(buf),
                 ptr(buf), ptr(buf), ptr(buf), ptr(buf), nb - short)

    for dtype in E.ALL:
        for bad in (dict(ch=10, s=2, k=6), dict(ch=16, s=5, k=64), dict(ch=128, s=4, k=64), dict(ch=8, s=2, k=6, short=1)):
            with pytest.raises(abi.MisegError):
                call(dtype, **bad)
    assert E.bwd_lds_bytes(128, 4, 64) > 150 * 1024      # (every accepted case above passes exactly the queried workspace size)


GLOBAL_PAIRS = [(n, d) for n in sorted(E.GLOBAL_CASES) for d in E.ALL]


@pytest.mark.parametrize("name,dtype", GLOBAL_PAIRS, ids=_ids(GLOBAL_PAIRS))
def test_global_head_pool_and_backward(name, dtype):
    """miseg_head_global_fwd's pooled output (integer features, H W a power of two: the mean is exact) and miseg_head_global_bwd /
    _rows on the dyadic recipe: gw, gb exact, gfeat = (sum W dz) / HW rounded once, on every pixel of the rows of src only."""
    abi = _abi()
    ch, h, s, k, m = E.GLOBAL_CASES[name]
    c = E.global_precondition(name, dtype)
    dt, b = DT(dtype), c["B"]
    feat, wt, src = nhwc(c["feat"], dtype), f32(c["w"]), i32(c["src"])
    bias = f32(R.ints(f"gheads/{name}/b", (s, k), -2, 2))
    pooled, prob_out = nans((m, ch)), nans((s, m, k))
    abi.call("miseg_head_global_fwd", st(), dt, ptr(feat), b, h, h, ch, ptr(src), m, ptr(wt), ptr(bias), s, k, c["T"], ptr(pooled), ptr(prob_out))
    assert torch.equal(pooled.cpu().to(F64), c["pooled"])
    assert bool(torch.isfinite(prob_out).all())
    want = torch.full((b, ch, h, h), SENTINEL, dtype=F64)
    want[c["src"]] = R.round_to(c["gvec"], dtype)[:, :, None, None].expand(m, ch, h, h)
    prob, gprob, pooled_in = f32(c["prob"]), f32(c["gprob"]), f32(c["pooled"])
    for rows in (False, True):
        gfeat = torch.full((b, h, h, ch), SENTINEL, dtype=dtype, device=DEV)
        gfeat[src.long()] = NAN
        gw, gb, dz = nans((s, k, ch)), nans((s, k)), nans((s, m, k))
        head = (st(), dt, b, h, h, ch, ptr(src), m, ptr(wt), s, k, c["T"], ptr(pooled_in), ptr(prob), ptr(gprob))
        if rows:
            abi.call("miseg_head_global_bwd_rows", *head, ptr(gfeat) + h * h * ch * gfeat.element_size(), 1, ptr(gw), ptr(gb), ptr(dz))
        else:
            abi.call("miseg_head_global_bwd", *head, ptr(gfeat), ptr(gw), ptr(gb), ptr(dz))
        assert torch.equal(gw.cpu().to(F64), c["gw"]) and torch.equal(gb.cpu().to(F64), c["gb"])
        assert torch.equal(dz.cpu().to(F64), E.dz_ref(c["prob"], c["gprob"], c["T"]))
        assert torch.equal(host(gfeat), want)


UNKNOWN_DT = 7        # none of MISEG_F32, MISEG_BF16, MISEG_F16


def _unknown_dt_calls():
    """Entry point -> (arguments after the stream and dt, outputs).  The entry points that used to hand an unknown storage type to their
    16-bit kernels, each at the smallest shape its own test uses (bn_relu_bwd_ext and the ext_parts form of
    bn_relu_bwd_stats have no direct test: one 4 x 4 map of 8 channels).  Every tensor is a device buffer sized for FLOAT storage, so
    a 16-bit kernel launched on it by mistake stays inside it; every output is filled with the sentinel."""
    def ones(*shape):
        return torch.ones(shape, dtype=torch.float32, device=DEV)

    def out(*shape):
        return torch.full(shape, SENTINEL, dtype=torch.float32, device=DEV)

    abi = _abi()
    ch, h, s, k, m = E.GLOBAL_CASES[min(E.GLOBAL_CASES, key=lambda n: E.GLOBAL_CASES[n][0] * E.GLOBAL_CASES[n][1] ** 2 * E.GLOBAL_CASES[n][4])]
    b, src = m + 1, i32(range(m, 0, -1))
    pooled, prob, gfeat, gw, gb, dz = out(m, ch), out(s, m, k), out(b, h, h, ch), out(s, k, ch), out(s, k), out(s, m, k)
    bwd = (b, h, h, ch, ptr(src), m, ptr(ones(s, k, ch)), s, k, 1.0, ptr(ones(m, ch)), ptr(ones(s, m, k) / k), ptr(ones(s, m, k)))
    n, c = 1, 8
    graw, ggamma, gbeta, coeffs, coef6 = out(n, 4, 4, c), out(c), out(c), out(3, c), out(6, c)
    bn = (ptr(ones(n, 4, 4, c)), ptr(ones(n, 4, 4, c)), n, 4, 4, c, ptr(ones(c)), ptr(ones(4, c)), 1)
    n1, h1, w1 = min(R.C1X1_SHAPES.values(), key=lambda t: t[0] * t[1] * t[2])
    cout = min(R.C1X1_COUTS)
    ws1 = out(abi.query("miseg_conv1x1_bwd_ws_bytes", n1, h1, w1, 16, cout) // 4 + 1)
    logits, gin, gw1, gb1 = out(n1, h1, w1, cout), out(n1, h1, w1, 16), out(cout, 16), out(cout)
    x1 = ones(n1, h1, w1, 16)
    return {
        "miseg_head_global_fwd": ((ptr(ones(b, h, h, ch)), b, h, h, ch, ptr(src), m, ptr(ones(s, k, ch)), ptr(ones(s, k)), s, k, 1.0, ptr(pooled), ptr(prob)),
                                  [pooled, prob]),
        "miseg_head_global_bwd": (bwd + (ptr(gfeat), ptr(gw), ptr(gb), ptr(dz)), [gfeat, gw, gb, dz]),
        "miseg_head_global_bwd_rows": (bwd + (ptr(gfeat), 0, ptr(gw), ptr(gb), ptr(dz)), [gfeat, gw, gb, dz]),
        "miseg_bn_relu_bwd_ext": (bn + (ptr(graw), ptr(ggamma), ptr(gbeta), ptr(ones(2, 2, c)), 2, ptr(coeffs), coeffs.numel() * 4), [graw, ggamma, gbeta, coeffs]),
        "miseg_bn_relu_bwd_stats": (bn + (ptr(coef6), ptr(ggamma), ptr(gbeta), ptr(ones(2, 2, c)), 2, ptr(coeffs), coeffs.numel() * 4), [coef6, ggamma, gbeta]),
        "miseg_conv1x1_fwd": ((ptr(x1), n1, h1, w1, 16, ptr(ones(cout, 16)), ptr(ones(cout)), cout, ptr(logits)), [logits]),
        "miseg_conv1x1_bwd": ((ptr(x1), ptr(ones(n1, h1, w1, cout)), n1, h1, w1, 16, ptr(ones(cout, 16)), cout, ptr(gin), ptr(gw1), ptr(gb1), ptr(ws1),
                               ws1.numel() * 4), [gin, gw1, gb1, ws1]),
    }


@pytest.mark.parametrize("entry", ["miseg_head_global_fwd", "miseg_head_global_bwd", "miseg_head_global_bwd_rows", "miseg_bn_relu_bwd_ext",
                                   "miseg_bn_relu_bwd_stats", "miseg_conv1x1_fwd", "miseg_conv1x1_bwd"])
def test_unknown_storage_type_is_refused_before_any_launch(entry):
    """A storage type that is none of the three is MISEG_E_INVALID "bad dtype" before the entry point's first launch: no output is touched."""
    abi = _abi()
    args, outputs = _unknown_dt_calls()[entry]
    with pytest.raises(abi.MisegError, match="bad dtype"):
        abi.call(entry, st(), UNKNOWN_DT, *args)
    torch.cuda.synchronize()
    for t in outputs:
        assert bool((t == SENTINEL).all()), entry
