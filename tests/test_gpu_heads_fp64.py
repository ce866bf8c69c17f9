"""Every branch of miseg_head_local_fwd (csrc/heads_fwd.hip) against a float64 evaluation of softmax((W f + b) / T) on the gathered, flipped,
storage-type-rounded features.  Not exact (the kernels go through exp2 / expf); the bounds are the project's own, those of
test_gpu_mi.py::test_local_head_forward_mfma_vs_float64: max |d| / (ref + 1e-9) <= 1e-5, max |d| <= 2e-6, no simplex violation, and the
kernel's fused violation counter equal to the count taken from its output (also with one sub-head poisoned by a NaN bias, where both
must count every pixel of that sub-head).  Same generator scales as that test (weights 0.7 randn, T in {0.8, 1}).

Case -> kernel instance (exact_heads.fwd_instance mirrors the dispatch; the CPU test pins every case to its instance).
16-bit = bf16 and, through the -DMISEG_F16_BUILD twins, IEEE half.
  mfma16_s3_*, mfma32_s3_22x36   16-bit   head_local_fwd_mfma_kernel<16 | 32> with S = 3 (test_gpu_mi.py runs S = 5); 72 x 36 is the largest map
  reg4_exact_k{4..32}            all      head_local_fwd_reg_kernel<., KPP, 4, true> at KPP in {4, 8, 12, 16, 24, 28, 32}; k20: fp32
  reg4_guard_k{6,7,10,19}        all      head_local_fwd_reg_kernel<., KPP, 4, false> (K % 4 != 0: the per-class guards)
  reg1_k10_37x45, _9x10          all      head_local_fwd_reg_kernel<., 12, 1, false> (W % 4 != 0: one pixel per thread)
  k20_off_mfma_7x9               16-bit   K = 20, C = 16 with H W % 4 != 0 -> reg<., 20, 1, false>
  k20_off_mfma_c32_s6            16-bit   K = 20, C = 32 with S K C = 3840 > 3200 -> reg<., 20, 4, true>
  generic_k33, generic_k64       all      head_local_fwd_kernel (K > 32; no fused counter there: the entry point refuses one)
Not covered: the one-pixel-per-thread form reg<., KPP, 1, false> runs at KPP = 12 and 20 only, and reg<bf16 | f16, 20, 4, true> only where
a K = 20 tap falls off the MFMA kernel; the other KPP of that form are the same code with another unroll count.
"""
import pytest
import torch

import exact_heads as E

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64
PAIRS = E.fwd_pairs()


@pytest.mark.parametrize("name,dtype", PAIRS, ids=[f"{n}-{E.tname(d)}" for n, d in PAIRS])
def test_local_head_forward_vs_float64(name, dtype):
    from miseg_amd import _cabi, checks
    _, ch, s, k, m, h, w = E.FWD_CASES[name]
    c = E.fwd_case(name, dtype)
    dt = {torch.float32: _cabi.F32, torch.bfloat16: _cabi.BF16, torch.float16: _cabi.F16}[dtype]
    stream = torch.cuda.current_stream().cuda_stream
    feat = c["feat"].permute(0, 2, 3, 1).contiguous().to(dtype).to(DEV)
    wt, bias = c["w"].float().to(DEV), c["b"].float().to(DEV)
    src = torch.tensor(c["src"], dtype=torch.int32, device=DEV)
    flips = torch.tensor(c["flips"], dtype=torch.int32, device=DEV)
    fused = k <= 32

    def run(b_):
        prob = torch.full((s, m, k, h, w), float("nan"), device=DEV)
        viol = torch.zeros(1, dtype=torch.int32, device=DEV)
        _cabi.call("miseg_head_local_fwd", stream, dt, feat.data_ptr(), c["B"], h, w, ch, src.data_ptr(), flips.data_ptr(), m, wt.data_ptr(),
                   b_.data_ptr(), s, k, c["T"], prob.data_ptr(), E.SIMPLEX_TOL, viol.data_ptr() if fused else None)
        torch.cuda.synchronize()
        return prob, int(viol)

    prob, nviol = run(bias)
    counted = int((~((prob.double().sum(2) - 1.0).abs() <= E.SIMPLEX_TOL)).sum())
    d = (prob.double().cpu() - c["ref"]).abs()
    rel, ab = float((d / (c["ref"] + 1e-9)).max()), float(d.max())
    print(f"\nFWD {E.fwd_instance(dtype, ch, s, k, h, w)} {name} rel={rel:.3e} abs={ab:.3e}")
    assert rel <= E.FWD_REL
    assert ab <= E.FWD_ABS
    assert int(checks.simplex_violations(prob, 2)) == 0 and counted == 0
    if fused:
        assert nviol == counted
        bad = bias.clone()
        bad[s - 1, k // 2] = float("nan")
        prob_bad, nviol_bad = run(bad)
        assert nviol_bad == int((~((prob_bad.double().sum(2) - 1.0).abs() <= E.SIMPLEX_TOL)).sum()) == m * h * w
        assert torch.equal(prob_bad[:s - 1], prob[:s - 1])
    else:
        with pytest.raises(_cabi.MisegError):      # K > 32: no fused counter
            viol = torch.zeros(1, dtype=torch.int32, device=DEV)
            _cabi.call("miseg_head_local_fwd", stream, dt, feat.data_ptr(), c["B"], h, w, ch, src.data_ptr(), flips.data_ptr(), m, wt.data_ptr(),
                       bias.data_ptr(), s, k, c["T"], prob.data_ptr(), E.SIMPLEX_TOL, viol.data_ptr())
