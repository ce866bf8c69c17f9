// Forward of the local head on 16-bit storage, and its entry point (heads.h has the file map).
#include "heads_fwd.h"

namespace miseg {

// MFMA form of the kernel above for the shipped taps (bf16 features, K = 20, C = 16 or 32).  The register kernel spends
// K*C FMAs per pixel and sub-head on the VALU and is bound by them, not by its 4 bytes-per-probability of output.  Here a wave
// computes logits[class][pixel] = W x feat^T on the matrix pipe: the fp32 weights are split once per block into three bf16
// planes (w = h1 + h2 + h3 to within 2^-25 relative, the features are bf16 already, the products exact and the accumulation
// fp32), so the logits agree with the FMA chain to rounding order.  The D tiles (4 classes x 1 pixel per lane) go through a
// per-wave LDS transpose, 128 pixels at a time, into the softmax layout of the register kernel (4 consecutive pixels x 20
// classes per lane), and the epilogue -- exp2 softmax, simplex check, one 16-byte store per class plane -- is that kernel's.
template <int C>
__global__ __launch_bounds__(kHT) void head_local_fwd_mfma_kernel(const bf16* __restrict__ feat, int H, int W,
                                                                  const int32_t* __restrict__ src, const int32_t* __restrict__ flips,
                                                                  int M, const float* __restrict__ w, const float* __restrict__ b, int S,
                                                                  float invT, float* __restrict__ prob, float tol,
                                                                  int32_t* __restrict__ viol) {
    constexpr int K = 20, ZS = kHeadZS, CP = head_mfma_cp<C>(), CQ = C / 4;
    typedef typename HeadFrag<C>::type frag_t;
    extern __shared__ __attribute__((aligned(16))) unsigned char hl[];
    float* ztw = reinterpret_cast<float*>(hl) + (size_t)(threadIdx.x >> 6) * K * ZS;   // this wave's [K][ZS]
    bf16* wp = reinterpret_cast<bf16*>(hl + (size_t)(kHT / 64) * K * ZS * 4);            // [S][3][K][CP]
    const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, q = lane >> 4;
    const int HW = H * W, m = blockIdx.y;
    for (int i = tid; i < S * K * C; i += kHT) {
        const float v = w[i];
        const bf16 h1 = __float2bfloat16(v);
        const float r1 = v - __bfloat162float(h1);
        const bf16 h2 = __float2bfloat16(r1);
        const bf16 h3 = __float2bfloat16(r1 - __bfloat162float(h2));
        const int s = i / (K * C), rem = i - s * K * C, k = rem / C, c = rem - k * C;
        bf16* d = wp + ((size_t)(s * 3) * K + k) * CP + c;
        d[0] = h1, d[(size_t)K * CP] = h2, d[(size_t)2 * K * CP] = h3;
    }
    __syncthreads();
    const int f = flips ? flips[m] : 0;
    const int wbase = (blockIdx.x * (kHT / 64) + (tid >> 6)) * 256;   // first pixel of this wave
    const bf16* fs = feat + (size_t)src[m] * HW * C + q * CQ;
    int foff[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        const int p = min(wbase + t * 16 + l15, HW - 1), h = p / W, wq = p - h * W;
        foff[t] = (flip_h(h, H, f) * W + flip_w(wq, W, f)) * C;
    }
    const int pix0 = wbase + lane * 4;
    const bool live = pix0 < HW;
    int nbad = 0;
    for (int s = 0; s < S; ++s) {
        frag_t wa[2][3];
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int p = 0; p < 3; ++p) {
                const int cls = min(ct * 16 + l15, K - 1);
                frag_t v = *reinterpret_cast<const frag_t*>(wp + ((size_t)(s * 3 + p) * K + cls) * CP + q * CQ);
                if (ct * 16 + l15 >= K)
#pragma unroll
                    for (int e = 0; e < (int)(sizeof(frag_t) / 2); ++e) v[e] = (__bf16)0.f;
                wa[ct][p] = v;
            }
        float z[4][K];
#pragma unroll
        for (int half = 0; half < 2; ++half) {
#pragma unroll
            for (int t8 = 0; t8 < 8; ++t8) {
                const frag_t fb = *reinterpret_cast<const frag_t*>(fs + foff[half * 8 + t8]);
                f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int p = 2; p >= 0; --p) {   // smallest plane first
                    a0 = HeadFrag<C>::mma(wa[0][p], fb, a0);
                    a1 = HeadFrag<C>::mma(wa[1][p], fb, a1);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) ztw[(4 * q + r) * ZS + t8 * 16 + l15] = a0[r];
                if (q == 0)
#pragma unroll
                    for (int r = 0; r < 4; ++r) ztw[(16 + r) * ZS + t8 * 16 + l15] = a1[r];
            }
            __builtin_amdgcn_wave_barrier();   // a wave's LDS traffic is in order: no workgroup barrier, only no reordering
            if ((lane >> 5) == half) {
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const float4 v = *reinterpret_cast<const float4*>(ztw + k * ZS + 4 * (lane & 31));
                    z[0][k] = v.x, z[1][k] = v.y, z[2][k] = v.z, z[3][k] = v.w;
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const float bv = b[s * K + k];
#pragma unroll
            for (int j = 0; j < 4; ++j) z[j][k] += bv;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float mx = -3.4e38f;
#pragma unroll
            for (int k = 0; k < K; ++k) mx = fmaxf(mx, z[j][k]);
            const float sc2 = invT * 1.4426950408889634f, off2 = -mx * sc2;
            float sum = 0.f;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                z[j][k] = __builtin_amdgcn_exp2f(fmaf(z[j][k], sc2, off2));
                sum += z[j][k];
            }
            const float inv = 1.0f / sum;
            float ps = 0.f;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                z[j][k] *= inv;
                ps += z[j][k];
            }
            nbad += !(fabsf(ps - 1.f) <= tol);
        }
        if (live) {
            float* out = prob + (((size_t)s * M + m) * K) * HW + pix0;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                // non-temporal: 839 MB that nothing re-reads from a cache
                const f32x4 v4 = {z[0][k], z[1][k], z[2][k], z[3][k]};
                __builtin_nontemporal_store(v4, reinterpret_cast<f32x4*>(out + (size_t)k * HW));
            }
        }
    }
    if (viol && live && nbad) atomicAdd(viol, nbad);
}

}  // namespace miseg

using namespace miseg;

template <int C> static size_t head_mfma_lds(int64_t S) { return (size_t)(kHT / 64) * 20 * kHeadZS * 4 + (size_t)S * 3 * 20 * head_mfma_cp<C>() * 2; }
extern "C" int miseg_head_local_fwd(void* stream, int dt, const void* feat, int64_t B, int64_t H, int64_t W, int64_t C,
                                    const int32_t* src, const int32_t* flips, int64_t M, const float* w, const float* b, int64_t S,
                                    int64_t K, float T, float* prob, float simplex_tol, int32_t* simplex_violations) {
    MISEG_TAPE(miseg_head_local_fwd, stream, dt, feat, B, H, W, C, src, flips, M, w, b, S, K, T, prob, simplex_tol, simplex_violations);
    MISEG_F16_DISPATCH_ON(dt, miseg_head_local_fwd, stream, MISEG_BF16, feat, B, H, W, C, src, flips, M, w, b, S, K, T, prob, simplex_tol, simplex_violations);
    MISEG_REQUIRE(feat && src && w && b && prob, "head_local_fwd: null pointer");
    MISEG_REQUIRE(C > 0 && C % 4 == 0 && K > 0 && K <= 64 && M > 0 && S > 0 && H > 0 && W > 0, "head_local_fwd: need C%%4==0, K<=64");
    MISEG_REQUIRE(simplex_violations == nullptr || K <= 32, "head_local_fwd: the fused simplex check needs K <= 32");
    dim3 grid((unsigned)cdiv(H * W, kHT), (unsigned)M);
    size_t ldsb = (size_t)K * kHT * 4;
    hipStream_t st = as_stream(stream);
    HeadFwd a{grid, ldsb, st, feat, (int)H, (int)W, (int)C, src, flips, (int)M, w, b, (int)S, (int)K, 1.0f / T, prob, simplex_tol, simplex_violations};
    if (!storage_type_served(dt)) return fail(MISEG_E_INVALID, "head_local_fwd: bad dtype %d", dt);
    if (dt == MISEG_BF16 && K == 20 && (C == 16 || C == 32) && (H * W) % 4 == 0 && S * K * C <= 3200) {
        const dim3 gridm((unsigned)cdiv(H * W, kHT * 4), (unsigned)M);
        if (C == 32)
            hipLaunchKernelGGL(head_local_fwd_mfma_kernel<32>, gridm, dim3(kHT), head_mfma_lds<32>(S), st, (const bf16*)feat, (int)H, (int)W,
                               src, flips, (int)M, w, b, (int)S, 1.0f / T, prob, simplex_tol, simplex_violations);
        else
            hipLaunchKernelGGL(head_local_fwd_mfma_kernel<16>, gridm, dim3(kHT), head_mfma_lds<16>(S), st, (const bf16*)feat, (int)H, (int)W,
                               src, flips, (int)M, w, b, (int)S, 1.0f / T, prob, simplex_tol, simplex_violations);
    } else if (K <= 32) {
        const bool quad = (H * W) % 4 == 0 && W % 4 == 0;
        if (quad) a.grid = dim3((unsigned)cdiv(H * W, kHT * 4), (unsigned)M);
        a.lds = (size_t)(S * K * C * 4);
        // the float kernels are in heads_f32.hip, a unit the fp16 build does not have
        MISEG_WITH_STORAGE_TYPE(dt, "head_local_fwd",
            if constexpr (std::is_same_v<TT, float>) return launch_head_fwd_reg_f32(a, quad);
            else return launch_head_fwd_reg<TT>(a, quad));
    } else {
        MISEG_WITH_STORAGE_TYPE(dt, "head_local_fwd",
            if constexpr (std::is_same_v<TT, float>) return launch_head_fwd_lds_f32(a);
            else return launch_head_fwd_lds<TT>(a));
    }
    MISEG_LAUNCH_CHECK("head_local_fwd_kernel");
    return MISEG_OK;
}
