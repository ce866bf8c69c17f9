// The forward kernels of the local head that exist per storage type, and their launchers: heads_fwd.hip instantiates them on the
// 16-bit type, heads_f32.hip on float (heads.h has the file map).
#pragma once
#include "heads.h"

namespace miseg {

template <typename T>
__global__ __launch_bounds__(kHT) void head_local_fwd_kernel(const T* __restrict__ feat, int H, int W, int C,
                                                             const int32_t* __restrict__ src, const int32_t* __restrict__ flips,
                                                             int M, const float* __restrict__ w, const float* __restrict__ b, int S,
                                                             int K, float invT, float* __restrict__ prob) {
    extern __shared__ float zs[];  // [K][kHT]
    const int tid = threadIdx.x, HW = H * W;
    const int m = blockIdx.y;
    const int pix = blockIdx.x * kHT + tid;
    const bool live = pix < HW;
    const int h = live ? pix / W : 0, wq = live ? pix % W : 0;
    const int f = flips ? flips[m] : 0;
    const T* fp = feat + ((size_t)src[m] * HW + (size_t)flip_h(h, H, f) * W + flip_w(wq, W, f)) * C;
    for (int s = 0; s < S; ++s) {
        const float* ws = w + (size_t)s * K * C;
        for (int k = 0; k < K; ++k) zs[k * kHT + tid] = b[s * K + k];
        for (int c0 = 0; c0 < C; c0 += 4) {
            Vec4<T> fv = *reinterpret_cast<const Vec4<T>*>(fp + c0);
            const float f0 = fv.get(0), f1 = fv.get(1), f2 = fv.get(2), f3 = fv.get(3);
            for (int k = 0; k < K; ++k) {
                const float* wr = ws + (size_t)k * C + c0;
                zs[k * kHT + tid] += wr[0] * f0 + wr[1] * f1 + wr[2] * f2 + wr[3] * f3;
            }
        }
        float mx = -3.4e38f;
        for (int k = 0; k < K; ++k) {
            float z = zs[k * kHT + tid] * invT;
            zs[k * kHT + tid] = z;
            mx = fmaxf(mx, z);
        }
        float sum = 0.f;
        for (int k = 0; k < K; ++k) {
            float e = expf(zs[k * kHT + tid] - mx);
            zs[k * kHT + tid] = e;
            sum += e;
        }
        if (live) {
            float* out = prob + (((size_t)s * M + m) * K) * HW + pix;
            for (int k = 0; k < K; ++k) out[(size_t)k * HW] = zs[k * kHT + tid] / sum;
        }
    }
}

// Register-resident variant for K <= 32 (KP = K rounded up to a multiple of 4): the K logits of a pixel live in VGPRs,
// the head weights arrive as scalar operands (wave-uniform addresses -> scalar cache), so a sub-head costs K*C FMAs per
// pixel and no LDS traffic at all (the LDS-column kernel above spends ~15 LDS operations per logit update).
// Logits accumulate through explicit FMAs (channel order) and the softmax multiplies by one reciprocal per pixel: results
// differ from head_local_fwd_kernel by an ulp or two, inside the parity tolerance of tests/test_gpu_mi.py.
template <typename T, int KP, int PPT, bool EXACT>   // EXACT: K == KP, no per-class guards (K = 20 ships)
__global__ __launch_bounds__(kHT) void head_local_fwd_reg_kernel(const T* __restrict__ feat, int H, int W, int C,
                                                                 const int32_t* __restrict__ src, const int32_t* __restrict__ flips,
                                                                 int M, const float* __restrict__ w, const float* __restrict__ b, int S,
                                                                 int K, float invT, float* __restrict__ prob, float tol,
                                                                 int32_t* __restrict__ viol) {
    // PPT consecutive pixels per thread (PPT = 4 needs HW % 4 == 0): every (s,k) plane is then written in 16-byte pieces,
    // 4 KB contiguous per block, instead of 100 interleaved 1 KB streams
    const int tid = threadIdx.x, HW = H * W;
    const int m = blockIdx.y;
    const int pix0 = (blockIdx.x * kHT + tid) * PPT;
    const bool live = pix0 < HW;
    const int f = flips ? flips[m] : 0;
    // all S*K*C weights staged once per block; the inner loop reads them as broadcast ds_read_b128 (every lane the same
    // address), which the compiler keeps a dozen deep in flight -- as scalar loads each batch of weights was a serial
    // scalar-cache round trip in front of its FMAs
    extern __shared__ __attribute__((aligned(16))) float wl[];
    for (int i = tid; i < S * K * C; i += kHT) wl[i] = w[i];
    __syncthreads();
    const T* fp[PPT];
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
        const int pix = live ? pix0 + j : 0, h = pix / W, wq = pix % W;
        fp[j] = feat + ((size_t)src[m] * HW + (size_t)flip_h(h, H, f) * W + flip_w(wq, W, f)) * C;
    }
    int nbad = 0;
    for (int s = 0; s < S; ++s) {
        const float* ws = wl + (size_t)s * K * C;
        float z[PPT][KP];
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            const float bv = b[s * K + (EXACT ? k : min(k, K - 1))];
#pragma unroll
            for (int j = 0; j < PPT; ++j) z[j][k] = bv;
        }
        for (int c0 = 0; c0 < C; c0 += 4) {
            float fr[PPT][4];
#pragma unroll
            for (int j = 0; j < PPT; ++j) {
                Vec4<T> fv = *reinterpret_cast<const Vec4<T>*>(fp[j] + c0);
#pragma unroll
                for (int i = 0; i < 4; ++i) fr[j][i] = fv.get(i);
            }
#pragma unroll
            for (int k = 0; k < KP; ++k) {
                const float4 wq4 = *reinterpret_cast<const float4*>(ws + (size_t)(EXACT ? k : min(k, K - 1)) * C + c0);
                const float w0 = wq4.x, w1 = wq4.y, w2 = wq4.z, w3 = wq4.w;
#pragma unroll
                for (int j = 0; j < PPT; ++j) z[j][k] = fmaf(w3, fr[j][3], fmaf(w2, fr[j][2], fmaf(w1, fr[j][1], fmaf(w0, fr[j][0], z[j][k]))));
            }
        }
#pragma unroll
        for (int j = 0; j < PPT; ++j) {
            // softmax(z / T): exp((z - max) / T) as ONE fma + v_exp_f32 (exp2 of a pre-scaled argument).  The library expf spends
            // ~12 instructions per value on range handling this argument (<= 0, finite) never needs -- it was 40 % of the kernel's
            // instructions -- and v_exp_f32 is accurate to ~1 ulp, inside the 1e-5 parity bound on the probabilities.
            float mx = -3.4e38f;
#pragma unroll
            for (int k = 0; k < KP; ++k)
                if (EXACT || k < K) mx = fmaxf(mx, z[j][k]);
            const float sc2 = invT * 1.4426950408889634f, off2 = -mx * sc2;
            float sum = 0.f;
#pragma unroll
            for (int k = 0; k < KP; ++k) {
                z[j][k] = __builtin_amdgcn_exp2f(fmaf(z[j][k], sc2, off2));
                if (EXACT || k < K) sum += z[j][k];
            }
            const float inv = 1.0f / sum;
            float ps = 0.f;
#pragma unroll
            for (int k = 0; k < KP; ++k) {
                z[j][k] *= inv;
                if (EXACT || k < K) ps += z[j][k];
            }
            nbad += !(fabsf(ps - 1.f) <= tol);   // the caller's simplex assertion, evaluated while the values are in registers
        }
        if (live) {
            float* out = prob + (((size_t)s * M + m) * K) * HW + pix0;
#pragma unroll
            for (int k = 0; k < KP; ++k)
                if (EXACT || k < K) {
                    if (PPT == 4) *reinterpret_cast<float4*>(out + (size_t)k * HW) = make_float4(z[0][k], z[1][k], z[2][k], z[3][k]);
                    else out[(size_t)k * HW] = z[0][k];
                }
        }
    }
    if (viol && live && nbad) atomicAdd(viol, nbad);
}

template <typename TT>
int launch_head_fwd_lds(const HeadFwd& a) {
    hipLaunchKernelGGL(head_local_fwd_kernel<TT>, a.grid, dim3(kHT), a.lds, a.st, (const TT*)a.feat, a.H, a.W, a.C, a.src, a.flips, a.M, a.w, a.b, a.S,
                       a.K, a.invT, a.prob);
    return MISEG_OK;
}

// quad: 4 consecutive pixels per thread (the entry point has sized a.grid for it)
template <typename TT>
int launch_head_fwd_reg(const HeadFwd& a, bool quad) {
    const int K = a.K;
#define HLF_L(KPP, PPT, EX)                                                                                                             \
    hipLaunchKernelGGL((head_local_fwd_reg_kernel<TT, KPP, PPT, EX>), a.grid, dim3(kHT), a.lds, a.st, (const TT*)a.feat, a.H, a.W, a.C, a.src, a.flips, \
                       a.M, a.w, a.b, a.S, a.K, a.invT, a.prob, a.tol, a.viol)
#define HLF(KPP)                                \
    {                                           \
        if (quad && K == KPP) HLF_L(KPP, 4, true); \
        else if (quad) HLF_L(KPP, 4, false);    \
        else HLF_L(KPP, 1, false);              \
    }
    switch ((K + 3) / 4) {
        case 1: HLF(4); break;
        case 2: HLF(8); break;
        case 3: HLF(12); break;
        case 4: HLF(16); break;
        case 5: HLF(20); break;
        case 6: HLF(24); break;
        case 7: HLF(28); break;
        case 8: HLF(32); break;
        default: return MISEG_E_INVALID;
    }
#undef HLF
#undef HLF_L
    return MISEG_OK;
}

}  // namespace miseg
