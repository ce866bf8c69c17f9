// Generalized Dice loss (optionally + KL) on fp32 NHWC logits: whl:deepclustering2/loss/dice_loss.py:79-135 on softmax(logits) with the
// one-hot of class2one_hot taken from int64 labels.  Per sample n and class c
//     I = sum_px p_c [label == c],   D = sum_px p_c^pow + n_c,   dice = w_c (1 - (2 I + eps) / (D + eps)),   GDL = mean_{n,c} dice,
// so the gradient of a pixel needs the FINISHED sums of its sample: three launches.
//   1. dice_partials_kernel   one pixel per thread, softmax in registers (as csrc/losses.hip); a block stays inside one sample
//                             (grid = blocks per sample x N, grid-stride inside the sample) and writes, per class, its partial
//                             I, S = sum p^pow, the integer label count and -- with a KL weight -- the KL partial.  No atomics.
//   2. dice_finish_kernel     one block, 16 lanes per (n, c): the partials summed in a fixed order in double, the two gradient
//                             coefficients a = -2 w / (D + eps), b = w (2 I + eps) pow / (D + eps)^2, both times
//                             dice_weight * upstream / (N C), and the scalar loss.
//   3. dice_grad_kernel       (only with glogits) softmax again, g_c = a [label == c] + b p_c^(pow-1) (+ the KL term at the label's
//                             class), dz_c = p_c (g_c - <g, p>).
// A label outside [0, C) sets *bad_label; that pixel adds to none of the sums and its gradient row is written as zeros.
#include "pixel_loss.h"

namespace miseg {
namespace dice {

constexpr int kDT = 256;        // threads per block of the two pixel passes
constexpr int kWaves = kDT / 64;
constexpr int kMaxBps = 128;    // blocks per sample: a sample with more than kMaxBps * kDT pixels takes the grid-stride loop
constexpr int kFT = 1024;       // threads of the finish block
constexpr int kTPE = 16;        // ... of which this many adjacent lanes sum one (sample, class)
constexpr int kEPR = kFT / kTPE;

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ double wave_sum_double(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// workspace: float I[N*C][bps] | float S[N*C][bps] | int32 cnt[N*C][bps] | float kl[N][bps] | float a[N*C] | float b[N*C]
struct Layout {
    int64_t I, S, cnt, kl, coef, end;      // offsets in 4-byte words
};
static Layout layout(int64_t N, int64_t C, int64_t bps) {
    Layout l;
    l.I = 0;
    l.S = l.I + N * C * bps;
    l.cnt = l.S + N * C * bps;
    l.kl = l.cnt + N * C * bps;
    l.coef = l.kl + N * bps;
    l.end = l.coef + 2 * N * C;
    return l;
}
static int blocks_per_sample(int64_t HW) { return (int)std::min<int64_t>(cdiv(HW, kDT), kMaxBps); }

template <int C, int POW, bool KL>
__global__ __launch_bounds__(kDT) void dice_partials_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                            int64_t HW, float* __restrict__ pI, float* __restrict__ pS,
                                                            int32_t* __restrict__ pcnt, float* __restrict__ pkl,
                                                            int32_t* __restrict__ bad) {
    __shared__ float red_f[kWaves][2 * C + 1];
    __shared__ int red_i[kWaves][C];
    const int n = blockIdx.y, bps = gridDim.x;
    const int64_t base = (int64_t)n * HW;
    const float eps = 1e-16f;
    float ai[C], as[C], akl = 0.f;
    int an[C];
#pragma unroll
    for (int c = 0; c < C; ++c) { ai[c] = 0.f; as[c] = 0.f; an[c] = 0; }
    for (int64_t i = blockIdx.x * (int64_t)kDT + threadIdx.x; i < HW; i += (int64_t)bps * kDT) {
        float z[C], p[C];
#pragma unroll
        for (int c = 0; c < C; ++c) z[c] = logits[(base + i) * C + c];
        softmax_c(z, C, p);
        const int64_t t = labels[base + i];
        if (t < 0 || t >= C) { *bad = 1; continue; }
        float kl = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const bool hit = c == t;
            ai[c] += hit ? p[c] : 0.f;
            as[c] += POW == 1 ? p[c] : p[c] * p[c];
            an[c] += hit ? 1 : 0;
            if (KL) {
                const float tc = hit ? 1.f : 0.f;
                kl += -tc * logf((p[c] + eps) / (tc + eps));
            }
        }
        akl += kl;
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float vi = wave_sum(ai[c]), vs = wave_sum(as[c]);
        const int vn = wave_sum_int(an[c]);
        if (lane == 0) { red_f[wid][c] = vi; red_f[wid][C + c] = vs; red_i[wid][c] = vn; }
    }
    if (KL) {
        const float vk = wave_sum(akl);
        if (lane == 0) red_f[wid][2 * C] = vk;
    }
    __syncthreads();
    if (threadIdx.x < C) {       // the waves in a fixed order
        const int c = threadIdx.x;
        float si = 0.f, ss = 0.f;
        int sn = 0;
        for (int w = 0; w < kWaves; ++w) { si += red_f[w][c]; ss += red_f[w][C + c]; sn += red_i[w][c]; }
        const int64_t o = ((int64_t)n * C + c) * bps + blockIdx.x;
        pI[o] = si;
        pS[o] = ss;
        pcnt[o] = sn;
    }
    if (KL && threadIdx.x == 64) {
        float sk = 0.f;
        for (int w = 0; w < kWaves; ++w) sk += red_f[w][2 * C];
        pkl[(int64_t)n * bps + blockIdx.x] = sk;
    }
}

__global__ __launch_bounds__(kFT) void dice_finish_kernel(const float* __restrict__ pI, const float* __restrict__ pS,
                                                          const int32_t* __restrict__ pcnt, const float* __restrict__ pkl, int N, int C,
                                                          int bps, int pow, float eps, const float* __restrict__ class_weight,
                                                          float kl_weight, float dice_weight, const float* __restrict__ upstream,
                                                          int64_t npix, float* __restrict__ coef, float* __restrict__ loss) {
    // kTPE adjacent lanes share one (n, c): each sums every kTPE-th partial (independent, coalesced loads), four shuffle steps join them.
    // Measured at [16,4,256,256]: 8.8 us; one wave per class (four classes in a row per wave, 18 double shuffles each) took 9.7 us.
    __shared__ double red_d[kEPR], red_k[kFT / 64];
    const int sub = threadIdx.x & (kTPE - 1), slot = threadIdx.x / kTPE;
    const int NC = N * C;
    const double scale = (double)dice_weight * (double)(upstream ? upstream[0] : 1.f) / (double)NC;
    double acc = 0.0;       // this slot's classes, in the order it meets them
    for (int e0 = 0; e0 < NC; e0 += kEPR) {
        const int e = e0 + slot;
        double si = 0.0, ss = 0.0, sn = 0.0;
        if (e < NC) {
#pragma unroll 8
            for (int j = sub; j < bps; j += kTPE) {
                const int64_t o = (int64_t)e * bps + j;
                si += (double)pI[o];
                ss += (double)pS[o];
                sn += (double)pcnt[o];
            }
        }
#pragma unroll
        for (int o = kTPE / 2; o > 0; o >>= 1) {
            si += __shfl_xor(si, o, 64);
            ss += __shfl_xor(ss, o, 64);
            sn += __shfl_xor(sn, o, 64);
        }
        if (e < NC) {
            const double w = class_weight ? (double)class_weight[e % C] : 1.0;
            const double den = ss + sn + (double)eps, num = 2.0 * si + (double)eps;
            if (sub == 0) {
                coef[e] = (float)(-2.0 * w / den * scale);
                coef[NC + e] = (float)(w * num * (double)pow / (den * den) * scale);
            }
            acc += w * (1.0 - num / den);
        }
    }
    double kl = 0.0;
    if (pkl) {
        const int total = N * bps;
        for (int j = threadIdx.x; j < total; j += kFT) kl += (double)pkl[j];
        kl = wave_sum_double(kl);
    }
    if (sub == 0) red_d[slot] = acc;
    if ((threadIdx.x & 63) == 0) red_k[threadIdx.x >> 6] = kl;
    __syncthreads();
    if (threadIdx.x == 0) {       // fixed order
        double d = 0.0, k = 0.0;
        for (int i = 0; i < kEPR; ++i) d += red_d[i];
        for (int i = 0; i < kFT / 64; ++i) k += red_k[i];
        double total = (double)dice_weight * d / (double)NC;
        if (pkl) total += (double)kl_weight * k / (double)npix;
        loss[0] = (float)total;
    }
}

__device__ __noinline__ void zero_row(float* __restrict__ g, int C) { for (int c = 0; c < C; ++c) g[c] = 0.f; }

template <int C, int POW, bool KL>
__global__ __launch_bounds__(kDT) void dice_grad_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels, int64_t HW,
                                                        const float* __restrict__ coef, int NC, const float* __restrict__ upstream,
                                                        float kl_weight, int64_t npix, float* __restrict__ glogits) {
    const int n = blockIdx.y;
    const int64_t base = (int64_t)n * HW;
    const float eps = 1e-16f;
    const float klup = KL ? kl_weight * ((upstream ? upstream[0] : 1.f) / (float)npix) : 0.f;
    float a[C], b[C];
#pragma unroll
    for (int c = 0; c < C; ++c) { a[c] = coef[n * C + c]; b[c] = coef[NC + n * C + c]; }
    for (int64_t i = blockIdx.x * (int64_t)kDT + threadIdx.x; i < HW; i += (int64_t)gridDim.x * kDT) {
        float z[C], p[C], g[C];
#pragma unroll
        for (int c = 0; c < C; ++c) z[c] = logits[(base + i) * C + c];
        softmax_c(z, C, p);
        const int64_t t = labels[base + i];
        float* out = glogits + (base + i) * C;
        if (t < 0 || t >= C) { zero_row(out, C); continue; }
        float dot = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const bool hit = c == t;
            g[c] = (hit ? a[c] : 0.f) + (POW == 1 ? b[c] : b[c] * p[c]);
            if (KL && hit) g[c] += -1.f / (p[c] + eps) * klup;
            dot += g[c] * p[c];
        }
#pragma unroll
        for (int c = 0; c < C; ++c) out[c] = p[c] * (g[c] - dot);
    }
}

}  // namespace dice
}  // namespace miseg

using namespace miseg;
using namespace miseg::dice;

extern "C" int64_t miseg_softmax_dice_ws_bytes(int64_t N, int64_t H, int64_t W, int64_t C) {
    if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || N > 65535 || C > 32) return -1;
    return layout(N, C, blocks_per_sample(H * W)).end * 4;
}

// MACRO(C, POW, KL) at the call's class count and power, with or without the KL term
#define MISEG_DICE_VARIANT(C, MACRO)                                                  \
    do {                                                                              \
        if (pow == 1) {                                                               \
            if (with_kl) { MISEG_DISPATCH_C(C, MACRO, 1, true) } else { MISEG_DISPATCH_C(C, MACRO, 1, false) } \
        } else {                                                                      \
            if (with_kl) { MISEG_DISPATCH_C(C, MACRO, 2, true) } else { MISEG_DISPATCH_C(C, MACRO, 2, false) } \
        }                                                                             \
    } while (0)

extern "C" int miseg_softmax_dice(void* stream, const float* logits, const int64_t* labels, int64_t N, int64_t H, int64_t W, int64_t C,
                                  int pow, float eps, const float* class_weight, float kl_weight, float dice_weight,
                                  const float* upstream, float* loss, float* glogits, int32_t* bad_label, void* ws, int64_t ws_bytes) {
    MISEG_TAPE(miseg_softmax_dice, stream, logits, labels, N, H, W, C, pow, eps, class_weight, kl_weight, dice_weight, upstream, loss,
               glogits, bad_label, ws, ws_bytes);
    MISEG_REQUIRE(logits && labels && loss && bad_label && ws, "softmax_dice: null pointer");
    MISEG_REQUIRE(N > 0 && H > 0 && W > 0 && N <= 65535, "softmax_dice: bad shape");
    if (!class_count_has_kernel(C)) return fail(MISEG_E_INVALID, "unsupported class count %ld (2-6,8,10,16)", (long)C);
    MISEG_REQUIRE(pow == 1 || pow == 2, "softmax_dice: pow must be 1 or 2");
    MISEG_REQUIRE(ws_bytes >= miseg_softmax_dice_ws_bytes(N, H, W, C), "softmax_dice: workspace too small");
    const int64_t HW = H * W, npix = N * HW;
    const int bps = blocks_per_sample(HW);
    const Layout l = layout(N, C, bps);
    float* wf = (float*)ws;
    float *pI = wf + l.I, *pS = wf + l.S, *pkl = wf + l.kl, *coef = wf + l.coef;
    int32_t* pcnt = (int32_t*)ws + l.cnt;
    const bool with_kl = kl_weight != 0.f;
    const dim3 grid((unsigned)bps, (unsigned)N);
    hipStream_t st = as_stream(stream);
#define P(CC, PP, KK) hipLaunchKernelGGL((dice_partials_kernel<CC, PP, KK>), grid, dim3(kDT), 0, st, logits, labels, HW, pI, pS, pcnt, pkl, bad_label)
    MISEG_DICE_VARIANT(C, P);
#undef P
    MISEG_LAUNCH_CHECK("dice_partials_kernel");
    hipLaunchKernelGGL(dice_finish_kernel, dim3(1), dim3(kFT), 0, st, (const float*)pI, (const float*)pS, (const int32_t*)pcnt,
                       with_kl ? (const float*)pkl : (const float*)nullptr, (int)N, (int)C, bps, pow, eps, class_weight, kl_weight,
                       dice_weight, upstream, npix, coef, loss);
    MISEG_LAUNCH_CHECK("dice_finish_kernel");
    if (glogits) {
#define G(CC, PP, KK) hipLaunchKernelGGL((dice_grad_kernel<CC, PP, KK>), grid, dim3(kDT), 0, st, logits, labels, HW, (const float*)coef, (int)(N * C), upstream, kl_weight, npix, glogits)
        MISEG_DICE_VARIANT(C, G);
#undef G
        MISEG_LAUNCH_CHECK("dice_grad_kernel");
    }
    return MISEG_OK;
}
