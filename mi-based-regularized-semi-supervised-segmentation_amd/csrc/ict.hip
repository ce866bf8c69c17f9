// Interpolation consistency training (Trainer.name=ict; Verma et al. 2019): the three pixel-streaming kernels of its iteration.
//   cat_mixed           out = [a | c0 * b_i + c1 * b_perm[i]]: the student's input batch, labeled rows copied, unlabeled rows mixed
//   softmax_mix_mse     mean((softmax(a_i) - q_i)^2),                          q_i = c0 * softmax(b_i) + c1 * softmax(b_perm[i])
//   softmax_mix_klcons  mean_pix sum_c -q_c log((p_c + eps) / (q_c + eps)),    p = softmax(a_i), q as above, eps = 1e-16
// The mix is a GATHER: sample i's partner is perm[i].  (c0, c1) and perm are read from device memory -- they live in the iteration's
// step block, so a replayed launch tape reads each step's values.  A perm[i] outside [0, N) counts as i (no partner) and adds 1 to
// *bad; nothing is ever read out of range.
//
// All three are HBM-bound: cat_mixed moves 16 bytes per lane where a sample is a whole number of 16-byte vectors; the losses take one
// pixel per thread with the channel vectors in registers (one 16-byte load per row where C is a multiple of 4) and sum in two
// deterministic passes (per-block partial -> one finishing block), as the pixel losses of losses.hip do, with the helpers those use
// (pixel_loss.h: softmax_c, the row loads, the class-count dispatch; the finishing sum is the kernel of losses.hip).
//
// Rounding: a mixed value is fma(c0, x, c1 * y) -- the product c1 * y rounded, then one fused multiply-add -- pinned by intrinsics
// whatever -ffp-contract says.  With (c0, c1) = (1, 0) it is x and with (0, 1) it is y, exactly (finite operands; a zero keeps its
// value, not always its sign).
#include "pixel_loss.h"

namespace miseg {
namespace ict {

constexpr int kT = 256;
static_assert(kT == kPixelThreads, "pixel_blocks() counts blocks of kT pixels");

__device__ __forceinline__ float mix(float c0, float x, float c1, float y) { return __fmaf_rn(c0, x, __fmul_rn(c1, y)); }

// sample i's partner, or i itself where perm[i] is no sample of the batch (`first`: one thread per sample reports it)
__device__ __forceinline__ int64_t partner(const int32_t* __restrict__ perm, int64_t i, int64_t N, bool first, int32_t* __restrict__ bad) {
    const int32_t p = perm[i];
    if (p >= 0 && (int64_t)p < N) return p;
    if (first && bad) atomicAdd(bad, 1);
    return i;
}

// ---- batch assembly ---------------------------------------------------------------------------------------------------------
// VEC: one element = one 16-byte vector (per = vectors per sample); else one float.
template <bool VEC>
__global__ __launch_bounds__(kT) void cat_mixed_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out,
                                                       int64_t Na, int64_t Nb, int64_t per, const int32_t* __restrict__ perm,
                                                       const float* __restrict__ coef, int32_t* __restrict__ bad) {
    const float c0 = coef[0], c1 = coef[1];
    const int64_t total = (Na + Nb) * per, head = Na * per;
    for (int64_t e = blockIdx.x * (int64_t)kT + threadIdx.x; e < total; e += (int64_t)gridDim.x * kT) {
        if (e < head) {          // the labeled rows: bits, not floats
            if (VEC) reinterpret_cast<uint4*>(out)[e] = reinterpret_cast<const uint4*>(a)[e];
            else reinterpret_cast<uint32_t*>(out)[e] = reinterpret_cast<const uint32_t*>(a)[e];
            continue;
        }
        const int64_t m = (e - head) / per, r = (e - head) - m * per;
        const int64_t src = partner(perm, m, Nb, r == 0, bad) * per + r;
        if (VEC) {
            const float4 x = reinterpret_cast<const float4*>(b)[e - head], y = reinterpret_cast<const float4*>(b)[src];
            reinterpret_cast<float4*>(out)[e] = make_float4(mix(c0, x.x, c1, y.x), mix(c0, x.y, c1, y.y), mix(c0, x.z, c1, y.z), mix(c0, x.w, c1, y.w));
        } else {
            out[e] = mix(c0, b[e - head], c1, b[src]);
        }
    }
}

// ---- the two consistency losses -----------------------------------------------------------------------------------------------
// KL: the klcons form, else the MSE.  d/da_c = p_c (g_c - <g, p>) through the softmax Jacobian, with g = 2 (p - q) / (npix C) (MSE;
// the factor sits in `up`) or g_c = -q_c / (p_c + eps) / npix (KL).  Nothing flows to b.
template <int C, bool V4, bool KL>
__global__ __launch_bounds__(kT) void mix_loss_kernel(const float* __restrict__ a, const float* __restrict__ b, const int32_t* __restrict__ perm,
                                                      const float* __restrict__ coef, int64_t N, int64_t HW, int64_t npix,
                                                      const float* __restrict__ upstream, float* __restrict__ partials,
                                                      float* __restrict__ ga, int32_t* __restrict__ bad) {
    __shared__ float red[17];
    const float eps = 1e-16f;
    const float up = (upstream ? upstream[0] : 1.f) * (KL ? 1.f / (float)npix : 2.f / ((float)npix * (float)C));
    const float c0 = coef[0], c1 = coef[1];
    float part = 0.f;
    for (int64_t i = blockIdx.x * (int64_t)kT + threadIdx.x; i < npix; i += (int64_t)gridDim.x * kT) {
        const int64_t n = i / HW, r = i - n * HW;
        const int64_t j = partner(perm, n, N, r == 0, bad) * HW + r;
        float z[C], p[C], q[C], t[C];
        load_row<C, V4>(b + i * C, z);
        softmax_c(z, C, q);
        load_row<C, V4>(b + j * C, z);
        softmax_c(z, C, t);
#pragma unroll
        for (int c = 0; c < C; ++c) q[c] = mix(c0, q[c], c1, t[c]);
        load_row<C, V4>(a + i * C, z);
        softmax_c(z, C, p);
        float acc = 0.f, dot = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            if (KL) {
                acc += -q[c] * logf((p[c] + eps) / (q[c] + eps));
                t[c] = -q[c] / (p[c] + eps);
            } else {
                t[c] = p[c] - q[c];
                acc += t[c] * t[c];
            }
            dot += t[c] * p[c];
        }
        part += acc;
        if (ga) {
#pragma unroll
            for (int c = 0; c < C; ++c) z[c] = up * p[c] * (t[c] - dot);
            store_row<C, V4>(ga + i * C, z);
        }
    }
    part = block_sum(part, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = part;
}

template <bool KL>
static int mix_loss(const char* who, void* stream, const float* a, const float* b, const int32_t* perm, const float* coef, int64_t N, int64_t H,
                    int64_t W, int64_t C, const float* upstream, float* loss, float* ga, int32_t* bad, void* ws, int64_t ws_bytes) {
    if (!(a && b && perm && coef && loss && ws)) return fail(MISEG_E_INVALID, "%s: null pointer", who);
    if (!class_count_has_kernel(C)) return fail(MISEG_E_INVALID, "%s: unsupported class count %ld (2-6,8,10,16)", who, (long)C);
    if (!(N > 0 && H > 0 && W > 0 && N < (1LL << 31))) return fail(MISEG_E_INVALID, "%s: empty batch / bad shape", who);
    const int64_t need = miseg_loss_ws_bytes(N, H, W);
    if (ws_bytes < need) return fail(MISEG_E_INVALID, "%s: workspace of %ld bytes, %ld needed", who, (long)ws_bytes, (long)need);
    const int64_t npix = N * H * W;
    const int nb = pixel_blocks(npix);
    const bool v4 = C % 4 == 0 && aligned16(a) && aligned16(b) && (!ga || aligned16(ga));
    hipStream_t st = as_stream(stream);
#define L(CC, VV) hipLaunchKernelGGL((mix_loss_kernel<CC, VV, KL>), dim3(nb), dim3(kT), 0, st, a, b, perm, coef, N, H * W, npix, upstream, (float*)ws, ga, bad)
    MISEG_DISPATCH_C_V4(C, v4, L)
#undef L
    MISEG_LAUNCH_CHECK("mix_loss_kernel");
    return launch_finish_sum(st, (const float*)ws, nb, 1.0f / (KL ? (float)npix : (float)npix * (float)C), loss);
}

}  // namespace ict
}  // namespace miseg

using namespace miseg;

extern "C" int miseg_cat_mixed(void* stream, const float* a, int64_t Na, const float* b, int64_t Nb, int64_t C, int64_t H, int64_t W,
                               const int32_t* perm, const float* coef, float* out, int32_t* bad) {
    MISEG_TAPE(miseg_cat_mixed, stream, a, Na, b, Nb, C, H, W, perm, coef, out, bad);
    MISEG_REQUIRE(out && b && perm && coef && (a || Na == 0), "cat_mixed: null pointer");
    MISEG_REQUIRE(Na >= 0 && Nb > 0 && Nb < (1LL << 31) && C > 0 && H > 0 && W > 0, "cat_mixed: empty batch / bad shape");
    MISEG_REQUIRE(out != b && out != a, "cat_mixed: in-place not supported");
    const int64_t per = C * H * W;
    const bool vec = per % 4 == 0 && aligned16(out) && aligned16(b) && (Na == 0 || aligned16(a));
    const int64_t units = (Na + Nb) * (vec ? per / 4 : per);
    const dim3 grid((unsigned)std::min<int64_t>(cdiv(units, ict::kT), 2048));
    if (vec) hipLaunchKernelGGL(ict::cat_mixed_kernel<true>, grid, dim3(ict::kT), 0, as_stream(stream), a, b, out, Na, Nb, per / 4, perm, coef, bad);
    else hipLaunchKernelGGL(ict::cat_mixed_kernel<false>, grid, dim3(ict::kT), 0, as_stream(stream), a, b, out, Na, Nb, per, perm, coef, bad);
    MISEG_LAUNCH_CHECK("cat_mixed_kernel");
    return MISEG_OK;
}

extern "C" int miseg_softmax_mix_mse(void* stream, const float* a, const float* b, const int32_t* perm, const float* coef, int64_t N, int64_t H,
                                     int64_t W, int64_t C, const float* upstream, float* loss, float* ga, int32_t* bad, void* ws,
                                     int64_t ws_bytes) {
    MISEG_TAPE(miseg_softmax_mix_mse, stream, a, b, perm, coef, N, H, W, C, upstream, loss, ga, bad, ws, ws_bytes);
    return ict::mix_loss<false>("softmax_mix_mse", stream, a, b, perm, coef, N, H, W, C, upstream, loss, ga, bad, ws, ws_bytes);
}

extern "C" int miseg_softmax_mix_klcons(void* stream, const float* a, const float* b, const int32_t* perm, const float* coef, int64_t N, int64_t H,
                                        int64_t W, int64_t C, const float* upstream, float* loss, float* ga, int32_t* bad, void* ws,
                                        int64_t ws_bytes) {
    MISEG_TAPE(miseg_softmax_mix_klcons, stream, a, b, perm, coef, N, H, W, C, upstream, loss, ga, bad, ws, ws_bytes);
    return ict::mix_loss<true>("softmax_mix_klcons", stream, a, b, perm, coef, N, H, W, C, upstream, loss, ga, bad, ws, ws_bytes);
}
