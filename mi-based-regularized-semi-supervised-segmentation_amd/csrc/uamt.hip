// Uncertainty-aware Mean Teacher (Trainer.name=uamt; Yu et al., MICCAI 2019): the three streaming kernels of its iteration.
//   noise_add      out[p] = x + clamp(sigma * z[p], -clip, +clip), p = 0..passes-1: the teacher's noisy copies of the unlabeled batch;
//                  z is the stream miseg_normal_fill defines for (seed64, p * M + i), the seed READ FROM THE DEVICE
//   softmax_accum  acc = first ? softmax(logits) : acc + softmax(logits): the sum of the teacher's predictions over the passes
//   softmax_umse   sum_pix mask * sum_c (softmax(a) - softmax(b))_c^2 / (C K + 1e-16),  mask = unc < thr,  K = sum mask,
//                  unc = -sum_c m_c log(m_c + 1e-6),  m = acc * inv_passes
// Seed and threshold live in the iteration's step block, so a replayed launch tape reads each step's values.
//
// All three are HBM-bound.  noise_add moves 16 bytes per lane where a copy is a whole number of aligned 16-byte vectors (then one
// Philox counter block is one vector); the pixel kernels take one pixel per thread with the channel vectors in registers (one 16-byte
// load per row where C is a multiple of 4).  softmax_umse sums in two deterministic passes (per-block partials -> one finishing
// block); the count K is an exact integer; the gradient's denominator is only known after the reduction, so the first pass stores
// the unscaled gradient 2 p_c (d_c - <d, p>) (exactly 0 at a masked-out pixel) and a last launch multiplies it by
// upstream / (C K + 1e-16), formed in double and rounded once.  The softmax, the row loads, the pixel grid and the class-count dispatch
// are those of pixel_loss.h, inline and so compiled under this unit's flags.  Built without contraction: the noise is one multiply, a
// clamp and one add, and its normals are the bits of vat.hip's.
#include "pixel_loss.h"
#include "philox.h"

namespace miseg {
namespace uamt {

constexpr int kT = 256;
static_assert(kT == kPixelThreads, "pixel_blocks() counts blocks of kT pixels");

// ---- the noisy copies -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float noisy(float x, float z, float sigma, float clip) {
    return __fadd_rn(x, fminf(fmaxf(__fmul_rn(sigma, z), -clip), clip));
}

// one thread = one counter block = elements [4 b, 4 b + 4) of the flat output [passes][M]; element j reads x[j mod M]
template <bool VEC>
__global__ __launch_bounds__(kT) void noise_add_kernel(const float* __restrict__ x, int64_t M, int64_t total, const int32_t* __restrict__ seed,
                                                       float sigma, float clip, float* __restrict__ out) {
    const unsigned long long seed64 = (unsigned long long)(uint32_t)seed[0] | ((unsigned long long)(uint32_t)seed[1] << 32);
    const int64_t nblk = (total + 3) >> 2;
    for (int64_t b = blockIdx.x * (int64_t)kT + threadIdx.x; b < nblk; b += (int64_t)gridDim.x * kT) {
        float z[4];
        philox_normals(philox_block(seed64, (unsigned long long)b), z);
        const int64_t j = 4 * b;
        if (VEC) {       // M % 4 == 0: the four elements lie in one pass and in one aligned vector of x
            const float4 v = *reinterpret_cast<const float4*>(x + j % M);
            *reinterpret_cast<float4*>(out + j) = make_float4(noisy(v.x, z[0], sigma, clip), noisy(v.y, z[1], sigma, clip),
                                                              noisy(v.z, z[2], sigma, clip), noisy(v.w, z[3], sigma, clip));
        } else {
#pragma unroll
            for (int l = 0; l < 4; ++l)
                if (j + l < total) out[j + l] = noisy(x[(j + l) % M], z[l], sigma, clip);
        }
    }
}

// ---- the pixel kernels ------------------------------------------------------------------------------------------------------------
template <int C, bool V4>
__global__ __launch_bounds__(kT) void softmax_accum_kernel(const float* __restrict__ logits, int64_t npix, int first, float* __restrict__ acc) {
    for (int64_t i = blockIdx.x * (int64_t)kT + threadIdx.x; i < npix; i += (int64_t)gridDim.x * kT) {
        float z[C], p[C];
        load_row<C, V4>(logits + i * C, z);
        softmax_c(z, C, p);
        if (!first) {
            load_row<C, V4>(acc + i * C, z);
#pragma unroll
            for (int c = 0; c < C; ++c) p[c] = z[c] + p[c];
        }
        store_row<C, V4>(acc + i * C, p);
    }
}

// The workspace: K partials (int64 [nb]) | masked squared-distance partials (fp32 [nb]) | uncertainty partials (fp32 [nb]) | the
// gradient's scale (fp32 [1]).
struct Workspace {
    long long* kept;
    float* dist;
    float* unc;
    float* gscale;
    __host__ __device__ Workspace(void* ws, int nb)
        : kept(static_cast<long long*>(ws)), dist(reinterpret_cast<float*>(kept + nb)), unc(dist + nb), gscale(unc + nb) {}
};

// pass 1: per-block partials, and the unscaled gradient g0_c = mask * 2 p_c (d_c - <d, p>) (softmax Jacobian applied to 2 d)
template <int C, bool V4>
__global__ __launch_bounds__(kT) void umse_kernel(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ acc,
                                                  int64_t npix, float inv_passes, const float* __restrict__ thr, void* __restrict__ ws,
                                                  float* __restrict__ ga) {
    __shared__ float red[17];
    __shared__ long long redk[17];
    const float th = thr[0];
    float part = 0.f, upart = 0.f;
    long long kept = 0;
    for (int64_t i = blockIdx.x * (int64_t)kT + threadIdx.x; i < npix; i += (int64_t)gridDim.x * kT) {
        float z[C], p[C], q[C];
        load_row<C, V4>(acc + i * C, z);
        float unc = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float m = z[c] * inv_passes;
            unc -= m * logf(m + 1e-6f);
        }
        const bool certain = unc < th;
        upart += unc;
        kept += certain ? 1 : 0;
        if (!certain) {         // masked out: nothing to the sum, an exactly zero gradient
            if (ga) {
#pragma unroll
                for (int c = 0; c < C; ++c) z[c] = 0.f;
                store_row<C, V4>(ga + i * C, z);
            }
            continue;
        }
        load_row<C, V4>(b + i * C, z);
        softmax_c(z, C, q);
        load_row<C, V4>(a + i * C, z);
        softmax_c(z, C, p);
        float s = 0.f, dot = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            q[c] = p[c] - q[c];
            s += q[c] * q[c];
            dot += q[c] * p[c];
        }
        part += s;
        if (ga) {
#pragma unroll
            for (int c = 0; c < C; ++c) z[c] = 2.f * p[c] * (q[c] - dot);
            store_row<C, V4>(ga + i * C, z);
        }
    }
    part = block_sum(part, red);
    upart = block_sum(upart, red);
    kept = block_sum_i64(kept, redk);
    if (threadIdx.x == 0) {
        const Workspace w(ws, gridDim.x);
        w.kept[blockIdx.x] = kept;
        w.dist[blockIdx.x] = part;
        w.unc[blockIdx.x] = upart;
    }
}

// pass 2, one block: the partials in a fixed order, then everything that needs K
__global__ __launch_bounds__(256) void umse_finish_kernel(void* __restrict__ ws, int nb, int64_t npix, int C, const float* __restrict__ upstream,
                                                          float* __restrict__ loss, long long* __restrict__ kept, float* __restrict__ stats) {
    __shared__ float red[17];
    __shared__ long long redk[17];
    const Workspace w(ws, nb);
    float s = 0.f, u = 0.f;
    long long k = 0;
    for (int i = threadIdx.x; i < nb; i += 256) { s += w.dist[i]; u += w.unc[i]; k += w.kept[i]; }
    s = block_sum(s, red);
    u = block_sum(u, red);
    k = block_sum_i64(k, redk);
    if (threadIdx.x == 0) {
        const double denom = (double)C * (double)k + 1e-16;
        loss[0] = (float)((double)s / denom);
        w.gscale[0] = (float)((double)(upstream ? upstream[0] : 1.f) / denom);
        if (kept) kept[0] = k;
        if (stats) {
            stats[0] = (float)((double)k / (double)npix);
            stats[1] = (float)((double)u / (double)npix);
        }
    }
}

// pass 3: ga = g0 * upstream / (C K + 1e-16); a zero stays +0.0 whatever the scale's sign
template <bool VEC>
__global__ __launch_bounds__(kT) void umse_scale_kernel(float* __restrict__ ga, int64_t units, const float* __restrict__ gscale) {
    const float sc = gscale[0];
    for (int64_t e = blockIdx.x * (int64_t)kT + threadIdx.x; e < units; e += (int64_t)gridDim.x * kT) {
        if (VEC) {
            float4 v = reinterpret_cast<float4*>(ga)[e];
            v.x = v.x == 0.f ? 0.f : v.x * sc; v.y = v.y == 0.f ? 0.f : v.y * sc;
            v.z = v.z == 0.f ? 0.f : v.z * sc; v.w = v.w == 0.f ? 0.f : v.w * sc;
            reinterpret_cast<float4*>(ga)[e] = v;
        } else {
            const float v = ga[e];
            ga[e] = v == 0.f ? 0.f : v * sc;
        }
    }
}

}  // namespace uamt
}  // namespace miseg

using namespace miseg;

extern "C" int miseg_noise_add(void* stream, const float* x, int64_t M, int64_t passes, const int32_t* seed, float sigma, float clip,
                               float* out) {
    MISEG_TAPE(miseg_noise_add, stream, x, M, passes, seed, sigma, clip, out);
    MISEG_REQUIRE(x && seed && out, "noise_add: null pointer");
    MISEG_REQUIRE(M > 0 && passes >= 1 && M <= (1LL << 40) && passes <= (1LL << 20), "noise_add: empty input / bad shape");
    MISEG_REQUIRE(out + passes * M <= x || x + M <= out, "noise_add: out overlaps x");
    const int64_t total = passes * M;
    const bool vec = M % 4 == 0 && aligned16(x) && aligned16(out);
    const dim3 grid((unsigned)std::min<int64_t>(cdiv(cdiv(total, 4), uamt::kT), 4096));
    if (vec) hipLaunchKernelGGL(uamt::noise_add_kernel<true>, grid, dim3(uamt::kT), 0, as_stream(stream), x, M, total, seed, sigma, clip, out);
    else hipLaunchKernelGGL(uamt::noise_add_kernel<false>, grid, dim3(uamt::kT), 0, as_stream(stream), x, M, total, seed, sigma, clip, out);
    MISEG_LAUNCH_CHECK("noise_add_kernel");
    return MISEG_OK;
}

extern "C" int miseg_softmax_accum(void* stream, const float* logits, int64_t N, int64_t H, int64_t W, int64_t C, int first, float* acc) {
    MISEG_TAPE(miseg_softmax_accum, stream, logits, N, H, W, C, first, acc);
    MISEG_REQUIRE(logits && acc, "softmax_accum: null pointer");
    MISEG_REQUIRE(class_count_has_kernel(C), "softmax_accum: unsupported class count %ld (2-6,8,10,16)", (long)C);
    MISEG_REQUIRE(N > 0 && H > 0 && W > 0 && N < (1LL << 31), "softmax_accum: empty batch / bad shape");
    const int64_t npix = N * H * W;
    const int nb = pixel_blocks(npix);
    const bool v4 = C % 4 == 0 && aligned16(logits) && aligned16(acc);
    hipStream_t st = as_stream(stream);
#define L(CC, VV) hipLaunchKernelGGL((uamt::softmax_accum_kernel<CC, VV>), dim3(nb), dim3(uamt::kT), 0, st, logits, npix, first, acc)
    MISEG_DISPATCH_C_V4(C, v4, L)
#undef L
    MISEG_LAUNCH_CHECK("softmax_accum_kernel");
    return MISEG_OK;
}

extern "C" int64_t miseg_softmax_umse_ws_bytes(int64_t N, int64_t H, int64_t W) {
    if (N <= 0 || H <= 0 || W <= 0) return 0;
    return (int64_t)pixel_blocks(N * H * W) * 16 + 16;
}

extern "C" int miseg_softmax_umse(void* stream, const float* a, const float* b, const float* acc, int64_t N, int64_t H, int64_t W, int64_t C,
                                  float inv_passes, const float* thr, const float* upstream, float* loss, float* ga, int64_t* kept,
                                  float* stats, void* ws, int64_t ws_bytes) {
    MISEG_TAPE(miseg_softmax_umse, stream, a, b, acc, N, H, W, C, inv_passes, thr, upstream, loss, ga, kept, stats, ws, ws_bytes);
    MISEG_REQUIRE(a && b && acc && thr && loss && ws, "softmax_umse: null pointer");
    MISEG_REQUIRE(class_count_has_kernel(C), "softmax_umse: unsupported class count %ld (2-6,8,10,16)", (long)C);
    MISEG_REQUIRE(N > 0 && H > 0 && W > 0 && N < (1LL << 31), "softmax_umse: empty batch / bad shape");
    const int64_t need = miseg_softmax_umse_ws_bytes(N, H, W);
    MISEG_REQUIRE(ws_bytes >= need && ((uintptr_t)ws & 7) == 0, "softmax_umse: workspace of %ld bytes (8-byte aligned), %ld needed", (long)ws_bytes,
                  (long)need);
    const int64_t npix = N * H * W;
    const int nb = pixel_blocks(npix);
    const bool v4 = C % 4 == 0 && aligned16(a) && aligned16(b) && aligned16(acc) && (!ga || aligned16(ga));
    hipStream_t st = as_stream(stream);
#define L(CC, VV) hipLaunchKernelGGL((uamt::umse_kernel<CC, VV>), dim3(nb), dim3(uamt::kT), 0, st, a, b, acc, npix, inv_passes, thr, ws, ga)
    MISEG_DISPATCH_C_V4(C, v4, L)
#undef L
    MISEG_LAUNCH_CHECK("umse_kernel");
    hipLaunchKernelGGL(uamt::umse_finish_kernel, dim3(1), dim3(256), 0, st, ws, nb, npix, (int)C, upstream, loss, (long long*)kept, stats);
    MISEG_LAUNCH_CHECK("umse_finish_kernel");
    if (ga) {
        const int64_t numel = npix * C;
        const bool vec = numel % 4 == 0 && aligned16(ga);
        const int64_t units = vec ? numel / 4 : numel;
        const dim3 grid((unsigned)std::min<int64_t>(cdiv(units, uamt::kT), 4096));
        const float* gscale = uamt::Workspace(ws, nb).gscale;
        if (vec) hipLaunchKernelGGL(uamt::umse_scale_kernel<true>, grid, dim3(uamt::kT), 0, st, ga, units, gscale);
        else hipLaunchKernelGGL(uamt::umse_scale_kernel<false>, grid, dim3(uamt::kT), 0, st, ga, units, gscale);
        MISEG_LAUNCH_CHECK("umse_scale_kernel");
    }
    return MISEG_OK;
}
