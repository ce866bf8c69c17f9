// Contrastive encoder pre-training (Trainer.name=contrast): the supervised-contrastive loss on the projector's raw embeddings, and
// the projection head's global average pool on the network's NHWC feature map.
// ref: contrastyou/losses/contrast_loss.py:21-100 (SupConLoss, contrast_mode='all'), contrastyou/epocher/contrast_epocher.py:90-95
// (F.normalize, chunk, stack), contrastyou/trainer/_utils.py:44-65 (ProjectionHead: AdaptiveAvgPool2d((1, 1)) first).
// Latency-only work (N = 32 rows of D = 256 at the bench shape): fp32, no matrix cores, no floating-point atomics, every sum in a
// fixed order.  The point is the launch count (the torch composition is ~60 ATen launches forward + backward) and determinism.
#include "common.h"

namespace miseg {

#ifndef MISEG_F16_BUILD
constexpr int kSupMaxN = 1024, kSupMaxD = 1024;

static inline bool supcon_shape_ok(int64_t N, int64_t D) {
    return N >= 2 && N <= kSupMaxN && D >= 4 && D <= kSupMaxD && D % 4 == 0;
}
// workspace: z [N][D] | G [N][N] | norm [N] | rowloss [N]   (floats; every section a multiple of 16 bytes from a 16-byte base)
static inline int64_t supcon_pad4(int64_t n) { return (n + 3) / 4 * 4; }
static inline int64_t supcon_ws_floats(int64_t N, int64_t D) { return N * D + supcon_pad4(N * N) + 2 * supcon_pad4(N); }

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// z_i = e_i / max(||e_i||, 1e-12): one wave per row, four rows per block
__global__ __launch_bounds__(256) void supcon_normalize_kernel(const float* __restrict__ e, int N, int D, float* __restrict__ z,
                                                               float* __restrict__ norm) {
    const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= N) return;                                  // whole waves leave together; no barrier below
    const float* row = e + (size_t)i * D;
    float s = 0.f;
    for (int d = lane; d < D; d += 64) s += row[d] * row[d];
    s = wave_sum(s);
    const float nrm = fmaxf(sqrtf(s), 1e-12f);
    for (int d = lane; d < D; d += 64) z[(size_t)i * D + d] = row[d] / nrm;
    if (lane == 0) norm[i] = nrm;
}

// Block i: s_ij for every j (one wave per j, lanes across D), the row's max, Z_i, |P_i|, the row's loss term and the row of G.
__global__ __launch_bounds__(256) void supcon_rows_kernel(const float* __restrict__ z, int N, int D, int B, const int32_t* __restrict__ labels,
                                                          float T, float coef, float* __restrict__ rowloss, float* __restrict__ G) {
    __shared__ float zi[kSupMaxD];
    __shared__ float s[kSupMaxN];
    __shared__ float red[17];
    const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    for (int d = tid; d < D; d += 256) zi[d] = z[(size_t)i * D + d];
    __syncthreads();
    const int d4 = D >> 2;
    for (int j = wid; j < N; j += 4) {
        const float4* zj = reinterpret_cast<const float4*>(z + (size_t)j * D);
        float a = 0.f;
        for (int q = lane; q < d4; q += 64) {
            const float4 v = zj[q];
            a += zi[4 * q] * v.x + zi[4 * q + 1] * v.y + zi[4 * q + 2] * v.z + zi[4 * q + 3] * v.w;
        }
        a = wave_sum(a);
        if (lane == 0) s[j] = a / T;
    }
    __syncthreads();
    float m = -INFINITY;
    for (int j = tid; j < N; j += 256) m = fmaxf(m, s[j]);
    m = -block_min(-m, red);                             // the diagonal takes part (contrast_loss.py:75)
    const int li = labels ? labels[i % B] : i % B;
    float zs = 0.f, cnt = 0.f;
    for (int j = tid; j < N; j += 256) {
        if (j == i) continue;
        zs += expf(s[j] - m);
        cnt += (labels ? labels[j % B] : j % B) == li ? 1.f : 0.f;
    }
    const float Z = block_sum(zs, red) + 1e-16f;
    cnt = block_sum(cnt, red);                           // >= V - 1 >= 1: the other views of the anchor's own sample
    const float logZ = logf(Z);
    float ps = 0.f;
    for (int j = tid; j < N; j += 256) {
        if (j == i) { if (G) G[(size_t)i * N + j] = 0.f; continue; }
        const bool pos = (labels ? labels[j % B] : j % B) == li;
        if (pos) ps += s[j] - m - logZ;
        if (G) G[(size_t)i * N + j] = coef * (expf(s[j] - m) / Z - (pos ? 1.f / cnt : 0.f));
    }
    ps = block_sum(ps, red);
    if (tid == 0) rowloss[i] = -ps / cnt;
}

// Block 0: loss = scale * (sum_i rowloss_i) / N.  With a gradient, block i also: gz_i = (1/T) sum_j (G_ij + G_ji) z_j, projected onto the
// tangent of the unit sphere at z_i and divided by the row's norm.  (A forward-only call launches ONE block with ge == nullptr.)
__global__ __launch_bounds__(256) void supcon_grad_kernel(const float* __restrict__ z, const float* __restrict__ norm, const float* __restrict__ G,
                                                          const float* __restrict__ rowloss, int N, int D, float T, float scale,
                                                          const float* __restrict__ upstream, float* __restrict__ loss, float* __restrict__ ge) {
    __shared__ float w[kSupMaxN];
    __shared__ float red[17];
    const int i = blockIdx.x, tid = threadIdx.x;
    if (i == 0) {
        float a = 0.f;
        for (int j = tid; j < N; j += 256) a += rowloss[j];
        a = block_sum(a, red);
        if (tid == 0) loss[0] = scale * (a / (float)N);
    }
    if (!ge) return;
    for (int j = tid; j < N; j += 256) w[j] = G[(size_t)i * N + j] + G[(size_t)j * N + i];
    __syncthreads();
    float gz[kSupMaxD / 256], dot = 0.f;
#pragma unroll
    for (int k = 0; k < kSupMaxD / 256; ++k) {
        const int d = tid + 256 * k;
        float a = 0.f;
        if (d < D)
            for (int j = 0; j < N; ++j) a += w[j] * z[(size_t)j * D + d];
        gz[k] = a / T;
        if (d < D) dot += z[(size_t)i * D + d] * gz[k];
    }
    dot = block_sum(dot, red);
    const float up = upstream ? upstream[0] : 1.f, nrm = norm[i];
#pragma unroll
    for (int k = 0; k < kSupMaxD / 256; ++k) {
        const int d = tid + 256 * k;
        if (d < D) ge[(size_t)i * D + d] = up * (gz[k] - z[(size_t)i * D + d] * dot) / nrm;
    }
}
#endif  // !MISEG_F16_BUILD

// ---------------------------------------------------------------- AdaptiveAvgPool2d((1, 1)) on an NHWC feature map
// pooled[n][c] = mean_{h,w} feat[n][h][w][c].  grid (N, ceil(C/32)): a block owns 32 channels of one sample; its 8 thread rows split the
// pixels (64/128-byte coalesced reads), four independent chains per thread, combined through LDS in a fixed order (the arrangement of
// the cluster head's pooling in mi_global.hip, which only exists inside miseg_head_global_fwd, behind a gather and in front of the
// Linear + softmax).
template <typename T>
__global__ __launch_bounds__(256) void avgpool_fwd_kernel(const T* __restrict__ feat, int HW, int C, float* __restrict__ pooled) {
    __shared__ float part[8][32];
    const int n = blockIdx.x, c = blockIdx.y * 32 + (threadIdx.x & 31), row = threadIdx.x >> 5;
    const T* f = feat + (size_t)n * HW * C;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    if (c < C) {
        int p = row;
        for (; p + 24 < HW; p += 32) {
            s0 += to_f32(f[(size_t)p * C + c]);
            s1 += to_f32(f[(size_t)(p + 8) * C + c]);
            s2 += to_f32(f[(size_t)(p + 16) * C + c]);
            s3 += to_f32(f[(size_t)(p + 24) * C + c]);
        }
        for (; p < HW; p += 8) s0 += to_f32(f[(size_t)p * C + c]);
    }
    part[row][threadIdx.x & 31] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    if (row == 0 && c < C) {
        float s = 0.f;
#pragma unroll
        for (int r = 0; r < 8; ++r) s += part[r][threadIdx.x];
        pooled[(size_t)n * C + c] = s / (float)HW;
    }
}

// gfeat[n][h][w][c] = T(g[n][c] / HW): grid (N, chunks), four channels per store (16 bytes of fp32, 8 of a 16-bit type; C % 4 == 0)
template <typename T>
__global__ __launch_bounds__(256) void avgpool_bwd_kernel(const float* __restrict__ g, int HW, int C, T* __restrict__ gfeat) {
    extern __shared__ float gp[];  // [C]
    const int n = blockIdx.x;
    for (int c = threadIdx.x; c < C; c += 256) gp[c] = g[(size_t)n * C + c] / (float)HW;
    __syncthreads();
    struct alignas(4 * sizeof(T)) Pack { T v[4]; };
    Pack* out = reinterpret_cast<Pack*>(gfeat + (size_t)n * HW * C);
    const int cv = C >> 2;
    const size_t nvec = (size_t)HW * cv;
    for (size_t e = (size_t)blockIdx.y * 256 + threadIdx.x; e < nvec; e += (size_t)gridDim.y * 256) {
        const int c0 = (int)(e % cv) * 4;
        Pack pk;
#pragma unroll
        for (int k = 0; k < 4; ++k) pk.v[k] = from_f32<T>(gp[c0 + k]);
        out[e] = pk;
    }
}

}  // namespace miseg

using namespace miseg;

#ifndef MISEG_F16_BUILD
extern "C" int64_t miseg_supcon_ws_bytes(int64_t N, int64_t D) {
    return supcon_shape_ok(N, D) ? supcon_ws_floats(N, D) * 4 : -1;
}

extern "C" int miseg_supcon(void* stream, const float* e, int64_t N, int64_t D, int64_t V, const int32_t* labels, float temperature,
                            float base_temperature, const float* upstream, float* loss, float* ge, void* ws, int64_t ws_bytes) {
    MISEG_TAPE(miseg_supcon, stream, e, N, D, V, labels, temperature, base_temperature, upstream, loss, ge, ws, ws_bytes);
    MISEG_REQUIRE(e && loss && ws, "supcon: null pointer");
    MISEG_REQUIRE(V >= 2 && N >= V && N % V == 0, "supcon: N = %lld rows are not V = %lld >= 2 views of a non-empty batch", (long long)N, (long long)V);
    MISEG_REQUIRE(supcon_shape_ok(N, D), "supcon: unsupported shape N = %lld, D = %lld (N <= 1024; D a multiple of 4, 4..1024)", (long long)N, (long long)D);
    MISEG_REQUIRE(temperature > 0.f && base_temperature > 0.f, "supcon: temperatures must be positive");
    MISEG_REQUIRE(ws_bytes >= supcon_ws_floats(N, D) * 4 && ((uintptr_t)ws & 15) == 0, "supcon: workspace too small or not 16-byte aligned");
    hipStream_t st = as_stream(stream);
    float* z = (float*)ws;
    float* G = z + N * D;
    float* norm = G + supcon_pad4(N * N);
    float* rowloss = norm + supcon_pad4(N);
    const int n = (int)N, d = (int)D, b = (int)(N / V);
    const float scale = temperature / base_temperature;
    hipLaunchKernelGGL(supcon_normalize_kernel, dim3((unsigned)cdiv(N, 4)), dim3(256), 0, st, e, n, d, z, norm);
    MISEG_LAUNCH_CHECK("supcon_normalize_kernel");
    hipLaunchKernelGGL(supcon_rows_kernel, dim3((unsigned)N), dim3(256), 0, st, z, n, d, b, labels, temperature, scale / (float)N, rowloss,
                       ge ? G : (float*)nullptr);
    MISEG_LAUNCH_CHECK("supcon_rows_kernel");
    hipLaunchKernelGGL(supcon_grad_kernel, dim3(ge ? (unsigned)N : 1u), dim3(256), 0, st, z, norm, G, rowloss, n, d, temperature, scale, upstream,
                       loss, ge);
    MISEG_LAUNCH_CHECK("supcon_grad_kernel");
    return MISEG_OK;
}
#endif  // !MISEG_F16_BUILD

#define AVGPOOL_CHECKS(what)                                                                                                  \
    MISEG_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0, what ": bad shape (C must be a multiple of 4)");             \
    MISEG_REQUIRE(H * W < (1ll << 31) / C && N < (1ll << 31) && cdiv(C, 32) < 65536, what ": a sample's H*W*C must stay below 2^31"); \
    MISEG_REQUIRE(dt == MISEG_F32 || dt == MISEG_BF16, what ": unknown dt")

extern "C" int miseg_avgpool_fwd(void* stream, int dt, const void* feat, int64_t N, int64_t H, int64_t W, int64_t C, float* pooled) {
    MISEG_TAPE(miseg_avgpool_fwd, stream, dt, feat, N, H, W, C, pooled);
    MISEG_F16_DISPATCH_ON(dt, miseg_avgpool_fwd, stream, MISEG_BF16, feat, N, H, W, C, pooled);
    MISEG_REQUIRE(feat && pooled, "avgpool_fwd: null pointer");
    AVGPOOL_CHECKS("avgpool_fwd");
    hipStream_t st = as_stream(stream);
    const dim3 grid((unsigned)N, (unsigned)cdiv(C, 32));
#ifndef MISEG_F16_BUILD      // dt == MISEG_F32 never reaches the fp16 build (conv.h)
    if (dt == MISEG_F32)
        hipLaunchKernelGGL(avgpool_fwd_kernel<float>, grid, dim3(256), 0, st, (const float*)feat, (int)(H * W), (int)C, pooled);
    else
#endif
        hipLaunchKernelGGL(avgpool_fwd_kernel<bf16>, grid, dim3(256), 0, st, (const bf16*)feat, (int)(H * W), (int)C, pooled);
    MISEG_LAUNCH_CHECK("avgpool_fwd_kernel");
    return MISEG_OK;
}

extern "C" int miseg_avgpool_bwd(void* stream, int dt, const float* g, int64_t N, int64_t H, int64_t W, int64_t C, void* gfeat) {
    MISEG_TAPE(miseg_avgpool_bwd, stream, dt, g, N, H, W, C, gfeat);
    MISEG_F16_DISPATCH_ON(dt, miseg_avgpool_bwd, stream, MISEG_BF16, g, N, H, W, C, gfeat);
    MISEG_REQUIRE(g && gfeat, "avgpool_bwd: null pointer");
    AVGPOOL_CHECKS("avgpool_bwd");
    MISEG_REQUIRE(C * 4 <= 64 * 1024, "avgpool_bwd: C too large for the LDS copy of the pooled gradient");
    MISEG_REQUIRE(((uintptr_t)gfeat & 15) == 0, "avgpool_bwd: gfeat must be 16-byte aligned");
    hipStream_t st = as_stream(stream);
    const unsigned chunks = (unsigned)std::min<int64_t>(std::max<int64_t>(cdiv(H * W * (C / 4), 256 * 4), 1), 64);
    const dim3 grid((unsigned)N, chunks);
#ifndef MISEG_F16_BUILD      // dt == MISEG_F32 never reaches the fp16 build (conv.h)
    if (dt == MISEG_F32)
        hipLaunchKernelGGL(avgpool_bwd_kernel<float>, grid, dim3(256), (size_t)C * 4, st, g, (int)(H * W), (int)C, (float*)gfeat);
    else
#endif
        hipLaunchKernelGGL(avgpool_bwd_kernel<bf16>, grid, dim3(256), (size_t)C * 4, st, g, (int)(H * W), (int)C, (bf16*)gfeat);
    MISEG_LAUNCH_CHECK("avgpool_bwd_kernel");
    return MISEG_OK;
}
