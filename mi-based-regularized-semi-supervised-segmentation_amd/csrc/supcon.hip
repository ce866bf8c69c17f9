// Contrastive encoder pre-training (Trainer.name=contrast): the supervised-contrastive loss on the projector's raw embeddings.
// ref: contrastyou/losses/contrast_loss.py:21-100 (SupConLoss, contrast_mode='all'), contrastyou/epocher/contrast_epocher.py:90-95
// (F.normalize, chunk, stack).
// Latency-only work (N = 32 rows of D = 256 at the bench shape): fp32, no matrix cores, no floating-point atomics, every sum in a
// fixed order.  The point is the launch count (the torch composition is ~60 ATen launches forward + backward) and determinism.
// No storage type: built once.
#include "common.h"

namespace miseg {

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

}  // namespace miseg

using namespace miseg;

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
