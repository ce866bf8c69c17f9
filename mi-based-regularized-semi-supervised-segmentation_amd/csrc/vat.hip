// Virtual adversarial training (Trainer.name=vat): the per-sample L2 normalisation + perturbation and the counter-based normal
// generator.  fp32 tensors, no storage type -- built once.  ref: whl:deepclustering2/utils/VAT.py (_l2_normalize, VATLoss.forward).
#include "common.h"
#include "philox.h"      // Philox4x32-10 + Box-Muller, shared with uamt.hip

namespace miseg {

// ---- per-sample L2 norm, pass 1: block (b, n) sums the squares of its chunk of sample n in double, in a fixed order
constexpr int kL2Chunk = 4096;        // elements per block of pass 1 (at most kL2MaxParts blocks per sample: longer samples, longer chunks)
constexpr int kL2MaxParts = 64;

__device__ __forceinline__ double block_sum_f64(double v, double* red /* >= 5 doubles of LDS */) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if (lane == 0) red[wid] = v;
    __syncthreads();
    if (threadIdx.x == 0) red[4] = ((red[0] + red[1]) + red[2]) + red[3];
    __syncthreads();
    return red[4];
}

__global__ __launch_bounds__(256) void l2_sumsq_kernel(const float* __restrict__ g, int M, int chunk, double* __restrict__ parts) {
    __shared__ double red[5];
    const int n = blockIdx.y, b = blockIdx.x, lo = b * chunk, hi = min(M, lo + chunk);
    const float* gp = g + (size_t)n * M;
    double s = 0.0;
    for (int i = lo + (int)threadIdx.x; i < hi; i += 256) {
        const double v = (double)gp[i];
        s += v * v;
    }
    s = block_sum_f64(s, red);
    if (threadIdx.x == 0) parts[(size_t)n * gridDim.x + b] = s;
}

// ---- pass 2: every block adds the sample's partial sums in order (the same value in every block), then d = g / s, r = scale * d, out = x + r
__global__ __launch_bounds__(256) void l2_apply_kernel(const float* __restrict__ g, const float* __restrict__ x, const float* __restrict__ scale,
                                                       int M, int nparts, const double* __restrict__ parts, float* __restrict__ out,
                                                       float* __restrict__ r, float* __restrict__ d, int* __restrict__ flag) {
    __shared__ float s_norm;
    const int n = blockIdx.y;
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int q = 0; q < nparts; ++q) t += parts[(size_t)n * nparts + q];
        const float s = (float)sqrt(t);
        const bool ok = s > 0.f && s <= 3.4028234e38f;             // (NaN fails both)
        if (!ok && blockIdx.x == 0) atomicAdd(flag, 1);
        s_norm = ok ? s : 0.f;
    }
    __syncthreads();
    const float s = s_norm, sc = scale[n];
    const size_t base = (size_t)n * M;
    for (int i = blockIdx.x * 256 + (int)threadIdx.x; i < M; i += (int)gridDim.x * 256) {
        const float dv = s > 0.f ? g[base + i] / s : 0.f;
        const float rv = sc * dv;
        if (d) d[base + i] = dv;
        if (r) r[base + i] = rv;
        if (out) out[base + i] = x[base + i] + rv;
    }
}

// one thread = one counter block = elements [4 b, 4 b + 4) of the stream, of which [offset, offset + numel) are written
template <bool NORMAL>
__global__ __launch_bounds__(256) void philox_fill_kernel(unsigned long long seed, unsigned long long offset, unsigned long long numel,
                                                          void* __restrict__ out) {
    const unsigned long long first = offset >> 2, nblk = ((offset + numel + 3) >> 2) - first;
    for (unsigned long long t = blockIdx.x * 256ull + threadIdx.x; t < nblk; t += (unsigned long long)gridDim.x * 256ull) {
        const unsigned long long b = first + t;
        const Philox4 p = philox_block(seed, b);
        float z[4];
        if (NORMAL) philox_normals(p, z);
#pragma unroll
        for (int l = 0; l < 4; ++l) {
            const unsigned long long j = 4ull * b + l;
            if (j < offset || j >= offset + numel) continue;
            if (NORMAL) static_cast<float*>(out)[j - offset] = z[l];
            else static_cast<unsigned*>(out)[j - offset] = p.v[l];
        }
    }
}

}  // namespace miseg

using namespace miseg;

static int l2_parts(int64_t M) { return (int)std::min<int64_t>(cdiv(M, kL2Chunk), kL2MaxParts); }

extern "C" int64_t miseg_l2_perturb_ws_bytes(int64_t N, int64_t M) {
    if (N <= 0 || M <= 0) return 0;
    return N * l2_parts(M) * (int64_t)sizeof(double);
}

extern "C" int miseg_l2_perturb(void* stream, const float* g, const float* x, const float* scale, int64_t N, int64_t M, float* out, float* r,
                                float* d, int32_t* flag, void* ws, int64_t ws_bytes) {
    MISEG_TAPE(miseg_l2_perturb, stream, g, x, scale, N, M, out, r, d, flag, ws, ws_bytes);
    MISEG_REQUIRE(g && scale && flag && ws && N > 0 && N <= 65535 && M > 0 && M <= (1LL << 30), "l2_perturb: bad args");      // (int indices: chunk and grid strides stay below 2^31)
    MISEG_REQUIRE(out || r || d, "l2_perturb: no output");
    MISEG_REQUIRE(!out || x, "l2_perturb: out needs x");
    MISEG_REQUIRE(((uintptr_t)ws & 7) == 0 && ws_bytes >= miseg_l2_perturb_ws_bytes(N, M), "l2_perturb: workspace too small or misaligned");
    const int nparts = l2_parts(M), chunk = (int)cdiv(M, nparts);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(l2_sumsq_kernel, dim3((unsigned)nparts, (unsigned)N), dim3(256), 0, st, g, (int)M, chunk, static_cast<double*>(ws));
    MISEG_LAUNCH_CHECK("l2_sumsq_kernel");
    const unsigned nb = (unsigned)std::min<int64_t>(cdiv(M, 1024), 256);
    hipLaunchKernelGGL(l2_apply_kernel, dim3(nb, (unsigned)N), dim3(256), 0, st, g, x, scale, (int)M, nparts, static_cast<const double*>(ws), out, r, d,
                       flag);
    MISEG_LAUNCH_CHECK("l2_apply_kernel");
    return MISEG_OK;
}

static int philox_launch(bool normal, void* stream, int64_t seed, int64_t offset, void* out, int64_t numel, const char* who) {
    if (!(out && numel > 0 && offset >= 0 && offset <= (1LL << 62) && numel <= (1LL << 40))) return fail(MISEG_E_INVALID, "%s: bad args", who);
    const int64_t nblk = ((offset + numel + 3) >> 2) - (offset >> 2);
    const unsigned nb = (unsigned)std::min<int64_t>(cdiv(nblk, 256), 4096);
    if (normal)
        hipLaunchKernelGGL(philox_fill_kernel<true>, dim3(nb), dim3(256), 0, as_stream(stream), (unsigned long long)seed, (unsigned long long)offset,
                           (unsigned long long)numel, out);
    else
        hipLaunchKernelGGL(philox_fill_kernel<false>, dim3(nb), dim3(256), 0, as_stream(stream), (unsigned long long)seed, (unsigned long long)offset,
                           (unsigned long long)numel, out);
    MISEG_LAUNCH_CHECK("philox_fill_kernel");
    return MISEG_OK;
}

extern "C" int miseg_normal_fill(void* stream, int64_t seed, int64_t offset, float* out, int64_t numel) {
    MISEG_TAPE(miseg_normal_fill, stream, seed, offset, out, numel);
    return philox_launch(true, stream, seed, offset, out, numel, "normal_fill");
}

extern "C" int miseg_philox_fill(void* stream, int64_t seed, int64_t offset, int32_t* out, int64_t numel) {
    MISEG_TAPE(miseg_philox_fill, stream, seed, offset, out, numel);
    return philox_launch(false, stream, seed, offset, out, numel, "philox_fill");
}
