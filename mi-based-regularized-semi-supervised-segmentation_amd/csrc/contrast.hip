// Contrastive encoder pre-training (Trainer.name=contrast): the projection head's global average pool on the network's NHWC
// feature map, typed by the storage type.  The supervised-contrastive loss behind it is in supcon.hip (fp32 only, built once).
// ref: contrastyou/trainer/_utils.py:44-65 (ProjectionHead: AdaptiveAvgPool2d((1, 1)) first).
#include "common.h"

namespace miseg {

// ---------------------------------------------------------------- AdaptiveAvgPool2d((1, 1)) on an NHWC feature map
// pooled[n][c] = mean_{h,w} feat[n][h][w][c].  grid (N, ceil(C/32)): a block owns 32 channels of one sample; its 8 thread rows split the
// pixels (64/128-byte coalesced reads), four independent chains per thread, combined through LDS in a fixed order (the arrangement of
// the cluster head's pooling in heads_global.hip, which only exists inside miseg_head_global_fwd, behind a gather and in front of the
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
    MISEG_WITH_STORAGE_TYPE(dt, "avgpool_fwd", hipLaunchKernelGGL(avgpool_fwd_kernel<TT>, grid, dim3(256), 0, st, (const TT*)feat, (int)(H * W), (int)C, pooled));
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
    MISEG_WITH_STORAGE_TYPE(dt, "avgpool_bwd", hipLaunchKernelGGL(avgpool_bwd_kernel<TT>, grid, dim3(256), (size_t)C * 4, st, g, (int)(H * W), (int)C, (TT*)gfeat));
    MISEG_LAUNCH_CHECK("avgpool_bwd_kernel");
    return MISEG_OK;
}
