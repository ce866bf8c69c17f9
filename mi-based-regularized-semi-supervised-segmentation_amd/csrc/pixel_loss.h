// What the pixel-streaming loss units share (losses.hip, dice.hip, ict.hip, uamt.hip; mi_out.hip takes the softmax alone): one pixel
// per thread with the channel vector in registers, blocks of 256 pixels, per-block partials and one finishing block.  Everything here
// is inline, a template or a macro, so each unit compiles it under its own flags (uamt.hip without contraction) and no kernel is
// emitted twice: finish_sum_kernel and its launcher are defined in losses.hip.  DESIGN.md section 29.
#pragma once
#include "common.h"

namespace miseg {

__device__ __forceinline__ void softmax_c(const float* __restrict__ z, int C, float* p) {
    float mx = -3.4e38f;
    for (int c = 0; c < C; ++c) mx = fmaxf(mx, z[c]);
    float s = 0.f;
    for (int c = 0; c < C; ++c) { p[c] = expf(z[c] - mx); s += p[c]; }
    for (int c = 0; c < C; ++c) p[c] = p[c] / s;
}

// One row of C floats; V4: as 16-byte vectors (C a multiple of 4, the row 16-byte aligned).
template <int C, bool V4>
__device__ __forceinline__ void load_row(const float* __restrict__ p, float* z) {
    if (V4) {
#pragma unroll
        for (int c = 0; c < C; c += 4) {
            const float4 v = *reinterpret_cast<const float4*>(p + c);
            z[c] = v.x; z[c + 1] = v.y; z[c + 2] = v.z; z[c + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int c = 0; c < C; ++c) z[c] = p[c];
    }
}

template <int C, bool V4>
__device__ __forceinline__ void store_row(float* __restrict__ p, const float* z) {
    if (V4) {
#pragma unroll
        for (int c = 0; c < C; c += 4) *reinterpret_cast<float4*>(p + c) = make_float4(z[c], z[c + 1], z[c + 2], z[c + 3]);
    } else {
#pragma unroll
        for (int c = 0; c < C; ++c) p[c] = z[c];
    }
}

// exact integer block sum (fixed order over the waves): the counts of uamt.hip and cps.hip
__device__ __forceinline__ long long block_sum_i64(long long v, long long* red /* >= 17 words of LDS */) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if (lane == 0) red[wid] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long t = 0;
        for (int i = 0; i < nw; ++i) t += red[i];
        red[16] = t;
    }
    __syncthreads();
    return red[16];
}

constexpr int kPixelThreads = 256;     // the block size of every pixel kernel (kLT, kDT, kT of the units)
static inline int pixel_blocks(int64_t npix) { return (int)std::min<int64_t>(cdiv(npix, kPixelThreads), 2048); }
static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static inline bool class_count_has_kernel(int64_t C) { return (C >= 2 && C <= 6) || C == 8 || C == 10 || C == 16; }

// out[0] = scale * sum of partials[0 .. n), by one block in a fixed order (losses.hip)
int launch_finish_sum(hipStream_t st, const float* partials, int n, float scale, float* out);

// The class counts that have a kernel, as a statement of a function that returns a status: MISEG_DISPATCH_C(C, MACRO, more...) runs
// MACRO(C as a literal, more...); MISEG_DISPATCH_C_V4(C, v4, MACRO) runs MACRO(C, V4) with V4 = v4 where C is a multiple of 4 and
// false elsewhere, so a vector form exists for 4, 8 and 16 only.  Any other C returns MISEG_E_INVALID.
#define MISEG_DISPATCH_C_ARMS(C, ODD, QUAD, ...)                                                     \
    switch (C) {                                                                                     \
        case 2: ODD(2, __VA_ARGS__); break;                                                          \
        case 3: ODD(3, __VA_ARGS__); break;                                                          \
        case 4: QUAD(4, __VA_ARGS__); break;                                                         \
        case 5: ODD(5, __VA_ARGS__); break;                                                          \
        case 6: ODD(6, __VA_ARGS__); break;                                                          \
        case 8: QUAD(8, __VA_ARGS__); break;                                                         \
        case 10: ODD(10, __VA_ARGS__); break;                                                        \
        case 16: QUAD(16, __VA_ARGS__); break;                                                       \
        default: return fail(MISEG_E_INVALID, "unsupported class count %ld (2-6,8,10,16)", (long)C);  \
    }
#define MISEG_ARM_PLAIN(CC, MACRO, ...) MACRO(CC, ##__VA_ARGS__)
#define MISEG_ARM_SCALAR(CC, MACRO, v4) MACRO(CC, false)
#define MISEG_ARM_EITHER(CC, MACRO, v4) if (v4) MACRO(CC, true); else MACRO(CC, false)
#define MISEG_DISPATCH_C(C, ...) MISEG_DISPATCH_C_ARMS(C, MISEG_ARM_PLAIN, MISEG_ARM_PLAIN, __VA_ARGS__)
#define MISEG_DISPATCH_C_V4(C, v4, MACRO) MISEG_DISPATCH_C_ARMS(C, MISEG_ARM_SCALAR, MISEG_ARM_EITHER, MACRO, v4)

}  // namespace miseg
