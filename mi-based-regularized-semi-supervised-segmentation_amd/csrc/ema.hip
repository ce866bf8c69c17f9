// Mean Teacher: the teacher's exponential moving average of the student, on flat fp32 buffers.
// ref: whl:deepclustering2/models/ema.py:107-131 (ema_updater.__call__), per parameter tensor:
//      t.mul_(alpha).add_(s, alpha=1 - alpha); t.mul_(1 - weight_decay)
// The teacher's parameters live in one flat buffer laid out exactly as the student's (miseg_amd/flat.py, MirrorBuffers), so the
// whole update is ONE grid-stride launch: 12 bytes of HBM traffic per parameter (read t, read s, write t), memory-bound.
//
// Rounding: each step rounds as torch's eager kernels do on this device, so the result is bit-equal to the reference's loop run on
// the GPU.  mul_ by a Python scalar is one fp32 multiply; add_(s, alpha=b) is torch's AddFunctor `a + alpha * b`, which the ROCm
// build of torch contracts into ONE fused multiply-add (bit-equal to torch on the device: tests/test_gpu_meanteacher.py);
// the final mul_ is one more multiply.  The intrinsics below pin those roundings whatever -ffp-contract says.
#include "common.h"

namespace miseg {

__device__ __forceinline__ float ema_one(float t, float s, float a, float b, float d) {
    return __fmul_rn(__fmaf_rn(b, s, __fmul_rn(t, a)), d);
}

__global__ __launch_bounds__(256) void ema_kernel(float* __restrict__ t, const float* __restrict__ s, int64_t n,
                                                  const float* __restrict__ coef, const float* __restrict__ guard, int nguard) {
    // guard: the iteration's deferred-check / overflow flags, as the fused Adam reads them -- a skipped update moves no teacher either
    for (int i = 0; i < nguard; ++i)
        if (!(guard[i] == 0.f)) return;
    const float a = coef[0], b = coef[1], d = coef[2];       // alpha, 1 - alpha, 1 - weight_decay (the step block's EMA row)
    const int64_t n4 = n >> 2;
    float4* __restrict__ t4 = reinterpret_cast<float4*>(t);
    const float4* __restrict__ s4 = reinterpret_cast<const float4*>(s);
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = blockIdx.x * 256LL + threadIdx.x; i < n4; i += stride) {
        float4 x = t4[i];
        const float4 y = s4[i];
        x.x = ema_one(x.x, y.x, a, b, d);
        x.y = ema_one(x.y, y.y, a, b, d);
        x.z = ema_one(x.z, y.z, a, b, d);
        x.w = ema_one(x.w, y.w, a, b, d);
        t4[i] = x;
    }
    for (int64_t i = (n4 << 2) + blockIdx.x * 256LL + threadIdx.x; i < n; i += stride) t[i] = ema_one(t[i], s[i], a, b, d);
}

}  // namespace miseg

using namespace miseg;

extern "C" int miseg_ema_update(void* stream, float* teacher, const float* student, int64_t numel, const float* coef,
                                const float* guard, int64_t nguard) {
    MISEG_TAPE(miseg_ema_update, stream, teacher, student, numel, coef, guard, nguard);
    MISEG_REQUIRE(teacher && student && coef && numel > 0, "ema_update: bad args");
    MISEG_REQUIRE(((uintptr_t)teacher & 15) == 0 && ((uintptr_t)student & 15) == 0, "ema_update: buffers must be 16-byte aligned");
    MISEG_REQUIRE(nguard >= 0 && nguard <= 1024 && (nguard == 0 || guard), "ema_update: bad guard");
    hipLaunchKernelGGL(ema_kernel, dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>(cdiv(cdiv(numel, 4), 256), 8192))), dim3(256), 0, as_stream(stream), teacher, student, numel, coef, guard,
                       (int)nguard);
    MISEG_LAUNCH_CHECK("ema_kernel");
    return MISEG_OK;
}
