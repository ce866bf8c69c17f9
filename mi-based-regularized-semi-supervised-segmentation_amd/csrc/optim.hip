// Fused Adam, RAdam, AdaBound / AdaBoundW and the gradient check that guards them: fp32 parameters, no storage type -- built once.
// ref: semi_seg/trainer.py:67-72,179-184 (torch.optim.Adam with L2 weight decay; the other names: whl:deepclustering2/optim).
#include "common.h"

namespace miseg {

__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, int64_t n, float b1, float b2, const float* __restrict__ hyper,
                                                   float inv_scale, const float* __restrict__ guard, int nguard) {
    // guard: the iteration's deferred-check flags (non-zero or NaN = a check failed).  A failed check leaves parameters and moments
    // untouched, so the exception the host raises one iteration later finds the state the reference -- which raises before
    // backward (iic_loss.py:147-148) -- would have left.
    for (int i = 0; i < nguard; ++i)
        if (!(guard[i] == 0.f)) return;
    const float step_size = hyper[0], inv_sqrt_bc2 = hyper[1], eps = hyper[2], wd = hyper[3];
    if (inv_scale < 0.f) inv_scale = hyper[4];       // the loss scale lives on the device (dynamic scale under a replayed launch tape)
    for (int64_t i = blockIdx.x * 256LL + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        float gi = g[i] * inv_scale + wd * p[i];
        float mi = m[i] * b1 + (1.f - b1) * gi;
        float vi = v[i] * b2 + (1.f - b2) * gi * gi;
        m[i] = mi; v[i] = vi;
        const float denom = sqrtf(vi) * inv_sqrt_bc2 + eps;
        p[i] = p[i] - step_size * (mi / denom);
    }
}

}  // namespace miseg

using namespace miseg;

extern "C" int miseg_adam_step_guarded(void* stream, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t numel,
                                       float beta1, float beta2, const float* hyper, float grad_scale, const float* guard, int64_t nguard) {
    MISEG_TAPE(miseg_adam_step_guarded, stream, param, grad, exp_avg, exp_avg_sq, numel, beta1, beta2, hyper, grad_scale, guard, nguard);
    MISEG_REQUIRE(param && grad && exp_avg && exp_avg_sq && hyper && numel > 0, "adam_step: bad args");
    MISEG_REQUIRE((grad_scale > 0.f || grad_scale == -1.f) && std::isfinite(grad_scale), "adam_step: grad_scale must be a positive finite number (or -1: read 1 / scale from hyper[4])");
    MISEG_REQUIRE(nguard >= 0 && nguard <= 1024 && (nguard == 0 || guard), "adam_step: bad guard");
    hipLaunchKernelGGL(adam_kernel, dim3(ew_blocks(numel)), dim3(256), 0, as_stream(stream), param, grad, exp_avg, exp_avg_sq, numel, beta1, beta2,
                       hyper, grad_scale > 0.f ? 1.f / grad_scale : -1.f, guard, (int)nguard);
    MISEG_LAUNCH_CHECK("adam_kernel");
    return MISEG_OK;
}
// RAdam and AdaBound / AdaBoundW as the wheel states them (whl:deepclustering2/optim/radam.py:16-91, adabound.py:67-136,199-270), on
// the same flat fp32 buffers and behind the same guard flags as Adam.  What changes from step to step -- the step size, RAdam's
// rectified flag, AdaBound's clamp bounds, weight decay x lr -- is computed on the host in double and read from the `hyper` row in
// device memory: a replayed launch tape replays by-value arguments, and RAdam turns rectified at its sixth step.  By value: the
// betas and 1 - beta (rounded from double, as torch rounds the scalar of `add_(1 - beta1, grad)`), which no step changes.
namespace miseg {

__global__ __launch_bounds__(256) void radam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                    float* __restrict__ v, int64_t n, float b1, float b2, float omb1, float omb2,
                                                    const float* __restrict__ hyper, float inv_scale, const float* __restrict__ guard, int nguard) {
    for (int i = 0; i < nguard; ++i)
        if (!(guard[i] == 0.f)) return;
    // hyper: step size (lr x rectification / bias correction 1), rectified (N_sma >= 5) as 1 / 0, eps, weight decay x lr, 1 / loss scale
    const float step_size = hyper[0], eps = hyper[2], wdlr = hyper[3];
    const bool rectified = hyper[1] != 0.f;
    if (inv_scale < 0.f) inv_scale = hyper[4];
    for (int64_t i = blockIdx.x * 256LL + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float gi = g[i] * inv_scale;                       // no L2 term: the decay is decoupled
        const float vi = v[i] * b2 + omb2 * gi * gi;
        const float mi = m[i] * b1 + omb1 * gi;
        m[i] = mi; v[i] = vi;
        float pi = p[i];
        if (wdlr != 0.f) pi = pi + (-wdlr) * pi;
        if (rectified) pi = pi + (-step_size * mi) / (sqrtf(vi) + eps);
        else pi = pi + (-step_size) * mi;
        p[i] = pi;
    }
}

// AMS: keep the running maximum of v and normalise by it (amsbound); W: decoupled decay (AdaBoundW) instead of the L2 term.
template <bool AMS, bool W>
__global__ __launch_bounds__(256) void adabound_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                       float* __restrict__ v, float* __restrict__ vmax, int64_t n, float b1, float b2,
                                                       float omb1, float omb2, const float* __restrict__ hyper, float inv_scale,
                                                       const float* __restrict__ guard, int nguard) {
    for (int i = 0; i < nguard; ++i)
        if (!(guard[i] == 0.f)) return;
    // hyper: step size (lr x sqrt(bias correction 2) / bias correction 1), lower bound, eps, weight decay, 1 / loss scale, upper bound
    const float step_size = hyper[0], lower = hyper[1], eps = hyper[2], wd = hyper[3], upper = hyper[5];
    if (inv_scale < 0.f) inv_scale = hyper[4];
    for (int64_t i = blockIdx.x * 256LL + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float p0 = p[i];
        float gi = g[i] * inv_scale;
        if (!W && wd != 0.f) gi = gi + wd * p0;
        const float mi = m[i] * b1 + omb1 * gi;
        float vi = v[i] * b2 + omb2 * gi * gi;
        m[i] = mi; v[i] = vi;
        if (AMS) {
            vi = fmaxf(vmax[i], vi);
            vmax[i] = vi;
        }
        const float rate = fminf(fmaxf(step_size / (sqrtf(vi) + eps), lower), upper);
        float pi = p0 - rate * mi;
        if (W && wd != 0.f) pi = pi - p0 * wd;          // the decayed weights are taken from p before the step
        p[i] = pi;
    }
}

}  // namespace miseg

static int check_step_args(const char* who, const void* param, const void* grad, const void* exp_avg, const void* exp_avg_sq, int64_t numel,
                           double beta1, double beta2, const void* hyper, float grad_scale, const void* guard, int64_t nguard) {
    MISEG_REQUIRE(param && grad && exp_avg && exp_avg_sq && hyper && numel > 0, "%s: bad args", who);
    MISEG_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "%s: betas must lie in [0, 1)", who);
    MISEG_REQUIRE((grad_scale > 0.f || grad_scale == -1.f) && std::isfinite(grad_scale), "%s: grad_scale must be a positive finite number (or -1: read 1 / scale from hyper[4])", who);
    MISEG_REQUIRE(nguard >= 0 && nguard <= 1024 && (nguard == 0 || guard), "%s: bad guard", who);
    return MISEG_OK;
}

extern "C" int miseg_radam_step(void* stream, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t numel,
                                double beta1, double beta2, const float* hyper, float grad_scale, const float* guard, int64_t nguard) {
    MISEG_TAPE(miseg_radam_step, stream, param, grad, exp_avg, exp_avg_sq, numel, beta1, beta2, hyper, grad_scale, guard, nguard);
    if (int rc = check_step_args("radam_step", param, grad, exp_avg, exp_avg_sq, numel, beta1, beta2, hyper, grad_scale, guard, nguard)) return rc;
    hipLaunchKernelGGL(radam_kernel, dim3(ew_blocks(numel)), dim3(256), 0, as_stream(stream), param, grad, exp_avg, exp_avg_sq, numel, (float)beta1,
                       (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), hyper, grad_scale > 0.f ? 1.f / grad_scale : -1.f, guard, (int)nguard);
    MISEG_LAUNCH_CHECK("radam_kernel");
    return MISEG_OK;
}

extern "C" int miseg_adabound_step(void* stream, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* max_exp_avg_sq,
                                   int64_t numel, double beta1, double beta2, const float* hyper, int decoupled, float grad_scale,
                                   const float* guard, int64_t nguard) {
    MISEG_TAPE(miseg_adabound_step, stream, param, grad, exp_avg, exp_avg_sq, max_exp_avg_sq, numel, beta1, beta2, hyper, decoupled, grad_scale, guard, nguard);
    if (int rc = check_step_args("adabound_step", param, grad, exp_avg, exp_avg_sq, numel, beta1, beta2, hyper, grad_scale, guard, nguard)) return rc;
    MISEG_REQUIRE(decoupled == 0 || decoupled == 1, "adabound_step: decoupled must be 0 (AdaBound) or 1 (AdaBoundW)");
    auto kernel = max_exp_avg_sq ? (decoupled ? adabound_kernel<true, true> : adabound_kernel<true, false>)
                                 : (decoupled ? adabound_kernel<false, true> : adabound_kernel<false, false>);
    hipLaunchKernelGGL(kernel, dim3(ew_blocks(numel)), dim3(256), 0, as_stream(stream), param, grad, exp_avg, exp_avg_sq, max_exp_avg_sq, numel,
                       (float)beta1, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), hyper, grad_scale > 0.f ? 1.f / grad_scale : -1.f,
                       guard, (int)nguard);
    MISEG_LAUNCH_CHECK("adabound_kernel");
    return MISEG_OK;
}

namespace miseg {
__global__ __launch_bounds__(256) void count_nonfinite_kernel(const float* __restrict__ g, int64_t n, float* __restrict__ count) {
    int bad = 0;
    for (int64_t i = blockIdx.x * 256LL + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) bad += !(fabsf(g[i]) <= 3.4028234e38f);   // inf or NaN
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bad += __shfl_xor(bad, o, 64);
    if ((threadIdx.x & 63) == 0 && bad) atomicAdd(count, (float)bad);       // integers below 2^24: exact in any order
}
}  // namespace miseg

extern "C" int miseg_count_nonfinite(void* stream, const float* grad, int64_t numel, float* count) {
    MISEG_TAPE(miseg_count_nonfinite, stream, grad, numel, count);
    MISEG_REQUIRE(grad && count && numel > 0, "count_nonfinite: bad args");
    hipMemsetAsync(count, 0, sizeof(float), as_stream(stream));
    hipLaunchKernelGGL(count_nonfinite_kernel, dim3((unsigned)std::min<int64_t>(cdiv(numel, 1024), 1024)), dim3(256), 0, as_stream(stream), grad, numel, count);
    MISEG_LAUNCH_CHECK("count_nonfinite_kernel");
    return MISEG_OK;
}

extern "C" int miseg_adam_step_scaled(void* stream, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t numel,
                                      float beta1, float beta2, const float* hyper, float grad_scale) {
    MISEG_TAPE(miseg_adam_step_scaled, stream, param, grad, exp_avg, exp_avg_sq, numel, beta1, beta2, hyper, grad_scale);
    return miseg_adam_step_guarded(stream, param, grad, exp_avg, exp_avg_sq, numel, beta1, beta2, hyper, grad_scale, nullptr, 0);
}
extern "C" int miseg_adam_step(void* stream, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t numel,
                               float beta1, float beta2, const float* hyper) {
    MISEG_TAPE(miseg_adam_step, stream, param, grad, exp_avg, exp_avg_sq, numel, beta1, beta2, hyper);
    return miseg_adam_step_scaled(stream, param, grad, exp_avg, exp_avg_sq, numel, beta1, beta2, hyper, 1.f);
}
