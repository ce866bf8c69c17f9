// BatchNorm2d statistics -> coefficients: the per-block sums of a producing convolution (training) or the running statistics
// (eval) become saved = [mean | invstd | scale | shift], which bn.hip's apply kernels read.  No storage type: built once.
// ref: contrastyou/arch/unet.py:16-17,19-20,34-35.
#include "common.h"

namespace miseg {

// ---- statistics -> coefficients.  saved = [mean | invstd | scale | shift] (4*C floats)
__global__ __launch_bounds__(256) void bn_finalize_kernel(const float* __restrict__ parts, int nparts, int C, float count,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                          float momentum, float* __restrict__ rmean, float* __restrict__ rvar,
                                                          long long* __restrict__ nbt, float* __restrict__ saved) {
    __shared__ float red[17];
    const int c = blockIdx.x;
    float s1 = 0.f, s2 = 0.f;
    for (int q = threadIdx.x; q < nparts; q += 256) {
        s1 += parts[((size_t)q * 2 + 0) * C + c];
        s2 += parts[((size_t)q * 2 + 1) * C + c];
    }
    s1 = block_sum(s1, red);
    s2 = block_sum(s2, red);
    if (threadIdx.x == 0) {
        const float mean = s1 / count;
        float var = s2 / count - mean * mean;  // biased batch variance
        var = fmaxf(var, 0.f);
        const float invstd = rsqrtf(var + eps);
        const float sc = gamma[c] * invstd;
        saved[c] = mean; saved[C + c] = invstd; saved[2 * C + c] = sc; saved[3 * C + c] = beta[c] - mean * sc;
        if (rmean) {
            const float unb = count > 1.f ? var * count / (count - 1.f) : var;
            rmean[c] = (1.f - momentum) * rmean[c] + momentum * mean;
            rvar[c] = (1.f - momentum) * rvar[c] + momentum * unb;
            if (c == 0 && nbt) nbt[0] += 1;
        }
    }
}

__global__ void bn_eval_coeffs_kernel(int C, const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                      const float* __restrict__ rmean, const float* __restrict__ rvar, float* __restrict__ saved) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < C) {
        const float invstd = rsqrtf(rvar[c] + eps), sc = gamma[c] * invstd;
        saved[c] = rmean[c]; saved[C + c] = invstd; saved[2 * C + c] = sc; saved[3 * C + c] = beta[c] - rmean[c] * sc;
    }
}

}  // namespace miseg

using namespace miseg;

extern "C" int miseg_bn_finalize(void* stream, const float* parts, int64_t nparts, int64_t C, int64_t count, const float* gamma,
                                 const float* beta, float eps, float momentum, float* rmean, float* rvar, int64_t* nbt, float* saved) {
    MISEG_TAPE(miseg_bn_finalize, stream, parts, nparts, C, count, gamma, beta, eps, momentum, rmean, rvar, nbt, saved);
    MISEG_REQUIRE(parts && gamma && beta && saved && C > 0 && nparts > 0 && count > 0, "bn_finalize: bad args");
    hipLaunchKernelGGL(bn_finalize_kernel, dim3((unsigned)C), dim3(256), 0, as_stream(stream), parts, (int)nparts, (int)C, (float)count, gamma,
                       beta, eps, momentum, rmean, rvar, (long long*)nbt, saved);
    MISEG_LAUNCH_CHECK("bn_finalize_kernel");
    return MISEG_OK;
}

extern "C" int miseg_bn_eval_coeffs(void* stream, int64_t C, const float* gamma, const float* beta, float eps, const float* rmean,
                                    const float* rvar, float* saved) {
    MISEG_TAPE(miseg_bn_eval_coeffs, stream, C, gamma, beta, eps, rmean, rvar, saved);
    MISEG_REQUIRE(gamma && beta && rmean && rvar && saved && C > 0, "bn_eval_coeffs: bad args");
    hipLaunchKernelGGL(bn_eval_coeffs_kernel, dim3((unsigned)cdiv(C, 64)), dim3(64), 0, as_stream(stream), (int)C, gamma, beta, eps, rmean, rvar, saved);
    MISEG_LAUNCH_CHECK("bn_eval_coeffs_kernel");
    return MISEG_OK;
}
