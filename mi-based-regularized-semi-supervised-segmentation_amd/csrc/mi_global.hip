// Global IIC mutual information (IIDLoss), all sub-heads per launch.  The encoder ClusterHead that feeds it is in heads_global.hip.
// ref: contrastyou/losses/iic_loss.py:43-94.
// These are latency-only ops (K <= 64, enforced; any N, a few dozen on the training path): one small block per sub-head, fp32, fixed order.
#include "common.h"

namespace miseg {

constexpr int kMaxK = 64;

// joint P (symmetrised, normalised) into LDS; returns via Ps[K*K], rowv[K], colv[K]
__device__ void global_joint(const float* x, const float* y, int N, int K, float* Ps, float* rowv, float* colv, float* red) {
    const int KK = K * K;
    for (int e = threadIdx.x; e < KK; e += blockDim.x) {
        int i = e / K, j = e % K;
        float s = 0.f, t = 0.f;
        for (int n = 0; n < N; ++n) {
            s += x[n * K + i] * y[n * K + j];
            t += x[n * K + j] * y[n * K + i];
        }
        Ps[e] = (s + t) / 2.0f;  // (P + P^T)/2, iic_loss.py:90-91
    }
    __syncthreads();
    float z = 0.f;
    for (int e = threadIdx.x; e < KK; e += blockDim.x) z += Ps[e];
    z = block_sum(z, red);
    for (int e = threadIdx.x; e < KK; e += blockDim.x) Ps[e] /= z;  // iic_loss.py:92
    __syncthreads();
    for (int c = threadIdx.x; c < K; c += blockDim.x) {
        float rs = 0.f, cs = 0.f;
        for (int t = 0; t < K; ++t) { rs += Ps[c * K + t]; cs += Ps[t * K + c]; }
        rowv[c] = rs;  // p_i = P.sum(dim=1)  (iic_loss.py:56-58)
        colv[c] = cs;  // p_j = P.sum(dim=0)  (iic_loss.py:59)
    }
    __syncthreads();
}

__global__ __launch_bounds__(256) void iic_global_fwd_kernel(const float* __restrict__ xs, const float* __restrict__ ys, int N,
                                                             int K, float lamb, float* __restrict__ loss,
                                                             float* __restrict__ loss_nl, float* __restrict__ joint, long long hs) {
    __shared__ float Ps[kMaxK * kMaxK];
    __shared__ float rowv[kMaxK], colv[kMaxK], red[17];
    const int s = blockIdx.x, KK = K * K;
    global_joint(xs + (size_t)s * hs, ys + (size_t)s * hs, N, K, Ps, rowv, colv, red);      // hs: elements between sub-heads
    const float eps = 1e-10f;
    float a = 0.f, b = 0.f;
    for (int e = threadIdx.x; e < KK; e += blockDim.x) {
        int i = e / K, j = e % K;
        float p = Ps[e], lp = logf(p + eps), lj = logf(colv[j] + eps), li = logf(rowv[i] + eps);
        a += -p * (lp - lamb * lj - lamb * li);
        b += -p * (lp - lj - li);
        joint[(size_t)s * KK + e] = p;
    }
    a = block_sum(a, red);
    b = block_sum(b, red);
    if (threadIdx.x == 0) { loss[s] = a; loss_nl[s] = b; }
}

// d loss / d x[n,i] = sum_j Gu[i][j] y[n,j], d loss / d y[n,j] = sum_i Gu[i][j] x[n,i], where
// Gu = d loss / d (unsymmetrised, unnormalised joint) = (Gsym - <Gsym, P>) / Z, Gsym = (Gp + Gp^T)/2.
__global__ __launch_bounds__(256) void iic_global_bwd_kernel(const float* __restrict__ xs, const float* __restrict__ ys, int N,
                                                             int K, float lamb, const float* __restrict__ upstream,
                                                             float* __restrict__ gxs, float* __restrict__ gys, long long hs) {
    __shared__ float Ps[kMaxK * kMaxK];
    __shared__ float Gp[kMaxK * kMaxK];
    __shared__ float rowv[kMaxK], colv[kMaxK], red[17];
    const int s = blockIdx.x, KK = K * K;
    const float* x = xs + (size_t)s * hs;
    const float* y = ys + (size_t)s * hs;
    global_joint(x, y, N, K, Ps, rowv, colv, red);
    // recover Z (sum of the symmetrised raw joint) = sum_n (sum_i x)(sum_j y)
    float z = 0.f;
    for (int n = threadIdx.x; n < N; n += blockDim.x) {
        float sx = 0.f, sy = 0.f;
        for (int k = 0; k < K; ++k) { sx += x[n * K + k]; sy += y[n * K + k]; }
        z += sx * sy;
    }
    z = block_sum(z, red);
    const float eps = 1e-10f;
    for (int e = threadIdx.x; e < KK; e += blockDim.x) {
        int i = e / K, j = e % K;
        float p = Ps[e], cj = colv[j], ri = rowv[i];
        Gp[e] = -(logf(p + eps) + p / (p + eps) - lamb * (logf(cj + eps) + cj / (cj + eps)) -
                  lamb * (logf(ri + eps) + ri / (ri + eps)));
    }
    __syncthreads();
    float dot = 0.f;
    for (int e = threadIdx.x; e < KK; e += blockDim.x) {
        int i = e / K, j = e % K;
        dot += (Gp[e] + Gp[j * K + i]) / 2.0f * Ps[e];
    }
    dot = block_sum(dot, red);
    const float up = upstream ? upstream[s] : 1.f;
    __syncthreads();
    // Gu overwrites Ps (symmetric)
    for (int e = threadIdx.x; e < KK; e += blockDim.x) {
        int i = e / K, j = e % K;
        Ps[e] = up * (((Gp[e] + Gp[j * K + i]) / 2.0f - dot) / z);
    }
    __syncthreads();
    // raw joint J = sum_n x_n y_n^T enters as (J + J^T)/2: dL/dJ = (Gu + Gu^T)/2 = Gu (symmetric)
    for (int e = threadIdx.x; e < N * K; e += blockDim.x) {
        int n = e / K, k = e % K;
        float ax = 0.f, ay = 0.f;
        for (int t = 0; t < K; ++t) {
            ax += Ps[k * K + t] * y[n * K + t];
            ay += Ps[t * K + k] * x[n * K + t];
        }
        gxs[(size_t)s * hs + e] = ax;
        gys[(size_t)s * hs + e] = ay;
    }
}

// compute_joint (ref iic_loss.py:74-94) on its own, with the reference's `symmetric` switch: P = sum_n x_n (x) y_n, optionally
// (P + P^T) / 2, divided by its sum.  IIDLoss always symmetrises (the fused kernels above); this pair serves direct callers.
__global__ __launch_bounds__(256) void iic_joint_fwd_kernel(const float* __restrict__ xs, const float* __restrict__ ys, int N, int K,
                                                            int symmetric, float* __restrict__ joint) {
    __shared__ float Ps[kMaxK * kMaxK];
    __shared__ float red[17];
    const int s = blockIdx.x, KK = K * K;
    const float* x = xs + (size_t)s * N * K;
    const float* y = ys + (size_t)s * N * K;
    for (int e = threadIdx.x; e < KK; e += blockDim.x) {
        const int i = e / K, j = e % K;
        float a = 0.f, t = 0.f;
        for (int n = 0; n < N; ++n) {
            a += x[n * K + i] * y[n * K + j];
            t += x[n * K + j] * y[n * K + i];
        }
        Ps[e] = symmetric ? (a + t) / 2.0f : a;
    }
    __syncthreads();
    float z = 0.f;
    for (int e = threadIdx.x; e < KK; e += blockDim.x) z += Ps[e];
    z = block_sum(z, red);
    for (int e = threadIdx.x; e < KK; e += blockDim.x) joint[(size_t)s * KK + e] = Ps[e] / z;
}

// given G = dL/dP:  dL/dQ = (G - <G, P>) / Z with Q the (symmetrised) raw joint; the raw outer-product sum J enters Q as
// (J + J^T)/2 when symmetric -> dL/dJ = (D + D^T)/2, else D;  gx[n,i] = sum_j dJ[i][j] y[n,j],  gy[n,j] = sum_i dJ[i][j] x[n,i].
__global__ __launch_bounds__(256) void iic_joint_bwd_kernel(const float* __restrict__ xs, const float* __restrict__ ys, int N, int K,
                                                            int symmetric, const float* __restrict__ joint, const float* __restrict__ gjoint,
                                                            float* __restrict__ gxs, float* __restrict__ gys) {
    __shared__ float D[kMaxK * kMaxK];
    __shared__ float red[17];
    const int s = blockIdx.x, KK = K * K;
    const float* x = xs + (size_t)s * N * K;
    const float* y = ys + (size_t)s * N * K;
    const float* P = joint + (size_t)s * KK;
    const float* G = gjoint + (size_t)s * KK;
    float z = 0.f;                                   // Z = sum_n (sum_i x)(sum_j y), symmetric or not
    for (int n = threadIdx.x; n < N; n += blockDim.x) {
        float sx = 0.f, sy = 0.f;
        for (int k = 0; k < K; ++k) { sx += x[n * K + k]; sy += y[n * K + k]; }
        z += sx * sy;
    }
    z = block_sum(z, red);
    float dot = 0.f;
    for (int e = threadIdx.x; e < KK; e += blockDim.x) dot += G[e] * P[e];
    dot = block_sum(dot, red);
    for (int e = threadIdx.x; e < KK; e += blockDim.x) {
        const int i = e / K, j = e % K;
        const float d = (G[e] - dot) / z, dt = (G[j * K + i] - dot) / z;
        D[e] = symmetric ? (d + dt) / 2.0f : d;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < N * K; e += blockDim.x) {
        const int n = e / K, k = e % K;
        float ax = 0.f, ay = 0.f;
        for (int t = 0; t < K; ++t) {
            ax += D[k * K + t] * y[n * K + t];
            ay += D[t * K + k] * x[n * K + t];
        }
        gxs[(size_t)s * N * K + e] = ax;
        gys[(size_t)s * N * K + e] = ay;
    }
}

}  // namespace miseg

using namespace miseg;

extern "C" int miseg_iic_global_joint_fwd(void* stream, const float* x, const float* y, int64_t S, int64_t N, int64_t K, int symmetric,
                                          float* joint) {
    MISEG_TAPE(miseg_iic_global_joint_fwd, stream, x, y, S, N, K, symmetric, joint);
    MISEG_REQUIRE(x && y && joint, "iic_global_joint_fwd: null pointer");
    MISEG_REQUIRE(S > 0 && N > 0 && K > 0 && K <= kMaxK, "iic_global_joint_fwd: need 0<K<=%d", kMaxK);
    hipLaunchKernelGGL(iic_joint_fwd_kernel, dim3((unsigned)S), dim3(256), 0, as_stream(stream), x, y, (int)N, (int)K, symmetric, joint);
    MISEG_LAUNCH_CHECK("iic_joint_fwd_kernel");
    return MISEG_OK;
}

extern "C" int miseg_iic_global_joint_bwd(void* stream, const float* x, const float* y, int64_t S, int64_t N, int64_t K, int symmetric,
                                          const float* joint, const float* gjoint, float* gx, float* gy) {
    MISEG_TAPE(miseg_iic_global_joint_bwd, stream, x, y, S, N, K, symmetric, joint, gjoint, gx, gy);
    MISEG_REQUIRE(x && y && joint && gjoint && gx && gy, "iic_global_joint_bwd: null pointer");
    MISEG_REQUIRE(S > 0 && N > 0 && K > 0 && K <= kMaxK, "iic_global_joint_bwd: need 0<K<=%d", kMaxK);
    hipLaunchKernelGGL(iic_joint_bwd_kernel, dim3((unsigned)S), dim3(256), 0, as_stream(stream), x, y, (int)N, (int)K, symmetric, joint, gjoint,
                       gx, gy);
    MISEG_LAUNCH_CHECK("iic_joint_bwd_kernel");
    return MISEG_OK;
}

extern "C" int miseg_iic_global_fwd_pair(void* stream, const float* prob, int64_t S, int64_t N, int64_t K, float lamb, float* loss,
                                         float* loss_no_lamb, float* joint) {
    MISEG_TAPE(miseg_iic_global_fwd_pair, stream, prob, S, N, K, lamb, loss, loss_no_lamb, joint);
    MISEG_REQUIRE(prob && loss && loss_no_lamb && joint, "iic_global_fwd: null pointer");
    MISEG_REQUIRE(S > 0 && N > 0 && K > 0 && K <= kMaxK, "iic_global_fwd: need 0<K<=%d", kMaxK);
    hipLaunchKernelGGL(iic_global_fwd_kernel, dim3((unsigned)S), dim3(256), 0, as_stream(stream), prob, prob + N * K, (int)N, (int)K, lamb, loss,
                       loss_no_lamb, joint, (long long)(2 * N * K));
    MISEG_LAUNCH_CHECK("iic_global_fwd_kernel");
    return MISEG_OK;
}

extern "C" int miseg_iic_global_bwd_pair(void* stream, const float* prob, int64_t S, int64_t N, int64_t K, float lamb, const float* upstream,
                                         float* gprob) {
    MISEG_TAPE(miseg_iic_global_bwd_pair, stream, prob, S, N, K, lamb, upstream, gprob);
    MISEG_REQUIRE(prob && gprob, "iic_global_bwd: null pointer");
    MISEG_REQUIRE(S > 0 && N > 0 && K > 0 && K <= kMaxK, "iic_global_bwd: need 0<K<=%d", kMaxK);
    hipLaunchKernelGGL(iic_global_bwd_kernel, dim3((unsigned)S), dim3(256), 0, as_stream(stream), prob, prob + N * K, (int)N, (int)K, lamb,
                       upstream, gprob, gprob + N * K, (long long)(2 * N * K));
    MISEG_LAUNCH_CHECK("iic_global_bwd_kernel");
    return MISEG_OK;
}

extern "C" int miseg_iic_global_fwd(void* stream, const float* x, const float* y, int64_t S, int64_t N, int64_t K, float lamb,
                                    float* loss, float* loss_no_lamb, float* joint) {
    MISEG_TAPE(miseg_iic_global_fwd, stream, x, y, S, N, K, lamb, loss, loss_no_lamb, joint);
    MISEG_REQUIRE(x && y && loss && loss_no_lamb && joint, "iic_global_fwd: null pointer");
    MISEG_REQUIRE(S > 0 && N > 0 && K > 0 && K <= kMaxK, "iic_global_fwd: need 0<K<=%d", kMaxK);
    hipLaunchKernelGGL(iic_global_fwd_kernel, dim3((unsigned)S), dim3(256), 0, as_stream(stream), x, y, (int)N, (int)K, lamb, loss,
                       loss_no_lamb, joint, (long long)(N * K));
    MISEG_LAUNCH_CHECK("iic_global_fwd_kernel");
    return MISEG_OK;
}

extern "C" int miseg_iic_global_bwd(void* stream, const float* x, const float* y, int64_t S, int64_t N, int64_t K, float lamb,
                                    const float* upstream, float* gx, float* gy) {
    MISEG_TAPE(miseg_iic_global_bwd, stream, x, y, S, N, K, lamb, upstream, gx, gy);
    MISEG_REQUIRE(x && y && gx && gy, "iic_global_bwd: null pointer");
    MISEG_REQUIRE(S > 0 && N > 0 && K > 0 && K <= kMaxK, "iic_global_bwd: need 0<K<=%d", kMaxK);
    hipLaunchKernelGGL(iic_global_bwd_kernel, dim3((unsigned)S), dim3(256), 0, as_stream(stream), x, y, (int)N, (int)K, lamb,
                       upstream, gx, gy, (long long)(N * K));
    MISEG_LAUNCH_CHECK("iic_global_bwd_kernel");
    return MISEG_OK;
}
