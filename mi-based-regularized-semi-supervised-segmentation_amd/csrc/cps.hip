// Cross pseudo supervision (Trainer.name=cps; Chen et al., CVPR 2021): the pixel-streaming loss of two networks that supervise each
// other with their hard predictions.
//   softmax_cross_pseudo   cps_a = mean_pix (logsumexp(a) - a[yb]),  cps_b = mean_pix (logsumexp(b) - b[ya]),
//                          ya = argmax_c a_c, yb = argmax_c b_c (the lowest index wins a tie; +0.0 and -0.0 tie), labels detached;
//                          ga = upstream (softmax(a) - e_yb) / npix, gb = upstream (softmax(b) - e_ya) / npix;
//                          agree = the number of pixels with ya == yb
// The first pixel loss with two differentiable operands, and the first whose target is computed on the device from the other operand.
//
// HBM-bound: one pixel per thread with both channel vectors in registers (one 16-byte load per row where C is a multiple of 4), every
// label-dependent access a compare-and-select over the unrolled class loop, so nothing is indexed at run time and nothing spills.
// Pass 1 reads a and b once, writes both gradients (the denominator npix is a constant: no later scaling launch) and leaves per-block
// partials -- two fp32 sums and an exact integer count; pass 2, one block, adds the partials in a fixed order in double.  No atomics:
// two calls give the same bits, and a call without gradients runs the same arithmetic for the loss.  The per-pixel loss is
// (max - z[y]) + log(sum exp(z - max)): plain cross entropy with no epsilon, finite wherever the logits are.  The softmax, the row
// loads, the pixel grid, the integer block sum and the class-count dispatch are those of pixel_loss.h.
#include "pixel_loss.h"

namespace miseg {
namespace cps {

constexpr int kT = 256;
static_assert(kT == kPixelThreads, "pixel_blocks() counts blocks of kT pixels");

// The workspace: agreement partials (int64 [nb]) | cps_a partials (fp32 [nb]) | cps_b partials (fp32 [nb]).
struct Workspace {
    long long* agree;
    float* sa;
    float* sb;
    __host__ __device__ Workspace(void* ws, int nb) : agree(static_cast<long long*>(ws)), sa(reinterpret_cast<float*>(agree + nb)), sb(sa + nb) {}
};

// first maximum of the row: a later entry wins only if it is strictly greater (so -0.0 does not beat +0.0, nor the reverse)
template <int C>
__device__ __forceinline__ int first_argmax(const float* z) {
    int y = 0;
    float m = z[0];
#pragma unroll
    for (int c = 1; c < C; ++c)
        if (z[c] > m) { m = z[c]; y = c; }
    return y;
}

// cross entropy of the row against the hard label y: (max - z[y]) + log(sum exp(z - max))
template <int C>
__device__ __forceinline__ float cross_entropy(const float* z, int y) {
    float mx = -3.4e38f, zy = z[0];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        mx = fmaxf(mx, z[c]);
        zy = c == y ? z[c] : zy;
    }
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) s += expf(z[c] - mx);
    return (mx - zy) + logf(s);
}

// g = k (softmax(z) - e_y), stored as one row
template <int C, bool V4>
__device__ __forceinline__ void store_grad(const float* z, int y, float k, float* __restrict__ g) {
    float p[C];
    softmax_c(z, C, p);
#pragma unroll
    for (int c = 0; c < C; ++c) p[c] = k * (p[c] - (c == y ? 1.f : 0.f));
    store_row<C, V4>(g, p);
}

template <int C, bool V4>
__global__ __launch_bounds__(kT) void cross_pseudo_kernel(const float* __restrict__ a, const float* __restrict__ b, int64_t npix,
                                                          const float* __restrict__ upstream, void* __restrict__ ws, float* __restrict__ ga,
                                                          float* __restrict__ gb) {
    __shared__ float red[17];
    __shared__ long long redk[17];
    const float k = (upstream ? upstream[0] : 1.f) / (float)npix;
    float part_a = 0.f, part_b = 0.f;
    long long same = 0;
    for (int64_t i = blockIdx.x * (int64_t)kT + threadIdx.x; i < npix; i += (int64_t)gridDim.x * kT) {
        float za[C], zb[C];
        load_row<C, V4>(a + i * C, za);
        load_row<C, V4>(b + i * C, zb);
        const int ya = first_argmax<C>(za), yb = first_argmax<C>(zb);
        same += ya == yb ? 1 : 0;
        part_a += cross_entropy<C>(za, yb);
        part_b += cross_entropy<C>(zb, ya);
        if (ga) store_grad<C, V4>(za, yb, k, ga + i * C);
        if (gb) store_grad<C, V4>(zb, ya, k, gb + i * C);
    }
    part_a = block_sum(part_a, red);
    part_b = block_sum(part_b, red);
    same = block_sum_i64(same, redk);
    if (threadIdx.x == 0) {
        const Workspace w(ws, gridDim.x);
        w.agree[blockIdx.x] = same;
        w.sa[blockIdx.x] = part_a;
        w.sb[blockIdx.x] = part_b;
    }
}

// pass 2, one block: thread t adds partials t, t + 256, ... in double, then a fixed tree over the 256 threads
__global__ __launch_bounds__(kT) void cross_pseudo_finish_kernel(void* __restrict__ ws, int nb, int64_t npix, float* __restrict__ loss,
                                                                 long long* __restrict__ agree) {
    __shared__ double ra[kT], rb[kT];
    __shared__ long long rk[kT];
    const Workspace w(ws, nb);
    double sa = 0.0, sb = 0.0;
    long long k = 0;
    for (int i = threadIdx.x; i < nb; i += kT) { sa += (double)w.sa[i]; sb += (double)w.sb[i]; k += w.agree[i]; }
    ra[threadIdx.x] = sa; rb[threadIdx.x] = sb; rk[threadIdx.x] = k;
    __syncthreads();
    for (int o = kT / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            ra[threadIdx.x] += ra[threadIdx.x + o];
            rb[threadIdx.x] += rb[threadIdx.x + o];
            rk[threadIdx.x] += rk[threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        loss[0] = (float)(ra[0] / (double)npix);
        loss[1] = (float)(rb[0] / (double)npix);
        if (agree) agree[0] = rk[0];
    }
}

static inline bool overlaps(const float* p, const float* q, int64_t numel) { return p && q && p < q + numel && q < p + numel; }

}  // namespace cps
}  // namespace miseg

using namespace miseg;

extern "C" int64_t miseg_softmax_cross_pseudo_ws_bytes(int64_t N, int64_t H, int64_t W) {
    if (N <= 0 || H <= 0 || W <= 0) return 0;
    return (int64_t)pixel_blocks(N * H * W) * 16;
}

extern "C" int miseg_softmax_cross_pseudo(void* stream, const float* a, const float* b, int64_t N, int64_t H, int64_t W, int64_t C,
                                          const float* upstream, float* loss, float* ga, float* gb, int64_t* agree, void* ws,
                                          int64_t ws_bytes) {
    MISEG_TAPE(miseg_softmax_cross_pseudo, stream, a, b, N, H, W, C, upstream, loss, ga, gb, agree, ws, ws_bytes);
    MISEG_REQUIRE(a && b && loss && ws, "softmax_cross_pseudo: null pointer");
    MISEG_REQUIRE(class_count_has_kernel(C), "softmax_cross_pseudo: unsupported class count %ld (2-6,8,10,16)", (long)C);
    MISEG_REQUIRE(N > 0 && H > 0 && W > 0 && N < (1LL << 31), "softmax_cross_pseudo: empty batch / bad shape");
    const int64_t need = miseg_softmax_cross_pseudo_ws_bytes(N, H, W);
    MISEG_REQUIRE(ws_bytes >= need && ((uintptr_t)ws & 7) == 0, "softmax_cross_pseudo: workspace of %ld bytes (8-byte aligned), %ld needed",
                  (long)ws_bytes, (long)need);
    const int64_t npix = N * H * W, numel = npix * C;
    MISEG_REQUIRE(!cps::overlaps(ga, a, numel) && !cps::overlaps(ga, b, numel) && !cps::overlaps(gb, a, numel) && !cps::overlaps(gb, b, numel) &&
                      !cps::overlaps(ga, gb, numel),
                  "softmax_cross_pseudo: a gradient overlaps an operand or the other gradient");
    const int nb = pixel_blocks(npix);
    const bool v4 = C % 4 == 0 && aligned16(a) && aligned16(b) && (!ga || aligned16(ga)) && (!gb || aligned16(gb));
    hipStream_t st = as_stream(stream);
#define L(CC, VV) hipLaunchKernelGGL((cps::cross_pseudo_kernel<CC, VV>), dim3(nb), dim3(cps::kT), 0, st, a, b, npix, upstream, ws, ga, gb)
    MISEG_DISPATCH_C_V4(C, v4, L)
#undef L
    MISEG_LAUNCH_CHECK("cross_pseudo_kernel");
    hipLaunchKernelGGL(cps::cross_pseudo_finish_kernel, dim3(1), dim3(cps::kT), 0, st, ws, nb, npix, loss, (long long*)agree);
    MISEG_LAUNCH_CHECK("cross_pseudo_finish_kernel");
    return MISEG_OK;
}
