// Per-sample affine warp of an fp32 batch and its exact adjoint: F.affine_grid + F.grid_sample(align_corners=True, padding_mode="zeros")
// without the [N][H][W][2] grid (ref contrastyou/augment/tensor_affine_transform.py:68-78, AffineTensorTransform._perform_affine_transform).
//
// One function, source_taps(), says where output pixel (i, j) of sample n reads and with which weights; the forward and the backward
// both call it, and this unit is compiled without floating-point contraction (Makefile), so the two see the same bits:
//
//   fwd   y[n,c,p] = sum over the taps q of p   w(p, q) * x[n,c,q]         a gather: one thread per output pixel and 4 channels
//   bwd   gx[n,c,q] = sum over p with q a tap  w(p, q) * gy[n,c,p]         a gather too: one thread per INPUT pixel and <= 16 channels
//
// The backward finds its output pixels by search.  In pixel units the map is s(p) = A p + b (A from theta and the two axis lengths);
// p reads q only if |s(p) - q| < 1 on both axes, i.e. p - A^-1 (q - b) = A^-1 u with |u| < 1: within the largest row sum of |A^-1|
// of the pre-image.  The thread rounds the pre-image to a pixel, clamps it into the image (a pixel of the image within `reach` of a
// centre outside it is within `reach` of the clamped one) and scans the (2 reach + 1)^2 box around it in row-major order, adding what
// source_taps() gives for every pixel that reads q.  No atomics, a fixed order: two calls give the same bits.  `reach` comes from the
// caller, who knows the matrices (include/miseg_hip.h); a box of reach >= max(H, W) - 1 is the whole image whatever the centre, which
// is what serves a singular A (a 90 degree turn of a one-pixel-wide image maps every pixel to one point).
//
// Memory order: NCHW blocks are 16 x 16 tiles of pixels, a wave four rows of 16 (64-byte runs along W, 4 channels = 4 planes each); NHWC
// threads run along C, 16 bytes each when C % 4 == 0 and the pointers are 16-byte aligned, one float each otherwise.  No LDS.
#include "common.h"
#include <math.h>

namespace miseg {
namespace {

constexpr int kMaxSide = 2048;
constexpr int kMaxReach = 8;
constexpr int kThreads = 256;
constexpr int kChunk = 4;                // channels per thread (NCHW planes, or one 16-byte NHWC vector)

enum Layout { kPlanes = 0, kVec4 = 1, kScalar = 2 };      // NCHW | NHWC, C % 4 == 0 | NHWC, any C

struct Theta {
    float t[6];
};
__device__ __forceinline__ Theta load_theta(const float* __restrict__ theta, int n) {
    Theta m;
#pragma unroll
    for (int k = 0; k < 6; ++k) m.t[k] = theta[(size_t)n * 6 + k];
    return m;
}

// torch's base grid for align_corners=True: linspace(-1, 1, L), and 0 for an axis of length 1
__device__ __forceinline__ float base_coord(int k, int L) { return L > 1 ? (float)(2 * k - (L - 1)) / (float)(L - 1) : 0.f; }

// Where output pixel (yn, xn in base-grid coordinates) reads: the top-left tap (x0, y0) and the fractions towards the next column /
// row.  MODE 0 bilinear: taps (x0 + dx, y0 + dy), dx, dy in {0, 1}.  MODE 1 nearest: the one tap (x0, y0), fractions 0.
// A point no tap of which lies in the image -- a NaN or an infinity among them: every comparison fails -- gets x0 = y0 = -2.
struct Taps {
    int x0, y0;
    float fx, fy;
};
template <int MODE> __device__ __forceinline__ Taps source_taps(const Theta& m, float xn, float yn, int H, int W) {
    const float gx = fmaf(m.t[0], xn, fmaf(m.t[1], yn, m.t[2]));
    const float gy = fmaf(m.t[3], xn, fmaf(m.t[4], yn, m.t[5]));
    const float sx = (gx + 1.f) * 0.5f * (float)(W - 1);
    const float sy = (gy + 1.f) * 0.5f * (float)(H - 1);
    Taps t;
    if (MODE == 0) {
        const float flx = floorf(sx), fly = floorf(sy);
        const bool ok = sx > -1.f && sx < (float)W && sy > -1.f && sy < (float)H;
        t.x0 = ok ? (int)flx : -2;
        t.y0 = ok ? (int)fly : -2;
        t.fx = sx - flx;
        t.fy = sy - fly;
    } else {
        const float rx = rintf(sx), ry = rintf(sy);              // ties to even, as nearbyint in the default rounding mode
        const bool ok = rx >= 0.f && rx <= (float)(W - 1) && ry >= 0.f && ry <= (float)(H - 1);
        t.x0 = ok ? (int)rx : -2;
        t.y0 = ok ? (int)ry : -2;
        t.fx = 0.f;
        t.fy = 0.f;
    }
    return t;
}
// weight of tap (dx, dy) in {0, 1}^2: (1 - |sx - x'|)(1 - |sy - y'|)
__device__ __forceinline__ float tap_weight(const Taps& t, int dx, int dy) { return (dx ? t.fx : 1.f - t.fx) * (dy ? t.fy : 1.f - t.fy); }

// ---- the channels a thread owns at one pixel: `nu` units of K channels (K = 4: four NCHW planes or one 16-byte NHWC vector; K = 1: one
// NHWC float).  The forward owns one unit; the backward up to kBwdUnits, so that its search is shared by 16 channels.
constexpr int kBwdUnits = 4;
template <int LAYOUT> struct Px {
    static constexpr int K = LAYOUT == kScalar ? 1 : kChunk;
    int nu;                          // units of this thread
    int cleft;                       // channels from this thread's first unit to the last one (kPlanes: the last unit may be short)
    size_t base, cstride, ustride;   // element offset of (n, first channel, pixel 0); channel stride; unit stride
    int pstride;                     // pixel stride
    __device__ __forceinline__ void fma_from(const float* __restrict__ src, int pix, float w, float* acc, int u = 0) const {
        const size_t o = base + u * ustride + (size_t)pix * pstride;
        if (LAYOUT == kVec4) {
            const float4 v = *reinterpret_cast<const float4*>(src + o);
            acc[0] = fmaf(w, v.x, acc[0]); acc[1] = fmaf(w, v.y, acc[1]); acc[2] = fmaf(w, v.z, acc[2]); acc[3] = fmaf(w, v.w, acc[3]);
        } else {
            const int nc = cleft - u * K;
            float v[K];
#pragma unroll
            for (int k = 0; k < K; ++k) v[k] = k < nc ? src[o + k * cstride] : 0.f;
#pragma unroll
            for (int k = 0; k < K; ++k) acc[k] = fmaf(w, v[k], acc[k]);
        }
    }
    __device__ __forceinline__ void store(float* __restrict__ dst, int pix, const float* acc, int u = 0) const {
        const size_t o = base + u * ustride + (size_t)pix * pstride;
        if (LAYOUT == kVec4) {
            *reinterpret_cast<float4*>(dst + o) = make_float4(acc[0], acc[1], acc[2], acc[3]);
        } else {
            const int nc = cleft - u * K;
#pragma unroll
            for (int k = 0; k < K; ++k)
                if (k < nc) dst[o + k * cstride] = acc[k];
        }
    }
};
static inline int64_t unit_count(int layout, int64_t C) { return layout == kScalar ? C : cdiv(C, kChunk); }

// Block and thread index -> (sample, channel group, pixel).
// kPlanes: a block is a kTileW x kTileH tile of one sample's channel group, a wave 16 x 4 pixels of it.  A turned image reads along
// slanted lines: a 256-pixel row of output pixels touches up to 256 rows of the source, a tile a patch of its own size.  Measured on
// an MI355X, 16 x 16 x 256 x 256, the default ranges' matrices, forward / forward + backward in us: tiles of 256 x 1: 218 / 483,
// 64 x 4: 162 / 391, 32 x 8: 98 / 318, 16 x 16: 88 / 303.  The tile's position is block-uniform arithmetic.
// NHWC: the channel group runs fastest, then the pixel (32-bit: there are fewer threads than elements, fewer than 2^31 of those).
constexpr int kTileW = 16, kTileH = kThreads / kTileW;
template <int LAYOUT, int UPT> __device__ __forceinline__ bool decode(unsigned total, int C, int H, int W, int& n, int& pix, Px<LAYOUT>& px) {
    const int HW = H * W, K = Px<LAYOUT>::K, units = (C + K - 1) / K, groups = (units + UPT - 1) / UPT;
    int g;
    if (LAYOUT == kPlanes) {
        const unsigned tiles_x = (W + kTileW - 1) / kTileW, tiles_y = (H + kTileH - 1) / kTileH;
        unsigned b = blockIdx.x;
        const int tx = b % tiles_x;
        b /= tiles_x;
        const int ty = b % tiles_y;
        b /= tiles_y;
        g = b % groups;
        n = b / groups;
        const int j = tx * kTileW + (int)(threadIdx.x % kTileW), i = ty * kTileH + (int)(threadIdx.x / kTileW);
        if (i >= H || j >= W) return false;
        pix = i * W + j;
        px.base = ((size_t)n * C + (size_t)g * UPT * K) * HW;
        px.cstride = (size_t)HW;
        px.ustride = (size_t)K * HW;
        px.pstride = 1;
    } else {
        const unsigned idx = blockIdx.x * kThreads + threadIdx.x;
        if (idx >= total) return false;
        const int r = (int)(idx / groups);
        g = (int)(idx % groups);
        pix = r % HW;
        n = r / HW;
        px.base = (size_t)n * HW * C + (size_t)g * UPT * K;
        px.cstride = 1;
        px.ustride = K;
        px.pstride = C;
    }
    px.nu = min(UPT, units - g * UPT);
    px.cleft = C - g * UPT * K;
    return true;
}
// (threads of the NHWC kernels, blocks of either)
struct Grid {
    unsigned total, blocks;
};
Grid grid_of(int layout, int upt, int64_t N, int64_t C, int64_t H, int64_t W) {
    const int64_t groups = cdiv(unit_count(layout, C), upt);
    if (layout == kPlanes) return {0u, (unsigned)(cdiv(W, kTileW) * cdiv(H, kTileH) * groups * N)};      // <= N C H W < 2^31
    const int64_t total = N * groups * H * W;
    return {(unsigned)total, (unsigned)cdiv(total, kThreads)};
}

template <int MODE, int LAYOUT>
__global__ __launch_bounds__(kThreads) void affine_warp_fwd_kernel(const float* __restrict__ x, const float* __restrict__ theta, unsigned total,
                                                                   int C, int H, int W, float* __restrict__ y) {
    int n, pix;
    Px<LAYOUT> px;
    if (!decode<LAYOUT, 1>(total, C, H, W, n, pix, px)) return;
    const int i = pix / W, j = pix - i * W;
    const Taps t = source_taps<MODE>(load_theta(theta, n), base_coord(j, W), base_coord(i, H), H, W);
    float acc[Px<LAYOUT>::K] = {};
    constexpr int NT = MODE == 0 ? 2 : 1;
#pragma unroll
    for (int dy = 0; dy < NT; ++dy)
#pragma unroll
        for (int dx = 0; dx < NT; ++dx) {
            const int yy = t.y0 + dy, xx = t.x0 + dx;
            if (yy >= 0 && yy < H && xx >= 0 && xx < W) px.fma_from(x, yy * W + xx, tap_weight(t, dx, dy), acc);
        }
    px.store(y, pix, acc);
}

// UPT = units per thread: kBwdUnits, or 1 when there is one unit in all (C <= 4 logits: 16 x 4 x 256 x 256 channels_last ran 137 us
// forward + backward through the 4-unit code against 118 us).
template <int MODE, int LAYOUT, int UPT>
__global__ __launch_bounds__(kThreads) void affine_warp_bwd_kernel(const float* __restrict__ gy, const float* __restrict__ theta, unsigned total,
                                                                   int C, int H, int W, int reach, float* __restrict__ gx) {
    int n, pix;
    Px<LAYOUT> px;
    if (!decode<LAYOUT, UPT>(total, C, H, W, n, pix, px)) return;
    const int qy = pix / W, qx = pix - qy * W;
    const Theta m = load_theta(theta, n);
    // s(p) = A p + b in pixels; an axis of length 1 neither moves the source point nor is moved along: its row and column of A are
    // those of the identity.  In double, once per thread: the centre is then off by its rounding to a pixel alone, whatever A's
    // condition, and `reach` carries one pixel of slack for that and for the fp32 rounding of the forward's source points.
    const bool both = H > 1 && W > 1;
    const double a00 = W > 1 ? (double)m.t[0] : 1.0, a11 = H > 1 ? (double)m.t[4] : 1.0;
    const double a01 = both ? (double)m.t[1] * (double)(W - 1) / (double)(H - 1) : 0.0;
    const double a10 = both ? (double)m.t[3] * (double)(H - 1) / (double)(W - 1) : 0.0;
    const double xn0 = W > 1 ? -1.0 : 0.0, yn0 = H > 1 ? -1.0 : 0.0;
    const double b0 = ((double)m.t[0] * xn0 + (double)m.t[1] * yn0 + (double)m.t[2] + 1.0) * 0.5 * (double)(W - 1);
    const double b1 = ((double)m.t[3] * xn0 + (double)m.t[4] * yn0 + (double)m.t[5] + 1.0) * 0.5 * (double)(H - 1);
    const double det = a00 * a11 - a01 * a10, u = (double)qx - b0, v = (double)qy - b1;
    // fmax / fmin drop a NaN operand: a singular or overflowing A gives SOME pixel of the image, and the caller's reach covers it all
    const int cj = (int)rint(fmin(fmax((a11 * u - a01 * v) / det, 0.0), (double)(W - 1)));
    const int ci = (int)rint(fmin(fmax((a00 * v - a10 * u) / det, 0.0), (double)(H - 1)));
    const int i0 = max(ci - reach, 0), i1 = min(ci + reach, H - 1), j0 = max(cj - reach, 0), j1 = min(cj + reach, W - 1);
    float acc[UPT][Px<LAYOUT>::K] = {};
    constexpr unsigned NT = MODE == 0 ? 2 : 1;
    for (int i = i0; i <= i1; ++i) {
        const float yn = base_coord(i, H);
        for (int j = j0; j <= j1; ++j) {
            const Taps t = source_taps<MODE>(m, base_coord(j, W), yn, H, W);
            const int dx = qx - t.x0, dy = qy - t.y0;
            if ((unsigned)dx < NT && (unsigned)dy < NT) {
                const float wgt = tap_weight(t, dx, dy);
#pragma unroll
                for (int un = 0; un < UPT; ++un)
                    if (un < px.nu) px.fma_from(gy, i * W + j, wgt, acc[un], un);
            }
        }
    }
#pragma unroll
    for (int un = 0; un < UPT; ++un)
        if (un < px.nu) px.store(gx, pix, acc[un], un);
}

bool affine_shape_ok(int64_t C, int64_t H, int64_t W, int channels_last, int mode) {
    return C >= 1 && H >= 1 && W >= 1 && H <= kMaxSide && W <= kMaxSide && (channels_last == 0 || channels_last == 1) &&
           (mode == 0 || mode == 1) && C * H * W < (1LL << 31);
}
bool affine_batch_ok(int64_t N, int64_t C, int64_t H, int64_t W) {
    return N >= 1 && N < (1LL << 31) && N * C * H * W < (1LL << 31);      // the first test keeps the product from wrapping: C H W < 2^31
}
int pick_layout(int channels_last, int64_t C, const void* a, const void* b) {
    if (!channels_last) return kPlanes;
    const bool aligned = ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) == 0;
    return C % kChunk == 0 && aligned ? kVec4 : kScalar;
}

// f(mode tag, layout tag) for the run-time pair
template <typename F> void with_mode_layout(int mode, int layout, F&& f) {
    auto with_layout = [&](auto mode_tag) {
        if (layout == kPlanes) f(mode_tag, std::integral_constant<int, kPlanes>{});
        else if (layout == kVec4) f(mode_tag, std::integral_constant<int, kVec4>{});
        else f(mode_tag, std::integral_constant<int, kScalar>{});
    };
    if (mode == 0) with_layout(std::integral_constant<int, 0>{});
    else with_layout(std::integral_constant<int, 1>{});
}

}  // namespace
}  // namespace miseg

using namespace miseg;

extern "C" int64_t miseg_affine_warp_supported(int64_t C, int64_t H, int64_t W, int channels_last, int mode) {
    return affine_shape_ok(C, H, W, channels_last, mode) ? 1 : -1;
}

extern "C" int miseg_affine_warp_fwd(void* stream, const float* x, const float* theta, int64_t N, int64_t C, int64_t H, int64_t W,
                                     int channels_last, int mode, float* y) {
    MISEG_TAPE(miseg_affine_warp_fwd, stream, x, theta, N, C, H, W, channels_last, mode, y);
    MISEG_REQUIRE(x && theta && y, "affine_warp_fwd: null pointer");
    MISEG_REQUIRE(affine_shape_ok(C, H, W, channels_last, mode) && affine_batch_ok(N, C, H, W),
                  "affine_warp_fwd: unsupported configuration (N, C >= 1, 1 <= H, W <= 2048, fewer than 2^31 elements, channels_last and mode 0 or 1)");
    const int layout = pick_layout(channels_last, C, x, y);
    const Grid grid = grid_of(layout, 1, N, C, H, W);
    with_mode_layout(mode, layout, [&](auto mode_tag, auto layout_tag) {
        hipLaunchKernelGGL((affine_warp_fwd_kernel<decltype(mode_tag)::value, decltype(layout_tag)::value>), dim3(grid.blocks),
                           dim3(kThreads), 0, as_stream(stream), x, theta, grid.total, (int)C, (int)H, (int)W, y);
    });
    MISEG_LAUNCH_CHECK("affine_warp_fwd_kernel");
    return MISEG_OK;
}

extern "C" int miseg_affine_warp_bwd(void* stream, const float* gy, const float* theta, int64_t N, int64_t C, int64_t H, int64_t W,
                                     int channels_last, int mode, int64_t reach, float* gx) {
    MISEG_TAPE(miseg_affine_warp_bwd, stream, gy, theta, N, C, H, W, channels_last, mode, reach, gx);
    MISEG_REQUIRE(gy && theta && gx, "affine_warp_bwd: null pointer");
    MISEG_REQUIRE(affine_shape_ok(C, H, W, channels_last, mode) && affine_batch_ok(N, C, H, W),
                  "affine_warp_bwd: unsupported configuration (N, C >= 1, 1 <= H, W <= 2048, fewer than 2^31 elements, channels_last and mode 0 or 1)");
    MISEG_REQUIRE(reach >= 1 && reach <= kMaxReach, "affine_warp_bwd: reach must lie in [1, 8]");
    const int layout = pick_layout(channels_last, C, gy, gx);
    const int upt = unit_count(layout, C) == 1 ? 1 : kBwdUnits;
    const Grid grid = grid_of(layout, upt, N, C, H, W);
    with_mode_layout(mode, layout, [&](auto mode_tag, auto layout_tag) {
        constexpr int M = decltype(mode_tag)::value, L = decltype(layout_tag)::value;
        auto* kernel = upt == 1 ? affine_warp_bwd_kernel<M, L, 1> : affine_warp_bwd_kernel<M, L, kBwdUnits>;
        hipLaunchKernelGGL(kernel, dim3(grid.blocks), dim3(kThreads), 0, as_stream(stream), gy, theta, grid.total, (int)C, (int)H, (int)W,
                           (int)reach, gx);
    });
    MISEG_LAUNCH_CHECK("affine_warp_bwd_kernel");
    return MISEG_OK;
}
