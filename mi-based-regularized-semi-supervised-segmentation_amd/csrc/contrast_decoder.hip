// Contrastive decoder pre-training (Trainer.name=contrastdecoder): what the reference's LocalProjectionHead needs around the bias-free
// 3x3 convolution kernels of conv_*.hip -- bias + LeakyReLU and its backward (with the bias gradient), and the adaptive max-pool with
// the bias of the convolution in front of it, written straight into the rows the supervised-contrastive loss reads.
// ref: contrastyou/trainer/_utils.py:68-93 (LocalProjectionHead), contrastyou/epocher/_utils.py:36-49 (unfold_position),
// contrastyou/epocher/contrast_epocher.py:149-155 (chunk, unfold, view(b, -1)).
// Every kernel is one streaming pass over an NHWC tensor of the storage type; fp32 arithmetic, no floating-point atomics, every sum in
// a fixed order.  A thread moves VEC channels at a time: 16 bytes, or 8 for a 16-bit type whose C is not a multiple of 8.
#include "common.h"

namespace miseg {

constexpr int kCdMaxC = 1024;            // one block spans all channels of a pixel: C / VEC <= 256 threads
constexpr int kCdMaxBlocks = 1024;       // grid cap of the grid-stride kernels (four blocks per CU)

template <typename T, int VEC> struct alignas(VEC * sizeof(T)) CdPack { T v[VEC]; };
struct alignas(16) CdIdx4 { int32_t v[4]; };

// fp32 add and multiply as two roundings whatever the contraction mode of the build
__device__ __forceinline__ float cd_lrelu(float raw, float b, float slope) {
    const float v = __fadd_rn(raw, b);
    return v > 0.f ? v : __fmul_rn(v, slope);
}

// ---------------------------------------------------------------- y = T(lrelu(raw + bias[c]))
// Grid-stride over the nvec = N*H*W*C/VEC vectors, four independent (bounds-checked) loads in flight per thread.  Each vector is read and written by the
// same thread, so y may be raw itself (no __restrict__ on the two).
template <typename T, int VEC>
__global__ __launch_bounds__(256) void bias_lrelu_fwd_kernel(const T* raw, size_t nvec, int cvn, const float* __restrict__ bias, float slope, T* y) {
    typedef CdPack<T, VEC> P;
    const P* in = reinterpret_cast<const P*>(raw);
    P* out = reinterpret_cast<P*>(y);
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += 4 * stride) {
        P p[4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (i + u * stride < nvec) p[u] = in[i + u * stride];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (i + u * stride >= nvec) break;
            const int c0 = (int)((i + u * stride) % (size_t)cvn) * VEC;
#pragma unroll
            for (int k = 0; k < VEC; ++k) p[u].v[k] = from_f32<T>(cd_lrelu(to_f32(p[u].v[k]), bias[c0 + k], slope));
            out[i + u * stride] = p[u];
        }
    }
}

// ---------------------------------------------------------------- gx = T(y > 0 ? g : g * slope), parts[block][C] = the block's fp32 sums
// A block is rpb = 256 / cvn pixel rows of cvn = C / VEC threads (consecutive threads read consecutive vectors); thread (r, col) walks
// the pixels blockIdx * rpb + r, + gridDim * rpb, ... and keeps the sums of its VEC channels.  The rpb rows are added through LDS in
// row order, the blocks' rows by bias_parts_reduce_kernel in block order.
static inline int cd_rows_per_block(int cvn) { return 256 / cvn; }
static inline int64_t cd_lrelu_bwd_blocks(int64_t npix, int cvn) { return std::min<int64_t>(cdiv(npix, cd_rows_per_block(cvn)), kCdMaxBlocks); }

template <typename T, int VEC>
__global__ __launch_bounds__(256) void bias_lrelu_bwd_kernel(const T* __restrict__ y, const T* gy, size_t npix, int cvn, float slope, T* gx,
                                                             float* __restrict__ parts) {
    typedef CdPack<T, VEC> P;
    extern __shared__ float cd_sm[];            // [rpb][C]
    const int rpb = 256 / cvn, r = threadIdx.x / cvn, col = threadIdx.x - r * cvn, C = cvn * VEC;
    const P* yv = reinterpret_cast<const P*>(y);
    const P* gv = reinterpret_cast<const P*>(gy);
    P* ov = reinterpret_cast<P*>(gx);
    float acc[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
    if (r < rpb) {
        const size_t step = (size_t)gridDim.x * rpb;
        for (size_t p = (size_t)blockIdx.x * rpb + r; p < npix; p += step) {
            const size_t i = p * cvn + col;
            const P a = yv[i];
            P g = gv[i];
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const float gf = to_f32(g.v[k]);
                const float v = to_f32(a.v[k]) > 0.f ? gf : __fmul_rn(gf, slope);
                acc[k] += v;
                g.v[k] = from_f32<T>(v);
            }
            if (ov) ov[i] = g;
        }
#pragma unroll
        for (int k = 0; k < VEC; ++k) cd_sm[r * C + col * VEC + k] = acc[k];
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
        float s = 0.f;
        for (int q = 0; q < rpb; ++q) s += cd_sm[q * C + c];
        parts[(size_t)blockIdx.x * C + c] = s;
    }
}

__global__ __launch_bounds__(256) void bias_parts_reduce_kernel(const float* __restrict__ parts, int nparts, int C, float* __restrict__ gbias) {
    reduce_partials_block(parts, nparts, (size_t)C, C, gbias, [](int e) { return e; });
}

// ---------------------------------------------------------------- adaptive max-pool (+ bias) into embedding rows
__host__ __device__ __forceinline__ int cd_win_start(int o, int64_t in, int64_t out) { return (int)(((int64_t)o * in) / out); }
__host__ __device__ __forceinline__ int cd_win_end(int o, int64_t in, int64_t out) { return (int)((((int64_t)o + 1) * in + out - 1) / out); }

// whether candidate (v2, i2) replaces (v1, i1): the outcome of torch's scan `if (val > max || isnan(val)) take` over the window in
// row-major order, as an order on (value, index) pairs -- so the candidates may be merged in any order: the first of equal maxima, a
// NaN over every number, the last of several NaNs
__device__ __forceinline__ bool cd_better(float v2, int i2, float v1, int i1) {
    if (v2 != v2) return !(v1 != v1) || i2 > i1;
    if (v1 != v1) return false;
    return v2 > v1 || (v2 == v1 && i2 < i1);
}

struct PoolGeo {
    int H, W, C, OH, OW, PH, PW, B;     // B = samples per view
};
// row and first column (dh = dw = 0 plus the in-block offset, channel 0) of pooled element (n, oh, ow) in e [N*PH*PW][C*bh*bw]
__device__ __forceinline__ size_t cd_embed_offset(const PoolGeo& g, int n, int oh, int ow, int& cstride) {
    const int bh = g.OH / g.PH, bw = g.OW / g.PW, ph = oh / bh, pw = ow / bw, dh = oh - ph * bh, dw = ow - pw * bw;
    const int v = n / g.B, b = n - v * g.B;
    const size_t row = ((size_t)v * g.PH * g.PW + (size_t)ph * g.PW + pw) * g.B + b;
    cstride = bh * bw;
    return row * ((size_t)g.C * cstride) + (size_t)dh * bw + dw;
}

// One block per window (n, oh, ow): thread (r, col) scans the window's pixels r, r + rpb, ... (row-major numbering inside the window) for
// its VEC channels, four loads in flight; the rpb candidates of a channel are merged by a tree in LDS (cd_better is an order, so the
// tree's shape does not matter); row 0 writes the values and the indices.
template <typename T, int VEC>
__global__ __launch_bounds__(256) void bias_amaxpool_fwd_kernel(const T* __restrict__ raw, PoolGeo g, const float* __restrict__ bias,
                                                                float* __restrict__ e, int32_t* __restrict__ idx) {
    typedef CdPack<T, VEC> P;
    extern __shared__ float cd_sm[];            // values [rpb][C] | indices [rpb][C]
    const int cvn = g.C / VEC, rpb = 256 / cvn, r = threadIdx.x / cvn, col = threadIdx.x - r * cvn;
    int* sm_i = reinterpret_cast<int*>(cd_sm + (size_t)rpb * g.C);
    const int win = blockIdx.x, ow = win % g.OW, oh = (win / g.OW) % g.OH, n = win / (g.OW * g.OH);
    const int h0 = cd_win_start(oh, g.H, g.OH), h1 = cd_win_end(oh, g.H, g.OH), w0 = cd_win_start(ow, g.W, g.OW), w1 = cd_win_end(ow, g.W, g.OW);
    const int ww = w1 - w0, npx = (h1 - h0) * ww;
    const P* in = reinterpret_cast<const P*>(raw) + (size_t)n * g.H * g.W * cvn + col;
    float m[VEC];
    int mi[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) { m[k] = -INFINITY; mi[k] = h0 * g.W + w0; }
    if (r < rpb) {
        for (int q = r; q < npx; q += 4 * rpb) {
            P p[4];
            int at[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int qq = q + u * rpb, dh = qq / ww;
                at[u] = (h0 + dh) * g.W + w0 + (qq - dh * ww);
                if (qq < npx) p[u] = in[(size_t)at[u] * cvn];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (q + u * rpb >= npx) break;
#pragma unroll
                for (int k = 0; k < VEC; ++k) {
                    const float v = to_f32(p[u].v[k]);
                    if (cd_better(v, at[u], m[k], mi[k])) { m[k] = v; mi[k] = at[u]; }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < VEC; ++k) { cd_sm[r * g.C + col * VEC + k] = m[k]; sm_i[r * g.C + col * VEC + k] = mi[k]; }
    }
    __syncthreads();
    for (int cnt = rpb; cnt > 1;) {
        const int half = (cnt + 1) >> 1;
        if (r < cnt - half) {
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const int a = r * g.C + col * VEC + k, b = (r + half) * g.C + col * VEC + k;
                if (cd_better(cd_sm[b], sm_i[b], cd_sm[a], sm_i[a])) { cd_sm[a] = cd_sm[b]; sm_i[a] = sm_i[b]; }
            }
        }
        __syncthreads();
        cnt = half;
    }
    if (r == 0) {
        int cstride;
        float* dst = e + cd_embed_offset(g, n, oh, ow, cstride);
        int32_t* di = idx + (size_t)win * g.C + col * VEC;
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const int c = col * VEC + k;
            const float v = cd_sm[c];
            dst[(size_t)c * cstride] = bias ? __fadd_rn(v, bias[c]) : v;
        }
#pragma unroll
        for (int k4 = 0; k4 < VEC / 4; ++k4) {
            CdIdx4 o;
#pragma unroll
            for (int k = 0; k < 4; ++k) o.v[k] = sm_i[col * VEC + 4 * k4 + k];
            reinterpret_cast<CdIdx4*>(di)[k4] = o;
        }
    }
}

// graw: a gather per output vector over the windows that contain its pixel -- rows floor(h*OH/H) .. ceil((h+1)*OH/H) - 1 of the window
// grid, columns likewise (two per axis where adjacent windows overlap, more only when the map is smaller than the window grid) -- in
// window order.  Writes every element; no atomics, no workspace.
template <typename T, int VEC>
__global__ __launch_bounds__(256) void bias_amaxpool_bwd_kernel(const float* __restrict__ ge, const int32_t* __restrict__ idx, PoolGeo g, size_t nvec,
                                                                T* __restrict__ graw) {
    typedef CdPack<T, VEC> P;
    const int cvn = g.C / VEC;
    P* out = reinterpret_cast<P*>(graw);
    const size_t stride = (size_t)gridDim.x * 256, HW = (size_t)g.H * g.W;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += stride) {
        const size_t pix = i / cvn;
        const int col = (int)(i - pix * cvn), n = (int)(pix / HW), at = (int)(pix - (size_t)n * HW), h = at / g.W, w = at - h * g.W;
        const int oh_lo = (int)(((int64_t)h * g.OH) / g.H), oh_hi = min(g.OH - 1, (int)((((int64_t)h + 1) * g.OH + g.H - 1) / g.H) - 1);
        const int ow_lo = (int)(((int64_t)w * g.OW) / g.W), ow_hi = min(g.OW - 1, (int)((((int64_t)w + 1) * g.OW + g.W - 1) / g.W) - 1);
        float acc[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
        for (int oh = oh_lo; oh <= oh_hi; ++oh)
            for (int ow = ow_lo; ow <= ow_hi; ++ow) {
                const int32_t* wi = idx + (((size_t)n * g.OH + oh) * g.OW + ow) * g.C + col * VEC;
                int cstride;
                const float* src = ge + cd_embed_offset(g, n, oh, ow, cstride);
#pragma unroll
                for (int k4 = 0; k4 < VEC / 4; ++k4) {
                    const CdIdx4 ix = reinterpret_cast<const CdIdx4*>(wi)[k4];
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (ix.v[k] == at) acc[4 * k4 + k] += src[(size_t)(col * VEC + 4 * k4 + k) * cstride];
                }
            }
        P p;
#pragma unroll
        for (int k = 0; k < VEC; ++k) p.v[k] = from_f32<T>(acc[k]);
        out[i] = p;
    }
}

// gbias[c] = sum over (n, oh, ow) of the channel's ge entries: a block owns 32 channels, its 8 thread rows split the windows, the rows are
// added in order (the arrangement of avgpool_fwd_kernel in contrast.hip)
__global__ __launch_bounds__(256) void amaxpool_gbias_kernel(const float* __restrict__ ge, PoolGeo g, int nwin, float* __restrict__ gbias) {
    __shared__ float part[8][32];
    const int c = blockIdx.x * 32 + (threadIdx.x & 31), row = threadIdx.x >> 5;
    float s = 0.f;
    if (c < g.C)
        for (int win = row; win < nwin; win += 8) {
            const int ow = win % g.OW, oh = (win / g.OW) % g.OH, n = win / (g.OW * g.OH);
            int cstride;
            const float* src = ge + cd_embed_offset(g, n, oh, ow, cstride);
            s += src[(size_t)c * cstride];
        }
    part[row][threadIdx.x & 31] = s;
    __syncthreads();
    if (row == 0 && c < g.C) {
        float t = 0.f;
#pragma unroll
        for (int q = 0; q < 8; ++q) t += part[q][threadIdx.x];
        gbias[c] = t;
    }
}

// the vector width of a call: 16 bytes where C allows, else 8 (16-bit types with C % 8 != 0)
static inline int cd_vec(int dt, int64_t C) { return dt == MISEG_F32 ? 4 : (C % 8 == 0 ? 8 : 4); }

}  // namespace miseg

using namespace miseg;

// LAUNCH(type, elements per vector): float in 16-byte vectors, a 16-bit type in 16-byte vectors where C allows (cd_vec)
#define CD_DISPATCH(dt, who, C, LAUNCH)                                      \
    MISEG_WITH_STORAGE_TYPE(dt, who,                                         \
        if constexpr (sizeof(TT) == 4) { LAUNCH(TT, 4); }                    \
        else if (C % 8 == 0) { LAUNCH(TT, 8); }                              \
        else { LAUNCH(TT, 4); })

#define CD_SHAPE_CHECKS(what)                                                                                                           \
    MISEG_REQUIRE(dt == MISEG_F32 || dt == MISEG_BF16, what ": unknown dt");                                                           \
    MISEG_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0 && C <= kCdMaxC, what ": bad shape (C must be a multiple of 4, at most %d)", kCdMaxC); \
    MISEG_REQUIRE(H < (1ll << 31) && W < (1ll << 31) && H * W < (1ll << 31) && N < (1ll << 31), what ": H*W and N must stay below 2^31")

extern "C" int miseg_bias_lrelu_fwd(void* stream, int dt, const void* raw, int64_t N, int64_t H, int64_t W, int64_t C, const float* bias,
                                    float slope, void* y) {
    MISEG_TAPE(miseg_bias_lrelu_fwd, stream, dt, raw, N, H, W, C, bias, slope, y);
    MISEG_F16_DISPATCH_ON(dt, miseg_bias_lrelu_fwd, stream, MISEG_BF16, raw, N, H, W, C, bias, slope, y);
    MISEG_REQUIRE(raw && bias && y, "bias_lrelu_fwd: null pointer");
    CD_SHAPE_CHECKS("bias_lrelu_fwd");
    const int vec = cd_vec(dt, C), cvn = (int)(C / vec);
    MISEG_REQUIRE(((uintptr_t)raw & 15) == 0 && ((uintptr_t)y & 15) == 0, "bias_lrelu_fwd: tensors must be 16-byte aligned");
    const size_t nvec = (size_t)N * H * W * cvn;
    const unsigned grid = (unsigned)std::min<int64_t>(cdiv((int64_t)nvec, 256), kCdMaxBlocks);
    hipStream_t st = as_stream(stream);
#define L(TT, VV) hipLaunchKernelGGL((bias_lrelu_fwd_kernel<TT, VV>), dim3(grid), dim3(256), 0, st, (const TT*)raw, nvec, cvn, bias, slope, (TT*)y)
    CD_DISPATCH(dt, "bias_lrelu_fwd", C, L);
#undef L
    MISEG_LAUNCH_CHECK("bias_lrelu_fwd_kernel");
    return MISEG_OK;
}

extern "C" int64_t miseg_bias_lrelu_bwd_ws_bytes(int dt, int64_t N, int64_t H, int64_t W, int64_t C) {
    if (!(dt == MISEG_F32 || dt == MISEG_BF16 || dt == MISEG_F16) || N <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 4 != 0 || C > kCdMaxC) return -1;
    const int cvn = (int)(C / cd_vec(dt, C));
    return cd_lrelu_bwd_blocks(N * H * W, cvn) * C * 4;
}

extern "C" int miseg_bias_lrelu_bwd(void* stream, int dt, const void* y, const void* gy, int64_t N, int64_t H, int64_t W, int64_t C, float slope,
                                    void* gx, float* gbias, void* ws, int64_t ws_bytes) {
    MISEG_TAPE(miseg_bias_lrelu_bwd, stream, dt, y, gy, N, H, W, C, slope, gx, gbias, ws, ws_bytes);
    MISEG_F16_DISPATCH_ON(dt, miseg_bias_lrelu_bwd, stream, MISEG_BF16, y, gy, N, H, W, C, slope, gx, gbias, ws, ws_bytes);
    MISEG_REQUIRE(y && gy && gbias && ws, "bias_lrelu_bwd: null pointer");
    CD_SHAPE_CHECKS("bias_lrelu_bwd");
    const int vec = cd_vec(dt, C), cvn = (int)(C / vec), rpb = cd_rows_per_block(cvn);
    MISEG_REQUIRE(((uintptr_t)y & 15) == 0 && ((uintptr_t)gy & 15) == 0 && ((uintptr_t)gx & 15) == 0 && ((uintptr_t)ws & 15) == 0,
                  "bias_lrelu_bwd: tensors and workspace must be 16-byte aligned");
    const size_t npix = (size_t)N * H * W;
    const int nblocks = (int)cd_lrelu_bwd_blocks((int64_t)npix, cvn);
    MISEG_REQUIRE(ws_bytes >= (int64_t)nblocks * C * 4, "bias_lrelu_bwd: workspace too small (miseg_bias_lrelu_bwd_ws_bytes)");
    hipStream_t st = as_stream(stream);
    float* parts = (float*)ws;
    const size_t lds = (size_t)rpb * C * 4;
#define L(TT, VV) hipLaunchKernelGGL((bias_lrelu_bwd_kernel<TT, VV>), dim3(nblocks), dim3(256), lds, st, (const TT*)y, (const TT*)gy, npix, cvn, slope, (TT*)gx, parts)
    CD_DISPATCH(dt, "bias_lrelu_bwd", C, L);
#undef L
    MISEG_LAUNCH_CHECK("bias_lrelu_bwd_kernel");
    hipLaunchKernelGGL(bias_parts_reduce_kernel, dim3(reduce_grid(C, nblocks)), dim3(256), 0, st, (const float*)parts, nblocks, (int)C, gbias);
    MISEG_LAUNCH_CHECK("bias_parts_reduce_kernel");
    return MISEG_OK;
}

#define CD_POOL_CHECKS(what)                                                                                                            \
    CD_SHAPE_CHECKS(what);                                                                                                              \
    MISEG_REQUIRE(OH > 0 && OW > 0 && PH > 0 && PW > 0 && V > 0, what ": output, partition and view counts must be positive");           \
    MISEG_REQUIRE(OH % PH == 0 && OW % PW == 0, what ": the output size (%lld, %lld) is not a multiple of the partition (%lld, %lld)",    \
                  (long long)OH, (long long)OW, (long long)PH, (long long)PW);                                                           \
    MISEG_REQUIRE(N % V == 0, what ": N = %lld samples are not V = %lld views of a batch", (long long)N, (long long)V);                  \
    MISEG_REQUIRE(OH < (1ll << 31) && OW < (1ll << 31) && N * OH < (1ll << 31) && N * OH * OW < (1ll << 31), what ": N*OH*OW must stay below 2^31")

extern "C" int miseg_bias_amaxpool_fwd(void* stream, int dt, const void* raw, int64_t N, int64_t H, int64_t W, int64_t C, const float* bias,
                                       int64_t OH, int64_t OW, int64_t PH, int64_t PW, int64_t V, float* e, int32_t* idx) {
    MISEG_TAPE(miseg_bias_amaxpool_fwd, stream, dt, raw, N, H, W, C, bias, OH, OW, PH, PW, V, e, idx);
    MISEG_F16_DISPATCH_ON(dt, miseg_bias_amaxpool_fwd, stream, MISEG_BF16, raw, N, H, W, C, bias, OH, OW, PH, PW, V, e, idx);
    MISEG_REQUIRE(raw && e && idx, "bias_amaxpool_fwd: null pointer");
    CD_POOL_CHECKS("bias_amaxpool_fwd");
    MISEG_REQUIRE(((uintptr_t)raw & 15) == 0 && ((uintptr_t)idx & 15) == 0, "bias_amaxpool_fwd: raw and idx must be 16-byte aligned");
    const int vec = cd_vec(dt, C), cvn = (int)(C / vec), rpb = cd_rows_per_block(cvn);
    const PoolGeo g{(int)H, (int)W, (int)C, (int)OH, (int)OW, (int)PH, (int)PW, (int)(N / V)};
    const size_t lds = (size_t)rpb * C * 8;
    const unsigned grid = (unsigned)(N * OH * OW);
    hipStream_t st = as_stream(stream);
#define L(TT, VV) hipLaunchKernelGGL((bias_amaxpool_fwd_kernel<TT, VV>), dim3(grid), dim3(256), lds, st, (const TT*)raw, g, bias, e, idx)
    CD_DISPATCH(dt, "bias_amaxpool_fwd", C, L);
#undef L
    MISEG_LAUNCH_CHECK("bias_amaxpool_fwd_kernel");
    return MISEG_OK;
}

extern "C" int miseg_bias_amaxpool_bwd(void* stream, int dt, const float* ge, const int32_t* idx, int64_t N, int64_t H, int64_t W, int64_t C,
                                       int64_t OH, int64_t OW, int64_t PH, int64_t PW, int64_t V, void* graw, float* gbias) {
    MISEG_TAPE(miseg_bias_amaxpool_bwd, stream, dt, ge, idx, N, H, W, C, OH, OW, PH, PW, V, graw, gbias);
    MISEG_F16_DISPATCH_ON(dt, miseg_bias_amaxpool_bwd, stream, MISEG_BF16, ge, idx, N, H, W, C, OH, OW, PH, PW, V, graw, gbias);
    MISEG_REQUIRE(ge && idx && graw, "bias_amaxpool_bwd: null pointer");
    CD_POOL_CHECKS("bias_amaxpool_bwd");
    MISEG_REQUIRE(((uintptr_t)graw & 15) == 0 && ((uintptr_t)idx & 15) == 0, "bias_amaxpool_bwd: graw and idx must be 16-byte aligned");
    const int vec = cd_vec(dt, C), cvn = (int)(C / vec);
    const PoolGeo g{(int)H, (int)W, (int)C, (int)OH, (int)OW, (int)PH, (int)PW, (int)(N / V)};
    const size_t nvec = (size_t)N * H * W * cvn;
    const unsigned grid = (unsigned)std::min<int64_t>(cdiv((int64_t)nvec, 256), 4 * kCdMaxBlocks);
    hipStream_t st = as_stream(stream);
#define L(TT, VV) hipLaunchKernelGGL((bias_amaxpool_bwd_kernel<TT, VV>), dim3(grid), dim3(256), 0, st, ge, idx, g, nvec, (TT*)graw)
    CD_DISPATCH(dt, "bias_amaxpool_bwd", C, L);
#undef L
    MISEG_LAUNCH_CHECK("bias_amaxpool_bwd_kernel");
    if (gbias) {
        hipLaunchKernelGGL(amaxpool_gbias_kernel, dim3((unsigned)cdiv(C, 32)), dim3(256), 0, st, ge, g, (int)(N * OH * OW), gbias);
        MISEG_LAUNCH_CHECK("amaxpool_gbias_kernel");
    }
    return MISEG_OK;
}
