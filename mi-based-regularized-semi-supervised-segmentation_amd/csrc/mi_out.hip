// Local (displacement-window) IIC mutual information on the NETWORK OUTPUT: the `midl` trainer's regulariser.
// ref: contrastyou/losses/iic_loss.py:107-149 (IIDSegmentationLoss), :152-189 (patch_generator / IIDSegmentationSmallPathLoss),
//      applied as IIDSegmentationSmallPathLoss(softmax(flip(unlabeled_logits)), softmax(unlabeled_tf_logits)).
//
// The generic local-MI kernels (mi_local.hip) read materialised NCHW probability planes.  Here the operands are the U-Net's own fp32
// NHWC logits with C = num_classes (2..8) channels: both softmaxes are computed in registers from the logits (never written), the
// per-sample flip of the `b` side is index math, and the backward ends in the softmax backward, so the gradient lands on the logits.
//
//   joint (forward): raw[p][a][b][i][j] = sum_{n, (h,w) in window p} Xpad_p[n,i,h+a,w+b] * Y[n,j,h,w]
//                    X = softmax(flip(b)), Y = softmax(a), Xpad_p = window p cropped and zero-padded by `pad` -- the layout
//                    miseg_iic_local_loss_fwd(_ws) consumes (the loss and grad_raw come from that epilogue unchanged).
//                    Deterministic: every block writes its partial sums to the workspace, a second kernel adds them in a fixed order.
//   backward       : per pixel, summed over the windows that contain it, G_p = grad_raw[p] * scale[p]:
//                    dY[j] = sum_{a,b,i} G_p[a][b][i][j] * Xwin_p[i](h+a-pad, w+b-pad)
//                    dX[i] = sum_{a,b,j} G_p[a][b][i][j] * Ywin_p[j](h-a+pad, w-b+pad)      (zero outside window p)
//                    then the softmax backward on both sides; ga at (h,w) (optionally added to what is there: the consistency
//                    gradient), gb at flip(h,w).  Every pixel is written exactly once: plain stores, no atomics.
// All arithmetic fp32 on the VALU: at C = 4, pad = 1 a pixel costs ~300 FMA each way, far below the HBM time of its logits.
#include "pixel_loss.h"

namespace miseg {

namespace {

constexpr int kOT = 256;                 // threads per block
constexpr int kTile = 16;                // 16 x 16 pixel tiles
constexpr int kMaxPad = 3;
constexpr int kMaxHS = kTile + 2 * kMaxPad;

// the window of entry p, clamped to the image (a window list from elsewhere is trusted for its values, never for memory safety)
__device__ __forceinline__ void load_window(const int32_t* __restrict__ win, int p, int H, int W, int& h0, int& h1, int& w0, int& w1) {
    h0 = max(0, win[4 * p + 0]);
    h1 = min(H, win[4 * p + 1]);
    w0 = max(0, win[4 * p + 2]);
    w1 = min(W, win[4 * p + 3]);
    if (h1 < h0) h1 = h0;
    if (w1 < w0) w1 = w0;
}

// softmax of the logits row of pixel (n, h, w) of an NHWC [N,H,W,C] tensor into p[C]
template <int C>
__device__ __forceinline__ void softmax_at(const float* __restrict__ z, int64_t pix, float* p) {
    float v[C];
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = z[pix * C + c];
    softmax_c(v, C, p);
}

// ---------------------------------------------------------------------------------------------------------------- forward
// grid (B, P): block b of window p handles the (sample, tile) items b, b + B, ... of that window.  ws[p][b][E], E = T*T*C*C.
template <int C>
__global__ __launch_bounds__(kOT) void out_joint_partial_kernel(const float* __restrict__ a, const float* __restrict__ bl,
                                                                const int32_t* __restrict__ flips, int N, int H, int W, int pad,
                                                                const int32_t* __restrict__ win, float* __restrict__ ws) {
    __shared__ float sY[kTile * kTile * C];
    __shared__ float sX[kMaxHS * kMaxHS * C];
    const int p = blockIdx.y, B = gridDim.x, tid = threadIdx.x;
    const int T = 2 * pad + 1, HS = kTile + 2 * pad, R = T * T * C;
    int h0, h1, w0, w1;
    load_window(win, p, H, W, h0, h1, w0, w1);
    const int wh = h1 - h0, ww = w1 - w0;
    const int ty = (wh + kTile - 1) / kTile, tx = (ww + kTile - 1) / kTile;
    const int64_t items = (int64_t)N * ty * tx;
    // row r = (a * T + b) * C + i of the joint; rows of this thread: r0 and r0 + 256 (R <= 7 * 7 * 8 = 392)
    const int npg = R < kOT ? kOT / R : 1;          // pixel groups sharing the tile when the rows do not fill the block
    const int g = R < kOT ? tid / R : 0;
    const int r0 = R < kOT ? tid % R : tid;
    const bool act0 = g < npg && r0 < R, act1 = R > kOT && r0 + kOT < R;
    int ra[2], rb[2], ri[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int r = r0 + k * kOT;
        ri[k] = r % C;
        rb[k] = (r / C) % T;
        ra[k] = r / (C * T);
    }
    float acc[2][C];
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int j = 0; j < C; ++j) acc[k][j] = 0.f;
    for (int64_t it = blockIdx.x; it < items; it += B) {
        const int n = (int)(it / ((int64_t)ty * tx));
        const int t = (int)(it % ((int64_t)ty * tx));
        const int oh = (t / tx) * kTile, ow = (t % tx) * kTile;           // tile origin in window coordinates
        const int f = flips ? flips[n] : 0;
        {   // Y tile: softmax(a) at the tile's pixels, zero outside the window
            const int qy = tid / kTile, qx = tid % kTile;
            const int lh = oh + qy, lw = ow + qx;
            float y[C];
            if (lh < wh && lw < ww) {
                softmax_at<C>(a, ((int64_t)n * H + (h0 + lh)) * W + (w0 + lw), y);
            } else {
#pragma unroll
                for (int c = 0; c < C; ++c) y[c] = 0.f;
            }
#pragma unroll
            for (int c = 0; c < C; ++c) sY[tid * C + c] = y[c];
        }
        for (int q = tid; q < HS * HS; q += kOT) {   // X halo: softmax(flip(b)), zero outside the window (the crop's zero padding)
            const int lh = oh + q / HS - pad, lw = ow + q % HS - pad;
            float x[C];
            if (lh >= 0 && lh < wh && lw >= 0 && lw < ww) {
                const int h = h0 + lh, w = w0 + lw;
                softmax_at<C>(bl, ((int64_t)n * H + flip_h(h, H, f)) * W + flip_w(w, W, f), x);
            } else {
#pragma unroll
                for (int c = 0; c < C; ++c) x[c] = 0.f;
            }
#pragma unroll
            for (int c = 0; c < C; ++c) sX[q * C + c] = x[c];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (k == 0 ? act0 : act1) {
                for (int q = g; q < kTile * kTile; q += npg) {
                    const int qy = q / kTile, qx = q % kTile;
                    const float xv = sX[((qy + ra[k]) * HS + qx + rb[k]) * C + ri[k]];
#pragma unroll
                    for (int j = 0; j < C; ++j) acc[k][j] = fmaf(xv, sY[q * C + j], acc[k][j]);
                }
            }
        }
        __syncthreads();
    }
    // pixel groups -> one partial per row, in group order
    const int E = R * C;
    float* out = ws + ((int64_t)p * B + blockIdx.x) * E;
    if (npg == 1) {
#pragma unroll
        for (int k = 0; k < 2; ++k)
            if (k == 0 ? act0 : act1)
#pragma unroll
                for (int j = 0; j < C; ++j) out[(r0 + k * kOT) * C + j] = acc[k][j];
        return;
    }
    float* red = sX;          // npg * R * C <= 256 * C floats
    if (act0)
#pragma unroll
        for (int j = 0; j < C; ++j) red[(g * R + r0) * C + j] = acc[0][j];
    __syncthreads();
    for (int e = tid; e < E; e += kOT) {
        float s = 0.f;
        for (int gg = 0; gg < npg; ++gg) s += red[gg * E + e];
        out[e] = s;
    }
}

// raw[p][e] = sum over the B partials of window p: one block per entry, thread t adds partials t, t + 256, ... in order, then a
// fixed-order block reduction (one thread walking all B partials serially was latency-bound: ~0.2 ms for B = 1024 at cfg2)
__global__ __launch_bounds__(kOT) void out_joint_reduce_kernel(const float* __restrict__ ws, int B, int E, float* __restrict__ raw) {
    __shared__ float red[17];
    const int p = blockIdx.y, e = blockIdx.x;
    const float* src = ws + (int64_t)p * B * E + e;
    float s = 0.f;
    for (int b = threadIdx.x; b < B; b += kOT) s += src[(int64_t)b * E];
    s = block_sum(s, red);
    if (threadIdx.x == 0) raw[(int64_t)p * E + e] = s;
}

// ---------------------------------------------------------------------------------------------------------------- backward
// grid (tiles of the image, N): one thread per pixel.  X and Y softmaxes of the tile and its halo in LDS (no window masking there:
// the window bounds are tested per neighbour), G_p = grad_raw[p] * scale[p] of one window at a time in LDS.
template <int C>
__global__ __launch_bounds__(kOT) void out_bwd_kernel(const float* __restrict__ a, const float* __restrict__ bl,
                                                      const int32_t* __restrict__ flips, int H, int W, int pad,
                                                      const int32_t* __restrict__ win, int P, const float* __restrict__ grad_raw,
                                                      const float* __restrict__ scale, float* __restrict__ ga, float* __restrict__ gb,
                                                      int accumulate) {
    __shared__ float sX[kMaxHS * kMaxHS * C];
    __shared__ float sY[kMaxHS * kMaxHS * C];
    __shared__ float sG[(2 * kMaxPad + 1) * (2 * kMaxPad + 1) * C * C];
    const int tid = threadIdx.x, n = blockIdx.y;
    const int T = 2 * pad + 1, HS = kTile + 2 * pad, E = T * T * C * C;
    const int tilesx = (W + kTile - 1) / kTile;
    const int oh = (blockIdx.x / tilesx) * kTile, ow = (blockIdx.x % tilesx) * kTile;
    const int f = flips ? flips[n] : 0;
    for (int q = tid; q < HS * HS; q += kOT) {
        const int h = oh + q / HS - pad, w = ow + q % HS - pad;
        float x[C], y[C];
        if (h >= 0 && h < H && w >= 0 && w < W) {
            softmax_at<C>(a, ((int64_t)n * H + h) * W + w, y);
            softmax_at<C>(bl, ((int64_t)n * H + flip_h(h, H, f)) * W + flip_w(w, W, f), x);
        } else {
#pragma unroll
            for (int c = 0; c < C; ++c) x[c] = y[c] = 0.f;
        }
#pragma unroll
        for (int c = 0; c < C; ++c) {
            sX[q * C + c] = x[c];
            sY[q * C + c] = y[c];
        }
    }
    const int ty = tid / kTile, tx = tid % kTile;
    const int h = oh + ty, w = ow + tx;
    float dX[C], dY[C];
#pragma unroll
    for (int c = 0; c < C; ++c) dX[c] = dY[c] = 0.f;
    for (int p = 0; p < P; ++p) {
        int h0, h1, w0, w1;
        load_window(win, p, H, W, h0, h1, w0, w1);
        if (h1 <= oh || h0 >= oh + kTile || w1 <= ow || w0 >= ow + kTile) continue;      // uniform: the window misses this tile
        __syncthreads();                              // the previous window's G (and, first time round, the halo) is complete
        const float sc = scale[p];
        for (int e = tid; e < E; e += kOT) sG[e] = grad_raw[(int64_t)p * E + e] * sc;
        __syncthreads();
        if (h >= h0 && h < h1 && w >= w0 && w < w1) {
            for (int da = 0; da < T; ++da) {
                for (int db = 0; db < T; ++db) {
                    const float* G = sG + (da * T + db) * C * C;       // G[i][j]
                    const int xh = h + da - pad, xw = w + db - pad;    // X neighbour feeding dY
                    if (xh >= h0 && xh < h1 && xw >= w0 && xw < w1) {
                        const float* xv = sX + ((ty + da) * HS + tx + db) * C;
#pragma unroll
                        for (int i = 0; i < C; ++i) {
                            const float xi = xv[i];
#pragma unroll
                            for (int j = 0; j < C; ++j) dY[j] = fmaf(G[i * C + j], xi, dY[j]);
                        }
                    }
                    const int yh = h - da + pad, yw = w - db + pad;    // Y neighbour feeding dX
                    if (yh >= h0 && yh < h1 && yw >= w0 && yw < w1) {
                        const float* yv = sY + ((ty - da + 2 * pad) * HS + tx - db + 2 * pad) * C;
#pragma unroll
                        for (int i = 0; i < C; ++i) {
                            float s = dX[i];
#pragma unroll
                            for (int j = 0; j < C; ++j) s = fmaf(G[i * C + j], yv[j], s);
                            dX[i] = s;
                        }
                    }
                }
            }
        }
    }
    __syncthreads();
    if (h >= H || w >= W) return;
    const float* xs = sX + ((ty + pad) * HS + tx + pad) * C;
    const float* ys = sY + ((ty + pad) * HS + tx + pad) * C;
    float dotx = 0.f, doty = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        dotx = fmaf(xs[c], dX[c], dotx);
        doty = fmaf(ys[c], dY[c], doty);
    }
    const int64_t ia = (((int64_t)n * H + h) * W + w) * C;
    const int64_t ib = (((int64_t)n * H + flip_h(h, H, f)) * W + flip_w(w, W, f)) * C;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float va = ys[c] * (dY[c] - doty);
        ga[ia + c] = accumulate ? ga[ia + c] + va : va;
        gb[ib + c] = xs[c] * (dX[c] - dotx);
    }
}

bool out_supported(int64_t C, int64_t pad) { return C >= 2 && C <= 8 && pad >= 0 && pad <= kMaxPad; }

int64_t out_blocks(int64_t N, int64_t H, int64_t W, int64_t P) {
    const int64_t most = N * cdiv(H, kTile) * cdiv(W, kTile);      // (sample, tile) items of the largest possible window
    return std::max<int64_t>(1, std::min<int64_t>(most, cdiv(1024, P)));
}

}  // namespace

}  // namespace miseg

using namespace miseg;

#define MISEG_OUT_DISPATCH(C, MACRO)                                                                    \
    switch (C) {                                                                                        \
        case 2: MACRO(2); break;                                                                        \
        case 3: MACRO(3); break;                                                                        \
        case 4: MACRO(4); break;                                                                        \
        case 5: MACRO(5); break;                                                                        \
        case 6: MACRO(6); break;                                                                        \
        case 7: MACRO(7); break;                                                                        \
        case 8: MACRO(8); break;                                                                        \
        default: return fail(MISEG_E_INVALID, "iic_out: unsupported configuration (C = %ld, 2..8)", (long)C); \
    }

extern "C" int64_t miseg_iic_out_joint_ws_bytes(int64_t N, int64_t C, int64_t H, int64_t W, int64_t pad, int64_t P) {
    if (N <= 0 || H <= 0 || W <= 0 || P <= 0 || !out_supported(C, pad)) return -1;
    const int64_t T = 2 * pad + 1;
    return out_blocks(N, H, W, P) * P * T * T * C * C * 4;
}

extern "C" int miseg_iic_out_joint_fwd(void* stream, const float* a, const float* b, const int32_t* flips, int64_t N, int64_t C,
                                       int64_t H, int64_t W, int64_t pad, const int32_t* win, int64_t P, float* raw, void* ws,
                                       int64_t ws_bytes) {
    MISEG_TAPE(miseg_iic_out_joint_fwd, stream, a, b, flips, N, C, H, W, pad, win, P, raw, ws, ws_bytes);
    MISEG_REQUIRE(out_supported(C, pad), "iic_out_joint_fwd: unsupported configuration (C = %ld in 2..8, pad = %ld in 0..3)", (long)C,
                  (long)pad);
    MISEG_REQUIRE(a && b && win && raw && ws, "iic_out_joint_fwd: null pointer");
    MISEG_REQUIRE(N > 0 && H > 0 && W > 0 && P > 0 && N < (1 << 30) && H < (1 << 20) && W < (1 << 20) && P < 65536,
                  "iic_out_joint_fwd: bad shape");
    MISEG_REQUIRE(ws_bytes >= miseg_iic_out_joint_ws_bytes(N, C, H, W, pad, P), "iic_out_joint_fwd: workspace too small");
    const int64_t B = out_blocks(N, H, W, P), T = 2 * pad + 1, E = T * T * C * C;
    hipStream_t st = as_stream(stream);
#define L(CC) hipLaunchKernelGGL(out_joint_partial_kernel<CC>, dim3((unsigned)B, (unsigned)P), dim3(kOT), 0, st, a, b, flips, (int)N, \
                                 (int)H, (int)W, (int)pad, win, (float*)ws)
    MISEG_OUT_DISPATCH(C, L)
#undef L
    MISEG_LAUNCH_CHECK("out_joint_partial_kernel");
    hipLaunchKernelGGL(out_joint_reduce_kernel, dim3((unsigned)E, (unsigned)P), dim3(kOT), 0, st, (const float*)ws, (int)B,
                       (int)E, raw);
    MISEG_LAUNCH_CHECK("out_joint_reduce_kernel");
    return MISEG_OK;
}

extern "C" int miseg_iic_out_bwd(void* stream, const float* a, const float* b, const int32_t* flips, int64_t N, int64_t C, int64_t H,
                                 int64_t W, int64_t pad, const int32_t* win, int64_t P, const float* grad_raw, const float* scale,
                                 float* ga, float* gb, int accumulate) {
    MISEG_TAPE(miseg_iic_out_bwd, stream, a, b, flips, N, C, H, W, pad, win, P, grad_raw, scale, ga, gb, accumulate);
    MISEG_REQUIRE(out_supported(C, pad), "iic_out_bwd: unsupported configuration (C = %ld in 2..8, pad = %ld in 0..3)", (long)C,
                  (long)pad);
    MISEG_REQUIRE(a && b && win && grad_raw && scale && ga && gb, "iic_out_bwd: null pointer");
    MISEG_REQUIRE(N > 0 && H > 0 && W > 0 && P > 0 && N < 65536 && H < (1 << 20) && W < (1 << 20) && P < (1 << 24),
                  "iic_out_bwd: bad shape");
    const int64_t tiles = cdiv(H, kTile) * cdiv(W, kTile);
    MISEG_REQUIRE(tiles < (1LL << 31), "iic_out_bwd: image too large");
    hipStream_t st = as_stream(stream);
#define L(CC) hipLaunchKernelGGL(out_bwd_kernel<CC>, dim3((unsigned)tiles, (unsigned)N), dim3(kOT), 0, st, a, b, flips, (int)H, (int)W, \
                                 (int)pad, win, (int)P, grad_raw, scale, ga, gb, accumulate)
    MISEG_OUT_DISPATCH(C, L)
#undef L
    MISEG_LAUNCH_CHECK("out_bwd_kernel");
    return MISEG_OK;
}
