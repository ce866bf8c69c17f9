// Weight gradients of the 3x3 convolutions: three kernels, their reduction and entry points (conv.h has the file map).
#include "conv.h"

namespace miseg {

// ------------------------------------------------------------------------------------------ wgrad
// gw[co][ci][ky][kx] = sum_{n,h,w} gout[n,h,w,co] * in[n,h+ky-1,w+kx-1,ci]   (fp32 MFMA, split over pixels)
// block = (co tile 32, ci chunk 32, split); wave = 2 of the tile's 8 rows; acc 2 x 18 tiles.
constexpr int WG_TH = 8, WG_TW = 32, WG_P = 34;  // tile rows / cols, LDS channel stride (32 + 2)

// BNL (all three weight-gradient kernels): `gout` is the layer's raw convolution output and bl.gy the gradient of its activation; the
// loader forms graw (common.h, bn_graw_vec) -- positions outside the image stay zero.
template <typename T, bool BNL = false>
__global__ __launch_bounds__(kCT, 1) void conv3x3_wgrad_kernel(ConvSrc src, int N, int H, int W, const T* __restrict__ gout, int Cout,
                                                              int nsplit, float* __restrict__ partials, BnLoad bl) {
    extern __shared__ __attribute__((aligned(16))) float wsm[];
    float* Gs = wsm;                                   // [WG_TH*WG_TW][WG_P]
    float* Is = wsm + WG_TH * WG_TW * WG_P;            // [(WG_TH+2)*(WG_TW+2)][WG_P]
    const int Cin = src.C0 + src.C1;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l15 = lane & 15, kq = lane >> 4;
    const int split = blockIdx.x, ci0 = blockIdx.y * 32, co0 = blockIdx.z * 32;
    const int tilesC = (W + WG_TW - 1) / WG_TW, tilesR = (H + WG_TH - 1) / WG_TH;
    const int ntiles = N * tilesR * tilesC;
    constexpr int IW = WG_TW + 2;
    f32x4 acc[2][18];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 18; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    float bc[kBwdCoefRows] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};       // BNL: this thread's channel (tid & 31) in every element it loads
    if (BNL && co0 + (tid & 31) < Cout)
#pragma unroll
        for (int r = 0; r < kBwdCoefRows; ++r) bc[r] = bl.coef[(size_t)r * Cout + co0 + (tid & 31)];

    for (int tile = split; tile < ntiles; tile += nsplit) {
        const int tc = tile % tilesC, tr = (tile / tilesC) % tilesR, n = tile / (tilesC * tilesR);
        const int h0 = tr * WG_TH, w0 = tc * WG_TW;
        __syncthreads();
        for (int idx = tid; idx < WG_TH * WG_TW * 32; idx += kCT) {
            const int c = idx & 31, px = idx >> 5, ix = px % WG_TW, iy = px / WG_TW;
            const int h = h0 + iy, w = w0 + ix;
            float v = 0.f;
            if (h < H && w < W && co0 + c < Cout) {
                const size_t o = (((size_t)n * H + h) * W + w) * Cout + co0 + c;
                v = to_f32(gout[o]);
                if (BNL) {
                    const float g = to_f32(reinterpret_cast<const T*>(bl.gy)[o]);
                    const float lin = bc[4] + bc[5] * (v - bc[2]);
                    v = v * bc[0] + bc[1] > relu_keep_threshold<T>() ? bc[3] * g + lin : lin;
                }
            }
            Gs[px * WG_P + c] = v;
        }
        for (int idx = tid; idx < (WG_TH + 2) * IW * 32; idx += kCT) {
            const int c = idx & 31, px = idx >> 5, ix = px % IW, iy = px / IW;
            const int h = h0 - 1 + iy, w = w0 - 1 + ix, cc = ci0 + c;
            float v = 0.f;
            if (h >= 0 && h < H && w >= 0 && w < W && cc < Cin) {
                if (cc < src.C0) {
                    const int hs = H >> src.ups0, wsz = W >> src.ups0;
                    v = to_f32(reinterpret_cast<const T*>(src.p0)[(((size_t)n * hs + (h >> src.ups0)) * wsz + (w >> src.ups0)) * src.C0 + cc]);
                } else {
                    const int hs = H >> src.ups1, wsz = W >> src.ups1;
                    v = to_f32(reinterpret_cast<const T*>(src.p1)[(((size_t)n * hs + (h >> src.ups1)) * wsz + (w >> src.ups1)) * src.C1 + cc - src.C0]);
                }
            }
            Is[px * WG_P + c] = v;
        }
        __syncthreads();
#pragma unroll 1
        for (int rr = 0; rr < 2; ++rr) {
            const int row = wv * 2 + rr;
#pragma unroll 1
            for (int cs = 0; cs < WG_TW; cs += 4) {
                const float a0 = Gs[(row * WG_TW + cs + kq) * WG_P + l15];
                const float a1 = Gs[(row * WG_TW + cs + kq) * WG_P + 16 + l15];
#pragma unroll
                for (int tap = 0; tap < 9; ++tap) {
                    const int ky = tap / 3, kx = tap % 3;
                    const float* ip = Is + ((row + ky) * IW + cs + kq + kx) * WG_P + l15;
                    const float b0 = ip[0], b1 = ip[16];
                    acc[0][tap * 2 + 0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][tap * 2 + 0], 0, 0, 0);
                    acc[0][tap * 2 + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][tap * 2 + 1], 0, 0, 0);
                    acc[1][tap * 2 + 0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][tap * 2 + 0], 0, 0, 0);
                    acc[1][tap * 2 + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][tap * 2 + 1], 0, 0, 0);
                }
            }
        }
    }
    // reduce the 4 waves in LDS (fixed order), write partial [split][co 32][tap 9][ci 32]
    float* Ds = wsm;  // 32 x 288 floats
    for (int w = 0; w < 4; ++w) {
        __syncthreads();
        if (wv == w) {
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 18; ++b)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int co = a * 16 + kq * 4 + r, col = (b / 2) * 32 + (b % 2) * 16 + l15;
                        if (w == 0) Ds[co * 288 + col] = acc[a][b][r];
                        else Ds[co * 288 + col] += acc[a][b][r];
                    }
        }
    }
    __syncthreads();
    float* outp = partials + (((size_t)split * gridDim.z + blockIdx.z) * gridDim.y + blockIdx.y) * (32 * 288);
    for (int e = tid; e < 32 * 288; e += kCT) outp[e] = Ds[e];
}

// bf16 variant: both operands need 8 consecutive PIXELS per lane for a fixed channel, while NHWC keeps channels
// contiguous -> the LDS tiles stay in their natural [pixel][16 channels] shape (32-byte rows: the 8 rows a 32-lane
// half touches tile the 64 banks exactly) and fragments come out of ds_read_b64_tr_b16 (hardware 4x16 transpose):
// lane 4q+p of a 16-lane group supplies (pixel 8g+q, channels 4p..4p+3) and receives its channel's 4 pixels.
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
#define LDS_S16X4(ptr) ((__attribute__((address_space(3))) s16x4*)(ptr))

// The same for a 32-pixel k-step of v_mfma_f32_16x16x32_bf16 with the k <-> pixel map  k = 8 kq + e  <->  pixel 16 (e >> 2) + 4 kq + (e & 3)
// (any bijection does, A and B share it): per transpose read the two lane groups of a half-wave (kq = 0, 1 or 2, 3) cover 8
// CONSECUTIVE pixels x 32 B = every bank once.  With pixel = 8 kq + e they read pixels 0-3 and 8-11, 256 B apart: a 2-way conflict
// on every read (38 % of conv3x3_wgrad_bf16_c16_kernel's LDS cycles, profiles/r02_pmc.json).
__device__ __forceinline__ bf16x8_t tr_frag32(const short* row_px0, int kq, int q, int p) {
    s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_S16X4(row_px0 + (4 * kq + q) * 16 + 4 * p));
    s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_S16X4(row_px0 + (16 + 4 * kq + q) * 16 + 4 * p));
    s16x8 f = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8_t, f);
}

__device__ __forceinline__ bf16x8_t tr_frag(const short* blk_px0, int q, int p) {
    // blk_px0: first pixel (of this lane group's 8) of a [pixel][16] sub-tile
    s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_S16X4(blk_px0 + q * 16 + 4 * p));
    s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_S16X4(blk_px0 + (4 + q) * 16 + 4 * p));
    s16x8 f = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8_t, f);
}

template <bool BNL>
__global__ __launch_bounds__(kCT, 2) void conv3x3_wgrad_bf16_kernel(ConvSrc src, int N, int H, int W, const bf16* __restrict__ gout,
                                                                   int Cout, int nsplit, float* __restrict__ partials, BnLoad bl) {
    constexpr int IW = WG_TW + 2, NPX = WG_TH * WG_TW, NIPX = (WG_TH + 2) * IW;
    extern __shared__ __attribute__((aligned(16))) unsigned char wsm_raw[];
    // The two 16-channel sub-tiles of a half-wave's transpose read (lanes 0-15 | 16-31) must land in different 128-byte bank windows:
    // NPX * 32 B = 8 KB is a multiple of the 256-byte bank period, so the second sub-tile of Gs starts 128 B late (GSUB); NIPX * 32 B
    // = 10 880 B already is 128 (mod 256).  Unpadded, 31 % of this kernel's LDS cycles were 2-way conflicts (profiles/r02_pmc.json).
    constexpr int GSUB = NPX * 16 + 64;
    short* Gs = reinterpret_cast<short*>(wsm_raw);            // [2][GSUB]: [NPX][16] twice
    short* Is = Gs + 2 * GSUB;                                // [2][NIPX][16]
    static_assert((NIPX * 32) % 256 == 128, "Is sub-tiles: re-check the bank offset for this tile shape");
    const int Cin = src.C0 + src.C1;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l15 = lane & 15, kq = lane >> 4;
    const int g8 = 8 * kq, q = (lane >> 2) & 3, p4 = lane & 3;
    const int split = blockIdx.x, ci0 = blockIdx.y * 32, co0 = blockIdx.z * 32;
    const int tilesC = (W + WG_TW - 1) / WG_TW, tilesR = (H + WG_TH - 1) / WG_TH;
    const int ntiles = N * tilesR * tilesC;
    // v_mfma_f32_32x32x16_bf16: one 32 co x 32 ci tile per tap (16 fp32 per lane), k = 16 pixels per step.  Lane map:
    // operand row/col = lane & 31, k-half (8 pixels) = lane >> 5; the 16-lane groups of ds_read_b64_tr_b16 are therefore
    // (channels 0-15 | 16-31) x (pixels 0-7 | 8-15) = (g16 & 1, g16 >> 1).  Half the LDS bytes per flop of 16x16x32.
    // Work split over the 4 waves BY TAP: wave w owns taps 2w and 2w+1 for all 8 rows of a tile, and the two rows 2w, 2w+1 of
    // tap 8.  A tap's accumulator then lives in exactly one wave: taps 0-7 leave through one parallel LDS write, only tap 8
    // (1/9 of the tile) is summed over the waves.  With rows split over the waves instead, all 9 x 16 accumulator registers of
    // every wave went through four serial read-modify-write rounds per block -- a quarter of the kernel's time (measured).
    f32x16 acc[3];
#pragma unroll
    for (int b = 0; b < 3; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[b][r] = 0.f;
    const int wvu = __builtin_amdgcn_readfirstlane(wv);
    const int tap0 = 2 * wvu, tap1 = 2 * wvu + 1;
    const int off0 = ((tap0 / 3) * IW + tap0 % 3) * 16, off1 = ((tap1 / 3) * IW + tap1 % 3) * 16, off8 = (2 * IW + 2) * 16;
    const uint4 zero4 = make_uint4(0, 0, 0, 0);
    const int g16 = lane >> 4, chh = g16 & 1, pxh = g16 >> 1;

    // next tile's operands travel global -> registers while the current tile is on the matrix cores
    constexpr int NG = NPX * 4 / kCT, NI = (NIPX * 4 + kCT - 1) / kCT;
    uint4 pg[NG], pi[NI];
    uint4 pr[BNL ? NG : 1];                                 // BNL: pg = activation gradient, pr = raw output, okg = slots inside the image
    unsigned okg = 0;
    float* Cf = reinterpret_cast<float*>(Is + 2 * NIPX * 16);   // BNL: [6][32] loader coefficients behind the operand tiles
    if (BNL) {
        for (int idx = tid; idx < kBwdCoefRows * 32; idx += kCT) Cf[idx] = co0 + (idx & 31) < Cout ? bl.coef[(size_t)(idx >> 5) * Cout + co0 + (idx & 31)] : 0.f;
        __syncthreads();
    }
    // A thread's slots of the two operand tiles never change: which pixel of the tile, which 8 channels, which source tensor.  Worked out
    // once -- per tile only the tile's corner moves (scalar) and two range tests per slot remain.  (Derived per tile, the index math was
    // ~10 vector instructions per MFMA: profiles/r04_pmc.json, SQ_INSTS_VALU / SQ_INSTS_MFMA of this kernel.)
    int g_iy[NG], g_ix[NG], g_rel[NG];                    // activation-gradient tile: row, column, element offset from the tile's corner (< 0: no such channel)
    int i_iy[NI], i_ix[NI], i_rel[NI], i_src[NI];         // input tile with halo: row - 1, column - 1, offset inside its source, source (0 | 1; -1: no slot)
    {
        const int hs0 = H >> src.ups0, ws0 = W >> src.ups0, ws1 = W >> src.ups1;
        (void)hs0;
#pragma unroll
        for (int j = 0; j < NG; ++j) {
            const int idx = tid + kCT * j, v = idx & 3, px = idx >> 2, c = co0 + v * 8;
            g_ix[j] = px % WG_TW, g_iy[j] = px / WG_TW;
            g_rel[j] = c < Cout ? (g_iy[j] * W + g_ix[j]) * Cout + c : -1;
        }
#pragma unroll
        for (int j = 0; j < NI; ++j) {
            const int idx = tid + kCT * j, v = idx & 3, px = idx >> 2, cc = ci0 + v * 8;
            i_ix[j] = px % IW - 1, i_iy[j] = px / IW - 1;
            const bool slot = idx < NIPX * (3 + 1) && cc < Cin, first = cc < src.C0;
            i_src[j] = slot ? (first ? 0 : 1) : -1;
            // (h0 + d) >> ups = (h0 >> ups) + (d >> ups): tile corners are multiples of 8 x 32, the shift is arithmetic (d = -1 stays outside)
            i_rel[j] = first ? ((i_iy[j] >> src.ups0) * ws0 + (i_ix[j] >> src.ups0)) * src.C0 + cc
                             : ((i_iy[j] >> src.ups1) * ws1 + (i_ix[j] >> src.ups1)) * src.C1 + cc - src.C0;
        }
    }
    auto fetch = [&](int tile) __attribute__((always_inline)) {
        const int tc = tile % tilesC, tr = (tile / tilesC) % tilesR, n = tile / (tilesC * tilesR);
        const int h0 = tr * WG_TH, w0 = tc * WG_TW;
        const bf16* gcorner = gout + (((size_t)n * H + h0) * W + w0) * Cout;
        const bf16* ycorner = BNL ? reinterpret_cast<const bf16*>(bl.gy) + (((size_t)n * H + h0) * W + w0) * Cout : nullptr;
        const bf16* s0 = reinterpret_cast<const bf16*>(src.p0) + (((size_t)n * (H >> src.ups0) + (h0 >> src.ups0)) * (W >> src.ups0) + (w0 >> src.ups0)) * src.C0;
        const bf16* s1 = reinterpret_cast<const bf16*>(src.p1) + (((size_t)n * (H >> src.ups1) + (h0 >> src.ups1)) * (W >> src.ups1) + (w0 >> src.ups1)) * src.C1;
        okg = 0;
#pragma unroll
        for (int j = 0; j < NG; ++j) {
            uint4 val = zero4;
            if (g_rel[j] >= 0 && g_iy[j] < H - h0 && g_ix[j] < W - w0) {
                if (BNL) { pr[j] = *reinterpret_cast<const uint4*>(gcorner + g_rel[j]); val = *reinterpret_cast<const uint4*>(ycorner + g_rel[j]); okg |= 1u << j; }
                else val = *reinterpret_cast<const uint4*>(gcorner + g_rel[j]);
            }
            pg[j] = val;
        }
#pragma unroll
        for (int j = 0; j < NI; ++j) {
            uint4 val = zero4;
            if (i_src[j] >= 0 && (unsigned)(h0 + i_iy[j]) < (unsigned)H && (unsigned)(w0 + i_ix[j]) < (unsigned)W)
                val = *reinterpret_cast<const uint4*>((i_src[j] ? s1 : s0) + i_rel[j]);
            pi[j] = val;
        }
    };
    if (split < ntiles) fetch(split);
    for (int tile = split; tile < ntiles; tile += nsplit) {
        __syncthreads();
        if (BNL) {
            asm volatile("" ::: "memory");
            float cf[kBwdCoefRows][8];
#pragma unroll
            for (int r = 0; r < kBwdCoefRows; ++r)
#pragma unroll
                for (int i = 0; i < 8; i += 4) {
                    const float4 q = *reinterpret_cast<const float4*>(Cf + r * 32 + (tid & 3) * 8 + i);
                    cf[r][i] = q.x; cf[r][i + 1] = q.y; cf[r][i + 2] = q.z; cf[r][i + 3] = q.w;
                }
#pragma unroll
            for (int j = 0; j < NG; ++j)
                pg[j] = (okg >> j) & 1u ? bn_graw_vec<bf16>(pr[j], pg[j], cf[0], cf[1], cf[2], cf[3], cf[4], cf[5]) : zero4;
        }
#pragma unroll
        for (int j = 0; j < NG; ++j) {
            const int idx = tid + kCT * j, v = idx & 3, px = idx >> 2;
            *reinterpret_cast<uint4*>(Gs + (v >> 1) * GSUB + px * 16 + (v & 1) * 8) = pg[j];
        }
#pragma unroll
        for (int j = 0; j < NI; ++j) {
            const int idx = tid + kCT * j, v = idx & 3, px = idx >> 2;
            if (idx < NIPX * 4) *reinterpret_cast<uint4*>(Is + ((v >> 1) * NIPX + px) * 16 + (v & 1) * 8) = pi[j];
        }
        __syncthreads();
        if (tile + nsplit < ntiles) fetch(tile + nsplit);
#pragma unroll 2
        for (int row = 0; row < WG_TH; ++row) {
            const short* gb = Gs + chh * GSUB + (row * WG_TW + 8 * pxh) * 16;
            const bf16x8_t a0 = tr_frag(gb, q, p4), a1 = tr_frag(gb + 16 * 16, q, p4);     // pixels 0-15 | 16-31 of the row
            const short* ib = Is + (chh * NIPX + row * IW + 8 * pxh) * 16;
            {
                const bf16x8_t b0 = tr_frag(ib + off0, q, p4), b1 = tr_frag(ib + off0 + 16 * 16, q, p4);
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0, acc[0], 0, 0, 0);
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, acc[0], 0, 0, 0);
            }
            {
                const bf16x8_t b0 = tr_frag(ib + off1, q, p4), b1 = tr_frag(ib + off1 + 16 * 16, q, p4);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0, acc[1], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, acc[1], 0, 0, 0);
            }
            if ((row >> 1) == wvu) {
                const bf16x8_t b0 = tr_frag(ib + off8, q, p4), b1 = tr_frag(ib + off8 + 16 * 16, q, p4);
                acc[2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0, acc[2], 0, 0, 0);
                acc[2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, acc[2], 0, 0, 0);
            }
        }
    }
    // partial [split][co 32][tap 9][ci 32] through LDS.  D[row = co = (reg&3) + 8*(reg>>2) + 4*(lane>>5)][col = ci = lane & 31]
    float* Ds = reinterpret_cast<float*>(wsm_raw);  // [32][288]; then the four waves' tap-8 planes [4][32][32]
    float* D8 = Ds + 32 * 288;
    __syncthreads();                                // the operand tiles are dead
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int co = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5), ci = lane & 31;
        Ds[co * 288 + tap0 * 32 + ci] = acc[0][r];
        Ds[co * 288 + tap1 * 32 + ci] = acc[1][r];
        D8[wvu * 1024 + co * 32 + ci] = acc[2][r];
    }
    __syncthreads();
    float* outp = partials + (((size_t)split * gridDim.z + blockIdx.z) * gridDim.y + blockIdx.y) * (32 * 288);
    for (int e = tid; e < 32 * 288; e += kCT) {
        const int co = e / 288, col = e - co * 288;
        float v = Ds[e];
        if (col >= 256) {
            const int i8 = co * 32 + col - 256;
            v = (D8[i8] + D8[1024 + i8]) + (D8[2048 + i8] + D8[3072 + i8]);
        }
        outp[e] = v;
    }
}

// Narrow-layer variant (the 256^2 / 128^2 layers that are HBM-bound): a block owns 16 output channels (grid.z) x one
// 16-channel slice of the input (grid.y), v_mfma_f32_16x16x32_bf16 (k = the 32 pixels of a tile row), 36 accumulator
// registers instead of 144 and 19 KB of LDS instead of 38 -> ~5 blocks per CU keep enough loads in flight to stream.
// Writes the same partial layout as conv3x3_wgrad_bf16_kernel (its 16 x 9 x 16 corner of the 32 x 288 tile).
template <bool BNL>
__global__ __launch_bounds__(kCT, BNL ? 3 : 4) void conv3x3_wgrad_bf16_c16_kernel(ConvSrc src, int N, int H, int W, const bf16* __restrict__ gout,
                                                                       int Cout, int nsplit, float* __restrict__ partials, BnLoad bl) {
    constexpr int IW = WG_TW + 2, NPX = WG_TH * WG_TW, NIPX = (WG_TH + 2) * IW;
    extern __shared__ __attribute__((aligned(16))) unsigned char wsm_raw[];
    short* Gs = reinterpret_cast<short*>(wsm_raw);            // [NPX][16]
    short* Is = Gs + NPX * 16;                                // [NIPX][16]
    const int Cin = src.C0 + src.C1;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l15 = lane & 15, kq = lane >> 4;
    const int q = (lane >> 2) & 3, p4 = lane & 3;
    const int split = blockIdx.x, ci0 = blockIdx.y * 16, co0 = blockIdx.z * 16;
    const int tilesC = (W + WG_TW - 1) / WG_TW, tilesR = (H + WG_TH - 1) / WG_TH;
    const int ntiles = N * tilesR * tilesC;
    f32x4 acc[9];
#pragma unroll
    for (int b = 0; b < 9; ++b) acc[b] = f32x4{0.f, 0.f, 0.f, 0.f};
    const uint4 zero4 = make_uint4(0, 0, 0, 0);
    constexpr int NG = NPX * 2 / kCT, NI = (NIPX * 2 + kCT - 1) / kCT;
    uint4 pg[NG], pi[NI];
    uint4 pr[BNL ? NG : 1];
    unsigned okg = 0;
    float* Cf = reinterpret_cast<float*>(Is + NIPX * 16);       // BNL: [6][16] loader coefficients behind the operand tiles
    if (BNL) {
        for (int idx = tid; idx < kBwdCoefRows * 16; idx += kCT) Cf[idx] = co0 + (idx & 15) < Cout ? bl.coef[(size_t)(idx >> 4) * Cout + co0 + (idx & 15)] : 0.f;
        __syncthreads();
    }
    // tile-invariant slot geometry, as in conv3x3_wgrad_bf16_kernel
    int g_iy[NG], g_ix[NG], g_rel[NG];                    // activation-gradient tile: row, column, element offset from the tile's corner (< 0: no such channel)
    int i_iy[NI], i_ix[NI], i_rel[NI], i_src[NI];         // input tile with halo: row - 1, column - 1, offset inside its source, source (0 | 1; -1: no slot)
    {
        const int hs0 = H >> src.ups0, ws0 = W >> src.ups0, ws1 = W >> src.ups1;
        (void)hs0;
#pragma unroll
        for (int j = 0; j < NG; ++j) {
            const int idx = tid + kCT * j, v = idx & 1, px = idx >> 1, c = co0 + v * 8;
            g_ix[j] = px % WG_TW, g_iy[j] = px / WG_TW;
            g_rel[j] = c < Cout ? (g_iy[j] * W + g_ix[j]) * Cout + c : -1;
        }
#pragma unroll
        for (int j = 0; j < NI; ++j) {
            const int idx = tid + kCT * j, v = idx & 1, px = idx >> 1, cc = ci0 + v * 8;
            i_ix[j] = px % IW - 1, i_iy[j] = px / IW - 1;
            const bool slot = idx < NIPX * (1 + 1) && cc < Cin, first = cc < src.C0;
            i_src[j] = slot ? (first ? 0 : 1) : -1;
            // (h0 + d) >> ups = (h0 >> ups) + (d >> ups): tile corners are multiples of 8 x 32, the shift is arithmetic (d = -1 stays outside)
            i_rel[j] = first ? ((i_iy[j] >> src.ups0) * ws0 + (i_ix[j] >> src.ups0)) * src.C0 + cc
                             : ((i_iy[j] >> src.ups1) * ws1 + (i_ix[j] >> src.ups1)) * src.C1 + cc - src.C0;
        }
    }
    auto fetch = [&](int tile) __attribute__((always_inline)) {
        const int tc = tile % tilesC, tr = (tile / tilesC) % tilesR, n = tile / (tilesC * tilesR);
        const int h0 = tr * WG_TH, w0 = tc * WG_TW;
        const bf16* gcorner = gout + (((size_t)n * H + h0) * W + w0) * Cout;
        const bf16* ycorner = BNL ? reinterpret_cast<const bf16*>(bl.gy) + (((size_t)n * H + h0) * W + w0) * Cout : nullptr;
        const bf16* s0 = reinterpret_cast<const bf16*>(src.p0) + (((size_t)n * (H >> src.ups0) + (h0 >> src.ups0)) * (W >> src.ups0) + (w0 >> src.ups0)) * src.C0;
        const bf16* s1 = reinterpret_cast<const bf16*>(src.p1) + (((size_t)n * (H >> src.ups1) + (h0 >> src.ups1)) * (W >> src.ups1) + (w0 >> src.ups1)) * src.C1;
        okg = 0;
#pragma unroll
        for (int j = 0; j < NG; ++j) {
            uint4 val = zero4;
            if (g_rel[j] >= 0 && g_iy[j] < H - h0 && g_ix[j] < W - w0) {
                if (BNL) { pr[j] = *reinterpret_cast<const uint4*>(gcorner + g_rel[j]); val = *reinterpret_cast<const uint4*>(ycorner + g_rel[j]); okg |= 1u << j; }
                else val = *reinterpret_cast<const uint4*>(gcorner + g_rel[j]);
            }
            pg[j] = val;
        }
#pragma unroll
        for (int j = 0; j < NI; ++j) {
            uint4 val = zero4;
            if (i_src[j] >= 0 && (unsigned)(h0 + i_iy[j]) < (unsigned)H && (unsigned)(w0 + i_ix[j]) < (unsigned)W)
                val = *reinterpret_cast<const uint4*>((i_src[j] ? s1 : s0) + i_rel[j]);
            pi[j] = val;
        }
    };
    if (split < ntiles) fetch(split);
    for (int tile = split; tile < ntiles; tile += nsplit) {
        __syncthreads();
        if (BNL) {
            asm volatile("" ::: "memory");
            float cf[kBwdCoefRows][8];
#pragma unroll
            for (int r = 0; r < kBwdCoefRows; ++r)
#pragma unroll
                for (int i = 0; i < 8; i += 4) {
                    const float4 q = *reinterpret_cast<const float4*>(Cf + r * 16 + (tid & 1) * 8 + i);
                    cf[r][i] = q.x; cf[r][i + 1] = q.y; cf[r][i + 2] = q.z; cf[r][i + 3] = q.w;
                }
#pragma unroll
            for (int j = 0; j < NG; ++j)
                pg[j] = (okg >> j) & 1u ? bn_graw_vec<bf16>(pr[j], pg[j], cf[0], cf[1], cf[2], cf[3], cf[4], cf[5]) : zero4;
        }
#pragma unroll
        for (int j = 0; j < NG; ++j) {
            const int idx = tid + kCT * j;
            *reinterpret_cast<uint4*>(Gs + (idx >> 1) * 16 + (idx & 1) * 8) = pg[j];
        }
#pragma unroll
        for (int j = 0; j < NI; ++j) {
            const int idx = tid + kCT * j;
            if (idx < NIPX * 2) *reinterpret_cast<uint4*>(Is + (idx >> 1) * 16 + (idx & 1) * 8) = pi[j];
        }
        __syncthreads();
        if (tile + nsplit < ntiles) fetch(tile + nsplit);
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {
            const int row = wv * 2 + rr;
            const bf16x8_t a0 = tr_frag32(Gs + row * WG_TW * 16, kq, q, p4);
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int ky = tap / 3, kx = tap % 3;
                const bf16x8_t b0 = tr_frag32(Is + ((row + ky) * IW + kx) * 16, kq, q, p4);
                acc[tap] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b0, acc[tap], 0, 0, 0);
            }
        }
    }
    // reduce the 4 waves in LDS (fixed order): D[row = co = kq*4 + r][col = ci = l15] -> Ds[co][tap*16 + ci]
    float* Ds = reinterpret_cast<float*>(wsm_raw);   // 16 x 144 floats = 9.2 KB
    for (int w = 0; w < 4; ++w) {
        __syncthreads();
        if (wv == w) {
#pragma unroll
            for (int tap = 0; tap < 9; ++tap)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int o = (kq * 4 + r) * 144 + tap * 16 + l15;
                    if (w == 0) Ds[o] = acc[tap][r];
                    else Ds[o] += acc[tap][r];
                }
        }
    }
    __syncthreads();
    const int nci32 = (Cin + 31) / 32, nco32 = (Cout + 31) / 32;
    float* outp = partials + (((size_t)split * nco32 + blockIdx.z / 2) * nci32 + blockIdx.y / 2) * (32 * 288) + (blockIdx.y & 1) * 16;
    for (int e = tid; e < 16 * 144; e += kCT) {
        const int co = (blockIdx.z & 1) * 16 + e / 144, tap = (e % 144) / 16, ci = e % 16;
        outp[co * 288 + tap * 32 + ci] = Ds[e];
    }
}

__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ partials, int nsplit, int Cout, int Cin, int nco,
                                                           int nci, float* __restrict__ gw) {
    // walk the partial tiles in THEIR order ([co tile][ci tile][co 32][tap 9][ci 32]: consecutive threads read consecutive
    // floats of every part); the weight-gradient index takes the permutation (read many parts, write once)
    const size_t stride = (size_t)nco * nci * (32 * 288);
    reduce_partials_block(partials, nsplit, stride, nco * nci * 32 * 288, gw, [](int e) { return (size_t)e; }, [=](int e) {
        const int ci32 = e & 31, tap = (e >> 5) % 9, co32 = (e / 288) & 31, tile = e / (32 * 288);
        const int co = (tile / nci) * 32 + co32, ci = (tile % nci) * 32 + ci32;
        return (co < Cout && ci < Cin) ? (co * Cin + ci) * 9 + tap : -1;
    });
}

}  // namespace miseg

using namespace miseg;

// gw[Cout][Cin][9] <- gw_pad[Cout][Cin_pad][9] (first Cin input channels): the stem's weight gradient, computed for one whole channel
// vector of (zero) input channels, into the parameter's own gradient (ref contrastyou/arch/unet.py:15: Conv2d(input_dim, 16, 3)).
namespace miseg {
__global__ __launch_bounds__(256) void slice_cin_kernel(const float* __restrict__ src, int Cout, int Cin_pad, int Cin, float* __restrict__ dst) {
    const int total = Cout * Cin * 9;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < total; e += gridDim.x * 256) {
        const int t = e % 9, ci = (e / 9) % Cin, co = e / (9 * Cin);
        dst[e] = src[((size_t)co * Cin_pad + ci) * 9 + t];
    }
}
}  // namespace miseg
extern "C" int miseg_conv3x3_wgrad_slice(void* stream, const float* gw_padded, int64_t Cout, int64_t Cin_pad, int64_t Cin, float* gw) {
    MISEG_TAPE(miseg_conv3x3_wgrad_slice, stream, gw_padded, Cout, Cin_pad, Cin, gw);
    MISEG_REQUIRE(gw_padded && gw && Cout > 0 && Cin > 0 && Cin <= Cin_pad, "conv3x3_wgrad_slice: bad args");
    const int total = (int)(Cout * Cin * 9);
    hipLaunchKernelGGL(slice_cin_kernel, dim3(std::min((total + 255) / 256, 256)), dim3(256), 0, as_stream(stream), gw_padded, (int)Cout, (int)Cin_pad,
                       (int)Cin, gw);
    MISEG_LAUNCH_CHECK("slice_cin_kernel");
    return MISEG_OK;
}

static int wgrad_splits(int64_t N, int64_t H, int64_t W, int64_t Cin, int64_t Cout) {
    const int64_t ntiles = N * cdiv(H, WG_TH) * cdiv(W, WG_TW);
    const int64_t per = cdiv(Cin, 32) * cdiv(Cout, 32);
    // Blocks a weight-gradient launch is split into.  The launches run on their own stream beside the main stream's backward: with 512
    // the wgrad kernels themselves are fastest (1.86 ms per step in total), with 256 they take 1.96 ms but the STEP is 0.14 ms
    // shorter (7.13 vs 7.27 ms, same box, two alternations; 192: 7.18-7.35, 128: 7.31-7.47) -- one block per CU leaves the other
    // half of every CU's wave slots and LDS to the critical-path kernels.
    static const int target = [] { const char* e = getenv("MISEG_WGRAD_BLOCKS"); return e ? atoi(e) : 256; }();
    int64_t s = std::max<int64_t>(1, target / per);
    return (int)std::min<int64_t>(s, ntiles);
}

extern "C" int64_t miseg_conv3x3_wgrad_ws_bytes(int64_t N, int64_t H, int64_t W, int64_t Cin, int64_t Cout) {
    return (int64_t)wgrad_splits(N, H, W, Cin, Cout) * cdiv(Cin, 32) * cdiv(Cout, 32) * 32 * 288 * 4;
}

static int conv3x3_wgrad_impl(void* stream, int dt, const void* in0, int64_t C0, int ups0, const void* in1, int64_t C1, int ups1, int64_t N,
                              int64_t H, int64_t W, const void* gout, int64_t Cout, float* gw, void* ws, int64_t ws_bytes, BnLoad bl) {
    MISEG_REQUIRE(in0 && gout && gw && ws, "conv3x3_wgrad: null pointer");
    MISEG_REQUIRE(C1 == 0 || in1, "conv3x3_wgrad: second source missing");
    const int64_t Cin = C0 + C1;
    MISEG_REQUIRE(ws_bytes >= miseg_conv3x3_wgrad_ws_bytes(N, H, W, Cin, Cout), "conv3x3_wgrad: workspace too small");
    ConvSrc s{in0, in1, (int)C0, (int)C1, ups0, ups1};
    const int ns = wgrad_splits(N, H, W, Cin, Cout), nci = (int)cdiv(Cin, 32), nco = (int)cdiv(Cout, 32);
    const size_t lb = ((size_t)WG_TH * WG_TW + (WG_TH + 2) * (WG_TW + 2)) * WG_P * 4;
    hipStream_t st = as_stream(stream);
    dim3 grid(ns, nci, nco);
    MISEG_WITH_STORAGE_TYPE(dt, "conv3x3_wgrad",
    if constexpr (std::is_same_v<TT, float>) {
        if (bl.gy) {
            hipFuncSetAttribute((const void*)conv3x3_wgrad_kernel<TT, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lb);
            hipLaunchKernelGGL((conv3x3_wgrad_kernel<TT, true>), grid, dim3(kCT), lb, st, s, (int)N, (int)H, (int)W, (const TT*)gout, (int)Cout, ns, (float*)ws, bl);
        } else {
            hipFuncSetAttribute((const void*)conv3x3_wgrad_kernel<TT, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lb);
            hipLaunchKernelGGL((conv3x3_wgrad_kernel<TT, false>), grid, dim3(kCT), lb, st, s, (int)N, (int)H, (int)W, (const TT*)gout, (int)Cout, ns, (float*)ws, bl);
        }
    } else {
        MISEG_REQUIRE(C0 % 8 == 0 && C1 % 8 == 0 && Cout % 8 == 0, "conv3x3_wgrad: bf16 needs channel counts that are multiples of 8");
        const size_t lbb = std::max<size_t>(((size_t)2 * WG_TH * WG_TW + 2 * (WG_TH + 2) * (WG_TW + 2)) * 16 * 2 + 2 * 64 * 2, (size_t)(32 * 288 + 4 * 1024) * 4);
        // narrow layers (measured per shape, scratch/time_conv.py): the lean 16x16-tile kernel wins when one side has <= 16
        // channels (256^2 16->16: 125 -> 52 us, 32->16: 129 -> 83, 128^2 16->32: 85 -> 48) and for 32->64 (71 -> 53);
        // from 32->32 up the 32x32-tile kernel's operand reuse wins
        // (tests/exact_ref.py wgrad_kernel() mirrors this choice to name its cases by kernel: change both together)
        const bool narrow = Cout % 16 == 0 && (std::min(Cin, Cout) <= 16 || (Cin == 32 && Cout == 64));
        if (narrow || Cout <= 16) {
            const size_t lbc = (size_t)(WG_TH * WG_TW + (WG_TH + 2) * (WG_TW + 2)) * 16 * 2 + (bl.gy ? kBwdCoefRows * 16 * 4 : 0);
            dim3 gridc(ns, (unsigned)cdiv(Cin, 16), (unsigned)cdiv(Cout, 16));
            if (bl.gy) hipLaunchKernelGGL(conv3x3_wgrad_bf16_c16_kernel<true>, gridc, dim3(kCT), lbc, st, s, (int)N, (int)H, (int)W, (const bf16*)gout, (int)Cout, ns, (float*)ws, bl);
            else hipLaunchKernelGGL(conv3x3_wgrad_bf16_c16_kernel<false>, gridc, dim3(kCT), lbc, st, s, (int)N, (int)H, (int)W, (const bf16*)gout, (int)Cout, ns, (float*)ws, bl);
        } else if (bl.gy) {
            hipFuncSetAttribute((const void*)conv3x3_wgrad_bf16_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lbb);
            hipLaunchKernelGGL(conv3x3_wgrad_bf16_kernel<true>, grid, dim3(kCT), lbb, st, s, (int)N, (int)H, (int)W, (const bf16*)gout, (int)Cout, ns, (float*)ws, bl);
        } else {
            hipFuncSetAttribute((const void*)conv3x3_wgrad_bf16_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lbb);
            hipLaunchKernelGGL(conv3x3_wgrad_bf16_kernel<false>, grid, dim3(kCT), lbb, st, s, (int)N, (int)H, (int)W, (const bf16*)gout, (int)Cout, ns, (float*)ws, bl);
        }
    }
    return MISEG_OK);
    MISEG_LAUNCH_CHECK("conv3x3_wgrad_kernel");
    const int total = nco * nci * 32 * 288;
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(reduce_grid(total, ns)), dim3(256), 0, st, (const float*)ws, ns, (int)Cout, (int)Cin, nco, nci, gw);
    MISEG_LAUNCH_CHECK("wgrad_reduce_kernel");
    return MISEG_OK;
}

extern "C" int miseg_conv3x3_wgrad(void* stream, int dt, const void* in0, int64_t C0, int ups0, const void* in1, int64_t C1, int ups1,
                                   int64_t N, int64_t H, int64_t W, const void* gout, int64_t Cout, float* gw, void* ws, int64_t ws_bytes) {
    MISEG_TAPE(miseg_conv3x3_wgrad, stream, dt, in0, C0, ups0, in1, C1, ups1, N, H, W, gout, Cout, gw, ws, ws_bytes);
    MISEG_F16_DISPATCH_ON(dt, miseg_conv3x3_wgrad, stream, MISEG_BF16, in0, C0, ups0, in1, C1, ups1, N, H, W, gout, Cout, gw, ws, ws_bytes);
    return conv3x3_wgrad_impl(stream, dt, in0, C0, ups0, in1, C1, ups1, N, H, W, gout, Cout, gw, ws, ws_bytes, BnLoad{nullptr, nullptr});
}

extern "C" int miseg_conv3x3_wgrad_bn(void* stream, int dt, const void* in0, int64_t C0, int ups0, const void* in1, int64_t C1, int ups1,
                                      int64_t N, int64_t H, int64_t W, const void* raw, const void* gy, const float* bwd_coef, int64_t Cout,
                                      float* gw, void* ws, int64_t ws_bytes) {
    MISEG_TAPE(miseg_conv3x3_wgrad_bn, stream, dt, in0, C0, ups0, in1, C1, ups1, N, H, W, raw, gy, bwd_coef, Cout, gw, ws, ws_bytes);
    MISEG_F16_DISPATCH_ON(dt, miseg_conv3x3_wgrad_bn, stream, MISEG_BF16, in0, C0, ups0, in1, C1, ups1, N, H, W, raw, gy, bwd_coef, Cout, gw, ws, ws_bytes);
    MISEG_REQUIRE(gy && bwd_coef, "conv3x3_wgrad_bn: null pointer");
    MISEG_REQUIRE(Cout % (dt == MISEG_F32 ? 4 : 8) == 0, "conv3x3_wgrad_bn: Cout must be a whole number of 16-byte vectors");
    return conv3x3_wgrad_impl(stream, dt, in0, C0, ups0, in1, C1, ups1, N, H, W, raw, Cout, gw, ws, ws_bytes, BnLoad{gy, bwd_coef});
}
