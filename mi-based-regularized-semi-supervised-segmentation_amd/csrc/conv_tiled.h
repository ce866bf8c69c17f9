// conv3x3_kernel, the per-tile 3x3 convolution: the template that conv_tiled.hip (16-bit storage, plain forms), conv_tiled_bn.hip (16-bit
// storage, BatchNorm-loader and epilogue-reduce forms) and conv_tiled_f32.hip (float, every form) instantiate, each its own forms --
// three units so that they compile side by side.
#pragma once
#include <type_traits>
#include "conv.h"

namespace miseg {

// COT: output channels per block; TW: tile width (32 or 16).  grid = (N*tilesR*tilesC, ceil(Cout/COT)).
// POOL: as in conv3x3_stream_kernel below -- the output leaves 2x2 sum-pooled (H, W even; no statistics).
// BNL: the (single, full-resolution) source is a BatchNorm layer's raw output and bl.gy the gradient of its activation -- the loader
// forms graw (common.h, bn_graw_vec); out-of-image halo pixels stay zero.  RED: the epilogue also takes the BatchNorm-backward sums of
// the layer that produced this launch's output tensor (BnRed; non-pooled output, Cout % 4 == 0, no forward statistics).
// NW waves per block (4, or 8 for the 16-row tiles of the deep layers: the same LDS tile -- one block per CU either way -- worked by two
// waves per SIMD that cover each other's LDS round trips, each with half the rows).
template <typename T, int COT, int TW, int THT, bool POOL = false, bool BNL = false, bool RED = false, int NW = 4>
__global__ __launch_bounds__(64 * NW, 1) void conv3x3_kernel(ConvSrc src, int N, int H, int W, const T* __restrict__ wpk, int Cout,
                                                        T* __restrict__ out, float* __restrict__ stats, BnFinish fin, BnLoad bl, BnRed br) {
    static_assert(!(RED && POOL), "the epilogue reduce exists for full-resolution outputs");
    typedef Mma<T> MM;
    constexpr int kCT = 64 * NW;                            // shadows the file-scope block size inside this kernel
    static_assert(THT % NW == 0, "whole rows per wave");
    constexpr int VEC = MM::VEC, NT = COT / 16, MTR = TW / 16, RW = THT / NW, MTW = RW * MTR;   // RW rows of the tile per wave
    constexpr int KP = MM::KP;                              // LDS stride of one pixel / one weight row (elements)
    constexpr int IW = TW + 2, IH = THT + 2;
    constexpr int NIS = (IH * IW * (CK / VEC) + kCT - 1) / kCT, NWS = (9 * COT * (CK / VEC) + kCT - 1) / kCT;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    T* Is = reinterpret_cast<T*>(smem);                    // [IH][IW][KP]
    T* Ws = Is + IH * IW * KP;                             // [9][COT][KP]
    const int Cin = src.C0 + src.C1;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l15 = lane & 15, kq = lane >> 4;
    const int tilesC = (W + TW - 1) / TW, tilesR = (H + THT - 1) / THT;
    const int tc = blockIdx.x % tilesC, tr = (blockIdx.x / tilesC) % tilesR, n = blockIdx.x / (tilesC * tilesR);
    const int h0 = tr * THT, w0 = tc * TW, co0 = blockIdx.y * COT;

    f32x4 acc[MTW][NT];
#pragma unroll
    for (int m = 0; m < MTW; ++m)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[m][t] = f32x4{0.f, 0.f, 0.f, 0.f};

    // One 32-channel chunk of the haloed input tile and of the weights is in flight in registers while the previous
    // chunk is on the matrix cores (the block is alone on its CU: 1 wave per SIMD, so nothing else hides the latency).
    uint4 pin[NIS], pwt[NWS];
    uint4 pgy[BNL ? NIS : 1];                    // BNL: the activation gradient beside the raw output, the slot's coefficients,
    float cfr[BNL ? kBwdCoefRows * VEC : 1];     // and which slots lie inside the image (the others stay zero, not P - Q * mean)
    unsigned okm = 0;
    static_assert(NIS <= 32 && kCT % (CK / VEC) == 0, "slot mask / per-thread channel vector");
    const uint4 zero4 = make_uint4(0u, 0u, 0u, 0u);
    auto fetch = [&](int c0) __attribute__((always_inline)) {
        if (BNL) {
            okm = 0;
            const int c = c0 + (tid % (CK / VEC)) * VEC;         // the same channel vector in every slot of this thread
#pragma unroll
            for (int r = 0; r < kBwdCoefRows; ++r)
#pragma unroll
                for (int i = 0; i < VEC; i += 4) {
                    const float4 q = c < Cin ? *reinterpret_cast<const float4*>(bl.coef + (size_t)r * Cin + c + i) : make_float4(0.f, 0.f, 0.f, 0.f);
                    cfr[r * VEC + i] = q.x; cfr[r * VEC + i + 1] = q.y; cfr[r * VEC + i + 2] = q.z; cfr[r * VEC + i + 3] = q.w;
                }
        }
#pragma unroll
        for (int j = 0; j < NIS; ++j) {
            const int idx = tid + kCT * j;
            const int v = idx % (CK / VEC), px = idx / (CK / VEC), ix = px % IW, iy = px / IW;
            const int h = h0 - 1 + iy, w = w0 - 1 + ix, c = c0 + v * VEC;
            uint4 val = zero4;
            if (idx < IH * IW * (CK / VEC) && h >= 0 && h < H && w >= 0 && w < W && c < Cin) {
                const T* sp;
                if (BNL) {
                    const size_t o = (((size_t)n * H + h) * W + w) * src.C0 + c;
                    sp = reinterpret_cast<const T*>(src.p0) + o;
                    pgy[j] = *reinterpret_cast<const uint4*>(reinterpret_cast<const T*>(bl.gy) + o);
                    okm |= 1u << j;
                } else if (c < src.C0) {
                    const int hs = H >> src.ups0, wsz = W >> src.ups0;
                    sp = reinterpret_cast<const T*>(src.p0) + (((size_t)n * hs + (h >> src.ups0)) * wsz + (w >> src.ups0)) * src.C0 + c;
                } else {
                    const int hs = H >> src.ups1, wsz = W >> src.ups1;
                    sp = reinterpret_cast<const T*>(src.p1) + (((size_t)n * hs + (h >> src.ups1)) * wsz + (w >> src.ups1)) * src.C1 + (c - src.C0);
                }
                val = *reinterpret_cast<const uint4*>(sp);
            }
            pin[j] = val;
        }
#pragma unroll
        for (int j = 0; j < NWS; ++j) {
            const int idx = tid + kCT * j;
            const int v = idx % (CK / VEC), co = (idx / (CK / VEC)) % COT, tap = idx / ((CK / VEC) * COT);
            const int c = c0 + v * VEC;
            uint4 val = zero4;
            if (idx < 9 * COT * (CK / VEC) && co0 + co < Cout && c < Cin)
                val = *reinterpret_cast<const uint4*>(wpk + ((size_t)tap * Cout + co0 + co) * Cin + c);
            pwt[j] = val;
        }
    };
    // every fragment read below is one of these two bases plus a compile-time offset (an instruction immediate)
    const T* Ib = Is + ((wv * RW) * IW + l15) * KP;
    const T* Wb = Ws + l15 * KP;
    fetch(0);
    auto chunk = [&](int c0) __attribute__((always_inline)) {
        __syncthreads();                       // previous chunk's MFMAs are done with Is / Ws
#pragma unroll
        for (int j = 0; j < NIS; ++j) {
            const int idx = tid + kCT * j;
            if (idx < IH * IW * (CK / VEC)) {
                uint4 val = pin[j];
                if (BNL) {
                    typedef typename VT<T>::Raw Raw;
                    if ((okm >> j) & 1u) {
                        const Raw g = bn_graw_vec<T>(*reinterpret_cast<const Raw*>(&pin[j]), *reinterpret_cast<const Raw*>(&pgy[j]), cfr, cfr + VEC,
                                                     cfr + 2 * VEC, cfr + 3 * VEC, cfr + 4 * VEC, cfr + 5 * VEC);
                        val = *reinterpret_cast<const uint4*>(&g);
                    } else val = zero4;
                }
                *reinterpret_cast<uint4*>(Is + (idx / (CK / VEC)) * KP + (idx % (CK / VEC)) * VEC) = val;
            }
        }
#pragma unroll
        for (int j = 0; j < NWS; ++j) {
            const int idx = tid + kCT * j;
            if (idx < 9 * COT * (CK / VEC)) *reinterpret_cast<uint4*>(Ws + (idx / (CK / VEC)) * KP + (idx % (CK / VEC)) * VEC) = pwt[j];
        }
        __syncthreads();
        if (c0 + CK < Cin) fetch(c0 + CK);
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int ky = tap / 3, kx = tap % 3;
            typename MM::Frag bf[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) bf[t] = MM::load(Wb + (tap * COT + t * 16) * KP, kq);
#pragma unroll
            for (int m = 0; m < MTW; ++m) {
                typename MM::Frag af = MM::load(Ib + ((m / MTR + ky) * IW + (m % MTR) * 16 + kx) * KP, kq);
#pragma unroll
                for (int t = 0; t < NT; ++t) MM::mma_chunk(bf[t], af, acc[m][t]);   // D^T: rows = channels, cols = pixels
            }
        }
    };
    // RED: the producer's raw output at this block's output positions (a lane's 4 channels of a pixel per (m, t)) and its coefficients
    // are requested before the LAST chunk goes to the matrix cores, so that they have arrived when the epilogue wants them
    struct RedQuad { float v[4]; };
    RedQuad rp[RED ? MTW : 1][RED ? NT : 1];
    float rsc[RED ? NT : 1][4], rsh[RED ? NT : 1][4], rmu[RED ? NT : 1][4];
    if (RED) {
        int c0 = 0;
        for (; c0 + CK < Cin; c0 += CK) chunk(c0);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int co = co0 + t * 16 + kq * 4;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool in = co + r < Cout;
                rmu[t][r] = in ? br.saved[co + r] : 0.f;
                rsc[t][r] = in ? br.saved[2 * Cout + co + r] : 0.f;
                rsh[t][r] = in ? br.saved[3 * Cout + co + r] : 0.f;
            }
        }
#pragma unroll
        for (int m = 0; m < MTW; ++m) {
            const int h = h0 + wv * RW + m / MTR, w = w0 + (m % MTR) * 16 + l15;
            const T* rq = reinterpret_cast<const T*>(br.raw) + (((size_t)n * H + h) * W + w) * Cout;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int co = co0 + t * 16 + kq * 4;
                T q[4] = {from_f32<T>(0.f), from_f32<T>(0.f), from_f32<T>(0.f), from_f32<T>(0.f)};
                if (h < H && w < W && co + 3 < Cout) {
                    if (sizeof(T) == 2) *reinterpret_cast<uint2*>(q) = *reinterpret_cast<const uint2*>(rq + co);
                    else *reinterpret_cast<uint4*>(q) = *reinterpret_cast<const uint4*>(rq + co);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) rp[m][t].v[r] = to_f32(q[r]);
            }
        }
        chunk(c0);
    } else {
        for (int c0 = 0; c0 < Cin; c0 += CK) chunk(c0);
    }
    // ---- epilogue: D^T[row = channel t*16 + kq*4 + r][col = pixel l15]: a lane owns 4 consecutive channels of one pixel, so
    // the 16 lanes x 4 kq of a wave store whole NHWC pixel vectors (8-byte pieces, contiguous across kq)
    if (POOL) {      // rows 2 pr, 2 pr + 1 of the wave (two registers of the lane) + the column neighbour's sum; even lanes store
        static_assert(!POOL || RW % 2 == 0, "pooled epilogue: a wave owns whole row pairs");
        const int Hp = H >> 1, Wp = W >> 1;
#pragma unroll
        for (int mp = 0; mp < MTW / 2; ++mp) {
            const int m0 = (2 * (mp / MTR)) * MTR + mp % MTR, m1 = m0 + MTR;
            const int hp = ((h0 + wv * RW) >> 1) + mp / MTR, wp = ((w0 + (mp % MTR) * 16) >> 1) + (l15 >> 1);
            const bool mine = !(l15 & 1) && hp < Hp && wp < Wp;
            T* op = out + (((size_t)n * Hp + hp) * Wp + wp) * Cout;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int co = co0 + t * 16 + kq * 4;
                T pk[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float v = acc[m0][t][r] + acc[m1][t][r];
                    v += __shfl_xor(v, 1, 64);
                    pk[r] = from_f32<T>(v);
                }
                if (!mine) continue;
                if (co + 3 < Cout) {
                    if (sizeof(T) == 2) *reinterpret_cast<uint2*>(op + co) = *reinterpret_cast<const uint2*>(pk);
                    else *reinterpret_cast<uint4*>(op + co) = *reinterpret_cast<const uint4*>(pk);
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (co + r < Cout) op[co + r] = pk[r];
                }
            }
        }
        return;
    }
    float s1[NT][4], s2[NT][4];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) s1[t][r] = s2[t][r] = 0.f;
#pragma unroll
    for (int m = 0; m < MTW; ++m) {
        const int h = h0 + wv * RW + m / MTR, w = w0 + (m % MTR) * 16 + l15;
        const bool ok = h < H && w < W;
        const size_t px = ((size_t)n * H + h) * W + w;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int co = co0 + t * 16 + kq * 4;
            // `op + co` is the lane's 4 channels; two destinations: a lane never straddles the split (a multiple of 4)
            T* op = out + px * Cout;
            if (fin.out1) op = co < fin.split ? out + px * fin.split : reinterpret_cast<T*>(fin.out1) + px * (Cout - fin.split) - fin.split;
            if (ok && co + 3 < Cout) {
                T pk[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float v = acc[m][t][r];
                    pk[r] = from_f32<T>(v);
                    if (RED) {      // dz = [y > 0] * (the gradient as the producer's backward will read it); sum dz, sum dz * (raw - mean)
                        const float x = rp[m][t].v[r];
                        const float dz = x * rsc[t][r] + rsh[t][r] > relu_keep_threshold<T>() ? to_f32(pk[r]) : 0.f;
                        s1[t][r] += dz;
                        s2[t][r] += dz * (x - rmu[t][r]);
                    } else {
                        s1[t][r] += v;
                        s2[t][r] += v * v;
                    }
                }
                if (sizeof(T) == 2) *reinterpret_cast<uint2*>(op + co) = *reinterpret_cast<const uint2*>(pk);
                else *reinterpret_cast<uint4*>(op + co) = *reinterpret_cast<const uint4*>(pk);
            } else if (ok) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (co + r < Cout) {
                        const float v = acc[m][t][r];
                        op[co + r] = from_f32<T>(v);
                        s1[t][r] += v;
                        s2[t][r] += v * v;
                    }
            }
        }
    }
    if (RED) stats = br.parts;
    if (stats) {
        __shared__ float sred[NW][2][COT];
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float a = s1[t][r], b = s2[t][r];
#pragma unroll
                for (int off = 1; off < 16; off <<= 1) {
                    a += __shfl_xor(a, off, 64);
                    b += __shfl_xor(b, off, 64);
                }
                if (l15 == 0) { sred[wv][0][t * 16 + kq * 4 + r] = a; sred[wv][1][t * 16 + kq * 4 + r] = b; }
            }
        __syncthreads();
        if (tid < COT && co0 + tid < Cout) {
            float a = sred[0][0][tid] + sred[1][0][tid] + sred[2][0][tid] + sred[3][0][tid];
            float b = sred[0][1][tid] + sred[1][1][tid] + sred[2][1][tid] + sred[3][1][tid];
#pragma unroll
            for (int q = 4; q < NW; ++q) { a += sred[q][0][tid]; b += sred[q][1][tid]; }
            if (RED) b *= br.saved[Cout + co0 + tid];          // sum dz * (raw - mean) -> sum dz * xhat
            if (!RED && fin.acc) {
                bn_acc_add(fin.acc + co0 + tid, fin.acc + 2 * Cout, a);
                bn_acc_add(fin.acc + Cout + co0 + tid, fin.acc + 2 * Cout, b);
            } else {
                store_part(&stats[((size_t)blockIdx.x * 2 + 0) * Cout + co0 + tid], a);
                store_part(&stats[((size_t)blockIdx.x * 2 + 1) * Cout + co0 + tid], b);
            }
        }
        if (!RED && fin.counter && last_block_arrives(fin.counter, gridDim.x * gridDim.y)) {   // the tile memory is dead: scratch for the sums
            bn_finish_block(stats, (int)gridDim.x, Cout, fin, reinterpret_cast<float*>(smem));
            last_block_done(fin.counter);
        }
    }
}

// One form of conv3x3_kernel on one tile shape.
template <typename TT, int COT, int TWW, int THH, bool POOL, bool BNL, bool RED, int NWW>
static void launch_conv3x3_kernel(dim3 grid, hipStream_t st, const ConvSrc& s, int N, int H, int W, const void* wpk, int Cout, void* out, float* stats,
                                  const BnFinish& fin, const BnLoad& bl, const BnRed& br) {
    const size_t lb = ((size_t)(THH + 2) * (TWW + 2) + 9 * COT) * Mma<TT>::KP * sizeof(TT);
    hipFuncSetAttribute((const void*)conv3x3_kernel<TT, COT, TWW, THH, POOL, BNL, RED, NWW>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lb);
    hipLaunchKernelGGL((conv3x3_kernel<TT, COT, TWW, THH, POOL, BNL, RED, NWW>), grid, dim3(64 * NWW), lb, st, s, N, H, W, (const TT*)wpk, Cout,
                       (TT*)out, stats, fin, bl, br);
}

// One tile shape in its fused forms (4 waves): BN loader, epilogue reduce, both; a pooled output has no reduce (conv3x3_fwd_impl).
template <typename TT, int COT, int TWW, int THH, bool POOL>
static int launch_tiled_bn(dim3 grid, hipStream_t st, const ConvSrc& s, int N, int H, int W, const void* wpk, int Cout, void* out, float* stats,
                           const BnFinish& fin, const BnLoad& bl, const BnRed& br) {
    if constexpr (POOL) launch_conv3x3_kernel<TT, COT, TWW, THH, true, true, false, 4>(grid, st, s, N, H, W, wpk, Cout, out, stats, fin, bl, br);
    else if (bl.gy && br.raw) launch_conv3x3_kernel<TT, COT, TWW, THH, false, true, true, 4>(grid, st, s, N, H, W, wpk, Cout, out, stats, fin, bl, br);
    else if (bl.gy) launch_conv3x3_kernel<TT, COT, TWW, THH, false, true, false, 4>(grid, st, s, N, H, W, wpk, Cout, out, stats, fin, bl, br);
    else launch_conv3x3_kernel<TT, COT, TWW, THH, false, false, true, 4>(grid, st, s, N, H, W, wpk, Cout, out, stats, fin, bl, br);
    return MISEG_OK;
}

// Every tile shape the library is built with, as a chain of `if (the run-time shape is this one) return F<T, COT, TW, TH, POOL>(args)`:
// the lists below name the candidates, tiled_shape_built (conv.h, beside the rule it follows from) keeps those a call can select -- a
// shape it rejects is not instantiated and ends in the message.  Expects cot, tw, th, pool in scope.
#define MISEG_TILED_SHAPE(F, TT, COT, TWW, THH, POOL, ...)                           \
    if constexpr (tiled_shape_built(std::is_same<TT, float>::value, COT, THH, POOL)) \
        if (cot == COT && tw == TWW && th == THH && pool == POOL) return F<TT, COT, TWW, THH, POOL>(__VA_ARGS__);
#define MISEG_TILED_TILES(F, TT, COT, POOL, ...)                                                                \
    MISEG_TILED_SHAPE(F, TT, COT, 32, 8, POOL, __VA_ARGS__) MISEG_TILED_SHAPE(F, TT, COT, 32, 16, POOL, __VA_ARGS__) \
    MISEG_TILED_SHAPE(F, TT, COT, 16, 8, POOL, __VA_ARGS__) MISEG_TILED_SHAPE(F, TT, COT, 16, 16, POOL, __VA_ARGS__)
#define MISEG_TILED_SELECT_16BIT(F, ...)                                                                                \
    MISEG_TILED_TILES(F, bf16, 16, false, __VA_ARGS__) MISEG_TILED_TILES(F, bf16, 32, false, __VA_ARGS__)               \
    MISEG_TILED_TILES(F, bf16, 64, false, __VA_ARGS__) MISEG_TILED_TILES(F, bf16, 64, true, __VA_ARGS__)                \
    return fail(MISEG_E_INVALID, "conv3x3: no tiled kernel with %d output channels per block, %d x %d tiles", cot, th, tw);
#define MISEG_TILED_SELECT_F32(F, ...)                                                                                  \
    MISEG_TILED_TILES(F, float, 16, false, __VA_ARGS__) MISEG_TILED_TILES(F, float, 32, false, __VA_ARGS__)             \
    return fail(MISEG_E_INVALID, "conv3x3: no tiled kernel with %d output channels per block, %d x %d tiles", cot, th, tw);

}  // namespace miseg
