// The tiled 3x3 convolution, 16-bit storage, plain forms: conv3x3_kernel per tile, conv3x3_pt_kernel persistent (conv.h has the file map).
#include "conv_tiled.h"

namespace miseg {

// Persistent form of conv3x3_kernel for 16-bit storage (plain forms: no BatchNorm loader / epilogue reduce / last-block finish).
// conv3x3_kernel spends most of a block's life outside the matrix cores: a 64^2 layer with 32 input channels is ONE chunk per tile, so
// the first (and only) global fetch, the two barriers, the epilogue stores and the 2 x NT x 4 x 4-shuffle statistics reduction are all
// exposed, once per tile, three to six block generations per CU (profiles/r04a_bench_bf16_kernel_stats.csv: 1.06 ms per step at 15-26 %
// of the matrix peak).  Here a block owns a CONTIGUOUS run of tiles of one output-channel slice and software-pipelines across them:
//   * while the LAST chunk of tile i is on the matrix cores, chunk 0 of tile i + 1 (haloed input + weights) is already in flight in
//     registers, so the epilogue of tile i (stores, statistics) runs under that fetch instead of in front of it;
//   * BatchNorm statistics are kept per lane across the block's tiles and reduced once per block (one partial row per block:
//     parts = gridDim.x, which also shrinks what bn_finalize has to read);
//   * consecutive tiles of a block are spatial neighbours (their halos hit the XCD's L2 while still warm) and share the weight slice.
// Arithmetic, tile shape, LDS layout and epilogues are those of conv3x3_kernel; only the summation order of the statistics differs
// (per block over its tiles instead of per tile).
template <typename T, int COT, int TW, int THT, bool POOL, int NW, int DEPTH>
__global__ __launch_bounds__(64 * NW, 1) void conv3x3_pt_kernel(ConvSrc src, int N, int H, int W, const T* __restrict__ wpk, int Cout,
                                                           T* __restrict__ out, float* __restrict__ stats, BnFinish fin, int ntiles, int per) {
    static_assert(sizeof(T) == 2, "persistent tiled form: 16-bit storage types");
    static_assert(DEPTH == 1 || DEPTH == 2, "stages in flight ahead of the one on the matrix cores");
    typedef Mma<T> MM;
    constexpr int kCT = 64 * NW;
    static_assert(THT % NW == 0, "whole rows per wave");
    constexpr int VEC = MM::VEC, NT = COT / 16, MTR = TW / 16, RW = THT / NW, MTW = RW * MTR;
    constexpr int KP = MM::KP;
    constexpr int IW = TW + 2, IH = THT + 2;
    constexpr int NIS = (IH * IW * (CK / VEC) + kCT - 1) / kCT, NWS = (9 * COT * (CK / VEC) + kCT - 1) / kCT;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    T* Is = reinterpret_cast<T*>(smem);                    // [IH][IW][KP]
    T* Ws = Is + IH * IW * KP;                             // [9][COT][KP]
    const int Cin = src.C0 + src.C1;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l15 = lane & 15, kq = lane >> 4;
    const int tilesC = (W + TW - 1) / TW, tilesR = (H + THT - 1) / THT;
    const int co0 = blockIdx.y * COT;
    const int t_begin = blockIdx.x * per, t_end = min(t_begin + per, ntiles);
    const int nck = (Cin + CK - 1) / CK;

    // A STAGE = one 32-channel chunk of one tile (haloed input + weights).  DEPTH stages are in flight in registers ahead of the one
    // on the matrix cores, across tile boundaries: set A / set B alternate (static register names: the stage loop is unrolled by two).
    uint4 pinA[NIS], pwtA[NWS], pinB[DEPTH == 2 ? NIS : 1], pwtB[DEPTH == 2 ? NWS : 1];
    const uint4 zero4 = make_uint4(0u, 0u, 0u, 0u);
    // A thread's slots of the haloed input tile and of the weight slice never change: pixel, channel vector, tap, output channel.  Their
    // geometry is worked out once; a stage adds the tile's corner and the chunk's first channel (both block-uniform) and tests ranges.
    // (Derived per stage, the index math was most of this kernel's 6.4 vector instructions per MFMA: profiles/r04_pmc.json.)
    constexpr int CV4 = CK / VEC;
    int i_iy[NIS], i_ix[NIS], i_cv[NIS], i_rel0[NIS], i_rel1[NIS];       // row - 1, column - 1, channel offset in the chunk (< 0: no slot), offsets inside source 0 / 1
    int w_cv[NWS], w_rel[NWS];                                            // channel offset in the chunk (< 0: no slot), offset of (tap, co) in the packed weights
    {
        const int ws0 = W >> src.ups0, ws1 = W >> src.ups1;
#pragma unroll
        for (int j = 0; j < NIS; ++j) {
            const int idx = tid + kCT * j, v = idx % CV4, px = idx / CV4;
            i_ix[j] = px % IW - 1, i_iy[j] = px / IW - 1;
            i_cv[j] = idx < IH * IW * CV4 ? v * VEC : -1;
            // (h0 + d) >> ups = (h0 >> ups) + (d >> ups): tile corners are multiples of THT x TW, the shift is arithmetic (d = -1 stays outside)
            i_rel0[j] = ((i_iy[j] >> src.ups0) * ws0 + (i_ix[j] >> src.ups0)) * src.C0 + v * VEC;
            i_rel1[j] = ((i_iy[j] >> src.ups1) * ws1 + (i_ix[j] >> src.ups1)) * src.C1 + v * VEC - src.C0;
        }
#pragma unroll
        for (int j = 0; j < NWS; ++j) {
            const int idx = tid + kCT * j, v = idx % CV4, co = (idx / CV4) % COT, tap = idx / (CV4 * COT);
            w_cv[j] = (idx < 9 * COT * CV4 && co0 + co < Cout) ? v * VEC : -1;
            w_rel[j] = (tap * Cout + co0 + co) * Cin + v * VEC;
        }
    }
    auto fetch = [&](uint4 (&pin)[NIS], uint4 (&pwt)[NWS], int n, int h0, int w0, int c0) __attribute__((always_inline)) {
        const T* s0 = reinterpret_cast<const T*>(src.p0) + (((size_t)n * (H >> src.ups0) + (h0 >> src.ups0)) * (W >> src.ups0) + (w0 >> src.ups0)) * src.C0 + c0;
        const T* s1 = reinterpret_cast<const T*>(src.p1) + (((size_t)n * (H >> src.ups1) + (h0 >> src.ups1)) * (W >> src.ups1) + (w0 >> src.ups1)) * src.C1 + c0;
#pragma unroll
        for (int j = 0; j < NIS; ++j) {
            const int c = c0 + i_cv[j];
            uint4 val = zero4;
            if (i_cv[j] >= 0 && c < Cin && (unsigned)(h0 + i_iy[j]) < (unsigned)H && (unsigned)(w0 + i_ix[j]) < (unsigned)W)
                val = *reinterpret_cast<const uint4*>(c < src.C0 ? s0 + i_rel0[j] : s1 + i_rel1[j]);
            pin[j] = val;
        }
        const T* wc = wpk + c0;
#pragma unroll
        for (int j = 0; j < NWS; ++j) {
            uint4 val = zero4;
            if (w_cv[j] >= 0 && c0 + w_cv[j] < Cin) val = *reinterpret_cast<const uint4*>(wc + w_rel[j]);
            pwt[j] = val;
        }
    };
    const T* Ib = Is + ((wv * RW) * IW + l15) * KP;
    const T* Wb = Ws + l15 * KP;
    float s1[NT][4], s2[NT][4];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) s1[t][r] = s2[t][r] = 0.f;
    f32x4 acc[MTW][NT];

    // two cursors over the block's stages, both block-uniform (scalar unit): f = the next stage to FETCH, p = the stage to PROCESS
    struct Cur { int tile, ck, n, h0, w0; };
    auto decode = [&](Cur& c) __attribute__((always_inline)) {
        c.n = c.tile / (tilesC * tilesR); c.h0 = ((c.tile / tilesC) % tilesR) * THT; c.w0 = (c.tile % tilesC) * TW;
    };
    auto advance = [&](Cur& c) __attribute__((always_inline)) {
        if (++c.ck == nck) { c.ck = 0; ++c.tile; if (c.tile < t_end) decode(c); }
    };
    Cur f{t_begin, 0, 0, 0, 0}, p{t_begin, 0, 0, 0, 0};
    if (t_begin < t_end) { decode(f); p = f; }
    if (f.tile < t_end) { fetch(pinA, pwtA, f.n, f.h0, f.w0, 0); advance(f); }
    if constexpr (DEPTH == 2) {
        if (f.tile < t_end) { fetch(pinB, pwtB, f.n, f.h0, f.w0, f.ck * CK); advance(f); }
    }
    auto stage = [&](uint4 (&pin)[NIS], uint4 (&pwt)[NWS]) __attribute__((always_inline)) {
        if (p.ck == 0) {
#pragma unroll
            for (int m = 0; m < MTW; ++m)
#pragma unroll
                for (int t = 0; t < NT; ++t) acc[m][t] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        __syncthreads();                       // the previous stage's MFMAs are done with Is / Ws
#pragma unroll
        for (int j = 0; j < NIS; ++j) {
            const int idx = tid + kCT * j;
            if (idx < IH * IW * (CK / VEC)) *reinterpret_cast<uint4*>(Is + (idx / (CK / VEC)) * KP + (idx % (CK / VEC)) * VEC) = pin[j];
        }
#pragma unroll
        for (int j = 0; j < NWS; ++j) {
            const int idx = tid + kCT * j;
            if (idx < 9 * COT * (CK / VEC)) *reinterpret_cast<uint4*>(Ws + (idx / (CK / VEC)) * KP + (idx % (CK / VEC)) * VEC) = pwt[j];
        }
        __syncthreads();
        if (f.tile < t_end) { fetch(pin, pwt, f.n, f.h0, f.w0, f.ck * CK); advance(f); }      // this register set is free again: DEPTH stages ahead
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
        if (p.ck == nck - 1) {
            // ---- epilogue of this tile (conv3x3_kernel's): a lane owns 4 consecutive channels of one pixel
            const int n = p.n, h0 = p.h0, w0 = p.w0;
            if (POOL) {
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
                        if (co + 3 < Cout) *reinterpret_cast<uint2*>(op + co) = *reinterpret_cast<const uint2*>(pk);
                        else {
#pragma unroll
                            for (int r = 0; r < 4; ++r)
                                if (co + r < Cout) op[co + r] = pk[r];
                        }
                    }
                }
            } else {
#pragma unroll
                for (int m = 0; m < MTW; ++m) {
                    const int h = h0 + wv * RW + m / MTR, w = w0 + (m % MTR) * 16 + l15;
                    const bool ok = h < H && w < W;
                    const size_t px = ((size_t)n * H + h) * W + w;
#pragma unroll
                    for (int t = 0; t < NT; ++t) {
                        const int co = co0 + t * 16 + kq * 4;
                        T* op = out + px * Cout;
                        if (fin.out1) op = co < fin.split ? out + px * fin.split : reinterpret_cast<T*>(fin.out1) + px * (Cout - fin.split) - fin.split;
                        if (ok && co + 3 < Cout) {
                            T pk[4];
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const float v = acc[m][t][r];
                                pk[r] = from_f32<T>(v);
                                s1[t][r] += v;
                                s2[t][r] += v * v;
                            }
                            *reinterpret_cast<uint2*>(op + co) = *reinterpret_cast<const uint2*>(pk);
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
            }
        }
        advance(p);
    };
    while (p.tile < t_end) {
        stage(pinA, pwtA);
        if constexpr (DEPTH == 2) {
            if (p.tile >= t_end) break;
            stage(pinB, pwtB);
        }
    }
    if (!POOL && stats) {          // one partial row per block
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
            if (fin.acc) {
                bn_acc_add(fin.acc + co0 + tid, fin.acc + 2 * Cout, a);
                bn_acc_add(fin.acc + Cout + co0 + tid, fin.acc + 2 * Cout, b);
            } else {
                stats[((size_t)blockIdx.x * 2 + 0) * Cout + co0 + tid] = a;
                stats[((size_t)blockIdx.x * 2 + 1) * Cout + co0 + tid] = b;
            }
        }
    }
}

// One conv3x3_pt_kernel launch (4 waves: the persistent form serves 8-row tiles).
template <typename TT, int COT, int TWW, int THH, bool POOL, int DEPTH>
static void launch_conv3x3_pt_kernel(dim3 grid, hipStream_t st, const ConvSrc& s, int N, int H, int W, const void* wpk, int Cout, void* out, float* stats,
                                     const BnFinish& fin) {
    const size_t lb = ((size_t)(THH + 2) * (TWW + 2) + 9 * COT) * Mma<TT>::KP * sizeof(TT);
    const int ntiles = (int)grid.x;
    const PtGrid g = pt_grid(ntiles, (int)grid.y, THH);
    hipFuncSetAttribute((const void*)conv3x3_pt_kernel<TT, COT, TWW, THH, POOL, 4, DEPTH>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lb);
    hipLaunchKernelGGL((conv3x3_pt_kernel<TT, COT, TWW, THH, POOL, 4, DEPTH>), dim3((unsigned)g.blocks, grid.y), dim3(64 * 4), lb, st, s, N, H, W,
                       (const TT*)wpk, Cout, (TT*)out, stats, fin, ntiles, g.per);
}

// One tile shape in its plain forms (every call that gets here: launch_conv_tiled hands the fused ones on).  8-row tiles: persistent
// or 4 waves per tile; 16-row tiles: 8 waves per tile.
template <typename TT, int COT, int TWW, int THH, bool POOL>
static int launch_tiled(dim3 grid, hipStream_t st, const ConvSrc& s, int N, int H, int W, const void* wpk, int Cout, void* out, float* stats,
                        const BnFinish& fin, const BnLoad& bl, const BnRed& br) {
    if constexpr (THH == 8) {
        // the plain forms of the 8-row tiles (maps from 64^2 up: several tiles per block): persistent blocks, pipelined across tiles.
        // Measured per launch, same box: 32-channel slices 48.1 -> 38.7 us, pooled 64-channel 75.5 -> 67.6; the
        // 16-row tiles of the deep layers have one tile per block either way and ran 4-29 % slower in this form -> they keep the other
        if (!bl.gy && !br.raw && !fin.counter && tiled_persistent()) {
            // stages in flight ahead of the matrix cores: ONE.  Two (201 instead of 155 registers in the 32-channel-slice form) measured
            // 6.72 / 6.73 against 6.66 / 6.63 ms per step, same box, two alternations; MISEG_CONV_DEPTH=2 selects it
            if constexpr (!POOL) {      // (the pooled 64-channel form with two stages in flight needs 256 registers: one wave per SIMD)
                static const int depth = [] { const char* e = getenv("MISEG_CONV_DEPTH"); return e ? atoi(e) : 1; }();
                if (depth == 2) {
                    launch_conv3x3_pt_kernel<TT, COT, TWW, THH, POOL, 2>(grid, st, s, N, H, W, wpk, Cout, out, stats, fin);
                    return MISEG_OK;
                }
            }
            launch_conv3x3_pt_kernel<TT, COT, TWW, THH, POOL, 1>(grid, st, s, N, H, W, wpk, Cout, out, stats, fin);
            return MISEG_OK;
        }
        launch_conv3x3_kernel<TT, COT, TWW, THH, POOL, false, false, 4>(grid, st, s, N, H, W, wpk, Cout, out, stats, fin, bl, br);
    } else {
        // 16-row tiles of 16-bit layers: 8 waves (plain forms; the fused forms keep 4).  Same box, forward, us: 32^2 64->128 21.3 -> 20.6,
        // 128->128 29.4 -> 26.5, 256->128 45.4 -> 41.9; 16^2 128->256 19.0 -> 17.8, 256->256 27.4 -> 26.3
        launch_conv3x3_kernel<TT, COT, TWW, THH, POOL, false, false, 8>(grid, st, s, N, H, W, wpk, Cout, out, stats, fin, bl, br);
    }
    return MISEG_OK;
}

int launch_conv_tiled(int dt, int cot, int tw, int th, bool pool, dim3 grid, hipStream_t st, const ConvSrc& s, int N, int H, int W, const void* wpk,
                      int Cout, void* out, float* stats, const BnFinish& fin, const BnLoad& bl, const BnRed& br) {
    // the float kernels are in conv_tiled_f32.hip, a unit the fp16 build does not have
    // not built (tiled_shape_built): 64-channel slices of 8-row tiles, not pooled -- tiled_shape gives an 8-row tile 32
    MISEG_WITH_STORAGE_TYPE(dt, "conv3x3",
        if constexpr (std::is_same_v<TT, float>) return launch_conv_tiled_f32(cot, tw, th, pool, grid, st, s, N, H, W, wpk, Cout, out, stats, fin, bl, br);
        else if (bl.gy || br.raw) return launch_conv_tiled_bn(cot, tw, th, pool, grid, st, s, N, H, W, wpk, Cout, out, stats, fin, bl, br);
        else { MISEG_TILED_SELECT_16BIT(launch_tiled, grid, st, s, N, H, W, wpk, Cout, out, stats, fin, bl, br) });
    return MISEG_OK;
}

}  // namespace miseg
