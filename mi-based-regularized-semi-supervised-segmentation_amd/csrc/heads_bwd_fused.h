// The fused backward kernel of the local head and its launcher: heads_bwd_fused.hip instantiates it on the 16-bit type, heads_f32.hip
// on float (heads.h has the file map).
#pragma once
#include "heads.h"

namespace miseg {

// Fused backward of the local head (one pass over prob / gprob: no dz tensor in memory).  One block = one 64-pixel chunk at a time (persistent, strided):
//   phase 1 (VALU, streaming): dz[(s,k)][px] = p*(g - <g,p>)/T from prob/gprob (coalesced along pixels) -> LDS
//   phase 2 (fp32 MFMA):       gfeat[px][c] = sum_(s,k) dz[(s,k)][px] * W[(s,k)][c]     (M=px, N=c, Kred=S*K)
//   phase 3 (fp32 MFMA):       gw[(s,k)][c] += sum_px dz[(s,k)][px] * f[px][c]          (M=(s,k), N=c, Kred=px)
// gw / gb accumulate in registers across the block's chunks; one deterministic partial per block at the end.
// BF (bf16 features, K20 only): phases 2 and 3 run on v_mfma_f32_16x16x32_bf16 instead of the fp32 16x16x4 form (5x the MACs per
// matrix-pipe cycle).  dz is kept in LDS as two bf16 planes (hi + lo, 2^-16 relative), the weights as two transposed bf16 planes,
// the features are bf16 already (exact): gw = (dz_hi + dz_lo) . f, gfeat = W_hi.dz_hi + W_hi.dz_lo + W_lo.dz_hi (then rounded
// to bf16 anyway).  The fp32 build keeps the exact fp32 MFMA path.
template <typename T, int CTM, int RW, bool K20, bool BF>   // K20: K == 20 and S*K <= 100 -> a row's sub-head is i / 5, a compile-time index
__global__ __launch_bounds__(256, (CTM == 1 ? 3 : 2)) void head_local_bwd_fused_kernel(const T* __restrict__ feat, int H, int W, int C,
                                                                   const int32_t* __restrict__ src, const int32_t* __restrict__ flips,
                                                                   int M, const float* __restrict__ w, int S, int K, float invT,
                                                                   const float* __restrict__ prob, const float* __restrict__ gprob,
                                                                   T* __restrict__ gfeat, float* __restrict__ partials, int nblk, int accumulate) {
    extern __shared__ float sm[];
    const int R = S * K, RT = (R + 15) / 16, RP = RT * 16, CT = (C + 15) / 16, HW = H * W;
    constexpr int DZS = 65;
    constexpr int FPT = CTM * 4;              // feature values per thread: 64 px * (CTM*16) channels / 256 threads
    const int FS = C + 1, WS = C + 1;
    constexpr int RPB = 128, DZB = 72, WTB = 136, CP = CTM * 16;   // BF layout: rows padded to 4 k-steps of 32; strides conflict-free for b128
    float* dzs = sm;                          // [RP][DZS]   p*g, then dz; rows >= R zero
    float* fs = dzs + (size_t)RP * DZS;       // [64][FS]    feature chunk (fp32)
    float* wsm = fs + (size_t)64 * FS;        // [RP][WS]    head weights, rows >= R zero
    float* dots = wsm + (size_t)RP * WS;      // [4 waves][S][64]  partial <g,p> per (wave, sub-head, pixel); generic path: [S][64]
    unsigned short* dzb = reinterpret_cast<unsigned short*>(sm);      // BF: [2][RPB][DZB]  dz hi | lo (bf16 bits), rows >= R zero
    unsigned short* fsT = dzb + 2 * RPB * DZB;                         // BF: [CP][DZB]      features transposed [c][px]
    unsigned short* wT = fsT + CP * DZB;                               // BF: [2][CP][WTB]   W^T hi | lo: [c][r], r >= R zero
    if (BF) dots = reinterpret_cast<float*>(wT + 2 * CP * WTB);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l15 = lane & 15, kq = lane >> 4;
    if (BF) {
        for (int idx = tid; idx < 2 * RPB * DZB; idx += 256) dzb[idx] = 0;
        for (int idx = tid; idx < CP * DZB; idx += 256) fsT[idx] = 0;
        for (int idx = tid; idx < CP * WTB; idx += 256) {
            const int c = idx / WTB, r = idx - c * WTB;
            const float v = (r < R && c < C) ? w[(size_t)r * C + c] : 0.f;
            const unsigned short hi = f32_to_bf16_bits(v);
            wT[idx] = hi;
            wT[CP * WTB + idx] = f32_to_bf16_bits(v - bf16_bits_to_f32(hi));
        }
    } else {
        for (int idx = tid; idx < RP * C; idx += 256) {
            const int c = idx % C, r = idx / C;
            wsm[r * WS + c] = r < R ? w[(size_t)r * C + c] : 0.f;
        }
        for (int idx = tid; idx < (RP - R) * 64; idx += 256) dzs[(R + idx / 64) * DZS + (idx & 63)] = 0.f;
    }
    constexpr int NA = K20 ? 2 : 4;   // row tiles per wave: 7 tiles (R <= 112) over 4 waves with K20, up to 16 otherwise
    f32x4 accw[NA][CTM];   // gw: row tiles rt = wv + 4a, column tiles c
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
        for (int c = 0; c < CTM; ++c) accw[a][c] = f32x4{0.f, 0.f, 0.f, 0.f};
    float gbacc = 0.f;
    float gbr[K20 ? 25 : 1];                  // K20: per-lane partial sums of dz per owned row, reduced across the wave at the end
#pragma unroll
    for (int i = 0; i < (K20 ? 25 : 1); ++i) gbr[i] = 0.f;
    int fq[FPT], fc[FPT];                     // chunk-invariant (pixel, channel) of this thread's feature slots
#pragma unroll
    for (int j = 0; j < FPT; ++j) { const int idx = tid + 256 * j; fq[j] = idx / C; fc[j] = idx - fq[j] * C; }
    const int chunksPerM = (HW + 63) / 64;
    const int64_t nchunks = (int64_t)M * chunksPerM;
    const uint32_t kmagic = (65536u + (uint32_t)K - 1u) / (uint32_t)K;   // r / K == (r * kmagic) >> 16 for r*K < 65536
    const int px = lane;
    // Rows r = wv + 4i of (s,k) belong to wave wv: every wave streams ~R/4 coalesced 256-byte row segments of prob and
    // gprob per chunk.  The chunk's values live in registers and are fetched one chunk ahead (issued before the MFMA
    // phases of the current chunk), so the HBM latency hides behind phases 2/3.
    // NOTHING in fetch() may read a loaded value: a select or a conversion right after the load makes the compiler wait for it,
    // and 50 loads then cost 50 serial memory latencies (measured: 28 k of a chunk's 52 k cycles).  Dead pixels get an
    // out-of-range buffer offset (the hardware returns 0); features stay raw T until phase 1.
    float pr[RW], gr[RW];
    T fr[FPT];
    const int wvu = __builtin_amdgcn_readfirstlane(wv);   // wave-uniform: row offsets below stay in SGPRs
    const size_t tot = (size_t)S * M * K * HW;            // floats in prob / gprob (host checks tot*4 < 2^32)
    auto fetch = [&](int64_t ch) {
        const int m = ch / chunksPerM, p0 = (ch % chunksPerM) * 64;
        const bool live = p0 + px < HW;
        const int voff = live ? px * 4 : (int)0x80000000;   // past num_records for any chunk
        // one buffer resource per chunk (uniform base), row offsets as scalar soffsets, px as the only VGPR offset
        const size_t boff = (size_t)m * K * HW + p0;
        const uint32_t rem = (uint32_t)((tot - boff) * 4);
        const __amdgpu_buffer_rsrc_t rp = __builtin_amdgcn_make_buffer_rsrc((void*)(prob + boff), 0, (int)rem, 0x00020000);
        const __amdgpu_buffer_rsrc_t rg = __builtin_amdgcn_make_buffer_rsrc((void*)(gprob + boff), 0, (int)rem, 0x00020000);
#pragma unroll
        for (int i = 0; i < RW; ++i) {
            const int r = min(wvu + 4 * i, R - 1);   // rows past R re-read row R-1 (branch-free issue); never stored
            const int sidx = (int)(((uint32_t)r * kmagic) >> 16);
            const uint32_t so = ((uint32_t)r + (uint32_t)sidx * (uint32_t)(M - 1) * (uint32_t)K) * (uint32_t)HW * 4u;
            pr[i] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rp, voff, (int)so, 0));
            gr[i] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rg, voff, (int)so, 0));
        }
        const int f = flips ? flips[m] : 0;
        const size_t fb = (size_t)src[m] * HW;
#pragma unroll
        for (int j = 0; j < FPT; ++j) {
            const int idx = tid + 256 * j, c = fc[j], q = fq[j];
            const bool ok = idx < 64 * C && p0 + q < HW;
            const int pq = ok ? p0 + q : 0, h = pq / W, wq = pq - h * W;
            fr[j] = feat[ok ? (fb + (size_t)flip_h(h, H, f) * W + flip_w(wq, W, f)) * C + c : 0];   // dead slots re-read element 0; masked at use
        }
    };
    if ((int64_t)blockIdx.x < nchunks) fetch(blockIdx.x);
    for (int64_t ch = blockIdx.x; ch < nchunks; ch += nblk) {
        const int m = ch / chunksPerM, p0 = (ch % chunksPerM) * 64;
        const int f = flips ? flips[m] : 0;
        __syncthreads();   // previous chunk's MFMA phases are done with dzs / fs
        // ---- phase 1: dz = p*(g - <g,p>)/T
        if (K20) {
            // <g,p> per sub-head from the wave's own registers: rows r = wv + 4i, sub-head i / 5 (5 rows of each sub-head per
            // wave); the four waves' partials meet in LDS.  No p*g round trip through LDS, the work is the same on every wave.
            float part[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int i = 0; i < 25; ++i) part[i / 5] = fmaf(pr[i], gr[i], part[i / 5]);
#pragma unroll
            for (int sh = 0; sh < 5; ++sh) dots[(wvu * 5 + sh) * 64 + px] = part[sh];
        } else {
#pragma unroll
            for (int i = 0; i < RW; ++i) {
                const int r = wvu + 4 * i;
                if (r < R) dzs[r * DZS + px] = pr[i] * gr[i];
            }
        }
#pragma unroll
        for (int j = 0; j < FPT; ++j)
            if (tid + 256 * j < 64 * C) {
                if (BF) fsT[fc[j] * DZB + fq[j]] = (p0 + fq[j] < HW) ? *reinterpret_cast<const unsigned short*>(&fr[j]) : (unsigned short)0;
                else fs[fq[j] * FS + fc[j]] = (p0 + fq[j] < HW) ? to_f32(fr[j]) : 0.f;
            }
        __syncthreads();
        if (K20) {
            float dot[5];
#pragma unroll
            for (int sh = 0; sh < 5; ++sh)
                dot[sh] = (sh < S) ? ((dots[(0 * 5 + sh) * 64 + px] + dots[(1 * 5 + sh) * 64 + px]) + (dots[(2 * 5 + sh) * 64 + px] + dots[(3 * 5 + sh) * 64 + px])) : 0.f;
#pragma unroll
            for (int i = 0; i < 25; ++i) {
                const int r = wvu + 4 * i;
                const float dz = pr[i] * (gr[i] - dot[i / 5]) * invT;
                if (r < R) {
                    if (BF) {
                        const unsigned short hi = f32_to_bf16_bits(dz);
                        dzb[r * DZB + px] = hi;
                        dzb[(RPB + r) * DZB + px] = f32_to_bf16_bits(dz - bf16_bits_to_f32(hi));
                    } else {
                        dzs[r * DZS + px] = dz;
                    }
                    gbr[i] += dz;
                }
            }
            if (ch + nblk < nchunks) fetch(ch + nblk);
            __syncthreads();
        } else {
            for (int sidx = wv; sidx < S; sidx += 4) {
                float dot = 0.f;
#pragma unroll 4
                for (int k = 0; k < K; ++k) dot += dzs[(sidx * K + k) * DZS + px];
                dots[sidx * 64 + px] = dot;
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < RW; ++i) {
                const int r = wvu + 4 * i;
                const int sidx = (int)(((uint32_t)r * kmagic) >> 16);
                if (r < R) dzs[r * DZS + px] = pr[i] * (gr[i] - dots[sidx * 64 + px]) * invT;
            }
            if (ch + nblk < nchunks) fetch(ch + nblk);
            __syncthreads();
            if (tid < R) {
                float a = 0.f;
#pragma unroll 8
                for (int q = 0; q < 64; ++q) a += dzs[tid * DZS + q];
                gbacc += a;
            }
        }
        // ---- phase 2: gfeat tile [64 px][C]: wave wv owns pixel tile wv (16 px).  Operands swapped so that D^T comes out:
        // a lane holds 4 consecutive channels of one pixel -> one 8-byte (bf16) / 16-byte (fp32) store.  Plain stores: every
        // gfeat element has exactly one writer (distinct src per window, see the entry point) and the buffer arrives zeroed.
        if (gfeat) {
            f32x4 accf[CTM];
#pragma unroll
            for (int c = 0; c < CTM; ++c) accf[c] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (BF) {
                // D[c][px] = sum_r W^T[c][r] dz[r][px]: A = W^T rows (b128), B = dz columns through the transposing LDS read
                // (lane 4*qq+pq of a 16-lane group reads 4 pixels of row k0+qq and receives its own pixel's 4 rows)
                const int qq = l15 >> 2, pq = l15 & 3;
#pragma unroll
                for (int ks = 0; ks < RPB / 32; ++ks) {
                    bf16x8h_t bz[2];
#pragma unroll
                    for (int pl = 0; pl < 2; ++pl) {
                        const unsigned short* b0 = dzb + (size_t)(pl * RPB + ks * 32 + 8 * kq + qq) * DZB + wv * 16 + 4 * pq;
                        const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(HLDS_S16X4(b0));
                        const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(HLDS_S16X4(b0 + 4 * DZB));
                        const s16x8 fv = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                        bz[pl] = __builtin_bit_cast(bf16x8h_t, fv);
                    }
#pragma unroll
                    for (int c = 0; c < CTM; ++c) {
                        const unsigned short* a0 = wT + (size_t)(c * 16 + l15) * WTB + ks * 32 + 8 * kq;
                        const bf16x8h_t whi = *reinterpret_cast<const bf16x8h_t*>(a0);
                        const bf16x8h_t wlo = *reinterpret_cast<const bf16x8h_t*>(a0 + CP * WTB);
                        accf[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wlo, bz[0], accf[c], 0, 0, 0);
                        accf[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(whi, bz[1], accf[c], 0, 0, 0);
                        accf[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(whi, bz[0], accf[c], 0, 0, 0);
                    }
                }
            } else {
#pragma unroll 7
                for (int ks = 0; ks < RP; ks += 4) {
                    const float av = dzs[(ks + kq) * DZS + wv * 16 + l15];
#pragma unroll
                    for (int c = 0; c < CTM; ++c)
                        if (c < CT) {
                            const float bv = wsm[(ks + kq) * WS + min(c * 16 + l15, C - 1)];
                            accf[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(bv, av, accf[c], 0, 0, 0);
                        }
                }
            }
            // D^T[row = channel c*16 + kq*4 + r][col = pixel l15]
            const int pq = p0 + wv * 16 + l15;
            if (pq < HW) {
                const int h = pq / W, wq = pq % W;
                T* gp = gfeat + ((size_t)src[m] * HW + (size_t)flip_h(h, H, f) * W + flip_w(wq, W, f)) * C;
#pragma unroll
                for (int c = 0; c < CTM; ++c) {
                    const int cc = c * 16 + kq * 4;
                    if (c < CT && accumulate) {      // gfeat holds another consumer's gradient of the feature (ops._GradJoin): add, round once
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            if (cc + r < C) gp[cc + r] = from_f32<T>(accf[c][r] + to_f32(gp[cc + r]));
                    } else if (c < CT && cc + 3 < C) {
                        T pk[4];
#pragma unroll
                        for (int r = 0; r < 4; ++r) pk[r] = from_f32<T>(accf[c][r]);
                        if (sizeof(T) == 2) *reinterpret_cast<uint2*>(gp + cc) = *reinterpret_cast<const uint2*>(pk);
                        else *reinterpret_cast<uint4*>(gp + cc) = *reinterpret_cast<const uint4*>(pk);
                    } else if (c < CT) {
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            if (cc + r < C) gp[cc + r] = from_f32<T>(accf[c][r]);
                    }
                }
            }
        }
        // ---- phase 3: gw += dz * f
        if (BF) {
            // D[r][c] = sum_px dz[r][px] f[px][c]: A = dz rows (hi, lo planes), B = transposed features, both plain b128 reads
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                bf16x8h_t bf_[CTM];
#pragma unroll
                for (int c = 0; c < CTM; ++c) bf_[c] = *reinterpret_cast<const bf16x8h_t*>(fsT + (size_t)(c * 16 + l15) * DZB + ks * 32 + 8 * kq);
#pragma unroll
                for (int a = 0; a < 2; ++a) {
                    const int rt = wv + 4 * a;           // 7 row tiles over 4 waves
                    if (rt < RT) {
                        const unsigned short* a0 = dzb + (size_t)(rt * 16 + l15) * DZB + ks * 32 + 8 * kq;
                        const bf16x8h_t dhi = *reinterpret_cast<const bf16x8h_t*>(a0);
                        const bf16x8h_t dlo = *reinterpret_cast<const bf16x8h_t*>(a0 + (size_t)RPB * DZB);
#pragma unroll
                        for (int c = 0; c < CTM; ++c) {
                            accw[a][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dlo, bf_[c], accw[a][c], 0, 0, 0);
                            accw[a][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dhi, bf_[c], accw[a][c], 0, 0, 0);
                        }
                    }
                }
            }
        } else
#pragma unroll 4
        for (int ks = 0; ks < 64; ks += 4) {
            float bfr[CTM];
#pragma unroll
            for (int c = 0; c < CTM; ++c) bfr[c] = (c < CT) ? fs[(ks + kq) * FS + min(c * 16 + l15, C - 1)] : 0.f;
#pragma unroll
            for (int a = 0; a < NA; ++a) {
                const int rt = wv + 4 * a;
                if (rt < RT) {
                    const float av = dzs[(rt * 16 + l15) * DZS + ks + kq];
#pragma unroll
                    for (int c = 0; c < CTM; ++c)
                        if (c < CT) accw[a][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bfr[c], accw[a][c], 0, 0, 0);
                }
            }
        }
    }
    float* out = partials + (size_t)blockIdx.x * (R * C + R);
#pragma unroll
    for (int a = 0; a < NA; ++a) {
        const int rt = wv + 4 * a;
        if (rt < RT) {
#pragma unroll
            for (int c = 0; c < CTM; ++c)
                if (c < CT) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        int row = rt * 16 + kq * 4 + r, col = c * 16 + l15;
                        if (row < R && col < C) out[row * C + col] = accw[a][c][r];
                    }
                }
        }
    }
    if (K20) {
#pragma unroll
        for (int i = 0; i < 25; ++i) {
            const float v = wave_sum(gbr[i]);
            if (lane == 0 && wvu + 4 * i < R) out[R * C + wvu + 4 * i] = v;
        }
    } else if (tid < R) out[R * C + tid] = gbacc;
}

template <typename TT, int CTM, int RW, bool K20V, bool BFV>
int launch_head_bwd_fused_kernel(const HeadBwdFused& a) {
    hipFuncSetAttribute((const void*)head_local_bwd_fused_kernel<TT, CTM, RW, K20V, BFV>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)a.lds);
    hipLaunchKernelGGL((head_local_bwd_fused_kernel<TT, CTM, RW, K20V, BFV>), dim3(a.nblk), dim3(256), a.lds, a.st, (const TT*)a.feat, a.H, a.W, a.C,
                       a.src, a.flips, a.M, a.w, a.S, a.K, a.invT, a.prob, a.gprob, (TT*)a.gfeat, a.partials, a.nblk, a.accumulate);
    return MISEG_OK;
}

template <typename TT, int CTM>
int launch_head_bwd_fused_rows(const HeadBwdFused& a) {
    const int R = a.S * a.K;
    if constexpr (sizeof(TT) == 2 && CTM == 2)      // the one bf16-MFMA form that a call can select: no other is instantiated
        if (a.K == 20 && R <= 100 && a.C == 32)     // 16 channels: HBM-bound either way and the bf16 variant does not fit 3 blocks per CU
            return launch_head_bwd_fused_kernel<TT, CTM, 25, true, true>(a);
    if (a.K == 20 && R <= 100) return launch_head_bwd_fused_kernel<TT, CTM, 25, true, false>(a);
    if (R <= 112) return launch_head_bwd_fused_kernel<TT, CTM, 28, false, false>(a);
    return launch_head_bwd_fused_kernel<TT, CTM, 64, false, false>(a);
}

template <typename TT>
int launch_head_bwd_fused_t(const HeadBwdFused& a) {
    if (a.C <= 16) return launch_head_bwd_fused_rows<TT, 1>(a);
    if (a.C <= 32) return launch_head_bwd_fused_rows<TT, 2>(a);
    if (a.C <= 64) return launch_head_bwd_fused_rows<TT, 4>(a);
    if (a.C <= 128) return launch_head_bwd_fused_rows<TT, 8>(a);
    return MISEG_E_INVALID;
}

}  // namespace miseg
