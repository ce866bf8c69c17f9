// The streaming 3x3 convolution of the HBM-bound layers: conv3x3_stream_kernel (conv.h has the file map).
#include "conv.h"

namespace miseg {

// Streaming variant for the HBM-bound layers (Cin <= 32, bf16): persistent blocks walk tiles; the next tile's haloed input
// (NVEC 16-byte channel vectors per pixel) is fetched into registers while the current tile is on the matrix cores, and the
// weight chunk is staged once per block.  Same arithmetic, tile shape and output as conv3x3_kernel.  These layers are
// instruction-issue bound, so everything tile-invariant is hoisted: per-slot byte offsets relative to a per-tile base (buffer
// loads with a scalar base; out-of-image lanes get an out-of-range offset and read 0), a branch-free epilogue for interior
// tiles, and BN statistics accumulated over all tiles of the block (one stats part per block: parts = gridDim.x).
// Logical block id is XCD-major (hardware deals consecutive workgroup ids round-robin to the 8 XCDs), so the tiles one
// XCD works on in a sweep are contiguous and their halos hit that XCD's L2.
// DUAL (concat of two sources): slots are vector-major so that one load instruction reads one source.
typedef unsigned int u32x4v __attribute__((ext_vector_type(4)));
// POOL: the output leaves 2x2 sum-pooled ([N, H/2, W/2, Cout]; H, W even) -- the backward of a convolution whose input was read
// through a nearest x2 upsample: its data gradient at full resolution (4x the bytes of what is wanted) is never written; the four
// fp32 accumulators of a 2x2 block are added (two registers of the lane, then its neighbour's sum) and rounded once.
// BNL / RED: as in conv3x3_kernel.  The loader keeps the raw output and the activation gradient of the next tile in registers and
// forms graw when the tile is committed to LDS (coefficients staged in LDS once per block); the epilogue reduce reads the producer's
// raw output at the tile's output positions after the tile has left the matrix cores and adds it up one iteration late, from the
// packed gradient registers, just before they are stored.
template <int COT, int TW, int NVEC, bool DUAL, bool POOL = false, bool BNL = false, bool RED = false, int RW = 4>
__global__ __launch_bounds__(kCT, 2) void conv3x3_stream_kernel(ConvSrc src, int N, int H, int W, const bf16* __restrict__ wpk, int Cout,
                                                               bf16* __restrict__ out, float* __restrict__ stats, int ntiles, BnFinish fin,
                                                               BnLoad bl, BnRed br) {
    typedef bf16 T;
    typedef Mma<T> MM;
    static_assert(!BNL || (!DUAL && (NVEC == 1 || NVEC == 2 || NVEC == 4)), "BN loader: one source, a thread keeps one channel vector");
    static_assert(!(RED && POOL), "the epilogue reduce exists for full-resolution outputs");
    // RW rows of a tile per wave: 4 (16-row tiles), or 2 for the fused forms with 32 output or 32 input channels, whose
    // accumulators, packed outputs and second operand stream do not fit 256 registers at 4
    constexpr int THS = 4 * RW;
    static_assert(RW == 2 || RW == 4, "rows per wave");
    constexpr int CKP = MM::CKP, VEC = MM::VEC, NT = COT / 16, MTR = TW / 16, MTW = RW * MTR;
    // pixel stride of the input tile: 48 elements (24 dwords) makes the 16-lane groups of ds_read_b128 conflict-free
    // (40 is 2-way); taken where the larger tile still leaves two blocks per CU
    constexpr int IKP = COT == 16 ? 48 : CKP;
    constexpr int IW = TW + 2, IH = THS + 2, NPIX = IH * IW;
    constexpr int NPF = DUAL ? NVEC * ((NPIX + kCT - 1) / kCT) : (NPIX * NVEC + kCT - 1) / kCT;
    constexpr unsigned OOB = 0xFFFFFF00u;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    T* Is = reinterpret_cast<T*>(smem);                    // [IH][IW][IKP]
    T* Ws = Is + IH * IW * IKP;                            // [9][COT][CKP]
    float* Cf = reinterpret_cast<float*>(Ws + 9 * COT * CKP);   // BNL: [6][CK] loader coefficients; RED: + [3][COT] mean | scale | shift
    float* Rf = Cf + (BNL ? kBwdCoefRows * CK : 0);
    const int Cin = src.C0 + src.C1;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l15 = lane & 15, kq = lane >> 4;
    const int tilesC = (W + TW - 1) / TW, tilesR = (H + THS - 1) / THS;
    const int co0 = blockIdx.y * COT;
    const int G = gridDim.x;
    const int lb = (G % 8 == 0) ? (int)(blockIdx.x % 8) * (G / 8) + (int)(blockIdx.x / 8) : (int)blockIdx.x;
    if (BNL)
        for (int idx = tid; idx < kBwdCoefRows * CK; idx += kCT) {
            const int r = idx / CK, c = idx % CK;
            Cf[idx] = c < Cin ? bl.coef[(size_t)r * Cin + c] : 0.f;
        }
    if (RED)
        for (int idx = tid; idx < 3 * COT; idx += kCT) {
            const int r = idx / COT, c = co0 + idx % COT;
            Rf[idx] = c < Cout ? br.saved[(size_t)(r == 0 ? 0 : r + 1) * Cout + c] : 0.f;
        }

    // channels [Cin, CK) of the tile stay zero for the whole kernel; the weight chunk is loaded once
    for (int idx = tid; idx < NPIX * (CK / VEC); idx += kCT) {
        const int v = idx % (CK / VEC), px = idx / (CK / VEC);
        if (v >= NVEC) zero_vec<T>(Is + px * IKP + v * VEC);
    }
    for (int idx = tid; idx < 9 * COT * (CK / VEC); idx += kCT) {
        const int v = idx % (CK / VEC), co = (idx / (CK / VEC)) % COT, tap = idx / ((CK / VEC) * COT);
        const int c = v * VEC;
        T* dst = Ws + (tap * COT + co) * CKP + v * VEC;
        if (co0 + co >= Cout || c >= Cin) { zero_vec<T>(dst); continue; }
        *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(wpk + ((size_t)tap * Cout + co0 + co) * Cin + c);
    }

    // ---- tile-invariant slot tables: rel = byte offset from the tile base (pixel (h0-1, w0-1) of the source, after its x2
    // upsampling shift), yx = iy | ix << 8 (0xFFFF for an unused slot), ldso = element offset into Is
    const int hs0 = H >> src.ups0, ws0 = W >> src.ups0, hs1 = H >> src.ups1, ws1 = W >> src.ups1;
    unsigned rel[NPF], yx[NPF];          // yx also carries ldso in its upper half (one register per slot instead of two)
#pragma unroll
    for (int j = 0; j < NPF; ++j) {
        int v, px;
        if (DUAL) { v = j % NVEC; px = tid + kCT * (j / NVEC); }
        else { const int idx = tid + kCT * j; v = idx % NVEC; px = idx / NVEC; }
        const int ix = px % IW, iy = px / IW, c = v * VEC;
        const bool used = px < NPIX;
        const bool from1 = c >= src.C0;
        const int ups = from1 ? src.ups1 : src.ups0, wsz = from1 ? ws1 : ws0, Cs = from1 ? src.C1 : src.C0, cs = from1 ? c - src.C0 : c;
        const int ry = ((iy - 1) >> ups) + 1, rx = ((ix - 1) >> ups) + 1;     // >= 0
        rel[j] = (unsigned)(((ry * wsz + rx) * Cs + cs) * 2);
        yx[j] = (used ? (unsigned)(iy | (ix << 8)) : 0xFFFFu) | ((unsigned)(used ? px * IKP + v * VEC : 0) << 16);
        static_assert(NPIX * IKP < 65536, "ldso must fit 16 bits");
    }

    if (BNL || RED) __syncthreads();                       // Cf / Rf are read before the loop's first barrier
    u32x4v pf[NPF];
    u32x4v pg[BNL ? NPF : 1];
    auto fetch = [&](int tile) __attribute__((always_inline)) {
        const int tc = tile % tilesC, tr = (tile / tilesC) % tilesR, n = tile / (tilesC * tilesR);
        const int h0 = tr * THS, w0 = tc * TW;
        const int ylo = h0 == 0 ? 1 : 0, yhi = min(IH, H - h0 + 1), xlo = w0 == 0 ? 1 : 0, xhi = min(IW, W - w0 + 1);
        const long long b0 = ((((long long)n * hs0 + (h0 >> src.ups0) - 1) * ws0 + (w0 >> src.ups0) - 1) * src.C0) * 2;
        const __amdgpu_buffer_rsrc_t r0 = __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)src.p0 + b0), 0, 0x7FFFFFFF, 0x00020000);
        __amdgpu_buffer_rsrc_t r1 = r0;
        if (DUAL) {
            const long long b1 = ((((long long)n * hs1 + (h0 >> src.ups1) - 1) * ws1 + (w0 >> src.ups1) - 1) * src.C1) * 2;
            r1 = __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)src.p1 + b1), 0, 0x7FFFFFFF, 0x00020000);
        }
        if (BNL) r1 = __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)bl.gy + b0), 0, 0x7FFFFFFF, 0x00020000);   // same shape as the source
#pragma unroll
        for (int j = 0; j < NPF; ++j) {
            const int iy = yx[j] & 0xFF, ix = (yx[j] >> 8) & 0xFF;
            const bool ok = iy >= ylo && iy < yhi && ix >= xlo && ix < xhi;     // an unused slot has ix = 255
            const unsigned off = ok ? rel[j] : OOB;
            if (DUAL && (j % NVEC) * VEC >= src.C0) pf[j] = __builtin_amdgcn_raw_buffer_load_b128(r1, (int)off, 0, 0);
            else pf[j] = __builtin_amdgcn_raw_buffer_load_b128(r0, (int)off, 0, 0);
            if (BNL) pg[j] = __builtin_amdgcn_raw_buffer_load_b128(r1, (int)off, 0, 0);
        }
    };
    // BNL: graw of the tile's slots (zero outside the image) from (pf, pg) and this thread's channel vector of coefficients
    auto to_graw = [&](int tile) __attribute__((always_inline)) {
        const int tc = tile % tilesC, tr = (tile / tilesC) % tilesR;
        const int h0 = tr * THS, w0 = tc * TW;
        const int ylo = h0 == 0 ? 1 : 0, yhi = min(IH, H - h0 + 1), xlo = w0 == 0 ? 1 : 0, xhi = min(IW, W - w0 + 1);
        // two passes of four channels: 24 coefficient registers live instead of 48 (read from LDS here, every tile -- held across
        // the MFMA phase they would spill); the result replaces the raw output's half of pf in place
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            asm volatile("" ::: "memory");
            float4 cf[kBwdCoefRows];
#pragma unroll
            for (int r = 0; r < kBwdCoefRows; ++r) cf[r] = *reinterpret_cast<const float4*>(Cf + r * CK + (tid % NVEC) * VEC + 4 * hf);
            const float sc[4] = {cf[0].x, cf[0].y, cf[0].z, cf[0].w}, sh[4] = {cf[1].x, cf[1].y, cf[1].z, cf[1].w},
                        mu[4] = {cf[2].x, cf[2].y, cf[2].z, cf[2].w}, ca[4] = {cf[3].x, cf[3].y, cf[3].z, cf[3].w},
                        cp[4] = {cf[4].x, cf[4].y, cf[4].z, cf[4].w}, cq[4] = {cf[5].x, cf[5].y, cf[5].z, cf[5].w};
#pragma unroll
            for (int j = 0; j < NPF; ++j) {
                const int iy = yx[j] & 0xFF, ix = (yx[j] >> 8) & 0xFF;
                const bool ok = iy >= ylo && iy < yhi && ix >= xlo && ix < xhi;
                unsigned o2[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const unsigned ur = pf[j][2 * hf + i], ug = pg[j][2 * hf + i];
                    float res[2];
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        const float fr = bf16_bits_to_f32((unsigned short)(e ? ur >> 16 : ur & 0xffffu));
                        const float fg = bf16_bits_to_f32((unsigned short)(e ? ug >> 16 : ug & 0xffffu));
                        const int c = 2 * i + e;
                        const float lin = cp[c] + cq[c] * (fr - mu[c]);
                        res[e] = fr * sc[c] + sh[c] > relu_keep_threshold<T>() ? ca[c] * fg + lin : lin;
                    }
                    o2[i] = (unsigned)f32_to_bf16_bits(res[0]) | ((unsigned)f32_to_bf16_bits(res[1]) << 16);
                }
                pf[j][2 * hf] = ok ? o2[0] : 0u;
                pf[j][2 * hf + 1] = ok ? o2[1] : 0u;
            }
        }
    };

    // The epilogue of tile i is issued one iteration late (from packed registers), in front of the next loads: the
    // s_waitcnt vmcnt(0) guarding the register->LDS commit then only sees memory operations one MFMA phase old.
    constexpr int MPK = POOL ? MTW / 2 : MTW;            // POOL: (pooled row 0 / 1 of the wave's four rows) x (16-column block)
    uint2 pk[MPK][NT];
    float s1[NT][4], s2[NT][4];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) s1[t][r] = s2[t][r] = 0.f;
    int ptile = -1;
    uint2 rp[RED ? MTW : 1][RED ? NT : 1];       // RED: the producer's raw output at the previous tile's output positions
    auto load_red = [&](int tile) __attribute__((always_inline)) {
        const int tc = tile % tilesC, tr = (tile / tilesC) % tilesR, n = tile / (tilesC * tilesR);
        const int h0 = tr * THS, w0 = tc * TW;
        const T* rb = reinterpret_cast<const T*>(br.raw) + (((size_t)n * H + h0 + wv * RW) * W + w0 + l15) * Cout + co0 + kq * 4;
#pragma unroll
        for (int m = 0; m < MTW; ++m) {
            const int h = h0 + wv * RW + m / MTR, w = w0 + (m % MTR) * 16 + l15;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                uint2 q = make_uint2(0u, 0u);
                if (h < H && w < W && co0 + t * 16 + kq * 4 + 4 <= Cout)
                    q = *reinterpret_cast<const uint2*>(rb + ((size_t)(m / MTR) * W + (m % MTR) * 16) * Cout + t * 16);
                rp[m][t] = q;
            }
        }
    };
    auto store_prev = [&]() __attribute__((always_inline)) {
        const int tc = ptile % tilesC, tr = (ptile / tilesC) % tilesR, n = ptile / (tilesC * tilesR);
        const int h0 = tr * THS, w0 = tc * TW;
        const bool full = h0 + THS <= H && w0 + TW <= W && co0 + COT <= Cout;
        if (RED) {      // sums of dz = [y > 0] * (gradient as stored) and dz * (raw - mean) over the previous tile's valid outputs
            asm volatile("" ::: "memory");
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const float4 mu = *reinterpret_cast<const float4*>(Rf + t * 16 + kq * 4);
                const float4 sc = *reinterpret_cast<const float4*>(Rf + COT + t * 16 + kq * 4);
                const float4 sh = *reinterpret_cast<const float4*>(Rf + 2 * COT + t * 16 + kq * 4);
                const float mua[4] = {mu.x, mu.y, mu.z, mu.w}, sca[4] = {sc.x, sc.y, sc.z, sc.w}, sha[4] = {sh.x, sh.y, sh.z, sh.w};
                const bool cok = co0 + t * 16 + kq * 4 + 4 <= Cout;
#pragma unroll
                for (int m = 0; m < MTW; ++m) {
                    const int h = h0 + wv * RW + m / MTR, w = w0 + (m % MTR) * 16 + l15;
                    const bool ok = full || (h < H && w < W && cok);
                    const T* ge = reinterpret_cast<const T*>(&pk[m][t]);
                    const T* xe = reinterpret_cast<const T*>(&rp[m][t]);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float x = to_f32(xe[r]);
                        const float dz = (ok && x * sca[r] + sha[r] > relu_keep_threshold<T>()) ? to_f32(ge[r]) : 0.f;
                        s1[t][r] += dz;
                        s2[t][r] += dz * (x - mua[r]);
                    }
                }
            }
        }
        if (POOL) {     // even lanes hold the sums of their 2x2 block: pooled pixel (h0/2 + 2 wv + pr, w0/2 + 8 mc + l15/2)
            const int Hp = H >> 1, Wp = W >> 1;
#pragma unroll
            for (int mp = 0; mp < MPK; ++mp) {
                const int hp = (h0 >> 1) + wv * (RW / 2) + mp / MTR, wp = (w0 >> 1) + (mp % MTR) * 8 + (l15 >> 1);
                if ((l15 & 1) || hp >= Hp || wp >= Wp) continue;
                T* op = out + (((size_t)n * Hp + hp) * Wp + wp) * Cout + co0 + kq * 4;
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    if (fin.accumulate_out) {   // the output already holds another consumer's gradient of this tensor (ops._GradJoin)
                        const T* e = reinterpret_cast<const T*>(&pk[mp][t]);
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            if (co0 + t * 16 + kq * 4 + r < Cout) op[t * 16 + r] = from_f32<T>(to_f32(op[t * 16 + r]) + to_f32(e[r]));
                    } else if (co0 + t * 16 + kq * 4 + 4 <= Cout) *reinterpret_cast<uint2*>(op + t * 16) = pk[mp][t];
                    else {
                        const T* e = reinterpret_cast<const T*>(&pk[mp][t]);
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            if (co0 + t * 16 + kq * 4 + r < Cout) op[t * 16 + r] = e[r];
                    }
                }
            }
            return;
        }
        // per 16-channel tile t: where its lanes' 4 channels go and the pixel stride there (two destinations: fin.out1, see BnFinish;
        // the split is a multiple of 16, so a tile never straddles it)
        const size_t px0 = ((size_t)n * H + h0 + wv * RW) * W + w0 + l15;
        T* ot[NT];
        int ost[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int c = co0 + t * 16 + kq * 4;
            if (!fin.out1) { ot[t] = out + px0 * Cout + c; ost[t] = Cout; }
            else if (c < fin.split) { ot[t] = out + px0 * fin.split + c; ost[t] = fin.split; }
            else { ot[t] = reinterpret_cast<T*>(fin.out1) + px0 * (Cout - fin.split) + c - fin.split; ost[t] = Cout - fin.split; }
        }
        if (full) {
#pragma unroll
            for (int m = 0; m < MTW; ++m)
#pragma unroll
                for (int t = 0; t < NT; ++t)
                    *reinterpret_cast<uint2*>(ot[t] + ((size_t)(m / MTR) * W + (m % MTR) * 16) * ost[t]) = pk[m][t];
        } else {
#pragma unroll
            for (int m = 0; m < MTW; ++m) {
                const int h = h0 + wv * RW + m / MTR, w = w0 + (m % MTR) * 16 + l15;
                if (h < H && w < W) {
#pragma unroll
                    for (int t = 0; t < NT; ++t) {
                        const T* e = reinterpret_cast<const T*>(&pk[m][t]);
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            if (co0 + t * 16 + kq * 4 + r < Cout) ot[t][((size_t)(m / MTR) * W + (m % MTR) * 16) * ost[t] + r] = e[r];
                    }
                }
            }
        }
    };
    if (lb < ntiles) fetch(lb);
    for (int tile = lb; tile < ntiles; tile += G) {
        const int tc = tile % tilesC, tr = (tile / tilesC) % tilesR;
        const int h0 = tr * THS, w0 = tc * TW;
        if (BNL) to_graw(tile);                // in registers, before the barrier: overlaps the other waves' last MFMAs
        __syncthreads();                       // previous tile's MFMAs are done with Is
#pragma unroll
        for (int j = 0; j < NPF; ++j)
            if ((yx[j] & 0xFFFFu) != 0xFFFFu) *reinterpret_cast<u32x4v*>(Is + (yx[j] >> 16)) = pf[j];
        __syncthreads();
        if (ptile >= 0) store_prev();
        if (tile + G < ntiles) fetch(tile + G);

        f32x4 acc[MTW][NT];
#pragma unroll
        for (int m = 0; m < MTW; ++m)
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[m][t] = f32x4{0.f, 0.f, 0.f, 0.f};
        const T* Ib = Is + ((wv * RW) * IW + l15) * IKP + 8 * kq;   // all 72 A-fragment reads are this base + an immediate
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int ky = tap / 3, kx = tap % 3;
            typename MM::Frag bf[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) bf[t] = MM::load(Ws + (tap * COT + t * 16 + l15) * CKP, kq);
#pragma unroll
            for (int m = 0; m < MTW; ++m) {
                typename MM::Frag af = *reinterpret_cast<const typename MM::Frag*>(Ib + ((m / MTR + ky) * IW + (m % MTR) * 16 + kx) * IKP);
#pragma unroll
                for (int t = 0; t < NT; ++t) MM::mma_chunk(bf[t], af, acc[m][t]);
            }
        }
        // D^T[row = channel t*16 + kq*4 + r][col = pixel l15]: pack to bf16, accumulate the BN statistics of valid outputs
        const bool full = h0 + THS <= H && w0 + TW <= W && co0 + COT <= Cout;
        if (POOL) {
#pragma unroll
            for (int mp = 0; mp < MPK; ++mp) {
                const int m0 = (2 * (mp / MTR)) * MTR + mp % MTR, m1 = m0 + MTR;       // rows 2 pr and 2 pr + 1, same column block
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    T e[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float v = acc[m0][t][r] + acc[m1][t][r];
                        v += __shfl_xor(v, 1, 64);                                    // the column neighbour (lane l15 ^ 1)
                        e[r] = from_f32<T>(v);
                    }
                    pk[mp][t] = *reinterpret_cast<const uint2*>(e);
                }
            }
            ptile = tile;
            continue;
        }
#pragma unroll
        for (int m = 0; m < MTW; ++m) {
            const int h = h0 + wv * RW + m / MTR, w = w0 + (m % MTR) * 16 + l15;
            const bool ok = full || (h < H && w < W);
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                T e[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float v = acc[m][t][r];
                    e[r] = from_f32<T>(v);
                    if (!RED) {
                        const float vv = (full || (ok && co0 + t * 16 + kq * 4 + r < Cout)) ? v : 0.f;
                        s1[t][r] += vv;
                        s2[t][r] += vv * vv;
                    }
                }
                pk[m][t] = *reinterpret_cast<const uint2*>(e);
            }
        }
        ptile = tile;
        if (RED) load_red(tile);               // in flight across the next commit, consumed by store_prev
    }
    if (ptile >= 0) store_prev();
    if (RED) stats = br.parts;
    if (stats) {   // one part per block (zero for a block without tiles)
        __shared__ float sred[4][2][COT];
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
            float b = sred[0][1][tid] + sred[1][1][tid] + sred[2][1][tid] + sred[3][1][tid];
            if (RED) b *= br.saved[Cout + co0 + tid];          // sum dz * (raw - mean) -> sum dz * xhat
            const float a = sred[0][0][tid] + sred[1][0][tid] + sred[2][0][tid] + sred[3][0][tid];
            if (!RED && fin.acc) {
                bn_acc_add(fin.acc + co0 + tid, fin.acc + 2 * Cout, a);
                bn_acc_add(fin.acc + Cout + co0 + tid, fin.acc + 2 * Cout, b);
            } else {
                store_part(&stats[((size_t)blockIdx.x * 2 + 0) * Cout + co0 + tid], a);
                store_part(&stats[((size_t)blockIdx.x * 2 + 1) * Cout + co0 + tid], b);
            }
        }
        if (!RED && fin.counter && last_block_arrives(fin.counter, gridDim.x * gridDim.y)) {
            bn_finish_block(stats, (int)gridDim.x, Cout, fin, reinterpret_cast<float*>(smem));
            last_block_done(fin.counter);
        }
    }
}

// rows per wave of the streaming kernel's fused forms (see the kernel): 2 unless 16 gradient channels meet 16 outputs or a pooled output
template <int COT, int NV, bool POOL> constexpr int fused_rw() { return (NV == 2 && (COT == 16 || POOL)) ? 4 : 2; }
template <int COT, int NV, bool DU, bool POOL>
static int launch_stream(unsigned blocks, hipStream_t st, const ConvSrc& s, int N, int H, int W, const void* wpk, int Cout, void* out, float* stats,
                         const BnFinish& fin, const BnLoad& bl, const BnRed& br) {
    const dim3 grid(blocks, (unsigned)cdiv(Cout, COT));
#define GO(BNL, RED, RWW)                                                                                                            \
    {                                                                                                                               \
        const size_t lb = ((size_t)(4 * RWW + 2) * (32 + 2) * (COT == 16 ? 48 : Mma<bf16>::CKP) + 9 * COT * Mma<bf16>::CKP) * sizeof(bf16) + \
                          (BNL ? kBwdCoefRows * CK * 4 : 0) + (RED ? 3 * COT * 4 : 0);                                               \
        const int ntiles = (int)(N * cdiv(H, 4 * RWW) * cdiv(W, 32));                                                                \
        hipFuncSetAttribute((const void*)conv3x3_stream_kernel<COT, 32, NV, DU, POOL, BNL, RED, RWW>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lb); \
        hipLaunchKernelGGL((conv3x3_stream_kernel<COT, 32, NV, DU, POOL, BNL, RED, RWW>), grid, dim3(kCT), lb, st, s, N, H, W,          \
                           (const bf16*)wpk, Cout, (bf16*)out, stats, ntiles, fin, bl, br);                                          \
    }
    constexpr bool kFusable = !DU && (NV == 2 || NV == 4);      // the data-gradient shapes of the U-Net: 16 or 32 gradient channels
    if constexpr (kFusable) {
        constexpr int FRW = fused_rw<COT, NV, POOL>();
        if constexpr (POOL) { if (bl.gy) GO(true, false, FRW) else GO(false, false, 4) }
        else { if (bl.gy && br.raw) GO(true, true, FRW) else if (bl.gy) GO(true, false, FRW) else if (br.raw) GO(false, true, FRW) else GO(false, false, 4) }
    } else {
        if (bl.gy || br.raw) return fail(MISEG_E_INVALID, "conv3x3: BatchNorm loader / reduce not built for this streaming shape");
        GO(false, false, 4)
    }
#undef GO
    return MISEG_OK;
}

int launch_conv_stream(int cot, int nv, bool dual, bool pool, unsigned blocks, hipStream_t st, const ConvSrc& s, int N, int H, int W, const void* wpk,
                       int Cout, void* out, float* stats, const BnFinish& fin, const BnLoad& bl, const BnRed& br) {
    // every slot layout conv3x3_fwd_impl can ask for: two sources have 2-4 channel vectors between them and no pooled output
#define SHAPE(COT, NV, DU, POOL) \
    if (cot == COT && nv == NV && dual == DU && pool == POOL) return launch_stream<COT, NV, DU, POOL>(blocks, st, s, N, H, W, wpk, Cout, out, stats, fin, bl, br);
#define SHAPES(COT)                                                                                       \
    SHAPE(COT, 2, true, false) SHAPE(COT, 3, true, false) SHAPE(COT, 4, true, false)                          \
    SHAPE(COT, 1, false, false) SHAPE(COT, 2, false, false) SHAPE(COT, 3, false, false) SHAPE(COT, 4, false, false) \
    SHAPE(COT, 1, false, true) SHAPE(COT, 2, false, true) SHAPE(COT, 3, false, true) SHAPE(COT, 4, false, true)
    SHAPES(16) SHAPES(32)
#undef SHAPES
#undef SHAPE
    return fail(MISEG_E_INVALID, "conv3x3: no streaming kernel with %d output channels per block, %d channel vectors", cot, nv);
}

}  // namespace miseg
