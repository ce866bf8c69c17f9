// U-Net convolutions on gfx950 MFMA (ref: contrastyou/arch/unet.py:10-40, 66-84, 86-133): what the conv_*.hip units share.
//
// conv3x3 (stride 1, pad 1, no bias) as an implicit GEMM over NHWC activations:
//   M = 16-pixel row segments, N = output channels, reduction = 9 taps x input channels.
// The A operand is gathered straight from a haloed LDS tile of the input (a tap shift is a whole
// pixel = a whole channel vector, so fragments stay 16-byte aligned); nearest-x2 upsampling and
// the skip-connection concat are index math in the tile loader, never materialised.
// dt = bf16: v_mfma_f32_16x16x32_bf16; dt = f32: v_mfma_f32_16x16x4_f32 (exact fp32 parity mode).
// Weight gradients use the fp32 MFMA for both dtypes (deterministic split-K over pixels).
//
// One kernel family per translation unit (each compiled for bf16 and, with -DMISEG_F16_BUILD, for IEEE half):
//   conv_tiled.hip      conv3x3_kernel (16-bit storage, plain forms), conv3x3_pt_kernel               -> launch_conv_tiled
//   conv_tiled_bn.hip   conv3x3_kernel (16-bit storage, BatchNorm-loader / epilogue-reduce forms)    -> launch_conv_tiled_bn
//   conv_tiled_f32.hip  conv3x3_kernel (float, every form; bf16 build only)                          -> launch_conv_tiled_f32
//   conv_stream.hip     conv3x3_stream_kernel                                                         -> launch_conv_stream
//   conv_fwd.hip        conv3x3_fwd_impl and the forward / data-gradient entry points (no kernels)
//   conv_wgrad.hip      the three weight-gradient kernels, their reductions and entry points
//   conv_small.hip      weight packing, the 1x1 logits head, the stem
// The float instantiations exist in the bf16 build only: the fp16 build is entered through MISEG_F16_DISPATCH_ON alone, which
// forwards dt == MISEG_F16 calls re-labelled MISEG_BF16, so dt == MISEG_F32 never arrives there.
#pragma once
#include "common.h"

namespace miseg {

constexpr int kCT = 256;  // threads per block (4 waves)
constexpr int TH = 16;    // tile rows: 4 per wave
constexpr int CK = 32;    // input channels per LDS chunk

template <typename T> struct Mma;
template <> struct Mma<bf16> {
    static constexpr int CKP = 40;   // padded channel stride (elements): 80 B rows, 16-B aligned (2-way on ds_read_b128's lane groups)
    static constexpr int KP = 48;    // 96 B rows: the 16-lane groups of ds_read_b128 hit 64 distinct banks (conv3x3_kernel)
    static constexpr int VEC = 8;    // elements per 16-byte vector
    typedef s16x8 Frag;
    static __device__ __forceinline__ Frag load(const bf16* base, int kq) { return *reinterpret_cast<const Frag*>(base + 8 * kq); }
    static __device__ __forceinline__ void mma_chunk(const Frag& a, const Frag& b, f32x4& c) {
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
    }
};
template <> struct Mma<float> {
    static constexpr int CKP = 34;   // 2m+kq bank pattern: conflict-free ds_read_b32 gathers
    static constexpr int KP = 34;
    static constexpr int VEC = 4;
    struct Frag { float v[8]; };
    static __device__ __forceinline__ Frag load(const float* base, int kq) {
        Frag f;
#pragma unroll
        for (int s = 0; s < 8; ++s) f.v[s] = base[4 * s + kq];
        return f;
    }
    static __device__ __forceinline__ void mma_chunk(const Frag& a, const Frag& b, f32x4& c) {
#pragma unroll
        for (int s = 0; s < 8; ++s) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.v[s], b.v[s], c, 0, 0, 0);
    }
};

struct ConvSrc {
    const void* p0; const void* p1;
    int C0, C1, ups0, ups1;
};

template <typename T>
__device__ __forceinline__ void zero_vec(T* dst) {
#pragma unroll
    for (int i = 0; i < Mma<T>::VEC; ++i) dst[i] = from_f32<T>(0.f);
}

// ---- shape predicates and grids that more than one unit asks for.  `inline`, not `static`: the environment switches below are read
// once per build flavour, whichever unit asks first.
inline int tile_w(int64_t W) { return W >= 32 ? 32 : 16; }

// the persistent streaming kernel serves the HBM-bound bf16 shapes (one channel chunk, enough tiles to fill the chip)
inline bool conv_streams(int dt, int64_t Cin, int64_t N, int64_t H, int64_t W) {
    return dt == MISEG_BF16 && Cin <= CK && tile_w(W) == 32 && N * cdiv(H, TH) * cdiv(W, 32) >= 512;
}
inline int64_t stream_blocks(int64_t N, int64_t H, int64_t W) {
    static const int64_t cap = [] { const char* e = getenv("MISEG_STREAM_BLOCKS"); return e ? atoll(e) : 512LL; }();    // persistent blocks (2 per CU)
    return std::min<int64_t>(N * cdiv(H, TH) * cdiv(W, 32), cap);
}

// Grid of the persistent tiled kernel: `blocks` x-blocks of `per` consecutive tiles each (none empty), sized so that blocks.x * slices
// fills the chip once: two blocks per CU for the 8-row tiles (60 KB of LDS each), one for the 16-row tiles.
struct PtGrid { int blocks, per; };
inline PtGrid pt_grid(int ntiles, int slices, int th) {
    static const int per_cu = [] { const char* e = getenv("MISEG_PT_BLOCKS_PER_CU"); return e ? std::max(1, atoi(e)) : 2; }();     // diagnostic: 1, 3, 4 measured slower
    const int target = std::max(1, (256 * (th == 8 ? per_cu : 1)) / std::max(1, slices));
    const int per = std::max(1, (ntiles + target - 1) / target);
    return PtGrid{(ntiles + per - 1) / per, per};
}
inline bool tiled_persistent() {
    static const bool on = [] { const char* e = getenv("MISEG_CONV_PERSISTENT"); return !e || atoi(e) != 0; }();
    return on;
}

// tile height of the generic kernel (bf16): 8 rows from 64^2 upwards (smaller LDS tile -> two blocks per CU; measured
// 128^2 64->32: 78 -> 64 us), 16 rows for the small deep layers (32^2: 8-row tiles cost 46 -> 55 us) and for exact fp32
inline int generic_tile_h(int dt, int64_t H, int64_t W) {
    if (dt != MISEG_BF16) return 16;
    return H * W >= 64 * 64 ? 8 : 16;
}

// ---- the tiled kernel's tile shape for a call that does not stream: output channels per block (grid.y slices), tile width, tile
// height.  THE selection rule: conv3x3_fwd_impl launches by it, the parts queries count blocks by it (the tile does not depend on Cout
// or pool), and tiled_shape_built below is what it can return.  cot == 0: no such storage type.
struct TiledShape { int cot, tw, th; };
inline TiledShape tiled_shape(int dt, int64_t H, int64_t W, int64_t Cout, bool pool) {
    const int tw = tile_w(W), th = generic_tile_h(dt, H, W);
    int cot = 0;
    if (dt == MISEG_BF16 && pool) cot = 64;
    // 8-row tiles (maps from 64^2 up) take 32 output channels per block: with 64 the weight chunk makes the block's LDS 88 KB -- one
    // block per CU --, with 32 it is 60 KB and two fit (64^2, same box: 32->64 31.8 -> 26.7 us, 64->64 39.2 -> 36.3, 128->64 55.5 -> 49.9;
    // the 16-row tiles of the deep layers are one block per CU either way and lose 20 % with the narrower slice)
    else if (dt == MISEG_BF16) cot = Cout <= 16 ? 16 : (Cout <= 32 || th == 8) ? 32 : 64;
    else if (dt == MISEG_F32) cot = Cout <= 16 ? 16 : 32;
    return TiledShape{cot, tw, th};
}
// The shapes tiled_shape can return, i.e. the ones the three tiled units are built with (MISEG_TILED_SHAPE, conv_tiled.h):
//   16-bit: 16 and 32 channels per block on all four tiles, not pooled (a pooled output always takes 64);
//           64 not pooled on the 16-row tiles only (an 8-row tile takes 32); 64 pooled on all four tiles;
//   float:  16 and 32 on the 16-row tiles only (generic_tile_h), never pooled (sumpool_supported), never 64.
// (Of cot in {16, 32, 64}, th in {8, 16}; both tile widths always.)
constexpr bool tiled_shape_built(bool is_float, int cot, int th, bool pool) {
    if (is_float) return cot <= 32 && th == 16 && !pool;
    return cot <= 32 ? !pool : (pool || th == 16);
}

// pooled-output forms exist for the streaming shapes and, in the tiled kernel, for 16-bit storage with more than 32 output channels
inline bool sumpool_supported(int dt, int64_t Cin, int64_t N, int64_t H, int64_t W, int64_t Cout) {
    if (H % 2 || W % 2) return false;
    return conv_streams(dt, Cin, N, H, W) || (dt == MISEG_BF16 && Cout > 32);
}

// ---- the kernel units' launchers: run-time (dt, COT, TW, TH, POOL) / (COT, NV, DUAL, POOL) -> the instantiation.  MISEG_OK, or
// MISEG_E_INVALID for a shape the library is not built with.
// launch_conv_tiled serves every call; it hands float on to launch_conv_tiled_f32 and the 16-bit calls with a BatchNorm loader or an
// epilogue reduce to launch_conv_tiled_bn.
int launch_conv_tiled(int dt, int cot, int tw, int th, bool pool, dim3 grid, hipStream_t st, const ConvSrc& s, int N, int H, int W, const void* wpk,
                      int Cout, void* out, float* stats, const BnFinish& fin, const BnLoad& bl, const BnRed& br);
int launch_conv_tiled_bn(int cot, int tw, int th, bool pool, dim3 grid, hipStream_t st, const ConvSrc& s, int N, int H, int W, const void* wpk,
                         int Cout, void* out, float* stats, const BnFinish& fin, const BnLoad& bl, const BnRed& br);
int launch_conv_tiled_f32(int cot, int tw, int th, bool pool, dim3 grid, hipStream_t st, const ConvSrc& s, int N, int H, int W, const void* wpk,
                          int Cout, void* out, float* stats, const BnFinish& fin, const BnLoad& bl, const BnRed& br);
int launch_conv_stream(int cot, int nv, bool dual, bool pool, unsigned blocks, hipStream_t st, const ConvSrc& s, int N, int H, int W, const void* wpk,
                       int Cout, void* out, float* stats, const BnFinish& fin, const BnLoad& bl, const BnRed& br);

}  // namespace miseg
