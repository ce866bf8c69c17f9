// LocalClusterHead: S x (1x1 conv C->K + bias -> channel softmax / T), fused with the flip replay and
// the cat([flip(f_u), f_tf]) of the caller (ref: contrastyou/trainer/_utils.py:137-168,
// semi_seg/epocher.py:258-273).  Feature NHWC (dt) in, probabilities fp32 NCHW out (the layout the
// local-MI kernels consume).  One thread = one output pixel; logits staged per-thread in LDS columns
// (conflict-free), weights come through the scalar cache (wave-uniform indices).
//
// One kernel family per translation unit (each compiled for bf16 and, with -DMISEG_F16_BUILD, for IEEE half):
//   heads_fwd.hip        head_local_fwd_kernel, head_local_fwd_reg_kernel (16-bit storage), head_local_fwd_mfma_kernel;
//                        the entry point miseg_head_local_fwd
//   heads_bwd_fused.hip  head_local_bwd_fused_kernel (16-bit storage)                                  -> launch_head_bwd_fused
//   heads_bwd.hip        head_local_bwd_wave_kernel, sum_partials_kernel, head_local_bwd_impl, the backward entry points and queries
//   heads_f32.hip        head_local_fwd_kernel, head_local_fwd_reg_kernel, head_local_bwd_fused_kernel on float (bf16 build only)
//                                                      -> launch_head_fwd_lds_f32, launch_head_fwd_reg_f32, launch_head_bwd_fused_f32
// heads_fwd.h and heads_bwd_fused.h are the kernel templates that a 16-bit unit and heads_f32.hip instantiate on disjoint types.
// The float instantiations exist in the bf16 build only: dt == MISEG_F32 never reaches the fp16 build (conv.h).
#pragma once
#include "common.h"

namespace miseg {

typedef __bf16 bf16x8h_t __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4h_t __attribute__((ext_vector_type(4)));
#define HLDS_S16X4(ptr) ((__attribute__((address_space(3))) s16x4*)(ptr))

constexpr int kHT = 256;

template <typename T> struct Vec4;
template <> struct Vec4<float> { float4 v; __device__ float get(int i) const { return (&v.x)[i]; } };
template <> struct Vec4<bf16> { ushort4 v; __device__ float get(int i) const { return bf16_bits_to_f32((&v.x)[i]); } };

// MFMA operand of a C-channel feature row (head_local_fwd_mfma_kernel, head_local_bwd_wave_kernel)
template <int C> struct HeadFrag;
template <> struct HeadFrag<32> {
    typedef bf16x8h_t type;
    static __device__ __forceinline__ f32x4 mma(type a, type b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
};
template <> struct HeadFrag<16> {
    typedef bf16x4h_t type;
    static __device__ __forceinline__ f32x4 mma(type a, type b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_bit_cast(s16x4, a), __builtin_bit_cast(s16x4, b), c, 0, 0, 0);
    }
};
constexpr int kHeadZS = 132;   // floats per class row of a wave's transpose buffer (128 pixels + 4: conflict-free D writes)
template <int C> constexpr int head_mfma_cp() { return C + 8; }

inline int head_w_blocks(int64_t M, int64_t HW) { return (int)std::min<int64_t>(M * cdiv(HW, 64), 768); }

inline bool head_bwd_wave_shape(int dt, int64_t C, int64_t S, int64_t K) { return dt == MISEG_BF16 && K == 20 && C == 16 && S == 5; }

// ---- the kernel units' launchers: run-time shape -> the instantiation.  MISEG_OK, or MISEG_E_INVALID for a shape the library is
// not built with.  The entry points size the grid and the LDS; a launcher sets a kernel's attributes in the unit that defines it.
struct HeadFwd {      // a launch of head_local_fwd_kernel / head_local_fwd_reg_kernel (tol, viol: the latter only)
    dim3 grid; size_t lds; hipStream_t st;
    const void* feat; int H, W, C; const int32_t* src; const int32_t* flips; int M; const float* w; const float* b; int S, K; float invT;
    float* prob; float tol; int32_t* viol;
};
struct HeadBwdFused {      // a launch of head_local_bwd_fused_kernel
    int nblk; size_t lds; hipStream_t st;
    const void* feat; int H, W, C; const int32_t* src; const int32_t* flips; int M; const float* w; int S, K; float invT;
    const float* prob; const float* gprob; void* gfeat; float* partials; int accumulate;
};
int launch_head_fwd_lds_f32(const HeadFwd& a);
int launch_head_fwd_reg_f32(const HeadFwd& a, bool quad);
int launch_head_bwd_fused(const HeadBwdFused& a);
int launch_head_bwd_fused_f32(const HeadBwdFused& a);

}  // namespace miseg
