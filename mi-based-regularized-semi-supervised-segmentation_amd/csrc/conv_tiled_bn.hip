// The tiled 3x3 convolution with the BatchNorm backward folded in, 16-bit storage: the BNL / RED forms of conv3x3_kernel (conv.h has
// the file map).
#include "conv_tiled.h"

namespace miseg {

int launch_conv_tiled_bn(int cot, int tw, int th, bool pool, dim3 grid, hipStream_t st, const ConvSrc& s, int N, int H, int W, const void* wpk,
                         int Cout, void* out, float* stats, const BnFinish& fin, const BnLoad& bl, const BnRed& br) {
    // not built (tiled_shape_built): 64-channel slices of 8-row tiles, not pooled -- tiled_shape gives an 8-row tile 32
    MISEG_TILED_SELECT_16BIT(launch_tiled_bn, grid, st, s, N, H, W, wpk, Cout, out, stats, fin, bl, br)
}

}  // namespace miseg
