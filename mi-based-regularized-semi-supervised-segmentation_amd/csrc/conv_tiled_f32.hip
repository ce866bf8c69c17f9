// The tiled 3x3 convolution in exact fp32 (the parity mode): every form of conv3x3_kernel on float.  Built once -- the fp16 build
// has no such unit (conv.h has the file map).
#include "conv_tiled.h"

namespace miseg {

template <typename TT, int COT, int TWW, int THH, bool POOL>
static int launch_tiled_f32(dim3 grid, hipStream_t st, const ConvSrc& s, int N, int H, int W, const void* wpk, int Cout, void* out, float* stats,
                            const BnFinish& fin, const BnLoad& bl, const BnRed& br) {
    if (bl.gy || br.raw) return launch_tiled_bn<TT, COT, TWW, THH, POOL>(grid, st, s, N, H, W, wpk, Cout, out, stats, fin, bl, br);
    launch_conv3x3_kernel<TT, COT, TWW, THH, POOL, false, false, 4>(grid, st, s, N, H, W, wpk, Cout, out, stats, fin, bl, br);
    return MISEG_OK;
}

int launch_conv_tiled_f32(int cot, int tw, int th, bool pool, dim3 grid, hipStream_t st, const ConvSrc& s, int N, int H, int W, const void* wpk,
                          int Cout, void* out, float* stats, const BnFinish& fin, const BnLoad& bl, const BnRed& br) {
    // not built (tiled_shape_built): 8-row tiles -- generic_tile_h gives float 16 rows at every size
    MISEG_TILED_SELECT_F32(launch_tiled_f32, grid, st, s, N, H, W, wpk, Cout, out, stats, fin, bl, br)
}

}  // namespace miseg
