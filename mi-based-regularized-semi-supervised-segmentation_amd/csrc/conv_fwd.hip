// Host side of the 3x3 convolutions: which kernel serves a call (conv3x3_fwd_impl) and the forward / data-gradient entry points.
// No kernels here (conv.h has the file map).
#include "conv.h"

using namespace miseg;

extern "C" int64_t miseg_conv3x3_stats_parts(int dt, int64_t Cin, int64_t N, int64_t H, int64_t W) {
    MISEG_F16_DISPATCH_ON(dt, miseg_conv3x3_stats_parts, MISEG_BF16, Cin, N, H, W);
    if (conv_streams(dt, Cin, N, H, W)) return stream_blocks(N, H, W);
    const TiledShape t = tiled_shape(dt, H, W, 0, false);      // (the tile depends on neither Cout nor pool)
    return N * cdiv(H, t.th) * cdiv(W, t.tw);
}

// Rows of the statistics matrix miseg_conv3x3_fwd writes for this layer (what bn_finalize must be told): one per block of the kernel
// that serves the shape -- the persistent tiled kernel has far fewer blocks than tiles.
extern "C" int64_t miseg_conv3x3_fwd_parts(int dt, int64_t Cin, int64_t N, int64_t H, int64_t W, int64_t Cout) {
    MISEG_F16_DISPATCH_ON(dt, miseg_conv3x3_fwd_parts, MISEG_BF16, Cin, N, H, W, Cout);
    const int64_t ntiles = miseg_conv3x3_stats_parts(dt, Cin, N, H, W);
    if (conv_streams(dt, Cin, N, H, W) || dt != MISEG_BF16 || !tiled_persistent()) return ntiles;
    const TiledShape t = tiled_shape(dt, H, W, Cout, false);                            // (statistics: never a pooled output)
    if (t.th != 8) return ntiles;                                                        // (launch_tiled: the persistent form serves 8-row tiles)
    return pt_grid((int)ntiles, (int)cdiv(Cout, t.cot), t.th).blocks;
}

static int conv3x3_fwd_impl(void* stream, int dt, const void* in0, int64_t C0, int ups0, const void* in1, int64_t C1, int ups1,
                            int64_t N, int64_t H, int64_t W, const void* packed_w, int64_t Cout, void* out, float* stats, BnFinish fin,
                            bool pool_out = false, BnLoad bl = BnLoad{nullptr, nullptr}, BnRed br = BnRed{nullptr, nullptr, nullptr}) {
    MISEG_REQUIRE(in0 && packed_w && out, "conv3x3_fwd: null pointer");
    MISEG_REQUIRE(N > 0 && H > 0 && W > 0 && Cout > 0 && C0 > 0 && C1 >= 0, "conv3x3_fwd: bad shape");
    MISEG_REQUIRE(C1 == 0 || in1, "conv3x3_fwd: second source missing");
    MISEG_REQUIRE((ups0 == 0 || ups0 == 1) && (ups1 == 0 || ups1 == 1), "conv3x3_fwd: ups must be 0/1");
    MISEG_REQUIRE((!ups0 || (H % 2 == 0 && W % 2 == 0)) && (!ups1 || (H % 2 == 0 && W % 2 == 0)), "conv3x3_fwd: upsampled size must be even");
    const int vec = dt == MISEG_BF16 ? 8 : 4;
    MISEG_REQUIRE(C0 % vec == 0 && C1 % vec == 0, "conv3x3_fwd: channel counts must be multiples of %d (use conv_small for the stem)", vec);
    ConvSrc s{in0, in1, (int)C0, (int)C1, ups0, ups1};
    hipStream_t st = as_stream(stream);
    MISEG_REQUIRE(!bl.gy || (bl.coef && C1 == 0 && ups0 == 0), "conv3x3: the BatchNorm loader reads one full-resolution source");
    MISEG_REQUIRE(!br.raw || (br.saved && br.parts && !pool_out && !stats && Cout % 4 == 0), "conv3x3: epilogue reduce needs a full-resolution "
                  "output with a multiple of 4 channels and no forward statistics");
    MISEG_REQUIRE(!pool_out || (sumpool_supported(dt, C0 + C1, N, H, W, Cout) && C1 == 0 && !stats),
                  "conv3x3_fwd_sumpool: shape not supported (ask miseg_conv3x3_fwd_sumpool_supported)");
    if (conv_streams(dt, C0 + C1, N, H, W)) {
        // wider outputs run as 32-channel slices (grid.y): a 64-channel block would need 97 KB of LDS and the whole
        // register file, i.e. one block per CU; re-reading the (narrow) input per slice is cheaper
        const int cot = Cout <= 16 ? 16 : 32;
        // one slot layout per number of 8-channel vectors of the (<= 32) input channels; a pooled output has one source (checked above)
        const int rc = launch_conv_stream(cot, (int)((C0 + C1) / 8), C1 > 0, pool_out, (unsigned)stream_blocks(N, H, W), st, s, (int)N, (int)H, (int)W,
                                          packed_w, (int)Cout, out, stats, fin, bl, br);
        if (rc != MISEG_OK) return rc;
    } else {
        const TiledShape t = tiled_shape(dt, H, W, Cout, pool_out);
        if (!t.cot) return fail(MISEG_E_INVALID, "conv3x3_fwd: bad dtype");
        const dim3 grid((unsigned)(N * cdiv(H, t.th) * cdiv(W, t.tw)), (unsigned)cdiv(Cout, t.cot));
        const int rc = launch_conv_tiled(dt, t.cot, t.tw, t.th, pool_out, grid, st, s, (int)N, (int)H, (int)W, packed_w, (int)Cout, out, stats, fin, bl, br);
        if (rc != MISEG_OK) return rc;
    }
    MISEG_LAUNCH_CHECK("conv3x3_kernel");
    return MISEG_OK;
}

extern "C" int miseg_conv3x3_fwd(void* stream, int dt, const void* in0, int64_t C0, int ups0, const void* in1, int64_t C1, int ups1,
                                 int64_t N, int64_t H, int64_t W, const void* packed_w, int64_t Cout, void* out, float* stats) {
    MISEG_TAPE(miseg_conv3x3_fwd, stream, dt, in0, C0, ups0, in1, C1, ups1, N, H, W, packed_w, Cout, out, stats);
    MISEG_F16_DISPATCH_ON(dt, miseg_conv3x3_fwd, stream, MISEG_BF16, in0, C0, ups0, in1, C1, ups1, N, H, W, packed_w, Cout, out, stats);
    return conv3x3_fwd_impl(stream, dt, in0, C0, ups0, in1, C1, ups1, N, H, W, packed_w, Cout, out, stats, BnFinish{});
}

extern "C" int64_t miseg_conv3x3_fwd_sumpool_supported(int dt, int64_t Cin, int64_t N, int64_t H, int64_t W, int64_t Cout) {
    return sumpool_supported(dt == MISEG_F16 ? MISEG_BF16 : dt, Cin, N, H, W, Cout);
}

extern "C" int miseg_conv3x3_fwd_sumpool(void* stream, int dt, const void* in, int64_t Cin, int64_t N, int64_t H, int64_t W,
                                         const void* packed_w, int64_t Cout, void* out_pooled) {
    MISEG_TAPE(miseg_conv3x3_fwd_sumpool, stream, dt, in, Cin, N, H, W, packed_w, Cout, out_pooled);
    MISEG_F16_DISPATCH_ON(dt, miseg_conv3x3_fwd_sumpool, stream, MISEG_BF16, in, Cin, N, H, W, packed_w, Cout, out_pooled);
    return conv3x3_fwd_impl(stream, dt, in, Cin, 0, nullptr, 0, 0, N, H, W, packed_w, Cout, out_pooled, nullptr, BnFinish{}, true);
}

extern "C" int64_t miseg_conv3x3_fwd_sumpool_acc_supported(int dt, int64_t Cin, int64_t N, int64_t H, int64_t W) {
    return conv_streams(dt == MISEG_F16 ? MISEG_BF16 : dt, Cin, N, H, W) && H % 2 == 0 && W % 2 == 0;
}

extern "C" int miseg_conv3x3_fwd_sumpool_acc(void* stream, int dt, const void* in, int64_t Cin, int64_t N, int64_t H, int64_t W,
                                             const void* packed_w, int64_t Cout, void* inout_pooled) {
    MISEG_TAPE(miseg_conv3x3_fwd_sumpool_acc, stream, dt, in, Cin, N, H, W, packed_w, Cout, inout_pooled);
    MISEG_F16_DISPATCH_ON(dt, miseg_conv3x3_fwd_sumpool_acc, stream, MISEG_BF16, in, Cin, N, H, W, packed_w, Cout, inout_pooled);
    MISEG_REQUIRE(miseg_conv3x3_fwd_sumpool_acc_supported(dt, Cin, N, H, W), "conv3x3_fwd_sumpool_acc: streaming shapes only");
    BnFinish opt{};
    opt.accumulate_out = 1;
    return conv3x3_fwd_impl(stream, dt, in, Cin, 0, nullptr, 0, 0, N, H, W, packed_w, Cout, inout_pooled, nullptr, opt, true);
}

// ---- data gradient of a convolution over the channel concat of two full-resolution sources: ONE launch, two destinations
extern "C" int miseg_conv3x3_dgrad_dual(void* stream, int dt, const void* graw, int64_t K, int64_t N, int64_t H, int64_t W, const void* packed_w,
                                        int64_t C0, void* out0, int64_t C1, void* out1) {
    MISEG_TAPE(miseg_conv3x3_dgrad_dual, stream, dt, graw, K, N, H, W, packed_w, C0, out0, C1, out1);
    MISEG_F16_DISPATCH_ON(dt, miseg_conv3x3_dgrad_dual, stream, MISEG_BF16, graw, K, N, H, W, packed_w, C0, out0, C1, out1);
    MISEG_REQUIRE(out0 && out1 && C0 > 0 && C1 > 0 && C0 % 16 == 0 && C1 % 4 == 0, "conv3x3_dgrad_dual: the first source must have a multiple of "
                  "16 channels, the second a multiple of 4");
    BnFinish opt{};
    opt.out1 = out1;
    opt.split = (int)C0;
    return conv3x3_fwd_impl(stream, dt, graw, K, 0, nullptr, 0, 0, N, H, W, packed_w, C0 + C1, out0, nullptr, opt);
}

// ---- data gradient with the BatchNorm backward folded in (unet_ops._ConvBNReLU.backward)
static bool dgrad_bn_stream_ok(int dt, int64_t K, int64_t N, int64_t H, int64_t W) {
    return !conv_streams(dt, K, N, H, W) || K == 16 || K == 32;
}
extern "C" int64_t miseg_conv3x3_dgrad_bn_supported(int dt, int64_t K, int64_t N, int64_t H, int64_t W, int64_t Cs, int pool_out) {
    if (dt == MISEG_F16) dt = MISEG_BF16;
    const int vec = dt == MISEG_BF16 ? 8 : 4;
    if (K % vec || !dgrad_bn_stream_ok(dt, K, N, H, W)) return 0;
    return pool_out ? sumpool_supported(dt, K, N, H, W, Cs) : 1;
}
extern "C" int64_t miseg_conv3x3_dgrad_red_parts(int dt, int64_t K, int64_t N, int64_t H, int64_t W, int64_t Cs) {
    if (dt == MISEG_F16) dt = MISEG_BF16;
    if (Cs % 4 || !dgrad_bn_stream_ok(dt, K, N, H, W)) return 0;
    return miseg_conv3x3_stats_parts(dt, K, N, H, W);
}
extern "C" int miseg_conv3x3_dgrad_bn(void* stream, int dt, const void* raw_or_graw, const void* gy, const float* bwd_coef, int64_t K,
                                      int64_t N, int64_t H, int64_t W, const void* packed_w, int64_t Cs, void* out, int pool_out,
                                      const void* red_raw, const float* red_saved, float* red_parts) {
    MISEG_TAPE(miseg_conv3x3_dgrad_bn, stream, dt, raw_or_graw, gy, bwd_coef, K, N, H, W, packed_w, Cs, out, pool_out, red_raw, red_saved, red_parts);
    MISEG_F16_DISPATCH_ON(dt, miseg_conv3x3_dgrad_bn, stream, MISEG_BF16, raw_or_graw, gy, bwd_coef, K, N, H, W, packed_w, Cs, out, pool_out, red_raw,
                          red_saved, red_parts);
    MISEG_REQUIRE(!gy || bwd_coef, "conv3x3_dgrad_bn: coefficients missing");
    MISEG_REQUIRE(!red_raw || (!pool_out && red_saved && red_parts && miseg_conv3x3_dgrad_red_parts(dt, K, N, H, W, Cs) > 0),
                  "conv3x3_dgrad_bn: epilogue reduce not available for this call (ask miseg_conv3x3_dgrad_red_parts)");
    MISEG_REQUIRE(!gy || miseg_conv3x3_dgrad_bn_supported(dt, K, N, H, W, Cs, pool_out), "conv3x3_dgrad_bn: shape not supported (ask _supported)");
    return conv3x3_fwd_impl(stream, dt, raw_or_graw, K, 0, nullptr, 0, 0, N, H, W, packed_w, Cs, out, nullptr, BnFinish{}, pool_out != 0,
                            BnLoad{gy, bwd_coef}, BnRed{red_raw, red_saved, red_parts});
}

extern "C" int64_t miseg_conv3x3_fwd_acc_supported(int dt, int64_t Cin, int64_t N, int64_t H, int64_t W, int64_t Cout) {
    return Cout <= 256 && miseg_conv3x3_fwd_parts(dt, Cin, N, H, W, Cout) <= kBnAccMaxBlocks;       // the fixed point's no-wrap bound
}

// miseg_conv3x3_fwd with the BatchNorm statistics added into acc[2 Cout + 1] (fixed point, common.h bn_acc_add) instead of written as one row
// per block: no finalize launch -- miseg_bn_relu_fwd_acc reads the two totals of a channel itself
extern "C" int miseg_conv3x3_fwd_acc(void* stream, int dt, const void* in0, int64_t C0, int ups0, const void* in1, int64_t C1, int ups1,
                                     int64_t N, int64_t H, int64_t W, const void* packed_w, int64_t Cout, void* out, void* acc) {
    MISEG_TAPE(miseg_conv3x3_fwd_acc, stream, dt, in0, C0, ups0, in1, C1, ups1, N, H, W, packed_w, Cout, out, acc);
    MISEG_F16_DISPATCH_ON(dt, miseg_conv3x3_fwd_acc, stream, MISEG_BF16, in0, C0, ups0, in1, C1, ups1, N, H, W, packed_w, Cout, out, acc);
    MISEG_REQUIRE(acc && ((uintptr_t)acc & 7) == 0, "conv3x3_fwd_acc: the accumulator must be an 8-byte aligned [2 Cout + 1] array");
    MISEG_REQUIRE(miseg_conv3x3_fwd_acc_supported(dt, C0 + C1, N, H, W, Cout), "conv3x3_fwd_acc: shape not supported (ask miseg_conv3x3_fwd_acc_supported)");
    BnFinish fin{};
    fin.acc = static_cast<unsigned long long*>(acc);
    return conv3x3_fwd_impl(stream, dt, in0, C0, ups0, in1, C1, ups1, N, H, W, packed_w, Cout, out, reinterpret_cast<float*>(acc), fin);
}

extern "C" int64_t miseg_conv3x3_bn_fwd_fusable(int dt, int64_t Cin, int64_t N, int64_t H, int64_t W, int64_t Cout) {
    const int64_t parts = miseg_conv3x3_stats_parts(dt == MISEG_F16 ? MISEG_BF16 : dt, Cin, N, H, W);
    return Cout % 4 == 0 && Cout <= 256 && parts * 2 * Cout <= kFinishFloats;
}

extern "C" int miseg_conv3x3_bn_fwd(void* stream, int dt, const void* in0, int64_t C0, int ups0, const void* in1, int64_t C1, int ups1,
                                    int64_t N, int64_t H, int64_t W, const void* packed_w, int64_t Cout, void* out, float* stats,
                                    const float* gamma, const float* beta, float eps, float momentum, float* rmean, float* rvar,
                                    int64_t* nbt, float* saved, int32_t* sync_counter) {
    MISEG_TAPE(miseg_conv3x3_bn_fwd, stream, dt, in0, C0, ups0, in1, C1, ups1, N, H, W, packed_w, Cout, out, stats, gamma, beta, eps, momentum, rmean, rvar, nbt, saved, sync_counter);
    MISEG_F16_DISPATCH_ON(dt, miseg_conv3x3_bn_fwd, stream, MISEG_BF16, in0, C0, ups0, in1, C1, ups1, N, H, W, packed_w, Cout, out, stats, gamma, beta,
                          eps, momentum, rmean, rvar, nbt, saved, sync_counter);
    MISEG_REQUIRE(stats && gamma && beta && saved && sync_counter, "conv3x3_bn_fwd: null pointer");
    MISEG_REQUIRE(miseg_conv3x3_bn_fwd_fusable(dt, C0 + C1, N, H, W, Cout), "conv3x3_bn_fwd: shape not fusable (ask miseg_conv3x3_bn_fwd_fusable)");
    BnFinish fin{reinterpret_cast<unsigned int*>(sync_counter), gamma, beta, rmean, rvar, (long long*)nbt, saved, (float)(N * H * W), eps, momentum};
    return conv3x3_fwd_impl(stream, dt, in0, C0, ups0, in1, C1, ups1, N, H, W, packed_w, Cout, out, stats, fin);
}
