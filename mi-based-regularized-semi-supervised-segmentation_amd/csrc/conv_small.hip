// The small kernels around the 3x3 convolutions: weight packing, the 1x1 logits head, the stem (conv.h has the file map).
#include "conv.h"

namespace miseg {

// OIHW fp32 -> packed [tap][n][k] of T.  kind 0 (forward): n = o, k = i, tap = ky*3+kx.
// kind 1 (dgrad): n = i - ci_begin (ci_count of them), k = o, tap mirrored (2-ky, 2-kx).
template <typename T>
__global__ void pack_w_kernel(const float* __restrict__ w, int Cout, int Cin, int kind, int ci_begin, int ci_count, T* __restrict__ pk) {
    // kind >> 8 = input channels the SOURCE tensor really has (0: Cin): the stem's [Cout, 1, 3, 3] weight packed as Cin = one channel
    // vector, the extra channels zero (forward layout only) -- the host no longer pads the weight with torch ops every step
    const int csrc = (kind >> 8) ? (kind >> 8) : Cin;
    kind &= 0xff;
    const int Nn = kind ? ci_count : Cout, Kk = kind ? Cout : Cin;
    const int total = 9 * Nn * Kk;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
        const int k = e % Kk, nn = (e / Kk) % Nn, tap = e / (Kk * Nn);
        const int ky = tap / 3, kx = tap % 3;
        float v;
        if (!kind) v = k < csrc ? w[(((size_t)nn * csrc + k) * 3 + ky) * 3 + kx] : 0.f;
        else v = w[(((size_t)k * Cin + ci_begin + nn) * 3 + (2 - ky)) * 3 + (2 - kx)];
        pk[e] = from_f32<T>(v);
    }
}

// All conv weights of a step in one launch: job j packs like pack_w_kernel; blocks [first_block[j], first_block[j+1]) belong to it.
struct PackJob {            // mirrors miseg_pack_job (include/miseg_hip.h)
    const float* w;
    void* packed;
    int32_t Cout, Cin, kind, ci_begin, ci_count, first_block;
};
template <typename T>
__global__ __launch_bounds__(256) void pack_w_multi_kernel(const PackJob* __restrict__ jobs, int njobs) {
    int lo = 0, hi = njobs - 1;                       // last job whose first_block <= blockIdx.x
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[mid].first_block <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    PackJob jb = jobs[lo];
    const int csrc = (jb.kind >> 8) ? (jb.kind >> 8) : jb.Cin;      // see pack_w_kernel
    jb.kind &= 0xff;
    const int Nn = jb.kind ? jb.ci_count : jb.Cout, Kk = jb.kind ? jb.Cout : jb.Cin, total = 9 * Nn * Kk;
    const int e = ((int)blockIdx.x - jb.first_block) * 256 + threadIdx.x;
    if (e >= total) return;
    const int k = e % Kk, nn = (e / Kk) % Nn, tap = e / (Kk * Nn), ky = tap / 3, kx = tap % 3;
    const float v = !jb.kind ? (k < csrc ? jb.w[(((size_t)nn * csrc + k) * 3 + ky) * 3 + kx] : 0.f)
                             : jb.w[(((size_t)k * jb.Cin + jb.ci_begin + nn) * 3 + (2 - ky)) * 3 + (2 - kx)];
    reinterpret_cast<T*>(jb.packed)[e] = from_f32<T>(v);
}

// ------------------------------------------------------------------------------------------ 1x1 logits head
template <typename T, int CI, int CO>
__global__ __launch_bounds__(256) void conv1x1_fwd_kernel(const T* __restrict__ in, int64_t npix, const float* __restrict__ w,
                                                          const float* __restrict__ bias, float* __restrict__ out) {
    // the pixel's CI channels arrive as 16-byte vectors and (CO == 4) the logits leave as one float4: per-element 2-byte loads
    // and 4-byte stores ran this 150 MB stream at 0.9 TB/s
    float wr[CO * CI], br[CO];
#pragma unroll
    for (int e = 0; e < CO * CI; ++e) wr[e] = w[e];
#pragma unroll
    for (int o = 0; o < CO; ++o) br[o] = bias[o];
    for (int64_t i = blockIdx.x * 256LL + threadIdx.x; i < npix; i += (int64_t)gridDim.x * 256) {
        constexpr int NV = CI * (int)sizeof(T) / 16;
        static_assert(CI * sizeof(T) % 16 == 0, "conv1x1_fwd: the channel vector must be a multiple of 16 bytes");
        uint4 vin[NV];
#pragma unroll
        for (int v = 0; v < NV; ++v) vin[v] = reinterpret_cast<const uint4*>(in + i * CI)[v];
        const T* fe = reinterpret_cast<const T*>(vin);
        float f[CI], a[CO];
#pragma unroll
        for (int c = 0; c < CI; ++c) f[c] = to_f32(fe[c]);
#pragma unroll
        for (int o = 0; o < CO; ++o) {
            a[o] = br[o];
#pragma unroll
            for (int c = 0; c < CI; ++c) a[o] += wr[o * CI + c] * f[c];
        }
        if (CO == 4) *reinterpret_cast<float4*>(out + i * 4) = make_float4(a[0], a[1 % CO], a[2 % CO], a[3 % CO]);
        else {
#pragma unroll
            for (int o = 0; o < CO; ++o) out[i * CO + o] = a[o];
        }
    }
}

template <typename T, int CI, int CO>
__global__ __launch_bounds__(256) void conv1x1_bwd_kernel(const T* __restrict__ in, const float* __restrict__ gout, int64_t npix,
                                                          const float* __restrict__ w, T* __restrict__ gin, float* __restrict__ partials) {
    __shared__ float red[4][CO * CI + CO];
    float gwacc[CO * CI], gbacc[CO];
#pragma unroll
    for (int e = 0; e < CO * CI; ++e) gwacc[e] = 0.f;
#pragma unroll
    for (int o = 0; o < CO; ++o) gbacc[o] = 0.f;
    for (int64_t i = blockIdx.x * 256LL + threadIdx.x; i < npix; i += (int64_t)gridDim.x * 256) {
        // the pixel's CI channels travel as 16-byte vectors both ways (2-byte scalar stores were the bottleneck)
        constexpr int NV = CI * (int)sizeof(T) / 16;
        static_assert(CI * sizeof(T) % 16 == 0, "conv1x1_bwd: the channel vector must be a multiple of 16 bytes");
        uint4 vin[NV];
#pragma unroll
        for (int v = 0; v < NV; ++v) vin[v] = reinterpret_cast<const uint4*>(in + i * CI)[v];
        const T* fe = reinterpret_cast<const T*>(vin);
        float f[CI], g[CO];
#pragma unroll
        for (int c = 0; c < CI; ++c) f[c] = to_f32(fe[c]);
        if (CO == 4) {
            const float4 g4 = *reinterpret_cast<const float4*>(gout + i * 4);
            g[0] = g4.x; g[1 % CO] = g4.y; g[2 % CO] = g4.z; g[3 % CO] = g4.w;
        } else {
#pragma unroll
            for (int o = 0; o < CO; ++o) g[o] = gout[i * CO + o];
        }
#pragma unroll
        for (int o = 0; o < CO; ++o) gbacc[o] += g[o];
        uint4 vout[NV];
        T* oe = reinterpret_cast<T*>(vout);
#pragma unroll
        for (int c = 0; c < CI; ++c) {
            float a = 0.f;
#pragma unroll
            for (int o = 0; o < CO; ++o) { a += w[o * CI + c] * g[o]; gwacc[o * CI + c] += g[o] * f[c]; }
            oe[c] = from_f32<T>(a);
        }
        if (gin) {
#pragma unroll
            for (int v = 0; v < NV; ++v) reinterpret_cast<uint4*>(gin + i * CI)[v] = vout[v];
        }
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int e = 0; e < CO * CI; ++e) {
        float v = wave_sum(gwacc[e]);
        if (lane == 0) red[wv][e] = v;
    }
#pragma unroll
    for (int o = 0; o < CO; ++o) {
        float v = wave_sum(gbacc[o]);
        if (lane == 0) red[wv][CO * CI + o] = v;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < CO * CI + CO; e += 256)
        partials[(size_t)blockIdx.x * (CO * CI + CO) + e] = red[0][e] + red[1][e] + red[2][e] + red[3][e];
}

__global__ __launch_bounds__(256) void sum_parts2_kernel(const float* __restrict__ partials, int nparts, int len, int n0, float* __restrict__ d0,
                                                         float* __restrict__ d1) {
    reduce_partials_block(partials, nparts, (size_t)len, len, Split2Out{d0, n0, d1}, [](int e) { return (size_t)e; });
}

// ---- The stem (one image channel in) without matrix cores (MISEG_STEM_KERNELS=0: the MFMA path).
// `conv3x3_stream_kernel` treats the padded channel vector as 8 (of 32) input channels: 31 of 32 multiplies are by zero, the launch takes
// 50 us at 256 x 256 for a 100 MB store, and the padded operand has to be written first (15 us); its weight gradient (59 + 10 us) is the
// LAST kernel of the backward pass, alone on the GPU, i.e. all of it is step tail.  These kernels read the fp32 image itself and take
// 50 / 52 + 7 us (rows through a prefetched LDS ring; staging three rows per output row without prefetch: 56 / 57; nine direct loads per
// thread: 122 / 140; on the padded operand, 16-byte stride: 148 / 156).
// A thread owns one pixel and four output channels: nine bf16 x bf16 products per output (exact in fp32, accumulated by FMA in tap order), 8-byte stores that
// are contiguous across the lanes of a pixel; statistics from the fp32 accumulators as everywhere.  x: [N][H][W][CP] (channel 0 is the
// image), w: the fp32 master [Cout][Cw][3][3] (Cw >= 1: only input channel 0 is read), rounded to the storage type as the packed
// weights of the MFMA path are.
// The input rows of a block's run of output rows, as a ring of four LDS rows (+ one row of zeros): an output row reads rows r - 1, r,
// r + 1; row r + 2 is committed from registers behind its compute and row r + 3 is already in flight (one barrier per row, the
// global round trip behind a whole row's arithmetic).  Rows of the neighbouring image / outside the image read the zero row.
template <typename T, typename TX, int NPRE>
struct StemRing {
    unsigned short* buf;      // [5][RB]: slots 0..3 the ring, slot 4 zeros
    const TX* x;
    int RB, W, CP, rows;
    unsigned short pre[NPRE];
    __device__ __forceinline__ void fetch(int rin) {
#pragma unroll
        for (int k = 0; k < NPRE; ++k) {
            const int c = (int)threadIdx.x + 256 * k - 1;
            T v = from_f32<T>(0.f);
            if ((unsigned)rin < (unsigned)rows && (unsigned)c < (unsigned)W) v = from_f32<T>(to_f32(x[((size_t)rin * W + c) * CP]));    // an fp32 image is rounded here
            pre[k] = *reinterpret_cast<const unsigned short*>(&v);
        }
    }
    __device__ __forceinline__ void commit(int rin) {
        unsigned short* d = buf + ((rin + 1) & 3) * RB;
#pragma unroll
        for (int k = 0; k < NPRE; ++k) {
            const int i = (int)threadIdx.x + 256 * k;
            if (i < RB) d[i] = pre[k];
        }
    }
    __device__ __forceinline__ const unsigned short* row(int rin, bool inside) const { return inside ? buf + ((rin + 1) & 3) * RB : buf + 4 * RB; }
    // rows r0 - 1, r0, r0 + 1 staged, r0 + 2 in flight
    __device__ __forceinline__ void start(int r0) {
        for (int i = threadIdx.x; i < RB; i += 256) buf[4 * RB + i] = 0;
        for (int d = -1; d <= 1; ++d) { fetch(r0 + d); commit(r0 + d); }
        fetch(r0 + 2);
        __syncthreads();
    }
    // after the compute of row r: row r + 2 becomes readable, row r + 3 takes off
    __device__ __forceinline__ void advance(int r) {
        commit(r + 2);
        fetch(r + 3);
        __syncthreads();
    }
};
constexpr int kStemPre = 4;       // W + 2 <= 1024

template <typename T, typename TX>
__global__ __launch_bounds__(256) void stem_conv_fwd_kernel(const TX* __restrict__ x, int CP, int N, int H, int W, const float* __restrict__ w, int Cw,
                                                            int Cout, T* __restrict__ out, unsigned long long* __restrict__ acc) {
    const int G = Cout / 4, g = threadIdx.x % G, ppb = 256 / G;
    float wr[9][4];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int r = 0; r < 4; ++r) wr[tap][r] = to_f32(from_f32<T>(w[((size_t)(g * 4 + r) * Cw) * 9 + tap]));
    float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
    // a block walks a contiguous run of image rows (row = n * H + h: block-uniform, so is h), its threads the row's pixels
    extern __shared__ unsigned short stem_rows[];        // [5][W + 2]
    const int rows = N * H, c0 = threadIdx.x / G, per = (rows + (int)gridDim.x - 1) / (int)gridDim.x;
    const int r_begin = blockIdx.x * per, r_end = min(rows, r_begin + per);
    StemRing<T, TX, kStemPre> ring{stem_rows, x, W + 2, W, CP, rows, {}};
    if (r_begin < r_end) ring.start(r_begin);
    for (int row = r_begin; row < r_end; ++row) {
      const int h = row % H;
      const unsigned short* rp[3] = {ring.row(row - 1, h > 0), ring.row(row, true), ring.row(row + 1, h < H - 1)};
      for (int wq = c0; wq < W; wq += ppb) {
        const size_t p = (size_t)row * W + wq;
        float a[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const float v = bf16_bits_to_f32(rp[tap / 3][wq + tap % 3]);
#pragma unroll
            for (int r = 0; r < 4; ++r) a[r] = fmaf(v, wr[tap][r], a[r]);
        }
        T o4[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) { o4[r] = from_f32<T>(a[r]); s1[r] += a[r]; s2[r] += a[r] * a[r]; }
        *reinterpret_cast<uint2*>(out + p * Cout + g * 4) = *reinterpret_cast<const uint2*>(o4);
      }
      ring.advance(row);
    }
    if (acc) {       // block sums per channel (fixed order), then the fixed-point accumulator (common.h bn_acc_add)
        __shared__ float sred[256][8];
#pragma unroll
        for (int r = 0; r < 4; ++r) { sred[threadIdx.x][r] = s1[r]; sred[threadIdx.x][4 + r] = s2[r]; }
        __syncthreads();
        if ((int)threadIdx.x < 2 * Cout) {
            const int which = threadIdx.x / Cout, c = threadIdx.x % Cout, gg = c / 4, r = c % 4;
            float t = 0.f;
            for (int m = 0; m < ppb; ++m) t += sred[m * G + gg][which * 4 + r];
            bn_acc_add(acc + which * Cout + c, acc + 2 * Cout, t);
        }
    }
}

// gw[co][tap] = sum_px graw[px][co] * x[px + tap]: the same thread map and row ring, 36 accumulators per thread over the block's pixels,
// one partial vector [Cout * 9] per block (summed by stem_wgrad_sum_kernel in fixed order: deterministic)
template <typename T, typename TX>
__global__ __launch_bounds__(256) void stem_wgrad_kernel(const TX* __restrict__ x, int CP, int N, int H, int W, const T* __restrict__ graw, int Cout,
                                                         float* __restrict__ partials) {
    const int G = Cout / 4, g = threadIdx.x % G, ppb = 256 / G;
    float a[9][4];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int r = 0; r < 4; ++r) a[tap][r] = 0.f;
    extern __shared__ float swr[];      // [256][37]: the threads' 36 sums (odd stride: conflict-free column reads); behind it the row ring
    const int rows = N * H, c0 = threadIdx.x / G, per = (rows + (int)gridDim.x - 1) / (int)gridDim.x;
    const int r_begin = blockIdx.x * per, r_end = min(rows, r_begin + per);
    StemRing<T, TX, kStemPre> ring{reinterpret_cast<unsigned short*>(swr + 256 * 37), x, W + 2, W, CP, rows, {}};
    if (r_begin < r_end) ring.start(r_begin);
    for (int row = r_begin; row < r_end; ++row) {
      const int h = row % H;
      const unsigned short* rp[3] = {ring.row(row - 1, h > 0), ring.row(row, true), ring.row(row + 1, h < H - 1)};
      for (int wq = c0; wq < W; wq += ppb) {
        const size_t p = (size_t)row * W + wq;
        const uint2 gq = *reinterpret_cast<const uint2*>(graw + p * Cout + g * 4);
        T g4[4];
        *reinterpret_cast<uint2*>(g4) = gq;
        const float gv[4] = {to_f32(g4[0]), to_f32(g4[1]), to_f32(g4[2]), to_f32(g4[3])};
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const float v = bf16_bits_to_f32(rp[tap / 3][wq + tap % 3]);
#pragma unroll
            for (int r = 0; r < 4; ++r) a[tap][r] = fmaf(gv[r], v, a[tap][r]);
        }
      }
      ring.advance(row);
    }
    __syncthreads();
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int r = 0; r < 4; ++r) swr[threadIdx.x * 37 + tap * 4 + r] = a[tap][r];
    __syncthreads();
    for (int o = threadIdx.x; o < Cout * 9; o += 256) {
        const int co = o / 9, tap = o % 9, gg = co / 4, r = co % 4;
        float t = 0.f;
        for (int m = 0; m < ppb; ++m) t += swr[(m * G + gg) * 37 + tap * 4 + r];
        partials[(size_t)blockIdx.x * Cout * 9 + o] = t;
    }
}
__global__ __launch_bounds__(256) void stem_wgrad_sum_kernel(const float* __restrict__ partials, int nparts, int len, float* __restrict__ gw) {
    reduce_partials_block(partials, nparts, (size_t)len, len, gw, [](int e) { return (size_t)e; });
}
// ---- the stem's data gradient: gimage[n,y,x] = sum_k sum_{dy,dx} graw[n, y+1-dy, x+1-dx, k] * w[k,0,dy,dx] (fp32 [N][1][H][W]).
// The same walk as the two kernels above -- a block owns a run of image rows (row = n * H + h), a thread the pixel columns
// threadIdx.x + 256 k -- turned around: for every INPUT row r of graw (the run and one row either side) a thread reads its pixel's Cout
// values once, in 16-byte vectors, and forms the nine tap sums T[dy][dx] = sum_k graw[r, x, k] * w[k, dy, dx] (weights rounded to the
// storage type beforehand, read through uniform loads); the sums cross the lanes through LDS (R[dy][x] = sum_dx T[dy][dx][x + 1 - dx],
// a zero column either side), and row r's R[dy] is added to output row r - 1 + dy where that row belongs to the same image.  Three
// running rows of accumulators per column; output row r - 1 is complete, and stored, once input row r has been added.  Sums in a fixed
// order: k ascending inside a tap, dx ascending, then dy = 2, 1, 0.
template <typename T>
__global__ void stem_dgrad_round_w_kernel(const float* __restrict__ w, int n, float* __restrict__ wr) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) wr[i] = to_f32(from_f32<T>(w[i]));
}

template <typename T>
__global__ __launch_bounds__(256) void stem_dgrad_kernel(const T* __restrict__ graw, int N, int H, int W, int Cout, const float* __restrict__ wr,
                                                         float* __restrict__ gimage) {
    constexpr int V = VT<T>::V;
    typedef typename VT<T>::Raw Raw;
    extern __shared__ float stem_taps[];                 // [9][W + 2]: column x lives at x + 1, columns 0 and W + 1 stay zero
    const int RB = W + 2, rows = N * H, per = (rows + (int)gridDim.x - 1) / (int)gridDim.x, CV = Cout / V;
    const int r_begin = blockIdx.x * per, r_end = min(rows, r_begin + per);
    if (r_begin >= r_end) return;
    for (int i = threadIdx.x; i < 9 * RB; i += 256) stem_taps[i] = 0.f;
    float prev[kStemPre], cur[kStemPre], next[kStemPre];     // output rows r - 1, r, r + 1 while input row r is added
#pragma unroll
    for (int k = 0; k < kStemPre; ++k) prev[k] = cur[k] = next[k] = 0.f;
    for (int r = r_begin - 1; r <= r_end; ++r) {
        const bool live = r >= 0 && r < rows;            // block-uniform
        const int h = live ? r % H : 0;
        __syncthreads();                                 // the readers of the previous row's sums (first pass: the zero fill) are done
        if (live) {
#pragma unroll
            for (int k = 0; k < kStemPre; ++k) {
                const int x = (int)threadIdx.x + 256 * k;
                if (x >= W) continue;
                float t[9];
#pragma unroll
                for (int tap = 0; tap < 9; ++tap) t[tap] = 0.f;
                const Raw* gp = reinterpret_cast<const Raw*>(graw + ((size_t)r * W + x) * Cout);
                for (int cv = 0; cv < CV; ++cv) {
                    float f[V];
                    VT<T>::unpack(gp[cv], f);
#pragma unroll
                    for (int i = 0; i < V; ++i) {
                        const float* wk = wr + (cv * V + i) * 9;
#pragma unroll
                        for (int tap = 0; tap < 9; ++tap) t[tap] = fmaf(f[i], wk[tap], t[tap]);
                    }
                }
#pragma unroll
                for (int tap = 0; tap < 9; ++tap) stem_taps[tap * RB + x + 1] = t[tap];
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kStemPre; ++k) {
            const int x = (int)threadIdx.x + 256 * k;
            if (x >= W) continue;
            if (live) {
                float R[3];
#pragma unroll
                for (int dy = 0; dy < 3; ++dy) {
                    float s = 0.f;
#pragma unroll
                    for (int dx = 0; dx < 3; ++dx) s += stem_taps[(dy * 3 + dx) * RB + (x + 1 - dx) + 1];
                    R[dy] = s;
                }
                if (h >= 1) prev[k] += R[0];             // output row r - 1 reads this row with dy = 0 (same image only)
                cur[k] += R[1];
                if (h <= H - 2) next[k] += R[2];         // output row r + 1 reads it with dy = 2
            }
            if (r - 1 >= r_begin && r - 1 < r_end) gimage[(size_t)(r - 1) * W + x] = prev[k];
            prev[k] = cur[k]; cur[k] = next[k]; next[k] = 0.f;
        }
    }
}

constexpr int kStemBlocksMax = 4096;
static const int kStemBlocks = [] { const char* e = getenv("MISEG_STEM_BLOCKS"); return e ? std::min(kStemBlocksMax, std::max(1, atoi(e))) : 1024; }();      // (ws sized for kStemBlocksMax)

}  // namespace miseg

using namespace miseg;

extern "C" int miseg_pack_conv3x3_weights(void* stream, int dt, const float* w, int64_t Cout, int64_t Cin, int kind, int64_t ci_begin,
                                          int64_t ci_count, void* packed) {
    MISEG_TAPE(miseg_pack_conv3x3_weights, stream, dt, w, Cout, Cin, kind, ci_begin, ci_count, packed);
    MISEG_F16_DISPATCH_ON(dt, miseg_pack_conv3x3_weights, stream, MISEG_BF16, w, Cout, Cin, kind, ci_begin, ci_count, packed);
    MISEG_REQUIRE(w && packed && Cout > 0 && Cin > 0, "pack_conv3x3_weights: bad args");
    MISEG_REQUIRE(kind >= 0 && (kind & 0xff) <= 1 && (kind >> 8) <= Cin && (!(kind >> 8) || !(kind & 0xff)), "pack_conv3x3_weights: bad kind");
    if (!(kind & 0xff)) { ci_begin = 0; ci_count = Cin; }
    MISEG_REQUIRE(ci_begin >= 0 && ci_count > 0 && ci_begin + ci_count <= Cin, "pack_conv3x3_weights: bad channel slice");
    const int total = (int)(9 * ((kind & 0xff) ? ci_count * Cout : Cout * Cin));
    const int nb = std::min((total + 255) / 256, 1024);
    MISEG_WITH_STORAGE_TYPE(dt, "pack_conv3x3_weights",
        hipLaunchKernelGGL(pack_w_kernel<TT>, dim3(nb), dim3(256), 0, as_stream(stream), w, (int)Cout, (int)Cin, kind, (int)ci_begin, (int)ci_count, (TT*)packed));
    MISEG_LAUNCH_CHECK("pack_w_kernel");
    return MISEG_OK;
}

extern "C" int miseg_pack_conv3x3_weights_multi(void* stream, int dt, const void* jobs_dev, int64_t njobs, int64_t total_blocks) {
    MISEG_TAPE(miseg_pack_conv3x3_weights_multi, stream, dt, jobs_dev, njobs, total_blocks);
    MISEG_F16_DISPATCH_ON(dt, miseg_pack_conv3x3_weights_multi, stream, MISEG_BF16, jobs_dev, njobs, total_blocks);
    MISEG_REQUIRE(jobs_dev && njobs > 0 && total_blocks > 0, "pack_conv3x3_weights_multi: bad args");
    static_assert(sizeof(PackJob) == 40, "PackJob layout must match miseg_pack_job");
    MISEG_WITH_STORAGE_TYPE(dt, "pack_conv3x3_weights_multi",
        hipLaunchKernelGGL(pack_w_multi_kernel<TT>, dim3((unsigned)total_blocks), dim3(256), 0, as_stream(stream), (const PackJob*)jobs_dev, (int)njobs));
    MISEG_LAUNCH_CHECK("pack_w_multi_kernel");
    return MISEG_OK;
}

// ---- the stem without matrix cores (one real input channel; see stem_conv_fwd_kernel)
extern "C" int64_t miseg_conv3x3_stem_supported(int dt, int64_t Cin_weight, int64_t CP, int64_t Cout) {
    return (dt == MISEG_BF16 || dt == MISEG_F16) && Cin_weight == 1 && CP >= 1 && Cout >= 4 && Cout <= 64 && Cout % 4 == 0 && 256 % (Cout / 4) == 0;     // (W <= 4096: LDS rows, checked per call)
}

extern "C" int miseg_conv3x3_stem_fwd(void* stream, int dt, const void* x, int x_f32, int64_t CP, int64_t N, int64_t H, int64_t W, const float* w,
                                      int64_t Cin_weight, int64_t Cout, void* out, void* acc_or_null) {
    MISEG_TAPE(miseg_conv3x3_stem_fwd, stream, dt, x, x_f32, CP, N, H, W, w, Cin_weight, Cout, out, acc_or_null);
    MISEG_F16_DISPATCH_ON(dt, miseg_conv3x3_stem_fwd, stream, MISEG_BF16, x, x_f32, CP, N, H, W, w, Cin_weight, Cout, out, acc_or_null);
    MISEG_REQUIRE(x && w && out && N > 0 && H > 0 && W > 0, "conv3x3_stem_fwd: bad args");
    MISEG_REQUIRE(miseg_conv3x3_stem_supported(dt, Cin_weight, CP, Cout), "conv3x3_stem_fwd: 16-bit storage, one weight input channel, Cout in {4, 8, 16, 32, 64}");
    MISEG_REQUIRE(!acc_or_null || ((uintptr_t)acc_or_null & 7) == 0, "conv3x3_stem_fwd: the accumulator must be 8-byte aligned");
    MISEG_REQUIRE(W + 2 <= 256 * kStemPre, "conv3x3_stem_fwd: rows of at most %d pixels", 256 * kStemPre - 2);
    const unsigned nb = (unsigned)std::min<int64_t>(N * H, (int64_t)kStemBlocks);
    if (x_f32)
        hipLaunchKernelGGL((stem_conv_fwd_kernel<bf16, float>), dim3(nb), dim3(256), (size_t)5 * (W + 2) * 2, as_stream(stream), (const float*)x, (int)CP, (int)N, (int)H, (int)W, w,
                           (int)Cin_weight, (int)Cout, (bf16*)out, static_cast<unsigned long long*>(acc_or_null));
    else
        hipLaunchKernelGGL((stem_conv_fwd_kernel<bf16, bf16>), dim3(nb), dim3(256), (size_t)5 * (W + 2) * 2, as_stream(stream), (const bf16*)x, (int)CP, (int)N, (int)H, (int)W, w,
                           (int)Cin_weight, (int)Cout, (bf16*)out, static_cast<unsigned long long*>(acc_or_null));
    MISEG_LAUNCH_CHECK("stem_conv_fwd_kernel");
    return MISEG_OK;
}

extern "C" int64_t miseg_conv3x3_stem_wgrad_ws_bytes(int64_t Cout) { return (int64_t)kStemBlocksMax * Cout * 9 * 4; }

extern "C" int miseg_conv3x3_stem_wgrad(void* stream, int dt, const void* x, int x_f32, int64_t CP, int64_t N, int64_t H, int64_t W, const void* graw,
                                        int64_t Cout, float* gw, void* ws, int64_t ws_bytes) {
    MISEG_TAPE(miseg_conv3x3_stem_wgrad, stream, dt, x, x_f32, CP, N, H, W, graw, Cout, gw, ws, ws_bytes);
    MISEG_F16_DISPATCH_ON(dt, miseg_conv3x3_stem_wgrad, stream, MISEG_BF16, x, x_f32, CP, N, H, W, graw, Cout, gw, ws, ws_bytes);
    MISEG_REQUIRE(x && graw && gw && ws && N > 0 && H > 0 && W > 0, "conv3x3_stem_wgrad: bad args");
    MISEG_REQUIRE(miseg_conv3x3_stem_supported(dt, 1, CP, Cout), "conv3x3_stem_wgrad: 16-bit storage, Cout in {4, 8, 16, 32, 64}");
    MISEG_REQUIRE(ws_bytes >= miseg_conv3x3_stem_wgrad_ws_bytes(Cout), "conv3x3_stem_wgrad: workspace too small");
    MISEG_REQUIRE(W + 2 <= 256 * kStemPre, "conv3x3_stem_wgrad: rows of at most %d pixels", 256 * kStemPre - 2);
    const unsigned nb = (unsigned)std::min<int64_t>(N * H, (int64_t)kStemBlocks);
    hipStream_t st = as_stream(stream);
    if (x_f32)
        hipLaunchKernelGGL((stem_wgrad_kernel<bf16, float>), dim3(nb), dim3(256), (size_t)256 * 37 * 4 + (size_t)5 * (W + 2) * 2, st, (const float*)x, (int)CP, (int)N, (int)H, (int)W,
                           (const bf16*)graw, (int)Cout, (float*)ws);
    else
        hipLaunchKernelGGL((stem_wgrad_kernel<bf16, bf16>), dim3(nb), dim3(256), (size_t)256 * 37 * 4 + (size_t)5 * (W + 2) * 2, st, (const bf16*)x, (int)CP, (int)N, (int)H, (int)W,
                           (const bf16*)graw, (int)Cout, (float*)ws);
    MISEG_LAUNCH_CHECK("stem_wgrad_kernel");
    const int len = (int)(Cout * 9);
    hipLaunchKernelGGL(stem_wgrad_sum_kernel, dim3(reduce_grid(len, nb)), dim3(256), 0, st, (const float*)ws, (int)nb, len, gw);
    MISEG_LAUNCH_CHECK("stem_wgrad_sum_kernel");
    return MISEG_OK;
}

// ---- the stem's data gradient (see stem_dgrad_kernel): every storage type; Cout in whole 16-byte vectors
extern "C" int64_t miseg_conv3x3_stem_dgrad_supported(int dt, int64_t Cout, int64_t W) {
    if (dt != MISEG_F32 && dt != MISEG_BF16 && dt != MISEG_F16) return 0;
    const int vec = dt == MISEG_F32 ? 4 : 8;
    return Cout >= vec && Cout <= 64 && Cout % vec == 0 && W >= 1 && W + 2 <= 256 * kStemPre;
}

extern "C" int64_t miseg_conv3x3_stem_dgrad_ws_bytes(int64_t Cout) { return Cout > 0 ? Cout * 9 * 4 : 0; }

extern "C" int miseg_conv3x3_stem_dgrad(void* stream, int dt, const void* graw, int64_t N, int64_t H, int64_t W, int64_t Cout, const float* w,
                                        float* gimage, void* ws, int64_t ws_bytes) {
    MISEG_TAPE(miseg_conv3x3_stem_dgrad, stream, dt, graw, N, H, W, Cout, w, gimage, ws, ws_bytes);
    MISEG_F16_DISPATCH_ON(dt, miseg_conv3x3_stem_dgrad, stream, MISEG_BF16, graw, N, H, W, Cout, w, gimage, ws, ws_bytes);
    MISEG_REQUIRE(graw && w && gimage && ws && N > 0 && H > 0 && W > 0 && N * H < (1LL << 31), "conv3x3_stem_dgrad: bad args");
    MISEG_REQUIRE(miseg_conv3x3_stem_dgrad_supported(dt, Cout, W), "conv3x3_stem_dgrad: Cout in whole 16-byte vectors up to 64, rows of at most %d pixels "
                  "(ask miseg_conv3x3_stem_dgrad_supported)", 256 * kStemPre - 2);
    MISEG_REQUIRE(((uintptr_t)graw & 15) == 0 && ((uintptr_t)ws & 3) == 0 && ws_bytes >= miseg_conv3x3_stem_dgrad_ws_bytes(Cout),
                  "conv3x3_stem_dgrad: graw must be 16-byte aligned, the workspace miseg_conv3x3_stem_dgrad_ws_bytes large");
    const unsigned nb = (unsigned)std::min<int64_t>(N * H, (int64_t)kStemBlocks);
    const int nw = (int)(Cout * 9);
    hipStream_t st = as_stream(stream);
    MISEG_WITH_STORAGE_TYPE(dt, "conv3x3_stem_dgrad",
        hipLaunchKernelGGL(stem_dgrad_round_w_kernel<TT>, dim3((unsigned)cdiv(nw, 256)), dim3(256), 0, st, w, nw, (float*)ws);
        hipLaunchKernelGGL(stem_dgrad_kernel<TT>, dim3(nb), dim3(256), (size_t)9 * (W + 2) * 4, st, (const TT*)graw, (int)N, (int)H, (int)W, (int)Cout,
                           (const float*)ws, gimage));
    MISEG_LAUNCH_CHECK("stem_dgrad_kernel");
    return MISEG_OK;
}

extern "C" int miseg_conv1x1_fwd(void* stream, int dt, const void* in, int64_t N, int64_t H, int64_t W, int64_t Cin, const float* w,
                                 const float* bias, int64_t Cout, float* out) {
    MISEG_TAPE(miseg_conv1x1_fwd, stream, dt, in, N, H, W, Cin, w, bias, Cout, out);
    MISEG_F16_DISPATCH_ON(dt, miseg_conv1x1_fwd, stream, MISEG_BF16, in, N, H, W, Cin, w, bias, Cout, out);
    MISEG_REQUIRE(in && w && bias && out, "conv1x1_fwd: null pointer");
    MISEG_REQUIRE(Cin == 16, "conv1x1_fwd: Cin must be 16 (unet.py:84)");
    const int64_t npix = N * H * W;
    const int nb = (int)std::min<int64_t>(cdiv(npix, 256), 4096);
    hipStream_t st = as_stream(stream);
#define L(CO) hipLaunchKernelGGL((conv1x1_fwd_kernel<TT, 16, CO>), dim3(nb), dim3(256), 0, st, (const TT*)in, npix, w, bias, out)
    MISEG_WITH_STORAGE_TYPE(dt, "conv1x1_fwd",
        switch (Cout) {
            case 1: L(1); break; case 2: L(2); break; case 3: L(3); break; case 4: L(4); break;
            case 5: L(5); break; case 8: L(8); break;
            default: return fail(MISEG_E_INVALID, "conv1x1_fwd: unsupported Cout %ld", (long)Cout);
        }
        return MISEG_OK);
#undef L
    MISEG_LAUNCH_CHECK("conv1x1_fwd_kernel");
    return MISEG_OK;
}

// 2 blocks per CU: the per-block epilogue (68 wave reductions) costs as much as ~20 pixels of the main loop
static int c1_blocks(int64_t npix) { return (int)std::min<int64_t>(cdiv(npix, 256), 512); }
extern "C" int64_t miseg_conv1x1_bwd_ws_bytes(int64_t N, int64_t H, int64_t W, int64_t Cin, int64_t Cout) {
    return ((int64_t)c1_blocks(N * H * W) + 1) * (Cout * Cin + Cout) * 4;
}

extern "C" int miseg_conv1x1_bwd(void* stream, int dt, const void* in, const float* gout, int64_t N, int64_t H, int64_t W, int64_t Cin,
                                 const float* w, int64_t Cout, void* gin, float* gw, float* gbias, void* ws, int64_t ws_bytes) {
    MISEG_TAPE(miseg_conv1x1_bwd, stream, dt, in, gout, N, H, W, Cin, w, Cout, gin, gw, gbias, ws, ws_bytes);
    MISEG_F16_DISPATCH_ON(dt, miseg_conv1x1_bwd, stream, MISEG_BF16, in, gout, N, H, W, Cin, w, Cout, gin, gw, gbias, ws, ws_bytes);
    MISEG_REQUIRE(in && gout && w && gw && gbias && ws, "conv1x1_bwd: null pointer");
    MISEG_REQUIRE(Cin == 16, "conv1x1_bwd: Cin must be 16");
    MISEG_REQUIRE(ws_bytes >= miseg_conv1x1_bwd_ws_bytes(N, H, W, Cin, Cout), "conv1x1_bwd: workspace too small");
    const int64_t npix = N * H * W;
    const int nb = c1_blocks(npix);
    hipStream_t st = as_stream(stream);
#define L(CO) hipLaunchKernelGGL((conv1x1_bwd_kernel<TT, 16, CO>), dim3(nb), dim3(256), 0, st, (const TT*)in, gout, npix, w, (TT*)gin, (float*)ws)
    MISEG_WITH_STORAGE_TYPE(dt, "conv1x1_bwd",
        switch (Cout) {
            case 1: L(1); break; case 2: L(2); break; case 3: L(3); break; case 4: L(4); break;
            case 5: L(5); break; case 8: L(8); break;
            default: return fail(MISEG_E_INVALID, "conv1x1_bwd: unsupported Cout %ld", (long)Cout);
        }
        return MISEG_OK);
#undef L
    MISEG_LAUNCH_CHECK("conv1x1_bwd_kernel");
    const int len = (int)(Cout * Cin + Cout);
    // the blocks' [gw | gbias] partial vectors, summed straight into the two gradients
    hipLaunchKernelGGL(sum_parts2_kernel, dim3(reduce_grid(len, nb)), dim3(256), 0, st, (const float*)ws, nb, len, (int)(Cout * Cin), gw, gbias);
    MISEG_LAUNCH_CHECK("sum_parts2_kernel");
    return MISEG_OK;
}
