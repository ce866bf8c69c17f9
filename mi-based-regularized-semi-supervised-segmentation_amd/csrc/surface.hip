// Surface-distance statistics of class-coded masks on the device: what Hausdorff, HD95 and the average surface distance are made of
// (ref whl:deepclustering2/meters2/individual_meters/surface_distance.py:9-29 -> medpy.metric.binary.__surface_distances, MedPy 0.4.0).
//
// With unit pixel spacing everything is an integer: a border pixel is a mask pixel with a 4-neighbour outside the mask (outside the
// image counts as outside the mask), the squared Euclidean distance from a border pixel of one mask to the nearest border pixel of the
// other is an integer below 2^20 (H, W <= 512), and so are the counts, the maximum and the order statistics.  Three kernels per call:
//
//   rows   one wave per (pair, side, row): the border flags of the row as ballot words, the number of border pixels (an integer atomic
//          add per row: order-independent) and g[y][x] = distance along the row to the nearest border pixel of that row (uint16,
//          kRowInf when the row has none) -- O(W / 64) per pixel from the ballot words.
//   cols   one block per (pair, direction, strip of 64 columns): the strip of the OTHER side's g in LDS, and for every border pixel of
//          this side D = min over rows y' of (y - y')^2 + g[y'][x]^2, walking outwards from y and stopping once dy^2 reaches the best
//          so far: exact (Felzenszwalb's lower envelope reduced to its definition), at most 2 H reads per pixel whatever the masks hold
//          -- O(H W (H + W)) per pair with the row pass, never border against border.
//   stats  one block per (pair, direction): maximum, sum of the square roots (double, a fixed tree: per-thread strided partial sums in
//          index order, then a fixed pairwise tree over the threads) and the two order statistics by a two-level radix select over
//          integer histograms (bits 19..10, then bits 9..0).  Integer atomics only: two calls give the same bits.
//
// A pair with an empty mask on either side gets zeros everywhere (its column blocks return at once).
#include "common.h"
#include <math.h>

namespace miseg {
namespace {

constexpr int kRowInf = 0x7fff;          // "no border pixel in this row": its square plus 511^2 still fits an int32
constexpr int kStrip = 64;               // columns per block of the column pass = one wave across
constexpr int kColsThreads = 1024;
constexpr int kStatsThreads = 1024;
constexpr int kBins = 1024;              // per radix level: squared distances are < 2^20
constexpr int kMaxSide = 512;

// grid (ceil(H / 4), pairs * 2): blockIdx.y = pair * 2 + side (0 = pred, 1 = target); 4 waves = 4 rows, no block-wide step
__global__ __launch_bounds__(256) void surface_rows_kernel(const int64_t* __restrict__ pred, const int64_t* __restrict__ target,
                                                           const int32_t* __restrict__ classes, int K, int H, int W,
                                                           int* __restrict__ count, unsigned short* __restrict__ g) {
    const int lane = threadIdx.x & 63, y = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (y >= H) return;
    const int ps = blockIdx.y, pair = ps >> 1, b = pair / K;
    const int64_t c = classes[pair - b * K];
    const int64_t* m = ((ps & 1) ? target : pred) + (size_t)b * H * W;
    unsigned long long bits[kMaxSide / 64];
    int n = 0;
#pragma unroll
    for (int ch = 0; ch < kMaxSide / 64; ++ch) {
        const int x = ch * 64 + lane;
        bool f = false;
        if (x < W && m[(size_t)y * W + x] == c)
            f = y == 0 || y == H - 1 || x == 0 || x == W - 1 || m[(size_t)(y - 1) * W + x] != c || m[(size_t)(y + 1) * W + x] != c ||
                m[(size_t)y * W + x - 1] != c || m[(size_t)y * W + x + 1] != c;
        bits[ch] = __ballot(f);
        n += __builtin_popcountll(bits[ch]);
    }
    if (lane == 0 && n) atomicAdd(&count[ps], n);
    constexpr int kFar = 1 << 20;
    int nxt[kMaxSide / 64], after = kFar;            // the first border pixel in the words behind word ch
#pragma unroll
    for (int ch = kMaxSide / 64 - 1; ch >= 0; --ch) {
        nxt[ch] = after;
        if (bits[ch]) after = ch * 64 + __builtin_ctzll(bits[ch]);
    }
    unsigned short* grow = g + ((size_t)ps * H + y) * W;
    int before = -kFar;                              // the last border pixel in the words before word ch
#pragma unroll
    for (int ch = 0; ch < kMaxSide / 64; ++ch) {
        const int x = ch * 64 + lane;
        const unsigned long long w = bits[ch], lo = w & (~0ull >> (63 - lane)), hi = w & (~0ull << lane);
        const int l = lo ? ch * 64 + 63 - __builtin_clzll(lo) : before;
        const int r = hi ? ch * 64 + __builtin_ctzll(hi) : nxt[ch];
        if (x < W) grow[x] = (unsigned short)min(min(x - l, r - x), kRowInf);
        if (w) before = ch * 64 + 63 - __builtin_clzll(w);
    }
}

// grid (ceil(W / 64), pairs * 2): blockIdx.y = pair * 2 + direction; direction d goes from the border of side d to that of side 1 - d.
// Dynamic LDS: H * 64 uint16, the other side's g for this strip of columns.  16 waves take the rows in turn; the walk is a chain of LDS
// round trips, so it goes four steps (eight independent reads) at a time.  A step past the image edge re-reads the edge row with a larger
// dy -- never below what that row gave at its own distance -- and so do the up to three steps past the stopping point.
__global__ __launch_bounds__(kColsThreads) void surface_cols_kernel(const unsigned short* __restrict__ g, const int* __restrict__ count, int H,
                                                                    int W, int* __restrict__ dist) {
    extern __shared__ __align__(16) unsigned short sg[];
    const int pd = blockIdx.y;
    if (count[pd] == 0 || count[pd ^ 1] == 0) return;            // block-uniform
    const int x0 = blockIdx.x * kStrip;
    const unsigned short* gsrc = g + (size_t)pd * H * W;
    const unsigned short* gdst = g + (size_t)(pd ^ 1) * H * W;
    for (int i = threadIdx.x; i < H * kStrip; i += kColsThreads) {
        const int y = i / kStrip, x = x0 + (i % kStrip);
        sg[i] = x < W ? gdst[(size_t)y * W + x] : (unsigned short)kRowInf;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, x = x0 + lane;
    if (x >= W) return;
    int* drow = dist + (size_t)pd * H * W;
    for (int y = threadIdx.x >> 6; y < H; y += kColsThreads / 64) {
        int best = -1;                                           // not a border pixel of this side
        if (gsrc[(size_t)y * W + x] == 0) {
            const int v = sg[y * kStrip + lane];
            best = v * v;
            for (int dy = 1; dy < H && dy * dy < best; dy += 4) {   // a row dy away cannot give less than dy^2
                int up[4], dn[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    up[u] = sg[max(y - dy - u, 0) * kStrip + lane];
                    dn[u] = sg[min(y + dy + u, H - 1) * kStrip + lane];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) best = min(best, min(up[u] * up[u], dn[u] * dn[u]) + (dy + u) * (dy + u));
            }
        }
        drow[(size_t)y * W + x] = best;
    }
}

// Bin of `hist` (kBins bins, one per thread) that holds the element of rank `rank` (0-based, ascending), and the number of elements
// in the bins before it.  `scan` = 17 ints of LDS, `res` = 2.  Every thread gets the answer.
__device__ __forceinline__ void find_bin(const int* hist, long long rank, int* scan, int* res, int& bin, int& below) {
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int own = hist[tid];
    int incl = own;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    __syncthreads();
    if (lane == 63) scan[wid] = incl;
    __syncthreads();
    int base = 0;
    for (int i = 0; i < wid; ++i) base += scan[i];
    incl += base;
    if ((long long)(incl - own) <= rank && rank < (long long)incl) { res[0] = tid; res[1] = incl - own; }
    __syncthreads();
    bin = res[0];
    below = res[1];
}

// grid (pairs * 2), kStatsThreads threads
__global__ __launch_bounds__(kStatsThreads) void surface_stats_kernel(const int* __restrict__ dist, const int* __restrict__ count, int HW,
                                                                      double q, int64_t* __restrict__ stats, double* __restrict__ sum_dist) {
    __shared__ int h_hi[kBins], h_a[kBins], h_b[kBins], s_max[kStatsThreads / 64], scan[17], res[2];
    __shared__ double s_sum[kStatsThreads];
    const int pd = blockIdx.x, tid = threadIdx.x;
    const int n = count[pd];
    if (n == 0 || count[pd ^ 1] == 0) {                          // block-uniform
        if (tid < 4) stats[(size_t)pd * 4 + tid] = 0;
        if (tid == 0) sum_dist[pd] = 0.0;
        return;
    }
    const int* d = dist + (size_t)pd * HW;
    h_hi[tid] = 0; h_a[tid] = 0; h_b[tid] = 0;
    __syncthreads();
    int mx = 0;
    double s = 0.0;
    for (int i = tid; i < HW; i += kStatsThreads) {
        const int v = d[i];
        if (v >= 0) {
            mx = max(mx, v);
            s += sqrt((double)v);
            atomicAdd(&h_hi[v >> 10], 1);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = max(mx, __shfl_xor(mx, o, 64));
    if ((tid & 63) == 0) s_max[tid >> 6] = mx;
    s_sum[tid] = s;
    __syncthreads();
    for (int o = kStatsThreads / 2; o > 0; o >>= 1) {            // the fixed tree: thread t adds what thread t + o holds
        if (tid < o) s_sum[tid] += s_sum[tid + o];
        __syncthreads();
    }
    const double v = (double)(n - 1) * q;                        // numpy's virtual index of np.percentile(.., 100 q)
    const long long rlo = (long long)floor(v), rhi = (long long)ceil(v);
    int bin_lo, below_lo, bin_hi, below_hi;
    find_bin(h_hi, rlo, scan, res, bin_lo, below_lo);
    find_bin(h_hi, rhi, scan, res, bin_hi, below_hi);
    for (int i = tid; i < HW; i += kStatsThreads) {
        const int e = d[i];
        if (e >= 0) {
            if ((e >> 10) == bin_lo) atomicAdd(&h_a[e & (kBins - 1)], 1);
            if ((e >> 10) == bin_hi) atomicAdd(&h_b[e & (kBins - 1)], 1);
        }
    }
    __syncthreads();
    int low_lo, low_hi, unused;
    find_bin(h_a, rlo - below_lo, scan, res, low_lo, unused);
    find_bin(h_b, rhi - below_hi, scan, res, low_hi, unused);
    if (tid == 0) {
        int m = s_max[0];
        for (int i = 1; i < kStatsThreads / 64; ++i) m = max(m, s_max[i]);
        int64_t* o = stats + (size_t)pd * 4;
        o[0] = n; o[1] = m; o[2] = (bin_lo << 10) | low_lo; o[3] = (bin_hi << 10) | low_hi;
        sum_dist[pd] = s_sum[0];
    }
}

// scratch: [border counts: pairs * 2 int32] [g: pairs * 2 * H * W uint16] [squared distances: pairs * 2 * H * W int32], each part 256-byte aligned
struct SurfaceWs {
    size_t count, g, dist, total;
};
SurfaceWs surface_ws(int64_t N, int64_t H, int64_t W, int64_t K) {
    const size_t sides = (size_t)N * K * 2, px = sides * H * W;
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    SurfaceWs w;
    w.count = 0;
    w.g = up(sides * 4);
    w.dist = w.g + up(px * 2);
    w.total = w.dist + up(px * 4);
    return w;
}
bool surface_shape_ok(int64_t N, int64_t H, int64_t W, int64_t K) {
    return N > 0 && K > 0 && H > 0 && W > 0 && H <= kMaxSide && W <= kMaxSide && N * K * 2 <= 65535;
}

}  // namespace
}  // namespace miseg

using namespace miseg;

extern "C" int64_t miseg_surface_stats_ws_bytes(int64_t N, int64_t H, int64_t W, int64_t n_classes) {
    if (!surface_shape_ok(N, H, W, n_classes)) return -1;
    return (int64_t)surface_ws(N, H, W, n_classes).total;
}

extern "C" int miseg_surface_stats(void* stream, const int64_t* pred, const int64_t* target, int64_t N, int64_t H, int64_t W,
                                   const int32_t* classes, int64_t n_classes, double q, int64_t* stats, double* sum_dist, void* ws,
                                   int64_t ws_bytes) {
    MISEG_TAPE(miseg_surface_stats, stream, pred, target, N, H, W, classes, n_classes, q, stats, sum_dist, ws, ws_bytes);
    MISEG_REQUIRE(pred && target && classes && stats && sum_dist && ws, "surface_stats: null pointer");
    MISEG_REQUIRE(surface_shape_ok(N, H, W, n_classes), "surface_stats: bad shape (H, W <= 512, N * n_classes <= 32767)");
    MISEG_REQUIRE(q >= 0.0 && q <= 1.0, "surface_stats: q must lie in [0, 1]");      // a NaN fails both comparisons
    const SurfaceWs lay = surface_ws(N, H, W, n_classes);
    MISEG_REQUIRE(ws_bytes >= (int64_t)lay.total, "surface_stats: workspace too small");
    MISEG_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 15) == 0, "surface_stats: workspace must be 16-byte aligned");
    hipStream_t st = as_stream(stream);
    char* base = static_cast<char*>(ws);
    int* count = reinterpret_cast<int*>(base + lay.count);
    unsigned short* g = reinterpret_cast<unsigned short*>(base + lay.g);
    int* dist = reinterpret_cast<int*>(base + lay.dist);
    const unsigned sides = (unsigned)(N * n_classes * 2);
    hipMemsetAsync(count, 0, (size_t)sides * 4, st);
    hipLaunchKernelGGL(surface_rows_kernel, dim3((unsigned)cdiv(H, 4), sides), dim3(256), 0, st, pred, target, classes, (int)n_classes,
                       (int)H, (int)W, count, g);
    MISEG_LAUNCH_CHECK("surface_rows_kernel");
    const size_t lds = (size_t)H * kStrip * 2;                   // 64 KiB at H = 512
    if (lds > 48 * 1024) hipFuncSetAttribute((const void*)surface_cols_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(surface_cols_kernel, dim3((unsigned)cdiv(W, kStrip), sides), dim3(kColsThreads), lds, st, g, count, (int)H, (int)W, dist);
    MISEG_LAUNCH_CHECK("surface_cols_kernel");
    hipLaunchKernelGGL(surface_stats_kernel, dim3(sides), dim3(kStatsThreads), 0, st, dist, count, (int)(H * W), q, stats, sum_dist);
    MISEG_LAUNCH_CHECK("surface_stats_kernel");
    return MISEG_OK;
}
