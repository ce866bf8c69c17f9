// Keep the largest connected component of each listed class of a class-coded mask, on the device.  The
// reference project has no post-processing: the definition is this project's own, pinned to scipy.ndimage.label + bincount
// (include/miseg_hip.h, miseg_largest_component).
//
// The labelling is a union-find over pixel indices in which a label only ever DECREASES (every write of a label is an integer
// minimum) and whose end state -- every pixel points at the smallest index of its component -- does not depend on the order of the
// merges: two calls give the same bits.  g = (n * H + y) * W + x is the pixel's index in the call; a unit (a slice for rank 2, the
// volume for rank 3) is a contiguous range of g, so the order of g inside a unit is the order of the unit's own pixel index.
// Six launches on the stream, each one depending on the whole of the one before:
//
//   init     the class table lut[64] (value -> listed?) from the device class list; zeroes the per-(unit, class) cells and inter / uni.
//   tile     one block per 64 x 64 tile of a slice: labels in LDS (16 KiB) + the class values (4 KiB).  Row runs by pointer doubling,
//            then every pixel is merged with its upper neighbours, then flattened; parent[g] = g of the tile-local root (-1 for a
//            pixel that is not of a listed class), size[g] = 0.
//   border   one thread per pixel of a tile's first column / first row (and, for rank 3, per pixel of every slice but the first):
//            merges with the neighbours in the tile to the left / above (the slice before).  Agent-scope atomics only.
//   flatten  parent[g] = root of g (path compression), then one integer add per pixel into size[root], one per wave where the wave
//            holds a single component.
//   select   every root offers (size << 32) | (0xFFFFFFFF - root) to its (unit, class) cell by a 64-bit integer maximum -- the larger
//            component wins, among equals the one with the smaller first pixel -- and is counted; reduced per block in LDS first.
//   rewrite  out = pred where the pixel's root is the kept one, else fill; labels; the Dice counts of out against target (LDS
//            histograms per block, then 64-bit integer adds); block 0 writes stats.
//
// Integer only: no floating point anywhere in this unit.
#include "common.h"

namespace miseg {
namespace {

constexpr int kTile = 64;                    // tile side: 4096 32-bit labels = 16 KiB of LDS
constexpr int kTilePx = kTile * kTile;
constexpr int kTileThreads = 1024;
constexpr int kMaxSide = 2048;
constexpr int kMaxVal = 64;                  // class values, fill and the Dice class count live in [0, 64)
constexpr int kPxThreads = 256;
constexpr int kPxPerBlock = 1024;            // pixels per block of the select and rewrite kernels (4 per thread)
constexpr unsigned char kNoClass = 255;

#define CC_RLX_WG __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP
#define CC_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

// ---- init: grid-stride, any grid.  A class value outside [0, 64) or equal to fill lists nothing; a repeated value lists once.
__global__ __launch_bounds__(256) void cc_init_kernel(const int32_t* __restrict__ classes, int K, int fill, signed char* __restrict__ lut,
                                                      unsigned long long* __restrict__ best, int* __restrict__ cnt, int* __restrict__ tot,
                                                      int64_t cells, unsigned long long* __restrict__ inter,
                                                      unsigned long long* __restrict__ uni, int64_t dice_cells) {
    const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
    if (t0 < kMaxVal) {
        int slot = -1;
        for (int k = K - 1; k >= 0; --k)                         // K <= 64 steps; the first entry with this value gives the slot
            if (classes[k] == (int32_t)t0) slot = k;
        lut[t0] = (signed char)((int)t0 == fill ? -1 : slot);
    }
    for (int64_t i = t0; i < cells; i += step) { best[i] = 0ull; cnt[i] = 0; tot[i] = 0; }
    for (int64_t i = t0; i < dice_cells; i += step) { inter[i] = 0ull; uni[i] = 0ull; }
}

// ---- union-find in LDS.  Invariant: L[i] <= i, and every write is an atomic minimum (or the initial store), so labels only decrease.
__device__ __forceinline__ int lds_find(int* L, int x) {
    // ends by itself: L[x] < x for every x that is not a root, so x strictly decreases and is bounded by 0
    for (;;) {
        const int l = __hip_atomic_load(&L[x], CC_RLX_WG);
        if (l >= x) return x;                                     // l == x: the root
        x = l;
    }
}
__device__ __forceinline__ void lds_union(int* L, int a, int b) {
    // ends by itself: a and b are the roots as read (a stale read gives an ancestor, which is as good); the atomic minimum on the
    // larger one decides.  If it did not find a root there (old != a) the pair becomes (old, b) with old < a: max(a, b) strictly
    // decreases from one round to the next and is bounded by 0.  Nobody waits for anybody.
    for (;;) {
        a = lds_find(L, a);
        b = lds_find(L, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = __hip_atomic_fetch_min(&L[a], b, CC_RLX_WG);
        if (old == a) return;
        a = old;
    }
}

// grid (N * tiles_y * tiles_x), 1024 threads, 4 pixels each.  Local index i = ly * 64 + lx grows with g inside the tile.
__global__ __launch_bounds__(kTileThreads) void cc_tile_kernel(const int64_t* __restrict__ pred, const signed char* __restrict__ lut, int H,
                                                               int W, int tiles_x, int tiles_y, int conn, int* __restrict__ parent,
                                                               int* __restrict__ size) {
    __shared__ int L[kTilePx];
    __shared__ unsigned char cls[kTilePx];
    __shared__ signed char s_lut[kMaxVal];
    const int tid = threadIdx.x;
    const int per = tiles_x * tiles_y, n = blockIdx.x / per, t = blockIdx.x - n * per, ty = t / tiles_x, tx = t - ty * tiles_x;
    const int y0 = ty * kTile, x0 = tx * kTile;
    const size_t base = (size_t)n * H * W;
    if (tid < kMaxVal) s_lut[tid] = lut[tid];
    __syncthreads();
    for (int i = tid; i < kTilePx; i += kTileThreads) {
        const int y = y0 + (i >> 6), x = x0 + (i & 63);
        unsigned char c = kNoClass;
        if (y < H && x < W) {
            const int64_t v = pred[base + (size_t)y * W + x];
            if (v >= 0 && v < kMaxVal && s_lut[v] >= 0) c = (unsigned char)v;
        }
        cls[i] = c;
    }
    __syncthreads();
    for (int i = tid; i < kTilePx; i += kTileThreads) {
        const unsigned char c = cls[i];
        L[i] = (c != kNoClass && (i & 63) && cls[i - 1] == c) ? i - 1 : i;
    }
    __syncthreads();
    // row runs: six rounds of pointer doubling reach the first pixel of a run of up to 64.  A racing read returns an older label,
    // which is still a pixel of the same run further to the right of the target: the value written is never below the run's start.
#pragma unroll 1
    for (int round = 0; round < 6; ++round) {
        for (int i = tid; i < kTilePx; i += kTileThreads) {
            const int l = __hip_atomic_load(&L[i], CC_RLX_WG);
            const int ll = __hip_atomic_load(&L[l], CC_RLX_WG);
            if (ll < l) __hip_atomic_fetch_min(&L[i], ll, CC_RLX_WG);
        }
        __syncthreads();
    }
    for (int i = tid; i < kTilePx; i += kTileThreads) {
        const unsigned char c = cls[i];
        if (c == kNoClass || i < kTile) continue;
        const int lx = i & 63;
        if (cls[i - kTile] == c) lds_union(L, i, i - kTile);
        else if (conn == 2) {                                     // with the pixel above joined, its row neighbours follow from the runs
            if (lx > 0 && cls[i - kTile - 1] == c) lds_union(L, i, i - kTile - 1);
            if (lx < kTile - 1 && cls[i - kTile + 1] == c) lds_union(L, i, i - kTile + 1);
        }
    }
    __syncthreads();
    int root[kTilePx / kTileThreads];
#pragma unroll
    for (int j = 0; j < kTilePx / kTileThreads; ++j) {
        const int i = tid + j * kTileThreads;
        root[j] = cls[i] == kNoClass ? -1 : lds_find(L, i);
    }
#pragma unroll
    for (int j = 0; j < kTilePx / kTileThreads; ++j) {
        const int i = tid + j * kTileThreads, y = y0 + (i >> 6), x = x0 + (i & 63);
        if (y < H && x < W) {
            const size_t g = base + (size_t)y * W + x;
            parent[g] = root[j] < 0 ? -1 : (int)(base + (size_t)(y0 + (root[j] >> 6)) * W + x0 + (root[j] & 63));
            size[g] = 0;
        }
    }
}

// ---- union-find in global memory.  parent[g] <= g; inside a launch every access is an agent-scope atomic and every write a minimum.
__device__ __forceinline__ int cc_find(int* parent, int x) {
    // ends by itself: parent[x] < x for every x that is not a root, so x strictly decreases and is bounded by 0.  A read that
    // returns an older label returns an ancestor.
    const int start = x;
    int hops = 0;
    for (;;) {
        const int l = __hip_atomic_load(&parent[x], CC_RLX_AGENT);
        if (l >= x || l < 0) break;                               // l == x: the root (the other two cannot be; they keep the index in range)
        x = l;
        ++hops;
    }
    if (hops <= 1) return x;                                      // the start is the root or points at it: nothing to shorten
    // path compression: the same walk again (it ends for the same reason, at the latest at the root found), every pixel on it
    // lowered to that root -- a minimum with an ancestor, so the invariant and the component stay what they are.
    int y = start;
    while (y > x) {
        const int l = __hip_atomic_load(&parent[y], CC_RLX_AGENT);
        if (l > x) __hip_atomic_fetch_min(&parent[y], x, CC_RLX_AGENT);
        if (l >= y || l < 0) break;                                   // a root (cannot be: y > x is on the path), kept for the bound
        y = l;
    }
    return x;
}
__device__ __forceinline__ void cc_union(int* parent, int a, int b) {
    // ends by itself: as lds_union -- after a round that does not return, the pair is (old, b) with old < a, so max(a, b)
    // strictly decreases and is bounded by 0.  No thread waits for a value another one has yet to write.
    for (;;) {
        a = cc_find(parent, a);
        b = cc_find(parent, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = __hip_atomic_fetch_min(&parent[a], b, CC_RLX_AGENT);
        if (old == a) return;
        a = old;
    }
}

// One thread per pixel; only the pixels on the first column / row of a tile (not of the image) and, for rank 3, of the slices after
// the first do anything.  pred is read-only in this launch (plain loads); the neighbours' indices are bounds-checked.
__global__ __launch_bounds__(kPxThreads) void cc_border_kernel(const int64_t* __restrict__ pred, int64_t total, int H, int W, int rank,
                                                               int conn, int* __restrict__ parent) {
    const int64_t g = (int64_t)blockIdx.x * kPxThreads + threadIdx.x;
    if (g >= total) return;
    const int64_t HW = (int64_t)H * W;
    const int n = (int)(g / HW), rem = (int)(g - (int64_t)n * HW), y = rem / W, x = rem - y * W;
    const bool left = x > 0 && (x & (kTile - 1)) == 0, top = y > 0 && (y & (kTile - 1)) == 0, prev = rank == 3 && n > 0;
    if (!(left || top || prev)) return;
    if (__hip_atomic_load(&parent[g], CC_RLX_AGENT) < 0) return;  // not of a listed class (tile_kernel's -1 is never changed)
    const int64_t v = pred[g];
    auto join = [&](int64_t q) {
        if (pred[q] == v) cc_union(parent, (int)g, (int)q);
    };
    if (left) {
        join(g - 1);
        if (conn == 2) {
            if (y > 0) join(g - W - 1);
            if (y < H - 1) join(g + W - 1);
        }
    }
    if (top) {
        join(g - W);
        if (conn == 2) {
            if (x > 0) join(g - W - 1);
            if (x < W - 1) join(g - W + 1);
        }
    }
    if (prev) {
        join(g - HW);
        if (conn == 2)
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx)
                    if ((dy || dx) && y + dy >= 0 && y + dy < H && x + dx >= 0 && x + dx < W) join(g - HW + (int64_t)dy * W + dx);
    }
}

// One thread per pixel.  The merges are complete (previous launch): cc_find returns the final root whatever the compression of the
// other threads has done so far.
__global__ __launch_bounds__(kPxThreads) void cc_flatten_kernel(int64_t total, int* __restrict__ parent, int* __restrict__ size) {
    const int64_t g = (int64_t)blockIdx.x * kPxThreads + threadIdx.x;
    int r = -1;
    if (g < total && __hip_atomic_load(&parent[g], CC_RLX_AGENT) >= 0) r = cc_find(parent, (int)g);
    const unsigned long long fg = __ballot(r >= 0);
    if (!fg) return;
    const int r0 = __shfl(r, __builtin_ctzll(fg), 64);
    if (__ballot(r == r0) == fg) {                                // the wave holds one component: one add
        if ((int)(threadIdx.x & 63) == __builtin_ctzll(fg)) __hip_atomic_fetch_add(&size[r0], __builtin_popcountll(fg), CC_RLX_AGENT);
    } else if (r >= 0) {
        __hip_atomic_fetch_add(&size[r], 1, CC_RLX_AGENT);
    }
}

// grid (units_or_slices * chunks): block b covers pixels [chunk * 1024, +1024) of slice b / chunks, so a block lies in one unit.
__global__ __launch_bounds__(kPxThreads) void cc_select_kernel(const int64_t* __restrict__ pred, const signed char* __restrict__ lut,
                                                               int64_t HW, int chunks, int K, int rank, const int* __restrict__ parent,
                                                               const int* __restrict__ size, unsigned long long* __restrict__ best,
                                                               int* __restrict__ cnt, int* __restrict__ tot) {
    __shared__ unsigned long long s_best[kMaxVal];
    __shared__ int s_cnt[kMaxVal], s_tot[kMaxVal];
    const int tid = threadIdx.x, n = blockIdx.x / chunks, chunk = blockIdx.x - n * chunks;
    if (tid < kMaxVal) { s_best[tid] = 0ull; s_cnt[tid] = 0; s_tot[tid] = 0; }
    __syncthreads();
    for (int j = 0; j < kPxPerBlock / kPxThreads; ++j) {
        const int64_t i = (int64_t)chunk * kPxPerBlock + j * kPxThreads + tid;
        if (i >= HW) break;
        const int64_t g = (int64_t)n * HW + i;
        if (parent[g] != (int)g) continue;                        // roots only
        const int k = lut[pred[g]];                               // a root is of a listed class: the value is in [0, 64)
        const int s = size[g];
        atomicMax(&s_best[k], ((unsigned long long)(unsigned)s << 32) | (0xFFFFFFFFull - (unsigned long long)g));
        atomicAdd(&s_cnt[k], 1);
        atomicAdd(&s_tot[k], s);
    }
    __syncthreads();
    if (tid < K && s_cnt[tid]) {
        const size_t cell = (size_t)(rank == 3 ? 0 : n) * K + tid;
        __hip_atomic_fetch_max(&best[cell], s_best[tid], CC_RLX_AGENT);
        __hip_atomic_fetch_add(&cnt[cell], s_cnt[tid], CC_RLX_AGENT);
        __hip_atomic_fetch_add(&tot[cell], s_tot[tid], CC_RLX_AGENT);
    }
}

// Same grid.  out may be pred: a thread reads pred[g] before it writes out[g], and reads no other pixel of pred.
__global__ __launch_bounds__(kPxThreads) void cc_rewrite_kernel(const int64_t* pred, const signed char* __restrict__ lut, int64_t HW,
                                                                int chunks, int K, int rank, int64_t fill, const int* __restrict__ parent,
                                                                const unsigned long long* __restrict__ best, const int* __restrict__ cnt,
                                                                const int* __restrict__ tot, int64_t cells, int64_t* out,
                                                                int32_t* __restrict__ labels, int64_t* __restrict__ stats,
                                                                const int64_t* __restrict__ target, int C,
                                                                unsigned long long* __restrict__ inter, unsigned long long* __restrict__ uni) {
    __shared__ unsigned int s_inter[kMaxVal], s_uni[kMaxVal];
    __shared__ int s_keep[kMaxVal];
    const int tid = threadIdx.x, n = blockIdx.x / chunks, chunk = blockIdx.x - n * chunks;
    const int unit = rank == 3 ? 0 : n;
    if (tid < kMaxVal) {
        s_inter[tid] = 0u; s_uni[tid] = 0u;
        // an absent class has best == 0: its "kept root" is 0xFFFFFFFF = -1, which no pixel of a listed class has for a parent
        s_keep[tid] = tid < K ? (int)(0xFFFFFFFFu - (unsigned)(best[(size_t)unit * K + tid] & 0xFFFFFFFFull)) : -1;
    }
    if (blockIdx.x == 0)
        for (int64_t c = tid; c < cells; c += kPxThreads) {
            stats[c * 3 + 0] = cnt[c];
            stats[c * 3 + 1] = (int64_t)(best[c] >> 32);
            stats[c * 3 + 2] = tot[c];
        }
    __syncthreads();
    const int64_t ubase = rank == 3 ? 0 : (int64_t)n * HW;
    for (int j = 0; j < kPxPerBlock / kPxThreads; ++j) {
        const int64_t i = (int64_t)chunk * kPxPerBlock + j * kPxThreads + tid;
        if (i >= HW) break;
        const int64_t g = (int64_t)n * HW + i;
        int64_t v = pred[g];
        const int r = parent[g];
        if (r >= 0 && r != s_keep[lut[v]]) v = fill;
        out[g] = v;
        if (labels) labels[g] = r < 0 ? -1 : (int32_t)(r - ubase);
        if (target) {
            const int64_t t = target[g];
            const bool vin = v >= 0 && v < C, tin = t >= 0 && t < C;
            if (vin) atomicAdd(&s_uni[v], 1u);
            if (tin) atomicAdd(&s_uni[t], 1u);
            if (vin && t == v) atomicAdd(&s_inter[v], 1u);
        }
    }
    if (!target) return;                                          // uniform
    __syncthreads();
    if (tid < C) {
        if (s_inter[tid]) __hip_atomic_fetch_add(&inter[(size_t)n * C + tid], (unsigned long long)s_inter[tid], CC_RLX_AGENT);
        if (s_uni[tid]) __hip_atomic_fetch_add(&uni[(size_t)n * C + tid], (unsigned long long)s_uni[tid], CC_RLX_AGENT);
    }
}

// scratch: [lut: 64 int8] [best: cells uint64] [cnt: cells int32] [tot: cells int32] [parent: px int32] [size: px int32], each part
// 256-byte aligned; cells = units * n_classes
struct ComponentsWs {
    size_t lut, best, cnt, tot, parent, size, total;
};
ComponentsWs components_ws(int64_t N, int64_t H, int64_t W, int64_t K, int rank) {
    const size_t cells = (size_t)(rank == 3 ? 1 : N) * K, px = (size_t)N * H * W;
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    ComponentsWs w;
    w.lut = 0;
    w.best = up(kMaxVal);
    w.cnt = w.best + up(cells * 8);
    w.tot = w.cnt + up(cells * 4);
    w.parent = w.tot + up(cells * 4);
    w.size = w.parent + up(px * 4);
    w.total = w.size + up(px * 4);
    return w;
}
bool components_shape_ok(int64_t N, int64_t H, int64_t W, int64_t K, int rank) {
    if (!(N >= 1 && H >= 1 && W >= 1 && H <= kMaxSide && W <= kMaxSide && K >= 1 && K <= kMaxVal && (rank == 2 || rank == 3))) return false;
    return N <= ((int64_t)1 << 31) && N * H * W < ((int64_t)1 << 31);      // H * W <= 2^22: the product cannot overflow
}

}  // namespace
}  // namespace miseg

using namespace miseg;

extern "C" int64_t miseg_largest_component_ws_bytes(int64_t N, int64_t H, int64_t W, int64_t n_classes, int rank) {
    if (!components_shape_ok(N, H, W, n_classes, rank)) return -1;
    return (int64_t)components_ws(N, H, W, n_classes, rank).total;
}

extern "C" int miseg_largest_component(void* stream, const int64_t* pred, int64_t N, int64_t H, int64_t W, const int32_t* classes,
                                       int64_t n_classes, int rank, int connectivity, int64_t fill, int64_t* out, int32_t* labels,
                                       int64_t* stats, const int64_t* target, int64_t C, int64_t* inter, int64_t* uni, void* ws,
                                       int64_t ws_bytes) {
    MISEG_TAPE(miseg_largest_component, stream, pred, N, H, W, classes, n_classes, rank, connectivity, fill, out, labels, stats, target, C,
               inter, uni, ws, ws_bytes);
    MISEG_REQUIRE(pred && classes && out && stats && ws, "largest_component: null pointer");
    MISEG_REQUIRE(rank == 2 || rank == 3, "largest_component: rank must be 2 or 3");
    MISEG_REQUIRE(connectivity == 1 || connectivity == 2, "largest_component: connectivity must be 1 or 2");
    MISEG_REQUIRE(components_shape_ok(N, H, W, n_classes, rank),
                  "largest_component: bad shape (1 <= H, W <= 2048, fewer than 2^31 pixels, 1 <= n_classes <= 64)");
    MISEG_REQUIRE(fill >= 0 && fill < kMaxVal, "largest_component: fill must lie in [0, 64)");
    if (target) {
        MISEG_REQUIRE(inter && uni, "largest_component: target without inter / uni");
        MISEG_REQUIRE(C >= 1 && C <= kMaxVal, "largest_component: the Dice class count must lie in [1, 64]");
    }
    const ComponentsWs lay = components_ws(N, H, W, n_classes, rank);
    MISEG_REQUIRE(ws_bytes >= (int64_t)lay.total, "largest_component: workspace too small");
    MISEG_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 15) == 0, "largest_component: workspace must be 16-byte aligned");
    hipStream_t st = as_stream(stream);
    char* base = static_cast<char*>(ws);
    signed char* lut = reinterpret_cast<signed char*>(base + lay.lut);
    unsigned long long* best = reinterpret_cast<unsigned long long*>(base + lay.best);
    int* cnt = reinterpret_cast<int*>(base + lay.cnt);
    int* tot = reinterpret_cast<int*>(base + lay.tot);
    int* parent = reinterpret_cast<int*>(base + lay.parent);
    int* size = reinterpret_cast<int*>(base + lay.size);
    const int K = (int)n_classes;
    const int64_t HW = H * W, total = N * HW, cells = (rank == 3 ? 1 : N) * n_classes, dice_cells = target ? N * C : 0;
    const int tiles_x = (int)cdiv(W, kTile), tiles_y = (int)cdiv(H, kTile), chunks = (int)cdiv(HW, kPxPerBlock);
    unsigned long long* uinter = reinterpret_cast<unsigned long long*>(inter);
    unsigned long long* uuni = reinterpret_cast<unsigned long long*>(uni);
    const unsigned init_blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>(cdiv(std::max(cells, dice_cells), 256), 1024));
    hipLaunchKernelGGL(cc_init_kernel, dim3(init_blocks), dim3(256), 0, st, classes, K, (int)fill, lut, best, cnt, tot, cells, uinter, uuni,
                       dice_cells);
    MISEG_LAUNCH_CHECK("cc_init_kernel");
    hipLaunchKernelGGL(cc_tile_kernel, dim3((unsigned)(N * tiles_x * tiles_y)), dim3(kTileThreads), 0, st, pred, lut, (int)H, (int)W, tiles_x,
                       tiles_y, connectivity, parent, size);
    MISEG_LAUNCH_CHECK("cc_tile_kernel");
    const unsigned px_blocks = (unsigned)cdiv(total, kPxThreads);
    if (tiles_x > 1 || tiles_y > 1 || (rank == 3 && N > 1)) {     // otherwise no two tiles touch
        hipLaunchKernelGGL(cc_border_kernel, dim3(px_blocks), dim3(kPxThreads), 0, st, pred, total, (int)H, (int)W, rank, connectivity, parent);
        MISEG_LAUNCH_CHECK("cc_border_kernel");
    }
    hipLaunchKernelGGL(cc_flatten_kernel, dim3(px_blocks), dim3(kPxThreads), 0, st, total, parent, size);
    MISEG_LAUNCH_CHECK("cc_flatten_kernel");
    const unsigned chunk_blocks = (unsigned)(N * chunks);
    hipLaunchKernelGGL(cc_select_kernel, dim3(chunk_blocks), dim3(kPxThreads), 0, st, pred, lut, HW, chunks, K, rank, parent, size, best, cnt, tot);
    MISEG_LAUNCH_CHECK("cc_select_kernel");
    hipLaunchKernelGGL(cc_rewrite_kernel, dim3(chunk_blocks), dim3(kPxThreads), 0, st, pred, lut, HW, chunks, K, rank, fill, parent, best, cnt,
                       tot, cells, out, labels, stats, target, (int)C, uinter, uuni);
    MISEG_LAUNCH_CHECK("cc_rewrite_kernel");
    return MISEG_OK;
}
