// The library's counter-based generator: Philox4x32-10 and the Box-Muller pair on top of it.  Shared by vat.hip (miseg_normal_fill,
// miseg_philox_fill: the seed is a host argument) and uamt.hip (miseg_noise_add: the seed is read from device memory), so that both
// define the SAME stream: element j of the stream of `seed` is lane j & 3 of counter block j >> 2.
#pragma once
#include <hip/hip_runtime.h>

namespace miseg {

// ---- Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11)
struct Philox4 { unsigned v[4]; };
__device__ __forceinline__ Philox4 philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
    constexpr unsigned M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const unsigned hi0 = __umulhi(M0, c0), lo0 = M0 * c0, hi1 = __umulhi(M1, c2), lo1 = M1 * c2;
        const unsigned n0 = hi1 ^ c1 ^ k0, n1 = lo1, n2 = hi0 ^ c3 ^ k1, n3 = lo0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += W0; k1 += W1;
    }
    return Philox4{{c0, c1, c2, c3}};
}

// counter block b of the stream of `seed`
__device__ __forceinline__ Philox4 philox_block(unsigned long long seed, unsigned long long b) {
    return philox4x32_10((unsigned)b, (unsigned)(b >> 32), 0u, 0u, (unsigned)seed, (unsigned)(seed >> 32));
}

// the four standard normals of one counter block: two Box-Muller pairs, (0, 1] x [0, 1) from the words' top 24 bits
__device__ __forceinline__ void philox_normals(const Philox4& p, float* z) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const float u1 = (float)((p.v[2 * q] >> 8) + 1u) * 0x1p-24f, u2 = (float)(p.v[2 * q + 1] >> 8) * 0x1p-24f;
        const float rad = sqrtf(-2.f * logf(u1)), ang = 6.283185307179586f * u2;
        z[2 * q] = rad * cosf(ang);
        z[2 * q + 1] = rad * sinf(ang);
    }
}

}  // namespace miseg
