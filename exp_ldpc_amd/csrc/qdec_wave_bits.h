// qdec_wave_bits.h -- device helpers the samplers and the triage share: the
// Philox4x32-10 block function and the 64 x 64 bit transpose across a wave.
#ifndef QDEC_WAVE_BITS_H
#define QDEC_WAVE_BITS_H
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace qdec {

__device__ __forceinline__ void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c[0]);
        const uint32_t lo0 = 0xD2511F53u * c[0];
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c[2]);
        const uint32_t lo1 = 0xCD9E8D57u * c[2];
        const uint32_t n0 = hi1 ^ c[1] ^ k0;
        const uint32_t n2 = hi0 ^ c[3] ^ k1;
        c[0] = n0;
        c[1] = lo1;
        c[2] = n2;
        c[3] = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}

// 64 x 64 bit transpose across the wave: lane r holds row r (bit c = entry
// (r, c)), and gets back column r (bit c = entry (c, r)).  Six block-swap
// stages, each one exchange with lane ^ j: the off-diagonal j x j blocks of
// every 2j x 2j block trade places.
__device__ __forceinline__ uint64_t wave_transpose64(uint64_t v, int lane) {
    const uint64_t keep[6] = {0x00000000FFFFFFFFull, 0x0000FFFF0000FFFFull, 0x00FF00FF00FF00FFull,
                              0x0F0F0F0F0F0F0F0Full, 0x3333333333333333ull, 0x5555555555555555ull};
#pragma unroll
    for (int st = 0; st < 6; ++st) {
        const int j = 32 >> st;
        const uint64_t k0 = keep[st];  // columns c with (c & j) == 0
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, j);
        const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), j);
        const uint64_t w = ((uint64_t)hi << 32) | lo;
        v = (lane & j) ? ((v & ~k0) | ((w >> j) & k0)) : ((v & k0) | ((w & k0) << j));
    }
    return v;
}

}  // namespace qdec
#endif
