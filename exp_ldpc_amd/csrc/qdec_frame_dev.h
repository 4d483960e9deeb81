// qdec_frame_dev.h -- device helpers shared by the two placements of the Pauli
// frame: the LDS kernels (qdec_frame.hip) and the HBM kernels (qdec_frame_hbm.hip).
// The draw convention is in the header of qdec_frame.hip and DESIGN §3.4c.
#ifndef QDEC_FRAME_DEV_H
#define QDEC_FRAME_DEV_H
#include <hip/hip_runtime.h>

#include "qdec_internal.h"
#include "qdec_wave_bits.h"

namespace qdec {

struct FrameOuts {
    void* p[kFrameGroups];
};

// floor(c u / T) for u < T, c <= 15, exactly: the largest k with k T <= c u
__device__ __forceinline__ uint32_t scaled_index(uint32_t u, uint32_t T, uint32_t c) {
    const uint64_t n = (uint64_t)u * c;
    uint32_t k = 0;
#pragma unroll
    for (uint32_t bit = 8; bit; bit >>= 1)
        if ((uint64_t)(k + bit) * T <= n) k += bit;
    return k;
}

// The 64 randomisation bits of site `rsite` for shots s0 .. s0 + 63 (s0 need
// not be a multiple of 32: the word is cut from up to three u32 chunks of at
// most two Philox blocks).
__device__ __forceinline__ uint64_t rand_word(uint32_t rsite, uint64_t s0, uint32_t k0, uint32_t k1) {
    const uint64_t c0 = s0 >> 5;  // first 32-shot chunk
    const int off = (int)(s0 & 31), l0 = (int)(c0 & 3);
    const uint64_t blk = c0 >> 2;
    uint32_t a[4] = {rsite, 1u, (uint32_t)blk, (uint32_t)(blk >> 32)};
    philox4x32_10(a, k0, k1);
    uint32_t b[4] = {0u, 0u, 0u, 0u};
    if (l0 >= 2) {  // chunks c0 + 1 or c0 + 2 lie in the next block (the same test in every lane)
        b[0] = rsite, b[1] = 1u, b[2] = (uint32_t)(blk + 1), b[3] = (uint32_t)((blk + 1) >> 32);
        philox4x32_10(b, k0, k1);
    }
    // chunk l0 + k of (a, b), by selects (a switch over the arrays indexes them dynamically: scratch)
    const uint32_t a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3], b0 = b[0], b1 = b[1];
    const uint32_t w0 = l0 == 0 ? a0 : l0 == 1 ? a1 : l0 == 2 ? a2 : a3;
    const uint32_t w1 = l0 == 0 ? a1 : l0 == 1 ? a2 : l0 == 2 ? a3 : b0;
    const uint32_t w2 = l0 == 0 ? a2 : l0 == 1 ? a3 : l0 == 2 ? b0 : b1;
    const uint64_t lo = (uint64_t)w0 | ((uint64_t)w1 << 32);
    return off ? (lo >> off) | ((uint64_t)w2 << (64 - off)) : lo;
}

// x / z bit of Pauli code P (0 = I, 1 = X, 2 = Y, 3 = Z)
__device__ __forceinline__ bool pauli_x(uint32_t P) { return P == 1u || P == 2u; }
__device__ __forceinline__ bool pauli_z(uint32_t P) { return P >= 2u; }

// The gate rules on the frame words (one word = 64 shots, or 64 faults)
__device__ __forceinline__ void frame_h(uint64_t* x, uint64_t* z, int q) {
    const uint64_t t = x[q];
    x[q] = z[q];
    z[q] = t;
}
__device__ __forceinline__ void frame_cx(uint64_t* x, uint64_t* z, int a, int b) {
    x[b] ^= x[a];
    z[a] ^= z[b];
}
__device__ __forceinline__ void frame_cz(uint64_t* x, uint64_t* z, int a, int b) {
    z[a] ^= x[b];
    z[b] ^= x[a];
}

// The output stage: row r of a group = the parity of its records, a word of the
// wave's 64 shots (faults); `valid` of them, the first being row b0 of the output.
template <bool PACKED>
__device__ __forceinline__ void frame_write_outputs(const DevCircuit& c, const uint64_t* rec, const FrameOuts& o,
                                                    int64_t b0, int valid, int lane) {
#pragma unroll
    for (int g = 0; g < kFrameGroups; ++g) {
        void* const og = o.p[g];
        if (!og) continue;
        const int rows = c.rows[g];
        const int32_t* rp = c.row_ptr + c.row_off[g];
        const int words = (rows + 63) / 64;
        for (int j = 0; j < words; ++j) {
            const int row = 64 * j + lane;
            uint64_t v = 0ull;  // rows past the end: the padding bits of a packed row, written 0
            if (row < rows)
                for (int e = rp[row]; e < rp[row + 1]; ++e) v ^= rec[c.rec_idx[e]];
            if constexpr (PACKED) {
                const uint64_t mine = wave_transpose64(v, lane);  // lane s: shot s's word j
                if (lane < valid) static_cast<uint64_t*>(og)[(b0 + lane) * words + j] = mine;
            } else {
                uint8_t* out = static_cast<uint8_t*>(og) + b0 * rows + row;
                if (row < rows)
                    for (int s = 0; s < valid; ++s) out[(int64_t)s * rows] = (uint8_t)((v >> s) & 1ull);
            }
        }
    }
}

}  // namespace qdec
#endif
