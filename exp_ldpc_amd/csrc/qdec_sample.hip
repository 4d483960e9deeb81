// qdec_sample.hip -- on-device sampler for the storage experiment.
//
// Restates what Stim samples from the reference's storage circuit
// (storage_sim.py:110-199) under depolarizing_noise(p, pm) (noise_model.py:117-123):
// DEPOLARIZE1(p) on every data qubit at the start of every timestep that contains
// a measurement, MRX(pm)/MZ(pm) record flips.  Only the X/Y part of DEPOLARIZE1
// (probability 2p/3) changes Z-basis records; the random X-stabilizer component
// of the readout is invisible to Hz and Lz and is not generated.  Per shot:
//   round t:  cum ^= Da(t); s_t = Hz cum ^ M_t; cum ^= Db(t); if t >= 1: cum ^= Dc(t)
//   (Dc = the DEPOLARIZE1 the rewriter places inside the REPEAT body before '}')
//   readout = cum ^ F   (R = 0: readout = D ^ F)
//   syn = [s_0, s_1^s_0, ..., Hz readout ^ s_{R-1}]   (spacetime_code.py:98-119)
// Bernoulli(p) bits are u32 < floor(p 2^32) from Philox4x32-10 with key
// (seed, stream_id) and counter (word, event, shot_lo, shot_hi); word w covers
// elements 4w..4w+3.  Event ids: R = 0: D=0, F=1; R >= 1: Da=4t, M=4t+1, Db=4t+2,
// Dc=4t+3, F=4R.  Identical to oracle/qdec_oracle.c qdo_sample_storage.
#include <hip/hip_runtime.h>

#include "qdec_internal.h"
#include "qdec_wave_bits.h"

namespace qdec {

// dst[e] ^= Bernoulli(thr) for e < count, event `ev`; lanes split the words.
__device__ __forceinline__ void bern_xor(uint8_t* dst, int count, uint32_t thr, uint32_t ev, int64_t shot,
                                         uint32_t k0, uint32_t k1, int lane) {
    if (thr == 0) return;
    const int words = (count + 3) / 4;
    for (int w = lane; w < words; w += 64) {
        uint32_t c[4] = {(uint32_t)w, ev, (uint32_t)shot, (uint32_t)((uint64_t)shot >> 32)};
        philox4x32_10(c, k0, k1);
#pragma unroll
        for (int l = 0; l < 4; ++l)
            if (4 * w + l < count) dst[4 * w + l] ^= (uint8_t)(c[l] < thr);
    }
}

__device__ __forceinline__ int row_parity(const DevGraph& g, const uint8_t* v, int i) {
    int p = 0;
    for (int e = g.row_ptr[i]; e < g.row_ptr[i + 1]; ++e) p ^= v[g.col_idx[e]];
    return p;
}

// OR a 64-bit ballot (bits of elements pos .. pos + 63) into a packed row held
// in LDS (one wave per block: lane 0 writes; the row has a spare word)
__device__ __forceinline__ void put_bits(uint64_t* w, int64_t pos, uint64_t mask, int lane) {
    if (lane == 0 && mask) {
        const int sh = (int)(pos & 63);
        w[pos >> 6] |= mask << sh;
        if (sh) w[(pos >> 6) + 1] |= mask >> (64 - sh);
    }
}

// PACKED: rows written as u64 words (bit j of word w = element 64 w + j; the
// layout of qd_sample_storage_packed_device), assembled in LDS by ballots.
template <bool PACKED>
__global__ __launch_bounds__(64) void sample_storage_kernel(DevGraph g, int rounds, uint32_t td, uint32_t tm,
                                                            uint32_t seed, uint32_t sid, int64_t shot0, int64_t B,
                                                            uint8_t* __restrict__ syn,
                                                            uint8_t* __restrict__ readout) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x;
    const int m = g.m, n = g.n;
    const int64_t syn_len = (int64_t)(rounds + 1) * m;
    const int sw_words = (int)((syn_len + 63) / 64), rw_words = (n + 63) / 64;
    uint64_t* synw = reinterpret_cast<uint64_t*>(smem);  // PACKED: [sw_words + 1], [rw_words + 1]
    uint64_t* rdw = synw + (PACKED ? sw_words + 1 : 0);
    uint8_t* cum = reinterpret_cast<uint8_t*>(rdw + (PACKED ? rw_words + 1 : 0));  // [n_pad]
    uint8_t* prev = cum + g.n_pad;    // [m_pad]
    uint8_t* cur = prev + g.m_pad;    // [m_pad]

    for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
        const int64_t shot = shot0 + b;
        for (int e = lane; e < g.n_pad; e += 64) cum[e] = 0;
        for (int e = lane; e < g.m_pad; e += 64) prev[e] = 0;
        if constexpr (PACKED) {
            for (int e = lane; e <= sw_words; e += 64) synw[e] = 0ull;
            for (int e = lane; e <= rw_words; e += 64) rdw[e] = 0ull;
        }
        __syncthreads();
        uint8_t* out = syn + b * syn_len;
        for (int t = 0; t < rounds; ++t) {
            bern_xor(cum, n, td, 4u * t + 0u, shot, seed, sid, lane);
            __syncthreads();
            for (int i = lane; i < m; i += 64) cur[i] = (uint8_t)row_parity(g, cum, i);
            __syncthreads();
            bern_xor(cur, m, tm, 4u * t + 1u, shot, seed, sid, lane);
            bern_xor(cum, n, td, 4u * t + 2u, shot, seed, sid, lane);
            __syncthreads();
            if (t >= 1) bern_xor(cum, n, td, 4u * t + 3u, shot, seed, sid, lane);
            if constexpr (PACKED) {
                for (int i0 = 0; i0 < m; i0 += 64) {
                    const int i = i0 + lane;
                    const bool bit = i < m && ((cur[i] ^ prev[i]) & 1);
                    if (i < m) prev[i] = cur[i];
                    put_bits(synw, (int64_t)t * m + i0, __ballot(bit), lane);
                }
            } else {
                for (int i = lane; i < m; i += 64) {
                    out[(int64_t)t * m + i] = cur[i] ^ prev[i];
                    prev[i] = cur[i];
                }
            }
            __syncthreads();
        }
        if (rounds == 0) {
            bern_xor(cum, n, td, 0u, shot, seed, sid, lane);
            __syncthreads();
        }
        bern_xor(cum, n, tm, rounds == 0 ? 1u : 4u * (uint32_t)rounds, shot, seed, sid, lane);
        __syncthreads();
        if constexpr (PACKED) {
            for (int j0 = 0; j0 < n; j0 += 64) {
                const int j = j0 + lane;
                put_bits(rdw, j0, __ballot(j < n && (cum[j] & 1)), lane);
            }
            for (int i0 = 0; i0 < m; i0 += 64) {
                const int i = i0 + lane;
                const bool bit = i < m && ((row_parity(g, cum, i) ^ prev[i]) & 1);
                put_bits(synw, (int64_t)rounds * m + i0, __ballot(bit), lane);
            }
            __syncthreads();
            uint64_t* so = reinterpret_cast<uint64_t*>(syn) + b * sw_words;
            uint64_t* ro = reinterpret_cast<uint64_t*>(readout) + b * rw_words;
            for (int e = lane; e < sw_words; e += 64) so[e] = synw[e];
            for (int e = lane; e < rw_words; e += 64) ro[e] = rdw[e];
        } else {
            for (int j = lane; j < n; j += 64) readout[b * n + j] = cum[j];
            for (int i = lane; i < m; i += 64) out[(int64_t)rounds * m + i] = (uint8_t)row_parity(g, cum, i) ^ prev[i];
        }
        __syncthreads();
    }
}

int launch_sample_storage(const DevGraph& g, int rounds, uint32_t thr_data, uint32_t thr_meas, uint32_t seed,
                          uint32_t stream_id, int64_t shot0, int64_t B, uint8_t* syn, uint8_t* readout,
                          int num_cus, hipStream_t stream, bool packed) {
    if (B <= 0) return 0;
    size_t lds = (size_t)g.n_pad + 2 * (size_t)g.m_pad;
    if (packed) lds += 8 * ((((int64_t)(rounds + 1) * g.m + 63) / 64 + 1) + ((int64_t)g.n + 63) / 64 + 1);
    const void* fn = packed ? reinterpret_cast<const void*>(sample_storage_kernel<true>)
                            : reinterpret_cast<const void*>(sample_storage_kernel<false>);
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    long long grid = (long long)num_cus * 16;
    if (grid > B) grid = B;
    if (packed)
        hipLaunchKernelGGL(sample_storage_kernel<true>, dim3((unsigned)grid), dim3(64), lds, stream, g, rounds,
                           thr_data, thr_meas, seed, stream_id, shot0, B, syn, readout);
    else
        hipLaunchKernelGGL(sample_storage_kernel<false>, dim3((unsigned)grid), dim3(64), lds, stream, g, rounds,
                           thr_data, thr_meas, seed, stream_id, shot0, B, syn, readout);
    return (int)hipGetLastError();
}

// ---------------------------------------------------------------- fault sampler
// B shots of a graph's own faults (qd_sample_faults_device): fault (column) j
// fires when lane j % 4 of the Philox block with counter (j / 4, 0, shot) is
// below smp_thr[j] -- bern_xor's convention with event 0 and a threshold per
// element.  One wave per shot.  Fired faults are few (about 8 of 2,800 on the
// R = 3 storage DEM at p = 0.003), so no check's row parity is computed: a lane
// that holds a fired fault sets its bit in an LDS bit image of e and walks the
// fault's column (smp_crow), toggling each detector in a bit image of H e by
// LDS atomics on 32-bit words (two lanes may hit one word).  The outputs are
// then written from the images.
struct SampleFaultsArgs {
    int m, n, k, lz_words;
    const int32_t* col_ptr;   // [n + 1]
    const int32_t* crow;      // [E]
    const uint32_t* thr;      // [(n + 3) / 4 * 4], pads 0
    const uint64_t* lz;       // [k][lz_words] or nullptr: then the CSR below
    const int32_t* lz_ptr;
    const int32_t* lz_idx;
    uint32_t seed, sid;
    int64_t shot0, B;
    void* det;
    void* faults;
    uint8_t* obs;
};

// words of a bit image of `bits` bits: whole u64 words (the packed row is copied
// as it is) plus a spare u64, so a 4-bit read at any bit offset may load the
// next u32 word unguarded
__host__ __device__ inline int image_words32(int bits) { return ((bits + 63) / 64 + 1) * 2; }

// Byte row dst[0 .. len) = the image's bits, written as aligned 4-byte stores
// (lane q: bytes head + 4 q ..) with single bytes at an unaligned head and tail.
__device__ __forceinline__ void expand_row(uint8_t* __restrict__ dst, int len, const uint32_t* img, int lane) {
    int head = (int)((4 - ((uintptr_t)dst & 3)) & 3);
    if (head > len) head = len;
    const int body = (len - head) / 4;
    auto bits4 = [&](int s) -> uint32_t {
        const uint64_t w = (uint64_t)img[s >> 5] | ((uint64_t)img[(s >> 5) + 1] << 32);
        return (uint32_t)(w >> (s & 31)) & 0xFu;
    };
    for (int q = lane; q < body; q += 64) {
        // bit i of the nibble -> byte i: 0x00204081 moves bit i to bit 8 i (i = 0..3)
        const uint32_t v = (bits4(head + 4 * q) * 0x00204081u) & 0x01010101u;
        *reinterpret_cast<uint32_t*>(dst + head + 4 * q) = v;
    }
    const int tail0 = head + 4 * body;
    if (lane < head) dst[lane] = (uint8_t)((img[lane >> 5] >> (lane & 31)) & 1u);
    if (lane < len - tail0) {
        const int i = tail0 + lane;
        dst[i] = (uint8_t)((img[i >> 5] >> (i & 31)) & 1u);
    }
}

template <bool PACKED>
__global__ __launch_bounds__(64) void sample_faults_kernel(SampleFaultsArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x;
    const int m = a.m, n = a.n;
    const int dw32 = image_words32(m), fw32 = image_words32(n);
    uint32_t* detw = reinterpret_cast<uint32_t*>(smem);  // [dw32] bit i = detector i
    uint32_t* fltw = detw + dw32;                        // [fw32] bit j = fault j
    const int words = (n + 3) / 4;
    const int dW = (m + 63) / 64, fW = (n + 63) / 64;

    for (int64_t b = blockIdx.x; b < a.B; b += gridDim.x) {
        const uint64_t shot = (uint64_t)(a.shot0 + b);
        for (int e = lane; e < dw32 + fw32; e += 64) detw[e] = 0u;
        __syncthreads();
        for (int w = lane; w < words; w += 64) {
            const uint4 t = *reinterpret_cast<const uint4*>(a.thr + 4 * w);
            uint32_t c[4] = {(uint32_t)w, 0u, (uint32_t)shot, (uint32_t)(shot >> 32)};
            philox4x32_10(c, a.seed, a.sid);
            uint32_t fired = (c[0] < t.x ? 1u : 0u) | (c[1] < t.y ? 2u : 0u) | (c[2] < t.z ? 4u : 0u) |
                             (c[3] < t.w ? 8u : 0u);
            if (fired) {
                atomicOr(&fltw[w >> 3], fired << (4 * (w & 7)));  // 8 lanes share a word
                do {
                    const int j = 4 * w + (__ffs(fired) - 1);
                    fired &= fired - 1;
                    const int t1 = a.col_ptr[j + 1];
                    for (int e = a.col_ptr[j]; e < t1; ++e) {
                        const int i = a.crow[e];
                        atomicXor(&detw[i >> 5], 1u << (i & 31));
                    }
                } while (fired);
            }
        }
        __syncthreads();
        if constexpr (PACKED) {
            const uint64_t* d64 = reinterpret_cast<const uint64_t*>(detw);
            const uint64_t* f64 = reinterpret_cast<const uint64_t*>(fltw);
            uint64_t* dout = static_cast<uint64_t*>(a.det) + b * dW;
            for (int e = lane; e < dW; e += 64) dout[e] = d64[e];
            if (a.faults) {
                uint64_t* fout = static_cast<uint64_t*>(a.faults) + b * fW;
                for (int e = lane; e < fW; e += 64) fout[e] = f64[e];
            }
        } else {
            expand_row(static_cast<uint8_t*>(a.det) + b * m, m, detw, lane);
            if (a.faults) expand_row(static_cast<uint8_t*>(a.faults) + b * n, n, fltw, lane);
        }
        if (a.obs) {  // F e: lanes split the logicals
            const uint64_t* f64 = reinterpret_cast<const uint64_t*>(fltw);
            for (int r = lane; r < a.k; r += 64) {
                uint32_t par = 0;
                if (a.lz) {
                    // a word of e without a fired fault (most of them) costs no load:
                    // the test is the same in every lane
                    for (int w = 0; w < a.lz_words; ++w) {
                        const uint64_t fw = f64[w];
                        if (fw) par ^= (uint32_t)__popcll(a.lz[(size_t)r * a.lz_words + w] & fw);
                    }
                } else {
                    for (int e = a.lz_ptr[r]; e < a.lz_ptr[r + 1]; ++e) {
                        const int q = a.lz_idx[e];
                        par ^= fltw[q >> 5] >> (q & 31);
                    }
                }
                a.obs[b * a.k + r] = (uint8_t)(par & 1u);
            }
        }
        __syncthreads();  // the images are zeroed for the next shot
    }
}

int launch_sample_faults(const DevGraph& g, const uint32_t* thr, const int32_t* crow, uint32_t seed,
                         uint32_t stream_id, int64_t shot0, int64_t B, bool packed, void* det, void* faults,
                         uint8_t* obs, int num_cus, hipStream_t stream) {
    if (B <= 0) return 0;
    SampleFaultsArgs a{};
    a.m = g.m, a.n = g.n, a.k = g.k, a.lz_words = g.lz_words;
    a.col_ptr = g.col_ptr, a.crow = crow, a.thr = thr;
    a.lz = g.lz, a.lz_ptr = g.lz_ptr, a.lz_idx = g.lz_idx;
    a.seed = seed, a.sid = stream_id, a.shot0 = shot0, a.B = B;
    a.det = det, a.faults = faults, a.obs = obs;
    const size_t lds = 4 * ((size_t)image_words32(g.m) + (size_t)image_words32(g.n));
    const void* fn = packed ? reinterpret_cast<const void*>(sample_faults_kernel<true>)
                            : reinterpret_cast<const void*>(sample_faults_kernel<false>);
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    long long grid = (long long)num_cus * 32;  // one wave per block: the 8 waves per SIMD the hardware holds
    if (grid > B) grid = B;
    if (packed)
        hipLaunchKernelGGL(sample_faults_kernel<true>, dim3((unsigned)grid), dim3(64), lds, stream, a);
    else
        hipLaunchKernelGGL(sample_faults_kernel<false>, dim3((unsigned)grid), dim3(64), lds, stream, a);
    return (int)hipGetLastError();
}

}  // namespace qdec
