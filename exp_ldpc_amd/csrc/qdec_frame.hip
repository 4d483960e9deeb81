// qdec_frame.hip -- Pauli-frame sampler of a compiled circuit (qd_circuit_sample_device)
// and its deterministic twin, the propagation of the circuit's elementary faults
// (qd_circuit_faults_device; frame_fault_kernel below).
//
// Stim's frame simulation of the gate set the storage experiment uses (H, CX, CZ,
// resets and measurements in Z and X, X/Y/Z_ERROR, DEPOLARIZE1/2, PAULI_CHANNEL_1/2),
// bit-sliced:
// one wave runs 64 consecutive shots, and x[Q], z[Q] (the frame) and rec[M] (the
// measurement record) are 64-bit words whose bit s is shot s of the wave.
// The record is the flip against the noiseless reference sample; a measurement
// target may carry an invert bit (kFrameInvert) for a reference sample of 1.
//
// Gates, resets and measurements: lanes split the targets of one instruction,
// which the host compiler has made pairwise disjoint (validated at create), a
// word operation each.  Noise sites: lane = shot; every lane draws its own u32
// and a ballot makes the word (skipped when no lane fired).  One workgroup is one
// wave, so the barrier between instructions only orders the wave's own traffic.
//
// Both kernels are templates over where the words live (DESIGN §3.4c "Frame
// placement"); the mapping, the frame rules, every draw and so every output bit
// are the same:
//   FrameInLds  the launch's dynamic LDS (16 Q + 8 M bytes, up to 160 KiB).  Lane 0
//               XORs a site's ballot words into the frame at once.
//   FrameInHbm  workgroup b owns slot b of the launch's scratch, x[Q] z[Q] rec[M];
//               it walks its 64-shot words grid-stride and re-zeroes the slot
//               between them.  No other workgroup touches the slot, so the barrier
//               between instructions (a fence at workgroup scope) orders all
//               traffic to it.  Lane 0 applying one site after the other would be
//               a chain of dependent memory round trips.  Instead the ballot words
//               of up to 64 consecutive sites are built so that lane l keeps site
//               e0 + l's words, and one exec-masked read-modify-write applies
//               them: lanes whose words are 0 do nothing (at low p most are), the
//               others name distinct frame words.  An instruction that names a
//               qubit twice (FrameOpRec::dup, set by build_circuit) applies its
//               fired sites one lane at a time in site order instead, a barrier
//               after each: plain loads and stores, no atomics (an atomic executes
//               at the memory side and drops the line from the XCD's L2).
//
// Draws, key (seed, stream_id):
//   Bernoulli / Pauli site s of global shot g: u = lane s % 4 of the
//     Philox4x32-10 block with counter (s / 4, 0, g_lo, g_hi); fires when u < T.
//     DEPOLARIZE1: Pauli 1 + floor(3 u / T) (1 = X, 2 = Y, 3 = Z); DEPOLARIZE2:
//     code 1 + floor(15 u / T), first qubit's Pauli = code >> 2, second's =
//     code & 3 (0 = I).  PAULI_CHANNEL_1 / 2, cumulative thresholds C_0 <= .. <=
//     C_{K-1} = T (K = 3 / 15): Pauli / code 1 + #{j : C_j <= u}, so an outcome of
//     probability 0 is never drawn.  Every instruction's first site is a multiple of 4.
//   Randomisation site r of shot g: bit g % 32 of lane (g / 32) % 4 of the block
//     with counter (r, 1, (g / 128)_lo, (g / 128)_hi).
// so a shot's bits depend on (seed, stream_id, site, global shot) only.
#include <hip/hip_runtime.h>

#include "qdec_internal.h"
#include "qdec_wave_bits.h"

namespace qdec {

namespace {

struct FrameOuts {
    void* p[kFrameGroups];
};

// The placements: where x starts, the targets a lane keeps in flight in one gate
// or measurement step, whether a lane keeps the ballot words of its own noise
// site, and how a fault is injected.
struct FrameInLds {
    static constexpr int kUnroll = 1;
    static constexpr bool kKeepSites = false;
    __device__ uint64_t* frame() const {
        extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
        return reinterpret_cast<uint64_t*>(smem);
    }
    // two lanes may name one word: an LDS atomic
    __device__ static void inject(uint64_t* word, unsigned long long bit, bool) {
        atomicXor(reinterpret_cast<unsigned long long*>(word), bit);
    }
};
struct FrameInHbm {
    static constexpr int kUnroll = 4;
    static constexpr bool kKeepSites = true;
    uint64_t* scratch;
    int64_t slot_words;
    __device__ uint64_t* frame() const { return scratch + (int64_t)blockIdx.x * slot_words; }
    // the lanes of one instruction name distinct words unless it names a qubit twice
    __device__ static void inject(uint64_t* word, unsigned long long bit, bool dup) {
        if (dup)
            atomicXor(reinterpret_cast<unsigned long long*>(word), bit);
        else
            *word ^= bit;
    }
};

// the arguments of the two jobs
struct SampleJob {
    uint32_t seed, sid;
    int64_t shot0, B;
};
struct FaultJob {
    int32_t kind, f0, F;
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

// The lanes split n targets (pairs), U of them per lane and step: load(r, e)
// reads target e into the registers r (a Regs) of the lane, store(r, e) writes it
// back.  All U loads are issued before the first store, so with the frame in
// memory their round trips overlap instead of queueing behind possible aliases.
// The registers belong to one step (declared outside it they would stay live
// from step to step: 6 more VGPRs in the fault kernel in HBM).
template <int U, class Regs, class Load, class Store>
__device__ __forceinline__ void for_targets(int n, int lane, Load&& load, Store&& store) {
    for (int e = lane; e < n; e += 64 * U) {
        Regs r[U];
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (e + 64 * u < n) load(r[u], e + 64 * u);
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (e + 64 * u < n) store(r[u], e + 64 * u);
    }
}

// The gate rules on the frame words (one word = 64 shots, or 64 faults).
// H: swap x and z of every target
template <int U>
__device__ __forceinline__ void frame_h(uint64_t* x, uint64_t* z, const int32_t* tg, int T, int lane) {
    struct Regs {
        int q;
        uint64_t x, z;
    };
    for_targets<U, Regs>(
        T, lane, [&](Regs& r, int e) { r.q = tg[e], r.x = x[r.q], r.z = z[r.q]; },
        [&](const Regs& r, int) { x[r.q] = r.z, z[r.q] = r.x; });
}

// CX (CZ = false): x_b ^= x_a, z_a ^= z_b; CZ: z_a ^= x_b, z_b ^= x_a; P pairs
template <int U, bool CZ>
__device__ __forceinline__ void frame_pairs(uint64_t* x, uint64_t* z, const int32_t* tg, int P, int lane) {
    struct Regs {
        int a, b;
        uint64_t xa, xb, za, zb;
    };
    for_targets<U, Regs>(
        P, lane,
        [&](Regs& r, int p) {
            r.a = tg[2 * p], r.b = tg[2 * p + 1];
            r.xa = x[r.a], r.xb = x[r.b], r.za = z[r.a], r.zb = z[r.b];
        },
        [&](const Regs& r, int) {
            if constexpr (CZ) {
                z[r.a] = r.za ^ r.xb;
                z[r.b] = r.zb ^ r.xa;
            } else {
                x[r.b] = r.xb ^ r.xa;
                z[r.a] = r.za ^ r.zb;
            }
        });
}

// What a noise site draws: a Bernoulli bit for a record (noisy M / MX) or for the
// Pauli of X/Y/Z_ERROR, or the Pauli(s) of DEPOLARIZE1 / 2 (equal shares of the
// threshold) or of PAULI_CHANNEL_1 / 2 (cumulative thresholds).
enum SiteKind { SK_REC, SK_PAULI, SK_DEP1, SK_DEP2, SK_PC1, SK_PC2 };
constexpr bool site_pair(int kind) { return kind == SK_DEP2 || kind == SK_PC2; }

// thresholds of a channel instruction a lane compares against: all but the last,
// which is the instruction's thr (a fired lane has u below it)
constexpr int site_thresholds(int kind) { return kind == SK_PC1 ? 2 : kind == SK_PC2 ? 14 : 0; }

// 1 + the number of j < N with C[j] <= u: a compare and an add per entry
template <int N>
__device__ __forceinline__ uint32_t cumulative_index(uint32_t u, const uint32_t* C) {
    uint32_t k = 1u;
#pragma unroll
    for (int j = 0; j < N; ++j) k += C[j] <= u ? 1u : 0u;
    return k;
}

// The ballot words of one site from its u32, given f = the ballot of `fired`
// (not 0): w = x, z of the (first) target and, on a pair, x, z of the second.
// C: the instruction's cumulative thresholds but the last (PAULI_CHANNEL_1 / 2 only).
template <int KIND>
__device__ __forceinline__ void site_words(int op, uint32_t u, uint32_t thr, const uint32_t* C, bool fired,
                                           uint64_t f, uint64_t (&w)[4]) {
    w[2] = w[3] = 0ull;
    if constexpr (KIND != SK_REC && KIND != SK_PAULI) {
        uint32_t code;
        if constexpr (KIND == SK_PC1 || KIND == SK_PC2)
            code = fired ? cumulative_index<site_thresholds(KIND)>(u, C) : 0u;
        else
            code = fired ? 1u + scaled_index(u, thr, KIND == SK_DEP1 ? 3u : 15u) : 0u;
        const uint32_t Pa = site_pair(KIND) ? code >> 2 : code;
        w[0] = __ballot(pauli_x(Pa)), w[1] = __ballot(pauli_z(Pa));
        if constexpr (site_pair(KIND)) w[2] = __ballot(pauli_x(code & 3u)), w[3] = __ballot(pauli_z(code & 3u));
    } else {
        w[0] = KIND == SK_REC || op != FO_ZERR ? f : 0ull;
        w[1] = KIND == SK_PAULI && op != FO_XERR ? f : 0ull;
    }
}

// Apply a batch of kept noise sites: `any` = this lane's site fired.  Distinct
// words (dup == false): every lane at once.  Otherwise one lane after the other in
// site order, each behind a barrier, so a word two sites name sees both XORs.
template <class Apply>
__device__ __forceinline__ void apply_sites(bool dup, bool any, int lane, Apply&& apply) {
    if (!dup) {
        if (any) apply();
        return;
    }
    uint64_t todo = __ballot(any);
    while (todo) {  // the same word in every lane
        const int l = __ffsll((unsigned long long)todo) - 1;
        todo &= todo - 1;
        if (lane == l) apply();
        __syncthreads();
    }
}

// The n noise sites of instruction r: the sampler's draws of the header, the
// words to the record (SK_REC: the records of one instruction are distinct words,
// and r.dup is 0) or to the frame of the site's target (pair).
template <class Place, int KIND>
__device__ __forceinline__ void frame_noise(const FrameOpRec& r, const int32_t* tg, int n, uint64_t* x, uint64_t* z,
                                            uint64_t* rec, int lane, uint32_t g_lo, uint32_t g_hi,
                                            const SampleJob& j, const uint32_t* cum = nullptr) {
    constexpr int kBatch = Place::kKeepSites ? 64 : 4;  // sites between two applications; 4 = one Philox block
    // The channel's thresholds, the same in every lane, are loaded once, here: the loads are in flight during
    // the first Philox block.  Loaded where a fired site needs them they cost a memory round trip per fired site
    // (+ 13 % to + 23 % at p = 0.01).
    constexpr int NC = site_thresholds(KIND);
    uint32_t C[NC ? NC : 1] = {0u};
#pragma unroll
    for (int k = 0; k < NC; ++k) C[k] = cum[k];
    auto apply = [&](int site, const uint64_t(&w)[4]) {
        if constexpr (KIND == SK_REC) {
            rec[r.rec0 + site] ^= w[0];
        } else {
            const int a = tg[site_pair(KIND) ? 2 * site : site];
            if (w[0]) x[a] ^= w[0];
            if (w[1]) z[a] ^= w[1];
            if constexpr (site_pair(KIND)) {
                const int b = tg[2 * site + 1];
                if (w[2]) x[b] ^= w[2];
                if (w[3]) z[b] ^= w[3];
            }
        }
    };
    for (int e0 = 0; e0 < n; e0 += kBatch) {
        uint64_t keep[4] = {0ull, 0ull, 0ull, 0ull};  // the words of site e0 + lane
        const int nb = n - e0 < kBatch ? n - e0 : kBatch;  // sites of this batch
        for (int k = 0; 4 * k < nb; ++k) {
            uint32_t u[4] = {r.site0 / 4u + (uint32_t)((e0 >> 2) + k), 0u, g_lo, g_hi};
            philox4x32_10(u, j.seed, j.sid);
#pragma unroll
            for (int l = 0; l < 4; ++l) {
                const bool fired = u[l] < r.thr;
                const uint64_t f = 4 * k + l < nb ? __ballot(fired) : 0ull;
                // some shot fired (the same test in every lane).  One nested `if`, no break or continue:
                // with those the compiler threads the loop through a per-lane state variable, + 40 % time
                if (f) {
                    uint64_t w[4];
                    site_words<KIND>(r.op, u[l], r.thr, C, fired, f, w);
                    if constexpr (Place::kKeepSites) {
                        if (lane == 4 * k + l) keep[0] = w[0], keep[1] = w[1], keep[2] = w[2], keep[3] = w[3];
                    } else if (lane == 0) {
                        apply(e0 + 4 * k + l, w);
                    }
                }
            }
        }
        if constexpr (Place::kKeepSites)
            apply_sites(r.dup != 0, (keep[0] | keep[1] | keep[2] | keep[3]) != 0ull, lane,
                        [&] { apply(e0 + lane, keep); });
    }
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

}  // namespace

template <class Place, bool PACKED>
__global__ __launch_bounds__(64) void frame_sample_kernel(DevCircuit c, Place place, SampleJob j, FrameOuts o) {
    constexpr int U = Place::kUnroll;
    const int lane = threadIdx.x;
    uint64_t* x = place.frame();  // [Q]
    uint64_t* z = x + c.Q;        // [Q]
    uint64_t* rec = z + c.Q;      // [M]: every word is written by its measurement
    const int64_t waves = (j.B + 63) / 64;

    for (int64_t w = blockIdx.x; w < waves; w += gridDim.x) {
        const int64_t b0 = w * 64;
        const int valid = (int)(j.B - b0 < 64 ? j.B - b0 : 64);
        const uint64_t s0 = (uint64_t)(j.shot0 + b0);
        const uint64_t shot = s0 + (uint64_t)lane;
        const uint32_t g_lo = (uint32_t)shot, g_hi = (uint32_t)(shot >> 32);
        for (int q = lane; q < 2 * c.Q; q += 64) x[q] = 0ull;
        __syncthreads();

        for (int i = 0; i < c.n_ops; ++i) {
            const FrameOpRec r = c.ops[i];
            const int32_t* tg = c.targets + r.tgt_off;
            const int T = r.tgt_cnt;
            switch (r.op) {
                case FO_H:
                    frame_h<U>(x, z, tg, T, lane);
                    break;
                case FO_CX:
                    frame_pairs<U, false>(x, z, tg, T / 2, lane);
                    break;
                case FO_CZ:
                    frame_pairs<U, true>(x, z, tg, T / 2, lane);
                    break;
                case FO_R:
                case FO_RX: {
                    uint64_t* keep = r.op == FO_R ? z : x;  // the component a reset leaves random
                    uint64_t* clr = r.op == FO_R ? x : z;
                    for (int e = lane; e < T; e += 64) {
                        const int q = tg[e];
                        clr[q] = 0ull;
                        keep[q] = rand_word(r.rsite0 + (uint32_t)e, s0, j.seed, j.sid);
                    }
                    break;
                }
                case FO_M:
                case FO_MX: {
                    uint64_t* read = r.op == FO_M ? x : z;
                    uint64_t* kick = r.op == FO_M ? z : x;
                    struct Regs {
                        int t;
                        uint64_t read, kick;
                    };
                    for_targets<U, Regs>(
                        T, lane,
                        [&](Regs& v, int e) {
                            v.t = tg[e];
                            v.read = read[v.t & kFrameQubitMask], v.kick = kick[v.t & kFrameQubitMask];
                        },
                        [&](const Regs& v, int e) {
                            rec[r.rec0 + e] = (v.t & kFrameInvert) ? ~v.read : v.read;
                            kick[v.t & kFrameQubitMask] = v.kick ^ rand_word(r.rsite0 + (uint32_t)e, s0, j.seed, j.sid);
                        });
                    if (r.thr) {
                        __syncthreads();
                        frame_noise<Place, SK_REC>(r, tg, T, x, z, rec, lane, g_lo, g_hi, j);
                    }
                    break;
                }
                case FO_XERR:
                case FO_YERR:
                case FO_ZERR:
                    if (r.thr) frame_noise<Place, SK_PAULI>(r, tg, T, x, z, rec, lane, g_lo, g_hi, j);
                    break;
                case FO_DEP1:
                    if (r.thr) frame_noise<Place, SK_DEP1>(r, tg, T, x, z, rec, lane, g_lo, g_hi, j);
                    break;
                case FO_DEP2:
                    if (r.thr) frame_noise<Place, SK_DEP2>(r, tg, T / 2, x, z, rec, lane, g_lo, g_hi, j);
                    break;
                case FO_PC1:
                    if (r.thr) frame_noise<Place, SK_PC1>(r, tg, T, x, z, rec, lane, g_lo, g_hi, j, c.cum + r.cum_off);
                    break;
                case FO_PC2:
                    if (r.thr)
                        frame_noise<Place, SK_PC2>(r, tg, T / 2, x, z, rec, lane, g_lo, g_hi, j, c.cum + r.cum_off);
                    break;
                default:
                    break;
            }
            __syncthreads();
        }

        frame_write_outputs<PACKED>(c, rec, o, b0, valid, lane);
        __syncthreads();  // the frame is zeroed for the next 64 shots
    }
}

// Fault propagation (qd_circuit_faults_device): the sampler's deterministic twin.
// Bit s of a word is fault f0 + 64 w + s of wave w instead of a shot, nothing is
// drawn, and the record is the flip the fault causes: a reset clears both
// components, a measurement copies the measured one (invert bits do not apply to
// a flip) and kicks nothing.  At instruction i the lanes whose fault belongs to i
// XOR their own bit into the word the fault names, after the instruction's own
// work (a record flip follows the measurement, a gauge fault the reset).  Two
// lanes may name one word (X_ERROR 0 1 0, a qubit in two DEPOLARIZE2 / PAULI_CHANNEL_2 pairs, two
// gauge faults never): Place::inject.  Before a wave's first fault the frame is
// all zero and stays so, so the wave starts at that fault's instruction, found by
// bisection over the instructions' first-fault indices (non-decreasing; the last
// instruction whose index is <= the fault holds it); rec is zeroed up front
// because the skipped measurements do not write their words.
template <class Place, bool PACKED>
__global__ __launch_bounds__(64) void frame_fault_kernel(DevCircuit c, Place place, FaultJob j, FrameOuts o) {
    constexpr int U = Place::kUnroll;
    const int lane = threadIdx.x;
    uint64_t* x = place.frame();  // [Q]
    uint64_t* z = x + c.Q;        // [Q]
    uint64_t* rec = z + c.Q;      // [M]
    const int kind = j.kind;
    const int waves = (j.F + 63) / 64;
    const unsigned long long bit = 1ull << lane;

    for (int w = blockIdx.x; w < waves; w += gridDim.x) {
        const int b0 = w * 64;
        const int valid = j.F - b0 < 64 ? j.F - b0 : 64;
        const int32_t first = j.f0 + b0;  // the wave's first fault
        const int32_t mine = lane < valid ? first + lane : -1;
        for (int q = lane; q < 2 * c.Q + c.M; q += 64) x[q] = 0ull;  // x, z and rec are one range
        int lo = 0, hi = c.n_ops - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            const int32_t base = kind ? (int32_t)c.ops[mid].rsite0 : c.ops[mid].fault0;
            if (base <= first) lo = mid; else hi = mid - 1;
        }
        __syncthreads();

        for (int i = lo; i < c.n_ops; ++i) {
            const FrameOpRec r = c.ops[i];
            const int32_t* tg = c.targets + r.tgt_off;
            const int T = r.tgt_cnt;
            bool wrote = true;  // the instruction's own work wrote words an injection may name
            switch (r.op) {
                case FO_H:
                    frame_h<U>(x, z, tg, T, lane);
                    break;
                case FO_CX:
                    frame_pairs<U, false>(x, z, tg, T / 2, lane);
                    break;
                case FO_CZ:
                    frame_pairs<U, true>(x, z, tg, T / 2, lane);
                    break;
                case FO_R:
                case FO_RX:
                    for (int e = lane; e < T; e += 64) x[tg[e]] = z[tg[e]] = 0ull;
                    break;
                case FO_M:
                case FO_MX: {
                    const uint64_t* read = r.op == FO_M ? x : z;
                    for_targets<U, uint64_t>(
                        T, lane, [&](uint64_t& v, int e) { v = read[tg[e] & kFrameQubitMask]; },
                        [&](uint64_t v, int e) { rec[r.rec0 + e] = v; });
                    break;
                }
                default:
                    wrote = false;
                    break;
            }
            const int32_t base = kind ? (int32_t)r.rsite0 : r.fault0;
            const int32_t cnt = fault_count(r.op, T, kind);
            if (base < first + valid && base + cnt > first) {  // some lane's fault is here (the same test in every lane)
                if (wrote) __syncthreads();
                const int32_t f = mine - base;
                if (mine >= 0 && f >= 0 && f < cnt) {
                    const int32_t comp = fault_comp(r.op, f, kind), e = fault_target(r.op, f, kind);
                    if (comp == FC_REC) {
                        Place::inject(rec + r.rec0 + e, bit, r.dup != 0);
                    } else {
                        const int q = tg[e] & kFrameQubitMask;
                        if (comp & FC_X) Place::inject(x + q, bit, r.dup != 0);
                        if (comp & FC_Z) Place::inject(z + q, bit, r.dup != 0);
                    }
                }
            }
            __syncthreads();
        }

        frame_write_outputs<PACKED>(c, rec, o, (int64_t)b0, valid, lane);
        __syncthreads();  // the frame is zeroed for the next 64 faults
    }
}

namespace {

// One launch of a kernel pair's instantiation for (placement, packed), `waves`
// 64-shot (64-fault) words: fn[placement][packed] takes (c, the placement, job, outs).
template <class Job>
int launch_frame(const void* const (&fn)[2][2], const DevCircuit& c, const FramePlace& at, int64_t waves,
                 bool packed, void* const outs[kFrameGroups], Job job, hipStream_t stream) {
    FrameOuts o;
    for (int g = 0; g < kFrameGroups; ++g) o.p[g] = outs[g];
    const bool hbm = at.placement == FP_HBM;
    const void* k = fn[hbm][packed];
    FrameInLds in_lds;
    FrameInHbm in_hbm{static_cast<uint64_t*>(at.scratch), (int64_t)(at.slot_bytes / 8)};
    size_t lds = 0;
    int64_t grid;
    if (hbm) {
        if (!at.scratch || at.slots < 1) return (int)hipErrorInvalidValue;
        grid = at.slots;  // a resident workgroup per slot
    } else {
        lds = at.lds < 16 ? 16 : at.lds;
        if (lds > 64 * 1024) {
            const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return (int)e;
        }
        grid = (int64_t)at.num_cus * 32;  // one wave per block; LDS decides how many a CU holds
    }
    if (grid > waves) grid = waves;
    void* args[] = {const_cast<DevCircuit*>(&c), hbm ? (void*)&in_hbm : (void*)&in_lds, &job, &o};
    (void)hipLaunchKernel(k, dim3((unsigned)grid), dim3(64), args, lds, stream);
    return (int)hipGetLastError();  // also clears it, as after every other launch of the library
}

}  // namespace

int launch_frame_sample(const DevCircuit& c, const FramePlace& at, uint32_t seed, uint32_t stream_id, int64_t shot0,
                        int64_t B, bool packed, void* const outs[kFrameGroups], hipStream_t stream) {
    if (B <= 0) return 0;
    static const void* const fn[2][2] = {
        {(const void*)frame_sample_kernel<FrameInLds, false>, (const void*)frame_sample_kernel<FrameInLds, true>},
        {(const void*)frame_sample_kernel<FrameInHbm, false>, (const void*)frame_sample_kernel<FrameInHbm, true>}};
    return launch_frame(fn, c, at, (B + 63) / 64, packed, outs, SampleJob{seed, stream_id, shot0, B}, stream);
}

int launch_frame_faults(const DevCircuit& c, const FramePlace& at, int kind, int32_t f0, int32_t F, bool packed,
                        void* const outs[kFrameGroups], hipStream_t stream) {
    if (F <= 0) return 0;
    static const void* const fn[2][2] = {
        {(const void*)frame_fault_kernel<FrameInLds, false>, (const void*)frame_fault_kernel<FrameInLds, true>},
        {(const void*)frame_fault_kernel<FrameInHbm, false>, (const void*)frame_fault_kernel<FrameInHbm, true>}};
    return launch_frame(fn, c, at, ((int64_t)F + 63) / 64, packed, outs, FaultJob{kind, f0, F}, stream);
}

}  // namespace qdec
