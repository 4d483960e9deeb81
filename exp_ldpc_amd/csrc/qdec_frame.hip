// qdec_frame.hip -- Pauli-frame sampler of a compiled circuit (qd_circuit_sample_device)
// and its deterministic twin, the propagation of the circuit's elementary faults
// (qd_circuit_faults_device; frame_fault_kernel below).
//
// Stim's frame simulation of the gate set the storage experiment uses (H, CX, CZ,
// resets and measurements in Z and X, X/Y/Z_ERROR, DEPOLARIZE1/2), bit-sliced:
// one wave runs 64 consecutive shots, and x[Q], z[Q] (the frame) and rec[M] (the
// measurement record) are 64-bit words in LDS whose bit s is shot s of the wave.
// The record is the flip against the noiseless reference sample; a measurement
// target may carry an invert bit (kFrameInvert) for a reference sample of 1.
//
// Gates, resets and measurements: lanes split the targets of one instruction,
// which the host compiler has made pairwise disjoint (validated at create), a
// word operation each.  Noise sites: lane = shot; every lane draws its own u32,
// a ballot makes the word, lane 0 XORs it into the frame (skipped when no lane
// fired).  One workgroup is one wave, so the barrier between instructions only
// orders the wave's own LDS traffic.
//
// Draws, key (seed, stream_id):
//   Bernoulli / Pauli site s of global shot g: u = lane s % 4 of the
//     Philox4x32-10 block with counter (s / 4, 0, g_lo, g_hi); fires when u < T.
//     DEPOLARIZE1: Pauli 1 + floor(3 u / T) (1 = X, 2 = Y, 3 = Z); DEPOLARIZE2:
//     code 1 + floor(15 u / T), first qubit's Pauli = code >> 2, second's =
//     code & 3 (0 = I).  Every instruction's first site is a multiple of 4.
//   Randomisation site r of shot g: bit g % 32 of lane (g / 32) % 4 of the block
//     with counter (r, 1, (g / 128)_lo, (g / 128)_hi).
// so a shot's bits depend on (seed, stream_id, site, global shot) only.
#include "qdec_frame_dev.h"

namespace qdec {

template <bool PACKED>
__global__ __launch_bounds__(64) void frame_sample_kernel(DevCircuit c, uint32_t seed, uint32_t sid, int64_t shot0,
                                                          int64_t B, FrameOuts o) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x;
    uint64_t* x = reinterpret_cast<uint64_t*>(smem);  // [Q]
    uint64_t* z = x + c.Q;                            // [Q]
    uint64_t* rec = z + c.Q;                          // [M]: every word is written by its measurement
    const int64_t waves = (B + 63) / 64;

    for (int64_t w = blockIdx.x; w < waves; w += gridDim.x) {
        const int64_t b0 = w * 64;
        const int valid = (int)(B - b0 < 64 ? B - b0 : 64);
        const uint64_t s0 = (uint64_t)(shot0 + b0);
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
                    for (int e = lane; e < T; e += 64) frame_h(x, z, tg[e]);
                    break;
                case FO_CX:
                    for (int e = lane; 2 * e < T; e += 64) frame_cx(x, z, tg[2 * e], tg[2 * e + 1]);
                    break;
                case FO_CZ:
                    for (int e = lane; 2 * e < T; e += 64) frame_cz(x, z, tg[2 * e], tg[2 * e + 1]);
                    break;
                case FO_R:
                case FO_RX: {
                    uint64_t* keep = r.op == FO_R ? z : x;  // the component a reset leaves random
                    uint64_t* clr = r.op == FO_R ? x : z;
                    for (int e = lane; e < T; e += 64) {
                        const int q = tg[e];
                        clr[q] = 0ull;
                        keep[q] = rand_word(r.rsite0 + (uint32_t)e, s0, seed, sid);
                    }
                    break;
                }
                case FO_M:
                case FO_MX: {
                    uint64_t* read = r.op == FO_M ? x : z;
                    uint64_t* kick = r.op == FO_M ? z : x;
                    for (int e = lane; e < T; e += 64) {
                        const int t = tg[e], q = t & kFrameQubitMask;
                        rec[r.rec0 + e] = (t & kFrameInvert) ? ~read[q] : read[q];
                        kick[q] ^= rand_word(r.rsite0 + (uint32_t)e, s0, seed, sid);
                    }
                    if (r.thr) {
                        __syncthreads();
                        for (int e0 = 0; e0 < T; e0 += 4) {
                            uint32_t u[4] = {r.site0 / 4u + (uint32_t)(e0 >> 2), 0u, g_lo, g_hi};
                            philox4x32_10(u, seed, sid);
#pragma unroll
                            for (int l = 0; l < 4; ++l) {
                                if (e0 + l >= T) break;
                                const uint64_t f = __ballot(u[l] < r.thr);
                                if (f && lane == 0) rec[r.rec0 + e0 + l] ^= f;
                            }
                        }
                    }
                    break;
                }
                case FO_XERR:
                case FO_YERR:
                case FO_ZERR:
                    if (r.thr) {
                        for (int e0 = 0; e0 < T; e0 += 4) {
                            uint32_t u[4] = {r.site0 / 4u + (uint32_t)(e0 >> 2), 0u, g_lo, g_hi};
                            philox4x32_10(u, seed, sid);
#pragma unroll
                            for (int l = 0; l < 4; ++l) {
                                if (e0 + l >= T) break;
                                const uint64_t f = __ballot(u[l] < r.thr);
                                if (f && lane == 0) {
                                    const int q = tg[e0 + l];
                                    if (r.op != FO_ZERR) x[q] ^= f;
                                    if (r.op != FO_XERR) z[q] ^= f;
                                }
                            }
                        }
                    }
                    break;
                case FO_DEP1:
                    if (r.thr) {
                        for (int e0 = 0; e0 < T; e0 += 4) {
                            uint32_t u[4] = {r.site0 / 4u + (uint32_t)(e0 >> 2), 0u, g_lo, g_hi};
                            philox4x32_10(u, seed, sid);
#pragma unroll
                            for (int l = 0; l < 4; ++l) {
                                if (e0 + l >= T) break;
                                const bool fired = u[l] < r.thr;
                                if (__ballot(fired) == 0ull) continue;
                                const uint32_t P = fired ? 1u + scaled_index(u[l], r.thr, 3u) : 0u;
                                const uint64_t fx = __ballot(pauli_x(P)), fz = __ballot(pauli_z(P));
                                if (lane == 0) {
                                    const int q = tg[e0 + l];
                                    x[q] ^= fx;
                                    z[q] ^= fz;
                                }
                            }
                        }
                    }
                    break;
                case FO_DEP2:
                    if (r.thr) {
                        const int pairs = T / 2;
                        for (int e0 = 0; e0 < pairs; e0 += 4) {
                            uint32_t u[4] = {r.site0 / 4u + (uint32_t)(e0 >> 2), 0u, g_lo, g_hi};
                            philox4x32_10(u, seed, sid);
#pragma unroll
                            for (int l = 0; l < 4; ++l) {
                                if (e0 + l >= pairs) break;
                                const bool fired = u[l] < r.thr;
                                if (__ballot(fired) == 0ull) continue;
                                const uint32_t code = fired ? 1u + scaled_index(u[l], r.thr, 15u) : 0u;
                                const uint32_t Pa = code >> 2, Pb = code & 3u;
                                const uint64_t ax = __ballot(pauli_x(Pa)), az = __ballot(pauli_z(Pa));
                                const uint64_t bx = __ballot(pauli_x(Pb)), bz = __ballot(pauli_z(Pb));
                                if (lane == 0) {
                                    const int a = tg[2 * (e0 + l)], b = tg[2 * (e0 + l) + 1];
                                    x[a] ^= ax;
                                    z[a] ^= az;
                                    x[b] ^= bx;
                                    z[b] ^= bz;
                                }
                            }
                        }
                    }
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
// lanes may name one word (X_ERROR 0 1 0, a qubit in two DEPOLARIZE2 pairs, two
// gauge faults never): the XOR is an LDS atomic.  Before a wave's first fault the frame is all zero and stays so, so
// the wave starts at that fault's instruction, found by bisection over the
// instructions' first-fault indices (non-decreasing; the last instruction whose
// index is <= the fault holds it); rec is zeroed up front because the skipped
// measurements do not write their words.
template <bool PACKED>
__global__ __launch_bounds__(64) void frame_fault_kernel(DevCircuit c, int kind, int32_t f0, int32_t F, FrameOuts o) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x;
    uint64_t* x = reinterpret_cast<uint64_t*>(smem);  // [Q]
    uint64_t* z = x + c.Q;                            // [Q]
    uint64_t* rec = z + c.Q;                          // [M]
    const int waves = (F + 63) / 64;
    const unsigned long long bit = 1ull << lane;

    for (int w = blockIdx.x; w < waves; w += gridDim.x) {
        const int b0 = w * 64;
        const int valid = F - b0 < 64 ? F - b0 : 64;
        const int32_t first = f0 + b0;                        // the wave's first fault
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
                    for (int e = lane; e < T; e += 64) frame_h(x, z, tg[e]);
                    break;
                case FO_CX:
                    for (int e = lane; 2 * e < T; e += 64) frame_cx(x, z, tg[2 * e], tg[2 * e + 1]);
                    break;
                case FO_CZ:
                    for (int e = lane; 2 * e < T; e += 64) frame_cz(x, z, tg[2 * e], tg[2 * e + 1]);
                    break;
                case FO_R:
                case FO_RX:
                    for (int e = lane; e < T; e += 64) x[tg[e]] = z[tg[e]] = 0ull;
                    break;
                case FO_M:
                case FO_MX: {
                    const uint64_t* read = r.op == FO_M ? x : z;
                    for (int e = lane; e < T; e += 64) rec[r.rec0 + e] = read[tg[e] & kFrameQubitMask];
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
                const int32_t j = mine - base;
                if (mine >= 0 && j >= 0 && j < cnt) {
                    const int32_t comp = fault_comp(r.op, j, kind), e = fault_target(r.op, j, kind);
                    if (comp == FC_REC) {
                        atomicXor(reinterpret_cast<unsigned long long*>(rec + r.rec0 + e), bit);
                    } else {
                        const int q = tg[e] & kFrameQubitMask;
                        if (comp & FC_X) atomicXor(reinterpret_cast<unsigned long long*>(x + q), bit);
                        if (comp & FC_Z) atomicXor(reinterpret_cast<unsigned long long*>(z + q), bit);
                    }
                }
            }
            __syncthreads();
        }

        frame_write_outputs<PACKED>(c, rec, o, (int64_t)b0, valid, lane);
        __syncthreads();  // the frame is zeroed for the next 64 faults
    }
}

int launch_frame_sample(const DevCircuit& c, size_t lds, uint32_t seed, uint32_t stream_id, int64_t shot0, int64_t B,
                        bool packed, void* const outs[kFrameGroups], int num_cus, hipStream_t stream) {
    if (B <= 0) return 0;
    FrameOuts o;
    for (int g = 0; g < kFrameGroups; ++g) o.p[g] = outs[g];
    const void* fn = packed ? reinterpret_cast<const void*>(frame_sample_kernel<true>)
                            : reinterpret_cast<const void*>(frame_sample_kernel<false>);
    if (lds < 16) lds = 16;
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    long long grid = (long long)num_cus * 32;  // one wave per block; LDS decides how many a CU holds
    const long long waves = (B + 63) / 64;
    if (grid > waves) grid = waves;
    if (packed)
        hipLaunchKernelGGL(frame_sample_kernel<true>, dim3((unsigned)grid), dim3(64), lds, stream, c, seed, stream_id,
                           shot0, B, o);
    else
        hipLaunchKernelGGL(frame_sample_kernel<false>, dim3((unsigned)grid), dim3(64), lds, stream, c, seed,
                           stream_id, shot0, B, o);
    return (int)hipGetLastError();
}

int launch_frame_faults(const DevCircuit& c, size_t lds, int kind, int32_t f0, int32_t F, bool packed,
                        void* const outs[kFrameGroups], int num_cus, hipStream_t stream) {
    if (F <= 0) return 0;
    FrameOuts o;
    for (int g = 0; g < kFrameGroups; ++g) o.p[g] = outs[g];
    const void* fn = packed ? reinterpret_cast<const void*>(frame_fault_kernel<true>)
                            : reinterpret_cast<const void*>(frame_fault_kernel<false>);
    if (lds < 16) lds = 16;
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    int grid = num_cus * 32;  // as the sampler: one wave per block
    const int waves = (F + 63) / 64;
    if (grid > waves) grid = waves;
    if (packed)
        hipLaunchKernelGGL(frame_fault_kernel<true>, dim3((unsigned)grid), dim3(64), lds, stream, c, kind, f0, F, o);
    else
        hipLaunchKernelGGL(frame_fault_kernel<false>, dim3((unsigned)grid), dim3(64), lds, stream, c, kind, f0, F, o);
    return (int)hipGetLastError();
}

}  // namespace qdec
