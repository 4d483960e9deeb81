// qdec_frame_hbm.hip -- the Pauli-frame sampler and the fault propagation of
// qdec_frame.hip with the frame in global memory (QD_FRAME_HBM):
// circuits whose x[Q], z[Q], rec[M] words (16 Q + 8 M bytes per 64 shots) do not
// fit the LDS kernels' 160 KiB.
//
// The mapping, the frame rules and every draw are those of qdec_frame.hip: one
// workgroup is one wave, a wave runs 64 consecutive shots (faults), lane = shot at
// a noise site, and the outputs are bit-identical.  What differs is where the
// words live and how a noise site reaches them:
//   slots   workgroup b owns slot b of the launch's scratch, `slot_words` u64
//           words laid out x[Q] z[Q] rec[M]; it walks its 64-shot words
//           grid-stride and re-zeroes the slot between them.  No other workgroup
//           touches the slot, so the barrier between instructions (a fence at
//           workgroup scope) orders all traffic to it.
//   gates   as in LDS, lanes split the (pairwise disjoint) targets; four targets
//           per lane are loaded before the first is stored, so their round trips
//           to memory overlap instead of queueing behind possible aliases.
//   noise   lane 0 applying one site after the other would be a chain of
//           dependent memory round trips.  Instead the ballot words of up to 64
//           consecutive sites are built so that lane l keeps site e0 + l's words,
//           and one exec-masked read-modify-write applies them: lanes whose words
//           are 0 do nothing (at low p most are), the others name distinct frame
//           words.  An instruction that names a qubit twice (FrameOpRec::dup, set
//           by build_circuit) applies its fired sites one lane at a time in site
//           order instead, a barrier after each: plain loads and stores, no
//           atomics (an atomic executes at the memory side and drops the line
//           from the XCD's L2).
// The fault kernel injects with a plain XOR per lane, and with atomicXor only in
// an instruction marked dup (two lanes may name one word there).
#include "qdec_frame_dev.h"

namespace qdec {

namespace {

constexpr int kGateUnroll = 4;  // targets per lane in flight in one gate step

// H: swap x and z of every target
__device__ __forceinline__ void hbm_h(uint64_t* x, uint64_t* z, const int32_t* tg, int T, int lane) {
    for (int e = lane; e < T; e += 64 * kGateUnroll) {
        int q[kGateUnroll];
        uint64_t vx[kGateUnroll], vz[kGateUnroll];
#pragma unroll
        for (int u = 0; u < kGateUnroll; ++u) {
            q[u] = e + 64 * u < T ? tg[e + 64 * u] : -1;
            if (q[u] >= 0) vx[u] = x[q[u]], vz[u] = z[q[u]];
        }
#pragma unroll
        for (int u = 0; u < kGateUnroll; ++u)
            if (q[u] >= 0) x[q[u]] = vz[u], z[q[u]] = vx[u];
    }
}

// CX (cz = false): x_b ^= x_a, z_a ^= z_b; CZ: z_a ^= x_b, z_b ^= x_a; P pairs
__device__ __forceinline__ void hbm_pairs(uint64_t* x, uint64_t* z, const int32_t* tg, int P, int lane, bool cz) {
    for (int e = lane; e < P; e += 64 * kGateUnroll) {
        int a[kGateUnroll], b[kGateUnroll];
        uint64_t xa[kGateUnroll], xb[kGateUnroll], za[kGateUnroll], zb[kGateUnroll];
#pragma unroll
        for (int u = 0; u < kGateUnroll; ++u) {
            const int p = e + 64 * u;
            a[u] = b[u] = -1;
            if (p < P) {
                a[u] = tg[2 * p], b[u] = tg[2 * p + 1];
                xa[u] = x[a[u]], xb[u] = x[b[u]], za[u] = z[a[u]], zb[u] = z[b[u]];
            }
        }
#pragma unroll
        for (int u = 0; u < kGateUnroll; ++u) {
            if (a[u] < 0) continue;
            if (cz) {
                z[a[u]] = za[u] ^ xb[u];
                z[b[u]] = zb[u] ^ xa[u];
            } else {
                x[b[u]] = xb[u] ^ xa[u];
                z[a[u]] = za[u] ^ zb[u];
            }
        }
    }
}

// Apply a batch of noise sites: `any` = this lane's site fired.  Distinct words
// (dup == false): every lane at once.  Otherwise one lane after the other in site
// order, each behind a barrier, so a word two sites name sees both XORs.
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

// The Philox block of sites e0 + 4 k .. + 3 of instruction r (e0 a multiple of 4)
__device__ __forceinline__ void site_block(uint32_t (&u)[4], const FrameOpRec& r, int e0, int k, uint32_t g_lo,
                                           uint32_t g_hi, uint32_t seed, uint32_t sid) {
    u[0] = r.site0 / 4u + (uint32_t)((e0 >> 2) + k), u[1] = 0u, u[2] = g_lo, u[3] = g_hi;
    philox4x32_10(u, seed, sid);
}

// Bernoulli sites e0 .. e0 + n (n <= 64): lane l < n gets the ballot word of site e0 + l
__device__ __forceinline__ uint64_t bernoulli_words(const FrameOpRec& r, int e0, int n, int lane, uint32_t g_lo,
                                                    uint32_t g_hi, uint32_t seed, uint32_t sid) {
    uint64_t w = 0ull;
    for (int k = 0; 4 * k < n; ++k) {
        uint32_t u[4];
        site_block(u, r, e0, k, g_lo, g_hi, seed, sid);
#pragma unroll
        for (int l = 0; l < 4; ++l) {
            if (4 * k + l >= n) break;
            const uint64_t f = __ballot(u[l] < r.thr);
            if (lane == 4 * k + l) w = f;
        }
    }
    return w;
}

}  // namespace

template <bool PACKED>
__global__ __launch_bounds__(64) void frame_sample_hbm_kernel(DevCircuit c, uint64_t* scratch, int64_t slot_words,
                                                              uint32_t seed, uint32_t sid, int64_t shot0, int64_t B,
                                                              FrameOuts o) {
    const int lane = threadIdx.x;
    uint64_t* x = scratch + (int64_t)blockIdx.x * slot_words;  // [Q]
    uint64_t* z = x + c.Q;                                     // [Q]
    uint64_t* rec = z + c.Q;                                   // [M]: every word is written by its measurement
    const int64_t waves = (B + 63) / 64;

    for (int64_t w = blockIdx.x; w < waves; w += gridDim.x) {
        const int64_t b0 = w * 64;
        const int valid = (int)(B - b0 < 64 ? B - b0 : 64);
        const uint64_t s0 = (uint64_t)(shot0 + b0);
        const uint64_t shot = s0 + (uint64_t)lane;
        const uint32_t g_lo = (uint32_t)shot, g_hi = (uint32_t)(shot >> 32);
        for (int64_t q = lane; q < 2 * (int64_t)c.Q; q += 64) x[q] = 0ull;
        __syncthreads();

        for (int i = 0; i < c.n_ops; ++i) {
            const FrameOpRec r = c.ops[i];
            const int32_t* tg = c.targets + r.tgt_off;
            const int T = r.tgt_cnt;
            switch (r.op) {
                case FO_H:
                    hbm_h(x, z, tg, T, lane);
                    break;
                case FO_CX:
                case FO_CZ:
                    hbm_pairs(x, z, tg, T / 2, lane, r.op == FO_CZ);
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
                    for (int e = lane; e < T; e += 64 * kGateUnroll) {
                        int t[kGateUnroll];
                        uint64_t vr[kGateUnroll], vk[kGateUnroll];
#pragma unroll
                        for (int u = 0; u < kGateUnroll; ++u) {
                            t[u] = e + 64 * u < T ? tg[e + 64 * u] : -1;
                            if (t[u] >= 0) vr[u] = read[t[u] & kFrameQubitMask], vk[u] = kick[t[u] & kFrameQubitMask];
                        }
#pragma unroll
                        for (int u = 0; u < kGateUnroll; ++u) {
                            if (t[u] < 0) continue;
                            const int ee = e + 64 * u;
                            rec[r.rec0 + ee] = (t[u] & kFrameInvert) ? ~vr[u] : vr[u];
                            kick[t[u] & kFrameQubitMask] = vk[u] ^ rand_word(r.rsite0 + (uint32_t)ee, s0, seed, sid);
                        }
                    }
                    if (r.thr) {
                        __syncthreads();
                        for (int e0 = 0; e0 < T; e0 += 64) {  // the records of one instruction are distinct words
                            const int n = T - e0 < 64 ? T - e0 : 64;
                            const uint64_t f = bernoulli_words(r, e0, n, lane, g_lo, g_hi, seed, sid);
                            if (f) rec[r.rec0 + e0 + lane] ^= f;
                        }
                    }
                    break;
                }
                case FO_XERR:
                case FO_YERR:
                case FO_ZERR:
                    if (r.thr) {
                        for (int e0 = 0; e0 < T; e0 += 64) {
                            const int n = T - e0 < 64 ? T - e0 : 64;
                            const uint64_t f = bernoulli_words(r, e0, n, lane, g_lo, g_hi, seed, sid);
                            apply_sites(r.dup != 0, f != 0ull, lane, [&] {
                                const int q = tg[e0 + lane];
                                if (r.op != FO_ZERR) x[q] ^= f;
                                if (r.op != FO_XERR) z[q] ^= f;
                            });
                        }
                    }
                    break;
                case FO_DEP1:
                    if (r.thr) {
                        for (int e0 = 0; e0 < T; e0 += 64) {
                            const int n = T - e0 < 64 ? T - e0 : 64;
                            uint64_t wx = 0ull, wz = 0ull;
                            for (int k = 0; 4 * k < n; ++k) {
                                uint32_t u[4];
                                site_block(u, r, e0, k, g_lo, g_hi, seed, sid);
#pragma unroll
                                for (int l = 0; l < 4; ++l) {
                                    if (4 * k + l >= n) break;
                                    const bool fired = u[l] < r.thr;
                                    if (__ballot(fired) == 0ull) continue;
                                    const uint32_t P = fired ? 1u + scaled_index(u[l], r.thr, 3u) : 0u;
                                    const uint64_t fx = __ballot(pauli_x(P)), fz = __ballot(pauli_z(P));
                                    if (lane == 4 * k + l) wx = fx, wz = fz;
                                }
                            }
                            apply_sites(r.dup != 0, (wx | wz) != 0ull, lane, [&] {
                                const int q = tg[e0 + lane];
                                if (wx) x[q] ^= wx;
                                if (wz) z[q] ^= wz;
                            });
                        }
                    }
                    break;
                case FO_DEP2:
                    if (r.thr) {
                        const int pairs = T / 2;
                        for (int e0 = 0; e0 < pairs; e0 += 64) {
                            const int n = pairs - e0 < 64 ? pairs - e0 : 64;
                            uint64_t ax = 0ull, az = 0ull, bx = 0ull, bz = 0ull;
                            for (int k = 0; 4 * k < n; ++k) {
                                uint32_t u[4];
                                site_block(u, r, e0, k, g_lo, g_hi, seed, sid);
#pragma unroll
                                for (int l = 0; l < 4; ++l) {
                                    if (4 * k + l >= n) break;
                                    const bool fired = u[l] < r.thr;
                                    if (__ballot(fired) == 0ull) continue;
                                    const uint32_t code = fired ? 1u + scaled_index(u[l], r.thr, 15u) : 0u;
                                    const uint32_t Pa = code >> 2, Pb = code & 3u;
                                    const uint64_t fax = __ballot(pauli_x(Pa)), faz = __ballot(pauli_z(Pa));
                                    const uint64_t fbx = __ballot(pauli_x(Pb)), fbz = __ballot(pauli_z(Pb));
                                    if (lane == 4 * k + l) ax = fax, az = faz, bx = fbx, bz = fbz;
                                }
                            }
                            apply_sites(r.dup != 0, (ax | az | bx | bz) != 0ull, lane, [&] {
                                const int a = tg[2 * (e0 + lane)], b = tg[2 * (e0 + lane) + 1];
                                if (ax) x[a] ^= ax;
                                if (az) z[a] ^= az;
                                if (bx) x[b] ^= bx;
                                if (bz) z[b] ^= bz;
                            });
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

// frame_fault_kernel (qdec_frame.hip) on a slot in global memory; see there for
// the rules, the injection order and the bisection to the wave's first instruction.
template <bool PACKED>
__global__ __launch_bounds__(64) void frame_fault_hbm_kernel(DevCircuit c, uint64_t* scratch, int64_t slot_words,
                                                             int kind, int32_t f0, int32_t F, FrameOuts o) {
    const int lane = threadIdx.x;
    uint64_t* x = scratch + (int64_t)blockIdx.x * slot_words;  // [Q]
    uint64_t* z = x + c.Q;                                     // [Q]
    uint64_t* rec = z + c.Q;                                   // [M]
    const int waves = (F + 63) / 64;
    const unsigned long long bit = 1ull << lane;

    for (int w = blockIdx.x; w < waves; w += gridDim.x) {
        const int b0 = w * 64;
        const int valid = F - b0 < 64 ? F - b0 : 64;
        const int32_t first = f0 + b0;  // the wave's first fault
        const int32_t mine = lane < valid ? first + lane : -1;
        for (int64_t q = lane; q < slot_words; q += 64) x[q] = 0ull;  // x, z and rec are one range
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
                    hbm_h(x, z, tg, T, lane);
                    break;
                case FO_CX:
                case FO_CZ:
                    hbm_pairs(x, z, tg, T / 2, lane, r.op == FO_CZ);
                    break;
                case FO_R:
                case FO_RX:
                    for (int e = lane; e < T; e += 64) x[tg[e]] = z[tg[e]] = 0ull;
                    break;
                case FO_M:
                case FO_MX: {
                    const uint64_t* read = r.op == FO_M ? x : z;
                    for (int e = lane; e < T; e += 64 * kGateUnroll) {
                        uint64_t v[kGateUnroll];
#pragma unroll
                        for (int u = 0; u < kGateUnroll; ++u)
                            if (e + 64 * u < T) v[u] = read[tg[e + 64 * u] & kFrameQubitMask];
#pragma unroll
                        for (int u = 0; u < kGateUnroll; ++u)
                            if (e + 64 * u < T) rec[r.rec0 + e + 64 * u] = v[u];
                    }
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
                    // the lanes of one instruction name distinct words unless it names a qubit twice
                    auto inject = [&](uint64_t* word) {
                        if (r.dup)
                            atomicXor(reinterpret_cast<unsigned long long*>(word), bit);
                        else
                            *word ^= bit;
                    };
                    if (comp == FC_REC) {
                        inject(rec + r.rec0 + e);
                    } else {
                        const int q = tg[e] & kFrameQubitMask;
                        if (comp & FC_X) inject(x + q);
                        if (comp & FC_Z) inject(z + q);
                    }
                }
            }
            __syncthreads();
        }

        frame_write_outputs<PACKED>(c, rec, o, (int64_t)b0, valid, lane);
        __syncthreads();  // the frame is zeroed for the next 64 faults
    }
}

int launch_frame_sample_hbm(const DevCircuit& c, void* scratch, size_t slot_bytes, int64_t slots, uint32_t seed,
                            uint32_t stream_id, int64_t shot0, int64_t B, bool packed,
                            void* const outs[kFrameGroups], hipStream_t stream) {
    if (B <= 0) return 0;
    if (!scratch || slots < 1) return (int)hipErrorInvalidValue;
    FrameOuts o;
    for (int g = 0; g < kFrameGroups; ++g) o.p[g] = outs[g];
    const int64_t waves = (B + 63) / 64;
    const int64_t grid = waves < slots ? waves : slots;  // a resident workgroup per slot
    auto* s = static_cast<uint64_t*>(scratch);
    const int64_t words = (int64_t)(slot_bytes / 8);
    if (packed)
        hipLaunchKernelGGL(frame_sample_hbm_kernel<true>, dim3((unsigned)grid), dim3(64), 0, stream, c, s, words, seed,
                           stream_id, shot0, B, o);
    else
        hipLaunchKernelGGL(frame_sample_hbm_kernel<false>, dim3((unsigned)grid), dim3(64), 0, stream, c, s, words,
                           seed, stream_id, shot0, B, o);
    return (int)hipGetLastError();
}

int launch_frame_faults_hbm(const DevCircuit& c, void* scratch, size_t slot_bytes, int64_t slots, int kind,
                            int32_t f0, int32_t F, bool packed, void* const outs[kFrameGroups], hipStream_t stream) {
    if (F <= 0) return 0;
    if (!scratch || slots < 1) return (int)hipErrorInvalidValue;
    FrameOuts o;
    for (int g = 0; g < kFrameGroups; ++g) o.p[g] = outs[g];
    const int64_t waves = ((int64_t)F + 63) / 64;
    const int64_t grid = waves < slots ? waves : slots;
    auto* s = static_cast<uint64_t*>(scratch);
    const int64_t words = (int64_t)(slot_bytes / 8);
    if (packed)
        hipLaunchKernelGGL(frame_fault_hbm_kernel<true>, dim3((unsigned)grid), dim3(64), 0, stream, c, s, words, kind,
                           f0, F, o);
    else
        hipLaunchKernelGGL(frame_fault_hbm_kernel<false>, dim3((unsigned)grid), dim3(64), 0, stream, c, s, words, kind,
                           f0, F, o);
    return (int)hipGetLastError();
}

}  // namespace qdec
