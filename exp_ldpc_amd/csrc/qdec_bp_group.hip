// qdec_bp_group.hip -- bp_group_kernel: slot-group BP, messages in HBM.
//
// BP for graphs whose messages do not fit LDS (configs 4 and 5: 10^4 to 1.3*10^5
// columns), laid out so every HBM access of the message loops is a whole
// cache line.  A workgroup of grp_waves<T>() waves decodes a group of 64 shot slots
// together: lane l of every wave works on slot l.  The group owns a scratch
// block in HBM:
//   v2c [E][64] T   messages by CSR edge, slot-minor: a wave reading edge e of
//                   its 64 slots reads one contiguous 256-B (fp32) / 512-B run
//   c2v [E][64] T   by CSC position (the column pass reads it sequentially)
//   sw  [m]  u64    syndrome bit of check i for every slot (bit l = slot l)
//   xw  [n]  u64    hard decision of column j for every slot (one ballot)
//   pw  [m]  u64    parity of check i under the hard decision (residual words)
//   rw  [n_data] u64  residual readout ^ corr of slots being finalised
// Per iteration: check pass (waves split the checks, UC checks per step with
// all their loads issued first), barrier, column pass (waves split the
// columns), barrier, syndrome test (lanes split the checks: each lane xors the
// 64-slot hard-decision words of its row, so one pass tests all 64 slots),
// barrier.  Slots whose shot converged or reached max_iter are finalised
// (or queued for SSF) and refilled at once from a group-aggregated atomic
// counter, so a slot's work is its own shot's iteration count.  Refilling
// writes no messages: a slot's first check pass reads its columns' priors
// instead of v2c (the same values ldpc initialises the messages to), and its
// syndrome bits go into sw in one coalesced sweep per refill batch.
// Outputs of a finished slot come from the words: corr = base ^ xor of the
// fold blocks' words, fail = any logical's parity over its CSR support of the
// residual words (64 slots per gather), x as bytes; BP-unconverged shots go
// to the SSF queue (bytes, as the other BP kernels write it) when SSF is on.
// Arithmetic is bp_block_kernel's unrolled loops, operation for operation
// (min-sum: med3/fmin row minimum and ldpc's column prefix/suffix sums;
// product-sum: ldpc's forward/backward products and NaN guards), with alpha_t
// of the slot's own iteration.  HBM traffic per shot-iteration: the 16*E-byte
// message model (fp32; 32*E fp64) plus O(m + n) bytes of words.
// Waves per group: 4 for f32 (a 4-wave group fits 3 waves per SIMD, i.e. three
// groups per CU: +30 % on config 5 against 8-wave groups), 8 for f64 (register
// bound at 2 waves per SIMD either way; 8-wave groups finish and refill slots
// with twice the threads: config 4 f64 at p = 0.005, 2.9 iterations per shot,
// 604 k vs 401 k shots/s).
#include <hip/hip_runtime.h>

#include "qdec_block_layout.h"
#include "qdec_device.h"
#include "qdec_kernels.h"

namespace qdec {

template <typename T>
constexpr int grp_waves() {
    return sizeof(T) == 4 ? 4 : 8;
}
// Checks / columns per wave step: every load of a step is issued before any is
// used, so a wave keeps UC * DR (check pass) or UV * (column degree) loads of
// whole 64-slot lines in flight; the column pass has few edges per column, so
// it takes more columns per step.
template <typename T, int DR>
constexpr int grp_uc() {
    return sizeof(T) == 4 ? 4 : (DR <= 8 ? 4 : 2);
}
template <typename T, int DC>
constexpr int grp_uv() {
    return sizeof(T) == 4 ? (DC <= 4 ? 16 : 8) : (DC <= 4 ? 8 : 4);
}
constexpr int kLzTGrp = 16;           // logical-parity words per slot in the group kernel (k <= 512)

__device__ __forceinline__ int64_t readlane64(int64_t v, int l) {
    const int lo = __builtin_amdgcn_readlane((int)(uint32_t)v, l);
    const int hi = __builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)v >> 32), l);
    return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}

template <typename T, int METHOD, int DR, int DC>
__global__ __launch_bounds__(64 * grp_waves<T>()) void bp_group_kernel(DevGraph g, DecodeArgs a, unsigned char* scratch,
                                                               size_t group_bytes,
                                                               const int32_t* __restrict__ rp,
                                                               const int32_t* __restrict__ ci,
                                                               const int32_t* __restrict__ cp,
                                                               const int32_t* __restrict__ ce,
                                                               const int32_t* __restrict__ ecs,
                                                               const T* __restrict__ prior,
                                                               const T* __restrict__ ep) {
    constexpr int kGrpWaves = grp_waves<T>(), kGrpThreads = 64 * kGrpWaves;
    __shared__ unsigned long long s_bad, s_fail;
    __shared__ long long s_base;
    __shared__ int s_qbase;
    // per slot the logical-parity words of its residual (DevGraph::lz_t)
    __shared__ uint32_t s_lp[64 * kLzTGrp];
    // wave index as a scalar: the graph index loads of the passes are scalar loads
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), tid = threadIdx.x;
    const int m = g.m, n = g.n, nd = g.n_data;
    const GroupLayout L = group_layout(g, sizeof(T));
    unsigned long long* counter = reinterpret_cast<unsigned long long*>(scratch);
    unsigned char* blk = scratch + kGrpHeader + (size_t)blockIdx.x * group_bytes;
    T* v2c = reinterpret_cast<T*>(blk + L.v2c) + lane;
    T* c2v = reinterpret_cast<T*>(blk + L.c2v) + lane;
    uint64_t* sw = reinterpret_cast<uint64_t*>(blk + L.sw);
    uint64_t* xw = reinterpret_cast<uint64_t*>(blk + L.xw);
    uint64_t* pw = reinterpret_cast<uint64_t*>(blk + L.pw);
    uint64_t* rw = reinterpret_cast<uint64_t*>(blk + L.rw);
    const uint64_t below = (1ull << lane) - 1ull;
    const bool want_fail = a.fail && a.readout && g.k > 0;
    const bool lzcols = want_fail && g.lz_t && g.lz_tw <= kLzTGrp;
    for (int i = tid; i < 64 * kLzTGrp; i += kGrpThreads) s_lp[i] = 0u;  // (the refill's barrier orders it)
    int64_t shot = -1;  // slot `lane`'s shot: identical in every wave (all decisions are group-uniform)
    int it = 0;
    uint64_t need = ~0ull;  // slots to refill (uniform)
    for (;;) {
        if (need) {
            if (tid == 0) s_base = (long long)atomicAdd(counter, (unsigned long long)__popcll(need));
            __syncthreads();
            const long long b0 = s_base;
            if ((need >> lane) & 1) {
                const long long s2 = b0 + __popcll(need & below);
                shot = s2 < a.B ? s2 : -1;
                it = 0;
            }
            const uint64_t live = __ballot(((need >> lane) & 1) && shot >= 0);
            // syndrome words: the refilled slots' bits are replaced in one sweep
            // (per slot l a coalesced read of its shot's syndrome row)
            for (int i = tid; i < m; i += kGrpThreads) {
                uint64_t w = sw[i] & ~need;
                // four slots per round: their loads issued before any is used
                for (uint64_t rem = live; rem;) {
                    int ls[4];
                    uint8_t bv[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        ls[u] = rem ? __builtin_ctzll(rem) : -1;
                        rem &= rem - 1;
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        bv[u] = ls[u] >= 0 ? a.syn[(b0 + __popcll(need & ((1ull << ls[u]) - 1ull))) * m + i] : 0;
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        if (ls[u] >= 0) w |= (uint64_t)(bv[u] & 1) << ls[u];
                }
                sw[i] = w;
            }
        }
        const bool active = shot >= 0;
        if (!__syncthreads_or(active)) break;
        // every thread read the previous iteration's s_bad before this barrier;
        // the next atomics come two barriers later
        if (tid == 0) s_bad = 0;
        ++it;
        const T alpha = alpha_at<T>(it, a.ms_scaling);
        const bool fresh = it == 1;  // first pass of this slot's shot: v2c = priors
        // Every lane runs the passes, idle slots on garbage, so control flow is
        // wave-uniform: scalar branches, no exec masking.
        constexpr int UC = grp_uc<T, DR>(), UV = grp_uv<T, DC>();
        // Loads first, for the whole step (scalar-guarded by the row / column
        // degree, 32-bit offsets), then the arithmetic with pad positions masked
        // by selects (Big for the row minimum, the neutral factor 1 for the
        // products), so no load waits behind another's use.
        for (int i0 = wv * UC; i0 < m; i0 += kGrpWaves * UC) {  // check pass
            int e0[UC], d[UC], par[UC];
            T mv[UC][DR], pv[UC][DR];
#pragma unroll
            for (int u = 0; u < UC; ++u) {
                const int i = i0 + u;
                const int ii = i < m ? i : m - 1;
                e0[u] = rp[ii];
                d[u] = i < m ? rp[ii + 1] - e0[u] : 0;
            }
#pragma unroll
            for (int u = 0; u < UC; ++u)
#pragma unroll
                for (int t = 0; t < DR; ++t)
                    if (t < d[u]) mv[u][t] = v2c[(uint32_t)(e0[u] + t) * 64u];
#pragma unroll
            for (int u = 0; u < UC; ++u) {
                const int ii = i0 + u < m ? i0 + u : m - 1;
                // sw is written by this kernel: a volatile (vector) load, never the scalar cache
                par[u] = (int)((*(volatile const uint64_t*)&sw[ii] >> lane) & 1ull);
#pragma unroll
                for (int t = 0; t < DR; ++t) pv[u][t] = ep[e0[u] + t];  // padded array: unguarded
            }
#pragma unroll
            for (int u = 0; u < UC; ++u) {
                T v[DR];
#pragma unroll
                for (int t = 0; t < DR; ++t) v[t] = fresh ? pv[u][t] : mv[u][t];
                if constexpr (METHOD == 1) {
                    T m1 = Big<T>::v, m2 = Big<T>::v;
                    int pu = par[u];
#pragma unroll
                    for (int t = 0; t < DR; ++t) {
                        const bool on = t < d[u];
                        const T av = on ? fabs(v[t]) : Big<T>::v;  // Big changes neither minimum
                        m2 = med3(av, m1, m2);
                        m1 = fmin(m1, av);
                        pu ^= on && v[t] <= (T)0;
                    }
                    const T m1a = m1 * alpha, m2a = m2 * alpha;
#pragma unroll
                    for (int t = 0; t < DR; ++t)
                        if (t < d[u]) {
                            const T y = (fabs(v[t]) == m1) ? m2a : m1a;
                            c2v[(uint32_t)ecs[e0[u] + t] * 64u] = (pu ^ (v[t] <= (T)0)) ? -y : y;
                        }
                } else {
                    T r[DR], fw[DR];
                    T f = par[u] ? (T)-1 : (T)1;
#pragma unroll
                    for (int t = 0; t < DR; ++t) {
                        fw[t] = f;
                        r[t] = t < d[u] ? (T)2 / ((T)1 + v[t]) - (T)1 : (T)1;  // pads: the neutral factor
                        f *= r[t];
                    }
                    T b = (T)1;
#pragma unroll
                    for (int t = DR - 1; t >= 0; --t) {
                        if (t < d[u]) {
                            const T c = fw[t] * b;
                            c2v[(uint32_t)ecs[e0[u] + t] * 64u] = ((T)1 - c) / ((T)1 + c);
                        }
                        b *= r[t];
                    }
                }
            }
        }
        __syncthreads();
        for (int j0 = wv * UV; j0 < n; j0 += kGrpWaves * UV) {  // column pass
            int t0[UV], d[UV];
            T c[UV][DC];
#pragma unroll
            for (int u = 0; u < UV; ++u) {
                const int j = j0 + u;
                const int jj = j < n ? j : n - 1;
                t0[u] = cp[jj];
                d[u] = j < n ? cp[jj + 1] - t0[u] : 0;
            }
#pragma unroll
            for (int u = 0; u < UV; ++u)
#pragma unroll
                for (int t = 0; t < DC; ++t)
                    if (t < d[u]) c[u][t] = c2v[(uint32_t)(t0[u] + t) * 64u];  // CSC order: contiguous
#pragma unroll
            for (int u = 0; u < UV; ++u) {
                const int j = j0 + u;
                if (j >= n) break;
                T pre[DC];
                T acc = prior[j];
                bool hard;
                if constexpr (METHOD == 1) {
#pragma unroll
                    for (int t = 0; t < DC; ++t) {
                        pre[t] = acc;
                        acc = t < d[u] ? acc + c[u][t] : acc;
                    }
                    hard = acc <= (T)0;
                } else {
#pragma unroll
                    for (int t = 0; t < DC; ++t) {
                        pre[t] = acc;
                        T x = acc * c[u][t];
                        if (isnan(x)) x = (T)1;
                        acc = t < d[u] ? x : acc;
                    }
                    hard = acc >= (T)1;
                }
                const uint64_t hw = __ballot(hard);
                if (lane == 0) xw[j] = hw;
                if (a.llr_out && active) {
                    T* lo = reinterpret_cast<T*>(a.llr_out);
                    if constexpr (METHOD == 1) lo[shot * n + j] = acc;
                    else lo[shot * n + j] = (T)log((double)((T)1 / acc));
                }
                if constexpr (METHOD == 1) {
                    T suf = (T)0;
#pragma unroll
                    for (int t = DC - 1; t >= 0; --t)
                        if (t < d[u]) {
                            v2c[(uint32_t)ce[t0[u] + t] * 64u] = pre[t] + suf;
                            suf += c[u][t];
                        }
                } else {
                    T suf = (T)1;
#pragma unroll
                    for (int t = DC - 1; t >= 0; --t)
                        if (t < d[u]) {
                            v2c[(uint32_t)ce[t0[u] + t] * 64u] = pre[t] * suf;
                            suf *= c[u][t];
                            if (isnan(suf)) suf = (T)1;
                        }
                }
            }
        }
        __syncthreads();
        {  // syndrome test: lane-parallel over checks, 64 slots per word
            uint64_t bad = 0;
            for (int i = tid; i < m; i += kGrpThreads) {
                const int e0 = rp[i], d = rp[i + 1] - e0;
                uint64_t p = sw[i];
                int cc[DR];
#pragma unroll
                for (int t = 0; t < DR; ++t)
                    if (t < d) cc[t] = ci[e0 + t];
#pragma unroll
                for (int t = 0; t < DR; ++t)
                    if (t < d) p ^= xw[cc[t]];
                pw[i] = p;
                bad |= p;
            }
            if (bad) atomicOr(&s_bad, (unsigned long long)bad);
        }
        __syncthreads();
        const uint64_t anybad = s_bad;
        const bool conv = active && !((anybad >> lane) & 1ull);
        const bool done = conv || (active && it >= a.max_iter);
        const uint64_t D = __ballot(done);
        need = D;
        if (!D) continue;
        const uint64_t C = __ballot(conv);
        const uint64_t Q = a.ssf ? (D & ~C) : 0ull;  // BP-unconverged shots -> the SSF queue
        const uint64_t F = D & ~Q;                   // finalised here
        if (wv == 0 && done && a.iters) a.iters[shot] = it;
        if (Q) {
            if (tid == 0) s_qbase = atomicAdd(a.q_count, __popcll(Q));
            __syncthreads();
            const int qb = s_qbase;
            if (wv == 0 && ((Q >> lane) & 1)) a.q_idx[qb + __popcll(Q & below)] = shot;
            for (int j = tid; j < n; j += kGrpThreads) {
                const uint64_t w = xw[j];
                int r = 0;
                for (uint64_t rem = Q; rem; rem &= rem - 1, ++r)
                    a.q_x[(int64_t)(qb + r) * n + j] = (uint8_t)((w >> __builtin_ctzll(rem)) & 1ull);
            }
            for (int i = tid; i < m; i += kGrpThreads) {
                const uint64_t w = pw[i];
                int r = 0;
                for (uint64_t rem = Q; rem; rem &= rem - 1, ++r)
                    a.q_r[(int64_t)(qb + r) * m + i] = (uint8_t)((w >> __builtin_ctzll(rem)) & 1ull);
            }
        }
        if (F) {
            if (a.x_out)
                for (int j = tid; j < n; j += kGrpThreads) {
                    const uint64_t w = xw[j];
                    for (uint64_t rem = F; rem; rem &= rem - 1) {
                        const int l = __builtin_ctzll(rem);
                        a.x_out[readlane64(shot, l) * n + j] = (uint8_t)((w >> l) & 1ull);
                    }
                }
            if (a.corr_out || want_fail) {
                for (int q = tid; q < nd; q += kGrpThreads) {
                    uint64_t cw = 0;
                    for (int b = 0; b < g.fold_blocks; ++b) cw ^= xw[b * nd + q];
                    uint64_t rword = 0;
                    // four finishing slots per round, loads first
                    for (uint64_t rem = F; rem;) {
                        int ls[4];
                        int64_t sls[4];
                        uint8_t bb[4], rb[4];
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            ls[u] = rem ? __builtin_ctzll(rem) : -1;
                            rem &= rem - 1;
                            sls[u] = ls[u] >= 0 ? readlane64(shot, ls[u]) : 0;
                        }
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            bb[u] = (ls[u] >= 0 && a.base) ? a.base[sls[u] * nd + q] : 0;
                            rb[u] = (ls[u] >= 0 && want_fail) ? a.readout[sls[u] * nd + q] : 0;
                        }
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            if (ls[u] < 0) continue;
                            const int cb = (int)((cw >> ls[u]) & 1ull) ^ (bb[u] & 1);
                            if (a.corr_out) a.corr_out[sls[u] * nd + q] = (uint8_t)cb;
                            if (want_fail) rword |= (uint64_t)((rb[u] ^ cb) & 1) << ls[u];
                        }
                    }
                    if (lzcols) {  // the residual's ones XOR their qubit's parity words into their slots'
                        if (rword)
                            for (int t = 0; t < g.lz_tw; ++t) {
                                const uint32_t v = g.lz_t[(size_t)q * g.lz_tw + t];
                                if (v)
                                    for (uint64_t rem = rword; rem; rem &= rem - 1)
                                        atomicXor(&s_lp[__builtin_ctzll(rem) * kLzTGrp + t], v);
                            }
                    } else if (want_fail) {
                        rw[q] = rword;
                    }
                }
            }
            if (lzcols) {
                __syncthreads();  // parity words complete
                if (wv == 0) {
                    uint32_t o = 0;
                    for (int t = 0; t < g.lz_tw; ++t) {
                        o |= s_lp[lane * kLzTGrp + t];
                        s_lp[lane * kLzTGrp + t] = 0u;
                    }
                    const uint64_t fb = __ballot(o != 0u);
                    if (lane == 0) s_fail = fb & F;
                }
                __syncthreads();
            } else if (want_fail) {
                if (tid == 0) s_fail = 0;
                __syncthreads();  // rw complete
                uint64_t fm = 0;
                for (int r = tid; r < g.k; r += kGrpThreads) {
                    uint64_t p = 0;
                    const int t1 = g.lz_ptr[r + 1];
                    int t = g.lz_ptr[r];
                    for (; t + 4 <= t1; t += 4) {  // four supports per round, loads first
                        int q4[4];
                        uint64_t v4[4];
#pragma unroll
                        for (int u = 0; u < 4; ++u) q4[u] = g.lz_idx[t + u];
#pragma unroll
                        for (int u = 0; u < 4; ++u) v4[u] = rw[q4[u]];
                        p ^= v4[0] ^ v4[1] ^ v4[2] ^ v4[3];
                    }
                    for (; t < t1; ++t) p ^= rw[g.lz_idx[t]];
                    fm |= p;
                }
                if (fm & F) atomicOr(&s_fail, (unsigned long long)(fm & F));
                __syncthreads();
            }
            if (wv == 0 && ((F >> lane) & 1)) {
                if (a.status) a.status[shot] = (uint8_t)(conv ? 3 : 0);
                if (a.ssf_steps) a.ssf_steps[shot] = 0;
                if (a.fail) a.fail[shot] = (uint8_t)(want_fail ? ((s_fail >> lane) & 1ull) : 0);
            }
        }
        __syncthreads();  // every read of s_fail and of the words before the refill
    }
}

// bp_group_kernel T, METHOD, DR, DC (DR in {8, 16} x DC in {4, 8}: the degrees it unrolls)
template <typename T, int METHOD>
static void add_group_types(KernelTable& t) {
    constexpr int kGrpThreads = 64 * grp_waves<T>();
    t.push_back(QDEC_INST(kGrpThreads, bp_group_kernel, T, METHOD, 8, 4));
    t.push_back(QDEC_INST(kGrpThreads, bp_group_kernel, T, METHOD, 8, 8));
    t.push_back(QDEC_INST(kGrpThreads, bp_group_kernel, T, METHOD, 16, 4));
    t.push_back(QDEC_INST(kGrpThreads, bp_group_kernel, T, METHOD, 16, 8));
}

void add_group_kernels(KernelTable& t) {
    add_group_types<float, 0>(t);
    add_group_types<float, 1>(t);
    add_group_types<double, 0>(t);
    add_group_types<double, 1>(t);
}

}  // namespace qdec
