// qdec_ms_lds64.hip -- bp_ms_lds64_kernel: LDS-resident min-sum BP, f64.
//
// bp_ms_lds_kernel's one-shot-per-CU scheme at ldpc's precision.  The f64 edge
// slots of config 4 (33,600 x 8 B) do not fit the 160 KB LDS, so no message is
// kept there: each variable thread keeps the v2c messages it sent last
// iteration in registers, and the check side is reduced to its min-sum state,
// built by LDS atomics on the IEEE bit patterns (|v| >= +0 orders like an
// unsigned integer, so ds_min_u64 is the exact minimum):
//   m1[b][i], m2[b][i]  u64 bits (two arrays): minimum and second minimum of
//             |v| over the row, with multiplicity (a repeated minimum gives m2 = m1)
//   parw[b]   per check: syndrome ^ parity of (v <= 0) over the row
//   hdw[b]    per check: parity of the hard decision (the syndrome test)
// Both minima come from ONE pass of the messages: each message x does
//   old = ds_min_rtn_u64(m1, x);  ds_min_u64(m2, max(old, x)).
// The updates of m1 are atomic, so they have a total order; with a1 <= a2 <= ...
// the row's sorted values, min over the messages of max(old, x) is a2:
//   >= a2: a message x >= a2 gives max >= a2; a minimum message x = a1 whose old
//          is >= a2 too unless an equal minimum came first (then a2 = a1);
//   <= a2: of the messages holding a1 and a2, the later one sees old <= the
//          other's value, and its max is a2.
// so m2 is the second minimum with multiplicity (kBig for a row of one edge),
// the two-pass construction's value bit for bit, without the second pass over
// the messages and its barrier.
// Buffers alternate by iteration parity b = it & 1.  Per iteration (2 barriers):
//   D  variable pass: c2v of edge (i, v) = alpha * (|v| == m1 ? m2 : m1) with
//      sign parw ^ (v <= 0) -- ldpc's leave-one-out minimum and sign, the same
//      selection as MsCore's and the f32 kernel's -- then ldpc's prefix / suffix
//      sums, the hard decision (xor into hdw[b]), and the new v2c messages'
//      atomics into buffer b ^ 1 (the two minima above, xor of the sign parity)
//   B  syndrome test of hdw[b] (a flag per wave); buffer b reset for iteration
//      it + 2 (every read of it is behind the barrier)
// A v2c message is never -0 (see bp_ms_lds_kernel), so (bits(v) - 1) >> 63 is
// ldpc's (v <= 0).  Finished shots are queued like bp_ms_lds_kernel's.
#include <hip/hip_runtime.h>

#include "qdec_block_layout.h"
#include "qdec_device.h"
#include "qdec_kernels.h"

namespace qdec {

__device__ __forceinline__ unsigned long long dbits(double x) { return (unsigned long long)__double_as_longlong(x); }

// Iteration 1's check states depend on the priors only (every v2c message of
// column j is its prior): m64_init_kernel builds them once per launch in slot
// order -- m1[m], m2[m] (u64 bits, the row's minimum and second minimum of
// |prior| with multiplicity), then par[W] (u32 words: parity of (prior <= 0) over
// the row) -- and every shot copies them into LDS instead of running the
// message atomics.  The values are those of the atomics (same multiset).
__global__ __launch_bounds__(256) void m64_init_kernel(DevGraph g, const double* __restrict__ prior,
                                                      const uint16_t* __restrict__ cslot,
                                                      unsigned long long* __restrict__ img) {
    const int s = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    const unsigned long long kBig = dbits(Big<double>::v);
    unsigned long long m1 = kBig, m2 = kBig;
    uint32_t par = 0;
    if (s < g.m) {
        const int i = cslot[s];
        for (int e = g.row_ptr[i]; e < g.row_ptr[i + 1]; ++e) {
            const unsigned long long pb = dbits(prior[g.col_idx[e]]);
            const unsigned long long x = pb & 0x7fffffffffffffffull;
            par ^= (uint32_t)((pb - 1ull) >> 63);  // (prior <= 0); a prior is never -0
            if (x < m1) {
                m2 = m1;
                m1 = x;
            } else if (x < m2) {
                m2 = x;
            }
        }
        img[s] = m1;
        img[(size_t)g.m + s] = m2;
    }
    const unsigned long long bw = __ballot(par != 0u);
    const int w0 = (s - lane) >> 5;
    uint32_t* pw = reinterpret_cast<uint32_t*>(img + (size_t)2 * g.m);
    if (lane < 2 && w0 + lane < (int)m64_words(g)) pw[w0 + lane] = (uint32_t)(bw >> (32 * lane));
}

// The check states live at host-placed slots (DevGraph::m64_etab / m64_check,
// m64_layout in qdec_abi.cpp: a wave's state accesses spread over the LDS
// banks); every array below is indexed by slot, and the syndrome input and the
// residual output go through cslot (slot -> check).
// D3R: the variable rounds r < D3R hold columns of degree <= 3 only (host:
// DevGraph::m64_d3r), so their messages take 3 registers instead of kMlDC.
template <int VPT, int D3R>
__global__ __launch_bounds__(kM64Threads) void bp_ms_lds64_kernel(DevGraph g, DecodeArgs a,
                                                                 const uint16_t* __restrict__ etab,
                                                                 const double* __restrict__ prior,
                                                                 const uint16_t* __restrict__ cslot,
                                                                 const unsigned long long* __restrict__ img) {
    static_assert(VPT * 3 <= 32 && VPT <= 32 && D3R <= VPT, "degree and decision bits");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    long long* next = reinterpret_cast<long long*>(smem + kCtrlNext);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int m = g.m, n = g.n;
    const int W = (int)m64_words(g);
    unsigned long long* st = reinterpret_cast<unsigned long long*>(smem + kCtrl);  // m1 [2][m], then m2 [2][m]
    uint32_t* synw = reinterpret_cast<uint32_t*>(smem + kCtrl + (size_t)2 * m * 16);
    uint32_t* parw = synw + W;     // [2][W]
    uint32_t* hdw = parw + 2 * W;  // [2][W]
    int* flags = reinterpret_cast<int*>(hdw + 2 * W);  // [2][16]
    // variable slot of this thread: tid * 67 mod 1024, so the 64 lanes of a wave own
    // columns 67 apart instead of 64 neighbours (neighbouring columns of a
    // hypergraph product share checks, and lanes of one wave hitting one check's
    // state serialise its atomics)
    const int tq = (tid * 67) & (kM64Threads - 1);
    const int ncr = tid < m ? (m - tid + kM64Threads - 1) / kM64Threads : 0;  // checks of this thread
    const unsigned long long kBig = dbits(Big<double>::v);
    constexpr unsigned long long kAbs = 0x7fffffffffffffffull;
    if (blockIdx.x == 0 && tid == 0) *a.q_count = (int32_t)a.B;

    // per-variable constants: degree, check of each edge (u16 pairs); the priors
    // are re-read from global memory (L1) where used, to leave the registers to
    // the messages
    uint32_t ep[VPT][kMlDC / 2];
    uint32_t djs = 0;  // 3 bits per owned variable: its degree (real edges come first)
    // prior of round r's column (a pad slot, j >= n, reads column n - 1: its value
    // only reaches the pad's unused hard decision); tqv is an opaque copy of tq
    // taken per pass, so the column offsets are re-derived where used instead of
    // being held (spilled) across the loop
    auto prior_of = [&](const double* pr, int tqv, int r) -> double {
        return pr[min(r * kM64Threads + tqv, n - 1)];
    };
    auto opaque_tq = [&]() {
        int t = tq;
        asm volatile("" : "+v"(t));
        return t;
    };
    // the same for tid: the per-shot addresses (syndrome, image, queue) are
    // re-derived each shot instead of being hoisted out of the shot loop and spilled
    auto opaque_tid = [&]() {
        int t = tid;
        asm volatile("" : "+v"(t));
        return t;
    };
    // barrier ordering LDS only: global stores (the queue) stay in flight
    auto lds_barrier = []() {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
    };
#pragma unroll
    for (int r = 0; r < VPT; ++r) {
        const int j = r * kM64Threads + tq;
        int dj = 0;
#pragma unroll
        for (int h = 0; h < kMlDC / 2; ++h) {
            uint32_t e0 = 0xffffu, e1 = 0xffffu;
            if (j < n) {
                e0 = etab[(size_t)(2 * h) * n + j];
                e1 = etab[(size_t)(2 * h + 1) * n + j];
            }
            dj += (e0 != 0xffffu) + (e1 != 0xffffu);
            e0 = e0 == 0xffffu ? 0u : e0;  // state slots (m64_etab)
            e1 = e1 == 0xffffu ? 0u : e1;
            ep[r][h] = e0 | (e1 << 16);
        }
        djs |= (uint32_t)dj << (3 * r);
        __builtin_amdgcn_sched_barrier(0);  // one variable's loads at a time (registers)
    }
    auto chk = [&](int r, int k) -> int { return (int)((ep[r][k >> 1] >> (16 * (k & 1))) & 0xffffu); };
    auto deg = [&](int r) -> int { return (int)((djs >> (3 * r)) & 7u); };
    auto dmax = [](int r) -> int { return r < D3R ? kMlDC - 1 : kMlDC; };  // compile time once unrolled
    // keeps the per-edge addresses from being hoisted out of the loops (as in
    // bp_ms_lds_kernel): they are re-derived from ep where used
    auto opaque_edges = [&]() {
#pragma unroll
        for (int r = 0; r < VPT; ++r)
#pragma unroll
            for (int h = 0; h < kMlDC / 2; ++h) asm volatile("" : "+v"(ep[r][h]));
        asm volatile("" : "+v"(djs));
    };
    // ldpc's (v <= 0) for a v2c message (never -0)
    auto neg = [](double v) -> uint32_t { return (uint32_t)((dbits(v) - 1ull) >> 63); };
    // one new message (magnitude bits x) into the minima of check slot i, buffer nb
    auto put_min = [&](int nb, int i, unsigned long long x) {
        const unsigned long long old = atomicMin(st + (size_t)nb * m + i, x);
        atomicMin(st + (size_t)(2 + nb) * m + i, old > x ? old : x);
    };

    QDEC_STAMP_DECL
    if (tid == 0) *next = (long long)atomicAdd(a.wave_ctr, 1ull);
    __syncthreads();
    for (;;) {
        const long long sl = *next;  // uniform: held in SGPRs
        const int64_t shot = (int64_t)((unsigned long long)__builtin_amdgcn_readfirstlane((unsigned)sl) |
                                       ((unsigned long long)__builtin_amdgcn_readfirstlane((unsigned)(sl >> 32)) << 32));
        if (shot >= a.B) break;
        QDEC_STAMP(4);
        QDEC_COUNT(8, 1);
        // the next shot's index, fetched under this shot's syndrome loads (stored
        // behind the barrier below, after every thread has read this one)
        // (an opaque offset keeps the atomic optimiser, which would wait for the
        // result right away, off this single-lane add)
        long long shot_next = 0;
        if (tid == 0) {
            int z = 0;
            asm volatile("" : "+v"(z));
            shot_next = (long long)atomicAdd(a.wave_ctr + z, 1ull);
        }
        const int to = opaque_tid();
        // ---- S: syndrome words (ballots of 64 consecutive slots); buffer 0 reset,
        // buffer 1 = iteration 1's states (img).  The kM64Nch syndrome loads of a
        // thread and its image loads are issued together (clamped index, masked).
        uint32_t sv[kM64Nch], ip[kM64Nch];
        unsigned long long i1[kM64Nch], i2[kM64Nch];
        const uint32_t* ipar = reinterpret_cast<const uint32_t*>(img + (size_t)2 * m);
        const int ln = to & 63, wbase = to & ~63;
#pragma unroll
        for (int c = 0; c < kM64Nch; ++c) {
            const int i = c * kM64Threads + to, ic = min(i, m - 1);
            sv[c] = a.syn[shot * m + cslot[ic]] & (i < m ? 1u : 0u);
            i1[c] = img[ic];
            i2[c] = img[(size_t)m + ic];
            ip[c] = ipar[min(((c * kM64Threads + wbase) >> 5) + (ln & 1), W - 1)];
        }
#pragma unroll
        for (int c = 0; c < kM64Nch; ++c) {
            const int i = c * kM64Threads + to;
            if (i < m) {
                st[i] = kBig;
                st[(size_t)m + i] = i1[c];
                st[(size_t)2 * m + i] = kBig;
                st[(size_t)3 * m + i] = i2[c];
            }
            const unsigned long long bw = __ballot(sv[c] != 0u);
            const int w0 = (c * kM64Threads + wbase) >> 5;
            if (ln < 2 && w0 + ln < W) {
                const uint32_t word = (uint32_t)(bw >> (32 * ln));
                synw[w0 + ln] = word;
                parw[w0 + ln] = word;
                parw[W + w0 + ln] = word ^ ip[c];
            }
        }
        for (int w = to; w < W; w += kM64Threads) hdw[w] = hdw[W + w] = 0u;
        lds_barrier();
        QDEC_STAMP(0);
        if (tid == 0) *next = shot_next;
        double v[VPT][kMlDC];
        {
            const int tq0 = opaque_tq();
#pragma unroll
            for (int r = 0; r < VPT; ++r) {
                const double Lr = prior_of(prior, tq0, r);
#pragma unroll
                for (int k = 0; k < kMlDC; ++k) v[r][k] = Lr;
            }
        }

        uint32_t xb = 0, bad = 0;  // hard decisions (bit r), failing owned checks (bit c)
        bool conv = false;
        int it = 1;
        for (;; ++it) {
            const int b = it & 1, nb = b ^ 1;
            const double alpha = alpha_at<double>(it, a.ms_scaling);
            // ---- D: c2v from buffer b, sums, hard decision, new v2c -> buffer nb
            xb = 0;
            opaque_edges();
            int pz = 0;
            asm volatile("" : "+s"(pz));  // the prior loads stay in the loop (global, not flat)
            const double* pr = prior + pz;
            const int tqv = opaque_tq();
#pragma unroll
            for (int r = 0; r < VPT; ++r) {
                const int dj = deg(r);
                const double Lr = prior_of(pr, tqv, r);
                double c[kMlDC];
#pragma unroll
                for (int k = 0; k < kMlDC; ++k) {
                    c[k] = 0.0;
                    if (k < dmax(r) && k < dj) {
                        const int i = chk(r, k);
                        const unsigned long long* s = st + (size_t)b * m + i;
                        const unsigned long long m1 = s[0], m2 = s[2 * (size_t)m];
                        const uint32_t pw = parw[b * W + (i >> 5)];
                        const unsigned long long vb = dbits(v[r][k]);
                        const double y = __longlong_as_double((long long)((vb & kAbs) == m1 ? m2 : m1)) * alpha;
                        const uint32_t sg = ((pw >> (i & 31)) ^ (uint32_t)((vb - 1ull) >> 63)) & 1u;
                        c[k] = __longlong_as_double((long long)(dbits(y) ^ ((unsigned long long)sg << 63)));
                    }
                    __builtin_amdgcn_sched_barrier(0);  // one edge's state in flight (registers; issuing a
                                                        // column's reads together measured the same, profiles/r06ab,
                                                        // profiles/r06c4/ab_edge_batch)
                }
                // ldpc's order: prefix sums from the prior, then each outgoing
                // message = prefix + (sum of the later edges, accumulated from the end)
                double pre[kMlDC];
                double acc = Lr;
#pragma unroll
                for (int k = 0; k < kMlDC; ++k) {
                    pre[k] = acc;
                    acc = (k < dmax(r) && k < dj) ? acc + c[k] : acc;
                }
                const bool x = acc <= 0.0;
                xb |= (uint32_t)x << r;
                double suf = 0.0;
                bool started = false;
#pragma unroll
                for (int k = kMlDC - 1; k >= 0; --k) {
                    if (k >= dmax(r)) continue;
                    const double o = started ? pre[k] + suf : pre[k];
                    suf = started ? suf + c[k] : c[k];
                    started = started || k < dj;
                    if (k < dj) {
                        v[r][k] = o;
                        const int i = chk(r, k);
                        put_min(nb, i, dbits(o) & kAbs);  // (every ds_min_rtn of the column first, then
                                                          // the m2 updates: spills, 11 % slower, r06c4)
                        if (neg(o)) atomicXor(&parw[nb * W + (i >> 5)], 1u << (i & 31));
                        if (x) atomicXor(&hdw[b * W + (i >> 5)], 1u << (i & 31));
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            __syncthreads();
            QDEC_STAMP(1);
            QDEC_COUNT(9, 1);
            // ---- B: syndrome test of iteration it; reset of buffer b
            bad = 0;
            for (int c = 0; c < ncr; ++c) {
                const int i = c * kM64Threads + tid;
                bad |= (((hdw[b * W + (i >> 5)] ^ synw[i >> 5]) >> (i & 31)) & 1u) << c;
            }
            const unsigned long long wb = __ballot(bad != 0u);
            if (lane == 0) flags[b * (kM64Threads / 64) + wv] = wb != 0ull;
            for (int i = tid; i < m; i += kM64Threads) {
                st[(size_t)b * m + i] = kBig;
                st[(size_t)(2 + b) * m + i] = kBig;
            }
            for (int w = tid; w < W; w += kM64Threads) {
                parw[b * W + w] = synw[w];
                hdw[nb * W + w] = 0u;
            }
            __syncthreads();
            int any_bad = 0;
#pragma unroll
            for (int w = 0; w < kM64Threads / 64; ++w) any_bad |= flags[b * (kM64Threads / 64) + w];
            QDEC_STAMP(2);
            if (!any_bad) {
                conv = true;
                break;
            }
            if (it >= a.max_iter) break;
        }
        // ---- queue the shot: hard decision, residual syndrome, converged bit.
        // The bytes are staged in LDS (the state arrays are free after the last
        // B barrier) in column / check order and leave as whole lines: written
        // directly, the lanes' columns 67 apart and the slot-ordered checks put
        // every lane of a store in its own line.
        {
            uint8_t* sx = reinterpret_cast<uint8_t*>(st);  // [n] hard decisions
            uint8_t* sr = sx + ((n + 15) & ~15);            // [m] residual syndrome
            const int tqs = opaque_tq(), tt = opaque_tid();
            int ck[kM64Nch];
#pragma unroll
            for (int c = 0; c < kM64Nch; ++c) ck[c] = cslot[min(c * kM64Threads + tt, m - 1)];
#pragma unroll
            for (int r = 0; r < VPT; ++r) {
                const int j = r * kM64Threads + tqs;
                if (j < n) sx[j] = (uint8_t)((xb >> r) & 1);
            }
#pragma unroll
            for (int c = 0; c < kM64Nch; ++c)
                if (c * kM64Threads + tt < m) sr[ck[c]] = (uint8_t)((bad >> c) & 1);
            lds_barrier();
            auto copy_row = [&](uint8_t* dst, const uint8_t* src, int len) {
                if ((((uintptr_t)dst | (uintptr_t)len) & 3) == 0) {
                    for (int w = tt; w < len / 4; w += kM64Threads)
                        reinterpret_cast<uint32_t*>(dst)[w] = reinterpret_cast<const uint32_t*>(src)[w];
                } else {
                    for (int j = tt; j < len; j += kM64Threads) dst[j] = src[j];
                }
            };
            copy_row(a.q_x + shot * n, sx, n);
            copy_row(a.q_r + shot * m, sr, m);
            if (tid == 0) {
                a.q_idx[shot] = shot | ((int64_t)(conv ? 1 : 0) << 62);
                if (a.iters) a.iters[shot] = conv ? it : a.max_iter;
            }
            lds_barrier();  // the staged bytes are read before the next shot's S phase writes
        }
        QDEC_STAMP(3);
    }
    QDEC_FLUSH_AT(16);
}

// slots 16.. of bp_ms_lds64_kernel (tools/dev/stamps_c4.py)
QDEC_STAMPS_READER(read_stamps_ms_lds64)

using Lds64Sig = KernelSig<DevGraph, DecodeArgs, const uint16_t*, const double*, const uint16_t*,
                           const unsigned long long*>;

// bp_ms_lds64_kernel VPT, D3R (columns per thread, leading column rounds of degree <= 3)
void add_ms_lds64_kernels(KernelTable& t) {
    t = {QDEC_INST(kM64Threads, bp_ms_lds64_kernel, 4, 0),  QDEC_INST(kM64Threads, bp_ms_lds64_kernel, 8, 0),
         QDEC_INST(kM64Threads, bp_ms_lds64_kernel, 8, 4),  QDEC_INST(kM64Threads, bp_ms_lds64_kernel, 10, 0),
         QDEC_INST(kM64Threads, bp_ms_lds64_kernel, 10, 3), QDEC_INST(kM64Threads, bp_ms_lds64_kernel, 10, 6)};
    for (KernelEntry& e : t) e.lds = [](const DevGraph& g, const DecodeArgs&) { return m64_lds_bytes(g); };
}

// The BP stage: iteration 1's image into `img` by the init kernel, then the
// plan's entry.  The caller runs the SSF / finalize kernel behind it.
int launch_ms_lds64(const DevGraph& g, const DecodePlan& p, const DecodeArgs& a, int num_cus, hipStream_t stream,
                  unsigned long long* img, size_t img_bytes) {
    const size_t lds = p.bp_k->lds(g, a);
    long long grid = 0;
    hipError_t e = resident_grid(p.bp_k->fn, p.bp_k->block, lds, num_cus, a.B, &grid);
    if (e != hipSuccess) return (int)e;
    e = hipMemsetAsync(a.wave_ctr, 0, sizeof(unsigned long long), stream);  // shot counter
    if (e != hipSuccess) return (int)e;
    if (!img || img_bytes < m64_image_bytes(g)) return (int)hipErrorInvalidValue;
    const double* prior = reinterpret_cast<const double*>(g.prior[1][0]);
    hipLaunchKernelGGL(m64_init_kernel, dim3((unsigned)((g.m + 255) / 256)), dim3(256), 0, stream, g, prior,
                       g.m64_check, img);
    record_ev(a, 0, stream);
    last_launch_names().bp = noted_name(p.bp_k);
    const int le = launch_entry(Lds64Sig{}, *p.bp_k, grid, lds, stream, g, a, g.m64_etab, prior, g.m64_check, img);
    record_ev(a, 1, stream);
    return le;
}

}  // namespace qdec
