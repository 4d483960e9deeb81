// qdec_ms_lds.hip -- bp_ms_lds_kernel: LDS-resident min-sum BP, f32.
//
// Min-sum BP (fp32) for graphs whose messages spill the small-graph LDS budget
// but whose edge slots alone fit one CU's 160 KB LDS (config 4: m = 4800 rows of
// kMlDRS = 8 floats = 150 KB).  One 1024-thread workgroup per CU decodes one
// shot at a time with every message on chip:
//   rows   [m][kMlDRS] f32: one slot per edge at (row, position); it holds the
//          edge's v2c message between the variable pass and the check pass and
//          its c2v message between the check pass and the variable pass
//   pbuf   two bit arrays of m bits: parity of the hard decision per check,
//          built by the variable pass with LDS xor atomics (only ones touch it)
// Thread t owns checks t + 1024 c and variables t + 1024 r.  Per iteration (2
// barriers):
//   A  check pass: syndrome test of the previous iteration's hard decision
//      (parity bits vs syndrome); each owned row reads its v2c slots (two
//      16-B halves), takes m1 / m2 (minimum and second minimum of |v|, counted
//      with multiplicity), the argmin position and the parity, and writes every
//      slot's c2v: alpha * (m2 at the argmin, m1 elsewhere) with sign parity ^
//      (own v2c <= 0) -- ldpc's leave-one-out minimum and sign, bit for bit
//      (when the minimum is tied m2 = m1, so the argmin's choice is immaterial)
//   B  barrier-or: all checks satisfied -> converged at it - 1
//   C  variable pass: read the c2v slots, prefix / suffix sums (ldpc's order),
//      hard decision, parity xors, and the new v2c written back into the same
//      slots at once (a slot is read and written by its own variable only)
//   D  barrier
// Finished shots go to the SSF queue in the byte format of the other BP kernels (hard
// decision, residual, converged bit); ssf_inc_block_kernel runs SSF and finalises.
// Pad edges (k >= the column's degree, variables j >= n) point at dummy rows
// past row m (element m * kMlDRS + lane, so no two lanes of a wave write the
// same address): they read garbage that the sums mask out and write into them,
// so the loops have no per-edge branches; only real edges xor parity.
#include <hip/hip_runtime.h>

#include "qdec_block_layout.h"
#include "qdec_device.h"
#include "qdec_kernels.h"

namespace qdec {

// Step A of bp_ms_lds_kernel on row i, in place (v2c slots in, c2v slots out);
// also ml_init_check_kernel's iteration 1 on the image in HBM.
__device__ __forceinline__ void ml_check_row(float* rows, int i, int deg, uint32_t sbit, float alpha) {
    // the row's halves in swizzled order (so = 4 * bit 4 of the row): the 16-B
    // reads of a 16-lane group (banks a/4 mod 64) and the 16-B writes of an
    // 8-lane group (banks a/4 mod 32) then land in distinct 4-bank slots; loaded
    // element u sits at row position u ^ so
    const int so = ((i >> 4) & 1) << 2;
    float v[kMlDRS];
    {
        const float4 h0 = *reinterpret_cast<const float4*>(rows + (size_t)i * kMlDRS + so);
        const float4 h1 = *reinterpret_cast<const float4*>(rows + (size_t)i * kMlDRS + (so ^ 4));
        v[0] = h0.x, v[1] = h0.y, v[2] = h0.z, v[3] = h0.w;
        v[4] = h1.x, v[5] = h1.y, v[6] = h1.z, v[7] = h1.w;
    }
    // sign test by bits: bit 31 of bits(v) - 1 is (v <= 0) for every v but -0,
    // and a v2c message is never -0 (the prior is not, and a sum is -0 only when
    // both terms are)
    float m1 = Big<float>::v, m2 = Big<float>::v;
    int au = 0;  // element index of the argmin
    uint32_t sx = sbit << 31;
    uint32_t sg[kMlDRS];
#pragma unroll
    for (int u = 0; u < kMlDRS; ++u) {
        const float vt = (u ^ so) < deg ? v[u] : Big<float>::v;
        const float av = fabsf(vt);
        au = av < m1 ? u : au;
        m2 = med3(av, m1, m2);
        m1 = med3(av, m1, -Big<float>::v);
        sg[u] = (uint32_t)__float_as_int(vt) - 1u;
        sx ^= sg[u];
    }
    // c2v of every position, in place of its v2c: alpha times the leave-one-out
    // minimum (m2 at the argmin, m1 elsewhere), sign = syndrome ^ the other
    // edges' signs = bit 31 of sx ^ sg[u]
    const float y1 = m1 * alpha, y2 = m2 * alpha;
    float o[kMlDRS];
#pragma unroll
    for (int u = 0; u < kMlDRS; ++u) {
        const float y = u == au ? y2 : y1;
        o[u] = __uint_as_float(__float_as_uint(y) ^ ((sg[u] ^ sx) & 0x80000000u));
    }
    *reinterpret_cast<float4*>(rows + (size_t)i * kMlDRS + so) = make_float4(o[0], o[1], o[2], o[3]);
    *reinterpret_cast<float4*>(rows + (size_t)i * kMlDRS + (so ^ 4)) = make_float4(o[4], o[5], o[6], o[7]);
}

// Iteration 1's c2v rows depend on the priors and, through one sign per row, on
// the syndrome: the image (rows of `ml_lds_bytes`' layout, m x kMlDRS f32 in
// HBM, syndrome bit 0) is built once per launch -- the priors scattered to the
// edge slots, then step A on every row -- and each shot copies it, flipping
// every sign of the rows whose syndrome bit is 1 (step A's sx carries that bit
// into all of a row's signs).  The image's unused row positions are never read
// (step A masks positions >= the degree, and pad edges use the dummy rows).
__global__ __launch_bounds__(256) void ml_init_scatter_kernel(DevGraph g, const uint16_t* __restrict__ etab,
                                                             const float* __restrict__ prior, float* __restrict__ img) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= g.n) return;
    const float L = prior[j];
#pragma unroll
    for (int k = 0; k < kMlDC; ++k) {
        const uint32_t e = etab[(size_t)k * g.n + j];
        if (e != 0xffffu) img[e] = L;
    }
}

__global__ __launch_bounds__(256) void ml_init_check_kernel(DevGraph g, float* __restrict__ img, double ms_scaling) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= g.m) return;
    ml_check_row(img, i, g.row_ptr[i + 1] - g.row_ptr[i], 0u, alpha_at<float>(1, ms_scaling));
}

template <int VPT>
__global__ __launch_bounds__(kMlThreads) void bp_ms_lds_kernel(DevGraph g, DecodeArgs a,
                                                              const uint16_t* __restrict__ etab,
                                                              const float* __restrict__ prior,
                                                              const float* __restrict__ img) {
    static_assert(VPT * 3 <= 64 && VPT <= 32, "degree and decision bits");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    long long* next = reinterpret_cast<long long*>(smem + kCtrlNext);
    float* rows = reinterpret_cast<float*>(smem + kCtrl);
    const int tid = threadIdx.x;
    const int m = g.m, n = g.n;
    const int npw = (m + kMlDummyRows + 31) / 32;
    const uint32_t pbw = (uint32_t)ml_pbuf_words(g);
    uint32_t* pb0 = reinterpret_cast<uint32_t*>(rows + ((size_t)m + kMlDummyRows) * kMlDRS);
    int* flags = reinterpret_cast<int*>(pb0 + 2 * pbw);  // [2][16]
    const uint32_t pad0 = (uint32_t)m * kMlDRS;        // first dummy element
    const uint32_t pad = pad0 + (uint32_t)(tid & 63);  // this lane's (distinct banks, no same-address writes)
    const int ncr = (m - tid + kMlThreads - 1) / kMlThreads;  // checks of this thread (<= 32)
    if (blockIdx.x == 0 && tid == 0) *a.q_count = (int32_t)a.B;

    // per-variable constants: prior, degree, LDS element of each edge (u16 pairs)
    float L[VPT];
    uint32_t ep[VPT][kMlDC / 2];
#pragma unroll
    for (int r = 0; r < VPT; ++r) {
        const int j = r * kMlThreads + tid;
        L[r] = j < n ? prior[j] : 0.0f;
#pragma unroll
        for (int h = 0; h < kMlDC / 2; ++h) {
            uint32_t e0 = pad, e1 = pad;
            if (j < n) {
                e0 = etab[(size_t)(2 * h) * n + j];
                e1 = etab[(size_t)(2 * h + 1) * n + j];
                e0 = e0 == 0xffffu ? pad : e0;
                e1 = e1 == 0xffffu ? pad : e1;
            }
            ep[r][h] = e0 | (e1 << 16);
        }
    }
    auto edge = [&](int r, int k) -> uint32_t { return (ep[r][k >> 1] >> (16 * (k & 1))) & 0xffffu; };
    // Keeps the compiler from hoisting the per-edge addresses, positions and
    // parity masks derived from ep out of the iteration loop (5 live values per
    // edge instead of half a register): they are re-derived where used.
    auto opaque_edges = [&]() {
#pragma unroll
        for (int r = 0; r < VPT; ++r)
#pragma unroll
            for (int h = 0; h < kMlDC / 2; ++h) asm volatile("" : "+v"(ep[r][h]));
    };
    uint64_t djs = 0;  // 3 bits per owned variable: its degree (real edges come first)
#pragma unroll
    for (int r = 0; r < VPT; ++r) {
        int dj = 0;
#pragma unroll
        for (int k = 0; k < kMlDC; ++k) dj += edge(r, k) < pad0;
        djs |= (uint64_t)dj << (3 * r);
    }
    uint32_t rdeg = 0;  // 4 bits per owned check (degrees <= 8), checks c < 8
    for (int c = 0; c < ncr && c < 8; ++c) {
        const int i = c * kMlThreads + tid;
        rdeg |= (uint32_t)(g.row_ptr[i + 1] - g.row_ptr[i]) << (4 * c);
    }

    // The next shot's index is fetched under this shot's syndrome loads and
    // stored behind the barrier below (every thread has read this one by then);
    // the barriers of the shot's iterations order it before the next read.  The
    // syndrome loads of a thread are issued together (kMlNch, clamped, masked),
    // and the barrier orders LDS only, so the last shot's queue stores stay in
    // flight (a __syncthreads would wait for them).
    if (tid == 0) *next = (long long)atomicAdd(a.wave_ctr, 1ull);
    __syncthreads();
    for (;;) {
        const long long sl = *next;  // uniform: held in SGPRs
        const int64_t shot = (int64_t)((unsigned long long)__builtin_amdgcn_readfirstlane((unsigned)sl) |
                                       ((unsigned long long)__builtin_amdgcn_readfirstlane((unsigned)(sl >> 32)) << 32));
        if (shot >= a.B) break;
        long long shot_next = 0;
        if (tid == 0) {
            int z = 0;  // opaque offset: keeps the atomic optimiser (which waits at once) off
            asm volatile("" : "+v"(z));
            shot_next = (long long)atomicAdd(a.wave_ctr + z, 1ull);
        }
        int to = tid;
        asm volatile("" : "+v"(to));  // per-shot addresses re-derived, not hoisted and spilled
        uint32_t sb = 0;  // syndrome bits of the owned checks
#pragma unroll
        for (int c = 0; c < kMlNch; ++c) {
            const int i = c * kMlThreads + to;
            sb |= (uint32_t)(a.syn[shot * m + min(i, m - 1)] & (i < m ? 1u : 0u)) << c;
        }
        // iteration 1's c2v rows: the image, signs flipped where the syndrome bit
        // is 1; the parity bits of iteration 1 cleared
#pragma unroll
        for (int c = 0; c < kMlNch; ++c) {
            const int i = c * kMlThreads + to;
            if (i < m) {
                const uint32_t f = ((sb >> c) & 1u) << 31;
                const uint4 h0 = *reinterpret_cast<const uint4*>(img + (size_t)i * kMlDRS);
                const uint4 h1 = *reinterpret_cast<const uint4*>(img + (size_t)i * kMlDRS + 4);
                *reinterpret_cast<uint4*>(rows + (size_t)i * kMlDRS) = make_uint4(h0.x ^ f, h0.y ^ f, h0.z ^ f, h0.w ^ f);
                *reinterpret_cast<uint4*>(rows + (size_t)i * kMlDRS + 4) = make_uint4(h1.x ^ f, h1.y ^ f, h1.z ^ f, h1.w ^ f);
            }
        }
        for (int w = to; w < npw; w += kMlThreads) pb0[pbw + w] = 0u;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
        if (tid == 0) *next = shot_next;

        uint32_t xb = 0, bad = 0;  // hard decisions (bit r), failing owned checks (bit c)
        bool conv = false;
        int it = 1;
        for (;; ++it) {
            // ---- A: test of iteration it - 1, then the c2v messages of iteration it
            // (iteration 1's came from the image)
            uint32_t* pcur = pb0 + (it & 1) * pbw;
            if (it > 1) {
                const uint32_t* pprev = pb0 + ((it - 1) & 1) * pbw;
                const bool work = it <= a.max_iter;
                const float alpha = alpha_at<float>(it, a.ms_scaling);
                bad = 0;
                for (int c = 0; c < ncr; ++c) {
                    const int i = c * kMlThreads + tid;
                    bad |= (((pprev[i >> 5] >> (i & 31)) ^ (sb >> c)) & 1u) << c;
                    if (work) {
                        const int deg = c < 8 ? (int)((rdeg >> (4 * c)) & 15u) : (g.row_ptr[i + 1] - g.row_ptr[i]);
                        ml_check_row(rows, i, deg, (sb >> c) & 1u, alpha);
                    }
                }
                if (work)
                    for (int w = tid; w < npw; w += kMlThreads) pcur[w] = 0u;
                // block-wide "any check failing": one flag per wave, double-buffered by
                // iteration parity so one barrier suffices
                int* fl = flags + (it & 1) * (kMlThreads / 64);
                const unsigned long long wb = __ballot(bad != 0u);
                if ((tid & 63) == 0) fl[tid >> 6] = wb != 0ull;
                __syncthreads();
                int any_bad = 0;
#pragma unroll
                for (int w = 0; w < kMlThreads / 64; ++w) any_bad |= fl[w];
                if (!any_bad) {
                    conv = true;
                    break;
                }
                if (!work) break;
            }
            // ---- C: variable pass.  Each edge's slot is read and rewritten by its
            // own variable only (c2v in, new v2c out), so no barrier separates them
            opaque_edges();
            xb = 0;
            // software-pipelined by one variable: the next variable's slots are
            // read before this one's arithmetic (distinct slots, so the order
            // against this variable's writes is immaterial)
            float cn[kMlDC];
#pragma unroll
            for (int k = 0; k < kMlDC; ++k) cn[k] = rows[edge(0, k)];
#pragma unroll
            for (int r = 0; r < VPT; ++r) {
                const int dj = (int)((djs >> (3 * r)) & 7u);  // degree: real edges come first
                float c[kMlDC];
#pragma unroll
                for (int k = 0; k < kMlDC; ++k) c[k] = cn[k];
                if (r + 1 < VPT)
#pragma unroll
                    for (int k = 0; k < kMlDC; ++k) cn[k] = rows[edge(r + 1, k)];
                // ldpc's order: prefix sums from the prior, then each outgoing
                // message = prefix + (sum of the later edges, accumulated from the end)
                float pre[kMlDC];
                float acc = L[r];
#pragma unroll
                for (int k = 0; k < kMlDC; ++k) {
                    pre[k] = acc;
                    acc = k < dj ? acc + c[k] : acc;
                }
                const bool x = acc <= 0.0f;
                xb |= (uint32_t)x << r;
                float suf = 0.0f;
                bool started = false;
#pragma unroll
                for (int k = kMlDC - 1; k >= 0; --k) {
                    const float o = started ? pre[k] + suf : pre[k];
                    suf = started ? suf + c[k] : c[k];
                    started = started || k < dj;
                    rows[edge(r, k)] = o;
                }
                if (x) {
#pragma unroll
                    for (int k = 0; k < kMlDC; ++k) {
                        const uint32_t i = edge(r, k) / kMlDRS;
                        if (k < dj) atomicXor(&pcur[i >> 5], 1u << (i & 31));
                    }
                }
                // two variables' reads in flight at most (otherwise the
                // scheduler hoists all of them and spills)
                __builtin_amdgcn_sched_barrier(0);
            }
            __syncthreads();
        }
        // ---- queue the shot: hard decision, residual syndrome, converged bit
#pragma unroll
        for (int r = 0; r < VPT; ++r) {
            const int j = r * kMlThreads + tid;
            if (j < n) a.q_x[shot * n + j] = (uint8_t)((xb >> r) & 1);
        }
        for (int c = 0; c < ncr; ++c) a.q_r[shot * m + c * kMlThreads + tid] = (uint8_t)((bad >> c) & 1);
        if (tid == 0) {
            a.q_idx[shot] = shot | ((int64_t)(conv ? 1 : 0) << 62);
            if (a.iters) a.iters[shot] = conv ? it - 1 : a.max_iter;
        }
    }
}

using LdsSig = KernelSig<DevGraph, DecodeArgs, const uint16_t*, const float*, const float*>;

// bp_ms_lds_kernel VPT (columns per thread)
void add_ms_lds_kernels(KernelTable& t) {
    t = {QDEC_INST(kMlThreads, bp_ms_lds_kernel, 4), QDEC_INST(kMlThreads, bp_ms_lds_kernel, 8),
         QDEC_INST(kMlThreads, bp_ms_lds_kernel, 10), QDEC_INST(kMlThreads, bp_ms_lds_kernel, 12),
         QDEC_INST(kMlThreads, bp_ms_lds_kernel, 16)};
    for (KernelEntry& e : t) e.lds = [](const DevGraph& g, const DecodeArgs&) { return ml_lds_bytes(g); };
}

// The BP stage: iteration 1's image into `img` by the init kernels, then the
// plan's entry.  The caller runs the SSF / finalize kernel behind it.
int launch_ms_lds(const DevGraph& g, const DecodePlan& p, const DecodeArgs& a, int num_cus, hipStream_t stream,
                  float* img, size_t img_bytes) {
    const size_t lds = p.bp_k->lds(g, a);
    long long grid = 0;
    hipError_t e = resident_grid(p.bp_k->fn, p.bp_k->block, lds, num_cus, a.B, &grid);
    if (e != hipSuccess) return (int)e;
    if (!img || img_bytes < ml_image_bytes(g)) return (int)hipErrorInvalidValue;
    e = hipMemsetAsync(a.wave_ctr, 0, sizeof(unsigned long long), stream);  // shot counter
    if (e != hipSuccess) return (int)e;
    const float* prior = reinterpret_cast<const float*>(g.prior[1][1]);
    hipLaunchKernelGGL(ml_init_scatter_kernel, dim3((unsigned)((g.n + 255) / 256)), dim3(256), 0, stream, g, g.ml_etab,
                       prior, img);
    hipLaunchKernelGGL(ml_init_check_kernel, dim3((unsigned)((g.m + 255) / 256)), dim3(256), 0, stream, g, img,
                       a.ms_scaling);
    record_ev(a, 0, stream);
    last_launch_names().bp = noted_name(p.bp_k);
    const int le = launch_entry(LdsSig{}, *p.bp_k, grid, lds, stream, g, a, g.ml_etab, prior, img);
    record_ev(a, 1, stream);
    return le;
}

}  // namespace qdec
