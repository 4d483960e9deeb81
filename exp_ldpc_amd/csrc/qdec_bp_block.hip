// qdec_bp_block.hip -- BP + SSF for graphs outside the wave kernels' shapes
// (multi-round spacetime matrices with R >= 2, codes with n > 576, degrees > 8/4).
//
// One 256-thread workgroup decodes one shot at a time (persistent grid).  Graph
// tables are read from global memory (CSR row_ptr/col_idx, CSC col_ptr/col_edge;
// L1/L2 resident, shared by every workgroup).  Messages are indexed by CSR edge
// id: v2c[E], c2v[E] live in LDS when 2*E*sizeof(T) fits, otherwise in a
// per-workgroup slice of an HBM scratch buffer (the HBM-bound regime of the 10k
// and 50k qubit configurations).  The loops are ldpc v1's, operation for
// operation (same arithmetic as the wave kernels and oracle/bp_impl.inc):
//   check pass: thread per check, forward/backward along the row
//   variable pass: thread per variable, prefix then suffix along the column
// Small-set-flip runs in ssf_block_kernel on the same HBM work queue as the wave
// path, with generators spread over the workgroup's threads.
#include <hip/hip_runtime.h>

#include "qdec_block_steps.h"
#include "qdec_kernels.h"

namespace qdec {

// dst[0..len) = src[0..len) (byte arrays, thread-strided), eight loads per
// thread issued before the stores; returns this thread's sum of the bytes
__device__ __forceinline__ int copy_bytes8(const uint8_t* src, uint8_t* dst, int len, int tid) {
    int sum = 0;
    for (int j0 = tid; j0 < len; j0 += 8 * kBlock) {
        uint8_t v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = j0 + u * kBlock < len ? src[j0 + u * kBlock] : (uint8_t)0;
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (j0 + u * kBlock < len) {
                dst[j0 + u * kBlock] = v[u];
                sum += v[u];
            }
    }
    return sum;
}

// Outputs of one shot from its hard decision xh (LDS): x_out, corr = base ^
// fold(xh), fail = any_r parity(lz[r] & (readout ^ corr)) (per-thread word parities
// xor-reduced into LDS), status, ssf_steps.
__device__ void finalize_block(const DevGraph& g, const DecodeArgs& a, int64_t shot, const uint8_t* xh, bool conv,
                               bool satisfied, int steps, int* lpar /* LDS [k] */,
                               const uint8_t* rd_lds = nullptr /* LDS copy of the shot's readout, or null */) {
    const int tid = threadIdx.x;
    auto rd = [&](int q) -> uint8_t { return rd_lds ? rd_lds[q] : a.readout[shot * g.n_data + q]; };
    if (a.x_out)
        for (int j = tid; j < g.n; j += kBlock) a.x_out[shot * g.n + j] = xh[j];
    const bool want_fail = a.fail && a.readout && g.k > 0;
    if (want_fail)
        for (int r = tid; r < g.k; r += kBlock) lpar[r] = 0;
    __syncthreads();
    // by qubit (DevGraph::lz_t): lpar holds lz_tw parity words; each residual one
    // XORs its qubit's words in
    const bool cols = want_fail && g.lz_t;
    const bool walk = want_fail && !cols && g.lz_sparse;
    if (cols) {
        uint32_t* lw = reinterpret_cast<uint32_t*>(lpar);  // lz_tw <= k words, zeroed above
        const int nd = g.n_data, tw = g.lz_tw;
        for (int q0 = tid; q0 < nd; q0 += 8 * kBlock) {
            uint8_t rv[8], bv[8];  // eight qubits per round, their loads first
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int q = q0 + u * kBlock;
                rv[u] = q < nd ? rd(q) : (uint8_t)0;
                bv[u] = (q < nd && a.base) ? a.base[shot * nd + q] : (uint8_t)0;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int q = q0 + u * kBlock;
                if (q >= nd) break;
                int cb = bv[u] & 1;
                for (int t = 0; t < g.fold_blocks; ++t) cb ^= xh[t * nd + q];
                if (a.corr_out) a.corr_out[shot * nd + q] = (uint8_t)cb;
                if ((rv[u] ^ cb) & 1)
                    for (int t = 0; t < tw; ++t) {
                        const uint32_t v = g.lz_t[(size_t)q * tw + t];
                        if (v) atomicXor(&lw[t], v);
                    }
            }
        }
    }
    if (walk) {  // sparse logicals: each thread tests whole logicals on their supports
        for (int r = tid; r < g.k; r += kBlock) {
            int par = 0;
            for (int t = g.lz_ptr[r]; t < g.lz_ptr[r + 1]; ++t) {
                const int q = g.lz_idx[t];
                int cb = rd(q) ^ (a.base ? a.base[shot * g.n_data + q] : 0);
                for (int b = 0; b < g.fold_blocks; ++b) cb ^= xh[b * g.n_data + q];
                par ^= cb & 1;
            }
            lpar[r] = par;
        }
    }
    if (a.corr_out && !cols && (!want_fail || walk)) {
        for (int q = tid; q < g.n_data; q += kBlock) {
            int cb = a.base ? (a.base[shot * g.n_data + q] & 1) : 0;
            for (int t = 0; t < g.fold_blocks; ++t) cb ^= xh[t * g.n_data + q];
            a.corr_out[shot * g.n_data + q] = (uint8_t)cb;
        }
    } else if (want_fail && !cols && !walk) {
        // dense logicals, kBlock words at a time: wave w builds words
        // base + 64 w + i (i < 64) by ballots over coalesced byte reads and lane
        // i keeps word i; then per logical r each lane ANDs its word with the
        // row's (a coalesced load across the lanes), the wave folds the parities
        // with one ballot, and one LDS XOR per wave and row accumulates them
        const int lane = tid & 63, wv = tid >> 6;
        for (int wbase = 0; wbase < g.lz_words; wbase += kBlock) {
            unsigned long long mine = 0ull;
            for (int i0 = 0; i0 < 64; i0 += 8) {
                if (wbase + wv * 64 + i0 >= g.lz_words) break;  // uniform
                // eight words per round: their readout / base bytes loaded first
                uint8_t rv[8], bv[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int q = (wbase + wv * 64 + i0 + u) * 64 + lane;
                    const bool in = q < g.n_data && wbase + wv * 64 + i0 + u < g.lz_words;
                    rv[u] = in ? rd(q) : (uint8_t)0;
                    bv[u] = (in && a.base) ? a.base[shot * g.n_data + q] : (uint8_t)0;
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int w0 = wbase + wv * 64 + i0 + u;
                    if (w0 >= g.lz_words) break;  // uniform
                    const int q = w0 * 64 + lane;
                    int v = 0;
                    if (q < g.n_data) {
                        int cb = bv[u] & 1;
                        for (int t = 0; t < g.fold_blocks; ++t) cb ^= xh[t * g.n_data + q];
                        if (a.corr_out) a.corr_out[shot * g.n_data + q] = (uint8_t)cb;
                        v = (rv[u] ^ cb) & 1;
                    }
                    const unsigned long long word = __ballot(v);
                    mine = lane == i0 + u ? word : mine;
                }
            }
            const int w0 = wbase + tid;
            const bool have = w0 < g.lz_words;
            for (int r = 0; r < g.k; ++r) {
                const int x = have ? (__popcll(g.lz[(size_t)r * g.lz_words + w0] & mine) & 1) : 0;
                if (__popcll(__ballot(x)) & 1) {  // uniform per wave
                    if (lane == 0) atomicXor(&lpar[r], 1);
                }
            }
        }
    }
    __syncthreads();
    int f = 0;
    if (want_fail)
        for (int r = tid; r < g.k; r += kBlock) f |= lpar[r] != 0;
    f = __syncthreads_or(f) ? 1 : 0;
    if (tid == 0) {
        if (a.status) a.status[shot] = (uint8_t)((conv ? 1 : 0) | (satisfied ? 2 : 0));
        if (a.ssf_steps) a.ssf_steps[shot] = steps;
        if (a.fail) a.fail[shot] = (uint8_t)(want_fail ? f : 0);
    }
    __syncthreads();
}

// DRM / DCM > 0 (row degree <= DRM, column degree <= DCM; both methods): the row and
// column loops are unrolled to that width with every load of a row (column)
// issued before any use, and the column pass keeps its prefix sums in registers
// (one scattered read and one scattered write per edge instead of five).  Same
// operations in the same order as the generic loops.
template <typename T, int METHOD, bool DEFER, int DRM = 0, int DCM = 0>
__global__ __launch_bounds__(kBlock) void bp_block_kernel(DevGraph g, DecodeArgs a, T* gscratch, int placement) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int E = g.E, m = g.m, n = g.n, tid = threadIdx.x;
    constexpr int PREC = sizeof(T) == 4 ? 1 : 0;
    int* slot_s = reinterpret_cast<int*>(smem + kCtrlSlot);
    // placement bit 0: messages in LDS, bit 1: per-shot byte arrays in LDS;
    // whatever is not in LDS lives in this workgroup's HBM scratch slice
    const size_t msg_bytes = ((size_t)2 * E * sizeof(T) + 15) / 16 * 16;
    unsigned char* slice = reinterpret_cast<unsigned char*>(gscratch) +
                           (size_t)blockIdx.x * block_slice_bytes(g, sizeof(T), placement);
    unsigned char* p = (placement & 2) ? smem + kCtrl : slice + ((placement & 1) ? 0 : msg_bytes);
    T* v2c;
    if (placement & 1) {
        v2c = reinterpret_cast<T*>(p);
        p += msg_bytes;
    } else {
        v2c = reinterpret_cast<T*>(slice);
    }
    T* c2v = v2c + E;
    uint8_t* xh = p;                      // [n_pad]
    uint8_t* sb = xh + g.n_pad;           // [m_pad] syndrome bits
    int* lpar = reinterpret_cast<int*>(sb + g.m_pad);  // [k]
    uint8_t* rs = reinterpret_cast<uint8_t*>(lpar + (g.k > 0 ? g.k : 1));  // [m_pad] last residual
    const T* prior = reinterpret_cast<const T*>(g.prior[METHOD][PREC]);
    const int32_t* rp = g.row_ptr;
    const int32_t* ci = g.col_idx;
    const int32_t* cp = g.col_ptr;
    const int32_t* ce = g.col_edge;
    // the unrolled instantiations store c2v in CSC (column) order, so the
    // column pass reads it sequentially and only the row pass's writes scatter
    const int32_t* ecs = g.edge_csc;
    constexpr bool kCsc = DRM > 0;
    // unrolled min-sum with messages in HBM: v2c in CSC order and c2v in CSR
    // order instead, so both passes write contiguously and only their reads
    // scatter.  A scattered 4-byte HBM write costs a partial-sector write-back
    // (C5: ~30 B of HBM writes per message write, 155 MB per shot); a
    // scattered read costs a sector fetch without the write-back.
    const bool vcsc = METHOD == 1 && DRM > 0 && !(placement & 1);
    // placement 0 (byte arrays in HBM): the unrolled instantiation also keeps the
    // hard decision as bits in LDS ([n_pad/64] words, one ballot per wave), so the
    // syndrome test gathers bits from LDS instead of bytes from HBM
    uint64_t* xbits = reinterpret_cast<uint64_t*>(smem + kCtrl);
    const bool xb = DRM > 0 && placement == 0;

    // next shot: from the launcher's counter (dynamic, a.work_ctr) or by stride
    long long* next_s = reinterpret_cast<long long*>(smem + kCtrlNext);
    auto next_shot = [&](int64_t cur) -> int64_t {
        if (!a.work_ctr) return cur < 0 ? (int64_t)blockIdx.x : cur + gridDim.x;
        return block_next_shot(a.work_ctr, next_s, tid);
    };
    for (int64_t shot = next_shot(-1); shot < a.B; shot = next_shot(shot)) {
        block_syndrome_rows(sb, a.syn, a.syn_flags, a.base, a.readout, shot, g.n_data, rp, ci, m, tid);
        if (vcsc) {
            for (int j = tid; j < n; j += kBlock) {
                const T pj = prior[j];
                for (int t = cp[j]; t < cp[j + 1]; ++t) v2c[t] = pj;  // CSC order
            }
        } else {
            for (int e = tid; e < E; e += kBlock) v2c[e] = prior[ci[e]];  // CSR order: coalesced
        }
        __syncthreads();
        int it = 1;
        bool conv = false;
        for (; it <= a.max_iter; ++it) {
            const T alpha = alpha_at<T>(it, a.ms_scaling);
            for (int i = tid; i < m; i += kBlock) {
                const int e0 = rp[i], e1 = rp[i + 1];
                if constexpr (METHOD == 1 && DRM > 0) {
                    const int d = e1 - e0;
                    T v[DRM];
#pragma unroll
                    for (int t = 0; t < DRM; ++t)
                        if (t < d) v[t] = v2c[vcsc ? ecs[e0 + t] : e0 + t];
                    T m1 = Big<T>::v, m2 = Big<T>::v;
                    int par = sb[i];
#pragma unroll
                    for (int t = 0; t < DRM; ++t)
                        if (t < d) {
                            const T av = fabs(v[t]);
                            m2 = med3(av, m1, m2);
                            m1 = fmin(m1, av);
                            par ^= v[t] <= (T)0;
                        }
                    const T m1a = m1 * alpha, m2a = m2 * alpha;
#pragma unroll
                    for (int t = 0; t < DRM; ++t)
                        if (t < d) {
                            const T y = (fabs(v[t]) == m1) ? m2a : m1a;
                            c2v[vcsc ? e0 + t : ecs[e0 + t]] = (par ^ (v[t] <= (T)0)) ? -y : y;
                        }
                } else if constexpr (METHOD == 1) {
                    ms_check_row(v2c, c2v, e0, e1, (int)sb[i], alpha);
                } else if constexpr (DRM > 0) {
                    // product-sum, unrolled: forward products, then backward
                    const int d = e1 - e0;
                    T v[DRM], r[DRM], fw[DRM];
#pragma unroll
                    for (int t = 0; t < DRM; ++t)
                        if (t < d) v[t] = v2c[e0 + t];
                    T f = sb[i] ? (T)-1 : (T)1;
#pragma unroll
                    for (int t = 0; t < DRM; ++t)
                        if (t < d) {
                            fw[t] = f;
                            r[t] = (T)2 / ((T)1 + v[t]) - (T)1;
                            f *= r[t];
                        }
                    T b = (T)1;
#pragma unroll
                    for (int t = DRM - 1; t >= 0; --t)
                        if (t < d) {
                            const T c = fw[t] * b;
                            c2v[ecs[e0 + t]] = ((T)1 - c) / ((T)1 + c);
                            b *= r[t];
                        }
                } else {
                    T f = sb[i] ? (T)-1 : (T)1;
                    for (int e = e0; e < e1; ++e) {
                        c2v[e] = f;
                        f *= (T)2 / ((T)1 + v2c[e]) - (T)1;
                    }
                    T b = (T)1;
                    for (int e = e1 - 1; e >= e0; --e) {
                        T c = c2v[e] * b;
                        c2v[e] = ((T)1 - c) / ((T)1 + c);
                        b *= (T)2 / ((T)1 + v2c[e]) - (T)1;
                    }
                }
            }
            __syncthreads();
            for (int j = tid; j < n; j += kBlock) {
                const int t0 = cp[j], t1 = cp[j + 1];
                T acc = prior[j];
                if constexpr (METHOD == 1 && DCM > 0) {
                    const int d = t1 - t0;
                    int ev[DCM];
                    T c[DCM], pre[DCM];
#pragma unroll
                    for (int t = 0; t < DCM; ++t)
                        if (t < d) ev[t] = ce[t0 + t];
#pragma unroll
                    for (int t = 0; t < DCM; ++t)
                        if (t < d) c[t] = c2v[vcsc ? ev[t] : t0 + t];  // CSC order: contiguous
#pragma unroll
                    for (int t = 0; t < DCM; ++t)
                        if (t < d) {
                            pre[t] = acc;
                            acc += c[t];
                        }
                    xh[j] = acc <= (T)0;
                    if (xb) {
                        const uint64_t w = __ballot(acc <= (T)0);
                        if ((tid & 63) == 0) xbits[j >> 6] = w;
                    }
                    T suf = (T)0;
#pragma unroll
                    for (int t = DCM - 1; t >= 0; --t)
                        if (t < d) {
                            v2c[vcsc ? t0 + t : ev[t]] = pre[t] + suf;
                            suf += c[t];
                        }
                } else if constexpr (METHOD == 1) {
                    for (int t = t0; t < t1; ++t) {
                        const int e = ce[t];
                        v2c[e] = acc;
                        acc += c2v[e];
                    }
                    xh[j] = acc <= (T)0;
                    T suf = (T)0;
                    for (int t = t1 - 1; t >= t0; --t) {
                        const int e = ce[t];
                        v2c[e] = v2c[e] + suf;
                        suf += c2v[e];
                    }
                } else if constexpr (DCM > 0) {
                    // product-sum, unrolled (NaN guards as in the generic loop)
                    const int d = t1 - t0;
                    int ev[DCM];
                    T c[DCM], pre[DCM];
#pragma unroll
                    for (int t = 0; t < DCM; ++t)
                        if (t < d) ev[t] = ce[t0 + t];
#pragma unroll
                    for (int t = 0; t < DCM; ++t)
                        if (t < d) c[t] = c2v[t0 + t];  // CSC order: contiguous
#pragma unroll
                    for (int t = 0; t < DCM; ++t)
                        if (t < d) {
                            pre[t] = acc;
                            acc *= c[t];
                            if (isnan(acc)) acc = (T)1;
                        }
                    xh[j] = acc >= (T)1;
                    if (xb) {
                        const uint64_t w = __ballot(acc >= (T)1);
                        if ((tid & 63) == 0) xbits[j >> 6] = w;
                    }
                    T suf = (T)1;
#pragma unroll
                    for (int t = DCM - 1; t >= 0; --t)
                        if (t < d) {
                            v2c[ev[t]] = pre[t] * suf;
                            suf *= c[t];
                            if (isnan(suf)) suf = (T)1;
                        }
                } else {
                    for (int t = t0; t < t1; ++t) {
                        const int e = ce[t];
                        v2c[e] = acc;
                        acc *= c2v[e];
                        if (isnan(acc)) acc = (T)1;
                    }
                    xh[j] = acc >= (T)1;
                    T suf = (T)1;
                    for (int t = t1 - 1; t >= t0; --t) {
                        const int e = ce[t];
                        v2c[e] = v2c[e] * suf;
                        suf *= c2v[e];
                        if (isnan(suf)) suf = (T)1;
                    }
                }
            }
            __syncthreads();
            bool open;
            if constexpr (DRM > 0) {
                int bad = 0;
                for (int i = tid; i < m; i += kBlock) {
                    int par = sb[i];
                    const int e0 = rp[i], d = rp[i + 1] - e0;
                    int cc[DRM];
#pragma unroll
                    for (int t = 0; t < DRM; ++t)
                        if (t < d) cc[t] = ci[e0 + t];
#pragma unroll
                    for (int t = 0; t < DRM; ++t)
                        if (t < d) par ^= xb ? (int)((xbits[cc[t] >> 6] >> (cc[t] & 63)) & 1ull) : (int)xh[cc[t]];
                    rs[i] = (uint8_t)par;
                    bad |= par;
                }
                open = __syncthreads_or(bad) != 0;
            } else {
                open = block_syndrome_open(sb, xh, rp, ci, m, tid, rs);
            }
            if (!open) {
                conv = true;
                break;
            }
        }
        const int iters = conv ? it : a.max_iter;
        if (tid == 0 && a.iters) a.iters[shot] = iters;
        if (a.llr_out) {  // soft output of the last iteration, same summation order
            T* lo = reinterpret_cast<T*>(a.llr_out);
            for (int j = tid; j < n; j += kBlock) {
                T acc = prior[j];
                for (int t = cp[j]; t < cp[j + 1]; ++t) {
                    if constexpr (METHOD == 1) {
                        acc += c2v[(kCsc && !vcsc) ? t : ce[t]];
                    } else {
                        acc *= c2v[kCsc ? t : ce[t]];
                        if (isnan(acc)) acc = (T)1;
                    }
                }
                if constexpr (METHOD == 1) lo[shot * n + j] = acc;
                else lo[shot * n + j] = (T)log((double)((T)1 / acc));
            }
        }
        if (DEFER && !conv) {
            if (tid == 0) *slot_s = atomicAdd(a.q_count, 1);
            __syncthreads();
            const int slot = *slot_s;
            for (int j = tid; j < n; j += kBlock) a.q_x[(int64_t)slot * n + j] = xh[j];
            for (int i = tid; i < m; i += kBlock) a.q_r[(int64_t)slot * m + i] = rs[i];
            if (tid == 0) a.q_idx[slot] = shot;
            __syncthreads();
        } else {
            finalize_block(g, a, shot, xh, conv, conv, 0, lpar);
        }
    }
}

// Small-set-flip for queued shots, one workgroup per shot; generator gi is
// scanned by thread gi % 256.  Same keys as ssf_wave_kernel.
// gstate: when non-null, the shot state (xh, sres, lpar) of workgroup b lives at
// gstate + b * block_state_stride(g) in HBM instead of LDS (graphs whose state
// exceeds the LDS budget, e.g. the 1.2*10^5-column spacetime graph of config 5).
__global__ __launch_bounds__(kBlock) void ssf_block_kernel(DevGraph g, DecodeArgs a, unsigned char* gstate) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    long long* redl = reinterpret_cast<long long*>(smem + kCtrlRed64);
    int* redi = reinterpret_cast<int*>(smem + kCtrlRed32);
    uint8_t* xh = gstate ? gstate + (size_t)blockIdx.x * block_state_stride(g) : smem + kCtrl;  // [n_pad]
    uint8_t* sres = xh + g.n_pad;     // [m_pad]
    int* lpar = reinterpret_cast<int*>(sres + g.m_pad);  // [k]
    const int tid = threadIdx.x, m = g.m, n = g.n;
    const int count = *a.q_count;
    const int nhi = g.g_wmax > 4 ? (1 << (g.g_wmax - 4)) : 1;
    for (int slot = blockIdx.x; slot < count; slot += gridDim.x) {
        // queue entries of the shot-lane kernel carry its BP-converged bit in bit 62
        const int64_t qv = a.q_idx[slot];
        const int64_t shot = qv & ((1ll << 62) - 1);
        const bool bp_conv = (qv >> 62) & 1;
        // the queued hard decision and residual, eight loads in flight per
        // thread before any LDS store (a loop of single byte loads waited for
        // each one: ~40 HBM round trips per shot at n = 10^4)
        copy_bytes8(a.q_x + (int64_t)slot * n, xh, n, tid);
        int wl = copy_bytes8(a.q_r + (int64_t)slot * m, sres, m, tid);
        int sw = block_sum(wl, redi, tid);  // includes a barrier: LDS fills visible
        int steps = 0;
        while (a.ssf && sw > 0 && (a.ssf_max_steps <= 0 || steps < a.ssf_max_steps)) {
            long long best = LLONG_MIN;
            for (int gi = tid; gi < g.n_gen; gi += kBlock) {
                const int nlc = g.g_nlc[gi];
                uint32_t sl = 0;
                for (int c = 0; c < nlc; ++c) sl |= (uint32_t)sres[g.g_lc[c * g.g_pad + gi]] << c;
                if (sl == 0) continue;
                uint32_t qm[kGenW];
#pragma unroll
                for (int k = 0; k < kGenW; ++k) qm[k] = g.g_qmask[k * g.g_pad + gi];
                best = max(best, gen_key64(gen_best_key(sl, qm, nhi), gi));
            }
            best = block_max(best, redl, tid);
            const int score = (int)(best >> 32);
            if (best == LLONG_MIN || score <= 0) break;
            const int gsel = 0xFFFFFF - (int)((best >> 8) & 0xFFFFFF);
            const int tsel = 255 - (int)(best & 255);
            const int gain = score * __builtin_popcount(tsel) / kSsfScale;
            const int w = g.g_w[gsel];
            uint32_t mask = 0;
            for (int k = 0; k < w; ++k)
                if ((tsel >> k) & 1) mask ^= g.g_qmask[k * g.g_pad + gsel];
            if (tid < g.g_nlc[gsel] && ((mask >> tid) & 1)) sres[g.g_lc[tid * g.g_pad + gsel]] ^= 1;
            if (tid < w && ((tsel >> tid) & 1)) xh[g.g_q[tid * g.g_pad + gsel]] ^= 1;
            __syncthreads();
            sw -= gain;
            ++steps;
        }
        finalize_block(g, a, shot, xh, bp_conv, sw == 0, steps, lpar);
    }
}

// Incremental small-set-flip for queued shots (same spec and keys as
// ssf_block_kernel, one workgroup per shot): every generator's local syndrome
// and best key are cached in LDS, and a step only re-scores the generators
// whose local syndrome it changed (found through the check -> generator inverse
// table g_iptr / g_ient), instead of re-gathering and re-scoring all of them.
// Key (int32): score << 13 | (8191 - g), so a signed max picks the highest
// score, then the lowest g; the lowest subset reaching that score is found
// afterwards by wave 0 (as in ssf_wave_kernel).
__global__ __launch_bounds__(kBlock) void ssf_inc_block_kernel(DevGraph g, DecodeArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    long long* redl = reinterpret_cast<long long*>(smem + kCtrlRed64);
    int* redi = reinterpret_cast<int*>(smem + kCtrlRed32);
    int* ctl = reinterpret_cast<int*>(smem + kCtrlSlot);  // [0] dirty count, [1] chosen subset, [2] its gain
    const size_t gp = (size_t)g.g_pad;
    int* key = reinterpret_cast<int*>(smem + kCtrl);
    uint32_t* slg = reinterpret_cast<uint32_t*>(key + gp);
    uint16_t* dlist = reinterpret_cast<uint16_t*>(slg + gp);
    uint32_t* dbits = reinterpret_cast<uint32_t*>(reinterpret_cast<unsigned char*>(dlist) + (gp * 2 + 15) / 16 * 16);
    uint8_t* xh = reinterpret_cast<uint8_t*>(dbits) + ((gp + 31) / 32 * 4 + 15) / 16 * 16;
    uint8_t* sres = xh + ((size_t)g.n_pad + 15) / 16 * 16;
    int* lpar = reinterpret_cast<int*>(sres + ((size_t)g.m_pad + 15) / 16 * 16);
    uint8_t* rdl = reinterpret_cast<uint8_t*>(lpar) + (4 * (size_t)(g.k > 0 ? g.k : 1) + 15) / 16 * 16;
    const int tid = threadIdx.x, m = g.m, n = g.n, ng = g.n_gen, nd = g.n_data;
    const int count = *a.q_count;
    // whole rows by 16-B loads, every load of a shot issued before the first LDS
    // store, when the rows allow (16-B multiples at 16-B aligned bases, <= kRowU
    // loads per thread): the byte rounds of copy_bytes8 (8 bytes of a thread's
    // share per HBM round trip) made the rows' loads ~8 dependent round trips
    // per shot at n = 10^4.  The readout row goes to LDS too (finalize_block).
    constexpr int kRowU = 3;
    const bool want_rd = a.fail && a.readout && g.k > 0;
    auto al16 = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
    const bool vec = ((n | m | (want_rd ? nd : 0)) & 15) == 0 && al16(a.q_x) && al16(a.q_r) &&
                     (!want_rd || al16(a.readout)) && n <= 16 * kRowU * kBlock && m <= 16 * kRowU * kBlock &&
                     nd <= 16 * kRowU * kBlock;
    const int nhi = g.g_wmax > 4 ? (1 << (g.g_wmax - 4)) : 1;
    for (int w = tid; w < (int)((gp + 31) / 32); w += kBlock) dbits[w] = 0u;
    if (tid == 0) ctl[0] = 0;
    // table scoring (DevGraph::s_lut, ssf_lut_tables): a generator's best
    // (score, subset) is one lookup on its local syndrome; the key then carries
    // the score's rank, which orders like the score
    const bool lut = g.s_lut && g.opt_ssf == kSsfAuto;
    auto rescore = [&](int gi) {
        const uint32_t sl = slg[gi];
        if (sl == 0u) {
            key[gi] = INT_MIN;
            return;
        }
        if (lut) {
            const uint32_t r = g.s_lut[g.s_off[gi] + sl] >> 24;
            key[gi] = r ? (int)((r << 13) | (uint32_t)(8191 - gi)) : INT_MIN;
            return;
        }
        uint32_t qm[kGenW];
#pragma unroll
        for (int k = 0; k < kGenW; ++k) qm[k] = g.g_qmask[k * gp + gi];
        key[gi] = (int)((unsigned)gen_best_score(sl, qm, nhi) << 13) | (8191 - gi);
    };
    for (int slot = blockIdx.x; slot < count; slot += gridDim.x) {
        const int64_t qv = a.q_idx[slot];
        const int64_t shot = qv & ((1ll << 62) - 1);
        const bool bp_conv = (qv >> 62) & 1;
        // the queued hard decision and residual, eight loads in flight per
        // thread before any LDS store (a loop of single byte loads waited for
        // each one: ~40 HBM round trips per shot at n = 10^4)
        int wl = 0;
        if (vec) {
            uint4 vx[kRowU], vr[kRowU], vd[kRowU];
            const uint4 z = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
            for (int u = 0; u < kRowU; ++u) {
                const int j = (u * kBlock + tid) * 16;
                vx[u] = j < n ? *reinterpret_cast<const uint4*>(a.q_x + (int64_t)slot * n + j) : z;
                vr[u] = j < m ? *reinterpret_cast<const uint4*>(a.q_r + (int64_t)slot * m + j) : z;
                vd[u] = (want_rd && j < nd) ? *reinterpret_cast<const uint4*>(a.readout + shot * nd + j) : z;
            }
#pragma unroll
            for (int u = 0; u < kRowU; ++u) {
                const int j = (u * kBlock + tid) * 16;
                if (j < n) *reinterpret_cast<uint4*>(xh + j) = vx[u];
                if (j < m) {
                    *reinterpret_cast<uint4*>(sres + j) = vr[u];
                    // bytes are 0 / 1: the bit count is the byte sum
                    wl += __builtin_popcount(vr[u].x) + __builtin_popcount(vr[u].y) + __builtin_popcount(vr[u].z) +
                          __builtin_popcount(vr[u].w);
                }
                if (want_rd && j < nd) *reinterpret_cast<uint4*>(rdl + j) = vd[u];
            }
        } else {
            copy_bytes8(a.q_x + (int64_t)slot * n, xh, n, tid);
            wl = copy_bytes8(a.q_r + (int64_t)slot * m, sres, m, tid);
        }
        int sw = block_sum(wl, redi, tid);  // includes a barrier: LDS fills visible
        int steps = 0;
        if (a.ssf && sw > 0) {
            for (int gi = tid; gi < ng; gi += kBlock) {
                const int nlc = g.g_nlc[gi];
                uint32_t sl = 0;
                for (int c = 0; c < nlc; ++c) sl |= (uint32_t)sres[g.g_lc[c * gp + gi]] << c;
                slg[gi] = sl;
                rescore(gi);
            }
            __syncthreads();
            while (sw > 0 && (a.ssf_max_steps <= 0 || steps < a.ssf_max_steps)) {
                long long best = LLONG_MIN;
                for (int gi = tid; gi < ng; gi += kBlock) best = max(best, (long long)key[gi]);
                best = block_max(best, redl, tid);
                const int kv = (int)best;
                const int score = kv >> 13;
                if (best == LLONG_MIN || kv == INT_MIN || score <= 0) break;
                const int gsel = 8191 - (kv & 8191);
                const int w = g.g_w[gsel];
                if (lut) {  // the table entry names the subset and the local checks it toggles
                    if (tid == 0) {
                        const uint32_t sl = slg[gsel];
                        const uint32_t e = g.s_lut[g.s_off[gsel] + sl];
                        ctl[1] = (int)(e & 0xffu);
                        ctl[2] = __builtin_popcount(sl) - __builtin_popcount(sl ^ ((e >> 8) & 0xffffu));  // gain
                    }
                } else if (tid < 64) {  // wave 0: the lowest subset reaching the score
                    const uint32_t sl = slg[gsel];
                    const int base = __builtin_popcount(sl);
                    uint32_t qs[kGenW];
#pragma unroll
                    for (int k = 0; k < kGenW; ++k) qs[k] = g.g_qmask[k * gp + gsel];
                    int tsel = -1;
                    for (int t0 = 0; t0 < 16 * nhi; t0 += 64) {
                        const int t = t0 + tid;
                        uint32_t mt = 0;
#pragma unroll
                        for (int k = 0; k < kGenW; ++k) mt ^= ((t >> k) & 1) ? qs[k] : 0u;
                        const int gain = base - __builtin_popcount(sl ^ mt);
                        const bool hit = t > 0 && t < 16 * nhi && gain * kSsfScale == score * __builtin_popcount(t);
                        const unsigned long long hb = __ballot(hit);
                        if (hb) {
                            tsel = t0 + __builtin_ctzll(hb);
                            break;
                        }
                    }
                    if (tid == 0) ctl[1] = tsel;
                }
                __syncthreads();
                const int tsel = ctl[1];
                if (tsel <= 0) break;  // unreachable: the best score is some subset's score
                uint32_t mask = 0;
                for (int k = 0; k < w; ++k)
                    if ((tsel >> k) & 1) mask ^= g.g_qmask[k * gp + gsel];
                // (read before any thread's flip below changes slg: set by tid 0
                // before the barrier)
                const int gain = lut ? ctl[2] : score * __builtin_popcount(tsel) / kSsfScale;
                // flip: residual, hard decision, and every generator's local syndrome
                // bit of each flipped check (those generators are queued for re-scoring)
                if (tid < g.g_nlc[gsel] && ((mask >> tid) & 1)) {
                    const int c = g.g_lc[tid * gp + gsel];
                    sres[c] ^= 1;
                    for (int e = g.g_iptr[c]; e < g.g_iptr[c + 1]; ++e) {
                        const uint32_t ent = g.g_ient[e];
                        const int g2 = (int)(ent & 0xffffu);
                        atomicXor(&slg[g2], 1u << (ent >> 16));
                        const uint32_t bit = 1u << (g2 & 31);
                        if (!(atomicOr(&dbits[g2 >> 5], bit) & bit)) dlist[atomicAdd(&ctl[0], 1)] = (uint16_t)g2;
                    }
                }
                if (tid < w && ((tsel >> tid) & 1)) xh[g.g_q[tid * gp + gsel]] ^= 1;
                __syncthreads();
                const int nd = ctl[0];
                for (int d = tid; d < nd; d += kBlock) {
                    const int g2 = dlist[d];
                    dbits[g2 >> 5] = 0u;  // whole word: every generator in it is being re-scored or clean
                    rescore(g2);
                }
                __syncthreads();
                if (tid == 0) ctl[0] = 0;
                sw -= gain;
                ++steps;
            }
        }
        finalize_block(g, a, shot, xh, bp_conv, sw == 0, steps, lpar, vec && want_rd ? rdl : nullptr);
    }
}

// bp_block_kernel T, METHOD, DEFER, DRM, DCM (DRM = DCM = 0: loops over the
// degrees; 16, 8: unrolled, row degree <= 16, column degree <= 8).  The SSF /
// finalize kernels are no templates: ssf[0] is ssf_inc_block_kernel, ssf[1]
// ssf_block_kernel with its shot state in LDS (in the scratch tail the launcher
// passes the control area alone).  qd_graph_last_kernels reports none of them.
template <typename T, int METHOD>
static void add_block_types(KernelTable& t) {
    for (KernelEntry e : {QDEC_INST(kBlock, bp_block_kernel, T, METHOD, false, 0, 0),
                          QDEC_INST(kBlock, bp_block_kernel, T, METHOD, true, 0, 0),
                          QDEC_INST(kBlock, bp_block_kernel, T, METHOD, false, 16, 8),
                          QDEC_INST(kBlock, bp_block_kernel, T, METHOD, true, 16, 8)}) {
        e.noted = false;
        t.push_back(e);
    }
}

void add_block_kernels(KernelTable& block, KernelTable& ssf) {
    add_block_types<float, 0>(block);
    add_block_types<float, 1>(block);
    add_block_types<double, 0>(block);
    add_block_types<double, 1>(block);
    KernelEntry inc, blk;
    inc.fn = reinterpret_cast<const void*>(&ssf_inc_block_kernel);
    inc.name = "qdec::ssf_inc_block_kernel";
    inc.lds = [](const DevGraph& g, const DecodeArgs&) { return ssf_inc_lds(g); };
    blk.fn = reinterpret_cast<const void*>(&ssf_block_kernel);
    blk.name = "qdec::ssf_block_kernel";
    blk.lds = [](const DevGraph& g, const DecodeArgs&) { return (block_small_lds(g) + 15) / 16 * 16; };
    inc.block = blk.block = kBlock;
    inc.noted = blk.noted = false;
    ssf = {inc, blk};
}

}  // namespace qdec
