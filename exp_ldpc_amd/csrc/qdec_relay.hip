// qdec_relay.hip -- relay-BP: an ensemble of min-sum legs with per-variable
// memory strengths, for the shots plain BP leaves open on graphs without flip
// sets (circuit detector error models).  DESIGN 3.6d holds the spec to the last
// rounding; tests/relay_model.py is its numpy model.
//
// One 256-thread workgroup per shot, persistent over the batch and fed by the
// launch's shot counter.  Generic CSR / CSC, messages indexed by CSR edge as in
// bp_block_kernel's generic path, whose check pass and variable order these are:
//   check pass     thread per check: the two smallest |v2c| of the row, the sign
//                  from the syndrome bit and the row's parity of v <= 0
//   variable pass  thread per variable: bias = (1 - gamma) prior + gamma M, prefix
//                  then suffix along the column, marginal and messages clamped
// The messages v2c[E], c2v[E] and the marginals M[n] live in LDS, or in this
// workgroup's slot of a scratch the graph handle owns (RelayLayout); a slot is
// touched by its own workgroup only, so a workgroup barrier orders its traffic.
// The hard decision and the syndrome stay in LDS as bytes, the best solution
// as bits.  A leg's tables (gamma row, weights) are indexed per lane, so they
// come through vector loads and stay in L2 across the workgroups.
#include <hip/hip_runtime.h>

#include "qdec_block_steps.h"
#include "qdec_kernels.h"
#include "qdec_relay.h"

namespace qdec {

namespace {

template <typename T>
__device__ __forceinline__ T clamp_to(T v, T clip) {
    return fmin(fmax(v, -clip), clip);
}

}  // namespace

template <typename T>
__global__ __launch_bounds__(kBlock) void relay_block_kernel(DevGraph g, RelayArgs a, RelayTables rt, RelayLayout L,
                                                             unsigned char* scratch) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int PREC = sizeof(T) == 4 ? 1 : 0;
    const int E = g.E, m = g.m, n = g.n, tid = threadIdx.x;
    long long* red = reinterpret_cast<long long*>(smem + kCtrlRed64);
    long long* next_s = reinterpret_cast<long long*>(smem + kCtrlNext);
    uint8_t* xh = smem + L.l_xh;                                  // [n_pad] hard decision
    uint8_t* sb = smem + L.l_sb;                                  // [m_pad] syndrome bits
    uint64_t* best = reinterpret_cast<uint64_t*>(smem + L.l_best);  // [n_pad / 64] best solution
    unsigned char* msg = scratch ? scratch + (size_t)blockIdx.x * (size_t)L.slot_bytes : smem + L.l_msg;
    T* v2c = reinterpret_cast<T*>(msg);
    T* c2v = reinterpret_cast<T*>(msg + L.o_c2v);
    T* M = reinterpret_cast<T*>(msg + L.o_M);
    const T* prior = reinterpret_cast<const T*>(g.prior[1][PREC]);
    const T* gam_all = reinterpret_cast<const T*>(rt.gamma[PREC]);
    const int32_t* rp = g.row_ptr;
    const int32_t* ci = g.col_idx;
    const int32_t* cp = g.col_ptr;
    const int32_t* ce = g.col_edge;
    const T alpha = (T)rt.alpha, clip = (T)rt.clip;
    (void)E;

    for (int64_t shot = block_next_shot(a.work_ctr, next_s, tid); shot < a.B;
         shot = block_next_shot(a.work_ctr, next_s, tid)) {
        if (a.only_failed && a.status && (a.status[shot] & 1)) continue;  // uniform over the workgroup
        block_syndrome_rows(sb, a.syn, a.syn_flags, a.base, a.readout, shot, g.n_data, rp, ci, m, tid);
        for (int j = tid; j < n; j += kBlock) M[j] = prior[j];
        __syncthreads();
        int found = 0, legs = 0, iters = 0;
        bool have_best = false;
        long long best_w = 0;
        for (int leg = 0; leg <= rt.num_sets; ++leg) {
            const T* gam = gam_all + (size_t)leg * n;
            const int leg_iter = leg == 0 ? rt.pre_iter : rt.set_max_iter;
            // leg start: every edge's v2c = the bias from the previous leg's marginals
            for (int j = tid; j < n; j += kBlock) {
                const T gj = gam[j];
                const T bias = ((T)1 - gj) * prior[j] + gj * M[j];
                for (int t = cp[j]; t < cp[j + 1]; ++t) v2c[ce[t]] = bias;
            }
            __syncthreads();
            bool conv = false;
            for (int it = 1; it <= leg_iter; ++it) {
                for (int i = tid; i < m; i += kBlock) ms_check_row(v2c, c2v, rp[i], rp[i + 1], (int)sb[i], alpha);
                __syncthreads();
                for (int j = tid; j < n; j += kBlock) {
                    const int t0 = cp[j], t1 = cp[j + 1];
                    const T gj = gam[j];
                    T acc = ((T)1 - gj) * prior[j] + gj * M[j];
                    for (int t = t0; t < t1; ++t) {
                        const int e = ce[t];
                        v2c[e] = acc;
                        acc += c2v[e];
                    }
                    acc = clamp_to(acc, clip);
                    M[j] = acc;
                    xh[j] = acc <= (T)0;
                    T suf = (T)0;
                    for (int t = t1 - 1; t >= t0; --t) {
                        const int e = ce[t];
                        v2c[e] = clamp_to(v2c[e] + suf, clip);
                        suf += c2v[e];
                    }
                }
                __syncthreads();
                ++iters;
                if (!block_syndrome_open(sb, xh, rp, ci, m, tid, nullptr)) {
                    conv = true;
                    break;
                }
            }
            ++legs;
            if (!conv) continue;
            ++found;
            long long wl = 0;
            for (int j = tid; j < n; j += kBlock)
                if (xh[j]) wl += rt.w[j];
            const long long wgt = block_sum(wl, red, tid);
            if (!have_best || wgt < best_w) {  // uniform; a tie keeps the earlier leg
                have_best = true;
                best_w = wgt;
                for (int j = tid; j < g.n_pad; j += kBlock) {  // whole waves: n_pad is a multiple of 64
                    const uint64_t word = __ballot(j < n && xh[j]);
                    if ((tid & 63) == 0) best[j >> 6] = word;
                }
            }
            if (found == rt.stop_nconv) break;
        }
        if (tid == 0) {
            if (a.iters) a.iters[shot] = iters;
            if (a.legs) a.legs[shot] = legs;
        }
        if (a.llr_out) {
            T* lo = reinterpret_cast<T*>(a.llr_out);
            for (int j = tid; j < n; j += kBlock) lo[shot * n + j] = M[j];
        }
        __syncthreads();  // the last leg's reads of xh are done, best is visible
        if (have_best)
            for (int j = tid; j < n; j += kBlock) xh[j] = (uint8_t)((best[j >> 6] >> (j & 63)) & 1ull);
        __syncthreads();
        if (tid < 64) {  // the fold and the failure check of the wave kernels, by one wave
            DecodeArgs fa{};
            fa.B = a.B;
            fa.base = a.base;
            fa.readout = a.readout;
            fa.x_out = a.x_out;
            fa.corr_out = a.corr_out;
            fa.status = a.status;
            fa.fail = a.fail;
            finalize_shot(g, fa, shot, xh, have_best, have_best, 0, tid);
        }
        __syncthreads();
    }
}

void add_relay_kernels(KernelTable& t) {
    t.push_back(QDEC_INST(kBlock, relay_block_kernel, double));
    t.push_back(QDEC_INST(kBlock, relay_block_kernel, float));
}

const KernelTable& relay_table() {
    static const KernelTable table = [] {
        KernelTable t;
        add_relay_kernels(t);
        return t;
    }();
    return table;
}

void append_relay_kernel_names(std::string& out) {
    for (const KernelEntry& e : relay_table()) out += e.name + "\n";
}

// `grid` workgroups; with the messages in HBM `scratch` holds `grid` slots of
// L.slot_bytes, with them in LDS it is null
int launch_relay(const DevGraph& g, int precision, const RelayArgs& a, const RelayTables& t, const RelayLayout& L,
                 void* scratch, int64_t grid, hipStream_t stream) {
    if (a.B <= 0 || grid <= 0) return 0;
    const KernelEntry* e = find_kernel(relay_table(), {precision});
    if (!e) return (int)hipErrorNotSupported;
    const size_t lds = (size_t)L.lds_bytes(scratch != nullptr);
    if (lds > 64 * 1024) {
        const hipError_t ea = hipFuncSetAttribute(e->fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (ea != hipSuccess) return (int)ea;
    }
    using RelaySig = KernelSig<DevGraph, RelayArgs, RelayTables, RelayLayout, unsigned char*>;
    return launch_entry(RelaySig{}, *e, grid, lds, stream, g, a, t, L, static_cast<unsigned char*>(scratch));
}

}  // namespace qdec
