// qdec_layered.hip -- layered (check-serial) min-sum BP: the rows of H are
// processed one after the other and the posteriors are updated after each, so
// information crosses the graph within an iteration.  DESIGN 3.6f holds the spec
// to the last rounding; tests/layered_model.py is its numpy model.
//
// One wave per workgroup and one shot at a time per workgroup, persistent over
// the batch and fed by the launch's shot counter.  The parallel axis is along
// the row: lane l takes entries e0 + l, e0 + l + 64, ... of row i, so col_idx and
// R are read contiguously and P is a gather.
//   sweep 1   q = P[j] - R[e]; lane-local two smallest |q| and parity of q <= 0,
//             merged across lanes by a butterfly (the minima) and a ballot (the
//             parity).  Min, max and xor are exact, so the order does not matter.
//   sweep 2   the same q again (nothing of the row was written in between), the
//             new R[e] and P[j].  A column occurs once per row: no two lanes
//             write the same P.
// A workgroup barrier follows each row: the next row's gather reads what other
// lanes stored.  In a one-wave workgroup it is a wait, not a rendezvous.
// P[n] and R[E] live in LDS, or in this workgroup's slot of a scratch the graph
// handle owns (LayeredLayout); a slot is touched by its own workgroup only.  The
// syndrome (bytes) and the hard decision (bits for the parity test, bytes for
// finalize_shot) stay in LDS.  No global atomic beside the shot counter.
#include <hip/hip_runtime.h>

#include "qdec_block_steps.h"
#include "qdec_kernels.h"
#include "qdec_layered.h"

namespace qdec {

namespace {

// (m1, m2) of two sets of values from the sets' own (a1, a2), (b1, b2)
template <typename T>
__device__ __forceinline__ void merge_min2(T& m1, T& m2, T b1, T b2) {
    const T hi = fmax(m1, b1);
    m1 = fmin(m1, b1);
    m2 = fmin(hi, fmin(m2, b2));
}

}  // namespace

template <typename T, bool InHbm>
__global__ __launch_bounds__(kWave) void layered_wave_kernel(DevGraph g, LayeredArgs a, LayeredLayout L,
                                                             unsigned char* scratch) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int PREC = sizeof(T) == 4 ? 1 : 0;
    const int m = g.m, n = g.n, E = g.E, lane = threadIdx.x;
    long long* next_s = reinterpret_cast<long long*>(smem + kCtrlNext);
    uint8_t* sb = smem + L.l_sb;                                // [m_pad] syndrome bits
    uint64_t* xb = reinterpret_cast<uint64_t*>(smem + L.l_xb);  // [n_pad / 64] hard decision, bits
    uint8_t* xh = smem + L.l_xh;                                // [n_pad] hard decision, bytes
    unsigned char* msg = InHbm ? scratch + (size_t)blockIdx.x * (size_t)L.slot_bytes : smem + L.l_msg;
    T* P = reinterpret_cast<T*>(msg);
    T* R = reinterpret_cast<T*>(msg + L.o_R);
    const T* prior = reinterpret_cast<const T*>(g.prior[1][PREC]);
    const int32_t* rp = g.row_ptr;
    const int32_t* ci = g.col_idx;
    const T clip = (T)a.clip;

    for (int64_t shot = block_next_shot(a.work_ctr, next_s, lane); shot < a.B;
         shot = block_next_shot(a.work_ctr, next_s, lane)) {
        // the syndrome: a lane per row, or with base / readout terms lanes along the row
        if (!a.syn_flags) {
            for (int i = lane; i < m; i += kWave) sb[i] = (uint8_t)syn_bit(a.syn, shot, m, i);
        } else {
            for (int i = 0; i < m; ++i) {
                int t = 0;
                for (int e = rp[i] + lane; e < rp[i + 1]; e += kWave)
                    t ^= syn_term(a.syn_flags, a.base, a.readout, shot, g.n_data, ci[e]);
                const int s = syn_bit(a.syn, shot, m, i) ^ (__popcll(__ballot(t)) & 1);
                if (lane == 0) sb[i] = (uint8_t)s;
            }
        }
        for (int j = lane; j < n; j += kWave) P[j] = prior[j];
        for (int e = lane; e < E; e += kWave) R[e] = (T)0;
        __syncthreads();

        bool conv = false;
        int iters = 0;
        for (int it = 1; it <= a.max_iter && !conv; ++it) {
            const T alpha = alpha_at<T>(it, a.ms_scaling);
            for (int i = 0; i < m; ++i) {
                const int e0 = rp[i], e1 = rp[i + 1];
                if (e0 == e1) continue;  // uniform
                T m1 = Big<T>::v, m2 = Big<T>::v;
                int neg = 0;
                for (int e = e0 + lane; e < e1; e += kWave) {
                    const T q = P[ci[e]] - R[e];
                    const T av = fabs(q);
                    m2 = med3(av, m1, m2);
                    m1 = fmin(m1, av);
                    neg ^= q <= (T)0;
                }
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) merge_min2(m1, m2, __shfl_xor(m1, off), __shfl_xor(m2, off));
                const int par = (int)sb[i] ^ (__popcll(__ballot(neg)) & 1);
                const T m1a = m1 * alpha, m2a = m2 * alpha;
                for (int e = e0 + lane; e < e1; e += kWave) {
                    const int j = ci[e];
                    const T q = P[j] - R[e];
                    const T y = fmin((fabs(q) == m1) ? m2a : m1a, clip);
                    const T r = (par ^ (q <= (T)0)) ? -y : y;
                    R[e] = r;
                    P[j] = fmin(fmax(q + r, -clip), clip);
                }
                __syncthreads();  // this row's P before the next row's gather
            }
            ++iters;
            // the hard decision as bits, then every row's parity with lanes along the row
            for (int j0 = 0; j0 < g.n_pad; j0 += kWave) {
                const int j = j0 + lane;
                const uint64_t word = __ballot(j < n && P[j] <= (T)0);
                if (lane == 0) xb[j0 >> 6] = word;
            }
            __syncthreads();
            bool open = false;
            for (int i = 0; i < m && !open; ++i) {
                int t = 0;
                for (int e = rp[i] + lane; e < rp[i + 1]; e += kWave) {
                    const int j = ci[e];
                    t ^= (int)((xb[j >> 6] >> (j & 63)) & 1ull);
                }
                open = ((__popcll(__ballot(t)) & 1) ^ (int)sb[i]) != 0;  // uniform
            }
            conv = !open;
        }
        if (lane == 0 && a.iters) a.iters[shot] = iters;
        if (a.llr_out) {
            T* lo = reinterpret_cast<T*>(a.llr_out);
            for (int j = lane; j < n; j += kWave) lo[shot * n + j] = P[j];
        }
        for (int j = lane; j < n; j += kWave) xh[j] = (uint8_t)((xb[j >> 6] >> (j & 63)) & 1ull);
        __syncthreads();
        DecodeArgs fa{};
        fa.B = a.B;
        fa.base = a.base;
        fa.readout = a.readout;
        fa.x_out = a.x_out;
        fa.corr_out = a.corr_out;
        fa.status = a.status;
        fa.fail = a.fail;
        finalize_shot(g, fa, shot, xh, conv, conv, 0, lane);
        __syncthreads();
    }
}

void add_layered_kernels(KernelTable& t) {
    t.push_back(QDEC_INST(kWave, layered_wave_kernel, double, false));
    t.push_back(QDEC_INST(kWave, layered_wave_kernel, double, true));
    t.push_back(QDEC_INST(kWave, layered_wave_kernel, float, false));
    t.push_back(QDEC_INST(kWave, layered_wave_kernel, float, true));
}

const KernelTable& layered_table() {
    static const KernelTable table = [] {
        KernelTable t;
        add_layered_kernels(t);
        return t;
    }();
    return table;
}

void append_layered_kernel_names(std::string& out) {
    for (const KernelEntry& e : layered_table()) out += e.name + "\n";
}

// `grid` workgroups; with the beliefs in HBM `scratch` holds `grid` slots of
// L.slot_bytes, with them in LDS it is null
int launch_layered(const DevGraph& g, int precision, const LayeredArgs& a, const LayeredLayout& L, void* scratch,
                   int64_t grid, hipStream_t stream) {
    if (a.B <= 0 || grid <= 0) return 0;
    const bool hbm = scratch != nullptr;
    const KernelEntry* e = find_kernel(layered_table(), {precision, hbm ? 1 : 0});
    if (!e) return (int)hipErrorNotSupported;
    const size_t lds = (size_t)L.lds_bytes(hbm);
    if (lds > 64 * 1024) {
        const hipError_t ea = hipFuncSetAttribute(e->fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (ea != hipSuccess) return (int)ea;
    }
    using LayeredSig = KernelSig<DevGraph, LayeredArgs, LayeredLayout, unsigned char*>;
    return launch_entry(LayeredSig{}, *e, grid, lds, stream, g, a, L, static_cast<unsigned char*>(scratch));
}

}  // namespace qdec
