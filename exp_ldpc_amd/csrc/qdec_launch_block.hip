// qdec_launch_block.hip -- the workgroup half of the launch plan
// (plan_decode_block) and the launchers of the graphs no wave shape holds.  The
// kernels are defined one family per unit (qdec_bp_block.hip, qdec_bp_group.hip,
// qdec_ms_lds.hip, qdec_ms_lds64.hip) and reached through their table entries;
// their sizes and limits come from qdec_block_layout.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>

#include "qdec_block_layout.h"
#include "qdec_kernels.h"

namespace qdec {

// SSF + finalize of queued shots whose state fits LDS: the incremental kernel
// when the inverse table exists (QD_OPT_SSF_INC = 0 selects the re-scanning one).
int ssf_fin_path(const DevGraph& g, const DecodeArgs& a) {
    return a.ssf && g.g_iptr && g.n_gen <= 8192 && ssf_inc_lds(g) <= 160 * 1024 && g.opt_ssf_inc ? kFinIncBlock
                                                                                                : kFinBlockLds;
}

// ---------------------------------------------------------------- kernel tables
// Every instantiation of the workgroup families, one table per family, each
// filled by its family's unit (as wave_tables of qdec_launch_wave.hip).
// Argument order of the entries' t[]:
//   bp_block_kernel    T, METHOD, DEFER, DRM, DCM   (DRM = DCM = 0: loops over the degrees;
//                                                    16, 8: unrolled, row degree <= 16, column degree <= 8)
//   bp_group_kernel    T, METHOD, DR, DC            (DR in {8, 16} x DC in {4, 8}: the degrees it unrolls)
//   bp_ms_lds_kernel   VPT                          (columns per thread)
//   bp_ms_lds64_kernel VPT, D3R                     (D3R leading column rounds of degree <= 3)
// ssf[0] is ssf_inc_block_kernel, ssf[1] ssf_block_kernel.
struct BlockTables {
    KernelTable block, group, lds, lds64, ssf;
};
using BlockSig = KernelSig<DevGraph, DecodeArgs, void*, int>;  // gscratch is T*
using GroupSig = KernelSig<DevGraph, DecodeArgs, unsigned char*, size_t, const int32_t*, const int32_t*,
                           const int32_t*, const int32_t*, const int32_t*, const void*, const void*>;  // priors: const T*

static const BlockTables& block_tables() {
    static const BlockTables tables = [] {
        BlockTables t;
        add_block_kernels(t.block, t.ssf);
        add_group_kernels(t.group);
        add_ms_lds_kernels(t.lds);
        add_ms_lds64_kernels(t.lds64);
        return t;
    }();
    return tables;
}

void append_block_kernel_names(std::string& out) {
    const BlockTables& t = block_tables();
    for (const KernelTable* tab : {&t.block, &t.group, &t.lds, &t.lds64, &t.ssf})
        for (const KernelEntry& e : *tab) out += e.name + "\n";
}

const KernelEntry* ssf_block_entry(int path) {
    const BlockTables& t = block_tables();
    if (path == kFinIncBlock) return &t.ssf[0];
    return path == kFinBlockLds || path == kFinBlockHbm ? &t.ssf[1] : nullptr;
}

// The LDS-resident kernels: the smallest built VPT that holds the graph's
// columns (vpt per thread) and, with it, the largest built D3R <= the graph's
// leading rounds of degree <= 3 (f64; the f32 kernel has no D3R)
static const KernelEntry* pick_lds_kernel(const KernelTable& tab, int vpt, int d3r) {
    const KernelEntry* best = nullptr;
    for (const KernelEntry& e : tab) {
        if (e.t[0] < vpt || (e.nt > 1 && e.t[1] > d3r)) continue;
        if (!best || e.t[0] < best->t[0] || (e.t[0] == best->t[0] && e.nt > 1 && e.t[1] > best->t[1])) best = &e;
    }
    return best;
}

// the plan's SSF / finalize kernel; fin_state: the HBM shot state of kFinBlockHbm
static int launch_ssf_fin(const DevGraph& g, const DecodePlan& p, const DecodeArgs& a, int num_cus,
                          hipStream_t stream, unsigned char* fin_state = nullptr) {
    switch (p.ssf) {
        case kFinNone: return 0;
        case kFinIncBlock:
            return launch_entry_resident(WaveSig{}, *p.fin_k, p.fin_k->lds(g, a), num_cus, a.B, stream, {}, g, a);
        case kFinBlockLds:
            return launch_entry_resident(KernelSig<DevGraph, DecodeArgs, unsigned char*>{}, *p.fin_k,
                                         p.fin_k->lds(g, a), num_cus, a.B, stream, {}, g, a, nullptr);
        case kFinBlockHbm:  // the shot state in the scratch tail: the control area alone stays in LDS
            if (!fin_state) return (int)hipErrorInvalidValue;
            return launch_entry_resident(KernelSig<DevGraph, DecodeArgs, unsigned char*>{}, *p.fin_k, kCtrl, num_cus,
                                         a.B, stream, GridRule{kFinPerCu}, g, a, fin_state);
    }
    return (int)hipErrorNotSupported;
}

constexpr size_t kLdsMsgLimit = 64 * 1024;  // messages in LDS up to this (2 workgroups per CU)

// Where the BP workgroup keeps its state: messages in LDS when everything fits
// kLdsMsgLimit, else in HBM; the per-shot byte arrays stay in LDS up to
// kLdsMsgLimit (n ~ 6*10^4), beyond that (e.g. the 1.2*10^5-column spacetime
// graph of config 5) they move to the HBM slice as well.
inline int block_placement(const DevGraph& g, size_t tsz) {
    const size_t msg = ((size_t)2 * g.E * tsz + 15) / 16 * 16;
    const size_t small = (block_small_lds(g) + 15) / 16 * 16;
    if (msg + small <= kLdsMsgLimit) return 3;
    return small <= kLdsMsgLimit ? 2 : 0;
}

// HBM shot state of the SSF/finalize workgroups (kFinBlockHbm: kFinPerCu
// workgroups per CU), at the tail of the message scratch
static size_t fin_hbm_bytes(const DevGraph& g, const DecodePlan& p, int num_cus) {
    return p.ssf == kFinBlockHbm ? (size_t)num_cus * kFinPerCu * block_state_stride(g) : 0;
}

static int launch_block(const DevGraph& g, const DecodePlan& p, const DecodeArgs& a0, int num_cus,
                        hipStream_t stream, void* scratch, size_t scratch_bytes) {
    const size_t tsz = p.precision == 1 ? 4 : 8;
    const size_t msg = ((size_t)2 * g.E * tsz + 15) / 16 * 16;
    const size_t small = (block_small_lds(g) + 15) / 16 * 16;
    const int placement = p.placement;
    // placement 0: control area + the hard-decision bits of the unrolled kernel
    const size_t lds = (placement & 2) ? small + ((placement & 1) ? msg : 0) : kCtrl + (size_t)g.n_pad / 8;
    int cap = 0;
    void* gs = nullptr;
    DecodeArgs a = a0;
    const size_t fin_bytes = fin_hbm_bytes(g, p, num_cus);
    if (placement != 3) {
        // scratch = header (dynamic shot counter) + per-workgroup slices in HBM
        const size_t per_wg = block_slice_bytes(g, tsz, placement);
        if (!scratch || per_wg == 0 || scratch_bytes <= kGrpHeader + fin_bytes) return (int)hipErrorInvalidValue;
        const long long max_wg = (long long)((scratch_bytes - kGrpHeader - fin_bytes) / per_wg);
        // the grid is num_cus * cap workgroups, each owning one slice: at least
        // one slice per CU (block_scratch_bytes sizes 4 per CU)
        if (max_wg < num_cus) return (int)hipErrorOutOfMemory;
        cap = (int)(max_wg / num_cus);
        // Resident workgroups per CU.  With the shot state in HBM too (placement
        // 0, the C5 spacetime graph: 3.3 MB of slices per shot) the scattered
        // message accesses of more resident shots only add HBM traffic: on C5 at
        // p = 0.005, 4 / 3 / 2 / 1 per CU ran 18.0 / 20.8 / 26.3 / 19.2 k shots/s
        // (scattered writes), 23.9 / 27.1 / 29.3 k (contiguous writes, vcsc), so
        // placement 0 runs 2.  QD_OPT_BLOCK_WG overrides.
        if (placement == 0) cap = std::min(cap, 2);
        if (g.opt_block_wg > 0) cap = std::min((int)(max_wg / num_cus), g.opt_block_wg);
        a.work_ctr = static_cast<unsigned long long*>(scratch);
        gs = static_cast<unsigned char*>(scratch) + kGrpHeader;
        const hipError_t e0 = hipMemsetAsync(a.work_ctr, 0, sizeof(unsigned long long), stream);
        if (e0 != hipSuccess) return (int)e0;
    }
    const GridRule rule{cap};
    if (p.ssf == kFinNone) {
        record_ev(a, 0, stream);
        const int rc = launch_entry_resident(BlockSig{}, *p.bp_k, lds, num_cus, a.B, stream, rule, g, a, gs, placement);
        record_ev(a, 1, stream);
        record_ev(a, 2, stream);
        return rc;
    }
    if (!a.q_count || !a.q_idx || !a.q_x || !a.q_r) return (int)hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(a.q_count, 0, sizeof(int32_t), stream);
    if (e != hipSuccess) return (int)e;
    record_ev(a, 0, stream);
    int rc = launch_entry_resident(BlockSig{}, *p.bp_k, lds, num_cus, a.B, stream, rule, g, a, gs, placement);
    record_ev(a, 1, stream);
    if (rc != 0) return rc;
    rc = launch_ssf_fin(g, p, a, num_cus, stream,
                        fin_bytes ? static_cast<unsigned char*>(scratch) + (scratch_bytes - fin_bytes) : nullptr);
    record_ev(a, 2, stream);
    return rc;
}

// ---------------------------------------------------------------- LDS-resident launch
// QD_OPT_LDS_KERNEL = 0 disables bp_ms_lds_kernel / bp_ms_lds64_kernel, 1 forces
// them on any graph they can hold (also those whose messages fit the small-graph
// LDS budget); by default they take the min-sum graphs whose messages would go
// to HBM (f32: edge slots <= 160 KB; f64: n <= 10240 and the check states <= 160 KB).
static bool lds_kernel_applies(const DevGraph& g, const DecodePlan& p, const DecodeArgs& a) {
    const int precision = p.precision;
    if (p.method != 1 || !g.ml_etab || (precision == 0 && (!g.m64_etab || !g.m64_check))) return false;
    if (!a.syn || a.syn_flags || a.llr_out) return false;
    if (precision == 0) {  // bp_ms_lds64_kernel (automatic: graphs whose messages would go to HBM)
        if (g.n > 10 * kM64Threads || g.m <= 0 || g.m > kM64Nch * kM64Threads || a.max_iter < 1) return false;
        if (m64_lds_bytes(g) > 160 * 1024 || p.placement == 0) return false;
        if (g.opt_lds_kernel == 0) return false;
        return g.opt_lds_kernel == 1 || p.placement != 3;
    }
    if (precision != 1) return false;
    if (g.n > 16 * kMlThreads || g.m <= 0 || g.m > kMlNch * kMlThreads || a.max_iter < 1 ||
        ml_lds_bytes(g) > 160 * 1024)
        return false;
    if (p.placement == 0) return false;  // the SSF/finalize state would not fit LDS
    if (g.opt_lds_kernel == 0) return false;
    if (g.opt_lds_kernel == 1) return true;
    return p.placement != 3;
}

// the BP stage by the kernels' own unit (iteration 1's image into the scratch: f64 check
// states, f32 c2v rows), then SSF / finalize of the queue
static int launch_lds(const DevGraph& g, const DecodePlan& p, const DecodeArgs& a, int num_cus, hipStream_t stream,
                      void* scratch, size_t scratch_bytes) {
    if (!a.q_count || !a.q_idx || !a.q_x || !a.q_r || !a.wave_ctr) return (int)hipErrorInvalidValue;
    const int le = p.precision == 0 ? launch_ms_lds64(g, p, a, num_cus, stream,
                                                      reinterpret_cast<unsigned long long*>(scratch), scratch_bytes)
                                    : launch_ms_lds(g, p, a, num_cus, stream, reinterpret_cast<float*>(scratch),
                                                    scratch_bytes);
    if (le != 0) return le;
    const int rc = launch_ssf_fin(g, p, a, num_cus, stream);
    record_ev(a, 2, stream);
    return rc;
}

// ---------------------------------------------------------------- slot-group launch
// HBM budget of one handle's group scratch: QD_OPT_GROUP_MB when set, else
// a quarter of the device memory free right now (a bpssf_hybrid pipeline holds
// two such handles; the batch cap in group_count keeps small decodes small)
static size_t group_scratch_budget(const DevGraph& g) {
    if (g.opt_group_mb > 0) return (size_t)std::max(64, g.opt_group_mb) << 20;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || free_b == 0) return (size_t)4 << 30;
    return std::max<size_t>(free_b / 4, (size_t)64 << 20);
}

// resident slot groups per CU of a bp_group_kernel entry (asked once per entry)
static int group_per_cu(const KernelEntry& k) {
    static std::atomic<int> per_cu[16];
    std::atomic<int>& slot = per_cu[&k - block_tables().group.data()];
    int v = slot.load(std::memory_order_relaxed);
    if (v == 0) {
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, k.fn, k.block, 0) != hipSuccess) v = 1;
        v = std::max(v, 1);
        slot.store(v, std::memory_order_relaxed);
    }
    return v;
}

// Groups in flight: as many as the planned kernel's occupancy keeps resident,
// capped by the scratch budget and by the batch (every slot should see >= 2
// shots, so the tail of a launch stays short and small test batches stay
// small).  The scratch is sized from exactly this count (block_scratch_bytes).
static int64_t group_count(const DevGraph& g, const DecodePlan& p, int num_cus, int64_t B) {
    const size_t per = group_layout(g, p.precision == 1 ? 4 : 8).total;
    int64_t c = std::min<int64_t>((int64_t)num_cus * group_per_cu(*p.bp_k),
                                  (int64_t)(group_scratch_budget(g) / per));
    c = std::min<int64_t>(c, (B + 127) / 128);
    return std::max<int64_t>(c, 1);
}

// The slot-group kernel takes min-sum and product-sum graphs whose messages do
// not fit the small-graph LDS budget (row degree <= 16, column degree <= 8, the
// syndrome given directly).  QD_OPT_GROUP_KERNEL = 0 disables it (workgroup kernel
// with HBM message slices), =1 forces it on any graph within those degrees.
// For fp32 min-sum graphs the LDS-resident kernel (bp_ms_lds_kernel) keeps
// precedence unless the group kernel is forced.
static bool group_kernel_applies(const DevGraph& g, const DecodePlan& p, const DecodeArgs& a) {
    if (g.max_rdeg > 16 || g.max_cdeg > 8 || !a.syn || a.syn_flags) return false;
    if (g.opt_group_kernel == 0) return false;
    if (g.opt_group_kernel == 1) return true;
    return p.placement != 3;
}

static int launch_group(const DevGraph& g, const DecodePlan& p, const DecodeArgs& a, int num_cus,
                        hipStream_t stream, void* scratch, size_t scratch_bytes) {
    const size_t gb = group_layout(g, p.precision == 1 ? 4 : 8).total;
    const size_t fin_bytes = fin_hbm_bytes(g, p, num_cus);
    if (!scratch || scratch_bytes < fin_bytes + kGrpHeader + gb) return (int)hipErrorOutOfMemory;
    unsigned char* base = static_cast<unsigned char*>(scratch);
    unsigned char* fin_state = fin_bytes ? base + (scratch_bytes - fin_bytes) : nullptr;
    const int64_t max_groups = (int64_t)((scratch_bytes - fin_bytes - kGrpHeader) / gb);
    const KernelEntry& k = *p.bp_k;
    long long grid = 0;
    hipError_t e = resident_grid(k.fn, k.block, 0, num_cus,
                                 std::min<int64_t>(max_groups, group_count(g, p, num_cus, a.B)), &grid);
    if (e != hipSuccess) return (int)e;
    if (grid <= 0) return (int)hipErrorOutOfMemory;
    e = hipMemsetAsync(base, 0, sizeof(unsigned long long), stream);  // shot counter
    if (e != hipSuccess) return (int)e;
    if (a.ssf) {
        if (!a.q_count || !a.q_idx || !a.q_x || !a.q_r) return (int)hipErrorInvalidValue;
        e = hipMemsetAsync(a.q_count, 0, sizeof(int32_t), stream);
        if (e != hipSuccess) return (int)e;
    }
    record_ev(a, 0, stream);
    last_launch_names().bp = noted_name(&k);
    const int le = launch_entry(GroupSig{}, k, grid, 0, stream, g, a, base, gb, g.row_ptr, g.col_idx, g.col_ptr,
                                g.col_edge, g.edge_csc, g.prior[p.method][p.precision], g.eprior[p.method][p.precision]);
    record_ev(a, 1, stream);
    if (le != 0) return le;
    const int rc = launch_ssf_fin(g, p, a, num_cus, stream, fin_state);
    record_ev(a, 2, stream);
    return rc;
}

// The workgroup half of plan_decode.  The slot-group kernel has precedence over
// the workgroup kernel; the LDS-resident kernels over both unless the group
// kernel is forced.  The LDS-resident kernels finalize through the queue even
// without SSF.
void plan_decode_block(const DevGraph& g, const DecodeArgs& a, DecodePlan& p) {
    p.placement = block_placement(g, p.precision == 1 ? 4 : 8);
    const bool lds = lds_kernel_applies(g, p, a);
    const bool group = group_kernel_applies(g, p, a) && !(lds && g.opt_group_kernel != 1);
    p.bp = group ? kBpGroup : lds ? kBpLds : kBpBlock;
    p.ssf = !a.ssf && p.bp != kBpLds ? kFinNone : p.placement == 0 ? kFinBlockHbm : ssf_fin_path(g, a);
    p.expand_packed = a.in_packed != 0;
    p.need_scratch = p.bp != kBpBlock || p.placement != 3;

    // ---- the instantiation of every stage ----
    const BlockTables& t = block_tables();
    if (p.bp == kBpGroup) {
        p.bp_k = find_kernel(t.group, {p.precision, p.method, g.max_rdeg <= 8 ? 8 : 16, g.max_cdeg <= 4 ? 4 : 8});
    } else if (p.bp == kBpLds) {
        p.bp_k = p.precision == 0
                     ? pick_lds_kernel(t.lds64, (g.n + kM64Threads - 1) / kM64Threads, g.m64_d3r)
                     : pick_lds_kernel(t.lds, (g.n + kMlThreads - 1) / kMlThreads, 0);
    } else {
        // graphs with row degree <= 16 and column degree <= 8: unrolled loops
        const bool unr = g.max_rdeg <= 16 && g.max_cdeg <= 8;
        p.bp_k = find_kernel(t.block, {p.precision, p.method, p.ssf != kFinNone, unr ? 16 : 0, unr ? 8 : 0});
    }
    p.fin_k = ssf_block_entry(p.ssf);
    if (!p.bp_k) p.missing = "workgroup BP kernel";
}

size_t block_scratch_bytes(const DevGraph& g, const DecodePlan& p, int num_cus, const DecodeArgs& a) {
    const size_t tsz = p.precision == 1 ? 4 : 8;
    const size_t fin = fin_hbm_bytes(g, p, num_cus);
    switch (p.bp) {
        case kBpGroup:
            return kGrpHeader + (size_t)group_count(g, p, num_cus, a.B) * group_layout(g, tsz).total + fin;
        case kBpLds:
            // iteration 1's image (f64: check states, m64_init_kernel; f32: c2v rows, ml_init_*_kernel)
            return p.precision == 0 ? m64_image_bytes(g) : ml_image_bytes(g);
        case kBpBlock:
            if (p.placement == 3) return 0;
            // shot-counter header + up to 4 workgroup slices per CU (+ the SSF/finalize
            // shot state when it lives in HBM)
            return kGrpHeader + (size_t)num_cus * 4 * block_slice_bytes(g, tsz, p.placement) + fin;
    }
    return 0;  // wave graphs
}

// The smallest scratch a launch can run with (one slot group, or one workgroup
// slice per CU); block_scratch_bytes' figure may be cut down to it when the
// allocation fails (fewer groups / slices in flight, same results).
size_t block_scratch_floor(const DevGraph& g, const DecodePlan& p, int num_cus, const DecodeArgs& a) {
    const size_t full = block_scratch_bytes(g, p, num_cus, a);
    if (p.bp != kBpGroup) return full;  // workgroup slices: the launch needs its per-CU slices
    const size_t tsz = p.precision == 1 ? 4 : 8;
    return std::min(full, kGrpHeader + group_layout(g, tsz).total + fin_hbm_bytes(g, p, num_cus));
}

int launch_decode_block(const DevGraph& g, const DecodePlan& p, const DecodeArgs& a, int num_cus,
                        hipStream_t stream, void* scratch, size_t scratch_bytes) {
    if (a.B <= 0) return 0;
    if (a.ssf && g.n_gen <= 0) return (int)hipErrorInvalidValue;
    switch (p.bp) {
        case kBpGroup: return launch_group(g, p, a, num_cus, stream, scratch, scratch_bytes);
        case kBpLds: return launch_lds(g, p, a, num_cus, stream, scratch, scratch_bytes);
        case kBpBlock: return launch_block(g, p, a, num_cus, stream, scratch, scratch_bytes);
    }
    return (int)hipErrorNotSupported;
}

int launch_ssf_block(const DevGraph& g, const DecodePlan& p, const DecodeArgs& a, int num_cus, hipStream_t stream) {
    return launch_ssf_fin(g, p, a, num_cus, stream);
}

#ifdef QDEC_STAMPS
extern "C" __attribute__((visibility("default"))) int qd_dev_read_stamps_block(unsigned long long* out, int n,
                                                                              int reset) {
    unsigned long long h[64] = {0};
    if (read_stamps_ms_lds64(h, reset) != 0) return -1;
    for (int i = 0; i < n && i < 64; ++i) out[i] = h[i];
    return 0;
}
#endif

}  // namespace qdec
