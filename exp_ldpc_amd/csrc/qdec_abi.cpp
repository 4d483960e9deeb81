// qdec_abi.cpp -- extern "C" entry points of libqdec_hip.so (include/qdec.h)
// on graph handles; qdec_abi_circuit.cpp has those of compiled circuits.
//
// The graph handle: its tables come from the host builders (qdec_tables.cpp)
// through a device sink (qdec_abi.h); this file owns the streams, events,
// workspaces and launches.  No C++ exception crosses the ABI.
#include "qdec_abi.h"

using namespace qdec;

// the builders' HostGraph (tables, host CSR / CSC copies, sinks) plus the
// runtime state of the handle
struct qd_graph : HostGraph {
    int device = 0;
    int num_cus = 0;
    hipStream_t stream = nullptr;
    bool has_priors = false;   // BP priors: every probability inside (0, 1)
    bool has_thr = false;      // qd_graph_set_priors succeeded: the fault sampler's thresholds exist
    // workspace for the host-buffer API (bytes)
    DevBuf ws;
    // SSF work queue scratch (shots): count | idx[B] | x[B][n] | r[B][m]
    DevBuf qws;
    // HBM message scratch for the workgroup kernels on graphs too large for LDS
    MessageScratch mws;
    // QD_INPUT_PACKED decodes off the two-pass path: the inputs expanded to
    // byte rows (bytes; DecodeArgs::unpack_buf)
    DevBuf ubuf;
    // compact-list segment counters, two sets (DecodeArgs::cmp_count_next):
    // two-pass decodes alternate between them, each triage zeroing the other
    void* cmpc = nullptr;
    int cmp_par = 0;
    // kernel timing ring (qd_graph_set_timing): 3 events per decode call
    // [0..3] around the launch's kernels (record_ev), [4] behind the copy of
    // the compact-list counters (note_listed): kTimingEvents per call
    std::vector<hipEvent_t> tev;
    int t_cap = 0, t_count = 0;
    // per timed call: compact-list length of a two-pass launch (summed segment
    // counters, copied into pinned memory behind the launch), -1 otherwise
    uint64_t* t_listed = nullptr;  // [t_cap][kCmpLists * kCmpSegs], hipHostMalloc
    std::vector<int> t_cmp;
    // workspace chain: every device-buffer decode records it on its stream after
    // its launches, so the queue and message scratch of one handle are never
    // used by two streams at once (ws_drain before a grow path frees a buffer)
    StreamChain ws_chain;
    // 256-B control block: [0] shot-chunk counter of the min-sum wave kernel
    void* ctl = nullptr;
    // qd_graph_set_ssf_stream: SSF kernels of device-buffer decodes go to this
    // stream behind ssf_ev (nullptr: the decode's own stream)
    hipStream_t ssf_stream = nullptr;
    hipEvent_t ssf_ev = nullptr;
    // split-SSF decodes alternate between two SSF queues (queue 1: qws2, the
    // SSF region of the layout; control words ctl + 32 * q), so a decode waits
    // for the SSF kernel of the decode two back on this handle, not the last
    // one: ssf_done[q] is recorded on the SSF stream behind the kernel that
    // used queue q
    DevBuf qws2;  // (shots)
    int q_buf = 0;
    hipEvent_t ssf_done[2] = {nullptr, nullptr};
    bool ssf_done_live[2] = {false, false};
    // slot scratch of osd_hbm_kernel: one slot per workgroup (slots_cfg: qd_osd_set_slots)
    ChainedSlots osd_ws;
    // relay stage (qd_graph_set_relay): the caller's parameters and strengths, kept
    // to rebuild the tables when the priors change; the tables (relay_ok: built
    // from BP priors); the slot scratch of the HBM placement, whose chain orders
    // the launches of both placements (slots_cfg: qd_relay_set_slots); and the
    // launches' shot counter
    bool relay_set = false, relay_ok = false;
    RelayParams relay_p{};
    std::vector<double> relay_gammas;
    std::unique_ptr<TableSink> relay_arena;
    RelayTables relay_t{};
    ChainedSlots relay_ws;
    void* relay_ctr = nullptr;
    // layered BP (qd_layered_batch*): the slot scratch of the HBM placement, whose
    // chain orders the launches of both placements (slots_cfg:
    // qd_layered_set_slots), and the launches' shot counter
    ChainedSlots layered_ws;
    void* layered_ctr = nullptr;
    // kernels the last decode on this handle launched (qd_graph_last_kernels)
    std::string last_bp, last_ssf, last_pre;
    // qd_graph_create_host: tables only, no device, no stream; decodes refuse it
    bool host_only = false;
    // hypergraph-product kernel (qd_graph_hgp_*): plan once per graph
    HgpPlan* hgp = nullptr;
    bool hgp_tried = false;
};

namespace {

constexpr int kTimingEvents = 5;
constexpr size_t kCtlBytes = 512;  // control words: queue q's at ctl + 32 q (u64), the HGP counter at 16

void set_device(qd_graph* g) {
    if (!g->host_only) hip_check(hipSetDevice(g->device), "hipSetDevice");
}

// the last users of the queues, message scratch and unpack buffer: the
// workspace chain and the SSF kernels of split decodes
void ws_drain(qd_graph* G) {
    G->ws_chain.drain();
    for (int q = 0; q < 2; ++q)
        if (G->ssf_done_live[q]) hip_check(hipEventSynchronize(G->ssf_done[q]), "hipEventSynchronize");
}

// Attach the queue scratch (capacity >= B shots) when the plan asks for the SSF
// queue or the compact shot lists; one buffer holds both (queue_layout).  s is
// the stream the decode's kernels go to.
void attach_queue(qd_graph* G, const DecodePlan& plan, DecodeArgs& a, hipStream_t s) {
    const DevGraph& g = G->dg;
    if (a.B <= 0 || (!plan.need_queue && !plan.need_lists)) return;
    if ((size_t)a.B > G->qws.cap)  // launches still in flight may use the old queue
        G->qws.regrow(a.B, queue_layout(g, a.B).bytes, "hipFree queue", "hipMalloc queue", [&] { ws_drain(G); });
    const QueueLayout L = queue_layout(g, G->qws.cap);
    auto* base = static_cast<uint8_t*>(G->qws.p);
    a.q_count = reinterpret_cast<int32_t*>(base);
    a.q_idx = reinterpret_cast<int64_t*>(base + L.idx);
    a.q_x = base + L.x;
    a.q_r = base + L.r;
    a.q_w = reinterpret_cast<uint64_t*>(a.q_x);
    if (plan.need_lists) {
        a.cmp_count = reinterpret_cast<unsigned long long*>(base + L.cmp_count);
        a.cmp = reinterpret_cast<uint64_t*>(base + L.cmp);
        a.cmp_cap = L.cmp_cap;
        // double-buffered counters (zeroed once here, then by each triage for
        // the next decode): no memset launch per decode.  Zeroed on the decode's
        // own stream: the handle's stream is non-blocking, so a memset on the
        // null stream is not ordered before the triage, which then adds to
        // whatever the allocation held and writes its list entries from there
        const size_t set = (size_t)kCmpLists * kCmpSegs * 128;
        if (!G->cmpc) {
            hip_check(hipMalloc(&G->cmpc, 2 * set), "hipMalloc list counters");
            hip_check(hipMemsetAsync(G->cmpc, 0, 2 * set, s), "hipMemsetAsync list counters");
            G->cmp_par = 0;
        }
        auto* c = static_cast<uint8_t*>(G->cmpc);
        a.cmp_count = reinterpret_cast<unsigned long long*>(c + (size_t)G->cmp_par * set);
        a.cmp_count_next = reinterpret_cast<unsigned long long*>(c + (size_t)(G->cmp_par ^ 1) * set);
    }
}

// The second SSF queue of split-SSF decodes (the SSF region of the layout:
// count, index, entries; the compact lists stay in the first buffer, which only
// the BP stage uses)
void attach_queue2(qd_graph* G, DecodeArgs& a) {
    if (!a.q_count) return;  // no queue for this launch
    const DevGraph& g = G->dg;
    if (G->qws2.cap < G->qws.cap) {
        const QueueLayout L = queue_layout(g, G->qws.cap);
        G->qws2.regrow(G->qws.cap, g.wave ? L.cmp_count : L.bytes, "hipFree queue 2", "hipMalloc queue 2",
                       [&] { ws_drain(G); });
    }
    const QueueLayout L = queue_layout(g, G->qws2.cap);
    auto* base = static_cast<uint8_t*>(G->qws2.p);
    a.q_count = reinterpret_cast<int32_t*>(base);
    a.q_idx = reinterpret_cast<int64_t*>(base + L.idx);
    a.q_x = base + L.x;
    a.q_r = base + L.r;
    a.q_w = reinterpret_cast<uint64_t*>(a.q_x);
}

// after a launch whose triage was enqueued: it used one counter set and zeroed
// the other, so the next two-pass decode takes the other set
void flip_counters(qd_graph* G, const DecodeArgs& a, bool triaged) {
    if (a.cmp_count_next && triaged) G->cmp_par ^= 1;
}

void* message_scratch(qd_graph* G, const DecodePlan& plan, const DecodeArgs& a, size_t* bytes) {
    const size_t need = plan.need_scratch ? block_scratch_bytes(G->dg, plan, G->num_cus, a) : 0;
    HipMem mem([&] { ws_drain(G); });
    return G->mws.acquire(mem, need, need ? block_scratch_floor(G->dg, plan, G->num_cus, a) : 0, bytes);
}

// byte rows for a packed decode whose plan expands them (every input the call
// passes: syn [B][m], base and readout [B][n_data], each region 16-B aligned)
void attach_unpack(qd_graph* G, const DecodePlan& plan, DecodeArgs& a) {
    if (!plan.need_unpack) return;
    const size_t need = unpack_region(a.B, G->dg.m) + 2 * unpack_region(a.B, G->dg.n_data) + 256;
    if (need > G->ubuf.cap)  // launches in flight may still read the old buffer
        G->ubuf.regrow(need, need, "hipFree unpack buffer", "hipMalloc unpack buffer", [&] { ws_drain(G); });
    a.unpack_buf = static_cast<uint8_t*>(G->ubuf.p);
}

void check_osd_placement(int32_t placement) {
    if (placement != QD_OSD_ONCHIP && placement != QD_OSD_HBM && placement != QD_OSD_AUTO)
        throw Fail(-44, "unknown OSD placement (0 on-chip, 1 HBM, 2 auto)");
}

// The slot scratch of osd_hbm_kernel: num_cus * kOsdHbmSlotsPerCu slots or
// qd_osd_set_slots, at most one per shot, within a quarter of the free device
// memory (-45 when that does not hold one slot); -46 when one slot is refused.
SlotRule osd_slot_rule(const qd_graph* G, const OsdHbmLayout& L) {
    return {(size_t)L.slot_bytes, (int64_t)G->num_cus * kOsdHbmSlotsPerCu, -46, "no memory for one OSD slot of ",
            -45, "one OSD slot of ", "hipMalloc OSD scratch", "hipFree OSD scratch"};
}

void check_relay_placement(int32_t placement) {
    if (placement != QD_RELAY_LDS && placement != QD_RELAY_HBM && placement != QD_RELAY_AUTO)
        throw Fail(-55, "unknown relay placement (0 LDS, 1 HBM, 2 auto)");
}

// The relay tables from the kept parameters and the current priors; a launch in
// flight may still read the old ones.
void build_relay(qd_graph* G) {
    if (!G->host_only) G->relay_ws.chain.drain();
    G->relay_arena->release();
    G->relay_ok = false;
    if (!G->bp_priors) return;
    const RelayParams& p = G->relay_p;
    const RelayHostTables t = relay_build_tables(p, G->relay_gammas.data(), G->dg.n, G->prior_ms64.data());
    RelayTables& rt = G->relay_t;
    rt.gamma[QD_F64] = G->relay_arena->upload(t.g64);
    rt.gamma[QD_F32] = G->relay_arena->upload(t.g32);
    rt.w = G->relay_arena->upload(t.w);
    rt.pre_iter = p.pre_iter, rt.num_sets = p.num_sets, rt.set_max_iter = p.set_max_iter;
    rt.stop_nconv = p.stop_nconv, rt.alpha = p.alpha, rt.clip = p.clip;
    G->relay_ok = true;
}

// the default grid with the messages in LDS: what a CU's LDS holds, at most kRelayLdsPerCu
int64_t relay_lds_grid(const qd_graph* G, const RelayLayout& L) {
    const int64_t per_cu = std::max<int64_t>(1, std::min<int64_t>(kRelayLdsPerCu, (int64_t)kRelayLdsMax / L.lds_bytes(false)));
    return G->relay_ws.slots_cfg > 0 ? G->relay_ws.slots_cfg : (int64_t)G->num_cus * per_cu;
}

void check_layered_placement(int32_t placement) {
    if (placement != QD_LAYERED_LDS && placement != QD_LAYERED_HBM && placement != QD_LAYERED_AUTO)
        throw Fail(-68, "unknown layered placement (0 LDS, 1 HBM, 2 auto)");
}

void note_kernels(qd_graph* G) {
    const LaunchNames& n = last_launch_names();
    G->last_bp = n.bp ? n.bp : "";
    G->last_ssf = n.ssf ? n.ssf : "";
    G->last_pre = n.pre ? n.pre : "";
}

// the one copy of a string into a caller's buffer: cut to len - 1 characters
// and terminated; returns the whole length
int64_t put_name(const std::string& v, char* out, int64_t len) {
    if (out && len > 0) {
        const size_t k = std::min(v.size(), (size_t)len - 1);
        std::memcpy(out, v.data(), k);
        out[k] = '\0';
    }
    return (int64_t)v.size();
}

// a stage whose instantiation the library does not build fails here, before anything is enqueued
void check_plan(const DecodePlan& plan) {
    if (plan.missing) throw Fail(-17, std::string("no built instantiation of the ") + plan.missing + " for this decode");
}

void attach_timing(qd_graph* G, DecodeArgs& a) {
    a.ev = nullptr;
    if (G->t_cap > 0 && G->t_count < G->t_cap) a.ev = &G->tev[(size_t)kTimingEvents * G->t_count++];
}

// after a timed launch: the compact list's length (the triage's segment
// counters, one per 128-B line) into the call's pinned slot, on the BP stream,
// with the call's event [4] behind the copy (read_timing_detail waits on it).
// A split SSF stream waits for that event too, so the workspace chain, which
// continues on the SSF stream, covers the copy: the next decode's triage never
// resets the counters while the copy still reads them.
void note_listed(qd_graph* G, const DecodePlan& plan, const DecodeArgs& a, hipStream_t s, hipStream_t chain) {
    if (!a.ev || !G->t_listed) return;
    const size_t slot = (size_t)(a.ev - G->tev.data()) / kTimingEvents;
    const bool cmp = plan.two_pass && a.cmp_count;
    G->t_cmp[slot] = cmp ? 1 : 0;
    if (cmp)
        hip_check(hipMemcpy2DAsync(G->t_listed + slot * kCmpLists * kCmpSegs, 8, a.cmp_count, 128, 8,
                                   kCmpLists * kCmpSegs,
                                   hipMemcpyDeviceToHost, s),
                  "hipMemcpy2DAsync list counters");
    hip_check(hipEventRecord(a.ev[4], s), "hipEventRecord");
    if (chain != s) hip_check(hipStreamWaitEvent(chain, a.ev[4], 0), "hipStreamWaitEvent");
}

void free_timing(qd_graph* G) {
    ws_drain(G);  // list-counter copies into t_listed may still be in flight
    for (hipEvent_t e : G->tev) (void)hipEventDestroy(e);
    G->tev.clear();
    if (G->t_listed) (void)hipHostFree(G->t_listed);
    G->t_listed = nullptr;
    G->t_cmp.clear();
    G->t_cap = G->t_count = 0;
}

void check_graph(const qd_graph* g) {
    if (!g) throw Fail(-1, "null graph handle");
}

void check_params(const qd_graph* g, const qd_params* p) {
    if (g->host_only) throw Fail(-16, "host-only graph (qd_graph_create_host): no device to decode on");
    if (!p) throw Fail(-2, "null params");
    if (p->method != QD_MIN_SUM && p->method != QD_PRODUCT_SUM) throw Fail(-3, "unknown BP method");
    if (p->precision != QD_F32 && p->precision != QD_F64) throw Fail(-4, "unknown precision");
    if (!g->has_priors && g->has_thr)
        throw Fail(-51, "the graph's priors hold a 0 or a 1: it samples faults, BP needs probabilities inside (0, 1)");
    if (!g->has_priors) throw Fail(-5, "priors not set (qd_graph_set_priors)");
    if (p->ssf && g->dg.n_gen <= 0) throw Fail(-6, "SSF requested but the graph has no flip sets");
}

DecodeArgs make_args(const qd_graph* g, const qd_params* p, int64_t B, const uint8_t* syn, const uint8_t* base,
                     const uint8_t* readout, uint8_t* x_out, uint8_t* corr_out, void* llr_out, int32_t* iters,
                     uint8_t* status, int32_t* ssf_steps, uint8_t* fail) {
    DecodeArgs a{};
    a.B = B;
    a.max_iter = p->max_iter > 0 ? p->max_iter : g->dg.n;
    a.ssf = p->ssf ? 1 : 0;
    a.ssf_max_steps = p->ssf_max_steps;
    a.syn_flags = p->syn_flags & 3;
    a.in_packed = (p->syn_flags & QD_INPUT_PACKED) ? 1 : 0;
    if (a.in_packed && (((uintptr_t)syn | (uintptr_t)base | (uintptr_t)readout) & 7))
        throw Fail(-9, "QD_INPUT_PACKED rows must be 8-B aligned");
    a.ms_scaling = p->ms_scaling;
    a.syn = syn;
    a.base = base;
    a.readout = readout;
    a.x_out = x_out;
    a.corr_out = corr_out;
    a.llr_out = llr_out;
    a.iters = iters;
    a.status = status;
    a.ssf_steps = ssf_steps;
    a.fail = fail;
    if (!syn && !(a.syn_flags && (base || readout))) throw Fail(-7, "no syndrome source");
    if (!g->ctl) hip_check(hipMalloc(&const_cast<qd_graph*>(g)->ctl, kCtlBytes), "hipMalloc control block");
    a.wave_ctr = static_cast<unsigned long long*>(g->ctl);
    a.ssf_nosplit = g->dg.opt_ssf == kSsfScanNoSplit ? 1 : 0;
    return a;
}

// Enqueue one decode on stream s: scratch buffers, workspace chain, launch,
// bookkeeping.  allow_split: SSF may go to the handle's SSF stream
// (qd_graph_set_ssf_stream); the host-buffer path never splits, since it
// copies the results back on s right behind the launch.
void enqueue_decode(qd_graph* G, const qd_params* p, DecodeArgs& a, hipStream_t s, bool allow_split) {
    const DecodePlan plan = plan_decode(G->dg, p->method, p->precision, a);
    check_plan(plan);
    attach_queue(G, plan, a, s);
    attach_unpack(G, plan, a);
    attach_timing(G, a);
    size_t sb = 0;
    void* scr = message_scratch(G, plan, a, &sb);
    const bool split = allow_split && G->ssf_stream && G->ssf_stream != s && a.ssf;
    const int qb = split ? G->q_buf : 0;
    if (split) {
        a.ssf_stream = G->ssf_stream;
        a.ssf_ev = G->ssf_ev;
        if (qb == 1) attach_queue2(G, a);
        a.wave_ctr = static_cast<unsigned long long*>(G->ctl) + 32 * qb;
    }
    G->ws_chain.acquire(s);
    // an SSF kernel still running on the SSF stream must have finished before
    // its queue and control words are reset: a split decode reuses those of the
    // split decode two back on this handle (queue qb); an unsplit one uses queue
    // 0 and the first control words, which either split queue's kernel may hold
    for (int q = 0; q < 2; ++q)
        if (G->ssf_done_live[q] && (!split || q == qb))
            hip_check(hipStreamWaitEvent(s, G->ssf_done[q], 0), "hipStreamWaitEvent");
    bool triaged = false;
    const int rc = launch_decode(G->dg, plan, a, G->num_cus, s, scr, sb, &triaged);
    note_kernels(G);
    flip_counters(G, a, triaged);  // also after a failed BP launch: its triage zeroed the other set
    if (rc != 0) throw Fail(-101, std::string("decode launch failed: ") + hipGetErrorString((hipError_t)rc));
    note_listed(G, plan, a, s, s);
    if (split) {  // the SSF kernel runs on its own stream behind this decode's BP
        if (!G->ssf_done[qb])
            hip_check(hipEventCreateWithFlags(&G->ssf_done[qb], hipEventDisableTiming), "hipEventCreate");
        hip_check(hipEventRecord(G->ssf_done[qb], G->ssf_stream), "hipEventRecord");
        G->ssf_done_live[qb] = true;
        G->q_buf ^= 1;
    }
    // the workspace chain (message scratch, compact lists, counters) ends with
    // the BP stage; the SSF queues are ordered by ssf_done
    G->ws_chain.release(s);
}

// Both graph constructors: validate the CSR, then build every graph table into
// device memory on `device`, or (host_only) into host copies with no HIP call.
int create_graph(int32_t m, int32_t n, const int32_t* row_ptr, const int32_t* col_idx, int32_t n_data,
                 int32_t fold_blocks, bool host_only, int32_t device, qd_graph** out) {
    return guarded([&] {
        if (!out) throw Fail(-1, "null output handle");
        *out = nullptr;
        if (m <= 0 || n <= 0 || !row_ptr || !col_idx) throw Fail(-10, "invalid graph shape or null arrays");
        if (n_data <= 0 || fold_blocks <= 0 || (int64_t)n_data * fold_blocks > n)
            throw Fail(-11, "invalid fold (n_data * fold_blocks must be <= n)");
        if (row_ptr[0] != 0) throw Fail(-12, "row_ptr[0] must be 0");
        for (int i = 0; i < m; ++i) {
            if (row_ptr[i + 1] < row_ptr[i]) throw Fail(-12, "row_ptr not monotone");
            for (int e = row_ptr[i]; e < row_ptr[i + 1]; ++e) {
                if (col_idx[e] < 0 || col_idx[e] >= n) throw Fail(-13, "column index out of range");
                if (e > row_ptr[i] && col_idx[e] <= col_idx[e - 1])
                    throw Fail(-14, "column indices must be strictly ascending within a row");
            }
        }
        if (!host_only) {
            int ndev = 0;
            hip_check(hipGetDeviceCount(&ndev), "hipGetDeviceCount");
            if (device < 0 || device >= ndev) throw Fail(-15, "device ordinal out of range");
        }
        auto* G = new qd_graph();
        try {
            G->host_only = host_only;
            G->num_cus = 256;
            if (!host_only) {
                G->device = device;
                set_device(G);
                hipDeviceProp_t prop;
                hip_check(hipGetDeviceProperties(&prop, device), "hipGetDeviceProperties");
                G->num_cus = prop.multiProcessorCount;
                hip_check(hipStreamCreateWithFlags(&G->stream, hipStreamNonBlocking), "hipStreamCreate");
            }
            for (auto* sink : {&G->arena, &G->flip_arena, &G->lz_arena, &G->prior_arena}) {
                if (host_only) sink->reset(new HostSink());
                else sink->reset(new DeviceSink());
            }
            if (host_only) G->relay_arena.reset(new HostSink());
            else G->relay_arena.reset(new DeviceSink());
            init_graph(G, m, n, row_ptr, col_idx, n_data, fold_blocks);
        } catch (...) {
            if (G->stream) (void)hipStreamDestroy(G->stream);
            delete G;  // its sinks free the tables uploaded so far
            throw;
        }
        *out = G;
    });
}

}  // namespace

extern "C" {

int qd_abi_version(void) { return QDEC_ABI_VERSION; }

const char* qd_last_error(void) { return g_last_error.c_str(); }

int qd_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int qd_graph_create(int32_t m, int32_t n, const int32_t* row_ptr, const int32_t* col_idx, int32_t n_data,
                    int32_t fold_blocks, int32_t device, qd_graph** out) {
    return create_graph(m, n, row_ptr, col_idx, n_data, fold_blocks, false, device, out);
}

int qd_graph_create_host(int32_t m, int32_t n, const int32_t* row_ptr, const int32_t* col_idx, int32_t n_data,
                         int32_t fold_blocks, qd_graph** out) {
    return create_graph(m, n, row_ptr, col_idx, n_data, fold_blocks, true, 0, out);
}

int qd_graph_table_digest(const qd_graph* G, uint64_t* digest, int64_t* bytes) {
    return guarded([&] {
        check_graph(G);
        if (!G->host_only) throw Fail(-16, "table digests are kept for host-only graphs (qd_graph_create_host)");
        table_digest(G, digest, bytes);
    });
}

static HgpPlan* hgp_plan_of(qd_graph* G) {
    if (!G->hgp_tried) {
        G->hgp = hgp_plan_create(G->dg.m, G->dg.n, G->row_ptr, G->col_idx);
        G->hgp_tried = true;
    }
    return G->hgp;
}

int qd_graph_hgp_set_slots(qd_graph* G, int32_t slots) {
    return guarded([&] {
        check_graph(G);
        if (slots < 0 || slots > 64) throw Fail(-95, "slots out of range");
        if (!G->host_only) set_device(G);
        if (G->stream) hip_check(hipStreamSynchronize(G->stream), "hipStreamSynchronize");
        ws_drain(G);  // an HGP launch on another stream may still use the plan's module
        HgpPlan* P = hgp_plan_create(G->dg.m, G->dg.n, G->row_ptr, G->col_idx, slots);
        if (!P && slots > 0 && hgp_plan_of(G))  // a hypergraph product, but no feasible plan with `slots`
            throw Fail(-95, "no feasible HGP plan with this many slots per workgroup");
        hgp_plan_destroy(G->hgp);
        G->hgp = P;
        G->hgp_tried = true;
    });
}

int qd_graph_hgp_info(qd_graph* G, int32_t* out8) {
    int rc = 0;
    const int e = guarded([&] {
        check_graph(G);
        HgpPlan* P = hgp_plan_of(G);
        rc = P ? 1 : 0;
        if (P && out8) hgp_plan_info(P, out8);
    });
    return e ? e : rc;
}

int64_t qd_graph_hgp_source(qd_graph* G, char* buf, int64_t cap) {
    int64_t len = 0;
    const int e = guarded([&] {
        check_graph(G);
        HgpPlan* P = hgp_plan_of(G);
        if (!P) throw Fail(-90, "not a hypergraph-product check matrix");
        len = put_name(hgp_plan_source(P), buf, cap);
    });
    return e ? e : len;
}

#ifdef QDEC_DEV_HOOKS
// development build only (python -m exp_ldpc_amd.build --tag dev -DQDEC_DEV_HOOKS):
// compile an edited kernel source at run time (tools/gpu/hgp_debug.py)
int qd_graph_hgp_replace_source(qd_graph* G, const char* src) {
    return guarded([&] {
        check_graph(G);
        HgpPlan* P = hgp_plan_of(G);
        if (!P || !src) throw Fail(-90, "not a hypergraph-product check matrix");
        if (G->stream) hip_check(hipStreamSynchronize(G->stream), "hipStreamSynchronize");
        hgp_plan_replace_source(P, src);
    });
}
#endif

int qd_graph_hgp_compile(qd_graph* G) {
    return guarded([&] {
        check_graph(G);
        HgpPlan* P = hgp_plan_of(G);
        if (!P) throw Fail(-90, "not a hypergraph-product check matrix");
        std::string log;
        if (hgp_plan_compile(P, hgp_target_arch(G->host_only ? -1 : G->device).c_str(), &log) != 0)
            throw Fail(-91, "HGP kernel compile failed: " + log);
    });
}

int qd_graph_hgp_decode_bp(qd_graph* G, int64_t B, const uint8_t* syn, uint8_t* x_out, int32_t* iters,
                           uint8_t* status, int32_t max_iter, double ms_scaling, void* stream) {
    return guarded([&] {
        check_graph(G);
        if (G->host_only) throw Fail(-2, "host-only graph handle");
        set_device(G);
        HgpPlan* P = hgp_plan_of(G);
        if (!P) throw Fail(-90, "not a hypergraph-product check matrix");
        if (!G->has_priors) throw Fail(-51, "priors not set");
        if (B < 0 || (B > 0 && !syn) || max_iter < 1) throw Fail(-92, "invalid HGP decode arguments");
        if (hgp_plan_load(P, G->num_cus, hgp_target_arch(G->device).c_str()) != 0)
            throw Fail(-93, "HGP kernel load failed");
        if (!G->ctl) hip_check(hipMalloc(&G->ctl, kCtlBytes), "hipMalloc control block");
        if (B == 0) return;
        HgpBpArgs a{};
        a.syn = syn;
        a.prior = static_cast<const double*>(G->dg.prior[QD_MIN_SUM][QD_F64]);
        a.x_out = x_out;
        a.iters = iters;
        a.status = status;
        // its own shot counter on its own 128-B line (words 0 / 1 are the BP and
        // SSF kernels' counters), and inside the workspace chain like every decode
        a.counter = static_cast<unsigned long long*>(G->ctl) + 16;
        a.B = B;
        a.max_iter = max_iter;
        a.ms_scaling = ms_scaling;
        hipStream_t st = stream ? static_cast<hipStream_t>(stream) : G->stream;
        G->ws_chain.acquire(st);
        if (hgp_launch_bp(P, a, st) != 0) throw Fail(-94, "HGP kernel launch failed");
        hip_check(hipGetLastError(), "HGP kernel");
        G->ws_chain.release(st);
    });
}

int qd_graph_destroy(qd_graph* g) {
    return guarded([&] {
        if (!g) return;
        if (g->host_only) {
            hgp_plan_destroy(g->hgp);
            delete g;
            return;
        }
        (void)hipSetDevice(g->device);
        if (g->stream) (void)hipStreamSynchronize(g->stream);
        g->ws_chain.destroy();  // waits first; free_timing's drain is then a no-op
        for (int q = 0; q < 2; ++q)
            if (g->ssf_done[q]) {
                if (g->ssf_done_live[q]) (void)hipEventSynchronize(g->ssf_done[q]);
                (void)hipEventDestroy(g->ssf_done[q]);
                g->ssf_done[q] = nullptr;
                g->ssf_done_live[q] = false;
            }
        if (g->qws2.p) (void)hipFree(g->qws2.p);
        if (g->ssf_ev) (void)hipEventDestroy(g->ssf_ev);
        for (void* p : {g->ws.p, g->qws.p, g->mws.ptr, g->ubuf.p})
            if (p) (void)hipFree(p);
        g->osd_ws.destroy();  // an HBM OSD launch may still use its slots
        g->relay_ws.destroy();
        if (g->relay_ctr) (void)hipFree(g->relay_ctr);
        g->layered_ws.destroy();
        if (g->layered_ctr) (void)hipFree(g->layered_ctr);
        if (g->cmpc) (void)hipFree(g->cmpc);
        if (g->ctl) (void)hipFree(g->ctl);
        hgp_plan_destroy(g->hgp);
        free_timing(g);
        if (g->stream) (void)hipStreamDestroy(g->stream);
        delete g;  // its sinks free the tables
    });
}

// the table groups a handle can rebuild: the builders (qdec_tables.cpp) check
// the arguments and upload through the handle's sinks
int qd_graph_set_flipsets(qd_graph* G, int32_t n_gen, const int32_t* gen_ptr, const int32_t* gen_idx) {
    return guarded([&] {
        check_graph(G);
        set_device(G);
        set_flipsets(G, n_gen, gen_ptr, gen_idx);
    });
}

int qd_graph_set_logicals(qd_graph* G, int32_t k, const uint8_t* lz) {
    return guarded([&] {
        check_graph(G);
        set_device(G);
        set_logicals(G, k, lz);
    });
}

int qd_graph_set_logicals_csr(qd_graph* G, int32_t k, const int32_t* lz_ptr, const int32_t* lz_idx) {
    return guarded([&] {
        check_graph(G);
        set_device(G);
        set_logicals_csr(G, k, lz_ptr, lz_idx);
    });
}

int qd_graph_set_priors(qd_graph* G, const double* probs) {
    return guarded([&] {
        check_graph(G);
        set_device(G);
        if (!G->host_only) G->layered_ws.chain.drain();  // a layered launch may still read the old priors
        set_priors(G, probs);  // on a throw the previous tables and flags stand
        G->has_priors = G->bp_priors;
        G->has_thr = true;
        if (G->relay_set) build_relay(G);
    });
}

int qd_decode_batch_device(qd_graph* G, const qd_params* p, int64_t B, const uint8_t* syn, const uint8_t* base,
                           const uint8_t* readout, uint8_t* x_out, uint8_t* corr_out, void* llr_out, int32_t* iters,
                           uint8_t* status, int32_t* ssf_steps, uint8_t* fail, void* stream) {
    return guarded([&] {
        check_graph(G);
        check_params(G, p);
        if (B < 0) throw Fail(-8, "negative batch");
        if (B == 0) return;  // nothing to enqueue
        set_device(G);
        DecodeArgs a = make_args(G, p, B, syn, base, readout, x_out, corr_out, llr_out, iters, status, ssf_steps, fail);
        enqueue_decode(G, p, a, (hipStream_t)stream, true);
    });
}

int qd_decode_batch(qd_graph* G, const qd_params* p, int64_t B, const uint8_t* syn, const uint8_t* base,
                    const uint8_t* readout, uint8_t* x_out, uint8_t* corr_out, void* llr_out, int32_t* iters,
                    uint8_t* status, int32_t* ssf_steps, uint8_t* fail) {
    return guarded([&] {
        check_graph(G);
        check_params(G, p);
        if (B < 0) throw Fail(-8, "negative batch");
        if (B == 0) return;
        set_device(G);
        const DevGraph& g = G->dg;
        const size_t tsz = p->precision == QD_F32 ? 4 : 8;
        // input row bytes: one byte per bit, or whole u64 words (QD_INPUT_PACKED)
        const bool pk = (p->syn_flags & QD_INPUT_PACKED) != 0;
        const size_t syn_row = pk ? ((size_t)g.m + 63) / 64 * 8 : (size_t)g.m;
        const size_t dat_row = pk ? ((size_t)g.n_data + 63) / 64 * 8 : (size_t)g.n_data;
        HostStage st;  // regions 0-2 the inputs, 3-9 the outputs
        st.add(syn, (size_t)B * syn_row, "syn");
        st.add(base, (size_t)B * dat_row, "base");
        st.add(readout, (size_t)B * dat_row, "readout");
        st.add(x_out, (size_t)B * g.n, "x");
        st.add(corr_out, (size_t)B * g.n_data, "corr");
        st.add(llr_out, (size_t)B * g.n * tsz, "llr");
        st.add(iters, (size_t)B * 4, "iters");
        st.add(status, (size_t)B, "status");
        st.add(ssf_steps, (size_t)B * 4, "ssf_steps");
        st.add(fail, (size_t)B, "fail");
        st.place(G->ws);
        hipStream_t s = G->stream;
        st.copy(0, 3, true, s);
        DecodeArgs a = make_args(G, p, B, st.dev<uint8_t>(0), st.dev<uint8_t>(1), st.dev<uint8_t>(2), st.dev<uint8_t>(3),
                                 st.dev<uint8_t>(4), st.dev(5), st.dev<int32_t>(6), st.dev<uint8_t>(7),
                                 st.dev<int32_t>(8), st.dev<uint8_t>(9));
        enqueue_decode(G, p, a, s, false);  // SSF stays on s: the copies out follow it
        st.finish(3, s);
    });
}

static int sample_storage(qd_graph* G, int32_t rounds, double p_data, double p_meas, uint32_t seed,
                          uint32_t stream_id, int64_t shot0, int64_t B, uint8_t* syn, uint8_t* readout,
                          void* stream, bool packed) {
    return guarded([&] {
        check_graph(G);
        if (rounds < 0 || B < 0) throw Fail(-60, "invalid sampler arguments");
        if (B == 0) return;
        if (!syn || !readout) throw Fail(-60, "invalid sampler arguments");
        if (packed && (((uintptr_t)syn | (uintptr_t)readout) & 7)) throw Fail(-60, "packed rows must be 8-B aligned");
        if (G->dg.fold_blocks != 1 || G->dg.n_data != G->dg.n) throw Fail(-61, "sampler needs a plain code graph (H = Hz)");
        set_device(G);
        const int rc = launch_sample_storage(G->dg, rounds, bern_threshold(2.0 * p_data / 3.0), bern_threshold(p_meas),
                                             seed, stream_id, shot0, B, syn, readout, G->num_cus, (hipStream_t)stream,
                                             packed);
        if (rc != 0) throw Fail(-102, std::string("sampler launch failed: ") + hipGetErrorString((hipError_t)rc));
    });
}

int qd_sample_storage_device(qd_graph* G, int32_t rounds, double p_data, double p_meas, uint32_t seed,
                             uint32_t stream_id, int64_t shot0, int64_t B, uint8_t* syn, uint8_t* readout,
                             void* stream) {
    return sample_storage(G, rounds, p_data, p_meas, seed, stream_id, shot0, B, syn, readout, stream, false);
}

int qd_sample_storage_packed_device(qd_graph* G, int32_t rounds, double p_data, double p_meas, uint32_t seed,
                                    uint32_t stream_id, int64_t shot0, int64_t B, uint64_t* syn, uint64_t* readout,
                                    void* stream) {
    return sample_storage(G, rounds, p_data, p_meas, seed, stream_id, shot0, B, reinterpret_cast<uint8_t*>(syn),
                          reinterpret_cast<uint8_t*>(readout), stream, true);
}

int qd_sample_faults_device(qd_graph* G, uint32_t seed, uint32_t stream_id, int64_t shot0, int64_t B, int32_t flags,
                            void* det, void* faults, uint8_t* obs, void* stream) {
    return guarded([&] {
        check_graph(G);
        if (G->host_only) throw Fail(-16, "host-only graph (qd_graph_create_host): no device to sample on");
        if (B < 0 || (flags & ~QD_INPUT_PACKED)) throw Fail(-60, "invalid sampler arguments");
        const DevGraph& g = G->dg;
        if (!G->has_thr || !G->smp_thr) throw Fail(-63, "priors not set (qd_graph_set_priors): no fault probabilities");
        if (g.fold_blocks != 1 || g.n_data != g.n)
            throw Fail(-64, "fault sampler needs an unfolded graph (fold_blocks = 1, n_data = n)");
        if (B == 0) return;
        if (!det) throw Fail(-66, "null detector buffer");
        if (obs && g.k <= 0) throw Fail(-65, "observables requested but the graph has no logicals");
        const bool packed = (flags & QD_INPUT_PACKED) != 0;
        if (packed && (((uintptr_t)det | (uintptr_t)faults) & 7)) throw Fail(-67, "packed rows must be 8-B aligned");
        set_device(G);
        const int rc = launch_sample_faults(g, G->smp_thr, G->smp_crow, seed, stream_id, shot0, B, packed, det, faults,
                                            obs, G->num_cus, (hipStream_t)stream);
        if (rc != 0) throw Fail(-102, std::string("sampler launch failed: ") + hipGetErrorString((hipError_t)rc));
    });
}

int qd_graph_sample_tables_copy(const qd_graph* G, uint32_t* thr, int32_t* crow) {
    return guarded([&] {
        check_graph(G);
        if (!G->host_only) throw Fail(-16, "table copies are kept for host-only graphs (qd_graph_create_host)");
        sample_tables_copy(G, thr, crow);
    });
}

int qd_osd_device_supported(const qd_graph* G) {
    if (!G) return 0;
    return osd_kernel_supports(G->dg) ? 1 : 0;
}

int qd_osd_kernel_info(const qd_graph* G, int32_t out[3]) {
    OsdChoice c{0, 0, 0};
    const bool ok = G && osd_choose(G->dg, &c);
    if (out) {
        out[0] = c.rs;
        out[1] = c.w;
        out[2] = c.lds;
    }
    return ok ? 1 : 0;
}

int qd_osd_batch_device(qd_graph* G, int32_t method, int32_t order, int64_t B, const uint8_t* syn, int32_t syn_flags,
                        const void* llr, int32_t llr_precision, const uint8_t* status, const uint8_t* base,
                        const uint8_t* readout, uint8_t* osd0_out, uint8_t* osdw_out, uint8_t* corr_out, uint8_t* fail,
                        void* stream) {
    return qd_osd_batch_device_placed(G, method, order, B, syn, syn_flags, llr, llr_precision, status, base, readout,
                                      osd0_out, osdw_out, corr_out, fail, stream, QD_OSD_ONCHIP);
}

int qd_osd_batch_device_placed(qd_graph* G, int32_t method, int32_t order, int64_t B, const uint8_t* syn,
                               int32_t syn_flags, const void* llr, int32_t llr_precision, const uint8_t* status,
                               const uint8_t* base, const uint8_t* readout, uint8_t* osd0_out, uint8_t* osdw_out,
                               uint8_t* corr_out, uint8_t* fail, void* stream, int32_t placement) {
    return guarded([&] {
        check_graph(G);
        if (method < 0 || method > 2) throw Fail(-80, "osd method must be 0 (osd0), 1 (osd_e), 2 (osd_cs)");
        if (method == 1 && order > 20) throw Fail(-81, "osd_e order above 20 is not supported");
        if (method == 2 && order > 64) throw Fail(-82, "osd_cs order above 64 is not supported on the device");
        if (B < 0) throw Fail(-8, "negative batch");
        check_osd_placement(placement);
        if (B == 0) return;
        if (!llr || (!syn && !syn_flags)) throw Fail(-83, "null OSD inputs");
        if (llr_precision != QD_F32 && llr_precision != QD_F64) throw Fail(-84, "invalid llr precision");
        OsdPlaced pl;
        osd_place(G->dg, placement, &pl);
        if (pl.kernel == kOsdNone) {
            if (placement == QD_OSD_ONCHIP)
                throw Fail(-85, "graph too large for the device OSD (LDS image above 160 KiB)");
            throw Fail(-48, "graph too large for the HBM OSD kernel (its LDS part above 160 KiB, or k > 256)");
        }
        if (fail && G->dg.k > 256) throw Fail(-86, "fused failure check after OSD supports <= 256 logicals");
        if (G->host_only) throw Fail(-16, "host-only graph (qd_graph_create_host): no device to run OSD on");
        set_device(G);
        OsdArgs a{};
        a.B = B;
        a.method = method;
        a.order = order;
        a.syn_flags = syn_flags;
        a.llr_f32 = llr_precision == QD_F32 ? 1 : 0;
        a.syn = syn;
        a.llr = llr;
        a.status = status;
        a.base = base;
        a.readout = readout;
        a.osd0_out = osd0_out;
        a.osdw_out = osdw_out;
        a.corr_out = corr_out;
        a.fail = fail;
        int rc;
        if (pl.kernel != kOsdHbm) {
            rc = launch_osd(G->dg, a, G->num_cus, (hipStream_t)stream);
        } else {
            const int64_t slots = G->osd_ws.acquire(osd_slot_rule(G, pl.L), B, (hipStream_t)stream);
            rc = launch_osd_hbm(G->dg, a, G->osd_ws.ptr, slots, (hipStream_t)stream);
            G->osd_ws.release(slots, (hipStream_t)stream);
        }
        if (rc != 0) throw Fail(-104, std::string("osd launch failed: ") + hipGetErrorString((hipError_t)rc));
    });
}

int qd_osd_kernel_info_placed(const qd_graph* G, int32_t placement, int64_t out[4]) {
    int held = 0;
    const int rc = guarded([&] {
        if (out) out[0] = out[1] = out[2] = out[3] = 0;
        check_osd_placement(placement);
        if (!G) return;
        OsdPlaced pl;
        osd_place(G->dg, placement, &pl);
        if (pl.kernel == kOsdNone) return;
        held = 1;
        if (!out) return;
        out[0] = pl.kernel;
        if (pl.kernel == kOsdHbm)
            out[1] = 0, out[2] = pl.L.W, out[3] = pl.L.slot_bytes;
        else
            out[1] = pl.c.rs, out[2] = pl.c.w, out[3] = pl.c.lds;
    });
    return rc != 0 ? rc : held;
}

int qd_osd_set_slots(qd_graph* G, int64_t slots) {
    return guarded([&] {
        check_graph(G);
        if (slots < 0 || slots > (1ll << 20)) throw Fail(-47, "osd slots must be 0 (default) .. 2^20");
        G->osd_ws.slots_cfg = slots;
    });
}

int qd_osd_hbm_info(const qd_graph* G, int64_t out[3]) {
    return guarded([&] {
        check_graph(G);
        if (!out) throw Fail(-83, "null output");
        OsdHbmLayout L;
        out[0] = osd_hbm_choose(G->dg, &L) ? L.slot_bytes : 0;
        out[1] = G->osd_ws.slots_last;
        out[2] = (int64_t)G->osd_ws.bytes;
    });
}

int qd_graph_set_relay(qd_graph* G, const qd_relay_params* prm, const double* gammas) {
    static_assert(sizeof(qd_relay_params) == sizeof(RelayParams), "qd_relay_params and RelayParams");
    return guarded([&] {
        check_graph(G);
        const RelayParams* p = reinterpret_cast<const RelayParams*>(prm);
        relay_check_params(p, gammas, G->dg.n);
        if (!G->has_priors && G->has_thr)
            throw Fail(-51, "the graph's priors hold a 0 or a 1: relay needs probabilities inside (0, 1)");
        if (!G->has_priors) throw Fail(-5, "priors not set (qd_graph_set_priors)");
        set_device(G);
        G->relay_p = *p;
        G->relay_gammas.assign(gammas, gammas + (gammas ? (size_t)p->num_sets * G->dg.n : 0));
        G->relay_set = true;
        build_relay(G);
    });
}

int qd_relay_set_slots(qd_graph* G, int64_t slots) {
    return guarded([&] {
        check_graph(G);
        if (slots < 0 || slots > kRelayMaxSlots) throw Fail(-52, "relay slots must be 0 (default) .. 2^20");
        G->relay_ws.slots_cfg = slots;
    });
}

int qd_relay_info(const qd_graph* G, int32_t precision, int32_t placement, int64_t out[4]) {
    return guarded([&] {
        check_graph(G);
        if (precision != QD_F32 && precision != QD_F64) throw Fail(-4, "unknown precision");
        check_relay_placement(placement);
        if (!out) throw Fail(-52, "null output");
        const RelayLayout L(G->dg, precision == QD_F32 ? 4 : 8);
        const int kind = relay_place(L, placement);
        if (kind < 0) throw Fail(-56, "graph too large for this relay placement (LDS above 160 KiB)");
        out[0] = kind;
        out[1] = L.lds_bytes(kind == QD_RELAY_HBM);
        out[2] = kind == QD_RELAY_HBM ? L.slot_bytes : 0;
        out[3] = G->relay_ws.slots_last;
    });
}

int64_t qd_relay_kernel_names(char* buf, int64_t cap) {
    int64_t len = 0;
    const int e = guarded([&] {
        std::string s;
        append_relay_kernel_names(s);
        len = put_name(s, buf, cap);
    });
    return e ? e : len;
}

// the checks both relay entry points share, in the order qdec.h lists them;
// false: B = 0, nothing to do
static bool check_relay_call(const qd_graph* G, int32_t precision, int64_t B, const uint8_t* syn, int32_t syn_flags,
                             const uint8_t* base, const uint8_t* readout, const uint8_t* fail, int32_t placement,
                             RelayLayout* L, int* kind) {
    check_graph(G);
    if (precision != QD_F32 && precision != QD_F64) throw Fail(-4, "unknown precision");
    if (B < 0) throw Fail(-8, "negative batch");
    check_relay_placement(placement);
    if (syn_flags & QD_INPUT_PACKED) throw Fail(-57, "the relay stage takes byte rows (QD_INPUT_PACKED refused)");
    if (syn_flags & ~3) throw Fail(-57, "unknown syn_flags");
    if (fail && readout && G->dg.k > 0 && (G->dg.k > 256 || !G->dg.lz))
        throw Fail(-57, "fused failure check after relay supports <= 256 logicals");
    if (!G->relay_set) throw Fail(-54, "relay tables not set (qd_graph_set_relay)");
    if (!G->has_priors && G->has_thr)
        throw Fail(-51, "the graph's priors hold a 0 or a 1: relay needs probabilities inside (0, 1)");
    if (!G->has_priors || !G->relay_ok) throw Fail(-5, "priors not set (qd_graph_set_priors)");
    if (B == 0) return false;
    if (!syn && !(syn_flags && (base || readout))) throw Fail(-7, "no syndrome source");
    *L = RelayLayout(G->dg, precision == QD_F32 ? 4 : 8);
    *kind = relay_place(*L, placement);
    if (*kind < 0) throw Fail(-56, "graph too large for this relay placement (LDS above 160 KiB)");
    if (G->host_only) throw Fail(-16, "host-only graph (qd_graph_create_host): no device to run relay on");
    return true;
}

static void enqueue_relay(qd_graph* G, int32_t precision, const RelayArgs& args, const RelayLayout& L, int kind,
                          hipStream_t s) {
    RelayArgs a = args;
    int64_t grid;
    void* scr = nullptr;
    if (kind == QD_RELAY_HBM) {
        grid = G->relay_ws.acquire(relay_slot_rule((size_t)L.slot_bytes, (int64_t)G->num_cus * kRelaySlotsPerCu), a.B, s);
        scr = G->relay_ws.ptr;
    } else {  // no slots, but the shot counter is the handle's: the same chain
        G->relay_ws.chain.acquire(s);
        grid = std::min(relay_lds_grid(G, L), a.B);
    }
    if (!G->relay_ctr) hip_check(hipMalloc(&G->relay_ctr, 256), "hipMalloc relay counter");
    a.work_ctr = static_cast<unsigned long long*>(G->relay_ctr);
    hip_check(hipMemsetAsync(a.work_ctr, 0, sizeof(unsigned long long), s), "hipMemsetAsync relay counter");
    const int rc = launch_relay(G->dg, precision, a, G->relay_t, L, scr, grid, s);
    G->relay_ws.release(grid, s);
    if (rc != 0) throw Fail(-105, std::string("relay launch failed: ") + hipGetErrorString((hipError_t)rc));
}

int qd_relay_batch_device(qd_graph* G, int32_t precision, int64_t B, const uint8_t* syn, int32_t syn_flags,
                          const uint8_t* base, const uint8_t* readout, uint8_t* x_out, uint8_t* corr_out,
                          void* llr_out, int32_t* iters, int32_t* legs, uint8_t* status, uint8_t* fail,
                          int32_t only_failed, int32_t placement, void* stream) {
    return guarded([&] {
        RelayLayout L;
        int kind = 0;
        if (!check_relay_call(G, precision, B, syn, syn_flags, base, readout, fail, placement, &L, &kind)) return;
        set_device(G);
        const RelayArgs a{B, syn_flags, only_failed ? 1 : 0, syn, base, readout, x_out, corr_out, llr_out,
                          iters, legs, status, fail, nullptr};
        enqueue_relay(G, precision, a, L, kind, (hipStream_t)stream);
    });
}

int qd_relay_batch(qd_graph* G, int32_t precision, int64_t B, const uint8_t* syn, int32_t syn_flags,
                   const uint8_t* base, const uint8_t* readout, uint8_t* x_out, uint8_t* corr_out, void* llr_out,
                   int32_t* iters, int32_t* legs, uint8_t* status, uint8_t* fail, int32_t only_failed,
                   int32_t placement) {
    return guarded([&] {
        RelayLayout L;
        int kind = 0;
        if (!check_relay_call(G, precision, B, syn, syn_flags, base, readout, fail, placement, &L, &kind)) return;
        set_device(G);
        const DevGraph& g = G->dg;
        const size_t tsz = precision == QD_F32 ? 4 : 8;
        HostStage st;  // regions 0-2 the inputs, 3-9 every output passed
        st.add(syn, (size_t)B * g.m, "relay input");
        st.add(base, (size_t)B * g.n_data, "relay input");
        st.add(readout, (size_t)B * g.n_data, "relay input");
        st.add(x_out, (size_t)B * g.n, "relay output");
        st.add(corr_out, (size_t)B * g.n_data, "relay output");
        st.add(llr_out, (size_t)B * g.n * tsz, "relay output");
        st.add(iters, (size_t)B * 4, "relay output");
        st.add(legs, (size_t)B * 4, "relay output");
        st.add(status, (size_t)B, "relay output");
        st.add(fail, (size_t)B, "relay output");
        st.place(G->ws);
        hipStream_t s = G->stream;
        // only_failed: skipped shots keep what the caller's buffers hold, status is read
        st.copy(0, only_failed ? 10 : 3, true, s);
        const RelayArgs a{B, syn_flags, only_failed ? 1 : 0, st.dev<uint8_t>(0), st.dev<uint8_t>(1), st.dev<uint8_t>(2),
                          st.dev<uint8_t>(3), st.dev<uint8_t>(4), st.dev(5), st.dev<int32_t>(6), st.dev<int32_t>(7),
                          st.dev<uint8_t>(8), st.dev<uint8_t>(9), nullptr};
        enqueue_relay(G, precision, a, L, kind, s);
        st.finish(3, s);
    });
}

int qd_layered_set_slots(qd_graph* G, int64_t slots) {
    return guarded([&] {
        check_graph(G);
        if (slots < 0 || slots > kLayeredMaxSlots) throw Fail(-49, "layered slots must be 0 (default) .. 2^20");
        G->layered_ws.slots_cfg = slots;
    });
}

int qd_layered_info(const qd_graph* G, int32_t precision, int32_t placement, int64_t out[4]) {
    return guarded([&] {
        check_graph(G);
        if (precision != QD_F32 && precision != QD_F64) throw Fail(-4, "unknown precision");
        check_layered_placement(placement);
        if (!out) throw Fail(-49, "null output");
        const LayeredLayout L(G->dg, precision == QD_F32 ? 4 : 8);
        const int kind = layered_place(L, placement);
        if (kind < 0) throw Fail(-111, "graph too large for this layered placement (LDS above 160 KiB)");
        out[0] = kind;
        out[1] = L.lds_bytes(kind == QD_LAYERED_HBM);
        out[2] = kind == QD_LAYERED_HBM ? L.slot_bytes : 0;
        out[3] = G->layered_ws.slots_last;
    });
}

int64_t qd_layered_kernel_names(char* buf, int64_t cap) {
    int64_t len = 0;
    const int e = guarded([&] {
        std::string s;
        append_layered_kernel_names(s);
        len = put_name(s, buf, cap);
    });
    return e ? e : len;
}

// the checks both layered entry points share, in the order qdec.h lists them
// (relay's order); false: B = 0, nothing to do
static bool check_layered_call(const qd_graph* G, const qd_layered_params* prm, int32_t precision, int64_t B,
                               const uint8_t* syn, int32_t syn_flags, const uint8_t* base, const uint8_t* readout,
                               const uint8_t* fail, int32_t placement, LayeredLayout* L, int* kind) {
    static_assert(sizeof(qd_layered_params) == sizeof(LayeredParams), "qd_layered_params and LayeredParams");
    check_graph(G);
    if (precision != QD_F32 && precision != QD_F64) throw Fail(-4, "unknown precision");
    if (B < 0) throw Fail(-8, "negative batch");
    check_layered_placement(placement);
    layered_check_params(reinterpret_cast<const LayeredParams*>(prm));
    if (syn_flags & QD_INPUT_PACKED) throw Fail(-69, "layered BP takes byte rows (QD_INPUT_PACKED refused)");
    if (syn_flags & ~3) throw Fail(-69, "unknown syn_flags");
    if (fail && readout && G->dg.k > 0 && (G->dg.k > 256 || !G->dg.lz))
        throw Fail(-69, "fused failure check after layered BP supports <= 256 logicals");
    if (!G->has_priors && G->has_thr)
        throw Fail(-51, "the graph's priors hold a 0 or a 1: layered BP needs probabilities inside (0, 1)");
    if (!G->has_priors) throw Fail(-5, "priors not set (qd_graph_set_priors)");
    if (B == 0) return false;
    if (!syn && !(syn_flags && (base || readout))) throw Fail(-7, "no syndrome source");
    *L = LayeredLayout(G->dg, precision == QD_F32 ? 4 : 8);
    *kind = layered_place(*L, placement);
    if (*kind < 0) throw Fail(-111, "graph too large for this layered placement (LDS above 160 KiB)");
    if (G->host_only) throw Fail(-16, "host-only graph (qd_graph_create_host): no device to run layered BP on");
    return true;
}

static void enqueue_layered(qd_graph* G, int32_t precision, const LayeredArgs& args, const LayeredLayout& L, int kind,
                            hipStream_t s) {
    LayeredArgs a = args;
    int64_t grid;
    void* scr = nullptr;
    if (kind == QD_LAYERED_HBM) {
        grid = G->layered_ws.acquire(layered_slot_rule((size_t)L.slot_bytes, (int64_t)G->num_cus * kLayeredSlotsPerCu),
                                     a.B, s);
        scr = G->layered_ws.ptr;
    } else {  // no slots, but the shot counter is the handle's: the same chain
        G->layered_ws.chain.acquire(s);
        const int64_t cfg = G->layered_ws.slots_cfg;
        grid = std::min(cfg > 0 ? cfg : (int64_t)G->num_cus * layered_lds_per_cu(L), a.B);
    }
    if (!G->layered_ctr) hip_check(hipMalloc(&G->layered_ctr, 256), "hipMalloc layered counter");
    a.work_ctr = static_cast<unsigned long long*>(G->layered_ctr);
    hip_check(hipMemsetAsync(a.work_ctr, 0, sizeof(unsigned long long), s), "hipMemsetAsync layered counter");
    const int rc = launch_layered(G->dg, precision, a, L, scr, grid, s);
    G->layered_ws.release(grid, s);
    if (rc != 0) throw Fail(-105, std::string("layered launch failed: ") + hipGetErrorString((hipError_t)rc));
}

int qd_layered_batch_device(qd_graph* G, const qd_layered_params* prm, int32_t precision, int64_t B,
                            const uint8_t* syn, int32_t syn_flags, const uint8_t* base, const uint8_t* readout,
                            uint8_t* x_out, uint8_t* corr_out, void* llr_out, int32_t* iters, uint8_t* status,
                            uint8_t* fail, int32_t placement, void* stream) {
    return guarded([&] {
        LayeredLayout L;
        int kind = 0;
        if (!check_layered_call(G, prm, precision, B, syn, syn_flags, base, readout, fail, placement, &L, &kind))
            return;
        set_device(G);
        const LayeredArgs a{B, prm->max_iter, syn_flags, prm->ms_scaling, prm->clip, syn, base, readout, x_out,
                            corr_out, llr_out, iters, status, fail, nullptr};
        enqueue_layered(G, precision, a, L, kind, (hipStream_t)stream);
    });
}

int qd_layered_batch(qd_graph* G, const qd_layered_params* prm, int32_t precision, int64_t B, const uint8_t* syn,
                     int32_t syn_flags, const uint8_t* base, const uint8_t* readout, uint8_t* x_out,
                     uint8_t* corr_out, void* llr_out, int32_t* iters, uint8_t* status, uint8_t* fail,
                     int32_t placement) {
    return guarded([&] {
        LayeredLayout L;
        int kind = 0;
        if (!check_layered_call(G, prm, precision, B, syn, syn_flags, base, readout, fail, placement, &L, &kind))
            return;
        set_device(G);
        const DevGraph& g = G->dg;
        const size_t tsz = precision == QD_F32 ? 4 : 8;
        HostStage st;  // regions 0-2 the inputs, 3-8 every output passed
        st.add(syn, (size_t)B * g.m, "layered input");
        st.add(base, (size_t)B * g.n_data, "layered input");
        st.add(readout, (size_t)B * g.n_data, "layered input");
        st.add(x_out, (size_t)B * g.n, "layered output");
        st.add(corr_out, (size_t)B * g.n_data, "layered output");
        st.add(llr_out, (size_t)B * g.n * tsz, "layered output");
        st.add(iters, (size_t)B * 4, "layered output");
        st.add(status, (size_t)B, "layered output");
        st.add(fail, (size_t)B, "layered output");
        st.place(G->ws);
        hipStream_t s = G->stream;
        st.copy(0, 3, true, s);
        const LayeredArgs a{B, prm->max_iter, syn_flags, prm->ms_scaling, prm->clip, st.dev<uint8_t>(0),
                            st.dev<uint8_t>(1), st.dev<uint8_t>(2), st.dev<uint8_t>(3), st.dev<uint8_t>(4), st.dev(5),
                            st.dev<int32_t>(6), st.dev<uint8_t>(7), st.dev<uint8_t>(8), nullptr};
        enqueue_layered(G, precision, a, L, kind, s);
        st.finish(3, s);
    });
}

int qd_graph_set_ssf_stream(qd_graph* G, void* ssf_stream) {
    return guarded([&] {
        check_graph(G);
        set_device(G);
        if (ssf_stream && !G->ssf_ev)
            hip_check(hipEventCreateWithFlags(&G->ssf_ev, hipEventDisableTiming), "hipEventCreate");
        G->ssf_stream = (hipStream_t)ssf_stream;
    });
}

int qd_graph_set_wave_occupancy(qd_graph* G, int32_t waves_per_cu) {
    return guarded([&] {
        check_graph(G);
        if (waves_per_cu < 0 || waves_per_cu > 64) throw Fail(-62, "waves_per_cu outside [0, 64]");
        G->dg.wave_occ = waves_per_cu;
    });
}

int qd_graph_set_timing(qd_graph* G, int32_t capacity) {
    return guarded([&] {
        check_graph(G);
        set_device(G);
        if (capacity < 0) throw Fail(-90, "negative timing capacity");
        free_timing(G);
        G->tev.resize((size_t)kTimingEvents * capacity);
        for (auto& e : G->tev) hip_check(hipEventCreate(&e), "hipEventCreate");
        if (capacity > 0) {
            void* h = nullptr;
            hip_check(hipHostMalloc(&h, (size_t)capacity * kCmpLists * kCmpSegs * 8, hipHostMallocDefault),
                      "hipHostMalloc");
            G->t_listed = static_cast<uint64_t*>(h);
            G->t_cmp.assign(capacity, 0);
        }
        G->t_cap = capacity;
        G->t_count = 0;
    });
}

int qd_graph_read_timing(qd_graph* G, float* bp_ms, float* ssf_ms, int32_t max_calls, int32_t* n_calls) {
    return guarded([&] {
        check_graph(G);
        set_device(G);
        if (!n_calls) throw Fail(-91, "null n_calls");
        const int n = std::min(G->t_count, std::max(0, max_calls));
        for (int i = 0; i < n; ++i) {
            hipEvent_t* e = &G->tev[(size_t)kTimingEvents * i];
            hip_check(hipEventSynchronize(e[2]), "hipEventSynchronize");
            float t0 = 0, t1 = 0;
            hip_check(hipEventElapsedTime(&t0, e[0], e[1]), "hipEventElapsedTime");
            hip_check(hipEventElapsedTime(&t1, e[1], e[2]), "hipEventElapsedTime");
            if (bp_ms) bp_ms[i] = t0;
            if (ssf_ms) ssf_ms[i] = t1;
        }
        *n_calls = n;
        G->t_count = 0;
    });
}

int qd_graph_read_timing_detail(qd_graph* G, float* pre_ms, float* bp_ms, float* ssf_ms, int64_t* listed,
                                int32_t max_calls, int32_t* n_calls) {
    return guarded([&] {
        check_graph(G);
        set_device(G);
        if (!n_calls) throw Fail(-91, "null n_calls");
        const int n = std::min(G->t_count, std::max(0, max_calls));
        for (int i = 0; i < n; ++i) {
            hipEvent_t* e = &G->tev[(size_t)kTimingEvents * i];
            hip_check(hipEventSynchronize(e[2]), "hipEventSynchronize");
            hip_check(hipEventSynchronize(e[1]), "hipEventSynchronize");
            if (G->t_cmp[i]) hip_check(hipEventSynchronize(e[4]), "hipEventSynchronize");
            float t0 = 0, t1 = 0, t2 = 0;
            hip_check(hipEventElapsedTime(&t0, e[0], e[3]), "hipEventElapsedTime");
            hip_check(hipEventElapsedTime(&t1, e[3], e[1]), "hipEventElapsedTime");
            hip_check(hipEventElapsedTime(&t2, e[1], e[2]), "hipEventElapsedTime");
            if (pre_ms) pre_ms[i] = t0;
            if (bp_ms) bp_ms[i] = t1;
            if (ssf_ms) ssf_ms[i] = t2;
            if (listed) {
                int64_t c = -1;
                if (G->t_cmp[i]) {
                    c = 0;
                    for (int k = 0; k < kCmpLists * kCmpSegs; ++k)
                        c += (int64_t)G->t_listed[((size_t)i * kCmpLists) * kCmpSegs + k];
                }
                listed[i] = c;
            }
        }
        *n_calls = n;
        G->t_count = 0;
    });
}

int qd_graph_last_kernels(qd_graph* G, char* bp, int32_t bp_len, char* ssf, int32_t ssf_len, char* pre,
                          int32_t pre_len) {
    return guarded([&] {
        check_graph(G);
        put_name(G->last_bp, bp, bp_len);
        put_name(G->last_ssf, ssf, ssf_len);
        put_name(G->last_pre, pre, pre_len);
    });
}

int qd_graph_set_option(qd_graph* G, int32_t option, int32_t value) {
    return guarded([&] {
        check_graph(G);
        DevGraph& g = G->dg;
        auto in = [&](int lo, int hi) {
            if (value < lo || value > hi) throw Fail(-2, "option value out of range");
        };
        switch (option) {
            case QD_OPT_COMPACT: in(0, 1); g.opt_compact = value; break;
            case QD_OPT_TRIAGE_IT1: in(0, 1); g.opt_triage_it1 = value; break;
            case QD_OPT_SSF: in(QD_SSF_AUTO, QD_SSF_SCAN_NOSPLIT); g.opt_ssf = value; break;
            case QD_OPT_LDS_KERNEL: in(-1, 1); g.opt_lds_kernel = value; break;
            case QD_OPT_GROUP_KERNEL: in(-1, 1); g.opt_group_kernel = value; break;
            case QD_OPT_SSF_INC: in(0, 1); g.opt_ssf_inc = value; break;
            case QD_OPT_BLOCK_WG: in(0, 64); g.opt_block_wg = value; break;
            case QD_OPT_GROUP_MB: in(0, 1 << 22); g.opt_group_mb = value; break;
            case QD_OPT_SSF_FUSE: in(0, 1); g.opt_ssf_fuse = value; break;
            default: throw Fail(-2, "unknown option");
        }
    });
}

int qd_graph_get_option(const qd_graph* G, int32_t option, int32_t* value) {
    return guarded([&] {
        check_graph(G);
        if (!value) throw Fail(-1, "null output");
        const DevGraph& g = G->dg;
        switch (option) {
            case QD_OPT_COMPACT: *value = g.opt_compact; break;
            case QD_OPT_TRIAGE_IT1: *value = g.opt_triage_it1; break;
            case QD_OPT_SSF: *value = g.opt_ssf; break;
            case QD_OPT_LDS_KERNEL: *value = g.opt_lds_kernel; break;
            case QD_OPT_GROUP_KERNEL: *value = g.opt_group_kernel; break;
            case QD_OPT_SSF_INC: *value = g.opt_ssf_inc; break;
            case QD_OPT_BLOCK_WG: *value = g.opt_block_wg; break;
            case QD_OPT_GROUP_MB: *value = g.opt_group_mb; break;
            case QD_OPT_SSF_FUSE: *value = g.opt_ssf_fuse; break;
            default: throw Fail(-2, "unknown option");
        }
    });
}

int qd_graph_ssf_tables(const qd_graph* G, int32_t* has_lut, int64_t* lut_bytes) {
    return guarded([&] {
        check_graph(G);
        if (has_lut) *has_lut = G->dg.s_lut ? (G->dg.s_tog ? 1 : 2) : 0;
        if (lut_bytes) *lut_bytes = G->dg.s_lut ? (int64_t)G->dg.s_lut_n * 4 : 0;
    });
}

int qd_graph_ssf_tables_copy(const qd_graph* G, uint32_t* lut, uint32_t* off, uint32_t* lcw, uint32_t* tog,
                             int32_t* g_pad, int32_t* m_pad) {
    return guarded([&] {
        check_graph(G);
        if (!G->host_only) throw Fail(-16, "table copies are kept for host-only graphs (qd_graph_create_host)");
        ssf_tables_copy(G->dg, lut, off, lcw, tog, g_pad, m_pad);
    });
}

int qd_graph_queue_layout(const qd_graph* G, int64_t B, int64_t* out) {
    return guarded([&] {
        check_graph(G);
        if (B <= 0 || !out) throw Fail(-8, "invalid batch or null output");
        const QueueLayout L = queue_layout(G->dg, B);
        const int64_t v[8] = {(int64_t)L.bytes, (int64_t)L.idx, (int64_t)L.x, (int64_t)L.r, (int64_t)L.cmp_count,
                              (int64_t)L.cmp, L.cmp_cap, (int64_t)cmp_entry_bytes(G->dg)};
        std::memcpy(out, v, sizeof(v));
    });
}

// the plan of a decode described by qd_graph_plan's inputs
static DecodePlan plan_of(const qd_graph* G, const qd_params* p, int64_t B, uint32_t present) {
    check_graph(G);
    if (!p || B <= 0) throw Fail(-8, "null params or invalid batch");
    if (p->method != QD_MIN_SUM && p->method != QD_PRODUCT_SUM) throw Fail(-3, "unknown BP method");
    if (p->precision != QD_F32 && p->precision != QD_F64) throw Fail(-4, "unknown precision");
    if (p->ssf && G->dg.n_gen <= 0) throw Fail(-6, "SSF requested but the graph has no flip sets");
    // the planner reads only whether a buffer is present and how its rows
    // are aligned: stand-in addresses, never dereferenced
    const bool aligned = present & QD_PLAN_ROWS_ALIGNED;
    auto in = [&](uint32_t bit) { return reinterpret_cast<uint8_t*>((present & bit) ? (aligned ? 64 : 65) : 0); };
    auto io = [&](uint32_t bit) { return reinterpret_cast<uint8_t*>((present & bit) ? 64 : 0); };
    DecodeArgs a{};
    a.B = B;
    a.max_iter = p->max_iter > 0 ? p->max_iter : G->dg.n;
    a.ssf = p->ssf ? 1 : 0;
    a.syn_flags = p->syn_flags & 3;
    a.in_packed = (p->syn_flags & QD_INPUT_PACKED) ? 1 : 0;
    a.ms_scaling = p->ms_scaling;
    a.syn = in(QD_PLAN_SYN);
    a.base = io(QD_PLAN_BASE);
    a.readout = in(QD_PLAN_READOUT);
    a.x_out = io(QD_PLAN_X);
    a.corr_out = io(QD_PLAN_CORR);
    a.llr_out = io(QD_PLAN_LLR);
    a.fail = io(QD_PLAN_FAIL);
    const DecodePlan plan = plan_decode(G->dg, p->method, p->precision, a);
    check_plan(plan);
    return plan;
}

int qd_graph_plan(const qd_graph* G, const qd_params* p, int64_t B, uint32_t present, int32_t* out) {
    return guarded([&] {
        if (!out) throw Fail(-8, "null output");
        const DecodePlan plan = plan_of(G, p, B, present);
        const int32_t v[8] = {plan.bp, plan.ssf, plan.two_pass, plan.expand_packed, plan.fuse, plan.q_rpar,
                              plan.placement,
                              plan.need_queue | plan.need_lists << 1 | plan.need_unpack << 2 | plan.need_scratch << 3};
        std::memcpy(out, v, sizeof(v));
    });
}

int qd_graph_plan_names(const qd_graph* G, const qd_params* p, int64_t B, uint32_t present, char* bp, int32_t bp_len,
                        char* ssf, int32_t ssf_len, char* pre, int32_t pre_len) {
    return guarded([&] {
        const DecodePlan plan = plan_of(G, p, B, present);
        put_name(noted_name(plan.bp_k), bp, bp_len);
        put_name(noted_name(plan.fin_k), ssf, ssf_len);
        put_name(noted_name(plan.pre_k), pre, pre_len);
    });
}

int qd_graph_plan_entries(const qd_graph* G, const qd_params* p, int64_t B, uint32_t present, char* bp, int32_t bp_len,
                          char* ssf, int32_t ssf_len, char* pre, int32_t pre_len) {
    return guarded([&] {
        const DecodePlan plan = plan_of(G, p, B, present);
        auto entry_name = [](const KernelEntry* e) { return e ? e->name.c_str() : ""; };
        put_name(entry_name(plan.bp_k), bp, bp_len);
        put_name(entry_name(plan.fin_k), ssf, ssf_len);
        put_name(entry_name(plan.pre_k), pre, pre_len);
    });
}

int64_t qd_kernel_table_names(char* buf, int64_t cap) {
    int64_t len = 0;
    const int e = guarded([&] {
        std::string s;
        append_wave_kernel_names(s);
        append_block_kernel_names(s);
        len = put_name(s, buf, cap);
    });
    return e ? e : len;
}

int qd_graph_it1_tables_copy(const qd_graph* G, int32_t precision, uint16_t* lut, uint64_t* vchk, int32_t* n_pad) {
    return guarded([&] {
        check_graph(G);
        if (!G->host_only) throw Fail(-16, "table copies are kept for host-only graphs (qd_graph_create_host)");
        if (precision != QD_F64 && precision != QD_F32) throw Fail(-4, "invalid precision");
        const DevGraph& g = G->dg;
        if (n_pad) *n_pad = g.n_pad;
        if (!g.it1_lut[precision] || !g.it1_vchk) throw Fail(-37, "no iteration-1 tables for this precision");
        if (lut) std::memcpy(lut, g.it1_lut[precision], (size_t)g.n_pad * 2);
        if (vchk) std::memcpy(vchk, g.it1_vchk, (size_t)g.n_pad * 8);
    });
}

int qd_graph_ms_state0_copy(const qd_graph* G, int32_t precision, void* state, uint16_t* sslot, int32_t* m_pad) {
    return guarded([&] {
        check_graph(G);
        if (!G->host_only) throw Fail(-16, "table copies are kept for host-only graphs (qd_graph_create_host)");
        if (precision != QD_F64 && precision != QD_F32) throw Fail(-4, "invalid precision");
        const DevGraph& g = G->dg;
        if (m_pad) *m_pad = g.m_pad;
        if (!g.ms_state0[precision] || !g.ms_sslot[precision])
            throw Fail(-39, "no first check state (not a wave-kernel graph, or priors not set)");
        if (state) std::memcpy(state, g.ms_state0[precision], 2 * (size_t)g.m_pad * (precision == QD_F64 ? 8 : 4));
        if (sslot) std::memcpy(sslot, g.ms_sslot[precision], (size_t)g.m_pad * 2);
    });
}

int qd_graph_lds64_slots_copy(const qd_graph* G, uint16_t* etab, uint16_t* check_of_slot) {
    return guarded([&] {
        check_graph(G);
        if (!G->host_only) throw Fail(-16, "table copies are kept for host-only graphs (qd_graph_create_host)");
        const DevGraph& g = G->dg;
        if (!g.m64_etab || !g.m64_check) throw Fail(-38, "no f64 LDS-kernel slot tables for this graph");
        if (etab) std::memcpy(etab, g.m64_etab, (size_t)kMlDC * g.n * 2);
        if (check_of_slot) std::memcpy(check_of_slot, g.m64_check, (size_t)g.m * 2);
    });
}

int qd_count_flags_device(const uint8_t* flags, int64_t B, uint8_t mask, int64_t* out, void* stream) {
    return guarded([&] {
        if (B < 0 || (B > 0 && (!flags || !out))) throw Fail(-70, "invalid count arguments");
        const int rc = launch_count_flags(flags, B, mask, out, (hipStream_t)stream);
        if (rc != 0) throw Fail(-103, std::string("count launch failed: ") + hipGetErrorString((hipError_t)rc));
    });
}

}  // extern "C"
