// qdec_internal.h -- launch arguments and launchers shared by the host ABI
// (qdec_abi.cpp) and the kernel and launch units (qdec_launch_wave.hip, qdec_sample.hip, ...); the graph
// description they work on is qdec_graph.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <initializer_list>
#include <string>
#include <vector>

#include "qdec_circuit.h"
#include "qdec_graph.h"
#include "qdec_layered.h"
#include "qdec_relay.h"
#include "qdec_window.h"

namespace qdec {

struct DecodeArgs {
    int64_t B;
    int max_iter, ssf, ssf_max_steps, syn_flags;
    double ms_scaling;
    const uint8_t* syn;
    const uint8_t* base;
    const uint8_t* readout;
    uint8_t* x_out;
    uint8_t* corr_out;
    void* llr_out;
    int32_t* iters;
    uint8_t* status;
    int32_t* ssf_steps;
    uint8_t* fail;
    // SSF work queue (device scratch owned by the graph handle)
    int32_t* q_count;  // [1]
    int64_t* q_idx;    // [B]   shot of queue slot
    uint8_t* q_x;      // [B][n] BP hard decision
    uint8_t* q_r;      // [B][m] residual syndrome
    // packed queue (wave kernels, q_packed = 1): entry s = q_w[s*(1+XW+RW) ..]:
    // shot index, hard decision by column (XW = n_pad/64 words), residual by
    // check (RW = m_pad/64 words); replaces q_idx/q_x/q_r
    int q_packed;
    uint64_t* q_w;
    // workgroup BP kernel with HBM message slices: shot counter handing out
    // shots dynamically (a straggler does not hold up a fixed stride of shots);
    // nullptr -> static stride.  Set by the launcher.
    unsigned long long* work_ctr;
    // min-sum wave kernel: counter of the dynamically scheduled shot chunks
    // (ShotSeq, qdec_shot_seq.h); zeroed by the launcher; nullptr -> static stride
    unsigned long long* wave_ctr;
    // SSF on a second stream (qd_graph_set_ssf_stream, wave kernels only): the
    // SSF kernel waits for ssf_ev (recorded after the BP kernel) on ssf_stream,
    // so a later BP launch on the BP stream can overlap it; nullptr -> same stream
    hipStream_t ssf_stream;
    hipEvent_t ssf_ev;
    // SSF wave kernel: 1 disables the two-lanes-per-generator scoring of short
    // listing steps (QDEC_SSF_NOSPLIT=1; parity tests run both ways)
    int ssf_nosplit;
    // optional timing (host side only): events recorded on the launch stream
    // before the BP kernel, after it, after the SSF kernel, and after the BP
    // stage's pre-pass (record_ev)
    hipEvent_t* ev;    // [4] or nullptr
    // compact shot list of lean min-sum wave launches (ms_triage_kernel ->
    // bp_ms_cmp_kernel), in kCmpLists x kCmpSegs segments: triage tile t appends
    // to segment t % kCmpSegs (light shots) and kCmpSegs + t % kCmpSegs (heavy
    // ones, decoded first), whose entries [cmp_cap][CmpEntry::EW] u64 start at
    // cmp + s * cmp_cap * EW, counted at cmp_count[s * 16] (one 128-B line per
    // counter; zeroed by the launcher).  nullptr -> no compact path
    uint64_t* cmp;
    unsigned long long* cmp_count;
    // the other counter set of the handle (double-buffered): the triage zeroes
    // it for the handle's next two-pass decode, so no decode needs a memset
    // launch (nullptr: the launcher memsets cmp_count itself)
    unsigned long long* cmp_count_next;
    int64_t cmp_cap;
    int cmp_zero_ok;  // every prior of the launch's precision > 0: zero syndromes finish in the triage
    // the triage runs iteration 1 itself (g.it1_lut of the launch's precision;
    // set by the launcher when the schedule's alpha_1 is 0.5): shots whose
    // iteration-1 decision meets the syndrome finish there
    const uint16_t* it1_lut;
    // packed SSF queue entries carry the readout's logical parities (bit r of
    // the dw area = parity of Lz[r] . readout) instead of the readout words
    int q_rpar;
    // QD_INPUT_PACKED: syn / base / readout are bit-packed rows of u64 words
    // (syn [B][ceil(m/64)], base / readout [B][ceil(n_data/64)]; bit j of word
    // w = element 64 w + j).  The two-pass path's triage reads them directly;
    // every other path first expands them into unpack_buf (library-owned,
    // B * (m + 2 n_data) bytes) with unpack_rows_kernel.
    int in_packed;
    uint8_t* unpack_buf;
};

// Arguments of the GPU OSD stage (qdec_osd.hip).  Shots whose status has bit 0
// (BP converged) set are skipped; outputs of other shots are left untouched.
struct OsdArgs {
    int64_t B;
    int method, order, syn_flags, llr_f32;
    const uint8_t* syn;      // [B][m] (nullable with syn_flags)
    const void* llr;         // [B][n] float or double: BP log-probability ratios
    const uint8_t* status;   // [B] nullable: every shot is post-processed
    const uint8_t* base;     // [B][n_data] nullable
    const uint8_t* readout;  // [B][n_data] nullable
    uint8_t* osd0_out;       // [B][n] nullable
    uint8_t* osdw_out;       // [B][n] nullable
    uint8_t* corr_out;       // [B][n_data] nullable: base ^ fold(osdw)
    uint8_t* fail;           // [B] nullable: any(Lz (readout ^ corr))
};
// Which OSD kernel holds a graph, by m, n (and k) alone: rs = row slots and w =
// row words of the register kernel osd_wave_kernel<rs, w>, or rs = 0 and w = the
// row words of the workgroup kernel; lds = the launch's dynamic LDS bytes.
// False (all zero): no device kernel.  No HIP call; launch_osd launches what it
// answers.
struct OsdChoice {
    int rs, w, lds;
};
bool osd_choose(const DevGraph& g, OsdChoice* c);
bool osd_kernel_supports(const DevGraph& g);
int launch_osd(const DevGraph& g, const OsdArgs& a, int num_cus, hipStream_t stream);

// osd_hbm_kernel (qdec_osd_hbm.hip): the same stage with the rows in a slot of
// device memory.  Byte offsets of a slot (s_*: rows [m][W] u64, sort keys u64
// and column indices u32 [ns], pos u32 [n], piv u32 [m], isp and out u8 [n];
// every region 16-B aligned, the slot a multiple of 256 B) and of the
// workgroup's LDS (l_*; the sort's chunk overlays the rest).
struct OsdHbmLayout {
    int64_t ns, W, RW;
    int64_t s_rows, s_key, s_idx, s_pos, s_piv, s_isp, s_out, slot_bytes;
    int64_t l_ctl, l_npv, l_x0, l_tcl, l_row, l_hit, l_skey, l_sidx, lds_bytes;
    OsdHbmLayout() = default;
    OsdHbmLayout(int64_t n, int64_t m);
};
// False: the kernel does not hold the graph (its LDS part above 160 KiB, or
// k > 256).  No HIP call.
bool osd_hbm_choose(const DevGraph& g, OsdHbmLayout* L);
// `scratch` holds `slots` slots of L.slot_bytes; the grid is min(slots, B)
int launch_osd_hbm(const DevGraph& g, const OsdArgs& a, void* scratch, int64_t slots, hipStream_t stream);
// Which kernel runs a graph under a placement (QD_OSD_ONCHIP / _HBM / _AUTO of
// qdec.h, checked by the caller): on chip where osd_choose holds the graph,
// unless the HBM kernel is forced; otherwise the HBM kernel where
// osd_hbm_choose holds it, unless on chip is forced.  The kernel's value is
// what qd_osd_kernel_info_placed reports in out[0]; c is set for the two
// on-chip kernels, L for the HBM kernel.  No HIP call.
enum OsdKernel { kOsdNone = -1, kOsdRegister = 0, kOsdWorkgroup = 1, kOsdHbm = 2 };
struct OsdPlaced {
    OsdKernel kernel;
    OsdChoice c;
    OsdHbmLayout L;
};
void osd_place(const DevGraph& g, int placement, OsdPlaced* p);
// slots per CU of the HBM kernel by default (DESIGN §3.6c has the sweep)
constexpr int kOsdHbmSlotsPerCu = 8;

// ev[3] marks the end of a pre-pass inside the BP timing (the shot triage):
// recorded with ev[0] and again after the pre-pass when one runs
inline void record_ev(const DecodeArgs& a, int i, hipStream_t s) {
    if (!a.ev) return;
    (void)hipEventRecord(a.ev[i], s);
    if (i == 0) (void)hipEventRecord(a.ev[3], s);
}

// One built instantiation of a kernel family: what a launch needs to know about
// it.  The families' tables (wave_tables in qdec_launch_wave.hip, block_tables in
// qdec_launch_block.hip) list every instantiation the library builds; plan_decode
// picks the entries of a decode, the launchers launch what the plan holds.
struct KernelEntry {
    const void* fn = nullptr;  // host address of the kernel (hipLaunchKernel, hipFuncSetAttribute)
    std::string name;          // rocprofv3's spelling: base<arg, arg, ...>
    int t[8] = {};             // the template arguments in the kernel's order (types: QD_F64 / QD_F32)
    int nt = 0;
    int block = 0;             // threads per workgroup
    bool noted = true;         // qd_graph_last_kernels reports the stage (false: it stays "")
    // dynamic LDS of a launch, for the families whose size depends on template
    // arguments (before the launcher's padding); nullptr: the launcher's own figure
    size_t (*lds)(const DevGraph&, const DecodeArgs&) = nullptr;
};
using KernelTable = std::vector<KernelEntry>;
// the entry with exactly these template arguments, nullptr when it is not built
inline const KernelEntry* find_kernel(const KernelTable& tab, std::initializer_list<int> targs) {
    for (const KernelEntry& e : tab)
        if ((size_t)e.nt == targs.size() && std::equal(targs.begin(), targs.end(), e.t)) return &e;
    return nullptr;
}

// Names of the BP and SSF kernels the calling host thread's last launch_decode
// enqueued, spelled as rocprofv3 prints them (template arguments included; ""
// when none / not recorded): the names of the plan's entries, noted as each
// stage is enqueued.  Host only; read by qd_graph_last_kernels.
struct LaunchNames {
    const char* bp = "";
    const char* ssf = "";
    const char* pre = "";  // a pass before the BP kernel (ms_triage_kernel), inside the BP timing
};
LaunchNames& last_launch_names();
inline const char* noted_name(const KernelEntry* e) { return e && e->noted ? e->name.c_str() : ""; }
// The name of every entry of the families' tables, one per line, in table order
// (wave_tables, qdec_launch_wave.hip; block_tables, qdec_launch_block.hip).  No
// HIP call.  Read by qd_kernel_table_names.
void append_wave_kernel_names(std::string& out);
void append_block_kernel_names(std::string& out);

// relay_block_kernel (qdec_relay.hip; arguments and layouts: qdec_relay.h).  Its
// entries have a table of their own (relay_table: one per precision), outside
// the decode plan's tables.  launch_relay enqueues `grid` workgroups; with the
// messages in HBM `scratch` holds `grid` slots of L.slot_bytes, else it is null.
void add_relay_kernels(KernelTable& t);
const KernelTable& relay_table();
void append_relay_kernel_names(std::string& out);
int launch_relay(const DevGraph& g, int precision, const RelayArgs& a, const RelayTables& t, const RelayLayout& L,
                 void* scratch, int64_t grid, hipStream_t stream);

// layered_wave_kernel (qdec_layered.hip; arguments and layouts: qdec_layered.h).
// A table of its own as well (layered_table: precision x placement).
// launch_layered enqueues `grid` one-wave workgroups; with the beliefs in HBM
// `scratch` holds `grid` slots of L.slot_bytes, else it is null.
void add_layered_kernels(KernelTable& t);
const KernelTable& layered_table();
void append_layered_kernel_names(std::string& out);
int launch_layered(const DevGraph& g, int precision, const LayeredArgs& a, const LayeredLayout& L, void* scratch,
                   int64_t grid, hipStream_t stream);

// window_advance_kernel (qdec_window.hip; tables and arguments: qdec_window.h):
// `grid` workgroups take the B shots grid-strided.  Returns hipError_t as int.
int launch_window(const WindowDev& w, const WindowArgs& a, int64_t grid, hipStream_t stream);

// ---------------------------------------------------------------- launch plan
// Everything a decode decides before its first launch, decided once
// (plan_decode) and read by the buffer attachment (qdec_abi.cpp) and by the
// launchers.  DESIGN §3 has the decision table.
enum BpPath {
    kBpWave = 0,     // bp_wave_kernel: wave graph, message arrays (product-sum)
    kBpMsWave = 1,   // bp_ms_wave_kernel: wave graph, min-sum, one pass
    kBpTwoPass = 2,  // ms_triage_kernel + bp_ms_cmp_kernel: wave graph, lean min-sum
    kBpGroup = 3,    // bp_group_kernel: slot groups, messages in HBM
    kBpLds = 4,      // bp_ms_lds_kernel (f32) / bp_ms_lds64_kernel (f64)
    kBpBlock = 5,    // bp_block_kernel, state placed by `placement`
};
enum SsfPath {
    kFinNone = 0,        // the BP kernel finalizes every shot itself
    kFinFused = 1,       // SSF inside bp_ms_cmp_kernel (FUSE = 1 / 2)
    kFinLut = 2,         // ssf_lut_kernel
    kFinScan = 3,        // ssf_wave_kernel
    kFinScanGather = 4,  // ssf_wave_kernel without the inverse table
    kFinScanNoSplit = 5, // ssf_wave_kernel, one lane per generator
    kFinIncBlock = 6,    // ssf_inc_block_kernel
    kFinBlockLds = 7,    // ssf_block_kernel, shot state in LDS
    kFinBlockHbm = 8,    // ssf_block_kernel, shot state in the scratch tail
};
struct DecodePlan {
    int method, precision;
    int bp;              // BpPath
    int ssf;             // SsfPath
    int placement;       // kBpBlock's block_placement (also decides kFinBlockHbm); 3 on wave graphs
    bool two_pass;       // bp == kBpTwoPass
    bool lean;           // wave min-sum: the LEAN instantiation of the one-pass kernel
    bool defer;          // a queue consumer follows the BP kernel (ssf != kFinNone and != kFinFused)
    int fuse;            // 0, or the generator words of the fused SSF (1: <= 64, 2: <= 128)
    int q_packed, q_rpar;  // DecodeArgs' queue flags
    bool ssf_lean;       // ssf_lut_kernel's LEAN instantiation
    bool expand_packed;  // packed inputs go through unpack_rows_kernel first
    int wave_cap;        // wave min-sum: waves per CU the launch is capped to (0: the kernel's occupancy)
    // the instantiation of every stage (entries of the families' tables):
    // pre-pass (two_pass), BP, SSF / finalize (nullptr: no such stage)
    const KernelEntry* pre_k;
    const KernelEntry* bp_k;
    const KernelEntry* fin_k;
    // a stage's instantiation is not built: the family's name (nullptr: the plan is complete)
    const char* missing;
    // library-owned buffers the launch needs
    bool need_queue, need_lists, need_unpack, need_scratch;
};
// Pure: reads the graph's fields and options and the caller's part of `a`
// (which buffers are present, syn_flags, in_packed, ssf, max_iter, ms_scaling,
// the alignment of syn / readout); no HIP call, so host-only graphs plan too.
DecodePlan plan_decode(const DevGraph& g, int method, int precision, const DecodeArgs& a);
// the workgroup half (qdec_launch_block.hip): graphs no wave shape holds
void plan_decode_block(const DevGraph& g, const DecodeArgs& a, DecodePlan& p);
// SSF + finalize of queued shots by a workgroup kernel with its state in LDS
int ssf_fin_path(const DevGraph& g, const DecodeArgs& a);
// the workgroup SSF / finalize kernel of a path (kFinIncBlock, kFinBlockLds, kFinBlockHbm)
const KernelEntry* ssf_block_entry(int path);
bool wave_kernel_supports(const DevGraph& g);
// byte rows of expanded packed inputs: the regions of unpack_buf (16-B aligned,
// so the byte-row triage can load them)
inline size_t unpack_region(int64_t B, int cols) { return ((size_t)B * cols + 15) / 16 * 16; }

// Launchers (qdec_launch_wave.hip, qdec_launch_block.hip, qdec_sample.hip).  Return hipError_t as int.
// *triaged: the two-pass path's triage was enqueued (it zeroed the other
// counter set of the handle)
int launch_decode(const DevGraph& g, const DecodePlan& p, const DecodeArgs& a, int num_cus, hipStream_t stream,
                  void* scratch, size_t scratch_bytes, bool* triaged);
int launch_decode_block(const DevGraph& g, const DecodePlan& p, const DecodeArgs& a, int num_cus,
                        hipStream_t stream, void* scratch, size_t scratch_bytes);
int launch_ssf_block(const DevGraph& g, const DecodePlan& p, const DecodeArgs& a, int num_cus, hipStream_t stream);
size_t block_scratch_bytes(const DevGraph& g, const DecodePlan& p, int num_cus, const DecodeArgs& a);
size_t block_scratch_floor(const DevGraph& g, const DecodePlan& p, int num_cus, const DecodeArgs& a);
int launch_sample_storage(const DevGraph& g, int rounds, uint32_t thr_data, uint32_t thr_meas,
                          uint32_t seed, uint32_t stream_id, int64_t shot0, int64_t B,
                          uint8_t* syn, uint8_t* readout, int num_cus, hipStream_t stream, bool packed = false);
// B shots of the graph's own faults (sample_faults_kernel): det = H e, faults = e
// (nullable), obs = F e (nullable; F = the graph's logicals); byte rows, or u64
// words when packed.  thr / crow: HostGraph::smp_thr / smp_crow (qdec_tables.h)
int launch_sample_faults(const DevGraph& g, const uint32_t* thr, const int32_t* crow, uint32_t seed,
                         uint32_t stream_id, int64_t shot0, int64_t B, bool packed, void* det, void* faults,
                         uint8_t* obs, int num_cus, hipStream_t stream);
int launch_count_flags(const uint8_t* flags, int64_t B, uint8_t mask, int64_t* out, hipStream_t stream);
// Where a launch of the frame kernels (qdec_frame.hip) keeps the frame.  FP_LDS:
// lds = the program's HostCircuit::lds_bytes; the grid is min(64-shot words,
// 32 num_cus).  FP_HBM: `scratch` holds `slots` slots of slot_bytes = 16 Q + 8 M
// each, one per resident workgroup; the grid is min(64-shot words, slots).
struct FramePlace {
    int32_t placement = FP_LDS;
    size_t lds = 0;
    int num_cus = 0;
    void* scratch = nullptr;
    size_t slot_bytes = 0;
    int64_t slots = 0;
};
// B shots of a compiled circuit (frame_sample_kernel): group g's rows to outs[g]
// (nullable), byte rows or u64 words when packed
int launch_frame_sample(const DevCircuit& c, const FramePlace& at, uint32_t seed, uint32_t stream_id, int64_t shot0,
                        int64_t B, bool packed, void* const outs[kFrameGroups], hipStream_t stream);
// Faults f0 .. f0 + F of one kind (0 noise, 1 gauge) propagated through the
// circuit (frame_fault_kernel): the same outputs, a fault where the sampler has a shot
int launch_frame_faults(const DevCircuit& c, const FramePlace& at, int kind, int32_t f0, int32_t F, bool packed,
                        void* const outs[kFrameGroups], hipStream_t stream);
// workgroups (slots) per CU of the frame kernels in HBM by default (DESIGN §3.4c has the measurement)
constexpr int kFrameHbmSlotsPerCu = 8;

// ---------------------------------------------------------------- HGP kernel
// Hypergraph-product codes get their own f64 min-sum BP kernel, generated and
// compiled per code with hipRTC (qdec_hgp.cpp, qdec_hgp_kernel.hip).
struct HgpPlan;
struct HgpBpArgs {  // the kernel's HgArgs, field for field
    const uint8_t* syn;           // [B][m]
    const double* prior;          // [n] min-sum prior per column
    uint8_t* x_out;               // [B][n] or null
    int32_t* iters;               // [B] or null
    uint8_t* status;              // [B] or null (bit 0: BP converged)
    unsigned long long* counter;  // shot counter (zeroed by hgp_launch_bp)
    int64_t B;
    int32_t max_iter;
    double ms_scaling;
};
// nullptr unless H = [I_a0 (x) B | A (x) I_b0] within the kernel's limits
// slots: shot slots per workgroup (0: the plan's choice)
HgpPlan* hgp_plan_create(int m, int n, const std::vector<int32_t>& rp, const std::vector<int32_t>& ci, int slots = 0);
void hgp_plan_destroy(HgpPlan* P);
const std::string& hgp_plan_source(const HgpPlan* P);
void hgp_plan_replace_source(HgpPlan* P, const std::string& src);  // development
int hgp_plan_compile(HgpPlan* P, const char* arch, std::string* log);  // hipRTC (no device needed)
int hgp_plan_load(HgpPlan* P, int num_cus, const char* arch);           // compile + load on the current device
std::string hgp_target_arch(int device);  // hipRTC target of `device` (< 0: the build's QDEC_ARCH)
int hgp_launch_bp(HgpPlan* P, const HgpBpArgs& a, hipStream_t stream);
void hgp_plan_info(const HgpPlan* P, int* out8);  // a0 a1 b0 b1 S WL WR per_cu

}  // namespace qdec
