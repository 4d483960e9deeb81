// qdec_graph.h -- the graph description the host table builders (qdec_tables.cpp)
// fill and the kernels (the kernel units, qdec_sample.hip) read.  No HIP type: the
// builders compile without the HIP headers; qdec_internal.h adds the launch side.
#pragma once
#include <stdint.h>

namespace qdec {

constexpr int kWave = 64;        // CDNA wavefront
constexpr int kDR = 8;           // max check degree of the wave kernels
constexpr int kDC = 4;           // max variable degree of the wave kernels
constexpr int kMlDRS = 8;        // LDS-resident min-sum kernel: row stride (elements), max check degree
constexpr int kMlDC = 4;         // LDS-resident min-sum kernel: max variable degree
constexpr int kGenW = 8;         // max flip-set generator weight (255 subsets)
constexpr int kGenLC = 32;       // max local checks per generator (u32 masks)
constexpr int kSsfScale = 840;   // lcm(1..8): gain/|F| compared as gain*(840/|F|)
constexpr int kLutLC = 16;       // table-driven SSF: max local checks per generator (16-bit local syndromes)
constexpr int kLutLCW = kLutLC / 4;  // words of u8 local-check ids per generator
constexpr int kEdgePad = 16;     // index / prior arrays padded past E (>= the largest row / column width)
constexpr int kCmpSegs = 64;     // segments (and counters) of each compact shot list
constexpr int kCmpLists = 2;     // the light list (segments 0..63) and the heavy list (64..127)
// entries a compact-list segment must hold for a batch of B shots (64-shot tiles)
inline int64_t cmp_seg_cap(int64_t B) { return ((B + 63) / 64 + kCmpSegs - 1) / kCmpSegs * 64; }

// Every workgroup kernel starts its dynamic LDS with a control area of kCtrl
// bytes (no static __shared__, so the dynamic base stays 16-byte aligned).
// Byte offsets of its fields; a kernel's own arrays start at kCtrl.
constexpr int kCtrlRed64 = 0;   // long long [4]: per-wave partials of a 64-bit block reduction
constexpr int kCtrlRed32 = 32;  // int [4]: the same for a 32-bit one
constexpr int kCtrlSlot = 48;   // int: a queue slot; ssf_inc_block_kernel's int ctl[3], which has no shot counter
constexpr int kCtrlNext = 56;   // long long: the shot counter's answer
constexpr int kCtrl = 64;

// Wave-kernel shapes (check rounds RC, variable rounds RV, check-node compute
// width D <= kDR): a graph is padded to the first shape that holds it (RC*64 >= m,
// RV*64 >= n, D >= max check degree), and the kernel is instantiated for exactly
// that shape so no per-round guard is needed.  (2, 4, 7) is the n = 225 HGP code.
#define QDEC_WAVE_SHAPES(X) X(1, 2, 8) X(2, 3, 6) X(2, 3, 8) X(2, 4, 7) X(2, 4, 8) X(2, 6, 8) X(4, 9, 8)
inline bool pick_wave_shape(int m, int n, int max_rdeg, int* rc, int* rv, int* drc) {
    const int need_c = (m + 63) / 64, need_v = (n + 63) / 64;
#define QDEC_PICK(R, V, D) \
    if (need_c <= R && need_v <= V && max_rdeg <= D) { *rc = R; *rv = V; *drc = D; return true; }
    QDEC_WAVE_SHAPES(QDEC_PICK)
#undef QDEC_PICK
    return false;
}

// LDS stride, in elements, of a per-lane block of D values of type T, chosen so a
// wave reading its 64 blocks with 16-byte ds_read_b128 is bank-conflict free:
// dword stride a multiple of 4 with an odd quotient (16 lanes cover 64 banks).
template <typename T, int D>
constexpr int lds_stride() {
    int dw = (int)((D * sizeof(T) + 3) / 4);
    dw = (dw + 3) / 4 * 4;
    if ((dw / 4) % 2 == 0) dw += 4;
    return dw * 4 / (int)sizeof(T);
}

// Slot tables depend on the element stride, i.e. on the precision.
struct SlotTables {
    const uint16_t* r_cslot;  // [kDR][m_pad]  c2v element written by check i, edge k
    const uint16_t* c_rslot;  // [kDC][n_pad]  v2c element written by variable j, edge k
};

struct DevGraph {
    int m, n, m_pad, n_pad;       // pads: multiples of 64
    int E;                        // edges (nnz of H)
    int wave;                     // 1: a wave-kernel shape holds this graph
    int n_data, fold_blocks;
    int max_rdeg, max_cdeg;
    int shape_drc;                // check-node compute width of the chosen wave shape
    const uint8_t* r_deg;         // [m_pad]
    const uint16_t* r_col;        // [kDR][m_pad]  column of edge k of check i (pad -> n_pad)
    const uint8_t* c_deg;         // [n_pad]
    SlotTables slots[2];          // [QD_F64], [QD_F32]
    const void* prior[2][2];      // [method][precision] initial message per column, [n_pad]
    // the same by CSR edge (the prior of edge e's column), [E + kEdgePad]
    // (slot-group kernel: one load per edge, no column-index chain)
    const void* eprior[2][2];
    // CSR / CSC copies (sampler; workgroup kernels)
    const int32_t* row_ptr;
    const int32_t* col_idx;
    const int32_t* col_ptr;       // [n+1]
    const int32_t* col_edge;      // [E] CSR edge ids of column j, ascending row
    const int32_t* edge_csc;      // [E] CSC position (col_ptr[col] + rank in column) of CSR edge e
    // col_idx, col_edge and edge_csc carry kEdgePad zero entries past E, so a
    // kernel may load a whole row's (column's) worth of indices unguarded
    // min-sum wave kernel with compressed check state (qdec_bp_ms.h).  Variables
    // sit in lane slots sorted by degree (ms_vslot); slot edge k scatters its v2c
    // message to element (etab & 0xffff) and gathers check state (etab >> 16);
    // pads -> a dummy element / the zero state m_pad.
    // Row positions inside a check's v2c row and the state slot of each check
    // are chosen on the host (per precision) to cut the LDS bank conflicts of
    // the scatter and of the state gather (ms_layout in qdec_tables.cpp).
    const uint32_t* ms_etab[2];   // [kDC][n_pad], per precision (element strides differ)
    const uint16_t* ms_sslot[2];  // [m_pad] state slot written by check lane i, per precision
    const uint64_t* ms_smask;     // [n_pad/64][m_pad] slots of check i's columns inside 64-slot word w
    const uint16_t* ms_vslot;     // [n_pad] column held by lane slot s (pads: n_pad + s % 64)
    const void* ms_prior[2];      // [precision][n_pad] min-sum priors in slot order
    // the check state (m1, m2) the first check pass of the compact kernel would
    // write for check lane i (ms_sslot's order, pads included) on rows holding
    // the priors under syndrome bit 0, in the kernel's precision and by its sign
    // rule (ms_state0_table in qdec_tables.cpp); the kernel starts each listed
    // shot from it instead of running that pass
    const void* ms_state0[2];     // [precision][m_pad][2]
    int ms_d3r;                   // leading 64-slot rounds whose variables all have degree <= 3
    int ms_allpos;                // bit p: every prior LLR of precision p is > 0
    // iteration 1 of min-sum inside the triage (ms_triage_kernel, qdec_ms_triage.hip):
    // the checks of column j's edges in edge order (4 x u16, pad -> m), the
    // columns of check i's row (8 x u16 over two words, pad -> n), and per
    // precision each column's hard decision after iteration 1 as a 16-bit table
    // over its checks' syndrome bits (nullptr unless every prior of that
    // precision is > 0; it1_tables in qdec_tables.cpp)
    const uint64_t* it1_vchk;     // [n_pad]
    const uint64_t* it1_cvar;     // [m_pad][2]
    const uint16_t* it1_lut[2];   // [precision][n_pad]
    int wave_occ;                 // qd_graph_set_wave_occupancy (0: default)
    // LDS-resident min-sum workgroup kernel (qdec_ms_lds.hip, bp_ms_lds_kernel):
    // [kMlDC][n] LDS element of edge k of column j (row * kMlDRS + CSR position),
    // pad 0xffff; nullptr when the graph's degrees exceed kMlDRS / kMlDC
    const uint16_t* ml_etab;
    // bp_ms_lds64_kernel: check states live at host-placed slots (m64_layout,
    // qdec_tables.cpp): [kMlDC][n] state slot of edge k of column j (pad 0xffff),
    // and [m] the check held by each slot
    const uint16_t* m64_etab;
    const uint16_t* m64_check;
    int m64_d3r;                  // leading variable rounds (1024 columns each) of degree <= 3
    // flip sets (SSF)
    int n_gen, g_pad, g_wmax;
    const uint8_t* g_w;           // [g_pad]
    const uint16_t* g_q;          // [kGenW][g_pad]   qubit (column) k of generator g
    const uint8_t* g_nlc;         // [g_pad]
    const uint16_t* g_lc;         // [kGenLC][g_pad]  local check c of generator g
    const uint32_t* g_lc8;        // [kGenLC/4][g_pad] the same ids packed 4 per word (pad -> m_pad)
    int g_nlcmax;
    // inverse of the local-check lists, for the wave SSF kernel's incremental
    // local syndromes: [m_pad][g_invd] u16 entries g | (bit << 8) (generator g has
    // check i as local check `bit`), pad 0xffff; g_invd a power of two (log2:
    // g_invl).  nullptr when unavailable (the kernel re-gathers every step).
    const uint16_t* g_inv;
    int g_invd, g_invl;
    const uint32_t* g_qmask;      // [kGenW][g_pad]   local-check mask of qubit k
    // every generator's local checks inverted, CSR by check: entries of check i
    // are g_ient[g_iptr[i] .. g_iptr[i+1]), each g | (local bit << 16)
    // (ssf_inc_block_kernel; nullptr when n_gen >= 65536)
    const int32_t* g_iptr;
    const uint32_t* g_ient;
    // table-driven SSF (ssf_lut_kernel, qdec_bp.hip; built by ssf_lut_tables in
    // qdec_tables.cpp, nullptr when the graph does not qualify).  A generator's
    // local checks are put in a canonical order (by the set of its qubits that
    // touch them), so generators with the same local structure share one table
    // over their <= 16-bit local syndrome sl: s_lut[s_off[g] + sl] = rank << 24 |
    // M_t << 8 | t, t the spec's best subset (lowest bitmask among the best
    // gain/|t|), M_t the local checks it toggles, rank the position of its score
    // among all positive scores (0: no positive gain).  s_lcw: the canonical local
    // checks as u8 ids, 4 per word ([kLutLCW][g_pad], pad 0xff); s_tog: per check
    // c and lane l the local-syndrome bits that toggle when c flips, generator l
    // in the low half-word, generator 64 + l in the high one ([m_pad + 1][64],
    // row m_pad all zero).
    const uint32_t* s_lut;
    int s_lut_n;
    const uint32_t* s_off;
    const uint32_t* s_lcw;
    const uint32_t* s_tog;
    // logicals (fused failure check)
    int k, lz_words;
    const uint64_t* lz;           // [k][lz_words]    bit q%64 of word q/64 (nullptr when too large)
    const uint64_t* ms_lzs;       // wave graphs: [k][n_pad/64] the same by min-sum lane slot (ms_vslot order)
    // the same logicals as CSR supports over data qubits (always set with k > 0);
    // lz_sparse: the workgroup finalize tests logicals on their supports (nnz small
    // against k * lz_words) instead of by dense words
    const int32_t* lz_ptr;        // [k+1]
    const int32_t* lz_idx;        // [nnz]
    int lz_sparse;
    // the same logicals by qubit: word t of qubit q holds bit r % 32 of logical
    // r = 32 t + (r % 32) (nullptr when n_data * lz_tw words exceed 64 MB).  The
    // workgroup finalizes test a residual through it: only the residual's ones
    // read their qubit's lz_tw words, so a decoded shot (residual zero or a
    // stabilizer) costs a few words instead of k * lz_words
    const uint32_t* lz_t;         // [n_data][lz_tw]
    int lz_tw;
    // per-handle kernel choices (qd_graph_set_option, QD_OPT_* in include/qdec.h;
    // defaults from default_options): the launchers read these, never the
    // environment
    int opt_compact;       // 1: two-pass lean min-sum decodes (triage + compact list); 0: one-pass kernel
    int opt_triage_it1;    // 1: min-sum iteration 1 inside the triage; 0: left to the BP kernel
    int opt_ssf;           // QD_SSF_*: table-driven, scanning (incremental / re-gathered / unsplit scorer)
    int opt_lds_kernel;    // -1: automatic; 0: never; 1: forced (bp_ms_lds_kernel)
    int opt_group_kernel;  // -1: automatic; 0: never; 1: forced (bp_group_kernel)
    int opt_ssf_inc;       // 1: incremental workgroup SSF (ssf_inc_block_kernel); 0: the re-scanning one
    int opt_block_wg;      // > 0: workgroups per CU of the HBM-slice workgroup kernels (0: automatic)
    int opt_group_mb;      // > 0: HBM budget of the slot-group scratch in MiB (0: a quarter of free HBM)
    int opt_ssf_fuse;      // 1: two-pass SSF decodes run SSF inside the compact BP kernel (no queue, no
                           // second launch); 0 (default): queue + ssf_lut_kernel
};

// SSF kernel choice of wave graphs (DevGraph::opt_ssf)
enum { kSsfAuto = 0, kSsfScan = 1, kSsfScanGather = 2, kSsfScanNoSplit = 3 };
inline void default_options(DevGraph& g) {
    g.opt_compact = 1;
    g.opt_triage_it1 = 1;
    g.opt_ssf = kSsfAuto;
    g.opt_lds_kernel = -1;
    g.opt_group_kernel = -1;
    g.opt_ssf_inc = 1;
    g.opt_block_wg = 0;
    g.opt_group_mb = 0;
    g.opt_ssf_fuse = 0;  // measured: 2x the separate SSF kernel's time at p = 0.1 (profiles/r06c)
}

}  // namespace qdec
