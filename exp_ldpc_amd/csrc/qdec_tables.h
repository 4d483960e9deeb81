// qdec_tables.h -- host-side graph preparation (qdec_tables.cpp): CSR -> per-lane
// slot tables for the wave kernels, the LDS layouts, flip-set tables for SSF,
// bit-packed logicals, priors in both precisions, the queue layout.  Pure host
// code with no HIP header: every table goes through a TableSink, which the
// library backs with device memory (qdec_abi.h) and a host-only graph or a
// stand-alone checker (tools/tables_check.cpp) with plain host copies.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "qdec_graph.h"

namespace qdec {

// an error with the code the ABI call returns
struct Fail : std::runtime_error {
    int code;
    Fail(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

// Bernoulli(p) as a 32-bit threshold: a uniform u32 word u fires when u < thr.
// floor(p 2^32) clamped to 0xFFFFFFFF; anything not > 0 (NaN included) never
// fires.  The one conversion of both samplers (qd_sample_storage_*: its two
// event probabilities; qd_sample_faults_device: smp_thr).
inline uint32_t bern_threshold(double p) {
    if (!(p > 0)) return 0u;
    const double v = std::floor(p * 4294967296.0);
    return v >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)v;
}

// Where the builders put a finished table: a copy that stays valid until
// release().  At least 16 bytes are allocated, so an empty table still has an
// address.
struct TableSink {
    virtual ~TableSink() = default;
    virtual const void* put(const void* src, size_t bytes) = 0;
    virtual void release() = 0;
    template <typename T>
    const T* upload(const std::vector<T>& h) {
        return static_cast<const T*>(put(h.data(), h.size() * sizeof(T)));
    }
};

// keeps the bytes on the host, in upload order (table_digest hashes them)
struct HostSink : TableSink {
    std::vector<std::vector<uint8_t>> kept;
    const void* put(const void* src, size_t bytes) override {
        kept.emplace_back(std::max<size_t>(bytes, 16), 0);
        if (bytes) std::memcpy(kept.back().data(), src, bytes);
        return kept.back().data();
    }
    void release() override { kept.clear(); }
};

// What the builders read and write: the host copies needed to rebuild tables,
// the graph description the kernels get, and one sink per table group (a group
// is released and rebuilt as a whole).
struct HostGraph {
    DevGraph dg{};
    std::vector<int32_t> row_ptr, col_idx;
    std::vector<int32_t> col_ptr, col_rows;  // CSC (row ids, ascending)
    // min-sum wave kernel: variable (column) held by each lane slot, -1 for pads
    std::vector<int> ms_var_of_slot;
    std::unique_ptr<TableSink> arena;        // graph tables
    std::unique_ptr<TableSink> flip_arena, lz_arena, prior_arena;
    // set_priors: every probability lay inside (0, 1), so the BP priors exist;
    // false after a call with a 0 or a 1 among them (sampler thresholds only)
    bool bp_priors = false;
    // the f64 min-sum priors log((1 - p) / p) of the last such call, kept on the
    // host (empty otherwise): the relay stage's solution weights come from them
    std::vector<double> prior_ms64;
    // fault sampler (sample_faults_kernel, qdec_sample.hip; kept beside DevGraph,
    // which every decode kernel takes by value): column j fires when a Philox
    // word is < smp_thr[j] (bern_threshold of the probability last given to
    // set_priors; zero entries pad n to a multiple of 4; nullptr before the
    // first set_priors), and then toggles the rows smp_crow[col_ptr[j] ..
    // col_ptr[j + 1]) (the row of each edge in CSC order)
    const uint32_t* smp_thr = nullptr;   // [(n + 3) / 4 * 4], prior_arena
    const int32_t* smp_crow = nullptr;   // [max(E, 1)], arena
};

// The build sequence of a graph handle.  init_graph expects a validated CSR
// (row_ptr monotone from 0, columns in range and strictly ascending in a row)
// and sinks in place; the set_* calls may follow in any order and be repeated.
// Each throws Fail on arguments it cannot build tables from.
void init_graph(HostGraph* G, int m, int n, const int32_t* row_ptr, const int32_t* col_idx, int n_data,
                int fold_blocks);
void set_flipsets(HostGraph* G, int32_t n_gen, const int32_t* gen_ptr, const int32_t* gen_idx);
void set_logicals(HostGraph* G, int32_t k, const uint8_t* lz);  // dense [k][n_data]
void set_logicals_csr(HostGraph* G, int32_t k, const int32_t* lz_ptr, const int32_t* lz_idx);
// probabilities in [0, 1].  Inside (0, 1) throughout: the BP priors and the
// sampler thresholds; with a 0 or a 1 among them BP has no finite message, so
// only the thresholds are built (G->bp_priors = false; decodes then refuse)
void set_priors(HostGraph* G, const double* probs);

// FNV-1a over every table in upload order (graph, flip sets, logicals, priors)
// and their total size; the graph's sinks must be HostSinks
void table_digest(const HostGraph* G, uint64_t* digest, int64_t* bytes);
// the fault sampler's tables of a host-only graph: thr[n], crow[E] (null outputs are skipped)
void sample_tables_copy(const HostGraph* G, uint32_t* thr, int32_t* crow);
// the table-driven wave SSF tables of a host-only graph (null outputs are skipped)
void ssf_tables_copy(const DevGraph& g, uint32_t* lut, uint32_t* off, uint32_t* lcw, uint32_t* tog, int32_t* g_pad,
                     int32_t* m_pad);

// Words of a compact-list entry (wave graphs; qdec_cmp_list.h CmpEntry): shot,
// syndrome words, readout logical-parity words.
size_t cmp_entry_bytes(const DevGraph& g);

// Byte layout of the queue scratch for a capacity of `cap` shots: the queue
// count (256 B), idx[cap] u64, then the byte-format x[cap][n] | r[cap][m] region
// (the packed format of the wave kernels reuses it for [cap][1 + 2 n_pad/64 +
// m_pad/64] u64 entries), and for wave graphs the compact shot list:
// kCmpSegs counters on their own 128-B lines (the triage's u64 atomics need
// natural alignment, so the region starts on a 256-B boundary), then the
// segments of cmp_seg_cap(cap) entries.
struct QueueLayout {
    size_t bytes, idx, x, r, cmp_count, cmp;
    int64_t cmp_cap;
};
QueueLayout queue_layout(const DevGraph& g, int64_t cap);

}  // namespace qdec
