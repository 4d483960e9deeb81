// qdec_tables.h -- host-side graph preparation (qdec_tables.cpp): CSR -> per-lane
// slot tables for the wave kernels, the LDS layouts, flip-set tables for SSF,
// bit-packed logicals, priors in both precisions, the queue layout.  Pure host
// code with no HIP header: every table goes through a TableSink, which the
// library backs with device memory (qdec_abi.cpp) and a host-only graph or a
// stand-alone checker (tools/tables_check.cpp) with plain host copies.
#pragma once
#include <stdint.h>

#include <algorithm>
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
void set_priors(HostGraph* G, const double* probs);

// FNV-1a over every table in upload order (graph, flip sets, logicals, priors)
// and their total size; the graph's sinks must be HostSinks
void table_digest(const HostGraph* G, uint64_t* digest, int64_t* bytes);
// the table-driven wave SSF tables of a host-only graph (null outputs are skipped)
void ssf_tables_copy(const DevGraph& g, uint32_t* lut, uint32_t* off, uint32_t* lcw, uint32_t* tog, int32_t* g_pad,
                     int32_t* m_pad);

// Words of a compact-list entry (wave graphs; qdec_bp_ms.h CmpEntry): shot,
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
