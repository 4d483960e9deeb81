// qdec_window.h -- the step between two windows of a sliding-window decode
// (window_advance_kernel, qdec_window.hip; DESIGN 3.6e has the spec): the tables
// of one window boundary, their validation (qdec_window.cpp) and the launch
// arguments.  Pure host code with no HIP header, so the ABI unit, the kernel
// unit and the stand-alone checker (tools/window_check.cpp) read the same rules.
#pragma once
#include "qdec_tables.h"

namespace qdec {

constexpr int kWindowBlock = 256;              // threads of a workgroup
constexpr int32_t kWindowMaxCols = 1 << 19;    // the x row as bits: 64 KiB of LDS
constexpr int64_t kWindowMaxBlocks = 1ll << 20;
constexpr int kWindowBlocksPerCu = 8;          // workgroups per CU by default

// One boundary, validated (window_build).  Carry row i is global row
// carry_rows[i] of the full syndrome and reads the window-local columns
// carry_cols[carry_ptr[i] .. carry_ptr[i + 1]); accumulator row i reads
// acc_cols[acc_ptr[i] .. acc_ptr[i + 1]).  The next window's syndrome is rows
// row0 .. row0 + m_next of the full one.
struct WindowTables {
    int32_t n_w = 0, m_total = 0, n_carry = 0, k_acc = 0, row0 = 0, m_next = 0;
    std::vector<int32_t> carry_rows, carry_ptr, carry_cols, acc_ptr, acc_cols;
};

// Copies the arrays into t after checking them; throws Fail:
//   -26 a null output or array, a negative size, n_w above kWindowMaxCols
//   -25 row0 < 0, m_next < 0 or row0 + m_next > m_total
//   -24 a pointer array that does not start at 0 or decreases
//   -22 carry rows not strictly ascending or outside [0, m_total)
//   -23 a column outside [0, n_w)
void window_build(WindowTables& t, int32_t n_w, int32_t m_total, int32_t n_carry, const int32_t* carry_rows,
                  const int32_t* carry_ptr, const int32_t* carry_cols, int32_t k_acc, const int32_t* acc_ptr,
                  const int32_t* acc_cols, int32_t row0, int32_t m_next);

// What the kernel reads: the tables on the device.
struct WindowDev {
    int32_t n_w, m_total, n_carry, k_acc, row0, m_next;
    const int32_t *carry_rows, *carry_ptr, *carry_cols, *acc_ptr, *acc_cols;
};

struct WindowArgs {
    int64_t B;
    const uint8_t* x;   // [B][n_w] nullable: no carry, no accumulate
    uint8_t* syn_full;  // [B][m_total], updated in place
    uint8_t* acc_out;   // [B][k_acc] nullable
    uint8_t* syn_next;  // [B][m_next] nullable
};

// Workgroups of a launch over B shots: `cfg` when set, else kWindowBlocksPerCu
// per compute unit; at most B.
inline int64_t window_grid(int64_t cfg, int num_cus, int64_t B) {
    const int64_t want = cfg > 0 ? cfg : (int64_t)std::max(num_cus, 1) * kWindowBlocksPerCu;
    return std::max<int64_t>(1, std::min(want, B));
}

}  // namespace qdec
