// qdec_window.cpp -- validation of a window boundary's tables (qdec_window.h).
// Pure host code with no HIP header: qd_window_create and qd_window_create_host
// both go through window_build, and tools/window_check.cpp links this unit alone.
#include "qdec_window.h"

namespace qdec {

namespace {

// ptr[0 .. rows] monotone from 0 (-24); it bounds every later read of the columns
void check_ptr(const std::string& w, int32_t rows, const int32_t* ptr) {
    if (!ptr) throw Fail(-26, "window: null " + w + " pointer array");
    if (ptr[0] != 0) throw Fail(-24, "window: " + w + " pointer array does not start at 0");
    for (int32_t i = 0; i < rows; ++i)
        if (ptr[i + 1] < ptr[i]) throw Fail(-24, "window: " + w + " pointer array decreases at row " + std::to_string(i));
}

// every column inside [0, n_w) (-23)
void check_cols(const std::string& w, int32_t nnz, const int32_t* cols, int32_t n_w) {
    if (nnz > 0 && !cols) throw Fail(-26, "window: null " + w + " column array");
    for (int32_t e = 0; e < nnz; ++e)
        if (cols[e] < 0 || cols[e] >= n_w)
            throw Fail(-23, "window: " + w + " column " + std::to_string(cols[e]) + " outside the window's " +
                                std::to_string(n_w) + " columns");
}

void copy(std::vector<int32_t>& to, const int32_t* from, int32_t count) {
    to.clear();
    if (count > 0) to.assign(from, from + count);
}

}  // namespace

void window_build(WindowTables& t, int32_t n_w, int32_t m_total, int32_t n_carry, const int32_t* carry_rows,
                  const int32_t* carry_ptr, const int32_t* carry_cols, int32_t k_acc, const int32_t* acc_ptr,
                  const int32_t* acc_cols, int32_t row0, int32_t m_next) {
    if (n_w < 1 || n_w > kWindowMaxCols || m_total < 0 || n_carry < 0 || k_acc < 0)
        throw Fail(-26, "window: sizes must satisfy 1 <= n_w <= 2^19 and m_total, n_carry, k_acc >= 0");
    if (row0 < 0 || m_next < 0 || (int64_t)row0 + m_next > m_total)
        throw Fail(-25, "window: rows " + std::to_string(row0) + " .. " + std::to_string((int64_t)row0 + m_next) +
                            " of the next window lie outside the " + std::to_string(m_total) + " syndrome rows");
    check_ptr("carry", n_carry, carry_ptr);
    check_ptr("accumulator", k_acc, acc_ptr);
    if (n_carry > 0 && !carry_rows) throw Fail(-26, "window: null carry row list");
    for (int32_t i = 0; i < n_carry; ++i)
        if (carry_rows[i] < 0 || carry_rows[i] >= m_total || (i > 0 && carry_rows[i] <= carry_rows[i - 1]))
            throw Fail(-22, "window: carry rows must be strictly ascending inside [0, " + std::to_string(m_total) +
                                ") (entry " + std::to_string(i) + ")");
    check_cols("carry", carry_ptr[n_carry], carry_cols, n_w);
    check_cols("accumulator", acc_ptr[k_acc], acc_cols, n_w);
    t.n_w = n_w, t.m_total = m_total, t.n_carry = n_carry, t.k_acc = k_acc, t.row0 = row0, t.m_next = m_next;
    copy(t.carry_rows, carry_rows, n_carry);
    copy(t.carry_ptr, carry_ptr, n_carry + 1);
    copy(t.carry_cols, carry_cols, carry_ptr[n_carry]);
    copy(t.acc_ptr, acc_ptr, k_acc + 1);
    copy(t.acc_cols, acc_cols, acc_ptr[k_acc]);
}

}  // namespace qdec
