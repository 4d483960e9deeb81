// window_check.cpp -- the validation of a window boundary's tables
// (exp_ldpc_amd/csrc/qdec_window.cpp, the unit qd_window_create and
// qd_window_create_host go through) as a stand-alone program, so it runs under
// ASan + UBSan with a static runtime and no GPU stack (no HIP header is on the
// include path; it links that unit alone):
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       tools/window_check.cpp exp_ldpc_amd/csrc/qdec_window.cpp -o window_check
//   window_check   ->  one "name code" line per case
//
// Every array is a heap block of exactly its length, so a read past a table
// that validation should have bounded is a sanitizer report.
// tests/test_window_host.py compares the output with the expected codes.
#include <cstdio>
#include <vector>

#include "../exp_ldpc_amd/csrc/qdec_window.h"

using namespace qdec;

struct Case {
    int32_t n_w = 8, m_total = 10, row0 = 4, m_next = 6;
    std::vector<int32_t> rows{4, 7, 9}, cptr{0, 2, 2, 3}, ccols{0, 7, 3}, aptr{0, 1, 3}, acols{7, 0, 1};
};

static const int32_t* data(const std::vector<int32_t>& v) {
    return v.empty() ? nullptr : v.data();
}

static void run(const char* name, const Case& c) {
    WindowTables t;
    int code = 0;
    try {
        window_build(t, c.n_w, c.m_total, (int32_t)c.rows.size(), data(c.rows), data(c.cptr), data(c.ccols),
                     (int32_t)c.aptr.size() - 1, data(c.aptr), data(c.acols), c.row0, c.m_next);
        // a built table is read in full, as the upload would
        long sum = 0;
        for (const auto* v : {&t.carry_rows, &t.carry_ptr, &t.carry_cols, &t.acc_ptr, &t.acc_cols})
            for (int32_t e : *v) sum += e;
        if (sum < 0) code = 1;
    } catch (const Fail& f) {
        code = f.code;
    }
    std::printf("%s %d\n", name, code);
}

int main() {
    Case c;
    run("valid", c);
    c = Case(), c.rows = {}, c.cptr = {0}, c.ccols = {}, c.aptr = {0}, c.acols = {};
    run("empty_tables", c);
    c = Case(), c.ccols[1] = 7, c.acols[0] = 7;
    run("last_column", c);
    c = Case(), c.rows = {4, 9, 7};
    run("carry_rows_unsorted", c);
    c = Case(), c.rows = {4, 7, 7};
    run("carry_row_repeated", c);
    c = Case(), c.rows = {4, 7, 10};
    run("carry_row_out_of_range", c);
    c = Case(), c.rows = {-1, 7, 9};
    run("carry_row_negative", c);
    c = Case(), c.ccols[2] = 8;
    run("carry_column_out_of_range", c);
    c = Case(), c.acols[1] = -1;
    run("acc_column_negative", c);
    c = Case(), c.acols[2] = 8;
    run("acc_column_out_of_range", c);
    c = Case(), c.cptr = {0, 2, 1, 3};
    run("carry_ptr_decreases", c);
    c = Case(), c.cptr = {1, 2, 2, 3};
    run("carry_ptr_not_from_zero", c);
    c = Case(), c.aptr = {0, 3, 1};
    run("acc_ptr_decreases", c);
    c = Case(), c.row0 = 5;
    run("next_rows_beyond_total", c);
    c = Case(), c.row0 = 0x7fffffff, c.m_next = 0x7fffffff;
    run("next_rows_overflow", c);
    c = Case(), c.n_w = 0;
    run("no_columns", c);
    c = Case(), c.n_w = (1 << 19) + 1;
    run("too_many_columns", c);
    return 0;
}
