// tables_check.cpp -- the host table builders (exp_ldpc_amd/csrc/qdec_tables.cpp)
// as a stand-alone program, so they can run under ASan + UBSan with a static
// runtime and no GPU stack:
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       tools/tables_check.cpp exp_ldpc_amd/csrc/qdec_tables.cpp -o tables_check
//   tables_check graph.bin      ->  "<FNV-1a digest, 16 hex digits> <table bytes>"
//
// It runs the build sequence of a host-only graph handle (tables, flip sets,
// logicals, priors with the iteration-1 and first-check-state tables) on host
// sinks and prints what qd_graph_table_digest reports for the same input
// (tests/test_tables_standalone.py compares the two).
//
// Input, little-endian: 10 x i32 header {m, n, n_data, fold_blocks, nnz, n_gen,
// gen_nnz, k, lz_nnz, has_priors} (n_gen / k = -1: that call is skipped), then
// i32 row_ptr[m+1], col_idx[nnz], gen_ptr[n_gen+1], gen_idx[gen_nnz],
// lz_ptr[k+1], lz_idx[lz_nnz], then f64 priors[n].  The CSR must be valid
// (the library validates it before it builds; this program does not).
#include <cstdio>
#include <fstream>
#include <iterator>

#include "../exp_ldpc_amd/csrc/qdec_tables.h"

using namespace qdec;

int main(int argc, char** argv) {
    if (argc != 2) return std::fprintf(stderr, "usage: tables_check graph.bin\n"), 2;
    std::ifstream in(argv[1], std::ios::binary);
    const std::vector<char> buf((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    size_t at = 0;
    bool ok = true;  // a file that cannot be opened reads as empty and fails below
    auto take = [&](auto& v, int64_t count) {  // the next `count` elements (none for count < 0)
        v.resize(count > 0 ? (size_t)count : 0);
        const size_t bytes = v.size() * sizeof(v[0]);
        if (bytes > buf.size() - at) return void(ok = false);
        if (bytes) std::memcpy(v.data(), buf.data() + at, bytes);
        at += bytes;
    };
    std::vector<int32_t> hd, rp, ci, gp, gi, lp, li;
    std::vector<double> pr;
    take(hd, 10);
    if (!ok) return std::fprintf(stderr, "tables_check: cannot read %s\n", argv[1]), 2;
    const int m = hd[0], n = hd[1], n_gen = hd[5], k = hd[7];
    take(rp, (int64_t)m + 1);
    take(ci, hd[4]);
    take(gp, n_gen < 0 ? 0 : (int64_t)n_gen + 1);
    take(gi, hd[6]);
    take(lp, k < 0 ? 0 : (int64_t)k + 1);
    take(li, hd[8]);
    take(pr, hd[9] ? n : 0);
    if (!ok || at != buf.size() || m <= 0 || n <= 0 || rp[m] != hd[4])
        return std::fprintf(stderr, "tables_check: %s does not match its header\n", argv[1]), 2;
    try {
        HostGraph G;
        for (auto* sink : {&G.arena, &G.flip_arena, &G.lz_arena, &G.prior_arena}) sink->reset(new HostSink());
        init_graph(&G, m, n, rp.data(), ci.data(), hd[2], hd[3]);
        if (n_gen >= 0) set_flipsets(&G, n_gen, gp.data(), gi.data());
        if (k >= 0) set_logicals_csr(&G, k, lp.data(), li.data());
        if (hd[9]) set_priors(&G, pr.data());
        uint64_t digest = 0;
        int64_t bytes = 0;
        table_digest(&G, &digest, &bytes);
        std::printf("%016llx %lld\n", (unsigned long long)digest, (long long)bytes);
    } catch (const Fail& e) {
        return std::fprintf(stderr, "tables_check: error %d: %s\n", e.code, e.what()), 2;
    }
    return 0;
}
