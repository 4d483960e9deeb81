// circuit_check.cpp -- the circuit program validator (exp_ldpc_amd/csrc/qdec_circuit.cpp)
// as a stand-alone program, so it can run under ASan + UBSan with a static
// runtime and no GPU stack:
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       tools/circuit_check.cpp exp_ldpc_amd/csrc/qdec_circuit.cpp -o circuit_check
//   circuit_check   ->  one line per case, "<case> <code>", exit 0 when every code is the expected one
//
// A valid two-qubit program and one broken variant per refusal of
// qd_circuit_create (include/qdec.h): the arrays are sized exactly, so a read
// past a bound the validator should have checked first is a sanitizer report.
#include <cstdio>
#include <vector>

#include "../exp_ldpc_amd/csrc/qdec_circuit.h"
#include "../exp_ldpc_amd/csrc/qdec_tables.h"

using namespace qdec;

struct Program {
    int32_t Q = 2;
    std::vector<int32_t> ops{FO_CX, 0, 2, 0, FO_DEP1, 2, 1, 0, FO_M, 3, 2, 0};
    std::vector<int32_t> targets{0, 1, 0, 0, 1};
    std::vector<double> probs{0.0, 0.5, 0.25};
    std::vector<int32_t> rows{1}, row_ptr{0, 2}, rec_idx{0, 1};
};

static int code_of(const Program& p) {
    HostCircuit c;
    try {
        build_circuit(c, p.Q, (int32_t)p.ops.size() / 4, p.ops.data(), (int32_t)p.targets.size(), p.targets.data(),
                      p.probs.data(), (int32_t)p.rows.size(), p.rows.data(), p.row_ptr.data(), p.rec_idx.data());
    } catch (const Fail& e) {
        return e.code;
    }
    return 0;
}

int main() {
    int bad = 0;
    auto expect = [&](const char* name, const Program& p, int want) {
        const int got = code_of(p);
        std::printf("%s %d\n", name, got);
        bad += got != want;
    };
    Program p;
    expect("valid", p, 0);
    p = Program(), p.targets[1] = 2;
    expect("qubit_out_of_range", p, -72);
    p = Program(), p.rec_idx[0] = -1;
    expect("record_before_start", p, -73);
    p = Program(), p.rec_idx[1] = 2;
    expect("record_not_measured", p, -73);
    p = Program(), p.targets[1] = 0;
    expect("repeated_qubit", p, -74);
    p = Program(), p.probs[1] = 1.5;
    expect("probability", p, -75);
    p = Program(), p.ops[10] = 3;
    expect("target_range", p, -71);
    p = Program(), p.ops[8] = FO_COUNT;
    expect("opcode", p, -71);
    p = Program(), p.row_ptr[0] = 1;
    expect("csr_start", p, -71);
    p = Program(), p.Q = (int32_t)(kFrameLdsLimit / 16) + 1;
    expect("lds_limit", p, -76);
    return bad ? 1 : 0;
}
