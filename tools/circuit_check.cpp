// circuit_check.cpp -- the circuit program validator (exp_ldpc_amd/csrc/qdec_circuit.cpp)
// as a stand-alone program, so it can run under ASan + UBSan with a static
// runtime and no GPU stack:
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       tools/circuit_check.cpp exp_ldpc_amd/csrc/qdec_circuit.cpp exp_ldpc_amd/csrc/qdec_tables.cpp \
//       -o circuit_check
//   circuit_check   ->  one line per case, "<case> <code>", exit 0 when every code is the expected one
//
// A valid two-qubit program and one broken variant per refusal of
// qd_circuit_create (include/qdec.h): the arrays are sized exactly, so a read
// past a bound the validator should have checked first is a sanitizer report.
// Every program that validates also has its elementary-fault tables built
// (circuit_fault_table, both kinds) into arrays of exactly the counted size and
// checked: instruction and target in range, the faults in program order.
// The PAULI_CHANNEL_1 / 2 cases go through the argument array of
// qd_circuit_create_args: offsets before, across and behind its end, arguments and
// sums out of range, and the entry points without the array.
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
    bool with_args = false;  // the entry points that take an argument array
    std::vector<double> args;
};

// PAULI_CHANNEL_1 on three targets (one named twice), PAULI_CHANNEL_2 on two pairs, a measurement
static Program channels() {
    Program p;
    p.Q = 3;
    p.ops = {FO_PC1, 0, 3, 0, FO_PC2, 3, 4, 3, FO_M, 7, 3, 0};
    p.targets = {0, 1, 0, 0, 1, 1, 2, 0, 1, 2};
    p.args = {0.02, 0.05, 0.11};
    double sum = 0.0;
    for (int k = 1; k <= 15; ++k) p.args.push_back(0.004 * k), sum += 0.004 * k;
    p.probs = {0.02 + 0.05 + 0.11, sum, 0.0};
    p.rows = {1}, p.row_ptr = {0, 1}, p.rec_idx = {2};
    p.with_args = true;
    return p;
}

// 0 when the fault tables of a validated program are consistent with it
static int walk_faults(const HostCircuit& c) {
    for (int kind = 0; kind < 2; ++kind) {
        const int32_t n = fault_total(c, kind);
        std::vector<int32_t> op(n), tgt(n), comp(n);
        circuit_fault_table(c, kind, op.data(), tgt.data(), comp.data());
        for (int32_t f = 0; f < n; ++f) {
            if (op[f] < 0 || op[f] >= (int32_t)c.ops.size() || (f && op[f] < op[f - 1])) return -1;
            const FrameOpRec& r = c.ops[op[f]];
            if (tgt[f] < r.tgt_off || tgt[f] >= r.tgt_off + r.tgt_cnt || comp[f] < FC_X || comp[f] > FC_REC) return -1;
            if (f < (kind ? (int32_t)r.rsite0 : r.fault0)) return -1;
        }
    }
    return 0;
}

static int code_of(const Program& p, int* faults = nullptr) {
    HostCircuit c;
    try {
        build_circuit(c, p.Q, (int32_t)p.ops.size() / 4, p.ops.data(), (int32_t)p.targets.size(), p.targets.data(),
                      p.probs.data(), (int32_t)p.rows.size(), p.rows.data(), p.row_ptr.data(), p.rec_idx.data(), false,
                      p.with_args ? (int32_t)p.args.size() : -1, p.args.data());
        for (const FrameOpRec& r : c.ops)  // the kernel reads channel_args(op) thresholds from cum_off on
            if (r.cum_off < 0 || (size_t)r.cum_off + channel_args(r.op) > c.cum.size() ||
                (channel_args(r.op) && c.cum[r.cum_off + channel_args(r.op) - 1] != r.thr))
                return -1;
        if (faults) faults[0] = fault_total(c, 0), faults[1] = fault_total(c, 1);
        if (walk_faults(c) != 0) return -1;
        int32_t one = 0;
        circuit_fault_table(c, 2, &one, &one, &one);  // a bad kind is refused before anything is written
        return -1;
    } catch (const Fail& e) {
        return e.code == -87 ? 0 : e.code;
    }
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
    int faults[2] = {0, 0};
    code_of(p, faults);  // DEPOLARIZE1 on one target and two noisy measurements; two measurement gauges
    std::printf("valid_faults %d %d\n", faults[0], faults[1]);
    bad += faults[0] != 4 || faults[1] != 2;
    p = Program();  // every fault-carrying opcode: X/Y/Z_ERROR, DEPOLARIZE2, R, RX, MX
    p.ops = {FO_R, 0, 2, 0, FO_RX, 0, 1, 0, FO_XERR, 0, 2, 0, FO_YERR, 0, 1, 0, FO_ZERR, 1, 1, 0,
             FO_DEP2, 0, 2, 0, FO_MX, 0, 1, 0, FO_M, 1, 1, 0};
    p.targets = {0, 1};
    p.probs = {0.0, 0.0, 0.1, 0.0, 0.2, 0.3, 0.0, 0.5};
    code_of(p, faults);
    std::printf("all_fault_ops %d %d %d\n", code_of(p), faults[0], faults[1]);
    bad += code_of(p) != 0 || faults[0] != 10 || faults[1] != 5;
    p = Program();
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
    // PAULI_CHANNEL_1 / 2
    p = channels();
    expect("channels", p, 0);
    code_of(p, faults);  // two faults per PAULI_CHANNEL_1 target, four per PAULI_CHANNEL_2 pair, three measurements
    std::printf("channel_faults %d %d\n", faults[0], faults[1]);
    bad += faults[0] != 6 + 8 + 3 || faults[1] != 3;
    p = channels(), p.with_args = false;
    expect("channels_without_array", p, -71);
    p = channels(), p.ops[7] = 4;  // the last of its 15 arguments lies one past the end
    expect("arg_range_across_end", p, -71);
    p = channels(), p.ops[7] = 18;
    expect("arg_range_behind_end", p, -71);
    p = channels(), p.ops[3] = -1;
    expect("arg_range_negative", p, -71);
    p = channels(), p.ops[3] = 0x7fffffff;
    expect("arg_range_overflow", p, -71);
    p = channels(), p.args.clear();
    expect("arg_array_empty", p, -71);
    p = channels(), p.ops[11] = 1;
    expect("arg_offset_on_measurement", p, -71);
    p = Program(), p.with_args = true, p.ops[3] = 2;
    expect("arg_offset_on_gate", p, -71);
    p = channels(), p.args[1] = -0.05, p.probs[0] = 0.08;
    expect("arg_negative", p, -75);
    p = channels(), p.args[4] = 1.5;
    expect("arg_above_one", p, -75);
    p = channels(), p.args[2] = 0.9301, p.probs[0] = 1.0001;
    expect("arg_sum_above_one", p, -75);
    p = channels(), p.probs[1] += 1e-9;
    expect("probability_is_not_the_sum", p, -75);
    p = channels(), p.targets[4] = 3;
    expect("channel_qubit_out_of_range", p, -72);
    p = channels(), p.ops[6] = 3, p.ops[9] = 6, p.ops[10] = 4;
    expect("channel_odd_pairs", p, -71);
    return bad ? 1 : 0;
}
