// qdec_circuit.cpp -- validation of a compiled Pauli-frame program (HIP-free).
// Nothing the kernel indexes with is taken on trust: every qubit, every record
// reference and every CSR bound is checked here, once, at create.
#include "qdec_circuit.h"

#include <string>

#include "qdec_tables.h"

namespace qdec {

void build_circuit(HostCircuit& c, int32_t num_qubits, int32_t n_ops, const int32_t* ops, int32_t n_targets,
                   const int32_t* targets, const double* probs, int32_t n_groups, const int32_t* group_rows,
                   const int32_t* row_ptr, const int32_t* rec_idx, bool beyond_lds, int32_t n_args,
                   const double* args) {
    if (num_qubits < 1 || num_qubits > kFrameQubitMask || n_ops < 0 || n_targets < 0 || n_groups < 0 ||
        n_groups > kFrameGroups)
        throw Fail(-71, "circuit: bad sizes (1 <= qubits, 0 <= ops, targets, 0 <= groups <= 4)");
    if ((n_ops && (!ops || !probs)) || (n_targets && !targets) || (n_groups && (!group_rows || !row_ptr)))
        throw Fail(-71, "circuit: null program array");
    if (n_args > 0 && !args) throw Fail(-71, "circuit: null program array");
    c.Q = num_qubits;
    c.cum.clear();
    c.ops.clear();
    c.ops.reserve(n_ops);
    c.targets.assign(targets, targets + n_targets);
    std::vector<int32_t> seen(num_qubits, -1);  // the last op that touched a qubit
    uint64_t site = 0, rsite = 0, rec = 0, fault = 0;
    for (int32_t i = 0; i < n_ops; ++i) {
        const int32_t op = ops[4 * i], off = ops[4 * i + 1], cnt = ops[4 * i + 2];
        const std::string at = " (instruction " + std::to_string(i) + ")";
        if (op < 0 || op >= FO_COUNT || (channel_args(op) && n_args < 0))
            throw Fail(-71, "circuit: unknown opcode" + at);
        if (off < 0 || cnt < 0 || (int64_t)off + cnt > n_targets) throw Fail(-71, "circuit: target range outside the target array" + at);
        const bool pair = op == FO_CX || op == FO_CZ || pair_noise(op);
        if (pair && (cnt & 1)) throw Fail(-71, "circuit: odd target count of a two-qubit instruction" + at);
        const bool meas = op == FO_M || op == FO_MX;
        const bool noise = op >= FO_XERR;
        const double p = probs[i];
        bool dup = false;
        if (channel_args(op)) {
            // checked against the sum of its arguments below (which rounding may leave a hair above 1)
        } else if (noise || meas) {
            if (!(p >= 0.0 && p <= 1.0)) throw Fail(-75, "circuit: probability outside [0, 1]" + at);
        } else if (p != 0.0) {
            throw Fail(-75, "circuit: a gate or reset takes no probability" + at);
        }
        for (int32_t e = off; e < off + cnt; ++e) {
            const int32_t t = targets[e];
            if (t < 0 || (!meas && (t & kFrameInvert)) || (t & kFrameQubitMask) >= num_qubits)
                throw Fail(-72, "circuit: qubit index out of range" + at);
            const int32_t q = t & kFrameQubitMask;
            if (seen[q] == i) {  // lanes split a gate's targets: they must be pairwise disjoint
                if (!noise) throw Fail(-74, "circuit: a qubit twice in one parallel group" + at);
                dup = true;      // legal in a noise line; the HBM kernels apply its sites in order
            }
            seen[q] = i;
        }
        FrameOpRec r{};
        r.dup = dup;
        r.op = op, r.tgt_off = off, r.tgt_cnt = cnt;
        r.thr = bern_threshold(p);
        const int32_t K = channel_args(op), a0 = ops[4 * i + 3];
        if (!K) {
            if (a0 != 0) throw Fail(-71, "circuit: an argument offset on an instruction without arguments" + at);
        } else {
            if (a0 < 0 || (int64_t)a0 + K > n_args) throw Fail(-71, "circuit: argument range outside the argument array" + at);
            double sum = 0.0;  // c_k, summed left to right
            r.cum_off = (int32_t)c.cum.size();
            for (int32_t k = 0; k < K; ++k) {
                const double a = args[a0 + k];
                if (!(a >= 0.0 && a <= 1.0)) throw Fail(-75, "circuit: channel argument outside [0, 1]" + at);
                sum += a;
                c.cum.push_back(bern_threshold(sum));
            }
            if (sum > 1.0 + 1e-12) throw Fail(-75, "circuit: channel arguments sum to more than 1" + at);
            if (!(p >= sum - 1e-12 && p <= sum + 1e-12))
                throw Fail(-75, "circuit: the probability of a channel is not the sum of its arguments" + at);
            r.thr = c.cum.back();
        }
        r.site0 = (uint32_t)site, r.rsite0 = (uint32_t)rsite, r.rec0 = (int32_t)rec, r.fault0 = (int32_t)fault;
        fault += (uint64_t)fault_count(op, cnt, 0);
        if (noise || meas) site += ((uint64_t)(pair_noise(op) ? cnt / 2 : cnt) + 3) / 4 * 4;
        if (meas || op == FO_R || op == FO_RX) rsite += (uint64_t)cnt;
        if (meas) rec += (uint64_t)cnt;
        if (site >= (1ull << 31) || rsite >= (1ull << 31) || rec >= (1ull << 28) || fault >= (1ull << 30) ||
            c.cum.size() >= (1ull << 30))
            throw Fail(-71, "circuit: too many draw sites, records or faults");
        c.ops.push_back(r);
    }
    c.M = (int32_t)rec;
    c.n_sites = (uint32_t)site, c.n_rsites = (uint32_t)rsite, c.n_faults = (int32_t)fault;
    c.lds_bytes = 16 * (size_t)c.Q + 8 * (size_t)c.M;
    // output groups: rows of record parities
    c.n_groups = n_groups;
    int64_t total = 0;
    for (int g = 0; g < kFrameGroups; ++g) {
        c.rows[g] = c.row_off[g] = 0;
        if (g >= n_groups) continue;
        if (group_rows[g] < 0) throw Fail(-71, "circuit: negative row count of an output group");
        c.rows[g] = group_rows[g];
        c.row_off[g] = (int32_t)total;
        total += group_rows[g];
        if (total >= (1ll << 30)) throw Fail(-71, "circuit: too many output rows");
    }
    c.row_ptr.assign(1, 0);
    c.rec_idx.clear();
    if (n_groups) {
        if (row_ptr[0] != 0) throw Fail(-71, "circuit: row_ptr[0] must be 0");
        for (int64_t r = 0; r < total; ++r)
            if (row_ptr[r + 1] < row_ptr[r]) throw Fail(-71, "circuit: row_ptr not monotone");
        const int32_t nnz = row_ptr[total];
        if (nnz && !rec_idx) throw Fail(-71, "circuit: null program array");
        for (int32_t e = 0; e < nnz; ++e)
            if (rec_idx[e] < 0 || rec_idx[e] >= c.M)
                throw Fail(-73, "circuit: record reference outside [0, measurements): entry " + std::to_string(e) +
                                    " = " + std::to_string(rec_idx[e]));
        c.row_ptr.assign(row_ptr, row_ptr + total + 1);
        c.rec_idx.assign(rec_idx, rec_idx + nnz);
    }
    if (c.lds_bytes > kFrameLdsLimit && !beyond_lds)
        throw Fail(-76, "circuit: " + std::to_string(c.lds_bytes) + " B of LDS (16 B per qubit, 8 B per measurement) "
                            "exceed the kernel's " + std::to_string(kFrameLdsLimit));
}

void circuit_fault_table(const HostCircuit& c, int kind, int32_t* op, int32_t* target, int32_t* comp) {
    if (kind != 0 && kind != 1) throw Fail(-87, "circuit faults: kind must be 0 (noise) or 1 (gauge)");
    if (fault_total(c, kind) && (!op || !target || !comp)) throw Fail(-71, "circuit: null fault table array");
    int64_t f = 0;
    for (size_t i = 0; i < c.ops.size(); ++i) {
        const FrameOpRec& r = c.ops[i];
        const int32_t cnt = fault_count(r.op, r.tgt_cnt, kind);
        for (int32_t j = 0; j < cnt; ++j, ++f) {
            op[f] = (int32_t)i;
            target[f] = r.tgt_off + fault_target(r.op, j, kind);
            comp[f] = fault_comp(r.op, j, kind);
        }
    }
}

}  // namespace qdec
