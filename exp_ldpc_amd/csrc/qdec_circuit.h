// qdec_circuit.h -- the compiled Pauli-frame program of qd_circuit_* (HIP-free):
// what the host hands over, what the validator makes of it, and what the kernel
// (qdec_frame.hip) reads.  The conventions are DESIGN §3.4c.
#ifndef QDEC_CIRCUIT_H
#define QDEC_CIRCUIT_H
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace qdec {

// opcodes of the program (exp_ldpc_amd/circuit.py OP_*)
enum FrameOp : int32_t {
    FO_H = 0, FO_CX, FO_CZ, FO_R, FO_RX, FO_M, FO_MX, FO_XERR, FO_YERR, FO_ZERR, FO_DEP1, FO_DEP2,
    FO_PC1, FO_PC2,  // PAULI_CHANNEL_1 / 2: one probability per Pauli (pair), see FrameOpRec::cum_off
    FO_COUNT
};
constexpr int kFrameGroups = 4;                    // output groups of one program
constexpr size_t kFrameLdsLimit = 160 * 1024;      // the launch's dynamic LDS
constexpr int32_t kFrameInvert = 1 << 30;          // measurement target bit: record inverted
constexpr int32_t kFrameQubitMask = kFrameInvert - 1;
// where a handle's kernels keep the frame (include/qdec.h QD_FRAME_*)
enum FramePlacement : int32_t { FP_LDS = 0, FP_HBM = 1, FP_AUTO = 2 };

// One instruction as the kernel reads it.  site0: its first Bernoulli / Pauli
// draw site (a multiple of 4: one Philox block serves four sites); rsite0: its
// first randomisation site, which is also its first gauge fault; rec0: the record
// index of its first target; fault0: its first noise fault (fault_count below);
// dup: 1 when a noise instruction names a qubit more than once (X_ERROR 0 1 0, a
// qubit in two DEPOLARIZE2 pairs), so two sites of it may name one frame word;
// cum_off: PAULI_CHANNEL_1 / 2 only, the instruction's first entry in the table of
// cumulative thresholds C_0 .. C_{K-1} (K = 3 / 15; thr = C_{K-1}), else 0.
struct FrameOpRec {
    int32_t op, tgt_off, tgt_cnt;
    uint32_t thr, site0, rsite0;
    int32_t rec0, fault0;
    int32_t dup;
    int32_t cum_off;
};
// arguments of a noise instruction that carries one probability per outcome
constexpr int32_t channel_args(int32_t op) { return op == FO_PC1 ? 3 : op == FO_PC2 ? 15 : 0; }
// noise on pairs of targets (one draw site per pair) / with an X and a Z fault per target
constexpr bool pair_noise(int32_t op) { return op == FO_DEP2 || op == FO_PC2; }
constexpr bool pauli_noise(int32_t op) { return op == FO_DEP1 || op == FO_DEP2 || op == FO_PC1 || op == FO_PC2; }

// Elementary faults of one instruction with cnt targets (include/qdec.h): noise
// faults (kind 0) of X/Y/Z_ERROR and M / MX one per target, of DEPOLARIZE1 / 2 and
// PAULI_CHANNEL_1 / 2 an X and a Z per target; gauge faults (kind 1) one per target of R, RX, M, MX.
constexpr int32_t fault_count(int32_t op, int32_t cnt, int kind) {
    return kind ? (op == FO_R || op == FO_RX || op == FO_M || op == FO_MX ? cnt : 0)
           : pauli_noise(op)                                ? 2 * cnt
           : op == FO_M || op == FO_MX || op >= FO_XERR     ? cnt
                                                            : 0;
}
// components of a fault (qd_circuit_fault_table)
enum FaultComp : int32_t { FC_X = 1, FC_Z = 2, FC_Y = 3, FC_REC = 4 };
// The component of fault j of an instruction: the Pauli channels alternate X, Z along
// the target list; a gauge fault is the component the sampler randomises there.
constexpr int32_t fault_comp(int32_t op, int32_t j, int kind) {
    return kind ? (op == FO_RX || op == FO_MX ? FC_X : FC_Z)
           : op == FO_M || op == FO_MX         ? FC_REC
           : op == FO_XERR                     ? FC_X
           : op == FO_ZERR                     ? FC_Z
           : op == FO_YERR                     ? FC_Y
                                               : ((j & 1) ? FC_Z : FC_X);
}
// ... and the index into the instruction's targets it acts on
constexpr int32_t fault_target(int32_t op, int32_t j, int kind) {
    return !kind && pauli_noise(op) ? j >> 1 : j;
}

struct HostCircuit {
    int32_t Q = 0, M = 0;
    std::vector<FrameOpRec> ops;
    std::vector<int32_t> targets;
    std::vector<uint32_t> cum;                     // cumulative thresholds of the PAULI_CHANNEL instructions
    int32_t n_groups = 0;
    int32_t rows[kFrameGroups] = {0, 0, 0, 0};     // rows of each group
    int32_t row_off[kFrameGroups] = {0, 0, 0, 0};  // its first row in row_ptr
    std::vector<int32_t> row_ptr, rec_idx;         // CSR over record indices, groups concatenated
    uint32_t n_sites = 0, n_rsites = 0;
    int32_t n_faults = 0;                          // noise faults; the gauge faults are n_rsites
    size_t lds_bytes = 0;                          // 16 Q + 8 M
};

// The program on the device (or, host-only, nothing): pointers into the handle's
// uploads.
struct DevCircuit {
    int32_t Q, M, n_ops;
    const FrameOpRec* ops;
    const int32_t* targets;
    const uint32_t* cum;
    const int32_t* row_ptr;
    const int32_t* rec_idx;
    int32_t rows[kFrameGroups], row_off[kFrameGroups];
};

// Validates every index of a program and derives the records, sites and the
// LDS need (throws Fail with the ABI's code; include/qdec.h qd_circuit_create).
// ops: [n_ops][4] = opcode, first target, target count, first argument
// (PAULI_CHANNEL_1 / 2: its 3 / 15 probabilities args[ops[4 i + 3] ..], 0 for every
// other opcode); probs: [n_ops], of a PAULI_CHANNEL the sum of its arguments.
// n_args < 0: an entry point without an argument array, which refuses the
// PAULI_CHANNEL opcodes (-71).  beyond_lds: a program over kFrameLdsLimit passes
// (its frame goes to HBM); otherwise it is refused with -76.
void build_circuit(HostCircuit& c, int32_t num_qubits, int32_t n_ops, const int32_t* ops, int32_t n_targets,
                   const int32_t* targets, const double* probs, int32_t n_groups, const int32_t* group_rows,
                   const int32_t* row_ptr, const int32_t* rec_idx, bool beyond_lds = false, int32_t n_args = -1,
                   const double* args = nullptr);

// The faults of one kind, in their numbering: the instruction, the index into
// `targets` and the component (FaultComp) of each; arrays of fault_total entries.
inline int32_t fault_total(const HostCircuit& c, int kind) { return kind ? (int32_t)c.n_rsites : c.n_faults; }
void circuit_fault_table(const HostCircuit& c, int kind, int32_t* op, int32_t* target, int32_t* comp);

}  // namespace qdec
#endif
