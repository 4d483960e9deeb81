// qdec_abi_circuit.cpp -- the extern "C" entry points of compiled circuits
// (qd_circuit_*, include/qdec.h): a validated Pauli-frame program
// (qdec_circuit.h) and, unless host-only, its copy on one device.  No C++
// exception crosses the ABI.
#include "qdec_abi.h"

using namespace qdec;

struct qd_circuit {
    HostCircuit hc;
    DevCircuit dc{};
    bool host_only = true;
    int device = 0;
    int num_cus = 0;
    DeviceSink arena;
    // where the kernels keep the frame: FP_LDS or FP_HBM (FP_AUTO is resolved at create)
    int32_t placement = FP_LDS;
    // HBM placement: the handle's slot scratch (slots_cfg: qd_circuit_set_frame_slots)
    ChainedSlots fws;
};

namespace {

int create_circuit(int32_t placement, bool host_only, int32_t device, int32_t num_qubits, int32_t n_ops,
                   const int32_t* ops, int32_t n_targets, const int32_t* targets, const double* probs,
                   int32_t n_groups, const int32_t* group_rows, const int32_t* row_ptr, const int32_t* rec_idx,
                   qd_circuit** out, int32_t n_args = -1, const double* args = nullptr) {
    return guarded([&] {
        if (!out) throw Fail(-71, "circuit: null output handle");
        *out = nullptr;
        if (placement != FP_LDS && placement != FP_HBM && placement != FP_AUTO)
            throw Fail(-96, "circuit: unknown frame placement (0 LDS, 1 HBM, 2 auto)");
        std::unique_ptr<qd_circuit> C(new qd_circuit());
        build_circuit(C->hc, num_qubits, n_ops, ops, n_targets, targets, probs, n_groups, group_rows, row_ptr,
                      rec_idx, placement != FP_LDS, n_args, args);
        C->placement = placement == FP_AUTO ? (C->hc.lds_bytes > kFrameLdsLimit ? FP_HBM : FP_LDS) : placement;
        C->host_only = host_only;
        const HostCircuit& h = C->hc;
        DevCircuit& d = C->dc;
        d.Q = h.Q, d.M = h.M, d.n_ops = (int32_t)h.ops.size();
        for (int g = 0; g < kFrameGroups; ++g) d.rows[g] = h.rows[g], d.row_off[g] = h.row_off[g];
        if (!host_only) {
            int ndev = 0;
            hip_check(hipGetDeviceCount(&ndev), "hipGetDeviceCount");
            if (device < 0 || device >= ndev) throw Fail(-15, "device ordinal out of range");
            C->device = device;
            hip_check(hipSetDevice(device), "hipSetDevice");
            hipDeviceProp_t prop;
            hip_check(hipGetDeviceProperties(&prop, device), "hipGetDeviceProperties");
            C->num_cus = prop.multiProcessorCount;
            d.ops = static_cast<const FrameOpRec*>(C->arena.put(h.ops.data(), h.ops.size() * sizeof(FrameOpRec)));
            d.targets = static_cast<const int32_t*>(C->arena.put(h.targets.data(), h.targets.size() * 4));
            d.cum = static_cast<const uint32_t*>(C->arena.put(h.cum.data(), h.cum.size() * 4));
            d.row_ptr = static_cast<const int32_t*>(C->arena.put(h.row_ptr.data(), h.row_ptr.size() * 4));
            d.rec_idx = static_cast<const int32_t*>(C->arena.put(h.rec_idx.data(), h.rec_idx.size() * 4));
        }
        *out = C.release();
    });
}

// The output list of a sampler / fault call (`what`) against the handle: -77 for
// a null list or a group the circuit lacks, -78 for a misaligned packed row.
// Copies the pointers to o; true when flags ask for packed rows (the callers
// refuse unknown flags where their own order of checks has it).
bool frame_outs(const qd_circuit* C, const char* what, int32_t flags, void* const outs[4], void* (&o)[kFrameGroups]) {
    if (!outs) throw Fail(-77, std::string("invalid circuit ") + what + " arguments: null output list");
    const bool packed = (flags & QD_INPUT_PACKED) != 0;
    for (int g = 0; g < kFrameGroups; ++g) {
        o[g] = outs[g];
        if (o[g] && g >= C->hc.n_groups) throw Fail(-77, "output buffer for a group the circuit does not have");
        if (packed && ((uintptr_t)o[g] & 7)) throw Fail(-78, "packed rows must be 8-B aligned");
    }
    return packed;
}

// One launch over `words` 64-shot (64-fault) words on the handle's placement: in
// HBM between the acquire and the release of its slot scratch.  -102 with the
// caller's wording (`what`) when launch(place) does not return 0.
template <class Launch>
void frame_launch(qd_circuit* C, const char* what, int64_t words, hipStream_t stream, Launch&& launch) {
    hip_check(hipSetDevice(C->device), "hipSetDevice");
    const bool hbm = C->placement == FP_HBM;
    FramePlace at;
    at.placement = C->placement, at.lds = at.slot_bytes = C->hc.lds_bytes, at.num_cus = C->num_cus;
    if (hbm) {  // a slot holds one frame; on a refusal the slots are halved down to one, then -97
        const SlotRule rule{C->hc.lds_bytes, (int64_t)C->num_cus * kFrameHbmSlotsPerCu, -97,
                            "circuit: no memory for one frame slot of ", 0, nullptr,
                            "hipMalloc frame scratch", "hipFree frame scratch"};
        at.slots = C->fws.acquire(rule, words, stream), at.scratch = C->fws.ptr;
    }
    const int rc = launch(at);
    if (hbm) C->fws.release(at.slots, stream);
    if (rc != 0) throw Fail(-102, std::string(what) + " launch failed: " + hipGetErrorString((hipError_t)rc));
}

}  // namespace

extern "C" {

int qd_circuit_create(int32_t device, int32_t num_qubits, int32_t n_ops, const int32_t* ops, int32_t n_targets,
                      const int32_t* targets, const double* probs, int32_t n_groups, const int32_t* group_rows,
                      const int32_t* row_ptr, const int32_t* rec_idx, qd_circuit** out) {
    return create_circuit(FP_LDS, false, device, num_qubits, n_ops, ops, n_targets, targets, probs, n_groups,
                          group_rows, row_ptr, rec_idx, out);
}

int qd_circuit_create_host(int32_t num_qubits, int32_t n_ops, const int32_t* ops, int32_t n_targets,
                           const int32_t* targets, const double* probs, int32_t n_groups, const int32_t* group_rows,
                           const int32_t* row_ptr, const int32_t* rec_idx, qd_circuit** out) {
    return create_circuit(FP_LDS, true, 0, num_qubits, n_ops, ops, n_targets, targets, probs, n_groups, group_rows,
                          row_ptr, rec_idx, out);
}

int qd_circuit_create_placed(int32_t placement, int32_t device, int32_t num_qubits, int32_t n_ops,
                             const int32_t* ops, int32_t n_targets, const int32_t* targets, const double* probs,
                             int32_t n_groups, const int32_t* group_rows, const int32_t* row_ptr,
                             const int32_t* rec_idx, qd_circuit** out) {
    return create_circuit(placement, false, device, num_qubits, n_ops, ops, n_targets, targets, probs, n_groups,
                          group_rows, row_ptr, rec_idx, out);
}

int qd_circuit_create_host_placed(int32_t placement, int32_t num_qubits, int32_t n_ops, const int32_t* ops,
                                  int32_t n_targets, const int32_t* targets, const double* probs, int32_t n_groups,
                                  const int32_t* group_rows, const int32_t* row_ptr, const int32_t* rec_idx,
                                  qd_circuit** out) {
    return create_circuit(placement, true, 0, num_qubits, n_ops, ops, n_targets, targets, probs, n_groups,
                          group_rows, row_ptr, rec_idx, out);
}

int qd_circuit_create_args(int32_t placement, int32_t device, int32_t num_qubits, int32_t n_ops, const int32_t* ops,
                           int32_t n_targets, const int32_t* targets, const double* probs, int32_t n_groups,
                           const int32_t* group_rows, const int32_t* row_ptr, const int32_t* rec_idx, int32_t n_args,
                           const double* args, qd_circuit** out) {
    if (n_args < 0) return guarded([] { throw Fail(-71, "circuit: negative argument count"); });
    return create_circuit(placement, false, device, num_qubits, n_ops, ops, n_targets, targets, probs, n_groups,
                          group_rows, row_ptr, rec_idx, out, n_args, args);
}

int qd_circuit_create_host_args(int32_t placement, int32_t num_qubits, int32_t n_ops, const int32_t* ops,
                                int32_t n_targets, const int32_t* targets, const double* probs, int32_t n_groups,
                                const int32_t* group_rows, const int32_t* row_ptr, const int32_t* rec_idx,
                                int32_t n_args, const double* args, qd_circuit** out) {
    if (n_args < 0) return guarded([] { throw Fail(-71, "circuit: negative argument count"); });
    return create_circuit(placement, true, 0, num_qubits, n_ops, ops, n_targets, targets, probs, n_groups,
                          group_rows, row_ptr, rec_idx, out, n_args, args);
}

int qd_circuit_set_frame_slots(qd_circuit* C, int64_t slots) {
    return guarded([&] {
        if (!C) throw Fail(-71, "circuit: null handle");
        if (slots < 0 || slots > (1ll << 20)) throw Fail(-98, "circuit: frame slots must be 0 (default) .. 2^20");
        C->fws.slots_cfg = slots;
    });
}

int qd_circuit_frame_info(const qd_circuit* C, int64_t out[4]) {
    return guarded([&] {
        if (!C || !out) throw Fail(-71, "circuit: null handle or output");
        out[0] = C->placement, out[1] = (int64_t)C->hc.lds_bytes, out[2] = C->fws.slots_last;
        out[3] = (int64_t)C->fws.bytes;
    });
}

int qd_circuit_op_flags_copy(const qd_circuit* C, int32_t* dup) {
    return guarded([&] {
        if (!C || (!dup && !C->hc.ops.empty())) throw Fail(-71, "circuit: null handle or output");
        for (size_t i = 0; i < C->hc.ops.size(); ++i) dup[i] = C->hc.ops[i].dup;
    });
}

int qd_circuit_destroy(qd_circuit* C) {
    return guarded([&] {
        if (!C) return;
        if (!C->host_only) (void)hipSetDevice(C->device);
        C->fws.destroy();
        delete C;  // its sink frees the uploads
    });
}

int qd_circuit_info(const qd_circuit* C, int64_t out[10]) {
    return guarded([&] {
        if (!C || !out) throw Fail(-71, "circuit: null handle or output");
        const HostCircuit& h = C->hc;
        out[0] = h.Q, out[1] = h.M;
        for (int g = 0; g < kFrameGroups; ++g) out[2 + g] = h.rows[g];
        out[6] = (int64_t)h.lds_bytes, out[7] = (int64_t)h.ops.size(), out[8] = h.n_sites, out[9] = h.n_rsites;
    });
}

int qd_circuit_sample_device(qd_circuit* C, uint32_t seed, uint32_t stream_id, int64_t shot0, int64_t B,
                             int32_t flags, void* const outs[4], void* stream) {
    return guarded([&] {
        if (!C) throw Fail(-71, "circuit: null handle");
        if (C->host_only) throw Fail(-79, "host-only circuit (qd_circuit_create_host): no device to sample on");
        if (B < 0 || (flags & ~QD_INPUT_PACKED)) throw Fail(-77, "invalid circuit sampler arguments");
        if (B == 0) return;
        void* o[kFrameGroups];
        const bool packed = frame_outs(C, "sampler", flags, outs, o);
        frame_launch(C, "sampler", (B + 63) / 64, (hipStream_t)stream, [&](const FramePlace& at) {
            return launch_frame_sample(C->dc, at, seed, stream_id, shot0, B, packed, o, (hipStream_t)stream);
        });
    });
}

int qd_circuit_fault_info(const qd_circuit* C, int64_t out[4]) {
    return guarded([&] {
        if (!C || !out) throw Fail(-71, "circuit: null handle or output");
        out[0] = fault_total(C->hc, 0), out[1] = fault_total(C->hc, 1), out[2] = out[3] = 0;
    });
}

int qd_circuit_fault_table(const qd_circuit* C, int32_t kind, int32_t* op, int32_t* target, int32_t* comp) {
    return guarded([&] {
        if (!C) throw Fail(-71, "circuit: null handle");
        circuit_fault_table(C->hc, kind, op, target, comp);
    });
}

int qd_circuit_faults_device(qd_circuit* C, int32_t kind, int64_t f0, int64_t F, int32_t flags, void* const outs[4],
                             void* stream) {
    return guarded([&] {
        if (!C) throw Fail(-71, "circuit: null handle");
        if (kind != 0 && kind != 1) throw Fail(-87, "circuit faults: kind must be 0 (noise) or 1 (gauge)");
        if (f0 < 0 || F < 0) throw Fail(-88, "circuit faults: negative first fault or count");
        if (F > (int64_t)fault_total(C->hc, kind) - f0)
            throw Fail(-89, "circuit faults: window beyond the circuit's " +
                                std::to_string(fault_total(C->hc, kind)) + " faults of this kind");
        if (flags & ~QD_INPUT_PACKED) throw Fail(-77, "invalid circuit fault arguments: unknown flags");
        if (C->host_only) throw Fail(-79, "host-only circuit (qd_circuit_create_host): no device to propagate on");
        if (F == 0) return;
        void* o[kFrameGroups];
        const bool packed = frame_outs(C, "fault", flags, outs, o);
        frame_launch(C, "fault", (F + 63) / 64, (hipStream_t)stream, [&](const FramePlace& at) {
            return launch_frame_faults(C->dc, at, kind, (int32_t)f0, (int32_t)F, packed, o, (hipStream_t)stream);
        });
    });
}

}  // extern "C"
