// qdec_relay.h -- the relay-BP stage (qdec_relay.hip; DESIGN 3.6d has the spec):
// its per-graph tables, launch arguments, the LDS and slot layouts of both
// placements, and the rule of its slot scratch.  Pure host code with no HIP
// header, so the ABI unit, the kernel unit and the stand-alone checker
// (tools/relay_scratch_check.cpp) read the same limits and the same rule.
#pragma once
#include "qdec_scratch.h"

namespace qdec {

constexpr int64_t kRelayMaxTable = 1ll << 23;  // (num_sets + 1) * n entries of the memory-strength table
constexpr int kRelayFixBits = 16;              // solution weights: llrint(prior * 2^16)
constexpr int kRelaySlotsPerCu = 2;            // workgroups per CU with the messages in HBM, by default
constexpr int kRelayLdsPerCu = 8;              // at most this many per CU with the messages in LDS
constexpr size_t kRelayLdsMax = 160 * 1024;
constexpr int64_t kRelayMaxSlots = 1ll << 20;

// qd_relay_params of include/qdec.h, field for field
struct RelayParams {
    double gamma0, alpha, clip;
    int32_t pre_iter, num_sets, set_max_iter, stop_nconv;
};

// What the kernel reads beside the graph: leg r's memory strengths at
// gamma[precision] + r * n (row 0 holds gamma0 throughout), the fixed-point
// solution weights, and the schedule.
struct RelayTables {
    const void* gamma[2];  // [QD_F64], [QD_F32]: [(num_sets + 1)][n]
    const long long* w;    // [n]
    int pre_iter, num_sets, set_max_iter, stop_nconv;
    double alpha, clip;
};

// Shots whose status has QD_ST_BP_CONVERGED set are skipped when only_failed is
// set; none of their outputs is touched.
struct RelayArgs {
    int64_t B;
    int syn_flags, only_failed;
    const uint8_t* syn;      // [B][m] (nullable with syn_flags)
    const uint8_t* base;     // [B][n_data] nullable
    const uint8_t* readout;  // [B][n_data] nullable
    uint8_t* x_out;          // [B][n] nullable
    uint8_t* corr_out;       // [B][n_data] nullable
    void* llr_out;           // [B][n] float / double, nullable
    int32_t* iters;          // [B] nullable
    int32_t* legs;           // [B] nullable
    uint8_t* status;         // [B] nullable; read first with only_failed
    uint8_t* fail;           // [B] nullable
    unsigned long long* work_ctr;  // the launch's shot counter, zeroed before it
};

// Byte offsets.  LDS: the control area (kCtrl of qdec_graph.h), the hard
// decision and the syndrome as bytes, the best solution as bits; with the
// messages in LDS they follow at l_msg.  The message region (LDS, or one slot
// of the scratch): v2c[E], c2v[E] by CSR edge, then the marginals M[n].
struct RelayLayout {
    int64_t l_xh, l_sb, l_best, l_msg, lds_small;
    int64_t o_c2v, o_M, msg_bytes, slot_bytes;
    RelayLayout() = default;
    RelayLayout(const DevGraph& g, int64_t tsz) {
        auto r16 = [](int64_t b) { return (b + 15) / 16 * 16; };
        l_xh = kCtrl;
        l_sb = l_xh + g.n_pad;
        l_best = l_sb + g.m_pad;
        l_msg = lds_small = r16(l_best + (int64_t)g.n_pad / 8);
        o_c2v = r16((int64_t)g.E * tsz);
        o_M = 2 * o_c2v;
        msg_bytes = o_M + r16((int64_t)g.n * tsz);
        slot_bytes = (msg_bytes + 255) / 256 * 256;
    }
    int64_t lds_bytes(bool hbm) const { return hbm ? lds_small : lds_small + msg_bytes; }
};

// Which placement runs a graph: placement 0 LDS, 1 HBM, 2 LDS where it fits,
// else HBM (QD_RELAY_* of qdec.h, checked by the caller).  -1: none holds it.
inline int relay_place(const RelayLayout& L, int placement) {
    if (placement != 1 && (size_t)L.lds_bytes(false) <= kRelayLdsMax) return 0;
    if (placement != 0 && (size_t)L.lds_bytes(true) <= kRelayLdsMax) return 1;
    return -1;
}

// The slot scratch of the HBM placement: as the OSD scratch, with the budget rule.
inline SlotRule relay_slot_rule(size_t slot_bytes, int64_t dflt) {
    return {slot_bytes, dflt, -58, "no memory for one relay slot of ", -59, "one relay slot of ",
            "hipMalloc relay scratch", "hipFree relay scratch"};
}

// Parameter checks of qd_graph_set_relay (-52, -53) and the tables in host
// memory: the strengths in both precisions, rounded once, and the weights from
// the f64 min-sum priors.
inline void relay_check_params(const RelayParams* p, const double* gammas, int n) {
    if (!p) throw Fail(-52, "null relay parameters");
    if (!(p->alpha > 0.0) || !std::isfinite(p->alpha)) throw Fail(-52, "relay alpha must be a finite number > 0");
    if (!(p->clip > 0.0)) throw Fail(-52, "relay clip must be > 0");
    if (!std::isfinite(p->gamma0)) throw Fail(-52, "relay gamma0 must be finite");
    if (p->pre_iter < 1 || p->set_max_iter < 1 || p->stop_nconv < 1 || p->num_sets < 0)
        throw Fail(-52, "relay needs pre_iter, set_max_iter, stop_nconv >= 1 and num_sets >= 0");
    if (((int64_t)p->num_sets + 1) * n > kRelayMaxTable)
        throw Fail(-53, "relay table above 2^23 entries ((num_sets + 1) * n)");
    if (p->num_sets > 0 && !gammas) throw Fail(-52, "null relay gammas with num_sets > 0");
    for (int64_t e = 0; e < (int64_t)p->num_sets * n; ++e)
        if (!std::isfinite(gammas[e])) throw Fail(-52, "relay gammas must be finite");
}

struct RelayHostTables {
    std::vector<double> g64;
    std::vector<float> g32;
    std::vector<long long> w;
};
inline RelayHostTables relay_build_tables(const RelayParams& p, const double* gammas, int n, const double* prior64) {
    RelayHostTables t;
    const size_t rows = (size_t)p.num_sets + 1;
    t.g64.assign(rows * n, p.gamma0);
    if (p.num_sets > 0) std::copy(gammas, gammas + (size_t)p.num_sets * n, t.g64.begin() + n);
    t.g32.resize(t.g64.size());
    for (size_t e = 0; e < t.g64.size(); ++e) t.g32[e] = (float)t.g64[e];
    t.w.resize(n);
    for (int j = 0; j < n; ++j) t.w[j] = std::llrint(std::ldexp(prior64[j], kRelayFixBits));
    return t;
}

}  // namespace qdec
