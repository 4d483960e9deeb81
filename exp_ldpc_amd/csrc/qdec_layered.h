// qdec_layered.h -- layered (check-serial) min-sum BP (qdec_layered.hip; DESIGN
// 3.6f has the spec): its launch arguments, the LDS and slot layouts of both
// placements, the placement rule and the rule of its slot scratch.  Pure host
// code with no HIP header, so the ABI unit, the kernel unit and the stand-alone
// checker (tools/layered_scratch_check.cpp) read the same limits and the same
// rule.
#pragma once
#include "qdec_scratch.h"

namespace qdec {

// workgroups per CU by default, from the sweeps of DESIGN 3.6f: with P and R in
// LDS (at most what a CU's LDS holds) and with them in HBM; and the workgroups
// that must fit a CU's LDS for QD_LAYERED_AUTO to take LDS
constexpr int kLayeredLdsPerCu = 16;
constexpr int kLayeredSlotsPerCu = 8;
constexpr int kLayeredAutoFit = 8;
constexpr size_t kLayeredLdsMax = 160 * 1024;
constexpr int64_t kLayeredMaxSlots = 1ll << 20;

// qd_layered_params of include/qdec.h, field for field
struct LayeredParams {
    int32_t max_iter;
    double ms_scaling, clip;
};

struct LayeredArgs {
    int64_t B;
    int max_iter, syn_flags;
    double ms_scaling, clip;
    const uint8_t* syn;      // [B][m] (nullable with syn_flags)
    const uint8_t* base;     // [B][n_data] nullable
    const uint8_t* readout;  // [B][n_data] nullable
    uint8_t* x_out;          // [B][n] nullable
    uint8_t* corr_out;       // [B][n_data] nullable
    void* llr_out;           // [B][n] float / double, nullable
    int32_t* iters;          // [B] nullable
    uint8_t* status;         // [B] nullable
    uint8_t* fail;           // [B] nullable
    unsigned long long* work_ctr;  // the launch's shot counter, zeroed before it
};

// Byte offsets.  LDS: the control area (kCtrl of qdec_graph.h), the syndrome as
// bytes, the hard decision as bits (the parity test reads them) and as bytes
// (finalize_shot reads those); with the beliefs in LDS they follow at l_msg.
// The belief region (LDS, or one slot of the scratch): P[n], then R[E] by CSR
// edge.
struct LayeredLayout {
    int64_t l_sb, l_xb, l_xh, l_msg, lds_small;
    int64_t o_R, msg_bytes, slot_bytes;
    LayeredLayout() = default;
    LayeredLayout(const DevGraph& g, int64_t tsz) {
        auto r16 = [](int64_t b) { return (b + 15) / 16 * 16; };
        l_sb = kCtrl;
        l_xb = l_sb + g.m_pad;
        l_xh = l_xb + (int64_t)g.n_pad / 8;
        l_msg = lds_small = r16(l_xh + g.n_pad);
        o_R = (int64_t)g.n * tsz;
        msg_bytes = ((int64_t)g.E + g.n) * tsz;
        slot_bytes = (msg_bytes + 255) / 256 * 256;
    }
    int64_t lds_bytes(bool hbm) const { return hbm ? lds_small : lds_small + (msg_bytes + 15) / 16 * 16; }
};

// Which placement runs a graph: placement 0 LDS, 1 HBM, 2 LDS while
// kLayeredAutoFit workgroups fit a CU's LDS, else HBM (QD_LAYERED_* of qdec.h,
// checked by the caller).  -1: none holds it.
inline int layered_place(const LayeredLayout& L, int placement) {
    const size_t lds = (size_t)L.lds_bytes(false), small = (size_t)L.lds_bytes(true);
    if (placement == 0) return lds <= kLayeredLdsMax ? 0 : -1;
    if (placement == 2 && lds * kLayeredAutoFit <= kLayeredLdsMax) return 0;
    return small <= kLayeredLdsMax ? 1 : -1;
}

// workgroups per CU of an LDS launch by default: what a CU's LDS holds, at most kLayeredLdsPerCu
inline int64_t layered_lds_per_cu(const LayeredLayout& L) {
    return std::max<int64_t>(1, std::min<int64_t>(kLayeredLdsPerCu, (int64_t)kLayeredLdsMax / L.lds_bytes(false)));
}

// The slot scratch of the HBM placement: the relay rule's policy (a grow stays
// within a quarter of the free device memory, a refusal halves down to one slot).
inline SlotRule layered_slot_rule(size_t slot_bytes, int64_t dflt) {
    return {slot_bytes, dflt, -112, "no memory for one layered-BP slot of ", -113, "one layered-BP slot of ",
            "hipMalloc layered scratch", "hipFree layered scratch"};
}

// Parameter checks of the decode entry points (-49)
inline void layered_check_params(const LayeredParams* p) {
    if (!p) throw Fail(-49, "null layered parameters");
    if (p->max_iter < 1) throw Fail(-49, "layered max_iter must be >= 1");
    if (!std::isfinite(p->ms_scaling) || p->ms_scaling < 0.0)
        throw Fail(-49, "layered ms_scaling must be finite and >= 0 (0: the 1 - 2^-t schedule)");
    if (!std::isfinite(p->clip) || !(p->clip > 0.0)) throw Fail(-49, "layered clip must be finite and > 0");
}

}  // namespace qdec
