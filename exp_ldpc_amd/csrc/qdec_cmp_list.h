// qdec_cmp_list.h -- the compact shot list between ms_triage_kernel
// (qdec_ms_triage.hip, the writer) and bp_ms_cmp_kernel (qdec_bp_ms.h, the
// reader); the segment counts kCmpSegs / kCmpLists are in qdec_graph.h.
#pragma once
#include "qdec_device.h"

namespace qdec {

// ---------------------------------------------------------------- compact shot list
// Lean min-sum launches on wave graphs run in two passes.  ms_triage_kernel
// streams every shot's syndrome and readout rows once (coalesced tiles of 64
// shots), packs the syndrome into bit words and reduces the readout to its
// logical parities (bit r = parity of Lz[r] . readout).  A shot with an
// all-zero syndrome under all-positive priors converges in iteration 1 with
// x = 0 (every message >= 0, so every posterior >= its prior > 0: the same
// shortcut the one-pass kernel takes), so its outputs are written right there
// (iterations 1, status 3, no SSF steps, failure = any readout parity).  Every
// other shot is appended to a compact list: shot index, syndrome words,
// readout-parity words.  bp_ms_cmp_kernel then decodes only the listed shots,
// reading each as one entry from registers (no row staging, no readout): its
// failure check is the parity of Lz (in lane-slot order, ms_lzs) against the
// ballot words of the hard decision, XOR the readout parities, and a
// BP-failed shot enters the SSF queue with the parities in place of the
// readout words (q_rpar), which the SSF kernel's check uses the same way.
template <int RC>
struct CmpEntry {
    static constexpr int EW = 1 + RC + kMaxLogicalRounds;  // shot, syndrome words, readout-parity words
    static constexpr int kPer = 4;                          // entries per chunk (one u64 load per lane)
    static_assert(kPer * EW <= 64, "chunk");
};

constexpr int kHeavyW = 6;  // listed shots of larger syndrome weight go to the heavy list

}  // namespace qdec
