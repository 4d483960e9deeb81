// qdec_osd_steps.h -- the pieces of the OSD stage that more than one of its
// device kernels uses (osd_wave_kernel, osd_block_kernel: qdec_osd.hip;
// osd_hbm_kernel: qdec_osd_hbm.hip).  The spec is steps 1-6 at the top of
// qdec_osd.hip.  Of the tie rules that keep the kernels bit-identical to the host
// stage (qdec_osd.cpp), two are in here, once: the column index breaks a sort
// tie (bitonic_exchange), and pairs go in lexicographic order (pair_of).  The
// third, the order of the candidates in a key (OSD-0, singles, pairs; osd_key),
// is applied by each kernel's own search.
//
// Device code only (plus the two layout helpers, which the host evaluates too).
// A step takes the thread's index t among the nt threads that share the shot
// (lane, 64 or tid, 256) and, where it touches index arrays, their type Idx
// (uint16_t on chip, uint32_t for the rows in HBM).  What stays in each kernel:
// where the rows live, the elimination, the HBM kernel's chunked sort driver,
// and steps 5 and 6 (the candidate search, the pick and the outputs).  The two
// workgroup kernels took those from here at first; each was measurably slower
// than with its own text, so they are written out in both.
#pragma once
#include <hip/hip_runtime.h>

#include "qdec_device.h"
#include "qdec_internal.h"

namespace qdec {

constexpr int kOsdMaxLam = 64;  // pair / exhaustive search width kept in LDS

// ---- layouts: the sort's padded size, and regions rounded up to 16 bytes
template <typename I>
__host__ __device__ inline I osd_sort_size(I n) {
    I ns = 64;
    while (ns < n) ns <<= 1;
    return ns;
}

template <typename I>
struct OsdTake {
    I o = 0;
    __host__ __device__ I operator()(I bytes) {
        const I at = o;
        o += (bytes + 15) / 16 * 16;
        return at;
    }
};

// ---- 1. stable sort of the columns by log-probability ratio
// Ascending doubles -> ascending unsigned keys (-0.0 folded onto +0.0, as the
// host's `<` comparison treats them as equal).
__device__ __forceinline__ uint64_t order_key(double v) {
    uint64_t b = (uint64_t)__double_as_longlong(v);
    if (b == 0x8000000000000000ull) b = 0;
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// (key, column) of the shot's n columns; the padding up to NS sorts behind them
template <typename Idx>
__device__ __forceinline__ void osd_fill_keys(const OsdArgs& a, int64_t shot, int n, int NS, uint64_t* key, Idx* idx,
                                              int t, int nt) {
    for (int k = t; k < NS; k += nt) {
        uint64_t kk = ~0ull;
        Idx ik = (Idx)~0u;
        if (k < n) {
            const double v = a.llr_f32 ? (double)static_cast<const float*>(a.llr)[shot * n + k]
                                       : static_cast<const double*>(a.llr)[shot * n + k];
            kk = order_key(v);
            ik = (Idx)k;
        }
        key[k] = kk;
        idx[k] = ik;
    }
}

// Compare-exchange of one pair; the column index breaks a tie (stable sort).
template <typename Idx>
__device__ __forceinline__ void bitonic_exchange(uint64_t* key, Idx* idx, int i, int j, bool ascending) {
    const uint64_t ki = key[i], kj = key[j];
    const Idx ii = idx[i], ij = idx[j];
    const bool gt = ki > kj || (ki == kj && ii > ij);
    if (gt == ascending) {
        key[i] = kj;
        key[j] = ki;
        idx[i] = ij;
        idx[j] = ii;
    }
}

// One pass of the network, `stride` inside runs of `size`, over count elements
// that stand at offset `base` of the whole sequence.  The caller's barrier follows.
template <typename Idx>
__device__ __forceinline__ void bitonic_pass(uint64_t* key, Idx* idx, int count, int size, int stride, int base, int t,
                                             int nt) {
    for (int p = t; p < count / 2; p += nt) {
        const int i = 2 * p - (p & (stride - 1));
        bitonic_exchange(key, idx, i, i + stride, ((base + i) & size) == 0);
    }
}

// The whole sort of NS (a power of two) pairs in LDS.
template <typename Idx>
__device__ __forceinline__ void bitonic_sort_lds(uint64_t* key, Idx* idx, int NS, int t, int nt) {
    for (int size = 2; size <= NS; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            bitonic_pass(key, idx, NS, size, stride, 0, t, nt);
            __syncthreads();
        }
}

// ---- 2. the syndrome bit of a row: syn_bit / syn_term of qdec_device.h, the
// rule the BP stages build their rows by

// ---- 4. the first `want` non-pivot positions, ascending (one wave); returns
// how many the positions walked hold, all of them when want >= n
template <typename Idx>
__device__ __forceinline__ int osd_nonpivots(const uint8_t* isp, int n, Idx* npv, int want, int lane) {
    int found = 0;
    for (int base = 0; base < n && found < want; base += 64) {
        const int k = base + lane;
        const bool f = k < n && !isp[k];
        const uint64_t bal = __ballot(f);
        const int at = found + __popcll(bal & ((1ull << lane) - 1ull));
        if (f && at < want) npv[at] = (Idx)k;
        found += __popcll(bal);
    }
    return found;
}

// search width: the order, at most the kn non-pivot columns and kOsdMaxLam
__device__ __forceinline__ int osd_lam(const OsdArgs& a, int kn) {
    const int lam = a.order < 0 ? 0 : (a.order < kn ? a.order : kn);
    return lam < kOsdMaxLam ? lam : kOsdMaxLam;
}

// ---- 5. a candidate's key in the workgroup kernels: weight << 32 | its place in
// the host's order (0: OSD-0; then the singles, ascending; then the pairs by
// pair index; or the OSD-E mask).  The least key wins, so an earlier candidate
// keeps a weight tie and OSD-0 keeps one against all.
__device__ __forceinline__ unsigned long long osd_key(int wgt, uint32_t place) {
    return ((unsigned long long)wgt << 32) | place;
}

// pair index q -> (u, v), u < v < lam_s, lexicographic
__device__ __forceinline__ void pair_of(int q, int lam_s, int& u, int& v) {
    u = 0;
    while (q >= lam_s - 1 - u) {
        q -= lam_s - 1 - u;
        ++u;
    }
    v = u + 1 + q;
}

// ---- 6. osdw, corr = base ^ fold(osdw) and the failure flag of one shot, by one wave
__device__ __forceinline__ void osd_finalize(const DevGraph& g, const OsdArgs& a, int64_t shot, const uint8_t* outb,
                                             int lane) {
    DecodeArgs fa{};
    fa.B = a.B;
    fa.base = a.base;
    fa.readout = a.readout;
    fa.x_out = a.osdw_out;
    fa.corr_out = a.corr_out;
    fa.fail = a.fail;
    finalize_shot(g, fa, shot, outb, false, false, 0, lane);
}

}  // namespace qdec
