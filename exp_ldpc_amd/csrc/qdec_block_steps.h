// qdec_block_steps.h -- the steps that more than one of the 256-thread shot
// kernels uses (bp_block_kernel, ssf_block_kernel, ssf_inc_block_kernel:
// qdec_bp_block.hip; relay_block_kernel: qdec_relay.hip): the shot hand-out, the
// syndrome row build, the generic min-sum check row, the syndrome test of the
// hard decision and the block-wide reduction through the control area
// (qdec_graph.h: kCtrl*).  relay-BP without memory is bp_block_kernel's generic
// min-sum decode bit for bit because both run the rows below.
//
// Device code only.  A step takes pointers and scalars the kernel has already
// loaded (rp, ci, m, tid), not DecodeArgs / RelayArgs, so it re-reads no kernel
// argument.  Steps that end in a barrier say so; all kBlock threads call them.
//
// What stays in each kernel: the variable passes (relay carries the bias of the
// memory term and clamps the marginal and the messages; a policy parameter for
// that would be more machinery than the two loops), the unrolled DRM / DCM
// paths and product-sum of bp_block_kernel, finalize_block, and everything of
// bp_group_kernel and the wave kernels.
#pragma once
#include <hip/hip_runtime.h>

#include "qdec_block_layout.h"
#include "qdec_device.h"

namespace qdec {

// ---- the next shot of a persistent workgroup from the launch's counter.
// Two barriers: every thread has read the answer before the next overwrite.
__device__ __forceinline__ int64_t block_next_shot(unsigned long long* work_ctr, long long* next_s, int tid) {
    if (tid == 0) *next_s = (long long)atomicAdd(work_ctr, 1ull);
    __syncthreads();
    const int64_t s = *next_s;
    __syncthreads();
    return s;
}

// ---- sb[i] = the syndrome bit of row i (syn_bit / syn_term), thread per row.
// The caller's barrier follows.
__device__ __forceinline__ void block_syndrome_rows(uint8_t* sb, const uint8_t* syn, int syn_flags, const uint8_t* base,
                                                    const uint8_t* readout, int64_t shot, int n_data,
                                                    const int32_t* rp, const int32_t* ci, int m, int tid) {
    for (int i = tid; i < m; i += kBlock) {
        int s = syn_bit(syn, shot, m, i);
        if (syn_flags)
            for (int e = rp[i]; e < rp[i + 1]; ++e) s ^= syn_term(syn_flags, base, readout, shot, n_data, ci[e]);
        sb[i] = (uint8_t)s;
    }
}

// ---- min-sum check row over edges [e0, e1), any degree: the two smallest
// |v2c|, the sign from the syndrome bit and the row's parity of v <= 0.  The
// order is the wave kernels' and the oracle's: med3 before fmin, the minimum's
// own edge found by fabs(v) == m1, the scaled minima computed once.
template <typename T>
__device__ __forceinline__ void ms_check_row(const T* v2c, T* c2v, int e0, int e1, int syn, T alpha) {
    T m1 = Big<T>::v, m2 = Big<T>::v;
    int par = syn;
    for (int e = e0; e < e1; ++e) {
        const T v = v2c[e];
        const T av = fabs(v);
        m2 = med3(av, m1, m2);
        m1 = fmin(m1, av);
        par ^= v <= (T)0;
    }
    const T m1a = m1 * alpha, m2a = m2 * alpha;
    for (int e = e0; e < e1; ++e) {
        const T v = v2c[e];
        const T y = (fabs(v) == m1) ? m2a : m1a;
        c2v[e] = (par ^ (v <= (T)0)) ? -y : y;
    }
}

// ---- does the hard decision xh leave a check open?  Thread per row, the
// row's residual bit into rs[i] when rs is not null; ends in a barrier.
__device__ __forceinline__ bool block_syndrome_open(const uint8_t* sb, const uint8_t* xh, const int32_t* rp,
                                                    const int32_t* ci, int m, int tid, uint8_t* rs) {
    int bad = 0;
    for (int i = tid; i < m; i += kBlock) {
        int par = sb[i];
        for (int e = rp[i]; e < rp[i + 1]; ++e) par ^= xh[ci[e]];
        if (rs) rs[i] = (uint8_t)par;
        bad |= par;
    }
    return __syncthreads_or(bad) != 0;
}

// ---- block-wide reduction through red[kBlock / 64] of the control area: the
// wave step (wave_sum_i32, wave_sum_i64, wave_max_i64), then `join` over the
// waves' partials.  Two barriers; every thread gets the result.
template <typename V, typename Wave, typename Join>
__device__ __forceinline__ V block_reduce(V v, V* red, int tid, Wave wave, Join join) {
    v = wave(v);
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    V r = red[0];
    for (int i = 1; i < kBlock / 64; ++i) r = join(r, red[i]);
    __syncthreads();
    return r;
}

template <typename V>
__device__ __forceinline__ V block_sum(V v, V* red, int tid) {
    if constexpr (sizeof(V) == 4) return block_reduce(v, red, tid, wave_sum_i32, [](V a, V b) { return a + b; });
    else return block_reduce(v, red, tid, wave_sum_i64, [](V a, V b) { return a + b; });
}

__device__ __forceinline__ long long block_max(long long v, long long* red, int tid) {
    return block_reduce(v, red, tid, wave_max_i64, [](long long a, long long b) { return b > a ? b : a; });
}

}  // namespace qdec
