// qdec_bp_ms.h -- min-sum BP wave kernel with compressed check-node state
// (MsCore) and the two BP kernels built on it, bp_ms_wave_kernel and
// bp_ms_cmp_kernel.  Both are compiled by qdec_ms_rv4.hip and qdec_ms_rvx.hip,
// each for its wave shapes, which is why they share a header.
//
// Same arithmetic as bp_wave_kernel<T, MIN_SUM> (ldpc v1 min-sum-log, bit-exact
// against the oracle), with less LDS traffic.  The check pass does not scatter
// c2v messages.  It only writes a per-check state (m1, m2, parity); m2's sign
// bit carries the parity.  The variable lane rebuilds each incoming message
// from that state and from the v2c message it sent last iteration, which it
// keeps in registers:
//     c = alpha * ((|v| == m1) ? m2 : m1),  negated iff parity ^ (v <= 0).
// This is the same selection the check pass of bp_wave_kernel makes, on the
// same operands.  Per iteration and wave, the LDS traffic is:
//   check pass  RC x (ds_read_b128 x2 row + ds_write_b64 state)
//   var pass    RV x 4 x (ds_read_b64 state gather + ds_write_b32 v2c scatter)
// The syndrome test needs no LDS at all.  Hard decisions are ballots
// (X[w] = 64 lane slots per word), and check i's parity is
// popc(X & smask_i) mod 2 with per-lane slot masks.  The host (qdec_abi.cpp
// ms_layout) places variables in lane slots by ascending degree, so the
// leading all-degree-3 rounds (D3R) run a 3-edge variable pass.  It also picks
// v2c row positions so each scatter instruction has at most 2-way bank
// conflicts, which ds_write_b32 absorbs for free.  Shot inputs are staged
// through LDS one shot ahead (ShotIo).
#pragma once
#include "qdec_cmp_list.h"
#include "qdec_device.h"
#include "qdec_kernels.h"
#include "qdec_shot_seq.h"

namespace qdec {

template <typename T>
struct FBits;
template <>
struct FBits<float> {
    using U = uint32_t;
    __device__ static U to(float x) { return __float_as_uint(x); }
    __device__ static float from(U u) { return __uint_as_float(u); }
};
template <>
struct FBits<double> {
    using U = unsigned long long;
    __device__ static U to(double x) { return (U)__double_as_longlong(x); }
    __device__ static double from(U u) { return __longlong_as_double((long long)u); }
};

// f64 min/max on the VALU without the IEEE canonicalisation of the operands
// (finite, non-NaN inputs only): max(a, |b|), min(a, |b|), min(a, b).
__device__ __forceinline__ double max_abs_f64(double a, double b) {
    double r;
    asm("v_max_f64 %0, %1, |%2|" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ double min_abs_f64(double a, double b) {
    double r;
    asm("v_min_f64 %0, %1, |%2|" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ double min_f64(double a, double b) {
    double r;
    asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

__device__ __forceinline__ double max_f64(double a, double b) {
    double r;
    asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ double min_abs2_f64(double a, double b) {
    double r;
    asm("v_min_f64 %0, |%1|, |%2|" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ double max_abs2_f64(double a, double b) {
    double r;
    asm("v_max_f64 %0, |%1|, |%2|" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// Sign-bit tests for f64 messages (LEAN launches only; the others keep the
// compares).  ldpc's sign test `v <= 0` equals v's sign bit for every v but +0.
// The check pass takes its row parity as the XOR of the high dwords (no f64
// compares) and the variable pass flips a message's sign by the sign bit of the
// v2c message it sent.  Both differ from the compares only through zero
// entries, and a zero entry makes the row's m1 zero, so a row with m1 == 0
// (one wave-uniform branch after all check rounds, which reads the row again:
// equal priors send an exact +0 in iteration 1, so every listed shot meets one
// in iteration 2) takes the parity from the compares and gives m2 (the magnitude
// its zero entries select) the sign that makes the variable side's sign bit
// test exact: the parity, flipped when the zeros are +0.  A
// row holding both +0 and -0 has m2 = 0, where only the sign of a zero message
// is left open, which changes no `<= 0` test, no magnitude and no hard
// decision (only the sign of an exactly-zero posterior, which LEAN launches do
// not output).
__device__ __forceinline__ uint32_t f64_hi(double x) { return (uint32_t)((unsigned long long)__double_as_longlong(x) >> 32); }
// x with its sign bit XORed with bit 31 of m: one v_bitop3_b32 on the high
// dword (table 0x6c = (src0 & src2) ^ src1)
__device__ __forceinline__ double f64_xor_sign(double x, uint32_t m) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    const uint32_t hi = __builtin_amdgcn_bitop3_b32(m, (uint32_t)(b >> 32), 0x80000000u, 0x6c);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | (uint32_t)b));
}

// (smallest, second smallest) of |v[B]| .. |v[E-1]|, counted with multiplicity
// (ldpc's leave-one-out minima need exactly these two).  Leaves are pairs
// (min, max) or a single value (hi = none); merge(A, B) = (min(A.lo, B.lo),
// min(max(A.lo, B.lo), min(A.hi, B.hi))).
struct Top2 {
    double lo, hi;
    bool has_hi;
};
template <int B, int E>
__device__ __forceinline__ Top2 top2_tree(const double* v) {
    static_assert(E > B, "empty range");
    if constexpr (E - B == 1) {
        return Top2{fabs(v[B]), 0.0, false};
    } else if constexpr (E - B == 2) {
        return Top2{min_abs2_f64(v[B], v[B + 1]), max_abs2_f64(v[B], v[B + 1]), true};
    } else {
        constexpr int M = B + ((E - B) / 2 + 1) / 2 * 2;  // left part: an even count of leaves' values
        const Top2 a = top2_tree<B, M>(v);
        Top2 r;
        if constexpr (E - M == 1) {
            // a single value on the right: |v[M]| as an operand modifier of the
            // merge itself (the same operands, without a register pair for the leaf)
            r.lo = min_abs_f64(a.lo, v[M]);
            double h = max_abs_f64(a.lo, v[M]);
            if (a.has_hi) h = min_f64(h, a.hi);
            r.hi = h;
            r.has_hi = true;
            return r;
        }
        const Top2 b = top2_tree<M, E>(v);
        r.lo = min_f64(a.lo, b.lo);
        double h = max_f64(a.lo, b.lo);
        if (a.has_hi && b.has_hi)
            h = min_f64(h, min_f64(a.hi, b.hi));
        else if (a.has_hi)
            h = min_f64(h, a.hi);
        else if (b.has_hi)
            h = min_f64(h, b.hi);
        r.hi = h;
        r.has_hi = true;
        return r;
    }
}

// LDS carve-up (elements of T, then bytes)
template <typename T>
struct MsLds {
    static constexpr int DRS = lds_stride<T, kDR>();
    // v2c rows: the m checks plus one all-Big row (index m) that every pad check
    // lane reads; then the 64 dummy elements pad edges scatter into
    __host__ __device__ static int rows(const DevGraph& g) { return g.m + 1; }
    __host__ __device__ static size_t v2c_elems(int nrows) { return ((size_t)nrows * DRS + 64 + 1) / 2 * 2; }
    __host__ __device__ static size_t state_elems(int m_pad) {
        return ((size_t)2 * (m_pad + 1) * sizeof(T) + 15) / 16 * 16 / sizeof(T);
    }
    __host__ __device__ static size_t core_bytes(const DevGraph& g) {
        return ((v2c_elems(rows(g)) + state_elems(g.m_pad)) * sizeof(T) + (size_t)g.n_pad + 64 + 15) / 16 * 16;
    }
    template <int RC, int RV>
    __host__ __device__ static size_t bytes(const DevGraph& g) {
        return core_bytes(g) + ShotIo<RC, RV>::bytes(g);
    }
};

// alpha_t = 1 - 2^-t (ms_scaling == 0) built from bits on the scalar unit:
// 1 - 2^-t is 1.0 minus 2^(P-t) units in the last place below 1.0 (P = 24 for
// float, 53 for double), and rounds to 1.0 for t > P, exactly as
// (T)(1.0 - ldexp(1.0, -t)) does.
template <typename T>
__device__ __forceinline__ T alpha_bits(int it, double ms_scaling) {
    if (ms_scaling != 0.0) return (T)ms_scaling;
    if constexpr (sizeof(T) == 4) {
        const uint32_t u = 0x3F800000u - (it <= 24 ? (1u << (24 - it)) : 0u);
        return __uint_as_float(u);
    } else {
        const unsigned long long u = 0x3FF0000000000000ull - (it <= 53 ? (1ull << (53 - it)) : 0ull);
        return __longlong_as_double((long long)u);
    }
}

// The per-wave part shared by the min-sum wave kernels: this lane's slot and
// state tables, and BP iterations on the wave's LDS rows.  D3R: leading
// variable rounds whose slots all have degree <= 3.  LEAN: the kernel writes no
// llr (Q is not kept) and may use the sign-bit check pass.
template <typename T, int RC, int RV, int DRC, bool LEAN, int D3R>
struct MsCore {
    static_assert(DRC <= kDR, "compute width exceeds the LDS row");
    static_assert(D3R <= RV, "degree rounds");
    using V2 = __attribute__((ext_vector_type(2))) T;
    static constexpr int DRS = MsLds<T>::DRS;
    // the variable pass runs rounds in pairs (2p, 2p+1) on packed fp32 pairs;
    // an odd last round pairs with itself.  D3P: leading 3-edge rounds, whole pairs.
    static constexpr int NP = (RV + 1) / 2;
    static constexpr int D3P = D3R & ~1;
    static constexpr int PREC = sizeof(T) == 4 ? 1 : 0;
    static constexpr bool SB = sizeof(T) == 8 && LEAN;

    uint32_t etab[RV][kDC];      // v2c element | state index << 16 (edges k < kd(rv))
    V2 L[NP];                    // priors of rounds (2p, 2p+1)
    uint32_t vsl[(RV + 1) / 2];  // columns of this lane's slots, u16 pairs
    int sslot[RC];               // where this lane's checks write their state (host-placed)
    uint64_t smask[RC][RV];      // slots of this lane's checks' columns, per 64-slot word

    __device__ __forceinline__ void load(const DevGraph& g, int lane) {
        const T* prior = reinterpret_cast<const T*>(g.ms_prior[PREC]);
#pragma unroll
        for (int rv = 0; rv < RV; ++rv) {
            const int sl = rv * 64 + lane;
            if (rv % 2 == 0) L[rv / 2].x = L[rv / 2].y = prior[sl];
            else L[rv / 2].y = prior[sl];
#pragma unroll
            for (int k = 0; k < kDC; ++k) etab[rv][k] = (rv < D3P && k == 3) ? 0u : g.ms_etab[PREC][k * g.n_pad + sl];
            if (rv % 2 == 0) vsl[rv / 2] = g.ms_vslot[sl];
            else vsl[rv / 2] |= (uint32_t)g.ms_vslot[sl] << 16;
        }
#pragma unroll
        for (int rc = 0; rc < RC; ++rc) sslot[rc] = g.ms_sslot[PREC][rc * 64 + lane];
#pragma unroll
        for (int rc = 0; rc < RC; ++rc)
#pragma unroll
            for (int w = 0; w < RV; ++w) smask[rc][w] = g.ms_smask[(size_t)w * g.m_pad + rc * 64 + lane];
    }
    __device__ __forceinline__ int col_of(int rv) const { return (int)((vsl[rv / 2] >> (16 * (rv % 2))) & 0xffffu); }

    // one-time LDS init: unused row positions hold Big forever (never the
    // minimum, positive sign), state m_pad is the zero state of pad edges
    __device__ __forceinline__ static void init_lds(const DevGraph& g, T* v2c, T* st, uint8_t* xh, int lane) {
        for (int e = lane; e < (int)MsLds<T>::v2c_elems(MsLds<T>::rows(g)); e += 64) v2c[e] = Big<T>::v;
        for (int e = lane; e < (int)MsLds<T>::state_elems(g.m_pad); e += 64) st[e] = (T)0;
        for (int e = lane; e < g.n_pad + 64; e += 64) xh[e] = 0;
    }

    // initial messages: v2c = prior
    __device__ __forceinline__ void write_priors(T* v2c) const {
#pragma unroll
        for (int rv = 0; rv < RV; ++rv)
#pragma unroll
            for (int k = 0; k < kDC; ++k)
                if (!(rv < D3P && k == 3)) v2c[etab[rv][k] & 0xffff] = (rv % 2 == 0) ? L[rv / 2].x : L[rv / 2].y;
    }

    // the first check state from the host's table (ms_state0, qdec_tables.cpp:
    // what the check pass writes for rows holding the priors, syndrome bit 0, by
    // check lane), both signs flipped where the shot's syndrome bit is set
    __device__ __forceinline__ static void load_state0(const DevGraph& g, int lane, V2 (&s0)[RC]) {
        // scalar base + 32-bit lane offset (opaque here, so no per-lane address is
        // formed ahead of the shot loop and kept in a VGPR pair across the BP loop)
        const char* t = static_cast<const char*>(g.ms_state0[PREC]);
        uint32_t off = (uint32_t)lane * (uint32_t)sizeof(V2);
        asm volatile("" : "+v"(off));
#pragma unroll
        for (int rc = 0; rc < RC; ++rc) s0[rc] = *reinterpret_cast<const V2*>(t + off + rc * 64 * sizeof(V2));
    }
    __device__ __forceinline__ void write_state0(T* st, const V2 (&s0)[RC], const bool (&sbit)[RC]) const {
#pragma unroll
        for (int rc = 0; rc < RC; ++rc) *reinterpret_cast<V2*>(st + 2 * sslot[rc]) = sbit[rc] ? -s0[rc] : s0[rc];
    }

    // BP iterations it, it + 1, .. max_iter.  STATE0 = false: on rows holding
    // the priors (write_priors, then a wave_lds_sync).  STATE0 = true (it = 1):
    // on the first check state (write_state0, then a wave_lds_sync); iteration
    // 1 has no check pass, and its variable pass, which sees the priors as the
    // messages sent (vp), fills the rows.  Returns true when the syndrome is
    // met (`it` = that iteration); X: hard decisions by slot (ballot words),
    // pres: the residual syndrome bit of this lane's checks, Q: posteriors (!LEAN).
    template <bool STATE0 = false>
    __device__ __forceinline__ bool iterate(const DecodeArgs& a, T* v2c, T* st, int m, int lane, const bool (&sbit)[RC],
                                            T (&Q)[RV], uint64_t (&X)[RV], bool (&pres)[RC], int& it) const {
        V2 vp[NP][kDC];  // v2c messages this lane sent last iteration, round pairs
#pragma unroll
        for (int p = 0; p < NP; ++p)
#pragma unroll
            for (int k = 0; k < kDC; ++k) vp[p][k] = L[p];
        for (; it <= a.max_iter; ++it) {
            const T alpha = alpha_bits<T>(it, a.ms_scaling);
            // ---- check pass: state (m1, m2) with the parity in both signs
            // (STATE0: iteration 1 starts from the table's state instead) ----
            if (!STATE0 || it != 1) {
                // three sweeps over a group of check rounds, so that no round's row
                // loads wait behind another round's minima, branch or store
                auto load_row = [&](int rc, T (&w)[kDR]) {
                    const int i = min(rc * 64 + lane, m);  // pad check lanes share the Big row m
                    // odd f64 rows load only their DRC slots (r03i A/B: -0.5% BP kernel time)
                    if constexpr (sizeof(T) == 8 && DRC % 2 == 1) lds_load_first<T, DRC>(v2c + i * DRS, w);
                    else lds_load<T, kDR>(v2c + i * DRS, w);
                };
                // (a group is every round; four rounds go two at a time: four rows at
                // once only add to the scratch of the (4, 9, 8) kernels)
                constexpr int G = RC > 2 ? 2 : RC;
                static_assert(RC % G == 0, "whole groups");
#pragma unroll
                for (int g0 = 0; g0 < RC; g0 += G) {
                    // sweep 1: the group's rows
                    T v[G][kDR];
#pragma unroll
                    for (int r = 0; r < G; ++r) load_row(g0 + r, v[r]);
                    // sweep 2: minima, parity and state per round
                    V2 s2[G];
#pragma unroll
                    for (int r = 0; r < G; ++r) {
                        const int rc = g0 + r;
                        T m1 = Big<T>::v, m2 = Big<T>::v;
                        if constexpr (sizeof(T) == 4) {
#pragma unroll
                            for (int k = 0; k < DRC; ++k) {
                                const T av = fabs(v[r][k]);
                                m2 = med3(av, m1, m2);
                                m1 = med3(av, m1, -Big<T>::v);  // true median = min(|v|, m1): one VALU, abs modifier
                            }
                        } else {
                            // f64: (minimum, second minimum) of |v| by a merge tree instead of a
                            // sequential chain (17 instead of 21 f64 ops for 7 values, depth 5
                            // instead of 14); the same two values, so bit-identical
                            const Top2 t = top2_tree<0, DRC>(v[r]);
                            m1 = t.lo;
                            m2 = t.hi;
                        }
                        if constexpr (SB) {
                            // sign-canonical row: the parity is the XOR of the sign bits
                            uint32_t hx = sbit[rc] ? 0x80000000u : 0u;
                            int k = 0;
#pragma unroll
                            for (; k + 1 < DRC; k += 2)
                                hx = __builtin_amdgcn_bitop3_b32(hx, f64_hi(v[r][k]), f64_hi(v[r][k + 1]), 0x96);
                            if (k < DRC) hx ^= f64_hi(v[r][k]);
                            // m1, m2 >= +0: the XOR of the parity bit sets their sign bit
                            s2[r].x = f64_xor_sign(m1, hx);
                            s2[r].y = f64_xor_sign(m2, hx);
                        } else {
                            bool par = sbit[rc];
#pragma unroll
                            for (int k = 0; k < DRC; ++k)
                                par ^= v[r][k] <= (T)0;  // ldpc: bit_to_check <= 0 flips the sign (s_xor of compare masks)
                            // both minima carry the parity in their sign bit (they are >= +0)
                            s2[r].x = par ? -m1 : m1;
                            s2[r].y = par ? -m2 : m2;
                        }
                    }
                    // sweep 3: the states
#pragma unroll
                    for (int r = 0; r < G; ++r) *reinterpret_cast<V2*>(st + 2 * sslot[g0 + r]) = s2[r];
                    if constexpr (SB) {
                        // a row with a zero entry (one wave-uniform test for the group):
                        // m1's sign is the parity by ldpc's compares; m2 (the magnitude the
                        // row's zero entries select) gets the parity flipped when those zeros
                        // are +0, so that the variable side's sign-bit test gives
                        // parity ^ (v <= 0) for them too.  The rare branch reads its rows
                        // again, one round at a time (nothing has written them since sweep 1:
                        // holding sweep 1's rows for it costs the 3-waves-per-SIMD build its
                        // register budget), and writes the state a second time (a state
                        // patched in registers ahead of sweep 3 costs the loop four copies)
                        bool zero = false;
#pragma unroll
                        for (int r = 0; r < G; ++r) zero |= s2[r].x == (T)0;
                        if (__builtin_expect(__ballot(zero) != 0ull, 0)) {
                            asm volatile("" ::: "memory");  // a load of its own, not sweep 1's registers
#pragma unroll
                            for (int r = 0; r < G; ++r) {
                                const int rc = g0 + r;
                                if (s2[r].x == (T)0) {
                                    T w[kDR];
                                    load_row(rc, w);
                                    bool par = sbit[rc], pz = false;
#pragma unroll
                                    for (int j = 0; j < DRC; ++j) {
                                        par ^= w[j] <= (T)0;
                                        pz |= FBits<T>::to(w[j]) == 0;  // +0
                                    }
                                    V2 f;
                                    f.x = par ? -(T)0 : (T)0;
                                    f.y = (par != pz) ? -fabs(s2[r].y) : fabs(s2[r].y);
                                    *reinterpret_cast<V2*>(st + 2 * sslot[rc]) = f;
                                }
                            }
                        }
                    }
                }
                wave_lds_sync();
            }

            // ---- variable pass, rounds in pairs (the next pair's states are
            // gathered while this pair sums) ----
            auto gather = [&](int p, V2 (&sa)[kDC], V2 (&sb)[kDC]) {
                const int r0 = 2 * p, r1 = 2 * p + 1 < RV ? 2 * p + 1 : 2 * p;
#pragma unroll
                for (int k = 0; k < kDC; ++k)
                    if (!(r1 < D3P && k == 3)) {
                        sa[k] = *reinterpret_cast<const V2*>(st + 2 * (etab[r0][k] >> 16));
                        if (r1 != r0) sb[k] = *reinterpret_cast<const V2*>(st + 2 * (etab[r1][k] >> 16));
                    }
            };
            V2 sa[kDC], sb[kDC];
            gather(0, sa, sb);
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const int r0 = 2 * p, r1 = 2 * p + 1 < RV ? 2 * p + 1 : 2 * p;
                const int KD = r1 < D3P ? 3 : kDC;
                // |c| = alpha * ((|v| == m1) ? m2 : m1), sign = parity ^ (v <= 0);
                // the state's signs carry the parity, so one select picks both
                V2 y[kDC];
#pragma unroll
                for (int k = 0; k < kDC; ++k) {
                    if (k < KD) {
                        y[k].x = (fabs(vp[p][k].x) == fabs(sa[k].x)) ? sa[k].y : sa[k].x;
                        const V2 sbk = r1 != r0 ? sb[k] : sa[k];
                        y[k].y = (fabs(vp[p][k].y) == fabs(sbk.x)) ? sbk.y : sbk.x;
                    }
                }
                if (p + 1 < NP) gather(p + 1 < NP ? p + 1 : p, sa, sb);
                V2 c[kDC];
#pragma unroll
                for (int k = 0; k < kDC; ++k) {
                    if (k < KD) {
                        const V2 yk = y[k] * alpha;
                        if constexpr (SB) {
                            c[k].x = f64_xor_sign(yk.x, f64_hi(vp[p][k].x));
                            c[k].y = f64_xor_sign(yk.y, f64_hi(vp[p][k].y));
                        } else {
                            c[k].x = (vp[p][k].x <= (T)0) ? -yk.x : yk.x;
                            c[k].y = (vp[p][k].y <= (T)0) ? -yk.y : yk.y;
                        }
                    }
                }
                V2 pre[kDC];
                V2 acc = L[p];
#pragma unroll
                for (int k = 0; k < kDC; ++k) {
                    if (k < KD) {
                        pre[k] = acc;
                        acc += c[k];
                    }
                }
                if constexpr (!LEAN) {
                    Q[r0] = acc.x;
                    Q[r1] = acc.y;
                }
                X[r0] = __ballot(acc.x <= (T)0);
                if (r1 != r0) X[r1] = __ballot(acc.y <= (T)0);
                // ldpc: out_k = pre_k + (sum of the later c); the last one adds an
                // empty sum (+0), which can only turn -0 into +0: both are <= 0 and
                // have |v| = 0, so the message is used identically either way
                V2 suf;
#pragma unroll
                for (int k = kDC - 1; k >= 0; --k) {
                    if (k < KD) {
                        const V2 out = (k == KD - 1) ? pre[k] : pre[k] + suf;
                        suf = (k == KD - 1) ? c[k] : suf + c[k];
                        vp[p][k] = out;
                        v2c[etab[r0][k] & 0xffff] = out.x;  // pads -> dummy element
                        if (r1 != r0) v2c[etab[r1][k] & 0xffff] = out.y;
                    }
                }
            }

            // ---- syndrome test (registers only), staged: a later round of checks
            // is tested only when the earlier rounds are all met (most failing
            // iterations stop at the first) ----
            bool failed = false;
#pragma unroll
            for (int rc = 0; rc < RC; ++rc) {
                if (!failed) {  // wave-uniform
                    pres[rc] = sbit[rc] != (masked_parity<RV>(smask[rc], X) != 0);
                    failed = __ballot(pres[rc]) != 0ull;
                }
            }
            wave_lds_sync();  // v2c scatter complete before the next check pass
            if (!failed) return true;
        }
        // not converged: the whole residual of the last iteration (the SSF queue's)
#pragma unroll
        for (int rc = 0; rc < RC; ++rc) pres[rc] = sbit[rc] != (masked_parity<RV>(smask[rc], X) != 0);
        return false;
    }
};

// LEAN: the throughput configuration (no x / corr / llr outputs, no base, no
// syndrome flags, no spacetime fold): the per-shot epilogue is the ballot-word
// failure check only, which keeps the kernel's scalar state small.
// D3R: leading variable rounds whose slots all have degree <= 3.
// f64: launched at 2 waves per SIMD (launch_bp_wave caps the grid; measured
// faster than 3), so the register budget is 256; f32: 4 waves (<= 128 VGPRs).
// OCC: waves per SIMD the registers are budgeted for (0 = the default above).
// The f64 LEAN kernel also comes as OCC = 3 (<= 168 VGPRs, a few dwords of the
// per-shot epilogue spilled), launched when a handle asks for more than 8 f64
// waves per CU (qd_graph_set_wave_occupancy: the bench's concurrent points).
template <typename T, int RC, int RV, int DRC, bool DEFER, bool LEAN, int D3R, int OCC = 0>
__global__ __launch_bounds__(64, OCC > 0 ? OCC : (sizeof(T) == 4 ? 4 : 2)) void bp_ms_wave_kernel(DevGraph g, DecodeArgs a) {
    using Io = ShotIo<RC, RV>;
    using Core = MsCore<T, RC, RV, DRC, LEAN, D3R>;
    constexpr int PREC = Core::PREC;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    T* v2c = reinterpret_cast<T*>(smem);
    T* st = v2c + MsLds<T>::v2c_elems(MsLds<T>::rows(g));
    uint8_t* xh = reinterpret_cast<uint8_t*>(st + MsLds<T>::state_elems(g.m_pad));
    Io io(g, smem + MsLds<T>::core_bytes(g));

    const int lane = threadIdx.x;
    const int m = g.m, n = g.n;
    Core core;
    core.load(g, lane);
    // zero syndrome + every prior > 0: iteration 1 converges with x = 0 (all
    // messages are >= 0, so every posterior is >= its prior > 0), and the LEAN
    // outputs (iterations 1, converged, failure from the readout alone) need
    // nothing else
    const bool zero_ok = LEAN && ((g.ms_allpos >> PREC) & 1);

    Core::init_lds(g, v2c, st, xh, lane);
    io.init(g, lane);
    ShotSeq seq(a, lane);
    int64_t shot = seq.next(lane);
    typename Io::Shift sh = io.stage(g, a, shot, 0, 0, lane);  // row offsets of `shot`'s stage
    int64_t nxt = seq.next(lane);
    wave_lds_sync();

    int sb = 0, buf = 0;  // syndrome / readout staging buffers of `shot`
    QDEC_STAMP_DECL
#ifdef QDEC_STAMPS
    const unsigned long long qdec_t0 = __builtin_amdgcn_s_memtime(), qdec_r0 = __builtin_amdgcn_s_memrealtime();
#endif
    for (; shot < a.B;) {
        // ---- syndrome (staged one shot ahead: at least the NR readout loads of
        // the same stage are younger); then stage the next shot ----
        QDEC_STAMP(5);
        wait_vmem<Io::kWaitSyn>();
        Io::patch_tail(a.syn, a.B, m, shot, io.syn_area(sb), sh.s, lane);
        wave_lds_sync();
        QDEC_STAMP(0);
        bool sbit[RC];  // lane masks: parity work stays on the scalar unit
        const uint8_t* srow = io.syn_area(sb) + sh.s;
#pragma unroll
        for (int rc = 0; rc < RC; ++rc) {
            const int i = rc * 64 + lane;
            sbit[rc] = (i < m && a.syn) ? (srow[i] & 1) != 0 : false;
        }
        wait_lds();
        const int64_t nn = seq.next(lane);  // any counter request is older than the stage
        const typename Io::Shift shn = io.stage(g, a, nxt, 0, buf ^ 1, lane);
        if (!LEAN && a.syn_flags) {
            const bool use_b = (a.syn_flags & 1) && a.base;
            const bool use_r = (a.syn_flags & 2) && a.readout;
            uint64_t Xf[RV];
#pragma unroll
            for (int w = 0; w < RV; ++w) {
                const int q = core.col_of(w);
                int v = 0;
                if (q < g.n_data) {
                    if (use_b) v ^= a.base[shot * g.n_data + q];
                    if (use_r) v ^= a.readout[shot * g.n_data + q];
                }
                Xf[w] = __ballot(v & 1);
            }
#pragma unroll
            for (int rc = 0; rc < RC; ++rc) {
                uint64_t acc = 0;
#pragma unroll
                for (int w = 0; w < RV; ++w) acc ^= core.smask[rc][w] & Xf[w];
                sbit[rc] ^= (__popcll(acc) & 1) != 0;
            }
        }

        // ---- initial messages: v2c = prior, unless the shot is skipped ----
        bool skip = false;
        if (zero_ok) {
            bool any = false;
#pragma unroll
            for (int rc = 0; rc < RC; ++rc) any |= sbit[rc];
            skip = __ballot(any) == 0ull;
        }
        if (!skip) core.write_priors(v2c);
        wave_lds_sync();

        QDEC_STAMP(1);
        T Q[RV];
        uint64_t X[RV];
        bool pres[RC];
        int it = 1;
        bool conv = false;
        if (skip) {
            conv = true;
#pragma unroll
            for (int rv = 0; rv < RV; ++rv) X[rv] = 0ull;
#pragma unroll
            for (int rc = 0; rc < RC; ++rc) pres[rc] = false;
        }
        if (!skip) conv = core.iterate(a, v2c, st, m, lane, sbit, Q, X, pres, it);
        const int iters = conv ? it : a.max_iter;
        QDEC_STAMP(2);
        QDEC_COUNT(8, iters);
        QDEC_COUNT(9, 1);
        // this shot's readout: wait before any store of this shot, so the
        // kWaitRd most recent vector-memory operations are the later shots' stages
        const bool need_rd = a.readout && a.fail && g.k > 0;  // the SSF queue carries it too
        if (need_rd) {
            wait_vmem<Io::kWaitRd>();
            Io::patch_tail(a.readout, a.B, g.n_data, shot, io.rd_area(buf), sh.r, lane);
        }
        if (lane == 0 && a.iters) a.iters[shot] = iters;
        // hard decision by column (slot order -> xh[column])
#pragma unroll
        for (int rv = 0; rv < RV; ++rv) xh[core.col_of(rv)] = (uint8_t)((X[rv] >> lane) & 1);
        if (!LEAN && a.llr_out) {
            T* lo = reinterpret_cast<T*>(a.llr_out);
#pragma unroll
            for (int rv = 0; rv < RV; ++rv) {
                const int j = core.col_of(rv);
                if (j < n) lo[shot * n + j] = Q[rv];
            }
        }
        wave_lds_sync();
        QDEC_STAMP(3);
        if (DEFER && !conv) {
            if (LEAN || a.q_packed) {  // LEAN launches always use the packed queue
                uint64_t xw[RV], rw[RC], dw[RV];
                const uint8_t* rrow = io.rd_area(buf) + sh.r;
#pragma unroll
                for (int w = 0; w < RV; ++w) {
                    const int q = w * 64 + lane;
                    xw[w] = __ballot(xh[q] & 1);
                    dw[w] = need_rd ? __ballot(q < g.n_data && (rrow[q] & 1)) : 0ull;
                }
#pragma unroll
                for (int rc = 0; rc < RC; ++rc) rw[rc] = __ballot(pres[rc]);
                queue_push_packed<RV, RC>(a, shot, xw, rw, dw, lane);
            } else {
                int slot = 0;
                if (lane == 0) slot = atomicAdd(a.q_count, 1);
                slot = __shfl(slot, 0);
                for (int j = lane; j < n; j += 64) a.q_x[(int64_t)slot * n + j] = xh[j];
#pragma unroll
                for (int rc = 0; rc < RC; ++rc) {
                    const int i = rc * 64 + lane;
                    if (i < m) a.q_r[(int64_t)slot * m + i] = (uint8_t)pres[rc];
                }
                if (lane == 0) a.q_idx[slot] = shot;
            }
        } else if (LEAN || (g.fold_blocks == 1 && !a.corr_out)) {
            if (!LEAN && a.x_out)
                for (int j = lane; j < n; j += 64) a.x_out[shot * n + j] = xh[j];
            int any_fail = 0;
            if (a.fail && a.readout && g.k > 0) {
                uint64_t Xc[RV];  // hard decision by column
#pragma unroll
                for (int w = 0; w < RV; ++w) Xc[w] = __ballot(xh[w * 64 + lane] & 1);
                any_fail = fail_from_words<RV, !LEAN>(g, a, shot, lane, Xc, io.rd_area(buf) + sh.r, io.lz);
            }
            if (lane == 0) {
                if (a.status) a.status[shot] = (uint8_t)(conv ? 3 : 0);
                if (a.ssf_steps) a.ssf_steps[shot] = 0;
                if (a.fail) a.fail[shot] = (uint8_t)any_fail;
            }
        } else {
            finalize_shot_io(g, a, shot, xh, conv, conv, 0, lane, io.rd_area(buf) + sh.r, io.lz);
        }
        wave_lds_sync();
        QDEC_STAMP(4);
        shot = nxt;
        nxt = nn;
        sh = shn;
        buf ^= 1;
    }
#ifdef QDEC_STAMPS
    QDEC_COUNT(10, __builtin_amdgcn_s_memtime() - qdec_t0);
    QDEC_COUNT(11, __builtin_amdgcn_s_memrealtime() - qdec_r0);
    QDEC_COUNT(12, 1);
#endif
    QDEC_FLUSH_AT(0);
}

// lane l's copy of v from lane l - off (lanes below off: their own value)
__device__ __forceinline__ uint64_t readlane64_up(uint64_t v, int off, int lane) {
    const int src = lane >= off ? lane - off : lane;
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src);
    const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src);
    return ((uint64_t)hi << 32) | lo;
}

// v_readlane of a 64-bit value (lane uniform)
__device__ __forceinline__ uint64_t readlane64(uint64_t v, int l) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l);
    return ((uint64_t)hi << 32) | lo;
}

// Small-set-flip of one BP-failed shot inside the compact BP kernel (FUSE > 0,
// QD_OPT_SSF_FUSE): the table-driven spec of ssf_lut_kernel (qdec_bp.hip), with
// the same tables (s_lut, s_off, s_lcw, s_tog), the same key, the same step
// order and the same flip application, so the same outputs; the tables are read
// through the cache hierarchy instead of a workgroup's LDS copy, and the shot
// never goes through the HBM queue or a second launch.  RG: generators per lane
// (n_gen <= 64 * RG).  xb: the wave's hard decision by column as LDS bit words
// (updated in place); flog: the wave's step log; R: residual words by check.
// Returns the steps taken; sw_out = the residual weight left.
template <int RG, int RW>
__device__ __forceinline__ int ssf_fused(const DevGraph& g, int max_steps, uint32_t* xb, uint16_t* flog,
                                      const uint64_t* Rin, int lane, int* sw_out) {
    const uint32_t* __restrict__ lut = g.s_lut;
    const uint32_t* __restrict__ tog = g.s_tog;
    // this lane's generators' table offsets (the winner's local-check ids are read
    // per step at a wave-uniform address instead of being held in registers)
    uint32_t off[RG];
#pragma unroll
    for (int rg = 0; rg < RG; ++rg) off[rg] = g.s_off[rg * 64 + lane];
    // first local syndromes: the toggle rows of the violated checks, 8 rows per
    // round (independent loads; row m_pad is all zero)
    const uint32_t zrow = (uint32_t)g.m_pad;
    uint32_t sl = 0;
    int sw = 0;
#pragma unroll
    for (int w = 0; w < RW; ++w) {
        uint64_t bits = Rin[w];
        sw += __popcll(bits);
        while (bits) {
            uint32_t t = 0;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                uint32_t c = zrow;
                if (bits) {
                    c = (uint32_t)(w * 64 + __builtin_ctzll(bits));
                    bits &= bits - 1;
                }
                t ^= tog[c * 64 + lane];
            }
            sl ^= t;
        }
    }
    int steps = 0;
    while (sw > 0 && (max_steps <= 0 || steps < max_steps)) {
        // every generator's best (rank, -g, t); wave max
        uint32_t e[RG];
        int kv = 0;
#pragma unroll
        for (int rg = 0; rg < RG; ++rg) {
            const uint32_t s = rg ? (sl >> 16) : (sl & 0xffffu);
            e[rg] = lut[off[rg] + s];
            const uint32_t rank = e[rg] >> 24;
            const int key = rank ? (int)((rank << 15) | ((uint32_t)(127 - (rg * 64 + lane)) << 8) | (e[rg] & 0xffu)) : 0;
            kv = max(kv, key);
        }
        const int best = wave_max_i32(kv);
        if (best == 0) break;  // no positive gain left
        const int gsel = 127 - ((best >> 8) & 127);
        const int tsel = best & 255;
        const int owner = gsel & 63;
        const bool hi = RG == 2 && gsel >= 64;
        const uint32_t esel = (uint32_t)__builtin_amdgcn_readlane((int)(hi ? e[RG - 1] : e[0]), owner);
        const uint32_t slg = ((uint32_t)__builtin_amdgcn_readlane((int)sl, owner) >> (hi ? 16 : 0)) & 0xffffu;
        const uint32_t fm = (esel >> 8) & 0xffffu;
        sw -= __builtin_popcount(slg) - __builtin_popcount(slg ^ fm);
        ++steps;
        // toggle the flipped checks' local-syndrome bits (all loads issued first)
        uint32_t tr[kLutLC];
#pragma unroll
        for (int w = 0; w < kLutLCW; ++w) {
            const uint32_t nib = (fm >> (4 * w)) & 0xfu;
            const uint32_t word = nib ? g.s_lcw[w * g.g_pad + gsel] : 0u;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                tr[4 * w + b] = 0u;
                if ((nib >> b) & 1u) tr[4 * w + b] = tog[((word >> (8 * b)) & 0xffu) * 64 + lane];
            }
        }
        uint32_t tg = 0;
#pragma unroll
        for (int b = 0; b < kLutLC; ++b) tg ^= tr[b];
        sl ^= tg;
        if (lane == 0) flog[steps - 1] = (uint16_t)(gsel | (tsel << 8));
    }
    wave_lds_sync();
    // x ^= 1_F of every logged step (a qubit flipped twice cancels, in any order)
    for (int b0 = 0; b0 < steps; b0 += 64) {
        if (b0 + lane < steps) {
            const uint32_t e = flog[b0 + lane];
            const int gg = (int)(e & 0xffu);
#pragma unroll
            for (int k = 0; k < kGenW; ++k)
                if ((e >> (8 + k)) & 1u) {
                    const uint32_t q = g.g_q[k * g.g_pad + gg];
                    atomicXor(&xb[q >> 5], 1u << (q & 31));
                }
        }
    }
    wave_lds_sync();
    *sw_out = sw;
    return steps;
}

// The compact-list BP kernel (see above): the lean bp_ms_wave_kernel's BP
// (MsCore) on the listed shots only.  Entries come in chunks of up to
// CmpEntry::kPer (one u64 per lane, the next chunk loaded while this one
// decodes; a list shorter than kPer entries per wave is cut finer); chunks are
// handed out by ShotSeq (static stride, then a counter for the tail).
// A shot starts from the host's first check state (DevGraph::ms_state0) with
// the syndrome's sign flips, not from rows of priors and a check pass over them.
// FUSE (with DEFER): 0 = BP-failed shots go to the SSF queue; 1 / 2 = SSF runs
// here (ssf_fused with RG = FUSE generators per lane).
template <typename T, int RC, int RV, int DRC, bool DEFER, int D3R, int OCC = 0, int FUSE = 0>
__global__ __launch_bounds__(64, OCC > 0 ? OCC : (sizeof(T) == 4 ? 4 : 2)) void bp_ms_cmp_kernel(DevGraph g, DecodeArgs a) {
    using Core = MsCore<T, RC, RV, DRC, true, D3R>;
    using Ent = CmpEntry<RC>;
    constexpr int EW = Ent::EW, KP = Ent::kPer;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    T* v2c = reinterpret_cast<T*>(smem);
    T* st = v2c + MsLds<T>::v2c_elems(MsLds<T>::rows(g));
    uint8_t* xh = reinterpret_cast<uint8_t*>(st + MsLds<T>::state_elems(g.m_pad));
    uint64_t* lzs = reinterpret_cast<uint64_t*>(smem + MsLds<T>::core_bytes(g));  // [k][RV] slot-order logicals

    const int lane = threadIdx.x;
    const int m = g.m;
    if constexpr (sizeof(T) == 8 && OCC == 0) {
        // f64 at 2 waves per SIMD (the one-pass kernel's placement): the kernel
        // needs ~160 VGPRs, which would let a CU put 3 waves on one SIMD and 1 on
        // another; claiming v175 makes the allocation 176, so at most 2 per SIMD
        asm volatile("" ::: "v175");
    }
    Core core;
    core.load(g, lane);
    Core::init_lds(g, v2c, st, xh, lane);
    const bool want_fail = a.fail && a.readout && g.k > 0;
    if (want_fail)
        for (int e = lane; e < g.k * RV; e += 64) lzs[e] = g.ms_lzs[e];
    wave_lds_sync();

    // chunks of KP entries inside the segments, the heavy list first: virtual
    // segment v < 64 is heavy segment v (physical kCmpSegs + v), v >= 64 light
    // segment v - 64; lane s holds heavy and light segment s's entry counts;
    // seg_end = inclusive prefix of the virtual segments' chunk counts
    static_assert(kCmpSegs == 64, "one lane per segment");
    const int64_t hcount = (int64_t)__builtin_nontemporal_load(a.cmp_count + 16 * (kCmpSegs + lane));
    const int64_t lcount = (int64_t)__builtin_nontemporal_load(a.cmp_count + 16 * lane);
    // entries per chunk: KP, fewer when the list is short (below KP entries per
    // wave the decode is latency-bound: spread the shots over more waves)
    auto wave_prefix = [&](int64_t v) {
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int64_t o = (int64_t)readlane64_up((uint64_t)v, off, lane);
            v += lane >= off ? o : 0;
        }
        return v;
    };
    const int64_t tot = (int64_t)readlane64((uint64_t)wave_prefix(hcount + lcount), 63);
    const int kp = (int)min((int64_t)KP, max((int64_t)1, (tot + gridDim.x - 1) / gridDim.x));
    const int64_t hend = wave_prefix((hcount + kp - 1) / kp);
    const int64_t hch = (int64_t)readlane64((uint64_t)hend, 63);
    const int64_t lend = hch + wave_prefix((lcount + kp - 1) / kp);
    const int64_t nch = (int64_t)readlane64((uint64_t)lend, 63);
    // kept in LDS (read once per chunk), not in registers across the BP loop
    int64_t* seg_end = reinterpret_cast<int64_t*>(lzs + (size_t)g.k * RV);  // [128] chunk prefix
    int64_t* seg_cnt = seg_end + 2 * kCmpSegs;                             // [128] entries
    seg_end[lane] = hend;
    seg_end[kCmpSegs + lane] = lend;
    seg_cnt[lane] = hcount;
    seg_cnt[kCmpSegs + lane] = lcount;
    wave_lds_sync();
    // the chunk counter only pays when the tail is long (>= 16 chunks per wave)
    unsigned long long* ctr = a.wave_ctr && nch >= 16 * (int64_t)gridDim.x ? a.wave_ctr : nullptr;
    ShotSeq seq(nch, ctr, blockIdx.x, gridDim.x, lane, 1);
    int ne_n = 0;  // entries in the chunk load_chunk loaded last
    auto load_chunk = [&](int64_t c) -> uint64_t {
        ne_n = 0;
        if (c >= nch) return 0ull;
        // the virtual segment holding chunk c, then its physical segment
        const int v = __popcll(__ballot(seg_end[lane] <= c)) + __popcll(__ballot(seg_end[kCmpSegs + lane] <= c));
        const int64_t c_in = c - (v ? seg_end[v - 1] : 0);
        const int64_t cnt = seg_cnt[v];
        ne_n = (int)min((int64_t)kp, cnt - c_in * kp);
        const int ps = v < kCmpSegs ? kCmpSegs + v : v - kCmpSegs;
        // uniform entry address + 32-bit lane offset (opaque, so `a.cmp + lane` is
        // not kept as a VGPR pair across the BP loop)
        const int64_t e = ((int64_t)ps * a.cmp_cap + c_in * kp) * EW;
        uint32_t lo = (uint32_t)lane * 8u;
        asm volatile("" : "+v"(lo));
        const char* src = reinterpret_cast<const char*>(a.cmp + e) + lo;
        return lane < ne_n * EW ? __builtin_nontemporal_load(reinterpret_cast<const uint64_t*>(src)) : 0ull;
    };
    // one flat loop over this wave's entries (chunk c, entry q of it; the next
    // chunk cn is in flight in entn)
    QDEC_STAMP_DECL
#ifdef QDEC_STAMPS
    const unsigned long long qdec_t0 = __builtin_amdgcn_s_memtime();
#endif
    int64_t c = seq.next(lane);
    uint64_t ent = load_chunk(c);
    int ne = ne_n;
    int64_t cn = c < nch ? seq.next(lane) : nch;
    uint64_t entn = load_chunk(cn);
    int q = 0;
    QDEC_STAMP(4);  // prologue
    while (c < nch) {
        {
            // the first check state: loaded per shot (a few KB that stay in the
            // caches; issued ahead of the entry's readlanes) and dead before the BP
            // loop, so it costs the loop no registers
            typename Core::V2 s0[RC];
            Core::load_state0(g, lane, s0);
            const int64_t shot = (int64_t)readlane64(ent, q * EW);
            bool sbit[RC];
#pragma unroll
            for (int rc = 0; rc < RC; ++rc) sbit[rc] = (readlane64(ent, q * EW + 1 + rc) >> lane) & 1;
            uint64_t rpar[kMaxLogicalRounds];
#pragma unroll
            for (int rr = 0; rr < kMaxLogicalRounds; ++rr) rpar[rr] = readlane64(ent, q * EW + 1 + RC + rr);
            core.write_state0(st, s0, sbit);
            wave_lds_sync();
            QDEC_STAMP(0);  // entry + first check state
            T Q[RV];
            uint64_t X[RV];
            bool pres[RC];
            int it = 1;
            const bool conv = core.template iterate<true>(a, v2c, st, m, lane, sbit, Q, X, pres, it);
            const int iters = conv ? it : a.max_iter;
            QDEC_STAMP(1);  // BP iterations
            QDEC_COUNT(8, iters);
            QDEC_COUNT(9, 1);
            if (lane == 0 && a.iters) a.iters[shot] = iters;
            if (DEFER && FUSE && !conv) {
                // SSF right here: hard decision by column as LDS bit words, residual
                // by check, then the table-driven flips (ssf_fused)
                uint64_t* xb = reinterpret_cast<uint64_t*>(seg_cnt + 2 * kCmpSegs);  // [RV] (kernel LDS tail)
                uint16_t* flog = reinterpret_cast<uint16_t*>(xb + RV);                // [m_pad]
#pragma unroll
                for (int rv = 0; rv < RV; ++rv) xh[core.col_of(rv)] = (uint8_t)((X[rv] >> lane) & 1);
                wave_lds_sync();
                uint64_t rw[RC];
#pragma unroll
                for (int w = 0; w < RV; ++w) {
                    const uint64_t xw = __ballot(xh[w * 64 + lane] & 1);
                    if (lane == 0) xb[w] = xw;
                }
#pragma unroll
                for (int rc = 0; rc < RC; ++rc) rw[rc] = __ballot(pres[rc]);
                wave_lds_sync();
                int sw = 0;
                const int steps = ssf_fused<(FUSE > 0 ? FUSE : 1), RC>(g, a.ssf_max_steps,
                                                                       reinterpret_cast<uint32_t*>(xb), flog, rw,
                                                                       lane, &sw);
                int f = 0;
                if (want_fail) {  // Lz (by column, the graph's dense table) x against the readout parities
#pragma unroll
                    for (int rr = 0; rr < kMaxLogicalRounds; ++rr) {
                        const int r = rr * 64 + lane;
                        if (r < g.k) {
                            int par = (int)((rpar[rr] >> lane) & 1);
                            for (int w = 0; w < g.lz_words && w < RV; ++w)
                                par += __popcll(g.lz[(size_t)r * g.lz_words + w] & xb[w]);
                            f |= par & 1;
                        }
                    }
                }
                const int any_fail = __ballot(f) != 0ull;
                if (lane == 0) {
                    if (a.status) a.status[shot] = (uint8_t)(sw == 0 ? 2 : 0);
                    if (a.ssf_steps) a.ssf_steps[shot] = steps;
                    if (a.fail) a.fail[shot] = (uint8_t)any_fail;
                }
                wave_lds_sync();
            } else if (DEFER && !conv) {
                // hard decision by column for the SSF queue (slot order -> xh[column])
#pragma unroll
                for (int rv = 0; rv < RV; ++rv) xh[core.col_of(rv)] = (uint8_t)((X[rv] >> lane) & 1);
                wave_lds_sync();
                uint64_t xw[RV], rw[RC], dw[RV];
#pragma unroll
                for (int w = 0; w < RV; ++w) {
                    xw[w] = __ballot(xh[w * 64 + lane] & 1);
                    dw[w] = w < kMaxLogicalRounds ? rpar[w < kMaxLogicalRounds ? w : 0] : 0ull;
                }
#pragma unroll
                for (int rc = 0; rc < RC; ++rc) rw[rc] = __ballot(pres[rc]);
                int ql = lane;  // opaque: the queue's per-lane address is formed here, not kept across the BP loop
                asm volatile("" : "+v"(ql));
                queue_push_packed<RV, RC>(a, shot, xw, rw, dw, ql);
                wave_lds_sync();
            } else {
                int f = 0;
                if (want_fail) {  // parity of Lz x (slot order) against the readout's
#pragma unroll
                    for (int rr = 0; rr < kMaxLogicalRounds; ++rr) {
                        const int r = rr * 64 + lane;
                        if (r < g.k) {
                            int par = (int)((rpar[rr] >> lane) & 1);
#pragma unroll
                            for (int w = 0; w < RV; ++w) par += __popcll(lz_word(lzs, (size_t)r * RV + w) & X[w]);
                            f |= par & 1;
                        }
                    }
                }
                const int any_fail = __ballot(f) != 0ull;
                if (lane == 0) {
                    if (a.status) a.status[shot] = (uint8_t)(conv ? 3 : 0);
                    if (a.ssf_steps) a.ssf_steps[shot] = 0;
                    if (a.fail) a.fail[shot] = (uint8_t)any_fail;
                }
            }
        }
        QDEC_STAMP(2);  // failure check, outputs / SSF queue
        if (++q == ne) {  // next chunk
            q = 0;
            c = cn;
            ent = entn;
            ne = ne_n;
            cn = c < nch ? seq.next(lane) : nch;
            entn = load_chunk(cn);
            QDEC_STAMP(3);  // chunk hand-off
        }
    }
#ifdef QDEC_STAMPS
    QDEC_COUNT(10, __builtin_amdgcn_s_memtime() - qdec_t0);
    QDEC_COUNT(12, 1);
#endif
    QDEC_FLUSH_AT(32);
}

// ---------------------------------------------------------------- table entries
// of bp_ms_wave_kernel and bp_ms_cmp_kernel, for the units that build them by
// wave shape (qdec_ms_rv4.hip, qdec_ms_rvx.hip; QDEC_INST: qdec_kernels.h).  A
// template is compiled only in the unit whose builder names it.
template <typename T, int RC, int RV, int DRC, bool DEFER, bool LEAN, int D3R, int OCC>
static void add_ms_wave(KernelTable& t) {
    t.push_back(QDEC_INST(64, bp_ms_wave_kernel, T, RC, RV, DRC, DEFER, LEAN, D3R, OCC));
    t.back().lds = [](const DevGraph& g, const DecodeArgs&) { return MsLds<T>::template bytes<RC, RV>(g); };
}

// FUSE (the table-driven SSF inside the compact kernel) only with DEFER
template <typename T, int RC, int RV, int DRC, bool DEFER, int D3R, int OCC, int FUSE>
static void add_ms_cmp(KernelTable& t) {
    static_assert(DEFER || FUSE == 0, "FUSE only with DEFER");
    t.push_back(QDEC_INST(64, bp_ms_cmp_kernel, T, RC, RV, DRC, DEFER, D3R, OCC, FUSE));
    t.back().lds = [](const DevGraph& g, const DecodeArgs&) {
        size_t b = MsLds<T>::core_bytes(g) + ((size_t)g.k * RV * 8 + 15) / 16 * 16 + 2 * kCmpLists * kCmpSegs * 8;
        if (FUSE) b += ((size_t)RV * 8 + (size_t)g.m_pad * 2 + 15) / 16 * 16;  // fused SSF: xb, flog
        return b;
    };
}

template <typename T, int RC, int RV, int DRC, bool DEFER, int D3R, int OCC>
static void add_ms_occ(KernelTable& wave, KernelTable& cmp) {
    if constexpr (OCC == 0) add_ms_wave<T, RC, RV, DRC, DEFER, false, D3R, OCC>(wave);
    add_ms_wave<T, RC, RV, DRC, DEFER, true, D3R, OCC>(wave);
    add_ms_cmp<T, RC, RV, DRC, DEFER, D3R, OCC, 0>(cmp);
    if constexpr (DEFER) {
        add_ms_cmp<T, RC, RV, DRC, DEFER, D3R, OCC, 1>(cmp);
        add_ms_cmp<T, RC, RV, DRC, DEFER, D3R, OCC, 2>(cmp);
    }
}

template <typename T, int RC, int RV, int DRC, bool DEFER>
static void add_ms_defer(KernelTable& wave, KernelTable& cmp) {
    add_ms_occ<T, RC, RV, DRC, DEFER, 0, 0>(wave, cmp);
    if constexpr (wave_has_d3r2(RC, RV, DRC)) {
        add_ms_occ<T, RC, RV, DRC, DEFER, 2, 0>(wave, cmp);
        if constexpr (wave_has_occ3(sizeof(T) == 4 ? 1 : 0, 2)) add_ms_occ<T, RC, RV, DRC, DEFER, 2, 3>(wave, cmp);
    }
}

// every instantiation of one wave shape
template <int RC, int RV, int DRC>
static void add_ms_shape(KernelTable& wave, KernelTable& cmp) {
    add_ms_defer<float, RC, RV, DRC, false>(wave, cmp);
    add_ms_defer<float, RC, RV, DRC, true>(wave, cmp);
    add_ms_defer<double, RC, RV, DRC, false>(wave, cmp);
    add_ms_defer<double, RC, RV, DRC, true>(wave, cmp);
}

}  // namespace qdec
