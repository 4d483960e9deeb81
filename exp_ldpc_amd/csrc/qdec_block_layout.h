// qdec_block_layout.h -- LDS and HBM layouts of the workgroup kernel families
// (qdec_bp_block.hip, qdec_bp_group.hip, qdec_ms_lds.hip, qdec_ms_lds64.hip):
// the sizes and limits that the kernels and the workgroup plan and launchers
// (qdec_launch_block.hip) both read.  No kernel is defined here.
#pragma once
#include <hip/hip_runtime.h>

#include "qdec_graph.h"

namespace qdec {

// ---- bp_block_kernel and the workgroup SSF kernels
constexpr int kBlock = 256;

// Every block kernel starts its dynamic LDS with the control area of
// qdec_graph.h (kCtrl bytes; fields kCtrlRed64, kCtrlRed32, kCtrlSlot, kCtrlNext).

// control area + xh + one or two m_pad byte arrays + logical parities
__host__ __device__ inline size_t block_small_lds(const DevGraph& g) {
    return kCtrl + (size_t)g.n_pad + 2 * (size_t)g.m_pad + 4 * (size_t)(g.k > 0 ? g.k : 1);
}

// Bytes of one workgroup's HBM scratch slice: the messages and/or the per-shot
// byte arrays that do not fit the LDS budget (placement bits as in bp_block_kernel).
__host__ __device__ inline size_t block_slice_bytes(const DevGraph& g, size_t tsz, int placement) {
    size_t b = 0;
    if (!(placement & 1)) b += ((size_t)2 * g.E * tsz + 15) / 16 * 16;
    if (!(placement & 2)) b += (block_small_lds(g) + 255) / 256 * 256;
    return (b + 255) / 256 * 256;
}

// HBM shot state of one SSF / finalize workgroup (ssf_block_kernel's gstate)
__host__ __device__ inline size_t block_state_stride(const DevGraph& g) {
    return (block_small_lds(g) + 255) / 256 * 256;
}

// ssf_inc_block_kernel:
//   LDS: ctrl | key[g_pad] i32 | slg[g_pad] u32 | dlist[g_pad] u16 | dbits
//        [g_pad/32] | xh[n_pad] | sres[m_pad] | lpar[k]
__host__ __device__ inline size_t ssf_inc_lds(const DevGraph& g) {
    const size_t gp = (size_t)g.g_pad;
    return kCtrl + gp * 4 + gp * 4 + (gp * 2 + 15) / 16 * 16 + ((gp + 31) / 32 * 4 + 15) / 16 * 16 +
           ((size_t)g.n_pad + 15) / 16 * 16 + ((size_t)g.m_pad + 15) / 16 * 16 +
           (4 * (size_t)(g.k > 0 ? g.k : 1) + 15) / 16 * 16 + ((size_t)g.n_data + 15) / 16 * 16;
}

constexpr int kFinPerCu = 8;          // SSF/finalize workgroups per CU when their state is in HBM
constexpr size_t kGrpHeader = 256;    // scratch header: the shot counter

// ---- bp_group_kernel
struct GroupLayout {  // byte offsets inside one group's scratch block
    size_t v2c, c2v, sw, xw, pw, rw, total;
};

__host__ __device__ inline size_t grp_round(size_t b) { return (b + 255) / 256 * 256; }

__host__ __device__ inline GroupLayout group_layout(const DevGraph& g, size_t tsz) {
    GroupLayout L;
    L.v2c = 0;
    L.c2v = L.v2c + grp_round(((size_t)g.E + kEdgePad) * 64 * tsz);
    L.sw = L.c2v + grp_round(((size_t)g.E + kEdgePad) * 64 * tsz);
    L.xw = L.sw + grp_round((size_t)g.m * 8);
    L.pw = L.xw + grp_round((size_t)g.n * 8);
    L.rw = L.pw + grp_round((size_t)g.m * 8);
    L.total = L.rw + grp_round((size_t)g.n_data * 8);
    return L;
}

// ---- bp_ms_lds_kernel
constexpr int kMlThreads = 1024;
constexpr int kMlNch = 5;  // check rounds per thread: 32 B of rows per check in 160 KB

constexpr int kMlDummyRows = 64 / kMlDRS;  // pad edges of lane l use element m * kMlDRS + l

__host__ __device__ inline size_t ml_pbuf_words(const DevGraph& g) {
    return ((size_t)g.m + kMlDummyRows + 31) / 32 + 3 & ~(size_t)3;
}
__host__ __device__ inline size_t ml_lds_bytes(const DevGraph& g) {
    return kCtrl + ((size_t)g.m + kMlDummyRows) * kMlDRS * 4 + 2 * 4 * ml_pbuf_words(g) + 2 * 4 * (kMlThreads / 64);
}

// iteration 1's image (ml_init_*_kernel)
__host__ __device__ inline size_t ml_image_bytes(const DevGraph& g) { return (size_t)g.m * kMlDRS * 4; }

// ---- bp_ms_lds64_kernel
constexpr int kM64Threads = 1024;
constexpr int kM64Nch = 5;  // check rounds per thread: 32 B of state per check in 160 KB

__host__ __device__ inline size_t m64_words(const DevGraph& g) { return ((size_t)g.m + 31) / 32; }
__host__ __device__ inline size_t m64_lds_bytes(const DevGraph& g) {
    return kCtrl + (size_t)2 * g.m * 16 + 5 * 4 * m64_words(g) + 2 * 4 * (kM64Threads / 64);
}

// iteration 1's image (m64_init_kernel)
__host__ __device__ inline size_t m64_image_bytes(const DevGraph& g) {
    return (size_t)g.m * 16 + 4 * ((m64_words(g) + 1) / 2 * 2);
}

}  // namespace qdec
