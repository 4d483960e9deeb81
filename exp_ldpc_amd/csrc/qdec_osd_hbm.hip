// qdec_osd_hbm.hip -- the OSD stage (steps 1-6 at the top of qdec_osd.hip) for
// graphs whose augmented rows do not fit a CU's LDS: circuit detector error
// models (648 x 25,684 at R = 3: 2 MiB of rows), deep spacetime graphs.  The
// steps it has in common with the on-chip kernels, and with them every tie rule,
// come from qdec_osd_steps.h (key fill, compare-exchange, syndrome bit,
// non-pivot list, search width, candidate key, pair index, finalize); the result
// is bit-identical to qd_osd_batch.  Its own: the slot, the chunked sort driver,
// the elimination, and steps 5 and 6 (candidate search, pick, outputs), which
// osd_block_kernel also has in its own text: shared through the header they
// cost this kernel 1 % on the 432 x 1224 graph.  A change to the
// candidate order or to emit is made in both workgroup kernels.
//
// One 256-thread workgroup per BP-unconverged shot, persistent over the batch.
// Workgroup b owns slot b of a scratch the graph handle owns (qdec_abi.cpp) and
// rebuilds it per shot.  A slot is touched by its own workgroup only, so a
// workgroup barrier orders all its traffic (as with frame_*_kernel<FrameInHbm>).
//
// Slot (HBM, OsdHbmLayout::s_*): the rows [H_sorted | s] as m x W 64-bit words,
// the sort keys and column indices padded to a power of two, pos (column ->
// sorted position), piv (rank row -> pivot position), isp (position is a pivot)
// and out (the solution bytes).  LDS (l_*): control words, x0, the first <= 64
// non-pivot positions and their transformed columns, the hit flags, and four
// row buffers of W words: one per wave while the rows are built, the first one
// the staged pivot row of an elimination step.  The sort's 2048-element chunk
// overlays them (it is done before any of them is live).  Indices are 32-bit.
//
//   sort      bitonic on (key, column) pairs; strides below the chunk run in LDS,
//             so a 32,768-key sort makes 10 passes over HBM, not 120
//   rows      a wave builds one row in its LDS buffer (ds XOR per entry) and
//             writes it out whole: no zero fill, no global atomics
//   pivot     one pass over word ww of the rows at or below the rank finds the
//             next column that has a candidate and its first row at once (LDS
//             atomic min of column << 32 | row): columns without a pivot cost
//             nothing, a word without one costs one pass
//   step      pivot row swapped into place and staged in LDS, hit flags taken,
//             then the waves XOR it into the flagged rows, lanes across words
//   OSD-CS    a wave scores 64 adjacent positions at once: each lane loads word
//             w of one row (64 rows per load) and the 64 words are broadcast
//             lane by lane (readlane), so a transformed column is never
//             gathered bit by bit and no transposed copy is kept
#include <hip/hip_runtime.h>

#include "../../include/qdec.h"
#include "qdec_device.h"
#include "qdec_internal.h"
#include "qdec_kernels.h"
#include "qdec_osd_steps.h"

namespace qdec {

namespace {

constexpr int kHbmBlock = 256;
constexpr int kHbmWaves = kHbmBlock / 64;
constexpr int kHbmSortChunk = 2048; // keys sorted in LDS at a time

__device__ __forceinline__ uint32_t readlane32(uint32_t v, int l) {
    return (uint32_t)__builtin_amdgcn_readlane((int)v, l);
}

}  // namespace

// Slot and LDS layouts (byte offsets); identical on host and device.
OsdHbmLayout::OsdHbmLayout(int64_t n, int64_t m) {
    ns = osd_sort_size(n);
    W = (n + 1 + 63) / 64;
    RW = (m + 63) / 64;
    OsdTake<int64_t> take;
    s_rows = take(8 * m * W);
    s_key = take(8 * ns);
    s_idx = take(4 * ns);
    s_pos = take(4 * n);
    s_piv = take(4 * (m > 0 ? m : 1));
    s_isp = take(n);
    s_out = take(n);
    slot_bytes = (take.o + 255) / 256 * 256;
    take.o = 0;
    l_ctl = take(64);
    l_npv = take(4 * kOsdMaxLam);
    l_x0 = take(8 * RW);
    l_tcl = take(8 * kOsdMaxLam * RW);
    l_row = take(8 * kHbmWaves * W);
    l_hit = take(m);
    const int64_t chunk = ns < kHbmSortChunk ? ns : kHbmSortChunk;
    l_skey = 0;  // the sort's chunk overlays everything above
    l_sidx = 8 * chunk;
    const int64_t sort_bytes = 12 * chunk;
    lds_bytes = take.o > sort_bytes ? take.o : sort_bytes;
}

__global__ __launch_bounds__(kHbmBlock) void osd_hbm_kernel(DevGraph g, OsdArgs a, unsigned char* scratch,
                                                             OsdHbmLayout L) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m = g.m, n = g.n;
    const int W = (int)L.W, RW = (int)L.RW, NS = (int)L.ns;
    unsigned char* slot = scratch + (size_t)blockIdx.x * (size_t)L.slot_bytes;
    uint64_t* A = reinterpret_cast<uint64_t*>(slot + L.s_rows);  // [m][W]
    uint64_t* gkey = reinterpret_cast<uint64_t*>(slot + L.s_key);
    uint32_t* sidx = reinterpret_cast<uint32_t*>(slot + L.s_idx);  // sorted position -> column
    uint32_t* pos = reinterpret_cast<uint32_t*>(slot + L.s_pos);   // column -> sorted position
    uint32_t* pivc = reinterpret_cast<uint32_t*>(slot + L.s_piv);  // rank row -> pivot position
    uint8_t* isp = slot + L.s_isp;
    uint8_t* outb = slot + L.s_out;
    unsigned long long* ctl = reinterpret_cast<unsigned long long*>(smem + L.l_ctl);  // [0], [3] search; [1] best
    uint32_t* npv = reinterpret_cast<uint32_t*>(smem + L.l_npv);  // the first <= 64 non-pivot positions
    uint64_t* x0 = reinterpret_cast<uint64_t*>(smem + L.l_x0);    // [RW] transformed syndrome over pivot rows
    uint64_t* tcl = reinterpret_cast<uint64_t*>(smem + L.l_tcl);  // [lam][RW] transformed columns
    uint64_t* rowbuf = reinterpret_cast<uint64_t*>(smem + L.l_row);  // [4][W]; [0] = the staged pivot row
    uint8_t* hit = smem + L.l_hit;
    uint64_t* lkey = reinterpret_cast<uint64_t*>(smem + L.l_skey);
    uint32_t* lidx = reinterpret_cast<uint32_t*>(smem + L.l_sidx);
    const int32_t* rp = g.row_ptr;
    const int32_t* ci = g.col_idx;
    const int CH = NS < kHbmSortChunk ? NS : kHbmSortChunk;
    auto bit = [&](int i, int k) -> int { return (int)((A[(size_t)i * W + (k >> 6)] >> (k & 63)) & 1); };

    // the sort's steps of stride < CH for sizes lo .. hi, chunk by chunk in LDS
    auto sort_local = [&](int lo, int hi) {
        for (int c0 = 0; c0 < NS; c0 += CH) {
            for (int t = tid; t < CH; t += kHbmBlock) {
                lkey[t] = gkey[c0 + t];
                lidx[t] = sidx[c0 + t];
            }
            __syncthreads();
            for (int size = lo; size <= hi; size <<= 1) {
                const int s0 = (size >> 1) < (CH >> 1) ? (size >> 1) : (CH >> 1);
                for (int stride = s0; stride > 0; stride >>= 1) {
                    bitonic_pass(lkey, lidx, CH, size, stride, c0, tid, kHbmBlock);
                    __syncthreads();
                }
            }
            for (int t = tid; t < CH; t += kHbmBlock) {
                gkey[c0 + t] = lkey[t];
                sidx[c0 + t] = lidx[t];
            }
            __syncthreads();
        }
    };

    for (int64_t shot = blockIdx.x; shot < a.B; shot += gridDim.x) {
        if (a.status && (a.status[shot] & 1)) continue;  // uniform over the workgroup
        // ---- 1. stable sort of the columns by log-probability ratio
        osd_fill_keys(a, shot, n, NS, gkey, sidx, tid, kHbmBlock);
        __syncthreads();
        sort_local(2, CH);
        for (int size = 2 * CH; size <= NS && size > 0; size <<= 1) {
            for (int stride = size >> 1; stride >= CH; stride >>= 1) {
                bitonic_pass(gkey, sidx, NS, size, stride, 0, tid, kHbmBlock);
                __syncthreads();
            }
            sort_local(size, size);
        }
        for (int k = tid; k < n; k += kHbmBlock) {
            const uint32_t c = sidx[k];  // the n real keys sort in front of the padding
            if (c < (uint32_t)n) pos[c] = (uint32_t)k;
            isp[k] = 0;
        }
        __syncthreads();

        // ---- 2. augmented rows [H_sorted | s]: a wave builds a row in LDS and writes it out
        {
            uint64_t* rb = rowbuf + (size_t)wave * W;
            for (int i = wave; i < m; i += kHbmWaves) {
                for (int w = lane; w < W; w += 64) rb[w] = 0;
                __builtin_amdgcn_wave_barrier();  // one wave: LDS operations complete in order
                int sb = lane == 0 ? syn_bit(a.syn, shot, m, i) : 0;
                for (int e = rp[i] + lane; e < rp[i + 1]; e += 64) {
                    const int j = ci[e];
                    const uint32_t k = pos[j];
                    if (k >= (uint32_t)n) continue;
                    atomicXor(reinterpret_cast<unsigned long long*>(&rb[k >> 6]), 1ull << (k & 63));
                    sb ^= syn_term(a.syn_flags, a.base, a.readout, shot, g.n_data, j);
                }
                const int par = __popcll(__ballot(sb & 1)) & 1;
                if (lane == 0 && par) atomicXor(reinterpret_cast<unsigned long long*>(&rb[n >> 6]), 1ull << (n & 63));
                __builtin_amdgcn_wave_barrier();
                for (int w = lane; w < W; w += 64) A[(size_t)i * W + w] = rb[w];
                __builtin_amdgcn_wave_barrier();
            }
        }
        if (tid == 0) ctl[0] = ~0ull;
        __syncthreads();

        // ---- 3. Gauss-Jordan in sorted column order
        int rank = 0;
        {
            int ww = 0, b = 0, it = 0;
            while (rank < m && ww * 64 < n) {
                unsigned long long* sk = &ctl[(it & 1) ? 3 : 0];
                uint64_t wmask = ~0ull << b;
                if (ww == (n >> 6)) wmask &= (1ull << (n & 63)) - 1ull;  // columns only, not the syndrome bit
                unsigned long long cand = ~0ull;
                for (int i = rank + tid; i < m; i += kHbmBlock) {
                    const uint64_t v = A[(size_t)i * W + ww] & wmask;
                    if (v) {
                        const unsigned long long key = ((unsigned long long)__builtin_ctzll(v) << 32) | (unsigned)i;
                        cand = key < cand ? key : cand;
                    }
                }
                if (cand != ~0ull) atomicMin(sk, cand);
                __syncthreads();
                const unsigned long long key = *sk;
                if (tid == 0) ctl[(it & 1) ? 0 : 3] = ~0ull;  // the next search's word
                ++it;
                if (key == ~0ull) {  // uniform: no column of this word has a pivot left
                    ++ww;
                    b = 0;
                    __syncthreads();
                    continue;
                }
                const int c = (int)(key >> 32), piv = (int)(key & 0xffffffffu);
                const int k = ww * 64 + c;
                for (int i = tid; i < m; i += kHbmBlock)
                    if (i != rank && i != piv) hit[i] = (uint8_t)((A[(size_t)i * W + ww] >> c) & 1);
                for (int w = ww + tid; w < W; w += kHbmBlock) {
                    const uint64_t p = A[(size_t)piv * W + w];
                    if (piv != rank) {
                        const uint64_t q = A[(size_t)rank * W + w];
                        A[(size_t)piv * W + w] = q;
                        A[(size_t)rank * W + w] = p;
                        if (w == ww) hit[piv] = (uint8_t)((q >> c) & 1);  // the swapped-out row
                    }
                    if (w == ww) hit[rank] = 0;
                    rowbuf[w] = p;
                }
                __syncthreads();
                for (int base = wave * 64; base < m; base += kHbmBlock) {
                    const int i = base + lane;
                    uint64_t bal = __ballot(i < m && hit[i]);
                    while (bal) {
                        const int r = base + __builtin_ctzll(bal);
                        bal &= bal - 1;
                        uint64_t* row = A + (size_t)r * W;
                        for (int w = ww + lane; w < W; w += 64) row[w] ^= rowbuf[w];
                    }
                }
                if (tid == 0) {
                    pivc[rank] = (uint32_t)k;
                    isp[k] = 1;
                }
                ++rank;
                b = c + 1;
                if (b == 64) {
                    ++ww;
                    b = 0;
                }
                __syncthreads();
            }
        }

        // ---- 4. transformed syndrome, the first lam non-pivot positions and their columns
        const int kn = n - rank;
        const int lam_s = osd_lam(a, kn);
        for (int w = tid; w < RW; w += kHbmBlock) x0[w] = 0;
        for (int e = tid; e < lam_s * RW; e += kHbmBlock) tcl[e] = 0;
        if (wave == 0) osd_nonpivots(isp, n, npv, lam_s, lane);
        __syncthreads();
        for (int i = tid; i < rank; i += kHbmBlock)
            if (bit(i, n)) atomicOr(reinterpret_cast<unsigned long long*>(&x0[i >> 6]), 1ull << (i & 63));
        for (int64_t e = tid; e < (int64_t)lam_s * rank; e += kHbmBlock) {
            const int t = (int)(e / rank), i = (int)(e % rank);
            if (bit(i, (int)npv[t]))
                atomicOr(reinterpret_cast<unsigned long long*>(&tcl[t * RW + (i >> 6)]), 1ull << (i & 63));
        }
        __syncthreads();
        int w0 = 0;
        for (int w = 0; w < RW; ++w) w0 += __popcll(x0[w]);
        if (tid == 0) ctl[1] = osd_key(w0, 0);  // OSD-0: weight, place 0
        __syncthreads();

        // ---- 5. candidates: osd_key(weight, place in the host's order), the place
        // 1 + k for the single at position k (ascending in k as the host's walk of
        // the non-pivot columns is), 1 + n + pair index, or the OSD-E mask
        unsigned long long best = ~0ull;
        if (a.method == 2) {
            const int rwr = (rank + 63) / 64;
            for (int w = wave; w * 64 < n; w += kHbmWaves) {
                const int k = w * 64 + lane;
                const bool valid = k < n && !isp[k];
                if (!__ballot(valid)) continue;
                int wgt = 1;
                for (int rbk = 0; rbk < rwr; ++rbk) {
                    const int i = rbk * 64 + lane;
                    uint64_t v = 0;
                    if (i < rank) {
                        v = A[(size_t)i * W + w];
                        if ((x0[rbk] >> lane) & 1) v = ~v;
                    }
                    const uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
#pragma unroll
                    for (int r = 0; r < 64; ++r) {
                        const uint32_t slo = readlane32(lo, r), shi = readlane32(hi, r);
                        wgt += (int)(((lane < 32 ? slo : shi) >> (lane & 31)) & 1u);
                    }
                }
                if (valid) {
                    const unsigned long long key = osd_key(wgt, 1u + (unsigned)k);
                    best = key < best ? key : best;
                }
            }
            const int np = lam_s * (lam_s - 1) / 2;
            for (int q = tid; q < np; q += kHbmBlock) {
                int u, v;
                pair_of(q, lam_s, u, v);
                int wgt = 2;
                for (int w = 0; w < RW; ++w) wgt += __popcll(x0[w] ^ tcl[u * RW + w] ^ tcl[v * RW + w]);
                const unsigned long long key = osd_key(wgt, 1u + (unsigned)n + (unsigned)q);
                best = key < best ? key : best;
            }
        } else if (a.method == 1 && lam_s > 0) {
            const uint32_t lim = 1u << lam_s;
            for (uint32_t sm = 1 + tid; sm < lim; sm += kHbmBlock) {
                int wgt = __popc(sm);
                for (int w = 0; w < RW; ++w) {
                    uint64_t c = x0[w];
                    for (int t = 0; t < lam_s; ++t)
                        if ((sm >> t) & 1) c ^= tcl[t * RW + w];
                    wgt += __popcll(c);
                }
                const unsigned long long key = osd_key(wgt, sm);
                best = key < best ? key : best;
            }
        }
        // OSD-0 keeps a tie (strict improvement): its key has the lowest place
        if (best != ~0ull) atomicMin(&ctl[1], best);
        __syncthreads();
        const unsigned long long bk = ctl[1];
        const uint32_t bpos = (uint32_t)(bk & 0xffffffffu);
        int kind = 0, ca = -1, cb = -1;  // kind 1: ca = the position; kind 2: ca, cb index npv
        uint32_t cmask = 0;
        if (bpos != 0) {
            if (a.method != 2) {
                kind = 3;
                cmask = bpos;
            } else if (bpos <= (uint32_t)n) {
                kind = 1;
                ca = (int)(bpos - 1);
            } else {
                kind = 2;
                pair_of((int)(bpos - 1 - (uint32_t)n), lam_s, ca, cb);
            }
        }

        // ---- 6. outputs (osd0, then the chosen candidate + fused fold / failure check)
        auto flip = [&](uint32_t position) {  // tid 0: the solution bit of a sorted position
            const uint32_t c = position < (uint32_t)n ? sidx[position] : 0xffffffffu;
            if (c < (uint32_t)n) outb[c] ^= 1;
        };
        auto emit = [&](int kd) {
            for (int j = tid; j < n; j += kHbmBlock) outb[j] = 0;
            __syncthreads();
            for (int i = tid; i < rank; i += kHbmBlock) {
                int xb = (int)((x0[i >> 6] >> (i & 63)) & 1);
                if (kd == 1) xb ^= bit(i, ca);
                if (kd == 2) xb ^= (int)(((tcl[ca * RW + (i >> 6)] ^ tcl[cb * RW + (i >> 6)]) >> (i & 63)) & 1);
                if (kd == 3)
                    for (int t = 0; t < lam_s; ++t)
                        if ((cmask >> t) & 1) xb ^= (int)((tcl[t * RW + (i >> 6)] >> (i & 63)) & 1);
                const uint32_t c = sidx[pivc[i]];
                if (xb && c < (uint32_t)n) outb[c] = 1;
            }
            __syncthreads();
            if (tid == 0) {
                if (kd == 1) flip((uint32_t)ca);
                if (kd == 2) {
                    flip(npv[ca]);
                    flip(npv[cb]);
                }
                if (kd == 3)
                    for (int t = 0; t < lam_s; ++t)
                        if ((cmask >> t) & 1) flip(npv[t]);
            }
            __syncthreads();
        };
        if (a.osd0_out) {
            emit(0);
            for (int j = tid; j < n; j += kHbmBlock) a.osd0_out[shot * n + j] = outb[j];
            __syncthreads();
        }
        emit(kind);
        if (wave == 0) osd_finalize(g, a, shot, outb, lane);
        __syncthreads();
    }
}

// Whether the HBM kernel holds the graph, by m, n and k alone (no HIP call): its
// LDS image (the hit flags, four row buffers, 64 transformed columns) must fit
// one CU and the fused failure check keeps its k <= 256 limit.
bool osd_hbm_choose(const DevGraph& g, OsdHbmLayout* L) {
    if (g.m <= 0 || g.n <= 0 || g.k > 256) return false;
    if ((int64_t)g.n + 1 + kOsdMaxLam * 32 >= (1ll << 31)) return false;
    *L = OsdHbmLayout(g.n, g.m);
    return L->lds_bytes <= 160 * 1024;
}

// The one place that turns a placement into a kernel (qdec_internal.h has the rule).
void osd_place(const DevGraph& g, int placement, OsdPlaced* p) {
    *p = OsdPlaced{kOsdNone, OsdChoice{0, 0, 0}, OsdHbmLayout()};
    if (placement != QD_OSD_HBM && osd_choose(g, &p->c))
        p->kernel = p->c.rs ? kOsdRegister : kOsdWorkgroup;
    else if (placement != QD_OSD_ONCHIP && osd_hbm_choose(g, &p->L))
        p->kernel = kOsdHbm;
}

int launch_osd_hbm(const DevGraph& g, const OsdArgs& a, void* scratch, int64_t slots, hipStream_t stream) {
    if (a.B <= 0 || slots <= 0) return 0;
    OsdHbmLayout L;
    if (!osd_hbm_choose(g, &L)) return (int)hipErrorNotSupported;
    if (L.lds_bytes > 64 * 1024) {
        const hipError_t ea = hipFuncSetAttribute(reinterpret_cast<const void*>(osd_hbm_kernel),
                                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.lds_bytes);
        if (ea != hipSuccess) return (int)ea;
    }
    const int64_t grid = slots < a.B ? slots : a.B;
    hipLaunchKernelGGL(osd_hbm_kernel, dim3((unsigned)grid), dim3(kHbmBlock), (size_t)L.lds_bytes, stream, g, a,
                       static_cast<unsigned char*>(scratch), L);
    return (int)hipGetLastError();
}

}  // namespace qdec
