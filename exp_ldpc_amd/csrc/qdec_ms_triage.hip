// qdec_ms_triage.hip -- ms_triage_kernel: the first pass of lean min-sum
// launches on wave graphs.  It finishes the shots that need no BP and appends
// the others to the compact list (qdec_cmp_list.h) bp_ms_cmp_kernel decodes.
#include <hip/hip_runtime.h>

#include "qdec_cmp_list.h"
#include "qdec_device.h"
#include "qdec_kernels.h"
#include "qdec_wave_bits.h"

namespace qdec {

// bits 24..27 of (d & 0x01010101) * 0x01020408 are bit 0 of d's four bytes
__device__ __forceinline__ uint32_t byte_bits4(uint32_t d) { return ((d & 0x01010101u) * 0x01020408u) >> 24; }

// One tile of a shot-major byte buffer, as the 16-B chunks covering bytes
// [start, start + len) of a buffer of `total` bytes (image chunk 0 = the chunk
// at or below `start`; `shift` = the byte offset of `start` inside the image).
// The LDS image keeps only bit 0 of every byte (16 bits per chunk, 1/8 of the
// bytes), so a tile pair needs ~3 KB of LDS instead of ~21 KB and more tiles
// are in flight per CU.
using u32x4 = __attribute__((ext_vector_type(4))) uint32_t;
// bit 0 of 16 bytes as a 16-bit word (byte t -> bit t)
__device__ __forceinline__ uint32_t chunk_bits16(u32x4 v) {
    return byte_bits4(v.x) | (byte_bits4(v.y) << 4) | (byte_bits4(v.z) << 8) | (byte_bits4(v.w) << 12);
}
struct TileSrc {
    const uint8_t* buf;
    int64_t total, c0;  // c0: first 16-B chunk
    int nch, shift;
    void* img;          // u16 bits per chunk
    __device__ TileSrc(const uint8_t* b, int64_t tot, int64_t start, int64_t len, void* dst) : buf(b), total(tot), img(dst) {
        c0 = start >> 4;
        nch = (int)(((start + len + 15) >> 4) - c0);
        shift = (int)(start & 15);
    }
    __device__ __forceinline__ void put(int c, u32x4 v) const { static_cast<uint16_t*>(img)[c] = (uint16_t)chunk_bits16(v); }
    // chunk c of the image from its bytes (the buffer's last partial chunk)
    __device__ u32x4 bytes(int c) const {
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        for (int t = 0; t < 16; ++t) {
            const int64_t q = 16 * (c0 + c) + t;
            if (q < total) w[t / 4] |= (uint32_t)buf[q] << (8 * (t % 4));
        }
        return u32x4{w[0], w[1], w[2], w[3]};
    }
};

// Copy a tile into its LDS image: U 16-B loads per lane per round (64 U
// chunks), all issued before any LDS store.  Every load is unconditional, from
// a chunk index clamped into the buffer's whole 16-B chunks (no exec-masked
// loads, so the compiler keeps them all in flight); chunks past the buffer's
// last whole 16 B are assembled from byte loads.  The buffer must be 16-B
// aligned (the launcher checks; torch allocations are).
template <int U>
__device__ __forceinline__ void tile_to_lds(const TileSrc& T, int lane) {
    const int64_t whole = T.total >> 4;
    const u32x4* src = reinterpret_cast<const u32x4*>(T.buf);
    for (int r0 = 0; r0 < T.nch; r0 += 64 * U) {
        u32x4 v[U];
        if (whole > 0) {  // uniform
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t gi = min(T.c0 + r0 + u * 64 + lane, whole - 1);
                v[u] = __builtin_nontemporal_load(src + gi);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c = r0 + u * 64 + lane;
            if (c < T.nch) T.put(c, T.c0 + c < whole ? v[u] : T.bytes(c));
        }
    }
}

// Two tiles (syndrome and readout) into their LDS images with every load of a
// round issued before any LDS store, so the second tile's HBM latency overlaps
// the first's: UA / UB 16-B loads per lane per round (the bench shape does
// both tiles in one round).  Same clamping and tail handling as tile_to_lds.
template <int UA, int UB>
__device__ __forceinline__ void tile_pair_to_lds(const TileSrc& A, const TileSrc& B, int lane) {
    const int64_t wa = A.total >> 4, wb = B.total >> 4;
    const u32x4* sa = reinterpret_cast<const u32x4*>(A.buf);
    const u32x4* sb = reinterpret_cast<const u32x4*>(B.buf);
    for (int ra = 0, rb = 0; ra < A.nch || rb < B.nch; ra += 64 * UA, rb += 64 * UB) {
        u32x4 va[UA], vb[UB];
        if (wa > 0 && ra < A.nch) {  // uniform
#pragma unroll
            for (int u = 0; u < UA; ++u) va[u] = __builtin_nontemporal_load(sa + min(A.c0 + ra + u * 64 + lane, wa - 1));
        }
        if (wb > 0 && rb < B.nch) {  // uniform
#pragma unroll
            for (int u = 0; u < UB; ++u) vb[u] = __builtin_nontemporal_load(sb + min(B.c0 + rb + u * 64 + lane, wb - 1));
        }
#pragma unroll
        for (int u = 0; u < UA; ++u) {
            const int c = ra + u * 64 + lane;
            if (c < A.nch) A.put(c, A.c0 + c < wa ? va[u] : A.bytes(c));
        }
#pragma unroll
        for (int u = 0; u < UB; ++u) {
            const int c = rb + u * 64 + lane;
            if (c < B.nch) B.put(c, B.c0 + c < wb ? vb[u] : B.bytes(c));
        }
    }
}

// Iteration 1 in the triage (DecodeArgs::it1_lut), bit-sliced over the tile's
// 64 shots: the syndrome is transposed to one word per check (bit s = shot s),
// each column's decision word is its 16-bit table (it1_tables, qdec_abi.cpp)
// applied to its <= 4 checks' words, and a shot whose decision meets its
// syndrome has converged in iteration 1 -- the BP kernel would report exactly
// that (iterations 1, status 3, failure = parity of Lz x against the readout).
// LDS (over the tile images, dead by then): check words [RC*64 + 1] (the last
// one zero: pad check id), decision words [RV*64 + 1] (the last zero: pad
// column id), logical parities [256].
template <int RC, int RV>
struct TriageIt1 {
    static constexpr size_t bytes = 8 * (size_t)(RC * 64 + 1 + RV * 64 + 1 + 64 * kMaxLogicalRounds) + 16;
};

constexpr int kT1GateW = 12;  // iteration-1 tile gate: syndrome weight bound ...
constexpr int kT1GateN = 8;   // ... and shots of the tile within it
constexpr int kTriageUB = 16;  // readout-tile loads per lane per round
// (wave_transpose64, the 64 x 64 bit transpose across the wave: qdec_wave_bits.h)

// f(w0..w3) of a 16-entry truth table, bit-sliced: OR over the patterns p with
// table bit p of the minterm (w_k or ~w_k by bit k of p)
__device__ __forceinline__ uint64_t lut4_words(uint32_t lut, uint64_t w0, uint64_t w1, uint64_t w2, uint64_t w3) {
    const uint64_t A[4] = {~w0 & ~w1, w0 & ~w1, ~w0 & w1, w0 & w1};
    const uint64_t C[4] = {~w2 & ~w3, w2 & ~w3, ~w2 & w3, w2 & w3};
    uint64_t f = 0ull;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        uint64_t gsel = 0ull;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            // all-ones / zero from table bit q + 4r
            const int64_t msk = -(int64_t)((lut >> (q + 4 * r)) & 1u);
            gsel |= A[q] & (uint64_t)msk;
        }
        f |= gsel & C[r];
    }
    return f;
}

// The same from a bit image: bit `off` onwards, `len` bits;
// reads up to three dwords past the row's last bit (the image has spares).
template <int NW>
__device__ __forceinline__ void row_bits_b(const uint32_t* img, int off, int len, uint64_t (&w)[NW]) {
    const int q = off >> 5;
    const uint32_t sh = (uint32_t)(off & 31);
#pragma unroll
    for (int i = 0; i < NW; ++i) {
        w[i] = 0ull;
        if (64 * i < len) {  // uniform
            const uint32_t d0 = img[q + 2 * i], d1 = img[q + 2 * i + 1], d2 = img[q + 2 * i + 2];
            uint64_t v = (uint64_t)__builtin_amdgcn_alignbit(d1, d0, sh) |
                         ((uint64_t)__builtin_amdgcn_alignbit(d2, d1, sh) << 32);
            if (64 * i + 64 > len) v &= (1ull << (len - 64 * i)) - 1ull;
            w[i] = v;
        }
    }
}

// LDS bytes of a triage tile image of `len` bytes (plus the spares the row
// readers run past its end)
__host__ __device__ inline size_t triage_img_bytes(int64_t len) {
    const int64_t nch = (len + 15) / 16 + 2;
    return (size_t)((2 * (nch + 8) + 15) / 16 * 16);
}

// One wave per tile of 64 shots (lane l = shot 64 * blockIdx.x + l).  PK:
// bit-packed input rows (QD_INPUT_PACKED; a.in_packed), read as u64 words, no
// tile images (its own instantiation: the byte path's 16-B tile loads keep ~100
// VGPRs in flight, which the packed path does not need).
template <int RC, int NWD, bool PK = false>
__global__ __launch_bounds__(64, 1) void ms_triage_kernel(DevGraph g, DecodeArgs a) {
    using Ent = CmpEntry<RC>;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x;
    const int m = g.m, nd = g.n_data;
    const int64_t s0 = (int64_t)blockIdx.x * 64;
    const int ns = (int)min((int64_t)64, a.B - s0);
    const bool want_fail = a.fail && a.readout && g.k > 0;
    // the launch's counters that run behind this pass (compact-kernel chunk
    // counter, SSF slot counter, SSF queue length) are zeroed here, saving a
    // memset launch each (the previous decode on the handle has finished with
    // them: the workspace chain orders decodes)
    if (blockIdx.x == 0 && lane == 0) {
        if (a.wave_ctr) a.wave_ctr[0] = a.wave_ctr[1] = 0ull;
        if (a.q_count) *a.q_count = 0;
    }
    // the handle's other list-counter set, for its next two-pass decode (the
    // decode that last used it has finished: the workspace chain orders them)
    if (blockIdx.x == 0 && a.cmp_count_next)
        for (int s = lane; s < kCmpLists * kCmpSegs; s += 64) a.cmp_count_next[16 * s] = 0ull;
    // LDS: the logicals (k x lz_words u64, read as broadcasts), then the
    // syndrome and readout tiles as 16-B chunk images (one spare chunk each:
    // row_bits reads one dword past a row)
    uint64_t* lz_lds = reinterpret_cast<uint64_t*>(smem);
    const int nlz = want_fail ? g.k * g.lz_words : 0;
    constexpr bool pk = PK;  // bit-packed input rows: no tile images
    unsigned char* syn_img = smem + ((size_t)nlz * 8 + 15) / 16 * 16;
    unsigned char* rd_img = syn_img + (pk ? 0 : triage_img_bytes(64 * (int64_t)m));
    // iteration-1 words: past the images
    unsigned char* it1_base = rd_img + (pk ? 0 : triage_img_bytes(64 * (int64_t)nd));
    for (int e = lane; e < nlz; e += 64) lz_lds[e] = g.lz[e];
    // iteration-1 tables (TriageIt1), loaded ahead of the tiles
    uint64_t it_ids[NWD], it_cv[RC][2];
    uint32_t it_lut[NWD];
    if (a.it1_lut) {
#pragma unroll
        for (int rv = 0; rv < NWD; ++rv) {
            it_ids[rv] = g.it1_vchk[rv * 64 + lane];
            it_lut[rv] = a.it1_lut[rv * 64 + lane];
        }
#pragma unroll
        for (int rc = 0; rc < RC; ++rc) {
            it_cv[rc][0] = g.it1_cvar[2 * (rc * 64 + lane)];
            it_cv[rc][1] = g.it1_cvar[2 * (rc * 64 + lane) + 1];
        }
    }
    const bool live = lane < ns;
    const int64_t shot = s0 + lane;
    uint64_t sw[RC];
    uint64_t rw[NWD];
    if constexpr (PK) {
        // one row of u64 words per shot: lane-strided loads, padding bits cleared.
        // Precondition (plan_decode, expand_packed): RC == ceil(m / 64), the row
        // length the ABI, the sampler and pack_rows write.  A wave shape may have
        // more check rounds than that (m <= 64 on (2, 3, *), m <= 128 on
        // (4, 9, 8)); those decodes expand their rows and take the byte branch.
        const uint64_t* sp = reinterpret_cast<const uint64_t*>(a.syn) + min(shot, a.B - 1) * RC;
#pragma unroll
        for (int rc = 0; rc < RC; ++rc) {
            uint64_t v = __builtin_nontemporal_load(sp + rc);
            if (64 * rc + 64 > m) v &= (m - 64 * rc >= 64) ? ~0ull : ((1ull << (m - 64 * rc)) - 1ull);
            sw[rc] = live ? v : 0ull;
        }
        if (want_fail) {
            const int rdw = (nd + 63) / 64;
            const uint64_t* rq = reinterpret_cast<const uint64_t*>(a.readout) + min(shot, a.B - 1) * rdw;
#pragma unroll
            for (int w = 0; w < NWD; ++w) {
                uint64_t v = w < rdw ? __builtin_nontemporal_load(rq + w) : 0ull;
                if (64 * w + 64 > nd) v &= (nd - 64 * w >= 64) ? ~0ull : (nd > 64 * w ? (1ull << (nd - 64 * w)) - 1ull : 0ull);
                rw[w] = v;
            }
        }
        __syncthreads();  // the logicals' LDS copy (above) before its reads
    } else {
        const TileSrc ts(a.syn, a.B * (int64_t)m, s0 * m, (int64_t)ns * m, syn_img);
        const TileSrc tr(want_fail ? a.readout : a.syn, want_fail ? a.B * (int64_t)nd : 0, s0 * nd,
                         want_fail ? (int64_t)ns * nd : 0, rd_img);
        if (want_fail)
            tile_pair_to_lds<(4 * RC < 8 ? 4 * RC : 8), (4 * NWD < kTriageUB ? 4 * NWD : kTriageUB)>(ts, tr, lane);
        else tile_to_lds<8>(ts, lane);
        __syncthreads();
        row_bits_b<RC>(reinterpret_cast<const uint32_t*>(syn_img), ts.shift + lane * m, m, sw);
        if (want_fail) row_bits_b<NWD>(reinterpret_cast<const uint32_t*>(rd_img), tr.shift + lane * nd, nd, rw);
    }
    uint64_t rp[kMaxLogicalRounds] = {0ull, 0ull, 0ull, 0ull};
    if (want_fail) {
        for (int r = 0; r < g.k; ++r) {  // uniform rows of the dense logical table (LDS broadcasts)
            int par = 0;
#pragma unroll
            for (int w = 0; w < NWD; ++w)
                if (w < g.lz_words) par += __popcll(lz_word(lz_lds, (size_t)r * g.lz_words + w) & rw[w]);
#pragma unroll
            for (int rr = 0; rr < kMaxLogicalRounds; ++rr)
                if (rr == (r >> 6)) rp[rr] |= (uint64_t)(par & 1) << (r & 63);
        }
    }
    bool trivial;
    uint8_t fbit;
    // iteration 1 pays only where shots converge in it: tiles with >= 8 shots of
    // syndrome weight <= 12 (about three isolated errors); others just list
    int wt = 0;
#pragma unroll
    for (int rc = 0; rc < RC; ++rc) wt += __popcll(sw[rc]);
    const bool it1 = a.it1_lut && __popcll(__ballot(live && wt <= kT1GateW)) >= kT1GateN;
    if (it1) {  // uniform: iteration 1 here (TriageIt1)
        wave_lds_sync();
        uint64_t* synT = reinterpret_cast<uint64_t*>(it1_base);
        uint64_t* xT = synT + RC * 64 + 1;
        uint64_t* lzp = xT + NWD * 64 + 1;
        // transpose: lane t gets the word of check rc * 64 + t
#pragma unroll
        for (int rc = 0; rc < RC; ++rc) {
            const uint64_t mine = wave_transpose64(live ? sw[rc] : 0ull, lane);
            synT[rc * 64 + lane] = mine;  // checks >= m: zero words
        }
        if (lane == 0) {
            synT[RC * 64] = 0ull;
            xT[NWD * 64] = 0ull;
        }
        wave_lds_sync();
        // decision words, one column per lane
#pragma unroll
        for (int rv = 0; rv < NWD; ++rv) {
            const uint64_t ids = it_ids[rv];
            xT[rv * 64 + lane] = lut4_words(it_lut[rv], synT[ids & 0xffff], synT[(ids >> 16) & 0xffff],
                                            synT[(ids >> 32) & 0xffff], synT[ids >> 48]);
        }
        wave_lds_sync();
        // residual syndrome words, one check per lane, OR-reduced over the wave
        uint64_t bad = 0ull;
#pragma unroll
        for (int rc = 0; rc < RC; ++rc) {
            const uint64_t c0 = it_cv[rc][0], c1 = it_cv[rc][1];
            uint64_t par = synT[rc * 64 + lane];
#pragma unroll
            for (int t = 0; t < 4; ++t) par ^= xT[(c0 >> (16 * t)) & 0xffff] ^ xT[(c1 >> (16 * t)) & 0xffff];
            bad |= par;
        }
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)bad, off);
            const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(bad >> 32), off);
            bad |= ((uint64_t)hi << 32) | lo;
        }
        trivial = live && !((bad >> lane) & 1ull);
        int f = 0;
        if (want_fail && __ballot(trivial)) {
            // parity words of the logicals (one logical per lane: the set bits of
            // its row of the dense table), then each shot's bits
            for (int r = lane; r < g.k; r += 64) {
                uint64_t p = 0ull;
                for (int w = 0; w < g.lz_words; ++w)
                    for (uint64_t bits = lz_word(lz_lds, (size_t)r * g.lz_words + w); bits; bits &= bits - 1ull)
                        p ^= xT[w * 64 + __builtin_ctzll(bits)];
                lzp[r] = p;
            }
            wave_lds_sync();
#pragma unroll
            for (int rr = 0; rr < kMaxLogicalRounds; ++rr) {
                const int nr = min(64, g.k - rr * 64);
                for (int t = 0; t < nr; ++t) f |= (int)(((lzp[rr * 64 + t] >> lane) ^ (rp[rr] >> t)) & 1ull);
            }
        }
        fbit = (uint8_t)f;
    } else {
        uint64_t any = 0ull;
#pragma unroll
        for (int rc = 0; rc < RC; ++rc) any |= sw[rc];
        trivial = live && any == 0ull && a.cmp_zero_ok;
        fbit = (uint8_t)((rp[0] | rp[1] | rp[2] | rp[3]) != 0ull);
    }
    if (live && trivial) {
        if (a.iters) a.iters[shot] = 1;
        if (a.status) a.status[shot] = 3;
        if (a.ssf_steps) a.ssf_steps[shot] = 0;
        if (a.fail) a.fail[shot] = want_fail ? fbit : (uint8_t)0;
    }
    const bool listed = live && !trivial;
    const unsigned long long bal = __ballot(listed);
    if (bal == 0ull) return;
    // segment blockIdx % kCmpSegs: 64 counters on their own lines, so the
    // per-tile atomics do not serialise on one address.  Shots of syndrome
    // weight > kHeavyW go to the heavy list (segments kCmpSegs..), which the BP
    // kernel hands out first: the long decodes start at the launch's beginning
    // instead of setting its end (longest-processing-time-first)
    const bool heavy = listed && wt > kHeavyW;
    const unsigned long long balh = __ballot(heavy), ball = bal & ~balh;
    const int seg = (int)(blockIdx.x % kCmpSegs);
    unsigned long long bh = 0, bl = 0;
    if (lane == 0) {
        if (balh) bh = atomicAdd(a.cmp_count + 16 * (kCmpSegs + seg), (unsigned long long)__popcll(balh));
        if (ball) bl = atomicAdd(a.cmp_count + 16 * seg, (unsigned long long)__popcll(ball));
    }
    bh = __shfl(bh, 0);
    bl = __shfl(bl, 0);
    if (listed) {
        const unsigned long long mb = heavy ? balh : ball;
        const uint64_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(mb >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mb, 0u));
        const int sg = heavy ? kCmpSegs + seg : seg;
        uint64_t* e = a.cmp + ((uint64_t)sg * a.cmp_cap + (heavy ? bh : bl) + rank) * Ent::EW;
        e[0] = (uint64_t)shot;
#pragma unroll
        for (int rc = 0; rc < RC; ++rc) e[1 + rc] = sw[rc];
#pragma unroll
        for (int rr = 0; rr < kMaxLogicalRounds; ++rr) e[1 + RC + rr] = rp[rr];
    }
}

template <int RC, int RV, bool PK>
static void add_triage(KernelTable& t) {
    t.push_back(QDEC_INST(64, ms_triage_kernel, RC, RV, PK));
    // the logicals, the tile images (byte rows), the iteration-1 words (over
    // the images; the kernel's layout, ms_triage_kernel)
    t.back().lds = [](const DevGraph& g, const DecodeArgs& a) {
        const bool want_fail = a.fail && a.readout && g.k > 0;
        const size_t tiles = PK ? 0 : triage_img_bytes(64 * (int64_t)g.m) + triage_img_bytes(64 * (int64_t)g.n_data);
        const size_t it1 = a.it1_lut ? TriageIt1<RC, RV>::bytes : 0;
        return ((want_fail ? (size_t)g.k * g.lz_words * 8 : 0) + 15) / 16 * 16 + tiles + it1;
    };
}

// the kernel depends on the rounds only: the shapes share it ((2, 3, *), (2, 4, *))
void add_triage_kernels(KernelTable& t) {
#define QDEC_SHAPE(R, V, D)               \
    if (!find_kernel(t, {R, V, 0})) {     \
        add_triage<R, V, false>(t);       \
        add_triage<R, V, true>(t);        \
    }
    QDEC_WAVE_SHAPES(QDEC_SHAPE)
#undef QDEC_SHAPE
}

}  // namespace qdec
