// qdec_tables.cpp -- host-side graph preparation (qdec_tables.h): CSR ->
// per-lane slot tables for the wave kernels, flip-set tables for SSF, bit-packed
// logicals, priors in both precisions.  No HIP header and no graph handle: the
// library (qdec_abi.cpp) and the stand-alone checker (tools/tables_check.cpp)
// both drive it through a HostGraph.
#include "qdec_tables.h"

#include <cmath>
#include <mutex>
#include <random>

#include "../../include/qdec.h"

namespace qdec {

namespace {

template <typename T>
int drs() { return lds_stride<T, kDR>(); }
template <typename T>
int dcs() { return lds_stride<T, kDC>(); }

// Check-state slots of bp_ms_lds64_kernel (f64, one shot per CU; qdec_ms_lds64.hip).
// Its variable thread t owns columns r * 1024 + (67 t mod 1024); per (wave,
// round r, edge k) one LDS instruction of 64 lanes reads or atomically updates
// the state of each lane's k-th check.  The banking gfx950 applies
// (tools/dev/lds_atomic_probe.hip): the u64 m1 / m2 reads (ds_read_b64) in two
// 32-lane halves, key slot mod 32; the u64 atomics (ds_min(_rtn)_u64) in four
// 16-lane quarters, key slot mod 16; the bit words (parw / hdw: word = slot >> 5)
// in halves, key word mod 32.  With checks in their natural order a group's
// lanes land on ~3-4 lanes per bank.  A seeded anneal over slot swaps spreads
// every group over its banks (objective: sum of squared lanes per bank, all
// three keys; tools/dev/c4_bank_model2.py's max-per-bank cycles on C4: 23,102
// natural -> 16,086, conflict-free 7,600; an anneal of the max model itself,
// tools/dev/c4_slots_anneal2.cpp, stops at the same 16.2k).  The kernel then works in
// slot space; m64_check maps a slot back to its check for the syndrome input and
// the residual output.  Cached per process like ms_layout.
void m64_layout(HostGraph* G, int m, int n, const std::vector<int32_t>& rp, const std::vector<int32_t>& ci,
                const std::vector<int>& edge_cpos) {
    DevGraph& g = G->dg;
    struct Entry {
        std::vector<int32_t> rp, ci;
        std::vector<uint16_t> et, chk;
        int d3r;
    };
    static std::mutex mu;
    static std::vector<Entry> cache;
    {
        std::lock_guard<std::mutex> lk(mu);
        for (const auto& c : cache)
            if (c.rp == rp && c.ci == ci) {
                g.m64_etab = G->arena->upload(c.et);
                g.m64_check = G->arena->upload(c.chk);
                g.m64_d3r = c.d3r;
                return;
            }
    }
    constexpr int T = 1024;  // kM64Threads
    const int E = rp[m];
    // k-th check of every column (edge_cpos order, as ml_etab)
    std::vector<int> colchk((size_t)kMlDC * n, -1);
    for (int i = 0; i < m; ++i)
        for (int e = rp[i]; e < rp[i + 1]; ++e)
            if (edge_cpos[e] < kMlDC) colchk[(size_t)edge_cpos[e] * n + ci[e]] = i;
    // the lane groups of one instruction: 32-lane halves (ds_read_b64 of m1 / m2,
    // key slot mod 32; b32 words, key (slot >> 5) mod 32) and 16-lane quarters
    // (ds_min(_rtn)_u64 on m1 / m2, key slot mod 16) -- the banking measured by
    // tools/dev/lds_atomic_probe.hip; occurrences of each check in both
    std::vector<std::vector<int>> halves, quarters;
    const int rounds = (n + T - 1) / T;
    for (int w = 0; w < T / 64; ++w)
        for (int r = 0; r < rounds; ++r)
            for (int k = 0; k < kMlDC; ++k)
                for (int q = 0; q < 4; ++q) {
                    std::vector<int> qq;
                    for (int l = 16 * q; l < 16 * q + 16; ++l) {
                        const int j = r * T + ((64 * w + l) * 67) % T;
                        if (j < n && colchk[(size_t)k * n + j] >= 0) qq.push_back(colchk[(size_t)k * n + j]);
                    }
                    if (q & 1) {  // the half: this quarter and the one before it
                        std::vector<int> hh(quarters.back());
                        hh.insert(hh.end(), qq.begin(), qq.end());
                        if (!hh.empty()) halves.push_back(std::move(hh));
                    }
                    quarters.push_back(std::move(qq));
                }
    const int nh = (int)halves.size(), nq = (int)quarters.size();
    std::vector<std::vector<int>> occ(m), occq(m);
    for (int h = 0; h < nh; ++h)
        for (int i : halves[h]) occ[i].push_back(h);
    for (int q = 0; q < nq; ++q)
        for (int i : quarters[q]) occq[i].push_back(q);
    std::vector<int> slot(m);
    for (int i = 0; i < m; ++i) slot[i] = i;
    std::vector<int> cx((size_t)nh * 32, 0), cy((size_t)nh * 32, 0), cz((size_t)nq * 16, 0);
    auto X = [](int s) { return s & 31; };
    auto Y = [](int s) { return (s >> 5) & 31; };
    auto Z = [](int s) { return s & 15; };
    for (int h = 0; h < nh; ++h)
        for (int i : halves[h]) ++cx[(size_t)h * 32 + X(slot[i])], ++cy[(size_t)h * 32 + Y(slot[i])];
    for (int q = 0; q < nq; ++q)
        for (int i : quarters[q]) ++cz[(size_t)q * 16 + Z(slot[i])];
    // per edge: two u64 reads (halves), two u64 atomics (quarters), one b32 read
    // and the occasional b32 xor (halves)
    const double WX = 2.0, WZ = 2.0, WY = 1.5;
    auto move = [&](int i, int from, int to) {
        for (int h : occ[i]) {
            --cx[(size_t)h * 32 + X(from)], --cy[(size_t)h * 32 + Y(from)];
            ++cx[(size_t)h * 32 + X(to)], ++cy[(size_t)h * 32 + Y(to)];
        }
        for (int q : occq[i]) --cz[(size_t)q * 16 + Z(from)], ++cz[(size_t)q * 16 + Z(to)];
    };
    auto local = [&](int i, int s) {  // check i's share of the squared loads at slot s
        double c = 0;
        for (int h : occ[i]) c += WX * (2 * cx[(size_t)h * 32 + X(s)] - 1) + WY * (2 * cy[(size_t)h * 32 + Y(s)] - 1);
        for (int q : occq[i]) c += WZ * (2 * cz[(size_t)q * 16 + Z(s)] - 1);
        return c;
    };
    std::mt19937_64 rng(20250221);
    std::uniform_real_distribution<double> uni(0.0, 1.0);
    const long iters = m > 1 ? std::min<long>(6000000L, 1500L * E) : 0;
    const double T0 = 1.0, T1 = 0.01;
    for (long it = 0; it < iters; ++it) {
        const int i = (int)(rng() % (uint64_t)m), j = (int)(rng() % (uint64_t)m);
        const int si = slot[i], sj = slot[j];
        if (i == j || (X(si) == X(sj) && Y(si) == Y(sj))) continue;
        const double before = local(i, si) + local(j, sj);
        move(i, si, sj);
        move(j, sj, si);
        const double d = local(i, sj) + local(j, si) - before;
        const double temp = T0 * std::pow(T1 / T0, (double)it / (double)iters);
        if (d <= 0 || uni(rng) < std::exp(-d / temp)) {
            slot[i] = sj;
            slot[j] = si;
        } else {
            move(j, si, sj);
            move(i, sj, si);
        }
    }
    // leading rounds whose columns all have degree <= 3 (the kernel's D3R)
    int d3r = 0;
    while (d3r < rounds) {
        bool ok = true;
        for (int j = d3r * T; j < std::min(n, (d3r + 1) * T) && ok; ++j) ok = colchk[(size_t)(kMlDC - 1) * n + j] < 0;
        if (!ok) break;
        ++d3r;
    }
    Entry e{rp, ci, std::vector<uint16_t>((size_t)kMlDC * n, 0xffff), std::vector<uint16_t>(m), d3r};
    for (size_t t = 0; t < colchk.size(); ++t)
        if (colchk[t] >= 0) e.et[t] = (uint16_t)slot[colchk[t]];
    for (int i = 0; i < m; ++i) e.chk[slot[i]] = (uint16_t)i;
    g.m64_etab = G->arena->upload(e.et);
    g.m64_check = G->arena->upload(e.chk);
    g.m64_d3r = d3r;
    std::lock_guard<std::mutex> lk(mu);
    if (cache.size() >= 8) cache.erase(cache.begin());
    cache.push_back(std::move(e));
}

// Layout of the compressed-state min-sum kernel (qdec_bp_ms.h).  Variable
// lane j = rv*64 + l scatters its k-th v2c message to element i*DRS + pos of
// check i's row.  One ds_write_b32 per (rv, k) serves 2 x 32 lanes, bank =
// dword % 32.  It costs max(4, L0 + L1) cycles, where L_h is the worst bank
// load in half h.  The check pass takes min/sign over the whole row, which is
// independent of the row order, so edge positions inside a row are free.  A
// seeded hill climb over position swaps drives every instruction to <= 2-way
// conflicts (tie-break: sum of squared loads).  Pad lanes of an instruction all
// write one dummy element, placed in the least-loaded bank.
void ms_layout(HostGraph* G, int m, int n, const std::vector<int>& edge_cpos) {
    DevGraph& g = G->dg;
    const auto& rp = G->row_ptr;
    const auto& ci = G->col_idx;
    const int E = rp[m];
    const int drc = g.shape_drc;
    const int RVn = g.n_pad / 64;
    // Lane slots of the variables: ascending column degree (stable), so the
    // leading 64-variable rounds whose variables all have degree <= 3 run a
    // 3-edge variable pass (ms_d3r).  Each variable's arithmetic is unchanged.
    std::vector<int> order(n);
    for (int j = 0; j < n; ++j) order[j] = j;
    auto cdeg = [&](int j) { return G->col_ptr[j + 1] - G->col_ptr[j]; };
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return cdeg(x) < cdeg(y); });
    std::vector<int> slot_of(n);
    G->ms_var_of_slot.assign(g.n_pad, -1);
    for (int s2 = 0; s2 < n; ++s2) {
        slot_of[order[s2]] = s2;
        G->ms_var_of_slot[s2] = order[s2];
    }
    g.ms_d3r = 0;
    for (int r = 0; r < RVn; ++r) {
        bool ok = true;
        for (int l = 0; l < 64; ++l) {
            const int j = G->ms_var_of_slot[r * 64 + l];
            if (j >= 0 && cdeg(j) > 3) ok = false;
        }
        if (!ok) break;
        g.ms_d3r = r + 1;
    }
    const int D3P = g.ms_d3r & ~1;  // leading 3-edge round pairs: no k = 3 instruction
    std::vector<int> row_of(E);
    for (int i = 0; i < m; ++i)
        for (int e = rp[i]; e < rp[i + 1]; ++e) row_of[e] = i;
    const int NG = RVn * kDC;
    auto has_pad = [&](int gi, int l) {
        const int j = G->ms_var_of_slot[(gi / kDC) * 64 + l];
        return j < 0 || gi % kDC >= cdeg(j);
    };
    const int DRS[2] = {drs<double>(), drs<float>()};
    // The placement below is a deterministic function of the graph; it is cached
    // per process (several handles on one graph, e.g. one per sweep point).
    struct LayoutCache {
        std::vector<int32_t> rp, ci;
        int m_pad, n_pad;
        std::vector<uint32_t> etab[2];
        std::vector<uint16_t> ss16[2];
    };
    static std::mutex cache_mu;
    static std::vector<LayoutCache> cache;
    {
        std::lock_guard<std::mutex> lk(cache_mu);
        for (const auto& c : cache)
            if (c.m_pad == g.m_pad && c.n_pad == g.n_pad && c.rp == rp && c.ci == ci) {
                for (int p = 0; p < 2; ++p) {
                    g.ms_sslot[p] = G->arena->upload(c.ss16[p]);
                    g.ms_etab[p] = G->arena->upload(c.etab[p]);
                }
                goto tables_done;
            }
    }
    {
    LayoutCache entry{rp, ci, g.m_pad, g.n_pad, {}, {}};
    std::mt19937 rng(12345);
    for (int p = 0; p < 2; ++p) {
        // ---- v2c scatter: one ds_write per (rv, k).  f32 (ds_write_b32): 2 lane
        // groups of 32, class = dword % 32, cost max(4, L0 + L1).  f64
        // (ds_write_b64): 4 groups of 16 contiguous lanes, class = element % 16,
        // cost max(6, sum of L).  Row positions are free (min/sign over the row).
        // f64: the transfer of a ds_write_b64 takes 6 cycles but every array
        // cycle beyond 4 is a bank-conflict cycle the CU's other waves wait
        // for (PMC: the array is the busiest unit), so the floor is 4
        const int ngl = p == 1 ? 2 : 4, ncl = p == 1 ? 32 : 16, floor_c = 4;
        const int lanes_per = 64 / ngl;
        std::vector<int> grp(E), lg(E), pos(E);
        for (int i = 0; i < m; ++i)
            for (int e = rp[i], t = 0; e < rp[i + 1]; ++e, ++t) {
                const int sl = slot_of[ci[e]];
                grp[e] = (sl / 64) * kDC + edge_cpos[e];
                lg[e] = (sl % 64) / lanes_per;
                pos[e] = t;
            }
        std::vector<int> load((size_t)NG * ngl * ncl, 0);
        auto cls = [&](int e) { return (row_of[e] * DRS[p] + pos[e]) % ncl; };
        for (int e = 0; e < E; ++e) load[((size_t)grp[e] * ngl + lg[e]) * ncl + cls(e)]++;
        auto gcost = [&](int gi) {
            int sum = 0, sq = 0;
            for (int h = 0; h < ngl; ++h) {
                int mx = 0;
                for (int b = 0; b < ncl; ++b) {
                    const int v = load[((size_t)gi * ngl + h) * ncl + b];
                    mx = std::max(mx, v);
                    sq += v * v;
                }
                sum += mx;
            }
            return (long)std::max(floor_c, sum) * 100000 + sq;
        };
        for (int iter = 0; iter < 40 * E; ++iter) {
            const int i = (int)(rng() % (unsigned)m);
            const int deg = rp[i + 1] - rp[i];
            if (deg < 1) continue;
            const int e1 = rp[i] + (int)(rng() % (unsigned)deg);
            const int p2 = (int)(rng() % (unsigned)drc);
            int e2 = -1;
            for (int e = rp[i]; e < rp[i + 1]; ++e)
                if (pos[e] == p2) e2 = e;
            if (e2 == e1) continue;
            const int g1 = grp[e1], g2 = e2 >= 0 ? grp[e2] : -1;
            const long before = gcost(g1) + (g2 >= 0 && g2 != g1 ? gcost(g2) : 0);
            auto move = [&](int e, int newpos) {
                load[((size_t)grp[e] * ngl + lg[e]) * ncl + cls(e)]--;
                pos[e] = newpos;
                load[((size_t)grp[e] * ngl + lg[e]) * ncl + cls(e)]++;
            };
            const int p1 = pos[e1];
            move(e1, p2);
            if (e2 >= 0) move(e2, p1);
            const long after = gcost(g1) + (g2 >= 0 && g2 != g1 ? gcost(g2) : 0);
            if (after > before) {  // undo
                if (e2 >= 0) move(e2, p2);
                move(e1, p1);
            }
        }
        // pad lanes of an instruction write one dummy element past the rows, in
        // the class least loaded over the lane groups that hold pads
        const int dstart = (m + 1) * DRS[p];  // past the m rows and the shared Big row (MsLds::rows)
        std::vector<int> dummy(NG, dstart);
        for (int gi = 0; gi < NG; ++gi) {
            std::vector<bool> pads(ngl, false);
            for (int l = 0; l < 64; ++l)
                if (has_pad(gi, l)) pads[l / lanes_per] = true;
            int bestb = 0, bestc = 1 << 30;
            for (int b = 0; b < ncl; ++b) {
                int c = 0;
                for (int h = 0; h < ngl; ++h)
                    if (pads[h]) c = std::max(c, load[((size_t)gi * ngl + h) * ncl + b]);
                if (c < bestc) { bestc = c; bestb = b; }
            }
            dummy[gi] = dstart + ((bestb - dstart % ncl) % ncl + ncl) % ncl;
        }
        // ---- check state (m1, m2): check i's state lives at slot sst[i] in
        // [0, m_pad); slot m_pad is the zero state read by pad lanes.  Variable
        // lanes gather it once per (rv, k): f32 ds_read_b64 (2 groups of 32 lanes,
        // class = slot % 32), f64 ds_read_b128 (4 groups of 16 lanes in the
        // hardware's grouping, class = slot % 16).  Only distinct slots in one
        // class of one group conflict; the anneal below minimises the sum over
        // instructions and groups of the worst class load.
        // every check lane, pads included, writes its state once per iteration:
        // f64 ds_write_b128 (8 groups of 8 contiguous lanes, class = slot % 8),
        // f32 ds_write_b64 (4 groups of 16, class = slot % 16); the anneal adds
        // the worst class load of each group (round 2 placed only the gathers:
        // modelled 37 state-write array cycles per iteration for f64, ideal 16)
        std::vector<int> sst(g.m_pad);
        for (int i = 0; i < g.m_pad; ++i) sst[i] = i;
        {
            const int rcl = p == 1 ? 32 : 16;
            auto rgroup = [&](int l) -> int {
                if (p == 1) return l / 32;
                const int q = l % 32, h = (l / 32) * 2;  // {0-3,12-15,20-27} / {4-11,16-19,28-31}
                return h + ((q < 4 || (q >= 12 && q < 16) || (q >= 20 && q < 28)) ? 0 : 1);
            };
            const int nrg = p == 1 ? 2 : 4;
            std::vector<std::vector<int>> mem;  // distinct checks per (instruction, group)
            std::vector<char> gpad;
            for (int gi = 0; gi < NG; ++gi) {
                if (gi / kDC < D3P && gi % kDC == 3) continue;
                std::vector<std::vector<int>> gm(nrg);
                std::vector<char> gp(nrg, 0);
                for (int l = 0; l < 64; ++l) {
                    const int j = G->ms_var_of_slot[(gi / kDC) * 64 + l];
                    if (j < 0 || gi % kDC >= cdeg(j)) { gp[rgroup(l)] = 1; continue; }
                    const int i = G->col_rows[G->col_ptr[j] + gi % kDC];
                    auto& v = gm[rgroup(l)];
                    if (std::find(v.begin(), v.end(), i) == v.end()) v.push_back(i);
                }
                for (int h = 0; h < nrg; ++h) {
                    mem.push_back(gm[h]);
                    gpad.push_back(gp[h]);
                }
            }
            const int NGR = (int)mem.size();
            std::vector<std::vector<int>> app(m);
            for (int q = 0; q < NGR; ++q)
                for (int i : mem[q]) app[i].push_back(q);
            auto qcost = [&](int q) {
                int cnt[32] = {0};
                int mx = 0;
                for (int i : mem[q]) mx = std::max(mx, ++cnt[sst[i] % rcl]);
                if (gpad[q]) mx = std::max(mx, ++cnt[g.m_pad % rcl]);
                return mx;
            };
            const int wl = p == 1 ? 16 : 8;  // state-write group width = classes
            const int NW = g.m_pad / wl;
            auto wcost = [&](int w) {
                int cnt[16] = {0};
                int mx = 0;
                for (int t = 0; t < wl; ++t) mx = std::max(mx, ++cnt[sst[w * wl + t] % wl]);
                return mx;
            };
            std::vector<int> qc(NGR), wc(NW);
            long cur = 0;
            for (int q = 0; q < NGR; ++q) cur += (qc[q] = qcost(q));
            for (int w = 0; w < NW; ++w) cur += (wc[w] = wcost(w));
            std::vector<int> occ(g.m_pad, -1);
            for (int i = 0; i < g.m_pad; ++i) occ[sst[i]] = i;
            std::vector<int> best = sst;
            long bestc = cur;
            const int iters = 60000;
            std::vector<int> aff;
            std::vector<int> newc;
            const int nmov = g.m_pad;
            for (int it = 0; it < iters; ++it) {
                const double T = 0.6 * (1.0 - (double)it / iters) + 0.02;
                const int c1 = (int)(rng() % (unsigned)nmov);
                const int s2 = (int)(rng() % (unsigned)g.m_pad);
                const int c2 = occ[s2];
                if (c2 == c1) continue;
                aff = app[c1 < m ? c1 : 0];
                if (c1 >= m) aff.clear();
                if (c2 >= 0 && c2 < m) aff.insert(aff.end(), app[c2].begin(), app[c2].end());
                std::sort(aff.begin(), aff.end());
                aff.erase(std::unique(aff.begin(), aff.end()), aff.end());
                const int w1 = NW ? c1 / wl : -1, w2 = NW && c2 >= 0 && c2 / wl != w1 ? c2 / wl : -1;
                long old = 0;
                for (int q : aff) old += qc[q];
                if (w1 >= 0) old += wc[w1];
                if (w2 >= 0) old += wc[w2];
                const int s1 = sst[c1];
                sst[c1] = s2;
                if (c2 >= 0) sst[c2] = s1;
                newc.resize(aff.size());
                long nw = 0;
                for (size_t t = 0; t < aff.size(); ++t) nw += (newc[t] = qcost(aff[t]));
                const int nw1 = w1 >= 0 ? wcost(w1) : 0, nw2 = w2 >= 0 ? wcost(w2) : 0;
                nw += nw1 + nw2;
                const long d = nw - old;
                const double u = (double)(rng() & 0xFFFFFF) / 16777216.0;
                if (d <= 0 || u < std::exp(-(double)d / T)) {
                    occ[s2] = c1;
                    occ[s1] = c2;
                    for (size_t t = 0; t < aff.size(); ++t) qc[aff[t]] = newc[t];
                    if (w1 >= 0) wc[w1] = nw1;
                    if (w2 >= 0) wc[w2] = nw2;
                    cur += d;
                    if (cur < bestc) { bestc = cur; best = sst; }
                } else {
                    sst[c1] = s1;
                    if (c2 >= 0) sst[c2] = s2;
                }
            }
            sst = best;
        }
        // pad check lanes write zeros into their own slots (min-sum of an empty
        // row never reaches them: their rows hold Big)
        std::vector<uint16_t> ss16(g.m_pad, (uint16_t)g.m_pad);
        for (int i = 0; i < g.m_pad; ++i) ss16[i] = (uint16_t)sst[i];
        g.ms_sslot[p] = G->arena->upload(ss16);
        std::vector<uint32_t> etab((size_t)kDC * g.n_pad);
        for (int gi = 0; gi < NG; ++gi) {
            const int rv = gi / kDC, k = gi % kDC;
            for (int l = 0; l < 64; ++l)
                etab[(size_t)k * g.n_pad + rv * 64 + l] = (uint32_t)dummy[gi] | ((uint32_t)g.m_pad << 16);
        }
        for (int i = 0; i < m; ++i)
            for (int e = rp[i]; e < rp[i + 1]; ++e)
                etab[(size_t)edge_cpos[e] * g.n_pad + slot_of[ci[e]]] =
                    (uint32_t)(i * DRS[p] + pos[e]) | ((uint32_t)sst[i] << 16);
        g.ms_etab[p] = G->arena->upload(etab);
        entry.etab[p] = std::move(etab);
        entry.ss16[p] = std::move(ss16);
    }
    std::lock_guard<std::mutex> lk(cache_mu);
    if (cache.size() >= 16) cache.erase(cache.begin());
    cache.push_back(std::move(entry));
    }
tables_done:
    // column of each slot (pads: a per-lane dummy past n_pad in the kernel's xh)
    std::vector<uint16_t> vsl(g.n_pad);
    for (int s2 = 0; s2 < g.n_pad; ++s2)
        vsl[s2] = (uint16_t)(G->ms_var_of_slot[s2] >= 0 ? G->ms_var_of_slot[s2] : g.n_pad + s2 % 64);
    g.ms_vslot = G->arena->upload(vsl);
    const int W = g.n_pad / 64;
    std::vector<uint64_t> smask((size_t)W * g.m_pad, 0);
    for (int i = 0; i < m; ++i)
        for (int e = rp[i]; e < rp[i + 1]; ++e) {
            const int sl = slot_of[ci[e]];
            smask[(size_t)(sl / 64) * g.m_pad + i] ^= 1ull << (sl % 64);
        }
    g.ms_smask = G->arena->upload(smask);
}

// Iteration 1 of lean min-sum as a table per column, for ms_triage_kernel.
// With every prior L > 0 nothing in the first check pass depends on signs but
// the syndrome: check i sends column j the message (s_i ? -1 : 1) * alpha_1 *
// (L_j == m1_i ? m2_i : m1_i), m1 / m2 the two smallest priors on row i (Big
// where the row has fewer: the kernels' unused row positions), alpha_1 = 1 -
// 2^-1 = 0.5 (exact).  So column j's decision after iteration 1 (posterior
// L_j + sum of the messages <= 0) is a function of its <= 4 checks' syndrome
// bits.  It is evaluated here in the kernels' precision and summation order
// (MsCore::iterate: edges by ascending row, acc += c_k), so the table is the
// kernel's decision bit for bit; bit b = the decision under pattern b (bit k =
// the syndrome bit of edge k's check).
template <typename T>
std::vector<uint16_t> it1_lut(const HostGraph* G, const std::vector<T>& L, T big) {
    const DevGraph& g = G->dg;
    std::vector<T> m1(g.m, big), m2(g.m, big);
    for (int i = 0; i < g.m; ++i)
        for (int e = G->row_ptr[i]; e < G->row_ptr[i + 1]; ++e) {
            const T av = std::fabs(L[G->col_idx[e]]);  // the med3 chain / top-2 tree of the check pass
            if (av < m1[i]) {
                m2[i] = m1[i];
                m1[i] = av;
            } else if (av < m2[i]) {
                m2[i] = av;
            }
        }
    std::vector<uint16_t> lut(g.n_pad, 0);
    for (int j = 0; j < g.n; ++j) {
        const int t0 = G->col_ptr[j], deg = G->col_ptr[j + 1] - t0;
        T y[kDC];
        for (int k = 0; k < deg; ++k) {
            const int i = G->col_rows[t0 + k];
            y[k] = (L[j] == m1[i] ? m2[i] : m1[i]) * (T)0.5;
        }
        uint32_t bits = 0;
        for (int b = 0; b < (1 << deg); ++b) {
            T acc = L[j];
            for (int k = 0; k < deg; ++k) acc = acc + (((b >> k) & 1) ? -y[k] : y[k]);
            if (acc <= (T)0) bits |= 1u << b;
        }
        lut[j] = (uint16_t)bits;
    }
    return lut;
}

// The precision-independent part: checks of each column, columns of each row.
void it1_tables(HostGraph* G, bool pos64, const std::vector<double>& L64, bool pos32,
                const std::vector<float>& L32) {
    DevGraph& g = G->dg;
    g.it1_vchk = nullptr;
    g.it1_cvar = nullptr;
    g.it1_lut[QD_F64] = g.it1_lut[QD_F32] = nullptr;
    if (!g.wave || g.max_cdeg > kDC || g.max_rdeg > kDR || g.m > 0xfffe || g.n > 0xfffe) return;
    std::vector<uint64_t> vchk(g.n_pad, 0), cvar(2 * (size_t)g.m_pad, 0);
    for (int j = 0; j < g.n_pad; ++j) {
        uint64_t w = 0;
        for (int k = 0; k < kDC; ++k) {
            const int t = j < g.n ? G->col_ptr[j] + k : 0;
            const int i = (j < g.n && t < G->col_ptr[j + 1]) ? G->col_rows[t] : g.m;
            w |= (uint64_t)i << (16 * k);
        }
        vchk[j] = w;
    }
    for (int i = 0; i < g.m_pad; ++i)
        for (int t = 0; t < kDR; ++t) {
            const int e = i < g.m ? G->row_ptr[i] + t : 0;
            const int j = (i < g.m && e < G->row_ptr[i + 1]) ? G->col_idx[e] : g.n;
            cvar[2 * (size_t)i + t / 4] |= (uint64_t)j << (16 * (t % 4));
        }
    g.it1_vchk = G->prior_arena->upload(vchk);
    g.it1_cvar = G->prior_arena->upload(cvar);
    if (pos64) g.it1_lut[QD_F64] = G->prior_arena->upload(it1_lut<double>(G, L64, 1e308));
    if (pos32) g.it1_lut[QD_F32] = G->prior_arena->upload(it1_lut<float>(G, L32, 1e30f));
}

// The first check state of the compact min-sum kernel (bp_ms_cmp_kernel,
// DevGraph::ms_state0).  Before iteration 1 every v2c row holds its columns'
// priors (Big in the unused positions), so what the first check pass writes
// depends only on the priors and the check's syndrome bit, and the bit only
// flips both signs.  Per check lane i (pads: an all-Big row) this is that pass
// under syndrome bit 0, in the kernel's precision: m1 / m2 the two smallest
// |prior| of the row counted with multiplicity (Big where the row has fewer;
// the med3 chain and the top-2 tree select exactly these), both negated when
// the row's parity (the count of priors <= 0, ldpc's sign test) is odd.
// signbit_rule: the f64 kernel's sign-bit check pass, where a row with a zero
// entry (m1 = 0) gives m2 the parity flipped when a zero is +0
// (MsCore::iterate); rows without one have the same signs under both rules.
template <typename T>
std::vector<T> ms_state0_table(const HostGraph* G, const std::vector<T>& L, T big, bool signbit_rule) {
    const DevGraph& g = G->dg;
    std::vector<T> st(2 * (size_t)g.m_pad);
    for (int i = 0; i < g.m_pad; ++i) {
        T m1 = big, m2 = big;
        bool par = false, pz = false;
        if (i < g.m)
            for (int e = G->row_ptr[i]; e < G->row_ptr[i + 1]; ++e) {
                const T v = L[G->col_idx[e]];
                const T av = std::fabs(v);
                if (av < m1) {
                    m2 = m1;
                    m1 = av;
                } else if (av < m2) {
                    m2 = av;
                }
                par ^= v <= (T)0;
                pz = pz || (v == (T)0 && !std::signbit(v));
            }
        const bool neg2 = par != (signbit_rule && m1 == (T)0 && pz);
        st[2 * (size_t)i] = par ? -m1 : m1;
        st[2 * (size_t)i + 1] = neg2 ? -m2 : m2;
    }
    return st;
}

// Row positions of the edges for the LDS-resident min-sum kernel
// (bp_ms_lds_kernel): edge e of row i sits at LDS element i * kMlDRS + pos[e].
// The check pass is independent of the order inside a row, so positions are
// free; the variable pass scatters with one ds_write_b32 per (variable round
// r, wave w, edge k): 2 x 32 lanes, bank = element % 32, cost max(4, L0 + L1)
// with L_h the worst bank load of half h (pad lanes write element m * kMlDRS +
// lane).  A seeded hill climb over position swaps inside rows lowers the sum
// over instructions (tie-break: sum of squared loads).  Cached per graph.
std::vector<int> ml_positions(int m, int n, const std::vector<int32_t>& rp, const std::vector<int32_t>& ci,
                              const std::vector<int>& edge_cpos) {
    struct Entry {
        std::vector<int32_t> rp, ci;
        std::vector<int> pos;
    };
    static std::mutex mu;
    static std::vector<Entry> cache;
    {
        std::lock_guard<std::mutex> lk(mu);
        for (const auto& c : cache)
            if (c.rp == rp && c.ci == ci) return c.pos;
    }
    const int E = rp[m];
    constexpr int NT = 1024, NB = 32;
    std::vector<int> pos(E), row(E), grp(E), half(E);
    const int rounds = (n + NT - 1) / NT;
    const int NG = rounds * (NT / 64) * kMlDC;
    std::vector<int> load((size_t)NG * 2 * NB, 0);
    for (int i = 0; i < m; ++i)
        for (int e = rp[i]; e < rp[i + 1]; ++e) {
            const int j = ci[e];
            pos[e] = e - rp[i];
            row[e] = i;
            grp[e] = ((j / NT) * (NT / 64) + (j % NT) / 64) * kMlDC + edge_cpos[e];
            half[e] = (j % 64) / 32;
        }
    auto bank = [&](int e) { return (row[e] * kMlDRS + pos[e]) % NB; };
    for (int e = 0; e < E; ++e) load[((size_t)grp[e] * 2 + half[e]) * NB + bank(e)]++;
    // pad lanes: variables without a k-th edge, slots past n
    std::vector<int> cdeg(n, 0);
    for (int e = 0; e < E; ++e) cdeg[ci[e]]++;
    for (int s = 0; s < rounds * NT; ++s)
        for (int k = 0; k < kMlDC; ++k)
            if (s >= n || k >= cdeg[s]) {
                const int gi = ((s / NT) * (NT / 64) + (s % NT) / 64) * kMlDC + k;
                load[((size_t)gi * 2 + (s % 64) / 32) * NB + (m * kMlDRS + s % 64) % NB]++;
            }
    auto gcost = [&](int gi) {
        int sum = 0, sq = 0;
        for (int h = 0; h < 2; ++h) {
            int mx = 0;
            for (int b = 0; b < NB; ++b) {
                const int v = load[((size_t)gi * 2 + h) * NB + b];
                mx = std::max(mx, v);
                sq += v * v;
            }
            sum += mx;
        }
        return (long)std::max(4, sum) * 100000 + sq;
    };
    std::mt19937 rng(2024);
    std::vector<int> at(kMlDRS);
    for (long it = 0; it < 40L * E; ++it) {
        const int i = (int)(rng() % (unsigned)m);
        const int deg = rp[i + 1] - rp[i];
        if (deg < 2) continue;
        const int e1 = rp[i] + (int)(rng() % (unsigned)deg);
        const int p2 = (int)(rng() % (unsigned)deg);
        int e2 = -1;
        for (int e = rp[i]; e < rp[i + 1]; ++e)
            if (pos[e] == p2) e2 = e;
        if (e2 == e1 || e2 < 0) continue;
        const int g1 = grp[e1], g2 = grp[e2];
        const long before = gcost(g1) + (g2 != g1 ? gcost(g2) : 0);
        auto move = [&](int e, int np) {
            load[((size_t)grp[e] * 2 + half[e]) * NB + bank(e)]--;
            pos[e] = np;
            load[((size_t)grp[e] * 2 + half[e]) * NB + bank(e)]++;
        };
        const int p1 = pos[e1];
        move(e1, p2);
        move(e2, p1);
        const long after = gcost(g1) + (g2 != g1 ? gcost(g2) : 0);
        if (after > before) {
            move(e2, p2);
            move(e1, p1);
        }
    }
    std::lock_guard<std::mutex> lk(mu);
    if (cache.size() >= 8) cache.erase(cache.begin());
    cache.push_back(Entry{rp, ci, pos});
    return pos;
}

void build_tables(HostGraph* G, int m, int n) {
    DevGraph& g = G->dg;
    g.m = m;
    g.n = n;
    const auto& rp = G->row_ptr;
    const auto& ci = G->col_idx;
    const int E = rp[m];
    // CSC with ascending rows; position of each edge inside its column list
    G->col_ptr.assign(n + 1, 0);
    for (int e = 0; e < E; ++e) G->col_ptr[ci[e] + 1]++;
    for (int j = 0; j < n; ++j) G->col_ptr[j + 1] += G->col_ptr[j];
    G->col_rows.assign(std::max(E, 1), 0);
    std::vector<int> fill(G->col_ptr.begin(), G->col_ptr.end() - 1);
    std::vector<int> edge_cpos(std::max(E, 1), 0);
    for (int i = 0; i < m; ++i)
        for (int e = rp[i]; e < rp[i + 1]; ++e) {
            const int j = ci[e];
            edge_cpos[e] = fill[j] - G->col_ptr[j];
            G->col_rows[fill[j]++] = i;
        }
    g.max_rdeg = 0;
    for (int i = 0; i < m; ++i) g.max_rdeg = std::max(g.max_rdeg, rp[i + 1] - rp[i]);
    g.max_cdeg = 0;
    for (int j = 0; j < n; ++j) g.max_cdeg = std::max(g.max_cdeg, G->col_ptr[j + 1] - G->col_ptr[j]);
    g.E = E;
    // CSC edge lists for the workgroup kernels
    std::vector<int32_t> col_edge(std::max(E, 1), 0);
    {
        std::vector<int> f2(G->col_ptr.begin(), G->col_ptr.end() - 1);
        for (int i = 0; i < m; ++i)
            for (int e = rp[i]; e < rp[i + 1]; ++e) col_edge[f2[ci[e]]++] = e;
    }
    std::vector<int32_t> edge_csc(std::max(E, 1), 0);
    for (int e = 0; e < E; ++e) edge_csc[e] = G->col_ptr[ci[e]] + edge_cpos[e];
    // edge arrays padded by kEdgePad zeros (unguarded whole-row index loads)
    col_edge.resize((size_t)E + kEdgePad, 0);
    edge_csc.resize((size_t)E + kEdgePad, 0);
    std::vector<int32_t> ci_pad(G->col_idx);
    ci_pad.resize((size_t)E + kEdgePad, 0);
    g.col_ptr = G->arena->upload(G->col_ptr);
    g.col_edge = G->arena->upload(col_edge);
    g.edge_csc = G->arena->upload(edge_csc);
    g.row_ptr = G->arena->upload(G->row_ptr);
    g.col_idx = G->arena->upload(ci_pad);
    G->smp_crow = G->arena->upload(G->col_rows);  // fault sampler: the column walk
    G->smp_thr = nullptr;
    int rc = 0, rv = 0, drc = 0;
    g.wave = (g.max_rdeg <= kDR && g.max_cdeg <= kDC && pick_wave_shape(m, n, g.max_rdeg, &rc, &rv, &drc)) ? 1 : 0;
    if (!g.wave) {  // workgroup kernels: plain 64-padding, no wave tables
        g.m_pad = (m + 63) / 64 * 64;
        g.n_pad = (n + 63) / 64 * 64;
        g.shape_drc = 0;
        // LDS-resident min-sum kernel (bp_ms_lds_kernel): edge k of column j (CSC
        // order) lives at LDS element row * kMlDRS + position in the CSR row
        g.ml_etab = nullptr;
        g.m64_etab = nullptr;
        g.m64_check = nullptr;
        g.m64_d3r = 0;
        if (g.max_rdeg <= kMlDRS && g.max_cdeg <= kMlDC && (size_t)m * kMlDRS + 64 < 0xffff) {
            const std::vector<int> pos = ml_positions(m, n, rp, ci, edge_cpos);
            std::vector<uint16_t> et((size_t)kMlDC * n, 0xffff);
            for (int i = 0; i < m; ++i)
                for (int e = rp[i]; e < rp[i + 1]; ++e)
                    et[(size_t)edge_cpos[e] * n + ci[e]] = (uint16_t)(i * kMlDRS + pos[e]);
            g.ml_etab = G->arena->upload(et);
            m64_layout(G, m, n, rp, ci, edge_cpos);
        }
        return;
    }
    g.m_pad = rc * 64;
    g.n_pad = rv * 64;
    g.shape_drc = drc;
    std::vector<uint8_t> r_deg(g.m_pad, 0), c_deg(g.n_pad, 0);
    // Pad edges (k >= degree, or padding rows/columns) point at per-lane dummies:
    // column n_pad + lane (a zero byte of xh) and message slot <array end> + lane.
    std::vector<uint16_t> r_col((size_t)kDR * g.m_pad);
    for (size_t t = 0; t < r_col.size(); ++t) r_col[t] = (uint16_t)(g.n_pad + (t % g.m_pad) % 64);
    std::vector<uint16_t> r_cslot[2], c_rslot[2];
    const int DRS[2] = {drs<double>(), drs<float>()};
    const int DCS[2] = {dcs<double>(), dcs<float>()};
    for (int p = 0; p < 2; ++p) {
        if ((size_t)g.m_pad * DRS[p] + 64 > 65535 || (size_t)g.n_pad * DCS[p] + 64 > 65535)
            throw Fail(-21, "graph too large for 16-bit LDS slots");
        r_cslot[p].resize((size_t)kDR * g.m_pad);
        for (size_t t = 0; t < r_cslot[p].size(); ++t)
            r_cslot[p][t] = (uint16_t)(g.n_pad * DCS[p] + (t % g.m_pad) % 64);
        c_rslot[p].resize((size_t)kDC * g.n_pad);
        for (size_t t = 0; t < c_rslot[p].size(); ++t)
            c_rslot[p][t] = (uint16_t)(g.m_pad * DRS[p] + (t % g.n_pad) % 64);
    }
    for (int i = 0; i < m; ++i) {
        r_deg[i] = (uint8_t)(rp[i + 1] - rp[i]);
        for (int e = rp[i], k = 0; e < rp[i + 1]; ++e, ++k) {
            const int j = ci[e];
            r_col[(size_t)k * g.m_pad + i] = (uint16_t)j;
            for (int p = 0; p < 2; ++p) {
                r_cslot[p][(size_t)k * g.m_pad + i] = (uint16_t)(j * DCS[p] + edge_cpos[e]);
            }
        }
    }
    for (int j = 0; j < n; ++j) {
        c_deg[j] = (uint8_t)(G->col_ptr[j + 1] - G->col_ptr[j]);
        for (int t = G->col_ptr[j], k = 0; t < G->col_ptr[j + 1]; ++t, ++k) {
            const int i = G->col_rows[t];
            // position of this edge inside row i
            int kr = 0;
            for (int e = rp[i]; e < rp[i + 1]; ++e, ++kr)
                if (ci[e] == j) break;
            for (int p = 0; p < 2; ++p) c_rslot[p][(size_t)k * g.n_pad + j] = (uint16_t)(i * DRS[p] + kr);
        }
    }
    g.r_deg = G->arena->upload(r_deg);
    g.r_col = G->arena->upload(r_col);
    g.c_deg = G->arena->upload(c_deg);
    for (int p = 0; p < 2; ++p) {
        g.slots[p].r_cslot = G->arena->upload(r_cslot[p]);
        g.slots[p].c_rslot = G->arena->upload(c_rslot[p]);
    }
    ms_layout(G, m, n, edge_cpos);
}

// Tables of the table-driven SSF kernel (ssf_lut_kernel, qdec_bp.hip; the s_*
// fields of DevGraph).  Inside one generator the spec's choice depends only on
// its local syndrome sl (the residual restricted to the checks its qubits
// touch): the best score max_t gain(t) * 840 / |t| over the non-empty subsets t,
// gain(t) = popc(sl) - popc(sl ^ M_t), and the lowest t reaching it (the
// oracle's strict-improvement scan in ascending t, oracle/qdec_oracle.c
// ssf_run).  One table over sl therefore replaces the per-step subset search,
// and generators whose qubits meet their local checks in the same pattern share
// it: local checks are ordered by signature (the bitmask of the generator's
// qubit positions touching them, ties by check id), which makes the masks M_t
// of two such generators identical (every generator of a hypergraph product
// code has the same 4 x 3 pattern).  Qualifies with <= 128 generators, m_pad <=
// 255 (u8 check ids), <= kLutLC local checks per generator, <= 255 distinct
// positive scores and tables within kLutBudget bytes of LDS; otherwise the s_*
// pointers stay null and the scanning kernel (ssf_wave_kernel) runs.
constexpr size_t kLutBudget = 96 * 1024;
void ssf_lut_tables(HostGraph* G, int n_gen, const int32_t* gen_ptr, const int32_t* gen_idx, int gp) {
    DevGraph& g = G->dg;
    g.s_lut = g.s_off = g.s_lcw = g.s_tog = nullptr;
    g.s_lut_n = 0;
    // the wave kernel's per-lane tables (u8 check ids, toggle rows by lane);
    // the workgroup SSF kernel reads only the score tables and offsets
    const bool lanes = n_gen <= 128 && g.m_pad <= 255;
    if (n_gen >= 8192) return;
    std::vector<std::vector<uint32_t>> shapes;  // (w, nlc, M_0 .. M_{w-1}) in first-seen order
    std::vector<int> shape_off;
    std::vector<uint32_t> off(gp, 0);
    std::vector<uint32_t> lcw((size_t)kLutLCW * gp, 0xffffffffu);
    std::vector<uint32_t> tog(lanes ? ((size_t)g.m_pad + 1) * 64 : 0, 0);  // row m_pad: zero (unflipped bits)
    int total = 0;
    for (int gi = 0; gi < n_gen; ++gi) {
        const int a = gen_ptr[gi], w = gen_ptr[gi + 1] - a;
        std::vector<std::pair<int, uint32_t>> sig;  // (check, signature)
        for (int k = 0; k < w; ++k) {
            const int q = gen_idx[a + k];
            for (int t = G->col_ptr[q]; t < G->col_ptr[q + 1]; ++t) {
                const int c = G->col_rows[t];
                auto it = std::find_if(sig.begin(), sig.end(), [c](const auto& e) { return e.first == c; });
                if (it == sig.end()) sig.push_back({c, 1u << k});
                else it->second ^= 1u << k;
            }
        }
        if ((int)sig.size() > kLutLC) return;
        std::sort(sig.begin(), sig.end(), [](const auto& x, const auto& y) {
            return x.second != y.second ? x.second < y.second : x.first < y.first;
        });
        const int nlc = (int)sig.size();
        std::vector<uint32_t> key = {(uint32_t)w, (uint32_t)nlc};
        for (int k = 0; k < w; ++k) {
            uint32_t mk = 0;
            for (int b = 0; b < nlc; ++b)
                if ((sig[b].second >> k) & 1) mk |= 1u << b;
            key.push_back(mk);
        }
        const auto it = std::find(shapes.begin(), shapes.end(), key);
        int o;
        if (it == shapes.end()) {
            o = total;
            shapes.push_back(key);
            shape_off.push_back(o);
            total += 1 << nlc;
        } else {
            o = shape_off[it - shapes.begin()];
        }
        off[gi] = (uint32_t)o;
        if (lanes)
            for (int b = 0; b < nlc; ++b) {
                const int c = sig[b].first;
                uint32_t& word = lcw[(size_t)(b / 4) * gp + gi];
                word = (word & ~(0xffu << (8 * (b % 4)))) | ((uint32_t)c << (8 * (b % 4)));
                tog[(size_t)c * 64 + (gi & 63)] |= (1u << b) << (16 * (gi >> 6));
            }
    }
    if ((size_t)total * 4 > kLutBudget) return;
    const bool lane_tabs = lanes && (size_t)total * 4 + ((size_t)g.m_pad + 1) * 256 <= kLutBudget;
    // best (score, t) of every local syndrome of every shape; scores -> ranks
    std::vector<int> score(total, 0);
    std::vector<uint32_t> lut(total, 0);
    for (size_t s = 0; s < shapes.size(); ++s) {
        const int w = (int)shapes[s][0], nlc = (int)shapes[s][1], o = shape_off[s];
        std::vector<uint32_t> Mt((size_t)1 << w, 0);
        for (int t = 1; t < (1 << w); ++t) Mt[t] = Mt[t & (t - 1)] ^ shapes[s][2 + __builtin_ctz(t)];
        for (int sl = 0; sl < (1 << nlc); ++sl) {
            const int base = __builtin_popcount(sl);
            int best = 0, bt = 0;
            for (int t = 1; t < (1 << w); ++t) {
                const int gain = base - __builtin_popcount((uint32_t)sl ^ Mt[t]);
                if (gain <= 0) continue;
                const int sc = gain * kSsfScale / __builtin_popcount(t);
                if (sc > best) {  // strict: ties keep the lowest t
                    best = sc;
                    bt = t;
                }
            }
            score[o + sl] = best;
            lut[o + sl] = bt ? (Mt[bt] << 8 | (uint32_t)bt) : 0u;
        }
    }
    std::vector<int> ranks(score.begin(), score.end());
    std::sort(ranks.begin(), ranks.end());
    ranks.erase(std::unique(ranks.begin(), ranks.end()), ranks.end());
    if (!ranks.empty() && ranks[0] == 0) ranks.erase(ranks.begin());
    if (ranks.size() > 255) return;
    for (int e = 0; e < total; ++e)
        if (score[e] > 0)
            lut[e] |= (uint32_t)(std::lower_bound(ranks.begin(), ranks.end(), score[e]) - ranks.begin() + 1) << 24;
    g.s_lut = G->flip_arena->upload(lut);
    g.s_lut_n = total;
    g.s_off = G->flip_arena->upload(off);
    if (lane_tabs) {
        g.s_lcw = G->flip_arena->upload(lcw);
        g.s_tog = G->flip_arena->upload(tog);
    }
}

// Upload logicals given as CSR supports: the CSR itself (duplicates cancelled,
// sorted) and, when it stays below 256 MB, the dense bit-packed table the wave
// kernels and the OSD finalize read.  lz_sparse picks the workgroup finalize's
// support walk when the supports are small against the dense words.
void upload_logicals(HostGraph* G, int32_t k, std::vector<int32_t> ptr, std::vector<int32_t> idx) {
    DevGraph& g = G->dg;
    const int W = g.lz_words;
    G->lz_arena->release();
    g.lz = nullptr;
    g.lz_ptr = g.lz_idx = nullptr;
    g.ms_lzs = nullptr;
    g.lz_t = nullptr;
    g.lz_tw = 0;
    g.k = 0;
    g.lz_sparse = 0;
    if (k == 0) return;
    // canonical supports: sorted, pairs cancel
    std::vector<int32_t> cptr(1, 0), cidx;
    cidx.reserve(idx.size());
    for (int r = 0; r < k; ++r) {
        std::vector<int32_t> row(idx.begin() + ptr[r], idx.begin() + ptr[r + 1]);
        std::sort(row.begin(), row.end());
        for (size_t t = 0; t < row.size();) {
            size_t u = t;
            while (u < row.size() && row[u] == row[t]) ++u;
            if ((u - t) & 1) cidx.push_back(row[t]);
            t = u;
        }
        cptr.push_back((int32_t)cidx.size());
    }
    if ((size_t)k * W * 8 <= ((size_t)256 << 20)) {
        std::vector<uint64_t> packed((size_t)k * W, 0);
        for (int r = 0; r < k; ++r)
            for (int t = cptr[r]; t < cptr[r + 1]; ++t) packed[(size_t)r * W + cidx[t] / 64] |= 1ull << (cidx[t] % 64);
        g.lz = G->lz_arena->upload(packed);
    }
    g.lz_ptr = G->lz_arena->upload(cptr);
    g.lz_idx = G->lz_arena->upload(cidx);
    const int tw = (k + 31) / 32;
    if ((size_t)g.n_data * tw * 4 <= ((size_t)64 << 20)) {
        std::vector<uint32_t> tr((size_t)g.n_data * tw, 0u);
        for (int r = 0; r < k; ++r)
            for (int t = cptr[r]; t < cptr[r + 1]; ++t) tr[(size_t)cidx[t] * tw + r / 32] |= 1u << (r % 32);
        g.lz_t = G->lz_arena->upload(tr);
        g.lz_tw = tw;
    }
    // wave graphs: the same logicals in the min-sum kernel's lane-slot order
    // ([k][n_pad/64] words, bit s%64 of word s/64 = the column of slot s), so the
    // compact-list kernel tests its ballot words without a column permutation
    g.ms_lzs = nullptr;
    if (!G->ms_var_of_slot.empty() && k <= 256) {
        const int RVn = g.n_pad / 64;
        std::vector<int> col_bit(g.n_data, -1);
        for (int sl = 0; sl < g.n_pad; ++sl) {
            const int j = G->ms_var_of_slot[sl];
            if (j >= 0 && j < g.n_data) col_bit[j] = sl;
        }
        std::vector<uint64_t> lzs((size_t)k * RVn, 0);
        for (int r = 0; r < k; ++r)
            for (int t = cptr[r]; t < cptr[r + 1]; ++t) {
                const int sl = col_bit[cidx[t]];
                if (sl >= 0) lzs[(size_t)r * RVn + sl / 64] |= 1ull << (sl % 64);
            }
        g.ms_lzs = G->lz_arena->upload(lzs);
    }
    // a support walk costs ~ one gather per entry, the dense test one word per
    // (logical, word): walk when that is clearly cheaper, or when there is no table
    g.lz_sparse = (!g.lz || cidx.size() <= (size_t)k * W / 4) ? 1 : 0;
    g.k = k;
}

}  // namespace

void init_graph(HostGraph* G, int m, int n, const int32_t* row_ptr, const int32_t* col_idx, int n_data,
                int fold_blocks) {
    G->row_ptr.assign(row_ptr, row_ptr + m + 1);
    G->col_idx.assign(col_idx, col_idx + row_ptr[m]);
    G->dg.n_data = n_data;
    G->dg.fold_blocks = fold_blocks;
    build_tables(G, m, n);
    G->dg.lz_words = (n_data + 63) / 64;
    G->dg.k = 0;
    G->dg.lz = nullptr;
    G->dg.lz_ptr = G->dg.lz_idx = nullptr;
    G->dg.lz_sparse = 0;
    G->dg.lz_t = nullptr;
    G->dg.lz_tw = 0;
    G->dg.n_gen = 0;
    G->dg.g_inv = nullptr;
    G->dg.g_invd = G->dg.g_invl = 0;
    default_options(G->dg);
}

void set_flipsets(HostGraph* G, int32_t n_gen, const int32_t* gen_ptr, const int32_t* gen_idx) {
    if (n_gen <= 0 || !gen_ptr || !gen_idx) throw Fail(-30, "invalid flip sets");
    DevGraph& g = G->dg;
    const int gp = std::max(g.m_pad, (n_gen + 63) / 64 * 64);
    const bool pack8 = g.m_pad <= 255;  // u8 local-check ids for the wave SSF kernel
    std::vector<uint8_t> w(gp, 0), nlc(gp, 0);
    std::vector<uint16_t> q((size_t)kGenW * gp, 0), lc((size_t)kGenLC * gp, 0);
    std::vector<uint32_t> qm((size_t)kGenW * gp, 0);
    std::vector<uint32_t> lc8((size_t)(kGenLC / 4) * gp, 0);
    for (int gi = 0; gi < gp; ++gi)
        for (int c = 0; c < kGenLC; ++c) lc8[(size_t)(c / 4) * gp + gi] |= (uint32_t)g.m_pad << (8 * (c % 4));
    int wmax = 0, nlcmax = 0;
    std::vector<std::vector<uint16_t>> inv(g.m_pad);  // check -> (generator, local bit)
    std::vector<std::vector<uint32_t>> inv_all(g.m);  // the same for every generator (block SSF)
    for (int gi = 0; gi < n_gen; ++gi) {
        const int a = gen_ptr[gi], b = gen_ptr[gi + 1];
        if (b < a) throw Fail(-31, "gen_ptr not monotone");
        const int wg = b - a;
        if (wg > kGenW) throw Fail(-32, "flip-set generator weight exceeds 8");
        // local checks in the canonical order of ssf_lut_tables: by signature
        // (the bitmask of this generator's qubit positions touching the
        // check), ties by check id.  The spec does not depend on the order
        // (it is internal to the local-syndrome words), and with it every
        // kernel's local syndrome indexes the shared score tables directly.
        std::vector<std::pair<uint32_t, int>> sig;  // (signature, check)
        for (int k = 0; k < wg; ++k) {
            const int qq = gen_idx[a + k];
            if (qq < 0 || qq >= g.n) throw Fail(-33, "flip-set qubit out of range");
            if (k > 0 && qq <= gen_idx[a + k - 1]) throw Fail(-34, "flip-set qubits must be strictly ascending");
            for (int t = G->col_ptr[qq]; t < G->col_ptr[qq + 1]; ++t) {
                const int c = G->col_rows[t];
                auto it = std::find_if(sig.begin(), sig.end(), [c](const auto& e) { return e.second == c; });
                if (it == sig.end()) sig.push_back({1u << k, c});
                else it->first ^= 1u << k;
            }
        }
        std::sort(sig.begin(), sig.end());
        std::vector<int> checks;
        for (const auto& e : sig) checks.push_back(e.second);
        if ((int)checks.size() > kGenLC) throw Fail(-35, "flip-set generator touches more than 32 checks");
        w[gi] = (uint8_t)wg;
        nlc[gi] = (uint8_t)checks.size();
        wmax = std::max(wmax, wg);
        nlcmax = std::max(nlcmax, (int)checks.size());
        for (size_t c = 0; c < checks.size(); ++c) {
            lc[c * gp + gi] = (uint16_t)checks[c];
            if (gi < 256) inv[checks[c]].push_back((uint16_t)(gi | (c << 8)));
            inv_all[checks[c]].push_back((uint32_t)gi | ((uint32_t)c << 16));
            uint32_t& word = lc8[(c / 4) * gp + gi];
            word = (word & ~(0xffu << (8 * (c % 4)))) | ((uint32_t)checks[c] << (8 * (c % 4)));
        }
        for (int k = 0; k < wg; ++k) {
            q[(size_t)k * gp + gi] = (uint16_t)gen_idx[a + k];
            uint32_t mask = 0;
            for (size_t c = 0; c < sig.size(); ++c)
                if ((sig[c].first >> k) & 1u) mask |= 1u << c;
            qm[(size_t)k * gp + gi] = mask;
        }
    }
    size_t invmax = 1;
    for (const auto& v : inv) invmax = std::max(invmax, v.size());
    int invl = 0;
    while ((size_t)1 << invl < invmax) ++invl;
    const int invd = 1 << invl;
    std::vector<uint16_t> invt;
    // graphs whose table would be too wide get none: the scanning wave SSF
    // kernel then re-gathers the local syndromes every step (QD_SSF_SCAN_GATHER
    // takes that path on any graph)
    if (pack8 && n_gen <= 128 && invd <= 64) {
        invt.assign((size_t)g.m_pad * invd, 0xffff);
        for (int i = 0; i < g.m_pad; ++i)
            for (size_t t = 0; t < inv[i].size(); ++t) invt[(size_t)i * invd + t] = inv[i][t];
    }
    G->flip_arena->release();
    g.g_lc8 = nullptr;
    g.g_inv = invt.empty() ? nullptr : G->flip_arena->upload(invt);
    g.g_invd = invt.empty() ? 0 : invd;
    g.g_invl = invt.empty() ? 0 : invl;
    g.g_w = G->flip_arena->upload(w);
    g.g_nlc = G->flip_arena->upload(nlc);
    g.g_q = G->flip_arena->upload(q);
    g.g_lc = G->flip_arena->upload(lc);
    g.g_qmask = G->flip_arena->upload(qm);
    if (pack8) g.g_lc8 = G->flip_arena->upload(lc8);
    g.g_nlcmax = nlcmax;
    ssf_lut_tables(G, n_gen, gen_ptr, gen_idx, gp);
    g.g_iptr = nullptr;
    g.g_ient = nullptr;
    if (n_gen < 65536) {
        std::vector<int32_t> iptr(g.m + 1, 0);
        std::vector<uint32_t> ient;
        for (int i = 0; i < g.m; ++i) {
            ient.insert(ient.end(), inv_all[i].begin(), inv_all[i].end());
            iptr[i + 1] = (int32_t)ient.size();
        }
        g.g_iptr = G->flip_arena->upload(iptr);
        g.g_ient = G->flip_arena->upload(ient);
    }
    g.n_gen = n_gen;
    g.g_pad = gp;
    g.g_wmax = wmax;
}

void set_logicals(HostGraph* G, int32_t k, const uint8_t* lz) {
    DevGraph& g = G->dg;
    if (k < 0 || (k > 0 && !lz)) throw Fail(-40, "invalid logicals");
    if (k > 65536) throw Fail(-41, "more than 65536 logicals not supported");
    std::vector<int32_t> ptr(1, 0), idx;
    for (int r = 0; r < k; ++r) {
        for (int q = 0; q < g.n_data; ++q)
            if (lz[(size_t)r * g.n_data + q] & 1) idx.push_back(q);
        ptr.push_back((int32_t)idx.size());
    }
    upload_logicals(G, k, std::move(ptr), std::move(idx));
}

void set_logicals_csr(HostGraph* G, int32_t k, const int32_t* lz_ptr, const int32_t* lz_idx) {
    const DevGraph& g = G->dg;
    if (k < 0 || (k > 0 && (!lz_ptr || (!lz_idx && lz_ptr[k] > 0)))) throw Fail(-40, "invalid logicals");
    if (k > 65536) throw Fail(-41, "more than 65536 logicals not supported");
    std::vector<int32_t> ptr(lz_ptr, lz_ptr + (k > 0 ? k + 1 : 0)), idx;
    if (k > 0) {
        if (ptr[0] != 0) throw Fail(-42, "logicals CSR must start at 0");
        for (int r = 0; r < k; ++r)
            if (ptr[r + 1] < ptr[r]) throw Fail(-42, "logicals CSR pointers must be non-decreasing");
        idx.assign(lz_idx, lz_idx + ptr[k]);
        for (int32_t q : idx)
            if (q < 0 || q >= g.n_data) throw Fail(-43, "logical support index out of range");
    }
    upload_logicals(G, k, std::move(ptr), std::move(idx));
}

void set_priors(HostGraph* G, const double* probs) {
    if (!probs) throw Fail(-50, "null channel_probs");
    DevGraph& g = G->dg;
    std::vector<double> ms64(g.n_pad, 0.0), ps64(g.n_pad, 0.0);
    std::vector<float> ms32(g.n_pad, 0.0f), ps32(g.n_pad, 0.0f);
    std::vector<uint32_t> thr(((size_t)g.n + 3) / 4 * 4, 0u);  // fault sampler; pads never fire
    bool open = true;
    for (int j = 0; j < g.n; ++j) {
        const double p = probs[j];
        if (!(p >= 0.0 && p <= 1.0)) throw Fail(-51, "channel probability outside [0, 1]");
        // open interval: keeps every BP message finite (and NaN-free), the
        // precondition of the kernels' min/med3 check-node formulation
        open = open && p > 0.0 && p < 1.0;
        thr[j] = bern_threshold(p);
    }
    if (!open) {  // a certain or impossible fault: a graph to sample from, not to decode on
        G->prior_arena->release();
        for (auto& m2 : g.prior)
            for (auto& q : m2) q = nullptr;
        for (auto& m2 : g.eprior)
            for (auto& q : m2) q = nullptr;
        g.ms_prior[QD_F64] = g.ms_prior[QD_F32] = nullptr;
        g.ms_state0[QD_F64] = g.ms_state0[QD_F32] = nullptr;
        g.it1_vchk = g.it1_cvar = nullptr;
        g.it1_lut[QD_F64] = g.it1_lut[QD_F32] = nullptr;
        g.ms_allpos = 0;
        G->smp_thr = G->prior_arena->upload(thr);
        G->bp_priors = false;
        G->prior_ms64.clear();
        return;
    }
    for (int j = 0; j < g.n; ++j) {
        const double p = probs[j];
        ms64[j] = std::log((1 - p) / p);   // ldpc v1: log((1-p)/p)
        ps64[j] = p / (1 - p);             // ldpc v1: p/(1-p)
        ms32[j] = (float)ms64[j];
        ps32[j] = (float)ps64[j];
    }
    G->prior_arena->release();
    g.prior[QD_MIN_SUM][QD_F64] = G->prior_arena->upload(ms64);
    g.prior[QD_MIN_SUM][QD_F32] = G->prior_arena->upload(ms32);
    if (!G->ms_var_of_slot.empty()) {  // min-sum wave kernel: lane-slot order
        std::vector<double> s64(g.n_pad, 0.0);
        std::vector<float> s32(g.n_pad, 0.0f);
        for (int s2 = 0; s2 < g.n_pad; ++s2) {
            const int j = G->ms_var_of_slot[s2];
            if (j >= 0) {
                s64[s2] = ms64[j];
                s32[s2] = ms32[j];
            }
        }
        g.ms_prior[QD_F64] = G->prior_arena->upload(s64);
        g.ms_prior[QD_F32] = G->prior_arena->upload(s32);
        // all priors > 0: the wave kernel's zero-syndrome shortcut applies
        bool pos64 = true, pos32 = true;
        for (int j = 0; j < g.n; ++j) {
            pos64 = pos64 && ms64[j] > 0.0;
            pos32 = pos32 && ms32[j] > 0.0f;
        }
        g.ms_allpos = (pos64 ? 1 << QD_F64 : 0) | (pos32 ? 1 << QD_F32 : 0);
        it1_tables(G, pos64, ms64, pos32, ms32);
        // the compact kernel is lean: f64 runs the sign-bit check pass, f32 the compares
        g.ms_state0[QD_F64] = G->prior_arena->upload(ms_state0_table<double>(G, ms64, 1e308, true));
        g.ms_state0[QD_F32] = G->prior_arena->upload(ms_state0_table<float>(G, ms32, 1e30f, false));
    }
    g.prior[QD_PRODUCT_SUM][QD_F64] = G->prior_arena->upload(ps64);
    g.prior[QD_PRODUCT_SUM][QD_F32] = G->prior_arena->upload(ps32);
    {  // by CSR edge, padded (slot-group kernel)
        const size_t ne = (size_t)g.E + kEdgePad;
        std::vector<double> ems64(ne, 0.0), eps64(ne, 0.0);
        std::vector<float> ems32(ne, 0.0f), eps32(ne, 0.0f);
        for (int e = 0; e < g.E; ++e) {
            const int j = G->col_idx[e];
            ems64[e] = ms64[j], eps64[e] = ps64[j], ems32[e] = ms32[j], eps32[e] = ps32[j];
        }
        g.eprior[QD_MIN_SUM][QD_F64] = G->prior_arena->upload(ems64);
        g.eprior[QD_MIN_SUM][QD_F32] = G->prior_arena->upload(ems32);
        g.eprior[QD_PRODUCT_SUM][QD_F64] = G->prior_arena->upload(eps64);
        g.eprior[QD_PRODUCT_SUM][QD_F32] = G->prior_arena->upload(eps32);
    }
    G->smp_thr = G->prior_arena->upload(thr);
    G->bp_priors = true;
    G->prior_ms64.assign(ms64.begin(), ms64.begin() + g.n);
}

void table_digest(const HostGraph* G, uint64_t* digest, int64_t* bytes) {
    uint64_t h = 1469598103934665603ull;  // FNV-1a over every table, in upload order
    int64_t total = 0;
    for (const TableSink* a : {G->arena.get(), G->flip_arena.get(), G->lz_arena.get(), G->prior_arena.get()})
        for (const auto& v : static_cast<const HostSink*>(a)->kept) {
            for (uint8_t b : v) h = (h ^ b) * 1099511628211ull;
            total += (int64_t)v.size();
        }
    if (digest) *digest = h;
    if (bytes) *bytes = total;
}

void sample_tables_copy(const HostGraph* G, uint32_t* thr, int32_t* crow) {
    const DevGraph& g = G->dg;
    if (!G->smp_thr) throw Fail(-63, "priors not set (qd_graph_set_priors): no fault thresholds");
    if (thr) std::memcpy(thr, G->smp_thr, (size_t)g.n * 4);
    if (crow && g.E > 0) std::memcpy(crow, G->smp_crow, (size_t)g.E * 4);
}

void ssf_tables_copy(const DevGraph& g, uint32_t* lut, uint32_t* off, uint32_t* lcw, uint32_t* tog, int32_t* g_pad,
                     int32_t* m_pad) {
    if (!g.s_lut || !g.s_tog) throw Fail(-36, "the graph has no table-driven wave SSF tables");
    if (g_pad) *g_pad = g.g_pad;
    if (m_pad) *m_pad = g.m_pad;
    auto put = [](uint32_t* dst, const uint32_t* src, size_t n) {
        if (dst) std::memcpy(dst, src, n * 4);
    };
    put(lut, g.s_lut, (size_t)g.s_lut_n);
    put(off, g.s_off, (size_t)g.g_pad);
    put(lcw, g.s_lcw, (size_t)kLutLCW * g.g_pad);
    put(tog, g.s_tog, ((size_t)g.m_pad + 1) * 64);
}

size_t cmp_entry_bytes(const DevGraph& g) { return 8 * (1 + (size_t)g.m_pad / 64 + 4); }

QueueLayout queue_layout(const DevGraph& g, int64_t cap) {
    QueueLayout L{};
    const size_t packed = 8 * (1 + 2 * (size_t)g.n_pad / 64 + (size_t)g.m_pad / 64);
    const size_t xr = std::max((size_t)g.n + (size_t)g.m, packed);
    L.idx = 256;
    L.x = 256 + (size_t)cap * 8;
    L.r = L.x + (size_t)cap * g.n;
    const size_t cbase = 256 + ((size_t)cap * (8 + xr) + 255) / 256 * 256 + 256;
    L.cmp_count = g.wave ? cbase : 0;
    L.cmp = g.wave ? cbase + (size_t)kCmpLists * kCmpSegs * 128 : 0;
    L.cmp_cap = g.wave ? cmp_seg_cap(cap) : 0;
    L.bytes = cbase +
              (g.wave ? (size_t)kCmpLists * kCmpSegs * (128 + (size_t)L.cmp_cap * cmp_entry_bytes(g)) : 0) + 256;
    return L;
}

}  // namespace qdec
