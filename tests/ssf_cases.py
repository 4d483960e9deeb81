"""Graphs, flip sets and decode cases shared by tests/test_ssf_mixed_host.py (CPU:
tables, plans, the instantiation ledger) and tests/test_gpu_ssf_mixed.py (GPU:
parity with the oracle).

The codes the rest of the suite decodes with SSF (hypergraph products, the
bivariate-bicycle lift) give every flip-set generator the same weight and the
same local pattern, so all generators share one score table.  mixed_flip_sets
draws generators of weight 1..4 (one of weight 8) with 1..max_lc local checks
that overlap, repeat and share checks inside a generator; the cases run them on
every wave shape and on the workgroup kernels, and a set of BP-only cases reaches
the instantiations of the workgroup BP families nothing else launches.

Everything is generated from seeds; nothing here needs a GPU."""
import functools
import itertools

import numpy as np
import scipy.sparse as sp

SSF_WANT = ("x", "corr", "iters", "status", "ssf_steps", "fail")
LEAN_WANT = ("iters", "status", "ssf_steps", "fail")
BP_WANT = ("x", "iters", "status")
TNAME = {"f32": "float", "f64": "double"}
# the wave shapes whose checks fit the wave SSF kernels' u8 check ids (m_pad <= 255)
SSF_WAVE_SHAPES = ((1, 2, 8), (2, 3, 6), (2, 3, 8), (2, 4, 7), (2, 4, 8), (2, 6, 8))
WAVE_NGEN = (40, 64, 65, 128)


# ---------------------------------------------------------------- flip sets
def mixed_flip_sets(H, seed, n_gen, max_lc, wmax=4):
    """n_gen flip-set generators on H's columns as CSR (ascending qubits):
    weights cycle through 1..wmax, every generator touches between 1 and max_lc
    checks, later generators reuse qubits of earlier ones, generator 1 has two
    qubits sharing a check (a two-bit signature), generator n_gen // 2 is an
    exact copy of generator 3 (a tie the lower index wins), and the last one has
    weight 8 on the lowest-degree columns when eight of them stay within
    max_lc checks."""
    H = sp.csr_matrix(H)
    Hc = H.tocsc()
    Hc.sort_indices()
    m, n = H.shape
    rng = np.random.default_rng(seed)
    chk = [frozenset(Hc.indices[Hc.indptr[j]:Hc.indptr[j + 1]].tolist()) for j in range(n)]
    live = np.array([j for j in range(n) if chk[j]])
    rows = [H.indices[H.indptr[i]:H.indptr[i + 1]] for i in range(m)]

    def union(qs):
        return frozenset().union(*(chk[q] for q in qs))

    def neighbours(qs):
        out = set()
        for c in union(qs):
            out.update(rows[c].tolist())
        return sorted(out - set(qs))

    def draw(w, used):
        for _ in range(400):
            pool = used if used and rng.random() < 0.5 else live
            qs = [int(rng.choice(pool))]
            while len(qs) < w:
                near = neighbours(qs) if rng.random() < 0.6 else []
                cand = [int(q) for q in rng.permutation(near if near else live)[:12] if q not in qs]
                cand = [q for q in cand if len(union(qs + [q])) <= max_lc]
                if not cand:
                    break
                qs.append(cand[0])
            if len(qs) == w and 1 <= len(union(qs)) <= max_lc:
                return sorted(qs)
        raise RuntimeError("no generator of this weight within max_lc")

    gens, used = [], []
    for gi in range(n_gen):
        w = 1 + gi % wmax
        if gi == 1:  # two qubits of one check
            pairs = [r for r in rows if len(r) >= 2]
            while True:
                r = pairs[int(rng.integers(len(pairs)))]
                qs = sorted(int(q) for q in rng.choice(r, 2, replace=False))
                if len(union(qs)) <= max_lc:
                    break
        elif gi == n_gen // 2 and gi > 3:
            qs = list(gens[3])
        else:
            qs = draw(w, used)
        gens.append(qs)
        used = sorted(set(used) | set(qs))
    # weight 8: greedily the columns that add the fewest checks
    qs = [int(live[np.argmin([len(chk[j]) for j in live])])]
    while len(qs) < 8:
        rest = [int(j) for j in live if j not in qs]
        grow = [len(union(qs + [j])) for j in rest]
        qs.append(rest[int(np.argmin(grow))])
    if len(union(qs)) <= max_lc:
        gens[-1] = sorted(qs)
    ptr = np.cumsum([0] + [len(g) for g in gens])
    G = sp.csr_matrix((np.ones(ptr[-1], np.uint8), np.concatenate(gens), ptr), shape=(n_gen, n))
    G.sort_indices()
    # the properties the cases rely on
    assert all(1 <= len(union(g)) <= max_lc for g in gens)
    assert {len(g) for g in gens} >= set(range(1, wmax + 1))
    assert len(chk[gens[1][0]] & chk[gens[1][1]]) >= 1
    assert n_gen <= 7 or gens[n_gen // 2] == gens[3]
    assert sum(len(set(a) & set(b)) > 0 for a, b in itertools.combinations(gens[:40], 2)) >= 8
    return G


def flip_set_stats(H, G):
    """(weights, local-check counts, the most generators on one check)."""
    Hc = sp.csc_matrix(H)
    G = sp.csr_matrix(G)
    per_check = np.zeros(H.shape[0], int)
    w, nlc = [], []
    for g in range(G.shape[0]):
        qs = G.indices[G.indptr[g]:G.indptr[g + 1]]
        cs = set()
        for q in qs:
            cs.update(Hc.indices[Hc.indptr[q]:Hc.indptr[q + 1]].tolist())
        w.append(len(qs))
        nlc.append(len(cs))
        per_check[list(cs)] += 1
    return np.array(w), np.array(nlc), int(per_check.max())


# ---------------------------------------------------------------- graphs
def column_graph(m, n, seed, degrees, row_cap):
    """Column-driven random graph: column j takes degrees[j] distinct rows among
    those still below row_cap (so the row-degree bound of a kernel holds by
    construction and the column degrees are exactly the ones asked for)."""
    from exp_ldpc_amd.codes import make_check_matrix
    rng = np.random.default_rng(seed)
    rows, cnt = [[] for _ in range(m)], np.zeros(m, int)
    for j in range(n):
        for i in rng.choice(np.flatnonzero(cnt < row_cap), int(degrees[j]), replace=False):
            rows[i].append(j)
            cnt[i] += 1
    return make_check_matrix(rows, n)  # columns were appended in ascending order


def row_graph(m, n, seed, rmin, rmax, cmax):
    """Row-driven ragged graph (as test_gpu_large_codes' random graphs): row
    degrees uniform in rmin..rmax, column degrees capped at cmax."""
    from exp_ldpc_amd.codes import make_check_matrix
    rng = np.random.default_rng(seed)
    rows, colcount = [], np.zeros(n, int)
    for _ in range(m):
        d = int(rng.integers(rmin, rmax + 1))
        cand = [j for j in rng.permutation(n) if colcount[j] < cmax][:d]
        for j in cand:
            colcount[j] += 1
        rows.append(sorted(cand))
    return make_check_matrix(rows, n)


def _with_priors(H, seed, lo, hi):
    rng = np.random.default_rng(seed)
    n = H.shape[1]
    return H, rng.uniform(lo, hi, n), (rng.random((3, n)) < 0.05).astype(np.uint8)


def _mixed_degrees(n, seed, probs):
    return np.random.default_rng(seed).choice(np.arange(1, len(probs) + 1), size=n, p=probs)


def _wave(shape):
    from test_gpu_compact import wave_shape_graph
    return wave_shape_graph(shape)


def _w247_dense():
    # (2, 4, 7) with fewer than 128 columns of degree <= 3 (the second 64-column
    # round of the degree-sorted slots holds a degree-4 column): the kernels' D3R = 0
    deg = np.random.default_rng(247).permutation(np.r_[np.full(104, 1), np.full(23, 2), np.full(104, 4)])
    return _with_priors(column_graph(121, 231, 2470, deg, 7), 2471, 0.005, 0.05)


def _lds(m, n, probs):
    return lambda: _with_priors(column_graph(m, n, n, _mixed_degrees(n, n + 1, probs), 8), n + 2, 0.002, 0.02)


GRAPHS = {
    **{"w%d%d%d" % s: functools.partial(_wave, s) for s in SSF_WAVE_SHAPES + ((4, 9, 8),)},
    "w247d0": _w247_dense,
    # workgroup graphs for SSF: check degrees 0..9 / column degrees 0..5, and the
    # variant within the LDS-resident kernels' bounds (8 / 4)
    "b300": lambda: _with_priors(row_graph(300, 700, 300, 0, 9, 5), 301, 0.01, 0.08),
    "b300lds": lambda: _with_priors(row_graph(300, 700, 302, 0, 8, 4), 303, 0.01, 0.08),
    # bp_ms_lds_kernel<8 / 12 / 16>: odd m, n one short of the 1024-column round
    "lds8191": _lds(5001, 8191, [0.1, 0.2, 0.3, 0.4]),
    "lds12287": _lds(5001, 12287, [0.1, 0.25, 0.3, 0.35]),
    "lds16383": _lds(5001, 16383, [0.2, 0.4, 0.3, 0.1]),
    "lds8193": _lds(5001, 8193, [0.1, 0.2, 0.3, 0.4]),    # 9 columns per thread -> <10>
    "lds4097": _lds(2001, 4097, [0.1, 0.2, 0.3, 0.4]),    # 5 -> <8>
    # bp_group_kernel's degree cells: (8, 8) and (16, 4); b300 is (16, 8), b300lds (8, 4)
    "g88": lambda: _with_priors(column_graph(400, 700, 88, _mixed_degrees(700, 87, [.15, .2, .15, .15, .1, .1, .1, .05]),
                                             8), 89, 0.01, 0.06),
    "g164": lambda: _with_priors(row_graph(300, 900, 164, 0, 16, 4), 165, 0.01, 0.06),
}


@functools.lru_cache(maxsize=None)
def graph(key):
    H, probs, L = GRAPHS[key]()
    H = sp.csr_matrix(H)
    H.sort_indices()
    return H, probs, L


@functools.lru_cache(maxsize=None)
def flip_sets(key, n_gen, max_lc):
    G = mixed_flip_sets(graph(key)[0], 1000 * n_gen + max_lc, n_gen, max_lc)
    assert np.diff(G.indptr).max() == 8, "every graph of the cases holds a weight-8 generator"
    return G


# error-rate classes of the shots, by shot index mod 4: light shots BP decodes
# in a few iterations next to heavy ones it does not, in every window of four
RATE_CLASSES = (0.1, 0.35, 1.0, 2.0)


@functools.lru_cache(maxsize=None)
def shots(key, B, p, seed=0):
    """(syn, readout) of B shots on the graph: shot b has error rate
    RATE_CLASSES[b % 4] * p; readout = error ^ noise.  No shot is forced to be
    error-free."""
    H = graph(key)[0]
    n = H.shape[1]
    rng = np.random.default_rng(seed + n)
    rate = (np.array(RATE_CLASSES)[np.arange(B) % 4] * p)[:, None]
    e = (rng.random((B, n)) < rate).astype(np.uint8)
    syn = np.ascontiguousarray(((H @ e.T).T % 2).astype(np.uint8))
    rd = (e ^ (rng.random((B, n)) < 0.01)).astype(np.uint8)
    return syn, rd


def case_shots(case):
    """(syn, readout) of a case.  The 5-shot cases take shots offset .. offset + 4
    of their graph's 700."""
    syn, rd = shots(case["graph"], case["B"] if case["B"] > 5 else 700, case["p"])
    return syn[case["offset"]:case["offset"] + case["B"]], rd[case["offset"]:case["offset"] + case["B"]]


# ---------------------------------------------------------------- cases
def max_lc_of(n_gen):
    """Local checks per generator that keep the score tables plus the toggle
    rows within the table kernels' 96 KB of LDS."""
    return 9 if n_gen <= 64 else 7


def _case(graph, **kw):
    c = dict(graph=graph, n_gen=0, max_lc=0, method="ms", precision="f64", options={}, occ=0, want=SSF_WANT, B=257,
             p=0.03, max_iter=3, steps=0, packed=False, scaling=0.0, ssf=True, bp="", fin="", pre=None, path=None,
             offset=0)
    c.update(kw)
    c["id"] = "-".join(str(v) for v in (c["graph"], c["n_gen"], c["method"], c["precision"],
                                        "lean" if "x" not in c["want"] else "full",
                                        ",".join(f"{k}={v}" for k, v in sorted(c["options"].items())) or "default",
                                        f"s{c['steps']}", f"i{c['max_iter']}", f"a{c['scaling']}",
                                        "pk" if c["packed"] else "by", f"o{c['occ']}", f"B{c['B']}", f"p{c['p']}"))
    return c


# error rate and BP iterations per graph, chosen on the oracle alone so that
# every case meets check_ssf_conditions / check_bp_conditions
RATES = {"w128": (0.09, 3), "w236": (0.06, 3), "w238": (0.05, 2), "w247": (0.045, 3), "w248": (0.045, 3),
         "w268": (0.045, 5), "w498": (0.03, 3), "w247d0": (0.03, 3), "b300": (0.03, 4), "b300lds": (0.03, 4)}
D3R = {"w247": 2, "w247d0": 0}  # the min-sum wave kernels' D3R on the (2, 4, 7) graphs; 0 on every other shape


def wave_shape_of(key):
    return tuple(int(ch) for ch in key[1:4])


def wave_ssf_cases(key, n_gen, precision):
    """The decodes of one (wave graph, flip sets, precision): lean and full
    outputs x SSF kernel x fused or not x compact or one-pass x step bound."""
    rc, rv, drc = wave_shape_of(key)
    T, rg, d3r = TNAME[precision], 1 if n_gen <= 64 else 2, D3R.get(key, 0)
    p, it = RATES[key]
    out = []
    for lean, ssf, fuse, compact, steps in itertools.product((True, False), ("auto", "scan", "scan_gather",
                                                                            "scan_nosplit"), (0, 1), (1, 0), (0, 2)):
        if not lean and (fuse or not compact):
            continue  # full outputs: always the one-pass kernel, nothing to fuse into
        fused = lean and fuse and compact and ssf == "auto"
        if lean and compact:
            bp = f"qdec::bp_ms_cmp_kernel<{T}, {rc}, {rv}, {drc}, true, {d3r}, 0, {(rg if fused else 0)}>"
        else:
            bp = f"qdec::bp_ms_wave_kernel<{T}, {rc}, {rv}, {drc}, true, {'true' if lean else 'false'}, {d3r}, 0>"
        fin = "" if fused else f"qdec::ssf_lut_kernel<{rg}, {rv}, {rc}, {'true' if lean else 'false'}>" \
            if ssf == "auto" else f"qdec::ssf_wave_kernel<{rg}, {rv}, {rc}>"
        out.append(_case(key, n_gen=n_gen, max_lc=max_lc_of(n_gen), precision=precision,
                         options={"ssf": ssf, "ssf_fuse": fuse, "compact": compact},
                         want=LEAN_WANT if lean else SSF_WANT, p=p, max_iter=it, steps=steps, bp=bp, fin=fin,
                         pre=f"qdec::ms_triage_kernel<{rc}, {rv}, false>" if lean and compact else ""))
    return out


def wave_extra_cases(key):
    """Per wave graph: one packed-rows decode, product-sum with SSF (f32 and
    f64), and on (2, 4, 7) the three-waves-per-SIMD build, fused and not."""
    rc, rv, drc = wave_shape_of(key)
    p, it = RATES[key]
    d3r = D3R.get(key, 0)
    direct = rc == (graph(key)[0].shape[0] + 63) // 64  # the triage reads packed rows itself
    out = [_case(key, n_gen=64, max_lc=9, precision="f32", options={"ssf_fuse": 0}, want=LEAN_WANT, p=p, max_iter=it,
                 packed=True, bp=f"qdec::bp_ms_cmp_kernel<float, {rc}, {rv}, {drc}, true, {d3r}, 0, 0>",
                 fin=f"qdec::ssf_lut_kernel<1, {rv}, {rc}, true>",
                 pre=f"qdec::ms_triage_kernel<{rc}, {rv}, {'true' if direct else 'false'}>")]
    for precision, n_gen in (("f32", 65), ("f64", 40)):
        out.append(_case(key, n_gen=n_gen, max_lc=max_lc_of(n_gen), method="ps", precision=precision,
                         want=("x", "iters", "status", "ssf_steps"), p=p, max_iter=it,
                         bp=f"qdec::bp_wave_kernel<{TNAME[precision]}, 0, {rc}, {rv}, {drc}, true>",
                         fin=f"qdec::ssf_lut_kernel<{1 if n_gen <= 64 else 2}, {rv}, {rc}, false>", pre=""))
    if d3r == 2:
        for n_gen, fuse in ((64, 1), (128, 1), (64, 0)):
            rg = 1 if n_gen <= 64 else 2
            out.append(_case(key, n_gen=n_gen, max_lc=max_lc_of(n_gen), options={"ssf_fuse": fuse}, occ=12,
                             want=LEAN_WANT, p=p, max_iter=it,
                             bp=f"qdec::bp_ms_cmp_kernel<double, 2, 4, 7, true, 2, 3, {rg if fuse else 0}>",
                             fin="" if fuse else f"qdec::ssf_lut_kernel<{rg}, 4, 2, true>",
                             pre="qdec::ms_triage_kernel<2, 4, false>"))
    return out


def queue_ssf_cases():
    """Wave BP into the byte queue into a workgroup SSF kernel: (4, 9, 8), whose
    checks do not fit u8 ids, and more than 128 generators on (2, 4, 8) (300:
    beyond the 256 generators the wave inverse table indexes).  The workgroup SSF
    kernels record no name."""
    out = []
    for key, n_gen in (("w498", 40), ("w498", 128), ("w248", 150), ("w248", 300)):
        rc, rv, drc = wave_shape_of(key)
        p, it = RATES[key]
        for precision, inc in itertools.product(("f32", "f64"), (1, 0)):
            out.append(_case(key, n_gen=n_gen, max_lc=9, precision=precision, options={"ssf_inc": inc}, p=p,
                             max_iter=it, fin="", pre="", path=(1, 6 if inc else 7),
                             bp=f"qdec::bp_ms_wave_kernel<{TNAME[precision]}, {rc}, {rv}, {drc}, true, false, 0, 0>"))
    for precision in ("f32", "f64"):  # product-sum's DEFER build on the last shape
        p, it = RATES["w498"]
        out.append(_case("w498", n_gen=40, max_lc=9, method="ps", precision=precision, p=p, max_iter=it, fin="",
                         pre="", want=("x", "iters", "status", "ssf_steps"),
                         bp=f"qdec::bp_wave_kernel<{TNAME[precision]}, 0, 4, 9, 8, true>"))
    return out


def block_ssf_cases():
    """Workgroup graphs with 200 mixed generators: the workgroup kernel into the
    incremental and the re-scanning SSF kernel, the slot-group kernel, and the
    LDS-resident kernels on the graph within their degree bounds."""
    out = []
    p, it = RATES["b300"]
    for precision in ("f32", "f64"):
        T = TNAME[precision]
        # path: the plan's (QD_BP_*, QD_FIN_*); bp_block_kernel and the workgroup SSF kernels record no name
        for opts, bp, path in (({"group_kernel": 0}, "", (5, 6)), ({"group_kernel": 0, "ssf_inc": 0}, "", (5, 7)),
                               ({"group_kernel": 1}, f"qdec::bp_group_kernel<{T}, 1, 16, 8>", (3, 6))):
            out.append(_case("b300", n_gen=200, max_lc=9, precision=precision, options=opts, p=p, max_iter=it, bp=bp,
                             pre="", path=path))
        out.append(_case("b300lds", n_gen=200, max_lc=9, precision=precision, options={"lds_kernel": 1},
                         p=RATES["b300lds"][0], max_iter=RATES["b300lds"][1], pre="", path=(4, 6),
                         bp="qdec::bp_ms_lds_kernel<4>" if precision == "f32" else "qdec::bp_ms_lds64_kernel<4, 0>"))
    return out


# BP only: (error rate, the instantiation) per LDS-kernel graph
LDS_CELLS = {"lds8191": (0.06, 8), "lds12287": (0.03, 12), "lds16383": (0.02, 16), "lds8193": (0.06, 10),
             "lds4097": (0.05, 8)}
# ms_scaling = 0.625 (a constant factor) converges far less on these graphs (many
# columns of degree 1 and 2), and one iteration decodes only the lightest shots:
# their own, lower error rates
LDS_SCALED_RATE = {"lds8191": 0.004, "lds12287": 0.002, "lds16383": 0.002}
LDS_ONE_ITERATION_RATE = 0.0005
GROUP_CELLS = {"g88": (8, 8), "g164": (16, 4), "b300": (16, 8), "b300lds": (8, 4)}
GROUP_RATE = {"g88": 0.08, "g164": 0.04, "b300": 0.08, "b300lds": 0.04}


def lds_bp_cases(key):
    p, vpt = LDS_CELLS[key]
    full = key in ("lds8191", "lds12287", "lds16383")
    out = [_case(key, precision="f32", options={"lds_kernel": 1}, ssf=False, want=BP_WANT, B=64,
                 p=LDS_SCALED_RATE[key] if a else LDS_ONE_ITERATION_RATE if it == 1 else p, max_iter=it, scaling=a, bp=f"qdec::bp_ms_lds_kernel<{vpt}>", pre="")
           for it, a in (((20, 0.0), (20, 0.625), (1, 0.0)) if full else ((20, 0.0),))]
    if key == "lds12287":  # more than 10240 columns: the f64 LDS kernel does not apply, the slot-group kernel runs
        out.append(_case(key, precision="f64", options={"lds_kernel": 1}, ssf=False, want=BP_WANT, B=64, p=p,
                         max_iter=20, bp="qdec::bp_group_kernel<double, 1, 8, 4>", pre=""))
    return out


def group_bp_cases(key):
    dr, dc = GROUP_CELLS[key]
    return [_case(key, method=method, precision=precision, options={"group_kernel": 1}, ssf=False,
                  want=("x", "llr", "iters", "status"), B=B, p=GROUP_RATE[key], max_iter=25, pre="",
                  bp=f"qdec::bp_group_kernel<{TNAME[precision]}, {0 if method == 'ps' else 1}, {dr}, {dc}>")
            for method, precision, B in itertools.product(("ms", "ps"), ("f32", "f64"), (700, 5))]


# bp_ms_lds64_kernel<VPT, D3R>: columns j < n3 of degree 3, the rest of degree 4
# (as test_gpu_large_codes.test_lds64_kernel_degree3_rounds) -> (m, n, n3)
LDS64_CELLS = {"<8, 4>": (4000, 8000, 4500), "<8, 0>": (4000, 7000, 0), "<10, 3>": (4800, 9800, 3500),
               "<10, 0>": (4900, 9300, 0), "<10, 6>": (4800, 9800, 6500)}
for _inst, (_m, _n, _n3) in LDS64_CELLS.items():
    GRAPHS["lds64" + _inst] = functools.partial(
        lambda m, n, n3: _with_priors(column_graph(m, n, n + n3, np.where(np.arange(n) < n3, 3, 4), 8), n3 + 1, 0.005,
                                      0.03), _m, _n, _n3)
LDS64_RATE = 0.04


def lds64_bp_cases(inst):
    return [_case("lds64" + inst, precision="f64", options={"lds_kernel": 1}, ssf=False, want=BP_WANT, B=64,
                  p=LDS64_RATE, max_iter=20, bp="qdec::bp_ms_lds64_kernel" + inst, pre="")]


WAVE_KEYS = tuple("w%d%d%d" % s for s in SSF_WAVE_SHAPES)
# the (2, 4, 7) graph without 3-edge rounds ("w247d0") adds only what differs from
# "w247": the FUSE = 1 and FUSE = 2 builds with D3R = 0
WAVE_PARAMS = [(key, n_gen) for key in WAVE_KEYS for n_gen in WAVE_NGEN] + [("w247d0", 40), ("w247d0", 128)]


# The one list of what runs: group name -> (parameters, cases of one parameter).
# tests/test_gpu_ssf_mixed.py has one test function per group, parametrised by
# the group's parameters, and all_cases() (the CPU plans and the ledger) is
# their union, so a case the ledger counts is a case the GPU module launches.
GROUPS = {
    "wave_ssf": ([(key, n_gen, precision) for key, n_gen in WAVE_PARAMS for precision in ("f32", "f64")],
                 wave_ssf_cases),
    "wave_extra": ([(key,) for key in WAVE_KEYS + ("w247d0",)], wave_extra_cases),
    "queue_ssf": ([()], queue_ssf_cases),
    "block_ssf": ([()], block_ssf_cases),
    "lds_bp": ([(key,) for key in LDS_CELLS], lds_bp_cases),
    "lds64_bp": ([(inst,) for inst in LDS64_CELLS], lds64_bp_cases),
    "group_bp": ([(key,) for key in GROUP_CELLS], group_bp_cases),
}


def group_params(name):
    """pytest parameters of a group: its tuples, with readable ids."""
    import pytest
    return [pytest.param(p, id="-".join(map(str, p)) or "all") for p in GROUPS[name][0]]


def group_cases(name, param):
    return GROUPS[name][1](*param)


def all_cases():
    return [c for name, (params, _) in GROUPS.items() for p in params for c in group_cases(name, p)]


def plan_request(case):
    """(options with every default spelled out, present-buffer names) of a case."""
    opts = {"compact": 1, "triage_it1": 1, "ssf": "auto", "lds_kernel": -1, "group_kernel": -1, "ssf_inc": 1,
            "block_wg": 0, "group_mb": 0, "ssf_fuse": 0}
    opts.update(case["options"])
    present = ["syn"] + [k for k in ("x", "corr", "llr", "fail") if k in case["want"]]
    if "fail" in case["want"]:
        present.append("readout")
    return opts, tuple(present)


# ---------------------------------------------------------------- oracle side
def oracle_decode(oracle_lib, case):
    H, probs, L = graph(case["graph"])
    syn, rd = case_shots(case)
    gens = flip_sets(case["graph"], case["n_gen"], case["max_lc"]) if case["ssf"] else None
    return oracle_lib.decode(H, probs, syn, method=case["method"], precision=case["precision"],
                             max_iter=case["max_iter"], ms_scaling=case["scaling"], ssf=case["ssf"],
                             ssf_max_steps=case["steps"], gens=gens, lz=L if case["ssf"] else None,
                             readout=rd if case["ssf"] else None, want_llr="llr" in case["want"], ssf_impl="fast")


def distinct_winners(gens, ref, bp):
    """A lower bound on the number of distinct generators that won an SSF step:
    a shot with one step changed exactly a subset of its winner, so changed sets
    whose candidate generators (equal supports counted once) are pairwise
    disjoint had different winners."""
    gens = sp.csr_matrix(gens)
    supp = sorted({tuple(gens.indices[gens.indptr[g]:gens.indptr[g + 1]]) for g in range(gens.shape[0])})
    cands = set()
    for b in np.flatnonzero(ref["ssf_steps"] == 1):
        S = set(np.flatnonzero(ref["x"][b] ^ bp["x"][b]).tolist())
        if S:
            cands.add(frozenset(i for i, g in enumerate(supp) if S <= set(g)))
    taken, count = set(), 0
    for c in sorted(cands, key=len):
        assert c, "a changed set no generator holds"
        if not (c & taken):
            taken |= c
            count += 1
    return count


def check_ssf_conditions(case, ref, gens, bp, free=None):
    """What keeps an SSF case from passing vacuously, on the oracle's outputs
    (ref: with SSF; bp: the same decode without; free: for a case with a step
    bound, the same decode without the bound).  Shots with a zero syndrome count
    for nothing: BP has nothing to do on them and the triage removes them, so
    the converged share is taken over shots whose syndrome is not zero."""
    B = case["B"]
    nz = case_shots(case)[0].any(axis=1)
    conv = (ref["status"] & 1).astype(bool)
    assert (conv & nz).sum() >= 0.15 * B and (~conv).sum() >= 0.15 * B, (case["id"], (conv & nz).sum(), (~conv).sum())
    # and as many by the BP kernel's own iterations (iteration 1 may be the triage's tables)
    assert (conv & (ref["iters"] >= 2)).sum() >= 0.15 * B, (case["id"], (conv & (ref["iters"] >= 2)).sum())
    assert ref["ssf_steps"].sum() >= B / 2, (case["id"], ref["ssf_steps"].sum())
    fixed = ~conv & ((ref["status"] & 2) != 0)
    assert fixed.any() and (~conv & ((ref["status"] & 2) == 0)).any(), case["id"]
    assert distinct_winners(gens, ref, bp) >= 8, (case["id"], distinct_winners(gens, ref, bp))
    if case["steps"]:  # cut at the bound: the unbounded decode takes more steps
        assert free is not None and (free["ssf_steps"] > case["steps"]).any(), case["id"]
        assert (ref["ssf_steps"][free["ssf_steps"] > case["steps"]] == case["steps"]).all(), case["id"]


def check_bp_conditions(case, ref):
    """Every BP-only case: among the shots whose syndrome is not zero, converged
    and unconverged ones, and at least 3 distinct iteration counts.  A case of
    one iteration can only count 1, so there the second condition cannot hold
    and only the first is asserted."""
    nz = case_shots(case)[0].any(axis=1)
    conv = (ref["status"] & 1).astype(bool)
    assert (conv & nz).any() and (~conv).any(), (case["id"], conv.mean())
    if case["max_iter"] > 1:
        assert len(set(ref["iters"][nz].tolist())) >= 3, (case["id"], sorted(set(ref["iters"][nz].tolist())))
