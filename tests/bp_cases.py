"""Decode cases of the BP kernel instantiations outside the ledger of
tests/test_ssf_mixed_host.py, shared by tests/test_bp_ledger_host.py (CPU: plans,
the second ledger, the conditions that keep a case from passing vacuously) and
tests/test_gpu_bp_ledger.py (GPU: parity with the oracle).

Two kinds of case.  Wave graphs without SSF: the DEFER = false builds of
bp_ms_wave_kernel, bp_ms_cmp_kernel and bp_wave_kernel on every wave shape, with
the triage reading byte and packed rows.  Workgroup graphs: every cell of
bp_block_kernel -- unrolled or generic body x placement 3 / 2 / 0 x product-sum
or min-sum x f32 or f64 x DEFER or not -- with both workgroup SSF kernels behind
the DEFER builds.

The graphs, flip sets and wave shots are those of tests/ssf_cases.py; the
workgroup graphs are added to its GRAPHS.  Everything is generated from seeds;
nothing here needs a GPU."""
import functools
import itertools

import numpy as np
import scipy.sparse as sp

import ssf_cases as sc
from ssf_cases import TNAME, _with_priors, column_graph, row_graph

FULL_WANT = ("x", "corr", "llr", "iters", "status", "fail")
LEAN_WANT = ("iters", "status", "fail")
PS_WANT = ("x", "llr", "iters", "status")
WAVE_B = (65, 257)  # one 64-shot triage tile plus one shot; several tiles and a ragged tail
MAX_ITER = 25
N_GEN, MAX_LC = 40, 9  # flip sets of the DEFER cases on workgroup graphs
POOL = 130             # shots drawn per workgroup graph; the 5-shot cases take a window of them
# 130 shots are fewer than the workgroups of one launch on a 256-CU device (the grid is the resident
# workgroups, at most 8 of 256 threads per CU, cut to the batch), so there every workgroup sees one shot.
# A third batch size makes the strided loop (placement 3) and the dynamic shot counter (placement 2, held to
# one workgroup per CU by block_wg = 1) hand a workgroup more than one: placement -> (shots, workgroups per CU)
MANY = {3: (2600, 8), 2: (600, 1)}


# ---------------------------------------------------------------- workgroup graphs
def _extra_rows(H, seed, degrees):
    """H with one more row per entry of degrees, on random columns."""
    rng = np.random.default_rng(seed)
    n = H.shape[1]
    rows = [np.sort(rng.choice(n, d, replace=False)) for d in degrees]
    ptr = np.cumsum([0] + [len(r) for r in rows])
    X = sp.csr_matrix((np.ones(ptr[-1], np.uint8), np.concatenate(rows), ptr), shape=(len(rows), n))
    out = sp.vstack([sp.csr_matrix(H), X]).tocsr()
    out.sort_indices()
    return out


def _relay_wide_row():
    import relay_cases as rc
    g = rc.graph("h35w17")
    return g["H"], g["probs"], g["lz"]


def _choice_degrees(n, seed, values, probs):
    return np.random.default_rng(seed).choice(values, size=n, p=probs)


# name -> builder of (H, priors, logicals).  Sizes are the smallest that plan the
# cell (block_placement, qdec_launch_block.hip: the messages 2 E sizeof(T) and the
# shot state n_pad + 2 m_pad against 64 KB of LDS); odd m and n, ragged degrees,
# rows of degree 0 and 1 and columns of degree 0 where the cell allows.
BLOCK_GRAPHS = {
    # generic body (a row beyond 16 or a column beyond 8), everything in LDS: the
    # 4 x 21 graph with one row of 17, and 302 x 523 (the 256-thread strides wrap)
    # with rows of 19 and 23 next to rows of 0 .. 9
    "gen3s": _relay_wide_row,
    "gen3": lambda: _with_priors(_extra_rows(row_graph(300, 523, 523, 0, 9, 5), 524, (19, 23)), 525, 0.01, 0.08),
    # generic, messages in HBM: 2 E sizeof(float) > 64 KB, rows of about 32
    "gen2": lambda: _with_priors(_extra_rows(column_graph(257, 2051, 2051, _choice_degrees(
        2051, 2052, (0, 1, 3, 4, 5), (.01, .04, .15, .5, .3)), 64), 2053, (1, 0)), 2054, 0.002, 0.012),
    # generic, shot state in HBM too (n_pad + 2 m_pad beyond 64 KB): the unrolled placement-0
    # graph below with rows of 1031 and 997 on top (columns of degree 1 under rows that wide
    # alone leave product-sum nothing to decode), and columns of degree 9 over rows of at most 4
    "gen0r": lambda: _with_priors(_extra_rows(sc.graph("unr0")[0], 65701, (1031, 997, 1)), 65703, 0.003, 0.02),
    "gen0c": lambda: _with_priors(column_graph(21001, 24001, 24001, _choice_degrees(
        24001, 24002, (0, 1, 2, 3, 9), (.01, .1, .4, .44, .05)), 4), 24003, 0.005, 0.04),
    # unrolled body (rows <= 16, columns <= 8): ssf_cases' "b300" at placement 3, then
    # messages in HBM and shot state in HBM
    "unr2": lambda: _with_priors(column_graph(1501, 2999, 2999, _choice_degrees(
        2999, 3000, (0, 1, 2, 3, 4), (.01, .05, .14, .5, .3)), 7), 3001, 0.005, 0.04),
    "unr0": lambda: _with_priors(column_graph(13001, 39999, 39999, _choice_degrees(
        39999, 40000, (0, 1, 2, 3, 4), (.01, .14, .3, .45, .1)), 10), 40001, 0.003, 0.02),
}
sc.GRAPHS.update(BLOCK_GRAPHS)

_NO_ALT = {"group_kernel": 0, "lds_kernel": 0}  # keep the slot-group and LDS-resident kernels away
# graph -> (DRM, DCM of the body, placement, options, batch sizes)
BLOCK_CELLS = {
    "gen3s": ((0, 0), 3, {}, (5, 130, 2600)),
    "gen3": ((0, 0), 3, {}, (5, 130, 2600)),
    "gen2": ((0, 0), 2, {}, (5, 130, 600)),
    "gen0r": ((0, 0), 0, {}, (5,)),
    "gen0c": ((0, 0), 0, {}, (5,)),
    "b300": ((16, 8), 3, _NO_ALT, (5, 130, 2600)),
    "unr2": ((16, 8), 2, _NO_ALT, (5, 130, 600)),
    "unr0": ((16, 8), 0, _NO_ALT, (5,)),
}
# one graph per body also takes its syndrome from base and readout (syn_flags = 3)
SYN_FLAGS_GRAPHS = ("gen3s", "b300")

# Error rate, BP iterations, and the first shot of the 5-shot window, per
# workgroup graph and (method, precision); error rate and iterations per wave
# graph.  Chosen on the oracle alone (test_bp_ledger_host.test_cases_are_not_vacuous)
# so that every case meets check_conditions.
BLOCK_RATES = {
    # f32 min-sum reaches a marginal of exactly 0 on the row of 17 (decided as 1) and
    # so converges at iteration 25 on every shot f64 leaves open: 12 iterations there
    "gen3s": {("ms", "f32"): (0.08, 12, 22), None: (0.08, 25, 22)},
    "gen3": {None: (0.08, 25, 0)},
    "gen2": {"ms": (0.03, 25, 4), "ps": (0.05, 25, 0)},
    "gen0r": {"ms": (0.08, 25, 4), "ps": (0.012, 25, 11)},
    "gen0c": {"ms": (0.4, 25, 0), ("ps", "f32"): (0.3, 25, 0), ("ps", "f64"): (0.4, 25, 0)},
    "b300": {None: (0.08, 25, 0)},
    "unr2": {None: (0.08, 25, 0)},
    "unr0": {"ms": (0.08, 25, 0), "ps": (0.012, 25, 1)},
}
WAVE_RATES = {"w128": (0.09, 20), "w236": (0.09, 20), "w238": (0.09, 20), "w247": (0.09, 20), "w248": (0.09, 20),
              "w268": (0.06, 20), "w498": (0.06, 20), "w247d0": (0.09, 20)}


def block_rate(key, method, precision):
    """(error rate, iterations, window start): the entry of (method, precision),
    else of the method, else the graph's."""
    rates = BLOCK_RATES[key]
    return rates.get((method, precision)) or rates.get(method) or rates[None]


# ---------------------------------------------------------------- shots
@functools.lru_cache(maxsize=None)
def block_shots(key, p, pool=POOL):
    """(syn, base, readout) of the pool of shots of a workgroup graph: shot b has
    error rate RATE_CLASSES[b % 4] * p; base is random and readout = base ^ error,
    so base ^ readout gives the same syndrome and the failure flag is the
    correction's logical error."""
    H = sc.graph(key)[0]
    n = H.shape[1]
    rng = np.random.default_rng(n + 17)
    rate = (np.array(sc.RATE_CLASSES)[np.arange(pool) % 4] * p)[:, None]
    e = (rng.random((pool, n)) < rate).astype(np.uint8)
    syn = np.ascontiguousarray((H @ e.T).T % 2).astype(np.uint8)
    base = (rng.random((pool, n)) < 0.1).astype(np.uint8)
    return syn, base, base ^ e


def case_inputs(case):
    """dict(syn, base, readout, nz) of a case: the decode's inputs (None for a
    buffer it does not pass) and which shots have a non-zero syndrome."""
    if case["kind"] == "wave":
        syn, rd = sc.case_shots(case)
        return dict(syn=syn, base=None, readout=rd, nz=syn.any(axis=1))
    lo = case["offset"]
    syn, base, rd = (a[lo:lo + case["B"]] for a in block_shots(case["graph"], case["p"], max(POOL, case["B"])))
    nz = syn.any(axis=1)
    if case["syn_flags"]:
        return dict(syn=None, base=base, readout=rd, nz=nz)
    return dict(syn=syn, base=None, readout=rd, nz=nz)


# ---------------------------------------------------------------- cases
def _case(kind, graph, syn_flags=0, **kw):
    c = sc._case(graph, **kw)
    c.update(kind=kind, syn_flags=syn_flags)
    c["id"] += f"-f{syn_flags}-" + ",".join(c["want"])
    return c


def wave_bp_cases(key):
    """BP only on one wave graph, f32 and f64, 65 and 257 shots: min-sum with all
    outputs, lean one-pass, lean compact behind the triage, lean compact from
    packed rows; product-sum with x and LLRs.  Where the graph has two 3-edge
    rounds (D3R = 2), the three-waves-per-SIMD f64 builds: one-pass, compact, and
    the deferring one-pass build into the table-driven SSF kernel."""
    rc, rv, drc = sc.wave_shape_of(key)
    d3r = sc.D3R.get(key, 0)
    p, it = WAVE_RATES[key]
    direct = rc == (sc.graph(key)[0].shape[0] + 63) // 64  # the triage reads packed rows itself
    out = []
    for precision, B in itertools.product(("f32", "f64"), WAVE_B):
        T = TNAME[precision]
        kw = dict(precision=precision, ssf=False, B=B, p=p, max_iter=it, fin="")
        one = f"qdec::bp_ms_wave_kernel<{T}, {rc}, {rv}, {drc}, false, %s, {d3r}, 0>"
        cmp_k = f"qdec::bp_ms_cmp_kernel<{T}, {rc}, {rv}, {drc}, false, {d3r}, 0, 0>"
        out += [
            _case("wave", key, want=FULL_WANT, bp=one % "false", pre="", **kw),
            _case("wave", key, want=LEAN_WANT, options={"compact": 0}, bp=one % "true", pre="", **kw),
            _case("wave", key, want=LEAN_WANT, bp=cmp_k, pre=f"qdec::ms_triage_kernel<{rc}, {rv}, false>", **kw),
            _case("wave", key, want=LEAN_WANT, packed=True, bp=cmp_k,
                  pre=f"qdec::ms_triage_kernel<{rc}, {rv}, {'true' if direct else 'false'}>", **kw),
            _case("wave", key, method="ps", want=PS_WANT, bp=f"qdec::bp_wave_kernel<{T}, 0, {rc}, {rv}, {drc}, false>",
                  pre="", **kw),
        ]
    if d3r == 2:
        for B in WAVE_B:
            kw = dict(precision="f64", occ=12, want=LEAN_WANT, B=B, p=p, max_iter=it)
            out += [
                _case("wave", key, ssf=False, options={"compact": 0}, fin="", pre="",
                      bp="qdec::bp_ms_wave_kernel<double, 2, 4, 7, false, true, 2, 3>", **kw),
                _case("wave", key, ssf=False, fin="", pre="qdec::ms_triage_kernel<2, 4, false>",
                      bp="qdec::bp_ms_cmp_kernel<double, 2, 4, 7, false, 2, 3, 0>", **kw),
                _case("wave", key, n_gen=64, max_lc=9, options={"compact": 0}, pre="",
                      bp="qdec::bp_ms_wave_kernel<double, 2, 4, 7, true, true, 2, 3>",
                      fin="qdec::ssf_lut_kernel<1, 4, 2, true>", **dict(kw, want=LEAN_WANT + ("ssf_steps",))),
            ]
    return out


def block_cases(key, method):
    """One workgroup graph and BP method, f32 and f64, every batch size of the
    cell: BP only with all six outputs (DEFER = false), and BP into the
    incremental and into the re-scanning workgroup SSF kernel (DEFER = true; at
    placement 0 the plan has one SSF kernel, with its shot state in HBM).  The
    batch of MANY runs BP only and BP into the incremental SSF kernel."""
    (drm, dcm), placement, options, sizes = BLOCK_CELLS[key]
    out = []
    for precision, B in itertools.product(("f32", "f64"), sizes):
        p, it, lo = block_rate(key, method, precision)
        kw = dict(method=method, precision=precision, B=B, p=p, max_iter=it, pre="", offset=lo if B == 5 else 0)
        opts = dict(options, block_wg=MANY[2][1]) if B > POOL and placement == 2 else options
        name = f"qdec::bp_block_kernel<{TNAME[precision]}, {0 if method == 'ps' else 1}, %s, {drm}, {dcm}>"
        out.append(_case("block", key, ssf=False, want=FULL_WANT, options=opts, bp=name % "false", fin="",
                         path=(5, 0, placement), **kw))
        if key in SYN_FLAGS_GRAPHS and B == POOL:
            out.append(_case("block", key, syn_flags=3, ssf=False, want=FULL_WANT, options=opts,
                             bp=name % "false", fin="", path=(5, 0, placement), **kw))
        for inc in (1, 0) if placement and B <= POOL else (1,):
            fin = 8 if placement == 0 else 6 if inc else 7
            out.append(_case("block", key, n_gen=N_GEN, max_lc=MAX_LC, want=sc.SSF_WANT,
                             options=dict(opts, ssf_inc=inc), bp=name % "true", path=(5, fin, placement),
                             fin="qdec::ssf_inc_block_kernel" if fin == 6 else "qdec::ssf_block_kernel", **kw))
    return out


# The one list of what runs, as ssf_cases.GROUPS: group name -> (parameters, cases
# of one parameter).  tests/test_gpu_bp_ledger.py has one test function per group.
WAVE_KEYS = tuple("w%d%d%d" % s for s in sc.SSF_WAVE_SHAPES + ((4, 9, 8),)) + ("w247d0",)
GROUPS = {
    "wave_bp": ([(key,) for key in WAVE_KEYS], wave_bp_cases),
    "block_bp": ([(key, method) for key in BLOCK_CELLS for method in ("ms", "ps")], block_cases),
}


def group_params(name):
    import pytest
    return [pytest.param(p, id="-".join(map(str, p))) for p in GROUPS[name][0]]


def group_cases(name, param):
    return GROUPS[name][1](*param)


def all_cases():
    return [c for name, (params, _) in GROUPS.items() for p in params for c in group_cases(name, p)]


def plan_request(case):
    """(options with every default spelled out, present-buffer names) of a case."""
    opts, present = sc.plan_request(case)
    if case["syn_flags"]:
        present = ("base",) + tuple(k for k in present if k != "syn")
    if "readout" not in present and (case["syn_flags"] or case["ssf"]):
        present += ("readout",)
    return opts, present


# ---------------------------------------------------------------- oracle side
def oracle_decode(oracle_lib, case):
    H, probs, L = sc.graph(case["graph"])
    inp = case_inputs(case)
    gens = sc.flip_sets(case["graph"], case["n_gen"], case["max_lc"]) if case["ssf"] else None
    return oracle_lib.decode(H, probs, inp["syn"], method=case["method"], precision=case["precision"],
                             max_iter=case["max_iter"], ms_scaling=case["scaling"], ssf=case["ssf"],
                             ssf_max_steps=case["steps"], gens=gens, lz=L, base=inp["base"], readout=inp["readout"],
                             syn_flags=case["syn_flags"], B=case["B"], want_llr="llr" in case["want"],
                             ssf_impl="fast")


def oracle_key(case):
    """Cases with the same key decode the same thing (the kernel options and the
    outputs asked for do not change what is computed)."""
    return (case["graph"], case["n_gen"], case["max_lc"], case["method"], case["precision"], case["max_iter"],
            case["steps"], case["scaling"], case["B"], case["offset"], case["p"], case["ssf"], case["syn_flags"],
            "llr" in case["want"])


def check_conditions(case, ref):
    """What keeps a case from passing vacuously, on the oracle's outputs: among
    the shots whose syndrome is not zero some converge and some do not, the
    iteration counts take at least three values, and a case with SSF behind BP
    queues at least one shot and takes at least one step."""
    nz = case_inputs(case)["nz"]
    conv = (ref["status"] & 1).astype(bool)
    assert (conv & nz).any() and (~conv).any(), (case["id"], int((conv & nz).sum()), int((~conv).sum()))
    iters = sorted(set(ref["iters"][nz].tolist()))
    assert len(iters) >= min(3, case["max_iter"]), (case["id"], iters)
    if case["ssf"]:
        assert ref["ssf_steps"].sum() >= 1, case["id"]
