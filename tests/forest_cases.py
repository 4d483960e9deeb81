"""Forest graphs and BP-only decode cases whose reference is the exact model of
tests/forest_model.py, shared by tests/test_forest_host.py (CPU: the oracle
against the model, plans, the conditions that keep a case from passing
vacuously) and tests/test_gpu_forest.py (GPU: every kernel family against the
model).

The graphs are registered in ssf_cases.GRAPHS, so the plan helpers of the two
ledgers work on them unchanged.  Product-sum, and min-sum with ms_scaling = 1
(scaled min-sum is not a marginal of anything); f32 and f64.  Everything is
generated from seeds; nothing here needs a GPU."""
import functools
import itertools
import re

import numpy as np

import bp_cases as bc
import forest_model as fm
import ssf_cases as sc
from forest_model import Template as T
from ssf_cases import TNAME

MAX_ITER = 6
FULL_WANT = ("x", "llr", "iters", "status")
LEAN_WANT = ("iters", "status")
LDS_WANT = ("x", "iters", "status")   # the LDS-resident kernels write no LLRs
WAVE_B = (65, 257)

# The oracle's largest deviation from the model over the cases of this file,
# |oracle - exact| / max(1, |exact|) on finite beliefs, measured on the CPU
# (test_forest_host.test_oracle_equals_the_model prints them).  The host test
# allows twice the figure; the GPU test adds the kernel-against-oracle tolerance
# of test_gpu_parity._cmp_llr on top (nothing for min-sum, rtol 1e-12 / 1e-6 for
# product-sum).  Nothing here was tuned on a kernel's output.
ORACLE_DEV = {
    ("ps", "f64"): 6.16e-15,   # measured 6.16e-15
    ("ps", "f32"): 3.54e-6,    # measured 3.54e-06
    ("ms", "f64"): 1.22e-15,   # measured 1.22e-15
    ("ms", "f32"): 4.41e-7,    # measured 4.41e-07
}
ORACLE_ABS_F32 = 1.64e-5   # measured 1.64e-05: the largest absolute f32 deviation, either method
GUARD = 64 * ORACLE_ABS_F32  # no belief of any case, at any iteration, is smaller than this
# No finite belief is larger than this (forest_model.settle: beyond it f32 probability
# ratios, not belief propagation, decide what product-sum returns)
CAP = 8.0
KERNEL_RTOL = {("ps", "f64"): 1e-12, ("ps", "f32"): 1e-6, ("ms", "f64"): 0.0, ("ms", "f32"): 0.0}


def host_tol(method, precision):
    return 2 * ORACLE_DEV[method, precision]


def gpu_tol(method, precision):
    return host_tol(method, precision) + KERNEL_RTOL[method, precision]


# ---------------------------------------------------------------- templates
# Degree-2 checks hand a message on whole, so beliefs add up along a path and
# around a high-degree variable: those templates draw flatter priors to stay
# below CAP.
FLAT, FLATTER = (0.25, 0.42), (0.32, 0.45)
ISO = T("iso", [], hot=True)                         # column of degree 0
ONE = T("one", [(0, 0)], hot=True)                   # a check of degree 1 alone: +-inf
PAIR = T("pair", [(0, 1)], hot=True)
PIN = T("pin", [(0, 2), (1, 0)], hot=True)           # a degree-1 check forces one of three
FAN = T("fan", [(0, 3)])
CHAIN = T("chain", [(0, 1), (1, 2)])
TWIG = T("twig", [(0, 2), (1, 1), (3, 2), (4, 1)], prior=FLAT)
PATH = T("path", [(i, 1) for i in range(11)], prior=FLATTER)   # radius 11 > MAX_ITER
BRANCH = T("branch", [(0, 2), (1, 1), (3, 1), (4, 2), (5, 1), (7, 1), (8, 1)], prior=FLATTER)


def star(dc):
    """A variable of degree dc under checks of degree 2 (one of degree 3)."""
    return T(f"star{dc}", [(0, 2)] + [(0, 1)] * (dc - 1), prior=FLAT if dc <= 4 else FLATTER)


def wide(dr, tail=((1, 1), (2, 1))):
    """A check of degree dr; two of its variables carry a degree-2 check."""
    return T(f"wide{dr}", [(0, dr - 1)] + list(tail))


def _fill(parts, m, n, cycle):
    """parts plus copies of the templates of cycle, then lone degree-1 checks
    and isolated variables, up to exactly m checks and n variables."""
    count = {}
    for t, K in parts:
        count[t] = count.get(t, 0) + K
    rm = m - sum(t.c * K for t, K in count.items())
    rn = n - sum(t.k * K for t, K in count.items())
    progress = True
    while progress:
        progress = False
        for t in cycle:
            if rm - t.c >= 1 and rn - t.k >= rm - t.c + 2:
                count[t] = count.get(t, 0) + 1
                rm, rn, progress = rm - t.c, rn - t.k, True
    assert rm >= 1 and rn - rm >= 2, (m, n, rm, rn)
    count[ONE] = count.get(ONE, 0) + rm
    count[ISO] = count.get(ISO, 0) + rn - rm
    return list(count.items())


SMALL = (CHAIN, FAN, PAIR, PIN, TWIG)
# name -> (m, n, required templates, filler cycle, (prior lo, hi), error rates of the shots by
# shot index, shots in the pool).  Sizes are the smallest that plan the cell: one below the
# wave shape's limits; workgroup graphs as tests/bp_cases.py sizes them.
SPECS = {
    # wave shapes (1, 2, 8), (2, 4, 7), (4, 9, 8): a row of the shape's DRC, a column of kDC = 4
    "fw128": (63, 127, [(wide(8), 2), (star(4), 3), (PATH, 2), (BRANCH, 1)], SMALL, 257),
    "fw247": (127, 255, [(wide(7), 3), (star(4), 6), (PATH, 4), (BRANCH, 3)], SMALL, 257),
    "fw498": (255, 575, [(wide(8), 6), (star(4), 12), (PATH, 8), (BRANCH, 6)], SMALL + (wide(6, ()),), 257),
    # workgroup kernel, unrolled body (rows <= 16, columns <= 8), everything in LDS; also bp_group_kernel's (16, 8)
    "fb3u": (301, 521, [(wide(16, ((1, 1),)), 2), (star(8), 4), (PATH, 6), (BRANCH, 5), (wide(9), 3)], SMALL, 130),
    # generic body: a row of 17 (k = 18) and a column of degree 9 under checks of degree 2
    "fb3g": (121, 263, [(wide(17, ((1, 1),)), 1), (T("star9", [(0, 1)] * 9, prior=FLATTER), 2), (PATH, 3),
                        (BRANCH, 2)], SMALL, 2600),
    # messages in HBM: 2 E sizeof(float) > 64 KB
    "fb2": (3601, 7001, [(wide(16, ((1, 1),)), 3), (star(8), 40), (PATH, 60), (BRANCH, 150), (wide(9), 30)],
            SMALL + (star(4),), 130),
    # shot state in HBM too: n_pad + 2 m_pad > 64 KB; templates of at most 10 variables
    "fb0": (16001, 34001, [(wide(8), 60), (star(8), 60), (BRANCH, 500)], SMALL + (star(4),), 48),
    # degrees within (8, 4), not a wave graph: bp_group_kernel's (8, 4) and the LDS-resident kernels
    "fg84": (401, 701, [(wide(8), 6), (star(4), 12), (PATH, 8), (BRANCH, 6)], SMALL, 130),
}
PRIORS = (0.06, 0.25)
# error rate of shot b: RATES[key][b % len]; light shots that converge next to heavy ones that do not
# (product-sum converges only while every check with syndrome 1 has a variable that outweighs the others)
RATES = {key: tuple(a / spec[1] for a in (0.7, 1.5, 3, 6, 15)) + (0.06, 0.2, 0.4) for key, spec in SPECS.items()}


class Bundle:
    """A forest with its pool of shots, settled (forest_model.settle) and
    decoded by the model once."""

    def __init__(self, key):
        m, n, parts, cycle, pool = SPECS[key]
        seed = sum(key.encode()) * 1000 + n
        self.forest = fm.Forest(_fill(parts, m, n, cycle), seed, *PRIORS)
        assert (self.forest.m, self.forest.n) == (m, n)
        self.e, self.rate = fm.sample_errors(self.forest, RATES[key], pool, seed + 1)
        self.redraws = fm.settle(self.forest, self.e, self.rate, MAX_ITER, GUARD, CAP, seed + 2)
        self.syn = self.forest.syndrome(self.e)
        self.model = self.forest.decode(self.e, MAX_ITER)
        for a in [self.e, self.syn, self.forest.probs] + [v for d in self.model.values() for v in d.values()]:
            a.setflags(write=False)

    def triple(self):
        return self.forest.H, self.forest.probs, self.forest.logicals


@functools.lru_cache(maxsize=None)
def bundle(key):
    return Bundle(key)


for _key in SPECS:
    sc.GRAPHS[_key] = functools.partial(lambda k: bundle(k).triple(), _key)


# ---------------------------------------------------------------- non-vacuity
def conditions(ref, nz):
    """What keeps a case from passing vacuously, on the model's outputs of its
    shots; among the shots with a non-zero syndrome: some converge at t >= 2,
    some do not converge, at least three iteration counts occur, one stops at a
    t smaller than its deepest component's radius, and one holds a variable
    whose decision differs between iterations t - 1 and t.  Returns the first
    condition that fails, or None."""
    conv = (ref["status"] & 1).astype(bool) & nz
    if not (conv & (ref["iters"] >= 2)).any():
        return "no shot converges at t >= 2"
    if not (nz & ~conv).any():
        return "every shot converges"
    if len(set(ref["iters"][nz].tolist())) < 3:
        return "fewer than three iteration counts"
    if not (conv & (ref["iters"] < ref["deep"])).any():
        return "no shot stops before its deepest component is crossed"
    if not (nz & ref["flip"]).any():
        return "no decision changes in the last iteration"
    return None


def window(key, method, B):
    """First shot of a case's window into the pool: 0 unless the case takes 5
    shots, then the first window that meets conditions (on the model alone)."""
    bd = bundle(key)
    if B != 5:
        return 0
    nz = bd.syn.any(axis=1)
    for lo in range(len(nz) - 4):
        sl = slice(lo, lo + 5)
        if conditions({k: v[sl] for k, v in bd.model[method].items()}, nz[sl]) is None:
            return lo
    raise AssertionError(f"no 5-shot window of {key} meets the conditions for {method}")


def case_shots(case):
    """(syn, model outputs) of a case's shots."""
    bd = bundle(case["graph"])
    lo = window(case["graph"], case["method"], case["B"])
    sl = slice(lo, lo + case["B"])
    return bd.syn[sl], {k: v[sl] for k, v in bd.model[case["method"]].items()}


# ---------------------------------------------------------------- cases
def _case(graph, **kw):
    kw.setdefault("want", FULL_WANT)
    kw.setdefault("fin", "")
    c = sc._case(graph, ssf=False, max_iter=MAX_ITER, p=0.0, **kw)
    c.update(kind="forest", syn_flags=0, scaling=1.0 if c["method"] == "ms" else 0.0)
    c["id"] = c["id"].replace("-a0.0-", f"-a{c['scaling']}-") + "-" + ",".join(c["want"])
    return c


def wave_cases(key):
    """One wave forest, f32 and f64, 65 and 257 shots: min-sum with all outputs,
    lean one-pass, lean compact behind the triage from byte and from packed
    rows; product-sum with all outputs.

    fw247 with 65 byte rows in f64 is the decode on which the first two-pass
    launch of a handle once faulted: the compact lists' counters were zeroed on
    the null stream, unordered with the handle's non-blocking stream
    (qdec_abi.cpp, attach_queue)."""
    rc, rv, drc = sc.wave_shape_of(key[1:])
    d3r = D3R.get(key, 0)
    direct = rc == (SPECS[key][0] + 63) // 64  # the triage reads packed rows itself
    out = []
    for precision, B in itertools.product(("f32", "f64"), WAVE_B):
        Tn = TNAME[precision]
        kw = dict(precision=precision, B=B)
        one = f"qdec::bp_ms_wave_kernel<{Tn}, {rc}, {rv}, {drc}, false, %s, {d3r}, 0>"
        cmp_k = f"qdec::bp_ms_cmp_kernel<{Tn}, {rc}, {rv}, {drc}, false, {d3r}, 0, 0>"
        out += [
            _case(key, bp=one % "false", pre="", **kw),
            _case(key, want=LEAN_WANT, options={"compact": 0}, bp=one % "true", pre="", **kw),
            _case(key, want=LEAN_WANT, bp=cmp_k, pre=f"qdec::ms_triage_kernel<{rc}, {rv}, false>", **kw),
            _case(key, want=LEAN_WANT, packed=True, bp=cmp_k,
                  pre=f"qdec::ms_triage_kernel<{rc}, {rv}, {'true' if direct else 'false'}>", **kw),
            _case(key, method="ps", bp=f"qdec::bp_wave_kernel<{Tn}, 0, {rc}, {rv}, {drc}, false>", pre="", **kw),
        ]
    return out


D3R = {"fw247": 2}  # the min-sum wave kernels' D3R on the (2, 4, 7) forest: two rounds of columns of degree <= 3
# graph -> (DRM, DCM of the body, placement, options, batch sizes)
BLOCK_CELLS = {
    "fb3u": ((16, 8), 3, bc._NO_ALT, (5, 130)),
    "fb3g": ((0, 0), 3, {}, (5, 130, 2600)),
    "fb2": ((16, 8), 2, bc._NO_ALT, (5, 130)),
    "fb0": ((16, 8), 0, bc._NO_ALT, (5,)),
}


def block_cases(key):
    (drm, dcm), placement, options, sizes = BLOCK_CELLS[key]
    return [_case(key, method=method, precision=precision, B=B, options=options, pre="", path=(5, 0, placement),
                  bp=f"qdec::bp_block_kernel<{TNAME[precision]}, {0 if method == 'ps' else 1}, false, {drm}, {dcm}>")
            for method, precision, B in itertools.product(("ms", "ps"), ("f32", "f64"), sizes)]


GROUP_CELLS = {"fg84": (8, 4), "fb3u": (16, 8)}


def group_cases(key):
    dr, dc = GROUP_CELLS[key]
    return [_case(key, method=method, precision=precision, B=B, options={"group_kernel": 1}, pre="",
                  bp=f"qdec::bp_group_kernel<{TNAME[precision]}, {0 if method == 'ps' else 1}, {dr}, {dc}>")
            for method, precision, B in itertools.product(("ms", "ps"), ("f32", "f64"), (5, 130))]


def lds_cases():
    """The LDS-resident kernels hand every shot to the finalize queue, SSF or not."""
    return [_case("fg84", precision=precision, B=B, options={"lds_kernel": 1}, want=LDS_WANT, pre="",
                  fin="qdec::ssf_block_kernel",
                  bp="qdec::bp_ms_lds_kernel<4>" if precision == "f32" else "qdec::bp_ms_lds64_kernel<4, 0>")
            for precision, B in itertools.product(("f32", "f64"), (5, 130))]


# The one list of what runs: group name -> (parameters, cases of one parameter).
# tests/test_gpu_forest.py has one test function per group.
GROUPS = {
    "wave": ([(key,) for key in ("fw128", "fw247", "fw498")], wave_cases),
    "block": ([(key,) for key in ("fb3u", "fb3g", "fb2")], block_cases),
    "block_hbm_state": ([("fb0",)], block_cases),
    "group": ([(key,) for key in GROUP_CELLS], group_cases),
    "lds": ([()], lds_cases),
}
# the kernel families the cases must reach: family -> what its entry name holds
FAMILIES = {
    "product-sum wave": r"bp_wave_kernel<\w+, 0, .*, false>",
    "min-sum wave, all outputs": r"bp_ms_wave_kernel<\w+, \d, \d, \d, false, false, ",
    "min-sum wave, lean": r"bp_ms_wave_kernel<\w+, \d, \d, \d, false, true, ",
    "compact": r"bp_ms_cmp_kernel<\w+, \d, \d, \d, false, \d, 0, 0>",
    "triage, byte rows": r"ms_triage_kernel<\d, \d, false>",
    "triage, packed rows": r"ms_triage_kernel<\d, \d, true>",
    "workgroup, unrolled": r"bp_block_kernel<\w+, \d, false, 16, 8>",
    "workgroup, generic": r"bp_block_kernel<\w+, \d, false, 0, 0>",
    "slot-group (8, 4)": r"bp_group_kernel<\w+, \d, 8, 4>",
    "slot-group (16, 8)": r"bp_group_kernel<\w+, \d, 16, 8>",
    "LDS-resident f32": r"bp_ms_lds_kernel<4>",
    "LDS-resident f64": r"bp_ms_lds64_kernel<4, 0>",
}
PLACEMENTS = (3, 2, 0)  # of the workgroup kernel: everything in LDS, messages in HBM, shot state in HBM too


def families_reached(cases):
    """The labels of FAMILIES whose mark an entry name of the cases holds, and
    ("placement", p) for the workgroup cases."""
    names = [n for c in cases for n in (c["bp"], c["pre"])]
    return ({f for f, mark in FAMILIES.items() if any(re.search(mark, n) for n in names)}
            | {("placement", c["path"][2]) for c in cases if c["path"]})


def group_params(name):
    import pytest
    return [pytest.param(p, id="-".join(map(str, p)) or "all") for p in GROUPS[name][0]]


def group_cases_of(name, param):
    return GROUPS[name][1](*param)


def all_cases():
    return [c for name, (params, _) in GROUPS.items() for p in params for c in group_cases_of(name, p)]


# ---------------------------------------------------------------- comparison
def llr_deviation(got, exact):
    """(largest |got - exact| / max(1, |exact|), largest |got - exact|) over the
    finite exact beliefs, after asserting that the signs agree where the exact
    belief is infinite."""
    got = np.asarray(got, np.float64)
    fin = np.isfinite(exact)
    assert np.array_equal(got[~fin] > 0, exact[~fin] > 0), "sign of a determined variable"
    d = np.abs(got[fin] - exact[fin])
    return (float((d / np.maximum(1.0, np.abs(exact[fin]))).max()) if d.size else 0.0,
            float(d.max()) if d.size else 0.0)


def compare(case, got, ref, tol):
    """got (a decoder's outputs for case["want"]) against the model's ref: x,
    iters and status equal, finite LLRs within tol, signs where the model says
    +-inf.  Returns the LLR deviation (or None)."""
    for k in case["want"]:
        if k != "llr":
            assert np.array_equal(got[k], ref[k]), (case["id"], k, int((got[k] != ref[k]).sum()))
    if "llr" not in case["want"]:
        return None
    dev = llr_deviation(got["llr"], ref["llr"])
    assert dev[0] <= tol, (case["id"], dev, tol)
    return dev


def oracle_decode(oracle_lib, case, **kw):
    H, probs, _ = sc.graph(case["graph"])
    syn = case_shots(case)[0]
    return oracle_lib.decode(H, probs, syn, method=case["method"], precision=case["precision"],
                             max_iter=case["max_iter"], ms_scaling=case["scaling"], want_llr=True, **kw)
