"""CPU side of tests/forest_cases.py: the oracle (oracle/bp_impl.inc) and its
Python twin (oracle/ldpc_py.py) against the exact model of tests/forest_model.py,
the plan of every case by entry name, the conditions that keep a case from
passing vacuously, the guard on the inputs, and two mutations of the model that
the comparison must notice.  No GPU."""
import numpy as np
import pytest

import forest_cases as fc
import forest_model as fm
import ssf_cases as sc
from forest_model import Template as T

KEYS = sorted(fc.SPECS)


def _pool_case(key, method, precision):
    """A case over the whole pool of a graph: every case's shots are a window of it."""
    return fc._case(key, method=method, precision=precision, B=fc.SPECS[key][4])


@pytest.fixture(scope="module")
def deviations(oracle_lib):
    """{(key, method, precision): (relative, absolute) LLR deviation} of the
    oracle from the model on the pool of every graph, after x, iters and status
    were found equal and the signs of the determined variables too."""
    out = {}
    for key in KEYS:
        for method in fm.METHODS:
            for precision in ("f32", "f64"):
                c = _pool_case(key, method, precision)
                ref = fc.case_shots(c)[1]
                got = fc.oracle_decode(oracle_lib, c)
                out[key, method, precision] = fc.compare(c, got, ref, np.inf)
    return out


def test_oracle_equals_the_model(deviations):
    """Every graph's pool (each case decodes a window of it), both methods and
    precisions: the oracle's x, iters and status equal the model's, its LLRs
    have the model's sign where the model says +-inf, and elsewhere deviate by
    at most twice the figures of forest_cases.ORACLE_DEV, which are the largest
    deviations measured here."""
    worst, abs32 = {}, 0.0
    for (key, method, precision), (rel, ab) in deviations.items():
        worst[method, precision] = max(worst.get((method, precision), 0.0), rel)
        if precision == "f32":
            abs32 = max(abs32, ab)
    print("measured:", {k: f"{v:.3g}" for k, v in worst.items()}, f"abs f32 {abs32:.3g}")
    for mp, v in worst.items():
        assert v <= fc.host_tol(*mp), (mp, v)
        assert v >= fc.ORACLE_DEV[mp] / 2, ("forest_cases.ORACLE_DEV is not the measured figure", mp, v)
    assert fc.ORACLE_ABS_F32 / 2 <= abs32 <= 2 * fc.ORACLE_ABS_F32
    assert fc.GUARD == 64 * fc.ORACLE_ABS_F32


def _toy(seed):
    """A forest of 30-odd columns with every kind of template, 6 settled shots."""
    parts = [(fc.ISO, 2), (fc.ONE, 1), (fc.PAIR, 2), (fc.PIN, 1), (fc.CHAIN, 1), (fc.TWIG, 1),
             (T("path7", [(i, 1) for i in range(6)], prior=fc.FLAT), 1), (fc.star(4), 1)]
    f = fm.Forest(parts, seed, *fc.PRIORS)
    e, rate = fm.sample_errors(f, (0.03, 0.1, 0.3), 6, seed + 1)
    fm.settle(f, e, rate, fc.MAX_ITER, fc.GUARD, fc.CAP, seed + 2)
    return f, e


def _assert_equal(case_id, got, ref, tol):
    fc.compare(dict(id=case_id, want=fc.FULL_WANT), got, ref, tol)


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("method", fm.METHODS)
def test_python_restatement_equals_the_model(seed, method):
    """oracle/ldpc_py.py, the oracle's only other cross-check, on a dozen small
    forests against the model."""
    from oracle.ldpc_py import bp_decode
    f, e = _toy(seed)
    ref = f.decode(e, fc.MAX_ITER)[method]
    syn = f.syndrome(e)
    rows = [bp_decode(f.H, f.probs, s, method=method, max_iter=fc.MAX_ITER, ms_scaling=1.0) for s in syn]
    got = dict(x=np.array([r[0] for r in rows]), llr=np.array([r[1] for r in rows]),
               iters=np.array([r[2] for r in rows], np.int32), status=np.array([3 * r[3] for r in rows], np.uint8))
    _assert_equal(f"toy{seed}-{method}", got, ref, fc.host_tol(method, "f64"))


@pytest.mark.parametrize("mutation", [dict(radius=lambda t: 2 * t + 1), dict(use_syndrome=False)],
                         ids=["radius", "syndrome"])
def test_a_wrong_model_is_noticed(oracle_lib, mutation):
    """With the radius 2 t - 1 replaced by 2 t + 1, and with the syndrome
    ignored, the comparison that passes on the model fails."""
    f, e = _toy(3)
    syn = f.syndrome(e)
    for method in fm.METHODS:
        got = oracle_lib.decode(f.H, f.probs, syn, method=method, precision="f64", max_iter=fc.MAX_ITER,
                                ms_scaling=1.0)
        _assert_equal("toy", got, f.decode(e, fc.MAX_ITER)[method], fc.host_tol(method, "f64"))
        with pytest.raises(AssertionError):
            _assert_equal("toy", got, f.decode(e, fc.MAX_ITER, **mutation)[method], fc.host_tol(method, "f64"))


# ---------------------------------------------------------------- plans
@pytest.fixture(scope="module")
def planned():
    """{case id: (plan, entry names)} of every case, on host-only graphs."""
    from exp_ldpc_amd import _abi
    from test_bp_ledger_host import plan_entries
    from test_ssf_mixed_host import HostGraphs
    lib = _abi.load()
    graphs = HostGraphs(lib)
    try:
        return {c["id"]: plan_entries(lib, graphs.get(c), c) for c in fc.all_cases()}
    finally:
        graphs.close()


def test_every_case_plans_what_it_names(planned):
    cases = fc.all_cases()
    assert len({c["id"] for c in cases}) == len(cases)
    for c in cases:
        plan, names = planned[c["id"]]
        assert names == (c["bp"], c["fin"], c["pre"]), (c["id"], plan, names)
        if c["path"]:
            assert (plan["bp"], plan["fin"], plan["placement"]) == c["path"], (c["id"], plan)
        assert c["method"] == "ps" or c["scaling"] == 1.0
        assert set(c["want"]) >= {"iters", "status"}


def test_every_family_is_reached():
    """Every family of forest_cases.FAMILIES and every placement of the
    workgroup kernel is named by a case (which test_every_case_plans_what_it_names
    holds to its plan), in both precisions, and the count notices a missing
    group: without the cases of any one group something is unreached."""
    everything = set(fc.FAMILIES) | {("placement", p) for p in fc.PLACEMENTS}
    assert fc.families_reached(fc.all_cases()) == everything
    for precision, other in (("f32", "LDS-resident f64"), ("f64", "LDS-resident f32")):
        assert fc.families_reached([c for c in fc.all_cases() if c["precision"] == precision]) == everything - {other}
    for group in fc.GROUPS:
        rest = [c for g, (params, _) in fc.GROUPS.items() if g != group for p in params
                for c in fc.group_cases_of(g, p)]
        assert fc.families_reached(rest) != everything, group
    wave = [c for c in fc.all_cases() if c["graph"].startswith("fw")]
    assert {c["B"] for c in wave} == set(fc.WAVE_B)
    assert {sc.wave_shape_of(c["graph"][1:]) for c in wave} == {(1, 2, 8), (2, 4, 7), (4, 9, 8)}
    assert {c["B"] for c in fc.all_cases() if c["graph"] == "fb3g"} == {5, 130, 2600}
    assert {c["B"] for c in fc.all_cases() if c["graph"] == "fb0"} == {5}


def test_gpu_module_runs_every_group():
    import test_gpu_forest as gpu
    assert sorted(gpu.GROUP_OF_TEST.values()) == sorted(fc.GROUPS)
    for fn_name, group in gpu.GROUP_OF_TEST.items():
        marks = [m for m in getattr(gpu, fn_name).pytestmark if m.name == "parametrize"]
        assert len(marks) == 1 and [p.values[0] for p in marks[0].args[1]] == fc.GROUPS[group][0], fn_name
    assert gpu.pytestmark.name == "gpu"


# ---------------------------------------------------------------- inputs
@pytest.mark.parametrize("key", KEYS)
def test_forests_hold_what_the_kernels_trip_on(key):
    """Each graph is a forest whose components are scattered over rows and
    columns, with isolated columns, checks of degree 1 and 2, a component too
    deep for MAX_ITER iterations to cross, priors above 0.5, and the largest
    row and column degree its kernel allows."""
    f = fc.bundle(key).forest
    m, n, parts = fc.SPECS[key][:3]
    H = f.H
    assert H.shape == (m, n) and H.nnz == sum(t.A.sum() * K for t, K in f.parts)
    # a forest: edges = vertices - components (no cycle), components as built
    import scipy.sparse as sp
    import scipy.sparse.csgraph as cg
    adj = sp.bmat([[None, H], [H.T, None]]).tocsr()
    ncomp, label = cg.connected_components(adj, directed=False)
    assert ncomp == sum(K for _, K in f.parts) and H.nnz == m + n - ncomp
    for (t, K), vo, co in zip(f.parts, f.var_of, f.chk_of):
        # components of at most 12 variables in the large graphs, but for the three copies of the
        # row of 16 (k = 17) that make fb2 a graph of the unrolled body's full width; 18 for the row of 17
        assert t.k <= {"fb3g": 18, "fb3u": 17, "fb0": 10}.get(key, 12) or (key == "fb2" and t.k == 17 and K == 3)
        if t.k > 1:
            assert np.abs(np.diff(np.sort(vo, axis=1), axis=1)).max() > 1, "a component on contiguous columns"
        if t.c > 1 and t.k > 4:
            assert np.abs(np.diff(np.sort(co, axis=1), axis=1)).max() > 1, "a component on contiguous rows"
    rdeg, cdeg = np.diff(H.indptr), np.diff(H.tocsc().indptr)
    assert (cdeg == 0).sum() >= 2 and (rdeg == 1).any() and (rdeg == 2).any()
    assert max(t.radius for t, _ in f.parts) > fc.MAX_ITER >= 6
    want_r, want_c = {"fw128": (8, 4), "fw247": (7, 4), "fw498": (8, 4), "fb3u": (16, 8), "fb3g": (17, 9),
                      "fb2": (16, 8), "fb0": (8, 8), "fg84": (8, 4)}[key]
    assert (rdeg.max(), cdeg.max()) == (want_r, want_c)
    p = f.probs
    assert 0.005 * n <= (p > 0.5).sum() and p.max() < 0.7 and np.abs(p - 0.5).min() > 0.01
    assert len(np.unique(p)) == n


@pytest.mark.parametrize("key", KEYS)
def test_guard(key):
    """No belief of any shot of the pool, at any iteration up to MAX_ITER and
    under either method, is smaller than forest_cases.GUARD, and no finite one
    larger than CAP: met by construction (forest_model.settle), no skip path.
    Every syndrome is that of an error."""
    bd = fc.bundle(key)
    assert np.array_equal(bd.syn, bd.forest.syndrome(bd.e))
    for method in fm.METHODS:
        a = np.abs(bd.model[method]["llr_t"])
        assert not np.isnan(a).any()
        assert a.min() >= fc.GUARD, (key, method, a.min())
        assert a[np.isfinite(a)].max() <= fc.CAP, (key, method)
        assert (~np.isfinite(a)).any()  # determined variables: sign only


def test_cases_are_not_vacuous():
    """forest_cases.conditions on the model's outputs of every case's shots."""
    seen = set()
    for c in fc.all_cases():
        key = (c["graph"], c["method"], c["B"])
        if key in seen:
            continue
        seen.add(key)
        syn, ref = fc.case_shots(c)
        assert syn.shape[0] == c["B"]
        assert fc.conditions(ref, syn.any(axis=1)) is None, (c["id"], fc.conditions(ref, syn.any(axis=1)))
