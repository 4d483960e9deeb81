"""Layered min-sum BP without a device: its numpy model against exact
min-marginals on forests and against the ldpc oracle on column-disjoint rows,
its gain over the flooding schedule, every refusal of the entry points and
qd_layered_info on host-only graphs, the Python argument checks, and the slot
rule's refusal paths under ASan + UBSan (tools/layered_scratch_check.cpp, a
stand-alone program: nothing sanitized is loaded into Python)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import layered_cases as lc
from layered_model import LayeredModel
from test_relay_host import SAN_FLAGS, host_graph

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The model's largest deviation from the exact min-marginals over the three
# forests below, |model - exact| / max(1, |exact|) on finite beliefs, measured
# on the CPU (test_model_reaches_the_exact_min_marginals_on_forests prints
# them).  The test allows twice the figure: the rule of forest_cases.ORACLE_DEV.
MODEL_DEV = {
    "f64": 4.31e-15,   # measured 4.31e-15 (fg84)
    "f32": 2.22e-6,    # measured 2.22e-06 (fg84)
}


# ---------------------------------------------------------------- 1. exact marginals on forests
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_model_reaches_the_exact_min_marginals_on_forests(precision):
    """Early stopping off, alpha = 1, 12 iterations: a check-serial sweep
    crosses every component of these forests well within that, and min-sum at
    alpha = 1 on a tree is the min-marginal.  Infinite beliefs (a lone degree-1
    check) are +-clip here and compared by sign."""
    import forest_cases as fc
    dtype = np.float32 if precision == "f32" else np.float64
    worst = 0.0
    for key in ("fb3g", "fw128", "fg84"):
        bd = fc.bundle(key)
        e = bd.e[:40]
        exact = bd.forest.decode(e, 1, radius=lambda t: 10 ** 6)["ms"]["llr_t"][:, 0]
        got = LayeredModel(bd.forest.H, bd.forest.probs, dtype, max_iter=12, ms_scaling=1.0).decode(
            bd.syn[:40], stop=False)
        assert (got["iters"] == 12).all() and not np.isnan(got["llr"]).any()
        assert np.isinf(exact).any() and np.isfinite(exact).any()
        dev = fc.llr_deviation(got["llr"], exact)
        print(f"{key} {precision}: relative {dev[0]:.3g}, absolute {dev[1]:.3g}")
        worst = max(worst, dev[0])
    print(f"{precision}: largest relative deviation {worst:.3g}")
    assert worst <= 2 * MODEL_DEV[precision]


# ---------------------------------------------------------------- 2. one iteration on disjoint rows
@pytest.mark.parametrize("ms_scaling", [1.0, 0.625, 0.0])
def test_model_is_the_oracles_flooding_iteration_on_disjoint_rows(oracle_lib, ms_scaling):
    """Rows that share no column and have at least two entries see the priors
    alone in iteration 1, under either schedule: x and the bytes of llr equal
    the ldpc loops' (oracle.ldpc_py in f64 on eight shots, the compiled oracle
    in both precisions on all 64)."""
    from oracle.ldpc_py import bp_decode
    g = lc.graph("disjoint")
    assert (np.diff(g["H"].indptr) >= 2).all() and (np.asarray(g["H"].sum(axis=0)) == 1).all()
    assert sorted(np.diff(g["H"].indptr)) == sorted(lc.DISJOINT_ROWS)
    syn, _, _ = lc.shots("disjoint", 64)
    for precision, dtype in (("f64", np.float64), ("f32", np.float32)):
        ref = lc.model("disjoint", dtype, 1, ms_scaling).decode(syn)
        assert 0 < (ref["status"] == 3).sum() < 64
        want = oracle_lib.decode(g["H"], g["probs"], syn, method="ms", precision=precision, max_iter=1,
                                 ms_scaling=ms_scaling, want_llr=True)
        assert np.array_equal(ref["x"], want["x"]), precision
        assert np.asarray(want["llr"], dtype).tobytes() == ref["llr"].tobytes(), precision
        assert np.array_equal(ref["status"] & 1, want["status"] & 1), precision
    ref = lc.model("disjoint", np.float64, 1, ms_scaling).decode(syn[:8])
    for b in range(8):
        x, llr, it, cv = bp_decode(g["H"], g["probs"], syn[b], method="ms", max_iter=1, ms_scaling=ms_scaling)
        assert np.array_equal(x, ref["x"][b]) and it == 1 and cv == (ref["status"][b] & 1), b
        assert llr.tobytes() == ref["llr"][b].tobytes(), b


# ---------------------------------------------------------------- 3. the gain over flooding
def test_layered_leaves_fewer_shots_open_than_flooding_in_fewer_iterations():
    """1000 code-capacity shots of the n = 225 code's Hz at p = 0.02 (numpy
    default_rng(2025)), f64, alpha = 1.  Open shots / mean iterations:
        10 iterations   flooding 327 / 6.25    layered 94 / 3.03
        50 iterations   flooding  94 / 12.74   layered 57 / 5.67
    Only the inequalities are asserted."""
    from relay_model import RelayModel
    hz = sp.csr_matrix(lc.rc.load_code("hgp_12_3_4_s1234").checks.z)
    p, B = 0.02, 1000
    e = (np.random.default_rng(2025).random((B, 225)) < p).astype(np.uint8)
    syn = (hz.dot(e.T.astype(np.int64)).T & 1).astype(np.uint8)
    for iters in (10, 50):
        fl = RelayModel(hz, p, np.float64, gamma0=0.0, pre_iter=iters, num_sets=0, alpha=1.0).decode(syn)
        ly = LayeredModel(hz, p, np.float64, max_iter=iters, ms_scaling=1.0).decode(syn)
        open_fl, open_ly = int((fl["status"] == 0).sum()), int((ly["status"] == 0).sum())
        print(f"{iters} iterations: flooding {open_fl} / {fl['iters'].mean():.2f}, layered {open_ly} / "
              f"{ly['iters'].mean():.2f}")
        done = ly["status"] == 3
        assert (hz.dot(ly["x"][done].T.astype(np.int64)).T & 1 == syn[done]).all()
        assert open_ly < open_fl
        assert ly["iters"].mean() < fl["iters"].mean()


# ---------------------------------------------------------------- 4. the no-HIP entry points
@pytest.fixture(scope="module")
def lib():
    from exp_ldpc_amd import _abi
    return _abi.load()


def layered_params(max_iter=8, ms_scaling=0.625, clip=2.0 ** 64):
    from exp_ldpc_amd import _abi
    return _abi.QdLayeredParams(max_iter, ms_scaling, clip)


def test_every_refusal_on_a_host_only_graph(lib):
    from exp_ldpc_amd import _abi
    g = lc.graph("hz225")
    n, m = 225, 108
    syn = np.zeros(m, np.uint8)
    ok = layered_params()

    def call(h, prm=ok, prec=1, B=1, s=syn, flags=0, place=2, rd=None, fail=None, host=False):
        p = None if prm is None else C.byref(prm)
        if host:
            return lib.qd_layered_batch(h, p, prec, B, _abi.ptr(s), flags, None, _abi.ptr(rd), None, None, None, None,
                                        None, _abi.ptr(fail), place)
        return lib.qd_layered_batch_device(h, p, prec, B, _abi.ptr(s), flags, None, _abi.ptr(rd), None, None, None,
                                           None, None, _abi.ptr(fail), place, None)

    assert call(None) == -1 and call(None, host=True) == -1
    h = host_graph(lib, g["H"])
    try:
        assert call(h) == -5  # priors never set
        p01 = np.full(n, 0.01)
        p01[3] = 0.0
        assert lib.qd_graph_set_priors(h, _abi.ptr(p01)) == 0
        assert call(h) == -51
        assert lib.qd_graph_set_priors(h, _abi.ptr(np.ascontiguousarray(g["probs"]))) == 0
        for host in (False, True):
            assert call(h, prec=2, host=host) == -4
            assert call(h, B=-1, host=host) == -8
            assert call(h, place=3, host=host) == -68 and call(h, place=-1, host=host) == -68
            assert call(h, prm=None, host=host) == -49
            for bad in (dict(max_iter=0), dict(max_iter=-3), dict(clip=0.0), dict(clip=-1.0), dict(clip=np.inf),
                        dict(clip=np.nan), dict(ms_scaling=-0.5), dict(ms_scaling=np.inf), dict(ms_scaling=np.nan)):
                assert call(h, prm=layered_params(**bad), host=host) == -49, bad
            assert call(h, flags=16, host=host) == -69 and call(h, flags=4, host=host) == -69
            assert call(h, s=None, host=host) == -7
            assert call(h, s=None, flags=3, host=host) == -7  # neither base nor readout
            assert call(h, B=0, host=host) == 0
            assert call(h, B=0, s=None, host=host) == 0
            assert call(h, host=host) == -16  # everything checked, no device
            assert b"host-only" in lib.qd_last_error()
        assert lib.qd_layered_set_slots(h, -1) == -49 and lib.qd_layered_set_slots(h, (1 << 20) + 1) == -49
        assert lib.qd_layered_set_slots(h, 2) == 0 and lib.qd_layered_set_slots(h, 0) == 0
        assert lib.qd_layered_set_slots(None, 0) == -1
        # more than 256 logicals in the fused check
        lz = np.zeros((257, n), np.uint8)
        lz[np.arange(257), np.arange(257) % n] = 1
        assert lib.qd_graph_set_logicals(h, 257, _abi.ptr(lz)) == 0
        one = np.zeros(1, np.uint8)
        assert call(h, rd=np.zeros(n, np.uint8), fail=one) == -69
        assert call(h, rd=np.zeros(n, np.uint8)) == -16  # no fail output: no fused check
    finally:
        lib.qd_graph_destroy(h)


def test_layered_info_and_kernel_names(lib):
    from exp_ldpc_amd import _abi
    from exp_ldpc_amd.decoder import layered_info, layered_kernel_names
    h = host_graph(lib, lc.graph("hz225")["H"], 0.02)
    try:
        # 108 x 225, E = 756: control 64 + syndrome 128 + bits 32 + bytes 256 = 480 B; beliefs (E + n) T
        assert layered_info(h, _abi.QD_F32, "lds") == (0, 480 + 3936, 0, 0)
        assert layered_info(h, _abi.QD_F32, "auto") == (0, 4416, 0, 0)
        assert layered_info(h, _abi.QD_F32, "hbm") == (1, 480, 4096, 0)
        assert layered_info(h, _abi.QD_F64, "lds") == (0, 480 + 7856, 0, 0)
        assert layered_info(h, _abi.QD_F64, "auto") == (0, 8336, 0, 0)
        assert layered_info(h, _abi.QD_F64, "hbm") == (1, 480, (981 * 8 + 255) // 256 * 256, 0)
        out = np.zeros(4, np.int64)
        assert lib.qd_layered_info(h, 1, 3, _abi.ptr(out)) == -68
        assert lib.qd_layered_info(h, 5, 0, _abi.ptr(out)) == -4
        assert lib.qd_layered_info(h, 0, 0, None) == -49
        assert lib.qd_layered_info(None, 0, 0, _abi.ptr(out)) == -1
    finally:
        lib.qd_graph_destroy(h)
    # the R = 2 spacetime graph fits LDS once but not eight times: auto goes to HBM
    h = host_graph(lib, lc.graph("st225r2")["H"], 0.02)
    try:
        lds = layered_info(h, _abi.QD_F64, "lds")
        assert lds[0] == 0 and 160 * 1024 // 8 < lds[1] <= 160 * 1024
        assert layered_info(h, _abi.QD_F64, "auto")[0] == 1
        assert layered_info(h, _abi.QD_F32, "auto")[0] == 0  # half the bytes: eight fit
    finally:
        lib.qd_graph_destroy(h)
    # beliefs beyond LDS: LDS is refused, auto goes to HBM
    n, m = 6000, 3000
    rows = np.repeat(np.arange(m), 6)
    cols = (np.arange(6 * m) * 7) % n
    H = sp.csr_matrix((np.ones(6 * m, np.uint8), (rows, cols)), shape=(m, n))
    H.sum_duplicates()
    H.data[:] = 1
    h = host_graph(lib, H, 0.01)
    try:
        out = np.zeros(4, np.int64)
        assert lib.qd_layered_info(h, 0, 0, _abi.ptr(out)) == -111
        assert layered_info(h, _abi.QD_F64, "auto")[0] == 1
    finally:
        lib.qd_graph_destroy(h)
    # the syndrome and the hard decision alone exceed LDS: no placement holds the graph
    n, m = 170000, 2
    H = sp.csr_matrix((np.ones(4, np.uint8), ([0, 0, 1, 1], [0, 1, 2, n - 1])), shape=(m, n))
    h = host_graph(lib, H, 0.01)
    try:
        out = np.zeros(4, np.int64)
        for place in (0, 1, 2):
            assert lib.qd_layered_info(h, 1, place, _abi.ptr(out)) == -111, place
        syn = np.zeros(m, np.uint8)
        prm = layered_params()
        assert lib.qd_layered_batch_device(h, C.byref(prm), 1, 1, _abi.ptr(syn), 0, None, None, None, None, None, None,
                                           None, None, 2, None) == -111
    finally:
        lib.qd_graph_destroy(h)
    names = layered_kernel_names()
    assert names == [f"qdec::layered_wave_kernel<{t}, {p}>" for t in ("double", "float") for p in ("false", "true")]
    big = C.create_string_buffer(1 << 16)
    lib.qd_kernel_table_names(big, 1 << 16)
    assert "layered" not in big.value.decode()  # the decode families' list is pinned and unchanged


# ---------------------------------------------------------------- 5. the Python argument checks
def test_python_argument_checks():
    from exp_ldpc_amd.decoder import Decoder, layered_placement_code, parse_schedule
    assert parse_schedule("flooding") == "flooding" and parse_schedule("parallel") == "flooding"
    assert parse_schedule("Layered") == "layered"
    for bad in ("serial", "", "layered ms"):
        with pytest.raises(ValueError):
            parse_schedule(bad)
    assert [layered_placement_code(p) for p in ("lds", "hbm", "auto")] == [0, 1, 2]
    with pytest.raises(ValueError):
        layered_placement_code("onchip")
    # refused before a handle is made, so no device is needed
    H = lc.rc.H35
    with pytest.raises(ValueError, match="schedule"):
        Decoder(H, 0.1, schedule="serial")
    with pytest.raises(ValueError, match="min-sum"):
        Decoder(H, 0.1, method="ps", schedule="layered")
    with pytest.raises(ValueError, match="SSF"):
        Decoder(H, 0.1, method="ms", schedule="layered", ssf=True)
    with pytest.raises(ValueError, match="SSF"):
        Decoder(H, 0.1, method="ms", schedule="layered", flip_sets=np.ones((1, 5), np.uint8))
    with pytest.raises(ValueError, match="layered_placement"):
        Decoder(H, 0.1, method="ms", schedule="layered", layered_placement="onchip")
    from exp_ldpc_amd.ldpc_compat import bp_decoder, bposd_decoder
    for cls in (bp_decoder, bposd_decoder):
        with pytest.raises(ValueError, match="schedule"):
            cls(H, error_rate=0.1, bp_method="ms", schedule="serial")
        with pytest.raises(ValueError, match="min-sum"):
            cls(H, error_rate=0.1, bp_method="ps", schedule="layered")


# ---------------------------------------------------------------- 6. the slot rule under sanitizers
FREE = "free (hipFree layered scratch)"
HALVING = ["alloc 8000 oom", "alloc 4000 oom", "alloc 2000 oom", "alloc 1000 oom"]
NO_SLOT = "-> - 0 1000 -112 no memory for one layered-BP slot of 1000 B"
EXPECTED = {
    # the budget is asked first (1 MiB free: 262 slots), then 8 -> 4 -> 2 -> 1 slots refused; every call tries again
    "everything_refused": ["free_bytes", "drain", *HALVING, NO_SLOT,
                           "free_bytes", "drain", *HALVING, NO_SLOT,
                           "drain"],
    # a quarter of 3999 B holds no slot; a quarter of 12000 B holds 3; fewer configured slots: no question
    "budget": ["free_bytes", "-> - 0 0 -113 one layered-BP slot of 1000 B is beyond the scratch budget "
                             "(a quarter of the free device memory)",
               "free_bytes", "drain", "alloc 3000 ok", "-> 3 3000 0 0",
               "-> 2 3000 0 0",
               "drain", FREE],
    # five shots, requests above 2500 B refused: 5 -> 3 -> 2 slots, the mark at 3000; not asked again
    "halved": ["free_bytes", "drain", "alloc 5000 oom", "alloc 3000 oom", "alloc 2000 ok", "-> 2 2000 3000 0",
               "-> 2 2000 3000 0",
               "drain", FREE],
    "other_error": ["free_bytes", "drain", "alloc 8000 error 7", "-> - 0 0 -107 hipMalloc layered scratch: fake error",
                    "drain"],
    # bytes of LDS with the beliefs in LDS / in HBM, bytes per slot, and the kind that
    # placements LDS / HBM / AUTO launch (-1: none); worked out by hand from LayeredLayout:
    # hz225 108 x 225, E 756: 64 + 128 + 32 + 256 = 480; (756 + 225) T = 3924 / 7848 -> 3936 / 7856 in 16-B units
    # st225r2 324 x 891, E 3159: 64 + 384 + 112 + 896 = 1456; 4050 x 8 = 32400; 33856 x 8 > 160 KiB
    # dem 648 x 25684, E 120000: 64 + 704 + 3216 + 25728 = 29712; 145684 x 8 = 1165472 -> 4553 x 256
    "layouts": ["layout hz225_f32 4416 480 4096 0 1 0",
                "layout hz225_f64 8336 480 7936 0 1 0",
                "layout st225r2_f64 33856 1456 32512 0 1 1",
                "layout dem_f64 1195184 29712 1165568 -1 1 1",
                "layout huge_f32 22250096 1450096 20800000 -1 -1 -1"],
}


def test_layered_slot_rule_is_clean_under_sanitizers_and_follows_the_policy(tmp_path):
    from exp_ldpc_amd import build
    cxx = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(build._hipcc()))), "lib", "llvm", "bin", "clang++")
    assert os.path.exists(cxx), f"ROCm's clang++ not found at {cxx}"
    exe = str(tmp_path / "layered_scratch_check")
    res = subprocess.run([cxx, *SAN_FLAGS, os.path.join(REPO, "tools", "layered_scratch_check.cpp"), "-o", exe],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0 and res.stderr == "", f"exit {res.returncode}\n{res.stderr[-4000:]}"
    got = {}
    for line in res.stdout.splitlines():
        if line.startswith("# "):
            got[line[2:]] = cur = []
        else:
            cur.append(line)
    assert list(got) == list(EXPECTED)
    for name, trace in EXPECTED.items():
        assert got[name] == trace, name
