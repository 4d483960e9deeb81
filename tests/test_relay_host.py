"""The relay stage without a device: its numpy model against the ldpc oracle,
qd_graph_set_relay and the other no-HIP entry points on host-only graphs, the
model's gain over plain min-sum, and the slot rule's refusal paths under ASan +
UBSan (tools/relay_scratch_check.cpp, a stand-alone program: nothing sanitized
is loaded into Python)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import relay_cases as rc
from relay_model import RelayModel

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- 1. gamma = 0 is plain min-sum
@pytest.mark.parametrize("gname,shots,max_iter", [("hz225", 5, 12), ("h35", 8, 6)])
@pytest.mark.parametrize("alpha", [1.0, 0.625])
def test_model_without_memory_is_the_oracles_min_sum(gname, shots, max_iter, alpha):
    from oracle.ldpc_py import bp_decode
    g = rc.graph(gname)
    H, probs = g["H"], g["probs"]
    # clip = inf: a degree-1 row sends Big, beyond any finite clip; the spec's
    # "clip not reached"
    mdl = RelayModel(H, probs, np.float64, gamma0=0.0, pre_iter=max_iter, num_sets=0, alpha=alpha, clip=np.inf)
    syn, _, _ = rc.shots(gname, shots, seed=11)
    if gname == "h35":
        syn = np.array([[(b >> i) & 1 for i in range(3)] for b in range(8)], np.uint8)  # every syndrome
    ref = mdl.decode(syn)
    conv = 0
    for b in range(syn.shape[0]):
        x, llr, it, cv = bp_decode(H, probs, syn[b], method="ms", max_iter=max_iter, ms_scaling=alpha)
        assert np.array_equal(x, ref["x"][b]), b
        assert it == ref["iters"][b] and cv == (ref["status"][b] & 1) and ref["legs"][b] == 1, b
        assert llr.tobytes() == ref["llr"][b].tobytes(), b
        conv += cv
    assert 0 < conv  # both outcomes of the syndrome test are exercised on hz225
    if gname == "hz225":
        assert conv < syn.shape[0]


# ---------------------------------------------------------------- 2. the no-HIP entry points
@pytest.fixture(scope="module")
def lib():
    from exp_ldpc_amd import _abi
    return _abi.load()


def host_graph(lib, H, probs=None):
    from exp_ldpc_amd import _abi
    H = sp.csr_matrix(H)
    H.sort_indices()
    h = C.c_void_p()
    rp, ci = H.indptr.astype(np.int32), H.indices.astype(np.int32)
    assert lib.qd_graph_create_host(H.shape[0], H.shape[1], _abi.ptr(rp), _abi.ptr(ci), H.shape[1], 1, C.byref(h)) == 0
    if probs is not None:
        p = np.ascontiguousarray(np.broadcast_to(np.asarray(probs, np.float64), (H.shape[1],)))
        assert lib.qd_graph_set_priors(h, _abi.ptr(p)) == 0
    return h


def relay_params(**kw):
    from exp_ldpc_amd import _abi
    v = dict(gamma0=0.125, alpha=1.0, clip=2.0 ** 64, pre_iter=8, num_sets=2, set_max_iter=4, stop_nconv=1)
    v.update(kw)
    return _abi.QdRelayParams(v["gamma0"], v["alpha"], v["clip"], v["pre_iter"], v["num_sets"], v["set_max_iter"],
                              v["stop_nconv"])


def digest(lib, h):
    d, b = C.c_uint64(0), C.c_int64(0)
    assert lib.qd_graph_table_digest(h, C.byref(d), C.byref(b)) == 0
    return d.value, b.value


def test_set_relay_refusals_and_acceptance_on_a_host_only_graph(lib):
    from exp_ldpc_amd import _abi
    g = rc.graph("hz225")
    n = 225
    gam = np.ascontiguousarray(np.linspace(-0.5, 1.5, 2 * n).reshape(2, n))
    ok = relay_params()
    assert lib.qd_graph_set_relay(None, C.byref(ok), _abi.ptr(gam)) == -1
    h = host_graph(lib, g["H"])
    try:
        assert lib.qd_graph_set_relay(h, C.byref(ok), _abi.ptr(gam)) == -5  # priors never set
        assert lib.qd_relay_batch_device(h, 1, 1, None, 0, None, None, None, None, None, None, None, None, None, 0, 2,
                                         None) == -54
        p01 = np.full(n, 0.01)
        p01[3] = 0.0
        assert lib.qd_graph_set_priors(h, _abi.ptr(p01)) == 0
        assert lib.qd_graph_set_relay(h, C.byref(ok), _abi.ptr(gam)) == -51
        assert lib.qd_graph_set_priors(h, _abi.ptr(np.ascontiguousarray(g["probs"]))) == 0
        before = digest(lib, h)
        assert lib.qd_graph_set_relay(h, None, _abi.ptr(gam)) == -52
        for bad in (dict(alpha=0.0), dict(alpha=-1.0), dict(alpha=np.inf), dict(alpha=np.nan), dict(clip=0.0),
                    dict(clip=-2.0), dict(clip=np.nan), dict(gamma0=np.nan), dict(gamma0=np.inf), dict(pre_iter=0),
                    dict(set_max_iter=0), dict(stop_nconv=0), dict(num_sets=-1)):
            assert lib.qd_graph_set_relay(h, C.byref(relay_params(**bad)), _abi.ptr(gam)) == -52, bad
        assert lib.qd_graph_set_relay(h, C.byref(ok), None) == -52  # no table with num_sets > 0
        nan_tab = gam.copy()
        nan_tab[1, 7] = np.nan
        assert lib.qd_graph_set_relay(h, C.byref(ok), _abi.ptr(nan_tab)) == -52
        # the cap: (num_sets + 1) n <= 2^23 entries; checked before the table is read
        over = (1 << 23) // n
        assert lib.qd_graph_set_relay(h, C.byref(relay_params(num_sets=over)), _abi.ptr(gam)) == -53
        assert b"2^23" in lib.qd_last_error()
        # accepted: with a table, without one, with clip = inf (no clamp)
        assert lib.qd_graph_set_relay(h, C.byref(ok), _abi.ptr(gam)) == 0
        assert lib.qd_graph_set_relay(h, C.byref(relay_params(num_sets=0)), None) == 0
        assert lib.qd_graph_set_relay(h, C.byref(relay_params(clip=np.inf)), _abi.ptr(gam)) == 0
        assert digest(lib, h) == before  # the relay tables are no part of the pinned digests
        # rebuilt by set_priors: still set afterwards; priors with a 1 leave it refusing with -51
        assert lib.qd_graph_set_priors(h, _abi.ptr(np.full(n, 0.03))) == 0
        assert lib.qd_relay_batch_device(h, 1, 1, np.zeros(108, np.uint8).ctypes.data_as(C.c_void_p), 0, None, None,
                                         None, None, None, None, None, None, None, 0, 2, None) == -16
        p01[3] = 1.0
        assert lib.qd_graph_set_priors(h, _abi.ptr(p01)) == 0
        assert lib.qd_relay_batch_device(h, 1, 1, np.zeros(108, np.uint8).ctypes.data_as(C.c_void_p), 0, None, None,
                                         None, None, None, None, None, None, None, 0, 2, None) == -51
        assert lib.qd_graph_set_priors(h, _abi.ptr(np.full(n, 0.03))) == 0
        syn = np.zeros(108, np.uint8).ctypes.data_as(C.c_void_p)
        call = lambda prec=1, B=1, s=syn, flags=0, place=2: lib.qd_relay_batch_device(
            h, prec, B, s, flags, None, None, None, None, None, None, None, None, None, 0, place, None)
        assert call(prec=2) == -4
        assert call(B=-1) == -8
        assert call(place=3) == -55
        assert call(flags=16) == -57 and call(flags=4) == -57
        assert call(s=None) == -7
        assert call(B=0) == 0
        assert call() == -16  # everything checked, no device
        assert lib.qd_relay_set_slots(h, -1) == -52 and lib.qd_relay_set_slots(h, (1 << 20) + 1) == -52
        assert lib.qd_relay_set_slots(h, 2) == 0 and lib.qd_relay_set_slots(h, 0) == 0
    finally:
        lib.qd_graph_destroy(h)


def test_relay_info_and_kernel_names(lib):
    from exp_ldpc_amd import _abi
    from exp_ldpc_amd.decoder import relay_info
    h = host_graph(lib, rc.graph("hz225")["H"], 0.02)
    try:
        # 108 x 225, E = 756: LDS part 64 + 256 + 128 + 32 = 480 B; messages (2 E + n) T in 16-B regions
        assert relay_info(h, _abi.QD_F32, "lds") == (0, 480 + 2 * 3024 + 912, 0, 0)
        assert relay_info(h, _abi.QD_F32, "auto") == (0, 7440, 0, 0)
        assert relay_info(h, _abi.QD_F32, "hbm") == (1, 480, 7168, 0)
        assert relay_info(h, _abi.QD_F64, "hbm") == (1, 480, (2 * 6048 + 1808 + 255) // 256 * 256, 0)
        out = np.zeros(4, np.int64)
        assert lib.qd_relay_info(h, 1, 3, _abi.ptr(out)) == -55
        assert lib.qd_relay_info(h, 5, 0, _abi.ptr(out)) == -4
    finally:
        lib.qd_graph_destroy(h)
    # a graph whose messages do not fit LDS: auto goes to HBM, LDS is refused
    n, m = 6000, 3000
    rows = np.repeat(np.arange(m), 6)
    cols = (np.arange(6 * m) * 7) % n
    H = sp.csr_matrix((np.ones(6 * m, np.uint8), (rows, cols)), shape=(m, n))
    H.sum_duplicates()
    H.data[:] = 1
    h = host_graph(lib, H, 0.01)
    try:
        out = np.zeros(4, np.int64)
        assert lib.qd_relay_info(h, 0, 0, _abi.ptr(out)) == -56
        assert relay_info(h, _abi.QD_F64, "auto")[0] == 1
    finally:
        lib.qd_graph_destroy(h)
    buf = C.create_string_buffer(4096)
    k = lib.qd_relay_kernel_names(buf, 4096)
    names = buf.value.decode().split("\n")
    assert k == len(buf.value) and names[:2] == ["qdec::relay_block_kernel<double>", "qdec::relay_block_kernel<float>"]
    big = C.create_string_buffer(1 << 16)
    lib.qd_kernel_table_names(big, 1 << 16)
    assert "relay" not in big.value.decode()  # the decode families' list is pinned and unchanged


def test_the_weight_17_row_plans_the_generic_block_kernel_and_its_shots_take_both_exits(lib):
    """"h35w17" (tests/relay_cases.py): the launch plan puts plain min-sum BP in
    the workgroup family (bp 5: bp_block_kernel) in both precisions.  That family
    reports no kernel name (qd_graph_plan_names stays "" for it, as
    qd_graph_last_kernels does), so the instantiation is pinned by the planner's
    rule instead: a row above 16 entries rules out <T, 1, *, 16, 8> and leaves
    <T, 1, *, 0, 0>.  And on the CPU: of the WIDE_ROW shots the model solves some
    and leaves some open, so test_gpu_relay.py runs both exits of the loop."""
    from exp_ldpc_amd import _abi
    from host_helpers import _plan_names
    g = rc.graph("h35w17")
    assert np.diff(g["H"].indptr).max() == 17 and g["H"].shape == (4, 21)
    h = host_graph(lib, g["H"], g["probs"])
    try:
        for prec in (_abi.QD_F64, _abi.QD_F32):
            prm = _abi.QdParams(rc.WIDE_ROW["max_iter"], 1, prec, 0, 0, 0, rc.WIDE_ROW["alpha"])
            for present in (1 | 4 | 64 | 128, 2 | 4 | 8 | 32 | 64):  # syn, readout, fail / base, readout, x, llr, fail
                out = np.zeros(8, np.int32)
                assert lib.qd_graph_plan(h, C.byref(prm), rc.WIDE_ROW["B"], present, _abi.ptr(out)) == 0
                assert out[0] == 5 and out[1] == 0  # kBpBlock, no SSF stage
                assert _plan_names(lib, h, prm, rc.WIDE_ROW["B"], present) == ["", "", ""]
    finally:
        lib.qd_graph_destroy(h)
    for dtype in (np.float32, np.float64):
        for flags in (0, 3):
            syn, base, rd = rc.wide_row_shots(flags)
            conv = rc.wide_row_model(dtype).decode(syn, base, rd, flags)["status"] & 1
            assert 0 < conv.sum() < rc.WIDE_ROW["B"], (dtype, flags)


# ---------------------------------------------------------------- 3. the gain over plain min-sum
def test_relay_leaves_fewer_unsatisfied_shots_than_long_min_sum():
    """1000 code-capacity shots of the n = 225 code at p = 0.02 (numpy PCG64
    seed 2025), f64: min-sum, alpha 1, 1040 iterations leaves 20 unsatisfied;
    relay (gamma0 0.125, 50 + 30 x 33 iterations, gamma in [-0.25, 0.75],
    stop_nconv 1) leaves 0."""
    code = rc.load_code("hgp_12_3_4_s1234")
    hz = sp.csr_matrix(code.checks.z)
    p, B = 0.02, 1000
    e = (np.random.default_rng(2025).random((B, 225)) < p).astype(np.uint8)
    syn = (hz.dot(e.T.astype(np.int64)).T & 1).astype(np.uint8)
    ms = RelayModel(hz, p, np.float64, gamma0=0.0, pre_iter=1040, num_sets=0, alpha=1.0).decode(syn)
    gam = np.random.Generator(np.random.PCG64(0)).uniform(-0.25, 0.75, (30, 225))
    rl = RelayModel(hz, p, np.float64, gamma0=0.125, pre_iter=50, num_sets=30, set_max_iter=33, stop_nconv=1,
                    alpha=1.0, gammas=gam).decode(syn)
    unsat_ms, unsat_rl = int((ms["status"] == 0).sum()), int((rl["status"] == 0).sum())
    print(f"unsatisfied: min-sum(1040) {unsat_ms}, relay {unsat_rl}; mean iterations {ms['iters'].mean():.1f} / "
          f"{rl['iters'].mean():.1f}")
    assert (hz.dot(rl["x"][rl["status"] == 3].T.astype(np.int64)).T & 1 == syn[rl["status"] == 3]).all()
    assert unsat_rl < unsat_ms


# ---------------------------------------------------------------- 4. the slot rule under sanitizers
SAN_FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
FREE = "free (hipFree relay scratch)"
HALVING = ["alloc 8000 oom", "alloc 4000 oom", "alloc 2000 oom", "alloc 1000 oom"]
NO_SLOT = "-> - 0 1000 -58 no memory for one relay slot of 1000 B"
EXPECTED = {
    # the budget is asked first (1 MiB free: 262 slots), then 8 -> 4 -> 2 -> 1 slots refused; every call tries again
    "everything_refused": ["free_bytes", "drain", *HALVING, NO_SLOT,
                           "free_bytes", "drain", *HALVING, NO_SLOT,
                           "drain"],
    # a quarter of 3999 B holds no slot; a quarter of 12000 B holds 3; fewer configured slots: no question
    "budget": ["free_bytes", "-> - 0 0 -59 one relay slot of 1000 B is beyond the scratch budget "
                             "(a quarter of the free device memory)",
               "free_bytes", "drain", "alloc 3000 ok", "-> 3 3000 0 0",
               "-> 2 3000 0 0",
               "drain", FREE],
    # five shots, requests above 2500 B refused: 5 -> 3 -> 2 slots, the mark at 3000; not asked again
    "halved": ["free_bytes", "drain", "alloc 5000 oom", "alloc 3000 oom", "alloc 2000 ok", "-> 2 2000 3000 0",
               "-> 2 2000 3000 0",
               "drain", FREE],
    "other_error": ["free_bytes", "drain", "alloc 8000 error 7", "-> - 0 0 -107 hipMalloc relay scratch: fake error",
                    "drain"],
    # bytes of LDS with the messages in LDS / in HBM, bytes per slot, and the kind that
    # placements LDS / HBM / AUTO launch (-1: none)
    "layouts": ["layout hz225_f32 7440 480 7168 0 1 0",
                "layout dem_f64 2155184 29712 2125568 -1 1 1",
                "layout huge_f32 38250096 1450096 36800000 -1 -1 -1"],
}


def test_relay_slot_rule_is_clean_under_sanitizers_and_follows_the_policy(tmp_path):
    from exp_ldpc_amd import build
    cxx = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(build._hipcc()))), "lib", "llvm", "bin", "clang++")
    assert os.path.exists(cxx), f"ROCm's clang++ not found at {cxx}"
    exe = str(tmp_path / "relay_scratch_check")
    res = subprocess.run([cxx, *SAN_FLAGS, os.path.join(REPO, "tools", "relay_scratch_check.cpp"), "-o", exe],
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
