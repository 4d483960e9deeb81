"""Host tables and argument checks of the fault sampler (qd_sample_faults_device),
on host-only graphs: no GPU."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import dem_model
from exp_ldpc_amd import _abi

PROBS = [0.0, 1e-12, 2.0 ** -32, 0.003, 0.5, 1.0 - 2.0 ** -33, 1.0]
E_NO_PRIORS = -63


def _host_graph(lib, H):
    H = sp.csr_matrix(H)
    H.sort_indices()
    rp = np.ascontiguousarray(H.indptr, np.int32)
    ci = np.ascontiguousarray(H.indices, np.int32)
    h = C.c_void_p()
    _abi.check(lib.qd_graph_create_host(H.shape[0], H.shape[1], _abi.ptr(rp), _abi.ptr(ci), H.shape[1], 1,
                                        C.byref(h)), "qd_graph_create_host")
    return h


def _small():
    """5 x 9: column 3 is empty, column 6 has weight 5."""
    H = np.zeros((5, 9), np.uint8)
    H[:, 6] = 1
    for j, rows in {0: [0, 1], 1: [1], 2: [2, 4], 4: [0, 3], 5: [3], 7: [1, 2, 3], 8: [4]}.items():
        H[rows, j] = 1
    assert H[:, 3].sum() == 0 and H[:, 6].sum() == 5
    return sp.csr_matrix(H)


@pytest.fixture(scope="module")
def lib():
    return _abi.load()


@pytest.fixture(params=["hz225", "small"])
def graph(request, code225):
    return sp.csr_matrix(code225.checks.z) if request.param == "hz225" else _small()


def test_threshold_values():
    """The conversion itself, on the values whose rounding matters."""
    t = dem_model.threshold(PROBS)
    assert t[0] == 0 and t[1] == 0 and t[2] == 1
    assert t[3] == int(np.floor(0.003 * 2.0 ** 32)) and t[4] == 1 << 31
    assert t[5] == 0xFFFFFFFF and t[6] == 0xFFFFFFFF


def test_sample_tables_match_numpy(lib, graph):
    H = graph
    m, n = H.shape
    h = _host_graph(lib, H)
    try:
        thr = np.full(n, 0xDEADBEEF, np.uint32)
        crow = np.full(max(H.nnz, 1), -7, np.int32)
        # before set_priors: the new error code, nothing written
        assert lib.qd_graph_sample_tables_copy(h, _abi.ptr(thr), _abi.ptr(crow)) == E_NO_PRIORS
        assert b"priors not set" in lib.qd_last_error()
        assert (thr == 0xDEADBEEF).all() and (crow == -7).all()
        probs = np.resize(np.array(PROBS, np.float64), n)
        _abi.check(lib.qd_graph_set_priors(h, _abi.ptr(probs)), "qd_graph_set_priors")
        _abi.check(lib.qd_graph_sample_tables_copy(h, _abi.ptr(thr), _abi.ptr(crow)), "sample_tables_copy")
        assert np.array_equal(thr, dem_model.threshold(probs))
        csc = sp.csc_matrix(H)
        csc.sort_indices()
        assert np.array_equal(crow[:H.nnz], csc.indices.astype(np.int32))
        # each output alone
        thr2 = np.zeros(n, np.uint32)
        _abi.check(lib.qd_graph_sample_tables_copy(h, _abi.ptr(thr2), None), "thr only")
        assert np.array_equal(thr2, thr)
        # priors inside (0, 1) afterwards: the thresholds follow the last call
        p2 = np.full(n, 0.25)
        _abi.check(lib.qd_graph_set_priors(h, _abi.ptr(p2)), "qd_graph_set_priors")
        _abi.check(lib.qd_graph_sample_tables_copy(h, _abi.ptr(thr2), None), "thr only")
        assert (thr2 == 1 << 30).all()
    finally:
        lib.qd_graph_destroy(h)


def test_priors_outside_unit_interval_are_refused(lib):
    H = _small()
    h = _host_graph(lib, H)
    try:
        for bad in (-1e-9, 1.0 + 1e-9, float("nan")):
            p = np.full(H.shape[1], 0.1)
            p[4] = bad
            assert lib.qd_graph_set_priors(h, _abi.ptr(p)) == -51
        assert lib.qd_graph_sample_tables_copy(h, None, None) == E_NO_PRIORS
    finally:
        lib.qd_graph_destroy(h)


def test_host_only_graph_is_refused_by_the_sampler(lib, graph):
    H = graph
    h = _host_graph(lib, H)
    try:
        probs = np.full(H.shape[1], 0.01)
        _abi.check(lib.qd_graph_set_priors(h, _abi.ptr(probs)), "qd_graph_set_priors")
        det = np.full((4, H.shape[0]), 9, np.uint8)
        rc = lib.qd_sample_faults_device(h, 1, 0, 0, 4, 0, _abi.ptr(det), None, None, None)
        assert rc == -16 and b"host-only" in lib.qd_last_error()
        assert (det == 9).all()
        assert lib.qd_sample_faults_device(None, 1, 0, 0, 4, 0, _abi.ptr(det), None, None, None) == -1
    finally:
        lib.qd_graph_destroy(h)


def test_numpy_philox_matches_the_oracle(oracle_lib):
    """The model's vectorised Philox4x32-10 against the oracle's block function,
    on 16 counters (word, event, shot low, shot high) with non-zero high words."""
    rng = np.random.default_rng(11)
    ctr = rng.integers(0, 1 << 32, size=(16, 4), dtype=np.uint64).astype(np.uint32)
    ctr[0] = (0, 0, 0, 0)
    ctr[1] = (0xFFFFFFFF, 0, 0xFFFFFFFF, 0)
    ctr[2] = (3, 0, 0, 1)           # shot 2^32
    ctr[3] = (700, 0, 0xFFFFFFFD, 7)
    assert (ctr[:, 3] != 0).sum() >= 3
    key = (20250221, 5)
    got = dem_model.philox4x32_10(ctr, key)
    for i in range(16):
        assert np.array_equal(got[i], oracle_lib.philox(ctr[i], key)), i
    # and the threshold against the oracle's
    for p in PROBS:
        assert int(dem_model.threshold(p)) == oracle_lib.threshold(p), p
