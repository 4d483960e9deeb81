"""The first check state of the compact min-sum kernel (ms_state0_table,
qdec_tables.cpp), built by a host-only graph, against a numpy restatement of
the kernel's first check pass: per check lane the two smallest |prior| of the
row (Big where the row has fewer, pads all Big), both negated on odd parity of
`prior <= 0`; f64 follows the sign-bit rule (a row holding a zero gives m2 the
parity flipped when a zero is +0), f32 the compares.  Bit for bit, in both
precisions.  tools/tables_check.cpp runs the same builder under ASan + UBSan."""
import ctypes as C
import math

import numpy as np
import pytest
import scipy.sparse as sp

from exp_ldpc_amd import _abi

BIG = {"f64": 1e308, "f32": 1e30}


def _host_graph(lib, H, probs):
    H = sp.csr_matrix(H)
    H.sort_indices()
    rp = np.ascontiguousarray(H.indptr, np.int32)
    ci = np.ascontiguousarray(H.indices, np.int32)
    h = C.c_void_p()
    _abi.check(lib.qd_graph_create_host(H.shape[0], H.shape[1], _abi.ptr(rp), _abi.ptr(ci), H.shape[1], 1,
                                        C.byref(h)), "qd_graph_create_host")
    _set_priors(lib, h, probs)
    return h


def _set_priors(lib, h, probs):
    pr = np.ascontiguousarray(probs, np.float64)
    _abi.check(lib.qd_graph_set_priors(h, _abi.ptr(pr)), "priors")


def _copy(lib, h, precision):
    prec = _abi.QD_F64 if precision == "f64" else _abi.QD_F32
    mp = C.c_int32(0)
    _abi.check(lib.qd_graph_ms_state0_copy(h, prec, None, None, C.byref(mp)), "state0 size")
    st = np.zeros((mp.value, 2), np.float64 if precision == "f64" else np.float32)
    ss = np.zeros(mp.value, np.uint16)
    _abi.check(lib.qd_graph_ms_state0_copy(h, prec, _abi.ptr(st), _abi.ptr(ss), None), "state0 copy")
    return st, ss


def _restate(H, probs, precision, m_pad):
    """The kernel's first check pass in numpy (priors: the library's
    log((1 - p) / p) in double, rounded to float for f32)."""
    T = np.float64 if precision == "f64" else np.float32
    H = sp.csr_matrix(H)
    H.sort_indices()
    L = np.array([math.log((1 - p) / p) for p in probs], np.float64).astype(T)
    big = T(BIG[precision])
    out = np.full((m_pad, 2), big, T)
    for i in range(H.shape[0]):
        v = L[H.indices[H.indptr[i]:H.indptr[i + 1]]]
        av = np.sort(np.abs(v))
        m1 = av[0] if len(av) > 0 else big
        m2 = av[1] if len(av) > 1 else big
        par = bool(np.count_nonzero(v <= 0) & 1)
        plus_zero = bool(np.any((v == 0) & ~np.signbit(v)))
        neg2 = par ^ (precision == "f64" and m1 == 0 and plus_zero)
        out[i, 0] = -m1 if par else m1
        out[i, 1] = -m2 if neg2 else m2
    return out


def _cases(code225):
    hz = sp.csr_matrix(code225.checks.z)
    hz.sort_indices()
    n = hz.shape[1]
    rng = np.random.default_rng(11)
    row = hz.indices[hz.indptr[5]:hz.indptr[6]]
    equal = np.full(n, 2 * 0.01 / 3)
    ties = rng.choice([0.001, 0.01, 0.02, 0.05, 0.1], size=n)
    zero_neg = ties.copy()
    zero_neg[row[0]], zero_neg[row[1]] = 0.5, 0.7  # +0 and a negative LLR in row 5
    zero_alone = equal.copy()
    zero_alone[row[2]] = 0.5
    small = sp.csr_matrix(np.array([[1, 0, 0, 0], [1, 1, 1, 0], [0, 1, 1, 1]], np.uint8))  # row 0: degree 1
    return {"equal": (hz, equal), "ties": (hz, ties), "zero_and_negative": (hz, zero_neg),
            "zero_alone": (hz, zero_alone), "all_zero": (hz, np.full(n, 0.5)),
            "degree_one_row": (small, np.array([0.01, 0.02, 0.02, 0.6]))}


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("case", ["equal", "ties", "zero_and_negative", "zero_alone", "all_zero", "degree_one_row"])
def test_ms_state0_equals_the_first_check_pass(code225, precision, case):
    lib = _abi.load()
    H, probs = _cases(code225)[case]
    h = _host_graph(lib, H, probs)
    try:
        st, ss = _copy(lib, h, precision)
        m = H.shape[0]
        assert st.shape[0] % 64 == 0 and st.shape[0] >= m
        assert len(set(ss[:m].tolist())) == m  # distinct state slots: the copy is by check lane
        ref = _restate(H, probs, precision, st.shape[0])
        U = np.uint64 if precision == "f64" else np.uint32
        assert np.array_equal(st.view(U), ref.view(U)), case  # bit patterns: signs of zeros count
        if case == "degree_one_row":
            assert st[0, 1] == st.dtype.type(BIG[precision]) and st[0, 0] < 10
        if case == "zero_and_negative":  # row 5: m1 = 0, parity odd twice over -> even; +0 flips m2 in f64 only
            assert st[5, 0] == 0 and not np.signbit(st[5, 0])
            assert np.signbit(st[5, 1]) == (precision == "f64")
    finally:
        lib.qd_graph_destroy(h)


def test_ms_state0_follows_set_priors(code225):
    """A second set_priors rebuilds the table; priors with a 0 or a 1 drop it."""
    lib = _abi.load()
    hz = sp.csr_matrix(code225.checks.z)
    n = hz.shape[1]
    h = _host_graph(lib, hz, np.full(n, 0.01))
    try:
        a, _ = _copy(lib, h, "f64")
        probs = np.random.default_rng(2).uniform(0.01, 0.2, n)
        _set_priors(lib, h, probs)
        b, _ = _copy(lib, h, "f64")
        assert not np.array_equal(a, b)
        assert np.array_equal(b.view(np.uint64), _restate(hz, probs, "f64", b.shape[0]).view(np.uint64))
        _set_priors(lib, h, np.where(np.arange(n) == 3, 0.0, 0.01))
        assert lib.qd_graph_ms_state0_copy(h, _abi.QD_F64, None, None, None) == -39
    finally:
        lib.qd_graph_destroy(h)
