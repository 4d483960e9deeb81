"""Sliding-window decoding on the host (exp_ldpc_amd/window.py):
the window plan against numpy, the ideal-decoder identity of the advance step,
single faults through the CPU oracle, the validation of a boundary's tables
(through the library and, under ASan + UBSan, through tools/window_check.cpp)
and the pipelines' argument checks.  No GPU."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import GOLDEN, REPO
from exp_ldpc_amd.spacetime import SpacetimeCode
from exp_ldpc_amd.window import WindowPlan, spacetime_windows
from window_model import advance_model, column_layers, window_spans, windowed_model

TOY = np.array([[1, 1, 0, 0], [0, 1, 1, 0], [0, 0, 1, 1]], np.uint8)
CASES = [(6, 3, 2), (6, 3, 1), (5, 2, 2), (4, 3, 3), (2, 5, 1)]
SAN_FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def _same(A, B):
    A, B = sp.csr_matrix(A), sp.csr_matrix(B)
    return A.shape == B.shape and (A.astype(np.int64) != B.astype(np.int64)).nnz == 0


def _checks(name, code225):
    return TOY if name == "toy" else code225.checks.z


def test_window_spans_follow_the_rule():
    assert window_spans(6, 3, 2) == [(0, 3, False), (2, 3, False), (4, 3, True)]
    assert window_spans(6, 3, 1) == [(0, 3, False), (1, 3, False), (2, 3, False), (3, 3, False), (4, 3, True)]
    assert window_spans(5, 2, 2) == [(0, 2, False), (2, 2, False), (4, 2, True)]
    assert window_spans(4, 3, 3) == [(0, 3, False), (3, 2, True)]
    assert window_spans(2, 5, 1) == [(0, 3, True)]
    assert window_spans(2, 3, 3) == [(0, 3, True)]


@pytest.mark.parametrize("name", ["toy", "n225"])
@pytest.mark.parametrize("R, W, Cm", CASES)
def test_spacetime_plan_against_numpy(code225, name, R, W, Cm):
    H = sp.csr_matrix(_checks(name, code225))
    r, n = H.shape
    plan = spacetime_windows(H, R, W, Cm)
    Hst = sp.csr_matrix(SpacetimeCode(H, R).spacetime_check_matrix)
    layer = np.arange((R + 1) * r) // r
    cl = np.concatenate([np.repeat(np.arange(R + 1), n), np.repeat(np.arange(R), r)])  # data block t, measurement block t
    assert np.array_equal(plan.col_layer, cl)
    spans = window_spans(R, W, Cm)
    assert [(w.start, w.size, w.final) for w in plan.windows] == spans
    assert plan.n_data == n and plan.k_acc == n
    nonfinal = [w for w in plan.windows if not w.final]
    for w in plan.windows:
        rows = np.flatnonzero((layer >= w.start) & (layer < w.start + w.size))
        cols = np.flatnonzero((cl >= w.start) & (cl < w.start + w.size))
        assert w.row0 == rows[0] and w.m == rows.size and np.array_equal(w.cols, cols)
        assert _same(w.graph, Hst[rows][:, cols])
        assert w.fold_blocks == w.size
        hi = w.start + (w.size if w.final else Cm)
        assert np.array_equal(w.cols[w.committed], np.flatnonzero((cl >= w.start) & (cl < hi)))
    for w in nonfinal:
        assert w.size == W and _same(w.graph, nonfinal[0].graph)
        # [blockdiag(H x W) | M], W measurement blocks, the last of column weight 1
        expect = sp.hstack([sp.block_diag([H] * W), sp.csr_matrix(
            (np.ones(2 * W * r - r), (np.concatenate([np.arange(W * r), np.arange(r, W * r)]),
                                      np.concatenate([np.arange(W * r), np.arange((W - 1) * r)]))),
            shape=(W * r, W * r))])
        assert _same(w.graph, expect)
        weights = np.asarray(sp.csr_matrix(w.graph).sum(axis=0)).ravel()
        assert np.all(weights[W * n + (W - 1) * r:] == 1) and np.all(weights[W * n:W * n + (W - 1) * r] == 2)
    fin = plan.windows[-1]
    assert fin.final and _same(fin.graph, SpacetimeCode(H, R - fin.start).spacetime_check_matrix)
    if W >= R + 1:  # one window: the whole graph
        assert len(plan.windows) == 1 and _same(fin.graph, Hst) and fin.row0 == 0


def test_plan_argument_checks():
    for W, Cm in ((3, 4), (3, 0), (0, 1), (3, -1)):
        with pytest.raises(ValueError):
            spacetime_windows(TOY, 4, W, Cm)
    with pytest.raises(ValueError):
        WindowPlan(TOY, [0, 2, 1], 2, 1)  # layers decrease
    with pytest.raises(ValueError):
        WindowPlan(TOY, [1, 1, 2], 2, 1)  # layers do not start at 0
    assert spacetime_windows(TOY, 4, 4, None).commit == 2 and spacetime_windows(TOY, 4, 1, None).commit == 1


def _ideal(plan, H, row_layer, acc, e, syn):
    """The model with e restricted to each window as its decode, advanced with
    the plan's own tables beside the model's dense rule: every window's syndrome
    must be consistent with its graph, by both."""
    W, Cm = plan.window, plan.commit
    ref = windowed_model(H, row_layer, W, Cm, acc, syn, lambda k, span, Hw, cols, syn_w: e[:, cols])
    syn_t = syn.copy()
    acc_t = np.zeros((e.shape[0], plan.k_acc), np.uint8)
    w0 = plan.windows[0]
    syn_w = advance_model(None, syn_t, None, [], [0], [], [0], [], w0.row0, w0.m)
    for w, rw in zip(plan.windows, ref["windows"]):
        e_w = e[:, w.cols]
        assert np.array_equal(w.cols, rw["cols"]) and np.array_equal(syn_w, rw["syn_w"])
        assert np.array_equal((e_w.astype(np.int64) @ w.graph.T.astype(np.int64)) % 2, syn_w)  # H_w e_w == syn_w
        masked = np.zeros_like(e_w)
        masked[:, w.committed] = e_w[:, w.committed]
        # the tables list committed columns only: the uncommitted part of x must not matter
        outs = []
        for x in (e_w, masked):
            s2, a2 = syn_t.copy(), acc_t.copy()
            nxt = advance_model(x, s2, a2, w.carry_rows, w.carry_ptr, w.carry_cols, w.acc_ptr, w.acc_cols,
                                w.next_row0, w.next_m)
            outs.append((s2, a2, nxt))
        assert all(np.array_equal(p, q) for p, q in zip(*outs))
        syn_t, acc_t, syn_w = outs[0]
    return ref, syn_t, acc_t


@pytest.mark.parametrize("name", ["toy", "n225"])
@pytest.mark.parametrize("R, W, Cm", CASES)
def test_ideal_decoder_identity_spacetime(code225, name, R, W, Cm):
    H = sp.csr_matrix(_checks(name, code225))
    r, n = H.shape
    plan = spacetime_windows(H, R, W, Cm)
    Hst = plan.H
    rng = np.random.default_rng(R * 100 + W * 10 + Cm)
    e = (rng.random((7, Hst.shape[1])) < 0.1).astype(np.uint8)
    syn = ((e.astype(np.int64) @ Hst.T.astype(np.int64)) % 2).astype(np.uint8)
    ref, syn_t, acc_t = _ideal(plan, Hst, plan.row_layer, plan.acc, e, syn)
    fold = np.bitwise_xor.reduce(e[:, :(R + 1) * n].reshape(7, R + 1, n), axis=1)
    assert np.array_equal(ref["x"], e) and np.array_equal(ref["acc"], fold) and np.array_equal(acc_t, fold)
    assert not ((syn.astype(np.int64) + ref["x"].astype(np.int64) @ Hst.T.astype(np.int64)) % 2).any()  # zero residual
    # rows from the final window's start on carry no committed column any more
    last = plan.windows[-1]
    e_last = np.zeros_like(e)
    e_last[:, last.cols] = e[:, last.cols]
    assert np.array_equal(syn_t[:, last.row0:], (e_last.astype(np.int64) @ Hst.T.astype(np.int64) % 2)[:, last.row0:])


def test_ideal_decoder_identity_columns_spanning_three_layers():
    """A hand-made graph, 5 layers of 2 rows, whose columns reach two layers
    ahead; W = 3, C = 1: a column committed after window a carries into rows of
    window a + 2, which is why the full syndrome is updated in place."""
    layer = np.repeat(np.arange(5), 2)
    cols = []
    for t in range(5):
        for rows in ((2 * t, 2 * t + 2, 2 * t + 5), (2 * t + 1, 2 * t + 4), (2 * t, 2 * t + 1), (2 * t + 1, 2 * t + 3, 2 * t + 4)):
            cols.append([g for g in rows if g < 10])
    H = np.zeros((10, len(cols)), np.uint8)
    for j, rows in enumerate(cols):
        H[rows, j] = 1
    assert np.array_equal(column_layers(H, layer), np.repeat(np.arange(5), 4))
    rng = np.random.default_rng(5)
    acc = (rng.random((3, H.shape[1])) < 0.4).astype(np.uint8)
    plan = WindowPlan(H, layer, 3, 1, acc=acc)
    assert [(w.start, w.size, w.final) for w in plan.windows] == [(0, 3, False), (1, 3, False), (2, 3, True)]
    # window 0 commits layer 0, whose first column touches row 5 (layer 2): beyond window 1's first layer
    assert plan.windows[0].carry_rows.max() >= 4 and plan.windows[0].next_row0 == 2
    e = (rng.random((33, H.shape[1])) < 0.3).astype(np.uint8)
    syn = (e.astype(np.int64) @ H.T.astype(np.int64) % 2).astype(np.uint8)
    ref, syn_t, acc_t = _ideal(plan, H, layer, acc, e, syn)
    want = (e.astype(np.int64) @ acc.T.astype(np.int64) % 2).astype(np.uint8)
    assert np.array_equal(ref["x"], e) and np.array_equal(ref["acc"], want) and np.array_equal(acc_t, want)
    assert np.array_equal(syn_t, ref["syn"])  # the tables and the dense rule leave the same full syndrome


def test_whole_graph_window(code225):
    H = sp.csr_matrix(code225.checks.z)
    for R, W in ((2, 3), (2, 5), (0, 1)):
        plan = spacetime_windows(H, R, W, 1)
        assert len(plan.windows) == 1
        w = plan.windows[0]
        assert w.final and w.row0 == 0 and _same(w.graph, SpacetimeCode(H, R).spacetime_check_matrix)
        assert np.array_equal(w.cols, np.arange(plan.n)) and w.carry_rows.size == 0


def test_single_faults_through_the_oracle(code225, oracle_lib):
    """n = 225, (R, W, C) = (4, 3, 1), min-sum f64 at p = 0.01 (priors 2p/3 on
    data and measurement columns alike, 50 iterations): every single-column
    fault of the spacetime graph, decoded window by window by the CPU oracle,
    must end with zero residual and corr == fold(e_j).  The columns that do not
    are pinned by tests/golden/window_single_faults_r4_w3_c1.json."""
    H = sp.csr_matrix(code225.checks.z)
    r, n = H.shape
    R, W, Cm = 4, 3, 1
    plan = spacetime_windows(H, R, W, Cm)
    Hst = plan.H
    N = Hst.shape[1]
    e = np.eye(N, dtype=np.uint8)
    syn = np.ascontiguousarray(Hst.T.toarray().astype(np.uint8) % 2)
    prior = 2 * 0.01 / 3

    def decode(k, span, Hw, cols, syn_w):
        return oracle_lib.decode(sp.csr_matrix(Hw), prior, syn_w, method="ms", precision="f64", max_iter=50,
                                 n_data=n, fold_blocks=span[1], want_llr=False)["x"]
    ref = windowed_model(Hst, plan.row_layer, W, Cm, plan.acc, syn, decode)
    resid = (syn.astype(np.int64) + ref["x"].astype(np.int64) @ Hst.T.astype(np.int64)) % 2
    fold = np.bitwise_xor.reduce(e[:, :(R + 1) * n].reshape(N, R + 1, n), axis=1)
    bad = np.flatnonzero(resid.any(axis=1) | (ref["acc"] != fold).any(axis=1))
    with open(os.path.join(GOLDEN, "window_single_faults_r4_w3_c1.json")) as f:
        pinned = json.load(f)["failing_columns"]
    print("failing single faults:", bad.tolist())
    assert bad.tolist() == pinned


# ------------------------------------------------------------------ validation
VALID = dict(n_w=8, m_total=10, rows=[4, 7, 9], cptr=[0, 2, 2, 3], ccols=[0, 7, 3], aptr=[0, 1, 3], acols=[7, 0, 1],
             row0=4, m_next=6)
MALFORMED = {
    "carry_rows_unsorted": (dict(rows=[4, 9, 7]), -22),
    "carry_row_repeated": (dict(rows=[4, 7, 7]), -22),
    "carry_row_out_of_range": (dict(rows=[4, 7, 10]), -22),
    "carry_row_negative": (dict(rows=[-1, 7, 9]), -22),
    "carry_column_out_of_range": (dict(ccols=[0, 7, 8]), -23),
    "acc_column_negative": (dict(acols=[7, -1, 1]), -23),
    "acc_column_out_of_range": (dict(acols=[7, 0, 8]), -23),
    "carry_ptr_decreases": (dict(cptr=[0, 2, 1, 3]), -24),
    "carry_ptr_not_from_zero": (dict(cptr=[1, 2, 2, 3]), -24),
    "acc_ptr_decreases": (dict(aptr=[0, 3, 1]), -24),
    "next_rows_beyond_total": (dict(row0=5), -25),
    "next_rows_overflow": (dict(row0=0x7fffffff, m_next=0x7fffffff), -25),
    "no_columns": (dict(n_w=0), -26),
    "too_many_columns": (dict(n_w=(1 << 19) + 1), -26),
}
WELL_FORMED = {
    "valid": {},
    "empty_tables": dict(rows=[], cptr=[0], ccols=[], aptr=[0], acols=[]),
    "last_column": dict(ccols=[0, 7, 3], acols=[7, 0, 1]),
}


def _create_host(lib, **over):
    a = {**VALID, **over}
    arr = {k: np.ascontiguousarray(a[k], dtype=np.int32) for k in ("rows", "cptr", "ccols", "aptr", "acols")}
    from exp_ldpc_amd import _abi
    h = C.c_void_p()
    rc = lib.qd_window_create_host(a["n_w"], a["m_total"], arr["rows"].size, _abi.ptr(arr["rows"]), _abi.ptr(arr["cptr"]),
                                   _abi.ptr(arr["ccols"]), arr["aptr"].size - 1, _abi.ptr(arr["aptr"]),
                                   _abi.ptr(arr["acols"]), a["row0"], a["m_next"], C.byref(h))
    return rc, h


def test_create_host_refuses_each_malformed_table_with_its_own_code():
    from exp_ldpc_amd import _abi
    lib = _abi.load()
    for name, over in WELL_FORMED.items():
        rc, h = _create_host(lib, **over)
        assert rc == 0 and h.value, name
        # a host-only boundary validates and never runs; its grid setting is range-checked
        assert lib.qd_window_advance_device(h, 1, None, None, None, None, None) == -16
        assert lib.qd_window_set_blocks(h, 2) == 0 and lib.qd_window_set_blocks(h, -1) == -29
        assert lib.qd_window_set_blocks(h, (1 << 20) + 1) == -29
        assert lib.qd_window_destroy(h) == 0
    for name, (over, code) in MALFORMED.items():
        rc, h = _create_host(lib, **over)
        assert rc == code and not h.value, (name, rc)
        assert b"window" in lib.qd_last_error()
    assert len({code for _, code in MALFORMED.values()}) == 5  # one code per kind of refusal
    assert lib.qd_window_create_host(8, 10, 0, None, None, None, 0, None, None, 0, 0, C.byref(C.c_void_p())) == -26
    assert lib.qd_window_destroy(None) == 0


@pytest.fixture(scope="module")
def window_check(tmp_path_factory):
    """tools/window_check.cpp with the HIP-free validation unit, built once with ROCm's clang++."""
    from exp_ldpc_amd import build
    cxx = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(build._hipcc()))), "lib", "llvm", "bin", "clang++")
    assert os.path.exists(cxx), f"ROCm's clang++ not found at {cxx}"
    exe = str(tmp_path_factory.mktemp("window_check") / "window_check")
    res = subprocess.run([cxx, *SAN_FLAGS, os.path.join(REPO, "tools", "window_check.cpp"),
                          os.path.join(REPO, "exp_ldpc_amd", "csrc", "qdec_window.cpp"), "-o", exe],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]
    return exe


def test_validation_is_clean_under_sanitizers(window_check):
    """The stand-alone checker (its own main, the HIP-free unit alone, a static
    sanitizer runtime: an ordinary child process) exits 0 with no report and
    gives every case the code the library gives it."""
    res = subprocess.run([window_check], capture_output=True, text=True)
    assert res.returncode == 0 and res.stderr == "", f"exit {res.returncode}\n{res.stderr[-4000:]}"
    got = dict(line.rsplit(" ", 1) for line in res.stdout.splitlines())
    want = {**{k: "0" for k in WELL_FORMED}, **{k: str(code) for k, (_, code) in MALFORMED.items()}}
    assert got == want


# ------------------------------------------------------------------ pipeline arguments
OPTS = {"max_iter": 30, "bp_method": "ms", "ms_scaling_factor": 0, "osd_method": "osd_cs", "osd_order": 2}


def test_pipeline_window_arguments(code225):
    """Refused before any device work: window with a mode other than bp / bposd,
    commit > window, commit = 0 (and a commit without a window)."""
    from exp_ldpc_amd.experiment import DECODER_MODES, BatchPipeline, p_sweep
    for mode in DECODER_MODES:
        if mode in ("bp", "bposd"):
            continue
        with pytest.raises(ValueError, match="window"):
            BatchPipeline(code225, 4, mode, OPTS, (0.01, 0.01), window=3)
    for mode in ("bp", "bposd"):
        for window, commit in ((3, 4), (3, 0), (0, None)):
            with pytest.raises(ValueError):
                BatchPipeline(code225, 4, mode, OPTS, (0.01, 0.01), window=window, commit=commit)
        with pytest.raises(ValueError):
            BatchPipeline(code225, 4, mode, OPTS, (0.01, 0.01), commit=1)
    with pytest.raises(ValueError, match="window"):
        p_sweep(10, [0.01], None, lambda p: {}, lambda *a: 0.01, lambda *a: 0.01, code=code225, rounds=4,
                decoder_mode="bposd_hybrid", bp_osd_options=OPTS, window=3)
    with pytest.raises(ValueError):
        p_sweep(10, [0.01], None, lambda p: {}, lambda *a: 0.01, lambda *a: 0.01, code=code225, rounds=4,
                decoder_mode="bp", bp_osd_options=OPTS, window=3, commit=4)
