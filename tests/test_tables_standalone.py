"""The host table builders (exp_ldpc_amd/csrc/qdec_tables.cpp) under ASan + UBSan.

tools/tables_check.cpp links the builders alone, with no HIP header on the
include path -- compiling it is the proof that they are HIP-free -- and a static
sanitizer runtime, so the program runs as an ordinary child process (this test
sets up no preload).  For every input it must exit 0, print no sanitizer
report, and print the digest and byte count libqdec_hip.so reports for the same
input through qd_graph_create_host: same tables, byte for byte, in the same
upload order."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

SAN_FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _i32(a):
    return np.ascontiguousarray(a, np.int32)


def _csr(rows):
    """(ptr, idx) of a list of index lists, entries kept as given."""
    ptr = np.cumsum([0] + [len(r) for r in rows])
    return _i32(ptr), _i32(np.concatenate([np.asarray(r, np.int64) for r in rows] + [np.zeros(0, np.int64)]))


def _spread_graph(m_used, n_used, E, m, n, seed):
    """E edges, edge t in row t % m_used and column perm[t % n_used]: row and
    column degrees within one of each other, rows >= m_used and the columns the
    permutation leaves out have degree 0.  No repeated entry while E <=
    lcm(m_used, n_used)."""
    perm = np.random.default_rng(seed).permutation(n)
    rows = [[] for _ in range(m)]
    for t in range(E):
        rows[t % m_used].append(int(perm[t % n_used]))
    return [sorted(r) for r in rows]


def _cases(code225):
    rng = np.random.default_rng(2025)
    out = {}
    # the n = 225 HGP code: wave shape (2, 4, 7), every generator shares one 4096-entry table
    hz, hx, lz = (sp.csr_matrix(a) for a in (code225.checks.z, code225.checks.x, code225.logicals.z))
    for a in (hz, hx, lz):
        a.sort_indices()
    g225 = (hz.shape[0], 225, _i32(hz.indptr), _i32(hz.indices))
    out["n225"] = dict(graph=g225, gens=(_i32(hx.indptr), _i32(hx.indices)), lz=(_i32(lz.indptr), _i32(lz.indices)),
                       probs=np.full(225, 0.01))
    # k > 256 logicals (no lane-slot copy), supports with repeated entries; one
    # p = 0.5: a zero prior, no iteration-1 table for either precision
    many = [list(rng.integers(0, 225, 3)) + [7, 7] for _ in range(260)]
    p = np.full(225, 0.02)
    p[100] = 0.5
    out["n225_k260_zero_prior"] = dict(graph=g225, lz=_csr(many), probs=p)
    # wave shape (2, 3, 6): RC * 64 > m
    rows = _spread_graph(60, 160, 300, 60, 160, 1)
    assert max(map(len, rows)) <= 6
    g236 = (60, 160, *_csr(rows))
    # > 128 generators (no per-lane tables), k = 0, priors with exact ties
    pairs = [sorted(rng.choice(160, 2, replace=False)) for _ in range(130)]
    out["wave236_130gens_k0_ties"] = dict(graph=g236, gens=_csr(pairs), lz=_csr([]),
                                          probs=np.where(np.arange(160) % 3 == 0, 0.01, 0.02))
    # generators of several local shapes; supports whose pairs cancel (one to nothing)
    few = [sorted(rng.choice(160, 1 + i % 4, replace=False)) for i in range(20)]
    out["wave236_shapes_dups"] = dict(graph=g236, gens=_csr(few), lz=_csr([[3, 9, 3, 150], [5, 5], [0, 1, 2, 2, 2]]),
                                      probs=rng.uniform(0.001, 0.2, 160))
    # no wave shape (n > 576) but the LDS-resident kernels' layouts (ml_positions,
    # m64_layout: 1500 E anneal steps); rows 140.. and 370 columns have degree 0
    rows = _spread_graph(140, 230, 690, 150, 600, 2)
    assert max(map(len, rows)) <= 8
    cols = {}
    for i, r in enumerate(rows):
        for j in r:
            cols.setdefault(j, set()).add(i)
    # one generator touching > 16 checks (no table-driven SSF): 8 columns with disjoint rows
    wide, seen = [], set()
    for j in sorted(cols):
        if len(wide) < 8 and not (cols[j] & seen):
            wide.append(j)
            seen |= cols[j]
    assert 16 < len(seen) <= 32
    out["lds_wide_generator"] = dict(graph=(150, 600, *_csr(rows)), gens=_csr([wide, sorted(cols)[:2]]),
                                     probs=rng.uniform(0.001, 0.2, 600))
    # ragged: a row of degree 9 (workgroup kernels, no LDS tables), empty rows
    rows = [sorted(rng.choice(100, 9 if i == 0 else (0 if i in (5, 6) else 1 + i % 5), replace=False))
            for i in range(40)]
    out["ragged_deg9"] = dict(graph=(40, 100, *_csr(rows)), lz=_csr([[1, 2, 3], [99]]),
                              probs=rng.uniform(0.001, 0.2, 100))
    return out


def _library_digest(lib, graph, gens=None, lz=None, probs=None):
    from exp_ldpc_amd import _abi
    m, n, rp, ci = graph
    h = C.c_void_p()
    _abi.check(lib.qd_graph_create_host(m, n, _abi.ptr(rp), _abi.ptr(ci), n, 1, C.byref(h)), "qd_graph_create_host")
    if gens is not None:
        _abi.check(lib.qd_graph_set_flipsets(h, len(gens[0]) - 1, _abi.ptr(gens[0]), _abi.ptr(gens[1])), "flipsets")
    if lz is not None:
        _abi.check(lib.qd_graph_set_logicals_csr(h, len(lz[0]) - 1, _abi.ptr(lz[0]), _abi.ptr(lz[1])), "logicals")
    if probs is not None:
        pr = np.ascontiguousarray(probs, np.float64)
        _abi.check(lib.qd_graph_set_priors(h, _abi.ptr(pr)), "priors")
    d, nb = C.c_uint64(0), C.c_int64(0)
    _abi.check(lib.qd_graph_table_digest(h, C.byref(d), C.byref(nb)), "digest")
    assert lib.qd_graph_destroy(h) == 0
    return d.value, nb.value


def _write_input(path, graph, gens=None, lz=None, probs=None):
    m, n, rp, ci = graph
    none = (np.zeros(0, np.int32), np.zeros(0, np.int32))
    gp, gi = gens if gens is not None else none
    lp, li = lz if lz is not None else none
    head = [m, n, n, 1, ci.size, gp.size - 1, gi.size, lp.size - 1, li.size, int(probs is not None)]
    with open(path, "wb") as f:
        for a in (_i32(head), rp, ci, gp, gi, lp, li):
            f.write(a.astype("<i4").tobytes())
        if probs is not None:
            f.write(np.asarray(probs).astype("<f8").tobytes())


@pytest.fixture(scope="session")
def tables_check(tmp_path_factory):
    """tools/tables_check.cpp + qdec_tables.cpp, built once with ROCm's clang++."""
    from exp_ldpc_amd import build
    cxx = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(build._hipcc()))), "lib", "llvm", "bin", "clang++")
    assert os.path.exists(cxx), f"ROCm's clang++ not found at {cxx}"
    exe = str(tmp_path_factory.mktemp("tables_check") / "tables_check")
    res = subprocess.run([cxx, *SAN_FLAGS, os.path.join(REPO, "tools", "tables_check.cpp"),
                          os.path.join(build.CSRC, "qdec_tables.cpp"), "-o", exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]
    return exe


def test_table_builders_are_clean_under_sanitizers_and_match_the_library(code225, tables_check, tmp_path):
    from exp_ldpc_amd import _abi
    lib = _abi.load()
    for name, case in _cases(code225).items():
        path = str(tmp_path / (name + ".bin"))
        _write_input(path, **case)
        res = subprocess.run([tables_check, path], capture_output=True, text=True)
        assert res.returncode == 0 and res.stderr == "", f"{name}: exit {res.returncode}\n{res.stderr[-4000:]}"
        digest, nbytes = res.stdout.split()
        assert (int(digest, 16), int(nbytes)) == _library_digest(lib, **case), name
