"""Every device OSD kernel shape at its edges, on rank-deficient graphs.

launch_osd (csrc/qdec_osd.hip) picks osd_wave_kernel<RS, W> from m and n alone
(RS = 2 / 4 / 6 for m <= 128 / 256 / 384, W = the first built width >=
ceil((n + 1) / 64)), or the workgroup kernel.  TABLE holds two small synthetic
graphs per register shape, at its two edges in n (low: n = 64 * the previous
built width of that RS, the syndrome bit alone in bit 0 of a word; high:
n = 64 W - 1, the syndrome bit in bit 63 of the last word; the first width of an
RS has no previous one, its low graph is a small one with m > n), with m at the
edges of RS, and the workgroup kernel's corners (m > n; three rows of 17 words;
an LDS image just under the 160 KiB limit; one graph past it, which no device
kernel holds).  Every graph is rank-deficient on
purpose: a duplicated row, a row that is the XOR of two others, an all-zero row
and an all-zero column (graphs of 1 or 3 rows take what fits).

Per graph B = 48 shots, the inputs a function of the shot index b alone:
  * LLR family b % 4: (a) all equal, (b) drawn from {-1.5, -0.0, +0.0, 0.5, 2.0},
    (c) distinct normals, (d) as (c) with +-inf and denormals mixed in; fed
    straight to osd_device as float64, and as the same values rounded to float32
    (reference: those float32 values widened);
  * syndrome kind (b // 4) % 2: H e, or arbitrary bits (mostly outside the image);
  * b % 3 == 2: marked converged, the device must leave the row's fill alone.
References: the host stage (OsdSolver, every shot) and the independent numpy
checker (oracle/osd_py.py, CHECK_SHOTS: the first two unconverged shots of each
family and syndrome kind, 16 per graph, chosen by index).

The numpy checker on the largest graph (384 x 1023) takes 0.07 s per shot at
osd_cs 64 and 0.13 s for all eight methods of a shot (one CPU core), so order 64
stays in the checker subset on every graph.
"""
import ctypes as C
import functools
import zlib
from collections import namedtuple

import numpy as np
import pytest

from conftest import REPO  # noqa: F401  (puts the repository on sys.path)

# (RS, W) of every osd_wave_kernel instantiation the library builds
# (QDEC_OSD_SHAPES in csrc/qdec_osd.hip), written once: a shape added there
# without rows here fails test_table_reaches_every_kernel.
OSD_SHAPES = [(2, 4), (2, 6), (2, 9), (2, 16), (4, 6), (4, 9), (4, 12), (4, 16), (6, 14), (6, 16)]
BLOCK = (0, None)  # the workgroup kernel (RS = 0; W follows n)
LDS_LIMIT = 160 * 1024

Row = namedtuple("Row", "name m n shape")
TABLE = [
    # register shapes: low edge, high edge
    Row("w2x4_lo_trivial", 1, 2, (2, 4)), Row("w2x4_hi", 64, 255, (2, 4)),
    Row("w2x6_lo", 65, 256, (2, 6)), Row("w2x6_hi", 128, 383, (2, 6)),
    Row("w2x9_lo_one_row", 1, 384, (2, 9)), Row("w2x9_hi", 128, 575, (2, 9)),
    Row("w2x16_lo", 64, 576, (2, 16)), Row("w2x16_hi", 65, 1023, (2, 16)),
    Row("w4x6_lo_m_gt_n", 129, 40, (4, 6)), Row("w4x6_hi", 256, 383, (4, 6)),
    Row("w4x9_lo", 256, 384, (4, 9)), Row("w4x9_hi", 129, 575, (4, 9)),
    Row("w4x12_lo", 129, 576, (4, 12)), Row("w4x12_hi", 256, 767, (4, 12)),
    Row("w4x16_lo", 256, 768, (4, 16)), Row("w4x16_hi", 129, 1023, (4, 16)),
    Row("w6x14_lo_m_gt_n", 257, 64, (6, 14)), Row("w6x14_hi", 384, 895, (6, 14)),
    Row("w6x16_lo", 257, 896, (6, 16)), Row("w6x16_hi", 384, 1023, (6, 16)),
    # workgroup kernel
    Row("blk_m_gt_n", 385, 100, BLOCK), Row("blk_three_rows", 3, 1024, BLOCK),
    Row("blk_near_limit", 187, 4095, BLOCK),
    Row("blk_past_limit", 188, 4095, None),  # 8 more row words than fit: no device kernel
]
SUPPORTED = [r for r in TABLE if r.shape is not None]
PAST_LIMIT = next(r for r in TABLE if r.shape is None)

METHODS = [("osd0", 0), ("osd_e", 0), ("osd_e", 1), ("osd_e", 10),
           ("osd_cs", 0), ("osd_cs", 1), ("osd_cs", 7), ("osd_cs", 64)]  # 64 = kOsdMaxLam
B = 48
FAMILIES = ("equal", "five_values", "normals", "normals_inf_denormal")


def _family(b):
    return b % 4


def _arbitrary(b):
    return (b // 4) % 2 == 1


def _converged(b):
    return b % 3 == 2


def _check_shots():
    out = []
    for f in range(4):
        for kind in (False, True):
            out += [b for b in range(B) if _family(b) == f and _arbitrary(b) == kind and not _converged(b)][:2]
    return sorted(out)


CHECK_SHOTS = _check_shots()
BAD = np.array([b for b in range(B) if not _converged(b)])
GOOD = np.array([b for b in range(B) if _converged(b)])


# ------------------------------------------------------------------ the graphs
def _overlapping_pair(rng, pool):
    """Two supports of weight 3..6 sharing two columns, their XOR of weight 3..8."""
    a = rng.choice(pool, size=int(rng.integers(4, 7)), replace=False)
    rest = np.setdiff1d(pool, a)
    c = np.concatenate([a[:2], rng.choice(rest, size=int(rng.integers(1, 5)), replace=False)])
    return sorted(a.tolist()), sorted(c.tolist())


def _rows(m, n, seed):
    rng = np.random.default_rng(seed)
    if n == 2:
        return [[0, 1]]
    zero_col = int(rng.integers(n))
    pool = np.array([j for j in range(n) if j != zero_col])
    if m == 1:
        return [sorted(rng.choice(pool, size=5, replace=False).tolist())]
    if m == 3:  # a, b, a ^ b
        a, c = _overlapping_pair(rng, pool)
        return [a, c, sorted(set(a) ^ set(c))]
    assert m >= 8 and pool.size >= 12
    rows = [sorted(rng.choice(pool, size=int(rng.integers(2, 9)), replace=False).tolist()) for _ in range(m - 3)]
    rows[1], rows[2] = _overlapping_pair(rng, pool)
    for extra in (list(rows[0]), sorted(set(rows[1]) ^ set(rows[2])), []):  # duplicate, XOR of two, all-zero
        rows.insert(int(rng.integers(len(rows) + 1)), extra)
    return rows


@functools.lru_cache(maxsize=None)
def graph(name):
    from exp_ldpc_amd.codes import make_check_matrix
    from exp_ldpc_amd.decoder import as_csr01
    row = next(r for r in TABLE + FUSED_ROWS if r.name == name)
    H = as_csr01(make_check_matrix(_rows(row.m, row.n, zlib.crc32(name.encode())), row.n))
    assert H.shape == (row.m, row.n)
    return H


@functools.lru_cache(maxsize=None)
def rank_and_left_null(name):
    """(rank of H, N with N H = 0 spanning the left null space): s is in the
    image of H exactly when N s = 0.  Plain elimination of [H | I] by rows."""
    H = graph(name)
    m, n = H.shape
    A = np.concatenate([H.toarray().astype(np.uint8) & 1, np.eye(m, dtype=np.uint8)], axis=1)
    r = 0
    for c in range(n):
        hit = np.nonzero(A[r:, c])[0]
        if hit.size == 0:
            continue
        A[[r, r + hit[0]]] = A[[r + hit[0], r]]
        rows = np.nonzero(A[:, c])[0]
        rows = rows[rows != r]
        A[rows] ^= A[r]
        r += 1
        if r == m:
            break
    assert not A[r:, :n].any()
    return r, A[r:, n:].astype(np.int64)


# ------------------------------------------------------------------ the inputs
_SPECIALS = np.array([np.inf, -np.inf, np.inf, 5e-324, -5e-324, 1e-310, 1e-40, -1e-40, 2.2250738585072014e-308,
                      -np.inf])


@functools.lru_cache(maxsize=None)
def inputs(name, precision):
    """syn uint8[B, m], llr [B, n] in the precision's dtype, ref_llr = llr as
    float64, status uint8[B], in_image bool[B]."""
    H = graph(name)
    m, n = H.shape
    rng = np.random.default_rng(zlib.crc32((name + "/inputs").encode()))
    e = (rng.random((B, n)) < 0.03).astype(np.int64)
    syn = ((H @ e.T).T % 2).astype(np.uint8)
    arb = rng.integers(0, 2, size=(B, m)).astype(np.uint8)
    llr = np.empty((B, n), np.float64)
    status = np.zeros(B, np.uint8)
    for b in range(B):
        if _arbitrary(b):
            syn[b] = arb[b]
        normals = rng.normal(1.0, 2.0, n)
        five = rng.choice([-1.5, -0.0, 0.0, 0.5, 2.0], n)
        where = rng.random(n) < 0.15
        special = rng.choice(_SPECIALS, n)
        f = _family(b)
        llr[b] = (np.full(n, 0.75), five, normals, np.where(where, special, normals))[f]
        # bit 0 = BP converged; bit 1 alone (2) is not a reason to skip the shot
        status[b] = (1, 3)[b % 2] if _converged(b) else (0, 2)[b % 2]
    if precision == "f32":
        llr = llr.astype(np.float32)  # 5e-324 and 1e-310 round to +-0, 1e-40 to a float32 denormal
    _, N = rank_and_left_null(name)
    in_image = ~((N @ syn.T.astype(np.int64)) % 2).any(axis=0)
    assert in_image[[b for b in range(B) if not _arbitrary(b)]].all()
    out = {"syn": np.ascontiguousarray(syn), "llr": np.ascontiguousarray(llr), "ref_llr": llr.astype(np.float64),
           "status": status, "in_image": in_image}
    for v in out.values():
        v.setflags(write=False)
    return out


# ------------------------------------------------------------------ the references, computed once
@functools.lru_cache(maxsize=None)
def host_ref(name, precision, method, order):
    """The host stage on every shot: (osd0, osdw) uint8[B, n]."""
    from exp_ldpc_amd.osd import OsdSolver
    x = inputs(name, precision)
    o0, ow = OsdSolver(graph(name), method, order).solve(x["syn"], x["ref_llr"])
    o0.setflags(write=False)
    ow.setflags(write=False)
    return o0, ow


_CHECKER = {}


def checker_ref(name, precision, b):
    """The numpy checker on shot b: [(osd0, osdw)] in METHODS' order.  Families
    (a) and (b) hold float32 values, so both precisions share their entry."""
    from oracle.osd_py import osd_decode_methods
    x = inputs(name, precision)
    key = (name, b, x["ref_llr"][b].tobytes())
    if key not in _CHECKER:
        _CHECKER[key] = osd_decode_methods(graph(name), x["syn"][b], x["ref_llr"][b], METHODS)
    return _CHECKER[key]


def _host_graph(H):
    from exp_ldpc_amd import _abi
    lib = _abi.load()
    rp = np.ascontiguousarray(H.indptr, dtype=np.int32)
    ci = np.ascontiguousarray(H.indices, dtype=np.int32)
    h = C.c_void_p()
    _abi.check(lib.qd_graph_create_host(H.shape[0], H.shape[1], _abi.ptr(rp), _abi.ptr(ci), H.shape[1], 1,
                                        C.byref(h)), "qd_graph_create_host")
    return lib, h


def _kernel_info_on_host(name):
    from exp_ldpc_amd.decoder import osd_kernel_info
    lib, h = _host_graph(graph(name))
    try:
        return osd_kernel_info(h), bool(lib.qd_osd_device_supported(h))
    finally:
        lib.qd_graph_destroy(h)


def _expected_w(row):
    return (row.n + 1 + 63) // 64 if row.shape == BLOCK else row.shape[1]


# ------------------------------------------------------------------ CPU tests
def test_table_is_rank_deficient_at_the_edges():
    """The table is what its docstring says: the edges in n and m, dependent
    rows and a zero column everywhere they fit, one graph with fewer non-pivot
    columns than the search order, inconsistent shots in the checker subset."""
    for rs, widths in ((2, [4, 6, 9, 16]), (4, [6, 9, 12, 16]), (6, [14, 16])):
        for prev, w in zip([0] + widths, widths):
            ns = sorted(r.n for r in TABLE if r.shape == (rs, w))
            assert len(ns) == 2 and ns[1] == 64 * w - 1, (rs, w, ns)
            assert ns[0] == 64 * prev or (prev == 0 and ns[0] < 64 * w - 1), (rs, w, ns)
    assert all(r.n >= 896 for r in TABLE if r.shape == (6, 16))
    assert {r.m for r in TABLE if r.shape in OSD_SHAPES} == {1, 64, 65, 128, 129, 256, 257, 384}
    assert any(r.m > r.n for r in TABLE if r.shape in OSD_SHAPES) and any(r.m > r.n for r in TABLE if r.shape == BLOCK)
    short_of_order = 0
    for row in TABLE:
        H = graph(row.name)
        rank, _ = rank_and_left_null(row.name)
        wts = np.diff(H.indptr)
        assert wts.max() <= 8 and sorted(set(wts) - {0})[0] >= 2
        if row.n > 2:
            assert (np.diff(H.tocsc().indptr) == 0).any(), row.name  # an all-zero column
            assert rank < row.n
        if row.m >= 8:
            assert (wts == 0).sum() == 1, row.name  # the all-zero row
            assert rank <= min(row.m - 3, row.n - 1), row.name  # duplicate, XOR of two, zero row, zero column
            x = inputs(row.name, "f64")
            assert not x["in_image"][[b for b in CHECK_SHOTS if _arbitrary(b)]].all(), row.name
        if row.m == 3:
            assert rank == 2
        short_of_order += 0 < row.n - rank < 7
    assert short_of_order >= 1
    assert len(CHECK_SHOTS) == 16 and all(sum(_family(b) == f for b in CHECK_SHOTS) == 4 for f in range(4))


def test_table_reaches_every_kernel():
    """qd_osd_kernel_info (the selection launch_osd itself uses) on host-only
    graphs: every row selects the kernel it names, the rows reach all ten
    register shapes and the workgroup kernel, no launch asks for more than
    160 KiB of LDS, and the graph past the limit has no device kernel."""
    reached = set()
    for row in SUPPORTED:
        info, supported = _kernel_info_on_host(row.name)
        assert supported and info is not None, row.name
        rs, w, lds = info
        assert (rs, w) == (row.shape[0], _expected_w(row)), (row.name, info)
        assert 0 < lds <= LDS_LIMIT, (row.name, lds)
        reached.add((rs, w) if rs else BLOCK)
    assert reached == set(OSD_SHAPES) | {BLOCK}
    for row in TABLE:
        if row.shape == (6, 16):
            assert _kernel_info_on_host(row.name)[0][2] > 64 * 1024  # needs the raised dynamic-LDS limit
    assert _kernel_info_on_host("blk_near_limit")[0][2] > LDS_LIMIT - 1024
    info, supported = _kernel_info_on_host(PAST_LIMIT.name)
    assert info is None and not supported


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("row", SUPPORTED, ids=lambda r: r.name)
def test_host_osd_matches_numpy_checker(row, precision):
    """The host stage (qdec_osd.cpp) on the same graphs and inputs: byte-equal
    to the numpy checker on CHECK_SHOTS for every method; H osdw = s wherever s
    is in the image; |osdw| <= |osd0|."""
    x = inputs(row.name, precision)
    H = graph(row.name)
    for mi, (method, order) in enumerate(METHODS):
        o0, ow = host_ref(row.name, precision, method, order)
        for b in CHECK_SHOTS:
            r0, rw = checker_ref(row.name, precision, b)[mi]
            assert np.array_equal(o0[b], r0), (method, order, b, FAMILIES[_family(b)])
            assert np.array_equal(ow[b], rw), (method, order, b, FAMILIES[_family(b)])
        _check_solutions(H, x, o0, ow, np.arange(B), (method, order))


def _check_solutions(H, x, o0, ow, shots, what):
    img = shots[x["in_image"][shots]]
    assert img.size > 0
    assert np.array_equal((H @ ow[img].T.astype(np.int64)).T % 2, x["syn"][img]), what
    assert np.array_equal((H @ o0[img].T.astype(np.int64)).T % 2, x["syn"][img]), what
    assert (ow[shots].sum(axis=1, dtype=np.int64) <= o0[shots].sum(axis=1, dtype=np.int64)).all(), what
    if what[0] == "osd0" or what[1] == 0 and what[0] == "osd_e":
        assert np.array_equal(ow[shots], o0[shots]), what


# ------------------------------------------------------------------ GPU tests
def _device_run(dec, x, method, order, sl=slice(None), status=True):
    """osd_device on the shots of slice `sl`; returns (osd0, osdw) with the fill
    0xAA wherever the device wrote nothing."""
    import torch
    dev = torch.device("cuda", 0)
    syn = torch.from_numpy(x["syn"][sl].copy()).to(dev)
    llr = torch.from_numpy(x["llr"][sl].copy()).to(dev)
    st = None
    if status is True:
        st = torch.from_numpy(x["status"][sl].copy()).to(dev)
    elif status is not None:
        st = torch.from_numpy(status).to(dev)
    nb, n = llr.shape
    o0 = torch.full((nb, n), 0xAA, dtype=torch.uint8, device=dev)
    ow = torch.full((nb, n), 0xAA, dtype=torch.uint8, device=dev)
    dec.osd_device(nb, llr=llr, method=method, order=order, syn=syn, status=st, osd0=o0, osdw=ow)
    torch.cuda.synchronize()
    if st is not None:
        assert np.array_equal(st.cpu().numpy(), x["status"][sl] if status is True else status)  # read only
    return o0.cpu().numpy(), ow.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("row", SUPPORTED, ids=lambda r: r.name)
def test_device_osd_every_shape(gpu_available, row, precision):
    """osd_device on every table row, every method: unconverged shots byte-equal
    to the host stage, CHECK_SHOTS byte-equal to the numpy checker, converged
    rows untouched, H osdw = s in the image, |osdw| <= |osd0|; then one B = 1
    call and one all-converged batch."""
    from exp_ldpc_amd.decoder import Decoder
    H = graph(row.name)
    x = inputs(row.name, precision)
    dec = Decoder(H, 0.05, method="ms", precision=precision, max_iter=1)
    assert dec.osd_device_supported
    assert dec.osd_kernel_info()[:2] == (row.shape[0], _expected_w(row))
    for mi, (method, order) in enumerate(METHODS):
        o0, ow = _device_run(dec, x, method, order)
        assert (o0[GOOD] == 0xAA).all() and (ow[GOOD] == 0xAA).all(), (method, order)
        h0, hw = host_ref(row.name, precision, method, order)
        assert np.array_equal(o0[BAD], h0[BAD]), (method, order)
        assert np.array_equal(ow[BAD], hw[BAD]), (method, order)
        for b in CHECK_SHOTS:
            r0, rw = checker_ref(row.name, precision, b)[mi]
            assert np.array_equal(o0[b], r0), (method, order, b, FAMILIES[_family(b)])
            assert np.array_equal(ow[b], rw), (method, order, b, FAMILIES[_family(b)])
        _check_solutions(H, x, o0, ow, BAD, (method, order))
    # B = 1: shot 4 (arbitrary syndrome, all-equal LLRs), no status vector
    o0, ow = _device_run(dec, x, "osd_cs", 7, slice(4, 5), status=None)
    r0, rw = checker_ref(row.name, precision, 4)[METHODS.index(("osd_cs", 7))]
    assert np.array_equal(o0[0], r0) and np.array_equal(ow[0], rw)
    # every shot converged: nothing is written
    o0, ow = _device_run(dec, x, "osd_cs", 7, status=np.where(np.arange(B) % 2, 1, 3).astype(np.uint8))
    assert (o0 == 0xAA).all() and (ow == 0xAA).all()
    dec.close()


@pytest.mark.gpu
def test_device_osd_refuses_the_graph_past_the_lds_limit(gpu_available):
    import torch
    from exp_ldpc_amd import _abi
    from exp_ldpc_amd.decoder import Decoder
    H = graph(PAST_LIMIT.name)
    dec = Decoder(H, 0.05, method="ms", precision="f64", max_iter=1)
    assert not dec.osd_device_supported and dec.osd_kernel_info() is None
    dev = torch.device("cuda", 0)
    llr = torch.zeros((2, H.shape[1]), dtype=torch.float64, device=dev)
    syn = torch.zeros((2, H.shape[0]), dtype=torch.uint8, device=dev)
    ow = torch.full((2, H.shape[1]), 0xAA, dtype=torch.uint8, device=dev)
    with pytest.raises(_abi.QdecError) as err:
        dec.osd_device(2, llr=llr, method="osd_cs", order=7, syn=syn, osdw=ow)
    assert err.value.rc == -85
    torch.cuda.synchronize()
    assert (ow.cpu().numpy() == 0xAA).all()
    dec.close()


# Spacetime-style graphs for the fused outputs: n_data data columns repeated
# fold_blocks times, then m columns more (n_data * fold_blocks < n).
Fused = namedtuple("Fused", "name m n shape n_data fold_blocks k")
FUSED_ROWS = [Fused("fused_wave", 120, 270, (2, 6), 50, 3, 5), Fused("fused_block", 400, 640, BLOCK, 60, 4, 70)]


@pytest.mark.gpu
@pytest.mark.parametrize("row", FUSED_ROWS, ids=lambda r: r.name)
def test_device_osd_fused_fold_and_failure_flag(gpu_available, row):
    """corr = base ^ fold(osdw) (fold(x)[q] = xor_t x[t * n_data + q]) and fail =
    any_r Lz[r] . (readout ^ corr), in numpy from those definitions; once with
    the syndrome composed on the device (syn_flags = 3: H[:, :n_data] (base ^
    readout)) and once with the same syndrome passed explicitly."""
    import torch
    from exp_ldpc_amd.decoder import Decoder
    H = graph(row.name)
    m, n = H.shape
    nd, fb = row.n_data, row.fold_blocks
    rng = np.random.default_rng(zlib.crc32((row.name + "/fused").encode()))
    Lz = (rng.random((row.k, nd)) < 0.2).astype(np.uint8)
    Lz[[r for r in range(row.k) if r not in (1, row.k - 1)]] = 0  # two logicals with support: some shots pass
    base = (rng.random((B, nd)) < 0.1).astype(np.uint8)
    readout = (rng.random((B, nd)) < 0.3).astype(np.uint8)
    syn = ((H[:, :nd] @ (base ^ readout).T.astype(np.int64)).T % 2).astype(np.uint8)
    x = inputs(row.name, "f64")
    dec = Decoder(H, 0.05, method="ms", precision="f64", max_iter=1, logicals=Lz, n_data=nd, fold_blocks=fb)
    assert dec.osd_kernel_info()[:2] == (row.shape[0], _expected_w(row))
    from exp_ldpc_amd.osd import OsdSolver
    _, hw = OsdSolver(H, "osd_cs", 7).solve(syn, x["ref_llr"])
    fold = np.zeros((B, nd), np.uint8)
    for t in range(fb):
        fold ^= hw[:, t * nd:(t + 1) * nd]
    corr_ref = base ^ fold
    fail_ref = ((Lz.astype(np.int64) @ (readout ^ corr_ref).T.astype(np.int64)) % 2).any(axis=0).astype(np.uint8)
    assert 0 < fail_ref[BAD].sum() < BAD.size
    dev = torch.device("cuda", 0)
    up = {k: torch.from_numpy(np.array(v, order="C")).to(dev)
          for k, v in (("syn", syn), ("llr", x["llr"]), ("status", x["status"]), ("base", base), ("readout", readout))}
    for flags, syn_arg in ((3, None), (0, up["syn"])):
        ow = torch.full((B, n), 0xAA, dtype=torch.uint8, device=dev)
        corr = torch.full((B, nd), 0xAA, dtype=torch.uint8, device=dev)
        fail = torch.full((B,), 0xAA, dtype=torch.uint8, device=dev)
        dec.osd_device(B, llr=up["llr"], method="osd_cs", order=7, syn=syn_arg, syn_flags=flags, status=up["status"],
                       base=up["base"], readout=up["readout"], osdw=ow, corr=corr, fail=fail)
        torch.cuda.synchronize()
        ow, corr, fail = ow.cpu().numpy(), corr.cpu().numpy(), fail.cpu().numpy()
        assert np.array_equal(ow[BAD], hw[BAD]), flags
        assert np.array_equal(corr[BAD], corr_ref[BAD]), flags
        assert np.array_equal(fail[BAD], fail_ref[BAD]), flags
        assert (ow[GOOD] == 0xAA).all() and (corr[GOOD] == 0xAA).all() and (fail[GOOD] == 0xAA).all(), flags
    dec.close()
