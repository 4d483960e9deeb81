"""osd_hbm_kernel (csrc/qdec_osd_hbm.hip): the OSD stage with its rows in a slot of
device memory, against the host stage on every shot, the numpy checker on a
subset, and the on-chip kernels where one holds the graph.

Graphs, all rank-deficient (test_osd_shapes.TABLE), each with what it can show:
  w2x4_lo_trivial  1 x 2       the trivial case
  w2x16_hi         65 x 1023   syndrome bit in bit 63 of the last word
  blk_three_rows   3 x 1024    syndrome bit alone in a word
  blk_m_gt_n       385 x 100   the loop ends by k = n with rank < m
  blk_near_limit   187 x 4095  just under the LDS limit
  blk_past_limit   188 x 4095  rows="auto": the graph qd_osd_batch_device refuses (-85)
  wide             3 x 65,600  32-bit indices, a 131,072-key sort
Inputs as in test_osd_shapes: B = 48, four LLR families (ties, +-0, +-inf,
denormals), both syndrome kinds, every third shot marked converged; all eight
METHODS; f32 and f64 llr.

The numpy checker runs on CHECK_SHOTS.  On the wide graph it takes 1.3 s per
shot for the eight methods (one CPU core; 0.38 s for three of them), so there it
checks one shot per LLR family and osd0, osd_e 10 and osd_cs 7: about 3 s for
both precisions.  The host stage stays the every-shot reference everywhere.
"""
import contextlib
import functools
import zlib

import numpy as np
import pytest

from test_osd_hbm_host import slot_bytes, wide_graph
from test_osd_shapes import B, BAD, CHECK_SHOTS, FUSED_ROWS, GOOD, METHODS, TABLE, graph, host_ref, inputs

pytestmark = pytest.mark.gpu

HBM_ROWS = ["w2x4_lo_trivial", "w2x16_hi", "blk_three_rows", "blk_m_gt_n", "blk_near_limit"]
PAST = "blk_past_limit"
_SPECIALS = np.array([np.inf, -np.inf, np.inf, 5e-324, -5e-324, 1e-310, 1e-40, -1e-40, 2.2250738585072014e-308,
                      -np.inf])
WIDE_CHECK = [next(b for b in CHECK_SHOTS if b % 4 == f and (b // 4) % 2 == (f % 2)) for f in range(4)]  # one per family
WIDE_CHECK_METHODS = [("osd0", 0), ("osd_e", 10), ("osd_cs", 7)]


@functools.lru_cache(maxsize=None)
def wide_inputs(precision):
    """test_osd_shapes.inputs restated for the wide graph (no left null space is
    needed: only H e = s on the shots that take it is checked)."""
    H = wide_graph()
    m, n = H.shape
    rng = np.random.default_rng(zlib.crc32(b"wide_3x65600/inputs"))
    e = (rng.random((B, n)) < 0.0005).astype(np.int64)
    syn = ((H @ e.T).T % 2).astype(np.uint8)
    llr = np.empty((B, n), np.float64)
    status = np.zeros(B, np.uint8)
    for b in range(B):
        if (b // 4) % 2 == 1:
            syn[b] = rng.integers(0, 2, size=m)
        normals = rng.normal(1.0, 2.0, n)
        five = rng.choice([-1.5, -0.0, 0.0, 0.5, 2.0], n)
        where = rng.random(n) < 0.15
        special = rng.choice(_SPECIALS, n)
        llr[b] = (np.full(n, 0.75), five, normals, np.where(where, special, normals))[b % 4]
        status[b] = (1, 3)[b % 2] if b % 3 == 2 else (0, 2)[b % 2]
    if precision == "f32":
        llr = llr.astype(np.float32)
    return {"syn": np.ascontiguousarray(syn), "llr": np.ascontiguousarray(llr), "ref_llr": llr.astype(np.float64),
            "status": status}


@functools.lru_cache(maxsize=None)
def wide_host_ref(precision, method, order):
    from exp_ldpc_amd.osd import OsdSolver
    x = wide_inputs(precision)
    return OsdSolver(wide_graph(), method, order).solve(x["syn"], x["ref_llr"])


def _run(dec, x, method, order, rows, sl=slice(None), stream=None):
    """osd_device on the shots of `sl`; (osd0, osdw) with the fill 0xAA wherever
    the device wrote nothing."""
    import torch
    dev = torch.device("cuda", 0)
    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        syn = torch.from_numpy(x["syn"][sl].copy()).to(dev)
        llr = torch.from_numpy(x["llr"][sl].copy()).to(dev)
        st = torch.from_numpy(x["status"][sl].copy()).to(dev)
        nb, n = llr.shape
        o0 = torch.full((nb, n), 0xAA, dtype=torch.uint8, device=dev)
        ow = torch.full((nb, n), 0xAA, dtype=torch.uint8, device=dev)
        dec.osd_device(nb, llr=llr, method=method, order=order, syn=syn, status=st, osd0=o0, osdw=ow, rows=rows)
    return (o0, ow), (syn, llr, st)


def _host(pair):
    import torch
    torch.cuda.synchronize()
    return pair[0].cpu().numpy(), pair[1].cpu().numpy()


def _check_graph(H, x, ref, rows, precision, check_shots, check_methods, checker, onchip):
    from exp_ldpc_amd.decoder import Decoder
    dec = Decoder(H, 0.05, method="ms", precision=precision, max_iter=1)
    m, n = H.shape
    info = dec.osd_kernel_info(rows=rows)
    assert info == (2, 0, (n + 1 + 63) // 64, slot_bytes(m, n))
    assert dec.osd_device_supported == onchip
    for mi, (method, order) in enumerate(METHODS):
        o0, ow = _host(_run(dec, x, method, order, rows)[0])
        assert (o0[GOOD] == 0xAA).all() and (ow[GOOD] == 0xAA).all(), (method, order)
        h0, hw = ref(method, order)
        assert np.array_equal(o0[BAD], h0[BAD]), (method, order)
        assert np.array_equal(ow[BAD], hw[BAD]), (method, order)
        assert (ow[BAD].sum(axis=1, dtype=np.int64) <= o0[BAD].sum(axis=1, dtype=np.int64)).all(), (method, order)
        if onchip:
            c0, cw = _host(_run(dec, x, method, order, "onchip")[0])
            assert np.array_equal(c0, o0) and np.array_equal(cw, ow), (method, order)
        if (method, order) in check_methods:
            for b in check_shots:
                r0, rw = checker(b, (method, order))
                assert np.array_equal(o0[b], r0) and np.array_equal(ow[b], rw), (method, order, b)
    per_slot, slots, held = dec.osd_hbm_info()
    assert per_slot == slot_bytes(m, n) and 1 <= slots <= B and held >= slots * per_slot
    dec.close()


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("name", HBM_ROWS + [PAST])
def test_hbm_kernel_on_the_table_graphs(gpu_available, name, precision):
    """Forced rows="hbm" (the graph past the LDS limit: rows="auto", which must
    pick the HBM kernel): every unconverged shot equals the host stage, the
    converged rows keep their fill, the on-chip kernel agrees where there is
    one, CHECK_SHOTS equal the numpy checker."""
    from test_osd_shapes import checker_ref
    row = next(r for r in TABLE if r.name == name)
    H = graph(name)
    x = inputs(name, precision)
    rows = "auto" if name == PAST else "hbm"
    _check_graph(H, x, lambda method, order: host_ref(name, precision, method, order), rows, precision, CHECK_SHOTS,
                 METHODS, lambda b, mo: checker_ref(name, precision, b)[METHODS.index(mo)], row.shape is not None)


_WIDE_CHECKER = {}


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_hbm_kernel_on_the_wide_graph(gpu_available, precision):
    """3 x 65,600: column indices past 16 bits, 131,072 sort keys, 1026 words
    per row; rows="auto" picks the HBM kernel."""
    from oracle.osd_py import osd_decode_methods
    H = wide_graph()
    x = wide_inputs(precision)

    def checker(b, mo):
        key = (b, x["ref_llr"][b].tobytes())
        if key not in _WIDE_CHECKER:
            _WIDE_CHECKER[key] = osd_decode_methods(H, x["syn"][b], x["ref_llr"][b], WIDE_CHECK_METHODS)
        return _WIDE_CHECKER[key][WIDE_CHECK_METHODS.index(mo)]

    assert len(WIDE_CHECK) == 4 and sorted(b % 4 for b in WIDE_CHECK) == [0, 1, 2, 3]
    _check_graph(H, x, lambda method, order: wide_host_ref(precision, method, order), "auto", precision, WIDE_CHECK,
                 WIDE_CHECK_METHODS, checker, False)


def test_slot_count_and_streams_do_not_change_the_bytes(gpu_available):
    """Slots forced to 1 and 3 give the default's bytes; a 20 + 28 split over two
    streams on one handle (chained through the handle's event) equals one call."""
    import torch
    from exp_ldpc_amd.decoder import Decoder
    H = graph(PAST)
    x = inputs(PAST, "f64")
    dec = Decoder(H, 0.05, method="ms", precision="f64", max_iter=1)
    base = _host(_run(dec, x, "osd_cs", 7, "hbm")[0])
    assert dec.osd_hbm_info()[1] == B  # the default is capped at the shots of the batch
    for slots in (1, 3):
        dec.set_osd_slots(slots)
        got = _host(_run(dec, x, "osd_cs", 7, "hbm")[0])
        assert dec.osd_hbm_info()[1] == slots
        assert np.array_equal(got[0], base[0]) and np.array_equal(got[1], base[1]), slots
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    a, keep_a = _run(dec, x, "osd_cs", 7, "hbm", slice(0, 20), s1)
    b, keep_b = _run(dec, x, "osd_cs", 7, "hbm", slice(20, 48), s2)
    a, b = _host(a), _host(b)
    assert np.array_equal(np.concatenate([a[0], b[0]]), base[0])
    assert np.array_equal(np.concatenate([a[1], b[1]]), base[1])
    dec.set_osd_slots(0)
    with pytest.raises(Exception) as err:
        dec.set_osd_slots(-1)
    assert getattr(err.value, "rc", None) == -47
    dec.close()


def test_hbm_kernel_fused_fold_and_failure_flag(gpu_available):
    """corr = base ^ fold(osdw) and fail = any_r Lz[r] . (readout ^ corr) from the
    HBM kernel, in numpy from those definitions, on the fused_block graph of
    test_osd_shapes (n_data = 60 < n = 640, four fold blocks, 70 logicals), for
    syn_flags 0 .. 3: the syndrome passed (0), composed with H[:, :n_data] base
    (1), readout (2) or both and no syn (3)."""
    import torch
    from exp_ldpc_amd.decoder import Decoder
    from exp_ldpc_amd.osd import OsdSolver
    row = next(r for r in FUSED_ROWS if r.name == "fused_block")
    H = graph(row.name)
    m, n = H.shape
    nd, fb = row.n_data, row.fold_blocks
    rng = np.random.default_rng(zlib.crc32(b"fused_block/hbm"))
    Lz = (rng.random((row.k, nd)) < 0.2).astype(np.uint8)
    Lz[[r for r in range(row.k) if r not in (1, row.k - 1)]] = 0
    base = (rng.random((B, nd)) < 0.1).astype(np.uint8)
    readout = (rng.random((B, nd)) < 0.3).astype(np.uint8)
    extra = rng.integers(0, 2, size=(B, m)).astype(np.uint8)
    Hd = H[:, :nd]
    x = inputs(row.name, "f64")
    dec = Decoder(H, 0.05, method="ms", precision="f64", max_iter=1, logicals=Lz, n_data=nd, fold_blocks=fb)
    assert dec.osd_kernel_info(rows="hbm")[0] == 2
    dev = torch.device("cuda", 0)
    up = {k: torch.from_numpy(np.array(v, order="C")).to(dev)
          for k, v in (("llr", x["llr"]), ("status", x["status"]), ("base", base), ("readout", readout))}
    for flags in (0, 1, 2, 3):
        v = (base if flags & 1 else 0 * base) ^ (readout if flags & 2 else 0 * readout)
        composed = ((Hd @ v.T.astype(np.int64)).T % 2).astype(np.uint8)
        syn_arg = None if flags == 3 else extra
        s = composed if flags == 3 else extra ^ composed
        _, hw = OsdSolver(H, "osd_cs", 7).solve(s, x["ref_llr"])
        fold = np.zeros((B, nd), np.uint8)
        for t in range(fb):
            fold ^= hw[:, t * nd:(t + 1) * nd]
        corr_ref = base ^ fold
        fail_ref = ((Lz.astype(np.int64) @ (readout ^ corr_ref).T.astype(np.int64)) % 2).any(axis=0).astype(np.uint8)
        ow = torch.full((B, n), 0xAA, dtype=torch.uint8, device=dev)
        corr = torch.full((B, nd), 0xAA, dtype=torch.uint8, device=dev)
        fail = torch.full((B,), 0xAA, dtype=torch.uint8, device=dev)
        syn_d = None if syn_arg is None else torch.from_numpy(np.ascontiguousarray(syn_arg)).to(dev)
        dec.osd_device(B, llr=up["llr"], method="osd_cs", order=7, syn=syn_d, syn_flags=flags, status=up["status"],
                       base=up["base"], readout=up["readout"], osdw=ow, corr=corr, fail=fail, rows="hbm")
        torch.cuda.synchronize()
        ow, corr, fail = ow.cpu().numpy(), corr.cpu().numpy(), fail.cpu().numpy()
        assert np.array_equal(ow[BAD], hw[BAD]), flags
        assert np.array_equal(corr[BAD], corr_ref[BAD]), flags
        assert np.array_equal(fail[BAD], fail_ref[BAD]), flags
        assert (ow[GOOD] == 0xAA).all() and (corr[GOOD] == 0xAA).all() and (fail[GOOD] == 0xAA).all(), flags
        if flags == 3:
            assert 0 < fail_ref[BAD].sum() < BAD.size
    dec.close()
