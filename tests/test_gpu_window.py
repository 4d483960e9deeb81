"""Sliding-window decoding on the GPU (exp_ldpc_amd/window.py, csrc/qdec_window.hip;
DESIGN 3.6e): window_advance_kernel against the numpy model bit for bit, the
windowed pipelines against the model with the CPU oracle as each window's
decoder, and the one-window case against the full-graph pipeline."""
import numpy as np
import pytest
import scipy.sparse as sp

from exp_ldpc_amd.spacetime import SpacetimeCode
from window_model import advance_model, windowed_model

pytestmark = pytest.mark.gpu

OPTS = {"max_iter": 30, "bp_method": "ms", "ms_scaling_factor": 0, "osd_method": "osd_cs", "osd_order": 2}


def _priors(p):
    """(data, measurement) priors at physical error rate p: they differ, so the column ranges matter."""
    return 2 * p / 3, p


def _tables(rng, n_w, m_total, k_acc):
    """Carry rows with empty rows among them and one row reading the last
    column; accumulator rows likewise."""
    rows = np.sort(rng.choice(m_total, size=min(m_total, 9), replace=False)).astype(np.int32)
    def csr(nrows):
        lists = [rng.choice(n_w, size=min(n_w, int(rng.integers(0, 6))), replace=False) for _ in range(nrows)]
        lists[0] = np.array([], np.int64)                    # an empty row
        lists[-1] = np.array([n_w - 1, 0][:max(1, min(n_w, 2))])  # the last column
        ptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int32)
        return ptr, np.concatenate(lists).astype(np.int32)
    cptr, ccols = csr(rows.size)
    aptr, acols = csr(k_acc)
    return rows, cptr, ccols, aptr, acols


@pytest.mark.parametrize("B", [1, 5, 65])
@pytest.mark.parametrize("n_w", [1, 63, 64, 65, 1332])
def test_advance_kernel_against_model(gpu_available, n_w, B):
    import torch
    from exp_ldpc_amd.window import WindowAdvance
    rng = np.random.default_rng(1000 * n_w + B)
    m_total, k_acc, row0, m_next = 41, 7, 11, 30
    rows, cptr, ccols, aptr, acols = _tables(rng, n_w, m_total, k_acc)
    assert (np.diff(cptr) == 0).any() and (ccols == n_w - 1).any()
    x = rng.integers(0, 256, size=(B, n_w), dtype=np.uint8)  # any byte: bit 0 counts
    syn0 = rng.integers(0, 2, size=(B, m_total), dtype=np.uint8)
    acc0 = rng.integers(0, 2, size=(B, k_acc), dtype=np.uint8)
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(a.copy()).to(dev)  # noqa: E731
    empty, zero = np.zeros(0, np.int32), np.zeros(1, np.int32)

    def run(wa, x_h, with_next=True, with_acc=True):
        syn_d, acc_d = t(syn0), t(acc0)
        nxt_d = torch.full((B, m_next), 0xAA, dtype=torch.uint8, device=dev) if with_next else None
        wa.advance(B, None if x_h is None else t(x_h), syn_d, acc_d if with_acc else None, nxt_d)
        torch.cuda.synchronize()
        return syn_d.cpu().numpy(), acc_d.cpu().numpy(), None if nxt_d is None else nxt_d.cpu().numpy()

    wa = WindowAdvance(n_w, m_total, rows, cptr, ccols, aptr, acols, row0, m_next, device=0)
    syn_m, acc_m = syn0.copy(), acc0.copy()
    nxt_m = advance_model(x, syn_m, acc_m, rows, cptr, ccols, aptr, acols, row0, m_next)
    got = run(wa, x)
    assert np.array_equal(got[0], syn_m) and np.array_equal(got[1], acc_m) and np.array_equal(got[2], nxt_m)
    untouched = np.setdiff1d(np.arange(m_total), rows)
    assert np.array_equal(got[0][:, untouched], syn0[:, untouched])  # only the listed rows are written
    if B == 65:  # and over 65 shots both tables did something
        assert (syn_m != syn0).any() and (acc_m != acc0).any()
    # the grid does not matter: two workgroups over the shots, then one
    for blocks in (2, 1, 0):
        wa.set_blocks(blocks)
        again = run(wa, x)
        assert all(np.array_equal(p, q) for p, q in zip(got, again)), blocks
    # x = NULL: a pure copy of the next window's rows, nothing else is written
    s, a, nx = run(wa, None)
    assert np.array_equal(s, syn0) and np.array_equal(a, acc0) and np.array_equal(nx, syn0[:, row0:row0 + m_next])
    # syn_next = NULL, and acc_out = NULL
    s, a, nx = run(wa, x, with_next=False)
    assert np.array_equal(s, syn_m) and np.array_equal(a, acc_m) and nx is None
    s, a, nx = run(wa, x, with_acc=False)
    assert np.array_equal(s, syn_m) and np.array_equal(a, acc0) and np.array_equal(nx, nxt_m)
    wa.close()
    # empty tables: x is read and nothing changes
    wa = WindowAdvance(n_w, m_total, empty, zero, empty, zero, empty, 0, m_total, device=0)
    syn_d = t(syn0)
    nxt_d = torch.full((B, m_total), 0xAA, dtype=torch.uint8, device=dev)
    wa.advance(B, t(x), syn_d, None, nxt_d)
    torch.cuda.synchronize()
    assert np.array_equal(syn_d.cpu().numpy(), syn0) and np.array_equal(nxt_d.cpu().numpy(), syn0)
    wa.close()


def _model_pipeline(oracle_lib, code, R, W, Cm, p, syn, rd, precision, osd):
    """corr, fail, iters, status of the windowed pipeline by the model: the CPU
    oracle decodes every window (BP, then OSD of order 2 for the shots BP leaves
    open), the final window with the committed fold as its base."""
    HZ = sp.csr_matrix(code.checks.z)
    lz = code.logicals.z
    r, n = HZ.shape
    Hst = sp.csr_matrix(SpacetimeCode(HZ, R).spacetime_check_matrix)
    layer = np.arange((R + 1) * r) // r
    fold = sp.hstack([sp.identity(n, format="csr")] * (R + 1) + [sp.csr_matrix((n, R * r))], format="csr")
    prior = np.concatenate([np.full((R + 1) * n, _priors(p)[0]), np.full(R * r, _priors(p)[1])])
    B = syn.shape[0]
    iters, conv, n_osd = np.zeros(B, np.int64), np.ones(B, np.uint8), [0]

    def bp_osd(Hw, cols, blocks, syn_w, **kw):
        Hw = sp.csr_matrix(Hw)
        ref = oracle_lib.decode(Hw, prior[cols], syn_w, method="ms", precision=precision, max_iter=OPTS["max_iter"],
                                n_data=n, fold_blocks=blocks, want_llr=True, **kw)
        x = ref["x"].copy()
        bad = np.flatnonzero((ref["status"] & 1) == 0)
        if osd and bad.size:
            _, ow = oracle_lib.osd(Hw, syn_w[bad], ref["llr"][bad], "osd_cs", OPTS["osd_order"])
            x[bad] = ow
            n_osd[0] += bad.size
        return ref, x, bad

    def decode(k, span, Hw, cols, syn_w):
        nonlocal conv
        ref, x, _ = bp_osd(Hw, cols, span[1], syn_w)
        iters[:] += ref["iters"]
        conv &= ref["status"] & 1
        return x
    out = windowed_model(Hst, layer, W, Cm, fold, syn, decode, stop_before_final=True)
    span, Hw, cols, syn_f = out["final"]
    base = out["acc"]
    ref, x, bad = bp_osd(Hw, cols, span[1], syn_f, lz=lz, base=base, readout=rd)
    corr, fail = ref["corr"].copy(), ref["fail"].copy()
    if osd and bad.size:
        corr[bad] = base[bad] ^ np.bitwise_xor.reduce(x[bad][:, :span[1] * n].reshape(bad.size, span[1], n), axis=1)
        L = np.asarray(lz.toarray() if sp.issparse(lz) else lz).astype(np.int64) % 2
        fail[bad] = (((rd[bad] ^ corr[bad]).astype(np.int64) @ L.T) % 2).any(axis=1)
    status = (conv & ref["status"] & 1) | (ref["status"] & 2)
    return dict(corr=corr, fail=fail, iters=iters + ref["iters"], status=status, n_osd=n_osd[0],
                windows=len(out["windows"]) + 1)


@pytest.fixture(scope="module")
def shots(oracle_lib, code225):
    """65 sampled shots per (rounds, p), made once."""
    HZ = sp.csr_matrix(code225.checks.z)
    return {(R, p): oracle_lib.sample_storage(HZ, R, p, p, seed=77, stream=R, shot0=0, B=65)
            for R, p in ((5, 0.02), (6, 0.02), (6, 0.004))}


@pytest.mark.parametrize("mode", ["bp", "bposd"])
@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("R, W, Cm, p", [(6, 3, 2, 0.02), (6, 3, 1, 0.02), (5, 2, 2, 0.02), (6, 3, 2, 0.004)])
def test_windowed_pipeline_against_model(gpu_available, oracle_lib, code225, shots, R, W, Cm, p, precision, mode):
    """p = 0.02 lies above this code's threshold over 6 rounds, so BP leaves
    nearly every shot open somewhere; the case at p = 0.004 has shots that
    converge in every window beside shots that do not."""
    import torch
    from exp_ldpc_amd.experiment import BatchPipeline
    syn, rd = shots[(R, p)]
    want = _model_pipeline(oracle_lib, code225, R, W, Cm, p, syn, rd, precision, osd=mode == "bposd")
    assert want["windows"] == {(6, 3, 2): 3, (6, 3, 1): 5, (5, 2, 2): 3}[(R, W, Cm)]
    if mode == "bposd":
        assert want["n_osd"] > 0  # OSD runs on some shots
    if p < 0.01:
        assert 0 < int((want["status"] & 1).sum()) < 65
    pipe = BatchPipeline(code225, R, mode, OPTS, _priors(p), precision=precision, window=W, commit=Cm)
    dev = torch.device("cuda", 0)
    syn_d, rd_d = torch.from_numpy(syn).to(dev), torch.from_numpy(rd).to(dev)
    res = pipe.run(syn_d, rd_d, want_corrections=True, want_detail=True)
    assert np.array_equal(syn_d.cpu().numpy(), syn)  # the pipeline works on its own copy
    assert np.array_equal(res.corrections, want["corr"])
    assert np.array_equal(res.fail, want["fail"].astype(bool))
    assert np.array_equal(res.detail["iters"], want["iters"])
    assert np.array_equal(res.detail["status"], want["status"])
    assert res.iters_sum == int(want["iters"].sum()) and res.bp_converged == int((want["status"] & 1).sum())
    for d in pipe.decoders() + [pipe.sampler_graph]:
        d.close()


def test_windowed_bposd_with_the_host_osd_stage(gpu_available, oracle_lib, code225, shots):
    """osd_rows="host": every window's OSD runs in the host stage (the path of
    graphs no device kernel holds); the same results as the model."""
    import torch
    from exp_ldpc_amd.experiment import BatchPipeline
    R, W, Cm, p = 5, 2, 2, 0.02
    syn, rd = shots[(R, p)]
    want = _model_pipeline(oracle_lib, code225, R, W, Cm, p, syn, rd, "f64", osd=True)
    pipe = BatchPipeline(code225, R, "bposd", OPTS, _priors(p), precision="f64", window=W, commit=Cm, osd_rows="host")
    dev = torch.device("cuda", 0)
    res = pipe.run(torch.from_numpy(syn).to(dev), torch.from_numpy(rd).to(dev), want_corrections=True,
                   want_detail=True)
    assert np.array_equal(res.corrections, want["corr"]) and np.array_equal(res.fail, want["fail"].astype(bool))
    assert np.array_equal(res.detail["iters"], want["iters"]) and np.array_equal(res.detail["status"], want["status"])
    for d in pipe.decoders() + [pipe.sampler_graph]:
        d.close()


@pytest.mark.parametrize("mode", ["bp", "bposd"])
def test_one_window_equals_the_full_graph(gpu_available, oracle_lib, code225, mode):
    import torch
    from exp_ldpc_amd.experiment import BatchPipeline
    R = 2
    syn, rd = oracle_lib.sample_storage(sp.csr_matrix(code225.checks.z), R, 0.02, 0.02, seed=78, stream=0, shot0=0, B=65)
    dev = torch.device("cuda", 0)
    out = []
    for window in (None, R + 1):
        pipe = BatchPipeline(code225, R, mode, OPTS, _priors(0.02), precision="f64", window=window)
        res = pipe.run(torch.from_numpy(syn).to(dev), torch.from_numpy(rd).to(dev), want_corrections=True,
                       want_detail=True)
        out.append(res)
        for d in pipe.decoders() + [pipe.sampler_graph]:
            d.close()
    full, one = out
    assert np.array_equal(full.fail, one.fail) and np.array_equal(full.corrections, one.corrections)
    assert (full.bp_converged, full.iters_sum, full.ssf_steps_sum) == (one.bp_converged, one.iters_sum, one.ssf_steps_sum)
    assert np.array_equal(full.detail["iters"], one.detail["iters"])
    assert np.array_equal(full.detail["status"], one.detail["status"])


def test_windowed_decoder_generic_graph(gpu_available, oracle_lib):
    """WindowedDecoder on a hand-made graph whose columns span 3 layers (W = 3,
    C = 1: the carry reaches the window after next), with an accumulator that
    is no fold: x_full, acc_out, iters and status against the model, BP and
    BP + OSD."""
    import torch
    from exp_ldpc_amd.window import WindowedDecoder, WindowPlan
    layer = np.repeat(np.arange(5), 2)
    cols = []
    for t in range(5):
        for rows in ((2 * t, 2 * t + 2, 2 * t + 5), (2 * t + 1, 2 * t + 4), (2 * t, 2 * t + 1), (2 * t + 1, 2 * t + 3, 2 * t + 4)):
            cols.append([g for g in rows if g < 10])
    H = np.zeros((10, len(cols)), np.uint8)
    for j, rows in enumerate(cols):
        H[rows, j] = 1
    rng = np.random.default_rng(9)
    acc = (rng.random((3, H.shape[1])) < 0.4).astype(np.uint8)
    prior = rng.uniform(0.05, 0.15, H.shape[1])
    e = (rng.random((65, H.shape[1])) < 0.1).astype(np.uint8)
    syn = (e.astype(np.int64) @ H.T.astype(np.int64) % 2).astype(np.uint8)
    plan = WindowPlan(H, layer, 3, 1, acc=acc)
    dev = torch.device("cuda", 0)
    for osd in (None, dict(method="osd_cs", order=2, rows="auto")):
        iters, conv, last = np.zeros(65, np.int64), np.ones(65, np.uint8), {}

        def decode(k, span, Hw, cols_w, syn_w):
            ref = oracle_lib.decode(sp.csr_matrix(Hw), prior[cols_w], syn_w, method="ms", precision="f64", max_iter=20,
                                    want_llr=True)
            x = ref["x"].copy()
            bad = np.flatnonzero((ref["status"] & 1) == 0)
            if osd and bad.size:
                _, ow = oracle_lib.osd(sp.csr_matrix(Hw), syn_w[bad], ref["llr"][bad], "osd_cs", 2)
                x[bad] = ow
            iters[:] += ref["iters"]
            conv[:] &= ref["status"] & 1
            last["status"] = ref["status"]
            return x
        want = windowed_model(H, layer, 3, 1, acc, syn, decode)
        wd = WindowedDecoder(plan, prior, method="ms", precision="f64", max_iter=20, device=0)
        syn_d = torch.from_numpy(syn.copy()).to(dev)
        acc_d = torch.zeros((65, 3), dtype=torch.uint8, device=dev)
        x_d = torch.zeros((65, H.shape[1]), dtype=torch.uint8, device=dev)
        it_d = torch.zeros(65, dtype=torch.int32, device=dev)
        st_d = torch.zeros(65, dtype=torch.uint8, device=dev)
        wd.decode_device(65, syn_d, acc_d, x_full=x_d, iters=it_d, status=st_d, osd=osd)
        torch.cuda.synchronize()
        assert np.array_equal(x_d.cpu().numpy(), want["x"]) and np.array_equal(acc_d.cpu().numpy(), want["acc"])
        assert np.array_equal(syn_d.cpu().numpy(), want["syn"])
        assert np.array_equal(it_d.cpu().numpy(), iters)
        assert np.array_equal(st_d.cpu().numpy(), (conv & 1) | (last["status"] & 2))
        wd.close()
