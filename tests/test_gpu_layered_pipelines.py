"""The layered schedule behind the public interfaces: ldpc_compat's decoder
objects, BatchPipeline (bp, bposd, a windowed bp, the detector modes) and
DemPipeline.  Each equals "the numpy model (tests/layered_model.py) as the BP
stage, then the existing host OSD (OsdSolver.solve) on the model's llr for the
shots it leaves open", flag for flag.  Min-sum f64, the n = 225 code."""
import numpy as np
import pytest
import scipy.sparse as sp

from layered_model import LayeredModel
from test_circuit_dem_host import lz_on_readout
from test_circuit_host import golden_text
from window_model import windowed_model

pytestmark = pytest.mark.gpu

SEED = 20250221
OPTS = {"max_iter": 20, "bp_method": "ms", "ms_scaling_factor": 0.625, "osd_method": "osd_cs", "osd_order": 7,
        "bp_schedule": "layered"}


def model(H, priors, **kw):
    return LayeredModel(H, priors, np.float64, max_iter=OPTS["max_iter"], ms_scaling=OPTS["ms_scaling_factor"], **kw)


def osd_fix(H, syn, ref):
    """x with the host OSD's solution on the shots the model left open, and their indices."""
    from exp_ldpc_amd.osd import OsdSolver
    x = ref["x"].copy()
    bad = np.flatnonzero((ref["status"] & 1) == 0)
    if bad.size:
        _, ow = OsdSolver(sp.csr_matrix(H), OPTS["osd_method"], OPTS["osd_order"]).solve(
            syn[bad], ref["llr"][bad].astype(np.float64))
        x[bad] = ow
    return x, bad


def flags(L, v):
    Lm = np.asarray(L.toarray() if hasattr(L, "toarray") else L).astype(np.int64) % 2
    return ((v.astype(np.int64) @ Lm.T) % 2).any(axis=1)


def close(pipe):
    for dec in pipe.decoders() + [pipe.sampler_graph]:
        dec.close()


def test_decoder_objects_single_shot(gpu_available, code225):
    from exp_ldpc_amd.ldpc_compat import bp_decoder, bposd_decoder
    hz = sp.csr_matrix(code225.checks.z)
    p, B = 0.03, 12
    e = (np.random.default_rng(9).random((B, 225)) < 0.04).astype(np.uint8)
    syn = (hz.dot(e.T.astype(np.int64)).T & 1).astype(np.uint8)
    ref = LayeredModel(hz, p, np.float64, max_iter=10, ms_scaling=0.625).decode(syn)
    assert 0 < int((ref["status"] == 3).sum()) < B
    kw = dict(error_rate=p, bp_method="ms", ms_scaling_factor=0.625, max_iter=10, schedule="layered")
    bp = bp_decoder(hz, **kw)
    bposd = bposd_decoder(hz, osd_method="osd_cs", osd_order=7, **kw)
    from exp_ldpc_amd.osd import OsdSolver
    solver = OsdSolver(hz, "osd_cs", 7)
    for b in range(B):
        x = bp.decode(syn[b] if b % 2 else e[b])  # a syndrome, or an error vector
        assert x.dtype == np.int64 and np.array_equal(x, ref["x"][b])
        assert bp.iter == ref["iters"][b] and bp.converge == int(ref["status"][b] == 3)
        assert bp.log_prob_ratios.tobytes() == ref["llr"][b].tobytes()
        y = bposd.decode(syn[b])
        assert np.array_equal(bposd.bp_decoding, ref["x"][b]) and bposd.converge == bp.converge
        want = ref["x"][b] if bp.converge else solver.solve(syn[b:b + 1], ref["llr"][b:b + 1])[1][0]
        assert np.array_equal(y, want), b
    # the flooding schedule given explicitly is the default's decode
    dflt = bp_decoder(hz, **{k: v for k, v in kw.items() if k != "schedule"}).decode_batch(syn)
    for name in ("flooding", "parallel"):
        got = bp_decoder(hz, **dict(kw, schedule=name)).decode_batch(syn)
        assert all(got[k].tobytes() == dflt[k].tobytes() for k in ("x", "llr", "iters", "status")), name
    assert not np.array_equal(dflt["iters"], ref["iters"])


@pytest.mark.parametrize("mode", ["bp", "bposd"])
def test_batch_pipeline_at_two_rounds(gpu_available, code225, mode):
    from exp_ldpc_amd.experiment import BatchPipeline
    from exp_ldpc_amd.noise_model import depolarizing_noise
    from exp_ldpc_amd.spacetime import SpacetimeCode
    from exp_ldpc_amd.storage_sim import build_storage_simulation
    p, B, n, R = 0.02, 128, 225, 2
    lz = np.asarray(code225.logicals.z) % 2
    sim = build_storage_simulation(R, depolarizing_noise(p, p), code225)
    pipe = BatchPipeline(code225, R, mode, OPTS, (2 * p / 3, 2 * p / 3))
    assert pipe.st.schedule == "layered"
    syn, rd = sim.sample_device(pipe.sampler_graph, B, seed=21, stream_id=1)
    res = pipe.run(syn, rd, want_corrections=True, want_detail=True)
    Hst = sp.csr_matrix(SpacetimeCode(code225.checks.z, R).spacetime_check_matrix)
    syn_h, rd_h = syn.cpu().numpy(), rd.cpu().numpy()
    ref = model(Hst, np.full(Hst.shape[1], 2 * p / 3), n_data=n, fold_blocks=R + 1, logicals=lz).decode(
        syn_h, None, rd_h)
    x = ref["x"]
    if mode == "bposd":
        x, bad = osd_fix(Hst, syn_h, ref)
        assert bad.size
    corr = np.bitwise_xor.reduce(x[:, :(R + 1) * n].reshape(B, R + 1, n), axis=1)
    assert 0 < int((ref["status"] & 1).sum()) < B
    assert np.array_equal(res.detail["iters"], ref["iters"]) and np.array_equal(res.detail["status"] & 1, ref["status"] & 1)
    assert res.bp_converged == int((ref["status"] & 1).sum()) and res.iters_sum == int(ref["iters"].sum())
    assert np.array_equal(res.corrections, corr) and np.array_equal(res.fail, flags(lz, rd_h ^ corr))
    close(pipe)
    # the flooding schedule given explicitly is the default's run
    runs = []
    for o in ({k: v for k, v in OPTS.items() if k != "bp_schedule"}, dict(OPTS, bp_schedule="flooding")):
        pf = BatchPipeline(code225, R, mode, o, (2 * p / 3, 2 * p / 3))
        assert pf.st.schedule == "flooding"
        runs.append(pf.run(syn, rd, want_corrections=True, want_detail=True))
        close(pf)
    assert np.array_equal(runs[0].corrections, runs[1].corrections) and np.array_equal(runs[0].fail, runs[1].fail)
    assert np.array_equal(runs[0].detail["iters"], runs[1].detail["iters"])
    assert not np.array_equal(runs[0].detail["iters"], ref["iters"])


def test_windowed_bp(gpu_available, code225):
    """bp with window=2 over R = 2: every window's decoder runs the layered kernel."""
    from exp_ldpc_amd.experiment import BatchPipeline
    from exp_ldpc_amd.noise_model import depolarizing_noise
    from exp_ldpc_amd.spacetime import SpacetimeCode
    from exp_ldpc_amd.storage_sim import build_storage_simulation
    p, B, n, R, W, Cm = 0.01, 96, 225, 2, 2, 1
    HZ = sp.csr_matrix(code225.checks.z)
    r = HZ.shape[0]
    lz = np.asarray(code225.logicals.z) % 2
    sim = build_storage_simulation(R, depolarizing_noise(p, p), code225)
    pipe = BatchPipeline(code225, R, "bp", OPTS, (2 * p / 3, 2 * p / 3), window=W, commit=Cm)
    assert all(d.schedule == "layered" for d in pipe.wd.distinct)
    syn, rd = sim.sample_device(pipe.sampler_graph, B, seed=22, stream_id=1)
    res = pipe.run(syn, rd, want_corrections=True, want_detail=True)
    syn_h, rd_h = syn.cpu().numpy(), rd.cpu().numpy()
    Hst = sp.csr_matrix(SpacetimeCode(HZ, R).spacetime_check_matrix)
    layer = np.arange((R + 1) * r) // r
    fold = sp.hstack([sp.identity(n, format="csr")] * (R + 1) + [sp.csr_matrix((n, R * r))], format="csr")
    prior = np.full(Hst.shape[1], 2 * p / 3)
    iters, conv = np.zeros(B, np.int64), np.ones(B, np.uint8)

    def decode(k, span, Hw, cols, syn_w):
        nonlocal conv
        out = model(sp.csr_matrix(Hw), prior[cols], n_data=n, fold_blocks=span[1]).decode(syn_w)
        iters[:] += out["iters"]
        conv &= out["status"] & 1
        return out["x"]
    out = windowed_model(Hst, layer, W, Cm, fold, syn_h, decode, stop_before_final=True)
    assert len(out["windows"]) >= 1
    span, Hw, cols, syn_f = out["final"]
    ref = model(sp.csr_matrix(Hw), prior[cols], n_data=n, fold_blocks=span[1], logicals=lz).decode(
        syn_f, out["acc"], rd_h)
    status = conv & ref["status"] & 1
    assert 0 < int(status.sum()) < B
    assert np.array_equal(res.corrections, ref["corr"]) and np.array_equal(res.fail, ref["fail"].astype(bool))
    assert np.array_equal(res.detail["iters"], iters + ref["iters"])
    assert np.array_equal(res.detail["status"] & 1, status)
    close(pipe)


@pytest.mark.parametrize("mode", ["bpd_detector", "bposd_detector"])
def test_detector_modes_on_the_storage_dem(gpu_available, code225, mode):
    from exp_ldpc_amd.experiment import BatchPipeline
    from exp_ldpc_amd.noise_model import depolarizing_noise
    from exp_ldpc_amd.storage_sim import build_storage_simulation
    p, B, n, R = 0.03, 96, 225, 1
    noise = depolarizing_noise(p, p)
    sim = build_storage_simulation(R, noise, code225)
    pipe = BatchPipeline(code225, R, mode, OPTS, (2 * p / 3, 2 * p / 3), noise=noise)
    assert pipe.det.schedule == "layered"
    H, F = sp.csr_matrix(pipe.dem.fault_check_matrix), pipe.dem.fault_map
    nf = H.shape[1]
    syn, rd = sim.sample_device(pipe.sampler_graph, B, seed=23, stream_id=1)
    res = pipe.run(syn, rd, want_detail=True)
    syn_h = syn.cpu().numpy()
    v = np.zeros((B, nf), np.uint8)
    v[:, nf - n:] = rd.cpu().numpy()
    ref = model(H, pipe.dem.fault_priors).decode(syn_h)
    x = ref["x"]
    if mode == "bposd_detector":
        x, bad = osd_fix(H, syn_h, ref)
        assert bad.size
    assert 0 < int((ref["status"] & 1).sum()) < B
    assert np.array_equal(res.detail["iters"], ref["iters"])
    assert res.bp_converged == int((ref["status"] & 1).sum())
    assert np.array_equal(res.fail, flags(F, v ^ x))
    close(pipe)


@pytest.mark.parametrize("osd", [False, True])
def test_dem_pipeline_on_a_golden_dem(gpu_available, code225, osd):
    from exp_ldpc_amd.circuit import compile_circuit
    from exp_ldpc_amd.dem import detector_error_model
    from exp_ldpc_amd.experiment import DemPipeline
    gold = compile_circuit(golden_text(2))
    observables = lz_on_readout(code225, gold.num_measurements)
    gold.close()
    dem = detector_error_model(golden_text(2), observables=observables)
    B = 96
    pipe = DemPipeline(dem, OPTS, osd=osd)
    assert pipe.dec.schedule == "layered"
    H = sp.csr_matrix(pipe.dem.fault_check_matrix)
    res = pipe.run(B, SEED, want_detail=True)  # packed=True by default: turned off under the layered schedule
    det, obs = res.detail["det"], res.detail["obs"]
    ref = model(H, pipe.dem.fault_priors).decode(det)
    x = ref["x"]
    if osd:
        x, bad = osd_fix(H, det, ref)
        assert bad.size
    assert 0 < int((ref["status"] & 1).sum()) < B
    assert np.array_equal(res.detail["iters"], ref["iters"])
    assert np.array_equal(res.detail["status"] & 1, ref["status"] & 1)
    Fm = np.asarray(pipe.dem.fault_map.toarray() if hasattr(pipe.dem.fault_map, "toarray") else pipe.dem.fault_map)
    want = ((obs.astype(np.int64) + x.astype(np.int64) @ (Fm.astype(np.int64) % 2).T) % 2).any(axis=1)
    assert np.array_equal(res.fail, want)
    pipe.dec.close()


def test_refusals_need_no_layered_launch(gpu_available, code225):
    from exp_ldpc_amd.decoder import Decoder
    from exp_ldpc_amd.experiment import BatchPipeline
    for mode, R in (("bpssf", 0), ("bpssf", 1), ("bpssf_hybrid", 1)):
        with pytest.raises(ValueError, match="SSF"):
            BatchPipeline(code225, R, mode, OPTS, (0.01, 0.01))
    hz = sp.csr_matrix(code225.checks.z)
    dec = Decoder(hz, 0.02, method="ms", precision="f64", max_iter=5, schedule="layered")
    try:
        syn = np.zeros((2, hz.shape[0]), np.uint8)
        with pytest.raises(ValueError, match="packed"):
            dec.decode(np.zeros((2, 2), np.uint64), packed=True)
        with pytest.raises(ValueError, match="ssf_steps"):
            dec.decode(syn, want=("x", "ssf_steps"))
        with pytest.raises(ValueError, match="SSF"):
            dec.decode(syn, ssf=True)
        with pytest.raises(ValueError, match="SSF"):
            dec.set_flip_sets(code225.checks.x)
        out = dec.decode(syn)  # the default outputs leave ssf_steps out
        assert set(out) == {"x", "corr", "iters", "status", "fail"} and (out["status"] == 3).all()
        assert len(dec.layered_kernel_names()) == 4
    finally:
        dec.close()
