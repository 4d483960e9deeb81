"""BP+OSD on detector error models end to end: the bposd_detector mode under
circuit noise, DemPipeline(osd=True) on the golden R = 3 DEM, and the existing
bposd mode with its OSD rows forced into HBM.  Min-sum f64, 30 iterations,
osd_cs 7, the n = 225 code; flags against the CPU oracle (BP, then the compiled
OSD on the shots BP left unconverged; oracle/osd_py.py on the first two of them).

Oracle cost at R = 2 (432 x 14,770, 256 shots, of which BP converges on one):
BP 1.4 s, compiled OSD 0.6 s, the numpy OSD 1.1 s per shot."""
import numpy as np
import pytest

from test_circuit_dem_host import lz_on_readout
from test_circuit_host import golden_text

pytestmark = pytest.mark.gpu

SEED = 20250221
P = 0.003
OPTS = {"max_iter": 30, "bp_method": "ms", "ms_scaling_factor": 0, "osd_method": "osd_cs", "osd_order": 7}


def oracle_bposd(oracle_lib, H, priors, F, det, obs, cross_check=2):
    """(flags, status) of the oracle: x from BP, replaced by the OSD solution on
    the shots BP did not converge on; flag = any(obs ^ F x).  The first
    `cross_check` unconverged shots also go through the numpy OSD."""
    from oracle.osd_py import osd_decode
    ref = oracle_lib.decode(H, priors, det, method="ms", precision="f64", max_iter=30, want_llr=True)
    x = ref["x"].copy()
    bad = np.flatnonzero((ref["status"] & 1) == 0)
    if bad.size:
        _, ow = oracle_lib.osd(H, det[bad], ref["llr"][bad], "osd_cs", 7)
        for i in range(min(cross_check, bad.size)):
            _, rw = osd_decode(H, det[bad[i]], ref["llr"][bad[i]], "osd_cs", 7)
            assert np.array_equal(ow[i], rw), bad[i]
        x[bad] = ow
    Fm = np.asarray(F.toarray() if hasattr(F, "toarray") else F).astype(np.int64) % 2
    flags = ((obs.astype(np.int64) + x.astype(np.int64) @ Fm.T) % 2).any(axis=1)
    return flags, ref["status"]


@pytest.mark.parametrize("R, shots, cols, kind", [(1, 512, 1518, 1), (2, 256, 14770, 2)])
def test_bposd_detector_under_circuit_noise(gpu_available, oracle_lib, code225, R, shots, cols, kind):
    """res.fail equals the oracle's any(obs ^ F x) with x the OSD solution where
    BP did not converge; osd_rows "auto" keeps R = 1 on chip and sends R = 2 to
    HBM; "hbm", "host" and a byte budget that forces sub-batches of about 100
    shots return the same flags."""
    from exp_ldpc_amd.experiment import BatchPipeline, _steps
    from exp_ldpc_amd.noise_model import circuit_noise
    from exp_ldpc_amd.storage_sim import build_storage_simulation
    lz = np.asarray(code225.logicals.z) % 2
    xs, zs = _steps(code225.checks)
    data_prior = lambda x_steps, z_steps: 2 * P / 3 * (x_steps + z_steps + 2)   # noqa: E731
    meas_prior = lambda x_steps, z_steps: P * (z_steps + 2)                     # noqa: E731
    sim = build_storage_simulation(R, circuit_noise(P), code225)
    pipe = BatchPipeline(code225, R, "bposd_detector", OPTS, (data_prior(xs, zs), meas_prior(xs, zs)),
                         noise=circuit_noise(P), precision="f64", sim=sim)
    assert pipe.dem_source == "circuit" and pipe.osd_rows == "auto"
    H = pipe.dem.fault_check_matrix
    assert H.shape == (216 * R, cols)
    assert pipe.det.osd_kernel_info(rows="auto")[0] == kind       # 1: the workgroup kernel, 2: the HBM kernel
    assert pipe.det.osd_device_supported == (kind == 1)
    det, rd = pipe.sample(sim, shots, SEED, 0, 0)
    res = pipe.run(det, rd)
    det_h, rd_h = det.cpu().numpy(), rd.cpu().numpy()
    obs = (rd_h.astype(np.int64) @ lz.T.astype(np.int64)) % 2
    want, status = oracle_bposd(oracle_lib, H, pipe.dem.fault_priors, pipe.dem.fault_map, det_h, obs)
    assert res.bp_converged == int((status & 1).sum()) and res.bp_converged < shots
    assert np.array_equal(res.fail, want)
    for rows, budget in (("hbm", None), ("host", None), ("auto", 100 * cols * 8)):
        pipe.osd_rows = rows
        pipe.llr_budget_bytes = budget or pipe.llr_budget_bytes
        again = pipe.run(det, rd)
        assert np.array_equal(again.fail, want), (rows, budget)
        assert again.bp_converged == res.bp_converged and again.iters_sum == res.iters_sum
    # the same decoder without the OSD stage, for the record (not asserted)
    pipe.mode = "bpd_detector"
    bp_only = pipe.run(det, rd)
    pipe.mode = "bposd_detector"
    print(f"R = {R}: failures of {shots} shots: bpd_detector {int(bp_only.fail.sum())}, "
          f"bposd_detector {int(res.fail.sum())}; BP converged on {res.bp_converged}")
    if R == 1:
        from qldpc.misc import run_simulation
        fail = run_simulation(shots, code225, meas_prior, data_prior, circuit_noise, dict(p=P), OPTS, R,
                              "bposd_detector", seed=SEED, batch=200, precision="f64")
        assert fail.dtype == bool and np.array_equal(fail, want)
    for dec in pipe.decoders() + [pipe.sampler_graph]:
        dec.close()


@pytest.fixture(scope="module")
def golden_dem(code225):
    """The DEM of the golden R = 3 circuit text (depolarizing 0.01 / 0.01) with
    Lz on the readout as observables: 648 detectors, 2,898 faults."""
    from exp_ldpc_amd.circuit import compile_circuit
    from exp_ldpc_amd.dem import detector_error_model
    gold = compile_circuit(golden_text(3))
    observables = lz_on_readout(code225, gold.num_measurements)
    gold.close()
    return detector_error_model(golden_text(3), observables=observables)


def test_dem_pipeline_with_osd_on_the_golden_dem(gpu_available, oracle_lib, golden_dem):
    """DemPipeline(osd=True): 648 x 2,898 is 233 KiB of rows, which "auto" sends
    to HBM; about half the shots do not converge; the flags equal the oracle's;
    run_dem_simulation(osd=True) does not depend on the batch; osd=False returns
    what it did (BP only, whatever osd_method the options carry)."""
    from exp_ldpc_amd.experiment import DemPipeline
    from qldpc.misc import run_dem_simulation
    B = 256
    pipe = DemPipeline(golden_dem, OPTS, osd=True)
    H = pipe.dem.fault_check_matrix
    assert H.shape == (648, 2898)
    assert pipe.dec.osd_kernel_info() is None and pipe.dec.osd_kernel_info(rows="auto")[0] == 2
    res = pipe.run(B, SEED, want_detail=True)
    want, status = oracle_bposd(oracle_lib, H, pipe.dem.fault_priors, pipe.dem.fault_map, res.detail["det"],
                                res.detail["obs"])
    assert np.array_equal(res.detail["status"], status)
    assert B // 4 < res.bp_converged < 3 * B // 4
    assert np.array_equal(res.fail, want)
    pipe.llr_budget_bytes = 100 * 2898 * 8
    assert np.array_equal(pipe.run(B, SEED).fail, want)
    pipe.dec.close()
    a = run_dem_simulation(B, golden_dem, OPTS, seed=SEED, batch=96, osd=True)
    assert a.dtype == bool and np.array_equal(a, want)
    # BP only, as before: the oracle's BP decision alone
    plain = DemPipeline(golden_dem, OPTS)
    bp = plain.run(B, SEED, want_detail=True)
    plain.dec.close()
    ref = oracle_lib.decode(H, pipe.dem.fault_priors, bp.detail["det"], method="ms", precision="f64", max_iter=30,
                            want_llr=False)
    Fm = pipe.dem.fault_map.toarray().astype(np.int64) % 2
    bp_want = ((bp.detail["obs"].astype(np.int64) + ref["x"].astype(np.int64) @ Fm.T) % 2).any(axis=1)
    assert np.array_equal(bp.detail["det"], res.detail["det"]) and np.array_equal(bp.fail, bp_want)
    assert np.array_equal(run_dem_simulation(B, golden_dem, OPTS, seed=SEED, batch=96), bp_want)
    print(f"golden R = 3 DEM: failures of {B} shots: BP {int(bp_want.sum())}, BP+OSD {int(want.sum())}; "
          f"BP converged on {res.bp_converged}")


def test_bposd_mode_with_rows_in_hbm_equals_the_default(gpu_available, code225):
    """The existing bposd mode at R = 1, 2,000 shots (as in
    test_pipeline_device_osd_equals_host_osd): osd_rows="hbm" returns the
    corrections and flags of the default (the register kernel)."""
    from exp_ldpc_amd.experiment import BatchPipeline
    from exp_ldpc_amd.noise_model import depolarizing_noise
    from exp_ldpc_amd.storage_sim import build_storage_simulation
    opts = {"max_iter": 20, "bp_method": "ms", "ms_scaling_factor": 0, "osd_method": "osd_cs", "osd_order": 7}
    p = 0.03
    sim = build_storage_simulation(1, depolarizing_noise(p, p), code225)
    pipe = BatchPipeline(code225, 1, "bposd", opts, (2 * p / 3, 2 * p / 3))
    assert pipe.osd_rows == "onchip"
    syn, rd = sim.sample_device(pipe.sampler_graph, 2000, seed=21, stream_id=1)
    default = pipe.run(syn, rd, want_corrections=True)
    assert pipe.st.osd_hbm_info()[1] == 0  # no HBM launch so far
    hbm = BatchPipeline(code225, 1, "bposd", opts, (2 * p / 3, 2 * p / 3), osd_rows="hbm")
    got = hbm.run(syn, rd, want_corrections=True)
    assert hbm.st.osd_hbm_info()[1] > 0
    assert np.array_equal(got.corrections, default.corrections) and np.array_equal(got.fail, default.fail)
    assert default.bp_converged < 2000
    for pl in (pipe, hbm):
        for dec in pl.decoders() + [pl.sampler_graph]:
            dec.close()
