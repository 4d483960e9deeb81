"""Relay-BP behind the pipelines: the bprelay and bprelay_detector modes,
DemPipeline(relay=...) and ldpc_compat.relay_decoder.  Each equals "the mode's
BP stage (the CPU oracle), then the numpy model (tests/relay_model.py) on the
shots BP left unconverged", flag for flag.  Min-sum f64, the n = 225 code."""
import numpy as np
import pytest

from relay_model import RelayModel
from test_circuit_dem_host import lz_on_readout
from test_circuit_host import golden_text

pytestmark = pytest.mark.gpu

SEED = 20250221
OPTS = {"max_iter": 20, "bp_method": "ms", "ms_scaling_factor": 0, "osd_method": "osd_cs", "osd_order": 7}
RELAY = dict(gamma0=0.125, pre_iter=8, num_sets=3, set_max_iter=8, gamma_dist_interval=(-0.25, 0.75), stop_nconv=2,
             alpha=1.0, seed=3)


def relay_model(H, priors, n, **kw):
    gam = np.random.Generator(np.random.PCG64(RELAY["seed"])).uniform(*RELAY["gamma_dist_interval"],
                                                                      (RELAY["num_sets"], n))
    keys = ("gamma0", "pre_iter", "num_sets", "set_max_iter", "stop_nconv", "alpha")
    return RelayModel(H, priors, np.float64, gammas=gam, **{k: RELAY[k] for k in keys}, **kw)


def bp_then_model(oracle_lib, H, priors, det, **kw):
    """(x, BP status, relay status of the shots BP left) of the oracle's BP
    followed by the model on the unconverged shots."""
    ref = oracle_lib.decode(H, priors, det, method="ms", precision="f64", max_iter=OPTS["max_iter"], want_llr=False)
    x = ref["x"].copy()
    bad = np.flatnonzero((ref["status"] & 1) == 0)
    solved = np.zeros(0, np.uint8)
    if bad.size:
        out = relay_model(H, priors, H.shape[1], **kw).decode(det[bad])
        x[bad] = out["x"]
        solved = out["status"]
    return x, ref["status"], solved


def dem_flags(F, obs, x):
    Fm = np.asarray(F.toarray() if hasattr(F, "toarray") else F).astype(np.int64) % 2
    return ((obs.astype(np.int64) + x.astype(np.int64) @ Fm.T) % 2).any(axis=1)


def test_bprelay_mode_at_one_round(gpu_available, oracle_lib, code225):
    from exp_ldpc_amd.experiment import BatchPipeline
    from exp_ldpc_amd.noise_model import depolarizing_noise
    from exp_ldpc_amd.spacetime import SpacetimeCode
    from exp_ldpc_amd.storage_sim import build_storage_simulation
    p, B, n = 0.03, 256, 225
    lz = np.asarray(code225.logicals.z) % 2
    sim = build_storage_simulation(1, depolarizing_noise(p, p), code225)
    pipe = BatchPipeline(code225, 1, "bprelay", OPTS, (2 * p / 3, 2 * p / 3), relay=RELAY)
    syn, rd = sim.sample_device(pipe.sampler_graph, B, seed=21, stream_id=1)
    res = pipe.run(syn, rd, want_corrections=True)
    Hst = SpacetimeCode(code225.checks.z, 1).spacetime_check_matrix
    x, status, solved = bp_then_model(oracle_lib, Hst, np.full(Hst.shape[1], 2 * p / 3), syn.cpu().numpy())
    corr = x[:, :n] ^ x[:, n:2 * n]
    want = ((rd.cpu().numpy() ^ corr).astype(np.int64) @ lz.T.astype(np.int64) % 2).any(axis=1)
    assert 0 < int((status & 1).sum()) < B and 0 < int((solved == 3).sum()) < solved.size
    assert res.bp_converged == int((status & 1).sum())
    assert np.array_equal(res.corrections, corr) and np.array_equal(res.fail, want)
    # the options may also travel in bp_osd_options, and the placement does not matter
    opts = dict(OPTS, **{f"relay_{k}": v for k, v in RELAY.items()}, relay_placement="hbm")
    again = BatchPipeline(code225, 1, "bprelay", opts, (2 * p / 3, 2 * p / 3)).run(syn, rd, want_corrections=True)
    assert np.array_equal(again.corrections, corr) and np.array_equal(again.fail, want)
    with pytest.raises(ValueError):
        BatchPipeline(code225, 1, "bposd", OPTS, (2 * p / 3, 2 * p / 3), relay=RELAY)
    print(f"bprelay R = 1: {B} shots, BP converged on {res.bp_converged}, relay solved {int((solved == 3).sum())} of "
          f"{solved.size}, failures {int(want.sum())}")
    for dec in pipe.decoders() + [pipe.sampler_graph]:
        dec.close()


def test_bprelay_detector_under_circuit_noise(gpu_available, oracle_lib, code225):
    from exp_ldpc_amd.experiment import BatchPipeline, _steps
    from exp_ldpc_amd.noise_model import circuit_noise
    from exp_ldpc_amd.storage_sim import build_storage_simulation
    from qldpc.misc import run_simulation
    P, R, shots = 0.003, 1, 128
    lz = np.asarray(code225.logicals.z) % 2
    xs, zs = _steps(code225.checks)
    data_prior = lambda x_steps, z_steps: 2 * P / 3 * (x_steps + z_steps + 2)   # noqa: E731
    meas_prior = lambda x_steps, z_steps: P * (z_steps + 2)                     # noqa: E731
    sim = build_storage_simulation(R, circuit_noise(P), code225)
    pipe = BatchPipeline(code225, R, "bprelay_detector", OPTS, (data_prior(xs, zs), meas_prior(xs, zs)),
                         noise=circuit_noise(P), precision="f64", sim=sim, relay=RELAY)
    assert pipe.dem_source == "circuit"
    H = pipe.dem.fault_check_matrix
    assert H.shape == (216, 1518)
    det, rd = pipe.sample(sim, shots, SEED, 0, 0)
    res = pipe.run(det, rd)
    obs = (rd.cpu().numpy().astype(np.int64) @ lz.T.astype(np.int64)) % 2
    x, status, solved = bp_then_model(oracle_lib, H, pipe.dem.fault_priors, det.cpu().numpy())
    want = dem_flags(pipe.dem.fault_map, obs, x)
    assert res.bp_converged == int((status & 1).sum()) < shots and (solved == 3).any()
    assert np.array_equal(res.fail, want)
    opts = dict(OPTS, **{f"relay_{k}": v for k, v in RELAY.items()})
    fail = run_simulation(shots, code225, meas_prior, data_prior, circuit_noise, dict(p=P), opts, R,
                          "bprelay_detector", seed=SEED, batch=50, precision="f64")
    assert fail.dtype == bool and np.array_equal(fail, want)
    print(f"bprelay_detector R = 1: {shots} shots, BP converged on {res.bp_converged}, relay solved "
          f"{int((solved == 3).sum())} of {solved.size}, failures {int(want.sum())}")
    for dec in pipe.decoders() + [pipe.sampler_graph]:
        dec.close()


def test_dem_pipeline_with_relay_on_a_golden_dem(gpu_available, oracle_lib, code225):
    from exp_ldpc_amd.circuit import compile_circuit
    from exp_ldpc_amd.dem import detector_error_model
    from exp_ldpc_amd.experiment import DemPipeline
    from qldpc.misc import run_dem_simulation
    gold = compile_circuit(golden_text(2))
    observables = lz_on_readout(code225, gold.num_measurements)
    gold.close()
    dem = detector_error_model(golden_text(2), observables=observables)
    B = 128
    with pytest.raises(ValueError):
        DemPipeline(dem, OPTS, osd=True, relay=RELAY)
    pipe = DemPipeline(dem, OPTS, relay=RELAY)
    H = pipe.dem.fault_check_matrix
    assert H.shape == (432, 1674)
    res = pipe.run(B, SEED, want_detail=True)
    x, status, solved = bp_then_model(oracle_lib, H, pipe.dem.fault_priors, res.detail["det"])
    want = dem_flags(pipe.dem.fault_map, res.detail["obs"], x)
    assert np.array_equal(res.detail["status"], status) and 0 < res.bp_converged < B
    assert (solved == 3).any()
    assert np.array_equal(res.fail, want)
    pipe.dec.close()
    a = run_dem_simulation(B, dem, OPTS, seed=SEED, batch=48, relay=RELAY)
    assert a.dtype == bool and np.array_equal(a, want)
    print(f"golden R = 2 DEM: {B} shots, BP converged on {res.bp_converged}, relay solved "
          f"{int((solved == 3).sum())} of {solved.size}, failures {int(want.sum())}")


def test_relay_decoder_object_agrees_with_the_batched_call(gpu_available, code225):
    from exp_ldpc_amd.decoder import Decoder
    from qldpc.misc import relay_decoder
    hz = code225.checks.z
    p, B = 0.03, 12
    kw = {k: v for k, v in RELAY.items() if k != "alpha"}
    obj = relay_decoder(hz, error_rate=p, ms_scaling_factor=0.625, precision="f64", **kw)
    dec = Decoder(hz, p, method="ms", precision="f64")
    dec.set_relay(**dict(RELAY, alpha=0.625))
    e = (np.random.default_rng(9).random((B, 225)) < 0.04).astype(np.uint8)
    syn = (hz.dot(e.T.astype(np.int64)).T & 1).astype(np.uint8)
    batch = dec.relay(syn, want=("x", "llr", "iters", "legs", "status"))
    mdl = RelayModel(hz, p, np.float64, gammas=obj.gammas,
                     **{k: RELAY[k] for k in ("gamma0", "pre_iter", "num_sets", "set_max_iter", "stop_nconv")},
                     alpha=0.625).decode(syn)
    assert 0 < int((batch["status"] == 3).sum()) < B
    for b in range(B):
        x = obj.decode(syn[b] if b % 2 else e[b])  # a syndrome, or an error vector
        assert x.dtype == np.int64 and np.array_equal(x, batch["x"][b]) and np.array_equal(x, mdl["x"][b])
        assert obj.iter == batch["iters"][b] == mdl["iters"][b] and obj.legs == batch["legs"][b] == mdl["legs"][b]
        assert obj.converge == int(batch["status"][b] == 3) == int(mdl["status"][b] == 3)
        assert obj.log_prob_ratios.tobytes() == batch["llr"][b].tobytes() == mdl["llr"][b].tobytes()
    dec.close()
