"""Fault propagation on the device (qd_circuit_faults_device, frame_fault_kernel in
csrc/qdec_frame.hip) bit for bit against the numpy model of tests/fault_model.py,
the DEM extracted with it against the model-built one and against the sampler,
and bpd_detector on the circuit's own DEM end to end."""
import numpy as np
import pytest

import fault_model
from test_circuit_dem_host import lz_on_readout, marginals
from test_circuit_host import assert_within_sigmas, golden_text
from test_gpu_circuit import OPTS, SEED, TOYS

pytestmark = pytest.mark.gpu
GROUPS = ("detectors", "observables", "records")


def _device(cc, kind, f0, F, packed):
    """{group: uint8 [F, rows]} of faults f0 .. f0 + F from the device."""
    import torch
    from exp_ldpc_amd.decoder import unpack_rows
    res = cc.fault_symptoms_device(kind=kind, f0=f0, F=F, packed=packed)
    torch.cuda.synchronize()
    out = {}
    for k, t in res.items():
        rows = cc.groups[k].shape[0]
        a = t.cpu().numpy()
        if packed:
            assert a.dtype == np.int64 and a.shape == (F, (rows + 63) // 64)
            a = a.view(np.uint64)
            if rows % 64 and F:
                assert not (a[:, -1] >> np.uint64(rows % 64)).any(), "padding bits must be 0"
            a = unpack_rows(a, rows) if rows and F else np.zeros((F, rows), np.uint8)
        assert a.shape == (F, rows)
        out[k] = a
    return out


@pytest.fixture(scope="module")
def toys():
    """name -> (compiled circuit, [the model's symptoms of every noise fault, of every gauge fault])."""
    from exp_ldpc_amd.circuit import compile_circuit
    out = {}
    for name, text in TOYS.items():
        cc = compile_circuit(text)
        out[name] = (cc, [fault_model.symptoms(cc, kind) for kind in (0, 1)])
    yield out
    for cc, _ in out.values():
        cc.close()


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("name", list(TOYS))
def test_toy_symptoms_equal_the_model(gpu_available, toys, name, kind):
    """Byte and packed rows over windows that start a wave inside an
    instruction (f0 = 37), span several instructions and a wave boundary
    (F = 65), and cover every fault."""
    cc, refs = toys[name]
    ref = refs[kind]
    total = ref["rec"].shape[0]
    if name == "all_ops":  # not vacuous: two waves, both components and record flips reach the outputs
        assert total == (83, 41)[kind] and ref["detectors"].any() and ref["observables"].any()
        assert 0 < ref["records"].mean() < 0.5
    for f0 in (0, 37):
        for F in (1, 63, 65, total):
            f0c = min(f0, total)
            Fc = min(F, total - f0c)            # the small toy ends before some windows do
            for packed in (False, True):
                got = _device(cc, kind, f0c, Fc, packed)
                for k in GROUPS:
                    assert np.array_equal(got[k], ref[k][f0c:f0c + Fc]), (k, f0, F, packed)
    for packed in (False, True):
        empty = _device(cc, kind, 3, 0, packed)
        assert all(empty[k].shape[0] == 0 for k in GROUPS)
    assert set(cc.fault_symptoms_device(kind=kind, F=1, outputs=("observables",))) == {"observables"}


def test_split_over_two_streams_equals_one_call(gpu_available, toys):
    import torch
    cc, refs = toys["all_ops"]
    whole = cc.fault_symptoms_device(kind=0, packed=True)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        a = cc.fault_symptoms_device(kind=0, f0=0, F=30, packed=True)
    with torch.cuda.stream(s2):
        b = cc.fault_symptoms_device(kind=0, f0=30, packed=True)
    torch.cuda.synchronize()
    for k in GROUPS:
        assert b[k].shape[0] == 53 and torch.equal(whole[k], torch.cat([a[k], b[k]])), k
    # bad arguments are refused before anything is enqueued, each with its code
    from exp_ldpc_amd import _abi
    ptrs = (__import__("ctypes").c_void_p * 4)(None, a["observables"].data_ptr() + 4, None, None)
    call = lambda *args: _abi.load().qd_circuit_faults_device(cc.handle(0), *args, ptrs, None)  # noqa: E731
    assert call(0, 0, 4, _abi.QD_INPUT_PACKED) == -78
    assert call(2, 0, 4, 0) == -87 and call(0, -1, 4, 0) == -88 and call(0, 80, 4, 0) == -89 and call(1, 41, 1, 0) == -89
    two = cc.with_groups({"records": cc.record_rows()})  # a buffer for a group the program lacks
    assert _abi.load().qd_circuit_faults_device(two.handle(0), 0, 0, 4, 0, ptrs, None) == -77
    two.close()


# ---------------------------------------------------------------- the DEM of whole circuits
@pytest.fixture(scope="module")
def generated(code225):
    """The circuit_noise(0.003) R = 1 circuit with all its detectors and Lz
    readout as observables, and its device-extracted DEM."""
    from exp_ldpc_amd.circuit import compile_circuit
    from exp_ldpc_amd.dem import detector_error_model
    from exp_ldpc_amd.noise_model import circuit_noise
    from exp_ldpc_amd.storage_sim import build_storage_simulation
    cc = compile_circuit(build_storage_simulation(1, circuit_noise(0.003), code225).circuit)
    cc = cc.with_groups({"detectors": cc.detectors, "observables": lz_on_readout(code225, cc.num_measurements)})
    dem = detector_error_model(cc, detectors=cc.groups["detectors"], observables=cc.groups["observables"])
    yield cc, dem
    cc.close()


def _model_dem(cc):
    from exp_ldpc_amd.dem import dem_from_symptoms
    s = fault_model.symptoms(cc, 0)
    return dem_from_symptoms(cc, s["detectors"], s["observables"])


def test_device_dem_equals_the_model_built_dem(gpu_available, code225, generated):
    """Column for column, probabilities equal as floats: the golden R = 1 text
    (depolarizing) and the generated circuit_noise R = 1 circuit."""
    from exp_ldpc_amd.circuit import compile_circuit
    from exp_ldpc_amd.dem import detector_error_model
    cc, dem = generated
    assert dem.num_errors == 1518 and dem.instructions == _model_dem(cc).instructions
    gold = compile_circuit(golden_text(1))
    gold = gold.with_groups({"detectors": gold.detectors,
                             "observables": lz_on_readout(code225, gold.num_measurements)})
    got = detector_error_model(golden_text(1), observables=gold.groups["observables"])
    assert got.num_errors == 558 and got.instructions == _model_dem(gold).instructions
    # the text's own observable lines are identically 0: the default observables give no L target
    own = detector_error_model(golden_text(1))
    assert own.num_errors == 558 and not any(i.observables for i in own if i.type == "error")
    with pytest.raises(ValueError, match="detector 0 "):
        detector_error_model("RX 0\nM 0\nDETECTOR rec[-1]")
    assert detector_error_model("RX 0\nM 0\nDETECTOR rec[-1]", check_deterministic=False).num_errors == 0


def test_sampler_fits_the_extracted_dem(gpu_available, generated):
    """2^16 device shots of the circuit_noise(0.003) R = 1 circuit: all 216
    detectors and 9 observables within 5.5 sigma of the device-extracted DEM's
    marginals (false alarm below 1e-5 over 225 quantities).  With this seed the
    largest deviation is 4.66 sigma (observable 6); the numpy frame model gives
    the same shots bit for bit and, with another seed, 2.95 sigma."""
    cc, dem = generated
    N = 1 << 16
    res = cc.sample_device(N, SEED + 7)
    freq = np.concatenate([res[k].float().mean(dim=0).cpu().numpy().astype(np.float64)
                           for k in ("detectors", "observables")])
    assert freq.size == 225
    assert_within_sigmas(freq, marginals(dem, 216, 9), N)


# ---------------------------------------------------------------- bpd_detector end to end
P = 0.003


def _oracle_fail(oracle_lib, pipe, det, rd, lz):
    ref = oracle_lib.decode(pipe.dem.fault_check_matrix, pipe.dem.fault_priors, det, method="ms", precision="f32",
                            max_iter=OPTS["max_iter"], want_llr=False)
    obs = (rd.astype(np.int64) @ lz.T.astype(np.int64)) % 2
    return ((obs + ref["x"].astype(np.int64) @ pipe.dem.fault_map.toarray().T.astype(np.int64)) % 2).any(axis=1)


@pytest.mark.parametrize("R, shots", [(1, 512), (2, 256)])
def test_bpd_detector_on_the_circuit_dem_matches_oracle(gpu_available, oracle_lib, code225, R, shots):
    """BatchPipeline under circuit_noise: res.fail equals the oracle's
    any(obs ^ F x) on the extracted matrix and priors and the same detectors; at
    R = 2 X-sector detectors enter.  run_simulation returns the same flags (on
    the parent commit it raises NotImplementedError)."""
    from exp_ldpc_amd.experiment import BatchPipeline, _steps
    from exp_ldpc_amd.noise_model import circuit_noise
    from exp_ldpc_amd.storage_sim import build_storage_simulation
    from qldpc.misc import run_simulation
    lz = np.asarray(code225.logicals.z) % 2
    xs, zs = _steps(code225.checks)
    data_prior = lambda x_steps, z_steps: 2 * P / 3 * (x_steps + z_steps + 2)   # noqa: E731
    meas_prior = lambda x_steps, z_steps: P * (z_steps + 2)                     # noqa: E731
    pipe = BatchPipeline(code225, R, "bpd_detector", OPTS, (data_prior(xs, zs), meas_prior(xs, zs)),
                         noise=circuit_noise(P), precision="f32")
    assert pipe.dem_source == "circuit" and pipe.undetectable_logical_faults == 0
    D = 216 * R
    assert pipe.dem.fault_check_matrix.shape[0] == D and pipe.dem.fault_map.shape[0] == 9
    if R == 1:
        assert pipe.dem.fault_check_matrix.shape[1] == 1518
    sim = build_storage_simulation(R, circuit_noise(P), code225)
    det, rd = pipe.sample(sim, shots, SEED, 0, 0)
    assert det.shape == (shots, D) and rd.shape == (shots, 225)
    res = pipe.run(det, rd)
    want = _oracle_fail(oracle_lib, pipe, det.cpu().numpy(), rd.cpu().numpy(), lz)
    print("failures", int(res.fail.sum()), "of", shots)
    assert np.array_equal(res.fail, want)
    assert 0 < res.fail.sum() < shots
    if R == 1:
        fail = run_simulation(shots, code225, meas_prior, data_prior, circuit_noise, dict(p=P), OPTS, R,
                              "bpd_detector", seed=SEED, batch=200, precision="f32")
        assert fail.dtype == bool and np.array_equal(fail, res.fail)
    for dec in pipe.decoders() + [pipe.sampler_graph]:
        dec.close()


def test_dem_source_circuit_under_depolarizing_noise(gpu_available, oracle_lib, code225):
    """dem_source="circuit" opts the depolarizing rewriter into the circuit DEM:
    432 detectors at R = 2 against the default path's 324, and the flags still
    equal the oracle's on that DEM."""
    import warnings
    from exp_ldpc_amd.experiment import BatchPipeline
    from exp_ldpc_amd.noise_model import depolarizing_noise
    from exp_ldpc_amd.storage_sim import build_storage_simulation
    noise = depolarizing_noise(0.01, 0.01)
    priors = (2 * 0.01 / 3, 0.01)
    with warnings.catch_warnings():
        warnings.simplefilter("error")          # the circuit path decodes the reference's problem: no warning
        pipe = BatchPipeline(code225, 2, "bpd_detector", OPTS, priors, noise=noise, precision="f32",
                             dem_source="circuit")
    with pytest.warns(RuntimeWarning, match="dem_source"):
        default = BatchPipeline(code225, 2, "bpd_detector", OPTS, priors, noise=noise, precision="f32")
    assert default.dem_source == "storage" and default.dem.fault_check_matrix.shape[0] == 324
    assert pipe.dem_source == "circuit" and pipe.dem.fault_check_matrix.shape[0] == 432
    assert pipe.undetectable_logical_faults == 0
    sim = build_storage_simulation(2, noise, code225)
    det, rd = pipe.sample(sim, 256, SEED, 0, 0)
    res = pipe.run(det, rd)
    lz = np.asarray(code225.logicals.z) % 2
    assert np.array_equal(res.fail, _oracle_fail(oracle_lib, pipe, det.cpu().numpy(), rd.cpu().numpy(), lz))
    with pytest.raises(ValueError):
        BatchPipeline(code225, 1, "bposd", OPTS, priors, noise=noise, dem_source="circuit")
    for p in (pipe, default):
        for dec in p.decoders() + [p.sampler_graph]:
            dec.close()
