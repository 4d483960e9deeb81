"""The device Pauli-frame sampler (qd_circuit_sample_device, csrc/qdec_frame.hip):
bit for bit against the numpy model of tests/frame_model.py, statistically
against the exact marginals of the storage experiment's DEM, and end to end
through run_simulation under circuit_noise."""
import numpy as np
import pytest

import frame_model
from test_circuit_host import assert_within_sigmas, dem_marginals, golden_text

pytestmark = pytest.mark.gpu

# every instruction, at most 6 qubits, p up to 0.3; qubit 5 is never reset and is
# measured after an H, one noise line names a qubit twice, one record is inverted
TOYS = {
    "all_ops": """
        R 0 1 2
        RX 3 4
        H 0 5
        CX 0 1 3 2
        CZ 1 2 3 4
        CNOT 4 0
        X_ERROR(0.3) 0 1 0
        Y_ERROR(0.2) 2
        Z_ERROR(0.25) 3 4 5
        DEPOLARIZE1(0.3) 0 1 2 3 4 5
        DEPOLARIZE2(0.3) 0 1 2 3 4 5 1 0
        M(0.1) 0 !1
        MX(0.05) 3
        MR 2
        MRX(0.3) 4
        H 2
        CX 2 4 0 1 5 3
        DEPOLARIZE2(0.15) 2 4
        MRZ 5 0
        REPEAT 3 {
            CZ 0 1 2 3
            DEPOLARIZE1(0.1) 0 1 2 3
            MR(0.02) 1 3
            DETECTOR rec[-1] rec[-2]
        }
        MX 0 2 4
        MZ 1 3 5 1
        DETECTOR rec[-1] rec[-4]
        OBSERVABLE_INCLUDE(0) rec[-7] rec[-3]
        OBSERVABLE_INCLUDE(1) rec[-1]
    """,
    "certain": """
        R 0 1
        X_ERROR(1) 0
        DEPOLARIZE1(0) 1
        M 0 1
        MX(1) 0
    """,
}
SEED = 20250221


def _device(cc, B, shot0=0, packed=False, outputs=None, stream_id=3, **kw):
    import torch
    from exp_ldpc_amd.decoder import unpack_rows
    res = cc.sample_device(B, SEED, stream_id=stream_id, shot0=shot0, packed=packed, outputs=outputs, **kw)
    torch.cuda.synchronize()
    out = {}
    for k, t in res.items():
        a = t.cpu().numpy()
        if packed:
            rows = cc.groups[k].shape[0]
            a = a.view(np.uint64).reshape(B, (rows + 63) // 64)
            if rows % 64 and B:
                assert not (a[:, -1] >> np.uint64(rows % 64)).any(), "padding bits must be 0"
            a = unpack_rows(a, rows) if rows else np.zeros((B, 0), np.uint8)
        out[k] = a
    return out


@pytest.fixture(scope="module")
def toys():
    """name -> (compiled circuit, the model's 294 shots from global shot 0)."""
    from exp_ldpc_amd.circuit import compile_circuit
    out = {}
    for name, text in TOYS.items():
        cc = compile_circuit(text)
        assert cc.num_qubits <= 6
        out[name] = (cc, frame_model.sample(cc, SEED, 3, 0, 37 + 257))
    yield out
    for cc, _ in out.values():
        cc.close()


@pytest.mark.parametrize("name", list(TOYS))
@pytest.mark.parametrize("shot0", [0, 37])
@pytest.mark.parametrize("B", [1, 63, 65, 257])
def test_toy_circuits_equal_the_model(gpu_available, toys, name, shot0, B):
    cc, ref = toys[name]
    if name == "all_ops":  # not vacuous: noise fires, randomisation is live, detectors see both values
        assert 0.2 < ref["records"][:, 0].mean() < 0.8 and 0 < ref["detectors"].mean() < 1
        assert {int(o) for o in cc.ops[:, 0]} == set(range(12))
    else:
        assert ref["records"][:, 0].all() and not ref["records"][:, 1].any() and ref["records"][:, 2].any()
    for packed in (False, True):
        got = _device(cc, B, shot0=shot0, packed=packed)
        for k in ("detectors", "observables", "records"):
            assert np.array_equal(got[k], ref[k][shot0:shot0 + B]), (k, packed)


def test_split_over_two_streams_equals_one_call(gpu_available, toys):
    import torch
    cc, ref = toys["all_ops"]
    whole = _device(cc, 257)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        a = cc.sample_device(100, SEED, stream_id=3, shot0=0)
    with torch.cuda.stream(s2):
        b = cc.sample_device(157, SEED, stream_id=3, shot0=100)
    torch.cuda.synchronize()
    for k in whole:
        assert np.array_equal(whole[k], np.concatenate([a[k].cpu().numpy(), b[k].cpu().numpy()])), k
        assert np.array_equal(whole[k], ref[k][:257])
    # other seed / stream: other shots
    assert not np.array_equal(_device(cc, 257, stream_id=4)["records"], whole["records"])


def test_outputs_are_optional_and_empty_batches_write_nothing(gpu_available, toys):
    import torch
    cc, ref = toys["all_ops"]
    only = _device(cc, 65, outputs=("observables",))
    assert list(only) == ["observables"] and np.array_equal(only["observables"], ref["observables"][:65])
    keep = {k: torch.full((0, m.shape[0]), 7, dtype=torch.uint8, device="cuda:0") for k, m in cc.groups.items()}
    assert cc.sample_device(0, SEED, out=keep)["records"].shape == (0, cc.num_measurements)
    words = torch.zeros((5, 1), dtype=torch.int64, device="cuda:0")
    ptrs = (__import__("ctypes").c_void_p * 4)(None, words.data_ptr() + 4, None, None)
    from exp_ldpc_amd import _abi
    rc = _abi.load().qd_circuit_sample_device(cc.handle(0), 1, 0, 0, 4, _abi.QD_INPUT_PACKED, ptrs, None)
    assert rc == -78
    assert _abi.load().qd_circuit_sample_device(cc.handle(0), 1, 0, 0, -1, 0, ptrs, None) == -77
    two = cc.with_groups({"records": cc.record_rows()})  # a buffer for a group the program lacks
    assert _abi.load().qd_circuit_sample_device(two.handle(0), 1, 0, 0, 4, 0, ptrs, None) == -77
    two.close()


# ---------------------------------------------------------------- the golden storage texts
def _golden(R, strip_noise=False):
    from exp_ldpc_amd.circuit import compile_circuit
    from exp_ldpc_amd.storage_sim import storage_output_groups
    text = golden_text(R)
    if strip_noise:
        text = "\n".join(l for l in text.splitlines() if not l.startswith("DEPOLARIZE")).replace("(0.01)", "")
        assert "DEPOLARIZE" not in text and "MRX 225" in text and "MZ 0 1" in text
    cc = compile_circuit(text)
    g = storage_output_groups(cc, 108, 108, 225, R)
    return cc.with_groups({"syn": g["syn"], "readout": g["readout"], "detectors": cc.detectors,
                           "records": cc.record_rows()}), cc.observables


@pytest.mark.parametrize("R", [0, 1, 2, 3])
def test_golden_storage_texts_equal_the_model(gpu_available, R):
    cc, _ = _golden(R)
    B = 130
    ref = frame_model.sample(cc, SEED, 0, 5, B)
    assert ref["syn"].any() and ref["readout"].any()
    for packed in (False, True):
        got = _device(cc, B, shot0=5, packed=packed, stream_id=0)
        for k in ("syn", "readout", "detectors", "records"):
            assert np.array_equal(got[k], ref[k]), (k, packed)
    cc.close()


def test_noiseless_circuit_fires_no_detector(gpu_available):
    """The golden R = 2 text with its noise stripped, 4096 shots: every detector
    and observable is 0 although resets and measurements randomise the frame (a
    test of the gate rules), and the round-1 X-check records are fair coins:
    their mean over 4096 x 108 bits lies in [0.49, 0.51], 13 sigma."""
    cc, observables = _golden(2, strip_noise=True)
    cc = cc.with_groups({"detectors": cc.detectors, "observables": observables, "records": cc.record_rows()})
    got = _device(cc, 4096, stream_id=0)
    assert got["detectors"].shape == (4096, 432) and not got["detectors"].any()
    assert got["observables"].shape == (4096, 9) and not got["observables"].any()
    xmean = got["records"][:, :108].mean()
    print("round-1 X-check mean", xmean)
    assert 0.49 <= xmean <= 0.51
    # the true logical observables Lz readout are 0 too (the text's own lines are degenerate)
    from conftest import load_code
    L = np.asarray(load_code("hgp_12_3_4_s1234").logicals.z) % 2
    assert not ((got["records"][:, -225:].astype(np.int64) @ L.T) % 2).any()
    cc.close()


@pytest.mark.parametrize("R", [1, 3])
def test_kernel_matches_the_dem_marginals(gpu_available, code225, R):
    """2^16 shots of the golden text (depolarizing 0.01 / 0.01): every Z-sector
    detector and every observable (Lz readout, see
    test_circuit_host.test_frame_model_matches_the_dem_marginals) within 5.5
    sigma of its exact DEM marginal."""
    import torch
    N = 1 << 16
    cc, _ = _golden(R)
    res = cc.sample_device(N, SEED + R, outputs=("syn", "readout"))
    H, L = code225.checks.z, np.asarray(code225.logicals.z) % 2
    Lt = torch.tensor(L.T.astype(np.float32), device="cuda:0")
    obs = (res["readout"].float() @ Lt) % 2
    freq = np.concatenate([res["syn"].float().mean(dim=0).cpu().numpy().astype(np.float64),
                           obs.mean(dim=0).cpu().numpy().astype(np.float64)])
    qd, qo = dem_marginals(H, L, R, 0.01, 0.01)
    assert qd.size == (R + 1) * 108 and qo.size == 9
    assert_within_sigmas(freq, np.concatenate([qd, qo]), N)
    cc.close()


# ---------------------------------------------------------------- circuit_noise end to end
OPTS = {"max_iter": 30, "bp_method": "ms", "ms_scaling_factor": 0, "osd_method": "osd_cs", "osd_order": 0}


@pytest.fixture(scope="module")
def noisy_sim(code225):
    from exp_ldpc_amd.noise_model import circuit_noise
    from exp_ldpc_amd.storage_sim import build_storage_simulation
    sim = build_storage_simulation(1, circuit_noise(0.002), code225)
    cc = sim.compiled()
    return sim, cc, frame_model.sample(cc, SEED, 0, 0, 512)


def test_circuit_noise_kernel_equals_the_model(gpu_available, noisy_sim):
    sim, cc, ref = noisy_sim
    assert {int(o) for o in cc.ops[:, 0]} >= {1, 2, 3, 4, 5, 6, 10, 11}  # CX CZ R RX M MX DEPOLARIZE1/2
    assert ref["syn"][:65].any()
    for packed in (False, True):
        got = _device(cc, 65, packed=packed, stream_id=0)
        assert np.array_equal(got["syn"], ref["syn"][:65]) and np.array_equal(got["readout"], ref["readout"][:65])


@pytest.mark.parametrize("mode", ["bposd", "bpssf"])
def test_run_simulation_under_circuit_noise(gpu_available, code225, noisy_sim, mode):
    """run_simulation with noise_model=circuit_noise returns the flags of
    BatchPipeline.run fed the model's samples for the same seed (on the parent
    commit: NotImplementedError at the first batch)."""
    import torch
    from exp_ldpc_amd.experiment import BatchPipeline, _steps
    from exp_ldpc_amd.noise_model import circuit_noise
    from qldpc.misc import run_simulation
    sim, cc, ref = noisy_sim
    xs, zs = _steps(code225.checks)
    p = 0.002
    data_prior = lambda x_steps, z_steps: 2 * p / 3 * (x_steps + z_steps + 2)   # noqa: E731
    meas_prior = lambda x_steps, z_steps: p * (z_steps + 2)                     # noqa: E731
    fail = run_simulation(512, code225, meas_prior, data_prior, circuit_noise, dict(p=p), OPTS, 1, mode, seed=SEED,
                          batch=200)
    assert fail.dtype == bool and fail.shape == (512,)
    pipe = BatchPipeline(code225, 1, mode, OPTS, (data_prior(xs, zs), meas_prior(xs, zs)), noise=circuit_noise(p))
    want = pipe.run(torch.tensor(ref["syn"], device="cuda:0"), torch.tensor(ref["readout"], device="cuda:0")).fail
    assert np.array_equal(fail, np.asarray(want, dtype=bool))
    for dec in pipe.decoders() + [pipe.sampler_graph]:
        dec.close()
