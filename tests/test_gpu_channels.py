"""PAULI_CHANNEL_1 / PAULI_CHANNEL_2 on the device: the sampler
(frame_sample_kernel, csrc/qdec_frame.hip) bit for bit against the numpy model
of tests/frame_model_channels.py under both frame placements, fault propagation
against tests/fault_model_channels.py, the extracted DEM against the model-built
one and the sampler's frequencies, and biased_circuit_noise through the
detector pipelines against the CPU oracle."""
import numpy as np
import pytest

import fault_model_channels as fmc
import frame_model_channels as frc
from test_channels_host import FIT_TOY, PC1_ARGS, PC2_SKEW, _fmt
from test_circuit_dem_host import lz_on_readout, marginals
from test_circuit_host import assert_within_sigmas
from test_gpu_circuit import OPTS, SEED
from test_gpu_circuit import _device as _sample
from test_gpu_circuit_dem import _device as _faults
from test_gpu_circuit_dem import _oracle_fail
from test_gpu_osd_hbm_pipelines import OPTS as OSD_OPTS
from test_gpu_osd_hbm_pipelines import oracle_bposd

pytestmark = pytest.mark.gpu
GROUPS = ("detectors", "observables", "records")
FRAMES = ("lds", "hbm")
COUNTS = (1, 3, 4, 5, 64, 65, 67)      # around the Philox block of 4 sites and the HBM batch of 64
Q = 2 * max(COUNTS)


def _counts_toy():
    """PAULI_CHANNEL_1 on n distinct targets and PAULI_CHANNEL_2 on n disjoint
    pairs for every n of COUNTS (no qubit twice: the HBM kernel keeps 64 sites
    and applies them at once), a CX layer between the counts so that the flips
    spread, then every qubit measured in Z and in X."""
    lines = [f"R {' '.join(map(str, range(0, Q, 2)))}", f"RX {' '.join(map(str, range(1, Q, 2)))}"]
    for n in COUNTS:
        lines.append(f"PAULI_CHANNEL_1({_fmt(PC1_ARGS)}) " + " ".join(str(Q - 1 - e) for e in range(n)))
        lines.append(f"PAULI_CHANNEL_2({_fmt(PC2_SKEW)}) " + " ".join(map(str, range(2 * n))))
        lines.append("CX " + " ".join(f"{q} {q + 1}" for q in range(0, Q, 2)))
    lines += ["M " + " ".join(map(str, range(Q))), "MX " + " ".join(map(str, range(Q)))]
    lines += ["DETECTOR rec[-1] rec[-2]", f"DETECTOR rec[-{Q + 1}] rec[-{2 * Q}]", "OBSERVABLE_INCLUDE(0) rec[-3] rec[-5]"]
    return "\n".join(lines)


# a qubit twice in one line and in two pairs (applied in site order), an outcome of probability 0 in the middle, totals
# of exactly 1 and of 0, and an argument of 2^-32 (threshold 1: that outcome needs u = 0)
_SIXTEENTHS = _fmt([0.0625] * 14 + [0.125])
_EDGES = f"""
    R 0 1 2
    RX 3 4 5
    CX 3 0 4 1
    PAULI_CHANNEL_1({_fmt(PC1_ARGS)}) 0 1 0 3 0
    PAULI_CHANNEL_2({_fmt(PC2_SKEW)}) 0 1 1 2 3 1 0 2 4 0
    PAULI_CHANNEL_1(0.3, 0, 0.2) 0 1 2 3 4 5
    PAULI_CHANNEL_2({_fmt([0.03 if k % 2 else 0.0 for k in range(15)])}) 0 1 2 3 4 5
    CZ 0 5 1 4
    PAULI_CHANNEL_1(0.25, 0.25, 0.5) 1 2
    PAULI_CHANNEL_2({_SIXTEENTHS}) 2 3 5 4
    PAULI_CHANNEL_1(0, 0, 0) 0 1 2
    PAULI_CHANNEL_2({_fmt([0.0] * 15)}) 0 1
    PAULI_CHANNEL_1({_fmt([2.0 ** -32, 0.2, 0.1])}) 0 4 5
    PAULI_CHANNEL_2({_fmt([2.0 ** -32] + [0.01] * 14)}) 5 0 1 3
    M(0.1) 0 !1 2
    MX 3 4 5
    MR 0 1 2 3 4 5
    PAULI_CHANNEL_1(0, 0.5, 0) 0 1 2 3 4 5
    M 0 1 2 3 4 5
    DETECTOR rec[-1] rec[-7]
    DETECTOR rec[-2]
    OBSERVABLE_INCLUDE(0) rec[-3] rec[-9]
"""
TOYS = {"counts": _counts_toy(), "edges": _EDGES, "fit": FIT_TOY}


@pytest.fixture(scope="module")
def toys():
    """name -> (compiled circuit, the model's 294 shots from global shot 0,
    [the model's symptoms of the noise faults, of the gauge faults])."""
    from exp_ldpc_amd.circuit import compile_circuit
    out = {}
    for name, text in TOYS.items():
        cc = compile_circuit(text)
        out[name] = (cc, frc.sample(cc, SEED, 3, 0, 37 + 257), [fmc.symptoms(cc, kind) for kind in (0, 1)])
    yield out
    for cc, _, _ in out.values():
        cc.close()


def test_the_toys_are_not_vacuous(toys):
    from exp_ldpc_amd import circuit as qc
    cc, ref, _ = toys["counts"]
    dup = qc.handle_op_flags(cc._create(None))
    assert cc.num_qubits == Q and not dup.any()
    assert sorted(int(c) for o, _, c, _ in cc.ops if o == 12) == sorted(COUNTS)
    assert sorted(int(c) // 2 for o, _, c, _ in cc.ops if o == 13) == sorted(COUNTS)
    assert 0.05 < ref["records"][:, :Q].mean() < 0.95 and 0.05 < ref["records"][:, Q:].mean() < 0.95
    cc, ref, _ = toys["edges"]
    dup = qc.handle_op_flags(cc._create(None))
    chan = [i for i, o in enumerate(cc.ops[:, 0]) if o >= 12]
    assert dup[chan].tolist() == [1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0]
    thr = cc.thresholds[chan].tolist()
    assert thr[4] == thr[5] == 0xFFFFFFFF and thr[6] == thr[7] == 0 and thr[8] > 1
    assert int(qc.bern_threshold(2.0 ** -32)) == 1
    assert ref["records"][:, -6:].mean(axis=0).min() > 0.3, "PAULI_CHANNEL_1(0, 0.5, 0) applies Y with probability 1/2"
    assert 0 < ref["detectors"].mean() < 1


@pytest.mark.parametrize("name", ["counts", "edges"])
@pytest.mark.parametrize("frame", FRAMES)
@pytest.mark.parametrize("shot0", [0, 37])
@pytest.mark.parametrize("B", [1, 63, 65, 257])
def test_sample_kernel_equals_the_model(gpu_available, toys, name, frame, shot0, B):
    cc, ref, _ = toys[name]
    assert cc.frame_info(0, frame)["placement"] == frame
    for packed in (False, True):
        got = _sample(cc, B, shot0=shot0, packed=packed, frame=frame)
        for k in GROUPS:
            assert np.array_equal(got[k], ref[k][shot0:shot0 + B]), (k, packed)


@pytest.mark.parametrize("name", ["counts", "edges", "fit"])
@pytest.mark.parametrize("frame", FRAMES)
@pytest.mark.parametrize("kind", [0, 1])
def test_fault_symptoms_equal_the_model(gpu_available, toys, name, frame, kind):
    cc, _, refs = toys[name]
    ref = refs[kind]
    total = ref["rec"].shape[0]
    assert total == len(fmc.enumerate_faults(cc.ops, kind)) > 0
    if kind == 0:
        assert ref["records"].any() and ref["detectors"].any()
    import torch
    from exp_ldpc_amd.decoder import unpack_rows
    for f0, F in ((0, total), (min(37, total // 2), min(65, total - min(37, total // 2)))):
        for packed in (False, True):
            res = cc.fault_symptoms_device(kind=kind, f0=f0, F=F, packed=packed, frame=frame)
            torch.cuda.synchronize()
            for k in GROUPS:
                rows = cc.groups[k].shape[0]
                a = res[k].cpu().numpy()
                if packed:
                    a = unpack_rows(a.view(np.uint64), rows) if rows else np.zeros((F, 0), np.uint8)
                assert np.array_equal(a, ref[k][f0:f0 + F]), (k, f0, F, packed)
    assert _faults(cc, kind, 0, 1, True)["records"].shape == (1, cc.num_measurements)


def test_device_dem_equals_the_model_built_dem_and_the_sampler_fits_it(gpu_available, toys):
    """FIT_TOY: the device-extracted DEM is the one dem.py builds from the
    model's symptoms; 2^16 device shots (the seed and stream of the CPU fit, so
    the same shots: checked on the first 2048) put the 8 detectors and 2
    observables within 5.5 sigma of its marginals, under both placements."""
    from exp_ldpc_amd.dem import dem_from_symptoms, detector_error_model
    cc, _, refs = toys["fit"]
    dem = detector_error_model(cc)
    assert dem.num_errors == 21
    assert dem.instructions == dem_from_symptoms(cc, refs[0]["detectors"], refs[0]["observables"]).instructions
    cols = fmc.dem_columns(cc)
    assert [(tuple(i.detectors), tuple(i.observables)) for i in dem if i.type == "error"] == [c[1:] for c in cols]
    N = 1 << 16
    model = frc.sample(cc, 20250221, 0, 0, 2048)
    for frame in FRAMES:
        res = cc.sample_device(N, 20250221, stream_id=0, frame=frame)
        for k in ("detectors", "observables"):
            assert np.array_equal(res[k][:2048].cpu().numpy(), model[k]), (frame, k)
        freq = np.concatenate([res[k].float().mean(dim=0).cpu().numpy().astype(np.float64)
                               for k in ("detectors", "observables")])
        assert_within_sigmas(freq, marginals(dem, 8, 2), N)
    with pytest.raises(ValueError, match=r"PAULI_CHANNEL_1\(0.1, 0.0, 0.1\)"):
        detector_error_model("PAULI_CHANNEL_1(0.1, 0, 0.1) 0\nM 0\nDETECTOR rec[-1]")
    approx = detector_error_model("PAULI_CHANNEL_1(0.1, 0, 0.1) 0\nM 0\nDETECTOR rec[-1]",
                                  approximate_disjoint_errors=True)
    assert [(i.args, i.detectors) for i in approx if i.type == "error"] == [([0.1], [0])]


# ---------------------------------------------------------------- the n = 225 code, R = 1
P = 0.003


def _extract(code225, noise):
    from exp_ldpc_amd.circuit import compile_circuit
    from exp_ldpc_amd.dem import detector_error_model
    from exp_ldpc_amd.storage_sim import build_storage_simulation
    cc = compile_circuit(build_storage_simulation(1, noise, code225).circuit)
    obs = lz_on_readout(code225, cc.num_measurements)
    try:
        return cc, detector_error_model(cc, detectors=cc.detectors, observables=obs)
    finally:
        cc.close()


def test_biased_noise_at_one_half_gives_the_depolarizing_dem(gpu_available, code225):
    from exp_ldpc_amd.noise_model import biased_circuit_noise, circuit_noise
    cb, biased = _extract(code225, biased_circuit_noise(P, 0.5))
    cd, plain = _extract(code225, circuit_noise(P))
    assert {12, 13} <= set(cb.ops[:, 0].tolist()) and not {10, 11} & set(cb.ops[:, 0].tolist())
    assert np.array_equal(cb.targets, cd.targets) and np.abs(cb.probs - cd.probs).max() <= 1e-15
    eb, ed = [i for i in biased if i.type == "error"], [i for i in plain if i.type == "error"]
    assert len(eb) == len(ed) == 1518
    assert all((a.detectors, a.observables) == (b.detectors, b.observables) for a, b in zip(eb, ed))
    diff = max(abs(a.args[0] - b.args[0]) for a, b in zip(eb, ed))
    print("largest difference of a probability", diff)
    assert diff <= 1e-12


@pytest.mark.parametrize("mode", ["bpd_detector", "bposd_detector"])
def test_detector_modes_under_biased_noise_match_the_oracle(gpu_available, oracle_lib, code225, mode):
    """run_simulation under biased_circuit_noise(P, eta = 10), 256 shots: the
    flags are the oracle's on the pipeline's own DEM and the same detectors
    (BP in f32 for bpd_detector, f64 BP then OSD for bposd_detector)."""
    from exp_ldpc_amd.experiment import BatchPipeline, _steps
    from exp_ldpc_amd.noise_model import biased_circuit_noise
    from exp_ldpc_amd.storage_sim import build_storage_simulation
    from qldpc.misc import run_simulation
    shots, eta = 256, 10.0
    bposd = mode == "bposd_detector"
    opts, precision = (OSD_OPTS, "f64") if bposd else (OPTS, "f32")
    lz = np.asarray(code225.logicals.z) % 2
    xs, zs = _steps(code225.checks)
    data_prior = lambda x_steps, z_steps: 2 * P / 3 * (x_steps + z_steps + 2)   # noqa: E731
    meas_prior = lambda x_steps, z_steps: P * (z_steps + 2)                     # noqa: E731
    noise = biased_circuit_noise(P, eta)
    sim = build_storage_simulation(1, noise, code225)
    assert "PAULI_CHANNEL_2" in "\n".join(sim.circuit) and "DEPOLARIZE" not in "\n".join(sim.circuit)
    pipe = BatchPipeline(code225, 1, mode, opts, (data_prior(xs, zs), meas_prior(xs, zs)), noise=noise,
                         precision=precision, sim=sim)
    assert pipe.dem_source == "circuit" and pipe.dem.fault_check_matrix.shape == (216, 1518)
    det, rd = pipe.sample(sim, shots, SEED, 0, 0)
    det_h, rd_h = det.cpu().numpy(), rd.cpu().numpy()
    if bposd:
        obs = (rd_h.astype(np.int64) @ lz.T.astype(np.int64)) % 2
        want, _ = oracle_bposd(oracle_lib, pipe.dem.fault_check_matrix, pipe.dem.fault_priors, pipe.dem.fault_map,
                               det_h, obs)
    else:
        want = _oracle_fail(oracle_lib, pipe, det_h, rd_h, lz)
    fail = run_simulation(shots, code225, meas_prior, data_prior, biased_circuit_noise, dict(p=P, eta=eta), opts, 1,
                          mode, seed=SEED, batch=200, precision=precision)
    print(mode, "failures", int(fail.sum()), "of", shots)
    assert fail.dtype == bool and np.array_equal(fail, want)
    for dec in pipe.decoders() + [pipe.sampler_graph]:
        dec.close()


def test_a_custom_rewriter_runs_through_p_sweep(gpu_available, code225):
    """A rewriter of the user's own that emits PAULI_CHANNEL_1 (dephasing-biased
    data noise before every measurement step), from text through p_sweep under
    bposd_detector to a failure count."""
    from exp_ldpc_amd.experiment import p_sweep
    from exp_ldpc_amd.noise_model import NoiseRewriter, biased_channel_1, circuit_ticks, tokenize_line

    def dephasing(p):
        def rewrite(targets, circuit):
            out = []
            for step in circuit_ticks(circuit):
                if any(tokenize_line(l)[:1] and tokenize_line(l)[0] in ("MR", "MRX", "M", "MZ", "MX") for l in step):
                    head = [l for l in step if tokenize_line(l)[:1] == ["TICK"]]
                    out += head + [f"PAULI_CHANNEL_1({_fmt(biased_channel_1(p, 1.0))}) " +
                                   " ".join(str(q) for q in targets.data)] + [l for l in step if l not in head]
                else:
                    out += step
            return out
        return NoiseRewriter(rewrite, kind="custom", p=p, pm=0.0)
    prior = lambda p, _, __: 2 * p / 3   # noqa: E731
    res = p_sweep(samples=128, p_values=[0.08], noise_model=dephasing, noise_model_args=lambda p: dict(p=p),
                  meas_prior=prior, data_prior=prior, code=code225, rounds=1, decoder_mode="bposd_detector",
                  bp_osd_options=OSD_OPTS, gpus=1, seed=5, batch=128)
    print(res[["failures", "dem_sector"]])
    assert len(res) == 1 and 0 < int(res["failures"].iloc[0]) < 128 and res["dem_sector"].iloc[0] == "circuit"
