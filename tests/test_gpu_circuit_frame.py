"""The Pauli frame in HBM (FrameInHbm in csrc/qdec_frame.hip; QD_FRAME_HBM / QD_FRAME_AUTO):
forced onto small circuits it equals the numpy models and the LDS kernels bit for
bit, and circuits beyond the LDS kernels' 160 KiB -- by one qubit, by
measurements, and the n = 10^4 storage circuit -- sample, propagate their faults
and decode end to end."""
import numpy as np
import pytest

import fault_model
import frame_model
from conftest import load_checks, load_logicals
from test_gpu_circuit import OPTS, SEED, TOYS, _device as _sample, _golden
from test_gpu_circuit_dem import GROUPS

pytestmark = pytest.mark.gpu


def _faults(cc, kind, f0, F, packed, frame):
    """{group: uint8 [F, rows]} of faults f0 .. f0 + F under a placement."""
    import torch
    from exp_ldpc_amd.decoder import unpack_rows
    res = cc.fault_symptoms_device(kind=kind, f0=f0, F=F, packed=packed, frame=frame)
    torch.cuda.synchronize()
    out = {}
    for k, t in res.items():
        rows = cc.groups[k].shape[0]
        a = t.cpu().numpy()
        if packed:
            a = a.view(np.uint64)
            if rows % 64 and F:
                assert not (a[:, -1] >> np.uint64(rows % 64)).any(), "padding bits must be 0"
            a = unpack_rows(a, rows) if rows and F else np.zeros((F, rows), np.uint8)
        assert a.shape == (F, rows)
        out[k] = a
    return out


def _both_placements_equal(cc, ref, keys, B, shot0=0, stream_id=3):
    assert cc.frame_info(0, "hbm")["placement"] == "hbm" and cc.frame_info(0, "lds")["placement"] == "lds"
    for packed in (False, True):
        hbm = _sample(cc, B, shot0=shot0, packed=packed, stream_id=stream_id, frame="hbm")
        lds = _sample(cc, B, shot0=shot0, packed=packed, stream_id=stream_id, frame="lds")
        for k in keys:
            assert np.array_equal(hbm[k], ref[k]), (k, packed)
            assert np.array_equal(hbm[k], lds[k]), (k, packed)


# ---------------------------------------------------------------- forced HBM on circuits that fit LDS
@pytest.fixture(scope="module")
def toys():
    """name -> (compiled circuit, the model's 294 shots from global shot 0)."""
    from exp_ldpc_amd.circuit import compile_circuit
    out = {}
    for name, text in TOYS.items():
        cc = compile_circuit(text)
        out[name] = (cc, frame_model.sample(cc, SEED, 3, 0, 37 + 257))
    yield out
    for cc, _ in out.values():
        cc.close()


@pytest.mark.parametrize("name", list(TOYS))
@pytest.mark.parametrize("shot0", [0, 37])
@pytest.mark.parametrize("B", [1, 63, 65, 257])
def test_toys_in_hbm_equal_the_model_and_the_lds_kernel(gpu_available, toys, name, shot0, B):
    cc, ref = toys[name]
    cut = {k: v[shot0:shot0 + B] for k, v in ref.items()}
    _both_placements_equal(cc, cut, ("detectors", "observables", "records"), B, shot0=shot0)


@pytest.mark.parametrize("R", [0, 3])
def test_golden_storage_texts_in_hbm(gpu_available, R):
    """225-target DEPOLARIZE1 lines: three full 64-site batches and a 33-site tail."""
    cc, _ = _golden(R)
    assert any(int(o) == 10 and int(c) == 225 for o, _, c, _ in cc.ops)
    ref = frame_model.sample(cc, SEED, 0, 5, 130)
    assert ref["syn"].any() and ref["readout"].any()
    _both_placements_equal(cc, ref, ("syn", "readout", "detectors", "records"), 130, shot0=5, stream_id=0)
    cc.close()


def test_circuit_noise_program_in_hbm(gpu_available, code225):
    from exp_ldpc_amd.noise_model import circuit_noise
    from exp_ldpc_amd.storage_sim import build_storage_simulation
    cc = build_storage_simulation(1, circuit_noise(0.002), code225).compiled()
    ref = frame_model.sample(cc, SEED, 0, 0, 65)
    assert ref["syn"].any()
    _both_placements_equal(cc, ref, ("syn", "readout"), 65, stream_id=0)
    cc.close()


def _wide_text():
    """150 qubits; an X_ERROR line of 155 targets (neither a multiple of 4 nor of
    64) whose tail repeats qubits inside one 64-site batch (5 5) and across
    batches (0, 64, 128); a DEPOLARIZE2 of 75 disjoint pairs plus two pairs that
    reuse a qubit; DEPOLARIZE1, noisy M and MRX over every qubit."""
    allq = " ".join(str(q) for q in range(150))
    pairs = " ".join(f"{2 * i} {2 * i + 1}" for i in range(75))
    return "\n".join([
        f"RX {' '.join(str(q) for q in range(0, 150, 3))}",
        f"H {' '.join(str(q) for q in range(1, 150, 3))}",
        f"CX {pairs}",
        f"X_ERROR(0.2) {allq} 0 64 128 5 5",
        f"DEPOLARIZE2(0.3) {pairs} 3 149 7 3",
        f"CZ {' '.join(f'{2 * i + 1} {2 * i + 2}' for i in range(74))}",
        f"DEPOLARIZE1(0.25) {allq}",
        f"M(0.1) {allq}",
        "DETECTOR rec[-1] rec[-150]",
        f"MRX(0.2) {allq}",
        "DETECTOR rec[-1] rec[-151] rec[-300]",
        f"MX {allq}",
        "OBSERVABLE_INCLUDE(0) rec[-1] rec[-2] rec[-450]",
    ])


def test_wide_circuit_with_repeated_noise_targets(gpu_available):
    from exp_ldpc_amd.circuit import compile_circuit, handle_op_flags
    cc = compile_circuit(_wide_text())
    assert cc.num_qubits == 150 and cc.num_measurements == 450
    flags = handle_op_flags(cc.handle(0, "hbm"))
    marked = [(int(cc.ops[i, 0]), int(cc.ops[i, 2])) for i in np.nonzero(flags)[0]]
    assert marked == [(7, 155), (11, 154)]            # the X_ERROR and the DEPOLARIZE2 line, nothing else
    ref = frame_model.sample(cc, SEED, 3, 0, 130)
    assert ref["detectors"].any() and ref["observables"].any() and 0.05 < ref["records"].mean() < 0.95
    _both_placements_equal(cc, ref, ("detectors", "observables", "records"), 130)
    cc.close()


@pytest.mark.parametrize("slots", [1, 3])
def test_slot_reuse_does_not_change_the_shots(gpu_available, toys, slots):
    """One block walks several 64-shot words and re-zeroes its slot between them."""
    cc, ref = toys["all_ops"]
    cc.set_frame_slots(0, frame="hbm")
    want = _sample(cc, 257, frame="hbm")
    assert cc.frame_info(0, "hbm")["slots"] == 5          # min(words, default slots)
    cc.set_frame_slots(slots, frame="hbm")
    try:
        for packed in (False, True):
            got = _sample(cc, 257, packed=packed, frame="hbm")
            assert cc.frame_info(0, "hbm")["slots"] == slots
            for k in want:
                assert np.array_equal(got[k], want[k]) and np.array_equal(got[k], ref[k][:257]), (k, packed)
        total = fault_model.symptoms(cc, 0)
        got = _faults(cc, 0, 0, total["rec"].shape[0], True, "hbm")      # 83 faults: two words on <= 3 slots
        assert all(np.array_equal(got[k], total[k]) for k in GROUPS)
    finally:
        cc.set_frame_slots(0, frame="hbm")
    fi = cc.frame_info(0, "hbm")
    assert fi["scratch_bytes"] >= 5 * fi["slot_bytes"] and fi["slot_bytes"] == cc.lds_bytes


def test_two_streams_on_one_hbm_handle(gpu_available, toys):
    import torch
    cc, ref = toys["all_ops"]
    whole = _sample(cc, 257, frame="hbm")
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        a = cc.sample_device(100, SEED, stream_id=3, shot0=0, frame="hbm")
    with torch.cuda.stream(s2):
        b = cc.sample_device(157, SEED, stream_id=3, shot0=100, frame="hbm")
    torch.cuda.synchronize()
    for k in whole:
        assert np.array_equal(whole[k], np.concatenate([a[k].cpu().numpy(), b[k].cpu().numpy()])), k
        assert np.array_equal(whole[k], ref[k][:257])
    # the fault kernel, its window split in two
    wf = cc.fault_symptoms_device(kind=0, packed=True, frame="hbm")
    with torch.cuda.stream(s1):
        fa = cc.fault_symptoms_device(kind=0, f0=0, F=30, packed=True, frame="hbm")
    with torch.cuda.stream(s2):
        fb = cc.fault_symptoms_device(kind=0, f0=30, packed=True, frame="hbm")
    torch.cuda.synchronize()
    for k in GROUPS:
        assert fb[k].shape[0] == 53 and torch.equal(wf[k], torch.cat([fa[k], fb[k]])), k


# ---------------------------------------------------------------- faults
def _faults_equal_everywhere(cc, refs, windows):
    for kind in (0, 1):
        ref = refs[kind]
        total = ref["rec"].shape[0]
        for f0, F in windows(total):
            for packed in (False, True):
                hbm = _faults(cc, kind, f0, F, packed, "hbm")
                lds = _faults(cc, kind, f0, F, packed, "lds")
                for k in cc.groups:
                    assert np.array_equal(hbm[k], ref[k][f0:f0 + F]), (k, kind, f0, F, packed)
                    assert np.array_equal(hbm[k], lds[k]), (k, kind, f0, F, packed)


@pytest.mark.parametrize("name", list(TOYS))
def test_toy_fault_symptoms_in_hbm(gpu_available, toys, name):
    cc, _ = toys[name]
    refs = [fault_model.symptoms(cc, kind) for kind in (0, 1)]
    _faults_equal_everywhere(cc, refs, lambda total: [(0, total), (min(37, total), min(65, total - min(37, total))),
                                                      (min(3, total), 0), (0, min(1, total))])


def test_generated_circuit_fault_symptoms_in_hbm(gpu_available, code225):
    """The circuit_noise R = 1 circuit of code225: every fault, and windows that
    start and end off a multiple of 64."""
    from exp_ldpc_amd.noise_model import circuit_noise
    from exp_ldpc_amd.storage_sim import build_storage_simulation
    from test_circuit_dem_host import lz_on_readout
    cc = build_storage_simulation(1, circuit_noise(0.003), code225).compiled()
    cc = cc.with_groups({"detectors": cc.detectors, "observables": lz_on_readout(code225, cc.num_measurements)})
    refs = [fault_model.symptoms(cc, kind) for kind in (0, 1)]
    assert refs[0]["detectors"].any() and refs[0]["observables"].any()
    _faults_equal_everywhere(cc, refs, lambda total: [(0, total), (37, 130), (total - 101, 101)])
    cc.close()


def test_lines_of_257_targets_take_the_gate_helpers_second_step(gpu_available):
    """514 qubits (10,280 B of frame and records, far inside LDS), every line over
    257 = 4 * 64 + 1 targets or pairs: with four targets per lane in flight the gate
    and measurement helpers run one full step and a step in which lane 0 alone holds
    a target; the noise lines run four 64-site batches and a one-site tail.  The
    order makes every line matter to the records (dropping any one changes the
    model's): RX's random x and DEPOLARIZE1 reach z of the odd qubits through CZ,
    come back to z of the even ones through CX with DEPOLARIZE2's, and H turns
    that into what M reads.  Shots against frame_model in both placements; all
    faults of both kinds, and noise faults 615 .. 745 (inside the DEPOLARIZE2
    line's 514 .. 1542), against fault_model."""
    from exp_ldpc_amd.circuit import compile_circuit
    even = " ".join(str(2 * i) for i in range(257))
    pairs = " ".join(f"{2 * i} {2 * i + 1}" for i in range(257))
    cc = compile_circuit("\n".join([
        f"RX {even}", f"DEPOLARIZE1(0.25) {even}", f"CZ {pairs}", f"DEPOLARIZE2(0.3) {pairs}", f"CX {pairs}",
        f"H {even}", f"M(0.1) {even}", "DETECTOR rec[-1] rec[-257]", "DETECTOR rec[-2] rec[-65] rec[-129]",
        "OBSERVABLE_INCLUDE(0) rec[-1] rec[-64] rec[-193]"]))
    assert cc.num_qubits == 514 and cc.num_measurements == 257 and cc.lds_bytes == 16 * 514 + 8 * 257
    ref = frame_model.sample(cc, SEED, 3, 37, 65)
    assert ref["detectors"].any() and ref["observables"].any() and 0.05 < ref["records"].mean() < 0.95
    _both_placements_equal(cc, ref, ("detectors", "observables", "records"), 65, shot0=37)
    refs = [fault_model.symptoms(cc, kind) for kind in (0, 1)]
    assert refs[0]["rec"].shape[0] == 514 + 1028 + 257 and fault_model.enumerate_faults(cc.ops, 0)[615][0] == 4
    assert all(r["detectors"].any() and r["observables"].any() for r in refs)
    _faults_equal_everywhere(cc, refs, lambda total: [(0, total)] + ([(615, 130)] if total == 1799 else []))
    cc.close()


# ---------------------------------------------------------------- beyond the LDS limit
def test_beyond_the_limit_by_one_qubit(gpu_available):
    """Q = LDS_LIMIT // 16 + 1: RX of all, CX on pairs, DEPOLARIZE1 and a noisy M
    on all; "auto" places it in HBM (the parent commit refuses it with -76) and
    70 shots equal the model; so do fault windows of both kinds that straddle
    instructions."""
    from exp_ldpc_amd import _abi
    from exp_ldpc_amd.circuit import LDS_LIMIT, compile_circuit
    Q = LDS_LIMIT // 16 + 1
    allq = " ".join(str(q) for q in range(Q))
    text = "\n".join([f"RX {allq}", f"CX {' '.join(str(q) for q in range(Q - Q % 2))}", f"DEPOLARIZE1(0.05) {allq}",
                      f"M(0.02) {allq}", f"DETECTOR rec[-1] rec[-{Q}]", f"DETECTOR rec[-2] rec[-{Q - 1}]",
                      f"OBSERVABLE_INCLUDE(0) rec[-1] rec[-{Q}]"])
    cc = compile_circuit(text)
    cc = cc.with_groups({"detectors": cc.detectors, "observables": cc.observables, "records": cc.record_rows()})
    assert cc.num_qubits == Q and cc.lds_bytes > LDS_LIMIT
    with pytest.raises(_abi.QdecError) as e:
        cc.handle(0, "lds")
    assert e.value.rc == -76
    ref = frame_model.sample(cc, SEED, 3, 0, 70)
    assert ref["detectors"].any() and ref["observables"].any()
    for packed in (False, True):
        got = _sample(cc, 70, packed=packed)               # frame="auto"
        for k in ("detectors", "observables", "records"):
            assert np.array_equal(got[k], ref[k]), (k, packed)
    fi = cc.frame_info(0)
    assert fi["placement"] == "hbm" and fi["slot_bytes"] == 24 * Q and fi["slots"] == 2
    # faults: the end of DEPOLARIZE1's 2 Q faults into M's record flips; the gauge faults of RX into M's
    for kind, f0 in ((0, 2 * Q - 101), (1, Q - 101)):
        full = fault_model.enumerate_faults(cc.ops, kind)
        ref = _window_symptoms(cc, kind, f0, 200)
        assert len({i for i, _, _ in full[f0:f0 + 200]}) == 2 and ref["records"].any()
        got = _faults(cc, kind, f0, 200, True, "auto")
        for k in ("detectors", "observables", "records"):
            assert np.array_equal(got[k], ref[k]), (k, kind)
    cc.close()


def _window_symptoms(cc, kind, f0, F):
    """fault_model.symptoms restricted to faults f0 .. f0 + F: the model's own
    propagation run on that slice of its fault list."""
    full = fault_model.enumerate_faults(cc.ops, kind)
    real = fault_model.enumerate_faults
    fault_model.enumerate_faults = lambda ops, k=0: full[f0:f0 + F]
    try:
        return fault_model.symptoms(cc, kind)
    finally:
        fault_model.enumerate_faults = real


def _mr_chain(nm):
    """RX 0, then nm noisy MRs of the qubit, a detector and an observable."""
    from exp_ldpc_amd.circuit import compile_circuit
    cc = compile_circuit("RX 0\nREPEAT %d {\nMR(0.1) 0\n}\nDETECTOR rec[-1] rec[-%d]\nOBSERVABLE_INCLUDE(0) rec[-2]"
                         % (nm, nm))
    return cc.with_groups({"detectors": cc.detectors, "observables": cc.observables, "records": cc.record_rows()})


def _mr_chain_records(cc, seed, stream_id, shot0, B):
    """The model's record of _mr_chain in closed form, from frame_model's own draw
    functions: the program is R 0, RX 0, then (M(0.1) 0, R 0) nm times, so M k is
    Bernoulli site 4 k, record 0 = RX's random bit (randomisation site 1) ^ flip_0
    and record k > 0 = flip_k (the R before it left x = 0).  frame_model.run
    gives the same but walks the 2 nm + 2 instructions one by one (12 s at nm =
    20,479 on a CPU); the test checks the closed form against it on a short chain."""
    nm = cc.num_measurements
    assert [int(o) for o in cc.ops[:4, 0]] == [3, 4, 5, 3] and cc.ops.shape[0] == 2 * nm + 2
    shots = np.uint64(shot0) + np.arange(B, dtype=np.uint64)
    thr = np.uint64(frame_model.threshold(np.asarray([0.1]))[0])
    rec = frame_model._uniforms(0, 4 * nm, shots, (seed, stream_id))[0::4] < thr          # [nm, B]
    rec[0] ^= frame_model._rand_bits(1, 1, shots, (seed, stream_id))[0]
    return np.ascontiguousarray(rec.T).astype(np.uint8)


def test_beyond_the_limit_by_measurements(gpu_available):
    """One qubit, (LDS_LIMIT - 16) // 8 + 1 noisy MRs: 8 B more than LDS holds (the
    parent commit refuses it with -76).  65 shots against the model's record
    (_mr_chain_records) and the detector and observable it implies."""
    from exp_ldpc_amd import _abi
    from exp_ldpc_amd.circuit import LDS_LIMIT
    short = _mr_chain(50)
    assert np.array_equal(_mr_chain_records(short, SEED, 3, 7, 65), frame_model.sample(short, SEED, 3, 7, 65)["rec"])
    nm = (LDS_LIMIT - 16) // 8 + 1
    cc = _mr_chain(nm)
    assert cc.num_measurements == nm and cc.lds_bytes == LDS_LIMIT + 8
    with pytest.raises(_abi.QdecError) as e:
        cc.handle(0, "lds")
    assert e.value.rc == -76
    rec = _mr_chain_records(cc, SEED, 3, 0, 65)
    assert 0.3 < rec[:, 0].mean() < 0.7 and 0.08 < rec[:, 1:].mean() < 0.12
    ref = {"records": rec, "detectors": rec[:, -1:] ^ rec[:, :1], "observables": rec[:, -2:-1]}
    for packed in (False, True):
        got = _sample(cc, 65, packed=packed)               # frame="auto"
        for k in ("detectors", "observables", "records"):
            assert np.array_equal(got[k], ref[k]), (k, packed)
    assert cc.frame_info(0)["placement"] == "hbm"
    short.close()
    cc.close()


# ---------------------------------------------------------------- the n = 10^4 code (config 4)
@pytest.fixture(scope="module")
def hgp10k():
    from exp_ldpc_amd.codes import QuantumCode, QuantumCodeChecks, QuantumCodeLogicals
    hx, hz = load_checks("hgp_80_3_4_s2025")
    lx, lz = load_logicals("hgp_80_3_4_s2025")
    return QuantumCode(QuantumCodeChecks(hx, hz), QuantumCodeLogicals(lx, lz))


@pytest.fixture(scope="module")
def n10k_cc(hgp10k):
    """The compiled circuit_noise(0.001), R = 1 storage circuit of the code (groups syn, readout)."""
    from exp_ldpc_amd.noise_model import circuit_noise
    from exp_ldpc_amd.storage_sim import build_storage_simulation
    cc = build_storage_simulation(1, circuit_noise(0.001), hgp10k).compiled()
    yield cc
    cc.close()


def test_n10k_circuit_noise_samples_equal_the_model(gpu_available, n10k_cc):
    """circuit_noise(0.001), R = 1, Q = M = 19,600 (470,400 B per slot): the device
    samples 70 shots from shot 0, the model only shots 62..69 (a shot depends on
    its global index alone); those rows of syn and readout are compared."""
    cc = n10k_cc
    ref = frame_model.sample(cc, SEED, 0, 62, 8)
    assert ref["syn"].any() and ref["readout"].any()
    for packed in (False, True):
        got = _sample(cc, 70, packed=packed, stream_id=0)
        assert np.array_equal(got["syn"][62:], ref["syn"]) and np.array_equal(got["readout"][62:], ref["readout"])
    fi = cc.frame_info(0)
    assert fi["placement"] == "hbm" and fi["slot_bytes"] == 470400 and fi["slots"] == 2


def test_n10k_noiseless_circuit_is_silent(gpu_available, hgp10k):
    """p = 0: 1,024 shots fire no syn bit and readout Lz^T = 0, although resets and
    measurements randomise the frame."""
    import torch
    from exp_ldpc_amd.noise_model import circuit_noise
    from exp_ldpc_amd.storage_sim import build_storage_simulation
    cc = build_storage_simulation(1, circuit_noise(0.0), hgp10k).compiled()
    res = cc.sample_device(1024, SEED, outputs=("syn", "readout"))
    assert res["syn"].shape == (1024, 2 * hgp10k.checks.z.shape[0]) and not bool(res["syn"].any())
    import scipy.sparse as sp
    lz = torch.tensor(sp.csr_matrix(hgp10k.logicals.z).toarray().astype(np.float32).T, device="cuda:0")
    assert not bool(((res["readout"].float() @ lz) % 2).any())
    rec = cc.with_groups({"records": cc.record_rows(0, hgp10k.checks.x.shape[0])})   # round 1's X-check records are fair coins
    mean = float(rec.sample_device(1024, SEED)["records"].float().mean())
    assert 0.49 <= mean <= 0.51                                    # 5 M bits: 0.01 is 45 sigma
    rec.close()
    cc.close()


def test_n10k_fault_window_equals_the_model(gpu_available, n10k_cc):
    """Noise faults of a 200-fault window that straddles two instructions, against
    fault_model restricted to that window."""
    cc = n10k_cc
    full = fault_model.enumerate_faults(cc.ops, 0)
    ops = [i for i, _, _ in full]
    edge = next(f for f in range(5000, len(full)) if ops[f] != ops[f - 1])    # the first boundary past 5,000 faults
    f0 = edge - 101
    assert len({ops[f] for f in range(f0, f0 + 200)}) == 2
    ref = _window_symptoms(cc, 0, f0, 200)
    assert ref["syn"].any() and ref["readout"].any()
    for packed in (False, True):
        got = _faults(cc, 0, f0, 200, packed, "auto")
        assert np.array_equal(got["syn"], ref["syn"]) and np.array_equal(got["readout"], ref["readout"])


def test_run_simulation_on_the_n10k_code_under_circuit_noise(gpu_available, hgp10k):
    """run_simulation under circuit_noise on the n = 10^4 code (the parent commit
    raises at the first batch): its flags equal BatchPipeline.run fed the device's
    own samples of the same seed, drawn separately through sim.sample_device."""
    from exp_ldpc_amd.experiment import BatchPipeline, _steps
    from exp_ldpc_amd.noise_model import circuit_noise
    from exp_ldpc_amd.storage_sim import build_storage_simulation
    from qldpc.misc import run_simulation
    p = 0.001
    xs, zs = _steps(hgp10k.checks)
    data_prior = lambda x_steps, z_steps: 2 * p / 3 * (x_steps + z_steps + 2)   # noqa: E731
    meas_prior = lambda x_steps, z_steps: p * (z_steps + 2)                     # noqa: E731
    fail = run_simulation(256, hgp10k, meas_prior, data_prior, circuit_noise, dict(p=p), OPTS, 1, "bpssf", seed=SEED,
                          batch=128)
    assert fail.dtype == bool and fail.shape == (256,)
    sim = build_storage_simulation(1, circuit_noise(p), hgp10k)
    pipe = BatchPipeline(hgp10k, 1, "bpssf", OPTS, (data_prior(xs, zs), meas_prior(xs, zs)), noise=circuit_noise(p))
    syn, rd = sim.sample_device(pipe.sampler_graph, 256, SEED, 0, 0)
    assert bool(syn.any()) and bool(rd.any())
    want = pipe.run(syn, rd).fail
    assert np.array_equal(fail, np.asarray(want, dtype=bool))
    for dec in pipe.decoders() + [pipe.sampler_graph]:
        dec.close()
