"""Circuit detector error models on the host: the library's elementary-fault
table, the mechanisms and the merge of dem.dem_from_symptoms, fed the symptoms
of the numpy model (tests/fault_model.py); the device propagation is
tests/test_gpu_circuit_dem.py."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import fault_model
import frame_model
from test_circuit_host import assert_within_sigmas, golden_text
from test_gpu_circuit import TOYS
from exp_ldpc_amd import circuit as qc
from exp_ldpc_amd.circuit import compile_circuit
from exp_ldpc_amd.dem import (DetectorSpacetimeCode, check_deterministic_symptoms, dem_from_symptoms, depolarize1_component,
                              depolarize2_component, fault_mechanisms, parse_dem, storage_experiment_dem)
from exp_ldpc_amd.noise_model import circuit_noise
from exp_ldpc_amd.storage_sim import build_storage_simulation, storage_output_groups


def lz_on_readout(code, M):
    """Lz over the last n of M records, the storage pipelines' observables."""
    L = sp.csr_matrix(np.asarray(code.logicals.z.todense() if sp.issparse(code.logicals.z) else code.logicals.z) % 2)
    n = L.shape[1]
    return sp.hstack([sp.csr_matrix((L.shape[0], M - n), dtype=L.dtype), L]).tocsr()


def columns(dem):
    """{(detectors, observables): probability} of a DetectorErrorModel."""
    out = {}
    for ins in dem:
        if ins.type == "error":
            key = (tuple(ins.detectors), tuple(ins.observables))
            assert key not in out, "a merged DEM holds every symptom once"
            out[key] = ins.args[0]
    return out


def marginals(dem, D, K):
    """q = (1 - prod (1 - 2 p_j)) / 2 of every detector and observable."""
    prod = np.ones(D + K)
    for ins in dem:
        if ins.type == "error":
            idx = list(ins.detectors) + [D + o for o in ins.observables]
            prod[idx] *= 1 - 2 * ins.args[0]
    return (1 - prod) / 2


@pytest.fixture(scope="module")
def generated(code225):
    """circuit_noise(0.003), R = 1: the compiled circuit with all its detectors
    and Lz readout as observables, the model's symptoms, the DEM made of them."""
    sim = build_storage_simulation(1, circuit_noise(0.003), code225)
    cc = compile_circuit(sim.circuit)
    obs = lz_on_readout(code225, cc.num_measurements)
    cc = cc.with_groups({"detectors": cc.detectors, "observables": obs})
    s = fault_model.symptoms(cc, 0)
    return cc, s, dem_from_symptoms(cc, s["detectors"], s["observables"])


# ---------------------------------------------------------------- 1. channel identities
_XZ = np.array([0, 1, 3, 2])  # Pauli 0 I, 1 X, 2 Y, 3 Z as bits (x, z): products are XORs


@pytest.mark.parametrize("p", [1e-3, 0.1, 0.75])
def test_independent_components_compose_to_the_depolarizing_channels(p):
    for q in (depolarize1_component(p), fault_model.q1(p)):
        sub = (np.arange(8)[:, None] >> np.arange(3)) & 1                     # subsets of {X, Y, Z}
        net = np.bitwise_xor.reduce(np.where(sub, _XZ[1:][None], 0), axis=1)
        dist = np.bincount(net, weights=np.prod(np.where(sub, q, 1 - q), axis=1), minlength=4)
        assert np.abs(dist - np.array([1 - p, p / 3, p / 3, p / 3])).max() <= 1e-15
    for q in (depolarize2_component(p), fault_model.q2(p)):
        code = np.arange(1, 16)
        gen = _XZ[code >> 2] << 2 | _XZ[code & 3]
        sub = (np.arange(1 << 15)[:, None] >> np.arange(15)) & 1              # the 2^15 subsets of the pairs
        net = np.bitwise_xor.reduce(np.where(sub, gen[None], 0), axis=1)
        dist = np.bincount(net, weights=np.prod(np.where(sub, q, 1 - q), axis=1), minlength=16)
        assert np.abs(dist - np.array([1 - p] + [p / 15] * 15)).max() <= 1e-13


def test_probabilities_above_the_limit_raise():
    assert depolarize1_component(0.75) == 0.5 and abs(depolarize2_component(15 / 16) - 0.5) < 1e-15
    with pytest.raises(ValueError):
        depolarize1_component(0.76)
    with pytest.raises(ValueError):
        depolarize2_component(0.94)
    with pytest.raises(ValueError):
        fault_mechanisms(compile_circuit("DEPOLARIZE1(0.8) 0\nM 0"))
    with pytest.raises(ValueError):
        fault_mechanisms(compile_circuit("DEPOLARIZE2(0.95) 0 1\nM 0"))
    assert fault_mechanisms(compile_circuit("DEPOLARIZE1(0) 0\nX_ERROR(0) 0\nM 0"))[0].size == 0


# ---------------------------------------------------------------- 2. the fault table
def _table_equals_model(cc):
    counts = []
    for kind in (0, 1):
        op, tgt, comp = cc.fault_table(kind)
        want = fault_model.enumerate_faults(cc.ops, kind)
        assert list(zip(op.tolist(), tgt.tolist(), comp.tolist())) == want
        counts.append(len(want))
    assert counts[1] == cc.validate()["rand_sites"]
    return counts


def test_fault_table_equals_the_model():
    cc = compile_circuit(TOYS["all_ops"])
    noise, gauge = _table_equals_model(cc)
    print("all_ops:", noise, "noise faults,", gauge, "gauge faults")
    assert noise >= 65                       # a second wave starts mid-program
    assert set(cc.fault_table(0)[2].tolist()) == {1, 2, 3, 4}
    assert _table_equals_model(compile_circuit(TOYS["certain"]))[0] == 6   # p = 0 and p = 1 are numbered alike
    assert _table_equals_model(compile_circuit(golden_text(1)))[0] == 1341
    # the numbering does not depend on the probabilities
    a = compile_circuit(TOYS["all_ops"].replace("(0.3)", "(0)")).fault_table(0)
    assert all(np.array_equal(u, v) for u, v in zip(a, cc.fault_table(0)))


# ---------------------------------------------------------------- 3. the golden texts
def _hand_written(code, R, p, pm):
    """storage_experiment_dem's columns merged by the same rule, each 2p/3 data
    column read as two independent components of probability q1(p)."""
    hz, lz = code.checks.z, code.logicals.z
    dem = DetectorSpacetimeCode(storage_experiment_dem(hz, lz, R, p, pm))
    Hc, Fc = sp.csc_matrix(dem.fault_check_matrix), sp.csc_matrix(dem.fault_map)
    out = {}
    for j, prior in enumerate(dem.fault_priors):
        key = (tuple(sorted(Hc.indices[Hc.indptr[j]:Hc.indptr[j + 1]].tolist())),
               tuple(sorted(Fc.indices[Fc.indptr[j]:Fc.indptr[j + 1]].tolist())))
        parts = [fault_model.q1(p)] * 2 if prior == 2 * p / 3 else [prior]
        assert prior in (2 * p / 3, pm)
        for q in parts:
            out[key] = out[key] * (1 - q) + q * (1 - out[key]) if key in out else q
    return out


@pytest.mark.parametrize("R, n_syn, n_all", [(1, 558, 558), (2, 891, 1674)])
def test_golden_texts_reproduce_the_hand_written_dem(code225, R, n_syn, n_all):
    cc = compile_circuit(golden_text(R))
    syn = storage_output_groups(cc, 108, 108, 225, R)["syn"]
    obs = lz_on_readout(code225, cc.num_measurements)
    s = fault_model.symptoms(cc, 0, {"syn": syn, "detectors": cc.detectors, "observables": obs})
    assert s["rec"].shape == ({1: 1341, 2: 2907}[R], cc.num_measurements)
    assert fault_mechanisms(cc)[0].size == {1: 1791, 2: 4032}[R]
    got = columns(dem_from_symptoms(cc, s["syn"], s["observables"]))
    want = _hand_written(code225, R, 0.01, 0.01)
    assert len(got) == n_syn and set(got) == set(want)
    worst = max(abs(got[k] - want[k]) for k in got)
    print("largest probability difference", worst)
    assert worst <= 1e-15
    full = dem_from_symptoms(cc, s["detectors"], s["observables"])
    assert full.num_errors == n_all and full.num_detectors == cc.detectors.shape[0] == 216 * R
    # the production rules against the model's own merge, and packed against 0/1 rows
    from exp_ldpc_amd.decoder import pack_rows
    model = fault_model.merge(fault_model.mechanisms(cc.ops, cc.probs), s["detectors"], s["observables"])
    assert [(i.args[0], tuple(i.detectors), tuple(i.observables)) for i in full if i.type == "error"] == model
    packed = dem_from_symptoms(cc, pack_rows(s["detectors"]).view(np.int64), pack_rows(s["observables"]),
                               216 * R, 9)
    assert packed.instructions == full.instructions


# ---------------------------------------------------------------- 4. the generated circuit
def test_generated_circuit_noise_dem(generated):
    cc, s, dem = generated
    assert s["rec"].shape[0] == 16317 and fault_mechanisms(cc)[0].size == 37863
    assert len(fault_model.mechanisms(cc.ops, cc.probs)) == 37863
    assert dem.num_errors == 1518 and dem.num_detectors == 216 and dem.num_observables == 9
    assert all(ins.detectors for ins in dem if ins.type == "error")   # no observable flips unseen
    model = fault_model.merge(fault_model.mechanisms(cc.ops, cc.probs), s["detectors"], s["observables"])
    assert [(i.args[0], tuple(i.detectors), tuple(i.observables)) for i in dem if i.type == "error"] == model
    back = parse_dem(dem.to_text())
    assert back.instructions == dem.instructions
    a, b = DetectorSpacetimeCode(dem), DetectorSpacetimeCode(dem.to_text())
    assert a.fault_check_matrix.shape == (216, 1518) and a.fault_map.shape == (9, 1518)
    assert (a.fault_check_matrix != b.fault_check_matrix).nnz == 0 and (a.fault_map != b.fault_map).nnz == 0
    assert np.array_equal(a.fault_priors, b.fault_priors)


# ---------------------------------------------------------------- 5. sampling against the DEM
def test_frame_model_samples_fit_the_extracted_dem(generated):
    """2^14 shots of the numpy frame model on the circuit_noise(0.003) R = 1
    circuit: each of the 216 detectors and 9 observables (Lz readout) fires
    within 5.5 sigma of q = (1 - prod (1 - 2 p_j)) / 2 over the extracted DEM's
    columns.  A wrong CX / CZ rule or a dropped hook error moves the marginals."""
    cc, _, dem = generated
    N = 1 << 14
    out = frame_model.sample(cc, 20250221, 0, 0, N)
    freq = np.concatenate([out["detectors"].mean(axis=0), out["observables"].mean(axis=0)])
    assert_within_sigmas(freq, marginals(dem, 216, 9), N)


# ---------------------------------------------------------------- 6. determinism
def test_determinism_check(generated, code225):
    cc = compile_circuit("RX 0\nM 0\nDETECTOR rec[-1]")
    g = fault_model.symptoms(cc, 1)
    with pytest.raises(ValueError, match="detector 0 "):
        check_deterministic_symptoms(g["detectors"], g["observables"], 1, 0)
    cc = compile_circuit("R 0\nRX 1\nM 0\nMX 1\nM 1\nDETECTOR rec[-3]\nDETECTOR rec[-2]\nOBSERVABLE_INCLUDE(2) rec[-1]")
    g = fault_model.symptoms(cc, 1)
    from exp_ldpc_amd.decoder import pack_rows
    with pytest.raises(ValueError, match="observable 2 "):
        check_deterministic_symptoms(pack_rows(g["detectors"]), g["observables"], 2, 3)
    gen = generated[0]
    g = fault_model.symptoms(gen, 1)
    assert g["rec"].shape[0] == gen.validate()["rand_sites"] and g["rec"].any()
    check_deterministic_symptoms(g["detectors"], g["observables"], 216, 9)
    for R in (1, 2):
        cc = compile_circuit(golden_text(R))
        g = fault_model.symptoms(cc, 1, {"detectors": cc.detectors,
                                         "observables": lz_on_readout(code225, cc.num_measurements)})
        check_deterministic_symptoms(g["detectors"], g["observables"], 216 * R, 9)


# ---------------------------------------------------------------- 7. edge cases
def test_faults_device_refuses_bad_arguments_each_with_its_code():
    from exp_ldpc_amd import _abi
    lib = _abi.load()
    cc = compile_circuit(TOYS["all_ops"])
    h = cc._create(None)
    noise, gauge = qc.handle_fault_info(h)
    ptrs = (C.c_void_p * 4)()
    call = lambda kind, f0, F, flags=0: lib.qd_circuit_faults_device(h, kind, f0, F, flags, ptrs, None)  # noqa: E731
    assert call(0, 0, noise) == -79 and call(1, 0, gauge) == -79 and call(0, 0, 0) == -79   # host-only
    assert call(2, 0, 1) == -87 and call(-1, 0, 1) == -87
    assert call(0, -1, 1) == -88 and call(0, 0, -1) == -88
    assert call(0, 0, noise + 1) == -89 and call(0, noise, 1) == -89 and call(1, gauge - 1, 2) == -89
    assert call(0, 1 << 40, 1) == -89 and call(0, 1, (1 << 63) - 1) == -89
    assert call(0, 0, 1, 1 << 20) == -77
    op = np.zeros(noise, np.int32)
    assert lib.qd_circuit_fault_table(h, 2, _abi.ptr(op), _abi.ptr(op), _abi.ptr(op)) == -87
    qc.destroy_handle(h)
    with pytest.raises(ValueError):
        cc.fault_table(2)


def test_merge_rules():
    cc = compile_circuit("X_ERROR(0.1) 0\nX_ERROR(0.2) 0\nZ_ERROR(0.3) 0\nM 0\nDETECTOR rec[-1]")
    s = fault_model.symptoms(cc, 0)
    assert s["detectors"].ravel().tolist() == [1, 1, 0, 1]   # the noiseless M has its record-flip fault too
    dem = dem_from_symptoms(cc, s["detectors"], s["observables"])
    assert dem.num_errors == 1 and dem.instructions[0].args == [0.1 + 0.2 - 2 * 0.1 * 0.2]
    assert dem.instructions[0].detectors == [0] and dem.to_text() == "error(%r) D0\ndetector D0\n" % 0.26
    # a fault named twice in one mechanism cancels; named three times it counts once
    twice = dem_from_symptoms(cc, s["detectors"], s["observables"], mechanisms=([0.5], [[0, 0, -1, -1]]))
    assert twice.num_errors == 0
    thrice = dem_from_symptoms(cc, s["detectors"], s["observables"], mechanisms=([0.5, 0.25], [[0, 0, 1, 2],
                                                                                              [1, 0, 0, -1]]))
    assert [i.args for i in thrice if i.type == "error"] == [[0.5 * 0.75 + 0.25 * 0.5]]
    # an observable without a detector is kept, in order of first appearance
    cc = compile_circuit("X_ERROR(0.125) 1 0\nM 0 1\nDETECTOR rec[-2]\nOBSERVABLE_INCLUDE(0) rec[-1]")
    s = fault_model.symptoms(cc, 0)
    dem = dem_from_symptoms(cc, s["detectors"], s["observables"])
    assert [(i.detectors, i.observables) for i in dem if i.type == "error"] == [([], [0]), ([0], [])]
