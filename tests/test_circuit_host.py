"""Host side of the circuit sampler: the parser and compiler (circuit.py), the
edge colouring and the generated storage circuit (schedule.py), the library's
program validation (qd_circuit_create_host) and the numpy frame model
(tests/frame_model.py) against the exact detector marginals of the storage
experiment's DEM."""
import gzip
import os
from collections import Counter

import numpy as np
import pytest
import scipy.sparse as sp

import frame_model
from conftest import GOLDEN, load_checks
from exp_ldpc_amd import circuit as qc
from exp_ldpc_amd.circuit import compile_circuit, parse
from exp_ldpc_amd.noise_model import circuit_noise, depolarizing_noise, trivial_noise
from exp_ldpc_amd.schedule import edge_color_bipartite, storage_circuit_text
from exp_ldpc_amd.storage_sim import build_storage_simulation, storage_output_groups


def golden_text(R):
    with gzip.open(os.path.join(GOLDEN, f"storage_R{R}.txt.gz"), "rt") as f:
        return f.read()


def dem_marginals(H, L, R, p, pm):
    """Exact firing probability of every detector and observable of the storage
    experiment: q = (1 - prod_j (1 - 2 p_j)) / 2 over the DEM's faults touching it."""
    from exp_ldpc_amd.dem import DetectorSpacetimeCode, storage_experiment_dem
    dem = DetectorSpacetimeCode(storage_experiment_dem(H, L, R, p, pm))

    def rows(mat):
        mat = sp.csr_matrix(mat)
        return np.array([(1 - np.prod(1 - 2 * dem.fault_priors[mat.indices[mat.indptr[i]:mat.indptr[i + 1]]])) / 2
                         for i in range(mat.shape[0])])
    return rows(dem.fault_check_matrix), rows(dem.fault_map)


def assert_within_sigmas(freq, q, N, sigmas=5.5):
    sigma = np.sqrt(q * (1 - q) / N)
    dev = np.abs(freq - q) / sigma
    print(f"largest deviation {dev.max():.2f} sigma over {q.size} quantities at N = {N}")
    assert (dev <= sigmas).all(), (int(dev.argmax()), float(dev.max()))


# ---------------------------------------------------------------- 1. parser
def test_every_supported_instruction_parses():
    text = """
        QUBIT_COORDS(0, 1) 0
        R 0 1      # comment
        RZ 2
        RX 3
        H 0
        CX 0 1 2 3
        CNOT 1 0
        CZ 0 2
        TICK
        X_ERROR(0.1) 0
        Y_ERROR(0.2) 1
        Z_ERROR(0.3) 2 3
        DEPOLARIZE1(0.05) 0 1
        DEPOLARIZE2(0.06) 0 1 2 3
        M 0
        MZ(0.01) 1
        MX 2
        MR(0.02) 3
        MRZ 0
        MRX !1
        SHIFT_COORDS(1, 0)
        DETECTOR(0, 1) rec[-1] rec[-6]
        OBSERVABLE_INCLUDE(1) rec[-2]
        OBSERVABLE_INCLUDE(1) rec[-3] rec[-2]
    """
    pc = parse(text)
    assert [i.name for i in pc.instructions] == ["R", "R", "RX", "H", "CX", "CX", "CZ", "X_ERROR", "Y_ERROR", "Z_ERROR",
                                                 "DEPOLARIZE1", "DEPOLARIZE2", "M", "M", "MX", "MR", "MR", "MRX"]
    assert pc.num_qubits == 4 and pc.num_measurements == 6 and pc.ticks == 1
    assert pc.detectors == [[5, 0]] and pc.observables == {1: [4, 3, 4]}
    assert [i.p for i in pc.instructions[12:16]] == [0.0, 0.01, 0.0, 0.02]
    assert pc.instructions[-1].targets == (1 | qc.INVERT,)
    cc = compile_circuit(pc)
    assert cc.num_qubits == 4 and cc.num_measurements == 6
    assert cc.observables.shape == (2, 6) and cc.observables[1].indices.tolist() == [3]  # rec 4 twice cancels
    assert list(cc.groups) == ["detectors", "observables", "records"]
    names = {v: k for k, v in qc.OPCODES.items()}
    got = [names[o] for o in cc.ops[:, 0]]
    # the implicit reset, R 0 1 + RZ 2 fused, ..., MR = M then R, MRX = MX then RX
    assert got == ["R", "R", "RX", "H", "CX", "CX", "CZ", "X_ERROR", "Y_ERROR", "Z_ERROR", "DEPOLARIZE1",
                   "DEPOLARIZE2", "M", "M", "MX", "M", "R", "M", "R", "MX", "RX"]
    assert np.array_equal(cc.thresholds, qc.bern_threshold(cc.probs))
    assert cc.thresholds[7] == int(0.1 * 2 ** 32) and cc.probs[13] == 0.01
    info = cc.validate()
    assert info["qubits"] == 4 and info["measurements"] == 6 and info["group_rows"] == [1, 2, 6, 0]
    assert info["lds_bytes"] == 16 * 4 + 8 * 6


def test_targets_split_into_disjoint_groups():
    cc = compile_circuit("CX 0 1 2 3 1 2 0 3\nH 0 0\nM 0 1 0")
    ops = [(int(o), cc.targets[a:a + c].tolist()) for o, a, c, _ in cc.ops[1:]]
    assert ops == [(qc.OP_CX, [0, 1, 2, 3]), (qc.OP_CX, [1, 2, 0, 3]), (qc.OP_H, [0]), (qc.OP_H, [0]),
                   (qc.OP_M, [0, 1]), (qc.OP_M, [0])]
    cc.validate()


def test_nested_repeat_resolves_lookbacks_across_the_unrolling():
    text = """
        R 0 1
        M 0
        REPEAT 2 {
            REPEAT 3 {
                M 1
                DETECTOR rec[-1] rec[-2]
            }
            M 0
            DETECTOR rec[-1] rec[-5]
        }
        OBSERVABLE_INCLUDE(0) rec[-9]
    """
    pc = parse(text)
    assert pc.num_measurements == 9
    assert pc.detectors == [[1, 0], [2, 1], [3, 2], [4, 0], [5, 4], [6, 5], [7, 6], [8, 4]]
    assert pc.observables == {0: [0]}


@pytest.mark.parametrize("text", ["S 0", "MY 0", "CX 0 1 2", "DEPOLARIZE2(0.1) 0 1 2", "CZ 3", "X_ERROR 0",
                                  "H(0.1) 0", "M 0\nDETECTOR rec[-2]", "REPEAT 2 {\nM 0", "X_ERROR(1.5) 0"])
def test_parser_refuses(text):
    with pytest.raises(ValueError) as e:
        parse(text)
    if text in ("S 0", "MY 0"):
        assert text.split()[0] in str(e.value) and "DEPOLARIZE2" in str(e.value)  # names it and the supported set


@pytest.mark.parametrize("R", [0, 1, 2, 3])
def test_golden_storage_texts(R):
    cc = compile_circuit(golden_text(R))
    assert cc.num_measurements == R * 216 + 225
    assert cc.observables.shape[0] == 9
    groups = storage_output_groups(cc, 108, 108, 225, R)
    assert groups["syn"].shape == ((R + 1) * 108, cc.num_measurements)
    assert groups["readout"].shape[0] == 225 and groups["readout"].indices.tolist() == list(range(R * 216, R * 216 + 225))
    # round t's Z-sector detectors compare the Z-check records of rounds t and t - 1
    syn = groups["syn"]
    for t in range(R):
        for i in (0, 107):
            want = [216 * t + 108 + i] + ([216 * (t - 1) + 108 + i] if t else [])
            assert sorted(syn[t * 108 + i].indices.tolist()) == sorted(want)
    info = cc.validate()
    assert info["lds_bytes"] == 16 * cc.num_qubits + 8 * cc.num_measurements <= qc.LDS_LIMIT


# ---------------------------------------------------------------- 2. edge colouring
def _irregular(seed=3):
    rng = np.random.default_rng(seed)
    H = (rng.random((23, 41)) < 0.12).astype(np.uint8)
    H[5, :] = 0           # an isolated check
    H[:, 7] = 0
    H[2, :30] = 1         # one heavy row sets Delta
    return sp.csr_matrix(H)


def _colouring_inputs():
    out = []
    for name in ("hgp_12_3_4_s1234", "hgp_24_3_4_s11"):
        hx, hz = load_checks(name)
        out += [(name + "_x", hx), (name + "_z", hz)]
    from exp_ldpc_amd import lifted
    bb = lifted.bivariate_bicycle_code(12, 6, [(3, 0), (0, 1), (0, 2)], [(0, 3), (1, 0), (2, 0)])
    out += [("bb144_x", sp.csr_matrix(bb.checks.x)), ("bb144_z", sp.csr_matrix(bb.checks.z))]
    out.append(("irregular", _irregular()))
    return out


@pytest.mark.parametrize("name,H", _colouring_inputs(), ids=lambda v: v if isinstance(v, str) else "")
def test_edge_colouring_is_proper_with_delta_colours(name, H):
    H = sp.csr_matrix(H)
    delta = max(int(H.sum(axis=0).max()), int(H.sum(axis=1).max()))
    classes = edge_color_bipartite(H)
    assert len(classes) == delta
    edges = Counter(e for c in classes for e in c)
    coo = H.tocoo()
    assert edges == Counter(zip(coo.row.tolist(), coo.col.tolist()))  # every edge exactly once
    for c in classes:
        assert c, "an empty colour class"
        rows, cols = [e[0] for e in c], [e[1] for e in c]
        assert len(set(rows)) == len(rows) and len(set(cols)) == len(cols)


# ---------------------------------------------------------------- 3. generated circuit
NOISE_LINE = ("X_ERROR", "Y_ERROR", "Z_ERROR", "DEPOLARIZE1", "DEPOLARIZE2", "DETECTOR", "OBSERVABLE_INCLUDE",
              "SHIFT_COORDS")


@pytest.mark.parametrize("R", [0, 1, 3])
def test_generated_storage_circuit(code225, R):
    hx, hz = sp.csr_matrix(code225.checks.x), sp.csr_matrix(code225.checks.z)
    targets, lines = storage_circuit_text(R, trivial_noise(), code225)
    # no qubit twice in a tick (annotations and REPEAT lines carry no qubits)
    tick = []
    for line in lines + ["TICK"]:
        tok = line.split()
        if tok[0] == "TICK":
            assert len(tick) == len(set(tick)), line
            tick = []
        elif not tok[0].startswith(NOISE_LINE) and tok[0] not in ("REPEAT", "}"):
            tick += [int(t) for t in tok[1:]]
    pc = parse(lines)
    pairs = Counter()
    for ins in pc.instructions:
        if ins.name in ("CX", "CZ"):
            pairs[ins.name] += len(ins.targets) // 2
    assert pairs["CX"] == R * hx.nnz and pairs["CZ"] == R * hz.nnz
    assert pc.num_measurements == R * 216 + 225 and len(pc.observables) == 9
    from exp_ldpc_amd.experiment import _steps
    body = sum(_steps(code225.checks)) + 2  # per round: a reset tick and Delta layers per sector
    assert pc.ticks == 1 + (body if R else 0) + (1 + (R - 1) * (body + 1) if R > 1 else 0)
    # every CX of a round joins an X ancilla to a qubit of its check
    if R:
        cx = next(i for i in pc.instructions if i.name == "CX").targets
        assert all(hx[a - 225, q] for a, q in zip(cx[0::2], cx[1::2]))
    # the same groups as the reference's text: shapes, and the final detectors' supports
    cc = compile_circuit(pc)
    g = storage_output_groups(cc, 108, 108, 225, R)
    ref = storage_output_groups(compile_circuit(golden_text(R)), 108, 108, 225, R)
    assert (g["syn"] != ref["syn"]).nnz == 0 and (g["readout"] != ref["readout"]).nnz == 0
    L = np.asarray(code225.logicals.z) % 2
    assert np.array_equal(cc.observables.toarray()[:, -225:], L) and cc.observables[:, :-225].nnz == 0
    # the text round-trips through circuit_noise, and the parser accepts the result
    _, noisy = storage_circuit_text(R, circuit_noise(0.1, 0.2), code225)
    pn = parse(noisy)
    assert [i for i in pn.instructions if i.name not in NOISE_LINE] == \
        [type(i)(i.name, 0.2 if i.name in ("M", "MX", "MR", "MRX") else 0.0, i.targets) for i in pc.instructions]
    d2 = sum(len(i.targets) // 2 for i in pn.instructions if i.name == "DEPOLARIZE2")
    assert d2 == R * (hx.nnz + hz.nnz) and all(i.p == 0.1 for i in pn.instructions if i.name.startswith("DEPOL"))
    assert compile_circuit(pn).validate()["measurements"] == pc.num_measurements


def test_storage_sim_builds_its_circuit_lazily(code225, monkeypatch):
    import exp_ldpc_amd.schedule as schedule
    calls = []
    real = schedule.edge_color_bipartite
    monkeypatch.setattr(schedule, "edge_color_bipartite", lambda H: (calls.append(1), real(H))[1])
    sim = build_storage_simulation(1, depolarizing_noise(0.01, 0.01), code225)
    sim.measurement_view(0, False, np.arange(441))
    assert not calls                     # the views and the depolarizing path never colour
    cc = sim.compiled()
    assert calls and list(cc.groups) == ["syn", "readout"]
    assert cc.groups["syn"].shape[0] == 216 and cc.groups["readout"].shape[0] == 225
    assert sim.compiled() is cc and "DEPOLARIZE1(0.01)" in " ".join(sim.circuit)


# ---------------------------------------------------------------- 4. qd_circuit_create_host
def _program(**over):
    """A valid two-qubit program (CX, a noisy M of both) with one group, and overrides."""
    prog = dict(num_qubits=2, ops=[[qc.OP_CX, 0, 2, 0], [qc.OP_DEP1, 2, 1, 0], [qc.OP_M, 3, 2, 0]], targets=[0, 1, 0, 0, 1],
                probs=[0.0, 0.5, 0.25], group_rows=[1], row_ptr=[0, 2], rec_idx=[0, 1])
    prog.update(over)
    return prog


def _rc(prog):
    from exp_ldpc_amd._abi import QdecError
    try:
        h = qc.create_handle(prog["num_qubits"], prog["ops"], prog["targets"], prog["probs"], prog["group_rows"],
                             prog["row_ptr"], prog["rec_idx"], device=None)
    except QdecError as e:
        return e.rc
    qc.destroy_handle(h)
    return 0


def test_create_host_refuses_bad_programs_each_with_its_code():
    assert _rc(_program()) == 0
    assert _rc(_program(targets=[0, 2, 0, 0, 1])) == -72                   # qubit index out of range
    assert _rc(_program(targets=[0, 1, -1, 0, 1])) == -72
    assert _rc(_program(rec_idx=[-1, 1])) == -73                           # a lookback before the start
    assert _rc(_program(rec_idx=[0, 2])) == -73                            # a record not yet measured
    assert _rc(_program(targets=[0, 0, 0, 0, 1])) == -74                   # CX 0 0
    assert _rc(_program(targets=[0, 1, 0, 1, 1])) == -74                   # M 1 1
    assert _rc(_program(probs=[0.0, 1.5, 0.25])) == -75                    # p > 1
    assert _rc(_program(probs=[0.0, 0.5, float("nan")])) == -75
    assert _rc(_program(ops=[[qc.OP_CX, 0, 2, 0], [qc.OP_DEP1, 2, 1, 0], [12, 3, 2, 0]])) == -71
    assert _rc(_program(ops=[[qc.OP_CX, 0, 2, 0], [qc.OP_DEP1, 2, 1, 0], [qc.OP_M, 3, 3, 0]])) == -71
    assert _rc(_program(ops=[[qc.OP_CX, 0, 1, 0], [qc.OP_DEP1, 2, 1, 0], [qc.OP_M, 3, 2, 0]])) == -71  # odd pair
    assert _rc(_program(row_ptr=[1, 2])) == -71
    # over the LDS limit: 16 Q + 8 M > 160 KiB, by qubits and by measurements
    big = qc.LDS_LIMIT // 16 + 1
    assert _rc(dict(num_qubits=big, ops=np.zeros((0, 4)), targets=[], probs=[], group_rows=[], row_ptr=[0],
                    rec_idx=[])) == -76
    assert _rc(dict(num_qubits=big - 1, ops=np.zeros((0, 4)), targets=[], probs=[], group_rows=[], row_ptr=[0],
                    rec_idx=[])) == 0
    nm = (qc.LDS_LIMIT - 16) // 8 + 1
    many = dict(num_qubits=1, ops=[[qc.OP_M, 0, 1, 0]] * nm, targets=[0], probs=[0.0] * nm, group_rows=[],
                row_ptr=[0], rec_idx=[])
    assert _rc(many) == -76
    many["ops"] = many["ops"][:-1]
    many["probs"] = many["probs"][:-1]
    assert _rc(many) == 0


def test_host_handle_cannot_sample():
    from exp_ldpc_amd import _abi
    p = _program()
    h = qc.create_handle(p["num_qubits"], p["ops"], p["targets"], p["probs"], p["group_rows"], p["row_ptr"],
                         p["rec_idx"], device=None)
    assert _abi.load().qd_circuit_sample_device(h, 1, 0, 0, 4, 0, None, None) == -79
    assert _abi.load().qd_circuit_sample_device(h, 1, 0, 0, 0, 0, None, None) == -79
    qc.destroy_handle(h)


# ---------------------------------------------------------------- 5. the model against the DEM
def test_frame_model_matches_the_dem_marginals(code225):
    """2^14 shots of the golden R = 1 text (depolarizing 0.01 / 0.01) from the
    numpy frame model: each of the 216 Z-sector detectors and 9 observables
    fires within 5.5 sigma of its exact marginal under
    dem.storage_experiment_dem (false alarm below 1e-5 over 225 quantities).
    The observables are Lz readout, as the pipelines compute them: the golden
    text's own OBSERVABLE_INCLUDE lines name rec[-225] an even number of times
    each (the reference indexes the logical's row, not its support) and are
    identically 0, which the model reproduces."""
    N = 1 << 14
    cc = compile_circuit(golden_text(1))
    groups = dict(storage_output_groups(cc, 108, 108, 225, 1), observables=cc.observables)
    out = frame_model.sample(cc, 20250221, 0, 0, N, groups=groups)
    assert cc.observables.nnz == 0 and not out["observables"].any()
    H, L = code225.checks.z, np.asarray(code225.logicals.z) % 2
    qd, qo = dem_marginals(H, L, 1, 0.01, 0.01)
    assert qd.size == 216 and qo.size == 9
    obs = (out["readout"].astype(np.int64) @ L.T.astype(np.int64)) % 2
    assert_within_sigmas(np.concatenate([out["syn"].mean(axis=0), obs.mean(axis=0)]), np.concatenate([qd, qo]), N)
    # randomised, as they really are: first-round X-check records and single readout bits
    assert 0.47 < out["rec"][:, :108].mean() < 0.53 and 0.47 < out["readout"][:, 0].mean() < 0.53


def test_generated_circuit_is_noiseless_without_noise(code225):
    """The generated R = 2 circuit under trivial_noise, 192 shots of the model:
    no detector fires (either sector: the colouring's layers commute as they
    must), no observable flips, yet the X-check records are coins."""
    _, lines = storage_circuit_text(2, trivial_noise(), code225)
    cc = compile_circuit(lines)
    out = frame_model.sample(cc, 11, 0, 0, 192)
    assert out["detectors"].shape == (192, 432) and not out["detectors"].any()
    assert out["observables"].shape == (192, 9) and not out["observables"].any()
    assert 0.45 < out["records"][:, :108].mean() < 0.55
