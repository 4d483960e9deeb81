"""Frame placement of compiled circuits on host-only handles
(qd_circuit_create_host_placed, qd_circuit_frame_info, qd_circuit_op_flags_copy):
programs beyond the LDS kernels' 160 KiB pass under "hbm" and "auto", every bad
program keeps its code, and noise lines that name a qubit twice are marked."""
import numpy as np
import pytest

import exp_ldpc_amd.circuit as qc
from conftest import load_checks, load_logicals
from test_circuit_host import _program


def _make(prog, frame):
    return qc.create_handle(prog["num_qubits"], prog["ops"], prog["targets"], prog["probs"], prog["group_rows"],
                            prog["row_ptr"], prog["rec_idx"], device=None, frame=frame)


def _rc(prog, frame):
    from exp_ldpc_amd._abi import QdecError
    try:
        h = _make(prog, frame)
    except QdecError as e:
        return e.rc
    qc.destroy_handle(h)
    return 0


def _over_limit():
    """The two over-limit programs of test_create_host_refuses_bad_programs_each_with_its_code."""
    big = qc.LDS_LIMIT // 16 + 1
    nm = (qc.LDS_LIMIT - 16) // 8 + 1
    return [dict(num_qubits=big, ops=np.zeros((0, 4)), targets=[], probs=[], group_rows=[], row_ptr=[0], rec_idx=[]),
            dict(num_qubits=1, ops=[[qc.OP_M, 0, 1, 0]] * nm, targets=[0], probs=[0.0] * nm, group_rows=[],
                 row_ptr=[0], rec_idx=[])], [(big, 0), (1, nm)]


def test_over_limit_programs_pass_under_hbm_and_auto_only():
    progs, sizes = _over_limit()
    for prog, (Q, M) in zip(progs, sizes):
        assert 16 * Q + 8 * M > qc.LDS_LIMIT
        assert _rc(prog, "lds") == -76
        for frame in ("auto", "hbm"):
            h = _make(prog, frame)
            info, fi = qc.handle_info(h), qc.handle_frame_info(h)
            qc.destroy_handle(h)
            assert info["qubits"] == Q and info["measurements"] == M and info["lds_bytes"] == 16 * Q + 8 * M
            assert fi == {"placement": "hbm", "slot_bytes": 16 * Q + 8 * M, "slots": 0, "scratch_bytes": 0}


def test_auto_keeps_a_small_program_in_lds_and_hbm_can_be_forced():
    for frame, want in (("auto", "lds"), ("lds", "lds"), ("hbm", "hbm")):
        h = _make(_program(), frame)
        fi = qc.handle_frame_info(h)
        qc.destroy_handle(h)
        assert fi["placement"] == want and fi["slot_bytes"] == 16 * 2 + 8 * 2


def test_unknown_placement_and_slot_counts_have_their_codes():
    from exp_ldpc_amd import _abi
    assert _rc(_program(), 3) == -96 and _rc(_program(), -1) == -96
    assert _rc(_program(targets=[0, 2, 0, 0, 1]), 3) == -96       # refused before the program is looked at
    h = _make(_program(), "hbm")
    lib = _abi.load()
    assert lib.qd_circuit_set_frame_slots(h, -1) == -98
    assert lib.qd_circuit_set_frame_slots(h, 3) == 0 and lib.qd_circuit_set_frame_slots(h, 0) == 0
    assert lib.qd_circuit_frame_info(h, None) == -71 and lib.qd_circuit_set_frame_slots(None, 1) == -71
    assert lib.qd_circuit_sample_device(h, 1, 0, 0, 4, 0, None, None) == -79      # still host-only
    qc.destroy_handle(h)


@pytest.mark.parametrize("frame", ["hbm", "auto"])
def test_bad_programs_keep_their_codes_under_every_placement(frame):
    assert _rc(_program(), frame) == 0
    assert _rc(_program(targets=[0, 2, 0, 0, 1]), frame) == -72
    assert _rc(_program(targets=[0, 1, -1, 0, 1]), frame) == -72
    assert _rc(_program(rec_idx=[-1, 1]), frame) == -73
    assert _rc(_program(rec_idx=[0, 2]), frame) == -73
    assert _rc(_program(targets=[0, 0, 0, 0, 1]), frame) == -74
    assert _rc(_program(targets=[0, 1, 0, 1, 1]), frame) == -74
    assert _rc(_program(probs=[0.0, 1.5, 0.25]), frame) == -75
    assert _rc(_program(probs=[0.0, 0.5, float("nan")]), frame) == -75
    assert _rc(_program(ops=[[qc.OP_CX, 0, 2, 0], [qc.OP_DEP1, 2, 1, 0], [12, 3, 2, 0]]), frame) == -71
    assert _rc(_program(ops=[[qc.OP_CX, 0, 2, 0], [qc.OP_DEP1, 2, 1, 0], [qc.OP_M, 3, 3, 0]]), frame) == -71
    assert _rc(_program(ops=[[qc.OP_CX, 0, 1, 0], [qc.OP_DEP1, 2, 1, 0], [qc.OP_M, 3, 2, 0]]), frame) == -71
    assert _rc(_program(row_ptr=[1, 2]), frame) == -71


def test_noise_lines_with_repeated_targets_are_marked_and_keep_their_sites():
    """X_ERROR 0 1 0 and a DEPOLARIZE2 whose pairs share a qubit are marked, the
    same lines without the repeat are not, and the repeat costs no site: sites
    count targets (pairs), each instruction rounded up to a multiple of 4."""
    text = """
        R 0 1 2 3
        X_ERROR(0.1) 0 1 0
        X_ERROR(0.1) 0 1 2
        DEPOLARIZE2(0.1) 0 1 2 3 1 0
        DEPOLARIZE2(0.1) 0 1 2 3
        DEPOLARIZE1(0.1) 3 3
        DEPOLARIZE1(0.1) 3 2
        M(0.1) 0 1 2 3
    """
    cc = qc.compile_circuit(text)
    h = cc._create(None, "hbm")
    flags, info = qc.handle_op_flags(h), qc.handle_info(h)
    qc.destroy_handle(h)
    names = [int(o) for o in cc.ops[:, 0]]
    assert names == [qc.OP_R, qc.OP_R, qc.OP_XERR, qc.OP_XERR, qc.OP_DEP2, qc.OP_DEP2, qc.OP_DEP1, qc.OP_DEP1, qc.OP_M]
    assert flags.tolist() == [0, 0, 1, 0, 1, 0, 1, 0, 0]
    assert info["sites"] == 4 + 4 + 4 + 4 + 4 + 4 + 4
    # the toy of the device tests: exactly its two repeating lines
    from test_gpu_circuit import TOYS
    toy = qc.compile_circuit(TOYS["all_ops"])
    h = toy._create(None, "auto")
    flags = qc.handle_op_flags(h)
    qc.destroy_handle(h)
    marked = [(int(toy.ops[i, 0]), toy.targets[toy.ops[i, 1]:toy.ops[i, 1] + toy.ops[i, 2]].tolist())
              for i in np.nonzero(flags)[0]]
    assert marked == [(qc.OP_XERR, [0, 1, 0]), (qc.OP_DEP2, [0, 1, 2, 3, 4, 5, 1, 0])]


@pytest.fixture(scope="module")
def hgp10k_code():
    from exp_ldpc_amd.codes import QuantumCode, QuantumCodeChecks, QuantumCodeLogicals
    hx, hz = load_checks("hgp_80_3_4_s2025")
    lx, lz = load_logicals("hgp_80_3_4_s2025")
    return QuantumCode(QuantumCodeChecks(hx, hz), QuantumCodeLogicals(lx, lz))


def test_the_n10k_circuit_validates_under_auto(hgp10k_code):
    """circuit_noise at R = 1 on the n = 10^4 code: Q = M = 19,600, 470,400 B per
    64 shots, refused by the LDS placement and placed in HBM by "auto"."""
    from exp_ldpc_amd._abi import QdecError
    from exp_ldpc_amd.noise_model import circuit_noise
    from exp_ldpc_amd.storage_sim import build_storage_simulation
    cc = build_storage_simulation(1, circuit_noise(0.001), hgp10k_code).compiled()
    info = cc.validate()                       # frame="auto"
    assert info["qubits"] == 19600 and info["measurements"] == 19600 and info["lds_bytes"] == 470400
    fi = cc.frame_info()
    assert fi["placement"] == "hbm" and fi["slot_bytes"] == 470400
    with pytest.raises(QdecError) as e:
        cc.validate(frame="lds")
    assert e.value.rc == -76
    with pytest.raises(QdecError):
        cc.validate(frame=None)                # the unplaced entry point refuses it as before
    h = cc._create(None, "auto")
    assert not qc.handle_op_flags(h).any()     # the generated circuit names no qubit twice in a noise line
    qc.destroy_handle(h)
