"""Host side of PAULI_CHANNEL_1 / PAULI_CHANNEL_2: the parser and compiler, the
library's validation through qd_circuit_create_host_args, the stand-alone
validator program under ASan + UBSan, the exact decomposition into independent
mechanisms (dem.pauli_channel_components), DEM equalities with the channels they
specialise to, and the numpy frame model against the DEM's exact marginals."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import fault_model
import fault_model_channels as fmc
import frame_model_channels as frc
from test_circuit_dem_host import marginals
from test_circuit_host import assert_within_sigmas
from exp_ldpc_amd import _abi
from exp_ldpc_amd import circuit as qc
from exp_ldpc_amd.circuit import compile_circuit, parse
from exp_ldpc_amd.dem import (dem_from_symptoms, depolarize1_component, depolarize2_component, fault_mechanisms,
                              pauli_channel_components)
from exp_ldpc_amd.noise_model import biased_channel_1, biased_channel_2, biased_circuit_noise

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PC1_ARGS = (0.02, 0.05, 0.11)
# a_k = 0.004 k, the other unequal example, has no exact decomposition (q_IX = -0.024): it serves the bit-for-bit
# tests; the fit against exact marginals takes a_k = 0.01 + 0.002 k (sum 0.39), which has one
PC2_SKEW = tuple(0.004 * k for k in range(1, 16))
PC2_ARGS = tuple(0.01 + 0.002 * k for k in range(1, 16))


def _fmt(a):
    return ", ".join(repr(float(v)) for v in a)


# Two Bell pairs (0, 1) and (2, 3): Z0 Z1, X0 X1, Z2 Z3, X2 X3 are deterministic, and ancillas 4 .. 7 read them (in Z:
# 4 and 6, in X: 5 and 7), so an X on data qubit 0 flips detector 0, a Z detector 1, a Y both; likewise 2 -> detectors
# 2, 3.  Round 1 follows PAULI_CHANNEL_1 on 0 and 2, round 2 (detectors 4 .. 7, against round 1) PAULI_CHANNEL_2 on
# the pair: each of the 3 and each of the 15 outcomes flips its own detector set.
_READ = """
    CX 0 4 2 6
    CX 1 4 3 6
    CX 5 0 7 2
    CX 5 1 7 3
    MR 4 6
    MRX 5 7
"""
FIT_TOY = f"""
    RX 0 2
    R 1 3 4 6
    RX 5 7
    CX 0 1 2 3
    PAULI_CHANNEL_1({_fmt(PC1_ARGS)}) 0 2
    {_READ}
    DETECTOR rec[-4]
    DETECTOR rec[-2]
    DETECTOR rec[-3]
    DETECTOR rec[-1]
    PAULI_CHANNEL_2({_fmt(PC2_ARGS)}) 0 2
    {_READ}
    DETECTOR rec[-4] rec[-8]
    DETECTOR rec[-2] rec[-6]
    DETECTOR rec[-3] rec[-7]
    DETECTOR rec[-1] rec[-5]
    OBSERVABLE_INCLUDE(0) rec[-4] rec[-1]
    OBSERVABLE_INCLUDE(1) rec[-8] rec[-2]
"""


# ---------------------------------------------------------------- 1. parser / compiler
def test_parser_and_compiler_take_the_channels():
    text = f"PAULI_CHANNEL_1({_fmt(PC1_ARGS)}) 0 1 0\nX_ERROR(0.1) 1\nPAULI_CHANNEL_2({_fmt(PC2_SKEW)}) 0 1 2 0\nM 0 1 2"
    pc = parse(text)
    assert [i.name for i in pc.instructions] == ["PAULI_CHANNEL_1", "X_ERROR", "PAULI_CHANNEL_2", "M"]
    assert pc.instructions[0].args == PC1_ARGS and pc.instructions[1].args == () and pc.instructions[3].args == ()
    assert pc.instructions[2].args == PC2_SKEW and pc.instructions[2].targets == (0, 1, 2, 0)
    assert {"PAULI_CHANNEL_1", "PAULI_CHANNEL_2"} <= set(qc.SUPPORTED)
    cc = compile_circuit(text)
    assert cc.ops[:, 0].tolist() == [qc.OP_R, qc.OP_PC1, qc.OP_XERR, qc.OP_PC2, qc.OP_M] == [3, 12, 7, 13, 5]
    assert cc.ops[:, 3].tolist() == [0, 0, 0, 3, 0], "the first argument; 0 for the instructions that take none"
    assert cc.args.dtype == np.float64 and cc.args.tolist() == list(PC1_ARGS + PC2_SKEW)
    c1 = (0.02 + 0.05) + 0.11                       # c_k = c_{k-1} + a_k, left to right
    c2 = 0.0
    for a in PC2_SKEW:
        c2 = c2 + a
    assert cc.probs.tolist() == [0.0, c1, 0.1, c2, 0.0]
    assert np.array_equal(cc.thresholds, qc.bern_threshold(cc.probs))
    again = cc.with_groups({"records": cc.record_rows()})
    assert again.args is cc.args and again.ops is cc.ops
    info = cc.validate()
    assert info["sites"] == 4 + 4 + 4 + 4 and info["instructions"] == 5


@pytest.mark.parametrize("text, match", [
    ("PAULI_CHANNEL_1(0.1, 0.1) 0", "takes 3"),
    ("PAULI_CHANNEL_1(0.1, 0.1, 0.1, 0.1) 0", "takes 3"),
    ("PAULI_CHANNEL_2(" + ", ".join(["0.01"] * 14) + ") 0 1", "takes 15"),
    ("PAULI_CHANNEL_2(" + ", ".join(["0.01"] * 16) + ") 0 1", "takes 15"),
    ("PAULI_CHANNEL_1 0", "takes 3"),
    ("PAULI_CHANNEL_1(0.1, -0.1, 0.1) 0", "outside"),
    ("PAULI_CHANNEL_2(" + ", ".join(["0.01"] * 14 + ["-0.01"]) + ") 0 1", "outside"),
    ("PAULI_CHANNEL_1(0.5, 0.3, 0.2001) 0", "sum"),
    ("PAULI_CHANNEL_2(" + ", ".join(["0.0625"] * 14 + ["0.1251"]) + ") 0 1", "sum"),
    ("PAULI_CHANNEL_2(" + ", ".join(["0.01"] * 15) + ") 0 1 2", "odd"),
    ("PAULI_CHANNEL_1(0.1, x, 0.1) 0", "bad probability"),
])
def test_parser_refuses(text, match):
    with pytest.raises(ValueError, match=match):
        parse(text)


def test_correlated_errors_stay_unsupported():
    with pytest.raises(ValueError, match=r"unsupported instruction 'E'.*supported: .*PAULI_CHANNEL_1, PAULI_CHANNEL_2"):
        parse("E(0.1) X0")
    for line in ("CORRELATED_ERROR(0.1) X0", "ELSE_CORRELATED_ERROR(0.1) Z1", "S 0", "MY 0"):
        with pytest.raises(ValueError, match="unsupported instruction"):
            parse(line)


def test_a_total_of_one_rounded_above_one_is_taken():
    """Fifteen decimals of sum 1 that add up to 1 + 2^-52 left to right: inside
    the parser's and the validator's 1e-12, threshold 2^32 - 1."""
    a = [0.111, 0.055, 0.033, 0.094, 0.099, 0.001, 0.08, 0.011, 0.014, 0.106, 0.005, 0.029, 0.119, 0.051, 0.192]
    cc = compile_circuit("PAULI_CHANNEL_2(" + _fmt(a) + ") 0 1\nM 0 1")
    assert cc.probs[1] > 1.0 and cc.thresholds[1] == 0xFFFFFFFF
    assert cc.validate()["sites"] == 8


# ---------------------------------------------------------------- 2. the library's validation
def _create(ops, targets, probs, args, Q=3, entry="qd_circuit_create_host_args", place=0):
    """(code, info) of a raw program with one group: record 0."""
    lib = _abi.load()
    ops = np.ascontiguousarray(ops, np.int32).reshape(-1, 4)
    targets, probs = np.ascontiguousarray(targets, np.int32), np.ascontiguousarray(probs, np.float64)
    rows, ptr, idx = (np.ascontiguousarray(a, np.int32) for a in ([1], [0, 1], [0]))
    h = C.c_void_p()
    head = (Q, ops.shape[0], _abi.ptr(ops), targets.size, _abi.ptr(targets), _abi.ptr(probs), 1, _abi.ptr(rows),
            _abi.ptr(ptr), _abi.ptr(idx))
    if entry == "qd_circuit_create_host_args":
        args = np.ascontiguousarray(args, np.float64)
        rc = lib.qd_circuit_create_host_args(place, *head, args.size, _abi.ptr(args), C.byref(h))
    elif entry == "qd_circuit_create_host_placed":
        rc = lib.qd_circuit_create_host_placed(place, *head, C.byref(h))
    else:
        rc = lib.qd_circuit_create_host(*head, C.byref(h))
    if rc != 0:
        assert not h.value
        return rc, None
    info = dict(qc.handle_info(h), faults=qc.handle_fault_info(h), dup=qc.handle_op_flags(h).tolist())
    qc.destroy_handle(h)
    return 0, info


def _program(n1=3, n2=2):
    """PAULI_CHANNEL_1 on n1 targets, PAULI_CHANNEL_2 on n2 pairs (qubits 0, 1 in turn), M 0."""
    t1 = [e % 3 for e in range(n1)]
    t2 = [v for e in range(n2) for v in (e % 2, 2)]
    ops = [12, 0, n1, 0, 13, n1, 2 * n2, 3, 5, n1 + 2 * n2, 1, 0]
    args = list(PC1_ARGS + PC2_SKEW)
    return ops, t1 + t2 + [0], [sum(PC1_ARGS), float(np.cumsum(PC2_SKEW)[-1]), 0.0], args


def test_validator_counts_sites_faults_and_dup():
    for n in (1, 3, 4, 5):
        ops, tg, probs, args = _program(n, n)
        # left-to-right sums, as the compiler makes them
        probs[0], probs[1] = (0.02 + 0.05) + 0.11, float(np.add.accumulate(np.asarray(PC2_SKEW))[-1])
        rc, info = _create(ops, tg, probs, args)
        assert rc == 0, n
        assert info["sites"] == 2 * ((n + 3) // 4 * 4) + 4, n          # each instruction from a multiple of 4
        assert info["faults"] == (2 * n + 4 * n + 1, 1), n              # X, Z per target; X_a, Z_a, X_b, Z_b per pair
        assert info["dup"] == [int(n > 3), int(n > 1), 0], n           # a qubit twice / qubit 2 in two pairs
    # the fault table numbers them as DEPOLARIZE1 / DEPOLARIZE2
    cc = compile_circuit(f"PAULI_CHANNEL_1({_fmt(PC1_ARGS)}) 0 1\nPAULI_CHANNEL_2({_fmt(PC2_SKEW)}) 0 1\nM 0")
    twin = compile_circuit("DEPOLARIZE1(0.1) 0 1\nDEPOLARIZE2(0.1) 0 1\nM 0")
    for kind in (0, 1):
        for a, b in zip(cc.fault_table(kind), twin.fault_table(kind)):
            assert np.array_equal(a, b)
    assert cc.fault_table(0)[2].tolist() == [1, 2, 1, 2] + [1, 2, 1, 2] + [4]
    want = [(i, t, c) for i, t, c in fmc.enumerate_faults(cc.ops)]
    assert [tuple(int(v[f]) for v in cc.fault_table(0)) for f in range(9)] == want


def test_validator_error_codes():
    ops, tg, probs, args = _program()
    probs[0], probs[1] = (0.02 + 0.05) + 0.11, float(np.add.accumulate(np.asarray(PC2_SKEW))[-1])
    assert _create(ops, tg, probs, args)[0] == 0

    def changed(**kw):
        o, t, p, a = list(ops), list(tg), list(probs), list(args)
        for k, v in kw.get("ops", {}).items():
            o[k] = v
        for k, v in kw.get("probs", {}).items():
            p[k] = v
        for k, v in kw.get("args", {}).items():
            a[k] = v
        return _create(o, t, p, kw.get("all_args", a))[0]
    assert changed(ops={7: 4}) == -71, "15 arguments from 4 on end one past the array"
    assert changed(ops={7: 18}) == -71 and changed(ops={3: -1}) == -71 and changed(ops={3: 2 ** 31 - 1}) == -71
    assert changed(ops={3: 16}) == -71, "3 arguments from 16 on end one past the array"
    assert changed(all_args=[]) == -71
    assert changed(ops={11: 1}) == -71, "an argument offset on a measurement"
    assert changed(args={1: -0.05}, probs={0: 0.08}) == -75
    assert changed(args={4: 1.5}) == -75 and changed(args={4: float("nan")}) == -75
    assert changed(args={2: 0.9301}, probs={0: 1.0001}) == -75, "a sum of 1.0001"
    assert changed(probs={1: probs[1] + 1e-9}) == -75 and changed(probs={0: 0.0}) == -75
    assert changed(probs={0: probs[0] + 1e-13}) == 0, "within 1e-12 of the sum"
    assert changed(ops={6: 3}) == -71, "an odd target count of PAULI_CHANNEL_2"
    # ops[:, 3] is 0 for every instruction without arguments, under every entry point
    old = ([1, 0, 2, 0, 10, 0, 2, 0, 5, 0, 1, 0], [0, 1], [0.0, 0.1, 0.0])
    for entry in ("qd_circuit_create_host_args", "qd_circuit_create_host_placed", "qd_circuit_create_host"):
        assert _create(*old, [], entry=entry)[0] == 0
        for i in range(3):
            bad = list(old[0])
            bad[4 * i + 3] = 1
            assert _create(bad, old[1], old[2], [0.0] * 20, entry=entry)[0] == -71, (entry, i)
    # the entry points without an argument array do not know the new opcodes
    for entry in ("qd_circuit_create_host_placed", "qd_circuit_create_host"):
        assert _create(ops, tg, probs, args, entry=entry)[0] == -71
        assert _create([12, 0, 1, 0, 5, 0, 1, 0], [0], [0.0, 0.0], [], entry=entry)[0] == -71
    lib = _abi.load()
    h = C.c_void_p()
    assert lib.qd_circuit_create_host_args(0, 1, 0, None, 0, None, None, 0, None, None, None, -1, None, C.byref(h)) == -71
    assert lib.qd_circuit_create_host_args(7, 1, 0, None, 0, None, None, 0, None, None, None, 0, None, C.byref(h)) == -96
    assert lib.qd_circuit_create_host_args(0, 1, 0, None, 0, None, None, 0, None, None, None, 2, None, C.byref(h)) == -71


def test_create_handle_uses_the_new_entry_points_only_for_channels(monkeypatch):
    calls = []
    lib = _abi.load()

    class Spy:
        def __getattr__(self, name):
            if name.startswith("qd_circuit_create"):
                calls.append(name)
            return getattr(lib, name)
    monkeypatch.setattr(_abi, "load", lambda: Spy())
    compile_circuit("DEPOLARIZE1(0.1) 0\nM 0").validate()
    compile_circuit(f"PAULI_CHANNEL_1({_fmt(PC1_ARGS)}) 0\nM 0").validate()
    assert calls == ["qd_circuit_create_host_placed", "qd_circuit_create_host_args"]


# ---------------------------------------------------------------- 3. the validator alone, under sanitizers
def test_validator_program_is_clean_under_sanitizers(tmp_path):
    """tools/circuit_check.cpp with qdec_circuit.cpp and qdec_tables.cpp, no HIP
    header, a static ASan + UBSan runtime: an ordinary child process.  Its arrays
    are sized exactly, so a read of an argument the validator should have refused
    first is a report.  Exit 0: every case gave its code."""
    from exp_ldpc_amd import build
    from test_tables_standalone import SAN_FLAGS
    cxx = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(build._hipcc()))), "lib", "llvm", "bin", "clang++")
    assert os.path.exists(cxx), f"ROCm's clang++ not found at {cxx}"
    exe = str(tmp_path / "circuit_check")
    res = subprocess.run([cxx, *SAN_FLAGS, os.path.join(REPO, "tools", "circuit_check.cpp"),
                          os.path.join(build.CSRC, "qdec_circuit.cpp"), os.path.join(build.CSRC, "qdec_tables.cpp"),
                          "-o", exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0 and res.stderr == "", f"exit {res.returncode}\n{res.stdout}\n{res.stderr[-4000:]}"
    got = dict(line.split(None, 1) for line in res.stdout.splitlines())
    assert got["channels"] == "0" and got["channel_faults"] == "17 3"
    for case in ("arg_range_across_end", "arg_range_behind_end", "arg_range_negative", "arg_range_overflow",
                 "arg_array_empty", "arg_offset_on_measurement", "arg_offset_on_gate", "channels_without_array"):
        assert got[case] == "-71", case
    for case in ("arg_negative", "arg_above_one", "arg_sum_above_one", "probability_is_not_the_sum"):
        assert got[case] == "-75", case


# ---------------------------------------------------------------- 4. the decomposition
def test_components_equal_the_depolarizing_closed_forms():
    """Both are 1/2 - 1/2 x with x near 1: a few ulp of 1/2 (1.1e-16) apart."""
    for p in (1e-4, 0.003, 0.01, 0.1, 0.3, 0.7):
        assert np.abs(pauli_channel_components([p / 3] * 3) - depolarize1_component(p)).max() <= 4e-16
        assert np.abs(pauli_channel_components([p / 15] * 15) - depolarize2_component(p)).max() <= 4e-16
        assert np.abs(np.asarray(fmc.components([p / 3] * 3)) - fault_model.q1(p)).max() <= 4e-16
        assert np.abs(np.asarray(fmc.components([p / 15] * 15)) - fault_model.q2(p)).max() <= 4e-16


@pytest.mark.parametrize("args", [PC1_ARGS, PC2_ARGS, biased_channel_1(0.1, 30.0)] +
                         [biased_channel_2(0.01, eta) for eta in (0.5, 10.0, 1e4)] +
                         [biased_channel_2(0.1, eta) for eta in (0.5, 10.0, 1e4)])
def test_components_compose_back_to_the_channel(args):
    q = pauli_channel_components(args)
    assert (q >= 0).all() and np.abs(q - np.asarray(fmc.components(args))).max() <= 4e-16
    dist = fmc.compose(q.tolist())
    err = np.abs(np.asarray(dist[1:]) - np.asarray(args)).max()
    print("largest error of the composed distribution", err)
    assert err <= 1e-15 and abs(dist[0] - (1 - sum(args))) <= 1e-15


def test_biased_channels():
    assert np.allclose(biased_channel_1(0.03, 0.5), [0.01] * 3, rtol=0, atol=1e-17)
    assert np.allclose(biased_channel_2(0.03, 0.5), [0.002] * 15, rtol=0, atol=1e-17)
    one, two = biased_channel_1(0.03, 1e9), biased_channel_2(0.03, 1e9)
    assert abs(one[2] - 0.03) < 1e-10 and max(one[:2]) < 1e-10
    assert all(abs(two[k - 1] - 0.01) < 1e-10 for k in (3, 12, 15)) and sum(two) == pytest.approx(0.03, abs=1e-15)
    for p in (1e-4, 0.01, 0.1):
        for eta in (0.5, 1.0, 3.0, 100.0, 1e4):
            pauli_channel_components(biased_channel_1(p, eta))
            pauli_channel_components(biased_channel_2(p, eta))
    with pytest.raises(ValueError):
        biased_circuit_noise(0.01, 0.0)


def test_channels_without_a_decomposition():
    rng = np.random.default_rng(7)
    v = rng.random(15)
    v = (0.2 * v / v.sum()).tolist()
    for args in ([0.1, 0.0, 0.1], v):
        with pytest.raises(ValueError, match="no decomposition"):
            pauli_channel_components(args)
        with pytest.raises(ValueError, match="no decomposition"):
            fmc.components(args)
        assert pauli_channel_components(args, approximate_disjoint_errors=True).tolist() == list(args)
    assert pauli_channel_components([0.1, 0.0, 0.1], True)[1] == 0.0
    q = fmc.components([0.1, 0.0, 0.1], approximate=True)
    assert q == [0.1, 0.0, 0.1]
    assert abs(-0.0164 - (0.5 - 0.5 * np.exp(-0.5 * (np.log(0.6) - 2 * np.log(0.8))))) < 1e-4   # q_Y
    cc = compile_circuit("PAULI_CHANNEL_1(0.1, 0, 0.1) 0 1\nM 0 1\nDETECTOR rec[-1]")
    with pytest.raises(ValueError, match=r"PAULI_CHANNEL_1\(0.1, 0.0, 0.1\) \(instruction 1\)"):
        fault_mechanisms(cc)
    probs, members = fault_mechanisms(cc, approximate_disjoint_errors=True)
    assert probs.tolist() == [0.1, 0.1] * 2 and members.tolist() == [[0, -1, -1, -1], [1, -1, -1, -1],
                                                                      [2, -1, -1, -1], [3, -1, -1, -1]]


# ---------------------------------------------------------------- 5. DEM equalities
def _dem(text, **kw):
    cc = compile_circuit(text)
    s = fmc.symptoms(cc, 0)
    return cc, dem_from_symptoms(cc, s["detectors"], s["observables"], **kw)


def _bell_toy(noise):
    return FIT_TOY.replace(f"PAULI_CHANNEL_1({_fmt(PC1_ARGS)}) 0 2", noise[0]).replace(
        f"PAULI_CHANNEL_2({_fmt(PC2_ARGS)}) 0 2", noise[1])


def _same_dem(a, b, exact=False):
    ea, eb = [i for i in a if i.type == "error"], [i for i in b if i.type == "error"]
    assert len(ea) == len(eb) and len(ea) > 0
    for x, y in zip(ea, eb):
        assert (x.detectors, x.observables) == (y.detectors, y.observables)
        assert abs(x.args[0] - y.args[0]) <= (0 if exact else 1e-12)


def test_dem_equalities():
    p = 0.09
    third, fifteenth = _fmt([p / 3] * 3), _fmt([p / 15] * 15)
    _, z = _dem(_bell_toy((f"Z_ERROR({p}) 0 2", f"DEPOLARIZE2({p}) 0 2")))
    _, pz = _dem(_bell_toy((f"PAULI_CHANNEL_1(0, 0, {p}) 0 2", f"DEPOLARIZE2({p}) 0 2")))
    _same_dem(pz, z)
    _, d = _dem(_bell_toy((f"DEPOLARIZE1({p}) 0 2", f"DEPOLARIZE2({p}) 0 2")))
    _, c1 = _dem(_bell_toy((f"PAULI_CHANNEL_1({third}) 0 2", f"DEPOLARIZE2({p}) 0 2")))
    _same_dem(c1, d)
    cc, c2 = _dem(_bell_toy((f"DEPOLARIZE1({p}) 0 2", f"PAULI_CHANNEL_2({fifteenth}) 0 2")))
    _same_dem(c2, d)
    assert d.num_errors == 3 + 3 + 15 and z.num_errors == 1 + 1 + 15
    # dem.py's columns are the model's
    cols = fmc.dem_columns(cc)
    assert [(tuple(i.detectors), tuple(i.observables)) for i in c2 if i.type == "error"] == [c[1:] for c in cols]
    assert np.abs(np.array([i.args[0] for i in c2 if i.type == "error"]) - np.array([c[0] for c in cols])).max() <= 1e-15


def test_the_fit_toy_separates_every_outcome():
    cc, dem = _dem(FIT_TOY)
    errs = [i for i in dem if i.type == "error"]
    assert len(errs) == 3 + 3 + 15 and len({(tuple(i.detectors), tuple(i.observables)) for i in errs}) == 21
    assert [i.detectors for i in errs[:6]] == [[0], [0, 1], [1], [2], [2, 3], [3]]
    got = sorted(tuple(i.detectors) for i in errs[6:])
    want = sorted(tuple(4 + k for k in (0, 1, 2, 3) if (m >> k) & 1) for m in range(1, 16))
    assert got == want
    q1s, q2s = pauli_channel_components(PC1_ARGS), pauli_channel_components(PC2_ARGS)
    assert [i.args[0] for i in errs] == q1s.tolist() * 2 + q2s.tolist()
    cols = fmc.dem_columns(cc)
    assert [(tuple(i.detectors), tuple(i.observables)) for i in errs] == [c[1:] for c in cols]
    assert np.abs(np.array([i.args[0] for i in errs]) - np.array([c[0] for c in cols])).max() <= 1e-15
    # no gauge fault reaches a detector or an observable
    g = fmc.symptoms(cc, 1)
    assert g["rec"].shape[0] == 8 + 8 + 2 * (4 + 4) and not g["detectors"].any() and not g["observables"].any()


def test_frame_model_fits_the_dem_marginals():
    """2^16 model shots of FIT_TOY, seed 20250221: the 8 detectors and 2
    observables within 5.5 sigma of the DEM's exact marginals (false alarm below
    1e-6 over 10 quantities).  The marginals are those of the channels themselves:
    detector 1, say, fires with py + pz.  Largest deviation with this seed: 1.62
    sigma."""
    cc, dem = _dem(FIT_TOY)
    q = marginals(dem, 8, 2)
    px, py, pz = PC1_ARGS
    assert np.abs(q[:4] - np.array([px + py, py + pz] * 2)).max() <= 1e-15
    a = np.asarray((0.0,) + PC2_ARGS)
    x0 = sum(a[c] for c in range(16) if (c >> 2) in (1, 2))
    assert abs(q[4] - x0) <= 1e-15
    N = 1 << 16
    s = frc.sample(cc, 20250221, 0, 0, N)
    freq = np.concatenate([s["detectors"].mean(axis=0), s["observables"].mean(axis=0)])
    assert_within_sigmas(freq, q, N)
