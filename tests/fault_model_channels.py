"""Numpy model of fault propagation and DEM composition with PAULI_CHANNEL_1 /
PAULI_CHANNEL_2, for the tests.  Extends tests/fault_model.py by the ABI's
statement (include/qdec.h, "Fault propagation") and the decomposition rule:

* elementary faults: PAULI_CHANNEL_1 is numbered exactly as DEPOLARIZE1 (two per
  target: X, Z), PAULI_CHANNEL_2 exactly as DEPOLARIZE2 (four per pair: X_a, Z_a,
  X_b, Z_b); no gauge faults.  So propagation is fault_model's on a program whose
  channel opcodes are replaced by the depolarizing ones;
* mechanisms: the members of DEPOLARIZE1 / 2 (Pauli 1 .. 3 on the target, code
  1 .. 15 on the pair), the probability of Pauli P being
    q_P = 1/2 - 1/2 exp(-(2 / 4^n) sum_{Q != I} chi(P, Q) ln lambda_Q),
    lambda_Q = sum_P p_P chi(P, Q), p_I = 1 - sum p, chi = +1 when P and Q commute
    and -1 when they anticommute, n = 1 or 2;
  a q_P in (-1e-15, 0) counts as 0; a component with q_P = 0 is no mechanism; a
  lambda_Q <= 0 or a q_P <= -1e-15 means the channel has no such decomposition
  (ValueError, or with `approximate` the arguments themselves).
"""
import math

import numpy as np

import fault_model
from fault_model import DEP1, DEP2, M, MX, XERR, YERR, ZERR, _PAULI, merge, q1, q2

PC1, PC2 = 12, 13
_XZ = {0: (0, 0), 1: (1, 0), 2: (1, 1), 3: (0, 1)}      # Pauli -> (x, z)


def _as_depolarizing(ops):
    ops = np.array(ops, dtype=np.int64).reshape(-1, 4)
    ops[ops[:, 0] == PC1, 0] = DEP1
    ops[ops[:, 0] == PC2, 0] = DEP2
    return ops


def enumerate_faults(ops, kind=0):
    return fault_model.enumerate_faults(_as_depolarizing(ops), kind)


def propagate(num_qubits, ops, targets, kind=0):
    return fault_model.propagate(num_qubits, _as_depolarizing(ops), targets, kind)


def symptoms(cc, kind=0, groups=None):
    """fault_model.symptoms of a CompiledCircuit that may hold channel instructions."""
    import types
    twin = types.SimpleNamespace(num_qubits=cc.num_qubits, ops=_as_depolarizing(cc.ops), targets=cc.targets,
                                 groups=cc.groups)
    return fault_model.symptoms(twin, kind, groups)


def _commute(P, Q, n):
    """+1 / -1: the symplectic product of two n-qubit Pauli codes (two bits per qubit)."""
    s = 0
    for k in range(n):
        (xp, zp), (xq, zq) = _XZ[(P >> (2 * k)) & 3], _XZ[(Q >> (2 * k)) & 3]
        s ^= (xp & zq) ^ (zp & xq)
    return -1.0 if s else 1.0


def components(a, approximate=False):
    """[q_1 .. q_K] of the channel with arguments a (K = 3 or 15)."""
    a = [float(v) for v in a]
    n = {3: 1, 15: 2}[len(a)]
    p = [1.0 - math.fsum(a)] + a
    lam = [math.fsum(p[P] * _commute(P, Q, n) for P in range(4 ** n)) for Q in range(4 ** n)]
    q = None
    if all(l > 0 for l in lam[1:]):
        q = [0.5 - 0.5 * math.exp(-(2.0 / 4 ** n) * math.fsum(_commute(P, Q, n) * math.log(lam[Q])
                                                               for Q in range(1, 4 ** n))) for P in range(1, 4 ** n)]
        q = [0.0 if -1e-15 < v < 0 else v for v in q]
        if any(v < 0 for v in q):
            q = None
    if q is None:
        if approximate:
            return a
        raise ValueError("the channel has no decomposition into independent Pauli flips")
    return q


def compose(q):
    """The distribution over the 4^n Paulis of independent flips of Pauli P with
    probability q[P - 1], by brute force over the group (XOR of codes)."""
    N = len(q) + 1
    dist = [1.0] + [0.0] * (N - 1)
    for P, qp in enumerate(q, start=1):
        dist = [dist[R_] * (1 - qp) + dist[R_ ^ P] * qp for R_ in range(N)]
    return dist


def mechanisms(ops, probs, args, approximate=False):
    """[(probability, [elementary noise faults])] in program order."""
    out, f = [], 0
    for (op, off, cnt, a0), p in zip(np.asarray(ops).reshape(-1, 4).tolist(), np.asarray(probs).tolist()):
        if op in (XERR, YERR, ZERR, M, MX):
            if p > 0:
                out += [(p, [f + e]) for e in range(cnt)]
            f += cnt
        elif op in (DEP1, PC1):
            if p > 0:
                q = [q1(p)] * 3 if op == DEP1 else components(args[a0:a0 + 3], approximate)
                out += [(q[P - 1], [f + 2 * e + k for k in _PAULI[P]]) for e in range(cnt) for P in (1, 2, 3)
                        if q[P - 1] > 0]
            f += 2 * cnt
        elif op in (DEP2, PC2):
            if p > 0:
                q = [q2(p)] * 15 if op == DEP2 else components(args[a0:a0 + 15], approximate)
                for e in range(cnt // 2):
                    for code in range(1, 16):
                        if q[code - 1] > 0:
                            out.append((q[code - 1], [f + 4 * e + k for k in _PAULI[code >> 2]] +
                                        [f + 4 * e + 2 + k for k in _PAULI[code & 3]]))
            f += 2 * cnt
    return out


def dem_columns(cc, detectors=None, observables=None, approximate=False):
    """The model's DEM columns of a CompiledCircuit: [(probability, detectors, observables)]."""
    s = symptoms(cc, 0, {"detectors": cc.detectors if detectors is None else detectors,
                         "observables": cc.observables if observables is None else observables})
    return merge(mechanisms(cc.ops, cc.probs, cc.args, approximate), s["detectors"], s["observables"])
