"""Numpy model of fault propagation and DEM composition, for the tests.

Restates the ABI's statement (include/qdec.h, "Fault propagation") on the arrays
qd_circuit_create takes, not on the kernel or on dem.py:

* elementary noise faults (kind 0), numbered in program order: X/Y/Z_ERROR one
  per target with the named Pauli (Y: x and z); DEPOLARIZE1 two per target
  (fault 2e X, 2e + 1 Z on target e); DEPOLARIZE2 four per pair (X_a, Z_a, X_b,
  Z_b); M / MX one per target, a flip of that record.  Gauge faults (kind 1): one
  per target of R, RX, M, MX in program order; component z after R and M, x
  after RX and MX.  The numbering does not depend on the probabilities;
* propagation: frame bits (x, z) per qubit and fault, all 0 at the start; H, CX,
  CZ as the sampler; R and RX clear both components; M q: record = x_q, MX q:
  record = z_q, nothing else changes, invert bits do not apply; a fault is
  injected after its instruction's own work;
* mechanisms: X/Y/Z_ERROR(p), M(p): probability p; DEPOLARIZE1(p): X, Y = {X, Z},
  Z with q1 = 1/2 - 1/2 (1 - 4p/3)^(1/2) each; DEPOLARIZE2(p): codes 1 .. 15,
  first qubit's Pauli code >> 2, second's code & 3 (1 X, 2 Y, 3 Z), with
  q2 = 1/2 - 1/2 (1 - 16p/15)^(1/8) each; p = 0 contributes nothing;
* merge: a mechanism's symptom is the XOR of its members' rows; equal symptoms
  merge by p <- p (1 - p') + p' (1 - p) in mechanism order; empty symptoms are
  dropped; columns in order of first appearance.

Bit f of the model's words is fault f (64 per uint64 word), as in the kernel;
that is a choice of speed, not of meaning.
"""
import numpy as np
import scipy.sparse as sp

H, CX, CZ, R, RX, M, MX, XERR, YERR, ZERR, DEP1, DEP2 = range(12)
INVERT = 1 << 30
X_, Z_, Y_, REC_ = 1, 2, 3, 4


def enumerate_faults(ops, kind=0):
    """[(instruction, index into targets, component)] of the faults of one kind."""
    out = []
    for i, (op, off, cnt, _) in enumerate(np.asarray(ops).reshape(-1, 4).tolist()):
        if kind == 1:
            if op in (R, RX, M, MX):
                out += [(i, off + e, X_ if op in (RX, MX) else Z_) for e in range(cnt)]
        elif op in (XERR, YERR, ZERR):
            out += [(i, off + e, {XERR: X_, YERR: Y_, ZERR: Z_}[op]) for e in range(cnt)]
        elif op in (DEP1, DEP2):
            out += [(i, off + e, c) for e in range(cnt) for c in (X_, Z_)]
        elif op in (M, MX):
            out += [(i, off + e, REC_) for e in range(cnt)]
    return out


def _flip(words, row, f):
    """words[row[k], bit f[k]] ^= 1 for every k (repeated rows included)."""
    np.bitwise_xor.at(words, (row, f >> 6), np.uint64(1) << (f & 63).astype(np.uint64))


def propagate(num_qubits, ops, targets, kind=0):
    """uint8 [F, M]: the record flips each fault of `kind` causes on its own."""
    ops = np.asarray(ops).reshape(-1, 4)
    targets = np.asarray(targets, dtype=np.int64)
    faults = enumerate_faults(ops, kind)
    F = len(faults)
    W = (F + 63) // 64
    by_op = {}
    for f, (i, t, c) in enumerate(faults):
        by_op.setdefault(i, []).append((f, t, c))
    x = np.zeros((num_qubits, W), np.uint64)
    z = np.zeros((num_qubits, W), np.uint64)
    rec = []
    for i, (op, off, cnt, _) in enumerate(ops.tolist()):
        q = targets[off:off + cnt] & (INVERT - 1)
        if op == H:
            x[q], z[q] = z[q].copy(), x[q].copy()
        elif op == CX:
            a, b = q[0::2], q[1::2]
            x[b] ^= x[a]
            z[a] ^= z[b]
        elif op == CZ:
            a, b = q[0::2], q[1::2]
            xa, xb = x[a].copy(), x[b].copy()
            z[a] ^= xb
            z[b] ^= xa
        elif op in (R, RX):
            x[q] = 0
            z[q] = 0
        elif op in (M, MX):
            rec.append((x if op == M else z)[q].copy())
        here = by_op.get(i)
        if here:
            f = np.array([h[0] for h in here], np.int64)
            t = np.array([h[1] for h in here], np.int64)
            c = np.array([h[2] for h in here], np.int64)
            qq = targets[t] & (INVERT - 1)
            _flip(x, qq[(c & X_) != 0], f[(c & X_) != 0])
            _flip(z, qq[(c & Z_) != 0], f[(c & Z_) != 0])
            if (c == REC_).any():
                _flip(rec[-1], t[c == REC_] - off, f[c == REC_])
    if not rec:
        return np.zeros((F, 0), np.uint8)
    words = np.concatenate(rec, axis=0)                  # [M, W]
    bits = np.unpackbits(words.astype("<u8").view(np.uint8).reshape(words.shape[0], -1), axis=1, bitorder="little")
    return np.ascontiguousarray(bits[:, :F].T)


def symptoms(cc, kind=0, groups=None):
    """{group: uint8 [F, rows]} of a CompiledCircuit's output groups (or the given
    {name: sparse matrix over records}) for every fault of `kind`, plus 'rec'."""
    rec = propagate(cc.num_qubits, cc.ops, cc.targets, kind)
    out = {"rec": rec}
    r64 = sp.csr_matrix(rec.astype(np.int64))
    for name, mat in (cc.groups if groups is None else groups).items():
        mat = sp.csr_matrix(mat).astype(np.int64)
        out[name] = np.asarray((r64 @ mat.T).todense() % 2, dtype=np.uint8).reshape(rec.shape[0], mat.shape[0])
    return out


def q1(p):
    if not 0 <= p <= 3 / 4:
        raise ValueError("DEPOLARIZE1 probability above 3/4")
    return 0.5 - 0.5 * (1 - 4 * p / 3) ** 0.5


def q2(p):
    if not 0 <= p <= 15 / 16:
        raise ValueError("DEPOLARIZE2 probability above 15/16")
    return 0.5 - 0.5 * (1 - 16 * p / 15) ** 0.125


_PAULI = {0: (), 1: (0,), 2: (0, 1), 3: (1,)}   # offsets of a Pauli's (X, Z) faults


def mechanisms(ops, probs):
    """[(probability, [elementary noise faults])] in program order."""
    out, f = [], 0
    for (op, off, cnt, _), p in zip(np.asarray(ops).reshape(-1, 4).tolist(), np.asarray(probs).tolist()):
        if op in (XERR, YERR, ZERR, M, MX):
            if p > 0:
                out += [(p, [f + e]) for e in range(cnt)]
            f += cnt
        elif op == DEP1:
            if p > 0:
                out += [(q1(p), [f + 2 * e + k for k in _PAULI[P]]) for e in range(cnt) for P in (1, 2, 3)]
            f += 2 * cnt
        elif op == DEP2:
            if p > 0:
                for e in range(cnt // 2):
                    for code in range(1, 16):
                        out.append((q2(p), [f + 4 * e + k for k in _PAULI[code >> 2]] +
                                    [f + 4 * e + 2 + k for k in _PAULI[code & 3]]))
            f += 2 * cnt
    return out


def merge(mechs, det_rows, obs_rows):
    """[(probability, detectors, observables)]: the DEM's columns from the
    mechanisms and the 0/1 symptom rows of the elementary faults."""
    det_rows, obs_rows = np.asarray(det_rows, np.uint8), np.asarray(obs_rows, np.uint8)
    cols = {}
    for p, members in mechs:
        d = np.bitwise_xor.reduce(det_rows[members], axis=0) if members else det_rows[0] * 0
        o = np.bitwise_xor.reduce(obs_rows[members], axis=0) if members else obs_rows[0] * 0
        if not d.any() and not o.any():
            continue
        key = (d.tobytes(), o.tobytes())
        if key in cols:
            q = cols[key][0]
            cols[key][0] = q * (1 - p) + p * (1 - q)
        else:
            cols[key] = [p, tuple(np.nonzero(d)[0].tolist()), tuple(np.nonzero(o)[0].tolist())]
    return [tuple(v) for v in cols.values()]


def dem_columns(cc, detectors=None, observables=None):
    """The model's DEM columns of a CompiledCircuit (merge of its mechanisms),
    with the symptom rows they were made from: (columns, det_rows, obs_rows)."""
    s = symptoms(cc, 0, {"detectors": cc.detectors if detectors is None else detectors,
                         "observables": cc.observables if observables is None else observables})
    return merge(mechanisms(cc.ops, cc.probs), s["detectors"], s["observables"]), s["detectors"], s["observables"]
