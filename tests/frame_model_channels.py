"""Numpy model of the Pauli-frame sampler with PAULI_CHANNEL_1 / PAULI_CHANNEL_2,
for the tests.  Extends tests/frame_model.py by the ABI's statement of the two
instructions (include/qdec.h) on the arrays qd_circuit_create_args takes:

* opcodes 12 (PAULI_CHANNEL_1) and 13 (PAULI_CHANNEL_2); ops[i][3] is the
  instruction's first entry of `args`, of which it reads K = 3 / 15: the
  probabilities of X, Y, Z, or of the two-qubit codes 1 .. 15 (first qubit's
  Pauli code >> 2, second's code & 3; 0 I, 1 X, 2 Y, 3 Z);
* one site per target (PAULI_CHANNEL_1) or pair (PAULI_CHANNEL_2), numbered with
  the other noise sites, every instruction starting at a multiple of 4; u as for
  every other site;
* c_k = c_{k-1} + a_k in double, left to right; C_k = threshold(c_k); a site fires
  when u < C_{K-1}; its outcome is 1 + #{j < K : C_j <= u}.

Every other instruction follows frame_model's rules, on its helpers for the draws.
"""
import numpy as np
import scipy.sparse as sp

from dem_model import threshold
from frame_model import (CX, CZ, DEP1, DEP2, H, INVERT, M, MX, R, RX, XERR, YERR, ZERR, _rand_bits, _uniforms)

PC1, PC2 = 12, 13


def cumulative_thresholds(a):
    """uint64 [K]: C_k of the arguments a_0 .. a_{K-1}."""
    c, out = 0.0, []
    for v in np.asarray(a, np.float64).tolist():
        c = c + v
        out.append(int(threshold(c)))
    return np.asarray(out, np.uint64)


def channel_outcome(u, a):
    """The outcome (0: none) of a site with uniform u (uint64 array)."""
    C = cumulative_thresholds(a)
    fired = u < C[-1]
    count = sum((C[j] <= u).astype(np.int64) for j in range(C.size))
    return np.where(fired, 1 + count, 0).astype(np.uint64)


def _apply(x, z, qq, P):
    x[qq] ^= (P == 1) | (P == 2)
    z[qq] ^= P >= 2


def run(num_qubits, ops, targets, probs, args, seed, stream_id, shot0, B):
    """The measurement record, uint8 [B, M], of shots shot0 .. shot0 + B."""
    ops = np.asarray(ops).reshape(-1, 4)
    targets = np.asarray(targets, dtype=np.int64)
    args = np.asarray(args, dtype=np.float64)
    thr = threshold(np.asarray(probs, dtype=np.float64)).astype(np.uint64)
    key = (seed, stream_id)
    shots = np.uint64(shot0) + np.arange(B, dtype=np.uint64)
    x = np.zeros((num_qubits, B), bool)
    z = np.zeros((num_qubits, B), bool)
    rec = []
    site = rsite = 0
    one = np.uint64(1)
    for (op, off, cnt, a0), T in zip(ops, thr):
        tg = targets[off:off + cnt]
        q = tg & (INVERT - 1)
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
            rnd = _rand_bits(rsite, cnt, shots, key)
            rsite += cnt
            if op == R:
                x[q], z[q] = False, rnd
            else:
                z[q], x[q] = False, rnd
        elif op in (M, MX):
            rnd = _rand_bits(rsite, cnt, shots, key)
            rsite += cnt
            flip = _uniforms(site, cnt, shots, key) < T
            site += (cnt + 3) // 4 * 4
            inv = ((tg & INVERT) != 0)[:, None]
            if op == M:
                rec.append(x[q] ^ flip ^ inv)
                z[q] ^= rnd
            else:
                rec.append(z[q] ^ flip ^ inv)
                x[q] ^= rnd
        elif op in (XERR, YERR, ZERR, DEP1, PC1):
            u = _uniforms(site, cnt, shots, key)
            site += (cnt + 3) // 4 * 4
            if op == PC1:
                P = channel_outcome(u, args[a0:a0 + 3])
            elif op == DEP1:
                P = np.where(u < T, one + (np.uint64(3) * u) // max(T, one), np.uint64(0))
            else:
                P = np.where(u < T, np.uint64({XERR: 1, YERR: 2, ZERR: 3}[int(op)]), np.uint64(0))
            for e, qq in enumerate(q):      # a noise instruction may name a qubit twice: in order
                _apply(x, z, qq, P[e])
        elif op in (DEP2, PC2):
            pairs = cnt // 2
            u = _uniforms(site, pairs, shots, key)
            site += (pairs + 3) // 4 * 4
            code = channel_outcome(u, args[a0:a0 + 15]) if op == PC2 else \
                np.where(u < T, one + (np.uint64(15) * u) // max(T, one), np.uint64(0))
            for e in range(pairs):
                _apply(x, z, q[2 * e], code[e] >> np.uint64(2))
                _apply(x, z, q[2 * e + 1], code[e] & np.uint64(3))
        else:
            raise ValueError(f"opcode {op}")
    if not rec:
        return np.zeros((B, 0), np.uint8)
    return np.concatenate(rec, axis=0).T.astype(np.uint8).copy()


def sample(cc, seed, stream_id, shot0, B, groups=None):
    """{group: uint8 [B, rows]} of a CompiledCircuit's output groups (or the
    given {name: sparse matrix over records}), plus 'rec' itself."""
    rec = run(cc.num_qubits, cc.ops, cc.targets, cc.probs, cc.args, seed, stream_id, shot0, B)
    out = {"rec": rec}
    r64 = sp.csr_matrix(rec.astype(np.int64))
    for name, mat in (cc.groups if groups is None else groups).items():
        mat = sp.csr_matrix(mat).astype(np.int64)
        out[name] = np.asarray((r64 @ mat.T).todense() % 2, dtype=np.uint8).reshape(B, mat.shape[0])
    return out
