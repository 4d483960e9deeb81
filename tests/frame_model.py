"""Numpy model of the Pauli-frame sampler (qd_circuit_sample_device), for the tests.

Restates the ABI's statement of the program and of the draws (include/qdec.h,
DESIGN §3.4c) on the arrays qd_circuit_create takes, not on the kernel:

* frame bits (x, z) per qubit and shot, all 0 at the start; H swaps them;
  CX c t: x_t ^= x_c, z_c ^= z_t; CZ a b: z_a ^= x_b, z_b ^= x_a;
  M q: record = x_q ^ flip ^ invert, z_q ^= rand; MX q: record = z_q ^ flip ^
  invert, x_q ^= rand; R q: x_q = 0, z_q = rand; RX q: z_q = 0, x_q = rand;
* Bernoulli / Pauli site s of shot g: u = lane s % 4 of Philox4x32-10, key
  (seed, stream_id), counter (s // 4, 0, g & 0xffffffff, g >> 32); fires when
  u < threshold(p).  DEPOLARIZE1: Pauli 1 + (3 u) // T (1 X, 2 Y, 3 Z).
  DEPOLARIZE2: code 1 + (15 u) // T, first qubit code >> 2, second code & 3.
  Sites number the targets (pairs for DEPOLARIZE2) of noise and measurement
  instructions in program order, every instruction starting at a multiple of 4;
* randomisation site r of shot g: bit g % 32 of lane (g // 32) % 4 of the block
  with counter (r, 1, (g // 128) & 0xffffffff, (g // 128) >> 32); sites number
  the targets of R, RX, M, MX in program order.
"""
import numpy as np
import scipy.sparse as sp

from dem_model import MASK, philox4x32_10, threshold

H, CX, CZ, R, RX, M, MX, XERR, YERR, ZERR, DEP1, DEP2 = range(12)
INVERT = 1 << 30


def _uniforms(site0, count, shots, key):
    """uint64 [count, B]: the u of sites site0 .. site0 + count for each shot."""
    assert site0 % 4 == 0
    nb = (count + 3) // 4
    ctr = np.zeros((nb, shots.size, 4), np.uint64)
    ctr[:, :, 0] = (site0 // 4 + np.arange(nb, dtype=np.uint64))[:, None]
    ctr[:, :, 2] = (shots & np.uint64(MASK))[None, :]
    ctr[:, :, 3] = (shots >> np.uint64(32))[None, :]
    u = philox4x32_10(ctr, key)                       # [nb, B, 4]
    return u.transpose(0, 2, 1).reshape(nb * 4, shots.size)[:count].astype(np.uint64)


def _rand_bits(rsite0, count, shots, key):
    """bool [count, B]: the randomisation bits of sites rsite0 .. rsite0 + count."""
    blk = shots >> np.uint64(7)
    ub, inv = np.unique(blk, return_inverse=True)
    ctr = np.zeros((count, ub.size, 4), np.uint64)
    ctr[:, :, 0] = (rsite0 + np.arange(count, dtype=np.uint64))[:, None]
    ctr[:, :, 1] = 1
    ctr[:, :, 2] = (ub & np.uint64(MASK))[None, :]
    ctr[:, :, 3] = (ub >> np.uint64(32))[None, :]
    w = philox4x32_10(ctr, key)                       # [count, blocks, 4]
    lane = ((shots >> np.uint64(5)) & np.uint64(3)).astype(np.int64)
    bit = (shots & np.uint64(31)).astype(np.uint32)
    words = w[:, inv, lane]                           # [count, B]
    return ((words >> bit[None, :]) & np.uint32(1)).astype(bool)


def run(num_qubits, ops, targets, probs, seed, stream_id, shot0, B):
    """The measurement record, uint8 [B, M], of shots shot0 .. shot0 + B."""
    ops = np.asarray(ops).reshape(-1, 4)
    targets = np.asarray(targets, dtype=np.int64)
    thr = threshold(np.asarray(probs, dtype=np.float64)).astype(np.uint64)
    key = (seed, stream_id)
    shots = np.uint64(shot0) + np.arange(B, dtype=np.uint64)
    x = np.zeros((num_qubits, B), bool)
    z = np.zeros((num_qubits, B), bool)
    rec = []
    site = rsite = 0
    for (op, off, cnt, _), T in zip(ops, thr):
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
        elif op in (XERR, YERR, ZERR, DEP1):
            u = _uniforms(site, cnt, shots, key)
            site += (cnt + 3) // 4 * 4
            fired = u < T
            one = np.uint64(1)
            P = np.where(fired, one + (np.uint64(3) * u) // max(T, one), np.uint64(0)) if op == DEP1 else \
                np.where(fired, np.uint64({XERR: 1, YERR: 2, ZERR: 3}[int(op)]), np.uint64(0))
            # a noise instruction may name a qubit twice: apply its targets in order
            for e, qq in enumerate(q):
                x[qq] ^= (P[e] == 1) | (P[e] == 2)
                z[qq] ^= P[e] >= 2
        elif op == DEP2:
            pairs = cnt // 2
            u = _uniforms(site, pairs, shots, key)
            site += (pairs + 3) // 4 * 4
            one = np.uint64(1)
            code = np.where(u < T, one + (np.uint64(15) * u) // max(T, one), np.uint64(0))
            for e in range(pairs):
                for qq, P in ((q[2 * e], code[e] >> np.uint64(2)), (q[2 * e + 1], code[e] & np.uint64(3))):
                    x[qq] ^= (P == 1) | (P == 2)
                    z[qq] ^= P >= 2
        else:
            raise ValueError(f"opcode {op}")
    if not rec:
        return np.zeros((B, 0), np.uint8)
    return np.concatenate(rec, axis=0).T.astype(np.uint8).copy()


def sample(cc, seed, stream_id, shot0, B, groups=None):
    """{group: uint8 [B, rows]} of a CompiledCircuit's output groups (or the
    given {name: sparse matrix over records}), plus 'rec' itself."""
    rec = run(cc.num_qubits, cc.ops, cc.targets, cc.probs, seed, stream_id, shot0, B)
    out = {"rec": rec}
    r64 = sp.csr_matrix(rec.astype(np.int64))
    for name, mat in (cc.groups if groups is None else groups).items():
        mat = sp.csr_matrix(mat).astype(np.int64)
        out[name] = np.asarray((r64 @ mat.T).todense() % 2, dtype=np.uint8).reshape(B, mat.shape[0])
    return out
