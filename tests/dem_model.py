"""Numpy model of the fault sampler (qd_sample_faults_device), for the tests.

Fault j of shot s fires when lane j % 4 of the Philox4x32-10 block with key
(seed, stream_id) and counter (j // 4, 0, s & 0xffffffff, s >> 32) is below
threshold(p_j); det = H e, obs = F e (mod 2).  Written from the ABI's statement
of the draw (include/qdec.h), not from the kernel.
"""
import numpy as np
import scipy.sparse as sp

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """ctr uint32 [..., 4], key (k0, k1) -> uint32 [..., 4]."""
    c = np.asarray(ctr, dtype=np.uint64) & np.uint64(MASK)
    c0, c1, c2, c3 = (c[..., i].copy() for i in range(4))
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    for _ in range(10):
        p0 = np.uint64(M0) * c0  # < 2^64: both factors are below 2^32
        p1 = np.uint64(M1) * c2
        hi0, lo0 = p0 >> np.uint64(32), p0 & np.uint64(MASK)
        hi1, lo1 = p1 >> np.uint64(32), p1 & np.uint64(MASK)
        c0, c1, c2, c3 = hi1 ^ c1 ^ np.uint64(k0), lo1, hi0 ^ c3 ^ np.uint64(k1), lo0
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def threshold(p):
    """The samplers' probability -> u32 threshold: 0 unless p > 0, else
    floor(p 2^32) clamped to 0xFFFFFFFF."""
    p = np.asarray(p, dtype=np.float64)
    v = np.floor(np.where(p > 0, p, 0.0) * 4294967296.0)
    return np.where(v >= 4294967295.0, 4294967295.0, v).astype(np.uint64).astype(np.uint32)


def sample(H, F, probs, seed, stream_id, shot0, B):
    """(det uint8 [B, m], faults uint8 [B, n], obs uint8 [B, k]) of shots
    shot0 .. shot0 + B (F may be None: k = 0)."""
    H = sp.csr_matrix(H)
    m, n = H.shape
    thr = threshold(np.broadcast_to(np.asarray(probs, dtype=np.float64), (n,)))
    words = (n + 3) // 4
    shots = (int(shot0) + np.arange(B, dtype=object)) if B else np.zeros(0, dtype=object)
    ctr = np.zeros((B, words, 4), np.uint64)
    ctr[:, :, 0] = np.arange(words, dtype=np.uint64)[None, :]
    ctr[:, :, 2] = np.array([int(s) & MASK for s in shots], dtype=np.uint64)[:, None]
    ctr[:, :, 3] = np.array([(int(s) >> 32) & MASK for s in shots], dtype=np.uint64)[:, None]
    u = philox4x32_10(ctr, (seed, stream_id)).reshape(B, words * 4)[:, :n]
    e = (u < thr[None, :]).astype(np.uint8)
    det = np.asarray((sp.csr_matrix(e.astype(np.int64)) @ H.T.astype(np.int64)).todense() % 2, dtype=np.uint8)
    if F is None or sp.csr_matrix(F).shape[0] == 0:
        obs = np.zeros((B, 0), np.uint8)
    else:
        F = sp.csr_matrix(F)
        obs = np.asarray((sp.csr_matrix(e.astype(np.int64)) @ F.T.astype(np.int64)).todense() % 2, dtype=np.uint8)
    return det.reshape(B, m), e, obs
