"""Numpy model of layered (check-serial) min-sum BP, the yardstick
of layered_wave_kernel: every operation of the spec in its stated order, in
float32 or float64, vectorised over shots with the rows in a Python loop.  A
product and a sum are separate numpy operations, so nothing is contracted.
Test infrastructure only.

Three facts the tests rest on:
  * min, max and parity are exact, so a row's result does not depend on the
    order in which its entries are combined: the kernel's lanes along the row,
    merged by a butterfly and a ballot, give the bits of the sort used here;
  * a column occurs once per row (the matrix is canonical CSR), so the P
    updates of one row do not collide and the fancy-indexed store below writes
    every P once;
  * with a finite clip every value stays finite and no NaN can arise:
    |R| <= clip and |P| <= clip by the min and the clamp, so |q| <= 2 clip, and
    no operation meets inf - inf or 0 * inf (Big * alpha is finite in both
    precisions).
A degree-1 row sends +-clip (Big * alpha is beyond it); a column pinned at
+-clip later reads q = 0 on that row, which is <= 0 and handled like any value.
"""
from __future__ import annotations

import math

import numpy as np
import scipy.sparse as sp

from relay_model import BIG, DEFAULT_CLIP, _csr01


def alpha_at(T, t, ms_scaling):
    """alpha_at<T> of the kernels: 1 - 2^-t when ms_scaling is 0, else constant."""
    return T(1.0 - math.ldexp(1.0, -t)) if ms_scaling == 0.0 else T(ms_scaling)


class LayeredModel:
    def __init__(self, H, probs, dtype, *, max_iter, ms_scaling=0.0, clip=DEFAULT_CLIP, n_data=None, fold_blocks=1,
                 logicals=None):
        H = _csr01(H)
        self.H = H
        self.m, self.n = H.shape
        self.T = T = np.dtype(dtype).type
        self.n_data = self.n if n_data is None else int(n_data)
        self.fold_blocks = int(fold_blocks)
        self.lz = None if logicals is None else (np.asarray(sp.csr_matrix(logicals).todense()) % 2).astype(np.uint8)
        p = np.broadcast_to(np.asarray(probs, dtype=np.float64), (self.n,))
        lam64 = np.array([math.log((1 - float(v)) / float(v)) for v in p], dtype=np.float64)  # libm, as the library
        self.lam = lam64.astype(T)
        self.max_iter = int(max_iter) if int(max_iter) > 0 else self.n
        self.ms_scaling = float(ms_scaling)
        self.clip, self.big = T(clip), BIG[T]
        assert np.isfinite(self.clip) and self.clip > 0

    def syndrome(self, syn=None, base=None, readout=None, syn_flags=0):
        u8 = lambda a, c: None if a is None else (np.asarray(a, np.uint8).reshape(-1, c) & 1)
        syn, base, readout = u8(syn, self.m), u8(base, self.n_data), u8(readout, self.n_data)
        B = next(a.shape[0] for a in (syn, base, readout) if a is not None)
        s = np.zeros((B, self.m), np.uint8) if syn is None else syn.copy()
        Hd = self.H[:, :self.n_data]
        if (syn_flags & 1) and base is not None:
            s ^= (Hd.dot(base.T.astype(np.int64)).T & 1).astype(np.uint8)
        if (syn_flags & 2) and readout is not None:
            s ^= (Hd.dot(readout.T.astype(np.int64)).T & 1).astype(np.uint8)
        return s, base, readout

    def _row(self, P, R, s, i, alpha):
        """Row i on the shots of P [b][n], R [b][E], s [b][m], in place."""
        T = self.T
        e0, e1 = self.H.indptr[i], self.H.indptr[i + 1]
        if e0 == e1:
            return
        cols = self.H.indices[e0:e1]
        q = P[:, cols] - R[:, e0:e1]
        av = np.abs(q)
        if e1 - e0 >= 2:
            two = np.partition(av, 1, axis=1)[:, :2]
            m1, m2 = two[:, 0], two[:, 1]
        else:
            m1, m2 = av[:, 0], np.full(av.shape[0], self.big, T)
        neg = q <= 0
        par = s[:, i].astype(bool) ^ (neg.sum(axis=1) & 1).astype(bool)
        m1a, m2a = m1 * alpha, m2 * alpha
        y = np.minimum(np.where(av == m1[:, None], m2a[:, None], m1a[:, None]), self.clip)
        r = np.where(par[:, None] ^ neg, -y, y).astype(T)
        R[:, e0:e1] = r
        P[:, cols] = np.clip(q + r, -self.clip, self.clip)

    def decode(self, syn=None, base=None, readout=None, syn_flags=0, stop=True):
        """x, corr, llr, iters, status, fail as the kernel writes them.  stop=False
        runs every shot for max_iter iterations (status and x are still those of
        the last iteration)."""
        T, n = self.T, self.n
        s, base, readout = self.syndrome(syn, base, readout, syn_flags)
        B = s.shape[0]
        P = np.tile(self.lam, (B, 1))
        R = np.zeros((B, self.H.nnz), T)
        x = np.zeros((B, n), np.uint8)
        iters = np.zeros(B, np.int32)
        conv = np.zeros(B, bool)
        run = np.arange(B)
        Hi = self.H.astype(np.int64)
        with np.errstate(all="raise", under="ignore"):  # a NaN or an overflow would be a bug of the model
            for t in range(1, self.max_iter + 1):
                if run.size == 0:
                    break
                alpha = alpha_at(T, t, self.ms_scaling)
                Pr, Rr, sr = P[run], R[run], s[run]
                for i in range(self.m):
                    self._row(Pr, Rr, sr, i, alpha)
                P[run], R[run] = Pr, Rr
                xr = (Pr <= 0).astype(np.uint8)
                x[run] = xr
                iters[run] += 1
                met = ((Hi.dot(xr.T.astype(np.int64)).T & 1) == sr).all(axis=1)
                conv[run] = met
                if stop:
                    run = run[~met]
        assert not np.isnan(P).any() and np.isfinite(P).all()
        fold = np.zeros((B, self.n_data), np.uint8)
        for t in range(self.fold_blocks):
            fold ^= x[:, t * self.n_data:(t + 1) * self.n_data]
        corr = fold if base is None else (fold ^ base)
        fail = np.zeros(B, np.uint8)
        if self.lz is not None and readout is not None:
            fail = (((readout ^ corr).astype(np.int64) @ self.lz.T.astype(np.int64)) & 1).any(axis=1).astype(np.uint8)
        return {"x": x, "corr": corr.astype(np.uint8), "llr": P, "iters": iters,
                "status": np.where(conv, 3, 0).astype(np.uint8), "fail": fail}
