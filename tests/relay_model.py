"""Numpy model of the relay-BP stage, the yardstick of
relay_block_kernel: every operation of the spec in its stated order, in
float32 or float64, vectorised over shots.  Sums along a row or a column run as
loops over degree slots, so each shot sees the additions in ascending row
order, and a product and a sum are separate numpy operations, so nothing is
contracted.  Test infrastructure only.
"""
from __future__ import annotations

import math

import numpy as np
import scipy.sparse as sp

BIG = {np.float32: np.float32(1e30), np.float64: np.float64(1e308)}  # Big<T>: "no minimum yet"
DEFAULT_CLIP = 2.0 ** 64
FIX_BITS = 16  # solution weights: llrint(prior * 2^16)


def _csr01(H):
    H = sp.csr_matrix(H, dtype=np.int64)
    H.sum_duplicates()
    H.data %= 2
    H.eliminate_zeros()
    H.sort_indices()
    return H


class RelayModel:
    def __init__(self, H, probs, dtype, *, gamma0=0.125, pre_iter=80, num_sets=60, set_max_iter=60, stop_nconv=1,
                 alpha=1.0, clip=DEFAULT_CLIP, gammas=None, n_data=None, fold_blocks=1, logicals=None):
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
        self.w = np.rint(np.ldexp(lam64, FIX_BITS)).astype(np.int64)
        self.pre_iter, self.num_sets, self.set_max_iter = int(pre_iter), int(num_sets), int(set_max_iter)
        self.stop_nconv = int(stop_nconv)
        self.alpha, self.clip, self.big = T(alpha), T(clip), BIG[T]
        g = np.full((self.num_sets + 1, self.n), float(gamma0), np.float64)
        if self.num_sets:
            g[1:] = np.asarray(gammas, dtype=np.float64).reshape(self.num_sets, self.n)
        self.gam = g.astype(T)           # rounded once
        self.om = T(1) - self.gam        # in T
        # messages by (row, slot in row); a column's edges in ascending row order
        indptr, indices = H.indptr, H.indices
        self.dr = dr = max(1, int(np.diff(indptr).max()))
        self.rcol = np.zeros((self.m, dr), np.int64)
        self.rmask = np.zeros((self.m, dr), bool)
        cols = [[] for _ in range(self.n)]
        for i in range(self.m):
            for t, e in enumerate(range(indptr[i], indptr[i + 1])):
                self.rcol[i, t] = indices[e]
                self.rmask[i, t] = True
                cols[indices[e]].append(i * dr + t)
        self.dc = dc = max(1, max(len(c) for c in cols))
        self.cedge = np.zeros((self.n, dc), np.int64)
        self.cmask = np.zeros((self.n, dc), bool)
        for j, c in enumerate(cols):
            self.cedge[j, :len(c)] = c
            self.cmask[j, :len(c)] = True
        self.flat_col = self.rcol.reshape(-1)

    # ------------------------------------------------------------ one iteration on a subset of shots
    def _iterate(self, v2c, M, s, gam, om):
        """v2c [b][m*dr], M [b][n], s [b][m] -> (v2c, M, x, met)."""
        T, m, dr, big = self.T, self.m, self.dr, self.big
        b = v2c.shape[0]
        v = v2c.reshape(b, m, dr)
        av = np.abs(v)
        neg = (v <= 0) & self.rmask
        m1 = np.full((b, m), big, T)
        m2 = np.full((b, m), big, T)
        for t in range(dr):
            on = self.rmask[:, t]
            a = av[:, :, t]
            m2 = np.where(on, np.minimum(m2, np.maximum(m1, a)), m2)
            m1 = np.where(on, np.minimum(m1, a), m1)
        par = (s.astype(bool) ^ (neg.sum(axis=2) & 1).astype(bool))
        m1a, m2a = m1 * self.alpha, m2 * self.alpha
        y = np.where(av == m1[:, :, None], m2a[:, :, None], m1a[:, :, None])
        c2v = np.where(par[:, :, None] ^ (v <= 0), -y, y).astype(T).reshape(b, m * dr)
        # variable pass
        acc = om * self.lam + gam * M          # both products rounded, then the sum
        pre = []
        cs = []
        for t in range(self.dc):
            on = self.cmask[:, t]
            c = c2v[:, self.cedge[:, t]]
            pre.append(acc)
            cs.append(c)
            acc = np.where(on, acc + c, acc)
        M = np.clip(acc, -self.clip, self.clip)
        x = (M <= 0).astype(np.uint8)
        out = v2c.copy()
        suf = np.zeros_like(acc)
        for t in range(self.dc - 1, -1, -1):
            on = self.cmask[:, t]
            val = np.clip(pre[t] + suf, -self.clip, self.clip)
            e = self.cedge[on, t]
            out[:, e] = val[:, on]
            suf = np.where(on, suf + cs[t], suf)
        hx = (x[:, self.flat_col].reshape(b, m, dr) & self.rmask).sum(axis=2) & 1
        met = (hx == s).all(axis=1)
        return out, M, x, met

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

    def decode(self, syn=None, base=None, readout=None, syn_flags=0):
        """x, corr, llr, iters, legs, status, fail as the kernel writes them, plus
        found (converged legs), first_leg / best_leg (-1: none)."""
        with np.errstate(all="ignore"):
            return self._decode(syn, base, readout, syn_flags)

    def _decode(self, syn, base, readout, syn_flags):
        T, n = self.T, self.n
        s, base, readout = self.syndrome(syn, base, readout, syn_flags)
        B = s.shape[0]
        M = np.tile(self.lam, (B, 1))
        v2c = np.zeros((B, self.m * self.dr), T)
        xh = np.zeros((B, n), np.uint8)
        best = np.zeros((B, n), np.uint8)
        best_w = np.zeros(B, np.int64)
        found = np.zeros(B, np.int64)
        iters = np.zeros(B, np.int32)
        legs = np.zeros(B, np.int32)
        first_leg = np.full(B, -1, np.int64)
        best_leg = np.full(B, -1, np.int64)
        done = np.zeros(B, bool)
        for leg in range(self.num_sets + 1):
            idx = np.nonzero(~done)[0]
            if idx.size == 0:
                break
            gam, om = self.gam[leg], self.om[leg]
            bias = om * self.lam + gam * M[idx]
            v2c[idx] = np.where(self.rmask.reshape(-1), bias[:, self.flat_col], T(0))
            legs[idx] += 1
            conv = np.zeros(B, bool)
            run = idx
            for _ in range(self.pre_iter if leg == 0 else self.set_max_iter):
                if run.size == 0:
                    break
                nv, nM, nx, met = self._iterate(v2c[run], M[run], s[run], gam, om)
                v2c[run], M[run], xh[run] = nv, nM, nx
                iters[run] += 1
                conv[run[met]] = True
                run = run[~met]
            for b in np.nonzero(conv)[0]:
                found[b] += 1
                wgt = int(self.w[xh[b] == 1].sum())
                if found[b] == 1 or wgt < best_w[b]:  # a tie keeps the earlier leg
                    best[b], best_w[b], best_leg[b] = xh[b], wgt, leg
                if found[b] == 1:
                    first_leg[b] = leg
                if found[b] == self.stop_nconv:
                    done[b] = True
        x = np.where((found > 0)[:, None], best, xh).astype(np.uint8)
        fold = np.zeros((B, self.n_data), np.uint8)
        for t in range(self.fold_blocks):
            fold ^= x[:, t * self.n_data:(t + 1) * self.n_data]
        corr = fold if base is None else (fold ^ base)
        fail = np.zeros(B, np.uint8)
        if self.lz is not None and readout is not None:
            fail = (((readout ^ corr).astype(np.int64) @ self.lz.T.astype(np.int64)) & 1).any(axis=1).astype(np.uint8)
        return {"x": x, "corr": corr.astype(np.uint8), "llr": M, "iters": iters, "legs": legs,
                "status": np.where(found > 0, 3, 0).astype(np.uint8), "fail": fail, "found": found,
                "first_leg": first_leg, "best_leg": best_leg}
