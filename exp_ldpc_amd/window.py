"""Sliding-window decoding of layered graphs.

A multi-round storage experiment is decoded on one spacetime graph that grows
with the round count; a window of W rounds has a fixed size whatever R is.  The
reference left this as a stub (``# def spacetime_code_sliding_window(...)``,
spacetime_code.py:95-96).

``WindowPlan`` cuts any check matrix whose rows carry a non-decreasing layer
number into windows (host, numpy); ``spacetime_windows`` is the instance of a
``SpacetimeCode``.  ``WindowAdvance`` is one window boundary on the device
(qd_window_*, csrc/qdec_window.hip): it commits part of a window's solution,
pushes its effect on the syndrome forward and hands the next window its rows.
``WindowedDecoder`` owns one ``Decoder`` per distinct window graph and one
boundary per window, and runs them in turn on device tensors.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np
import scipy.sparse as sp

from . import _abi
from .decoder import Decoder, _current_stream, as_csr01
from .spacetime import SpacetimeCode

__all__ = ["Window", "WindowPlan", "WindowAdvance", "WindowedDecoder", "spacetime_windows", "check_window_args"]


def check_window_args(window, commit):
    """(window, commit) as integers with 1 <= commit <= window; commit defaults
    to max(1, window // 2).  ValueError otherwise."""
    window = int(window)
    commit = max(1, window // 2) if commit is None else int(commit)
    if window < 1:
        raise ValueError(f"window must be >= 1, got {window}")
    if not 1 <= commit <= window:
        raise ValueError(f"commit must satisfy 1 <= commit <= window, got commit={commit}, window={window}")
    return window, commit


@dataclass
class Window:
    start: int                # first layer
    size: int                 # layers
    final: bool
    row0: int                 # rows [row0, row0 + m) of the full graph
    cols: np.ndarray          # global columns, ascending
    graph: sp.csr_matrix      # H[row0 : row0 + m, cols]
    committed: np.ndarray     # window-local columns committed after this window (all of them in the final one)
    # the boundary behind this window (WindowAdvance's arguments): the carry of the
    # committed columns into later rows, their accumulator rows, and the next
    # window's rows (none behind the final one)
    carry_rows: np.ndarray = None
    carry_ptr: np.ndarray = None
    carry_cols: np.ndarray = None
    acc_ptr: np.ndarray = None
    acc_cols: np.ndarray = None
    next_row0: int = 0
    next_m: int = 0
    fold_blocks: int = 1

    @property
    def m(self) -> int:
        return self.graph.shape[0]

    @property
    def n(self) -> int:
        return self.graph.shape[1]


def _csr_tables(M):
    M = as_csr01(M)
    return np.ascontiguousarray(M.indptr, dtype=np.int32), np.ascontiguousarray(M.indices, dtype=np.int32)


class WindowPlan:
    """Windows of W = `window` layers over a check matrix whose row r lies in
    layer row_layer[r] (non-decreasing, 0 .. T); a column's layer is the
    smallest layer among its rows.  Non-final windows start at layers 0, C, 2C,
    ... (C = `commit`) for as long as start + W <= T; the final window starts at
    the next multiple of C and runs to T.  W >= T + 1: one window, the whole
    graph.  A window's graph holds the rows of its layers and the columns whose
    layer lies in it (entries in later rows are cut off); behind a non-final
    window the columns of its first C layers are committed.  `acc` (sparse
    k_acc x n): the committed part of x is accumulated through it."""

    def __init__(self, H, row_layer, window, commit, acc=None, n_data=None):
        self.window, self.commit = check_window_args(window, commit)
        H = as_csr01(H)
        self.H = H
        m, n = H.shape
        self.m, self.n = m, n
        layer = np.asarray(row_layer, dtype=np.int64).reshape(-1)
        if layer.size != m or m == 0:
            raise ValueError("row_layer must give one layer per row of a non-empty matrix")
        if layer[0] != 0 or np.any(np.diff(layer) < 0):
            raise ValueError("row_layer must start at 0 and never decrease")
        self.row_layer = layer
        T = self.T = int(layer[-1])
        Hc = sp.csc_matrix(H)
        Hc.sort_indices()
        if np.any(np.diff(Hc.indptr) == 0):
            raise ValueError("a column without a row has no layer")
        self.col_layer = layer[Hc.indices[Hc.indptr[:-1]]]  # rows ascend, and so do their layers
        self.acc = as_csr01(acc) if acc is not None else sp.csr_matrix((0, n), dtype=np.int64)
        if self.acc.shape[1] != n:
            raise ValueError("acc must have one column per column of H")
        self.k_acc = self.acc.shape[0]
        self.n_data = None if n_data is None else int(n_data)
        W, Cm = self.window, self.commit
        spans = []  # (start, size, final)
        a = 0
        if W < T + 1:
            while a + W <= T:
                spans.append((a, W, False))
                a += Cm
        spans.append((a, T + 1 - a, True))
        first_row = np.searchsorted(layer, np.arange(T + 2), side="left")  # first row of every layer (and m)
        self.windows = []
        for a, size, final in spans:
            r0, r1 = int(first_row[a]), int(first_row[a + size])
            cols = np.flatnonzero((self.col_layer >= a) & (self.col_layer < a + size))
            graph = as_csr01(H[r0:r1][:, cols])
            hi = a + size if final else a + Cm
            committed = np.flatnonzero(self.col_layer[cols] < hi)
            self.windows.append(Window(a, size, final, r0, cols, graph, committed, fold_blocks=size))
        acc_c = sp.csc_matrix(self.acc)
        for k, w in enumerate(self.windows):
            gcols = w.cols[w.committed]
            local = sp.csr_matrix((np.ones(gcols.size, np.int64), (np.arange(gcols.size), w.committed)),
                                  shape=(gcols.size, w.n))  # committed column -> window-local column
            w.acc_ptr, w.acc_cols = _csr_tables(sp.csr_matrix(acc_c[:, gcols]) @ local)
            if w.final:
                w.carry_rows = np.zeros(0, np.int32)
                w.carry_ptr, w.carry_cols = np.zeros(1, np.int32), np.zeros(0, np.int32)
                continue
            nxt = self.windows[k + 1]
            w.next_row0, w.next_m = nxt.row0, nxt.m
            later = sp.csr_matrix(sp.csc_matrix(H[nxt.row0:])[:, gcols]) @ local
            later = as_csr01(later)
            hit = np.flatnonzero(np.diff(later.indptr) > 0)
            w.carry_rows = np.ascontiguousarray(nxt.row0 + hit, dtype=np.int32)
            w.carry_ptr, w.carry_cols = _csr_tables(later[hit])

    def priors(self, priors):
        """Per window, the entries of a full-graph prior vector (or a scalar)."""
        p = np.broadcast_to(np.asarray(priors, dtype=np.float64), (self.n,))
        return [np.ascontiguousarray(p[w.cols]) for w in self.windows]


def spacetime_windows(H, R: int, window, commit=None) -> WindowPlan:
    """The windows of ``SpacetimeCode(H, R)``: layers are rounds (row // r), the
    accumulator is the fold map.  A non-final window's graph is
    ``[blockdiag(H x W) | M]`` with W measurement blocks, the last of column
    weight 1 (the future boundary is open); the final window's graph is
    ``SpacetimeCode(H, R - start).spacetime_check_matrix``.  Data blocks come
    first, so every window is an ordinary Decoder graph with n_data = n and
    fold_blocks = its layers."""
    h = sp.csr_matrix(H)
    r, n = h.shape
    R = int(R)
    Hst = SpacetimeCode(h, R).spacetime_check_matrix
    fold = sp.hstack([sp.identity(n, dtype=np.int64, format="csr")] * (R + 1)
                     + [sp.csr_matrix((n, R * r), dtype=np.int64)], format="csr")
    return WindowPlan(Hst, np.arange((R + 1) * r) // r, window, commit, acc=fold, n_data=n)


class WindowAdvance:
    """One window boundary on a device (qd_window_create): see include/qdec.h."""

    def __init__(self, n_w, m_total, carry_rows, carry_ptr, carry_cols, acc_ptr, acc_cols, row0, m_next, *,
                 device: int | None = 0):
        self._lib = _abi.load()
        i32 = lambda a: np.ascontiguousarray(np.asarray(a), dtype=np.int32)  # noqa: E731
        rows, cp, cc, ap, ac = i32(carry_rows), i32(carry_ptr), i32(carry_cols), i32(acc_ptr), i32(acc_cols)
        self.n_w, self.m_total, self.k_acc, self.m_next = int(n_w), int(m_total), ap.size - 1, int(m_next)
        self.device = device
        self._handle = C.c_void_p()
        args = (self.n_w, self.m_total, rows.size, _abi.ptr(rows), _abi.ptr(cp), _abi.ptr(cc), ap.size - 1,
                _abi.ptr(ap), _abi.ptr(ac), int(row0), self.m_next, C.byref(self._handle))
        if device is None:  # validation only: no HIP call, the handle refuses to run
            _abi.check(self._lib.qd_window_create_host(*args), "qd_window_create_host")
        else:
            _abi.check(self._lib.qd_window_create(int(device), *args), "qd_window_create")

    def set_blocks(self, blocks: int = 0) -> None:
        """Workgroups of later launches (0 = the default); results do not depend on it."""
        _abi.check(self._lib.qd_window_set_blocks(self._handle, int(blocks)), "qd_window_set_blocks")

    def advance(self, B: int, x, syn_full, acc_out=None, syn_next=None, stream=None) -> None:
        """Enqueue the step for B device-resident shots (uint8 tensors): x
        [B][n_w] or None, syn_full [B][m_total] (in place), acc_out [B][k_acc]
        or None, syn_next [B][m_next] or None."""
        B = int(B)
        for name, t, cols in (("x", x, self.n_w), ("syn_full", syn_full, self.m_total),
                              ("acc_out", acc_out, self.k_acc), ("syn_next", syn_next, self.m_next)):
            Decoder._check_device_buffer(self, name, t, "uint8", B * cols)
        if stream is None:
            stream = _current_stream(self.device or 0)
        _abi.check(self._lib.qd_window_advance_device(self._handle, B, _abi.ptr(x), _abi.ptr(syn_full),
                                                      _abi.ptr(acc_out), _abi.ptr(syn_next), C.c_void_p(stream)),
                   "qd_window_advance_device")

    def close(self) -> None:
        if getattr(self, "_handle", None) and self._handle.value:
            self._lib.qd_window_destroy(self._handle)
            self._handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class WindowedDecoder:
    """The windows of a plan on one device: one ``Decoder`` per distinct window
    graph (all non-final windows of a spacetime code share one), one
    ``WindowAdvance`` per window and one that stages the first window.
    `priors`: per column of the full graph (or a scalar); decoder_kwargs go to
    every Decoder (method, precision, max_iter, ms_scaling, logicals, device)."""

    def __init__(self, plan: WindowPlan, priors, **decoder_kwargs):
        self.plan = plan
        self.device = int(decoder_kwargs.get("device", 0))
        shared = {}
        self.decoders = []
        for w, pr in zip(plan.windows, plan.priors(priors)):
            key = (w.graph.shape, w.graph.indptr.tobytes(), w.graph.indices.tobytes(), pr.tobytes(), w.fold_blocks)
            if key not in shared:
                fold = dict(n_data=plan.n_data, fold_blocks=w.fold_blocks) if plan.n_data is not None else {}
                shared[key] = Decoder(w.graph, pr, **fold, **decoder_kwargs)
            self.decoders.append(shared[key])
        self.distinct = list(shared.values())
        w0 = plan.windows[0]
        empty, zero = np.zeros(0, np.int32), np.zeros(1, np.int32)
        self.stage = WindowAdvance(1, plan.m, empty, zero, empty, zero, empty, w0.row0, w0.m, device=self.device)
        self.bounds = [WindowAdvance(w.n, plan.m, w.carry_rows, w.carry_ptr, w.carry_cols, w.acc_ptr, w.acc_cols,
                                     w.next_row0, w.next_m, device=self.device) for w in plan.windows]
        self._osd_solvers = {}

    @property
    def final_decoder(self) -> Decoder:
        return self.decoders[-1]

    def _osd(self, B, dec, osd, llr, syn_w, st_w, x_w):
        """OSD's answer into x_w for the shots whose st_w lacks the BP-converged
        bit: a device kernel where osd["rows"] has one for the graph, else the
        host stage."""
        from .experiment import _osd_rows_for
        method, order = osd.get("method", "osd_cs"), int(osd.get("order", 0))
        rows = _osd_rows_for(dec, osd.get("rows", "auto"))
        if rows:
            dec.osd_device(B, llr=llr, method=method, order=order, syn=syn_w, status=st_w, osdw=x_w, rows=rows)
            return
        import torch
        from .osd import OsdSolver
        bad = torch.nonzero((st_w & 1) == 0).flatten()
        if bad.numel() == 0:
            return
        solver = self._osd_solvers.get(id(dec))
        if solver is None:
            solver = self._osd_solvers[id(dec)] = OsdSolver(dec.H, method, order, int(osd.get("threads", 0)))
        _, ow = solver.solve(syn_w.index_select(0, bad).cpu().numpy(),
                             llr.index_select(0, bad).double().cpu().numpy())
        x_w[bad] = torch.from_numpy(np.ascontiguousarray(ow, dtype=np.uint8)).to(x_w.device)

    def decode_device(self, B: int, syn, acc_out, x_full=None, iters=None, status=None, osd=None,
                      stop_before_final: bool = False):
        """Decode B shots window by window on torch's current stream.  syn
        (uint8 [B][m], the caller's own copy) is updated in place; acc_out
        (uint8 [B][k_acc]) is toggled by acc . x of every committed column;
        x_full (uint8 [B][n], optional) receives the committed solution.  iters
        (int32 [B]) = the sum over windows; status (uint8 [B]): the BP-converged
        bit is the AND over windows, the satisfied bit the final window's.
        osd = {"method", "order", "rows", "threads"}: x of the shots BP leaves
        open is OSD's answer in every window.  stop_before_final: the final
        window is staged but not decoded, and its syndrome (uint8 [B][m_final])
        is returned for the caller's own fused stage on ``final_decoder``."""
        import torch
        B = int(B)
        dev = syn.device
        u8 = dict(dtype=torch.uint8, device=dev)
        wins = self.plan.windows
        if iters is not None:
            iters.zero_()
        conv = torch.ones(B, **u8)
        st_w = torch.zeros(B, **u8)
        it_w = torch.zeros(B, dtype=torch.int32, device=dev)
        syn_w = torch.empty((B, wins[0].m), **u8)
        self.stage.advance(B, None, syn, None, syn_w)
        for k, w in enumerate(wins):
            if w.final and stop_before_final:
                break
            dec = self.decoders[k]
            x_w = torch.empty((B, w.n), **u8)
            llr = (torch.empty((B, w.n), dtype=torch.float32 if dec.precision == _abi.QD_F32 else torch.float64,
                               device=dev) if osd is not None else None)
            dec.decode_device(B, syn=syn_w, x=x_w, llr=llr, iters=it_w, status=st_w)
            if osd is not None:
                self._osd(B, dec, osd, llr, syn_w, st_w, x_w)
            if x_full is not None:
                x_full[:, torch.from_numpy(w.cols[w.committed]).to(dev)] = \
                    x_w[:, torch.from_numpy(w.committed).to(dev)]
            nxt = None if w.final else torch.empty((B, w.next_m), **u8)
            self.bounds[k].advance(B, x_w, syn, acc_out, nxt)
            if iters is not None:
                iters += it_w
            conv &= st_w
            syn_w = nxt if nxt is not None else syn_w
        if status is not None:
            status.copy_((conv & 1) if stop_before_final else ((conv & 1) | (st_w & 2)))
        return syn_w if stop_before_final else None

    def close(self) -> None:
        for d in self.distinct:
            d.close()
        for b in [self.stage] + self.bounds:
            b.close()
