"""Numpy model of sliding-window decoding (exp_ldpc_amd/window.py),
written from the rule and not from the plan's tables: the tests hold the plan,
the advance kernel and the pipelines against it.

window_spans        the windows (start, size, final) of W layers committing C
advance_model       one qd_window_advance_device call on host arrays
windowed_model      a windowed decode of a layered graph with any per-window
                    decoder, window by window on a syndrome updated in place
"""
import numpy as np
import scipy.sparse as sp


def window_spans(T, W, C):
    """Non-final windows at 0, C, 2C, ... while start + W <= T; the final one at
    the next multiple of C, up to layer T.  W >= T + 1: the whole graph."""
    spans, a = [], 0
    if W < T + 1:
        while a + W <= T:
            spans.append((a, W, False))
            a += C
    spans.append((a, T + 1 - a, True))
    return spans


def column_layers(H, row_layer):
    Hd = np.asarray(sp.csr_matrix(H).toarray()) % 2
    layer = np.asarray(row_layer)
    return np.array([layer[np.flatnonzero(Hd[:, j])].min() for j in range(Hd.shape[1])])


def advance_model(x, syn_full, acc_out, carry_rows, carry_ptr, carry_cols, acc_ptr, acc_cols, row0, m_next):
    """Returns syn_next; syn_full and acc_out (either may be None) are updated in
    place.  x = None: only the copy.  Bit 0 of an x byte counts."""
    if x is not None:
        xb = np.asarray(x) & 1
        for i, g in enumerate(carry_rows):
            cols = carry_cols[carry_ptr[i]:carry_ptr[i + 1]]
            syn_full[:, g] ^= np.bitwise_xor.reduce(xb[:, cols], axis=1) if len(cols) else 0
        if acc_out is not None:
            for i in range(len(acc_ptr) - 1):
                cols = acc_cols[acc_ptr[i]:acc_ptr[i + 1]]
                acc_out[:, i] ^= np.bitwise_xor.reduce(xb[:, cols], axis=1) if len(cols) else 0
    return syn_full[:, row0:row0 + m_next].copy()


def windowed_model(H, row_layer, W, C, acc, syn, decode, stop_before_final=False):
    """Decode every window in turn.  decode(k, span, Hw, cols, syn_w) -> x_w
    (uint8 [B][len(cols)]).  Returns a dict: x (the committed solution, [B][n]),
    acc (acc x), syn (the full syndrome after the last carry), windows (per
    window: span, rows, cols, Hw, syn_w, x_w), and with stop_before_final the
    final window's (span, Hw, cols, syn_w) under "final" instead of its decode."""
    Hd = (np.asarray(sp.csr_matrix(H).toarray()) % 2).astype(np.uint8)
    A = (np.asarray(sp.csr_matrix(acc).toarray()) % 2).astype(np.uint8)
    layer = np.asarray(row_layer)
    cl = column_layers(Hd, layer)
    syn = np.array(syn, dtype=np.uint8, copy=True)
    B = syn.shape[0]
    x = np.zeros((B, Hd.shape[1]), np.uint8)
    out = {"windows": [], "final": None}
    for k, (a, size, final) in enumerate(window_spans(int(layer[-1]), W, C)):
        rows = np.flatnonzero((layer >= a) & (layer < a + size))
        cols = np.flatnonzero((cl >= a) & (cl < a + size))
        Hw = Hd[np.ix_(rows, cols)]
        syn_w = syn[:, rows].copy()
        if final and stop_before_final:
            out["final"] = ((a, size, final), Hw, cols, syn_w)
            break
        x_w = np.asarray(decode(k, (a, size, final), Hw, cols, syn_w), dtype=np.uint8) & 1
        commit = cols[cl[cols] < (a + size if final else a + C)]
        x[:, commit] = x_w[:, np.searchsorted(cols, commit)]
        # the committed columns leave every row that a later window reads
        later = np.flatnonzero(layer >= (a + size if final else a + C))
        syn[:, later] ^= (x[:, commit].astype(np.int64) @ Hd[np.ix_(later, commit)].T.astype(np.int64) % 2).astype(np.uint8)
        out["windows"].append(dict(span=(a, size, final), rows=rows, cols=cols, Hw=Hw, syn_w=syn_w, x_w=x_w))
    out["x"] = x
    out["acc"] = (x.astype(np.int64) @ A.T.astype(np.int64) % 2).astype(np.uint8)
    out["syn"] = syn
    return out
