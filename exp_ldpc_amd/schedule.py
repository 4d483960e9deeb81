"""Gate schedule and circuit text of the storage experiment.

``edge_color_bipartite`` properly colours the edges of a Tanner graph with
exactly Delta colours, Delta its largest degree (König's theorem; the classical
constructive proof: colour the edges one at a time, and when the colour free at
one end is taken at the other, swap the two colours along the alternating path
that starts there).  One colour is one layer of two-qubit gates in which no
qubit appears twice, so a check matrix is measured in Delta layers -- the
``x_steps`` / ``z_steps`` the phenomenological priors already assume
(``experiment._steps``).  The colouring need not equal the reference's
(``python/qldpc/edge_coloring.py``): any proper Delta-colouring gives a valid
circuit of the same depth.

``storage_circuit_text`` writes the storage experiment in the shape of the
reference's ``build_storage_simulation`` (``storage_sim.py:110-199``): data
reset; per round RX, the CX layers, MRX, then RX, the CZ layers, MRX; the first
round's detectors, the REPEAT body comparing consecutive rounds, the
transversal readout with the final detectors and the observables.
"""
from __future__ import annotations

from typing import List, Tuple

import numpy as np
import scipy.sparse as sp

from .codes import CircuitTargets

__all__ = ["edge_color_bipartite", "perfect_round", "storage_circuit_text"]


def edge_color_bipartite(H) -> List[List[Tuple[int, int]]]:
    """Colour classes of the bipartite graph of H (rows = checks, columns =
    qubits): a list of Delta lists of (row, column) edges, every edge in exactly
    one, no row and no column twice in a list."""
    H = sp.csr_matrix(H)
    m, n = H.shape
    coo = H.tocoo()
    edges = sorted((int(i), int(j)) for i, j, v in zip(coo.row, coo.col, coo.data) if v)
    if not edges:
        return []
    deg_r = np.bincount([e[0] for e in edges], minlength=m)
    deg_c = np.bincount([e[1] for e in edges], minlength=n)
    delta = int(max(deg_r.max(), deg_c.max()))
    at_row = -np.ones((m, delta), dtype=np.int64)  # at_row[i, c] = the column joined to row i by colour c
    at_col = -np.ones((n, delta), dtype=np.int64)
    for i, j in edges:
        a = int(np.flatnonzero(at_row[i] < 0)[0])  # free at the row (its degree is at most delta)
        b = int(np.flatnonzero(at_col[j] < 0)[0])  # free at the column
        if at_col[j, a] >= 0:
            # a is taken at column j.  Walk the path j -a- row -b- column -a- ... ; it
            # cannot reach row i (it enters rows by colour a, which is free at i),
            # so swapping a and b along it frees a at j and keeps the colouring proper.
            path, col, c = [], j, a
            while True:
                row = int(at_col[col, c])
                if row < 0:
                    break
                path.append((row, col, c))
                c = b if c == a else a
                col2 = int(at_row[row, c])
                if col2 < 0:
                    break
                path.append((row, col2, c))
                c = b if c == a else a
                col = col2
            for row, col, c in path:
                at_row[row, c] = -1
                at_col[col, c] = -1
            for row, col, c in path:
                c2 = b if c == a else a
                at_row[row, c2] = col
                at_col[col, c2] = row
        at_row[i, a] = j
        at_col[j, a] = i
    return [[(i, int(at_row[i, c])) for i in range(m) if at_row[i, c] >= 0] for c in range(delta)]


def _ints(qs) -> str:
    return " ".join(str(int(q)) for q in qs)


def perfect_round(code) -> Tuple[CircuitTargets, List[str]]:
    """One noiseless round of syndrome extraction, X checks then Z checks: qubits
    0 .. n - 1 are data, then one ancilla per X check, then one per Z check.  An
    ancilla prepared in |+> controls a CX (X check) or a CZ (Z check) on each
    qubit of its check, a colour class per layer, and is measured in X.  The
    last line carries no TICK, so the caller decides what follows."""
    hx, hz = sp.csr_matrix(code.checks.x), sp.csr_matrix(code.checks.z)
    n = hx.shape[1]
    xa = list(range(n, n + hx.shape[0]))
    za = list(range(n + hx.shape[0], n + hx.shape[0] + hz.shape[0]))
    lines: List[str] = []
    for gate, anc, H in (("CX", xa, hx), ("CZ", za, hz)):
        if not anc:
            continue
        lines += [f"RX {_ints(anc)}", "TICK"]
        for layer in edge_color_bipartite(H):
            lines += [f"{gate} " + " ".join(f"{anc[i]} {j}" for i, j in layer), "TICK"]
        lines.append(f"MRX {_ints(anc)}")
    return CircuitTargets(list(range(n)), xa, za), lines


def storage_circuit_text(rounds: int, noise_model, code, use_x_logicals: bool = False):
    """(targets, lines): prepare logical 0 (or + with use_x_logicals), run
    `rounds` rounds of syndrome extraction, read the data out transversally;
    the noiseless text passed through ``noise_model.rewrite``."""
    targets, body = perfect_round(code)
    hx, hz = sp.csr_matrix(code.checks.x), sp.csr_matrix(code.checks.z)
    mx, mz, n = hx.shape[0], hz.shape[0], hx.shape[1]
    per = mx + mz
    basis = "X" if use_x_logicals else "Z"
    H = hx if use_x_logicals else hz
    L = code.logicals.x if use_x_logicals else code.logicals.z
    L = sp.csr_matrix(L)
    first = 0 if use_x_logicals else mx  # the decoded sector's first record inside a round
    count = mx if use_x_logicals else mz
    lines = [f"R{basis} {_ints(targets.data)}", "TICK"]
    if rounds > 0:
        lines += body
        # the state starts as a product state in this basis: only its sector is deterministic
        lines += [f"DETECTOR(0, {first + i}) rec[{first + i - per}]" for i in range(count)]
        if rounds > 1:
            lines += ["TICK", f"REPEAT {rounds - 1} {{"] + body + ["SHIFT_COORDS(1, 0)"]
            lines += [f"DETECTOR(0, {i}) rec[{i - per}] rec[{i - 2 * per}]" for i in range(per)]
            lines += ["TICK", "}"]
    lines.append(f"M{basis} {_ints(targets.data)}")
    for i in range(count):
        recs = [f"rec[{first + i - n - per}]"] if rounds > 0 else []
        recs += [f"rec[{int(j) - n}]" for j in H.indices[H.indptr[i]:H.indptr[i + 1]]]
        lines.append(f"DETECTOR(1, {i}) " + " ".join(recs))
    for i in range(L.shape[0]):
        sup = L.indices[L.indptr[i]:L.indptr[i + 1]][L.data[L.indptr[i]:L.indptr[i + 1]] % 2 == 1]
        lines.append(f"OBSERVABLE_INCLUDE({i}) " + " ".join(f"rec[{int(j) - n}]" for j in sup))
    return targets, list(noise_model.rewrite(targets, lines))
