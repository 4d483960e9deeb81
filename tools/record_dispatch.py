"""Record which kernels each decode configuration launches.

``python tools/record_dispatch.py [OUT.json]`` decodes B = 128 shots for every
row of ROWS on cuda:0 and writes ``Decoder.last_kernels()`` (BP, SSF, pre-pass;
rocprofv3's spelling, template arguments included) per row id to
tests/golden/dispatch_names.json.  The committed file is the record of what the
launch layer chose before the launch plan existed; tests/test_gpu_parity.py and
tests/test_gpu_large_codes.py decode the same rows and compare, and
tests/test_cpu_host.py asks the planner (qd_graph_plan) for the same rows on a
host-only graph.

Only ``Decoder`` calls are used, no dispatch logic of its own: the table says
what to decode, the library says what ran.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
GOLDEN = os.path.join(REPO, "tests", "golden")
OUT = os.path.join(GOLDEN, "dispatch_names.json")
B = 128

WAVE_GRAPH = "hgp_12_3_4_s1234"                       # n = 225, wave shape (2, 4, 7)
BLOCK_GRAPHS = ["hgp_24_3_4_s11", "hgp_36_3_4_s42_g4"]  # workgroup kernels, messages in LDS
LARGE_GRAPH = "hgp_80_3_4_s2025"                      # n = 10^4 (C4): LDS-resident / group / HBM slices


def _row(graph, method, precision, out, ssf, packed=False, options=None, occ=0, misaligned=False):
    options = dict(options or {})
    tag = [graph, method, precision, out, "ssf" if ssf else "bp"]
    if packed:
        tag.append("packed")
    tag += [f"{k}={v}" for k, v in options.items()]
    if occ:
        tag.append(f"occ={occ}")
    if misaligned:
        tag.append("misaligned")
    return {"id": "-".join(tag), "graph": graph, "method": method, "precision": precision, "out": out,
            "ssf": bool(ssf), "packed": bool(packed), "options": options, "occ": int(occ),
            "misaligned": bool(misaligned)}


def _rows():
    w, rows = WAVE_GRAPH, []
    for method in ("ms", "ps"):
        for precision in ("f32", "f64"):
            for out in ("lean", "x"):
                for ssf in (True, False):
                    rows.append(_row(w, method, precision, out, ssf))
    # packed rows: read by the triage on the two-pass path, expanded first elsewhere
    for precision in ("f32", "f64"):
        for ssf in (True, False):
            rows.append(_row(w, "ms", precision, "lean", ssf, packed=True))
    rows.append(_row(w, "ms", "f64", "x", True, packed=True))
    rows.append(_row(w, "ps", "f64", "lean", True, packed=True))
    rows.append(_row(w, "ms", "f64", "lean", True, packed=True, options={"compact": 0}))
    # options
    for ssf in (True, False):
        rows.append(_row(w, "ms", "f64", "lean", ssf, options={"compact": 0}))
    rows.append(_row(w, "ms", "f32", "lean", True, options={"compact": 0}))
    for kern in ("scan", "scan_gather", "scan_nosplit"):
        rows.append(_row(w, "ms", "f64", "lean", True, options={"ssf": kern}))
        rows.append(_row(w, "ms", "f32", "x", True, options={"ssf": kern}))
    for precision in ("f32", "f64"):
        rows.append(_row(w, "ms", precision, "lean", True, options={"ssf_fuse": 1}))
    rows.append(_row(w, "ms", "f64", "x", True, options={"ssf_fuse": 1}))
    rows.append(_row(w, "ms", "f64", "lean", True, options={"ssf_fuse": 1, "ssf": "scan"}))
    for precision in ("f32", "f64"):
        for ssf in (True, False):
            rows.append(_row(w, "ms", precision, "lean", ssf, occ=12))
    rows.append(_row(w, "ms", "f64", "lean", True, options={"compact": 0}, occ=12))
    rows.append(_row(w, "ms", "f64", "x", True, occ=12))
    rows.append(_row(w, "ps", "f64", "lean", True, occ=12))
    # a syndrome view that is not 16-B aligned: no triage
    for ssf in (True, False):
        rows.append(_row(w, "ms", "f64", "lean", ssf, misaligned=True))
    for graph in BLOCK_GRAPHS:
        for method in ("ms", "ps"):
            for precision in ("f32", "f64"):
                for ssf in (True, False):
                    rows.append(_row(graph, method, precision, "x", ssf))
        for precision in ("f32", "f64"):
            for ssf in (True, False):
                rows.append(_row(graph, "ms", precision, "x", ssf, options={"lds_kernel": 1}))
    g = LARGE_GRAPH
    for options in ({}, {"group_kernel": 1}, {"lds_kernel": 0, "group_kernel": 0}):
        for precision in ("f32", "f64"):
            for ssf in (True, False):
                rows.append(_row(g, "ms", precision, "x", ssf, options=options))
    for ssf in (True, False):
        rows.append(_row(g, "ps", "f32", "x", ssf))
    return rows


ROWS = _rows()
assert len({r["id"] for r in ROWS}) == len(ROWS)


def rows_of(graphs):
    return [r for r in ROWS if r["graph"] in graphs]


def load_graph(name):
    """(hz, hx, lz) of a tests/golden fixture."""
    import scipy.sparse as sp
    if name == LARGE_GRAPH:
        from exp_ldpc_amd import gf2
        d = np.load(os.path.join(GOLDEN, f"{name}_checks.npz"))

        def csr(p):
            return sp.csr_matrix((np.ones(d[p + "_indices"].size, np.uint8), d[p + "_indices"], d[p + "_indptr"]),
                                 shape=tuple(d[p + "_shape"]))
        hx, hz = csr("hx"), csr("hz")
        _, lz = gf2.css_logicals(hx, hz)
        return hz, hx, lz
    from exp_ldpc_amd.codes import read_quantum_code
    with open(os.path.join(GOLDEN, f"{name}.qecc")) as f:
        code = read_quantum_code(f)
    return code.checks.z, code.checks.x, code.logicals.z


def make_decoder(row, graph):
    from exp_ldpc_amd.decoder import Decoder
    hz, hx, lz = graph
    dec = Decoder(hz, 0.02, method=row["method"], precision=row["precision"], max_iter=20, flip_sets=hx,
                  ssf=row["ssf"], logicals=lz)
    for name, value in row["options"].items():
        dec.set_option(name, value)
    if row["occ"]:
        dec.set_wave_occupancy(row["occ"])
    return dec


def run_row(row, graph, dec=None):
    """Decode the row's B shots; (bp, ssf, pre) kernel names."""
    import torch

    from exp_ldpc_amd.decoder import pack_rows
    hz = graph[0]
    m, n = hz.shape
    dec = dec or make_decoder(row, graph)
    rng = np.random.default_rng(7)
    rd = (rng.random((B, n)) < 0.03).astype(np.uint8)
    syn = np.ascontiguousarray(((hz @ rd.T).T % 2).astype(np.uint8))
    if row["packed"]:
        syn_t = torch.from_numpy(pack_rows(syn).view(np.int64)).to("cuda")
        rd_t = torch.from_numpy(pack_rows(rd).view(np.int64)).to("cuda")
    else:
        rd_t = torch.from_numpy(rd).to("cuda")
        if row["misaligned"]:  # the rows start one byte into a buffer
            buf = torch.empty(B * m + 16, dtype=torch.uint8, device="cuda")
            syn_t = buf[1:1 + B * m]
            syn_t.copy_(torch.from_numpy(syn).reshape(-1).to("cuda"))
            assert syn_t.data_ptr() % 16 == 1
        else:
            syn_t = torch.from_numpy(syn).to("cuda")
    out = {"iters": torch.empty(B, dtype=torch.int32, device="cuda"),
           "status": torch.empty(B, dtype=torch.uint8, device="cuda"),
           "fail": torch.empty(B, dtype=torch.uint8, device="cuda")}
    if row["ssf"]:
        out["ssf_steps"] = torch.empty(B, dtype=torch.int32, device="cuda")
    if row["out"] == "x":
        out["x"] = torch.empty((B, n), dtype=torch.uint8, device="cuda")
    dec.decode_device(B, syn=syn_t, readout=rd_t, packed=row["packed"], **out)
    torch.cuda.synchronize()
    return list(dec.last_kernels())


def load_golden():
    with open(OUT) as f:
        return json.load(f)


def main(argv):
    out = argv[1] if len(argv) > 1 else OUT
    names, graphs = {}, {}
    for row in ROWS:
        if row["graph"] not in graphs:
            graphs[row["graph"]] = load_graph(row["graph"])
        names[row["id"]] = run_row(row, graphs[row["graph"]])
        print(row["id"], names[row["id"]], flush=True)
    with open(out, "w") as f:
        json.dump(names, f, indent=1)
        f.write("\n")
    print(f"{len(names)} rows -> {out}")


if __name__ == "__main__":
    main(sys.argv)
