"""Graphs, parameter sets and shots shared by the relay tests (test_relay_host.py,
test_gpu_relay.py, test_gpu_relay_pipelines.py).  The seeds of the "mix" batches
were chosen on the CPU, with the model, so that each batch holds a shot solved in
leg 0, one solved in a later leg, one never solved and one whose best solution
is not its first (mix_kinds; the GPU test asserts it before it compares)."""
from __future__ import annotations

import functools

import numpy as np
import scipy.sparse as sp

from conftest import load_code
from relay_model import RelayModel

P_SHOT = 0.04

# a degree-1 row (row 2) and degree-1 columns (0, 2, 3, 4)
H35 = np.array([[1, 1, 0, 1, 0],
                [0, 1, 1, 0, 0],
                [0, 0, 0, 0, 1]], np.uint8)


@functools.lru_cache(maxsize=None)
def graph(name):
    """-> dict(H, n_data, fold_blocks, lz, probs)."""
    if name == "h35":
        H, n_data, fb, lz = sp.csr_matrix(H35), 5, 1, np.array([[1, 0, 1, 0, 1]], np.uint8)
    elif name == "h35w17":
        # the 3 x 5 graph and one check of weight 17 on columns 4 .. 20 (4 x 21): the
        # smallest row past the unrolled 16, 8 instantiation of bp_block_kernel and
        # outside the wave shapes, so plain BP runs the generic <T, 1, *, 0, 0>
        Hw = np.zeros((4, 21), np.uint8)
        Hw[:3, :5] = H35
        Hw[3, 4:] = 1
        H, n_data, fb, lz = sp.csr_matrix(Hw), 21, 1, (np.arange(21)[None, :] % 3 == 0).astype(np.uint8)
    elif name == "hz225":
        code = load_code("hgp_12_3_4_s1234")
        H, n_data, fb, lz = sp.csr_matrix(code.checks.z), 225, 1, np.asarray(code.logicals.z) % 2
    elif name == "st225r2":  # 324 x 891: the 256-thread strides wrap; fold_blocks 3
        from exp_ldpc_amd.spacetime import SpacetimeCode
        code = load_code("hgp_12_3_4_s1234")
        H = sp.csr_matrix(SpacetimeCode(code.checks.z, 2).spacetime_check_matrix)
        n_data, fb, lz = 225, 3, np.asarray(code.logicals.z) % 2
    elif name == "bb144":
        from exp_ldpc_amd.lifted import bivariate_bicycle_code
        code = bivariate_bicycle_code(12, 6, [(3, 0), (0, 1), (0, 2)], [(0, 3), (1, 0), (2, 0)], compute_logicals=True)
        H, n_data, fb, lz = sp.csr_matrix(code.checks.z), 144, 1, np.asarray(code.logicals.z) % 2
    else:
        raise KeyError(name)
    n = H.shape[1]
    probs = P_SHOT * (0.5 + (np.arange(n) % 5) / 4.0)  # 0.02 .. 0.06: the solution weights differ
    return dict(H=H, n_data=n_data, fold_blocks=fb, lz=lz.astype(np.uint8), probs=probs)


GRAPHS = ("h35", "h35w17", "hz225", "st225r2", "bb144")
# name -> relay parameters and the interval the strengths are drawn from
PARAM_SETS = {
    "mix": dict(gamma0=0.125, pre_iter=8, num_sets=4, set_max_iter=8, stop_nconv=2, alpha=1.0, clip=2.0 ** 64,
                interval=(-0.25, 0.75)),
    "one_iter": dict(gamma0=0.125, pre_iter=1, num_sets=0, set_max_iter=1, stop_nconv=1, alpha=0.625, clip=2.0 ** 64,
                     interval=(0.0, 0.0)),
    # strengths below 0 and above 1; stop_nconv above num_sets + 1
    "wide": dict(gamma0=-0.25, pre_iter=8, num_sets=1, set_max_iter=1, stop_nconv=7, alpha=0.625, clip=2.0 ** 64,
                 interval=(-0.5, 1.5)),
    # a small clip that engages: strengths above 1 make the marginals grow from leg to leg
    "clip": dict(gamma0=0.125, pre_iter=8, num_sets=4, set_max_iter=8, stop_nconv=3, alpha=1.0, clip=2.0 ** 10,
                 interval=(-0.5, 1.5)),
}
# seeds of the B = 64 "mix" batch per graph, good in both precisions (chosen
# with the model; the 3 x 5 graph and its 4 x 21 extension are too small to
# hold all four kinds)
MIX_SEED = {"h35": 0, "h35w17": 0, "hz225": 4, "st225r2": 84, "bb144": 1}


def relay_kwargs(gname, pset):
    """Keyword arguments of Decoder.set_relay / RelayModel for a parameter set."""
    g = graph(gname)
    p = dict(PARAM_SETS[pset])
    lo, hi = p.pop("interval")
    n = g["H"].shape[1]
    p["gammas"] = np.random.Generator(np.random.PCG64(7)).uniform(lo, hi, (p["num_sets"], n))
    return p


def model(gname, pset, dtype, **over):
    g = graph(gname)
    kw = relay_kwargs(gname, pset)
    kw.update(over)
    return RelayModel(g["H"], g["probs"], dtype, n_data=g["n_data"], fold_blocks=g["fold_blocks"], logicals=g["lz"],
                      **kw)


def shots(gname, B, seed):
    """syn = H e of errors at P_SHOT, a random base row and the matching readout."""
    g = graph(gname)
    rng = np.random.default_rng(seed)
    m, n = g["H"].shape
    e = (rng.random((B, n)) < P_SHOT).astype(np.uint8)
    syn = (g["H"].dot(e.T.astype(np.int64)).T & 1).astype(np.uint8)
    base = (rng.random((B, g["n_data"])) < 0.1).astype(np.uint8)
    # readout = base ^ fold(e): the failure flag is the correction's logical error, so both values occur
    readout = base.copy()
    for t in range(g["fold_blocks"]):
        readout ^= e[:, t * g["n_data"]:(t + 1) * g["n_data"]]
    return syn, base, readout


# The generic rows of bp_block_kernel and relay_block_kernel on "h35w17": min-sum,
# max_iter = pre_iter, the same alpha.  Seeds chosen with the model so that in
# both precisions some of the 8 shots converge and some stay open, with the
# syndrome given (syn_flags 0) and derived from base and readout (syn_flags 3).
WIDE_ROW = dict(B=8, seed=0, max_iter=3, alpha=0.625)


def wide_row_shots(syn_flags):
    """(syn or None, base, readout) of the WIDE_ROW batch."""
    syn, base, rd = shots("h35w17", WIDE_ROW["B"], WIDE_ROW["seed"])
    if syn_flags == 0:
        return syn, base, rd
    rng = np.random.default_rng(5)  # sparse rows, so the derived syndromes are decodable
    return None, (rng.random(base.shape) < 0.05).astype(np.uint8), (rng.random(rd.shape) < 0.05).astype(np.uint8)


def wide_row_model(dtype):
    g = graph("h35w17")
    # clip = inf: the degree-1 row sends Big, beyond any finite clip
    return RelayModel(g["H"], g["probs"], dtype, gamma0=0.0, pre_iter=WIDE_ROW["max_iter"], num_sets=0,
                      alpha=WIDE_ROW["alpha"], clip=np.inf, n_data=g["n_data"], fold_blocks=1, logicals=g["lz"])


def mix_kinds(ref):
    """Which of the four kinds of shot a model result holds."""
    return {"leg0": bool((ref["first_leg"] == 0).any()), "later": bool((ref["first_leg"] > 0).any()),
            "never": bool((ref["found"] == 0).any()),
            "best_not_first": bool(((ref["found"] > 1) & (ref["best_leg"] != ref["first_leg"])).any())}
