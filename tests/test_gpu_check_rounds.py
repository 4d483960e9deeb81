"""The min-sum check pass in three sweeps (qdec_bp_ms.h: every round's row loads,
then the minima and states, one zero test for all rounds, then the stores)
against the oracle, byte for byte in iters, status, fail and ssf_steps.

What the restructure can break is the zero-row branch of the f64 lean kernels,
which now serves every check round from one ballot, so the cases put rows with
zero entries into round 0 only (checks < 64), round 1 only and both, on the
n = 225 code at B = 2048, at 2, 3 and 50 iterations, through the compact kernel
and through the one-pass kernel (whose first check pass runs on the rows of
priors themselves); negative priors by round (rows whose parity comes from the
compares); the bench's uniform-prior call at p = 0.1 and p = 0.0178 with byte
and packed inputs, default and three-waves-per-SIMD build (every listed shot
takes the branch at iteration 2); and a graph with one check round and one
with four, f64 and f32.

A zero prior is probability 0.5, whose LLR log((1 - p) / p) is +0.  A prior of
-0 cannot be asked for (no probability has that LLR), and no message can be -0
either: every v2c message is a sum that starts from the prior, x + (-x) is +0,
and (+0) + (-0) is +0.  So the issue's -0 and mixed +0 / -0 rows cannot be built
through the decoder and are not here.

Every case checks first, on the oracle alone, that among the shots with a
non-zero syndrome at least 10 % converge at iteration >= 2 and at least 10 % do
not converge, and that the decode ran the instantiation the plan names."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import ssf_cases as sc

pytestmark = pytest.mark.gpu

OUTS = (("iters", "int32"), ("status", "uint8"), ("ssf_steps", "int32"), ("fail", "uint8"))
B225 = 2048
P_REST = 0.03  # the priors that are not the case's own: 2p/3 at p = 0.03
# shot b is drawn at error rate RATES[b % 4] * p: light and heavy shots side by side
RATES = (0.1, 0.35, 1.0, 2.0)


def _shots(H, B, p, seed):
    n = H.shape[1]
    rng = np.random.default_rng(seed)
    rate = (np.array(RATES)[np.arange(B) % 4] * p)[:, None]
    e = (rng.random((B, n)) < rate).astype(np.uint8)
    syn = np.ascontiguousarray(((H @ e.T).T % 2).astype(np.uint8))
    rd = (e ^ (rng.random((B, n)) < 0.003)).astype(np.uint8)
    return syn, rd


def _round_qubits(H, which, count=3):
    """`count` qubits whose checks all run in check round 0 (checks < 64), all
    in round 1, or `count` of each ("both")."""
    Hc = sp.csc_matrix(H)
    rounds = [set((Hc.indices[Hc.indptr[j]:Hc.indptr[j + 1]] // 64).tolist()) for j in range(H.shape[1])]
    pick = {r: [j for j, s in enumerate(rounds) if s == {r}][:count] for r in (0, 1)}
    assert len(pick[0]) == count and len(pick[1]) == count
    return {"round0": pick[0], "round1": pick[1], "both": pick[0] + pick[1]}[which]


def _priors(H, kind, which):
    probs = np.full(H.shape[1], 2 * P_REST / 3)
    probs[_round_qubits(H, which)] = {"zero": 0.5, "negative": 0.7}[kind]
    return probs


def _conditions(ref, syn, tag):
    nz = syn.any(axis=1)
    conv = (ref["status"] & 1).astype(bool)
    late, unconv = (nz & conv & (ref["iters"] >= 2)).sum(), (nz & ~conv).sum()
    assert late >= 0.1 * nz.sum() and unconv >= 0.1 * nz.sum(), (tag, int(late), int(unconv), int(nz.sum()))


def _oracle(oracle_lib, H, gens, lz, probs, syn, rd, precision, max_iter, tag):
    kw = dict(ssf=True, gens=gens, ssf_impl="fast") if gens is not None else {}
    ref = oracle_lib.decode(H, probs, syn, method="ms", precision=precision, max_iter=max_iter, lz=lz, readout=rd,
                            want_llr=False, **kw)
    _conditions(ref, syn, tag)
    return ref


def _decode(dec, syn, rd, packed=False):
    import torch

    from exp_ldpc_amd.decoder import pack_rows
    dev = torch.device("cuda", 0)
    B = syn.shape[0]
    out = {k: torch.full((B,), 77, dtype=getattr(torch, dt), device=dev) for k, dt in OUTS}

    def put(a):
        a = pack_rows(a).view(np.int64) if packed else a
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    dec.decode_device(B, syn=put(syn), readout=put(rd), packed=packed, **out)
    torch.cuda.synchronize()
    names = dec.last_kernels()
    assert names == dec.planned_kernels(B, packed=packed), names
    return {k: v.cpu().numpy() for k, v in out.items()}, names[0]


def _same(got, ref, tag):
    for key, _ in OUTS:
        assert np.array_equal(got[key], ref[key]), (tag, key, int((got[key] != ref[key]).sum()))


@functools.lru_cache(maxsize=None)
def _shots225(p, seed):
    from conftest import load_code
    return _shots(sp.csr_matrix(load_code("hgp_12_3_4_s1234").checks.z), B225, p, seed)


# error rate of the shots per prior kind, chosen on the oracle alone so that
# _conditions holds at 2, 3 and 50 iterations
P_SHOTS = {"zero": 0.03, "negative": 0.03}


@pytest.mark.parametrize("which", ["round0", "round1", "both"])
@pytest.mark.parametrize("kind", ["zero", "negative"])
def test_special_priors_by_check_round(gpu_available, oracle_lib, code225, kind, which):
    """Zero (+0) or negative priors on qubits whose checks all run in one check
    round, or in both: f64 lean, 2, 3 and 50 iterations, the compact kernel and
    the one-pass kernel."""
    from exp_ldpc_amd.decoder import Decoder
    H, gens, lz = sp.csr_matrix(code225.checks.z), code225.checks.x, code225.logicals.z
    probs = _priors(H, kind, which)
    syn, rd = _shots225(P_SHOTS[kind], 11)
    dec = Decoder(H, probs, method="ms", precision="f64", max_iter=50, flip_sets=gens, logicals=lz)
    for max_iter in (2, 3, 50):
        dec.max_iter = max_iter
        ref = _oracle(oracle_lib, H, gens, lz, probs, syn, rd, "f64", max_iter, (kind, which, max_iter))
        for compact, name in ((1, "bp_ms_cmp_kernel<double, 2, 4, 7, true, 2, 0, 0>"),
                              (0, "bp_ms_wave_kernel<double, 2, 4, 7, true, true, 2, 0>")):
            dec.set_option("compact", compact)
            got, bp_k = _decode(dec, syn, rd)
            assert name in bp_k, bp_k
            _same(got, ref, (kind, which, max_iter, compact))
    dec.close()


# the bench points' priors -> the error rate their shots are drawn at (at 0.0178
# itself fewer than 10 % of the shots stay unconverged)
P_UNIFORM = {0.1: 0.1, 0.0178: 0.03}


@pytest.mark.parametrize("p", sorted(P_UNIFORM))
def test_uniform_prior_bench_call(gpu_available, oracle_lib, code225, p):
    """The bench's decode (priors 2p/3, 50 iterations, BP + SSF): byte and
    packed inputs, the default build and the three-waves-per-SIMD build."""
    from exp_ldpc_amd.decoder import Decoder
    H, gens, lz = sp.csr_matrix(code225.checks.z), code225.checks.x, code225.logicals.z
    syn, rd = _shots225(P_UNIFORM[p], 12)
    dec = Decoder(H, 2 * p / 3, method="ms", precision="f64", max_iter=50, flip_sets=gens, logicals=lz)
    ref = _oracle(oracle_lib, H, gens, lz, np.full(H.shape[1], 2 * p / 3), syn, rd, "f64", 50, p)
    for occ, inst in ((0, "2, 0, 0>"), (12, "2, 3, 0>")):
        dec.set_wave_occupancy(occ)
        for packed in (False, True):
            got, bp_k = _decode(dec, syn, rd, packed=packed)
            assert "bp_ms_cmp_kernel<double, 2, 4, 7, true, " + inst in bp_k, bp_k
            _same(got, ref, (p, occ, packed))
    dec.close()


# graphs of ssf_cases with one and with four check rounds -> the shots' error rate
SHAPE_P = {"w128": 0.09, "w498": 0.05}


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("key", sorted(SHAPE_P))
def test_one_and_four_check_rounds(gpu_available, oracle_lib, key, precision):
    """RC = 1 and RC = 4 (two groups of two rounds), lean BP, both precisions,
    the compact and the one-pass kernel."""
    from exp_ldpc_amd.decoder import Decoder
    H, probs, L = sc.graph(key)
    rc, rv, drc = sc.wave_shape_of(key)
    syn, rd = _shots(H, 512, SHAPE_P[key], 13)
    dec = Decoder(H, probs, method="ms", precision=precision, max_iter=20, logicals=L)
    ref = _oracle(oracle_lib, H, None, L, probs, syn, rd, precision, 20, (key, precision))
    T = sc.TNAME[precision]
    for compact, name in ((1, f"bp_ms_cmp_kernel<{T}, {rc}, {rv}, {drc}, false, 0, 0, 0>"),
                          (0, f"bp_ms_wave_kernel<{T}, {rc}, {rv}, {drc}, false, true, 0, 0>")):
        dec.set_option("compact", compact)
        got, bp_k = _decode(dec, syn, rd)
        assert name in bp_k, bp_k
        _same(got, ref, (key, precision, compact))
    dec.close()
