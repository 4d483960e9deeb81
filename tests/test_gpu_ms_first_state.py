"""The compact min-sum kernel's start of a listed shot against the oracle: the
first check state comes from the host's table (ms_state0) instead of a check
pass over the priors, and rows holding a zero entry fix their parity in
registers.  iters, status, fail and ssf_steps equal the oracle's byte for byte
on the n = 225 code (BP + SSF) and on a ragged graph of another wave shape, for
batch sizes around the 64-shot tile and the 4-entry chunks, max_iter 1, 2, 3
and 50, light and heavy syndromes (shots ending at iteration 2, at 3 and
unconverged), equal / tied / all-zero / partly negative priors, a fixed
scaling, both precisions, byte and packed inputs, the 3-waves-per-SIMD build,
a misaligned buffer (one-pass kernel) and a second set_priors on one handle."""
import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

OUTS = (("iters", "int32"), ("status", "uint8"), ("ssf_steps", "int32"), ("fail", "uint8"))
BATCHES = (1, 63, 65, 257)
BMAX = max(BATCHES)


def _decode_device(dec, syn, rd, packed=False):
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
    return {k: v.cpu().numpy() for k, v in out.items()}, dec.last_kernels()


def _random_graph(rng, m, n, dmax=7, cmax=4):
    from exp_ldpc_amd.codes import make_check_matrix
    rows, colcount = [], np.zeros(n, int)
    for _ in range(m):
        d = int(rng.integers(1, dmax + 1))
        cand = [j for j in rng.permutation(n) if colcount[j] < cmax][:d]
        for j in cand:
            colcount[j] += 1
        rows.append(sorted(cand))
    return make_check_matrix(rows, n)


def _graph(which, code225):
    """(H, flip sets or None, logicals): the n = 225 code, or a ragged graph on
    the (2, 3, 8) wave shape (BP only)."""
    if which == "hgp225":
        return sp.csr_matrix(code225.checks.z), code225.checks.x, code225.logicals.z
    rng = np.random.default_rng(110170)
    H = sp.csr_matrix(_random_graph(rng, 110, 170))
    return H, None, (rng.random((3, 170)) < 0.05).astype(np.uint8)


def _priors(kind, n, p, rng):
    if kind == "equal":
        return np.full(n, 2 * p / 3)
    if kind == "tied":
        return rng.choice([0.5 * p, p, p, 2 * p], size=n)
    if kind == "zero":
        return np.full(n, 0.5)
    pr = rng.choice([0.5 * p, p, 2 * p], size=n)  # one negative prior LLR
    pr[n // 3] = 0.7
    return pr


def _shots(H, p, rng, B=BMAX):
    n = H.shape[1]
    e = (rng.random((B, n)) < p).astype(np.uint8)
    e[0, :] = 0
    e[0, n // 2] = 1  # B = 1 decodes a listed shot
    syn = (H @ e.T).T.astype(np.int64) % 2
    rd = e ^ (rng.random((B, n)) < 0.003)
    return syn.astype(np.uint8), rd.astype(np.uint8)


def _oracle(oracle_lib, H, gens, lz, probs, syn, rd, precision, max_iter, scaling=0.0):
    kw = dict(ssf=True, gens=gens, ssf_impl="fast") if gens is not None else {}
    return oracle_lib.decode(H, probs, syn, method="ms", precision=precision, max_iter=max_iter, ms_scaling=scaling,
                             lz=lz, readout=rd, want_llr=False, **kw)


def _same(got, ref, rows, tag):
    for key, _ in OUTS:
        assert np.array_equal(got[key], ref[key][:rows]), (tag, key)


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("which", ["hgp225", "ragged"])
def test_first_state_equals_the_oracle(gpu_available, oracle_lib, code225, which, precision):
    """Every prior kind x max_iter x error rate, each batch size a prefix of one
    257-shot batch (one oracle run per combination)."""
    from exp_ldpc_amd.decoder import Decoder
    H, gens, lz = _graph(which, code225)
    n = H.shape[1]
    rng = np.random.default_rng(5)
    seen = set()
    for p in (0.01, 0.1):
        syn, rd = _shots(H, p, rng)
        for kind in ("equal", "tied", "zero", "negative"):
            probs = _priors(kind, n, p, rng)
            dec = Decoder(H, probs, method="ms", precision=precision, max_iter=1, flip_sets=gens, logicals=lz)
            for max_iter in (1, 2, 3, 50):
                dec.max_iter = max_iter
                ref = _oracle(oracle_lib, H, gens, lz, probs, syn, rd, precision, max_iter)
                if kind == "equal" and max_iter == 50:
                    seen |= {("it", int(i)) for i in ref["iters"][ref["status"] == 3]}
                    seen |= {("unconverged",)} if (ref["status"] != 3).any() else set()
                for B in BATCHES:
                    got, (bp_k, _, pre_k) = _decode_device(dec, syn[:B], rd[:B])
                    assert "cmp_kernel" in bp_k and "triage" in pre_k, bp_k
                    _same(got, ref, B, (p, kind, max_iter, B))
            dec.close()
    # between them the two rates end listed shots at iteration 2, at 3 and unconverged
    assert {("it", 2), ("it", 3), ("unconverged",)} <= seen, seen


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_first_state_with_fixed_scaling_and_packed_rows(gpu_available, oracle_lib, code225, precision):
    """ms_scaling != 0 (iteration 1 stays in the BP kernel: no triage tables), and
    bit-packed input rows, on both graphs."""
    from exp_ldpc_amd.decoder import Decoder
    rng = np.random.default_rng(6)
    for which in ("hgp225", "ragged"):
        H, gens, lz = _graph(which, code225)
        for p in (0.01, 0.1):
            syn, rd = _shots(H, p, rng)
            probs = _priors("equal", H.shape[1], p, rng)
            for scaling, max_iter in ((0.625, 50), (0.625, 1), (0.0, 50), (0.0, 2)):
                dec = Decoder(H, probs, method="ms", precision=precision, max_iter=max_iter, ms_scaling=scaling,
                              flip_sets=gens, logicals=lz)
                ref = _oracle(oracle_lib, H, gens, lz, probs, syn, rd, precision, max_iter, scaling)
                for packed in (False, True):
                    for B in (65, BMAX):
                        got, (bp_k, _, _) = _decode_device(dec, syn[:B], rd[:B], packed=packed)
                        assert "cmp_kernel" in bp_k, bp_k
                        _same(got, ref, B, (which, p, scaling, max_iter, packed, B))
                dec.close()


def test_first_state_three_waves_per_simd_and_second_set_priors(gpu_available, oracle_lib, code225):
    """set_wave_occupancy(12) launches the OCC = 3 build of the f64 kernel; a
    second set_priors on the same handle rebuilds the table the kernel reads."""
    from exp_ldpc_amd.decoder import Decoder
    H, gens, lz = _graph("hgp225", code225)
    n = H.shape[1]
    rng = np.random.default_rng(7)
    syn, rd = _shots(H, 0.03, rng)
    dec = Decoder(H, _priors("equal", n, 0.03, rng), method="ms", precision="f64", max_iter=50, flip_sets=gens,
                  logicals=lz)
    dec.set_wave_occupancy(12)
    for kind in ("equal", "tied", "negative", "zero", "equal"):
        probs = _priors(kind, n, 0.03 if kind != "tied" else 0.01, rng)
        dec.set_priors(probs)
        for max_iter in (1, 2, 50):
            dec.max_iter = max_iter
            ref = _oracle(oracle_lib, H, gens, lz, probs, syn, rd, "f64", max_iter)
            got, (bp_k, _, _) = _decode_device(dec, syn, rd)
            assert "bp_ms_cmp_kernel<double, 2, 4, 7, true, 2, 3, 0>" in bp_k, bp_k
            _same(got, ref, BMAX, (kind, max_iter))
    dec.close()


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_misaligned_buffer_keeps_the_prior_rows(gpu_available, oracle_lib, code225, precision):
    """A syndrome view off the 16-B grid runs the one-pass kernel, which still
    starts from rows holding the priors: same bytes as the oracle."""
    import torch

    from exp_ldpc_amd.decoder import Decoder
    H, gens, lz = _graph("hgp225", code225)
    m, n = H.shape
    rng = np.random.default_rng(8)
    syn, rd = _shots(H, 0.02, rng)
    B = BMAX
    dev = torch.device("cuda", 0)
    sbuf = torch.zeros(B * m + 16, dtype=torch.uint8, device=dev)
    rbuf = torch.zeros(B * n + 16, dtype=torch.uint8, device=dev)
    sv, rv = sbuf[3:3 + B * m].view(B, m), rbuf[5:5 + B * n].view(B, n)
    sv.copy_(torch.from_numpy(syn))
    rv.copy_(torch.from_numpy(rd))
    for kind, max_iter in (("equal", 50), ("equal", 1), ("zero", 3), ("negative", 50)):
        probs = _priors(kind, n, 0.02, rng)
        dec = Decoder(H, probs, method="ms", precision=precision, max_iter=max_iter, flip_sets=gens, logicals=lz)
        out = {k: torch.full((B,), 77, dtype=getattr(torch, dt), device=dev) for k, dt in OUTS}
        dec.decode_device(B, syn=sv, readout=rv, **out)
        torch.cuda.synchronize()
        assert "bp_ms_wave_kernel" in dec.last_kernels()[0]
        ref = _oracle(oracle_lib, H, gens, lz, probs, syn, rd, precision, max_iter)
        _same({k: v.cpu().numpy() for k, v in out.items()}, ref, B, (kind, max_iter))
        dec.close()
