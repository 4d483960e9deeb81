"""relay_block_kernel against the numpy model (tests/relay_model.py), bit for bit:
x, iters, legs, status, corr, fail and the bytes of llr, in both precisions and
both placements, on the 3 x 5 graph, its 4 x 21 extension with a row of weight
17 (bp_block_kernel's generic rows too), Hz of the n = 225 code, its R = 2 spacetime
graph (324 x 891: the 256-thread strides wrap, fold_blocks 3) and the
[[144,12,12]] Hz.  Graphs, parameter sets and seeds: tests/relay_cases.py."""
import functools

import numpy as np
import pytest

import relay_cases as rc

pytestmark = pytest.mark.gpu

DTYPES = {"f32": np.float32, "f64": np.float64}
FIELDS = ("x", "iters", "legs", "status", "corr", "fail")
WANT = FIELDS + ("llr",)


def make_decoder(gname, precision, pset="mix", **over):
    from exp_ldpc_amd.decoder import Decoder
    g = rc.graph(gname)
    dec = Decoder(g["H"], g["probs"], method="ms", precision=precision, logicals=g["lz"], n_data=g["n_data"],
                  fold_blocks=g["fold_blocks"])
    kw = rc.relay_kwargs(gname, pset)
    kw.update(over)
    dec.set_relay(**kw)
    return dec


@functools.lru_cache(maxsize=None)
def reference(gname, precision, pset, B, seed, syn_flags=0):
    """The model's result on the batch, computed once and shared."""
    syn, base, rd = rc.shots(gname, B, seed)
    ref = rc.model(gname, pset, DTYPES[precision]).decode(None if syn_flags == 3 else syn, base, rd, syn_flags)
    for v in ref.values():
        v.setflags(write=False)
    return ref


def assert_equal(got, ref, rows=slice(None), what=""):
    for k in FIELDS:
        assert np.array_equal(got[k][rows], ref[k][rows]), f"{what}: {k}"
    assert got["llr"].dtype == ref["llr"].dtype
    assert got["llr"][rows].tobytes() == ref["llr"][rows].tobytes(), f"{what}: llr"


@pytest.mark.parametrize("pset", list(rc.PARAM_SETS))
@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("gname", rc.GRAPHS)
def test_relay_matches_the_model_in_both_placements(gpu_available, gname, precision, pset):
    B, seed = 64, rc.MIX_SEED[gname]
    ref = reference(gname, precision, pset, B, seed)
    if pset == "mix" and not gname.startswith("h35"):
        kinds = rc.mix_kinds(ref)
        assert all(kinds.values()), kinds
    if pset == "clip":  # the small clip engages
        assert np.abs(ref["llr"]).max() == 2.0 ** 10
    if pset == "wide":
        g = rc.relay_kwargs(gname, pset)["gammas"]
        assert g.min() < 0 and g.max() > 1 and rc.PARAM_SETS[pset]["stop_nconv"] > rc.PARAM_SETS[pset]["num_sets"] + 1
    syn, base, rd = rc.shots(gname, B, seed)
    dec = make_decoder(gname, precision, pset)
    try:
        for placement in ("lds", "hbm"):
            got = dec.relay(syn, base=base, readout=rd, placement=placement, want=WANT)
            assert_equal(got, ref, what=placement)
            assert dec.relay_info(placement)[0] == (placement == "hbm")
    finally:
        dec.close()


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("gname", rc.GRAPHS)
def test_small_batches(gpu_available, gname, precision):
    dec = make_decoder(gname, precision, "mix")
    try:
        for B in (1, 3):
            ref = reference(gname, precision, "mix", B, 100 + B)
            syn, base, rd = rc.shots(gname, B, 100 + B)
            for placement in ("lds", "hbm"):
                assert_equal(dec.relay(syn, base=base, readout=rd, placement=placement, want=WANT), ref,
                             what=f"B={B} {placement}")
    finally:
        dec.close()


def device_run(dec, precision, syn, base, rd, *, placement, syn_flags=0, status=None, fill=None, stream=None):
    """relay_device on torch tensors; outputs pre-filled with `fill` (name -> value)."""
    import torch
    B = next(a.shape[0] for a in (syn, base, rd) if a is not None)
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    fill = fill or {}
    lt = torch.float32 if precision == "f32" else torch.float64
    out = {"x": torch.full((B, dec.n), fill.get("x", 0), dtype=torch.uint8, device="cuda"),
           "corr": torch.full((B, dec.n_data), fill.get("corr", 0), dtype=torch.uint8, device="cuda"),
           "llr": torch.full((B, dec.n), fill.get("llr", 0.0), dtype=lt, device="cuda"),
           "iters": torch.full((B,), fill.get("iters", 0), dtype=torch.int32, device="cuda"),
           "legs": torch.full((B,), fill.get("legs", 0), dtype=torch.int32, device="cuda"),
           "status": torch.zeros(B, dtype=torch.uint8, device="cuda") if status is None else dev(status),
           "fail": torch.full((B,), fill.get("fail", 0), dtype=torch.uint8, device="cuda")}
    d_in = (dev(syn), dev(base), dev(rd))
    if stream is not None:
        torch.cuda.synchronize()  # inputs and fills were enqueued on the current stream
    dec.relay_device(B, syn=d_in[0], base=d_in[1], readout=d_in[2], syn_flags=syn_flags,
                     only_failed=status is not None, placement=placement,
                     stream=None if stream is None else stream.cuda_stream, **out)
    out["_inputs"] = d_in  # alive until the results are read: a side stream's kernel still reads them
    return out


def to_host(out):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items() if not k.startswith("_")}


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("gname", ["hz225", "st225r2"])
def test_two_workgroups_take_five_shots(gpu_available, gname, precision):
    """qd_relay_set_slots(2) with B = 5: a workgroup decodes several shots, so state
    left over from the previous shot would show."""
    B, seed = 5, rc.MIX_SEED[gname]
    ref = reference(gname, precision, "mix", B, seed)
    syn, base, rd = rc.shots(gname, B, seed)
    dec = make_decoder(gname, precision, "mix")
    try:
        dec.set_relay_slots(2)
        for placement in ("lds", "hbm"):
            got = to_host(device_run(dec, precision, syn, base, rd, placement=placement))
            assert_equal(got, ref, what=placement)
            assert dec.relay_info(placement)[3] == 2
        dec.set_relay_slots(0)
        got = to_host(device_run(dec, precision, syn, base, rd, placement="hbm"))
        assert_equal(got, ref)
        assert dec.relay_info("hbm")[3] == 5  # the default, at most one per shot
    finally:
        dec.close()


@pytest.mark.parametrize("alpha", [1.0, 0.625])
@pytest.mark.parametrize("pre_iter", [1, 20])
@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("gname", rc.GRAPHS)
def test_without_memory_relay_is_the_tested_min_sum_decode(gpu_available, gname, precision, pre_iter, alpha):
    """gamma0 = 0, num_sets = 0, clip not reached: every output equals
    Decoder.decode(method="ms", ms_scaling=alpha, max_iter=pre_iter), llr included."""
    from exp_ldpc_amd.decoder import Decoder
    g = rc.graph(gname)
    B = 32
    syn, base, rd = rc.shots(gname, B, 7)
    # a degree-1 row sends Big, beyond every finite clip: no clamp on the 3 x 5 graph
    clip = np.inf if gname.startswith("h35") else 2.0 ** 64
    bp = Decoder(g["H"], g["probs"], method="ms", precision=precision, max_iter=pre_iter, ms_scaling=alpha,
                 logicals=g["lz"], n_data=g["n_data"], fold_blocks=g["fold_blocks"])
    dec = make_decoder(gname, precision, gamma0=0.0, num_sets=0, pre_iter=pre_iter, alpha=alpha, clip=clip,
                       stop_nconv=1, gammas=None)
    try:
        want = bp.decode(syn, base=base, readout=rd, want=("x", "corr", "llr", "iters", "status", "fail"))
        assert np.abs(want["llr"]).max() < clip
        for placement in ("lds", "hbm"):
            got = dec.relay(syn, base=base, readout=rd, placement=placement, want=WANT)
            for k in ("x", "corr", "iters", "status", "fail"):
                assert np.array_equal(got[k], want[k]), (placement, k)
            assert got["llr"].tobytes() == want["llr"].tobytes(), placement
            assert (got["legs"] == 1).all()
    finally:
        bp.close()
        dec.close()


@pytest.mark.parametrize("syn_flags", [0, 3])
@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_generic_rows_of_both_kernels_on_the_weight_17_row(gpu_available, precision, syn_flags):
    """bp_block_kernel<T, 1, false, 0, 0> (the plan: test_relay_host.py) and
    relay_block_kernel at gamma = 0 against the numpy model on "h35w17": x, iters
    and the bytes of llr, with the syndrome given and derived from base and
    readout; some shots converge and some stay open."""
    from exp_ldpc_amd.decoder import Decoder
    g, w = rc.graph("h35w17"), rc.WIDE_ROW
    syn, base, rd = rc.wide_row_shots(syn_flags)
    ref = rc.wide_row_model(DTYPES[precision]).decode(syn, base, rd, syn_flags)
    assert 0 < (ref["status"] & 1).sum() < w["B"]
    bp = Decoder(g["H"], g["probs"], method="ms", precision=precision, max_iter=w["max_iter"], ms_scaling=w["alpha"],
                 logicals=g["lz"], n_data=g["n_data"], fold_blocks=g["fold_blocks"])
    dec = make_decoder("h35w17", precision, gamma0=0.0, num_sets=0, pre_iter=w["max_iter"], alpha=w["alpha"],
                       clip=np.inf, stop_nconv=1, gammas=None)
    try:
        runs = {"bp": bp.decode(syn, base=base, readout=rd, syn_flags=syn_flags, want=("x", "llr", "iters", "status"))}
        for placement in ("lds", "hbm"):
            runs[placement] = dec.relay(syn, base=base, readout=rd, syn_flags=syn_flags, placement=placement, want=WANT)
        for name, got in runs.items():
            print(name, got["iters"].tolist(), (got["status"] & 1).tolist())
            assert np.array_equal(got["x"], ref["x"]), name
            assert np.array_equal(got["iters"], ref["iters"]), name
            assert np.array_equal(got["status"] & 1, ref["status"] & 1), name
            assert got["llr"].dtype == ref["llr"].dtype and got["llr"].tobytes() == ref["llr"].tobytes(), name
    finally:
        bp.close()
        dec.close()


@pytest.mark.parametrize("placement", ["lds", "hbm"])
@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_only_failed_leaves_converged_shots_untouched(gpu_available, precision, placement):
    gname, B = "st225r2", 16
    seed = rc.MIX_SEED[gname]
    ref = reference(gname, precision, "mix", B, seed)
    syn, base, rd = rc.shots(gname, B, seed)
    status = (np.arange(B) % 2).astype(np.uint8)  # every other shot is marked BP-converged
    fill = {"x": 0xEE, "corr": 0xEE, "llr": -7.5, "iters": -5, "legs": -5, "fail": 0xEE}
    dec = make_decoder(gname, precision, "mix")
    try:
        got = to_host(device_run(dec, precision, syn, base, rd, placement=placement, status=status, fill=fill))
        skip, run = status == 1, status == 0
        for k, v in fill.items():
            assert (got[k][skip] == v).all(), k
        assert (got["status"][skip] == 1).all()
        assert_equal(got, ref, rows=run)
        # the host path: the same, with the caller's arrays as the skipped shots' contents
        host = dec.relay(syn, base=base, readout=rd, status=status, placement=placement, want=WANT,
                         out={"x": np.full((B, dec.n), 0xEE, np.uint8), "iters": np.full(B, -5, np.int32)})
        assert (host["x"][skip] == 0xEE).all() and (host["iters"][skip] == -5).all() and (host["status"][skip] == 1).all()
        assert_equal(host, ref, rows=run)
    finally:
        dec.close()


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("gname", ["hz225", "st225r2"])
def test_syndromes_from_base_and_readout(gpu_available, gname, precision):
    B, seed = 16, 31
    syn, base, rd = rc.shots(gname, B, seed)
    # sparse rows, so the derived syndromes are decodable
    rng = np.random.default_rng(5)
    base = (rng.random(base.shape) < 0.02).astype(np.uint8)
    rd = (rng.random(rd.shape) < 0.02).astype(np.uint8)
    mdl = rc.model(gname, "mix", DTYPES[precision])
    dec = make_decoder(gname, precision, "mix")
    try:
        for flags, s in ((3, None), (1, syn), (2, syn)):
            ref = mdl.decode(s, base, rd, flags)
            assert flags != 3 or ref["status"].any()  # derived syndromes alone: some shots are solved
            for placement in ("lds", "hbm"):
                got = dec.relay(s, base=base, readout=rd, syn_flags=flags, placement=placement, want=WANT)
                assert_equal(got, ref, what=f"flags {flags} {placement}")
    finally:
        dec.close()


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_two_streams_on_one_handle_in_hbm(gpu_available, precision):
    import torch
    gname = "st225r2"
    seed = rc.MIX_SEED[gname]
    refs = [reference(gname, precision, "mix", 64, seed), reference(gname, precision, "mix", 3, 103)]
    batches = [rc.shots(gname, 64, seed), rc.shots(gname, 3, 103)]
    dec = make_decoder(gname, precision, "mix")
    try:
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        torch.cuda.synchronize()
        outs = [device_run(dec, precision, *b, placement="hbm", stream=s) for b, s in zip(batches, streams)]
        for out, ref in zip(outs, refs):
            assert_equal(to_host(out), ref)
    finally:
        dec.close()
