"""layered_wave_kernel against the numpy model (tests/layered_model.py), bit for
bit: x, iters, status, corr, fail and the bytes of llr, in both precisions and
both placements.  Graphs, seeds and the conditions that keep a comparison from
passing vacuously: tests/layered_cases.py."""
import functools

import numpy as np
import pytest

import layered_cases as lc

pytestmark = pytest.mark.gpu

DTYPES = {"f32": np.float32, "f64": np.float64}
FIELDS = ("x", "iters", "status", "corr", "fail")
WANT = FIELDS + ("llr",)


def make_decoder(gname, precision, **kw):
    from exp_ldpc_amd.decoder import Decoder
    g = lc.graph(gname)
    return Decoder(g["H"], g["probs"], method="ms", precision=precision, logicals=g["lz"], n_data=g["n_data"],
                   fold_blocks=g["fold_blocks"], schedule="layered", **kw)


def run(dec, syn, base, rd, *, max_iter, ms_scaling, placement, syn_flags=0, want=WANT):
    dec.max_iter, dec.ms_scaling, dec.layered_placement = max_iter, ms_scaling, placement
    return dec.decode(syn, base=base, readout=rd, syn_flags=syn_flags, want=want)


def assert_equal(got, ref, what=""):
    for k in FIELDS:
        assert np.array_equal(got[k], ref[k]), f"{what}: {k} differs in {int((got[k] != ref[k]).sum())} places"
    assert got["llr"].dtype == ref["llr"].dtype
    assert got["llr"].tobytes() == ref["llr"].tobytes(), f"{what}: llr"


@functools.lru_cache(maxsize=None)
def seeded_reference(gname, precision, B, seed, max_iter, ms_scaling, clip=2.0 ** 64, syn_flags=0):
    syn, base, rd = lc.shots(gname, B, seed)
    ref = lc.model(gname, DTYPES[precision], max_iter, ms_scaling, clip).decode(None if syn_flags else syn, base, rd,
                                                                                syn_flags)
    for v in ref.values():
        v.setflags(write=False)
    return ref


@pytest.mark.parametrize("max_iter", lc.MAX_ITERS)
@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("gname", lc.GRAPHS)
def test_layered_matches_the_model_in_both_placements(gpu_available, gname, precision, max_iter):
    syn, base, rd = lc.shots(gname, 64)
    dec = make_decoder(gname, precision)
    try:
        for ms_scaling in lc.SCALINGS:
            ref = lc.reference(gname, precision, max_iter, ms_scaling)
            if max_iter == 8 and gname not in lc.MIXED_EXEMPT:
                assert lc.mixed(ref), lc.batch_kinds(ref)
            for placement in ("lds", "hbm"):
                got = run(dec, syn, base, rd, max_iter=max_iter, ms_scaling=ms_scaling, placement=placement)
                assert_equal(got, ref, what=f"a={ms_scaling} {placement}")
                assert dec.layered_info(placement)[0] == (placement == "hbm")
    finally:
        dec.close()


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("gname", ["hz225", "wide200"])
def test_results_do_not_depend_on_the_slots(gpu_available, gname, precision):
    """B = 1, 5, 65 with one and two workgroups: a workgroup decodes several
    shots, so state left over from the previous shot would show."""
    dec = make_decoder(gname, precision)
    try:
        for B in (1, 5, 65):
            ref = seeded_reference(gname, precision, B, 100 + B, 8, 0.625)
            syn, base, rd = lc.shots(gname, B, 100 + B)
            for slots in (1, 2):
                dec.set_layered_slots(slots)
                for placement in ("lds", "hbm"):
                    got = run(dec, syn, base, rd, max_iter=8, ms_scaling=0.625, placement=placement)
                    assert_equal(got, ref, what=f"B={B} slots={slots} {placement}")
                    assert dec.layered_info(placement)[3] == min(slots, B)
        dec.set_layered_slots(0)
        got = run(dec, syn, base, rd, max_iter=8, ms_scaling=0.625, placement="hbm")
        assert_equal(got, ref, what="default slots")
        assert dec.layered_info("hbm")[3] == 65  # the default, at most one per shot
    finally:
        dec.close()


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("gname", ["hz225", "h35"])
def test_a_small_clip_engages(gpu_available, gname, precision):
    clip = 2.0 ** 4
    syn, base, rd = lc.shots(gname, 64)
    ref = lc.reference(gname, precision, 8, 1.0, clip=clip)
    assert np.abs(ref["llr"]).max() == clip
    assert not np.array_equal(ref["llr"], lc.reference(gname, precision, 8, 1.0)["llr"])
    dec = make_decoder(gname, precision, layered_clip=clip)
    try:
        for placement in ("lds", "hbm"):
            assert_equal(run(dec, syn, base, rd, max_iter=8, ms_scaling=1.0, placement=placement), ref, what=placement)
    finally:
        dec.close()


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_syndromes_from_base_and_readout(gpu_available, precision):
    gname, B = "st225r2", 16
    assert lc.graph(gname)["fold_blocks"] == 3
    syn, base, rd = lc.shots(gname, B, 31)
    rng = np.random.default_rng(5)  # sparse rows, so the derived syndromes are decodable
    base = (rng.random(base.shape) < 0.02).astype(np.uint8)
    rd = (rng.random(rd.shape) < 0.02).astype(np.uint8)
    mdl = lc.model(gname, DTYPES[precision], 8, 0.625)
    dec = make_decoder(gname, precision)
    try:
        for flags, s in ((3, None), (1, syn), (2, syn)):
            ref = mdl.decode(s, base, rd, flags)
            assert flags != 3 or ref["status"].any()
            for placement in ("lds", "hbm"):
                got = run(dec, s, base, rd, max_iter=8, ms_scaling=0.625, placement=placement, syn_flags=flags)
                assert_equal(got, ref, what=f"flags {flags} {placement}")
    finally:
        dec.close()


def device_run(dec, precision, syn, base, rd, *, names=WANT, stream=None):
    """decode_device on torch tensors; only the outputs of `names` are passed."""
    import torch
    B = syn.shape[0]
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    lt = torch.float32 if precision == "f32" else torch.float64
    shapes = {"x": ((B, dec.n), torch.uint8), "corr": ((B, dec.n_data), torch.uint8), "llr": ((B, dec.n), lt),
              "iters": ((B,), torch.int32), "status": ((B,), torch.uint8), "fail": ((B,), torch.uint8)}
    out = {k: torch.full(shapes[k][0], 0xEE if shapes[k][1] == torch.uint8 else -5, dtype=shapes[k][1], device="cuda")
           for k in names}
    d_in = (dev(syn), dev(base), dev(rd))
    if stream is not None:
        torch.cuda.synchronize()  # inputs and fills were enqueued on the current stream
    dec.decode_device(B, syn=d_in[0], base=d_in[1], readout=d_in[2],
                      stream=None if stream is None else stream.cuda_stream, **out)
    out["_inputs"] = d_in  # alive until the results are read: a side stream's kernel still reads them
    return out


def to_host(out):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items() if not k.startswith("_")}


@pytest.mark.parametrize("placement", ["lds", "hbm"])
def test_null_outputs(gpu_available, placement):
    """Every output is nullable: each one alone gives the model's values, and a
    launch with none of them completes."""
    gname, precision = "hz225", "f64"
    syn, base, rd = lc.shots(gname, 64)
    ref = lc.reference(gname, precision, 8, 0.625)
    dec = make_decoder(gname, precision, max_iter=8, ms_scaling=0.625, layered_placement=placement)
    try:
        for name in WANT:
            got = to_host(device_run(dec, precision, syn, base, rd, names=(name,)))
            assert got[name].tobytes() == ref[name].tobytes(), name
        to_host(device_run(dec, precision, syn, base, rd, names=()))
        assert dec.decode(syn[:0], want=WANT)["x"].shape == (0, dec.n)  # B = 0 writes nothing
    finally:
        dec.close()


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_two_streams_on_one_handle_in_hbm(gpu_available, precision):
    import torch
    gname = "st225r2"
    refs = [lc.reference(gname, precision, 8, 0.625), seeded_reference(gname, precision, 3, 103, 8, 0.625)]
    batches = [lc.shots(gname, 64), lc.shots(gname, 3, 103)]
    dec = make_decoder(gname, precision, max_iter=8, ms_scaling=0.625, layered_placement="hbm")
    try:
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        torch.cuda.synchronize()
        outs = [device_run(dec, precision, *b, stream=s) for b, s in zip(batches, streams)]
        for out, ref in zip(outs, refs):
            assert_equal(to_host(out), ref)
    finally:
        dec.close()


@pytest.mark.parametrize("ms_scaling", [1.0, 0.625])
@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_one_iteration_on_disjoint_rows_is_one_flooding_iteration(gpu_available, precision, ms_scaling):
    """The anchor: rows that share no column and have at least two entries see
    the priors alone, under either schedule.  The flooding decode is the
    library's tested one, so this ties the new kernel's bytes to it."""
    from exp_ldpc_amd.decoder import Decoder
    g = lc.graph("disjoint")
    assert (np.diff(g["H"].indptr) >= 2).all() and (np.asarray(g["H"].sum(axis=0)) == 1).all()
    syn, base, rd = lc.shots("disjoint", 64)
    flood = Decoder(g["H"], g["probs"], method="ms", precision=precision, max_iter=1, ms_scaling=ms_scaling,
                    logicals=g["lz"], n_data=g["n_data"], fold_blocks=1)
    dec = make_decoder("disjoint", precision)
    try:
        want = flood.decode(syn, base=base, readout=rd, want=WANT)
        assert 0 < (want["status"] & 1).sum() < 64
        for placement in ("lds", "hbm"):
            got = run(dec, syn, base, rd, max_iter=1, ms_scaling=ms_scaling, placement=placement)
            assert_equal(got, want, what=placement)
    finally:
        flood.close()
        dec.close()


@pytest.mark.parametrize("precision", ["f32", "f64"])
@pytest.mark.parametrize("key", ["fb3g", "fg84"])
def test_forests_match_the_model(gpu_available, key, precision):
    """Forest graphs (rows of 17, columns of degree 9, lone degree-1 checks,
    isolated columns) at alpha = 1 and 12 iterations."""
    import forest_cases as fc
    from exp_ldpc_amd.decoder import Decoder
    from layered_model import LayeredModel
    bd = fc.bundle(key)
    H, probs, _ = bd.triple()
    syn = np.ascontiguousarray(bd.syn[:40])
    ref = LayeredModel(H, probs, DTYPES[precision], max_iter=12, ms_scaling=1.0).decode(syn)
    assert 0 < (ref["status"] == 3).sum()
    dec = Decoder(H, probs, method="ms", precision=precision, max_iter=12, ms_scaling=1.0, schedule="layered")
    try:
        for placement in ("lds", "hbm"):
            dec.layered_placement = placement
            got = dec.decode(syn, want=("x", "iters", "status", "llr"))
            for k in ("x", "iters", "status"):
                assert np.array_equal(got[k], ref[k]), (placement, k)
            assert got["llr"].tobytes() == ref["llr"].tobytes(), placement
    finally:
        dec.close()
