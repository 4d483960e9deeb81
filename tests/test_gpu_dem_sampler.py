"""The device fault sampler (qd_sample_faults_device) and the batched DEM
pipeline on top of it, bit for bit against the numpy model of tests/dem_model.py
(draws, H e, F e) and the CPU oracle's BP."""
import numpy as np
import pytest
import scipy.sparse as sp

import dem_model
from conftest import load_code

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (3, 5, 0), (64, 63, 1), (65, 64, 2), (129, 130, 65), (40, 257, 3)]
OPTS = {"max_iter": 30, "bp_method": "ms", "ms_scaling_factor": 0}
DEM_SEED, DEM_B = 7, 256


def _torch():
    import torch
    return torch


def _problem(m, n, k, seed):
    """Random sparse H (m x n) and F (k x n) with the columns that can break a
    column walk: an all-zero one, a heavy one (weight 9 where m allows) and two
    identical ones; priors with 0, 1, 0.5 and values in 1e-3 .. 1e-1."""
    rng = np.random.default_rng(seed)
    H = np.zeros((m, n), np.uint8)
    for j in range(n):
        H[rng.choice(m, size=min(m, int(rng.integers(1, 4))), replace=False), j] = 1
    p = 10.0 ** rng.uniform(-3, -1, size=n)
    p[0] = 0.5
    if n >= 2:
        p[n - 1] = 1.0
        H[:, n - 1] = 0
        H[rng.choice(m, size=min(m, 9), replace=False), n - 1] = 1   # weight 9 (m >= 9), always fires
    if n >= 5:
        H[:, 1] = 0                  # never toggles a detector
        p[1] = 0.5
        H[:, 3] = H[:, 0]            # identical columns, both likely to fire
        p[3] = 0.5
        p[n // 2] = 0.0
    F = (rng.random((k, n)) < 0.3).astype(np.uint8) if k else None
    return sp.csr_matrix(H), F, p


def _sample(dec, B, seed, stream_id, shot0, packed, want_obs=True, want_faults=True):
    torch = _torch()
    dev = torch.device("cuda", dec.device)
    if packed:
        det = torch.full((B, (dec.m + 63) // 64), -1, dtype=torch.int64, device=dev)
        flt = torch.full((B, (dec.n + 63) // 64), -1, dtype=torch.int64, device=dev)
    else:
        det = torch.full((B, dec.m), 7, dtype=torch.uint8, device=dev)
        flt = torch.full((B, dec.n), 7, dtype=torch.uint8, device=dev)
    obs = torch.full((B, dec.k), 7, dtype=torch.uint8, device=dev) if want_obs and dec.k else None
    dec.sample_faults_device(seed, stream_id, shot0, B, det, flt if want_faults else None, obs, packed=packed)
    torch.cuda.synchronize()
    out = [det.cpu().numpy(), flt.cpu().numpy(), None if obs is None else obs.cpu().numpy()]
    if packed:
        out[0], out[1] = out[0].view(np.uint64), out[1].view(np.uint64)
    return out


def _pad_mask(bits):
    """uint64 mask of the padding bits in the last word of a packed row."""
    r = bits % 64
    return np.uint64(0) if r == 0 else np.uint64(((1 << 64) - 1) ^ ((1 << r) - 1))


@pytest.mark.parametrize("m,n,k", SHAPES)
def test_shapes_match_the_model(gpu_available, m, n, k):
    from exp_ldpc_amd.decoder import Decoder, pack_rows
    H, F, p = _problem(m, n, k, seed=100 + m)
    if m >= 9 and n >= 2:
        assert H[:, n - 1].sum() == 9
    if n >= 5:
        assert H[:, 1].sum() == 0 and (H[:, 3] != H[:, 0]).nnz == 0
        assert {0.0, 0.5, 1.0} <= set(p.tolist())
    dec = Decoder(H, p, logicals=F)
    B, seed, sid, shot0 = 130, 31337, 3, 12345
    det, flt, obs = dem_model.sample(H, F, p, seed, sid, shot0, B)
    if n >= 5:
        assert flt[:, n - 1].all() and not flt[:, n // 2].any() and 0 < flt[:, 0].sum() < B
    gd, gf, go = _sample(dec, B, seed, sid, shot0, packed=False)
    assert np.array_equal(gf, flt)
    assert np.array_equal(gd, det)
    if k:
        assert np.array_equal(go, obs)
    else:
        assert go is None
    pd, pf, po = _sample(dec, B, seed, sid, shot0, packed=True)
    assert np.array_equal(pd, pack_rows(gd)) and np.array_equal(pf, pack_rows(gf))
    assert not (pd[:, -1] & _pad_mask(m)).any() and not (pf[:, -1] & _pad_mask(n)).any()
    if k:
        assert np.array_equal(po, obs)
    # det alone (faults and obs are optional), both layouts
    assert np.array_equal(_sample(dec, B, seed, sid, shot0, False, want_obs=False, want_faults=False)[0], det)
    assert np.array_equal(_sample(dec, B, seed, sid, shot0, True, want_obs=False, want_faults=False)[0], pd)
    dec.close()


@pytest.fixture(scope="module")
def mid():
    """A 65 x 64 problem with every prior inside (0, 1) (decodable) for the
    counter and batching tests."""
    from exp_ldpc_amd.decoder import Decoder
    H, F, p = _problem(65, 64, 2, seed=5)
    p = np.clip(p, 1e-3, 0.5)
    p[p == 0.0] = 0.25
    dec = Decoder(H, p, logicals=F)
    yield H, F, p, dec
    dec.close()


def test_shot_counter_crosses_the_high_word(gpu_available, mid):
    H, F, p, dec = mid
    shot0 = 2 ** 32 - 3
    det, flt, obs = dem_model.sample(H, F, p, 9, 1, shot0, 8)
    for packed in (False, True):
        gd, gf, go = _sample(dec, 8, 9, 1, shot0, packed)
        if packed:
            from exp_ldpc_amd.decoder import unpack_rows
            gd, gf = unpack_rows(gd, dec.m), unpack_rows(gf, dec.n)
        assert np.array_equal(gd, det) and np.array_equal(gf, flt) and np.array_equal(go, obs)
    # the high word is read: shots 2^32 + i differ from shots i
    low = dem_model.sample(H, F, p, 9, 1, 0, 5)[1]
    assert not np.array_equal(flt[3:], low)


def test_batch_split_seed_and_stream(gpu_available, mid):
    H, F, p, dec = mid
    whole = _sample(dec, 200, 4, 2, 1000, False)
    a = _sample(dec, 77, 4, 2, 1000, False)
    b = _sample(dec, 123, 4, 2, 1077, False)
    for w, x, y in zip(whole, a, b):
        assert np.array_equal(w, np.concatenate([x, y]))
    assert np.array_equal(whole[1], dem_model.sample(H, F, p, 4, 2, 1000, 200)[1])
    assert not np.array_equal(_sample(dec, 200, 5, 2, 1000, False)[1], whole[1])  # other seed
    assert not np.array_equal(_sample(dec, 200, 4, 3, 1000, False)[1], whole[1])  # other stream
    one = _sample(dec, 1, 4, 2, 1000, True)
    from exp_ldpc_amd.decoder import pack_rows
    assert np.array_equal(one[0], pack_rows(whole[0][:1])) and np.array_equal(one[1], pack_rows(whole[1][:1]))
    assert np.array_equal(one[2], whole[2][:1])


def test_empty_batch_writes_nothing(gpu_available, mid):
    torch = _torch()
    H, F, p, dec = mid
    det = torch.full((4, dec.m), 7, dtype=torch.uint8, device="cuda:0")
    flt = torch.full((4, dec.n), 7, dtype=torch.uint8, device="cuda:0")
    obs = torch.full((4, dec.k), 7, dtype=torch.uint8, device="cuda:0")
    dec.sample_faults_device(1, 0, 0, 0, det, flt, obs)
    dec.sample_faults_device(1, 0, 0, 0, None, None, None)
    torch.cuda.synchronize()
    assert bool((det == 7).all()) and bool((flt == 7).all()) and bool((obs == 7).all())


def test_argument_errors(gpu_available, mid):
    from exp_ldpc_amd._abi import QdecError
    from exp_ldpc_amd.decoder import Decoder
    torch = _torch()
    H, F, p, dec = mid
    B = 4
    det = torch.zeros((B, dec.m), dtype=torch.uint8, device="cuda:0")
    obs = torch.zeros((B, 2), dtype=torch.uint8, device="cuda:0")

    def rc_of(fn):
        with pytest.raises(QdecError) as e:
            fn()
        return e.value.rc

    bare = Decoder(H, p)  # no logicals
    assert rc_of(lambda: bare.sample_faults_device(1, 0, 0, B, det, None, obs)) == -65
    assert rc_of(lambda: bare.sample_faults_device(1, 0, 0, B, None)) == -66
    words = torch.zeros((B + 1, (dec.m + 63) // 64), dtype=torch.int64, device="cuda:0")
    assert rc_of(lambda: bare.sample_faults_device(1, 0, 0, B, words.data_ptr() + 4, packed=True)) == -67
    assert rc_of(lambda: bare.sample_faults_device(1, 0, 0, -1, det)) == -60
    bare.close()
    folded = Decoder(H, p, n_data=32, fold_blocks=2)
    assert rc_of(lambda: folded.sample_faults_device(1, 0, 0, B, det)) == -64
    folded.close()
    # a prior of 1: the graph samples, and a decode says why it cannot run
    p1 = p.copy()
    p1[5] = 1.0
    certain = Decoder(H, p1)
    certain.sample_faults_device(1, 0, 0, B, det)
    torch.cuda.synchronize()
    it = torch.zeros(B, dtype=torch.int32, device="cuda:0")
    assert rc_of(lambda: certain.decode_device(B, syn=det, iters=it)) == -51
    certain.close()


# ---------------------------------------------------------------- the real shape
@pytest.fixture(scope="module")
def storage_dem():
    """storage_experiment_dem of the n = 225 code at R = 2, p = 0.01: text, the
    parsed matrices and the model's 256 shots."""
    from exp_ldpc_amd.dem import DetectorSpacetimeCode, storage_experiment_dem
    code = load_code("hgp_12_3_4_s1234")
    text = storage_experiment_dem(code.checks.z, np.asarray(code.logicals.z) % 2, 2, 0.01, 0.01)
    dem = DetectorSpacetimeCode(text)
    det, flt, obs = dem_model.sample(dem.fault_check_matrix, dem.fault_map, dem.fault_priors, DEM_SEED, 0, 0, DEM_B)
    # not a vacuous comparison: syndromes and observables are exercised
    assert (det.any(axis=1)).sum() >= DEM_B // 2
    assert obs.any()
    return text, dem, det, flt, obs


@pytest.fixture(scope="module")
def oracle_fail(storage_dem, oracle_lib):
    """Per precision: the oracle's BP decode of the model's detectors and the
    reference's flag any(obs ^ F x)."""
    text, dem, det, flt, obs = storage_dem
    out = {}
    Fm = dem.fault_map.toarray().astype(np.int64)
    for prec in ("f64", "f32"):
        ref = oracle_lib.decode(dem.fault_check_matrix, dem.fault_priors, det, method="ms", precision=prec,
                                max_iter=30, want_llr=False)
        fail = ((obs.astype(np.int64) + ref["x"].astype(np.int64) @ Fm.T) % 2).any(axis=1)
        out[prec] = (ref, fail)
    return out


def test_storage_dem_matches_the_model(gpu_available, storage_dem):
    from exp_ldpc_amd.decoder import Decoder, pack_rows
    from exp_ldpc_amd.dem import sample_dem_device
    text, dem, det, flt, obs = storage_dem
    dec = Decoder(dem.fault_check_matrix, dem.fault_priors, logicals=dem.fault_map)
    gd, gf, go = sample_dem_device(dec, DEM_B, DEM_SEED)
    assert np.array_equal(gf.cpu().numpy(), flt)
    assert np.array_equal(gd.cpu().numpy(), det) and np.array_equal(go.cpu().numpy(), obs)
    pd, pf, po = sample_dem_device(dec, DEM_B, DEM_SEED, packed=True)
    assert np.array_equal(pd.cpu().numpy().view(np.uint64), pack_rows(det))
    assert np.array_equal(pf.cpu().numpy().view(np.uint64), pack_rows(flt))
    assert np.array_equal(po.cpu().numpy(), obs)
    assert sample_dem_device(dec, 8, DEM_SEED, want_obs=False)[2] is None
    dec.close()


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_dem_pipeline_matches_the_oracle(gpu_available, storage_dem, oracle_fail, precision):
    from exp_ldpc_amd.experiment import DemPipeline
    text, dem, det, flt, obs = storage_dem
    ref, ref_fail = oracle_fail[precision]
    assert 0 < ref_fail.sum() < DEM_B
    pipe = DemPipeline(text, OPTS, precision=precision)
    res = {pk: pipe.run(DEM_B, DEM_SEED, packed=pk, want_detail=True) for pk in (True, False)}
    for pk, r in res.items():
        # the flag from this call's own samples and the oracle's decode of them
        assert np.array_equal(r.detail["det"], det) and np.array_equal(r.detail["obs"], obs), pk
        assert np.array_equal(r.fail, ref_fail), pk
        assert np.array_equal(r.detail["iters"], ref["iters"]) and np.array_equal(r.detail["status"], ref["status"])
    assert np.array_equal(res[True].fail, res[False].fail)
    assert np.array_equal(res[True].detail["iters"], res[False].detail["iters"])
    assert np.array_equal(res[True].detail["status"], res[False].detail["status"])
    assert res[True].bp_converged == int((ref["status"] & 1).sum())
    pipe.dec.close()


def test_run_dem_simulation_does_not_depend_on_the_batch(gpu_available, storage_dem, oracle_fail):
    from qldpc.misc import run_dem_simulation
    text = storage_dem[0]
    stats = {}
    a = run_dem_simulation(600, text, OPTS, seed=DEM_SEED, batch=256, stats=stats)
    b = run_dem_simulation(600, text, OPTS, seed=DEM_SEED, batch=600)
    assert a.dtype == bool and a.shape == (600,) and np.array_equal(a, b)
    assert np.array_equal(a[:DEM_B], oracle_fail["f64"][1])
    assert 0 < stats["bp_converged"] <= 600 and stats["iters_sum"] > 0


def test_per_shot_api_agrees(gpu_available, storage_dem, oracle_fail):
    """BPDetectorCorrect on concat(det, obs) is non-zero exactly where the
    pipeline's flag is set, on 8 shots of both outcomes."""
    from exp_ldpc_amd.experiment import BPDetectorCorrect, DemPipeline
    text, dem, det, flt, obs = storage_dem
    ref_fail = oracle_fail["f64"][1]
    bad, good = np.flatnonzero(ref_fail)[:4], np.flatnonzero(~ref_fail)
    pick = np.concatenate([bad, good[:8 - bad.size]])
    assert pick.size == 8 and ref_fail[pick].any() and not ref_fail[pick].all()
    pipe = DemPipeline(text, OPTS, precision="f64")
    fail = pipe.run(DEM_B, DEM_SEED).fail
    pipe.dec.close()
    w = BPDetectorCorrect(text, OPTS, precision="f64")
    for b in pick:
        corrected = w.readout_correction(np.concatenate([det[b], obs[b]]))
        assert bool(corrected.any()) == bool(fail[b]), b
