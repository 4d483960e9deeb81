"""The OSD stage with its rows in HBM (osd_hbm_kernel, csrc/qdec_osd_hbm.hip) on
one MI355X.  Diagnostic companion of bench.py; numbers are recorded, nothing is
asserted except that the compared paths return the same bytes.

n = 225 code, min-sum f64, 30 iterations, osd_cs 7, circuit_noise(p) (default
0.003).  Device times are HIP events around the launch, warm, median and
[min, max] of --reps runs; host times are wall clock.

(a) host     the OSD stage on the circuit DEMs of R = 2 and R = 3, on the shots BP
             leaves unconverged in a 2^14-shot batch: the HBM kernel against the
             host stage (OsdSolver.solve, 16 threads) on the same shots and llr.
             The host stage runs once on the first --host_shots of them (it
             takes tens of ms per shot and thread); both are reported per shot.
(b) onchip   the R = 3 spacetime matrix 432 x 1224 (bposd mode, depolarizing
             0.03), which osd_block_kernel holds: on chip against forced HBM on
             the same shots; the ratio is the price of the placement.
(c) slots    slots per CU in {1, 2, 4, 8} on the R = 3 DEM.
(d) point    bposd_detector at R = 3, 2^14 shots end to end: wall time of the
             sampler, BP, OSD and the rest (host glue), beside the same point
             with osd_rows="host".

Prints one JSON line and writes it to profiles/osd_hbm/bench.json.

Usage: python tools/bench_osd_hbm.py [--shots N] [--reps K] [--p P] [--host_shots N] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

OPTS = {"max_iter": 30, "bp_method": "ms", "ms_scaling_factor": 0, "osd_method": "osd_cs", "osd_order": 7}


def _stat(ms):
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms), "n": len(ms)}


def _events(fn, reps, warmup=1):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def _say(*a):
    print(*a, file=sys.stderr, flush=True)


def _unconverged(dec, syn, readout=None):
    """BP with llr on the batch; (bad indices, syn, llr of the unconverged shots, BP ms)."""
    import torch
    B = syn.shape[0]
    dev = syn.device
    llr = torch.empty((B, dec.n), dtype=torch.float64, device=dev)
    status = torch.zeros(B, dtype=torch.uint8, device=dev)
    bp_ms = _events(lambda: dec.decode_device(B, syn=syn, readout=readout, llr=llr, status=status), 3)
    bad = torch.nonzero((status & 1) == 0).flatten()
    return bad, syn.index_select(0, bad).contiguous(), llr.index_select(0, bad).contiguous(), bp_ms


def _osd(dec, syn, llr, rows, reps, out=None):
    import torch
    nb = syn.shape[0]
    ow = out if out is not None else torch.zeros((nb, dec.n), dtype=torch.uint8, device=syn.device)
    ms = _events(lambda: dec.osd_device(nb, llr=llr, method="osd_cs", order=7, syn=syn, osdw=ow, rows=rows), reps)
    return ms, ow


def dem_pipe(code, R, p, **kw):
    from exp_ldpc_amd.experiment import BatchPipeline, _steps
    from exp_ldpc_amd.noise_model import circuit_noise
    from exp_ldpc_amd.storage_sim import build_storage_simulation
    xs, zs = _steps(code.checks)
    nm = circuit_noise(p)
    sim = build_storage_simulation(R, nm, code)
    pipe = BatchPipeline(code, R, "bposd_detector", OPTS, (2 * p / 3 * (xs + zs + 2), p * (zs + 2)), noise=nm,
                         precision="f64", sim=sim, **kw)
    return pipe, sim


def close(pipe):
    for dec in pipe.decoders() + [pipe.sampler_graph]:
        dec.close()


def against_host(code, R, a):
    import numpy as np
    import torch
    from exp_ldpc_amd.osd import OsdSolver
    pipe, sim = dem_pipe(code, R, a.p)
    dec = pipe.det
    det, rd = pipe.sample(sim, a.shots, a.seed, 0, 0)
    bad, syn, llr, bp_ms = _unconverged(dec, det)
    nb = int(bad.numel())
    _say(f"(a) R = {R}: {dec.m} x {dec.n}, {nb} of {a.shots} shots unconverged")
    ms, ow = _osd(dec, syn, llr, "hbm", a.reps)
    info = dec.osd_hbm_info()
    hs = min(nb, a.host_shots)
    solver = OsdSolver(pipe.dem.fault_check_matrix, "osd_cs", 7, 16)
    s_h, l_h = syn[:hs].cpu().numpy(), llr[:hs].cpu().numpy()
    t0 = time.perf_counter()
    _, hw = solver.solve(s_h, l_h)
    host_s = time.perf_counter() - t0
    same = bool(np.array_equal(ow[:hs].cpu().numpy(), hw))
    res = {"rounds": R, "m": dec.m, "n": dec.n, "shots": a.shots, "unconverged": nb, "bp_ms": _stat(bp_ms),
           "hbm_ms": _stat(ms), "hbm_us_per_shot": 1e3 * statistics.median(ms) / max(nb, 1),
           "slot_bytes": info[0], "slots": info[1], "host_threads": 16, "host_shots": hs, "host_s": host_s,
           "host_us_per_shot": 1e6 * host_s / max(hs, 1), "same_bytes": same,
           "speedup_per_shot": (host_s / max(hs, 1)) / (1e-3 * statistics.median(ms) / max(nb, 1))}
    _say(json.dumps(res))
    assert same, "the HBM kernel and the host stage disagree"
    keep = (pipe, sim, dec, syn, llr) if R == 3 else None
    if keep is None:
        close(pipe)
    return res, keep


def slots_sweep(dec, syn, llr, a):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    out = {"num_cus": cus, "per_cu": {}}
    for per in (1, 2, 4, 8):
        dec.set_osd_slots(cus * per)
        try:
            ms, _ = _osd(dec, syn, llr, "hbm", a.reps)
        except Exception as e:  # noqa: BLE001 - the scratch did not fit: recorded, not fatal
            out["per_cu"][per] = {"error": str(e)}
            continue
        out["per_cu"][per] = dict(_stat(ms), slots=dec.osd_hbm_info()[1], scratch_bytes=dec.osd_hbm_info()[2])
        _say(f"(c) {per} slots per CU: {out['per_cu'][per]}")
    dec.set_osd_slots(0)
    return out


def onchip_price(code, a):
    import numpy as np
    from exp_ldpc_amd.experiment import BatchPipeline
    from exp_ldpc_amd.noise_model import depolarizing_noise
    from exp_ldpc_amd.storage_sim import build_storage_simulation
    p = 0.03
    sim = build_storage_simulation(3, depolarizing_noise(p, p), code)
    pipe = BatchPipeline(code, 3, "bposd", OPTS, (2 * p / 3, 2 * p / 3))
    dec = pipe.st
    syn, rd = sim.sample_device(pipe.sampler_graph, a.shots, seed=a.seed, stream_id=1)
    bad, s, llr, _ = _unconverged(dec, syn, rd)
    on_ms, on = _osd(dec, s, llr, "onchip", a.reps)
    hb_ms, hb = _osd(dec, s, llr, "hbm", a.reps)
    same = bool(np.array_equal(on.cpu().numpy(), hb.cpu().numpy()))
    res = {"m": dec.m, "n": dec.n, "p": p, "shots": a.shots, "unconverged": int(bad.numel()),
           "onchip_kernel": dec.osd_kernel_info(), "onchip_ms": _stat(on_ms), "hbm_ms": _stat(hb_ms),
           "hbm_over_onchip": statistics.median(hb_ms) / statistics.median(on_ms), "same_bytes": same}
    _say("(b)", json.dumps(res))
    assert same, "the HBM kernel and the on-chip kernel disagree"
    close(pipe)
    return res


def point(pipe, sim, a, bp_ms, osd_ms):
    import torch

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, time.perf_counter() - t0
    out = {}
    fails = {}
    for rows in ("auto", "host"):
        pipe.osd_rows = rows
        (det, rd), ts = wall(lambda: pipe.sample(sim, a.shots, a.seed, 0, 0))
        res, tr = wall(lambda: pipe.run(det, rd))
        fails[rows] = res.fail
        out[rows] = {"sampler_s": ts, "run_s": tr, "failures": int(res.fail.sum()), "bp_converged": res.bp_converged}
        _say(f"(d) osd_rows = {rows}: {out[rows]}")
    bp, osd = 1e-3 * statistics.median(bp_ms), 1e-3 * statistics.median(osd_ms)
    total = out["auto"]["sampler_s"] + out["auto"]["run_s"]
    out["auto"]["shares"] = {"sampler": out["auto"]["sampler_s"] / total, "bp": bp / total, "osd": osd / total,
                             "host_glue": max(0.0, out["auto"]["run_s"] - bp - osd) / total}
    out["same_flags"] = bool((fails["auto"] == fails["host"]).all())
    out["host_over_auto"] = ((out["host"]["sampler_s"] + out["host"]["run_s"]) / total)
    assert out["same_flags"]
    return out


def main():
    import torch
    from conftest import load_code
    ap = argparse.ArgumentParser()
    ap.add_argument("--shots", type=int, default=1 << 14)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--p", type=float, default=0.003, help="circuit_noise strength")
    ap.add_argument("--seed", type=int, default=20250221)
    ap.add_argument("--host_shots", type=int, default=1024, help="shots the host stage is timed on in (a)")
    ap.add_argument("--skip_point", action="store_true", help="leave out (d)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "osd_hbm", "bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_osd_hbm.py needs a GPU")
    code = load_code("hgp_12_3_4_s1234")
    res = {"code": "hgp_12_3_4_s1234", "p": a.p, "reps": a.reps, "bp": "min-sum f64, 30 iterations", "osd": "osd_cs 7",
           "timing": "device ms by HIP events around the launch (warm); host seconds by wall clock"}
    res["against_host"] = []
    keep = None
    for R in (2, 3):
        r, k = against_host(code, R, a)
        res["against_host"].append(r)
        keep = k or keep
    pipe, sim, dec, syn, llr = keep
    res["slots_per_cu"] = slots_sweep(dec, syn, llr, a)
    if not a.skip_point:
        r3 = res["against_host"][-1]
        res["point_R3"] = point(pipe, sim, a, [r3["bp_ms"]["median"]], [r3["hbm_ms"]["median"]])
    close(pipe)
    res["against_onchip"] = onchip_price(code, a)
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
