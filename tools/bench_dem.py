"""Sampling + decoding a detector error model on one MI355X: the device fault
sampler (qd_sample_faults_device) and the batched BP decode behind it
(exp_ldpc_amd.experiment.DemPipeline's two launches), timed apart and together.
Diagnostic companion of bench.py (which measures BASELINE config 2).

Default DEM: dem.storage_experiment_dem of the n = 225 code at R = 3, p = 0.003;
2^18 shots per launch.  Every figure is HIP-event time around the launches on one
stream, after warm-up launches, as the median over --reps launches with the
spread (min, max).  Prints one JSON line:

  sampler_ms / decode_ms / total_ms   per path ("byte", "packed")
  shots_per_s                         sampling + decode, per path
  sampler_share                       sampler_ms / (sampler_ms + decode_ms), per path
  yardsticks (--yardsticks)           the storage-experiment sampler
                                      (sample_storage_kernel) on the same code, R and
                                      p, which draws the same number of Bernoulli
                                      words, and the host dem.sample_dem on the DEM

Usage: python tools/bench_dem.py [--dem FILE] [--shots N] [--reps K] [--yardsticks]
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


def _stat(ms):
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms), "n": len(ms)}


def _timed(fn, reps, warmup):
    """HIP-event ms of fn() (which only enqueues), per launch."""
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


def main():
    import numpy as np
    import torch
    from conftest import load_code
    from exp_ldpc_amd.decoder import Decoder
    from exp_ldpc_amd.dem import sample_dem, storage_experiment_dem
    from exp_ldpc_amd.experiment import DemPipeline
    ap = argparse.ArgumentParser()
    ap.add_argument("--dem", default=None, help="DEM text file (default: the storage experiment's, n = 225)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--p", type=float, default=0.003)
    ap.add_argument("--shots", type=int, default=1 << 18)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--bp_method", default="ms")
    ap.add_argument("--max_iter", type=int, default=30)
    ap.add_argument("--precision", default="f64", choices=["f32", "f64"])
    ap.add_argument("--yardsticks", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dem.py needs a GPU")
    code = load_code("hgp_12_3_4_s1234")
    hz, lz = code.checks.z, np.asarray(code.logicals.z) % 2
    if a.dem:
        with open(a.dem) as f:
            text, name = f.read(), os.path.basename(a.dem)
    else:
        text, name = storage_experiment_dem(hz, lz, a.rounds, a.p, a.p), f"storage_n225_R{a.rounds}_p{a.p}"
    opts = {"max_iter": a.max_iter, "bp_method": a.bp_method, "ms_scaling_factor": 0}
    pipe = DemPipeline(text, opts, precision=a.precision)
    dec, B = pipe.dec, a.shots
    dev = torch.device("cuda", 0)
    res = {"dem": name, "detectors": dec.m, "faults": dec.n, "observables": dec.k, "shots": B, "reps": a.reps,
           "warmup": a.warmup, "bp_method": a.bp_method, "max_iter": a.max_iter, "precision": a.precision,
           "timing": "HIP events around the launches, ms per launch of `shots` shots"}
    iters = torch.zeros(B, dtype=torch.int32, device=dev)
    status = torch.zeros(B, dtype=torch.uint8, device=dev)
    fail = torch.zeros(B, dtype=torch.uint8, device=dev)
    for path, packed in (("byte", False), ("packed", True)):
        dt = torch.int64 if packed else torch.uint8
        w = (lambda c: (c + 63) // 64) if packed else (lambda c: c)
        det = torch.empty((B, w(dec.m)), dtype=dt, device=dev)
        flt = torch.empty((B, w(dec.n)), dtype=dt, device=dev)
        shot0 = [0]

        def sample():
            dec.sample_faults_device(20250221, 0, shot0[0], B, det, flt, None, packed=packed)
            shot0[0] += B

        def decode():
            dec.decode_device(B, syn=det, readout=flt if dec.k else None, iters=iters, status=status,
                              fail=fail if dec.k else None, packed=packed)

        def both():
            sample()
            decode()

        s_ms = _timed(sample, a.reps, a.warmup)
        d_ms = _timed(decode, a.reps, a.warmup)
        t_ms = _timed(both, a.reps, a.warmup)
        sm, dm = statistics.median(s_ms), statistics.median(d_ms)
        res[path] = {"sampler_ms": _stat(s_ms), "decode_ms": _stat(d_ms), "total_ms": _stat(t_ms),
                     "shots_per_s": B / (statistics.median(t_ms) * 1e-3), "sampler_share": sm / (sm + dm),
                     "ler_last_launch": float(fail.float().mean().item()),
                     "bp_converged_frac": float((status & 1).float().mean().item())}
    if a.yardsticks:
        y = {}
        if not a.dem:
            # the storage-experiment sampler on the plain Hz graph: same code, R and p
            g = Decoder(hz, 0.01)
            m, n, R = g.m, g.n, a.rounds
            for path, packed in (("byte", False), ("packed", True)):
                if packed:
                    syn = torch.empty((B, ((R + 1) * m + 63) // 64), dtype=torch.int64, device=dev)
                    rd = torch.empty((B, (n + 63) // 64), dtype=torch.int64, device=dev)
                else:
                    syn = torch.empty((B, (R + 1) * m), dtype=torch.uint8, device=dev)
                    rd = torch.empty((B, n), dtype=torch.uint8, device=dev)
                ms = _timed(lambda: g.sample_storage_device(R, a.p, a.p, 20250221, 0, 0, B, syn, rd, packed=packed),
                            a.reps, a.warmup)
                y["sample_storage_kernel_ms_" + path] = _stat(ms)
        hb = min(B, 1 << 12)  # the host sampler, on fewer shots (it is the slow one)
        t0 = time.perf_counter()
        sample_dem(pipe.dem, hb, seed=1)
        y["host_sample_dem"] = {"shots": hb, "shots_per_s": hb / (time.perf_counter() - t0)}
        res["yardsticks"] = y
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
