"""The Pauli-frame circuit sampler (frame_sample_kernel, qd_circuit_sample_device)
on one MI355X, against its yardstick and inside run_simulation's loop.
Diagnostic companion of bench.py (which measures BASELINE config 2).

1. The frame kernel on the reference's R = 3 storage circuit of the n = 225 code
   (tests/golden/storage_R3.txt.gz, depolarizing 0.01 / 0.01), writing the
   ``syn`` and ``readout`` groups, byte and packed rows.  Yardstick: the
   storage-experiment sampler (sample_storage_kernel) on the same code, R, p and
   shots.  Both draw from the same distribution; the ratio is the price of
   simulating the circuit's gates instead of restating its noise events.
2. The sampler's share of sampling + decode in run_simulation's loop under
   circuit_noise(p) (default 0.003), R = 3, decoder mode ``bposd``: the sampler
   (StorageSim.sample_device, HIP events) and BatchPipeline.run (wall clock; it
   ends with a host synchronisation) on the same batch.

2^18 shots per launch, warm, median and [min, max] of --reps launches.  Prints
one JSON line and writes it to profiles/circuit_sampler/bench_circuit.json.

Usage: python tools/bench_circuit.py [--shots N] [--reps K] [--p P] [--out FILE]
"""
from __future__ import annotations

import argparse
import gzip
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


def _op_counts(cc):
    import numpy as np
    from exp_ldpc_amd.circuit import OPCODES
    names = {v: k for k, v in OPCODES.items()}
    out = {}
    for op, _, cnt, _ in cc.ops:
        d = out.setdefault(names[int(op)], {"instructions": 0, "targets": 0})
        d["instructions"] += 1
        d["targets"] += int(cnt)
    info = cc.validate()
    return {"by_opcode": out, "instructions": int(np.shape(cc.ops)[0]), "draw_sites": info["sites"],
            "philox_blocks_per_shot": info["sites"] // 4, "rand_sites": info["rand_sites"],
            "lds_bytes": info["lds_bytes"], "qubits": info["qubits"], "measurements": info["measurements"]}


def main():
    import torch
    from conftest import GOLDEN, load_code
    from exp_ldpc_amd.circuit import compile_circuit
    from exp_ldpc_amd.decoder import Decoder
    from exp_ldpc_amd.experiment import BatchPipeline, _steps
    from exp_ldpc_amd.noise_model import circuit_noise
    from exp_ldpc_amd.storage_sim import build_storage_simulation, storage_output_groups
    ap = argparse.ArgumentParser()
    ap.add_argument("--shots", type=int, default=1 << 18)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--p", type=float, default=0.003, help="circuit_noise strength of part 2")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skip-decode", action="store_true", help="part 1 only")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "circuit_sampler", "bench_circuit.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_circuit.py needs a GPU")
    code = load_code("hgp_12_3_4_s1234")
    hz = code.checks.z
    m, n = hz.shape
    B, R = a.shots, a.rounds
    dev = torch.device("cuda", 0)
    res = {"code": "hgp_12_3_4_s1234", "rounds": R, "shots": B, "reps": a.reps, "warmup": a.warmup,
           "timing": "HIP events around the launch, ms per launch of `shots` shots, unless stated"}

    # ---- 1. the golden circuit (depolarizing 0.01 / 0.01) against sample_storage_kernel
    with gzip.open(os.path.join(GOLDEN, f"storage_R{R}.txt.gz"), "rt") as f:
        cc = compile_circuit(f.read())
    cc = cc.with_groups(storage_output_groups(cc, m, m, n, R))
    g = Decoder(hz, 0.01)
    part1 = {"circuit": f"tests/golden/storage_R{R}.txt.gz", "p": 0.01, "program": _op_counts(cc)}
    for path, packed in (("byte", False), ("packed", True)):
        dt = torch.int64 if packed else torch.uint8
        w = (lambda c: (c + 63) // 64) if packed else (lambda c: c)
        out = {"syn": torch.empty((B, w((R + 1) * m)), dtype=dt, device=dev),
               "readout": torch.empty((B, w(n)), dtype=dt, device=dev)}
        f_ms = _timed(lambda: cc.sample_device(B, 20250221, packed=packed, out=out), a.reps, a.warmup)
        y_ms = _timed(lambda: g.sample_storage_device(R, 0.01, 0.01, 20250221, 0, 0, B, out["syn"], out["readout"],
                                                      packed=packed), a.reps, a.warmup)
        fm, ym = statistics.median(f_ms), statistics.median(y_ms)
        part1[path] = {"frame_sample_kernel_ms": _stat(f_ms), "sample_storage_kernel_ms": _stat(y_ms),
                       "ratio": fm / ym, "frame_shots_per_s": B / (fm * 1e-3)}
    res["golden_depolarizing"] = part1
    cc.close()

    # ---- 2. circuit_noise inside run_simulation's loop
    if not a.skip_decode:
        nm = circuit_noise(a.p)
        sim = build_storage_simulation(R, nm, code)
        t0 = time.perf_counter()
        cn = sim.compiled()
        compile_s = time.perf_counter() - t0
        xs, zs = _steps(code.checks)
        dp, mp = 2 * a.p / 3 * (xs + zs + 2), a.p * (zs + 2)
        opts = {"max_iter": 30, "bp_method": "ms", "ms_scaling_factor": 0, "osd_method": "osd_cs", "osd_order": 0}
        pipe = BatchPipeline(code, R, "bposd", opts, (dp, mp), noise=nm)
        out = (torch.empty((B, (R + 1) * m), dtype=torch.uint8, device=dev),
               torch.empty((B, n), dtype=torch.uint8, device=dev))
        shot0 = [0]

        def sample():
            sim.sample_device(pipe.sampler_graph, B, 20250221, 0, shot0[0], out=out)
            shot0[0] += B

        s_ms = _timed(sample, a.reps, a.warmup)
        d_ms, fails = [], []
        for i in range(a.warmup + a.reps):
            sample()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = pipe.run(*out)
            torch.cuda.synchronize()
            if i >= a.warmup:
                d_ms.append((time.perf_counter() - t0) * 1e3)
                fails.append(float(r.fail.mean()))
        sm, dm = statistics.median(s_ms), statistics.median(d_ms)
        res["circuit_noise_run_simulation"] = {
            "p": a.p, "decoder_mode": "bposd", "bp_osd_options": opts, "data_prior": dp, "meas_prior": mp,
            "program": _op_counts(cn), "build_and_compile_s": compile_s,
            "sampler_ms": _stat(s_ms), "decode_ms_wall": _stat(d_ms), "sampler_share": sm / (sm + dm),
            "shots_per_s": B / ((sm + dm) * 1e-3), "ler": statistics.mean(fails)}
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
