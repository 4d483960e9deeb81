"""Detector-error-model extraction (dem.detector_error_model) on one MI355X: the
fault-propagation kernel (frame_fault_kernel, qd_circuit_faults_device), the host
composition, and the whole call, beside the numpy model as the yardstick.
Diagnostic companion of bench.py; numbers are recorded, nothing is asserted.

For the reference's R = 3 storage circuit of the n = 225 code
(tests/golden/storage_R3.txt.gz, depolarizing 0.01 / 0.01) and the generated
circuit_noise(p) R = 3 circuit (default p = 0.003), all detectors and Lz readout
as observables, warm, median and [min, max] of --reps runs:

* kernel_ms      the fault kernel over all noise faults, packed rows, HIP events
* compose_ms     dem.dem_from_symptoms on the symptoms copied to the host (wall)
* dem_ms         the whole detector_error_model call, gauge check included (wall)
* model_ms       tests/fault_model.py's propagation of the same faults (wall)
* setup_s        one BatchPipeline(bpd_detector, circuit DEM) construction, which
                 is what a run_simulation point pays before its first shot, and
                 the extraction's share of it

Prints one JSON line and writes it to profiles/circuit_dem/bench_circuit_dem.json.

Usage: python tools/bench_circuit_dem.py [--reps K] [--p P] [--rounds R] [--out FILE]
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


def _wall(fn, reps, warmup):
    import torch
    out = []
    for i in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warmup:
            out.append((time.perf_counter() - t0) * 1e3)
    return out


def _events(fn, reps, warmup):
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


def measure(name, cc, code, a):
    import fault_model
    import numpy as np
    import scipy.sparse as sp
    from exp_ldpc_amd.circuit import handle_fault_info
    from exp_ldpc_amd.dem import dem_from_symptoms, detector_error_model, fault_mechanisms
    L = sp.csr_matrix(np.asarray(code.logicals.z) % 2)
    obs = sp.hstack([sp.csr_matrix((L.shape[0], cc.num_measurements - L.shape[1]), dtype=L.dtype), L]).tocsr()
    prog = cc.with_groups({"detectors": cc.detectors, "observables": obs})
    D, K = prog.groups["detectors"].shape[0], obs.shape[0]
    noise, gauge = handle_fault_info(prog.handle(0))
    k_ms = _events(lambda: prog.fault_symptoms_device(kind=0, packed=True), a.reps, a.warmup)
    s = prog.fault_symptoms_device(kind=0, packed=True)
    det, ob = s["detectors"].cpu().numpy(), s["observables"].cpu().numpy()
    c_ms = _wall(lambda: dem_from_symptoms(prog, det, ob, D, K), a.reps, a.warmup)
    d_ms = _wall(lambda: detector_error_model(prog, detectors=prog.groups["detectors"], observables=obs), a.reps,
                 a.warmup)
    m_ms = _wall(lambda: fault_model.propagate(prog.num_qubits, prog.ops, prog.targets, 0), max(1, a.reps // 2), 0)
    dem = dem_from_symptoms(prog, det, ob, D, K)
    info = prog.validate()
    prog.close()
    return {"circuit": name, "qubits": info["qubits"], "measurements": info["measurements"],
            "instructions": info["instructions"], "lds_bytes": info["lds_bytes"], "noise_faults": noise,
            "gauge_faults": gauge, "mechanisms": int(fault_mechanisms(cc)[0].size), "columns": dem.num_errors,
            "detectors": D, "observables": K, "kernel_ms": _stat(k_ms), "compose_ms": _stat(c_ms),
            "dem_ms": _stat(d_ms), "model_ms": _stat(m_ms)}


def main():
    import torch
    from conftest import GOLDEN, load_code
    from exp_ldpc_amd.circuit import compile_circuit
    from exp_ldpc_amd.experiment import BatchPipeline, _steps
    from exp_ldpc_amd.noise_model import circuit_noise
    from exp_ldpc_amd.storage_sim import build_storage_simulation
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--p", type=float, default=0.003, help="circuit_noise strength")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "circuit_dem", "bench_circuit_dem.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_circuit_dem.py needs a GPU")
    code = load_code("hgp_12_3_4_s1234")
    R = a.rounds
    res = {"code": "hgp_12_3_4_s1234", "rounds": R, "reps": a.reps, "warmup": a.warmup,
           "timing": "ms; kernel_ms by HIP events around the launch, the rest wall clock with a device "
                     "synchronisation on either side"}
    with gzip.open(os.path.join(GOLDEN, f"storage_R{R}.txt.gz"), "rt") as f:
        res["golden_depolarizing"] = measure(f"tests/golden/storage_R{R}.txt.gz", compile_circuit(f.read()), code, a)
    nm = circuit_noise(a.p)
    sim = build_storage_simulation(R, nm, code)
    t0 = time.perf_counter()
    cc = sim.compiled()
    build_s = time.perf_counter() - t0
    res["circuit_noise"] = dict(measure(f"circuit_noise({a.p})", cc, code, a), p=a.p, build_and_compile_s=build_s)
    # one run_simulation point's setup on this path
    xs, zs = _steps(code.checks)
    opts = {"max_iter": 30, "bp_method": "ms", "ms_scaling_factor": 0, "osd_method": "osd_cs", "osd_order": 0}
    setup = []
    for _ in range(3):
        t0 = time.perf_counter()
        pipe = BatchPipeline(code, R, "bpd_detector", opts, (2 * a.p / 3 * (xs + zs + 2), a.p * (zs + 2)), noise=nm,
                             precision="f32")
        torch.cuda.synchronize()
        setup.append(time.perf_counter() - t0)
        for dec in pipe.decoders() + [pipe.sampler_graph]:
            dec.close()
    dem_s = res["circuit_noise"]["dem_ms"]["median"] * 1e-3
    res["circuit_noise"]["pipeline_setup_s"] = _stat(setup)
    res["circuit_noise"]["extraction_share_of_setup"] = dem_s / statistics.median(setup)
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
