"""The Pauli frame in HBM (frame_sample_kernel / frame_fault_kernel with FrameInHbm,
csrc/qdec_frame.hip) on one MI355X.  Diagnostic companion of bench.py.

(a) The n = 225, R = 3 circuit_noise circuit, which fits LDS, under the LDS
    placement and under forced HBM placement: the price of the placement.
(b) The n = 10^4 code's circuit (biregular_hgp(80, 3, 4, seed = 2025), config 4)
    at R = 1 and R = 3, p = 0.001 and 0.01, with W = 1, 2, 4, 8 slots (resident
    one-wave workgroups) per compute unit: shots/s, the fastest W, and the slot
    working set against the 256 MiB Infinity Cache.  README's config-4 decode
    rates are printed beside them: which of sampler and decoder bounds a
    circuit-noise sweep of that code.  The parent commit refuses these circuits,
    so there is nothing to compare against.
(c) Fault propagation of the n = 10^4, R = 1 circuit in faults/s (a window of
    --faults noise faults, packed rows), and the host time of composing its DEM
    (dem.detector_error_model over all of the circuit's detectors, wall clock,
    once, with the host's peak memory; skipped with --skip-dem).

Packed output rows, HIP events around the launch, --warmup warm launches, then
median and [min, max] of --reps.  Prints one JSON line and writes it to
profiles/frame_hbm/bench.json.

Usage: python tools/bench_circuit_frame.py [--parts abc] [--skip-dem] [--shots N] [--reps K] [--out FILE]
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

# README "Numbers", config 4 (BP + SSF + logical check, R = 0), shots/s at p = 0.005 / 0.01 / 0.03
README_C4_DECODE = {"f64": {"0.005": 4.97e6, "0.01": 2.73e6, "0.03": 369e3},
                    "f32": {"0.005": 8.15e6, "0.01": 4.40e6, "0.03": 540e3}}
INFINITY_CACHE = 256 << 20


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


def _sampler(cc, B, frame, reps, warmup):
    import torch
    dev = torch.device("cuda", 0)
    out = {k: torch.empty((B, (m.shape[0] + 63) // 64), dtype=torch.int64, device=dev) for k, m in cc.groups.items()}
    ms = _timed(lambda: cc.sample_device(B, 20250221, packed=True, out=out, frame=frame), reps, warmup)
    return {"ms": _stat(ms), "shots_per_s": B / (statistics.median(ms) * 1e-3)}


def main():
    import torch
    from conftest import load_checks, load_code, load_logicals
    from exp_ldpc_amd.circuit import handle_fault_info
    from exp_ldpc_amd.codes import QuantumCode, QuantumCodeChecks, QuantumCodeLogicals
    from exp_ldpc_amd.noise_model import circuit_noise
    from exp_ldpc_amd.storage_sim import build_storage_simulation
    ap = argparse.ArgumentParser()
    ap.add_argument("--shots", type=int, default=1 << 18,
                    help="shots per launch of (b): at least 2 x 64 x 8 slots per CU x CUs, so that every slot is reused")
    ap.add_argument("--small-shots", type=int, default=1 << 18, help="shots per launch of (a)")
    ap.add_argument("--faults", type=int, default=1 << 16, help="faults per launch of (c)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-dem", action="store_true", help="(c) without the DEM composition on the host")
    ap.add_argument("--parts", default="abc", help="which of (a), (b), (c) to run")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "frame_hbm", "bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_circuit_frame.py needs a GPU")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    res = {"device": torch.cuda.get_device_name(0), "compute_units": cus, "reps": a.reps, "warmup": a.warmup,
           "timing": "HIP events around the launch, ms per launch, packed rows", "readme_config4_decode": README_C4_DECODE}

    # ---- (a) a circuit that fits LDS, under both placements
    if "a" in a.parts:
        small = build_storage_simulation(3, circuit_noise(0.003), load_code("hgp_12_3_4_s1234")).compiled()
        part = {"code": "hgp_12_3_4_s1234", "rounds": 3, "p": 0.003, "shots": a.small_shots,
                "slot_bytes": small.lds_bytes}
        for frame in ("lds", "hbm"):
            part[frame] = _sampler(small, a.small_shots, frame, a.reps, a.warmup)
        part["hbm_over_lds_time"] = part["hbm"]["ms"]["median"] / part["lds"]["ms"]["median"]
        part["hbm_slots"] = small.frame_info(0, "hbm")["slots"]
        res["n225"] = part
        print(json.dumps({"n225": part}), flush=True)
        small.close()

    # ---- (b) the n = 10^4 code over slots per CU
    hx, hz = load_checks("hgp_80_3_4_s2025")
    code = QuantumCode(QuantumCodeChecks(hx, hz), QuantumCodeLogicals(*load_logicals("hgp_80_3_4_s2025")))
    rows = []
    for R in (1, 3) if "b" in a.parts else ():
        for p in (0.001, 0.01):
            t0 = time.perf_counter()
            cc = build_storage_simulation(R, circuit_noise(p), code).compiled()
            host_s = time.perf_counter() - t0
            row = {"rounds": R, "p": p, "shots": a.shots, "slot_bytes": cc.lds_bytes, "qubits": cc.num_qubits,
                   "measurements": cc.num_measurements, "instructions": int(cc.ops.shape[0]),
                   "text_and_compile_s": host_s, "by_slots_per_cu": {}}
            for W in (1, 2, 4, 8):
                cc.set_frame_slots(cus * W)
                r = _sampler(cc, a.shots, "auto", a.reps, a.warmup)
                fi = cc.frame_info(0)
                r["slots"] = fi["slots"]
                r["working_set_bytes"] = fi["slots"] * fi["slot_bytes"]
                r["working_set_over_infinity_cache"] = r["working_set_bytes"] / INFINITY_CACHE
                row["by_slots_per_cu"][str(W)] = r
            best = max(row["by_slots_per_cu"], key=lambda w: row["by_slots_per_cu"][w]["shots_per_s"])
            row["fastest_slots_per_cu"] = int(best)
            row["shots_per_s"] = row["by_slots_per_cu"][best]["shots_per_s"]
            cc.set_frame_slots(0)
            row["default_slots"] = _sampler(cc, a.shots, "auto", a.reps, a.warmup)
            rows.append(row)
            print(json.dumps({"n10k": row}), flush=True)
            cc.close()
    if rows:
        res["n10k"] = rows

    # ---- (c) fault propagation of the R = 1 circuit, and its DEM
    if "c" in a.parts:
        keep = build_storage_simulation(1, circuit_noise(0.001), code).compiled()
        noise, gauge = handle_fault_info(keep.handle(0))
        F = min(a.faults, noise)
        ms = _timed(lambda: keep.fault_symptoms_device(kind=0, f0=0, F=F, packed=True), a.reps, a.warmup)
        part = {"rounds": 1, "p": 0.001, "noise_faults": noise, "gauge_faults": gauge, "window": F, "ms": _stat(ms),
                "faults_per_s": F / (statistics.median(ms) * 1e-3), "slots": keep.frame_info(0)["slots"]}
        print(json.dumps({"n10k_faults": part}), flush=True)
        if not a.skip_dem:
            # every detector of the circuit, no observables; wall clock, once: the fault kernel's windows and
            # their copies to the host, then the numpy composition (dem.dem_from_symptoms)
            import resource
            from exp_ldpc_amd.dem import detector_error_model
            t0 = time.perf_counter()
            dem = detector_error_model(keep, detectors=keep.detectors, observables=keep.groups["readout"][:0])
            part["dem_wall_s"] = time.perf_counter() - t0
            part["dem_detectors"] = int(keep.detectors.shape[0])
            part["dem_errors"] = dem.num_errors
            part["host_max_rss_gb"] = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1e6
        res["n10k_faults"] = part
        keep.close()

    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
