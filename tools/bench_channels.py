"""Sampling throughput of the Pauli-frame kernel (frame_sample_kernel) under the
two ways to write the same noise: circuit_noise(p) (DEPOLARIZE1 / DEPOLARIZE2,
equal shares of one threshold) and biased_circuit_noise(p, 1/2) (PAULI_CHANNEL_1 /
PAULI_CHANNEL_2 with equal arguments, cumulative thresholds).  Both circuits have
the same sites and firing rates, so the gap is the cost of the cumulative-threshold
path.  Diagnostic companion of tools/bench_circuit.py.

The n = 225 code, R = 3 (default), the ``syn`` and ``readout`` groups, byte and
packed rows, the frame in LDS and in HBM: the four instantiations of the sample
kernel.  2^18 shots per launch, warm, HIP events, median and [min, max] of
--reps launches.  Prints one JSON line; --out writes it to a file as well.

--noise circuit measures the depolarizing circuits alone (to set a build against
another one).

Usage: python tools/bench_channels.py [--shots N] [--reps K] [--p P ...] [--noise circuit biased] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from bench_circuit import _op_counts, _stat, _timed  # noqa: E402


def main():
    import torch
    from conftest import load_code
    from exp_ldpc_amd import noise_model
    from exp_ldpc_amd.storage_sim import build_storage_simulation
    ap = argparse.ArgumentParser()
    ap.add_argument("--shots", type=int, default=1 << 18)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--p", type=float, nargs="+", default=[0.001, 0.01])
    ap.add_argument("--eta", type=float, default=0.5, help="bias of biased_circuit_noise (1/2: depolarizing)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--noise", nargs="+", choices=["circuit", "biased"], default=["circuit", "biased"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_channels.py needs a GPU")
    code = load_code("hgp_12_3_4_s1234")
    m, n = code.checks.z.shape
    B, R = a.shots, a.rounds
    dev = torch.device("cuda", 0)
    res = {"code": "hgp_12_3_4_s1234", "rounds": R, "shots": B, "reps": a.reps, "warmup": a.warmup, "eta": a.eta,
           "timing": "HIP events around the launch, ms per launch of `shots` shots", "points": []}
    for p in a.p:
        point = {"p": p}
        for kind in a.noise:
            nm = noise_model.circuit_noise(p) if kind == "circuit" else noise_model.biased_circuit_noise(p, a.eta)
            cc = build_storage_simulation(R, nm, code).compiled()
            entry = {"program": _op_counts(cc)}
            for frame in ("lds", "hbm"):
                for path, packed in (("byte", False), ("packed", True)):
                    dt = torch.int64 if packed else torch.uint8
                    w = (lambda c: (c + 63) // 64) if packed else (lambda c: c)
                    out = {"syn": torch.empty((B, w((R + 1) * m)), dtype=dt, device=dev),
                           "readout": torch.empty((B, w(n)), dtype=dt, device=dev)}
                    ms = _timed(lambda: cc.sample_device(B, 20250221, packed=packed, out=out, frame=frame,
                                                         outputs=("syn", "readout")), a.reps, a.warmup)
                    entry[f"{frame}_{path}"] = {"ms": _stat(ms), "shots_per_s": B / (statistics.median(ms) * 1e-3)}
            cc.close()
            point[kind] = entry
        if "circuit" in point and "biased" in point:
            point["biased_over_circuit"] = {k: point["biased"][k]["ms"]["median"] / point["circuit"][k]["ms"]["median"]
                                            for k in point["circuit"] if k != "program"}
        res["points"].append(point)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
