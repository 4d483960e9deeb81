"""Sliding-window decoding (exp_ldpc_amd/window.py, csrc/qdec_window.hip) against
the full spacetime graph on one MI355X, on identical shots.  Diagnostic
companion of bench.py; numbers are recorded, nothing is asserted.

The n = 225 code under depolarizing_noise(p, p), modes bp and bposd (min-sum
f64, 30 iterations; osd_cs of order 7 with osd_rows="auto", so the OSD stage
stays on the device for every graph), R in {4, 12, 24}: the full graph
(window=None, the yardstick) against (W, C) in {(3, 1), (4, 2), (6, 3)}.  Per
setting: shots/s of BatchPipeline.run on shots sampled once (wall clock around
the call with a device synchronise, warm, median of --reps), the logical error
rate on those shots, the kernels the launch plan gives every graph involved
(Decoder.planned_kernels), the OSD kernel of every graph, and the advance
kernel's own time (HIP events around one boundary's launch on the batch).

Prints one JSON line and writes it to profiles/window/bench.json (rewritten
after every setting, so a run that is cut short leaves what it measured).

Usage: python tools/bench_window.py [--shots N] [--osd_shots N] [--reps K] [--p P] [--rounds 4,12,24] [--out FILE]
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

SETTINGS = (None, (3, 1), (4, 2), (6, 3))
OPTS = {"max_iter": 30, "bp_method": "ms", "ms_scaling_factor": 0, "osd_method": "osd_cs", "osd_order": 7}


def _say(*a):
    print(*a, file=sys.stderr, flush=True)


def _stat(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}


BP_PATHS = ("bp_wave_kernel", "bp_ms_wave_kernel", "ms_triage_kernel + bp_ms_cmp_kernel", "bp_group_kernel",
            "bp_ms_lds_kernel / bp_ms_lds64_kernel", "bp_block_kernel")
PLACEMENTS = {3: "messages and shot state in LDS", 2: "messages in HBM", 0: "messages and shot state in HBM"}


def _plan(d, B, present):
    """The launch plan's BP path (qd_graph_plan) by family name, and where a
    workgroup kernel keeps its state; planned_kernels gives "" for the families
    whose instantiations the launchers do not note."""
    import ctypes as C
    from exp_ldpc_amd import _abi
    bits = {"syn": 1, "base": 2, "readout": 4, "x": 8, "corr": 16, "llr": 32, "fail": 64}
    out = (C.c_int32 * 8)()
    prm = d._params(0, False)
    _abi.check(_abi.load().qd_graph_plan(d._handle, C.byref(prm), int(B), sum(bits[k] for k in present) | 128, out),
               "qd_graph_plan")
    row = {"bp": BP_PATHS[out[0]]}
    if out[0] >= 3:
        row["state"] = PLACEMENTS.get(out[6], str(out[6]))
    return row


def _graphs(pipe, B, mode):
    """Per distinct graph of the pipeline: its shape, the windows it serves, the
    planned BP kernels of the call the pipeline makes, and the OSD kernel."""
    out = []
    wd = pipe.wd
    decs = pipe.decoders()
    for d in decs:
        serves = sum(x is d for x in wd.decoders) if wd is not None else 1
        final = d is pipe.st
        present = ("syn", "readout", "corr", "fail") if final else ("syn", "x")
        if final and wd is not None:
            present += ("base",)
        if mode == "bposd":
            present += ("llr",)
        row = {"m": d.m, "n": d.n, "windows": serves, "final": final, "plan": _plan(d, B, present),
               "planned_kernels": list(d.planned_kernels(B, present=present, ssf=False))}
        if mode == "bposd":
            info = d.osd_kernel_info("auto")
            row["osd_kernel"] = None if info is None else dict(zip(("kind", "RS", "W", "bytes"), info))
        out.append(row)
    return out


def _advance_ms(pipe, B, reps):
    """ms of one non-final boundary's launch on B shots, and of the staging copy."""
    import torch
    wd = pipe.wd
    if wd is None or len(wd.plan.windows) < 2:
        return None
    w, wa = wd.plan.windows[0], wd.bounds[0]
    dev = torch.device("cuda", pipe.device)
    x = torch.randint(0, 2, (B, w.n), dtype=torch.uint8, device=dev)
    syn = torch.zeros((B, wd.plan.m), dtype=torch.uint8, device=dev)
    acc = torch.zeros((B, wd.plan.k_acc), dtype=torch.uint8, device=dev)
    nxt = torch.empty((B, w.next_m), dtype=torch.uint8, device=dev)
    first = torch.empty((B, w.m), dtype=torch.uint8, device=dev)

    def timed(fn):
        ms = []
        for r in range(reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r:
                ms.append(e0.elapsed_time(e1))
        return _stat(ms)
    return {"boundary_ms": timed(lambda: wa.advance(B, x, syn, acc, nxt)),
            "stage_ms": timed(lambda: wd.stage.advance(B, None, syn, None, first)),
            "boundaries_per_batch": len(wd.plan.windows) - 1,
            "bytes_per_shot": w.n + 2 * len(w.carry_rows) + w.next_m * 2 + wd.plan.k_acc}


def measure(code, R, mode, setting, syn, rd, p, reps):
    import torch
    from exp_ldpc_amd.experiment import BatchPipeline
    B = syn.shape[0]
    kw = {} if setting is None else {"window": setting[0], "commit": setting[1]}
    pipe = BatchPipeline(code, R, mode, OPTS, (2 * p / 3, p), precision="f64", osd_rows="auto", **kw)
    row = {"rounds": R, "mode": mode, "window": None if setting is None else setting[0],
           "commit": None if setting is None else setting[1], "shots": B}
    try:
        row["graphs"] = _graphs(pipe, B, mode)
        secs = []
        for r in range(reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = pipe.run(syn, rd)
            torch.cuda.synchronize()
            if r:
                secs.append(time.perf_counter() - t0)
        row.update(seconds=_stat(secs), shots_per_s=B / statistics.median(secs), failures=int(res.fail.sum()),
                   ler=float(res.fail.mean()), bp_converged_frac=res.bp_converged / B, iters_mean=res.iters_sum / B,
                   advance=_advance_ms(pipe, B, reps))
    except Exception as e:  # noqa: BLE001 - a setting the library refuses is recorded, the rest goes on
        from exp_ldpc_amd.experiment import device_error
        if device_error(e):  # the device itself failed: nothing more is started on it
            raise
        row["error"] = f"{type(e).__name__}: {e}"
    for d in pipe.decoders() + [pipe.sampler_graph]:
        d.close()
    if pipe.wd is not None:
        pipe.wd.close()
    return row


def main():
    import torch
    from conftest import load_code
    from exp_ldpc_amd.decoder import Decoder
    ap = argparse.ArgumentParser()
    ap.add_argument("--shots", type=int, default=1 << 15, help="shots of the bp settings")
    ap.add_argument("--osd_shots", type=int, default=1 << 12, help="shots of the bposd settings")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--p", type=float, default=0.004)
    ap.add_argument("--seed", type=int, default=20250221)
    ap.add_argument("--rounds", default="4,12,24")
    ap.add_argument("--modes", default="bp,bposd")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "window", "bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_window.py needs a GPU")
    code = load_code("hgp_12_3_4_s1234")
    hz = code.checks.z
    sampler = Decoder(hz, 0.01)
    res = {"code": "hgp_12_3_4_s1234", "noise": f"depolarizing_noise({a.p}, {a.p})", "bp": "min-sum f64, 30 iterations",
           "osd": 'osd_cs 7, osd_rows="auto"', "reps": a.reps,
           "timing": "BatchPipeline.run wall clock with a device synchronise, warm, median; advance: HIP events",
           "yardstick": "window = null rows: the full spacetime graph on the same shots", "rows": []}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    for mode in a.modes.split(","):
        B = a.shots if mode == "bp" else a.osd_shots
        for R in (int(v) for v in a.rounds.split(",")):
            syn = torch.empty((B, (R + 1) * hz.shape[0]), dtype=torch.uint8, device="cuda")
            rd = torch.empty((B, hz.shape[1]), dtype=torch.uint8, device="cuda")
            sampler.sample_storage_device(R, a.p, a.p, seed=a.seed, stream_id=R, shot0=0, B=B, syn=syn, readout=rd)
            for setting in SETTINGS:
                row = measure(code, R, mode, setting, syn, rd, a.p, a.reps)
                _say(json.dumps({k: v for k, v in row.items() if k != "graphs"}))
                res["rows"].append(row)
                with open(a.out, "w") as f:
                    f.write(json.dumps(res) + "\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
