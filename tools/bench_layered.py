"""Layered min-sum BP (layered_wave_kernel, csrc/qdec_layered.hip) on one MI355X
against the flooding decode of the same tree on identical shots, in the same
process.  Diagnostic companion of bench.py; numbers are recorded, nothing is
asserted except that the two placements return the same bytes.

Device times are HIP events around the BP stage's launch alone, warm, median
and [min, max] of --reps runs (5 by default).  Min-sum f64, alpha = 1.

(a) code     the n = 225 code, code capacity, p = 0.01 / 0.02 / 0.03, 50
             iterations: flooding (the plan's kernel) against layered in LDS,
             each followed by OSD-CS 7 on chip; at p = 0.02 the LDS launch and
             the HBM launch at 4 / 8 / 16 workgroups per CU.
(b) dem225   the circuit DEM of that code under circuit_noise (R = 2), 30
             iterations: bp_block_kernel against layered in HBM at 4 / 8 / 16 /
             32 workgroups per CU; then bposd_detector end to end both ways.
(c) dem144   the same on the [[144,12,12]] code's circuit DEM, R = 2.

Prints one JSON line and writes it to profiles/layered/bench.json.

Usage: python tools/bench_layered.py [--shots N] [--dem_shots N] [--reps K] [--p P] [--parts abc] [--out FILE]
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

OSD = ("osd_cs", 7)


def _stat(ms):
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms), "n": len(ms)}


def _say(*a):
    print(*a, file=sys.stderr, flush=True)


def _timed(fn, reps, warmup=1):
    """ms of fn() alone by HIP events."""
    import torch
    out = []
    for r in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if r >= warmup:
            out.append(e0.elapsed_time(e1))
    return out


class Bp:
    """One decoder's BP stage on a batch: time, converged shots, mean iterations, flags."""

    def __init__(self, dec, syn, readout, reps):
        import torch
        self.dec, self.syn, self.rd, self.reps = dec, syn, readout, reps
        self.B = B = syn.shape[0]
        dev = syn.device
        self.llr = torch.empty((B, dec.n), dtype=torch.float64, device=dev)
        self.status = torch.zeros(B, dtype=torch.uint8, device=dev)
        self.fail = torch.zeros(B, dtype=torch.uint8, device=dev)
        self.iters = torch.zeros(B, dtype=torch.int32, device=dev)

    def run(self):
        ms = _timed(lambda: self.dec.decode_device(self.B, syn=self.syn, readout=self.rd, llr=self.llr,
                                                   iters=self.iters, status=self.status, fail=self.fail), self.reps)
        res = dict(_stat(ms), converged=int((self.status & 1).sum().item()),
                   mean_iters=float(self.iters.double().mean().item()), failures=int(self.fail.sum().item()))
        res["us_per_shot_iteration"] = 1e3 * res["median"] / max(1.0, res["mean_iters"] * self.B)
        if self.dec.schedule == "layered":
            info = self.dec.layered_info()
            res.update(kind="hbm" if info[0] else "lds", lds_bytes=info[1], slot_bytes=info[2], workgroups=info[3])
        return res

    def osd(self, rows):
        st, fl = self.status.clone(), self.fail.clone()

        def go():
            st.copy_(self.status)
            fl.copy_(self.fail)
            self.dec.osd_device(self.B, llr=self.llr, method=OSD[0], order=OSD[1], syn=self.syn, status=st,
                                readout=self.rd, fail=fl, rows=rows)
        ms = _timed(go, self.reps)
        return dict(_stat(ms), failures=int(fl.sum().item()), shots=int(((self.status & 1) == 0).sum().item()))


def part_code(code, a, cus):
    import torch
    from exp_ldpc_amd.decoder import Decoder
    hz, lz = code.checks.z, code.logicals.z
    out = []
    for p in (0.01, 0.02, 0.03):
        kw = dict(method="ms", precision="f64", max_iter=50, ms_scaling=1.0, logicals=lz)
        flood = Decoder(hz, 2 * p / 3, **kw)
        lay = Decoder(hz, 2 * p / 3, schedule="layered", layered_placement="lds", **kw)
        B = a.shots
        syn = torch.empty((B, flood.m), dtype=torch.uint8, device="cuda")
        rd = torch.empty((B, flood.n), dtype=torch.uint8, device="cuda")
        flood.sample_storage_device(0, p, p, seed=a.seed, stream_id=0, shot0=0, B=B, syn=syn, readout=rd)
        row = {"p": p, "shots": B}
        for name, dec in (("flooding", flood), ("layered_lds", lay)):
            bp = Bp(dec, syn, rd, a.reps)
            row[name] = bp.run()
            row[name]["osd"] = bp.osd("onchip")
            if name == "flooding":
                row[name]["kernel"] = dec.last_kernels()[0]
        if p == 0.02:
            row["layered_lds_per_cu"] = {}
            for per in (4, 8, 16):
                lay.set_layered_slots(cus * per)
                row["layered_lds_per_cu"][per] = Bp(lay, syn, rd, a.reps).run()
            # the same graph from HBM slots: what the placement alone costs
            lay.layered_placement = "hbm"
            row["layered_hbm_per_cu"] = {}
            for per in (4, 8, 16):
                lay.set_layered_slots(cus * per)
                row["layered_hbm_per_cu"][per] = Bp(lay, syn, rd, a.reps).run()
            lay.layered_placement = "lds"
            lay.set_layered_slots(0)
        _say("(a)", json.dumps(row))
        out.append(row)
        flood.close()
        lay.close()
    return out


def part_dem(code, R, a, name, cus):
    import numpy as np
    import torch
    from exp_ldpc_amd.experiment import BatchPipeline, _steps
    from exp_ldpc_amd.noise_model import circuit_noise
    from exp_ldpc_amd.storage_sim import build_storage_simulation
    xs, zs = _steps(code.checks)
    nm = circuit_noise(a.p)
    sim = build_storage_simulation(R, nm, code)
    opts = {"max_iter": 30, "bp_method": "ms", "ms_scaling_factor": 1.0, "osd_method": OSD[0], "osd_order": OSD[1]}
    priors = (2 * a.p / 3 * (xs + zs + 2), a.p * (zs + 2))
    pipes = {"flooding": BatchPipeline(code, R, "bposd_detector", opts, priors, noise=nm, precision="f64", sim=sim),
             "layered": BatchPipeline(code, R, "bposd_detector", dict(opts, bp_schedule="layered"), priors, noise=nm,
                                      precision="f64", sim=sim)}
    B = a.dem_shots
    ref = pipes["flooding"]
    det, rd = ref.sample(sim, B, a.seed, 0, 0)
    v = ref._circuit_readout_faults(rd, 0, B) if ref.L.shape[0] else None
    res = {"graph": name, "rounds": R, "m": ref.det.m, "n": ref.det.n, "E": int(ref.det.H.nnz),
           "max_row": int(np.diff(ref.det.H.indptr).max()), "p": a.p, "shots": B, "num_cus": cus}
    res["flooding"] = Bp(ref.det, det, v, a.reps).run()
    _say(f"{name}: {res['m']} x {res['n']}, flooding", json.dumps(res["flooding"]))
    lay = pipes["layered"].det
    res["layered_hbm_per_cu"] = {}
    llr = {}
    for per in (4, 8, 16, 32):
        lay.set_layered_slots(cus * per)
        lay.layered_placement = "hbm"
        bp = Bp(lay, det, v, a.reps)
        res["layered_hbm_per_cu"][per] = bp.run()
        llr[per] = bp.llr
        _say(f"  layered hbm {per} per CU", json.dumps(res["layered_hbm_per_cu"][per]))
    assert torch.equal(llr[4], llr[32]), "results depend on the slots"
    lay.set_layered_slots(0)
    try:
        lay.layered_placement = "lds"
        bp = Bp(lay, det, v, a.reps)
        res["layered_lds"] = bp.run()
        assert torch.equal(bp.llr, llr[4]), "the two placements disagree"
    except Exception as e:  # noqa: BLE001 - the placement does not hold the graph: recorded
        res["layered_lds"] = {"error": str(e)}
    lay.layered_placement = "auto"
    res["bposd_detector"] = {}
    for key, pipe in pipes.items():
        out = {}

        def go():
            out["res"] = pipe.run(det, rd)
        ms = _timed(go, max(1, a.reps // 2))
        res["bposd_detector"][key] = dict(_stat(ms), failures=int(out["res"].fail.sum()),
                                          bp_converged=int(out["res"].bp_converged))
        _say(f"  bposd_detector {key}", json.dumps(res["bposd_detector"][key]))
    for pipe in pipes.values():
        for d in pipe.decoders() + [pipe.sampler_graph]:
            d.close()
    return res


def main():
    import torch
    from conftest import load_code
    ap = argparse.ArgumentParser()
    ap.add_argument("--shots", type=int, default=1 << 16, help="shots of (a)")
    ap.add_argument("--dem_shots", type=int, default=1 << 12, help="shots of (b) and (c)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--p", type=float, default=0.003, help="circuit_noise strength of (b) and (c)")
    ap.add_argument("--seed", type=int, default=20250221)
    ap.add_argument("--parts", default="abc")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "layered", "bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_layered.py needs a GPU")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    code = load_code("hgp_12_3_4_s1234")
    res = {"reps": a.reps, "bp": "min-sum f64, alpha 1", "osd": f"{OSD[0]} {OSD[1]}", "num_cus": cus,
           "timing": "device ms by HIP events around the stage's launch (warm)"}
    if "a" in a.parts:
        res["code225"] = part_code(code, a, cus)
    if "b" in a.parts:
        res["dem225"] = part_dem(code, 2, a, "hgp_12_3_4_s1234 circuit DEM", cus)
    if "c" in a.parts:
        from exp_ldpc_amd.lifted import bivariate_bicycle_code
        bb = bivariate_bicycle_code(12, 6, [(3, 0), (0, 1), (0, 2)], [(0, 3), (1, 0), (2, 0)], compute_logicals=True)
        res["dem144"] = part_dem(bb, 2, a, "[[144,12,12]] circuit DEM", cus)
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
