"""The relay-BP stage (relay_block_kernel, csrc/qdec_relay.hip) on one MI355X
against the post-processors the project already has, on identical shots.
Diagnostic companion of bench.py; numbers are recorded, nothing is asserted
except that the two placements return the same bytes.

Device times are HIP events around the stage's launch alone, warm, median and
[min, max] of --reps runs (5 by default).  Min-sum f64 throughout; the relay
stage runs Decoder.set_relay's defaults unless --relay_* say otherwise.

(a) code     the n = 225 code, code capacity, p = 0.01 / 0.02 / 0.03: BP(50) +
             relay against BP + SSF and BP + OSD-CS 7 (on chip).
(b) dem225   bposd_detector's circuit DEM of that code under circuit_noise
             (R = 2): the relay stage against the OSD stage with its rows in
             HBM on the same BP-failed shots; both placements where they hold
             the graph; 1 / 2 / 4 / 8 workgroups per CU.
(c) dem144   the same on the [[144,12,12]] code's circuit DEM
             (dem.detector_error_model), R = 2.

Prints one JSON line and writes it to profiles/relay/bench.json.

Usage: python tools/bench_relay.py [--shots N] [--dem_shots N] [--reps K] [--p P] [--parts abc] [--out FILE]
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


def _timed(setup, fn, reps, warmup=1):
    """ms of fn() alone by HIP events; setup() runs before each, outside the events."""
    import torch
    out = []
    for r in range(warmup + reps):
        setup()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if r >= warmup:
            out.append(e0.elapsed_time(e1))
    return out


class Stages:
    """BP once on a batch, then each post-processor on the shots it left, from the
    same BP status, llr and flags."""

    def __init__(self, dec, syn, readout, reps):
        import torch
        self.dec, self.syn, self.rd, self.reps = dec, syn, readout, reps
        self.B = B = syn.shape[0]
        dev = syn.device
        self.llr = torch.empty((B, dec.n), dtype=torch.float64, device=dev)
        self.status0 = torch.zeros(B, dtype=torch.uint8, device=dev)
        self.fail0 = torch.zeros(B, dtype=torch.uint8, device=dev)
        self.status, self.fail = self.status0.clone(), self.fail0.clone()
        self.iters = torch.zeros(B, dtype=torch.int32, device=dev)
        self.legs = torch.zeros(B, dtype=torch.int32, device=dev)
        self.bp_ms = _timed(lambda: None, lambda: dec.decode_device(B, syn=syn, readout=readout, llr=self.llr,
                                                                    status=self.status0, fail=self.fail0, ssf=False),
                            reps)
        self.unconverged = int(((self.status0 & 1) == 0).sum().item())

    def _reset(self):
        self.status.copy_(self.status0)
        self.fail.copy_(self.fail0)

    def _result(self, ms):
        left = int(((self.status & 1) == 0).sum().item())
        return dict(_stat(ms), failures=int(self.fail.sum().item()), unsolved=left,
                    us_per_bp_failed_shot=1e3 * statistics.median(ms) / max(self.unconverged, 1))

    def relay(self, placement):
        d = self.dec
        ms = _timed(self._reset, lambda: d.relay_device(self.B, syn=self.syn, readout=self.rd, status=self.status,
                                                        fail=self.fail, iters=self.iters, legs=self.legs,
                                                        only_failed=True, placement=placement), self.reps)
        res = self._result(ms)
        run = (self.status0 & 1) == 0
        if self.unconverged:
            res["mean_iters"] = float(self.iters[run].double().mean().item())
            res["mean_legs"] = float(self.legs[run].double().mean().item())
        info = d.relay_info(placement)
        res.update(kind="hbm" if info[0] else "lds", lds_bytes=info[1], slot_bytes=info[2], workgroups=info[3])
        return res

    def osd(self, rows):
        d = self.dec
        ms = _timed(self._reset, lambda: d.osd_device(self.B, llr=self.llr, method=OSD[0], order=OSD[1], syn=self.syn,
                                                      status=self.status, readout=self.rd, fail=self.fail, rows=rows),
                    self.reps)
        res = self._result(ms)
        res["unsolved"] = 0  # OSD always meets the syndrome
        return res


def part_code(code, a, relay_kw):
    import torch
    from exp_ldpc_amd.decoder import Decoder
    hz, hx, lz = code.checks.z, code.checks.x, code.logicals.z
    out = []
    for p in (0.01, 0.02, 0.03):
        dec = Decoder(hz, 2 * p / 3, method="ms", precision="f64", max_iter=50, ms_scaling=1.0, flip_sets=hx, logicals=lz)
        dec.set_relay(**relay_kw)
        B = a.shots
        syn = torch.empty((B, dec.m), dtype=torch.uint8, device="cuda")
        rd = torch.empty((B, dec.n), dtype=torch.uint8, device="cuda")
        dec.sample_storage_device(0, p, p, seed=a.seed, stream_id=0, shot0=0, B=B, syn=syn, readout=rd)
        st = Stages(dec, syn, rd, a.reps)
        ssf_fail = torch.zeros(B, dtype=torch.uint8, device="cuda")
        ssf_ms = _timed(lambda: None, lambda: dec.decode_device(B, syn=syn, readout=rd, fail=ssf_fail, ssf=True), a.reps)
        row = {"p": p, "shots": B, "bp_ms": _stat(st.bp_ms), "bp_unconverged": st.unconverged,
               "bp_failures": int(st.fail0.sum().item()),
               "bp_ssf": dict(_stat(ssf_ms), failures=int(ssf_fail.sum().item()), note="BP and SSF in one decode call"),
               "osd": st.osd("onchip"), "relay": st.relay("auto")}
        _say("(a)", json.dumps(row))
        out.append(row)
        dec.close()
    return out


def part_dem(code, R, a, relay_kw, name):
    import numpy as np
    import torch
    from exp_ldpc_amd.experiment import BatchPipeline, _steps
    from exp_ldpc_amd.noise_model import circuit_noise
    from exp_ldpc_amd.storage_sim import build_storage_simulation
    xs, zs = _steps(code.checks)
    nm = circuit_noise(a.p)
    sim = build_storage_simulation(R, nm, code)
    opts = {"max_iter": 30, "bp_method": "ms", "ms_scaling_factor": 1.0}
    pipe = BatchPipeline(code, R, "bprelay_detector", opts, (2 * a.p / 3 * (xs + zs + 2), a.p * (zs + 2)), noise=nm,
                         precision="f64", sim=sim, relay=relay_kw)
    dec = pipe.det
    B = a.dem_shots
    det, rd = pipe.sample(sim, B, a.seed, 0, 0)
    v = pipe._circuit_readout_faults(rd, 0, B) if pipe.L.shape[0] else None
    st = Stages(dec, det, v, a.reps)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    res = {"graph": name, "rounds": R, "m": dec.m, "n": dec.n, "p": a.p, "shots": B, "bp_ms": _stat(st.bp_ms),
           "bp_unconverged": st.unconverged, "bp_failures": int(st.fail0.sum().item()), "num_cus": cus}
    _say(f"{name}: {dec.m} x {dec.n}, {st.unconverged} of {B} shots BP-failed")
    res["osd_hbm"] = st.osd("hbm")
    _say("  osd hbm", json.dumps(res["osd_hbm"]))
    res["relay"] = {}
    flags = {}
    for placement in ("lds", "hbm"):
        try:
            res["relay"][placement] = st.relay(placement)
            flags[placement] = st.fail.cpu().numpy().copy()
        except Exception as e:  # noqa: BLE001 - the placement does not hold the graph: recorded
            res["relay"][placement] = {"error": str(e)}
        _say(f"  relay {placement}", json.dumps(res["relay"][placement]))
    if len(flags) == 2:
        assert np.array_equal(flags["lds"], flags["hbm"]), "the two placements disagree"
    res["relay_slots_per_cu"] = {}
    for per in (1, 2, 4, 8):
        dec.set_relay_slots(cus * per)
        res["relay_slots_per_cu"][per] = {k: st.relay(k) for k in flags}
        _say(f"  {per} per CU", json.dumps(res["relay_slots_per_cu"][per]))
    dec.set_relay_slots(0)
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
    ap.add_argument("--relay_pre_iter", type=int, default=80)
    ap.add_argument("--relay_num_sets", type=int, default=60)
    ap.add_argument("--relay_set_max_iter", type=int, default=60)
    ap.add_argument("--relay_stop_nconv", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "relay", "bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_relay.py needs a GPU")
    relay_kw = dict(gamma0=0.125, pre_iter=a.relay_pre_iter, num_sets=a.relay_num_sets,
                    set_max_iter=a.relay_set_max_iter, gamma_dist_interval=(-0.24, 0.66),
                    stop_nconv=a.relay_stop_nconv, alpha=1.0, seed=0)
    code = load_code("hgp_12_3_4_s1234")
    res = {"relay": {k: v for k, v in relay_kw.items()}, "reps": a.reps, "bp": "min-sum f64, alpha 1",
           "osd": f"{OSD[0]} {OSD[1]}", "timing": "device ms by HIP events around the stage's launch (warm)"}
    if "a" in a.parts:
        res["code225"] = part_code(code, a, relay_kw)
    if "b" in a.parts:
        res["dem225"] = part_dem(code, 2, a, relay_kw, "hgp_12_3_4_s1234 circuit DEM")
    if "c" in a.parts:
        from exp_ldpc_amd.lifted import bivariate_bicycle_code
        bb = bivariate_bicycle_code(12, 6, [(3, 0), (0, 1), (0, 2)], [(0, 3), (1, 0), (2, 0)], compute_logicals=True)
        res["dem144"] = part_dem(bb, 2, a, relay_kw, "[[144,12,12]] circuit DEM")
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
