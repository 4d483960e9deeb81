"""Storage experiment: measurement-record views and the on-device sampler.

Mirrors ``build_storage_simulation`` (``python/qldpc/storage_sim.py:110-199``) for
what the decoding path consumes:

* the record layout -- per round ``[X-check outcomes (mx), Z-check outcomes (mz)]``
  then the transversal data readout (n) -- and its views ``measurement_view``
  (:187-192) and ``data_view`` (:194-196);
* the noise, by one of two device samplers.  Under ``depolarizing_noise`` and
  ``trivial_noise`` shots are drawn by the Philox sampler in csrc/qdec_sample.hip,
  which restates the few events the rewrite places on the circuit (schedule
  pinned against the reference's circuit text, tests/test_storage_schedule.py);
  gates are noiseless there and the gate schedule does not change what the
  decoder sees.  Under every other rewriter (``circuit_noise``,
  a custom ``NoiseRewriter``) the circuit itself is sampled: ``StorageSim.circuit``
  is the noisy circuit text (gate layers by edge colouring, schedule.py),
  ``compiled()`` its Pauli-frame program (circuit.py) with the output groups
  ``syn`` (the decoded sector's detectors in spacetime order, round t in columns
  t m .. (t + 1) m - 1) and ``readout`` (the last n records), run by
  csrc/qdec_frame.hip.  ``compiled_detectors()`` is the same program with every
  detector of the circuit (both sectors) for bpd_detector on the circuit's own
  detector error model (dem.detector_error_model).

Circuit and program are built on first use: the depolarizing / trivial device
path never pays for a colouring.  X-check outcomes in host records
(``records_from_samples``) are zero: they are random in the first round and
never read by the Z-basis decoders (get_x_checks=False).
"""
from __future__ import annotations

from typing import Callable

import numpy as np

__all__ = ["StorageSim", "build_storage_simulation", "storage_output_groups"]


def storage_output_groups(compiled, mx: int, mz: int, n: int, rounds: int, use_x_logicals: bool = False) -> dict:
    """The storage experiment's two output groups of a compiled storage circuit
    (this module's text or the reference's): ``syn``, the decoded sector's
    detectors in spacetime order, and ``readout``, the last n records.  The text
    declares the first round's sector detectors, then both sectors (X first) for
    every further round, then the final round's."""
    per, m = mx + mz, (mx if use_x_logicals else mz)
    off = 0 if use_x_logicals else mx
    pick = []
    if rounds > 0:
        pick += list(range(m))
        for t in range(rounds - 1):
            pick += list(range(m + t * per + off, m + t * per + off + m))
    nd = (m + (rounds - 1) * per if rounds > 0 else 0)
    pick += list(range(nd, nd + m))
    if compiled.detectors.shape[0] != nd + m:
        raise ValueError(f"not a storage circuit of {rounds} rounds: {compiled.detectors.shape[0]} detectors, "
                         f"expected {nd + m}")
    M = compiled.num_measurements
    return {"syn": compiled.detectors[pick], "readout": compiled.record_rows(M - n, M)}


class StorageSim:
    """Views, noise model and samplers of one storage experiment (reference
    StorageSim, qecc_util.py; ``circuit`` is built on first use)."""

    def __init__(self, circuit, measurement_view: Callable, data_view: Callable, rounds: int = 0, noise_model=None,
                 code=None, use_x_logicals: bool = False):
        self._circuit = circuit
        self.measurement_view = measurement_view
        self.data_view = data_view
        self.rounds = rounds
        self.noise_model = noise_model
        self.code = code
        self.use_x_logicals = use_x_logicals
        self._targets = None
        self._compiled = None
        self._compiled_detectors = None

    @property
    def circuit(self):
        """The noisy circuit text (a list of lines), generated on first use."""
        if self._circuit is None and self.code is not None and self.noise_model is not None:
            from .schedule import storage_circuit_text
            self._targets, self._circuit = storage_circuit_text(self.rounds, self.noise_model, self.code,
                                                                self.use_x_logicals)
        return self._circuit

    def compiled(self):
        """The circuit's Pauli-frame program with the groups ``syn`` and ``readout``."""
        if self._compiled is None:
            from .circuit import compile_circuit
            cc = compile_circuit(self.circuit)
            mx, mz = self.code.checks.x.shape[0], self.code.checks.z.shape[0]
            self._compiled = cc.with_groups(storage_output_groups(cc, mx, mz, self.code.num_qubits, self.rounds,
                                                                  self.use_x_logicals))
        return self._compiled

    def compiled_detectors(self):
        """The same program with the groups ``detectors`` (every DETECTOR of the
        circuit, both sectors, in the circuit's order) and ``readout``: what the
        circuit's own detector error model is decoded from."""
        if self._compiled_detectors is None:
            cc = self.compiled()
            self._compiled_detectors = cc.with_groups({"detectors": cc.detectors, "readout": cc.groups["readout"]})
        return self._compiled_detectors

    # ---- sampler (device) ----
    def check_matrix(self):
        return self.code.checks.x if self.use_x_logicals else self.code.checks.z

    def sample_device(self, decoder, B: int, seed: int, stream_id: int = 0, shot0: int = 0, out=None):
        """Sample B shots on `decoder`'s device (decoder must be built on the
        decoding check matrix).  Returns (spacetime syndrome uint8[B, (R+1)m],
        readout uint8[B, n]) as torch tensors."""
        import torch
        nm = self.noise_model
        if nm is None:
            raise NotImplementedError("the device sampler needs a noise model")
        if getattr(nm, "kind", None) not in ("depolarizing", "trivial"):
            # any other rewriter: sample the circuit itself (csrc/qdec_frame.hip)
            res = self.compiled().sample_device(B, seed, stream_id, shot0, outputs=("syn", "readout"),
                                                device=decoder.device,
                                                out=None if out is None else {"syn": out[0], "readout": out[1]})
            return res["syn"], res["readout"]
        H = self.check_matrix()
        m, n = H.shape
        dev = torch.device("cuda", decoder.device)
        if out is None:
            syn = torch.empty((B, (self.rounds + 1) * m), dtype=torch.uint8, device=dev)
            rd = torch.empty((B, n), dtype=torch.uint8, device=dev)
        else:
            syn, rd = out
        decoder.sample_storage_device(self.rounds, nm.p, nm.pm, seed, stream_id, shot0, B, syn, rd)
        return syn, rd

    def sample_detectors_device(self, B: int, seed: int, stream_id: int = 0, shot0: int = 0, device: int = 0):
        """Sample B shots of the circuit itself under any noise model
        (csrc/qdec_frame.hip).  Returns (detectors uint8[B, D], readout
        uint8[B, n]): every detector of the circuit, in the circuit's order."""
        res = self.compiled_detectors().sample_device(B, seed, stream_id, shot0, outputs=("detectors", "readout"),
                                                      device=device)
        return res["detectors"], res["readout"]

    def records_from_samples(self, syn: np.ndarray, readout: np.ndarray) -> np.ndarray:
        """Host measurement records (reference layout) from sampler output:
        undo the round differencing; X-check outcomes are 0."""
        checks = self.code.checks
        mx, mz = checks.x.shape[0], checks.z.shape[0]
        R = self.rounds
        B = syn.shape[0]
        m = mx if self.use_x_logicals else mz
        diff = syn.reshape(B, R + 1, m)
        raw = np.bitwise_xor.accumulate(diff[:, :R], axis=1) if R else np.zeros((B, 0, m), np.uint8)
        rec = np.zeros((B, (mx + mz) * R + readout.shape[1]), dtype=np.uint8)
        for t in range(R):
            off = (mx + mz) * t + (0 if self.use_x_logicals else mx)
            rec[:, off:off + m] = raw[:, t]
        rec[:, (mx + mz) * R:] = readout
        return rec


def build_storage_simulation(rounds: int, noise_model, code, use_x_logicals=None) -> StorageSim:
    """Record views of the storage experiment with `rounds` noisy rounds
    (storage_sim.py:110-199; the circuit text is generated on first use)."""
    if use_x_logicals is None:
        use_x_logicals = False
    mx, mz = code.checks.x.shape[0], code.checks.z.shape[0]
    n = code.num_qubits

    def meas_result(round_index, get_x_checks, measurement_vector, *_, mx=mx, mz=mz):
        off = (mx + mz) * round_index + (0 if get_x_checks else mx)
        cnt = mx if get_x_checks else mz
        return measurement_vector[off:off + cnt]

    def data_result(measurement_vector, *_, mx=mx, mz=mz, rounds=rounds, n=n):
        off = (mx + mz) * rounds
        return measurement_vector[off:off + n]

    return StorageSim(None, meas_result, data_result, rounds=int(rounds), noise_model=noise_model, code=code,
                      use_x_logicals=bool(use_x_logicals))
