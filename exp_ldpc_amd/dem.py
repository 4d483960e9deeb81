"""Detector-error-model (DEM) input for the detector decoding mode (host side).

Reference: ``DetectorSpacetimeCode`` (``python/qldpc/spacetime_code.py:122-183``)
turns a Stim ``DetectorErrorModel`` into a fault check matrix (detectors x
faults), a fault map (observables x faults) and fault priors; ``BPDetectorCorrect``
(``python/qldpc/misc/_experiment.py:128-151``) decodes detector samples with BP on
that matrix and corrects the observables.  Stim (1.13.0, absent here) produced
the DEM via ``circuit.detector_error_model()`` (``_experiment.py:174``).

This module supplies the two pieces without Stim:

* ``parse_dem`` reads the DEM text format (Stim's wire format:
  ``error(p) D.. L.. [^ ...]``, ``detector(...) D..``, ``logical_observable L..``,
  ``shift_detectors[(...)] k``, ``repeat N { ... }``, ``detector_separator``),
  flattening repeat blocks and detector shifts as ``DetectorErrorModel.flattened()``
  does.  Decomposition separators ``^`` are dropped: the reference keeps the
  union of an error's targets (``spacetime_code.py:157-158``).
* ``storage_experiment_dem`` writes the DEM of the storage experiment's Z
  sector for any R under ``depolarizing_noise(p, pm)`` from the circuit's
  noise semantics: X components of data DEPOLARIZE1 (2p/3 per
  event, the rate the reference's priors use, ``scripts/p_sweep.py:4-5``) and
  measurement / readout flips (pm).  Detectors are those of
  ``storage_sim.py:146-182`` (first-round Z detectors, then final-round Z
  detectors); observables are the Z logicals.  Faults with identical symptoms
  are kept as separate columns (Stim would merge them); the decoding problem is
  the spacetime code of ``spacetime_code.py:46-75``.  Agreement of this
  generator with Stim's output is **unpinned** (Stim absent).

* ``detector_error_model`` extracts the DEM of a circuit of the storage gate
  set (circuit.py) under any noise: the library propagates every elementary
  fault of the circuit through the Pauli-frame rules on the GPU
  (``qd_circuit_faults_device``, csrc/qdec_frame.hip) and ``dem_from_symptoms``
  composes the symptoms into independent mechanisms (``fault_mechanisms``) and
  merges equal ones.  It covers both sectors and the faults gates spread, which
  ``storage_experiment_dem`` does not.  Agreement with Stim's own
  ``circuit.detector_error_model()`` stays **unpinned** (Stim absent): the
  column order (here: first appearance in program order), Stim's ``^``
  decompositions (none are made here) and its approximations for probabilities
  above 1/2 are not reproduced; the symptom sets and the merged probabilities
  follow Stim's documented convention of independent X, Y, Z (and 15 two-qubit)
  components per depolarizing channel.

``sample_dem`` draws detector samples by sampling every fault independently
from its prior -- for independent fault mechanisms the distribution Stim's
detector sampler produces.  ``sample_dem_device`` does the same on the GPU
(``qd_sample_faults_device``, counter-based Philox), for the batched pipeline
``experiment.DemPipeline``.
"""
from __future__ import annotations

import re
from dataclasses import dataclass, field
from typing import List, Tuple

import numpy as np
import scipy.sparse as sp

__all__ = ["DemInstruction", "DetectorErrorModel", "parse_dem", "DetectorSpacetimeCode", "storage_experiment_dem",
           "sample_dem", "sample_dem_device", "depolarize1_component", "depolarize2_component",
           "pauli_channel_components", "fault_mechanisms",
           "dem_from_symptoms", "check_deterministic_symptoms", "detector_error_model"]


@dataclass
class DemInstruction:
    type: str                       # 'error' | 'detector' | 'logical_observable'
    args: List[float] = field(default_factory=list)
    detectors: List[int] = field(default_factory=list)   # absolute detector ids
    observables: List[int] = field(default_factory=list)


@dataclass
class DetectorErrorModel:
    """A flattened DEM: instructions with absolute detector ids."""
    instructions: List[DemInstruction]

    def flattened(self) -> "DetectorErrorModel":
        return self

    def __iter__(self):
        return iter(self.instructions)

    @property
    def num_detectors(self) -> int:
        ids = [d for ins in self.instructions for d in ins.detectors]
        return 1 + max(ids) if ids else 0

    @property
    def num_observables(self) -> int:
        ids = [o for ins in self.instructions for o in ins.observables]
        return 1 + max(ids) if ids else 0

    @property
    def num_errors(self) -> int:
        return sum(1 for ins in self.instructions if ins.type == "error")

    def to_text(self) -> str:
        """DEM text that ``parse_dem`` reads back to the same model."""
        lines = []
        for ins in self.instructions:
            tg = " ".join([f"D{d}" for d in ins.detectors] + [f"L{o}" for o in ins.observables])
            head = "error(%r)" % float(ins.args[0]) if ins.type == "error" else ins.type
            lines.append((head + " " + tg).rstrip())
        return "\n".join(lines) + "\n"


_HEAD = re.compile(r"^([a-z_]+)\s*(?:\(([^)]*)\))?\s*(.*)$")


def parse_dem(text: str) -> DetectorErrorModel:
    """Parse DEM text into a flattened model (repeat blocks unrolled,
    ``shift_detectors`` applied)."""
    lines = [l.split("#", 1)[0].strip() for l in text.splitlines()]
    lines = [l for l in lines if l]
    out: List[DemInstruction] = []

    def block_end(i: int) -> int:
        """Index after the '}' closing the block opened on line i."""
        depth, j = 1, i + 1
        while depth:
            if j >= len(lines):
                raise ValueError("unterminated repeat block in DEM")
            depth += lines[j].endswith("{") - (lines[j] == "}")
            j += 1
        return j

    def run(i: int, stop: int, offset: int) -> int:
        while i < stop:
            line = lines[i]
            if line == "}":
                raise ValueError("unbalanced '}' in DEM")
            m = _HEAD.match(line)
            if not m:
                raise ValueError(f"cannot parse DEM line: {line!r}")
            name, args, rest = m.group(1), m.group(2), m.group(3)
            if name == "repeat":
                if not line.endswith("{"):
                    raise ValueError("repeat block must open with '{'")
                count = int(rest.rstrip("{").strip())
                end = block_end(i)
                for _ in range(count):
                    offset = run(i + 1, end - 1, offset)
                i = end
                continue
            argv = [float(v) for v in args.split(",")] if args else []
            toks = rest.split()
            if name == "shift_detectors":
                offset += int(toks[0]) if toks else 0
            elif name in ("error", "detector", "logical_observable"):
                ins = DemInstruction(name, argv)
                for t in toks:
                    if t == "^":
                        continue
                    if t[0] == "D":
                        ins.detectors.append(int(t[1:]) + offset)
                    elif t[0] == "L":
                        ins.observables.append(int(t[1:]))
                    else:
                        raise ValueError(f"bad DEM target {t!r}")
                if name == "error" and len(argv) != 1:
                    raise ValueError("error instruction takes one probability")
                out.append(ins)
            elif name != "detector_separator":
                raise ValueError(f"unknown DEM instruction {name!r}")
            i += 1
        return offset

    run(0, len(lines), 0)
    return DetectorErrorModel(out)


def _from_columns(cols, nrows) -> sp.csr_matrix:
    r = np.fromiter((i for c in cols for i in c), dtype=np.int64)
    c = np.fromiter((j for j, col in enumerate(cols) for _ in col), dtype=np.int64)
    m = sp.coo_matrix((np.ones(r.size, dtype=np.uint32), (r, c)), shape=(nrows, len(cols))).tocsr()
    m.data %= 2  # a target listed twice in one error cancels
    m.eliminate_zeros()
    return m


class DetectorSpacetimeCode:
    """Fault check matrix (detectors x faults), fault map (observables x faults)
    and fault priors of a DEM (reference ``spacetime_code.py:122-183``).  Accepts
    DEM text or a parsed model."""

    def __init__(self, detector_model):
        dem = parse_dem(detector_model) if isinstance(detector_model, str) else detector_model.flattened()
        det_cols, obs_cols, priors = [], [], []
        for ins in dem:
            if ins.type not in ("error", "detector", "logical_observable"):
                raise AssertionError("requires a flattened model")
            if ins.type == "error":
                det_cols.append(ins.detectors)
                obs_cols.append(ins.observables)
                priors.append(ins.args[0])
        self.fault_check_matrix = _from_columns(det_cols, dem.num_detectors)
        self.fault_map = _from_columns(obs_cols, dem.num_observables)
        self.fault_priors = np.array(priors, dtype=np.float64)


def storage_experiment_dem(hz, lz, rounds: int, p: float, pm: float | None = None) -> str:
    """DEM text of the storage experiment's Z sector for any R >= 0 (module
    docstring).  Detector block t (rows t*m ..) is the differenced Z syndrome of
    round t (storage_sim.py:146-179: first-round detectors, then s_t ^ s_{t-1}),
    block R the final readout's Hz parities against the last round; observable i
    is LZ row i (:180-182).

    Fault columns follow the circuit's noise events in time order (the
    schedule the sampler restates: noise_model.py:163-193 on storage_sim.py:110-199,
    including the REPEAT-body DEPOLARIZE1 of rounds t >= 1):
      for t < R: the data error before round t's Z readout (flips block t),
                 round t's Z measurement flips (blocks t and t+1),
                 the data error after the readout (block t+1), and for t >= 1 the
                 one the rewriter places at the end of the REPEAT body (block t+1);
      then the readout flips (block R).  R = 0 has one data event and the readout.
    A data X error in slot t flips every later syndrome and the readout, so it
    fires only detector block t and the observables.

    Deviation from the reference at R >= 2 (unpinned: Stim is absent): the
    reference's bpd_detector decodes Stim's full circuit DEM
    (_experiment.py:174,186), which also holds the X-check detectors of the
    REPEAT body (storage_sim.py:156-157) and keeps X, Y and Z faults as separate
    columns, so Y errors couple the two sectors there.  This DEM is the Z sector
    only, with X and Y merged into one column of prior 2p/3 per event; for
    R <= 1 the two sectors do not interact on the Z detectors the decoder sees.
    At R >= 2 the GPU bpd_detector therefore solves this Z-sector BP problem,
    not Stim's two-sector one."""
    if rounds < 0:
        raise ValueError("rounds must be >= 0")
    pm = p if pm is None else pm
    hz = sp.csc_matrix(hz)
    lz = sp.csc_matrix(np.asarray(lz.todense() if sp.issparse(lz) else lz) % 2)
    m, n = hz.shape
    px = 2 * p / 3
    R = rounds
    col = lambda M, j: M.indices[M.indptr[j]:M.indptr[j + 1]].tolist()
    lines = []

    def err(prob, dets, obs):
        lines.append(("error(%r) " % float(prob) + " ".join([f"D{d}" for d in dets] + [f"L{o}" for o in obs])).rstrip())

    def data_slot(t):
        for j in range(n):
            err(px, [t * m + d for d in col(hz, j)], col(lz, j))

    for t in range(R):
        data_slot(t)                      # before round t's Z readout
        for i in range(m):                # Z-check measurement flip of round t
            err(pm, [t * m + i, (t + 1) * m + i], [])
        data_slot(t + 1)                  # after the readout
        if t >= 1:
            data_slot(t + 1)              # end of the REPEAT body (noise_model.py:183-189)
    if R == 0:
        data_slot(0)                      # single timestep: noise, then the final MZ
    for j in range(n):                    # readout flip of data qubit j
        err(pm, [R * m + d for d in col(hz, j)], col(lz, j))
    lines += [f"detector D{i}" for i in range(m * (R + 1))]
    lines += [f"logical_observable L{o}" for o in range(lz.shape[0])]
    return "\n".join(lines) + "\n"


def sample_dem(code: DetectorSpacetimeCode, shots: int, seed: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """(detectors uint8[B, D], observables uint8[B, K]): every fault drawn
    independently from its prior."""
    rng = np.random.default_rng(seed)
    f = (rng.random((shots, code.fault_priors.size)) < code.fault_priors).astype(np.int64)
    det = (code.fault_check_matrix.astype(np.int64) @ f.T).T % 2
    obs = (code.fault_map.astype(np.int64) @ f.T).T % 2
    return np.asarray(det, dtype=np.uint8), np.asarray(obs, dtype=np.uint8)


def sample_dem_device(decoder, shots: int, seed: int = 0, stream_id: int = 0, shot0: int = 0, packed: bool = False,
                      want_obs: bool = True):
    """The device counterpart of ``sample_dem``: ``decoder`` is a ``Decoder`` on a
    DEM's fault check matrix with the fault priors (and the fault map as
    logicals when observables are wanted).  Returns device tensors
    ``(det, faults, obs)``: detectors ``H e`` and the fault vectors ``e``
    themselves (uint8 rows, or with ``packed`` int64 words in the
    QD_INPUT_PACKED layout) and observables ``F e`` (uint8 [B, K]; None without
    ``want_obs`` or without logicals).  Counter-based (Philox keyed by seed and
    stream_id, counted by fault word and shot0 + row): the shots do not depend
    on how they are split across calls or devices, and differ from
    ``sample_dem``'s numpy stream."""
    import torch
    B = int(shots)
    dev = torch.device("cuda", decoder.device)
    if packed:
        det = torch.empty((B, (decoder.m + 63) // 64), dtype=torch.int64, device=dev)
        faults = torch.empty((B, (decoder.n + 63) // 64), dtype=torch.int64, device=dev)
    else:
        det = torch.empty((B, decoder.m), dtype=torch.uint8, device=dev)
        faults = torch.empty((B, decoder.n), dtype=torch.uint8, device=dev)
    obs = torch.empty((B, decoder.k), dtype=torch.uint8, device=dev) if want_obs and decoder.k else None
    with torch.cuda.device(dev):
        decoder.sample_faults_device(seed, stream_id, shot0, B, det, faults, obs, packed=packed)
    return det, faults, obs


# ---------------------------------------------------------------- circuit -> DEM
def depolarize1_component(p: float) -> float:
    """q1 with: independent X, Y and Z flips of probability q1 each compose to
    DEPOLARIZE1(p) exactly (Stim's convention): q1 = 1/2 - 1/2 (1 - 4p/3)^(1/2)."""
    if not 0.0 <= p <= 0.75:
        raise ValueError(f"DEPOLARIZE1({p!r}) has no independent components: p must lie in [0, 3/4]")
    return 0.5 - 0.5 * (1.0 - 4.0 * p / 3.0) ** 0.5


def depolarize2_component(p: float) -> float:
    """q2 with: independent flips of the 15 two-qubit Paulis, probability q2 each,
    compose to DEPOLARIZE2(p) exactly: q2 = 1/2 - 1/2 (1 - 16p/15)^(1/8)."""
    if not 0.0 <= p <= 0.9375:
        raise ValueError(f"DEPOLARIZE2({p!r}) has no independent components: p must lie in [0, 15/16]")
    return 0.5 - 0.5 * (1.0 - 16.0 * p / 15.0) ** 0.125


def _commutation_signs(n: int) -> np.ndarray:
    """chi[P, Q] = +1 / -1 where the n-qubit Paulis P and Q commute / anticommute;
    a Pauli is its code, two bits per qubit (0 I, 1 X, 2 Y, 3 Z), first qubit high."""
    one = np.ones((4, 4))
    one[1:, 1:] = 2.0 * np.eye(3) - 1.0          # two single-qubit Paulis anticommute iff both differ from I and from each other
    chi = one
    for _ in range(n - 1):
        chi = np.kron(chi, one)
    return chi


_CHI = {3: _commutation_signs(1), 15: _commutation_signs(2)}


def pauli_channel_components(probs, approximate_disjoint_errors: bool = False, name: str = "the channel") -> np.ndarray:
    """q[K] with: independent flips of the K = 3 (X, Y, Z) or 15 (codes 1 .. 15:
    IX .. ZZ) Paulis, probability q_P each, compose to exactly the channel that
    applies Pauli P with probability probs[P - 1] (and nothing otherwise).  With
    lambda_Q = sum_P p_P chi(P, Q) over all 4^n Paulis (p_I = 1 - sum probs):
    q_P = 1/2 - 1/2 exp(-(2 / 4^n) sum_{Q != I} chi(P, Q) ln lambda_Q).  On the
    uniform channels this is depolarize1_component / depolarize2_component.
    The decomposition exists when every lambda_Q > 0 and every q_P >= 0 (a q_P in
    (-1e-15, 0) is rounding and becomes 0); otherwise ValueError naming `name`,
    or with approximate_disjoint_errors (Stim's keyword) the arguments themselves
    as independent probabilities."""
    p = np.asarray(probs, dtype=np.float64).ravel()
    if p.size not in _CHI:
        raise ValueError(f"{name}: a Pauli channel has 3 or 15 probabilities, not {p.size}")
    if not ((p >= 0.0).all() and (p <= 1.0).all() and p.sum() <= 1.0 + 1e-12):
        raise ValueError(f"{name}: probabilities outside [0, 1] or of sum above 1")
    chi = _CHI[p.size]
    full = np.concatenate([[1.0 - p.sum()], p])
    lam = chi[:, 1:].T @ full                    # lambda_Q for Q != I
    q = None
    if (lam > 0.0).all():
        q = 0.5 - 0.5 * np.exp(-(2.0 / (p.size + 1)) * (chi[1:, 1:] @ np.log(lam)))
        q = np.where((q < 0.0) & (q > -1e-15), 0.0, q)
        if (q < 0.0).any():
            q = None
    if q is None:
        if approximate_disjoint_errors:
            return p.copy()
        raise ValueError(f"{name} has no decomposition into independent Pauli flips; "
                         f"approximate_disjoint_errors=True takes its arguments as independent probabilities")
    return q


# members of the mechanisms of one DEPOLARIZE1 target (faults X = 0, Z = 1) and of
# one DEPOLARIZE2 pair (X_a, Z_a, X_b, Z_b = 0 .. 3), -1 padded; Pauli 1 X, 2 Y, 3 Z
_PAULI = {0: [], 1: [0], 2: [0, 1], 3: [1]}
_DEP1 = np.array([(_PAULI[P] + [-1] * 4)[:4] for P in (1, 2, 3)], np.int64)
_DEP2 = np.array([(_PAULI[c >> 2] + [2 + k for k in _PAULI[c & 3]] + [-1] * 4)[:4] for c in range(1, 16)], np.int64)


def fault_mechanisms(cc, approximate_disjoint_errors: bool = False) -> Tuple[np.ndarray, np.ndarray]:
    """The independent error mechanisms of a CompiledCircuit, in program order:
    (probabilities float64 [K], members int64 [K, 4]: the elementary noise faults
    (include/qdec.h numbering) a mechanism fires together, -1 padded).
    X/Y/Z_ERROR(p) and M(p): one mechanism of probability p per target;
    DEPOLARIZE1(p): X, Y = {X, Z}, Z per target, q1 each; DEPOLARIZE2(p): the 15
    non-identity pairs (first qubit's Pauli = code >> 2, second's = code & 3 for
    code 1 .. 15), q2 each.  PAULI_CHANNEL_1 / 2: the members of DEPOLARIZE1 / 2
    with pauli_channel_components of the instruction's arguments; a component of
    probability 0 is no mechanism.  Instructions with p = 0 contribute nothing."""
    from .circuit import OP_DEP1, OP_DEP2, OP_M, OP_MX, OP_PC1, OP_PC2, OP_XERR
    probs, members, f = [], [], 0
    for i, ((op, _, cnt, a0), p) in enumerate(zip(np.asarray(cc.ops).reshape(-1, 4).tolist(),
                                                   np.asarray(cc.probs).tolist())):
        if op in (OP_PC1, OP_PC2):
            nf, unit, pat = (2 * cnt, 2, _DEP1) if op == OP_PC1 else (2 * cnt, 4, _DEP2)
            q = 0.0
            if p > 0:
                a = np.asarray(cc.args, np.float64)[a0:a0 + pat.shape[0]]
                name = f"PAULI_CHANNEL_{1 if op == OP_PC1 else 2}({', '.join(repr(float(v)) for v in a)}) (instruction {i})"
                q = pauli_channel_components(a, approximate_disjoint_errors, name)
                pat = pat[q > 0]
                q = q[q > 0]
        elif op == OP_DEP1:
            nf, unit, pat = 2 * cnt, 2, _DEP1
            q = depolarize1_component(p) if p > 0 else 0.0
        elif op == OP_DEP2:
            nf, unit, pat = 2 * cnt, 4, _DEP2
            q = depolarize2_component(p) if p > 0 else 0.0
        elif op >= OP_XERR or op in (OP_M, OP_MX):
            nf, unit, pat, q = cnt, 1, np.array([[0, -1, -1, -1]], np.int64), p
        else:
            continue
        if p > 0 and nf:
            base = f + unit * np.arange(nf // unit, dtype=np.int64)
            mem = np.where(pat[None] >= 0, base[:, None, None] + pat[None], -1).reshape(-1, 4)
            members.append(mem)
            probs.append(np.broadcast_to(q, (nf // unit, pat.shape[0])).reshape(-1).astype(np.float64))
        f += nf
    if not members:
        return np.zeros(0, np.float64), np.zeros((0, 4), np.int64)
    return np.concatenate(probs), np.concatenate(members)


def _as_words(sym) -> np.ndarray:
    """Symptom rows as uint64 words: 0/1 rows (uint8 / bool) are packed, int64 /
    uint64 rows are taken as QD_INPUT_PACKED words."""
    from .decoder import pack_rows
    a = np.asarray(sym.cpu().numpy() if hasattr(sym, "cpu") else sym)
    if a.dtype in (np.int64, np.uint64):
        return np.ascontiguousarray(a).view(np.uint64).reshape(a.shape[0], -1)
    if a.shape[1] == 0:
        return np.zeros((a.shape[0], 0), np.uint64)
    return pack_rows(a)


def _bits_of(words: np.ndarray, nbits: int) -> np.ndarray:
    from .decoder import unpack_rows
    return unpack_rows(words, nbits) if words.shape[1] else np.zeros((words.shape[0], nbits), np.uint8)


def dem_from_symptoms(cc, det_sym, obs_sym, num_detectors: int | None = None,
                      num_observables: int | None = None, mechanisms=None,
                      approximate_disjoint_errors: bool = False) -> DetectorErrorModel:
    """The DEM of a CompiledCircuit from the symptoms of its elementary noise
    faults: row f of det_sym / obs_sym = the detectors / observables fault f
    flips, as 0/1 rows (uint8) or packed words (int64 / uint64; then the counts
    default to the circuit's own detectors and observables), arrays or tensors.
    A mechanism's symptom is the XOR of its members' rows (a fault named twice
    cancels); mechanisms with identical (detectors, observables) merge by
    p <- p (1 - p') + p' (1 - p), folded in mechanism order; empty symptoms are
    dropped; columns come in order of first appearance; a column with
    observables and no detector is kept.  `mechanisms`: (probabilities, members)
    in place of fault_mechanisms(cc, approximate_disjoint_errors)."""
    det_in = np.asarray(det_sym.cpu().numpy() if hasattr(det_sym, "cpu") else det_sym)
    obs_in = np.asarray(obs_sym.cpu().numpy() if hasattr(obs_sym, "cpu") else obs_sym)
    packed_d, packed_o = det_in.dtype in (np.int64, np.uint64), obs_in.dtype in (np.int64, np.uint64)
    D = num_detectors if num_detectors is not None else (cc.detectors.shape[0] if packed_d else det_in.shape[1])
    K = num_observables if num_observables is not None else (cc.observables.shape[0] if packed_o else obs_in.shape[1])
    wd, wo = _as_words(det_in), _as_words(obs_in)
    if wd.shape[0] != wo.shape[0] or wd.shape[1] != (D + 63) // 64 or wo.shape[1] != (K + 63) // 64:
        raise ValueError("symptom rows do not fit the detector / observable counts")
    probs, members = fault_mechanisms(cc, approximate_disjoint_errors) if mechanisms is None else mechanisms
    probs, members = np.asarray(probs, np.float64), np.asarray(members, np.int64).reshape(-1, 4)
    if members.size and members.max() >= wd.shape[0]:
        raise ValueError(f"{wd.shape[0]} symptom rows for {int(members.max()) + 1} elementary faults")
    W = np.concatenate([wd, wo], axis=1)
    S = np.zeros((probs.size, W.shape[1]), np.uint64)
    for j in range(4):
        on = members[:, j] >= 0
        S[on] ^= W[members[on, j]]
    keep = S.any(axis=1)
    S, probs = S[keep], probs[keep]
    out: List[DemInstruction] = []
    if S.shape[0]:
        # equal rows by a stable lexicographic sort (np.unique(axis=0) compares rows as byte strings: ~10x slower)
        by_row = np.lexsort(S.T[::-1])
        edge = np.concatenate([[True], (S[by_row[1:]] != S[by_row[:-1]]).any(axis=1)])
        first = by_row[edge]                                 # stable: a group's first row is its earliest mechanism
        inv = np.empty(S.shape[0], np.int64)
        inv[by_row] = np.cumsum(edge) - 1
        rank_of = np.empty(first.size, np.int64)
        rank_of[np.argsort(first, kind="stable")] = np.arange(first.size)
        col = rank_of[inv]                                   # column of each mechanism, by first appearance
        order = np.argsort(col, kind="stable")               # mechanisms by column, in mechanism order within
        start = np.searchsorted(col[order], np.arange(first.size))
        size = np.diff(np.append(start, order.size))
        merged = probs[order[start]].copy()
        for r in range(1, int(size.max())):                  # the r-th member of every column that has one
            cols = np.nonzero(size > r)[0]
            p2 = probs[order[start[cols] + r]]
            merged[cols] = merged[cols] * (1.0 - p2) + p2 * (1.0 - merged[cols])
        rows = S[order[start]]
        dbits, obits = _bits_of(rows[:, :wd.shape[1]], D), _bits_of(rows[:, wd.shape[1]:], K)
        for c in range(rows.shape[0]):
            out.append(DemInstruction("error", [float(merged[c])], np.nonzero(dbits[c])[0].tolist(),
                                      np.nonzero(obits[c])[0].tolist()))
    out += [DemInstruction("detector", [], [d], []) for d in range(D)]
    out += [DemInstruction("logical_observable", [], [], [o]) for o in range(K)]
    return DetectorErrorModel(out)


def check_deterministic_symptoms(det_sym, obs_sym, num_detectors: int, num_observables: int) -> None:
    """From the symptoms of a circuit's gauge faults (kind 1; 0/1 rows or packed
    words): raise ValueError naming the first detector, else the first
    observable, that some reset's or measurement's random component flips.  Its
    parity is random in the noiseless circuit, and a DEM over it would be wrong."""
    for name, sym, n in (("detector", det_sym, num_detectors), ("observable", obs_sym, num_observables)):
        w = _as_words(sym)
        if w.size:
            hit = np.nonzero(_bits_of(np.bitwise_or.reduce(w, axis=0)[None], n)[0])[0]
            if hit.size:
                raise ValueError(f"{name} {int(hit[0])} is not deterministic: a reset's or measurement's random "
                                 f"component flips it in the noiseless circuit")


# the most symptom output one qd_circuit_faults_device call of detector_error_model
# writes: a circuit of 10^5 - 10^6 faults is propagated in windows of this size
FAULT_WINDOW_BYTES = 256 << 20


def detector_error_model(circuit, device: int = 0, check_deterministic: bool = True, detectors=None,
                         observables=None, approximate_disjoint_errors: bool = False) -> DetectorErrorModel:
    """The detector error model of a circuit (text, ParsedCircuit or
    CompiledCircuit) of the storage gate set: the counterpart of Stim's
    ``circuit.detector_error_model()`` (reference _experiment.py:174).  Detectors
    are the circuit's DETECTORs and observables its OBSERVABLE_INCLUDEs unless
    `detectors` / `observables` give matrices over the measurement records.
    Every elementary fault is propagated on `device` (qd_circuit_faults_device),
    in windows of at most FAULT_WINDOW_BYTES of symptoms.
    check_deterministic: the gauge faults (every reset's and measurement's
    randomised component) are propagated too, and a detector or observable one of
    them flips raises ValueError (check_deterministic_symptoms).
    approximate_disjoint_errors: a PAULI_CHANNEL_1 / 2 without an exact
    decomposition into independent flips (pauli_channel_components) contributes
    its arguments as independent probabilities instead of raising ValueError."""
    import torch
    from .circuit import CompiledCircuit, compile_circuit
    cc = circuit if isinstance(circuit, CompiledCircuit) else compile_circuit(circuit)
    prog = cc.with_groups({"detectors": cc.detectors if detectors is None else detectors,
                           "observables": cc.observables if observables is None else observables})
    D, K = prog.groups["detectors"].shape[0], prog.groups["observables"].shape[0]
    from .circuit import handle_fault_info
    mechanisms = fault_mechanisms(prog, approximate_disjoint_errors)   # refuses a channel before any launch
    row_bytes = 8 * ((D + 63) // 64 + (K + 63) // 64)
    window = max(64, FAULT_WINDOW_BYTES // max(row_bytes, 1) // 64 * 64)   # whole 64-fault words

    def symptoms(kind, total):
        """Packed symptom words of every fault of `kind` on the host, propagated a
        window at a time so that no call asks the device for more than
        FAULT_WINDOW_BYTES of output."""
        det, obs = [], []
        for f0 in range(0, max(total, 1), window):
            s = prog.fault_symptoms_device(kind=kind, f0=f0, F=min(window, total - f0), device=device)
            det.append(s["detectors"].cpu().numpy())
            obs.append(s["observables"].cpu().numpy())
        return np.concatenate(det), np.concatenate(obs)

    try:
        with torch.cuda.device(device):
            noise, gauge = handle_fault_info(prog.handle(device))
            if check_deterministic:
                check_deterministic_symptoms(*symptoms(1, gauge), D, K)
            return dem_from_symptoms(prog, *symptoms(0, noise), D, K, mechanisms=mechanisms)
    finally:
        prog.close()
