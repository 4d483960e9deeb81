"""Stim-style circuit text -> a Pauli-frame program for the device sampler.

``parse`` reads the subset of Stim's circuit language that the reference's
storage circuits (``python/qldpc/storage_sim.py:110-199``) and noise rewriters
(``noise_model.py:117-151``) produce; ``compile_circuit`` turns it into a
``CompiledCircuit``: flat integer arrays the C ABI takes (``qd_circuit_create``,
include/qdec.h), one probability / u32 threshold per instruction, and the
detector and observable rows as CSR matrices over absolute record indices.
``PAULI_CHANNEL_1(px, py, pz)`` and ``PAULI_CHANNEL_2(15 probabilities, Stim's
order IX .. ZZ)`` keep their arguments in ``CompiledCircuit.args``; their entry
of ``probs`` is the sum (``qd_circuit_create_args``).

Stim applies an instruction's targets in order.  The compiler splits every gate,
reset and measurement instruction into groups whose qubits are pairwise
disjoint, so the kernel (csrc/qdec_frame.hip) may apply one group in parallel;
``MR`` / ``MRX`` become a measurement group followed by a reset group.

The sampled record is the flip against the noiseless reference sample.  For
the storage circuits that sample is all zero (every deterministic measurement
reads 0 and a random one may be taken as 0), which is the default here;
``reference_sample`` gives other circuits theirs, folded into the measurement
targets as an invert bit.  An implicit ``R`` of every qubit opens the program,
Stim's initial state.
"""
from __future__ import annotations

import ctypes as C
import re
from dataclasses import dataclass, field
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import scipy.sparse as sp

__all__ = ["CompiledCircuit", "Instruction", "ParsedCircuit", "compile_circuit", "parse", "bern_threshold",
           "SUPPORTED", "OPCODES", "CHANNEL_ARGS", "INVERT", "MAX_GROUPS", "LDS_LIMIT", "FRAME_PLACEMENTS"]

OP_H, OP_CX, OP_CZ, OP_R, OP_RX, OP_M, OP_MX, OP_XERR, OP_YERR, OP_ZERR, OP_DEP1, OP_DEP2, OP_PC1, OP_PC2 = range(14)
OPCODES = {"H": OP_H, "CX": OP_CX, "CZ": OP_CZ, "R": OP_R, "RX": OP_RX, "M": OP_M, "MX": OP_MX,
           "X_ERROR": OP_XERR, "Y_ERROR": OP_YERR, "Z_ERROR": OP_ZERR, "DEPOLARIZE1": OP_DEP1,
           "DEPOLARIZE2": OP_DEP2, "PAULI_CHANNEL_1": OP_PC1, "PAULI_CHANNEL_2": OP_PC2}
# noise instructions with one probability per outcome: name -> argument count
CHANNEL_ARGS = {"PAULI_CHANNEL_1": 3, "PAULI_CHANNEL_2": 15}
INVERT = 1 << 30       # measurement target bit: record inverted
MAX_GROUPS = 4
LDS_LIMIT = 160 * 1024
# where the kernels keep the frame (include/qdec.h QD_FRAME_*): "auto" = LDS when
# 16 Q + 8 M fits LDS_LIMIT, else a slot per workgroup in device memory
FRAME_PLACEMENTS = {"lds": 0, "hbm": 1, "auto": 2}

_ALIAS = {"RZ": "R", "MZ": "M", "MRZ": "MR", "CNOT": "CX"}
_RESETS = ("R", "RX")
_MEASURES = ("M", "MX", "MR", "MRX")
_GATES = ("H", "CX", "CZ")
_NOISE = ("X_ERROR", "Y_ERROR", "Z_ERROR", "DEPOLARIZE1", "DEPOLARIZE2", "PAULI_CHANNEL_1", "PAULI_CHANNEL_2")
_ANNOT = ("TICK", "REPEAT", "DETECTOR", "OBSERVABLE_INCLUDE", "SHIFT_COORDS", "QUBIT_COORDS")
_PAIRED = ("CX", "CZ", "DEPOLARIZE2", "PAULI_CHANNEL_2")
SUPPORTED = tuple(sorted(set(_RESETS + _MEASURES + _GATES + _NOISE + _ANNOT + tuple(_ALIAS))))

_LINE_RE = re.compile(r"^([A-Za-z_][A-Za-z0-9_]*)\s*(?:\(([^)]*)\))?\s*(.*)$")
_REC_RE = re.compile(r"^rec\[-(\d+)\]$", re.I)


def bern_threshold(p) -> np.ndarray:
    """Probability -> the samplers' u32 threshold (csrc/qdec_tables.h
    bern_threshold): 0 unless p > 0, else floor(p 2^32) clamped to 2^32 - 1."""
    p = np.asarray(p, dtype=np.float64)
    v = np.floor(np.where(p > 0, p, 0.0) * 4294967296.0)
    return np.where(v >= 4294967295.0, 4294967295.0, v).astype(np.uint64).astype(np.uint32)


@dataclass(frozen=True)
class Instruction:
    """One unrolled instruction: canonical name, probability argument (0 when
    absent), targets (qubit, or qubit | INVERT for an inverted measurement).
    PAULI_CHANNEL_1 / 2: `args` holds the 3 / 15 probabilities and `p` their sum
    (c_k = c_{k-1} + a_k in double, left to right)."""
    name: str
    p: float
    targets: Tuple[int, ...]
    args: Tuple[float, ...] = ()


@dataclass
class ParsedCircuit:
    instructions: List[Instruction]
    num_qubits: int
    num_measurements: int
    detectors: List[List[int]]            # absolute record indices per detector, in text order
    observables: Dict[int, List[int]]     # observable index -> record indices (lines accumulate)
    ticks: int = 0


def _unsupported(name: str, line: str):
    return ValueError(f"unsupported instruction {name!r} in line {line!r}; supported: {', '.join(SUPPORTED)}")


def _blocks(lines: Sequence[str]):
    """Nest the text: a list of (name, arg, rest, line) and ('REPEAT', n, body)."""
    stack = [[]]
    counts = []
    for raw in lines:
        line = raw.split("#")[0].strip()
        if not line:
            continue
        if line == "}":
            if not counts:
                raise ValueError("unmatched '}'")
            body = stack.pop()
            stack[-1].append(("REPEAT", counts.pop(), body))
            continue
        m = _LINE_RE.match(line)
        if m is None:
            raise ValueError(f"cannot parse line {raw!r}")
        name, arg, rest = m.group(1).upper(), m.group(2), m.group(3).strip()
        if name == "REPEAT":
            mm = re.match(r"^(\d+)\s*\{$", rest)
            if mm is None or arg is not None:
                raise ValueError(f"malformed REPEAT: {raw!r}")
            counts.append(int(mm.group(1)))
            stack.append([])
            continue
        stack[-1].append((name, arg, rest, line))
    if counts:
        raise ValueError("REPEAT block not closed")
    return stack[0]


def parse(text) -> ParsedCircuit:
    """Parse circuit text (a string or an iterable of lines) and unroll its
    REPEAT blocks; ``rec[-k]`` is resolved against the measurements made so far
    at that point of the unrolled program."""
    lines = text.splitlines() if isinstance(text, str) else [l for t in text for l in str(t).splitlines()]
    out = ParsedCircuit([], 0, 0, [], {})

    def records(rest, line):
        idx = []
        for tok in rest.split():
            m = _REC_RE.match(tok)
            if m is None:
                raise ValueError(f"expected rec[-k] targets in line {line!r}")
            k = int(m.group(1))
            if k < 1 or k > out.num_measurements:
                raise ValueError(f"rec[-{k}] looks back before the start of the record in line {line!r}")
            idx.append(out.num_measurements - k)
        return idx

    def run(block):
        for item in block:
            if item[0] == "REPEAT":
                for _ in range(item[1]):
                    run(item[2])
                continue
            name, arg, rest, line = item
            name = _ALIAS.get(name, name)
            if name == "TICK":
                out.ticks += 1
            elif name in ("SHIFT_COORDS", "QUBIT_COORDS"):
                pass
            elif name == "DETECTOR":
                out.detectors.append(records(rest, line))
            elif name == "OBSERVABLE_INCLUDE":
                try:
                    i = int(float(arg))
                except (TypeError, ValueError):
                    raise ValueError(f"OBSERVABLE_INCLUDE needs an index: {line!r}") from None
                out.observables.setdefault(i, []).extend(records(rest, line))
            elif name in _RESETS or name in _MEASURES or name in _GATES or name in _NOISE:
                p, chan = 0.0, ()
                if name in CHANNEL_ARGS:
                    try:
                        chan = tuple(float(a) for a in arg.split(",")) if arg is not None and arg.strip() else ()
                    except ValueError:
                        raise ValueError(f"bad probability in line {line!r}") from None
                    if len(chan) != CHANNEL_ARGS[name]:
                        raise ValueError(f"{name} takes {CHANNEL_ARGS[name]} probabilities, not {len(chan)}: {line!r}")
                    if not all(0.0 <= a <= 1.0 for a in chan):
                        raise ValueError(f"probability outside [0, 1] in line {line!r}")
                    for a in chan:
                        p += a
                    if p > 1.0 + 1e-12:
                        raise ValueError(f"the probabilities of {name} sum to more than 1 in line {line!r}")
                elif arg is not None:
                    if name in _RESETS or name in _GATES:
                        raise ValueError(f"{name} takes no argument: {line!r}")
                    try:
                        p = float(arg)
                    except ValueError:
                        raise ValueError(f"bad probability in line {line!r}") from None
                    if not 0.0 <= p <= 1.0:
                        raise ValueError(f"probability outside [0, 1] in line {line!r}")
                elif name in _NOISE:
                    raise ValueError(f"{name} needs a probability: {line!r}")
                tg = []
                for tok in rest.split():
                    inv = tok.startswith("!")
                    if inv and name not in _MEASURES:
                        raise ValueError(f"'!' is a measurement target modifier: {line!r}")
                    try:
                        q = int(tok[1:] if inv else tok)
                    except ValueError:
                        raise ValueError(f"bad target {tok!r} in line {line!r}") from None
                    if q < 0 or q >= INVERT:
                        raise ValueError(f"bad target {tok!r} in line {line!r}")
                    tg.append(q | (INVERT if inv else 0))
                    out.num_qubits = max(out.num_qubits, q + 1)
                if name in _PAIRED and len(tg) % 2:
                    raise ValueError(f"odd number of targets for the two-qubit instruction {name}: {line!r}")
                if name in _MEASURES:
                    out.num_measurements += len(tg)
                out.instructions.append(Instruction(name, p, tuple(tg), chan))
            else:
                raise _unsupported(name, line)

    run(_blocks(lines))
    return out


def _disjoint_groups(targets: Sequence[int], width: int) -> List[List[int]]:
    """Split a target list (width 1, or 2 for pairs) in order into maximal runs
    whose qubits are pairwise disjoint."""
    groups, cur, used = [], [], set()
    for i in range(0, len(targets), width):
        qs = [t & (INVERT - 1) for t in targets[i:i + width]]
        if len(set(qs)) < width:
            raise ValueError(f"a two-qubit instruction on one qubit: {qs}")
        if used.intersection(qs):
            groups.append(cur)
            cur, used = [], set()
        cur.extend(targets[i:i + width])
        used.update(qs)
    if cur:
        groups.append(cur)
    return groups


def _rows_csr(rows: Iterable[Iterable[int]], ncols: int) -> sp.csr_matrix:
    """CSR (uint8) of index lists, duplicates cancelled mod 2, indices sorted."""
    ptr, idx = [0], []
    for r in rows:
        u, cnt = np.unique(np.asarray(list(r), dtype=np.int64), return_counts=True)
        idx.extend(u[cnt % 2 == 1].tolist())
        ptr.append(len(idx))
    return sp.csr_matrix((np.ones(len(idx), np.uint8), np.asarray(idx, np.int32), np.asarray(ptr, np.int32)),
                         shape=(len(ptr) - 1, ncols))


def compile_circuit(text, reference_sample=None, groups: Optional[Dict[str, object]] = None) -> "CompiledCircuit":
    """Compile circuit text (or a ParsedCircuit).  `groups`: the program's output
    groups by name, each a sparse matrix over record bits (at most four); default
    the standard three, ``detectors``, ``observables`` and ``records``."""
    pc = text if isinstance(text, ParsedCircuit) else parse(text)
    Q, M = max(pc.num_qubits, 1), pc.num_measurements
    ref = None
    if reference_sample is not None:
        ref = np.asarray(reference_sample).astype(bool).ravel()
        if ref.size != M:
            raise ValueError(f"reference_sample has {ref.size} bits, the circuit {M} measurements")
    ops, targets, probs, args = [], [], [], []

    def emit(op, tg, p=0.0, chan=()):
        ops.append((op, len(targets), len(tg), len(args) if chan else 0))
        targets.extend(tg)
        probs.append(p)
        args.extend(chan)

    emit(OP_R, list(range(Q)))  # Stim's initial state: every qubit reset
    rec = 0
    # adjacent instructions of one name and argument are one target list (the
    # reference writes a CX per line): the groups below then span the lines
    fused: List[Tuple[str, float, list, tuple]] = []
    for ins in pc.instructions:
        if fused and ins.name not in _NOISE and fused[-1][0] == ins.name and fused[-1][1] == ins.p:
            fused[-1][2].extend(ins.targets)
        else:
            fused.append((ins.name, ins.p, list(ins.targets), ins.args))
    for name, p_arg, tg, chan in fused:
        if not tg:
            continue
        if name in _NOISE:
            emit(OPCODES[name], tg, p_arg, chan)
            continue
        for g in _disjoint_groups(tg, 2 if name in _PAIRED else 1):
            if name in _MEASURES:
                if ref is not None:
                    g = [t ^ (INVERT if ref[rec + i] else 0) for i, t in enumerate(g)]
                rec += len(g)
                emit(OP_MX if name in ("MX", "MRX") else OP_M, g, p_arg)
                if name in ("MR", "MRX"):
                    emit(OP_RX if name == "MRX" else OP_R, [t & (INVERT - 1) for t in g])
            else:
                emit(OPCODES[name], g)
    nobs = max(pc.observables) + 1 if pc.observables else 0
    cc = CompiledCircuit(
        num_qubits=Q, num_measurements=M,
        ops=np.asarray(ops, dtype=np.int32).reshape(-1, 4), targets=np.asarray(targets, dtype=np.int32),
        probs=np.asarray(probs, dtype=np.float64),
        detectors=_rows_csr(pc.detectors, M),
        observables=_rows_csr([pc.observables.get(i, []) for i in range(nobs)], M),
        args=np.asarray(args, dtype=np.float64))
    cc.thresholds = bern_threshold(cc.probs)
    if groups is None:
        groups = {"detectors": cc.detectors, "observables": cc.observables, "records": cc.record_rows()}
    return cc.with_groups(groups)


@dataclass
class CompiledCircuit:
    """A circuit as the device sampler takes it (see the module docstring)."""
    num_qubits: int
    num_measurements: int
    ops: np.ndarray            # int32 [n_ops, 4]: opcode, first target, target count, first argument (else 0)
    targets: np.ndarray        # int32 [n_targets]
    probs: np.ndarray          # float64 [n_ops]
    detectors: sp.csr_matrix   # [D, M] over absolute record indices
    observables: sp.csr_matrix  # [K, M]
    thresholds: np.ndarray = None   # uint32 [n_ops]: bern_threshold(probs)
    groups: Dict[str, sp.csr_matrix] = field(default_factory=dict)
    args: np.ndarray = field(default_factory=lambda: np.zeros(0, np.float64))   # float64: PAULI_CHANNEL arguments
    _handles: dict = field(default_factory=dict, repr=False)

    # ---- output groups
    def record_rows(self, start: int = 0, stop: Optional[int] = None) -> sp.csr_matrix:
        """Identity rows over records start .. stop (default: all of them)."""
        stop = self.num_measurements if stop is None else stop
        k = stop - start
        return sp.csr_matrix((np.ones(k, np.uint8), (np.arange(k), np.arange(start, stop))),
                             shape=(k, self.num_measurements))

    def with_groups(self, groups: Dict[str, object]) -> "CompiledCircuit":
        """The same program with other output groups (at most four)."""
        if len(groups) > MAX_GROUPS:
            raise ValueError(f"a program carries at most {MAX_GROUPS} output groups")
        g = {}
        for name, mat in groups.items():
            mat = sp.csr_matrix(mat)
            if mat.shape[1] != self.num_measurements:
                raise ValueError(f"group {name!r} has {mat.shape[1]} columns, the circuit "
                                 f"{self.num_measurements} measurements")
            mat = mat.astype(np.uint8)
            mat.sum_duplicates()
            mat.data %= 2
            mat.eliminate_zeros()
            mat.sort_indices()
            g[name] = mat
        return CompiledCircuit(self.num_qubits, self.num_measurements, self.ops, self.targets, self.probs,
                               self.detectors, self.observables, self.thresholds, g, self.args)

    @property
    def lds_bytes(self) -> int:
        return 16 * self.num_qubits + 8 * self.num_measurements

    def abi_arrays(self):
        """(ops, targets, probs, group_rows, row_ptr, rec_idx) as qd_circuit_create takes them."""
        mats = list(self.groups.values())
        rows = np.asarray([m.shape[0] for m in mats], dtype=np.int32)
        ptr, idx, base = [np.zeros(1, np.int32)], [], 0
        for m in mats:
            ptr.append(m.indptr[1:].astype(np.int32) + base)
            idx.append(m.indices.astype(np.int32))
            base += int(m.indptr[-1])
        return (np.ascontiguousarray(self.ops, dtype=np.int32), np.ascontiguousarray(self.targets, dtype=np.int32),
                np.ascontiguousarray(self.probs, dtype=np.float64), rows, np.concatenate(ptr),
                np.concatenate(idx) if idx else np.zeros(0, np.int32))

    # ---- handles
    def _create(self, device: Optional[int], frame: Optional[str] = "auto"):
        return create_handle(self.num_qubits, *self.abi_arrays(), device=device, frame=frame, args=self.args)

    def validate(self, frame: Optional[str] = "auto") -> dict:
        """Run the library's validation without a device
        (qd_circuit_create_host_placed) and return qd_circuit_info's figures."""
        h = self._create(None, frame)
        try:
            return handle_info(h)
        finally:
            destroy_handle(h)

    def frame_info(self, device: Optional[int] = None, frame: Optional[str] = "auto") -> dict:
        """qd_circuit_frame_info of the (device, frame) handle, or with
        device=None of a host-only handle made for the call."""
        if device is not None:
            return handle_frame_info(self.handle(device, frame))
        h = self._create(None, frame)
        try:
            return handle_frame_info(h)
        finally:
            destroy_handle(h)

    def handle(self, device: int = 0, frame: Optional[str] = "auto"):
        if (device, frame) not in self._handles:
            self._handles[(device, frame)] = self._create(device, frame)
        return self._handles[(device, frame)]

    def set_frame_slots(self, slots: int, device: int = 0, frame: Optional[str] = "auto") -> None:
        """Slots (resident workgroups) of the HBM kernels' launches on this
        handle; 0 = the default.  Results do not depend on it."""
        from . import _abi
        _abi.check(_abi.load().qd_circuit_set_frame_slots(self.handle(device, frame), int(slots)),
                   "qd_circuit_set_frame_slots")

    def close(self):
        for h in self._handles.values():
            destroy_handle(h)
        self._handles.clear()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- sampling
    def _output_tensors(self, n: int, packed: bool, outputs, out: Optional[dict], device: int):
        """The {group name: tensor} of a sample / fault call and its c_void_p
        list: n rows per group of `outputs` (default: every group), uint8
        [n, rows] or with packed int64 [n, ceil(rows / 64)]; tensors of `out`
        are checked and used instead of new ones."""
        import torch
        names = list(self.groups) if outputs is None else list(outputs)
        for nme in names:
            if nme not in self.groups:
                raise KeyError(f"no output group {nme!r}; the program has {list(self.groups)}")
        dev = torch.device("cuda", device)
        res, ptrs = {}, (C.c_void_p * MAX_GROUPS)()
        for g, (nme, mat) in enumerate(self.groups.items()):
            if nme not in names:
                continue
            rows = mat.shape[0]
            shape = (n, (rows + 63) // 64) if packed else (n, rows)
            dt = torch.int64 if packed else torch.uint8
            t = out[nme] if out is not None and nme in out else torch.empty(shape, dtype=dt, device=dev)
            if tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous():
                raise ValueError(f"output {nme!r} must be a contiguous {dt} tensor of shape {shape}")
            res[nme] = t
            ptrs[g] = t.data_ptr() if t.numel() else None
        return res, C.cast(ptrs, C.c_void_p), dev

    def sample_device(self, B: int, seed: int, stream_id: int = 0, shot0: int = 0, packed: bool = False,
                      outputs: Optional[Sequence[str]] = None, device: int = 0, out: Optional[dict] = None,
                      stream=None, frame: Optional[str] = "auto") -> dict:
        """Sample B shots (global indices shot0 .. shot0 + B) on `device`; `frame`
        places the frame (FRAME_PLACEMENTS; every placement gives the same bits).
        Returns {group name: tensor} for `outputs` (default: every group):
        uint8 [B, rows], or with packed=True int64 [B, ceil(rows / 64)] holding
        the decode's packed u64 words.  `out` supplies the tensors to write."""
        import torch
        from . import _abi
        res, ptrs, dev = self._output_tensors(B, packed, outputs, out, device)
        s = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        _abi.check(_abi.load().qd_circuit_sample_device(self.handle(device, frame), seed & 0xFFFFFFFF,
                                                        stream_id & 0xFFFFFFFF, int(shot0), int(B),
                                                        _abi.QD_INPUT_PACKED if packed else 0, ptrs, C.c_void_p(s)),
                   "qd_circuit_sample_device")
        return res

    # ---- elementary faults (include/qdec.h, "Fault propagation"; composed into a DEM by dem.py)
    def fault_table(self, kind: int = 0):
        """The library's table of the circuit's elementary faults of one kind
        (0 noise, 1 gauge), from a host-only handle: int32 arrays (instruction
        index, index into ``targets``, component: 1 x, 2 z, 3 both, 4 a record flip)."""
        from . import _abi
        lib = _abi.load()
        h = self._create(None)
        try:
            if kind not in (0, 1):
                raise ValueError("fault kind must be 0 (noise) or 1 (gauge)")
            n = handle_fault_info(h)[kind]
            op, tgt, comp = (np.zeros(n, np.int32) for _ in range(3))
            _abi.check(lib.qd_circuit_fault_table(h, int(kind), _abi.ptr(op), _abi.ptr(tgt), _abi.ptr(comp)),
                       "qd_circuit_fault_table")
            return op, tgt, comp
        finally:
            destroy_handle(h)

    def fault_symptoms_device(self, kind: int = 0, f0: int = 0, F: Optional[int] = None, packed: bool = True,
                              outputs: Optional[Sequence[str]] = None, device: int = 0, stream=None,
                              frame: Optional[str] = "auto") -> dict:
        """Propagate faults f0 .. f0 + F of one kind (default: all from f0) through
        the circuit on `device` (qd_circuit_faults_device).  Returns {group name:
        tensor} like sample_device, row f the symptom of fault f0 + f alone."""
        import torch
        from . import _abi
        if F is None:
            if kind not in (0, 1):
                raise ValueError("fault kind must be 0 (noise) or 1 (gauge)")
            F = handle_fault_info(self.handle(device, frame))[kind] - int(f0)
        res, ptrs, dev = self._output_tensors(max(F, 0), packed, outputs, None, device)
        s = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        _abi.check(_abi.load().qd_circuit_faults_device(self.handle(device, frame), int(kind), int(f0), int(F),
                                                        _abi.QD_INPUT_PACKED if packed else 0, ptrs, C.c_void_p(s)),
                   "qd_circuit_faults_device")
        return res


# ---- the raw ABI (tests hand qd_circuit_create_host broken programs through these)
def create_handle(num_qubits, ops, targets, probs, group_rows, row_ptr, rec_idx, device: Optional[int] = None,
                  frame=None, args=None):
    """qd_circuit_create (device ordinal) or qd_circuit_create_host (None);
    with `frame` ("lds", "hbm", "auto", or a raw placement number) the _placed
    entry points.  `args`: the PAULI_CHANNEL arguments; a program with such an
    instruction goes through qd_circuit_create_args / _create_host_args (frame
    None there means "lds", as in the entry points without a placement).  Raises
    _abi.QdecError carrying the library's code."""
    from . import _abi
    lib = _abi.load()
    ops = np.ascontiguousarray(ops, dtype=np.int32).reshape(-1, 4)
    targets = np.ascontiguousarray(targets, dtype=np.int32)
    probs = np.ascontiguousarray(probs, dtype=np.float64)
    group_rows = np.ascontiguousarray(group_rows, dtype=np.int32)
    row_ptr = np.ascontiguousarray(row_ptr, dtype=np.int32)
    rec_idx = np.ascontiguousarray(rec_idx, dtype=np.int32)
    if probs.size != ops.shape[0] or row_ptr.size != int(group_rows.sum()) + 1 or \
            (row_ptr.size and rec_idx.size < max(int(row_ptr[-1]), 0)):
        raise ValueError("circuit arrays do not fit together")
    h = C.c_void_p()
    head = (int(num_qubits), ops.shape[0], _abi.ptr(ops), targets.size, _abi.ptr(targets), _abi.ptr(probs),
            group_rows.size, _abi.ptr(group_rows), _abi.ptr(row_ptr), _abi.ptr(rec_idx))
    place = None if frame is None else FRAME_PLACEMENTS[frame] if isinstance(frame, str) else int(frame)
    if args is not None and ops.size and bool((ops[:, 0] >= OP_PC1).any()):
        chan = np.ascontiguousarray(args, dtype=np.float64)
        place = FRAME_PLACEMENTS["lds"] if place is None else place
        if device is None:
            _abi.check(lib.qd_circuit_create_host_args(place, *head, chan.size, _abi.ptr(chan), C.byref(h)),
                       "qd_circuit_create_host_args")
        else:
            _abi.check(lib.qd_circuit_create_args(place, int(device), *head, chan.size, _abi.ptr(chan), C.byref(h)),
                       "qd_circuit_create_args")
        return h
    args = head + (C.byref(h),)
    if place is not None:
        if device is None:
            _abi.check(lib.qd_circuit_create_host_placed(place, *args), "qd_circuit_create_host_placed")
        else:
            _abi.check(lib.qd_circuit_create_placed(place, int(device), *args), "qd_circuit_create_placed")
    elif device is None:
        _abi.check(lib.qd_circuit_create_host(*args), "qd_circuit_create_host")
    else:
        _abi.check(lib.qd_circuit_create(int(device), *args), "qd_circuit_create")
    return h


def handle_frame_info(h) -> dict:
    """qd_circuit_frame_info: the placement in effect, bytes per slot, the slots
    of the last HBM launch and the scratch bytes held."""
    from . import _abi
    out = np.zeros(4, np.int64)
    _abi.check(_abi.load().qd_circuit_frame_info(h, _abi.ptr(out)), "qd_circuit_frame_info")
    return {"placement": {v: k for k, v in FRAME_PLACEMENTS.items()}[int(out[0])], "slot_bytes": int(out[1]),
            "slots": int(out[2]), "scratch_bytes": int(out[3])}


def handle_op_flags(h) -> np.ndarray:
    """int32 [instructions]: 1 where a noise instruction names a qubit more than
    once (qd_circuit_op_flags_copy)."""
    from . import _abi
    out = np.zeros(handle_info(h)["instructions"], np.int32)
    _abi.check(_abi.load().qd_circuit_op_flags_copy(h, _abi.ptr(out)), "qd_circuit_op_flags_copy")
    return out


def handle_info(h) -> dict:
    from . import _abi
    out = np.zeros(10, np.int64)
    _abi.check(_abi.load().qd_circuit_info(h, _abi.ptr(out)), "qd_circuit_info")
    return {"qubits": int(out[0]), "measurements": int(out[1]), "group_rows": [int(v) for v in out[2:6]],
            "lds_bytes": int(out[6]), "instructions": int(out[7]), "sites": int(out[8]), "rand_sites": int(out[9])}


def handle_fault_info(h) -> Tuple[int, int]:
    """(noise faults, gauge faults) of a handle (qd_circuit_fault_info)."""
    from . import _abi
    out = np.zeros(4, np.int64)
    _abi.check(_abi.load().qd_circuit_fault_info(h, _abi.ptr(out)), "qd_circuit_fault_info")
    return int(out[0]), int(out[1])


def destroy_handle(h) -> None:
    from . import _abi
    _abi.load().qd_circuit_destroy(h)
