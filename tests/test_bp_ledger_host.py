"""CPU side of tests/bp_cases.py: the launch plan of every case by entry name
(qd_graph_plan_entries, which also names the stages last_kernels() leaves out),
the second instantiation ledger -- every entry of the kernel tables outside the
ledger of tests/test_ssf_mixed_host.py against the cases tests/test_gpu_bp_ledger.py
launches -- and, on the oracle alone, the conditions that keep a case from
passing vacuously.  No GPU."""
import ctypes as C
import itertools

import numpy as np
import pytest

import bp_cases as bc
import ssf_cases as sc
import test_ssf_mixed_host as mixed
from test_ssf_mixed_host import HostGraphs, in_ledger, kernel_table_names

PLAN_FIELDS = ("bp", "fin", "two_pass", "expand_packed", "fuse", "q_rpar", "placement", "buffers")


def plan_entries(lib, h, case):
    """(plan fields, (bp, ssf, pre) entry names) of a case on host graph h."""
    from exp_ldpc_amd import _abi
    from exp_ldpc_amd.decoder import OPTIONS, SSF_KERNELS, parse_bp_method, parse_precision
    opts, present = bc.plan_request(case)
    for name, value in opts.items():
        _abi.check(lib.qd_graph_set_option(h, OPTIONS[name], SSF_KERNELS.get(value, value)), name)
    _abi.check(lib.qd_graph_set_wave_occupancy(h, case["occ"]), "occupancy")
    prm = _abi.QdParams(case["max_iter"], parse_bp_method(case["method"]), parse_precision(case["precision"]),
                        int(case["ssf"]), case["steps"],
                        case["syn_flags"] | (_abi.QD_INPUT_PACKED if case["packed"] else 0), case["scaling"])
    mask = sum(mixed.PRESENT[k] for k in present) | mixed.ALIGNED
    out = np.zeros(8, np.int32)
    _abi.check(lib.qd_graph_plan(h, C.byref(prm), case["B"], mask, _abi.ptr(out)), "qd_graph_plan")
    bufs = [C.create_string_buffer(512) for _ in range(3)]
    _abi.check(lib.qd_graph_plan_entries(h, C.byref(prm), case["B"], mask, bufs[0], 512, bufs[1], 512, bufs[2], 512),
               "qd_graph_plan_entries")
    noted = [C.create_string_buffer(512) for _ in range(3)]
    _abi.check(lib.qd_graph_plan_names(h, C.byref(prm), case["B"], mask, noted[0], 512, noted[1], 512, noted[2], 512),
               "qd_graph_plan_names")
    names = tuple(b.value.decode() for b in bufs)
    # the recorded names are the entries, or "" for a stage that records none
    assert all(n in ("", e) for n, e in zip((b.value.decode() for b in noted), names)), (case["id"], names)
    return dict(zip(PLAN_FIELDS, (int(v) for v in out))), names


@pytest.fixture(scope="module")
def lib():
    from exp_ldpc_amd import _abi
    return _abi.load()


@pytest.fixture(scope="module")
def planned(lib):
    """{case id: (plan, entry names)} of every case of bp_cases."""
    graphs = HostGraphs(lib)
    try:
        cases = sorted(bc.all_cases(), key=lambda c: (c["graph"], c["n_gen"], c["max_lc"]))
        return {c["id"]: plan_entries(lib, graphs.get(c), c) for c in cases}
    finally:
        graphs.close()


@pytest.fixture(scope="module")
def planned_mixed(lib):
    """The names the cases of ssf_cases plan (the first ledger's side)."""
    graphs = HostGraphs(lib)
    try:
        cases = sorted(sc.all_cases(), key=lambda c: (c["graph"], c["n_gen"], c["max_lc"]))
        return {n for c in cases for n in mixed.plan_case(lib, graphs.get(c), c)[1] if n}
    finally:
        graphs.close()


def test_plan_entries_names_the_unrecorded_stages(lib):
    """qd_graph_plan_entries next to qd_graph_plan_names on the 4 x 21 graph:
    bp_block_kernel and the workgroup SSF kernel under their table names where
    the recorded names stay "", a stage without an entry "" in both, and a short
    buffer gets a cut, terminated copy."""
    from exp_ldpc_amd import _abi
    graphs = HostGraphs(lib)
    try:
        c = bc._case("block", "gen3s", n_gen=bc.N_GEN, max_lc=bc.MAX_LC, method="ps", precision="f32", B=5)
        h = graphs.get(c)
        assert plan_entries(lib, h, c)[1] == ("qdec::bp_block_kernel<float, 0, true, 0, 0>",
                                              "qdec::ssf_inc_block_kernel", "")
        assert mixed.plan_case(lib, h, c)[1] == ("", "", "")
        prm = _abi.QdParams(3, 0, 1, 1, 0, 0, 0.0)
        small = C.create_string_buffer(b"\xff" * 12, 12)
        _abi.check(lib.qd_graph_plan_entries(h, C.byref(prm), 5, 1 | 128, small, 12, None, 0, None, 0), "entries")
        assert small.raw == b"qdec::bp_bl\0"
        assert lib.qd_graph_plan_entries(h, None, 5, 1, None, 0, None, 0, None, 0) != 0
    finally:
        graphs.close()


def test_every_case_plans_what_it_names(planned):
    """Each case names its three entries in full; the plan of the same request
    on a host-only graph gives exactly them, and for the workgroup cases the
    BP path, the SSF path and the placement the cell stands for."""
    cases = bc.all_cases()
    assert len({c["id"] for c in cases}) == len(cases)
    for c in cases:
        plan, names = planned[c["id"]]
        assert names == (c["bp"], c["fin"], c["pre"]), (c["id"], plan, names)
        if c["kind"] == "block":
            assert (plan["bp"], plan["fin"], plan["placement"]) == c["path"], (c["id"], plan)
        else:
            two = "cmp_kernel" in c["bp"]
            assert plan["bp"] == (0 if c["method"] == "ps" else 2 if two else 1) and plan["placement"] == 3, c["id"]
            assert plan["fin"] == (2 if c["ssf"] else 0), (c["id"], plan)
            assert plan["expand_packed"] == int(c["packed"] and c["pre"].endswith("false>")), (c["id"], plan)


def test_workgroup_cases_cover_every_cell():
    """T x METHOD x DEFER x {unrolled, generic} x placement {3, 2, 0}: 48 cells,
    each with a case; both workgroup SSF kernels at placements 3 and 2, the
    HBM-state one at 0; 5 and 130 shots where the state is in LDS, and a batch
    beyond one launch's workgroups (bp_cases.MANY); each body once from base and
    readout."""
    cells = {}
    for c in bc.all_cases():
        if c["kind"] == "block":
            cells.setdefault((c["bp"], c["path"][2]), []).append(c)
    assert len(cells) == 48
    for (bp, placement), cs in cells.items():
        assert {c["B"] for c in cs} == ({5, 130, bc.MANY[placement][0]} if placement else {5}), bp
        assert all(c["options"].get("block_wg", 0) == (bc.MANY[2][1] if placement == 2 and c["B"] > 130 else 0)
                   for c in cs)
        assert all(c["max_iter"] <= 25 for c in cs)
        if ", true, " in bp:
            assert {c["path"][1] for c in cs} == ({6, 7} if placement else {8}), bp
            assert all(c["ssf"] and set(c["want"]) == set(sc.SSF_WANT) for c in cs)
        else:
            assert all(set(c["want"]) == set(bc.FULL_WANT) for c in cs)
    flagged = {c["bp"] for c in bc.all_cases() if c["syn_flags"] == 3}
    assert any(b.endswith("0, 0>") for b in flagged) and any(b.endswith("16, 8>") for b in flagged)
    for key in bc.BLOCK_CELLS:  # per-column priors, logicals for the failure flag
        _, probs, L = sc.graph(key)
        assert len(set(np.asarray(probs).tolist())) > 4 and np.asarray(L).any()


# Built, but no input reaches the plan's branch (plan_decode_wave): the lean
# deferring kernels hand their failed shots to the packed queue of the wave SSF
# kernels, which a graph of shape (4, 9, 8) never has (its 256 padded checks are
# beyond their u8 check ids; test_ssf_mixed_host.UNREACHED), so with SSF its plan
# is never lean and never two-pass.  test_shape_498_is_never_lean_with_ssf
# establishes it.
_NOT_LEAN = ("shape (4, 9, 8) pads to 256 checks, beyond the u8 check ids of the packed SSF queue: "
             "a deferring decode on it is never lean")
UNREACHED = {
    **{f"qdec::bp_ms_wave_kernel<{T}, 4, 9, 8, true, true, 0, 0>": _NOT_LEAN for T in ("float", "double")},
    **{f"qdec::bp_ms_cmp_kernel<{T}, 4, 9, 8, true, 0, 0, 0>": _NOT_LEAN + " (the two-pass path is lean)"
       for T in ("float", "double")},
}


def _defers(name):
    """A wave BP entry built with DEFER = true (the entries ssf_cases plans too)."""
    fam, args = name[len("qdec::"):].split("<")[0], name.split("<")[-1].rstrip(">").split(", ")
    at = {"bp_wave_kernel": 5, "bp_ms_wave_kernel": 4, "bp_ms_cmp_kernel": 4}.get(fam)
    return at is not None and args[at] == "true"


def ledger_gaps(names, reached):
    """Names outside the first ledger neither planned by a case nor listed as unreachable."""
    return [n for n in names if not in_ledger(n) and n not in reached and n not in UNREACHED]


def _reached(planned, without=None):
    return {n for _, ns in planned.values() if without is None or without not in ns for n in ns if n}


def test_ledger_of_the_remaining_instantiations(lib, planned, planned_mixed):
    """Every built entry outside the first ledger is planned by a case of
    bp_cases or ssf_cases (each of which a GPU module launches and compares with
    the oracle) or stands in UNREACHED; nothing in UNREACHED is planned; with the
    first ledger no built entry is outside both; and the check notices a missing
    case: without the cases of one entry the ledger reports exactly that name."""
    names = kernel_table_names(lib)
    reached = _reached(planned)
    assert reached <= set(names)
    assert not (set(UNREACHED) - set(names)), "UNREACHED names an entry the library does not build"
    assert not any(in_ledger(n) for n in UNREACHED)
    assert not (set(UNREACHED) & (reached | planned_mixed))
    assert ledger_gaps(names, reached | planned_mixed) == []
    # the two ledgers split the tables: each name belongs to exactly one, and in it
    # is either reached or listed with a reason
    assert not (set(UNREACHED) & set(mixed.UNREACHED))
    for n in names:
        book = mixed.UNREACHED if in_ledger(n) else UNREACHED
        assert (n in reached | planned_mixed) != (n in book), n
    # bp_cases alone plans every workgroup entry, every triage entry and every DEFER = false wave entry
    own = [n for n in names if not in_ledger(n) and not _defers(n)]
    assert len(own) > 80 and ledger_gaps(own, reached) == []
    for victim in ("qdec::bp_block_kernel<float, 0, true, 0, 0>", "qdec::bp_block_kernel<double, 1, false, 16, 8>",
                   "qdec::bp_ms_wave_kernel<double, 2, 4, 7, false, false, 2, 0>",
                   "qdec::bp_ms_wave_kernel<double, 2, 4, 7, true, true, 2, 3>",
                   "qdec::bp_ms_cmp_kernel<float, 4, 9, 8, false, 0, 0, 0>", "qdec::ms_triage_kernel<4, 9, true>",
                   "qdec::bp_wave_kernel<float, 0, 2, 6, 8, false>"):
        assert ledger_gaps(names, _reached(planned, victim) | planned_mixed) == [victim]


@pytest.mark.parametrize("group", sorted(bc.GROUPS))
def test_ledger_misses_every_group(lib, planned, planned_mixed, group):
    """Without the cases of one group the ledger has gaps."""
    ids = {c["id"] for p in bc.GROUPS[group][0] for c in bc.group_cases(group, p)}
    fewer = {n for cid, (_, ns) in planned.items() if cid not in ids for n in ns if n}
    assert ledger_gaps(kernel_table_names(lib), fewer | planned_mixed)


def test_shape_498_is_never_lean_with_ssf(lib):
    """What UNREACHED claims: on the (4, 9, 8) graph, with SSF, under every SSF
    kernel choice, fused or not, compact or not, lean or full outputs, byte or
    packed rows, 40 or 128 generators, either precision and default or raised
    wave occupancy, the min-sum plan is the non-lean one-pass deferring kernel."""
    graphs = HostGraphs(lib)
    try:
        for n_gen in (40, 128):
            for precision, want, ssf, fuse, compact, packed, occ in itertools.product(
                    ("f32", "f64"), (sc.LEAN_WANT, sc.SSF_WANT), ("auto", "scan", "scan_gather", "scan_nosplit"),
                    (0, 1), (0, 1), (False, True), (0, 12)):
                c = bc._case("wave", "w498", n_gen=n_gen, max_lc=9, precision=precision, want=want, packed=packed,
                             occ=occ, options={"ssf": ssf, "ssf_fuse": fuse, "compact": compact})
                plan, names = plan_entries(lib, graphs.get(c), c)
                assert not plan["two_pass"] and plan["q_rpar"] == 0 and plan["fin"] in (6, 7), (c["id"], plan)
                assert names[0] == f"qdec::bp_ms_wave_kernel<{sc.TNAME[precision]}, 4, 9, 8, true, false, 0, 0>"
                assert names[0] not in UNREACHED and names[2] == ""
    finally:
        graphs.close()


def test_gpu_module_runs_every_group():
    """The ledger counts the cases of bp_cases.GROUPS; the GPU module has one
    test function per group, parametrised by the group's own parameters, so
    every case counted is launched there."""
    import test_gpu_bp_ledger as gpu
    assert sorted(gpu.GROUP_OF_TEST.values()) == sorted(bc.GROUPS)
    for fn_name, group in gpu.GROUP_OF_TEST.items():
        marks = [m for m in getattr(gpu, fn_name).pytestmark if m.name == "parametrize"]
        assert len(marks) == 1 and [p.values[0] for p in marks[0].args[1]] == bc.GROUPS[group][0], fn_name
    assert gpu.pytestmark.name == "gpu"


def test_cases_are_not_vacuous(oracle_lib):
    """On the oracle alone, every case (bp_cases.check_conditions): converged and
    unconverged shots, at least three iteration counts, and behind a DEFER build
    a queued shot and an SSF step; the wave batches hold 65 and 257 shots, the
    workgroup cases a 5-shot window and the whole pool."""
    seen = set()
    for c in bc.all_cases():
        assert c["B"] in (bc.WAVE_B if c["kind"] == "wave" else (5, bc.POOL, bc.MANY[c["path"][2] or 3][0]))
        key = bc.oracle_key(dict(c, want=()))
        if key in seen:
            continue
        seen.add(key)
        bc.check_conditions(c, bc.oracle_decode(oracle_lib, dict(c, want=sc.SSF_WANT)))
