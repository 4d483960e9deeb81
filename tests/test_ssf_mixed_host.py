"""CPU side of the mixed-flip-set cases (tests/ssf_cases.py): the table-driven SSF
kernel's tables for generators of different weights and local patterns, emulated
on the host against the oracle; the launch plan of every case; and a ledger that
holds every instantiation of the SSF, fused-SSF, LDS-resident, slot-group and
deferring product-sum families against the cases that launch it on the GPU
(tests/test_gpu_ssf_mixed.py).  No GPU."""
import ctypes as C
import itertools

import numpy as np
import pytest

import ssf_cases as sc
from host_helpers import _host_graph, _lut_ssf_emulate, _lut_tables

PRESENT = {"syn": 1, "base": 2, "readout": 4, "x": 8, "corr": 16, "llr": 32, "fail": 64}
ALIGNED = 128


def kernel_table_names(lib):
    n = lib.qd_kernel_table_names(None, 0)
    assert n > 0
    buf = C.create_string_buffer(int(n) + 1)
    assert lib.qd_kernel_table_names(buf, n + 1) == n
    text = buf.value.decode()
    assert text.endswith("\n")
    return text[:-1].split("\n")


class HostGraphs:
    """One host-only graph per case graph; flip sets are replaced per case."""

    def __init__(self, lib):
        self.lib, self.h, self.gens = lib, {}, {}

    def get(self, case):
        key = case["graph"]
        if key not in self.h:
            H, probs, L = sc.graph(key)
            self.h[key] = _host_graph(self.lib, H, lz=L, probs=probs)[0]
        want = (case["n_gen"], case["max_lc"]) if case["ssf"] else None
        if want and self.gens.get(key) != want:
            from exp_ldpc_amd import _abi
            G = sc.flip_sets(key, *want)
            gp, gi = np.ascontiguousarray(G.indptr, np.int32), np.ascontiguousarray(G.indices, np.int32)
            _abi.check(self.lib.qd_graph_set_flipsets(self.h[key], G.shape[0], _abi.ptr(gp), _abi.ptr(gi)), "flipsets")
            self.gens[key] = want
        return self.h[key]

    def close(self):
        for h in self.h.values():
            self.lib.qd_graph_destroy(h)


def plan_case(lib, h, case):
    """(plan fields, (bp, ssf, pre) names) of a case on host graph h."""
    from exp_ldpc_amd import _abi
    from exp_ldpc_amd.decoder import OPTIONS, SSF_KERNELS, parse_bp_method, parse_precision
    opts, present = sc.plan_request(case)
    for name, value in opts.items():
        _abi.check(lib.qd_graph_set_option(h, OPTIONS[name], SSF_KERNELS.get(value, value)), name)
    _abi.check(lib.qd_graph_set_wave_occupancy(h, case["occ"]), "occupancy")
    prm = _abi.QdParams(case["max_iter"], parse_bp_method(case["method"]), parse_precision(case["precision"]),
                        int(case["ssf"]), case["steps"], _abi.QD_INPUT_PACKED if case["packed"] else 0,
                        case["scaling"])
    mask = sum(PRESENT[k] for k in present) | ALIGNED
    out = np.zeros(8, np.int32)
    _abi.check(lib.qd_graph_plan(h, C.byref(prm), case["B"], mask, _abi.ptr(out)), "qd_graph_plan")
    bufs = [C.create_string_buffer(512) for _ in range(3)]
    _abi.check(lib.qd_graph_plan_names(h, C.byref(prm), case["B"], mask, bufs[0], 512, bufs[1], 512, bufs[2], 512),
               "qd_graph_plan_names")
    plan = dict(zip(("bp", "fin", "two_pass", "expand_packed", "fuse", "q_rpar", "placement", "buffers"),
                    (int(v) for v in out)))
    return plan, tuple(b.value.decode() for b in bufs)


@pytest.fixture(scope="module")
def lib():
    from exp_ldpc_amd import _abi
    return _abi.load()


@pytest.fixture(scope="module")
def planned(lib):
    """{case id: (plan, names)} of every case."""
    graphs = HostGraphs(lib)
    try:
        cases = sorted(sc.all_cases(), key=lambda c: (c["graph"], c["n_gen"], c["max_lc"]))
        return {c["id"]: plan_case(lib, graphs.get(c), c) for c in cases}
    finally:
        graphs.close()


def test_kernel_table_names_lists_the_tables(lib):
    """qd_kernel_table_names without a device: every entry once, spelled as the
    plan spells it, the wave families before the workgroup ones; a short buffer
    gets a cut, terminated copy and the full length."""
    names = kernel_table_names(lib)
    assert len(set(names)) == len(names) and all(n.startswith("qdec::") for n in names)
    fams = [n.split("<")[0][6:] for n in names]
    assert [f for i, f in enumerate(fams) if i == 0 or fams[i - 1] != f] == [
        "bp_wave_kernel", "bp_ms_wave_kernel", "bp_ms_cmp_kernel", "ms_triage_kernel", "ssf_wave_kernel",
        "ssf_lut_kernel", "bp_block_kernel", "bp_group_kernel", "bp_ms_lds_kernel", "bp_ms_lds64_kernel",
        "ssf_inc_block_kernel", "ssf_block_kernel"]
    assert "qdec::bp_ms_lds_kernel<16>" in names and "qdec::ssf_lut_kernel<2, 6, 2, true>" in names
    small = C.create_string_buffer(b"\xff" * 16, 16)
    assert lib.qd_kernel_table_names(small, 16) == sum(len(n) + 1 for n in names)
    assert small.raw == ("\n".join(names) + "\n")[:15].encode() + b"\0"


def test_every_case_plans_what_it_expects(planned):
    """Each case names its instantiations in full (ssf_cases); the plan of the
    same request on a host-only graph gives exactly them."""
    cases = sc.all_cases()
    assert len({c["id"] for c in cases}) == len(cases)
    for c in cases:
        plan, (bp, fin, pre) = planned[c["id"]]
        assert (bp, fin, pre) == (c["bp"], c["fin"], c["pre"]), (c["id"], plan, bp, fin, pre)
        if c["path"]:  # stages that record no name: the plan's paths
            assert (plan["bp"], plan["fin"]) == c["path"], (c["id"], plan)


def test_gpu_module_runs_every_group():
    """The ledger counts the cases of ssf_cases.GROUPS; the GPU module has one
    test function per group, parametrised by the group's own parameters, so
    every case counted is launched there."""
    import test_gpu_ssf_mixed as gpu
    assert sorted(gpu.GROUP_OF_TEST.values()) == sorted(sc.GROUPS)
    for fn_name, group in gpu.GROUP_OF_TEST.items():
        marks = [m for m in getattr(gpu, fn_name).pytestmark if m.name == "parametrize"]
        assert len(marks) == 1 and [p.values[0] for p in marks[0].args[1]] == sc.GROUPS[group][0], fn_name
    assert gpu.pytestmark.name == "gpu"


def in_ledger(name):
    fam = name.split("<")[0][len("qdec::"):]
    if fam == "bp_ms_cmp_kernel":
        return not name.endswith(", 0>")   # FUSE != 0
    if fam == "bp_wave_kernel":
        return name.endswith(", true>")    # DEFER
    return fam in ("ssf_wave_kernel", "ssf_lut_kernel", "bp_ms_lds_kernel", "bp_ms_lds64_kernel", "bp_group_kernel")


# Built, but no input reaches the plan's branch (plan_decode_wave): a graph of
# shape (4, 9, 8) has m_pad = 256, beyond the u8 check ids (m_pad <= 255) of the
# wave SSF kernels' generator tables (g_lc8) and of the table kernels' toggle
# rows (s_tog), so its queue is never packed and its SSF is a workgroup kernel.
# test_shape_498_never_reaches_the_wave_ssf_kernels establishes it.
_NO_U8 = "shape (4, 9, 8) pads to 256 checks; the kernel's u8 check ids hold m_pad <= 255"
UNREACHED = {
    **{f"qdec::ssf_wave_kernel<{rg}, 9, 4>": _NO_U8 for rg in (1, 2)},
    **{f"qdec::ssf_lut_kernel<{rg}, 9, 4, {lean}>": _NO_U8 for rg in (1, 2) for lean in ("false", "true")},
    **{f"qdec::bp_ms_cmp_kernel<{T}, 4, 9, 8, true, 0, 0, {fuse}>": _NO_U8 + " (the fused SSF reads the same tables)"
       for T in ("float", "double") for fuse in (1, 2)},
}


def ledger_gaps(names, reached):
    """Ledger names neither planned by a case nor listed as unreachable."""
    return [n for n in names if in_ledger(n) and n not in reached and n not in UNREACHED]


def test_ledger_of_launched_instantiations(lib, planned):
    """Every instantiation of the ledger's families that the library builds is
    planned by a case of ssf_cases.all_cases (each of which the GPU module
    launches and compares with the oracle) or stands in UNREACHED; nothing in
    UNREACHED is planned; and the check notices a missing case: without the cases
    of one instantiation the ledger reports exactly that name."""
    names = kernel_table_names(lib)
    reached = {n for _, ns in planned.values() for n in ns if n}
    assert reached <= set(names)
    assert not (set(UNREACHED) - set(names)), "UNREACHED names an entry the library does not build"
    assert not (set(UNREACHED) & reached)
    assert ledger_gaps(names, reached) == []
    assert sum(map(in_ledger, names)) == len([n for n in reached if in_ledger(n)]) + len(UNREACHED)
    for victim in ("qdec::bp_ms_lds_kernel<12>", "qdec::ssf_lut_kernel<2, 6, 2, true>",
                   "qdec::bp_ms_cmp_kernel<double, 1, 2, 8, true, 0, 0, 2>", "qdec::bp_group_kernel<float, 0, 16, 4>"):
        fewer = {n for _, ns in planned.values() if victim not in ns for n in ns if n}
        assert ledger_gaps(names, fewer) == [victim]


def test_shape_498_never_reaches_the_wave_ssf_kernels(lib):
    """What UNREACHED claims: on the (4, 9, 8) graph (m_pad = 256, as for every
    graph of that shape) the library builds no lane tables for the table-driven
    kernel, and under every SSF kernel choice, fused or not, compact or not,
    lean or full outputs, 40 or 128 generators, either precision and either
    method, the plan keeps the byte queue (q_rpar = 0, no fused SSF) and a
    workgroup SSF kernel behind the non-lean deferring BP kernel."""
    from exp_ldpc_amd import _abi
    graphs = HostGraphs(lib)
    try:
        for n_gen in (40, 128):
            base = sc._case("w498", n_gen=n_gen, max_lc=9)
            h = graphs.get(base)
            m_pad = C.c_int32(0)
            _abi.check(lib.qd_graph_ms_state0_copy(h, _abi.QD_F64, None, None, C.byref(m_pad)), "state0")
            assert m_pad.value == 256
            has = C.c_int32(0)
            _abi.check(lib.qd_graph_ssf_tables(h, C.byref(has), None), "ssf tables")
            assert has.value != 1  # score tables at most (2), never the lane tables
            for method, precision, want, ssf, fuse, compact in itertools.product(
                    ("ms", "ps"), ("f32", "f64"), (sc.LEAN_WANT, sc.SSF_WANT),
                    ("auto", "scan", "scan_gather", "scan_nosplit"), (0, 1), (0, 1)):
                c = sc._case("w498", n_gen=n_gen, max_lc=9, method=method, precision=precision, want=want,
                             options={"ssf": ssf, "ssf_fuse": fuse, "compact": compact})
                plan, (bp, fin, pre) = plan_case(lib, h, c)
                assert plan["fin"] in (6, 7) and plan["fuse"] == 0 and plan["q_rpar"] == 0 and not plan["two_pass"], c
                T = sc.TNAME[precision]
                assert bp == (f"qdec::bp_ms_wave_kernel<{T}, 4, 9, 8, true, false, 0, 0>" if method == "ms" else
                              f"qdec::bp_wave_kernel<{T}, 0, 4, 9, 8, true>") and fin == "" and pre == "", (c, bp)
    finally:
        graphs.close()


def test_more_than_128_generators_take_the_workgroup_ssf(lib):
    """150 generators on the (2, 4, 8) graph: no packed queue (the plan's q_rpar
    and two_pass stay 0 although the request is lean), the incremental workgroup
    SSF kernel (QD_FIN_INC_BLOCK; the re-scanning one with ssf_inc = 0) and the
    non-lean deferring BP kernel."""
    graphs = HostGraphs(lib)
    try:
        for inc, fin_path in ((1, 6), (0, 7)):
            c = sc._case("w248", n_gen=150, max_lc=9, want=sc.LEAN_WANT, options={"ssf_inc": inc, "ssf_fuse": 1})
            plan, (bp, fin, pre) = plan_case(lib, graphs.get(c), c)
            assert (plan["fin"], plan["two_pass"], plan["q_rpar"], plan["fuse"]) == (fin_path, 0, 0, 0), plan
            assert bp == "qdec::bp_ms_wave_kernel<double, 2, 4, 8, true, false, 0, 0>" and fin == "" and pre == ""
    finally:
        graphs.close()


def test_block_ssf_placement_zero_needs_a_large_graph(lib, planned):
    """The workgroup SSF cases keep messages and shot state in LDS (placement 3).
    Placement 0 (shot state in HBM, ssf_block_kernel from the scratch tail) needs
    per-shot byte arrays beyond 64 KB of LDS (block_placement: n of about 6 * 10^4),
    which no graph of a few-second test reaches; test_gpu_large_codes' config-5
    spacetime graph (130,560 columns) covers it without SSF."""
    for c in sc.block_ssf_cases():
        assert planned[c["id"]][0]["placement"] == 3, c["id"]


@pytest.mark.parametrize("n_gen", sc.WAVE_NGEN)
@pytest.mark.parametrize("key", sc.WAVE_KEYS)
def test_mixed_tables_follow_the_spec(lib, oracle_lib, key, n_gen):
    """ssf_lut_tables on generators of different weights and local patterns:
    the graph qualifies, the generators spread over at least 8 score tables,
    every check carries at most 64 generators (so the scanning kernel keeps its
    inverse table), and the table kernel's step rule run on the host over the
    library's tables reproduces the oracle's SSF -- x and step counts, unbounded
    and cut at 2 steps -- on every BP-failed shot; the oracle's subset search
    and its incremental implementation agree."""
    H, probs, L = sc.graph(key)
    max_lc = sc.max_lc_of(n_gen)
    G = sc.flip_sets(key, n_gen, max_lc)
    w, nlc, per_check = sc.flip_set_stats(H, G)
    assert set(w) >= {1, 2, 3, 4, 8} and 1 <= nlc.min() and nlc.max() <= max_lc and len(set(nlc)) >= 4
    assert per_check <= 64
    h, _, _ = _host_graph(lib, H, gens=G, lz=L, probs=probs)
    try:
        tab = _lut_tables(lib, h)
        assert tab is not None
        lut, off = tab[0], tab[1]
        assert len(set(off[:n_gen].tolist())) >= 8
        assert lut.size * 4 + (tab[3].shape[0]) * 256 <= 96 * 1024 and not tab[3][-1].any()
        p, it = sc.RATES[key]
        base = sc._case(key, n_gen=n_gen, max_lc=max_lc, p=p, max_iter=it)
        syn, _ = sc.case_shots(base)
        bp = sc.oracle_decode(oracle_lib, dict(base, ssf=False, want=sc.BP_WANT))
        for steps in (0, 2):
            ref = sc.oracle_decode(oracle_lib, dict(base, steps=steps))
            brute = oracle_lib.decode(H, probs, syn, method="ms", precision="f64", max_iter=it, ssf=True, gens=G,
                                      ssf_max_steps=steps, want_llr=False, ssf_impl="brute")
            assert np.array_equal(brute["x"], ref["x"]) and np.array_equal(brute["ssf_steps"], ref["ssf_steps"])
            checked = 0
            for b in np.flatnonzero((bp["status"] & 1) == 0):
                resid = (syn[b] ^ (H @ bp["x"][b]) % 2).astype(np.uint8)
                x, n_steps = _lut_ssf_emulate(tab, H, G, bp["x"][b], resid, steps)
                assert np.array_equal(x, ref["x"][b]) and n_steps == ref["ssf_steps"][b], (steps, b)
                checked += 1
            assert checked >= 0.15 * base["B"]
        # the inputs tell a reader of s_off from one that ignores it: the same
        # emulation with every generator on the first table leaves the oracle
        blind = (tab[0], np.zeros_like(tab[1])) + tab[2:]

        def blind_differs(b):
            resid = (syn[b] ^ (H @ bp["x"][b]) % 2).astype(np.uint8)
            try:
                return not np.array_equal(_lut_ssf_emulate(blind, H, G, bp["x"][b], resid, 2)[0], ref["x"][b])
            except IndexError:  # the other table's entry flips a local check this generator does not have
                return True
        assert any(blind_differs(b) for b in np.flatnonzero((bp["status"] & 1) == 0))
    finally:
        lib.qd_graph_destroy(h)


def test_cases_are_not_vacuous(oracle_lib):
    """The conditions the GPU module asserts per case, on the oracle alone: both
    BP outcomes, enough SSF steps, repaired and unrepaired shots, many winning
    generators, shots cut at the step bound; BP-only cases with both outcomes
    and several iteration counts."""
    seen = set()
    for c in sc.all_cases():
        key = (c["graph"], c["n_gen"], c["max_lc"], c["method"], c["precision"], c["max_iter"], c["steps"],
               c["scaling"], c["B"], c["offset"], c["p"], c["ssf"])
        if key in seen:
            continue
        seen.add(key)
        ref = sc.oracle_decode(oracle_lib, dict(c, want=sc.SSF_WANT if c["ssf"] else sc.BP_WANT))
        if c["ssf"]:
            bp = sc.oracle_decode(oracle_lib, dict(c, ssf=False, want=sc.BP_WANT))
            free = sc.oracle_decode(oracle_lib, dict(c, steps=0, want=sc.SSF_WANT)) if c["steps"] else None
            sc.check_ssf_conditions(c, ref, sc.flip_sets(c["graph"], c["n_gen"], c["max_lc"]), bp, free)
        else:
            sc.check_bp_conditions(c, ref)
