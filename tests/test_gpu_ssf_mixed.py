"""GPU parity of the cases of tests/ssf_cases.py against the CPU oracle: SSF on
flip sets whose generators differ in weight, local-check count and score table
(every wave shape, every SSF kernel, fused and queued, lean and full outputs,
the step bound), wave BP into the workgroup SSF kernels, workgroup graphs with
mixed generators, and the instantiations of the LDS-resident and slot-group BP
kernels no other test launches.  Every output is bit-exact (product-sum and
min-sum LLRs by test_gpu_parity._cmp_llr), what was launched is what the plan
named, and it is the instantiation the case expects.  Each case first checks on
the oracle's output that it cannot pass vacuously (ssf_cases.check_*)."""
import numpy as np
import pytest

import ssf_cases as sc

pytestmark = pytest.mark.gpu

_ORACLE = {}


def _oracle(oracle_lib, case):
    """The oracle's outputs of a case, computed once per distinct decode (the
    kernel options of a case do not change what it computes) and checked for
    the conditions that keep the case from passing vacuously."""
    key = (case["graph"], case["n_gen"], case["max_lc"], case["method"], case["precision"], case["max_iter"],
           case["steps"], case["scaling"], case["B"], case["offset"], case["p"], case["ssf"], "llr" in case["want"])
    if key not in _ORACLE:
        want = tuple(sorted(set(sc.SSF_WANT if case["ssf"] else sc.BP_WANT) | set(case["want"])))
        ref = sc.oracle_decode(oracle_lib, dict(case, want=want))
        if case["ssf"]:
            bp = sc.oracle_decode(oracle_lib, dict(case, ssf=False, want=sc.BP_WANT))
            free = _oracle(oracle_lib, dict(case, steps=0)) if case["steps"] else None
            sc.check_ssf_conditions(case, ref, sc.flip_sets(case["graph"], case["n_gen"], case["max_lc"]), bp, free)
        else:
            sc.check_bp_conditions(case, ref)
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _ORACLE[key] = ref
    return _ORACLE[key]


def _run(oracle_lib, cases):
    """Decode the cases (one Decoder per graph, flip sets, method and
    precision) and compare each with the oracle."""
    from exp_ldpc_amd.decoder import Decoder, pack_rows
    from test_gpu_parity import _cmp_llr
    decoders = {}
    for c in cases:
        ref = _oracle(oracle_lib, c)
        H, probs, L = sc.graph(c["graph"])
        dkey = (c["graph"], c["n_gen"], c["max_lc"], c["method"], c["precision"], c["ssf"])
        if dkey not in decoders:
            gens = sc.flip_sets(c["graph"], c["n_gen"], c["max_lc"]) if c["ssf"] else None
            decoders[dkey] = Decoder(H, probs, method=c["method"], precision=c["precision"], flip_sets=gens,
                                     logicals=L if c["ssf"] else None)
        dec = decoders[dkey]
        opts, present = sc.plan_request(c)
        for name, value in opts.items():
            dec.set_option(name, value)
        dec.set_wave_occupancy(c["occ"])
        dec.max_iter, dec.ms_scaling, dec.ssf_max_steps = c["max_iter"], c["scaling"], c["steps"]
        syn, rd = sc.case_shots(c)
        rd = rd if "fail" in c["want"] else None
        if c["packed"]:
            syn, rd = pack_rows(syn), None if rd is None else pack_rows(rd)
        got = dec.decode(syn, readout=rd, want=c["want"], packed=c["packed"])
        names = dec.last_kernels()
        assert names == dec.planned_kernels(c["B"], present=present, packed=c["packed"]), (c["id"], names)
        assert names == (c["bp"], c["fin"], c["pre"]), (c["id"], names)
        for k in c["want"]:
            if k == "llr":
                _cmp_llr(got[k], ref[k], c["method"], c["precision"])
            else:
                assert np.array_equal(got[k], ref[k]), (c["id"], k, int((got[k] != ref[k]).sum()))
    for dec in decoders.values():
        dec.close()


# One test function per group of ssf_cases.GROUPS, parametrised by the group's
# own parameters (tests/test_ssf_mixed_host.py checks that every group has one).
GROUP_OF_TEST = {}


def _group_test(name):
    def deco(fn):
        GROUP_OF_TEST[fn.__name__] = name
        return pytest.mark.parametrize("param", sc.group_params(name))(fn)
    return deco


@_group_test("wave_ssf")
def test_wave_ssf_mixed_flip_sets(gpu_available, oracle_lib, param):
    """One wave graph, flip sets and precision: lean and full outputs x the
    table-driven and the three scanning SSF kernels x fused into the compact BP
    kernel or behind the queue x compact or one-pass BP x unbounded or 2 steps
    (40 decodes of 257 shots: four triage tiles and one shot)."""
    cases = sc.group_cases("wave_ssf", param)
    assert len(cases) == 40
    _run(oracle_lib, cases)


@_group_test("wave_extra")
def test_wave_ssf_packed_product_sum_occupancy(gpu_available, oracle_lib, param):
    """Per wave graph: bit-packed input rows, product-sum into the table kernel
    (bp_wave_kernel's DEFER build, f32 and f64), and where the graph has two
    3-edge rounds the three-waves-per-SIMD f64 build, fused and not."""
    _run(oracle_lib, sc.group_cases("wave_extra", param))


@_group_test("queue_ssf")
def test_wave_bp_into_workgroup_ssf(gpu_available, oracle_lib, param):
    """Wave BP kernels filling the byte queue of a workgroup SSF kernel: shape
    (4, 9, 8) with 40 and 128 generators, (2, 4, 8) with 150 and 300; f32 and
    f64, the incremental and the re-scanning kernel, all six outputs; and
    product-sum on (4, 9, 8)."""
    _run(oracle_lib, sc.group_cases("queue_ssf", param))


@_group_test("block_ssf")
def test_workgroup_graphs_mixed_flip_sets(gpu_available, oracle_lib, param):
    """200 mixed generators on ragged 300 x 700 graphs: bp_block_kernel into
    ssf_inc_block_kernel and into ssf_block_kernel, the slot-group kernel, and
    the LDS-resident kernels (f32 and f64) on the graph within their degrees."""
    _run(oracle_lib, sc.group_cases("block_ssf", param))


@_group_test("lds_bp")
def test_lds_kernel_columns_per_thread(gpu_available, oracle_lib, param):
    """bp_ms_lds_kernel<8 / 12 / 16> (and <10>, <8> just past a round boundary):
    odd m, a ragged last round, row degree <= 8, column degrees 1..4,
    per-column priors; 20 iterations with and without a constant scaling, and one
    iteration; past 10240 columns f64 falls through to the slot-group kernel."""
    _run(oracle_lib, sc.group_cases("lds_bp", param))


@_group_test("lds64_bp")
def test_lds64_kernel_cells(gpu_available, oracle_lib, param):
    """Every bp_ms_lds64_kernel<VPT, D3R> beyond <4, 0>, by name."""
    _run(oracle_lib, sc.group_cases("lds64_bp", param))


@_group_test("group_bp")
def test_group_kernel_degree_cells(gpu_available, oracle_lib, param):
    """bp_group_kernel<T, METHOD, DR, DC> on a graph of each degree cell:
    min-sum and product-sum, f32 and f64, 700 shots (slots refilled mid-flight)
    and 5 (idle slots from the start); x, iterations, status and LLRs."""
    _run(oracle_lib, sc.group_cases("group_bp", param))
