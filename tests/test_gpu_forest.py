"""Every BP kernel family against exact marginals on forests (the cases of
tests/forest_cases.py, the model of tests/forest_model.py): not "kernel ==
oracle" as the two ledgers, but "kernel == belief propagation".  What was
launched is what the plan named, the plan's entries are the ones the case names,
and the outputs are the model's: x, iterations and status exactly, LLRs within
forest_cases.gpu_tol where the exact belief is finite and by sign where it is
+-inf.  tests/test_forest_host.py checks on the CPU that no case can pass
vacuously and that no belief is close enough to zero for rounding to decide a
bit."""
import numpy as np
import pytest

import forest_cases as fc
import ssf_cases as sc

pytestmark = pytest.mark.gpu


def _run(cases):
    """Decode the cases (one Decoder per graph, method and precision) and
    compare each with the model; the model's outputs are computed once per
    graph (forest_cases.bundle) and read-only."""
    from exp_ldpc_amd.decoder import Decoder, pack_rows
    decoders = {}
    try:
        for c in cases:
            syn, ref = fc.case_shots(c)
            H, probs, L = sc.graph(c["graph"])
            dkey = (c["graph"], c["method"], c["precision"])
            if dkey not in decoders:
                decoders[dkey] = Decoder(H, probs, method=c["method"], precision=c["precision"], logicals=L)
            dec = decoders[dkey]
            opts, present = sc.plan_request(c)
            for name, value in opts.items():
                dec.set_option(name, value)
            dec.set_wave_occupancy(c["occ"])
            dec.max_iter, dec.ms_scaling, dec.ssf_max_steps = c["max_iter"], c["scaling"], c["steps"]
            got = dec.decode(pack_rows(syn) if c["packed"] else syn, want=c["want"], packed=c["packed"])
            plan_kw = dict(present=present, packed=c["packed"])
            names = dec.last_kernels()
            assert names == dec.planned_kernels(c["B"], **plan_kw), (c["id"], names)
            assert dec.planned_entries(c["B"], **plan_kw) == (c["bp"], c["fin"], c["pre"]), c["id"]
            dev = fc.compare(c, got, ref, fc.gpu_tol(c["method"], c["precision"]))
            print(c["id"], "LLR deviation (relative, absolute):", dev)
    finally:
        for dec in decoders.values():
            dec.close()


# One test function per group of forest_cases.GROUPS, parametrised by the group's
# own parameters (tests/test_forest_host.py checks that every group has one).
GROUP_OF_TEST = {}


def _group_test(name):
    def deco(fn):
        GROUP_OF_TEST[fn.__name__] = name
        return pytest.mark.parametrize("param", fc.group_params(name))(fn)
    return deco


@_group_test("wave")
def test_wave_kernels_on_forests(gpu_available, param):
    """One wave shape, f32 and f64, 65 and 257 shots: bp_wave_kernel,
    bp_ms_wave_kernel with all outputs and lean, ms_triage_kernel +
    bp_ms_cmp_kernel from byte and from packed rows."""
    _run(fc.group_cases_of("wave", param))


@_group_test("block")
def test_workgroup_kernel_on_forests(gpu_available, param):
    """bp_block_kernel with its state in LDS (unrolled and generic body) and
    with the messages in HBM; both methods and precisions; 5 and 130 shots, and
    2600 on the generic graph."""
    _run(fc.group_cases_of("block", param))


@_group_test("block_hbm_state")
def test_workgroup_kernel_state_in_hbm_on_forests(gpu_available, param):
    """bp_block_kernel with messages and shot state in HBM, 5 shots, both
    methods and precisions."""
    _run(fc.group_cases_of("block_hbm_state", param))


@_group_test("group")
def test_slot_group_kernel_on_forests(gpu_available, param):
    """bp_group_kernel's (8, 4) and (16, 8) cells, both methods and precisions."""
    _run(fc.group_cases_of("group", param))


@_group_test("lds")
def test_lds_resident_kernels_on_forests(gpu_available, param):
    """bp_ms_lds_kernel<4> and bp_ms_lds64_kernel<4, 0>: x, iterations, status."""
    _run(fc.group_cases_of("lds", param))
