"""GPU parity of the cases of tests/bp_cases.py against the CPU oracle: the
BP-only builds of the wave min-sum, compact and product-sum kernels on every wave
shape, and every cell of bp_block_kernel (unrolled and generic body, messages and
shot state in LDS or HBM, both methods and precisions, with and without the SSF
queue behind it).  What was launched is what the plan named, the plan's entries
are the ones the case names, and every output equals the oracle's: x, corr,
iterations, status, SSF steps and failure flags exactly, min-sum LLRs byte for
byte, product-sum LLRs by test_gpu_parity._cmp_llr.  tests/test_bp_ledger_host.py
checks on the oracle alone that no case can pass vacuously."""
import numpy as np
import pytest

import bp_cases as bc
import ssf_cases as sc

pytestmark = pytest.mark.gpu

_ORACLE = {}


def _oracle(oracle_lib, case):
    """The oracle's outputs of a case, computed once per distinct decode, checked
    for bp_cases.check_conditions, and read-only from then on."""
    key = bc.oracle_key(case)
    if key not in _ORACLE:
        ref = bc.oracle_decode(oracle_lib, case)
        bc.check_conditions(case, ref)
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
    try:
        for c in cases:
            ref = _oracle(oracle_lib, c)
            H, probs, L = sc.graph(c["graph"])
            dkey = (c["graph"], c["n_gen"], c["max_lc"], c["method"], c["precision"], c["ssf"])
            if dkey not in decoders:
                gens = sc.flip_sets(c["graph"], c["n_gen"], c["max_lc"]) if c["ssf"] else None
                decoders[dkey] = Decoder(H, probs, method=c["method"], precision=c["precision"], flip_sets=gens,
                                         logicals=L)
            dec = decoders[dkey]
            opts, present = bc.plan_request(c)
            for name, value in opts.items():
                dec.set_option(name, value)
            dec.set_wave_occupancy(c["occ"])
            dec.max_iter, dec.ms_scaling, dec.ssf_max_steps = c["max_iter"], c["scaling"], c["steps"]
            if c["kind"] == "block" and c["B"] > bc.POOL:  # more shots than one launch has workgroups
                import torch
                per_cu = bc.MANY[c["path"][2]][1]
                assert torch.cuda.get_device_properties(0).multi_processor_count * per_cu < c["B"], c["id"]
            inp = bc.case_inputs(c)
            syn, base, rd = inp["syn"], inp["base"], inp["readout"] if "readout" in present else None
            if c["packed"]:
                syn, rd = pack_rows(syn), None if rd is None else pack_rows(rd)
            got = dec.decode(syn, base=base, readout=rd, syn_flags=c["syn_flags"], want=c["want"], packed=c["packed"])
            plan_kw = dict(present=present, packed=c["packed"], syn_flags=c["syn_flags"])
            names = dec.last_kernels()
            assert names == dec.planned_kernels(c["B"], **plan_kw), (c["id"], names)
            assert dec.planned_entries(c["B"], **plan_kw) == (c["bp"], c["fin"], c["pre"]), c["id"]
            for k in c["want"]:
                if k == "llr" and c["method"] == "ms":
                    assert got[k].tobytes() == ref[k].astype(got[k].dtype).tobytes(), (c["id"], k)
                elif k == "llr":
                    _cmp_llr(got[k], ref[k], c["method"], c["precision"])
                else:
                    assert np.array_equal(got[k], ref[k]), (c["id"], k, int((got[k] != ref[k]).sum()))
    finally:
        for dec in decoders.values():
            dec.close()


# One test function per group of bp_cases.GROUPS, parametrised by the group's own
# parameters (tests/test_bp_ledger_host.py checks that every group has one).
GROUP_OF_TEST = {}


def _group_test(name):
    def deco(fn):
        GROUP_OF_TEST[fn.__name__] = name
        return pytest.mark.parametrize("param", bc.group_params(name))(fn)
    return deco


@_group_test("wave_bp")
def test_wave_bp_only_builds(gpu_available, oracle_lib, param):
    """One wave graph, f32 and f64, 65 and 257 shots, no SSF: min-sum with all
    six outputs, lean one-pass, lean compact behind the triage on byte and on
    packed rows, product-sum with x and LLRs; on the (2, 4, 7) graph with two
    3-edge rounds also the three-waves-per-SIMD f64 builds."""
    _run(oracle_lib, bc.group_cases("wave_bp", param))


@_group_test("block_bp")
def test_workgroup_kernel_cells(gpu_available, oracle_lib, param):
    """One workgroup graph (a body and a placement of bp_block_kernel) and BP
    method, f32 and f64: BP only with all six outputs, from the syndrome and (one
    graph per body) from base and readout, and BP into the incremental and the
    re-scanning workgroup SSF kernel; 5 shots, and where the shot state is in
    LDS 130 and a batch beyond one launch's workgroups (bp_cases.MANY)."""
    _run(oracle_lib, bc.group_cases("block_bp", param))
