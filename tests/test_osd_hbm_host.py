"""The OSD placements' host side (qd_osd_kernel_info_placed, the slot layout of
osd_hbm_kernel in csrc/qdec_osd_hbm.hip) on host-only graphs through the built
library, and the Python surface of the new mode.  No GPU."""
import ctypes as C
import zlib

import numpy as np
import pytest

from conftest import REPO  # noqa: F401  (puts the repository on sys.path)
from test_osd_shapes import TABLE, _rows, graph

ONCHIP, HBM, AUTO = 0, 1, 2
PAST = "blk_past_limit"


def wide_graph():
    """3 x 65,600: past the 16-bit indices of the on-chip kernels."""
    from exp_ldpc_amd.codes import make_check_matrix
    from exp_ldpc_amd.decoder import as_csr01
    return as_csr01(make_check_matrix(_rows(3, 65600, zlib.crc32(b"wide_3x65600")), 65600))


def slot_bytes(m, n):
    """The slot of one workgroup, restated: rows [m][W] u64, sort keys u64 and
    column indices u32 padded to a power of two >= max(n, 64), pos u32 [n], piv
    u32 [m], isp and out u8 [n]; every region rounded up to 16 B, the slot to
    256 B."""
    ns = 64
    while ns < n:
        ns *= 2
    W = (n + 1 + 63) // 64
    regions = [8 * m * W, 8 * ns, 4 * ns, 4 * n, 4 * max(m, 1), n, n]
    return (sum((r + 15) // 16 * 16 for r in regions) + 255) // 256 * 256


class HostGraph:
    def __init__(self, H):
        from exp_ldpc_amd import _abi
        self.lib = _abi.load()
        rp = np.ascontiguousarray(H.indptr, dtype=np.int32)
        ci = np.ascontiguousarray(H.indices, dtype=np.int32)
        self.h = C.c_void_p()
        _abi.check(self.lib.qd_graph_create_host(H.shape[0], H.shape[1], _abi.ptr(rp), _abi.ptr(ci), H.shape[1], 1,
                                                 C.byref(self.h)), "qd_graph_create_host")

    def placed(self, placement):
        out = np.full(4, -7, np.int64)
        rc = self.lib.qd_osd_kernel_info_placed(self.h, placement, out.ctypes.data_as(C.c_void_p))
        return rc, tuple(int(v) for v in out)

    def plain(self):
        out = np.zeros(3, np.int32)
        rc = self.lib.qd_osd_kernel_info(self.h, out.ctypes.data_as(C.c_void_p))
        return rc, tuple(int(v) for v in out)

    def close(self):
        self.lib.qd_graph_destroy(self.h)


def test_kernel_info_placed_on_every_table_row():
    for row in TABLE:
        H = graph(row.name)
        g = HostGraph(H)
        try:
            rc0, (rs, w, lds) = g.plain()
            rc, info = g.placed(ONCHIP)
            # ONCHIP: qd_osd_kernel_info's answer with the kind in front
            assert rc == rc0 and info == ((0 if rs else 1, rs, w, lds) if rc0 else (0, 0, 0, 0)), row.name
            if row.name == PAST:
                assert rc == 0
            want_hbm = (2, 0, (row.n + 1 + 63) // 64, slot_bytes(row.m, row.n))
            rc_a, info_a = g.placed(AUTO)
            assert rc_a == 1 and info_a == (want_hbm if row.name == PAST else info), row.name
            rc_h, info_h = g.placed(HBM)
            assert rc_h == 1 and info_h == want_hbm, row.name
            # an unknown placement is refused, whatever the graph
            for bad in (-1, 3, 17):
                assert g.placed(bad) == (-44, (0, 0, 0, 0)), (row.name, bad)
        finally:
            g.close()


def test_wide_graph_goes_to_hbm_under_auto():
    H = wide_graph()
    assert H.shape == (3, 65600)
    g = HostGraph(H)
    try:
        assert g.plain()[0] == 0 and g.placed(ONCHIP) == (0, (0, 0, 0, 0))
        want = (1, (2, 0, 1026, slot_bytes(3, 65600)))
        assert g.placed(AUTO) == want and g.placed(HBM) == want
        # 131,072 sort slots of 12 B are most of the slot
        assert 12 * 131072 < want[1][3] < 12 * 131072 + 8 * 3 * 1026 + 10 * 65600 + 1024
    finally:
        g.close()


def test_python_surface():
    from exp_ldpc_amd import experiment
    from exp_ldpc_amd.decoder import Decoder, osd_kernel_info, osd_rows_placement
    assert "bposd_detector" in experiment.DECODER_MODES
    assert [osd_rows_placement(r) for r in ("onchip", "hbm", "auto")] == [ONCHIP, HBM, AUTO]
    with pytest.raises(ValueError):
        osd_rows_placement("host")  # the host stage is a pipeline choice, not a kernel placement
    for name in ("set_osd_slots", "osd_hbm_info"):
        assert callable(getattr(Decoder, name))
    g = HostGraph(graph(PAST))
    try:
        assert osd_kernel_info(g.h) is None and osd_kernel_info(g.h, "onchip") is None
        assert osd_kernel_info(g.h, "auto") == (2, 0, 64, slot_bytes(188, 4095))
        with pytest.raises(ValueError):
            osd_kernel_info(g.h, "lds")
    finally:
        g.close()


def test_bad_osd_rows_is_refused_before_anything_is_built(code225):
    from exp_ldpc_amd.dem import storage_experiment_dem
    from exp_ldpc_amd.experiment import BatchPipeline, DemPipeline
    opts = {"max_iter": 30, "bp_method": "ms", "ms_scaling_factor": 0, "osd_method": "osd_cs", "osd_order": 7}
    for mode in ("bposd", "bposd_detector"):
        with pytest.raises(ValueError, match="osd_rows"):
            BatchPipeline(code225, 1, mode, opts, (0.01, 0.01), osd_rows="lds")
    text = storage_experiment_dem(code225.checks.z, np.asarray(code225.logicals.z) % 2, 1, 0.01, 0.01)
    with pytest.raises(ValueError, match="osd_rows"):
        DemPipeline(text, opts, osd=True, osd_rows="device")
