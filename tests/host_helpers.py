"""Helpers shared by the CPU-side tests: host-only graphs (qd_graph_create_host),
copies of the table-driven SSF kernel's tables with a host emulation of its step
rule, and the plan's kernel names.  No GPU."""
import numpy as np
import scipy.sparse as sp


def _host_graph(lib, H, n_data=None, gens=None, lz=None, probs=None):
    import ctypes as C

    from exp_ldpc_amd import _abi
    H = sp.csr_matrix(H)
    H.sort_indices()
    rp = np.ascontiguousarray(H.indptr, np.int32)
    ci = np.ascontiguousarray(H.indices, np.int32)
    h = C.c_void_p()
    nd = n_data or H.shape[1]
    _abi.check(lib.qd_graph_create_host(H.shape[0], H.shape[1], _abi.ptr(rp), _abi.ptr(ci), nd, 1, C.byref(h)),
               "qd_graph_create_host")
    if gens is not None:
        G = sp.csr_matrix(gens)
        G.sort_indices()
        gp, gi = np.ascontiguousarray(G.indptr, np.int32), np.ascontiguousarray(G.indices, np.int32)
        _abi.check(lib.qd_graph_set_flipsets(h, G.shape[0], _abi.ptr(gp), _abi.ptr(gi)), "flipsets")
    if lz is not None:
        L = sp.csr_matrix(lz)
        L.sort_indices()
        lp, li = np.ascontiguousarray(L.indptr, np.int32), np.ascontiguousarray(L.indices, np.int32)
        _abi.check(lib.qd_graph_set_logicals_csr(h, L.shape[0], _abi.ptr(lp), _abi.ptr(li)), "logicals")
    if probs is not None:
        pr = np.ascontiguousarray(np.broadcast_to(np.asarray(probs, np.float64), (H.shape[1],)))
        _abi.check(lib.qd_graph_set_priors(h, _abi.ptr(pr)), "priors")
    d, nb = C.c_uint64(0), C.c_int64(0)
    _abi.check(lib.qd_graph_table_digest(h, C.byref(d), C.byref(nb)), "digest")
    return h, d.value, nb.value


def _lut_ssf_emulate(tab, H, gens, x, resid, max_steps=0):
    """The table-driven SSF kernel's steps (ssf_lut_kernel, qdec_bp.hip) run on
    the host over the library's own tables: local syndromes from the toggle rows
    of the violated checks, then per step the table entry of every generator,
    the max of (rank, -g), the winner's subset applied (qubits x, toggle rows of
    the checks it flips).  Returns (x, steps)."""
    lut, off, lcw, tog, gp = tab
    x = x.copy()
    ng = gens.shape[0]
    gq = [gens.indices[gens.indptr[g]:gens.indptr[g + 1]] for g in range(ng)]
    sl = np.zeros(ng, np.int64)
    for c in np.flatnonzero(resid):
        for g in range(ng):
            sl[g] ^= (int(tog[c, g & 63]) >> (16 * (g >> 6))) & 0xffff
    sw = int(resid.sum())
    steps = 0
    while sw > 0 and (max_steps <= 0 or steps < max_steps):
        best, bg = 0, -1
        for g in range(ng):
            e = int(lut[off[g] + sl[g]])
            if e >> 24:
                key = ((e >> 24) << 15) | ((127 - g) << 8) | (e & 0xff)
                if key > best:
                    best, bg = key, g
        if bg < 0:
            break
        e = int(lut[off[bg] + sl[bg]])
        t, fm = e & 0xff, (e >> 8) & 0xffff
        slg = int(sl[bg])
        sw -= bin(slg).count("1") - bin(slg ^ fm).count("1")
        steps += 1
        for b in range(16):
            if (fm >> b) & 1:
                c = (int(lcw[b // 4, bg]) >> (8 * (b % 4))) & 0xff
                for g in range(ng):
                    sl[g] ^= (int(tog[c, g & 63]) >> (16 * (g >> 6))) & 0xffff
        for k in range(len(gq[bg])):
            if (t >> k) & 1:
                x[gq[bg][k]] ^= 1
    return x, steps


def _lut_tables(lib, h):
    import ctypes as C

    from exp_ldpc_amd import _abi
    has, nb = C.c_int32(0), C.c_int64(0)
    _abi.check(lib.qd_graph_ssf_tables(h, C.byref(has), C.byref(nb)), "ssf_tables")
    if not has.value:
        return None
    gp, mp = C.c_int32(0), C.c_int32(0)
    _abi.check(lib.qd_graph_ssf_tables_copy(h, None, None, None, None, C.byref(gp), C.byref(mp)), "copy")
    lut = np.zeros(nb.value // 4, np.uint32)
    off = np.zeros(gp.value, np.uint32)
    lcw = np.zeros((4, gp.value), np.uint32)
    tog = np.zeros((mp.value + 1, 64), np.uint32)
    _abi.check(lib.qd_graph_ssf_tables_copy(h, _abi.ptr(lut), _abi.ptr(off), _abi.ptr(lcw), _abi.ptr(tog), None,
                                            None), "copy")
    return lut, off, lcw, tog, gp.value


def _plan_names(lib, h, prm, B, present):
    """(bp, ssf, pre) of qd_graph_plan_names."""
    import ctypes as C

    from exp_ldpc_amd import _abi
    bufs = [C.create_string_buffer(512) for _ in range(3)]
    _abi.check(lib.qd_graph_plan_names(h, C.byref(prm), B, present, bufs[0], 512, bufs[1], 512, bufs[2], 512),
               "qd_graph_plan_names")
    return [b.value.decode() for b in bufs]
