"""The deblocking level search restated (include/av1mi.h: av1mi_params.deblock = 2): the candidate pool, the
first-minimum rule, and the probing of the oracle that gives every candidate's squared error - shared by
tests/test_deblock_search_host.py (CPU) and tests/test_deblock_search.py (GPU).  Plain numpy and the oracle, no GPU."""
import ctypes as C

import numpy as np

import edge_content

D = [-12, -8, -6, -4, -3, -2, -1, 0, 1, 2, 3, 4, 6, 8, 12, 16]


def pool(g, chroma):
    """the 16 candidate levels around the formula's level g"""
    return [min(max(g + d, 0 if chroma else 1), 63) for d in D]


def first_min(e):
    """index of the first minimum"""
    e = [int(x) for x in e]
    return e.index(min(e))


def formula_level(oracle, cfg, key):
    """the level deblock = 1 gives the frame kind (the oracle's restatement of libaom's pick-from-q rule)"""
    c = oracle.default_config(cfg.width, cfg.height, cfg.bit_depth, base_q_idx=cfg.base_q_idx, deblock=1)
    lv = (C.c_int * 4)()
    fn = oracle.lib().av1o_deblock_levels
    fn.argtypes = [C.POINTER(oracle.Config), C.c_int, C.POINTER(C.c_int)]
    fn(C.byref(c), 1 if key else 0, lv)
    assert lv[0] == lv[1] == lv[2] == lv[3]
    return int(lv[0])


def plane_sse(rec, src):
    return [int(((np.asarray(rec[p]).astype(np.int64) - np.asarray(src[p]).astype(np.int64)) ** 2).sum()) for p in range(3)]


def reference(oracle, case, frames):
    """The chunk as the rule prescribes it, from the oracle alone.  Per frame: 16 oracle runs without CDEF and restoration at explicit
    levels (Py[i], Py[i], Pc[i], Pc[i]) - their reconstruction is the deblocked frame, so numpy has E[plane][i] over the signalled
    size -, the rule, then one run with the case's tools at the chosen levels: the expected bytes, reconstruction and next reference.
    Returns (temporal units, reconstructions, levels [frame][4], E [frame][3][16], g per frame)."""
    keyint = case["params"].get("keyint", 1)
    tus, recs, levels, errs, gs = [], [], [], [], []
    ref = prev = None
    for t, f in enumerate(frames):
        key = t % keyint == 0
        cfg = edge_content.oracle_config(oracle, case, t)
        g = formula_level(oracle, cfg, key)
        py, pc = pool(g, False), pool(g, True)
        E = np.zeros((3, 16), dtype=np.uint64)
        for i in range(16):
            probe = edge_content.oracle_config(oracle, case, t)
            probe.enable_cdef, probe.enable_lr, probe.deblock = 0, 0, 2
            for k, v in enumerate((py[i], py[i], pc[i], pc[i])):
                probe.lf_level[k] = v
            _, rec, _ = oracle.encode_frame(probe, f, with_seq_hdr=key, ref=None if key else ref, prev_src=None if key else prev)
            E[:, i] = plane_sse(rec, f)
        iy, iu, iv = (first_min(E[p]) for p in range(3))
        lv = [py[iy], py[iy], pc[iu], pc[iv]]
        cfg.deblock = 2
        for k, v in enumerate(lv):
            cfg.lf_level[k] = v
        tu, rec, _ = oracle.encode_frame(cfg, f, with_seq_hdr=key, ref=None if key else ref, prev_src=None if key else prev)
        tus.append(tu)
        recs.append(rec)
        levels.append(lv)
        errs.append(E)
        gs.append(g)
        ref, prev = rec, f
    return tus, recs, levels, errs, gs
