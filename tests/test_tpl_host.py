"""CPU tests of the temporal term's interface (include/av1mi.h: av1mi_params.cq_level bits 12-14, av1mi_tpl_analysis): how the field
packs and what is refused, the three frame-header bits a temporal strength alone implies, the ABI staying what it was, and the rule header
(av1-base_amd/csrc/tpl_rule.h) compiled for the host against tests/tpl_ref.py on synthetic inputs - also those no small clip reaches."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import aq_ref
import host_build
import tpl_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def av1mi():
    return host_build.library()


def _bits(data, n):
    return [(data[i >> 3] >> (7 - (i & 7))) & 1 for i in range(n)]


# ---------------------------------------------------------------- packing
@pytest.mark.parametrize("aq", [None, 0, 2, 4])
@pytest.mark.parametrize("s", [1, 2, 3, 4])
def test_packed_field_accepted(av1mi, s, aq):
    kw = {} if aq is None else dict(aq_strength=aq)
    p = av1mi.default_params(640, 360, 8, cq_level=30, tpl_strength=s, **kw)
    assert p.cq_level == 30 | (aq or 0) << 8 | s << 12 == av1mi.cq_aq_tpl(30, aq or 0, s)
    assert av1mi.cq_level_of(p.cq_level) == 30 and av1mi.aq_strength_of(p.cq_level) == (aq or 0) and av1mi.tpl_strength_of(p.cq_level) == s
    assert tpl_ref.field_decode(p.cq_level) == (True, 30, aq or 0, s)
    av1mi.write_headers(p)
    av1mi.write_headers(av1mi.default_params(640, 360, 8, cq_level=30 | s << 12))   # the raw field, as the issue of the feature states it


@pytest.mark.parametrize("v", [30 | 5 << 12, 30 | 7 << 12, 30 | 1 << 15, 30 | 1 << 11 | 1 << 12, 30 | 1 << 16 | 2 << 12, 30 | 5 << 8 | 1 << 12, 0 | 1 << 12])
def test_packed_field_refused(av1mi, v):
    assert not tpl_ref.field_decode(v)[0]
    with pytest.raises(av1mi.EncodeFailed) as e:
        av1mi.write_headers(av1mi.default_params(640, 360, 8, cq_level=v))
    assert e.value.code == 1   # AV1MI_E_INVALID_ARG


def test_default_params_keywords(av1mi):
    assert av1mi.default_params(64, 64, 8, tpl_strength=3).cq_level == 30 | 3 << 12
    assert av1mi.default_params(64, 64, 8, tpl_strength=2, aq_strength=1, cq_level=8).cq_level == 8 | 1 << 8 | 2 << 12
    assert av1mi.default_params(64, 64, 8, aq_strength=1, cq_level=8 | 2 << 12).cq_level == 8 | 1 << 8 | 2 << 12   # one keyword keeps the other's bits
    assert av1mi.default_params(64, 64, 8, tpl_strength=0, cq_level=8 | 2 << 12).cq_level == 8
    assert av1mi.TPL_MAX_STRENGTH == 4


def test_abi_unchanged_and_symbol_exported(av1mi):
    assert C.sizeof(av1mi.Params) == 36 * 4 and av1mi.struct_sizes() == av1mi.mirror_sizes()
    assert av1mi.ABI_VERSION == int(av1mi._lib.av1mi_abi_version()) == 8
    assert "av1mi_tpl_analysis" in av1mi.ABI_SYMBOLS
    assert getattr(av1mi._lib, "av1mi_tpl_analysis") is not None   # exported
    hdr = open(os.path.join(ROOT, "include", "av1mi.h")).read()
    assert re.search(r"\bint\s+av1mi_tpl_analysis\s*\(", hdr)
    for macro in ("AV1MI_CQ_AQ_TPL", "AV1MI_TPL_STRENGTH"):
        assert re.search(r"#define\s+%s\(" % macro, hdr), macro
    assert "#define AV1MI_ABI_VERSION 8" in hdr
    shim = open(os.path.join(ROOT, "integration", "mi355x.rs")).read()
    assert "fn cq_aq_tpl(" in shim and "36 * 4" in shim


def test_analysis_checks_its_arguments_first(av1mi):
    """no context: AV1MI_E_INVALID_ARG before anything touches a device"""
    p = av1mi.default_params(64, 64, 8, tpl_strength=2)
    assert av1mi._lib.av1mi_tpl_analysis(None, C.byref(p), None, 1, 0, None, None, None, None, None, None) == 1


# ---------------------------------------------------------------- frame header
@pytest.mark.parametrize("kw", [{}, dict(film_grain=20, deblock=1, enable_lr=2, enable_qm=1), dict(keyint=240, cdef_search=3)])
def test_header_gains_the_three_bits(av1mi, kw):
    """a temporal strength alone: delta_q_present 0 -> 1, delta_q_res = 2, delta_lf_present = 0 - exactly what a spatial strength adds"""
    seq0, fh0, bits0 = av1mi.write_headers(av1mi.default_params(1920, 1080, 10, cq_level=30, **kw))
    got = [av1mi.write_headers(av1mi.default_params(1920, 1080, 10, cq_level=30, tpl_strength=s, **kw)) for s in (1, 2, 3, 4)]
    assert all(g == got[0] for g in got)   # the header does not carry the strength
    assert got[0] == av1mi.write_headers(av1mi.default_params(1920, 1080, 10, cq_level=30, aq_strength=2, **kw))
    assert got[0] == av1mi.write_headers(av1mi.default_params(1920, 1080, 10, cq_level=30, aq_strength=2, tpl_strength=3, **kw))
    seq1, fh1, bits1 = got[0]
    assert seq1 == seq0 and bits1 == bits0 + 3
    b0, b1 = _bits(fh0, bits0), _bits(fh1, bits1)
    d = next(i for i in range(bits0) if b0[i] != b1[i])
    assert b0[d] == 0 and b1[d:d + 4] == [1, 1, 0, 0] and b1[d + 4:] == b0[d + 1:]


# ---------------------------------------------------------------- the rule header, compiled for the host
@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    lib = C.CDLL(host_build.build_shared(host_build.host_cxx(), os.path.join(ROOT, "tests", "host", "tpl_rule_host.cpp"), tmp_path_factory.mktemp("tpl") / "libtplrule.so"))
    u64 = C.c_ulonglong
    lib.tpl_log2_q4.argtypes = [u64]
    lib.tpl_intra.argtypes = [C.c_void_p]
    lib.tpl_intra.restype = C.c_uint
    lib.tpl_inter.argtypes = [C.c_uint, C.c_uint]
    lib.tpl_inter.restype = C.c_uint
    lib.tpl_flow.argtypes = [C.c_uint, C.c_uint, u64]
    lib.tpl_flow.restype = u64
    lib.tpl_split.argtypes = [C.c_int] * 6 + [u64, C.c_void_p, C.c_void_p]
    lib.tpl_split.restype = None
    lib.tpl_beta.argtypes = [u64, u64]
    lib.tpl_mean_beta.argtypes = [u64, u64]
    lib.tpl_qindex_of.argtypes = [C.c_int] * 7
    lib.tpl_flow_entries.argtypes = [C.c_int] * 3
    lib.tpl_flow_entries.restype = u64
    return lib


def test_rule_log2_on_64_bit_arguments(rule):
    xs = list(range(1, 2048)) + [v for k in range(1, 59) for v in ((1 << k) - 1, 1 << k, (1 << k) + 1, (1 << k) + (1 << k >> 1), 3 << k >> 1)]
    xs += [int(v) for v in np.random.default_rng(1).integers(1, 1 << 58, 2000)]
    for x in xs:
        if 1 <= x <= 1 << 58:
            assert rule.tpl_log2_q4(x) == aq_ref.L(x), x
    assert rule.tpl_log2_q4(1 << 58) == 16 * 58
    assert rule.tpl_beta(1000, 1000) == 0 and rule.tpl_beta(1000, 2000) == 16 and rule.tpl_beta(1, 1 << 58) == 16 * 58


@pytest.mark.parametrize("bd", [8, 10])
def test_rule_costs(rule, bd):
    rng = np.random.default_rng(bd)
    mx = (1 << bd) - 1
    blocks = [np.full((16, 16), v) for v in (0, mx, mx // 2)] + [np.where(np.arange(256).reshape(16, 16) % 16 < 8, 0, mx)]
    blocks += [rng.integers(0, mx + 1, (16, 16)) for _ in range(30)] + [rng.integers(mx - 2, mx + 1, (16, 16)) for _ in range(6)]
    for b in blocks:
        a = np.ascontiguousarray(b, dtype=np.uint16)
        assert rule.tpl_intra(a.ctypes.data) == tpl_ref.intra_cost(b)
    assert rule.tpl_intra(np.full(256, mx, np.uint16).ctypes.data) == 1          # flat: at least 1
    assert rule.tpl_intra(np.ascontiguousarray(blocks[3], dtype=np.uint16).ctypes.data) >= 128 * mx - 256
    assert [rule.tpl_inter(s, 500) for s in (0, 499, 500, 501, 1 << 20)] == [0, 499, 500, 500, 500]
    for I, Cc, A in [(1, 1, 0), (1, 0, 0), (500, 0, 0), (500, 499, 12345), (261888, 0, 1 << 43), (261888, 17, (1 << 43) + 12345), (7, 3, 10**12)]:
        assert rule.tpl_flow(I, Cc, A) == tpl_ref.flow_of(I, Cc, A), (I, Cc, A)
    assert rule.tpl_flow_entries(200, 120, 5) == 5 * 13 * 8 + 1 and rule.tpl_flow_entries(8, 8, 1) == 2


def _split(rule, bx, by, dx, dy, nbx, nby, T):
    cell = (C.c_int * 4)()
    share = (C.c_ulonglong * 4)()
    rule.tpl_split(bx, by, dx, dy, nbx, nby, T, cell, share)
    return [(cell[k], share[k]) for k in range(4) if cell[k] >= 0]


def test_rule_flow_split(rule):
    """every vector of +-16 at the grid's corners, its edges and inside; and away from the edge the four shares add up to T less at
    most the four floors"""
    nbx, nby = 5, 4
    T = 987654321987
    at = [(0, 0), (nbx - 1, 0), (0, nby - 1), (nbx - 1, nby - 1), (2, 0), (0, 2), (nbx - 1, 1), (2, nby - 1), (2, 2)]
    for bx, by in at:
        for dy in range(-16, 17):
            for dx in range(-16, 17):
                got, want = _split(rule, bx, by, dx, dy, nbx, nby, T), tpl_ref.split(bx, by, dx, dy, nbx, nby, T)
                assert got == want, (bx, by, dx, dy)
                assert len(got) <= 4 and all(0 <= c < nbx * nby for c, _ in got)
                total = sum(s for _, s in got)
                if (bx, by) == (2, 2):   # one block from every edge: no area is lost
                    assert T - 4 < total <= T
                    assert len(got) == (1 if dx % 16 == 0 else 2) * (1 if dy % 16 == 0 else 2)
                else:
                    assert total <= T
    assert _split(rule, 0, 0, -16, -16, nbx, nby, T) == [] and _split(rule, 0, 0, 0, 0, nbx, nby, T) == [(0, T)]
    assert _split(rule, 1, 1, -16, 16, nbx, nby, T) == [(2 * nbx, T)]
    assert _split(rule, 0, 0, -1, -1, 1, 1, 256) == [(0, 225)]   # a one-block grid keeps what stays inside


def test_rule_mean_and_combined_delta(rule):
    """the chunk mean, and the combined delta with every pair of strengths: base indices in the middle and at both ends (4 and 255: the
    one-sided clamps), reaching -6 and +6"""
    rng = np.random.default_rng(9)
    for n in (1, 2, 7, 35, 600):
        b = rng.integers(0, 120, n)
        assert rule.tpl_mean_beta(int(b.sum()), n) == tpl_ref.mean_beta(b)
    seen = set()
    for base in (4, 8, 120, 236, 249, 255):
        for aq in (0, 1, 2, 4):
            for tpl in (1, 2, 4):
                for shape in ((1, 1), (2, 4), (9, 15)):
                    for spread in (4, 48, 130):
                        E = rng.integers(0, 240, shape)
                        beta = rng.integers(0, spread, shape)
                        Mb = tpl_ref.mean_beta(beta) + int(rng.integers(-3, 4))   # (the chunk's mean, not this frame's)
                        M = (int(E.sum()) + E.size // 2) // E.size
                        want = tpl_ref.qindex_of(E if aq else None, beta, Mb, aq, tpl, base)
                        got = np.array([rule.tpl_qindex_of(aq, int(e), M, tpl, int(b), Mb, base) for e, b in zip(E.ravel(), beta.ravel())]).reshape(shape)
                        assert np.array_equal(got, want), (base, aq, tpl, shape)
                        assert want.min() >= 1 and want.max() <= 255
                        seen.update((base, (int(v) - base) // 4) for v in want.ravel())
    assert {d for b, d in seen if b == 120} == set(range(-6, 7))
    assert {d for b, d in seen if b == 4} == set(range(0, 7))
    assert {d for b, d in seen if b == 255} == set(range(-6, 1))
    # a superblock everything depends on gets the finer quantiser, one nothing depends on the coarser
    assert rule.tpl_qindex_of(0, 0, 0, 4, 40, 20, 120) == 120 - 4 * 3 and rule.tpl_qindex_of(0, 0, 0, 4, 0, 20, 120) == 120 + 4 * 3
    # without a temporal strength: the spatial rule
    for E in (0, 17, 200):
        assert rule.tpl_qindex_of(3, E, 100, 0, 55, 7, 120) == int(aq_ref.qindex_of(np.array([E, 200 - E]), 3, 120)[0])


def test_reference_properties():
    """the restatement on tiny clips: nothing flows into the last frame or across a key frame, a static clip's beta falls frame by frame,
    independent noise has none"""
    import tf_ref
    w, h, n = 72, 56, 4
    st = tpl_ref.analysis(tf_ref.pattern_clip(w, h, 8, n, 3, sigma=0.0, static=True)[0], w, h, 8, n, 240, 8)
    assert (st["beta"][-1] == 0).all() and all(st["beta"][f].min() > st["beta"][f + 1].max() for f in range(n - 1))
    assert (st["flow"][-1] == 0).all() and (st["key"][0] == tpl_ref.NONE).all() and (st["key"][1:] != tpl_ref.NONE).all()
    k2 = tpl_ref.analysis(tf_ref.pattern_clip(w, h, 8, n, 3, sigma=0.0, static=True)[0], w, h, 8, n, 2, 8)
    assert (k2["beta"][1] == 0).all() and (k2["beta"][3] == 0).all() and (k2["beta"][0] > 0).all() and (k2["inter"][2] == k2["intra"][2]).all()
    rng = np.random.default_rng(4)
    noise = rng.integers(0, 256, n * w * h * 3 // 2).astype(np.uint8).tobytes()
    assert tpl_ref.analysis(noise, w, h, 8, n, 240, 8)["beta"].max() <= 1
