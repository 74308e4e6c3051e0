"""CPU tests of the adaptive quantisation's interface (include/av1mi.h: av1mi_params.cq_level bits 8-10, av1mi_aq_qindex): how the
field packs and what is refused, the three frame-header bits it implies (delta_q_present 1, delta_q_res 2, delta_lf_present 0), the ABI
staying what it was, and the rule header (av1-base_amd/csrc/aq_rule.h) compiled for the host against tests/aq_ref.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import host_build
import aq_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def av1mi():
    return host_build.library()


def _bits(data, n):
    return [(data[i >> 3] >> (7 - (i & 7))) & 1 for i in range(n)]


# ---------------------------------------------------------------- packing
@pytest.mark.parametrize("cq", [1, 30, 63])
@pytest.mark.parametrize("s", [0, 1, 2, 3, 4])
def test_packed_field_accepted(av1mi, cq, s):
    p = av1mi.default_params(640, 360, 8, cq_level=cq, aq_strength=s)
    assert p.cq_level == cq | (s << 8) == av1mi.cq_aq(cq, s)
    assert av1mi.cq_level_of(p.cq_level) == cq and av1mi.aq_strength_of(p.cq_level) == s
    av1mi.write_headers(p)


@pytest.mark.parametrize("v", [30 | 5 << 8, 30 | 7 << 8, 30 | 1 << 11, 30 | 1 << 31, 0 | 2 << 8, 64 | 2 << 8, 64, 0])
def test_packed_field_refused(av1mi, v):
    with pytest.raises(av1mi.EncodeFailed) as e:
        av1mi.write_headers(av1mi.default_params(640, 360, 8, cq_level=v))
    assert e.value.code == 1   # AV1MI_E_INVALID_ARG


def test_default_params_keywords(av1mi):
    """aq_strength packs the field whatever the order, with the default CQ level too; every other keyword is a structure field"""
    assert av1mi.default_params(64, 64, 8, aq_strength=3).cq_level == 30 | 3 << 8
    assert av1mi.default_params(64, 64, 8, aq_strength=2, cq_level=8).cq_level == 8 | 2 << 8
    assert av1mi.default_params(64, 64, 8, cq_level=8).cq_level == 8
    with pytest.raises(AttributeError):
        av1mi.default_params(64, 64, 8, no_such_field=1)
    assert [av1mi.cq_to_qindex(c) for c in (0, 1, 30, 62, 63)] == [0, 4, 120, 249, 255]


def test_abi_unchanged_and_symbol_exported(av1mi):
    assert C.sizeof(av1mi.Params) == 36 * 4 and av1mi.struct_sizes() == av1mi.mirror_sizes()
    assert av1mi.ABI_VERSION == int(av1mi._lib.av1mi_abi_version()) == 8
    assert "av1mi_aq_qindex" in av1mi.ABI_SYMBOLS
    assert getattr(av1mi._lib, "av1mi_aq_qindex") is not None   # exported
    hdr = open(os.path.join(ROOT, "include", "av1mi.h")).read()
    assert re.search(r"\bint\s+av1mi_aq_qindex\s*\(", hdr)
    for macro in ("AV1MI_CQ_AQ", "AV1MI_CQ_LEVEL", "AV1MI_AQ_STRENGTH"):
        assert re.search(r"#define\s+%s\(" % macro, hdr), macro
    assert "#define AV1MI_ABI_VERSION 8" in hdr
    shim = open(os.path.join(ROOT, "integration", "mi355x.rs")).read()
    assert "fn cq_aq(" in shim and "36 * 4" in shim


# ---------------------------------------------------------------- frame header
MIXES = [{}, dict(film_grain=20, deblock=1, enable_lr=2, enable_qm=1), dict(w=328, h=200, bd=8, cdf_update=0),
         dict(w=3840, h=2160, tile_sb=2, cdef_damping=4, cdef_y_pri=5, cdef_y_sec=1), dict(cdef_search=3)]


def _headers(av1mi, cq, s, **kw):
    kw = dict(kw)
    args = (kw.pop("w", 1920), kw.pop("h", 1080), kw.pop("bd", 10))
    if s is None:
        return av1mi.write_headers(av1mi.default_params(*args, cq_level=cq, **kw))
    return av1mi.write_headers(av1mi.default_params(*args, cq_level=cq, aq_strength=s, **kw))


@pytest.mark.parametrize("kw", MIXES)
@pytest.mark.parametrize("cq", [30, 1, 63])
def test_header_layout(av1mi, kw, cq):
    seq0, fh0, bits0 = _headers(av1mi, cq, None, **kw)
    assert _headers(av1mi, cq, 0, **kw) == (seq0, fh0, bits0)   # strength 0: the plain CQ value's bytes
    b0 = _bits(fh0, bits0)
    got = [_headers(av1mi, cq, s, **kw) for s in (1, 2, 3, 4)]
    assert all(g == got[0] for g in got)                        # the header does not carry the strength
    seq1, fh1, bits1 = got[0]
    assert seq1 == seq0 and bits1 == bits0 + 3
    b1 = _bits(fh1, bits1)
    d = next(i for i in range(bits0) if b0[i] != b1[i])
    assert b0[:d] == b1[:d]
    assert b0[d] == 0 and b1[d:d + 4] == [1, 1, 0, 0]           # delta_q_present 0 -> 1, delta_q_res = 2, delta_lf_present = 0
    assert b1[d + 4:] == b0[d + 1:]
    # ... and it is the bit behind segmentation_enabled: base_q_idx, three delta flags, using_qmatrix (+ two levels), 0, then this one
    qidx = av1mi.cq_to_qindex(cq)
    lead = 8 + 3 + 1 + (8 if kw.get("enable_qm") else 0) + 1
    assert sum(b << (7 - i) for i, b in enumerate(b1[d - lead:d - lead + 8])) == qidx


# ---------------------------------------------------------------- the rule header, compiled for the host
@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    lib = C.CDLL(host_build.build_shared(host_build.host_cxx(), os.path.join(ROOT, "tests", "host", "aq_rule_host.cpp"), tmp_path_factory.mktemp("aq") / "libaqrule.so"))
    lib.aq_log2_q4.argtypes = [C.c_uint]
    lib.aq_unit_energy.argtypes = [C.c_uint, C.c_uint, C.c_int]
    lib.aq_sb_energy.argtypes = [C.c_void_p, C.c_int]
    lib.aq_frame_qindex.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    return lib


def test_rule_log2(rule):
    xs = list(range(1, 4096)) + [v for k in range(1, 27) for v in ((1 << k) - 1, 1 << k, (1 << k) + 1)]
    for x in xs:
        assert rule.aq_log2_q4(x) == aq_ref.L(x), x
    assert aq_ref.L(1) == 0 and aq_ref.L(2) == 16 and aq_ref.L(3) == 24 and aq_ref.L(4) == 32


@pytest.mark.parametrize("bd", [8, 10])
def test_rule_unit_energy(rule, bd):
    """steps 1-2 on 8x8 units: flat, one step edge, full-range noise (10 bit: 64 Q and S^2 beyond 32 bits)"""
    rng = np.random.default_rng(bd)
    mx = (1 << bd) - 1
    units = [np.full((8, 8), v) for v in (0, mx, mx // 2)] + [np.where(np.arange(64).reshape(8, 8) % 8 < 4, 0, mx)]
    units += [rng.integers(0, mx + 1, (8, 8)) for _ in range(40)] + [rng.integers(mx - 3, mx + 1, (8, 8)) for _ in range(10)]
    for u in units:
        S, Q = int(u.sum()), int((u.astype(np.int64) ** 2).sum())
        assert rule.aq_unit_energy(S, Q, bd) == int(aq_ref.unit_energy(u, bd)[0, 0])
    assert rule.aq_unit_energy(64 * mx, 64 * mx * mx, bd) == 0   # flat: variance 0, L(1)


def test_rule_superblock_frame_delta_index(rule):
    """steps 3-6 on random grids: every strength, base indices in the middle and at both ends (4 and 255: the one-sided clamps), a
    single-superblock frame (d = 0)"""
    rng = np.random.default_rng(5)
    for n in (1, 2, 7, 35, 64):
        e = rng.integers(0, 240, n).astype(np.int32)
        assert rule.aq_sb_energy(e.ctypes.data, n) == (int(e.sum()) + n // 2) // n
    seen = set()
    for base in (4, 8, 120, 236, 249, 255):
        for strength in (1, 2, 3, 4):
            for shape in ((1, 1), (1, 2), (2, 4), (4, 6), (17, 30)):
                for spread in (4, 40, 240):
                    E = rng.integers(0, spread, shape).astype(np.int32)
                    q = np.zeros(E.size, np.int32)
                    M = rule.aq_frame_qindex(np.ascontiguousarray(E).ctypes.data, E.size, strength, base, q.ctypes.data)
                    assert M == (int(E.sum()) + E.size // 2) // E.size
                    want = aq_ref.qindex_of(E, strength, base)
                    assert np.array_equal(q.reshape(shape), want), (base, strength, shape)
                    assert want.min() >= 1 and want.max() <= 255 and len(set(want.ravel())) <= 13
                    if shape == (1, 1):
                        assert int(q[0]) == base
                    seen.update((base, int(v) - base) for v in want.ravel())
    assert {d for b, d in seen if b == 120} == set(range(-24, 25, 4))
    assert min(d for b, d in seen if b == 4) == 0 and max(d for b, d in seen if b == 4) == 24
    assert max(d for b, d in seen if b == 255) == 0 and min(d for b, d in seen if b == 255) == -24
