"""CPU tests of the CDEF strength search's interface (include/av1mi.h: av1mi_params.cdef_search): the parameter's range, the
frame header it implies (cdef_bits = k - 1 and 2^(k-1) strength pairs) and the ABI layout with the new last field."""
import ctypes as C
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def av1mi():
    lib = os.path.join(ROOT, "av1-base_amd", "libav1mi.so")
    if not os.path.exists(lib):
        import importlib.util
        spec = importlib.util.spec_from_file_location("av1mi_build", os.path.join(ROOT, "av1-base_amd", "build.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mod.build()
    import av1mi as m
    return m


def _bits(data, n):
    return [(data[i >> 3] >> (7 - (i & 7))) & 1 for i in range(n)]


def _headers(av1mi, k, **kw):
    p = av1mi.default_params(kw.pop("w", 1920), kw.pop("h", 1080), kw.pop("bd", 10), cdef_search=k, **kw)
    return av1mi.write_headers(p)


@pytest.mark.parametrize("k", [0, 1, 2, 3, 4])
def test_cdef_search_accepted(av1mi, k):
    p = av1mi.default_params(640, 360, 8, cdef_search=k)
    assert p.cdef_search == k
    av1mi.write_headers(p)


def test_cdef_search_refused(av1mi):
    with pytest.raises(av1mi.EncodeFailed) as e:
        av1mi.write_headers(av1mi.default_params(640, 360, 8, cdef_search=5))
    assert e.value.code == 1   # AV1MI_E_INVALID_ARG
    with pytest.raises(av1mi.EncodeFailed) as e:
        av1mi.write_headers(av1mi.default_params(640, 360, 8, cdef_search=1, enable_cdef=0))
    assert e.value.code == 1
    av1mi.write_headers(av1mi.default_params(640, 360, 8, cdef_search=0, enable_cdef=0))


@pytest.mark.parametrize("kw", [{}, dict(film_grain=20, deblock=1, enable_lr=2, enable_qm=1), dict(w=328, h=200, bd=8, cdf_update=0),
                                dict(w=3840, h=2160, tile_sb=2, cdef_damping=4, cdef_y_pri=5, cdef_y_sec=1)])
def test_cdef_search_header_layout(av1mi, kw):
    seq0, fh0, bits0 = _headers(av1mi, 0, **dict(kw))
    seq1, fh1, bits1 = _headers(av1mi, 1, **dict(kw))
    assert (seq1, fh1, bits1) == (seq0, fh0, bits0)   # one pair: cdef_bits 0, the same bytes as without the search
    fh2 = _headers(av1mi, 2, **dict(kw))[1]
    b1, b2 = _bits(fh1, bits1), _bits(fh2, bits1)
    d = next(i for i in range(bits1) if b1[i] != b2[i])
    # cdef_bits is the 2-bit field in front of the strengths: 00 for k = 1, 01 for k = 2
    cb = d - 1
    assert b1[cb:cb + 2] == [0, 0] and b2[cb:cb + 2] == [0, 1]
    str_bit = cb + 2
    for k in (2, 3, 4):
        _, fh, bits = _headers(av1mi, k, **dict(kw))
        n = 1 << (k - 1)
        assert bits == bits1 + 12 * (n - 1)
        b = _bits(fh, bits)
        assert b[:cb] == b1[:cb]
        assert b[cb] * 2 + b[cb + 1] == k - 1
        # the placeholders: the fixed strengths, n times; everything after them as without the search
        for j in range(n):
            assert b[str_bit + 12 * j:str_bit + 12 * (j + 1)] == b1[str_bit:str_bit + 12]
        assert b[str_bit + 12 * n:] == b1[str_bit + 12:]


def test_cdef_search_layout(av1mi):
    sizes = av1mi.struct_sizes()
    assert sizes == av1mi.mirror_sizes()
    assert av1mi.Params.cdef_search.offset == C.sizeof(av1mi.Params) - 4 == av1mi.Params.me_presearch.offset + 4
    assert sizes[0] == C.sizeof(av1mi.Params) == 36 * 4
    assert av1mi.ABI_VERSION == int(av1mi._lib.av1mi_abi_version()) == 8
