"""CPU tests of chroma loop restoration's interface (include/av1mi.h: enable_lr 3 / 4): the parameter's range,
the frame header it implies (U and V take luma's lr_type, lr_uv_shift 1), and tests/lr_ref.py pinned against the oracle's luma
restoration bit for bit."""
import os

import numpy as np
import pytest

import host_build
import lr_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def av1mi():
    return host_build.library()


def _bits(data, n):
    return [(data[i >> 3] >> (7 - (i & 7))) & 1 for i in range(n)]


def _headers(av1mi, lr, **kw):
    p = av1mi.default_params(kw.pop("w", 1920), kw.pop("h", 1080), kw.pop("bd", 10), enable_lr=lr, **kw)
    return av1mi.write_headers(p)


@pytest.mark.parametrize("v", [3, 4])
def test_enable_lr_chroma_accepted(av1mi, v):
    av1mi.write_headers(av1mi.default_params(640, 360, 8, enable_lr=v))


@pytest.mark.parametrize("v", [5, 255])
def test_enable_lr_refused(av1mi, v):
    with pytest.raises(av1mi.EncodeFailed) as e:
        av1mi.write_headers(av1mi.default_params(640, 360, 8, enable_lr=v))
    assert e.value.code == 1   # AV1MI_E_INVALID_ARG


@pytest.mark.parametrize("kw", [{}, dict(film_grain=20, cdef_search=3, deblock=1), dict(w=202, h=122, bd=8, cdf_update=0),
                                dict(w=3840, h=2160, tile_sb=2, enable_qm=1, film_grain=5, cdef_search=4)])
def test_lr_params_header(av1mi, kw):
    """3 / 4 against 1 / 2: the U and V lr_type fields take luma's (10 / 01 instead of 00) and lr_uv_shift = 1 follows
    lr_unit_shift; everything after lr_params moves by one bit"""
    seq0, fh0, bits0 = _headers(av1mi, 0, **dict(kw))
    _, fh1, bits1 = _headers(av1mi, 1, **dict(kw))
    b0, b1 = _bits(fh0, bits0), _bits(fh1, bits1)
    lr = next(i for i in range(bits0) if b0[i] != b1[i])   # lr_params starts with luma lr_type 10 where enable_lr 0 has tx_mode_select 0
    for lo, hi, t in ((1, 3, [1, 0]), (2, 4, [0, 1])):
        seq_l, fh_l, bits_l = _headers(av1mi, lo, **dict(kw))
        seq_h, fh_h, bits_h = _headers(av1mi, hi, **dict(kw))
        assert seq_h == seq_l
        assert bits_h == bits_l + 1
        bl, bh = _bits(fh_l, bits_l), _bits(fh_h, bits_h)
        assert bh[:lr] == bl[:lr] == b0[:lr]
        assert bl[lr:lr + 7] == t + [0, 0, 0, 0] + [0]      # Y, U = none, V = none, lr_unit_shift 0
        assert bh[lr:lr + 8] == t + t + t + [0] + [1]        # Y, U, V, lr_unit_shift 0, lr_uv_shift 1
        assert bh[lr + 8:] == bl[lr + 7:]


def _oracle_runs(oracle, w, h, bd, lr, seed, **kw):
    planes = [p.astype(np.int64) for p in oracle.synthclip_frame(w, h, bd, seed=seed, t=0)]
    _, pre, _ = oracle.encode_frame(oracle.default_config(w, h, bd, enable_cdef=0, enable_lr=0, **kw), planes)
    _, cdef, _ = oracle.encode_frame(oracle.default_config(w, h, bd, enable_cdef=1, enable_lr=0, **kw), planes)
    _, rest, _ = oracle.encode_frame(oracle.default_config(w, h, bd, enable_cdef=1, enable_lr=lr, **kw), planes)
    return planes, pre, cdef, rest


@pytest.mark.parametrize("w,h,bd,lr,kw", [
    (200, 120, 8, 1, {}),
    (200, 120, 8, 2, {}),
    (328, 248, 10, 2, dict(deblock=1)),
    (328, 248, 10, 1, dict(deblock=1, min_bs_log2=4, max_bs_log2=4)),
    (202, 122, 8, 2, dict(base_q_idx=180)),
    (202, 122, 10, 1, {}),
    (88, 72, 10, 2, dict(deblock=1)),       # a single unit
])
def test_lr_ref_matches_the_oracle_luma(oracle, w, h, bd, lr, kw):
    """lr_ref's rule and filters on the oracle's pre-CDEF and CDEF frames give the oracle's restored luma"""
    src, pre, cdef, rest = _oracle_runs(oracle, w, h, bd, lr, 300 + w + lr, **kw)
    assert np.array_equal(cdef[1], rest[1]) and np.array_equal(cdef[2], rest[2])
    got, choice, _ = lr_ref.restore(pre[0], cdef[0], src[0], bd, 0, lr == 2)
    assert np.array_equal(got, rest[0].astype(np.int64))
    assert choice.shape == (lr_ref.count_units(h, 64), lr_ref.count_units(w, 64))
