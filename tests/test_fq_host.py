"""CPU tests of the frame term's interface (include/av1mi.h: av1mi_params.cq_level bits 20-22, av1mi_tpl_frame_q, av1mi_frame_q_result):
how the field packs and what is refused, the frame header keeping the chunk's index as its placeholder, the ABI staying what it was, and
the rule (av1-base_amd/csrc/tpl_rule.h: av1mi_fq_*) compiled for the host against tests/fq_ref.py on synthetic inputs."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fq_ref
import host_build
import tpl_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def av1mi():
    return host_build.library()


# ---------------------------------------------------------------- packing
@pytest.mark.parametrize("aq,tpl", [(None, None), (0, 0), (2, 0), (0, 3), (4, 4)])
@pytest.mark.parametrize("s", [1, 2, 3, 4])
def test_packed_field_accepted(av1mi, s, aq, tpl):
    kw = {}
    if aq is not None:
        kw = dict(aq_strength=aq, tpl_strength=tpl)
    p = av1mi.default_params(640, 360, 8, cq_level=30, frame_q_strength=s, **kw)
    assert p.cq_level == 30 | (aq or 0) << 8 | (tpl or 0) << 12 | s << 20 == av1mi.cq_aq_tpl_fq(30, aq or 0, tpl or 0, s)
    assert av1mi.cq_level_of(p.cq_level) == 30 and av1mi.aq_strength_of(p.cq_level) == (aq or 0)
    assert av1mi.tpl_strength_of(p.cq_level) == (tpl or 0) and av1mi.frame_q_strength_of(p.cq_level) == s
    assert fq_ref.field_decode(p.cq_level) == (True, 30, aq or 0, tpl or 0, s)
    av1mi.write_headers(p)
    av1mi.write_headers(av1mi.default_params(640, 360, 8, cq_level=30 | s << 20))   # the raw field


@pytest.mark.parametrize("v", [30 | 5 << 20, 30 | 1 << 19, 30 | 1 << 23, 0 | 1 << 20,
                               30 | 7 << 20, 30 | 1 << 20 | 1 << 11, 30 | 1 << 20 | 1 << 15, 30 | 1 << 20 | 1 << 16, 30 | 1 << 20 | 1 << 31, 30 | 1 << 20 | 5 << 12])
def test_packed_field_refused(av1mi, v):
    assert not fq_ref.field_decode(v)[0]
    with pytest.raises(av1mi.EncodeFailed) as e:
        av1mi.write_headers(av1mi.default_params(640, 360, 8, cq_level=v))
    assert e.value.code == 1   # AV1MI_E_INVALID_ARG


def test_default_params_keywords(av1mi):
    assert av1mi.default_params(64, 64, 8, frame_q_strength=3).cq_level == 30 | 3 << 20
    assert av1mi.default_params(64, 64, 8, frame_q_strength=2, aq_strength=1, cq_level=8).cq_level == 8 | 1 << 8 | 2 << 20
    assert av1mi.default_params(64, 64, 8, tpl_strength=1, cq_level=8 | 2 << 20).cq_level == 8 | 1 << 12 | 2 << 20   # one keyword keeps the other's bits
    assert av1mi.default_params(64, 64, 8, frame_q_strength=0, cq_level=8 | 2 << 20 | 3 << 12).cq_level == 8 | 3 << 12
    assert av1mi.default_params(64, 64, 8).cq_level == 30   # off by default
    assert av1mi.FQ_MAX_STRENGTH == 4


# ---------------------------------------------------------------- frame header
@pytest.mark.parametrize("kw", [{}, dict(film_grain=20, deblock=1, enable_lr=2, enable_qm=1), dict(keyint=240, cdef_search=3)])
def test_header_keeps_the_chunks_index_as_placeholder(av1mi, kw):
    """the frame term alone adds no bit: delta_q_present stays "aq_strength or tpl_strength"; with a superblock strength the header
    is that strength's"""
    plain = av1mi.write_headers(av1mi.default_params(1920, 1080, 10, cq_level=30, **kw))
    for s in (1, 2, 3, 4):
        assert av1mi.write_headers(av1mi.default_params(1920, 1080, 10, cq_level=30, frame_q_strength=s, **kw)) == plain
    for sb in (dict(aq_strength=2), dict(tpl_strength=3), dict(aq_strength=4, tpl_strength=1)):
        want = av1mi.write_headers(av1mi.default_params(1920, 1080, 10, cq_level=30, **sb, **kw))
        assert want != plain
        assert av1mi.write_headers(av1mi.default_params(1920, 1080, 10, cq_level=30, frame_q_strength=4, **sb, **kw)) == want


# ---------------------------------------------------------------- params and ABI
def test_abi_unchanged_and_symbols_exported(av1mi):
    assert C.sizeof(av1mi.Params) == 36 * 4 and av1mi.struct_sizes() == av1mi.mirror_sizes()
    assert av1mi.ABI_VERSION == int(av1mi._lib.av1mi_abi_version()) == 8
    hdr = open(os.path.join(ROOT, "include", "av1mi.h")).read()
    for name in ("av1mi_tpl_frame_q", "av1mi_frame_q_result"):
        assert name in av1mi.ABI_SYMBOLS
        assert getattr(av1mi._lib, name) is not None   # exported
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
    for macro in ("AV1MI_CQ_AQ_TPL_FQ", "AV1MI_FQ_STRENGTH"):
        assert re.search(r"#define\s+%s\(" % macro, hdr), macro
    assert "#define AV1MI_ABI_VERSION 8" in hdr
    shim = open(os.path.join(ROOT, "integration", "mi355x.rs")).read()
    assert "fn cq_aq_tpl_fq(" in shim and "36 * 4" in shim
    assert re.search(r"fn\s+av1mi_tpl_frame_q\s*\(", shim) and re.search(r"fn\s+av1mi_frame_q_result\s*\(", shim)


def test_entry_points_check_their_arguments_first(av1mi):
    """no context: AV1MI_E_INVALID_ARG before anything touches a device"""
    p = av1mi.default_params(64, 64, 8, frame_q_strength=2)
    assert av1mi._lib.av1mi_tpl_frame_q(None, C.byref(p), None, 1, 0, None, None, None, None, None) == 1
    assert av1mi._lib.av1mi_frame_q_result(None, 1, None, None) == 1


# ---------------------------------------------------------------- the rule, compiled for the host
@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    lib = C.CDLL(host_build.build_shared(host_build.host_cxx(), os.path.join(ROOT, "tests", "host", "fq_rule_host.cpp"), tmp_path_factory.mktemp("fq") / "libfqrule.so"))
    u64 = C.c_ulonglong
    lib.fq_beta.argtypes = [u64, u64]
    lib.fq_mean.argtypes = [u64, u64]
    lib.fq_step.argtypes = [C.c_int] * 4
    lib.fq_qindex.argtypes = [C.c_int] * 4
    lib.fq_sb_qindex.argtypes = [C.c_int] * 7
    return lib


BASES = (4, 8, 120, 236, 249, 255)


def test_rule_constants_and_frame_beta(rule):
    assert (rule.fq_min_step(), rule.fq_max_step(), rule.fq_max_strength()) == (fq_ref.MIN_STEP, fq_ref.MAX_STEP, 4) == (-10, 4, 4)
    rng = np.random.default_rng(3)
    for _ in range(300):
        OF = int(rng.integers(1, 1 << 40))
        PF = OF + int(rng.integers(0, 1 << int(rng.integers(1, 56))))
        assert rule.fq_beta(OF, PF) == fq_ref.L(PF) - fq_ref.L(OF) >= 0
    assert rule.fq_beta(1000, 1000) == 0 and rule.fq_beta(1000, 2000) == 16 and rule.fq_beta(1, 1 << 58) == 16 * 58


def test_rule_steps_equal_the_restatement(rule):
    """random betaF vectors of 1 .. 600 frames, every base and strength; the reference reaches both step clamps at base 120 and only
    one side at the ends of the index range"""
    rng = np.random.default_rng(20)
    seen = set()
    for n in (1, 2, 3, 5, 7, 35, 240, 600):
        for spread in (2, 20, 90, 400):
            bF = [int(v) for v in rng.integers(0, spread, n)]
            MF = fq_ref.mean_of(bF)
            assert rule.fq_mean(sum(bF), n) == MF
            for base in BASES:
                for s in (1, 2, 3, 4):
                    want = fq_ref.steps(bF, s, base)
                    got = [rule.fq_step(s, b, MF, base) for b in bF]
                    assert got == want, (n, spread, base, s)
                    assert [rule.fq_qindex(s, b, MF, base) for b in bF] == fq_ref.frame_q(bF, s, base)
                    assert all(1 <= base + 4 * k <= 255 and fq_ref.MIN_STEP <= k <= fq_ref.MAX_STEP for k in want)
                    seen.update((base, k) for k in want)
    assert {k for b, k in seen if b == 120} == set(range(-10, 5))
    assert {k for b, k in seen if b == 4} == set(range(0, 5))
    assert {k for b, k in seen if b == 255} == set(range(-10, 1))
    assert min(k for b, k in seen if b == 8) == -1 and max(k for b, k in seen if b == 249) == 1
    # strength 1 is one step per doubling of PF / OF against the mean, strength 4 four; a frame everything depends on gets the finer index
    assert rule.fq_step(1, 48, 32, 120) == -1 and rule.fq_step(4, 48, 32, 120) == -4 and rule.fq_step(4, 16, 32, 120) == 4
    assert rule.fq_step(4, 32, 32, 120) == 0 and rule.fq_step(1, 39, 32, 120) == 0 and rule.fq_step(1, 40, 32, 120) == -1


def test_rule_superblock_delta_against_the_frames_index(rule):
    """the superblock delta with the frame's own mean beta and the clamp against q_f: every q_f the steps can give, every pair of
    strengths; the index never leaves 1 .. 255"""
    rng = np.random.default_rng(21)
    for base in BASES:
        lo, hi = fq_ref.step_range(base)
        for k in range(lo, hi + 1):
            q_f = base + 4 * k
            for aq, tpl in ((0, 0), (4, 0), (0, 2), (4, 2), (1, 4), (2, 1)):
                for shape in ((1, 1), (2, 4), (4, 6)):
                    for spread in (4, 48, 130):
                        E = rng.integers(0, 240, shape)
                        beta = rng.integers(0, spread, shape)
                        M = (int(E.sum()) + E.size // 2) // E.size
                        Mbf = tpl_ref.mean_beta(beta)
                        want = fq_ref.sb_qindex(E if aq else None, beta, aq, tpl, q_f)
                        if aq or tpl:
                            got = np.array([rule.fq_sb_qindex(aq, int(e) if aq else 0, M, tpl, int(b) if tpl else 0, Mbf if tpl else 0, q_f)
                                            for e, b in zip(E.ravel(), beta.ravel())]).reshape(shape)
                            assert np.array_equal(got, want), (base, k, aq, tpl, shape)
                        assert want.min() >= 1 and want.max() <= 255, (base, k, aq, tpl)
                        assert ((want - q_f) % 4 == 0).all() and np.abs(want - q_f).max() <= 24
                        assert -16 <= (int(want.min()) - base) // 4 and (int(want.max()) - base) // 4 <= 10   # the 27 slots around the chunk's index


def test_reference_on_a_tiny_static_clip():
    """the restatement: a static clip's frames fall in betaF from the key frame to the last frame, which nothing depends on - the steps
    rise frame by frame and have both signs; all key frames: no dependency, every step 0"""
    import tf_ref
    w, h, n = 72, 56, 5
    buf = tf_ref.pattern_clip(w, h, 8, n, 3, sigma=0.0, static=True)[0]
    d = fq_ref.decision(tpl_ref.analysis(buf, w, h, 8, n, 240, 8), 4, 120)
    assert d["beta"][-1] == 0 and all(a > b for a, b in zip(d["beta"], d["beta"][1:]))
    assert all(a <= b for a, b in zip(d["steps"], d["steps"][1:])) and d["steps"][0] < 0 < d["steps"][-1]
    assert fq_ref.decision(tpl_ref.analysis(buf, w, h, 8, n, 1, 8), 4, 120)["steps"] == [0] * n
