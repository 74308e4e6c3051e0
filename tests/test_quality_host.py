"""CPU tests of the quality pass (include/av1mi.h: av1mi_quality, av1mi_ctx_set_quality, av1mi_quality_result,
av1mi_encode_file_quality): the rule (av1-base_amd/csrc/ssim_rule.h) compiled for the host against tests/ssim_ref.py - random windows,
the fixed points, the bounds that keep its 64-bit products in range - the stand-alone program plain and under the sanitizers, what
the entry points refuse without a device, and the mirrors."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import host_build
import ssim_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "ssim_rule_host.cpp")
ONE = 1 << 24


@pytest.fixture(scope="module")
def av1mi():
    return host_build.library()


@pytest.fixture(scope="module")
def cxx():
    return host_build.host_cxx()


@pytest.fixture(scope="module")
def rule(cxx, tmp_path_factory):
    lib = C.CDLL(host_build.build_shared(cxx, SRC, tmp_path_factory.mktemp("ssim") / "libssimrule.so"))
    lib.ssim_window.argtypes = [C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_int]
    lib.ssim_factors.argtypes = [C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_int, C.POINTER(C.c_longlong)]
    lib.ssim_c1.restype = lib.ssim_c2.restype = C.c_uint
    return lib


def blocks(bd, seed=5):
    """pairs of 8x8 blocks: independent noise, saturated, anticorrelated, near-identical, flat - at the range's ends and inside it"""
    rng = np.random.default_rng(seed + bd)
    m = (1 << bd) - 1
    cb = (np.add.outer(np.arange(8), np.arange(8)) & 1) * m
    out = [(np.full((8, 8), m), np.zeros((8, 8), int)), (np.zeros((8, 8), int), np.full((8, 8), m)), (cb, m - cb), (cb, cb),
           (np.zeros((8, 8), int), np.zeros((8, 8), int)), (np.full((8, 8), m), np.full((8, 8), m)), (np.full((8, 8), m), cb)]
    for k in range(150):
        a = rng.integers(0, m + 1, (8, 8))
        if k % 3 == 0:
            b = rng.integers(0, m + 1, (8, 8))
        elif k % 3 == 1:
            b = np.clip(a + rng.integers(-3, 4, (8, 8)), 0, m)
        else:
            b = m - a   # anticorrelated
        if k % 10 == 0:
            a = (a > m // 2) * m   # saturated both ways
        out.append((a, b))
    return out


# ---------------------------------------------------------------- the rule, compiled for the host
@pytest.mark.parametrize("bd", [8, 10])
def test_rule_equals_the_restatement_and_stays_in_range(rule, bd):
    assert (rule.ssim_c1(bd), rule.ssim_c2(bd)) == ssim_ref.C[bd]
    signs = set()
    for a, b in blocks(bd):
        s = ssim_ref.sums_of(a, b)
        F = (C.c_longlong * 4)()
        rule.ssim_factors(*s, bd, F)
        A, B, Cn, D = list(F)
        assert (A, B, Cn, D) == ssim_ref.factors(*s, bd)
        assert 0 < A <= B < 2 ** 34 and abs(Cn) <= D < 2 ** 35, (A, B, Cn, D)   # the four bounds
        w = rule.ssim_window(*s, bd)
        assert w == ssim_ref.window(*s, bd) and -ONE <= w <= ONE
        signs.add(w < 0)
    assert signs == {False, True}


@pytest.mark.parametrize("bd", [8, 10])
def test_fixed_points(rule, bd):
    m = (1 << bd) - 1
    cb = (np.add.outer(np.arange(8), np.arange(8)) & 1) * m
    rng = np.random.default_rng(9)
    for a in (np.zeros((8, 8), int), np.full((8, 8), m), cb, rng.integers(0, m + 1, (8, 8))):
        assert rule.ssim_window(*ssim_ref.sums_of(a, a), bd) == ONE           # identical planes
    assert rule.ssim_window(*ssim_ref.sums_of(np.full((8, 8), m), np.zeros((8, 8), int)), bd) == 1677   # all-max against all-zero
    assert rule.ssim_window(*ssim_ref.sums_of(cb, m - cb), bd) == -16716926   # a full-swing checkerboard against its inverse
    for n, want in ((0, 0), (7, 0), (8, 1), (11, 1), (12, 2), (33, 7), (35, 7), (65, 15), (66, 15), (136, 33), (1080, 269)):
        assert rule.ssim_windows(n) == ssim_ref.windows_along(n) == want


def test_restatement_planes_equal_its_windows():
    """ssim_ref's vectorised planes against its one-window form, and independent noise giving negative windows"""
    rng = np.random.default_rng(2)
    for bd, (h, w) in ((8, (8, 8)), (10, (35, 65)), (8, (33, 20))):
        m = (1 << bd) - 1
        a, b = rng.integers(0, m + 1, (h, w)), rng.integers(0, m + 1, (h, w))
        W = ssim_ref.window_map(a, b, bd)
        assert W.shape == (ssim_ref.windows_along(h), ssim_ref.windows_along(w))
        for i in range(W.shape[0]):
            for j in range(W.shape[1]):
                assert W[i, j] == ssim_ref.window(*ssim_ref.sums_of(a[4 * i:4 * i + 8, 4 * j:4 * j + 8], b[4 * i:4 * i + 8, 4 * j:4 * j + 8]), bd)
        assert (W < 0).any() or W.size == 1
        assert (ssim_ref.window_map(a, a, bd) == ONE).all()
    assert ssim_ref.window_map(np.zeros((4, 4), int), np.zeros((4, 4), int), 8).size == 0   # the chroma of an 8x8 frame


# ---------------------------------------------------------------- the stand-alone program
@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    lines, want = [], []
    for bd in (8, 10):
        for k, (a, b) in enumerate(blocks(bd, seed=11)):
            s = ssim_ref.sums_of(a, b)
            if k % 2:
                lines.append("S %d %d %d %d %d" % ((bd,) + s))
                want.append("%d %d %d %d %d" % (ssim_ref.factors(*s, bd) + (ssim_ref.window(*s, bd),)))
            else:
                lines.append("W %d %s %s" % (bd, " ".join(map(str, a.ravel())), " ".join(map(str, b.ravel()))))
                want.append("%d %d %d %d %d" % (s + (ssim_ref.window(*s, bd),)))
    for n in (0, 7, 8, 65, 1080):
        lines.append("N %d" % n)
        want.append("%d" % ssim_ref.windows_along(n))
    path = tmp_path_factory.mktemp("ssim_cases") / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    return str(path), want


def test_standalone_program_equals_the_restatement(cxx, cases, tmp_path):
    out = host_build.run_program(cxx, SRC, tmp_path / "ssim_rule_host", args=[cases[0]])
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.split("\n")[:-1] == cases[1]


def test_standalone_program_under_sanitizers(cxx, cases, tmp_path):
    """... and under AddressSanitizer and UndefinedBehaviorSanitizer (host code only, run on its own).  Skipped only where an empty
    program does not build and run under the sanitizers - their runtimes are not installed"""
    out = host_build.run_program(cxx, SRC, tmp_path / "ssim_rule_host_san", args=[cases[0]], sanitized=True)
    assert out.returncode == 0, out.stdout[-500:] + out.stderr[-2000:]
    assert out.stdout.split("\n")[:-1] == cases[1]


# ---------------------------------------------------------------- entry points and mirrors
def test_entry_points_check_their_arguments_first(av1mi):
    """no context, no frames, no output, no frame: AV1MI_E_INVALID_ARG before anything touches a device"""
    p = av1mi.default_params(64, 64, 8)
    buf = C.create_string_buffer(64 * 64 * 3 // 2)
    out = (av1mi.PlaneQuality * 3)()
    q = av1mi._lib.av1mi_quality
    assert q(None, C.byref(p), buf, buf, 1, 0, out, None) == av1mi.E_INVALID_ARG
    fake = C.c_void_p(16)   # never dereferenced: the null checks come first
    assert q(fake, None, buf, buf, 1, 0, out, None) == av1mi.E_INVALID_ARG
    assert q(fake, C.byref(p), None, buf, 1, 0, out, None) == av1mi.E_INVALID_ARG
    assert q(fake, C.byref(p), buf, None, 1, 0, out, None) == av1mi.E_INVALID_ARG
    assert q(fake, C.byref(p), buf, buf, 0, 0, out, None) == av1mi.E_INVALID_ARG
    assert q(fake, C.byref(p), buf, buf, 1, 0, None, None) == av1mi.E_INVALID_ARG
    assert av1mi._lib.av1mi_ctx_set_quality(None, 1) == av1mi.E_INVALID_ARG
    assert av1mi._lib.av1mi_quality_result(None, 1, out) == av1mi.E_INVALID_ARG
    assert av1mi._lib.av1mi_encode_file_quality(None, C.cast(None, av1mi.PROGRESS_CB), None, None, out) == av1mi.E_INVALID_ARG
    job = av1mi.Job()   # no paths
    assert av1mi._lib.av1mi_encode_file_quality(C.byref(job), C.cast(None, av1mi.PROGRESS_CB), None, None, out) == av1mi.E_INVALID_ARG


def test_abi_unchanged_and_symbols_named(av1mi):
    assert C.sizeof(av1mi.PlaneQuality) == 24
    assert [(n, C.sizeof(t)) for n, t in av1mi.PlaneQuality._fields_] == [("sse", 8), ("ssim_sum", 8), ("windows", 4), ("reserved", 4)]
    assert av1mi.ABI_VERSION == int(av1mi._lib.av1mi_abi_version()) == 8 and av1mi.struct_sizes() == av1mi.mirror_sizes()
    hdr = open(os.path.join(ROOT, "include", "av1mi.h")).read()
    shim = open(os.path.join(ROOT, "integration", "mi355x.rs")).read()
    assert "#define AV1MI_ABI_VERSION 8" in hdr and re.search(r"\}\s*av1mi_plane_quality\s*;", hdr)
    for name in ("av1mi_quality", "av1mi_ctx_set_quality", "av1mi_quality_result", "av1mi_encode_file_quality"):
        assert name in av1mi.ABI_SYMBOLS
        assert getattr(av1mi._lib, name) is not None   # exported
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert re.search(r"fn\s+%s\s*\(" % name, shim), name
    assert "pub struct Av1miPlaneQuality" in shim and "size_of::<Av1miPlaneQuality>() == 24" in shim


def test_ssim_helper(av1mi):
    """plane sums -> SSIM Y / U / V / all and dB; a plane without windows drops out and the weights are renormalised"""
    one = 1 << av1mi.SSIM_Q
    r = av1mi.ssim_of([(0, 10 * one, 10), (0, 2 * one, 4), (0, 0, 4)])
    assert (r["y"], r["u"], r["v"]) == (1.0, 0.5, 0.0) and abs(r["all"] - 0.85) < 1e-12 and abs(r["db"] + 10 * np.log10(0.15)) < 1e-9
    r = av1mi.ssim_of([(5, 3 * one // 4, 1), (7, 0, 0), (7, 0, 0)])   # an 8x8 frame: luma alone
    assert r["u"] is None and r["v"] is None and r["y"] == 0.75 and abs(r["all"] - 0.75) < 1e-12   # (the renormalising division rounds)
    assert av1mi.ssim_of([(0, one, 1), (0, 0, 0), (0, 0, 0)])["db"] == 99.0 and av1mi.ssim_of([(0, 0, 0)] * 3)["all"] is None
    assert abs(av1mi.ssim_of([(0, -one // 2, 1)] * 3)["all"] + 0.5) < 1e-12
    assert [tuple(x) for x in av1mi.quality_window_grid(130, 70)] == [(16, 31), (7, 15), (7, 15)]
    assert av1mi.quality_window_grid(8, 8) == [(1, 1), (0, 0), (0, 0)]
    got = ssim_ref.ssim_of([(0, 10 * one, 10), (0, 2 * one, 4), (0, 0, 4)])
    assert got[:3] == [1.0, 0.5, 0.0] and abs(got[3] - 0.85) < 1e-12
