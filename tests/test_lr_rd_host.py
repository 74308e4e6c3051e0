"""CPU tests of the rate term of the restoration unit decisions (include/av1mi.h: AV1MI_LR_RD): the rule header
(av1-base_amd/csrc/lr_rate_rule.h) compiled for the host as a stand-alone program, plain and under the sanitizers, against the Python
restatement (tests/lr_rd_ref.py); the restated writers through the repo's decoders; the field decode, the refused values and the
behaviour without a device."""
import ctypes as C
import os

import pytest

import host_build
import lr_rd_ref as ref
import sgr_fit_ref
import wiener_fit_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "lr_rate_rule_host.cpp")


@pytest.fixture(scope="module")
def av1mi():
    return host_build.library()


@pytest.fixture(scope="module")
def cxx():
    return host_build.host_cxx(gcc=True)


def _grid(lo, hi):
    return list(range(lo, hi, 7)) + [hi]


def _expected():
    """what the program must print, from the restatement"""
    lines = ["CDF ok", "T16 %d %d %d %d %d" % tuple([ref.type_t16(True, t) for t in range(3)] + [ref.type_t16(False, t) for t in range(2)])]
    mn, mx = wiener_fit_ref.TAPS_MIN, wiener_fit_ref.TAPS_MAX
    for first in (0, 1):
        for c0 in ([0] if first else range(mn[0], mx[0] + 1)):
            for c1 in range(mn[1], mx[1] + 1):
                lens = [ref.wiener_lc(first, (c0, c1, c2), (c0, c1, c2)) for c2 in range(mn[2], mx[2] + 1)]
                lines.append(("WC %d :" % c1 if first else "WY %d %d :" % (c0, c1)) + "".join(" %d" % v for v in lens))
    for t in range(16):
        for x0 in _grid(sgr_fit_ref.XQD_MIN[0], sgr_fit_ref.XQD_MAX[0]):
            lines.append("S %d %d :" % (t, x0) + "".join(" %d" % ref.sgr_lc(t, x0, x1) for x1 in _grid(sgr_fit_ref.XQD_MIN[1], sgr_fit_ref.XQD_MAX[1])))
    for bd in (8, 10):
        for s in range(4):
            lines.append("LAM %d %d :" % (bd, s) + "".join(" %d" % ref.lam(q, bd, s) for q in range(1, 256)))
    lines.append("BOUND %d" % (ref.lam(255, 10, 3) * ref.b16(42, 30)))
    return lines


def test_type_costs_are_pinned():
    """the five T16 values of the issue, from av1_tables.h's default CDFs"""
    assert [ref.type_t16(True, t) for t in range(3)] == [30, 23, 29]
    assert [ref.type_t16(False, t) for t in range(2)] == [26, 12]
    assert ref.L(1) == 0 and ref.L(2) == 16 and ref.L(3) == 24 and ref.L(32768) == 240


def test_lambda_restated():
    """lambda0 = (13 q^2) >> 9 of the dc step, the four scales, never below 1; the 10-bit value is about 16 x the 8-bit one (the SSE scale)"""
    q8, q10 = ref.table("av1_dc_q8"), ref.table("av1_dc_q10")
    assert len(q8) == len(q10) == 256
    for bd, tab in ((8, q8), (10, q10)):
        for qi in (1, 60, 120, 180, 255):
            l0 = (13 * tab[qi] ** 2) >> 9
            assert [ref.lam(qi, bd, s) for s in range(4)] == [max(1, v) for v in (l0, l0 >> 1, l0 >> 2, l0 << 1)]
    assert ref.lam(1, 8, 2) == 1
    assert 12 <= ref.lam(120, 10, 0) / ref.lam(120, 8, 0) <= 20
    assert ref.lam(255, 10, 3) * ref.b16(42, 30) < 1 << 32
    assert [ref.qindex_of_cq(c) for c in (1, 30, 45, 61, 62, 63)] == [4, 120, 180, 244, 249, 255]


def test_restated_writers_through_the_decoders():
    """every length the restatement gives is the length the repo's decoders consume, and they read the coefficients back: Wiener units
    of luma and chroma against the tile-start reference and against another one, self-guided units of every set on the grid"""
    mn, mx, mid = wiener_fit_ref.TAPS_MIN, wiener_fit_ref.TAPS_MAX, wiener_fit_ref.TAPS_MID
    other = [[-5, 8, -17], [10, -23, 46]]
    for first in (0, 1):
        for c0 in ([0] if first else range(mn[0], mx[0] + 1)):
            for c1 in range(mn[1], mx[1] + 1, 3):
                for c2 in range(mn[2], mx[2] + 1, 5):
                    cv, ch = [c0, c1, c2], [0 if first else mx[0] + mn[0] - c0, mx[1] + mn[1] - c1, c2]
                    for rf in ([list(mid), list(mid)], other):
                        bits, n = ref.wiener_code(first, cv, ch, rf)
                        assert wiener_fit_ref.decode_wiener_unit(bits, n, first, rf) == (cv, ch, 0)
                    assert ref.wiener_lc(first, cv, ch) == ref.wiener_code(first, cv, ch)[1] <= 42
    for t in range(16):
        r0, _, r1, _ = sgr_fit_ref.SGR_PARAMS[t]
        for x0 in _grid(sgr_fit_ref.XQD_MIN[0], sgr_fit_ref.XQD_MAX[0]) if r0 else [0]:
            for x1 in _grid(sgr_fit_ref.XQD_MIN[1], sgr_fit_ref.XQD_MAX[1]):
                if not r1:
                    x1 = sgr_fit_ref.clamp(128 - x0, sgr_fit_ref.XQD_MIN[1], sgr_fit_ref.XQD_MAX[1])   # implied, not coded
                for rf in (sgr_fit_ref.XQD_MID, (17, -3)):
                    bits, n = ref.sgr_code(t, x0, x1, rf)
                    assert sgr_fit_ref.decode_sgr_unit(bits, n, rf) == (t, x0, x1, 0), (t, x0, x1, rf)
                assert 4 < ref.sgr_lc(t, x0, x1) <= 22
    assert [ref.fixed_lc(0, k) for k in range(7)][0] == 0 and all(ref.fixed_lc(s, k) > 0 for s in (0, 1) for k in range(1, 7))


def test_decide_rule():
    """the first minimum of J, absent candidates, the strict override, and lambda = 0 as the error's own order"""
    err = [100, 90, 90, 95, 80, 80, None] + [ref.ABSENT] * 16
    lc = [0, 20, 10, 10, 12, 12, 12] + [0] * 16
    assert ref.decide(err, lc, True, 0)[0] == 4                       # the first of the two minima of D
    assert ref.decide(err, lc, True, 1) == (4, 221, 1501)             # 1280 + 221 against 1600 + 30, 1440 + 183, ...
    assert ref.decide(err, lc, True, 3) == (0, 30, 1690)              # 1600 + 90 against 1280 + 663, 1440 + 549, ...
    assert ref.decide(err + [79], lc + [40], True, 0)[0] == 23
    assert ref.decide(err + [80], lc + [0], True, 0)[0] == 4          # strictly
    assert ref.decide(err + [ref.ABSENT], lc + [0], True, 0)[0] == 4
    assert ref.decide([50, 49, 60, 60], [0, 30, 0, 0], False, 1) == (0, 26, 826)   # 800 + 26 against 784 + 492
    assert ref.decide([50, 10, 60, 60], [0, 30, 0, 0], False, 1)[0] == 1


def test_standalone_program(cxx, tmp_path):
    out = host_build.run_program(cxx, SRC, tmp_path / "lr_rate_main")
    assert out.returncode == 0, out.stdout[-500:] + out.stderr
    got, want = out.stdout.splitlines(), _expected()
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a == b, (a[:200], b[:200])
    assert got[1] == "T16 30 23 29 26 12"


def test_standalone_program_under_sanitizers(cxx, tmp_path):
    """... and under AddressSanitizer and UndefinedBehaviorSanitizer (host code only).  Skipped only where an empty program does not
    build and run under the sanitizers - their runtimes are not installed"""
    out = host_build.run_program(cxx, SRC, tmp_path / "lr_rate_main_san", sanitized=True)
    assert out.returncode == 0, out.stdout[-500:] + out.stderr
    assert out.stdout.splitlines() == _expected()


# ---------------------------------------------------------------- the parameter
LOWS = [1, 2, 3, 4, 0x102, 0x104, 0x401, 0x403, 0x504, 0x1001, 0x2104, 0x2504, (1 << 9 << 16) | 0x104]


@pytest.mark.parametrize("s", [0, 1, 2, 3])
def test_field_layout(av1mi, s):
    """AV1MI_LR_RD(s) = 0xC000 | bit 0 of s in bit 9 | bit 1 of s in bit 11, in the mirror and through default_params"""
    want = 0xC000 | ((s & 1) << 9) | ((s & 2) << 10)
    assert av1mi.lr_rd_field(s) == ref.rd_field(s) == want and av1mi.LR_RD == 0xC000
    assert av1mi.lr_rd_scale_of(want | 0x104) == s and av1mi.lr_rd_scale_of(0x104) is None and av1mi.lr_rd_scale_of(0x4204) is None
    p = av1mi.default_params(640, 360, 8, enable_lr=4, lr_fit=True, lr_wiener_fit=True, lr_unit_shift=1, lr_rd=s)
    assert p.enable_lr == 0x1504 | want
    assert av1mi.default_params(640, 360, 8, enable_lr=3).enable_lr == 3


@pytest.mark.parametrize("s", [0, 1, 2, 3])
def test_mode_accepted_with_headers_unchanged(av1mi, s):
    """every combination of the other bits takes the mode, and the headers are those without it: the syntax does not change"""
    for v in LOWS:
        for kw in ({}, dict(bit_depth=10, film_grain=20, cdef_search=3, deblock=1)):
            kw = dict(kw)
            bd = kw.pop("bit_depth", 8)
            assert av1mi.write_headers(av1mi.default_params(640, 360, bd, enable_lr=v | av1mi.lr_rd_field(s), **kw)) == \
                av1mi.write_headers(av1mi.default_params(640, 360, bd, enable_lr=v, **kw)), hex(v)


PINNED_REFUSED = [0x204, 0x1204, 0x802, 0x1802, 0x1902, 0x5001, 0x9002]


@pytest.mark.parametrize("v", PINNED_REFUSED + [0x4001, 0x8001, 0x4A04, 0x8A04, 0x0A04, 0x4204, 0xC000, 0xC200, 0xC005, 0xC0FF, 0xF001, 0xC101, 0xC103,
                                                0xC001 | (1 << 16), 0xC401 | (1 << 16)])
def test_refused(av1mi, v):
    """bits 9, 11, 14 or 15 without both of 14 and 15 stay refused, as do the mode with a low byte of 0 or above 4, with both unit-size
    bits, and with a fit bit the low byte does not take"""
    with pytest.raises(av1mi.EncodeFailed) as e:
        av1mi.write_headers(av1mi.default_params(640, 360, 8, enable_lr=v))
    assert e.value.code == 1   # AV1MI_E_INVALID_ARG


def test_abi_unchanged(av1mi):
    assert av1mi._lib.av1mi_abi_version() == 8 == av1mi.ABI_VERSION
    sizes = av1mi.struct_sizes()
    assert sizes == av1mi.mirror_sizes()
    assert sizes[:8] == [144, 184, 120, 16, 32, 40, 184, 64], sizes
    for name in ("av1mi_lr_rd_result", "av1mi_lr_rd_units"):
        assert name in av1mi.ABI_SYMBOLS and hasattr(av1mi._lib, name)


def test_without_a_context(av1mi):
    """the result calls refuse a null context"""
    assert av1mi._lib.av1mi_lr_rd_units(None) == 0
    ch = (C.c_int8 * 4)()
    assert av1mi._lib.av1mi_lr_rd_result(None, 1, ch, None, None) == 1   # AV1MI_E_INVALID_ARG


def test_without_a_device(av1mi):
    """without a HIP device a context with the mode is refused as ever: no quiet fall-back"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(av1mi.EncodeFailed) as ei:
        av1mi.Context(0)
    assert ei.value.code == av1mi.E_NO_DEVICE
