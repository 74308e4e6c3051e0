"""CPU tests of restoration units of 128x128 and 256x256 luma samples (include/av1mi.h: AV1MI_LR_UNIT_128 / _256, enable_lr bits 12-13;
DESIGN.md §3 item 9f): the geometry header (av1-base_amd/csrc/lr_geometry.h, compiled for the host) against tests/lr_ref.py and
tests/lr_unit_ref.py for every even size 8 .. 1200 and every shift, its stand-alone program plain and under the sanitizers, the two fit
rules on sums at the bound of a 256-unit, and the parameter's range, the frame header's bits and the ABI."""
import ctypes as C
import os
import random

import numpy as np
import pytest

import host_build
import lr_ref
import lr_unit_ref as uref
import sgr_fit_ref
import wiener_fit_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "host")
SRC = os.path.join(HOST, "lr_geometry_host.cpp")
SIZES = range(8, 1201, 2)


@pytest.fixture(scope="module")
def av1mi():
    return host_build.library()


@pytest.fixture(scope="module")
def cxx():
    return host_build.host_cxx(gcc=True)


def _shared(cxx, tmp_path_factory, name):
    return C.CDLL(host_build.build_shared(cxx, os.path.join(HOST, name + ".cpp"), tmp_path_factory.mktemp(name) / ("lib%s.so" % name)))


@pytest.fixture(scope="module")
def geo(cxx, tmp_path_factory):
    lib = _shared(cxx, tmp_path_factory, "lr_geometry_host")
    lib.geo_bounds.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    return lib


# ---------------------------------------------------------------- the geometry against the restatement
@pytest.mark.parametrize("shift", [0, 1, 2])
def test_counts_and_bounds_are_the_restatements(geo, shift):
    """counts against lr_ref.count_units, bounds of both plane kinds against lr_unit_ref.unit_bounds (at shift 0: lr_ref.unit_bounds)"""
    out = np.zeros(2 * 32, dtype=np.int32)
    for size in SIZES:
        n = geo.geo_count(size, shift)
        assert n == lr_ref.count_units(size, 64 << shift)
        for sub in (0, 1):
            plane = (size + sub) >> sub
            assert n == lr_ref.count_units(plane, (64 << shift) >> sub)   # the planes share the grid
            rows, cols = uref.unit_bounds(plane, plane, sub, shift)
            if shift == 0:
                assert (rows, cols) == lr_ref.unit_bounds(plane, plane, sub)
            for want, is_cols in ((rows, 0), (cols, 1)):
                geo.geo_bounds(size, shift, sub, is_cols, out.ctypes.data)
                assert [(int(out[2 * u]), int(out[2 * u + 1])) for u in range(n)] == want, (size, shift, sub, is_cols)


@pytest.mark.parametrize("shift", [0, 1, 2])
def test_cells_and_superblocks(geo, shift):
    """every cell of the 64-grid lies inside exactly one unit of the restatement's bounds, the one the header's map names; shift 0
    reproduces the grid of 64x64 units; every unit is read with one superblock that exists, and no superblock reads two"""
    for size in SIZES:
        cells, units = max((size + 32) // 64, 1), geo.geo_count(size, shift)
        if shift == 0:
            assert units == cells
        for sub in (0, 1):
            plane = (size + sub) >> sub
            crow, ccol = lr_ref.unit_bounds(plane, plane, sub)
            urow, ucol = uref.unit_bounds(plane, plane, sub, shift)
            assert len(crow) == cells
            for c in range(cells):
                for cb, ub in ((crow, urow), (ccol, ucol)):
                    holders = [u for u, (a, b) in enumerate(ub) if a <= cb[c][0] and cb[c][1] <= b]
                    assert holders == [geo.geo_unit_of_cell(c, units, shift)], (size, shift, sub, c)
            for u in range(units):
                assert urow[u][0] == crow[geo.geo_first_cell(u, shift)][0] and ucol[u][0] == ccol[geo.geo_first_cell(u, shift)][0]
        sbs = (((size + 7) & ~7) + 63) // 64
        coded = [geo.geo_unit_sb(u, shift) for u in range(units)]
        assert len(set(coded)) == units and max(coded) < sbs, (size, shift)
        assert [geo.geo_sb_unit(sb, units, shift) for sb in coded] == list(range(units))
        assert sum(geo.geo_sb_unit(sb, units, shift) >= 0 for sb in range(sbs)) == units


def test_264_rows_make_five_superblock_rows_and_two_units_of_128(geo):
    assert geo.geo_count(264, 1) == 2 and [geo.geo_sb_unit(sb, 2, 1) for sb in range(5)] == [0, -1, 1, -1, -1]
    assert geo.geo_count(328, 1) == 3 and geo.geo_count(248, 1) == 2 and geo.geo_count(328, 2) == 1   # 2x3 units of 128, one of 256


# ---------------------------------------------------------------- the stand-alone program
def test_standalone_program(cxx, tmp_path):
    out = host_build.run_program(cxx, SRC, tmp_path / "geo_main", defines=["LR_GEOMETRY_MAIN"])
    assert out.returncode == 0 and " 0 failures" in out.stdout, out.stdout + out.stderr


def test_standalone_program_under_sanitizers(cxx, tmp_path):
    """... and under AddressSanitizer and UndefinedBehaviorSanitizer (host code only).  Skipped only where an empty program does not
    build and run under the sanitizers - their runtimes are not installed"""
    out = host_build.run_program(cxx, SRC, tmp_path / "geo_main_san", defines=["LR_GEOMETRY_MAIN"], sanitized=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert " 0 failures" in out.stdout


# ---------------------------------------------------------------- the rules on a 256-unit's sums
SAMPLES = 383 * 391   # the largest unit: a last unit of 256 is at most 1.5 x 256 - 1 wide and 1.5 x 256 + 7 tall


def test_self_guided_rule_carries_a_256_units_sums(cxx, tmp_path_factory):
    """the five sums of 383 x 391 samples of extreme 10-bit terms (|f0|, |f1|, |s| <= 2^14: |sum| < 2^46), random signs and magnitudes
    down from the bound: the C++ rule equals the restatement, whose k = bitlength - 26 normalisation takes them"""
    lib = _shared(cxx, tmp_path_factory, "lr_fit_rule_host")
    lib.fit_solve.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    top = SAMPLES * (1 << 14) ** 2
    assert 1 << 45 < top < 1 << 46
    rng = random.Random(256)
    probs = []
    for it in range(4000):
        mag = top >> rng.choice([0, 0, 1, 3, 8, 19])
        if it % 3 == 0:      # sums of squares that are what they say: H00, H11 > 0, |H01| <= sqrt(H00 H11)
            h00, h11 = rng.randint(mag // 2, mag), rng.randint(mag // 2, mag)
            h01 = rng.randint(-int((h00 * h11) ** 0.5), int((h00 * h11) ** 0.5))
            s = [h00, h01, h11, rng.randint(-mag, mag), rng.randint(-mag, mag)]
        elif it % 3 == 1:    # every entry at the magnitude, any sign
            s = [rng.choice([-mag, mag]) for _ in range(5)]
        else:
            s = [rng.randint(-mag, mag) for _ in range(5)]
        probs.append((it % 16, s))
    n = len(probs)
    t = np.array([p[0] for p in probs], dtype=np.int32)
    sums = np.array([p[1] for p in probs], dtype=np.int64)
    w, present = np.zeros((n, 2), dtype=np.int32), np.zeros(n, dtype=np.int32)
    lib.fit_solve(t.ctypes.data, sums.ctypes.data, n, w.ctypes.data, present.ctypes.data)
    seen = 0
    for i, (ti, s) in enumerate(probs):
        want = sgr_fit_ref.solve(ti, s)
        assert (tuple(int(v) for v in w[i]) if present[i] else None) == want, (ti, s)
        seen += want is not None
    assert seen > n // 4


def test_wiener_rule_carries_a_256_units_sums(cxx, tmp_path_factory):
    """the 27 sums of 383 x 391 samples with |D| <= 2046 and |e| <= 1023 (|sum| < 2^40), random signs: the C++ rule equals the restatement,
    which asserts that every intermediate stays inside 63 bits"""
    lib = _shared(cxx, tmp_path_factory, "wiener_fit_rule_host")
    lib.wf_fit.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    top = SAMPLES * 2046 * 2046
    assert 1 << 39 < top < 1 << 40
    rng = random.Random(257)
    diag = (0, 3, 5, 6, 9, 11)
    probs = []
    for it in range(4000):
        mag = top >> rng.choice([0, 0, 1, 4, 12])
        if it % 2:
            s = [rng.choice([-mag, mag]) for _ in range(wiener_fit_ref.N_SUMS)]
        else:
            s = [rng.randint(-mag, mag) for _ in range(wiener_fit_ref.N_SUMS)]
        if it % 4 < 3:
            for k in diag:   # sums of squares on the diagonals, at the magnitude
                s[k] = mag - rng.randrange(0, mag // 8 + 1)
        if it % 4 == 2:
            for k in range(wiener_fit_ref.N_SUMS):   # ... and diagonally dominant, so that solutions exist
                if k not in diag:
                    s[k] = s[k] >> rng.choice([3, 5, 9])
        probs.append((s, it & 1))
    n = len(probs)
    sums = np.array([p[0] for p in probs], dtype=np.int64)
    first = np.array([p[1] for p in probs], dtype=np.int32)
    taps, present, flags = np.zeros((n, 6), dtype=np.int32), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    lib.wf_fit(sums.ctypes.data, first.ctypes.data, n, taps.ctypes.data, present.ctypes.data, flags.ctypes.data)
    seen = 0
    for i, (s, f) in enumerate(probs):
        want = wiener_fit_ref.fit(s, f)
        got = ([int(v) for v in taps[i, :3]], [int(v) for v in taps[i, 3:]]) if present[i] else None
        assert got == want, (s, f, got, want)
        seen += want is not None
    assert seen > n // 8


# ---------------------------------------------------------------- the parameter
@pytest.mark.parametrize("v", [0x1001, 0x1002, 0x1003, 0x1004, 0x2001, 0x2004, 0x1102, 0x2104, 0x1401, 0x2403, 0x1504, 0x2504, 0x2104 | (1 << 25)])
def test_unit_size_accepted(av1mi, v):
    """this is what the library before the feature refuses"""
    av1mi.write_headers(av1mi.default_params(640, 360, 8, enable_lr=v))


@pytest.mark.parametrize("v", [0x3001, 0x3504, 0x1000, 0x2000, 0x3000, 0x1005, 0x1101, 0x2103, 0x1100, 0x2400, 0x1800 | 2, 0x1200 | 4, 0x5001, 0x9002, 0x1001 | (1 << 16)])
def test_unit_size_refused(av1mi, v):
    """both bits, a bit with a low byte of 0, and a unit size on a value that is refused without it"""
    with pytest.raises(av1mi.EncodeFailed) as e:
        av1mi.write_headers(av1mi.default_params(640, 360, 8, enable_lr=v))
    assert e.value.code == 1   # AV1MI_E_INVALID_ARG


def _bits(data, n):
    return "".join("%d" % (data[i >> 3] >> (7 - (i & 7)) & 1) for i in range(n))


@pytest.mark.parametrize("kw", [{}, dict(film_grain=20, cdef_search=3, deblock=1), dict(width=202, height=122, bit_depth=8, cdf_update=0)])
def test_frame_header_grows_by_lr_unit_extra_shift_alone(av1mi, kw):
    """lr_params: lr_unit_shift = (shift > 0) and, when it is 1, lr_unit_extra_shift = (shift == 2), before lr_uv_shift; the sequence
    header does not change, the rest of the frame header follows one bit later, and the fits do not touch the header"""
    kw = dict(kw)
    w, h, bd = kw.pop("width", 1920), kw.pop("height", 1080), kw.pop("bit_depth", 10)
    hdr = lambda **k: av1mi.write_headers(av1mi.default_params(w, h, bd, **dict(kw, **k)))
    for lr in (1, 2, 3, 4):
        seq, frame, n = hdr(enable_lr=lr)
        plain = _bits(frame, n)
        one = hdr(enable_lr=lr, lr_unit_shift=1)
        at = next(i for i in range(n) if plain[i] != _bits(one[1], one[2])[i])   # lr_unit_shift: the first bit that differs
        t = "01" if lr in (2, 4) else "10"   # lr_type: RESTORE_SWITCHABLE / RESTORE_WIENER, then U and V
        assert plain[at - 6:at + 1] == t + (t + t if lr >= 3 else "0000") + "0"
        if lr >= 3:
            assert plain[at + 1] == "1"   # lr_uv_shift
        for shift, field in ((1, "10"), (2, "11")):
            s2, f2, n2 = hdr(enable_lr=lr, lr_unit_shift=shift)
            assert s2 == seq and n2 == n + 1
            assert _bits(f2, n2) == plain[:at] + field + plain[at + 1:], (lr, shift)
            if lr in (2, 4):
                assert hdr(enable_lr=lr, lr_unit_shift=shift, lr_fit=True, lr_wiener_fit=True) == (s2, f2, n2)
    assert av1mi.default_params(w, h, bd, enable_lr=3, lr_unit_shift=1).enable_lr == 0x1003 == 3 | av1mi.LR_UNIT_128
    assert av1mi.default_params(w, h, bd, enable_lr=4, lr_fit=True, lr_wiener_fit=True, lr_unit_shift=2).enable_lr == 0x2504
    assert av1mi.lr_unit_shift_of(0x2504) == 2 and av1mi.lr_unit_grid(328, 248, 1) == (2, 3) and av1mi.lr_unit_grid(88, 72, 2) == (1, 1)


def test_abi_unchanged(av1mi):
    assert av1mi._lib.av1mi_abi_version() == 8 == av1mi.ABI_VERSION
    sizes = av1mi.struct_sizes()
    assert sizes == av1mi.mirror_sizes()
    assert sizes[:8] == [144, 184, 120, 16, 32, 40, 184, 64], sizes   # the structures' sizes before the feature
    header = open(os.path.join(ROOT, "include", "av1mi.h")).read()
    assert "#define AV1MI_LR_UNIT_128 0x1000u" in header and "#define AV1MI_LR_UNIT_256 0x2000u" in header
