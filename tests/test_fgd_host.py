"""CPU tests of the film-grain denoiser's interface and rule (include/av1mi.h: av1mi_params.film_grain bits 8 and 10,
av1mi_film_grain_denoise): how the field packs and what is refused, the ABI staying what it was, the rule header
(av1-base_amd/csrc/fg_denoise_rule.h) compiled for the host - a stand-alone program, run plain and under the sanitizers - against the numpy
restatement (tests/fgd_ref.py) on inputs no clip reaches, the consequences of the rule on the restatement, and what the restatement gains
on a noisy clip whose clean original is known."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import edge_content
import fg_ref
import fgd_ref
import host_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [os.path.join(ROOT, "tests", "host", "fgd_rule_host.cpp")]


@pytest.fixture(scope="module")
def av1mi():
    return host_build.library()


# ---------------------------------------------------------------- packing
@pytest.mark.parametrize("n", [1, 20, 50])
def test_packed_field_accepted(av1mi, n):
    p = av1mi.default_params(640, 360, 8, film_grain_denoise=n)
    assert p.film_grain == n | 0x100 | 0x400 == av1mi.film_grain_denoise(n) == fgd_ref.field(n)
    assert av1mi.film_grain_denoised(p.film_grain) == 1 and av1mi.film_grain_estimated(p.film_grain) == 1 and av1mi.film_grain_level_of(p.film_grain) == n
    assert av1mi.film_grain_denoised(av1mi.film_grain_estimate(n)) == 0 and av1mi.FILM_GRAIN_DENOISE == 0x400
    assert fgd_ref.field_decode(p.film_grain) == (True, n, True, True)
    # the headers are the estimate mode's: the denoiser signals nothing
    assert av1mi.write_headers(p) == av1mi.write_headers(av1mi.default_params(640, 360, 8, film_grain_estimate=n))
    av1mi.write_headers(av1mi.default_params(640, 360, 8, film_grain=n | 0x500))   # the raw field
    assert av1mi.default_params(640, 360, 8, film_grain=n, film_grain_denoise=True).film_grain == n | 0x500
    assert av1mi.default_params(640, 360, 8, film_grain=n, film_grain_denoise=False).film_grain == n
    assert av1mi.default_params(640, 360, 8).film_grain == 0   # the default stays off


@pytest.mark.parametrize("v", [0x400 | 20, 0x400, 0x500, 0x500 | 51, 0x500 | 255, 0x700 | 20, 0x600 | 20, 0x200 | 20, 0x300 | 20, 1 << 11 | 0x500 | 20,
                               1 << 16 | 0x500 | 20, 1 << 31 | 0x500 | 20, 1 << 31 | 0x400 | 20])
def test_packed_field_refused(av1mi, v):
    assert not fgd_ref.field_decode(v)[0]
    with pytest.raises(av1mi.EncodeFailed) as e:
        av1mi.write_headers(av1mi.default_params(640, 360, 8, film_grain=v))
    assert e.value.code == 1   # AV1MI_E_INVALID_ARG


def test_abi_unchanged_and_symbol_exported(av1mi):
    assert C.sizeof(av1mi.Params) == 36 * 4 and av1mi.struct_sizes() == av1mi.mirror_sizes()
    assert av1mi.ABI_VERSION == int(av1mi._lib.av1mi_abi_version()) == 8
    hdr = open(os.path.join(ROOT, "include", "av1mi.h")).read()
    shim = open(os.path.join(ROOT, "integration", "mi355x.rs")).read()
    sym = "av1mi_film_grain_denoise"
    assert sym in av1mi.ABI_SYMBOLS
    assert getattr(av1mi._lib, sym) is not None   # exported
    assert re.search(r"\bint\s+%s\s*\(" % sym, hdr)
    assert "fn %s(" % sym in shim
    assert re.search(r"#define\s+AV1MI_FILM_GRAIN_DENOISE\(", hdr) and re.search(r"#define\s+AV1MI_FILM_GRAIN_DENOISED\(", hdr)
    assert "#define AV1MI_ABI_VERSION 8" in hdr
    assert "fn film_grain_denoise(" in shim and "fn film_grain_denoised(" in shim and "36 * 4" in shim


def test_entry_point_checks_its_arguments_first(av1mi):
    """no context: AV1MI_E_INVALID_ARG before anything touches a device"""
    p = av1mi.default_params(64, 64, 8, film_grain_denoise=20)
    assert av1mi._lib.av1mi_film_grain_denoise(None, C.byref(p), None, 1, 0, None, None, None) == 1


# ---------------------------------------------------------------- the stand-alone program: the rule
FALLING = [255, 200, 131, 130, 77, 3, 1, 0]   # negative steps: the LUT's shift must be arithmetic


def _tables():
    rng = np.random.default_rng(21)
    return [[0] * 8, [255] * 8, FALLING, FALLING[::-1], [0, 255, 0, 255, 0, 255, 0, 255], [0, 0, 0, 37, 0, 0, 0, 0]] + \
        [[int(v) for v in rng.integers(0, 256, 8)] for _ in range(6)]


def _index_cases():
    return [(bd, y0, y1, lut) for bd in (8, 10) for y0, y1 in ((0, 0), ((1 << bd) - 1, (1 << bd) - 1), (0, (1 << bd) - 1), (5, 6), (130 << (bd - 8), 131 << (bd - 8)))
            for lut in (0, 1, 7, 8, 24, 100, 255)]


def _windows():
    """(T, centre, the 25 samples): random windows, T = 0, 1 and 64, samples at 0 and at the maximum"""
    rng = np.random.default_rng(22)
    out = []
    for mx in (255, 1023):
        for T in (0, 1, 2, 7, 16, 63, 64):
            for _ in range(4):
                c = int(rng.integers(0, mx + 1))
                x = np.clip(c + rng.integers(-T - 3, T + 4, 25), 0, mx)
                x[12] = c
                out.append((T, c, [int(v) for v in x]))
            for c, fill in ((0, 0), (mx, mx), (0, mx), (mx, 0), (mx, mx - 1), (0, 1)):
                x = [fill] * 25
                x[12] = c
                out.append((T, c, x))
    return out


def _planes():
    """(bd, w, h, values, plane): the flat plane of 1023 with value 255 - the largest numerator -, random planes under random and falling
    tables, planes smaller than the window"""
    rng = np.random.default_rng(23)
    out = [(10, 7, 6, [255] * 8, np.full((6, 7), 1023)), (8, 7, 6, [255] * 8, np.full((6, 7), 255)), (10, 1, 1, [255] * 8, np.full((1, 1), 512)),
           (8, 2, 3, [255] * 8, rng.integers(100, 110, (3, 2))), (10, 4, 2, FALLING, rng.integers(0, 1024, (2, 4)))]
    for bd in (8, 10):
        sc = 1 << (bd - 8)
        for tab in (FALLING, [64] * 8, [int(v) for v in rng.integers(0, 256, 8)]):
            base = np.add.outer(np.arange(9) * 7, np.arange(13) * 19) * sc
            out.append((bd, 13, 9, tab, np.clip(base + np.rint(rng.normal(0, 2.0 * sc, (9, 13))).astype(np.int64), 0, (1 << bd) - 1)))
    return out


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """(the case lines, the lines the plain program prints for them, the path of the case file)"""
    lines = ["L " + " ".join(str(v) for v in t) for t in _tables()]
    lines += ["X %d %d %d %d" % c for c in _index_cases()]
    lines += ["W %d %d %s" % (T, c, " ".join(str(v) for v in x)) for T, c, x in _windows()]
    lines += ["P %d %d %d %s %s" % (bd, w, h, " ".join(str(v) for v in tab), " ".join(str(int(v)) for v in np.asarray(x).ravel())) for bd, w, h, tab, x in _planes()]
    d = tmp_path_factory.mktemp("fgd_rule")
    path = d / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    out = host_build.run_program(host_build.host_cxx(gcc=True), SOURCES, d / "fgd_rule_host", args=[path])
    assert out.returncode == 0, out.stderr[-2000:]
    got = out.stdout.split("\n")[:-1]
    assert len(got) == len(lines)
    return lines, got, path


def _of(program, kind):
    lines, got, _ = program
    return [[int(v) for v in g.split()] for ln, g in zip(lines, got) if ln[0] == kind]


def test_rule_lut_equals_the_restatement(program):
    outs = _of(program, "L")
    for t, g in zip(_tables(), outs):
        assert g == [int(v) for v in fgd_ref.lut_of(t)], t
    lut = fgd_ref.lut_of(FALLING)
    # the points themselves, the flat ends, and a negative step rounded like a positive one: halfway goes up
    assert [int(lut[16 + 32 * k]) for k in range(8)] == FALLING and int(lut[0]) == int(lut[15]) == 255 and int(lut[240]) == int(lut[255]) == 0
    assert int(lut[16 + 32 * 2 + 16]) == 131 + ((16 * (130 - 131) + 16) >> 5) == 131 and int(lut[16 + 32 * 2 + 17]) == 130
    assert (np.diff(lut) <= 0).all()


def test_rule_index_and_reach(program):
    for (bd, y0, y1, lut), g in zip(_index_cases(), _of(program, "X")):
        assert g == [y0 >> (bd - 8), ((y0 + y1 + 1) >> 1) >> (bd - 8), int(fgd_ref.reach_of(lut, bd))], (bd, y0, y1, lut)
    assert int(fgd_ref.reach_of(255, 8)) == 16 and int(fgd_ref.reach_of(255, 10)) == 64 and int(fgd_ref.reach_of(7, 8)) == 0 and int(fgd_ref.reach_of(8, 8)) == 1


def test_rule_windows_equal_the_restatement(program):
    seen_copy = seen_moved = 0
    for (T, c, x), (num, den, out) in zip(_windows(), _of(program, "W")):
        xs = np.array(x, dtype=np.int64)
        wt = np.maximum(0, T - np.abs(xs - c))
        assert (num, den) == (int((wt * xs).sum()), int(wt.sum())), (T, c, x)
        want = (num + den // 2) // den if den else c
        assert out == want and abs(out - c) <= max(0, T - 1), (T, c, x)
        if T <= 1:
            assert out == c
        seen_copy += out == c
        seen_moved += out != c
    assert seen_copy and seen_moved > 20


def test_rule_planes_equal_the_restatement(program):
    for (bd, w, h, tab, x), g in zip(_planes(), _of(program, "P")):
        x = np.asarray(x, dtype=np.int64)
        T = fgd_ref.reach_of(fgd_ref.lut_of(tab)[x >> (bd - 8)], bd)
        want = fgd_ref.filter_plane(x, T)
        assert g == [int(v) for v in want.ravel()], (bd, w, h, tab)
    # the largest numerator: 25 samples of 1023 weighing 64 each, below 2^21
    assert 25 * 64 * 1023 < 1 << 21


def test_standalone_program_under_sanitizers(program, tmp_path):
    """the same cases once under AddressSanitizer and UndefinedBehaviorSanitizer (host code only, a program of its own).  Skipped only where
    an empty program does not build and run under the sanitizers - their runtimes are not installed"""
    lines, got, path = program
    out = host_build.run_program(host_build.host_cxx(gcc=True), SOURCES, tmp_path / "fgd_rule_host_san", args=[path], sanitized=True)
    assert out.returncode == 0, out.stdout[-500:] + out.stderr[-2000:]
    assert out.stdout.split("\n")[:-1] == got


# ---------------------------------------------------------------- what follows from the rule (the restatement alone)
@pytest.mark.parametrize("bd", [8, 10])
def test_consequences_of_the_rule(bd):
    rng = np.random.default_rng(24 + bd)
    w, h, n, mx = 40, 24, 2, (1 << bd) - 1
    raw = fg_ref.two_level_clip(w, h, bd, n)
    frames = fg_ref.split(raw, w, h, bd, n)
    assert fgd_ref.denoise(raw, w, h, bd, n, np.zeros((3, 8), dtype=np.uint8)) == raw                       # a zero table is the identity
    table = rng.integers(0, 256, (3, 8))
    out = fgd_ref.denoise_frames(frames, table, bd)
    for fr, fo in zip(frames, out):
        for x, o, T in zip(fr, fo, fgd_ref.reaches(fr[0], table, bd)):
            assert (np.abs(o - x) <= np.maximum(0, T - 1)).all()                                             # no sample moves by T or more
    flat = fg_ref.join([[np.full((h, w), 517 >> (10 - bd)), np.full((h // 2, w // 2), 3), np.full((h // 2, w // 2), mx)]], bd)
    assert fgd_ref.denoise(flat, w, h, bd, 1, np.full((3, 8), 255)) == flat                                  # a constant plane is unchanged
    checker = fg_ref.checker_clip(w, h, bd, 1)
    assert fgd_ref.denoise(checker, w, h, bd, 1, np.full((3, 8), 255)) == checker                            # neighbours equal or a full amplitude away: unchanged
    x = np.full((9, 9), 100 << (bd - 8))
    x[4, 4] += 64                                                                                            # every neighbour differs by T or more
    assert np.array_equal(fgd_ref.filter_plane(x, np.full((9, 9), int(fgd_ref.reach_of(255, bd))))[4, 4], x[4, 4])
    # the edge extension replicates the denoised edge
    padded = fgd_ref.pad(fgd_ref.denoise_frames(fg_ref.split(fg_ref.two_level_clip(10, 14, bd, 1), 10, 14, bd, 1), table, bd), 10, 14)
    assert padded[0][0].shape == (16, 16) and padded[0][1].shape == (8, 8) and (padded[0][0][:, 9:] == padded[0][0][:, 9:10]).all() and \
        (padded[0][2][7:, :] == padded[0][2][6:7, :]).all()


# ---------------------------------------------------------------- what the filter gains (the restatement alone)
GAIN_SIZE = (136, 72, 3)
N = 50   # the ceiling: 100 luma, 50 chroma - above 64 sigma of the clip's noise in every plane and half


@pytest.mark.parametrize("bd", [8, 10])
def test_restatement_gains_three_decibels(bd):
    """on the ramps with an edge and a bar and noise of sigma 1.0 / 1.4 (luma halves), 0.5 / 0.7 (chroma), with the restatement's own estimate
    of the noisy clip as the table: both occupied luma bins populated, no value at the ceiling, and the denoised clip at least 3 dB nearer the
    clean clip than the noisy one.  Measured: +5.41 dB at 8 bits (46.99 -> 52.39), +8.01 dB at 10 bits (47.59 -> 55.60)"""
    w, h, n = GAIN_SIZE
    clean, noisy = fgd_ref.ramp_clip(w, h, bd, n)
    table, counts, _ = fg_ref.estimate(noisy, w, h, bd, n, N)
    cy, cc = fg_ref.ceilings(N)
    assert counts[0][2] >= 16 and counts[0][4] >= 16 and (table[0] < cy).all() and (table[1:] < cc).all() and (table > 0).all(), (table.tolist(), counts.tolist())
    den = fgd_ref.denoise(noisy, w, h, bd, n, table)
    before, after = fgd_ref.psnr(noisy, clean, bd), fgd_ref.psnr(den, clean, bd)
    print("%dx%dx%d bits: noisy %.2f dB, denoised %.2f dB, gain %.2f dB, table %s" % (w, h, bd, before, after, after - before, table.tolist()))
    assert after - before >= 3.0, (before, after)


def test_oracle_codes_the_denoised_frames_in_fewer_bytes(oracle):
    """what tests/test_fgd.py's byte comparison relies on: the oracle's key-frame encodes of the noisy clip and of its restatement-denoised
    frames, at CQ 20, are ordered the way the encoder's must be"""
    w, h, n = GAIN_SIZE
    _, noisy = fgd_ref.ramp_clip(w, h, 8, n)
    table, _, _ = fg_ref.estimate(noisy, w, h, 8, n, N)
    case = dict(w=w, h=h, bd=8, n=n, params=dict(keyint=1, cq_level=20))
    size = {}
    for name, raw in (("noisy", noisy), ("denoised", fgd_ref.denoise(noisy, w, h, 8, n, table))):
        tus, _, _ = edge_content.oracle_encode(oracle, case, fg_ref.split(raw, w, h, 8, n))
        size[name] = sum(len(t) for t in tus)
    print("oracle bytes: noisy %d, denoised %d" % (size["noisy"], size["denoised"]))
    assert size["denoised"] < size["noisy"], size
