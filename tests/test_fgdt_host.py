"""CPU tests of the film-grain denoiser's temporal term (include/av1mi.h: av1mi_params.film_grain bits 14 and 15,
av1mi_film_grain_denoise_temporal): how the field packs and what is refused, the ABI staying what it was, the rule
header (av1-base_amd/csrc/fg_denoise_rule.h) compiled for the host - a stand-alone program, run plain and under the sanitizers - against the
numpy restatement (tests/fgdt_ref.py) on inputs no clip reaches, the consequences of the rule on the restatement, what the restatement
gains over the spatial filter on clips whose clean original is known, and the order in which the oracle codes the two outputs."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import edge_content
import fg_ref
import fgd_ref
import fgdt_ref
import host_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [os.path.join(ROOT, "tests", "host", "fgdt_rule_host.cpp")]
NONE = fgdt_ref.NONE


@pytest.fixture(scope="module")
def av1mi():
    return host_build.library()


# ---------------------------------------------------------------- packing
@pytest.mark.parametrize("n,span,lag", [(1, 1, 0), (20, 1, 0), (20, 2, 0), (50, 2, 3), (20, 1, 1)])
def test_packed_field_accepted(av1mi, n, span, lag):
    v = n | 0x100 | 0x400 | 0xC000 | (0x200 if span == 2 else 0)
    assert av1mi.film_grain_denoise_temporal(n, span) == fgdt_ref.field(n, span) == v
    assert av1mi.film_grain_denoise_span(v) == span and av1mi.film_grain_denoise_span(av1mi.film_grain_denoise(n)) == 0
    assert av1mi.film_grain_denoised(v) == 1 and av1mi.film_grain_estimated(v) == 1 and av1mi.film_grain_level_of(v) == n
    p = av1mi.default_params(640, 360, 8, film_grain_denoise=n, film_grain_temporal=span, film_grain_ar=lag)
    assert p.film_grain == v | av1mi.film_grain_ar(lag) and av1mi.film_grain_ar_lag(p.film_grain) == lag
    assert fgdt_ref.field_decode(p.film_grain) == (True, n, True, True, span, lag)
    # the headers are the estimate mode's: the temporal term signals nothing
    assert av1mi.write_headers(p) == av1mi.write_headers(av1mi.default_params(640, 360, 8, film_grain_estimate=n, film_grain_ar=lag))
    assert av1mi.default_params(640, 360, 8, film_grain_denoise=n).film_grain == n | 0x500   # the default stays spatial


def test_the_smallest_temporal_field_is_accepted(av1mi):
    """0xC500 | 20: refused before the temporal term existed"""
    av1mi.write_headers(av1mi.default_params(640, 360, 8, film_grain=0xC500 | 20))
    av1mi.write_headers(av1mi.default_params(640, 360, 8, film_grain=0xC700 | 20))


@pytest.mark.parametrize("v", [0x4000 | 0x500 | 20, 0x8000 | 0x500 | 20, 0x4000 | 20, 0x8000 | 20, 0xC000 | 20, 0xC000 | 0x100 | 20, 0xC000 | 0x300 | 20,
                               0xC000 | 0x400 | 20, 0x200 | 0x500 | 20, 0x200 | 0x100 | 20, 0x4000 | 0x700 | 20, 0x8000 | 0x700 | 20, 0xC500 | 0x800 | 20,
                               0xC500 | 1 << 16 | 20, 0xC500 | 1 << 31 | 20, 0xC500, 0xC500 | 51, 0xC700 | 255])
def test_packed_field_refused(av1mi, v):
    assert not fgdt_ref.field_decode(v)[0]
    with pytest.raises(av1mi.EncodeFailed) as e:
        av1mi.write_headers(av1mi.default_params(640, 360, 8, film_grain=v))
    assert e.value.code == 1   # AV1MI_E_INVALID_ARG


def test_abi_unchanged_and_symbol_exported(av1mi):
    assert C.sizeof(av1mi.Params) == 36 * 4 and av1mi.struct_sizes() == av1mi.mirror_sizes()
    assert av1mi.ABI_VERSION == int(av1mi._lib.av1mi_abi_version()) == 8
    hdr = open(os.path.join(ROOT, "include", "av1mi.h")).read()
    shim = open(os.path.join(ROOT, "integration", "mi355x.rs")).read()
    sym = "av1mi_film_grain_denoise_temporal"
    assert sym in av1mi.ABI_SYMBOLS
    assert getattr(av1mi._lib, sym) is not None   # exported
    assert re.search(r"\bint\s+%s\s*\(" % sym, hdr)
    assert "fn %s(" % sym in shim
    assert re.search(r"#define\s+AV1MI_FILM_GRAIN_DENOISE_TEMPORAL\(", hdr) and re.search(r"#define\s+AV1MI_FILM_GRAIN_DENOISE_SPAN\(", hdr)
    assert "#define AV1MI_ABI_VERSION 8" in hdr
    assert "fn film_grain_denoise_temporal(" in shim and "fn film_grain_denoise_span(" in shim and "36 * 4" in shim


def test_entry_point_checks_its_arguments_first(av1mi):
    """no context: AV1MI_E_INVALID_ARG before anything touches a device"""
    p = av1mi.default_params(64, 64, 8, film_grain_denoise=20, film_grain_temporal=1)
    assert av1mi._lib.av1mi_film_grain_denoise_temporal(None, C.byref(p), None, 1, 0, None, None, None, None, None) == 1


# ---------------------------------------------------------------- the stand-alone program: the rule
def key_of(dy, dx, R, cost=0):
    return (cost << 11) | ((dy + R) * (2 * R + 1) + dx + R)


def _fields():
    return [0, 20, 0x500 | 20, 0xC500 | 20, 0xC700 | 20, 0x4500 | 20, 0x8500 | 20, 0x4700 | 20, 0x700 | 20, 0xF500 | 20, 0xFFFFFFFF]


def _slots():
    return [(f, s, span, n) for n in (1, 2, 3, 5) for span in (1, 2) for f in range(n) for s in range(4)]


def _filters():
    """(chroma, R, w, h, nbx, nb, T, x, [None or (keys, y)] * 4)"""
    rng = np.random.default_rng(41)
    out = []

    def near(x, mx, spread):
        return np.clip(x + rng.integers(-spread, spread + 1, x.shape), 0, mx)

    # random planes of 3 x 2 blocks: every T, neighbours absent and present, random vectors per block - chroma with odd and negative ones
    for chroma, (w, h) in ((0, (37, 21)), (1, (19, 11))):
        for T in (0, 1, 2, 16, 64):
            mx = 1023 if T == 64 else 255
            for R in (8, 16):
                x = rng.integers(0, mx + 1, (h, w))
                nbrs = []
                for s in range(4):
                    if rng.integers(0, 3) == 0 and not (T == 16 and R == 8):
                        nbrs.append(None)
                        continue
                    keys = [key_of(int(rng.integers(-R, R + 1)), int(rng.integers(-R, R + 1)), R, int(rng.integers(0, 1 << 20))) for _ in range(6)]
                    if s == 1:
                        keys[2] = NONE          # one block without the neighbour
                    nbrs.append((keys, near(x, mx, max(T, 2))))
                out.append((chroma, R, w, h, 3, 6, T, x, nbrs))
    # the arithmetic shift: chroma under (-1, -1), (1, -3), (-15, 7) and (3, 1) - the vector halves to (-1, -1), (0, -2), (-8, 3), (1, 0)
    x = rng.integers(100, 140, (11, 19))
    for vecs in (((-1, -1), (1, -3), (-15, 7), (3, 1)),):
        out.append((1, 16, 19, 11, 3, 6, 16, x, [([key_of(dy, dx, 16)] * 6, near(x, 255, 6)) for dy, dx in vecs]))
    # vectors of +-R into every corner of planes smaller than the window
    for (w, h) in ((1, 1), (2, 3), (4, 2), (3, 3)):
        for chroma in (0, 1):
            for R in (8, 16):
                x = rng.integers(500, 520, (h, w))
                corners = [(-R, -R), (-R, R), (R, -R), (R, R)]
                out.append((chroma, R, w, h, 1, 1, 64, x, [([key_of(dy, dx, R)], near(x, 1023, 20)) for dy, dx in corners]))
    # the largest num and den: a flat plane of 1023 under table 255 (T = 64 at 10 bits) with four flat neighbours
    flat = np.full((6, 7), 1023)
    out.append((0, 8, 7, 6, 1, 1, int(fgd_ref.reach_of(255, 10)), flat, [([key_of(0, 0, 8)], flat)] * 4))
    out.append((0, 8, 7, 6, 1, 1, int(fgd_ref.reach_of(255, 10)), flat, [([key_of(0, 0, 8)], flat), None, None, ([key_of(8, -8, 8)], flat)]))
    return out


def _flat(a):
    return " ".join(str(int(v)) for v in np.asarray(a).ravel())


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """(the case lines, the lines the plain program prints for them, the path of the case file)"""
    lines = ["S %d" % v for v in _fields()]
    lines += ["E %d %d %d %d" % c for c in _slots()]
    for chroma, R, w, h, nbx, nb, T, x, nbrs in _filters():
        parts = ["F %d %d %d %d %d %d %d %s" % (chroma, R, w, h, nbx, nb, T, _flat(x))]
        for nbr in nbrs:
            parts.append("0" if nbr is None else "1 %s %s" % (_flat(nbr[0]), _flat(nbr[1])))
        lines.append(" ".join(parts))
    d = tmp_path_factory.mktemp("fgdt_rule")
    path = d / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    out = host_build.run_program(host_build.host_cxx(gcc=True), SOURCES, d / "fgdt_rule_host", args=[path])
    assert out.returncode == 0, out.stderr[-2000:]
    got = out.stdout.split("\n")[:-1]
    assert len(got) == len(lines)
    return lines, got, path


def _of(program, kind):
    lines, got, _ = program
    return [[int(v) for v in g.split()] for ln, g in zip(lines, got) if ln[0] == kind]


def test_rule_field_and_slots(program):
    for v, g in zip(_fields(), _of(program, "S")):
        want = (2 if v & 0x200 else 1) if v & 0xC000 == 0xC000 else 0
        assert g == [want], hex(v)
    for (f, s, span, n), g in zip(_slots(), _of(program, "E")):
        assert g == [fgdt_ref.OFFSETS[s], int(fgdt_ref.exists(f, s, span, n))], (f, s, span, n)
    assert [fgdt_ref.exists(0, s, 2, 3) for s in range(4)] == [False, False, True, True] and not any(fgdt_ref.exists(0, s, 2, 1) for s in range(4))
    assert [fgdt_ref.exists(2, s, 1, 5) for s in range(4)] == [False, True, True, False]


def test_rule_filter_equals_the_restatement(program):
    moved = absent = 0
    largest = (0, 0)
    for (chroma, R, w, h, nbx, nb, T, x, nbrs), g in zip(_filters(), _of(program, "F")):
        keys = [np.full(nb, NONE, dtype=np.int64) if n is None else np.array(n[0], dtype=np.int64) for n in nbrs]
        planes = [None if n is None else n[1] for n in nbrs]
        want, num, den = fgdt_ref.filter_plane(x, np.full((h, w), T), planes, keys, R, nbx, chroma)
        assert g[:-2] == [int(v) for v in want.ravel()], (chroma, R, w, h, T)
        assert g[-2:] == [num, den], (chroma, R, w, h, T)
        assert (np.abs(want - x) <= max(0, T - 1)).all()
        if T <= 1:
            assert np.array_equal(want, x)
        moved += int((want != x).sum())
        absent += sum(n is None for n in nbrs)
        largest = max(largest, (den, num))
    assert moved > 200 and absent > 5
    # the bounds: den <= 1600 + 2 S * 12 * 64 and num < 2^23, reached by the flat plane of 1023 with four neighbours
    assert largest == (1600 + 4 * 12 * 64, (1600 + 4 * 12 * 64) * 1023) and largest[0] == 4672 and largest[1] < 1 << 23
    assert _of(program, "F")[-1][-1] == 1600 + 2 * 12 * 64


def test_standalone_program_under_sanitizers(program, tmp_path):
    """the same cases once under AddressSanitizer and UndefinedBehaviorSanitizer (host code only, a program of its own).  Skipped only where
    an empty program does not build and run under the sanitizers - their runtimes are not installed"""
    lines, got, path = program
    out = host_build.run_program(host_build.host_cxx(gcc=True), SOURCES, tmp_path / "fgdt_rule_host_san", args=[path], sanitized=True)
    assert out.returncode == 0, out.stdout[-500:] + out.stderr[-2000:]
    assert out.stdout.split("\n")[:-1] == got


# ---------------------------------------------------------------- what follows from the rule (the restatement alone)
@pytest.mark.parametrize("bd", [8, 10])
def test_consequences_of_the_rule(bd):
    rng = np.random.default_rng(44 + bd)
    w, h, n, R = 40, 24, 3, 8
    _, raw = fgdt_ref.texture_clip(w, h, bd, n)
    frames = fg_ref.split(raw, w, h, bd, n)
    nbx, nby = fgdt_ref.blocks(w, h)
    for span in (1, 2):
        assert fgdt_ref.denoise(raw, w, h, bd, n, np.zeros((3, 8), dtype=np.uint8), span, R) == raw          # a zero table is the identity
    table = rng.integers(0, 256, (3, 8))
    mv = fgdt_ref.search(frames, w, h, 2, R)
    assert (mv[0, :2] == NONE).all() and (mv[1, 0] == NONE).all() and (mv[1, 1:3] != NONE).all() and (mv[1, 3] == NONE).all() and (mv[2, 2:] == NONE).all()
    out = fgdt_ref.denoise_frames(frames, table, bd, mv, R, nbx)
    for fr, fo in zip(frames, out):
        for x, o, T in zip(fr, fo, fgd_ref.reaches(fr[0], table, bd)):
            assert (np.abs(o - x) <= np.maximum(0, T - 1)).all()                                              # no sample moves by T or more
    assert fg_ref.join(out, bd) != fgd_ref.denoise(raw, w, h, bd, n, table)                                   # (the term does something)
    # a one-frame chunk is the spatial filter's, and so is a chunk whose keys say "no neighbour" everywhere
    one = raw[:len(raw) // n]
    assert fgdt_ref.denoise(one, w, h, bd, 1, table, 2, R) == fgd_ref.denoise(one, w, h, bd, 1, table)
    assert fgdt_ref.denoise(raw, w, h, bd, n, table, 2, R, use_mv=np.full((n, 4, nbx * nby), NONE)) == fgd_ref.denoise(raw, w, h, bd, n, table)
    # a static noiseless clip is unchanged: a constant one, one whose neighbours are equal or a full amplitude away, and the clean ramps
    # under their own estimate (nothing in them reads as grain)
    full = np.full((3, 8), 255)
    flat = fg_ref.join([[np.full((h, w), 517 >> (10 - bd)), np.full((h // 2, w // 2), 3), np.full((h // 2, w // 2), (1 << bd) - 1)]] * 3, bd)
    assert fgdt_ref.denoise(flat, w, h, bd, 3, full, 2, R) == flat
    checker = fg_ref.checker_clip(w, h, bd, 1) * 3
    assert fgdt_ref.denoise(checker, w, h, bd, 3, full, 2, R) == checker
    ramps = fgd_ref.ramp_clip(72, 56, bd, 1)[0] * 3
    assert fgdt_ref.denoise(ramps, 72, 56, bd, 3, fg_ref.estimate(ramps, 72, 56, bd, 3, 50)[0], 2, R) == ramps
    # an unrelated neighbour - a scene cut - moves no sample by T or more, whatever the search found in it
    other = fg_ref.split(fgdt_ref.texture_clip(w, h, bd, 1, seed=99)[1], w, h, bd, 1)
    cut = [frames[0], other[0]]
    mv = fgdt_ref.search(cut, w, h, 1, R)
    out = fgdt_ref.denoise_frames(cut, full, bd, mv, R, nbx)
    for fr, fo in zip(cut, out):
        for x, o, T in zip(fr, fo, fgd_ref.reaches(fr[0], full, bd)):
            assert (np.abs(o - x) <= np.maximum(0, T - 1)).all()
    # the edge extension replicates the denoised edge
    _, small = fgdt_ref.texture_clip(10, 14, bd, 2)
    fs = fg_ref.split(small, 10, 14, bd, 2)
    padded = fgd_ref.pad(fgdt_ref.denoise_frames(fs, table, bd, fgdt_ref.search(fs, 10, 14, 1, R), R, 1), 10, 14)
    assert padded[0][0].shape == (16, 16) and (padded[0][0][:, 9:] == padded[0][0][:, 9:10]).all() and (padded[1][2][7:, :] == padded[1][2][6:7, :]).all()


# ---------------------------------------------------------------- what the term gains (the restatement alone)
TEXTURE_SIZE = (96, 64, 5)
RAMP_SIZE = (136, 72, 5)
N = 50   # the ceiling of the ramps' estimate, as tests/test_fgd_host.py has it

_gains = {}


def gains(kind, bd):
    """(noisy, spatial, S = 1, S = 2) PSNR against the clean clip, computed once"""
    if (kind, bd) not in _gains:
        if kind == "texture":
            w, h, n = TEXTURE_SIZE
            clean, noisy = fgdt_ref.texture_clip(w, h, bd, n)
            table = fgdt_ref.uniform_table()
        else:
            w, h, n = RAMP_SIZE
            clean, noisy = fgd_ref.ramp_clip(w, h, bd, n)
            table = fg_ref.estimate(noisy, w, h, bd, n, N)[0]
        outs = [noisy, fgd_ref.denoise(noisy, w, h, bd, n, table)] + [fgdt_ref.denoise(noisy, w, h, bd, n, table, s, 8) for s in (1, 2)]
        _gains[(kind, bd)] = [fgd_ref.psnr(o, clean, bd) for o in outs]
    return _gains[(kind, bd)]


@pytest.mark.parametrize("bd", [8, 10])
def test_restatement_gains_on_the_texture(bd):
    """the moving random texture under noise of sigma 1, the table signalling that sigma (64 in every bin): the spatial filter finds no
    honest neighbour, the temporal term does - S = 1 and S = 2 are each at least 2 dB nearer the clean clip than the spatial filter's output.
    Measured, noisy / spatial / S = 1 / S = 2 in dB: 8 bits 47.78 / 46.65 / 49.73 / 50.70 (+3.08, +4.05), 10 bits 48.15 / 47.27 / 50.68 / 51.77
    (+3.41, +4.50); the spatial filter leaves the clip 0.9 - 1.1 dB worse than it found it"""
    noisy, spatial, s1, s2 = gains("texture", bd)
    print("texture %d bits: noisy %.2f, spatial %.2f, S = 1 %.2f (%+.2f), S = 2 %.2f (%+.2f) dB" % (bd, noisy, spatial, s1, s1 - spatial, s2, s2 - spatial))
    assert s1 - spatial >= 2.0 and s2 - spatial >= 2.0


@pytest.mark.parametrize("bd", [8, 10])
def test_restatement_gains_on_the_ramps(bd):
    """tests/fgd_ref.py's ramps with an edge and a bar under their own estimate: the spatial filter already gains several dB there, and each
    span is nearer the clean clip still.
    Measured, noisy / spatial / S = 1 / S = 2 in dB: 8 bits 46.99 / 52.18 / 52.53 / 52.66 (+0.36, +0.48), 10 bits 47.57 / 55.51 / 55.99 / 56.25
    (+0.48, +0.75)"""
    noisy, spatial, s1, s2 = gains("ramp", bd)
    print("ramps %d bits: noisy %.2f, spatial %.2f, S = 1 %.2f (%+.2f), S = 2 %.2f (%+.2f) dB" % (bd, noisy, spatial, s1, s1 - spatial, s2, s2 - spatial))
    assert s1 - spatial > 0.0 and s2 - spatial > 0.0


# ---------------------------------------------------------------- the order of the bytes (the oracle)
BYTES_CLIP = (136, 72, 10, 3)
BYTES_CQ = 4


def bytes_clip():
    """(noisy bytes, the restatement's estimate of it at the ceiling N): what tests/test_fgdt.py's byte comparison encodes"""
    w, h, bd, n = BYTES_CLIP
    noisy = fgd_ref.ramp_clip(w, h, bd, n)[1]
    return noisy, fg_ref.estimate(noisy, w, h, bd, n, N)[0]


def test_oracle_codes_the_temporal_output_in_fewer_bytes(oracle):
    """what tests/test_fgdt.py's byte comparison relies on: on the noisy ramps at 10 bits and CQ 4, under the clip's own estimate, the oracle's
    key-frame encode of the S = 1 output is smaller than that of the spatial filter's output by more than 1 %.  Chosen among the ramps at 8
    and 10 bits and CQ 4, 8, 12 and 20, where the oracle's sizes were (spatial / S = 1): 10 bits 3516 / 3446, 2209 / 2195, 1669 / 1668, 1214 / 1216;
    8 bits 2638 / 2611, 1915 / 1919, 1562 / 1561, 1198 / 1197 - from CQ 8 on the quantiser removes what is left of a sigma of 1 and the two
    differ by less than a symbol's noise; on the moving texture the content's own 140 levels drown the grain's bytes (16 456 / 16 452 at CQ 8).
    Measured here: 3516 and 3446 bytes, 2.0 %"""
    w, h, bd, n = BYTES_CLIP
    noisy, table = bytes_clip()
    case = dict(w=w, h=h, bd=bd, n=n, params=dict(keyint=1, cq_level=BYTES_CQ))
    size = {}
    for name, raw in (("spatial", fgd_ref.denoise(noisy, w, h, bd, n, table)), ("S = 1", fgdt_ref.denoise(noisy, w, h, bd, n, table, 1, 8))):
        tus, _, _ = edge_content.oracle_encode(oracle, case, fg_ref.split(raw, w, h, bd, n))
        size[name] = sum(len(t) for t in tus)
    print("oracle bytes at CQ %d: spatial %d, S = 1 %d" % (BYTES_CQ, size["spatial"], size["S = 1"]))
    assert size["S = 1"] * 100 < size["spatial"] * 99, size
