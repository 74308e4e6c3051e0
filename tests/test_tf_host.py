"""CPU tests of the key frames' temporal filter (include/av1mi.h: av1mi_params.me_presearch bits 8-14, av1mi_temporal_filter; DESIGN.md
§3 item 8d): the rule header (av1-base_amd/csrc/tf_rule.h) compiled for the host (tests/host/tf_rule_host.cpp, a stand-alone program,
once more under AddressSanitizer and UndefinedBehaviorSanitizer) against tests/tf_ref.py; how the field packs and what is refused, the
ABI staying what it was; and properties of the reference alone, among them that the content of every GPU case (tests/tf_cases.py)
exercises the rule."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import host_build
import tf_cases
import tf_ref
from test_aq_host import av1mi  # noqa: F401  (the library through its host-only path)
from test_part_inter_host import cxx  # noqa: F401  (the same compiler lookup)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "tf_rule_host.cpp")


# ---------------------------------------------------------------- the rule header against the restatement
@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """(path of the case file, per line what the program must print)"""
    path = str(tmp_path_factory.mktemp("tf_rule") / "cases.txt")
    lines, want = [], []
    for v in sorted({tf_ref_field(pre, n, s) for pre in (0, 1) for n in range(8) for s in range(8)} | {1 << b for b in range(32)} | {0x7701, 0xFFFFFFFF, 0x1000, 0x1100}):
        ok, pre, n, s = tf_ref.field_decode(v)
        lines.append("F %d" % v)
        want.append("%d %d %d %d" % (ok, pre, n, s))
    for N in (1, 3, 7):
        for keyint in (1, 2, 3, 8, 240):
            for n_frames in (1, 2, 7, 8, 9):
                for f in range(0, n_frames, keyint):
                    lines.append("N %d %d %d %d" % (N, keyint, n_frames, f))
                    want.append("%d %d" % (tf_ref.followers(N, keyint, n_frames, f), (n_frames + keyint - 1) // keyint))
    rng = np.random.default_rng(7)
    big = False
    for bd in (8, 10):
        top = (1 << bd) - 1
        for s in range(8):
            sh = tf_ref.shift_of(s, bd)
            for chroma in (0, 1):
                nsamp = 64 if chroma else 256
                for S, B in [(0, 0), (9 * top * top, nsamp * top * top), (1 << sh, 0), (0, nsamp << sh), ((1 << sh) - 1, (nsamp << sh) // 9)] + \
                            [(int(rng.integers(0, 9 * top * top + 1)), int(rng.integers(0, nsamp * top * top + 1))) for _ in range(6)]:
                    S, B = min(S, 9 * top * top), min(B, nsamp * top * top)
                    big |= 9 * B > 1 << 31
                    i = int(tf_ref.index(S, B, sh, chroma))
                    lines.append("I %d %d %d %d" % (S, B, sh, chroma))
                    want.append("%d %d" % (i, tf_ref.WEIGHTS[i]))
    assert big   # 9 B beyond 2^31 is among them
    for den in (16, 17, 31, 64, 127, 128):
        for num in (0, 1, den // 2 - 1, den // 2, den - 1, 16 * 255, den * 1023 - 1, den * 1023):
            lines.append("L %d %d" % (num, den))
            want.append("%d" % tf_ref.blend(num, den))
    for dx in (-16, -3, -2, -1, 0, 1, 2, 15):   # odd / even vectors, both signs: the shift is arithmetic
        for dy in (-5, -2, 0, 1, 4):
            for a, b, c, d in [(0, 0, 0, 0), (1023, 1023, 1023, 1023), (1, 2, 4, 8), (1023, 0, 1022, 1), (0, 1, 0, 0)]:
                for p in (0, 7, 100):
                    lines.append("C %d %d %d %d %d %d %d" % (a, b, c, d, dx, dy, p))
                    want.append("%d %d %d" % (tf_ref.chroma_pred(a, b, c, d, dx, dy), p + (dx >> 1), p + (dy >> 1)))
    # generated blocks: constant key against constant predictions
    dens = set()
    for bd, key, pred in [(10, 0, 1023), (10, 1023, 0), (10, 512, 512), (8, 0, 255), (8, 100, 100), (8, 100, 103), (10, 400, 409), (8, 17, 20)]:
        for s in (0, 2, 7):
            for chroma in (0, 1):
                for n in (0, 1, 7):
                    side = 8 if chroma else 16
                    e2 = np.full((side, side), (key - pred) ** 2, dtype=np.int64)
                    S, B = int(tf_ref.window_sum(e2)[0, 0]), int(e2.sum())
                    i = int(tf_ref.index(S, B, tf_ref.shift_of(s, bd), chroma))
                    w = int(tf_ref.WEIGHTS[i])
                    den = 16 + n * w
                    dens.add(den)
                    lines.append("K %d %d %d %d %d %d" % (bd, s, key, pred, chroma, n))
                    want.append("%d %d %d %d %d %d" % (S, B, i, w, den, tf_ref.blend(16 * key + n * w * pred, den)))
                    if (bd, key, pred, chroma) == (10, 0, 1023, 0):
                        assert 9 * B > 1 << 31 and w == 0   # all-zero against all-max at 10 bit: no overflow, no weight
    assert {16, 128} <= dens
    open(path, "w").write("\n".join(lines) + "\n")
    return path, want


def tf_ref_field(pre, n, s):
    return (pre & 1) | ((n & 7) << 8) | ((s & 7) << 12)


def _check(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, g, w)


def test_standalone_program_equals_the_restatement(cxx, cases, tmp_path):  # noqa: F811
    out = host_build.run_program(cxx, SRC, tmp_path / "tf_rule_host", args=[cases[0]])
    assert out.returncode == 0, out.stderr[-2000:]
    _check(out.stdout.split("\n")[:-1], cases[1])


def test_standalone_program_under_sanitizers(cxx, cases, tmp_path):  # noqa: F811
    """... and under AddressSanitizer and UndefinedBehaviorSanitizer (host code only, run on its own).  Skipped only where an empty
    program does not build and run under the sanitizers - their runtimes are not installed"""
    out = host_build.run_program(cxx, SRC, tmp_path / "tf_rule_host_san", args=[cases[0]], sanitized=True)
    assert out.returncode == 0, out.stdout[-500:] + out.stderr[-2000:]
    _check(out.stdout.split("\n")[:-1], cases[1])


# ---------------------------------------------------------------- packing
@pytest.mark.parametrize("pre", [0, 1])
@pytest.mark.parametrize("n", range(8))
def test_packed_field_accepted(av1mi, pre, n):  # noqa: F811
    for s in range(8) if n else (0,):
        p = av1mi.default_params(640, 360, 8, me_presearch=pre, tf_frames=n, tf_strength=s)
        assert p.me_presearch == pre | (n << 8) | (s << 12) == av1mi.me_tf(pre, n, s)
        assert (av1mi.me_presearch_of(p.me_presearch), av1mi.tf_frames_of(p.me_presearch), av1mi.tf_strength_of(p.me_presearch)) == (pre, n, s)
        assert tf_ref.field_decode(p.me_presearch) == (True, pre, n, s)
        av1mi.write_headers(p)


@pytest.mark.parametrize("v", [1 << b for b in list(range(1, 8)) + [11] + list(range(15, 32))] + [0x1000, 0x7000, 0x1001, 2, 3, 0x7703])
def test_packed_field_refused(av1mi, v):  # noqa: F811
    """bits 1-7, 11 and 15 and above, and a strength without frames"""
    with pytest.raises(av1mi.EncodeFailed) as e:
        av1mi.write_headers(av1mi.default_params(640, 360, 8, me_presearch=v))
    assert e.value.code == 1   # AV1MI_E_INVALID_ARG


def test_default_params_keywords(av1mi):  # noqa: F811
    assert av1mi.default_params(64, 64, 8).me_presearch == 0                      # the default stays off
    assert av1mi.default_params(64, 64, 8, tf_frames=3).me_presearch == 3 << 8
    assert av1mi.default_params(64, 64, 8, tf_strength=2, tf_frames=7, me_presearch=1).me_presearch == 1 | 7 << 8 | 2 << 12
    assert av1mi.default_params(64, 64, 8, me_presearch=1).me_presearch == 1


def test_abi_unchanged_and_symbol_exported(av1mi):  # noqa: F811
    assert C.sizeof(av1mi.Params) == 36 * 4 == 144 and av1mi.struct_sizes() == av1mi.mirror_sizes()
    assert av1mi.ABI_VERSION == int(av1mi._lib.av1mi_abi_version()) == 8
    assert "av1mi_temporal_filter" in av1mi.ABI_SYMBOLS
    assert getattr(av1mi._lib, "av1mi_temporal_filter") is not None   # exported
    hdr = open(os.path.join(ROOT, "include", "av1mi.h")).read()
    assert re.search(r"\bint\s+av1mi_temporal_filter\s*\(", hdr)
    for macro in ("AV1MI_ME_TF", "AV1MI_ME_PRESEARCH", "AV1MI_TF_FRAMES", "AV1MI_TF_STRENGTH"):
        assert re.search(r"#define\s+%s\(" % macro, hdr), macro
    assert "#define AV1MI_ABI_VERSION 8" in hdr
    shim = open(os.path.join(ROOT, "integration", "mi355x.rs")).read()
    assert "fn me_tf(" in shim and "36 * 4" in shim


# ---------------------------------------------------------------- properties of the reference alone
def test_static_noise_free_clip_comes_back_identical():
    _, clean = tf_ref.pattern_clip(72, 56, 8, 4, seed=1, static=True)
    for s in (0, 2, 7):
        out, mv, st = tf_ref.filter_chunk(clean, 72, 56, 8, 4, 4, 3, s, 8)
        assert out == clean
        assert ((mv & 0x7FF) == 8 * 17 + 8).all() and (mv >> 11 == 0).all()   # the zero vector at no cost
        assert st["hist"][0] == st["hist"].sum()                                # full weight everywhere


@pytest.mark.parametrize("bd", [8, 10])
def test_unrelated_follower_leaves_the_key_frame_identical(bd):
    _, clean = tf_ref.pattern_clip(72, 56, bd, 1, seed=2)
    key = tf_ref.split(clean, 72, 56, bd, 1)[0]
    top = (1 << bd) - 1
    buf = tf_ref.join([key, [top - p for p in key]], bd)
    for s in range(5):
        out, _, st = tf_ref.filter_chunk(buf, 72, 56, bd, 2, 2, 1, s, 8)
        assert out == buf and st["rejected"] == st["pairs"], s


def test_no_followers_no_change():
    noisy, _ = tf_ref.pattern_clip(24, 40, 8, 3, seed=3)
    for keyint, n in ((1, 3), (3, 1), (2, 3)):
        out, mv, _ = tf_ref.filter_chunk(noisy[:24 * 40 * 3 // 2 * n], 24, 40, 8, n, keyint, 3, 2, 8)
        want_same = keyint == 1 or n == 1
        assert (out == noisy[:len(out)]) == want_same
        if want_same:
            assert (mv == tf_ref.NONE).all()
    # keyint 2 of 3 frames: the key frame 2 is the chunk's last and stays, frame 1 is a follower and stays
    out, mv, _ = tf_ref.filter_chunk(noisy, 24, 40, 8, 3, 2, 3, 2, 8)
    fb = 24 * 40 * 3 // 2
    assert out[fb:] == noisy[fb:] and out[:fb] != noisy[:fb]
    assert (mv[1] == tf_ref.NONE).all() and (mv[0, 1:] == tf_ref.NONE).all() and (mv[0, 0] != tf_ref.NONE).all()


def test_zeros_against_all_max_is_the_identity():
    z = tf_cases.zeros_then_max()
    out, mv, st = tf_ref.filter_chunk(z, 16, 16, 10, 3, 3, 2, 0, 8)
    assert out == z and st["rejected"] == st["pairs"] == 2
    assert (mv >> 11 == 256 * 1023).all()   # the zero vector: every candidate has the same SAD


def test_filter_reduces_the_noise():
    """what the filter is for: against the clean pattern the key frame's luma error falls"""
    w, h, bd, n = 72, 56, 8, 4
    noisy, clean = tf_cases.content(w, h, bd, n)
    out = tf_cases.reference((72, 56, 8, 4, 4, 3, 2, 8))[0]
    k, c, o = (tf_ref.split(b, w, h, bd, n)[0][0] for b in (noisy, clean, out))
    assert ((o - c) ** 2).mean() < ((k - c) ** 2).mean()


@pytest.mark.parametrize("case", tf_cases.FILTER_CASES, ids=tf_cases.case_id)
def test_gpu_cases_exercise_the_rule(case):
    tf_cases.exercises_the_rule(case)
    w, h, bd, n, keyint, N, s, R = case
    out, mv, st = tf_cases.reference(case)
    fb = w * h * 3 // 2 * (2 if bd > 8 else 1)
    noisy = tf_cases.content(w, h, bd, n)[0]
    for f in range(n):   # followers, and key frames without one, are never modified
        if f % keyint or tf_ref.followers(N, keyint, n, f) == 0:
            assert out[f * fb:(f + 1) * fb] == noisy[f * fb:(f + 1) * fb], f
    assert len(set(int(v) & 0x7FF for v in mv.ravel() if v != tf_ref.NONE)) >= (1 if (w, h) == (8, 8) else 2)   # more than one vector
    # the whole-frame statement of the weights' statistics (what tools/tf_ab.py reports) gives the block-wise one's figures
    W, H = (w + 7) & ~7, (h + 7) & ~7
    coded = [[tf_ref.extend(fr[0], W, H), tf_ref.extend(fr[1], W // 2, H // 2), tf_ref.extend(fr[2], W // 2, H // 2)] for fr in tf_ref.split(noisy, w, h, bd, n)]
    hist, rejected = np.zeros(16, dtype=np.int64), 0
    for f in range(0, n, keyint):
        nf = tf_ref.followers(N, keyint, n, f)
        if nf:
            h1, r1 = tf_ref.frame_stats(coded[f], coded[f + 1:f + 1 + nf], mv[f // keyint, :nf], W, H, bd, s, R)
            hist, rejected = hist + h1, rejected + r1
    assert np.array_equal(hist, st["hist"]) and rejected == st["rejected"]
