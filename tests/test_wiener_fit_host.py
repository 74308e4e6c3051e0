"""CPU tests of the Wiener restoration fit (include/av1mi.h: AV1MI_LR_WIENER_FIT): the rule header
(av1-base_amd/csrc/wiener_fit_rule.h, compiled for the host) against the Python restatement (tests/wiener_fit_ref.py) - the two-stage
solve on sums of real planes, random sums and built ones, the unit-code writer through the spec's decoder - the stand-alone program
plain and under the sanitizers, and the parameter's range, headers and ABI."""
import ctypes as C
import itertools
import os
import random

import numpy as np
import pytest

import host_build
import lr_ref
import wiener_fit_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "wiener_fit_rule_host.cpp")
CODE_BITS = 64   # the container of a unit's code: two 32-bit words (Av1miLrWfit::code, beside the length)


@pytest.fixture(scope="module")
def av1mi():
    return host_build.library()


@pytest.fixture(scope="module")
def cxx():
    return host_build.host_cxx(gcc=True)


@pytest.fixture(scope="module")
def rule(cxx, tmp_path_factory):
    lib = C.CDLL(host_build.build_shared(cxx, SRC, tmp_path_factory.mktemp("wfit") / "libwfitrule.so"))
    lib.wf_fit.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.wf_solve.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.wf_code.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
    lib.wf_tap_table.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    return lib


def _fit_both(rule, probs):
    """probs: [(sums[27], first)]; the C++ rule against the restatement (which asserts its intermediates stay inside 63 bits)"""
    n = len(probs)
    sums = np.array([p[0] for p in probs], dtype=np.int64).reshape(n, ref.N_SUMS)
    first = np.array([p[1] for p in probs], dtype=np.int32)
    taps = np.zeros((n, 6), dtype=np.int32)
    present = np.zeros(n, dtype=np.int32)
    flags = np.zeros(n, dtype=np.int32)
    rule.wf_fit(sums.ctypes.data, first.ctypes.data, n, taps.ctypes.data, present.ctypes.data, flags.ctypes.data)
    seen = dict(present=0, absent=0, refit=0, clamped=0, free=0)
    for i, (s, f) in enumerate(probs):
        info = {}
        want = ref.fit([int(v) for v in s], f, info)
        got = ([int(v) for v in taps[i, :3]], [int(v) for v in taps[i, 3:]]) if present[i] else None
        assert got == want, (s, f, got, want)
        seen["present" if want else "absent"] += 1
        if want:
            assert bool(flags[i] >> 12 & 1) == info["v"]["refit"] and bool(flags[i] >> 13 & 1) == info["h"]["refit"], (s, f)
            assert {j for j in range(3) if flags[i] >> j & 1} == info["v"]["clamped"], (s, f)
            assert {j for j in range(3) if flags[i] >> (6 + j) & 1} == info["h"]["clamped"], (s, f)
            seen["refit"] += info["v"]["refit"] or info["h"]["refit"]
            seen["clamped"] += bool(info["v"]["clamped"] or info["h"]["clamped"])
            seen["free"] += not (info["v"]["clamped"] or info["h"]["clamped"])
            for t in want:
                assert all(ref.TAPS_MIN[j] <= t[j] <= ref.TAPS_MAX[j] for j in range(f, 3)) and all(t[j] == 0 for j in range(f)), t
    return seen


# ---------------------------------------------------------------- sums of real planes
FRAMES = [(200, 120, 8, {}), (328, 248, 10, dict(deblock=1)), (202, 122, 8, dict(base_q_idx=180))]


def test_fit_on_frame_sums(rule, oracle):
    """every unit of all three planes of the oracle's pre-CDEF / CDEF planes; and the restated sums stay below 2^36"""
    probs = []
    for w, h, bd, kw in FRAMES:
        planes = [p.astype(np.int64) for p in oracle.synthclip_frame(w, h, bd, seed=500 + w, t=0)]
        _, pre, _ = oracle.encode_frame(oracle.default_config(w, h, bd, enable_cdef=0, enable_lr=0, **kw), planes)
        _, cdef, _ = oracle.encode_frame(oracle.default_config(w, h, bd, enable_cdef=1, enable_lr=0, **kw), planes)
        for pl in range(3):
            ph, pw = (h + (pl > 0)) >> (pl > 0), (w + (pl > 0)) >> (pl > 0)
            p, c, s = (np.asarray(a[pl][:ph, :pw], dtype=np.int64) for a in (pre, cdef, planes))
            dv, dh = ref.plane_d(p, c, int(pl > 0))
            rows, cols = lr_ref.unit_bounds(ph, pw, int(pl > 0))
            for y0, y1 in rows:
                for x0, x1 in cols:
                    sl = (slice(y0, y1), slice(x0, x1))
                    sums = ref.unit_sums(c[sl], s[sl], [d[sl] for d in dv], [d[sl] for d in dh])
                    assert max(abs(v) for v in sums) < 1 << 36
                    probs.append((sums, int(pl > 0)))
    seen = _fit_both(rule, probs)
    print(seen)
    assert seen["present"] > 0 and seen["clamped"] > 0


# ---------------------------------------------------------------- random and built sums
def _gram(rng, mag, n=6):
    """sums of a positive semi-definite kind: the Gram matrix of n random vectors of a few samples, scaled to the magnitude"""
    vecs = [[rng.randint(-2046, 2046) for _ in range(8)] for _ in range(n + 1)]
    g = [[sum(a * b for a, b in zip(vecs[i], vecs[j])) for j in range(n + 1)] for i in range(n + 1)]
    top = max(abs(v) for row in g for v in row) or 1
    sc = lambda v: v * mag // top
    s = [sc(g[j][k]) for j in range(3) for k in range(j, 3)] + [sc(g[3 + j][3 + k]) for j in range(3) for k in range(j, 3)]
    s += [sc(g[j][3 + k]) for j in range(3) for k in range(3)] + [sc(g[j][6]) for j in range(3)] + [sc(g[3 + k][6]) for k in range(3)]
    return s


def test_fit_on_random_and_built_sums(rule):
    """random sums of every magnitude up to the 2^36 bound (Gram matrices and arbitrary signed entries), singular systems, negative
    diagonals, every entry at the bound with every sign pattern of the right-hand sides, and right-hand sides that push every subset
    of the taps to a clamp"""
    rng = random.Random(11)
    B = 1 << 36
    probs = []
    for it in range(3000):
        mag = rng.choice([1 << 8, 1 << 17, 1 << 18, 1 << 27, B - 1, B])
        kind = it % 6
        if kind <= 1:
            s = _gram(rng, mag)
        elif kind == 2:      # anything
            s = [rng.randint(-mag, mag) for _ in range(ref.N_SUMS)]
        elif kind == 3:      # singular: rank one in both blocks
            a, b = [rng.randint(1, 1 << 17) for _ in range(3)], [rng.randint(1, 1 << 17) for _ in range(3)]
            s = [a[j] * a[k] for j in range(3) for k in range(j, 3)] + [b[j] * b[k] for j in range(3) for k in range(j, 3)]
            s += [a[j] * b[k] for j in range(3) for k in range(3)] + [rng.randint(-mag, mag) for _ in range(6)]
        elif kind == 4:      # negative diagonals
            s = _gram(rng, mag)
            for k in (0, 3, 5, 6, 9, 11):
                if rng.random() < 0.5:
                    s[k] = -abs(s[k]) - 1
        else:                # every entry at the bound
            s = [rng.choice([-B, B]) for _ in range(ref.N_SUMS)]
            for k in (0, 3, 5, 6, 9, 11):
                s[k] = B
        probs.append((s, it & 1))
    # every subset of taps clamped: a diagonal system whose right-hand side puts tap j far outside (subset) or well inside its range
    for first in (0, 1):
        idx = list(range(first, 3))
        for r in range(len(idx) + 1):
            for sub in itertools.combinations(idx, r):
                for sign in (-1, 1):
                    d = 1 << 30
                    s = [0] * ref.N_SUMS
                    for k in (0, 3, 5):
                        s[ref.HVV + k] = s[ref.HHH + k] = d
                    s[ref.HVV + 1] = s[ref.HHH + 1] = d >> 3   # a coupling, so that the refit moves the free taps
                    for j in idx:
                        v = sign * 4 * d if j in sub else (ref.TAPS_MIN[j] + ref.TAPS_MAX[j]) // 2 * d // 128
                        s[ref.CV + j], s[ref.CH + j] = v, v
                    probs.append((s, first))
    seen = _fit_both(rule, probs)
    print(seen)
    assert all(v > 0 for v in seen.values()), seen


def test_single_pass_solve_every_clamp_subset(rule):
    """av1mi_wf_solve alone on the built systems: the clamp acts on exactly the subset asked for, and the refit runs iff the subset is a
    proper, non-empty one"""
    for first in (0, 1):
        idx = list(range(first, 3))
        for r in range(len(idx) + 1):
            for sub in itertools.combinations(idx, r):
                d = 1 << 30
                H = [[d if i == j else 0 for j in range(3)] for i in range(3)]
                R = [(4 * d if j in sub else (ref.TAPS_MIN[j] + ref.TAPS_MAX[j]) // 2 * d // 128) for j in range(3)]
                info = {}
                want = ref.solve(H, R, first, info)
                t = (C.c_int * 3)()
                cl, rf = C.c_int(0), C.c_int(0)
                ok = rule.wf_solve(np.array(H, dtype=np.int64).ctypes.data, np.array(R, dtype=np.int64).ctypes.data, first, t, C.byref(cl), C.byref(rf))
                assert ok and list(t) == want, (first, sub, list(t), want)
                assert info["clamped"] == set(sub) == {j for j in range(3) if cl.value >> j & 1}
                assert info["refit"] == bool(rf.value) == (0 < len(sub) < len(idx))


# ---------------------------------------------------------------- the writer against the decoder
def test_code_writer_round_trip(rule):
    """every (reference, value) pair of each tap, and random whole units of luma and chroma, through the spec's decoder; the longest
    code fits the container"""
    import sgr_fit_ref
    longest_tap = []
    for j in range(3):
        n = ref.TAPS_MAX[j] - ref.TAPS_MIN[j] + 1
        bits, lens = np.zeros(n * n, dtype=np.uint64), np.zeros(n * n, dtype=np.int32)
        rule.wf_tap_table(j, bits.ctypes.data, lens.ctypes.data)
        for r in range(n):
            for v in range(n):
                b = sgr_fit_ref.Bits(int(bits[r * n + v]), int(lens[r * n + v]))
                got = sgr_fit_ref._signed_subexp_with_ref(b, ref.TAPS_MIN[j], ref.TAPS_MAX[j] + 1, j + 1, ref.TAPS_MIN[j] + r)
                assert got == ref.TAPS_MIN[j] + v and b.n == 0, (j, r, v)
        longest_tap.append(int(lens.max()))
    rng = random.Random(5)
    longest = 0
    word = C.c_uint64()
    for it in range(4000):
        first = it & 1
        pick = lambda: [0 if j < first else rng.randint(ref.TAPS_MIN[j], ref.TAPS_MAX[j]) for j in range(3)]
        cv, ch, rf = pick(), pick(), [pick(), pick()]
        if it < 8:   # the extremes against each other
            cv = [0 if j < first else (ref.TAPS_MIN, ref.TAPS_MAX)[it >> 1 & 1][j] for j in range(3)]
            ch = cv
            rf = [[(ref.TAPS_MAX, ref.TAPS_MIN)[it >> 2 & 1][j] for j in range(3)]] * 2
        n = rule.wf_code(first, (C.c_int * 3)(*cv), (C.c_int * 3)(*ch), (C.c_int * 6)(*(rf[0] + rf[1])), C.byref(word))
        assert ref.decode_wiener_unit(word.value, n, first, rf) == (cv, ch, 0), (first, cv, ch, rf)
        longest = max(longest, n)
    print("longest code per tap", longest_tap, "bits; longest unit", longest, "bits; bound", 2 * sum(longest_tap), "bits")
    assert longest <= 2 * sum(longest_tap) <= CODE_BITS


# ---------------------------------------------------------------- the stand-alone program
def test_standalone_program(cxx, tmp_path):
    out = host_build.run_program(cxx, SRC, tmp_path / "wfit_main", defines=["WIENER_FIT_RULE_MAIN"])
    assert out.returncode == 0 and " 0 failures" in out.stdout, out.stdout + out.stderr


def test_standalone_program_under_sanitizers(cxx, tmp_path):
    """... and under AddressSanitizer and UndefinedBehaviorSanitizer (host code only; a signed overflow in the rule would stop it).
    Skipped only where an empty program does not build and run under the sanitizers - their runtimes are not installed"""
    out = host_build.run_program(cxx, SRC, tmp_path / "wfit_main_san", defines=["WIENER_FIT_RULE_MAIN"], sanitized=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert " 0 failures" in out.stdout


# ---------------------------------------------------------------- the parameter
@pytest.mark.parametrize("v", [0x401, 0x402, 0x403, 0x404, 0x502, 0x504])
def test_wiener_fit_accepted(av1mi, v):
    av1mi.write_headers(av1mi.default_params(640, 360, 8, enable_lr=v))


@pytest.mark.parametrize("v", [0x400, 0x405, 0x501, 0x204, 0x800 | 2])
def test_wiener_fit_refused(av1mi, v):
    with pytest.raises(av1mi.EncodeFailed) as e:
        av1mi.write_headers(av1mi.default_params(640, 360, 8, enable_lr=v))
    assert e.value.code == 1   # AV1MI_E_INVALID_ARG


@pytest.mark.parametrize("kw", [{}, dict(film_grain=20, cdef_search=3, deblock=1), dict(width=202, height=122, bit_depth=8, cdf_update=0)])
def test_wiener_fit_headers_are_the_plain_ones(av1mi, kw):
    kw = dict(kw)
    w, h, bd = kw.pop("width", 1920), kw.pop("height", 1080), kw.pop("bit_depth", 10)
    for lr in (1, 2, 3, 4):
        plain = av1mi.write_headers(av1mi.default_params(w, h, bd, enable_lr=lr, **kw))
        assert av1mi.write_headers(av1mi.default_params(w, h, bd, enable_lr=lr, lr_wiener_fit=True, **kw)) == plain
        if lr in (2, 4):
            assert av1mi.write_headers(av1mi.default_params(w, h, bd, enable_lr=lr, lr_fit=True, lr_wiener_fit=True, **kw)) == plain
    assert av1mi.default_params(w, h, bd, enable_lr=3, lr_wiener_fit=True).enable_lr == 0x403
    assert av1mi.default_params(w, h, bd, enable_lr=4, lr_fit=True, lr_wiener_fit=True).enable_lr == 0x504


def test_abi_unchanged(av1mi):
    assert av1mi._lib.av1mi_abi_version() == 8 == av1mi.ABI_VERSION
    sizes = av1mi.struct_sizes()
    assert sizes == av1mi.mirror_sizes()
    assert sizes[:8] == [144, 184, 120, 16, 32, 40, 184, 64], sizes   # the structures' sizes before the Wiener fit
    for name in ("av1mi_lr_wiener_fit_result", "av1mi_lr_wiener_fit_units", "av1mi_lr_fit_result", "av1mi_lr_fit_units"):
        assert name in av1mi.ABI_SYMBOLS and hasattr(av1mi._lib, name)
