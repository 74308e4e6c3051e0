"""CPU tests of the self-guided restoration fit (include/av1mi.h: AV1MI_LR_FIT): tests/sgr_fit_ref.py's filter
against the oracle's for all 16 parameter sets, the rule header (av1-base_amd/csrc/lr_fit_rule.h, compiled for the host) against the
Python restatement - parameter table, solve, unit-code writer round trip - and the parameter's range and headers."""
import ctypes as C
import os
import random

import numpy as np
import pytest

import host_build
import sgr_fit_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def av1mi():
    return host_build.library()


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    lib = C.CDLL(host_build.build_shared(host_build.host_cxx(gcc=True), os.path.join(ROOT, "tests", "host", "lr_fit_rule_host.cpp"), tmp_path_factory.mktemp("fit") / "libfitrule.so"))
    lib.fit_params.argtypes = [C.c_int, C.c_void_p]
    lib.fit_solve.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.fit_code.argtypes = [C.c_int] * 5 + [C.POINTER(C.c_uint64)]
    lib.fit_code_table.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    return lib


# ---------------------------------------------------------------- the restated filter against the oracle's
FRAMES = [(200, 120, 8, {}), (328, 248, 10, dict(deblock=1)), (202, 122, 8, dict(base_q_idx=180))]


@pytest.fixture(scope="module")
def oracle_frames(oracle):
    out = []
    for w, h, bd, kw in FRAMES:
        planes = [p.astype(np.int64) for p in oracle.synthclip_frame(w, h, bd, seed=500 + w, t=0)]
        _, pre, _ = oracle.encode_frame(oracle.default_config(w, h, bd, enable_cdef=0, enable_lr=0, **kw), planes)
        _, cdef, _ = oracle.encode_frame(oracle.default_config(w, h, bd, enable_cdef=1, enable_lr=0, **kw), planes)
        out.append((w, h, bd, kw, planes, pre, cdef))
    return out


def _oracle_sgr(oracle, w, h, bd, kw, pre, cdef, t, w0, w1):
    import av1o
    L = oracle.lib()
    L.av1o_sgr_plane.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
    L.av1o_sgr_plane.restype = None
    cfg = oracle.default_config(w, h, bd, **kw)
    fp, fc = av1o._planes_to_frame(pre), av1o._planes_to_frame(cdef)
    fo = L.av1o_frame_alloc(cfg.width, cfg.height)
    L.av1o_sgr_plane(C.byref(cfg), fp, fc, fo, t, w0, w1)
    got = av1o._frame_to_planes(fo)[0].astype(np.int64)
    for f in (fp, fc, fo):
        L.av1o_frame_free(f)
    return got


@pytest.mark.parametrize("case", range(len(FRAMES)))
def test_filter_matches_the_oracle(oracle, oracle_frames, case):
    """all 16 sets on luma; a single-radius set gets the weight the syntax implies"""
    w, h, bd, kw, planes, pre, cdef = oracle_frames[case]
    for t in range(16):
        r0, _, r1, _ = ref.SGR_PARAMS[t]
        w0, w1 = (0, 70) if not r0 else ((-20, ref.clamp(128 + 20, -32, 95)) if not r1 else (-40, 60))
        got = ref.filtered_set(pre[0][:h, :w], cdef[0][:h, :w], bd, 0, t, w0, w1)
        want = _oracle_sgr(oracle, w, h, bd, kw, pre, cdef, t, w0, w1)[:h, :w]
        assert np.array_equal(got, want), "set %d" % t


# ---------------------------------------------------------------- the rule header
def test_parameter_table(rule):
    out = (C.c_int * 4)()
    for t in range(16):
        rule.fit_params(t, out)
        assert tuple(out) == ref.SGR_PARAMS[t], t


def _solve_both(rule, probs):
    n = len(probs)
    ts = np.array([p[0] for p in probs], dtype=np.int32)
    sums = np.array([p[1] for p in probs], dtype=np.int64).reshape(n, 5)
    w = np.zeros((n, 2), dtype=np.int32)
    present = np.zeros(n, dtype=np.int32)
    rule.fit_solve(ts.ctypes.data, sums.ctypes.data, n, w.ctypes.data, present.ctypes.data)
    for i, (t, s) in enumerate(probs):
        want = ref.solve(t, s)
        got = (int(w[i, 0]), int(w[i, 1])) if present[i] else None
        assert got == want, (t, s, got, want)


def test_solve_on_frame_sums(rule, oracle_frames):
    import lr_ref
    probs = []
    for w, h, bd, kw, planes, pre, cdef in oracle_frames:
        p, c, s = (np.asarray(a[0][:h, :w], dtype=np.int64) for a in (pre, cdef, planes))
        rows, cols = lr_ref.unit_bounds(h, w, 0)
        for t in range(16):
            f0, f1 = ref.plane_outputs(p, c, bd, 0, t)
            for y0, y1 in rows:
                for x0, x1 in cols:
                    sl = (slice(y0, y1), slice(x0, x1))
                    probs.append((t, ref.unit_sums(c[sl], s[sl], f0[sl], f1[sl], t)))
    _solve_both(rule, probs)


def test_solve_on_constructed_sums(rule):
    """random sums up to 2^42 (positive-definite and not), negative numerators, det <= 0, both clamps, the refit with D > 0 and with
    D <= 0, the single-radius sets with a zero, negative or vanishing diagonal.
    For real sums of squares (H00, H11 >= 0) the rule's guard D > 0 cannot fail where the refit runs: det > 0 means
    H00 H11 > H01^2 >= 0, so (H00 + H11)^2 >= 4 H00 H11 > 4 H01^2 and D = H00 - 2 H01 + H11 > 0 - asserted for those cases.  The
    function takes any signed sums, though, and with both diagonals negative det > 0 gives H00 + H11 < -2 |H01|, that is D < 0
    (never D = 0: equality needs H01^2 >= H00 H11): kinds 6 and 7 build such sums, where the guard is what keeps x0 - without it
    the division by a negative D would round differently in C and here."""
    rng = random.Random(7)
    probs, seen = [], dict(absent=0, clamp1=0, clamp0=0, refit=0, refit_skipped=0, inside=0, neg=0, absent_r0=0, absent_r1=0, absent_shift=0)
    for it in range(6000):
        t = rng.randrange(16)
        mag = rng.choice([1 << 10, 1 << 20, 1 << 27, 1 << 34, (1 << 42) - 1])
        h00, h11 = rng.randrange(mag + 1), rng.randrange(mag + 1)
        kind = it % 9
        if kind == 0:      # anything, correlations beyond Cauchy-Schwarz included
            h01 = rng.randrange(-mag, mag + 1)
        elif kind == 1:    # singular: H01^2 = H00 H11
            a, b = rng.randrange(1, 1 << 20), rng.randrange(1, 1 << 20)
            h00, h01, h11 = a * a, a * b, b * b
        elif kind == 2:    # nearly equal outputs: D as small as it gets
            h01 = h00 = h11 = rng.randrange(1, mag + 1)
            h00 += rng.randrange(0, 3)
        else:
            h01 = int((h00 * h11) ** 0.5 * rng.uniform(-0.99, 0.99))
        c0, c1 = rng.randrange(-mag, mag + 1), rng.randrange(-mag, mag + 1)
        if kind == 4:      # weights far outside: both clamps
            c0, c1 = rng.choice([-1, 1]) * 3 * max(h00, 1), rng.choice([-1, 1]) * 3 * max(h11, 1)
        if kind == 5:      # small numerators of either sign: rounding of negative quotients
            c0, c1 = rng.randrange(-h00 // 64 - 1, 1), rng.randrange(-h11 // 64 - 1, h11 // 64 + 1)
        if kind in (6, 7):   # negative diagonals with det > 0: D < 0.  Numerators that push w outside its range, so the refit is reached
            t = rng.randrange(10)
            h00, h11 = -rng.randrange(1, mag + 1), -rng.randrange(1, mag + 1)
            h01 = int((h00 * h11) ** 0.5 * rng.uniform(-0.9, 0.9)) if kind == 6 else 0
            c0, c1 = rng.choice([-1, 1]) * 5 * abs(h00), rng.choice([-1, 1]) * rng.randrange(0, abs(h11) + 1)
        if kind == 8:        # single-radius sets: the diagonal zero, negative, or positive but gone after the normalising shift
            t = rng.randrange(10, 16)
            d = rng.choice([0, -rng.randrange(1, mag + 1), rng.randrange(1, 1 << 12)])
            big = rng.choice([1, -1]) * rng.randrange(1 << 40, 1 << 42)   # k = 15 .. 16: d >> k = 0 for d < 2^12
            h00, h01, h11, c0, c1 = (d, 0, 0, big, 0) if t >= 14 else (0, 0, d, 0, big)
        s = (h00, h01, h11, c0, c1)
        probs.append((t, s))
        # what the case exercises, restated step by step
        r0, _, r1, _ = ref.SGR_PARAMS[t]
        got = ref.solve(t, s)
        seen["absent"] += got is None
        if got is None and not (r0 and r1):
            seen["absent_r1" if r0 else "absent_r0"] += 1
            seen["absent_shift"] += (s[0] if r0 else s[2]) > 0
        seen["neg"] += c0 < 0 or c1 < 0
        if got is not None and r0 and r1:
            k = max(0, max(abs(v) for v in s).bit_length() - 26)
            H00, H01, H11, C0, C1 = (v >> k for v in s)
            det = H00 * H11 - H01 * H01
            wv = 128 - ref.rdiv(128 * (C0 * H11 - C1 * H01), det) - ref.rdiv(128 * (C1 * H00 - C0 * H01), det)
            D = H00 - 2 * H01 + H11
            if wv != got[1]:
                seen["clamp1"] += 1
                seen["refit" if D > 0 else "refit_skipped"] += 1
            assert D != 0 and (D > 0 or (h00 < 0 and h11 < 0))
            seen["clamp0"] += got[0] in (-96, 31)
            seen["inside"] += -96 < got[0] < 31 and -32 < got[1] < 95
    assert all(v > 0 for v in seen.values()), seen
    _solve_both(rule, probs)


def test_code_writer_round_trip(rule):
    """every (reference, value) pair of both weights, and every set's coded / uncoded pattern, through the spec's decoder"""
    bits = np.zeros(128 * 128, dtype=np.uint64)
    lens = np.zeros(128 * 128, dtype=np.int32)
    longest = 0
    for i in range(2):
        other = ref.XQD_MID[1 - i]
        rule.fit_code_table(9, i, other, bits.ctypes.data, lens.ctypes.data)
        for r in range(128):
            for v in range(128):
                rv, vv = ref.XQD_MIN[i] + r, ref.XQD_MIN[i] + v
                want = (9, vv, other) if i == 0 else (9, other, vv)
                rf = (rv, other) if i == 0 else (other, rv)
                n = int(lens[r * 128 + v])
                assert ref.decode_sgr_unit(int(bits[r * 128 + v]), n, rf) == want + (0,), (i, rv, vv)
                longest = max(longest, n)
    assert longest <= 22
    rng = random.Random(3)
    b = C.c_uint64()
    for t in range(16):
        r0, _, r1, _ = ref.SGR_PARAMS[t]
        for _ in range(200):
            rf = (rng.randint(-96, 31), rng.randint(-32, 95))
            x0 = rng.randint(-96, 31) if r0 else 0
            x1 = rng.randint(-32, 95) if r1 else ref.clamp(128 - x0, -32, 95)
            n = rule.fit_code(t, x0, x1, rf[0], rf[1], C.byref(b))
            assert n <= 22
            assert ref.decode_sgr_unit(b.value, n, rf) == (t, x0, x1, 0), (t, x0, x1, rf)
            # the uncoded weight costs nothing: only the coded one(s) follow the 4 bits of the set
            if not r0 or not r1:
                assert n <= 4 + 9


# ---------------------------------------------------------------- the parameter
@pytest.mark.parametrize("v", [0x102, 0x104, 0x2000104])
def test_fit_accepted(av1mi, v):
    av1mi.write_headers(av1mi.default_params(640, 360, 8, enable_lr=v))


@pytest.mark.parametrize("v", [0x100, 0x101, 0x103, 0x105, 0x204])
def test_fit_refused(av1mi, v):
    with pytest.raises(av1mi.EncodeFailed) as e:
        av1mi.write_headers(av1mi.default_params(640, 360, 8, enable_lr=v))
    assert e.value.code == 1   # AV1MI_E_INVALID_ARG


@pytest.mark.parametrize("kw", [{}, dict(film_grain=20, cdef_search=3, deblock=1), dict(width=202, height=122, bit_depth=8, cdf_update=0)])
def test_fit_headers_are_those_of_2_and_4(av1mi, kw):
    kw = dict(kw)
    w, h, bd = kw.pop("width", 1920), kw.pop("height", 1080), kw.pop("bit_depth", 10)
    for lr in (2, 4):
        plain = av1mi.write_headers(av1mi.default_params(w, h, bd, enable_lr=lr, **kw))
        for fit in (True, 1 << 9, 0xC000):
            assert av1mi.write_headers(av1mi.default_params(w, h, bd, enable_lr=lr, lr_fit=fit, **kw)) == plain
    assert av1mi.default_params(w, h, bd, enable_lr=4, lr_fit=True).enable_lr == 0x104
    assert av1mi.default_params(w, h, bd, enable_lr=2, lr_fit=0x200).enable_lr == 0x2000102 == av1mi.lr_fit_field(2, 0x200)


def test_abi_unchanged(av1mi):
    assert av1mi._lib.av1mi_abi_version() == 8 == av1mi.ABI_VERSION
    assert av1mi.struct_sizes() == av1mi.mirror_sizes()
    for name in ("av1mi_lr_fit_result", "av1mi_lr_fit_units"):
        assert name in av1mi.ABI_SYMBOLS and hasattr(av1mi._lib, name)
