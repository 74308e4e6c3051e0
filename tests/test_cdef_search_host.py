"""CPU tests of CDEF and its strength search.  The interface (include/av1mi.h: av1mi_params.cdef_search): the parameter's range, the
frame header it implies (cdef_bits = k - 1 and 2^(k-1) strength pairs) and the ABI layout with the new last field.  The shared pieces
(av1-base_amd/csrc/cdef_pieces.h) compiled for the host (tests/host/cdef_pieces_host.cpp): the filter against oracle/av1o_cdef.c, the
search's 24 errors per superblock against 16 oracle runs at fixed strengths, the candidate pool against P8.  All comparisons are exact."""
import ctypes as C
import os

import numpy as np
import pytest

import host_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "cdef_pieces_host.cpp")
U16P = C.POINTER(C.c_uint16)
P8 = [0, 1, 2, 3, 4, 6, 8, 11]   # the pool's primary strengths (tests/test_cdef_search.py)


@pytest.fixture(scope="module")
def av1mi():
    return host_build.library()


def _bits(data, n):
    return [(data[i >> 3] >> (7 - (i & 7))) & 1 for i in range(n)]


def _headers(av1mi, k, **kw):
    p = av1mi.default_params(kw.pop("w", 1920), kw.pop("h", 1080), kw.pop("bd", 10), cdef_search=k, **kw)
    return av1mi.write_headers(p)


@pytest.mark.parametrize("k", [0, 1, 2, 3, 4])
def test_cdef_search_accepted(av1mi, k):
    p = av1mi.default_params(640, 360, 8, cdef_search=k)
    assert p.cdef_search == k
    av1mi.write_headers(p)


def test_cdef_search_refused(av1mi):
    with pytest.raises(av1mi.EncodeFailed) as e:
        av1mi.write_headers(av1mi.default_params(640, 360, 8, cdef_search=5))
    assert e.value.code == 1   # AV1MI_E_INVALID_ARG
    with pytest.raises(av1mi.EncodeFailed) as e:
        av1mi.write_headers(av1mi.default_params(640, 360, 8, cdef_search=1, enable_cdef=0))
    assert e.value.code == 1
    av1mi.write_headers(av1mi.default_params(640, 360, 8, cdef_search=0, enable_cdef=0))


@pytest.mark.parametrize("kw", [{}, dict(film_grain=20, deblock=1, enable_lr=2, enable_qm=1), dict(w=328, h=200, bd=8, cdf_update=0),
                                dict(w=3840, h=2160, tile_sb=2, cdef_damping=4, cdef_y_pri=5, cdef_y_sec=1)])
def test_cdef_search_header_layout(av1mi, kw):
    seq0, fh0, bits0 = _headers(av1mi, 0, **dict(kw))
    seq1, fh1, bits1 = _headers(av1mi, 1, **dict(kw))
    assert (seq1, fh1, bits1) == (seq0, fh0, bits0)   # one pair: cdef_bits 0, the same bytes as without the search
    fh2 = _headers(av1mi, 2, **dict(kw))[1]
    b1, b2 = _bits(fh1, bits1), _bits(fh2, bits1)
    d = next(i for i in range(bits1) if b1[i] != b2[i])
    # cdef_bits is the 2-bit field in front of the strengths: 00 for k = 1, 01 for k = 2
    cb = d - 1
    assert b1[cb:cb + 2] == [0, 0] and b2[cb:cb + 2] == [0, 1]
    str_bit = cb + 2
    for k in (2, 3, 4):
        _, fh, bits = _headers(av1mi, k, **dict(kw))
        n = 1 << (k - 1)
        assert bits == bits1 + 12 * (n - 1)
        b = _bits(fh, bits)
        assert b[:cb] == b1[:cb]
        assert b[cb] * 2 + b[cb + 1] == k - 1
        # the placeholders: the fixed strengths, n times; everything after them as without the search
        for j in range(n):
            assert b[str_bit + 12 * j:str_bit + 12 * (j + 1)] == b1[str_bit:str_bit + 12]
        assert b[str_bit + 12 * n:] == b1[str_bit + 12:]


def test_cdef_search_layout(av1mi):
    sizes = av1mi.struct_sizes()
    assert sizes == av1mi.mirror_sizes()
    assert av1mi.Params.cdef_search.offset == C.sizeof(av1mi.Params) - 4 == av1mi.Params.me_presearch.offset + 4
    assert sizes[0] == C.sizeof(av1mi.Params) == 36 * 4
    assert av1mi.ABI_VERSION == int(av1mi._lib.av1mi_abi_version()) == 8


# ---------------------------------------------------------------- the pieces on the host
@pytest.fixture(scope="module")
def cxx():
    return host_build.host_cxx()


@pytest.fixture(scope="module")
def pieces(cxx, tmp_path_factory):
    lib = C.CDLL(host_build.build_shared(cxx, SRC, tmp_path_factory.mktemp("cdef") / "libcdefpieces.so"))
    lib.cdef_frame.argtypes = [U16P] * 6 + [C.c_int] * 8 + [C.c_void_p, C.c_void_p]
    lib.cdef_frame.restype = None
    lib.cdef_search_errors.argtypes = [U16P] * 6 + [C.c_int] * 6 + [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.cdef_search_errors.restype = None
    lib.cdef_pair_strengths.argtypes = [C.c_int, C.POINTER(C.c_int)]
    lib.cdef_pair_bits.restype = C.c_uint
    lib.cdef_pair_err.argtypes = [C.POINTER(C.c_uint64), C.c_int]
    lib.cdef_pair_err.restype = C.c_uint64
    return lib


# signalled size, coded size
SIZES = [((8, 8), (8, 8)), ((72, 56), (72, 56)), ((200, 136), (200, 136)), ((202, 122), (208, 128))]
# beside the pool: cdef_y_sec 1 and 3, cdef_uv_sec 2 and 3, cdef_y_pri 15 (y_pri, y_sec, uv_pri, uv_sec)
EXTRA = [(15, 1, 11, 2), (15, 3, 6, 3), (5, 3, 0, 2), (0, 1, 15, 3)]


def pair_fields(p):
    l, c = p >> 3, p & 7
    return (P8[l >> 1], 2 * (l & 1), P8[c], 0)


_scenes = {}


def scene(oracle, tw, th, w, h, bd):
    """source: synthclip; reconstruction: the source plus 8x8-blocky noise of +-6 << (bd - 8) (test_deblock_search_host.py::content);
    skip map: a quarter of the 8x8 blocks at random, and one whole superblock where there is more than one.  Built once per case."""
    key = (tw, th, w, h, bd)
    if key not in _scenes:
        rng = np.random.default_rng(w * 131 + h * 7 + bd)
        src = [np.ascontiguousarray(p.astype(np.uint16)) for p in oracle.synthclip_frame(w, h, bd, seed=w + h, t=1)]
        amp = 6 << (bd - 8)
        rec = []
        for pl in src:
            ph, pw = pl.shape
            blocky = np.kron(rng.integers(-amp, amp + 1, ((ph + 7) // 8, (pw + 7) // 8)), np.ones((8, 8), dtype=np.int64))[:ph, :pw] // 2
            rec.append(np.ascontiguousarray(np.clip(pl.astype(np.int64) + blocky + rng.integers(-amp // 2, amp // 2 + 1, (ph, pw)), 0, (1 << bd) - 1).astype(np.uint16)))
        skip8 = (rng.integers(4, size=(h // 8, w // 8)) == 0).astype(np.uint8)
        sb_rows, sb_cols = -(-h // 64), -(-w // 64)
        if sb_rows * sb_cols > 1:
            skip8[-(h // 8 - (sb_rows - 1) * 8):, -(w // 8 - (sb_cols - 1) * 8):] = 1   # the last superblock: nothing coded
        skip8 = np.ascontiguousarray(skip8)
        idx = np.array([-1 if skip8[r * 8:r * 8 + 8, c * 8:c * 8 + 8].all() else 0 for r in range(sb_rows) for c in range(sb_cols)], dtype=np.int8)
        assert (idx >= 0).any() and (sb_rows * sb_cols == 1 or idx[-1] == -1)
        _scenes[key] = (src, rec, skip8, idx, {})
    return _scenes[key]


def oracle_cdef(oracle, sc, w, h, tw, th, bd, damping, fields):
    """av1o_cdef_frame of the scene's reconstruction at fixed strengths (kept per scene: the filter and the search tests share the runs)"""
    src, rec, skip8, idx, runs = sc
    key = (damping,) + tuple(fields)
    if key not in runs:
        L = oracle.lib()
        cfg = oracle.default_config(w, h, bd, true_width=tw, true_height=th, cdef_damping=damping, enable_cdef=1, cdef_y_pri=fields[0],
                                    cdef_y_sec=fields[1], cdef_uv_pri=fields[2], cdef_uv_sec=fields[3])
        fin, fout = oracle._planes_to_frame(rec), L.av1o_frame_alloc(w, h)
        skip_mi = np.ascontiguousarray(np.kron(skip8, np.ones((2, 2), dtype=np.uint8)))
        L.av1o_cdef_frame(C.byref(cfg), fin, fout, skip_mi.ctypes.data, w // 4, idx.ctypes.data)
        runs[key] = oracle._frame_to_planes(fout)
        L.av1o_frame_free(fin)
        L.av1o_frame_free(fout)
    return runs[key]


def pieces_cdef(pieces, sc, w, h, bd, damping, fields):
    src, rec, skip8, idx, _ = sc
    out = [np.zeros_like(p) for p in rec]
    pieces.cdef_frame(*(p.ctypes.data_as(U16P) for p in rec + out), w, h, bd, damping, *fields, skip8.ctypes.data, idx.ctypes.data)
    return out


CASES = [(tw, th, w, h, bd, damping) for (tw, th), (w, h) in SIZES for bd in (8, 10) for damping in (3, 4, 5, 6)]


@pytest.mark.parametrize("tw,th,w,h,bd,damping", CASES)
def test_filter_through_the_pieces_equals_the_oracle(pieces, oracle, tw, th, w, h, bd, damping):
    """direction, adjusted strength and the sample filter piece (av1mi_cdef_sample on av1mi_cdef_tap's taps; cdef_rows keeps a loop of its
    own from the same weight, constrain and finish pieces, which the GPU tests cover) against av1o_cdef_frame: all 128 pairs of the pool
    and the strengths outside it"""
    sc = scene(oracle, tw, th, w, h, bd)
    rec = sc[1]
    sets = [pair_fields(p) for p in range(128)] + EXTRA
    moved = 0
    for fields in sets:
        want, got = oracle_cdef(oracle, sc, w, h, tw, th, bd, damping, fields), pieces_cdef(pieces, sc, w, h, bd, damping, fields)
        for pl in range(3):
            assert np.array_equal(got[pl], want[pl]), "plane %d, strengths %s" % (pl, fields)
            moved += int((want[pl] != rec[pl]).sum())
    assert moved > 0
    # luma candidate 1 (secondary only) moves at least one sample of the frame
    assert (oracle_cdef(oracle, sc, w, h, tw, th, bd, damping, pair_fields(8))[0] != rec[0]).any()


def sb_sse(a, b, size, cw, ch):
    """per superblock (raster order) the squared error of two planes over the counted size cw x ch, superblocks of size x size samples"""
    d = (a.astype(np.int64) - b.astype(np.int64))[:ch, :cw] ** 2
    rows, cols = -(-a.shape[0] // size), -(-a.shape[1] // size)
    return np.array([int(d[r * size:(r + 1) * size, c * size:(c + 1) * size].sum()) for r in range(rows) for c in range(cols)], dtype=np.uint64)


@pytest.mark.parametrize("tw,th,w,h,bd,damping", CASES)
def test_search_errors_equal_sixteen_oracle_runs(pieces, oracle, tw, th, w, h, bd, damping):
    """the table as the kernel forms it - primary and secondary sums once, the candidates from them, counted over the signalled size -
    against oracle run i = luma candidate i, chroma candidate i mod 8"""
    sc = scene(oracle, tw, th, w, h, bd)
    src, rec, skip8, idx, _ = sc
    nsb = len(idx)
    err, got_idx = np.zeros((nsb, 24), dtype=np.uint64), np.zeros(nsb, dtype=np.int8)
    pieces.cdef_search_errors(*(p.ctypes.data_as(U16P) for p in rec + src), w, h, tw, th, bd, damping, skip8.ctypes.data, err.ctypes.data,
                              got_idx.ctypes.data)
    assert np.array_equal(got_idx, idx)
    want = np.zeros((nsb, 24), dtype=np.uint64)
    for i in range(16):
        out = oracle_cdef(oracle, sc, w, h, tw, th, bd, damping, pair_fields(8 * i + i % 8))
        want[:, i] = sb_sse(out[0], src[0], 64, tw, th)
        if i < 8:
            want[:, 16 + i] = sb_sse(out[1], src[1], 32, tw // 2, th // 2) + sb_sse(out[2], src[2], 32, tw // 2, th // 2)
        else:   # the second run of a chroma candidate gives what the first gave
            assert np.array_equal(want[:, 8 + i], sb_sse(out[1], src[1], 32, tw // 2, th // 2) + sb_sse(out[2], src[2], 32, tw // 2, th // 2))
    want[idx < 0] = 0   # nothing coded: the errors stay 0
    assert np.array_equal(err, want)
    # the inputs discriminate between the candidates
    for sb in np.flatnonzero(idx >= 0):
        assert len(set(err[sb, :16].tolist())) >= 8 and len(set(err[sb, 16:].tolist())) >= 6, (sb, err[sb])
    e = err[int(np.flatnonzero(idx >= 0)[0])]
    for p in (0, 9, 77, 127):
        assert pieces.cdef_pair_err(e.ctypes.data_as(C.POINTER(C.c_uint64)), p) == int(e[p >> 3]) + int(e[16 + (p & 7)])


def test_pool(pieces):
    """pair -> the four strength fields and pair -> the header's 12 bits, all 128 pairs"""
    seen = set()
    for p in range(128):
        out = (C.c_int * 4)()
        pieces.cdef_pair_strengths(p, out)
        want = pair_fields(p)
        assert tuple(out) == want
        assert pieces.cdef_pair_bits(p) == (want[0] << 8) | (want[1] << 6) | (want[2] << 2) | want[3] < 4096
        seen.add(want)
    assert len(seen) == 128


def test_standalone_program(cxx, tmp_path):
    """the same source as a program with its own main: the search's errors are the filter's at every candidate's strengths"""
    out = host_build.run_program(cxx, SRC, tmp_path / "cdef_main", defines=["CDEF_PIECES_MAIN"])
    assert out.returncode == 0 and " 0 mismatches" in out.stdout, out.stdout + out.stderr


def test_standalone_program_under_sanitizers(cxx, tmp_path):
    """... and under AddressSanitizer and UndefinedBehaviorSanitizer (host code only).  Skipped only where an empty program does not
    build and run under the sanitizers - their runtimes are not installed; a failure of the project's source is a failure"""
    out = host_build.run_program(cxx, SRC, tmp_path / "cdef_main_san", defines=["CDEF_PIECES_MAIN"], sanitized=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert " 0 mismatches" in out.stdout
