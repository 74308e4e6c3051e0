"""The non-directional piece-wise predictors SMOOTH, SMOOTH_V, SMOOTH_H and PAETH (av1-base_amd/csrc/intra_pieces.h, plain_piece) compiled for
the host (tests/host/intra_pieces_host.cpp) and checked, without a GPU, against the oracle's predictor (oracle/av1o_pred.c) beyond what
tests/test_intra_pieces.py covers: N = 8, 16, 32, 64 at 8 and 10 bit, a whole wave and half a wave per block, edges of random samples,
all zero and all maximum, and a corner above and below both neighbours - Paeth's three branches - the prediction itself and the SAD."""
import ctypes as C
import os

import numpy as np
import pytest

import host_build
from test_intra_pieces import SM_WEIGHTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "intra_pieces_host.cpp")
SMOOTH, SMOOTH_V, SMOOTH_H, PAETH = 9, 10, 11, 12


@pytest.fixture(scope="module")
def pieces(tmp_path_factory):
    lib = C.CDLL(host_build.build_shared(host_build.host_cxx(), SRC, tmp_path_factory.mktemp("plain") / "libpieces.so"))
    lib.pieces_run.restype = C.c_long
    lib.pieces_run.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    return lib


def edge_sets(rng, n, maxv):
    """(name, above, left): element 0 of each is the corner, then 2 n samples"""
    m = 2 * n + 1
    rnd = lambda: rng.integers(0, maxv + 1, m)   # noqa: E731
    yield "random", rnd(), rnd()
    yield "random2", rnd(), rnd()
    yield "zero", np.zeros(m, np.int64), np.zeros(m, np.int64)
    yield "max", np.full(m, maxv), np.full(m, maxv)
    yield "zero_above_max_left", np.zeros(m, np.int64), np.full(m, maxv)
    lo, hi = maxv // 4, maxv - maxv // 4
    a, l = rng.integers(lo, hi + 1, m), rng.integers(lo, hi + 1, m)
    for name, corner in (("corner_above_both", maxv), ("corner_below_both", 0), ("corner_between", maxv // 2)):
        a2, l2 = a.copy(), l.copy()
        a2[0] = l2[0] = corner
        yield name, a2, l2
    # neighbours a step apart around the corner: the distances tie and differ by one (the <= of both tests)
    a2, l2 = (maxv // 2 + rng.integers(-2, 3, m)), (maxv // 2 + rng.integers(-2, 3, m))
    a2[0] = l2[0] = maxv // 2
    yield "near_ties", a2, l2


@pytest.mark.parametrize("n,lanes", [(8, 64), (8, 32), (16, 64), (16, 32), (32, 64), (32, 32), (64, 64)])
@pytest.mark.parametrize("bd", [8, 10])
def test_plain_pieces_equal_the_oracle_predictor(pieces, oracle, n, lanes, bd):
    L = oracle.lib()
    rng = np.random.default_rng(n * 1000 + lanes * 10 + bd)
    log2n = {8: 3, 16: 4, 32: 5, 64: 6}[n]
    maxv = (1 << bd) - 1
    smw = np.zeros(64, np.uint8)
    smw[:n] = SM_WEIGHTS[n]
    src = rng.integers(0, maxv + 1, (n, n)).astype(np.uint16)
    branches = set()
    for name, ea, el in edge_sets(rng, n, maxv):
        ea, el = ea.astype(np.uint16), el.astype(np.uint16)
        el[0] = ea[0]
        buf_a, buf_l = np.zeros(8 + 3 * n + 9, np.uint16), np.zeros(8 + 3 * n + 9, np.uint16)
        for buf, e in ((buf_a, ea), (buf_l, el)):
            buf[:7] = 0xAAAA                      # elements -8 .. -2: never part of a valid sample
            buf[7:8 + 2 * n] = e
            buf[8 + 2 * n:] = e[-1]
        pa, pl = buf_a.ctypes.data + 16, buf_l.ctypes.data + 16   # element 0
        for mode in (SMOOTH, SMOOTH_V, SMOOTH_H, PAETH):
            want = np.zeros((n, n), np.uint16)
            L.av1o_predict_intra(want.ctypes.data, n, log2n, mode, 0, ea.ctypes.data, el.ctypes.data, 1, 1, bd)
            got = np.zeros((n, n), np.uint16)
            assert pieces.pieces_run(n, lanes, mode, 0, 0, pa, pl, smw.ctypes.data, src.ctypes.data, got.ctypes.data, 1) == 0
            assert (got == want).all(), (name, mode, np.argwhere(got != want)[:4])
            sad = pieces.pieces_run(n, lanes, mode, 0, 0, pa, pl, smw.ctypes.data, src.ctypes.data, None, 0)
            assert sad == int(np.abs(src.astype(np.int64) - want.astype(np.int64)).sum()), (name, mode)
            if mode == PAETH and name.startswith("corner"):
                # which neighbour each sample took (the three values differ in these sets wherever this counts)
                A, Lc, T = ea[1:n + 1][None, :], el[1:n + 1][:, None], int(ea[0])
                distinct = (A != Lc) & (A != T) & (Lc != T)
                branches |= {"left"} if ((want == Lc) & distinct).any() else set()
                branches |= {"above"} if ((want == A) & distinct).any() else set()
                branches |= {"corner"} if ((want == T) & distinct).any() else set()
    assert branches == {"left", "above", "corner"}
