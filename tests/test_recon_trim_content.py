"""CPU check of the content tests/test_recon_trim.py feeds the GPU: where the levels of its `row_impulses` frames fall, and how large the
levels of its noise frames get - by the oracle's forward transforms (oracle/av1o_txfm.c) and the quantiser rule on the residual against
a flat prediction (what the encoder predicts differs from the block's mean by a constant over these frames' blocks, which moves the DC
coefficient only).

 * every whole 32x32 luma block with frequency k > 0 has its last nonzero level, in scan order, at (row k, column 0), every 16x16 chroma
   block at (row 0, column k); over the GPU test's cases the luma rows cover 1 .. 31 - each of the 16 accumulator registers of both wave
   halves of the matrix-core quantiser holds the last level of some block - and the chroma columns 1 .. 15, both lanes of a row;
 * the noise frames at the lowest quantiser index leave no zero level in a block, and their largest level stays far below the 0x7FFF
   cap: the cap cannot be reached through the transform at 8 or 10 bit (tests/test_quant_pieces_host.py reaches it)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import edge_content as E
import test_recon_trim as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32P = C.POINTER(C.c_int32)


def table(name):
    txt = open(os.path.join(ROOT, "av1-base_amd", "csrc", "av1_tables.h")).read()
    return [int(x) for x in re.search(name + r"\[256\]\s*=\s*\{([^}]*)\}", txt).group(1).replace("\n", " ").split(",") if x.strip()]


def of_block(block):
    return block.astype(np.int64) - int(np.rint(block.mean()))


def levels(oracle, resid, plane, bd, qidx):
    """quantised levels of a residual block, by the oracle's transform of the plane and size and the rule of DESIGN.md §3.5"""
    L = oracle.lib()
    L.av1o_fwd_dct32x32_matrix.argtypes = [I32P, C.c_int, I32P]
    L.av1o_fwd_txfm2d.argtypes = [I32P, C.c_int, I32P, C.c_int, C.c_int, C.c_int]
    n = resid.shape[0]
    resid = np.ascontiguousarray(resid.astype(np.int32))
    coef = np.zeros((n, n), np.int32)
    if plane == 0:
        L.av1o_fwd_dct32x32_matrix(resid.ctypes.data_as(I32P), n, coef.ctypes.data_as(I32P))
    else:
        L.av1o_fwd_txfm2d(resid.ctypes.data_as(I32P), n, coef.ctypes.data_as(I32P), 4, 0, bd)
    dcq, acq = table("av1_dc_q%d" % bd)[qidx], table("av1_ac_q%d" % bd)[qidx]
    sh = 1 if n == 32 else 0
    out = np.zeros((n, n), np.int64)
    for i in range(n):
        for j in range(n):
            q = acq if (i | j) else dcq
            rnd = (3 * q) >> 3 if i + j < n // 4 else (q >> 2 if i + j < n // 2 else q >> 3)
            out[i, j] = min((((abs(int(coef[i, j])) << sh) + rnd) * ((2 ** 32 + q - 1) // q)) >> 32, 0x7FFF)
    return out


def last_nonzero(lv):
    """(row, column) of the last nonzero level in scan order: by anti-diagonal, odd ones by increasing row, even ones by increasing column"""
    pos = [(((i + j) << 6) | (i if (i + j) & 1 else j), i, j) for i, j in np.argwhere(lv)]
    return max(pos)[1:] if pos else None


def whole_blocks(plane, n):
    h, w = plane.shape
    for by in range(h // n):
        for bx in range(w // n):
            yield bx, by, plane[by * n:(by + 1) * n, bx * n:(bx + 1) * n]


def test_row_impulses_put_the_last_level_in_every_register_row_and_column(oracle):
    rows, cols = set(), set()
    for w, h in T.SIZES:
        for bd in (10, 8):
            for mask in T.MASKS:
                k0 = T.impulse_k0(w, h, bd, mask)
                for t in range(T.N):
                    f = T.row_impulses(w, h, bd, t, k0)
                    for pl, n in ((0, 32), (1, 16), (2, 16)):
                        for bx, by, blk in whole_blocks(f[pl], n):
                            k = T.impulse_k(bx, by, pl, n, t, k0)
                            if k == 0:
                                continue
                            assert last_nonzero(levels(oracle, of_block(blk), pl, bd, E.QINDEX[30])) == ((k, 0) if pl == 0 else (0, k)), (w, h, bd, t, pl, bx, by, k)
                            (rows if pl == 0 else cols).add(k)
    assert rows == set(range(1, 32))
    assert cols == set(range(1, 16))


@pytest.mark.parametrize("bd", [10, 8])
def test_noise_fills_every_level_and_stays_below_the_cap(oracle, bd):
    w, h = T.SIZES[-1]
    rng = np.random.default_rng(5)
    top = 0
    for t in range(T.N):
        f = T.noise(rng, w, h, bd, t)
        for pl, n in ((0, 32), (1, 16)):
            for bx, by, blk in whole_blocks(f[pl], n):
                lv = levels(oracle, of_block(blk), pl, bd, E.QINDEX[1])
                assert (lv[1:, 1:] != 0).mean() > 0.95   # practically every lane's every register holds a level
                top = max(top, int(lv.max()))
    # a block at one extreme predicted from the other - a residual of maxv everywhere - gives the largest DC level there can be
    bound = int(levels(oracle, np.full((32, 32), E.maxv_of(bd)), 0, bd, E.QINDEX[1]).max())
    assert top <= bound < 0x7FFF
