"""CPU check of the inputs tests/test_lr_unit.py feeds the GPU - that they do what they are for.  The restatement at the unit size
(tests/lr_unit_ref.py) runs on the oracle's pre-CDEF and CDEF planes of the first key frame of every case, at the cases' own parameters:

 * at each of shifts 1 and 2, at least a third of the units hold cells (units of shift 0) that do not all share the unit's choice among
   the fixed candidates - a product that decided per cell and stored the result per unit would not pass;
 * at shift 2 at least two luma units and two chroma units take the fitted Wiener filter (choice 23) and at least four units a fitted
   self-guided set; at shift 1 at least ten units take 23.

The product's own decisions on its own planes are asserted against the restatement where it runs, in the GPU test."""
import numpy as np
import pytest

import edge_content as E
import lr_unit_ref as uref
import test_lr_unit as T


def oracle_planes(oracle, ci):
    """(source, pre-CDEF, CDEF) planes of a case's first frame at the signalled size"""
    w, h, bd, extra = T.KEY_CASES[ci][:4]
    src = T.case_frames(oracle, ci, 1)[0]
    out = []
    for cdef in (0, 1):
        case = dict(w=w, h=h, bd=bd, params=dict(extra, enable_cdef=cdef))
        out.append(oracle.encode_frame(E.oracle_config(oracle, case, 0), src)[1])
    crop = lambda planes: [np.asarray(p[:(h + (i > 0)) >> (i > 0), :(w + (i > 0)) >> (i > 0)], dtype=np.int64) for i, p in enumerate(planes)]
    return crop(src), crop(out[0]), crop(out[1])


@pytest.fixture(scope="module")
def tallies(oracle):
    """per shift: units, units whose cells do not all share the unit's fixed choice (enable_lr 4), and under fit | 4 | W the luma and
    chroma units choosing 23 and the units choosing a fitted self-guided set"""
    tot = {s: dict(units=0, mixed=0, w23_luma=0, w23_chroma=0, fitted=0) for s in (1, 2)}
    for ci, case in enumerate(T.KEY_CASES):
        src, pre, cdef = oracle_planes(oracle, ci)
        bd = case[2]
        for pl in range(3):
            sub = int(pl > 0)
            cells = uref.restore_value(pre[pl], cdef[pl], src[pl], bd, sub, 4)["choice"]
            for s in case[5]:
                fixed = uref.restore_value(pre[pl], cdef[pl], src[pl], bd, sub, s << 12 | 4)["choice"]
                for (i, j), k in np.ndenumerate(fixed):
                    part = cells[i << s:cells.shape[0] if i == fixed.shape[0] - 1 else (i + 1) << s, j << s:cells.shape[1] if j == fixed.shape[1] - 1 else (j + 1) << s]
                    tot[s]["units"] += 1
                    tot[s]["mixed"] += bool((part != k).any())
                final = uref.restore_value(pre[pl], cdef[pl], src[pl], bd, sub, s << 12 | 0x504)
                tot[s]["w23_chroma" if sub else "w23_luma"] += int((final["choice"] == 23).sum())
                tot[s]["fitted"] += int(((final["choice"] >= 7) & (final["choice"] < 23)).sum())
    uref.forget()
    print(tot)
    return tot


@pytest.mark.parametrize("s", [1, 2])
def test_units_mix_their_cells_choices(tallies, s):
    assert 3 * tallies[s]["mixed"] >= tallies[s]["units"], tallies[s]


def test_fits_win_units_of_256(tallies):
    assert tallies[2]["w23_luma"] >= 2 and tallies[2]["w23_chroma"] >= 2, tallies[2]
    assert tallies[2]["fitted"] >= 4, tallies[2]


def test_wiener_fit_wins_units_of_128(tallies):
    assert tallies[1]["w23_luma"] + tallies[1]["w23_chroma"] >= 10, tallies[1]
