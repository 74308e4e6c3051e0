"""CPU check of the inputs tests/test_lr_rd.py feeds the GPU - that they make the rate term act.  The restated rule (tests/lr_rd_ref.py)
runs on the oracle's pre-CDEF and CDEF planes of both key frames of every case, at the cases' own parameters and unit sizes (the oracle
has no chroma restoration; its chroma planes before restoration are all the rule needs).  Across the cases at s = 0 and s = 1:

 * at least one unit goes off that the error alone filters, at least one keeps a filter, at least one moves to a different filter;
 * at least one Wiener unit survives in a Wiener-only mode (at s = 1: at the nominal lambda none of these clips keeps one);
 * the 200x120 case alone meets the first three on luma at either scale, and its bytes change under the fixed candidates too.

The product's own decisions on its own planes are asserted against the restatement where it runs, in the GPU test."""
import numpy as np
import pytest

import edge_content as E
import lr_rd_ref as ref
import lr_unit_ref as uref
import test_lr_rd as T


def oracle_planes(oracle, ci, f):
    """(source, pre-CDEF, CDEF) planes of frame f of a case at the signalled size"""
    w, h, bd, extra = T.KEY_CASES[ci][:4]
    src = T.case_frames(oracle, ci)[f]
    out = []
    for cdef in (0, 1):
        case = dict(w=w, h=h, bd=bd, params=dict(extra, enable_cdef=cdef))
        out.append(oracle.encode_frame(E.oracle_config(oracle, case, 0), src)[1])
    crop = lambda planes: [np.asarray(p[:(h + (i > 0)) >> (i > 0), :(w + (i > 0)) >> (i > 0)], dtype=np.int64) for i, p in enumerate(planes)]
    return crop(src), crop(out[0]), crop(out[1])


def tally(cands, v, lam, into):
    c = ref.view(cands, v)
    a, b = ref.restore_rd(c, 0)[1], ref.restore_rd(c, lam)[1]
    into["units"] += a.size
    into["off"] += int(((a != 0) & (b == 0)).sum())
    into["kept"] += int(((a != 0) & (b != 0)).sum())
    into["moved"] += int(((a != 0) & (b != 0) & (b != a)).sum())
    into["on"] += int(((a == 0) & (b != 0)).sum())
    into["wiener_left"] += int((((b >= 1) & (b <= 3)) | (b == 23)).sum())


@pytest.fixture(scope="module")
def tallies(oracle):
    """per (case, mode, scale): the units, those the rule switches off, keeps, moves, switches on, and the Wiener units it leaves"""
    tot = {}
    for ci, case in enumerate(T.KEY_CASES):
        w, h, bd, extra, shift = case[:5]
        for f in range(2):
            src, pre, cdef = oracle_planes(oracle, ci, f)
            for pl in range(3):
                cands = ref.candidates(pre[pl], cdef[pl], src[pl], bd, int(pl > 0), shift << 12 | T.FIT4 | T.W)
                for low in T.LOW:
                    if pl and (low & 0xFF) in (1, 2):
                        continue
                    for s in T.SCALES:
                        key = (ci, low, s, "luma" if pl == 0 else "chroma")
                        tally(cands, shift << 12 | low, T.case_lambda(ci, s), tot.setdefault(key, dict(units=0, off=0, kept=0, moved=0, on=0, wiener_left=0)))
    uref.forget()
    for k in sorted(tot):
        print("case %d lr %#x s %d %s" % k, tot[k])
    return tot


def _sum(tallies, field, pred):
    return sum(v[field] for k, v in tallies.items() if pred(*k))


@pytest.mark.parametrize("s", T.SCALES)
def test_the_rule_acts_across_the_cases(tallies, s):
    for field in ("off", "kept", "moved"):
        assert _sum(tallies, field, lambda ci, low, sc, kind: sc == s) >= 1, field
    assert _sum(tallies, "on", lambda ci, low, sc, kind: True) == 0   # a unit the error leaves off has the cheapest symbol as well


def test_a_wiener_unit_survives_in_a_wiener_only_mode(tallies):
    assert _sum(tallies, "wiener_left", lambda ci, low, sc, kind: (low & 0xFF) in (1, 3)) >= 1
    assert _sum(tallies, "wiener_left", lambda ci, low, sc, kind: low in (1, 3)) >= 1   # ... a fixed filter among them


@pytest.mark.parametrize("s", T.SCALES)
def test_200x120_luma_meets_all_three_under_the_fit(tallies, s):
    t = tallies[(1, T.FIT4, s, "luma")]
    assert t["off"] >= 1 and t["kept"] >= 1 and t["moved"] >= 1, t


@pytest.mark.parametrize("s", T.SCALES)
@pytest.mark.parametrize("low", [4, T.FIT4 | T.W])
def test_200x120_changes_its_units(tallies, low, s):
    """what test_deterministic_and_differs_from_the_mode_off relies on"""
    assert sum(tallies[(1, low, s, kind)]["off"] + tallies[(1, low, s, kind)]["moved"] for kind in ("luma", "chroma")) >= 1
