"""CPU check of the inputs tests/test_lr_edges.py feeds the GPU - that the edge matrix reaches the states it is for.  By the pattern
of tests/test_lr_rd_content.py: the restatement (tests/lr_rd_ref.py) runs on the oracle's pre-CDEF and CDEF planes of both key frames of
every case of tests/lr_edge_cases.py, at the case's parameters and unit sizes, and the tallies per case are printed.  Each test below
asserts one condition across the cases; together they keep the matrix from going soft when content or parameters change.

The product's own decisions on its own planes are asserted against the restatement where it runs, in the GPU test."""
import pytest

import lr_edge_cases as M
import lr_rd_ref as ref
import lr_unit_ref as uref
import wiener_fit_ref as wref

FIELDS = ("units", "wiener_absent_luma", "wiener_absent_chroma", "sgr_absent_8", "fitted_absent_17", "taps_all_clamped_luma", "taps_all_zero",
          "refit", "moved_by_lambda", "off_by_lambda", "kept_23_at_largest_lambda", "chose_fitted_set", "units_below_16_rows")
LARGEST = ref.lam(255, 10, 3)


def tally_case(oracle, case):
    t = dict.fromkeys(FIELDS, 0)
    t.update(wiener_sum_max=0, sgr_sum_max=[0] * 16, lambdas=set(), narrowest_plane=1 << 30, choices=set())
    bd = case["bd"]
    for f in range(2):
        src, pre, cdef = M.oracle_planes(oracle, case, f)
        for pl in range(3):
            sub = int(pl > 0)
            t["narrowest_plane"] = min(t["narrowest_plane"], src[pl].shape[1])
            for shift in case["shifts"]:
                cands = M.candidates(pre[pl], cdef[pl], src[pl], bd, sub, shift)
                units = M.probe(pre[pl], cdef[pl], src[pl], bd, sub, shift)
                for i, row in enumerate(cands["err"]):
                    for j, err in enumerate(row):
                        coef, u = cands["coef"][i][j], units[i][j]
                        absent = [c for c in range(7, 24) if err[c] is None]
                        t["units"] += 1
                        t["wiener_absent_chroma" if sub else "wiener_absent_luma"] += 23 in absent
                        t["sgr_absent_8"] += len([c for c in absent if c < 23]) >= 8
                        t["fitted_absent_17"] += len(absent) == 17
                        if 23 in coef:
                            taps = [(k, v) for p in coef[23] for k, v in enumerate(p) if k >= sub]
                            t["taps_all_clamped_luma"] += (not sub) and all(v in (wref.TAPS_MIN[k], wref.TAPS_MAX[k]) for k, v in taps)
                            t["taps_all_zero"] += all(v == 0 for k, v in taps)
                        t["refit"] += bool(u["winfo"]["v"].get("refit") or u["winfo"].get("h", {}).get("refit"))
                        t["units_below_16_rows"] += u["rows"] < 16
                        t["wiener_sum_max"] = max(t["wiener_sum_max"], max(abs(v) for v in u["wsums"]))
                        for s in range(16):
                            t["sgr_sum_max"][s] = max(t["sgr_sum_max"][s], max(abs(v) for v in u["ssums"][s]))
                for low in M.LOW:
                    if not M.restored(pl, low):
                        continue
                    c = ref.view(cands, shift << 12 | low)
                    a = ref.restore_rd(c, 0)[1]
                    t["choices"] |= set(int(x) for x in a.ravel())
                    for s in case["scales"]:
                        lam = M.lam(case, s)
                        t["lambdas"].add(lam)
                        b = ref.restore_rd(c, lam)[1]
                        t["choices"] |= set(int(x) for x in b.ravel())
                        t["moved_by_lambda"] += int((a != b).sum())
                        t["off_by_lambda"] += int(((a != 0) & (b == 0)).sum())
                        t["chose_fitted_set"] += int((((a >= 7) & (a < 23)) | ((b >= 7) & (b < 23))).sum())
                        if lam == LARGEST:
                            t["kept_23_at_largest_lambda"] += int((b == 23).sum())
    return t


@pytest.fixture(scope="module")
def tallies(oracle):
    out = {}
    for case in M.CASES:
        out[case["name"]] = t = tally_case(oracle, case)
        print(case["name"], {k: t[k] for k in FIELDS if t[k]}, "choices", sorted(t["choices"]), "lambdas", sorted(t["lambdas"]),
              "narrowest plane", t["narrowest_plane"], "max |Wiener sum| 2^%.2f" % _log2(t["wiener_sum_max"]),
              "max |self-guided sum| 2^%.2f (set %d)" % (_log2(max(t["sgr_sum_max"])), t["sgr_sum_max"].index(max(t["sgr_sum_max"]))))
    uref.forget()
    return out


def _log2(v):
    import math
    return math.log2(v) if v else float("-inf")


def _total(tallies, field):
    return sum(t[field] for t in tallies.values())


@pytest.mark.parametrize("field", ["wiener_absent_luma", "wiener_absent_chroma", "sgr_absent_8", "fitted_absent_17", "taps_all_clamped_luma", "taps_all_zero",
                                   "refit", "moved_by_lambda", "off_by_lambda", "kept_23_at_largest_lambda", "chose_fitted_set", "units_below_16_rows"])
def test_a_unit_reaches_the_state(tallies, field):
    """a luma and a chroma unit without the fitted Wiener candidate; a unit with 8 or more self-guided sets absent; one with all 17 fitted
    candidates absent; a luma unit with all six fitted taps at TAPS_MIN / TAPS_MAX; a unit with all-zero fitted taps; one in which the
    refit ran; one whose choice differs between lambda 0 and lambda > 0, one that goes off; one that keeps choice 23 at the largest
    lambda; one that chooses a fitted self-guided set; one of fewer than 16 rows"""
    assert _total(tallies, field) >= 1, {k: t[field] for k, t in tallies.items()}


def test_the_fitted_wiener_candidate_is_absent_beside_present_self_guided_sets(tallies, oracle):
    """the 16x8 case: a unit without candidate 23 that has a fitted self-guided set"""
    case = next(c for c in M.CASES if (c["w"], c["h"]) == (16, 8))
    seen = 0
    for f in range(2):
        src, pre, cdef = M.oracle_planes(oracle, case, f)
        for pl in range(3):
            cands = M.candidates(pre[pl], cdef[pl], src[pl], case["bd"], int(pl > 0), 0)
            seen += sum(u[23] is None and any(e is not None for e in u[7:23]) for row in cands["err"] for u in row)
    uref.forget()
    assert seen >= 1


def test_sums_outgrow_36_and_32_bits(tallies):
    """A Wiener sum of magnitude >= 2^36 (wiener_fit_rule.h bounds them by 2^40 at units of 256) and a self-guided sum that does not
    fit 32 bits, over all 16 sets.  Measured on the oracle's planes of 392x264 10-bit checker1 at cq 63 with 8x8 leaves and units of
    256: max |Wiener sum| = 2^37.06; max |self-guided sum| per set 0 .. 15 = 2^24.24, 24.89, 25.55, 25.78, 27.56, 29.46, 30.43, 31.59,
    31.94, 32.35, 23.29, 24.40, 27.69, 27.70, 29.85, 32.46 - sets 9 and 15 outgrow 32 bits, by a third of a bit and more.  (With
    32x32 leaves the same frame stays at 2^31.63, with 16x16 leaves it reaches 2^32.06: the 8x8 leaves are there for the margin.)"""
    wmax = max(t["wiener_sum_max"] for t in tallies.values())
    smax = [max(t["sgr_sum_max"][s] for t in tallies.values()) for s in range(16)]
    print("max |Wiener sum| 2^%.2f; max |self-guided sum| per set" % _log2(wmax), ["2^%.2f" % _log2(v) for v in smax])
    assert wmax >= 1 << 36
    assert wmax < 1 << 40   # the bound the rule's 63-bit arithmetic rests on
    assert max(smax) >= 1 << 32


def test_lambda_at_both_ends(tallies):
    lams = set().union(*(t["lambdas"] for t in tallies.values()))
    assert 1 in lams and LARGEST in lams, sorted(lams)
    assert LARGEST == 1451856


def test_small_geometry():
    """a restored plane narrower than 8 columns; a frame smaller than its unit at shifts 1 and 2"""
    assert any(c["w"] // 2 < 8 for c in M.CASES)
    for shift in (1, 2):
        assert any(shift in c["shifts"] and c["w"] < 64 << shift and c["h"] < 64 << shift for c in M.CASES), shift
