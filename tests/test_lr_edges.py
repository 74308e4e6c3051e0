"""GPU tests of the restoration decisions at the edge matrix (tests/lr_edge_cases.py): 8x8 and 8-sample-thin frames, cq 1 and 63,
full-range checkers, impulses, steps and flat planes in 8 and 10 bit, at units of 64, 128 and 256, through the self-guided fit
(lr_fit_kernel.hip), the Wiener fit (lr_wfit_kernel.hip) and the rate term (lr_rate_rule.h).

The method is tests/test_lr_rd.py's: two key frames; a run with CDEF and restoration off gives the pre-CDEF planes, a run with
enable_lr = 0 the CDEF planes, and the restated rule (tests/lr_rd_ref.py) applied to them must give, bit for bit,

  1. the restored planes,
  2. av1mi_lr_rd_result's choices, bits and lambda,
  3. the fits' own tables - av1mi_lr_wiener_fit_result's present flag, taps and error of every unit, av1mi_lr_fit_result's error of
     every candidate and its record of the decision before the Wiener fit.  At these inputs "off" often wins, and only the tables show
     what the fit kernels summed,

and dav1d (libavif) decodes every stream to the reconstruction.  tests/test_lr_edges_content.py asserts on the CPU
that the matrix reaches the states it is for."""
import numpy as np
import pytest

import lr_edge_cases as M
import lr_rd_ref as ref
import lr_unit_ref as uref
import test_lr_fit as base

pytestmark = pytest.mark.gpu

ABSENT = np.uint64(ref.ABSENT)


@pytest.fixture(scope="module")
def ctx(av1mi):
    c = av1mi.Context(0)
    yield c
    c.close()
    uref.forget()
    _planes.clear()
    _cands.clear()


_planes, _cands = {}, {}


def case_planes(ctx, av1mi, ci):
    """a case's frames with their pre-CDEF and CDEF planes, computed once"""
    if ci not in _planes:
        case = M.CASES[ci]
        w, h, bd = case["w"], case["h"], case["bd"]
        frames = [[p.astype(np.int64) for p in f] for f in M.frames(case)]
        pre = base.encode(ctx, av1mi, frames, w, h, bd, **dict(M.params(case), enable_cdef=0, enable_lr=0))[3]
        cdef = base.encode(ctx, av1mi, frames, w, h, bd, **dict(M.params(case), enable_lr=0))[3]
        _planes[ci] = (frames, pre, cdef)
    return _planes[ci]


def case_candidates(ctx, av1mi, ci, shift, f, pl):
    """every candidate of a plane's units at a unit size - both fits, every set - computed once; a mode sees its own (ref.view)"""
    if (ci, shift, f, pl) not in _cands:
        frames, pre, cdef = case_planes(ctx, av1mi, ci)
        _cands[(ci, shift, f, pl)] = M.candidates(pre[f][pl], cdef[f][pl], frames[f][pl], M.CASES[ci]["bd"], int(pl > 0), shift)
    return _cands[(ci, shift, f, pl)]


def check_wiener_table(cands, units, err, want_choice, tag, bad):
    """av1mi_lr_wiener_fit_result of one plane: final choice, present flag, six taps and error of every unit"""
    for i, row in enumerate(cands["err"]):
        for j, e in enumerate(row):
            rec, got_e = [int(x) for x in units[i, j]], int(err[i, j])
            if e[23] is None:
                want, want_e = [int(want_choice[i, j]), 0, 0, 0, 0, 0, 0, 0], ref.ABSENT
            else:
                cv, ch = cands["coef"][i][j][23]
                want, want_e = [int(want_choice[i, j]), 1] + list(cv) + list(ch), e[23]
            if rec != want or got_e != want_e:
                bad.append(tag + ": Wiener fit of unit (%d, %d) %s error %d, restated %s error %d" % (i, j, rec, got_e, want, want_e))


def check_fit_table(cands, units, err, lam, tag, bad):
    """av1mi_lr_fit_result of one plane: the error of every candidate 0 .. 22 (UINT64_MAX where absent) and the record of the
    decision before the Wiener fit"""
    before = M.before_wiener_fit(cands)
    for i, row in enumerate(cands["err"]):
        for j, e in enumerate(row):
            want_e = [ref.ABSENT if x is None else x for x in e[:23]]
            got_e = [int(x) for x in err[i, j]]
            if got_e != want_e:
                bad.append(tag + ": fit errors of unit (%d, %d) %s, restated %s" % (i, j, got_e, want_e))
            c = ref.decide(before["err"][i][j], before["lc"][i][j], before["switchable"], lam)[0]
            if tuple(int(x) for x in units[i, j]) != M.fit_record(cands, i, j, c):
                bad.append(tag + ": fit record of unit (%d, %d) %s, restated %s" % (i, j, units[i, j].tolist(), M.fit_record(cands, i, j, c)))


@pytest.mark.parametrize("ci,shift,low", M.RUNS, ids=M.RUN_IDS)
def test_key_frames_restated(av1mi, ctx, ci, shift, low):
    """planes, choices, bits, lambda and the fits' tables of two key frames are the restated rule's with the rate term off and at every
    scale of the case; dav1d decodes every stream to the reconstruction"""
    import oracle_avif
    case = M.CASES[ci]
    w, h, bd = case["w"], case["h"], case["bd"]
    frames, pre, cdef = case_planes(ctx, av1mi, ci)
    n = len(frames)
    nr, nc = uref.grid(w, h, shift)
    base_v = M.value(shift, low, None)
    bad, streams = [], []
    for s in (None,) + case["scales"]:
        v, lam = M.value(shift, low, s), M.lam(case, s)
        data, sizes, _, got = base.encode(ctx, av1mi, frames, w, h, bd, enable_lr=v, **M.params(case))
        choice, bits16, got_lam = ctx.lr_rd_result(n)
        wfit = ctx.lr_wiener_fit_result(n) if low & ref.WFIT else None
        fit = ctx.lr_fit_result(n) if low & ref.FIT else None
        assert choice.shape == (n, 3, nr, nc) and int(av1mi._lib.av1mi_lr_rd_units(ctx._h)) == nr * nc
        assert got_lam == lam, (hex(v), got_lam, lam)
        streams.append((data, sizes, got))
        for f in range(n):
            for pl in range(3):
                tag = "%s lr %#x frame %d plane %d" % (case["name"], v, f, pl)
                if not M.restored(pl, low):
                    if not np.array_equal(got[f][pl], cdef[f][pl]) or choice[f, pl].any() or bits16[f, pl].any():
                        bad.append(tag + ": a plane that is not restored")
                    if wfit is not None and (wfit[0][f, pl].any() or wfit[1][f, pl].any()):
                        bad.append(tag + ": Wiener fit entries of a plane that is not restored")
                    continue
                cands = ref.view(case_candidates(ctx, av1mi, ci, shift, f, pl), base_v)
                want, wc, wb, wj = ref.restore_rd(cands, lam)
                print(tag, "lambda", lam, "choices", wc.ravel().tolist(), "bits16", wb.ravel().tolist())
                if not np.array_equal(choice[f, pl].astype(np.int64), wc):
                    bad.append(tag + ": choices %s" % choice[f, pl].ravel().tolist())
                if not np.array_equal(bits16[f, pl].astype(np.int64), wb):
                    bad.append(tag + ": bits16 %s" % bits16[f, pl].ravel().tolist())
                if not np.array_equal(got[f][pl], want):
                    bad.append(tag + ": samples")
                if wfit is not None:
                    check_wiener_table(cands, wfit[0][f, pl], wfit[1][f, pl], wc, tag, bad)
                if fit is not None:
                    check_fit_table(cands, fit[0][f, pl], fit[1][f, pl], lam, tag, bad)
    assert not bad, bad
    if oracle_avif.have_libavif():
        for data, sizes, got in streams:
            base._assert_decodes(base._decode(oracle_avif, data, sizes, w, h, bd, n, 1), got, n)
