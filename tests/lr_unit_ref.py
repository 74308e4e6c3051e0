"""Restoration units of 128x128 and 256x256 luma samples (include/av1mi.h: AV1MI_LR_UNIT_128 / _256) for the numpy
restatements: lr_ref.restore, sgr_fit_ref.restore_fit and wiener_fit_ref.restore_wiener_fit take their units from lr_ref.unit_bounds, so
`units_at(shift)` gives them the bounds of lr_unit_shift = shift for the length of a `with` block and nothing of the rules is said twice.

Geometry (§5.9.20, §7.17): U = 64 << shift luma samples, a chroma unit U / 2 chroma samples; max((size + U / 2) / U, 1) units each way;
unit row R covers the plane rows R U - 8 .. (R + 1) U - 9 (chroma: halved), the first from 0, the last to the plane's end; the row offset
and the 64-row stripes do not depend on the unit size.

The whole-plane filter outputs do not depend on the unit size either: inside `units_at` they are kept per (planes, candidate), so the
three unit sizes of one frame share them."""
import contextlib
import hashlib

import numpy as np

import lr_ref
import sgr_fit_ref
import wiener_fit_ref

WFIT, FIT = 0x400, 0x100


def shift_of(v):
    """lr_unit_shift of an enable_lr value"""
    return (v >> 12) & 3


def unit_bounds(h, w, sub, shift):
    """lr_ref.unit_bounds at a unit size: ([(y0, y1)] per unit row, [(x0, x1)] per unit column) of a plane of h x w samples"""
    us, off = (64 << shift) >> sub, 8 >> sub
    nr, nc = lr_ref.count_units(h, us), lr_ref.count_units(w, us)
    rows = [(0 if r == 0 else r * us - off, h if r == nr - 1 else (r + 1) * us - off) for r in range(nr)]
    cols = [(c * us, w if c == nc - 1 else (c + 1) * us) for c in range(nc)]
    return rows, cols


def grid(w, h, shift):
    """(unit rows, unit columns) of every plane of a w x h frame (the size is even: the planes share the grid)"""
    return lr_ref.count_units(h, 64 << shift), lr_ref.count_units(w, 64 << shift)


_memo = {}


def _key(*arrays):
    return tuple(hashlib.sha1(np.ascontiguousarray(a, dtype=np.int64).tobytes()).hexdigest() for a in arrays)


def _memoised(fn, name):
    def wrapped(pre, cdef, bd, sub, *rest):
        k = (name, bd, sub, repr(rest)) + _key(pre, cdef)
        if k not in _memo:
            _memo[k] = fn(pre, cdef, bd, sub, *rest)
        return _memo[k]
    return wrapped


def forget():
    """drop the kept plane outputs (a test module's teardown)"""
    _memo.clear()


@contextlib.contextmanager
def units_at(shift):
    """inside the block the three restatements see units of 64 << shift luma samples"""
    saved = (lr_ref.unit_bounds, lr_ref.filtered, sgr_fit_ref.plane_outputs)
    lr_ref.unit_bounds = lambda h, w, sub: unit_bounds(h, w, sub, shift)
    lr_ref.filtered = _memoised(saved[1], "filtered")
    sgr_fit_ref.plane_outputs = _memoised(saved[2], "plane_outputs")
    try:
        yield
    finally:
        lr_ref.unit_bounds, lr_ref.filtered, sgr_fit_ref.plane_outputs = saved


def restore(pre, cdef, src, bd, sub, switchable, shift):
    with units_at(shift):
        return lr_ref.restore(pre, cdef, src, bd, sub, switchable)


def restore_fit(pre, cdef, src, bd, sub, mask, shift):
    with units_at(shift):
        return sgr_fit_ref.restore_fit(pre, cdef, src, bd, sub, mask)


def restore_value(pre, cdef, src, bd, sub, v, infos=None):
    """One plane under the enable_lr value v, unit size and fit bits included.  Returns a dict: plane, choice[unit row][unit column]
    (the final one: 23 = the fitted Wiener filter), sse (the fixed candidates', without the self-guided fit), fit = (records, errors) of
    the self-guided fit or None, wfit = (records, errors) of the Wiener fit or None."""
    shift = shift_of(v)
    out = dict(fit=None, wfit=None, sse=None)
    with units_at(shift):
        if v & FIT:
            res, rec, err = sgr_fit_ref.restore_fit(pre, cdef, src, bd, sub, v >> 16)
            out["fit"], choice = (rec, err), rec[..., 0]
        else:
            res, choice, out["sse"] = lr_ref.restore(pre, cdef, src, bd, sub, (v & 0xFF) in (2, 4))
        if v & WFIT:
            res, rec, err = wiener_fit_ref.restore_wiener_fit(pre, cdef, src, bd, sub, res, choice, infos)
            out["wfit"], choice = (rec, err), rec[..., 0]
    out.update(plane=res, choice=np.asarray(choice))
    return out
