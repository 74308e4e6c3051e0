"""numpy / Python-integer restatement of the rate term of the restoration unit decisions (include/av1mi.h: AV1MI_LR_RD; DESIGN.md §3
item 9g; av1-base_amd/csrc/lr_rate_rule.h), built on lr_ref, sgr_fit_ref, wiener_fit_ref and lr_unit_ref:

  * L (log2 in sixteenths), T16 of the five type symbols from av1_tables.h's default CDFs, lambda from the dc step tables,
  * the writers of a unit's coefficients (§5.11.58) restated bit by bit, so that the repo's decoders can read them back, and Lc, B16, J,
  * decide: the first minimum of J over the candidates 0 .. 22 and the strict override by candidate 23,
  * candidates / restore_rd: every candidate of a plane's units - error, coefficients, filtered plane - from the existing restatements'
    pieces, and the plane, choices and bits the mode gives for an enable_lr value."""
import os
import re

import numpy as np

import lr_ref
import lr_unit_ref
import sgr_fit_ref
import wiener_fit_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RD, FIT, WFIT = 0xC000, 0x100, 0x400
ABSENT = (1 << 64) - 1


def rd_field(s):
    """include/av1mi.h: AV1MI_LR_RD"""
    return RD | ((s & 1) << 9) | ((s & 2) << 10)


def rd_scale_of(v):
    """the scale s of an enable_lr value, None with the mode off"""
    return (((v >> 9) & 1) | ((v >> 10) & 2)) if (v & RD) == RD else None


_tables = {}


def table(name):
    """a one-dimensional view of an integer table of av1_tables.h"""
    if name not in _tables:
        txt = open(os.path.join(ROOT, "av1-base_amd", "csrc", "av1_tables.h")).read()
        m = re.search(r"\b%s(?:\[\d+\])+\s*=\s*\{(.*?)\};" % re.escape(name), txt, re.S)
        _tables[name] = [int(x) for x in re.findall(r"-?\d+", m.group(1))]
    return _tables[name]


def L(x):
    """aq_rule.h's log2 in sixteenths"""
    k = x.bit_length() - 1
    return 16 * k + (((x << 4) >> k) & 15)


def T16(p):
    return 240 - L(p)


def type_t16(switchable, typ):
    """typ: 0 = NONE / off, 1 = WIENER / on, 2 = SGRPROJ"""
    if switchable:
        c = table("av1_default_switchable_restore_cdf")
        return T16((c[0], c[1] - c[0], 32768 - c[1])[typ])
    c = table("av1_default_use_wiener_cdf")
    return T16((c[0], 32768 - c[0])[typ])


def choice_type(c):
    return 0 if c == 0 else (1 if c <= 3 or c == 23 else 2)


def lam_of_step(q, s):
    l0 = (13 * q * q) >> 9
    return max(1, (l0, l0 >> 1, l0 >> 2, l0 << 1)[s])


def lam(qidx, bd, s):
    return lam_of_step(table("av1_dc_q8" if bd == 8 else "av1_dc_q10")[qidx], s)


def qindex_of_cq(cq):
    """aom's quantizer_to_qindex"""
    return (cq * 4 if cq < 62 else (249, 255)[cq - 62])


# ---- the writers (lr_fit_rule.h: lr_put_ns, lr_put_subexp, lr_recenter, lr_put_signed_ref), as lists of bits
def _put(out, v, n):
    out.extend((v >> i) & 1 for i in range(n - 1, -1, -1))


def _put_ns(out, n, v):
    w = n.bit_length()
    m = (1 << w) - n
    if v < m:
        _put(out, v, w - 1)
    else:
        _put(out, (v + m) >> 1, w - 1)
        _put(out, (v + m) & 1, 1)


def _put_subexp(out, num_syms, k, v):
    i = mk = 0
    while True:
        b2 = k + i - 1 if i else k
        a = 1 << b2
        if num_syms <= mk + 3 * a:
            return _put_ns(out, num_syms - mk, v - mk)
        if v >= mk + a:
            _put(out, 1, 1)
            i += 1
            mk += a
        else:
            _put(out, 0, 1)
            return _put(out, v - mk, b2)


def _recenter(r, v):
    return v if v > 2 * r else ((v - r) << 1 if v >= r else ((r - v) << 1) - 1)


def _put_signed_ref(out, low, high, k, r, v):
    mx, x, rr = high - low, v - low, r - low
    if (rr << 1) <= mx:
        _put_subexp(out, mx, k, _recenter(rr, x))
    else:
        _put_subexp(out, mx, k, _recenter(mx - 1 - rr, mx - 1 - x))


def _pack(out):
    v = 0
    for b in out:
        v = (v << 1) | b
    return v, len(out)


def wiener_code(first, cv, ch, ref=None):
    """(bits, length) of a Wiener unit against ref[pass][tap] (default: Wiener_Taps_Mid)"""
    ref = ref or (wiener_fit_ref.TAPS_MID, wiener_fit_ref.TAPS_MID)
    out = []
    for p, t in enumerate((cv, ch)):
        for j in range(first, 3):
            _put_signed_ref(out, wiener_fit_ref.TAPS_MIN[j], wiener_fit_ref.TAPS_MAX[j] + 1, j + 1, ref[p][j], t[j])
    return _pack(out)


def sgr_code(t, x0, x1, ref=sgr_fit_ref.XQD_MID):
    """(bits, length) of a self-guided unit against ref = RefSgrXqd (default: Sgrproj_Xqd_Mid)"""
    out = []
    _put(out, t, 4)
    for i, x in enumerate((x0, x1)):
        if sgr_fit_ref.SGR_PARAMS[t][2 * i]:
            _put_signed_ref(out, sgr_fit_ref.XQD_MIN[i], sgr_fit_ref.XQD_MAX[i] + 1, 4, ref[i], x)
    return _pack(out)


def wiener_lc(first, cv, ch):
    return wiener_code(first, cv, ch)[1]


def sgr_lc(t, x0, x1):
    return sgr_code(t, x0, x1)[1]


def fixed_lc(sub, k):
    """Lc of the fixed candidate k = 0 .. 6"""
    if k == 0:
        return 0
    if k <= 3:
        c = (lr_ref.WIENER_UV if sub else lr_ref.WIENER_Y)[k - 1]
        return wiener_lc(sub, c, c)
    return sgr_lc(9, *lr_ref.SGR_WEIGHTS[k - 4])


def b16(lc, t16):
    return 16 * lc + t16


def cost(d, lam_, b):
    assert 16 * d < 1 << 42 and lam_ * b < 1 << 32
    return 16 * d + lam_ * b


def decide(err, lc, switchable, lam_):
    """The rule for one unit.  err[c]: the exact SSE of candidate c = 0 .. 22 (and 23, with the Wiener fit), None or ABSENT where the
    candidate is absent; lc[c]: its coefficient length.  Returns (choice, B16 of the choice, J of the choice); lam_ = 0 is the mode off."""
    def j_of(c):
        return cost(int(err[c]), lam_, b16(lc[c], type_t16(switchable, choice_type(c))))
    best = None
    for c in range(min(len(err), 23)):
        if err[c] is None or int(err[c]) == ABSENT:
            continue
        if best is None or j_of(c) < best[0]:
            best = (j_of(c), c)
    if len(err) > 23 and err[23] is not None and int(err[23]) != ABSENT and j_of(23) < best[0]:
        best = (j_of(23), 23)
    c = best[1]
    return c, b16(lc[c], type_t16(switchable, choice_type(c))), best[0]


def candidates(pre, cdef, src, bd, sub, v):
    """Every candidate of the plane's units under the enable_lr value v (fit bits and unit size; the mode bits are ignored): a dict
    err[unit row][unit column][24] (Python integers, None where absent), lc likewise, coef[unit row][unit column][c] = the coefficients
    ((set, xqd0, xqd1) or (cv, ch)) of fitted candidates, and plane(c, i, j) = the filtered samples of unit (i, j) under candidate c."""
    pre, cdef, src = (np.asarray(p, dtype=np.int64) for p in (pre, cdef, src))
    switchable = (v & 0xFF) in (2, 4)
    with lr_unit_ref.units_at(lr_unit_ref.shift_of(v)):
        rows, cols = lr_ref.unit_bounds(src.shape[0], src.shape[1], sub)
        fixed = [lr_ref.filtered(pre, cdef, bd, sub, c) for c in lr_ref.candidates(sub, switchable)]
        mask = ((v >> 16) or 0xFFFF) if v & FIT else 0
        outs = {t: sgr_fit_ref.plane_outputs(pre, cdef, bd, sub, t) for t in range(16) if (mask >> t) & 1}
    dv = dh = None
    if v & WFIT:
        dv, dh = wiener_fit_ref.plane_d(pre, cdef, sub)
    nr, nc = len(rows), len(cols)
    err = [[[None] * 24 for _ in range(nc)] for _ in range(nr)]
    lc = [[[0] * 24 for _ in range(nc)] for _ in range(nr)]
    coef = [[{} for _ in range(nc)] for _ in range(nr)]
    samples, memo = {}, {}
    for i, (y0, y1) in enumerate(rows):
        for j, (x0, x1) in enumerate(cols):
            sl = (slice(y0, y1), slice(x0, x1))

            def put(c, out, length):
                samples[(c, i, j)] = out
                err[i][j][c] = int(((out - src[sl]) ** 2).sum())
                lc[i][j][c] = length
            for k, o in enumerate(fixed):
                put(k, o[sl], fixed_lc(sub, k))
            for t in outs:
                f0, f1 = outs[t][0][sl], outs[t][1][sl]
                w = sgr_fit_ref.solve(t, sgr_fit_ref.unit_sums(cdef[sl], src[sl], f0, f1, t))
                if w is not None:
                    coef[i][j][7 + t] = (t, w[0], w[1])
                    put(7 + t, sgr_fit_ref.blend(cdef[sl], f0, f1, t, w[0], w[1], bd), sgr_lc(t, w[0], w[1]))
            if v & WFIT:
                w = wiener_fit_ref.fit(wiener_fit_ref.unit_sums(cdef[sl], src[sl], [d[sl] for d in dv], [d[sl] for d in dh]), sub)
                if w is not None:
                    key = (tuple(w[0]), tuple(w[1]))
                    if key not in memo:
                        memo[key] = wiener_fit_ref.filtered2(pre, cdef, bd, sub, w[0], w[1])
                    coef[i][j][23] = (list(w[0]), list(w[1]))
                    put(23, memo[key][sl], wiener_lc(sub, w[0], w[1]))
    return dict(err=err, lc=lc, coef=coef, rows=rows, cols=cols, switchable=switchable, plane=lambda c, i, j: samples[(c, i, j)],
                shape=src.shape)


def view(cands, v):
    """`candidates`' tables of a superset value (the same unit size, both fits, every set) as the enable_lr value v sees them: the
    candidates v does not have are absent, and the type symbols are those of v's restoration type"""
    sw = (v & 0xFF) in (2, 4)
    mask = ((v >> 16) or 0xFFFF) if v & FIT else 0
    has = lambda c: c <= 3 or (c <= 6 and sw) or (7 <= c < 23 and (mask >> (c - 7)) & 1) or (c == 23 and bool(v & WFIT))
    err = [[[e if has(c) else None for c, e in enumerate(u)] for u in row] for row in cands["err"]]
    return dict(cands, err=err, switchable=sw)


def restore_rd(cands, lam_):
    """The plane the rule gives from `candidates`' tables at lam_ (0: the mode off).  Returns (plane, choice[unit row][unit column],
    bits16 likewise, J likewise)."""
    rows, cols = cands["rows"], cands["cols"]
    res = np.empty(cands["shape"], dtype=np.int64)
    choice = np.zeros((len(rows), len(cols)), dtype=np.int64)
    bits = np.zeros((len(rows), len(cols)), dtype=np.int64)
    js = [[0] * len(cols) for _ in rows]
    for i, (y0, y1) in enumerate(rows):
        for j, (x0, x1) in enumerate(cols):
            c, b, jj = decide(cands["err"][i][j], cands["lc"][i][j], cands["switchable"], lam_)
            choice[i, j], bits[i, j], js[i][j] = c, b, jj
            res[y0:y1, x0:x1] = cands["plane"](c, i, j)
    return res, choice, bits, js


def cost_of(cands, i, j, c, lam_):
    """J of candidate c of unit (i, j)"""
    return cost(cands["err"][i][j][c], lam_, b16(cands["lc"][i][j][c], type_t16(cands["switchable"], choice_type(c))))
