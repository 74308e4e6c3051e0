"""numpy / Python-integer restatement of the self-guided restoration fit (include/av1mi.h: AV1MI_LR_FIT; DESIGN.md §3 item 9d;
av1-base_amd/csrc/lr_fit_rule.h), built on lr_ref's window, stripes, unit bounds and A / B:

  * the two box-filter outputs and the filtered plane of any of the 16 parameter sets (§7.17.3),
  * the rule: a unit's five sums, their normalisation, the 2x2 solve with both clamps and the refit on the clamped line,
  * restore_fit: the decision over the 23 candidates of a unit (off, 3 Wiener, 3 fixed self-guided, 16 fitted sets),
  * the spec's decoder of a self-guided unit's bits (§5.11.58, §4.10.7 .. §4.10.10), for the round trip of the code writer."""
import numpy as np

import lr_ref

SGR_PARAMS = ((2, 12, 1, 4), (2, 15, 1, 6), (2, 18, 1, 8), (2, 21, 1, 9), (2, 24, 1, 10), (2, 29, 1, 11), (2, 36, 1, 12), (2, 45, 1, 13),
              (2, 56, 1, 14), (2, 68, 1, 15), (0, 0, 1, 5), (0, 0, 1, 8), (0, 0, 1, 11), (0, 0, 1, 14), (2, 30, 0, 0), (2, 75, 0, 0))
XQD_MIN, XQD_MAX, XQD_MID = (-96, -32), (31, 95), (-32, 31)
ABSENT = (1 << 64) - 1
N_CANDS = 23


def clamp(v, lo, hi):
    return lo if v < lo else (hi if v > hi else v)


def box_outputs(win, cur, y0, t, bd):
    """(flt0, flt1) of parameter set t for the window's centre (None for a pass whose radius is 0); cur: the CDEF samples there, y0:
    the plane row of its first row"""
    rows, w = cur.shape
    r0, e0, r1, e1 = SGR_PARAMS[t]

    def nb(M, dy, dx):
        return M[1 + dy:1 + dy + rows, 1 + dx:1 + dx + w]
    flt0 = flt1 = None
    if r1:
        A1, B1 = lr_ref._ab(win, r1, e1, bd, rows, w)
        cross = [(dy, dx, 4 if dy == 0 or dx == 0 else 3) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
        flt1 = (sum(k * nb(A1, dy, dx) for dy, dx, k in cross) * cur + sum(k * nb(B1, dy, dx) for dy, dx, k in cross) + (1 << 8)) >> 9
    if r0:
        A0, B0 = lr_ref._ab(win, r0, e0, bd, rows, w)

        def r565(M, dy):
            return 5 * nb(M, dy, -1) + 6 * nb(M, dy, 0) + 5 * nb(M, dy, 1)
        odd = ((np.arange(y0, y0 + rows) & 1) == 1)[:, None]
        v_odd = (r565(A0, 0) * cur + r565(B0, 0) + (1 << 7)) >> 8
        v_even = ((r565(A0, -1) + r565(A0, 1)) * cur + r565(B0, -1) + r565(B0, 1) + (1 << 8)) >> 9
        flt0 = np.where(odd, v_odd, v_even)
    return flt0, flt1


def plane_outputs(pre, cdef, bd, sub, t):
    """(flt0, flt1) of set t over the whole plane, stripe by stripe (an all-zero array for a pass whose radius is 0)"""
    pre, cdef = np.asarray(pre, dtype=np.int64), np.asarray(cdef, dtype=np.int64)
    f0, f1 = np.zeros_like(cdef), np.zeros_like(cdef)
    for s0, s1, a, b in lr_ref.stripes(cdef.shape[0], sub):
        o0, o1 = box_outputs(lr_ref.window(pre, cdef, s0, s1, a, b), cdef[a:b], a, t, bd)
        if o0 is not None:
            f0[a:b] = o0
        if o1 is not None:
            f1[a:b] = o1
    return f0, f1


def blend(cdef, f0, f1, t, w0, w1, bd):
    """§7.17.3's last step with LrSgrXqd = (w0, w1): a pass whose radius is 0 contributes u"""
    r0, _, r1, _ = SGR_PARAMS[t]
    u = cdef << 4
    v = w1 * u + w0 * (f0 if r0 else u) + (128 - w0 - w1) * (f1 if r1 else u)
    return np.clip((v + (1 << 10)) >> 11, 0, (1 << bd) - 1)


def filtered_set(pre, cdef, bd, sub, t, w0, w1):
    """the whole plane filtered with set t and the weights (w0, w1)"""
    cdef = np.asarray(cdef, dtype=np.int64)
    f0, f1 = plane_outputs(pre, cdef, bd, sub, t)
    return blend(cdef, f0, f1, t, w0, w1, bd)


def unit_sums(cdef, src, f0, f1, t):
    """(H00, H01, H11, C0, C1) of a unit's samples as Python integers"""
    r0, _, r1, _ = SGR_PARAMS[t]
    u = cdef << 4
    a = f0 - u if r0 else np.zeros_like(u)
    b = f1 - u if r1 else np.zeros_like(u)
    s = (src << 4) - u
    return tuple(int(v.sum()) for v in (a * a, a * b, b * b, a * s, b * s))


def rdiv(a, b):
    q = (abs(a) + (b >> 1)) // b
    return -q if a < 0 else q


def solve(t, sums):
    """the rule: (xqd0, xqd1) of set t from the five sums, or None if the candidate is absent"""
    k = max(0, max(abs(v) for v in sums).bit_length() - 26)
    H00, H01, H11, C0, C1 = (v >> k for v in sums)
    r0, _, r1, _ = SGR_PARAMS[t]
    if r0 and r1:
        det = H00 * H11 - H01 * H01
        if det <= 0:
            return None
        x0 = rdiv(128 * (C0 * H11 - C1 * H01), det)
        x1 = rdiv(128 * (C1 * H00 - C0 * H01), det)
        w = 128 - x0 - x1
        xqd1 = clamp(w, XQD_MIN[1], XQD_MAX[1])
        if xqd1 != w:
            T, D = 128 - xqd1, H00 - 2 * H01 + H11
            if D > 0:
                x0 = rdiv(128 * (C0 - C1) - T * (H01 - H11), D)
        return clamp(x0, XQD_MIN[0], XQD_MAX[0]), xqd1
    if r0:
        if H00 <= 0:
            return None
        xqd0 = clamp(rdiv(128 * C0, H00), XQD_MIN[0], XQD_MAX[0])
        return xqd0, clamp(128 - xqd0, XQD_MIN[1], XQD_MAX[1])
    if H11 <= 0:
        return None
    return 0, clamp(128 - rdiv(128 * C1, H11), XQD_MIN[1], XQD_MAX[1])


def restore_fit(pre, cdef, src, bd, sub, mask=0):
    """The decision with the fit: per unit the first minimum of the exact SSE over off, the 3 Wiener filters, the 3 fixed self-guided
    candidates and, for every set t of the mask (0: all), set t with the unit's fitted weights.
    Returns (plane, records[unit row][unit column][4] = choice, set, xqd0, xqd1, err[unit row][unit column][23] (ABSENT where there
    is no candidate))."""
    pre, cdef, src = (np.asarray(p, dtype=np.int64) for p in (pre, cdef, src))
    mask = mask or 0xFFFF
    fixed = [lr_ref.filtered(pre, cdef, bd, sub, c) for c in lr_ref.candidates(sub, True)]
    outs = {t: plane_outputs(pre, cdef, bd, sub, t) for t in range(16) if (mask >> t) & 1}
    rows, cols = lr_ref.unit_bounds(src.shape[0], src.shape[1], sub)
    rec = np.zeros((len(rows), len(cols), 4), dtype=np.int64)
    err = np.full((len(rows), len(cols), N_CANDS), ABSENT, dtype=np.uint64)
    res = np.empty_like(src)
    for i, (y0, y1) in enumerate(rows):
        for j, (x0, x1) in enumerate(cols):
            sl = (slice(y0, y1), slice(x0, x1))
            cands = [(o[sl], 0, 0, 0) for o in fixed[:4]] + [(o[sl], 9, w[0], w[1]) for o, w in zip(fixed[4:], lr_ref.SGR_WEIGHTS)]
            for t in range(16):
                cands.append(None)
                if t not in outs:
                    continue
                f0, f1 = outs[t][0][sl], outs[t][1][sl]
                w = solve(t, unit_sums(cdef[sl], src[sl], f0, f1, t))
                if w is not None:
                    cands[-1] = (blend(cdef[sl], f0, f1, t, w[0], w[1], bd), t, w[0], w[1])
            best = None
            for k, c in enumerate(cands):
                if c is None:
                    continue
                e = int(((c[0] - src[sl]) ** 2).sum())
                err[i, j, k] = e
                if best is None or e < best[0]:
                    best = (e, k)
            k = best[1]
            res[sl] = cands[k][0]
            rec[i, j] = (k,) + tuple(cands[k][1:])
    return res, rec, err


# ---- the decoder's side of a self-guided unit (spec §5.11.58 and the subexp descriptors)
class Bits:
    def __init__(self, bits, n):
        self.v, self.n = bits, n

    def L(self, k):
        assert k <= self.n, "read past the end of the unit's bits"
        self.n -= k
        return (self.v >> self.n) & ((1 << k) - 1)


def _ns(b, n):
    w = n.bit_length()
    m = (1 << w) - n
    v = b.L(w - 1)
    if v < m:
        return v
    return (v << 1) - m + b.L(1)


def _subexp(b, num_syms, k):
    i = mk = 0
    while True:
        b2 = k + i - 1 if i else k
        a = 1 << b2
        if num_syms <= mk + 3 * a:
            return _ns(b, num_syms - mk) + mk
        if b.L(1):
            i += 1
            mk += a
        else:
            return b.L(b2) + mk


def _inverse_recenter(r, v):
    if v > 2 * r:
        return v
    return r - ((v + 1) >> 1) if v & 1 else r + (v >> 1)


def _signed_subexp_with_ref(b, low, high, k, r):
    mx, r = high - low, r - low
    v = _subexp(b, mx, k)
    x = _inverse_recenter(r, v) if (r << 1) <= mx else mx - 1 - _inverse_recenter(mx - 1 - r, v)
    return x + low


def decode_sgr_unit(bits, n, ref):
    """(lr_sgr_set, xqd0, xqd1, bits left over) of a self-guided unit coded against ref = RefSgrXqd"""
    b = Bits(bits, n)
    t = b.L(4)
    ref = list(ref)
    for i in range(2):
        if SGR_PARAMS[t][2 * i] == 0:
            v = 0 if i == 0 else clamp(128 - ref[0], XQD_MIN[1], XQD_MAX[1])
        else:
            v = _signed_subexp_with_ref(b, XQD_MIN[i], XQD_MAX[i] + 1, 4, ref[i])
        ref[i] = v
    return t, ref[0], ref[1], b.n
