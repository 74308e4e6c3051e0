"""numpy / Python-integer restatement of the Wiener restoration fit (include/av1mi.h: AV1MI_LR_WIENER_FIT; DESIGN.md §3 item 9e;
av1-base_amd/csrc/wiener_fit_rule.h), built on lr_ref's window, stripes and unit bounds:

  * the D planes of a plane and a unit's 27 sums,
  * the rule: solve_idx (normalise, Cramer), solve (clamp, one refit of the free taps), the two stages - every intermediate asserted
    to stay inside 63 bits, which is what lets the C++ run it in signed 64-bit arithmetic,
  * the two-pass filter with separate vertical and horizontal taps (§7.17.4),
  * restore_wiener_fit: the final choice over a base decision plus candidate 23,
  * the spec's decoder of a Wiener unit's bits (§5.11.58), for the round trip of the code writer."""
import numpy as np

import lr_ref
import sgr_fit_ref

TAPS_MIN, TAPS_MAX, TAPS_MID = (-5, -23, -17), (10, 8, 46), (3, -7, 15)
ABSENT = (1 << 64) - 1
CHOICE = 23
N_SUMS = 27
HVV, HHH, HVH, CV, CH = 0, 6, 12, 21, 24   # offsets into a unit's sums
SYM = ((0, 1, 2), (1, 3, 4), (2, 4, 5))    # index of (j, k) in a symmetric matrix stored as 00 01 02 11 12 22


def i63(v):
    """an intermediate of the rule: it must fit a signed 64-bit integer with a bit to spare"""
    assert -(1 << 63) < v < (1 << 63), v
    return v


rdiv = sgr_fit_ref.rdiv
clamp = sgr_fit_ref.clamp


def d_planes(win):
    """(X, [Dv_0, Dv_1, Dv_2], [Dh_0, Dh_1, Dh_2]) for the window's centre (lr_ref.window: 3 rows / columns of margin)"""
    rows, w = win.shape[0] - 6, win.shape[1] - 6
    X = win[3:3 + rows, 3:3 + w]
    dv = [win[3 - o:3 - o + rows, 3:3 + w] + win[3 + o:3 + o + rows, 3:3 + w] - 2 * X for o in (3, 2, 1)]
    dh = [win[3:3 + rows, 3 - o:3 - o + w] + win[3:3 + rows, 3 + o:3 + o + w] - 2 * X for o in (3, 2, 1)]
    return X, dv, dh


def plane_d(pre, cdef, sub):
    """the D planes over the whole plane, stripe by stripe: (dv[3], dh[3])"""
    pre, cdef = np.asarray(pre, dtype=np.int64), np.asarray(cdef, dtype=np.int64)
    dv, dh = [np.zeros_like(cdef) for _ in range(3)], [np.zeros_like(cdef) for _ in range(3)]
    for s0, s1, a, b in lr_ref.stripes(cdef.shape[0], sub):
        _, v, h = d_planes(lr_ref.window(pre, cdef, s0, s1, a, b))
        for k in range(3):
            dv[k][a:b], dh[k][a:b] = v[k], h[k]
    return dv, dh


def unit_sums(cdef, src, dv, dh):
    """the 27 sums of a unit's samples as Python integers (arguments: the unit's slices)"""
    e = src - cdef
    out = [int((dv[j] * dv[k]).sum()) for j in range(3) for k in range(j, 3)]
    out += [int((dh[j] * dh[k]).sum()) for j in range(3) for k in range(j, 3)]
    out += [int((dv[j] * dh[k]).sum()) for j in range(3) for k in range(3)]
    out += [int((dv[j] * e).sum()) for j in range(3)] + [int((dh[k] * e).sum()) for k in range(3)]
    return out


def _det3(a):
    return i63(i63(a[0][0] * i63(a[1][1] * a[2][2] - a[1][2] * a[2][1])) - i63(a[0][1] * i63(a[1][0] * a[2][2] - a[1][2] * a[2][0]))
               + i63(a[0][2] * i63(a[1][0] * a[2][1] - a[1][1] * a[2][0])))


def solve_idx(H, R, idx):
    """x over the taps of idx (a dict tap -> value), or None if absent"""
    idx = list(idx)
    n = len(idx)
    m = max([abs(H[i][j]) for i in idx for j in idx] + [abs(R[i]) for i in idx])
    s = max(0, m.bit_length() - 17)
    a = [[H[i][j] >> s for j in idx] for i in idx]
    r = [R[i] >> s for i in idx]
    if n == 1:
        det, d = a[0][0], [r[0]]
    elif n == 2:
        det = i63(a[0][0] * a[1][1] - a[0][1] * a[1][0])
        d = [i63(r[0] * a[1][1] - a[0][1] * r[1]), i63(a[0][0] * r[1] - r[0] * a[1][0])]
    else:
        det = _det3(a)
        d = [_det3([[r[i] if j == q else a[i][j] for j in range(3)] for i in range(3)]) for q in range(3)]
    if det <= 0:
        return None
    return {idx[q]: rdiv(i63(128 * d[q]), det) for q in range(n)}


def solve(H, R, first, info=None):
    """the taps [t0, t1, t2] of one pass, or None; info (a dict) gets clamped = the set of taps the first clamp acted on and refit = the
    refit ran and gave a solution"""
    idx = list(range(first, 3))
    x = solve_idx(H, R, idx)
    if info is not None:
        info.update(clamped=set(), refit=False)
    if x is None:
        return None
    t = [0, 0, 0]
    for i in idx:
        t[i] = clamp(x[i], TAPS_MIN[i], TAPS_MAX[i])
    cl = [i for i in idx if t[i] != x[i]]
    if info is not None:
        info["clamped"] = set(cl)
    if cl and len(cl) < len(idx):
        free = [i for i in idx if i not in cl]
        R2 = list(R)
        for i in idx:
            R2[i] = i63(R[i] - rdiv(i63(sum(i63(H[i][j] * t[j]) for j in cl)), 128))
        y = solve_idx(H, R2, free)
        if y is not None:
            if info is not None:
                info["refit"] = True
            for i in free:
                t[i] = clamp(y[i], TAPS_MIN[i], TAPS_MAX[i])
    return t


def fit(sums, first, info=None):
    """(cv, ch) from the 27 sums, or None if the candidate is absent; info gets v = / h = the passes' info dicts"""
    Hvv = [[sums[HVV + SYM[j][k]] for k in range(3)] for j in range(3)]
    Hhh = [[sums[HHH + SYM[j][k]] for k in range(3)] for j in range(3)]
    iv, ih = {}, {}
    if info is not None:
        info.update(v=iv, h=ih)
    cv = solve(Hvv, sums[CV:CV + 3], first, iv)
    if cv is None:
        return None
    R = [i63(sums[CH + k] - rdiv(i63(sum(i63(sums[HVH + j * 3 + k] * cv[j]) for j in range(3))), 128)) for k in range(3)]
    ch = solve(Hhh, R, first, ih)
    if ch is None:
        return None
    return cv, ch


def wiener2(win, cv, ch, bd):
    """§7.17.4: the horizontal pass with the taps of pass 1 (ch), the vertical with those of pass 0 (cv)"""
    fv, fh = lr_ref.taps(cv), lr_ref.taps(ch)
    rows, w = win.shape[0] - 6, win.shape[1] - 6
    offset, limit = 1 << (bd + 7 - 3 - 1), (1 << (bd + 1 + 7 - 3)) - 1
    hp = sum(fh[t] * win[:, t:t + w] for t in range(7))
    hp = np.clip((hp + 4) >> 3, -offset, limit - offset)
    v = sum(fv[t] * hp[t:t + rows] for t in range(7))
    return np.clip((v + 1024) >> 11, 0, (1 << bd) - 1)


def filtered2(pre, cdef, bd, sub, cv, ch):
    """the whole plane filtered with the taps (cv, ch)"""
    pre, cdef = np.asarray(pre, dtype=np.int64), np.asarray(cdef, dtype=np.int64)
    out = np.empty_like(cdef)
    for s0, s1, a, b in lr_ref.stripes(cdef.shape[0], sub):
        out[a:b] = wiener2(lr_ref.window(pre, cdef, s0, s1, a, b), cv, ch, bd)
    return out


def base_decision(pre, cdef, src, bd, sub, lr):
    """the decision before the Wiener fit for enable_lr = lr without bit 10: (plane, choice[unit row][unit column])"""
    if lr & 0x100:
        res, rec, _ = sgr_fit_ref.restore_fit(pre, cdef, src, bd, sub, lr >> 16)
        return res, rec[..., 0]
    res, choice, _ = lr_ref.restore(pre, cdef, src, bd, sub, (lr & 0xFF) in (2, 4))
    return res, choice


def restore_wiener_fit(pre, cdef, src, bd, sub, base, base_choice, infos=None):
    """The final decision: per unit the fitted filter (candidate 23) where its exact SSE is strictly below that of the base decision's
    plane `base`.  Returns (plane, records[unit row][unit column][8] = final choice, present, cv, ch; err[unit row][unit column]);
    infos (a list) gets one (unit row, unit column, info dict of fit) per unit."""
    pre, cdef, src, base = (np.asarray(p, dtype=np.int64) for p in (pre, cdef, src, base))
    dv, dh = plane_d(pre, cdef, sub)
    rows, cols = lr_ref.unit_bounds(src.shape[0], src.shape[1], sub)
    rec = np.zeros((len(rows), len(cols), 8), dtype=np.int64)
    err = np.full((len(rows), len(cols)), ABSENT, dtype=np.uint64)
    res, memo = base.copy(), {}
    for i, (y0, y1) in enumerate(rows):
        for j, (x0, x1) in enumerate(cols):
            sl = (slice(y0, y1), slice(x0, x1))
            info = {}
            w = fit(unit_sums(cdef[sl], src[sl], [d[sl] for d in dv], [d[sl] for d in dh]), sub, info)
            if infos is not None:
                infos.append((i, j, info))
            rec[i, j, 0] = base_choice[i][j]
            if w is None:
                continue
            key = (tuple(w[0]), tuple(w[1]))
            if key not in memo:
                memo[key] = filtered2(pre, cdef, bd, sub, w[0], w[1])
            e = int(((memo[key][sl] - src[sl]) ** 2).sum())
            err[i, j] = e
            rec[i, j, 1:] = [1] + list(w[0]) + list(w[1])
            if e < int(((base[sl] - src[sl]) ** 2).sum()):
                rec[i, j, 0] = CHOICE
                res[sl] = memo[key][sl]
    return res, rec, err


def decode_wiener_unit(bits, n, first, ref):
    """(cv, ch, bits left over) of a Wiener unit coded against ref[pass][tap] = RefLrWiener (§5.11.58)"""
    b = sgr_fit_ref.Bits(bits, n)
    out = [[0, 0, 0], [0, 0, 0]]
    for p in range(2):
        for j in range(first, 3):
            out[p][j] = sgr_fit_ref._signed_subexp_with_ref(b, TAPS_MIN[j], TAPS_MAX[j] + 1, j + 1, ref[p][j])
    return out[0], out[1], b.n
