"""numpy restatement of loop restoration on one plane (AV1 spec §7.17) and of the encoder's per-unit decision (DESIGN.md §3 items 9,
9b and 9c), for luma (sub = 0: 64x64 units offset by 8 rows, 64-row stripes) and 4:2:0 chroma (sub = 1: 32x32 units offset by 4 rows,
32-row stripes from 32 s - 4).

Planes are 2-D integer arrays of the signalled size (chroma: Round2(size, 1)), which is where the plane ends for the filters' clamps.
Box sums by cumsum, one stripe at a time, so a 1080p plane takes seconds for all seven candidates."""
import numpy as np

WIENER_Y = ((0, 0, -4), (1, -3, -6), (3, -7, 15))
WIENER_UV = ((0, 0, -4), (0, 0, 16), (0, 6, 20))   # chroma: tap 0 is 0 (§5.11.58 codes taps 1 and 2)
SGR_WEIGHTS = ((31, 31), (0, 31), (31, 95))         # (xqd0, xqd1) of the self-guided candidates, all with parameter set 9
SET9 = ((2, 68), (1, 15))                           # Sgr_Params[9]: (r0, eps0), (r1, eps1)


def geometry(sub):
    """(unit size = stripe height, row offset) of a plane"""
    return 64 >> sub, 8 >> sub


def count_units(size, unit):
    """count_units_in_frame (§7.17)"""
    return max((size + (unit >> 1)) // unit, 1)


def unit_bounds(h, w, sub):
    """([(y0, y1)] per unit row, [(x0, x1)] per unit column): the last unit of a row / column runs to the plane's end"""
    us, off = geometry(sub)
    nr, nc = count_units(h, us), count_units(w, us)
    rows = [(0 if r == 0 else r * us - off, h if r == nr - 1 else (r + 1) * us - off) for r in range(nr)]
    cols = [(c * us, w if c == nc - 1 else (c + 1) * us) for c in range(nc)]
    return rows, cols


def stripes(h, sub):
    """[(s0, s1, a, b)]: stripe rows s0 .. s1 (StripeStartY = (64 s - 8) >> sub) and the plane's rows [a, b) inside it"""
    sh, off = geometry(sub)
    out, s = [], 0
    while s * sh - off < h:
        s0 = s * sh - off
        out.append((s0, s0 + sh - 1, max(s0, 0), min(s0 + sh, h)))
        s += 1
    return out


def window(pre, cdef, s0, s1, a, b):
    """get_source_sample (§7.17.6) for rows a - 3 .. b + 2 and columns -3 .. w + 2: coordinates clamp to the plane, rows outside
    the stripe come from the pre-CDEF plane, at most 2 rows away"""
    h = cdef.shape[0]
    rows = []
    for y in range(a - 3, b + 3):
        yy = min(max(y, 0), h - 1)
        if yy < s0:
            rows.append(pre[max(yy, s0 - 2)])
        elif yy > s1:
            rows.append(pre[min(yy, s1 + 2)])
        else:
            rows.append(cdef[yy])
    return np.pad(np.stack(rows).astype(np.int64), ((0, 0), (3, 3)), mode="edge")


def taps(c):
    c0, c1, c2 = c
    return (c0, c1, c2, 128 - 2 * (c0 + c1 + c2), c2, c1, c0)


def wiener(win, c, bd):
    """§7.17.4 with the same taps in both passes, for the rows and columns of the window's centre"""
    f = taps(c)
    rows, w = win.shape[0] - 6, win.shape[1] - 6
    offset, limit = 1 << (bd + 7 - 3 - 1), (1 << (bd + 1 + 7 - 3)) - 1
    hp = sum(f[t] * win[:, t:t + w] for t in range(7))
    hp = np.clip((hp + 4) >> 3, -offset, limit - offset)
    v = sum(f[t] * hp[t:t + rows] for t in range(7))
    return np.clip((v + 1024) >> 11, 0, (1 << bd) - 1)


def _box(v, r, rows, cols):
    """sums of v over the (2r+1)^2 windows centred at v[2 + i, 2 + j], i < rows, j < cols"""
    n = 2 * r + 1
    s = np.zeros((v.shape[0] + 1, v.shape[1] + 1), dtype=np.int64)
    s[1:, 1:] = v.cumsum(0).cumsum(1)
    y, x = 2 - r, 2 - r
    return s[y + n:y + n + rows, x + n:x + n + cols] - s[y:y + rows, x + n:x + n + cols] - s[y + n:y + n + rows, x:x + cols] + s[y:y + rows, x:x + cols]


def _ab(win, r, eps, bd, rows, cols):
    """A and B of the box filter process at the rows -1 .. rows and columns -1 .. cols of the window's centre"""
    b = _box(win, r, rows + 2, cols + 2)
    a = _box(win * win, r, rows + 2, cols + 2)
    n = (2 * r + 1) ** 2
    s = ((1 << 20) + n * n * eps // 2) // (n * n * eps)
    one_by_n = ((1 << 12) + n // 2) // n
    a = (a + ((1 << (2 * (bd - 8))) >> 1)) >> (2 * (bd - 8))
    d = (b + ((1 << (bd - 8)) >> 1)) >> (bd - 8)
    p = np.maximum(a * n - d * d, 0)
    z = (p * s + (1 << 19)) >> 20
    A = np.where(z >= 255, 256, np.where(z == 0, 1, ((z << 8) + z // 2) // (z + 1)))
    return A, ((256 - A) * b * one_by_n + (1 << 11)) >> 12


def sgr(win, cur, y0, w0, w1, bd):
    """§7.17.3 with parameter set 9 and the weights (w0, w1) for the window's centre; cur: the CDEF samples there, y0: the plane row
    of its first row (pass 0 treats odd and even rows differently)"""
    rows, w = cur.shape
    (r0, e0), (r1, e1) = SET9
    A0, B0 = _ab(win, r0, e0, bd, rows, w)
    A1, B1 = _ab(win, r1, e1, bd, rows, w)

    def nb(M, dy, dx):
        return M[1 + dy:1 + dy + rows, 1 + dx:1 + dx + w]
    cross = [(dy, dx, 4 if dy == 0 or dx == 0 else 3) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
    flt1 = (sum(k * nb(A1, dy, dx) for dy, dx, k in cross) * cur + sum(k * nb(B1, dy, dx) for dy, dx, k in cross) + (1 << 8)) >> 9

    def r565(M, dy):
        return 5 * nb(M, dy, -1) + 6 * nb(M, dy, 0) + 5 * nb(M, dy, 1)
    odd = ((np.arange(y0, y0 + rows) & 1) == 1)[:, None]
    v_odd = (r565(A0, 0) * cur + r565(B0, 0) + (1 << 7)) >> 8
    v_even = ((r565(A0, -1) + r565(A0, 1)) * cur + r565(B0, -1) + r565(B0, 1) + (1 << 8)) >> 9
    flt0 = np.where(odd, v_odd, v_even)
    v = w1 * (cur << 4) + w0 * flt0 + (128 - w0 - w1) * flt1
    return np.clip((v + (1 << 10)) >> 11, 0, (1 << bd) - 1)


def candidates(sub, switchable):
    """the candidates in decision order: None (off), ("w", taps) x 3, then with switchable units ("s", weights) x 3"""
    wc = WIENER_UV if sub else WIENER_Y
    return [None] + [("w", c) for c in wc] + ([("s", c) for c in SGR_WEIGHTS] if switchable else [])


def filtered(pre, cdef, bd, sub, cand):
    """the whole plane restored with one candidate (None: the CDEF plane itself)"""
    pre, cdef = np.asarray(pre, dtype=np.int64), np.asarray(cdef, dtype=np.int64)
    if cand is None:
        return cdef.copy()
    out = np.empty_like(cdef)
    for s0, s1, a, b in stripes(cdef.shape[0], sub):
        win = window(pre, cdef, s0, s1, a, b)
        out[a:b] = wiener(win, cand[1], bd) if cand[0] == "w" else sgr(win, cdef[a:b], a, cand[1][0], cand[1][1], bd)
    return out


def restore(pre, cdef, src, bd, sub, switchable):
    """The encoder's rule: per unit the candidate with the smallest SSE against src, the first minimum in candidate order.
    Returns (restored plane, choice[unit row][unit column] (0 off, 1..3 Wiener, 4..6 self-guided), sse[unit row][unit column][cand])."""
    src = np.asarray(src, dtype=np.int64)
    outs = [filtered(pre, cdef, bd, sub, c) for c in candidates(sub, switchable)]
    rows, cols = unit_bounds(src.shape[0], src.shape[1], sub)
    sse = np.zeros((len(rows), len(cols), len(outs)), dtype=np.int64)
    choice = np.zeros((len(rows), len(cols)), dtype=np.int64)
    res = np.empty_like(src)
    for i, (y0, y1) in enumerate(rows):
        for j, (x0, x1) in enumerate(cols):
            for k, o in enumerate(outs):
                sse[i, j, k] = int(((o[y0:y1, x0:x1] - src[y0:y1, x0:x1]) ** 2).sum())
            choice[i, j] = k = int(np.argmin(sse[i, j]))
            res[y0:y1, x0:x1] = outs[k][y0:y1, x0:x1]
    return res, choice, sse
