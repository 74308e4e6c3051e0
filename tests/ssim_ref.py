"""The quality pass's rule (av1-base_amd/csrc/ssim_rule.h) restated: libaom's aom_ssim2 geometry and constants in integers, every
window value truncated to Q24 - in Python integers for one window, in numpy int64 for planes and chunks - with the window map's
layout: per frame Y, U, V, each plane's ny x nx window values in raster order, dense."""
import numpy as np

Q = 24
C = {8: (26634, 239708), 10: (428658, 3857925)}   # 64^2 (0.01 L)^2 and 64^2 (0.03 L)^2 as libaom rounds them
WEIGHTS = (0.8, 0.1, 0.1)


def windows_along(n):
    return (n - 8) // 4 + 1 if n >= 8 else 0


def factors(s1, s2, ss, s12, bd):
    """A, B, Cn, D of a window from its sums (Python integers)"""
    c1, c2 = C[bd]
    return 2 * s1 * s2 + c1, s1 * s1 + s2 * s2 + c1, 2 * (64 * s12 - s1 * s2) + c2, 64 * ss - s1 * s1 - s2 * s2 + c2


def bounds_hold(A, B, Cn, D):
    """the four inequalities that keep every 64-bit product of the rule under 2^59"""
    return 0 < A <= B < 2 ** 34 and abs(Cn) <= D < 2 ** 35


def window(s1, s2, ss, s12, bd):
    """w of a window from its sums, in Python integers"""
    A, B, Cn, D = factors(s1, s2, ss, s12, bd)
    assert bounds_hold(A, B, Cn, D), (A, B, Cn, D)
    v = (((A << Q) // B) * ((abs(Cn) << Q) // D)) >> Q
    return -v if Cn < 0 else v


def sums_of(x, y):
    """s1, s2, ss, s12 of two equal-sized blocks of samples"""
    x = np.asarray(x, dtype=np.int64)
    y = np.asarray(y, dtype=np.int64)
    return int(x.sum()), int(y.sum()), int((x * x).sum() + (y * y).sum()), int((x * y).sum())


def _box(x, ny, nx):
    """the sums of x over the 8x8 windows at (4 i, 4 j)"""
    I = np.zeros((x.shape[0] + 1, x.shape[1] + 1), dtype=np.int64)
    I[1:, 1:] = x.cumsum(0).cumsum(1)
    ys, xs = 4 * np.arange(ny)[:, None], 4 * np.arange(nx)[None, :]
    return I[ys + 8, xs + 8] - I[ys, xs + 8] - I[ys + 8, xs] + I[ys, xs]


def window_map(a, b, bd):
    """the window values of plane b against plane a: int64 [ny][nx]"""
    h, w = a.shape
    ny, nx = windows_along(h), windows_along(w)
    if ny == 0 or nx == 0:
        return np.zeros((ny, nx), dtype=np.int64)   # (empty)
    a = a.astype(np.int64)
    b = b.astype(np.int64)
    c1, c2 = C[bd]
    s1, s2, ss, s12 = _box(a, ny, nx), _box(b, ny, nx), _box(a * a + b * b, ny, nx), _box(a * b, ny, nx)
    A, B = 2 * s1 * s2 + c1, s1 * s1 + s2 * s2 + c1
    Cn, D = 2 * (64 * s12 - s1 * s2) + c2, 64 * ss - s1 * s1 - s2 * s2 + c2
    assert (A > 0).all() and (A <= B).all() and (B < 2 ** 34).all() and (np.abs(Cn) <= D).all() and (D < 2 ** 35).all()
    v = (((A << Q) // B) * ((np.abs(Cn) << Q) // D)) >> Q
    return np.where(Cn < 0, -v, v)


def planes(buf, w, h, bd, n):
    """[frame][plane] views of n tight planar 4:2:0 frames"""
    x = np.frombuffer(bytes(buf), dtype=np.uint16 if bd > 8 else np.uint8)
    cw, ch = (w + 1) // 2, (h + 1) // 2
    per = w * h + 2 * cw * ch
    assert x.size == n * per, (x.size, n, per)
    out = []
    for f in range(n):
        fr = x[f * per:(f + 1) * per]
        out.append([fr[:w * h].reshape(h, w), fr[w * h:w * h + cw * ch].reshape(ch, cw), fr[w * h + cw * ch:].reshape(ch, cw)])
    return out


def quality(ref, test, w, h, bd, n):
    """What av1mi_quality returns for two chunks: (q, maps) - q int64-safe Python integers [frame][plane] = (sse, ssim_sum, windows),
    maps [frame][plane] = the window values [ny][nx]"""
    q, maps = [], []
    for pa, pb in zip(planes(ref, w, h, bd, n), planes(test, w, h, bd, n)):
        fq, fm = [], []
        for a, b in zip(pa, pb):
            m = window_map(a, b, bd)
            d = a.astype(np.int64) - b.astype(np.int64)
            fq.append((int((d * d).sum()), int(m.sum()), int(m.size)))
            fm.append(m)
        q.append(fq)
        maps.append(fm)
    return q, maps


def ssim_of(plane_sums):
    """y, u, v, all of three (sse, ssim_sum, windows): a plane without windows is None and drops out of `all`, the weights renormalised"""
    vals = [s / (n * float(1 << Q)) if n else None for _, s, n in plane_sums]
    wsum = sum(w for w, v in zip(WEIGHTS, vals) if v is not None)
    return vals + [sum(w * v for w, v in zip(WEIGHTS, vals) if v is not None) / wsum if wsum else None]
