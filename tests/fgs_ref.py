"""numpy restatement of AV1's film-grain synthesis (spec 7.18.3; av1-base_amd/csrc/fg_synth_rule.h; include/av1mi.h:
av1mi_film_grain_synth) for 4:2:0, as dav1d applies it: the whole of film_grain_params, not only what this encoder writes.

A parameter set is a dict (params()): the points, lag, coefficients, shifts and multipliers of one film_grain_params without its seed.
synth(planes, bd, g, seed) returns [Y, U, V] with the grain added."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LUMA_H, LUMA_W, CHROMA_H, CHROMA_W = 73, 82, 38, 44
TABLE_SHA256 = "3b46df1c6c84b2c0e374d10e3fbaf443d2b5f87a857f903d16486defc52525a9"


def gaussian_sequence():
    """the 2048 values of av1-base_amd/csrc/fg_gauss_table.h"""
    txt = open(os.path.join(ROOT, "av1-base_amd", "csrc", "fg_gauss_table.h")).read()
    body = txt[txt.index("{", txt.index("av1mi_fg_gaussian_sequence[")) + 1:txt.rindex("}")]
    return np.array([int(v) for v in re.findall(r"-?\d+", body)], dtype=np.int64)


_GAUSS = None


def _gauss():
    global _GAUSS
    if _GAUSS is None:
        _GAUSS = gaussian_sequence()
    return _GAUSS


def params(**kw):
    """a parameter set: the fixed table's form by default, every field overridable"""
    g = dict(point_y=[], point_cb=[], point_cr=[], chroma_scaling_from_luma=0, grain_scaling_minus_8=3, ar_coeff_lag=0,
             ar_coeffs_y=[0] * 24, ar_coeffs_cb=[0] * 25, ar_coeffs_cr=[0] * 25, ar_coeff_shift_minus_6=0, grain_scale_shift=0,
             cb_mult=128, cb_luma_mult=192, cb_offset=256, cr_mult=128, cr_luma_mult=192, cr_offset=256, overlap_flag=1,
             clip_to_restricted_range=0, mc_identity=0)
    for k in kw:
        assert k in g, k
    g.update(kw)
    return g


def fixed_params(n):
    """what film_grain = N writes: two points per plane, 2 N luma / N chroma"""
    y, c = min(2 * n, 255), n
    return params(point_y=[(0, y), (255, y)], point_cb=[(0, c), (255, c)], point_cr=[(0, c), (255, c)])


def grain_seed(first_frame, frame):
    return (7391 + 173 * (first_frame + frame)) & 0xFFFF


def lfsr(r):
    bit = (r ^ (r >> 1) ^ (r >> 3) ^ (r >> 12)) & 1
    return (r >> 1) | (bit << 15)


def round2(x, n):
    """on signed values: the arithmetic shift of x + half"""
    return (x + ((1 << n) >> 1)) >> n


def _draws(seed, n):
    """n successive get_random_number(11) values"""
    out, r = np.zeros(n, dtype=np.int64), seed
    for i in range(n):
        r = lfsr(r)
        out[i] = r >> 5
    return out


def templates(g, bd, seed):
    """(LumaGrain 73x82, CbGrain 38x44, CrGrain 38x44)"""
    shift = 12 - bd + g["grain_scale_shift"]
    centre = 128 << (bd - 8)
    gmin, gmax = -centre, (256 << (bd - 8)) - 1 - centre
    lag, ar_shift = g["ar_coeff_lag"], g["ar_coeff_shift_minus_6"] + 6
    has = [len(g["point_y"]) > 0, len(g["point_cb"]) > 0 or g["chroma_scaling_from_luma"], len(g["point_cr"]) > 0 or g["chroma_scaling_from_luma"]]
    out = []
    for pl, (h, w, key) in enumerate(((LUMA_H, LUMA_W, 0), (CHROMA_H, CHROMA_W, 0xb524), (CHROMA_H, CHROMA_W, 0x49d8))):
        if has[pl]:
            t = round2(_gauss()[_draws(seed ^ key, h * w)], shift).reshape(h, w)
        else:
            t = np.zeros((h, w), dtype=np.int64)
        out.append([[int(v) for v in row] for row in t])
    luma = out[0]
    cy = g["ar_coeffs_y"]
    for y in range(3, LUMA_H):
        for x in range(3, LUMA_W - 3):
            s, pos = 0, 0
            for dr in range(-lag, 1):
                for dc in range(-lag, lag + 1):
                    if dr == 0 and dc == 0:
                        break
                    s += cy[pos] * luma[y + dr][x + dc]
                    pos += 1
            luma[y][x] = min(gmax, max(gmin, luma[y][x] + round2(s, ar_shift)))
    for pl in (1, 2):
        c, t = g["ar_coeffs_cb" if pl == 1 else "ar_coeffs_cr"], out[pl]
        for y in range(3, CHROMA_H):
            for x in range(3, CHROMA_W - 3):
                s, pos = 0, 0
                for dr in range(-lag, 1):
                    for dc in range(-lag, lag + 1):
                        if dr == 0 and dc == 0:
                            break
                        s += c[pos] * t[y + dr][x + dc]
                        pos += 1
                if has[0]:
                    ly, lx = ((y - 3) << 1) + 3, ((x - 3) << 1) + 3
                    s += c[pos] * round2(luma[ly][lx] + luma[ly][lx + 1] + luma[ly + 1][lx] + luma[ly + 1][lx + 1], 2)
                t[y][x] = min(gmax, max(gmin, t[y][x] + round2(s, ar_shift)))
    return [np.array(t, dtype=np.int64) for t in out]


def scaling_lut(points):
    """the 256 entries of a scaling function: piece-wise linear between the points, flat outside them; no points: zeros"""
    lut = np.zeros(256, dtype=np.int64)
    if not points:
        return lut
    lut[:points[0][0]] = points[0][1]
    for (x0, y0), (x1, y1) in zip(points[:-1], points[1:]):
        dx = x1 - x0
        delta = (y1 - y0) * ((65536 + (dx >> 1)) // dx)
        for x in range(dx):
            lut[x0 + x] = y0 + ((x * delta + 32768) >> 16)
    lut[points[-1][0]:] = points[-1][1]
    return lut


def scale_lut(lut, index, bd):
    """scale_lut of the spec on an array of sample values"""
    shift = bd - 8
    x = index >> shift
    rem = index - (x << shift)
    start, end = lut[x], lut[np.minimum(x + 1, 255)]
    return np.where(x == 255, start, start + round2((end - start) * rem, shift))   # (at 8 bits rem is 0)


def block_offsets(seed, stripes, blocks):
    """[stripe][block] the 8-bit random value of every 32x32 luma block: offsetX = v >> 4, offsetY = v & 15"""
    out = np.zeros((stripes, blocks), dtype=np.int64)
    for n in range(stripes):
        r = seed ^ (((n * 37 + 178) & 255) << 8) ^ ((n * 173 + 105) & 255)
        for b in range(blocks):
            r = lfsr(r)
            out[n, b] = r >> 8
    return out


def noise_image(t, offs, w, h, sub, bd, overlap):
    """a plane's NoiseImage, h x w: the stripes' blocks blended horizontally, then the stripes vertically"""
    centre = 128 << (bd - 8)
    gmin, gmax = -centre, (256 << (bd - 8)) - 1 - centre
    n = 32 >> sub                      # a block's samples each way, without the overlap
    ov = 2 >> sub                      # the overlap's samples
    wts = [(27, 17), (17, 27)] if sub == 0 else [(23, 22)]
    stripes = []
    for s in range(offs.shape[0]):
        st = np.zeros((n + ov, w), dtype=np.int64)
        for b in range(offs.shape[1]):
            x0 = b * n
            if x0 >= w:
                break
            ox, oy = int(offs[s, b]) >> 4, int(offs[s, b]) & 15
            px, py = (6 + ox, 6 + oy) if sub else (9 + 2 * ox, 9 + 2 * oy)
            cols = min(n + ov, w - x0)
            blk = t[py:py + n + ov, px:px + cols].copy()
            if overlap and b > 0:
                for j in range(min(ov, cols)):
                    blk[:, j] = np.clip(round2(st[:, x0 + j] * wts[j][0] + blk[:, j] * wts[j][1], 5), gmin, gmax)
            st[:, x0:x0 + cols] = blk
        stripes.append(st)
    img = np.zeros((h, w), dtype=np.int64)
    for y in range(h):
        s, i = y // n, y % n
        v = stripes[s][i]
        if overlap and s > 0 and i < ov:
            v = np.clip(round2(stripes[s - 1][i + n] * wts[i][0] + v * wts[i][1], 5), gmin, gmax)
        img[y] = v
    return img


def synth(planes, bd, g, seed):
    """[Y, U, V] (4:2:0, even sizes) with the grain of parameter set g and grain_seed `seed` added"""
    y, u, v = [np.asarray(p, dtype=np.int64) for p in planes]
    h, w = y.shape
    assert u.shape == v.shape == (h // 2, w // 2) and not (w & 1 or h & 1)
    csfl = g["chroma_scaling_from_luma"]
    if not g["point_y"] and not g["point_cb"] and not g["point_cr"] and not csfl:
        return [y.copy(), u.copy(), v.copy()]
    tl, tcb, tcr = templates(g, bd, seed)
    stripes, blocks = (h // 2 + 15) // 16, (w // 2 + 15) // 16
    offs = block_offsets(seed, stripes, blocks)
    shift = g["grain_scaling_minus_8"] + 8
    sc = bd - 8
    if g["clip_to_restricted_range"]:
        lo, hi_y, hi_c = 16 << sc, 235 << sc, (235 if g["mc_identity"] else 240) << sc
    else:
        lo, hi_y, hi_c = 0, (1 << bd) - 1, (1 << bd) - 1
    out = [y.copy(), u.copy(), v.copy()]
    lut_y = scaling_lut(g["point_y"])
    if g["point_y"]:
        n = noise_image(tl, offs, w, h, 0, bd, g["overlap_flag"])
        out[0] = np.clip(y + round2(scale_lut(lut_y, y, bd) * n, shift), lo, hi_y)
    x1 = np.minimum(np.arange(0, w, 2) + 1, w - 1)
    avg = round2(y[0::2, 0::2] + y[0::2][:, x1], 1)
    for pl, (src, t, pts, mult, lmult, off) in enumerate(((u, tcb, g["point_cb"], g["cb_mult"], g["cb_luma_mult"], g["cb_offset"]),
                                                         (v, tcr, g["point_cr"], g["cr_mult"], g["cr_luma_mult"], g["cr_offset"])), 1):
        if not pts and not csfl:
            continue
        if csfl:
            merged, lut = avg, lut_y
        else:
            merged = np.clip(((avg * (lmult - 128) + src * (mult - 128)) >> 6) + ((off - 256) << sc), 0, (1 << bd) - 1)
            lut = scaling_lut(pts)
        n = noise_image(t, offs, w // 2, h // 2, 1, bd, g["overlap_flag"])
        out[pl] = np.clip(src + round2(scale_lut(lut, merged, bd) * n, shift), lo, hi_c)
    return out


# ---------------------------------------------------------------- the C struct, frames and the cases both test modules share
PARAMS_SIZE = 164


def pack(g):
    """the parameter set as include/av1mi.h's av1mi_grain_params"""
    b = bytearray([len(g["point_y"]), len(g["point_cb"]), len(g["point_cr"]), g["chroma_scaling_from_luma"]])
    for key, n in (("point_y", 14), ("point_cb", 10), ("point_cr", 10)):
        pts = list(g[key]) + [(0, 0)] * (n - len(g[key]))
        for x, y in pts[:n]:
            b += bytes([x, y])
    b += bytes([g["grain_scaling_minus_8"], g["ar_coeff_lag"], g["ar_coeff_shift_minus_6"], g["grain_scale_shift"]])
    for key, n in (("ar_coeffs_y", 24), ("ar_coeffs_cb", 25), ("ar_coeffs_cr", 25)):
        assert len(g[key]) == n
        b += np.array(g[key], dtype=np.int8).tobytes()
    b += bytes([g["overlap_flag"], g["clip_to_restricted_range"], g["cb_mult"], g["cb_luma_mult"], g["cr_mult"], g["cr_luma_mult"]])
    b += np.array([g["cb_offset"], g["cr_offset"]], dtype="<u2").tobytes()
    b += bytes([g["mc_identity"], 0, 0, 0])
    assert len(b) == PARAMS_SIZE
    return bytes(b)


def unpack(b):
    """av1mi_grain_params bytes as a parameter set"""
    b = bytes(b)
    assert len(b) == PARAMS_SIZE
    ny, ncb, ncr, csfl = b[0], b[1], b[2], b[3]
    pts = lambda at, n: [(b[at + 2 * k], b[at + 2 * k + 1]) for k in range(n)]
    co = lambda at, n: [int(v) for v in np.frombuffer(b[at:at + n], dtype=np.int8)]
    off = np.frombuffer(b[156:160], dtype="<u2")
    return params(point_y=pts(4, ny), point_cb=pts(32, ncb), point_cr=pts(52, ncr), chroma_scaling_from_luma=csfl, grain_scaling_minus_8=b[72],
                  ar_coeff_lag=b[73], ar_coeff_shift_minus_6=b[74], grain_scale_shift=b[75], ar_coeffs_y=co(76, 24), ar_coeffs_cb=co(100, 25),
                  ar_coeffs_cr=co(125, 25), overlap_flag=b[150], clip_to_restricted_range=b[151], cb_mult=b[152], cb_luma_mult=b[153],
                  cr_mult=b[154], cr_luma_mult=b[155], cb_offset=int(off[0]), cr_offset=int(off[1]), mc_identity=b[160])


def frame_bytes(planes, bd):
    """[Y, U, V] as a tight planar frame"""
    return b"".join(np.ascontiguousarray(p).astype("<u2" if bd > 8 else np.uint8).tobytes() for p in planes)


def frame_planes(raw, w, h, bd):
    a = np.frombuffer(bytes(raw), dtype="<u2" if bd > 8 else np.uint8).astype(np.int64)
    return [a[:w * h].reshape(h, w), a[w * h:w * h * 5 // 4].reshape(h // 2, w // 2), a[w * h * 5 // 4:].reshape(h // 2, w // 2)]


def synth_frames(raw, w, h, bd, g, seeds):
    """a chunk of len(seeds) tight frames with its grain"""
    fb = w * h * 3 // 2 * (2 if bd > 8 else 1)
    return b"".join(frame_bytes(synth(frame_planes(raw[f * fb:(f + 1) * fb], w, h, bd), bd, g, s), bd) for f, s in enumerate(seeds))


def content(kind, w, h, bd, n, seed=1):
    """n tight frames: "ramps" - ramps with noise over the whole range; "max" - saturated samples; "zero"; "low" / "high" - near either end"""
    rng = np.random.default_rng(seed)
    mx = (1 << bd) - 1
    out = []
    for f in range(n):
        fr = []
        for pw, ph in ((w, h), (w // 2, h // 2), (w // 2, h // 2)):
            if kind == "max":
                p = np.full((ph, pw), mx)
            elif kind == "zero":
                p = np.zeros((ph, pw))
            else:
                ramp = np.add.outer(np.arange(ph) * (mx // 2) // max(ph - 1, 1), np.arange(pw) * (mx // 2) // max(pw - 1, 1))
                p = np.clip(ramp + rng.integers(-6 << (bd - 8), (6 << (bd - 8)) + 1, (ph, pw)) + 3 * f, 0, mx)
            fr.append(p.astype(np.int64))
        out.append(frame_bytes(fr, bd))
    return b"".join(out)


def _coeffs(rng, lag, extreme):
    """(luma, cb, cr) coefficients at a lag, the chroma planes' luma tap behind theirs: small ones, or the whole range with both ends"""
    n = 2 * lag * (lag + 1)

    def one(extra):
        c = rng.integers(-128, 128, n + extra) if extreme else rng.integers(-24, 25, n + extra)
        if extreme:
            c[:2] = [-128, 127]
        return [int(v) for v in c] + [0] * (24 - n)
    return one(0), one(1), one(1)


def parameter_sets():
    """name -> parameter set: every field of film_grain_params at work somewhere"""
    rng = np.random.default_rng(9)
    eight = lambda lo, hi: [(16 + 32 * k, int(v)) for k, v in enumerate(np.linspace(lo, hi, 8).round())]
    sets = {"fixed20": fixed_params(20), "fixed50": fixed_params(50), "zero": params(),
            "eight": params(point_y=eight(10, 90), point_cb=eight(60, 5), point_cr=[(0, 0), (40, 70), (41, 10), (200, 255), (255, 3)]),
            "full": params(point_y=[(k * 19, int(v)) for k, v in enumerate(rng.integers(0, 256, 14))],
                           point_cb=[(3 + k * 25, int(v)) for k, v in enumerate(rng.integers(0, 256, 10))],
                           point_cr=[(k * 28, int(v)) for k, v in enumerate(rng.integers(0, 256, 10))], grain_scaling_minus_8=0),
            "luma_only": params(point_y=[(0, 80), (255, 20)]), "chroma_only": params(point_cb=[(0, 40), (255, 90)], point_cr=[(128, 64)]),
            "from_luma": params(point_y=eight(20, 100), chroma_scaling_from_luma=1),
            "restricted": params(point_y=[(0, 255), (255, 255)], point_cb=[(0, 255), (255, 255)], point_cr=[(0, 255), (255, 255)], grain_scaling_minus_8=0,
                                 clip_to_restricted_range=1),
            "restricted_identity": params(point_y=[(0, 200)], point_cb=[(0, 255)], point_cr=[(0, 255)], grain_scaling_minus_8=0, clip_to_restricted_range=1, mc_identity=1),
            "no_overlap": dict(fixed_params(40), overlap_flag=0, grain_scale_shift=1),
            "mults": dict(fixed_params(30), cb_mult=200, cb_luma_mult=90, cb_offset=300, cr_mult=0, cr_luma_mult=255, cr_offset=0, grain_scale_shift=2,
                          grain_scaling_minus_8=1)}
    for lag in (1, 2, 3):
        for extreme in (False, True):
            y, cb, cr = _coeffs(rng, lag, extreme)
            sets["lag%d%s" % (lag, "x" if extreme else "")] = dict(fixed_params(40), ar_coeff_lag=lag, ar_coeffs_y=y, ar_coeffs_cb=cb, ar_coeffs_cr=cr,
                                                                  ar_coeff_shift_minus_6=lag if extreme else 1)
    sets["luma_tap"] = dict(fixed_params(40), ar_coeffs_cb=[100] + [0] * 24, ar_coeffs_cr=[-128] + [0] * 24)
    sets["lag3x_shift6"] = dict(sets["lag3x"], ar_coeff_shift_minus_6=0)
    return sets


SEEDS = [0, 0xFFFF, 7391]
SIZES = [(8, 8), (34, 34), (98, 66), (200, 120)]


def cases():
    """(name, bd, w, h, parameter set, seeds, raw frames): what the host program and the kernel must both reproduce"""
    sets = parameter_sets()
    out = []
    for bd in (8, 10):
        for w, h in SIZES:
            out.append(("fixed20/%dx%d/%d" % (w, h, bd), bd, w, h, sets["fixed20"], SEEDS, content("ramps", w, h, bd, 3, seed=w + bd)))
        for i, name in enumerate(sorted(sets)):
            w, h = (98, 66) if i & 1 else (34, 34)
            out.append(("%s/%dx%d/%d" % (name, w, h, bd), bd, w, h, sets[name], SEEDS[:2] if i & 2 else SEEDS[1:], content("ramps", w, h, bd, 2, seed=i)))
        for kind in ("max", "zero"):
            for name in ("fixed50", "restricted", "eight"):
                out.append(("%s/%s/%d" % (name, kind, bd), bd, 34, 34, sets[name], [1234], content(kind, 34, 34, bd, 1)))
    return out


# ---------------------------------------------------------------- film_grain_params (spec 5.9.30) of a parameter set, and OBUs
def _put(bits, v, n):
    bits.extend((v >> i) & 1 for i in range(n - 1, -1, -1))


def params_bits(g, seed, inter):
    """the bits from apply_grain to clip_to_restricted_range of a shown frame that updates its grain, 4:2:0"""
    bits = []
    _put(bits, 1, 1)                      # apply_grain
    _put(bits, seed, 16)
    if inter:
        _put(bits, 1, 1)                  # update_grain
    _put(bits, len(g["point_y"]), 4)
    for x, y in g["point_y"]:
        _put(bits, x, 8)
        _put(bits, y, 8)
    _put(bits, g["chroma_scaling_from_luma"], 1)
    if g["chroma_scaling_from_luma"] or not g["point_y"]:   # 4:2:0 without luma points carries no chroma points either
        assert not g["point_cb"] and not g["point_cr"], "not a set a 4:2:0 stream can carry"
    else:
        for key in ("point_cb", "point_cr"):
            _put(bits, len(g[key]), 4)
            for x, y in g[key]:
                _put(bits, x, 8)
                _put(bits, y, 8)
    _put(bits, g["grain_scaling_minus_8"], 2)
    lag = g["ar_coeff_lag"]
    _put(bits, lag, 2)
    n = 2 * lag * (lag + 1)
    if g["point_y"]:
        for c in g["ar_coeffs_y"][:n]:
            _put(bits, c + 128, 8)
    for key, pts in (("ar_coeffs_cb", "point_cb"), ("ar_coeffs_cr", "point_cr")):
        if g["chroma_scaling_from_luma"] or g[pts]:
            for c in g[key][:n + (1 if g["point_y"] else 0)]:
                _put(bits, c + 128, 8)
    _put(bits, g["ar_coeff_shift_minus_6"], 2)
    _put(bits, g["grain_scale_shift"], 2)
    for pts, m, lm, off in (("point_cb", "cb_mult", "cb_luma_mult", "cb_offset"), ("point_cr", "cr_mult", "cr_luma_mult", "cr_offset")):
        if g[pts]:
            _put(bits, g[m], 8)
            _put(bits, g[lm], 8)
            _put(bits, g[off], 9)
    _put(bits, g["overlap_flag"], 1)
    _put(bits, g["clip_to_restricted_range"], 1)
    return bits


def parse_params(bits, at, inter):
    """(parameter set, seed, the bit behind clip_to_restricted_range) of the film_grain_params that start at bit `at`; None where the bits
    are no such string (apply_grain or update_grain 0, too many points, points out of order, the end of the bits)"""
    pos = [at]

    def get(n):
        if pos[0] + n > len(bits):
            raise IndexError
        v = 0
        for b in bits[pos[0]:pos[0] + n]:
            v = v << 1 | b
        pos[0] += n
        return v

    def points(most):
        n = get(4)
        if n > most:
            raise IndexError
        pts = [(get(8), get(8)) for _ in range(n)]
        if any(b[0] <= a[0] for a, b in zip(pts[:-1], pts[1:])):
            raise IndexError
        return pts
    try:
        if get(1) != 1:
            return None
        seed = get(16)
        if inter and get(1) != 1:
            return None
        g = params()
        g["point_y"] = points(14)
        g["chroma_scaling_from_luma"] = get(1)
        if not g["chroma_scaling_from_luma"] and g["point_y"]:
            g["point_cb"], g["point_cr"] = points(10), points(10)
        g["grain_scaling_minus_8"], g["ar_coeff_lag"] = get(2), get(2)
        n = 2 * g["ar_coeff_lag"] * (g["ar_coeff_lag"] + 1)
        if g["point_y"]:
            g["ar_coeffs_y"] = [get(8) - 128 for _ in range(n)] + [0] * (24 - n)
        for key, pts in (("ar_coeffs_cb", "point_cb"), ("ar_coeffs_cr", "point_cr")):
            if g["chroma_scaling_from_luma"] or g[pts]:
                k = n + (1 if g["point_y"] else 0)
                g[key] = [get(8) - 128 for _ in range(k)] + [0] * (25 - k)
        g["ar_coeff_shift_minus_6"], g["grain_scale_shift"] = get(2), get(2)
        for pts, m, lm, off in (("point_cb", "cb_mult", "cb_luma_mult", "cb_offset"), ("point_cr", "cr_mult", "cr_luma_mult", "cr_offset")):
            if g[pts]:
                g[m], g[lm], g[off] = get(8), get(8), get(9)
        g["overlap_flag"], g["clip_to_restricted_range"] = get(1), get(1)
    except IndexError:
        return None
    return g, seed, pos[0]


def to_bits(data):
    return [(b >> (7 - i)) & 1 for b in bytes(data) for i in range(8)]


def to_bytes(bits):
    bits = list(bits) + [0] * (-len(bits) % 8)
    return bytes(int("".join(map(str, bits[i:i + 8])), 2) for i in range(0, len(bits), 8))


def obus(data):
    """[(type, where the OBU starts, where its payload starts, where it ends)] of a stream of OBUs that carry their size"""
    out, i = [], 0
    while i < len(data):
        head = data[i]
        assert head & 2, "an OBU without a size field"
        j = i + 1 + (1 if head & 4 else 0)
        size, k = 0, 0
        while True:
            size |= (data[j] & 0x7F) << (7 * k)
            j, k = j + 1, k + 1
            if not data[j - 1] & 0x80:
                break
        out.append(((head >> 3) & 15, i, j, j + size))
        i = j + size
    return out


def leb128(v):
    out = bytearray()
    while True:
        out.append((v & 0x7F) | (0x80 if v >> 7 else 0))
        v >>= 7
        if not v:
            return bytes(out)


def find_params(data, seed, inter, limit=2048, length=None):
    """the film_grain_params of a frame OBU's payload (OBU_FRAME: the header, byte alignment, tile data): (parameter set, first bit, the
    bit behind) of the one place within the first `limit` bits where a string with this seed parses and only zero bits follow up to the
    byte's end - of `length` bits where the caller knows the string's form (a long string of coefficients can hold a shorter one that
    parses); asserts that there is exactly one"""
    bits = to_bits(data[:limit // 8 + 64])
    head = [1] + [(seed >> i) & 1 for i in range(15, -1, -1)] + ([1] if inter else [])
    found = []
    for at in range(min(limit, len(bits) - len(head))):
        if bits[at:at + len(head)] != head:
            continue
        r = parse_params(bits, at, inter)
        if r and r[1] == seed and not any(bits[r[2]:r[2] + (-r[2] % 8)]) and length in (None, r[2] - at):
            found.append((r[0], at, r[2]))
    assert len(found) == 1, "film_grain_params: %d candidates" % len(found)
    return found[0]


def header_params(n, estimate=False, lag=0, table=None, coeffs=None):
    """the set this encoder's frame headers carry with film_grain = N (fg_synth_rule.h: av1mi_fgs_header_params): the fixed table, or the
    estimate's 24 values [plane][8] at x = 16 + 32 k; with a lag the fit's coefficients [plane][25] at shift 7, the luma tap 0"""
    if not estimate:
        g = fixed_params(n)
    else:
        t = np.asarray(table).reshape(3, 8)
        g = params(**{key: [(16 + 32 * k, int(t[pl][k])) for k in range(8)] for pl, key in enumerate(("point_y", "point_cb", "point_cr"))})
    if lag:
        c, n_pos = np.asarray(coeffs).reshape(3, 25), 2 * lag * (lag + 1)
        g.update(ar_coeff_lag=lag, ar_coeff_shift_minus_6=1, ar_coeffs_y=[int(v) for v in c[0][:n_pos]] + [0] * (24 - n_pos),
                 ar_coeffs_cb=[int(v) for v in c[1][:n_pos]] + [0] * (25 - n_pos), ar_coeffs_cr=[int(v) for v in c[2][:n_pos]] + [0] * (25 - n_pos))
    return g
