"""The edge matrix of the restoration decisions (tests/test_lr_edges.py on the GPU, tests/test_lr_edges_content.py on the CPU): the
smallest frames, the extreme quantisers and the full-range patterns of tests/edge_content.py, fed to the self-guided fit, the Wiener
fit, the rate term and the three unit sizes, whose restatements (tests/lr_rd_ref.py and what it builds on) had only seen smoothed noise
at middling quantisers.  Plain numpy, no GPU.

A case is two key frames (keyint = 1) of one pattern, the second displaced by the case's motion.  `modes` gives the enable_lr values a
case runs: six low bytes at each of its unit shifts, each with the rate term off and at its scales.  `probe` gives what the CPU test
tallies per unit beyond lr_rd_ref.candidates' tables: the Wiener fit's 27 sums and whether its refit ran, and the five sums of each
of the 16 self-guided sets."""
import numpy as np

import edge_content as E
import lr_rd_ref as ref
import lr_ref
import lr_unit_ref as uref
import sgr_fit_ref
import wiener_fit_ref

LOW = (1, 2, 0x104, 0x403, 0x402, 0x504)
ALL = 0x504   # both fits, every set, on all three planes: the superset lr_rd_ref.view cuts every mode from


def _case(w, h, bd, pattern, cq, shifts, motion=(1, -3), scales=(0, 1), **extra):
    name = "%dx%d_%db_%s_cq%d" % (w, h, bd, pattern, cq)
    return dict(name=name, w=w, h=h, bd=bd, pattern=pattern, cq=cq, shifts=tuple(shifts), motion=motion, scales=tuple(scales), extra=extra)


CASES = [
    _case(8, 8, 8, "checker1", 30, (0, 2)),                       # 4x4 chroma, one slice of 8 rows, a frame far below a unit of 256
    _case(10, 10, 10, "checker2", 30, (2,)),                      # signalled size != coded size at the smallest size
    _case(16, 8, 10, "checker_bs", 63, (0,), scales=(0, 1, 3), block_log2=3),   # the fitted Wiener candidate absent, self-guided sets present
    _case(8, 136, 8, "steps4_v", 1, (0, 1), scales=(0, 1, 2)),    # two unit rows of one 8-column cell; lambda at its floor
    _case(136, 8, 10, "impulse_white", 1, (0, 1), motion=(2, 1), scales=(0, 1, 2)),   # the second chroma cell of a pair is 4 columns wide
    _case(264, 8, 10, "checker4", 63, (0, 2), scales=(0, 1, 3), deblock=1),   # every tap at its clamp; the largest lambda
    _case(66, 130, 10, "steps4_h", 30, (0, 1), tile_sb=2),        # the reference carried across a tile
    _case(72, 56, 10, "checker1", 1, (0,), scales=(0, 1, 2)),     # 15 of 24 candidates absent, all-zero fitted taps
    _case(72, 56, 10, "checker1", 63, (1,), scales=(0, 1, 3), block_log2=3),   # choice 23 at the largest lambda
    _case(72, 56, 8, "impulse_black", 63, (0,), motion=(2, 1), scales=(0, 1, 3)),   # clamped taps, and the refit
    _case(72, 56, 8, "flat", 30, (0,)),                           # every sum zero, equal errors: the first minimum must be "off"
    _case(72, 56, 10, "flat", 30, (0,)),
    _case(392, 264, 10, "checker1", 63, (2,), scales=(0, 1, 3), block_log2=3),   # sums beyond 32 bits at units of 256
]
assert len({c["name"] for c in CASES}) == len(CASES)


def flat(w, h, bd):
    """flat planes at the extremes: luma at maxv, U at 0, V at mid-level"""
    mx = E.maxv_of(bd)
    cw, ch = w // 2, h // 2
    return [np.full((h, w), mx, np.uint16), np.zeros((ch, cw), np.uint16), np.full((ch, cw), 1 << (bd - 1), np.uint16)]


def frames(case, n=2):
    if case["pattern"] == "flat":
        return [flat(case["w"], case["h"], case["bd"]) for _ in range(n)]
    return E.clip(case["pattern"], case["w"], case["h"], case["bd"], n, bs=case["extra"].get("block_log2", 5), motion=case["motion"])


def params(case):
    """the encoder's parameters of a case beside enable_lr"""
    return dict(case["extra"], cq_level=case["cq"], keyint=1)


def lam(case, s):
    """lambda of the case at scale s (None: the rate term off)"""
    return 0 if s is None else ref.lam(ref.qindex_of_cq(case["cq"]), case["bd"], s)


def modes(case):
    """[(unit shift, low bytes and fit bits)]; each runs with the rate term off and at every scale of the case"""
    return [(shift, low) for shift in case["shifts"] for low in LOW]


def value(shift, low, s):
    return shift << 12 | low | (0 if s is None else ref.rd_field(s))


RUNS = [(ci, shift, low) for ci, c in enumerate(CASES) for shift, low in modes(c)]
RUN_IDS = ["%s-u%d-%#x" % (CASES[ci]["name"], 64 << shift, low) for ci, shift, low in RUNS]


def restored(pl, low):
    """does the mode restore plane pl"""
    return pl == 0 or (low & 0xFF) in (3, 4)


def oracle_planes(oracle, case, f):
    """(source, pre-CDEF, CDEF) planes of frame f of a case at the signalled size, from the oracle"""
    w, h, bd = case["w"], case["h"], case["bd"]
    src = frames(case)[f]
    out = []
    for cdef in (0, 1):
        c = dict(w=w, h=h, bd=bd, params=dict(params(case), enable_cdef=cdef))
        out.append(oracle.encode_frame(E.oracle_config(oracle, c, 0), src)[1])
    crop = lambda planes: [np.asarray(p[:(h + (i > 0)) >> (i > 0), :(w + (i > 0)) >> (i > 0)], dtype=np.int64) for i, p in enumerate(planes)]
    return crop(src), crop(out[0]), crop(out[1])


def candidates(pre, cdef, src, bd, sub, shift):
    return ref.candidates(pre, cdef, src, bd, sub, shift << 12 | ALL)


def fit_record(cands, i, j, c):
    """av1mi_lr_fit_result's record of a unit whose decision before the Wiener fit is c: (choice, set, xqd0, xqd1)"""
    if c >= 7:
        return (c,) + tuple(cands["coef"][i][j][c])
    if c >= 4:
        return (c, 9) + tuple(lr_ref.SGR_WEIGHTS[c - 4])
    return (c, 0, 0, 0)


def before_wiener_fit(cands):
    """the view without candidate 23: what the decision before the Wiener fit sees"""
    return dict(cands, err=[[u[:23] + [None] for u in row] for row in cands["err"]])


def probe(pre, cdef, src, bd, sub, shift):
    """per unit [unit row][unit column] a dict: wsums = the Wiener fit's 27 sums, winfo = its info (v / h: clamped, refit), ssums[t] =
    the five sums of self-guided set t"""
    pre, cdef, src = (np.asarray(p, dtype=np.int64) for p in (pre, cdef, src))
    with uref.units_at(shift):
        rows, cols = lr_ref.unit_bounds(src.shape[0], src.shape[1], sub)
        outs = [sgr_fit_ref.plane_outputs(pre, cdef, bd, sub, t) for t in range(16)]
    dv, dh = wiener_fit_ref.plane_d(pre, cdef, sub)
    out = []
    for y0, y1 in rows:
        out.append([])
        for x0, x1 in cols:
            sl = (slice(y0, y1), slice(x0, x1))
            info = {}
            ws = wiener_fit_ref.unit_sums(cdef[sl], src[sl], [d[sl] for d in dv], [d[sl] for d in dh])
            wiener_fit_ref.fit(ws, sub, info)
            ss = [sgr_fit_ref.unit_sums(cdef[sl], src[sl], outs[t][0][sl], outs[t][1][sl], t) for t in range(16)]
            out[-1].append(dict(wsums=ws, winfo=info, ssums=ss, rows=y1 - y0, cols=x1 - x0))
    return out
