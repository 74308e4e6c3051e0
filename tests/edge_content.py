"""Patterned content and the case matrix of the edge tests (tests/test_edges.py on the GPU, tests/test_edges_oracle.py on the CPU).

Plain numpy, no GPU.  Every generator returns [Y, U, V] uint16 planes (w x h luma, 4:2:0 chroma) with samples in 0..maxv,
maxv = 2^bd - 1, and takes a frame number `t`: frame t is the pattern displaced by (sx * t, sy * t) samples plus half a sample on
odd frames, so that P frames find quarter-sample vectors and the 8-tap interpolation overshoots the full-range edges.  U carries the
opposite extreme of the luma pattern (chroma from luma then needs a negative alpha), V the same one.
"""
import numpy as np


def maxv_of(bd):
    return (1 << bd) - 1


def _checker(period):
    return lambda X, Y: ((X // period + Y // period) & 1).astype(np.float64)


def _dct_signs(n):
    """in every n x n block: the sign of one 2-D DCT-II basis function as 0 / 1, a different (row, column) frequency per block
    (DC and the highest frequencies first); DC blocks alternate between the two extremes"""
    freqs = [(0, 0), (n - 1, n - 1), (0, n - 1), (n - 1, 0), (1, 0), (0, 1), (1, 1), (n // 2, n // 2), (n - 2, 1), (3, n - 3), (n // 4, 0),
             (0, n // 4), (n - 1, n // 2), (5, 7)]

    def f(X, Y):
        bx, by, x, y = X // n, Y // n, X % n, Y % n
        k = (bx * 5 + by * 3) % len(freqs)
        fr = np.array(freqs)[k]
        v, u = fr[..., 0], fr[..., 1]
        s = np.cos(np.pi * (2 * x + 1) * u / (2 * n)) * np.cos(np.pi * (2 * y + 1) * v / (2 * n))
        flip = ((bx + by) & 1) == 1
        return ((s >= -1e-9) ^ flip).astype(np.float64)
    return f


def _impulses(on_white):
    """isolated single samples on a 7 x 5 lattice (staggered per row of the lattice): maxv on 0, or 0 on maxv"""
    def f(X, Y):
        hit = ((X + 3 * (Y // 5)) % 7 == 0) & (Y % 5 == 2)
        return (hit ^ on_white).astype(np.float64)
    return f


def _steps(spacing, vertical):
    """full-range steps every `spacing` samples: vertical edges (columns) or horizontal ones (rows)"""
    return lambda X, Y: (((X if vertical else Y) // spacing) & 1).astype(np.float64)


PATTERNS = {
    "checker1": lambda bs: _checker(1), "checker2": lambda bs: _checker(2), "checker4": lambda bs: _checker(4),
    "checker8": lambda bs: _checker(8), "checker_bs": lambda bs: _checker(1 << bs),
    "dct_signs": lambda bs: _dct_signs(32 if bs <= 5 else 64),
    "impulse_white": lambda bs: _impulses(False), "impulse_black": lambda bs: _impulses(True),
    "steps4_v": lambda bs: _steps(4, True), "steps8_h": lambda bs: _steps(8, False), "steps16_v": lambda bs: _steps(16, True),
    "steps4_h": lambda bs: _steps(4, False), "steps8_v": lambda bs: _steps(8, True), "steps16_h": lambda bs: _steps(16, False),
}


def _render(fn, w, h, ox2, oy2):
    """fn at the sample grid displaced by (ox2, oy2) half-samples: evaluated at twice the resolution, then 2 x 2 averages (a
    half-sample displacement gives mid-level samples on every edge)"""
    Y2, X2 = np.mgrid[0:2 * h, 0:2 * w]
    v = fn((X2 + ox2) // 2, (Y2 + oy2) // 2)
    return v.reshape(h, 2, w, 2).mean(axis=(1, 3))


def frame(pattern, w, h, bd, bs=5, t=0, motion=(2, -1)):
    """[Y, U, V] of `pattern` (a PATTERNS key) at frame t; bs: the leaf size log2 (checker_bs, dct_signs follow it)"""
    mx = maxv_of(bd)
    fn = PATTERNS[pattern](bs)
    ox2, oy2 = 2 * motion[0] * t + (t & 1), 2 * motion[1] * t + (t & 1)
    y = np.rint(_render(fn, w, h, ox2, oy2) * mx)
    c = _render(fn, w // 2, h // 2, ox2 // 2, oy2 // 2)
    u = np.rint((1.0 - c) * mx)
    v = np.rint(c * mx)
    return [a.astype(np.uint16) for a in (y, u, v)]


def clip(pattern, w, h, bd, n, bs=5, motion=(2, -1)):
    return [frame(pattern, w, h, bd, bs, t, motion) for t in range(n)]


def synth(oracle, w, h, bd, n, seed):
    """the oracle's synthetic clip at any even size (generated at the next multiple of 8 plus a margin, then cropped)"""
    big = [oracle.synthclip_frame(((w + 7) & ~7) + 8, ((h + 7) & ~7) + 8, bd, seed=seed, t=t) for t in range(n)]
    return [[f[0][:h, :w].copy(), f[1][:h // 2, :w // 2].copy(), f[2][:h // 2, :w // 2].copy()] for f in big]


def source(oracle, case):
    c = case["content"]
    if c[0] == "synth":
        return synth(oracle, case["w"], case["h"], case["bd"], case["n"], c[1])
    return clip(c[0], case["w"], case["h"], case["bd"], case["n"], bs=case["params"].get("block_log2", 5), motion=tuple(c[1]))


# ------------------------------------------------------------------ the C ABI's parameters -> the oracle's configuration
# aom's quantizer_to_qindex (av1mi_cq_to_qindex)
QINDEX = [4 * i for i in range(62)] + [249, 255]


def oracle_config(oracle, case, t):
    """the oracle configuration of frame t of `case` (what av1mi's resolve() derives from the parameters)"""
    p = dict(case["params"])
    w, h, bd = case["w"], case["h"], case["bd"]
    bs = p.get("block_log2", 5)
    qidx = QINDEX[p.get("cq_level", 30)]
    kw = dict(min_bs_log2=p.get("min_block_log2", 3) if p.get("partition_search") else bs, max_bs_log2=bs, base_q_idx=qidx,
              disable_cdf_update=0 if p.get("cdf_update", 1) else 1, me_range=p.get("me_range", 8))
    for k in ("deblock", "subpel", "partition_search", "me_presearch", "intra_edge_filter", "cfl", "tx_search", "enable_cdef",
              "cdef_y_pri", "cdef_y_sec", "cdef_uv_pri", "cdef_uv_sec", "cdef_damping", "color_primaries", "transfer_characteristics",
              "matrix_coefficients", "color_range"):
        if k in p:
            kw[k] = p[k]
    if "intra_mode_mask" in p:
        kw["mode_mask"] = p["intra_mode_mask"]
    if "intra_angle_delta" in p:
        kw["angle_delta"] = p["intra_angle_delta"]
    if p.get("enable_lr"):
        assert p["enable_lr"] <= 2, "enable_lr 3 / 4 have no oracle"
        kw["enable_lr"] = p["enable_lr"]
    sbc, sbr = (((w + 7) & ~7) + 63) // 64, (((h + 7) & ~7) + 63) // 64
    tsb = p.get("tile_sb") or (2 if sbc > 64 or sbr > 64 else 1)
    kw["tile_w_sb"] = kw["tile_h_sb"] = tsb
    if p.get("enable_qm"):
        lvl = oracle.qm_level(qidx, p.get("qm_min", 0), p.get("qm_max", 15))
        kw.update(enable_qm=1, qm_y=lvl, qm_uv=lvl)
    fg = p.get("film_grain", 0)
    if fg:
        kw.update(film_grain=1, fg_y_scaling=min(2 * fg, 255), fg_c_scaling=fg, fg_seed=(7391 + 173 * (p.get("first_frame", 0) + t)) & 0xFFFF)
    return oracle.default_config(w, h, bd, **kw)


def oracle_encode(oracle, case, frames):
    """(temporal units, reconstructions, SSE per plane summed over the chunk) of the oracle's restatement of the chunk"""
    keyint = case["params"].get("keyint", 1)
    tus, recs, sse, ref, prev = [], [], [0, 0, 0], None, None
    for t, f in enumerate(frames):
        key = t % keyint == 0
        tu, rec, st = oracle.encode_frame(oracle_config(oracle, case, t), f, with_seq_hdr=key, ref=None if key else ref, prev_src=None if key else prev)
        tus.append(tu)
        recs.append(rec)
        sse = [a + int(b) for a, b in zip(sse, st.sse)]
        ref, prev = rec, f
    return tus, recs, sse


def dav1d_decode(tus, w, h, bd, keyint):
    """every frame of the chunk as dav1d decodes it (tools/oracle_avif.py: key frames as stills, P frames in an image sequence)"""
    import oracle_avif
    if keyint == 1:
        return [oracle_avif.decode_obus(t, w, h, bd) for t in tus]
    keys = [i + 1 for i in range(len(tus)) if i % keyint == 0]
    return oracle_avif.decode_sequence(oracle_avif.wrap_avis(tus, w, h, bd, sync=keys), w, h)


def decodes_to(got, want, bd, grain):
    """(frame, plane) of the first mismatch between dav1d's frames and the reconstruction, or None.  With film grain the decoder adds
    the grain: a bounded MSE (a desynchronised stream decodes to garbage, not to noise)"""
    if len(got) != len(want):
        return ("frames", len(got), len(want))
    for f in range(len(want)):
        for pl in range(3):
            g, r = np.asarray(got[f][pl]).astype(np.int64), np.asarray(want[f][pl]).astype(np.int64)
            if g.shape != r.shape:
                return (f, pl, "shape")
            if grain:
                if float(((g - r) ** 2).mean()) >= maxv_of(bd) ** 2 / 10 ** 2.5:
                    return (f, pl)
            elif not np.array_equal(g, r):
                return (f, pl)
    return None


# ------------------------------------------------------------------ the case matrix
def _case(name, w, h, bd, n, content, **params):
    params.setdefault("keyint", 3 if n > 1 else 1)
    return dict(name=name, w=w, h=h, bd=bd, n=n, content=content, params=params)


GEOM = dict(subpel=1, me_range=16, deblock=1, enable_lr=2)
INTRA_ALL = dict(intra_mode_mask=0x1FFF, intra_angle_delta=1, intra_edge_filter=1, cfl=1, tx_search=1)


def _geometry():
    out = []
    specs = [("8x8_bs3", 8, 8, dict(block_log2=3)), ("8x8_bs6", 8, 8, dict(block_log2=6)), ("10x10", 10, 10, dict(block_log2=4)),
             ("16x8", 16, 8, dict(block_log2=4)), ("8x16", 8, 16, dict(block_log2=3)),
             ("8x136_part", 8, 136, dict(block_log2=6, partition_search=1, min_block_log2=3, me_presearch=1)),
             ("136x8_part", 136, 8, dict(block_log2=6, partition_search=1, min_block_log2=3, me_presearch=1)),
             ("264x8_cq63", 264, 8, dict(block_log2=5, cq_level=63)), ("66x130_tile2", 66, 130, dict(block_log2=5, tile_sb=2)),
             ("4160x16_autotile", 4160, 16, dict(block_log2=5))]
    for i, (name, w, h, kw) in enumerate(specs):
        bd = 8 if i % 2 == 0 else 10
        out.append(_case("geom_%s_%db" % (name, bd), w, h, bd, 3, ("synth", 5000 + i), **GEOM, **kw))
        # the same geometry on full-range moving content
        out.append(_case("geom_%s_%db_checker" % (name, bd), w, h, bd, 3, ("checker_bs" if i % 3 else "steps4_v", (1, -3)), **GEOM, **kw))
    return out


def _quantiser():
    out = []
    for bd in (8, 10):
        for bs in (3, 4, 5, 6):
            for cq in (1, 63):
                out.append(_case("q_cq%d_bs%d_%db" % (cq, bs, bd), 72, 56, bd, 3, ("synth", 5100 + bs), block_log2=bs, cq_level=cq, subpel=1))
                for qmin, qmax in ((0, 0), (15, 15), (0, 15)):
                    out.append(_case("qm%d_%d_cq%d_bs%d_%db" % (qmin, qmax, cq, bs, bd), 40, 24, bd, 1, ("checker_bs", (0, 0)), block_log2=bs, cq_level=cq,
                                     enable_qm=1, qm_min=qmin, qm_max=qmax))
            for damp in (3, 6):
                out.append(_case("cdef15_3_d%d_bs%d_%db" % (damp, bs, bd), 72, 56, bd, 3, ("impulse_white", (1, 2)), block_log2=bs, cdef_y_pri=15, cdef_y_sec=3,
                                 cdef_uv_pri=15, cdef_uv_sec=3, cdef_damping=damp))
            out.append(_case("deblock_cq63_bs%d_%db" % (bs, bd), 72, 56, bd, 3, ("checker_bs", (3, 1)), block_log2=bs, cq_level=63, deblock=1, subpel=1))
            out.append(_case("grain50_bs%d_%db" % (bs, bd), 72, 56, bd, 3, ("synth", 5200 + bs), block_log2=bs, film_grain=50, first_frame=3))
    return out


def _content():
    out = []
    for bd in (8, 10):
        for pat in PATTERNS:
            for bs in ((5, 6) if pat == "dct_signs" else (3, 4, 5, 6)):
                w, h = (128, 64) if pat == "dct_signs" else (72, 40)
                out.append(_case("c_%s_bs%d_%db_key" % (pat, bs, bd), w, h, bd, 2, (pat, (0, 0)), block_log2=bs, keyint=1, **INTRA_ALL))
                out.append(_case("c_%s_bs%d_%db_p" % (pat, bs, bd), w, h, bd, 3, (pat, (1 + bs % 3, -(1 + bd % 3))), block_log2=bs, keyint=3, subpel=1,
                                 **INTRA_ALL))
    return out


CASES = _geometry() + _quantiser() + _content()

# the patterned inputs and quantiser edges pinned as dav1d-checked fixtures (tests/golden/index_edges.json, tools/make_golden.py --edges)
FIXTURES = ["geom_8x8_bs3_8b_checker", "geom_136x8_part_8b_checker", "geom_264x8_cq63_10b", "q_cq1_bs5_10b", "q_cq63_bs3_8b",
            "qm0_15_cq1_bs4_10b", "cdef15_3_d6_bs4_10b", "deblock_cq63_bs6_10b", "c_dct_signs_bs5_10b_key", "c_dct_signs_bs6_8b_p",
            "c_checker1_bs3_10b_p", "c_impulse_black_bs4_8b_p"]


def case(name):
    return next(c for c in CASES if c["name"] == name)


# the GPU-only tools (no oracle): every geometry and content case again with both on
GPU_ONLY = dict(cdef_search=4, enable_lr=4)


def with_gpu_only_tools(c):
    c = dict(c, name=c["name"] + "_gpu_only", params=dict(c["params"], **GPU_ONLY))
    c["params"].pop("enable_cdef", None)
    return c


GPU_ONLY_CASES = [with_gpu_only_tools(c) for c in CASES if c["name"].startswith(("geom_", "c_"))]
assert len({c["name"] for c in CASES + GPU_ONLY_CASES}) == len(CASES) + len(GPU_ONLY_CASES)

# the encoder-side decisions together (no oracle for the combination): the AQ map, the deblocking level search, the CDEF search with four
# pairs, and restoration on all planes in units of 256 with both fits and the rate term (include/av1mi.h: AV1MI_LR_RD(0) = 0xC000) -
# every geometry case, and the moving content cases at the smallest and the largest leaf; a base case's own values of these give way
DECISION_TOOLS = dict(aq_strength=4, deblock=2, cdef_search=3, enable_lr=0x2504 | 0xC000)


def with_decision_tools(c):
    c = dict(c, name=c["name"] + "_decisions", params=dict(c["params"], **DECISION_TOOLS))
    c["params"].pop("enable_cdef", None)
    return c


DECISION_CASES = [with_decision_tools(c) for c in CASES
                  if c["name"].startswith("geom_") or (c["name"].startswith("c_") and c["name"].endswith("_p") and c["params"]["block_log2"] in (3, 6))]
assert len({c["name"] for c in CASES + GPU_ONLY_CASES + DECISION_CASES}) == len(CASES) + len(GPU_ONLY_CASES) + len(DECISION_CASES)


# ------------------------------------------------------------------ a minimal sequence header reader (spec 5.5)
def color_config(seq_obu):
    """(color_description_present_flag, CP, TC, MC, color_range) of a sequence_header_obu (OBU header + leb128 size + payload); the
    values a decoder infers (2 = unspecified) when no description is present"""
    assert (seq_obu[0] >> 3) & 15 == 1, "not a sequence header OBU"
    pos, size, shift = 1, 0, 0
    while True:
        b = seq_obu[pos]
        pos += 1
        size |= (b & 0x7F) << shift
        shift += 7
        if not b & 0x80:
            break
    bits = "".join("{:08b}".format(x) for x in seq_obu[pos:pos + size])
    at = [0]

    def f(n):
        v = int(bits[at[0]:at[0] + n], 2) if n else 0
        at[0] += n
        return v
    profile = f(3)
    still, reduced = f(1), f(1)
    assert profile == 0 and not reduced
    timing, delay = f(1), f(1)
    assert not timing and not delay
    for _ in range(f(5) + 1):
        f(12)
        if f(5) > 7:
            f(1)
    wb, hb = f(4) + 1, f(4) + 1
    f(wb), f(hb)
    if f(1):   # frame_id_numbers_present_flag
        f(4), f(3)
    f(1), f(1), f(1)   # use_128x128_superblock, enable_filter_intra, enable_intra_edge_filter
    f(1), f(1), f(1), f(1)   # interintra, masked compound, warped motion, dual filter
    order_hint = f(1)
    if order_hint:
        f(1), f(1)
    force_sct = 2 if f(1) else f(1)
    if force_sct > 0 and not f(1):
        f(1)
    if order_hint:
        f(3)
    f(1), f(1), f(1)   # enable_superres, enable_cdef, enable_restoration
    high = f(1)
    assert f(1) == 0, "mono_chrome"
    desc = f(1)
    cp, tc, mc = (f(8), f(8), f(8)) if desc else (2, 2, 2)
    assert not (cp == 1 and tc == 13 and mc == 0), "sRGB + identity: 4:4:4 syntax"
    cr = f(1)
    del high, still
    return desc, cp, tc, mc, cr
