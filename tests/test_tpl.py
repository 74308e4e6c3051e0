"""GPU tests of the adaptive quantisation's temporal term (include/av1mi.h: cq_level bits 12-14, av1mi_tpl_analysis).

The analysis is restated with tests/tpl_ref.py and compared stage by stage.  What the encoder does with the map has the references the
spatial term has (tests/test_aq.py): one oracle run per quantiser index for a key frame's superblocks, and dav1d (libavif) for the syntax."""
import os
import sys

import numpy as np
import pytest

import edge_content
import tf_ref
import tpl_ref
from test_lr_chroma import split_frames

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def encode(ctx, av1mi, raw, w, h, bd, n, **kw):
    p = av1mi.default_params(w, h, bd, **kw)
    data, sizes, rep, rec = ctx.encode_chunk(p, raw, n, want_recon=True)
    return data, sizes, rep, split_frames(rec.tobytes(), w, h, bd, n)


def same_frames(a, b):
    return all(np.array_equal(x, y) for fa, fb in zip(a, b) for x, y in zip(fa, fb))


@pytest.fixture(scope="module")
def ctx(av1mi):
    c = av1mi.Context(0)
    yield c
    c.close()


_clips = {}


def the_clip(kind, w, h, bd, n):
    """(bytes, the search of every frame in the frame before it at the case's range) - computed once per clip and left unchanged"""
    key = (kind, w, h, bd, n)
    if key not in _clips:
        if kind == "pattern":
            buf = tf_ref.pattern_clip(w, h, bd, n, seed=7)[0]
        elif kind == "static":
            buf = tf_ref.pattern_clip(w, h, bd, n, seed=7, static=True)[0]
        elif kind == "noise":
            rng = np.random.default_rng(11)
            buf = tf_ref.join([[rng.integers(0, 1 << bd, (ph, pw)) for pw, ph in ((w, h), (w // 2, h // 2), (w // 2, h // 2))] for _ in range(n)], bd)
        else:
            buf = tpl_ref.half_clip(w, h, bd, n, seed=7)
        luma, W, H = tpl_ref.coded_luma(buf, w, h, bd, n)
        _clips[key] = (buf, tpl_ref.search_all(luma, W, H, range_of(bd)))
    return _clips[key]


def range_of(bd):
    return 16 if bd == 10 else 8


# ---------------------------------------------------------------- (a) the stages and the map
SIZES = [(8, 8, 8, 5), (72, 56, 8, 5), (136, 72, 8, 5), (200, 120, 8, 5), (202, 122, 8, 5), (328, 248, 10, 6)]
EXERCISED = {("pattern", 200, 120, 240), ("half", 328, 248, 240), ("half", 72, 56, 240)}   # the rule must move these maps both ways


@pytest.mark.parametrize("kind", ["pattern", "half"])
@pytest.mark.parametrize("w,h,bd,n", SIZES)
def test_stages_and_map_equal_the_rule(av1mi, ctx, w, h, bd, n, kind):
    import torch
    raw, searched = the_clip(kind, w, h, bd, n)
    R = range_of(bd)
    dev = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()
    base = av1mi.cq_to_qindex(30)
    for keyint in (1, 3, 240):
        want = tpl_ref.analysis(raw, w, h, bd, n, keyint, R, searched)
        p = av1mi.default_params(w, h, bd, keyint=keyint, me_range=R, tpl_strength=2)
        for where, got in (("host input", ctx.tpl_analysis(p, raw, n)), ("device input", ctx.tpl_analysis(p, dev.data_ptr(), n, on_device=True))):
            for stage in ("intra", "inter", "key", "flow", "beta"):
                a, b = got[stage], want[stage]
                assert a.shape == b.shape, (keyint, where, stage)
                bad = [i for i in np.ndindex(a.shape) if int(a[i]) != int(b[i])]
                assert not bad, (keyint, where, stage, bad[:4], [(int(a[i]), int(b[i])) for i in bad[:4]])
            assert got["mean_beta"] == want["mean_beta"], (keyint, where)
        assert (want["beta"] >= 0).all() and (want["beta"][-1] == 0).all()
        for tpl in (1, 2, 4):
            for aq in (0, 4):
                ref = tpl_ref.qindex_map(raw, w, h, bd, n, keyint, R, aq, tpl, base, ana=want)
                p = av1mi.default_params(w, h, bd, keyint=keyint, me_range=R, tpl_strength=tpl, aq_strength=aq)
                got = ctx.aq_qindex(p, raw, n)
                assert got.shape == ref.shape and np.array_equal(got, ref), (keyint, tpl, aq, "host input")
                assert np.array_equal(ctx.aq_qindex(p, dev.data_ptr(), n, on_device=True), ref), (keyint, tpl, aq, "device input")
                if (tpl, aq) == (4, 0) and (kind, w, h, keyint) in EXERCISED:
                    vals = sorted(set(int(v) for v in ref.ravel()))
                    assert len(vals) >= 3 and vals[0] < base < vals[-1], vals


# ---------------------------------------------------------------- (b) properties
def test_static_clip_falls_frame_by_frame(av1mi, ctx):
    """every superblock of a static clip: the key frame above every later frame, each frame above the next, the last at 0"""
    w, h, bd, n = 136, 72, 8, 5
    raw, _ = the_clip("static", w, h, bd, n)
    beta = ctx.tpl_analysis(av1mi.default_params(w, h, bd, keyint=240, tpl_strength=1), raw, n)["beta"].astype(np.int64)
    for f in range(n - 1):
        assert (beta[f] > beta[f + 1]).all(), f
    assert (beta[n - 2] > 0).all() and (beta[n - 1] == 0).all()


def test_independent_noise_has_no_dependency(av1mi, ctx):
    """uniform noise, every frame its own: no vector predicts a block better than its mean does (E|x - y| = 85 against E|x - m| = 64 of
    255), so C = I and nothing flows.  The size is a multiple of 16: an overhanging block repeats its last row or column in both
    frames, which is a dependency the content does not have (the stage test has those blocks)."""
    w, h, bd, n = 128, 80, 8, 5
    raw, _ = the_clip("noise", w, h, bd, n)
    got = ctx.tpl_analysis(av1mi.default_params(w, h, bd, keyint=240, tpl_strength=4), raw, n)
    assert got["beta"].max() <= 1 and got["mean_beta"] == 0
    assert (ctx.aq_qindex(av1mi.default_params(w, h, bd, keyint=240, tpl_strength=4), raw, n) == av1mi.cq_to_qindex(30)).all()


def test_all_key_frames_leave_the_spatial_map(av1mi, ctx):
    """keyint = 1: nothing is predicted, beta is 0 and the map is the spatial rule's; with the spatial strength 0 too it is all base, and
    the chunk differs from the strength-0 chunk in the stream alone (three header bits, a delta_q_abs of 0 per superblock)"""
    w, h, bd, n = 200, 120, 8, 3
    frames = tf_ref.split(the_clip("pattern", w, h, bd, 5)[0], w, h, bd, 5)[:n]
    for fr in frames:   # a flat right half: the spatial rule has something to tell apart
        fr[0][:, w // 2:] = 128
    raw = tf_ref.join(frames, bd)
    spatial = ctx.aq_qindex(av1mi.default_params(w, h, bd, aq_strength=4), raw, n)
    assert len(set(spatial.ravel())) >= 2
    for tpl in (1, 4):
        assert np.array_equal(ctx.aq_qindex(av1mi.default_params(w, h, bd, aq_strength=4, tpl_strength=tpl), raw, n), spatial)
        assert (ctx.aq_qindex(av1mi.default_params(w, h, bd, tpl_strength=tpl), raw, n) == av1mi.cq_to_qindex(30)).all()
    d0, s0, _, r0 = encode(ctx, av1mi, raw, w, h, bd, n, tpl_strength=0)
    for tpl in (1, 4):
        d1, s1, _, r1 = encode(ctx, av1mi, raw, w, h, bd, n, tpl_strength=tpl)
        assert same_frames(r0, r1) and d1 != d0
    da, _, _, ra = encode(ctx, av1mi, raw, w, h, bd, n, aq_strength=4)
    db, _, _, rb = encode(ctx, av1mi, raw, w, h, bd, n, aq_strength=4, tpl_strength=4)
    assert da == db and same_frames(ra, rb)


# ---------------------------------------------------------------- (c) a key frame against one oracle run per index
@pytest.mark.parametrize("w,h,bd", [(200, 120, 8), (328, 248, 10)])
def test_key_frame_equals_the_oracle_per_superblock(av1mi, oracle, ctx, w, h, bd):
    """frame 0 of a three-frame P chunk: with tiles of one superblock and the loop filters off a key frame's superblock depends on its own
    source and index only, and the oracle takes base_q_idx directly"""
    n, R = 3, range_of(bd)
    raw = the_clip("half", w, h, bd, 6 if bd == 10 else 5)[0][:n * w * h * 3 // 2 * (2 if bd > 8 else 1)]
    frames = split_frames(raw, w, h, bd, n)
    params = dict(tile_sb=1, enable_cdef=0, deblock=0, enable_lr=0, partition_search=0, keyint=240, cq_level=30, me_range=R)
    qmap = ctx.aq_qindex(av1mi.default_params(w, h, bd, tpl_strength=4, **params), raw, n)
    assert np.array_equal(qmap, tpl_ref.qindex_map(raw, w, h, bd, n, 240, R, 0, 4, av1mi.cq_to_qindex(30)))
    _, _, _, rec = encode(ctx, av1mi, raw, w, h, bd, n, tpl_strength=4, **params)
    assert len(set(qmap[0].ravel())) >= 2
    case = dict(w=w, h=h, bd=bd, params=params)
    for q in sorted(set(int(v) for v in qmap[0].ravel())):
        cfg = edge_content.oracle_config(oracle, case, 0)
        cfg.base_q_idx = q
        _, want, _ = oracle.encode_frame(cfg, frames[0])
        for r, c in zip(*np.nonzero(qmap[0] == q)):
            for pl in range(3):
                k = 64 if pl == 0 else 32
                a = rec[0][pl][k * r:k * r + k, k * c:k * c + k]
                b = np.asarray(want[pl]).astype(np.int64)[k * r:k * r + k, k * c:k * c + k]
                assert np.array_equal(a, b), "superblock (%d, %d) index %d plane %d" % (r, c, q, pl)


# ---------------------------------------------------------------- (d) dav1d decodes to the reconstruction
DECODE = [
    # w, h, bd, frames, parameters
    (200, 136, 8, 4, dict(tpl_strength=4, keyint=240, subpel=1, me_presearch=1)),
    (328, 248, 10, 5, dict(tpl_strength=4, aq_strength=2, keyint=3, subpel=1, me_presearch=1, me_range=16)),
    (264, 200, 10, 4, dict(tpl_strength=4, tile_sb=2, keyint=3)),
    (200, 136, 8, 4, dict(tpl_strength=3, keyint=240, deblock=1, enable_lr=4, cdef_search=2)),
    (200, 136, 8, 4, dict(tpl_strength=4, keyint=240, tf_frames=3, tf_strength=2)),
    (328, 248, 8, 4, dict(tpl_strength=4, keyint=3, partition_search=2, min_block_log2=3)),
]


@pytest.mark.parametrize("w,h,bd,n,extra", DECODE)
def test_dav1d_decodes_to_the_reconstruction(av1mi, w, h, bd, n, extra):
    import oracle_avif
    if not oracle_avif.have_libavif():
        pytest.skip("libavif (dav1d) is not available on this machine")
    raw = tf_ref.pattern_clip(w, h, bd, n, seed=7)[0]
    with av1mi.Context(0) as c:
        data, sizes, rep, want = encode(c, av1mi, raw, w, h, bd, n, **extra)
        p = av1mi.default_params(w, h, bd, **extra)
        src = raw
        if extra.get("tf_frames"):   # the encoder codes, and reports against, the filtered key frames
            src = c.temporal_filter(p, raw, n, want_mv=False)[0].tobytes()
        qmap = c.aq_qindex(p, src, n)
    assert len(set(qmap.ravel())) >= 2, "the content moves no superblock off the base index"
    frames = split_frames(src, w, h, bd, n)
    tus, off = [], 0
    for s in sizes:
        tus.append(data[off:off + s])
        off += s
    got = edge_content.dav1d_decode(tus, w, h, bd, extra["keyint"])
    assert len(got) == n
    tot = [0, 0, 0]
    for f in range(n):
        for pl in range(3):
            assert np.array_equal(np.asarray(got[f][pl]).astype(np.int64), want[f][pl]), "frame %d plane %d" % (f, pl)
            tot[pl] += int(((want[f][pl] - frames[f][pl]) ** 2).sum())
    assert [int(x) for x in rep.sse] == tot


# ---------------------------------------------------------------- (e) reuse and determinism
def test_workspace_reuse_and_determinism(av1mi):
    w, h, bd, n = 200, 120, 8, 5
    raw, _ = the_clip("pattern", w, h, bd, n)
    runs = [dict(tpl_strength=s, keyint=240, subpel=1) for s in (0, 4, 0, 2)] + [dict(tpl_strength=2, aq_strength=3, keyint=3, deblock=1)]
    seen = {}
    with av1mi.Context(0) as c:
        for kw in runs:
            d, s, _, r = encode(c, av1mi, raw, w, h, bd, n, **kw)
            d2, s2, _, r2 = encode(c, av1mi, raw, w, h, bd, n, **kw)
            assert d == d2 and s == s2 and same_frames(r, r2), kw
            with av1mi.Context(0) as fresh:
                d0, s0, _, r0 = encode(fresh, av1mi, raw, w, h, bd, n, **kw)
            assert d == d0 and s == s0 and same_frames(r, r0), kw
            if kw["tpl_strength"] == 0:   # the packed field with strength 0 is the plain CQ value, before and after a run with the term on
                plain = {k: v for k, v in kw.items() if k != "tpl_strength"}
                dp, sp, _, rp = encode(c, av1mi, raw, w, h, bd, n, cq_level=30, **plain)
                assert d == dp and s == sp and same_frames(r, rp), kw
                assert seen.setdefault(0, d) == d
            seen[kw["tpl_strength"], kw.get("aq_strength", 0)] = d
    assert seen[4, 0] != seen[0] and seen[2, 0] != seen[0] and seen[4, 0] != seen[2, 0]
