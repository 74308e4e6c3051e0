"""GPU tests of the frame term of the quantiser (include/av1mi.h: cq_level bits 20-22, av1mi_tpl_frame_q, av1mi_frame_q_result; DESIGN.md
§3 item 1e): every frame of a chunk its own base_q_idx from the chunk's look-ahead.

The decision is restated with tests/fq_ref.py on tests/tpl_ref.py's analysis and compared stage by stage.  What the encoder does with
the frames' indices has an exact reference for whole temporal units: oracle.encode_frame takes one configuration per frame, so a chunk
with fq_strength alone is the oracle run frame by frame with cfg.base_q_idx = q_f.  With the superblock terms on top the references are
the delta-q features' (tests/test_tpl.py): one oracle run per quantiser index for a key frame's superblocks, and dav1d for the syntax."""
import os
import sys

import numpy as np
import pytest

import edge_content
import fq_ref
import tf_ref
import tpl_ref
from test_lr_chroma import split_frames
from test_tpl import SIZES, encode, range_of, same_frames, the_clip   # (the clips and their searches are computed once for both modules)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

BASE = 120   # cq_level 30


@pytest.fixture(scope="module")
def ctx(av1mi):
    c = av1mi.Context(0)
    yield c
    c.close()


def tus_of(data, sizes):
    out, off = [], 0
    for s in sizes:
        out.append(data[off:off + s])
        off += s
    return out


# ---------------------------------------------------------------- (a) the stages and the map
# what the content must give at strength 4 (computed on the CPU from tpl_ref, base 120): the rule is exercised both ways
STEPS = {("static", 136, 72, 240): [-3, -2, -1, 2, 4], ("pattern", 200, 120, 240): [-3, -3, -1, 1, 4], ("pattern", 200, 120, 3): [-3, -1, 3, -1, 3],
         ("half", 328, 248, 240): [-3, -2, -1, 0, 2, 4]}


def check_exercised(kind, w, h, keyint, want):
    """on the reference, not the library: steps of both signs, indices on both sides of 120 - two q contexts - and, where the whole
    clip is one key-frame interval, the +4 clamp (intervals of three frames end at +3)"""
    k = want["steps"]
    assert k == STEPS[kind, w, h, keyint], k
    assert min(k) < 0 < max(k) and (max(k) == fq_ref.MAX_STEP or keyint == 3)
    assert min(want["frame_q"]) <= BASE < max(want["frame_q"])
    assert len({0 if q <= 20 else (1 if q <= 60 else (2 if q <= 120 else 3)) for q in want["frame_q"]}) >= 2


def check_stages(av1mi, ctx, kind, w, h, bd, n, keyints):
    import torch
    raw, searched = the_clip(kind, w, h, bd, n)
    R = range_of(bd)
    dev = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()
    assert av1mi.cq_to_qindex(30) == BASE
    for keyint in keyints:
        ana = tpl_ref.analysis(raw, w, h, bd, n, keyint, R, searched)
        for fq in (1, 2, 4):
            want = fq_ref.decision(ana, fq, BASE)
            p = av1mi.default_params(w, h, bd, keyint=keyint, me_range=R, frame_q_strength=fq)
            for where, got in (("host input", ctx.tpl_frame_q(p, raw, n)), ("device input", ctx.tpl_frame_q(p, dev.data_ptr(), n, on_device=True))):
                for stage in ("intra_sum", "dep_sum", "beta", "frame_q"):
                    assert [int(v) for v in got[stage]] == [int(v) for v in want[stage]], (keyint, fq, where, stage)
                assert got["mean_beta"] == want["mean_beta"], (keyint, fq, where)
            if fq == 4 and (kind, w, h, keyint) in STEPS:
                check_exercised(kind, w, h, keyint, want)
            for aq, tpl in ((0, 0), (4, 0), (0, 2), (4, 2)):
                ref = fq_ref.qindex_map(raw, w, h, bd, n, aq, tpl, fq, BASE, ana)
                p = av1mi.default_params(w, h, bd, keyint=keyint, me_range=R, frame_q_strength=fq, aq_strength=aq, tpl_strength=tpl)
                got = ctx.aq_qindex(p, raw, n)
                assert got.shape == ref.shape and np.array_equal(got, ref), (keyint, fq, aq, tpl, "host input")
                assert np.array_equal(ctx.aq_qindex(p, dev.data_ptr(), n, on_device=True), ref), (keyint, fq, aq, tpl, "device input")
                if (aq, tpl) == (0, 0):
                    assert all((ref[f] == want["frame_q"][f]).all() for f in range(n))


@pytest.mark.parametrize("kind", ["pattern", "half"])
@pytest.mark.parametrize("w,h,bd,n", SIZES)
def test_stages_and_map_equal_the_rule(av1mi, ctx, w, h, bd, n, kind):
    check_stages(av1mi, ctx, kind, w, h, bd, n, (1, 3, 240))


def test_stages_on_the_static_clip(av1mi, ctx):
    check_stages(av1mi, ctx, "static", 136, 72, 8, 5, (240,))


def test_frame_q_is_refused_without_the_strength(av1mi, ctx):
    raw, _ = the_clip("pattern", 200, 120, 8, 5)
    with pytest.raises(av1mi.EncodeFailed) as e:
        ctx.tpl_frame_q(av1mi.default_params(200, 120, 8, keyint=240, tpl_strength=2), raw, 5)
    assert e.value.code == 1   # AV1MI_E_INVALID_ARG


# ---------------------------------------------------------------- (b) whole temporal units against the oracle
def oracle_chunk(oracle, case, frames, frame_q, lf_levels=None):
    """the chunk as the oracle codes it frame by frame at the frames' own indices, as edge_content.oracle_encode chains it;
    lf_levels: the deblocking levels per frame, which stay with the chunk's index (the oracle's own formula would follow q_f)"""
    keyint = case["params"].get("keyint", 1)
    tus, recs, ref, prev = [], [], None, None
    for t, f in enumerate(frames):
        key = t % keyint == 0
        cfg = edge_content.oracle_config(oracle, case, t)
        cfg.base_q_idx = int(frame_q[t])
        if lf_levels is not None:
            cfg.deblock = 2
            for k in range(4):
                cfg.lf_level[k] = int(lf_levels[t][k])
        tu, rec, _ = oracle.encode_frame(cfg, f, with_seq_hdr=key, ref=None if key else ref, prev_src=None if key else prev)
        tus.append(tu)
        recs.append(rec)
        ref, prev = rec, f
    return tus, recs


UNITS = [
    # kind, w, h, bd, frames, parameters
    ("pattern", 200, 120, 8, 5, dict(keyint=240)),
    ("static", 136, 72, 8, 5, dict(keyint=240, subpel=1, me_presearch=1)),
    ("half", 328, 248, 10, 6, dict(keyint=3, me_range=16, block_log2=6)),
    ("pattern", 202, 122, 8, 5, dict(keyint=240, cdf_update=0)),
    ("pattern", 264, 200, 8, 4, dict(keyint=3, tile_sb=2)),
    ("pattern", 200, 120, 8, 5, dict(keyint=240, enable_qm=1, qm_min=1)),   # (oracle_config derives the level from the chunk's CQ: what stays)
    ("pattern", 200, 120, 8, 5, dict(keyint=240, deblock=1, enable_lr=2)),
    ("static", 136, 72, 8, 5, dict(keyint=240, cq_level=1)),               # the one-sided clamps
    ("static", 136, 72, 8, 5, dict(keyint=240, cq_level=63)),
]


@pytest.mark.parametrize("kind,w,h,bd,n,extra", UNITS)
def test_temporal_units_equal_the_oracle(av1mi, oracle, ctx, kind, w, h, bd, n, extra):
    """fq_strength = 4 alone: every temporal unit's bytes and every plane of the reconstruction"""
    if (kind, w, h, bd, n) == ("pattern", 264, 200, 8, 4):
        raw = tf_ref.pattern_clip(w, h, bd, n, seed=7)[0]
    else:
        raw = the_clip(kind, w, h, bd, n)[0]
    frames = split_frames(raw, w, h, bd, n)
    params = dict(partition_search=0, cq_level=30, me_range=range_of(bd))
    params.update(extra)
    cq = params.pop("cq_level")
    base = av1mi.cq_to_qindex(cq)
    p = av1mi.default_params(w, h, bd, cq_level=cq, frame_q_strength=4, **params)
    data, sizes, _, rec = ctx.encode_chunk(p, raw, n, want_recon=True)
    rec = split_frames(rec.tobytes(), w, h, bd, n)
    frame_q, beta = ctx.frame_q_result(n)
    lf_on, _ = ctx.lf_search_result(n)
    decided = ctx.tpl_frame_q(p, raw, n)
    assert np.array_equal(frame_q, decided["frame_q"]) and np.array_equal(beta, decided["beta"])
    k = [(int(q) - base) // 4 for q in frame_q]
    if cq == 1:
        assert min(k) == 0 < max(k)
    elif cq == 63:
        assert min(k) < 0 == max(k)
    else:
        assert min(k) < 0 < max(k), k
    lf = None
    if params.get("deblock"):
        ctx.encode_chunk(av1mi.default_params(w, h, bd, cq_level=cq, **params), raw, n)
        lf_off, _ = ctx.lf_search_result(n)
        assert np.array_equal(lf_on, lf_off)   # the levels stay with the chunk's index
        lf = lf_on
    case = dict(w=w, h=h, bd=bd, params=dict(params, cq_level=cq))
    tus, recs = oracle_chunk(oracle, case, frames, frame_q, lf)
    got = tus_of(data, sizes)
    for f in range(n):
        assert got[f] == tus[f], "temporal unit %d (q %d): %d bytes against the oracle's %d" % (f, frame_q[f], len(got[f]), len(tus[f]))
        for pl in range(3):
            assert np.array_equal(rec[f][pl], np.asarray(recs[f][pl]).astype(np.int64)), "frame %d plane %d" % (f, pl)


# ---------------------------------------------------------------- (c) a key frame per superblock with all three terms
@pytest.mark.parametrize("w,h,bd", [(200, 120, 8), (328, 248, 10)])
def test_key_frame_equals_the_oracle_per_superblock(av1mi, oracle, ctx, w, h, bd):
    """frame 0 of a three-frame P chunk with fq = 4, tpl = 4, aq = 2: with tiles of one superblock and the loop filters off a key
    frame's superblock depends on its own source and index only, and the oracle takes base_q_idx directly"""
    n, R = 3, range_of(bd)
    raw = the_clip("half", w, h, bd, 6 if bd == 10 else 5)[0][:n * w * h * 3 // 2 * (2 if bd > 8 else 1)]
    frames = split_frames(raw, w, h, bd, n)
    params = dict(tile_sb=1, enable_cdef=0, deblock=0, enable_lr=0, partition_search=0, keyint=240, cq_level=30, me_range=R)
    strengths = dict(frame_q_strength=4, tpl_strength=4, aq_strength=2)
    ana = tpl_ref.analysis(raw, w, h, bd, n, 240, R)
    qmap = ctx.aq_qindex(av1mi.default_params(w, h, bd, **strengths, **params), raw, n)
    assert np.array_equal(qmap, fq_ref.qindex_map(raw, w, h, bd, n, 2, 4, 4, BASE, ana))
    _, _, _, rec = encode(ctx, av1mi, raw, w, h, bd, n, **strengths, **params)
    q0 = int(ctx.frame_q_result(n)[0][0])
    assert q0 == fq_ref.decision(ana, 4, BASE)["frame_q"][0] and q0 < BASE
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
    (200, 136, 8, 5, dict(frame_q_strength=4, keyint=240, subpel=1, me_presearch=1)),
    (328, 248, 10, 5, dict(frame_q_strength=4, tpl_strength=2, aq_strength=2, keyint=3, me_range=16)),
    (264, 200, 8, 4, dict(frame_q_strength=4, tile_sb=2, keyint=3)),
    (200, 136, 8, 4, dict(frame_q_strength=3, tpl_strength=3, keyint=240, deblock=2, enable_lr=4, cdef_search=2)),
    (200, 136, 8, 4, dict(frame_q_strength=4, keyint=240, tf_frames=3, tf_strength=2)),
    (328, 248, 8, 4, dict(frame_q_strength=4, tpl_strength=4, keyint=3, partition_search=2, min_block_log2=3)),
]


@pytest.mark.parametrize("w,h,bd,n,extra", DECODE)
def test_dav1d_decodes_to_the_reconstruction(av1mi, w, h, bd, n, extra):
    import oracle_avif
    if not oracle_avif.have_libavif():
        pytest.skip("libavif (dav1d) is not available on this machine")
    raw = tf_ref.pattern_clip(w, h, bd, n, seed=7)[0]
    with av1mi.Context(0) as c:
        data, sizes, rep, want = encode(c, av1mi, raw, w, h, bd, n, **extra)
        frame_q = c.frame_q_result(n)[0]
        p = av1mi.default_params(w, h, bd, **extra)
        src = raw
        if extra.get("tf_frames"):   # the encoder codes, and reports against, the filtered key frames
            src = c.temporal_filter(p, raw, n, want_mv=False)[0].tobytes()
        assert np.array_equal(frame_q, c.tpl_frame_q(p, src, n)["frame_q"])
    assert len(set(int(q) for q in frame_q)) >= 2, "the content moves no frame off the base index"
    frames = split_frames(src, w, h, bd, n)
    got = edge_content.dav1d_decode(tus_of(data, sizes), w, h, bd, extra["keyint"])
    assert len(got) == n
    tot = [0, 0, 0]
    for f in range(n):
        for pl in range(3):
            assert np.array_equal(np.asarray(got[f][pl]).astype(np.int64), want[f][pl]), "frame %d plane %d" % (f, pl)
            tot[pl] += int(((want[f][pl] - frames[f][pl]) ** 2).sum())
    assert [int(x) for x in rep.sse] == tot


# ---------------------------------------------------------------- (e) properties
def test_no_dependency_leaves_the_chunk_as_it_is(av1mi, ctx):
    """all key frames, a one-frame chunk and independent noise (betaF <= 1): every k_f = 0, and with fq_strength alone the bytes are
    those of the chunk without it"""
    cases = [("pattern", 200, 120, 8, 5, 5, dict(keyint=1)), ("pattern", 200, 120, 8, 5, 1, dict(keyint=240)), ("noise", 128, 80, 8, 5, 5, dict(keyint=240))]
    for kind, w, h, bd, n_clip, n, kw in cases:
        raw = the_clip(kind, w, h, bd, n_clip)[0][:n * w * h * 3 // 2]
        p = av1mi.default_params(w, h, bd, frame_q_strength=4, **kw)
        got = ctx.tpl_frame_q(p, raw, n)
        assert got["beta"].max() <= 1 and (got["frame_q"] == BASE).all(), (kind, n)
        assert (ctx.aq_qindex(p, raw, n) == BASE).all()
        d1, s1, _, r1 = encode(ctx, av1mi, raw, w, h, bd, n, frame_q_strength=4, **kw)
        assert (ctx.frame_q_result(n)[0] == BASE).all()
        d0, s0, _, r0 = encode(ctx, av1mi, raw, w, h, bd, n, **kw)
        assert d1 == d0 and s1 == s0 and same_frames(r0, r1), (kind, n)
        q, beta = ctx.frame_q_result(n)   # a chunk without the term: the chunk's index and zeros
        assert (q == BASE).all() and (beta == 0).all()
    with pytest.raises(av1mi.EncodeFailed):
        ctx.frame_q_result(n + 1)


def test_static_clip_rises_frame_by_frame(av1mi, ctx):
    """inside a key-frame interval of a static clip q_f does not fall from frame to frame: every frame is needed by more frames than
    the next"""
    w, h, bd, n = 136, 72, 8, 5
    raw, _ = the_clip("static", w, h, bd, n)
    for keyint, s in ((240, 4), (240, 1), (3, 4)):
        q = [int(v) for v in ctx.tpl_frame_q(av1mi.default_params(w, h, bd, keyint=keyint, frame_q_strength=s), raw, n)["frame_q"]]
        for f in range(n - 1):
            if (f + 1) % keyint:
                assert q[f] <= q[f + 1], (keyint, s, q)
    assert q[0] < q[2] and q[3] < q[4]


# ---------------------------------------------------------------- (f) reuse and determinism
def test_workspace_reuse_and_determinism(av1mi):
    """one context alternates the term on and off at two sizes, two runs each: bytes identical per configuration, the off runs a fresh
    context's"""
    clips = [(200, 120, 8, 5), (136, 72, 8, 5)]
    runs = [dict(frame_q_strength=s, keyint=240, subpel=1) for s in (0, 4, 0, 2)] + [dict(frame_q_strength=4, tpl_strength=2, aq_strength=3, keyint=3, deblock=1),
                                                                                     dict(frame_q_strength=0, keyint=3, deblock=1)]
    seen = {}
    with av1mi.Context(0) as c:
        for kw in runs:
            for w, h, bd, n in clips:
                raw, _ = the_clip("pattern" if w == 200 else "static", w, h, bd, n)
                d, s, _, r = encode(c, av1mi, raw, w, h, bd, n, **kw)
                d2, s2, _, r2 = encode(c, av1mi, raw, w, h, bd, n, **kw)
                assert d == d2 and s == s2 and same_frames(r, r2), kw
                key = (w, tuple(sorted(kw.items())))
                assert seen.setdefault(key, d) == d, kw
                if kw["frame_q_strength"] == 0:
                    plain = {k: v for k, v in kw.items() if k != "frame_q_strength"}
                    with av1mi.Context(0) as fresh:
                        d0, s0, _, r0 = encode(fresh, av1mi, raw, w, h, bd, n, cq_level=30, **plain)
                    assert d == d0 and s == s0 and same_frames(r, r0), kw
    on = seen[200, tuple(sorted(dict(frame_q_strength=4, keyint=240, subpel=1).items()))]
    off = seen[200, tuple(sorted(dict(frame_q_strength=0, keyint=240, subpel=1).items()))]
    assert on != off
