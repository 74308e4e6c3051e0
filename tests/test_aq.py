"""GPU tests of the activity-adaptive quantisation (include/av1mi.h: cq_level bits 8-10, av1mi_aq_qindex).

The decision is restated with tests/aq_ref.py.  The reconstruction has an exact reference without a new oracle: with tiles of one
superblock and the loop filters off, a key frame's superblock depends only on its own source and quantiser index, and the oracle takes
base_q_idx directly - one oracle run per distinct index of the map gives every superblock's Y, U and V.  dav1d (libavif) pins the syntax:
it decodes the streams to the reconstruction in every plane."""
import os
import sys

import numpy as np
import pytest

import aq_ref
import edge_content
from test_lr_chroma import clip, raw_of, split_frames

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def encode(ctx, av1mi, frames, w, h, bd, **kw):
    p = av1mi.default_params(w, h, bd, **kw)
    data, sizes, rep, rec = ctx.encode_chunk(p, raw_of(frames, bd), len(frames), want_recon=True)
    return data, sizes, rep, split_frames(rec.tobytes(), w, h, bd, len(frames))


def same_frames(a, b):
    return all(np.array_equal(x, y) for fa, fb in zip(a, b) for x, y in zip(fa, fb))


@pytest.fixture(scope="module")
def ctx(av1mi):
    c = av1mi.Context(0)
    yield c
    c.close()


_clips = {}


def the_clip(oracle, w, h, bd, n=3):
    """the content of every test here: tests/test_lr_chroma.py's clip (noise, left half smoothed strongly, top right quarter lightly)"""
    key = (w, h, bd)
    if key not in _clips or len(_clips[key]) < n:
        _clips[key] = clip(oracle, w, h, bd, n, seed=40 + w)
    return _clips[key][:n]


# ---------------------------------------------------------------- 1. the map
MAP_SIZES = [(8, 8, 8), (72, 56, 8), (136, 72, 8), (200, 120, 8), (202, 122, 8), (328, 248, 10)]


@pytest.mark.parametrize("w,h,bd", MAP_SIZES)
def test_map_equals_the_rule(av1mi, oracle, ctx, w, h, bd):
    import torch
    n = 3
    frames = the_clip(oracle, w, h, bd, n)
    raw = raw_of(frames, bd)
    dev = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()
    E = [aq_ref.sb_energy(f[0], bd) for f in frames]
    for cq in (1, 30, 63):
        base = av1mi.cq_to_qindex(cq)
        for s in (0, 1, 2, 4):
            want = np.stack([aq_ref.qindex_of(e, s, base) for e in E])
            p = av1mi.default_params(w, h, bd, cq_level=cq, aq_strength=s)
            got = ctx.aq_qindex(p, raw, n)
            assert got.shape == want.shape and np.array_equal(got, want), (cq, s, "host input")
            got = ctx.aq_qindex(p, dev.data_ptr(), n, on_device=True)
            assert np.array_equal(got, want), (cq, s, "device input")
            if s == 0:
                assert (want == base).all()
            if (cq, s) == (30, 4) and (w, h) in ((200, 120), (328, 248)):
                # the content must exercise the rule: several indices, finer and coarser than the base
                assert len(set(want.ravel())) >= 4 and want.min() < base < want.max(), sorted(set(want.ravel()))


# ---------------------------------------------------------------- 2. key frames against one oracle run per index
KEY_CASES = [
    (200, 120, 8, dict(block_log2=3)),
    (200, 120, 8, dict(block_log2=5)),
    (328, 248, 10, dict(block_log2=6)),
    (136, 72, 8, dict(intra_mode_mask=0x1FFF, intra_angle_delta=1, intra_edge_filter=1, cfl=1, tx_search=1)),
    (200, 120, 8, dict(enable_qm=1, qm_min=1)),
    (202, 122, 8, dict()),
]


@pytest.mark.parametrize("w,h,bd,extra", KEY_CASES)
def test_key_frames_equal_the_oracle_per_superblock(av1mi, oracle, ctx, w, h, bd, extra):
    n = 2
    frames = the_clip(oracle, w, h, bd, n)
    params = dict(extra, tile_sb=1, enable_cdef=0, deblock=0, enable_lr=0, partition_search=0, keyint=1, cq_level=30)
    p = av1mi.default_params(w, h, bd, aq_strength=4, **params)
    qmap = ctx.aq_qindex(p, raw_of(frames, bd), n)
    _, _, _, rec = encode(ctx, av1mi, frames, w, h, bd, aq_strength=4, **params)
    case = dict(w=w, h=h, bd=bd, params=params)
    for f in range(n):
        assert len(set(qmap[f].ravel())) >= 2
        for q in sorted(set(int(v) for v in qmap[f].ravel())):
            cfg = edge_content.oracle_config(oracle, case, f)   # (the quantiser-matrix level is that of the base index)
            cfg.base_q_idx = q
            _, want, _ = oracle.encode_frame(cfg, frames[f])
            for r, c in zip(*np.nonzero(qmap[f] == q)):
                for pl in range(3):
                    k = 64 if pl == 0 else 32
                    a = rec[f][pl][k * r:k * r + k, k * c:k * c + k]
                    b = np.asarray(want[pl]).astype(np.int64)[k * r:k * r + k, k * c:k * c + k]
                    assert np.array_equal(a, b), "frame %d superblock (%d, %d) index %d plane %d" % (f, r, c, q, pl)


# ---------------------------------------------------------------- 3. dav1d decodes to the reconstruction
def half_constant(frames, bd, const_w):
    """the clip with the columns left of luma column const_w at mid grey in every plane: whole 64x64 blocks that are skipped"""
    out = []
    for fr in frames:
        g = []
        for pl, p in enumerate(fr):
            p = p.copy()
            p[:, :const_w >> (1 if pl else 0)] = 1 << (bd - 1)
            g.append(p)
        out.append(g)
    return out


DECODE = [
    # w, h, bd, frames, parameters, AV1MI_ENTROPY_GROUP, constant columns
    (200, 120, 8, 3, dict(aq_strength=4), None, 0),
    (328, 248, 10, 3, dict(aq_strength=2, block_log2=6), None, 0),
    (328, 248, 10, 5, dict(aq_strength=4, keyint=3, subpel=1, me_presearch=1), None, 0),
    (200, 136, 8, 4, dict(aq_strength=4, keyint=240, subpel=1, me_presearch=1), None, 0),
    (328, 248, 10, 3, dict(aq_strength=4, deblock=1, enable_lr=4, cdef_search=2), None, 0),
    (200, 136, 8, 4, dict(aq_strength=3, keyint=240, deblock=1, enable_lr=4, cdef_search=2, enable_qm=1, qm_min=1), None, 0),
    (328, 248, 8, 4, dict(aq_strength=4, keyint=3, partition_search=1, min_block_log2=3), None, 0),
    (200, 120, 8, 3, dict(aq_strength=4, cdf_update=0, keyint=2), None, 0),
    (264, 200, 10, 4, dict(aq_strength=4, tile_sb=2, keyint=3), None, 0),
    (264, 200, 8, 3, dict(aq_strength=4, block_log2=6, tile_sb=1, keyint=2), None, 132),
    (264, 200, 8, 3, dict(aq_strength=4, block_log2=6, tile_sb=2, keyint=2), None, 132),
    (264, 200, 8, 3, dict(aq_strength=4, block_log2=6, tile_sb=2, keyint=2), None, 192),   # a tile of skipped, then coded superblocks
    (200, 120, 8, 3, dict(aq_strength=4, cq_level=1, keyint=2), None, 0),
    (200, 120, 8, 3, dict(aq_strength=4, cq_level=63, keyint=2), None, 0),
    (256, 192, 8, 5, dict(aq_strength=4, keyint=240, subpel=1), "2", 0),
]


@pytest.mark.parametrize("w,h,bd,n,extra,group,const_w", DECODE)
def test_dav1d_decodes_to_the_reconstruction(av1mi, oracle, monkeypatch, w, h, bd, n, extra, group, const_w):
    import oracle_avif
    if not oracle_avif.have_libavif():
        pytest.skip("libavif (dav1d) is not available on this machine")
    if group is not None:
        monkeypatch.setenv("AV1MI_ENTROPY_GROUP", group)
    frames = the_clip(oracle, w, h, bd, n)
    if const_w:
        frames = half_constant(frames, bd, const_w)
    keyint = extra.get("keyint", 1)
    with av1mi.Context(0) as c:
        data, sizes, rep, want = encode(c, av1mi, frames, w, h, bd, **extra)
        p = av1mi.default_params(w, h, bd, **extra)
        qmap = c.aq_qindex(p, raw_of(frames, bd), n)
    base = av1mi.cq_to_qindex(extra.get("cq_level", 30))
    assert len(set(qmap.ravel())) >= 2, "the content moves no superblock off the base index"
    if base == 4:
        assert qmap.min() == base and qmap.max() > base
    if base == 255:
        assert qmap.max() == base and qmap.min() < base
    tus, off = [], 0
    for s in sizes:
        tus.append(data[off:off + s])
        off += s
    got = edge_content.dav1d_decode(tus, w, h, bd, keyint)
    assert len(got) == n
    tot = [0, 0, 0]
    for f in range(n):
        for pl in range(3):
            assert np.array_equal(np.asarray(got[f][pl]).astype(np.int64), want[f][pl]), "frame %d plane %d" % (f, pl)
            tot[pl] += int(((want[f][pl] - frames[f][pl]) ** 2).sum())
    assert [int(x) for x in rep.sse] == tot


# ---------------------------------------------------------------- 4. a map that is all base
def test_uniform_map_changes_the_stream_only(av1mi, oracle, ctx):
    """every superblock of a frame holds the same 64x64 pattern: E = M everywhere, all deltas 0 - the reconstruction is the strength-0
    run's, the stream is not (three header bits, a delta_q_abs of 0 per superblock)"""
    w, h, bd, n = 192, 128, 8, 4
    frames = []
    for t in range(n):
        pat = oracle.synthclip_frame(64, 64, bd, seed=9, t=t)
        frames.append([np.tile(np.asarray(p).astype(np.int64), (2, 3)) for p in pat])
    kw = dict(keyint=3, subpel=1, deblock=1)
    p = av1mi.default_params(w, h, bd, aq_strength=4, **kw)
    assert (ctx.aq_qindex(p, raw_of(frames, bd), n) == av1mi.cq_to_qindex(30)).all()
    d0, s0, _, r0 = encode(ctx, av1mi, frames, w, h, bd, aq_strength=0, **kw)
    for s in (1, 4):
        d1, s1, _, r1 = encode(ctx, av1mi, frames, w, h, bd, aq_strength=s, **kw)
        assert same_frames(r0, r1)
        assert d1 != d0


# ---------------------------------------------------------------- 5. reuse and determinism
def test_workspace_reuse_and_determinism(av1mi, oracle):
    w, h, bd = 264, 200, 10
    frames = the_clip(oracle, w, h, bd, 3)
    runs = [dict(aq_strength=s) for s in (0, 4, 0, 2, 1)] + [dict(aq_strength=s, enable_qm=1, qm_min=1) for s in (0, 3, 0)]
    runs.append(dict(aq_strength=2, keyint=3, subpel=1, deblock=1))
    with av1mi.Context(0) as c:
        for kw in runs:
            d, s, _, r = encode(c, av1mi, frames, w, h, bd, **kw)
            d2, s2, _, r2 = encode(c, av1mi, frames, w, h, bd, **kw)
            assert d == d2 and s == s2 and same_frames(r, r2), kw
            with av1mi.Context(0) as fresh:
                d0, s0, _, r0 = encode(fresh, av1mi, frames, w, h, bd, **kw)
            assert d == d0 and s == s0 and same_frames(r, r0), kw
            if kw["aq_strength"] == 0:   # the packed field with strength 0 is the plain CQ value
                plain = {k: v for k, v in kw.items() if k != "aq_strength"}
                dp, sp, _, rp = encode(c, av1mi, frames, w, h, bd, cq_level=30, **plain)
                assert d == dp and s == sp and same_frames(r, rp), kw
