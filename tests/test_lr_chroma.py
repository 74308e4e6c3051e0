"""GPU tests of loop restoration on the chroma planes (include/av1mi.h: enable_lr 3 / 4).

The decision is restated with tests/lr_ref.py: a key frame's reconstruction before CDEF does not depend on CDEF or restoration, and
with enable_lr 1 / 2 the chroma planes are the CDEF output, so a run with CDEF and restoration off gives the pre-CDEF chroma, the
enable_lr 1 / 2 run the CDEF chroma, and lr_ref's rule applied to them must give U and V of the 3 / 4 run bit for bit, while Y stays
that of the 1 / 2 run.  dav1d (libavif) decodes the streams to the reconstruction in every plane."""
import os
import sys

import numpy as np
import pytest

import lr_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _smooth(p, k):
    h, w = p.shape
    c = np.pad(np.pad(p, k, mode="edge").cumsum(0).cumsum(1), ((1, 0), (1, 0)))
    n = 2 * k + 1
    return (c[n:n + h, n:n + w] - c[:h, n:n + w] - c[n:n + h, :w] + c[:h, :w] + n * n // 2) // (n * n)


def clip(oracle, w, h, bd, n, seed):
    """synthclip frames (white noise) with the left half smoothed strongly and the top right quarter lightly, so that units choose
    off, Wiener and self-guided filters"""
    frames = []
    for t in range(n):
        fr = []
        for p in oracle.synthclip_frame(w, h, bd, seed=seed, t=t):
            p = p.astype(np.int64)
            q = p.copy()
            ph, pw = p.shape
            q[:, :pw // 2] = _smooth(p, 3)[:, :pw // 2]
            q[:ph // 2, pw // 2:] = _smooth(p, 1)[:ph // 2, pw // 2:]
            fr.append(q)
        frames.append(fr)
    return frames


def raw_of(frames, bd):
    dt = np.uint8 if bd == 8 else np.dtype("<u2")
    return b"".join(p.astype(dt).tobytes() for f in frames for p in f)


def split_frames(raw, w, h, bd, n):
    a = np.frombuffer(raw, dtype=np.uint8 if bd == 8 else np.dtype("<u2")).astype(np.int64)
    fs, cw, ch = w * h * 3 // 2, w // 2, h // 2
    return [[a[f * fs:f * fs + w * h].reshape(h, w), a[f * fs + w * h:f * fs + w * h + cw * ch].reshape(ch, cw),
             a[f * fs + w * h + cw * ch:(f + 1) * fs].reshape(ch, cw)] for f in range(n)]


def encode(ctx, av1mi, frames, w, h, bd, **kw):
    p = av1mi.default_params(w, h, bd, **kw)
    data, sizes, rep, rec = ctx.encode_chunk(p, raw_of(frames, bd), len(frames), want_recon=True)
    return data, sizes, rep, split_frames(rec.tobytes(), w, h, bd, len(frames))


@pytest.fixture(scope="module")
def ctx(av1mi):
    c = av1mi.Context(0)
    yield c
    c.close()


KEY_CASES = [
    # w, h, bd, extra
    (200, 120, 8, dict(block_log2=5)),
    (202, 122, 8, dict(block_log2=4, deblock=1)),
    (328, 248, 10, dict(block_log2=6, deblock=1, cq_level=40)),
    (328, 248, 10, dict(block_log2=5, cdef_search=2)),
    (648, 360, 8, dict(block_log2=5, tile_sb=2, deblock=1)),
]


def test_key_frames_restated(av1mi, oracle, ctx):
    """test 1: U and V of the 3 / 4 runs are lr_ref's rule on the pre-CDEF and CDEF chroma; Y is that of the 1 / 2 run; across the
    cases each chroma plane chooses off, a Wiener and (with 4) a self-guided candidate"""
    seen = {(pl, lr): set() for pl in (1, 2) for lr in (3, 4)}
    for w, h, bd, extra in KEY_CASES:
        frames = clip(oracle, w, h, bd, 2, seed=40 + w)
        pre_kw = dict(extra, enable_cdef=0, enable_lr=0, cdef_search=0)
        pre = encode(ctx, av1mi, frames, w, h, bd, **pre_kw)[3]
        for lo, hi in ((1, 3), (2, 4)):
            base = encode(ctx, av1mi, frames, w, h, bd, enable_lr=lo, **extra)[3]
            got = encode(ctx, av1mi, frames, w, h, bd, enable_lr=hi, **extra)[3]
            for f in range(len(frames)):
                assert np.array_equal(got[f][0], base[f][0]), "%dx%d enable_lr %d frame %d: Y" % (w, h, hi, f)
                for pl in (1, 2):
                    want, choice, _ = lr_ref.restore(pre[f][pl], base[f][pl], frames[f][pl], bd, 1, hi == 4)
                    assert np.array_equal(got[f][pl], want), "%dx%d %s enable_lr %d frame %d plane %d" % (w, h, extra, hi, f, pl)
                    seen[(pl, hi)].update(int(c) for c in choice.ravel())
    for (pl, lr), s in seen.items():
        assert 0 in s and s & {1, 2, 3}, "plane %d enable_lr %d chose %s" % (pl, lr, sorted(s))
        if lr == 4:
            assert s & {4, 5, 6}, "plane %d enable_lr 4 chose %s" % (pl, sorted(s))


DECODE = [
    # w, h, bd, frames, extra, AV1MI_ENTROPY_GROUP
    (200, 120, 8, 3, dict(enable_lr=3), None),
    (328, 248, 10, 3, dict(enable_lr=4, deblock=1), None),
    (328, 248, 10, 5, dict(enable_lr=4, keyint=3, subpel=1, deblock=1), None),
    (200, 136, 8, 5, dict(enable_lr=3, keyint=240, subpel=1, deblock=1), None),
    (256, 192, 8, 6, dict(enable_lr=4, keyint=240, subpel=1), "2"),
    (1920, 1080, 10, 2, dict(enable_lr=4, intra_mode_mask=0x1FFF), None),
    (3840, 2160, 10, 2, dict(enable_lr=4, keyint=2), None),
    (202, 122, 8, 2, dict(enable_lr=4, tile_sb=2), None),
    (328, 200, 8, 3, dict(enable_lr=4, cdef_search=4, cq_level=45), None),
]


@pytest.mark.parametrize("w,h,bd,n,extra,group", DECODE)
def test_dav1d_decodes_to_the_reconstruction(av1mi, oracle, monkeypatch, w, h, bd, n, extra, group):
    """test 2: key chunks, IPPP chunks (keyint 3 / 240, sub-sample vectors, deblocking, entropy groups of 2), 1080p, 4K key + P,
    tiles of 2x2 superblocks at a small size, the CDEF search"""
    import oracle_avif
    if not oracle_avif.have_libavif():
        pytest.skip("libavif (dav1d) is not available on this machine")
    if group is not None:
        monkeypatch.setenv("AV1MI_ENTROPY_GROUP", group)
    frames = clip(oracle, w, h, bd, n, seed=60 + w)
    keyint = extra.get("keyint", 1)
    with av1mi.Context(0) as c:
        data, sizes, rep, want = encode(c, av1mi, frames, w, h, bd, **extra)
    tus, off = [], 0
    for s in sizes:
        tus.append(data[off:off + s])
        off += s
    if keyint == 1:
        got = [oracle_avif.decode_obus(t, w, h, bd) for t in tus]
    else:
        keys = [i + 1 for i in range(n) if i % keyint == 0]
        got = oracle_avif.decode_sequence(oracle_avif.wrap_avis(tus, w, h, bd, sync=keys), w, h)
    assert len(got) == n
    for f in range(n):
        for pl in range(3):
            assert np.array_equal(np.asarray(got[f][pl]).astype(np.int64), want[f][pl]), "frame %d plane %d" % (f, pl)


@pytest.mark.parametrize("w,h,bd,extra", [(328, 248, 10, dict(keyint=3, subpel=1, deblock=1)), (200, 136, 8, dict(keyint=240))])
def test_p_chunk_luma_unchanged(av1mi, oracle, ctx, w, h, bd, extra):
    """test 3: in P chunks every frame's Y is that of the 1 / 2 run - the block decisions are luma's and the luma reference is the
    same.  With CDEF off: CDEF filters only 8x8 blocks that are not skipped, and a block's skip flag covers its chroma residual, which
    a restored chroma reference changes."""
    extra = dict(extra, enable_cdef=0)
    frames = clip(oracle, w, h, bd, 5, seed=80 + w)
    for lo, hi in ((1, 3), (2, 4)):
        base = encode(ctx, av1mi, frames, w, h, bd, enable_lr=lo, **extra)[3]
        got = encode(ctx, av1mi, frames, w, h, bd, enable_lr=hi, **extra)[3]
        for f in range(len(frames)):
            assert np.array_equal(got[f][0], base[f][0]), "enable_lr %d frame %d" % (hi, f)


@pytest.mark.parametrize("w,h,bd", [(328, 248, 10), (648, 360, 8)])
def test_unit_sse_report_and_determinism(av1mi, oracle, ctx, w, h, bd):
    """test 4: on key frames no chroma unit's SSE exceeds the 1 / 2 run's (off is a candidate); report.sse is numpy's SSE of the
    reconstruction; two runs give the same bytes"""
    n = 3
    frames = clip(oracle, w, h, bd, n, seed=90 + w)
    for lo, hi in ((1, 3), (2, 4)):
        base = encode(ctx, av1mi, frames, w, h, bd, enable_lr=lo)[3]
        d1, s1, rep, got = encode(ctx, av1mi, frames, w, h, bd, enable_lr=hi)
        d2, s2, _, got2 = encode(ctx, av1mi, frames, w, h, bd, enable_lr=hi)
        assert d1 == d2 and s1 == s2
        assert all(np.array_equal(a, b) for fa, fb in zip(got, got2) for a, b in zip(fa, fb))
        tot = [0, 0, 0]
        for f in range(n):
            for pl in range(3):
                tot[pl] += int(((got[f][pl] - frames[f][pl]) ** 2).sum())
            for pl in (1, 2):
                rows, cols = lr_ref.unit_bounds(h // 2, w // 2, 1)
                for y0, y1 in rows:
                    for x0, x1 in cols:
                        e = lambda r: int(((r[f][pl][y0:y1, x0:x1] - frames[f][pl][y0:y1, x0:x1]) ** 2).sum())
                        assert e(got) <= e(base), "enable_lr %d frame %d plane %d unit (%d, %d)" % (hi, f, pl, y0, x0)
        assert [int(x) for x in rep.sse] == tot


def test_workspace_reuse(av1mi, oracle):
    """test 5: one context at one geometry through enable_lr 1 -> 3 -> 1 -> 4 -> 2, then a key chunk and an IPPP chunk; every output
    equals a fresh context's"""
    w, h, bd = 264, 200, 10
    frames = clip(oracle, w, h, bd, 4, seed=7)
    runs = [dict(enable_lr=v) for v in (1, 3, 1, 4, 2)] + [dict(enable_lr=4), dict(enable_lr=3, keyint=3, subpel=1, deblock=1)]
    with av1mi.Context(0) as c:
        for kw in runs:
            d, s, _, r = encode(c, av1mi, frames, w, h, bd, **kw)
            with av1mi.Context(0) as fresh:
                d0, s0, _, r0 = encode(fresh, av1mi, frames, w, h, bd, **kw)
            assert d == d0 and s == s0, kw
            assert all(np.array_equal(a, b) for fa, fb in zip(r, r0) for a, b in zip(fa, fb)), kw
