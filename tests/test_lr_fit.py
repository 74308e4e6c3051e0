"""GPU tests of the self-guided restoration fit (include/av1mi.h: AV1MI_LR_FIT).

The fit is restated with tests/sgr_fit_ref.py: a key frame's reconstruction before CDEF does not depend on CDEF or restoration and its
CDEF output not on restoration, so a run with both off gives the pre-CDEF planes, a run with enable_lr = 0 the CDEF planes, and the
rule applied to them must give the fit run's planes, unit records and error table bit for bit.  dav1d (libavif) decodes the streams to
the reconstruction in every plane."""
import os
import sys

import numpy as np
import pytest

import lr_ref
import sgr_fit_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _smooth(p, k):
    h, w = p.shape
    c = np.pad(np.pad(p, k, mode="edge").cumsum(0).cumsum(1), ((1, 0), (1, 0)))
    n = 2 * k + 1
    return (c[n:n + h, n:n + w] - c[:h, n:n + w] - c[n:n + h, :w] + c[:h, :w] + n * n // 2) // (n * n)


def clip(oracle, w, h, bd, n, seed):
    """tests/test_lr_chroma.py's recipe: synthclip frames (white noise) with the left half smoothed strongly and the top right quarter
    lightly, so that units choose off, Wiener and self-guided filters"""
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


def apply_records(pre, cdef, bd, sub, rec):
    """the plane the numpy filters give for a plane's unit records"""
    pre, cdef = np.asarray(pre, dtype=np.int64), np.asarray(cdef, dtype=np.int64)
    rows, cols = lr_ref.unit_bounds(cdef.shape[0], cdef.shape[1], sub)
    cands, memo, out = lr_ref.candidates(sub, True), {}, np.empty_like(cdef)
    for i, (y0, y1) in enumerate(rows):
        for j, (x0, x1) in enumerate(cols):
            k, t, w0, w1 = (int(v) for v in rec[i, j])
            key = (k,) if k < 4 else ("s", t, w0, w1)
            if key not in memo:
                memo[key] = lr_ref.filtered(pre, cdef, bd, sub, cands[k]) if k < 4 else ref.filtered_set(pre, cdef, bd, sub, t, w0, w1)
            out[y0:y1, x0:x1] = memo[key][y0:y1, x0:x1]
    return out


def check_restated(ctx, av1mi, frames, w, h, bd, extra, lr, mask, stats):
    """one fit run against the restatement: planes, records, errors; returns the run's (data, sizes, planes, records)"""
    pre = encode(ctx, av1mi, frames, w, h, bd, **dict(extra, enable_cdef=0, enable_lr=0, cdef_search=0))[3]
    cdef = encode(ctx, av1mi, frames, w, h, bd, **dict(extra, enable_lr=0))[3]
    data, sizes, _, got = encode(ctx, av1mi, frames, w, h, bd, enable_lr=av1mi.lr_fit_field(lr, mask), **extra)
    units, err = ctx.lr_fit_result(len(frames))
    for f in range(len(frames)):
        for pl in range(3):
            tag = "%dx%d %s lr %d mask %#x frame %d plane %d" % (w, h, extra, lr, mask, f, pl)
            if pl and lr == 2:
                assert np.array_equal(got[f][pl], cdef[f][pl]), tag
                assert not units[f, pl].any() and not err[f, pl].any(), tag
                continue
            want, rec, e = ref.restore_fit(pre[f][pl], cdef[f][pl], frames[f][pl], bd, int(pl > 0), mask)
            print(tag, "choices", sorted(int(c) for c in rec[..., 0].ravel()))
            assert np.array_equal(units[f, pl].astype(np.int64), rec), tag
            assert np.array_equal(err[f, pl], e), tag
            assert np.array_equal(got[f][pl], want), tag
            assert np.array_equal(got[f][pl], apply_records(pre[f][pl], cdef[f][pl], bd, int(pl > 0), units[f, pl])), tag
            for k, t, w0, w1 in rec.reshape(-1, 4):
                stats["units"] += 1
                stats["wiener"] += 1 <= k <= 3
                if k >= 7:
                    r0, _, r1, _ = ref.SGR_PARAMS[t]
                    stats["fitted"] += 1
                    stats["sets"].add(int(t))
                    stats["inside"] += bool(r0 and r1 and -96 < w0 < 31 and -32 < w1 < 95)
                    stats["clamped1"] += bool(r0 and r1 and w1 in (-32, 95))
    return data, sizes, got, units


def new_stats():
    return dict(units=0, wiener=0, fitted=0, sets=set(), inside=0, clamped1=0)


KEY_CASES = [
    # w, h, bd, extra
    (88, 72, 10, dict(deblock=1)),                        # one unit, 88 columns: the second column pass
    (200, 120, 8, {}),
    (202, 122, 8, dict(block_log2=4, cq_level=45)),       # base_q_idx 180; signalled != coded size
    (328, 248, 10, dict(block_log2=6, deblock=1)),        # 103-row last units
    (648, 360, 8, dict(tile_sb=2)),                       # the reference carried across a tile's four units
]


def test_key_frames_restated(av1mi, oracle, ctx):
    """test 1: Y (0x102) and Y, U, V (0x104) of two key frames are the restated rule's, with records and errors; across the cases the
    fit wins at least half of the units, with 5 sets or more, a set with r0 = 0, weights strictly inside, a clamped xqd1 (the refit ran)
    and a Wiener unit"""
    st = new_stats()
    for w, h, bd, extra in KEY_CASES:
        frames = clip(oracle, w, h, bd, 2, seed=40 + w)
        for lr in (2, 4):
            check_restated(ctx, av1mi, frames, w, h, bd, extra, lr, 0, st)
    print(st)
    assert 2 * st["fitted"] >= st["units"], st
    assert len(st["sets"]) >= 5 and st["sets"] & {10, 11, 12, 13}, st
    assert st["inside"] >= 1 and st["clamped1"] >= 1 and st["wiener"] >= 1, st


def _decode(oracle_avif, data, sizes, w, h, bd, n, keyint):
    tus, off = [], 0
    for s in sizes:
        tus.append(data[off:off + s])
        off += s
    if keyint == 1:
        return [oracle_avif.decode_obus(t, w, h, bd) for t in tus]
    keys = [i + 1 for i in range(n) if i % keyint == 0]
    return oracle_avif.decode_sequence(oracle_avif.wrap_avis(tus, w, h, bd, sync=keys), w, h)


def _assert_decodes(got, want, n):
    assert len(got) == n
    for f in range(n):
        for pl in range(3):
            assert np.array_equal(np.asarray(got[f][pl]).astype(np.int64), want[f][pl]), "frame %d plane %d" % (f, pl)


@pytest.mark.parametrize("w,h,bd", [(200, 120, 8), (328, 248, 10)])
@pytest.mark.parametrize("mask", [0x3C00, 0xC000, 1 << 9])
def test_forced_pools(av1mi, oracle, ctx, w, h, bd, mask):
    """test 2: pools with r0 = 0 only, r1 = 0 only and set 9 alone, restated and decoded by dav1d; every fitted choice is in the pool,
    and with r1 = 0 some unit takes set 14 or 15 - the path of the uncoded xqd1"""
    import oracle_avif
    frames = clip(oracle, w, h, bd, 2, seed=50 + w)
    st = new_stats()
    data, sizes, got, units = check_restated(ctx, av1mi, frames, w, h, bd, {}, 4, mask, st)
    assert st["sets"] and all((mask >> t) & 1 for t in st["sets"]), st
    if mask == 0xC000:
        assert st["sets"] & {14, 15}, st
    if not oracle_avif.have_libavif():
        pytest.skip("libavif (dav1d) is not available on this machine")
    _assert_decodes(_decode(oracle_avif, data, sizes, w, h, bd, 2, 1), got, 2)


DECODE = [
    # w, h, bd, frames, extra, AV1MI_ENTROPY_GROUP
    (200, 120, 8, 2, dict(enable_lr=0x102), None),
    (328, 248, 10, 2, dict(enable_lr=0x104), None),
    (328, 248, 10, 5, dict(enable_lr=0x104, keyint=3, subpel=1, deblock=1), None),
    (200, 136, 8, 5, dict(enable_lr=0x104, keyint=240), None),
    (256, 192, 8, 6, dict(enable_lr=0x104, keyint=240, subpel=1), "2"),
    (202, 122, 8, 2, dict(enable_lr=0x104, tile_sb=2), None),
    (328, 200, 8, 2, dict(enable_lr=0x104, cdef_search=4, cq_level=45), None),
    (328, 200, 8, 2, dict(enable_lr=0x102, aq_strength=2), None),
    (1920, 1080, 10, 2, dict(enable_lr=0x104), None),
]


@pytest.mark.parametrize("w,h,bd,n,extra,group", DECODE)
def test_dav1d_decodes_to_the_reconstruction(av1mi, oracle, monkeypatch, w, h, bd, n, extra, group):
    """test 3: key chunks, IPPP chunks (keyint 3 / 240, entropy groups of 2), tiles of 2x2 superblocks, the CDEF search, adaptive
    quantisation, 1080p"""
    import oracle_avif
    if not oracle_avif.have_libavif():
        pytest.skip("libavif (dav1d) is not available on this machine")
    if group is not None:
        monkeypatch.setenv("AV1MI_ENTROPY_GROUP", group)
    frames = clip(oracle, w, h, bd, n, seed=60 + w)
    with av1mi.Context(0) as c:
        data, sizes, rep, want = encode(c, av1mi, frames, w, h, bd, **extra)
    _assert_decodes(_decode(oracle_avif, data, sizes, w, h, bd, n, extra.get("keyint", 1)), want, n)


@pytest.mark.parametrize("w,h,bd", [(328, 248, 10), (648, 360, 8)])
def test_monotonic_report_and_determinism(av1mi, oracle, ctx, w, h, bd):
    """test 4: on key frames no unit's SSE in a restored plane exceeds the 2 / 4 run's; report.sse is numpy's; err[choice] is the unit's
    SSE; two runs give the same bytes"""
    n = 2
    frames = clip(oracle, w, h, bd, n, seed=90 + w)
    for lr in (2, 4):
        base = encode(ctx, av1mi, frames, w, h, bd, enable_lr=lr)[3]
        d1, s1, rep, got = encode(ctx, av1mi, frames, w, h, bd, enable_lr=av1mi.lr_fit_field(lr))
        units, err = ctx.lr_fit_result(n)
        d2, s2, _, got2 = encode(ctx, av1mi, frames, w, h, bd, enable_lr=av1mi.lr_fit_field(lr))
        assert d1 == d2 and s1 == s2
        assert all(np.array_equal(a, b) for fa, fb in zip(got, got2) for a, b in zip(fa, fb))
        tot, tot_base = [0, 0, 0], [0, 0, 0]
        for f in range(n):
            for pl in range(3):
                tot[pl] += int(((got[f][pl] - frames[f][pl]) ** 2).sum())
                tot_base[pl] += int(((base[f][pl] - frames[f][pl]) ** 2).sum())
            for pl in range(3 if lr == 4 else 1):
                rows, cols = lr_ref.unit_bounds(h >> (pl > 0), w >> (pl > 0), int(pl > 0))
                for i, (y0, y1) in enumerate(rows):
                    for j, (x0, x1) in enumerate(cols):
                        e = lambda r: int(((r[f][pl][y0:y1, x0:x1] - frames[f][pl][y0:y1, x0:x1]) ** 2).sum())
                        assert e(got) <= e(base), "lr %d frame %d plane %d unit (%d, %d)" % (lr, f, pl, i, j)
                        assert int(err[f, pl, i, j, int(units[f, pl, i, j, 0])]) == e(got)
        assert [int(x) for x in rep.sse] == tot
        assert all(a <= b for a, b in zip(tot, tot_base))


def test_workspace_reuse(av1mi, oracle):
    """test 5: one context at one geometry through enable_lr 2 -> 0x102 -> 4 -> 0x104 -> 1 -> 0x104 (IPPP); every output equals a
    fresh context's, and the fit's result after a chunk without the fit is all zero"""
    w, h, bd = 264, 200, 10
    frames = clip(oracle, w, h, bd, 4, seed=7)
    runs = [dict(enable_lr=2), dict(enable_lr=0x102), dict(enable_lr=4), dict(enable_lr=0x104), dict(enable_lr=1),
            dict(enable_lr=0x104, keyint=3)]
    with av1mi.Context(0) as c:
        for kw in runs:
            d, s, _, r = encode(c, av1mi, frames, w, h, bd, **kw)
            units, err = c.lr_fit_result(len(frames))
            with av1mi.Context(0) as fresh:
                d0, s0, _, r0 = encode(fresh, av1mi, frames, w, h, bd, **kw)
                units0, err0 = fresh.lr_fit_result(len(frames))
            assert d == d0 and s == s0, kw
            assert all(np.array_equal(a, b) for fa, fb in zip(r, r0) for a, b in zip(fa, fb)), kw
            assert np.array_equal(units, units0) and np.array_equal(err, err0), kw
            with pytest.raises(av1mi.EncodeFailed):   # another frame size's unit grid is not the library's count: refused, nothing copied
                c.lr_fit_result(len(frames), 640, 360)
            if kw["enable_lr"] & 0x100:
                assert units[:, 0, :, :, 0].any() or err[:, 0].any(), kw
            else:
                assert not units.any() and not err.any(), kw


def test_p_chunk_luma_unchanged(av1mi, oracle, ctx):
    """test 6: in a P chunk with CDEF off every frame's Y under 0x104 is that under 0x102 (DESIGN.md §3 item 9c's invariant: the block
    decisions are luma's and the luma reference is the same)"""
    w, h, bd = 200, 136, 8
    frames = clip(oracle, w, h, bd, 5, seed=80 + w)
    base = encode(ctx, av1mi, frames, w, h, bd, enable_lr=0x102, keyint=240, enable_cdef=0)[3]
    got = encode(ctx, av1mi, frames, w, h, bd, enable_lr=0x104, keyint=240, enable_cdef=0)[3]
    for f in range(len(frames)):
        assert np.array_equal(got[f][0], base[f][0]), "frame %d" % f
