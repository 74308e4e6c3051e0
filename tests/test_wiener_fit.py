"""GPU tests of the Wiener restoration fit (include/av1mi.h: AV1MI_LR_WIENER_FIT), by tests/test_lr_fit.py's
method: a key frame's reconstruction before CDEF does not depend on CDEF or restoration and its CDEF output not on restoration, so a
run with both off gives the pre-CDEF planes, a run with enable_lr = 0 the CDEF planes, and tests/wiener_fit_ref.py applied to them
must give the fit run's planes, unit records and errors bit for bit.  dav1d (libavif) decodes the streams to the reconstruction in
every plane, which pins the pass order and the syntax.

Content.  tests/test_lr_fit.py's clip with the bottom right quarter smoothed along rows only (a 5-tap mean), so that the vertical and
the horizontal taps must differ.  The conditions test_content_conditions asserts were first checked without a GPU, with the
restatement on the oracle's planes at the same parameters (two key frames of each of the five cases); of the units of the restored
planes there
  0x401: 186 units, 172 choose 23;   0x402: 186 units, 127;   0x403: 558 units, 531 (>= one third);   0x504: 558 units, 166 (>= one tenth)
and across the four values 996 units choose 23: cv != ch in 971 of them, the refit ran in 840, no tap sits at a clamp in 124, 479 are
chroma units, and 3 tiles of the 648x360 case (tiles of 2x2 superblocks) hold a fixed Wiener filter beside a fitted one."""
import hashlib

import numpy as np
import pytest

import lr_ref
import test_lr_fit as base
import wiener_fit_ref as ref

pytestmark = pytest.mark.gpu

WFIT = 0x400
VALUES = (0x401, 0x403, 0x402, 0x504)
KEY_CASES = [
    # w, h, bd, extra
    (88, 72, 10, dict(deblock=1)),                        # one unit, 88 columns: the second column pass
    (200, 120, 8, {}),
    (202, 122, 8, dict(block_log2=4, cq_level=45)),       # signalled != coded size
    (328, 248, 10, dict(block_log2=6, deblock=1)),        # 103-row last units
    (648, 360, 8, dict(tile_sb=2)),                       # the reference carried across a tile's four units
]


def _rows5(p):
    q = np.pad(p, ((0, 0), (2, 2)), mode="edge")
    return (sum(q[:, t:t + p.shape[1]] for t in range(5)) + 2) // 5


def clip(oracle, w, h, bd, n, seed):
    """tests/test_lr_fit.py's recipe (left half smoothed strongly, top right quarter lightly) plus the bottom right quarter smoothed
    along rows only"""
    frames = []
    for t in range(n):
        fr = []
        for p in oracle.synthclip_frame(w, h, bd, seed=seed, t=t):
            p = p.astype(np.int64)
            q = p.copy()
            ph, pw = p.shape
            q[:, :pw // 2] = base._smooth(p, 3)[:, :pw // 2]
            q[:ph // 2, pw // 2:] = base._smooth(p, 1)[:ph // 2, pw // 2:]
            q[ph // 2:, pw // 2:] = _rows5(p)[ph // 2:, pw // 2:]
            fr.append(q)
        frames.append(fr)
    return frames


@pytest.fixture(scope="module")
def ctx(av1mi):
    c = av1mi.Context(0)
    yield c
    c.close()


_planes, _runs = {}, {}


def case_planes(ctx, av1mi, oracle, ci):
    """a case's frames with their pre-CDEF and CDEF planes, computed once"""
    if ci not in _planes:
        w, h, bd, extra = KEY_CASES[ci]
        frames = clip(oracle, w, h, bd, 2, seed=40 + w)
        pre = base.encode(ctx, av1mi, frames, w, h, bd, **dict(extra, enable_cdef=0, enable_lr=0, cdef_search=0))[3]
        cdef = base.encode(ctx, av1mi, frames, w, h, bd, **dict(extra, enable_lr=0))[3]
        _planes[ci] = (frames, pre, cdef)
    return _planes[ci]


def run_case(ctx, av1mi, oracle, ci, v):
    """one fit run against the restatement; returns (failures, stats), computed once per (case, value)"""
    if (ci, v) in _runs:
        return _runs[(ci, v)]
    w, h, bd, extra = KEY_CASES[ci]
    tsb = extra.get("tile_sb", 1)
    frames, pre, cdef = case_planes(ctx, av1mi, oracle, ci)
    _, _, _, got = base.encode(ctx, av1mi, frames, w, h, bd, enable_lr=v, **extra)
    units, err = ctx.lr_wiener_fit_result(len(frames))
    bad, st = [], dict(units=0, win=0, differ=0, refit=0, free=0, chroma=0, mixed=0)
    for f in range(len(frames)):
        for pl in range(3):
            tag = "%dx%d %s lr %#x frame %d plane %d" % (w, h, extra, v, f, pl)
            if pl and (v & 0xFF) in (1, 2):
                if not np.array_equal(got[f][pl], cdef[f][pl]) or units[f, pl].any() or err[f, pl].any():
                    bad.append(tag + ": a plane that is not restored")
                continue
            sub = int(pl > 0)
            b, bch = ref.base_decision(pre[f][pl], cdef[f][pl], frames[f][pl], bd, sub, v & ~WFIT)
            infos = []
            want, rec, e = ref.restore_wiener_fit(pre[f][pl], cdef[f][pl], frames[f][pl], bd, sub, b, bch, infos)
            print(tag, "choices", sorted(int(c) for c in rec[..., 0].ravel()))
            if not np.array_equal(units[f, pl].astype(np.int64), rec):
                bad.append(tag + ": records %s, restated %s" % (units[f, pl].reshape(-1, 8)[:4].tolist(), rec.reshape(-1, 8)[:4].tolist()))
            if not np.array_equal(err[f, pl], e):
                bad.append(tag + ": errors")
            if not np.array_equal(got[f][pl], want):
                bad.append(tag + ": samples")
            info = {(i, j): d for i, j, d in infos}
            nr, nc = rec.shape[:2]
            for i in range(nr):
                for j in range(nc):
                    st["units"] += 1
                    if rec[i, j, 0] != ref.CHOICE:
                        continue
                    cv, ch = list(rec[i, j, 2:5]), list(rec[i, j, 5:8])
                    st["win"] += 1
                    st["differ"] += cv != ch
                    st["refit"] += info[(i, j)]["v"]["refit"] or info[(i, j)]["h"]["refit"]
                    st["free"] += all(ref.TAPS_MIN[k] < t[k] < ref.TAPS_MAX[k] for t in (cv, ch) for k in range(sub, 3))
                    st["chroma"] += sub
            for ti in range(0, nr, tsb):
                for tj in range(0, nc, tsb):
                    tile = [int(rec[i, j, 0]) for i in range(ti, min(ti + tsb, nr)) for j in range(tj, min(tj + tsb, nc))]
                    st["mixed"] += ref.CHOICE in tile and any(1 <= c <= 3 for c in tile)
    _runs[(ci, v)] = (bad, st)
    return bad, st


@pytest.mark.parametrize("v", VALUES)
@pytest.mark.parametrize("ci", range(len(KEY_CASES)))
def test_key_frames_restated(av1mi, oracle, ctx, ci, v):
    """the planes, the records and the errors of two key frames are the restated rule's"""
    bad, st = run_case(ctx, av1mi, oracle, ci, v)
    print(st)
    assert not bad, bad


def test_content_conditions(av1mi, oracle, ctx):
    """across the cases: under 0x504 candidate 23 wins at least one tenth of the units, under 0x403 at least one third; some unit has
    cv != ch, in one the refit ran, one has no tap at a clamp, a chroma unit chooses 23, and a tile holds a fixed Wiener filter beside a
    fitted one (the carried reference)"""
    tot = {v: dict(units=0, win=0, differ=0, refit=0, free=0, chroma=0, mixed=0) for v in VALUES}
    for ci in range(len(KEY_CASES)):
        for v in VALUES:
            for k, n in run_case(ctx, av1mi, oracle, ci, v)[1].items():
                tot[v][k] += int(n)
    print({hex(v): s for v, s in tot.items()})
    assert 10 * tot[0x504]["win"] >= tot[0x504]["units"], tot[0x504]
    assert 3 * tot[0x403]["win"] >= tot[0x403]["units"], tot[0x403]
    for k in ("differ", "refit", "free", "chroma", "mixed"):
        assert sum(s[k] for s in tot.values()) >= 1, (k, tot)


DECODE = [
    # w, h, bd, frames, extra, AV1MI_ENTROPY_GROUP
    (200, 120, 8, 2, dict(enable_lr=0x403), None),
    (328, 248, 10, 2, dict(enable_lr=0x504), None),
    (328, 248, 10, 5, dict(enable_lr=0x504, keyint=3, subpel=1, deblock=1), None),
    (200, 136, 8, 5, dict(enable_lr=0x403, keyint=240), None),
    (256, 192, 8, 6, dict(enable_lr=0x504, keyint=240, subpel=1), "2"),
    (202, 122, 8, 2, dict(enable_lr=0x403, tile_sb=2), None),
    (648, 360, 8, 2, dict(enable_lr=0x504, tile_sb=2), None),
    (328, 200, 8, 2, dict(enable_lr=0x504, cdef_search=4, cq_level=45), None),
    (328, 200, 8, 2, dict(enable_lr=0x402, aq_strength=2), None),
    (1920, 1080, 10, 2, dict(enable_lr=0x504), None),
]


@pytest.mark.parametrize("w,h,bd,n,extra,group", DECODE)
def test_dav1d_decodes_to_the_reconstruction(av1mi, oracle, monkeypatch, w, h, bd, n, extra, group):
    """key chunks at 0x403 and 0x504, IPPP chunks (keyint 3 / 240, sub-sample vectors, entropy groups of 2), tiles of 2x2 superblocks,
    the CDEF search, adaptive quantisation, 1080p"""
    import oracle_avif
    if not oracle_avif.have_libavif():
        pytest.skip("libavif (dav1d) is not available on this machine")
    if group is not None:
        monkeypatch.setenv("AV1MI_ENTROPY_GROUP", group)
    frames = clip(oracle, w, h, bd, n, seed=60 + w)
    with av1mi.Context(0) as c:
        data, sizes, rep, want = base.encode(c, av1mi, frames, w, h, bd, **extra)
        units, _ = c.lr_wiener_fit_result(n)
    assert (units[..., 0] == ref.CHOICE).any()   # the stream holds fitted units
    base._assert_decodes(base._decode(oracle_avif, data, sizes, w, h, bd, n, extra.get("keyint", 1)), want, n)


@pytest.mark.parametrize("lr", [1, 2, 3, 4])
def test_monotonic_report_and_determinism(av1mi, oracle, ctx, lr):
    """on key frames no unit's SSE exceeds its SSE under the same enable_lr without bit 10; err is numpy's SSE of the fitted output;
    report.sse is numpy's; two runs give the same bytes"""
    w, h, bd, n = 328, 248, 10, 2
    frames = clip(oracle, w, h, bd, n, seed=90 + w)
    plain = base.encode(ctx, av1mi, frames, w, h, bd, enable_lr=lr)[3]
    pre = base.encode(ctx, av1mi, frames, w, h, bd, enable_cdef=0, enable_lr=0)[3]
    cdef = base.encode(ctx, av1mi, frames, w, h, bd, enable_lr=0)[3]
    d1, s1, rep, got = base.encode(ctx, av1mi, frames, w, h, bd, enable_lr=lr | WFIT)
    units, err = ctx.lr_wiener_fit_result(n)
    d2, s2, _, got2 = base.encode(ctx, av1mi, frames, w, h, bd, enable_lr=lr | WFIT)
    assert d1 == d2 and s1 == s2
    assert all(np.array_equal(a, b) for fa, fb in zip(got, got2) for a, b in zip(fa, fb))
    tot = [0, 0, 0]
    for f in range(n):
        for pl in range(3):
            tot[pl] += int(((got[f][pl] - frames[f][pl]) ** 2).sum())
        for pl in range(3 if lr >= 3 else 1):
            sub = int(pl > 0)
            rows, cols = lr_ref.unit_bounds(h >> sub, w >> sub, sub)
            for i, (y0, y1) in enumerate(rows):
                for j, (x0, x1) in enumerate(cols):
                    sl = (slice(y0, y1), slice(x0, x1))
                    e = lambda r: int(((r[sl] - frames[f][pl][sl]) ** 2).sum())
                    u = [int(x) for x in units[f, pl, i, j]]
                    assert e(got[f][pl]) <= e(plain[f][pl]), "lr %d frame %d plane %d unit (%d, %d)" % (lr, f, pl, i, j)
                    if u[1]:
                        fitted = ref.filtered2(pre[f][pl], cdef[f][pl], bd, sub, u[2:5], u[5:8])
                        assert int(err[f, pl, i, j]) == e(fitted)
                        assert (u[0] == ref.CHOICE) == (e(fitted) < e(plain[f][pl]))
                    else:
                        assert int(err[f, pl, i, j]) == ref.ABSENT and u[0] != ref.CHOICE
    assert [int(x) for x in rep.sse] == tot


def test_workspace_reuse(av1mi, oracle):
    """one context at one geometry through enable_lr 4 -> 0x404 -> 0x104 -> 0x504 -> 1 -> 0x401 (IPPP); every output equals a fresh
    context's, and the Wiener fit's result after a chunk without bit 10 is all zero"""
    w, h, bd = 264, 200, 10
    frames = clip(oracle, w, h, bd, 4, seed=7)
    runs = [dict(enable_lr=4), dict(enable_lr=0x404), dict(enable_lr=0x104), dict(enable_lr=0x504), dict(enable_lr=1),
            dict(enable_lr=0x401, keyint=3)]
    with av1mi.Context(0) as c:
        for kw in runs:
            d, s, _, r = base.encode(c, av1mi, frames, w, h, bd, **kw)
            units, err = c.lr_wiener_fit_result(len(frames))
            sg_units, sg_err = c.lr_fit_result(len(frames))
            with av1mi.Context(0) as fresh:
                d0, s0, _, r0 = base.encode(fresh, av1mi, frames, w, h, bd, **kw)
                units0, err0 = fresh.lr_wiener_fit_result(len(frames))
                sg_units0, sg_err0 = fresh.lr_fit_result(len(frames))
            assert d == d0 and s == s0, kw
            assert all(np.array_equal(a, b) for fa, fb in zip(r, r0) for a, b in zip(fa, fb)), kw
            assert np.array_equal(units, units0) and np.array_equal(err, err0), kw
            assert np.array_equal(sg_units, sg_units0) and np.array_equal(sg_err, sg_err0), kw
            with pytest.raises(av1mi.EncodeFailed):   # another frame size's unit grid is not the library's count: refused
                c.lr_wiener_fit_result(len(frames), 640, 360)
            if kw["enable_lr"] & WFIT:
                assert units[:, 0, :, :, 1].any() and err[:, 0].any(), kw
                assert sg_units[..., 0].max() <= 22   # av1mi_lr_fit_result keeps reporting the decision before the Wiener fit
            else:
                assert not units.any() and not err.any(), kw


# sha256 of the bitstream of the clip below under enable_lr without bit 10, recorded from a build of the commit before the Wiener fit
PARENT_BYTES = {
    0x1: "b4fa05461339f28ffc39748dbd5f49a3877625c996d3e833a734a7e7c7a6c42d",
    0x2: "b88809ea4fd264122f99bf1326ba5b49332cba0ba56c39e889cd488346483628",
    0x3: "c402a1cb4e867dfbe2156f3ed710eab3e09df427a86e96356c59beaffbfef54d",
    0x4: "973de334b7c0f5bccb890c0a091318f4020ffb03d354496f46555ab939517f2d",
    0x102: "b4a5ef9cb7029c85503b0237401f7f906530f1a0d8a4437eeca6454a05920cfc",
    0x104: "a38f0760481cfcde25f8d153814d9714e4f7a547cedb4271d78c987aff2170f0",
}


@pytest.mark.parametrize("lr", [1, 2, 3, 4, 0x102, 0x104])
def test_bit_10_off_is_unchanged(av1mi, oracle, ctx, lr):
    """without bit 10 the bytes are those of the commit before the feature"""
    w, h, bd = 328, 248, 10
    frames = clip(oracle, w, h, bd, 3, seed=123)
    data, sizes, _, _ = base.encode(ctx, av1mi, frames, w, h, bd, enable_lr=lr, keyint=2, deblock=1)
    digest = hashlib.sha256(data).hexdigest()
    print("enable_lr %#x: %s" % (lr, digest))
    assert digest == PARENT_BYTES[lr]
