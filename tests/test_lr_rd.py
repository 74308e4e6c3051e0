"""GPU tests of the rate term of the restoration unit decisions (include/av1mi.h: AV1MI_LR_RD, enable_lr bits 14 and 15; DESIGN.md §3
item 9g), by the method of tests/test_lr_fit.py: a key frame's reconstruction before CDEF does not depend on CDEF or restoration and its
CDEF output not on restoration, so a run with both off gives the pre-CDEF planes, a run with enable_lr = 0 the CDEF planes, and the
restated rule (tests/lr_rd_ref.py) applied to them must give the mode's planes, the choices, their bits and lambda bit for bit.  dav1d
(libavif) decodes the streams to the reconstruction.  tests/test_lr_rd_content.py asserts on the CPU, with the same restatement on the
oracle's planes, that the cases make the rule act: units that go off, that keep a filter, that move to another one."""
import numpy as np
import pytest

import lr_rd_ref as ref
import lr_unit_ref as uref
import test_lr_fit as base

pytestmark = pytest.mark.gpu

FIT4, FIT4_SET9, W = 0x104, (1 << 9 << 16) | 0x104, 0x400
LOW = (1, 2, 3, 4, FIT4, FIT4_SET9, 3 | W, FIT4 | W)
SCALES = (0, 1)
KEY_CASES = [
    # w, h, bd, extra, lr_unit_shift, the clip's seed (tests/test_lr_fit.py's 40 + w, or one at which a fixed Wiener filter survives)
    (88, 72, 10, dict(deblock=1), 0, 7),                    # one unit
    (200, 120, 8, {}, 0, 240),                              # six units
    (202, 122, 8, dict(tile_sb=2, cq_level=45), 0, 242),    # a tile carries its reference over four units: Lc is an estimate
    (328, 248, 10, {}, 1, 368),
    (264, 200, 8, {}, 1, 4),                                # superblock row 4 reads no unit
    (520, 392, 8, {}, 2, 560),
]
RUNS = [(ci, low) for ci in range(len(KEY_CASES)) for low in LOW]   # (the whole product: a run is tens of milliseconds)


def case_frames(oracle, ci, n=2):
    w, h, bd = KEY_CASES[ci][:3]
    return base.clip(oracle, w, h, bd, n, seed=KEY_CASES[ci][5])


def case_lambda(ci, s):
    w, h, bd, extra = KEY_CASES[ci][:4]
    return ref.lam(ref.qindex_of_cq(extra.get("cq_level", 30)), bd, s)


@pytest.fixture(scope="module")
def ctx(av1mi):
    c = av1mi.Context(0)
    yield c
    c.close()
    uref.forget()
    _planes.clear()
    _cands.clear()


_planes, _cands = {}, {}


def case_planes(ctx, av1mi, oracle, ci):
    """a case's frames with their pre-CDEF and CDEF planes, computed once"""
    if ci not in _planes:
        w, h, bd, extra = KEY_CASES[ci][:4]
        frames = case_frames(oracle, ci)
        pre = base.encode(ctx, av1mi, frames, w, h, bd, **dict(extra, enable_cdef=0, enable_lr=0))[3]
        cdef = base.encode(ctx, av1mi, frames, w, h, bd, **dict(extra, enable_lr=0))[3]
        _planes[ci] = (frames, pre, cdef)
    return _planes[ci]


def case_candidates(ctx, av1mi, oracle, ci, f, pl):
    """every candidate of a plane's units at the case's unit size - both fits, every set - computed once; a mode sees its own (ref.view)"""
    if (ci, f, pl) not in _cands:
        bd, shift = KEY_CASES[ci][2], KEY_CASES[ci][4]
        frames, pre, cdef = case_planes(ctx, av1mi, oracle, ci)
        _cands[(ci, f, pl)] = ref.candidates(pre[f][pl], cdef[f][pl], frames[f][pl], bd, int(pl > 0), shift << 12 | FIT4 | W)
    return _cands[(ci, f, pl)]


def run(ctx, av1mi, oracle, ci, v):
    w, h, bd, extra = KEY_CASES[ci][:4]
    frames = case_planes(ctx, av1mi, oracle, ci)[0]
    data, sizes, _, got = base.encode(ctx, av1mi, frames, w, h, bd, enable_lr=v, **extra)
    return data, sizes, got, ctx.lr_rd_result(len(frames))


@pytest.mark.parametrize("ci,low", RUNS, ids=["%dx%d-%d-%#x" % (KEY_CASES[ci][:3] + (low,)) for ci, low in RUNS])
def test_key_frames_restated(av1mi, oracle, ctx, ci, low):
    """planes, choices, bits and lambda of two key frames are the restated rule's at both scales - and with the mode off, where the rule
    at lambda 0 is the error's own order; per unit J of the mode's choice is at most J of the choice with the mode off; dav1d decodes
    the mode's streams to the reconstruction"""
    import oracle_avif
    w, h, bd, extra, shift = KEY_CASES[ci][:5]
    frames, pre, cdef = case_planes(ctx, av1mi, oracle, ci)
    base_v = shift << 12 | low
    nr, nc = uref.grid(w, h, shift)
    bad, streams = [], []
    off_choice = None
    for s in (None,) + SCALES:
        v = base_v if s is None else base_v | ref.rd_field(s)
        lam = 0 if s is None else case_lambda(ci, s)
        data, sizes, got, (choice, bits16, got_lam) = run(ctx, av1mi, oracle, ci, v)
        assert choice.shape == (len(frames), 3, nr, nc) and int(av1mi._lib.av1mi_lr_rd_units(ctx._h)) == nr * nc
        assert got_lam == lam, (hex(v), got_lam, lam)
        if s is None:
            off_choice = choice
        else:
            streams.append((data, sizes, got))
        for f in range(len(frames)):
            for pl in range(3):
                tag = "%dx%d %s lr %#x frame %d plane %d" % (w, h, extra, v, f, pl)
                if pl and (low & 0xFF) in (1, 2):
                    if not np.array_equal(got[f][pl], cdef[f][pl]) or choice[f, pl].any() or bits16[f, pl].any():
                        bad.append(tag + ": a plane that is not restored")
                    continue
                cands = ref.view(case_candidates(ctx, av1mi, oracle, ci, f, pl), base_v)
                want, wc, wb, wj = ref.restore_rd(cands, lam)
                print(tag, "lambda", lam, "choices", wc.ravel().tolist(), "bits16", wb.ravel().tolist())
                if not np.array_equal(choice[f, pl].astype(np.int64), wc):
                    bad.append(tag + ": choices %s" % choice[f, pl].ravel().tolist())
                if not np.array_equal(bits16[f, pl].astype(np.int64), wb):
                    bad.append(tag + ": bits16 %s" % bits16[f, pl].ravel().tolist())
                if not np.array_equal(got[f][pl], want):
                    bad.append(tag + ": samples")
                if s is not None:
                    for i in range(nr):
                        for j in range(nc):
                            if wj[i][j] > ref.cost_of(cands, i, j, int(off_choice[f, pl, i, j]), lam):
                                bad.append(tag + ": J of unit (%d, %d) above that of the choice with the mode off" % (i, j))
    assert not bad, bad
    if not oracle_avif.have_libavif():
        pytest.skip("libavif (dav1d) is not available on this machine: the streams' syntax is not pinned")
    for data, sizes, got in streams:
        base._assert_decodes(base._decode(oracle_avif, data, sizes, w, h, bd, len(frames), 1), got, len(frames))


def test_mode_acts_on_the_cases(av1mi, oracle, ctx):
    """on the product's own planes, across the 64x64 cases at both scales: a unit goes off that the error alone filters, a unit keeps a
    filter, a unit moves to another filter"""
    seen = dict(off=0, kept=0, moved=0)
    for ci in (1, 2):
        for s in SCALES:
            for f in range(2):
                c = ref.view(case_candidates(ctx, av1mi, oracle, ci, f, 0), FIT4)
                a, b = ref.restore_rd(c, 0)[1], ref.restore_rd(c, case_lambda(ci, s))[1]
                seen["off"] += int(((a != 0) & (b == 0)).sum())
                seen["kept"] += int(((a != 0) & (b != 0)).sum())
                seen["moved"] += int(((a != 0) & (b != 0) & (b != a)).sum())
    print(seen)
    assert all(seen.values()), seen


def test_deterministic_and_differs_from_the_mode_off(av1mi, oracle, ctx):
    """with s fixed two runs give identical bytes; the mode changes the bytes of a case whose units it switches off"""
    for low in (4, FIT4 | W):
        for s in SCALES:
            a, b = run(ctx, av1mi, oracle, 1, low | ref.rd_field(s)), run(ctx, av1mi, oracle, 1, low | ref.rd_field(s))
            assert a[0] == b[0] and a[1] == b[1] and np.array_equal(a[3][0], b[3][0]) and np.array_equal(a[3][1], b[3][1])
            assert a[0] != run(ctx, av1mi, oracle, 1, low)[0]


def test_mode_alternates_between_chunks(av1mi, oracle):
    """one context through the mode on and off, scales, fits and unit sizes; every chunk's bytes, planes and result are a fresh context's"""
    w, h, bd = 264, 200, 10
    frames = base.clip(oracle, w, h, bd, 3, seed=7)
    rd = ref.rd_field
    runs = [dict(enable_lr=0x504 | rd(0)), dict(enable_lr=0x504), dict(enable_lr=0x1003 | rd(1)), dict(enable_lr=3), dict(enable_lr=0x104 | rd(3), keyint=3),
            dict(enable_lr=0x104, keyint=3), dict(enable_lr=2 | rd(2)), dict(enable_lr=0), dict(enable_lr=0x2403 | rd(0))]
    with av1mi.Context(0) as c:
        for kw in runs:
            d, s, _, r = base.encode(c, av1mi, frames, w, h, bd, **kw)
            res = c.lr_rd_result(len(frames))
            with av1mi.Context(0) as fresh:
                d0, s0, _, r0 = base.encode(fresh, av1mi, frames, w, h, bd, **kw)
                res0 = fresh.lr_rd_result(len(frames))
            assert d == d0 and s == s0, kw
            assert all(np.array_equal(a, b) for fa, fb in zip(r, r0) for a, b in zip(fa, fb)), kw
            assert np.array_equal(res[0], res0[0]) and np.array_equal(res[1], res0[1]) and res[2] == res0[2], kw
            assert (res[2] != 0) == ((kw["enable_lr"] & 0xC000) == 0xC000), kw
            if kw["enable_lr"] == 0:
                assert not res[0].any() and not res[1].any()
            with pytest.raises(av1mi.EncodeFailed):   # another frame count is not the last chunk's
                c.lr_rd_result(len(frames) + 1)


DECODE = [
    # w, h, bd, frames, extra, AV1MI_ENTROPY_GROUP
    (328, 248, 10, 5, dict(enable_lr=0x504 | ref.rd_field(0), keyint=3, subpel=1, deblock=1), None),
    (200, 136, 8, 5, dict(enable_lr=0x104 | ref.rd_field(1), keyint=240), "2"),
    (328, 200, 8, 2, dict(enable_lr=0x1504 | ref.rd_field(0), cdef_search=4), None),
    (328, 200, 8, 2, dict(enable_lr=0x403 | ref.rd_field(1), aq_strength=2), None),
]


@pytest.mark.parametrize("w,h,bd,n,extra,group", DECODE)
def test_dav1d_decodes_to_the_reconstruction(av1mi, oracle, monkeypatch, w, h, bd, n, extra, group):
    """IPPP chunks (keyint 3 with sub-sample vectors, keyint 240 in entropy groups of 2), the CDEF search, adaptive quantisation - lambda
    stays with base_q_idx - with the mode on"""
    import oracle_avif
    if not oracle_avif.have_libavif():
        pytest.skip("libavif (dav1d) is not available on this machine")
    if group is not None:
        monkeypatch.setenv("AV1MI_ENTROPY_GROUP", group)
    frames = base.clip(oracle, w, h, bd, n, seed=60 + w)
    with av1mi.Context(0) as c:
        data, sizes, rep, want = base.encode(c, av1mi, frames, w, h, bd, **extra)
        choice, bits16, lam = c.lr_rd_result(n)
    assert lam == ref.lam(120, bd, ref.rd_scale_of(extra["enable_lr"]))
    assert choice.shape[:2] == (n, 3) and (bits16[:, 0] > 0).all()   # every luma unit codes at least its type
    base._assert_decodes(base._decode(oracle_avif, data, sizes, w, h, bd, n, extra.get("keyint", 1)), want, n)


@pytest.mark.parametrize("v", [1, 0x2403, 0x504])
@pytest.mark.parametrize("s", [0, 1, 2, 3])
def test_mode_values_encode(av1mi, oracle, ctx, v, s):
    """enable_lr with bits 14 and 15 encodes at every scale (the library before the feature returns AV1MI_E_INVALID_ARG), and lambda is
    the restated one"""
    w, h, bd = 200, 136, 8
    frames = base.clip(oracle, w, h, bd, 1, seed=3)
    data = base.encode(ctx, av1mi, frames, w, h, bd, enable_lr=v | ref.rd_field(s))[0]
    assert data and ctx.lr_rd_result(1)[2] == ref.lam(120, bd, s)


@pytest.mark.parametrize("v", [0x204, 0x1204, 0x802, 0x1802, 0x1902, 0x5001, 0x9002, 0x4001, 0x8001, 0xC000, 0xC005, 0xF001, 0xC101])
def test_refused_values(av1mi, oracle, ctx, v):
    """bits 9, 11, 14 or 15 without both of 14 and 15, the mode with a low byte of 0 or above 4, with no unit size, with a fit its low byte
    does not take"""
    w, h, bd = 200, 136, 8
    frames = base.clip(oracle, w, h, bd, 1, seed=3)
    with pytest.raises(av1mi.EncodeFailed) as e:
        base.encode(ctx, av1mi, frames, w, h, bd, enable_lr=v)
    assert e.value.code == 1   # AV1MI_E_INVALID_ARG
