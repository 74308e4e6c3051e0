"""GPU tests of restoration units of 128x128 and 256x256 luma samples (include/av1mi.h: AV1MI_LR_UNIT_128 / _256, enable_lr bits 12-13;
DESIGN.md §3 item 9f), by the method of tests/test_lr_fit.py and tests/test_wiener_fit.py: a key frame's reconstruction before CDEF does
not depend on CDEF or restoration and its CDEF output not on restoration, so a run with both off gives the pre-CDEF planes, a run with
enable_lr = 0 the CDEF planes, and the restatements at the unit size (tests/lr_unit_ref.py) applied to them must give the product's
planes, unit records and errors bit for bit.  dav1d (libavif) decodes every stream to the reconstruction, which pins lr_params and the
superblock a unit is read with.

Content.  tests/test_wiener_fit.py's clip - the left part smoothed strongly, the top right lightly, the bottom right along rows only -
with the point where the three regions meet as a parameter: the frame's centre, or for 520x392 luma (256, 248), so that units of 256
lie on either side of a region's edge.  tests/test_lr_unit_content.py asserts on the CPU, with the restatement on the oracle's planes,
what the cases are for."""
import hashlib

import numpy as np
import pytest

import lr_unit_ref as uref
import test_lr_fit as base
import test_wiener_fit as wbase

pytestmark = pytest.mark.gpu

LOW = (0x001, 0x003, 0x002, 0x504)   # or-ed with the unit size: 0x1001, 0x1003, 0x1002, 0x1504 and the same with 0x2...
KEY_CASES = [
    # w, h, bd, extra, where the regions meet (luma; None: the centre), shifts
    (328, 248, 10, dict(block_log2=6, deblock=1), None, (1, 2)),   # 2x3 units of 128, the last column one cell; one unit of 256 with the extended last cells
    (392, 264, 8, {}, None, (1, 2)),                               # 128: superblock row 4 reads no unit; 256: 1x2 units
    (202, 122, 8, dict(block_log2=4), None, (1, 2)),               # signalled != coded size; 128: 1x2 units
    (520, 392, 8, dict(deblock=1), (256, 248), (1, 2)),            # 256: 2x2 units, 128: 3x4 (deblocked: a luma unit of 256 takes the fitted Wiener filter)
    (520, 392, 10, {}, (256, 248), (1, 2)),
    (648, 360, 8, dict(tile_sb=2), None, (1, 2)),                  # a tile of 2x2 superblocks starts one unit per plane or none
    (88, 72, 10, {}, None, (2,)),                                  # one unit, smaller than U
]
RUNS = [(ci, s << 12 | low) for ci, c in enumerate(KEY_CASES) for s in c[5] for low in LOW]


def clip(oracle, w, h, bd, n, seed, meet=None):
    """tests/test_wiener_fit.py's recipe with the regions meeting at luma `meet` (None: every plane's centre, that recipe itself)"""
    frames = []
    for t in range(n):
        fr = []
        for pl, p in enumerate(oracle.synthclip_frame(w, h, bd, seed=seed, t=t)):
            p = p.astype(np.int64)
            q = p.copy()
            ph, pw = p.shape
            cx, cy = (pw // 2, ph // 2) if meet is None else (meet[0] >> (pl > 0), meet[1] >> (pl > 0))
            q[:, :cx] = base._smooth(p, 3)[:, :cx]
            q[:cy, cx:] = base._smooth(p, 1)[:cy, cx:]
            q[cy:, cx:] = wbase._rows5(p)[cy:, cx:]
            fr.append(q)
        frames.append(fr)
    return frames


def case_frames(oracle, ci, n=2):
    w, h, bd, extra, meet, _ = KEY_CASES[ci]
    return clip(oracle, w, h, bd, n, seed=40 + w, meet=meet)


@pytest.fixture(scope="module")
def ctx(av1mi):
    c = av1mi.Context(0)
    yield c
    c.close()
    uref.forget()


_planes, _runs = {}, {}


def case_planes(ctx, av1mi, oracle, ci):
    """a case's frames with their pre-CDEF and CDEF planes, computed once"""
    if ci not in _planes:
        w, h, bd, extra = KEY_CASES[ci][:4]
        frames = case_frames(oracle, ci)
        pre = base.encode(ctx, av1mi, frames, w, h, bd, **dict(extra, enable_cdef=0, enable_lr=0, cdef_search=0))[3]
        cdef = base.encode(ctx, av1mi, frames, w, h, bd, **dict(extra, enable_lr=0))[3]
        _planes[ci] = (frames, pre, cdef)
    return _planes[ci]


def product_run(ctx, av1mi, oracle, ci, v):
    """one product run of a case, once: (data, sizes, planes, (self-guided fit's units, errors), (Wiener fit's units, errors), unit counts)"""
    if (ci, v) not in _runs:
        w, h, bd, extra = KEY_CASES[ci][:4]
        frames = case_planes(ctx, av1mi, oracle, ci)[0]
        data, sizes, _, got = base.encode(ctx, av1mi, frames, w, h, bd, enable_lr=v, **extra)
        counts = (int(av1mi._lib.av1mi_lr_fit_units(ctx._h)), int(av1mi._lib.av1mi_lr_wiener_fit_units(ctx._h)))
        _runs[(ci, v)] = (data, sizes, got, ctx.lr_fit_result(len(frames)), ctx.lr_wiener_fit_result(len(frames)), counts)
    return _runs[(ci, v)]


def restated(ctx, av1mi, oracle, ci, v, f, pl):
    w, h, bd = KEY_CASES[ci][:3]
    frames, pre, cdef = case_planes(ctx, av1mi, oracle, ci)
    return uref.restore_value(pre[f][pl], cdef[f][pl], frames[f][pl], bd, int(pl > 0), v)


@pytest.mark.parametrize("ci,v", RUNS, ids=["%dx%d-%d-%#x" % (KEY_CASES[ci][:3] + (v,)) for ci, v in RUNS])
def test_key_frames_restated(av1mi, oracle, ctx, ci, v):
    """the planes, the unit records, the errors and the unit counts of two key frames are the restated rule's at the unit size, and
    dav1d decodes the stream to them"""
    import oracle_avif
    w, h, bd, extra = KEY_CASES[ci][:4]
    frames, pre, cdef = case_planes(ctx, av1mi, oracle, ci)
    data, sizes, got, (fu, fe), (wu, we), counts = product_run(ctx, av1mi, oracle, ci, v)
    nr, nc = uref.grid(w, h, uref.shift_of(v))
    assert counts == (nr * nc, nr * nc) and fu.shape[2:4] == (nr, nc) and wu.shape[2:4] == (nr, nc)
    bad = []
    for f in range(len(frames)):
        for pl in range(3):
            tag = "%dx%d %s lr %#x frame %d plane %d" % (w, h, extra, v, f, pl)
            if pl and (v & 0xFF) in (1, 2):
                if not np.array_equal(got[f][pl], cdef[f][pl]) or fu[f, pl].any() or wu[f, pl].any() or we[f, pl].any():
                    bad.append(tag + ": a plane that is not restored")
                continue
            r = restated(ctx, av1mi, oracle, ci, v, f, pl)
            print(tag, "choices", r["choice"].ravel().tolist())
            assert r["choice"].shape == (nr, nc)
            if not np.array_equal(got[f][pl], r["plane"]):
                bad.append(tag + ": samples")
            if r["fit"] is not None and not (np.array_equal(fu[f, pl].astype(np.int64), r["fit"][0]) and np.array_equal(fe[f, pl], r["fit"][1])):
                bad.append(tag + ": the self-guided fit's records or errors")
            if r["wfit"] is not None and not (np.array_equal(wu[f, pl].astype(np.int64), r["wfit"][0]) and np.array_equal(we[f, pl], r["wfit"][1])):
                bad.append(tag + ": the Wiener fit's records or errors")
            if r["fit"] is None and fu[f, pl].any() or r["wfit"] is None and wu[f, pl].any():
                bad.append(tag + ": records of a fit that did not run")
    assert not bad, bad
    if not oracle_avif.have_libavif():
        pytest.skip("libavif (dav1d) is not available on this machine: lr_params and read_lr are not pinned")
    base._assert_decodes(base._decode(oracle_avif, data, sizes, w, h, bd, len(frames), 1), got, len(frames))


@pytest.mark.parametrize("ci", [0, 3])
@pytest.mark.parametrize("low", LOW)
def test_larger_units_never_lower_a_planes_sse(av1mi, oracle, ctx, ci, low):
    """per key frame and plane the restored plane's SSE at shift 1 is >= that at shift 0, and shift 2 >= shift 1, for the same low byte
    and fit bits: a unit never does better than its parts decided on their own"""
    w, h, bd, extra = KEY_CASES[ci][:4]
    frames = case_planes(ctx, av1mi, oracle, ci)[0]
    sse = []
    for s in (0, 1, 2):
        got = base.encode(ctx, av1mi, frames, w, h, bd, enable_lr=s << 12 | low, **extra)[3] if s == 0 else product_run(ctx, av1mi, oracle, ci, s << 12 | low)[2]
        sse.append([[int(((got[f][pl] - frames[f][pl]) ** 2).sum()) for pl in range(3)] for f in range(len(frames))])
    print("%dx%d lr %#x SSE [shift][frame][plane]" % (w, h, low), sse)
    for f in range(len(frames)):
        for pl in range(3):
            assert sse[0][f][pl] <= sse[1][f][pl] <= sse[2][f][pl], (f, pl, sse)


DECODE = [
    # w, h, bd, frames, extra, where the regions meet
    (328, 248, 10, 5, dict(enable_lr=0x1504, keyint=3, subpel=1, deblock=1), None),
    (392, 264, 8, 5, dict(enable_lr=0x2504, keyint=240), None),
    (328, 200, 8, 2, dict(enable_lr=0x1504, cdef_search=4, cq_level=45), None),
    (328, 200, 8, 2, dict(enable_lr=0x2402, aq_strength=2), None),
    (1920, 1080, 10, 2, dict(enable_lr=0x2504), (1024, 504)),
]


@pytest.mark.parametrize("w,h,bd,n,extra,meet", DECODE)
def test_dav1d_decodes_to_the_reconstruction(av1mi, oracle, w, h, bd, n, extra, meet):
    """IPPP chunks (keyint 3 with sub-sample vectors at 128, keyint 240 at 256), the CDEF search, adaptive quantisation, 1080p at 256"""
    import oracle_avif
    if not oracle_avif.have_libavif():
        pytest.skip("libavif (dav1d) is not available on this machine")
    frames = clip(oracle, w, h, bd, n, seed=60 + w, meet=meet)
    with av1mi.Context(0) as c:
        data, sizes, rep, want = base.encode(c, av1mi, frames, w, h, bd, **extra)
        units, _ = c.lr_wiener_fit_result(n)
    nr, nc = uref.grid(w, h, uref.shift_of(extra["enable_lr"]))
    assert units.shape[2:4] == (nr, nc) and units[:, 0, :, :, 0].any()   # the stream holds restored units
    base._assert_decodes(base._decode(oracle_avif, data, sizes, w, h, bd, n, extra.get("keyint", 1)), want, n)


def test_unit_size_changes_between_chunks(av1mi, oracle):
    """one context at one geometry through the unit sizes and back, fits on and off; every output and result equals a fresh context's"""
    w, h, bd = 264, 200, 10
    frames = wbase.clip(oracle, w, h, bd, 3, seed=7)
    runs = [dict(enable_lr=0x504), dict(enable_lr=0x2504), dict(enable_lr=0x1003), dict(enable_lr=0x1504, keyint=3), dict(enable_lr=4), dict(enable_lr=0x2402)]
    with av1mi.Context(0) as c:
        for kw in runs:
            d, s, _, r = base.encode(c, av1mi, frames, w, h, bd, **kw)
            res = c.lr_fit_result(len(frames)) + c.lr_wiener_fit_result(len(frames))
            with av1mi.Context(0) as fresh:
                d0, s0, _, r0 = base.encode(fresh, av1mi, frames, w, h, bd, **kw)
                res0 = fresh.lr_fit_result(len(frames)) + fresh.lr_wiener_fit_result(len(frames))
            assert d == d0 and s == s0, kw
            assert all(np.array_equal(a, b) for fa, fb in zip(r, r0) for a, b in zip(fa, fb)), kw
            assert all(a.shape == b.shape and np.array_equal(a, b) for a, b in zip(res, res0)), kw
            assert res[0].shape[2:4] == uref.grid(w, h, uref.shift_of(kw["enable_lr"])), kw


@pytest.mark.parametrize("v", [0x1001, 0x2001, 0x1504, 0x2403])
def test_unit_bits_encode(av1mi, oracle, ctx, v):
    """enable_lr with bit 12 or 13 encodes (the library before the feature returns AV1MI_E_INVALID_ARG), and the bytes differ from
    those of 64x64 units"""
    w, h, bd = 200, 136, 8
    frames = wbase.clip(oracle, w, h, bd, 1, seed=3)
    data = base.encode(ctx, av1mi, frames, w, h, bd, enable_lr=v)[0]
    assert data and data != base.encode(ctx, av1mi, frames, w, h, bd, enable_lr=v & ~0x3000)[0]


@pytest.mark.parametrize("v", [0x3001, 0x3504, 0x1000, 0x2000, 0x1005, 0x2101, 0x1900 | 2, 0x5001, 0x9002])
def test_unit_bits_refused(av1mi, oracle, ctx, v):
    """both bits, a bit with a low byte of 0, and a unit size on a value that is refused without it"""
    w, h, bd = 200, 136, 8
    frames = wbase.clip(oracle, w, h, bd, 1, seed=3)
    with pytest.raises(av1mi.EncodeFailed) as e:
        base.encode(ctx, av1mi, frames, w, h, bd, enable_lr=v)
    assert e.value.code == 1   # AV1MI_E_INVALID_ARG


# sha256 of the bitstream of the clip below with bits 12-13 clear, recorded from a build of the commit before the feature
PARENT_BYTES = {
    0x1: "b4fa05461339f28ffc39748dbd5f49a3877625c996d3e833a734a7e7c7a6c42d",
    0x2: "b88809ea4fd264122f99bf1326ba5b49332cba0ba56c39e889cd488346483628",
    0x3: "c402a1cb4e867dfbe2156f3ed710eab3e09df427a86e96356c59beaffbfef54d",
    0x4: "973de334b7c0f5bccb890c0a091318f4020ffb03d354496f46555ab939517f2d",
    0x104: "a38f0760481cfcde25f8d153814d9714e4f7a547cedb4271d78c987aff2170f0",
    0x403: "458a4c57aac290c121f810efb35afb5fdec599f2eae9ec5b5736bd2b8cb623a2",
    0x504: "312b22dbb0342f2addb1ab8b85ff9ff4de1c3ef4d2e4443338458f62ba83263d",
}


@pytest.mark.parametrize("lr", [1, 2, 3, 4, 0x104, 0x403, 0x504])
def test_bits_clear_is_unchanged(av1mi, oracle, ctx, lr):
    """with bits 12-13 clear the bytes are those of the commit before the feature"""
    w, h, bd = 328, 248, 10
    frames = wbase.clip(oracle, w, h, bd, 3, seed=123)
    data, sizes, _, _ = base.encode(ctx, av1mi, frames, w, h, bd, enable_lr=lr, keyint=2, deblock=1)
    digest = hashlib.sha256(data).hexdigest()
    print("enable_lr %#x: %s" % (lr, digest))
    assert digest == PARENT_BYTES[lr]


# sha256 of the bitstreams of the clips below, recorded from a build of the commit before the restoration kernels took their box filter,
# wave walk and tail from lr_pieces.h: with the seven above, every instantiation of the three kernels at both sample types, chroma
# sections of one unit and of two, and units larger than a cell
SHARED_CASES = [(202, 122, 8), (328, 248, 10)]   # signalled != coded size and a chroma pair with a lone last cell; 10-bit
SHARED_LR = (0x1001, 0x2002, 0x1003, 0x2104, 0x1403, 0x2504)
SHARED_BYTES = {
    (202, 8, 0x1001): "0c5fec41bdfe81e371b4780487a1ee5e86db49d2affb1b884ebe0f8c1cf7dba5",
    (328, 10, 0x1001): "2ea6f7992f218db91a56336580391e0c43a1ab9997321135515604570448e547",
    (202, 8, 0x2002): "00badb92c61dcc57ef50075d3db870ecf6eff0ea9bf8bf1dca91d25287f753be",
    (328, 10, 0x2002): "de954c3896726189a67b8475f76f38abf7da5440229cde9cf334fb33942291ca",
    (202, 8, 0x1003): "5be5fca06a868a870250fb8b2fa1a16aef63cddf4edae796da304dd6103a1d25",
    (328, 10, 0x1003): "fc21a2cb86cc18cb6562a3c102cfb70d7f51cac2bd288e0e756eff5bf1d13ba2",
    (202, 8, 0x2104): "d1803718bdf6a13ac2bf13932128de5d1908e39b88c91156ed1b7f63823ce50a",
    (328, 10, 0x2104): "7c899ac66a3a6796fa49d42a6408caa678da48cc5df2223ac96312cec52cd57d",
    (202, 8, 0x1403): "a007e48a7bc1989a7ca2299b5eca89c4e88090a2b2fc7313b9b8fe2dc96d5d9e",
    (328, 10, 0x1403): "1b3521c71ddc23c2d9b6132c5fcb25f7f2741f8b607806f3645bc568de677e02",
    (202, 8, 0x2504): "980cf72cc740625655c5f12f8bd2d6f38bbebada75f9c94d8cc7a67202eaf2f4",
    (328, 10, 0x2504): "2d01a2c471814edac92e44f9e9c89c7a9a2b54d08ca3b00669778d52aa306d65",
}


@pytest.mark.parametrize("w,h,bd", SHARED_CASES)
@pytest.mark.parametrize("lr", SHARED_LR, ids=["%#x" % v for v in SHARED_LR])
def test_shared_pieces_keep_the_bytes(av1mi, oracle, ctx, w, h, bd, lr):
    """with the kernels' shared pieces the bytes are those of the commit before them"""
    frames = wbase.clip(oracle, w, h, bd, 3, seed=123)
    data, sizes, _, _ = base.encode(ctx, av1mi, frames, w, h, bd, enable_lr=lr, keyint=2, deblock=1)
    digest = hashlib.sha256(data).hexdigest()
    print("%dx%d-%d enable_lr %#x: %s" % (w, h, bd, lr, digest))
    assert digest == SHARED_BYTES[(w, bd, lr)]
