"""Tests of the film-grain denoiser (include/av1mi.h: av1mi_params.film_grain bits 8 and 10, av1mi_film_grain_denoise).

The pass is restated with tests/fgd_ref.py and compared exactly, at every table the caller may give and at the chunk's own estimate.  What
the encoder does with it is held against the estimate mode on the stand-alone call's output: same frame sizes, same reconstruction, same
tile data, the table of the frames as the caller gave them in the headers."""
import ctypes as C

import numpy as np
import pytest

import edge_content
import fg_ref
import fgd_ref
from test_fg import encode, frame_payloads, same_frames
from test_lr_chroma import split_frames

N = 50   # the ceiling: above 64 sigma of the generator's noise in every plane
# w, h, bit depth, frames: a chroma plane smaller than the window; padded and tiny; three frames; 10 bits; padded with an odd count of
# blocks (chroma 101 wide: rows of the caller's layout on odd addresses); more than one tile either way
SIZES = [(8, 8, 8, 1), (10, 14, 8, 1), (72, 56, 8, 3), (136, 72, 10, 2), (202, 122, 8, 2), (328, 248, 10, 2)]
FALLING = [[255, 200, 131, 130, 77, 3, 1, 0], [90, 80, 64, 33, 32, 9, 8, 0], [255, 0, 255, 0, 255, 0, 255, 0]]
ONE_BIN = [[0, 0, 0, 0, 200, 0, 0, 0]] * 3
TABLES = [("all 255", [[255] * 8] * 3), ("falling", FALLING), ("one bin", ONE_BIN)]

_clips = {}


def the_clip(kind, w, h, bd, n):
    """the bytes of a clip, made once"""
    key = (kind, w, h, bd, n)
    if key not in _clips:
        if kind == "ramp":
            _clips[key] = fgd_ref.ramp_clip(w, h, bd, n)[1]
        elif kind == "synth":
            import av1o
            _clips[key] = fg_ref.join([av1o.synthclip_frame(w, h, bd, seed=1080, t=t) for t in range(n)], bd)
        elif kind == "checker":
            _clips[key] = fg_ref.checker_clip(w, h, bd, n)
        else:
            mx = (1 << bd) - 1
            _clips[key] = fg_ref.join([[np.full((h, w), 517 >> (10 - bd)), np.full((h // 2, w // 2), 3), np.full((h // 2, w // 2), mx)] for _ in range(n)], bd)
    return _clips[key]


_wants = {}


def the_restatement(kind, w, h, bd, n, name, table):
    key = (kind, w, h, bd, n, name)
    if key not in _wants:
        _wants[key] = fgd_ref.denoise(the_clip(kind, w, h, bd, n), w, h, bd, n, np.asarray(table))
    return _wants[key]


def both_residencies(ctx, p, raw, n, **kw):
    """((where, denoised bytes, table)) of the stand-alone call on host and on device input; the device input must come back unchanged"""
    import torch
    out, table = ctx.film_grain_denoise(p, raw, n, **kw)
    yield "host input", out.tobytes(), table
    dev = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()
    res = torch.zeros_like(dev)
    _, table = ctx.film_grain_denoise(p, dev.data_ptr(), n, on_device=True, out_ptr=res.data_ptr(), **kw)
    assert dev.cpu().numpy().tobytes() == raw, "the caller's device frames were written"
    yield "device input", res.cpu().numpy().tobytes(), table


def first_difference(got, want, w, h, bd, n):
    a, b = fg_ref.split(got, w, h, bd, n), fg_ref.split(want, w, h, bd, n)
    for f in range(n):
        for pl in range(3):
            bad = np.argwhere(a[f][pl] != b[f][pl])
            if len(bad):
                r, c = bad[0]
                return "frame %d plane %d: %d samples differ, first at (%d, %d): %d, wanted %d" % (f, pl, len(bad), r, c, a[f][pl][r, c], b[f][pl][r, c])
    return None


# ---------------------------------------------------------------- (a) the pass equals the restatement
@pytest.mark.gpu
@pytest.mark.parametrize("w,h,bd,n", SIZES)
def test_pass_equals_the_rule_at_given_tables(av1mi, ctx, w, h, bd, n):
    raw = the_clip("ramp", w, h, bd, n)
    p = av1mi.default_params(w, h, bd, film_grain_denoise=N)
    for name, table in TABLES:
        want = the_restatement("ramp", w, h, bd, n, name, table)
        for where, got, ran_with in both_residencies(ctx, p, raw, n, use_table=table):
            assert np.array_equal(ran_with, np.asarray(table)), (name, where)   # as given: no ceiling
            assert got == want, (name, where, first_difference(got, want, w, h, bd, n))
    # the one-bin table filters chroma only under that luma range: the left half (luma 66 .. 90) comes back as it was, the right half does not
    if w >= 72:
        xs = fg_ref.split_column(w) // 2
        one = fg_ref.split(the_restatement("ramp", w, h, bd, n, "one bin", ONE_BIN), w, h, bd, n)
        src = fg_ref.split(raw, w, h, bd, n)
        assert all(np.array_equal(one[f][pl][:, :xs - 4], src[f][pl][:, :xs - 4]) and not np.array_equal(one[f][pl][:, xs:], src[f][pl][:, xs:])
                   for f in range(n) for pl in (1, 2))


@pytest.mark.gpu
@pytest.mark.parametrize("kind,w,h,bd,n", [("ramp", 202, 122, 8, 2), ("ramp", 136, 72, 10, 2), ("synth", 202, 122, 8, 2), ("synth", 136, 72, 10, 2)])
def test_pass_equals_the_rule_at_the_chunks_estimate(av1mi, ctx, kind, w, h, bd, n):
    raw = the_clip(kind, w, h, bd, n)
    table, _, _ = fg_ref.estimate(raw, w, h, bd, n, N)
    want = the_restatement(kind, w, h, bd, n, "estimate", table)
    assert want != raw
    p = av1mi.default_params(w, h, bd, film_grain_denoise=N)
    for where, got, ran_with in both_residencies(ctx, p, raw, n):
        assert np.array_equal(ran_with, table), (where, ran_with.tolist(), table.tolist())
        assert got == want, (where, first_difference(got, want, w, h, bd, n))


@pytest.mark.gpu
def test_pass_refuses_what_is_not_the_denoiser(av1mi, ctx):
    raw = the_clip("ramp", 72, 56, 8, 3)
    for kw in (dict(film_grain=0), dict(film_grain=20), dict(film_grain_estimate=20)):
        with pytest.raises(av1mi.EncodeFailed) as e:
            ctx.film_grain_denoise(av1mi.default_params(72, 56, 8, **kw), raw, 3)
        assert e.value.code == 1


# ---------------------------------------------------------------- (b) edge content
@pytest.mark.gpu
@pytest.mark.parametrize("w,h,bd,n", [(72, 56, 8, 3), (136, 72, 10, 2)])
def test_edge_content_comes_back_unchanged(av1mi, ctx, w, h, bd, n):
    p = av1mi.default_params(w, h, bd, film_grain_denoise=N)
    full = [[255] * 8] * 3
    for kind, table in (("ramp", [[0] * 8] * 3), ("flat", full), ("checker", full)):   # a zero table; a constant plane; neighbours equal or a full amplitude away
        raw = the_clip(kind, w, h, bd, n)
        for where, got, _ in both_residencies(ctx, p, raw, n, use_table=table):
            assert got == raw, (kind, where, first_difference(got, raw, w, h, bd, n))
    # the caller's host buffer, handed over as it is (the Python mirror would copy it), is only read
    raw = the_clip("ramp", w, h, bd, n)
    mine = np.frombuffer(bytearray(raw), dtype=np.uint8)
    out = np.empty_like(mine)
    given = np.array(full, dtype=np.uint8).reshape(24)
    rc = av1mi._lib.av1mi_film_grain_denoise(ctx._h, C.byref(p), mine.ctypes.data_as(C.c_void_p), n, 0, given.ctypes.data_as(C.POINTER(C.c_uint8)),
                                             out.ctypes.data_as(C.c_void_p), None)
    assert rc == 0 and mine.tobytes() == raw and out.tobytes() == the_restatement("ramp", w, h, bd, n, "all 255", full)


# ---------------------------------------------------------------- (c) the chunk codes the denoised frames under the table of the caller's
CHUNKS = [(w, h, bd, n, dict(keyint=k, **tf)) for (w, h, bd, n) in ((200, 136, 8, 4), (202, 122, 8, 3)) for k in (1, 3) for tf in ({}, dict(tf_frames=2, tf_strength=3))]


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,bd,n,kw", CHUNKS)
def test_chunk_codes_the_denoised_frames(av1mi, w, h, bd, n, kw):
    raw = the_clip("ramp", w, h, bd, n)
    table_raw, _, _ = fg_ref.estimate(raw, w, h, bd, n, N)
    with av1mi.Context(0) as c:
        denoised = c.film_grain_denoise(av1mi.default_params(w, h, bd, film_grain_denoise=N, **kw), raw, n)[0].tobytes()
        d1, s1, rep1, r1 = encode(c, av1mi, raw, w, h, bd, n, film_grain_denoise=N, **kw)
        got_table = c.film_grain_result()
        d2, s2, rep2, r2 = encode(c, av1mi, denoised, w, h, bd, n, film_grain_estimate=N, **kw)
        table_den = c.film_grain_result()
        coded = denoised
        if kw.get("tf_frames"):   # the encoder codes, and reports against, the filtered key frames of the denoised chunk
            coded = c.temporal_filter(av1mi.default_params(w, h, bd, film_grain_estimate=N, **kw), denoised, n, want_mv=False)[0].tobytes()
    assert denoised == the_restatement("ramp", w, h, bd, n, "estimate", table_raw) and denoised != raw
    assert np.array_equal(got_table, table_raw), (got_table.tolist(), table_raw.tolist())       # the estimate of the frames as the caller gave them
    assert np.array_equal(table_den, fg_ref.estimate(denoised, w, h, bd, n, N)[0]) and not np.array_equal(table_den, table_raw)
    assert list(s1) == list(s2) and same_frames(r1, r2)
    src = split_frames(coded, w, h, bd, n)
    want_sse = [sum(int(((r1[f][pl] - src[f][pl]) ** 2).sum()) for f in range(n)) for pl in range(3)]
    # against the denoised source: the estimate mode's report on `denoised`, and where the coded size is the signalled one the squared
    # error itself (the report sums over the coded size, whose samples past the picture no reconstruction is returned for)
    assert [int(x) for x in rep1.sse] == [int(x) for x in rep2.sse]
    if (w | h) & 7:
        assert all(int(a) >= b for a, b in zip(rep1.sse, want_sse))
    else:
        assert [int(x) for x in rep1.sse] == want_sse
    first = kw.get("first_frame", 0)
    for f, (a, b) in enumerate(zip(frame_payloads(d1, s1), frame_payloads(d2, s2))):
        inter = int(f % kw["keyint"] != 0)
        seed = fg_ref.grain_seed(first, f)
        ta, tb = fg_ref.params_bits(table_raw, seed, inter), fg_ref.params_bits(table_den, seed, inter)
        ba, bb = fg_ref.header_bits(a, min(len(a), 548) * 8), fg_ref.header_bits(b, min(len(b), 548) * 8)
        at = [i for i in range(len(ba) - len(ta) + 1) if ba[i:i + len(ta)] == ta]
        assert len(at) == 1, (f, at)                                # where the header's film_grain_params stand: the table of `raw`
        head = at[0]
        assert len(a) == len(b) and ba[:head] == bb[:head], f       # the same header in front of them
        assert bb[head:head + len(tb)] == tb, f
        assert a[(head + len(ta) + 7) // 8:] == b[(head + len(tb) + 7) // 8:], f   # and the same tiles behind


# ---------------------------------------------------------------- (d) dav1d decodes a denoise-mode stream
DECODE = [
    (328, 248, 10, 5, dict(tpl_strength=4, aq_strength=2, keyint=3, subpel=1, me_presearch=1, me_range=16)),
    (200, 136, 8, 4, dict(tpl_strength=4, keyint=240, tf_frames=3, tf_strength=2)),
]


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,bd,n,extra", DECODE)
def test_dav1d_decodes_to_the_reconstruction(av1mi, w, h, bd, n, extra):
    """two of tests/test_tpl.py's cases with the mode added; the decoder adds the table's grain to the reconstruction (edge_content.decodes_to
    with grain: a desynchronised stream decodes to garbage, not to noise)"""
    import oracle_avif
    if not oracle_avif.have_libavif():
        pytest.skip("libavif (dav1d) is not available on this machine")
    raw = the_clip("ramp", w, h, bd, n)
    with av1mi.Context(0) as c:
        data, sizes, _, rec = encode(c, av1mi, raw, w, h, bd, n, film_grain_denoise=N, **extra)
        assert np.array_equal(c.film_grain_result(), fg_ref.estimate(raw, w, h, bd, n, N)[0])
    tus, off = [], 0
    for s in sizes:
        tus.append(data[off:off + s])
        off += s
    got = edge_content.dav1d_decode(tus, w, h, bd, extra["keyint"])
    assert edge_content.decodes_to(got, rec, bd, N) is None


# ---------------------------------------------------------------- (e) reuse and determinism
@pytest.mark.gpu
def test_workspace_reuse_and_determinism(av1mi):
    w, h, bd, n = 202, 122, 8, 3
    raw = the_clip("ramp", w, h, bd, n)
    runs = [dict(film_grain_estimate=N), dict(film_grain_denoise=N), dict(), dict(film_grain_denoise=N), dict(film_grain=N), dict(film_grain_denoise=20, keyint=3)]
    seen = {}
    with av1mi.Context(0) as c:
        for kw in runs:
            d, s, _, r = encode(c, av1mi, raw, w, h, bd, n, **kw)
            with av1mi.Context(0) as fresh:
                d0, s0, _, r0 = encode(fresh, av1mi, raw, w, h, bd, n, **kw)
            assert d == d0 and list(s) == list(s0) and same_frames(r, r0), kw
            key = tuple(sorted(kw.items()))
            if key in seen:   # the same mode again on the same workspace
                assert seen[key] == d, kw
            seen[key] = d
    assert len(set(seen.values())) == len(seen)   # (every mode codes something else)


# ---------------------------------------------------------------- (f) bytes
@pytest.mark.gpu
def test_denoised_chunk_is_smaller(av1mi, ctx):
    """the generator's noisy clip at CQ 20: the chunk coded from the denoised frames is smaller than the estimate mode's (the oracle orders
    its key-frame encodes of the two the same way: tests/test_fgd_host.py).  Measured: 1 396 bytes in the estimate mode, 1 381 in the denoise
    mode - at this quantiser little of a sigma of 1 survives to be coded; the oracle's 1 213 and 1 198"""
    w, h, bd, n = 136, 72, 8, 3
    raw = the_clip("ramp", w, h, bd, n)
    est, _, _, _ = encode(ctx, av1mi, raw, w, h, bd, n, film_grain_estimate=N, cq_level=20)
    den, _, _, _ = encode(ctx, av1mi, raw, w, h, bd, n, film_grain_denoise=N, cq_level=20)
    print("bytes: estimate mode %d, denoise mode %d" % (len(est), len(den)))
    assert len(den) < len(est)
