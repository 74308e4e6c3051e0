"""Tests of the film grain's autoregressive fit on the GPU (include/av1mi.h: av1mi_params.film_grain bits 12-13, av1mi_film_grain_ar_estimate,
av1mi_film_grain_ar_result).

The pass is restated with tests/fg_ar_ref.py and compared exactly - sums, flat blocks, coefficients, gains and both tables.  What the
encoder does with the fit is held against the same mode without a lag (same reconstruction, same tile data) and against the restatement's
film_grain_params string; what a decoder makes of it against dav1d (libavif): the grain it adds keeps the sigma the estimate measured and
has the horizontal correlation of the noise the clip was made with."""
import os
import sys

import numpy as np
import pytest

import edge_content
import fg_ar_ref as ar
import fg_ref
from test_fg import encode, frame_payloads, same_frames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

N = 50
TRUTH = [0.05, 0.20, -0.05, 0.45]   # lag 1: above left, above, above right, left
LAGS = (1, 2, 3)

_clips = {}


def the_clip(kind, w, h, bd, n):
    """(bytes, {lag: the restatement's fit at the ceiling N}) - computed once per clip and left unchanged"""
    key = (kind, w, h, bd, n)
    if key not in _clips:
        if kind == "ar":
            raw = ar.ar_clip(w, h, bd, n, TRUTH, 1, split=True)
        elif kind == "const_u":
            fr = fg_ref.split(ar.ar_clip(w, h, bd, n, TRUTH, 1), w, h, bd, n)
            raw = fg_ref.join([[y, np.full_like(u, 128 << (bd - 8)), v] for y, u, v in fr], bd)
        elif kind == "checker":
            raw = fg_ref.checker_clip(w, h, bd, n)
        else:
            raw = ar.step_clip(w, h, bd, n, kind == "vstep")
        _clips[key] = (raw, {lag: ar.fit(raw, w, h, bd, n, N, lag) for lag in LAGS})
    return _clips[key]


@pytest.fixture(scope="module")
def ctx(av1mi):
    c = av1mi.Context(0)
    yield c
    c.close()


# one block (the fit is absent); no block; two blocks a frame; 10 bits; a width that is no multiple of 16 with an odd count of block pairs;
# more than one workgroup at 10 bits (75 steps, one each); more than one step of a workgroup - 35 x 58 blocks of 4 frames are 1044 steps for
# the grid's 1024 workgroups, and every row's last pair lacks its right block; a plane without noise; blocks only the energy condition
# keeps out
CONTENT = [("ar", 16, 16, 8, 1), ("ar", 8, 8, 8, 1), ("ar", 40, 24, 8, 2), ("ar", 72, 56, 10, 3), ("ar", 202, 122, 8, 2), ("ar", 328, 248, 10, 2),
           ("ar", 568, 928, 8, 4), ("const_u", 202, 122, 8, 2), ("vstep", 202, 122, 8, 2), ("hstep", 136, 120, 10, 2), ("checker", 72, 56, 8, 3), ("checker", 136, 72, 10, 2)]
FIELDS = ("sums", "flat", "coeffs", "gain", "table", "sigma_table")


def assert_equal_fit(got, want, where):
    for name in FIELDS:
        assert np.array_equal(got[name], want[name]), (where, name, np.asarray(got[name]).tolist(), np.asarray(want[name]).tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("kind,w,h,bd,n", CONTENT)
def test_pass_equals_the_rule(av1mi, ctx, kind, w, h, bd, n):
    import torch
    raw, fits = the_clip(kind, w, h, bd, n)
    dev = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()
    for lag in LAGS:
        want = fits[lag]
        p = av1mi.default_params(w, h, bd, film_grain_estimate=N, film_grain_ar=lag)
        assert_equal_fit(ctx.film_grain_ar_estimate(p, raw, n), want, ("host input", lag))
        assert_equal_fit(ctx.film_grain_ar_estimate(p, dev.data_ptr(), n, on_device=True), want, ("device input", lag))
        assert_equal_fit(ctx.film_grain_ar_estimate(p, raw, n), want, ("a second launch", lag))
        # the estimate and the denoiser's table are the sigma table, with or without the lag in the field
        t, _, _ = ctx.film_grain_estimate(p, raw, n, want_blocks=False)
        assert np.array_equal(t, want["sigma_table"]), lag
        used = 2 * lag * (lag + 1)
        assert not want["coeffs"][:, used:].any()
        for k in range(ar.SUMS):
            dy, dx = (0, k) if k < 7 else (1 + (k - 7) // 13, (k - 7) % 13 - 6)
            if dy > lag or abs(dx) > 2 * lag:
                assert not want["sums"][:, k].any()
        if (w, h) in ((16, 16), (8, 8), (40, 24)) or kind == "checker":
            assert want["present"] == [False] * 3 and (want["gain"] == 256).all() and np.array_equal(want["table"], want["sigma_table"])
            if (w, h) == (8, 8) or kind == "checker":
                assert not want["flat"].any() and not want["sums"].any()
        elif kind == "ar" and w >= 202:
            assert want["present"] == [True] * 3 and (want["gain"] < 250).all() and (want["flat"] >= 16).all()
            assert (want["table"] <= want["sigma_table"]).all() and (want["table"] < want["sigma_table"]).any()
        elif kind == "const_u":
            assert want["present"] == [True, False, True] and want["flat"][1] == 0 and want["gain"][1] == 256 and not want["coeffs"][1].any()
        elif kind in ("vstep", "hstep"):   # the step blocks of the top row are candidates - v = 0 under a quartile of at least 1 - and none of them is flat
            blocks = fg_ref.blocks_of(raw, w, h, bd, n)
            q, _ = ar.quartiles(blocks)
            k = int(blocks[0, 0, 0, 0])
            for pl in range(3):
                assert q[pl][k] >= 1 and (blocks[:, 0, :, 1 + pl] == 0).all()
                assert 0 < want["flat"][pl] <= int((blocks[:, 1:, :, 1 + pl] <= q[pl][k]).sum())


@pytest.mark.gpu
def test_pass_refuses_a_field_without_a_lag(av1mi, ctx):
    raw, _ = the_clip("ar", 72, 56, 10, 3)
    for kw in (dict(film_grain=20), dict(film_grain_estimate=20), dict(film_grain_denoise=20)):
        with pytest.raises(av1mi.EncodeFailed) as e:
            ctx.film_grain_ar_estimate(av1mi.default_params(72, 56, 10, **kw), raw, 3)
        assert e.value.code == 1


# ---------------------------------------------------------------- the chunk: the lag-free mode's reconstruction and tiles, the pass's fit
CHUNKS = [(202, 122, 8, 2, 1, dict(keyint=1, film_grain_estimate=N)), (202, 122, 8, 2, 2, dict(keyint=240, first_frame=9, film_grain_denoise=N)),
          (328, 248, 10, 2, 3, dict(keyint=240, deblock=2, cdef_search=2, enable_lr=2, tf_frames=1, tf_strength=2, film_grain_denoise=N)),
          (202, 122, 8, 2, 3, dict(keyint=1, film_grain_denoise=N))]


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,bd,n,lag,kw", CHUNKS)
def test_chunk_carries_the_pass_fit(av1mi, w, h, bd, n, lag, kw):
    """all key frames and IPPP; with the header-patching searches, the temporal filter and the denoiser on: the fit reads the caller's
    frames, its coefficients and scaled points stand in every header, and nothing else moves"""
    raw, fits = the_clip("ar", w, h, bd, n)
    want = fits[lag]
    other = 1 if lag == 3 else lag + 1
    with av1mi.Context(0) as c:
        d0, s0, _, r0 = encode(c, av1mi, raw, w, h, bd, n, **kw)
        table0 = c.film_grain_result()
        coeffs0, sigma0, gain0 = c.film_grain_ar_result()
        d1, s1, _, r1 = encode(c, av1mi, raw, w, h, bd, n, film_grain_ar=lag, **kw)
        table1 = c.film_grain_result()
        coeffs1, sigma1, gain1 = c.film_grain_ar_result()
        alone = c.film_grain_ar_estimate(av1mi.default_params(w, h, bd, film_grain_ar=lag, **kw), raw, n)
        d2, s2, _, r2 = encode(c, av1mi, raw, w, h, bd, n, film_grain_ar=other, **kw)      # another lag on the same workspace
        table2 = c.film_grain_result()
        d3, s3, _, r3 = encode(c, av1mi, raw, w, h, bd, n, film_grain_ar=lag, **kw)        # ... the first one again
        d4, s4, _, r4 = encode(c, av1mi, raw, w, h, bd, n, **kw)                           # ... and none
        d5, s5, _, _ = encode(c, av1mi, raw, w, h, bd, n, keyint=kw["keyint"], film_grain=N)   # the mode off
        d6, s6, _, _ = encode(c, av1mi, raw, w, h, bd, n, film_grain_ar=lag, **kw)
    assert not coeffs0.any() and not sigma0.any() and (gain0 == 256).all() and np.array_equal(table0, want["sigma_table"])
    assert_equal_fit(alone, want, "the pass alone")
    assert np.array_equal(table1, want["table"]) and np.array_equal(coeffs1, want["coeffs"]) and np.array_equal(sigma1, want["sigma_table"])
    assert np.array_equal(gain1, want["gain"]) and np.array_equal(table2, fits[other]["table"])
    assert same_frames(r0, r1) and same_frames(r0, r2) and same_frames(r0, r3)
    assert (d3, s3) == (d1, s1) == (d6, s6) and (d4, s4) == (d0, s0) and len(d2) != len(d1) and d5 != d0
    first = kw.get("first_frame", 0)
    extra = 6 * lag * (lag + 1)
    for f, (base, fit) in enumerate(zip(frame_payloads(d0, s0), frame_payloads(d1, s1))):
        inter = int(f % kw["keyint"] != 0)
        seed = fg_ref.grain_seed(first, f)
        btail, tail = fg_ref.params_bits(table0, seed, inter), ar.params_bits(want["table"], want["coeffs"], lag, seed, inter)
        bb, fb = fg_ref.header_bits(base, min(len(base), 600) * 8), fg_ref.header_bits(fit, min(len(fit), 600 + extra) * 8)
        at = [i for i in range(len(bb) - len(btail) + 1) if bb[i:i + len(btail)] == btail]
        assert len(at) == 1, (f, at)                     # where the lag-free header's film_grain_params stand
        head = at[0]
        assert len(fit) == len(base) + extra, f           # 48 L (L + 1) bits
        assert fb[:head] == bb[:head], f                 # everything before them, the other searches' fields included
        assert fb[head:head + len(tail)] == tail, f      # the pass's fit
        assert fit[(head + len(tail) + 7) // 8:] == base[(head + len(btail) + 7) // 8:], f   # and the same tiles behind


# ---------------------------------------------------------------- dav1d synthesises the grain the fit asks for
def lag1(x):
    """horizontal lag-1 correlation of the planes' rows in x [frame][row][column], less each frame's mean"""
    x = x - x.mean(axis=(1, 2), keepdims=True)
    return float((x[:, :, :-1] * x[:, :, 1:]).mean() / (x * x).mean())


CORR_MARGIN = 0.226


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,bd,n,lag", [(202, 122, 8, 2, 1), (328, 248, 10, 2, 2)])
def test_dav1d_adds_the_fitted_grain(av1mi, w, h, bd, n, lag):
    """decoded minus reconstruction has, per half and plane, a standard deviation within 15 % of sigma_table / 64 * 2^(bd - 8) wherever that
    value is at least 40 - the gain compensation at work - and per plane a horizontal lag-1 correlation within CORR_MARGIN of the injected
    noise's.  Measured with the restatement's header values (the device's, by the tests above), injected -> synthesised: 202x122 lag 1
    Y 0.482 -> 0.420, U 0.459 -> 0.373, V 0.423 -> 0.310; 328x248 lag 2 Y 0.478 -> 0.461, U 0.476 -> 0.369, V 0.470 -> 0.404.  The worst
    deviation is 0.113, the margin twice that.  (The standard deviations came out within 7 % of the wanted ones.)"""
    import oracle_avif
    if not oracle_avif.have_libavif():
        pytest.skip("libavif (dav1d) is not available on this machine")
    raw, fits = the_clip("ar", w, h, bd, n)
    want = fits[lag]
    with av1mi.Context(0) as c:
        data, sizes, _, rec = encode(c, av1mi, raw, w, h, bd, n, film_grain_estimate=N, film_grain_ar=lag, keyint=1)
        assert np.array_equal(c.film_grain_result(), want["table"]) and np.array_equal(c.film_grain_ar_result()[0], want["coeffs"])
    tus, off = [], 0
    for s in sizes:
        tus.append(data[off:off + s])
        off += s
    got = edge_content.dav1d_decode(tus, w, h, bd, 1)
    assert edge_content.decodes_to(got, rec, bd, N) is None
    src = fg_ref.split(raw, w, h, bd, n)
    xs, checked = fg_ref.split_column(w), 0
    for pl in range(3):
        at = xs if pl == 0 else xs // 2
        diff = np.concatenate([(np.asarray(got[f][pl]).astype(np.int64) - rec[f][pl])[None] for f in range(n)]).astype(np.float64)
        for half, region in ((0, diff[:, :, :at]), (1, diff[:, :, at:])):
            value = int(want["sigma_table"][pl][(112, 208)[half] >> 5])   # (the chroma planes go by their luma's bin)
            wanted = value / 64.0 * (1 << (bd - 8))
            sd = float(region.std())
            print("%dx%dx%d lag %d plane %d half %d: sigma table %d, header %d, sigma %.3f, wanted %.3f" % (w, h, bd, lag, pl, half, value, int(want["table"][pl][(112, 208)[half] >> 5]), sd, wanted))
            if value >= 40:
                assert abs(sd - wanted) <= 0.15 * wanted, (pl, half, value, sd, wanted)
                checked += 1
        noise = np.concatenate([src[f][pl][None, :, :at] for f in range(n)]).astype(np.float64)
        injected, synthesised = lag1(noise), lag1(diff[:, :, :at])
        print("%dx%dx%d lag %d plane %d: lag-1 correlation injected %.3f, synthesised %.3f, deviation %.3f" % (w, h, bd, lag, pl, injected, synthesised, abs(injected - synthesised)))
        assert abs(injected - synthesised) <= CORR_MARGIN, (pl, injected, synthesised)
    assert checked >= 3
