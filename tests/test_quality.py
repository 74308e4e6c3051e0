"""GPU tests of the quality pass (include/av1mi.h: av1mi_quality, av1mi_ctx_set_quality, av1mi_quality_result,
av1mi_encode_file_quality; av1-base_amd/csrc/quality_kernel.hip): every figure and every window of the map against the integer
restatement tests/ssim_ref.py, exactly - at the smallest sizes at which the pass can go wrong - then the same pass inside the
encoder and summed over a file."""
import functools

import numpy as np
import pytest

import ssim_ref

pytestmark = pytest.mark.gpu
ONE = 1 << 24

# (w, h, bit depth, frames): one luma window and chroma without any; 16x8; windows that start in one 64x64 tile and end in the next with
# chroma 33 wide; chroma 65x35 - rows that are not 4-byte aligned and a remainder the windows do not cover; three frames at both depths
SHAPES = [(8, 8, 8, 1), (16, 8, 8, 1), (66, 66, 8, 1), (72, 72, 8, 1), (72, 72, 10, 1), (130, 70, 10, 1), (200, 136, 8, 3), (200, 136, 10, 3)]
CONTENTS = ["noise", "identical", "max_zero", "checkerboard", "plus_minus_3"]


def plane_sizes(w, h):
    return [(h, w), ((h + 1) // 2, (w + 1) // 2), ((h + 1) // 2, (w + 1) // 2)]


def pack(frames, bd):
    """[frame][plane] arrays -> the tight chunk"""
    dt = np.uint16 if bd > 8 else np.uint8
    return b"".join(np.ascontiguousarray(p, dtype=dt).tobytes() for fr in frames for p in fr)


def random_frames(rng, w, h, bd, n):
    return [[rng.integers(0, 1 << bd, s) for s in plane_sizes(w, h)] for _ in range(n)]


@functools.lru_cache(maxsize=None)
def case(w, h, bd, n, content):
    """(ref chunk, test chunk, ssim_ref's quality of the pair): computed once, shared, never changed"""
    m = (1 << bd) - 1
    if content == "noise":
        # independent noise, the first seed whose reference has a negative window (an 8x8 frame has one window in all)
        for seed in range(64):
            rng = np.random.default_rng(seed)
            a, b = pack(random_frames(rng, w, h, bd, n), bd), pack(random_frames(rng, w, h, bd, n), bd)
            want = ssim_ref.quality(a, b, w, h, bd, n)
            if any((mp < 0).any() for fr in want[1] for mp in fr):
                return a, b, want
        raise AssertionError("no seed gives a negative window")
    rng = np.random.default_rng(1000 + w + h + bd)
    fa = random_frames(rng, w, h, bd, n)
    if content == "identical":
        fb = fa
    elif content == "max_zero":
        fa = [[np.full(s, m) for s in plane_sizes(w, h)] for _ in range(n)]
        fb = [[np.zeros(s, int) for s in plane_sizes(w, h)] for _ in range(n)]
    elif content == "checkerboard":
        fa = [[(np.add.outer(np.arange(s[0]), np.arange(s[1])) & 1) * m for s in plane_sizes(w, h)] for _ in range(n)]
        fb = [[m - p for p in fr] for fr in fa]
    else:
        fb = [[np.clip(p + rng.integers(-3, 4, p.shape), 0, m) for p in fr] for fr in fa]
    a, b = pack(fa, bd), pack(fb, bd)
    return a, b, ssim_ref.quality(a, b, w, h, bd, n)


def check(got, want, n):
    """out and the whole window map, exactly"""
    q, maps = got
    wq, wmaps = want
    for f in range(n):
        for pl in range(3):
            assert (int(q[f, pl]["sse"]), int(q[f, pl]["ssim_sum"]), int(q[f, pl]["windows"])) == wq[f][pl], (f, pl)
            assert maps[f][pl].shape == wmaps[f][pl].shape and np.array_equal(maps[f][pl], wmaps[f][pl]), (f, pl)


@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("w,h,bd,n", SHAPES)
def test_quality_equals_the_restatement(av1mi, ctx, w, h, bd, n, content):
    a, b, want = case(w, h, bd, n, content)
    p = av1mi.default_params(w, h, bd)
    got = ctx.quality(p, a, b, n, want_map=True)
    check(got, want, n)
    allmaps = [mp for fr in want[1] for mp in fr if mp.size]
    if content == "noise":
        assert any((mp < 0).any() for mp in allmaps)   # the sign path is run
    elif content == "identical":
        assert all((mp == ONE).all() for mp in allmaps) and all(s == 0 for fr in want[0] for s, _, _ in fr)
        assert int(got[0]["sse"].sum()) == 0
    elif content == "max_zero":
        assert all((mp == 1677).all() for mp in allmaps)
    elif content == "checkerboard":
        assert all((mp == -16716926).all() for mp in allmaps)
    if (w, h) == (8, 8):
        assert [int(x) for x in got[0][0]["windows"]] == [1, 0, 0]   # the chroma of an 8x8 frame has no window - and still its squared error
        assert [s for s, _, _ in want[0][0]] == [int(x) for x in got[0][0]["sse"]]


@pytest.mark.parametrize("w,h,bd,n", [(130, 70, 10, 1), (200, 136, 8, 3)])
def test_device_input_and_repeatability(av1mi, ctx, w, h, bd, n):
    """frames on the device give what host frames give; two runs of one input give equal bytes; a misaligned device pointer is refused"""
    import torch
    a, b, want = case(w, h, bd, n, "noise")
    p = av1mi.default_params(w, h, bd)
    da, db = torch.frombuffer(bytearray(a), dtype=torch.uint8).cuda(), torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
    got = ctx.quality(p, da.data_ptr(), db.data_ptr(), n, on_device=True, want_map=True)
    check(got, want, n)
    again = ctx.quality(p, da.data_ptr(), db.data_ptr(), n, on_device=True, want_map=True)
    assert got[0].tobytes() == again[0].tobytes()
    assert all(x.tobytes() == y.tobytes() for fx, fy in zip(got[1], again[1]) for x, y in zip(fx, fy))
    host = ctx.quality(p, a, b, n, want_map=True)
    assert got[0].tobytes() == host[0].tobytes()
    q_only = ctx.quality(p, a, b, n)   # without the map
    assert q_only.tobytes() == got[0].tobytes()
    with pytest.raises(av1mi.EncodeFailed) as e:
        ctx.quality(p, da.data_ptr() + 2, db.data_ptr(), n, on_device=True)
    assert e.value.code == av1mi.E_INVALID_ARG
    # only the size and the depth of the parameters matter
    other = av1mi.default_params(w, h, bd, cq_level=63, keyint=240, enable_lr=2, film_grain=20)
    assert ctx.quality(other, a, b, n).tobytes() == got[0].tobytes()


def clip(w, h, bd, n, seed=3):
    """a moving texture with a little noise: something the encoder codes with a real error"""
    rng = np.random.default_rng(seed)
    m = (1 << bd) - 1
    frames = []
    for t in range(n):
        fr = []
        for k, (ph, pw) in enumerate(plane_sizes(w, h)):
            y, x = np.mgrid[0:ph, 0:pw]
            v = 0.5 + 0.25 * np.sin((x + 2 * t) / (5.0 + k)) * np.cos((y - t) / (7.0 + k)) + 0.2 * (((x + t) // 16 + y // 16) & 1) + rng.normal(0, 0.02, (ph, pw))
            fr.append(np.clip(np.rint(v * m * 0.8), 0, m).astype(np.int64))
        frames.append(fr)
    return pack(frames, bd)


# all key frames; IPPP; IPPP at a size that is no multiple of 8 - the encoder's buffers at the coded size with the signalled size inside
@pytest.mark.parametrize("w,h,bd,n,kw", [(200, 136, 8, 3, dict(keyint=1)), (200, 136, 10, 5, dict(keyint=240)), (202, 138, 8, 5, dict(keyint=240))])
def test_encoder_switch(av1mi, ctx, w, h, bd, n, kw):
    src = clip(w, h, bd, n)
    p = av1mi.default_params(w, h, bd, **kw)
    try:
        ctx.set_quality(True)
        data, sizes, rep, recon = ctx.encode_chunk(p, src, n, want_recon=True)
        got = ctx.quality_result(n)
        want = ctx.quality(p, src, recon.tobytes(), n)   # the coded source is the caller's: no temporal filter, no denoiser
        assert got.tobytes() == want.tobytes()
        ref = ssim_ref.quality(src, recon.tobytes(), w, h, bd, n)[0]
        assert [[tuple(int(v) for v in got[f, pl]) for pl in range(3)] for f in range(n)] == ref
        assert int(got["sse"].sum()) > 0 and (got["windows"][:, 0] == ssim_ref.windows_along(h) * ssim_ref.windows_along(w)).all()
        if w % 8 == 0 and h % 8 == 0:   # (the report's squared error runs over the coded size)
            for pl in range(3):
                assert float(int(got["sse"][:, pl].sum())) == rep.sse[pl]
        ctx.set_quality(False)
        data_off, sizes_off, rep_off, recon_off = ctx.encode_chunk(p, src, n, want_recon=True)
        assert data_off == data and sizes_off == sizes and recon_off.tobytes() == recon.tobytes()
        assert [rep_off.sse[pl] for pl in range(3)] == [rep.sse[pl] for pl in range(3)]
        off = ctx.quality_result(n)
        assert not off["sse"].any() and not off["ssim_sum"].any() and not off["windows"].any()
        with pytest.raises(av1mi.EncodeFailed) as e:
            ctx.quality_result(n + 1)
        assert e.value.code == av1mi.E_INVALID_ARG
    finally:
        ctx.set_quality(False)


def test_quality_result_without_a_chunk(av1mi):
    with av1mi.Context(0) as c:
        with pytest.raises(av1mi.EncodeFailed) as e:
            c.quality_result(1)
        assert e.value.code == av1mi.E_INVALID_ARG


def test_file_path_sums_its_chunks(av1mi, ctx, tmp_path):
    """av1mi_encode_file_quality: the sums of its chunks' results, and the file av1mi_encode_file writes"""
    w, h, bd, n, cf = 200, 136, 8, 7, 3
    src = clip(w, h, bd, n, seed=8)
    fb = w * h * 3 // 2
    y4m = tmp_path / "clip.y4m"
    with open(y4m, "wb") as f:
        f.write(b"YUV4MPEG2 W%d H%d F30:1 Ip A1:1 C420jpeg\n" % (w, h))
        for t in range(n):
            f.write(b"FRAME\n" + src[t * fb:(t + 1) * fb])
    enc = dict(keyint=240)
    plain, withq = tmp_path / "plain.ivf", tmp_path / "quality.ivf"
    rep_plain = av1mi.run_mi355x(av1mi.EncodeParams(y4m, plain, tmp_path, av1mi.derive_plan(8), chunk_frames=cf, **enc))
    rep, qsum = av1mi.encode_file_quality(av1mi.EncodeParams(y4m, withq, tmp_path, av1mi.derive_plan(8), chunk_frames=cf, **enc))
    assert withq.read_bytes() == plain.read_bytes() and rep.frames == rep_plain.frames == n and rep.chunks == 3
    assert [rep.sse[pl] for pl in range(3)] == [rep_plain.sse[pl] for pl in range(3)]
    # the chunks one by one, as the file path cuts them
    total = np.zeros(3, dtype=qsum.dtype)
    try:
        ctx.set_quality(True)
        for first in range(0, n, cf):
            k = min(cf, n - first)
            p = av1mi.default_params(w, h, bd, first_frame=first, **enc)
            ctx.encode_chunk(p, src[first * fb:(first + k) * fb], k)
            q = ctx.quality_result(k)
            for name in ("sse", "ssim_sum", "windows"):
                total[name] += q[name].sum(axis=0)
    finally:
        ctx.set_quality(False)
    assert qsum.tobytes() == total.tobytes()
    assert [float(int(v)) for v in qsum["sse"]] == [rep.sse[pl] for pl in range(3)]
    s = av1mi.ssim_of(qsum)
    assert 0.0 < s["y"] < 1.0 and 0.0 < s["all"] < 1.0 and s["db"] > 0
    # the contexts went back to the cache with the switch off: a plain job after it reports nothing and writes the same file
    again = tmp_path / "again.ivf"
    av1mi.run_mi355x(av1mi.EncodeParams(y4m, again, tmp_path, av1mi.derive_plan(8), chunk_frames=cf, **enc))
    assert again.read_bytes() == plain.read_bytes()
