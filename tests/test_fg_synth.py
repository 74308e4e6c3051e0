"""GPU tests of the film-grain synthesis (include/av1mi.h: av1mi_film_grain_synth, av1mi_film_grain_params_result,
av1mi_ctx_set_displayed_quality, av1mi_displayed_quality_result; av1-base_amd/csrc/fg_synth_kernel.hip): the kernels against the
restatement tests/fgs_ref.py - which dav1d's output pins (tests/test_fg_synth_host.py) - bit for bit, at the smallest sizes at which they
can go wrong; then inside the encoder: what the headers carry, the displayed picture's quality against the caller's frames, a stream
that does not depend on the switch, and dav1d's decode of the chunk against the synthesis of its reconstruction."""
import functools

import pytest

import fg_ar_ref
import fgs_ref as F

pytestmark = pytest.mark.gpu

CASES = F.cases()


@functools.lru_cache(maxsize=None)
def reference(i):
    """the restatement's frames of case i: computed once, shared, never changed"""
    name, bd, w, h, g, seeds, raw = CASES[i]
    return F.synth_frames(raw, w, h, bd, g, seeds)


def grain(av1mi, g):
    return av1mi.GrainParams.from_buffer_copy(F.pack(g))


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c[0] for c in CASES])
def test_kernel_equals_the_restatement(av1mi, ctx, i):
    """8x8 (one partial block, 4x4 chroma), 34x34 and 98x66 (a second block and stripe of overlap alone), 200x120; both depths; seeds 0 and
    0xFFFF; every form of the parameter set; saturated samples and zeros; the empty table copies"""
    name, bd, w, h, g, seeds, raw = CASES[i]
    got = ctx.film_grain_synth(av1mi.default_params(w, h, bd), raw, len(seeds), grain(av1mi, g), seeds=seeds)
    assert got.tobytes() == reference(i), name
    if name.startswith("zero/"):
        assert got.tobytes() == raw


def test_case_list_covers_the_paths():
    names = [c[0] for c in CASES]
    assert {(c[2], c[3], c[1]) for c in CASES} >= {(w, h, bd) for w, h in F.SIZES for bd in (8, 10)}
    assert any(len(c[5]) == 3 and 0 in c[5] and 0xFFFF in c[5] for c in CASES)
    for lag in (1, 2, 3):
        assert any(n.startswith("lag%dx/" % lag) for n in names)
    assert any("/max/" in n for n in names) and any("/zero/" in n for n in names) and any(n.startswith("zero/") for n in names)


def test_device_pointers_and_refusals(av1mi, ctx):
    """frames on the device give what host frames give; a misaligned pointer, out == frames and a refused parameter set are
    AV1MI_E_INVALID_ARG"""
    import torch
    i = [c[0] for c in CASES].index("fixed20/200x120/10")
    name, bd, w, h, g, seeds, raw = CASES[i]
    p = av1mi.default_params(w, h, bd)
    d_in = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()
    d_out = torch.zeros_like(d_in)
    assert ctx.film_grain_synth(p, d_in.data_ptr(), len(seeds), grain(av1mi, g), seeds=seeds, on_device=True, out_ptr=d_out.data_ptr()) is None
    torch.cuda.synchronize()
    assert d_out.cpu().numpy().tobytes() == reference(i) and d_in.cpu().numpy().tobytes() == raw
    for bad_in, bad_out in ((d_in.data_ptr() + 2, d_out.data_ptr()), (d_in.data_ptr(), d_out.data_ptr() + 2), (d_in.data_ptr(), d_in.data_ptr())):
        with pytest.raises(av1mi.EncodeFailed) as e:
            ctx.film_grain_synth(p, bad_in, len(seeds), grain(av1mi, g), seeds=seeds, on_device=True, out_ptr=bad_out)
        assert e.value.code == av1mi.E_INVALID_ARG
    bad = bytearray(F.pack(g))
    bad[73] = 4   # ar_coeff_lag
    with pytest.raises(av1mi.EncodeFailed) as e:
        ctx.film_grain_synth(p, raw, len(seeds), bytes(bad), seeds=seeds)
    assert e.value.code == av1mi.E_INVALID_ARG


def test_default_seeds_are_the_encoders_rule(av1mi, ctx):
    name, bd, w, h, g, seeds, raw = CASES[[c[0] for c in CASES].index("fixed20/98x66/8")]
    n = len(seeds)
    p = av1mi.default_params(w, h, bd, first_frame=336)   # 7391 + 173 * 337 wraps past 65535
    rule = [F.grain_seed(336, f) for f in range(n)]
    assert rule[0] > rule[1]
    by_rule = ctx.film_grain_synth(p, raw, n, grain(av1mi, g))
    assert by_rule.tobytes() == ctx.film_grain_synth(p, raw, n, grain(av1mi, g), seeds=rule).tobytes() == F.synth_frames(raw, w, h, bd, g, rule)
    assert by_rule.tobytes() != ctx.film_grain_synth(av1mi.default_params(w, h, bd), raw, n, grain(av1mi, g)).tobytes()


# ---------------------------------------------------------------- inside the encoder
N = 20
MODES = {"fixed": dict(film_grain=N), "estimate": dict(film_grain_estimate=N), "denoise": dict(film_grain_denoise=N),
         "estimate_ar2": dict(film_grain_estimate=N, film_grain_ar=2), "denoise_ar2": dict(film_grain_denoise=N, film_grain_ar=2),
         "fixed_tf": dict(film_grain=N, tf_frames=2, tf_strength=4)}
# all modes at both sizes as key and inter frames; the temporal filter rewrites the key frame of a chunk uploaded from the host; a size
# that is no multiple of 8: the reconstruction at the coded size, the caller's frames tight
ENCODES = [(w, h, bd, mode, keyint) for (w, h, bd) in ((64, 64, 8), (136, 72, 10)) for mode in ("fixed", "estimate", "denoise", "estimate_ar2") for keyint in (1, 240)]
ENCODES += [(136, 72, 8, "denoise_ar2", 240), (136, 72, 10, "fixed_tf", 240), (70, 58, 8, "fixed", 240), (70, 58, 10, "estimate", 1)]
FRAMES = 3
FIRST = 4


@functools.lru_cache(maxsize=None)
def clip(w, h, bd):
    """flat levels with correlated noise: an estimate with values, a fit with coefficients"""
    return fg_ar_ref.ar_clip(w, h, bd, FRAMES, [0.05, 0.20, -0.05, 0.45], 1, seed=w + bd)


def headers_of(data, sizes, keyint, mode):
    """per frame the parameter set its frame header carries: the mode says how long the string is - the fixed table's two points or the
    estimate's eight, the lag's coefficients"""
    form = F.header_params(N, not mode.startswith("fixed"), 2 if mode.endswith("ar2") else 0, [0] * 24, [0] * 75)
    out, pos = [], 0
    for f, size in enumerate(sizes):
        tu = data[pos:pos + size]
        pos += size
        frame = [o for o in F.obus(tu) if o[0] in (3, 6)][0]
        inter = f % keyint != 0
        g, _, _ = F.find_params(tu[frame[2]:frame[3]], F.grain_seed(FIRST, f), inter, length=len(F.params_bits(form, 0, inter)))
        out.append(g)
    return out


_ENCODED = {}


def encoded(av1mi, ctx, case):
    """a case's chunk encoded once with the switch on: (parameters, source, bytes, frame sizes, report, reconstruction, displayed
    quality, the headers' GrainParams, the reconstruction with that grain, av1mi_film_grain_result's table)"""
    if case not in _ENCODED:
        w, h, bd, mode, keyint = case
        src = clip(w, h, bd)
        p = av1mi.default_params(w, h, bd, keyint=keyint, first_frame=FIRST, **MODES[mode])
        try:
            ctx.set_displayed_quality(True)
            data, sizes, rep, recon = ctx.encode_chunk(p, src, FRAMES, want_recon=True)
            got, g, table = ctx.displayed_quality_result(FRAMES), ctx.film_grain_params_result(), ctx.film_grain_result()
        finally:
            ctx.set_displayed_quality(False)
        shown = ctx.film_grain_synth(p, recon.tobytes(), FRAMES, g).tobytes()
        _ENCODED[case] = (p, src, data, sizes, rep, recon.tobytes(), got, g, shown, table)
    return _ENCODED[case]


@pytest.mark.parametrize("w,h,bd,mode,keyint", ENCODES)
def test_encoder_reports_its_grain_and_the_displayed_picture(av1mi, ctx, w, h, bd, mode, keyint):
    p, src, data, sizes, rep, recon, got, g, shown, table = encoded(av1mi, ctx, (w, h, bd, mode, keyint))
    n = FRAMES
    # what the chunk's own frame headers carry, every frame
    mine = F.unpack(bytes(g))
    assert headers_of(data, sizes, keyint, mode) == [mine] * n
    assert len(mine["point_y"]) == (2 if mode.startswith("fixed") else 8) and mine["ar_coeff_lag"] == (2 if mode.endswith("ar2") else 0)
    if mode.startswith("fixed"):
        assert mine == F.fixed_params(N)
    else:
        assert [y for _, y in mine["point_y"]] == [int(v) for v in table[0]] and any(y for _, y in mine["point_y"])
    # the displayed picture: the reconstruction with the headers' grain, against the frames as the caller gave them
    assert shown == F.synth_frames(recon, w, h, bd, mine, [F.grain_seed(FIRST, f) for f in range(n)]) != recon
    assert got.tobytes() == ctx.quality(p, src, shown, n).tobytes() and int(got["sse"].sum()) > 0
    assert got.tobytes() != ctx.quality(p, src, recon, n).tobytes()
    # the stream, the reconstruction and the report do not depend on the switch
    data_off, sizes_off, rep_off, recon_off = ctx.encode_chunk(p, src, n, want_recon=True)
    assert data_off == data and sizes_off == sizes and recon_off.tobytes() == recon
    assert [rep_off.sse[pl] for pl in range(3)] == [rep.sse[pl] for pl in range(3)]
    off = ctx.displayed_quality_result(n)
    assert not off["sse"].any() and not off["ssim_sum"].any() and not off["windows"].any()
    assert bytes(ctx.film_grain_params_result()) == bytes(g)
    with pytest.raises(av1mi.EncodeFailed) as e:
        ctx.displayed_quality_result(n + 1)
    assert e.value.code == av1mi.E_INVALID_ARG


@pytest.mark.parametrize("w,h,bd,mode,keyint", ENCODES)
def test_dav1d_decodes_the_chunk_to_the_synthesis_of_its_reconstruction(av1mi, ctx, w, h, bd, mode, keyint):
    import oracle_avif
    if not oracle_avif.have_libavif():
        pytest.skip("libavif (dav1d) is not available on this machine")
    import edge_content
    p, src, data, sizes, rep, recon, got, g, shown, table = encoded(av1mi, ctx, (w, h, bd, mode, keyint))
    tus, pos = [], 0
    for s in sizes:
        tus.append(data[pos:pos + s])
        pos += s
    dec = edge_content.dav1d_decode(tus, w, h, bd, keyint)
    assert len(dec) == FRAMES and F.frame_bytes([pl for fr in dec for pl in fr], bd) == shown


def test_device_frames_and_the_other_switch(av1mi, ctx):
    """a chunk given on the device, with the quality switch on beside the displayed one: both results, each what its own pass gives"""
    import torch
    w, h, bd, n = 136, 72, 10, FRAMES
    src = clip(w, h, bd)
    p = av1mi.default_params(w, h, bd, keyint=240, first_frame=FIRST, film_grain_denoise=N, film_grain_temporal=1)
    d_src = torch.frombuffer(bytearray(src), dtype=torch.uint8).cuda()
    try:
        ctx.set_displayed_quality(True)
        ctx.set_quality(True)
        data, sizes, rep, recon = ctx.encode_chunk(p, src, n, want_recon=True)
        host = ctx.displayed_quality_result(n), ctx.quality_result(n)
        d_rec = torch.zeros_like(d_src)
        data_d, sizes_d, _, _ = ctx.encode_chunk(p, d_src.data_ptr(), n, on_device=True, want_recon=True, recon_ptr=d_rec.data_ptr())
        torch.cuda.synchronize()
        assert data_d == data and d_rec.cpu().numpy().tobytes() == recon.tobytes() and d_src.cpu().numpy().tobytes() == src
        assert ctx.displayed_quality_result(n).tobytes() == host[0].tobytes() and ctx.quality_result(n).tobytes() == host[1].tobytes()
        shown = ctx.film_grain_synth(p, recon.tobytes(), n, ctx.film_grain_params_result())
        assert host[0].tobytes() == ctx.quality(p, src, shown.tobytes(), n).tobytes()
        assert host[1].tobytes() != host[0].tobytes()   # the quality pass compares with the denoised source, without the grain
    finally:
        ctx.set_displayed_quality(False)
        ctx.set_quality(False)


def test_results_without_grain_or_chunk(av1mi, ctx):
    with av1mi.Context(0) as c:
        for call in (c.film_grain_params_result, lambda: c.displayed_quality_result(1)):
            with pytest.raises(av1mi.EncodeFailed) as e:
                call()
            assert e.value.code == av1mi.E_INVALID_ARG
    w, h, bd = 64, 64, 8
    try:
        ctx.set_displayed_quality(True)
        ctx.encode_chunk(av1mi.default_params(w, h, bd), clip(w, h, bd), FRAMES)   # film_grain = 0
        off = ctx.displayed_quality_result(FRAMES)
        assert not off["sse"].any() and not off["windows"].any()
        with pytest.raises(av1mi.EncodeFailed) as e:
            ctx.film_grain_params_result()
        assert e.value.code == av1mi.E_INVALID_ARG
    finally:
        ctx.set_displayed_quality(False)
