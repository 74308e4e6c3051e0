#!/usr/bin/env python3
"""Film-grain table A/B: 1080p x 60, 10-bit, one chunk, the clip in HBM - bench.py's synthclip, textured
everywhere, and a clip of smooth ramps with injected Gaussian noise whose sigma grows with the luma (0.5 at black to 2.0 at white, 8-bit
scale; chroma 0.75) - coded with the fixed table, film_grain = N, with the table estimated from the chunk,
film_grain = AV1MI_FILM_GRAIN_ESTIMATE(N), and with the source denoised by that table as well, film_grain = AV1MI_FILM_GRAIN_DENOISE(N)
(DESIGN.md section 3 item 7c).  One JSON line per clip and chunk kind: the estimated table and the bins' block counts, frames/s of the estimate
and of the denoise runs (best of --steps after --warmup) and of the fixed runs alternated with them, bytes per frame of the three, "start ->
source ready" of the three (ms_h2d: the passes run there) and their differences - the estimate's milliseconds and the denoiser's -, the time
of the estimate's call alone (av1mi_film_grain_estimate, with its allocation), and on the noise clip, whose clean ramps the tool keeps, the
PSNR of the coded source against them before and after the denoiser (the caller's frames, and av1mi_film_grain_denoise's output).
A third clip, "arnoise", is the ramps with the same noise passed through a known autoregressive filter (AR_TRUTH, lag 1) first; on it the
tool also runs the fourth mode, estimated + denoised + the grain's autoregressive fit at lag 1, 2 and 3,
alternated with the denoise mode, and adds per lag the fitted Q7 coefficients beside the injected ones, the gains, the flat blocks and
their share of all blocks, the milliseconds of the new pass (the difference of "start -> source ready" against the denoise mode's)
beside the estimate's, and bytes per frame.
A fourth clip, "texture", is a field of independent random samples that moves two samples right and down per frame under Gaussian noise of
sigma 1 (8-bit scale) - what the spatial window finds no honest neighbour in.  On the clips whose clean original the tool keeps it also
runs the denoiser's temporal term at S = 1 and S = 2, film_grain = AV1MI_FILM_GRAIN_DENOISE_TEMPORAL(N, S),
alternated with the spatial mode (--spans; empty: none): per span the milliseconds of the denoiser's launches (the difference of "start ->
source ready" against the estimate mode's, as ms_pass_denoise is the spatial mode's), bytes per frame, and the PSNR of the coded source
against the clean clip.
On the two ramp clips it also measures the picture as displayed (--no-displayed leaves it out): per mode - fixed,
estimated, denoised, denoised + temporal, the last three also with the autoregressive fit at lag 1 - the chunk is coded with the
displayed-quality switch on, and the line carries the PSNR and SSIM of reconstruction + synthesised grain against the frames the tool
handed in (av1mi_displayed_quality_result) beside those of the reconstruction against the coded source, and the film-grain estimate of the
synthesised output (av1mi_film_grain_synth, then av1mi_film_grain_estimate on it) beside the source's: the displayed picture's noise per
luma bin.  It reports what it measures, nothing more."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "av1-base_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench  # noqa: E402


AR_TRUTH = [0.05, 0.20, -0.05, 0.45]   # lag 1: above left, above, above right, left


def ar_noise(torch, shape, g, dev, coeffs):
    """unit-variance noise through g[y][x] = sum c_i g[y + r_i][x + d_i] + white[y][x] (lag 1; the periodic plane, in the frequency domain)"""
    white = torch.randn(shape, generator=g, device=dev)
    if coeffs is None:
        return white
    wy = 2 * torch.pi * torch.fft.fftfreq(shape[0], device=dev)[:, None]
    wx = 2 * torch.pi * torch.fft.fftfreq(shape[1], device=dev)[None, :]
    H = 1 - sum(c * torch.exp(1j * (wy * r + wx * d)) for c, (r, d) in zip(coeffs, ((-1, -1), (-1, 0), (-1, 1), (0, -1))))
    out = torch.fft.ifft2(torch.fft.fft2(white) / H).real
    return out / out.std()


def noisy_ramp_clip(torch, w, h, bd, n, dev, seed=7, coeffs=None):
    """n frames of a horizontal luma ramp (black to white, a slow vertical tilt; the operator is blind to both) with Gaussian noise of
    sigma 0.5 + 1.5 luma / white at 8-bit scale, U and V flat with sigma 0.75; a new noise field every frame, white or (coeffs) through
    ar_noise.  Returns (the clip, the
    clean ramps in the same layout)"""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    sc, mx = float(1 << (bd - 8)), float((1 << bd) - 1)
    x = torch.arange(w, device=dev, dtype=torch.float32)[None, :] / (w - 1)
    y = torch.arange(h, device=dev, dtype=torch.float32)[:, None] / (h - 1)
    level = (16.0 + 219.0 * (0.9 * x + 0.1 * y)) * sc
    sigma = (0.5 + 1.5 * level / mx) * sc
    dt = torch.int16 if bd > 8 else torch.uint8
    frames = []
    clean_planes = [level.round().clamp(0, mx)] + [torch.full((h // 2, w // 2), 128.0 * sc, device=dev) for _ in range(2)]
    clean = torch.cat([p.to(dt).reshape(-1) for p in clean_planes]).repeat(n)
    for _ in range(n):
        luma = (level + sigma * ar_noise(torch, (h, w), g, dev, coeffs)).round().clamp(0, mx)
        planes = [luma] + [(128.0 * sc + 0.75 * sc * ar_noise(torch, (h // 2, w // 2), g, dev, coeffs)).round().clamp(0, mx) for _ in range(2)]
        frames.append(torch.cat([p.to(dt).reshape(-1) for p in planes]))
    return torch.cat(frames).view(torch.uint8), clean.view(torch.uint8)


def noisy_texture_clip(torch, w, h, bd, n, dev, seed=9, motion=(2, 2), sigma=1.0):
    """n frames of a random texture - luma independent uniform samples 60 .. 200 (8-bit scale), U and V 100 .. 156 - that moves `motion`
    luma samples right and down per frame (chroma half as far), with Gaussian noise of `sigma`, a new field every frame.  Returns (the clip,
    the clean frames in the same layout)"""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    sc, mx = 1 << (bd - 8), float((1 << bd) - 1)
    dt = torch.int16 if bd > 8 else torch.uint8
    mxs, mys = motion[0] * (n - 1), motion[1] * (n - 1)
    fields = [torch.randint(60 * sc, 200 * sc + 1, (h + mys, w + mxs), generator=g, device=dev).float()] + [
        torch.randint(100 * sc, 156 * sc + 1, (h // 2 + mys // 2, w // 2 + mxs // 2), generator=g, device=dev).float() for _ in range(2)]
    frames, clean = [], []
    for t in range(n):
        fc, fn = [], []
        for pl, fld in enumerate(fields):
            d, ph, pw = (1, h, w) if pl == 0 else (2, h // 2, w // 2)
            oy, ox = (n - 1 - t) * motion[1] // d, (n - 1 - t) * motion[0] // d
            c = fld[oy:oy + ph, ox:ox + pw]
            fc.append(c.to(dt).reshape(-1))
            fn.append((c + sigma * sc * torch.randn(c.shape, generator=g, device=dev)).round().clamp(0, mx).to(dt).reshape(-1))
        clean.append(torch.cat(fc))
        frames.append(torch.cat(fn))
    return torch.cat(frames).view(torch.uint8), torch.cat(clean).view(torch.uint8)


def psnr(av1mi, ctx, p, a, b, n):
    """of clip a against clip b, two device tensors in one tight layout, over every sample: compared on the device (av1mi_quality)"""
    s = av1mi.quality_sum(ctx.quality(p, b.data_ptr(), a.data_ptr(), n, on_device=True))
    return av1mi.psnr_of(s, p.width, p.height, p.bit_depth, n)["all"]


def displayed(torch, av1mi, ctx, p, est, clip, n):
    """one chunk with the displayed-quality switch on: the displayed picture's figures against the caller's frames, the reconstruction's
    against the coded source, and the estimate's luma table of reconstruction + synthesised grain (est: the parameters the estimate runs with)"""
    rec, shown = torch.empty_like(clip), torch.empty_like(clip)
    try:
        ctx.set_displayed_quality(True)
        ctx.set_quality(True)
        ctx.encode_chunk(p, clip.data_ptr(), n, on_device=True, want_recon=True, recon_ptr=rec.data_ptr(), copy_out=False)
        shown_q, coded_q = av1mi.quality_sum(ctx.displayed_quality_result(n)), av1mi.quality_sum(ctx.quality_result(n))
        g = ctx.film_grain_params_result()
    finally:
        ctx.set_displayed_quality(False)
        ctx.set_quality(False)
    ctx.film_grain_synth(p, rec.data_ptr(), n, g, on_device=True, out_ptr=shown.data_ptr())
    table, _, _ = ctx.film_grain_estimate(est, shown.data_ptr(), n, on_device=True, want_blocks=False)
    size = (p.width, p.height, p.bit_depth, n)
    return {"psnr_displayed_against_original": round(av1mi.psnr_of(shown_q, *size)["all"], 3), "ssim_displayed_against_original": round(av1mi.ssim_of(shown_q)["all"], 5),
            "psnr_recon_against_coded_source": round(av1mi.psnr_of(coded_q, *size)["all"], 3), "ssim_recon_against_coded_source": round(av1mi.ssim_of(coded_q)["all"], 5),
            "header_table_y": [int(g.point_y[k][1]) for k in range(g.num_y_points)], "displayed_estimate_table_y": table[0].tolist()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--clips", default="synth,noise,arnoise,texture")
    ap.add_argument("--spans", default="1,2", help="the temporal term's spans to run on the clips with a clean original; empty: none")
    ap.add_argument("--level", type=int, default=20, help="N: the fixed table's level and the estimate's ceiling")
    ap.add_argument("--keyints", default="1,240")
    ap.add_argument("--no-displayed", action="store_true", help="leave out the displayed picture's figures on the ramp clips")
    ap.add_argument("--extra", default="", help="further parameters for every run, name=value,...")
    args = ap.parse_args()
    import torch
    import av1mi
    w, h, bd, n = 1920, 1080, 10, args.frames
    dev = torch.device("cuda:0")
    extra = {k: int(v) for k, v in (kv.split("=") for kv in args.extra.split(",") if kv)}
    with av1mi.Context(0) as ctx:
        for name in args.clips.split(","):
            if name == "synth":
                clip, clean = bench.make_clip_torch(w, h, bd, n, 1080, dev), None
            elif name == "texture":
                clip, clean = noisy_texture_clip(torch, w, h, bd, n, dev)
            else:
                clip, clean = noisy_ramp_clip(torch, w, h, bd, n, dev, coeffs=AR_TRUTH if name == "arnoise" else None)
            torch.cuda.synchronize(dev)
            for keyint in (int(k) for k in args.keyints.split(",")):
                kw = dict(keyint=keyint, intra_mode_mask=0x7, **extra)
                fixed = av1mi.default_params(w, h, bd, film_grain=args.level, **kw)
                est = av1mi.default_params(w, h, bd, film_grain_estimate=args.level, **kw)
                den = av1mi.default_params(w, h, bd, film_grain_denoise=args.level, **kw)
                for _ in range(args.warmup):
                    for p in (fixed, est, den):
                        ctx.encode_chunk(p, clip.data_ptr(), n, on_device=True, copy_out=False)
                best = {"fixed": None, "estimate": None, "denoise": None}
                rep = {}
                for _ in range(args.steps):   # alternated: a fixed run in front of every estimate and denoise run
                    for tag, p in (("fixed", fixed), ("estimate", est), ("denoise", den)):
                        t0 = time.perf_counter()
                        _, _, r, _ = ctx.encode_chunk(p, clip.data_ptr(), n, on_device=True, copy_out=False)
                        dt = time.perf_counter() - t0
                        if best[tag] is None or dt < best[tag]:
                            best[tag], rep[tag] = dt, r
                table = ctx.film_grain_result()
                ctx.film_grain_estimate(est, clip.data_ptr(), n, on_device=True, want_blocks=False)
                t0 = time.perf_counter()
                alone, counts, _ = ctx.film_grain_estimate(est, clip.data_ptr(), n, on_device=True, want_blocks=False)
                ms_call = (time.perf_counter() - t0) * 1e3
                assert (alone == table).all()
                line = {"clip": name, "keyint": keyint, "level": args.level, "table_y": table[0].tolist(), "table_u": table[1].tolist(),
                        "table_v": table[2].tolist(), "blocks_per_bin": counts[0].tolist(),
                        "fps_estimate": round(n / best["estimate"], 1), "fps_denoise": round(n / best["denoise"], 1),
                        "fps_fixed_alternated": round(n / best["fixed"], 1),
                        "bytes_per_frame_estimate": round(rep["estimate"].bytes / n, 1), "bytes_per_frame_denoise": round(rep["denoise"].bytes / n, 1),
                        "bytes_per_frame_fixed": round(rep["fixed"].bytes / n, 1),
                        "psnr_y_estimate": round(rep["estimate"].psnr[0], 3), "psnr_y_denoise_against_the_denoised_source": round(rep["denoise"].psnr[0], 3),
                        "ms_start_to_source_ready_estimate": round(rep["estimate"].ms_h2d, 3),
                        "ms_start_to_source_ready_denoise": round(rep["denoise"].ms_h2d, 3),
                        "ms_start_to_source_ready_fixed": round(rep["fixed"].ms_h2d, 3),
                        "ms_pass": round(rep["estimate"].ms_h2d - rep["fixed"].ms_h2d, 3),
                        "ms_pass_denoise": round(rep["denoise"].ms_h2d - rep["estimate"].ms_h2d, 3), "ms_estimate_call": round(ms_call, 3)}
                if clean is not None:   # the coded source against the clean ramps, before and after the denoiser
                    out = torch.empty_like(clip)
                    _, ran_with = ctx.film_grain_denoise(den, clip.data_ptr(), n, on_device=True, out_ptr=out.data_ptr())
                    assert (ran_with == table).all()
                    line["psnr_source_against_clean_before"] = round(psnr(av1mi, ctx, den, clip, clean, n), 3)
                    line["psnr_source_against_clean_after"] = round(psnr(av1mi, ctx, den, out, clean, n), 3)
                    # the temporal term, alternated with the spatial mode
                    spans = {int(v): av1mi.default_params(w, h, bd, film_grain_denoise=args.level, film_grain_temporal=int(v), **kw) for v in args.spans.split(",") if v}
                    for p in spans.values():
                        ctx.encode_chunk(p, clip.data_ptr(), n, on_device=True, copy_out=False)
                    ms, ms_spatial, nbytes = {v: None for v in spans}, None, {}
                    for _ in range(args.steps):
                        for v, p in spans.items():
                            _, _, r0, _ = ctx.encode_chunk(den, clip.data_ptr(), n, on_device=True, copy_out=False)
                            _, _, r1, _ = ctx.encode_chunk(p, clip.data_ptr(), n, on_device=True, copy_out=False)
                            d0, d1 = r0.ms_h2d - rep["estimate"].ms_h2d, r1.ms_h2d - rep["estimate"].ms_h2d
                            ms_spatial = d0 if ms_spatial is None or d0 < ms_spatial else ms_spatial
                            if ms[v] is None or d1 < ms[v]:
                                ms[v], nbytes[v] = d1, r1.bytes
                    for v, p in spans.items():
                        ctx.film_grain_denoise(p, clip.data_ptr(), n, on_device=True, out_ptr=out.data_ptr())
                        line["temporal_s%d" % v] = {"ms_pass_denoise": round(ms[v], 3), "ms_pass_denoise_spatial_alternated": round(ms_spatial, 3),
                                                    "bytes_per_frame": round(nbytes[v] / n, 1),
                                                    "psnr_source_against_clean_after": round(psnr(av1mi, ctx, den, out, clean, n), 3)}
                    del out
                if name == "arnoise":   # the fourth mode, alternated with the denoise mode
                    lags = {lag: av1mi.default_params(w, h, bd, film_grain_denoise=args.level, film_grain_ar=lag, **kw) for lag in (1, 2, 3)}
                    for p in lags.values():
                        ctx.encode_chunk(p, clip.data_ptr(), n, on_device=True, copy_out=False)
                    ms, nbytes = {lag: None for lag in lags}, {}
                    for _ in range(args.steps):
                        for lag, p in lags.items():
                            _, _, r0, _ = ctx.encode_chunk(den, clip.data_ptr(), n, on_device=True, copy_out=False)
                            _, _, r1, _ = ctx.encode_chunk(p, clip.data_ptr(), n, on_device=True, copy_out=False)
                            d = r1.ms_h2d - r0.ms_h2d
                            if ms[lag] is None or d < ms[lag]:
                                ms[lag], nbytes[lag] = d, r1.bytes
                    line["ar_injected_q7"] = [round(128 * c) for c in AR_TRUTH]
                    for lag, p in lags.items():
                        fit = ctx.film_grain_ar_estimate(p, clip.data_ptr(), n, on_device=True)
                        used = 2 * lag * (lag + 1)
                        line["ar_lag%d" % lag] = {"coeffs_y": fit["coeffs"][0][:used].tolist(), "coeffs_u": fit["coeffs"][1][:used].tolist(),
                                                  "coeffs_v": fit["coeffs"][2][:used].tolist(), "gain": fit["gain"].tolist(), "flat_blocks": fit["flat"].tolist(),
                                                  "flat_share": round(float(fit["flat"][0]) / (n * (w // 16) * (h // 16)), 4),
                                                  "table_y": fit["table"][0].tolist(), "ms_pass_ar": round(ms[lag], 3), "ms_pass_estimate": line["ms_pass"],
                                                  "bytes_per_frame": round(nbytes[lag] / n, 1)}
                if name in ("noise", "arnoise") and not args.no_displayed:   # the picture as displayed, per mode; the source's own estimate beside it
                    modes = {"fixed": dict(film_grain=args.level), "estimate": dict(film_grain_estimate=args.level), "denoise": dict(film_grain_denoise=args.level),
                             "denoise_temporal": dict(film_grain_denoise=args.level, film_grain_temporal=1)}
                    line["source_estimate_table_y"] = table[0].tolist()
                    line["displayed"] = {}
                    for tag, mode in modes.items():
                        for lag in (0,) if tag == "fixed" else (0, 1):
                            p = av1mi.default_params(w, h, bd, film_grain_ar=lag or None, **mode, **kw)
                            line["displayed"][tag + ("_ar1" if lag else "")] = displayed(torch, av1mi, ctx, p, est, clip, n)
                print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
