#!/usr/bin/env python3
"""Film-grain table A/B: 1080p x 60, 10-bit, one chunk, the clip in HBM - bench.py's synthclip, textured
everywhere, and a clip of smooth ramps with injected Gaussian noise whose sigma grows with the luma (0.5 at black to 2.0 at white, 8-bit
scale; chroma 0.75) - coded with the fixed table, film_grain = N, with the table estimated from the chunk,
film_grain = AV1MI_FILM_GRAIN_ESTIMATE(N), and with the source denoised by that table as well, film_grain = AV1MI_FILM_GRAIN_DENOISE(N)
(DESIGN.md section 3 item 7c).  One JSON line per clip and chunk kind: the estimated table and the bins' block counts, frames/s of the estimate
and of the denoise runs (best of --steps after --warmup) and of the fixed runs alternated with them, bytes per frame of the three, "start ->
source ready" of the three (ms_h2d: the passes run there) and their differences - the estimate's milliseconds and the denoiser's -, the time
of the estimate's call alone (av1mi_film_grain_estimate, with its allocation), and on the noise clip, whose clean ramps the tool keeps, the
PSNR of the coded source against them before and after the denoiser (the caller's frames, and av1mi_film_grain_denoise's output).  It
reports what it measures, nothing more."""
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


def noisy_ramp_clip(torch, w, h, bd, n, dev, seed=7):
    """n frames of a horizontal luma ramp (black to white, a slow vertical tilt; the operator is blind to both) with Gaussian noise of
    sigma 0.5 + 1.5 luma / white at 8-bit scale, U and V flat with sigma 0.75; a new noise field every frame.  Returns (the clip, the
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
        luma = (level + sigma * torch.randn((h, w), generator=g, device=dev)).round().clamp(0, mx)
        planes = [luma] + [(128.0 * sc + 0.75 * sc * torch.randn((h // 2, w // 2), generator=g, device=dev)).round().clamp(0, mx) for _ in range(2)]
        frames.append(torch.cat([p.to(dt).reshape(-1) for p in planes]))
    return torch.cat(frames).view(torch.uint8), clean.view(torch.uint8)


def psnr(torch, a, b, bd):
    """of two clips in one layout, over every sample"""
    dt = torch.int16 if bd > 8 else torch.uint8
    d = a.view(dt).to(torch.float64) - b.view(dt).to(torch.float64)
    mse = float((d * d).mean())
    return 99.0 if mse == 0 else 10.0 * float(torch.log10(torch.tensor(((1 << bd) - 1) ** 2 / mse)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--clips", default="synth,noise")
    ap.add_argument("--level", type=int, default=20, help="N: the fixed table's level and the estimate's ceiling")
    ap.add_argument("--keyints", default="1,240")
    ap.add_argument("--extra", default="", help="further parameters for every run, name=value,...")
    args = ap.parse_args()
    import torch
    import av1mi
    w, h, bd, n = 1920, 1080, 10, args.frames
    dev = torch.device("cuda:0")
    extra = {k: int(v) for k, v in (kv.split("=") for kv in args.extra.split(",") if kv)}
    with av1mi.Context(0) as ctx:
        for name in args.clips.split(","):
            clip, clean = (bench.make_clip_torch(w, h, bd, n, 1080, dev), None) if name == "synth" else noisy_ramp_clip(torch, w, h, bd, n, dev)
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
                    line["psnr_source_against_clean_before"] = round(psnr(torch, clip, clean, bd), 3)
                    line["psnr_source_against_clean_after"] = round(psnr(torch, out, clean, bd), 3)
                    del out
                print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
