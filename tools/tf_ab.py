#!/usr/bin/env python3
"""Temporal filter A/B: the key frames' filter off against tf_frames N in {1, 3, 7} x tf_strength s in {1, 3, 5} on two clips in HBM -
bench.py's 1080p synthclip as one IPPP chunk (10 bit, keyint = the chunk), and a translating pattern with Gaussian noise (1080p, 8 bit,
tests/tf_ref.py's generator).  One JSON line per clip and setting:
  fps / fps_off       frames/s of the chunk with the setting and of the filter off, timed alternately (off, on, off, on ...) in this
                      process after --warmup, best of --steps each; off_spread: lowest and highest of that row's off timings, and the
                      first line of a clip has the spread of all its off timings - what a difference has to exceed to mean anything
  bytes_per_frame, psnr, ssim   PSNR Y / U / V and SSIM Y / all-planes of the returned reconstruction against the ORIGINAL source (and
                      against the clean pattern where there is one), compared on the device (av1mi_quality) - the report's own PSNR is
                      against the filtered key frames
  ms_filter_call      av1mi_temporal_filter alone, with its allocations and copies; ms_copy: a device copy of the chunk, what the
                      filter costs a device-resident chunk before its kernels run
  index_hist, rejected_share   histogram of the weight indices over the samples of all block-followers, and the share of
                      block-followers whose weights are all 0 (tests/tf_ref.py: frame_stats on the library's vectors)
The default stays off whatever this prints; where the filter loses bytes or PSNR the line says so."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "av1-base_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench  # noqa: E402
import tf_ref  # noqa: E402

SETTINGS = [(n, s) for n in (1, 3, 7) for s in (1, 3, 5)]


def against(av1mi, ctx, p, ref, test, w, h, bd, n):
    """(PSNR per plane, [SSIM Y, SSIM all planes]) of chunk `test` against chunk `ref`, two device tensors in the tight layout"""
    s = av1mi.quality_sum(ctx.quality(p, ref.data_ptr(), test.data_ptr(), n, on_device=True))
    ps, ss = av1mi.psnr_of(s, w, h, bd, n), av1mi.ssim_of(s)
    return [round(ps[k], 3) for k in "yuv"], [round(ss["y"], 5), round(ss["all"], 5)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--frames", type=int, default=60, help="frames of the synthclip chunk")
    ap.add_argument("--pattern-frames", type=int, default=16)
    ap.add_argument("--clips", default="synthclip,pattern")
    args = ap.parse_args()
    import torch
    import av1mi
    dev = torch.device("cuda:0")
    w, h = 1920, 1080
    clips = []
    if "synthclip" in args.clips.split(","):
        t = bench.make_clip_torch(w, h, 10, args.frames, 1080, dev)
        clips.append(("synthclip_1080p_ippp", 10, args.frames, t, None, dict(cq_level=30, intra_mode_mask=0x7)))
    if "pattern" in args.clips.split(","):
        noisy, clean = tf_ref.pattern_clip(w, h, 8, args.pattern_frames, seed=7, sigma=2.0)
        t = torch.frombuffer(bytearray(noisy), dtype=torch.uint8).to(dev)
        clips.append(("pattern_noise_1080p", 8, args.pattern_frames, t, torch.frombuffer(bytearray(clean), dtype=torch.uint8).to(dev),
                      dict(cq_level=30, intra_mode_mask=0x7)))
    with av1mi.Context(0) as ctx:
        for name, bd, n, clip, clean, kw in clips:
            clip = clip.reshape(-1)
            src = clip.cpu().numpy().tobytes()
            recon = torch.empty_like(clip)
            scratch = torch.empty_like(clip)

            def run(p, want_recon=False):
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                _, _, rep, _ = ctx.encode_chunk(p, clip.data_ptr(), n, on_device=True, copy_out=False, recon_ptr=recon.data_ptr() if want_recon else None)
                return time.perf_counter() - t0, rep

            def line(p, t_on, t_offs, rep, extra):
                run(p, want_recon=True)
                torch.cuda.synchronize(dev)
                psnr, ssim = against(av1mi, ctx, p, clip, recon, w, h, bd, n)
                d = {"clip": name, "fps": round(n / t_on, 1), "fps_off": round(n / min(t_offs), 1),
                     "off_spread_fps": [round(n / max(t_offs), 1), round(n / min(t_offs), 1)], "bytes_per_frame": round(rep.bytes / n, 1),
                     "psnr": psnr, "ssim": ssim, "psnr_report": [round(x, 3) for x in rep.psnr], "ms_h2d": round(rep.ms_h2d, 3)}
                if clean is not None:
                    d["psnr_clean"], d["ssim_clean"] = against(av1mi, ctx, p, clean, recon, w, h, bd, n)
                d.update(extra)
                print(json.dumps(d), flush=True)
                return d

            p_off = av1mi.default_params(w, h, bd, keyint=n, **kw)
            for _ in range(args.warmup):
                run(p_off)
            all_off = []
            rows = []
            for N, s in SETTINGS:
                p_on = av1mi.default_params(w, h, bd, keyint=n, tf_frames=N, tf_strength=s, **kw)
                for _ in range(args.warmup):
                    run(p_on)
                t_offs, t_ons, rep = [], [], None
                for _ in range(args.steps):
                    t_offs.append(run(p_off)[0])
                    dt, r = run(p_on)
                    t_ons.append(dt)
                    rep = r if dt <= min(t_ons) else rep
                all_off += t_offs
                # the filter alone, the copy it needs, and the weights' statistics from the library's vectors
                ctx.temporal_filter(p_on, clip.data_ptr(), n, on_device=True, out_ptr=scratch.data_ptr(), want_mv=False)
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                _, mv = ctx.temporal_filter(p_on, clip.data_ptr(), n, on_device=True, out_ptr=scratch.data_ptr())
                ms_call = (time.perf_counter() - t0) * 1e3
                t0 = time.perf_counter()
                scratch.copy_(clip)
                torch.cuda.synchronize(dev)
                ms_copy = (time.perf_counter() - t0) * 1e3
                nf = tf_ref.followers(N, n, n, 0)
                fr = tf_ref.split(src[:len(src) // n * (nf + 1)], w, h, bd, nf + 1)
                W, H = (w + 7) & ~7, (h + 7) & ~7
                coded = [[tf_ref.extend(f[0], W, H), tf_ref.extend(f[1], W // 2, H // 2), tf_ref.extend(f[2], W // 2, H // 2)] for f in fr]
                hist, rej = tf_ref.frame_stats(coded[0], coded[1:], mv[0, :nf], W, H, bd, s, 8)
                rows.append((p_on, min(t_ons), t_offs, rep, {"tf_frames": N, "tf_strength": s, "ms_filter_call": round(ms_call, 3), "ms_copy": round(ms_copy, 3),
                                                             "index_hist": [int(v) for v in hist], "rejected_share": round(rej / (nf * mv.shape[2]), 4)}))
            _, rep_off = run(p_off)
            off = line(p_off, min(all_off), all_off, rep_off, {"tf_frames": 0, "tf_strength": 0})
            for p_on, t_on, t_offs, rep, extra in rows:
                d = line(p_on, t_on, t_offs, rep, extra)
                worse = [k for k, v in (("bytes", d["bytes_per_frame"] > off["bytes_per_frame"]), ("psnr_y", d["psnr"][0] < off["psnr"][0])) if v]
                if worse:
                    print(json.dumps({"clip": name, "tf_frames": extra["tf_frames"], "tf_strength": extra["tf_strength"], "loses": worse}), flush=True)


if __name__ == "__main__":
    main()
