#!/usr/bin/env python3
"""The quality pass A/B: bench.py's synthclip (1080p x 60, 10-bit, CQ 30, the clip in HBM) as
the headline all-key chunk and as cfg3_1080p_ippp.  One JSON line per point:
  fps_on / fps_off      frames/s of the chunk with the context's quality switch on and off, timed alternately (off, on, off, on ...) after
                        --warmup, best of --steps each; off_spread_fps: lowest and highest of the off timings - what a difference has to
                        exceed to mean anything
  ms_pass               the pass alone on the device: the second stream's interval (the report's ms_cdef, device events: CDEF or the
                        squared error, and with the switch on the pass behind it) on minus off, best of each
  ms_quality_call       av1mi_quality alone on two device-resident chunks, with its allocations and copies (host clock around the call)
  gbytes_per_s          the bytes of two chunks over ms_pass
  ssim / psnr           per aq_strength in --strengths at the point's CQ: SSIM Y and all-planes (av1mi_quality_result) beside the report's
                        PSNR Y and bytes per frame
and the bitstream's bytes with the switch on equal to those with it off.  It reports what it measures, nothing more."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "av1-base_amd"))
import bench  # noqa: E402

POINTS = [
    ("headline_cq30", dict(keyint=1, cq_level=30, intra_mode_mask=0x1FFF)),
    ("cfg3_1080p_ippp", dict(keyint=240, cq_level=30, intra_mode_mask=0x7)),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--strengths", default="0,2")
    args = ap.parse_args()
    import torch
    import av1mi
    w, h, bd, n = 1920, 1080, 10, args.frames
    dev = torch.device("cuda:0")
    clip = bench.make_clip_torch(w, h, bd, n, 1080, dev).reshape(-1)
    recon = torch.empty_like(clip)
    torch.cuda.synchronize(dev)
    with av1mi.Context(0) as ctx:

        def run(p, on, **kw):
            ctx.set_quality(on)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            data, _, rep, _ = ctx.encode_chunk(p, clip.data_ptr(), n, on_device=True, **kw)
            return time.perf_counter() - t0, rep, data

        for name, kw in POINTS:
            p = av1mi.default_params(w, h, bd, **kw)
            for _ in range(args.warmup):
                run(p, False, copy_out=False)
                run(p, True, copy_out=False)
            t_off, t_on, s2_off, s2_on = [], [], [], []
            for _ in range(args.steps):
                dt, rep, _ = run(p, False, copy_out=False)
                t_off.append(dt)
                s2_off.append(rep.ms_cdef)
                dt, rep, _ = run(p, True, copy_out=False)
                t_on.append(dt)
                s2_on.append(rep.ms_cdef)
            same = run(p, True)[2] == run(p, False)[2]
            run(p, False, copy_out=False, recon_ptr=recon.data_ptr())
            ctx.quality(p, clip.data_ptr(), recon.data_ptr(), n, on_device=True)
            calls = []
            for _ in range(args.steps):
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                ctx.quality(p, clip.data_ptr(), recon.data_ptr(), n, on_device=True)
                calls.append((time.perf_counter() - t0) * 1e3)
            ms_pass = min(s2_on) - min(s2_off)
            line = {"point": name, "fps_on": round(n / min(t_on), 1), "fps_off": round(n / min(t_off), 1),
                    "off_spread_fps": [round(n / max(t_off), 1), round(n / min(t_off), 1)], "on_spread_fps": [round(n / max(t_on), 1), round(n / min(t_on), 1)],
                    "ms_second_stream_on": round(min(s2_on), 3), "ms_second_stream_off": round(min(s2_off), 3), "ms_pass": round(ms_pass, 3),
                    "ms_quality_call": round(min(calls), 3), "gbytes_per_s": round(2 * clip.numel() / (ms_pass * 1e6), 1) if ms_pass > 0 else None,
                    "bitstream_equal": bool(same), "by_aq_strength": {}}
            for s in [int(x) for x in args.strengths.split(",")]:
                q = av1mi.default_params(w, h, bd, aq_strength=s, **kw)
                _, rep, _ = run(q, True, copy_out=False)
                sums = av1mi.quality_sum(ctx.quality_result(n))
                ss, ps = av1mi.ssim_of(sums), av1mi.psnr_of(sums, w, h, bd, n)
                line["by_aq_strength"][s] = {"bytes_per_frame": round(rep.bytes / n, 1), "psnr_y_report": round(rep.psnr[0], 3), "psnr_y": round(ps["y"], 3),
                                             "ssim_y": round(ss["y"], 5), "ssim_all": round(ss["all"], 5), "ssim_all_db": round(ss["db"], 3)}
            ctx.set_quality(False)
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
