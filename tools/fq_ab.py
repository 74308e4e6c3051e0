#!/usr/bin/env python3
"""Frame term of the quantiser A/B: 1080p x 60, 10-bit, IPPP (keyint 240), one chunk, the clip in HBM -
bench.py's synthclip and tools/inter_partition_ab.py's moving-patches clip - coded with fq_strength 0, 1, 2 and 4 at CQ 24, 30, 36 and
42, alone or (--tpl N) on top of tpl_strength N.  One JSON line per clip, CQ and strength: frames/s (best of --steps after --warmup) and
the frames/s of the strength-0 runs alternated with them, bytes per frame, PSNR Y / U / V against the source over all frames, "start ->
source ready" (ms_h2d: the look-ahead runs there) of the run and of the alternated off runs, and k_f per frame position.  Then per clip
and strength one line with the figure that says whether the term pays on this encoder: the bytes at the strength-0 run's luma PSNR,
interpolated (log bytes linear in PSNR, tools/tpl_ab.py's) between the strength's four CQ points, over the strength-0 run's bytes - below
1 saves bytes at equal PSNR; null where the PSNR lies outside the strength's points.  It reports what it measures, nothing more."""
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
from aq_ab import ssim_columns  # noqa: E402
from tpl_ab import bytes_at_psnr  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--clips", default="synth,patch")
    ap.add_argument("--cqs", default="24,30,36,42")
    ap.add_argument("--strengths", default="0,1,2,4")
    ap.add_argument("--tpl", type=int, default=0, help="tpl_strength of every run, the off runs included")
    ap.add_argument("--extra", default="", help="further parameters for every run, name=value,...")
    args = ap.parse_args()
    import torch
    import av1mi
    from inter_partition_ab import patch_clip
    w, h, bd, n = 1920, 1080, 10, args.frames
    dev = torch.device("cuda:0")
    extra = {k: int(v) for k, v in (kv.split("=") for kv in args.extra.split(",") if kv)}
    cqs = [int(x) for x in args.cqs.split(",")]
    strengths = [int(x) for x in args.strengths.split(",")]
    with av1mi.Context(0) as ctx:
        for name in args.clips.split(","):
            clip = bench.make_clip_torch(w, h, bd, n, 1080, dev) if name == "synth" else patch_clip(torch, w, h, bd, n, dev)
            torch.cuda.synchronize(dev)
            curve = {s: [] for s in strengths}   # (luma PSNR, bytes) per CQ
            for cq in cqs:
                kw = dict(keyint=240, cq_level=cq, intra_mode_mask=0x7, tpl_strength=args.tpl, **extra)
                off = av1mi.default_params(w, h, bd, **kw)
                for s in strengths:
                    p = av1mi.default_params(w, h, bd, frame_q_strength=s, **kw)
                    for _ in range(args.warmup):
                        ctx.encode_chunk(p, clip.data_ptr(), n, on_device=True, copy_out=False)
                    best, best_off, rep, ready_off = None, None, None, None
                    for _ in range(args.steps):   # alternated: an off run in front of every run
                        t0 = time.perf_counter()
                        _, _, r0, _ = ctx.encode_chunk(off, clip.data_ptr(), n, on_device=True, copy_out=False)
                        dt = time.perf_counter() - t0
                        best_off = dt if best_off is None or dt < best_off else best_off
                        ready_off = r0.ms_h2d if ready_off is None or r0.ms_h2d < ready_off else ready_off
                        t0 = time.perf_counter()
                        _, _, r, _ = ctx.encode_chunk(p, clip.data_ptr(), n, on_device=True, copy_out=False)
                        dt = time.perf_counter() - t0
                        if best is None or dt < best:
                            best, rep = dt, r
                    base = av1mi.cq_to_qindex(cq)
                    k = [(int(q) - base) // 4 for q in ctx.frame_q_result(n)[0]]
                    curve[s].append((rep.psnr[0], rep.bytes))
                    print(json.dumps({"clip": name, "cq": cq, "tpl_strength": args.tpl, "fq_strength": s, "fps": round(n / best, 1),
                                      "fps_off_alternated": round(n / best_off, 1), "bytes_per_frame": round(rep.bytes / n, 1),
                                      "psnr": [round(x, 3) for x in rep.psnr], "ms_start_to_source_ready": round(rep.ms_h2d, 3),
                                      "ms_start_to_source_ready_off": round(ready_off, 3), "k_by_frame": k,
                                      **ssim_columns(av1mi, ctx, p, clip.data_ptr(), n)}), flush=True)
            if 0 in curve:
                for s in strengths:
                    if s == 0:
                        continue
                    ratios = {}
                    for cq, (psnr0, bytes0) in zip(cqs, curve[0]):
                        b = bytes_at_psnr(curve[s], psnr0)
                        ratios[cq] = None if b is None else round(b / bytes0, 4)
                    print(json.dumps({"clip": name, "tpl_strength": args.tpl, "fq_strength": s, "bytes_at_the_off_runs_psnr_over_its_bytes": ratios}), flush=True)


if __name__ == "__main__":
    main()
