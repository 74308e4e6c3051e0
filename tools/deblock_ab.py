#!/usr/bin/env python3
"""Deblocking A/B: bench.py's synthclip (1080p x 60, 10-bit) encoded with deblock 0 (off), 1 (one level from the quantiser) and 2 (the
level searched per frame and plane on the GPU) at the headline point (all key frames, CQ 30), IPPP at
CQ 30 and the production point (CQ 8).  One JSON line per point and value: frames/s (best of --steps after --warmup, the clip in
HBM), bytes per frame, PSNR Y / U / V of the reconstruction, the report's stage times, and the histogram of the levels the frames were
deblocked with, per plane and frame kind (av1mi_lf_search_result).  It reports what it measures, nothing more."""
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
    ("production_1080p", dict(keyint=240, cq_level=8, intra_mode_mask=0x7, film_grain=20, subpel=1, enable_lr=2,
                              enable_qm=1, qm_min=1, qm_max=15)),
]


def level_hist(levels, keyint):
    """{frame kind: {plane: {level: frames}}} of levels[frame][4] (luma's two fields are equal: the first stands for both)"""
    out = {}
    for f, lv in enumerate(levels):
        kind = "key" if f % keyint == 0 else "inter"
        for name, v in (("y", lv[0]), ("u", lv[2]), ("v", lv[3])):
            h = out.setdefault(kind, {}).setdefault(name, {})
            h[int(v)] = h.get(int(v), 0) + 1
    return {k: {p: dict(sorted(h.items())) for p, h in v.items()} for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--points", default="", help="comma-separated subset of the point names")
    ap.add_argument("--values", default="0,1,2")
    args = ap.parse_args()
    import torch
    import av1mi
    w, h, bd, n = 1920, 1080, 10, args.frames
    dev = torch.device("cuda:0")
    clip = bench.make_clip_torch(w, h, bd, n, 1080, dev)
    torch.cuda.synchronize(dev)
    want = set(args.points.split(",")) if args.points else None
    with av1mi.Context(0) as ctx:
        for name, kw in POINTS:
            if want and name not in want:
                continue
            for d in [int(x) for x in args.values.split(",")]:
                p = av1mi.default_params(w, h, bd, deblock=d, **kw)
                for _ in range(args.warmup):
                    ctx.encode_chunk(p, clip.data_ptr(), n, on_device=True, copy_out=False)
                best, rep = None, None
                for _ in range(args.steps):
                    t0 = time.perf_counter()
                    _, _, r, _ = ctx.encode_chunk(p, clip.data_ptr(), n, on_device=True, copy_out=False)
                    dt = time.perf_counter() - t0
                    if best is None or dt < best:
                        best, rep = dt, r
                levels, _ = ctx.lf_search_result(n)
                print(json.dumps({"point": name, "deblock": d, "fps": round(n / best, 1), "ms": round(best * 1e3, 2),
                                  "bytes_per_frame": round(rep.bytes / n, 1), "psnr": [round(x, 3) for x in rep.psnr],
                                  "ms_recon": round(rep.ms_recon, 3), "ms_cdef": round(rep.ms_cdef, 3), "ms_entropy": round(rep.ms_entropy, 3),
                                  "levels": level_hist(levels, kw["keyint"])}), flush=True)


if __name__ == "__main__":
    main()
