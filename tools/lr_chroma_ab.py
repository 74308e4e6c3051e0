#!/usr/bin/env python3
"""Chroma loop restoration A/B: bench.py's synthclip encoded with enable_lr 1 against 3 and 2 against 4 at three operating points -
the headline workload (1080p x 60, 10-bit, all key frames, all 13 intra candidates), cfg3_1080p_ippp with restoration and the production
point (CQ 8, quantiser matrices, film grain, sub-sample vectors, deblocking) - on the clip as it is (white noise: restoration has little
to gain) and smoothed (--content smooth: every plane through a 5x5 box filter).  One JSON line per point and value:
frames/s (best of --steps after --warmup, the clip in HBM), bytes per frame and PSNR Y / U / V of the reconstruction."""
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
    ("headline", dict(keyint=1, cq_level=30, intra_mode_mask=0x1FFF), ((1, 3), (2, 4))),
    ("cfg3_1080p_ippp", dict(keyint=240, cq_level=30, intra_mode_mask=0x7), ((1, 3), (2, 4))),
    ("production_1080p", dict(keyint=240, cq_level=8, intra_mode_mask=0x7, film_grain=20, subpel=1, deblock=1, enable_qm=1, qm_min=1,
                              qm_max=15), ((2, 4),)),
]


def smoothed(clip, w, h, bd, n):
    """every plane of every frame through a 5x5 box filter (edges replicated), on the device"""
    import torch
    import torch.nn.functional as F
    v = (clip.view(torch.int16) if bd > 8 else clip).reshape(n, -1)
    out = torch.empty_like(v)
    planes = [(0, w, h), (w * h, w // 2, h // 2), (w * h * 5 // 4, w // 2, h // 2)]
    for f in range(n):
        for off, pw, ph in planes:
            p = v[f, off:off + pw * ph].reshape(1, 1, ph, pw).float()
            q = F.avg_pool2d(F.pad(p, (2, 2, 2, 2), mode="replicate"), 5, stride=1)
            out[f, off:off + pw * ph] = torch.round(q).reshape(-1).to(v.dtype)
    return (out.view(torch.uint8) if bd > 8 else out).reshape(clip.shape)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--content", default="plain,smooth", help="comma-separated: plain (the synthclip), smooth (5x5 box-filtered)")
    ap.add_argument("--points", default="", help="comma-separated subset of the point names")
    args = ap.parse_args()
    import torch
    import av1mi
    w, h, bd, n = 1920, 1080, 10, args.frames
    dev = torch.device("cuda:0")
    plain = bench.make_clip_torch(w, h, bd, n, 1080, dev)
    want = set(args.points.split(",")) if args.points else None
    with av1mi.Context(0) as ctx:
        for content in args.content.split(","):
            clip = plain if content == "plain" else smoothed(plain, w, h, bd, n).contiguous()
            torch.cuda.synchronize(dev)
            for name, kw, pairs in POINTS:
                if want and name not in want:
                    continue
                for pair in pairs:
                    for lr in pair:
                        p = av1mi.default_params(w, h, bd, enable_lr=lr, **kw)
                        for _ in range(args.warmup):
                            ctx.encode_chunk(p, clip.data_ptr(), n, on_device=True, copy_out=False)
                        best = None
                        for _ in range(args.steps):
                            t0 = time.perf_counter()
                            _, _, rep, _ = ctx.encode_chunk(p, clip.data_ptr(), n, on_device=True, copy_out=False)
                            dt = time.perf_counter() - t0
                            best = dt if best is None or dt < best else best
                        print(json.dumps({"content": content, "point": name, "enable_lr": lr, "fps": round(n / best, 1),
                                          "ms": round(best * 1e3, 2), "bytes_per_frame": round(rep.bytes / n, 1),
                                          "psnr": [round(x, 3) for x in rep.psnr]}), flush=True)


if __name__ == "__main__":
    main()
