#!/usr/bin/env python3
"""CDEF strength search A/B: bench.py's synthclip encoded with cdef_search 0 and 4 at three operating points - the headline workload
(1080p x 60, 10-bit, all 13 intra candidates), cfg3_1080p_ippp and the production point (CQ 8, quantiser matrices, film grain,
sub-sample vectors, deblocking, enable_lr 2) - and, for the headline, CQ 8 / 30 / 50.  One JSON line per point: frames/s (best of
--steps after --warmup, the clip in HBM), bytes per frame and PSNR Y / U / V of the reconstruction."""
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
    ("headline_cq8", dict(keyint=1, cq_level=8, intra_mode_mask=0x1FFF)),
    ("headline_cq50", dict(keyint=1, cq_level=50, intra_mode_mask=0x1FFF)),
    ("cfg3_1080p_ippp", dict(keyint=240, cq_level=30, intra_mode_mask=0x7)),
    ("production_1080p", dict(keyint=240, cq_level=8, intra_mode_mask=0x7, film_grain=20, subpel=1, deblock=1, enable_lr=2,
                              enable_qm=1, qm_min=1, qm_max=15)),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--points", default="", help="comma-separated subset of the point names")
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
            for k in (0, 4):
                p = av1mi.default_params(w, h, bd, cdef_search=k, **kw)
                for _ in range(args.warmup):
                    ctx.encode_chunk(p, clip.data_ptr(), n, on_device=True, copy_out=False)
                best = None
                for _ in range(args.steps):
                    t0 = time.perf_counter()
                    _, _, rep, _ = ctx.encode_chunk(p, clip.data_ptr(), n, on_device=True, copy_out=False)
                    dt = time.perf_counter() - t0
                    best = dt if best is None or dt < best else best
                print(json.dumps({"point": name, "cdef_search": k, "fps": round(n / best, 1), "ms": round(best * 1e3, 2),
                                  "bytes_per_frame": round(rep.bytes / n, 1), "psnr": [round(x, 3) for x in rep.psnr],
                                  "ms_recon": round(rep.ms_recon, 3), "ms_cdef": round(rep.ms_cdef, 3)}), flush=True)


if __name__ == "__main__":
    main()
