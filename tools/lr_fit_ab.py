#!/usr/bin/env python3
"""Self-guided fit A/B: bench.py's synthclip (1080p x 60, 10-bit) encoded with enable_lr 0 (off), 4 (switchable units on all planes, fixed
candidates), fit | 4 (the self-guided filter fitted per unit over all 16 parameter sets) and fit | 4 with
the mask 1 << 9 (set 9 alone: the fixed candidates' set with fitted weights), and with the Wiener fit (bit 10, item 9e) on 3, on 4 and on
fit | 4, at the headline point (all key frames, CQ 30), IPPP at
CQ 30 and the production point (CQ 8), each at restoration units of 64, 128 and 256 luma samples (--unit-shifts; bits 12-13, item 9f).
One JSON line per point, value and unit size: frames/s (best of --steps after --warmup, the clip in HBM),
milliseconds per frame, bytes per frame, PSNR Y / U / V of the reconstruction, the report's stage times and, with the fit, the
histogram of the units' choices (off / Wiener / fixed / fitted), of the fitted sets and of the fitted weights at their clamps
(av1mi_lr_fit_result) and, with the Wiener fit, the units choosing the fitted filter, those of them with a tap at a clamp and with
different vertical and horizontal taps (av1mi_lr_wiener_fit_result).  With --rd 0,1,2,3 every row with restoration also runs with the
rate term of the unit decisions (bits 14 and 15, item 9g) at those lambda scales; every row with restoration then reports the final
choices - units off / Wiener (fixed or fitted) / fixed self-guided / fitted self-guided - and the units' side information per frame in
bits, the sum of bits16 / 16 (av1mi_lr_rd_result), and the rate term's rows lambda.  It reports what it measures, nothing more."""
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
    ("production_1080p", dict(keyint=240, cq_level=8, intra_mode_mask=0x7, film_grain=20, subpel=1, enable_qm=1, qm_min=1, qm_max=15)),
]
VALUES = {"0": 0, "3": 3, "4": 4, "fit4": 0x104, "fit4_set9": 0x104 | ((1 << 9) << 16), "wfit3": 0x403, "wfit4": 0x404, "wfit_fit4": 0x504}
TAPS_MIN, TAPS_MAX = (-5, -23, -17), (10, 8, 46)


def fit_hist(units):
    """choices, fitted sets and clamped weights of units[frame][plane][row][column][4] over the restored planes"""
    u = units.reshape(-1, 4)
    k = u[:, 0]
    fitted = u[k >= 7]
    sets = {int(t): int((fitted[:, 1] == t).sum()) for t in sorted(set(fitted[:, 1].tolist()))}
    both = fitted[(fitted[:, 1] < 10)]
    return {"units": int(len(u)), "off": int((k == 0).sum()), "wiener": int(((k >= 1) & (k <= 3)).sum()),
            "fixed": int(((k >= 4) & (k <= 6)).sum()), "fitted": int(len(fitted)), "sets": sets,
            "xqd0_at_clamp": int(((both[:, 2] == -96) | (both[:, 2] == 31)).sum()),
            "xqd1_at_clamp": int(((both[:, 3] == -32) | (both[:, 3] == 95)).sum())}


def wfit_hist(units):
    """of units[frame][plane][row][column][8] over the restored planes: present candidates, units choosing the fitted Wiener filter,
    those with a tap at a clamp and those whose vertical and horizontal taps differ"""
    import numpy as np
    u = units.reshape(-1, 8).astype(np.int64)
    won = u[u[:, 0] == 23]
    lo, hi = np.array(TAPS_MIN * 2), np.array(TAPS_MAX * 2)
    return {"present": int((u[:, 1] != 0).sum()), "fitted_wiener": int(len(won)),
            "tap_at_clamp": int(((won[:, 2:] == lo) | (won[:, 2:] == hi)).any(axis=1).sum()),
            "cv_ne_ch": int((won[:, 2:5] != won[:, 5:8]).any(axis=1).sum())}


def rd_hist(choice, bits16, n):
    """final choices of choice[frame][plane][row][column] over all planes (a plane that is not restored counts as off) and the units'
    side information per frame in bits"""
    k = choice.reshape(-1)
    return {"off": int((k == 0).sum()), "wiener": int((((k >= 1) & (k <= 3)) | (k == 23)).sum()), "fixed": int(((k >= 4) & (k <= 6)).sum()),
            "fitted": int(((k >= 7) & (k < 23)).sum()), "unit_bits_per_frame": round(float(bits16.sum()) / 16 / n, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--points", default="", help="comma-separated subset of the point names")
    ap.add_argument("--values", default="0,4,fit4,fit4_set9,3,wfit3,wfit4,wfit_fit4")
    ap.add_argument("--unit-shifts", default="0", help="comma-separated lr_unit_shift values: 0 = units of 64 luma samples, 1 = 128, 2 = 256")
    ap.add_argument("--rd", default="", help="comma-separated lambda scales 0 .. 3: every row with restoration also runs with the rate term at each")
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
            rds = [None] + [int(s) for s in args.rd.split(",") if s != ""]
            for v, shift, rd in ((v, int(s), rd) for v in args.values.split(",") for s in args.unit_shifts.split(",") for rd in rds):
                if (shift or rd is not None) and not VALUES[v]:
                    continue   # a unit size and the rate term need restoration
                p = av1mi.default_params(w, h, bd, enable_lr=VALUES[v], lr_unit_shift=shift, lr_rd=rd, **kw)
                for _ in range(args.warmup):
                    ctx.encode_chunk(p, clip.data_ptr(), n, on_device=True, copy_out=False)
                best, rep = None, None
                for _ in range(args.steps):
                    t0 = time.perf_counter()
                    _, _, r, _ = ctx.encode_chunk(p, clip.data_ptr(), n, on_device=True, copy_out=False)
                    dt = time.perf_counter() - t0
                    if best is None or dt < best:
                        best, rep = dt, r
                line = {"point": name, "enable_lr": v, "unit": 64 << shift, "rd": rd, "fps": round(n / best, 1), "ms": round(best * 1e3, 2), "ms_per_frame": round(best * 1e3 / n, 3),
                        "bytes_per_frame": round(rep.bytes / n, 1), "psnr": [round(x, 3) for x in rep.psnr], "sse": [int(x) for x in rep.sse],
                        "ms_recon": round(rep.ms_recon, 3), "ms_entropy": round(rep.ms_entropy, 3)}
                if VALUES[v] & 0x100:
                    line["fit"] = fit_hist(ctx.lr_fit_result(n)[0])
                if VALUES[v] & 0x400:
                    line["wiener_fit"] = wfit_hist(ctx.lr_wiener_fit_result(n)[0])
                if VALUES[v] and args.rd:
                    choice, bits16, lam = ctx.lr_rd_result(n)
                    line["lambda"] = lam
                    line["choices"] = rd_hist(choice, bits16, n)
                print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
