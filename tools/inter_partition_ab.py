#!/usr/bin/env python3
"""Partition of inter frames A/B: 1080p x 60, 10-bit, IPPP (keyint 240), one chunk, the clip in HBM, coded with
fixed 32x32 and fixed 64x64 leaves, partition_search = 1 with leaves 3..6 and partition_search = 2 with leaves 3..6 and 4..6, and three points
with the sub-sample refinement and the pre-search (so that a run launches every kernel of me_kernel.hip) - on bench.py's
synthclip and on the same clip with, in every 128x128 region, a 48x48 patch that moves by (3, -2) per frame over a background that pans
by (1, 0).  One JSON line per clip and mode: frames/s (best of --steps after --warmup), bytes per frame, PSNR Y / U / V, the report's
chain time (source ready -> last reconstruction: ms_recon) and entropy time, and the histogram of the inter frames' leaf sizes.  With
--kernels each mode is run once more under torch's profiler and the summed device time of the search, decision and chain kernels is
added.  AV1MI_LIB selects another build of the library (the sweep of the penalty's shift: -DAV1MI_PI_K=k builds).  It reports what it
measures, nothing more."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "av1-base_amd"))
import bench  # noqa: E402

MODES = [
    ("fixed32", dict(block_log2=5)),
    ("fixed64", dict(block_log2=6)),
    ("ps1_3..6", dict(block_log2=6, partition_search=1, min_block_log2=3)),
    ("ps2_3..6", dict(block_log2=6, partition_search=2, min_block_log2=3)),
    ("ps2_4..6", dict(block_log2=6, partition_search=2, min_block_log2=4)),
    # the search's other kernels: the refinement, the pre-search (bench.py's cfg3_1080p_ippp_presearch_partition), and
    # node mode with both at the wider range
    ("fixed32_subpel", dict(block_log2=5, subpel=1)),
    ("ps1_3..6_pre", dict(block_log2=6, partition_search=1, min_block_log2=3, me_presearch=1)),
    ("ps2_3..6_pre_r16_subpel", dict(block_log2=6, partition_search=2, min_block_log2=3, me_presearch=1, me_range=16, subpel=1)),
]


def patch_clip(torch, w, h, bd, n, dev):
    """the synthclip's first frame as a background that pans by (1, 0) per frame; in every 128x128 region a 48x48 patch of its own
    texture that moves by (3, -2) per frame and wraps inside its region (80 samples of travel each way: of 59 inter frames three,
    t = 27, 40, 54, jump instead)"""
    assert bd > 8   # bench.make_clip_torch returns bytes: 16-bit little-endian samples above 8 bit, handled as int16 here
    flat = bench.make_clip_torch(w, h, bd, 1, 1080, dev).view(-1).view(torch.int16)
    dt = torch.int16
    y0 = flat[:w * h].view(h, w)
    u0 = flat[w * h:w * h * 5 // 4].view(h // 2, w // 2)
    v0 = flat[w * h * 5 // 4:w * h * 3 // 2].view(h // 2, w // 2)
    g = torch.Generator(device="cpu").manual_seed(48)
    tex = torch.randint(0, 1 << bd, (48, 48), generator=g).to(dev).to(dt)
    frames = []
    for t in range(n):
        y = torch.roll(y0, shifts=t, dims=1).clone()
        u = torch.roll(u0, shifts=t // 2, dims=1)
        v = torch.roll(v0, shifts=t // 2, dims=1)
        for ry in range(0, h - 127, 128):
            for rx in range(0, w - 127, 128):
                px, py = rx + (3 * t) % 80, ry + 80 - (2 * t) % 80   # (wraps inside its region: a jump at t = 27, 54 and at t = 40)
                if py >= ry and py + 48 <= h and px + 48 <= w:
                    y[py:py + 48, px:px + 48] = tex
        frames.append(torch.cat([y.reshape(-1), u.reshape(-1), v.reshape(-1)]))
    return torch.stack(frames).contiguous().view(torch.uint8)


def leaf_hist(masks, w, h, lo, hi, have_mask, frames):
    """leaf counts {8, 16, 32, 64} of the given frames by the library's partition rule (av1mi_node_split), from the masks"""
    hist = {8: 0, 16: 0, 32: 0, 64: 0}

    def walk(mask, sx, sy, ox, oy, bsl):
        n = 1 << bsl
        if sx + ox >= w or sy + oy >= h:
            return
        split = False
        if bsl > 3:
            if sy + oy + n // 2 >= h or sx + ox + n // 2 >= w:
                split = True
            elif bsl <= lo:
                split = False
            elif bsl > hi:
                split = True
            elif have_mask:
                bit = 0 if bsl == 6 else (1 + ((oy >> 5) << 1 | (ox >> 5)) if bsl == 5 else
                                          5 + (((ox >> 4) & 1) | (((oy >> 4) & 1) << 1) | (((ox >> 5) & 1) << 2) | (((oy >> 5) & 1) << 3)))
                split = bool((mask >> bit) & 1)
        if not split:
            hist[n] += 1
            return
        for q in range(4):
            walk(mask, sx, sy, ox + (q & 1) * (n // 2), oy + (q >> 1) * (n // 2), bsl - 1)

    sbr, sbc = (h + 63) // 64, (w + 63) // 64
    for f in frames:
        for r in range(sbr):
            for c in range(sbc):
                walk(int(masks[f][r][c]) if have_mask else 0, 64 * c, 64 * r, 0, 0, 6)
    return hist


def kernel_times(torch, fn):
    """summed device time in ms of the kernels of one call, by family"""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    out = {"search": 0.0, "decision": 0.0, "refine": 0.0, "chain": 0.0}
    for e in prof.key_averages():
        name = e.key
        us = getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0.0)
        if "motion_search" in name or "me64_reduce" in name or "presearch" in name:
            out["search"] += us
        elif "inter_partition" in name:
            out["decision"] += us
        elif "subpel_refine" in name:
            out["refine"] += us
        elif any(k in name for k in ("recon", "deblock", "cdef", "lr_")):
            out["chain"] += us
    return {k: round(v / 1e3, 3) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--clips", default="synth,patch")
    ap.add_argument("--modes", default="", help="comma-separated subset of the mode names")
    ap.add_argument("--kernels", action="store_true", help="one more run per mode under the profiler: kernel times by family")
    args = ap.parse_args()
    import torch
    import av1mi
    w, h, bd, n = 1920, 1080, 10, args.frames
    dev = torch.device("cuda:0")
    want = set(args.modes.split(",")) if args.modes else None
    for clip_name in args.clips.split(","):
        clip = bench.make_clip_torch(w, h, bd, n, 1080, dev) if clip_name == "synth" else patch_clip(torch, w, h, bd, n, dev)
        torch.cuda.synchronize(dev)
        assert clip.dtype == torch.uint8 and clip.numel() == n * (w * h * 3 // 2) * 2, "the encoder reads n frames of 16-bit I420 from this buffer"
        with av1mi.Context(0) as ctx:
            for name, kw in MODES:
                if want and name not in want:
                    continue
                p = av1mi.default_params(w, h, bd, keyint=240, cq_level=30, intra_mode_mask=0x7, **kw)
                for _ in range(args.warmup):
                    ctx.encode_chunk(p, clip.data_ptr(), n, on_device=True, copy_out=False)
                times, rep = [], None
                for _ in range(args.steps):
                    t0 = time.perf_counter()
                    _, _, r, _ = ctx.encode_chunk(p, clip.data_ptr(), n, on_device=True, copy_out=False)
                    times.append(time.perf_counter() - t0)
                    if times[-1] == min(times):
                        rep = r
                res = ctx.inter_partition_result(n) if hasattr(ctx, "inter_partition_result") else None   # (a library from before the accessor: geometry only)
                hist = leaf_hist(res[0] if res else None, w, h, kw.get("min_block_log2", kw["block_log2"]), kw["block_log2"], res is not None, range(1, n))
                line = {"clip": clip_name, "mode": name, "lib": os.path.basename(av1mi.LIB_PATH), "fps": round(n / min(times), 1),
                        "fps_range": [round(n / max(times), 1), round(n / min(times), 1)], "bytes_per_frame": round(rep.bytes / n, 1),
                        "psnr": [round(x, 3) for x in rep.psnr], "ms_recon": round(rep.ms_recon, 3), "ms_entropy": round(rep.ms_entropy, 3),
                        "inter_leaves": hist}
                if args.kernels:
                    line["kernel_ms"] = kernel_times(torch, lambda: ctx.encode_chunk(p, clip.data_ptr(), n, on_device=True, copy_out=False))
                print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
