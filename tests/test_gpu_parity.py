"""GPU parity tests: the HIP path (through the C ABI) against the CPU oracle and the dav1d-pinned
golden fixtures.  Bit-exact is the bar: identical bitstreams and identical reconstructions."""
import hashlib
import os

import numpy as np
import pytest

from mkv_ref import _ebml

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def raw_of(planes, bd):
    dt = np.uint8 if bd == 8 else np.dtype("<u2")
    return b"".join(p.astype(dt).tobytes() for p in planes)


def sha(planes):
    h = hashlib.sha256()
    for p in planes:
        h.update(np.ascontiguousarray(p.astype("<u2")).tobytes())
    return h.hexdigest()


def split_planes(raw, w, h, bd):
    dt = np.uint8 if bd == 8 else np.dtype("<u2")
    a = np.frombuffer(raw, dtype=dt)
    y = a[:w * h].reshape(h, w)
    u = a[w * h:w * h + w * h // 4].reshape(h // 2, w // 2)
    v = a[w * h + w * h // 4:].reshape(h // 2, w // 2)
    return [y, u, v]


def test_extension_is_the_hip_library(av1mi):
    assert os.path.basename(av1mi.LIB_PATH) == "libav1mi.so"
    import torch
    assert torch.cuda.is_available()


def test_golden_fixtures_through_the_c_abi(av1mi, ctx, oracle, golden_cases):
    """Every fixture the GPU path can express (one-superblock tiles, 8..64 blocks, decision-driven
    modes): same bytes as the committed stream, reconstruction hash == dav1d's."""
    n = 0
    for m in golden_cases:
        cfgk = dict(m["config"])
        min_bs = cfgk.pop("min_bs_log2", 4)
        bs = cfgk.pop("max_bs_log2", min_bs)   # block_log2 = the largest leaf; under partition_search leaves go down to min_block_log2
        qidx = cfgk.get("base_q_idx", 120)
        # what the C ABI cannot express stays with the oracle tests: fuzzed levels / modes, a film-grain seed other than the ABI's
        # rule, tile layouts other than 1x1 / 2x2 superblocks, quantiser indices no CQ level maps to
        if any(k.startswith("fuzz") for k in cfgk) or (cfgk.get("film_grain") and cfgk.get("fg_seed") != 7391) or cfgk.get("tile_w_sb", 1) != 1 or qidx % 4 or qidx > 244:
            continue
        p = av1mi.default_params(m["width"], m["height"], m["bit_depth"], block_log2=bs, cq_level=qidx // 4,
                                 cdf_update=0 if cfgk.get("disable_cdf_update") else 1, enable_cdef=cfgk.get("enable_cdef", 1))
        assert av1mi.cq_to_qindex(qidx // 4) == qidx
        p.intra_mode_mask = cfgk.get("mode_mask", 0)
        p.intra_angle_delta = cfgk.get("angle_delta", 0)
        p.intra_edge_filter = cfgk.get("intra_edge_filter", 0)
        p.cfl = cfgk.get("cfl", 0)
        p.tx_search = cfgk.get("tx_search", 0)
        p.partition_search, p.min_block_log2 = cfgk.get("partition_search", 0), min_bs
        for k in ("color_primaries", "transfer_characteristics", "matrix_coefficients", "color_range"):
            setattr(p, k, cfgk.get(k, 0))
        p.film_grain = cfgk.get("fg_c_scaling", 0)  # table N: scaling 2N / N, seed 7391 for frame 0
        p.enable_lr = cfgk.get("enable_lr", 0)
        if cfgk.get("deblock", 0) == 2:
            continue   # explicit levels: oracle-only test hook
        p.deblock = cfgk.get("deblock", 0)
        if cfgk.get("enable_qm"):
            if cfgk["qm_y"] != cfgk["qm_uv"]:
                continue   # the HIP path derives one level for all planes
            p.enable_qm, p.qm_min, p.qm_max = 1, cfgk["qm_y"], cfgk["qm_y"]   # min == max: that level at any quantiser
        for k in ("cdef_y_pri", "cdef_y_sec", "cdef_uv_pri", "cdef_uv_sec", "cdef_damping"):
            if k in cfgk:
                setattr(p, k, cfgk[k])
        src = [(pl >> m.get("src_shift", 0)) << m.get("src_shift", 0) for pl in oracle.synthclip_frame(m["width"], m["height"], m["bit_depth"], seed=m["seed"], t=m["t"])]
        data, sizes, rep, recon = ctx.encode_chunk(p, raw_of(src, m["bit_depth"]), 1, want_recon=True)
        assert data == m["obu"], m["name"]
        assert sha(split_planes(recon.tobytes(), m["width"], m["height"], m["bit_depth"])) == m["recon_sha256"], m["name"]
        n += 1
    assert n >= 10


@pytest.mark.parametrize("w,h,bd,n,bs,cdf", [
    (64, 64, 8, 1, 5, 1), (64, 64, 10, 3, 4, 1), (8, 8, 8, 2, 5, 1), (72, 56, 8, 2, 3, 1), (200, 120, 8, 4, 5, 0),
    (328, 248, 10, 2, 5, 1), (136, 136, 8, 3, 4, 1), (640, 360, 8, 2, 5, 1),
    # widths whose remainder modulo 64 mixes block sizes side by side (24 = 16 + 8, 40, 48, 56): regression for the
    # level-buffer layout, which let horizontally adjacent blocks of different sizes overlap
    (216, 72, 8, 1, 5, 1), (232, 120, 10, 2, 5, 1), (248, 88, 8, 1, 4, 1), (120, 184, 8, 2, 5, 0),
    # 64x64 leaf blocks (64-point luma transforms, 32x32 chroma): whole superblocks, edge superblocks that split to smaller
    # leaves, leaves that overhang the frame (remainders 40..56), static CDFs
    (64, 64, 8, 1, 6, 1), (200, 120, 8, 2, 6, 1), (184, 176, 10, 2, 6, 1), (328, 248, 10, 2, 6, 0), (648, 360, 8, 2, 6, 1)])
def test_chunk_bitstream_and_recon_equal_oracle(av1mi, ctx, oracle, w, h, bd, n, bs, cdf):
    frames = [oracle.synthclip_frame(w, h, bd, seed=1000 + w, t=t, scene_len=2) for t in range(n)]
    p = av1mi.default_params(w, h, bd, block_log2=bs, cdf_update=cdf)
    data, sizes, rep, recon = ctx.encode_chunk(p, b"".join(raw_of(f, bd) for f in frames), n, want_recon=True)
    cfg = oracle.default_config(w, h, bd, min_bs_log2=bs, max_bs_log2=bs, disable_cdf_update=0 if cdf else 1)
    ref, refrec, sse, nsym = b"", b"", [0, 0, 0], 0
    for i, f in enumerate(frames):
        tu, rec, st = oracle.encode_frame(cfg, f)
        assert sizes[i] == len(tu)
        ref += tu
        refrec += raw_of(rec, bd)
        nsym += st.n_symbols
        for k in range(3):
            sse[k] += st.sse[k]
    assert data == ref
    assert recon.tobytes() == refrec
    assert [int(x) for x in rep.sse] == sse          # SSE kernel vs oracle, exact integers
    assert rep.n_symbols == nsym and rep.frames == n and rep.bytes == len(ref)


def test_edge_cases_flat_and_extreme_inputs(av1mi, ctx, oracle):
    """all-skip (flat mid-grey), saturated black/white, and a checkerboard at full amplitude"""
    w, h = 136, 72
    cases = []
    for val in (128, 0, 255):
        cases.append([np.full((h, w), val, np.uint16), np.full((h // 2, w // 2), val, np.uint16), np.full((h // 2, w // 2), val, np.uint16)])
    yy, xx = np.mgrid[0:h, 0:w]
    cb = (((yy // 4 + xx // 4) & 1) * 255).astype(np.uint16)
    cases.append([cb, cb[::2, ::2].copy(), 255 - cb[::2, ::2]])
    p = av1mi.default_params(w, h, 8, block_log2=4)
    cfg = oracle.default_config(w, h, 8, min_bs_log2=4, max_bs_log2=4)
    for planes in cases:
        data, sizes, rep, recon = ctx.encode_chunk(p, raw_of(planes, 8), 1, want_recon=True)
        tu, rec, st = oracle.encode_frame(cfg, planes)
        assert data == tu and recon.tobytes() == raw_of(rec, 8)


def test_full_size_properties_1080p(av1mi, ctx, oracle, monkeypatch):
    """At BASELINE's full frame size the oracle is still used for one frame (seconds), plus
    size-independent properties on a 6-frame chunk: per-frame independence (chunk == concatenation of
    single-frame encodes), determinism, the checksum of the frame sizes, and the same bytes from either form of the range coder."""
    w, h, bd = 1920, 1080, 10
    frames = [oracle.synthclip_frame(w, h, bd, seed=1080, t=t) for t in range(6)]
    raws = [raw_of(f, bd) for f in frames]
    p = av1mi.default_params(w, h, bd)
    data, sizes, rep, _ = ctx.encode_chunk(p, b"".join(raws), 6)
    data2, sizes2, _, _ = ctx.encode_chunk(p, b"".join(raws), 6)
    assert data == data2 and sizes == sizes2 and sum(sizes) == len(data)
    for form in ("2", "4"):
        monkeypatch.setenv("AV1MI_RC_STAGES", form)
        data3, sizes3, _, _ = ctx.encode_chunk(p, b"".join(raws), 6)
        assert data == data3 and sizes == sizes3, form
    monkeypatch.delenv("AV1MI_RC_STAGES")
    for i in (0, 5):
        one, s1, _, _ = ctx.encode_chunk(p, raws[i], 1)
        start = sum(sizes[:i])
        assert data[start:start + sizes[i]] == one
    tu, rec, st = oracle.encode_frame(oracle.default_config(w, h, bd, min_bs_log2=5, max_bs_log2=5), frames[0])
    assert data[:sizes[0]] == tu
    assert 33.0 < rep.psnr[0] < 37.0


def test_range_coder_forms_and_tile_orders_in_rounds(av1mi, ctx, oracle, monkeypatch):
    """More range-coder workgroups than CUs (1080p x 34 all-key frames = 271 groups of 64 tiles): the four-stage form then runs in rounds
    over tiles sorted by length (tile_order_kernel), the two-stage form has everything resident - and either form in either order
    must give the bytes of the default choice; the first frame is checked against the oracle."""
    w, h, bd, n = 1920, 1080, 8, 34
    f0 = oracle.synthclip_frame(w, h, bd, seed=77, t=0)
    frames = [f0] + [oracle.synthclip_frame(w, h, bd, seed=77, t=t) for t in range(1, 4)]
    raw = b"".join(raw_of(frames[t % 4], bd) for t in range(n))
    p = av1mi.default_params(w, h, bd)
    for k in ("AV1MI_RC_STAGES", "AV1MI_RC_SORT"):
        monkeypatch.delenv(k, raising=False)
    data, sizes, rep, _ = ctx.encode_chunk(p, raw, n)
    for env in ({"AV1MI_RC_STAGES": "4"}, {"AV1MI_RC_STAGES": "2", "AV1MI_RC_SORT": "1"}, {"AV1MI_RC_STAGES": "4", "AV1MI_RC_SORT": "0"}):
        for k in ("AV1MI_RC_STAGES", "AV1MI_RC_SORT"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        d2, s2, _, _ = ctx.encode_chunk(p, raw, n)
        assert d2 == data and list(s2) == list(sizes), env
    for k in ("AV1MI_RC_STAGES", "AV1MI_RC_SORT"):
        monkeypatch.delenv(k, raising=False)
    tu, _, _ = oracle.encode_frame(oracle.default_config(w, h, bd, min_bs_log2=5, max_bs_log2=5), f0)
    assert data[:sizes[0]] == tu and data[sum(sizes[:4]):sum(sizes[:5])] == tu   # (frame 4 repeats frame 0)


def test_device_resident_input_matches_host_input(av1mi, ctx, oracle):
    import torch
    w, h, bd, n = 200, 120, 8, 3
    raw = b"".join(raw_of(oracle.synthclip_frame(w, h, bd, seed=5, t=t), bd) for t in range(n))
    p = av1mi.default_params(w, h, bd)
    a = ctx.encode_chunk(p, raw, n)[0]
    d = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()   # the encoder runs on its own non-blocking stream
    b = ctx.encode_chunk(p, d.data_ptr(), n, on_device=True)[0]
    assert a == b


def test_output_blocks_are_recycled_and_bitstreams_stay_exact(av1mi, ctx, oracle):
    """av1mi_buf.data is a page-locked block of the library's pool (the device -> host copy lands in it directly); av1mi_free() puts
    it back and the next chunk gets the same block.  Two buffers held at once are distinct, a smaller chunk after a larger one
    fits the recycled block, and every bitstream equals the oracle's."""
    import ctypes as C
    w, h, bd = 200, 120, 8
    cfg = oracle.default_config(w, h, bd, min_bs_log2=5, max_bs_log2=5)
    frames = [oracle.synthclip_frame(w, h, bd, seed=9, t=t) for t in range(3)]
    want = [oracle.encode_frame(cfg, f)[0] for f in frames]
    p = av1mi.default_params(w, h, bd)

    def raw_call(n):
        out, sizes, rep = av1mi.Buf(), (C.c_uint32 * n)(), av1mi.Report()
        raw = np.frombuffer(b"".join(raw_of(f, bd) for f in frames[:n]), dtype=np.uint8)
        rc = av1mi._lib.av1mi_encode_chunk(ctx._h, C.byref(p), raw.ctypes.data_as(C.c_void_p), n, 0, C.byref(out), sizes, None, C.byref(rep))
        assert rc == 0
        return out

    av1mi._lib.av1mi_release_caches()                 # blocks earlier tests put back: the pool starts empty
    a = raw_call(3)
    b = raw_call(3)                                   # a is still held: b must be another block
    pa, pb = C.cast(a.data, C.c_void_p).value, C.cast(b.data, C.c_void_p).value
    assert pa != pb
    assert C.string_at(a.data, a.size) == b"".join(want) == C.string_at(b.data, b.size)
    av1mi._lib.av1mi_free(a.data)
    av1mi._lib.av1mi_free(b.data)
    c = raw_call(1)                                   # smaller chunk: one of the two blocks comes back
    pc = C.cast(c.data, C.c_void_p).value
    assert pc in (pa, pb)
    assert C.string_at(c.data, c.size) == want[0]
    av1mi._lib.av1mi_free(c.data)


def test_encode_file_y4m_to_ivf(av1mi, oracle, tmp_path):
    """The run_av1an drop-in: Y4M in, IVF out (atomic), frames in order across chunk boundaries."""
    w, h, n = 136, 72, 7
    frames = [oracle.synthclip_frame(w, h, 8, seed=77, t=t) for t in range(n)]
    y4m = tmp_path / "clip.y4m"
    with open(y4m, "wb") as f:
        f.write(b"YUV4MPEG2 W%d H%d F30:1 Ip A1:1 C420jpeg\n" % (w, h))
        for fr in frames:
            f.write(b"FRAME\n" + raw_of(fr, 8))
    out = tmp_path / "clip.ivf"
    seen = []
    rep = av1mi.run_mi355x(av1mi.EncodeParams(y4m, out, tmp_path, av1mi.derive_plan(8), chunk_frames=3),
                           progress=lambda d, t, fps, b: seen.append(d))
    blob = out.read_bytes()
    assert blob[:4] == b"DKIF" and blob[8:12] == b"AV01" and int.from_bytes(blob[24:28], "little") == n
    cfg = oracle.default_config(w, h, 8, min_bs_log2=5, max_bs_log2=5)
    pos = 32
    for i, fr in enumerate(frames):
        sz = int.from_bytes(blob[pos:pos + 4], "little")
        assert int.from_bytes(blob[pos + 4:pos + 12], "little") == i
        tu, _, _ = oracle.encode_frame(cfg, fr)
        assert blob[pos + 12:pos + 12 + sz] == tu
        pos += 12 + sz
    assert pos == len(blob) and rep.frames == n and seen and seen[-1] == n
    assert not list(tmp_path.glob("*.tmp*"))


def test_encode_file_at_the_reference_operating_point(av1mi, oracle, tmp_path):
    """The drop-in with the reference's SVT_PARAMS (av1an.rs:14: --crf 8 --film-grain 20 --enable-qm 1 --qm-min 1 --qm-max 15
    --keyint 240) plus the tools SVT-AV1 has on at preset 3 (sub-sample motion, deblocking, restoration), 10-bit as the
    reference's pix-format: several IPPP chunks through the worker pool, every temporal unit equal to the oracle's."""
    w, h, bd, n, cf = 200, 120, 10, 10, 4
    frames = [oracle.synthclip_frame(w, h, bd, seed=88, t=t) for t in range(n)]
    y4m = tmp_path / "clip.y4m"
    with open(y4m, "wb") as f:
        f.write(b"YUV4MPEG2 W%d H%d F30:1 Ip A1:1 C420p10\n" % (w, h))
        for fr in frames:
            f.write(b"FRAME\n" + raw_of(fr, bd))
    out = tmp_path / "clip.obu"
    rep = av1mi.run_mi355x(av1mi.EncodeParams(y4m, out, tmp_path, av1mi.derive_plan(8), cq_level=8, chunk_frames=cf, keyint=240, film_grain=20,
                                              enable_qm=1, qm_min=1, qm_max=15, subpel=1, deblock=1, enable_lr=2))
    qidx = av1mi.cq_to_qindex(8)
    lvl = oracle.qm_level(qidx, 1, 15)
    ref_stream = b""
    for c0 in range(0, n, cf):
        ref = prev = None
        for t in range(c0, min(n, c0 + cf)):
            cfg = oracle.default_config(w, h, bd, min_bs_log2=5, max_bs_log2=5, base_q_idx=qidx, subpel=1, deblock=1, enable_lr=2,
                                        enable_qm=1, qm_y=lvl, qm_uv=lvl, film_grain=1, fg_y_scaling=40, fg_c_scaling=20,
                                        fg_seed=(7391 + 173 * t) & 0xFFFF)
            tu, rec, _ = oracle.encode_frame(cfg, frames[t], with_seq_hdr=(t == c0), ref=ref, prev_src=prev)
            ref_stream += tu
            ref, prev = rec, frames[t]
    assert out.read_bytes() == ref_stream
    assert rep.frames == n and rep.chunks == 3


def test_stress_carries_and_long_tiles(av1mi, ctx, oracle):
    """High-rate content (uniform noise, low CQ) makes long tiles, many output bytes, 0xFF runs and
    carries that ripple into words already stored - the paths of the range-coding kernel that ordinary
    content rarely takes.  Bit-exact against the oracle on every frame."""
    rng = np.random.default_rng(99)
    w, h, n = 328, 248, 6
    frames = []
    for t in range(n):
        y = rng.integers(0, 256, (h, w)).astype(np.uint16)
        u = rng.integers(0, 256, (h // 2, w // 2)).astype(np.uint16)
        v = rng.integers(0, 256, (h // 2, w // 2)).astype(np.uint16)
        frames.append([y, u, v])
    for cq, bs in ((4, 5), (12, 4), (20, 3)):
        p = av1mi.default_params(w, h, 8, cq_level=cq, block_log2=bs)
        data, sizes, rep, recon = ctx.encode_chunk(p, b"".join(raw_of(f, 8) for f in frames), n, want_recon=True)
        cfg = oracle.default_config(w, h, 8, min_bs_log2=bs, max_bs_log2=bs, base_q_idx=av1mi.cq_to_qindex(cq))
        off = 0
        for i, f in enumerate(frames):
            tu, rec, st = oracle.encode_frame(cfg, f)
            assert data[off:off + sizes[i]] == tu, (cq, bs, i)
            off += sizes[i]
        assert rep.max_tile_symbols > 3000
        if cq == 4:  # 64x64 tiles of noise at CQ 4 outgrow the x1 capacities: the re-run path was taken
            assert rep.max_tile_symbols > 16384 and rep.cap_scale > 1


def test_bitstream_slots_beyond_4_gb(av1mi, monkeypatch):
    """A long chunk at a raised capacity multiplier has more than 4 GB of per-tile bitstream slots (1080p: 510 tiles x 4096 x scale
    entries x 2 bytes per frame - 136 frames at scale 8): the range coder addresses a tile's slot with a 64-bit base, so such a chunk
    encodes, and to the same bytes as at scale 1.  (AV1MI_CAP_SCALE is the context's starting multiplier: what content that
    overflows the x1 capacities - test_stress_carries_and_long_tiles - raises it to.)"""
    import sys
    import torch
    sys.path.insert(0, ROOT)
    import bench
    w, h, n = 1920, 1080, 136
    base = bench.make_clip_torch(w, h, 8, 8, 77, torch.device("cuda", 0))   # 8 distinct frames, repeated
    clip = base.repeat(n // 8, 1).contiguous()
    torch.cuda.synchronize()
    p = av1mi.default_params(w, h, 8)
    with av1mi.Context(0) as c1:
        d1, s1, r1, _ = c1.encode_chunk(p, clip.data_ptr(), n, on_device=True)
    monkeypatch.setenv("AV1MI_CAP_SCALE", "8")
    with av1mi.Context(0) as c8:
        d8, s8, r8, _ = c8.encode_chunk(p, clip.data_ptr(), n, on_device=True)
    assert r1.cap_scale == 1 and r8.cap_scale == 8
    assert n * 510 * 4096 * 8 * 2 > 1 << 32
    assert list(s1) == list(s8) and d1 == d8


@pytest.mark.parametrize("w,h,bd,n,lo,hi,keyint,extra", [
    (648, 360, 8, 2, 3, 5, 1, dict()), (648, 360, 10, 3, 3, 6, 2, dict(intra_mode_mask=0x1FFF)), (328, 248, 8, 4, 4, 5, 240, dict(subpel=1, deblock=1)),
    (392, 264, 10, 3, 3, 6, 240, dict(enable_lr=2, me_range=16)), (202, 122, 8, 3, 3, 6, 3, dict(cfl=1, intra_edge_filter=1, intra_mode_mask=0x1FFF, intra_angle_delta=1))])
def test_content_driven_partition_equals_oracle(av1mi, ctx, oracle, w, h, bd, n, lo, hi, keyint, extra):
    """partition_search: the split masks come from the GPU's pass over the source (partition_kernel), every kernel that walks blocks -
    reconstruction, motion search and refinement, symbolize - follows them; bitstream and reconstruction equal the oracle's, whose rule
    (partition_wants_split) reads the same source, and more than one block size occurs."""
    frames = [oracle.synthclip_frame(w, h, bd, seed=117, t=t) for t in range(n)]
    p = av1mi.default_params(w, h, bd, block_log2=hi, keyint=keyint, partition_search=1, min_block_log2=lo, **extra)
    data, sizes, rep, recon = ctx.encode_chunk(p, b"".join(raw_of(f, bd) for f in frames), n, want_recon=True)
    okw = dict(min_bs_log2=lo, max_bs_log2=hi, partition_search=1)
    for k, v in extra.items():
        okw[{"intra_mode_mask": "mode_mask", "intra_angle_delta": "angle_delta"}.get(k, k)] = v
    cfg = oracle.default_config(w, h, bd, **okw)
    tus, recs = oracle_chunk(oracle, cfg, frames, keyint)
    assert data == b"".join(tus) and [len(t) for t in tus] == list(sizes)
    assert recon.tobytes() == b"".join(raw_of(r, bd) for r in recs)
    _, _, st = oracle.encode_frame(cfg, frames[0])
    assert sum(1 for k in (3, 4, 5, 6) if st.bs_hist[k]) >= 2, list(st.bs_hist)


@pytest.mark.parametrize("w,h,bd,n,bs,me,step,extra", [
    (648, 360, 8, 3, 5, 8, 12, dict()), (392, 264, 10, 3, 6, 16, 20, dict(subpel=1)), (328, 248, 8, 4, 5, 8, 7, dict(partition_search=1, min_block_log2=3, deblock=1)),
    (202, 122, 8, 3, 4, 8, 12, dict())])
def test_hierarchical_motion_search_equals_oracle(av1mi, ctx, oracle, w, h, bd, n, bs, me, step, extra):
    """me_presearch: quarter-resolution luma + a +-64 pre-search per superblock on the GPU give the centres the full search runs around;
    on a clip that moves (2 step, step) samples per frame - beyond the one-level search's reach - bitstream and reconstruction equal the
    oracle's (presearch_centres), and the hierarchy pays: fewer bytes than the one-level search of the same range."""
    frames = [oracle.synthclip_frame(w, h, bd, seed=120, t=t * step) for t in range(n)]
    raw = b"".join(raw_of(f, bd) for f in frames)
    p = av1mi.default_params(w, h, bd, block_log2=bs, keyint=240, me_range=me, me_presearch=1, **extra)
    data, sizes, rep, recon = ctx.encode_chunk(p, raw, n, want_recon=True)
    okw = dict(min_bs_log2=extra.get("min_block_log2", bs), max_bs_log2=bs, me_range=me, me_presearch=1)
    for k, v in extra.items():
        if k != "min_block_log2":
            okw[k] = v
    cfg = oracle.default_config(w, h, bd, **okw)
    tus, recs = oracle_chunk(oracle, cfg, frames, 240)
    assert data == b"".join(tus) and recon.tobytes() == b"".join(raw_of(r, bd) for r in recs)
    if w >= 600:   # (on the small clips the pre-search has little to find: a handful of superblocks)
        p.me_presearch = 0
        flat, _, _, _ = ctx.encode_chunk(p, raw, n)
        assert len(data) < len(flat)


def test_film_grain_table_in_frame_headers(av1mi, ctx, oracle):
    """`film_grain = N` (the reference's `--film-grain N`, av1an.rs:14): every frame header carries a
    film-grain table with its own grain_seed; tile data and reconstruction are untouched.  Bit-exact
    against the oracle writing the same table (the syntax itself is pinned by dav1d, tests/test_oracle.py)."""
    w, h, n = 200, 120, 3
    frames = [oracle.synthclip_frame(w, h, 10, seed=4, t=t) for t in range(n)]
    raw = b"".join(raw_of(f, 10) for f in frames)
    p0 = av1mi.default_params(w, h, 10)
    d0, s0, _, _ = ctx.encode_chunk(p0, raw, n)
    p = av1mi.default_params(w, h, 10)
    p.film_grain, p.first_frame = 20, 7
    d, s, rep, _ = ctx.encode_chunk(p, raw, n)
    cfg = oracle.default_config(w, h, 10, min_bs_log2=5, max_bs_log2=5)
    cfg.film_grain, cfg.fg_y_scaling, cfg.fg_c_scaling = 1, 40, 20
    off = 0
    for i, f in enumerate(frames):
        cfg.fg_seed = (7391 + 173 * (7 + i)) & 0xFFFF
        tu, _, _ = oracle.encode_frame(cfg, f)
        assert d[off:off + s[i]] == tu, i
        off += s[i]
    assert len(d) > len(d0) and list(s) != list(s0)


def oracle_chunk(oracle, cfg, frames, keyint):
    """The oracle's restatement of a chunk: key frame every `keyint` frames, P frames from the previous reconstruction."""
    tus, recs, ref, prev = [], [], None, None
    for t, f in enumerate(frames):
        key = t % keyint == 0
        tu, rec, st = oracle.encode_frame(cfg, f, with_seq_hdr=key, ref=None if key else ref, prev_src=None if key else prev)
        tus.append(tu)
        recs.append(rec)
        ref, prev = rec, f
    return tus, recs


@pytest.mark.parametrize("w,h,bd,n,bs,keyint,me,cdf", [
    (64, 64, 8, 3, 5, 8, 8, 1), (200, 120, 8, 5, 5, 4, 8, 1), (200, 120, 10, 4, 4, 240, 8, 1), (136, 136, 8, 3, 3, 3, 8, 1),
    (328, 248, 10, 3, 5, 240, 16, 1), (72, 56, 8, 4, 4, 2, 16, 0), (648, 360, 8, 3, 5, 240, 8, 1),
    # 64x64 leaves: the search sums four 32x32 cells per candidate, motion compensation and the candidate list at 64x64
    (200, 120, 8, 4, 6, 240, 8, 1), (328, 248, 10, 3, 6, 240, 16, 1), (184, 248, 8, 3, 6, 2, 8, 0), (648, 360, 10, 3, 6, 240, 8, 1)])
def test_inter_chunk_bitstream_and_recon_equal_oracle(av1mi, ctx, oracle, w, h, bd, n, bs, keyint, me, cdf):
    """keyint > 1: P frames (motion search, motion compensation, inter syntax incl. the motion-vector candidate
    list) - every temporal unit and every reconstructed frame bit-exact against the oracle."""
    frames = [oracle.synthclip_frame(w, h, bd, seed=500 + w, t=t) for t in range(n)]
    p = av1mi.default_params(w, h, bd, block_log2=bs, cdf_update=cdf, keyint=keyint, me_range=me)
    data, sizes, rep, recon = ctx.encode_chunk(p, b"".join(raw_of(f, bd) for f in frames), n, want_recon=True)
    cfg = oracle.default_config(w, h, bd, min_bs_log2=bs, max_bs_log2=bs, disable_cdf_update=0 if cdf else 1, me_range=me)
    tus, recs = oracle_chunk(oracle, cfg, frames, keyint)
    assert list(sizes) == [len(t) for t in tus]
    off = 0
    for i, tu in enumerate(tus):
        assert data[off:off + sizes[i]] == tu, "frame %d" % i
        off += sizes[i]
    fb = w * h * 3 // 2 * (2 if bd > 8 else 1)
    rb = recon.tobytes()
    for i, rec in enumerate(recs):
        assert rb[i * fb:(i + 1) * fb] == raw_of(rec, bd), "reconstruction of frame %d" % i


@pytest.mark.parametrize("w,h,bd,n,group,extra", [(200, 120, 8, 7, 2, dict()), (328, 248, 10, 5, 1, dict(enable_lr=2, deblock=1)), (136, 136, 8, 6, 4, dict(subpel=1, keyint=3))])
def test_entropy_coding_in_groups_beside_the_chain(av1mi, oracle, monkeypatch, w, h, bd, n, group, extra):
    """Inter chunks entropy-code finished groups of frames on a third stream while the chain reconstructs the next ones
    (production chunks: groups of >= 8 frames).  Forced to small groups here: streams and reconstructions must not depend on
    the grouping - bit-exact against the oracle, and equal to the ungrouped run."""
    frames = [oracle.synthclip_frame(w, h, bd, seed=600 + w, t=t) for t in range(n)]
    raw = b"".join(raw_of(f, bd) for f in frames)
    keyint = extra.pop("keyint", 240)
    p = av1mi.default_params(w, h, bd, keyint=keyint, **extra)
    outs = []
    for group_env in (str(group), "0"):
        monkeypatch.setenv("AV1MI_ENTROPY_GROUP", group_env)
        with av1mi.Context(0) as c:
            data, sizes, rep, recon = c.encode_chunk(p, raw, n, want_recon=True)
        outs.append((data, list(sizes), recon.tobytes()))
    assert outs[0] == outs[1]
    cfg = oracle.default_config(w, h, bd, min_bs_log2=5, max_bs_log2=5, enable_lr=extra.get("enable_lr", 0), deblock=extra.get("deblock", 0), subpel=extra.get("subpel", 0))
    tus, recs = oracle_chunk(oracle, cfg, frames, keyint)
    assert outs[0][0] == b"".join(tus) and outs[0][2] == b"".join(raw_of(r, bd) for r in recs)


def test_alternative_schedules_give_the_same_bytes(av1mi, oracle, monkeypatch):
    """The range coder's two forms on the all-key-frame path (the launcher picks one by the number of workgroups; forced here) change
    how tiles are coded, never what they code: the default's stream and reconstruction."""
    w, h, bd, n = 328, 248, 10, 7
    frames = [oracle.synthclip_frame(w, h, bd, seed=610, t=t) for t in range(n)]
    raw = b"".join(raw_of(f, bd) for f in frames)
    p = av1mi.default_params(w, h, bd, deblock=1, cdef_y_sec=1, cdef_uv_sec=2)
    outs = []
    for env in ({}, {"AV1MI_RC_STAGES": "2"}, {"AV1MI_RC_STAGES": "4"}):
        monkeypatch.delenv("AV1MI_RC_STAGES", raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        with av1mi.Context(0) as c:
            data, sizes, rep, recon = c.encode_chunk(p, raw, n, want_recon=True)
        outs.append((data, list(sizes), recon.tobytes()))
    assert all(o == outs[0] for o in outs)
    cfg = oracle.default_config(w, h, bd, min_bs_log2=5, max_bs_log2=5, deblock=1, cdef_y_sec=1, cdef_uv_sec=2)
    tus, recs = oracle_chunk(oracle, cfg, frames, 1)
    assert outs[0][0] == b"".join(tus) and outs[0][2] == b"".join(raw_of(r, bd) for r in recs)


def _set_rc_env(monkeypatch, env):
    for k in ("AV1MI_RC_STAGES", "AV1MI_RC_SORT", "AV1MI_ENTROPY_GROUP"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _oracle_tus(oracle, frames, w, h, bd, keyint, fg=0, **kw):
    """the oracle's temporal units of a chunk whose first frame is frame 0 of the clip; fg = N: the film-grain table of --film-grain N
    with the ABI's grain_seed per frame"""
    tus, ref, prev = [], None, None
    for t, f in enumerate(frames):
        key = t % keyint == 0
        if fg:
            kw.update(film_grain=1, fg_y_scaling=2 * fg, fg_c_scaling=fg, fg_seed=(7391 + 173 * t) & 0xFFFF)
        tu, rec, _ = oracle.encode_frame(oracle.default_config(w, h, bd, **kw), f, with_seq_hdr=key, ref=None if key else ref,
                                         prev_src=None if key else prev)
        tus.append(tu)
        ref, prev = rec, f
    return tus


def test_stress_carries_and_long_tiles_under_both_range_coder_forms(av1mi, oracle, monkeypatch):
    """The noise content of test_stress_carries_and_long_tiles through each form of the range coder, forced, with the tiles in the
    order of decreasing length: every frame equals the oracle, and each fresh context takes the capacity re-run path at CQ 4"""
    rng = np.random.default_rng(99)
    w, h, n = 328, 248, 6
    frames = [[rng.integers(0, 256, (h, w)).astype(np.uint16), rng.integers(0, 256, (h // 2, w // 2)).astype(np.uint16),
               rng.integers(0, 256, (h // 2, w // 2)).astype(np.uint16)] for _ in range(n)]
    raw = b"".join(raw_of(f, 8) for f in frames)
    confs = ((4, 5), (12, 4), (20, 3))
    refs = {}
    for cq, bs in confs:
        cfg = oracle.default_config(w, h, 8, min_bs_log2=bs, max_bs_log2=bs, base_q_idx=av1mi.cq_to_qindex(cq))
        refs[cq] = [oracle.encode_frame(cfg, f)[0] for f in frames]
    for form in ("2", "4"):
        _set_rc_env(monkeypatch, {"AV1MI_RC_STAGES": form, "AV1MI_RC_SORT": "1"})
        with av1mi.Context(0) as c:
            for cq, bs in confs:
                data, sizes, rep, _ = c.encode_chunk(av1mi.default_params(w, h, 8, cq_level=cq, block_log2=bs), raw, n)
                assert list(sizes) == [len(t) for t in refs[cq]], (form, cq)
                assert data == b"".join(refs[cq]), (form, cq)
                if cq == 4:
                    assert rep.max_tile_symbols > 16384 and rep.cap_scale > 1, form
    _set_rc_env(monkeypatch, {})


@pytest.mark.parametrize("conf", ["ippp_static_cdfs", "tiles_2x2_lr_qm_grain", "entropy_groups"])
def test_range_coder_forms_and_orders_on_inter_chunks(av1mi, oracle, monkeypatch, conf):
    """Both forms of the range coder (AV1MI_RC_STAGES 2 / 4), each in the natural and the length-sorted tile order (AV1MI_RC_SORT 0 / 1),
    on what the all-key tests do not reach: inter syntax with static CDFs; 2 x 2-superblock tiles with switchable restoration,
    quantiser matrices and film grain; an inter chunk entropy-coded in groups of two frames (launches whose first tile is not the
    chunk's first, with a tile order).  Every run equals the oracle."""
    if conf == "ippp_static_cdfs":
        w, h, bd, n, keyint, fg = 200, 120, 8, 5, 240, 0
        pkw, okw, env = dict(block_log2=5, cdf_update=0), dict(min_bs_log2=5, max_bs_log2=5, disable_cdf_update=1), {}
    elif conf == "tiles_2x2_lr_qm_grain":
        w, h, bd, n, keyint, fg, cq = 328, 248, 10, 4, 2, 20, 30
        qidx = av1mi.cq_to_qindex(cq)
        lvl = oracle.qm_level(qidx, 1, 15)
        pkw = dict(block_log2=4, tile_sb=2, enable_lr=2, enable_qm=1, qm_min=1, qm_max=15, film_grain=fg, cq_level=cq)
        okw = dict(min_bs_log2=4, max_bs_log2=4, tile_w_sb=2, tile_h_sb=2, enable_lr=2, enable_qm=1, qm_y=lvl, qm_uv=lvl, base_q_idx=qidx)
        env = {}
    else:
        w, h, bd, n, keyint, fg = 200, 120, 8, 7, 240, 0
        pkw, okw, env = dict(block_log2=5, subpel=1), dict(min_bs_log2=5, max_bs_log2=5, subpel=1), {"AV1MI_ENTROPY_GROUP": "2"}
    frames = [oracle.synthclip_frame(w, h, bd, seed=620 + w, t=t) for t in range(n)]
    raw = b"".join(raw_of(f, bd) for f in frames)
    tus = _oracle_tus(oracle, frames, w, h, bd, keyint, fg, **okw)
    p = av1mi.default_params(w, h, bd, keyint=keyint, **pkw)
    for stages in ("2", "4"):
        for sort in ("0", "1"):
            _set_rc_env(monkeypatch, dict(env, AV1MI_RC_STAGES=stages, AV1MI_RC_SORT=sort))
            with av1mi.Context(0) as c:
                data, sizes, _, _ = c.encode_chunk(p, raw, n)
            assert list(sizes) == [len(t) for t in tus], (stages, sort)
            assert data == b"".join(tus), (stages, sort)
    _set_rc_env(monkeypatch, {})


def test_production_point_where_the_default_is_the_two_stage_form(av1mi, oracle, monkeypatch):
    """The reference's production point on a 1080p chunk of 40 frames (10-bit, keyint 240, CQ 8 -> base_q_idx 32, the reference's
    tools): 40 x 510 tiles are 319 workgroups and the quantiser index is below 64, so the launcher's default is the two-stage form.
    The default's bytes equal forced form 4 and forced form 2 in the sorted order; the first two temporal units equal the oracle
    (frame i depends only on the frames before it)."""
    w, h, bd, n, cq = 1920, 1080, 10, 40, 8
    qidx = av1mi.cq_to_qindex(cq)
    assert qidx < 64 and (n * 30 * 17 + 63) // 64 == 319
    frames = [oracle.synthclip_frame(w, h, bd, seed=1080, t=t) for t in range(n)]
    raw = b"".join(raw_of(f, bd) for f in frames)
    p = av1mi.default_params(w, h, bd, keyint=240, cq_level=cq, film_grain=20, enable_qm=1, qm_min=1, qm_max=15, subpel=1, deblock=1, enable_lr=2)
    outs = []
    for env in ({}, {"AV1MI_RC_STAGES": "4"}, {"AV1MI_RC_STAGES": "2", "AV1MI_RC_SORT": "1"}):
        _set_rc_env(monkeypatch, env)
        with av1mi.Context(0) as c:
            data, sizes, _, _ = c.encode_chunk(p, raw, n)
        outs.append((data, list(sizes)))
    _set_rc_env(monkeypatch, {})
    assert outs[1] == outs[0] and outs[2] == outs[0]
    lvl = oracle.qm_level(qidx, 1, 15)
    tus = _oracle_tus(oracle, frames[:2], w, h, bd, 240, 20, min_bs_log2=5, max_bs_log2=5, base_q_idx=qidx, subpel=1,
                      deblock=1, enable_lr=2, enable_qm=1, qm_y=lvl, qm_uv=lvl)
    data, sizes = outs[0]
    assert sizes[:2] == [len(t) for t in tus]
    assert data[:sizes[0] + sizes[1]] == b"".join(tus)


def test_golden_inter_sequences_through_the_c_abi(av1mi, ctx, oracle, golden_sequences):
    """The dav1d-pinned inter sequences the GPU path can express (decision-driven, one-superblock tiles)."""
    n = 0
    for m in golden_sequences:
        cfgk = dict(m["config"])
        min_bs = cfgk.get("min_bs_log2", 4)
        bs = cfgk.get("max_bs_log2", min_bs)
        if any(k.startswith("fuzz") for k in cfgk) or cfgk.get("tile_w_sb", 1) != 1 or cfgk.get("film_grain"):
            continue
        if m["width"] % 8 or m["height"] % 8:
            continue   # (covered by test_sizes_that_are_not_multiples_of_8: fixtures here are generated full-size)
        p = av1mi.default_params(m["width"], m["height"], m["bit_depth"], block_log2=bs, keyint=240, me_range=cfgk.get("me_range", 8),
                                 cdf_update=0 if cfgk.get("disable_cdf_update") else 1, enable_lr=cfgk.get("enable_lr", 0), deblock=cfgk.get("deblock", 0),
                                 subpel=cfgk.get("subpel", 0), intra_mode_mask=cfgk.get("mode_mask", 0), intra_angle_delta=cfgk.get("angle_delta", 0))
        p.intra_edge_filter = cfgk.get("intra_edge_filter", 0)
        p.cfl = cfgk.get("cfl", 0)
        p.partition_search, p.min_block_log2 = cfgk.get("partition_search", 0), min_bs
        p.me_presearch = cfgk.get("me_presearch", 0)
        if cfgk.get("enable_qm"):
            p.enable_qm, p.qm_min, p.qm_max = 1, cfgk["qm_y"], cfgk["qm_y"]
        frames = [oracle.synthclip_frame(m["width"], m["height"], m["bit_depth"], seed=m["seed"], t=t * m.get("t_step", 1)) for t in range(m["frames"])]
        data, sizes, rep, recon = ctx.encode_chunk(p, b"".join(raw_of(f, m["bit_depth"]) for f in frames), m["frames"], want_recon=True)
        assert data == m["obu"], m["name"]
        fb = m["width"] * m["height"] * 3 // 2 * (2 if m["bit_depth"] > 8 else 1)
        for t in range(m["frames"]):
            assert sha(split_planes(recon.tobytes()[t * fb:(t + 1) * fb], m["width"], m["height"], m["bit_depth"])) == m["dav1d_sha256"][t], (m["name"], t)
        n += 1
    assert n >= 4


@pytest.mark.parametrize("w,h,bd,n,bs,cq,qmin,qmax,extra", [
    (200, 120, 10, 4, 5, 8, 1, 15, dict(film_grain=20)),      # the reference's production string (av1an.rs:14)
    (328, 248, 8, 3, 4, 30, 8, 15, dict(deblock=1)),          # the encoder's default range at the benchmark's quantiser
    (136, 136, 10, 3, 3, 50, 0, 15, dict(enable_lr=1)),
    (232, 120, 8, 2, 5, 63, 0, 14, dict()),
    (72, 56, 8, 2, 5, 20, 15, 15, dict())])                   # using_qmatrix with flat matrices
def test_quantiser_matrices_equal_oracle(av1mi, ctx, oracle, w, h, bd, n, bs, cq, qmin, qmax, extra):
    """enable_qm: level from the quantiser index, per-position dequantiser steps in the quantiser and the
    dequantiser, using_qmatrix / qm_y / qm_u in every frame header - IPPP chunk bit-exact against the oracle."""
    frames = [oracle.synthclip_frame(w, h, bd, seed=900 + w, t=t) for t in range(n)]
    p = av1mi.default_params(w, h, bd, block_log2=bs, keyint=240, cq_level=cq, enable_qm=1, qm_min=qmin, qm_max=qmax, **extra)
    data, sizes, rep, recon = ctx.encode_chunk(p, b"".join(raw_of(f, bd) for f in frames), n, want_recon=True)
    qidx = av1mi.cq_to_qindex(cq)
    lvl = oracle.qm_level(qidx, qmin, qmax)
    assert 0 <= lvl <= 15
    kw = dict(min_bs_log2=bs, max_bs_log2=bs, base_q_idx=qidx, enable_qm=1, qm_y=lvl, qm_uv=lvl, deblock=extra.get("deblock", 0), enable_lr=extra.get("enable_lr", 0))
    tus, recs = [], []
    ref = prev = None
    for t, f in enumerate(frames):
        if extra.get("film_grain"):
            kw.update(film_grain=1, fg_y_scaling=2 * extra["film_grain"], fg_c_scaling=extra["film_grain"], fg_seed=(7391 + 173 * t) & 0xFFFF)   # first_frame 0
        cfg = oracle.default_config(w, h, bd, **kw)
        tu, rec, st = oracle.encode_frame(cfg, f, with_seq_hdr=(t == 0), ref=ref, prev_src=prev)
        tus.append(tu)
        recs.append(rec)
        ref, prev = rec, f
    assert list(sizes) == [len(t) for t in tus]
    assert data == b"".join(tus)
    assert recon.tobytes() == b"".join(raw_of(r, bd) for r in recs)


@pytest.mark.parametrize("w,h,bd,n,bs,me,extra", [
    (64, 64, 8, 3, 5, 8, dict()), (200, 120, 8, 4, 5, 8, dict()), (200, 120, 10, 3, 4, 8, dict(deblock=1)), (136, 136, 8, 3, 3, 8, dict()),
    (328, 248, 10, 3, 5, 16, dict(enable_lr=1)), (130, 66, 8, 3, 4, 8, dict()), (648, 360, 10, 3, 5, 8, dict(enable_qm=1, qm_min=4, qm_max=4)),
    (200, 120, 8, 3, 6, 8, dict()), (184, 248, 10, 3, 6, 16, dict(deblock=1, enable_lr=2)), (648, 360, 8, 3, 6, 8, dict(enable_qm=1, qm_min=2, qm_max=2))])
def test_subsample_motion_vectors_equal_oracle(av1mi, ctx, oracle, w, h, bd, n, bs, me, extra):
    """subpel = 1: half- then quarter-sample refinement of the full search (EIGHTTAP-interpolated previous source),
    8-tap motion compensation of luma and chroma, fractional vectors in the candidate list and the NEWMV syntax,
    interpolation_filter = EIGHTTAP in the frame header - IPPP chunk bit-exact against the oracle."""
    frames = [oracle.synthclip_frame(w, h, bd, seed=700 + w, t=t) for t in range(n)]
    p = av1mi.default_params(w, h, bd, block_log2=bs, keyint=240, me_range=me, subpel=1, **extra)
    data, sizes, rep, recon = ctx.encode_chunk(p, b"".join(raw_of(f, bd) for f in frames), n, want_recon=True)
    kw = dict(min_bs_log2=bs, max_bs_log2=bs, me_range=me, subpel=1, deblock=extra.get("deblock", 0), enable_lr=extra.get("enable_lr", 0))
    if extra.get("enable_qm"):
        kw.update(enable_qm=1, qm_y=extra["qm_min"], qm_uv=extra["qm_min"])
    cfg = oracle.default_config(w, h, bd, **kw)
    tus, recs = oracle_chunk(oracle, cfg, frames, 240)
    assert list(sizes) == [len(t) for t in tus]
    off = 0
    for i, tu in enumerate(tus):
        assert data[off:off + sizes[i]] == tu, "frame %d" % i
        off += sizes[i]
    assert recon.tobytes() == b"".join(raw_of(r, bd) for r in recs)


def test_qm_is_validated(av1mi, ctx):
    for bad in (dict(qm_min=9, qm_max=8), dict(qm_min=16, qm_max=16), dict(qm_max=16)):
        p = av1mi.default_params(64, 64, 8, enable_qm=1, **bad)
        with pytest.raises(av1mi.EncodeFailed):
            ctx.encode_chunk(p, bytes(64 * 64 * 3 // 2), 1)


@pytest.mark.parametrize("extra", [dict(), dict(subpel=1, enable_qm=1, qm_min=1, qm_max=15, deblock=1, enable_lr=2, film_grain=20)])
def test_1080p_key_and_inter_frame_equal_oracle(av1mi, ctx, oracle, extra):
    """BASELINE config 3 at its own size (1920x1080, 10-bit, IPPP): 30 x 17 superblocks whose bottom row is 56 samples tall
    (a 32 / 16 / 8 mix of leaf sizes through recon_inter_pre_kernel and the tile walk).  One key frame and two P frames,
    plain and with every optional tool on - every temporal unit and every reconstruction bit-exact against the oracle."""
    w, h, bd, n = 1920, 1080, 10, 3
    frames = [oracle.synthclip_frame(w, h, bd, seed=1080, t=t) for t in range(n)]
    p = av1mi.default_params(w, h, bd, keyint=240, **extra)
    data, sizes, rep, recon = ctx.encode_chunk(p, b"".join(raw_of(f, bd) for f in frames), n, want_recon=True)
    kw = dict(min_bs_log2=5, max_bs_log2=5)
    if extra:
        lvl = oracle.qm_level(av1mi.cq_to_qindex(30), 1, 15)
        kw.update(subpel=1, enable_qm=1, qm_y=lvl, qm_uv=lvl, deblock=1, enable_lr=2, film_grain=1, fg_y_scaling=40, fg_c_scaling=20)
    tus, recs, ref, prev = [], [], None, None
    for t, f in enumerate(frames):
        if extra:
            kw["fg_seed"] = (7391 + 173 * t) & 0xFFFF
        cfg = oracle.default_config(w, h, bd, **kw)
        tu, rec, st = oracle.encode_frame(cfg, f, with_seq_hdr=(t == 0), ref=ref, prev_src=prev)
        tus.append(tu)
        recs.append(rec)
        ref, prev = rec, f
    assert list(sizes) == [len(t) for t in tus]
    for i, tu in enumerate(tus):
        assert data[sum(sizes[:i]):sum(sizes[:i + 1])] == tu, "frame %d" % i
    fb = w * h * 3
    for i, rec in enumerate(recs):
        assert recon.tobytes()[i * fb:(i + 1) * fb] == raw_of(rec, bd), "reconstruction of frame %d" % i


def test_1080p_64x64_blocks_equal_oracle(av1mi, ctx, oracle):
    """block_log2 = 6 at BASELINE's 1080p size: 64x64 leaves with the 64-point transform in 16 superblock rows, the bottom row
    (56 samples) as 64x64 leaves that overhang the frame by 8 - key frame and P frame with sub-sample motion, bit-exact."""
    w, h, bd, n = 1920, 1080, 10, 2
    frames = [oracle.synthclip_frame(w, h, bd, seed=1081, t=t) for t in range(n)]
    p = av1mi.default_params(w, h, bd, keyint=240, block_log2=6, subpel=1)
    data, sizes, rep, recon = ctx.encode_chunk(p, b"".join(raw_of(f, bd) for f in frames), n, want_recon=True)
    cfg = oracle.default_config(w, h, bd, min_bs_log2=6, max_bs_log2=6, subpel=1)
    tus, recs = oracle_chunk(oracle, cfg, frames, 240)
    assert list(sizes) == [len(t) for t in tus]
    assert data == b"".join(tus)
    assert recon.tobytes() == b"".join(raw_of(r, bd) for r in recs)


def test_4k_key_and_inter_frame_equal_oracle(av1mi, ctx, oracle):
    """BASELINE config 4's frame size (3840x2160, 10-bit: 60 x 34 one-superblock tiles, the bottom row 48 samples
    tall): one key frame and one P frame, bit-exact against the oracle."""
    w, h, bd, n = 3840, 2160, 10, 2
    frames = [oracle.synthclip_frame(w, h, bd, seed=2160, t=t) for t in range(n)]
    p = av1mi.default_params(w, h, bd, keyint=2)
    data, sizes, rep, recon = ctx.encode_chunk(p, b"".join(raw_of(f, bd) for f in frames), n, want_recon=True)
    cfg = oracle.default_config(w, h, bd, min_bs_log2=5, max_bs_log2=5)
    tus, recs = oracle_chunk(oracle, cfg, frames, 2)
    assert data == b"".join(tus)
    fb = w * h * 3
    assert recon.tobytes()[fb:2 * fb] == raw_of(recs[1], bd)


def test_4k_every_optional_tool_equals_oracle(av1mi, ctx, oracle):
    """3840x2160 10-bit key + P frame with every optional tool on at once: quarter-sample vectors with the SATD refinement,
    quantiser matrices, deblocking, switchable Wiener / self-guided restoration, film-grain table."""
    w, h, bd, n = 3840, 2160, 10, 2
    frames = [oracle.synthclip_frame(w, h, bd, seed=2161, t=t) for t in range(n)]
    p = av1mi.default_params(w, h, bd, keyint=2, subpel=1, enable_qm=1, qm_min=1, qm_max=15, deblock=1, enable_lr=2, film_grain=20)
    data, sizes, rep, recon = ctx.encode_chunk(p, b"".join(raw_of(f, bd) for f in frames), n, want_recon=True)
    lvl = oracle.qm_level(av1mi.cq_to_qindex(30), 1, 15)
    tus, recs, ref, prev = [], [], None, None
    for t, f in enumerate(frames):
        cfg = oracle.default_config(w, h, bd, min_bs_log2=5, max_bs_log2=5, subpel=1, enable_qm=1, qm_y=lvl, qm_uv=lvl, deblock=1, enable_lr=2,
                                    film_grain=1, fg_y_scaling=40, fg_c_scaling=20, fg_seed=(7391 + 173 * t) & 0xFFFF)
        tu, rec, st = oracle.encode_frame(cfg, f, with_seq_hdr=(t == 0), ref=ref, prev_src=prev)
        tus.append(tu)
        recs.append(rec)
        ref, prev = rec, f
    assert list(sizes) == [len(t) for t in tus]
    assert data == b"".join(tus)
    assert recon.tobytes() == b"".join(raw_of(r, bd) for r in recs)


def test_encode_file_matroska_and_obu_outputs(av1mi, oracle, tmp_path):
    """output_path ending in .mkv (the reference's job output, jobs.rs:187-188): EBML header, Segment with Info,
    one V_AV1 track whose CodecPrivate is the av1C record + sequence header, one Cluster per key frame with a
    SimpleBlock per frame (temporal delimiters dropped).  .obu: the bare stream.  Payloads equal the IVF path's."""
    w, h, n = 136, 72, 7
    frames = [oracle.synthclip_frame(w, h, 8, seed=78, t=t) for t in range(n)]
    y4m = tmp_path / "clip.y4m"
    with open(y4m, "wb") as f:
        f.write(b"YUV4MPEG2 W%d H%d F25:1 Ip A1:1 C420jpeg\n" % (w, h))
        for fr in frames:
            f.write(b"FRAME\n" + raw_of(fr, 8))
    outs = {}
    for ext in ("ivf", "mkv", "obu"):
        out = tmp_path / ("clip." + ext)
        rep = av1mi.run_mi355x(av1mi.EncodeParams(y4m, out, tmp_path, av1mi.derive_plan(8), chunk_frames=4, keyint=2))
        assert rep.frames == n
        outs[ext] = out.read_bytes()
    tus, pos = [], 32
    while pos < len(outs["ivf"]):
        sz = int.from_bytes(outs["ivf"][pos:pos + 4], "little")
        tus.append(outs["ivf"][pos + 12:pos + 12 + sz])
        pos += 12 + sz
    assert len(tus) == n
    if outs["obu"] != b"".join(tus):   # diagnostic for a rare flake: which frames differ between two runs of the same encode
        pos, sizes = 0, []
        cfg = oracle.default_config(w, h, 8, min_bs_log2=5, max_bs_log2=5)
        ref_tus = oracle_chunk(oracle, cfg, frames[:4], 2)[0] + oracle_chunk(oracle, cfg, frames[4:], 2)[0]
        raise AssertionError("ivf run vs oracle: %s; obu bytes %d vs %d" % ([i for i in range(n) if tus[i] != ref_tus[i]], len(outs["obu"]), len(b"".join(tus))))
    mkv = outs["mkv"]
    top = list(_ebml(mkv, 0, len(mkv)))
    assert [e[0] for e in top] == [0x1A45DFA3, 0x18538067] and top[1][2] == len(mkv)
    hdr = {e[0]: mkv[e[1]:e[2]] for e in _ebml(mkv, top[0][1], top[0][2])}
    assert hdr[0x4282] == b"matroska"
    seg = list(_ebml(mkv, top[1][1], top[1][2]))
    assert [e[0] for e in seg][:2] == [0x1549A966, 0x1654AE6B] and all(e[0] == 0x1F43B675 for e in seg[2:])
    info = {e[0]: mkv[e[1]:e[2]] for e in _ebml(mkv, seg[0][1], seg[0][2])}
    import struct
    assert int.from_bytes(info[0x2AD7B1], "big") == 1000000 and struct.unpack(">d", info[0x4489])[0] == n * 1000 // 25
    entry = next(_ebml(mkv, seg[1][1], seg[1][2]))
    te = {e[0]: (e[1], e[2]) for e in _ebml(mkv, entry[1], entry[2])}
    assert mkv[te[0x86][0]:te[0x86][1]] == b"V_AV1"
    priv = mkv[te[0x63A2][0]:te[0x63A2][1]]
    seq_obu = tus[0][2:2 + 2 + tus[0][3]]
    assert priv[:4] == bytes([0x81, 31, 0x0C, 0]) and priv[4:] == seq_obu
    vid = {e[0]: int.from_bytes(mkv[e[1]:e[2]], "big") for e in _ebml(mkv, te[0xE0][0], te[0xE0][1])}
    assert vid == {0xB0: w, 0xBA: h}
    blocks = []
    for c in seg[2:]:
        els = list(_ebml(mkv, c[1], c[2]))
        t0 = int.from_bytes(mkv[els[0][1]:els[0][2]], "big")
        assert els[0][0] == 0xE7
        for e in els[1:]:
            assert e[0] == 0xA3 and mkv[e[1]] == 0x81
            blocks.append((t0 + int.from_bytes(mkv[e[1] + 1:e[1] + 3], "big", signed=True), mkv[e[1] + 3], mkv[e[1] + 4:e[2]]))
    assert [b[0] for b in blocks] == [i * 1000 // 25 for i in range(n)]
    # chunks of 4 frames, key frame every 2 frames inside a chunk: frames 0, 2, 4, 6 are key frames
    assert [b[1] for b in blocks] == [0x80, 0, 0x80, 0, 0x80, 0, 0x80]
    assert [b[2] for b in blocks] == [t[2:] for t in tus]


@pytest.mark.parametrize("triple", [(9, 16, 0), (0, 0, 1), (1, 0, 0), (9, 16, 9)])
def test_encode_file_matroska_colour_equals_the_sequence_header(av1mi, oracle, tmp_path, triple):
    """The Matroska track's Colour element says what the sequence header's color_config says, also for a partial colour triple (a field
    left at 0 is 2 "unspecified" in both; MC 0 would be MC_IDENTITY, which 4:2:0 forbids)."""
    from edge_content import color_config
    w, h = 72, 56
    y4m = tmp_path / "clip.y4m"
    y4m.write_bytes(b"YUV4MPEG2 W%d H%d F25:1 Ip A1:1 C420jpeg\n" % (w, h) + b"FRAME\n" + raw_of(oracle.synthclip_frame(w, h, 8, seed=81, t=0), 8))
    out = tmp_path / "clip.mkv"
    hdr = dict(zip(("color_primaries", "transfer_characteristics", "matrix_coefficients"), triple))
    rep = av1mi.run_mi355x(av1mi.EncodeParams(y4m, out, tmp_path, av1mi.derive_plan(8), chunk_frames=1, **hdr))
    assert rep.frames == 1
    mkv = out.read_bytes()
    top = list(_ebml(mkv, 0, len(mkv)))
    seg = list(_ebml(mkv, top[1][1], top[1][2]))
    entry = next(_ebml(mkv, seg[1][1], seg[1][2]))
    te = {e[0]: (e[1], e[2]) for e in _ebml(mkv, entry[1], entry[2])}
    vid = {e[0]: (e[1], e[2]) for e in _ebml(mkv, te[0xE0][0], te[0xE0][1])}
    col = {e[0]: int.from_bytes(mkv[e[1]:e[2]], "big") for e in _ebml(mkv, vid[0x55B0][0], vid[0x55B0][1])}
    desc, cp, tc, mc, cr = color_config(mkv[te[0x63A2][0]:te[0x63A2][1]][4:])
    assert desc == 1 and 0 not in (cp, tc, mc)
    assert (col[0x55BB], col[0x55BA], col[0x55B1], col[0x55B9]) == (cp, tc, mc, 2 if cr else 1)
    assert (cp, tc, mc) == tuple(v or 2 for v in triple)


def test_encode_file_hdr_colour_frame_parameters_and_gpu_mask(av1mi, oracle, tmp_path):
    """BASELINE config 5's "HDR": the job's colour description (BT.2020 / PQ / BT.2020 NCL) reaches the sequence header - the same bytes
    as the oracle's, which dav1d / libavif read back (tests/golden/k200x120_hdr_bt2020_pq_10b) - and the Matroska track's Colour element.
    The clip's FRAME markers carry parameters ("FRAME Ip"): the sequential reader takes over from the offset-based one.  `workers` = 2 under
    `gpu_mask` = GPU 0 reports exactly that GPU as used; a mask that allows no visible GPU is AV1MI_E_NO_DEVICE."""
    import torch
    w, h, n = 136, 72, 5
    frames = [oracle.synthclip_frame(w, h, 10, seed=80, t=t) for t in range(n)]
    y4m = tmp_path / "clip.y4m"
    with open(y4m, "wb") as f:
        f.write(b"YUV4MPEG2 W%d H%d F25:1 Ip A1:1 C420p10 XYSCSS=420P10\n" % (w, h))
        for fr in frames:
            f.write(b"FRAME Ip\n" + raw_of(fr, 10))
    hdr = dict(color_primaries=9, transfer_characteristics=16, matrix_coefficients=9)
    out = tmp_path / "clip.mkv"
    plan = av1mi.derive_plan(8)
    plan.av1an_workers = 2
    rep = av1mi.run_mi355x(av1mi.EncodeParams(y4m, out, tmp_path, plan, chunk_frames=2, gpu_mask=0b1, **hdr))
    assert rep.frames == n and rep.chunks == 3 and rep.gpus_used == 0b1
    mkv = out.read_bytes()
    top = list(_ebml(mkv, 0, len(mkv)))
    seg = list(_ebml(mkv, top[1][1], top[1][2]))
    entry = next(_ebml(mkv, seg[1][1], seg[1][2]))
    te = {e[0]: (e[1], e[2]) for e in _ebml(mkv, entry[1], entry[2])}
    vid = {e[0]: (e[1], e[2]) for e in _ebml(mkv, te[0xE0][0], te[0xE0][1])}
    col = {e[0]: int.from_bytes(mkv[e[1]:e[2]], "big") for e in _ebml(mkv, vid[0x55B0][0], vid[0x55B0][1])}
    assert col == {0x55B1: 9, 0x55B2: 10, 0x55B3: 1, 0x55B4: 1, 0x55B9: 1, 0x55BA: 16, 0x55BB: 9}
    priv = mkv[te[0x63A2][0]:te[0x63A2][1]]
    cfg = oracle.default_config(w, h, 10, min_bs_log2=5, max_bs_log2=5, **hdr)
    tu, _, _ = oracle.encode_frame(cfg, frames[0])
    assert priv[4:] == tu[2:2 + 2 + tu[3]]            # CodecPrivate's sequence header == the oracle's, colour description included
    first_block = next(e for c in seg[2:] for e in list(_ebml(mkv, c[1], c[2]))[1:])
    assert mkv[first_block[1] + 4:first_block[2]] == tu[2:]   # and the first frame's payload (temporal delimiter dropped)
    if torch.cuda.device_count() < 2:
        with pytest.raises(av1mi.EncodeFailed) as ei:
            av1mi.run_mi355x(av1mi.EncodeParams(y4m, tmp_path / "no.mkv", tmp_path, plan, chunk_frames=2, gpu_mask=0b10, **hdr))
        assert ei.value.code == av1mi.E_NO_DEVICE and not (tmp_path / "no.mkv").exists()


def test_job_execute_segment_states_and_metrics(av1mi, oracle, tmp_path):
    """Success path of the caller's encode segment: encoding -> validating -> (hands back at) size_gating, chunks
    directory created and removed, JobMetrics fields filled from the progress callback."""
    w, h, n = 136, 72, 9
    y4m = tmp_path / "clip.y4m"
    with open(y4m, "wb") as f:
        f.write(b"YUV4MPEG2 W%d H%d F30:1 Ip A1:1 C420jpeg\n" % (w, h))
        for t in range(n):
            f.write(b"FRAME\n" + raw_of(oracle.synthclip_frame(w, h, 8, seed=79, t=t), 8))
    out = tmp_path / "out.mkv"
    rc, stages, m, err = av1mi.job_execute("abc", y4m, out, tmp_path / "work", workers=2, keyint=4)
    assert rc == 0 and err == "" and stages == ["encoding", "validating", "size_gating"]
    assert m.frames_encoded == n and m.total_frames == n and m.progress == 1.0 and m.fps > 0 and m.bitrate_kbps > 0
    # bitrate at the clip's own frame rate (30 fps here): bytes of the finished file over n / 30 seconds, within the container overhead
    assert 0.5 < m.bitrate_kbps / (m.size_in_bytes_after * 8 / 1000 / (n / 30)) <= 1.0
    assert m.size_in_bytes_after == out.stat().st_size > 0 and 25 < m.psnr < 60 and m.crf == 30 and m.workers == 2
    assert (tmp_path / "work").exists() and not (tmp_path / "work" / "chunks_abc").exists()


def test_progress_reports_the_clip_length_and_range_tag_is_honoured(av1mi, oracle, tmp_path):
    """The progress callback's total is the clip's length from the start (not "frames read so far"), progress is monotonic,
    and an XCOLORRANGE=FULL tag of the Y4M header ends up in the sequence header (default: studio range)."""
    w, h, n = 72, 56, 10
    frames = [oracle.synthclip_frame(w, h, 8, seed=83, t=t) for t in range(n)]
    streams = {}
    for tag, cr in ((b"", 0), (b" XCOLORRANGE=FULL", 1), (b" XCOLORRANGE=LIMITED", 0)):
        y4m = tmp_path / ("clip%d%d.y4m" % (cr, len(tag)))
        with open(y4m, "wb") as f:
            f.write(b"YUV4MPEG2 W%d H%d F24:1 Ip A1:1 C420jpeg%s\n" % (w, h, tag))
            for fr in frames:
                f.write(b"FRAME\n" + raw_of(fr, 8))
        out = tmp_path / ("o%d%d.obu" % (cr, len(tag)))
        seen = []
        av1mi.run_mi355x(av1mi.EncodeParams(y4m, out, tmp_path, av1mi.derive_plan(8, workers_override=2), chunk_frames=2),
                         progress=lambda d, t, fps, b: seen.append((d, t)))
        assert seen and all(t == n for _, t in seen) and [d for d, _ in seen] == sorted(d for d, _ in seen) and seen[-1][0] == n
        cfg = oracle.default_config(w, h, 8, min_bs_log2=5, max_bs_log2=5, color_range=cr)
        assert out.read_bytes() == b"".join(oracle.encode_frame(cfg, fr)[0] for fr in frames), tag
        streams[tag] = out.read_bytes()
    assert streams[b""] == streams[b" XCOLORRANGE=LIMITED"] != streams[b" XCOLORRANGE=FULL"]


def test_one_context_switching_tile_size_at_the_same_frame_size(av1mi, oracle):
    """Regression: the per-tile buffers are sized by the tile grid.  648x360 is 11 x 6 superblocks: 66 tiles x 4096 entries at
    tile_sb 1 but 18 tiles x 16384 at tile_sb 2 - a context reusing its workspace across that switch wrote past the end."""
    w, h, bd, n = 648, 360, 8, 2
    frames = [oracle.synthclip_frame(w, h, bd, seed=84, t=t) for t in range(n)]
    raw = b"".join(raw_of(f, bd) for f in frames)
    with av1mi.Context(0) as c:
        for tsb in (1, 2, 1):
            p = av1mi.default_params(w, h, bd, tile_sb=tsb)
            data, sizes, rep, recon = c.encode_chunk(p, raw, n, want_recon=True)
            cfg = oracle.default_config(w, h, bd, min_bs_log2=5, max_bs_log2=5, tile_w_sb=tsb, tile_h_sb=tsb)
            tus, recs = oracle_chunk(oracle, cfg, frames, 1)
            assert data == b"".join(tus), tsb
            assert recon.tobytes() == b"".join(raw_of(r, bd) for r in recs), tsb


def test_encode_file_many_chunks_few_workers(av1mi, oracle, tmp_path):
    """More chunks than 2 x workers: the reader must keep writing finished chunks while it waits for room
    (regression: it used to wait for room only, and deadlocked once every outstanding chunk was finished)."""
    w, h, n = 72, 56, 12
    y4m = tmp_path / "clip.y4m"
    with open(y4m, "wb") as f:
        f.write(b"YUV4MPEG2 W%d H%d F30:1 Ip A1:1 C420jpeg\n" % (w, h))
        for t in range(n):
            f.write(b"FRAME\n" + raw_of(oracle.synthclip_frame(w, h, 8, seed=80, t=t), 8))
    outs = []
    for workers in (1, 3):
        out = tmp_path / ("o%d.obu" % workers)
        rep = av1mi.run_mi355x(av1mi.EncodeParams(y4m, out, tmp_path, av1mi.derive_plan(8, workers_override=workers), chunk_frames=1))
        assert rep.frames == n and rep.chunks == n
        outs.append(out.read_bytes())
    assert outs[0] == outs[1]


def test_encode_file_failure_mid_job_leaves_the_process_sound(av1mi, oracle, tmp_path):
    """A job that fails with chunks in flight - a host-side format error: 100 bytes of a seventh frame behind six whole ones, one frame per
    chunk, two workers - leaves neither an output nor a temporary file, and the process encodes the good clip afterwards to the bytes it
    gave before (the failed job's contexts are destroyed, not recycled); the caches are released at the end."""
    w, h, n = 72, 56, 6
    fr = [raw_of(oracle.synthclip_frame(w, h, 8, seed=85, t=t), 8) for t in range(n + 1)]
    good = b"YUV4MPEG2 W%d H%d F30:1 Ip A1:1 C420jpeg\n" % (w, h) + b"".join(b"FRAME\n" + f for f in fr[:n])
    (tmp_path / "good.y4m").write_bytes(good)
    (tmp_path / "bad.y4m").write_bytes(good + b"FRAME\n" + fr[n][:94])   # marker and 94 bytes: 100 trailing bytes
    plan = av1mi.derive_plan(8, workers_override=2)

    def encode(name):
        out = tmp_path / (name + ".obu")
        rep = av1mi.run_mi355x(av1mi.EncodeParams(tmp_path / "good.y4m", out, tmp_path, plan, chunk_frames=1))
        assert rep.frames == n and rep.chunks == n
        return out.read_bytes()

    first = encode("first")
    with pytest.raises(av1mi.EncodeFailed) as ei:
        av1mi.run_mi355x(av1mi.EncodeParams(tmp_path / "bad.y4m", tmp_path / "bad.obu", tmp_path, plan, chunk_frames=1))
    assert ei.value.code == av1mi.E_FORMAT
    assert not (tmp_path / "bad.obu").exists() and not list(tmp_path.glob("*.tmp.*"))
    assert encode("again") == first
    av1mi.release_caches()


@pytest.mark.parametrize("w,h,bd,n,bs,keyint", [(200, 120, 8, 2, 5, 1), (328, 248, 10, 2, 4, 1), (72, 104, 8, 2, 5, 1), (648, 360, 8, 3, 5, 240),
                                               (200, 120, 10, 3, 4, 2)])
def test_loop_restoration_equals_oracle(av1mi, ctx, oracle, w, h, bd, n, bs, keyint):
    """enable_lr: per-unit Wiener decision + filter on key and inter frames (the restored frame is the
    next frame's reference); streams and reconstructions bit-exact against the oracle.  72x104: the last unit holds
    two stripes."""
    frames = [oracle.synthclip_frame(w, h, bd, seed=900 + w, t=t) for t in range(n)]
    p = av1mi.default_params(w, h, bd, block_log2=bs, keyint=keyint, enable_lr=1)
    data, sizes, rep, recon = ctx.encode_chunk(p, b"".join(raw_of(f, bd) for f in frames), n, want_recon=True)
    cfg = oracle.default_config(w, h, bd, min_bs_log2=bs, max_bs_log2=bs, enable_lr=1)
    tus, recs = oracle_chunk(oracle, cfg, frames, keyint)
    assert data == b"".join(tus)
    fb = w * h * 3 // 2 * (2 if bd > 8 else 1)
    for i, rec in enumerate(recs):
        assert recon.tobytes()[i * fb:(i + 1) * fb] == raw_of(rec, bd), "reconstruction of frame %d" % i


@pytest.mark.parametrize("w,h,bd,n,bs,keyint,cq,extra", [
    (64, 64, 8, 1, 5, 1, 30, dict()), (200, 120, 8, 3, 5, 240, 30, dict()), (328, 248, 10, 2, 4, 1, 30, dict(deblock=1)),
    (648, 360, 10, 3, 5, 2, 45, dict(tile_sb=2)), (202, 122, 8, 3, 5, 240, 50, dict(subpel=1)), (136, 200, 10, 2, 3, 1, 20, dict())])
def test_switchable_restoration_equals_oracle(av1mi, ctx, oracle, w, h, bd, n, bs, keyint, cq, extra):
    """enable_lr = 2 (RESTORE_SWITCHABLE): per unit off, one of the Wiener filters or one of the self-guided filters (both
    box-filter passes, A/B grids across stripe and unit edges); restoration_type / lr_sgr_set / weights against
    RefSgrXqd in the tile data - bit-exact against the oracle (whose self-guided filter dav1d pins for all 16 sets)."""
    frames = [oracle.synthclip_frame(w, h, bd, seed=950 + w, t=t) for t in range(n)]
    p = av1mi.default_params(w, h, bd, block_log2=bs, keyint=keyint, enable_lr=2, cq_level=cq, **extra)
    data, sizes, rep, recon = ctx.encode_chunk(p, b"".join(raw_of(f, bd) for f in frames), n, want_recon=True)
    tsb = extra.get("tile_sb", 1)
    cfg = oracle.default_config(w, h, bd, min_bs_log2=bs, max_bs_log2=bs, enable_lr=2, base_q_idx=av1mi.cq_to_qindex(cq), deblock=extra.get("deblock", 0),
                                subpel=extra.get("subpel", 0), tile_w_sb=tsb, tile_h_sb=tsb)
    tus, recs = oracle_chunk(oracle, cfg, frames, keyint)
    assert list(sizes) == [len(t) for t in tus]
    assert data == b"".join(tus)
    assert recon.tobytes() == b"".join(raw_of(r, bd) for r in recs)


@pytest.mark.parametrize("w,h,bd,n,bs,keyint,lr", [(328, 248, 8, 2, 4, 1, 0), (200, 120, 10, 3, 5, 240, 0), (264, 200, 8, 3, 3, 2, 1),
                                                  (648, 360, 10, 2, 5, 2, 1), (136, 136, 8, 2, 5, 1, 0), (312, 248, 8, 3, 6, 2, 0)])
def test_tiles_of_two_by_two_superblocks_equal_oracle(av1mi, ctx, oracle, w, h, bd, n, bs, keyint, lr):
    """tile_sb = 2 (what frames beyond 64 superblock rows/columns, i.e. 8K, need): intra edges, entropy contexts, CDF
    adaptation, motion-vector candidates and the restoration reference all run across the four superblocks of a
    tile.  Forced on small frames and compared with the oracle's 2 x 2 tiles (golden-pinned by dav1d)."""
    frames = [oracle.synthclip_frame(w, h, bd, seed=700 + w, t=t) for t in range(n)]
    p = av1mi.default_params(w, h, bd, block_log2=bs, keyint=keyint, enable_lr=lr, tile_sb=2)
    data, sizes, rep, recon = ctx.encode_chunk(p, b"".join(raw_of(f, bd) for f in frames), n, want_recon=True)
    cfg = oracle.default_config(w, h, bd, min_bs_log2=bs, max_bs_log2=bs, enable_lr=lr, tile_w_sb=2, tile_h_sb=2)
    tus, recs = oracle_chunk(oracle, cfg, frames, keyint)
    assert list(sizes) == [len(t) for t in tus]
    assert data == b"".join(tus)
    fb = w * h * 3 // 2 * (2 if bd > 8 else 1)
    for i, rec in enumerate(recs):
        assert recon.tobytes()[i * fb:(i + 1) * fb] == raw_of(rec, bd), "reconstruction of frame %d" % i


def test_8k_key_and_inter_frame_equal_oracle(av1mi, ctx, oracle):
    """BASELINE config 5's frame size (7680x4320, 10-bit): 120 x 68 superblocks exceed AV1's 64 x 64 tile limit, so the
    encoder switches to tiles of 2 x 2 superblocks by itself (60 x 34 tiles).  One key frame and one P frame, bit-exact
    against the oracle."""
    w, h, bd, n = 7680, 4320, 10, 2
    frames = [oracle.synthclip_frame(w, h, bd, seed=4320, t=t) for t in range(n)]
    p = av1mi.default_params(w, h, bd, keyint=2)
    data, sizes, rep, recon = ctx.encode_chunk(p, b"".join(raw_of(f, bd) for f in frames), n, want_recon=True)
    cfg = oracle.default_config(w, h, bd, min_bs_log2=5, max_bs_log2=5, tile_w_sb=2, tile_h_sb=2)
    tus, recs = oracle_chunk(oracle, cfg, frames, 2)
    assert data == b"".join(tus)
    fb = w * h * 3
    assert recon.tobytes()[fb:2 * fb] == raw_of(recs[1], bd)


def test_encode_file_ragged_and_empty_inputs(av1mi, oracle, tmp_path):
    """Edge cases at the file boundary: a Y4M with a header but no frames, a truncated last frame, a frame size that
    is odd - each a clean encoder failure (-> EncodeError::Av1anFailed in the reference's taxonomy),
    no output file and no temporary file left behind; a one-frame clip encodes."""
    w, h = 72, 56
    fr = raw_of(oracle.synthclip_frame(w, h, 8, seed=81, t=0), 8)
    hdr = b"YUV4MPEG2 W%d H%d F30:1 Ip A1:1 C420jpeg\n" % (w, h)
    cases = {"empty": hdr, "truncated": hdr + b"FRAME\n" + fr + b"FRAME\n" + fr[:100], "odd_size": b"YUV4MPEG2 W71 H56 F30:1 C420jpeg\nFRAME\n" + bytes(71 * 56 + 2 * 36 * 28)}
    for name, blob in cases.items():
        src = tmp_path / (name + ".y4m")
        src.write_bytes(blob)
        out = tmp_path / (name + ".ivf")
        with pytest.raises(av1mi.EncodeFailed) as ei:
            av1mi.run_mi355x(av1mi.EncodeParams(src, out, tmp_path, av1mi.derive_plan(8)))
        assert ei.value.code in (av1mi.E_FORMAT, av1mi.E_INVALID_ARG), name
        assert not out.exists() and not list(tmp_path.glob("*.tmp*")), name
    one = tmp_path / "one.y4m"
    one.write_bytes(hdr + b"FRAME\n" + fr)
    out = tmp_path / "one.ivf"
    rep = av1mi.run_mi355x(av1mi.EncodeParams(one, out, tmp_path, av1mi.derive_plan(8), chunk_frames=0))
    assert rep.frames == 1 and rep.chunks == 1 and out.stat().st_size > 32


def test_random_configurations_equal_oracle(av1mi, ctx, oracle):
    """Seeded sweep over combinations of the operating point (frame size, bit depth, block size, CQ, candidate modes,
    static/adaptive CDFs, key-frame interval, search range, loop restoration, film grain, tile size): every stream and
    every reconstruction bit-exact against the oracle."""
    # AV1MI_SWEEP_ITERS / AV1MI_SWEEP_SEED: longer hunts during bring-up (the default sweep found the level-buffer overlap)
    rng = np.random.default_rng(int(os.environ.get("AV1MI_SWEEP_SEED", "2026")))
    rng2 = np.random.default_rng(int(os.environ.get("AV1MI_SWEEP_SEED", "2026")) + 1)   # later additions: keeps the earlier cases as they were
    for it in range(int(os.environ.get("AV1MI_SWEEP_ITERS", "14"))):
        w, h = int(rng.integers(1, 30)) * 8, int(rng.integers(1, 22)) * 8
        if rng.integers(0, 3) == 0:   # every third case: an even size that is not a multiple of 8
            w, h = w + 2 * int(rng.integers(0, 4)), h + 2 * int(rng.integers(0, 4))
        bd = int(rng.choice([8, 10]))
        bs = int(rng.choice([3, 4, 5]))
        cq = int(rng.choice([12, 24, 30, 40, 55]))
        mask = int(rng.choice([0x7, 0x1, 0x1FFF, 0x1E07, 0x0015]))
        cdf = int(rng.integers(0, 2))
        keyint = int(rng.choice([1, 2, 3, 240]))
        me = int(rng.choice([8, 16]))
        lr = int(rng.integers(0, 2))
        fg = int(rng.choice([0, 0, 20]))
        tsb = int(rng.choice([1, 1, 2]))
        n = int(rng.integers(1, 4))
        db = int(rng.integers(0, 2))
        sp = int(rng2.integers(0, 2))
        qm = int(rng2.integers(0, 2))
        qmin = int(rng2.integers(0, 16))
        qmax = int(rng2.integers(qmin, 16))
        if lr and rng2.integers(0, 2):
            lr = 2   # RESTORE_SWITCHABLE
        if rng2.integers(0, 2) and bs == 5:
            bs = 6   # 64x64 leaves
        ad = int(rng2.integers(0, 2))   # angle deltas
        ef = int(rng2.integers(0, 2))   # enable_intra_edge_filter
        cf = int(rng2.integers(0, 2))   # chroma from luma
        ts = int(rng2.integers(0, 2))   # transform type search (IDTX)
        post = int(rng2.choice([0, 0, 5]))   # posterised source: sparse residuals
        big = [oracle.synthclip_frame(((w + 7) & ~7) + 8, ((h + 7) & ~7) + 8, bd, seed=3000 + it, t=t) for t in range(n)]
        frames = [[(f[0][:h, :w] >> post) << post, (f[1][:h // 2, :w // 2] >> post) << post, (f[2][:h // 2, :w // 2] >> post) << post] for f in big]
        p = av1mi.default_params(w, h, bd, block_log2=bs, cq_level=cq, intra_mode_mask=mask, cdf_update=cdf, keyint=keyint, me_range=me,
                                 enable_lr=lr, film_grain=fg, first_frame=5, tile_sb=tsb, deblock=db, subpel=sp, enable_qm=qm, qm_min=qmin, qm_max=qmax,
                                 intra_angle_delta=ad, intra_edge_filter=ef, cfl=cf, tx_search=ts)
        data, sizes, rep, recon = ctx.encode_chunk(p, b"".join(raw_of(f, bd) for f in frames), n, want_recon=True)
        qml = oracle.qm_level(av1mi.cq_to_qindex(cq), qmin, qmax)
        cfg = oracle.default_config(w, h, bd, min_bs_log2=bs, max_bs_log2=bs, base_q_idx=av1mi.cq_to_qindex(cq), mode_mask=mask, deblock=db,
                                    subpel=sp, enable_qm=qm, qm_y=qml, qm_uv=qml, angle_delta=ad, intra_edge_filter=ef, cfl=cf, tx_search=ts,
                                    disable_cdf_update=0 if cdf else 1, me_range=me, enable_lr=lr, tile_w_sb=tsb, tile_h_sb=tsb,
                                    film_grain=1 if fg else 0, fg_y_scaling=2 * fg, fg_c_scaling=fg)
        tus, recs, ref, prev = [], [], None, None
        for t, f in enumerate(frames):
            key = t % keyint == 0
            cfg.fg_seed = (7391 + 173 * (5 + t)) & 0xFFFF
            tu, rec, st = oracle.encode_frame(cfg, f, with_seq_hdr=key, ref=None if key else ref, prev_src=None if key else prev)
            tus.append(tu)
            recs.append(rec)
            ref, prev = rec, f
        desc = dict(it=it, ad=ad, ef=ef, cf=cf, ts=ts, post=post, w=w, h=h, bd=bd, bs=bs, cq=cq, mask=hex(mask), cdf=cdf, keyint=keyint, me=me, lr=lr, fg=fg, tsb=tsb, n=n, db=db, sp=sp, qm=qm, qmin=qmin, qmax=qmax)
        assert list(sizes) == [len(t) for t in tus], desc
        assert data == b"".join(tus), desc
        fb = w * h * 3 // 2 * (2 if bd > 8 else 1)
        for i, rec in enumerate(recs):
            assert recon.tobytes()[i * fb:(i + 1) * fb] == raw_of(rec, bd), (desc, i)


@pytest.mark.parametrize("w,h,bd,n,bs,keyint,mask,ad,tsb", [(200, 120, 8, 1, 5, 1, 0x1FFF, 1, 1), (202, 122, 10, 2, 3, 2, 0x1FFF, 1, 1), (264, 200, 8, 2, 4, 240, 0x01FE, 0, 2),
                                                          (184, 176, 10, 1, 6, 1, 0x1FFF, 1, 1), (136, 136, 8, 3, 3, 240, 0x1FFF, 1, 1), (648, 360, 8, 2, 5, 2, 0x1FFF, 1, 1)])
def test_intra_edge_filter_equals_oracle(av1mi, ctx, oracle, w, h, bd, n, bs, keyint, mask, ad, tsb):
    """enable_intra_edge_filter (spec 7.11.2.7 - 7.11.2.12): corner filter, edge filter strengths by block size / angle / smooth
    neighbours, edge upsampling for the 8x8 and 4x4 blocks - key and inter frames, luma and chroma; the oracle's side is pinned by
    dav1d (tests/golden/*_ef_*)."""
    big = [oracle.synthclip_frame(((w + 7) & ~7) + 8, ((h + 7) & ~7) + 8, bd, seed=4100 + w + bs, t=t) for t in range(n)]
    frames = [[f[0][:h, :w].copy(), f[1][:h // 2, :w // 2].copy(), f[2][:h // 2, :w // 2].copy()] for f in big]
    p = av1mi.default_params(w, h, bd, block_log2=bs, keyint=keyint, intra_mode_mask=mask, intra_angle_delta=ad, tile_sb=tsb)
    p.intra_edge_filter = 1
    data, sizes, rep, recon = ctx.encode_chunk(p, b"".join(raw_of(f, bd) for f in frames), n, want_recon=True)
    cfg = oracle.default_config(w, h, bd, min_bs_log2=bs, max_bs_log2=bs, mode_mask=mask, angle_delta=ad, intra_edge_filter=1, tile_w_sb=tsb, tile_h_sb=tsb)
    tus, recs = oracle_chunk(oracle, cfg, frames, keyint)
    assert data == b"".join(tus)
    fb = w * h * 3 // 2 * (2 if bd > 8 else 1)
    for i, rec in enumerate(recs):
        assert recon.tobytes()[i * fb:(i + 1) * fb] == raw_of(rec, bd), "reconstruction of frame %d" % i
    p.intra_edge_filter = 0
    data0, _, _, _ = ctx.encode_chunk(p, b"".join(raw_of(f, bd) for f in frames), n)
    assert data0 != data   # the switch does something on this input


@pytest.mark.parametrize("w,h,bd,n,bs,keyint,mask,ef,tsb", [(200, 120, 8, 1, 5, 1, 0x7, 0, 1), (202, 122, 10, 2, 3, 1, 0x1FFF, 1, 1), (264, 200, 8, 3, 4, 2, 0x1FFF, 0, 2),
                                                          (248, 216, 10, 1, 5, 1, 0x7, 1, 1), (184, 176, 8, 2, 6, 240, 0x7, 0, 1), (648, 360, 8, 2, 5, 1, 0x7, 0, 1)])
def test_chroma_from_luma_equals_oracle(av1mi, ctx, oracle, w, h, bd, n, bs, keyint, mask, ef, tsb):
    """UV_CFL_PRED (spec 7.11.5): subsampled reconstructed luma incl. the overhanging part of edge blocks, the per-plane alpha
    (least squares + neighbours), the joint decision against the luma-derived chroma mode, cfl_alpha_signs / cfl_alpha_u / _v
    syntax - on key frames; inter frames of the same chunk code without it.  The oracle's side is pinned by dav1d
    (tests/golden/*cfl*)."""
    big = [oracle.synthclip_frame(((w + 7) & ~7) + 8, ((h + 7) & ~7) + 8, bd, seed=4300 + w + bs, t=t) for t in range(n)]
    frames = [[f[0][:h, :w].copy(), f[1][:h // 2, :w // 2].copy(), f[2][:h // 2, :w // 2].copy()] for f in big]
    p = av1mi.default_params(w, h, bd, block_log2=bs, keyint=keyint, intra_mode_mask=mask, intra_edge_filter=ef, tile_sb=tsb, cfl=1)
    data, sizes, rep, recon = ctx.encode_chunk(p, b"".join(raw_of(f, bd) for f in frames), n, want_recon=True)
    cfg = oracle.default_config(w, h, bd, min_bs_log2=bs, max_bs_log2=bs, mode_mask=mask, intra_edge_filter=ef, cfl=1, tile_w_sb=tsb, tile_h_sb=tsb)
    tus, recs = oracle_chunk(oracle, cfg, frames, keyint)
    assert data == b"".join(tus)
    fb = w * h * 3 // 2 * (2 if bd > 8 else 1)
    for i, rec in enumerate(recs):
        assert recon.tobytes()[i * fb:(i + 1) * fb] == raw_of(rec, bd), "reconstruction of frame %d" % i
    if bs < 6:
        p.cfl = 0
        data0, _, _, _ = ctx.encode_chunk(p, b"".join(raw_of(f, bd) for f in frames), n)
        assert data0 != data   # chroma from luma was chosen somewhere


@pytest.mark.parametrize("w,h,bd,n,bs,keyint,mask,qm,shift", [(200, 120, 8, 1, 4, 1, 0x7, 0, 5), (202, 122, 10, 2, 3, 1, 0x1FFF, 1, 7), (264, 200, 8, 3, 4, 2, 0x1FFF, 0, 5),
                                                             (648, 360, 8, 2, 3, 240, 0x7, 1, 5)])
def test_identity_transform_search_equals_oracle(av1mi, ctx, oracle, w, h, bd, n, bs, keyint, mask, qm, shift):
    """tx_search: intra luma blocks up to 16x16 with a sparse residual (posterised source: flat areas, sharp edges) are coded with
    IDTX - identity 1-D transforms both ways, intra_tx_type symbol 0, no quantiser matrix on those blocks (spec 7.12.3) - on key
    frames and for the intra blocks of inter frames (two-wave tile walk).  The oracle's side is pinned by dav1d (tests/golden/*idtx*)."""
    big = [oracle.synthclip_frame(((w + 7) & ~7) + 8, ((h + 7) & ~7) + 8, bd, seed=4500 + w + bs, t=t) for t in range(n)]
    frames = [[(f[0][:h, :w] >> shift) << shift, (f[1][:h // 2, :w // 2] >> shift) << shift, (f[2][:h // 2, :w // 2] >> shift) << shift] for f in big]
    p = av1mi.default_params(w, h, bd, block_log2=bs, keyint=keyint, intra_mode_mask=mask, tx_search=1, enable_qm=qm, qm_min=5, qm_max=5)
    data, sizes, rep, recon = ctx.encode_chunk(p, b"".join(raw_of(f, bd) for f in frames), n, want_recon=True)
    cfg = oracle.default_config(w, h, bd, min_bs_log2=bs, max_bs_log2=bs, mode_mask=mask, tx_search=1, enable_qm=qm, qm_y=5, qm_uv=5)
    tus, recs = oracle_chunk(oracle, cfg, frames, keyint)
    assert data == b"".join(tus)
    fb = w * h * 3 // 2 * (2 if bd > 8 else 1)
    for i, rec in enumerate(recs):
        assert recon.tobytes()[i * fb:(i + 1) * fb] == raw_of(rec, bd), "reconstruction of frame %d" % i
    p.tx_search = 0
    data0, _, _, _ = ctx.encode_chunk(p, b"".join(raw_of(f, bd) for f in frames), n)
    assert data0 != data   # IDTX was chosen somewhere


@pytest.mark.parametrize("w,h,bd,n,bs,keyint,lr,tsb", [(70, 58, 8, 1, 5, 1, 0, 1), (202, 122, 10, 3, 5, 240, 0, 1), (130, 66, 8, 3, 4, 2, 1, 1),
                                                      (90, 100, 8, 3, 3, 240, 0, 1), (134, 70, 10, 2, 5, 2, 1, 2), (1366, 768 - 2, 8, 2, 5, 2, 0, 1)])
def test_sizes_that_are_not_multiples_of_8(av1mi, ctx, oracle, w, h, bd, n, bs, keyint, lr, tsb):
    """Any even frame size: coded at the next multiple of 8 (source edge-extended on the device), signalled exactly;
    references are clamped and restoration runs within the signalled size.  Frames in and reconstruction out use the
    caller's tight w x h layout.  Bit-exact against the oracle (pinned by dav1d for such sizes: tests/golden/*odd*)."""
    big = [oracle.synthclip_frame(((w + 7) & ~7) + 8, ((h + 7) & ~7) + 8, bd, seed=1200 + w, t=t) for t in range(n)]
    frames = [[f[0][:h, :w].copy(), f[1][:h // 2, :w // 2].copy(), f[2][:h // 2, :w // 2].copy()] for f in big]
    p = av1mi.default_params(w, h, bd, block_log2=bs, keyint=keyint, enable_lr=lr, tile_sb=tsb)
    data, sizes, rep, recon = ctx.encode_chunk(p, b"".join(raw_of(f, bd) for f in frames), n, want_recon=True)
    cfg = oracle.default_config(w, h, bd, min_bs_log2=bs, max_bs_log2=bs, enable_lr=lr, tile_w_sb=tsb, tile_h_sb=tsb)
    tus, recs = oracle_chunk(oracle, cfg, frames, keyint)
    assert data == b"".join(tus)
    fb = w * h * 3 // 2 * (2 if bd > 8 else 1)
    for i, rec in enumerate(recs):
        assert recon.tobytes()[i * fb:(i + 1) * fb] == raw_of(rec, bd), "reconstruction of frame %d" % i


@pytest.mark.parametrize("w,h,bd,n,bs,keyint,lr,cq", [(200, 120, 8, 2, 5, 1, 0, 30), (216, 88, 10, 3, 4, 2, 1, 40), (136, 72, 8, 3, 3, 240, 0, 20),
                                                     (130, 134, 10, 2, 5, 2, 0, 55), (640, 360, 8, 3, 5, 240, 1, 30)])
def test_deblocking_equals_oracle(av1mi, ctx, oracle, w, h, bd, n, bs, keyint, lr, cq):
    """deblock = 1: the deblocking filter runs on the reconstruction before CDEF - and, being the
    "pre-CDEF" frame, feeds the restoration filter's stripe edges; levels follow the quantiser (key frames 4 lower).
    Streams (the header carries the levels) and reconstructions bit-exact against the oracle (dav1d-pinned)."""
    big = [oracle.synthclip_frame(((w + 7) & ~7) + 8, ((h + 7) & ~7) + 8, bd, seed=1500 + w, t=t) for t in range(n)]
    frames = [[f[0][:h, :w].copy(), f[1][:h // 2, :w // 2].copy(), f[2][:h // 2, :w // 2].copy()] for f in big]
    p = av1mi.default_params(w, h, bd, block_log2=bs, keyint=keyint, enable_lr=lr, cq_level=cq, deblock=1)
    data, sizes, rep, recon = ctx.encode_chunk(p, b"".join(raw_of(f, bd) for f in frames), n, want_recon=True)
    cfg = oracle.default_config(w, h, bd, min_bs_log2=bs, max_bs_log2=bs, enable_lr=lr, base_q_idx=av1mi.cq_to_qindex(cq), deblock=1)
    tus, recs = oracle_chunk(oracle, cfg, frames, keyint)
    assert data == b"".join(tus)
    fb = w * h * 3 // 2 * (2 if bd > 8 else 1)
    for i, rec in enumerate(recs):
        assert recon.tobytes()[i * fb:(i + 1) * fb] == raw_of(rec, bd), "reconstruction of frame %d" % i
