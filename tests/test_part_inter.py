"""partition_search = 2 on the GPU: inter frames are partitioned bottom up from the motion search's node costs.
The masks and leaf keys of every inter frame equal tests/part_inter_ref.py's brute-force restatement (tests/test_part_inter_content.py
asserts on the CPU that these inputs split, keep, force and tie at every level); where nothing is to decide, and on a pure pan, the bytes
equal the oracle's; dav1d decodes the streams to the encoder's reconstruction; the value 3 is refused."""
import numpy as np
import pytest

import edge_content as E
import part_inter_ref as PR
from test_gpu_parity import oracle_chunk, raw_of

pytestmark = pytest.mark.gpu


def encode(av1mi, ctx, case, frames, mode, **more):
    p = av1mi.default_params(case["w"], case["h"], case["bd"], keyint=240, partition_search=mode, cq_level=case["cq"], **dict(case["params"], **more))
    n = len(frames)
    data, sizes, rep, recon = ctx.encode_chunk(p, b"".join(raw_of(f, case["bd"]) for f in frames), n, want_recon=True)
    return data, list(sizes), recon, ctx.inter_partition_result(n)


def centres_of(keys_f, sbr, sbc):
    """the superblocks' centre codes from the frame's keys: the first unit of the superblock that holds a key"""
    out = np.zeros((sbr, sbc), np.uint32)
    for r in range(sbr):
        for c in range(sbc):
            blk = keys_f[8 * r:8 * r + 8, 8 * c:8 * c + 8].ravel()
            real = blk[blk != np.uint64(PR.ALL_ONES)]
            out[r, c] = int(real[0]) >> 40 if len(real) else 0
    return out


def assert_inter_frames_equal_the_reference(case, frames, masks2, keys2):
    """masks and leaf keys of every inter frame against part_inter_ref.reference_frame, the centres taken from the keys"""
    p = case["params"]
    sbr, sbc = masks2.shape[1:]
    acq = PR.case_ac_q(case)
    for t in range(1, len(frames)):
        cen = centres_of(keys2[t], sbr, sbc)
        if not p.get("me_presearch"):
            assert not cen.any()
        want_masks, want_keys = PR.reference_frame(frames[t][0].astype(np.int32), frames[t - 1][0].astype(np.int32), p.get("me_range", 8),
                                                   p["min_block_log2"], p["block_log2"], acq, cen)
        assert np.array_equal(masks2[t], want_masks), (t, [hex(int(x)) for x in masks2[t].ravel()], [hex(int(x)) for x in want_masks.ravel()])
        # every leaf's key, centre code included: all leaves of a superblock carry the superblock's code
        bad = [(u, hex(int(keys2[t][u])), hex(k)) for u, k in want_keys.items() if int(keys2[t][u]) != k]
        assert not bad, (t, bad[:8])


@pytest.mark.parametrize("case", PR.CASES, ids=[c["name"] for c in PR.CASES])
def test_masks_and_leaf_keys_equal_the_reference(av1mi, ctx, case):
    frames = PR.make_frames(case)
    _, _, _, (masks1, _) = encode(av1mi, ctx, case, frames, 1)
    _, _, _, (masks2, keys2) = encode(av1mi, ctx, case, frames, 2)
    assert np.array_equal(masks2[0], masks1[0])   # the key frame keeps the source rule
    assert_inter_frames_equal_the_reference(case, frames, masks2, keys2)


@pytest.mark.parametrize("me_range", [8, 16])
@pytest.mark.parametrize("bd", [8, 10])
def test_every_instantiation_of_the_node_search_equals_the_reference(av1mi, ctx, bd, me_range):
    """the node-mode search is built per sample type and range; the cases above reach (8-bit, 8) and (10-bit, 16).  The 72x56 case - two
    superblocks, four frames - at every combination; what its content ties on is the content test's matter, not this one's"""
    base = next(c for c in PR.CASES if c["name"] == "72x56")
    case = dict(base, bd=bd, params=dict(base["params"], me_range=me_range))
    frames = PR.make_frames(case)
    _, _, _, (masks2, keys2) = encode(av1mi, ctx, case, frames, 2)
    assert_inter_frames_equal_the_reference(case, frames, masks2, keys2)


@pytest.mark.parametrize("bs", [5, 6])
def test_nothing_to_decide_equals_mode_1_and_the_oracle(av1mi, ctx, oracle, bs):
    w, h, bd, n = 200, 136, 8, 3
    frames = [oracle.synthclip_frame(w, h, bd, seed=2200 + bs, t=2 * t) for t in range(n)]
    case = dict(w=w, h=h, bd=bd, cq=30, params=dict(block_log2=bs, min_block_log2=bs))
    d1, s1, r1, _ = encode(av1mi, ctx, case, frames, 1)
    d2, s2, r2, _ = encode(av1mi, ctx, case, frames, 2)
    assert d2 == d1 and s2 == s1 and r2.tobytes() == r1.tobytes()
    cfg = oracle.default_config(w, h, bd, min_bs_log2=bs, max_bs_log2=bs, partition_search=1)
    tus, recs = oracle_chunk(oracle, cfg, frames, 240)
    assert d2 == b"".join(tus) and s2 == [len(t) for t in tus]
    assert r2.tobytes() == b"".join(raw_of(r, bd) for r in recs)


def pan_frames(w, h, n):
    rng = np.random.default_rng(31)
    big = rng.integers(64, 193, (h + n + 2, w + 3 * n + 6)).astype(np.uint16)
    out = []
    for t in range(n):
        oy, ox = n - t, 3 * (n - t)
        y = big[oy:oy + h, ox:ox + w]
        c = np.full((h // 2, w // 2), 128, np.uint16)
        out.append([y.copy(), c, c.copy()])
    return out


def test_pure_pan_codes_as_fixed_64x64(av1mi, ctx, oracle):
    """uniform noise: the source rule leaves the key frame unsplit; the P frames are a pan of (3, 1), which every node matches with the
    same vector - no node splits, and the bytes are the oracle's with fixed 64x64 leaves"""
    w, h, bd, n = 192, 128, 8, 3
    frames = pan_frames(w, h, n)
    case = dict(w=w, h=h, bd=bd, cq=30, params=dict(block_log2=6, min_block_log2=3))
    d2, s2, r2, (masks, _) = encode(av1mi, ctx, case, frames, 2)
    assert not masks.any()
    tus, recs = oracle_chunk(oracle, oracle.default_config(w, h, bd, min_bs_log2=6, max_bs_log2=6), frames, 240)
    assert d2 == b"".join(tus) and s2 == [len(t) for t in tus]
    assert r2.tobytes() == b"".join(raw_of(r, bd) for r in recs)


@pytest.mark.parametrize("ci,extra,group", [(0, dict(subpel=1, deblock=2, cdef_search=2, enable_lr=4), None), (1, dict(), "2")])
def test_dav1d_decodes_to_the_reconstruction(av1mi, monkeypatch, ci, extra, group):
    """200x136 with subpel, deblock = 2, cdef_search and enable_lr = 4; 264x200 with tile_sb = 2 and AV1MI_ENTROPY_GROUP = 2.  (The second
    case also pins symbolize's handling of a tile that holds 64-point and 32-point luma transforms, which share their range CDFs: with a
    slot each the key frame of this clip came out one byte off the oracle's and dav1d did not decode it to the reconstruction.)"""
    import oracle_avif
    if not oracle_avif.have_libavif():
        pytest.skip("libavif (dav1d) is not available on this machine")
    if group:
        monkeypatch.setenv("AV1MI_ENTROPY_GROUP", group)
    case = PR.CASES[ci]
    frames = PR.make_frames(case)
    w, h, bd, n = case["w"], case["h"], case["bd"], len(frames)
    with av1mi.Context(0) as c:
        data, sizes, recon, (masks, _) = encode(av1mi, c, case, frames, 2, **extra)
    assert masks[1:].any()
    from test_edges import split_frames
    want = split_frames(recon, w, h, bd, n)
    tus, off = [], 0
    for s in sizes:
        tus.append(data[off:off + s])
        off += s
    assert E.decodes_to(E.dav1d_decode(tus, w, h, bd, 240), want, bd, 0) is None


def test_mode_1_key_frame_in_two_superblock_tiles_equals_the_oracle(av1mi, ctx, oracle):
    """partition_search = 1, one key frame, tile_sb = 2, leaves 4...6: a tile of 2 x 2 superblocks that holds a 64x64 leaf beside a split
    superblock codes 64-point and 32-point luma transforms, whose range CDFs are one - symbolize must adapt them in one copy.  The
    stream and the reconstruction equal the oracle's."""
    w, h, bd = 264, 200, 10
    frame = oracle.synthclip_frame(w, h, bd, seed=77, t=0)
    p = av1mi.default_params(w, h, bd, tile_sb=2, partition_search=1, block_log2=6, min_block_log2=4, cq_level=30)
    data, sizes, rep, recon = ctx.encode_chunk(p, raw_of(frame, bd), 1, want_recon=True)
    cfg = oracle.default_config(w, h, bd, tile_w_sb=2, tile_h_sb=2, min_bs_log2=4, max_bs_log2=6, partition_search=1, base_q_idx=120)
    tu, rec, st = oracle.encode_frame(cfg, frame)
    assert st.bs_hist[6] and st.bs_hist[5]   # both leaf sizes occur
    assert data == tu and recon.tobytes() == raw_of(rec, bd)


def test_value_3_is_refused(av1mi, ctx):
    p = av1mi.default_params(200, 136, 8, keyint=240, partition_search=3, block_log2=6, min_block_log2=3)
    frames = PR.make_frames(PR.CASES[0])
    with pytest.raises(av1mi.EncodeFailed) as e:
        ctx.encode_chunk(p, b"".join(raw_of(f, 8) for f in frames), len(frames))
    assert e.value.code == av1mi.E_INVALID_ARG
