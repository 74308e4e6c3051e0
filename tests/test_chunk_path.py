"""GPU tests of the chunk's host path: what a context keeps from one chunk to the next (header blob, default CDFs and kernel
parameters on the device), the chunk record the packing kernels fill, the
compact grid of the frame-edge tiles' symbolize variant, and the launches over part of a chunk (frames [frame0, frame0 + count):
av1-base_amd/csrc/av1mi_launch.h).  Every expectation is the oracle's bytes, or a fresh context's."""
import numpy as np
import pytest

import edge_content as E
from test_lr_chroma import clip

pytestmark = pytest.mark.gpu


def raw_of(planes, bd):
    dt = np.uint8 if bd == 8 else np.dtype("<u2")
    return b"".join(p.astype(dt).tobytes() for p in planes)


def case_of(w, h, bd, n, **params):
    return dict(name="chunk_path", w=w, h=h, bd=bd, n=n, params=params)


def run_gpu(av1mi, ctx, case, frames):
    """(bitstream, frame sizes, report, reconstruction bytes) of the chunk on `ctx`"""
    p = av1mi.default_params(case["w"], case["h"], case["bd"], **case["params"])
    data, sizes, rep, recon = ctx.encode_chunk(p, b"".join(raw_of(f, case["bd"]) for f in frames), case["n"], want_recon=True)
    assert rep.frames == case["n"] and rep.bytes == len(data) == sum(sizes)
    return data, list(sizes), rep, recon.tobytes()


def run_oracle(oracle, case, frames):
    """(temporal units, reconstruction bytes, SSE per plane over the chunk, symbols per frame) of the oracle's restatement"""
    keyint = case["params"].get("keyint", 1)
    tus, recs, sse, nsym, ref, prev = [], b"", [0, 0, 0], [], None, None
    for t, f in enumerate(frames):
        key = t % keyint == 0
        tu, rec, st = oracle.encode_frame(E.oracle_config(oracle, case, t), f, with_seq_hdr=key, ref=None if key else ref, prev_src=None if key else prev)
        tus.append(tu)
        recs += raw_of(rec, case["bd"])
        sse = [a + int(b) for a, b in zip(sse, st.sse)]
        nsym.append(int(st.n_symbols))
        ref, prev = rec, f
    return tus, recs, sse, nsym


def assert_equals_oracle(av1mi, ctx, oracle, case, frames, report=True, what="", expect=None):
    """`expect`: run_oracle's result for the chunk, where several tests share it"""
    data, sizes, rep, recon = run_gpu(av1mi, ctx, case, frames)
    tus, recs, sse, nsym = expect if expect is not None else run_oracle(oracle, case, frames)
    assert sizes == [len(t) for t in tus], what
    assert data == b"".join(tus), what
    assert recon == recs, what
    if report:
        assert [int(x) for x in rep.sse] == sse, what
        assert rep.n_symbols == sum(nsym), what
    return rep


def assert_equals_fresh_context(av1mi, ctx, case, frames, what="", scale_before=1):
    """`scale_before`: the capacity multiplier the context's earlier chunks left.  It is the one piece of a context's history that
    shows in a report by design: an overflow retry raises it and it stays raised for the context's later chunks.  The fresh context
    starts at 1 and doubles until the chunk fits, `ctx` does the same from `scale_before`, so it must report the larger of the two."""
    data, sizes, rep, recon = run_gpu(av1mi, ctx, case, frames)
    with av1mi.Context(0) as fresh:
        fdata, fsizes, frep, frecon = run_gpu(av1mi, fresh, case, frames)
    assert sizes == fsizes and data == fdata, what
    assert recon == frecon, what
    assert [int(x) for x in rep.sse] == [int(x) for x in frep.sse], what
    assert (rep.n_symbols, rep.max_tile_symbols) == (frep.n_symbols, frep.max_tile_symbols), what
    assert rep.cap_scale == max(scale_before, frep.cap_scale), what
    return rep


def flat(w, h, value):
    return [np.full((h, w), value, np.uint16), np.full((h // 2, w // 2), value, np.uint16), np.full((h // 2, w // 2), value, np.uint16)]


def test_consecutive_chunks_same_parameters_changing_content(av1mi, oracle):
    """a job's case: nothing is uploaded again after the first chunk"""
    case = case_of(200, 120, 8, 2)
    with av1mi.Context(0) as c:
        for seed in (11, 12, 13):
            assert_equals_oracle(av1mi, c, oracle, case, E.synth(oracle, 200, 120, 8, 2, seed), what="seed %d" % seed)


def test_every_cached_input_changing_in_turn(av1mi, oracle):
    """each of the inputs of the header blob, the CDF blob and the kernel parameters changes between chunks of one context, then the
    geometry (the workspace is reallocated): the context's result is a fresh context's"""
    clip = {(w, h): E.synth(oracle, w, h, 8, 4, 21) for w, h in ((136, 136), (200, 120))}
    first = dict(cq_level=30, film_grain=0, cdf_update=1, intra_mode_mask=0)
    steps = [dict(), dict(cq_level=8), dict(cq_level=50), dict(film_grain=20), dict(cdf_update=0), dict(cdf_update=1),
             dict(intra_mode_mask=0x1FFF), dict(n=4), dict(n=2), dict(first, n=1),
             dict(size=(200, 120)), dict(size=(136, 136))]
    state = dict(first, n=1, size=(136, 136))
    scale = 1
    with av1mi.Context(0) as c:
        for i, step in enumerate(steps):
            state.update(step)
            params = {k: v for k, v in state.items() if k not in ("n", "size")}
            (w, h), n = state["size"], state["n"]
            scale = assert_equals_fresh_context(av1mi, c, case_of(w, h, 8, n, **params), clip[(w, h)][:n], what="step %d: %s" % (i, step),
                                                scale_before=scale).cap_scale


def test_strength_search_uploads_its_headers_every_chunk(av1mi, oracle):
    """cdef_search: cdef_select_kernel writes the strengths into the frame headers on the device, so the device's blob is not the one
    uploaded and an equal blob on the host is no reason to skip the upload"""
    case = case_of(200, 120, 8, 2, cdef_search=4)
    scale = 1
    with av1mi.Context(0) as c:
        for seed in (31, 32):
            scale = assert_equals_fresh_context(av1mi, c, case, E.synth(oracle, 200, 120, 8, 2, seed), what="seed %d" % seed, scale_before=scale).cap_scale
        # ... and the search going off leaves headers on the device that no upload put there
        assert_equals_fresh_context(av1mi, c, case_of(200, 120, 8, 2), E.synth(oracle, 200, 120, 8, 2, 32), what="search off", scale_before=scale)


def test_small_and_large_chunks_alternating(av1mi, oracle):
    """the bitstream buffer is sized by the chunk record alone: a flat chunk at CQ 50, a chunk of far more bytes at CQ 8 (it may outgrow
    the x1 tile capacities and re-run) and at CQ 30 (it must fit them), each twice, in turn on one context"""
    w, h, n = 200, 120, 2
    small = (case_of(w, h, 8, n, cq_level=50), [flat(w, h, 128)] * n)
    large = (case_of(w, h, 8, n, cq_level=8), E.synth(oracle, w, h, 8, n, 41))
    medium = (case_of(w, h, 8, n, cq_level=30), large[1])
    for big, fits in ((large, False), (medium, True)):
        reps = []
        with av1mi.Context(0) as c:
            for i, (case, frames) in enumerate((small, big, small, big)):
                reps.append(assert_equals_oracle(av1mi, c, oracle, case, frames, what="cq %d chunk %d" % (big[0]["params"]["cq_level"], i)))
        assert reps[1].bytes > 2 * reps[0].bytes and reps[3].bytes == reps[1].bytes and reps[0].cap_scale == 1
        if fits:
            assert reps[1].cap_scale == 1


def test_overflow_retry_after_a_small_chunk(av1mi, oracle):
    """64x64 tiles of noise at CQ 4 outgrow the x1 capacities (the recipe of test_stress_carries_and_long_tiles) on a context that has
    already encoded a small chunk: the overflow is found in the chunk record, the chunk re-runs at the next multiplier"""
    rng = np.random.default_rng(99)
    w, h, n = 328, 248, 6
    noise = [[rng.integers(0, 256, (h, w)).astype(np.uint16), rng.integers(0, 256, (h // 2, w // 2)).astype(np.uint16),
              rng.integers(0, 256, (h // 2, w // 2)).astype(np.uint16)] for _ in range(n)]
    case = case_of(w, h, 8, n, cq_level=4, block_log2=5)
    with av1mi.Context(0) as c:
        rep = assert_equals_oracle(av1mi, c, oracle, case, [flat(w, h, 128)] * n, what="flat")
        assert rep.cap_scale == 1
        for i in range(2):   # the retry, then the same chunk at the raised multiplier from the start
            rep = assert_equals_oracle(av1mi, c, oracle, case, noise, what="noise %d" % i)
            assert rep.max_tile_symbols > 16384 and rep.cap_scale > 1


REM = (0, 8, 16, 24, 32, 40, 48, 56)


def edge_grid_check(av1mi, ctx, oracle, w, h, n=2, seed=51, **params):
    assert_equals_oracle(av1mi, ctx, oracle, case_of(w, h, 8, n, **params), E.synth(oracle, w, h, 8, n, seed), report=False,
                         what="%dx%d %s" % (w, h, params))


@pytest.mark.parametrize("bs", [5, 4])
@pytest.mark.parametrize("w0", [64, 128])
@pytest.mark.parametrize("r", REM)
def test_edge_tile_grid(av1mi, ctx, oracle, w0, r, bs):
    """frame sizes whose last superblock row / column forces splits (the full variant's tiles, launched over the frames' edge tiles
    only) or does not (no launch), one and two tile columns, two frames: the second frame's tiles are found through the compact grid"""
    for r2 in REM:
        edge_grid_check(av1mi, ctx, oracle, w0 + r, 64 + r2, block_log2=bs)


@pytest.mark.parametrize("w0", [64, 128])
@pytest.mark.parametrize("params", [dict(block_log2=6), dict(block_log2=5, cdf_update=0)], ids=["bs6", "static"])
def test_edge_tile_grid_64x64_leaves_and_static_cdfs(av1mi, ctx, oracle, w0, params):
    for r in (0, 24, 40, 56):
        for r2 in (0, 8, 40, 48):
            edge_grid_check(av1mi, ctx, oracle, w0 + r, 64 + r2, **params)


@pytest.mark.parametrize("w,h,n,params", [
    (328, 248, 2, dict(tile_sb=2)),                                  # tiles of 2 x 2 superblocks, the last row and column one short
    (168, 104, 3, dict(keyint=240)), (152, 120, 3, dict(keyint=240, block_log2=4)),   # key + inter launches of both variants
    (168, 104, 2, dict(partition_search=1, min_block_log2=3))],      # split masks on the device: both variants over the whole grid
    ids=["tile_sb2", "inter", "inter_bs4", "partition"])
def test_edge_tile_grid_other_launches(av1mi, ctx, oracle, w, h, n, params):
    edge_grid_check(av1mi, ctx, oracle, w, h, n=n, **params)


def test_report_symbol_counts_come_from_the_chunk_record(av1mi, ctx, oracle):
    """one tile per frame: the longest tile is the largest frame, the total their sum"""
    case = case_of(64, 64, 8, 3)
    frames = [oracle.synthclip_frame(64, 64, 8, seed=61, t=t, scene_len=1) for t in range(3)]
    data, sizes, rep, recon = run_gpu(av1mi, ctx, case, frames)
    nsym = run_oracle(oracle, case, frames)[3]
    assert len(set(nsym)) > 1
    assert rep.max_tile_symbols == max(nsym) and rep.n_symbols == sum(nsym)


# Launches over part of a chunk, at the smallest frame with more than one superblock each way and a partial last row and column
# (136 x 72: 3 x 2 superblocks); content whose restoration units choose off, Wiener and self-guided filters.
RANGE_CASES = {
    # frames 1, 2, 3 are inter launches at frame0 = 1, 2, 3: split masks, sub-sample keys, the inter frames' deblocking levels,
    # restoration choices and sums per frame
    "inter_10bit": case_of(136, 72, 10, 4, keyint=240, deblock=1, subpel=1, me_presearch=1, partition_search=1, min_block_log2=3, enable_lr=2,
                           enable_qm=1, qm_min=1),
    # key-frame launches at frame0 = 2 and 4 inside an inter chunk; the 64x64 reconstruction units, tiles of two superblocks
    "keys_8bit": case_of(136, 72, 8, 5, keyint=2, block_log2=6, deblock=1, enable_lr=1, tile_sb=2),
}


@pytest.fixture(scope="module")
def range_cases(oracle):
    """name -> (case, frames, the oracle's chunk)"""
    out = {}
    for name, case in RANGE_CASES.items():
        frames = clip(oracle, case["w"], case["h"], case["bd"], case["n"], seed=61)
        out[name] = (case, frames, run_oracle(oracle, case, frames))
    return out


@pytest.mark.parametrize("group", [None, "2"], ids=["one_group", "groups_of_2"])
def test_inter_launches_at_every_frame_of_a_chunk(av1mi, ctx, oracle, range_cases, monkeypatch, group):
    """... and with AV1MI_ENTROPY_GROUP = 2 the entropy coder's ranges: frames [0, 2) on the third stream, [2, 4) after the chain"""
    if group is not None:
        monkeypatch.setenv("AV1MI_ENTROPY_GROUP", group)
    case, frames, expect = range_cases["inter_10bit"]
    assert_equals_oracle(av1mi, ctx, oracle, case, frames, expect=expect)


def test_key_frame_launches_inside_an_inter_chunk(av1mi, ctx, oracle, range_cases):
    case, frames, expect = range_cases["keys_8bit"]
    assert_equals_oracle(av1mi, ctx, oracle, case, frames, expect=expect)


def test_frame_ranges_on_a_reused_context(av1mi, oracle, range_cases):
    """both chunks in turn, twice, on one context: the parameters a context keeps (and the block cached on the device) are the chunk's,
    never a launch's range of it"""
    with av1mi.Context(0) as c:
        for turn in range(2):
            for name in ("inter_10bit", "keys_8bit"):
                case, frames, expect = range_cases[name]
                assert_equals_oracle(av1mi, c, oracle, case, frames, what="turn %d: %s" % (turn, name), expect=expect)
