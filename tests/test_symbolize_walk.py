"""GPU tests of the symbolize kernel's block walk and literal runs (the walk steps from leaf origin to leaf origin, a run
of literal bits goes out with one store, a coefficient's range symbols with predicated stores) and of the same walk in the
reconstruction kernel (§4.2): bitstream, reconstruction and SSE equal the oracle's, bit for bit.

Walk: fixed leaves of 8, 16, 32 and 64 samples (a step of 1, 4, 16 and 64 units) and the content-driven partition with leaves 8 .. 64
on `mixed` - superblocks that are flat (one 64x64 leaf), and superblocks cut into 32x32, 16x16 and 8x8 leaves - at 64x64, 128x128, 72x88 and
200x136 (superblocks with units outside the frame and leaves forced smaller at the edge), key-frame and IPPP chunks, 8 and 10 bit, and
tiles of 2 x 2 superblocks (the partition there with adaptive and with static CDFs).  Literal runs: noise at the lowest quantiser index (DC levels above 14: the Golomb tail) and
`eob_ladder`, blocks whose spectrum ends at a chosen scan position (every eob_extra length); a flat frame at the highest (no run at all).
tests/test_symbolize_walk_content.py asserts on the CPU that these inputs do what they are for.

The oracle has no per-superblock cdef_idx, no delta_q and no fitted restoration units, so the three runs behind them - the cdef_idx
bits, the delta_q remainder / abs / sign bits, the units' bit strings - have dav1d (libavif) as their reference, as in tests/test_aq.py,
tests/test_cdef_search.py and tests/test_wiener_fit.py: it decodes the stream to the reconstruction in every plane.  One case overflows
a tile's stream capacity; the retried chunk equals the oracle."""
import numpy as np
import pytest

import edge_content as E
from test_edges import encode
from test_recon_trim import check, flat, noise

pytestmark = pytest.mark.gpu

SIZES = [(64, 64), (128, 128), (72, 88), (200, 136)]
PART = dict(partition_search=1, min_block_log2=3, block_log2=6)


def mixed(w, h, bd, t, seed=7):
    """Flat and sample noise by area, for a partition search that splits a node whose quadrants differ in activity.
    Superblocks alternate (with their raster position and t) between all flat - one 64x64 leaf - and: top left quadrant flat, top
    right noise (32x32 leaves); bottom left noise in its first 16x16 block only (16x16 leaves); bottom right noise in its first 8x8
    unit only (that 16x16 block in 8x8 leaves, the others whole).  Chroma follows luma at half the scale."""
    rng = np.random.default_rng(seed + 31 * t)
    mx = E.maxv_of(bd)
    out = []
    for sh in (0, 1, 1):
        ph, pw = h >> sh, w >> sh
        Y, X = np.mgrid[0:ph, 0:pw]
        Xl, Yl = X << sh, Y << sh
        cut = ((Xl // 64 + Yl // 64 + t) & 1) == 1
        quad = ((Xl // 32) & 1) | (((Yl // 32) & 1) << 1)
        lx, ly = Xl % 32, Yl % 32
        busy = cut & ((quad == 1) | ((quad == 2) & (lx < 16) & (ly < 16)) | ((quad == 3) & (lx < 8) & (ly < 8)))
        out.append(np.where(busy, rng.integers(0, mx + 1, (ph, pw)), mx // 2 + 8 * sh).astype(np.uint16))
    return out


def eob_ladder(w, h, bd, t):
    """flat, plus in every 32x32 luma block (16x16 chroma block) the inverse DCT of a spectrum whose last coefficient, in scan order, is
    number ladder_last() - stepping over the blocks, planes and frames - so that the blocks' eob covers every eob_extra length"""
    f = flat(w, h, bd)
    amp = 64 << (bd - 8)
    for pl, n in ((0, 32), (1, 16), (2, 16)):
        ph, pw = f[pl].shape
        plane = f[pl].astype(np.float64)
        for by in range(0, ph, n):
            for bx in range(0, pw, n):
                last = ladder_last(bx // n, by // n, pl, n, t)
                r, c = scan_rc(last, n)
                y, x = np.mgrid[0:n, 0:n]
                wave = np.cos(np.pi * (2 * y + 1) * r / (2 * n)) * np.cos(np.pi * (2 * x + 1) * c / (2 * n))
                blk = plane[by:by + n, bx:bx + n]
                blk += (amp * wave)[:blk.shape[0], :blk.shape[1]]
        f[pl] = np.clip(np.rint(plane), 0, E.maxv_of(bd)).astype(np.uint16)
    return f


def ladder_last(bx, by, pl, n, t):
    """scan index of the block's last coefficient: 2^k + 1 + (a little), k = 1 .. log2(n * n) - 1, i.e. eob = that + 1 in (2^k + 1, 2^(k + 1)]"""
    kmax = 2 * int(np.log2(n)) - 1
    k = 1 + (bx + 2 * by + 3 * t + pl) % kmax
    return (1 << k) + ((bx + by + t) % (1 << (k - 1)) if k > 1 else 0) + 1


def scan_rc(idx, n):
    """(row, column) of scan index idx in the default zig-zag of an n x n block (anti-diagonals; odd ones by increasing row)"""
    pos = sorted((((i + j) << 8) | (i if (i + j) & 1 else j), i, j) for i in range(n) for j in range(n))
    return pos[idx][1], pos[idx][2]


def alternating(w, h, bd, t):
    """superblocks alternate between flat and sample noise: the activity map puts them at the two ends of the delta_q range"""
    rng = np.random.default_rng(11 + t)
    mx = E.maxv_of(bd)
    out = []
    for sh in (0, 1, 1):
        ph, pw = h >> sh, w >> sh
        Y, X = np.mgrid[0:ph, 0:pw]
        busy = ((((X << sh) // 64) + ((Y << sh) // 64) + t) & 1) == 1
        out.append(np.where(busy, rng.integers(0, mx + 1, (ph, pw)), mx // 2).astype(np.uint16))
    return out


def walk_case(w, h, bd, keyint, params, tag):
    n = 3 if keyint > 1 else 2
    return dict(name="walk_%s_%dx%d_%db_k%d" % (tag, w, h, bd, keyint), w=w, h=h, bd=bd, n=n, params=dict(params, keyint=keyint))


def walk_frames(case):
    return [mixed(case["w"], case["h"], case["bd"], t) for t in range(case["n"])]


LEAVES = [("bs%d" % b, dict(block_log2=b)) for b in (3, 4, 5, 6)] + [("part", dict(PART))]


@pytest.mark.parametrize("keyint", [1, 3], ids=["key", "ippp"])
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("tag,params", LEAVES, ids=[t for t, _ in LEAVES])
@pytest.mark.parametrize("w,h", SIZES)
def test_walk_equals_the_oracle(av1mi, ctx, oracle, w, h, tag, params, bd, keyint):
    case = walk_case(w, h, bd, keyint, dict(params, subpel=1) if keyint > 1 else params, tag)
    check(av1mi, ctx, oracle, case, walk_frames(case))


@pytest.mark.parametrize("params", [dict(block_log2=4), dict(PART), dict(PART, cdf_update=0)], ids=["bs4", "part", "part_static"])
def test_walk_in_tiles_of_two_by_two_superblocks(av1mi, ctx, oracle, params):
    case = walk_case(200, 136, 10, 3, dict(params, tile_sb=2), "tile2")
    check(av1mi, ctx, oracle, case, walk_frames(case))


@pytest.mark.parametrize("bd", [8, 10])
def test_literal_runs_equal_the_oracle(av1mi, ctx, oracle, bd):
    w, h, n = 128, 96, 2
    rng = np.random.default_rng(bd)
    contents = [
        ("noise_cq1", dict(cq_level=1), [noise(rng, w, h, bd, t) for t in range(n)]),
        ("ladder_cq30", dict(cq_level=30, intra_mode_mask=1), [eob_ladder(w, h, bd, t) for t in range(n)]),
        ("flat_cq63", dict(cq_level=63), [flat(w, h, bd) for t in range(n)]),
    ]
    sizes = {}
    for name, extra, frames in contents:
        case = dict(name="%s_%db" % (name, bd), w=w, h=h, bd=bd, n=n, params=extra)
        sizes[name] = check(av1mi, ctx, oracle, case, frames)
    assert sizes["flat_cq63"] < sizes["ladder_cq30"] < sizes["noise_cq1"]


def decoded_by_dav1d(av1mi, case, frames):
    import oracle_avif
    if not oracle_avif.have_libavif():
        pytest.skip("libavif (dav1d) is not available on this machine")
    with av1mi.Context(0) as c:
        tus, recs, rep = encode(av1mi, c, case, frames)
        extra = c.lr_wiener_fit_result(case["n"])[0] if case["params"].get("enable_lr") else None
    got = E.dav1d_decode(tus, case["w"], case["h"], case["bd"], case["params"].get("keyint", 1))
    assert E.decodes_to(got, recs, case["bd"], 0) is None, case["name"]
    return rep, extra


@pytest.mark.parametrize("keyint", [1, 3], ids=["key", "ippp"])
def test_cdef_idx_bits_decode(av1mi, oracle, keyint):
    w, h, bd, n = 200, 136, 10, 3
    case = dict(name="cdef_idx", w=w, h=h, bd=bd, n=n, params=dict(cdef_search=4, keyint=keyint))
    decoded_by_dav1d(av1mi, case, E.synth(oracle, w, h, bd, n, 1080))


@pytest.mark.parametrize("keyint", [1, 3], ids=["key", "ippp"])
def test_delta_q_bits_decode(av1mi, oracle, keyint):
    w, h, bd, n = 200, 136, 8, 3
    case = dict(name="delta_q", w=w, h=h, bd=bd, n=n, params=dict(keyint=keyint, cq_level=av1mi.cq_aq(30, 4)))   # strength 4 beside the CQ level
    decoded_by_dav1d(av1mi, case, [alternating(w, h, bd, t) for t in range(n)])


@pytest.mark.parametrize("bd", [8, 10])
def test_restoration_unit_bits_decode(av1mi, oracle, bd):
    from test_lr_chroma import clip
    w, h, n = 200, 136, 2
    p = av1mi.default_params(w, h, bd, enable_lr=2, lr_fit=True, lr_wiener_fit=True)
    case = dict(name="lr_units", w=w, h=h, bd=bd, n=n, params=dict(enable_lr=p.enable_lr))
    rep, units = decoded_by_dav1d(av1mi, case, clip(oracle, w, h, bd, n, seed=40 + w))
    choice = np.asarray(units)[:, 0, :, :, 0].ravel()   # the luma units' final choices: 1 .. 3 and 23 Wiener, 4 .. 22 self-guided
    assert ((choice >= 4) & (choice <= 22)).any() and ((choice == 23) | ((choice >= 1) & (choice <= 3))).any(), sorted(set(choice.tolist()))


def test_stream_overflow_is_retried_and_equals_the_oracle(av1mi, oracle):
    """64x64 tiles of noise at CQ 4 outgrow a fresh context's stream capacity (tests/test_gpu_parity.py reaches it the same way): entries
    beyond the capacity are not written, the length still counts them, the chunk is run again at a larger capacity"""
    w, h, bd, n = 200, 136, 8, 2
    rng = np.random.default_rng(99)
    frames = [[rng.integers(0, 256, (h >> s, w >> s)).astype(np.uint16) for s in (0, 1, 1)] for _ in range(n)]
    case = dict(name="overflow", w=w, h=h, bd=bd, n=n, params=dict(cq_level=4, block_log2=5))
    with av1mi.Context(0) as c:
        tus, recs, rep = encode(av1mi, c, case, frames)
    assert rep.max_tile_symbols > 16384 and rep.cap_scale > 1
    otus, orecs, osse = E.oracle_encode(oracle, case, frames)
    assert tus == otus
    assert all(np.array_equal(a[pl], b[pl]) for a, b in zip(recs, orecs) for pl in range(3))
    assert [int(x) for x in rep.sse] == osse
