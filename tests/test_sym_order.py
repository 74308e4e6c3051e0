"""GPU tests of the order symbolize takes a key-frame chunk's tiles in (the reconstruction wave sums its tile's eobs,
the sum picks one of 16 classes - av1-base_amd/csrc/tile_weight_rule.h - and symbolize walks the classes from the heaviest down).

Every case encodes with AV1MI_SYM_ORDER=1 and =0 in fresh contexts (the variable is read when a context is made): bitstream, frame
sizes, reconstruction and SSE are equal, and equal to the oracle's.  With the order on, Context.sym_order_result is a permutation of
the chunk's tiles whose classes never increase along it.  Shapes, all 10 bit: fewer tiles than classes, an overhanging bottom row,
one tile, a frame whose tiles are either sample noise or flat (the two ends of the classes and nothing between - the noise tiles come
first; tests/test_sym_order_content.py asserts on the CPU that these inputs do that), the same frame at the highest and the lowest
quantiser index, and an all-flat frame (every tile in class 0).  Inter chunks, static CDFs, tiles of 2 x 2 superblocks and 64x64
leaves keep natural order whatever the variable says; a second chunk of another size on one context equals a fresh context's."""
import os

import numpy as np
import pytest

import edge_content as E
from test_edges import encode

pytestmark = pytest.mark.gpu

TOP = 15


def synth(oracle, w, h, n, seed=1080):
    return E.synth(oracle, w, h, 10, n, seed)


def flat_mid(w, h, bd=10):
    """every plane at 1 << (bd - 1), what a tile's first block is predicted with: no residual anywhere"""
    mid = 1 << (bd - 1)
    return [np.full((h, w), mid, np.uint16), np.full((h // 2, w // 2), mid, np.uint16), np.full((h // 2, w // 2), mid, np.uint16)]


def noise_tiles(w, h, t):
    """the 64x64 regions (= tiles) of frame t that are noise: one per frame, moving along the first row"""
    return [t % (w // 64)]


def noise_island(w, h, t, bd=10):
    """flat_mid with one 64x64 region of full-range sample noise in every plane (tile t % tile columns of the first tile row)"""
    rng = np.random.default_rng(300 + t)
    f = flat_mid(w, h, bd)
    x0 = noise_tiles(w, h, t)[0] * 64
    for pl, sh in ((0, 0), (1, 1), (2, 1)):
        f[pl][0:64 >> sh, x0 >> sh:(x0 + 64) >> sh] = rng.integers(0, 1 << bd, (64 >> sh, 64 >> sh))
    return f


def with_order(av1mi, knob, fn):
    """fn(context) on a fresh context made with AV1MI_SYM_ORDER=knob"""
    old = os.environ.get("AV1MI_SYM_ORDER")
    os.environ["AV1MI_SYM_ORDER"] = str(knob)
    try:
        with av1mi.Context(0) as c:
            return fn(c)
    finally:
        if old is None:
            del os.environ["AV1MI_SYM_ORDER"]
        else:
            os.environ["AV1MI_SYM_ORDER"] = old


def run(av1mi, knob, case, frames):
    def go(c):
        tus, recs, rep = encode(av1mi, c, case, frames)
        return tus, recs, [int(x) for x in rep.sse], c.sym_order_result()
    return with_order(av1mi, knob, go)


def same(a, b):
    return a[0] == b[0] and a[2] == b[2] and all(np.array_equal(x[pl], y[pl]) for x, y in zip(a[1], b[1]) for pl in range(3))


def both_orders_equal_the_oracle(av1mi, oracle, case, frames):
    """the two encodes' outputs are equal and the oracle's; returns (order, classes) of the weighted encode"""
    on, off = run(av1mi, 1, case, frames), run(av1mi, 0, case, frames)
    assert [len(t) for t in on[0]] == [len(t) for t in off[0]], case["name"]
    assert same(on, off), case["name"]
    otus, orecs, osse = E.oracle_encode(oracle, case, frames)
    assert same(on, (otus, orecs, osse)), case["name"]
    assert off[3] is None, case["name"]
    return on[3]


def n_tiles(case):
    return case["n"] * (-(-case["w"] // 64)) * (-(-case["h"] // 64))


def check_table(case, res):
    assert res is not None, case["name"]
    order, classes = res
    n = n_tiles(case)
    assert sorted(order.tolist()) == list(range(n)), case["name"]
    along = classes[order].astype(int)
    assert classes.max() <= TOP and (np.diff(along) <= 0).all(), (case["name"], along.tolist())
    return order, classes


CASES = [
    dict(name="six_tiles", w=128, h=64, n=3),
    dict(name="overhang", w=192, h=136, n=2),
    dict(name="one_tile", w=64, h=64, n=1),
]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_weighted_order_changes_no_byte(av1mi, oracle, case):
    case = dict(case, bd=10, params={})
    res = both_orders_equal_the_oracle(av1mi, oracle, case, synth(oracle, case["w"], case["h"], case["n"]))
    check_table(case, res)


ISLAND = dict(w=256, h=128, n=2, bd=10)


def island_frames():
    return [noise_island(ISLAND["w"], ISLAND["h"], t) for t in range(ISLAND["n"])]


def island_noise_ids():
    per = (ISLAND["w"] // 64) * (ISLAND["h"] // 64)
    return sorted(t * per + k for t in range(ISLAND["n"]) for k in noise_tiles(ISLAND["w"], ISLAND["h"], t))


@pytest.mark.parametrize("cq", [30, 1, 63], ids=["cq30", "lowest_cq", "cq63"])
def test_noise_tiles_come_first(av1mi, oracle, cq):
    """noise in one tile of a frame, flat elsewhere: the flat tiles are class 0 at every quantiser; the noise tiles are the top class at
    CQ 30 and at the lowest CQ (where every coefficient position is coded: the largest sum there is), and even the coarsest quantiser
    leaves full-range noise levels, so they stay ahead of the flat tiles there (tests/test_sym_order_content.py)"""
    case = dict(ISLAND, name="island_cq%d" % cq, params=dict(cq_level=cq, intra_mode_mask=1))
    order, classes = check_table(case, both_orders_equal_the_oracle(av1mi, oracle, case, island_frames()))
    noisy = island_noise_ids()
    assert sorted(order[:len(noisy)].tolist()) == noisy, order.tolist()
    rest = np.setdiff1d(np.arange(n_tiles(case)), noisy)
    assert (classes[rest] == 0).all(), classes.tolist()
    if cq != 63:
        assert (classes[noisy] == TOP).all(), classes.tolist()   # classes 0 and top occupied, the ones between empty
    else:
        assert (classes[noisy] > 0).all(), classes.tolist()


def test_all_tiles_in_class_zero(av1mi, oracle):
    case = dict(name="flat_cq63", w=256, h=128, n=2, bd=10, params=dict(cq_level=63))
    order, classes = check_table(case, both_orders_equal_the_oracle(av1mi, oracle, case, [flat_mid(256, 128) for _ in range(2)]))
    assert (classes == 0).all()


OUT_OF_SCOPE = [("inter", dict(keyint=240)), ("static_cdf", dict(cdf_update=0)), ("tile_sb2", dict(tile_sb=2)), ("bs6", dict(block_log2=6))]


@pytest.mark.parametrize("tag,params", OUT_OF_SCOPE, ids=[t for t, _ in OUT_OF_SCOPE])
def test_out_of_scope_chunks_keep_natural_order(av1mi, oracle, tag, params):
    case = dict(name=tag, w=128, h=64, n=3, bd=10, params=params)
    frames = synth(oracle, 128, 64, 3)
    on, off = run(av1mi, 1, case, frames), run(av1mi, 0, case, frames)
    assert same(on, off) and on[3] is None and off[3] is None


def test_second_chunk_of_another_size_on_one_context(av1mi, oracle):
    a = dict(name="first", w=128, h=64, n=3, bd=10, params={})
    b = dict(name="second", w=192, h=136, n=2, bd=10, params={})
    fa, fb = synth(oracle, 128, 64, 3), synth(oracle, 192, 136, 2, seed=7)

    def two(c):
        encode(av1mi, c, a, fa)
        first = c.sym_order_result()
        tus, recs, rep = encode(av1mi, c, b, fb)
        again = encode(av1mi, c, b, fb)   # the same size once more: the counters start from zero every chunk
        return first, (tus, recs, [int(x) for x in rep.sse], c.sym_order_result()), (again[0], again[1], [int(x) for x in again[2].sse], c.sym_order_result())
    first, second, third = with_order(av1mi, 1, two)
    fresh = run(av1mi, 1, b, fb)
    check_table(a, first)
    assert same(second, fresh) and same(third, fresh)
    for res in (second[3], third[3], fresh[3]):
        order, classes = check_table(b, res)
        assert np.array_equal(classes, fresh[3][1])   # a tile's class is its content's: the same in every run
