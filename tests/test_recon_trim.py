"""GPU tests of the reconstruction kernel's trimmed block items (DESIGN.md §4.2 xiv: the quantiser loops over quant_pieces.h - dead-zone
class from compile-time register rows, scan key and extent from the last nonzero register, a chroma row's columns shared between two
lanes): bitstream, reconstruction and SSE equal the oracle's, bit for bit.

Frames of 64x64 (one superblock), 96x80 (overhanging blocks: the sample-by-sample path, and the 16x16 chroma pair at the edge) and
128x64, two frames each, 10 and 8 bit, with all 13 luma candidates (0x1FFF), DC / V / H only (0x7: only the quantiser trims act) and DC
plus the three smooth candidates (0xE01).  Content: full-range noise on blocks at alternating extremes at the lowest quantiser index
the encoder takes (a level in every register of every lane; the 0x7FFF cap lies beyond what a residual reaches at that step, 15 for
DC at 10 bit - tests/test_quant_pieces_host.py covers it); a flat frame at the highest (eob 0); a flat frame with, per 32x32 block,
one vertical cosine of frequency k - an impulse at coefficient row k, k stepping through all rows over the blocks, frames and cases,
so that the last nonzero coefficient falls in each of the 16 register rows of both wave halves - and per 16x16 chroma block a horizontal
one, so that a chroma row's last level falls in every column of both lanes that share the row (tests/test_recon_trim_content.py
asserts on the CPU where the levels fall); and `synthclip v1`.  One case with
quantiser matrices (that instantiation keeps its table reads) and one with 64x64 leaf blocks.

The item's shared pieces (recon_pieces.h, the one quantiser step of quant_pieces.h) run in every case here; two of their branches no
other case reached have cases of their own below: the hand-over of a motion-compensated block that overhangs the frame (the staged
rows' clamps), and the quantiser-matrix row loop on blocks that took the identity transform."""
import numpy as np
import pytest

import edge_content as E
from test_edges import encode

pytestmark = pytest.mark.gpu

SIZES = [(64, 64), (96, 80), (128, 64)]
MASKS = [0x1FFF, 0x7, 0xE00 | 1]
N = 2


def noise(rng, w, h, bd, t):
    mx = E.maxv_of(bd)
    out = []
    for pw, ph, n in ((w, h, 32), (w // 2, h // 2, 16), (w // 2, h // 2, 16)):
        Y, X = np.mgrid[0:ph, 0:pw]
        base = (((X // n + Y // n + t) & 1) * mx).astype(np.int64)   # blocks at alternating extremes: the largest DC residuals
        v = np.where(rng.integers(0, 4, (ph, pw)) == 0, base, rng.integers(0, mx + 1, (ph, pw)))
        out.append(v.astype(np.uint16))
    return out


def flat(w, h, bd):
    mid = 1 << (bd - 1)
    return [np.full((h, w), mid, np.uint16), np.full((h // 2, w // 2), mid - 3, np.uint16), np.full((h // 2, w // 2), mid + 5, np.uint16)]


def row_impulses(w, h, bd, t, k0):
    """flat, plus in every 32x32 luma block a vertical cosine of frequency k (one coefficient in row k, column 0) and in every 16x16
    chroma block a horizontal one (row 0, column k: both halves of the columns a chroma row's two lanes share);
    tests/test_recon_trim_content.py checks on the CPU that the last nonzero level lies there and that the cases cover every k"""
    f = flat(w, h, bd)
    amp = 40 << (bd - 8)
    for pl, n in ((0, 32), (1, 16), (2, 16)):
        ph, pw = f[pl].shape
        Y, X = np.mgrid[0:ph, 0:pw]
        k = impulse_k(X // n, Y // n, pl, n, t, k0)
        along = Y if pl == 0 else X
        f[pl] = (f[pl] + np.rint(amp * np.cos(np.pi * (2 * (along % n) + 1) * k / (2 * n)))).astype(np.uint16)
    return f


def impulse_k(bx, by, pl, n, t, k0):
    return (k0 + 16 * t + 5 * bx + 11 * by + 3 * pl) % n


def impulse_k0(w, h, bd, mask):
    return (SIZES.index((w, h)) * 6 + MASKS.index(mask) * 2 + (bd == 8)) * 5


def check(av1mi, ctx, oracle, case, frames):
    tus, recs, rep = encode(av1mi, ctx, case, frames)
    otus, orecs, osse = E.oracle_encode(oracle, case, frames)
    assert [len(t) for t in tus] == [len(t) for t in otus], case["name"]
    for i, (a, b) in enumerate(zip(tus, otus)):
        assert a == b, "%s: bitstream of frame %d" % (case["name"], i)
    for i, (a, b) in enumerate(zip(recs, orecs)):
        for pl in range(3):
            assert np.array_equal(a[pl], b[pl]), "%s: reconstruction of frame %d plane %d" % (case["name"], i, pl)
    assert [int(x) for x in rep.sse] == osse, case["name"]
    return sum(len(t) for t in tus)


@pytest.mark.parametrize("mask", MASKS, ids=["all13", "dcvh", "smooth"])
@pytest.mark.parametrize("bd", [10, 8])
@pytest.mark.parametrize("w,h", SIZES)
def test_trimmed_items_equal_the_oracle(av1mi, ctx, oracle, w, h, bd, mask):
    rng = np.random.default_rng(w * 7 + h * 3 + bd + mask)
    k0 = impulse_k0(w, h, bd, mask)
    contents = [
        ("noise_cq1", dict(cq_level=1), [noise(rng, w, h, bd, t) for t in range(N)]),
        ("flat_cq63", dict(cq_level=63), [flat(w, h, bd) for t in range(N)]),
        ("row_impulses", dict(cq_level=30), [row_impulses(w, h, bd, t, k0) for t in range(N)]),
        ("synthclip", dict(), E.synth(oracle, w, h, bd, N, 1080)),
    ]
    sizes = {}
    for name, extra, frames in contents:
        case = dict(name="%s_%dx%d_%db_%x" % (name, w, h, bd, mask), w=w, h=h, bd=bd, n=N, params=dict(intra_mode_mask=mask, **extra))
        sizes[name] = check(av1mi, ctx, oracle, case, frames)
    assert sizes["flat_cq63"] < sizes["row_impulses"] < sizes["noise_cq1"]   # the contents do what they are named for


@pytest.mark.parametrize("params", [dict(enable_qm=1, qm_min=1, qm_max=15), dict(block_log2=6)], ids=["qm", "bs6"])
def test_untouched_instantiations_equal_the_oracle(av1mi, ctx, oracle, params):
    for w, h, bd in ((96, 80, 10), (128, 64, 8)):
        case = dict(name="synth_%dx%d_%db_%s" % (w, h, bd, sorted(params)[0]), w=w, h=h, bd=bd, n=N, params=dict(params))
        check(av1mi, ctx, oracle, case, E.synth(oracle, w, h, bd, N, 1080))


def leaves32_overhanging(w, h):
    """the 32x32 leaves that cross the frame's edge: a node is split where half of it or more lies outside (av1mi_dev.h, av1mi_node_split)"""
    return [(x, y) for y in range(0, h, 32) for x in range(0, w, 32) if x + 16 < w and y + 16 < h and (x + 32 > w or y + 32 > h)]


@pytest.mark.parametrize("bd", [10, 8])
@pytest.mark.parametrize("w,h", [(88, 88), (96, 80)])
def test_inter_hand_over_of_overhanging_blocks_equals_the_oracle(av1mi, ctx, oracle, w, h, bd):
    """two identical frames, the second a P frame of 32x32 leaves: motion compensation wins everywhere, so at 88x88 the blocks that
    overhang the right edge, the bottom edge and - the corner block - both hand their bottom row and right column over from the staged
    rows of the inter version, clamped to the last sample inside, in luma and, following it, in both chroma planes.  (88 is no multiple
    of 16 either: the 8-bit rows take the sample-by-sample copies.)  96x80 is the counterpart without a clamp: exactly half of its
    bottom 32x32 nodes lies inside, so they are split and nothing overhangs."""
    f = E.synth(oracle, w, h, bd, 1, 1080)[0]
    frames = [f, [pl.copy() for pl in f]]
    case = dict(name="static_%dx%d_%db" % (w, h, bd), w=w, h=h, bd=bd, n=N, params=dict(keyint=240, block_log2=5))
    # on the CPU first: the oracle codes EVERY block of the P frame as an inter block, the overhanging ones of each plane among them
    # (a chroma block follows its luma block) - otherwise the case proves nothing
    over = leaves32_overhanging(w, h)
    assert len(over) == (5 if (w, h) == (88, 88) else 0) and ((64, 64) in over) == ((w, h) == (88, 88))
    _, rec0, _ = oracle.encode_frame(E.oracle_config(oracle, case, 0), frames[0], with_seq_hdr=True, ref=None, prev_src=None)
    _, _, st = oracle.encode_frame(E.oracle_config(oracle, case, 1), frames[1], with_seq_hdr=False, ref=rec0, prev_src=frames[0])
    assert st.n_inter_blocks == st.n_blocks == (9 if (w, h) == (88, 88) else 12)
    check(av1mi, ctx, oracle, case, frames)


@pytest.mark.parametrize("bd", [10, 8])
@pytest.mark.parametrize("bs", [4, 3])
def test_quantiser_matrices_with_identity_transform_search_equal_the_oracle(av1mi, ctx, oracle, bs, bd):
    """posterised content (flat areas, sharp edges: sparse residuals) with tx_search under quantiser matrices: the blocks that take the
    identity transform are quantised with the flat steps inside the quantiser-matrix row loop (spec 7.12.3: PlaneTxType < IDTX)"""
    w = h = 64
    shift = bd - 3
    frames = [[(pl >> shift) << shift for pl in f] for f in E.synth(oracle, w, h, bd, N, {4: 4504, 3: 4500}[bs])]
    params = dict(block_log2=bs, tx_search=1, enable_qm=1, qm_min=1, qm_max=15)
    case = dict(name="idtx_qm_bs%d_%db" % (bs, bd), w=w, h=h, bd=bd, n=N, params=params)
    # on the CPU first: the identity transform is chosen somewhere - without the search the oracle's stream is another
    assert E.oracle_encode(oracle, case, frames)[0] != E.oracle_encode(oracle, dict(case, params=dict(params, tx_search=0)), frames)[0]
    check(av1mi, ctx, oracle, case, frames)
