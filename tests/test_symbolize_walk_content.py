"""CPU check of the inputs tests/test_symbolize_walk.py feeds the GPU - that they do what they are for:

 * `mixed` under the content-driven partition: the oracle cuts it into leaves of all four sizes - at 200x136 inside one frame - and the
   sizes that are no multiple of 64 have 8x8 units outside the frame (the walk's step of one);
 * `eob_ladder` (DC prediction only, so the residual's AC coefficients are the block's own): by the oracle's forward transforms and the
   quantiser rule of DESIGN.md §3.5 every whole block's eob is the chosen one, and over the GPU test's frames the eob_extra lengths
   cover 1 .. 9 for the 32x32 luma blocks and 1 .. 7 for the 16x16 chroma blocks - every length the sizes allow;
 * `noise` at the lowest quantiser index: a block at one extreme beside one at the other has a DC level far above 14 whichever
   neighbour predicts it (the Golomb tail of the DC coefficient);
 * `alternating` at strength 4: the activity rule (tests/aq_ref.py) moves superblocks three and more steps of 4 off the base index, in
   both directions (delta_q remainder and abs bits, both signs).

That both restoration kinds occur among the fitted units is asserted where the fit runs, in the GPU test itself: neither the oracle
nor a reference on the CPU takes that decision."""
import numpy as np

import aq_ref
import edge_content as E
import test_recon_trim_content as RC
import test_symbolize_walk as W


def bs_hist(oracle, w, h, bd, keyint, n):
    case = W.walk_case(w, h, bd, keyint, dict(W.PART), "part")
    hist = np.zeros(7, np.int64)
    per_frame = []
    ref = prev = None
    for t in range(n):
        f = W.mixed(w, h, bd, t)
        key = t % keyint == 0
        tu, rec, st = oracle.encode_frame(E.oracle_config(oracle, case, t), f, with_seq_hdr=key, ref=None if key else ref, prev_src=None if key else prev)
        per_frame.append(np.array(list(st.bs_hist), np.int64))
        hist += per_frame[-1]
        ref, prev = rec, f
    return hist, per_frame


def test_mixed_has_leaves_of_all_four_sizes_and_units_outside_the_frame(oracle):
    for w, h in W.SIZES:
        hist, per_frame = bs_hist(oracle, w, h, 8, 1, 3)
        assert all(hist[b] > 0 for b in (3, 4, 5, 6)), (w, h, hist.tolist())
        if (w, h) == (200, 136):
            assert any(all(f[b] > 0 for b in (3, 4, 5, 6)) for f in per_frame), [f.tolist() for f in per_frame]
        units_outside = (-(-w // 64) * 8) * (-(-h // 64) * 8) - (-(-w // 8)) * (-(-h // 8))
        assert (units_outside > 0) == (w % 64 != 0 or h % 64 != 0)
    assert sum(1 for w, h in W.SIZES if w % 64 or h % 64) >= 2


def test_eob_ladder_covers_every_eob_extra_length(oracle):
    w, h = 128, 96
    for bd in (8, 10):
        lengths = {0: set(), 1: set()}
        for t in range(2):
            f = W.eob_ladder(w, h, bd, t)
            for pl, n in ((0, 32), (1, 16), (2, 16)):
                for bx, by, blk in RC.whole_blocks(f[pl], n):
                    want = W.ladder_last(bx, by, pl, n, t)
                    lv = RC.levels(oracle, RC.of_block(blk), min(pl, 1), bd, E.QINDEX[30])
                    lv[0, 0] = 0   # (the DC level follows the prediction; it is never the last)
                    assert RC.last_nonzero(lv) == W.scan_rc(want, n), (bd, t, pl, bx, by, want)
                    eob = want + 1
                    eob_pt = eob if eob <= 2 else int(np.floor(np.log2(eob - 1))) + 2
                    lengths[min(pl, 1)].add(eob_pt - 2)
        assert lengths[0] == set(range(1, 10)), sorted(lengths[0])
        assert lengths[1] == set(range(1, 8)), sorted(lengths[1])


def test_noise_has_dc_levels_above_14(oracle):
    w, h = 128, 96
    for bd in (8, 10):
        rng = np.random.default_rng(bd)
        f = W.noise(rng, w, h, bd, 0)
        blocks = {(bx, by): blk for bx, by, blk in RC.whole_blocks(f[0], 32)}
        top = 0
        for (bx, by), blk in blocks.items():
            for nb in ((bx - 1, by), (bx, by - 1)):
                if nb in blocks:   # predicted from a neighbour's samples: their mean is the other extreme's
                    resid = blk.astype(np.int64) - int(np.rint(blocks[nb].mean()))
                    top = max(top, int(RC.levels(oracle, resid, 0, bd, E.QINDEX[1])[0, 0]))
        assert top > 14, top


def test_alternating_moves_superblocks_three_steps_and_more(oracle):
    w, h, bd = 200, 136, 8
    base = E.QINDEX[30]
    steps = set()
    for t in range(3):
        q = aq_ref.qindex_map(W.alternating(w, h, bd, t)[0], bd, 4, base)
        steps |= set(((q - base) // 4).ravel().tolist())
    assert min(steps) <= -3 and max(steps) >= 3, sorted(steps)
