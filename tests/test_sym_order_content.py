"""CPU check of the content tests/test_sym_order.py feeds the GPU - that its noise-island frames really put tiles at both ends of the
weight classes (av1-base_amd/csrc/tile_weight_rule.h), so that "the noise tiles come first" cannot hold by accident:

 * the flat tiles: the oracle codes every block outside the noise tile as a skip block (all three eobs zero - a weight of 0, class 0),
   at CQ 30, at the lowest CQ and at the highest;
 * the noise tile (DC prediction only, so a block's AC levels are those of the block itself): by the oracle's forward transforms and
   the quantiser rule of DESIGN.md §3.5 the scan position of every block's last nonzero AC level + 1 - a lower bound of its eob - sums
   over the tile's twelve transform blocks to the top class's bound and more at CQ 30 and at the lowest CQ, where it is the largest sum
   there is, 6 144; at the highest CQ levels are still left (the tile is not class 0), though the sum may fall below the top class."""
import os
import re

import numpy as np
import pytest

import edge_content as E
import test_recon_trim_content as RC
import test_sym_order as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rule():
    txt = open(os.path.join(ROOT, "av1-base_amd", "csrc", "tile_weight_rule.h")).read()
    step_log2 = int(re.search(r"#define AV1MI_TILE_WEIGHT_STEP_LOG2 (\d+)", txt).group(1))
    classes = int(re.search(r"#define AV1MI_TILE_CLASSES (\d+)", txt).group(1))
    return ((classes - 2) << step_log2) + 1, int(re.search(r"#define AV1MI_TILE_WEIGHT_MAX_SB (\d+)", txt).group(1))


def scan_pos(i, j, n):
    """index of (row i, column j) in the default zig-zag of an n x n block (RC.last_nonzero's order)"""
    d = i + j
    before = sum(min(k, n - 1) - max(0, k - n + 1) + 1 for k in range(d))
    lo = max(0, d - n + 1)
    return before + ((i if d & 1 else j) - lo)


def eob_lower_bound(oracle, blk, plane, bd, qidx):
    lv = RC.levels(oracle, RC.of_block(blk), plane, bd, qidx)
    lv[0, 0] = 0   # (the DC level follows the prediction)
    last = RC.last_nonzero(lv)
    return 0 if last is None else scan_pos(int(last[0]), int(last[1]), lv.shape[0]) + 1


def noise_tile_weight(oracle, cq):
    """per frame: the lower bound of the noise tile's eob sum"""
    out = []
    for t, f in enumerate(S.island_frames()):
        x0 = S.noise_tiles(S.ISLAND["w"], S.ISLAND["h"], t)[0] * 64
        total = 0
        for pl, n, sh in ((0, 32, 0), (1, 16, 1), (2, 16, 1)):
            tile = f[pl][0:64 >> sh, x0 >> sh:(x0 + 64) >> sh]
            for bx, by, blk in RC.whole_blocks(tile, n):
                total += eob_lower_bound(oracle, blk, min(pl, 1), 10, E.QINDEX[cq])
        out.append(total)
    return out


def test_scan_pos_is_the_scan():
    for n in (16, 32):
        lv = np.zeros((n, n), np.int64)
        seen = set()
        for i in range(n):
            for j in range(n):
                lv[:] = 0
                lv[i, j] = 1
                assert RC.last_nonzero(lv) == (i, j)
                seen.add(scan_pos(i, j, n))
        assert seen == set(range(n * n))
    assert scan_pos(0, 0, 32) == 0 and scan_pos(31, 31, 32) == 1023 and scan_pos(0, 1, 32) < scan_pos(2, 0, 32)


@pytest.mark.parametrize("cq", [30, 1, 63])
def test_flat_tiles_are_all_skip_blocks(oracle, cq):
    case = dict(S.ISLAND, name="island", params=dict(cq_level=cq, intra_mode_mask=1))
    tiles = (S.ISLAND["w"] // 64) * (S.ISLAND["h"] // 64)
    for t, f in enumerate(S.island_frames()):
        tu, rec, st = oracle.encode_frame(E.oracle_config(oracle, case, t), f)
        assert st.n_blocks == 4 * tiles
        assert st.n_skip_blocks == 4 * (tiles - 1), (cq, t, st.n_skip_blocks)   # every block but the noise tile's four
        x0 = S.noise_tiles(S.ISLAND["w"], S.ISLAND["h"], t)[0] * 64
        flat_part = np.ones(f[0].shape, bool)
        flat_part[0:64, x0:x0 + 64] = False
        assert np.array_equal(rec[0][flat_part], f[0][flat_part])   # the skipped blocks are the flat ones: coded without a residual, exact


def test_noise_tile_sums_reach_the_top_class(oracle):
    top, max_sb = rule()
    assert all(w >= top for w in noise_tile_weight(oracle, 30))
    assert noise_tile_weight(oracle, 1) == [max_sb] * S.ISLAND["n"]   # every position is coded: the sum saturates
    assert all(w > 0 for w in noise_tile_weight(oracle, 63))
