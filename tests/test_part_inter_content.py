"""CPU check of the content tests/test_part_inter.py feeds the GPU - a condition on the inputs, not a measurement: by the reference
alone (tests/part_inter_ref.py) every case's inter frames must, at each level the case decides (16, 32, 64 within min_block_log2 <
level <= block_log2), split at least 10 % of the decided nodes and keep at least 10 %, hold at least one forced node and at least one
decided node whose split cost equals its leaf cost exactly (S == cL: the tie that must keep the larger block).

72x56 is one superblock beside a strip: its three inter frames hold one decided 64x64 node each, so its frames are built to split it
twice and to tie it once, with the ties at 32 and 16 in the frames that split it (tests/part_inter_ref.py: make_luma).  In the
8-sample-wide or -high strips 8x136 and 136x8 the frame edge forces every node above 8x8: nothing is decided there, and they must show
exactly that - forced nodes at every level and 8x8 leaves alone."""
import numpy as np
import pytest

import part_inter_ref as PR

_stats = {}


def stats_of(case):
    if case["name"] not in _stats:
        ys = PR.make_luma(case)
        p = case["params"]
        st = PR.Stats()
        for t in range(1, case["n"]):
            cur, prev = ys[t].astype(np.int32), ys[t - 1].astype(np.int32)
            sbr, sbc = (case["h"] + 63) // 64, (case["w"] + 63) // 64
            cen = PR.presearch_centres(cur, prev) if p.get("me_presearch") else np.zeros((sbr, sbc), np.uint32)
            PR.reference_frame(cur, prev, p.get("me_range", 8), p["min_block_log2"], p["block_log2"], PR.case_ac_q(case), cen, st)
        _stats[case["name"]] = st
    return _stats[case["name"]]


def levels_of(case):
    p = case["params"]
    return [b for b in (4, 5, 6) if p["min_block_log2"] < b <= p["block_log2"]]


@pytest.mark.parametrize("case", PR.CASES[:4], ids=[c["name"] for c in PR.CASES[:4]])
def test_every_decidable_level_splits_keeps_forces_and_ties(case):
    assert PR.case_ac_q(case) >> 4 == 1   # the ties are built for T(n) = n^2 / 8
    st = stats_of(case)
    assert levels_of(case)
    for b in levels_of(case):
        decided = st.split[b] + st.keep[b]
        print(case["name"], 1 << b, "split", st.split[b], "keep", st.keep[b], "forced", st.forced[b], "ties", st.tie[b])
        assert decided >= (10 if case["w"] >= 192 else case["n"] - 1)   # (one superblock: a decided 64x64 node per inter frame at the least)
        assert 10 * st.split[b] >= decided and 10 * st.keep[b] >= decided, (b, st.split[b], st.keep[b])
        assert st.forced[b] >= 1 and st.tie[b] >= 1, (b, st.forced[b], st.tie[b])
    assert sum(1 for b in (3, 4, 5, 6) if st.leaves[b]) >= 3


@pytest.mark.parametrize("case", PR.CASES[4:], ids=[c["name"] for c in PR.CASES[4:]])
def test_strips_are_all_forced(case):
    st = stats_of(case)
    for b in (4, 5, 6):
        assert st.split[b] + st.keep[b] == 0 and st.forced[b] >= 1
    assert st.leaves[3] == (case["n"] - 1) * 17 and not (st.leaves[4] or st.leaves[5] or st.leaves[6])
