"""GPU tests of the CDEF strength search (cdef_search_kernel, cdef_select_kernel) at the edge inputs of
tests/edge_content.py: one superblock of 8x8 samples, 8-sample-thin frames, cq 1 and 63, cdef_damping 3 and 6, full-range checkers,
impulses, steps and flat planes.  tests/test_cdef_search.py's restatement unchanged: 16 fixed-strength encodes give every candidate's
output and error per superblock, the rule picks the set and the indices (np.argmin: the first minimum, which is all that orders the
candidates of a flat frame), the search run's reconstruction is the rule's assembly and every frame header carries the rule's set."""
import numpy as np
import pytest

import edge_content as E
import lr_edge_cases
import test_cdef_search as T

pytestmark = pytest.mark.gpu

CASES = [
    # w, h, bd, pattern, motion, k, extra
    (8, 8, 8, "checker1", (1, -3), 4, {}),                               # one superblock, eight pairs to choose for it
    (72, 56, 10, "impulse_white", (1, 2), 4, dict(cdef_damping=3)),
    (72, 56, 10, "impulse_white", (1, 2), 4, dict(cdef_damping=6)),
    (72, 56, 8, "flat", (0, 0), 2, {}),                                  # every candidate's error is equal: the first minima
    (136, 8, 10, "steps4_v", (1, -3), 3, dict(cq_level=63)),
    (8, 136, 8, "checker_bs", (1, -3), 1, dict(cq_level=1)),
    (200, 120, 10, "impulse_black", (2, 1), 4, dict(block_log2=3)),
]
IDS = ["%dx%d_%db_%s_k%d%s" % (c[0], c[1], c[2], c[3], c[5], "".join("_%s%d" % kv for kv in sorted(c[6].items()))) for c in CASES]


@pytest.fixture(scope="module")
def ctx(av1mi):
    c = av1mi.Context(0)
    yield c
    c.close()


def frames_of(w, h, bd, pattern, motion, extra, n=2):
    if pattern == "flat":
        return [lr_edge_cases.flat(w, h, bd) for _ in range(n)]
    return E.clip(pattern, w, h, bd, n, bs=extra.get("block_log2", 5), motion=motion)


@pytest.mark.parametrize("w,h,bd,pattern,motion,k,extra", CASES, ids=IDS)
def test_decision_restated_and_header(av1mi, ctx, w, h, bd, pattern, motion, k, extra):
    """two key frames: the search run's reconstruction is the rule's assembly of the fixed-strength runs, and every frame header
    carries cdef_bits = k - 1 and the rule's set"""
    n = 2
    frames = frames_of(w, h, bd, pattern, motion, extra, n)
    (data, sizes, rep, rec), sets, runs = T.restate(ctx, av1mi, frames, w, h, bd, k, **dict(extra))
    hs = T.header_sets(av1mi, data, sizes, w, h, bd, k, **dict(extra))
    print("sets", sets, "pairs", [hs[f][1] for f in range(n)])
    for f in range(n):
        assert hs[f][0] == k - 1
        assert hs[f][1] == [T.pair_fields(p) for p in sets[f]], "frame %d" % f
    if pattern == "flat":   # no strength changes a sample, so every error is equal and the rule takes pair 0 every time
        assert all(np.array_equal(runs[i][f][pl], runs[0][f][pl]) for i in range(16) for f in range(n) for pl in range(3))
        assert sets == [[0] * (1 << (k - 1))] * n
