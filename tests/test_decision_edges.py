"""GPU tests of three decision kernels at the edge inputs of tests/edge_content.py, each against the restatement its own test file
uses: the AQ map (tests/aq_ref.py), the deblocking level search (tests/deblock_ref.py through the oracle) and partition_search = 2
(tests/part_inter_ref.py).  Their own cases are synthclip noise, or low-amplitude patches at cq 1 and 3; here they meet full-range
checkers, impulses, steps and flat planes, cq 1 and 63, and frames whose every candidate has the same error."""
import numpy as np
import pytest

import aq_ref
import edge_content as E
import lr_edge_cases
import part_inter_ref as PR
import test_deblock_search as D
import test_part_inter as P
from test_edges import raw_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(av1mi):
    c = av1mi.Context(0)
    yield c
    c.close()


# ---------------------------------------------------------------- the AQ map
AQ_ROWS = [(pat, w, h, bd) for pat in ("checker1", "impulse_white", "steps16_h", "flat") for w, h in ((8, 8), (72, 56), (202, 122)) for bd in (8, 10)]


def aq_frames(pat, w, h, bd, n):
    if pat == "flat":
        return [lr_edge_cases.flat(w, h, bd) for _ in range(n)]
    return E.clip(pat, w, h, bd, n, motion=(1, -3))


@pytest.mark.parametrize("pat,w,h,bd", AQ_ROWS, ids=["%s_%dx%d_%db" % r for r in AQ_ROWS])
def test_aq_map_equals_the_rule(av1mi, ctx, pat, w, h, bd):
    """av1mi_aq_qindex of two frames from host and from device memory is aq_ref.qindex_map at cq 1 / 30 / 63 and strengths 1, 2, 4.
    Flat content has every unit's energy at the log's floor, L(1) = 0; the 10-bit 1-sample checker the largest a unit can have."""
    import torch
    n = 2
    frames = aq_frames(pat, w, h, bd, n)
    raw = b"".join(raw_of(f, bd) for f in frames)
    dev = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()
    energy = [aq_ref.sb_energy(f[0], bd) for f in frames]
    if pat == "flat":
        assert not any(e.any() for e in energy)
    if pat == "checker1":
        mx = E.maxv_of(bd)
        assert int(energy[0].max()) == aq_ref.L(((64 * 32 * mx * mx - (32 * mx) ** 2) >> (12 + 2 * (bd - 8))) + 1)
    for cq in (1, 30, 63):
        base = av1mi.cq_to_qindex(cq)
        for s in (1, 2, 4):
            want = np.stack([aq_ref.qindex_map(f[0], bd, s, base) for f in frames])
            p = av1mi.default_params(w, h, bd, cq_level=cq, aq_strength=s)
            got = ctx.aq_qindex(p, raw, n)
            assert got.shape == want.shape and np.array_equal(got, want), (cq, s, "host input", got.tolist(), want.tolist())
            got = ctx.aq_qindex(p, dev.data_ptr(), n, on_device=True)
            assert np.array_equal(got, want), (cq, s, "device input", got.tolist(), want.tolist())


# ---------------------------------------------------------------- the deblocking level search
def lf_case(name, w, h, bd, n, content, **params):
    return dict(name=name, w=w, h=h, bd=bd, n=n, content=content, params=dict(params, deblock=2))


# (test_deblock_search.reference keeps one restatement per (w, h, bd, n): the two 72x56 rows differ in their frame count)
LF_CASES = [
    lf_case("72x56_10b_checker_bs3_cq63", 72, 56, 10, 2, ("checker_bs", (3, 1)), cq_level=63, block_log2=3, keyint=1),
    lf_case("72x56_10b_checker_bs6_cq63", 72, 56, 10, 3, ("checker_bs", (3, 1)), cq_level=63, block_log2=6, keyint=3, subpel=1),
    lf_case("136x72_8b_steps8_v_cq1", 136, 72, 8, 2, ("steps8_v", (1, -3)), cq_level=1, keyint=240),
]


@pytest.mark.parametrize("case", LF_CASES, ids=[c["name"] for c in LF_CASES])
def test_deblock_search_equals_the_reference(av1mi, ctx, oracle, case):
    """levels, error table, bytes and reconstruction are the oracle's under the rule, on full-range edges at the block size and at
    the extreme quantisers (g = 63: clamped duplicate candidates; g = 0 on the key frame: the luma floor of 1)"""
    olevels, oerrs, gs = D.check_against_reference(av1mi, ctx, oracle, case)
    print("levels", olevels, "formula", gs)
    if case["params"]["cq_level"] == 63:
        assert gs[0] == 63
    if case["params"]["cq_level"] == 1:
        assert gs[0] == 0 and olevels[0][0] >= 1


# ---------------------------------------------------------------- partition_search = 2
def pi_case(w, h, cq, content, **params):
    name = "%dx%d_%s_cq%d_r%d%s" % (w, h, content, cq, params.get("me_range", 8), "_pre" if params.get("me_presearch") else "")
    return dict(name=name, w=w, h=h, bd=10, n=3, cq=cq, content=content, params=dict(params, block_log2=6, min_block_log2=3))


PI_CASES = [
    pi_case(72, 56, 63, "alternating", me_range=8),       # every candidate has the maximal SAD: only the vector penalty orders them
    pi_case(136, 72, 1, "alternating", me_range=16),
    pi_case(72, 56, 63, "identical", me_range=16),        # every SAD is 0: nothing may split by choice
    pi_case(136, 72, 1, "identical", me_range=8, me_presearch=1),
    pi_case(72, 56, 1, "checker1", me_range=8),
    pi_case(136, 72, 63, "checker1", me_range=16, me_presearch=1),
]


def pi_frames(case):
    w, h, bd, n = case["w"], case["h"], case["bd"], case["n"]
    if case["content"] == "alternating":
        mid = np.full((h // 2, w // 2), 1 << (bd - 1), np.uint16)
        return [[np.full((h, w), (t & 1) * E.maxv_of(bd), np.uint16), mid, mid.copy()] for t in range(n)]
    if case["content"] == "identical":
        return [E.frame("impulse_white", w, h, bd) for _ in range(n)]
    return E.clip("checker1", w, h, bd, n, motion=(1, -3))


@pytest.mark.parametrize("case", PI_CASES, ids=[c["name"] for c in PI_CASES])
def test_inter_partition_equals_the_reference(av1mi, ctx, case):
    """tests/test_part_inter.py's comparison: the masks and every leaf's key of the inter frames are part_inter_ref.reference_frame's,
    at the largest split penalty (cq 63) and the smallest (cq 1)"""
    frames = pi_frames(case)
    n = len(frames)
    _, _, _, (masks1, _) = P.encode(av1mi, ctx, case, frames, 1)
    _, _, _, (masks2, keys2) = P.encode(av1mi, ctx, case, frames, 2)
    assert np.array_equal(masks2[0], masks1[0])   # the key frame keeps the source rule
    p = case["params"]
    sbr, sbc = masks2.shape[1:]
    acq = PR.case_ac_q(case)
    for t in range(1, n):
        cen = P.centres_of(keys2[t], sbr, sbc)
        if not p.get("me_presearch"):
            assert not cen.any()
        want_masks, want_keys = PR.reference_frame(frames[t][0].astype(np.int32), frames[t - 1][0].astype(np.int32), p.get("me_range", 8),
                                                   p["min_block_log2"], p["block_log2"], acq, cen)
        assert np.array_equal(masks2[t], want_masks), (t, [hex(int(x)) for x in masks2[t].ravel()], [hex(int(x)) for x in want_masks.ravel()])
        bad = [(u, hex(int(keys2[t][u])), hex(k)) for u, k in want_keys.items() if int(keys2[t][u]) != k]
        assert not bad, (t, bad[:8])
        if case["content"] == "identical":
            assert not want_masks.any()
