"""GPU tests of the deblocking level search (include/av1mi.h: av1mi_params.deblock = 2, av1mi_lf_search_result).

The oracle is an exact reference for the whole feature (tests/deblock_ref.py): it takes explicit levels, a frame's reconstruction
before deblocking does not depend on them, so 16 oracle runs per frame with CDEF and restoration off give every candidate's deblocked
frame, numpy the error table and the rule, and one more run at the chosen levels the expected bytes and the next frame's reference.
dav1d (libavif) decodes the streams of the tool combinations the oracle cannot restate."""
import numpy as np
import pytest

import deblock_ref
import edge_content as E
from test_edges import encode, raw_of

pytestmark = pytest.mark.gpu


def case_of(w, h, bd, n, seed, **params):
    params.setdefault("keyint", 1)
    return dict(name="lf", w=w, h=h, bd=bd, n=n, content=("synth", seed), params=dict(params, deblock=2))


# ---------------------------------------------------------------- 5. decision, error table, parity
CASES = [
    case_of(8, 8, 8, 2, 6100, keyint=240),                                     # no filtered edge: all errors equal, index 0
    case_of(72, 56, 8, 2, 6101, block_log2=3, cq_level=63, keyint=240),         # one superblock, overhang; g = 63: clamped duplicates
    case_of(136, 72, 10, 2, 6102, cq_level=1),                                 # g = 0 on the key frame: luma floor 1, 12 more header bits
    case_of(200, 136, 10, 3, 6103, block_log2=4, keyint=2),                    # 8-sample sliver superblocks right and bottom
    case_of(256, 192, 8, 2, 6104, block_log2=6, cq_level=50),                  # 16-wide filters across every superblock edge
    case_of(392, 264, 10, 2, 6105, partition_search=1, block_log2=6, min_block_log2=3, keyint=240),   # mixed sizes across superblock edges
    case_of(202, 122, 8, 3, 6106, keyint=240, subpel=1),                       # true size below coded size
    case_of(328, 248, 10, 4, 6107, keyint=3, subpel=1, enable_lr=2, enable_qm=1, qm_min=1),   # tools behind the deblocked frame
    case_of(648, 360, 8, 2, 6108, tile_sb=2, intra_mode_mask=0x1FFF),          # 2x2-superblock tiles
]
IDS = ["%dx%d_%db_%df" % (c["w"], c["h"], c["bd"], c["n"]) for c in CASES]

_refs = {}


def reference(oracle, case):
    """the oracle's restatement of a case, computed once"""
    key = (case["w"], case["h"], case["bd"], case["n"])
    if key not in _refs:
        frames = E.source(oracle, case)
        _refs[key] = (frames,) + deblock_ref.reference(oracle, case, frames)
    return _refs[key]


def check_against_reference(av1mi, ctx, oracle, case):
    frames, otus, orecs, olevels, oerrs, gs = reference(oracle, case)
    n = case["n"]
    if (case["w"] + 63) // 64 * ((case["h"] + 63) // 64) > 1:
        # the case must exercise the search: the rule moves some frame's levels off the formula's
        assert any(olevels[f] != [gs[f]] * 4 for f in range(n)), (olevels, gs)
    tus, recs, rep = encode(av1mi, ctx, case, frames)
    levels, errs = ctx.lf_search_result(n)
    for f in range(n):
        assert [int(x) for x in levels[f]] == olevels[f], "levels of frame %d: %s, errors %s" % (f, levels[f], errs[f])
        assert np.array_equal(errs[f], oerrs[f]), "error table of frame %d" % f
    assert [len(t) for t in tus] == [len(t) for t in otus]
    for f in range(n):
        assert tus[f] == otus[f], "bitstream of frame %d" % f
        for pl in range(3):
            assert np.array_equal(recs[f][pl], orecs[f][pl]), "reconstruction of frame %d plane %d" % (f, pl)
    return olevels, oerrs, gs


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_decision_errors_and_parity(av1mi, ctx, oracle, case):
    olevels, oerrs, gs = check_against_reference(av1mi, ctx, oracle, case)
    if case["w"] == 8:
        assert all(len(set(int(x) for x in e[p])) == 1 for e in oerrs for p in range(3))   # no edge: every candidate alike
        assert olevels == [[deblock_ref.pool(g, False)[0]] * 2 + [deblock_ref.pool(g, True)[0]] * 2 for g in gs]   # index 0
    if case["params"].get("cq_level") == 1:
        assert gs[0] == 0 and olevels[0][0] >= 1
    if case["params"].get("cq_level") == 63:
        assert gs[0] == 63


def test_header_patch_beside_entropy_groups(av1mi, oracle, monkeypatch):
    """the P chunk at the true size below the coded size once more with the frames entropy-coded in groups of one on the third stream"""
    monkeypatch.setenv("AV1MI_ENTROPY_GROUP", "1")
    with av1mi.Context(0) as c:
        check_against_reference(av1mi, c, oracle, CASES[6])


# ---------------------------------------------------------------- 6. never worse than the formula
def sse_per_frame(recs, frames):
    return [deblock_ref.plane_sse(r, f) for r, f in zip(recs, frames)]


@pytest.mark.parametrize("w,h,bd", [(328, 200, 8), (648, 360, 10)])
@pytest.mark.parametrize("cq", [30, 50])
def test_never_worse_than_the_formula(av1mi, ctx, oracle, w, h, bd, cq):
    n = 2
    case = case_of(w, h, bd, n, 6200 + w, cq_level=cq, enable_cdef=0)
    frames = E.source(oracle, case)
    one = dict(case, params=dict(case["params"], deblock=1))
    tus1, recs1, rep1 = encode(av1mi, ctx, one, frames)
    tus2, recs2, rep2 = encode(av1mi, ctx, case, frames)
    levels, errs = ctx.lf_search_result(n)
    tus2b, recs2b, _ = encode(av1mi, ctx, case, frames)
    assert tus2 == tus2b and all(np.array_equal(a[pl], b[pl]) for a, b in zip(recs2, recs2b) for pl in range(3))
    assert tus2 != tus1
    e1, e2 = sse_per_frame(recs1, frames), sse_per_frame(recs2, frames)
    for f in range(n):
        for pl in range(3):
            assert e2[f][pl] <= e1[f][pl], "frame %d plane %d" % (f, pl)
            # the D = 0 candidate is the formula's run, the chosen one the search's
            assert int(errs[f][pl][7]) == e1[f][pl] and int(errs[f][pl].min()) == e2[f][pl]
    assert [int(x) for x in rep2.sse] == [sum(e[pl] for e in e2) for pl in range(3)]
    assert [int(x) for x in rep1.sse] == [sum(e[pl] for e in e1) for pl in range(3)]


# ---------------------------------------------------------------- 7. context reuse
def test_context_reuse(av1mi, oracle):
    w, h, bd, n = 264, 200, 10, 3
    base = case_of(w, h, bd, n, 6300, keyint=3, subpel=1, cdef_search=2)
    frames = E.source(oracle, base)
    variants = [dict(base, params=dict(base["params"], deblock=d)) for d in (2, 1, 0)]
    fresh = []
    for v in variants:
        with av1mi.Context(0) as c:
            tus, recs, _ = encode(av1mi, c, v, frames)
            fresh.append((tus, recs, c.lf_search_result(n)))
    assert fresh[0][0] != fresh[1][0] != fresh[2][0]
    with av1mi.Context(0) as c:
        for v, (tus0, recs0, (lv0, er0)) in list(zip(variants, fresh)) + [(variants[0], fresh[0])]:
            tus, recs, _ = encode(av1mi, c, v, frames)
            assert tus == tus0, v["params"]["deblock"]
            assert all(np.array_equal(a[pl], b[pl]) for a, b in zip(recs, recs0) for pl in range(3))
            lv, er = c.lf_search_result(n)
            assert np.array_equal(lv, lv0) and np.array_equal(er, er0)
            if v["params"]["deblock"] != 2:
                assert not er.any() and len(set(int(x) for x in lv[0])) == 1
            with pytest.raises(av1mi.EncodeFailed):
                c.lf_search_result(n + 1)
    assert not fresh[2][2][0].any()   # deblock = 0: all levels 0


def test_error_table_is_cleared_per_attempt(av1mi, oracle):
    """full-range noise at CQ 4 outgrows the x1 tile capacities (tests/test_gpu_parity.py: test_stress_carries_and_long_tiles): the
    chunk runs twice on a fresh context, and the error table is that of one run"""
    rng = np.random.default_rng(99)
    w, h, n = 328, 248, 2
    frames = [[rng.integers(0, 256, (h, w)).astype(np.uint16), rng.integers(0, 256, (h // 2, w // 2)).astype(np.uint16),
               rng.integers(0, 256, (h // 2, w // 2)).astype(np.uint16)] for _ in range(n)]
    case = dict(name="noise", w=w, h=h, bd=8, n=n, content=None, params=dict(cq_level=4, block_log2=5, deblock=2, keyint=1))
    otus, orecs, olevels, oerrs, gs = deblock_ref.reference(oracle, case, frames)
    with av1mi.Context(0) as c:
        tus, recs, rep = encode(av1mi, c, case, frames)
        levels, errs = c.lf_search_result(n)
    assert rep.cap_scale > 1
    for f in range(n):
        assert np.array_equal(errs[f], oerrs[f]) and [int(x) for x in levels[f]] == olevels[f]
        assert tus[f] == otus[f]


# ---------------------------------------------------------------- 8. dav1d
DECODE = [
    (328, 248, 10, 5, dict(keyint=3, subpel=1, cdef_search=3, enable_lr=4, aq_strength=2)),
    (200, 136, 8, 5, dict(keyint=240, cdef_search=2, enable_lr=3, cdf_update=0)),
    (3840, 2160, 10, 2, dict(keyint=2, tile_sb=2)),
]


@pytest.mark.parametrize("w,h,bd,n,extra", DECODE)
def test_dav1d_decodes_to_the_reconstruction(av1mi, oracle, w, h, bd, n, extra):
    import oracle_avif
    if not oracle_avif.have_libavif():
        pytest.skip("libavif (dav1d) is not available on this machine")
    frames = [oracle.synthclip_frame(w, h, bd, seed=6400 + w, t=t) for t in range(n)]
    p = av1mi.default_params(w, h, bd, deblock=2, **extra)
    with av1mi.Context(0) as c:
        data, sizes, rep, recon = c.encode_chunk(p, b"".join(raw_of(f, bd) for f in frames), n, want_recon=True)
        levels, errs = c.lf_search_result(n)
    assert (levels[:, 0] >= 1).all() and (levels[:, 0] == levels[:, 1]).all()
    from test_edges import split_frames
    want = split_frames(recon, w, h, bd, n)
    tus, off = [], 0
    for s in sizes:
        tus.append(data[off:off + s])
        off += s
    got = E.dav1d_decode(tus, w, h, bd, extra.get("keyint", 1))
    assert E.decodes_to(got, want, bd, 0) is None
