"""CPU side of the edge tests (no GPU): the oracle against dav1d on the edge case matrix of tests/edge_content.py, the dav1d-pinned
edge fixtures (tests/golden/index_edges.json), and the parameter and header rules those edges need - cq_level 0 (lossless) is refused,
a colour description never writes the code point 0, the tile-count limit."""
import ctypes as C
import hashlib
import itertools
import json
import os

import numpy as np
import pytest

import host_build
import edge_content as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def sha(planes):
    h = hashlib.sha256()
    for p in planes:
        h.update(np.ascontiguousarray(p.astype("<u2")).tobytes())
    return h.hexdigest()


def edge_fixtures():
    out = []
    for name in json.load(open(os.path.join(GOLDEN, "index_edges.json"))):
        meta = json.load(open(os.path.join(GOLDEN, name + ".json")))
        meta["obu"] = open(os.path.join(GOLDEN, name + ".obu"), "rb").read()
        out.append(meta)
    return out


@pytest.fixture(scope="module")
def av1mi():
    return host_build.library()


@pytest.mark.parametrize("case", E.CASES, ids=[c["name"] for c in E.CASES])
def test_oracle_decodes_in_dav1d(oracle, case):
    """Every edge case the GPU is held to: dav1d decodes the oracle's chunk to the oracle's reconstruction (film grain: a bounded
    perturbation of it), so the oracle is a sound reference there."""
    import oracle_avif
    if not oracle_avif.have_libavif():
        pytest.skip("libavif (dav1d) is not available on this machine")
    frames = E.source(oracle, case)
    for f in frames:
        assert all(p.max() <= E.maxv_of(case["bd"]) for p in f)
    tus, recs, _ = E.oracle_encode(oracle, case, frames)
    got = E.dav1d_decode(tus, case["w"], case["h"], case["bd"], case["params"].get("keyint", 1))
    assert E.decodes_to(got, recs, case["bd"], case["params"].get("film_grain", 0)) is None


def test_edge_fixtures_are_reproduced(oracle):
    """The committed edge fixtures: the generator gives the recorded source, the oracle the recorded stream, and its reconstruction is
    what dav1d decoded from that stream."""
    fx = edge_fixtures()
    assert len(fx) >= 10 and sorted(m["name"] for m in fx) == sorted(E.FIXTURES)
    for m in fx:
        assert m["case"] == json.loads(json.dumps(E.case(m["name"]))), m["name"]   # the matrix still holds the case the fixture was made from
        frames = E.source(oracle, m["case"])
        assert [sha(f) for f in frames] == m["src_sha256"], m["name"]
        tus, recs, sse = E.oracle_encode(oracle, m["case"], frames)
        assert [len(t) for t in tus] == m["frame_bytes"] and b"".join(tus) == m["obu"], m["name"]
        assert [sha(r) for r in recs] == m["dav1d_sha256"] and sse == m["sse"], m["name"]


def test_patterns_reach_both_extremes():
    """The generators do what the edge cases rely on: every pattern holds 0 and maxv in luma and chroma, U is the opposite extreme of
    V, odd frames sit half a sample off (mid-level samples on the edges), and the DCT sign blocks drive single coefficients."""
    for bd, pat in itertools.product((8, 10), E.PATTERNS):
        mx = E.maxv_of(bd)
        y, u, v = E.frame(pat, 128, 64, bd, bs=5, t=0)
        assert y.shape == (64, 128) and u.shape == v.shape == (32, 64)
        assert y.min() == 0 and y.max() == mx and u.min() == 0 and u.max() == mx, (pat, bd)
        assert np.array_equal(u.astype(int) + v, np.full(u.shape, mx)), pat
        y1 = E.frame(pat, 128, 64, bd, bs=5, t=1)[0]
        assert not np.array_equal(y1, y) and 0 < np.count_nonzero((y1 > 0) & (y1 < mx)), pat
    # a 32x32 DCT sign block puts most of its AC energy into its own basis function
    y = E.frame("dct_signs", 128, 64, 10, bs=5)[0].astype(np.float64)
    n = 32
    k = np.arange(n)
    basis = np.cos(np.pi * (2 * k[None, :] + 1) * k[:, None] / (2 * n))
    for by in range(2):
        for bx in range(4):
            c = basis @ y[by * n:(by + 1) * n, bx * n:(bx + 1) * n] @ basis.T
            c[0, 0] = 0
            if np.abs(c).max() < 1e-6 * np.abs(y).max():
                continue   # a DC block: flat at one extreme
            top = np.sort(np.abs(c).ravel())[::-1]
            assert top[0] > 2 * top[1], (bx, by)


def test_cq_level_0_is_refused(av1mi, oracle):
    """cq_level 0 is base_q_idx 0: with no segmentation and no delta-q every frame is CodedLossless (spec 5.9.2), whose header and 4x4
    WHT blocks this encoder does not write.  The parameter check refuses it, the oracle refuses base_q_idx 0; CQ 1 (base_q_idx 4) is the
    finest quantiser, and cq_to_qindex keeps the aom table."""
    with pytest.raises(av1mi.EncodeFailed) as ei:
        av1mi.write_headers(av1mi.default_params(72, 56, 8, cq_level=0))
    assert ei.value.code == av1mi.E_INVALID_ARG
    assert [av1mi.cq_to_qindex(i) for i in range(64)] == [0] + E.QINDEX[1:]
    for cq in (1, 63):
        av1mi.write_headers(av1mi.default_params(72, 56, 8, cq_level=cq))
    with pytest.raises(av1mi.EncodeFailed) as ei:
        av1mi.write_headers(av1mi.default_params(72, 56, 8, cq_level=64))
    assert ei.value.code == av1mi.E_INVALID_ARG
    src = oracle.synthclip_frame(72, 56, 8, seed=3, t=0)
    with pytest.raises(RuntimeError):
        oracle.encode_frame(oracle.default_config(72, 56, 8, base_q_idx=0), src)
    oracle.encode_frame(oracle.default_config(72, 56, 8, base_q_idx=4), src)


TRIPLES = [t for t in itertools.product((0, 1, 2, 9), (0, 1, 13, 16), (0, 1, 9)) if t != (1, 13, 0)]


@pytest.mark.parametrize("cr", [0, 1])
def test_colour_description_never_writes_zero(av1mi, oracle, cr):
    """color_config of this 4:2:0 stream: a description is written when any of CP / TC / MC is set, and then no field is 0 - a field left
    at 0 is written as 2 (unspecified): MC 0 is MC_IDENTITY, which 4:2:0 forbids (spec 5.5.2), and CP / TC 0 are reserved.  Full triples
    are written as given (their streams stay as they were), no triple writes no description; the oracle writes the same header."""
    for cp, tc, mc in TRIPLES:
        kw = dict(color_primaries=cp, transfer_characteristics=tc, matrix_coefficients=mc, color_range=cr)
        seq, _, _ = av1mi.write_headers(av1mi.default_params(200, 120, 10, **kw))
        desc, wcp, wtc, wmc, wcr = E.color_config(seq)
        assert desc == (1 if (cp or tc or mc) else 0) and wcr == cr, kw
        assert 0 not in (wcp, wtc, wmc), kw
        assert (wcp, wtc, wmc) == (cp or 2, tc or 2, mc or 2), kw
        buf = C.create_string_buffer(64)
        n = oracle.lib().av1o_write_sequence_header(C.byref(oracle.default_config(200, 120, 10, **kw)), buf, 64)
        assert buf.raw[:n] == seq, kw
    with pytest.raises(av1mi.EncodeFailed):   # sRGB + identity implies 4:4:4: still refused
        av1mi.write_headers(av1mi.default_params(64, 64, 8, color_primaries=1, transfer_characteristics=13, matrix_coefficients=0))


def test_partial_triple_reads_back_as_unspecified(oracle):
    """9 / 16 / 0 (the triple the Matroska muxer used to disagree with): libavif's own parser of the oracle's stream reads MC 2, and dav1d
    decodes it to the reconstruction."""
    import oracle_avif
    if not oracle_avif.have_libavif():
        pytest.skip("libavif (dav1d) is not available on this machine")
    src = oracle.synthclip_frame(72, 56, 10, seed=4, t=0)
    tu, rec, _ = oracle.encode_frame(oracle.default_config(72, 56, 10, color_primaries=9, transfer_characteristics=16), src)
    assert tuple(oracle_avif.decode_colour(oracle_avif.wrap_avif(tu, 72, 56, 10))) == (9, 16, 2, 0)
    dec = oracle_avif.decode_obus(tu, 72, 56, 10)
    assert all(np.array_equal(d, r) for d, r in zip(dec, rec))


@pytest.mark.parametrize("w,h,tile_sb,ok", [(8192, 16, 0, True), (8194, 16, 0, False), (4096, 16, 1, True), (4098, 16, 1, False),
                                            (4160, 16, 0, True), (16, 8192, 0, True), (16, 8194, 0, False)])
def test_tile_count_limit(av1mi, w, h, tile_sb, ok):
    """AV1 allows at most 64 tile columns / rows: beyond 64 superblocks the encoder uses tiles of 2 x 2 superblocks by itself (4160 = 65
    superblocks), 8192 samples (128 superblocks) is the widest frame that fits, and one more superblock is AV1MI_E_UNSUPPORTED; with
    tile_sb = 1 the limit is 64 superblocks."""
    p = av1mi.default_params(w, h, 8, tile_sb=tile_sb)
    if ok:
        av1mi.write_headers(p)
    else:
        with pytest.raises(av1mi.EncodeFailed) as ei:
            av1mi.write_headers(p)
        assert ei.value.code == av1mi.E_UNSUPPORTED
