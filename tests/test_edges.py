"""GPU edge tests: tiny and thin frames, extreme quantisers and strengths, full-range patterned content (tests/edge_content.py), each
checked three ways - (a) bitstream, reconstruction and the reported SSE equal the oracle's, (b) dav1d decodes the GPU's stream to the
GPU's reconstruction, (c) with the GPU-only tools (cdef_search 4, enable_lr 4), which have no oracle: dav1d decodes the stream to the
reconstruction and two runs give the same bytes, (d) the same for the encoder-side decisions together (edge_content.DECISION_TOOLS).
Without libavif the dav1d checks are replaced by the committed edge fixtures."""
import hashlib
import json
import os

import numpy as np
import pytest

import edge_content as E

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def raw_of(planes, bd):
    dt = np.uint8 if bd == 8 else np.dtype("<u2")
    return b"".join(p.astype(dt).tobytes() for p in planes)


def sha(planes):
    h = hashlib.sha256()
    for p in planes:
        h.update(np.ascontiguousarray(p.astype("<u2")).tobytes())
    return h.hexdigest()


def split_frames(recon, w, h, bd, n):
    dt = np.uint8 if bd == 8 else np.dtype("<u2")
    a = np.frombuffer(recon.tobytes(), dtype=dt)
    fs, out = w * h * 3 // 2, []
    for t in range(n):
        f = a[t * fs:(t + 1) * fs]
        out.append([f[:w * h].reshape(h, w), f[w * h:w * h * 5 // 4].reshape(h // 2, w // 2), f[w * h * 5 // 4:].reshape(h // 2, w // 2)])
    return out


def encode(av1mi, ctx, case, frames):
    p = av1mi.default_params(case["w"], case["h"], case["bd"], **case["params"])
    data, sizes, rep, recon = ctx.encode_chunk(p, b"".join(raw_of(f, case["bd"]) for f in frames), case["n"], want_recon=True)
    tus, off = [], 0
    for s in sizes:
        tus.append(data[off:off + s])
        off += s
    assert off == len(data) == rep.bytes and rep.frames == case["n"]
    return tus, split_frames(recon, case["w"], case["h"], case["bd"], case["n"]), rep


def check_dav1d(case, tus, recs):
    import oracle_avif
    if not oracle_avif.have_libavif():
        return False
    got = E.dav1d_decode(tus, case["w"], case["h"], case["bd"], case["params"].get("keyint", 1))
    bad = E.decodes_to(got, recs, case["bd"], case["params"].get("film_grain", 0))
    assert bad is None, "dav1d decodes the GPU stream to something else than the GPU reconstruction: %s" % (bad,)
    return True


@pytest.mark.parametrize("case", E.CASES, ids=[c["name"] for c in E.CASES])
def test_edge_case_equals_oracle_and_decodes(av1mi, ctx, oracle, case):
    frames = E.source(oracle, case)
    tus, recs, rep = encode(av1mi, ctx, case, frames)
    otus, orecs, osse = E.oracle_encode(oracle, case, frames)
    assert [len(t) for t in tus] == [len(t) for t in otus]
    for i, (a, b) in enumerate(zip(tus, otus)):
        assert a == b, "frame %d" % i
    for i, (a, b) in enumerate(zip(recs, orecs)):
        for pl in range(3):
            assert np.array_equal(a[pl], b[pl]), "reconstruction of frame %d plane %d" % (i, pl)
    assert [int(x) for x in rep.sse] == osse
    check_dav1d(case, tus, recs)


@pytest.mark.parametrize("case", E.GPU_ONLY_CASES, ids=[c["name"] for c in E.GPU_ONLY_CASES])
def test_gpu_only_tools_decode_and_repeat(av1mi, ctx, oracle, case):
    frames = E.source(oracle, case)
    tus, recs, rep = encode(av1mi, ctx, case, frames)
    tus2, recs2, rep2 = encode(av1mi, ctx, case, frames)
    assert tus == tus2 and [int(x) for x in rep.sse] == [int(x) for x in rep2.sse]
    assert all(np.array_equal(a[pl], b[pl]) for a, b in zip(recs, recs2) for pl in range(3))
    check_dav1d(case, tus, recs)


@pytest.mark.parametrize("case", E.DECISION_CASES, ids=[c["name"] for c in E.DECISION_CASES])
def test_decision_tools_decode_and_repeat(av1mi, ctx, oracle, case):
    """the AQ map, the deblocking level search, the CDEF search and restoration with both fits, the rate term and units of 256 together:
    the only check of the syntax of their combination at tiny frames (each decision has its own restatement elsewhere)"""
    frames = E.source(oracle, case)
    tus, recs, rep = encode(av1mi, ctx, case, frames)
    tus2, recs2, rep2 = encode(av1mi, ctx, case, frames)
    assert tus == tus2 and [int(x) for x in rep.sse] == [int(x) for x in rep2.sse]
    assert all(np.array_equal(a[pl], b[pl]) for a, b in zip(recs, recs2) for pl in range(3))
    check_dav1d(case, tus, recs)


def test_edge_fixtures_through_the_c_abi(av1mi, ctx, oracle):
    """The dav1d-pinned edge fixtures (tests/golden/index_edges.json): the GPU writes the committed stream, and every frame of its
    reconstruction hashes to what dav1d decoded - the check that stands in for (b) on a machine without libavif."""
    gdir = os.path.join(ROOT, "tests", "golden")
    names = json.load(open(os.path.join(gdir, "index_edges.json")))
    assert len(names) >= 10
    for name in names:
        m = json.load(open(os.path.join(gdir, name + ".json")))
        obu = open(os.path.join(gdir, name + ".obu"), "rb").read()
        case = m["case"]
        case["content"] = tuple(case["content"])
        tus, recs, rep = encode(av1mi, ctx, case, E.source(oracle, case))
        assert b"".join(tus) == obu and [len(t) for t in tus] == m["frame_bytes"], name
        assert [sha(r) for r in recs] == m["dav1d_sha256"], name
        assert [int(x) for x in rep.sse] == m["sse"], name


@pytest.mark.parametrize("w,h,tile_sb", [(8192, 16, 0), (4096, 16, 1)])
def test_widest_frames_the_tile_limit_allows(av1mi, ctx, oracle, w, h, tile_sb):
    """64 tile columns, the most AV1 allows: 8192 samples in tiles of 2 x 2 superblocks (chosen by itself), 4096 with tile_sb = 1 - one key
    and one P frame, equal to the oracle, decoded by dav1d; one superblock more is refused before anything runs."""
    case = dict(name="wide", w=w, h=h, bd=8, n=2, content=("steps8_v", (3, 0)), params=dict(keyint=2, tile_sb=tile_sb, subpel=1))
    frames = E.source(oracle, case)
    tus, recs, rep = encode(av1mi, ctx, case, frames)
    otus, orecs, osse = E.oracle_encode(oracle, case, frames)
    assert tus == otus and all(np.array_equal(a[pl], b[pl]) for a, b in zip(recs, orecs) for pl in range(3))
    assert [int(x) for x in rep.sse] == osse
    check_dav1d(case, tus, recs)
    p = av1mi.default_params(w + 2, h, 8, tile_sb=tile_sb)
    with pytest.raises(av1mi.EncodeFailed) as ei:
        ctx.encode_chunk(p, bytes((w + 2) * h * 3 // 2), 1)
    assert ei.value.code == av1mi.E_UNSUPPORTED


def test_cq_level_0_is_refused_by_the_encoder(av1mi, ctx):
    p = av1mi.default_params(72, 56, 8, cq_level=0)
    with pytest.raises(av1mi.EncodeFailed) as ei:
        ctx.encode_chunk(p, bytes(72 * 56 * 3 // 2), 1)
    assert ei.value.code == av1mi.E_INVALID_ARG
