"""GPU tests of the CDEF strength search (include/av1mi.h: av1mi_params.cdef_search).

The decision is restated in numpy: a key frame's reconstruction before CDEF does not depend on the CDEF strengths and CDEF reads only
pre-CDEF samples, so 16 encodes with fixed strengths (run i: luma candidate i, chroma candidate i mod 8) give every candidate's output
and squared error per 64x64 superblock; the rule picks the frame's set and each superblock's pair, and the search run's reconstruction
must equal the assembled one bit for bit.  dav1d (libavif) decodes the search's streams to the reconstruction."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

P8 = [0, 1, 2, 3, 4, 6, 8, 11]
INF = np.iinfo(np.uint64).max


def luma_cand(l):
    return P8[l >> 1], 2 * (l & 1)


def raw_of(planes, bd):
    dt = np.uint8 if bd == 8 else np.dtype("<u2")
    return b"".join(p.astype(dt).tobytes() for p in planes)


def split_frames(raw, w, h, bd, n):
    a = np.frombuffer(raw, dtype=np.uint8 if bd == 8 else np.dtype("<u2")).astype(np.int64)
    fs = w * h * 3 // 2
    out = []
    for f in range(n):
        b = a[f * fs:(f + 1) * fs]
        out.append([b[:w * h].reshape(h, w), b[w * h:w * h * 5 // 4].reshape(h // 2, w // 2), b[w * h * 5 // 4:].reshape(h // 2, w // 2)])
    return out


def clip(oracle, w, h, bd, n, seed):
    """synthclip frames with a flat band (whole superblocks with nothing to code at a coarse quantiser)"""
    frames = []
    for t in range(n):
        y, u, v = [p.copy() for p in oracle.synthclip_frame(w, h, bd, seed=seed, t=t)]
        mid = 1 << (bd - 1)
        fy, fx = min(h, 128), min(w, 192)
        y[:fy, :fx] = mid
        u[:fy // 2, :fx // 2] = mid
        v[:fy // 2, :fx // 2] = mid
        frames.append([y, u, v])
    return frames


def sb_sse(a, b, size):
    """per superblock (raster order) sum of squared differences of two planes, superblocks of size x size samples"""
    d = (a - b) ** 2
    h, w = d.shape
    rows, cols = -(-h // size), -(-w // size)
    out = np.zeros(rows * cols, dtype=np.uint64)
    for r in range(rows):
        for c in range(cols):
            out[r * cols + c] = int(d[r * size:(r + 1) * size, c * size:(c + 1) * size].sum())
    return out


def select(E, n):
    """the rule of DESIGN.md §3 item 11b: E[sb][p] (uint64) -> the set S and every superblock's index into it"""
    E = np.asarray(E, dtype=np.uint64)

    def argmin_cost(others):   # cost of every pair: sum over superblocks of min(others, E[:, p]) (exact: no term is INF)
        c = np.minimum(others[:, None], E).sum(axis=0, dtype=np.uint64)
        return int(np.argmin(c)), c   # (np.argmin: the first minimum)

    best = np.full(E.shape[0], INF, dtype=np.uint64)
    S = []
    for _ in range(n):
        p, _ = argmin_cost(best)
        S.append(p)
        best = np.minimum(best, E[:, p])
    if n > 1:
        for _ in range(2):
            for j in range(n):
                others = np.full(E.shape[0], INF, dtype=np.uint64)
                for i in range(n):
                    if i != j:
                        others = np.minimum(others, E[:, S[i]])
                p, c = argmin_cost(others)
                if c[p] < c[S[j]]:
                    S[j] = p
    idx = [int(np.argmin(E[s, S])) for s in range(E.shape[0])]
    return S, idx


def encode(ctx, av1mi, frames, w, h, bd, **kw):
    p = av1mi.default_params(w, h, bd, **kw)
    data, sizes, rep, recon = ctx.encode_chunk(p, raw_of_frames(frames, bd), len(frames), want_recon=True)
    return data, sizes, rep, recon.tobytes()


def raw_of_frames(frames, bd):
    return b"".join(raw_of(f, bd) for f in frames)


def restate(ctx, av1mi, frames, w, h, bd, k, **kw):
    """the 16 fixed-strength runs, the rule, the expected reconstruction; and the search run"""
    n_fr = len(frames)
    damping = kw.pop("cdef_damping", 5)
    runs = []
    for i in range(16):
        yp, ys = luma_cand(i)
        _, _, _, rec = encode(ctx, av1mi, frames, w, h, bd, cdef_y_pri=yp, cdef_y_sec=ys, cdef_uv_pri=P8[i % 8], cdef_uv_sec=0,
                              cdef_damping=damping, **kw)
        runs.append(split_frames(rec, w, h, bd, n_fr))
    search = encode(ctx, av1mi, frames, w, h, bd, cdef_search=k, cdef_damping=damping, **kw)
    rec_s = split_frames(search[3], w, h, bd, n_fr)
    src = [[p.astype(np.int64) for p in f] for f in frames]
    sets = []
    n = 1 << (k - 1)
    for f in range(n_fr):
        ey = np.stack([sb_sse(runs[l][f][0], src[f][0], 64) for l in range(16)], axis=1)
        euv = np.stack([sb_sse(runs[c][f][1], src[f][1], 32) + sb_sse(runs[c][f][2], src[f][2], 32) for c in range(8)], axis=1)
        E = (ey[:, :, None] + euv[:, None, :]).reshape(-1, 128)
        S, idx = select(E, n)
        sets.append(S)
        cols = -(-w // 64)
        exp = [np.empty_like(p) for p in src[f]]
        for s, j in enumerate(idx):
            r, c = divmod(s, cols)
            l, cc = S[j] >> 3, S[j] & 7
            exp[0][r * 64:(r + 1) * 64, c * 64:(c + 1) * 64] = runs[l][f][0][r * 64:(r + 1) * 64, c * 64:(c + 1) * 64]
            for pl in (1, 2):
                exp[pl][r * 32:(r + 1) * 32, c * 32:(c + 1) * 32] = runs[cc][f][pl][r * 32:(r + 1) * 32, c * 32:(c + 1) * 32]
        for pl in range(3):
            assert np.array_equal(exp[pl], rec_s[f][pl]), "frame %d plane %d" % (f, pl)
    return search, sets, runs


def header_sets(av1mi, data, sizes, w, h, bd, k, **kw):
    """cdef_bits and the strength pairs of every (key) frame header in the stream, at the offset write_headers implies"""
    def bits_of(b, n):
        return [(b[i >> 3] >> (7 - (i & 7))) & 1 for i in range(n)]
    kw.pop("cdef_damping", None)
    seq, fh1, nb1 = av1mi.write_headers(av1mi.default_params(w, h, bd, cdef_search=1, cdef_damping=5, **kw))
    _, fh2, _ = av1mi.write_headers(av1mi.default_params(w, h, bd, cdef_search=2, cdef_damping=5, **kw))
    b1, b2 = bits_of(fh1, nb1), bits_of(fh2, nb1)
    str_bit = next(i for i in range(nb1) if b1[i] != b2[i]) + 1
    out, off = [], 0
    n = 1 << (k - 1)
    for sz in sizes:
        tu = data[off:off + sz]
        off += sz
        assert tu[:2] == b"\x12\x00" and tu[2:2 + len(seq)] == seq and tu[2 + len(seq)] == 0x32
        q = 3 + len(seq)
        while tu[q] & 0x80:
            q += 1
        hb = bits_of(tu[q + 1:q + 1 + (str_bit + 12 * n + 7) // 8 + 1], str_bit + 12 * n)
        val = lambda a, m: int("".join(map(str, hb[a:a + m])), 2)
        cdef_bits = val(str_bit - 2, 2)
        pairs = []
        for j in range(n):
            o = str_bit + 12 * j
            pairs.append((val(o, 4), val(o + 4, 2), val(o + 6, 4), val(o + 10, 2)))
        out.append((cdef_bits, pairs))
    return out


def pair_fields(p):
    l, c = p >> 3, p & 7
    return (P8[l >> 1], 2 * (l & 1), P8[c], 0)


CASES = [
    # w, h, bd, frames, k, extra
    (328, 200, 8, 2, 1, dict(cq_level=50)),
    (328, 200, 10, 2, 4, dict(cq_level=20, block_log2=3)),
    (256, 192, 8, 2, 2, dict(cq_level=50, block_log2=6, deblock=1)),
    (392, 264, 10, 2, 3, dict(cq_level=50, partition_search=1, block_log2=6)),
    (648, 360, 8, 2, 4, dict(cq_level=50, intra_mode_mask=0x1FFF)),
]


@pytest.fixture(scope="module")
def ctx(av1mi):
    c = av1mi.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("w,h,bd,n,k,extra", CASES)
def test_decision_restated_and_header(av1mi, oracle, ctx, w, h, bd, n, k, extra):
    """tests 1 and 5: the search run's reconstruction is the rule's assembly of the fixed-strength runs, and every frame header carries
    cdef_bits = k - 1 and the rule's set"""
    frames = clip(oracle, w, h, bd, n, seed=700 + w + k)
    (data, sizes, rep, rec), sets, runs = restate(ctx, av1mi, frames, w, h, bd, k, **dict(extra))
    hs = header_sets(av1mi, data, sizes, w, h, bd, k, **dict(extra))
    for f in range(n):
        assert hs[f][0] == k - 1
        assert hs[f][1] == [pair_fields(p) for p in sets[f]], "frame %d" % f


def test_decision_restated_1080p_headline(av1mi, oracle, ctx):
    """the headline's parameter set at its own size: 1920x1080 10-bit, all 13 intra modes"""
    w, h, bd = 1920, 1080, 10
    frames = [oracle.synthclip_frame(w, h, bd, seed=1080, t=t) for t in range(2)]
    restate(ctx, av1mi, frames, w, h, bd, 4, intra_mode_mask=0x1FFF, enable_lr=0)


def test_decision_restated_1918x1078(av1mi, oracle, ctx):
    w, h, bd = 1918, 1078, 10
    frames = clip(oracle, w, h, bd, 1, seed=1918)
    restate(ctx, av1mi, frames, w, h, bd, 3, cq_level=20)


DECODE = [
    (328, 200, 8, 3, 4, dict(cq_level=50), None),
    (328, 248, 10, 4, 3, dict(subpel=1, deblock=1, film_grain=10, keyint=1), None),
    (328, 248, 10, 5, 4, dict(subpel=1, deblock=1, keyint=3, enable_lr=1), None),
    (200, 136, 8, 5, 2, dict(keyint=240, enable_lr=2, deblock=1, cdf_update=0), None),
    (256, 192, 8, 6, 4, dict(keyint=240, film_grain=20, subpel=1), "2"),
    (3840, 2160, 10, 2, 4, dict(keyint=2, tile_sb=2), None),
]


@pytest.mark.parametrize("w,h,bd,n,k,extra,group", DECODE)
def test_dav1d_decodes_to_the_reconstruction(av1mi, oracle, ctx, monkeypatch, w, h, bd, n, k, extra, group):
    import oracle_avif
    if not oracle_avif.have_libavif():
        pytest.skip("libavif (dav1d) is not available on this machine")
    if group is not None:
        monkeypatch.setenv("AV1MI_ENTROPY_GROUP", group)
    frames = clip(oracle, w, h, bd, n, seed=800 + w)
    extra = dict(extra)
    keyint = extra.get("keyint", 1)
    with av1mi.Context(0) as c:
        data, sizes, rep, rec = encode(c, av1mi, frames, w, h, bd, cdef_search=k, **extra)
    want = split_frames(rec, w, h, bd, n)
    tus, off = [], 0
    for s in sizes:
        tus.append(data[off:off + s])
        off += s
    if keyint == 1:
        got = [oracle_avif.decode_obus(t, w, h, bd) for t in tus]
    else:
        keys = [i + 1 for i in range(n) if i % keyint == 0]
        got = oracle_avif.decode_sequence(oracle_avif.wrap_avis(tus, w, h, bd, sync=keys), w, h)
    assert len(got) == n
    for f in range(n):
        for pl in range(3):
            g = np.asarray(got[f][pl]).astype(np.int64)
            if extra.get("film_grain"):   # the decoder adds the grain: a desynchronised stream decodes to garbage, not to noise
                mse = float(((g - want[f][pl]) ** 2).mean())
                assert mse < ((1 << bd) - 1) ** 2 / 10 ** 2.5, "frame %d plane %d" % (f, pl)
            else:
                assert np.array_equal(g, want[f][pl]), "frame %d plane %d" % (f, pl)


@pytest.mark.parametrize("w,h,bd,cq", [(328, 200, 8, 20), (648, 360, 10, 50), (1920, 1080, 10, 30)])
def test_never_worse_than_the_default_on_key_frames(av1mi, oracle, ctx, w, h, bd, cq):
    """test 3: pair 33 ((2, 0) / (1, 0), the default strengths) is in the pool, so per key frame the search's Y+U+V SSE is at most the
    default's; test 4: report.sse is numpy's SSE of the reconstruction, and two runs give the same bytes"""
    n = 3
    frames = clip(oracle, w, h, bd, n, seed=900 + w)
    src = [[p.astype(np.int64) for p in f] for f in frames]
    d0, _, r0, rec0 = encode(ctx, av1mi, frames, w, h, bd, cq_level=cq)
    d4, s4, r4, rec4 = encode(ctx, av1mi, frames, w, h, bd, cq_level=cq, cdef_search=4)
    d4b, _, _, rec4b = encode(ctx, av1mi, frames, w, h, bd, cq_level=cq, cdef_search=4)
    assert d4 == d4b and rec4 == rec4b
    a0, a4 = split_frames(rec0, w, h, bd, n), split_frames(rec4, w, h, bd, n)
    tot = [0, 0, 0]
    for f in range(n):
        e0 = sum(int(((a0[f][pl] - src[f][pl]) ** 2).sum()) for pl in range(3))
        e4 = [int(((a4[f][pl] - src[f][pl]) ** 2).sum()) for pl in range(3)]
        assert sum(e4) <= e0, "frame %d" % f
        for pl in range(3):
            tot[pl] += e4[pl]
    assert [int(x) for x in r4.sse] == tot
