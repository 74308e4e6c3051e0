"""Tests of the film-grain estimate (include/av1mi.h: av1mi_params.film_grain bit 8, av1mi_film_grain_estimate, av1mi_film_grain_result;
DESIGN.md §3 item 7b).

The pass is restated with tests/fg_ref.py and compared exactly - blocks, counts and table.  What the encoder does with the table is held
against the fixed mode (same reconstruction, same tile data) and against the restatement's film_grain_params string; what a decoder makes of
it against dav1d (libavif): the grain it adds has the standard deviation the table asks for.  The first test needs no GPU: the restatement
alone, against the noise the clip was made with."""
import os
import sys

import numpy as np
import pytest

import edge_content
import fg_ref
from test_lr_chroma import split_frames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# w, h, bit depth, frames: no block at all; 4 x 3 blocks; 10 bits; a size that is no multiple of 8 (the coded size is padded, the
# padding must not count) with an odd number of blocks per row (a pair with one block); more than one workgroup at 10 bits (75 steps,
# one each)
SIZES = [(8, 8, 8, 1), (72, 56, 8, 3), (136, 72, 10, 2), (202, 122, 8, 2), (328, 248, 10, 2)]
N = 50   # the ceiling: 100 luma, 50 chroma - above the left half's 64 sigma = 32, below the right half's 80 for chroma

_clips = {}


def the_clip(kind, w, h, bd, n):
    """(bytes, the restatement's (table, counts, blocks) at the ceiling N) - computed once per clip and left unchanged"""
    key = (kind, w, h, bd, n)
    if key not in _clips:
        if kind == "two_level":
            raw = fg_ref.two_level_clip(w, h, bd, n)
        elif kind == "two_level_x4":   # a quarter of the frames, four times over: the records are per block
            raw = fg_ref.two_level_clip(w, h, bd, n // 4) * 4
        elif kind == "checker":
            raw = fg_ref.checker_clip(w, h, bd, n)
        else:
            import av1o
            raw = fg_ref.join([av1o.synthclip_frame(w, h, bd, seed=1080, t=t) for t in range(n)], bd)
        _clips[key] = (raw, fg_ref.estimate(raw, w, h, bd, n, N))
    return _clips[key]


# ---------------------------------------------------------------- the restatement alone (CPU)
@pytest.mark.parametrize("w,h,bd,n", SIZES[1:])
def test_restatement_finds_the_noise_it_was_given(w, h, bd, n):
    """each level covers at least 16 whole blocks, and the unclamped value of its bin lies within 15 % (luma) / 25 % (chroma) of 64 sigma.
    Measured, value / (64 sigma) over the four sizes: luma 0.91 - 1.03, chroma 0.75 - 1.00 (the quartile of few small blocks reads low)"""
    raw, (_, counts, blocks) = the_clip("two_level", w, h, bd, n)
    table, _ = fg_ref.table_of(blocks, 255, 255)
    for level, sigma in zip(fg_ref.LEVEL, fg_ref.SIGMA):
        b = level >> 5
        assert counts[0][b] >= 16 and (counts[1] == counts[0]).all() and (counts[2] == counts[0]).all()
        for pl in range(3):
            ratio = int(table[pl][b]) / (64 * sigma)
            print("%dx%dx%d level %d plane %d: value %d, ratio %.3f" % (w, h, bd, level, pl, table[pl][b], ratio))
            assert abs(int(table[pl][b]) - 64 * sigma) <= (0.25 if pl else 0.15) * 64 * sigma, (level, pl, ratio)


# ---------------------------------------------------------------- (1) the pass equals the restatement
@pytest.fixture(scope="module")
def ctx(av1mi):
    c = av1mi.Context(0)
    yield c
    c.close()


# ... and more than one step of a workgroup: 35 x 58 blocks of 16 frames are 4176 steps for the grid's 4096 workgroups (every row's last
# pair lacks its right block)
CONTENT = [("two_level",) + s for s in SIZES] + [("synth", 202, 122, 8, 2), ("synth", 136, 72, 10, 2), ("checker", 72, 56, 8, 3), ("checker", 136, 72, 10, 2),
                                                 ("two_level_x4", 568, 928, 8, 16)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,w,h,bd,n", CONTENT)
def test_pass_equals_the_rule(av1mi, ctx, kind, w, h, bd, n):
    import torch
    raw, (table, counts, blocks) = the_clip(kind, w, h, bd, n)
    dev = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()
    p = av1mi.default_params(w, h, bd, film_grain_estimate=N)
    for where, (t, c, b) in (("host input", ctx.film_grain_estimate(p, raw, n)), ("device input", ctx.film_grain_estimate(p, dev.data_ptr(), n, on_device=True))):
        assert b.shape == blocks.shape, where
        bad = [i for i in np.ndindex(b.shape[:3]) if not np.array_equal(b[i], blocks[i])]
        assert not bad, (where, bad[:4], [(b[i].tolist(), blocks[i].tolist()) for i in bad[:4]])
        assert np.array_equal(c, counts), (where, c.tolist(), counts.tolist())
        assert np.array_equal(t, table), (where, t.tolist(), table.tolist())
    cy, cc = fg_ref.ceilings(N)
    if (w, h) == (8, 8):
        assert not table.any() and not counts.any()   # no block: no grain
    elif kind == "synth":                              # textured everywhere: the ceiling, i.e. the fixed table
        assert (table[0] == cy).all() and (table[1:] == cc).all()
    elif kind == "checker":
        assert (blocks[..., 1:] == 255).all() and (table[0] == cy).all() and (table[1:] == cc).all()
    else:                                              # the estimate tells the halves apart, and stays below the ceiling where the noise does
        assert table[0][2] < table[0][6] <= cy and table[0][2] < 40 and (table[1:, 6] == cc).all() and (table[1:, 2] < 40).all()
    # a lower ceiling clamps the same estimate
    t1, c1, _ = ctx.film_grain_estimate(av1mi.default_params(w, h, bd, film_grain_estimate=7), raw, n, want_blocks=False)
    want1, _ = fg_ref.table_of(blocks, *fg_ref.ceilings(7))
    assert np.array_equal(t1, want1) and np.array_equal(c1, counts)


@pytest.mark.gpu
def test_pass_refuses_what_is_not_the_estimate(av1mi, ctx):
    raw, _ = the_clip("two_level", 72, 56, 8, 3)
    for fg in (0, 20):
        with pytest.raises(av1mi.EncodeFailed) as e:
            ctx.film_grain_estimate(av1mi.default_params(72, 56, 8, film_grain=fg), raw, 3)
        assert e.value.code == 1


# ---------------------------------------------------------------- (2) the chunk: the fixed mode's reconstruction and tiles, the pass's table
def obus(tu):
    """[(type, payload)] of a temporal unit"""
    out, at = [], 0
    while at < len(tu):
        typ, has_size = (tu[at] >> 3) & 15, tu[at] & 2
        assert has_size and not tu[at] & 4
        at += 1
        size = shift = 0
        while True:
            b = tu[at]
            at += 1
            size |= (b & 127) << shift
            shift += 7
            if not b & 128:
                break
        out.append((typ, tu[at:at + size]))
        at += size
    return out


def frame_payloads(data, sizes):
    out, off = [], 0
    for s in sizes:
        fr = [p for t, p in obus(data[off:off + s]) if t == 6]   # OBU_FRAME
        assert len(fr) == 1
        out.append(fr[0])
        off += s
    assert off == len(data)
    return out


def encode(ctx, av1mi, raw, w, h, bd, n, **kw):
    p = av1mi.default_params(w, h, bd, **kw)
    data, sizes, rep, rec = ctx.encode_chunk(p, raw, n, want_recon=True)
    return data, sizes, rep, split_frames(rec.tobytes(), w, h, bd, n)


def same_frames(a, b):
    return all(np.array_equal(x, y) for fa, fb in zip(a, b) for x, y in zip(fa, fb))


CHUNKS = [(202, 122, 8, 2, dict(keyint=1)), (202, 122, 8, 2, dict(keyint=240, first_frame=9)),
          (328, 248, 10, 2, dict(keyint=240, deblock=2, cdef_search=2, enable_lr=2, tf_frames=1, tf_strength=2))]


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,bd,n,kw", CHUNKS)
def test_chunk_carries_the_pass_table(av1mi, w, h, bd, n, kw):
    """all key frames and IPPP; with the header-patching searches and the temporal filter on: the estimate reads the caller's frames,
    before the filter, and its values stand in front of the searches' in the headers"""
    raw, (table, counts, _) = the_clip("two_level", w, h, bd, n)
    with av1mi.Context(0) as c:
        d0, s0, _, r0 = encode(c, av1mi, raw, w, h, bd, n, film_grain=N, **kw)
        assert not c.film_grain_result().any()          # a chunk without the estimate
        d1, s1, _, r1 = encode(c, av1mi, raw, w, h, bd, n, film_grain_estimate=N, **kw)
        got = c.film_grain_result()
        alone, alone_counts, _ = c.film_grain_estimate(av1mi.default_params(w, h, bd, film_grain_estimate=N, **kw), raw, n, want_blocks=False)
        d2, s2, _, r2 = encode(c, av1mi, raw, w, h, bd, n, film_grain_estimate=N, **kw)   # the same workspace again
        d3, s3, _, r3 = encode(c, av1mi, raw, w, h, bd, n, film_grain=N, **kw)            # ... and the mode off again
    assert np.array_equal(got, table) and np.array_equal(alone, table) and np.array_equal(alone_counts, counts)
    assert same_frames(r0, r1) and (d2, s2) == (d1, s1) and same_frames(r1, r2) and (d3, s3) == (d0, s0)
    first = kw.get("first_frame", 0)
    for f, (fix, est) in enumerate(zip(frame_payloads(d0, s0), frame_payloads(d1, s1))):
        inter = int(f % kw["keyint"] != 0)
        seed = fg_ref.grain_seed(first, f)
        ftail, tail = fg_ref.fixed_bits(N, seed, inter), fg_ref.params_bits(table, seed, inter)
        fb, eb = fg_ref.header_bits(fix, 512 * 8 if len(fix) > 512 else len(fix) * 8), fg_ref.header_bits(est, 548 * 8 if len(est) > 548 else len(est) * 8)
        at = [i for i in range(len(fb) - len(ftail) + 1) if fb[i:i + len(ftail)] == ftail]
        assert len(at) == 1, (f, at)                     # where the fixed header's film_grain_params stand
        head = at[0]
        assert len(est) == len(fix) + 36, f               # 288 bits
        assert eb[:head] == fb[:head], f                 # everything before them, the other searches' fields included
        assert eb[head:head + len(tail)] == tail, f      # the pass's table
        assert est[(head + len(tail) + 7) // 8:] == fix[(head + len(ftail) + 7) // 8:], f   # and the same tiles behind


# ---------------------------------------------------------------- (3) dav1d adds the grain the table asks for
@pytest.mark.gpu
@pytest.mark.parametrize("w,h,bd,n", [(202, 122, 8, 2), (328, 248, 10, 2)])
def test_dav1d_adds_the_tables_grain(av1mi, w, h, bd, n):
    """decoded minus reconstruction has, per half and plane, a standard deviation within 15 % of table / 64 * 2^(bd - 8) wherever the
    table's value is at least 40 (measured with fixed tables of 40 / 100 / 255 on oracle streams: within 9 %)"""
    import oracle_avif
    if not oracle_avif.have_libavif():
        pytest.skip("libavif (dav1d) is not available on this machine")
    raw, (table, _, _) = the_clip("two_level", w, h, bd, n)
    with av1mi.Context(0) as c:
        data, sizes, _, rec = encode(c, av1mi, raw, w, h, bd, n, film_grain_estimate=N, keyint=1)
        assert np.array_equal(c.film_grain_result(), table)
    tus, off = [], 0
    for s in sizes:
        tus.append(data[off:off + s])
        off += s
    got = edge_content.dav1d_decode(tus, w, h, bd, 1)
    assert edge_content.decodes_to(got, rec, bd, N) is None
    xs, checked = fg_ref.split_column(w), 0
    for pl in range(3):
        at = xs if pl == 0 else xs // 2
        diff = np.concatenate([(np.asarray(got[f][pl]).astype(np.int64) - rec[f][pl])[None] for f in range(n)])
        for half, region in ((0, diff[:, :, :at]), (1, diff[:, :, at:])):
            value = int(table[pl][fg_ref.LEVEL[half] >> 5])
            want = value / 64.0 * (1 << (bd - 8))
            sd = float(region.std())
            print("%dx%dx%d plane %d half %d: table %d, sigma %.3f, wanted %.3f" % (w, h, bd, pl, half, value, sd, want))
            if value >= 40:
                assert abs(sd - want) <= 0.15 * want, (pl, half, value, sd, want)
                checked += 1
    assert checked >= 3   # the right half of every plane
