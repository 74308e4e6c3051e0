"""GPU tests of the key frames' temporal filter (include/av1mi.h: av1mi_params.me_presearch bits 8-14, av1mi_temporal_filter; DESIGN.md
§3 item 8d, §4.5c).  Every comparison is exact.

The filter is a pre-processing of the source: its output equals the numpy restatement (tests/tf_ref.py; cases and content in
tests/tf_cases.py), and a chunk encoded with the filter on equals - bytes, frame sizes, reconstruction, report - the chunk with the
filtered key frames encoded with the filter off, so that the frozen oracle stays the reference of everything downstream."""
import numpy as np
import pytest

import edge_content as E
import tf_cases
import tf_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(av1mi):
    c = av1mi.Context(0)
    yield c
    c.close()


def params_of(av1mi, case, **extra):
    w, h, bd, n, keyint, N, s, R = case
    return av1mi.default_params(w, h, bd, keyint=keyint, me_range=R, tf_frames=N, tf_strength=s, **extra)


# ---------------------------------------------------------------- 1. the filter equals the restatement
@pytest.mark.parametrize("case", tf_cases.FILTER_CASES, ids=tf_cases.case_id)
def test_filter_equals_the_restatement(av1mi, ctx, case):
    import torch
    w, h, bd, n = case[:4]
    tf_cases.exercises_the_rule(case)
    raw = tf_cases.content(w, h, bd, n)[0]
    want, want_mv, _ = tf_cases.reference(case)
    p = params_of(av1mi, case)
    got, mv = ctx.temporal_filter(p, raw, n)
    assert mv.shape == want_mv.shape and np.array_equal(mv, want_mv), "host input: vectors"
    assert got.tobytes() == want, "host input"
    dev = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()
    out = torch.zeros_like(dev)
    _, mv = ctx.temporal_filter(p, dev.data_ptr(), n, on_device=True, out_ptr=out.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(mv, want_mv), "device input: vectors"
    assert out.cpu().numpy().tobytes() == want, "device input"
    assert dev.cpu().numpy().tobytes() == raw, "the caller's frames were written"
    # ... and at an address that is no multiple of 16 (the filter works on a copy of its own: any sample-aligned address is taken)
    buf = torch.zeros(len(raw) + 16, dtype=torch.uint8, device="cuda")
    off = 8 if buf.data_ptr() % 16 == 0 else 0
    buf[off:off + len(raw)] = dev
    out.zero_()
    _, mv = ctx.temporal_filter(p, buf.data_ptr() + off, n, on_device=True, out_ptr=out.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(mv, want_mv) and out.cpu().numpy().tobytes() == want, "device input at an odd address"


def test_zeros_followed_by_all_max_is_the_identity(av1mi, ctx):
    """16x16 at 10 bit: 9 B = 9 * 256 * 1023^2 > 2^31 - no overflow, every weight 0, the key frame comes back"""
    z = tf_cases.zeros_then_max()
    want, want_mv, _ = tf_ref.filter_chunk(z, 16, 16, 10, 3, 3, 2, 0, 8)
    assert want == z
    got, mv = ctx.temporal_filter(av1mi.default_params(16, 16, 10, keyint=3, tf_frames=2, tf_strength=0), z, 3)
    assert got.tobytes() == z and np.array_equal(mv, want_mv)


# ---------------------------------------------------------------- 2. filter on = filter off on the filtered key frames
def encode(ctx, p, raw, n):
    data, sizes, rep, rec = ctx.encode_chunk(p, raw, n, want_recon=True)
    return data, list(sizes), rec.tobytes(), [int(x) for x in rep.sse]


IDENTITY_CASES = [
    ((72, 56, 8, 4, 4, 3, 2, 8), dict()),
    ((202, 122, 8, 3, 3, 2, 3, 8), dict(subpel=1, me_presearch=1, partition_search=2, min_block_log2=3)),
    ((136, 72, 10, 3, 240, 7, 2, 16), dict(aq_strength=2, deblock=2, enable_lr=4, cdef_search=2)),
]


@pytest.mark.parametrize("case,extra", IDENTITY_CASES, ids=[tf_cases.case_id(c) for c, _ in IDENTITY_CASES])
def test_encode_equals_the_encode_of_the_filtered_frames(av1mi, ctx, case, extra):
    w, h, bd, n, keyint, N, s, R = case
    raw = tf_cases.content(w, h, bd, n)[0]
    filtered = tf_cases.reference(case)[0]
    assert filtered != raw
    on = encode(ctx, params_of(av1mi, case, **extra), raw, n)
    off = encode(ctx, av1mi.default_params(w, h, bd, keyint=keyint, me_range=R, **extra), filtered, n)
    for a, b, what in zip(on, off, ("bytes", "frame sizes", "reconstruction", "report SSE")):
        assert a == b, what
    plain = encode(ctx, av1mi.default_params(w, h, bd, keyint=keyint, me_range=R, **extra), raw, n)
    assert plain[0] != on[0]   # (the filter does change what is coded)


def test_device_resident_chunk_is_not_written(av1mi, ctx):
    """an unpadded chunk on the device is used in place without the filter; with it the library works on a copy"""
    import torch
    case = (72, 56, 8, 4, 4, 3, 2, 8)
    w, h, bd, n, keyint, N, s, R = case
    raw = tf_cases.content(w, h, bd, n)[0]
    dev = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()
    p = params_of(av1mi, case)
    data, sizes, rep, _ = ctx.encode_chunk(p, dev.data_ptr(), n, on_device=True)
    torch.cuda.synchronize()
    assert dev.cpu().numpy().tobytes() == raw
    off = encode(ctx, av1mi.default_params(w, h, bd, keyint=keyint, me_range=R), tf_cases.reference(case)[0], n)
    assert (data, list(sizes), [int(x) for x in rep.sse]) == (off[0], off[1], off[3])


# ---------------------------------------------------------------- 3. the oracle
def test_first_temporal_unit_equals_the_oracle_on_the_filtered_key_frame(av1mi, ctx, oracle):
    case = (72, 56, 8, 4, 4, 3, 2, 8)
    w, h, bd, n, keyint, N, s, R = case
    raw = tf_cases.content(w, h, bd, n)[0]
    data, sizes, rec, _ = encode(ctx, params_of(av1mi, case), raw, n)
    key = tf_ref.split(tf_cases.reference(case)[0], w, h, bd, n)[0]
    cfg = E.oracle_config(oracle, dict(w=w, h=h, bd=bd, params=dict(keyint=keyint, me_range=R)), 0)
    tu, want_rec, _ = oracle.encode_frame(cfg, key, with_seq_hdr=True)
    assert sizes[0] == len(tu) and data[:sizes[0]] == tu
    got = tf_ref.split(rec, w, h, bd, n)[0]
    assert all(np.array_equal(got[pl], np.asarray(want_rec[pl]).astype(np.int64)) for pl in range(3))


# ---------------------------------------------------------------- 4. no-ops
def test_no_followers_and_switching(av1mi, ctx):
    """keyint = 1 and a one-frame chunk give the bytes of the filter off; a context may switch the filter from chunk to chunk"""
    w, h, bd, n = 72, 56, 8, 4
    raw = tf_cases.content(w, h, bd, n)[0]
    one = raw[:w * h * 3 // 2]
    off_all_key = encode(ctx, av1mi.default_params(w, h, bd, keyint=1), raw, n)
    assert encode(ctx, av1mi.default_params(w, h, bd, keyint=1, tf_frames=3, tf_strength=2), raw, n) == off_all_key
    off_one = encode(ctx, av1mi.default_params(w, h, bd, keyint=4), one, 1)
    assert encode(ctx, av1mi.default_params(w, h, bd, keyint=4, tf_frames=3, tf_strength=2), one, 1) == off_one
    got, mv = ctx.temporal_filter(av1mi.default_params(w, h, bd, keyint=1, tf_frames=3, tf_strength=2), raw, n)
    assert got.tobytes() == raw and (mv == tf_ref.NONE).all()
    # on, off, on with other settings, off: each chunk is what a fresh context gives
    seq = [dict(tf_frames=3, tf_strength=2), dict(), dict(tf_frames=1, tf_strength=5), dict()]
    runs = [encode(ctx, av1mi.default_params(w, h, bd, keyint=4, **kw), raw, n) for kw in seq]
    assert runs[1] == runs[3] and runs[0] != runs[1] and runs[2] != runs[1] and runs[0] != runs[2]
    with av1mi.Context(0) as fresh:
        assert encode(fresh, av1mi.default_params(w, h, bd, keyint=4, **seq[2]), raw, n) == runs[2]
        assert encode(fresh, av1mi.default_params(w, h, bd, keyint=4), raw, n) == runs[1]
