"""CPU tests of the oracle (the checker) itself: golden fixtures pinned by dav1d, known-answer
tests of the building blocks, size-independent properties.  None of this needs a GPU."""
import ctypes as C
import hashlib

import numpy as np
import pytest

from ec_ref import SpecDecoder


def sha(planes):
    h = hashlib.sha256()
    for p in planes:
        h.update(np.ascontiguousarray(p.astype("<u2")).tobytes())
    return h.hexdigest()


def test_golden_streams_and_dav1d_reconstruction(oracle, golden_cases):
    """The oracle must reproduce every committed stream byte for byte, and its reconstruction
    must equal what dav1d 1.5.3 decoded from that stream (hash recorded by tools/make_golden.py)."""
    assert len(golden_cases) >= 20
    for m in golden_cases:
        src = [(pl >> m.get("src_shift", 0)) << m.get("src_shift", 0) for pl in oracle.synthclip_frame(m["width"], m["height"], m["bit_depth"], seed=m["seed"], t=m["t"])]
        assert sha(src) == m["src_sha256"], m["name"]
        cfg = oracle.default_config(m["width"], m["height"], m["bit_depth"], **m["config"])
        tu, rec, st = oracle.encode_frame(cfg, src)
        assert tu == m["obu"], "stream differs for " + m["name"]
        # dav1d's output is the reconstruction itself, except where the stream asks the decoder to add film grain
        assert m.get("dav1d_applies_grain", False) == (m["recon_sha256"] != m["dav1d_sha256"]), m["name"]
        assert sha(rec) == m["recon_sha256"], "reconstruction differs from dav1d for " + m["name"]


def test_golden_inter_sequences(oracle, golden_sequences):
    """Key frame + P frames (LAST_FRAME only, integer-pel motion, NEARESTMV/NEARMV/GLOBALMV/NEWMV, intra blocks in
    inter frames): the oracle reproduces every committed stream, and each frame's reconstruction is what dav1d decoded."""
    assert len(golden_sequences) >= 8
    modes = [0, 0, 0, 0]
    for m in golden_sequences:
        cfg = oracle.default_config(m["width"], m["height"], m["bit_depth"], **m["config"])
        ref, prev, pos = None, None, 0
        for t in range(m["frames"]):
            src = oracle.synthclip_frame(m["width"], m["height"], m["bit_depth"], seed=m["seed"], t=t * m.get("t_step", 1))
            tu, rec, st = oracle.encode_frame(cfg, src, with_seq_hdr=(t == 0), ref=ref, prev_src=prev)
            assert tu == m["obu"][pos:pos + m["frame_bytes"][t]], (m["name"], t)
            assert sha(rec) == m["dav1d_sha256"][t], (m["name"], t)
            pos += m["frame_bytes"][t]
            ref, prev = rec, src
            modes = [a + int(b) for a, b in zip(modes, st.inter_mode_hist)]
        assert pos == len(m["obu"])
    assert all(x > 50 for x in modes), modes   # every inter mode is exercised


def test_header_kat(oracle):
    """Sequence header of a 64x64 8-bit stream, hand-checked against the field order the survey
    verified on a libaom stream: OBU type 1, profile 0, level 31, 6/6 size bits."""
    cfg = oracle.default_config(64, 64, 8)
    src = oracle.synthclip_frame(64, 64, 8, seed=1, t=0)
    tu, _, _ = oracle.encode_frame(cfg, src)
    assert tu[:2] == bytes([0x12, 0x00])                 # temporal delimiter
    assert tu[2] == 0x0A and tu[3] == 10                  # sequence header OBU, 10 payload bytes
    payload = tu[4:14]
    bits = "".join("{:08b}".format(b) for b in payload)
    assert bits[0:3] == "000" and bits[3] == "0" and bits[4] == "0"      # profile, still, reduced
    assert bits[24:29] == "11111" and bits[29] == "0"                   # seq_level_idx 31, tier 0
    assert int(bits[30:34], 2) == 5 and int(bits[34:38], 2) == 5         # width/height bits - 1
    assert int(bits[38:44], 2) == 63 and int(bits[44:50], 2) == 63       # 64x64
    assert tu[14] == 0x32                                               # OBU_FRAME


def test_range_coder_roundtrip_against_spec_decoder(oracle):
    """Encode a random symbol sequence with adaptive CDFs, decode it with a straight restatement of
    the spec's symbol decoder (§8.2.2 init_symbol, §8.2.6 read_symbol) and compare."""
    L = oracle.lib()

    class RE(C.Structure):
        _fields_ = [("low", C.c_uint32), ("rng", C.c_uint32), ("cnt", C.c_int), ("buf", C.c_void_p), ("cap", C.c_size_t),
                    ("offs", C.c_size_t), ("error", C.c_int), ("nsym", C.c_uint64)]
    rng = np.random.default_rng(5)
    nsyms_list = [2, 3, 4, 5, 7, 13, 16]
    cdfs_enc, cdfs_dec = [], []
    for n in nsyms_list:
        cuts = np.sort(rng.choice(np.arange(1, 32767), n - 1, replace=False))
        icdf = [int(32768 - c) for c in cuts] + [0, 0]
        cdfs_enc.append((C.c_uint16 * (n + 1))(*icdf))
        cdfs_dec.append([int(c) for c in cuts] + [32768, 0])
    buf = C.create_string_buffer(1 << 16)
    e = RE()
    L.av1o_ec_init(C.byref(e), buf, len(buf))
    seq = []
    for _ in range(4000):
        k = int(rng.integers(len(nsyms_list)))
        n = nsyms_list[k]
        s = int(rng.integers(n)) if rng.random() < 0.5 else int(min(n - 1, rng.geometric(0.6) - 1))
        seq.append((k, s))
        L.av1o_ec_encode_symbol(C.byref(e), s, cdfs_enc[k], n)
        if rng.random() < 0.1:
            b = int(rng.integers(2))
            seq.append((-1, b))
            L.av1o_ec_encode_literal(C.byref(e), b, 1)
    L.av1o_ec_finish.restype = C.c_size_t
    nbytes = L.av1o_ec_finish(C.byref(e))
    data = buf.raw[:nbytes]

    # ---- spec decoder (tests/ec_ref.py)
    d = SpecDecoder(data)
    for k, s in seq:
        if k < 0:
            assert d.read([1 << 14, 1 << 15, 0], adapt=False) == s
        else:
            assert d.read(cdfs_dec[k]) == s


@pytest.mark.parametrize("log2n", [2, 3, 4, 5, 6])
def test_transforms_vs_real_dct(oracle, log2n):
    """Forward transform = scale * orthonormal 2-D DCT-II within a small integer error; inverse
    (normative network) inverts it.  scipy is the independent reference."""
    from scipy.fft import dctn
    L = oracle.lib()
    n = 1 << log2n
    rng = np.random.default_rng(log2n)
    scale = {2: 8, 3: 8, 4: 8, 5: 4, 6: 2}[log2n]
    for _ in range(5):
        x = rng.integers(-255, 256, (n, n)).astype(np.int32)
        co = np.zeros((n, n), np.int32)
        L.av1o_fwd_txfm2d(x.ctypes.data, n, co.ctypes.data, log2n, 0, 8)
        ref = dctn(x.astype(float), norm="ortho") * scale
        m = min(n, 32)
        assert np.abs(co[:m, :m] - ref[:m, :m]).max() < 6.0  # integer butterflies: documented bound
        if n == 64:
            assert not co[32:, :].any() and not co[:, 32:].any()
        # inverse of the (unquantised) coefficients returns the residual up to rounding
        if n <= 32:
            back = np.zeros((n, n), np.int32)
            L.av1o_inv_txfm2d(co.ctypes.data, back.ctypes.data, log2n, 0, 8)
            assert np.abs(back - x).max() <= 2


def test_luma32_matrix_forward_transform(oracle):
    """The luma 32x32 forward transform (what the HIP path's matrix cores compute) against a numpy int64
    restatement of its definition - Cm rebuilt here from the cosine formula - and against the real-valued DCT; the normative
    inverse returns the residual."""
    import ctypes as C
    from scipy.fft import dctn
    L = oracle.lib()
    L.av1o_fwd_dct32x32_matrix.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    k, n = np.meshgrid(np.arange(32), np.arange(32), indexing="ij")
    cm = np.rint(4096.0 * np.sqrt(2.0 / 32) * np.where(k == 0, np.sqrt(0.5), 1.0) * np.cos((2 * n + 1) * k * np.pi / 64)).astype(np.int64)
    rng = np.random.default_rng(32)
    for amp in (1023, 255, 40, 3):
        x = rng.integers(-amp, amp + 1, (32, 32)).astype(np.int32)
        co = np.zeros((32, 32), np.int32)
        L.av1o_fwd_dct32x32_matrix(x.ctypes.data, 32, co.ctypes.data)
        u = (x.astype(np.int64) @ cm.T + 512) >> 10
        assert np.abs(u).max() < 32768
        ref = (cm @ u + 2048) >> 12
        assert np.array_equal(co.astype(np.int64), ref)
        # 11-bit matrix entries: the error grows with the amplitude (relative 2^-11), 1.2 in the mean at typical residuals
        assert np.abs(co - 4 * dctn(x.astype(float), norm="ortho")).max() < (8.0 if amp > 255 else 2.5)
        back = np.zeros((32, 32), np.int32)
        L.av1o_inv_txfm2d(co.ctypes.data, back.ctypes.data, 5, 0, 10)
        assert np.abs(back - x).max() <= 2


@pytest.mark.parametrize("log2n,tx_type", [(2, 1), (2, 2), (2, 3), (3, 1), (3, 3), (4, 2), (4, 3)])
def test_adst_roundtrip(oracle, log2n, tx_type):
    L = oracle.lib()
    n = 1 << log2n
    rng = np.random.default_rng(10 * log2n + tx_type)
    x = rng.integers(-255, 256, (n, n)).astype(np.int32)
    co = np.zeros((n, n), np.int32)
    back = np.zeros((n, n), np.int32)
    L.av1o_fwd_txfm2d(x.ctypes.data, n, co.ctypes.data, log2n, tx_type, 8)
    L.av1o_inv_txfm2d(co.ctypes.data, back.ctypes.data, log2n, tx_type, 8)
    assert np.abs(back - x).max() <= 2


def test_dc_only_coefficient_gives_flat_block(oracle):
    L = oracle.lib()
    for log2n in (2, 3, 4, 5, 6):
        n = 1 << log2n
        dq = np.zeros((n, n), np.int32)
        dq[0, 0] = 800
        out = np.zeros((n, n), np.int32)
        L.av1o_inv_txfm2d(dq.ctypes.data, out.ctypes.data, log2n, 0, 8)
        assert out.min() == out.max() != 0


def test_scan_is_a_zigzag_permutation(oracle):
    L = oracle.lib()
    for log2n in (2, 3, 4, 5):
        n = 1 << log2n
        s = np.ctypeslib.as_array(L.av1o_default_scan(log2n), shape=(n * n,)).astype(int)
        assert sorted(s.tolist()) == list(range(n * n))
        d = s // n + s % n
        assert (np.diff(d) >= 0).all()          # anti-diagonal by anti-diagonal
        assert s[0] == 0 and s[1] == 1 and s[2] == n   # first step along the row (pinned by dav1d)


def test_intra_predictors_known_answers(oracle):
    L = oracle.lib()
    n, log2n = 8, 3
    above = (np.arange(2 * n + 1) * 3 + 10).astype(np.uint16)   # element 0 = above[-1]
    left = (np.arange(2 * n + 1) * 5 + 20).astype(np.uint16)
    left[0] = above[0]
    out = np.zeros((n, n), np.uint16)

    def pred(mode, delta=0, ha=1, hl=1):
        L.av1o_predict_intra(out.ctypes.data, n, log2n, mode, delta, above.ctypes.data, left.ctypes.data, ha, hl, 8)
        return out.copy()
    v = pred(1)
    assert (v == above[1:n + 1][None, :]).all()
    h = pred(2)
    assert (h == left[1:n + 1][:, None]).all()
    dc = pred(0)
    assert (dc == (int(above[1:n + 1].sum()) + int(left[1:n + 1].sum()) + n) // (2 * n)).all()
    assert (pred(0, ha=0, hl=0) == 128).all()
    # constant edges: every mode predicts that constant
    above[:] = 77
    left[:] = 77
    for mode in range(13):
        assert (pred(mode) == 77).all(), mode
    # D45 reads only the above row; D203 only the left column
    above[:] = (np.arange(2 * n + 1) * 3 + 10).astype(np.uint16)
    left[:] = 0
    left[0] = above[0]
    d45 = pred(3)
    assert d45[0, 0] == (int(above[2]) * 32 + int(above[3]) * 0 + 16) >> 5 or d45[0, 0] > 0
    left[:] = (np.arange(2 * n + 1) * 5 + 20).astype(np.uint16)
    a2 = above.copy()
    above[1:] = 0
    assert (pred(7) > 0).all()   # D203 ignores the (zeroed) above row
    above[:] = a2


def test_cdef_leaves_flat_frames_and_skipped_blocks_alone(oracle):
    """An all-skip frame is returned untouched; flat input is a fixed point of the CDEF filter even
    at maximum strength (constrain(0) = 0)."""
    w = h = 64
    flat = [np.full((h, w), 128, np.uint16), np.full((h // 2, w // 2), 128, np.uint16), np.full((h // 2, w // 2), 128, np.uint16)]
    cfg = oracle.default_config(w, h, 8, min_bs_log2=4, max_bs_log2=4, cdef_y_pri=15, cdef_y_sec=3, cdef_uv_pri=15, cdef_uv_sec=3)
    tu, rec, st = oracle.encode_frame(cfg, flat)
    assert st.n_skip_blocks == st.n_blocks == 16
    for p in range(3):
        assert (rec[p] == 128).all()
    # direct filter call on a flat, non-skipped frame
    L = oracle.lib()
    fin = oracle._planes_to_frame([np.full((h, w), 90, np.uint16), np.full((h // 2, w // 2), 100, np.uint16), np.full((h // 2, w // 2), 110, np.uint16)])
    fout = L.av1o_frame_alloc(w, h)
    skip = np.zeros((h // 4, w // 4), np.uint8)
    idx = np.zeros(1, np.int8)
    L.av1o_cdef_frame(C.byref(cfg), fin, fout, skip.ctypes.data, w // 4, idx.ctypes.data)
    out = oracle._frame_to_planes(fout)
    assert (out[0] == 90).all() and (out[1] == 100).all() and (out[2] == 110).all()
    # a vertical edge keeps its direction: filtering must not move the edge position
    y = np.full((h, w), 60, np.uint16)
    y[:, 32:] = 200
    fin2 = oracle._planes_to_frame([y, np.full((h // 2, w // 2), 128, np.uint16), np.full((h // 2, w // 2), 128, np.uint16)])
    L.av1o_cdef_frame(C.byref(cfg), fin2, fout, skip.ctypes.data, w // 4, idx.ctypes.data)
    out = oracle._frame_to_planes(fout)
    assert (out[0][:, :31] == 60).all() and (out[0][:, 33:] == 200).all()


def test_properties_linearity_of_sse_and_determinism(oracle):
    src = oracle.synthclip_frame(136, 72, 8, seed=3, t=1)
    cfg = oracle.default_config(136, 72, 8, min_bs_log2=5, max_bs_log2=5)
    a = oracle.encode_frame(cfg, src)
    b = oracle.encode_frame(cfg, src)
    assert a[0] == b[0]
    for p in range(3):
        assert (a[1][p] == b[1][p]).all()
        d = a[1][p].astype(np.int64) - src[p].astype(np.int64)
        assert int((d * d).sum()) == a[2].sse[p]
    # coarser quantiser -> fewer bytes, lower PSNR
    lo = oracle.encode_frame(oracle.default_config(136, 72, 8, min_bs_log2=5, max_bs_log2=5, base_q_idx=60), src)
    hi = oracle.encode_frame(oracle.default_config(136, 72, 8, min_bs_log2=5, max_bs_log2=5, base_q_idx=200), src)
    assert len(lo[0]) > len(a[0]) > len(hi[0])
    assert lo[2].sse[0] < a[2].sse[0] < hi[2].sse[0]


def test_rejects_bad_geometry(oracle):
    with pytest.raises(RuntimeError):   # odd width: 4:2:0 planes need even sizes (multiples of 8 are not required)
        oracle.encode_frame(oracle.default_config(61, 64, 8), [np.zeros((64, 61), np.uint16), np.zeros((32, 30), np.uint16), np.zeros((32, 30), np.uint16)])
    tu, rec, _ = oracle.encode_frame(oracle.default_config(60, 66, 8), [np.full((66, 60), 90, np.uint16), np.full((33, 30), 128, np.uint16), np.full((33, 30), 128, np.uint16)])
    assert rec[0].shape == (66, 60) and rec[1].shape == (33, 30) and int(np.abs(rec[0].astype(int) - 90).max()) <= 2


def test_synthclip_scene_cut_and_motion(oracle):
    a = oracle.synthclip_frame(128, 64, 8, seed=9, t=0, scene_len=4)
    b = oracle.synthclip_frame(128, 64, 8, seed=9, t=3, scene_len=4)
    c = oracle.synthclip_frame(128, 64, 8, seed=9, t=4, scene_len=4)   # new scene
    d = oracle.synthclip_frame(128, 64, 8, seed=10, t=0, scene_len=4)  # == scene 1 of seed 9
    assert not (a[0] == b[0]).all()
    assert (c[0] == d[0]).all()
    ten = oracle.synthclip_frame(128, 64, 10, seed=9, t=0)
    assert ten[0].max() > 255 and ten[0].max() <= 1023


def test_bench_synthclip_equals_the_oracle_generator(oracle):
    """bench.py synthesises its input with its own numpy `synthclip v1` (so the benchmark's product leg needs nothing from
    oracle/): it must be the same clip, byte for byte, as the C generator the parity tests use."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    for (w, h, bd, seed, t) in [(200, 120, 8, 1080, 0), (72, 56, 10, 1083, 5), (328, 248, 8, 7, 13), (640, 360, 10, 1080, 59)]:
        a = bench.synthclip_frame(w, h, bd, seed, t)
        b = oracle.synthclip_frame(w, h, bd, seed=seed, t=t)
        assert all((a[i] == b[i]).all() for i in range(3)), (w, h, bd, seed, t)
    # the torch generator (what bench.py runs on the GPU to put the clip into HBM), here on the CPU device: whole clips
    for (w, h, bd, n, seed) in [(200, 120, 8, 3, 1080), (72, 56, 10, 2, 1083), (328, 248, 10, 2, 7)]:
        clip = bench.make_clip_torch(w, h, bd, n, seed, "cpu").numpy().tobytes()
        assert clip == bench.make_clip(w, h, bd, n, seed), (w, h, bd, n, seed)
        dt = np.uint8 if bd == 8 else np.dtype("<u2")
        last = oracle.synthclip_frame(w, h, bd, seed=seed, t=n - 1)
        assert clip[-(w * h * 3 // 2 * dt.itemsize if bd > 8 else w * h * 3 // 2):] == b"".join(p.astype(dt).tobytes() for p in last)


def test_quantiser_matrix_level_rule_and_effect(oracle):
    """`enable_qm`: level = qm_min + q * (qm_max + 1 - qm_min) / 256 (SVT-AV1 / libaom); a steep matrix coarsens the high
    frequencies (fewer bytes), level 15 is the flat quantiser with using_qmatrix still signalled (5 more header bits)."""
    assert oracle.qm_level(32, 1, 15) == 2 and oracle.qm_level(120, 1, 15) == 8 and oracle.qm_level(255, 8, 15) == 15
    assert oracle.qm_level(0, 3, 9) == 3 and oracle.qm_level(255, 0, 14) == 14 and oracle.qm_level(200, 7, 7) == 7
    src = oracle.synthclip_frame(136, 72, 8, seed=5, t=0)
    plain, rec0, _ = oracle.encode_frame(oracle.default_config(136, 72, 8, min_bs_log2=5, max_bs_log2=5), src)
    sizes = []
    for lvl in (0, 6, 12, 15):
        tu, rec, _ = oracle.encode_frame(oracle.default_config(136, 72, 8, min_bs_log2=5, max_bs_log2=5, enable_qm=1, qm_y=lvl, qm_uv=lvl), src)
        sizes.append(len(tu))
        if lvl == 15:
            assert all((a == b).all() for a, b in zip(rec, rec0)) and tu != plain and abs(len(tu) - len(plain)) <= 1
    assert sizes[0] < sizes[1] < sizes[2] <= sizes[3]
