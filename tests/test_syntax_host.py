"""The host code that needs no GPU (av1-base_amd/csrc/av1mi_syntax.cpp: resolve() and its packed-field rules, the header writers, the
default CDF blob, dev_params) compiled by the plain host compiler - which is the check that the file needs no HIP - as a stand-alone
program (tests/host/syntax_host.cpp), once plain and once under AddressSanitizer and UndefinedBehaviorSanitizer.  It is fed the
defaults at four shapes and both bit depths and, for every packed or ranged field of av1mi_params, the lowest and highest accepted
value and the first refused one on each side.  What it must print does not come from the code under test: the return codes are a literal
table written from the field documentation of include/av1mi.h, the resolved fields are restated with the wrapper's field helpers, the
sequence header and the defaults' key and inter frame headers are the oracle's, and where the oracle does not write a syntax
(placeholders of the two searches, the fits' fields) the headers are held to properties."""
import ctypes as C
import os
import shutil

import pytest

import host_build
from test_aq_host import av1mi  # noqa: F401  (default_params and the field helpers, through the library's host-only path)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [os.path.join(ROOT, "tests", "host", "syntax_host.cpp"), os.path.join(ROOT, "av1-base_amd", "csrc", "av1mi_syntax.cpp")]
OK, INVALID, UNSUPPORTED = 0, 1, 7

# (width, height): the smallest frame, one padded both ways, the oracle comparisons' size, and 129 superblock columns
SHAPES = [((8, 8), OK), ((70, 58), OK), ((200, 120), OK), ((8256, 64), UNSUPPORTED)]

# field -> [(value or {field: value}, code)], at 200 x 120, 8 bit, every other field at its default: from include/av1mi.h
FIELDS = {
    # bits 0-7 1..63, 0 refused; bits 8-10 aq_strength 0..4; strengths 5..7 and any higher bit refused
    "cq_level": [(1, OK), (63, OK), (0, INVALID), (64, INVALID), (1 | 4 << 8, OK), (63 | 4 << 8, OK), (30 | 1 << 8, OK), (30 | 5 << 8, INVALID),
                 (30 | 7 << 8, INVALID), (30 | 1 << 11, INVALID), (30 | 1 << 31, INVALID), (0 | 1 << 8, INVALID), (64 | 1 << 8, INVALID)],
    "enable_lr": [
        (0, OK), (1, OK), (4, OK), (5, INVALID), (255, INVALID),                                      # the low byte
        (0x102, OK), (0x104, OK), (0x100, INVALID), (0x101, INVALID), (0x103, INVALID), (0x105, INVALID),   # bit 8: with 2 or 4
        (0x102 | 1 << 16, OK), (0x104 | 0xFFFF << 16, OK), (2 | 1 << 16, INVALID),                    # bits 16-31: the fit's sets
        (2 | 0x200, INVALID), (2 | 0x800, INVALID), (2 | 0x4000, INVALID), (2 | 0x8000, INVALID),     # bits 9, 11, 14, 15 alone
        (1 | 0x400, OK), (4 | 0x400, OK), (0x502, OK), (0x400, INVALID), (5 | 0x400, INVALID), (1 | 0x400 | 1 << 16, INVALID),   # bit 10
        (1 | 0x1000, OK), (4 | 0x2000, OK), (1 | 0x3000, INVALID), (0x1000, INVALID), (5 | 0x1000, INVALID),   # bits 12-13
        (1 | 0xC000, OK), (4 | 0xC000 | 0x200 | 0x800, OK), (0xC000, INVALID), (5 | 0xC000, INVALID),          # bits 14 and 15, scale in 9 and 11
        (0x104 | 0xFFFF << 16 | 0x400 | 0x2000 | 0xC000 | 0x200 | 0x800, OK), (0x101 | 0xC000, INVALID)],      # everything at once
    # bit 0 the pre-search, bits 8-10 frames 1..7, bits 12-14 strength 0..7; any other bit, or a strength without frames, refused
    "me_presearch": [(0, OK), (1, OK), (2, INVALID), (1 << 8, OK), (1 | 7 << 8 | 7 << 12, OK), (7 << 8, OK), (1 << 12, INVALID),
                     (1 | 7 << 12, INVALID), (1 << 11, INVALID), (1 << 15, INVALID), (1 << 16, INVALID), (1 << 8 | 1 << 31, INVALID)],
    "me_range": [(0, OK), (8, OK), (16, OK), (7, INVALID), (9, INVALID), (15, INVALID), (17, INVALID)],
    "block_log2": [(0, OK), (3, OK), (6, OK), (2, INVALID), (7, INVALID)],
    "min_block_log2": [(0, OK), (3, OK), (5, OK), (2, INVALID), (6, INVALID), ({"block_log2": 6, "min_block_log2": 6}, OK),
                       ({"block_log2": 3, "min_block_log2": 4}, INVALID)],
    "cdef_damping": [(3, OK), (6, OK), (2, INVALID), (7, INVALID), (0, OK)],
    "cdef_y_pri": [(0, OK), (15, OK), (16, INVALID)], "cdef_uv_pri": [(0, OK), (15, OK), (16, INVALID)],
    "cdef_y_sec": [(0, OK), (3, OK), (4, INVALID)], "cdef_uv_sec": [(0, OK), (3, OK), (4, INVALID)],
    "cdef_search": [(0, OK), (1, OK), (4, OK), (5, INVALID), ({"enable_cdef": 0, "cdef_search": 1}, INVALID), ({"enable_cdef": 0}, OK)],
    "deblock": [(0, OK), (1, OK), (2, OK), (3, INVALID)],
    "qm_min": [({"enable_qm": 1, "qm_min": 0}, OK), ({"enable_qm": 1, "qm_min": 15}, OK), ({"enable_qm": 1, "qm_min": 16}, INVALID),
               ({"enable_qm": 1, "qm_min": 9, "qm_max": 8}, INVALID), ({"enable_qm": 1, "qm_min": 8, "qm_max": 8}, OK)],
    "qm_max": [({"enable_qm": 1, "qm_min": 0, "qm_max": 0}, OK), ({"enable_qm": 1, "qm_max": 15}, OK), ({"enable_qm": 1, "qm_max": 16}, INVALID),
               ({"enable_qm": 2}, INVALID)],
    "tile_sb": [(0, OK), (1, OK), (2, OK), (3, INVALID)],
    # 0..255 each; sRGB + identity (1 / 13 / 0) implies 4:4:4 and is refused
    "colour": [({"color_primaries": 9, "transfer_characteristics": 16, "matrix_coefficients": 9}, OK),
               ({"color_primaries": 255, "transfer_characteristics": 255, "matrix_coefficients": 255}, OK),
               ({"color_primaries": 256}, INVALID), ({"transfer_characteristics": 256}, INVALID), ({"matrix_coefficients": 256}, INVALID),
               ({"color_primaries": 1, "transfer_characteristics": 13, "matrix_coefficients": 0}, INVALID),
               ({"color_primaries": 1, "transfer_characteristics": 13, "matrix_coefficients": 1}, OK)],
    "film_grain": [(0, OK), (1, OK), (50, OK), (51, INVALID)],
}


def _cases(av1mi):  # noqa: F811
    """[(name, Params, code)]"""
    out = []
    for (w, h), code in SHAPES:
        for bd in (8, 10):
            out.append(("%dx%d_%d" % (w, h, bd), av1mi.default_params(w, h, bd), code))
    for field, rows in FIELDS.items():
        for v, code in rows:
            kw = v if isinstance(v, dict) else {field: v}
            out.append(("%s:%s" % (field, ",".join("%s=%#x" % kv for kv in kw.items())), av1mi.default_params(200, 120, 8, **kw), code))
    out.append(("10bit_all", av1mi.default_params(200, 120, 10, cq_level=63 | 4 << 8, deblock=2, cdef_search=4, film_grain=50, enable_lr=4 | 0x1000), OK))
    return out


def _words(p):
    return list((C.c_uint32 * (C.sizeof(p) // 4)).from_buffer_copy(p))


@pytest.fixture(scope="module")
def cases(av1mi, tmp_path_factory):  # noqa: F811
    cs = _cases(av1mi)
    path = tmp_path_factory.mktemp("syntax") / "params.txt"
    path.write_text("".join(" ".join(str(v) for v in _words(p)) + "\n" for _, p, _ in cs))
    return cs, str(path)


def _parse(stdout, n):
    rows = [dict(t.split("=", 1) for t in line.split()) for line in stdout.splitlines()]
    assert len(rows) == n
    return rows


@pytest.fixture(scope="module")
def plain(cases, tmp_path_factory):
    """the plain build's output: built by the host compiler alone - g++ where there is one, so that no HIP-aware compiler is involved"""
    cxx = shutil.which("g++") or host_build.host_cxx(gcc=True)
    out = host_build.run_program(cxx, SOURCES, tmp_path_factory.mktemp("syntax_plain") / "syntax_host", args=[cases[1]])
    assert out.returncode == 0, out.stdout[-500:] + out.stderr[-2000:]
    return out.stdout


def test_sanitized_build_prints_what_the_plain_one_does(cases, plain, tmp_path):
    """... and runs clean under AddressSanitizer and UndefinedBehaviorSanitizer (a stand-alone program, host code only).  Skipped only
    where an empty program does not build and run under the sanitizers"""
    out = host_build.run_program(host_build.host_cxx(gcc=True), SOURCES, tmp_path / "syntax_host_san", args=[cases[1]], sanitized=True)
    assert out.returncode == 0, out.stdout[-500:] + out.stderr[-2000:]
    assert out.stdout == plain   # every field, header and checksum


def test_return_codes(cases, plain):
    rows = _parse(plain, len(cases[0]))
    bad = [(name, int(r["rc"]), code) for (name, _, code), r in zip(cases[0], rows) if int(r["rc"]) != code]
    assert not bad, bad


def _qindex(cq):
    """aom's quantizer_to_qindex: 4 per level, the last two steps 249 and 255 (av1mi.h: "mapped to base_q_idx like aom (30 -> 120)")"""
    return {62: 249, 63: 255}.get(cq, 4 * cq)


def test_resolved_fields(av1mi, oracle, cases, plain):  # noqa: F811
    for (name, p, code), r in zip(cases[0], _parse(plain, len(cases[0]))):
        if code:
            continue
        lr = p.enable_lr & 0xFF
        cw, ch = (p.width + 7) & ~7, (p.height + 7) & ~7
        sbc, sbr = (cw + 63) // 64, (ch + 63) // 64
        tsb = p.tile_sb or (2 if max(sbc, sbr) > 64 else 1)
        qidx = _qindex(av1mi.cq_level_of(p.cq_level))
        want = dict(cq=av1mi.cq_level_of(p.cq_level), aq=av1mi.aq_strength_of(p.cq_level), tf_frames=av1mi.tf_frames_of(p.me_presearch),
                    tf_strength=av1mi.tf_strength_of(p.me_presearch), presearch=av1mi.me_presearch_of(p.me_presearch),
                    lr=lr - 2 if lr >= 3 else lr, lr_chroma=int(lr >= 3), lr_unit_shift=av1mi.lr_unit_shift_of(p.enable_lr),
                    lr_rd=int(av1mi.lr_rd_scale_of(p.enable_lr) is not None),
                    lr_fit_mask=((p.enable_lr >> 16) or 0xFFFF) if p.enable_lr & 0x100 else 0, lr_wfit=int(bool(p.enable_lr & av1mi.LR_WIENER_FIT)),
                    qidx=qidx, cw=cw, ch=ch, padded=int((cw, ch) != (p.width, p.height)), sb="%dx%d" % (sbc, sbr), tile_sb=tsb,
                    tiles="%dx%d" % (-(-sbc // tsb), -(-sbr // tsb)), qm_level=oracle.qm_level(qidx, p.qm_min, p.qm_max) if p.enable_qm else 15,
                    keyint=p.keyint or 1, me_range=p.me_range or 8, block_log2=p.block_log2 or 5, min_block_log2=p.min_block_log2 or 3,
                    damping=p.cdef_damping or 5)
        got = {k: r[k] for k in want}
        assert got == {k: str(v) for k, v in want.items()}, name


def _oracle_cfg(oracle, p, **kw):
    lr = p.enable_lr & 0xFF
    return oracle.default_config(p.width, p.height, p.bit_depth, enable_cdef=p.enable_cdef, enable_lr=lr - 2 if lr >= 3 else lr, film_grain=p.film_grain,
                                 color_range=p.color_range, intra_edge_filter=p.intra_edge_filter, color_primaries=p.color_primaries,
                                 transfer_characteristics=p.transfer_characteristics, matrix_coefficients=p.matrix_coefficients, **kw)


def test_sequence_header_is_the_oracles(oracle, cases, plain):
    """every accepted case: what the oracle's configuration cannot express (packed fields, searches) is not in the sequence header"""
    n = 0
    for (name, p, code), r in zip(cases[0], _parse(plain, len(cases[0]))):
        if code:
            continue
        buf = C.create_string_buffer(64)
        k = oracle.lib().av1o_write_sequence_header(C.byref(_oracle_cfg(oracle, p)), buf, 64)
        assert buf.raw[:k].hex() == r["seq"], name
        n += 1
    assert n > 60


def _payload(tu, skip):
    """the OBU_FRAME payload of a temporal unit, `skip` bytes behind the temporal delimiter (test_abi_host.py: test_headers_match_oracle)"""
    off = 2 + skip + 1
    while tu[off] & 0x80:
        off += 1
    return tu[off + 1:]


def test_default_frame_headers_are_the_oracles(oracle, cases, plain):
    """the defaults up to 200 x 120, both bit depths: the key frame's header is the oracle's, and so is the inter frame's"""
    n = 0
    for (name, p, code), r in zip(cases[0], _parse(plain, len(cases[0]))):
        if ":" in name or name == "10bit_all" or code:
            continue
        cfg = _oracle_cfg(oracle, p, min_bs_log2=5, max_bs_log2=5)
        src = oracle.synthclip_frame(p.width, p.height, p.bit_depth, seed=1, t=0)
        tu, rec, _ = oracle.encode_frame(cfg, src)
        key = bytes.fromhex(r["key"])
        assert _payload(tu, len(r["seq"]) // 2)[:len(key)] == key, name
        tu2, _, _ = oracle.encode_frame(cfg, src, with_seq_hdr=False, ref=rec, prev_src=src)
        inter = bytes.fromhex(r["inter"])
        assert _payload(tu2, 0)[:len(inter)] == inter, name
        n += 1
    assert n == 6
    anchor = next(r for (name, _, _), r in zip(cases[0], _parse(plain, len(cases[0]))) if name == "70x58_8")
    assert (len(anchor["seq"]) // 2, anchor["key_bits"], len(anchor["key"]) // 2, anchor["cdf_words"], anchor["stream_cap"]) == (12, "61", 9, "5974", "8192")


def _bits(hexstr, n):
    data = bytes.fromhex(hexstr)
    return [(data[i >> 3] >> (7 - (i & 7))) & 1 for i in range(n)]


def _field(bits, at, n):
    return sum(b << (n - 1 - i) for i, b in enumerate(bits[at:at + n]))


def test_inter_header_differs_from_the_key_header_in_the_documented_fields(cases, plain):
    """Every accepted case.  frame_type 1 and error_resilient_mode 0; primary_ref_frame 7, refresh_frame_flags 1 and seven ref_frame_idx
    of 0 behind frame_size_override_flag; allow_high_precision_mv 0, is_filter_switchable 0, interpolation_filter BILINEAR (3: no
    sub-sample vectors in these cases) and is_motion_mode_switchable 0 behind render_and_frame_size_different; reference_select 0
    behind tx_mode_select and seven is_global 0 behind reduced_tx_set - 46 bits, one more (update_grain) with film grain.  Everything
    else is the key header's but the deblocking levels, which are 4 lower on key frames."""
    for (name, p, code), r in zip(cases[0], _parse(plain, len(cases[0]))):
        if code:
            continue
        kb, ib = int(r["key_bits"]), int(r["inter_bits"])
        assert ib == kb + 46 + (1 if p.film_grain else 0), name
        if p.film_grain:
            continue
        k, i = _bits(r["key"], kb), _bits(r["inter"], ib)
        want = k[0:1] + [0, 1] + k[3:4] + [0] + k[4:6] + [1, 1, 1] + [0] * 7 + [1] + [0] * 21 + k[6:7] + [0, 0, 1, 1, 0] + k[7:kb - 1] + [0] + k[kb - 1:] + [0] * 7
        assert k[1:3] == [0, 0] and len(want) == ib
        klf, ilf = int(r["key_lf_bit"]), int(r["inter_lf_bit"])
        assert ilf == klf + 38   # everything inserted in front of the levels
        if p.deblock:   # the four levels (luma never 0 here: all four are coded) are the frame kind's own
            for j in range(24):
                want[ilf + j] = i[ilf + j]
            assert all(_field(i, ilf + 6 * j, 6) >= _field(k, klf + 6 * j, 6) for j in range(4)), name
        assert i == want, name
        assert int(r["inter_cdef_bit"]) == int(r["key_cdef_bit"]) + 38 or not p.enable_cdef, name


def test_placeholder_offsets_point_at_the_placeholders(cases, plain):
    """cdef_str_bit: behind cdef_damping_minus_3 and cdef_bits, 2^cdef_bits times the fixed strengths (y_pri 4, y_sec 2, uv_pri 4, uv_sec 2
    bits).  lf_bit: loop_filter_level[0]; with the level search the luma fields carry max(g, 1) and the chroma fields g, where g is what
    the same parameters carry with deblock = 1 (g = 0 .. 63 from the quantiser; 0 only codes two fields)."""
    rows = {name: (p, r) for (name, p, code), r in zip(cases[0], _parse(plain, len(cases[0]))) if not code}
    n_cdef = n_lf = 0
    for name, (p, r) in rows.items():
        for kind in ("key", "inter"):
            b = _bits(r[kind], int(r[kind + "_bits"]))
            if p.enable_cdef:
                at = int(r[kind + "_cdef_bit"])
                cdef_bits = p.cdef_search - 1 if p.cdef_search else 0
                assert _field(b, at - 4, 2) == int(r["damping"]) - 3 and _field(b, at - 2, 2) == cdef_bits, name
                fixed = (2, 0, 1, 0) if not p.cdef_damping else (p.cdef_y_pri, p.cdef_y_sec, p.cdef_uv_pri, p.cdef_uv_sec)
                for s in range(1 << cdef_bits):
                    assert tuple(_field(b, at + 12 * s + o, n) for o, n in ((0, 4), (4, 2), (6, 4), (10, 2))) == fixed, name
                n_cdef += 1
            at = int(r[kind + "_lf_bit"])
            if not p.deblock:
                assert _field(b, at, 12) == 0, name   # two zero levels, then sharpness
            elif name == "deblock:deblock=0x2":
                g = _field(_bits(rows["deblock:deblock=0x1"][1][kind], at + 24), at, 6)
                assert 0 < g < 64
                assert [_field(b, at + 6 * j, 6) for j in range(4)] == [max(g, 1), max(g, 1), g, g], name
                n_lf += 1
    assert n_cdef > 100 and n_lf == 2


def test_checksums_tell_the_cases_apart(cases, plain):
    """(their stability is test_sanitized_build_prints_what_the_plain_one_does.)  The CDF blob depends on the q context alone - qidx up to
    20, 60, 120, above - and the kernels' parameters differ wherever the resolved parameters the kernels see do."""
    rows = {name: r for (name, _, code), r in zip(cases[0], _parse(plain, len(cases[0]))) if not code}
    qctx = lambda r: sum(int(r["qidx"]) > t for t in (20, 60, 120))   # noqa: E731
    by_ctx = {}
    for r in rows.values():
        by_ctx.setdefault(qctx(r), set()).add(r["cdf_sum"])
        assert r["cdf_words"] == "5974"
    assert sorted(by_ctx) == [0, 2, 3] and all(len(v) == 1 for v in by_ctx.values()) and len(set.union(*by_ctx.values())) == 3
    d = rows["200x120_8"]["dev_sum"]
    assert rows["tile_sb:tile_sb=0x0"]["dev_sum"] == d and rows["me_range:me_range=0x0"]["dev_sum"] == rows["me_range:me_range=0x8"]["dev_sum"] == d
    for other in ("200x120_10", "70x58_8", "8x8_8", "cq_level:cq_level=0x1", "cq_level:cq_level=0x3f", "me_range:me_range=0x10", "block_log2:block_log2=0x3",
                  "deblock:deblock=0x1", "deblock:deblock=0x2", "cdef_search:cdef_search=0x4", "enable_lr:enable_lr=0x1", "enable_lr:enable_lr=0x1001",
                  "enable_lr:enable_lr=0xc001", "tile_sb:tile_sb=0x2", "cdef_damping:cdef_damping=0x3"):
        assert rows[other]["dev_sum"] != d, other
    assert len({rows[k]["dev_sum"] for k in rows if k.startswith("enable_lr:")}) >= 8
