"""CPU tests of the film-grain estimate's interface (include/av1mi.h: av1mi_params.film_grain bit 8, av1mi_film_grain_estimate,
av1mi_film_grain_result): how the field packs and what is refused, the frame header of both frame kinds against the fixed mode's and
against tests/fg_ref.py's bit string, the ABI staying what it was, and the rule header (av1-base_amd/csrc/fg_rule.h) compiled for the host
- a stand-alone program, run plain and under the sanitizers - against the restatement on synthetic inputs no clip reaches, and its block
walk, which the estimate's and the fit's kernels place their lanes by, against a plain enumeration."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fg_ref
import host_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [os.path.join(ROOT, "tests", "host", "fg_rule_host.cpp"), os.path.join(ROOT, "av1-base_amd", "csrc", "av1mi_syntax.cpp")]


@pytest.fixture(scope="module")
def av1mi():
    return host_build.library()


# ---------------------------------------------------------------- packing
@pytest.mark.parametrize("n", [1, 20, 50])
def test_packed_field_accepted(av1mi, n):
    p = av1mi.default_params(640, 360, 8, film_grain_estimate=n)
    assert p.film_grain == n | 0x100 == av1mi.film_grain_estimate(n) == fg_ref.field(n)
    assert av1mi.film_grain_estimated(p.film_grain) == 1 and av1mi.film_grain_level_of(p.film_grain) == n
    assert fg_ref.field_decode(p.film_grain) == (True, n, True)
    av1mi.write_headers(p)
    av1mi.write_headers(av1mi.default_params(640, 360, 8, film_grain=n | 0x100))   # the raw field
    assert av1mi.default_params(640, 360, 8, film_grain=n, film_grain_estimate=True).film_grain == n | 0x100
    assert av1mi.default_params(640, 360, 8, film_grain=n, film_grain_estimate=False).film_grain == n
    assert av1mi.default_params(640, 360, 8).film_grain == 0   # the default stays off


@pytest.mark.parametrize("v", [0x100, 0x100 | 51, 0x100 | 255, 0x200 | 20, 0x300 | 20, 0x200, 1 << 16 | 0x100 | 20, 1 << 31 | 0x100 | 20, 1 << 31 | 20, 51, 255])
def test_packed_field_refused(av1mi, v):
    assert not fg_ref.field_decode(v)[0]
    with pytest.raises(av1mi.EncodeFailed) as e:
        av1mi.write_headers(av1mi.default_params(640, 360, 8, film_grain=v))
    assert e.value.code == 1   # AV1MI_E_INVALID_ARG


def test_abi_unchanged_and_symbols_exported(av1mi):
    assert C.sizeof(av1mi.Params) == 36 * 4 and av1mi.struct_sizes() == av1mi.mirror_sizes()
    assert av1mi.ABI_VERSION == int(av1mi._lib.av1mi_abi_version()) == 8
    hdr = open(os.path.join(ROOT, "include", "av1mi.h")).read()
    shim = open(os.path.join(ROOT, "integration", "mi355x.rs")).read()
    for sym in ("av1mi_film_grain_estimate", "av1mi_film_grain_result"):
        assert sym in av1mi.ABI_SYMBOLS
        assert getattr(av1mi._lib, sym) is not None   # exported
        assert re.search(r"\bint\s+%s\s*\(" % sym, hdr), sym
        assert "fn %s(" % sym in shim, sym
    assert re.search(r"#define\s+AV1MI_FILM_GRAIN_ESTIMATE\(", hdr) and "#define AV1MI_ABI_VERSION 8" in hdr
    assert "fn film_grain_estimate(" in shim and "36 * 4" in shim
    assert av1mi.FILM_GRAIN_MAX == fg_ref.MAX_N == 50


def test_entry_points_check_their_arguments_first(av1mi):
    """no context: AV1MI_E_INVALID_ARG before anything touches a device"""
    p = av1mi.default_params(64, 64, 8, film_grain_estimate=20)
    assert av1mi._lib.av1mi_film_grain_estimate(None, C.byref(p), None, 1, 0, None, None, None) == 1
    assert av1mi._lib.av1mi_film_grain_result(None, None) == 1


# ---------------------------------------------------------------- the stand-alone program: headers of both kinds and the rule
MIXES = [{}, dict(deblock=2, enable_lr=2, enable_qm=1, cdef_search=3, first_frame=7), dict(width=202, height=122, bit_depth=8, cdf_update=0, cq_level=30 | 2 << 8)]


def _words(p):
    return " ".join(str(v) for v in np.frombuffer(bytes(p), dtype=np.uint32))


def _block_cases():
    rng = np.random.default_rng(3)
    out = []
    for bd in (8, 10):
        mx = (1 << bd) - 1
        for n in (16, 8):
            checker = (np.add.outer(np.arange(n), np.arange(n)) & 1) * mx                 # Nsum at the format's maximum
            ramp = np.add.outer(np.arange(n) * 3, np.arange(n) * 5) + 7                    # a plane: the operator is blind to it
            blocks = [checker, mx - checker, ramp, np.full((n, n), mx), np.zeros((n, n), dtype=np.int64)]
            blocks += [np.clip(np.rint(rng.normal(lv << (bd - 8), s * (1 << (bd - 8)), (n, n))), 0, mx).astype(np.int64)
                       for lv in (16, 100, 240) for s in (0.5, 1.25, 4.0, 30.0)]
            blocks += [rng.integers(0, mx + 1, (n, n)) for _ in range(3)]
            out += [(bd, n, b) for b in blocks]
    return out


def _record(b, vy, vu, vv):
    return b | vy << 8 | vu << 16 | vv << 24


def _table_cases():
    """(ceil_y, ceil_c, records): counts of 15 and 16, fill ties, all bins empty, clamps, one bin only"""
    rng = np.random.default_rng(8)

    def bin_blocks(b, n, lo, hi):
        return [_record(b, int(rng.integers(lo, hi)), int(rng.integers(lo, hi)), int(rng.integers(lo, hi))) for _ in range(n)]
    return [
        (100, 50, []),                                                                     # no block at all
        (100, 50, bin_blocks(2, 15, 10, 40) + bin_blocks(6, 15, 10, 40)),                  # 15 and 15: no bin populated, all 0
        (100, 50, bin_blocks(2, 16, 10, 40) + bin_blocks(6, 15, 60, 90)),                  # 16 and 15: bin 2 fills every bin
        (255, 255, bin_blocks(1, 16, 10, 40) + bin_blocks(5, 16, 60, 90)),                 # bin 3 is two away from both: the lower index wins
        (255, 255, bin_blocks(0, 40, 5, 9) + bin_blocks(7, 40, 200, 256)),                 # bins 3 | 4: the nearer end each
        (100, 50, bin_blocks(0, 40, 120, 256) + bin_blocks(4, 17, 0, 3) + bin_blocks(7, 100, 30, 70)),   # clamps at both ceilings
        (2, 1, bin_blocks(3, 64, 0, 256)),                                                 # film_grain = 1
        (100, 50, [_record(b, 16 * b, 8 * b, 4 * b) for b in range(8) for _ in range(16)]),   # every bin populated, its own value
        (100, 50, [_record(4, v, 255 - v, v // 2) for v in range(256)]),
    ]


# (blocks per row, block rows, frames, workgroups): one block; no block; an odd count of blocks per row on one workgroup and on two; more
# workgroups than steps; the GPU tests' multi-step clips - 1044 steps on the fit's 1024 workgroups, 4176 on the estimate's 4096
WALKS = [(1, 1, 1, 1), (0, 3, 2, 1), (3, 2, 2, 1), (3, 2, 2, 2), (5, 1, 3, 4), (4, 3, 5, 3), (35, 58, 4, 1024), (35, 58, 16, 4096)]


def _walk_plain(nbx, nby, nf, grid):
    """what the program prints for a W line, from a plain enumeration: the pairs in frame, row, column order, four a step, the steps dealt
    round the workgroups; slot 2 k + side of a step holds side `side` of its k-th pair"""
    pairs = [(f, by, px) for f in range(nf) for by in range(nby) for px in range((nbx + 1) // 2)]
    steps = (len(pairs) + 3) // 4
    order = both = 0
    for gp, (f, by, px) in enumerate(pairs):
        for side in (0, 1):
            if 2 * px + side < nbx:
                order += 16 * ((gp // 4) * 8 + (gp % 4) * 2 + side + 1) * ((f * nby + by) * nbx + 2 * px + side + 1)   # 16 rows
        both += 16 * (2 * px + 1 < nbx)   # 2 planes of 8 rows
    wg_sum = sum((g + 1) * len(range(g, steps, grid)) for g in range(grid))
    blocks = nf * nby * nbx
    return [steps, 16 * blocks, 16 * blocks, 16 * len(pairs), 16 * len(pairs), both, 0, 0, wg_sum, order % (1 << 64)]


@pytest.fixture(scope="module")
def program(av1mi, tmp_path_factory):
    """(the case lines, the lines the plain program prints for them, the path of the case file)"""
    lines = []
    for bd, n, b in _block_cases():
        lines.append("B %d %d %s" % (bd, n, " ".join(str(int(v)) for v in b.ravel())))
    rng = np.random.default_rng(12)
    for n in list(range(1, 10)) + [15, 16, 17, 64]:
        for _ in range(3):
            lines.append("Q %d %s" % (n, " ".join(str(int(v)) for v in rng.integers(0, 256 if n > 4 else 4, n))))
    for cy, cc, recs in _table_cases():
        lines.append("T %d %d %d %s" % (cy, cc, len(recs), " ".join("%x" % r for r in recs)))
    lines += ["W %d %d %d %d" % w for w in WALKS]
    for kw in MIXES:
        kw = dict(kw)
        geom = (kw.pop("width", 1920), kw.pop("height", 1080), kw.pop("bit_depth", 10))
        for n in (1, 20, 50):
            for fg in (n, n | 0x100):
                for frame, inter in ((0, 0), (3, 1), (5, 0)):
                    lines.append("H %s %d %d" % (_words(av1mi.default_params(*geom, film_grain=fg, keyint=240, **kw)), frame, inter))
    lines.append("H %s 0 0" % _words(av1mi.default_params(64, 64, 8, film_grain=0x100)))   # refused
    d = tmp_path_factory.mktemp("fg_rule")
    path = d / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    out = host_build.run_program(host_build.host_cxx(gcc=True), SOURCES, d / "fg_rule_host", args=[path])
    assert out.returncode == 0, out.stderr[-2000:]
    got = out.stdout.split("\n")[:-1]
    assert len(got) == len(lines)
    return lines, got, path


def test_rule_blocks_equal_the_restatement(program):
    lines, got, _ = program
    outs = [g for ln, g in zip(lines, got) if ln[0] == "B"]
    seen = set()
    for (bd, n, b), g in zip(_block_cases(), outs):
        nsum = int(fg_ref.nsum_blocks(b, n, 1, 1)[0, 0])
        want = (nsum, int(fg_ref.value_of(nsum, n == 8, bd)), int(fg_ref.bin_of(b.sum(), bd)) if n == 16 else -1)
        assert tuple(int(v) for v in g.split()) == want, (bd, n)
        seen.add(want[1])
    # the 10-bit checkerboard: the product that needs 64 bits, and the operator's blindness to a plane
    mx = 1023
    assert int(fg_ref.nsum_blocks((np.add.outer(np.arange(16), np.arange(16)) & 1) * mx, 16, 1, 1)[0, 0]) == 196 * 8 * mx   # (centre and corners at the maximum, the four edges at 0: 8 of the 16 in sum |M|)
    assert 196 * 8 * mx * fg_ref.K_LUMA > 1 << 32
    assert int(fg_ref.nsum_blocks(np.add.outer(np.arange(16) * 3, np.arange(16) * 5), 16, 1, 1)[0, 0]) == 0
    assert {0, 255} <= seen and len(seen) > 8


def test_rule_quartile_ranks(program):
    lines, got, _ = program
    for ln, g in zip(lines, got):
        if ln[0] == "Q":
            vals = [int(v) for v in ln.split()[2:]]
            assert int(g) == fg_ref.quartile(vals), vals
    # the rank is (n + 3) // 4, counted from 1: n = 1 .. 4 the smallest, 5 .. 8 the second smallest, 9 the third
    assert [fg_ref.quartile(list(range(10, 10 + n))) - 10 for n in range(1, 10)] == [0, 0, 0, 0, 1, 1, 1, 1, 2]


def test_rule_table_equals_the_restatement(program):
    lines, got, _ = program
    outs = [g for ln, g in zip(lines, got) if ln[0] == "T"]
    cases = _table_cases()
    assert len(outs) == len(cases)
    for i, ((cy, cc, recs), g) in enumerate(zip(cases, outs)):
        blocks = np.array([[r & 0xFF, r >> 8 & 0xFF, r >> 16 & 0xFF, r >> 24 & 0xFF] for r in recs], dtype=np.uint8).reshape(-1, 4)
        table, counts = fg_ref.table_of(blocks, cy, cc)
        v = [int(x) for x in g.split()]
        assert v[:24] == [int(x) for x in table.ravel()], i
        assert v[24:] == [int(x) for x in counts.ravel()], i
    t = lambda i: fg_ref.table_of(np.array([[r & 0xFF, r >> 8 & 0xFF, r >> 16 & 0xFF, r >> 24 & 0xFF] for r in cases[i][2]], dtype=np.uint8).reshape(-1, 4), *cases[i][:2])
    assert not t(0)[0].any() and not t(1)[0].any() and t(1)[1][0, 2] == 15
    assert len(set(t(2)[0][0])) == 1 and t(2)[0][0, 0] > 0                       # the one populated bin fills the plane
    assert t(3)[0][0, 3] == t(3)[0][0, 1] != t(3)[0][0, 5]                        # the tie goes to the lower index
    assert list(t(4)[0][0]) == [t(4)[0][0, 0]] * 4 + [t(4)[0][0, 7]] * 4
    assert t(5)[0][0].max() <= 100 and t(5)[0][1:].max() <= 50 and t(5)[0][0, 0] == 100 and t(5)[0][1, 0] == 50
    assert t(6)[0][0].max() <= 2 and t(6)[0][1:].max() <= 1
    assert [int(x) for x in t(7)[0][0]] == [min(16 * b, 100) for b in range(8)]


def test_walk_takes_every_block_once(program):
    """fg_rule.h's block walk, every lane of every workgroup over its steps: every block of every frame by exactly 16 luma lanes with the
    rows 0 .. 15, every pair by exactly 8 lanes per chroma plane with the rows 0 .. 7, the right block flagged exactly when it exists,
    nothing outside the picture, every lane of a workgroup as many steps as its index gives it, and the slots in the enumeration's order"""
    lines, got, _ = program
    outs = [[int(v) for v in g.split()] for ln, g in zip(lines, got) if ln[0] == "W"]
    assert len(outs) == len(WALKS)
    for w, g in zip(WALKS, outs):
        assert g == _walk_plain(*w), w
    steps = {w: g[0] for w, g in zip(WALKS, outs)}
    assert steps[(0, 3, 2, 1)] == 0 and steps[(35, 58, 4, 1024)] == 1044 and steps[(35, 58, 16, 4096)] == 4176   # more steps than workgroups


def test_standalone_program_under_sanitizers(program, tmp_path):
    """the same cases once under AddressSanitizer and UndefinedBehaviorSanitizer (host code only, a program of its own).  Skipped only where
    an empty program does not build and run under the sanitizers - their runtimes are not installed"""
    lines, got, path = program
    out = host_build.run_program(host_build.host_cxx(gcc=True), SOURCES, tmp_path / "fg_rule_host_san", args=[path], sanitized=True)
    assert out.returncode == 0, out.stdout[-500:] + out.stderr[-2000:]
    assert out.stdout.split("\n")[:-1] == got


def test_frame_headers_of_both_kinds(av1mi, program):
    """the estimate's header equals the fixed mode's up to num_y_points, is 288 bits longer, and its tail is the restatement's string with
    the ceiling's values - key and inter frames, whatever else the header carries; av1mi_write_headers returns the key frame's"""
    lines, got, _ = program
    hs = [(ln.split(), g.split()) for ln, g in zip(lines, got) if ln[0] == "H"]
    assert hs[-1][1] == ["1"]   # bit 8 without a level: refused
    hs = hs[:-1]
    assert len(hs) == len(MIXES) * 3 * 2 * 3
    by_key = {}
    for ln, g in hs:
        words, frame, inter = [int(v) for v in ln[1:37]], int(ln[37]), int(ln[38])
        assert g[0] == "0"
        by_key[(tuple(w for i, w in enumerate(words) if i != 14), words[14], frame, inter)] = (int(g[1]), int(g[2]), bytes.fromhex(g[3]), words)
    assert len(by_key) == len(hs)
    for (rest, fg, frame, inter), (bits, fg_bit, data, words) in by_key.items():
        if not fg & 0x100:
            assert fg_bit == 0
            continue
        n = fg & 0xFF
        fbits, _, fdata, _ = by_key[(rest, n, frame, inter)]
        seed = fg_ref.grain_seed(words[15], frame)   # first_frame
        est, fix = fg_ref.header_bits(data, bits), fg_ref.header_bits(fdata, fbits)
        tail = fg_ref.params_bits([[c] * 8 for c in (min(2 * n, 255), n, n)], seed, inter)
        ftail = fg_ref.fixed_bits(n, seed, inter)
        assert bits == fbits + 288 and len(tail) == len(ftail) + 288
        head = fbits - len(ftail)
        assert est[:head] == fix[:head] and fix[head:] == ftail and est[head:] == tail
        assert est[:head + 17 + inter] == fix[:head + 17 + inter]     # ... up to num_y_points
        assert fg_bit == head + 17 + inter + 4                        # the first luma point
        if frame == 0 and not inter:
            p = av1mi.Params.from_buffer_copy(np.array(words, dtype=np.uint32).tobytes())
            _, fh, hbits = av1mi.write_headers(p)
            assert hbits == bits and fh == data[:(bits + 7) // 8]
