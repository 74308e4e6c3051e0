"""CPU tests of the film-grain synthesis (include/av1mi.h: av1mi_film_grain_synth, av1mi_grain_params): the
Gaussian table's hash; the restatement (tests/fgs_ref.py) against dav1d's output - the two grain fixtures of tests/golden and every
fixture of tests/golden/grain (tools/make_grain_golden.py), the oracle's reconstruction with the restatement's grain hashed against what
dav1d decoded; the rule header (av1-base_amd/csrc/fg_synth_rule.h) compiled for the host - a stand-alone program, run plain and under the
sanitizers - against the restatement; what the entry points refuse, the struct's size and the exported symbols."""
import ctypes as C
import hashlib
import json
import os
import re

import numpy as np
import pytest

import fgs_ref as F
import host_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAIN = os.path.join(ROOT, "tests", "golden", "grain")
SOURCES = [os.path.join(ROOT, "tests", "host", "fg_synth_rule_host.cpp")]


def sha(planes):
    h = hashlib.sha256()
    for p in planes:
        h.update(np.ascontiguousarray(np.asarray(p).astype("<u2")).tobytes())
    return h.hexdigest()


@pytest.fixture(scope="module")
def av1mi():
    return host_build.library()


# ---------------------------------------------------------------- the table and the restatement against dav1d
def test_gaussian_table_hash():
    t = F.gaussian_sequence()
    assert len(t) == 2048 and hashlib.sha256(t.astype("<i2").tobytes()).hexdigest() == F.TABLE_SHA256
    assert [int(v) for v in t[:4]] == [56, 568, -180, 172] and int(t.min()) == -1752 and int(t.max()) == 1688 and not (t % 4).any()


def _golden(oracle, name):
    m = json.load(open(os.path.join(ROOT, "tests", "golden", name + ".json")))
    src = oracle.synthclip_frame(m["width"], m["height"], m["bit_depth"], seed=m["seed"], t=m["t"])
    _, rec, _ = oracle.encode_frame(oracle.default_config(m["width"], m["height"], m["bit_depth"], **m["config"]), src)
    assert sha(rec) == m["recon_sha256"]
    ys, cs = m["config"]["fg_y_scaling"], m["config"]["fg_c_scaling"]
    g = F.params(point_y=[(0, ys), (255, ys)] if ys else [], point_cb=[(0, cs), (255, cs)] if cs else [], point_cr=[(0, cs), (255, cs)] if cs else [])
    return m, rec, F.synth(rec, m["bit_depth"], g, m["config"]["fg_seed"])


def test_restatement_reproduces_the_committed_dav1d_hash(oracle):
    m, rec, out = _golden(oracle, "k200x120_grain20_10b")
    assert m["dav1d_applies_grain"] and sha(out) == m["dav1d_sha256"] != m["recon_sha256"]


def test_restatement_copies_under_an_empty_table(oracle):
    m, rec, out = _golden(oracle, "k200x120_grain_tab0_10b")
    assert all(np.array_equal(a, b) for a, b in zip(out, rec)) and sha(out) == m["dav1d_sha256"] == m["recon_sha256"]


GRAIN_FIXTURES = json.load(open(os.path.join(GRAIN, "index.json")))


def test_grain_fixtures_cover_the_forms():
    metas = [json.load(open(os.path.join(GRAIN, n + ".json"))) for n in GRAIN_FIXTURES]
    sets = [F.unpack(bytes.fromhex(m["grain_params"])) for m in metas]
    assert {(m["width"], m["height"], m["bit_depth"]) for m in metas if not m["spliced"]} >= {(34, 34, 8), (34, 34, 10), (98, 66, 8), (98, 66, 10)}
    assert any(m["frames"] > 1 and not m["spliced"] for m in metas)                                   # an inter frame of the oracle's own
    assert any(len(g["point_y"]) == 8 for g in sets) and any(len(g["point_y"]) == 14 and len(g["point_cb"]) == 10 for g in sets)
    for lag in (1, 2, 3):
        assert any(g["ar_coeff_lag"] == lag and min(g["ar_coeffs_y"]) == -128 and max(g["ar_coeffs_y"]) == 127 for g in sets), lag
    assert {g["ar_coeff_shift_minus_6"] for g in sets} == {0, 1, 2, 3}
    assert any(g["ar_coeff_lag"] == 0 and g["ar_coeffs_cb"][0] for g in sets)                          # a luma tap alone
    assert any(g["chroma_scaling_from_luma"] for g in sets) and any(g["clip_to_restricted_range"] for g in sets)
    assert any(not g["overlap_flag"] for g in sets) and any(g["cb_mult"] != 128 for g in sets) and any(g["grain_scale_shift"] for g in sets)


@pytest.mark.parametrize("name", GRAIN_FIXTURES)
def test_restatement_equals_dav1d_on_the_grain_fixtures(oracle, name):
    """the oracle's stream up to film_grain_params (a spliced fixture carries the set's own string there: the committed stream parses to
    the set), its reconstruction, and the restatement's grain on it against dav1d's planes"""
    m = json.load(open(os.path.join(GRAIN, name + ".json")))
    w, h, bd = m["width"], m["height"], m["bit_depth"]
    g = F.unpack(bytes.fromhex(m["grain_params"]))
    obu = open(os.path.join(GRAIN, name + ".obu"), "rb").read()
    assert len(obu) == sum(m["frame_bytes"])
    ref, prev, pos = None, None, 0
    for t in range(m["frames"]):
        seed = m["grain_seeds"][t]
        cfg = oracle.default_config(w, h, bd, film_grain=1, fg_y_scaling=m["oracle_table"][0], fg_c_scaling=m["oracle_table"][1], fg_seed=seed)
        src = oracle.synthclip_frame(w, h, bd, seed=m["seed"], t=t)
        tu, rec, _ = oracle.encode_frame(cfg, src, with_seq_hdr=(t == 0), ref=ref, prev_src=prev)
        stored = obu[pos:pos + m["frame_bytes"][t]]
        pos += len(stored)
        if not m["spliced"]:
            assert stored == tu
        frame = [o for o in F.obus(stored) if o[0] == 6][0]
        carried, at, _ = F.find_params(stored[frame[2]:frame[3]], seed, t > 0)
        assert carried == dict(g, mc_identity=0)
        mine = [o for o in F.obus(tu) if o[0] == 6][0]
        assert F.to_bits(stored[frame[2]:frame[3]])[:at] == F.to_bits(tu[mine[2]:mine[3]])[:at]        # the header in front of it
        assert sha(rec) == m["recon_sha256"][t]
        assert sha(F.synth(rec, bd, g, seed)) == m["dav1d_sha256"][t] != m["recon_sha256"][t]
        ref, prev = rec, src


# ---------------------------------------------------------------- the rule header as a stand-alone program
def _bad_sets():
    sets = F.parameter_sets()
    full = F.pack(sets["full"])
    out = []
    for at, v in ((0, 15), (1, 11), (2, 11), (73, 4), (72, 4), (74, 4), (75, 4)):   # too many points; lag, scaling and shifts above 3
        b = bytearray(full)
        b[at] = v
        out.append(bytes(b))
    b = bytearray(full)
    b[4 + 2 * 5] = b[4 + 2 * 4]            # two luma points at one x
    out.append(bytes(b))
    b = bytearray(full)
    b[32 + 2 * 3] = 0                      # a cb point out of order
    out.append(bytes(b))
    for at in (156, 158):                  # cb_offset, cr_offset = 512
        b = bytearray(full)
        b[at:at + 2] = (512).to_bytes(2, "little")
        out.append(bytes(b))
    return out


def _header_cases():
    rng = np.random.default_rng(4)
    out = []
    for n in (1, 20, 50, 200):
        out.append((n, 0, 0, np.zeros(24, dtype=np.uint8), np.zeros(75, dtype=np.int8)))
    for lag in (0, 1, 2, 3):
        out.append((50, 1, lag, rng.integers(0, 256, 24).astype(np.uint8), rng.integers(-128, 128, 75).astype(np.int8)))
    return out


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """(the case lines, the lines the plain program prints for them, the path of the case file)"""
    lines = ["G"]
    for name, bd, w, h, g, seeds, raw in F.cases():
        fb = len(raw) // len(seeds)
        for f, s in enumerate(seeds):
            lines.append("F %d %d %d %d %s %s" % (bd, w, h, s, F.pack(g).hex(), raw[f * fb:(f + 1) * fb].hex()))
    for name, g in sorted(F.parameter_sets().items()):
        lines.append("T 10 %d %s" % (0xBEEF, F.pack(g).hex()))
        lines.append("V %s" % F.pack(g).hex())
    for b in _bad_sets():
        lines.append("V %s" % b.hex())
    for n, est, lag, table, coeffs in _header_cases():
        lines.append("H %d %d %d %s %s" % (n, est, lag, table.tobytes().hex(), coeffs.tobytes().hex()))
    d = tmp_path_factory.mktemp("fg_synth_rule")
    path = d / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    out = host_build.run_program(host_build.host_cxx(gcc=True), SOURCES, d / "fg_synth_rule_host", args=[path])
    assert out.returncode == 0, out.stderr[-2000:]
    got = out.stdout.split("\n")[:-1]
    assert len(got) == len(lines)
    return lines, got, path


def test_rule_table_is_the_spec_table(program):
    lines, got, _ = program
    assert lines[0] == "G" and hashlib.sha256(bytes.fromhex(got[0])).hexdigest() == F.TABLE_SHA256


def test_rule_frames_equal_the_restatement(program):
    lines, got, _ = program
    outs = [g for ln, g in zip(lines, got) if ln[0] == "F"]
    i, changed = 0, 0
    for name, bd, w, h, g, seeds, raw in F.cases():
        want = F.synth_frames(raw, w, h, bd, g, seeds)
        fb = len(want) // len(seeds)
        for f in range(len(seeds)):
            assert outs[i] == want[f * fb:(f + 1) * fb].hex(), (name, f)
            i += 1
        changed += want != raw
        assert (want == raw) == name.startswith("zero/"), name      # every set but the empty one changes its frames
    assert i == len(outs) and changed > 40


def test_rule_templates_equal_the_restatement(program):
    lines, got, _ = program
    outs = [g for ln, g in zip(lines, got) if ln[0] == "T"]
    sets = sorted(F.parameter_sets().items())
    assert len(outs) == len(sets)
    clamped = 0
    for (name, g), o in zip(sets, outs):
        t = np.concatenate([p.ravel() for p in F.templates(g, 10, 0xBEEF)])
        assert [int(v) for v in o.split()] == t.tolist(), name
        clamped += int((t == -512).any() and (t == 511).any())
    assert clamped >= 3                                              # the extreme coefficients drive the filter into GrainMin and GrainMax


def test_rule_refuses_what_the_entry_point_refuses(program):
    lines, got, _ = program
    outs = [int(g) for ln, g in zip(lines, got) if ln[0] == "V"]
    n_good = len(F.parameter_sets())
    assert outs == [1] * n_good + [0] * len(_bad_sets())


def test_rule_header_params(program):
    lines, got, _ = program
    outs = [g for ln, g in zip(lines, got) if ln[0] == "H"]
    cases = _header_cases()
    assert len(outs) == len(cases)
    for (n, est, lag, table, coeffs), o in zip(cases, outs):
        assert bytes.fromhex(o) == F.pack(F.header_params(n, est, lag, table, coeffs)), (n, est, lag)


def test_standalone_program_under_sanitizers(program, tmp_path):
    """the same cases once under AddressSanitizer and UndefinedBehaviorSanitizer (host code only, a program of its own).  Skipped only where
    an empty program does not build and run under the sanitizers - their runtimes are not installed"""
    lines, got, path = program
    out = host_build.run_program(host_build.host_cxx(gcc=True), SOURCES, tmp_path / "fg_synth_rule_host_san", args=[path], sanitized=True)
    assert out.returncode == 0, out.stdout[-500:] + out.stderr[-2000:]
    assert out.stdout.split("\n")[:-1] == got


def test_bit_string_round_trip():
    for name, g in F.parameter_sets().items():
        if name == "chroma_only":                                     # chroma points without luma points: no 4:2:0 stream carries them
            with pytest.raises(AssertionError):
                F.params_bits(g, 1, 0)
            continue
        for inter in (0, 1):
            bits = [0] * 11 + F.params_bits(g, 0xA5A5, inter) + [0] * 5
            got, seed, behind = F.parse_params(bits, 11, inter)
            assert (got, seed, behind) == (dict(g, mc_identity=0), 0xA5A5, len(bits) - 5), name


# ---------------------------------------------------------------- the ABI
def test_struct_size_and_symbols(av1mi):
    assert C.sizeof(av1mi.GrainParams) == int(av1mi._lib.av1mi_grain_params_size()) == F.PARAMS_SIZE == 164
    assert C.sizeof(av1mi.Params) == 36 * 4 and av1mi.struct_sizes() == av1mi.mirror_sizes() and av1mi.ABI_VERSION == int(av1mi._lib.av1mi_abi_version()) == 8
    g = av1mi.GrainParams.from_buffer_copy(F.pack(F.parameter_sets()["full"]))
    assert (g.num_y_points, g.num_cb_points, g.point_cb[0][0], g.cb_offset, g.grain_scaling_minus_8) == (14, 10, 3, 256, 0)
    assert F.unpack(bytes(g)) == F.parameter_sets()["full"]
    hdr = open(os.path.join(ROOT, "include", "av1mi.h")).read()
    shim = open(os.path.join(ROOT, "integration", "mi355x.rs")).read()
    for sym in ("av1mi_film_grain_synth", "av1mi_film_grain_params_result", "av1mi_ctx_set_displayed_quality", "av1mi_displayed_quality_result",
                "av1mi_grain_params_size"):
        assert sym in av1mi.ABI_SYMBOLS
        assert getattr(av1mi._lib, sym) is not None   # exported
        assert re.search(r"\b(int|uint32_t)\s+%s\s*\(" % sym, hdr), sym
        assert "fn %s(" % sym in shim, sym
    assert "#define AV1MI_ABI_VERSION 8" in hdr and "} av1mi_grain_params;" in hdr and "struct Av1miGrainParams" in shim


def test_entry_points_check_their_arguments_first(av1mi):
    """AV1MI_E_INVALID_ARG before anything touches a device: no context; and (the checks stand in front of the context's use) null
    frames, out == frames, no frames"""
    lib = av1mi._lib
    p = av1mi.default_params(64, 64, 8)
    g = av1mi.GrainParams.from_buffer_copy(F.pack(F.fixed_params(20)))
    buf = (C.c_uint8 * (64 * 64 * 3 // 2 * 2))()
    a, b = C.cast(buf, C.c_void_p), C.c_void_p(C.addressof(buf) + 64 * 64 * 3 // 2)
    assert lib.av1mi_film_grain_synth(None, C.byref(p), a, 1, 0, C.byref(g), None, b) == 1
    fake = C.c_void_p(1)   # never dereferenced: every call below is refused by its other arguments
    assert lib.av1mi_film_grain_synth(fake, None, a, 1, 0, C.byref(g), None, b) == 1
    assert lib.av1mi_film_grain_synth(fake, C.byref(p), None, 1, 0, C.byref(g), None, b) == 1
    assert lib.av1mi_film_grain_synth(fake, C.byref(p), a, 1, 0, None, None, b) == 1
    assert lib.av1mi_film_grain_synth(fake, C.byref(p), a, 1, 0, C.byref(g), None, None) == 1
    assert lib.av1mi_film_grain_synth(fake, C.byref(p), a, 1, 0, C.byref(g), None, a) == 1          # out == frames
    assert lib.av1mi_film_grain_synth(fake, C.byref(p), a, 0, 0, C.byref(g), None, b) == 1
    assert lib.av1mi_film_grain_params_result(None, C.byref(g)) == 1
    assert lib.av1mi_ctx_set_displayed_quality(None, 1) == 1
    assert lib.av1mi_displayed_quality_result(None, 1, None) == 1
