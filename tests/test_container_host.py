"""The file formats of av1mi_encode_file (av1-base_amd/csrc/av1mi_container.cpp: the Y4M reader, the IVF / Matroska / OBU writers and
av1mi_probe_y4m) compiled by the plain host compiler - which is the check that the file needs no HIP - as a stand-alone program
(tests/host/container_host.cpp), once plain and once under AddressSanitizer and UndefinedBehaviorSanitizer.  What it must print and write
does not come from the code under test: the clip fields are the literals of the headers written here, the frames are the bytes written
here, and the container files are mkv_ref.py's restatements of the formats."""
import os
import shutil

import pytest

import host_build
import mkv_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [os.path.join(ROOT, "tests", "host", "container_host.cpp"), os.path.join(ROOT, "av1-base_amd", "csrc", "av1mi_container.cpp")]
E_FORMAT = 6


def _frames(w, h, bd, n, seed):
    size = w * h * 3 // 2 * (2 if bd > 8 else 1)
    return [bytes((seed + 31 * t + 7 * i) & 0xFF for i in range(size)) for t in range(n)]


def _clip(header, frames, marker=b"FRAME\n"):
    return header + b"\n" + b"".join(marker + f for f in frames)


# name -> (header, width, height, bit depth, what av1mi_probe_y4m must say: None = AV1MI_E_FORMAT, else (bd, fps_n, fps_d, colour range))
HEADERS = {
    "jpeg": (b"YUV4MPEG2 W16 H8 F25:1 Ip A1:1 C420jpeg", 16, 8, 8, (8, 25, 1, 0)),
    "mpeg2": (b"YUV4MPEG2 W16 H8 F25:1 Ip A1:1 C420mpeg2", 16, 8, 8, (8, 25, 1, 0)),
    "paldv": (b"YUV4MPEG2 W16 H8 F30000:1001 Ip A1:1 C420paldv", 16, 8, 8, (8, 30000, 1001, 0)),
    "bare420": (b"YUV4MPEG2 W16 H8 F24:1 C420", 16, 8, 8, (8, 24, 1, 0)),
    "p10": (b"YUV4MPEG2 W6 H2 F50:1 Ip C420p10 XYSCSS=420P10", 6, 2, 10, (10, 50, 1, 0)),
    "c444": (b"YUV4MPEG2 W16 H8 F25:1 C444", 16, 8, 8, None),
    "no_w": (b"YUV4MPEG2 H8 F25:1 C420jpeg", 16, 8, 8, None),
    "full": (b"YUV4MPEG2 W16 H8 F25:1 C420jpeg XCOLORRANGE=FULL", 16, 8, 8, (8, 25, 1, 1)),
    "limited": (b"YUV4MPEG2 W6 H2 F25:1 C420p10 XCOLORRANGE=LIMITED", 6, 2, 10, (10, 25, 1, 0)),
    "f0": (b"YUV4MPEG2 W16 H8 F0:0 C420jpeg", 16, 8, 8, (8, 30, 1, 0)),
}
N_PROBE = 3   # frames in each of those clips

# The temporal units of the muxer runs: (key, bytes).  Most begin with the temporal delimiter 12 00; number 3 does not and stays whole
# in Matroska; number 5 is the delimiter alone; key frames alternate.
UNITS = [(i % 2 == 0, (b"\x32\x05" if i == 3 else b"\x12\x00") + (b"" if i == 5 else bytes((i * 7 + j) & 0xFF for j in range(3 + i)))) for i in range(9)]
LONG_UNITS = [(i == 0, b"\x12\x00" + bytes([i, i ^ 0x55])) for i in range(34)]   # at 1:1 frame 31 lies 31 s behind the only key frame
SEQ = bytes([0x0A, 0x0B, 0, 0, 0, 0x24, 0xC4, 0xFF, 0xDF, 0x3F, 0xFE, 0x10, 0x40])   # stands for the sequence header OBU: any bytes
W, H = 72, 56


def _mux_runs():
    """[(output name, units, fps_n, fps_d, bit depth, colour triple, full range)]"""
    runs = []
    for fps in ((25, 1), (30000, 1001)):
        for bd in (8, 10):
            for ci, colour in enumerate(((0, 0, 0), (9, 16, 9), (0, 0, 1))):
                for ext in ("mkv", "webm"):
                    runs.append(("m%d_%d_%d.%s" % (fps[0], bd, ci, ext), UNITS, fps[0], fps[1], bd, colour, ci == 1 and bd == 10))
            runs.append(("m%d_%d.ivf" % (fps[0], bd), UNITS, fps[0], fps[1], bd, (0, 0, 0), False))
            runs.append(("m%d_%d.obu" % (fps[0], bd), UNITS, fps[0], fps[1], bd, (9, 16, 9), False))
    runs.append(("long.mkv", LONG_UNITS, 1, 1, 8, (0, 0, 0), False))
    return runs


def _write_inputs(d):
    """the clips, the units and commands.txt in directory d; returns the commands' names in order"""
    names, cmds = [], []
    for name, (hdr, w, h, bd, _) in HEADERS.items():
        (d / (name + ".y4m")).write_bytes(_clip(hdr, _frames(w, h, bd, N_PROBE, 3)))
        names.append("probe:" + name)
        cmds.append("probe %s.y4m" % name)
    five = _frames(16, 8, 8, 5, 11)
    hdr = HEADERS["jpeg"][0]
    (d / "five.y4m").write_bytes(_clip(hdr, five))
    (d / "tail.y4m").write_bytes(_clip(hdr, five) + b"FRAME\n1")   # 7 bytes of a sixth frame
    (d / "header_only.y4m").write_bytes(hdr + b"\n")
    (d / "ip.y4m").write_bytes(_clip(hdr, five, b"FRAME Ip\n"))
    (d / "bad_marker.y4m").write_bytes(hdr + b"\nFRAME Ip\n" + five[0] + b"BOGUS\n" + five[1])
    (d / "late_ip.y4m").write_bytes(hdr + b"\nFRAME\n" + five[0] + b"FRAME Ip\n" + five[1])   # plain first marker: the parallel reader, which refuses frame parameters
    for clip, threads in (("five", 1), ("five", 3), ("five", 8), ("tail", 3), ("header_only", 3), ("ip", 3), ("bad_marker", 3), ("late_ip", 3)):
        names.append("read:%s:%d" % (clip, threads))
        cmds.append("read %s.y4m 2 %d %s_%d.frames" % (clip, threads, clip, threads))
    names += ["probe:header_only", "probe:ip", "fifo"]
    cmds += ["probe header_only.y4m", "probe ip.y4m", "fifo five.y4m 2 fifo.frames"]
    for units, fname in ((UNITS, "units.bin"), (LONG_UNITS, "long_units.bin")):
        (d / fname).write_bytes(b"".join(bytes([key]) + len(tu).to_bytes(4, "little") + tu for key, tu in units))
    for out, units, fn, fd, bd, (cp, tc, mc), full in _mux_runs():
        names.append("mux:" + out)
        cmds.append("mux %s %s %s %d %d %d %d %d %d %d %d %d" % ("units.bin" if units is UNITS else "long_units.bin", out, SEQ.hex(), W, H, fn, fd, bd, cp, tc, mc, int(full)))
    (d / "commands.txt").write_text("\n".join(cmds) + "\n")
    return names


def _run(cxx, tmp, sanitized=False):
    d = tmp / "work"
    d.mkdir()
    names = _write_inputs(d)
    out = host_build.run_program(cxx, SOURCES, tmp / "container_host", args=[d], sanitized=sanitized, extra=["-pthread"], timeout=60)
    assert out.returncode == 0, out.stdout[-500:] + out.stderr[-2000:]
    lines = out.stdout.splitlines()
    assert len(lines) == len(names), out.stdout[-2000:]
    return dict(zip(names, lines)), d


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    """the plain build's lines and directory: built by the host compiler alone - g++ where there is one, so that no HIP-aware compiler is involved"""
    return _run(shutil.which("g++") or host_build.host_cxx(gcc=True), tmp_path_factory.mktemp("container_plain"))


def test_sanitized_build_prints_and_writes_what_the_plain_one_does(plain, tmp_path):
    """... and runs clean under AddressSanitizer and UndefinedBehaviorSanitizer (a stand-alone program, host code only).  Skipped only where
    an empty program does not build and run under the sanitizers"""
    lines, d = _run(host_build.host_cxx(gcc=True), tmp_path, sanitized=True)
    assert lines == plain[0]
    written = sorted(p.name for p in plain[1].iterdir())
    assert written == sorted(p.name for p in d.iterdir()) and len(written) > 50
    for name in written:
        assert (d / name).read_bytes() == (plain[1] / name).read_bytes(), name


def test_headers_and_clip_info(plain):
    for name, (_, w, h, _, want) in HEADERS.items():
        line = plain[0]["probe:" + name]
        if want is None:
            assert line == "probe rc=%d" % E_FORMAT, name
        else:
            assert line == "probe rc=0 w=%d h=%d bd=%d fps=%d:%d cr=%d frames=%d" % ((w, h) + want + (N_PROBE,)), name


def test_regular_file_in_windows_with_any_number_of_readers(plain):
    """5 frames in windows of 2: every frame once, in order, the file's bytes - with 1 reader, 3, and 8 (more than frames)"""
    want = b"".join(_frames(16, 8, 8, 5, 11))
    for threads in (1, 3, 8):
        assert plain[0]["read:five:%d" % threads] == "read open=0 regular=1 total=5 counts=2,2,1,0, err=0"
        assert (plain[1] / ("five_%d.frames" % threads)).read_bytes() == want


def test_trailing_partial_frame_is_a_format_error_after_the_whole_frames(plain):
    assert plain[0]["read:tail:3"] == "read open=0 regular=1 total=5 counts=2,2,1,0, err=%d" % E_FORMAT
    assert (plain[1] / "tail_3.frames").read_bytes() == b"".join(_frames(16, 8, 8, 5, 11))


def test_header_only_is_an_empty_clip(plain):
    assert plain[0]["read:header_only:3"] == "read open=0 regular=0 total=0 counts=0, err=0"
    assert plain[0]["probe:header_only"] == "probe rc=0 w=16 h=8 bd=8 fps=25:1 cr=0 frames=0"


def test_frame_parameters_go_through_the_sequential_reader(plain):
    """FRAME Ip markers: frame count unknown, the same frames; a marker that is not FRAME... is a format error, and so are frame parameters
    behind a plain first marker, which the parallel reader cannot place"""
    five = _frames(16, 8, 8, 5, 11)
    assert plain[0]["probe:ip"] == "probe rc=0 w=16 h=8 bd=8 fps=25:1 cr=0 frames=0"
    assert plain[0]["read:ip:3"] == "read open=0 regular=0 total=0 counts=2,2,1,0, err=0"
    assert (plain[1] / "ip_3.frames").read_bytes() == b"".join(five)
    assert plain[0]["read:bad_marker:3"] == "read open=0 regular=0 total=0 counts=1, err=%d" % E_FORMAT
    assert (plain[1] / "bad_marker_3.frames").read_bytes() == five[0]
    assert plain[0]["read:late_ip:3"] == "read open=0 regular=1 total=2 counts=0, err=%d" % E_FORMAT


def test_fifo_goes_through_the_sequential_reader(plain):
    assert plain[0]["fifo"] == "read open=0 regular=0 total=0 counts=2,2,1,0, err=0"
    assert (plain[1] / "fifo.frames").read_bytes() == b"".join(_frames(16, 8, 8, 5, 11))


def test_container_files_equal_their_restatement(plain):
    n = 0
    for out, units, fn, fd, bd, colour, full in _mux_runs():
        ext = out.rsplit(".", 1)[1]
        if ext == "ivf":
            want, kind = mkv_ref.ivf(units, W, H, fn, fd), 0
        elif ext == "obu":
            want, kind = mkv_ref.obu(units), 2
        else:
            want, kind = mkv_ref.matroska(units, SEQ, W, H, fn, fd, bd, colour, full, b"webm" if ext == "webm" else b"matroska"), 1
        got = (plain[1] / out).read_bytes()
        assert got == want, out
        # the muxer's running byte count (the progress callback's) is the file's length - in Matroska up to the last closed cluster, which end() closes
        assert plain[0]["mux:" + out] == "mux kind=%d frames=%d bytes=%d io=0" % (kind, len(units), len(want)), out
        n += 1
    assert n == 33


def test_the_long_run_splits_a_cluster_without_a_key_frame():
    """(of the restatement, so that the case above is known to hold what it is there for)"""
    mkv = mkv_ref.matroska(LONG_UNITS, SEQ, W, H, 1, 1, 8)
    top = list(mkv_ref._ebml(mkv, 0, len(mkv)))
    clusters = [e for e in mkv_ref._ebml(mkv, top[1][1], top[1][2]) if e[0] == mkv_ref.CLUSTER]
    blocks = [[mkv[b[1] + 3] for b in list(mkv_ref._ebml(mkv, c[1], c[2]))[1:]] for c in clusters]
    assert [len(b) for b in blocks] == [31, 3] and blocks[0][0] == 0x80 and not any(blocks[1])
