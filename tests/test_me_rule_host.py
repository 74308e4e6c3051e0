"""The motion search's rules (av1-base_amd/csrc/me_rule.h) compiled for the host (tests/host/me_rule_host.cpp, a stand-alone program)
against a Python restatement built from tests/part_inter_ref.py - sext12, node_key's ok / cost / key expressions and presearch_centres'
centre code: reach, cost and key of every candidate of blocks at the frame's edges, the round trips of the leaf, node and refined keys
and of the reader of a leaf's motion, the pre-search's centre and reach, and the refinement's candidate sequence and cost.  The same
program runs once more under AddressSanitizer and UndefinedBehaviorSanitizer."""
import os

import numpy as np
import pytest

import host_build
import part_inter_ref as PR
from test_part_inter_host import cxx  # noqa: F401  (the same compiler lookup)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "me_rule_host.cpp")
SIZES = [8, 16, 24, 64, 72, 136]
CENTRES = [-80, -8, 0, 8, 80]
_US = {}   # per range: an all-zero [dy][dx][8][8] table of unit SADs that block_line fills one unit of


def code_of(ccx, ccy):
    """presearch_centres' centre code, from a centre in luma samples (multiples of 8)"""
    return (((ccy >> 3) & 0xFFF) << 12) | ((ccx >> 3) & 0xFFF)


def centre_of(code):
    return 8 * PR.sext12(code), 8 * PR.sext12(code >> 12)


def sad_table(R, seed, n):
    nc = 2 * R + 1
    return ((np.arange(nc)[:, None] * 37 + np.arange(nc)[None, :] * 101 + seed) % 7) * n


def block_line(W, H, n, x, y, R, code, seed):
    """what the program prints of a B case, and (has valid, has invalid candidates)"""
    nc = 2 * R + 1
    ccx, ccy = centre_of(code)
    sad = sad_table(R, seed, n).astype(np.int64)
    # node_key's expressions
    dy = np.arange(nc)[:, None] - R + ccy
    dx = np.arange(nc)[None, :] - R + ccx
    cost = sad + n * (np.abs(dx) + np.abs(dy))
    ok = (x + dx >= -16) & (x + dx + n <= W + 16) & (y + dy >= -16) & (y + dy + n <= H + 16)
    idx = np.arange(nc)[:, None] * nc + np.arange(nc)[None, :]
    valid = int(ok.sum())
    total = int(np.where(ok, (cost << 11) + idx + 1, 0).sum())
    # ... and node_key itself, on unit SADs that hold the table in the block's first unit
    sb_x, sb_y = x & ~63, y & ~63
    us = _US.setdefault(R, np.zeros((nc, nc, 8, 8), np.int64))
    us[:, :, (y - sb_y) >> 3, (x - sb_x) >> 3] = sad
    nk = PR.node_key(us, W, H, R, ccx, ccy, x, y, n, sb_x, sb_y)
    us[:, :, (y - sb_y) >> 3, (x - sb_x) >> 3] = 0
    if nk is None:
        assert valid == 0
        best, nbest = PR.ALL_ONES, 0xFFFFFFFF
    else:
        best = (code << 40) | (nk[0] << 16) | nk[1]
        assert best == (code << 40) | int(np.where(ok, (cost << 16) | idx, np.int64(1) << 62).min())
        nbest = (nk[0] << 11) | nk[1] if n <= 32 else 0xFFFFFFFF
    return "%d %d %d %d %016x %08x" % (ccx, ccy, valid, total, best, nbest), valid > 0, valid < nc * nc


def refine_line(step, br, bc, n, satd):
    """the explicit list: step 8 the base only; steps 4 and 2 the eight neighbours in (row, col) raster order, the centre skipped"""
    if step == 8:
        cands = {4: (br, bc)}
    else:
        cands = {k: (br + r * step, bc + c * step) for k, (r, c) in enumerate((r, c) for r in (-1, 0, 1) for c in (-1, 0, 1)) if (r, c) != (0, 0)}
    return {k: (mr, mc, (satd >> 3) + ((n * (abs(mr) + abs(mc))) >> 3)) for k, (mr, mc) in cands.items()}


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """(path of the case file, per line what the program must print - a string, or for S lines the candidates' dictionary)"""
    path = str(tmp_path_factory.mktemp("me_rule") / "cases.txt")
    lines, want = [], []
    seen = {n: [False, False] for n in (8, 16, 32, 64)}
    none_at_all, seed = 0, 0
    for W in SIZES:
        for H in SIZES:
            for n in (8, 16, 32, 64):
                for x in sorted({0, W - 8}):
                    for y in sorted({0, H - 8}):
                        for R in (8, 16):
                            for ccx in CENTRES:
                                for ccy in CENTRES:
                                    seed += 1
                                    code = code_of(ccx, ccy)
                                    assert centre_of(code) == (ccx, ccy)
                                    lines.append("B %d %d %d %d %d %d %d %d" % (W, H, n, x, y, R, code, seed))
                                    w, some, some_not = block_line(W, H, n, x, y, R, code, seed)
                                    want.append(w)
                                    seen[n][0] |= some
                                    seen[n][1] |= some_not
                                    none_at_all += not some
    assert all(a and b for a, b in seen.values()), seen   # every block size has valid and invalid candidates
    assert none_at_all > 0                                # and some block has no valid candidate at all
    nk = PR.node_key(np.zeros((17, 17, 8, 8), np.int64), 8, 8, 8, -80, 0, 0, 0, 8, 0, 0)
    assert nk is None                                     # (a centre of -80 at W = 8 is one)
    # round trips
    codes = [code_of(cx, cy) for cx in (-80, 8) for cy in (-8, 80)]
    for code in codes:
        ccx, ccy = centre_of(code)
        for cost in (0, (1 << 24) - 1):
            for R, idx in ((16, 0), (16, 33 * 33 - 1), (8, 0), (8, 17 * 17 - 1)):
                nc = 2 * R + 1
                key = (code << 40) | (cost << 16) | idx
                dy, dx = idx // nc - R + ccy, idx % nc - R + ccx
                lines.append("K %d %d %d %d" % (code, cost, idx, R))
                want.append("%016x %d %d %d %d %d" % (key, cost, idx, dy, dx, cost))
                for n in (8, 64):   # the reader without subpel: the vector in eighth samples, the cost less the vector's penalty
                    pen = n * (abs(dx) + abs(dy))
                    c = max(cost, pen)
                    lines.append("M %d %d %d %d %d" % (code, c, idx, R, n))
                    want.append("%d %d %d" % (8 * dy, 8 * dx, c - pen))
    for cost in (0, (1 << 21) - 1):
        for idx in (0, 33 * 33 - 1):
            lines.append("N %d %d" % (cost, idx))
            want.append("%08x %d %d" % ((cost << 11) | idx, cost, idx))
    mvs = [s * ((80 + 16) * 8) + o for s in (-1, 1) for o in (-6, 6)]
    for mr in mvs:
        for mc in mvs:
            for sad in (0, 64 * 64 * 1023):
                lines.append("F %d %d %d" % (sad, mr, mc))
                want.append("%016x %d %d %d" % ((sad << 36) | ((mr & 0xFFFF) << 16) | (mc & 0xFFFF), mr, mc, sad))
    # the pre-search: the winner's centre and code (presearch_centres' expressions), and its reach with the clipped superblock
    for dqx in range(-16, 17):
        for dqy in (-16, -15, -1, 0, 1, 2, 15, 16):
            cx, cy = ((dqx + 1) >> 1) * 8, ((dqy + 1) >> 1) * 8
            code = ((((dqy + 1) >> 1) & 0xFFF) << 12) | (((dqx + 1) >> 1) & 0xFFF)
            lines.append("Q %d %d" % (dqx, dqy))
            want.append("%d %d %d %d %d" % (cx, cy, code, cx, cy))
            assert centre_of(code) == (cx, cy)
    for W in SIZES:
        for H in SIZES:
            for sx in range(0, W, 64):
                for sy in range(0, H, 64):
                    for dqx in (-16, -5, -4, -3, 0, 3, 4, 5, 16):
                        for dqy in (-16, -4, 0, 4, 16):
                            ccx, ccy = ((dqx + 1) >> 1) * 8, ((dqy + 1) >> 1) * 8
                            sbw, sbh = min(W - sx, 64), min(H - sy, 64)
                            out = sx + ccx < -16 or sx + ccx + sbw > W + 16 or sy + ccy < -16 or sy + ccy + sbh > H + 16
                            lines.append("P %d %d %d %d %d %d" % (W, H, sx, sy, dqx, dqy))
                            want.append("%d %d %d" % (sbw, sbh, not out))
    # reach in eighth samples (the refinement's form of the bound)
    for size in SIZES:
        for n in (8, 64):
            for p in sorted({0, size - 8}):
                for m in [s * 8 * d + o for s in (-1, 1) for d in (0, 15, 16, 17, 80) for o in (-6, -2, 0, 2, 6)]:
                    out = p * 8 + m < -128 or (p + n) * 8 + m > (size + 16) * 8
                    lines.append("E %d %d %d %d" % (p, m, n, size))
                    want.append("%d" % (not out))
    # the refinement's stages
    for step in (8, 4, 2):
        for br in (-100, 36):
            for bc in (-44, 120):
                for n in (8, 64):
                    for satd in (0, 7, 8, 9, 4095, 4096, 4097):
                        lines.append("S %d %d %d %d %d" % (step, br, bc, n, satd))
                        want.append(refine_line(step, br, bc, n, satd))
    open(path, "w").write("\n".join(lines) + "\n")
    return path, want


def _check(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        if isinstance(w, dict):   # S: "flag mr mc cost" per k; the candidates in order are the explicit list
            v = [int(t) for t in g.split()]
            g = {k: tuple(v[4 * k + 1:4 * k + 4]) for k in range(9) if v[4 * k]}
            assert list(g) == sorted(g)
        assert g == w, (i, g, w)


def test_standalone_program_equals_the_restatement(cxx, cases, tmp_path):  # noqa: F811
    out = host_build.run_program(cxx, SRC, tmp_path / "me_rule_host", args=[cases[0]])
    assert out.returncode == 0, out.stderr[-2000:]
    _check(out.stdout.split("\n")[:-1], cases[1])


def test_standalone_program_under_sanitizers(cxx, cases, tmp_path):  # noqa: F811
    """... and under AddressSanitizer and UndefinedBehaviorSanitizer (host code only, run on its own).  Skipped only where an empty
    program does not build and run under the sanitizers - their runtimes are not installed"""
    out = host_build.run_program(cxx, SRC, tmp_path / "me_rule_host_san", args=[cases[0]], sanitized=True)
    assert out.returncode == 0, out.stdout[-500:] + out.stderr[-2000:]
    _check(out.stdout.split("\n")[:-1], cases[1])
