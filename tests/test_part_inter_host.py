"""The inter frames' partition rule (av1-base_amd/csrc/part_inter_rule.h) compiled for the host (tests/host/part_inter_host.cpp, a
stand-alone program) against the numpy restatement (tests/part_inter_ref.py): every frame width and height 8 .. 136 in steps of 8 - every
remainder against 64, one to three superblocks each way - and every min_block_log2 <= block_log2 in 3 .. 6, on node costs read from a file:
costs that tie exactly (S == cL), costs one off either way, and nodes without a valid candidate.  The same program runs once more under
AddressSanitizer and UndefinedBehaviorSanitizer."""
import os

import numpy as np
import pytest

import host_build
import part_inter_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "part_inter_host.cpp")
INF = 0xFFFFFFFF


def heap_index(ox, oy, bsl):
    """node (ox, oy, 2^bsl) of a superblock in heap order: levels 64, 32, 16, 8, each in Z order"""
    level = 6 - bsl
    z = 0
    for d in range(level):   # digit d of z, most significant first, is the quadrant at size 32 >> d
        s = 32 >> d
        z = (z << 2) | (((oy // s) & 1) << 1) | ((ox // s) & 1)
    return (0, 1, 5, 21)[level] + z


def make_costs(rng, W, H, lo, hi, acq, sb_x, sb_y):
    """85 costs, bottom up: a decidable node's cost is its S, S - 1, S + 1, anything, or infinite"""
    cL = [INF] * 85

    def gen(x, y, bsl):
        n, h = 1 << bsl, 1 << (bsl - 1)
        i = heap_index(x - sb_x, y - sb_y, bsl)
        if bsl == 3:
            c = None if rng.random() < 0.04 else int(rng.integers(0, 300))
            cL[i] = INF if c is None else c
            return c
        s = 0
        for q in range(4):
            qx, qy = x + (q & 1) * h, y + (q >> 1) * h
            if qx < W and qy < H:
                s = PR._add(s, gen(qx, qy, bsl - 1))
        S = PR._add(s, PR.penalty(n, acq))
        pick = rng.integers(0, 6)
        c = None if pick == 5 or (S is None and pick < 3) else (S + int(pick) - 1 if pick < 3 else int(rng.integers(0, 1 << 20)))
        if c is not None and c < 0:
            c = 0
        cL[i] = INF if c is None else c
        if y + h >= H or x + h >= W:
            return s
        if bsl <= lo:
            return c
        if bsl > hi:
            return s
        return S if S is not None and (c is None or S < c) else c

    gen(sb_x, sb_y, 6)
    return cL


@pytest.fixture(scope="module")
def cxx():
    return host_build.host_cxx(gcc=True)


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """(path of the case file, the numpy rule's answer per line)"""
    rng = np.random.default_rng(85)
    path = str(tmp_path_factory.mktemp("part_inter") / "cases.txt")
    want, ties, infs = [], 0, 0
    with open(path, "w") as f:
        for W in range(8, 137, 8):
            for H in range(8, 137, 8):
                for hi in range(3, 7):
                    for lo in range(3, hi + 1):
                        acq = int(rng.choice([4, 19, 140, 1828, 21387]))
                        for sb_y in range(0, H, 64):
                            for sb_x in range(0, W, 64):
                                cL = make_costs(rng, W, H, lo, hi, acq, sb_x, sb_y)
                                f.write(" ".join(str(v) for v in [W, H, lo, hi, acq, sb_x, sb_y] + cL) + "\n")
                                st = PR.Stats()
                                mask, leaves = PR.decide_sb(lambda x, y, b: None if cL[heap_index(x - sb_x, y - sb_y, b)] == INF else cL[heap_index(x - sb_x, y - sb_y, b)],
                                                            W, H, lo, hi, acq, sb_x, sb_y, st)
                                flags = ["0"] * 85
                                for (x, y, b) in leaves:
                                    flags[heap_index(x - sb_x, y - sb_y, b)] = "1"
                                want.append("%d %s" % (mask, "".join(flags)))
                                ties += sum(st.tie.values())
                                infs += cL.count(INF)
    assert ties > 100 and infs > 100   # the file does hold ties and nodes without a candidate
    return path, want


def test_standalone_program_equals_the_numpy_rule(cxx, cases, tmp_path):
    out = host_build.run_program(cxx, SRC, tmp_path / "part_inter_host", args=[cases[0]])
    assert out.returncode == 0, out.stderr[-2000:]
    got = out.stdout.split("\n")[:-1]
    assert len(got) == len(cases[1])
    bad = [(i, g, w) for i, (g, w) in enumerate(zip(got, cases[1])) if g != w]
    assert not bad, bad[:3]


def test_standalone_program_under_sanitizers(cxx, cases, tmp_path):
    """... and under AddressSanitizer and UndefinedBehaviorSanitizer (host code only, run on its own).  Skipped only where an empty
    program does not build and run under the sanitizers - their runtimes are not installed"""
    out = host_build.run_program(cxx, SRC, tmp_path / "part_inter_host_san", args=[cases[0]], sanitized=True)
    assert out.returncode == 0, out.stdout[-500:] + out.stderr[-2000:]
    assert out.stdout.split("\n")[:-1] == cases[1]
