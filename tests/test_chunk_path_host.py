"""CPU test of the geometry the symbolize launcher relies on: the ownership predicate the kernels and the launcher share
(av1-base_amd/csrc/av1mi_dev.h), compiled as plain C++ (tests/host/edge_tiles.cpp)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def edge_tiles(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("edge_tiles") / "edge_tiles")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "-x", "c++", "-O1", "-std=c++17", "-Wall", os.path.join(ROOT, "tests", "host", "edge_tiles.cpp"), "-o", exe])
    return exe


def test_full_variant_tiles_are_edge_tiles(edge_tiles):
    """every coded size up to 400 x 400, leaves 8 .. 64, both tile sizes: the compact grid is a superset of the full variant's tiles"""
    assert subprocess.check_output([edge_tiles]).decode().split() == ["ok", "20000"]


@pytest.mark.parametrize("w,h,leaf,tsb,static,want", [
    # (a leaf may overhang the frame edge by less than half its size; an edge superblock whose leaves would overhang by more splits)
    (1920, 1080, 5, 1, 0, 0),      # the headline: the bottom row's 56 lines keep their 32x32 leaves - no launch of the full variant
    (1920, 1080, 6, 1, 0, 0),      # ... and their 64x64 leaves (56 > 32)
    (1920, 1048, 6, 1, 0, 30),     # 24 lines: every superblock of the bottom row splits
    (1920, 1064, 5, 1, 0, 30),     # 40 lines: the leaves at line 32 of the bottom row have 8 lines inside
    (200, 120, 5, 1, 0, 2),        # 8 columns over: the right column's 2 superblocks; the bottom row's 56 lines are left alone
    (200, 104, 5, 1, 0, 5),        # 8 columns and 40 lines over: the right column (2) and the bottom row (4) share the corner
    (128, 64, 5, 1, 0, 0), (128, 64, 5, 1, 1, 2),   # whole superblocks: none - unless the CDFs are static, then every tile
    (328, 248, 5, 2, 0, 2)])       # tiles of 2 x 2 superblocks, 3 x 2 of them: 8 columns over, the right tile column
def test_named_geometries(edge_tiles, w, h, leaf, tsb, static, want):
    assert int(subprocess.check_output([edge_tiles] + [str(v) for v in (w, h, leaf, tsb, static)])) == want
