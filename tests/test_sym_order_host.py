"""CPU test of the rule that orders symbolize's tiles (av1-base_amd/csrc/tile_weight_rule.h: weight -> class), compiled as plain C++
(tests/host/tile_weight_rule.cpp, a program of its own) - once as it is and once with the address and undefined-behaviour sanitizers:
every weight up to a 2 x 2-superblock tile's largest sum has a class in 0 .. 15, the classes never decrease, weight 0 alone is class 0
and the largest sums are in the top class."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "sanitized"])
def test_weight_classes_are_monotone_and_bounded(tmp_path, flags):
    exe = str(tmp_path / "tile_weight_rule")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "-x", "c++", "-O1", "-std=c++17", "-Wall"] + flags + [os.path.join(ROOT, "tests", "host", "tile_weight_rule.cpp"), "-o", exe])
    out = subprocess.check_output([exe]).decode().split()
    assert out[:2] == ["ok", "16"] and 0 < int(out[2]) <= 6144
