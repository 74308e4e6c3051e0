"""CPU test of the compact CDF image the host builds for the regular symbolize variants (av1-base_amd/csrc/av1mi_dev.h:
av1mi_cdf_compact_build), compiled as plain C++ (tests/host/cdf_compact.cpp) - once as it is and once with the address and
undefined-behaviour sanitizers: for leaves of 8 .. 64 samples it equals the gather the kernel's waves did before, restated there."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "sanitized"])
def test_image_equals_the_gather(tmp_path, flags):
    exe = str(tmp_path / "cdf_compact")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "-x", "c++", "-O1", "-std=c++17", "-Wall"] + flags + [os.path.join(ROOT, "tests", "host", "cdf_compact.cpp"), "-o", exe])
    assert subprocess.check_output([exe]).decode().split() == ["ok", "4"]
