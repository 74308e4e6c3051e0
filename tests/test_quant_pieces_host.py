"""The reconstruction kernel's quantiser rule (av1-base_amd/csrc/quant_pieces.h: the one step all four quantiser loops of recon_kernel.hip call)
compiled for the host and checked, without a GPU, against the oracle's quantiser (oracle/av1o_enc.c, code_tx_block, restated per
coefficient in tests/host/quant_pieces_host.cpp) and the oracle's scan tables: level, dequantised value, dead-zone class, scan key and
extent - transform sizes 4 .. 64, 8 and 10 bit, the lowest quantiser index, 120 (CQ 30) and the highest, every coefficient value in
+-2^16 plus the extremes that reach the 0x7FFF cap, every (row, column) at every coded width; and the same at the extreme steps of the
quantiser-matrix tables."""
import ctypes as C
import os

import numpy as np
import pytest

import host_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "quant_pieces_host.cpp")
QIDX = (1, 120, 255)


@pytest.fixture(scope="module")
def cxx():
    return host_build.host_cxx()


@pytest.fixture(scope="module")
def quant(cxx, tmp_path_factory):
    lib = C.CDLL(host_build.build_shared(cxx, SRC, tmp_path_factory.mktemp("quant") / "libquantpieces.so"))
    lib.qp_sweep.restype = C.c_long
    lib.qp_sweep.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_long)]
    lib.qp_sweep_qm.restype = C.c_long
    lib.qp_sweep_qm.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_long)]
    lib.qp_qm_max_step.restype = C.c_uint32
    lib.qp_qm_max_step.argtypes = [C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    lib.qp_positions.restype = C.c_long
    lib.qp_keys.argtypes = [C.c_int, C.c_void_p]
    lib.qp_scan_indices.argtypes = [C.c_int, C.c_void_p]
    return lib


@pytest.mark.parametrize("log2n", [2, 3, 4, 5, 6])
@pytest.mark.parametrize("bd", [8, 10])
def test_levels_and_dequantised_values_equal_the_oracle(quant, log2n, bd):
    for qidx in QIDX:
        capped = C.c_long(0)
        assert quant.qp_sweep(log2n, bd, qidx, C.byref(capped)) == 0, qidx
        assert capped.value > 0, qidx   # the extremes reach the cap at every step


@pytest.mark.parametrize("log2n", [2, 3, 4, 5])
@pytest.mark.parametrize("bd", [8, 10])
def test_unified_step_at_the_extreme_quantiser_matrix_steps(quant, log2n, bd):
    """the same sweep - every magnitude class, both signs, the cap, level and dequantised value against the oracle's arithmetic - at the
    steps Round2(q * entry, 5) of the smallest and the largest matrix entry, on the DC and AC steps of the lowest and highest index"""
    for qidx in QIDX:
        capped = C.c_long(0)
        assert quant.qp_sweep_qm(log2n, bd, qidx, C.byref(capped)) == 0, qidx
        assert capped.value > 0, qidx


@pytest.mark.parametrize("bd,top", [(8, 13824), (10, 55297)])
def test_largest_quantiser_matrix_step_is_what_the_header_says(quant, bd, top):
    """q_mul24 needs both operands below 2^24: the level is at most 0x7FFF, and the largest step any table holds is the bound
    quant_pieces.h states (entries 30 .. 242 on ac_q of index 255: 1828 at 8 bit, 7312 at 10)"""
    lo, hi = C.c_uint32(0), C.c_uint32(0)
    assert quant.qp_qm_max_step(bd, C.byref(lo), C.byref(hi)) == top
    assert (lo.value, hi.value) == (30, 242)
    assert top == (({8: 1828, 10: 7312}[bd] * 242 + 16) >> 5) and top < 1 << 16 < 1 << 24


def test_class_key_and_extent_at_every_position(quant):
    assert quant.qp_positions() == 0


@pytest.mark.parametrize("cw", [4, 8, 16, 32])
def test_scan_key_orders_positions_as_the_oracle_scan(quant, oracle, cw):
    """positions sorted by key are the oracle's default scan: the largest key among the nonzero levels is the one eob comes from"""
    keys = np.zeros(cw * cw, np.int32)
    quant.qp_keys(cw, keys.ctypes.data)
    L = oracle.lib()
    L.av1o_default_scan.restype = C.POINTER(C.c_int16)
    L.av1o_default_scan.argtypes = [C.c_int]
    scan = np.ctypeslib.as_array(L.av1o_default_scan({4: 2, 8: 3, 16: 4, 32: 5}[cw]), shape=(cw * cw,)).astype(np.int64)
    assert len(set(keys.tolist())) == cw * cw
    assert np.array_equal(np.argsort(keys, kind="stable"), scan)
    # ... and scan_index names each position's place in that scan outright
    idx = np.full(cw * cw, -1, np.int32)
    quant.qp_scan_indices(cw, idx.ctypes.data)
    assert np.array_equal(scan[idx], np.arange(cw * cw))


def test_standalone_program(cxx, tmp_path):
    out = host_build.run_program(cxx, SRC, tmp_path / "quant_main", defines=["QUANT_PIECES_MAIN"])
    assert out.returncode == 0 and " 0 mismatches" in out.stdout, out.stdout + out.stderr


def test_standalone_program_under_sanitizers(cxx, tmp_path):
    """... and under AddressSanitizer and UndefinedBehaviorSanitizer (host code only).  Skipped only where an empty program does not
    build and run under the sanitizers - their runtimes are not installed; a failure of the project's source is a failure"""
    out = host_build.run_program(cxx, SRC, tmp_path / "quant_main_san", defines=["QUANT_PIECES_MAIN"], sanitized=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert " 0 mismatches" in out.stdout
