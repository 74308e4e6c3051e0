"""GPU test of what a context reports of its last chunk (include/av1mi.h: the *_result, *_units and *_tiles entry points): nothing on
a fresh context, the chunk's own frame count and no other after an encode, zeros for a fit that did not run, and nothing again after
a chunk that was refused for its parameters - resolve() fails before anything is launched."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, N = 64, 64, 2


def _nothing_to_report(av1mi, c):
    with pytest.raises(av1mi.EncodeFailed) as e:
        c.lf_search_result(N)
    assert e.value.code == av1mi.E_INVALID_ARG
    L = av1mi._lib
    assert [int(f(c._h)) for f in (L.av1mi_lr_fit_units, L.av1mi_lr_wiener_fit_units, L.av1mi_lr_rd_units, L.av1mi_sym_order_tiles,
                                   L.av1mi_inter_partition_units)] == [0, 0, 0, 0, 0]


def test_last_chunk_contract(av1mi):
    p = av1mi.default_params(W, H, 8, keyint=1)
    frames = np.random.default_rng(64).integers(0, 256, N * W * H * 3 // 2, dtype=np.uint8)
    with av1mi.Context(0) as c:
        _nothing_to_report(av1mi, c)
        data, sizes, rep, _ = c.encode_chunk(p, frames, N)
        assert len(data) == sum(sizes) and rep.frames == N
        levels, err = c.lf_search_result(N)
        assert levels.shape == (N, 4) and not err.any()   # (no level search: the table is zeros)
        for n in (N - 1, N + 1):
            with pytest.raises(av1mi.EncodeFailed) as e:
                c.lf_search_result(n)
            assert e.value.code == av1mi.E_INVALID_ARG
        units, fit_err = c.lr_fit_result(N)
        assert units.shape[:2] == (N, 3) and not units.any() and not fit_err.any()   # the fit is off
        # bit_depth 12 is refused by resolve(), before anything is launched: the context then has no last chunk
        bad = av1mi.default_params(W, H, 8, keyint=1)
        bad.bit_depth = 12
        with pytest.raises(av1mi.EncodeFailed) as e:
            c.encode_chunk(bad, np.zeros(N * W * H * 3 // 2 * 2, dtype=np.uint8), N)
        assert e.value.code == av1mi.E_INVALID_ARG
        _nothing_to_report(av1mi, c)
        out = (C.c_int8 * (N * 3 * 4))()
        assert av1mi._lib.av1mi_lr_fit_result(c._h, N, out, None) == av1mi.E_INVALID_ARG
