"""Host side of the fp8 weight-only decode option, without a GPU: argument checks that must answer before anything is launched,
the launch plan of ss_gemv_w8 (a pure function of the shape) and the new tuning knob."""
import ctypes as C

import pytest

from seedstory import _lib

SS_EINVAL = -1
BF16, F16, F32 = _lib.SS_BF16, _lib.SS_F16, _lib.SS_F32
W8, W8_16, W8_43 = 6, 7, 8      # SS_GEMV_FORM_W8 / _EXACT16 / _EXACT43 (include/seedstory_hip.h)


def err():
    return _lib.lib().ss_last_error().decode()


def plan(N, K, nb, dtype=BF16, epi=0, norm=0):
    rows = (C.c_int32 * (16 * 10))()
    n = _lib.lib().ss_gemv_w8_plan(N, K, nb, dtype, epi, norm, rows, 16)
    return n if n < 0 else [list(rows[i * 10:(i + 1) * 10]) for i in range(n)]


def test_set_decode_w8_null_handle():
    assert _lib.lib().ss_llama_set_decode_w8(None, None, None, None) == SS_EINVAL
    assert "null handle" in err()


@pytest.mark.parametrize("K", [0, 8, 24, 4104, 4112, 8192, 11024])
def test_gemv_w8_bad_k(K):
    """checked before any pointer is touched or a device is needed: the pointers here are not device memory"""
    lib = _lib.lib()
    buf = C.create_string_buffer(64)
    p = C.addressof(buf)
    assert lib.ss_gemv_w8(p, p, p, p, 32, K, 2, None, 0.0, None, None, 0, BF16, None) == SS_EINVAL
    assert "K=%d" % K in err() and "gemv_w8" in err()
    assert plan(32, K, 2) == SS_EINVAL


def test_gemv_w8_bad_arguments():
    lib = _lib.lib()
    buf = C.create_string_buffer(64)
    p = C.addressof(buf)
    assert lib.ss_gemv_w8(p, p, p, p, 32, 64, 2, None, 0.0, None, None, 0, F32, None) == SS_EINVAL and "bf16 or fp16" in err()
    assert lib.ss_gemv_w8(p, p, p, p, 32, 64, 17, None, 0.0, None, None, 0, BF16, None) == SS_EINVAL and "batch" in err()
    assert lib.ss_gemv_w8(p, p, p, p, 32, 64, 2, None, 0.0, None, None, 8 | 4, BF16, None) == SS_EINVAL and "SILU_MUL" in err()
    assert lib.ss_gemv_w8(p, p, p, p, 32, 64, 2, None, 0.0, None, None, 2, BF16, None) == SS_EINVAL       # GELU
    assert lib.ss_gemv_w8(p, p, p, p, 32, 11008, 2, p, 1e-5, None, None, 0, BF16, None) == SS_EINVAL and "RMSNorm" in err()
    assert lib.ss_gemv_w8(None, p, p, p, 32, 64, 2, None, 0.0, None, None, 0, BF16, None) == SS_EINVAL and "NULL" in err()
    assert lib.ss_gemv_w8(p, p, p, p, 32, 64, 2, None, 0.0, None, None, 1, BF16, None) == SS_EINVAL and "bias" in err()


def test_gemv_w8_plan_forms():
    """the stream loops at the two LLaMA-7B depths, the predicated kernel elsewhere and under gemv_mfma_generic; one sequence takes
    the same family; the packed 11008-deep form sweeps 9..16 sequences twice; whole rounds of row tiles as the 16-bit MFMA forms"""
    for dt in (BF16, F16):
        for nb in (1, 3, 8, 16):
            assert plan(4096, 4096, nb, dt) == [[0, nb, W8_16, 16, 256, 512, 0, 0, 0, 0]]
            assert plan(100, 272, nb, dt) == [[0, nb, W8, 2, 7, 512, 0, 0, 0, 0]]
            assert plan(33, 16, nb, dt) == [[0, nb, W8, 2, 3, 512, 0, 0, 0, 0]]
    assert plan(12288, 4096, 8, norm=1) == [[0, 8, W8_16, 16, 256, 512, 0, 0, 0, 0]]
    assert plan(11008, 4096, 8, epi=8, norm=1) == [[0, 8, W8_16, 16, 230, 512, 0, 0, 1, 0]]       # 688 tiles: 230 x 3
    assert plan(4096, 11008, 1, epi=4) == [[0, 1, W8_43, 43, 256, 512, 0, 0, 0, 0]]
    assert plan(4096, 11008, 8) == [[0, 8, W8_43, 43, 256, 512, 0, 0, 0, 0]]
    assert plan(4096, 11008, 9) == [[0, 4, W8_43, 43, 256, 512, 0, 0, 0, 0], [4, 5, W8_43, 43, 256, 512, 0, 0, 0, 0]]
    assert plan(4096, 11008, 16) == [[0, 8, W8_43, 43, 256, 512, 0, 0, 0, 0], [8, 8, W8_43, 43, 256, 512, 0, 0, 0, 0]]
    assert plan(64, 4080, 4) == [[0, 4, W8, 16, 4, 512, 0, 0, 0, 0]]
    _lib.set_tuning("gemv_mfma_generic", 1)
    try:
        assert plan(4096, 4096, 8) == [[0, 8, W8, 16, 256, 512, 0, 0, 0, 0]]
        assert plan(4096, 11008, 8) == [[0, 8, W8_43, 43, 256, 512, 0, 0, 0, 0]]     # no predicated kernel that deep
    finally:
        _lib.set_tuning("gemv_mfma_generic", 0)
    _lib.set_tuning("gemv_mfma_blocks", 2)
    try:
        assert plan(40, 4096, 8)[0][4] == 2 and plan(37, 4096, 8)[0][4] == 2 and plan(16, 4096, 8)[0][4] == 1
    finally:
        _lib.set_tuning("gemv_mfma_blocks", 256)
    assert plan(4096, 4096, 8, dtype=F32) == SS_EINVAL
    assert _lib.lib().ss_gemv_w8_plan(4096, 11008, 16, BF16, 0, 0, (C.c_int32 * 10)(), 1) == SS_EINVAL and "rows needed" in err()


def test_knob_llama_decode_w8_round_trips():
    assert _lib.get_tuning("llama_decode_w8", 7) == 0            # declared, default 0: a constant default wins over the caller's
    _lib.set_tuning("llama_decode_w8", 1)
    try:
        assert _lib.get_tuning("llama_decode_w8", 0) == 1
    finally:
        _lib.set_tuning("llama_decode_w8", 0)
    assert _lib.get_tuning("llama_decode_w8", 5) == 0
