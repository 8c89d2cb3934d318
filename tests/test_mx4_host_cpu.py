"""Host side of the MXFP4 weight-only decode option, without a GPU: argument checks that must answer before anything is launched,
the launch plan of ss_gemv_mx4 (a pure function of the shape), the new tuning knob, and the reference quantiser the GPU tests
compare against (tests/mxfp4_ref.py) on the cases its definition names."""
import ctypes as C

import pytest
import torch

import mxfp4_ref as R
from seedstory import _lib

SS_EINVAL = -1
BF16, F16, F32 = _lib.SS_BF16, _lib.SS_F16, _lib.SS_F32
MX4, MX4_16, MX4_43 = 9, 10, 11     # SS_GEMV_FORM_MX4 / _EXACT16 / _EXACT43 (include/seedstory_hip.h)


def err():
    return _lib.lib().ss_last_error().decode()


def plan(N, K, nb, dtype=BF16, epi=0, norm=0):
    rows = (C.c_int32 * (16 * 10))()
    n = _lib.lib().ss_gemv_mx4_plan(N, K, nb, dtype, epi, norm, rows, 16)
    return n if n < 0 else [list(rows[i * 10:(i + 1) * 10]) for i in range(n)]


def test_set_decode_mx4_null_handle():
    assert _lib.lib().ss_llama_set_decode_mx4(None, None, None, None) == SS_EINVAL
    assert "llama_set_decode_mx4" in err() and "null handle" in err()


@pytest.mark.parametrize("K", [0, 16, 48, 4112, 8192, 11040])
def test_gemv_mx4_bad_k(K):
    """checked before any pointer is touched or a device is needed: the pointers here are not device memory"""
    lib = _lib.lib()
    buf = C.create_string_buffer(64)
    p = C.addressof(buf)
    assert lib.ss_gemv_mx4(p, p, p, p, 32, K, 2, None, 0.0, None, None, 0, BF16, None) == SS_EINVAL
    assert "K=%d" % K in err() and "gemv_mx4" in err() and "multiple of 32" in err()
    assert plan(32, K, 2) == SS_EINVAL


def test_gemv_mx4_bad_arguments():
    lib = _lib.lib()
    buf = C.create_string_buffer(64)
    p = C.addressof(buf)
    assert lib.ss_gemv_mx4(p, p, p, p, 32, 64, 2, None, 0.0, None, None, 0, F32, None) == SS_EINVAL and "bf16 or fp16" in err()
    assert lib.ss_gemv_mx4(p, p, p, p, 32, 64, 17, None, 0.0, None, None, 0, BF16, None) == SS_EINVAL and "batch" in err()
    assert lib.ss_gemv_mx4(p, p, p, p, 32, 64, 0, None, 0.0, None, None, 0, BF16, None) == SS_EINVAL and "batch" in err()
    assert lib.ss_gemv_mx4(p, p, p, p, 32, 64, 2, None, 0.0, None, None, 8 | 4, BF16, None) == SS_EINVAL and "SILU_MUL" in err()
    assert lib.ss_gemv_mx4(p, p, p, p, 32, 64, 2, None, 0.0, None, None, 2, BF16, None) == SS_EINVAL and "not supported" in err()
    assert lib.ss_gemv_mx4(p, p, p, p, 32, 11008, 2, p, 1e-5, None, None, 0, BF16, None) == SS_EINVAL and "RMSNorm" in err()
    assert lib.ss_gemv_mx4(None, p, p, p, 32, 64, 2, None, 0.0, None, None, 0, BF16, None) == SS_EINVAL and "NULL" in err()
    assert lib.ss_gemv_mx4(p, None, p, p, 32, 64, 2, None, 0.0, None, None, 0, BF16, None) == SS_EINVAL and "NULL" in err()
    assert lib.ss_gemv_mx4(p, p, p, p, 32, 64, 2, None, 0.0, None, None, 1, BF16, None) == SS_EINVAL and "bias" in err()
    assert lib.ss_gemv_mx4(p, p, p, p, 32, 64, 2, None, 0.0, None, None, 4, BF16, None) == SS_EINVAL and "residual" in err()
    assert lib.ss_gemv_mx4(p + 8, p, p, p, 32, 64, 2, None, 0.0, None, None, 0, BF16, None) == SS_EINVAL and "16-byte aligned" in err()
    assert lib.ss_quantize_rows_mxfp4(p, 48, 2, 48, p, p, BF16, None) == SS_EINVAL and "multiple of 32" in err()
    assert lib.ss_quantize_rows_mxfp4(None, 64, 2, 64, p, p, BF16, None) == SS_EINVAL


def test_gemv_mx4_plan_forms():
    """the stream loops at the two LLaMA-7B depths, the predicated kernel elsewhere and under gemv_mfma_generic; one sequence takes
    the same family; the packed 11008-deep form sweeps 9..16 sequences twice; whole rounds of row tiles as the fp8 plan.  The
    parameter column: MFMA steps of 32 k a wave walks, four per 16-byte load (11008: 11 load slots)"""
    for dt in (BF16, F16):
        for nb in (1, 8, 9, 16):
            assert plan(4096, 4096, nb, dt) == [[0, nb, MX4_16, 16, 256, 512, 0, 0, 0, 0]]
            assert plan(12288, 4096, nb, dt, norm=1) == [[0, nb, MX4_16, 16, 256, 512, 0, 0, 0, 0]]
            assert plan(11008, 4096, nb, dt, epi=8, norm=1) == [[0, nb, MX4_16, 16, 230, 512, 0, 0, 1, 0]]    # 688 tiles: 230 x 3
            assert plan(100, 288, nb, dt) == [[0, nb, MX4, 4, 7, 512, 0, 0, 0, 0]]
            assert plan(33, 32, nb, dt) == [[0, nb, MX4, 4, 3, 512, 0, 0, 0, 0]]
    row43 = lambda s0, n: [s0, n, MX4_43, 44, 256, 512, 0, 0, 0, 0]     # noqa: E731
    assert plan(4096, 11008, 1, epi=4) == [row43(0, 1)]
    assert plan(4096, 11008, 8) == [row43(0, 8)]
    assert plan(4096, 11008, 9) == [row43(0, 4), row43(4, 5)]
    assert plan(4096, 11008, 16) == [row43(0, 8), row43(8, 8)]
    assert plan(64, 4064, 4) == [[0, 4, MX4, 16, 4, 512, 0, 0, 0, 0]]
    assert plan(64, 1056, 4) == [[0, 4, MX4, 8, 4, 512, 0, 0, 0, 0]]       # 9 loads of 128 k: two per wave
    _lib.set_tuning("gemv_mfma_generic", 1)
    try:
        assert plan(4096, 4096, 8) == [[0, 8, MX4, 16, 256, 512, 0, 0, 0, 0]]
        assert plan(4096, 11008, 8) == [row43(0, 8)]                        # no predicated kernel that deep
    finally:
        _lib.set_tuning("gemv_mfma_generic", 0)
    _lib.set_tuning("gemv_mfma_blocks", 2)
    try:
        assert plan(40, 4096, 8)[0][4] == 2 and plan(37, 4096, 8)[0][4] == 2 and plan(16, 4096, 8)[0][4] == 1
        assert plan(40, 11008, 16) == [[0, 8, MX4_43, 44, 2, 512, 0, 0, 0, 0], [8, 8, MX4_43, 44, 2, 512, 0, 0, 0, 0]]
    finally:
        _lib.set_tuning("gemv_mfma_blocks", 256)
    assert plan(4096, 4096, 8, dtype=F32) == SS_EINVAL
    assert plan(4096, 4096, 17) == SS_EINVAL and plan(4096, 4096, 0) == SS_EINVAL
    assert plan(4096, 4096, 8, epi=8 | 1) == SS_EINVAL and plan(4096, 4096, 8, epi=2) == SS_EINVAL
    assert plan(4096, 11008, 8, norm=1) == SS_EINVAL and "RMSNorm" in err()
    assert _lib.lib().ss_gemv_mx4_plan(4096, 11008, 16, BF16, 0, 0, (C.c_int32 * 10)(), 1) == SS_EINVAL and "rows needed" in err()


def test_mx4_leaves_the_other_plans_alone():
    """the 16-bit and fp8 plans of the decode shapes are what they were"""
    rows = (C.c_int32 * (16 * 10))()
    assert _lib.lib().ss_gemv_w8_plan(4096, 4096, 8, BF16, 0, 0, rows, 16) == 1 and list(rows[:10]) == [0, 8, 7, 16, 256, 512, 0, 0, 0, 0]
    assert _lib.lib().ss_gemv_plan(4096, 4096, 8, BF16, 0, 0, 1, rows, 16) == 1 and list(rows[:10]) == [0, 8, 3, 16, 256, 512, 0, 0, 0, 0]


def test_knob_llama_decode_mx4_round_trips():
    assert _lib.get_tuning("llama_decode_mx4", 7) == 0           # declared, default 0: a constant default wins over the caller's
    _lib.set_tuning("llama_decode_mx4", 1)
    try:
        assert _lib.get_tuning("llama_decode_mx4", 0) == 1
    finally:
        _lib.set_tuning("llama_decode_mx4", 0)
    assert _lib.get_tuning("llama_decode_mx4", 5) == 0


def test_both_decode_knobs_refused():
    """decode_weights=None reads the knobs: one of them picks its option for a 16-bit engine, both together are an error that
    names both; fp32 engines ignore them"""
    from seedstory.llama import knob_decode_weights
    assert knob_decode_weights(torch.bfloat16) is None
    try:
        _lib.set_tuning("llama_decode_mx4", 1)
        assert knob_decode_weights(torch.bfloat16) == "mxfp4" and knob_decode_weights(torch.float16) == "mxfp4"
        assert knob_decode_weights(torch.float32) is None
        _lib.set_tuning("llama_decode_w8", 1)
        with pytest.raises(ValueError) as ei:
            knob_decode_weights(torch.bfloat16)
        assert "llama_decode_w8" in str(ei.value) and "llama_decode_mx4" in str(ei.value)
        assert knob_decode_weights(torch.float32) is None
        _lib.set_tuning("llama_decode_mx4", 0)
        assert knob_decode_weights(torch.float16) == "fp8"
    finally:
        _lib.set_tuning("llama_decode_w8", 0)
        _lib.set_tuning("llama_decode_mx4", 0)


# ---- the reference quantiser itself ---------------------------------------------------------------------------------------------
def q1(vals, dtype=torch.bfloat16):
    """one block holding vals (padded with zeros) -> (codes [32], X)"""
    w = torch.zeros(1, 32, dtype=dtype)
    w[0, :len(vals)] = torch.tensor(vals, dtype=torch.float32).to(dtype)
    c, X = R.quantize(w)
    return c[0].tolist(), int(X[0, 0])


def test_ref_ties_go_to_the_even_code():
    # amax 6 -> X = 0 (6 = 1.5 * 2^2: mantissa field 0x400000, exponent 2): the values are their own grid coordinates
    ties = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]
    c, X = q1([6.0] + ties + [-t for t in ties])
    assert X == 0 and c[0] == 7
    assert [R.GRID[i] for i in c[1:8]] == [0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0]
    assert c[8] == 0                                                        # -0.25 rounds to zero: code 0, never -0
    assert [c_ - 8 for c_ in c[9:15]] == c[2:8]                              # the sign is kept
    # just off the ties, both sides
    eps = 2.0 ** -7
    c, X = q1([6.0] + [t * (1 + eps) for t in ties] + [t * (1 - eps) for t in ties])
    assert [R.GRID[i] for i in c[1:8]] == [0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]
    assert [R.GRID[i] for i in c[8:15]] == [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0]


def test_ref_block_exponent_rule():
    # the smallest power of two with amax / 2^X <= 6: 6 -> 0, just above 6 -> 1, 4 -> 0, 3 -> -1, just above 3 -> 0
    for a, X in ((6.0, 0), (6.0625, 1), (4.0, 0), (3.0, -1), (3.015625, 0), (1.0, -2), (0.02, -8), (7.0, 1), (8.0, 1), (12.0, 1), (12.5, 2)):
        c, got = q1([a])
        assert got == X, (a, got, X)
        assert a / 2.0 ** got <= 6.0 and a / 2.0 ** (got - 1) > 6.0
        assert c[0] != 0 and abs(R.GRID[c[0]] * 2.0 ** got - a) <= a / 4      # nothing saturates, error <= half a grid step


def test_ref_zero_block_and_clamps():
    c, X = q1([])
    assert X == -13 and not any(c)
    c, X = q1([-0.0, 0.0])
    assert X == -13 and not any(c)
    # amax so small that the clamp acts at the low end: values below 2^-15 round to zero, the grid is {0.5 .. 6} * 2^-13
    c, X = q1([2.0 ** -20, 2.0 ** -14, -(2.0 ** -13), 2.0 ** -15])
    assert X == -13 and c[:4] == [0, 1, 8 | 2, 0]
    # and at the high end: 6 * 2^13 = 49152 is the largest value; beyond it saturates and keeps the sign (fp16 reaches 65504)
    for dtype in (torch.bfloat16, torch.float16):
        c, X = q1([65504.0, -60000.0, 49152.0, 8192.0], dtype)
        assert X == 13 and c[:4] == [7, 15, 7, 2]
    c, X = q1([2.0 ** 40, -(2.0 ** 30)])
    assert X == 13 and c[:2] == [7, 15]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_ref_decoded_values_are_exact_in_the_dtype(dtype):
    """every code under every exponent of the contract: dec * 2^X converts to the dtype and back exactly, and is a normal number"""
    codes = torch.arange(16).repeat(2)[None, :].expand(27, 32).contiguous()
    X = torch.arange(-13, 14)[:, None]
    v = R.decode(codes, X)
    assert torch.equal(v.to(dtype).double(), v)
    nz = v[v != 0].abs()
    assert nz.min() >= torch.finfo(dtype).tiny and nz.max() <= torch.finfo(dtype).max
    assert float(nz.min()) == 2.0 ** -14 and float(nz.max()) == 6.0 * 2.0 ** 13
    # pack / unpack round trip, low nibble = even k
    cu, su = R.pack(codes, X)
    assert cu.dtype == torch.uint8 and tuple(cu.shape) == (27, 16) and int(cu[0, 0]) == 0x10 and int(cu[0, 7]) == 0xFE
    assert int(su[0, 0]) == 114 and int(su[26, 0]) == 140
    c2, X2 = R.unpack(cu, su)
    assert torch.equal(c2, codes) and torch.equal(X2, X)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_ref_quantiser_is_round_to_nearest(dtype):
    """random weights: the de-quantised value is a nearest grid point (|error| <= half the local grid step), never saturated when
    the clamp does not act; relative Frobenius error of N(0, 0.02) weights near the 0.119 of the format"""
    g = torch.Generator().manual_seed(3)
    w = (torch.randn(64, 256, generator=g) * 0.02).to(dtype)
    c, X = R.quantize(w)
    back = R.decode(c, X)
    s = (2.0 ** X.double()).repeat_interleave(32, dim=1)
    m = back.abs() / s
    step = torch.where(m < 2, 0.5, torch.where(m < 4, 1.0, 2.0))
    step = torch.where(m == 2, 1.0, torch.where(m == 4, 2.0, step))           # (at a binade's first point the step above counts)
    assert ((back - w.double()).abs() <= 0.5 * step * s).all()
    assert (w.double().abs() <= 6.0 * s).all()
    rel = float((back - w.double()).norm() / w.double().norm())
    assert 0.10 < rel < 0.14, rel
