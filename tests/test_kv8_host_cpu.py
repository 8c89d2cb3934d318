"""Host side of the fp8 KV shadow cache (kv_cache="fp8"), without a GPU: argument checks that must answer before anything is
launched or a device is needed, the tuning knob, and the properties of the reference quantiser the GPU tests compare against."""
import ctypes as C
import types

import pytest
import torch

import kv8_ref
from seedstory import _lib

SS_EINVAL = -1
BF16, F16, F32 = _lib.SS_BF16, _lib.SS_F16, _lib.SS_F32


def err():
    return _lib.lib().ss_last_error().decode()


@pytest.fixture()
def ptr():
    """host memory, 64-byte aligned: the calls below must refuse before they touch it"""
    buf = C.create_string_buffer(256)
    yield (C.addressof(buf) + 63) // 64 * 64


def test_kv8_null_handle():
    lib = _lib.lib()
    assert lib.ss_llama_set_kv8(None, None, None, None, None) == SS_EINVAL and "null handle" in err()
    assert lib.ss_llama_kv8_invalidate(None, 0) == SS_EINVAL and "kv8_invalidate" in err()


def test_kv8_bytes_query():
    lib = _lib.lib()
    nc, ns = C.c_size_t(), C.c_size_t()
    cfg = _lib.LlamaConfig(4096, 32, 32, 11008, 32066, 4096, 1e-5, BF16, 1152, 512, 66, 2, 8)
    assert lib.ss_llama_kv8_bytes(C.byref(cfg), C.byref(nc), C.byref(ns)) == 0
    rows = 8 * 32 * 32 * 1152
    assert nc.value == rows * 128 and ns.value == rows * 4
    # the cost the documents quote: 2 planes x (128 + 4) bytes x 32 layers x 32 heads = 0.27 MB per position per slot
    assert 2 * (nc.value + ns.value) // (8 * 1152) == 2 * 132 * 32 * 32 == 270336
    cfg.dtype = F32
    assert lib.ss_llama_kv8_bytes(C.byref(cfg), C.byref(nc), C.byref(ns)) == SS_EINVAL and "bf16 or fp16" in err()
    cfg.dtype, cfg.hidden, cfg.n_heads = F16, 48, 2         # head dim 24
    assert lib.ss_llama_kv8_bytes(C.byref(cfg), C.byref(nc), C.byref(ns)) == SS_EINVAL and "head_dim 24" in err()
    assert lib.ss_llama_kv8_bytes(None, C.byref(nc), C.byref(ns)) == SS_EINVAL and "null" in err()


def test_kv_quantize_fp8_bad_arguments(ptr):
    lib, p = _lib.lib(), ptr
    q = lambda *planes, hd=128, dt=BF16, lo=0, hi=4: lib.ss_kv_quantize_fp8(*planes, 2, 8, hd, lo, hi, dt, None)
    assert q(p, p, p, p, p, p, dt=F32) == SS_EINVAL and "bf16 or fp16" in err() and "kv_quantize_fp8" in err()
    for hd in (24, 272, 48, 0):
        assert q(p, p, p, p, p, p, hd=hd) == SS_EINVAL and "head_dim %d" % hd in err()
    for i in range(6):
        planes = [p] * 6
        planes[i] = None
        assert q(*planes) == SS_EINVAL and "NULL" in err(), i
    assert q(p, p, p + 8, p, p, p) == SS_EINVAL and "aligned" in err()
    assert q(p, p, p, p, p, p, lo=5, hi=4) == SS_EINVAL and "rows [5, 4)" in err()
    assert q(p, p, p, p, p, p, lo=0, hi=9) == SS_EINVAL and "rows [0, 9)" in err()


def test_attn_decode_kv8_bad_arguments(ptr):
    lib, p = _lib.lib(), ptr
    a = lambda *ptrs, hd=128, dt=BF16: lib.ss_attn_decode_kv8(*ptrs, 2, hd, 8, dt, None)
    assert a(*[p] * 8, dt=F32) == SS_EINVAL and "bf16 or fp16" in err() and "attn_decode_kv8" in err()
    for hd in (24, 272):
        assert a(*[p] * 8, hd=hd) == SS_EINVAL and "head_dim %d" % hd in err()
    for i in range(8):
        ptrs = [p] * 8
        ptrs[i] = None
        assert a(*ptrs) == SS_EINVAL and "NULL" in err(), i
    assert a(p, p + 4, p, p, p, p, p, p) == SS_EINVAL and "aligned" in err()


def test_kv_cache_value_is_checked():
    from seedstory.llama import LlamaEngine
    stub = types.SimpleNamespace(dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="kv_cache"):
        LlamaEngine._init_kv_cache(stub, "int4")
    LlamaEngine._init_kv_cache(stub, "16bit")       # off whatever the knob says: nothing to enable
    LlamaEngine._init_kv_cache(stub, None)          # the knob's default is off


def test_knob_llama_kv8_round_trips():
    assert _lib.get_tuning("llama_kv8", 7) == 0     # declared, default 0
    _lib.set_tuning("llama_kv8", 1)
    try:
        assert _lib.get_tuning("llama_kv8", 0) == 1
    finally:
        _lib.set_tuning("llama_kv8", 0)
    assert _lib.get_tuning("llama_kv8", 5) == 0


def test_model_level_attribute():
    """LlamaForCausalLM.kv_cache sits beside decode_weights and is part of the engine signature"""
    import inspect
    from src.models_clm import modeling_llama_xformer as M
    src = inspect.getsource(M.LlamaForCausalLM)
    assert "self.kv_cache = None" in src and "self.decode_weights, self.kv_cache)" in src and "kv_cache=self.kv_cache" in src


# ---- the reference quantiser ------------------------------------------------------------------------------------------------
def next_up(x):
    """the next value of x's dtype above a positive x"""
    return (x.view(torch.int16) + 1).view(x.dtype)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_reference_quantiser_properties(dtype):
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(64, 128, generator=g) * torch.logspace(-3, 3, 64, base=2.0)[:, None]).to(dtype)
    x[7] = 0.0
    codes, scale, back = kv8_ref.quantize(x)
    amax = x.float().abs().amax(-1)
    ratio = amax / scale
    nz = amax > 0
    assert bool((ratio[nz] > 224).all()) and bool((ratio[nz] <= 448).all())
    assert float(scale[7]) == 1.0 and not codes[7].any()
    assert torch.equal(scale, torch.exp2(torch.log2(scale).round()))          # powers of two
    assert not ((codes & 0x7f) == 0x7f).any()                                # no NaN code
    # e4m3 keeps 4 significand bits: relative error of a normal code <= 2^-4, absolute error of the small ones <= 2^-10 scale
    d = (back.float() - x.float()).abs()
    assert bool((d <= torch.maximum(x.float().abs() * 2.0 ** -4, scale[:, None] * 2.0 ** -10)).all())
    # boundary rows: amax = 448 * 2^k is the largest value of scale 2^k; the next 16-bit value above it takes 2^(k+1)
    for k in (-10, -3, 0, 4, 7):
        row = torch.zeros(2, 128)
        row[:, 3] = 448.0 * 2.0 ** k
        row = row.to(dtype)
        row[1, 3] = next_up(row[1, 3])
        row[:, 9] = -row[:, 3] / 4
        c, s, _ = kv8_ref.quantize(row)
        assert s.tolist() == [2.0 ** k, 2.0 ** (k + 1)], k
        assert c[0, 3] == 0x7e and c[0, 9] == 0x80 | 0x6e          # 448 and -112
        assert c[1, 3] == 0x76                                     # 224 (+ one 16-bit ulp, rounded away)
