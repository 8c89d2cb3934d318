"""CPU reference of the MXFP4 weight format of ss_gemv_mx4 / ss_quantize_rows_mxfp4 (include/seedstory_hip.h), written from the
definition alone: integer arithmetic on the fp32 bit patterns and a 16-entry table, no fp4 dtype of torch.

  codes  uint8 [N, K / 2]: byte j of a row = code(k = 2j) | code(k = 2j + 1) << 4; a code is sign (bit 3) and an index into GRID
  scales uint8 [N, K / 32]: e8m0, block b (k = 32 b .. 32 b + 31) is multiplied by 2^(byte - 127)

Quantiser, per block of 32: a = amax in fp32; X = exponent(a) - 2 when a's fp32 mantissa field is <= 0x400000, else
exponent(a) - 1 (the smallest power of two with a / 2^X <= 6), clamped to [-13, 13]; an all-zero block gets X = -13.  Codes:
|w| / 2^X rounded to nearest on GRID, ties to the even mantissa bit (= the even grid index), saturated at 6; the sign is kept
unless the value rounds to zero (code 8, -0, is never written)."""
import torch

GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
TABLE = torch.tensor(GRID + tuple(-g for g in GRID), dtype=torch.float64)       # code -> value
X_MIN, X_MAX = -13, 13
# (threshold, inclusive): index = number of thresholds passed; the inclusive ones are the ties that go UP to an even index
_STEPS = ((0.25, False), (0.75, True), (1.25, False), (1.75, True), (2.5, False), (3.5, True), (5.0, False))


def block_exponent(amax):
    """amax fp32 tensor (>= 0) -> int64 X by the bit-defined rule"""
    bits = amax.contiguous().view(torch.int32).to(torch.int64)
    e = ((bits >> 23) & 0xFF) - 127
    X = torch.where((bits & 0x7FFFFF) <= 0x400000, e - 2, e - 1)
    return X.clamp(X_MIN, X_MAX)


def round_codes(v):
    """v fp64 (already divided by 2^X) -> int64 codes 0..15"""
    m = v.abs()
    idx = torch.zeros(v.shape, dtype=torch.int64)
    for th, incl in _STEPS:
        idx += (m >= th) if incl else (m > th)
    return idx | (((v < 0) & (idx > 0)).to(torch.int64) << 3)


def quantize(w):
    """w [N, K] bf16 / fp16 / fp32 holding 16-bit values (CPU), K % 32 == 0 -> (codes [N, K] int64 unpacked, X [N, K / 32] int64)"""
    N, K = w.shape
    assert K % 32 == 0
    wf = w.float().reshape(N, K // 32, 32)
    X = block_exponent(wf.abs().amax(dim=2))
    v = wf.double() * torch.pow(torch.tensor(2.0, dtype=torch.float64), -X.double())[:, :, None]     # a power of two: exact
    return round_codes(v).reshape(N, K), X


def pack(codes, X):
    """unpacked codes [N, K] + exponents [N, K / 32] -> (uint8 [N, K / 2], uint8 [N, K / 32]) in the public layout"""
    c = codes.to(torch.int64)
    return (c[:, 0::2] | (c[:, 1::2] << 4)).to(torch.uint8), (X + 127).to(torch.uint8)


def unpack(codes_u8, scales_u8):
    """the inverse of pack"""
    c = codes_u8.to(torch.int64)
    out = torch.empty(c.shape[0], c.shape[1] * 2, dtype=torch.int64)
    out[:, 0::2] = c & 0xF
    out[:, 1::2] = c >> 4
    return out, scales_u8.to(torch.int64) - 127


def decode(codes, X):
    """unpacked codes [N, K] + exponents [N, K / 32] -> fp64 [N, K]: TABLE[code] * 2^X"""
    s = torch.pow(torch.tensor(2.0, dtype=torch.float64), X.double())
    return TABLE[codes] * s.repeat_interleave(32, dim=1)


def quantize_packed(w):
    """w -> (codes uint8 [N, K / 2], scales uint8 [N, K / 32], fp64 de-quantised values [N, K])"""
    c, X = quantize(w)
    cu, su = pack(c, X)
    return cu, su, decode(c, X)
