"""The quantisation of the fp8 (e4m3) KV shadow cache (include/seedstory_hip.h, ss_kv_quantize_fp8) in torch on the CPU: the
reference of tests/test_kv8_*.py.  Not a test file."""
import torch

F8 = torch.float8_e4m3fn


def quantize(x):
    """x [..., hd] bf16 / fp16 (finite) -> (codes uint8 [..., hd], scales fp32 [...], de-quantised tensor in x's dtype).
    scale = 2^e, e the smallest integer with amax <= 448 * 2^e: frexp, not log2 (amax = m * 2^t, m in [0.5, 1): e = t - 9 if
    m <= 0.875 else t - 8), e >= -126; amax == 0 -> scale 1.  The de-quantised values are exact in x's dtype (asserted)."""
    assert x.dtype in (torch.bfloat16, torch.float16) and x.device.type == "cpu"
    xf = x.float()
    amax = xf.abs().amax(-1)
    m, t = torch.frexp(amax)
    e = torch.where(m <= 0.875, t - 9, t - 8).clamp_min(-126)
    e = torch.where(amax == 0, torch.zeros_like(e), e)
    one = torch.ones_like(amax)
    scale, inv = torch.ldexp(one, e), torch.ldexp(one, -e)
    scaled = xf * inv[..., None]                        # exact: a power of two, no overflow, no underflow
    assert float(scaled.abs().max()) <= 448.0 if scaled.numel() else True
    codes = scaled.to(F8)                               # round to nearest even
    deq = codes.float() * scale[..., None]
    back = deq.to(x.dtype)
    assert torch.equal(back.float(), deq), "code * scale must be exact in %s" % x.dtype
    return codes.view(torch.uint8), scale, back
