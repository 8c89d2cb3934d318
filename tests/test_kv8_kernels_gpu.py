"""The kernels of the fp8 (e4m3) KV shadow cache: ss_kv_quantize_fp8 (bit-equal to tests/kv8_ref.py) and ss_attn_decode_kv8
(element-wise fp64 bound over the de-quantised operands, which are exact in the model dtype; poisoned tail; exact probe)."""
import math

import pytest
import torch

import kernel_check as KC
import kv8_ref
from test_kernel_edges_gpu import DEV, D16, dev, dname, guarded, knobs, ops  # noqa: F401  (ops: the fixture)

pytestmark = pytest.mark.gpu


def next_up(x):
    return (x.view(torch.int16) + 1).view(x.dtype)


def quantiser_planes(H, cap, hd, dtype, seed):
    """K / V planes [H, cap, hd]: random normal rows of many magnitudes, and in K the rows the definition turns on"""
    g = torch.Generator().manual_seed(700 + seed)
    mag = torch.logspace(-6, 6, cap, base=2.0)[None, :, None]
    k = (torch.randn(H, cap, hd, generator=g) * mag).to(dtype)
    v = (torch.randn(H, cap, hd, generator=g) * mag.flip(1)).to(dtype)
    r = 0
    for kexp in (-10, -3, 0, 4, 7):                     # amax = 448 * 2^k, and the next 16-bit value above it
        for up in (False, True):
            row = (torch.randn(hd, generator=g) * 2.0 ** kexp).to(dtype)
            top = torch.tensor(448.0 * 2.0 ** kexp).to(dtype)
            row[(5 * r) % hd] = -(next_up(top) if up else top) if r % 2 else (next_up(top) if up else top)
            k[r % H, r] = row
            r += 1
    k[1, r] = 0.0                                       # an all-zero row
    k[2, r + 1] = 0.0
    k[2, r + 1, hd - 1] = -0.0                          # -0.0 among zeros
    k[3, r + 2] = (torch.randn(hd, generator=g) * 1e-3).to(dtype)      # one large, many tiny entries
    k[3, r + 2, 17] = 300.0
    k[0, r + 3] = (torch.randn(hd, generator=g) * 3.0).to(dtype)
    k[0, r + 3, 0::2] = -0.0                            # -0.0 among ordinary values
    assert r + 3 < cap
    return k, v


@pytest.mark.parametrize("dtype", D16, ids=dname)
@pytest.mark.parametrize("hd", [64, 128])
def test_kv_quantize_fp8_bit_equal(ops, hd, dtype):
    H, cap = KC.DECODE_HEADS, 80
    k, v = quantiser_planes(H, cap, hd, dtype, hd)
    ref = [kv8_ref.quantize(t) for t in (k, v)]
    kd, vd = dev(k), dev(v)
    for lo, hi in ((0, 1), (3, 37), (0, cap)):
        out = (torch.full((H, cap, hd), 0xA5, dtype=torch.uint8, device=DEV), torch.full((H, cap, hd), 0x5A, dtype=torch.uint8, device=DEV),
               torch.full((H, cap), 0x7FA5A5A5, dtype=torch.int32, device=DEV).view(torch.float32),
               torch.full((H, cap), 0x7FA5A5A5, dtype=torch.int32, device=DEV).view(torch.float32))
        ops.kv_quantize_fp8(kd, vd, lo, hi, out=out)
        for i, (name, fill) in enumerate((("K", 0xA5), ("V", 0x5A))):
            what = "kv_quantize_fp8 %s hd %d %s rows [%d, %d)" % (name, hd, dname(dtype), lo, hi)
            codes, scale = out[i].cpu(), out[2 + i].cpu()
            bad = (codes[:, lo:hi] != ref[i][0][:, lo:hi]).nonzero()
            assert not bad.numel(), "%s: %d codes differ, first at %s: got %#x, want %#x" % (
                what, bad.shape[0], bad[0].tolist(), int(codes[:, lo:hi][tuple(bad[0])]), int(ref[i][0][:, lo:hi][tuple(bad[0])]))
            assert torch.equal(scale[:, lo:hi].view(torch.int32), ref[i][1][:, lo:hi].view(torch.int32)), what + ": scales"
            outside = torch.ones(cap, dtype=torch.bool)
            outside[lo:hi] = False
            assert bool((codes[:, outside] == fill).all()), what + ": codes outside the rows written"
            assert bool((scale.view(torch.int32)[:, outside] == 0x7FA5A5A5).all()), what + ": scales outside the rows written"


def shadow_planes(kc, vc, kvl):
    """kv8_ref of the first kvl rows of 16-bit planes [H, cap, hd]; the tail of all four planes poisoned (codes 0x7f = NaN, NaN
    scales).  -> (k_codes, v_codes, k_scale, v_scale) on the device, de-quantised K, V [H, kvl, hd]"""
    H, cap, hd = kc.shape
    kq, ks, kb = kv8_ref.quantize(kc[:, :kvl])
    vq, vs, vb = kv8_ref.quantize(vc[:, :kvl])
    codes = [torch.full((H, cap, hd), 0x7f, dtype=torch.uint8) for _ in range(2)]
    scales = [torch.full((H, cap), float("nan")) for _ in range(2)]
    codes[0][:, :kvl], codes[1][:, :kvl], scales[0][:, :kvl], scales[1][:, :kvl] = kq, vq, ks, vs
    return [dev(t) for t in codes + scales], kb, vb


@pytest.mark.parametrize("dtype", D16, ids=dname)
@pytest.mark.parametrize("hd", [64, 128])
def test_attn_decode_kv8_splits_poison_bound(ops, hd, dtype):
    """the cases of test_attn_decode_splits_poison_selector over the shadow: every element inside KC.attention_bound of the
    de-quantised operands (exact in the model dtype; the kernel accumulates in fp32, so the bound needs no change)"""
    H, cap = KC.DECODE_HEADS, KC.DECODE_CAP
    scale = 1.0 / math.sqrt(hd)
    for kvl in KC.DECODE_KV_LENS:
        g_ = torch.Generator().manual_seed(hd + kvl)
        q = torch.randn(H * hd, generator=g_).to(dtype)
        kc = torch.randn(H, cap, hd, generator=g_).to(dtype)
        vc = torch.randn(H, cap, hd, generator=g_).to(dtype)
        planes, kb, vb = shadow_planes(kc, vc, kvl)
        ref, tol = KC.attention_bound(q.view(H, 1, hd), kb, vb, scale, None, dtype)
        n = torch.tensor([kvl], dtype=torch.int32, device=DEV)
        outs = {}
        for ns in KC.DECODE_NSPLITS:
            what = "attn_decode_kv8 hd %d %s nsplit %d kv_len %d" % (hd, dname(dtype), ns, kvl)
            with knobs(attn_decode_nsplit=ns):
                g = guarded(1, H * hd, dtype)
                ops.attn_decode_kv8(dev(q), *planes, n, out=g.view(H * hd))
                y = g.check(what).view(H, 1, hd)
                KC.check(y, ref, tol, what, family="attn_decode_kv8", dtype=dtype)
                outs[ns] = y
        assert torch.equal(outs[0], outs[16]), "attn_decode_kv8 nsplit 0 vs 16, kv_len %d" % kvl
    print(KC.worst_table())


def kv8_selector(kvl, hd, dtype, H, seed):
    """KC.attention_selector restricted to what e4m3 holds exactly: key j = 16 hi + lo (hi, lo in 0..15) has entries 16 hi and
    16 lo (multiples of 16 up to 240: four significand bits), q = 128 (16 e0 + e1): the scores are 2048 j / sqrt(hd), at least
    128 apart, so the last visible key gets exp(0) = 1 and the rest underflow to 0.  V goes through kv8_ref first."""
    assert kvl <= 256
    g = torch.Generator().manual_seed(4000 + seed)
    q = torch.zeros(H, hd)
    q[:, 0], q[:, 1] = 128.0 * 16.0, 128.0
    j = torch.arange(kvl)
    k = torch.zeros(H, kvl, hd)
    k[:, :, 0], k[:, :, 1] = (j // 16).float() * 16.0, (j % 16).float() * 16.0
    v = torch.randn(H, kvl, hd, generator=g).to(dtype)
    k = k.to(dtype)
    kq, ks, kb = kv8_ref.quantize(k)
    assert torch.equal(kb, k)
    return q.to(dtype), k, kv8_ref.quantize(v)[2]


@pytest.mark.parametrize("dtype", D16, ids=dname)
@pytest.mark.parametrize("hd", [64, 128])
def test_attn_decode_kv8_exact_probe(ops, hd, dtype):
    H, cap = KC.DECODE_HEADS, 256
    for kvl in (1, 17, 255, 256):
        q, k, v = kv8_selector(kvl, hd, dtype, H, kvl)
        kc, vc = torch.zeros(H, cap, hd, dtype=dtype), torch.zeros(H, cap, hd, dtype=dtype)
        kc[:, :kvl], vc[:, :kvl] = k, v
        planes, kb, vb = shadow_planes(kc, vc, kvl)
        assert torch.equal(vb, v)
        n = torch.tensor([kvl], dtype=torch.int32, device=DEV)
        for ns in (0, 4, 32):
            what = "attn_decode_kv8 selector hd %d %s nsplit %d kv_len %d" % (hd, dname(dtype), ns, kvl)
            with knobs(attn_decode_nsplit=ns):
                g = guarded(1, H * hd, dtype)
                ops.attn_decode_kv8(dev(q.reshape(H * hd)), *planes, n, out=g.view(H * hd))
                assert torch.equal(g.check(what).view(H, hd), v[:, kvl - 1]), what
