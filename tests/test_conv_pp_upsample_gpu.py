"""The ping-pong conv3x3 tiles with a nearest-2x upsampled input (ss_gemm_pp.inc, CONV && UP; the source offsets and padding
masks are ss_conv_up.h, walked on the host by test_conv_up_addr.py), and the two-super-phase 320-wide tile (cfg 58) as a
stride-1 convolution.  Every tile is compared bit for bit with the one-barrier tile 69 (same k order: tap-major, 64 channels per
K tile), over three launches, bf16 and fp16, four epilogue forms, and once with F.conv2d in fp32."""
import math

import pytest
import torch
import torch.nn.functional as F

import synth
from test_conv_pp_staging_gpu import CASES as S1_CASES, nchw, nhwc, operands as s1_operands, rel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (B, Ci, Co, H_in, W_in), output 2H x 2W; Co is given for the 320-wide tile, the 256-wide tiles take 256 / 512 in its place
UP_CASES = [
    (8, 64, 320, 2, 4),       # M = 256: eight images in one tile; output W = 8: every piece is the left AND the right border; top and
                              # bottom rows in every image; one K tile per tap
    (2, 64, 640, 8, 4),       # two N tiles
    (1, 128, 320, 8, 8),      # two K tiles per tap; pieces alternate between the left and the right border
    (1, 1280, 320, 4, 16),    # 20 K tiles per tap; interior pieces
    (4, 192, 640, 4, 4),      # an odd count of K tiles (27)
    (1, 64, 320, 16, 16),     # M = 1024: four M tiles, tile boundaries on even and on odd output rows
]
# the ping-pong tiles that take an upsampled input (no persistent 55, no two-super-phase 320-wide 58: see gemm_pp_dispatch)
UP_TILES = {54: 256, 56: 320, 57: 256}

_OPERANDS = {}   # (case, Co, dtype) -> host operands and the fp32 references of the four forms (computed once, never written)


def up_pp_eligible(B, Ci, Co, H, W, bn):
    """pp_launch's rule for conv_up (ss_gemm_pp.inc), a hand copy: stride 1, OUTPUT W a power of two >= 8, output H a power of two,
    whole tiles, <= 64 K tiles per tap, 32-bit byte offsets on the SOURCE (M / 4 pixels) and on a tile's weight rows"""
    Ho, Wo = 2 * H, 2 * W
    M = B * Ho * Wo
    return (Ci % 64 == 0 and Ci <= 4096 and Wo >= 8 and Wo & (Wo - 1) == 0 and Ho & (Ho - 1) == 0 and M % 256 == 0 and Co % bn == 0
            and (M // 4) * Ci * 2 < 2 ** 31 and bn * 9 * Ci * 2 < 2 ** 31)


def s1_pp320_eligible(B, Ci, Co, H, W):
    """the same rule for a stride-1 convolution on a 320-wide tile"""
    M = B * H * W
    return (Ci % 64 == 0 and Ci <= 4096 and W >= 8 and W & (W - 1) == 0 and H & (H - 1) == 0 and M % 256 == 0 and Co % 320 == 0
            and M * Ci * 2 < 2 ** 31 and 320 * 9 * Ci * 2 < 2 ** 31)


def up_operands(B, Ci, Co, H, W, dtype):
    key = (B, Ci, Co, H, W, dtype)
    if key not in _OPERANDS:
        x = synth.normal_like(241, (B, Ci, H, W), 1.0, dtype=dtype)
        w = synth.normal_like(242, (Co, Ci, 3, 3), 1.0 / math.sqrt(9 * Ci), dtype=dtype)
        b = synth.normal_like(243, (Co,), 0.5, dtype=dtype)
        tv = synth.normal_like(244, (B, Co), 0.5, dtype=dtype)
        res = synth.normal_like(245, (B, Co, 2 * H, 2 * W), 1.0, dtype=dtype)
        conv = F.conv2d(F.interpolate(x.float(), scale_factor=2, mode="nearest"), w.float(), None, padding=1)
        cb = conv + b.float()[None, :, None, None]
        rv = tv.float()[:, :, None, None]
        _OPERANDS[key] = (x, w, b, tv, res, [conv, cb + rv, cb + res.float(), conv + rv])
    return _OPERANDS[key]


def _compare(cfg, ops_, refs, B, Ho, Wo):
    """ops_: the four launches (plain | bias + rowvec | bias + residual | rowvec only) as one callable"""
    from seedstory import _lib
    try:
        _lib.set_tuning("gemm_cfg", 69)
        y69 = ops_()
        _lib.set_tuning("gemm_cfg", cfg)
        outs = [ops_() for _ in range(3)]
    finally:
        _lib.set_tuning("gemm_cfg", 0)
    for y, r in zip(outs[0], refs):
        e = rel(nchw(y.cpu(), B, Ho, Wo), r)
        print("cfg %d rel %.3e" % (cfg, e))
        assert e < 1e-2
    for o in outs:
        for y, r in zip(o, y69):
            assert torch.equal(y, r)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("cfg", sorted(UP_TILES))
@pytest.mark.parametrize("B,Ci,Co,H,W", UP_CASES)
def test_conv_pp_upsample(B, Ci, Co, H, W, cfg, dtype):
    from seedstory import ops
    from seedstory.diffusion import _conv_w
    if UP_TILES[cfg] == 256:
        Co = Co // 320 * 256
    assert up_pp_eligible(B, Ci, Co, H, W, UP_TILES[cfg])
    x, w, b, tv, res, refs = up_operands(B, Ci, Co, H, W, dtype)
    xd, wd_, bd, tvd, rd = nhwc(x).to(DEV), _conv_w(w).to(DEV), b.to(DEV), tv.to(DEV), nhwc(res).to(DEV)

    def run():
        kw = dict(upsample=True)
        return [ops.conv3x3(xd, wd_, B, H, W, **kw)[0], ops.conv3x3(xd, wd_, B, H, W, bias=bd, rowvec=tvd, **kw)[0],
                ops.conv3x3(xd, wd_, B, H, W, bias=bd, residual=rd, **kw)[0], ops.conv3x3(xd, wd_, B, H, W, rowvec=tvd, **kw)[0]]
    _compare(cfg, run, refs, B, 2 * H, 2 * W)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("B,Ci,Co,H,W", S1_CASES)
def test_conv_pp58_stride1(B, Ci, Co, H, W, dtype):
    """cfg 58 (<320, 12, true>) as a stride-1 convolution, on the shapes of test_conv_pp_staging_gpu.py"""
    from seedstory import ops
    from seedstory.diffusion import _conv_w
    assert s1_pp320_eligible(B, Ci, Co, H, W)
    x, w, b, tv, res, refs = s1_operands(B, Ci, Co, H, W, dtype)
    xd, wd_, bd, tvd, rd = nhwc(x).to(DEV), _conv_w(w).to(DEV), b.to(DEV), tv.to(DEV), nhwc(res).to(DEV)

    def run():
        return [ops.conv3x3(xd, wd_, B, H, W)[0], ops.conv3x3(xd, wd_, B, H, W, bias=bd, rowvec=tvd)[0],
                ops.conv3x3(xd, wd_, B, H, W, bias=bd, residual=rd)[0], ops.conv3x3(xd, wd_, B, H, W, rowvec=tvd)[0]]
    _compare(58, run, refs, B, H, W)
