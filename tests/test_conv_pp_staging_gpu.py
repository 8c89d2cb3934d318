"""The A-operand staging of the ping-pong conv3x3 tiles (ss_gemm_pp.inc, CONV): per-piece offsets and padding masks formed once
per output tile, the tap offset once per tap, one bit test + one scalar add + one DMA per piece and K tile.  The shapes are the
smallest that reach every branch of it (see CASES); every ping-pong conv tile, bf16 and fp16, four epilogue forms, is compared
bit for bit with the one-barrier tile 69 (same k order), over three launches, and once with F.conv2d in fp32."""
import math

import pytest
import torch
import torch.nn.functional as F

import kernel_check as KC
import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (B, Ci, Co, H, W); Co is given for the 320-wide tile, the 256-wide tiles take 256 / 512 in its place
CASES = [
    (8, 64, 320, 4, 8),       # M = 256: eight images in one tile; W = 8: every piece is the left AND the right border; one K tile per
                              # tap (the tap changes every K tile); top and bottom rows in every image
    (2, 64, 640, 16, 8),      # two N tiles, W = 8
    (1, 128, 320, 16, 16),    # two K tiles per tap; pieces alternate between the left and the right border
    (1, 1280, 320, 8, 32),    # 20 K tiles per tap (K = 11520); interior pieces exist
    (4, 192, 640, 8, 8),      # three K tiles per tap: an odd count of K tiles (27)
]
BN = {54: 256, 55: 256, 56: 320, 57: 256}
assert sorted(BN) == sorted(KC.CONV_PP_TILES)

_OPERANDS = {}   # (case, Co, dtype) -> host operands and the fp32 references of the four forms (computed once, never written)


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def nhwc(x):  # [B,C,H,W] -> [B*H*W, C]
    B, C, H, W = x.shape
    return x.permute(0, 2, 3, 1).reshape(B * H * W, C).contiguous()


def nchw(y, B, H, W):
    return y.reshape(B, H, W, -1).permute(0, 3, 1, 2)


def operands(B, Ci, Co, H, W, dtype):
    key = (B, Ci, Co, H, W, dtype)
    if key not in _OPERANDS:
        x = synth.normal_like(231, (B, Ci, H, W), 1.0, dtype=dtype)
        w = synth.normal_like(232, (Co, Ci, 3, 3), 1.0 / math.sqrt(9 * Ci), dtype=dtype)
        b = synth.normal_like(233, (Co,), 0.5, dtype=dtype)
        tv = synth.normal_like(234, (B, Co), 0.5, dtype=dtype)
        res = synth.normal_like(235, (B, Co, H, W), 1.0, dtype=dtype)
        conv = F.conv2d(x.float(), w.float(), None, padding=1)
        cb = conv + b.float()[None, :, None, None]
        rv = tv.float()[:, :, None, None]
        refs = [conv, cb + rv, cb + res.float(), conv + rv]
        _OPERANDS[key] = (x, w, b, tv, res, refs)
    return _OPERANDS[key]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("cfg", KC.CONV_PP_TILES)
@pytest.mark.parametrize("B,Ci,Co,H,W", CASES)
def test_conv_pp_staging(B, Ci, Co, H, W, cfg, dtype):
    from seedstory import _lib, ops
    from seedstory.diffusion import _conv_w
    if BN[cfg] == 256:
        Co = Co // 320 * 256
        # the rule of pp_launch for the 256-wide tiles (KC.conv_pp320_eligible with the tile width replaced)
        assert KC.conv_pp320_eligible(B, Ci, Co // 256 * 320, H, W, 1, False) and Co % 256 == 0
    else:
        assert KC.conv_pp320_eligible(B, Ci, Co, H, W, 1, False)
    x, w, b, tv, res, refs = operands(B, Ci, Co, H, W, dtype)
    xd, wd_, bd, tvd, rd = nhwc(x).to(DEV), _conv_w(w).to(DEV), b.to(DEV), tv.to(DEV), nhwc(res).to(DEV)

    def run():   # plain | bias + rowvec | bias + residual | rowvec only
        return [ops.conv3x3(xd, wd_, B, H, W)[0], ops.conv3x3(xd, wd_, B, H, W, bias=bd, rowvec=tvd)[0],
                ops.conv3x3(xd, wd_, B, H, W, bias=bd, residual=rd)[0], ops.conv3x3(xd, wd_, B, H, W, rowvec=tvd)[0]]
    try:
        _lib.set_tuning("gemm_cfg", 69)
        y69 = run()
        _lib.set_tuning("gemm_cfg", cfg)
        outs = [run() for _ in range(3)]
    finally:
        _lib.set_tuning("gemm_cfg", 0)
    for y, r in zip(outs[0], refs):
        assert rel(nchw(y.cpu(), B, H, W), r) < 1e-2
    for o in outs:
        for y, r in zip(o, y69):
            assert torch.equal(y, r)
