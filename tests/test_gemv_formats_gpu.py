"""The three weight formats of the MFMA decode projection are one algorithm (one shared predicated tile loop, a stream loop per
format in ss_gemv.hip); on integers they must agree exactly.  Weights in {-4 .. 4} are exact in bf16 / fp16, in e4m3 and in e2m1
under scale byte 127, activations are in {-3 .. 3}: every fp32 partial sum is an exact integer (<= 12 K < 2^24), so ops.gemv_batched (gemv_mfma_min_nb = 1: the MFMA
kernels at every sequence count), ops.gemv_w8 with unit row scales and ops.gemv_mx4 must return the SAME tensor, round_T of the
fp64 sum, whatever order each format walks k in; a k taken twice, not at all or under another lane's activation changes the integer.
Shapes: (33, 32) the partial last load, (100, 288) a partial wave slice, (37, 4096) the 16-step stream loop with a partial row tile
(also through the predicated kernel, gemv_mfma_generic = 1), (40, 11008) the packed loop with fp8's 8-byte tail and MXFP4's dead
slot.  The SiLU pair ([gate; up] rows, even row counts) runs the same device epilogue on the same integers: the three outputs are
identical and obey kernel_check's bound for round(round(silu(round g)) * round u) around the exact sums."""
import pytest
import torch

import kernel_check as KC
import mxfp4_ref as R
from test_kernel_edges_gpu import D16, dev, dname, guarded, knobs, ops  # noqa: F401  (ops: fixture)

pytestmark = pytest.mark.gpu

SHAPES = [(33, 32), (100, 288), (37, 4096), (40, 11008)]
NBS = [1, 3, 8, 16]
F8 = torch.float8_e4m3fn


def planes(wi):
    """integer weights [rows, K] -> ((16-bit,), (e4m3 codes, unit scales), (e2m1 codes, scale bytes 127)), each asserted to decode
    back to wi on the CPU"""
    q8 = wi.float().to(F8).view(torch.uint8)
    assert torch.equal(q8.view(F8).double(), wi.double())
    c4 = R.round_codes(wi.double())
    X = torch.zeros(wi.shape[0], wi.shape[1] // 32, dtype=torch.int64)
    assert torch.equal(R.decode(c4, X), wi.double())
    cu, su = R.pack(c4, X)
    assert int(su.min()) == 127 and int(su.max()) == 127
    return q8, torch.ones(wi.shape[0]), cu, su


def silu_bound(v, dtype):
    v, t = KC.mid_round(v, torch.zeros_like(v), dtype)
    I = v.shape[1] // 2
    sv, st = KC.silu(v[:, :I], t[:, :I], dtype)
    sv, st = KC.mid_round(sv, st, dtype)
    return KC.final_round(*KC.product(v[:, I:], t[:, I:], sv, st), dtype)


@pytest.mark.parametrize("dtype", D16, ids=dname)
@pytest.mark.parametrize("N,K", SHAPES)
def test_gemv_formats_agree_on_integers(ops, N, K, dtype):
    gen = torch.Generator().manual_seed(N * 11 + K)
    for silu in (False, True):
        rows = N + N % 2 if silu else N                 # [gate; up]: 34, 100, 38, 40 rows
        n_out = rows // 2 if silu else rows
        wi = torch.randint(-4, 5, (rows, K), generator=gen)
        w16 = wi.to(dtype)
        assert torch.equal(w16.double(), wi.double())
        q8, s8, c4, s4 = planes(wi)
        w16, q8, s8, c4, s4 = (dev(t) for t in (w16, q8, s8, c4, s4))
        for nb in NBS:
            x = torch.randint(-3, 4, (nb, K), generator=gen).to(dtype)
            exact = x.double() @ wi.double().t()
            assert float(exact.abs().max()) < 2 ** 24
            xd = dev(x)
            for generic in ((0, 1) if K == 4096 else (0,)):
                what = "%s %s nb %d silu %d generic %d" % ((rows, K), dname(dtype), nb, silu, generic)
                with knobs(gemv_mfma_min_nb=1, gemv_mfma_generic=generic):
                    got = {}
                    for name, call in (("16-bit", lambda o: ops.gemv_batched(w16, xd, silu_mul=silu, out=o)),
                                       ("fp8", lambda o: ops.gemv_w8(q8, s8, xd, silu_mul=silu, out=o)),
                                       ("mxfp4", lambda o: ops.gemv_mx4(c4, s4, xd, silu_mul=silu, out=o))):
                        g = guarded(nb, n_out, dtype)
                        call(g.out)
                        got[name] = g.check("%s %s" % (name, what))
                for name in ("fp8", "mxfp4"):
                    KC.check_exact(got[name], got["16-bit"], "%s against 16-bit, %s" % (name, what))
                if silu:        # (|silu(g) * u| reaches 1e5: past fp16's range the identity above is the whole check)
                    v, t = silu_bound(exact, dtype)
                    fits = (v.abs() + t) < torch.finfo(dtype).max
                    zero, one = torch.zeros_like(v), torch.ones_like(v)
                    KC.check(torch.where(fits, got["16-bit"].double(), zero), torch.where(fits, v, zero), torch.where(fits, t, one), "silu pair " + what)
                else:
                    KC.check_exact(got["16-bit"], exact.to(dtype), "rounded fp64 sum, " + what)
