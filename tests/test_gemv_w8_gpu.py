"""fp8 (OCP e4m3fn) weight-only decode projection, ss_gemv_w8: y[b][n] = epilogue(s[n] * sum_k dec(Wq[n, k]) * x[b][k]).

Element-wise a-priori bounds against fp64 on s * dec(q) * x (kernel_check.py's notation), derived, not tuned:
  * dec(q) has 4 significand bits, x 8 (bf16) or 11 (fp16): every product is exact in fp32, so the accumulator obeys
    kernel_check.accumulate's bound, 2 K u32 |x| @ |dec(q)|^T;
  * the row scale is ONE fp32 multiply on the finished sum: v -> s v, t -> s t, then kernel_check.op32;
  * then kernel_check.epilogue (bias in fp32, round, residual, round), or for the SiLU pair the rounding points of
    kernel_check.silu_mul_bound with the gate and up rows scaled by their own s;
  * with the RMSNorm prologue the activations carry an error of their own (rmsnorm_inputs below, the derivation of
    tests/test_kernel_edges_gpu.py restated), which enters the accumulator's bound as t_x @ |dec(q)|^T.
Shapes are the smallest that reach each code path: (33, 16) one pack and one valid lane chunk; (100, 272) 17 packs, a ragged last
load, generic form; (37, 4096) the 16-step stream loop with a clamped last tile; (40, 11008) the packed 43-step loop (<= 8
sequences per sweep: 16 run as two sweeps, and it has no RMSNorm prologue: that call must refuse).  Outputs sit in guarded
buffers; the allocation tails of Wq (0x7f bytes: NaN in e4m3fn), of the scales and of x (NaN / +Inf) are poisoned, so an
over-read shows as a NaN, not as a fault.
Exact probes: every one of the 254 non-NaN codes at selected k (both MFMA steps of a load, the first and last k of every wave
slice, the 8-byte tail load of the 43-step form) with power-of-two scales, and an integer probe whose partial sums are exact."""
import pytest
import torch

import kernel_check as KC
from test_kernel_edges_gpu import DEV, D16, dev, dname, guarded, knobs, ops, padded  # noqa: F401  (ops: fixture)

pytestmark = pytest.mark.gpu

W8_SHAPES = [(33, 16), (100, 272), (37, 4096), (40, 11008)]
W8_NB = [1, 2, 3, 8, 16]
F8 = torch.float8_e4m3fn


def dec(q):
    """uint8 codes -> fp64 values (CPU)"""
    return q.view(F8).double()


def quantize(w):
    """w [N, K] float (CPU) -> (q uint8 [N, K], s fp32 [N] = amax / 448): the recipe of ops.quantize_weight_rows_fp8"""
    s = (w.float().abs().amax(dim=1) / 448.0).clamp_min(2.0 ** -100)
    q = (w.float() / s[:, None]).clamp(-448.0, 448.0).to(F8).view(torch.uint8)
    assert not ((q & 0x7f) == 0x7f).any()
    return q, s


def w8_inputs(nb, N, K, dtype, seed):
    x, w = KC.gemm_inputs(nb, N, K, dtype, seed)
    q, s = quantize(w)
    return x, q, s


def padded_q(q, extra_rows=3):
    """the byte plane as the head of a longer allocation whose tail is 0x7f (NaN in e4m3fn)"""
    buf = torch.full((q.shape[0] + extra_rows, q.shape[1]), 0x7f, dtype=torch.uint8)
    buf[:q.shape[0]] = q
    return dev(buf)[:q.shape[0]]


def padded_s(s, extra=8):
    buf = torch.empty(s.numel() + extra, dtype=torch.float32)
    buf[:s.numel()] = s
    KC.poison_(buf[s.numel():])
    return dev(buf)[:s.numel()]


def scaled_acc(x, q, s, tx=None):
    """(v, t) of s[n] * sum_k dec(q)[n, k] x[b, k] as the kernel forms it; tx: error bound of the activations (RMSNorm)"""
    wd = dec(q)
    v, t = KC.accumulate(x, wd)
    if tx is not None:
        t = t + (1.0 + 2.0 * x.shape[1] * KC.U32) * (tx @ wd.abs().t())
    sd = s.double()[None, :]
    return KC.op32(v * sd, t * sd)


def w8_bound(x, q, s, dtype, tx=None, **epi):
    v, t = scaled_acc(x, q, s, tx)
    return KC.epilogue(v, t, dtype, **epi)


def w8_silu_bound(x, q, s, dtype):
    """q [2I, K] = [gate; up]: round(round(silu(round(g))) * round(u)) with g, u the scaled sums"""
    v, t = scaled_acc(x, q, s)
    v, t = KC.mid_round(v, t, dtype)
    I = q.shape[0] // 2
    sv, st = KC.silu(v[:, :I], t[:, :I], dtype)
    sv, st = KC.mid_round(sv, st, dtype)
    v, t = KC.product(v[:, I:], t[:, I:], sv, st)
    return KC.final_round(v, t, dtype)


def rmsnorm_inputs(x, K, dtype, seed):
    """(gain [K] of the model dtype, fp64 reference of the RMS-normalised activations, bound of their error).
    The kernels form rstd = 1 / sqrt(sum x^2 / K + eps) in fp32 (K positive terms, then a division, an addition, a square root
    and a reciprocal: relative error <= (K + 8) u32 together with the product x * rstd), round x * rstd to T, multiply by the gain
    in fp32 and round to T again when the pack is formed."""
    g = torch.Generator().manual_seed(8000 + seed)
    gain = (1.0 + 0.1 * torch.randn(K, generator=g)).to(dtype)
    xd = x.double()
    v = xd / torch.sqrt((xd * xd).mean(dim=1, keepdim=True) + 1e-5)
    v, t = KC.mid_round(v, (K + 8) * KC.U32 * v.abs(), dtype)
    v, t = KC.product(v, t, gain.double().expand_as(v), torch.zeros_like(v))
    v, t = KC.mid_round(v, t, dtype)
    return gain, v, t


def run_variants(ops, N, K, nb, dtype, what, family):
    from seedstory._lib import SSError
    seed = N + K + nb
    x, q, s = w8_inputs(nb, N, K, dtype, seed)
    kw = KC.epilogue_inputs("bias+residual", nb, N, dtype, seed)
    gain, xn, tx = rmsnorm_inputs(x, K, dtype, seed)
    qd, sd, xd = padded_q(q), padded_s(s), padded(x, 1)
    g = guarded(nb, N, dtype)
    ops.gemv_w8(qd, sd, xd, out=g.out)
    KC.check(g.check(what), *w8_bound(x, q, s, dtype), what, family=family, dtype=dtype)
    g = guarded(nb, N, dtype)
    ops.gemv_w8(qd, sd, xd, bias=dev(kw["bias"]), residual=dev(kw["residual"]), out=g.out)
    KC.check(g.check(what), *w8_bound(x, q, s, dtype, **kw), what + " bias+residual", family=family, dtype=dtype)
    if K == 11008:          # the packed form has no RMSNorm prologue: refused before a launch
        with pytest.raises(SSError, match="RMSNorm"):
            ops.gemv_w8(qd, sd, xd, norm_w=dev(gain), eps=1e-5)
    else:
        g = guarded(nb, N, dtype)
        ops.gemv_w8(qd, sd, xd, norm_w=dev(gain), eps=1e-5, out=g.out)
        KC.check(g.check(what), *w8_bound(xn, q, s, dtype, tx=tx), what + " rmsnorm", family=family, dtype=dtype)
    for I in (24, 40):
        xs, qs, ss = w8_inputs(nb, 2 * I, K, dtype, seed + I)
        g = guarded(nb, I, dtype)
        ops.gemv_w8(padded_q(qs), padded_s(ss), padded(xs, 1), silu_mul=True, out=g.out)
        KC.check(g.check(what), *w8_silu_bound(xs, qs, ss, dtype), what + " silu_mul I %d" % I, family=family + " silu_mul", dtype=dtype)


@pytest.mark.parametrize("dtype", D16, ids=dname)
@pytest.mark.parametrize("N,K", W8_SHAPES)
def test_gemv_w8_bound_poison(ops, N, K, dtype):
    """plain, bias + residual, RMSNorm prologue and the SiLU pair at 1 / 2 / 3 / 8 / 16 sequences; (37, 4096) also through the
    predicated kernel (gemv_mfma_generic = 1); the batch-1 call with a 1-D x"""
    for nb in W8_NB:
        for generic in ((0, 1) if K == 4096 else (0,)):
            with knobs(gemv_mfma_generic=generic):
                run_variants(ops, N, K, nb, dtype, "gemv_w8 %s %s nb %d generic %d" % ((N, K), dname(dtype), nb, generic), "gemv_w8")
    x, q, s = w8_inputs(1, N, K, dtype, N + K)
    g = guarded(1, N, dtype)
    ops.gemv_w8(padded_q(q), padded_s(s), padded(x, 1)[0], out=g.view(N))
    KC.check(g.check("1-D x"), *w8_bound(x, q, s, dtype), "gemv_w8 1-D x %s" % ((N, K),), family="gemv_w8", dtype=dtype)


@pytest.mark.parametrize("dtype", D16, ids=dname)
def test_gemv_w8_multi_tile_bound(ops, dtype):
    """gemv_mfma_blocks = 2: every persistent workgroup walks several row tiles (two register buffers, LDS parity, the prefetch
    across the tile boundary; I = 40: three tiles on two workgroups), at the sizes of the other test"""
    with knobs(gemv_mfma_blocks=2):
        for (N, K) in W8_SHAPES[1:]:
            for nb in (1, 8, 16):
                run_variants(ops, N, K, nb, dtype, "gemv_w8 multi-tile %s %s nb %d" % ((N, K), dname(dtype), nb), "gemv_w8 multi-tile")


def probe_positions(K):
    """k positions of the one-hot activations: kernel_check.boundary_indices (both sides of every multiple of 32 / 64 / 128: the
    first and last k of every load, lane chunk pair and wave slice), both sides of every multiple of 8 (the two MFMA steps of a
    load, the lane chunks) in the first and last 128 k, and for K = 11008 the 32 k of the first and last wave's 8-byte tail load"""
    s = set(KC.boundary_indices(K))
    for lo in (0, max(K - 128, 0)):
        for b in range(lo, min(lo + 128, K), 8):
            s.update((b, min(b + 7, K - 1)))
    if K == 11008:
        for w in (0, 7):
            s.update(range(w * 1376 + 1344, w * 1376 + 1376))
    return sorted(s)


CODES = torch.tensor([c for c in range(256) if (c & 0x7f) != 0x7f], dtype=torch.uint8)       # the 254 non-NaN codes


@pytest.mark.parametrize("dtype", D16, ids=dname)
@pytest.mark.parametrize("N,K", [(254, 16), (254, 272), (254, 4096), (254, 11008)])
def test_gemv_w8_every_code_exact(ops, N, K, dtype):
    """Wq[n, k] = code (n + k) mod 254: every row meets every code, every k holds another code of a row.  x[b] is one-hot at k =
    pi(b), the scales are powers of two: y[b][n] must EQUAL dec(Wq[n, pi(b)]) * s[n] (exact in bf16 and fp16).  Pins the
    conversion instruction and the k <-> lane mapping of both MFMA steps of a load."""
    n_i, k_i = torch.arange(N)[:, None], torch.arange(K)[None, :]
    q = CODES[(n_i + k_i) % CODES.numel()]
    s = 2.0 ** ((torch.arange(N) % 5) - 2).float()
    pos = probe_positions(K)
    qd, sd = padded_q(q), padded_s(s)
    wv = dec(q) * s.double()[:, None]
    for generic in ((0, 1) if K == 4096 else (0,)):
        with knobs(gemv_mfma_generic=generic):
            for i0 in range(0, len(pos), 16):
                pi = torch.tensor(pos[i0:i0 + 16])
                nb = pi.numel()
                x = torch.zeros(nb, K, dtype=dtype)
                x[torch.arange(nb), pi] = 1.0
                g = guarded(nb, N, dtype)
                ops.gemv_w8(qd, sd, padded(x, 1), out=g.out)
                exp = wv[:, pi].t().to(dtype)
                assert torch.equal(exp.double(), wv[:, pi].t())             # the expectation itself is exact in T
                got = g.check("every code")
                assert torch.equal(got, exp), "K %d generic %d positions %s: %d mismatches" % (
                    K, generic, pi.tolist(), int((got != exp).sum()))
            x = torch.zeros(1, K, dtype=dtype)                             # one sequence, the last k
            x[0, K - 1] = 1.0
            g = guarded(1, N, dtype)
            ops.gemv_w8(qd, sd, padded(x, 1), out=g.out)
            assert torch.equal(g.check("every code nb 1"), wv[:, K - 1:].t().to(dtype))


@pytest.mark.parametrize("dtype", D16, ids=dname)
@pytest.mark.parametrize("N,K", W8_SHAPES)
def test_gemv_w8_integer_probe(ops, N, K, dtype):
    """weights in {-4 .. 4}, activations in {-3 .. 3}, scale 2: every fp32 partial sum is an exact integer (<= 12 K < 2^24), so
    the result is round_T(2 * sum) whatever the accumulation order; a k taken twice or not at all changes the integer"""
    gen = torch.Generator().manual_seed(N * 7 + K)
    for nb in W8_NB:
        wi = torch.randint(-4, 5, (N, K), generator=gen).float()
        q = wi.to(F8).view(torch.uint8)
        assert torch.equal(dec(q), wi.double())
        x = torch.randint(-3, 4, (nb, K), generator=gen).to(dtype)
        s = torch.full((N,), 2.0)
        g = guarded(nb, N, dtype)
        ops.gemv_w8(padded_q(q), padded_s(s), padded(x, 1), out=g.out)
        exp = (2.0 * (x.double() @ wi.double().t())).to(dtype)
        assert torch.equal(g.check("integer probe"), exp), "integer probe %s nb %d" % ((N, K), nb)


def test_gemv_w8_refuses_bad_shapes(ops):
    from seedstory._lib import SSError
    mk = lambda N, K, dt=torch.bfloat16, nb=2: (dev(torch.zeros(N, K, dtype=torch.uint8)), dev(torch.ones(N)), dev(torch.zeros(nb, K, dtype=dt)))  # noqa: E731
    for K in (24, 4112, 8192):              # not a multiple of 16; past 4096 and not 11008
        with pytest.raises(SSError, match="gemv_w8"):
            ops.gemv_w8(*mk(32, K))
    with pytest.raises(SSError):            # fp32 activations
        ops.gemv_w8(*mk(32, 64, torch.float32))
    with pytest.raises(SSError, match="gemv_w8"):
        ops.gemv_w8(*mk(32, 64, nb=17))
    q, s, x = mk(32, 64)
    with pytest.raises(SSError, match="SILU_MUL"):
        ops.gemv_w8(q, s, x, silu_mul=True, bias=dev(torch.zeros(16, dtype=torch.bfloat16)))


def test_quantize_weight_rows_fp8(ops):
    """the wrapper over ss_quantize_rows_fp8: scale = amax / 448, codes = RNE_e4m3(w / scale); an all-zero row gets a finite scale
    and a zero output; gemv_w8 on the result stays within e4m3's half-ulp (2^-4 relative per weight) of the 16-bit product"""
    g = torch.Generator().manual_seed(5)
    w = (torch.randn(48, 256, generator=g) * 0.05).to(torch.bfloat16)
    w[7] = 0
    q, s = ops.quantize_weight_rows_fp8(dev(w))
    q, s = q.cpu(), s.cpu()
    assert q.dtype == torch.uint8 and tuple(q.shape) == (48, 256) and s.dtype == torch.float32 and tuple(s.shape) == (48,)
    assert torch.isfinite(s).all() and not ((q & 0x7f) == 0x7f).any()
    amax = w.float().abs().amax(dim=1)
    assert ((s - amax / 448.0).abs() <= 2.0 ** -22 * s).all()        # one fp32 division: within 2 ulp of torch's
    assert float(s[7]) == 0.0 and not q[7].any()
    back = dec(q) * s.double()[:, None]
    assert ((back - w.double()).abs() <= 2.0 ** -4 * w.double().abs() + s.double()[:, None] * 2.0 ** -10).all()
    x = torch.randn(2, 256, generator=g).to(torch.bfloat16)
    y = ops.gemv_w8(dev(q), dev(s), dev(x)).cpu()
    assert torch.isfinite(y).all() and not y[:, 7].any()


def test_zz_w8_worst_ratios():
    print("\n" + KC.worst_table())
