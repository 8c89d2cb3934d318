"""MXFP4 weight-only decode projection, ss_gemv_mx4: y[b][n] = epilogue(sum_k dec(code[n, k]) * 2^X[n, k / 32] * x[b][k]).

Element-wise a-priori bounds against fp64 on dec * 2^X * x (kernel_check.py's notation), derived, not tuned:
  * dec * 2^X has 2 significand bits and is exact in the model dtype for X in [-13, 13]; x has 8 (bf16) or 11 (fp16): every product
    is exact in fp32, so the accumulator obeys kernel_check.accumulate's bound on x and dec * 2^X, 2 K u32 |x| @ |w|^T.  There is
    no row scale and no multiply behind the sum;
  * then kernel_check.epilogue (bias in fp32, round, residual, round), or for the SiLU pair the rounding points of
    kernel_check.silu_mul_bound;
  * with the RMSNorm prologue the activations carry an error of their own (test_gemv_w8_gpu.rmsnorm_inputs), which enters the
    accumulator's bound as t_x @ |w|^T.
Shapes are the smallest that reach each code path: (33, 32) one block, one valid lane group; (100, 288) nine blocks, a ragged last
load across the lane groups, generic form; (37, 4096) the 4-load stream loop with a clamped last tile, also through the predicated
kernel (gemv_mfma_generic = 1); (40, 11008) the packed 11-slot loop whose waves 6 and 7 own ten loads (<= 8 sequences per sweep: 16
run as two sweeps, and it has no RMSNorm prologue: that call must refuse).  Outputs sit in guarded buffers; the allocation tail
of the codes is 0x77, of the scales 0xFF (NaN in e8m0), of x NaN / +Inf, so an over-read shows as a non-finite output, not as a
fault.
Exact probes: every code in both nibbles of every byte at selected k under block exponents that differ between neighbouring
blocks and rows, and an integer probe whose partial sums are exact.  The quantiser kernel against tests/mxfp4_ref.py bit for bit."""
import pytest
import torch

import kernel_check as KC
import mxfp4_ref as R
from test_gemv_w8_gpu import rmsnorm_inputs
from test_kernel_edges_gpu import DEV, D16, dev, dname, guarded, knobs, ops, padded  # noqa: F401  (ops: fixture)

pytestmark = pytest.mark.gpu

MX4_SHAPES = [(33, 32), (100, 288), (37, 4096), (40, 11008)]
MX4_NB = [1, 2, 3, 8, 16]


def mx4_inputs(nb, N, K, dtype, seed):
    """(x, codes uint8 [N, K / 2], scales uint8 [N, K / 32], fp64 de-quantised weights)"""
    x, w = KC.gemm_inputs(nb, N, K, dtype, seed)
    cu, su, wd = R.quantize_packed(w)
    assert torch.equal(wd.to(dtype).double(), wd)
    return x, cu, su, wd


def padded_bytes(t, fill, extra_rows=3):
    """a byte plane as the head of a longer allocation whose tail holds `fill`"""
    buf = torch.full((t.shape[0] + extra_rows, t.shape[1]), fill, dtype=torch.uint8)
    buf[:t.shape[0]] = t
    return dev(buf)[:t.shape[0]]


def planes(cu, su):
    return padded_bytes(cu, 0x77), padded_bytes(su, 0xFF)


def acc(x, wd, tx=None):
    v, t = KC.accumulate(x, wd)
    if tx is not None:
        t = t + (1.0 + 2.0 * x.shape[1] * KC.U32) * (tx @ wd.abs().t())
    return v, t


def mx4_bound(x, wd, dtype, tx=None, **epi):
    return KC.epilogue(*acc(x, wd, tx), dtype, **epi)


def mx4_silu_bound(x, wd, dtype):
    """wd [2I, K] = [gate; up]: round(round(silu(round(g))) * round(u))"""
    v, t = KC.mid_round(*acc(x, wd), dtype)
    I = wd.shape[0] // 2
    sv, st = KC.silu(v[:, :I], t[:, :I], dtype)
    sv, st = KC.mid_round(sv, st, dtype)
    v, t = KC.product(v[:, I:], t[:, I:], sv, st)
    return KC.final_round(v, t, dtype)


def run_variants(ops, N, K, nb, dtype, what, family):
    from seedstory._lib import SSError
    seed = N + K + nb
    x, cu, su, wd = mx4_inputs(nb, N, K, dtype, seed)
    kw = KC.epilogue_inputs("bias+residual", nb, N, dtype, seed)
    gain, xn, tx = rmsnorm_inputs(x, K, dtype, seed)
    (cd, sd), xd = planes(cu, su), padded(x, 1)
    g = guarded(nb, N, dtype)
    ops.gemv_mx4(cd, sd, xd, out=g.out)
    KC.check(g.check(what), *mx4_bound(x, wd, dtype), what, family=family, dtype=dtype)
    g = guarded(nb, N, dtype)
    ops.gemv_mx4(cd, sd, xd, bias=dev(kw["bias"]), out=g.out)
    KC.check(g.check(what), *mx4_bound(x, wd, dtype, bias=kw["bias"]), what + " bias", family=family, dtype=dtype)
    g = guarded(nb, N, dtype)
    ops.gemv_mx4(cd, sd, xd, residual=dev(kw["residual"]), out=g.out)
    KC.check(g.check(what), *mx4_bound(x, wd, dtype, residual=kw["residual"]), what + " residual", family=family, dtype=dtype)
    g = guarded(nb, N, dtype)
    ops.gemv_mx4(cd, sd, xd, bias=dev(kw["bias"]), residual=dev(kw["residual"]), out=g.out)
    KC.check(g.check(what), *mx4_bound(x, wd, dtype, **kw), what + " bias+residual", family=family, dtype=dtype)
    if K == 11008:          # the packed form has no RMSNorm prologue: refused before a launch
        with pytest.raises(SSError, match="RMSNorm"):
            ops.gemv_mx4(cd, sd, xd, norm_w=dev(gain), eps=1e-5)
    else:
        g = guarded(nb, N, dtype)
        ops.gemv_mx4(cd, sd, xd, norm_w=dev(gain), eps=1e-5, out=g.out)
        KC.check(g.check(what), *mx4_bound(xn, wd, dtype, tx=tx), what + " rmsnorm", family=family, dtype=dtype)
    for I in (24, 40):
        xs, cs, ss, ws = mx4_inputs(nb, 2 * I, K, dtype, seed + I)
        g = guarded(nb, I, dtype)
        ops.gemv_mx4(*planes(cs, ss), padded(xs, 1), silu_mul=True, out=g.out)
        KC.check(g.check(what), *mx4_silu_bound(xs, ws, dtype), what + " silu_mul I %d" % I, family=family + " silu_mul", dtype=dtype)


@pytest.mark.parametrize("dtype", D16, ids=dname)
@pytest.mark.parametrize("N,K", MX4_SHAPES)
def test_gemv_mx4_bound_poison(ops, N, K, dtype):
    """plain, bias, residual, bias + residual, RMSNorm prologue and the SiLU pair at 1 / 2 / 3 / 8 / 16 sequences; (37, 4096) also
    through the predicated kernel (gemv_mfma_generic = 1); the batch-1 call with a 1-D x"""
    for nb in MX4_NB:
        for generic in ((0, 1) if K == 4096 else (0,)):
            with knobs(gemv_mfma_generic=generic):
                run_variants(ops, N, K, nb, dtype, "gemv_mx4 %s %s nb %d generic %d" % ((N, K), dname(dtype), nb, generic), "gemv_mx4")
    x, cu, su, wd = mx4_inputs(1, N, K, dtype, N + K)
    g = guarded(1, N, dtype)
    ops.gemv_mx4(*planes(cu, su), padded(x, 1)[0], out=g.view(N))
    KC.check(g.check("1-D x"), *mx4_bound(x, wd, dtype), "gemv_mx4 1-D x %s" % ((N, K),), family="gemv_mx4", dtype=dtype)


@pytest.mark.parametrize("dtype", D16, ids=dname)
def test_gemv_mx4_multi_tile_bound(ops, dtype):
    """gemv_mfma_blocks = 2: every persistent workgroup walks several row tiles (two register buffers, LDS parity, the prefetch
    across the tile boundary; I = 40: three tiles on two workgroups), at the sizes of the other test"""
    with knobs(gemv_mfma_blocks=2):
        for (N, K) in MX4_SHAPES[1:]:
            for nb in (1, 8, 16):
                run_variants(ops, N, K, nb, dtype, "gemv_mx4 multi-tile %s %s nb %d" % ((N, K), dname(dtype), nb), "gemv_mx4 multi-tile")


def probe_positions(K):
    """k positions of the one-hot activations: kernel_check.boundary_indices (both sides of every multiple of 32 / 64 / 128: the
    first and last k of every block, every load and every wave's range), both sides of every multiple of 8 (the four MFMA steps of
    a load) in the first and last 128 k, and for K = 11008 every k of the first and last wave's tail blocks: the 43-block slices
    of a plain split end at k = 1376 w, this kernel's ranges at 1408 w (w <= 6) and 9728: the last 128 k in front of both"""
    s = set(KC.boundary_indices(K))
    for lo in (0, max(K - 128, 0)):
        for b in range(lo, min(lo + 128, K), 8):
            s.update((b, min(b + 7, K - 1)))
    if K == 11008:
        for end in (1376, 1408, 9632, 9728, 11008):
            s.update(range(end - 128, end))
    return sorted(s)


@pytest.mark.parametrize("dtype", D16, ids=dname)
@pytest.mark.parametrize("K", [32, 288, 4096, 11008])
def test_gemv_mx4_every_code_exact(ops, K, dtype):
    """code[n, k] = (n + k) mod 16, N = 32: both nibbles of every byte meet every code.  X[n, b] = ((n + 3 b) mod 7) - 3: a scale
    byte taken from the wrong block or row changes the answer.  x[b] is one-hot at k = pi(b): y[b][n] must EQUAL
    dec(code[n, pi(b)]) * 2^X[n, pi(b) / 32] (exact in bf16 and fp16).  Pins the conversion instruction, its nibble and byte
    order and the lane <-> k <-> scale mapping of the four MFMA steps of a load."""
    N = 32
    n_i = torch.arange(N)[:, None]
    codes = (n_i + torch.arange(K)[None, :]) % 16
    X = ((n_i + 3 * torch.arange(K // 32)[None, :]) % 7) - 3
    wv = R.decode(codes, X)
    cd, sd = planes(*R.pack(codes, X))
    pos = probe_positions(K)
    for generic in ((0, 1) if K == 4096 else (0,)):
        with knobs(gemv_mfma_generic=generic):
            for i0 in range(0, len(pos), 16):
                pi = torch.tensor(pos[i0:i0 + 16])
                nb = pi.numel()
                x = torch.zeros(nb, K, dtype=dtype)
                x[torch.arange(nb), pi] = 1.0
                g = guarded(nb, N, dtype)
                ops.gemv_mx4(cd, sd, padded(x, 1), out=g.out)
                exp = wv[:, pi].t().to(dtype)
                assert torch.equal(exp.double(), wv[:, pi].t())             # the expectation itself is exact in T
                got = g.check("every code")
                assert torch.equal(got, exp), "K %d generic %d positions %s: %d mismatches" % (
                    K, generic, pi.tolist(), int((got != exp).sum()))
            x = torch.zeros(1, K, dtype=dtype)                             # one sequence, the last k
            x[0, K - 1] = 1.0
            g = guarded(1, N, dtype)
            ops.gemv_mx4(cd, sd, padded(x, 1), out=g.out)
            assert torch.equal(g.check("every code nb 1"), wv[:, K - 1:].t().to(dtype))


@pytest.mark.parametrize("dtype", D16, ids=dname)
def test_gemv_mx4_every_exponent_exact(ops, dtype):
    """every exponent of the contract, X = -13 .. 13, under every code: the decoded value is exact in the dtype (the smallest,
    0.5 * 2^-13 = 2^-14, is fp16's smallest normal number)"""
    N, K = 27, 32
    codes = torch.arange(16).repeat(2)[None, :].expand(N, K).contiguous()
    X = torch.arange(-13, 14)[:, None]
    wv = R.decode(codes, X)
    cd, sd = planes(*R.pack(codes, X))
    for i0 in (0, 16):
        x = torch.zeros(16, K, dtype=dtype)
        x[torch.arange(16), torch.arange(i0, i0 + 16)] = 1.0
        g = guarded(16, N, dtype)
        ops.gemv_mx4(cd, sd, padded(x, 1), out=g.out)
        assert torch.equal(g.check("every exponent").double(), wv[:, i0:i0 + 16].t())


INT_CODES = torch.tensor([0, 2, 4, 5, 6, 7, 10, 12, 13, 14, 15])      # 0, 1, 2, 3, 4, 6 and the negatives: integers under X = 1 too


@pytest.mark.parametrize("dtype", D16, ids=dname)
@pytest.mark.parametrize("N,K", MX4_SHAPES)
def test_gemv_mx4_integer_probe(ops, N, K, dtype):
    """integer-valued codes {0, +-1, +-2, +-3, +-4, +-6} under X = 1, activations in {-3 .. 3}: every fp32 partial sum is an exact
    integer (<= 36 K < 2^24), so the result is round_T(sum) whatever the accumulation order; a k taken twice or not at all
    changes the integer"""
    gen = torch.Generator().manual_seed(N * 7 + K)
    for nb in MX4_NB:
        codes = INT_CODES[torch.randint(0, INT_CODES.numel(), (N, K), generator=gen)]
        X = torch.ones(N, K // 32, dtype=torch.int64)
        wv = R.decode(codes, X)
        assert torch.equal(wv, wv.round()) and float(wv.abs().max()) == 12.0
        x = torch.randint(-3, 4, (nb, K), generator=gen).to(dtype)
        g = guarded(nb, N, dtype)
        ops.gemv_mx4(*planes(*R.pack(codes, X)), padded(x, 1), out=g.out)
        exp = (x.double() @ wv.t()).to(dtype)
        assert torch.equal(g.check("integer probe"), exp), "integer probe %s nb %d" % ((N, K), nb)


def test_gemv_mx4_refuses_bad_shapes(ops):
    from seedstory._lib import SSError
    mk = lambda N, K, dt=torch.bfloat16, nb=2: (dev(torch.zeros(N, K // 2, dtype=torch.uint8)),  # noqa: E731
                                                dev(torch.full((N, K // 32), 127, dtype=torch.uint8)), dev(torch.zeros(nb, K, dtype=dt)))
    for K in (4128, 8192):                  # past 4096 and not 11008
        with pytest.raises(SSError, match="gemv_mx4"):
            ops.gemv_mx4(*mk(32, K))
    with pytest.raises(SSError, match="K / 32"):        # K = 48: the planes do not pair up
        ops.gemv_mx4(dev(torch.zeros(32, 24, dtype=torch.uint8)), dev(torch.zeros(32, 1, dtype=torch.uint8)), dev(torch.zeros(2, 48, dtype=torch.bfloat16)))
    with pytest.raises(SSError):            # fp32 activations
        ops.gemv_mx4(*mk(32, 64, torch.float32))
    with pytest.raises(SSError, match="gemv_mx4"):
        ops.gemv_mx4(*mk(32, 64, nb=17))
    q, s, x = mk(32, 64)
    with pytest.raises(SSError, match="SILU_MUL"):
        ops.gemv_mx4(q, s, x, silu_mul=True, bias=dev(torch.zeros(16, dtype=torch.bfloat16)))


@pytest.mark.parametrize("dtype", D16, ids=dname)
def test_quantize_weight_rows_mxfp4(ops, dtype):
    """ops.quantize_weight_rows_mxfp4 equals the reference bit for bit, codes and scales, on random rows that include the tie
    values, an all-zero block, an all-zero row, blocks that force the clamp at both ends and a strided input; gemv_mx4 on the
    result is finite, and zero for the zero row"""
    g = torch.Generator().manual_seed(5)
    w = (torch.randn(48, 256, generator=g) * 0.05).to(dtype)
    ties = torch.tensor([6.0, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, -0.25, -0.75, -1.25, -1.75, -2.5, -3.5, -5.0, -6.0])
    w[3, :32] = 0
    w[3, :16] = ties.to(dtype)                         # X = 0: the ties themselves
    w[4, 32:48] = (ties * 2.0 ** -6).to(dtype)         # and under another exponent, beside random values (amax may exceed 6 * 2^-6)
    w[4, 48:64] = 0
    w[5, 64:96] = 0                                    # an all-zero block
    w[7] = 0                                           # an all-zero row
    w[8, :32] = (torch.randn(32, generator=g) * 2.0 ** -18).to(dtype)      # clamp at -13
    w[9, :32] = (torch.randn(32, generator=g) * 30000.0).to(dtype)         # clamp at +13 (saturates)
    w[9, 0] = 60000.0 if dtype == torch.float16 else 2.0 ** 20
    cu, su = ops.quantize_weight_rows_mxfp4(dev(w))
    assert cu.dtype == torch.uint8 and tuple(cu.shape) == (48, 128) and su.dtype == torch.uint8 and tuple(su.shape) == (48, 8)
    rc, rs, wd = R.quantize_packed(w)
    assert int(rs[8, 0]) == 127 - 13 and int(rs[9, 0]) == 127 + 13 and int(rs[5, 2]) == 127 - 13 and int(rs[3, 0]) == 127
    assert torch.equal(su.cpu(), rs), "scales differ at %s" % (su.cpu() != rs).nonzero()[:8].tolist()
    assert torch.equal(cu.cpu(), rc), "codes differ at %s" % (cu.cpu() != rc).nonzero()[:8].tolist()
    assert not cu[7].any() and not cu[5, 32:48].any()
    wide = torch.zeros(48, 320, dtype=dtype)           # a row stride that is not K
    wide[:, :256] = w
    from seedstory._lib import lib, check
    wd_dev = dev(wide)
    cu2 = torch.empty(48, 128, dtype=torch.uint8, device=DEV)
    su2 = torch.empty(48, 8, dtype=torch.uint8, device=DEV)
    check(lib().ss_quantize_rows_mxfp4(wd_dev.data_ptr(), 320, 48, 256, cu2.data_ptr(), su2.data_ptr(), ops.dt(wd_dev),
                                       ops.stream()), "ss_quantize_rows_mxfp4")
    assert torch.equal(cu2.cpu(), rc) and torch.equal(su2.cpu(), rs)
    x = torch.randn(2, 256, generator=g).to(dtype)
    x[:, :32] = 0                                      # (row 9's saturated block would overflow fp16 outputs)
    y = ops.gemv_mx4(cu, su, dev(x)).cpu()
    assert torch.isfinite(y).all() and not y[:, 7].any()
    KC.check(y, *mx4_bound(x, wd, dtype), "gemv_mx4 on quantised rows", family="gemv_mx4", dtype=dtype)


def test_zz_mx4_worst_ratios():
    print("\n" + KC.worst_table())
