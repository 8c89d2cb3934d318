"""Kernel edges: element-wise bounds against an fp64 reference, guarded outputs, exact probes (tests/kernel_check.py).

Every launch writes into a `GuardedOut` (sentinel-filled front / back guards and row gaps; a sentinel left in the payload is an
element the kernel never wrote); inputs are fresh per case and seeded by the tile id as well, so a tile that skips part of its
store cannot find the previous case's answer in a recycled block.  References are fp64 evaluations of the same formula on the
same (already rounded) inputs — never another kernel.  The bounds are derived in kernel_check.py's docstring, not tuned here.

Out of scope: the experimental 4-wave tiles, the gate-mode split GEMM (fp8, the LN-folded, statistics and split-K GEMMs:
tests/test_gemm_variants_edges_gpu.py).

Worst error / bound per kernel family and dtype, measured on an MI355X against the fp64 reference (test_zz_worst_ratios prints
this table; a ratio above 1 fails the case that produced it):

  attention cache v1     bf16  worst error / bound = 0.484
  attention cache v1     fp16  worst error / bound = 0.414
  attention cache v1     fp32  worst error / bound = 0.005
  attention cache v3     bf16  worst error / bound = 0.469
  attention cache v3     fp16  worst error / bound = 0.397
  attention cache v4     bf16  worst error / bound = 0.481
  attention cache v4     fp16  worst error / bound = 0.386
  attention cache v5     bf16  worst error / bound = 0.418
  attention cache v5     fp16  worst error / bound = 0.417
  attention cache v6     bf16  worst error / bound = 0.467
  attention cache v6     fp16  worst error / bound = 0.472
  attention v1           bf16  worst error / bound = 0.407
  attention v1           fp16  worst error / bound = 0.429
  attention v1           fp32  worst error / bound = 0.005
  attention v3           bf16  worst error / bound = 0.434
  attention v3           fp16  worst error / bound = 0.370
  attention v4           bf16  worst error / bound = 0.485
  attention v4           fp16  worst error / bound = 0.423
  attention v5           bf16  worst error / bound = 0.442
  attention v5           fp16  worst error / bound = 0.365
  attention v6           bf16  worst error / bound = 0.489
  attention v6           fp16  worst error / bound = 0.400
  attn_decode            bf16  worst error / bound = 0.295
  attn_decode            fp16  worst error / bound = 0.288
  attn_decode            fp32  worst error / bound = 0.003
  conv3x3                bf16  worst error / bound = 0.988
  conv3x3                fp16  worst error / bound = 0.958
  conv3x3                fp32  worst error / bound = 0.022
  gemm                   bf16  worst error / bound = 0.996
  gemm                   fp16  worst error / bound = 0.997
  gemm                   fp32  worst error / bound = 0.063
  gemm persistent        bf16  worst error / bound = 0.987
  gemm strided           bf16  worst error / bound = 0.975
  gemm strided           fp16  worst error / bound = 0.921
  gemm strided           fp32  worst error / bound = 0.057
  gemv                   bf16  worst error / bound = 0.958
  gemv                   fp16  worst error / bound = 0.977
  gemv                   fp32  worst error / bound = 0.154
  gemv multi-tile        bf16  worst error / bound = 0.905
  gemv multi-tile        fp16  worst error / bound = 0.670
  gemv multi-tile        fp32  worst error / bound = 0.001
  gemv multi-tile silu_mul bf16  worst error / bound = 0.149
  gemv multi-tile silu_mul fp16  worst error / bound = 0.152
  gemv multi-tile silu_mul fp32  worst error / bound = 0.001
  gemv multi-tile split  fp32  worst error / bound = 0.001
  gemv silu_mul          bf16  worst error / bound = 0.166
  gemv silu_mul          fp16  worst error / bound = 0.174
  gemv silu_mul          fp32  worst error / bound = 0.001
"""
import contextlib
import math
import os

import pytest
import torch

import kernel_check as KC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF, FH, F32 = torch.bfloat16, torch.float16, torch.float32
D16 = [BF, FH]
dname = lambda d: KC.NAME[d]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (no CPU fallback exists)")
    from seedstory import ops as _ops
    return _ops


@contextlib.contextmanager
def knobs(**kw):
    from seedstory import _lib
    old = {k: _lib.get_tuning(k) for k in kw}
    try:
        for k, v in kw.items():
            _lib.set_tuning(k, v)
        yield
    finally:
        for k, v in old.items():
            _lib.set_tuning(k, v)


def dev(t):
    return t.to(DEV).contiguous()


def guarded(rows, width, dtype, **kw):
    return KC.GuardedOut(rows, width, dtype, device=DEV, **kw)


# ---- GEMM ---------------------------------------------------------------------------------------------------------------------
def launch_gemm(ops, a, w, kw, out):
    if kw.get("geglu"):
        return ops.gemm_geglu(a, w, dev(kw["bias"]), out=out)
    return ops.gemm(a, w, bias=None if kw.get("bias") is None else dev(kw["bias"]),
                    residual=None if kw.get("residual") is None else dev(kw["residual"]), gelu=bool(kw.get("gelu_")), out=out)


def gemm_case(ops, M, N, K, dtype, epi, seed, family, what):
    a, w = KC.gemm_inputs(M, N, K, dtype, seed)
    kw = KC.epilogue_inputs(epi, M, N, dtype, seed)
    g = guarded(M, N // 2 if epi == "geglu" else N, dtype)
    launch_gemm(ops, dev(a), dev(w), kw, g.out)
    y = g.check(what)
    ref, tol = KC.gemm_bound(a, w, dtype, **kw)
    KC.check(y, ref, tol, what, family=family, dtype=dtype)


@pytest.mark.parametrize("dtype", D16, ids=dname)
@pytest.mark.parametrize("cfg", [0] + KC.GEMM_TILES)
def test_gemm_bound_every_tile(ops, cfg, dtype):
    """every shipped tile id (0: the table / closed-form choice) x epilogue x 16-bit dtype on ragged and whole-tile M / N, 1 .. 7
    K tiles and K % 64 != 0 (forced 20+ ids then run their double-buffered fallback)"""
    with knobs(gemm_cfg=cfg, gemm_autotune=0):
        for i, (M, N, K) in enumerate(KC.GEMM_EDGE_SHAPES):
            for j, epi in enumerate(KC.GEMM_EPILOGUES):
                gemm_case(ops, M, N, K, dtype, epi, cfg * 1000 + i * 10 + j, "gemm", "gemm cfg %d %s %s %s" % (cfg, dname(dtype), (M, N, K), epi))


@pytest.mark.parametrize("cfg", [0] + KC.GEMM_REG_TILES)
def test_gemm_bound_fp32(ops, cfg):
    with knobs(gemm_cfg=cfg, gemm_autotune=0):
        for i, (M, N, K) in enumerate(KC.GEMM_SHAPES):
            for j, epi in enumerate(["plain", "bias+residual", "gelu"] + (["geglu"] if N % 2 == 0 else [])):
                gemm_case(ops, M, N, K, F32, epi, cfg * 1000 + i * 10 + j, "gemm", "gemm cfg %d fp32 %s %s" % (cfg, (M, N, K), epi))


@pytest.mark.parametrize("dtype", D16, ids=dname)
@pytest.mark.parametrize("cfg", KC.GEMM_TILES)
def test_gemm_exact_probes_every_tile(ops, cfg, dtype):
    """selector (one-hot A rows on 0, K - 1 and both sides of every 32 / 64 / 128 boundary), its mirror (one-hot W rows) and the
    all-ones counter: no tolerance"""
    assert any(KC.pp320_eligible(*s) for s in KC.GEMM_PROBE_SHAPES)      # else tiles 56 / 58 would only ever run their fallback
    with knobs(gemm_cfg=cfg, gemm_autotune=0):
        for (M, N, K) in KC.GEMM_PROBE_SHAPES:
            for probe in (KC.selector_probe, KC.selector_probe_w, KC.counter_probe):
                a, w, exp = probe(M, N, K, dtype, seed=cfg)
                g = guarded(M, N, dtype)
                ops.gemm(dev(a), dev(w), out=g.out)
                what = "%s cfg %d %s %s" % (probe.__name__, cfg, dname(dtype), (M, N, K))
                y = g.check(what)
                bad = (y != exp).nonzero()
                assert not bad.numel(), "%s: %d wrong elements, first at %s (got %s, want %s)" % (
                    what, bad.shape[0], tuple(bad[0].tolist()), float(y[tuple(bad[0])]), float(exp[tuple(bad[0])]))


@pytest.mark.parametrize("cfg", [0] + KC.GEMM_REG_TILES)
def test_gemm_exact_probes_fp32(ops, cfg):
    with knobs(gemm_cfg=cfg, gemm_autotune=0):
        for (M, N, K) in [(257, 330, 448), (37, 100, 256), (129, 72, 24)]:
            for probe in (KC.selector_probe, KC.selector_probe_w, KC.counter_probe):
                a, w, exp = probe(M, N, K, F32, seed=cfg)
                g = guarded(M, N, F32)
                ops.gemm(dev(a), dev(w), out=g.out)
                assert torch.equal(g.check(probe.__name__), exp), (probe.__name__, cfg, M, N, K)


@pytest.mark.parametrize("cfg", KC.GEMM_PERSISTENT_TILES)
@pytest.mark.parametrize("M,N,K", KC.GEMM_PERSISTENT_SHAPES)
def test_gemm_bound_persistent_multi_tile(ops, cfg, M, N, K):
    """the shapes of test_gemm_persistent_multi_tile (several output tiles per workgroup), element-wise; the fp64 reference of
    these sizes is a torch fp64 product on the device"""
    dtype = BF
    a, w, bias, res = KC.persistent_inputs(M, N, K, dtype, M + N + K + 31 * cfg, device=DEV)
    g = guarded(M, N, dtype)
    with knobs(gemm_cfg=cfg):
        ops.gemm(a, w, bias=bias, residual=res, out=g.out)
    what = "gemm persistent cfg %d %s" % (cfg, (M, N, K))
    y = g.check(what, cpu=False)
    ref, tol = KC.gemm_bound(a, w, dtype, bias=bias, residual=res)
    KC.check(y, ref, tol, what, family="gemm persistent", dtype=dtype)


@pytest.mark.parametrize("dtype", D16, ids=dname)
@pytest.mark.parametrize("cfg", [0] + KC.GEMM_TILES)
def test_gemm_in_place_residual(ops, cfg, dtype):
    """out aliases residual (the ViT's attention out-projection and MLP down-projection run that way): bit-equal to the call with
    separate buffers.  The pipelined epilogue prefetches the residual two chunks ahead of its own stores."""
    assert any(KC.pp320_eligible(*s) for s in KC.GEMM_INPLACE_SHAPES)    # the 320-wide pipelined epilogue's residual prefetch
    with knobs(gemm_cfg=cfg, gemm_autotune=0):
        for i, (M, N, K) in enumerate(KC.GEMM_INPLACE_SHAPES):
            a, w = KC.gemm_inputs(M, N, K, dtype, 500 + cfg * 10 + i)
            kw = KC.epilogue_inputs("bias+residual", M, N, dtype, 500 + cfg * 10 + i)
            a, w, bias, res = dev(a), dev(w), dev(kw["bias"]), dev(kw["residual"])
            g0 = guarded(M, N, dtype)
            ops.gemm(a, w, bias=bias, residual=res, out=g0.out)
            want = g0.check("separate buffers")
            g1 = guarded(M, N, dtype)
            g1.out.copy_(res)
            ops.gemm(a, w, bias=bias, residual=g1.out, out=g1.out)
            got = g1.check("in place cfg %d %s %s" % (cfg, dname(dtype), (M, N, K)))
            bad = (got != want).nonzero()
            assert not bad.numel(), "in place cfg %d %s %s: %d elements differ, first at %s" % (
                cfg, dname(dtype), (M, N, K), bad.shape[0], tuple(bad[0].tolist()))


@pytest.mark.parametrize("cfg,dtype", [(c, d) for c in [0] + KC.GEMM_TILES for d in D16] + [(c, F32) for c in [0] + KC.GEMM_REG_TILES],
                         ids=lambda x: KC.NAME.get(x, str(x)))
def test_gemm_strides_and_alignment(ops, cfg, dtype):
    """ss_gemm through ctypes: ldc in {N, N + 1, N + 8} with the row gaps guarded, and C / residual / bias each one element off
    their 16-byte alignment.  The staged epilogues test the alignment of C / residual / bias and ldc / ldr % 8 per launch
    (ss_gemm_sp.inc / ss_gemm_pp.inc `staged`) and fall to gemm_epilogue, whose vector paths test C, ldc, bias, residual and ldr
    again (`vec_ok`, `vec_c`, the GEGLU pair store) before their scalar forms; A, W, lda, ldw stay aligned as the header requires.
    Accepted: a correct result with untouched gaps, or a clean SSError with nothing written."""
    from seedstory import _lib
    lib, DT = _lib.lib(), ops.dt(dtype)
    stream = lambda: torch.cuda.current_stream().cuda_stream
    with knobs(gemm_cfg=cfg, gemm_autotune=0):
        for i, (M, N, K) in enumerate(KC.GEMM_STRIDE_SHAPES):
            a, w = KC.gemm_inputs(M, N, K, dtype, 900 + cfg * 10 + i)
            kw = KC.epilogue_inputs("bias+residual", M, N, dtype, 900 + cfg * 10 + i)
            ad, wd = dev(a), dev(w)
            resbuf = torch.zeros(M * N + 1, dtype=dtype, device=DEV)
            biasbuf = torch.zeros(N + 1, dtype=dtype, device=DEV)
            cases = [(ldc, 0, 0, 0, geglu) for ldc in (0, 1, 8) for geglu in (False, True)]
            cases += [(0, 1, 0, 0, False), (0, 0, 1, 0, False), (0, 0, 0, 1, False), (8, 1, 1, 1, False), (0, 1, 0, 1, True)]
            for (dld, oc, orr, ob, geglu) in cases:
                No = N // 2 if geglu else N
                res = resbuf[orr:orr + M * N].view(M, N)
                res.copy_(kw["residual"])
                bias = biasbuf[ob:ob + N]
                bias.copy_(kw["bias"])
                g = guarded(M, No, dtype, ld=No + dld, offset=oc)
                epi = (_lib.EPI_BIAS | _lib.EPI_GEGLU_PAIR) if geglu else (_lib.EPI_BIAS | _lib.EPI_RESIDUAL)
                what = "ss_gemm cfg %d %s %s ldc N%+d C%+d res%+d bias%+d %s" % (cfg, dname(dtype), (M, N, K), dld, oc, orr, ob, "geglu" if geglu else "bias+residual")
                rc = lib.ss_gemm(ad.data_ptr(), wd.data_ptr(), g.data_ptr(), M, N, K, K, K, No + dld, bias.data_ptr(),
                                 None if geglu else res.data_ptr(), 0 if geglu else N, epi, DT, stream())
                if rc != 0:
                    with pytest.raises(_lib.SSError):
                        _lib.check(rc, what)
                    torch.cuda.synchronize()
                    assert bool((g.flat == KC.SENTINEL[dtype]).all()), what + ": refused, yet something was written"
                    continue
                y = g.check(what)
                ref, tol = KC.gemm_bound(a, w, dtype, bias=kw["bias"], geglu=True) if geglu else \
                    KC.gemm_bound(a, w, dtype, bias=kw["bias"], residual=kw["residual"])
                KC.check(y, ref, tol, what, family="gemm strided", dtype=dtype)


# ---- conv3x3 ------------------------------------------------------------------------------------------------------------------
def nhwc(x):
    B, C, H, W = x.shape
    return x.permute(0, 2, 3, 1).reshape(B * H * W, C).contiguous()


def conv_w(w):
    """[Co, Ci, 3, 3] -> [Co, 9 * Ci], k = (ky * 3 + kx) * Ci + ci"""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).contiguous()


@pytest.mark.parametrize("cfg,dtype", [(c, d) for c in [0] + KC.CONV_TILES for d in D16] + [(0, F32)], ids=lambda x: KC.NAME.get(x, str(x)))
def test_conv3x3_bound_every_tile(ops, cfg, dtype):
    """conv alone, + bias, + row vector, + residual — each against its own reference (no shared denominator); fp32 has the one
    register-staged kernel"""
    with knobs(gemm_cfg=cfg, gemm_autotune=0):
        for i, (B, Ci, Co, H, W, stride, up) in enumerate(KC.CONV_EDGE_CASES):
            x, w, bias, tv, res = KC.conv_inputs(B, Ci, Co, H, W, stride, up, dtype, cfg * 100 + i)
            xd, wd = dev(nhwc(x)), dev(conv_w(w))
            for names in KC.CONV_VARIANTS:
                kw = {n: {"bias": bias, "rowvec": tv, "residual": res}[n] for n in names}
                ref, tol = KC.conv_bound(x, w, dtype, stride, up, **kw)
                Ho, Wo = ref.shape[2], ref.shape[3]
                g = guarded(B * Ho * Wo, Co, dtype)
                _, ho, wo = ops.conv3x3(xd, wd, B, H, W, stride=stride, upsample=up, bias=None if "bias" not in kw else dev(bias),
                                        rowvec=None if "rowvec" not in kw else dev(tv),
                                        residual=None if "residual" not in kw else dev(nhwc(res)), out=g.out)
                what = "conv3x3 cfg %d %s %s %s" % (cfg, dname(dtype), (B, Ci, Co, H, W, stride, up), "+".join(sorted(kw)) or "alone")
                assert (ho, wo) == (Ho, Wo), what
                KC.check(g.check(what), nhwc(ref), nhwc(tol), what, family="conv3x3", dtype=dtype)


@pytest.mark.parametrize("dtype", D16, ids=dname)
@pytest.mark.parametrize("cfg", [0] + KC.CONV_TILES)
def test_conv3x3_impulse_probes_every_tile(ops, cfg, dtype):
    """one nonzero pixel per launch (corners, edges, w = W - 1, the last image): every output holds one weight (up to four under
    the fused upsample) — equal to the fp64 convolution rounded to T, bit for bit"""
    assert any(KC.conv_pp320_eligible(*c) for c in KC.CONV_IMPULSE_CASES)        # conv tile 56 itself, not its fallback
    with knobs(gemm_cfg=cfg, gemm_autotune=0):
        for i, (B, Ci, Co, H, W, stride, up) in enumerate(KC.CONV_IMPULSE_CASES):
            w = (torch.randint(-32, 32, (Co, Ci, 3, 3), generator=torch.Generator().manual_seed(cfg * 10 + i)) / 8.0).to(dtype)
            wd = dev(conv_w(w))
            for p in KC.conv_impulse_positions(B, H, W):
                x = KC.conv_impulse(B, Ci, H, W, p, (p[1] * 5 + p[2] + cfg) % Ci, dtype)
                exp = KC.conv_expected(x, w, dtype, stride, up)
                g = guarded(B * exp.shape[2] * exp.shape[3], Co, dtype)
                ops.conv3x3(dev(nhwc(x)), wd, B, H, W, stride=stride, upsample=up, out=g.out)
                what = "conv impulse cfg %d %s %s at %s" % (cfg, dname(dtype), (B, Ci, Co, H, W, stride, up), p)
                y = g.check(what)
                bad = (y != nhwc(exp)).nonzero()
                assert not bad.numel(), "%s: %d wrong outputs, first at (pixel row %d, channel %d)" % (what, bad.shape[0], int(bad[0, 0]), int(bad[0, 1]))


def test_conv3x3_impulse_probes_fp32(ops):
    with knobs(gemm_autotune=0):
        for i, (B, Ci, Co, H, W, stride, up) in enumerate(KC.CONV_IMPULSE_CASES):
            w = (torch.randint(-32, 32, (Co, Ci, 3, 3), generator=torch.Generator().manual_seed(77 + i)) / 8.0).to(F32)
            for p in KC.conv_impulse_positions(B, H, W):
                x = KC.conv_impulse(B, Ci, H, W, p, (p[1] * 5 + p[2]) % Ci, F32)
                exp = KC.conv_expected(x, w, F32, stride, up)
                g = guarded(B * exp.shape[2] * exp.shape[3], Co, F32)
                ops.conv3x3(dev(nhwc(x)), dev(conv_w(w)), B, H, W, stride=stride, upsample=up, out=g.out)
                assert torch.equal(g.check("conv impulse fp32"), nhwc(exp)), (B, Ci, Co, H, W, stride, up, p)


# ---- attention ----------------------------------------------------------------------------------------------------------------
# (attn_ver, attn_waves): v1 | v3 swizzled V | v3 linear V | v3p with prefetch | v3p by rule, 4, 8, 16 waves
ATTN_KERNELS = [(1, 0), (3, 0), (4, 0), (5, 0), (6, 0), (6, 4), (6, 8), (6, 16)]
ATTN_PARAMS = [(v, wv, d) for (v, wv) in ATTN_KERNELS for d in D16] + [(6, 0, F32)]      # fp32 has the one (v1) kernel


@pytest.mark.parametrize("ver,waves,dtype", ATTN_PARAMS, ids=lambda x: KC.NAME.get(x, str(x)))
def test_attention_bound_and_selector(ops, ver, waves, dtype):
    with knobs(attn_ver=ver, attn_waves=waves):
        for i, (B, H, hd, Lq, Lk, causal) in enumerate(KC.ATTN_EDGE_CASES):
            what = "attention ver %d waves %d %s %s" % (ver, waves, dname(dtype), (B, H, hd, Lq, Lk, causal))
            q, k, v = KC.attn_inputs(B, H, hd, Lq, Lk, dtype, ver * 1000 + waves * 50 + i)
            scale = 1.0 / math.sqrt(hd)
            g = guarded(B * Lq, H * hd, dtype)
            ops.attention(dev(q), dev(k), dev(v), H, scale, causal, out=g.view(B, Lq, H * hd))
            y = g.check(what).view(B, Lq, H * hd)
            ref, tol = KC.attention_bound(KC.heads(q, H), KC.heads(k, H), KC.heads(v, H), scale, KC.causal_allow(Lq, Lk) if causal else None, dtype)
            KC.check(KC.heads(y, H), ref, tol, what, family="attention v%d" % (1 if dtype == F32 else ver), dtype=dtype)
            # selector probe: scale 1, one head's probe repeated over batch and heads with different V
            qs, ks, vs = KC.attention_selector(Lq, Lk, hd, dtype, seed=i + ver, H=B * H)
            pk = lambda t: KC.unheads(t.view(B, H, t.shape[1], hd))
            g = guarded(B * Lq, H * hd, dtype)
            ops.attention(dev(pk(qs)), dev(pk(ks)), dev(pk(vs)), H, 1.0, causal, out=g.view(B, Lq, H * hd))
            y = KC.heads(g.check(what + " selector").view(B, Lq, H * hd), H).reshape(B * H, Lq, hd)
            exp = KC.attention_selector_expected(vs, Lq, Lk, causal)
            bad = (y != exp).any(-1).nonzero()
            assert not bad.numel(), "%s selector: %d query rows select the wrong key, first (head %d, query %d)" % (
                what, bad.shape[0], int(bad[0, 0]), int(bad[0, 1]))


def cache_planes(H, cap, hd, kvl, dtype, seed, S=None):
    """K / V cache planes [H, cap, hd] (or [S, H, cap, hd]): rows < kv_len random, rows in [kv_len, cap) NaN / +Inf"""
    g = torch.Generator().manual_seed(9000 + seed)
    kc, vc = torch.randn(H, cap, hd, generator=g).to(dtype), torch.randn(H, cap, hd, generator=g).to(dtype)
    if kvl < cap:
        KC.poison_(kc[:, kvl:])
        KC.poison_(vc[:, kvl:])
    return kc, vc


@pytest.mark.parametrize("ver,waves,dtype", ATTN_PARAMS, ids=lambda x: KC.NAME.get(x, str(x)))
def test_attention_cache_poisoned_tail(ops, ver, waves, dtype):
    """attention_cache / attention_cache_slots with unequal kv_lens; cache rows in [kv_len, cap) hold NaN and +Inf: memory outside
    the declared extent must never reach the result (finite, inside the bound, bit-equal to the run over a zeroed tail; at
    hd = 104 the 128-wide kernels' head-dim padding of the last valid row IS the first poisoned row)"""
    with knobs(attn_ver=ver, attn_waves=waves):
        for i, (H, hd, cap, M, lens) in enumerate(KC.ATTN_CACHE_CASES):
            E, S = H * hd, len(lens)
            g_ = torch.Generator().manual_seed(ver * 100 + waves + i)
            q = torch.randn(S * M, E, generator=g_).to(dtype)
            planes = [cache_planes(H, cap, hd, kvl, dtype, ver * 1000 + waves * 50 + i * 10 + s) for s, kvl in enumerate(lens)]
            kc, vc = torch.stack([p[0] for p in planes]), torch.stack([p[1] for p in planes])
            kz, vz = torch.nan_to_num(kc, nan=0.0, posinf=0.0), torch.nan_to_num(vc, nan=0.0, posinf=0.0)
            what = "attention_cache ver %d waves %d %s %s lens %s" % (ver, waves, dname(dtype), (H, hd, cap, M), lens)
            g = guarded(S * M, E, dtype)
            ops.attention_cache_slots(dev(q), dev(kc), dev(vc), lens, out=g.out)
            y_slots = g.check(what + " slots")
            gz = guarded(S * M, E, dtype)
            ops.attention_cache_slots(dev(q), dev(kz), dev(vz), lens, out=gz.out)
            assert torch.equal(y_slots, gz.check(what + " slots, zeroed tail")), what + ": the poisoned tail changed the result"
            for s, kvl in enumerate(lens):
                qs = q[s * M:(s + 1) * M].contiguous()
                g1 = guarded(M, E, dtype)
                ops.attention_cache(dev(qs), dev(kc[s]), dev(vc[s]), kvl, causal_br=True, out=g1.out)
                y1 = g1.check(what + " slot %d" % s)
                to_h = lambda t: t.view(M, H, hd).transpose(0, 1)
                ref, tol = KC.attention_bound(to_h(qs), kc[s][:, :kvl], vc[s][:, :kvl], 1.0 / math.sqrt(hd), KC.causal_allow(M, kvl), dtype)
                fam = "attention cache v%d" % (1 if dtype == F32 else ver)
                KC.check(to_h(y1), ref, tol, what + " slot %d" % s, family=fam, dtype=dtype)
                KC.check(to_h(y_slots[s * M:(s + 1) * M]), ref, tol, what + " slots[%d]" % s, family=fam, dtype=dtype)
            # selector through the cache entry points (scale fixed at 1 / sqrt(hd): kscale 16), poisoned tail kept
            s, kvl = 1, lens[1]
            qs_, ks_, vs_ = KC.attention_selector(M, kvl, hd, dtype, seed=i, H=H, kscale=16.0)
            kc1, vc1 = kc[s].clone(), vc[s].clone()
            kc1[:, :kvl], vc1[:, :kvl] = ks_, vs_
            g1 = guarded(M, E, dtype)
            ops.attention_cache(dev(qs_.transpose(0, 1).reshape(M, E)), dev(kc1), dev(vc1), kvl, causal_br=True, out=g1.out)
            y = g1.check(what + " selector").view(M, H, hd).transpose(0, 1)
            assert torch.equal(y, KC.attention_selector_expected(vs_, M, kvl, True)), what + " selector"
            # ... and through the ragged launch: every slot holds the probe at ITS length, tails stay poisoned
            kcs, vcs, qss, exps = kc.clone(), vc.clone(), [], []
            for s, kvl in enumerate(lens):
                qs_, ks_, vs_ = KC.attention_selector(M, kvl, hd, dtype, seed=i * 10 + s, H=H, kscale=16.0)
                kcs[s][:, :kvl], vcs[s][:, :kvl] = ks_, vs_
                qss.append(qs_.transpose(0, 1).reshape(M, E))
                exps.append(KC.attention_selector_expected(vs_, M, kvl, True).transpose(0, 1).reshape(M, E))
            g1 = guarded(S * M, E, dtype)
            ops.attention_cache_slots(dev(torch.cat(qss)), dev(kcs), dev(vcs), lens, out=g1.out)
            assert torch.equal(g1.check(what + " slots selector"), torch.cat(exps)), what + " slots selector"


@pytest.mark.parametrize("dtype", D16 + [F32], ids=dname)
@pytest.mark.parametrize("hd", [64, 128])
def test_attn_decode_splits_poison_selector(ops, hd, dtype):
    """attn_decode_nsplit 0 / 4 / 8 / 16 / 32 x kv_len 1, nsplit - 1, nsplit, nsplit + 1 (empty splits in the merge), 500, cap;
    poisoned tail; selector probe; every split count inside the bound of the same fp64 reference"""
    H, cap = KC.DECODE_HEADS, KC.DECODE_CAP
    scale = 1.0 / math.sqrt(hd)
    for kvl in KC.DECODE_KV_LENS:
        g_ = torch.Generator().manual_seed(hd + kvl)
        q = torch.randn(H * hd, generator=g_).to(dtype)
        kc, vc = cache_planes(H, cap, hd, kvl, dtype, hd + kvl)
        ref, tol = KC.attention_bound(q.view(H, 1, hd), kc[:, :kvl], vc[:, :kvl], scale, None, dtype)
        qs_, ks_, vs_ = KC.attention_selector(1, kvl, hd, dtype, seed=kvl, H=H, kscale=16.0)
        kc1, vc1 = kc.clone(), vc.clone()
        kc1[:, :kvl], vc1[:, :kvl] = ks_, vs_
        n = torch.tensor([kvl], dtype=torch.int32, device=DEV)
        kd, vd, k1d, v1d = dev(kc), dev(vc), dev(kc1), dev(vc1)
        outs = {}
        for ns in KC.DECODE_NSPLITS:
            what = "attn_decode hd %d %s nsplit %d kv_len %d" % (hd, dname(dtype), ns, kvl)
            with knobs(attn_decode_nsplit=ns):
                g = guarded(1, H * hd, dtype)
                ops.attn_decode(dev(q), kd, vd, n, out=g.view(H * hd))
                y = g.check(what).view(H, 1, hd)
                KC.check(y, ref, tol, what, family="attn_decode", dtype=dtype)
                outs[ns] = y
                g = guarded(1, H * hd, dtype)
                ops.attn_decode(dev(qs_.reshape(H * hd)), k1d, v1d, n, out=g.view(H * hd))
                assert torch.equal(g.check(what + " selector").view(H, 1, hd), KC.attention_selector_expected(vs_, 1, kvl, False)), what + " selector"
        # equality across split counts within the bound: every count was held to the bound of the SAME fp64 reference above.
        # Where the launch is the same the results must agree bit for bit: nsplit 0 means 16 at one slot.
        assert torch.equal(outs[0], outs[16]), "attn_decode nsplit 0 vs 16, kv_len %d" % kvl


# ---- GEMV ---------------------------------------------------------------------------------------------------------------------
def padded(t, extra_rows):
    """t [R, C] as the head of a longer allocation whose tail is NaN / +Inf"""
    buf = torch.empty(t.shape[0] + extra_rows, t.shape[1], dtype=t.dtype)
    buf[:t.shape[0]] = t
    KC.poison_(buf[t.shape[0]:])
    return dev(buf)[:t.shape[0]]


@pytest.mark.parametrize("dtype", D16 + [F32], ids=dname)
@pytest.mark.parametrize("N,K", KC.GEMV_SHAPES)
def test_gemv_bound_probes_poison(ops, N, K, dtype):
    """dot-product GEMV and its batched / MFMA forms (nb 1 .. 16 with gemv_mfma_min_nb = 1, specialised and generic): bound,
    selector and counter probes; the memory right after W's last row and after x holds NaN / +Inf"""
    seed = N + K
    forms = [(0, 0)] + ([(1, 0), (1, 1)] if dtype != F32 else [])        # (min_nb forced to 1, generic)
    for nb in KC.GEMV_NB:
        x, w = KC.gemm_inputs(nb, N, K, dtype, seed + nb)
        kw = KC.epilogue_inputs("bias+residual", nb, N, dtype, seed + nb)
        wd, xd = padded(w, 3), padded(x, 1)
        sa, sw, sexp = KC.selector_probe(nb, N, K, dtype, seed=seed + nb)
        ca, cw, cexp = KC.counter_probe(nb, N, K, dtype, seed=seed + nb)
        ref0, tol0 = KC.gemm_bound(x, w, dtype)
        ref1, tol1 = KC.gemm_bound(x, w, dtype, **kw)
        for (mfma1, generic) in forms:
            what = "gemv %s %s nb %d mfma_min_nb %d generic %d" % ((N, K), dname(dtype), nb, 1 if mfma1 else 3, generic)
            with knobs(gemv_mfma_min_nb=1 if mfma1 else 3, gemv_mfma_generic=generic):
                g = guarded(nb, N, dtype)
                ops.gemv_batched(wd, xd, out=g.out)
                KC.check(g.check(what), ref0, tol0, what, family="gemv", dtype=dtype)
                g = guarded(nb, N, dtype)
                ops.gemv_batched(wd, xd, bias=dev(kw["bias"]), residual=dev(kw["residual"]), out=g.out)
                KC.check(g.check(what), ref1, tol1, what + " bias+residual", family="gemv", dtype=dtype)
                for (pa, pw, pexp, name) in ((sa, sw, sexp, "selector"), (ca, cw, cexp, "counter")):
                    g = guarded(nb, N, dtype)
                    ops.gemv_batched(padded(pw, 3), padded(pa, 1), out=g.out)
                    assert torch.equal(g.check(what + " " + name), pexp), what + " " + name
                if nb == 1 and not mfma1:        # the batch-1 entry point
                    g = guarded(1, N, dtype)
                    ops.gemv(wd, xd[0], out=g.view(N))
                    KC.check(g.check(what + " ss_gemv"), ref0, tol0, what + " ss_gemv", family="gemv", dtype=dtype)
                    g = guarded(1, N, dtype)
                    ops.gemv(padded(sw, 3), padded(sa, 1)[0], out=g.view(N))
                    assert torch.equal(g.check(what + " ss_gemv selector"), sexp), what + " ss_gemv selector"


@pytest.mark.parametrize("dtype", D16 + [F32], ids=dname)
@pytest.mark.parametrize("I,K", KC.GEMV_SILU_SHAPES)
def test_gemv_silu_mul_bound(ops, I, K, dtype):
    for nb in (1, 2, 4, 8):
        x, w = KC.gemm_inputs(nb, 2 * I, K, dtype, I + K + nb)
        ref, tol = KC.silu_mul_bound(w, x, dtype)
        wd, xd = padded(w, 3), padded(x, 1)
        for mfma1 in ((0, 1) if dtype != F32 else (0,)):
            what = "gemv silu_mul %s %s nb %d mfma_min_nb %d" % ((I, K), dname(dtype), nb, 1 if mfma1 else 3)
            with knobs(gemv_mfma_min_nb=1 if mfma1 else 3):
                g = guarded(nb, I, dtype)
                ops.gemv_batched(wd, xd, silu_mul=True, out=g.out)
                KC.check(g.check(what), ref, tol, what, family="gemv silu_mul", dtype=dtype)
        if nb == 1:
            g = guarded(1, I, dtype)
            ops.gemv(wd, xd[0], silu_mul=True, out=g.view(I))
            KC.check(g.check("ss_gemv silu_mul"), ref, tol, "ss_gemv silu_mul %s" % ((I, K),), family="gemv silu_mul", dtype=dtype)


GEMV_MULTI_SHAPES = [(100, 256), (37, 4096), (40, 11008)]       # N, K: generic MFMA / exact 16-step / packed 43-step depths


def rmsnorm_inputs(x, K, dtype, seed):
    """(gain [K] of the model dtype, fp64 reference of the RMS-normalised activations, bound of their error).
    The kernels form rstd = 1 / sqrt(sum x^2 / K + eps) in fp32 (K positive terms, then a division, an addition, a square root
    and a reciprocal: relative error <= (K + 8) u32 together with the product x * rstd), round x * rstd to T, multiply by the gain
    in fp32 and round to T again when the pack is formed (fp32: both roundings are the fp32 operation's own)."""
    g = torch.Generator().manual_seed(8000 + seed)
    gain = (1.0 + 0.1 * torch.randn(K, generator=g)).to(dtype)
    xd = x.double()
    v = xd / torch.sqrt((xd * xd).mean(dim=1, keepdim=True) + 1e-5)
    v, t = KC.mid_round(v, (K + 8) * KC.U32 * v.abs(), dtype)
    v, t = KC.product(v, t, gain.double().expand_as(v), torch.zeros_like(v))
    v, t = KC.mid_round(v, t, dtype)
    return gain, v, t


@pytest.mark.parametrize("dtype", D16 + [F32], ids=dname)
def test_gemv_multi_tile_bound(ops, dtype):
    """gemv_mfma_blocks = 2 and gemv_max_blocks = 1: every persistent workgroup of the MFMA forms walks several row tiles (two
    register buffers, LDS parity, the prefetch across the tile boundary) and every wave of the dot-product forms several row
    groups, at sizes where only the LLaMA-sized shapes do under the default knobs.  Plain, bias + residual, the fused RMSNorm
    prologue and the SiLU pair (I = 24, and I = 40: three tiles on two workgroups) at 1 / 4 / 8 sequences, against the same bounds as the other GEMV tests; with the
    RMSNorm the activations themselves carry an error (rmsnorm_inputs), which enters the accumulator's bound as t_x |w|.
    fp32 also runs the split-bf16 form (gemm_f32_split = 1) over two K slices, (37, 4104): its operands are hi + lo bf16 pairs
    with the lo x lo term dropped, 2^-16 per product relative, far inside the 2 K u32 = 2^-11 of the exact chain's bound."""
    with knobs(gemv_mfma_blocks=2, gemv_max_blocks=1):
        for (N, K) in GEMV_MULTI_SHAPES:
            for nb in (1, 4, 8):
                seed = N + K + nb
                x, w = KC.gemm_inputs(nb, N, K, dtype, seed)
                kw = KC.epilogue_inputs("bias+residual", nb, N, dtype, seed)
                gain, xn, tx = rmsnorm_inputs(x, K, dtype, seed)
                wd, xd = padded(w, 3), padded(x, 1)
                what = "gemv multi-tile %s %s nb %d" % ((N, K), dname(dtype), nb)
                run = lambda g, **k: (ops.gemv(wd, xd[0], out=g.view(N), **k) if nb == 1 else ops.gemv_batched(wd, xd, out=g.out, **k))  # noqa: E731
                g = guarded(nb, N, dtype)
                run(g)
                KC.check(g.check(what), *KC.gemm_bound(x, w, dtype), what, family="gemv multi-tile", dtype=dtype)
                g = guarded(nb, N, dtype)
                run(g, bias=dev(kw["bias"]), residual=dev(kw["residual"])[0] if nb == 1 else dev(kw["residual"]))
                KC.check(g.check(what), *KC.gemm_bound(x, w, dtype, **kw), what + " bias+residual", family="gemv multi-tile", dtype=dtype)
                g = guarded(nb, N, dtype)
                run(g, norm_w=dev(gain), eps=1e-5)
                v, t = KC.accumulate(xn, w)
                ref, tol = KC.epilogue(v, t + (1.0 + 2.0 * K * KC.U32) * (tx @ w.double().abs().t()), dtype)
                KC.check(g.check(what), ref, tol, what + " rmsnorm", family="gemv multi-tile", dtype=dtype)
                for I in (24, 40):
                    xs, ws = KC.gemm_inputs(nb, 2 * I, K, dtype, seed + I)
                    g = guarded(nb, I, dtype)
                    if nb == 1:
                        ops.gemv(padded(ws, 3), padded(xs, 1)[0], silu_mul=True, out=g.view(I))
                    else:
                        ops.gemv_batched(padded(ws, 3), padded(xs, 1), silu_mul=True, out=g.out)
                    KC.check(g.check(what), *KC.silu_mul_bound(ws, xs, dtype), what + " silu_mul I %d" % I, family="gemv multi-tile silu_mul", dtype=dtype)
        if dtype == F32:
            N, K, nb = 37, 4104, 8
            x, w = KC.gemm_inputs(nb, N, K, dtype, N + K)
            kw = KC.epilogue_inputs("bias+residual", nb, N, dtype, N + K)
            with knobs(gemm_f32_split=1):
                for name, k in (("plain", {}), ("bias+residual", kw)):
                    g = guarded(nb, N, dtype)
                    ops.gemv_batched(padded(w, 3), padded(x, 1), out=g.out, **{n: dev(v) for n, v in k.items()})
                    what = "gemv multi-tile split %s %s" % ((N, K), name)
                    KC.check(g.check(what), *KC.gemm_bound(x, w, dtype, **k), what, family="gemv multi-tile split", dtype=dtype)


def test_out_argument_is_checked(ops):
    from seedstory import _lib
    a, w = dev(torch.zeros(4, 64, dtype=BF)), dev(torch.zeros(8, 64, dtype=BF))
    with pytest.raises(_lib.SSError):
        ops.gemv_batched(w, a, out=torch.empty(4, 9, dtype=BF, device=DEV))
    with pytest.raises(_lib.SSError):
        ops.gemm_geglu(a, w, dev(torch.zeros(8, dtype=BF)), out=torch.empty(4, 4, dtype=FH, device=DEV))


def test_zz_worst_ratios():
    """prints the worst error / bound per kernel family and dtype seen by this file's checks (the record kept in the module
    docstring); SS_KERNEL_RATIO_FILE=<path> also writes it"""
    table = KC.worst_table()
    print("\nworst error / bound per family and dtype:\n" + table)
    path = os.environ.get("SS_KERNEL_RATIO_FILE")
    if path:
        with open(path, "w") as f:
            f.write(table + "\n")
    assert all(r <= 1.0 for r in KC.WORST.values())
