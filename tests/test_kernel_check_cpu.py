"""The checker (tests/kernel_check.py) is tested before it judges a kernel: a correct kernel SIMULATED on the CPU (fp32 math,
chunked and reversed summation, the kernels' rounding points; attention: a tile-64 online softmax with P rounded to T) must
produce zero violations on every case tests/test_kernel_edges_gpu.py, tests/test_pointwise_edges_gpu.py,
tests/test_gemm_variants_edges_gpu.py and tests/test_decode_step_gpu.py run (the grid-stride shapes of the second reduced to a
small shape of the same family), and every seeded mutant must be flagged."""
import math

import pytest
import torch

import kernel_check as KC

DTYPES16 = [torch.bfloat16, torch.float16]
ALL = DTYPES16 + [torch.float32]


# ---- simulated kernels --------------------------------------------------------------------------------------------------------
def sim_acc(a, w, chunk=32):
    """fp32 accumulation of a @ w^T in chunks of `chunk` k, last chunk first"""
    a32, w32 = a.float(), w.float()
    K = a.shape[1]
    acc = torch.zeros(a.shape[0], w.shape[0], dtype=torch.float32)
    for k0 in reversed(range(0, K, chunk)):
        acc = acc + a32[:, k0:k0 + chunk] @ w32[:, k0:k0 + chunk].t()
    return acc


def r(x, dtype, trunc=False):
    if trunc:
        return trunc_to(x, dtype)
    return x.to(dtype).float()


def trunc_to(x, dtype):
    """round toward zero to T (the mutant store)"""
    y = x.to(dtype).float()
    over = y.abs() > x.abs()
    step = torch.nextafter(y.to(dtype), torch.zeros_like(y).to(dtype)).float() if dtype != torch.float32 else y
    return torch.where(over, step, y)


def gelu32(x):
    return 0.5 * x * (1.0 + torch.erf(x * 0.7071067811865476))


def sim_epilogue(acc, dtype, bias=None, residual=None, gelu_=False, geglu=False, rowvec=None, trunc=False):
    t = acc
    if bias is not None:
        t = t + bias.float()
    if geglu:
        v = r(t, dtype)
        return (v[:, 0::2] * r(gelu32(v[:, 1::2]), dtype)).to(dtype)
    if gelu_:
        t = gelu32(r(t, dtype))
    v = r(t, dtype, trunc and rowvec is None and residual is None)
    if rowvec is not None:
        v = r(v + rowvec.float(), dtype, trunc and residual is None)
    if residual is not None:
        v = r(v + residual.float(), dtype, trunc)
    return v.to(dtype)


def sim_gemm(a, w, dtype, trunc=False, **epi):
    return sim_epilogue(sim_acc(a, w), dtype, trunc=trunc, **epi)


def sim_conv(x, w, dtype, stride, up, bias=None, rowvec=None, residual=None):
    F = torch.nn.functional
    xi = F.interpolate(x.float(), scale_factor=2.0, mode="nearest") if up else x.float()
    acc = torch.zeros(1)
    for ky in (2, 1, 0):                 # one tap row at a time, last first
        wk = torch.zeros_like(w.float())
        wk[:, :, ky] = w.float()[:, :, ky]
        acc = acc + F.conv2d(xi, wk, None, stride=stride, padding=1)
    t = acc + bias.float()[None, :, None, None] if bias is not None else acc
    v = r(t, dtype)
    if rowvec is not None:
        v = r(v + rowvec.float()[:, :, None, None], dtype)
    if residual is not None:
        v = v + residual.float()
    return v.to(dtype)


def sim_attention(q, k, v, scale, allow, dtype, tile=64):
    """q [.., Lq, hd], k / v [.., Lk, hd]: online softmax over key tiles of 64 in fp32, P rounded to T before P V"""
    q32, k32, v32 = q.float(), k.float(), v.float()
    Lq, Lk = q.shape[-2], k.shape[-2]
    m = torch.full(q.shape[:-1] + (1,), -1e30)
    l = torch.zeros_like(m)
    acc = torch.zeros(q.shape[:-1] + (v.shape[-1],))
    for t0 in range(0, Lk, tile):
        s = q32 @ k32[..., t0:t0 + tile, :].transpose(-1, -2) * scale
        ok = torch.ones(Lq, s.shape[-1], dtype=torch.bool) if allow is None else allow[:, t0:t0 + tile]
        s = torch.where(ok, s, torch.full_like(s, -1e30))
        m_new = torch.maximum(m, s.amax(-1, keepdim=True))
        p = torch.where(ok, torch.exp(s - m_new), torch.zeros_like(s))
        alpha = torch.exp(m - m_new)
        l = l * alpha + p.sum(-1, keepdim=True)
        acc = acc * alpha + r(p, dtype) @ v32[..., t0:t0 + tile, :]
        m = m_new
    return (acc / l).to(dtype)


def count(y, ref, tol):
    return KC.violations(y, ref, tol)[0]


# ---- zero violations on every GPU case ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES16, ids=lambda d: KC.NAME[d])
@pytest.mark.parametrize("epi", KC.GEMM_EPILOGUES)
def test_simulated_gemm_stays_inside_the_bound(epi, dtype):
    worst = 0.0
    for i, (M, N, K) in enumerate(KC.GEMM_EDGE_SHAPES + KC.GEMM_STRIDE_SHAPES + KC.GEMM_INPLACE_SHAPES + [(1024, 640, 1280), (4096, 256, 2560)]):
        a, w = KC.gemm_inputs(M, N, K, dtype, i)
        kw = KC.epilogue_inputs(epi, M, N, dtype, i)
        ref, tol = KC.gemm_bound(a, w, dtype, **kw)
        worst = max(worst, KC.check(sim_gemm(a, w, dtype, **kw), ref, tol, "sim gemm %s %s" % (epi, (M, N, K))))
    print("simulated gemm %s %s: worst error / bound %.3f" % (epi, KC.NAME[dtype], worst))
    assert worst > 0.05         # a bound nothing comes near checks nothing


@pytest.mark.parametrize("dtype", ALL, ids=lambda d: KC.NAME[d])
def test_simulated_persistent_and_strided_cases_stay_inside_the_bound(dtype):
    """the persistent multi-tile cases keep their N, K and operand scaling (w ~ 0.05 N(0, 1), bias ~ N(0, 1)) on 520 of their rows:
    the bound of an element depends on its own row of A only; the strided ss_gemm cases in every dtype they run in"""
    if dtype == torch.bfloat16:
        for i, (M, N, K) in enumerate(KC.GEMM_PERSISTENT_SHAPES):
            a, w, bias, res = KC.persistent_inputs(520, N, K, dtype, M + N + K + 31 * i)
            ref, tol = KC.gemm_bound(a, w, dtype, bias=bias, residual=res)
            KC.check(sim_gemm(a, w, dtype, bias=bias, residual=res), ref, tol, "sim persistent %s" % ((M, N, K),))
    for i, (M, N, K) in enumerate(KC.GEMM_STRIDE_SHAPES):
        a, w = KC.gemm_inputs(M, N, K, dtype, 900 + i)
        for epi in ("bias+residual", "geglu"):
            kw = KC.epilogue_inputs(epi, M, N, dtype, 900 + i)
            ref, tol = KC.gemm_bound(a, w, dtype, **kw)
            KC.check(sim_gemm(a, w, dtype, **kw), ref, tol, "sim strided %s %s" % ((M, N, K), epi))


@pytest.mark.parametrize("epi", ["plain", "bias+residual", "gelu", "geglu"])
def test_simulated_gemm_fp32_stays_inside_the_bound(epi):
    dtype = torch.float32
    for i, (M, N, K) in enumerate(KC.GEMM_SHAPES):
        a, w = KC.gemm_inputs(M, N, K, dtype, i)
        kw = KC.epilogue_inputs(epi, M, N, dtype, i)
        ref, tol = KC.gemm_bound(a, w, dtype, **kw)
        KC.check(sim_gemm(a, w, dtype, **kw), ref, tol, "sim gemm fp32 %s %s" % (epi, (M, N, K)))


@pytest.mark.parametrize("dtype", ALL, ids=lambda d: KC.NAME[d])
def test_simulated_gemv_stays_inside_the_bound(dtype):
    for (N, K) in KC.GEMV_SHAPES:
        for nb in KC.GEMV_NB:                   # the batch sizes and seeds of test_gemv_bound_probes_poison
            x, w = KC.gemm_inputs(nb, N, K, dtype, N + K + nb)
            for kw in ({}, KC.epilogue_inputs("bias+residual", nb, N, dtype, N + K + nb)):
                ref, tol = KC.gemm_bound(x, w, dtype, **kw)
                KC.check(sim_gemm(x, w, dtype, **kw), ref, tol, "sim gemv %s nb %d" % ((N, K), nb))
    for (I, K) in KC.GEMV_SILU_SHAPES:
        for nb in (1, 2, 4, 8):                 # ... and of test_gemv_silu_mul_bound
            x, w = KC.gemm_inputs(nb, 2 * I, K, dtype, I + K + nb)
            gu = r(sim_acc(x, w), dtype)
            y = (r(gu[:, :I] * torch.sigmoid(gu[:, :I]), dtype) * gu[:, I:]).to(dtype)
            ref, tol = KC.silu_mul_bound(w, x, dtype)
            KC.check(y, ref, tol, "sim silu_mul %s nb %d" % ((I, K), nb))


@pytest.mark.parametrize("dtype", ALL, ids=lambda d: KC.NAME[d])
def test_simulated_conv_stays_inside_the_bound(dtype):
    for i, (B, Ci, Co, H, W, stride, up) in enumerate(KC.CONV_EDGE_CASES):
        x, w, bias, tv, res = KC.conv_inputs(B, Ci, Co, H, W, stride, up, dtype, i)
        for names in KC.CONV_VARIANTS:
            kw = {n: {"bias": bias, "rowvec": tv, "residual": res}[n] for n in names}
            ref, tol = KC.conv_bound(x, w, dtype, stride, up, **kw)
            KC.check(sim_conv(x, w, dtype, stride, up, **kw), ref, tol, "sim conv %s %s" % ((B, Ci, Co, H, W, stride, up), sorted(kw)))


@pytest.mark.parametrize("dtype", ALL, ids=lambda d: KC.NAME[d])
def test_simulated_attention_stays_inside_the_bound(dtype):
    worst = 0.0
    for i, (B, H, hd, Lq, Lk, causal) in enumerate(KC.ATTN_EDGE_CASES):
        q, k, v = KC.attn_inputs(B, H, hd, Lq, Lk, dtype, i)
        allow = KC.causal_allow(Lq, Lk) if causal else None
        scale = 1.0 / math.sqrt(hd)
        ref, tol = KC.attention_bound(KC.heads(q, H), KC.heads(k, H), KC.heads(v, H), scale, allow, dtype)
        y = sim_attention(KC.heads(q, H), KC.heads(k, H), KC.heads(v, H), scale, allow, dtype)
        worst = max(worst, KC.check(y, ref, tol, "sim attention %s" % ((B, H, hd, Lq, Lk, causal),)))
    for i, (H, hd, cap, M, lens) in enumerate(KC.ATTN_CACHE_CASES):
        for s, kvl in enumerate(lens):
            q, k, v = KC.attn_inputs(1, H, hd, M, kvl, dtype, 100 + 10 * i + s)
            allow = KC.causal_allow(M, kvl)
            ref, tol = KC.attention_bound(KC.heads(q, H), KC.heads(k, H), KC.heads(v, H), 1.0 / math.sqrt(hd), allow, dtype)
            y = sim_attention(KC.heads(q, H), KC.heads(k, H), KC.heads(v, H), 1.0 / math.sqrt(hd), allow, dtype)
            KC.check(y, ref, tol, "sim attention_cache %s kv_len %d" % ((H, hd, cap, M), kvl))
    print("simulated attention %s: worst error / bound %.3f" % (KC.NAME[dtype], worst))


@pytest.mark.parametrize("dtype", ALL, ids=lambda d: KC.NAME[d])
@pytest.mark.parametrize("hd", [64, 128])
def test_simulated_decode_stays_inside_the_bound(hd, dtype):
    H = KC.DECODE_HEADS
    for nsplit in KC.DECODE_NSPLITS:
        for kvl in KC.DECODE_KV_LENS:
            q, k, v = KC.attn_inputs(1, H, hd, 1, kvl, dtype, 200 + kvl)
            ref, tol = KC.attention_bound(KC.heads(q, H), KC.heads(k, H), KC.heads(v, H), 1.0 / math.sqrt(hd), None, dtype)
            # split-KV: a tile per split, merged like the combine kernel (same online-softmax algebra)
            tile = max(1, -(-kvl // (nsplit or 16)))
            y = sim_attention(KC.heads(q, H), KC.heads(k, H), KC.heads(v, H), 1.0 / math.sqrt(hd), None, torch.float32, tile=tile).to(dtype)
            KC.check(y, ref, tol, "sim decode hd %d nsplit %d kv_len %d" % (hd, nsplit, kvl))


# ---- exact probes: the simulated kernel reproduces them, a wrong k does not ------------------------------------------------------
@pytest.mark.parametrize("dtype", ALL, ids=lambda d: KC.NAME[d])
def test_exact_gemm_probes(dtype):
    for (M, N, K) in KC.GEMM_PROBE_SHAPES + [(129, 72, 64), (257, 330, 256), (256, 72, 448), (129, 330, 24), (37, 100, 256)]:
        idx = KC.boundary_indices(K)
        assert 0 in idx and K - 1 in idx and all((b - 1 in idx and b in idx) for s in (32, 64, 128) for b in range(s, K, s))
        for probe in (KC.selector_probe, KC.selector_probe_w, KC.counter_probe):
            a, w, exp = probe(M, N, K, dtype, seed=K)
            assert torch.equal(sim_gemm(a, w, dtype), exp), probe.__name__
            if K >= 16:
                a2 = a.clone()
                a2[:, K - 8:] = 0                      # the K tail dropped
                w2 = w.clone()
                w2[:, K - 8:] = 0
                assert not torch.equal(sim_gemm(a2, w2, dtype), exp), probe.__name__


@pytest.mark.parametrize("dtype", ALL, ids=lambda d: KC.NAME[d])
def test_exact_conv_impulse_probes(dtype):
    for i, (B, Ci, Co, H, W, stride, up) in enumerate(KC.CONV_IMPULSE_CASES):
        w = (torch.randint(-32, 32, (Co, Ci, 3, 3), generator=torch.Generator().manual_seed(i)) / 8.0).to(dtype)
        pos = KC.conv_impulse_positions(B, H, W)
        assert (0, 0, 0) in pos and (0, H - 1, W - 1) in pos and (B - 1, H - 1, W - 1) in pos and any(p[2] == W - 1 and 0 < p[1] < H - 1 for p in pos)
        for p in pos:
            x = KC.conv_impulse(B, Ci, H, W, p, (p[1] * 5 + p[2]) % Ci, dtype)
            exp = KC.conv_expected(x, w, dtype, stride, up)
            assert torch.equal(sim_conv(x, w, dtype, stride, up), exp)
            # an impulse at w = W - 1 must not reach column 0 of the next row
            if p[2] == W - 1 and stride == 1 and not up and p[1] + 1 < H:
                assert float(exp[p[0], :, p[1] + 1, 0].abs().sum()) == 0.0
                assert float(exp[p[0], :, p[1] + 1, W - 1].abs().sum()) > 0.0


@pytest.mark.parametrize("dtype", ALL, ids=lambda d: KC.NAME[d])
def test_exact_attention_selector(dtype):
    for (Lq, Lk, hd, causal) in [(15, 17, 64, False), (64, 128, 64, True), (65, 128, 128, True), (129, 129, 128, True), (17, 64, 104, False),
                                 (1, 1200, 128, False)]:
        q, k, v = KC.attention_selector(Lq, Lk, hd, dtype, seed=Lk)
        allow = KC.causal_allow(Lq, Lk) if causal else None
        exp = KC.attention_selector_expected(v, Lq, Lk, causal)
        assert torch.equal(sim_attention(q, k, v, 1.0, allow, dtype), exp)
        if causal and Lk > Lq:      # mask off by one: every query sees one key more
            wrong = torch.ones(Lq, Lk, dtype=torch.bool).tril(diagonal=Lk - Lq + 1)
            assert not torch.equal(sim_attention(q, k, v, 1.0, wrong, dtype), exp)
        # a key at index kv_len leaking in: Lk - 1 keys declared, the simulated kernel reads all Lk
        if Lk > Lq + 1:
            exp_short = KC.attention_selector_expected(v, Lq, Lk - 1, causal)
            short = None if allow is None else KC.causal_allow(Lq, Lk - 1)
            assert torch.equal(sim_attention(q, k[:, :Lk - 1], v[:, :Lk - 1], 1.0, short, dtype), exp_short)
            leak = torch.ones(Lq, Lk, dtype=torch.bool) if short is None else torch.cat([short, torch.ones(Lq, 1, dtype=torch.bool)], 1)
            assert not torch.equal(sim_attention(q, k, v, 1.0, leak, dtype), exp_short)


# ---- mutants ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mutant_case():
    dtype = torch.bfloat16
    M, N, K = 1024, 640, 1280
    a, w = KC.gemm_inputs(M, N, K, dtype, 99)
    ref, tol = KC.gemm_bound(a, w, dtype)
    y = sim_gemm(a, w, dtype)
    assert count(y, ref, tol) == 0
    return a, w, ref, tol, y


def test_mutant_zeroed_elements(mutant_case):
    a, w, ref, tol, y = mutant_case
    big = (ref.abs() > ref.abs().median()).nonzero()
    pick = big[torch.randperm(big.shape[0], generator=torch.Generator().manual_seed(1))[:8]]
    z = y.clone()
    z[pick[:, 0], pick[:, 1]] = 0
    assert count(z, ref, tol) == 8
    n, worst, coords = KC.violations(z, ref, tol)
    assert {c for c, _ in coords} <= {tuple(p.tolist()) for p in pick}
    _, msg = KC.report(z, ref, tol, "zeroed")
    assert "8 of %d" % ref.numel() in msg and "mod 16" in msg and "mod 256" in msg


def test_mutant_four_ulp_offsets(mutant_case):
    a, w, ref, tol, y = mutant_case
    g = torch.Generator().manual_seed(2)
    rows, cols = torch.randint(0, y.shape[0], (16,), generator=g), torch.randint(0, y.shape[1], (16,), generator=g)
    z = y.clone()
    bits = z.view(torch.int16)
    bits[rows, cols] += 4                 # 4 ulp away from zero
    assert count(z, ref, tol) >= 13


def test_mutant_dropped_k_tail_in_one_fragment(mutant_case):
    a, w, ref, tol, y = mutant_case
    K = a.shape[1]
    z = y.clone()
    a2 = a.clone()
    a2[:, K - 8:] = 0
    z[320:336, 160:176] = sim_gemm(a2[320:336], w[160:176], torch.bfloat16)
    n, worst, coords = KC.violations(z, ref, tol)
    assert n >= 128 and all(320 <= c[0] < 336 and 160 <= c[1] < 176 for c, _ in coords)


def test_mutant_swapped_adjacent_columns(mutant_case):
    a, w, ref, tol, y = mutant_case
    z = y.clone()
    z[64:80, 10], z[64:80, 11] = y[64:80, 11], y[64:80, 10]
    assert count(z, ref, tol) >= 24


def test_mutant_truncating_store(mutant_case):
    a, w, ref, tol, y = mutant_case
    z = sim_gemm(a, w, torch.bfloat16, trunc=True)
    assert count(z, ref, tol) > 0.005 * ref.numel()      # K = 1280: the accumulation term hides most of the extra half-ulp
    for dtype in (torch.bfloat16, torch.float16):       # K = 64: rounding dominates (u_T |v| is 1 .. 2 half-ulps: about a quarter of the truncated values exceed it)
        a16, w16 = KC.gemm_inputs(129, 72, 64, dtype, 3)
        r16, t16 = KC.gemm_bound(a16, w16, dtype)
        assert count(sim_gemm(a16, w16, dtype), r16, t16) == 0
        assert count(sim_gemm(a16, w16, dtype, trunc=True), r16, t16) > 0.15 * r16.numel()


def test_mutant_stale_row(mutant_case):
    a, w, ref, tol, y = mutant_case
    a_prev, _ = KC.gemm_inputs(a.shape[0], w.shape[0], a.shape[1], torch.bfloat16, 98)      # the previous case's operands
    z = y.clone()
    z[517] = sim_gemm(a_prev[517:518], w, torch.bfloat16)[0]
    n, worst, coords = KC.violations(z, ref, tol)
    assert n > 0.9 * y.shape[1] and all(c[0] == 517 for c, _ in coords)


@pytest.mark.parametrize("dtype", ALL, ids=lambda d: KC.NAME[d])
def test_guarded_out_catches_stray_and_missing_writes(dtype):
    def fresh(**kw):
        g = KC.GuardedOut(37, 72, dtype, **kw)
        g.out.copy_(torch.randn(37, 72).to(dtype))
        return g
    for kw in ({}, {"ld": 73}, {"ld": 80}, {"offset": 1}, {"ld": 80, "offset": 1}):
        g = fresh(**kw)
        assert g.flat.data_ptr() % 16 == 0 and (g.out.data_ptr() - g.flat.data_ptr()) % 16 == (kw.get("offset", 0) * g.out.element_size()) % 16
        pay = g.check("clean")
        assert torch.equal(pay, g.out.contiguous())
        g = fresh(**kw)
        g.flat.view(dtype)[g.start - 1] = 1.0                                    # one element before the payload
        assert any("BEFORE" in m for m in g.problems()[0])
        g = fresh(**kw)
        g.flat.view(dtype)[g.total - g.guard] = 0.0                              # the first element past the end
        assert any("PAST" in m for m in g.problems()[0])
        with pytest.raises(AssertionError):
            g.check("past")
        g = fresh(**kw)
        g.out[20, 71] = float("nan")                                             # an ordinary NaN is a written value, not the sentinel
        assert not g.problems()[0]
        g.flat[g.start + 20 * g.ld + 71] = KC.SENTINEL[dtype]                    # one payload element left unwritten
        msgs = g.problems()[0]
        assert len(msgs) == 1 and "never written" in msgs[0] and "(20, 71)" in msgs[0]
        if g.ld > g.width:
            g = fresh(**kw)
            g.flat.view(dtype)[g.start + 5 * g.ld + g.width] = 2.0               # one write into the gap after row 5
            msgs = g.problems()[0]
            assert len(msgs) == 1 and "gap" in msgs[0] and "row 5" in msgs[0]


def test_mutant_attention_mask_off_by_one_and_key_at_kv_len():
    dtype = torch.bfloat16
    H, hd, Lq, Lk = 2, 128, 65, 128
    q, k, v = KC.attn_inputs(1, H, hd, Lq, Lk + 1, dtype, 5)
    qh, kh, vh = KC.heads(q, H), KC.heads(k, H), KC.heads(v, H)
    scale = 1.0 / math.sqrt(hd)
    allow = KC.causal_allow(Lq, Lk)
    ref, tol = KC.attention_bound(qh, kh[:, :, :Lk], vh[:, :, :Lk], scale, allow, dtype)
    assert count(sim_attention(qh, kh[:, :, :Lk], vh[:, :, :Lk], scale, allow, dtype), ref, tol) == 0
    wrong = torch.ones(Lq, Lk, dtype=torch.bool).tril(diagonal=Lk - Lq + 1)
    assert count(sim_attention(qh, kh[:, :, :Lk], vh[:, :, :Lk], scale, wrong, dtype), ref, tol) > 0.2 * ref.numel()
    # non-causal: the key at index kv_len (one past the declared length) included
    ref, tol = KC.attention_bound(qh, kh[:, :, :Lk], vh[:, :, :Lk], scale, None, dtype)
    assert count(sim_attention(qh, kh[:, :, :Lk], vh[:, :, :Lk], scale, None, dtype), ref, tol) == 0
    assert count(sim_attention(qh, kh, vh, scale, None, dtype), ref, tol) > 0.2 * ref.numel()


def test_frobenius_norm_misses_what_the_bound_flags(mutant_case):
    """the finding this file exists for: the three small mutants pass `rel < 4e-3`"""
    a, w, ref, tol, y = mutant_case
    z = y.clone()
    z[100, 100:108] = 0
    rel = float((z.double() - ref).norm() / ref.norm())
    assert rel < 4e-3 and count(z, ref, tol) >= 7


# ==== norms, softmax, point-wise kernels, loss heads: simulated kernels ========================================================
def fsum(t, chunk=64):
    """fp32 sum over the last dim in chunks of `chunk`, last chunk first"""
    acc = torch.zeros(t.shape[:-1], dtype=torch.float32)
    for k0 in reversed(range(0, t.shape[-1], chunk)):
        acc = acc + t[..., k0:k0 + chunk].sum(-1)
    return acc


def f32(v):
    return torch.tensor(v, dtype=torch.float32)


def bump(y, idx, n=4):
    """y with element idx moved n ulps of T away from zero"""
    z = y.clone()
    v = z[idx].reshape(1)
    for _ in range(n):
        v = torch.nextafter(v, torch.full_like(v, float("inf")) * torch.sign(v.float()).to(v.dtype))
    z[idx] = v[0]
    return z


def sim_rmsnorm(x, w, eps, dtype, drop_last=False, trunc=False):
    x32, V = x.float(), KC.vec(dtype)
    sq = x32 * x32
    ss = fsum(sq[:, :-V] if drop_last else sq)
    rstd = 1.0 / torch.sqrt(ss / f32(x.shape[1]) + f32(eps))
    return r(w.float() * r(x32 * rstd[:, None], dtype), dtype, trunc).to(dtype)


def sim_layernorm(x, w, b, eps, dtype, drop_last=False, unbiased=False, onepass=False, trunc=False):
    x32, V = x.float(), KC.vec(dtype)
    cols = x.shape[1]
    xs = x32[:, :-V] if drop_last else x32
    mean = (fsum(xs) / f32(cols))[:, None]
    if onepass:
        var = fsum(xs * xs) / f32(cols) - mean[:, 0] * mean[:, 0]
    else:
        d = xs - mean
        var = fsum(d * d) / f32(cols - 1 if unbiased else cols)
    rstd = (1.0 / torch.sqrt(var + f32(eps)))[:, None]
    return r((x32 - mean) * rstd * w.float() + b.float(), dtype, trunc).to(dtype)


def prev_row_last_pack(y, dtype):
    z, V = y.clone(), KC.vec(dtype)
    z[1:, -V:] = y[:-1, -V:]
    return z


def sim_groupnorm(x, gw, gb, G, eps, silu_, dtype, group_of_pack=False, fp32_var=False):
    """the three passes: per-thread fp32 chains over a block's rows (stride rows-in-flight), the fold over the row lanes, fp64
    over channels and blocks, the fp32 apply.  group_of_pack: mutant, every channel of a pack takes the group of the pack's first
    channel.  fp32_var: mutant, E[x^2] - mean^2 in fp32."""
    B, HW, C = x.shape
    V, cg = KC.vec(dtype), C // G
    rpb = KC.groupnorm_rows_per_block(B, HW, C, dtype)
    x32 = x.float()
    S = torch.zeros(B, C, 2, dtype=torch.float64)
    for r0 in range(0, HW, rpb):
        r1 = min(HW, r0 + rpb)
        chs = torch.zeros(B, C, 2, dtype=torch.float32)
        for pc in range(0, C // V, 256):
            cw = min(256, C // V - pc)
            rip = 256 // cw
            c0, c1 = pc * V, (pc + cw) * V
            tot1 = tot2 = None
            for ry in range(rip):
                s1 = torch.zeros(B, c1 - c0)
                s2 = torch.zeros(B, c1 - c0)
                for rr in range(r0 + ry, r1, rip):
                    f = x32[:, rr, c0:c1]
                    s1 = s1 + f
                    s2 = s2 + f * f
                tot1 = s1 if tot1 is None else tot1 + s1
                tot2 = s2 if tot2 is None else tot2 + s2
            chs[:, c0:c1, 0], chs[:, c0:c1, 1] = tot1, tot2
        S += chs.double()
    Sg = S.view(B, G, cg, 2).sum(2)                                  # [B, G, 2] fp64
    inv_n = (f32(1.0) / (f32(HW) * f32(cg))).double()
    md = Sg[..., 0] * inv_n
    mean = md.float()
    if fp32_var:
        var = ((Sg[..., 1] * inv_n).float() - mean * mean).clamp_min(0.0)
    else:
        var = (Sg[..., 1] * inv_n - md * md).clamp_min(0.0).float()
    rstd = 1.0 / torch.sqrt(var + f32(eps))
    ch = torch.arange(C)
    gi = ((ch // V) * V // cg) if group_of_pack else ch // cg
    sc = rstd[:, gi] * gw.float()[None]
    sh = gb.float()[None] - mean[:, gi] * sc
    v = (x32.double() * sc.double()[:, None] + sh.double()[:, None]).float()          # fma: one rounding
    if silu_:
        v = r(v, dtype)
        v = v * (1.0 / (1.0 + torch.exp2(-1.4426950408889634 * v)))
    return v.to(dtype)


def sim_softmax(x, scale, dtype, skip_wave=None):
    V = KC.vec(dtype)
    s = x.float() * f32(scale)
    m = s.amax(1, keepdim=True)
    e = torch.exp(s - m)
    es = e
    if skip_wave is not None:            # mutant: the partial of one wave (threads 64 w .. 64 w + 63 own packs p with p % 256 in that range) is lost
        p = torch.arange(x.shape[1]) // V % 256
        es = e[:, (p // 64) != skip_wave]
    inv = 1.0 / fsum(es)
    return (e * inv[:, None]).to(dtype)


def silu32(g):
    return g / (1.0 + torch.exp(-g))


def sim_silu_mul(gu, dtype):
    I = gu.shape[1] // 2
    return (r(silu32(gu[:, :I].float()), dtype) * gu[:, I:].float()).to(dtype)


def sim_geglu(x, dtype):
    D = x.shape[1] // 2
    return (x[:, :D].float() * r(gelu32(x[:, D:].float()), dtype)).to(dtype)


def sim_l2norm(x, dtype):
    x32 = x.float()
    s = torch.zeros(x.shape[0], x.shape[2])
    for l in reversed(range(x.shape[1])):
        s = s + x32[:, l] * x32[:, l]
    nrm = torch.maximum(r(torch.sqrt(s), dtype), f32(1e-12))
    return (x32 / nrm[:, None]).to(dtype)


def sim_cross_entropy(logits, labels, vocab, dtype, ignore_index=-100):
    """logits [rows, ld]: only the first `vocab` columns are read"""
    x = logits[:, :vocab].float()
    m = x.amax(1)
    s = fsum(torch.exp(x - m[:, None]), chunk=256)
    lab = labels.clamp(0, vocab - 1)
    lsm = r(x.gather(1, lab[:, None])[:, 0] - m - torch.log(s), dtype)
    ok = labels != ignore_index
    return torch.where(ok, -lsm, torch.zeros_like(lsm)), ok.float()


def sim_cosine(rec, tgt, dtype):
    a, b = rec.float(), tgt.float()
    na, nb = r(torch.sqrt(fsum(a * a)), dtype), r(torch.sqrt(fsum(b * b)), dtype)
    p = r(r(b / nb[:, None], dtype) * r(a / na[:, None], dtype), dtype)
    return r(1.0 - r(fsum(p), dtype), dtype)


def sim_mse(a, b):
    d = a.float() - b.float()
    return ((d * d).double().sum() / a.numel()).float()


def sim_masked_mean(vals, mask):
    m = torch.ones_like(vals) if mask is None else mask
    c = m.double().sum()
    return ((vals * m).double().sum() / c).float() if c > 0 else f32(0.0)


def sim_euler_scale_dup(x, sigma, dtype):
    sg = f32(sigma)
    inv = 1.0 / torch.sqrt(sg * sg + 1.0)
    v = (x.float().flatten() * inv).to(dtype)
    return torch.stack([v, v])


# ---- zero violations on every listed case (the grid-stride shapes reduced to a small shape of the same family) -----------------
dt_ids = lambda d: KC.NAME[d]


@pytest.mark.parametrize("dtype", ALL, ids=dt_ids)
def test_simulated_norms_stay_inside_the_bound(dtype):
    V = KC.vec(dtype)
    worst_r = worst_l = 0.0
    cases = [(rows, p) for rows in KC.NORM_BLOCK_ROWS for p in KC.NORM_BLOCK_PACKS] + [(3, 63), (3, 65), (7, 64)]
    for i, (rows, packs) in enumerate(cases):
        x, w, b = KC.norm_inputs(rows, packs * V, dtype, i, zero_row=True)
        worst_r = max(worst_r, KC.check(sim_rmsnorm(x, w, KC.NORM_EPS, dtype), *KC.rmsnorm_bound(x, w, KC.NORM_EPS, dtype), "sim rmsnorm %s" % ((rows, packs),)))
        x, w, b = KC.norm_inputs(rows, packs * V, dtype, i)
        worst_l = max(worst_l, KC.check(sim_layernorm(x, w, b, KC.NORM_EPS, dtype), *KC.layernorm_bound(x, w, b, KC.NORM_EPS, dtype), "sim layernorm %s" % ((rows, packs),)))
    print("simulated rmsnorm / layernorm %s: worst error / bound %.3f / %.3f" % (KC.NAME[dtype], worst_r, worst_l))
    assert worst_r > 0.05 and worst_l > 0.05


@pytest.mark.parametrize("dtype", ALL, ids=dt_ids)
@pytest.mark.parametrize("silu_", [False, True], ids=["plain", "silu"])
def test_simulated_groupnorm_stays_inside_the_bound(silu_, dtype):
    worst = 0.0
    for i, (B, HW, C, G) in enumerate(KC.gn_cases(dtype)):
        for offset in ([False, True] if i == 1 else [False]):
            x, gw, gb = KC.gn_inputs(B, HW, C, dtype, i, offset)
            y = sim_groupnorm(x, gw, gb, G, KC.NORM_EPS, silu_, dtype)
            worst = max(worst, KC.check(y, *KC.groupnorm_bound(x, gw, gb, G, KC.NORM_EPS, silu_, dtype), "sim groupnorm %s offset %s" % ((B, HW, C, G), offset)))
    assert worst > 0.05


@pytest.mark.parametrize("dtype", ALL, ids=dt_ids)
def test_simulated_softmax_stays_inside_the_bound(dtype):
    V, worst = KC.vec(dtype), 0.0
    for i, (rows, packs) in enumerate((rows, p) for rows in KC.SOFTMAX_ROWS for p in KC.SOFTMAX_PACKS):
        for scale in KC.SOFTMAX_SCALES:
            x = KC.softmax_inputs(rows, packs * V, dtype, i)
            worst = max(worst, KC.check(sim_softmax(x, scale, dtype), *KC.softmax_rows_bound(x, scale, dtype), "sim softmax %s %s" % ((rows, packs), scale)))
    assert worst > 0.05


@pytest.mark.parametrize("dtype", ALL, ids=dt_ids)
def test_simulated_pointwise_stay_inside_the_bound(dtype):
    V = KC.vec(dtype)
    for i, (rows, inter) in enumerate(KC.gated_shapes(dtype)[:2] + [(5, 65 * V)]):
        x = KC.gated_inputs(rows, inter, dtype, i)
        KC.check(sim_silu_mul(x, dtype), *KC.silu_mul_ew_bound(x, dtype), "sim silu_mul")
        KC.check(sim_geglu(x, dtype), *KC.geglu_ew_bound(x, dtype), "sim geglu")
    for i, n in enumerate(KC.EW_N[:2] + [4099]):
        x = KC.gated_inputs(1, n, dtype, 10 + i)[0, :n]
        KC.check(silu32(x.float()).to(dtype), *KC.unary_bound(x, 0, dtype), "sim unary silu")
        KC.check(gelu32(x.float()).to(dtype), *KC.unary_bound(x, 1, dtype), "sim unary gelu")
        lat = KC.randn_t((n,), dtype, 20 + i)
        for sg, _ in KC.EULER_SIGMAS:
            KC.check(sim_euler_scale_dup(lat, sg, dtype), *KC.euler_scale_dup_bound(lat, sg, dtype), "sim euler_scale_dup")
    for i, (B, L, C) in enumerate(KC.L2_CASES):
        x = KC.randn_t((B, L, C), dtype, 30 + i)
        if C > 1:
            x[:, :, 1] = 0
        KC.check(sim_l2norm(x, dtype), *KC.l2normalize_bound(x, dtype), "sim l2normalize")


def ce_case(vocab, dtype, seed):
    rows = 5
    x = KC.randn_t((rows, vocab + KC.CE_PAD), dtype, 40 + seed, std=3.0)
    KC.poison_(x[:, vocab:])
    labels = torch.tensor([0, vocab - 1, -100, (vocab * 3) // 7, int(x[4, :vocab].float().argmax())])
    return x, labels


@pytest.mark.parametrize("dtype", ALL, ids=dt_ids)
def test_simulated_losses_stay_inside_the_bound(dtype):
    for i, vocab in enumerate(KC.CE_VOCABS):
        x, labels = ce_case(vocab, dtype, i)
        loss, valid = sim_cross_entropy(x, labels, vocab, dtype)
        ref, tol, vref = KC.cross_entropy_rows_bound(x[:, :vocab], labels, dtype)
        KC.check(loss, ref, tol, "sim cross-entropy vocab %d" % vocab)
        assert torch.equal(valid.double(), vref)
        # mutant: one column of the ld pad read
        assert count(sim_cross_entropy(x, labels, vocab + 1, dtype)[0], ref, tol) >= 4
    for i, (dim, rows) in enumerate((d, n) for d in KC.COSINE_DIMS for n in KC.COSINE_ROWS):
        a, b = KC.randn_t((rows, dim), dtype, 50 + i), KC.randn_t((rows, dim), dtype, 80 + i)
        KC.check(sim_cosine(a, b, dtype), *KC.cosine_rows_bound(a, b, dtype), "sim cosine %s" % ((rows, dim),))
    for i, n in enumerate(KC.MEAN_N):
        a, b = KC.randn_t((n,), dtype, 110 + i), KC.randn_t((n,), dtype, 120 + i)
        KC.check(sim_mse(a, b).reshape(1), *(t.reshape(1) for t in KC.mse_bound(a, b)), "sim mse %d" % n)
        if dtype == torch.float32:
            for mask in (None, (torch.arange(n) % 3 != 0).float(), torch.zeros(n)):
                ref, tol, cnt = KC.masked_mean_bound(a, mask)
                KC.check(sim_masked_mean(a, mask).reshape(1), ref.reshape(1), tol.reshape(1), "sim masked_mean %d" % n)
                assert cnt == (n if mask is None else float(mask.sum()))


# ---- seeded mutants -------------------------------------------------------------------------------------------------------------
def test_mutants_norm_statistics():
    eps = KC.NORM_EPS
    dtype = torch.float32
    V = KC.vec(dtype)
    # the last pack of a row left out of the statistic (3 x 255 packs, fp32; 16-bit rounding hides 4 of 1020 terms)
    x, w, b = KC.norm_inputs(3, 255 * V, dtype, 1, zero_row=True)
    ref, tol = KC.rmsnorm_bound(x, w, eps, dtype)
    assert count(sim_rmsnorm(x, w, eps, dtype), ref, tol) == 0
    assert count(sim_rmsnorm(x, w, eps, dtype, drop_last=True), ref, tol) > 0.3 * x.shape[1]
    x, w, b = KC.norm_inputs(3, 255 * V, dtype, 1)
    ref, tol = KC.layernorm_bound(x, w, b, eps, dtype)
    good = sim_layernorm(x, w, b, eps, dtype)
    assert count(good, ref, tol) == 0
    assert count(sim_layernorm(x, w, b, eps, dtype, drop_last=True), ref, tol) > 0.3 * x.shape[1]
    # fp32 E[x^2] - mean^2 on the offset row (|mean| / std = 100): the one-pass variance is off by u32 mean^2 / var = 6e-4
    # whatever the width, the bound's gamma_cols mean|x| grows with it: one pack per row is where the mutant stands out
    hits = 0
    for seed in (1, 2, 3, 4):
        x, w, b = KC.norm_inputs(3, V, dtype, seed)
        ref, tol = KC.layernorm_bound(x, w, b, eps, dtype)
        assert count(sim_layernorm(x, w, b, eps, dtype), ref, tol) == 0
        n, _, coords = KC.violations(sim_layernorm(x, w, b, eps, dtype, onepass=True), ref, tol)
        assert all(c[0] == 1 for c, _ in coords)
        hits += n
    assert hits >= 4
    # unbiased variance on a <= 256-column case, every dtype
    for dt_ in ALL:
        x, w, b = KC.norm_inputs(3, 256 if dt_ != torch.float32 else 252, dt_, 2)
        ref, tol = KC.layernorm_bound(x, w, b, eps, dt_)
        assert count(sim_layernorm(x, w, b, eps, dt_), ref, tol) == 0
        assert count(sim_layernorm(x, w, b, eps, dt_, unbiased=True), ref, tol) > (0.05 if dt_ == torch.bfloat16 else 0.2) * x.shape[1]
        # the last pack stored from the previous row
        n, _, coords = KC.violations(prev_row_last_pack(sim_layernorm(x, w, b, eps, dt_), dt_), ref, tol)
        assert n >= KC.vec(dt_) and all(c[1] >= x.shape[1] - KC.vec(dt_) for c, _ in coords)
        # a truncating store (16-bit) and a 4-ulp offset on one element
        x, w, b = KC.norm_inputs(3, 256 * KC.vec(dt_), dt_, 3, zero_row=True)
        ref, tol = KC.rmsnorm_bound(x, w, eps, dt_)
        y = sim_rmsnorm(x, w, eps, dt_)
        assert count(y, ref, tol) == 0
        if dt_ != torch.float32:        # one final round is all the LayerNorm bound grants (RMSNorm's mid round hides a truncation)
            xl, wl, bl = KC.norm_inputs(3, 256, dt_, 2)
            assert count(sim_layernorm(xl, wl, bl, eps, dt_, trunc=True), *KC.layernorm_bound(xl, wl, bl, eps, dt_)) > 0.1 * xl.shape[1]
        if dt_ != torch.float32:        # (4 fp32 ulps vanish under gamma_1024 of the statistic; test_mutants_softmax_and_pointwise bumps an fp32 element)
            n, _, coords = KC.violations(bump(y, (1, 77)), ref, tol)
            assert n == 1 and coords[0][0] == (1, 77)


def test_mutants_groupnorm():
    for dtype in ALL:
        B, HW, C, G = KC.gn_cases(dtype)[1]                 # cg = 10: group edges inside a pack
        x, gw, gb = KC.gn_inputs(B, HW, C, dtype, 1)
        ref, tol = KC.groupnorm_bound(x, gw, gb, G, KC.NORM_EPS, False, dtype)
        assert count(sim_groupnorm(x, gw, gb, G, KC.NORM_EPS, False, dtype), ref, tol) == 0
        assert count(sim_groupnorm(x, gw, gb, G, KC.NORM_EPS, False, dtype, group_of_pack=True), ref, tol) > 0.05 * ref.numel()
    # E[x^2] - mean^2 narrowed to fp32 before the subtraction errs by 2 u32 E[x^2]; the GroupNorm bound grants the fp32 chains
    # (gamma_k + 2 u32) E[x^2] on the same quantity, so THIS bound cannot tell the two apart (the two-pass LayerNorm bound does:
    # test_mutants_norm_statistics).  What it must do is stay valid on the offset data:
    dtype = torch.float32
    x, gw, gb = KC.gn_inputs(B, HW, C, dtype, 1, offset=True)
    ref, tol = KC.groupnorm_bound(x, gw, gb, G, KC.NORM_EPS, False, dtype)
    assert count(sim_groupnorm(x, gw, gb, G, KC.NORM_EPS, False, dtype), ref, tol) == 0


def test_mutants_softmax_and_pointwise():
    for dtype in ALL:
        V = KC.vec(dtype)
        x = KC.softmax_inputs(3, 257 * V, dtype, 7)
        ref, tol = KC.softmax_rows_bound(x, 0.3, dtype)
        y = sim_softmax(x, 0.3, dtype)
        assert count(y, ref, tol) == 0
        # one wave's partial missing from the normaliser: every entry of the random and the constant row grows by a quarter
        n, _, coords = KC.violations(sim_softmax(x, 0.3, dtype, skip_wave=1), ref, tol)
        assert n > 0.5 * x.shape[1]
        x = KC.gated_inputs(3, 33 * V, dtype, 1)
        ref, tol = KC.silu_mul_ew_bound(x, dtype)
        y = sim_silu_mul(x, dtype)
        assert count(y, ref, tol) == 0
        I = x.shape[1] // 2          # a positive gate: silu of a large negative one is a cancellation, and the evaluation term says so
        idx = (2, int(((x[2, :I].float() > 1) & (x[2, I:].float().abs() > 1)).nonzero()[0]))
        n, _, coords = KC.violations(bump(y, idx), ref, tol)
        assert n == 1 and coords[0][0] == idx
        if dtype != torch.float32:
            # a truncating store, where one final round is all the bound grants (the mid round of silu_mul hides it)
            ref, tol = KC.unary_bound(x, 0, dtype)
            assert count(silu32(x.float()).to(dtype), ref, tol) == 0
            assert count(trunc_to(silu32(x.float()), dtype).to(dtype), ref, tol) > 0.1 * ref.numel()


def test_mutants_exact_expectations():
    # a transpose that drops the ragged tile column
    x = KC.randn_t((45, 70), torch.bfloat16, 1)
    good = x.t().contiguous()
    z = torch.zeros_like(good)
    z[:64] = good[:64]
    assert not torch.equal(z, good) and torch.equal(x.t().contiguous(), good)
    # image_to_u8 rounding half up: 255 v is exact for a 16-bit v and then 127.5 is its only tie (-> 128 either way); an fp32 v
    # times 255 rounds onto other ties, and the listed inputs (the neighbours of every tie) reach them
    for dtype in ALL:
        x = KC.u8_inputs(349527, 8, dtype, 0)
        even, up = KC.image_to_u8_exact(x, 349527), KC.image_to_u8_exact(x, 349527, half_up=True)
        assert even[0, 0] == 0 and int(even.max()) == 255
        assert (dtype == torch.float32) == (not torch.equal(even, up))
    # the mirrors round where the kernel rounds: an fp64 evaluation rounded once differs on random data
    x, e = KC.randn_t((4099,), torch.bfloat16, 2), KC.randn_t((2, 4099), torch.bfloat16, 3)
    exact = KC.euler_cfg_step_exact(x, e, 7.5, *KC.EULER_SIGMAS[0])
    once = (x.double() + (e[0].double() + 7.5 * (e[1].double() - e[0].double())) * (KC.EULER_SIGMAS[0][1] - KC.EULER_SIGMAS[0][0])).to(torch.bfloat16)
    assert not torch.equal(exact, once)


def test_euler_fp16_fused_product_is_a_second_admissible_mirror():
    """the two fp16 mirrors of euler_cfg_step differ on a few elements in ten thousand at a 24-bit dsigma, check_exact admits either
    per element and still flags a third value"""
    n = 1048579
    x, e = KC.randn_t((n,), torch.float16, 2, std=3.0), KC.randn_t((2, n), torch.float16, 3)
    sg, sn = KC.EULER_SIGMAS[1]
    a, b = KC.euler_cfg_step_exact(x, e, 7.5, sg, sn), KC.euler_cfg_step_exact(x, e, 7.5, sg, sn, fused_f16=True)
    d = (a != b).nonzero().flatten()
    assert 0 < d.numel() < n // 2000
    mixed = a.clone()
    mixed[d[::2]] = b[d[::2]]
    KC.check_exact(mixed, a, "either", alt=b)
    with pytest.raises(AssertionError):
        KC.check_exact(mixed, a, "one mirror only")
    with pytest.raises(AssertionError):
        KC.check_exact(bump(mixed, int(d[0]), 1), a, "a third value", alt=b)
    with pytest.raises(AssertionError):
        KC.check_exact(bump(mixed, 5, 1), a, "elsewhere", alt=b)


def test_guarded_out_guards_only_mode():
    g = KC.GuardedOut(6, 16, torch.float16)
    g.out[2] = 1.0
    assert any("never written" in m for m in g.problems()[0])
    pay = g.check("rows in part", payload=False)
    assert g.untouched(pay)[[0, 1, 3, 4, 5]].all() and not g.untouched(pay)[2].any()
    g.flat[g.start - 1] = 0
    with pytest.raises(AssertionError):
        g.check("before", payload=False)


# ==== GEMM variants: fp8, LN-folded, statistics producers, split-K: simulated kernels ==========================================
BF = torch.bfloat16


def sim_fp8(a8, sa, w8, sw, drop=None):
    """fp32 accumulation of the code values (K tiles of 128, last first) -> (acc, fl(sa sw)); fp8_out applies the rest"""
    a, w = a8.view(KC.F8).float(), w8.view(KC.F8).float()
    acc = sim_acc(a, w, chunk=128)
    if drop is not None:                    # (rows, cols, k0): one K tile missing in one fragment
        rs, cs, k0 = drop
        a2 = a.clone()
        a2[:, k0:k0 + 128] = 0
        acc[rs, cs] = sim_acc(a2[rs], w[cs], chunk=128)
    return acc, sa.float()[:, None] * sw.float()[None, :]


def fp8_out(acc, s, trunc=False, **epi):
    """acc * fl(sa sw), the usual epilogue in bf16"""
    return sim_epilogue(acc * s, BF, trunc=trunc, **epi)


def sim_lnfold(acc, rstd, shift, colsum, dtype, skip=None, trunc=False, **epi):
    """fma(acc, rstd, fl(shift colsum)) (the product exact in fp64, one narrowing), the usual epilogue"""
    c = shift.float()[:, None] * colsum.float()[None, :]
    if skip is not None:
        c[skip] = 0.0
    t = (acc.double() * rstd.double()[:, None] + c.double()).float()
    return sim_epilogue(t, dtype, trunc=trunc, **{{"bias_d": "bias"}.get(k, k): v for k, v in epi.items()})


def sim_part_stats(part, width, eps):
    """the consumer's epilogue: fp64 sums 16 partials at a time, the fp32 1 / width, E[x^2] - mean^2 in fp64, fp32 narrowings"""
    a = torch.zeros(part.shape[0], dtype=torch.float64)
    b = torch.zeros_like(a)
    for k0 in range(0, part.shape[1], 16):
        for k in range(k0, min(k0 + 16, part.shape[1])):
            a, b = a + part[:, k, 0].double(), b + part[:, k, 1].double()
    iw = (torch.ones((), dtype=torch.float32) / torch.tensor(float(width), dtype=torch.float32)).double()
    mean = a * iw
    var = (b * iw - mean * mean).clamp_min(0.0)
    r = (1.0 / torch.sqrt(var + f32(eps).double())).float()
    return r, -mean.float() * r


def sim_finalize(acc, width, eps):
    mean = acc[:, 0] * (1.0 / width)
    var = (acc[:, 1] * (1.0 / width) - mean * mean).clamp_min(0.0)
    r = (1.0 / torch.sqrt(var + f32(eps).double())).float()
    return r, -mean.float() * r


def sim_rowstats(x, eps, cols=None):
    """two-pass fp32 statistics (cols: the mutant that stops short)"""
    xf = x.float()[:, :cols]
    n = f32(float(x.shape[1]))
    mean = fsum(xf, 8) / n
    d = xf - mean[:, None]
    r = 1.0 / torch.sqrt(fsum(d * d, 8) / n + f32(eps))
    return r, -mean * r


def sim_rowsums(y, tn):
    """per-strip fp32 (sum, sum of squares) of the stored rows: 8-wide pieces, folded last piece first -> [M, N / tn, 2]"""
    ys = y.float().view(y.shape[0], y.shape[1] // tn, tn)
    return torch.stack([fsum(ys, 8), fsum(ys * ys, 8)], 2)


def sim_splitk(a, w, dtype, S, bias=None, residual=None, drop=None, twice=None):
    """one fp32 accumulator per K range (stored exactly), the slices added in fp32 in order, the epilogue of the reduce kernel"""
    tot = torch.zeros(a.shape[0], w.shape[0], dtype=torch.float32)
    for i, (k0, k1) in enumerate(KC.splitk_ranges(a.shape[1], S)):
        p = sim_acc(a[:, k0:k1], w[:, k0:k1], chunk=64) if k1 > k0 else torch.zeros_like(tot)
        if i == drop:
            continue
        tot = tot + p + (p if i == twice else 0.0)
    return sim_epilogue(tot, dtype, bias=bias, residual=residual)


def sim_quant_ln(x, g, b, eps, dtype):
    """quantize_rows_fp8(x, ln=): fp32 two-pass LayerNorm rounded to T, amax, s = amax / 448, q = RNE_e4m3(o (448 / amax))"""
    xf, n = x.float(), f32(float(x.shape[1]))
    mean = fsum(xf, 8) / n
    d = xf - mean[:, None]
    rstd = 1.0 / torch.sqrt(fsum(d * d, 8) / n + f32(eps))
    o = r(d * rstd[:, None] * g.float() + b.float(), dtype)
    amax = o.abs().amax(1)
    inv = torch.where(amax > 0, f32(448.0) / amax, torch.zeros_like(amax))
    return (o * inv[:, None]).to(KC.F8).view(torch.uint8), amax / 448.0


# ---- zero violations on every case of tests/test_gemm_variants_edges_gpu.py -------------------------------------------------------
@pytest.mark.parametrize("cfg", KC.FP8_TILES)
def test_simulated_fp8_gemm_stays_inside_the_bound(cfg):
    """the inputs of test_fp8_gemm_bound_every_tile[cfg] and test_fp8_gemm_strides_and_alignment[cfg] (same seed functions)"""
    worst = 0.0
    for i, (M, N, K) in enumerate(KC.FP8_SHAPES):
        q = KC.fp8_inputs(M, N, K, KC.fp8_seeds(cfg, i, 0)[0])
        acc, s = sim_fp8(*q)
        for j, epi in enumerate(KC.FP8_EPILOGUES):
            kw = KC.epilogue_inputs(epi, M, N, BF, KC.fp8_seeds(cfg, i, j)[1])
            ref, tol = KC.gemm_fp8_bound(*q, **kw)
            worst = max(worst, KC.check(fp8_out(acc, s, **kw), ref, tol, "sim fp8 cfg %d %s %s" % (cfg, epi, (M, N, K))))
    M, N, K = KC.FP8_STRIDE_SHAPE
    for c, (_, _, geglu) in enumerate(KC.FP8_STRIDE_CASES):
        q = KC.fp8_inputs(M, N, K, KC.fp8_stride_seed(cfg, c))
        kw = KC.epilogue_inputs("geglu" if geglu else "bias+residual", M, N, BF, KC.fp8_stride_seed(cfg, c))
        ref, tol = KC.gemm_fp8_bound(*q, **kw)
        KC.check(fp8_out(*sim_fp8(*q), **kw), ref, tol, "sim fp8 strided cfg %d case %d" % (cfg, c))
    print("simulated fp8 gemm, inputs of cfg %d: worst error / bound %.3f" % (cfg, worst))
    assert worst > 0.05


def test_exact_fp8_probes():
    for (M, N, K) in KC.FP8_PROBE_SHAPES:
        for kind in ("selector", "selector_w", "counter"):
            a8, sa, w8, sw, exp = KC.fp8_probe(kind, M, N, K, seed=K)
            # the operands quantise exactly: the quantiser gives these bytes and scales back from the de-quantised matrices
            for q, s in ((a8, sa), (w8, sw)):
                q2, s2 = KC.quantize_rows_e4m3((KC.f8_values(q) * s.double()[:, None]).float())
                assert torch.equal(q2, q) and torch.equal(s2, s), kind
            assert torch.equal(fp8_out(*sim_fp8(a8, sa, w8, sw)), exp), kind
            w2 = w8.clone()
            w2[:, K - 8:] = 0                                  # the K tail dropped
            a2 = a8.clone()
            a2[:, K - 8:] = 0
            assert not torch.equal(fp8_out(*sim_fp8(a2, sa, w2, sw)), exp), kind


def lnfold_kw(epi, bias_d):
    return dict(bias_d=None if epi == "plain" else bias_d, gelu_=epi == "gelu", geglu=epi == "geglu")


@pytest.mark.parametrize("dtype", DTYPES16, ids=lambda d: KC.NAME[d])
@pytest.mark.parametrize("cfg", KC.LNFOLD_TILES)
def test_simulated_lnfold_gemm_stays_inside_the_bound(cfg, dtype):
    """the inputs of test_lnfold_gemm_bound_every_tile[cfg] (statistics from the simulated ss_rowstats, handed over as the
    kernel's inputs) and of test_lnfold_part_gemm_bound_every_tile[cfg] (statistics from partials, known to a tolerance; the
    shape the library refuses is simulated all the same)"""
    worst = 0.0
    for i, (M, N, K) in enumerate(KC.LNFOLD_SHAPES):
        x, wg, colsum, bias_d = KC.lnfold_inputs(M, N, K, dtype, KC.lnfold_seed(cfg, i))
        acc = sim_acc(x, wg, chunk=64)
        rstd, shift = sim_rowstats(x, KC.LN_EPS)
        for epi in KC.LNFOLD_EPILOGUES:
            kw = lnfold_kw(epi, bias_d)
            ref, tol = KC.gemm_lnfold_bound(x, wg, rstd, shift, colsum, dtype, **kw)
            worst = max(worst, KC.check(sim_lnfold(acc, rstd, shift, colsum, dtype, **kw), ref, tol, "sim lnfold cfg %d %s %s" % (cfg, epi, (M, N, K))))
    for i, (M, N, K) in enumerate(KC.LNFOLD_PART_SHAPES):
        x, wg, colsum, bias_d = KC.lnfold_inputs(M, N, K, dtype, KC.lnfold_seed(cfg, i, part=True))
        lnfold_part_case(x, wg, colsum, bias_d, KC.lnfold_parts(x), K, dtype, KC.LNFOLD_EPILOGUES, "sim lnfold_part cfg %d %s" % (cfg, (M, N, K)))
    print("simulated lnfold, inputs of cfg %d %s: worst error / bound %.3f" % (cfg, KC.NAME[dtype], worst))
    assert worst > 0.05


def lnfold_part_case(x, wg, colsum, bias_d, part, width, dtype, epis, what):
    (rv, rt), (sv, st) = KC.lnfold_part_stats_bound(part, width, KC.LN_EPS)
    r2, s2 = sim_part_stats(part, width, KC.LN_EPS)
    KC.check(r2, rv, rt, what + " rstd")
    KC.check(s2, sv, st, what + " shift")
    acc = sim_acc(x, wg, chunk=64)
    for epi in epis:
        kw = lnfold_kw(epi, bias_d)
        ref, tol = KC.gemm_lnfold_bound(x, wg, rv, sv, colsum, dtype, t_rstd=rt, t_shift=st, **kw)
        KC.check(sim_lnfold(acc, r2, s2, colsum, dtype, **kw), ref, tol, what + " " + epi)


@pytest.mark.parametrize("dtype", DTYPES16, ids=lambda d: KC.NAME[d])
def test_simulated_lnfold_part_alignment_and_chain_cases_stay_inside_the_bound(dtype):
    """the one launch test_lnfold_part_refuses_what_the_staged_epilogue_cannot_take lets through, and the producer -> consumer
    chain of test_producer_partials_into_folded_consumer (the producer's strips are 64 or 80 wide there)"""
    M, N, K, seed = KC.LNFOLD_REFUSAL_CASE
    x, wg, colsum, bias_d = KC.lnfold_inputs(M, N, K, dtype, seed)
    lnfold_part_case(x, wg, colsum, bias_d, KC.lnfold_parts(x), K, dtype, ["bias"], "sim lnfold_part aligned")
    for (M, N, K, seed) in KC.PRODUCER_CHAIN_CASES:
        a, w, bias, res = KC.producer_inputs(M, N, K, dtype, seed)
        y = sim_gemm(a, w, dtype, bias=bias, residual=res)
        _, wg, colsum, bias_d = KC.lnfold_inputs(8, 160, N, dtype, seed)
        lnfold_part_case(y, wg, colsum, bias_d, sim_rowsums(y, 64 if N % 80 else 80), N, dtype, ["bias"], "sim chain %s" % ((M, N, K),))


@pytest.mark.parametrize("dtype", DTYPES16, ids=lambda d: KC.NAME[d])
def test_simulated_rowstats_and_finalize_stay_inside_the_bound(dtype):
    for i, (M, K) in enumerate(KC.ROWSTATS_SHAPES):
        x = KC.lnfold_inputs(M, 16, K, dtype, 50 + i)[0]
        (rv, rt), (sv, st) = KC.rowstats_bound(x, KC.LN_EPS, dtype)
        r1, s1 = sim_rowstats(x, KC.LN_EPS)
        KC.check(r1, rv, rt, "sim rowstats rstd %s" % ((M, K),))
        KC.check(s1, sv, st, "sim rowstats shift %s" % ((M, K),))
        xd = x.double()
        acc = torch.stack([xd.sum(1), (xd * xd).sum(1)], 1)
        (rv, rt), (sv, st) = KC.rowstat_finalize_bound(acc, K, KC.LN_EPS)
        r2, s2 = sim_finalize(acc, K, KC.LN_EPS)
        KC.check(r2, rv, rt, "sim finalize rstd")
        KC.check(s2, sv, st, "sim finalize shift")


@pytest.mark.parametrize("dtype", DTYPES16, ids=lambda d: KC.NAME[d])
def test_simulated_producer_sums_stay_inside_the_bound(dtype):
    for fallback, (i, (M, N, K)) in [(f, c) for f in (0, 1) for c in enumerate(KC.PRODUCER_SHAPES)]:
        a, w, bias, res = KC.producer_inputs(M, N, K, dtype, KC.producer_seed(fallback, i))
        for residual in (None, res):
            y = sim_gemm(a, w, dtype, bias=bias, residual=residual)
            ref, tol = KC.gemm_bound(a, w, dtype, bias=bias, residual=residual)
            KC.check(y, ref, tol, "sim producer %s" % ((M, N, K),))
            for tn in (8, 64, 80):
                if N % tn:
                    continue
                part = sim_rowsums(y, tn)
                (s1, t1), (s2, t2) = KC.rowsum_bound(y, tn)
                KC.check(part[:, :, 0], s1, t1, "sim strip sums")
                KC.check(part[:, :, 1], s2, t2, "sim strip squares")
            part = sim_rowsums(y, 8).double().sum(1)            # the accumulator form: fp32 pieces added in fp64
            (s1, t1), (s2, t2) = KC.rowsum_bound(y)
            KC.check(part[:, 0], s1, t1, "sim row sums")
            KC.check(part[:, 1], s2, t2, "sim row squares")


@pytest.mark.parametrize("dtype", DTYPES16, ids=lambda d: KC.NAME[d])
def test_simulated_splitk_stays_inside_the_bound(dtype):
    for i, (M, N, K) in enumerate(KC.SPLITK_SHAPES):
        for S in KC.SPLITK_S:
            a, w = KC.gemm_inputs(M, N, K, dtype, KC.splitk_seed(i, S))
            for epi in KC.SPLITK_EPILOGUES:
                kw = KC.epilogue_inputs(epi, M, N, dtype, KC.splitk_seed(i, S))
                Su = S or KC.splitk_planned(M, N, K)
                ref, tol = KC.gemm_splitk_bound(a, w, dtype, Su, **kw)
                KC.check(sim_splitk(a, w, dtype, Su, **kw), ref, tol, "sim splitk %s S %d %s" % ((M, N, K), Su, epi))
    assert [KC.splitk_planned(*s) for s in KC.SPLITK_SHAPES] == [2, 2, 4]
    assert KC.splitk_ranges(1088, 8)[-2:] == [(1088, 1088)] * 2 and KC.splitk_ranges(1024, 3) == [(0, 384), (384, 768), (768, 1024)]


@pytest.mark.parametrize("dtype", DTYPES16, ids=lambda d: KC.NAME[d])
def test_simulated_ln_quantiser_stays_inside_the_bound(dtype):
    for i, (M, K) in enumerate(KC.QUANT_LN_SHAPES):
        x, g, b = KC.norm_inputs(M, K, dtype, 70 + i)
        (v, tq), (s, ts) = KC.quantize_ln_bound(x, g, b, KC.LN_EPS, dtype)
        q, sc = sim_quant_ln(x, g, b, KC.LN_EPS, dtype)
        KC.check(sc, s, ts, "sim ln quantiser scale %s" % ((M, K),))
        KC.check(KC.f8_values(q) * sc.double()[:, None], v, tq, "sim ln quantiser q * s %s" % ((M, K),))
        q2 = q.clone()
        q2[M // 2, K - 1] ^= 2                                   # two code steps away
        assert count(KC.f8_values(q2) * sc.double()[:, None], v, tq) == 1
        assert count(sc * 1.01, s, ts) >= M - 2                  # a scale 1 % off (bf16 leaves amax 0.4 %; the offset and the
        #                                                          constant row pay for their fp32 mean and are wider)


# ---- mutants ------------------------------------------------------------------------------------------------------------------
def inside(coords, rows, cols):
    return all(rows.start <= c[0] < rows.stop and cols.start <= c[1] < cols.stop for c, _ in coords)


def test_mutants_fp8():
    M, N, K = 257, 160, 640
    a8, sa, w8, sw = KC.fp8_inputs(M, N, K, 7)
    kw = KC.epilogue_inputs("bias", M, N, BF, 7)
    ref, tol = KC.gemm_fp8_bound(a8, sa, w8, sw, **kw)
    acc, s = sim_fp8(a8, sa, w8, sw)
    assert count(fp8_out(acc, s, **kw), ref, tol) == 0
    rows, cols = slice(64, 80), slice(32, 48)
    # one K tile dropped in one 16x16 fragment
    n, _, coords = KC.violations(fp8_out(*sim_fp8(a8, sa, w8, sw, drop=(rows, cols, 256)), **kw), ref, tol)
    assert n >= 128 and inside(coords, rows, cols)
    # scale_w shifted by one column in one 4-column group
    s2 = s.clone()
    s2[rows, 36:40] = s[rows, 37:41]
    n, _, coords = KC.violations(fp8_out(acc, s2, **kw), ref, tol)
    assert n >= 16 and inside(coords, rows, slice(36, 40))
    # scale_a taken from row m + 16
    s2 = s.clone()
    s2[rows, cols] = s[80:96, cols]
    n, _, coords = KC.violations(fp8_out(acc, s2, **kw), ref, tol)
    assert n >= 200 and inside(coords, rows, cols)
    # a truncating store (K = 128: the rounding dominates)
    a8, sa, w8, sw = KC.fp8_inputs(257, 208, 128, 8)
    ref, tol = KC.gemm_fp8_bound(a8, sa, w8, sw)
    assert count(fp8_out(*sim_fp8(a8, sa, w8, sw)), ref, tol) == 0
    assert count(fp8_out(*sim_fp8(a8, sa, w8, sw), trunc=True), ref, tol) > 0.15 * ref.numel()


@pytest.mark.parametrize("dtype", DTYPES16, ids=lambda d: KC.NAME[d])
def test_mutants_lnfold(dtype):
    M, N, K = 257, 640, 192
    x, wg, colsum, bias_d = KC.lnfold_inputs(M, N, K, dtype, 9)
    rstd, shift = sim_rowstats(x, KC.LN_EPS)
    ref, tol = KC.gemm_lnfold_bound(x, wg, rstd, shift, colsum, dtype, bias_d=bias_d)
    acc = sim_acc(x, wg, chunk=64)
    assert count(sim_lnfold(acc, rstd, shift, colsum, dtype, bias_d=bias_d), ref, tol) == 0
    rows, cols = slice(64, 80), slice(32, 48)
    # one K tile dropped in one 16x16 fragment
    x2 = x.clone()
    x2[:, 64:128] = 0
    acc2 = acc.clone()
    acc2[rows, cols] = sim_acc(x2[rows], wg[cols], chunk=64)
    n, _, coords = KC.violations(sim_lnfold(acc2, rstd, shift, colsum, dtype, bias_d=bias_d), ref, tol)
    assert n >= 128 and inside(coords, rows, cols)
    # colsum shifted by one column in one 4-column group
    y = sim_lnfold(acc, rstd, shift, colsum, dtype, bias_d=bias_d)
    cs2 = colsum.clone()
    cs2[36:40] = colsum[37:41]
    z = y.clone()
    z[rows, 36:40] = sim_lnfold(acc, rstd, shift, cs2, dtype, bias_d=bias_d)[rows, 36:40]
    n, _, coords = KC.violations(z, ref, tol)
    assert n >= 32 and inside(coords, rows, slice(36, 40))
    # rstd taken from row m + 16
    r2 = rstd.clone()
    r2[rows] = rstd[80:96]
    z = y.clone()
    z[rows, cols] = sim_lnfold(acc, r2, shift, colsum, dtype, bias_d=bias_d)[rows, cols]
    n, _, coords = KC.violations(z, ref, tol)
    assert n >= 64 and inside(coords, rows, cols)
    # shift * colsum omitted for one element (row 65: |mean| ~ 9 std, the term the product cancels against)
    skip = torch.zeros(M, N, dtype=torch.bool)
    skip[65, 37] = True
    n, _, coords = KC.violations(sim_lnfold(acc, rstd, shift, colsum, dtype, skip=skip, bias_d=bias_d), ref, tol)
    assert n == 1 and coords[0][0] == (65, 37)
    # a truncating store (K = 64)
    x, wg, colsum, bias_d = KC.lnfold_inputs(129, 160, 64, dtype, 10)
    rstd, shift = sim_rowstats(x, KC.LN_EPS)
    ref, tol = KC.gemm_lnfold_bound(x, wg, rstd, shift, colsum, dtype)
    assert count(sim_lnfold(sim_acc(x, wg), rstd, shift, colsum, dtype), ref, tol) == 0
    assert count(sim_lnfold(sim_acc(x, wg), rstd, shift, colsum, dtype, trunc=True), ref, tol) > 0.15 * ref.numel()


@pytest.mark.parametrize("dtype", DTYPES16, ids=lambda d: KC.NAME[d])
def test_mutants_statistics(dtype):
    M, N, K = 257, 640, 192
    a, w, bias, res = KC.producer_inputs(M, N, K, dtype, 11)
    y = sim_gemm(a, w, dtype, bias=bias, residual=res)
    part = sim_rowsums(y, 80)
    (s1, t1), (s2, t2) = KC.rowsum_bound(y, 80)
    assert count(part[:, :, 0], s1, t1) == 0 and count(part[:, :, 1], s2, t2) == 0
    # one stale strip partial (the previous case's)
    a0, w0, b0, r0 = KC.producer_inputs(M, N, K, dtype, 10)
    stale = part.clone()
    stale[100, 3] = sim_rowsums(sim_gemm(a0, w0, dtype, bias=b0, residual=r0), 80)[100, 3]
    n, _, coords = KC.violations(stale[:, :, 0], s1, t1)
    assert n == 1 and coords[0][0] == (100, 3) and count(stale[:, :, 1], s2, t2) == 1
    # ... and what the consumer makes of it
    (rv, rt), (sv, st) = KC.lnfold_part_stats_bound(part, N, KC.LN_EPS)
    r2, sh2 = sim_part_stats(stale, N, KC.LN_EPS)
    assert KC.violations(r2, rv, rt)[2][0][0] == (100,) and count(sh2, sv, st) == 1
    # a statistics row that misses its last 8 columns: the accumulator form, the strip form, ss_rowstats
    short = sim_rowsums(y, 8)
    short[77, -1] = 0.0
    (a1, ta1), (a2, ta2) = KC.rowsum_bound(y)
    full = sim_rowsums(y, 8).double().sum(1)
    assert count(full[:, 0], a1, ta1) == 0 and count(full[:, 1], a2, ta2) == 0
    sh = short.double().sum(1)
    assert KC.violations(sh[:, 0], a1, ta1)[2][0][0] == (77,) and count(sh[:, 1], a2, ta2) == 1
    x = y
    (rv, rt), (sv, st) = KC.rowstats_bound(x, KC.LN_EPS, dtype)
    r1, sh1 = sim_rowstats(x, KC.LN_EPS)
    assert count(r1, rv, rt) == 0 and count(sh1, sv, st) == 0
    r3, sh3 = sim_rowstats(x[77:78], KC.LN_EPS, cols=N - 8)
    r1[77], sh1[77] = r3[0], sh3[0]
    assert count(r1, rv, rt) == 1 and count(sh1, sv, st) == 1
    # finalize with the wrong width (N + 1): every row's statistics move by 1 / N, far outside the finalize bound
    yd = y.double()
    acc = torch.stack([yd.sum(1), (yd * yd).sum(1)], 1)
    (rv, rt), (sv, st) = KC.rowstat_finalize_bound(acc, N, KC.LN_EPS)
    assert count(sim_finalize(acc, N, KC.LN_EPS)[0], rv, rt) == 0
    wrong = sim_finalize(acc, N + 1, KC.LN_EPS)
    assert count(wrong[0], rv, rt) > 0.9 * M


@pytest.mark.parametrize("dtype", DTYPES16, ids=lambda d: KC.NAME[d])
def test_mutants_splitk(dtype):
    M, N, K = 257, 128, 1088
    a, w = KC.gemm_inputs(M, N, K, dtype, 12)
    kw = KC.epilogue_inputs("bias+residual", M, N, dtype, 12)
    for S in (2, 8):
        ref, tol = KC.gemm_splitk_bound(a, w, dtype, S, **kw)
        assert count(sim_splitk(a, w, dtype, S, **kw), ref, tol) == 0
        # one slice dropped / added twice (the last non-empty one: 2 of 17 K tiles at S = 8)
        last = max(i for i, (k0, k1) in enumerate(KC.splitk_ranges(K, S)) if k1 > k0)
        assert count(sim_splitk(a, w, dtype, S, drop=last, **kw), ref, tol) > 0.8 * ref.numel()
        assert count(sim_splitk(a, w, dtype, S, twice=last, **kw), ref, tol) > 0.8 * ref.numel()
        # one K tile dropped in one 16x16 fragment
        a2 = a.clone()
        a2[:, 1024:] = 0
        z = sim_splitk(a, w, dtype, S, **kw)
        z[64:80, 32:48] = sim_splitk(a2[64:80], w[32:48], dtype, S, bias=kw["bias"][32:48], residual=kw["residual"][64:80, 32:48])
        n, _, coords = KC.violations(z, ref, tol)
        assert n >= 128 and inside(coords, slice(64, 80), slice(32, 48))
        # the counter probe spans every K range: a range taken twice or never changes the integer
        ca, cw, exp = KC.counter_probe(M, N, K, dtype, seed=S)
        assert torch.equal(sim_splitk(ca, cw, dtype, S), exp)
        for i, (k0, k1) in enumerate(KC.splitk_ranges(K, S)):
            if k1 > k0:
                assert not torch.equal(sim_splitk(ca, cw, dtype, S, drop=i), exp)
                assert not torch.equal(sim_splitk(ca, cw, dtype, S, twice=i), exp)


# ---- the decode step (tests/test_decode_step_gpu.py): the simulated kernel on every case, and the mutants ----------------------
import types

import kv8_ref

STEP_MUTANTS = {
    # mutant -> the assertions of KC.decode_step_failures / the selector probes that must flag it
    "skip new key": {"bound", "selector"},              # the new key is never attended
    "new key twice": {"bound"},                         # attended by two key groups (a split boundary owned twice)
    "row + 1": {"append", "untouched"},                 # the new row stored at n_old + 1
    "done appends": {"untouched"},                      # a finished sequence stores its row all the same
    "previous kv_len": {"bound", "append", "untouched"},        # sequence b reads sequence b - 1's kv_len word
    "pos from kv_len": {"bound", "append"},             # the RoPE position taken from the kv_len word
    "stride without gap": {"bound", "append", "untouched"},     # cache_stride = H cap hd: later sequences miss their planes
    "kv8 quantised new key": {"bound", "selector"},     # shadow: the new key attended from its codes
    "kv8 scale row - 1": {"shadow append", "shadow untouched"},  # shadow: the new row's scales written one row early
}


def sim_decode_step(inp, cos, sin, ns, mutant=None):
    """attn_decode_kernel / attn_decode_kv8_kernel in their fused, batched mode, restated in fp32 torch over the flat buffers of
    KC.decode_step_pack: per sequence the state words, RoPE of q and the new k, the append, then per split the chunk
    [sp * chunk, (sp + 1) * chunk) of the n_old + 1 keys walked by NKG key groups (keys kg, kg + NKG, ... with a private online
    softmax each; the 16-bit kernel meets the new key in that order, the shadow kernel after its loop, unquantised, scales 1),
    the merge of the groups into the split's record and the merge of the records.  -> the `got` of KC.decode_step_failures."""
    dtype, H, cap, hd, nb, shadow = inp.dtype, inp.H, inp.cap, inp.hd, inp.nb, inp.shadow
    V = 16 if shadow else (4 if dtype == torch.float32 else 8)
    NKG = 256 // (hd // V)
    E = H * hd
    scale = torch.tensor(1.0 / math.sqrt(hd), dtype=torch.float32)
    stride = inp.plane if mutant == "stride without gap" else inp.cache_stride
    got = types.SimpleNamespace(out=torch.zeros(nb, E, dtype=dtype), written=torch.zeros(nb, E, dtype=torch.bool), kflat=inp.kflat.clone(),
                                vflat=inp.vflat.clone(), state=inp.state.clone())
    if shadow:
        got.kq, got.vq, got.ks, got.vs = inp.kq.clone(), inp.vq.clone(), inp.ks.clone(), inp.vs.clone()
    rows = inp.qkv.view(nb, 3, H, hd)
    f8 = lambda c: c.view(torch.float8_e4m3fn).float()
    for b in range(nb):
        st = inp.state[b]
        n_old = int(inp.state[b - 1 if mutant == "previous kv_len" and b else b][KC.ST_KV_LEN])
        pos = int(st[KC.ST_KV_LEN if mutant == "pos from kv_len" else KC.ST_POS])
        if st[KC.ST_DONE] and mutant != "done appends":
            continue
        p1 = torch.tensor([pos])
        q = KC.rope_exact(rows[b:b + 1, 0], cos, sin, p1)[0].float()
        k_new = KC.rope_exact(rows[b:b + 1, 1], cos, sin, p1)[0]
        v_new = rows[b, 2]
        base = b * stride
        if n_old < cap:
            row = n_old + (1 if mutant == "row + 1" else 0)
            for h in range(H):
                o = base + (h * cap + row) * hd
                got.kflat[o:o + hd], got.vflat[o:o + hd] = k_new[h], v_new[h]
                if shadow:
                    got.kq[o:o + hd], ksc, _ = kv8_ref.quantize(k_new[h])
                    got.vq[o:o + hd], vsc, _ = kv8_ref.quantize(v_new[h])
                    so = o // hd - (1 if mutant == "kv8 scale row - 1" and n_old else 0)
                    got.ks[so], got.vs[so] = ksc, vsc
        if st[KC.ST_DONE]:
            continue
        # the old keys as the kernel reads them, the new one from registers
        if shadow:
            sbase = base // hd
            k_old = f8(inp.kq[base:base + inp.plane].view(H, cap, hd)[:, :n_old])
            v_old = f8(inp.vq[base:base + inp.plane].view(H, cap, hd)[:, :n_old])
            ksc = torch.cat([inp.ks[sbase:sbase + H * cap].view(H, cap)[:, :n_old], torch.ones(H, 1)], 1)
            vsc = torch.cat([inp.vs[sbase:sbase + H * cap].view(H, cap)[:, :n_old], torch.ones(H, 1)], 1)
            kn, vn = k_new, v_new
            if mutant == "kv8 quantised new key":
                kn, vn = kv8_ref.quantize(k_new)[2], kv8_ref.quantize(v_new)[2]
        else:
            k_old = inp.kflat[base:base + inp.plane].view(H, cap, hd)[:, :n_old].float()
            v_old = inp.vflat[base:base + inp.plane].view(H, cap, hd)[:, :n_old].float()
            ksc = vsc = torch.ones(H, n_old + 1)
            kn, vn = k_new, v_new
        K = torch.cat([k_old, kn.float()[:, None]], 1)
        Vv = torch.cat([v_old, vn.float()[:, None]], 1)
        kv_len = n_old + 1
        chunk = -(-kv_len // ns)
        in_loop = not shadow and mutant != "skip new key"
        after = {"skip new key": 0, "new key twice": 2 if shadow else 1}.get(mutant, 1 if shadow else 0)
        ms, ls, os_ = [], [], []
        for sp in range(ns):
            k_lo = sp * chunk
            k_hi = min(kv_len, k_lo + chunk)
            m = torch.full((H, NKG), -1e30)
            l = torch.zeros(H, NKG)
            acc = torch.zeros(H, NKG, hd)

            def step(idx, valid, m, l, acc):
                s = (K[:, idx] * q[:, None]).sum(-1) * ksc[:, idx] * scale
                mn = torch.where(valid, torch.maximum(m, s), m)
                al = torch.exp(m - mn)
                pw = torch.where(valid, torch.exp(s - mn), torch.zeros_like(s))
                return mn, l * al + pw, acc * al[..., None] + (pw * vsc[:, idx])[..., None] * Vv[:, idx]

            for t0 in range(k_lo, k_hi, NKG):
                idx = t0 + torch.arange(NKG)
                valid = (idx < k_hi) & ((idx != n_old) | in_loop)
                m, l, acc = step(idx.clamp(max=kv_len - 1), valid[None].expand(H, NKG), m, l, acc)
            if k_lo <= n_old < k_hi:
                own = torch.zeros(H, NKG, dtype=torch.bool)
                own[:, (n_old - k_lo) % NKG] = True
                for _ in range(after):
                    m, l, acc = step(torch.full((NKG,), n_old), own, m, l, acc)
            mm = m.amax(-1)
            w = torch.where(l > 0, torch.exp(m - mm[:, None]), torch.zeros_like(l))
            ms.append(mm), ls.append((w * l).sum(-1)), os_.append((w[..., None] * acc).sum(1))
        ms, ls, os_ = torch.stack(ms), torch.stack(ls), torch.stack(os_)        # [ns, H], [ns, H], [ns, H, hd]
        w = torch.where(ls > 0, torch.exp(ms - ms.amax(0)), torch.zeros_like(ls))
        got.out[b] = ((w[..., None] * os_).sum(0) / (w * ls).sum(0)[:, None]).to(dtype).reshape(E)
        got.written[b] = True
    return got


def step_expect(inp, cos, sin):
    return KC.decode_step_expect(inp.qkv, inp.kc, inp.vc, cos, sin, inp.kv_lens, inp.pos, inp.done, inp.dtype, inp.shadow)


STEP_PARAMS = [(hd, dtype, False) for hd in (64, 128) for dtype in ALL] + [(hd, dtype, True) for hd in (64, 128) for dtype in DTYPES16]
step_ids = lambda p: "%s%d-%s" % ("kv8-" if p[2] else "", p[0], KC.NAME[p[1]])


def test_decode_step_cases_cover_what_they_claim():
    cap = KC.DECODE_STEP_CAP
    assert [KC.decode_step_nsplit(nb) for nb in (1, 2, 3, 4, 8)] == [16, 8, 8, 4, 4]
    assert (KC.decode_step_nsplit(1, 4), KC.decode_step_nsplit(1, 32)) == (4, 32)
    seen = {}
    for nb, knob, ns, n_olds, done in KC.DECODE_STEP_CASES:
        assert ns == KC.decode_step_nsplit(nb, knob) and len(n_olds) == len(done) == nb and len(set(n_olds)) == nb
        assert sum(done) == (1 if nb >= 2 else 0) and all(0 <= n <= cap for n in n_olds)
        seen.setdefault((nb, knob), set()).update(n for n, d in zip(n_olds, done) if not d)
    assert set(seen) == {(1, 0), (1, 4), (1, 32), (2, 0), (3, 0), (4, 0), (8, 0)}
    for (nb, knob), vals in seen.items():       # every n_old at one sequence, and on a live sequence of every batch size
        assert vals >= set(KC.decode_step_n_olds(KC.decode_step_nsplit(nb, knob))), (nb, knob)
    # the new key in a later 4-keys-per-thread sub-chunk of its split (ns = 4), for every NKG * 4 the kernels run with
    # (the owner is the last split: offsets 127, 125 and 147 into it; the shadow kernel at hd 64 walks 256 keys per sub-chunk,
    # more than a split holds at this cap)
    offs = [n - 3 * (-(-(n + 1) // 4)) for n in (511, 512, 600)]
    assert min(offs) >= 64 and max(offs) >= 128


@pytest.mark.parametrize("param", STEP_PARAMS, ids=step_ids)
def test_simulated_decode_step_stays_inside_the_bound(param):
    hd, dtype, shadow = param
    cos, sin = KC.rope_tables(hd, KC.DECODE_STEP_CAP + 16, dtype)
    for case in KC.DECODE_STEP_CASES:
        what = "sim decode step hd %d %s nb %d ns %d n_old %s" % (hd, KC.NAME[dtype], case[0], case[2], case[3])
        inp = KC.decode_step_inputs(case, hd, dtype, shadow=shadow)
        fails = KC.decode_step_failures(inp, step_expect(inp, cos, sin), sim_decode_step(inp, cos, sin, case[2]), what)
        assert not fails, "\n".join(m for _, m in fails)


@pytest.mark.parametrize("param", STEP_PARAMS, ids=step_ids)
def test_simulated_decode_step_selector(param):
    hd, dtype, shadow = param
    cos, sin = torch.ones(KC.DECODE_STEP_CAP + 16, hd).to(dtype), torch.zeros(KC.DECODE_STEP_CAP + 16, hd).to(dtype)
    for case in KC.decode_step_selector_cases():
        for second in (False, True):
            if second and min(n for n, d in zip(case[3], case[4]) if not d) < 2:
                continue
            inp, want = KC.decode_step_selector_inputs(case, hd, dtype, second, shadow)
            got = sim_decode_step(inp, cos, sin, case[2])
            live = [b for b in range(case[0]) if not case[4][b]]
            assert torch.equal(KC.bits(got.out[live]), KC.bits(want[live])), (case, second)


def step_mutant_labels(mutant, hd, dtype, shadow):
    """the labels that flag `mutant` over a few cases: one sequence at n_old 0, 1, ns - 1, cap - 1, cap, the first batch of
    every nb > 1, and the selector probes"""
    cos, sin = KC.rope_tables(hd, KC.DECODE_STEP_CAP + 16, dtype)
    picked, seen_nb = [], set()
    for case in KC.DECODE_STEP_CASES:
        nb, knob, ns, n_olds, _ = case
        if (nb == 1 and knob == 0 and n_olds[0] in (0, 1, ns - 1, KC.DECODE_STEP_CAP - 1, KC.DECODE_STEP_CAP)) or (nb > 1 and nb not in seen_nb):
            picked.append(case)
            seen_nb.add(nb)
    labels = set()
    for case in picked:
        inp = KC.decode_step_inputs(case, hd, dtype, shadow=shadow)
        labels |= {l for l, _ in KC.decode_step_failures(inp, step_expect(inp, cos, sin), sim_decode_step(inp, cos, sin, case[2], mutant), "mutant")}
    one, zero = torch.ones(KC.DECODE_STEP_CAP + 16, hd).to(dtype), torch.zeros(KC.DECODE_STEP_CAP + 16, hd).to(dtype)
    for case in KC.decode_step_selector_cases():
        inp, want = KC.decode_step_selector_inputs(case, hd, dtype, False, shadow)
        got = sim_decode_step(inp, one, zero, case[2], mutant)
        live = [b for b in range(case[0]) if not case[4][b]]
        if not torch.equal(KC.bits(got.out[live]), KC.bits(want[live])):
            labels.add("selector")
    return labels


@pytest.mark.parametrize("mutant", sorted(STEP_MUTANTS))
def test_mutants_decode_step(mutant):
    """every mutant is flagged by the assertions STEP_MUTANTS names for it (bf16 and fp32 planes; the shadow in bf16)"""
    worst = dict(KC.WORST)
    try:
        for hd, dtype, shadow in ((64, torch.bfloat16, False), (128, torch.float32, False), (64, torch.bfloat16, True), (128, torch.float16, True)):
            if mutant.startswith("kv8") and not shadow:
                continue
            labels = step_mutant_labels(mutant, hd, dtype, shadow)
            assert labels >= STEP_MUTANTS[mutant], "%s hd %d %s shadow %d: flagged by %s only" % (mutant, hd, KC.NAME[dtype], shadow, sorted(labels))
    finally:
        KC.WORST.clear()
        KC.WORST.update(worst)          # a mutant's ratios are not a kernel's
