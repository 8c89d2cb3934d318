"""The checker (tests/kernel_check.py) is tested before it judges a kernel: a correct kernel SIMULATED on the CPU (fp32 math,
chunked and reversed summation, the kernels' rounding points; attention: a tile-64 online softmax with P rounded to T) must
produce zero violations on every case tests/test_kernel_edges_gpu.py runs, and every seeded mutant must be flagged."""
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
