"""GEMM variants with extra epilogue arithmetic, element-wise: ss_gemm_fp8, ss_gemm_lnfold / ss_gemm_lnfold_part, the statistics
producers (ss_gemm_rowstat / ss_gemm_rowpart / the fallback pass, ss_rowstat_finalize, ss_rowstats), ss_gemm_splitk and the
LN-fused fp8 quantiser.  The companion of tests/test_kernel_edges_gpu.py: a-priori bounds against an fp64 reference
(tests/kernel_check.py derives them), every launch into a `GuardedOut` / `GuardedBytes`, inputs fresh per case and seeded by
the tile id, exact probes where the arithmetic allows them.  References are fp64 evaluations of the kernel's own formula on the
kernel's own inputs (e4m3 bytes and fp32 scales; the fp32 statistics vectors; the STORED output for the producers' sums) — never
another kernel.  tests/test_kernel_check_cpu.py runs a simulated kernel over every case here and flags the seeded mutants.

Out of scope: the experimental fp8 tiles 95 / 96, and the 4-wave folded tiles behind `lnfold_w4` (their known defect stays
behind the dispatcher's reroute and is not exercised).

ss_gemm_lnfold_part forms its statistics in the LDS-staged epilogue only (the direct epilogue reads the rstd / shift vectors,
which this form does not have), so every wave must take it: gemm_lnfold_launch moves a shape whose tile width does not divide N
to the 160- / 128-wide 8-wave tile and refuses what is left (N no multiple of 160 or 128; C or the bias pointer off 16 bytes;
ldc % 8 != 0) with SS_EINVAL.  test_lnfold_part_refuses_what_the_staged_epilogue_cannot_take and the N = 208 cases of
test_lnfold_part_gemm_bound_every_tile pin that.

Worst error / bound per family and dtype, measured on an MI355X against the fp64 reference (test_zz_worst_ratios_variants
prints this table; a ratio above 1 fails the case that produced it):

  fp8 gemm               bf16  worst error / bound = 0.992
  fp8 gemm strided       bf16  worst error / bound = 0.983
  fp8 ln quantiser       bf16  worst error / bound = 0.931
  fp8 ln quantiser       fp16  worst error / bound = 0.937
  lnfold gemm            bf16  worst error / bound = 0.991
  lnfold gemm            fp16  worst error / bound = 0.956
  lnfold_part gemm       bf16  worst error / bound = 0.992
  lnfold_part gemm       fp16  worst error / bound = 0.966
  producer gemm          bf16  worst error / bound = 0.995
  producer gemm          fp16  worst error / bound = 0.988
  producer sums          bf16  worst error / bound = 0.012
  producer sums          fp16  worst error / bound = 0.045
  producer sums fallback bf16  worst error / bound = 0.013
  producer sums fallback fp16  worst error / bound = 0.029
  rowstat finalize       bf16  worst error / bound = 0.984
  rowstat finalize       fp16  worst error / bound = 0.989
  rowstats               bf16  worst error / bound = 0.216
  rowstats               fp16  worst error / bound = 0.216
  splitk gemm            bf16  worst error / bound = 0.819
  splitk gemm            fp16  worst error / bound = 0.469
"""
import contextlib

import pytest
import torch

import kernel_check as KC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF, FH, F32 = torch.bfloat16, torch.float16, torch.float32
D16 = [BF, FH]
dname = lambda d: KC.NAME[d]
EPS = KC.LN_EPS
FAMILIES = ["fp8 gemm", "fp8 gemm strided", "fp8 ln quantiser", "lnfold gemm", "lnfold_part gemm", "rowstats", "rowstat finalize",
            "producer gemm", "producer sums", "producer sums fallback", "splitk gemm"]


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
    return None if t is None else t.to(DEV).contiguous()


def guarded(rows, width, dtype, **kw):
    return KC.GuardedOut(rows, width, dtype, device=DEV, **kw)


def stream():
    return torch.cuda.current_stream().cuda_stream


def refused(rc, what, *bufs):
    """a non-zero return is a clean SSError and nothing was written"""
    from seedstory import _lib
    assert rc != 0, what + ": accepted"
    with pytest.raises(_lib.SSError):
        _lib.check(rc, what)
    torch.cuda.synchronize()
    for g in bufs:
        assert bool((g.flat == KC.SENTINEL[g.dtype]).all()), what + ": refused, yet something was written"


# ---- fp8 ------------------------------------------------------------------------------------------------------------------------
def fp8_launch(ops, q, kw, out):
    a8, sa, w8, sw = q
    return ops.gemm_fp8(dev(a8), dev(sa), dev(w8), dev(sw), bias=dev(kw.get("bias")), residual=dev(kw.get("residual")),
                        gelu=bool(kw.get("gelu_")), geglu=bool(kw.get("geglu")), out=out)


@pytest.mark.parametrize("cfg", KC.FP8_TILES)
def test_fp8_gemm_bound_every_tile(ops, cfg):
    """every shipped fp8 tile (0: the closed-form rule) x epilogue on M on both sides of each BM, N whole / a multiple of 16 / ragged
    (direct epilogue and scalar tails on whichever tile is forced), 1 .. 5 K tiles of the two-slot pipeline"""
    with knobs(gemm_fp8_cfg=cfg):
        for i, (M, N, K) in enumerate(KC.FP8_SHAPES):
            q = KC.fp8_inputs(M, N, K, KC.fp8_seeds(cfg, i, 0)[0])
            for j, epi in enumerate(KC.FP8_EPILOGUES):
                kw = KC.epilogue_inputs(epi, M, N, BF, KC.fp8_seeds(cfg, i, j)[1])
                what = "gemm_fp8 cfg %d %s %s" % (cfg, (M, N, K), epi)
                g = guarded(M, N // 2 if epi == "geglu" else N, BF)
                fp8_launch(ops, q, kw, g.out)
                y = g.check(what)
                ref, tol = KC.gemm_fp8_bound(*q, **kw)
                KC.check(y, ref, tol, what, family="fp8 gemm", dtype=BF)


@pytest.mark.parametrize("cfg", KC.FP8_TILES)
def test_fp8_gemm_strides_and_alignment(ops, cfg):
    """ss_gemm_fp8 through ctypes: `out` at ld > width (gaps guarded; ld % 8 == 0 keeps the staged epilogue, ld % 4 the 8-byte
    stores, ld + 1 the scalar ones) and the bias 8 bytes off its 16-byte alignment (no staged epilogue, vector loads stay)"""
    from seedstory import _lib
    lib = _lib.lib()
    M, N, K = KC.FP8_STRIDE_SHAPE
    with knobs(gemm_fp8_cfg=cfg):
        for c, (dld, ob, geglu) in enumerate(KC.FP8_STRIDE_CASES):
            q = KC.fp8_inputs(M, N, K, KC.fp8_stride_seed(cfg, c))
            kw = KC.epilogue_inputs("geglu" if geglu else "bias+residual", M, N, BF, KC.fp8_stride_seed(cfg, c))
            a8, sa, w8, sw = (dev(t) for t in q)
            No = N // 2 if geglu else N
            biasbuf = torch.zeros(N + 8, dtype=BF, device=DEV)
            bias = biasbuf[ob:ob + N]
            bias.copy_(kw["bias"])
            assert bias.data_ptr() % 16 == 2 * ob
            res = dev(kw.get("residual"))
            g = guarded(M, No, BF, ld=No + dld)
            epi = (_lib.EPI_BIAS | _lib.EPI_GEGLU_PAIR) if geglu else (_lib.EPI_BIAS | _lib.EPI_RESIDUAL)
            what = "ss_gemm_fp8 cfg %d %s ldc N%+d bias%+d %s" % (cfg, (M, N, K), dld, ob, "geglu" if geglu else "bias+residual")
            _lib.check(lib.ss_gemm_fp8(a8.data_ptr(), sa.data_ptr(), w8.data_ptr(), sw.data_ptr(), g.data_ptr(), M, N, K, No + dld,
                                       bias.data_ptr(), None if geglu else res.data_ptr(), 0 if geglu else N, epi, stream()), what)
            y = g.check(what)
            ref, tol = KC.gemm_fp8_bound(*q, **kw)
            KC.check(y, ref, tol, what, family="fp8 gemm strided", dtype=BF)


@pytest.mark.parametrize("cfg", KC.FP8_TILES)
def test_fp8_gemm_exact_probes_every_tile(ops, cfg):
    """operands that quantise exactly (one-hot / all-ones rows: code 448, scale fl(1 / 448); integer rows with one +-7: codes 64 w,
    scale 2^-6): selector, its mirror and the counter, the two de-quantisation products mirrored in fp32 — no tolerance"""
    with knobs(gemm_fp8_cfg=cfg):
        for (M, N, K) in KC.FP8_PROBE_SHAPES:
            for kind in ("selector", "selector_w", "counter"):
                a8, sa, w8, sw, exp = KC.fp8_probe(kind, M, N, K, seed=cfg)
                g = guarded(M, N, BF)
                fp8_launch(ops, (a8, sa, w8, sw), {}, g.out)
                what = "fp8 %s cfg %d %s" % (kind, cfg, (M, N, K))
                KC.check_exact(g.check(what), exp, what)


@pytest.mark.parametrize("dtype", D16, ids=dname)
def test_fp8_ln_quantiser_bound(ops, dtype):
    """quantize_rows_fp8(x, ln=): q * s within the LayerNorm bound plus the e4m3 rounding of the fp64 LayerNorm, the scale within
    the propagated tolerance of amax / 448 (next to test_fp8_gpu's comparison with the unfused pair, which stays)"""
    from seedstory import _lib
    lib = _lib.lib()
    for i, (M, K) in enumerate(KC.QUANT_LN_SHAPES):
        x, gm, bt = KC.norm_inputs(M, K, dtype, 70 + i)
        gq, gs = KC.GuardedBytes(M * K, device=DEV), guarded(1, M, F32)
        xd, gd, bd = dev(x), dev(gm), dev(bt)
        what = "quantize_rows_fp8 ln %s %s" % (dname(dtype), (M, K))
        _lib.check(lib.ss_quantize_rows_fp8(xd.data_ptr(), K, M, K, gq.data_ptr(), gs.data_ptr(), gd.data_ptr(), bd.data_ptr(), EPS,
                                            ops.dt(dtype), stream()), what)
        q, s = gq.bytes(what).view(M, K), gs.check(what)[0]
        assert not bool(((q & 0x7F) == 0x7F).any()), what + ": NaN codes"
        (v, tq), (sv, ts) = KC.quantize_ln_bound(x, gm, bt, EPS, dtype)
        KC.check(s, sv, ts, what + " scale", family="fp8 ln quantiser", dtype=dtype)
        KC.check(KC.f8_values(q) * s.double()[:, None], v, tq, what + " q * s", family="fp8 ln quantiser", dtype=dtype)


# ---- folded LayerNorm ---------------------------------------------------------------------------------------------------------------
def rowstats_guarded(ops, xd, M, K, dtype, what):
    """ss_rowstats into a guarded [2, M] fp32 buffer -> (rstd, shift) on the CPU"""
    from seedstory import _lib
    g = guarded(2, M, F32)
    _lib.check(_lib.lib().ss_rowstats(xd.data_ptr(), K, M, K, EPS, g.out[0].data_ptr(), g.out[1].data_ptr(), ops.dt(dtype), stream()), what)
    st = g.check(what)
    return st[0].clone(), st[1].clone()


@pytest.mark.parametrize("dtype", D16, ids=dname)
def test_rowstats_bound(ops, dtype):
    """ss_rowstats per row: K = 8 .. 2048 (1 .. 4 packs per lane, partly filled waves), rows with |mean| ~ 9 std, a constant row"""
    for i, (M, K) in enumerate(KC.ROWSTATS_SHAPES):
        x = KC.lnfold_inputs(M, 16, K, dtype, 50 + i)[0]
        what = "rowstats %s %s" % (dname(dtype), (M, K))
        rstd, shift = rowstats_guarded(ops, dev(x), M, K, dtype, what)
        (rv, rt), (sv, st) = KC.rowstats_bound(x, EPS, dtype)
        KC.check(rstd, rv, rt, what + " rstd", family="rowstats", dtype=dtype)
        KC.check(shift, sv, st, what + " shift", family="rowstats", dtype=dtype)


def lnfold_kw(epi, bias_d):
    return dict(bias_d=None if epi == "plain" else bias_d, gelu_=epi == "gelu", geglu=epi == "geglu")


@pytest.mark.parametrize("dtype", D16, ids=dname)
@pytest.mark.parametrize("cfg", KC.LNFOLD_TILES)
def test_lnfold_gemm_bound_every_tile(ops, cfg, dtype):
    """ss_gemm_lnfold on the library's own choice (0) and on every forced staged tile id.  What this does and does not show: the
    library does not report which tile ran, so nothing here asserts it.  ss_gemm_lnfold has no unfolded fall-back (a missing
    folded instantiation is an SSError), so every returned result comes from SOME folded tile; which one follows from
    gemm_lnfold_launch: the 8-wave ids 60 / 62 / 63 / 64 / 66 / 69 / 71 / 72 run as forced; 68 is a 4-wave tile and takes the
    dispatcher's reroute to 62 (N % 160 == 0) or 66, so it repeats those cases on other inputs; and 0, with tuning off and these
    shapes absent from the tile table, is the closed-form rule (67 / 70, rerouted to 62 / 66 as well), not a table entry.
    The statistics are ss_rowstats' output, handed to the reference as the fp32 vectors the kernel was given."""
    with knobs(gemm_cfg=cfg, gemm_autotune=0):
        for i, (M, N, K) in enumerate(KC.LNFOLD_SHAPES):
            x, wg, colsum, bias_d = KC.lnfold_inputs(M, N, K, dtype, KC.lnfold_seed(cfg, i))
            xd, wd, cd, bd = dev(x), dev(wg), dev(colsum), dev(bias_d)
            rstd, shift = rowstats_guarded(ops, xd, M, K, dtype, "rowstats")
            rd, sd = dev(rstd), dev(shift)
            for epi in KC.LNFOLD_EPILOGUES:
                kw = lnfold_kw(epi, bias_d)
                what = "gemm_lnfold cfg %d %s %s %s" % (cfg, dname(dtype), (M, N, K), epi)
                g = guarded(M, N // 2 if epi == "geglu" else N, dtype)
                ops.gemm_lnfold(xd, wd, rd, sd, cd, bias_d=None if epi == "plain" else bd, gelu=kw["gelu_"], geglu=kw["geglu"], out=g.out)
                y = g.check(what)
                ref, tol = KC.gemm_lnfold_bound(x, wg, rstd, shift, colsum, dtype, **kw)
                KC.check(y, ref, tol, what, family="lnfold gemm", dtype=dtype)


@pytest.mark.parametrize("dtype", D16, ids=dname)
@pytest.mark.parametrize("cfg", KC.LNFOLD_TILES)
def test_lnfold_part_gemm_bound_every_tile(ops, cfg, dtype):
    """ss_gemm_lnfold_part: (rstd, shift) formed in the consumer's epilogue from per-strip partials, known to the reference only to
    the tolerance of lnfold_part_stats_bound.  Launched: (129, 160, 64) with 2 strips, (257, 640, 192) with 6 and (520, 320, 640)
    with 20 (the loop takes 16 at a time: a second batch with a masked tail; three 256-row / five 128-row tiles).  (520, 208, 640):
    N = 208 is no multiple of 160 or 128 and is refused with nothing written (see the module docstring).  The tile ids are forced
    as in test_lnfold_gemm_bound_every_tile; a forced tile whose width does not divide N (any but the 160-wide at N = 160, say)
    gives way to 62."""
    from seedstory import _lib
    with knobs(gemm_cfg=cfg, gemm_autotune=0):
        for i, (M, N, K) in enumerate(KC.LNFOLD_PART_SHAPES):
            x, wg, colsum, bias_d = KC.lnfold_inputs(M, N, K, dtype, KC.lnfold_seed(cfg, i, part=True))
            part = KC.lnfold_parts(x)
            xd, wd, cd, bd, pd = dev(x), dev(wg), dev(colsum), dev(bias_d), dev(part)
            (rv, rt), (sv, st) = KC.lnfold_part_stats_bound(part, K, EPS)
            for epi in KC.LNFOLD_EPILOGUES:
                kw = lnfold_kw(epi, bias_d)
                what = "gemm_lnfold_part cfg %d %s %s %s" % (cfg, dname(dtype), (M, N, K), epi)
                g = guarded(M, N // 2 if epi == "geglu" else N, dtype)
                if N % 160 and N % 128:
                    with pytest.raises(_lib.SSError):
                        ops.gemm_lnfold_part(xd, wd, pd, K, EPS, cd, bias_d=None if epi == "plain" else bd, gelu=kw["gelu_"], geglu=kw["geglu"], out=g.out)
                    torch.cuda.synchronize()
                    assert bool((g.flat == KC.SENTINEL[dtype]).all()), what + ": refused, yet something was written"
                    continue
                ops.gemm_lnfold_part(xd, wd, pd, K, EPS, cd, bias_d=None if epi == "plain" else bd, gelu=kw["gelu_"], geglu=kw["geglu"], out=g.out)
                y = g.check(what)
                ref, tol = KC.gemm_lnfold_bound(x, wg, rv, sv, colsum, dtype, t_rstd=rt, t_shift=st, **kw)
                KC.check(y, ref, tol, what, family="lnfold_part gemm", dtype=dtype)


@pytest.mark.parametrize("dtype", D16, ids=dname)
def test_lnfold_part_refuses_what_the_staged_epilogue_cannot_take(ops, dtype):
    """ss_gemm_lnfold_part through ctypes with ldc % 8 != 0, C 8 bytes off, the bias 8 bytes off: each sends waves to the direct
    epilogue, which has no statistics in this form — a clean SSError, nothing written; the aligned launch at ld > width runs"""
    from seedstory import _lib
    lib = _lib.lib()
    M, N, K, seed = KC.LNFOLD_REFUSAL_CASE
    x, wg, colsum, bias_d = KC.lnfold_inputs(M, N, K, dtype, seed)
    part = KC.lnfold_parts(x)
    xd, wd, cd, pd = dev(x), dev(wg), dev(colsum), dev(part)
    biasbuf = torch.zeros(N + 8, dtype=dtype, device=DEV)
    with knobs(gemm_autotune=0):
        for (dld, oc, ob) in [(8, 0, 0), (4, 0, 0), (0, 4, 0), (0, 0, 4)]:
            bias = biasbuf[ob:ob + N]
            bias.copy_(bias_d)
            g = guarded(M, N, dtype, ld=N + dld, offset=oc)
            what = "ss_gemm_lnfold_part %s ldc N%+d C%+d bias%+d" % (dname(dtype), dld, oc, ob)
            rc = lib.ss_gemm_lnfold_part(xd.data_ptr(), wd.data_ptr(), g.data_ptr(), M, N, K, N + dld, pd.data_ptr(), part.shape[1], K, EPS,
                                         cd.data_ptr(), bias.data_ptr(), _lib.EPI_BIAS, ops.dt(dtype), stream())
            if (dld, oc, ob) != (8, 0, 0):
                refused(rc, what, g)
                continue
            _lib.check(rc, what)
            y = g.check(what)
            (rv, rt), (sv, st) = KC.lnfold_part_stats_bound(part, K, EPS)
            ref, tol = KC.gemm_lnfold_bound(x, wg, rv, sv, colsum, dtype, bias_d=bias_d, t_rstd=rt, t_shift=st)
            KC.check(y, ref, tol, what, family="lnfold_part gemm", dtype=dtype)


# ---- statistics producers -----------------------------------------------------------------------------------------------------------
def accumulator(M):
    """a zeroed fp64 [M, 2] accumulator carved from guarded bytes -> (the guarded buffer, the accumulator view)"""
    g = KC.GuardedBytes(M * 16, device=DEV)
    g.out.zero_()
    return g, g.out.view(torch.float64).view(M, 2)


def check_sums(got1, got2, y, tn, what, family, dtype):
    (s1, t1), (s2, t2) = KC.rowsum_bound(y, tn)
    KC.check(got1, s1, t1, what + " sums", family=family, dtype=dtype)
    KC.check(got2, s2, t2, what + " sums of squares", family=family, dtype=dtype)


@pytest.mark.parametrize("dtype", D16, ids=dname)
@pytest.mark.parametrize("fallback", [0, 1], ids=["epilogue", "fallback"])
def test_producer_statistics(ops, fallback, dtype):
    """gemm(rowstat=) / gemm(rowpart=) and the fallback pass: the stored output against gemm_bound, the sums per row / per strip
    against rowsum_bound of that stored output; N = 200: staged and direct waves mix in the accumulator form.  The accumulator
    is exactly 0 after rowstat_finalize and its second use gives the same bits; the partials start as NaN sentinels."""
    fam = "producer sums fallback" if fallback else "producer sums"
    with knobs(gemm_autotune=0, gemm_rowstat_fallback=fallback):
        for i, (M, N, K) in enumerate(KC.PRODUCER_SHAPES):
            a, w, bias, res = KC.producer_inputs(M, N, K, dtype, KC.producer_seed(fallback, i))
            ad, wd, bd = dev(a), dev(w), dev(bias)
            for residual in (None, res):
                rd = dev(residual)
                ref, tol = KC.gemm_bound(a, w, dtype, bias=bias, residual=residual)
                what = "gemm rowstat %s %s %s%s" % ("fallback" if fallback else "", dname(dtype), (M, N, K), " +residual" if residual is not None else "")
                ga, acc = accumulator(M)
                g = guarded(M, N, dtype)
                ops.gemm(ad, wd, bias=bd, residual=rd, out=g.out, rowstat=acc)
                y = g.check(what)
                KC.check(y, ref, tol, what, family="producer gemm", dtype=dtype)
                st = ga.bytes(what).view(torch.float64).view(M, 2)
                check_sums(st[:, 0], st[:, 1], y, None, what, fam, dtype)
                gs = guarded(2, M, F32)
                ops.rowstat_finalize(acc, N, EPS, out=gs.out)
                fin = gs.check(what + " finalize")
                (rv, rt), (sv, sts) = KC.rowstat_finalize_bound(st, N, EPS)
                KC.check(fin[0], rv, rt, what + " finalize rstd", family="rowstat finalize", dtype=dtype)
                KC.check(fin[1], sv, sts, what + " finalize shift", family="rowstat finalize", dtype=dtype)
                zero = ga.bytes(what + " after finalize")
                assert not bool(zero.any()), what + ": accumulator not exactly 0 after finalize"
                g2 = guarded(M, N, dtype)
                ops.gemm(ad, wd, bias=bd, residual=rd, out=g2.out, rowstat=acc)
                KC.check_exact(g2.check(what + " second use"), y, what + " second use")
                st2 = ga.bytes(what).view(torch.float64).view(M, 2)
                check_sums(st2[:, 0], st2[:, 1], y, None, what + " second use", fam, dtype)
                # per-strip partials
                strips = ops.rowpart_strips(M, N, K, dtype)
                if N == 200:
                    assert strips == 0          # ragged last tile: no strip form
                    continue
                assert strips > 0 and N % strips == 0, (strips, N)
                what = what.replace("rowstat", "rowpart")
                gp = guarded(M, strips * 2, F32)
                g3 = guarded(M, N, dtype)
                ops.gemm(ad, wd, bias=bd, residual=rd, out=g3.out, rowpart=gp.view(M, strips, 2))
                y3 = g3.check(what)
                KC.check(y3, ref, tol, what, family="producer gemm", dtype=dtype)
                part = gp.check(what + " partials").view(M, strips, 2)
                check_sums(part[:, :, 0], part[:, :, 1], y3, N // strips, what, fam, dtype)


@pytest.mark.parametrize("dtype", D16, ids=dname)
def test_producer_partials_into_folded_consumer(ops, dtype):
    """the chain the UNet runs: gemm(rowpart=) -> gemm_lnfold_part on the stored output, judged against the fp64 formula on the
    producer's own partials"""
    with knobs(gemm_autotune=0):
        for (M, N, K, seed) in KC.PRODUCER_CHAIN_CASES:
            a, w, bias, res = KC.producer_inputs(M, N, K, dtype, seed)
            strips = ops.rowpart_strips(M, N, K, dtype)
            gp, gy = guarded(M, strips * 2, F32), guarded(M, N, dtype)
            ops.gemm(dev(a), dev(w), bias=dev(bias), residual=dev(res), out=gy.out, rowpart=gp.view(M, strips, 2))
            y, part = gy.check("producer"), gp.check("partials").view(M, strips, 2)
            _, wg, colsum, bias_d = KC.lnfold_inputs(8, 160, N, dtype, seed)
            g = guarded(M, 160, dtype)
            ops.gemm_lnfold_part(gy.out, dev(wg), gp.view(M, strips, 2), N, EPS, dev(colsum), bias_d=dev(bias_d), out=g.out)
            what = "producer -> gemm_lnfold_part %s %s" % (dname(dtype), (M, N, K))
            z = g.check(what)
            (rv, rt), (sv, st) = KC.lnfold_part_stats_bound(part, N, EPS)
            ref, tol = KC.gemm_lnfold_bound(y, wg, rv, sv, colsum, dtype, bias_d=bias_d, t_rstd=rt, t_shift=st)
            KC.check(z, ref, tol, what, family="lnfold_part gemm", dtype=dtype)


# ---- split-K ------------------------------------------------------------------------------------------------------------------------
def splitk_launch(ops, a, w, bias, res, out, ws, dtype, M, N, K, what):
    from seedstory import _lib
    _lib.check(_lib.lib().ss_gemm_splitk(a.data_ptr(), w.data_ptr(), out.data_ptr(), M, N, K, None if bias is None else bias.data_ptr(),
                                         None if res is None else res.data_ptr(), ws.data_ptr(), ws.nbytes, ops.dt(dtype), stream()), what)


@pytest.mark.parametrize("dtype", D16, ids=dname)
@pytest.mark.parametrize("S", KC.SPLITK_S)
def test_splitk_gemm_bound(ops, S, dtype):
    """ss_gemm_splitk with the planned (0) and every forced split count: uneven ranges (16 K tiles at S = 3, 5), empty last ranges
    (17 K tiles at S = 8, 16 at S = 5: exact zeros), a NaN-filled guarded workspace of which exactly the first S slices are
    written, and the counter probe across every K range"""
    from seedstory import _lib
    sent = KC.SENTINEL[F32]
    with knobs(gemm_splitk_s=S, gemm_autotune=0):
        for i, (M, N, K) in enumerate(KC.SPLITK_SHAPES):
            planned = KC.splitk_planned(M, N, K)
            assert _lib.lib().ss_gemm_splitk_workspace_bytes(M, N, K) == planned * M * N * 4, "not eligible / another plan"
            Su = S or planned
            a, w = KC.gemm_inputs(M, N, K, dtype, KC.splitk_seed(i, S))
            ad, wd = dev(a), dev(w)
            for epi in KC.SPLITK_EPILOGUES:
                kw = KC.epilogue_inputs(epi, M, N, dtype, KC.splitk_seed(i, S))
                what = "gemm_splitk S %d (%d) %s %s %s" % (S, Su, dname(dtype), (M, N, K), epi)
                ws, g = KC.GuardedBytes(8 * M * N * 4, device=DEV), guarded(M, N, dtype)
                splitk_launch(ops, ad, wd, dev(kw.get("bias")), dev(kw.get("residual")), g, ws, dtype, M, N, K, what)
                y = g.check(what)
                ref, tol = KC.gemm_splitk_bound(a, w, dtype, Su, **kw)
                KC.check(y, ref, tol, what, family="splitk gemm", dtype=dtype)
                slices = ws.bytes(what).view(torch.int32).view(8, M * N)
                assert not bool((slices[:Su] == sent).any()) and bool((slices[Su:] == sent).all()), what + ": not exactly %d slices written" % Su
                for s, (k0, k1) in enumerate(KC.splitk_ranges(K, Su)):
                    if k1 == k0:
                        assert not bool(slices[s].any()), what + ": empty K range %d is not exact zeros" % s
            ca, cw, exp = KC.counter_probe(M, N, K, dtype, seed=S)
            ws, g = KC.GuardedBytes(8 * M * N * 4, device=DEV), guarded(M, N, dtype)
            what = "splitk counter probe S %d %s %s" % (S, dname(dtype), (M, N, K))
            splitk_launch(ops, dev(ca), dev(cw), None, None, g, ws, dtype, M, N, K, what)
            KC.check_exact(g.check(what), exp, what)


@pytest.mark.parametrize("dtype", D16, ids=dname)
def test_splitk_ineligible_shape_equals_gemm(ops, dtype):
    """M = 128 is below the split-K range: ss_gemm_splitk must run ss_gemm, bit for bit, and leave the workspace alone"""
    from seedstory import _lib
    M, N, K = 128, 64, 1024
    assert _lib.lib().ss_gemm_splitk_workspace_bytes(M, N, K) == 0
    a, w = KC.gemm_inputs(M, N, K, dtype, 390)
    kw = KC.epilogue_inputs("bias+residual", M, N, dtype, 390)
    ad, wd, bd, rd = dev(a), dev(w), dev(kw["bias"]), dev(kw["residual"])
    with knobs(gemm_autotune=0):
        ws, g, g0 = KC.GuardedBytes(8 * M * N * 4, device=DEV), guarded(M, N, dtype), guarded(M, N, dtype)
        splitk_launch(ops, ad, wd, bd, rd, g, ws, dtype, M, N, K, "splitk M = 128")
        ops.gemm(ad, wd, bias=bd, residual=rd, out=g0.out)
        KC.check_exact(g.check("splitk M = 128"), g0.check("gemm"), "splitk M = 128 vs gemm")
        assert bool((ws.bytes("workspace").view(torch.int32) == KC.SENTINEL[F32]).all())


def test_zz_worst_ratios_variants():
    """runs last in this file: the table of the module docstring"""
    print("\nworst error / bound per family and dtype (fp64 reference):\n" + KC.worst_table(FAMILIES))
    assert all(r <= 1.0 for (f, _), r in KC.WORST.items() if f in FAMILIES)
