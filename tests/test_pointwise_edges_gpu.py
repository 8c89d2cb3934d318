"""Norms, softmax, point-wise kernels, data movers and loss heads: element-wise bounds against an fp64 reference or a bit-exact
fp32 mirror, guarded outputs (tests/kernel_check.py; the contraction kernels are in tests/test_kernel_edges_gpu.py).

The kernels are called through the C ABI with `seedstory.ops`' own `lib()`, `check`, `p`, `dt`, `stream`, because the `ops`
wrappers allocate their outputs: here every output is a `GuardedOut` (in-place kernels run on a payload copied into one; the uint8
image and the GroupNorm workspace are `GuardedBytes`).  Inputs are fresh and seeded per case; references are computed on the CPU,
never by another kernel.  Every family has a case above 1,048,576 work items where its kernel walks a grid-stride loop.

Findings of the first run on an MI355X: one, a gap in the derivation.  euler_cfg_step in fp16 differed from the fp32 mirror on 96
of 1,048,579 elements at sigma 0.0413 -> 0: rnd_T(e dsigma) is compiled to one v_fma_mixlo_f16, which rounds the exact product
once where the mirror rounds twice.  Both roundings are admitted there, element by element (KC.euler_cfg_step_exact); no kernel
changed.  The row "one entry 80 above the rest" is an exact one-hot only in fp16 (see test_softmax_rows_pack_edges).

Worst error / bound per kernel family and dtype, measured on an MI355X (test_zz_worst_ratios prints this table; exact expectations
record 0.000, a ratio above 1 fails the case that produced it; masked_mean takes fp32 values only):

  add_bcast              bf16  worst error / bound = 0.000
  add_bcast              fp16  worst error / bound = 0.000
  add_bcast              fp32  worst error / bound = 0.000
  concat_channels        bf16  worst error / bound = 0.000
  concat_channels        fp16  worst error / bound = 0.000
  concat_channels        fp32  worst error / bound = 0.000
  cosine_rows            bf16  worst error / bound = 0.135
  cosine_rows            fp16  worst error / bound = 0.139
  cosine_rows            fp32  worst error / bound = 0.013
  cross_entropy_rows     bf16  worst error / bound = 0.775
  cross_entropy_rows     fp16  worst error / bound = 0.807
  cross_entropy_rows     fp32  worst error / bound = 0.033
  euler_cfg_step         bf16  worst error / bound = 0.000
  euler_cfg_step         fp16  worst error / bound = 0.000
  euler_cfg_step         fp32  worst error / bound = 0.000
  euler_scale_dup        bf16  worst error / bound = 0.934
  euler_scale_dup        fp16  worst error / bound = 0.974
  euler_scale_dup        fp32  worst error / bound = 0.318
  gather_rows            bf16  worst error / bound = 0.000
  gather_rows            fp16  worst error / bound = 0.000
  gather_rows            fp32  worst error / bound = 0.000
  geglu                  bf16  worst error / bound = 0.329
  geglu                  fp16  worst error / bound = 0.963
  geglu                  fp32  worst error / bound = 0.418
  groupnorm              bf16  worst error / bound = 0.994
  groupnorm              fp16  worst error / bound = 0.992
  groupnorm              fp32  worst error / bound = 0.226
  groupnorm silu         bf16  worst error / bound = 0.790
  groupnorm silu         fp16  worst error / bound = 0.869
  groupnorm silu         fp32  worst error / bound = 0.204
  im2col_patch           bf16  worst error / bound = 0.000
  im2col_patch           fp16  worst error / bound = 0.000
  im2col_patch           fp32  worst error / bound = 0.000
  image_to_u8            bf16  worst error / bound = 0.000
  image_to_u8            fp16  worst error / bound = 0.000
  image_to_u8            fp32  worst error / bound = 0.000
  l2normalize_dim1       bf16  worst error / bound = 0.328
  l2normalize_dim1       fp16  worst error / bound = 0.544
  l2normalize_dim1       fp32  worst error / bound = 0.322
  layernorm block        bf16  worst error / bound = 0.916
  layernorm block        fp16  worst error / bound = 0.695
  layernorm block        fp32  worst error / bound = 0.070
  layernorm wave         bf16  worst error / bound = 0.986
  layernorm wave         fp16  worst error / bound = 0.976
  layernorm wave         fp32  worst error / bound = 0.282
  layernorm wave R=1     bf16  worst error / bound = 0.996
  layernorm wave R=1     fp16  worst error / bound = 0.994
  layernorm wave R=1     fp32  worst error / bound = 0.363
  layernorm wave R=2     bf16  worst error / bound = 0.996
  layernorm wave R=2     fp16  worst error / bound = 0.994
  layernorm wave R=2     fp32  worst error / bound = 0.363
  layernorm wave R=4     bf16  worst error / bound = 0.996
  layernorm wave R=4     fp16  worst error / bound = 0.994
  layernorm wave R=4     fp32  worst error / bound = 0.363
  masked_mean            fp32  worst error / bound = 0.018
  mse                    bf16  worst error / bound = 0.106
  mse                    fp16  worst error / bound = 0.231
  mse                    fp32  worst error / bound = 0.148
  nchw_to_nhwc           bf16  worst error / bound = 0.000
  nchw_to_nhwc           fp16  worst error / bound = 0.000
  nchw_to_nhwc           fp32  worst error / bound = 0.000
  nhwc_to_nchw           bf16  worst error / bound = 0.000
  nhwc_to_nchw           fp16  worst error / bound = 0.000
  nhwc_to_nchw           fp32  worst error / bound = 0.000
  rmsnorm                bf16  worst error / bound = 0.328
  rmsnorm                fp16  worst error / bound = 0.329
  rmsnorm                fp32  worst error / bound = 0.276
  rope k                 bf16  worst error / bound = 0.000
  rope k                 fp16  worst error / bound = 0.000
  rope k                 fp32  worst error / bound = 0.000
  rope q                 bf16  worst error / bound = 0.000
  rope q                 fp16  worst error / bound = 0.000
  rope q                 fp32  worst error / bound = 0.000
  rope v copy            bf16  worst error / bound = 0.000
  rope v copy            fp16  worst error / bound = 0.000
  rope v copy            fp32  worst error / bound = 0.000
  scatter_rows           bf16  worst error / bound = 0.000
  scatter_rows           fp16  worst error / bound = 0.000
  scatter_rows           fp32  worst error / bound = 0.000
  silu_mul               bf16  worst error / bound = 0.329
  silu_mul               fp16  worst error / bound = 0.991
  silu_mul               fp32  worst error / bound = 0.420
  softmax_rows           bf16  worst error / bound = 0.965
  softmax_rows           fp16  worst error / bound = 0.875
  softmax_rows           fp32  worst error / bound = 0.164
  transpose              bf16  worst error / bound = 0.000
  transpose              fp16  worst error / bound = 0.000
  transpose              fp32  worst error / bound = 0.000
  unary gelu             bf16  worst error / bound = 0.975
  unary gelu             fp16  worst error / bound = 0.991
  unary gelu             fp32  worst error / bound = 0.410
  unary silu             bf16  worst error / bound = 0.996
  unary silu             fp16  worst error / bound = 0.986
  unary silu             fp32  worst error / bound = 0.394
"""
import contextlib
import os

import pytest
import torch

import kernel_check as KC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF, FH, F32 = torch.bfloat16, torch.float16, torch.float32
ALL = [BF, FH, F32]
dname = lambda d: KC.NAME[d]
EPS = KC.NORM_EPS
FAMILIES = set()


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


def guarded(rows, width, dtype):
    return KC.GuardedOut(rows, width, dtype, device=DEV)


def bound(y, ref, tol, what, family, dtype):
    FAMILIES.add(family)
    KC.check(y, ref, tol, what, family=family, dtype=dtype)


def exact(y, expected, what, family, dtype, alt=None):
    FAMILIES.add(family)
    KC.check_exact(y, expected, what, family=family, dtype=dtype, alt=alt)


def call(ops, name, *args):
    ops.check(getattr(ops.lib(), name)(*args), name)


# ---- RMSNorm, LayerNorm ---------------------------------------------------------------------------------------------------------
def run_rmsnorm(ops, x, w, dtype):
    g = guarded(x.shape[0], x.shape[1], dtype)
    xd, wd = dev(x), dev(w)
    call(ops, "ss_rmsnorm", ops.p(xd), ops.p(wd), g.data_ptr(), x.shape[0], x.shape[1], EPS, ops.dt(dtype), ops.stream())
    return g


def run_layernorm(ops, x, w, b, dtype):
    g = guarded(x.shape[0], x.shape[1], dtype)
    xd, wd, bd = dev(x), dev(w), dev(b)
    call(ops, "ss_layernorm", ops.p(xd), ops.p(wd), ops.p(bd), g.data_ptr(), x.shape[0], x.shape[1], EPS, ops.dt(dtype), ops.stream())
    return g


@pytest.mark.parametrize("dtype", ALL, ids=dname)
def test_rmsnorm_layernorm_block_pack_edges(ops, dtype):
    """one block per row: 1, 255, 256, 257 and the maximum 2048 packs (the second register pack begins at 257); N(0.3, 2^2) rows,
    an offset row (|mean| / std = 100), a constant row, for RMSNorm an all-zero row"""
    V = KC.vec(dtype)
    for i, (rows, packs) in enumerate((r, p) for r in KC.NORM_BLOCK_ROWS for p in KC.NORM_BLOCK_PACKS):
        what = "%s %d x %d packs" % (dname(dtype), rows, packs)
        x, w, b = KC.norm_inputs(rows, packs * V, dtype, i, zero_row=True)
        y = run_rmsnorm(ops, x, w, dtype).check("rmsnorm " + what)
        bound(y, *KC.rmsnorm_bound(x, w, EPS, dtype), "rmsnorm " + what, "rmsnorm", dtype)
        if rows >= 3:
            assert not y[0].float().abs().sum(), "rmsnorm of an all-zero row must be exactly zero"
        x, w, b = KC.norm_inputs(rows, packs * V, dtype, i)
        y = run_layernorm(ops, x, w, b, dtype).check("layernorm " + what)
        bound(y, *KC.layernorm_bound(x, w, b, EPS, dtype), "layernorm " + what, "layernorm block", dtype)


@pytest.mark.parametrize("dtype", ALL, ids=dname)
def test_layernorm_wave_pack_and_row_edges(ops, dtype):
    """one wave per row (>= 256 rows, <= 256 packs): rows on both sides of a whole block of four waves, 1 .. 4 packs per lane"""
    V = KC.vec(dtype)
    for i, (rows, packs) in enumerate((r, p) for r in KC.LN_WAVE_ROWS for p in KC.LN_WAVE_PACKS):
        what = "layernorm wave %s %d x %d packs" % (dname(dtype), rows, packs)
        x, w, b = KC.norm_inputs(rows, packs * V, dtype, 100 + i)
        y = run_layernorm(ops, x, w, b, dtype).check(what)
        bound(y, *KC.layernorm_bound(x, w, b, EPS, dtype), what, "layernorm wave", dtype)


@pytest.mark.parametrize("dtype", ALL, ids=dname)
@pytest.mark.parametrize("packs", KC.LN_KNOB_PACKS)
def test_layernorm_rows_per_wave_knob(ops, packs, dtype):
    """>= 8192 rows: 1 / 2 / 4 rows per wave (knob layernorm_rows_per_wave), with every ragged last wave (rows % 4 in 0, 1, 3 and
    rows % 8 = 7); the three results bit-equal and each inside the bound"""
    V = KC.vec(dtype)
    for i, rows in enumerate(KC.LN_KNOB_ROWS):
        x, w, b = KC.norm_inputs(rows, packs * V, dtype, 200 + 10 * packs + i)
        ref, tol = KC.layernorm_bound(x, w, b, EPS, dtype)
        ys = []
        for R in KC.LN_KNOBS:
            what = "layernorm wave R=%d %s %d x %d packs" % (R, dname(dtype), rows, packs)
            with knobs(layernorm_rows_per_wave=R):
                y = run_layernorm(ops, x, w, b, dtype).check(what)
            bound(y, ref, tol, what, "layernorm wave R=%d" % R, dtype)
            ys.append(y)
        assert torch.equal(ys[0], ys[1]) and torch.equal(ys[0], ys[2]), "rows per wave changed the result (%d rows)" % rows


# ---- GroupNorm --------------------------------------------------------------------------------------------------------------------
def run_groupnorm(ops, x, gw, gb, G, silu, dtype):
    B, HW, C = x.shape
    g = guarded(B * HW, C, dtype)
    ws = KC.GuardedBytes(int(ops.lib().ss_groupnorm_workspace_bytes(B, HW, C, G, ops.dt(dtype))), device=DEV)
    xd, gwd, gbd = dev(x), dev(gw), dev(gb)
    call(ops, "ss_groupnorm", ops.p(xd), ops.p(gwd), ops.p(gbd), g.data_ptr(), ws.data_ptr(), B, HW, C, G, EPS, int(silu), ops.dt(dtype), ops.stream())
    return g, ws


@pytest.mark.parametrize("dtype", ALL, ids=dname)
@pytest.mark.parametrize("silu", [False, True], ids=["plain", "silu"])
def test_groupnorm_chunk_and_group_edges(ops, silu, dtype):
    """cg < V; group edges inside a pack with idle threads and HW = rows_per_block + 1; HW = 1; cg = 1 with ten block partials (the
    finalize loop twice, ragged); G = 264 > 256 (second sweep of finalize and of the per-group fold); 257 packs (second chunk one
    pack wide, 256 rows in flight); a group mean of 8 spreads; two runs bit-equal; the workspace stays inside its size"""
    for i, (B, HW, C, G) in enumerate(KC.gn_cases(dtype)):
        for offset in ([False, True] if i == 1 else [False]):
            what = "groupnorm %s %s silu %s offset %s" % (dname(dtype), (B, HW, C, G), silu, offset)
            x, gw, gb = KC.gn_inputs(B, HW, C, dtype, i, offset)
            g, ws = run_groupnorm(ops, x, gw, gb, G, silu, dtype)
            y = g.check(what)
            ws.bytes(what + " workspace")
            bound(y.view(B, HW, C), *KC.groupnorm_bound(x, gw, gb, G, EPS, silu, dtype), what, "groupnorm silu" if silu else "groupnorm", dtype)
            g2, ws2 = run_groupnorm(ops, x, gw, gb, G, silu, dtype)
            assert torch.equal(g2.check(what + " (second run)").view(KC._INT[dtype]), y.view(KC._INT[dtype])), what + ": two runs differ"


# ---- softmax_rows -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ALL, ids=dname)
def test_softmax_rows_pack_edges(ops, dtype):
    """in place on a guarded payload; 1 .. 1000 packs per row (the strided loop past 256), both signs of the scale, a row with one
    entry 80 above the rest, a constant row.  At |scale| 0.3 the 80 becomes 24 and exp(-24) = 3.8e-11 is a normal bf16 / fp32 number:
    the row is an exact one-hot in fp16 only (asserted there); a row whose peak stands 400 above the rest (120 after the scale:
    expf underflows to 0) is an exact one-hot in every dtype."""
    V = KC.vec(dtype)
    for i, (rows, packs) in enumerate((r, p) for r in KC.SOFTMAX_ROWS for p in KC.SOFTMAX_PACKS):
        cols = packs * V
        for scale in KC.SOFTMAX_SCALES:
            what = "softmax_rows %s %d x %d packs scale %g" % (dname(dtype), rows, packs, scale)
            x = KC.softmax_inputs(rows, cols, dtype, i)
            peak = None
            if rows >= 3 and cols > 1 and scale > 0:
                peak = int(x[1].float().argmax())
                x[0] = x[0].float().clamp(-9.0, 9.0).to(dtype)
                x[0, 3 % cols] = 400.0
            g = guarded(rows, cols, dtype)
            g.out.copy_(dev(x))
            call(ops, "ss_softmax_rows", g.data_ptr(), rows, cols, scale, ops.dt(dtype), ops.stream())
            y = g.check(what)
            bound(y, *KC.softmax_rows_bound(x, scale, dtype), what, "softmax_rows", dtype)
            if peak is not None:
                onehot = torch.zeros(cols, dtype=dtype)
                onehot[3 % cols] = 1.0
                assert torch.equal(y[0], onehot), what + ": a peak 120 above the rest must give an exact one-hot"
                if dtype == FH:
                    onehot = torch.zeros(cols, dtype=dtype)
                    onehot[peak] = 1.0
                    assert torch.equal(y[1], onehot), what + ": a peak 24 above the rest is an exact one-hot in fp16"


# ---- silu_mul, geglu, unary, add_bcast ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ALL, ids=dname)
def test_silu_mul_geglu(ops, dtype):
    """one pack, a ragged 3 x 33 packs, 1025 x 1025 packs (the grid-stride loop); gates from -20 to 20 (fp16: subnormal outputs)"""
    for i, (rows, inter) in enumerate(KC.gated_shapes(dtype)):
        x = KC.gated_inputs(rows, inter, dtype, i)
        xd = dev(x)
        for name, fam, fn in (("ss_silu_mul", "silu_mul", KC.silu_mul_ew_bound), ("ss_geglu", "geglu", KC.geglu_ew_bound)):
            what = "%s %s %s" % (fam, dname(dtype), (rows, inter))
            g = guarded(rows, inter, dtype)
            call(ops, name, ops.p(xd), g.data_ptr(), rows, inter, ops.dt(dtype), ops.stream())
            y = g.check(what)
            bound(y, *fn(x, dtype), what, fam, dtype)


@pytest.mark.parametrize("dtype", ALL, ids=dname)
def test_add_bcast_exact(ops, dtype):
    for i, (B, R, C) in enumerate(KC.add_bcast_shapes(dtype)):
        what = "add_bcast %s %s" % (dname(dtype), (B, R, C))
        x, pos = KC.randn_t((B, R, C), dtype, 300 + i), KC.randn_t((R, C), dtype, 310 + i, std=0.7)
        xd, pd = dev(x), dev(pos)
        g = guarded(B * R, C, dtype)
        call(ops, "ss_add_bcast", ops.p(xd), ops.p(pd), g.data_ptr(), B, R, C, R * C, ops.dt(dtype), ops.stream())
        exact(g.check(what).view(B, R, C), KC.add_bcast_exact(x, pos), what, "add_bcast", dtype)


@pytest.mark.parametrize("dtype", ALL, ids=dname)
@pytest.mark.parametrize("n", KC.EW_N)
def test_unary_and_euler(ops, n, dtype):
    """unary silu / gelu and euler_scale_dup inside their bounds, euler_cfg_step (in place) bit-exact (fp16: either rounding of
    e dsigma, see KC.euler_cfg_step_exact); sigma pairs from both ends of the 30-step table, guidance 0 / 1 / 7.5"""
    x = KC.gated_inputs(1, n, dtype, 400 + n % 97)[0, :n].contiguous()
    xd = dev(x)
    for op, nm in ((0, "silu"), (1, "gelu")):
        what = "unary %s %s n %d" % (nm, dname(dtype), n)
        g = guarded(1, n, dtype)
        call(ops, "ss_unary", ops.p(xd), g.data_ptr(), n, op, ops.dt(dtype), ops.stream())
        bound(g.check(what)[0], *KC.unary_bound(x, op, dtype), what, "unary " + nm, dtype)
    lat = KC.randn_t((n,), dtype, 410 + n % 97, std=3.0)
    eps = KC.randn_t((2, n), dtype, 420 + n % 97)
    latd, epsd = dev(lat), dev(eps)
    for sg, sg_next in KC.EULER_SIGMAS:
        what = "euler_scale_dup %s n %d sigma %g" % (dname(dtype), n, sg)
        g = guarded(2, n, dtype)
        call(ops, "ss_euler_scale_dup", ops.p(latd), g.data_ptr(), n, sg, ops.dt(dtype), ops.stream())
        bound(g.check(what), *KC.euler_scale_dup_bound(lat, sg, dtype), what, "euler_scale_dup", dtype)
        for guidance in KC.EULER_GUIDANCE:
            what = "euler_cfg_step %s n %d sigma %g -> %g guidance %g" % (dname(dtype), n, sg, sg_next, guidance)
            g = guarded(1, n, dtype)
            g.out.copy_(latd.view(1, n))
            call(ops, "ss_euler_cfg_step", g.data_ptr(), ops.p(epsd), n, guidance, sg, sg_next, ops.dt(dtype), ops.stream())
            alt = KC.euler_cfg_step_exact(lat, eps, guidance, sg, sg_next, fused_f16=True) if dtype == FH else None
            exact(g.check(what)[0], KC.euler_cfg_step_exact(lat, eps, guidance, sg, sg_next), what, "euler_cfg_step", dtype, alt=alt)


@pytest.mark.parametrize("dtype", ALL, ids=dname)
def test_image_to_u8_exact(ops, dtype):
    """every level 2 (k / 255) - 1, the 127.5 tie, +-1, +-1.5 and the neighbours of every other tie: no +-1 level of slack"""
    for i, (pixels, cpad) in enumerate(KC.U8_CASES):
        what = "image_to_u8 %s %d pixels cpad %d" % (dname(dtype), pixels, cpad)
        x = KC.u8_inputs(pixels, cpad, dtype, i)
        xd = dev(x)
        g = KC.GuardedBytes(pixels * 3, device=DEV)
        call(ops, "ss_image_to_u8", ops.p(xd), g.data_ptr(), pixels, cpad, ops.dt(dtype), ops.stream())
        exact(g.bytes(what).view(pixels, 3), KC.image_to_u8_exact(x, pixels), what, "image_to_u8", dtype)


# ---- data movers ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ALL, ids=dname)
def test_gather_scatter_exact(ops, dtype):
    """repeated ids, the first and the last table row; scatter leaves every other row of the (sentinel-filled) target untouched"""
    for i, (n, R, cols) in enumerate(KC.gather_cases(dtype)):
        what = "%s n %d of %d rows x %d" % (dname(dtype), n, R, cols)
        gen = torch.Generator().manual_seed(500 + i)
        table = KC.randn_t((R, cols), dtype, 500 + i)
        ids = torch.randint(0, R, (n,), generator=gen)
        ids[0], ids[-1], ids[n // 2] = R - 1, 0, R - 1
        td, idd = dev(table), dev(ids.to(torch.int32))
        g = guarded(n, cols, dtype)
        call(ops, "ss_gather_rows", ops.p(td), ops.p(idd), g.data_ptr(), n, cols, ops.dt(dtype), ops.stream())
        exact(g.check("gather " + what), table[ids], "gather " + what, "gather_rows", dtype)
        Rd = n + 100
        idx = torch.randperm(Rd, generator=gen)[:n]
        if 0 not in idx:
            idx[0] = 0
        if Rd - 1 not in idx:
            idx[1 % n] = Rd - 1
        if n == 1:
            idx[0] = Rd - 1
        src = KC.randn_t((n, cols), dtype, 520 + i)
        sd, idd = dev(src), dev(idx.to(torch.int32))
        g = guarded(Rd, cols, dtype)
        call(ops, "ss_scatter_rows", ops.p(sd), ops.p(idd), g.data_ptr(), n, cols, ops.dt(dtype), ops.stream())
        pay = g.check("scatter " + what, payload=False)
        exact(pay[idx], src, "scatter " + what, "scatter_rows", dtype)
        rest = torch.ones(Rd, dtype=torch.bool)
        rest[idx] = False
        assert g.untouched(pay)[rest].all(), "scatter %s: a row outside idx was written" % what


@pytest.mark.parametrize("dtype", ALL, ids=dname)
def test_transpose_concat_layout_im2col_exact(ops, dtype):
    dtc = ops.dt(dtype)
    for i, (R, C) in enumerate(KC.TRANSPOSE_SHAPES):
        what = "transpose %s %s" % (dname(dtype), (R, C))
        x = KC.randn_t((R, C), dtype, 600 + i)
        xd = dev(x)
        g = guarded(C, R, dtype)
        call(ops, "ss_transpose", ops.p(xd), g.data_ptr(), R, C, dtc, ops.stream())
        exact(g.check(what), x.t().contiguous(), what, "transpose", dtype)
    for i, (rows, C1, C2) in enumerate(KC.concat_cases(dtype)):
        what = "concat %s %s" % (dname(dtype), (rows, C1, C2))
        a, b = KC.randn_t((rows, C1), dtype, 620 + i), KC.randn_t((rows, C2), dtype, 630 + i)
        ad, bd = dev(a), dev(b)
        g = guarded(rows, C1 + C2, dtype)
        call(ops, "ss_concat_channels", ops.p(ad), ops.p(bd), g.data_ptr(), rows, C1, C2, dtc, ops.stream())
        exact(g.check(what), torch.cat([a, b], 1), what, "concat_channels", dtype)
    for i, (B, C, HW, Cpad) in enumerate(KC.LAYOUT_CASES):
        what = "layout %s %s" % (dname(dtype), (B, C, HW, Cpad))
        x = KC.randn_t((B, C, HW), dtype, 640 + i)
        xd = dev(x)
        g = guarded(B * HW, Cpad, dtype)
        call(ops, "ss_layout_nchw_nhwc", ops.p(xd), g.data_ptr(), B, C, HW, Cpad, 1, dtc, ops.stream())
        want = torch.zeros(B, HW, Cpad, dtype=dtype)                # pad channels: +0 bit for bit
        want[:, :, :C] = x.transpose(1, 2)
        exact(g.check(what + " to NHWC").view(B, HW, Cpad), want, what + " to NHWC", "nchw_to_nhwc", dtype)
        g2 = guarded(B * C, HW, dtype)
        call(ops, "ss_layout_nchw_nhwc", g.data_ptr(), g2.data_ptr(), B, C, HW, Cpad, 0, dtc, ops.stream())
        exact(g2.check(what + " round trip").view(B, C, HW), x, what + " round trip", "nhwc_to_nchw", dtype)
    for i, (B, S, P, kpad) in enumerate(KC.IM2COL_CASES + [KC.IM2COL_LARGE]):
        what = "im2col_patch %s %s" % (dname(dtype), (B, S, P, kpad))
        img = KC.randn_t((B, 3, S, S), dtype, 660 + i)
        imd = dev(img)
        G = S // P
        g = guarded(B * G * G, kpad, dtype)
        call(ops, "ss_im2col_patch", ops.p(imd), g.data_ptr(), B, S, P, kpad, dtc, ops.stream())
        exact(g.check(what), KC.im2col_exact(img, P, kpad), what, "im2col_patch", dtype)


# ---- RoPE + KV append -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ALL, ids=dname)
@pytest.mark.parametrize("hd", KC.ROPE_HD)
def test_rope_kv_append_head_dims(ops, hd, dtype):
    """every head dim the kernel accepts a launch shape for (hd / 2 threads: 1 at hd = 2, a partial wave at 104, two waves at 256);
    positions 0 and the table's last; the last row lands on cap - 1; cache rows outside [kv_start, kv_start + M) keep the sentinel"""
    H, cap = 3, 11
    E = H * hd
    cos, sin = KC.rope_tables(hd, KC.ROPE_MAXPOS, dtype)
    cd, sd = dev(cos), dev(sin)
    for M in KC.ROPE_M:
        what = "rope %s hd %d M %d" % (dname(dtype), hd, M)
        qkv = KC.randn_t((M, 3 * E), dtype, 700 + hd + M)
        pos = torch.tensor([KC.ROPE_MAXPOS - 1, 0, 3, 40, 63, 257][:M] if M > 1 else [KC.ROPE_MAXPOS - 1])
        kv_start = cap - M
        qd, pd = dev(qkv), dev(pos.to(torch.int32))
        gq, gk, gv = guarded(M, E, dtype), guarded(H * cap, hd, dtype), guarded(H * cap, hd, dtype)
        call(ops, "ss_rope_kv_append", ops.p(qd), gq.data_ptr(), gk.data_ptr(), gv.data_ptr(), ops.p(cd), ops.p(sd), ops.p(pd), 0, M, H, hd,
             kv_start, cap, ops.dt(dtype), ops.stream())
        q3, k3, v3 = (qkv[:, j * E:(j + 1) * E].reshape(M, H, hd) for j in range(3))
        exact(gq.check(what + " q"), KC.rope_exact(q3, cos, sin, pos).reshape(M, E), what + " q", "rope q", dtype)
        kp = gk.check(what + " k cache", payload=False).view(H, cap, hd)
        vp = gv.check(what + " v cache", payload=False).view(H, cap, hd)
        exact(kp[:, kv_start:], KC.rope_exact(k3, cos, sin, pos).transpose(0, 1), what + " k", "rope k", dtype)
        exact(vp[:, kv_start:], v3.transpose(0, 1), what + " v", "rope v copy", dtype)
        assert gk.untouched(kp)[:, :kv_start].all() and gv.untouched(vp)[:, :kv_start].all(), what + ": a cache row before kv_start was written"
        if M > 1:           # the contiguous-positions path (pos_start), landing on position table's last row
            gq2, gk2, gv2 = guarded(M, E, dtype), guarded(H * cap, hd, dtype), guarded(H * cap, hd, dtype)
            p0 = KC.ROPE_MAXPOS - M
            call(ops, "ss_rope_kv_append", ops.p(qd), gq2.data_ptr(), gk2.data_ptr(), gv2.data_ptr(), ops.p(cd), ops.p(sd), None, p0, M, H, hd,
                 0, cap, ops.dt(dtype), ops.stream())
            exact(gq2.check(what + " q pos_start"), KC.rope_exact(q3, cos, sin, torch.arange(p0, p0 + M)).reshape(M, E), what + " q pos_start", "rope q", dtype)
            kp = gk2.check(what + " k cache pos_start", payload=False).view(H, cap, hd)
            assert gk2.untouched(kp)[:, M:].all() and not gk2.untouched(kp)[:, :M].any()


# ---- l2normalize, loss heads -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ALL, ids=dname)
def test_l2normalize_dim1(ops, dtype):
    for i, (B, L, C) in enumerate(KC.L2_CASES):
        what = "l2normalize_dim1 %s %s" % (dname(dtype), (B, L, C))
        x = KC.randn_t((B, L, C), dtype, 800 + i)
        if C > 1:
            x[:, :, 1] = 0
        xd = dev(x)
        g = guarded(B * L, C, dtype)
        call(ops, "ss_l2normalize_dim1", ops.p(xd), g.data_ptr(), B, L, C, ops.dt(dtype), ops.stream())
        y = g.check(what).view(B, L, C)
        bound(y, *KC.l2normalize_bound(x, dtype), what, "l2normalize_dim1", dtype)
        if C > 1:
            assert not y[:, :, 1].float().abs().sum(), what + ": an all-zero column must stay exactly zero"


@pytest.mark.parametrize("dtype", ALL, ids=dname)
@pytest.mark.parametrize("vocab", KC.CE_VOCABS)
def test_cross_entropy_rows_ld_pad(ops, vocab, dtype):
    """ld = vocab + 24 with NaN / Inf in the pad; labels 0, vocab - 1, ignored, an inner one and the row's own maximum; the per-row
    loss inside its bound, the valid flags exact"""
    rows, ld = 5, vocab + KC.CE_PAD
    what = "cross_entropy_rows %s vocab %d" % (dname(dtype), vocab)
    x = KC.randn_t((rows, ld), dtype, 900 + vocab % 89, std=3.0)
    KC.poison_(x[:, vocab:])
    labels = torch.tensor([0, vocab - 1, -100, (vocab * 3) // 7, int(x[4, :vocab].float().argmax())])
    xd, ld_ = dev(x), dev(labels)
    gl, gv = guarded(1, rows, F32), guarded(1, rows, F32)
    call(ops, "ss_cross_entropy_rows", ops.p(xd), ld, ops.p(ld_), rows, vocab, -100, gl.data_ptr(), gv.data_ptr(), ops.dt(dtype), ops.stream())
    ref, tol, valid = KC.cross_entropy_rows_bound(x[:, :vocab], labels, dtype)
    bound(gl.check(what + " loss")[0], ref, tol, what, "cross_entropy_rows", dtype)
    assert torch.equal(gv.check(what + " valid")[0].double(), valid), what + ": valid flags"


@pytest.mark.parametrize("dtype", ALL, ids=dname)
def test_cosine_rows(ops, dtype):
    for i, (dim, rows) in enumerate((d, n) for d in KC.COSINE_DIMS for n in KC.COSINE_ROWS):
        what = "cosine_rows %s %d x %d" % (dname(dtype), rows, dim)
        a, b = KC.randn_t((rows, dim), dtype, 1000 + i), KC.randn_t((rows, dim), dtype, 1030 + i)
        ad, bd = dev(a), dev(b)
        g = guarded(1, rows, F32)
        call(ops, "ss_cosine_rows", ops.p(ad), ops.p(bd), rows, dim, g.data_ptr(), ops.dt(dtype), ops.stream())
        bound(g.check(what)[0], *KC.cosine_rows_bound(a, b, dtype), what, "cosine_rows", dtype)


@pytest.mark.parametrize("dtype", ALL, ids=dname)
def test_mse_and_masked_mean(ops, dtype):
    """n on both sides of one 65536-element block and a ragged last block of four; masks None, 0 / 1 and all zero (mean 0, count 0).
    masked_mean takes fp32 row values whatever the model dtype: it is run (and recorded) once, under fp32"""
    for i, n in enumerate(KC.MEAN_N):
        a, b = KC.randn_t((n,), dtype, 1100 + i), KC.randn_t((n,), dtype, 1110 + i)
        ad, bd = dev(a), dev(b)
        ws = torch.empty(max(int(ops.lib().ss_loss_workspace_bytes(n)) // 8, 1), dtype=torch.float64, device=DEV)
        g = guarded(1, 2, F32)
        call(ops, "ss_mse", ops.p(ad), ops.p(bd), n, ops.p(ws), g.data_ptr(), ops.dt(dtype), ops.stream())
        out = g.check("mse n %d" % n)[0]
        ref, tol = KC.mse_bound(a, b)
        bound(out[:1], ref.reshape(1), tol.reshape(1), "mse %s n %d" % (dname(dtype), n), "mse", dtype)
        assert float(out[1]) == n
        if dtype != F32:
            continue
        for mask in (None, (torch.arange(n) % 3 != 0).float(), torch.zeros(n)):
            md = None if mask is None else dev(mask)
            g = guarded(1, 2, F32)
            call(ops, "ss_masked_mean", ops.p(ad), ops.p(md), n, ops.p(ws), g.data_ptr(), ops.stream())
            out = g.check("masked_mean n %d" % n)[0]
            ref, tol, cnt = KC.masked_mean_bound(a, mask)
            bound(out[:1], ref.reshape(1), tol.reshape(1), "masked_mean n %d" % n, "masked_mean", dtype)
            assert float(out[1]) == cnt


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ALL, ids=dname)
def test_unsupported_widths_are_refused_untouched(ops, dtype):
    """cols % V != 0, more than 2048 packs, C % G != 0, odd or too large a head dim, KV overflow: SSError, and not one element of
    the guarded output written"""
    from seedstory import _lib
    V, dtc, st = KC.vec(dtype), ops.dt(dtype), ops.stream()
    big = dev(torch.zeros(4, 2049 * V + 8, dtype=dtype))
    ids = dev(torch.zeros(4, dtype=torch.int32))

    def refused(g, name, *args):
        with pytest.raises(_lib.SSError):
            call(ops, name, *args)
        pay = g.check(name + " refused", payload=False)
        assert g.untouched(pay).all(), name + ": a refused call wrote to its output"
    for cols in (V + 1, 2 * V - 1, 2049 * V):
        g = guarded(2, cols, dtype)
        refused(g, "ss_rmsnorm", ops.p(big), ops.p(big), g.data_ptr(), 2, cols, EPS, dtc, st)
        refused(g, "ss_layernorm", ops.p(big), ops.p(big), ops.p(big), g.data_ptr(), 2, cols, EPS, dtc, st)
    cols = V + 1
    g = guarded(2, cols, dtype)
    refused(g, "ss_softmax_rows", g.data_ptr(), 2, cols, 0.3, dtc, st)
    refused(g, "ss_silu_mul", ops.p(big), g.data_ptr(), 2, cols, dtc, st)
    refused(g, "ss_geglu", ops.p(big), g.data_ptr(), 2, cols, dtc, st)
    refused(g, "ss_add_bcast", ops.p(big), ops.p(big), g.data_ptr(), 1, 2, cols, 2 * cols, dtc, st)
    refused(g, "ss_gather_rows", ops.p(big), ops.p(ids), g.data_ptr(), 2, cols, dtc, st)
    refused(g, "ss_scatter_rows", ops.p(big), ops.p(ids), g.data_ptr(), 2, cols, dtc, st)
    g = guarded(2, 2 * V + 1, dtype)
    refused(g, "ss_concat_channels", ops.p(big), ops.p(big), g.data_ptr(), 2, V, V + 1, dtc, st)
    ws = KC.GuardedBytes(4096, device=DEV)
    g = guarded(4, 8 * V, dtype)
    refused(g, "ss_groupnorm", ops.p(big), ops.p(big), ops.p(big), g.data_ptr(), ws.data_ptr(), 1, 4, 8 * V, 3, EPS, 0, dtc, st)     # C % G != 0
    g = guarded(4, V + 2, dtype)
    refused(g, "ss_groupnorm", ops.p(big), ops.p(big), ops.p(big), g.data_ptr(), ws.data_ptr(), 1, 4, V + 2, 1, EPS, 0, dtc, st)     # C % V != 0
    assert ws.untouched(ws.check("groupnorm refused workspace", payload=False)).all()
    for hd, M, kv_start, cap in ((7, 2, 0, 8), (258, 2, 0, 8), (64, 3, 6, 8)):          # odd, > 256, 6 + 3 > 8
        gq, gk, gv = guarded(M, 2 * hd, dtype), guarded(2 * cap, hd, dtype), guarded(2 * cap, hd, dtype)
        with pytest.raises(_lib.SSError):
            call(ops, "ss_rope_kv_append", ops.p(big), gq.data_ptr(), gk.data_ptr(), gv.data_ptr(), ops.p(big), ops.p(big), None, 0, M, 2, hd,
                 kv_start, cap, dtc, st)
        for g in (gq, gk, gv):
            assert g.untouched(g.check("rope refused", payload=False)).all(), "rope hd %d: a refused call wrote to its output" % hd


def test_zz_worst_ratios():
    """prints the worst error / bound per kernel family and dtype seen by this file's checks (the record kept in the module
    docstring; exact expectations record 0); SS_KERNEL_RATIO_FILE=<path> also writes it"""
    table = KC.worst_table(FAMILIES)
    print("\nworst error / bound per family and dtype:\n" + table)
    path = os.environ.get("SS_KERNEL_RATIO_FILE")
    if path:
        with open(path, "w") as f:
            f.write(table + "\n")
    assert all(r <= 1.0 for (f, _), r in KC.WORST.items() if f in FAMILIES)
