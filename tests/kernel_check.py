"""Element-wise checker for the kernel tests: a-priori error bounds against an fp64 reference, guarded output buffers and
exact probes.  Plain torch on the CPU; imports nothing from seed-story_amd/ (test infrastructure, like truth_cache.py).

Why element-wise: a relative Frobenius norm over a [1024, 640] bf16 product is 1.7e-3 from rounding alone, and eight zeroed
outputs, sixteen 4-ulp offsets or a K tail dropped in one 16x16 fragment all stay under the 4e-3 the sweeps assert.  Every bound
here is PER ELEMENT and derived from the number formats, never from what a kernel returned.

Notation.  u_T = unit roundoff of the stored type (2^-8 bf16, 2^-11 fp16, 2^-24 fp32); u32 = 2^-24.  Every helper carries a
pair (v, t): v the fp64 reference value with the kernel's own intermediate roundings mirrored, t a tolerance such that a correct
kernel's value x satisfies |x - v| <= t.  The steps (each a function below):

  accumulate   v = sum_k a_k w_k exactly (fp64), S = sum_k |a_k| |w_k|.  fp32 accumulation of Kacc terms in ANY order obeys
               |x - v| <= gamma_Kacc S with gamma_n = n u32 / (1 - n u32) ~ n u32 (Higham, Accuracy and Stability, 3.1).
               t = 2 Kacc u32 S.  The factor 2 is the only slack in this file: MFMA's internal summation tree is not specified to
               round after every term.  (products of two 16-bit values are exact in fp32: 8 + 8 or 11 + 11 significand bits.)
  fp32 op      x' = fl(x + b): |x' - (v + b)| <= t + u32 |x'| <= t + u32 (|v + b| + t).
  mid round    both sides round to T: |rnd(x) - rnd(v)| <= u_T |x| + |x - v| + u_T |v| <= 2 u_T |v| + (1 + u_T) t.  (the kernel's
               value may land on the other side of a rounding boundary than the reference's: two half-ulps, not one.)
  final round  only the kernel rounds; the reference stays unrounded: |rnd(x) - v| <= u_T |x| + t <= u_T |v| + (1 + u_T) t.
               For a plain product this is the bound  |y - ref| <= u_T |ref| + (1 + u_T) e_acc.  A truncating store errs by
               up to 2 u_T |v| and fails it.
  subnormals   u_T |v| is the half-ulp of a NORMAL v; below the smallest normal (fp16: 6.1e-5, reached by GELU / SiLU of a negative
               gate) the spacing stops shrinking, so every rounding also carries eta_T = half the subnormal spacing (fp16 2^-25,
               bf16 2^-134, fp32 2^-150): 3e-8 at most, invisible next to any other term unless the value itself is that small.
  f(x)         |f(x) - f(v)| <= L t with L = max |f'| over [v - t, v + t].  L is taken as min(Lmax, max(|f'(v - t)|, |f'(v)|,
               |f'(v + t)|) + M2 t): every point of the interval is within t of a sample and |f''| <= M2.  erf-GELU: Lmax = 1.13
               (f' peaks at 1.129, x = 1.41), M2 = 0.8 (f'' = phi(x) (2 - x^2) <= 2 phi(0) = 0.798).  SiLU: Lmax = 1.1, M2 = 0.5.
               The kernel's own evaluation (16-bit GELU: Abramowitz-Stegun 7.1.26, |erf error| < 1.5e-7, on hardware rcp / exp2;
               SiLU: expf and one division) adds at most 2^-21 max(|v|, |f(v)|): 0.5 |v| 1.5e-7 = |v| 2^-23.7 plus four fp32 ops.
               fp32 kernels call libm's erff / expf (<= 2 ulp) and do three more fp32 operations: 2^-22 max(|v|, |f(v)|).
               This term is not in the first-order recipe; without it the bound would charge the kernel's approximation of f to
               its accumulation.  It is 1 / 8192 of a bf16 half-ulp.
  a * g        |x_a x_g - a g| <= |a| t_g + |g| t_a + t_a t_g, then one fp32 op.

Epilogues mirror the rounding points of the kernels (ss_gemm_common.h gemm_epilogue): bias is added in fp32 and the sum rounded;
GELU is applied to the rounded value and rounded; a row vector (conv) and the residual are each added to the rounded value and
rounded again; GEGLU multiplies the rounded value by the rounded GELU of the rounded gate.

Attention (per query row; P = fp64 softmax of the fp64 scores, masked keys have P = 0):
  score error   delta_s(j) = 2 hd u32 scale (|q| . |k_j|): the accumulate step above with Kacc = hd (the scale is one more fp32
                op, inside the factor 2).
  softmax       with scores off by d_j, P'_j = P_j e^{d_j} / sum_i P_i e^{d_i}; to first order |P'_j - P_j| <= P_j (|d_j| +
                sum_i P_i |d_i|) <= 2 P_j max_j delta_s, so the output moves by at most 2 max_j delta_s (P @ |V|).
  P rounded     the kernels round exp(s - m) to T before the P V product (MFMA operands) and sum the row normaliser from the same
                values or from the unrounded ones: numerator and denominator each move by a relative u_T at most:
                2 u_T (P @ |V|).  (fp32 kernels do not round P; u_T = u32 then and the term is noise.)
  output        one final round: u_T |ref|.
  bound         |out - ref| <= u_T |ref| + (2 u_T + 2 max_j delta_s) (P @ |V|).
The fp32 accumulation of P V (kv_len terms of one sign pattern, rescaled per tile) is not budgeted on its own; it rides in the
factor 2 of delta_s.  The constants are derived, not tuned: the GPU file records the worst error / bound ratio per family.

Norms, softmax, point-wise kernels and loss heads (tests/test_pointwise_edges_gpu.py).  Two more steps:

  sum32        an fp32 sum of n terms in ANY order (thread chains, shuffle trees, LDS folds): |x - v| <= gamma_n sum |term|,
               gamma_n = n u32 / (1 - n u32).  Additions of an exact 0 (idle lanes, a chain's first term) round nothing, so a tree
               over n terms has at most n - 1 rounding additions whatever its shape.  No factor 2: no MFMA is involved.
  sqrt, 1 / x  |sqrt(x) - sqrt(v)| = |x - v| / (sqrt(x) + sqrt(v)) <= t / (sqrt(max(v - t, 0)) + sqrt(v));
               |1 / x - 1 / v| <= t / (v (v - t));  each followed by its own fp32 rounding (an fp32 op).

  RMSNorm      ss = sum x^2 (sum32 over cols; the fma rounds once per term); ss / cols, + eps, sqrt, 1 / : four fp32 ops -> rstd.
               h = rnd_T(x rstd): one fp32 op, mid round.  y = rnd_T(w h): w h is exact in fp32 for 16-bit T (for fp32 the
               product's own rounding IS the final round): final round.  An all-zero row gives h = 0 exactly, bound eta_T.
  LayerNorm    two-pass, block and wave kernels alike.  mean: sum32 over cols, one division: t_mean = gamma_cols mean|x| +
               u32 |mean|.  d = x - mean is one fp32 op on an operand known to t_mean; d^2 moves by 2 |d| t_d + t_d^2 and the
               squares are summed by sum32; / cols, + eps, sqrt, 1 / -> rstd.  y = rnd_T(((x - mean) rstd) w + b): the
               subtraction, two products, one addition (four fp32 ops), final round.  A constant row has variance 0 in the
               reference and rstd = 1 / sqrt(eps); the kernel's mean may be off by t_mean, which the bound carries through d
               (it is loose there, gamma_cols |c| / sqrt(eps), and valid).  |mean| >> std costs gamma_cols mean|x| in every
               d: the price of an fp32 mean, charged as such.
  GroupNorm    per (image, group), n = HW cg elements.  Pass 1 sums x and x^2 per channel and block in fp32: a thread chain
               over the block's rows followed by one fold over the row lanes, together an any-order sum of at most
               rows_per_block terms: sum32 with k = min(HW, max(16, 128 KiB / row bytes)), the largest rows_per_block the launch
               rule can return (GN_ROWS_MAX_BYTES below: a hand copy).  Everything after that is fp64 (channels of a group,
               blocks, E[x^2] - mean^2) except 1 / n, which the kernel forms in fp32 (two roundings) before widening it:
               t_S1 = (gamma_k + 2 u32) sum|x|, t_S2 = (gamma_k + 2 u32) sum x^2, t_mean = t_S1 / n, and var = E[x^2] - mean^2
               carries t_S2 / n + 2 |mean| t_mean + t_mean^2: the error of the fp32 chains scaled by E[x^2], NOT by the
               variance; a group with mean 8 and spread 1 pays 65 gamma_k, the design's price.  mean and var are narrowed
               to fp32 (one rounding each); + eps, sqrt, 1 / ; sc = rstd gamma, sh = beta - mean sc (two fp32 ops);
               out = fma(x, sc, sh): one rounding.  Since x sc + (beta - mean sc) = (x - mean) sc + beta, the error of sc
               multiplies x - mean, not x: t = |x - mean| t_sc + |sc| t_mean + u32 (|mean sc| + |sh| + |out|).  Then the final round.  With SiLU: mid round, the fast SiLU on hardware rcp /
               exp2 (evaluation term 2^-21 max(|v|, |f(v)|) in every dtype, as for the 16-bit GELU), final round.
  softmax_rows s = x scale: one fp32 op.  The kernel's own maximum m' enters every term of the row alike and cancels in e / sum
               e, so m' is a parameter, not an error: d = s - m is one more fp32 op, |d' - d| <= u32 (|s| + |s - m|).
               e = expf(d): e (exp(t_d) - 1) + 4 u32 e (libm: 2 ulp).  sum: the terms' errors plus sum32 over cols of positive
               terms; 1 / ; e inv: product; final round.
  silu_mul     rnd_T(rnd_T(silu(g)) u): silu of an exact gate (evaluation term only), mid round, product with the exact u,
               final round.  geglu: rnd_T(a rnd_T(gelu(g))) the same way.  unary: f(x), final round.
  l2normalize  s = sum of L squares (sum32), sqrt (fp32 op), mid round of the norm, clamp at 1e-12, x / norm (1 / x step times
               |x|, one fp32 op), final round.  An all-zero column divides 0 by the clamp: exactly 0.
  cross-entropy row  m is the exact maximum of exact inputs.  d = x - m: one fp32 op; e = expf(d) as above; s: sum32 over vocab
               of positive terms (s >= 1: the maximum contributes e^0); logf(s): t_s / (s - t_s) + 4 u32 |log s|;
               (x_lab - m) - logf(s): two fp32 ops; rnd_T: final round.  The loss is stored in fp32 without another rounding.
  cosine row   na = rnd_T(sqrt(sum32 a^2)), nb alike: mid rounds.  rnd_T(a / na), rnd_T(b / nb): 1 / x step, fp32 op, mid round.
               p = rnd_T(product): mid round.  s = rnd_T(sum32 over dim of p): the terms' errors add up (each mid round may flip:
               2 u_T |p| per term; this dominates and grows with sum |p| <= 1), mid round.  1 - s: fp32 op, final round.
  mse          d = fl(a - b), fl(d d): relative 3 u32 per term (+ eta32); the terms are summed in fp64 (n 2^-53, below), divided
               and narrowed once: (4 u32 + n 2^-52) sum|term| / n.  masked_mean: fl(val mask), fp64 sums, one narrowing:
               (2 u32 + n 2^-52) sum|term| / count; the count is an exact integer; an all-zero mask gives (0, 0) exactly.
  euler_scale_dup  inv = 1 / sqrtf(sigma^2 + 1) formed on the host in fp32: four fp32 ops.  x inv: one fp32 op, final round.

GEMM variants with extra epilogue arithmetic (tests/test_gemm_variants_edges_gpu.py).  The rounding points are read from
gemm_epilogue / gemm_epilogue_staged (ss_gemm_common.h, `EM`) and splitk_reduce_kernel (ss_gemm.hip); every variant ends in the
epilogue() above.

  fp8          the operands are the kernel's own inputs: e4m3 code values (exact in fp64) and fp32 scales, so the quantisation
               error is not part of the bound.  A product of two e4m3 values has 4 + 4 significand bits and is exact in fp32:
               `accumulate` on the code values, Kacc = K.  Its factor 2 IS taken over for v_mfma_scale_f32_16x16x128_f8f6f4: the
               instruction sums 128 products per lane group in a tree whose internal roundings are not specified, exactly the
               reason the factor exists (with unit block scales the scaling itself is exact).  Then t = acc * (sa * sw): s =
               fl(sa sw) is mirrored in fp32 (one operation on two known numbers, no error against the mirror), fl(acc s) is one
               fp32 op; then epilogue() with T = bf16.
  LN-fold      the reference is the kernel's own formula on the fp32 vectors it was handed: fma(acc, rstd, fl(shift colsum))
               (+ bias_d).  p = acc rstd is exact inside the fma and carries t_acc |rstd|; c = shift colsum is one fp32 op:
               u32 |c|; the fma rounds once: u32 |p + c| <= u32 (|p| + |c|).  On a row with |mean| >> std p and c cancel, so the
               bound carries u32 (|p| + |c|) + u32 |c| and NOT u32 |result|: that is the price of the folded form.  Statistics
               known only to (t_rstd, t_shift) (the producer-partial form) add (|acc| + t_acc) t_rstd + |colsum| t_shift:
               charged independently, although the two errors are correlated (loose by |p| / |result| on offset rows, valid).
  part stats   (rstd, shift) formed by the consumer from fp32 (sum, sum of squares) partials: the partials are summed in fp64
               (n 2^-53, charged as e64 = 2^-48), mean = a iw, var = max(b iw - mean^2, 0), rstd = (float)(1 / sqrt(var + eps)),
               shift = -(float)mean * rstd, where iw is the FP32 1.0f / width widened: off from 1 / width by up to u32 relative.
               It scales a and b alike: t_mean = (u32 + e64) |mean|, t_var = (u32 + e64) E[x^2] + 2 |mean| t_mean + t_mean^2
               ~ u32 (E[x^2] + 2 mean^2), NOT u32 var: a row with mean 9 and spread 1 pays 240 u32 on a variance of 1.
               |d r| <= t_var / 2 (var + eps - t_var)^-3/2; one narrowing for rstd (u32 |r|), two for shift (the narrowed mean,
               the fp32 product).  ss_rowstat_finalize is the same formula with an fp64 1 / width: u_inv = 2^-53 instead of u32.
  rowstats     ss_rowstats is the first half of the two-pass LayerNorm (mean: sum32 and a division; squared deviations: fma,
               sum32; / cols, + eps, sqrt, 1 / ) and one fp32 product -mean rstd: shared code with layernorm_bound.
  row sums     the producers' statistics are sums over the STORED output y of the launch under test (exact inputs), per strip
               (ss_gemm_rowpart, the fallback kernel) or per row (the fp64 accumulator): |S1 - sum y| <= gamma_n sum |y| and
               |S2 - sum y^2| <= gamma_(n+1) sum y^2 (an fma per term; the + 1 covers a kernel that rounds the square first),
               n = the fp32 terms of one strip, or of the whole row for the accumulator, whose fp32 pieces (16 or TN columns)
               are added in fp64 by atomics in any order: + e64 sum |.|.
  split-K      every slice's fp32 accumulator is stored exactly, splitk_reduce_kernel adds the S slices in fp32 (S - 1 ops):
               `accumulate` with Kacc = K + S, then epilogue(bias, residual).  An empty K range stores exact zeros.
  LN quantiser quantize_rows_fp8(x, ln=...): o = rnd_T(LayerNorm) as layernorm_bound (the squares are rounded before they are
               added: gamma_(cols + 1); rsqrtf is within 1 ulp = the two roundings of sqrt and 1 / ), amax' = max |o| moves by
               at most max_row t_ln, s = fl(amax' / 448): t_s = max t_ln / 448 + u32 s.  q = RNE_e4m3(fl(o fl(448 / amax'))):
               relative 2^-4 (3 mantissa bits) plus 2^-10 in code units (half the subnormal spacing 2^-9) plus 3 u32; times s:
               |q s - ln| <= t_ln + (2^-4 + 4 u32)(|ln| + t_ln) + 2^-10 (s + t_s).

Exact expectations (no bound; mirrored in fp32 on the CPU with the kernel's rnd points, so double rounding cannot differ): every
data mover; add_bcast (one correctly rounded fp32 add, stored); RoPE q / k (rnd(rnd(a c) + rnd(-b s)) in T); euler_cfg_step
(rnd(eu + rnd(g rnd(ec - eu))), x + rnd(e dsigma), stored); image_to_u8 (rnd_T(0.5 x + 0.5), clamp, rintf(255 v): 255 v is exact
in fp32 for a 16-bit v, one fp32 rounding otherwise; ties to even).  The library is built with -ffp-contract=off, so the fp32
mirrors see the same operations."""
import numpy as np
import torch

U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -24}
U32 = 2.0 ** -24
ETA = {torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25, torch.float32: 2.0 ** -150}   # half the subnormal spacing
NAME = {torch.bfloat16: "bf16", torch.float16: "fp16", torch.float32: "fp32"}

# ---- tile ids: the one list (tests/test_kernels_gpu.py, tests/test_sdxl_gpu.py and tests/test_kernel_edges_gpu.py import these) ----
GEMM_REG_TILES = [1, 2, 3]                                      # register-staged
GEMM_DMA_TILES = [8, 10, 15, 20, 21, 22, 23, 24, 26, 28, 29, 30, 31, 32, 33, 34, 35, 36, 37, 38, 39, 40, 41, 42, 43, 44, 45, 46, 54, 55, 56,
                  57, 58, 60, 61, 62, 63, 64, 65, 66, 67, 68, 69, 70, 71, 72]
GEMM_PP_TILES = [54, 55, 56, 57, 58]                            # ping-pong
GEMM_RING_TILES = [30, 31, 32, 33, 35, 36, 38, 39, 40, 41, 42, 43, 60, 61, 62, 64]
GEMM_PERSISTENT_TILES = [33, 35, 36, 38, 39, 40, 43, 54, 55, 56, 57, 58, 60, 64, 72]
GEMM_TILES = GEMM_REG_TILES + GEMM_DMA_TILES                    # every shipped GEMM tile id
CONV_PP_TILES = [54, 55, 56, 57]
CONV_DMA_TILES = [8, 15, 20, 21, 22, 23, 24, 26, 28, 29, 30, 33, 34, 36, 37, 38, 39, 40, 41, 42, 43, 44, 45, 46, 54, 56, 60, 61, 62, 63, 64, 65,
                  66, 67, 68, 69, 70, 71, 72]
CONV_PERSISTENT_TILES = [33, 36, 38, 39, 40, 43, 60, 64, 72]
CONV_TILES = sorted(set(CONV_DMA_TILES + CONV_PP_TILES))        # every shipped conv tile id


def rnd(x, dtype):
    """fp64 -> T -> fp64 (round to nearest even)."""
    return x.to(dtype).double()


# ---- (v, t) propagation ------------------------------------------------------------------------------------------------------
def accumulate(a, w, kacc=None):
    """a [M, K], w [N, K] (any float dtype, exact in fp64) -> (a @ w^T, 2 Kacc u32 |a| @ |w|^T)."""
    a, w = a.double(), w.double()
    k = a.shape[1] if kacc is None else kacc
    return a @ w.t(), 2.0 * k * U32 * (a.abs() @ w.abs().t())


def op32(v, t):
    """one fp32 operation whose exact result is v, on an operand known to t."""
    return v, t + U32 * (v.abs() + t)


def mid_round(v, t, dtype):
    u = U[dtype]
    return rnd(v, dtype), 2.0 * (u * v.abs() + ETA[dtype]) + (1.0 + u) * t


def final_round(v, t, dtype):
    u = U[dtype]
    return v, u * v.abs() + ETA[dtype] + (1.0 + u) * t


def _gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x * 0.7071067811865476))


def _gelu_d(x):
    return 0.5 * (1.0 + torch.erf(x * 0.7071067811865476)) + x * torch.exp(-0.5 * x * x) * 0.3989422804014327


def _silu(x):
    return x * torch.sigmoid(x)


def _silu_d(x):
    s = torch.sigmoid(x)
    return s * (1.0 + x * (1.0 - s))


def _apply(f, fd, lmax, m2, v, t, feval):
    L = torch.maximum(torch.maximum(fd(v - t).abs(), fd(v).abs()), fd(v + t).abs()) + m2 * t
    L = torch.clamp(L, max=lmax)
    fv = f(v)
    return fv, L * t + feval * torch.maximum(v.abs(), fv.abs())


FEVAL = {torch.bfloat16: 2.0 ** -21, torch.float16: 2.0 ** -21, torch.float32: 2.0 ** -22}


def gelu(v, t, dtype):
    return _apply(_gelu, _gelu_d, 1.13, 0.8, v, t, FEVAL[dtype])


def silu(v, t, dtype):
    return _apply(_silu, _silu_d, 1.1, 0.5, v, t, FEVAL[dtype])


def product(va, ta, vg, tg):
    return op32(va * vg, va.abs() * tg + vg.abs() * ta + ta * tg)


def epilogue(v, t, dtype, bias=None, gelu_=False, rowvec=None, residual=None, geglu=False):
    """The rounding points of gemm_epilogue on an accumulator (v, t) -> (reference, bound) of the stored value.
    bias [N] / rowvec [M, N] (already broadcast) / residual [M, N]: tensors of the model dtype (exact in fp64)."""
    if bias is not None:
        v, t = op32(v + bias.double(), t)
    if geglu:
        v, t = mid_round(v, t, dtype)
        gv, gt = gelu(v[:, 1::2], t[:, 1::2], dtype)
        gv, gt = mid_round(gv, gt, dtype)
        v, t = product(v[:, 0::2], t[:, 0::2], gv, gt)
        return final_round(v, t, dtype)
    if gelu_:
        v, t = mid_round(v, t, dtype)
        v, t = gelu(v, t, dtype)
    for extra in (rowvec, residual):
        if extra is not None:
            v, t = mid_round(v, t, dtype)
            v, t = op32(v + extra.double(), t)
    return final_round(v, t, dtype)


def gemm_bound(a, w, dtype, bias=None, residual=None, gelu_=False, geglu=False):
    """(reference, bound) [M, N] (N / 2 for GEGLU) of ss_gemm on a [M, K], w [N, K]."""
    v, t = accumulate(a, w)
    return epilogue(v, t, dtype, bias=bias, gelu_=gelu_, residual=residual, geglu=geglu)


def silu_mul_bound(w, x, dtype):
    """ss_gemv / ss_gemv_batched with the SiLU pair: w [2I, K], x [nb, K] -> y [nb, I] = round(round(silu(round(g))) * round(u))."""
    v, t = accumulate(x, w)
    v, t = mid_round(v, t, dtype)
    I = w.shape[0] // 2
    sv, st = silu(v[:, :I], t[:, :I], dtype)
    sv, st = mid_round(sv, st, dtype)
    v, t = product(v[:, I:], t[:, I:], sv, st)
    return final_round(v, t, dtype)


def conv_bound(x, w, dtype, stride=1, upsample=False, bias=None, rowvec=None, residual=None):
    """x [B, Ci, H, W], w [Co, Ci, 3, 3], bias [Co], rowvec [B, Co], residual [B, Co, Ho, Wo] -> (reference, bound) NCHW of
    ss_conv3x3 (padding 1; Kacc = 9 Cin, padding taps included: they add exact zeros)."""
    F = torch.nn.functional
    xd, wd = x.double(), w.double()
    if upsample:
        xd = F.interpolate(xd, scale_factor=2.0, mode="nearest")
    v = F.conv2d(xd, wd, None, stride=stride, padding=1)
    t = 2.0 * 9 * x.shape[1] * U32 * F.conv2d(xd.abs(), wd.abs(), None, stride=stride, padding=1)
    return epilogue(v, t, dtype, bias=None if bias is None else bias.double()[None, :, None, None],
                    rowvec=None if rowvec is None else rowvec.double()[:, :, None, None], residual=residual)


def attention_bound(q, k, v, scale, allow, dtype):
    """q [..., Lq, hd], k / v [..., Lk, hd] (per head), allow [Lq, Lk] bool or None -> (reference, bound) [..., Lq, hd]."""
    qd, kd, vd = q.double(), k.double(), v.double()
    hd = q.shape[-1]
    s = qd @ kd.transpose(-1, -2) * scale
    ds = 2.0 * hd * U32 * abs(scale) * (qd.abs() @ kd.abs().transpose(-1, -2))
    if allow is not None:
        s = s.masked_fill(~allow, float("-inf"))
        ds = ds.masked_fill(~allow, 0.0)
    P = torch.softmax(s, -1)
    ref = P @ vd
    u = U[dtype]
    return ref, u * ref.abs() + (2.0 * u + 2.0 * ds.amax(-1, keepdim=True)) * (P @ vd.abs())


def causal_allow(Lq, Lk):
    """bottom-right aligned causal mask: query i sees keys j <= i + Lk - Lq."""
    return torch.ones(Lq, Lk, dtype=torch.bool).tril(diagonal=Lk - Lq)


# ---- the check ----------------------------------------------------------------------------------------------------------------
WORST = {}   # (family, dtype name) -> worst error / bound seen by check(); the GPU file prints it


def violations(y, ref, tol):
    """-> (count, worst ratio, [(index tuple, ratio), ...] of the worst few).  Non-finite outputs always violate."""
    yd = y.double().to(ref.device).reshape(ref.shape)
    err = (yd - ref).abs()
    err = torch.where(torch.isfinite(yd), err, torch.full_like(err, float("inf")))
    ratio = torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    bad = ratio > 1.0
    n = int(bad.sum())
    worst = float(ratio.max()) if ratio.numel() else 0.0
    coords = []
    if n:
        flat = ratio.flatten()
        for i in torch.topk(flat, min(6, n)).indices.tolist():
            coords.append((tuple(int(c) for c in np.unravel_index(i, tuple(ratio.shape))), float(flat[i])))
    return n, worst, coords


def report(y, ref, tol, what=""):
    n, worst, coords = violations(y, ref, tol)
    if not n:
        return worst, ""
    lines = ["%s: %d of %d elements outside the bound, worst error / bound = %.3g" % (what, n, ref.numel(), worst)]
    for idx, r in coords:
        rc = idx[-2:] if len(idx) >= 2 else (0,) + idx
        lines.append("  at %s ratio %.3g   (row, col) mod 16 = (%d, %d)  mod 64 = (%d, %d)  mod 256 = (%d, %d)"
                     % (idx, r, rc[0] % 16, rc[1] % 16, rc[0] % 64, rc[1] % 64, rc[0] % 256, rc[1] % 256))
    return worst, "\n".join(lines)


def check(y, ref, tol, what="", family=None, dtype=None):
    """assert |y - ref| <= tol element-wise; records the worst ratio under (family, dtype)."""
    worst, msg = report(y, ref, tol, what)
    if family is not None:
        key = (family, NAME.get(dtype, str(dtype)))
        WORST[key] = max(WORST.get(key, 0.0), worst)
    assert not msg, msg
    return worst


def worst_table(families=None):
    """families: only these (a test file prints the ones it recorded itself)"""
    return "\n".join("  %-22s %-5s worst error / bound = %.3f" % (f, d, r) for (f, d), r in sorted(WORST.items())
                     if families is None or f in families)


def check_exact(y, expected, what="", family=None, dtype=None, alt=None):
    """bit-for-bit (compared as integers: -0 and NaN payloads count); recorded under (family, dtype) as ratio 0.  alt: a second
    admissible mirror (see euler_cfg_step_exact): an element must equal one of the two."""
    y, expected = y.cpu().contiguous(), expected.contiguous()
    if alt is not None:
        expected = torch.where(y.view(_INT[y.dtype]) == alt.contiguous().view(_INT[y.dtype]), alt.contiguous(), expected)
    assert y.shape == expected.shape and y.dtype == expected.dtype, "%s: %s %s, expected %s %s" % (what, tuple(y.shape), y.dtype, tuple(expected.shape), expected.dtype)
    it = _INT.get(y.dtype)
    a, b = (y.view(it), expected.view(it)) if it is not None else (y, expected)
    bad = (a != b).nonzero()
    if family is not None:
        key = (family, NAME.get(dtype, str(dtype)))
        WORST[key] = max(WORST.get(key, 0.0), float("inf") if bad.numel() else 0.0)
    assert not bad.numel(), "%s: %d of %d elements differ from the exact expectation, first at %s: got %r, expected %r" % (
        what, bad.shape[0], y.numel(), tuple(bad[0].tolist()), y[tuple(bad[0].tolist())].item(), expected[tuple(bad[0].tolist())].item())


# ---- guarded outputs ----------------------------------------------------------------------------------------------------------
SENTINEL = {torch.bfloat16: 0x7FA5, torch.float16: 0x7DA5, torch.float32: 0x7FA5A5A5}    # NaN bit patterns with a payload (compared as integers, never as floats)
_INT = {torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float32: torch.int32}


def _sentinel_int(dtype):
    return SENTINEL[dtype]      # sign bit clear: the same number as int16 / int32


class GuardedOut:
    """One flat allocation: [front guard | offset | rows x (width payload + (ld - width) gap) | back guard], every element preset
    to a NaN sentinel.  Guards are multiples of 16 bytes, so the payload keeps the alignment `offset` (in elements) asks for.
    `out` is the payload view handed to the kernel ([rows, width], row stride ld); `check()` asserts guards, offset and gaps are
    bit-identical to the sentinel and no sentinel remains in the payload, and returns the payload on the CPU."""
    GUARD_BYTES = 1024

    def __init__(self, rows, width, dtype, device="cpu", ld=None, offset=0):
        self.rows, self.width, self.dtype = int(rows), int(width), dtype
        self.ld = self.width if ld is None else int(ld)
        assert self.ld >= self.width and offset >= 0
        esz = 2 if dtype != torch.float32 else 4
        self.guard = self.GUARD_BYTES // esz
        self.start = self.guard + int(offset)
        body = (self.rows - 1) * self.ld + self.width if self.rows else 0
        self.total = self.start + body + self.guard
        self.flat = torch.full((self.total,), _sentinel_int(dtype), dtype=_INT[dtype], device=device)
        assert self.flat.data_ptr() % 16 == 0
        self.out = self.flat.view(dtype).as_strided((self.rows, self.width), (self.ld, 1), self.start)

    def view(self, *shape):
        """the (contiguous, ld == width) payload under another shape"""
        assert self.ld == self.width
        return self.flat.view(self.dtype)[self.start:self.start + self.rows * self.width].view(*shape)

    def data_ptr(self):
        return self.out.data_ptr()

    def problems(self, cpu=True, payload=True):
        """-> (messages, payload).  The comparisons run where the buffer lives (integers); the payload comes back on the CPU
        unless cpu=False.  payload=False checks guards, offset and gaps only (buffers a kernel fills in part, byte outputs)."""
        if self.flat.is_cuda:
            torch.cuda.synchronize()
        f = self.flat.cpu() if cpu else self.flat
        s = _sentinel_int(self.dtype)
        msgs = []
        body_end = self.start + ((self.rows - 1) * self.ld + self.width if self.rows else 0)
        front = (f[:self.start] != s).nonzero().flatten()
        if front.numel():
            msgs.append("%d elements written BEFORE the output (first at element %d of %d)" % (front.numel(), int(front[0]) - self.start, self.start))
        back = (f[body_end:] != s).nonzero().flatten()
        if back.numel():
            msgs.append("%d elements written PAST the output (first %d elements after its end)" % (back.numel(), int(back[0])))
        body = f[self.start:body_end]
        if self.ld > self.width and self.rows > 1:
            pad = torch.full((self.rows * self.ld - body.numel(),), s, dtype=f.dtype, device=f.device)
            grid = torch.cat([body, pad]).view(self.rows, self.ld)
            gap = (grid[:, self.width:] != s).nonzero()
            if gap.numel():
                msgs.append("%d gap elements written (first: row %d, column %d of a %d-wide row)"
                            % (gap.shape[0], int(gap[0, 0]), self.width + int(gap[0, 1]), self.width))
            pay = grid[:, :self.width]
        else:
            pay = body.view(self.rows, self.width)
        left = (pay == s).nonzero() if payload else pay[:0]
        if left.numel():
            r, c = int(left[0, 0]), int(left[0, 1])
            msgs.append("%d payload elements never written (first at (%d, %d): mod 16 = (%d, %d), mod 64 = (%d, %d), mod 256 = (%d, %d))"
                        % (left.shape[0], r, c, r % 16, c % 16, r % 64, c % 64, r % 256, c % 256))
        return msgs, pay.contiguous().view(self.dtype)

    def untouched(self, pay):
        """bool mask over a payload that check() returned: elements that still hold the sentinel bits"""
        return pay.view(_INT[self.dtype]) == _sentinel_int(self.dtype)

    def check(self, what="", cpu=True, payload=True):
        msgs, pay = self.problems(cpu, payload)
        assert not msgs, "%s: %s" % (what, "; ".join(msgs))
        return pay


class GuardedBytes(GuardedOut):
    """nbytes of raw output (a uint8 image, an opaque workspace) carved from a guarded fp32 allocation: 16-byte aligned, the
    bytes between nbytes and the next multiple of 4 belong to the guard."""

    def __init__(self, nbytes, device="cpu"):
        self.nbytes = int(nbytes)
        super().__init__(1, max((self.nbytes + 3) // 4, 1), torch.float32, device=device)

    def bytes(self, what=""):
        """asserts the guards (and the tail bytes of the last word) and returns the nbytes as uint8 on the CPU"""
        pay = self.check(what, payload=False).view(torch.uint8).flatten()
        fresh = torch.full((self.width,), _sentinel_int(self.dtype), dtype=torch.int32).view(torch.uint8)
        assert torch.equal(pay[self.nbytes:], fresh[self.nbytes:]), "%s: bytes written past the %d-byte output" % (what, self.nbytes)
        return pay[:self.nbytes].clone()


# ---- exact probes -------------------------------------------------------------------------------------------------------------
def boundary_indices(K):
    """0, K-1 and both sides of every multiple of 32 / 64 / 128 inside [0, K)."""
    s = {0, K - 1}
    for step in (32, 64, 128):
        for b in range(step, K, step):
            s.update((b - 1, b))
    return sorted(i for i in s if 0 <= i < K)


def selector_probe(M, N, K, dtype, seed=0):
    """A one-hot rows (A[m, pi(m)] = 1), W arbitrary -> (A, W, expected y[m, n] = W[n, pi(m)] exactly)."""
    g = torch.Generator().manual_seed(1000 + seed)
    idx = boundary_indices(K)
    pi = torch.tensor([idx[m % len(idx)] for m in range(M)])
    if M > len(idx):            # rows beyond the boundary list walk every k
        pi[len(idx):] = (torch.arange(M - len(idx)) * 7 + seed) % K
    A = torch.zeros(M, K, dtype=dtype)
    A[torch.arange(M), pi] = 1.0
    W = torch.randn(N, K, generator=g).to(dtype)
    return A, W, W[:, pi].t().contiguous()


def selector_probe_w(M, N, K, dtype, seed=0):
    """the mirrored form: W one-hot rows, A arbitrary -> expected y[m, n] = A[m, pi(n)]."""
    W, A, exp_t = selector_probe(N, M, K, dtype, seed + 500)
    return A, W, exp_t.t().contiguous()


def counter_probe(M, N, K, dtype, seed=0):
    """A all ones, W integers in [-4, 4]: every fp32 partial sum is an exact integer (|sum| <= 4 K < 2^24), so whatever the order,
    y = round_T(sum_k W[n, k]); a k taken twice or not at all changes the integer."""
    assert 4 * K < 2 ** 24
    g = torch.Generator().manual_seed(2000 + seed)
    W = torch.randint(-4, 5, (N, K), generator=g).to(dtype)
    A = torch.ones(M, K, dtype=dtype)
    exp = W.double().sum(1).to(dtype)[None, :].expand(M, N).contiguous()
    return A, W, exp


def conv_impulse_positions(B, H, W):
    """(b, h, w) of the impulse probes: corners, one pixel on each edge, w = W - 1 on an inner row, an interior pixel, and the
    last pixel of the last image."""
    hm, wm = H // 2, W // 2
    pos = [(0, 0, 0), (0, 0, W - 1), (0, H - 1, 0), (0, H - 1, W - 1), (0, 0, wm), (0, H - 1, wm), (0, hm, 0), (0, hm, W - 1),
           (0, max(hm - 1, 0), W - 1), (0, hm, wm), (B - 1, H - 1, W - 1), (B - 1, 0, 0)]
    out = []
    for p in pos:
        if p not in out:
            out.append(p)
    return out


def conv_impulse(B, Ci, H, W, pos, ci, dtype, value=1.0):
    x = torch.zeros(B, Ci, H, W, dtype=dtype)
    x[pos[0], ci, pos[1], pos[2]] = value
    return x


def conv_expected(x, w, dtype, stride=1, upsample=False):
    """fp64 conv2d rounded to T (exact for impulse inputs: every output is one product value * weight, or a sum of the <= 4
    products of an upsampled impulse, formed exactly in fp64)."""
    F = torch.nn.functional
    xd = x.double()
    if upsample:
        xd = F.interpolate(xd, scale_factor=2.0, mode="nearest")
    return F.conv2d(xd, w.double(), None, stride=stride, padding=1).to(dtype)


def attention_selector(Lq, Lk, hd, dtype, seed=0, H=1, kscale=1.0):
    """q_i = 128 (64 e0 + e1), k_j = hi(j) e0 + lo(j) e1 with j = 64 hi + lo, scale = 1: the scores are exactly 128 j (integers
    below 2^24 for Lk <= 4096; every operand is exact in bf16 / fp16), neighbouring keys differ by 128, and exp(-128) underflows
    to exactly 0 in fp32 — each query selects the LAST key it may see, bit for bit.  -> (q, k, v) [H, L, hd]; expected rows are
    v[:, j*] with j* = kv_len - 1, or i + Lk - Lq under the bottom-right causal mask.  Entry points that fix scale = 1 / sqrt(hd)
    take kscale = 16 (k stays exact: 63 * 16 needs 6 bits): neighbouring scores are then >= 128 * 16 / sqrt(hd) >= 128 apart for
    hd <= 256, the maximum still gets exp(0) = 1 and the rest underflow."""
    assert Lk <= 4096 and hd >= 2
    g = torch.Generator().manual_seed(3000 + seed)
    q = torch.zeros(H, Lq, hd)
    q[:, :, 0], q[:, :, 1] = 128.0 * 64.0, 128.0
    j = torch.arange(Lk)
    k = torch.zeros(H, Lk, hd)
    k[:, :, 0], k[:, :, 1] = (j // 64).float() * kscale, (j % 64).float() * kscale
    v = torch.randn(H, Lk, hd, generator=g)
    return q.to(dtype), k.to(dtype), v.to(dtype)


def attention_selector_expected(v, Lq, kv_len, causal):
    """v [H, Lk, hd] -> expected [H, Lq, hd]"""
    if causal:
        idx = torch.arange(Lq) + (kv_len - Lq)
    else:
        idx = torch.full((Lq,), kv_len - 1)
    return v[:, idx]


def poison_(t, seed=0):
    """fill t (any view) with alternating NaN / +Inf, in place"""
    n = t.numel()
    pat = torch.where(torch.arange(n) % 2 == 0, torch.tensor(float("nan")), torch.tensor(float("inf")))
    t.copy_(pat.view(t.shape).to(device=t.device, dtype=t.dtype))
    return t


# ---- the cases of tests/test_kernel_edges_gpu.py (tests/test_kernel_check_cpu.py runs a simulated kernel over every one) --------
GEMV_SHAPES = [(512, 256), (100, 512), (4096, 4096), (4096, 11008), (1000, 1664), (33, 8)]
GEMM_SHAPES = [(1, 64, 64), (37, 100, 256), (65, 4096, 4096), (114, 1000, 4096), (343, 768, 512),
               (130, 4992, 1664), (256, 1664, 608), (300, 256, 8192), (1024, 512, 1664)]
# every M of {129, 255, 256, 257, 520}, N of {72, 330, 640} and K of {1 .. 7 K tiles, 8, 24, 72} at least once
GEMM_EDGE_SHAPES = [(129, 72, 64), (255, 330, 128), (256, 640, 192), (257, 330, 256), (520, 640, 320), (520, 330, 384),
                    (256, 72, 448), (257, 640, 8), (129, 330, 24), (255, 72, 72)]
GEMM_EPILOGUES = ["plain", "bias", "residual", "bias+residual", "gelu", "geglu"]
# out aliases residual (ss_models.hip vit_blocks: attention out-projection and MLP down-projection of the ViT, rows = batch * 257;
# the resampler's toy width)
# + whole 256 x 320 tiles: the 320-wide ping-pong tiles 56 / 58 refuse anything else and hand the launch to tile 60
GEMM_INPLACE_SHAPES = [(257, 1664, 1664), (514, 1664, 8192), (1028, 1664, 1664), (514, 256, 512), (512, 1280, 640), (256, 320, 64)]
GEMM_PROBE_SHAPES = [(257, 330, 448), (129, 72, 24), (520, 640, 320), (512, 640, 320)]
GEMM_STRIDE_SHAPES = [(257, 330, 192), (256, 640, 128)]
GEMM_PERSISTENT_SHAPES = [(8200, 3840, 192), (8192, 10240, 128), (8192, 5120, 64), (16384, 2560, 640)]


def pp320_eligible(M, N, K):
    """the rule of pp_launch<T, 320, ...> (ss_gemm_pp.inc): whole 256 x 320 tiles, whole K tiles.  A hand copy (the library does
    not report which kernel ran): pp_launch carries a comment that points here, change both together."""
    return M % 256 == 0 and N % 320 == 0 and K % 64 == 0 and K >= 64


def conv_pp320_eligible(B, Ci, Co, H, W, stride, up):
    """the conv form of the same rule: stride 1, no upsample, W >= 8 and H powers of two, Cin % 64 == 0"""
    return (stride == 1 and not up and Ci % 64 == 0 and Ci <= 4096 and W >= 8 and W & (W - 1) == 0 and H & (H - 1) == 0 and (B * H * W) % 256 == 0
            and Co % 320 == 0)


def persistent_inputs(M, N, K, dtype, seed, device="cpu"):
    """operands of the persistent multi-tile cases: w ~ 0.05 N(0, 1), bias and residual ~ N(0, 1)"""
    g = torch.Generator(device=device).manual_seed(seed)
    a = torch.randn(M, K, device=device, dtype=dtype, generator=g)
    w = (torch.randn(N, K, device=device, generator=g) * 0.05).to(dtype)
    bias = torch.randn(N, device=device, dtype=dtype, generator=g)
    res = torch.randn(M, N, device=device, dtype=dtype, generator=g)
    return a, w, bias, res

# B, Cin, Cout, H, W, stride, upsample
CONV_EDGE_CASES = [(2, 8, 16, 4, 8, 1, False), (1, 64, 96, 16, 16, 1, False), (1, 128, 8, 33, 31, 1, False), (1, 64, 64, 64, 64, 1, False),
                   (2, 320, 64, 9, 8, 2, False), (1, 64, 40, 6, 5, 1, True), (1, 1920, 64, 8, 8, 1, False), (2, 64, 320, 16, 16, 1, False),
                   (1, 64, 256, 16, 16, 1, False)]
CONV_IMPULSE_CASES = [(2, 64, 32, 8, 8, 1, False), (2, 64, 32, 8, 8, 2, False), (2, 64, 32, 4, 8, 1, True), (2, 64, 256, 8, 16, 1, False),
                      (4, 64, 320, 8, 8, 1, False)]       # the last: whole 256 x 320 tiles (conv tile 56)
CONV_VARIANTS = [(), ("bias",), ("bias", "rowvec"), ("bias", "residual"), ("rowvec", "residual"), ("bias", "rowvec", "residual")]
# B, heads, hd, Lq, Lk, causal: Lq / Lk on both sides of 16 / 64 / 128, causal with Lk - Lq in {0, 1, 63, 64}
ATTN_EDGE_CASES = [(1, 2, 64, 15, 17, False), (2, 2, 64, 63, 65, False), (1, 2, 64, 129, 127, False), (1, 2, 64, 128, 128, True),
                   (1, 2, 64, 64, 65, True), (1, 2, 64, 65, 128, True), (1, 2, 64, 64, 128, True), (1, 2, 64, 17, 17, True),
                   (1, 2, 128, 16, 15, False), (1, 2, 128, 65, 63, False), (2, 2, 128, 127, 129, False), (1, 2, 128, 129, 129, True),
                   (1, 2, 128, 127, 128, True), (1, 2, 128, 65, 128, True), (1, 2, 128, 63, 127, True),
                   (1, 2, 104, 17, 64, False), (1, 2, 104, 128, 65, False), (1, 2, 104, 64, 64, True), (1, 2, 104, 33, 96, True),
                   (1, 2, 104, 64, 65, True), (1, 2, 104, 64, 128, True),
                   # several 128 / 256 / 512-row query blocks with a ragged last one (the 4 / 8 / 16-wave v3p kernels)
                   (1, 2, 64, 600, 333, False), (1, 2, 64, 700, 763, True),
                   # batch x heads = 8 with several ragged query blocks: the XCD-aware 1-D work-group mapping (v3 at 128 rows, v3p at 128 / 256 / 512)
                   (1, 8, 64, 600, 333, False), (1, 8, 64, 600, 763, True), (1, 8, 128, 300, 333, True)]
# attention_cache / attention_cache_slots: heads, hd, cap, rows per slot, kv_lens (unequal), one per slot
ATTN_CACHE_CASES = [(2, 128, 200, 17, [17, 81, 128, 200]), (2, 64, 160, 40, [40, 41, 103, 104, 129]), (2, 128, 300, 66, [66, 67, 130, 257]),
                    (2, 104, 96, 8, [8, 9, 71, 72]), (2, 104, 96, 40, [40, 41, 95, 96])]
DECODE_NSPLITS = [0, 4, 8, 16, 32]
DECODE_HEADS, DECODE_CAP = 4, 1200


def decode_kv_lens(nsplit):
    ns = nsplit if nsplit else 16
    return sorted({1, ns - 1, ns, ns + 1, 500, DECODE_CAP})


DECODE_KV_LENS = sorted({kvl for ns in DECODE_NSPLITS for kvl in decode_kv_lens(ns)})      # every length runs at every split count


GEMV_NB = [1, 2, 3, 4, 5, 8, 16]
GEMV_SILU_SHAPES = [(256, 256), (512, 4096), (100, 512)]        # I, K


def epilogue_inputs(name, M, N, dtype, seed):
    """bias / residual of a GEMM epilogue case -> kwargs of gemm_bound (CPU tensors)"""
    g = torch.Generator().manual_seed(7000 + seed)
    bias = (torch.randn(N, generator=g) * 0.5).to(dtype)
    res = torch.randn(M, N, generator=g).to(dtype)
    return {"plain": {}, "bias": {"bias": bias}, "residual": {"residual": res}, "bias+residual": {"bias": bias, "residual": res},
            "gelu": {"bias": bias, "gelu_": True}, "geglu": {"bias": bias, "geglu": True}}[name]


def gemm_inputs(M, N, K, dtype, seed):
    """fresh operands per case: a ~ N(0, 1), w ~ N(0, 1 / K) so the product is O(1) in every dtype"""
    g = torch.Generator().manual_seed(5000 + seed)
    return torch.randn(M, K, generator=g).to(dtype), (torch.randn(N, K, generator=g) / K ** 0.5).to(dtype)


def conv_inputs(B, Ci, Co, H, W, stride, up, dtype, seed):
    g = torch.Generator().manual_seed(6000 + seed)
    x = torch.randn(B, Ci, H, W, generator=g).to(dtype)
    w = (torch.randn(Co, Ci, 3, 3, generator=g) / (9 * Ci) ** 0.5).to(dtype)
    bias = (torch.randn(Co, generator=g) * 0.5).to(dtype)
    tv = (torch.randn(B, Co, generator=g) * 0.5).to(dtype)
    Hin, Win = (2 * H, 2 * W) if up else (H, W)
    Ho, Wo = (Hin - 1) // stride + 1, (Win - 1) // stride + 1
    res = torch.randn(B, Co, Ho, Wo, generator=g).to(dtype)
    return x, w, bias, tv, res


def attn_inputs(B, H, hd, Lq, Lk, dtype, seed):
    g = torch.Generator().manual_seed(8000 + seed)
    E = H * hd
    return (torch.randn(B, Lq, E, generator=g).to(dtype), torch.randn(B, Lk, E, generator=g).to(dtype),
            torch.randn(B, Lk, E, generator=g).to(dtype))


def heads(x, H):
    """[B, L, H * hd] -> [B, H, L, hd]"""
    B, L, E = x.shape
    return x.view(B, L, H, E // H).transpose(1, 2)


def unheads(x):
    """[B, H, L, hd] -> [B, L, H * hd]"""
    B, H, L, hd = x.shape
    return x.transpose(1, 2).reshape(B, L, H * hd)


# ==== norms, softmax, point-wise kernels, loss heads (tests/test_pointwise_edges_gpu.py) ======================================
def vec(dtype):
    """elements per 16-byte pack"""
    return 4 if dtype == torch.float32 else 8


def esize(dtype):
    return 4 if dtype == torch.float32 else 2


def gamma(n):
    return n * U32 / (1.0 - n * U32)


def sqrt32(v, t):
    lo = (v - t).clamp_min(0.0)
    den = lo.sqrt() + v.sqrt()
    return op32(v.sqrt(), torch.where(t > 0, t / den.clamp_min(1e-300), torch.zeros_like(t)))


def recip32(v, t):
    return op32(1.0 / v, t / (v.abs() * (v.abs() - t).clamp_min(1e-300)))


def exp32(v, t):
    e = torch.exp(v)
    return e, e * torch.expm1(t) + 4.0 * U32 * e


def rmsnorm_bound(x, w, eps, dtype):
    """x [rows, cols], w [cols] -> (reference, bound) of ss_rmsnorm"""
    xd, wd = x.double(), w.double()
    cols = x.shape[1]
    ss = (xd * xd).sum(1, keepdim=True)
    v, t = op32(ss / cols, gamma(cols) * ss / cols)
    v, t = op32(v + float(np.float32(eps)), t)
    v, t = recip32(*sqrt32(v, t))
    h, th = op32(xd * v, xd.abs() * t)
    h, th = mid_round(h, th, dtype)
    return final_round(wd * h, wd.abs() * th, dtype)


def _two_pass_stats(xd, eps, fma_squares=True):
    """the first half of the two-pass LayerNorm kernels (layernorm, ss_rowstats, the LN-fused fp8 quantiser) on xd [rows, cols]
    fp64 -> (mean, t_mean, d, t_d, rstd, t_rstd).  fma_squares=False: d * d is rounded before it is added (one more rounding per
    term: the quantiser's `ss2 += d * d` under -ffp-contract=off)."""
    cols = xd.shape[1]
    mean, tm = op32(xd.mean(1, keepdim=True), gamma(cols) * xd.abs().mean(1, keepdim=True))
    d, td = op32(xd - mean, tm.expand_as(xd))
    s2 = (d * d).sum(1, keepdim=True)
    ts2 = (2.0 * d.abs() * td + td * td).sum(1, keepdim=True) + gamma(cols if fma_squares else cols + 1) * ((d.abs() + td) ** 2).sum(1, keepdim=True)
    v, t = op32(s2 / cols, ts2 / cols)
    v, t = op32(v + float(np.float32(eps)), t)
    rv, rt = recip32(*sqrt32(v, t))
    return mean, tm, d, td, rv, rt


def layernorm_bound(x, w, b, eps, dtype, fma_squares=True):
    """x [rows, cols], w / b [cols] -> (reference, bound) of ss_layernorm (block and wave kernels)"""
    xd, wd, bd = x.double(), w.double(), b.double()
    _, _, d, td, rv, rt = _two_pass_stats(xd, eps, fma_squares)
    v, t = product(d, td, rv.expand_as(d), rt.expand_as(d))
    v, t = op32(v * wd, t * wd.abs())
    v, t = op32(v + bd, t)
    return final_round(v, t, dtype)


# ss_diffusion.hip groupnorm_rows_per_block: "~128 KiB of activations per block", at least 16 rows.  A hand copy (the library
# does not report its launch geometry); groupnorm_rows_per_block carries a comment that points here, change both together.
GN_ROWS_MAX_BYTES = 128 * 1024


def groupnorm_rows_per_block(B, HW, C, dtype):
    """the whole launch rule (the CPU simulation needs the block boundaries; the bound only the maximum)"""
    rpb = max(16, GN_ROWS_MAX_BYTES // (C * esize(dtype)))
    while rpb > 16 and B * (-(-HW // rpb)) < 2048:
        rpb //= 2
    return min(rpb, HW)


def groupnorm_bound(x, gw, gb, G, eps, silu_, dtype):
    """x [B, HW, C], gw / gb [C] -> (reference, bound) [B, HW, C] of ss_groupnorm"""
    B, HW, C = x.shape
    cg = C // G
    n = HW * cg
    k = min(HW, max(16, GN_ROWS_MAX_BYTES // (C * esize(dtype))))
    xd = x.double().view(B, HW, G, cg)
    ga, be = gw.double().view(1, 1, G, cg), gb.double().view(1, 1, G, cg)
    c = gamma(k) + 2.0 * U32
    S1, S2 = xd.sum((1, 3), keepdim=True), (xd * xd).sum((1, 3), keepdim=True)
    md, tmd = S1 / n, c * xd.abs().sum((1, 3), keepdim=True) / n
    var = (S2 / n - md * md).clamp_min(0.0)
    tvar = c * S2 / n + 2.0 * md.abs() * tmd + tmd * tmd
    mean, tmean = op32(md, tmd)
    v, t = op32(var, tvar)
    v, t = op32(v + float(np.float32(eps)), t)
    rv, rt = recip32(*sqrt32(v, t))
    sc, tsc = op32(rv * ga, rt * ga.abs())
    # x sc' + sh' = (x - mean') sc' + beta up to the roundings of mean' sc', of sh' and of the fma: the error of sc meets x - mean
    sh = be - mean * sc
    v = xd * sc + sh
    t = (xd - mean).abs() * tsc + sc.abs() * tmean + tmean * tsc
    t = t + U32 * ((mean * sc).abs() + sh.abs() + v.abs() + 3.0 * t)
    if silu_:
        v, t = mid_round(v, t, dtype)
        v, t = _apply(_silu, _silu_d, 1.1, 0.5, v, t, 2.0 ** -21)
    v, t = final_round(v, t, dtype)
    return v.reshape(B, HW, C), t.reshape(B, HW, C)


def softmax_rows_bound(x, scale, dtype):
    """x [rows, cols] -> (reference, bound) of ss_softmax_rows (in place on x)"""
    sc = float(np.float32(scale))
    s, ts = op32(x.double() * sc, torch.zeros_like(x, dtype=torch.float64))
    m = s.amax(1, keepdim=True)
    e, te = exp32(*op32(s - m, ts))
    tot, ttot = op32(e.sum(1, keepdim=True), te.sum(1, keepdim=True) + gamma(x.shape[1]) * e.sum(1, keepdim=True))
    iv, it = recip32(tot, ttot)
    v, t = product(e, te, iv.expand_as(e), it.expand_as(e))
    return final_round(v, t, dtype)


def silu_mul_ew_bound(gu, dtype):
    """gu [rows, 2 I] = [gate | up] -> (reference, bound) of ss_silu_mul"""
    I = gu.shape[1] // 2
    g, u = gu[:, :I].double(), gu[:, I:].double()
    v, t = silu(g, torch.zeros_like(g), dtype)
    v, t = mid_round(v, t, dtype)
    return final_round(v * u, t * u.abs(), dtype)


def geglu_ew_bound(x, dtype):
    """x [rows, 2 D] = [val | gate] -> (reference, bound) of ss_geglu"""
    D = x.shape[1] // 2
    a, g = x[:, :D].double(), x[:, D:].double()
    v, t = gelu(g, torch.zeros_like(g), dtype)
    v, t = mid_round(v, t, dtype)
    return final_round(v * a, t * a.abs(), dtype)


def unary_bound(x, op, dtype):
    """op 0: silu, 1: gelu"""
    xd = x.double()
    v, t = (silu if op == 0 else gelu)(xd, torch.zeros_like(xd), dtype)
    return final_round(v, t, dtype)


def l2normalize_bound(x, dtype):
    """x [B, L, C], normalised over dim 1"""
    xd = x.double()
    L = x.shape[1]
    s = (xd * xd).sum(1, keepdim=True)
    v, t = sqrt32(s, gamma(L) * s)
    v, t = mid_round(v, t, dtype)
    floor = float(np.float32(1e-12))
    v = v.clamp_min(floor)
    q, tq = op32(xd / v, xd.abs() * t / (v * (v - t).clamp_min(floor)))
    return final_round(q, tq, dtype)


def cross_entropy_rows_bound(logits, labels, dtype, ignore_index=-100):
    """logits [rows, vocab] (the valid columns only), labels [rows] -> (loss reference, bound, valid flags) per row"""
    x = logits.double()
    rows, vocab = x.shape
    valid = (labels != ignore_index) & (labels >= 0) & (labels < vocab)
    lab = labels.clamp(0, vocab - 1)
    m = x.amax(1, keepdim=True)
    e, te = exp32(*op32(x - m, torch.zeros_like(x)))
    s, ts = e.sum(1), te.sum(1) + gamma(vocab) * e.sum(1)
    lg = torch.log(s)
    tlg = ts / (s - ts).clamp_min(0.5) + 4.0 * U32 * lg.abs()
    a, ta = op32(x.gather(1, lab[:, None])[:, 0] - m[:, 0], torch.zeros(rows, dtype=torch.float64))
    v, t = op32(a - lg, ta + tlg)
    v, t = final_round(v, t, dtype)
    z = torch.zeros_like(v)
    return torch.where(valid, -v, z), torch.where(valid, t, z), valid.double()


def cosine_rows_bound(rec, tgt, dtype):
    """rec / tgt [rows, dim] -> (reference, bound) [rows] of ss_cosine_rows"""
    dim = rec.shape[1]

    def unit(a):
        ad = a.double()
        s = (ad * ad).sum(1, keepdim=True)
        n, tn = mid_round(*sqrt32(s, gamma(dim) * s), dtype)
        q, tq = op32(ad / n, ad.abs() * tn / (n * (n - tn).clamp_min(1e-300)))
        return mid_round(q, tq, dtype)
    (x, tx), (y, ty) = unit(rec), unit(tgt)
    p, tp = mid_round(*product(y, ty, x, tx), dtype)
    s, ts = mid_round(p.sum(1), tp.sum(1) + gamma(dim) * (p.abs() + tp).sum(1), dtype)
    v, t = op32(1.0 - s, ts)
    return final_round(v, t, dtype)


def mse_bound(a, b):
    """-> (reference, bound) scalars of ss_mse: fl(fl(a - b)^2) summed in fp64, one division, one narrowing"""
    d = (a.double() - b.double()).flatten()
    n = d.numel()
    terms = d * d
    return terms.sum() / n, ((4.0 * U32 + n * 2.0 ** -52) * terms.sum() + n * 2.0 ** -149) / n


def masked_mean_bound(vals, mask):
    """-> (mean reference, bound, count) of ss_masked_mean (fp32 inputs)"""
    v = vals.double().flatten()
    m = torch.ones_like(v) if mask is None else mask.double().flatten()
    cnt = float(m.sum())
    if cnt <= 0:
        return torch.zeros((), dtype=torch.float64), torch.zeros((), dtype=torch.float64), 0.0
    terms = v * m
    n = v.numel()
    return terms.sum() / cnt, ((2.0 * U32 + n * 2.0 ** -52) * terms.abs().sum() + n * 2.0 ** -149) / cnt, cnt


def euler_scale_dup_bound(x, sigma, dtype):
    """-> (reference, bound) [2, n] of ss_euler_scale_dup"""
    sg = torch.tensor(float(np.float32(sigma)), dtype=torch.float64)
    v, t = op32(sg * sg, torch.zeros((), dtype=torch.float64))
    v, t = op32(v + 1.0, t)
    iv, it = recip32(*sqrt32(v, t))
    xd = x.double().flatten()
    v, t = final_round(*op32(xd * iv, xd.abs() * it), dtype)
    return torch.stack([v, v]), torch.stack([t, t])


# ---- exact mirrors (fp32 on the CPU, the kernel's rnd points) ---------------------------------------------------------------
def r32(x, dtype):
    """fp32 -> T -> fp32"""
    return x.to(dtype).float()


def add_bcast_exact(x, pos):
    return (x.float() + pos.float()[None]).to(x.dtype)


def rope_tables(hd, max_pos, dtype, base=10000.0):
    """cat(freqs, freqs) cos / sin tables [max_pos, hd] cast to T (the LLaMA rotary embedding)"""
    inv_freq = 1.0 / (base ** (torch.arange(0, hd, 2).float() / hd))
    fr = torch.arange(max_pos, dtype=torch.float32)[:, None] * inv_freq[None]
    emb = torch.cat([fr, fr], -1)
    return emb.cos().to(dtype), emb.sin().to(dtype)


def rope_exact(x, cos, sin, pos):
    """x [M, H, hd] T, cos / sin [P, hd] T, pos [M] -> rnd(rnd(x c) + rnd(rot(x) s)) [M, H, hd] T"""
    dtype = x.dtype
    half = x.shape[-1] // 2
    xf = x.float()
    c, s = cos[pos].float()[:, None], sin[pos].float()[:, None]
    rot = torch.cat([-xf[..., half:], xf[..., :half]], -1)
    return (r32(xf * c, dtype) + r32(rot * s, dtype)).to(dtype)


def euler_cfg_step_exact(x, eps, guidance, sigma, sigma_next, fused_f16=False):
    """x [n] T, eps [2, n] T -> x after ss_euler_cfg_step.
    fused_f16 (fp16 only): rnd_T(s v), an fp32 scalar s times a value v of T, written as an fp32 product followed by a conversion,
    is compiled for gfx950 to one v_fma_mixlo_f16, which converts the EXACT product to fp16: one rounding where the source (and
    torch's fp16 multiply) has two.  The two differ when the fp32 product lands on an fp16 midpoint the exact product is not on:
    about 2^-11 of the elements for a 24-bit dsigma, none for a guidance of a few bits.  Both are roundings of the same product
    and which one comes out is the compiler's choice, so the fp16 check admits either, element by element (found on the MI355X:
    96 of 1,048,579 elements at sigma 0.0413 -> 0, exactly the elements this flag changes)."""
    dtype = x.dtype
    g = torch.tensor(guidance, dtype=torch.float32)
    ds = torch.tensor(sigma_next, dtype=torch.float32) - torch.tensor(sigma, dtype=torch.float32)

    def mul(s, v):
        if fused_f16:           # numpy converts float64 -> float16 in one step (torch goes through fp32)
            assert dtype == torch.float16
            return torch.from_numpy((v.double().numpy() * float(s)).astype(np.float16)).float()
        return r32(s * v, dtype)
    eu, ec = eps[0].float(), eps[1].float()
    e = r32(eu + mul(g, r32(ec - eu, dtype)), dtype)
    return (x.float() + mul(ds, e)).to(dtype)


def image_to_u8_exact(x, pixels, half_up=False):
    """x [pixels, cpad] T -> uint8 [pixels, 3].  half_up: the mutant (floor(v + 0.5))"""
    v = r32(x[:pixels, :3].float() * 0.5 + 0.5, x.dtype).clamp(0.0, 1.0) * 255.0
    return (torch.floor(v + 0.5) if half_up else torch.round(v)).to(torch.uint8)


def im2col_exact(img, P, kpad):
    """img [B, 3, S, S] -> [B G G, kpad], column (c P + dy) P + dx, zero beyond 3 P P"""
    B, _, S, _ = img.shape
    G = S // P
    t = img.view(B, 3, G, P, G, P).permute(0, 2, 4, 1, 3, 5).reshape(B * G * G, 3 * P * P)
    out = torch.zeros(B * G * G, kpad, dtype=img.dtype)
    out[:, :3 * P * P] = t
    return out


# ---- cases and inputs --------------------------------------------------------------------------------------------------------
NORM_BLOCK_ROWS, NORM_BLOCK_PACKS = [1, 3], [1, 255, 256, 257, 2048]
LN_WAVE_ROWS, LN_WAVE_PACKS = [256, 257, 259], [1, 63, 64, 65, 255, 256]
LN_KNOB_ROWS, LN_KNOB_PACKS, LN_KNOBS = [8192, 8193, 8195, 8199], [1, 65], [1, 2, 4]
NORM_EPS = 1e-5


def norm_inputs(rows, cols, dtype, seed, zero_row=False):
    """N(0.3, 2^2) rows; the last row of three or more (and the only row of one-row cases with an odd seed) is replaced:
    rows >= 3 carry an offset row (mean 50, std 0.5: |mean| / std = 100) and a constant row, RMSNorm also an all-zero row."""
    g = torch.Generator().manual_seed(11000 + seed)
    x = torch.randn(rows, cols, generator=g) * 2.0 + 0.3
    if rows >= 3:
        x[1] = torch.randn(cols, generator=g) * 0.5 + 50.0
        x[2] = 1.75
        if zero_row:
            x[0] = 0.0
    elif seed % 2:
        x[0] = torch.randn(cols, generator=g) * 0.5 + 50.0
    w = torch.randn(cols, generator=g) * 0.1 + 1.0
    b = torch.randn(cols, generator=g) * 0.1
    return x.to(dtype), w.to(dtype), b.to(dtype)


def gn_cases(dtype):
    V = vec(dtype)
    return [(2, 35, 64, 32), (1, 17, 320, 32), (1, 1, 128, 32), (2, 145, 256, 256), (1, 33, 66 * V, 264), (1, 16, 257 * V, 1)]


def gn_inputs(B, HW, C, dtype, seed, offset=False):
    """N(0.5, 2^2), or mean 8 / std 1 in every group (offset)"""
    g = torch.Generator().manual_seed(12000 + seed)
    x = torch.randn(B, HW, C, generator=g) + 8.0 if offset else torch.randn(B, HW, C, generator=g) * 2.0 + 0.5
    return x.to(dtype), (torch.randn(C, generator=g) * 0.1 + 1.0).to(dtype), (torch.randn(C, generator=g) * 0.1).to(dtype)


SOFTMAX_ROWS, SOFTMAX_PACKS, SOFTMAX_SCALES = [1, 3], [1, 255, 256, 257, 1000], [0.3, -0.3]


def softmax_inputs(rows, cols, dtype, seed):
    """N(0, 3^2); with three rows: row 1 has one entry 80 above the rest, row 2 is constant"""
    g = torch.Generator().manual_seed(13000 + seed)
    x = torch.randn(rows, cols, generator=g) * 3.0
    if rows >= 3:
        x[1] = x[1].clamp(-9.0, 9.0)
        x[1, (7 * seed + cols // 2) % cols] = x[1].max() + 80.0
        x[2] = -2.5
    return x.to(dtype)


def gated_shapes(dtype):
    V = vec(dtype)
    return [(1, V), (3, 33 * V), (1025, 1025 * V)]


def gated_inputs(rows, inter, dtype, seed):
    """[rows, 2 inter]: both halves span -20 .. 20 and hold exact zeros (silu_mul gates on the left, geglu gates on the right)"""
    g = torch.Generator().manual_seed(14000 + seed)
    x = (torch.rand(rows, 2 * inter, generator=g) * 40.0 - 20.0)
    x[:, ::7] *= 0.05
    x[0, 0], x[0, inter], x[-1, -1], x[-1, inter - 1] = 0.0, 0.0, -20.0, 20.0
    return x.to(dtype)


def add_bcast_shapes(dtype):
    V = vec(dtype)
    return [(1, 1, V), (3, 5, 7 * V), (5, 1031, 204 * V)]


EW_N = [1, 257, 1048579]
EULER_SIGMAS = [(11.476846458, 9.543582567), (0.041314412, 0.0)]      # both ends of the 30-step table (tests/test_sdxl_oracle.py)
EULER_GUIDANCE = [0.0, 1.0, 7.5]
U8_CASES = [(px, cpad) for px in (1, 85, 349527) for cpad in (4, 8)]


def u8_inputs(pixels, cpad, dtype, seed):
    """[pixels, cpad]: N(0, 0.8^2), then (as far as they fit) every level 2 (k / 255) - 1, the 127.5 tie 0, +-1, +-1.5 and the
    neighbours of each tie (k + 0.5) / 127.5 - 1 in T"""
    g = torch.Generator().manual_seed(15000 + seed)
    x = torch.randn(pixels, cpad, generator=g) * 0.8
    k = torch.arange(256, dtype=torch.float64)
    special = torch.cat([2.0 * k / 255.0 - 1.0, torch.tensor([0.0, 1.0, -1.0, 1.5, -1.5], dtype=torch.float64), (k + 0.5) / 127.5 - 1.0]).float()
    flat = x[:, :3].reshape(-1).clone()
    m = min(flat.numel(), special.numel())
    flat[:m] = special[:m] if pixels > 1 else torch.tensor([0.0, 1.5, -1.0])[:m]
    x[:, :3] = flat.view(pixels, 3)
    return x.to(dtype)


def gather_cases(dtype):
    V = vec(dtype)
    return [(5, 9, V), (37, 50, 33 * V), (4100, 300, 257 * V)]       # n, table rows, cols


TRANSPOSE_SHAPES = [(1, 1), (31, 33), (32, 32), (33, 31), (45, 70), (65, 129), (1, 1000), (1000, 1)]


def concat_cases(dtype):
    V = vec(dtype)
    return [(1, V, V), (11, 8 * V, 3 * V), (7, V, 40 * V), (4099, 200 * V, 56 * V)]      # the last: 1,049,344 packs


LAYOUT_CASES = [(1, 4, 1, 8), (2, 4, 30, 8), (2, 3, 35, 4), (1, 8, 9, 8), (1, 4, 300000, 8)]
IM2COL_CASES = [(1, 14, 14, 588), (2, 56, 14, 640), (1, 28, 7, 152)]
IM2COL_LARGE = (6, 224, 14, 688)          # 6 * 256 * 688 = 1,056,768 elements: the grid-stride loop
ROPE_HD, ROPE_M, ROPE_MAXPOS = [2, 64, 104, 128, 256], [1, 6], 512
L2_CASES = [(1, 1, 1), (2, 16, 256), (3, 7, 257)]
CE_VOCABS, CE_PAD = [1, 255, 256, 257, 32066], 24
COSINE_DIMS, COSINE_ROWS = [1, 63, 64, 65, 4096], [1, 4, 5]
MEAN_N = [1, 255, 65536, 65537, 200001]


def randn_t(shape, dtype, seed, std=1.0, mean=0.0):
    g = torch.Generator().manual_seed(16000 + seed)
    return (torch.randn(*shape, generator=g) * std + mean).to(dtype)


# ==== GEMM variants: fp8, LN-folded, statistics producers, split-K (tests/test_gemm_variants_edges_gpu.py) ====================
F8 = torch.float8_e4m3fn
E64 = 2.0 ** -48          # what an fp64 sum / product chain of a few thousand terms can lose, relative
U8 = 2.0 ** -4            # unit roundoff of e4m3 (3 mantissa bits)
ETA8 = 2.0 ** -10         # half the e4m3 subnormal spacing (2^-9), in code units


def f8_values(codes):
    """e4m3 bytes (uint8) -> their values in fp64"""
    return codes.view(F8).double()


def quantize_rows_e4m3(x):
    """the quantiser restated on the CPU in fp32 (s = amax / 448, q = RNE(x * (448 / amax))) -> (codes uint8, scale fp32)"""
    xf = x.float()
    amax = xf.abs().amax(1)
    inv = torch.where(amax > 0, torch.full_like(amax, 448.0) / amax, torch.zeros_like(amax))
    return (xf * inv[:, None]).to(F8).view(torch.uint8), amax / 448.0


def gemm_fp8_bound(a8, sa, w8, sw, bias=None, residual=None, gelu_=False, geglu=False):
    """a8 [M, K] / w8 [N, K] e4m3 bytes, sa [M] / sw [N] fp32 -> (reference, bound) of ss_gemm_fp8 (bf16 out)"""
    v, t = accumulate(f8_values(a8), f8_values(w8))
    s = (sa.float()[:, None] * sw.float()[None, :]).double()        # fl(sa sw): the kernel's own fp32 product
    v, t = op32(v * s, t * s.abs())
    return epilogue(v, t, torch.bfloat16, bias=bias, gelu_=gelu_, residual=residual, geglu=geglu)


def gemm_lnfold_bound(x, wg, rstd, shift, colsum, dtype, bias_d=None, gelu_=False, geglu=False, t_rstd=None, t_shift=None):
    """x [M, K], wg [N, K] (T), rstd / shift [M], colsum [N] fp32 -> (reference, bound) of ss_gemm_lnfold.  t_rstd / t_shift [M]:
    the statistics are known to these tolerances only (ss_gemm_lnfold_part)."""
    av, at = accumulate(x, wg)
    rs, sh, cs = rstd.double()[:, None], shift.double()[:, None], colsum.double()[None, :]
    trs = torch.zeros_like(rs) if t_rstd is None else t_rstd.double()[:, None]
    tsh = torch.zeros_like(sh) if t_shift is None else t_shift.double()[:, None]
    p, tp = av * rs, at * rs.abs() + (av.abs() + at) * trs
    c, tc = op32(sh * cs, cs.abs() * tsh)
    v = p + c
    t = tp + tc + U32 * (p.abs() + c.abs() + tp + tc)
    return epilogue(v, t, dtype, bias=bias_d, gelu_=gelu_, geglu=geglu)


def _stats_from_sums(a, b, width, eps, u_inv):
    """a = sum x, b = sum x^2 [M] fp64 (exact inputs) -> ((rstd, t), (shift, t)) of the fp64 E[x^2] - mean^2 form narrowed to
    fp32; u_inv: relative error of the kernel's 1 / width"""
    e = u_inv + E64
    mean, ex2 = a / width, b / width
    tmean = e * mean.abs()
    var = (ex2 - mean * mean).clamp_min(0.0)
    tvar = e * ex2.abs() + 2.0 * mean.abs() * tmean + tmean * tmean + E64 * (ex2.abs() + mean * mean)
    ve = var + float(np.float32(eps))
    r = 1.0 / ve.sqrt()
    lo = (ve - tvar).clamp_min(1e-300)
    r, tr = op32(r, 0.5 * tvar * lo ** -1.5 + E64 * r)
    m32, tm32 = op32(mean, tmean)
    s, ts = op32(-m32 * r, m32.abs() * tr + r.abs() * tm32 + tr * tm32)
    return (r, tr), (s, ts)


def lnfold_part_stats_bound(part, width, eps):
    """part [M, strips, 2] fp32 -> ((rstd, t_rstd), (shift, t_shift)) the consumer's epilogue forms (ln_inv_width is fp32)"""
    pd = part.double()
    return _stats_from_sums(pd[:, :, 0].sum(1), pd[:, :, 1].sum(1), width, eps, U32)


def rowstat_finalize_bound(acc, width, eps):
    """acc [M, 2] fp64 -> ((rstd, t), (shift, t)) of ss_rowstat_finalize (1 / width in fp64)"""
    return _stats_from_sums(acc[:, 0].double(), acc[:, 1].double(), width, eps, 2.0 ** -53)


def rowstats_bound(x, eps, dtype):
    """x [M, K] (T) -> ((rstd, t), (shift, t)) [M] of ss_rowstats"""
    mean, tm, _, _, rv, rt = _two_pass_stats(x.double(), eps)
    s, ts = product(-mean, tm, rv, rt)
    return (rv[:, 0], rt[:, 0]), (s[:, 0], ts[:, 0])


def rowsum_bound(y, tn=None):
    """y [M, N]: the STORED output -> ((S1, t1), (S2, t2)), [M, N / tn] per strip of tn columns, or [M] per row (tn=None: the
    fp64 accumulator over fp32 pieces)"""
    yd = y.double()
    M, N = yd.shape
    if tn is None:
        s1, a1, s2, n, extra = yd.sum(1), yd.abs().sum(1), (yd * yd).sum(1), N, E64
    else:
        assert N % tn == 0
        ys = yd.view(M, N // tn, tn)
        s1, a1, s2, n, extra = ys.sum(2), ys.abs().sum(2), (ys * ys).sum(2), tn, 0.0
    return (s1, (gamma(n) + extra) * a1), (s2, (gamma(n + 1) + extra) * s2)


def gemm_splitk_bound(a, w, dtype, S, bias=None, residual=None):
    """(reference, bound) of ss_gemm_splitk at S slices"""
    v, t = accumulate(a, w, kacc=a.shape[1] + S)
    return epilogue(v, t, dtype, bias=bias, residual=residual)


def quantize_ln_bound(x, g, b, eps, dtype):
    """x [M, K], g / b [K] -> ((LayerNorm reference, bound of q * s), (scale reference, bound)) of quantize_rows_fp8(x, ln=)"""
    v, t = layernorm_bound(x, g, b, eps, dtype, fma_squares=False)
    tmax = t.amax(1)
    s = v.abs().amax(1) / 448.0
    ts = tmax / 448.0 + U32 * (s + tmax / 448.0)
    tq = t + (U8 + 4.0 * U32) * (v.abs() + t) + ETA8 * (s + ts)[:, None]
    return (v, tq), (s, ts)


def fp8_probe(kind, M, N, K, seed=0):
    """exact fp8 probes: operands that quantise exactly.  One-hot (or all-ones) rows: code value 448, scale fl(1 / 448); integer
    rows in [-4, 4] with one entry +-7: code values 64 w, scale 7 / 448 = 2^-6.  -> (a8, sa, w8, sw, expected bf16): the two
    de-quantisation products mirrored in fp32 (every partial sum is 2^12 x an integer below 2^24: exact in any order)."""
    g = torch.Generator().manual_seed(3500 + seed)

    def ints(R):
        w = torch.randint(-4, 5, (R, K), generator=g).float()
        w[torch.arange(R), (torch.arange(R) * 5 + seed) % K] = torch.where(torch.arange(R) % 2 == 0, 7.0, -7.0)
        return w * 64.0, torch.full((R,), 2.0 ** -6)

    def onehot(R, sd):
        return selector_probe(R, 1, K, torch.float32, sd)[0] * 448.0, torch.full((R,), 1.0) / 448.0
    if kind == "selector":
        (a, sa), (w, sw) = onehot(M, seed), ints(N)
    elif kind == "selector_w":
        (a, sa), (w, sw) = ints(M), onehot(N, seed + 500)
    else:
        (a, sa), (w, sw) = (torch.full((M, K), 448.0), torch.full((M,), 1.0) / 448.0), ints(N)
    acc = a.double() @ w.double().t()
    assert float(acc.abs().max()) < 2.0 ** 36 and torch.equal(acc.float().double(), acc)
    exp = (acc.float() * (sa[:, None] * sw[None, :])).to(torch.bfloat16)
    return a.to(F8).view(torch.uint8), sa, w.to(F8).view(torch.uint8), sw, exp


# ---- cases ---------------------------------------------------------------------------------------------------------------------
FP8_TILES = [0, 80, 81, 82, 85, 86, 88]
# every M of {63, 64, 65, 129, 257, 520}, N of {160, 320, 640 | 64, 208 | 72, 330} and K of {1, 2, 3, 5 K tiles} at least once
FP8_SHAPES = [(63, 160, 128), (64, 320, 256), (65, 640, 384), (129, 64, 640), (257, 208, 128), (520, 72, 256), (129, 330, 384),
              (257, 160, 640)]
FP8_EPILOGUES = ["plain", "bias", "bias+residual", "gelu", "geglu"]
FP8_PROBE_SHAPES = [(129, 160, 384), (257, 330, 128)]
FP8_STRIDE_SHAPE = (129, 208, 256)
FP8_STRIDE_CASES = [(8, 0, False), (4, 0, False), (1, 0, False), (0, 4, False), (8, 4, True), (1, 0, True)]   # ldc - width, bias offset, geglu
LNFOLD_TILES = [0, 60, 62, 63, 64, 66, 68, 69, 71, 72]
LNFOLD_SHAPES = [(129, 160, 64), (257, 640, 192), (520, 208, 640)]
LNFOLD_EPILOGUES = ["plain", "bias", "gelu", "geglu"]
# the partial form: N = 208 is the refused shape (no folded tile width divides it); (520, 320, 640) gives it M = 520 and K = 640
LNFOLD_PART_SHAPES = LNFOLD_SHAPES + [(520, 320, 640)]
LNFOLD_PART_WIDTH = 32                                # strip width of the synthetic partials: 2, 6 and 20 strips (> 16: the
#                                                       consumer's loop takes 16 at a time, the second batch has a masked tail)
ROWSTATS_SHAPES = [(5, 8), (129, 64), (257, 192), (130, 640), (67, 2048), (4, 1032)]
PRODUCER_SHAPES = [(129, 160, 64), (257, 640, 192), (333, 200, 64), (257, 128, 192), (333, 640, 64)]
SPLITK_SHAPES = [(129, 64, 1024), (257, 128, 1088), (512, 192, 2048)]
SPLITK_S = [0, 2, 3, 5, 8]
SPLITK_EPILOGUES = ["bias", "residual", "bias+residual"]
QUANT_LN_SHAPES = [(5, 8), (130, 640), (67, 1288)]
LN_EPS = 1e-5


# ---- seeds: one function per family, used by the GPU file and by the CPU simulation alike ------------------------------------------
def fp8_seeds(cfg, i, j):
    """(operands, epilogue inputs) of shape i, epilogue j on tile cfg"""
    return cfg * 1000 + i, cfg * 1000 + i * 10 + j


def fp8_stride_seed(cfg, c):
    return cfg * 1000 + 500 + c


def lnfold_seed(cfg, i, part=False):
    return cfg * 100 + (50 if part else 0) + i


def producer_seed(fallback, i):
    return 100 * fallback + i


def splitk_seed(i, S):
    return 300 + 10 * i + S


LNFOLD_REFUSAL_CASE = (129, 160, 64, 77)            # M, N, K, seed of the alignment cases of ss_gemm_lnfold_part
PRODUCER_CHAIN_CASES = [(257, 640, 192, 200), (129, 128, 64, 201)]      # M, N, K, seed of producer -> folded consumer (160 wide)


def splitk_planned(M, N, K):
    """the split count splitk_plan (ss_gemm.hip) gives the shapes above (2, 2, 4): a hand copy, asserted against the workspace
    size the library reports"""
    base = -(-M // 128) * -(-N // 64)
    s = min(-(-512 // base), (K // 64) // 8, 8)
    kt = K // 64
    while s > 2 and (s - 1) * -(-kt // s) >= kt:
        s -= 1
    return s


def splitk_ranges(K, S):
    """[(k0, k1)] of the S slices: ceil(tiles / S) K tiles of 64 each, the last ranges short or empty"""
    kt = K // 64
    per = -(-kt // S)
    return [(min(i * per, kt) * 64, min((i + 1) * per, kt) * 64) for i in range(S)]


def fp8_inputs(M, N, K, seed):
    """fresh quantised operands: a ~ N(0, 1) rows scaled over two decades, w ~ N(0, 1 / K) -> (a8, sa, w8, sw)"""
    g = torch.Generator().manual_seed(17000 + seed)
    a = torch.randn(M, K, generator=g) * torch.logspace(-1, 1, M)[:, None]
    w = torch.randn(N, K, generator=g) / K ** 0.5
    return quantize_rows_e4m3(a.to(torch.bfloat16)) + quantize_rows_e4m3(w.to(torch.bfloat16))


def lnfold_inputs(M, N, K, dtype, seed):
    """x: N(0.7, 3^2) rows; rows 1 (mod 16) sit at |mean| ~ 9 std, row 2 is constant.  -> (x, wg, colsum fp32, bias_d)"""
    g = torch.Generator().manual_seed(18000 + seed)
    x = torch.randn(M, K, generator=g) * 3.0 + 0.7
    x[1::16] = torch.randn(len(range(1, M, 16)), K, generator=g) * 1.4 + 12.6
    x[2] = 1.75
    wg = ((torch.randn(N, K, generator=g) / K ** 0.5) * (1.0 + 0.1 * torch.randn(K, generator=g))[None, :]).to(dtype)
    bias_d = (torch.randn(N, generator=g) * 0.5).to(dtype)
    return x.to(dtype), wg, wg.float().sum(1).contiguous(), bias_d


def lnfold_parts(x, width=LNFOLD_PART_WIDTH):
    """per-strip (sum, sum of squares) of x's rows as a producer would leave them: fp64 sums rounded to fp32 -> [M, strips, 2]"""
    xs = x.double().view(x.shape[0], x.shape[1] // width, width)
    return torch.stack([xs.sum(2), (xs * xs).sum(2)], 2).float().contiguous()


def producer_inputs(M, N, K, dtype, seed):
    """a, w, bias (+9: |row mean| ~ 9 std of the output), residual"""
    g = torch.Generator().manual_seed(19000 + seed)
    a = torch.randn(M, K, generator=g).to(dtype)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(dtype)
    return a, w, (torch.randn(N, generator=g) * 0.3 + 9.0).to(dtype), torch.randn(M, N, generator=g).to(dtype)


# ---- the decode step as the engine launches it (tests/test_decode_step_gpu.py; simulated in tests/test_kernel_check_cpu.py) ---
# ss_attn_decode_step / ss_attn_decode_kv8_step: attn_decode_kernel / attn_decode_kv8_kernel in their fused, batched mode.
DECODE_STEP_CAP = 640
DECODE_STEP_GAP_ROWS = 16               # poisoned rows between consecutive sequences' planes: cache_stride = (H cap + 16) hd
DECODE_STEP_WORDS = 8                   # int32 state words per sequence; kv_len, pos, done at words 0, 1, 3 (ss_llama.hip's ST_*)
ST_KV_LEN, ST_POS, ST_DONE = 0, 1, 3
DECODE_STEP_POS_AHEAD = 3               # pos = kv_len + 3: the RoPE position is its own word
DECODE_STEP_DONE_KV_LEN = 37            # kv_len of a finished sequence: a row it appended all the same would land on poison
DECODE_STEP_FAMILY = {False: "attn_decode step", True: "attn_decode_kv8 step"}


def decode_step_nsplit(nb, knob=0):
    """decode_nsplit of ss_attn.hip: the splits of a launch over nb sequences under knob attn_decode_nsplit"""
    n = knob if knob > 0 else 16 // max(nb, 1)
    return 4 if n <= 4 else 8 if n <= 8 else 16 if n <= 16 else 32


def decode_step_n_olds(ns, cap=DECODE_STEP_CAP):
    """cached keys before the step: ns - 1, ns, ns + 1 give empty splits and one key per split (the new key makes n_old + 1);
    511, 512, 600 at ns = 4 put the new key into a later 4-keys-per-thread sub-chunk of its split for every NKG * 4 in
    {32, 64, 128}; cap - 1 writes the last row; cap writes nothing and still attends the new key"""
    return sorted({0, 1, ns - 2, ns - 1, ns, ns + 1, 63, 64, 500, 511, 512, 600, cap - 1, cap})


def _decode_step_cases():
    """(nb, knob, ns, n_old per sequence, done per sequence): every n_old of decode_step_n_olds(ns) at nb = 1 under knob 0 (16
    splits), 4 and 32, and again on a live sequence of every nb > 1 (default knob: 8, 8, 4, 4 splits at 2, 3, 4, 8 sequences).
    A batch holds nb - 1 live sequences with unequal n_old and one finished one, whose place moves from batch to batch."""
    cases = []
    for knob in (0, 4, 32):
        ns = decode_step_nsplit(1, knob)
        cases += [(1, knob, ns, (n,), (False,)) for n in decode_step_n_olds(ns)]
    for nb in (2, 3, 4, 8):
        ns = decode_step_nsplit(nb)
        vals, live = decode_step_n_olds(ns), nb - 1
        for i in range(0, len(vals), live):
            chunk = vals[i:i + live]
            chunk += [v for v in vals if v not in chunk][:live - len(chunk)]
            d = (i // live) % nb
            cases.append((nb, 0, ns, tuple(chunk[:d] + [DECODE_STEP_DONE_KV_LEN] + chunk[d:]), tuple(b == d for b in range(nb))))
    return cases


DECODE_STEP_CASES = _decode_step_cases()


def decode_step_selector_cases(cap=DECODE_STEP_CAP):
    """the exact probes: n_old 0, ns - 1, ns, 511, cap - 1 at one sequence, and two batches (8 and 4 splits)"""
    cases = [(1, 0, 16, (n,), (False,)) for n in (0, 15, 16, 511, cap - 1)]
    cases.append((3, 0, 8, (7, DECODE_STEP_DONE_KV_LEN, 8), (False, True, False)))
    cases.append((4, 0, 4, (3, 4, 511, cap - 1), (False,) * 4))
    return cases


def bits(t):
    """the integer view under which tensors are compared bit for bit"""
    t = t.contiguous()
    return t if t.dtype == torch.uint8 else t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def decode_step_pack(qkv, kc, vc, kv_lens, pos, done, dtype, shadow=False, gap_rows=DECODE_STEP_GAP_ROWS):
    """The buffers of one launch, on the CPU, arranged so that a wrong stride or word index lands on garbage: kc / vc
    [nb, H, cap, hd] (rows >= kv_len are poisoned here) flat with gap_rows poisoned rows after every sequence; the state
    [nb, 8] with kv_len, pos, done at words 0, 1, 3 and large garbage elsewhere; shadow: code planes of the same layout (0x7f
    from row kv_len on and in the gaps) and scale planes, one fp32 per row (NaN likewise), rows < kv_len from kv8_ref."""
    import types
    nb, H, cap, hd = kc.shape
    plane = H * cap * hd
    stride = plane + gap_rows * hd
    kc, vc = kc.clone(), vc.clone()
    flats = []
    for pl in (kc, vc):
        for b in range(nb):
            poison_(pl[b][:, kv_lens[b]:])
        f = poison_(torch.empty(nb, stride, dtype=dtype))
        f[:, :plane] = pl.reshape(nb, plane)
        flats.append(f.reshape(-1))
    state = (0x40000000 + 0x00010101 * (1 + torch.arange(nb * DECODE_STEP_WORDS))).to(torch.int32).view(nb, DECODE_STEP_WORDS)
    for b in range(nb):
        state[b, ST_KV_LEN], state[b, ST_POS], state[b, ST_DONE] = kv_lens[b], pos[b], int(done[b])
    inp = types.SimpleNamespace(qkv=qkv, kc=kc, vc=vc, kflat=flats[0], vflat=flats[1], state=state, kv_lens=tuple(kv_lens), pos=tuple(pos),
                                done=tuple(done), dtype=dtype, nb=nb, H=H, cap=cap, hd=hd, plane=plane, cache_stride=stride,
                                shadow=shadow)
    if shadow:
        import kv8_ref
        codes = [torch.full((nb, stride), 0x7f, dtype=torch.uint8) for _ in range(2)]
        scales = [torch.full((nb, stride // hd), float("nan")) for _ in range(2)]
        for i, pl in enumerate((kc, vc)):
            for b in range(nb):
                n = kv_lens[b]
                c, s, _ = kv8_ref.quantize(pl[b][:, :n])
                codes[i][b, :plane].view(H, cap, hd)[:, :n] = c
                scales[i][b, :H * cap].view(H, cap)[:, :n] = s
        inp.kq, inp.vq, inp.ks, inp.vs = [t.reshape(-1) for t in codes + scales]
    return inp


def decode_step_inputs(case, hd, dtype, seed=0, shadow=False, H=DECODE_HEADS, cap=DECODE_STEP_CAP):
    """fresh N(0, 1) operands of one case of DECODE_STEP_CASES -> decode_step_pack"""
    nb, _, _, n_olds, done = case
    g = torch.Generator().manual_seed(21000 + 131 * hd + 17 * sum(n_olds) + nb + seed)
    qkv = torch.randn(nb, 3 * H * hd, generator=g).to(dtype)
    kc = torch.randn(nb, H, cap, hd, generator=g).to(dtype)
    vc = torch.randn(nb, H, cap, hd, generator=g).to(dtype)
    return decode_step_pack(qkv, kc, vc, n_olds, [n + DECODE_STEP_POS_AHEAD for n in n_olds], done, dtype, shadow)


def decode_step_expect(qkv, kc, vc, cos, sin, kv_lens, pos, done, dtype, shadow=False):
    """What one decode step must leave behind, per sequence b (a list of namespaces):
      q, k_new, v_new [H, hd]   the rotated q, the new rotated K row and the V row (rope_exact: bit-exact);
      wrote                      not done[b] and kv_len[b] < cap: the row is stored at kv_len[b] — k_after / v_after [H, cap, hd] are
                                 the planes after the step (that row and nothing else);
      ref, tol [H, 1, hd]        attention_bound over keys [0, kv_len[b]], the new key included (None for a finished sequence).
    shadow: the old keys are the de-quantised shadow (kv8_ref of rows < kv_len, exact in the model dtype), the new key is the
    unquantised rotated row; kq_new, vq_new [H, hd] uint8 and ks_new, vs_new [H] are kv8_ref.quantize of the new rows.
    No constant of its own: attention_bound is derived for fp32 accumulation over operands that are exact in T."""
    import types
    nb, H, cap, hd = kc.shape
    rows = qkv.view(nb, 3, H, hd)
    p = torch.tensor(list(pos))
    q_rot, k_rot = rope_exact(rows[:, 0], cos, sin, p), rope_exact(rows[:, 1], cos, sin, p)
    if shadow:
        import kv8_ref
    out = []
    for b in range(nb):
        n = int(kv_lens[b])
        e = types.SimpleNamespace(q=q_rot[b], k_new=k_rot[b], v_new=rows[b, 2].clone(), wrote=(not done[b]) and n < cap, ref=None, tol=None,
                                  k_after=kc[b].clone(), v_after=vc[b].clone())
        if e.wrote:
            e.k_after[:, n], e.v_after[:, n] = e.k_new, e.v_new
        if shadow:
            e.kq_new, e.ks_new, _ = kv8_ref.quantize(e.k_new)
            e.vq_new, e.vs_new, _ = kv8_ref.quantize(e.v_new)
        if not done[b]:
            k_old, v_old = kc[b][:, :n], vc[b][:, :n]
            if shadow:
                k_old, v_old = kv8_ref.quantize(k_old)[2], kv8_ref.quantize(v_old)[2]
            e.ref, e.tol = attention_bound(e.q[:, None], torch.cat([k_old, e.k_new[:, None]], 1), torch.cat([v_old, e.v_new[:, None]], 1),
                                           1.0 / hd ** 0.5, None, dtype)
        out.append(e)
    return out


def decode_step_failures(inp, exp, got, what):
    """The assertions of the decode-step tests over what a launch (or the simulated kernel) left behind.  got: namespace with out
    [nb, E], written [nb, E] bool (the element no longer holds the output buffer's sentinel), kflat, vflat, state and, for the
    shadow, kq, vq, ks, vs — all on the CPU.  -> [(label, message)], empty when everything holds:
      bound             every output element of a live sequence inside attention_bound (recorded under the family)
      out rows          a live sequence's output row is written completely, a finished one's not at all
      append            row kv_len of every head of both planes bit-equal to the mirror (sequences that store)
      untouched         every other element of both flat buffers, gaps included, bit-identical to before
      state             the state array bit-identical
      shadow append     codes and both scales of the new row bit-equal to kv8_ref of the rotated row
      shadow untouched  every other code and scale bit-identical"""
    H, cap, hd, nb = inp.H, inp.cap, inp.hd, inp.nb
    fails = []
    fam = DECODE_STEP_FAMILY[inp.shadow]
    for b in range(nb):
        wb = "%s seq %d (n_old %d)" % (what, b, inp.kv_lens[b])
        if inp.done[b]:
            if bool(got.written[b].any()):
                fails.append(("out rows", wb + ": the output row of a finished sequence was written"))
            continue
        if not bool(got.written[b].all()):
            fails.append(("out rows", wb + ": %d output elements never written" % int((~got.written[b]).sum())))
        try:
            check(got.out[b].view(H, 1, hd), exp[b].ref, exp[b].tol, wb, family=fam, dtype=inp.dtype)
        except AssertionError as err:
            fails.append(("bound", str(err)))
    planes = [("k", inp.kflat, got.kflat, "k_new", "append", "untouched"), ("v", inp.vflat, got.vflat, "v_new", "append", "untouched")]
    if inp.shadow:
        planes += [("k codes", inp.kq, got.kq, "kq_new", "shadow append", "shadow untouched"),
                   ("v codes", inp.vq, got.vq, "vq_new", "shadow append", "shadow untouched"),
                   ("k scales", inp.ks, got.ks, "ks_new", "shadow append", "shadow untouched"),
                   ("v scales", inp.vs, got.vs, "vs_new", "shadow append", "shadow untouched")]
    for name, before, after, attr, l_app, l_unt in planes:
        width = 1 if "scales" in name else hd
        stride = inp.cache_stride // hd * width
        a, b0 = bits(after).view(nb, stride), bits(before).view(nb, stride)
        appended = torch.zeros(nb, stride, dtype=torch.bool)
        for b in range(nb):
            if not exp[b].wrote:
                continue
            n = inp.kv_lens[b]
            sl = a[b, :H * cap * width].view(H, cap, width)[:, n]
            appended[b, :H * cap * width].view(H, cap, width)[:, n] = True
            want = bits(getattr(exp[b], attr)).view(H, width)
            if not torch.equal(sl, want):
                fails.append((l_app, "%s seq %d: row %d of the %s plane differs from the mirror in %d elements"
                              % (what, b, n, name, int((sl != want).sum()))))
        changed = ((a != b0) & ~appended).nonzero()
        if changed.numel():
            s, i = int(changed[0, 0]), int(changed[0, 1])
            fails.append((l_unt, "%s: %d elements of the %s buffer written outside the new rows, first in sequence %d's stride at "
                          "element %d (head %d, row %d; beyond %d: the gap)" % (what, changed.shape[0], name, s, i, i // (cap * width),
                                                                               i // width % cap, H * cap * width)))
    if not torch.equal(got.state, inp.state):
        fails.append(("state", what + ": the state array changed"))
    return fails


def decode_step_selector_inputs(case, hd, dtype, second=False, shadow=False, H=DECODE_HEADS, cap=DECODE_STEP_CAP):
    """Exact probe of the step (identity RoPE tables keep the vectors exact): old keys and the new key form attention_selector's
    family at kscale = 16, so the LAST key — the new one — takes all the weight and the output is the new V row, bit for bit.
    second: the new K row is zero (score 0), so the largest score sits on key n_old - 1 and the output is v[n_old - 1]: the
    new key does not mask the old ones (needs n_old >= 2: key 0 scores 0 as well).
    shadow: kv8_selector's family with a third digit, key j = 256 a + 16 b + c (a <= 2; b, c <= 15) -> entries 16 a, 16 b, 16 c
    (four significand bits: exact in e4m3 under any power-of-two row scale), q = 128 (256 e0 + 16 e1 + e2): scores
    2048 j / sqrt(hd) again; the old V rows go through kv8_ref first, the new V row does not (it is attended unquantised).
    -> (inp, expected [nb, H * hd] — rows of finished sequences unspecified)"""
    nb, _, _, n_olds, done = case
    E = H * hd
    qkv = torch.zeros(nb, 3, H, hd, dtype=dtype)
    kc, vc = torch.zeros(nb, H, cap, hd, dtype=dtype), torch.zeros(nb, H, cap, hd, dtype=dtype)
    want = torch.zeros(nb, H, hd, dtype=dtype)
    for b, n in enumerate(n_olds):
        assert not second or n >= 2 or done[b]
        if shadow:
            import kv8_ref
            g = torch.Generator().manual_seed(4100 + 7 * n + b)
            j = torch.arange(n + 1)
            q = torch.zeros(H, 1, hd)
            q[..., 0], q[..., 1], q[..., 2] = 128.0 * 256.0, 128.0 * 16.0, 128.0
            k = torch.zeros(H, n + 1, hd)
            k[..., 0], k[..., 1], k[..., 2] = (j // 256).float() * 16.0, (j // 16 % 16).float() * 16.0, (j % 16).float() * 16.0
            q, k, v = q.to(dtype), k.to(dtype), torch.randn(H, n + 1, hd, generator=g).to(dtype)
            assert torch.equal(kv8_ref.quantize(k)[2], k)
            v[:, :n] = kv8_ref.quantize(v[:, :n])[2]
        else:
            q, k, v = attention_selector(1, n + 1, hd, dtype, seed=n + b, H=H, kscale=16.0)
        kc[b, :, :n], vc[b, :, :n] = k[:, :n], v[:, :n]
        qkv[b, 0], qkv[b, 1], qkv[b, 2] = q[:, 0], (torch.zeros_like(k[:, n]) if second else k[:, n]), v[:, n]
        want[b] = v[:, n - 1] if second else v[:, n]
    inp = decode_step_pack(qkv.reshape(nb, 3 * E), kc, vc, n_olds, [0] * nb, done, dtype, shadow)
    return inp, want.reshape(nb, E)
