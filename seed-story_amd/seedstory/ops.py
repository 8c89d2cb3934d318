"""Tensor-level wrappers over the C ABI: each function takes torch CUDA(HIP) tensors, enqueues
the HIP kernel on torch's current stream and returns the output tensor.  torch is plumbing here
(device memory + streams); all arithmetic happens in ``libseedstory_hip.so``."""
import math

import torch

from . import _lib, tune
from ._lib import EPI_BIAS, EPI_GELU, EPI_NONE, EPI_RESIDUAL, EPI_SILU_MUL, check, lib

_DT = {torch.float32: _lib.SS_F32, torch.bfloat16: _lib.SS_BF16, torch.float16: _lib.SS_F16}


def dt(t):
    try:
        return _DT[t.dtype if isinstance(t, torch.Tensor) else t]
    except KeyError:
        raise _lib.SSError("unsupported dtype %s" % (t.dtype if isinstance(t, torch.Tensor) else t))


def stream():
    return torch.cuda.current_stream().cuda_stream


def p(t):
    return None if t is None else t.data_ptr()


def _req(t, name="tensor"):
    if not t.is_cuda:
        raise _lib.SSError("%s must live on the GPU (there is no CPU path)" % name)
    if not t.is_contiguous():
        raise _lib.SSError("%s must be contiguous" % name)
    return t


def _out(out, shape, like, name):
    """The caller's ``out=`` buffer (checked) or a fresh one: every wrapper with an ``out`` argument writes its result there."""
    if out is None:
        return torch.empty(shape, dtype=like.dtype, device=like.device)
    _req(out, name + "(out=)")
    if tuple(out.shape) != tuple(shape) or out.dtype != like.dtype or out.device != like.device:
        raise _lib.SSError("%s(out=): expected %s %s on %s, got %s %s on %s"
                           % (name, tuple(shape), like.dtype, like.device, tuple(out.shape), out.dtype, out.device))
    return out


def rmsnorm(x, w, eps):
    _req(x); _req(w)
    y = torch.empty_like(x)
    cols = x.shape[-1]
    check(lib().ss_rmsnorm(p(x), p(w), p(y), x.numel() // cols, cols, eps, dt(x), stream()), "ss_rmsnorm")
    return y


def layernorm(x, w, b, eps):
    _req(x); _req(w); _req(b)
    y = torch.empty_like(x)
    cols = x.shape[-1]
    check(lib().ss_layernorm(p(x), p(w), p(b), p(y), x.numel() // cols, cols, eps, dt(x), stream()), "ss_layernorm")
    return y


def add_bcast(x, pos):
    """x [B, R, C] + pos [R, C]"""
    _req(x); _req(pos)
    B, R, Cc = x.shape
    y = torch.empty_like(x)
    check(lib().ss_add_bcast(p(x), p(pos), p(y), B, R, Cc, R * Cc, dt(x), stream()), "ss_add_bcast")
    return y


def silu_mul(gu):
    _req(gu)
    rows, two_i = gu.shape
    out = torch.empty(rows, two_i // 2, dtype=gu.dtype, device=gu.device)
    check(lib().ss_silu_mul(p(gu), p(out), rows, two_i // 2, dt(gu), stream()), "ss_silu_mul")
    return out


def gather_rows(table, ids):
    _req(table)
    ids = ids.to(device=table.device, dtype=torch.int32).contiguous()
    out = torch.empty(ids.numel(), table.shape[1], dtype=table.dtype, device=table.device)
    check(lib().ss_gather_rows(p(table), p(ids), p(out), ids.numel(), table.shape[1], dt(table), stream()),
          "ss_gather_rows")
    return out


def scatter_rows_(dst, idx, src):
    _req(dst); _req(src)
    idx = idx.to(device=dst.device, dtype=torch.int32).contiguous()
    check(lib().ss_scatter_rows(p(src), p(idx), p(dst), idx.numel(), dst.shape[-1], dt(dst), stream()),
          "ss_scatter_rows")
    return dst


def im2col_patch(img, patch, kpad):
    _req(img)
    B, _, S, _ = img.shape
    G = S // patch
    out = torch.empty(B * G * G, kpad, dtype=img.dtype, device=img.device)
    check(lib().ss_im2col_patch(p(img), p(out), B, S, patch, kpad, dt(img), stream()), "ss_im2col_patch")
    return out


def l2normalize_dim1(x):
    _req(x)
    B, L, Cc = x.shape
    y = torch.empty_like(x)
    check(lib().ss_l2normalize_dim1(p(x), p(y), B, L, Cc, dt(x), stream()), "ss_l2normalize_dim1")
    return y


def rope_kv_append(qkv, kcache, vcache, cos, sin, n_heads, kv_start, pos_ids=None, pos_start=0):
    """qkv [M, 3*E]; caches [n_heads, cap, hd]; returns rotated q [M, E]."""
    _req(qkv); _req(kcache); _req(vcache)
    M = qkv.shape[0]
    E = qkv.shape[1] // 3
    hd = E // n_heads
    q = torch.empty(M, E, dtype=qkv.dtype, device=qkv.device)
    pid = None if pos_ids is None else pos_ids.to(device=qkv.device, dtype=torch.int32).contiguous()
    check(lib().ss_rope_kv_append(p(qkv), p(q), p(kcache), p(vcache), p(cos), p(sin), p(pid), pos_start, M, n_heads,
                                  hd, kv_start, kcache.shape[1], dt(qkv), stream()), "ss_rope_kv_append")
    return q


def attention(q, k, v, n_heads, scale=None, causal_br=False, out=None):
    """q [B, Lq, E], k/v [B, Lk, E] (heads packed along E) -> [B, Lq, E]."""
    _req(q); _req(k); _req(v)
    B, Lq, E = q.shape
    Lk = k.shape[1]
    hd = E // n_heads
    out = _out(out, q.shape, q, "attention")
    scale = 1.0 / math.sqrt(hd) if scale is None else scale
    kb = 0 if k.shape[0] == 1 and B > 1 else Lk * E
    check(lib().ss_attention(p(q), p(k), p(v), p(out), B, n_heads, Lq, Lk, hd, Lq * E, hd, E, kb, hd, E, kb, hd, E,
                             Lq * E, hd, E, scale, int(causal_br), dt(q), stream()), "ss_attention")
    return out


def attention_cache(q, kcache, vcache, kv_len, causal_br=True, out=None):
    """q [M, n_heads*hd] against cache planes [n_heads, cap, hd] (first kv_len slots)."""
    _req(q); _req(kcache)
    M, E = q.shape
    n_heads, cap, hd = kcache.shape
    out = _out(out, q.shape, q, "attention_cache")
    check(lib().ss_attention(p(q), p(kcache), p(vcache), p(out), 1, n_heads, M, kv_len, hd, 0, hd, E, 0, cap * hd, hd,
                             0, cap * hd, hd, 0, hd, E, 1.0 / math.sqrt(hd), int(causal_br), dt(q), stream()),
          "ss_attention")
    return out


def attention_cache_slots(q, kcache, vcache, kv_lens, causal_br=True, out=None):
    """Stacked slots: q [S * M, n_heads*hd] (M rows per slot) against caches [S, n_heads, cap, hd]; slot b attends to its
    first kv_lens[b] entries (ss_attention_ragged: one launch for the S slots)."""
    import ctypes
    _req(q); _req(kcache)
    S, n_heads, cap, hd = kcache.shape
    E = n_heads * hd
    M = q.shape[0] // S
    out = _out(out, q.shape, q, "attention_cache_slots")
    lens = (ctypes.c_int32 * S)(*[int(x) for x in kv_lens])
    check(lib().ss_attention_ragged(p(q), p(kcache), p(vcache), p(out), S, n_heads, M, ctypes.cast(lens, ctypes.c_void_p), hd,
                                    M * E, hd, E, n_heads * cap * hd, cap * hd, hd, n_heads * cap * hd, cap * hd, hd, M * E, hd, E,
                                    1.0 / math.sqrt(hd), int(causal_br), dt(q), stream()), "ss_attention_ragged")
    return out


def attn_decode(q, kcache, vcache, kv_len_dev, out=None):
    _req(q); _req(kcache)
    n_heads, cap, hd = kcache.shape
    ws = torch.empty(lib().ss_attn_decode_workspace_bytes(n_heads, hd), dtype=torch.uint8, device=q.device)
    out = _out(out, q.shape, q, "attn_decode")
    check(lib().ss_attn_decode(p(q), p(kcache), p(vcache), p(out), p(ws), p(kv_len_dev), n_heads, hd, cap, dt(q),
                               stream()), "ss_attn_decode")
    return out


def attn_decode_spec(qkv, kcache, vcache, cos, sin, kv_len_dev, pos_dev, n_active_dev, out=None):
    """Decode attention of one speculative step (``ss_attn_decode_spec``): ``qkv`` [R, 3*E] pre-RoPE rows (R <= 8) of ONE slot
    whose cache planes [n_heads, cap, hd] hold ``kv_len_dev[0]`` keys; row r sits at RoPE position ``pos_dev[0] + r`` and
    attends keys [0, L + r].  The first ``n_active_dev[0]`` rows are active: their rotated K / V rows are stored at cache rows
    L .. L + A - 1 and their outputs written to ``out`` [R, E]; everything else is left as it is.  The three scalars are
    int32 device tensors."""
    _req(qkv, "qkv"); _req(kcache, "kcache"); _req(vcache, "vcache"); _req(cos, "cos"); _req(sin, "sin")
    for t, name in ((kv_len_dev, "kv_len_dev"), (pos_dev, "pos_dev"), (n_active_dev, "n_active_dev")):
        _req(t, name)
        if t.dtype != torch.int32 or t.numel() < 1:
            raise _lib.SSError("%s must be an int32 device tensor" % name)
    n_heads, cap, hd = kcache.shape
    R = qkv.shape[0]
    if qkv.dim() != 2 or qkv.shape[1] != 3 * n_heads * hd or tuple(vcache.shape) != tuple(kcache.shape):
        raise _lib.SSError("attn_decode_spec: qkv %s does not fit cache planes %s" % (tuple(qkv.shape), tuple(kcache.shape)))
    if not 1 <= R <= _lib.SPEC_MAX_ROWS:
        raise _lib.SSError("attn_decode_spec: %d rows outside [1, %d]" % (R, _lib.SPEC_MAX_ROWS))
    ws = torch.empty(R * lib().ss_attn_decode_workspace_bytes(n_heads, hd), dtype=torch.uint8, device=qkv.device)
    out = _out(out, (R, n_heads * hd), qkv, "attn_decode_spec")
    check(lib().ss_attn_decode_spec(p(qkv), p(kcache), p(vcache), p(cos), p(sin), p(out), p(ws), p(kv_len_dev), p(pos_dev),
                                    p(n_active_dev), R, n_heads, hd, cap, dt(qkv), stream()), "ss_attn_decode_spec")
    return out


def _decode_step_args(name, qkv, kcache, vcache, cos, sin, state, n_heads, cache_cap, cache_stride, words, shadow=()):
    """shared by attn_decode_step / attn_decode_kv8_step: the checks that keep every sequence inside the caller's buffers
    (the argument rules themselves are the C entry point's) -> (nb, hd, cache_stride, state_stride)"""
    for t, n in ((qkv, "qkv"), (kcache, "kcache"), (vcache, "vcache"), (cos, "cos"), (sin, "sin"), (state, "state")) + tuple(shadow):
        _req(t, n)
    if qkv.dim() != 2 or qkv.shape[1] % (3 * n_heads) or state.dtype != torch.int32 or state.dim() != 2 or state.shape[0] != qkv.shape[0]:
        raise _lib.SSError("%s: qkv [nb, 3 * n_heads * hd] and an int32 state [nb, words] expected, got %s and %s %s"
                           % (name, tuple(qkv.shape), state.dtype, tuple(state.shape)))
    if max(words) >= state.shape[1]:
        raise _lib.SSError("%s: state word %d of %d" % (name, max(words), state.shape[1]))
    nb, hd = qkv.shape[0], qkv.shape[1] // (3 * n_heads)
    plane = n_heads * cache_cap * hd
    cache_stride = plane if cache_stride is None else int(cache_stride)
    need = max(nb - 1, 0) * max(cache_stride, 0) + plane
    for t, n, have in ((kcache, "kcache", kcache.numel()), (vcache, "vcache", vcache.numel())) + \
            tuple((t, n, t.numel() * (hd if t.dtype == torch.float32 else 1)) for t, n in shadow):
        if have < need:
            raise _lib.SSError("%s: %s holds %d elements, %d sequences %d apart need %d" % (name, n, have, nb, cache_stride, need))
    return nb, hd, cache_stride, state.shape[1]


def attn_decode_step(qkv, kcache, vcache, cos, sin, state, n_heads, cache_cap, cache_stride=None, kv_len_word=0, pos_word=1,
                     done_word=-1, out=None):
    """The attention of one decode token as the engine launches it (``ss_attn_decode_step``): ``qkv`` [nb, 3*E] pre-RoPE rows of
    nb <= 8 sequences; ``kcache`` / ``vcache`` any contiguous tensors that hold sequence b's planes [n_heads, cache_cap, hd] at
    element ``b * cache_stride`` (default: back to back); ``state`` int32 [nb, words] on the device with the cached key count,
    the RoPE position and (``done_word`` >= 0) the finished flag of sequence b in row b.  Rotates q / k, stores the new K / V
    row at row kv_len of every live sequence's planes (in place) and returns the attention over keys [0, kv_len] as ``out``
    [nb, E]; rows of finished sequences are left as they are."""
    nb, hd, cache_stride, words = _decode_step_args("attn_decode_step", qkv, kcache, vcache, cos, sin, state, n_heads, cache_cap,
                                                    cache_stride, (kv_len_word, pos_word, done_word))
    ws = torch.empty(max(nb, 1) * lib().ss_attn_decode_workspace_bytes(n_heads, max(hd, 1)), dtype=torch.uint8, device=qkv.device)
    out = _out(out, (nb, n_heads * hd), qkv, "attn_decode_step")
    check(lib().ss_attn_decode_step(p(qkv), p(kcache), p(vcache), p(cos), p(sin), p(out), p(ws), p(state), int(kv_len_word),
                                    int(pos_word), int(done_word), words, nb, n_heads, hd, cache_cap, cache_stride, dt(qkv), stream()),
          "ss_attn_decode_step")
    return out


def attn_decode_kv8_step(qkv, kcache, vcache, k_codes, v_codes, k_scale, v_scale, cos, sin, state, n_heads, cache_cap,
                         cache_stride=None, kv_len_word=0, pos_word=1, done_word=-1, out=None):
    """``attn_decode_step`` over the e4m3 shadow (``ss_attn_decode_kv8_step``): old keys come from ``k_codes`` / ``v_codes``
    (uint8, laid out like the planes) and ``k_scale`` / ``v_scale`` (fp32, one per row: sequence b at ``b * cache_stride / hd``),
    the new key is attended unquantised; the new row is stored into the 16-bit planes and, quantised, into the shadow."""
    shadow = ((k_codes, "k_codes"), (v_codes, "v_codes"), (k_scale, "k_scale"), (v_scale, "v_scale"))
    nb, hd, cache_stride, words = _decode_step_args("attn_decode_kv8_step", qkv, kcache, vcache, cos, sin, state, n_heads, cache_cap,
                                                    cache_stride, (kv_len_word, pos_word, done_word), shadow)
    if k_codes.dtype != torch.uint8 or v_codes.dtype != torch.uint8 or k_scale.dtype != torch.float32 or v_scale.dtype != torch.float32:
        raise _lib.SSError("attn_decode_kv8_step: uint8 code planes and fp32 scale planes expected")
    ws = torch.empty(max(nb, 1) * lib().ss_attn_decode_workspace_bytes(n_heads, max(hd, 1)), dtype=torch.uint8, device=qkv.device)
    out = _out(out, (nb, n_heads * hd), qkv, "attn_decode_kv8_step")
    check(lib().ss_attn_decode_kv8_step(p(qkv), p(kcache), p(vcache), p(k_codes), p(v_codes), p(k_scale), p(v_scale), p(cos), p(sin),
                                        p(out), p(ws), p(state), int(kv_len_word), int(pos_word), int(done_word), words, nb, n_heads,
                                        hd, cache_cap, cache_stride, dt(qkv), stream()), "ss_attn_decode_kv8_step")
    return out


def spec_draft(history, max_ngram=2, num_tokens=3, stop_ids=()):
    """The prompt-lookup draft (``ss_spec_draft``): transformers' ``PromptLookupCandidateGenerator.get_candidates`` on the int32
    device tensor ``history`` — n-gram sizes from ``min(max_ngram, len - 1)`` down to 1, the leftmost match with a non-empty
    continuation, at most ``num_tokens`` (<= 7) ids, cut in front of the first of ``stop_ids`` (at most two).  Returns the
    drafted ids as a list (empty: no draft)."""
    import ctypes as C
    _req(history, "history")
    if history.dtype != torch.int32 or history.dim() != 1:
        raise _lib.SSError("history must be a 1-D int32 device tensor")
    stops = [int(t) for t in stop_ids]
    arr = (C.c_int32 * max(1, len(stops)))(*stops)
    out = torch.full((_lib.SPEC_MAX_ROWS,), -1, dtype=torch.int32, device=history.device)
    cnt = torch.zeros(1, dtype=torch.int32, device=history.device)
    check(lib().ss_spec_draft(p(history), history.numel(), int(max_ngram), int(num_tokens), len(stops), arr, p(out), p(cnt),
                              stream()), "ss_spec_draft")
    return out[:int(cnt.item())].tolist()


def kv_quantize_fp8(k, v, lo=0, hi=None, out=None):
    """e4m3 codes + power-of-two fp32 scales of rows [lo, hi) of one layer's cache planes k, v [n_heads, cap, hd]
    (ss_kv_quantize_fp8; the definition is in include/seedstory_hip.h).  Returns ``(k_codes, v_codes, k_scale, v_scale)``:
    uint8 [n_heads, cap, hd] and fp32 [n_heads, cap]; ``out`` = such a tuple to write into (rows outside [lo, hi) are left)."""
    _req(k); _req(v)
    n_heads, cap, hd = k.shape
    hi = cap if hi is None else hi
    if out is None:
        out = tuple(torch.zeros(k.shape, dtype=torch.uint8, device=k.device) for _ in range(2)) + \
              tuple(torch.ones(n_heads, cap, dtype=torch.float32, device=k.device) for _ in range(2))
    for t in out:
        _req(t)
    check(lib().ss_kv_quantize_fp8(p(k), p(v), p(out[0]), p(out[1]), p(out[2]), p(out[3]), n_heads, cap, hd, int(lo), int(hi), dt(k),
                                   stream()), "ss_kv_quantize_fp8")
    return out


def attn_decode_kv8(q, k_codes, v_codes, k_scale, v_scale, kv_len_dev, out=None):
    """``attn_decode`` over an e4m3 shadow: codes uint8 [n_heads, cap, hd], scales fp32 [n_heads, cap] (ss_attn_decode_kv8)."""
    _req(q); _req(k_codes); _req(v_codes); _req(k_scale); _req(v_scale)
    n_heads, cap, hd = k_codes.shape
    ws = torch.empty(lib().ss_attn_decode_workspace_bytes(n_heads, hd), dtype=torch.uint8, device=q.device)
    out = _out(out, q.shape, q, "attn_decode_kv8")
    check(lib().ss_attn_decode_kv8(p(q), p(k_codes), p(v_codes), p(k_scale), p(v_scale), p(out), p(ws), p(kv_len_dev), n_heads, hd, cap,
                                   dt(q), stream()), "ss_attn_decode_kv8")
    return out


def attn_scores(q, k, out, row_calls=False):
    """Attention map of one head, the reference's ``output_attentions`` values (ss_attn_scores): q [M, hd] rows of one head
    (post-RoPE), k [kv, hd] one head's plane of the KV cache, out [M, >= kv] in the same dtype — any of them may be a strided
    view with unit inner stride.  Writes ``out[:, :kv]`` in place (``row_calls``: each row only up to its own key, the rest is
    left as the caller filled it) and returns ``out``."""
    for t, name in ((q, "q"), (k, "k"), (out, "out")):
        if not t.is_cuda:
            raise _lib.SSError("%s must live on the GPU (there is no CPU path)" % name)
        if t.dim() != 2 or t.stride(1) != 1 or t.dtype != q.dtype:
            raise _lib.SSError("%s must be a 2-D view with unit inner stride, in q's dtype" % name)
    M, hd = q.shape
    kv = k.shape[0]
    if k.shape[1] != hd or out.shape[0] != M or out.shape[1] < kv:
        raise _lib.SSError("attn_scores: q %s, k %s, out %s do not fit" % (tuple(q.shape), tuple(k.shape), tuple(out.shape)))
    check(lib().ss_attn_scores(p(q), q.stride(0), p(k), k.stride(0), p(out), out.stride(0), M, kv, hd, 1 if row_calls else 0,
                               dt(q), stream()), "ss_attn_scores")
    return out


def gemm(a, w, bias=None, residual=None, gelu=False, out=None, rowstat=None, rowpart=None):
    """a [M, K] @ w[N, K]^T (+bias)(+gelu)(+residual) -> [M, N].  ``rowstat`` (fp64 [M, 2], zeroed by the caller): the
    epilogue also accumulates (sum, sum of squares) of every stored output row into it (ss_gemm_rowstat)."""
    _req(a); _req(w)
    M, K = a.shape
    N = w.shape[0]
    out = _out(out, (M, N), a, "gemm")
    epi = (EPI_BIAS if bias is not None else 0) | (EPI_GELU if gelu else 0) | (EPI_RESIDUAL if residual is not None else 0)
    tune.ensure_gemm(M, N, K, dt(a), epi, a.device)
    if rowstat is not None:
        assert rowstat.dtype == torch.float64 and rowstat.is_contiguous() and rowstat.numel() == 2 * M
        check(lib().ss_gemm_rowstat(p(a), p(w), p(out), M, N, K, K, w.stride(0), N, p(bias), p(residual), N, epi, p(rowstat),
                                    dt(a), stream()), "ss_gemm_rowstat")
        return out
    if rowpart is not None:      # [M, strips, 2] fp32: per-strip (sum, sum of squares) of the stored rows, no atomics
        assert rowpart.dtype == torch.float32 and rowpart.is_contiguous() and rowpart.shape[0] == M
        if rowpart.shape[1] != rowpart_strips(M, N, K, a.dtype):
            raise _lib.SSError("gemm(rowpart=): buffer has %d strips, this shape's tile writes %d"
                               % (rowpart.shape[1], rowpart_strips(M, N, K, a.dtype)))
        check(lib().ss_gemm_rowpart(p(a), p(w), p(out), M, N, K, K, w.stride(0), N, p(bias), p(residual), N, epi, p(rowpart),
                                    dt(a), stream()), "ss_gemm_rowpart")
        return out
    check(lib().ss_gemm(p(a), p(w), p(out), M, N, K, K, w.stride(0), N, p(bias), p(residual), N, epi, dt(a), stream()),
          "ss_gemm")
    return out


def gemm_splitk(a, w, bias=None, residual=None, out=None):
    """Small-M weight-streaming GEMM (ss_gemm_splitk): a [M, K] @ w[N, K]^T for 128 < M <= 512; falls back to ss_gemm."""
    _req(a); _req(w)
    M, K = a.shape
    N = w.shape[0]
    out = _out(out, (M, N), a, "gemm_splitk")
    nbytes = lib().ss_gemm_splitk_workspace_bytes(M, N, K)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=a.device)
    check(lib().ss_gemm_splitk(p(a), p(w), p(out), M, N, K, p(bias), p(residual), p(ws), nbytes, dt(a), stream()), "ss_gemm_splitk")
    return out


def gemm_geglu(a, w_pairs, bias_pairs, out=None):
    """a [M, K] @ w_pairs[2D, K]^T with rows interleaved (value_i, gate_i) -> [M, D] = value * gelu(gate)."""
    _req(a); _req(w_pairs)
    M, K = a.shape
    N = w_pairs.shape[0]
    out = _out(out, (M, N // 2), a, "gemm_geglu")
    tune.ensure_gemm(M, N, K, dt(a), _lib.EPI_GEGLU_PAIR, a.device)
    check(lib().ss_gemm(p(a), p(w_pairs), p(out), M, N, K, K, K, N // 2, p(bias_pairs), None, 0,
                        _lib.EPI_BIAS | _lib.EPI_GEGLU_PAIR, dt(a), stream()), "ss_gemm(geglu)")
    return out


def rowstats(x, eps):
    """Per-row LayerNorm statistics for `gemm_lnfold`: (rstd [M], -mean * rstd [M]) fp32."""
    _req(x)
    M, K = x.shape
    st = torch.empty(2, M, dtype=torch.float32, device=x.device)
    check(lib().ss_rowstats(p(x), x.stride(0), M, K, float(eps), p(st[0]), p(st[1]), dt(x), stream()), "ss_rowstats")
    return st[0], st[1]


def gemm_lnfold(x, wg, rstd, shift, colsum, bias_d=None, gelu=False, geglu=False, out=None):
    """LN(x) @ W^T + b with the LayerNorm folded: x raw rows, wg = gamma-scaled weight, colsum = wg.sum(1) fp32, bias_d = d."""
    _req(x); _req(wg)
    M, K = x.shape
    N = wg.shape[0]
    No = N // 2 if geglu else N
    out = _out(out, (M, No), x, "gemm_lnfold")
    epi = (EPI_BIAS if bias_d is not None else 0) | (EPI_GELU if gelu else 0) | (_lib.EPI_GEGLU_PAIR if geglu else 0)
    tune.ensure_gemm(M, N, K, dt(x), epi, x.device)
    check(lib().ss_gemm_lnfold(p(x), p(wg), p(out), M, N, K, No, p(rstd), p(shift), p(colsum), p(bias_d), epi, dt(x), stream()),
          "ss_gemm_lnfold")
    return out


def rowpart_strips(M, N, K, dtype):
    """Number of (sum, sum of squares) partials per row that ``gemm(..., rowpart=)`` writes for this shape (0: not eligible).
    The answer depends on the tile the table holds for the shape, so the shape is tuned FIRST (a first forward on a
    shape absent from the table used to size the strip buffer from the closed-form tile and then re-tune inside `gemm`).  It is
    tuned without GELU / GEGLU: a statistics producer feeds a LayerNorm, GEGLU is refused by ss_gemm_rowpart, and no producer on
    the path applies GELU (the former `epi` argument had no caller and is gone)."""
    tune.ensure_gemm(M, N, K, dt(dtype), 0, None)
    return int(lib().ss_gemm_rowpart_strips(M, N, K, dt(dtype)))


def gemm_lnfold_part(x, wg, rowpart, width, eps, colsum, bias_d=None, gelu=False, geglu=False, out=None):
    """`gemm_lnfold` fed by the producer's per-strip partials ``rowpart`` [M, strips, 2]: the row statistics are formed in the
    GEMM's own epilogue (no finalize launch)."""
    _req(x); _req(wg); _req(rowpart)
    M, K = x.shape
    N = wg.shape[0]
    No = N // 2 if geglu else N
    out = _out(out, (M, No), x, "gemm_lnfold_part")
    epi = (EPI_BIAS if bias_d is not None else 0) | (EPI_GELU if gelu else 0) | (_lib.EPI_GEGLU_PAIR if geglu else 0)
    tune.ensure_gemm(M, N, K, dt(x), epi, x.device)
    check(lib().ss_gemm_lnfold_part(p(x), p(wg), p(out), M, N, K, No, p(rowpart), rowpart.shape[1], int(width), float(eps),
                                    p(colsum), p(bias_d), epi, dt(x), stream()), "ss_gemm_lnfold_part")
    return out


def rowstat_finalize(rowstat, width, eps, out=None):
    """(sum, sum of squares) accumulated by ``gemm(..., rowstat=)`` -> (rstd [M], -mean * rstd [M]) fp32 for
    `gemm_lnfold`; ``rowstat`` is re-zeroed for its next producer."""
    M = rowstat.shape[0]
    st = torch.empty(2, M, dtype=torch.float32, device=rowstat.device) if out is None else out
    check(lib().ss_rowstat_finalize(p(rowstat), M, int(width), float(eps), p(st[0]), p(st[1]), stream()), "ss_rowstat_finalize")
    return st[0], st[1]


def quantize_rows_fp8(x, ln=None):
    """x [M, K] (bf16 / fp16) -> (q uint8 [M, K] holding OCP e4m3 bytes, scale fp32 [M]); ``ln`` = (gamma, beta, eps)
    fuses a LayerNorm in front (the normalised bf16 tensor is never written)."""
    _req(x)
    M, K = x.shape
    q = torch.empty(M, K, dtype=torch.uint8, device=x.device)
    sc = torch.empty(M, dtype=torch.float32, device=x.device)
    g, b, eps = ln if ln is not None else (None, None, 0.0)
    check(lib().ss_quantize_rows_fp8(p(x), x.stride(0), M, K, p(q), p(sc), p(g), p(b), float(eps), dt(x), stream()),
          "ss_quantize_rows_fp8")
    return q, sc


def gemm_fp8(a8, sa, w8, sw, bias=None, residual=None, gelu=False, geglu=False, out=None):
    """(a8 * sa[:, None]) @ (w8 * sw[:, None])^T (+bias)(+gelu | geglu pairs)(+residual) -> bf16 [M, N (N/2 for geglu)]."""
    M, K = a8.shape
    N = w8.shape[0]
    No = N // 2 if geglu else N
    if out is None:
        out = torch.empty(M, No, dtype=torch.bfloat16, device=a8.device)
    epi = (EPI_BIAS if bias is not None else 0) | (EPI_GELU if gelu else 0) | (EPI_RESIDUAL if residual is not None else 0) | \
        (_lib.EPI_GEGLU_PAIR if geglu else 0)
    check(lib().ss_gemm_fp8(p(a8), p(sa), p(w8), p(sw), p(out), M, N, K, No, p(bias), p(residual), No, epi, stream()), "ss_gemm_fp8")
    return out


def gemv(w, x, norm_w=None, eps=0.0, bias=None, residual=None, silu_mul=False, out=None):
    _req(w); _req(x)
    N, K = w.shape
    if silu_mul:
        N //= 2
    y = _out(out, (N,), x, "gemv")
    epi = (EPI_BIAS if bias is not None else 0) | (EPI_RESIDUAL if residual is not None else 0) | \
          (EPI_SILU_MUL if silu_mul else 0)
    check(lib().ss_gemv(p(w), p(x), p(y), N, K, p(norm_w), eps, p(bias), p(residual), epi, dt(x), stream()), "ss_gemv")
    return y


def gemv_batched(w, x, norm_w=None, eps=0.0, bias=None, residual=None, silu_mul=False, out=None):
    """x [nb, K] (nb <= 4) -> y [nb, N]: one sweep of W for all rows."""
    _req(w); _req(x)
    N, K = w.shape
    if silu_mul:
        N //= 2
    nb = x.shape[0]
    y = _out(out, (nb, N), x, "gemv_batched")
    epi = (EPI_BIAS if bias is not None else 0) | (EPI_RESIDUAL if residual is not None else 0) | \
          (EPI_SILU_MUL if silu_mul else 0)
    check(lib().ss_gemv_batched(p(w), p(x), p(y), N, K, nb, p(norm_w), eps, p(bias), p(residual), epi, dt(x),
                                stream()), "ss_gemv_batched")
    return y


def gemv_w8(wq, w_scale, x, norm_w=None, eps=0.0, bias=None, residual=None, silu_mul=False, out=None):
    """``gemv_batched`` over fp8 weights: wq uint8 [N, K] of OCP e4m3fn codes ([2N, K] = [gate; up] with ``silu_mul``), w_scale
    fp32 with one entry per row of wq; x [nb, K] (nb <= 16) or [K] in bf16 / fp16 -> y [nb, N] or [N] in x's dtype:
    ``epilogue(w_scale[n] * sum_k dec(wq[n, k]) * x[b, k])``.  K % 16 == 0 and K <= 4096, or K == 11008."""
    _req(wq); _req(x); _req(w_scale)
    if wq.dtype != torch.uint8 or w_scale.dtype != torch.float32 or w_scale.numel() != wq.shape[0]:
        raise _lib.SSError("gemv_w8: wq must be uint8 [N, K] and w_scale fp32 [N]")
    N, K = wq.shape
    if silu_mul:
        N //= 2
    one = x.dim() == 1
    nb = 1 if one else x.shape[0]
    y = _out(out, (N,) if one else (nb, N), x, "gemv_w8")
    epi = (EPI_BIAS if bias is not None else 0) | (EPI_RESIDUAL if residual is not None else 0) | \
          (EPI_SILU_MUL if silu_mul else 0)
    check(lib().ss_gemv_w8(p(wq), p(w_scale), p(x), p(y), N, K, nb, p(norm_w), eps, p(bias), p(residual), epi, dt(x), stream()),
          "ss_gemv_w8")
    return y


def quantize_weight_rows_fp8(w):
    """w [N, K] (bf16 / fp16 on the GPU) -> (q uint8 [N, K] of OCP e4m3fn codes, scale fp32 [N] = amax(row) / 448) for
    ``gemv_w8`` / ``LlamaEngine.set_decode_fp8``: ``scale[n] * dec(q[n])`` is w[n] rounded to e4m3 on the row's own grid.  An
    all-zero row gets scale 0 and codes 0 (``ss_quantize_rows_fp8`` does that itself), so its output is 0."""
    return quantize_rows_fp8(w.contiguous())


def gemv_mx4(codes, scales, x, norm_w=None, eps=0.0, bias=None, residual=None, silu_mul=False, out=None):
    """``gemv_batched`` over MXFP4 weights: codes uint8 [N, K / 2] (two OCP e2m1 codes per byte, k = 2j in bits 0-3 of byte j),
    scales uint8 [N, K / 32] (e8m0: 32 consecutive k times ``2^(byte - 127)``); [2N, ...] = [gate; up] with ``silu_mul``.
    x [nb, K] (nb <= 16) or [K] in bf16 / fp16 -> y [nb, N] or [N] in x's dtype:
    ``epilogue(sum_k dec(codes[n, k]) * 2^(scales[n, k // 32] - 127) * x[b, k])``.  K % 32 == 0 and K <= 4096, or K == 11008."""
    _req(codes); _req(x); _req(scales)
    if (codes.dtype != torch.uint8 or scales.dtype != torch.uint8 or codes.dim() != 2 or scales.dim() != 2
            or scales.shape[0] != codes.shape[0] or scales.shape[1] * 16 != codes.shape[1]):
        raise _lib.SSError("gemv_mx4: codes must be uint8 [N, K / 2] and scales uint8 [N, K / 32]")
    N, K = codes.shape[0], codes.shape[1] * 2
    if silu_mul:
        N //= 2
    one = x.dim() == 1
    nb = 1 if one else x.shape[0]
    y = _out(out, (N,) if one else (nb, N), x, "gemv_mx4")
    epi = (EPI_BIAS if bias is not None else 0) | (EPI_RESIDUAL if residual is not None else 0) | \
          (EPI_SILU_MUL if silu_mul else 0)
    check(lib().ss_gemv_mx4(p(codes), p(scales), p(x), p(y), N, K, nb, p(norm_w), eps, p(bias), p(residual), epi, dt(x), stream()),
          "ss_gemv_mx4")
    return y


def quantize_weight_rows_mxfp4(w):
    """w [N, K] (bf16 / fp16 on the GPU, K % 32 == 0) -> (codes uint8 [N, K / 2], scales uint8 [N, K / 32]) in the MXFP4 format
    of ``gemv_mx4`` / ``LlamaEngine.set_decode_mxfp4``: per block of 32 k the smallest power of two 2^X (X clamped to
    [-13, 13]) with ``amax / 2^X <= 6``, codes rounded to nearest on the e2m1 grid with ties to even (the bit-exact definition
    is in include/seedstory_hip.h).  An all-zero block gets X = -13 and codes 0."""
    _req(w)
    w = w.contiguous()
    N, K = w.shape
    codes = torch.empty(N, K // 2, dtype=torch.uint8, device=w.device)
    scales = torch.empty(N, max(K // 32, 1), dtype=torch.uint8, device=w.device)[:, :K // 32]
    check(lib().ss_quantize_rows_mxfp4(p(w), w.stride(0), N, K, p(codes), p(scales), dt(w), stream()), "ss_quantize_rows_mxfp4")
    return codes, scales


def imgproc_argmax(logits, last_id, img_ids):
    """In-place processor + argmax; returns an int32 device scalar tensor."""
    _req(logits)
    dev = logits.device
    last = torch.tensor([last_id], dtype=torch.int32, device=dev)
    ids = torch.as_tensor(list(img_ids), dtype=torch.int32, device=dev)
    tok = torch.zeros(1, dtype=torch.int32, device=dev)
    check(lib().ss_imgproc_argmax(p(logits), logits.numel(), p(last), p(ids), ids.numel(), p(tok), dt(logits),
                                  stream()), "ss_imgproc_argmax")
    return tok


def sampling_struct(temperature=1.0, top_k=0, top_p=1.0, seed=0):
    """The C ABI's ``ss_sampling``.  Ranges are checked by the library (``SSError``); only what ctypes would mangle silently
    is checked here."""
    if int(top_k) != top_k or not -2 ** 31 <= int(top_k) < 2 ** 31:
        raise _lib.SSError("top_k must be an integer, not %r" % (top_k,))
    return _lib.Sampling(float(temperature), float(top_p), int(top_k), int(seed) & (2 ** 64 - 1))


def sample_logits(logits, temperature=1.0, top_k=0, top_p=1.0, seed=0, u=None, draw0=0, last_ids=None, img_ids=None,
                  return_n_kept=False):
    """One token per row of ``logits`` [rows, vocab] (or [vocab]; rows may be strided, unit stride inside a row) by the
    engine's sampler: processor edit (only with ``last_ids`` [rows] AND ``img_ids``; in place, like ``imgproc_argmax``) ->
    temperature -> top-k (0 = off) -> top-p -> one draw.  ``u`` float32 [rows] supplies the uniforms; None draws Philox4x32-10
    with key ``seed`` and counter (``draw0``, row).  Returns int32 [rows] tokens (and the kept-set sizes with
    ``return_n_kept``).  The definition is in include/seedstory_hip.h (``ss_sample_logits``)."""
    if not logits.is_cuda:
        raise _lib.SSError("logits must live on the GPU (there is no CPU path)")
    lg = logits if logits.dim() == 2 else logits.view(1, -1)
    if lg.dim() != 2 or (lg.shape[1] > 1 and lg.stride(1) != 1) or (lg.shape[0] > 1 and lg.stride(0) < lg.shape[1]):
        raise _lib.SSError("logits must be [rows, vocab] with unit stride inside a row")
    rows, vocab = lg.shape
    dev = lg.device
    sp = sampling_struct(temperature, top_k, top_p, seed)
    if u is not None:
        u = _req(torch.as_tensor(u, dtype=torch.float32, device=dev).reshape(-1), "u")
        if u.numel() != rows:
            raise _lib.SSError("u must hold one value per row (%d), not %d" % (rows, u.numel()))
    last = ids = None
    if last_ids is not None and img_ids is not None:
        last = torch.as_tensor(last_ids, dtype=torch.int32, device=dev).reshape(-1).contiguous()
        if last.numel() != rows:
            raise _lib.SSError("last_ids must hold one id per row (%d), not %d" % (rows, last.numel()))
        ids = torch.as_tensor(list(img_ids), dtype=torch.int32, device=dev)
    tok = torch.zeros(rows, dtype=torch.int32, device=dev)
    kept = torch.zeros(rows, dtype=torch.int32, device=dev) if return_n_kept else None
    import ctypes as C
    check(lib().ss_sample_logits(p(lg), rows, vocab, lg.stride(0) if rows > 1 else vocab, C.byref(sp), p(u), int(draw0) & 0xFFFFFFFF,
                                 p(last), p(ids), 0 if ids is None else ids.numel(), p(tok), p(kept), dt(lg), stream()),
          "ss_sample_logits")
    return (tok, kept) if return_n_kept else tok


def token_logprobs(logits, ids, sampling=None, top_n=0):
    """Log-probability of ``ids`` [rows] on the rows of ``logits`` [rows, vocab] (or [vocab]; rows may be strided, unit stride
    inside a row), which are only read.  ``sampling=None``: the log-softmax at temperature 1 over the whole vocabulary
    (``model_logprob``); ``sampling`` = a dict of ``temperature`` / ``top_k`` / ``top_p``: the sampler's renormalised
    ``log(w / Z_P)``, -inf outside its kept set.  Returns float32 [rows]; with ``top_n`` > 0 (at most 8) the tuple
    (logprobs, top_ids int32 [rows, top_n], top_logprobs float32 [rows, top_n]) — the largest entries with their log-softmax
    values, descending, ties by ascending id, -1 / -inf where fewer carry mass.  The definition is in
    include/seedstory_hip.h (``ss_token_logprobs``)."""
    if not logits.is_cuda:
        raise _lib.SSError("logits must live on the GPU (there is no CPU path)")
    lg = logits if logits.dim() == 2 else logits.view(1, -1)
    if lg.dim() != 2 or (lg.shape[1] > 1 and lg.stride(1) != 1) or (lg.shape[0] > 1 and lg.stride(0) < lg.shape[1]):
        raise _lib.SSError("logits must be [rows, vocab] with unit stride inside a row")
    rows, vocab = lg.shape
    dev = lg.device
    if int(top_n) != top_n or not -2 ** 31 <= int(top_n) < 2 ** 31:
        raise _lib.SSError("top_n must be an integer, not %r" % (top_n,))
    top_n = int(top_n)
    tok = torch.as_tensor(ids, dtype=torch.int32, device=dev).reshape(-1).contiguous()
    if tok.numel() != rows:
        raise _lib.SSError("ids must hold one id per row (%d), not %d" % (rows, tok.numel()))
    import ctypes as C
    sps = None if sampling is None else sampling_struct(**dict(sampling))
    sp = None if sps is None else C.byref(sps)
    lp = torch.zeros(rows, dtype=torch.float32, device=dev)
    tid = torch.zeros(rows, max(top_n, 0), dtype=torch.int32, device=dev) if top_n > 0 else None
    tlp = torch.zeros(rows, max(top_n, 0), dtype=torch.float32, device=dev) if top_n > 0 else None
    check(lib().ss_token_logprobs(p(lg), rows, vocab, lg.stride(0) if rows > 1 else vocab, p(tok), sp, top_n, p(lp), p(tid), p(tlp),
                                  dt(lg), stream()), "ss_token_logprobs")
    return (lp, tid, tlp) if top_n > 0 else lp


def beam_step(logits, beam_scores, stop_ids=(), out=None):
    """One selection step of a beam search (``ss_beam_step`` in include/seedstory_hip.h): row b of ``logits`` [rows, vocab]
    (rows <= 8; only read) is running hypothesis b's edited row, ``beam_scores`` float32 [rows] its accumulated score, -inf for
    a dead row.  Returns ``(scores float32 [K], beams int32 [K], tokens int32 [K])``, the K = max(2, 1 + len(stop_ids)) * rows
    best of ``beam_scores[b] + log_softmax(row b)[t]``, descending, equal scores by ascending ``b * vocab + t``; -inf / -1 / -1
    where fewer candidates carry mass.  ``out`` = a caller's three buffers of those shapes."""
    if not logits.is_cuda:
        raise _lib.SSError("logits must live on the GPU (there is no CPU path)")
    lg = logits if logits.dim() == 2 else logits.view(1, -1)
    if lg.dim() != 2 or (lg.shape[1] > 1 and lg.stride(1) != 1) or (lg.shape[0] > 1 and lg.stride(0) < lg.shape[1]):
        raise _lib.SSError("logits must be [rows, vocab] with unit stride inside a row")
    rows, vocab = lg.shape
    dev = lg.device
    sc = torch.as_tensor(beam_scores, dtype=torch.float32, device=dev).reshape(-1).contiguous()
    if sc.numel() != rows:
        raise _lib.SSError("beam_scores must hold one score per row (%d), not %d" % (rows, sc.numel()))
    stops = [int(t) for t in stop_ids]
    for t in stops:
        if not -2 ** 31 <= t < 2 ** 31:
            raise _lib.SSError("beam_step: stop id %d is no int32" % t)
    K = max(2, 1 + len(stops)) * rows
    if out is None:
        out = (torch.empty(K, dtype=torch.float32, device=dev), torch.empty(K, dtype=torch.int32, device=dev),
               torch.empty(K, dtype=torch.int32, device=dev))
    cs, cb, ct = out
    for t, d in ((cs, torch.float32), (cb, torch.int32), (ct, torch.int32)):
        _req(t, "beam_step(out=)")
        if t.numel() != K or t.dtype != d or t.device != dev:
            raise _lib.SSError("beam_step(out=): expected %d %s entries on %s" % (K, d, dev))
    import ctypes as C
    arr = (C.c_int32 * max(1, len(stops)))(*stops)
    check(lib().ss_beam_step(p(lg), rows, vocab, lg.stride(0) if rows > 1 else vocab, p(sc), len(stops), arr, p(cs), p(cb), p(ct),
                             dt(lg), stream()), "ss_beam_step")
    return cs, cb, ct


def logits_rules_struct(repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0, spare_img_ids=False):
    """The C ABI's ``ss_logits_rules``.  Ranges are checked by the library (``SSError``); only what ctypes would mangle
    silently is checked here."""
    for name, v in (("no_repeat_ngram_size", no_repeat_ngram_size), ("min_new_tokens", min_new_tokens)):
        if int(v) != v or not -2 ** 31 <= int(v) < 2 ** 31:
            raise _lib.SSError("%s must be an integer, not %r" % (name, v))
    return _lib.LogitsRules(float(repetition_penalty), int(no_repeat_ngram_size), int(min_new_tokens), 1 if spare_img_ids else 0)


def process_logits(logits, hist, hist_len=None, prompt_len=None, repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0,
                   spare_img_ids=False, eos_id=-1, img_ids=None):
    """Hugging Face's repetition penalty -> no-repeat n-gram -> min_new_tokens on the rows of ``logits`` [rows, vocab] (or
    [vocab]; rows may be strided, unit stride inside a row), IN PLACE, by the engine's kernel routine; the image-token
    processor does not run.  ``hist`` int32 [rows, hist_ld] (or [hist_ld]) holds each row's token history, ``hist_len`` [rows]
    its length (default: all of ``hist``), ``prompt_len`` [rows] the length at hand-over (default 0); ids outside
    [0, vocab) are skipped.  ``img_ids`` is used by ``spare_img_ids`` only.  Returns ``logits``.  The definition is in
    include/seedstory_hip.h (``ss_process_logits``)."""
    if not logits.is_cuda:
        raise _lib.SSError("logits must live on the GPU (there is no CPU path)")
    lg = logits if logits.dim() == 2 else logits.view(1, -1)
    if lg.dim() != 2 or (lg.shape[1] > 1 and lg.stride(1) != 1) or (lg.shape[0] > 1 and lg.stride(0) < lg.shape[1]):
        raise _lib.SSError("logits must be [rows, vocab] with unit stride inside a row")
    rows, vocab = lg.shape
    dev = lg.device
    rp = logits_rules_struct(repetition_penalty, no_repeat_ngram_size, min_new_tokens, spare_img_ids)
    hs = torch.as_tensor(hist, dtype=torch.int32, device=dev)
    hs = _req(hs.reshape(1, -1) if hs.dim() < 2 else hs, "hist")
    if hs.shape[0] != rows:
        raise _lib.SSError("hist must hold one history per row (%d), not %d" % (rows, hs.shape[0]))

    def per_row(v, default, what):
        t = torch.full((rows,), default, dtype=torch.int32, device=dev) if v is None else \
            torch.as_tensor(v, dtype=torch.int32, device=dev).reshape(-1).contiguous()
        if t.numel() != rows:
            raise _lib.SSError("%s must hold one value per row (%d), not %d" % (what, rows, t.numel()))
        return t
    hl = per_row(hist_len, hs.shape[1], "hist_len")
    pl = per_row(prompt_len, 0, "prompt_len")
    ids = None if img_ids is None else torch.as_tensor(list(img_ids), dtype=torch.int32, device=dev)
    import ctypes as C
    check(lib().ss_process_logits(p(lg), rows, vocab, lg.stride(0) if rows > 1 else vocab, C.byref(rp), p(hs) if hs.numel() else None,
                                  hs.shape[1], p(hl), p(pl), int(eos_id), p(ids), 0 if ids is None else ids.numel(), dt(lg), stream()),
          "ss_process_logits")
    return logits


# ---- SDXL de-tokenizer ops (NHWC activations: [B, H*W, C]) ------------------------------------------
def conv3x3(x, w, B, H, W, stride=1, upsample=False, bias=None, rowvec=None, residual=None, rowvec_stride=0, out=None):
    """x [B*H*W, Cin] (NHWC) -> [B*Ho*Wo, Cout]; w [Cout, 9*Cin] (tap-major, channel-minor)."""
    _req(x); _req(w)
    Cin = x.shape[-1]
    Cout = w.shape[0]
    Hin, Win = (2 * H, 2 * W) if upsample else (H, W)
    Ho, Wo = (Hin + 2 - 3) // stride + 1, (Win + 2 - 3) // stride + 1
    y = _out(out, (B * Ho * Wo, Cout), x, "conv3x3")
    tune.ensure_conv(B, H, W, Cin, Cout, stride, upsample, dt(x), x.device)
    check(lib().ss_conv3x3(p(x), p(w), p(y), B, H, W, Cin, Cout, stride, int(upsample), p(bias), p(rowvec),
                           rowvec_stride, p(residual), dt(x), stream()), "ss_conv3x3")
    return y, Ho, Wo


def groupnorm(x, gamma, beta, B, groups, eps, silu=False):
    """x [B*HW, C] NHWC"""
    _req(x)
    C = x.shape[-1]
    HW = x.shape[0] // B
    y = torch.empty_like(x)
    nb = int(lib().ss_groupnorm_workspace_bytes(B, HW, C, groups, dt(x)))      # final sums + deterministic block partials
    ws = torch.empty(max(nb // 8, 1), dtype=torch.float64, device=x.device)
    check(lib().ss_groupnorm(p(x), p(gamma), p(beta), p(y), p(ws), B, HW, C, groups, eps, int(silu), dt(x), stream()),
          "ss_groupnorm")
    return y


# ---- loss heads of the training-side forward (forward only) ---------------------------------------
def _mean2(vals, mask):
    n = vals.numel()
    ws = torch.empty(max(int(lib().ss_loss_workspace_bytes(n)) // 8, 1), dtype=torch.float64, device=vals.device)
    out = torch.empty(2, dtype=torch.float32, device=vals.device)
    check(lib().ss_masked_mean(p(vals), p(mask) if mask is not None else None, n, p(ws), p(out), stream()), "ss_masked_mean")
    return out


def cross_entropy(logits, labels, ignore_index=-100):
    """CrossEntropyLoss()(logits [R, V], labels [R]) as modeling_llama_xformer.py:769-772 calls it: the mean over the rows whose
    label is not ``ignore_index`` -> (loss scalar tensor fp32, number of valid rows tensor)."""
    _req(logits)
    R, V = logits.shape
    labels = labels.to(device=logits.device, dtype=torch.int64).contiguous()
    assert labels.numel() == R and logits.stride(1) == 1
    row = torch.empty(R, dtype=torch.float32, device=logits.device)
    valid = torch.empty(R, dtype=torch.float32, device=logits.device)
    check(lib().ss_cross_entropy_rows(p(logits), logits.stride(0), p(labels), R, V, ignore_index, p(row), p(valid), dt(logits),
                                      stream()), "ss_cross_entropy_rows")
    out = _mean2(row, valid)
    return out[0], out[1]


def cosine_loss(rec, target):
    """models.py:13-17: (1 - (target/|target| * rec/|rec|).sum(-1)).mean() -> scalar tensor fp32."""
    _req(rec)
    _req(target)
    assert rec.shape == target.shape and rec.dtype == target.dtype
    dim = rec.shape[-1]
    r2, t2 = rec.reshape(-1, dim).contiguous(), target.reshape(-1, dim).contiguous()
    val = torch.empty(r2.shape[0], dtype=torch.float32, device=rec.device)
    check(lib().ss_cosine_rows(p(r2), p(t2), r2.shape[0], dim, p(val), dt(rec), stream()), "ss_cosine_rows")
    return _mean2(val, None)[0]


def mse_loss(a, b):
    """F.mse_loss(a.float(), b.float(), reduction='mean') (adapter_modules.py:339) -> scalar tensor fp32."""
    _req(a)
    _req(b)
    assert a.shape == b.shape and a.dtype == b.dtype
    a2, b2 = a.contiguous(), b.contiguous()
    n = a2.numel()
    ws = torch.empty(max(int(lib().ss_loss_workspace_bytes(n)) // 8, 1), dtype=torch.float64, device=a.device)
    out = torch.empty(2, dtype=torch.float32, device=a.device)
    check(lib().ss_mse(p(a2), p(b2), n, p(ws), p(out), dt(a), stream()), "ss_mse")
    return out[0]


def geglu(x):
    _req(x)
    rows, two_d = x.shape
    out = torch.empty(rows, two_d // 2, dtype=x.dtype, device=x.device)
    check(lib().ss_geglu(p(x), p(out), rows, two_d // 2, dt(x), stream()), "ss_geglu")
    return out


def silu(x):
    _req(x)
    y = torch.empty_like(x)
    check(lib().ss_unary(p(x), p(y), x.numel(), 0, dt(x), stream()), "ss_unary")
    return y


def attention_qkv_packed(qkv, B, L, n_heads, out=None):
    """Self-attention on a fused projection qkv [B*L, 3E] = [q | k | v] per token -> [B*L, E]."""
    _req(qkv)
    E = qkv.shape[1] // 3
    hd = E // n_heads
    out = _out(out, (B * L, E), qkv, "attention_qkv_packed")
    esz = qkv.element_size()
    base = qkv.data_ptr()
    check(lib().ss_attention(base, base + E * esz, base + 2 * E * esz, p(out), B, n_heads, L, L, hd, L * 3 * E, hd, 3 * E,
                             L * 3 * E, hd, 3 * E, L * 3 * E, hd, 3 * E, L * E, hd, E, 1.0 / math.sqrt(hd), 0, dt(qkv),
                             stream()), "ss_attention")
    return out


def attention_q_kvpacked(q, kv, B, Lq, Lk, n_heads, out=None):
    """Cross-attention: q [B*Lq, E], kv [B*Lk, 2E] = [k | v] per context token -> [B*Lq, E]."""
    _req(q); _req(kv)
    E = q.shape[1]
    hd = E // n_heads
    out = _out(out, q.shape, q, "attention_q_kvpacked")
    esz = q.element_size()
    kb = kv.data_ptr()
    check(lib().ss_attention(p(q), kb, kb + E * esz, p(out), B, n_heads, Lq, Lk, hd, Lq * E, hd, E, Lk * 2 * E, hd, 2 * E,
                             Lk * 2 * E, hd, 2 * E, Lq * E, hd, E, 1.0 / math.sqrt(hd), 0, dt(q), stream()), "ss_attention")
    return out


def softmax_rows_(s, scale):
    _req(s)
    check(lib().ss_softmax_rows(p(s), s.shape[0], s.shape[1], scale, dt(s), stream()), "ss_softmax_rows")
    return s


def transpose(x):
    _req(x)
    R, Cc = x.shape
    out = torch.empty(Cc, R, dtype=x.dtype, device=x.device)
    check(lib().ss_transpose(p(x), p(out), R, Cc, dt(x), stream()), "ss_transpose")
    return out


def concat_channels(a, b):
    _req(a); _req(b)
    rows = a.shape[0]
    out = torch.empty(rows, a.shape[1] + b.shape[1], dtype=a.dtype, device=a.device)
    check(lib().ss_concat_channels(p(a), p(b), p(out), rows, a.shape[1], b.shape[1], dt(a), stream()),
          "ss_concat_channels")
    return out


def nchw_to_nhwc(x, cpad):
    _req(x)
    B, Cc = x.shape[0], x.shape[1]
    HW = x[0, 0].numel()
    out = torch.empty(B * HW, cpad, dtype=x.dtype, device=x.device)
    check(lib().ss_layout_nchw_nhwc(p(x), p(out), B, Cc, HW, cpad, 1, dt(x), stream()), "ss_layout_nchw_nhwc")
    return out


def nhwc_to_nchw(x, B, C, H, W):
    _req(x)
    out = torch.empty(B, C, H, W, dtype=x.dtype, device=x.device)
    check(lib().ss_layout_nchw_nhwc(p(x), p(out), B, C, H * W, x.shape[-1], 0, dt(x), stream()), "ss_layout_nchw_nhwc")
    return out


def euler_scale_dup(x, sigma):
    _req(x)
    xin = torch.empty((2,) + tuple(x.shape), dtype=x.dtype, device=x.device)
    check(lib().ss_euler_scale_dup(p(x), p(xin), x.numel(), float(sigma), dt(x), stream()), "ss_euler_scale_dup")
    return xin


def euler_cfg_step_(x, eps, guidance, sigma, sigma_next):
    _req(x); _req(eps)
    check(lib().ss_euler_cfg_step(p(x), p(eps), x.numel(), float(guidance), float(sigma), float(sigma_next), dt(x),
                                  stream()), "ss_euler_cfg_step")
    return x


def multistep_cfg_step_(state, eps, guidance, sigma, a, b, c, inv_next, x_out=None, xin_next=None):
    """One sampler step on the fp32 state [2, n] = (x, d_prev) from eps [2, ...] = [uncond; cond] (``ss_multistep_cfg_step``):
    x' = a x + b d + c d_prev with d = x - sigma (eu + g (ec - eu)); state <- (x', d).  ``x_out`` (n elements of eps's dtype)
    receives x', ``xin_next`` (2 n elements) the next step's scaled, CFG-duplicated UNet input x' * inv_next."""
    _req(state, "state"); _req(eps, "eps")
    n = eps.numel() // 2
    if state.dtype != torch.float32 or state.numel() != 2 * n or eps.numel() != 2 * n:
        raise _lib.SSError("multistep_cfg_step: state must be fp32 [2, n] for eps [2, n]")
    for t, name, cnt in ((x_out, "x_out", n), (xin_next, "xin_next", 2 * n)):
        if t is not None:
            _req(t, name)
            if t.dtype != eps.dtype or t.numel() != cnt or t.device != eps.device:
                raise _lib.SSError("multistep_cfg_step: %s must hold %d %s elements on %s" % (name, cnt, eps.dtype, eps.device))
    check(lib().ss_multistep_cfg_step(p(state), p(eps), p(x_out), p(xin_next), n, float(guidance), float(sigma), float(a),
                                      float(b), float(c), float(inv_next), dt(eps), stream()), "ss_multistep_cfg_step")
    return state


def multistep_step_(state, eps, guidance, sigma, a, b, c, inv_next, eps_rows=2, x_out=None, xin_next=None, xin_rows=2):
    """``multistep_cfg_step_`` for limited-interval guidance (``ss_multistep_step``): eps is [eps_rows, n] — [uncond; cond], or
    the conditional prediction alone (``eps_rows`` 1: e = ec, ``guidance`` unused) — and ``xin_next`` [xin_rows, n] receives one
    copy of the next step's scaled input (the next step is unguided) or two."""
    _req(state, "state"); _req(eps, "eps")
    if eps_rows not in (1, 2) or xin_rows not in (1, 2):
        raise _lib.SSError("multistep_step: eps_rows %r / xin_rows %r must be 1 or 2" % (eps_rows, xin_rows))
    n = state.numel() // 2
    if state.dtype != torch.float32 or state.numel() != 2 * n or eps.numel() != eps_rows * n or n == 0:
        raise _lib.SSError("multistep_step: state must be fp32 [2, n] for eps [%d, n]" % eps_rows)
    for t, name, cnt in ((x_out, "x_out", n), (xin_next, "xin_next", xin_rows * n)):
        if t is not None:
            _req(t, name)
            if t.dtype != eps.dtype or t.numel() != cnt or t.device != eps.device:
                raise _lib.SSError("multistep_step: %s must hold %d %s elements on %s" % (name, cnt, eps.dtype, eps.device))
    check(lib().ss_multistep_step(p(state), p(eps), p(x_out), p(xin_next), n, eps_rows, xin_rows, float(guidance), float(sigma),
                                  float(a), float(b), float(c), float(inv_next), dt(eps), stream()), "ss_multistep_step")
    return state


def noise_seeds(seeds, device):
    """64-bit noise seeds (an int or a sequence of ints, any sign; taken mod 2^64) -> int64 [B] on ``device`` holding their
    bits: what ``randn_philox`` and ``multistep_noise_step_`` read as uint64."""
    vals = [int(seeds)] if isinstance(seeds, int) else [int(v) for v in seeds]
    vals = [v % (1 << 64) for v in vals]
    return torch.tensor([v - (1 << 64) if v >= (1 << 63) else v for v in vals], dtype=torch.int64).to(device)


def _req_seeds(seeds, who):
    _req(seeds, "seeds")
    if seeds.dtype != torch.int64 or seeds.dim() != 1 or seeds.numel() == 0:
        raise _lib.SSError("%s: seeds must be int64 [batch] (the bits of the uint64 seeds; see noise_seeds)" % who)
    return seeds


def randn_philox(seeds, n_img, step, dtype, out=None):
    """[batch, n_img] standard normals, row b from ``seeds[b]`` (int64 [batch] device tensor, see ``noise_seeds``) and ``step``
    alone — the noise of the stochastic samplers (``ss_randn_philox``); a row does not depend on the batch it is drawn in."""
    _req_seeds(seeds, "randn_philox")
    B, n_img, step = seeds.numel(), int(n_img), int(step)
    if n_img <= 0 or step < 0:
        raise _lib.SSError("randn_philox: n_img %d must be > 0 and step %d >= 0" % (n_img, step))
    if out is None:
        out = torch.empty(B, n_img, dtype=dtype, device=seeds.device)
    else:
        _req(out, "out")
        if out.numel() != B * n_img or out.dtype != dtype or out.device != seeds.device:
            raise _lib.SSError("randn_philox: out must hold %d %s elements on %s" % (B * n_img, dtype, seeds.device))
    check(lib().ss_randn_philox(p(out), p(seeds), B, n_img, step, dt(dtype), stream()), "ss_randn_philox")
    return out


def multistep_noise_step_(state, eps, guidance, sigma, a, b, c, s, inv_next, seeds, step, eps_rows=2, x_out=None, xin_next=None,
                          xin_rows=2):
    """``multistep_step_`` with a noise term (``ss_multistep_noise_step``): x' = a x + b d + c d_prev + s z, z the standard
    normals of ``randn_philox(seeds, n / len(seeds), step)``, generated inside the same launch.  ``seeds``: int64 [B] on the
    device (``noise_seeds``), the state holds B images of n / B elements; ``seeds`` may be None when s == 0."""
    _req(state, "state"); _req(eps, "eps")
    if eps_rows not in (1, 2) or xin_rows not in (1, 2):
        raise _lib.SSError("multistep_noise_step: eps_rows %r / xin_rows %r must be 1 or 2" % (eps_rows, xin_rows))
    n = state.numel() // 2
    if state.dtype != torch.float32 or state.numel() != 2 * n or eps.numel() != eps_rows * n or n == 0:
        raise _lib.SSError("multistep_noise_step: state must be fp32 [2, n] for eps [%d, n]" % eps_rows)
    if seeds is None:
        if float(s) != 0.0:
            raise _lib.SSError("multistep_noise_step: s = %r needs seeds" % (s,))
        B = 1
    else:
        B = _req_seeds(seeds, "multistep_noise_step").numel()
        if n % B or seeds.device != eps.device:
            raise _lib.SSError("multistep_noise_step: %d seeds on %s for a state of %d elements on %s" % (B, seeds.device, n, eps.device))
    for t, name, cnt in ((x_out, "x_out", n), (xin_next, "xin_next", xin_rows * n)):
        if t is not None:
            _req(t, name)
            if t.dtype != eps.dtype or t.numel() != cnt or t.device != eps.device:
                raise _lib.SSError("multistep_noise_step: %s must hold %d %s elements on %s" % (name, cnt, eps.dtype, eps.device))
    check(lib().ss_multistep_noise_step(p(state), p(eps), p(x_out), p(xin_next), n, eps_rows, xin_rows, float(guidance),
                                        float(sigma), float(a), float(b), float(c), float(s), float(inv_next), p(seeds), n // B,
                                        int(step), dt(eps), stream()), "ss_multistep_noise_step")
    return state


def euler_step_(x, eps, sigma, sigma_next):
    """Unguided Euler step in place: x += eps * (sigma_next - sigma), eps the conditional prediction (``ss_euler_step``)."""
    _req(x, "x"); _req(eps, "eps")
    if eps.numel() != x.numel() or eps.dtype != x.dtype or eps.device != x.device:
        raise _lib.SSError("euler_step: eps must hold %d %s elements on %s" % (x.numel(), x.dtype, x.device))
    check(lib().ss_euler_step(p(x), p(eps), x.numel(), float(sigma), float(sigma_next), dt(x), stream()), "ss_euler_step")
    return x


def euler_scale(x, sigma, rows=2, out=None):
    """scale_model_input into ``rows`` (1 | 2) copies: [rows, *x.shape] = x / sqrt(sigma^2 + 1) (``ss_euler_scale``); ``out``:
    a tensor of rows * x.numel() elements to write into (a captured forward's input buffer)."""
    _req(x, "x")
    if rows not in (1, 2):
        raise _lib.SSError("euler_scale: rows %r must be 1 or 2" % (rows,))
    if out is None:
        out = torch.empty((rows,) + tuple(x.shape), dtype=x.dtype, device=x.device)
    else:
        _req(out, "out")
        if out.numel() != rows * x.numel() or out.dtype != x.dtype or out.device != x.device:
            raise _lib.SSError("euler_scale: out must hold %d %s elements on %s" % (rows * x.numel(), x.dtype, x.device))
    check(lib().ss_euler_scale(p(x), p(out), x.numel(), rows, float(sigma), dt(x), stream()), "ss_euler_scale")
    return out


def image_to_u8(x, pixels):
    _req(x)
    out = torch.empty(pixels, 3, dtype=torch.uint8, device=x.device)
    check(lib().ss_image_to_u8(p(x), p(out), pixels, x.shape[-1], dt(x), stream()), "ss_image_to_u8")
    return out
