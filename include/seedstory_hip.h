/* libseedstory_hip.so — C ABI of the MI355X-native (gfx950) SEED-Story hot path.
 *
 * The reference (TencentARC/SEED-Story) has no FFI: its hot path sits behind Python-level
 * plug points.  This header is the boundary a maintainer binds with
 * ctypes from those plug points; every entry point cites the
 * reference interface it replaces (paths relative to the reference repo root).
 *
 * Rules of the ABI
 *   - plain pointers and sizes only; pointers are DEVICE pointers unless named host_*;
 *   - every call enqueues asynchronously on the caller's `stream` (a hipStream_t passed
 *     as void*; NULL = the legacy default stream) and returns immediately; the only
 *     exceptions are named: ss_llama_generate* (return a host count), ss_llama_profile_decode
 *     and the explicit tuning calls ss_gemm_tune / ss_conv3x3_tune;
 *   - return 0 (SS_OK) or a negative SS_E* code; ss_last_error() gives the message
 *     (thread-local); nothing throws; nothing allocates or frees caller memory —
 *     workspaces are passed in, sized by the *_workspace_bytes() queries; the only
 *     library-owned objects are the engine handles (ss_llama_create / ss_vit_create …);
 *   - `dtype` is the model dtype of activations AND weights: SS_F32 (CPU-parity mode),
 *     SS_BF16 (production), SS_F16.  Accumulation is always fp32; values are rounded to
 *     the model dtype where the reference's torch graph rounds them.
 *   - there is no CPU fallback: every function fails with SS_EHIP when no gfx950 device
 *     is usable.
 */
#ifndef SEEDSTORY_HIP_H_
#define SEEDSTORY_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SS_ABI_VERSION 1

enum { SS_F32 = 0, SS_BF16 = 1, SS_F16 = 2 };
enum { SS_OK = 0, SS_EINVAL = -1, SS_EHIP = -2, SS_ENOMEM = -3, SS_ESTATE = -4 };

/* GEMM / GEMV epilogues (bit flags) */
enum {
    SS_EPI_NONE = 0,
    SS_EPI_BIAS = 1,      /* + bias[N]                                                   */
    SS_EPI_GELU = 2,      /* exact-erf GELU after bias (nn.GELU, qwen_visual.py:258-260)  */
    SS_EPI_RESIDUAL = 4,  /* out = residual + round_T(acc [+bias])                        */
    SS_EPI_SILU_MUL = 8,  /* GEMV only: y[n] = silu(acc[n]) * acc[n+N]  (LlamaMLP :190)   */
    SS_EPI_GEGLU_PAIR = 16 /* GEMM only: W rows interleaved (value_i, gate_i); C[m][i] = (acc+b)[2i] * gelu_erf((acc+b)[2i+1]),
                              C has N/2 columns (diffusers GEGLU fused into ff.net.0.proj)   */
};

const char* ss_last_error(void);
int ss_abi_version(void);
/* Device properties of the current HIP device: out[0]=CU count, out[1]=is_gfx950,
 * out[2]=total HBM MiB, out[3]=wavefront size. */
int ss_device_info(int32_t out[4]);
/* Runtime tuning knobs (kernel choices, grid sizes, arithmetic modes, …).  The complete list, with defaults and one line per
 * knob, is csrc/ss_knobs.h; a key that is not in it does not exist.
 *   ss_set_tuning: stores the value of a known key; an unknown or NULL key returns SS_EINVAL and ss_last_error() names it.
 *                  Counters (gemv_split_refused) may be set too, which is how a caller resets them.
 *   ss_get_tuning: the value of a known key that has been set or has a constant default; `dflt` for a known key that is still
 *                  unset (gemm_fp8_swz, img_block_decode: the default is decided where the knob is read) and for an unknown key. */
int ss_set_tuning(const char* key, int value);
int ss_get_tuning(const char* key, int dflt);

/* LayerNorm folded into the GEMM that consumes it (the UNet's norm1 -> q|k|v, norm2 -> to_q, norm3 -> ff1; reference:
 * diffusers BasicTransformerBlock, `attn(norm(h))`): with  LN(h) = (h - mean) * rstd * gamma + beta
 *     LN(h) · W^T + b  =  rstd[m] * (h · Wg^T)[m][n]  -  rstd[m] * mean[m] * c[n]  +  d[n]
 * where Wg = gamma ∘ W (rounded to the model dtype once at load), c[n] = sum_k Wg[n][k] (fp32), d[n] = b[n] + sum_k
 * beta[k] W[n][k].  The normalised activation tensor is never written or re-read: the GEMM streams the RAW rows, the
 * epilogue applies  t = acc * rstd[m] + shift[m] * c[n] + d[n]  (shift = -mean * rstd) in fp32 and continues with GELU /
 * GEGLU pairs as ss_gemm does.  Rounding differs from the unfused form (LN output not rounded to bf16; gamma rounded
 * into the weight): same order of magnitude, covered by the bf16 parity gates.
 *   ss_rowstats     x [M, K] (16-bit, row stride ld, K <= 2048) -> rstd_out[M], shift_out[M] (fp32)
 *   ss_gemm_lnfold  A [M, K] raw rows, Wg [N, K]; `bias` carries d (model dtype); K % 64 == 0, N % 16 == 0;
 *                   epilogue flags BIAS | GELU | GEGLU_PAIR.
 *
 * Producer-carried statistics (round 3): the LayerNorm's row statistics need no pass of their own when the GEMM that
 * PRODUCES h (attn.to_out + residual, ff.net.2 + residual, proj_in) accumulates them while it stores h:
 *   ss_gemm_rowstat      ss_gemm whose epilogue also adds, per output row m, sum_n C[m][n] and sum_n C[m][n]^2 of the
 *                        values as stored (rounded to the model dtype, residual included) into rowstat_accum[2m],
 *                        rowstat_accum[2m+1] (fp64 atomics — one pair per row per column tile; the caller zeroes the
 *                        array before the call; 16-byte aligned; any epilogue except GEGLU_PAIR);
 *   ss_rowstat_finalize  rowstat[2m .. 2m+1] -> rstd_out[m], shift_out[m] (mean = s / width, var = q / width - mean^2
 *                        formed in fp64: no cancellation), the inputs of ss_gemm_lnfold; re-zeroes rowstat for the next
 *                        producer.  One accumulator per row count serves a whole forward: producer, finalize and
 *                        consumer follow each other on the stream. */
int ss_rowstats(const void* x, int64_t ld, int64_t M, int64_t K, float eps, float* rstd_out, float* shift_out, int dtype, void* stream);
/* Small-M weight-streaming GEMM (128 < M <= 512 rows against a LLaMA projection: the stacked image-token block of the
 * lock-step stories, 4 x 66 rows, and their first prompts): C = A W^T (+bias)(+residual), A [M, K], W [N, K], C [M, N]
 * contiguous.  K is split over grid.y so that every CU holds two workgroups with short K loops; fp32 partial sums go to
 * the caller's workspace (ss_gemm_splitk_workspace_bytes; 0 = shape not eligible) and a reduce pass applies the epilogue
 * in ss_gemm's order.  Falls back to ss_gemm when the shape is not eligible or the workspace is missing / too small. */
size_t ss_gemm_splitk_workspace_bytes(int64_t M, int64_t N, int64_t K);
int ss_gemm_splitk(const void* A, const void* W, void* C, int64_t M, int64_t N, int64_t K, const void* bias, const void* residual,
                   void* workspace, size_t workspace_bytes, int dtype, void* stream);
int ss_gemm_rowstat(const void* A, const void* W, void* C, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldw,
                    int64_t ldc, const void* bias, const void* residual, int64_t ldr, int epilogue, double* rowstat_accum,
                    int dtype, void* stream);
int ss_rowstat_finalize(double* rowstat, int64_t M, int64_t width, float eps, float* rstd_out, float* shift_out, void* stream);
int ss_gemm_lnfold(const void* A, const void* Wg, void* C, int64_t M, int64_t N, int64_t K, int64_t ldc, const float* rstd,
                   const float* shift, const float* colsum, const void* bias, int epilogue, int dtype, void* stream);
/* Round 4 — the same pair WITHOUT atomics and WITHOUT a finalize launch (deterministic; what UNet2DConditionModel.enable_lnfold
 * uses): every wave column strip of the producer tile writes its (sum, sum of squares) of row m ONCE to
 * rowpart[(m * strips + strip) * 2 .. +1] (fp32; strips = ss_gemm_rowpart_strips(M, N, K, dtype) = N / strip width of the
 * tile ss_gemm_rowpart will run, 0 = shape not eligible: N must be a multiple of the tile width, operands 16-byte aligned);
 * nothing needs zeroing.  ss_gemm_lnfold_part is ss_gemm_lnfold whose epilogue sums the `strips` partials of its rows and
 * forms rstd / -mean * rstd itself (mean = s / width, var = q / width - mean^2 in fp64).  Only the LDS-staged epilogue does
 * that, so every wave must take it: N a multiple of 160 or 128 (a wider tile gives way to the 160- / 128-wide one), C and a
 * non-null bias pointer (whether or not the epilogue uses it) 16-byte aligned, ldc % 8 == 0; anything else is SS_EINVAL. */
int64_t ss_gemm_rowpart_strips(int64_t M, int64_t N, int64_t K, int dtype);
int ss_gemm_rowpart(const void* A, const void* W, void* C, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldw,
                    int64_t ldc, const void* bias, const void* residual, int64_t ldr, int epilogue, float* rowpart,
                    int dtype, void* stream);
int ss_gemm_lnfold_part(const void* A, const void* Wg, void* C, int64_t M, int64_t N, int64_t K, int64_t ldc, const float* rowpart,
                        int64_t strips, int64_t width, float eps, const float* colsum, const void* bias, int epilogue, int dtype,
                        void* stream);

/* fp8 (OCP e4m3fn) GEMM path of the SDXL UNet's linear layers (SURVEY §8 ★ row; BASELINE configs[4]).  The reference
 * has no fp8 path; this is the bf16 GEMM  C = A · W^T (+bias)(+GELU | GEGLU)(+residual)  with both operands quantised:
 *   q = RNE_e4m3(x * 448 / amax(row)),  scale = amax(row) / 448   (activations: per token row; weights: per output channel)
 * and  C = round_bf16(acc_fp32 * scale_a[m] * scale_w[n] + bias ...).  The matrix instruction is
 * v_mfma_scale_f32_16x16x128_f8f6f4 with unit block scales (twice the bf16 MFMA rate on gfx950).
 *   ss_quantize_rows_fp8  x [M, K] (16-bit dtype, row stride ld) -> q [M, K] bytes + scale [M] fp32.  With ln_gamma /
 *       ln_beta != NULL the rows are LayerNorm-ed first (eps = ln_eps; the normalised value is rounded to `dtype` as the
 *       unfused ss_layernorm would) — the bf16 normalised tensor is never written.  Also used once per weight at load.
 *   ss_gemm_fp8  A8 [M, K], W8 [N, K] row-major bytes, K % 128 == 0; C / bias / residual are bf16.  Epilogue flags as
 *       ss_gemm (BIAS, GELU, RESIDUAL, GEGLU_PAIR).  Exact w.r.t. its quantised operands (fp32 accumulation). */
int ss_quantize_rows_fp8(const void* x, int64_t ld, int64_t M, int64_t K, void* q_out, float* scale_out, const void* ln_gamma,
                         const void* ln_beta, float ln_eps, int dtype, void* stream);
int ss_gemm_fp8(const void* A8, const float* scale_a, const void* W8, const float* scale_w, void* C, int64_t M, int64_t N,
                int64_t K, int64_t ldc, const void* bias, const void* residual, int64_t ldr, int epilogue, void* stream);

/* Device context ("no hidden global state except a per-device handle").  A process drives one GPU; the
 * library's only state besides the thread-local error string — the tuning knobs and the GEMM tile table — is
 * process-global and valid for any gfx950 device (the only architecture accepted).  ss_create validates `device`, makes
 * it the current HIP device and returns a handle; ss_destroy releases the handle and leaves the tile table alone (other
 * users of the library in the process keep their tuned tiles; ss_tune_clear drops it explicitly).  Op entry points act
 * on the current HIP device and take no handle.
 * ss_context_info: out = {device ordinal, CU count, HBM bytes}. */
typedef struct ss_context ss_context;
int ss_create(int device, ss_context** out);
int ss_context_info(const ss_context* ctx, int64_t out[3]);
void ss_destroy(ss_context* ctx);

/* RCCL exchange step of the multi-GPU slot ring (reference: single device, gen_george.py:18; the dependency between
 * story steps is `image_embeds = torch.cat((image_embeds, image_embeds_gen))`, :224): the regressed image feature and
 * the KV-cache rows a round appended travel from the round's owner to the other ranks (seedstory/parallel.py does the
 * same through torch.distributed).  librccl is resolved with dlopen at the first call (SS_ESTATE when it is absent).
 * ss_rccl_unique_id: rank 0 fills a 128-byte id and hands it to the other ranks out of band; ss_rccl_init is collective.
 * send / recv / bcast enqueue on `stream`; `count` elements of `dtype`; bcast is in place. */
typedef struct ss_rccl ss_rccl;
int ss_rccl_unique_id(void* id_out_128_bytes);
int ss_rccl_init(const void* id_128_bytes, int nranks, int rank, ss_rccl** out);
void ss_rccl_destroy(ss_rccl* c);
int ss_rccl_send(ss_rccl* c, const void* buf, int64_t count, int dtype, int peer, void* stream);
int ss_rccl_recv(ss_rccl* c, void* buf, int64_t count, int dtype, int peer, void* stream);
int ss_rccl_bcast(ss_rccl* c, void* buf, int64_t count, int dtype, int root, void* stream);

/* ---------------------------------------------------------------------------------------
 * Norms and element-wise ops
 * ------------------------------------------------------------------------------------- */

/* LlamaRMSNorm.forward — src/models_clm/modeling_llama_xformer.py:107-115.
 * y = w * round_T(x * rsqrt(mean_fp32(x^2) + eps)); x,y [rows, cols]; w [cols]. */
int ss_rmsnorm(const void* x, const void* w, void* y, int64_t rows, int64_t cols, float eps, int dtype,
               void* stream);

/* nn.LayerNorm (qwen_visual.py:103,353; resampler.py norm layers): fp32 statistics,
 * y = round_T((x-mean)*rstd*w + b). */
int ss_layernorm(const void* x, const void* w, const void* b, void* y, int64_t rows, int64_t cols, float eps,
                 int dtype, void* stream);

/* y[b, r, :] = x[b, r, :] + p[r, :]   (position-embedding adds, qwen_visual.py:147-148,387;
 * x may be NULL-batched: if x_batch_stride == 0 the same x rows are used for every b). */
int ss_add_bcast(const void* x, const void* p, void* y, int64_t batch, int64_t rows, int64_t cols,
                 int64_t x_batch_stride, int dtype, void* stream);

/* out[r, i] = silu(gu[r, i]) * gu[r, inter + i]; gu [rows, 2*inter] (LlamaMLP, :190-191). */
int ss_silu_mul(const void* gu, void* out, int64_t rows, int64_t inter, int dtype, void* stream);

/* Embedding lookup: out[i, :] = table[ids[i], :] (models.py:127); ids int32 on device. */
int ss_gather_rows(const void* table, const int32_t* ids, void* out, int64_t n, int64_t cols, int dtype,
                   void* stream);
/* Splice: dst[idx[i], :] = src[i, :] (models.py:135: input_embeds[ids_cmp_mask] = ...). */
int ss_scatter_rows(const void* src, const int32_t* idx, void* dst, int64_t n, int64_t cols, int dtype,
                    void* stream);
/* Conv2d(k=stride=patch, no bias) input re-layout for the ViT patch embed (qwen_visual.py:347,382):
 * img [B,3,S,S] (T) -> patches [B*(S/p)^2, kpad] with column order (c, dy, dx), zero padded to kpad. */
int ss_im2col_patch(const void* img, void* out, int64_t batch, int64_t size, int64_t patch, int64_t kpad,
                    int dtype, void* stream);
/* F.normalize(x) over dim=1 of [B, L, C] (resampler.py:269): x / max(||x||_2 over L, 1e-12). */
int ss_l2normalize_dim1(const void* x, void* y, int64_t batch, int64_t len, int64_t cols, int dtype,
                        void* stream);

/* ---------------------------------------------------------------------------------------
 * RoPE + KV cache
 * ------------------------------------------------------------------------------------- */

/* apply_rotary_pos_emb + KV concatenation — modeling_llama_xformer.py:158-173, 236-242.
 * qkv [M, 3*n_heads*hd] (q | k | v per token).  Rotates q in the model dtype with the
 * (model-dtype) tables cos/sin [max_pos, hd] at positions pos_ids[m] (device int32; if NULL,
 * pos_start + m), writes q_out [M, n_heads*hd], and appends rotated k and v into the caches
 * kcache/vcache [n_heads, cache_cap, hd] at slots kv_start + m (keys cached AFTER RoPE). */
int ss_rope_kv_append(const void* qkv, void* q_out, void* kcache, void* vcache, const void* cos,
                      const void* sin, const int32_t* pos_ids, int64_t pos_start, int64_t M, int64_t n_heads,
                      int64_t hd, int64_t kv_start, int64_t cache_cap, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------
 * Attention
 * ------------------------------------------------------------------------------------- */

/* Fused softmax attention (flash style, MFMA) replacing
 *   xops.memory_efficient_attention(q,k,v, LowerTriangularFromBottomRightMask) (:289-295)
 *   when causal_br=1 (query i attends keys j <= i + kv_len - q_len), and the unfused
 *   bmm/softmax/bmm of VisualAttention (qwen_visual.py:207-220), nn.MultiheadAttention
 *   (:147-149) and PerceiverAttention (resampler.py:69-72) when causal_br=0.
 * Element (b,h,i,d) of q is at q + b*q_sb + h*q_sh + i*q_ss + d (strides in elements),
 * likewise k/v (k_s*, v_s*) and out (o_s*).  hd <= 128 (104 and 64 are supported);
 * softmax in fp32; P and output rounded to T.  `scale` multiplies q·k. */
int ss_attention(const void* q, const void* k, const void* v, void* out, int64_t batch, int64_t n_heads,
                 int64_t q_len, int64_t kv_len, int64_t hd, int64_t q_sb, int64_t q_sh, int64_t q_ss,
                 int64_t k_sb, int64_t k_sh, int64_t k_ss, int64_t v_sb, int64_t v_sh, int64_t v_ss,
                 int64_t o_sb, int64_t o_sh, int64_t o_ss, float scale, int causal_br, int dtype,
                 void* stream);

/* The same with one key count PER batch element (host array of `batch` <= 8 ints; strides as above): the stacked forward
 * of several story slots whose caches hold different lengths — query rows [b*q_len, (b+1)*q_len) of slot b attend to the
 * first host_kv_lens[b] entries of slot b's cache, bottom-right causal per slot (modeling_llama_xformer.py:289-295 run
 * once per story by the reference; LlamaEngine.prefill_batch issues ONE launch for the group). */
int ss_attention_ragged(const void* q, const void* k, const void* v, void* out, int64_t batch, int64_t n_heads,
                        int64_t q_len, const int32_t* host_kv_lens, int64_t hd, int64_t q_sb, int64_t q_sh, int64_t q_ss,
                        int64_t k_sb, int64_t k_sh, int64_t k_ss, int64_t v_sb, int64_t v_sh, int64_t v_ss,
                        int64_t o_sb, int64_t o_sh, int64_t o_ss, float scale, int causal_br, int dtype,
                        void* stream);

/* Single-query decode attention over the KV cache (q_len = 1 case of :289-295), split-KV.
 * q [n_heads*hd]; caches [n_heads, cache_cap, hd]; kv_len read on the device from
 * *kv_len_dev (so the launch can be replayed from a hipGraph); out [n_heads*hd].
 * workspace: ss_attn_decode_workspace_bytes(n_heads, hd). */
size_t ss_attn_decode_workspace_bytes(int64_t n_heads, int64_t hd);
int ss_attn_decode(const void* q, const void* kcache, const void* vcache, void* out, void* workspace,
                   const int32_t* kv_len_dev, int64_t n_heads, int64_t hd, int64_t cache_cap, int dtype,
                   void* stream);

/* fp8 (OCP e4m3fn) shadow of a KV cache, for the q_len = 1 decode token (the engine option: ss_llama_set_kv8).
 * The quantisation, per (head, position), of the hd values x of a key (post-RoPE, as stored) or a value in the model dtype:
 *   amax = max |x_j|;  amax == 0: scale = 1, every code 0;  otherwise scale = 2^e with the smallest integer e such that
 *   amax <= 448 * 2^e  (amax = m * 2^t, m in [0.5, 1): e = t - 9 if m <= 0.875, else t - 8), e >= -126;
 *   code_j = e4m3fn(x_j * 2^-e), round to nearest even (the product is exact in fp32 and at most 448: nothing saturates).
 * A power-of-two scale costs no relative precision in e4m3's normal range, and code * scale is exactly representable in bf16
 * and fp16.  Rows with non-finite entries are outside the definition (no fault, any result).
 * ss_kv_quantize_fp8: rows [lo, hi) of the planes k, v [n_heads, cache_cap, hd] of ONE layer -> k_codes, v_codes (same shape,
 * bytes) and k_scale, v_scale fp32 [n_heads, cache_cap]; nothing outside those rows is written.
 * ss_attn_decode_kv8: ss_attn_decode over such planes, fp32 throughout: s = (q . codes) * k_scale[key] / sqrt(hd),
 * out = sum softmax(s) * v_scale[key] * codes.  Positions >= *kv_len_dev are never read, codes or scales.  Same workspace.
 * bf16 / fp16 only; hd a multiple of 16, at most 256, hd / 16 a power of two (64 and 128 are).  SS_EINVAL before anything is
 * launched: fp32, another hd, a NULL plane, a code plane that is not 16-byte aligned. */
int ss_kv_quantize_fp8(const void* k, const void* v, void* k_codes, void* v_codes, float* k_scale, float* v_scale,
                       int64_t n_heads, int64_t cache_cap, int64_t hd, int64_t lo, int64_t hi, int dtype, void* stream);
int ss_attn_decode_kv8(const void* q, const void* k_codes, const void* v_codes, const float* k_scale, const float* v_scale,
                       void* out, void* workspace, const int32_t* kv_len_dev, int64_t n_heads, int64_t hd, int64_t cache_cap,
                       int dtype, void* stream);

/* The attention of ONE decode token as the engine launches it, for nb <= 8 sequences at once: RoPE of q and of the new k, the
 * append of the new K / V row, split-KV attention over the old keys and the new one, the split merge.  Sequence b reads
 *   qkv + b * 3 * n_heads * hd          its pre-RoPE q | k | v row;
 *   state[b * state_stride + w]         int32 words (device): w = kv_len_word -> L, the keys already cached (0 <= L <= cache_cap);
 *                                       w = pos_word -> P, the RoPE position of the new token (its own word: not L);
 *                                       w = done_word -> non-zero: the sequence is finished (done_word < 0: no such flag);
 *   kcache / vcache + b * cache_stride  its planes [n_heads, cache_cap, hd] (cache_stride in elements),
 * and writes out + b * n_heads * hd.  It rotates q and k at row P of cos / sin [max_pos, hd] (the bits ss_rope_kv_append
 * produces), stores the rotated k and v at row L of every head when L < cache_cap (L == cache_cap: nothing is stored, the new
 * key is attended all the same), and attends keys [0, L]: rows [0, L) from the cache, the new one from registers.  Rows > L are
 * never read.  A finished sequence is skipped altogether: nothing of its planes or its out row is written.  The state is only read.
 * The split count is that of the engine: 16 / nb rounded to 4 / 8 / 16 (knob attn_decode_nsplit).
 * workspace: nb * ss_attn_decode_workspace_bytes(n_heads, hd).
 * ss_attn_decode_kv8_step: the same over the fp8 shadow.  Old keys are read from k_codes / v_codes / k_scale / v_scale
 * (sequence b: b * cache_stride codes and b * cache_stride / hd scales further on — the shadow is laid out like the planes, one
 * scale per row), the new key is attended UNQUANTISED from registers; the new row goes to the 16-bit planes as above and, quantised as
 * ss_kv_quantize_fp8 defines, to the shadow (codes and both scales of row L, every head).  bf16 / fp16 only.
 * SS_EINVAL before anything is launched: a NULL pointer; qkv, a plane, a code plane or a RoPE table that is not 16-byte aligned
 * (scales: 4); nb outside [1, 8]; a head dim the kernel does not take (hd * element size a multiple of 16, hd / vector width a
 * power of two <= 64; the shadow: the rule of ss_attn_decode_kv8); cache_stride below n_heads * cache_cap * hd or not a multiple
 * of hd; a negative kv_len_word / pos_word. */
int ss_attn_decode_step(const void* qkv, void* kcache, void* vcache, const void* cos, const void* sin, void* out, void* workspace,
                        const int32_t* state, int64_t kv_len_word, int64_t pos_word, int64_t done_word, int64_t state_stride,
                        int64_t nb, int64_t n_heads, int64_t hd, int64_t cache_cap, int64_t cache_stride, int dtype, void* stream);
int ss_attn_decode_kv8_step(const void* qkv, void* kcache, void* vcache, void* k_codes, void* v_codes, float* k_scale,
                            float* v_scale, const void* cos, const void* sin, void* out, void* workspace, const int32_t* state,
                            int64_t kv_len_word, int64_t pos_word, int64_t done_word, int64_t state_stride, int64_t nb,
                            int64_t n_heads, int64_t hd, int64_t cache_cap, int64_t cache_stride, int dtype, void* stream);

/* Attention MAP of one head, as the reference returns it under `output_attentions`
 * (modeling_llama_xformer.py:246-276, 299-301): PRE-softmax scores with the mask added, every rounding in the model dtype:
 *   s = rnd_T(rnd_T(q . k) / sqrt(head_dim)), q / k post-RoPE.
 * q [M, head_dim] rows of one head (row stride ldq), k [kv, head_dim] one head's plane of the KV cache (row stride ldk),
 * out [M, ldo] in the model dtype.  Row i's own key is column kv - M + i (kv >= M).
 *   row_calls = 0: the M rows are ONE reference call.  M > 1: all kv columns are written, s where j <= own(i), else
 *                  rnd_T(s + finfo(T).min) (the additive causal mask; added and rounded, not a constant).  M == 1: all kv
 *                  columns are written, s, and rnd_T(s + 1) on the last one (the bool mask of the one-row call).
 *   row_calls = 1: every row is its own one-row call: row i writes columns [0, own(i)], rnd_T(s + 1) on own(i); columns
 *                  beyond are NOT touched (the caller pre-fills them, with NaN to match the reference's merged maps).
 * Nothing outside [M, kv] of out is written.  head_dim 128 or 64; q, k and their strides 16-byte aligned. */
int ss_attn_scores(const void* q, int64_t ldq, const void* k, int64_t ldk, void* out, int64_t ldo, int64_t M,
                   int64_t kv, int64_t head_dim, int row_calls, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------
 * Dense contractions
 * ------------------------------------------------------------------------------------- */

/* C[M,N] = A[M,K] · W[N,K]^T (+bias) (+GELU) (+residual)   — nn.Linear everywhere on the path
 * (modeling_llama_xformer.py:228-230,297,191; qwen_visual.py:191,259; resampler.py).
 * MFMA (bf16/f16: 16x16x32, f32: 16x16x4); lda/ldw/ldc/ldr in elements; K % 8 == 0. */
int ss_gemm(const void* A, const void* W, void* C, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldw,
            int64_t ldc, const void* bias, const void* residual, int64_t ldr, int epilogue, int dtype,
            void* stream);

/* Tile-configuration table of ss_gemm / ss_conv3x3 (16-bit dtypes, M > 128).  The best (tile, XCD group) of a shape
 * is data: ss_gemm / ss_conv3x3 only LOOK THE SHAPE UP (GEMM keys bucket M up to a multiple of 128) and otherwise use a
 * closed-form rule — they never time, allocate or synchronise, so they stay asynchronous and hipGraph-capturable.
 * Entries come from the two explicit tuning calls below or from ss_tune_import.
 *
 * ss_gemm_tune / ss_conv3x3_tune: time every candidate tile x tile order for one shape on `stream` with HIP events in
 * SUSTAINED mode (back-to-back launches over rotating weight copies that cycle through more than the Infinity Cache;
 * the way the kernel runs inside a forward), operands synthesised (pseudo-random) inside the caller's `workspace`
 * (>= *_tune_workspace_bytes), SYNCHRONISES, stores the winner in the table; *best_us_host (optional) receives its
 * time.  `epilogue` may carry SS_EPI_GELU / SS_EPI_GEGLU_PAIR (their arithmetic is timed; bias/residual are not).
 * ss_tune_lookup: out = {cfg, xcd_group} of the entry (returns 1 and out[0] = -1 when the shape has none).
 * ss_tune_export / ss_tune_import: the table as int32 records [n][10] = {dtype, M', N, K, conv_Cin,
 * 2*stride+upsample, conv_H, conv_W, cfg, xcd_group}; export returns the number of entries it holds. */
size_t ss_gemm_tune_workspace_bytes(int64_t M, int64_t N, int64_t K, int dtype);
int ss_gemm_tune(int64_t M, int64_t N, int64_t K, int epilogue, int dtype, void* workspace, size_t workspace_bytes,
                 void* stream, float* best_us_host);
size_t ss_conv3x3_tune_workspace_bytes(int64_t batch, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int64_t stride,
                                       int64_t upsample2x, int dtype);
int ss_conv3x3_tune(int64_t batch, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int64_t stride, int64_t upsample2x,
                    int dtype, void* workspace, size_t workspace_bytes, void* stream, float* best_us_host);
int ss_tune_lookup(int64_t M, int64_t N, int64_t K, int64_t conv_Cin, int64_t conv_H, int64_t conv_W, int64_t stride,
                   int64_t upsample2x, int dtype, int32_t out[2]);
int64_t ss_tune_export(int32_t* out, int64_t cap_entries);
int ss_tune_import(const int32_t* in, int64_t n_entries);
int ss_tune_clear(void);

/* y[N] = W[N,K] · x[K] — the batch-1 decode projection (weight streaming, HBM-bound).
 * Optional fused prologue: if norm_w != NULL, x is first RMS-normalised (as ss_rmsnorm).
 * Epilogues: SS_EPI_RESIDUAL (y = residual + round_T(acc)), SS_EPI_SILU_MUL (W is
 * [2N, K] = [gate; up], y[n] = silu(gate·x) * (up·x)), SS_EPI_BIAS.  K % 8 == 0. */
int ss_gemv(const void* W, const void* x, void* y, int64_t N, int64_t K, const void* norm_w, float eps,
            const void* bias, const void* residual, int epilogue, int dtype, void* stream);
/* The same projection for nb <= 4 rows at once (the lock-step decode of nb story slots):
 * x [nb, K], y / residual [nb, N] contiguous.  W is swept ONCE; every 16-byte weight pack is
 * dotted with all nb activation slices.  Row b equals ss_gemv on row b. */
int ss_gemv_batched(const void* W, const void* x, void* y, int64_t N, int64_t K, int64_t nb,
                    const void* norm_w, float eps, const void* bias, const void* residual, int epilogue,
                    int dtype, void* stream);
/* Host only (no GPU needed): which kernels the two calls above would launch for this shape under the current tuning knobs.
 * One row of SS_GEMV_PLAN_COLS ints per launch, in launch order: first sequence, sequence count, form (SS_GEMV_FORM_*),
 * NIT of the register form | k-steps per wave of the MFMA forms | 0, workgroups, threads per workgroup, dynamic LDS bytes,
 * non-temporal weight loads (0 / 1), SiLU pair (0 / 1), refused (1: gemm_f32_split asked for the split form and this launch is
 * an exact one instead).  has_norm: a norm_w would be passed; aligned16: W, x and norm_w are 16-byte aligned and the row stride
 * of x is a multiple of 4 elements (what the split form needs).  rows has room for max_rows rows (SS_GEMV_PLAN_MAX always
 * suffices).  Returns the number of launches, or a negative error code. */
#define SS_GEMV_PLAN_COLS 10
#define SS_GEMV_PLAN_MAX 16
enum { SS_GEMV_FORM_REG = 0, SS_GEMV_FORM_LDSX = 1, SS_GEMV_FORM_MFMA = 2, SS_GEMV_FORM_MFMA_EXACT16 = 3,
       SS_GEMV_FORM_MFMA_EXACT43 = 4, SS_GEMV_FORM_SPLIT_F32 = 5,
       SS_GEMV_FORM_W8 = 6, SS_GEMV_FORM_W8_EXACT16 = 7, SS_GEMV_FORM_W8_EXACT43 = 8 /* ss_gemv_w8 only */,
       SS_GEMV_FORM_MX4 = 9, SS_GEMV_FORM_MX4_EXACT16 = 10, SS_GEMV_FORM_MX4_EXACT43 = 11 /* ss_gemv_mx4 only */ };
int ss_gemv_plan(int64_t N, int64_t K, int64_t nb, int dtype, int epilogue, int has_norm, int aligned16, int32_t* rows,
                 int64_t max_rows);

/* The decode projection over fp8 weights (weight-only: activations and outputs stay in the 16-bit model dtype):
 *   y[b][n] = epilogue( w_scale[n] * sum_k dec(Wq[n][k]) * x[b][k] ),  b < nb <= 16
 * Wq [N, K] bytes of OCP e4m3fn in the 16-bit weights' row layout ([2N, K] = [gate; up] for SS_EPI_SILU_MUL, w_scale [2N]),
 * w_scale fp32, one per row of Wq (ops.quantize_weight_rows_fp8: amax / 448); x [nb, K], y / residual [nb, N] contiguous,
 * bias [N], norm_w [K] (RMSNorm prologue as ss_gemv) in `dtype` = SS_BF16 | SS_F16.  Every code is converted exactly to the
 * 16-bit type in registers and multiplied in the bf16 / f16 MFMA with fp32 accumulation; the scale is one fp32 multiply on the
 * finished sum, then the epilogue of ss_gemv (NONE, BIAS, RESIDUAL, BIAS | RESIDUAL, SILU_MUL alone).  Half the weight bytes
 * of ss_gemv_batched per call.  Shapes: K % 16 == 0 and K <= 4096, or K == 11008 (no norm_w there; 9..16 sequences run as two
 * sweeps); Wq, x and norm_w 16-byte aligned.  Anything else returns SS_EINVAL with a message before a launch.
 * ss_gemv_w8_plan: host only, the launches of that call as rows of ss_gemv_plan's layout (forms SS_GEMV_FORM_W8*; the
 * parameter column holds MFMA steps of 32 k per wave). */
int ss_gemv_w8(const void* Wq, const float* w_scale, const void* x, void* y, int64_t N, int64_t K, int64_t nb,
               const void* norm_w, float eps, const void* bias, const void* residual, int epilogue, int dtype, void* stream);
int ss_gemv_w8_plan(int64_t N, int64_t K, int64_t nb, int dtype, int epilogue, int has_norm, int32_t* rows, int64_t max_rows);

/* The decode projection over MXFP4 weights (OCP microscaling fp4, weight-only: activations and outputs stay in the 16-bit dtype):
 *   y[b][n] = epilogue( sum_k dec(code[n][k]) * 2^(scales[n][k / 32] - 127) * x[b][k] ),  b < nb <= 16
 * The format, for a weight W [N, K] with K % 32 == 0 ([2N, K] = [gate; up] for SS_EPI_SILU_MUL):
 *   codes   uint8 [N, K / 2] row-major: byte j of a row holds k = 2j in bits 0-3 and k = 2j + 1 in bits 4-7.  A code is sign
 *           (bit 3) and a magnitude index into {0, 0.5, 1, 1.5, 2, 3, 4, 6}: OCP e2m1, no Inf, no NaN.
 *   scales  uint8 [N, K / 32] row-major: byte b is e8m0, the 32 values k = 32 b .. 32 b + 31 are multiplied by 2^(byte - 127).
 * The exactness contract covers scale exponents X = byte - 127 in [-13, 13]: there every decoded value is a normal number of
 * bf16 and of fp16 and exact in both; it is decoded in registers (v_cvt_scalef32_pk_{bf16,f16}_fp4) and multiplied in the
 * bf16 / f16 MFMA with fp32 accumulation, every product exact in fp32; then the epilogue of ss_gemv (NONE, BIAS, RESIDUAL,
 * BIAS | RESIDUAL, SILU_MUL alone).  Outside that range the result is whatever the conversion instruction yields, never an
 * out-of-range access.  0.53 bytes per weight.  ss_quantize_rows_mxfp4 writes the format: per block, a = amax in fp32; the
 * block exponent X = exponent(a) - 2 when the fp32 mantissa field of a is <= 0x400000, else exponent(a) - 1, clamped to
 * [-13, 13] (an all-zero block: -13); codes = w / 2^X rounded to nearest on the e2m1 grid, ties to the even mantissa bit,
 * saturated at +-6; a value that rounds to zero gets code 0.  x [M, K] 16-bit with row stride ld (elements), 16-byte aligned.
 * Shapes of ss_gemv_mx4: K % 32 == 0 and K <= 4096, or K == 11008 (no norm_w there; 9..16 sequences run as two sweeps); codes,
 * x and norm_w 16-byte aligned.  Anything else returns SS_EINVAL with a message before a launch.
 * ss_gemv_mx4_plan: host only, the launches of that call as rows of ss_gemv_plan's layout (forms SS_GEMV_FORM_MX4*; the
 * parameter column holds MFMA steps of 32 k per wave, four per 16-byte load). */
int ss_gemv_mx4(const void* codes, const void* scales, const void* x, void* y, int64_t N, int64_t K, int64_t nb,
                const void* norm_w, float eps, const void* bias, const void* residual, int epilogue, int dtype, void* stream);
int ss_gemv_mx4_plan(int64_t N, int64_t K, int64_t nb, int dtype, int epilogue, int has_norm, int32_t* rows, int64_t max_rows);
int ss_quantize_rows_mxfp4(const void* x, int64_t ld, int64_t M, int64_t K, void* codes_out, void* scales_out, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------
 * Sampling: lm_head logits -> AutoImageTokenGenerationProcessor -> greedy argmax
 * ------------------------------------------------------------------------------------- */

/* src/models_clm/generation.py:19-31 + HF greedy argmax, on device:
 * logits [vocab] (T, modified in place like the reference does), last_id = *last_id_dev,
 * img_ids int32[n_img_ids] = ids of <img><img_00000>…</img>.  If last_id is one of
 * img_ids[:-1] the successor's score becomes max+10, else scores[img_ids[1:]] = 0.0;
 * then the first maximal index is written to *token_out_dev. */
int ss_imgproc_argmax(void* logits, int64_t vocab, const int32_t* last_id_dev, const int32_t* img_ids,
                      int64_t n_img_ids, int32_t* token_out_dev, int dtype, void* stream);

/* Sampling in the arg max's place: processor edit -> temperature -> top-k -> top-p -> one draw (Hugging Face's order; this
 * definition, in fp32, is what is implemented — not the library's arithmetic in the model dtype).
 *   z        the logits in the model dtype after the processor's in-place edit above.
 *   successor  last id in img_ids[:-1]: the successor is the token, with certainty, and no draw is consumed.  DEVIATION: the
 *            reference's processor only makes it overwhelmingly likely (max + 10); the engine's image-token block already
 *            treats those 65 tokens as forced.
 *   top-k    top_k > 0: keep i iff z_i >= the k-th largest z; ties are all kept (TopKLogitsWarper).  0 = off.
 *   weights  w_i = exp((z_i - z_max) / temperature) over the top-k set, fp32; Z_k = sum w.
 *   top-p    keep i iff A_i < top_p * Z_k, A_i = sum{ w_j : z_j > z_i }, the mass strictly above z_i: the arg max is always
 *            kept, top_p = 1 keeps the whole top-k set.  DEVIATION: equal to TopPLogitsWarper except that tied values are
 *            kept or dropped together, and in rounding when a cumulative mass meets top_p * Z_k to ~1e-5.
 *   draw     u in [0, 1), t = u * Z_P (the kept mass); token = the first kept index, ascending, whose inclusive cumulative
 *            weight exceeds t; fallback: the last kept index.
 *   NaN and -inf entries are never kept; a row with nothing else gives token 0 (n_kept 0), like the greedy kernel's guard.
 *   u        Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; Weyl 0x9E3779B9, 0xBB67AE85), key = the seed as (lo, hi),
 *            counter = (draw, lane, 0, 0), u = (out0 >> 8) * 2^-24.
 * Every mass is summed in one fixed order and there are no atomics: the same seed gives the same tokens on every run.
 * temperature finite and > 0, 0 < top_p <= 1, top_k >= 0: SS_EINVAL otherwise, before any launch. */
typedef struct ss_sampling {
    float temperature;
    float top_p;
    int32_t top_k;
    uint64_t seed;
} ss_sampling;

/* The sampler on rows of logits [rows][ld] (vocab <= 65535 entries each, model dtype), one token per row to
 * token_out_dev[rows].  u_dev non-NULL: one u per row (clamped to [0, 1)); NULL: Philox with counter (draw0, row).
 * last_ids_dev int32[rows] + img_ids (device, as in ss_imgproc_argmax), both optional: with both, the processor runs first
 * and edits the row in place; otherwise the rows are only read.  n_kept_out_dev (optional) int32[rows]: the size of the final
 * kept set, or 1 on the certain-successor path. */
int ss_sample_logits(void* logits, int64_t rows, int64_t vocab, int64_t ld, const ss_sampling* p, const float* u_dev,
                     uint32_t draw0, const int32_t* last_ids_dev, const int32_t* img_ids, int64_t n_img_ids,
                     int32_t* token_out_dev, int32_t* n_kept_out_dev, int dtype, void* stream);

/* Hugging Face's three history rules, applied to a logits row IN FRONT of the image-token processor, in the order of HF's
 * processor list: repetition penalty -> no-repeat n-gram -> min_new_tokens -> processor -> arg max or sampler.
 *   hist     the slot's token history: the ids the caller handed over (the whole running input_ids) followed by every token
 *            the decode loop has appended since; prompt_len = its length at hand-over.  z = the row in the model dtype T.
 *   1. repetition_penalty p (finite, > 0; 1 = off): for every id that occurs in hist, ONCE however often it occurs,
 *            z_i <- round_T(z_i < 0 ? z_i * p : z_i / p), computed in fp32 with p at its float32 value, a correctly rounded
 *            IEEE division and one rounding to T (bit-equal to RepetitionPenaltyLogitsProcessor in bf16, fp16 and fp32).
 *            NaN stays NaN (the entry is not rewritten); +-inf follow the formula.
 *   2. no_repeat_ngram n (0 = off, 1 <= n <= SS_LOGITS_RULES_MAX_NGRAM): when len(hist) + 1 >= n, every id that has followed
 *            an earlier occurrence of the last n - 1 ids of hist gets -inf; n = 1 bans every id of hist.
 *   3. min_new_tokens m (0 = off): while len(hist) - prompt_len < m the EOS id gets -inf.  The second stop id of
 *            ss_llama_set_stop_id is not EOS and is left alone.
 *   spare_img_ids (DEVIATION from Hugging Face, off by default): non-zero exempts the ids of img_ids from rule 1 only — a
 *            story prompt carries earlier images' <img> ... </img> tokens, and the literal penalty would talk the model out
 *            of producing images.
 * -inf entries are never the arg max unless nothing else is left, and the sampler never keeps them.  No atomics: membership
 * for rule 1 is a bitmap of ceil(vocab / 32) words in which every word has one owner thread.
 * SS_EINVAL before any launch: p <= 0 or not finite, n < 0 or above the cap, m < 0. */
#define SS_LOGITS_RULES_MAX_NGRAM 8
typedef struct ss_logits_rules {
    float repetition_penalty;
    int32_t no_repeat_ngram;
    int32_t min_new_tokens;
    int32_t spare_img_ids;
} ss_logits_rules;

/* The three rules on caller-owned rows logits [rows][ld] (vocab <= 65535 entries each, model dtype), edited in place; the
 * processor does not run.  Row r's history is hist_dev[r * hist_ld .. + hist_len_dev[r]) (int32, device; the length is
 * clamped to [0, hist_ld]); prompt_len_dev int32[rows] (NULL = 0 for every row).  The history is device memory, so an id
 * outside [0, vocab) cannot be refused: it is skipped and never used as an index.  eos_id < 0 = none.  img_ids (device,
 * n_img_ids <= 1024) is read only with spare_img_ids. */
int ss_process_logits(void* logits, int64_t rows, int64_t vocab, int64_t ld, const ss_logits_rules* rules,
                      const int32_t* hist_dev, int64_t hist_ld, const int32_t* hist_len_dev, const int32_t* prompt_len_dev,
                      int32_t eos_id, const int32_t* img_ids, int64_t n_img_ids, int dtype, void* stream);

/* Token log-probabilities: how likely was the token that was chosen, and what would the model have said instead.
 * For the decode token that produces gen_ids[n] of a slot, raw = the lm_head row in the model dtype before anything edits it,
 * z = the row after the slot's history rules (if on) and the image-token processor's in-place edit.  All arithmetic is fp32;
 * every sum is taken in one fixed order (per thread in index order, xor butterfly over the wave, xor butterfly over the 16
 * wave sums) and there are no atomics: a row gives the same bits on every run.
 *   lsm(x)[t]      = (x_t - x_max) - log sum_i exp(x_i - x_max), the log-softmax at temperature 1 over the whole vocabulary.
 *                  NaN and -inf entries carry no mass, as in the sampler; x_max is taken over the others.  x_t = -inf gives
 *                  -inf and x_t = NaN gives NaN (by the entry alone, never a NaN made by the arithmetic: a row without any
 *                  mass gives -inf / NaN as well).  A row whose maximum is +inf is outside the definition.
 *   model_logprob[n] = lsm(raw)[tok]: the model's own score of the token.
 *   logprob[n]     the log of the probability with which the engine's policy picked tok:
 *                  greedy slot    lsm(z)[tok] (for a free token: Hugging Face's compute_transition_scores(...,
 *                                 normalize_logits=True) of a greedy run);
 *                  sampling slot  log(w_tok / Z_P) = (z_tok - z_max) / temperature - log Z_P, with w, the kept set and Z_P
 *                                 exactly as ss_sample_logits defines them; in the decode loop it is computed by the sampling
 *                                 kernel from the kept set and the Z_P of the draw itself; -inf for a token outside the set;
 *                  0.0            for a token the policy did not choose: an entry of forced_tokens (even one that z bans), and
 *                                 the certain image-token successor.  DEVIATION: the successor rule is the one ss_sample_logits
 *                                 declares for sampling, extended to greedy slots (the reference's processor only makes the
 *                                 successor overwhelmingly likely).
 *   top_ids[n][0 .. top_n), top_logprobs[n][0 .. top_n)   the top_n largest entries of raw with their model_logprob values, in
 *                  descending order, equal values by ascending id; 0 <= top_n <= 8; when fewer than top_n entries carry mass
 *                  the remaining places hold id -1 and -inf.
 * Recording changes nothing else: the tokens, the hidden rows, the final logits row and the Philox draw counter are
 * bit-equal to a run without it.
 *
 * ss_token_logprobs: the operator on caller-owned rows logits [rows][ld] (vocab <= 65535 entries each, model dtype), which it
 * only reads; one block per row, one pass over the row.  p = NULL: lp_out[r] = lsm(row r)[ids_dev[r]].  p non-NULL:
 * lp_out[r] = the sampler's log(w / Z_P) of ids_dev[r] on row r (the processor does not run: hand it z).  top_n > 0:
 * top_ids_out / top_lp_out [rows][top_n] as defined above, from lsm(row r) in either form.  An id outside [0, vocab) is never
 * used as an index: NaN (p = NULL) or -inf.  SS_EINVAL before any launch: a bad shape, top_n outside [0, 8], top_n > 0
 * without both top-n buffers, a sampling parameter outside its range. */
int ss_token_logprobs(const void* logits, int64_t rows, int64_t vocab, int64_t ld, const int32_t* ids_dev, const ss_sampling* p,
                      int32_t top_n, float* lp_out, int32_t* top_ids_out, float* top_lp_out, int dtype, void* stream);

/* Beam search, one step of the selection (the search itself: ss_llama_beam_search below).
 * Row b of logits [rows][ld] (vocab <= 65535 entries each, model dtype; only read) is the edited row z of running hypothesis b,
 * beam_scores[b] (device, fp32) its accumulated score; a score of -inf marks a dead row, which offers nothing (step 0 of a
 * search is the vector [0, -inf, ...]).  The candidates are  beam_scores[b] + lsm(z_b)[t]  over every live row b and every
 * token t that carries mass (lsm, NaN and -inf as ss_token_logprobs defines them; fp32, fixed summation order, no atomics).
 * Written (device): the K = max(2, 1 + n_stop) * rows best, descending, equal scores by ascending b * vocab + t — Hugging Face
 * leaves ties to torch.topk, this operator does not: cand_score / cand_beam / cand_token [K]; where fewer than K candidates
 * exist the remaining places hold -inf / -1 / -1.  stop_ids (host, n_stop <= 2 ids inside [0, vocab)) only set K here: which
 * candidates are finished is the caller's bookkeeping.  rows <= SS_BEAM_MAX.  One block: the rows one after the other, their
 * lists in LDS, then the merge.  SS_EINVAL before any launch: a NULL pointer, a bad shape, n_stop outside [0, 2], a stop id
 * outside the row. */
#define SS_BEAM_MAX 8
int ss_beam_step(const void* logits, int64_t rows, int64_t vocab, int64_t ld, const float* beam_scores_dev, int32_t n_stop,
                 const int32_t* stop_ids, float* cand_score_out, int32_t* cand_beam_out, int32_t* cand_token_out, int dtype,
                 void* stream);

/* ---------------------------------------------------------------------------------------
 * LLaMA decoder engine (native runtime: KV cache, prefill loop, hipGraph-captured decode)
 * ------------------------------------------------------------------------------------- */

typedef struct ss_llama ss_llama;

typedef struct ss_llama_config {
    int32_t hidden, n_heads, n_layers, inter, vocab, max_pos; /* LlamaConfig */
    float rms_eps;
    int32_t dtype;
    int32_t cache_cap;   /* KV slots per head */
    int32_t max_new;     /* capacity of the generated-token / hidden-state ring */
    int32_t n_img_ids;   /* 66 for SEED-Story */
    int32_t eos_id;
    int32_t n_seq;       /* sequence slots (independent stories decoded in lock-step, sharing one
                            sweep of the weights per token); 0 or 1 = the reference's batch-1 loop */
} ss_llama_config;

/* Per-layer weights, all [out, in] row-major in the model dtype, LoRA already merged
 * (or absent): wqkv [3*hidden, hidden] = [q;k;v], wo [hidden, hidden],
 * wgu [2*inter, hidden] = [gate; up], wdown [hidden, inter], ln1, ln2 [hidden]. */
typedef struct ss_llama_layer_weights {
    const void *wqkv, *wo, *wgu, *wdown, *ln1, *ln2;
} ss_llama_layer_weights;

typedef struct ss_llama_weights {
    const void* embed;    /* [vocab, hidden] */
    const void* lm_head;  /* [vocab, hidden] */
    const void* final_norm;
    const void* rope_cos; /* [max_pos, hd] model dtype (LlamaRotaryEmbedding, :118-134) */
    const void* rope_sin;
    const ss_llama_layer_weights* layers; /* host array[n_layers] */
} ss_llama_weights;

/* Bytes of device memory the engine needs (KV cache + activations); the caller allocates it
 * (torch) and hands it over in ss_llama_create — the engine never calls hipMalloc for it. */
size_t ss_llama_workspace_bytes(const ss_llama_config* cfg, int64_t max_prefill_rows);
int ss_llama_create(const ss_llama_config* cfg, const ss_llama_weights* w, void* workspace,
                    size_t workspace_bytes, int64_t max_prefill_rows, const int32_t* host_img_ids,
                    ss_llama** out);
void ss_llama_destroy(ss_llama* h);

/* Select the sequence slot (0 <= seq < n_seq) that ss_llama_buffer / set_lengths / get_lengths /
 * kv_gather / prefill / generate address.  Slots have private KV caches, logits, token and hidden
 * rings; they share the weights and the activation scratch.  Default slot 0. */
int ss_llama_select(ss_llama* h, int32_t seq);
/* Optional second stop token of the decode loop (besides EOS and the token limit): generation ends right AFTER producing
 * `token_id` (it is in the generated ids, not yet fed).  -1 = none (default).  Used to stop at `<img>`: the 64
 * `<img_000NN>` tokens + `</img>` that follow are forced by the logits processor (generation.py:19-31), so the host
 * feeds them as ONE batched continuation (ss_llama_prefill, weights streamed once for 66 rows instead of 66 times) and
 * resumes the loop from its logits.  Applies to every sequence slot.  Range: -1 <= token_id < min(vocab, 32766) — the
 * loop's stop word holds EOS in 16 bits and this id + 1 in the 15 bits above; ss_llama_create therefore requires
 * vocab <= 65535 and eos_id < 65535 (LLaMA-2 + 66 added tokens: 32066). */
int ss_llama_set_stop_id(ss_llama* h, int32_t token_id);

/* Attention-map capture (the reference's `config.output_attentions`: one map per decoder layer, head `head`, the values
 * ss_attn_scores documents).  maps = device memory [n_layers][n_rows][ld] in the model dtype, owned AND PRE-FILLED by the
 * caller (NaN reproduces the reference's merged maps; the engine never clears it); buffer row r belongs to the query whose
 * key sits at cache index row0 + r.  While capture is on,
 *   ss_llama_prefill   writes its M rows x (kv_len + M) columns per layer; row_calls = 1 makes every multi-row prefill
 *                      write each row as its own one-row call (the image-token block, which the reference feeds one
 *                      token at a time); SS_EINVAL before anything is launched when the rows or columns do not fit;
 *   ss_llama_generate  writes one row per decode token from inside the token (eager or captured; the captured graph has
 *                      one more node per layer and is cached apart from the shipped one; it reads the buffer from a device
 *                      descriptor, so changing buffers does not re-capture); kv_len + n_steps must fit, SS_EINVAL otherwise;
 *   ss_llama_prefill_batch / ss_llama_generate_batch  refuse (SS_EINVAL): maps are a single-sequence tool — an n_seq > 1
 *                      engine captures through the single-sequence entry points on the selected slot.
 * maps = NULL turns capture off (the default): the decode token then launches exactly what it launched before.  Call it
 * between engine calls, not while one is in flight (it updates the descriptor with a blocking copy). */
int ss_llama_set_attn_capture(ss_llama* h, void* maps, int64_t n_rows, int64_t ld, int64_t row0, int32_t head,
                              int32_t row_calls);

/* Sampling in the decode loop (definition: ss_sample_logits).  seq = a slot, or -1 for all; p = NULL = greedy (the default).
 * The parameters, the seed and a per-slot draw counter live in device memory: ss_llama_generate / ss_llama_generate_batch
 * (eager or captured) then open each token with the sampling kernel, which draws Philox (draw, slot) for a slot with sampling
 * on and takes the arg max for one with it off (mixed batches work); changing temperature or seed does not re-capture.  A
 * forced token and the certain image-token successor consume no draw; only a real draw advances the counter, which persists
 * across generate calls (so the image-token block path and the token-by-token loop give the same sequence) and is reset to 0
 * by this call.  The captured sampling graph is cached apart from the greedy one; with every addressed slot greedy the decode
 * token launches exactly what it launched before.  Works with attention-map capture and fp8 decode weights.  Call it between
 * engine calls (blocking copy).  SS_EINVAL: a parameter outside its range (ss_sampling), or a bad slot. */
int ss_llama_set_sampling(ss_llama* h, int32_t seq, const ss_sampling* p);

/* The history rules in the decode loop (definition: ss_process_logits).  seq = a slot, or -1 for all; rules = NULL = off (the
 * default).  While a slot has rules on, every decode token of ss_llama_generate / ss_llama_generate_batch (eager or captured)
 * opens with one more kernel, which appends the slot's previous token to its history and edits its logits row before the
 * opening kernel (greedy or sampling, unchanged) reads it; a slot with rules off is skipped by it (mixed batches work), and
 * with every addressed slot off the decode token launches exactly what it launched before.  The rules, the history
 * int32[cache_cap + max_new], its length, prompt_len and the rule-1 bitmap live in device memory: changing them does not
 * re-capture, and the captured rules graph is cached apart from the others.  EOS is the engine's eos_id.  Works with
 * sampling, attention-map capture and fp8 decode weights.  A generate call on a rules-on slot whose history could outgrow
 * the buffer is refused (SS_EINVAL).  Call it between engine calls (blocking copy). */
int ss_llama_set_logits_rules(ss_llama* h, int32_t seq, const ss_logits_rules* rules);

/* Token log-probabilities in the decode loop (definition: ss_token_logprobs).  seq = a slot, or -1 for all; every buffer NULL =
 * off (the default).  The buffers are device memory owned by the caller and kept alive while the option is on, per slot
 * model_lp, policy_lp float[max_new] and, for top_n > 0, top_ids int32 / top_lp float [max_new][top_n]; with seq = -1 they
 * hold n_seq such blocks, slot-major.  While a slot records, every decode token of ss_llama_generate /
 * ss_llama_generate_batch (eager or captured) runs two more small kernels: one in front of the rules kernel, which reads raw
 * (statistics, the top-n, a scratch copy of the row), and one behind the opening kernel, which writes entry n = the index of
 * the token in gen_ids; with sampling on, the sampling kernel's sibling also hands over log(w_tok / Z_P) of its draw.  A done
 * slot writes nothing, a slot with the option off writes nothing (mixed batches work), and with every addressed slot off the
 * decode token launches exactly what it launched before.  The buffers are reached through a descriptor in device memory:
 * other buffers or another top_n do not re-capture, and the captured graph is cached apart from the others.  Works with
 * sampling, the history rules, attention-map capture, fp8 decode weights and the fp8 KV shadow.  Call it between engine
 * calls (blocking copy).  SS_EINVAL before anything is written: top_n outside [0, 8], a bad slot, or some but not all of the
 * buffers NULL (model_lp and policy_lp always; top_ids and top_lp exactly when top_n > 0). */
int ss_llama_set_logprobs(ss_llama* h, int32_t seq, float* model_lp, float* policy_lp, int32_t* top_ids, float* top_lp,
                          int32_t top_n);

/* Hands slot seq's history over (seq = -1: the selected slot).  append = 0: the history becomes host_ids[0 .. n) and
 * prompt_len = n (n = 0 empties it); append = 1: host_ids are added behind it — tokens that were fed outside the decode loop
 * (the batched image-token block) — and prompt_len stays.  The history advances by itself only while the slot has rules on.
 * SS_EINVAL before anything is copied: an id outside [0, vocab), or more ids than the buffer holds.  Blocking; call it
 * between engine calls. */
int ss_llama_set_history(ss_llama* h, int32_t seq, const int32_t* host_ids, int64_t n, int32_t append);

/* fp8 (OCP e4m3fn) weight-only decode.  Per layer: the four byte planes in the 16-bit weights' layouts (wqkv [3*hidden, hidden],
 * wo [hidden, hidden], wgu [2*inter, hidden] = [gate; up], wdown [hidden, inter]) and one fp32 scale per row of each
 * (s_qkv [3*hidden], s_o [hidden], s_gu [2*inter], s_down [hidden]); lm_head_q [vocab, hidden] bytes + lm_head_scale [vocab].
 * Device memory owned by the caller and kept alive while the option is on; `layers` is a host array[n_layers] (copied).
 * While it is set, the five decode projections of ss_llama_generate / ss_llama_generate_batch (and of
 * ss_llama_profile_decode) run ss_gemv_w8 on these planes: eager or captured, with attention-map capture too; half the
 * weight bytes per generated token.  ss_llama_prefill*, the one-row lm_head at the end of a prefill and the image-token block
 * keep the 16-bit weights, which therefore stay resident.  layers = NULL turns it off (the default).  Call it between
 * engine calls; the captured fp8 decode graph is cached apart from the 16-bit one and dropped when the planes change.
 * SS_EINVAL: an fp32 engine, or a projection shape ss_gemv_w8 does not take (hidden / inter not a multiple of 16, wider than
 * 4096 and not 11008, ...), a NULL or misaligned plane. */
typedef struct ss_llama_layer_w8 {
    const void *wqkv, *wo, *wgu, *wdown;
    const float *s_qkv, *s_o, *s_gu, *s_down;
} ss_llama_layer_w8;
int ss_llama_set_decode_w8(ss_llama* h, const ss_llama_layer_w8* layers, const void* lm_head_q, const float* lm_head_scale);

/* MXFP4 weight-only decode: ss_llama_set_decode_w8 with planes in the format of ss_gemv_mx4.  Per layer the four code planes
 * ([rows, K / 2] bytes over the 16-bit weights' layouts) and the four scale planes ([rows, K / 32] bytes); lm_head_codes
 * [vocab, hidden / 2] + lm_head_scales [vocab, hidden / 32].  The same ownership, scope (decode tokens only: prefill, the
 * one-row lm_head at its end and the image-token block keep the 16-bit weights, which stay resident) and graph caching as the
 * fp8 option; the two exclude each other: setting one clears the other.  layers = NULL turns it off.  A quarter of the
 * weight bytes per generated token plus one scale byte per 32 weights.  SS_EINVAL: an fp32 engine, a projection shape
 * ss_gemv_mx4 does not take (hidden / inter not a multiple of 32, wider than 4096 and not 11008), a NULL plane, a code plane
 * that is not 16-byte aligned.  End quality on real checkpoints has not been measured. */
typedef struct ss_llama_layer_mx4 {
    const void *wqkv, *wo, *wgu, *wdown;            /* codes */
    const void *s_qkv, *s_o, *s_gu, *s_down;        /* e8m0 scales */
} ss_llama_layer_mx4;
int ss_llama_set_decode_mx4(ss_llama* h, const ss_llama_layer_mx4* layers, const void* lm_head_codes, const void* lm_head_scales);

/* fp8 (e4m3) KV shadow cache for decode attention (the quantisation: ss_kv_quantize_fp8).  k_codes, v_codes
 * [n_seq][n_layers][n_heads][cache_cap][hd] bytes and k_scale, v_scale [n_seq][n_layers][n_heads][cache_cap] fp32: device
 * memory owned by the caller and kept alive while the option is on (sizes: ss_llama_kv8_bytes; ss_llama_workspace_bytes does
 * not change).  All four NULL = off (the default): the decode token then launches exactly what it launched before.
 * While it is on, the attention of every decode token of ss_llama_generate / ss_llama_generate_batch / ss_llama_profile_decode
 * (eager or captured; the captured graph is cached apart and dropped when the planes change) reads keys and values from the
 * shadow — half the KV bytes per token — and its fused append writes the new row to the 16-bit cache, as before, AND to the
 * shadow.  The new token's own k / v are used unquantised.
 * The 16-bit cache stays the truth and everything else keeps using it unchanged: ss_llama_prefill*, the image-token block,
 * ss_llama_buffer's views, ss_llama_kv_gather, attention-map capture.  The option therefore COSTS memory: hd + 4 bytes per
 * (slot, layer, head, position) on top (LLaMA-7B: 0.27 MB per position per slot, 0.31 GB per slot at cache_cap 1152).
 * Attention-map capture keeps computing its decode rows from the 16-bit keys: with the option on, the maps show the 16-bit
 * scores, not the ones the token used.
 * Each slot has a host-side watermark: shadow rows below it equal the quantiser applied to the 16-bit rows.  The three
 * decode entry points start with one launch that quantises the rows [watermark, kv_len) of their slots, whoever wrote them.
 * ss_llama_set_lengths lowers the watermark to min(watermark, kv_len), ss_llama_kv_gather to 0; a caller that writes cache
 * rows through ss_llama_buffer's views calls ss_llama_kv8_invalidate(h, first row written) for the selected slot.
 * Works with fp8 decode weights, sampling and the history rules.  Call these between engine calls.
 * SS_EINVAL: an fp32 engine, a head dim ss_attn_decode_kv8 does not take, some but not all planes NULL, a misaligned plane. */
int ss_llama_kv8_bytes(const ss_llama_config* cfg, size_t* codes_bytes, size_t* scales_bytes);    /* per plane, all slots */
int ss_llama_set_kv8(ss_llama* h, void* k_codes, void* v_codes, float* k_scale, float* v_scale);
int ss_llama_kv8_invalidate(ss_llama* h, int64_t from_row);

/* Device pointers into the engine's workspace (views for the Python side), for the selected slot:
 * which: 0 = K cache [n_layers, n_heads, cache_cap, hd], 1 = V cache (same shape),
 * 2 = generated ids int32[max_new], 3 = hidden rows [max_new, hidden] (post final norm,
 * row j = state whose input token was generated id j; models.py:182-184),
 * 4 = last-token logits [vocab], 5 = state int32[8] {kv_len,pos,n_gen,done,last_id,…},
 * 6 = token history int32[cache_cap + max_new] (ss_llama_set_history), 7 = its rule-1 bitmap uint32[ceil(vocab / 32)]. */
void* ss_llama_buffer(ss_llama* h, int which);

/* Set / get the live KV length and next rope position (host view).  Truncating the cache
 * (vis_george_sink.py:243) is ss_llama_set_lengths(h, new_len, new_pos). */
int ss_llama_set_lengths(ss_llama* h, int64_t kv_len, int64_t pos, void* stream);
int ss_llama_get_lengths(ss_llama* h, int64_t* kv_len, int64_t* pos);
/* KV re-pack for the multimodal attention sink (vis_george_sink.py:266-295): new cache =
 * old cache gathered at keep_idx[0..n_keep) (device int32, ascending), kv_len = n_keep. */
int ss_llama_kv_gather(ss_llama* h, const int32_t* keep_idx_dev, int64_t n_keep, void* stream);

/* Slot fork: after it each of the n_dst slots of host_dst (host array, at most n_seq - 1 = 7 entries) is in the state slot
 * src is in, so that ss_llama_generate / ss_llama_generate_batch / ss_llama_prefill* on a destination behave as on src —
 * n sampled continuations of one prompt cost one prefill, not n.
 * Copied: K and V rows [0, kv_len[src]) of every layer and head (rows at and above kv_len of a destination are not touched),
 * the last-token logits row, the state words kv_len / pos / last_id, the token history with its length, prompt_len and the
 * rule-1 bitmap (rules on or off: they are small) and, with the fp8 KV shadow on, its codes and scales below
 * min(watermark[src], kv_len[src]); the destinations' watermarks are set to that.  The host views of kv_len, pos and the
 * history length follow.
 * Not copied, because they belong to the slot: the sampling parameters and the draw counter (slots given one seed diverge
 * because the slot is part of the Philox counter), the rule parameters and on/off flags, the log-probability descriptor,
 * attention capture, the generated-id and hidden-row rings, the forced-token buffer.
 * One kernel per plane kind, over (K|V plane, layer, head, row chunk): each 16-byte packet of the source is loaded once and
 * stored to every destination (the list travels by value); one more small launch moves the per-slot pieces.  Asynchronous on
 * `stream`: no host synchronisation, no allocation.  kv_len[src] == 0 is legal (the state alone is copied).
 * SS_EINVAL before anything is launched or any host view changes: h or host_dst NULL, src outside [0, n_seq), n_dst < 1, a
 * destination out of range, equal to src, or listed twice. */
int ss_llama_fork(ss_llama* h, int32_t src, const int32_t* host_dst, int32_t n_dst, void* stream);

/* Beam search over forked slots, on the device inside the captured decode token.
 * The prompt is on slot 0 (prefilled, its last-token logits in place).  The call forks slot 0 to slots 1 .. n-1
 * (ss_llama_fork), then runs the decode loop on slots [0, n) with the token opened by three kernels instead of the arg max:
 *   [logits_rules]  each slot's history rules, when on (they must be on for all n slots or for none)
 *   beam_topk       one block per slot: image-token processor edit, then the K best of  running score + lsm(z)  (ss_beam_step)
 *   beam_advance    one block: merge to the K best overall, the update below, parent[n] / token[n], the slots' generated ids,
 *                   last-id / n-generated words and embedding rows; the done word of every slot once the search is over
 *   beam_permute    K and V rows [kv0, kv_len) of every layer and head follow parent[] (kv0 = the cache length at the start:
 *                   the shared prompt below it never moves); one thread per 16-byte packet position across the n slots loads
 *                   from every parent, then stores to every slot whose parent is another slot, so cycles and fan-out are safe
 *                   in one launch; an all-identity parent[] stores nothing.  With rules on, the history suffix and the rule-1
 *                   bitmap follow in one more small launch.
 * then the layers and lm_head, unchanged.  One graph per (n, n_steps, workspace).
 * Definition (Hugging Face transformers 5.x GenerationMixin._beam_search and its helpers, one batch item): the running
 * scores start as [0, dead ...]; per step t = 0, 1, ... the K = max(2, 1 + stop ids) * n best candidates are taken (stop ids:
 * the engine's eos_id and the id of ss_llama_set_stop_id); a candidate whose token is a stop id, or with t + 1 >= n_steps, is
 * finished; the n best unfinished ones run on; the finished ones among the first n enter the finished table with score
 * sum / (t + 1) ** length_penalty, which keeps its n best, sorted (equal scores: the older entry first); once the table is
 * full the sticky heuristic  best running sum / hyp ** length_penalty > worst table score  (hyp = t + 1, or n_steps for
 * early_stopping "never" with length_penalty > 0) must hold for the search to go on; it also ends when the table is full and
 * early_stopping is True, when every candidate of the step was finished, or when no hypothesis is left running.
 * DEVIATION from Hugging Face: the row scores are the log-softmax of the row AFTER the history rules and the image-token
 * processor; HF hands its processors the log-softmax row, on which the image-token processor's `scores[ids] = 0.0` would
 * turn 65 ids into probability 1 — the reference's own num_beams > 1 cannot work, so there is nothing to be compatible with.
 * NaN and -inf entries offer no candidate.
 * ss_beam_state is the head of the caller-owned workspace of ss_llama_beam_bytes() bytes (device memory, 16-byte aligned, owned
 * as the planes of ss_llama_set_kv8 are); it is readable after the call: fin_* sorted best first, the sequences behind it as
 * int32 [2][n][max_new] running | [2][n][max_new] finished at byte offset ss_llama_beam_seq_offset(), buffer (step & 1) current.
 * Afterwards slots [0, n) hold the running hypotheses' caches; the caller puts the slot it goes on with back in shape
 * (ss_llama_set_lengths + ss_llama_prefill of the winner).
 * SS_EINVAL before any launch or state change: num_beams outside [1, min(n_seq, 8)], a selected slot other than 0, the fp8 KV
 * shadow on (permuting the shadow is not built), attention capture on, log-probability recording or sampling on for a slot
 * of the group, rules on for only some of them, n_steps outside [1, max_new], a non-finite length_penalty, early_stopping
 * outside 0..2, a cache, position or history overflow. */
typedef struct ss_beam_params {
    int32_t num_beams;
    float length_penalty;
    int32_t early_stopping;     /* 0 False, 1 True, 2 "never" */
} ss_beam_params;
typedef struct ss_beam_state {
    int32_t n, K, n_stop, stop_ids[2], limit, max_new, early_stopping;
    float length_penalty;
    int32_t kv0, hist0, step, unsat, ended, pad[2];
    float run_score[SS_BEAM_MAX];       /* running hypotheses: accumulated score, live flag */
    int32_t run_live[SS_BEAM_MAX];
    float fin_score[SS_BEAM_MAX];       /* finished table, best first: score, length, valid flag */
    int32_t fin_len[SS_BEAM_MAX], fin_flag[SS_BEAM_MAX];
    int32_t parent[SS_BEAM_MAX], token[SS_BEAM_MAX];    /* of the last step */
} ss_beam_state;
size_t ss_llama_beam_bytes(const ss_llama_config* cfg, int32_t num_beams);
size_t ss_llama_beam_seq_offset(void);
int ss_llama_beam_search(ss_llama* h, const ss_beam_params* p, void* beam_ws, int64_t n_steps, int32_t last_prompt_id,
                         void* stream);
/* test hook: one beam_permute (+ the history launch when rules are on for slot 0) of slots [0, n) with parent[] (host) over the
 * cache rows [kv0, kv_len of slot 0) and history entries [hist0, history length of slot 0), through `beam_ws`.  Same refusals. */
int ss_llama_beam_permute(ss_llama* h, void* beam_ws, const int32_t* host_parent, int32_t n, int64_t kv0, int64_t hist0,
                          void* stream);

/* Prompt-lookup speculative decoding of ONE slot's greedy loop (off by default; ss_llama_generate only).
 *
 * A speculative step forwards R <= 8 rows of the selected slot in one sweep of the weights: row 0 carries the token greedy just
 * chose, rows 1 .. A-1 drafted successors at the following cache / RoPE positions.  The next step's opening kernel walks the R
 * logits rows: row r's arg max (image-token processor applied with row r's own token as predecessor, forced tokens first) is the
 * token greedy would emit after row r's token; while it equals draft r + 1 the draft is emitted under greedy's stop rules, the
 * first one that differs becomes row 0 of the next step.  Rejected rows' K/V and hidden rows lie beyond kv_len / n_generated and
 * are overwritten.  The emitted ids are greedy's by construction wherever the R-row and the 1-row kernels agree on the arg max
 * (they order their sums differently: equality holds away from near-ties).
 *
 *   spec_open         one block: settle the previous step, emit, append to the slot's token history, draft, write the R row-state
 *                     blocks (kv_len = L + r, pos = P + r, done = row unused), embed the rows
 *   per layer         the batched GEMVs at nb = R over the row-state blocks; ss_attn_decode_spec in the attention's place
 *   spec_final_norm   hidden row n_generated_base + r per used row, then the lm_head GEMV -> R logits rows
 *
 * Draft sources.  SS_SPEC_LOOKUP: transformers' PromptLookupCandidateGenerator.get_candidates on the slot's history (the ids
 * handed over with ss_llama_set_history plus everything generated, the token just chosen included): n-gram sizes from
 * min(max_ngram, len - 1) down to 1, the leftmost match with a non-empty continuation, at most R - 1 tokens, cut in front of the
 * first stop id (EOS / the second stop id); an empty cut gives no draft.  SS_SPEC_GIVEN: draft r of a step whose row 0 is
 * generated index n is given_ids[n + r] (device int32[given_len]); cut in front of a stop id or an id outside the vocabulary.
 * Either source: while generated indices lie below n_forced the drafts are the forced tokens themselves.  A row is never used
 * beyond the call's limit (the last token of a call needs no forward), max_new, cache_cap or max_pos; without a draft the step is
 * a plain token.
 *
 * ss_attn_decode_spec — the attention of such a step as an operator.  qkv: `rows` pre-RoPE q|k|v rows, 3 * n_heads * hd apart;
 * L = *kv_len_dev cached keys, row r at RoPE position *pos_dev + r; A = min(*n_active_dev, rows, cache_cap - L) active rows.
 * Row r < A attends keys [0, L + r]; the kernel rotates and stores the A new K/V rows at cache rows L .. L + A - 1 (the bits
 * ss_rope_kv_append stores) and takes them from registers, each 16-byte packet of the old cache is loaded once for all rows.
 * out [rows, n_heads * hd]: rows >= A are not written.  workspace: rows * ss_attn_decode_workspace_bytes(n_heads, hd).
 * ss_spec_draft — the lookup draft alone: hist_dev int32[len] -> out_ids_dev[0 .. *out_count_dev), k <= 7 tokens at most.
 *
 * The workspace of ss_llama_spec_bytes is caller-owned device memory (256-byte aligned), as the planes of ss_llama_set_kv8 are: it
 * holds the R-row activations, R logits rows, attention partials, row states, drafts and counters, so an n_seq = 1 engine can
 * speculate.  ss_llama_set_speculation(h, NULL, NULL) turns the option off.  While it is on, ss_llama_generate runs speculative
 * steps (eager or captured; the captured graph is keyed by the parameters and the workspace) and appends every emitted token to
 * the slot's history; ss_llama_generate_batch, ss_llama_fork and ss_llama_beam_search run as they always do.
 * ss_llama_generate returns SS_EINVAL before anything is launched when the selected slot also has sampling, history rules,
 * log-probability recording, the fp8 KV shadow or attention-map capture on (none of these is built for R rows).
 * ss_llama_spec_stats: out[4] = speculative steps, rows drafted, drafts accepted, tokens emitted by the last ss_llama_generate. */
#define SS_SPEC_LOOKUP 0
#define SS_SPEC_GIVEN 1
#define SS_SPEC_MAX_ROWS 8
typedef struct ss_spec_params {
    int32_t rows;               /* 2 .. 8 */
    int32_t max_ngram;          /* 1 .. 8 (SS_SPEC_LOOKUP) */
    int32_t source;             /* SS_SPEC_LOOKUP | SS_SPEC_GIVEN */
    int32_t given_len;
    const int32_t* given_ids;   /* device, SS_SPEC_GIVEN */
} ss_spec_params;
int ss_llama_spec_bytes(const ss_llama_config* cfg, int32_t rows, size_t* bytes);
int ss_llama_set_speculation(ss_llama* h, const ss_spec_params* p, void* spec_ws);
int ss_llama_spec_stats(ss_llama* h, int32_t seq, int64_t out[4]);
int ss_attn_decode_spec(const void* qkv, void* kcache, void* vcache, const void* cos, const void* sin, void* out, void* workspace,
                        const int32_t* kv_len_dev, const int32_t* pos_dev, const int32_t* n_active_dev, int64_t rows,
                        int64_t n_heads, int64_t hd, int64_t cache_cap, int dtype, void* stream);
int ss_spec_draft(const int32_t* hist_dev, int64_t len, int32_t max_ngram, int32_t k, int32_t n_stop, const int32_t* stop_ids,
                  int32_t* out_ids_dev, int32_t* out_count_dev, void* stream);

/* LlamaModel.forward on M new rows against the cached prefix (prefill when the cache is
 * empty, bottom-right-causal continuation otherwise) — modeling_llama_xformer.py:532-666.
 * embeds [M, hidden]; pos_ids device int32[M] or NULL (pos, pos+1, …).  Writes the
 * post-final-norm hidden rows to hidden_out [M, hidden] if non-NULL, and the LAST row's
 * lm_head logits into the engine's logits buffer (the reference computes all rows, :759,
 * but only row -1 is consumed by greedy search).  Advances kv_len/pos by M. */
int ss_llama_prefill(ss_llama* h, const void* embeds, int64_t M, const int32_t* pos_ids, void* hidden_out,
                     void* stream);
/* ss_llama_prefill for several sequence slots in ONE sweep of the weights: embeds = the slots' new rows stacked
 * slot-major [sum(host_rows), hidden], host_rows[n_seq] (host array; 0 = slot sits out).  Every projection runs once on
 * the stack (the layer weights are streamed once per call, not once per slot); RoPE / KV append / bottom-right causal
 * attention run per slot against that slot's cache, positions continue from each slot's own `pos`.  Each slot's last
 * row's logits land in that slot's logits buffer; hidden_out [sum(host_rows), hidden] or NULL.  Used for the image-token
 * block continuation of lock-step stories (generation.py:19-31 forces those ids) and their prompt prefill. */
int ss_llama_prefill_batch(ss_llama* h, const void* embeds, const int64_t* host_rows, void* hidden_out, void* stream);

/* Greedy decode (HF greedy search as driven from models.py:146-153):
 * starting from the logits buffer left by prefill, runs up to n_steps iterations of
 * {processor -> argmax (or forced[i] while i < n_forced) -> append -> embed -> 32 layers ->
 * final norm -> lm_head}, entirely on device from a captured hipGraph, stopping at EOS.
 * last_prompt_id seeds the processor's "last token" for the first step.
 * host_n_generated receives the number of tokens produced (synchronises the stream). */
int ss_llama_generate(ss_llama* h, int64_t n_steps, int32_t last_prompt_id, const int32_t* host_forced,
                      int64_t n_forced, int64_t* host_n_generated, void* stream);

/* The same loop for all n_seq slots at once: every decode projection sweeps the weights ONCE and
 * dots each pack with all slots' activations (HBM bytes per generated token fall as 1/n_seq).
 * Per slot b: last_prompt_ids[b], forced tokens host_forced[b*forced_ld .. +n_forced[b]) (both
 * optional), active[b] == 0 leaves the slot untouched (NULL = all active).  Slots stop
 * independently at EOS / n_steps; host_n_generated[n_seq] receives the per-slot token counts.
 * After the call the logits buffer of a slot that stopped early is undefined. */
int ss_llama_generate_batch(ss_llama* h, int64_t n_steps, const int32_t* last_prompt_ids,
                            const int32_t* host_forced, int64_t forced_ld, const int64_t* n_forced,
                            const int32_t* active, int64_t* host_n_generated, void* stream);

/* Per-kernel-class device time of one decode token (all n_seq slots together), measured with a hipEvent pair around EVERY
 * launch of un-captured (eager) decode steps on `stream`, averaged over n_tokens:
 * out_ms[0] = sum over the K=hidden GEMV launches (qkv, o, gate|up per layer + lm_head:
 *             ss::gemv_kernel), [1] = attention (+split merge), [2] = sum over the down-projection
 *             GEMV launches (ss::gemv_ldsx_kernel), [3] = sampling + final norm, [4] = whole token;
 * out_bytes[0] = weight bytes streamed by the class-0 launches of one token, [1] = their count,
 * out_bytes[2] / [3] = the same for class 2.  With ss_llama_set_decode_w8 on, the token is the fp8 one and the bytes are
 * the bytes it streams: one per weight plus the fp32 row scales; with ss_llama_set_decode_mx4 on, the MXFP4 one: weights / 2
 * of codes plus weights / 32 of block scales. */
int ss_llama_profile_decode(ss_llama* h, int64_t n_tokens, float out_ms[8], double out_bytes[4],
                            void* stream);

/* ---------------------------------------------------------------------------------------
 * Learnable-query cross-attention Resampler (qwen_visual.py:95-153) — input_resampler,
 * output_resampler ("image-feature regressor") and the ViT attn_pool.
 * ------------------------------------------------------------------------------------- */
typedef struct ss_resampler_weights {
    const void* q_in;      /* [nq, E]  = ln_q(query) + pos_embed, precomputed once at load      */
    const void* pos_kv;    /* [Lkv, E] = get_abs_pos(pos_embed, Lkv) (bicubic, :23-39)           */
    const void* kv_proj;   /* [E, kv_dim] or NULL (Identity when kv_dim == E, :116-121)          */
    const void *ln_kv_w, *ln_kv_b;
    const void *in_w, *in_b;   /* nn.MultiheadAttention in_proj [3E, E], [3E] ([Q;K;V] blocks) */
    const void *out_w, *out_b; /* out_proj [E, E], [E]                                          */
    int32_t nq, embed, n_heads, kv_dim, l_kv;
    float ln_eps;
} ss_resampler_weights;
size_t ss_resampler_workspace_bytes(const ss_resampler_weights* w, int64_t batch, int dtype);
/* x [batch, l_kv, kv_dim] -> y [batch, nq, E] */
int ss_resampler_forward(const ss_resampler_weights* w, const void* x, void* y, int64_t batch, void* workspace,
                         size_t workspace_bytes, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------
 * Qwen ViT-G trunk (qwen_visual.py:376-392: conv1 -> +pos -> ln_pre -> 48 blocks)
 * ------------------------------------------------------------------------------------- */
typedef struct ss_vit_layer_weights {
    const void *ln1_w, *ln1_b, *ln2_w, *ln2_b;
    const void *in_w, *in_b;   /* attn.in_proj [3*width, width], head-interleaved [h][q|k|v] (:192-199) */
    const void *out_w, *out_b;
    const void *fc_w, *fc_b, *proj_w, *proj_b;
} ss_vit_layer_weights;
typedef struct ss_vit_weights {
    const void* conv_w;   /* [width, kpad]  (conv1.weight flattened (c,dy,dx), zero padded to kpad) */
    const void* pos;      /* [tokens, width] = get_abs_pos(positional_embedding, tokens)           */
    const void *ln_pre_w, *ln_pre_b;
    const ss_vit_layer_weights* layers; /* host array[n_layers] */
    int32_t width, n_layers, n_heads, mlp_width, patch, image, kpad;
    float ln_eps;
} ss_vit_weights;
size_t ss_vit_workspace_bytes(const ss_vit_weights* w, int64_t batch, int dtype);
/* img [batch,3,image,image] (T) -> tokens [batch, (image/patch)^2, width] */
int ss_vit_forward(const ss_vit_weights* w, const void* img, void* out, int64_t batch, void* workspace,
                   size_t workspace_bytes, int dtype, void* stream);

/* The transformer trunk alone: VisualAttentionBlock layers [layer0, layer0 + n_layers) of w applied IN PLACE to
 * tokens x [batch, tokens, width] (qwen_visual.py:275-287: x += attn(ln_1(x)); x += mlp(ln_2(x))); ss_vit_forward is
 * patch-embed + pos + ln_pre + this call over all layers.  Workspace as ss_vit_workspace_bytes. */
int ss_vit_blocks(const ss_vit_weights* w, void* x, int64_t batch, int64_t tokens, int64_t layer0, int64_t n_layers,
                  void* workspace, size_t workspace_bytes, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------
 * SDXL de-tokenizer half (the reference reaches these ops through diffusers:
 * src/models_ipa/adapter_modules.py:455-466, gen_george.py:60-64).
 * Activations are NHWC: [batch, H*W, C] row-major.
 * ------------------------------------------------------------------------------------- */

/* 3x3 convolution, padding 1, stride 1|2, as an implicit GEMM on the matrix cores (diffusers
 * ResnetBlock2D.conv1/conv2, Downsample2D.conv, Upsample2D.conv, conv_in/conv_out):
 * x [B,H,W,Cin] -> y [B,Ho,Wo,Cout]; w [Cout, 9*Cin] with k = (ky*3+kx)*Cin + ci (re-laid once at
 * load); upsample2x fuses F.interpolate(scale 2, nearest) of the input into the gather;
 * bias [Cout] | NULL; rowvec | NULL = per-batch vector added after the bias (ResBlock time embedding,
 * `h + temb[:, :, None, None]`): element (b, co) at rowvec[b * rowvec_stride + co] (stride 0 = Cout);
 * residual [B,Ho,Wo,Cout] | NULL is added last. Cin % 8 == 0. */
int ss_conv3x3(const void* x, const void* w, void* y, int64_t batch, int64_t H, int64_t W, int64_t Cin,
               int64_t Cout, int64_t stride, int64_t upsample2x, const void* bias, const void* rowvec,
               int64_t rowvec_stride, const void* residual, int dtype, void* stream);

/* nn.GroupNorm over NHWC (+ optional fused SiLU) — replaces diffusers' ResnetBlock2D.norm1/norm2, Transformer2DModel.norm,
 * UNet conv_norm_out and the VAE decoder's norms (reference call site: src/models_ipa/adapter_modules.py:455-466 through
 * the diffusers UNet / AutoencoderKL).  Statistics per (batch, group) are reduced in a FIXED order (block partials in fp64,
 * folded by a second pass in block order): two runs on the same input give the same bits.  stats_ws must hold
 * ss_groupnorm_workspace_bytes(batch, hw, channels, groups, dtype) bytes (final sums + block partials). */
size_t ss_groupnorm_workspace_bytes(int64_t batch, int64_t hw, int64_t channels, int64_t groups, int dtype);
int ss_groupnorm(const void* x, const void* gamma, const void* beta, void* y, void* stats_ws, int64_t batch,
                 int64_t hw, int64_t channels, int64_t groups, float eps, int fuse_silu, int dtype, void* stream);

/* ---- loss heads of the training-side forward (forward only) ------------------------------------------
 * Deterministic (fixed-order reductions, no atomics); 16-bit dtypes round where the reference's torch graph rounds.
 *
 * ss_cross_entropy_rows — the token loss of LlamaForCausalLM.forward(labels=...)
 *   (src/models_clm/modeling_llama_xformer.py:761-772: CrossEntropyLoss over logits[..., :-1, :] / labels[..., 1:]):
 *   row_loss[r] = -log_softmax(logits[r, :vocab])[labels[r]], row_valid[r] = 1; labels[r] == ignore_index -> 0 / 0.
 *   The caller passes the already shifted rows (logits row r with the label of position r + 1).
 * ss_cosine_rows — cosine_loss of src/models_clm/models.py:13-17: row_val[r] = 1 - <rec_r/|rec_r|, target_r/|target_r|>.
 * ss_masked_mean — out2[0] = sum(vals * mask) / sum(mask) (mask NULL: plain mean), out2[1] = the denominator;
 *   workspace = ss_loss_workspace_bytes(n).
 * ss_mse — F.mse_loss(a.float(), b.float(), reduction="mean") of src/models_ipa/adapter_modules.py:339 -> out2[0]. */
size_t ss_loss_workspace_bytes(int64_t n);
int ss_cross_entropy_rows(const void* logits, int64_t ld, const int64_t* labels, int64_t rows, int64_t vocab,
                          int64_t ignore_index, float* row_loss, float* row_valid, int dtype, void* stream);
int ss_cosine_rows(const void* rec, const void* target, int64_t rows, int64_t dim, float* row_val, int dtype, void* stream);
int ss_masked_mean(const float* vals, const float* mask, int64_t n, void* workspace, float* out2, void* stream);
int ss_mse(const void* a, const void* b, int64_t n, void* workspace, float* out2, int dtype, void* stream);

/* diffusers GEGLU: in [rows, 2d] = [value | gate] -> out[r,i] = value * gelu_erf(gate). */
int ss_geglu(const void* in, void* out, int64_t rows, int64_t d, int dtype, void* stream);
/* y = silu(x) (op 0) | gelu_erf(x) (op 1), element-wise (time-embedding activations). */
int ss_unary(const void* x, void* y, int64_t n, int op, int dtype, void* stream);
/* in-place row softmax of scores[rows, cols] * scale (VAE mid-block attention, head_dim 512). */
int ss_softmax_rows(void* scores, int64_t rows, int64_t cols, float scale, int dtype, void* stream);
/* out[c, r] = in[r, c] */
int ss_transpose(const void* in, void* out, int64_t rows, int64_t cols, int dtype, void* stream);
/* out[r, :] = [a[r, :c1] | b[r, :c2]]  (torch.cat([h, skip], dim=1) of the UNet up path, NHWC). */
int ss_concat_channels(const void* a, const void* b, void* out, int64_t rows, int64_t c1, int64_t c2, int dtype,
                       void* stream);
/* NCHW [B,C,HW] <-> NHWC [B,HW,cpad] (zero padded channels) for the 4-channel latents. */
int ss_layout_nchw_nhwc(const void* in, void* out, int64_t batch, int64_t channels, int64_t hw, int64_t cpad,
                        int to_nhwc, int dtype, void* stream);
/* EulerDiscreteScheduler.scale_model_input + CFG duplication: xin[0] = xin[1] = x / sqrt(sigma^2+1). */
int ss_euler_scale_dup(const void* x, void* xin, int64_t n, float sigma, int dtype, void* stream);
/* e = eps[0] + guidance * (eps[1] - eps[0]);  x += e * (sigma_next - sigma)   (adapter_modules.py:437;
 * EulerDiscreteScheduler.step, epsilon prediction). eps = [uncond; cond], n elements each. */
int ss_euler_cfg_step(void* x, const void* eps, int64_t n, float guidance, float sigma, float sigma_next,
                      int dtype, void* stream);
/* One step of a linear multistep sampler with classifier-free guidance, fused with the NEXT step's
 * scale_model_input + CFG duplication (DPMSolverMultistepScheduler: dpmsolver++, midpoint, order <= 2):
 *   e = eps[0] + guidance * (eps[1] - eps[0]);  d = x - sigma * e;  x' = a * x + b * d + c * d_prev
 * state fp32 [2, n]: row 0 = x, row 1 = d_prev; rewritten as (x', d).  The arithmetic is fp32 end to end: the solver
 * state is never rounded to `dtype` between steps.  eps [2, n] in `dtype` = [uncond; cond].
 *   x_out [n] | NULL          receives rnd(x')
 *   xin_next [2, n] | NULL    both rows receive rnd(x' * inv_next)   (inv_next = 1 / sqrt(sigma_next^2 + 1))
 * c == 0 (first step, first-order step, last step): row 1 of state is NOT read (it may be uninitialised).  (a, b, c) are
 * the host's (computed in double): DPM++ 2M, first order (s'/s, E, 0), second order (s'/s, E (1 + 1/2r), -E/2r), last step
 * (0, 1, 0); Euler is (s'/s, 1 - s'/s, 0).  Any n >= 1: 16-byte packets over the first rows (second rows too when n is a
 * multiple of the packet), single elements for the tail, and for everything when a base pointer is not 16-byte aligned.
 * SS_EINVAL before anything is launched or written: n <= 0, NULL state or eps, a non-finite guidance / sigma / a / b /
 * c / inv_next, an unknown dtype. */
int ss_multistep_cfg_step(float* state, const void* eps, void* x_out, void* xin_next, int64_t n, float guidance,
                          float sigma, float a, float b, float c, float inv_next, int dtype, void* stream);
/* Limited-interval guidance (CFG only while sigma_lo < sigma <= sigma_hi): the same step for a forward that
 * ran on [uncond; cond] (eps_rows 2) or on the conditional rows alone (eps_rows 1), writing the next step's input once
 * (xin_rows 1: the next step is unguided) or twice (xin_rows 2).
 *   eps_rows 2: e = eps[0] + guidance * (eps[1] - eps[0])     eps_rows 1: e = eps[0] as loaded, guidance is not used
 *   d = x - sigma * e;  x' = a * x + b * d + c * d_prev;  state <- (x', d);  x_out = rnd(x');
 *   xin_next[0 .. xin_rows) = rnd(x' * inv_next)
 * eps is [eps_rows, n] and xin_next [xin_rows, n]: a row the form does not have is neither read nor written.  Operation
 * order, packets, tail, unaligned bases and the c == 0 rule are ss_multistep_cfg_step's; (2, 2) is bit-equal to it.
 * SS_EINVAL before anything is launched or written: as ss_multistep_cfg_step, and eps_rows or xin_rows outside {1, 2}. */
int ss_multistep_step(float* state, const void* eps, void* x_out, void* xin_next, int64_t n, int eps_rows, int xin_rows,
                      float guidance, float sigma, float a, float b, float c, float inv_next, int dtype, void* stream);
/* Gaussian noise of the stochastic samplers (Euler ancestral, DPM++ 2M SDE; definition: tests/sde_ref.py).
 * z for image seed S (64 bit), step i and flat element j of that image's latent depends on nothing else:
 *   (w0, w1, w2, w3) = Philox4x32-10(counter (j >> 2, i, 1, 0), key (S & 0xFFFFFFFF, S >> 32));  u(w) = (w >> 8) 2^-24;
 *   r(w) = sqrt(-2 ln(u(w) + 2^-24));  element j takes lane j & 3 of
 *   [r(w0) cos(2 pi u(w1)), r(w0) sin(2 pi u(w1)), r(w2) cos(2 pi u(w3)), r(w2) sin(2 pi u(w3))]      (fp32; |z| <= 5.77)
 * Counter word 2 = 1 keeps the stream apart from ss_sample_logits' (draw, slot, 0, 0).  Images with equal seeds get equal
 * noise; the value does not depend on the batch.
 *   out [batch, n_img] in `dtype` receives rnd(z(seeds_dev[b], step, j));  seeds_dev: uint64 [batch] in DEVICE memory.
 * Any n_img >= 1: one store per quad when n_img % 4 == 0 and `out` is 16-byte aligned, single elements otherwise.
 * SS_EINVAL before anything is launched or written: NULL out or seeds, batch <= 0, n_img <= 0 (or > 2^34), step < 0, an
 * unknown dtype. */
int ss_randn_philox(void* out, const uint64_t* seeds_dev, int64_t batch, int64_t n_img, int step, int dtype, void* stream);
/* ss_multistep_step with a noise term: x' = ((a * x + b * d) [+ c * d_prev]) + s * z — one fp32 product and one fp32 sum after
 * ss_multistep_step's chain, everything else (forms, state, outputs, c == 0 rule) as there.  z is ss_randn_philox's value
 * (the same device function: bit-equal) for element i % n_img of image i / n_img, seed seeds_dev[i / n_img], step `step`.
 * Euler ancestral: (a, b, c, s) = (sd/s_i, 1 - sd/s_i, 0, s_up); DPM++ 2M SDE: DESIGN §6.0l; the last step of both (0, 1, 0, 0).
 * 16-byte packets when every base is 16-byte aligned and n_img is a multiple of the packet (a packet then lies in one
 * image), single elements for everything otherwise.  s == 0: z is not generated, seeds_dev may be NULL, and every output is
 * bit-equal to ss_multistep_step (its kernels are launched).
 * SS_EINVAL before anything is launched or written: as ss_multistep_step, and n_img <= 0 (or > 2^34), n % n_img != 0,
 * step < 0, a non-finite s, s != 0 with NULL seeds_dev. */
int ss_multistep_noise_step(float* state, const void* eps, void* x_out, void* xin_next, int64_t n, int eps_rows, int xin_rows,
                            float guidance, float sigma, float a, float b, float c, float s, float inv_next,
                            const uint64_t* seeds_dev, int64_t n_img, int step, int dtype, void* stream);
/* Unguided Euler step: x += rnd(eps * (sigma_next - sigma)), eps [n] the conditional prediction (ss_euler_cfg_step
 * without its guidance arithmetic, same rounding point).  SS_EINVAL: n <= 0, NULL x or eps, unknown dtype. */
int ss_euler_step(void* x, const void* eps, int64_t n, float sigma, float sigma_next, int dtype, void* stream);
/* scale_model_input into `rows` copies: xin[0 .. rows) = x / sqrt(sigma^2+1); rows 2 is bit-equal to ss_euler_scale_dup,
 * rows 1 writes n elements only.  SS_EINVAL: n <= 0, NULL x or xin, rows outside {1, 2}, unknown dtype. */
int ss_euler_scale(const void* x, void* xin, int64_t n, int rows, float sigma, int dtype, void* stream);
/* Image pre-processing on the device: the reference's `image_transform(image).to(device, dtype)`
 * (src/processer/transforms.py:4-19 = torchvision Resize [+ CenterCrop] on a PIL image, ToTensor, Normalize;
 * gen_george.py:166).  The resize is Pillow's 8-bit separable resampler restated bit-exactly: 22-bit fixed-point
 * taps, horizontal pass into a uint8 intermediate, vertical pass, then fp32 (u8/255 - mean)/std rounded to `dtype`.
 *   ss_resample_ksize / ss_resample_coeffs  HOST functions: the tap table of one axis (Pillow's precompute + normalize
 *       coefficient steps, in double): coef [out_size * ksize] int32, bounds [out_size * 2] = {first tap, tap count}.
 *   ss_image_preprocess  src uint8 HWC [H, W, 3] (device) -> dst [3, CH, CW] `dtype` = rows crop_top.., columns
 *       crop_left.. of the [OH, OW] resize (CenterCrop; pass 0, 0, OH, OW for none); dst_u8_hwc (optional, [CH, CW, 3])
 *       receives the resized uint8 pixels (what PIL would return).  coef / bounds tables are DEVICE pointers.
 *       Only source rows [first_row, first_row + n_rows) are read (the span the cropped output needs: from
 *       bounds_v[2*crop_top] to the last tap of row crop_top+CH-1); tmp_u8 holds n_rows * OW * 3 bytes. */
#define SS_FILTER_BILINEAR 0 /* torchvision's default for Resize ('clip' / 'clipa' transforms) */
#define SS_FILTER_BICUBIC 1  /* the 'sd' transform */
int ss_resample_ksize(int64_t in_size, int64_t out_size, int filter);
int ss_resample_coeffs(int64_t in_size, int64_t out_size, int filter, int32_t* coef, int32_t* bounds);
int ss_image_preprocess(const void* src_u8_hwc, int64_t H, int64_t W, void* dst_chw, void* dst_u8_hwc, int64_t OH, int64_t OW,
                        int64_t crop_top, int64_t crop_left, int64_t CH, int64_t CW, const int32_t* coef_h,
                        const int32_t* bounds_h, int ksize_h, const int32_t* coef_v, const int32_t* bounds_v, int ksize_v,
                        int64_t first_row, int64_t n_rows, void* tmp_u8, const float mean[3], const float std[3], int dtype,
                        void* stream);
/* VAE output NHWC [pixels, cpad] -> uint8 HWC: round(clamp(x/2 + 0.5, 0, 1) * 255). */
int ss_image_to_u8(const void* in, void* out_u8, int64_t pixels, int64_t cpad, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------
 * Diagnostics
 * ------------------------------------------------------------------------------------- */
/* One wave executes ds_read_b64_tr_b16 with per-lane LDS offsets lane_off[64] (int32, in 16-bit
 * elements) over an 8 KB LDS image copied from src (4096 u16), and writes each lane's four 16-bit
 * results to dst[64*4].
 * Documents the transposed-read lane mapping flash_attn2_kernel relies on (tools/tr_probe.py). */
int ss_debug_tr_probe(const void* src, void* dst, const void* lane_off, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SEEDSTORY_HIP_H_ */
