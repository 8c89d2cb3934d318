// Native forward drivers for the non-LLaMA modules of the MLLM half of the hot path:
//   * learnable-query cross-attention Resampler (src/models/qwen_visual.py:95-153) — used as
//     input_resampler (256 -> 64 tokens), output_resampler (the image-feature regressor,
//     64 -> 256 tokens; src/models_clm/models.py:205) and the ViT's attn_pool;
//   * Qwen ViT-G trunk (qwen_visual.py:376-392 with VisualAttention :184-235 and
//     VisualAttentionBlock :275-287);
//   * the stand-alone logits-processor + argmax entry point.
// These are host loops over the HIP kernels of this library: one C call per module forward
// instead of hundreds of framework-level op dispatches.
#include "ss_common.h"
#include "ss_sample.h"
#include "ss_rules.h"
#include "ss_logprob.h"
#include "ss_beam.h"

namespace ss {
int gemm_dev(const void* A, const void* W, void* C, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldw,
             int64_t ldc, const void* bias, const void* residual, int64_t ldr, int epi, int dtype, hipStream_t s);

template <typename T>
__global__ __launch_bounds__(1024) void imgproc_argmax_kernel(T* logits, int vocab, const int32_t* last_id,
                                                              const int32_t* img_ids, int n_img_ids, int32_t* tok) {
    __shared__ float sv[16];
    __shared__ int si[16];
    const int t = imgproc_argmax_block<T>(logits, vocab, *last_id, img_ids, n_img_ids, sv, si);
    if (threadIdx.x == 0) *tok = t;
}

template <typename T>
int imgproc_argmax_launch(void* logits, int64_t vocab, const int32_t* last_id, const int32_t* img_ids, int64_t n,
                          int32_t* tok, hipStream_t s) {
    hipLaunchKernelGGL(imgproc_argmax_kernel<T>, dim3(1), dim3(1024), 0, s, (T*)logits, (int)vocab, last_id, img_ids,
                       (int)n, tok);
    SS_LAUNCH_CHECK("imgproc_argmax");
    return SS_OK;
}

// ss_sample_logits: one block per row
template <typename T, int NS>
__global__ __launch_bounds__(1024) void sample_logits_kernel(T* logits, int vocab, int64_t ld, SampleParams p,
                                                             const float* __restrict__ u_dev, uint32_t draw0,
                                                             const int32_t* __restrict__ last_ids, const int32_t* img_ids,
                                                             int n_img_ids, int32_t* tok, int32_t* n_kept) {
    __shared__ float sv[16];
    __shared__ int si[16];
    __shared__ SampleSmem sm;
    const int r = blockIdx.x;
    logits += (int64_t)r * ld;
    float u = u_dev ? u_dev[r] : philox_uniform(p.seed_lo, p.seed_hi, draw0, (uint32_t)r);
    u = fminf(fmaxf(u, 0.f), 0.99999994f);      // a caller's u outside [0, 1) (or NaN) is clamped
    int nk = 0, drew = 0;
    const int t = imgproc_sample_block<T, NS>(logits, vocab, last_ids != nullptr, last_ids ? last_ids[r] : -1, img_ids,
                                              n_img_ids, p.inv_temp, p.top_p, p.top_k, u, sv, si, sm, &nk, &drew);
    if (threadIdx.x == 0) {
        tok[r] = t;
        if (n_kept) n_kept[r] = nk;
    }
}

template <typename T>
int sample_logits_launch(void* logits, int64_t rows, int64_t vocab, int64_t ld, const SampleParams& p, const float* u_dev,
                         uint32_t draw0, const int32_t* last_ids, const int32_t* img_ids, int64_t n, int32_t* tok,
                         int32_t* n_kept, hipStream_t s) {
    if (sample_ns_half_fits(vocab))
        hipLaunchKernelGGL((sample_logits_kernel<T, sample_ns_full<T>() / 2>), dim3((unsigned)rows), dim3(1024), 0, s, (T*)logits,
                           (int)vocab, ld, p, u_dev, draw0, last_ids, img_ids, (int)n, tok, n_kept);
    else
        hipLaunchKernelGGL((sample_logits_kernel<T, sample_ns_full<T>()>), dim3((unsigned)rows), dim3(1024), 0, s, (T*)logits,
                           (int)vocab, ld, p, u_dev, draw0, last_ids, img_ids, (int)n, tok, n_kept);
    SS_LAUNCH_CHECK("sample_logits");
    return SS_OK;
}

// ss_process_logits: one block per row; the rule-1 bitmap of the row's history is built in LDS (one owner thread per word)
template <typename T>
__global__ __launch_bounds__(1024) void process_logits_kernel(T* logits, int vocab, int64_t ld, RulesState p,
                                                              const int32_t* __restrict__ hist, int64_t hist_ld,
                                                              const int32_t* __restrict__ hist_len,
                                                              const int32_t* __restrict__ prompt_len, int eos,
                                                              const int32_t* __restrict__ img_ids, int n_img_ids) {
    __shared__ uint32_t bm[2048];       // vocab <= 65535
    const int r = blockIdx.x;
    logits += (int64_t)r * ld;
    hist += (int64_t)r * hist_ld;
    int len = hist_len[r];
    len = len < 0 ? 0 : (len > hist_ld ? (int)hist_ld : len);
    if (p.penalty != 1.0f) {
        rules_bitmap_add(bm, rules_bitmap_words(vocab), threadIdx.x, 1024, hist, len, false);
        __syncthreads();
    }
    logits_rules_block<T>(logits, vocab, p.penalty, p.ngram, p.min_new, p.spare_img != 0, bm, hist, len,
                          prompt_len ? prompt_len[r] : 0, eos, img_ids, n_img_ids);
}

template <typename T>
int process_logits_launch(void* logits, int64_t rows, int64_t vocab, int64_t ld, const RulesState& p, const int32_t* hist,
                          int64_t hist_ld, const int32_t* hist_len, const int32_t* prompt_len, int eos, const int32_t* img_ids,
                          int64_t n, hipStream_t s) {
    hipLaunchKernelGGL(process_logits_kernel<T>, dim3((unsigned)rows), dim3(1024), 0, s, (T*)logits, (int)vocab, ld, p, hist,
                       hist_ld, hist_len, prompt_len, eos, img_ids, (int)n);
    SS_LAUNCH_CHECK("process_logits");
    return SS_OK;
}

// ss_token_logprobs, plain form: one block per row, the row only read
template <typename T, int EPT>
__global__ __launch_bounds__(1024) void token_logprobs_kernel(const T* logits, int vocab, int64_t ld, const int32_t* __restrict__ ids,
                                                              int top_n, float* lp_out, int32_t* top_ids, float* top_lp) {
    __shared__ LogprobSmem sm;
    const int r = blockIdx.x;
    logits += (int64_t)r * ld;
    float v[EPT];
    int flip = 0;
    const LogprobStats s = logprob_load_block<T, EPT>(logits, vocab, v, sm, flip);
    if (lp_out && threadIdx.x == 0) {
        const int tok = ids[r];         // device memory cannot be refused: an id outside the row is never used as an index
        lp_out[r] = (unsigned)tok < (unsigned)vocab ? logprob_value(Tr<T>::ld(logits + tok), s) : __uint_as_float(0x7FC00000u);
    }
    if (top_n > 0) logprob_top_block(v, vocab, s, top_n, top_ids + (int64_t)r * top_n, top_lp + (int64_t)r * top_n, sm);
}

// ss_token_logprobs, sampling form: the sampler's own kept set and Z_P, scored at ids[r]; nothing is drawn
template <typename T, int NS>
__global__ __launch_bounds__(1024) void token_logprobs_sampling_kernel(const T* logits, int vocab, int64_t ld, SampleParams p,
                                                                       const int32_t* __restrict__ ids, float* lp_out) {
    __shared__ SampleSmem sm;
    const int r = blockIdx.x;
    int nk = 0;
    float lp = -INFINITY;
    const int tok = ids[r];
    sample_block<T, NS, true>(logits + (int64_t)r * ld, vocab, p.inv_temp, p.top_p, p.top_k, 0.f, sm, &nk,
                              (unsigned)tok < (unsigned)vocab ? tok : 0x7ffffffe, &lp);
    if (threadIdx.x == 0) lp_out[r] = lp;
}

template <typename T>
int token_logprobs_launch(const void* logits, int64_t rows, int64_t vocab, int64_t ld, const int32_t* ids, const SampleParams* p,
                          int top_n, float* lp_out, int32_t* top_ids, float* top_lp, hipStream_t s) {
    if (!p || top_n > 0) {
        if (logprob_ept_half_fits(vocab))
            hipLaunchKernelGGL((token_logprobs_kernel<T, kLpEptFull / 2>), dim3((unsigned)rows), dim3(1024), 0, s, (const T*)logits,
                               (int)vocab, ld, ids, top_n, p ? nullptr : lp_out, top_ids, top_lp);
        else
            hipLaunchKernelGGL((token_logprobs_kernel<T, kLpEptFull>), dim3((unsigned)rows), dim3(1024), 0, s, (const T*)logits,
                               (int)vocab, ld, ids, top_n, p ? nullptr : lp_out, top_ids, top_lp);
        SS_LAUNCH_CHECK("token_logprobs");
    }
    if (p) {
        if (sample_ns_half_fits(vocab))
            hipLaunchKernelGGL((token_logprobs_sampling_kernel<T, sample_ns_full<T>() / 2>), dim3((unsigned)rows), dim3(1024), 0, s,
                               (const T*)logits, (int)vocab, ld, *p, ids, lp_out);
        else
            hipLaunchKernelGGL((token_logprobs_sampling_kernel<T, sample_ns_full<T>()>), dim3((unsigned)rows), dim3(1024), 0, s,
                               (const T*)logits, (int)vocab, ld, *p, ids, lp_out);
        SS_LAUNCH_CHECK("token_logprobs_sampling");
    }
    return SS_OK;
}

// ss_beam_step: one block, the rows one after the other
template <typename T>
int beam_step_launch(const void* logits, int64_t rows, int64_t vocab, int64_t ld, const float* beam_scores, int K, float* cand_score,
                     int32_t* cand_beam, int32_t* cand_tok, hipStream_t s) {
    if (logprob_ept_half_fits(vocab))
        hipLaunchKernelGGL((beam_step_kernel<T, kLpEptFull / 2>), dim3(1), dim3(1024), 0, s, (const T*)logits, (int)rows, (int)vocab, ld,
                           beam_scores, K, cand_score, cand_beam, cand_tok);
    else
        hipLaunchKernelGGL((beam_step_kernel<T, kLpEptFull>), dim3(1), dim3(1024), 0, s, (const T*)logits, (int)rows, (int)vocab, ld,
                           beam_scores, K, cand_score, cand_beam, cand_tok);
    SS_LAUNCH_CHECK("beam_step");
    return SS_OK;
}

struct Bump {
    char* p; size_t off, cap;
    void* take(size_t bytes) { void* r = p + off; off += (bytes + 255) / 256 * 256; return r; }
};
}  // namespace ss

using namespace ss;

extern "C" {

int ss_imgproc_argmax(void* logits, int64_t vocab, const int32_t* last_id_dev, const int32_t* img_ids,
                      int64_t n_img_ids, int32_t* token_out_dev, int dtype, void* stream) {
    SS_REQUIRE(logits && last_id_dev && token_out_dev && vocab > 0, "imgproc_argmax: bad arguments");
    return SS_DISPATCH(dtype, imgproc_argmax_launch, logits, vocab, last_id_dev, img_ids, n_img_ids, token_out_dev,
                       (hipStream_t)stream);
}

int ss_sample_logits(void* logits, int64_t rows, int64_t vocab, int64_t ld, const ss_sampling* p, const float* u_dev,
                     uint32_t draw0, const int32_t* last_ids_dev, const int32_t* img_ids, int64_t n_img_ids,
                     int32_t* token_out_dev, int32_t* n_kept_out_dev, int dtype, void* stream) {
    SS_REQUIRE(logits && token_out_dev && p, "sample_logits: null argument");
    SS_REQUIRE(rows > 0 && rows <= 0x7FFFFFFF && vocab > 0 && vocab <= 65535 && ld >= vocab,
               "sample_logits: bad shape (rows=%lld vocab=%lld ld=%lld; vocab <= 65535)", (long long)rows, (long long)vocab,
               (long long)ld);
    SS_REQUIRE(n_img_ids >= 0 && n_img_ids <= 1024, "sample_logits: n_img_ids=%lld out of range (0..1024)", (long long)n_img_ids);
    SampleParams sp;
    if (int rc = sampling_params(p, "sample_logits", &sp)) return rc;
    const bool proc = last_ids_dev && img_ids;
    return SS_DISPATCH(dtype, sample_logits_launch, logits, rows, vocab, ld, sp, u_dev, draw0, proc ? last_ids_dev : nullptr,
                       proc ? img_ids : nullptr, proc ? n_img_ids : 0, token_out_dev, n_kept_out_dev, (hipStream_t)stream);
}

int ss_process_logits(void* logits, int64_t rows, int64_t vocab, int64_t ld, const ss_logits_rules* rules,
                      const int32_t* hist_dev, int64_t hist_ld, const int32_t* hist_len_dev, const int32_t* prompt_len_dev,
                      int32_t eos_id, const int32_t* img_ids, int64_t n_img_ids, int dtype, void* stream) {
    SS_REQUIRE(logits && rules && hist_len_dev, "process_logits: null argument");
    SS_REQUIRE(rows > 0 && rows <= 0x7FFFFFFF && vocab > 0 && vocab <= 65535 && ld >= vocab,
               "process_logits: bad shape (rows=%lld vocab=%lld ld=%lld; vocab <= 65535)", (long long)rows, (long long)vocab,
               (long long)ld);
    SS_REQUIRE(hist_ld >= 0 && hist_ld <= 0x7FFFFFFF && (hist_dev || hist_ld == 0), "process_logits: bad history (hist_ld=%lld)",
               (long long)hist_ld);
    SS_REQUIRE(n_img_ids >= 0 && n_img_ids <= 1024 && (img_ids || n_img_ids == 0), "process_logits: n_img_ids=%lld out of range (0..1024)",
               (long long)n_img_ids);
    RulesState rp = {1.0f, 0, 0, 0, 0, 0, 0, 0};
    if (int rc = logits_rules_params(rules, "process_logits", &rp)) return rc;
    return SS_DISPATCH(dtype, process_logits_launch, logits, rows, vocab, ld, rp, hist_dev, hist_ld, hist_len_dev, prompt_len_dev,
                       (int)eos_id, img_ids, n_img_ids, (hipStream_t)stream);
}

int ss_token_logprobs(const void* logits, int64_t rows, int64_t vocab, int64_t ld, const int32_t* ids_dev, const ss_sampling* p,
                      int32_t top_n, float* lp_out, int32_t* top_ids_out, float* top_lp_out, int dtype, void* stream) {
    SS_REQUIRE(logits && ids_dev && lp_out, "token_logprobs: null argument");
    SS_REQUIRE(rows > 0 && rows <= 0x7FFFFFFF && vocab > 0 && vocab <= 65535 && ld >= vocab,
               "token_logprobs: bad shape (rows=%lld vocab=%lld ld=%lld; vocab <= 65535)", (long long)rows, (long long)vocab,
               (long long)ld);
    SS_REQUIRE(top_n >= 0 && top_n <= SS_LOGPROB_MAX_TOP, "token_logprobs: top_n %d outside [0, %d]", (int)top_n, SS_LOGPROB_MAX_TOP);
    SS_REQUIRE(top_n == 0 || (top_ids_out && top_lp_out), "token_logprobs: top_n %d needs both top-n buffers", (int)top_n);
    SampleParams sp;
    if (p)
        if (int rc = sampling_params(p, "token_logprobs", &sp)) return rc;
    return SS_DISPATCH(dtype, token_logprobs_launch, logits, rows, vocab, ld, ids_dev, p ? &sp : nullptr, (int)top_n, lp_out,
                       top_ids_out, top_lp_out, (hipStream_t)stream);
}

int ss_beam_step(const void* logits, int64_t rows, int64_t vocab, int64_t ld, const float* beam_scores_dev, int32_t n_stop,
                 const int32_t* stop_ids, float* cand_score_out, int32_t* cand_beam_out, int32_t* cand_token_out, int dtype,
                 void* stream) {
    SS_REQUIRE(logits && beam_scores_dev && cand_score_out && cand_beam_out && cand_token_out, "beam_step: null argument");
    SS_REQUIRE(rows > 0 && rows <= SS_BEAM_MAX && vocab > 0 && vocab <= 65535 && ld >= vocab,
               "beam_step: bad shape (rows=%lld vocab=%lld ld=%lld; rows <= %d, vocab <= 65535)", (long long)rows, (long long)vocab,
               (long long)ld, SS_BEAM_MAX);
    SS_REQUIRE(n_stop >= 0 && n_stop <= 2 && (stop_ids || n_stop == 0), "beam_step: n_stop %d outside [0, 2]", (int)n_stop);
    for (int i = 0; i < n_stop; ++i)
        SS_REQUIRE(stop_ids[i] >= 0 && stop_ids[i] < vocab, "beam_step: stop id %d outside [0, %lld)", (int)stop_ids[i], (long long)vocab);
    const int K = (n_stop + 1 > 2 ? n_stop + 1 : 2) * (int)rows;
    return SS_DISPATCH(dtype, beam_step_launch, logits, rows, vocab, ld, beam_scores_dev, K, cand_score_out, cand_beam_out,
                       cand_token_out, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------
// Resampler
// ---------------------------------------------------------------------------------------------
size_t ss_resampler_workspace_bytes(const ss_resampler_weights* w, int64_t batch, int dtype) {
    if (!w) return 0;
    const size_t e = dtype_size(dtype), E = w->embed, rows = (size_t)batch * w->l_kv, q = (size_t)w->nq;
    size_t n = 0;
    auto add = [&](size_t b) { n += (b + 255) / 256 * 256; };
    add(rows * E * e);               // xk (kv_proj output)
    add(rows * E * e);               // xln
    add(rows * E * e);               // kin
    add(rows * E * e);               // K
    add(rows * E * e);               // V
    add(q * E * e);                  // Q
    add((size_t)batch * q * E * e);  // ctx
    return n + 256;
}

int ss_resampler_forward(const ss_resampler_weights* w, const void* x, void* y, int64_t batch, void* workspace,
                         size_t workspace_bytes, int dtype, void* stream) {
    SS_REQUIRE(w && x && y && workspace && batch > 0, "resampler_forward: bad arguments");
    SS_REQUIRE(workspace_bytes >= ss_resampler_workspace_bytes(w, batch, dtype), "resampler_forward: workspace too small");
    SS_REQUIRE(w->embed % w->n_heads == 0, "resampler_forward: embed %% heads != 0");
    const size_t e = dtype_size(dtype);
    const int64_t E = w->embed, L = w->l_kv, rows = batch * L, nq = w->nq;
    const int64_t hd = E / w->n_heads;
    hipStream_t s = (hipStream_t)stream;
    Bump b{(char*)workspace, 0, workspace_bytes};
    void* xk = b.take(rows * E * e);
    void* xln = b.take(rows * E * e);
    void* kin = b.take(rows * E * e);
    void* K = b.take(rows * E * e);
    void* Vv = b.take(rows * E * e);
    void* Q = b.take(nq * E * e);
    void* ctx = b.take(batch * nq * E * e);
    int rc;
    const void* src = x;
    if (w->kv_proj) {  // x = self.kv_proj(x)  (:142)
        if ((rc = gemm_dev(x, w->kv_proj, xk, rows, E, w->kv_dim, w->kv_dim, w->kv_dim, E, nullptr, nullptr, 0,
                           SS_EPI_NONE, dtype, s)))
            return rc;
        src = xk;
    }
    // x = self.ln_kv(x)  (:143);  key input = x + pos_embed (:148)
    if ((rc = ss_layernorm(src, w->ln_kv_w, w->ln_kv_b, xln, rows, E, w->ln_eps, dtype, stream))) return rc;
    if ((rc = ss_add_bcast(xln, w->pos_kv, kin, batch, L, E, L * E, dtype, stream))) return rc;
    // nn.MultiheadAttention in-projections ([Q;K;V] row blocks of in_proj_weight)
    const char* in_w = (const char*)w->in_w;
    const char* in_b = (const char*)w->in_b;
    if ((rc = gemm_dev(w->q_in, in_w, Q, nq, E, E, E, E, E, in_b, nullptr, 0, SS_EPI_BIAS, dtype, s))) return rc;
    if ((rc = gemm_dev(kin, in_w + (size_t)E * E * e, K, rows, E, E, E, E, E, in_b + (size_t)E * e, nullptr, 0,
                       SS_EPI_BIAS, dtype, s)))
        return rc;
    if ((rc = gemm_dev(xln, in_w + (size_t)2 * E * E * e, Vv, rows, E, E, E, E, E, in_b + (size_t)2 * E * e, nullptr, 0,
                       SS_EPI_BIAS, dtype, s)))
        return rc;
    // softmax(q k^T / sqrt(hd)) v per head; the same Q for every batch element (q batch stride 0)
    if ((rc = ss_attention(Q, K, Vv, ctx, batch, w->n_heads, nq, L, hd, 0, hd, E, L * E, hd, E, L * E, hd, E, nq * E, hd,
                           E, 1.0f / sqrtf((float)hd), 0, dtype, stream)))
        return rc;
    return gemm_dev(ctx, w->out_w, y, batch * nq, E, E, E, E, E, w->out_b, nullptr, 0, SS_EPI_BIAS, dtype, s);
}

// ---------------------------------------------------------------------------------------------
// ViT trunk
// ---------------------------------------------------------------------------------------------
// VisualAttentionBlock layers [l0, l0 + nl) in place on x [batch, L, width]; y/qkv/ctx/hm are scratch
static int vit_blocks(const ss_vit_weights* w, void* x, void* y, void* qkv, void* ctx, void* hm, int64_t batch, int64_t L,
                      int64_t l0, int64_t nl, int dtype, void* stream) {
    const size_t e = dtype_size(dtype);
    const int64_t rows = batch * L, Wd = w->width, hd = Wd / w->n_heads;
    hipStream_t s = (hipStream_t)stream;
    int rc;
    for (int64_t l = l0; l < l0 + nl; ++l) {
        const ss_vit_layer_weights& Lw = w->layers[l];
        if ((rc = ss_layernorm(x, Lw.ln1_w, Lw.ln1_b, y, rows, Wd, w->ln_eps, dtype, stream))) return rc;
        if ((rc = gemm_dev(y, Lw.in_w, qkv, rows, 3 * Wd, Wd, Wd, Wd, 3 * Wd, Lw.in_b, nullptr, 0, SS_EPI_BIAS, dtype, s)))
            return rc;
        // per token the in_proj output is [head][q(hd) | k(hd) | v(hd)]  (:192-199)
        const char* q = (const char*)qkv;
        if ((rc = ss_attention(q, q + (size_t)hd * e, q + (size_t)2 * hd * e, ctx, batch, w->n_heads, L, L, hd,
                               L * 3 * Wd, 3 * hd, 3 * Wd, L * 3 * Wd, 3 * hd, 3 * Wd, L * 3 * Wd, 3 * hd, 3 * Wd, L * Wd,
                               hd, Wd, 1.0f / sqrtf((float)hd), 0, dtype, stream)))
            return rc;
        if ((rc = gemm_dev(ctx, Lw.out_w, x, rows, Wd, Wd, Wd, Wd, Wd, Lw.out_b, x, Wd, SS_EPI_BIAS | SS_EPI_RESIDUAL,
                           dtype, s)))
            return rc;
        if ((rc = ss_layernorm(x, Lw.ln2_w, Lw.ln2_b, y, rows, Wd, w->ln_eps, dtype, stream))) return rc;
        if ((rc = gemm_dev(y, Lw.fc_w, hm, rows, w->mlp_width, Wd, Wd, Wd, w->mlp_width, Lw.fc_b, nullptr, 0,
                           SS_EPI_BIAS | SS_EPI_GELU, dtype, s)))
            return rc;
        if ((rc = gemm_dev(hm, Lw.proj_w, x, rows, Wd, w->mlp_width, w->mlp_width, w->mlp_width, Wd, Lw.proj_b, x, Wd,
                           SS_EPI_BIAS | SS_EPI_RESIDUAL, dtype, s)))
            return rc;
    }
    return SS_OK;
}

size_t ss_vit_workspace_bytes(const ss_vit_weights* w, int64_t batch, int dtype) {
    if (!w) return 0;
    const size_t e = dtype_size(dtype);
    const size_t G = w->image / w->patch, rows = (size_t)batch * G * G, Wd = w->width;
    size_t n = 0;
    auto add = [&](size_t b) { n += (b + 255) / 256 * 256; };
    add(rows * w->kpad * e);       // patches
    add(rows * Wd * e);            // x
    add(rows * Wd * e);            // y
    add(rows * 3 * Wd * e);        // qkv
    add(rows * Wd * e);            // ctx
    add(rows * w->mlp_width * e);  // mlp hidden
    return n + 256;
}

int ss_vit_forward(const ss_vit_weights* w, const void* img, void* out, int64_t batch, void* workspace,
                   size_t workspace_bytes, int dtype, void* stream) {
    SS_REQUIRE(w && img && out && workspace && batch > 0, "vit_forward: bad arguments");
    SS_REQUIRE(workspace_bytes >= ss_vit_workspace_bytes(w, batch, dtype), "vit_forward: workspace too small");
    SS_REQUIRE(w->width % w->n_heads == 0 && w->image % w->patch == 0, "vit_forward: bad geometry");
    const size_t e = dtype_size(dtype);
    const int64_t G = w->image / w->patch, L = G * G, rows = batch * L, Wd = w->width, hd = Wd / w->n_heads;
    hipStream_t s = (hipStream_t)stream;
    Bump b{(char*)workspace, 0, workspace_bytes};
    void* patches = b.take(rows * w->kpad * e);
    void* x = b.take(rows * Wd * e);
    void* y = b.take(rows * Wd * e);
    void* qkv = b.take(rows * 3 * Wd * e);
    void* ctx = b.take(rows * Wd * e);
    void* hm = b.take(rows * w->mlp_width * e);
    int rc;
    // conv1 (k = stride = patch, no bias) as im2col + GEMM (:382), + interpolated pos (:387), ln_pre (:389)
    if ((rc = ss_im2col_patch(img, patches, batch, w->image, w->patch, w->kpad, dtype, stream))) return rc;
    if ((rc = gemm_dev(patches, w->conv_w, y, rows, Wd, w->kpad, w->kpad, w->kpad, Wd, nullptr, nullptr, 0, SS_EPI_NONE,
                       dtype, s)))
        return rc;
    if ((rc = ss_add_bcast(y, w->pos, y, batch, L, Wd, L * Wd, dtype, stream))) return rc;
    if ((rc = ss_layernorm(y, w->ln_pre_w, w->ln_pre_b, x, rows, Wd, w->ln_eps, dtype, stream))) return rc;
    if ((rc = vit_blocks(w, x, y, qkv, ctx, hm, batch, L, 0, w->n_layers, dtype, stream))) return rc;
    SS_HIP(hipMemcpyAsync(out, x, rows * Wd * e, hipMemcpyDeviceToDevice, s));
    return SS_OK;
}

int ss_vit_blocks(const ss_vit_weights* w, void* x, int64_t batch, int64_t tokens, int64_t layer0, int64_t n_layers,
                  void* workspace, size_t workspace_bytes, int dtype, void* stream) {
    SS_REQUIRE(w && x && workspace && batch > 0 && tokens > 0, "vit_blocks: bad arguments");
    SS_REQUIRE(layer0 >= 0 && n_layers >= 0 && layer0 + n_layers <= w->n_layers, "vit_blocks: layer range");
    SS_REQUIRE(w->width % w->n_heads == 0, "vit_blocks: bad geometry");
    const size_t e = dtype_size(dtype);
    const size_t rows = (size_t)batch * tokens, Wd = w->width;
    auto up = [](size_t b) { return (b + 255) / 256 * 256; };
    const size_t need = up(rows * Wd * e) + up(rows * 3 * Wd * e) + up(rows * Wd * e) + up(rows * w->mlp_width * e);
    SS_REQUIRE(workspace_bytes >= need, "vit_blocks: workspace too small");
    Bump b{(char*)workspace, 0, workspace_bytes};
    void* y = b.take(rows * Wd * e);
    void* qkv = b.take(rows * 3 * Wd * e);
    void* ctx = b.take(rows * Wd * e);
    void* hm = b.take(rows * w->mlp_width * e);
    return vit_blocks(w, x, y, qkv, ctx, hm, batch, tokens, layer0, n_layers, dtype, stream);
}

}  // extern "C"
