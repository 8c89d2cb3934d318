// Native LLaMA-2 decoder engine for the SEED-Story MLLM (replaces, for inference,
// LlamaModel.forward / LlamaForCausalLM.forward / prepare_inputs_for_generation of
// src/models_clm/modeling_llama_xformer.py:532-852 and the HF greedy loop around them).
//
//  * KV cache lives in one preallocated slab  K,V : [n_layers][n_heads][cache_cap][hd]  — the
//    reference's per-layer (k, v) [1, n_heads, len, hd] tuples (keys post-RoPE) are *views* of
//    it; no per-token torch.cat (:239-242 copies O(S) per token per layer).
//  * prefill / continuation (q_len = M rows against the cached prefix): host loop over layers,
//    MFMA GEMMs + flash attention with the bottom-right causal mask.
//  * decode: ONE token = sample -> embed -> 32 x {GEMV(qkv, fused RMSNorm) -> RoPE+append ->
//    split-KV attention -> GEMV(o)+residual -> GEMV(gate|up, fused RMSNorm, SiLU*mul) ->
//    GEMV(down)+residual} -> final norm -> GEMV(lm_head), captured once into a hipGraph.  All
//    per-token scalars (kv_len, rope position, last token id, EOS flag) live in device memory, so
//    the graph replays without host round trips; the reference syncs the host every token
//    (`.item()` in generation.py:22, EOS check in HF).
//  * option (ss_llama_set_kv8, off by default): the attention of the decode token reads an fp8 (e4m3) SHADOW of the slab (caller-owned
//    code + scale planes, ss_attn_kv8.hip) and appends to both; the slab stays the truth for everything else.  A host-side
//    watermark per slot says how many shadow rows are valid; the decode entry points quantise the rest in one launch up front.
//  * slot fork (ss_llama_fork): one slot's cache rows, last logits, lengths and history copied to up to 7 others on the device,
//    each packet read once and written to all of them — n sampled continuations of one prompt cost one prefill.
//  * beam search (ss_llama_beam_search, ss_beam.h): slots [0, n) carry the running hypotheses; the token is opened by top-K,
//    advance and a cycle-safe permutation of the slots' cache suffixes instead of the arg max, inside the same captured graph.
//  * prompt-lookup speculative decoding (ss_llama_set_speculation, ss_spec.h, off by default): the token of ss_llama_generate forwards
//    R <= 8 rows of the one slot — the chosen token and drafted successors — through the same batched GEMVs over R row-state blocks
//    and a decode attention for R rows of one slot (ss_attn_spec.hip); the next opening kernel keeps the prefix greedy agrees with.
#include <stddef.h>
#include <string.h>

#include <vector>

#include "ss_common.h"
#include "ss_gemv.h"
#include "ss_sample.h"
#include "ss_rules.h"
#include "ss_kv8.h"
#include "ss_logprob.h"
#include "ss_beam.h"
#include "ss_spec.h"

namespace ss {

size_t gemm_splitk_workspace_bytes(int64_t M, int64_t N, int64_t K);
int gemm_splitk_dev(const void* A, const void* W, void* C, int64_t M, int64_t N, int64_t K, const void* bias,
                    const void* residual, void* ws, size_t ws_bytes, int dtype, hipStream_t s);
int gemm_dev(const void* A, const void* W, void* C, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldw,
             int64_t ldc, const void* bias, const void* residual, int64_t ldr, int epi, int dtype, hipStream_t s);
int rope_kv_append_dev(const void* qkv, void* q_out, void* kc, void* vc, const void* cos_t, const void* sin_t,
                       const int32_t* pos_ids, int64_t M, int64_t n_heads, int64_t hd, const int32_t* kv_start_dev,
                       int64_t cache_cap, int dtype, hipStream_t s);
int attn_decode_fused_dev(const void* qkv_raw, void* kc, void* vc, const void* cos_t, const void* sin_t, void* out,
                          void* ws, const int32_t* kv_len_dev, const int32_t* pos_dev, const int32_t* done_flag,
                          int64_t n_heads, int64_t hd, int64_t cache_cap, int nb, int state_stride,
                          int64_t cache_stride, int dtype, hipStream_t s);
int attn_decode_spec_dev(const void* qkv, void* kc, void* vc, const void* cos_t, const void* sin_t, void* out, void* ws,
                         const int32_t* kv_len_dev, const int32_t* pos_dev, const int32_t* n_active_dev, int rows, int64_t n_heads,
                         int64_t hd, int64_t cache_cap, int dtype, hipStream_t s);
int attn_scores_dev(const void* q, int64_t ldq, const void* k, int64_t ldk, void* out, int64_t ldo, int64_t M, int64_t kv,
                    int64_t hd, int row_calls, int dtype, hipStream_t s);
int attn_scores_decode_dev(const void* qkv_raw, const void* kplane, const void* cos_t, const void* sin_t,
                           const int32_t* kv_len_dev, const int32_t* pos_dev, const int32_t* done_flag,
                           const AttnCaptureDesc* desc, int layer, int64_t n_heads, int64_t hd, int64_t cap, int dtype,
                           hipStream_t s);

// device state words (ST_WORDS per sequence slot)
enum { ST_KV_LEN = 0, ST_POS = 1, ST_NGEN = 2, ST_DONE = 3, ST_LAST = 4, ST_NFORCED = 5, ST_LIMIT = 6, ST_EOS = 7, ST_WORDS = 8 };

// ---- engine kernels ---------------------------------------------------------------------------

// sample -> (forced?) -> append -> EOS/limit check -> embed.  One block per sequence (blockIdx.x).
template <typename T>
__global__ __launch_bounds__(1024) void sample_embed_kernel(T* logits, int vocab, int32_t* st,
                                                            const int32_t* __restrict__ img_ids, int n_img_ids,
                                                            const int32_t* __restrict__ forced, int32_t* gen_ids,
                                                            const T* __restrict__ embed, T* x, int hidden,
                                                            int max_new) {
    __shared__ float sv[16];
    __shared__ int si[16];
    {
        const int b = blockIdx.x;
        logits += (int64_t)b * vocab;
        st += b * ST_WORDS;
        forced += (int64_t)b * max_new;
        gen_ids += (int64_t)b * max_new;
        x += (int64_t)b * hidden;
    }
    if (st[ST_DONE]) return;
    int tok = imgproc_argmax_block<T>(logits, vocab, st[ST_LAST], img_ids, n_img_ids, sv, si);
    if ((unsigned)tok >= (unsigned)vocab) tok = 0;     // all-NaN logits have no maximum (torch.argmax: the first NaN): never
                                                       // index the embedding table with the sentinel
    const int n = st[ST_NGEN];
    if (n < st[ST_NFORCED]) tok = forced[n];
    // ST_EOS packs two stop ids: the EOS token in the low half and an optional second stop token + 1 in the high half
    // (ss_llama_set_stop_id: the drivers stop at <img> to run the processor-forced image tokens as one batched forward)
    const int eos_word = st[ST_EOS];
    const int eos_id = eos_word & 0xFFFF, stop2 = (eos_word >> 16) - 1;
    const bool stop = (tok == eos_id) || (tok == stop2) || (n + 1 >= st[ST_LIMIT]);
    __syncthreads();
    if (threadIdx.x == 0) {
        gen_ids[n] = tok;
        st[ST_LAST] = tok;
        st[ST_NGEN] = n + 1;
        if (stop) st[ST_DONE] = 1;
    }
    if (stop) return;
    constexpr int V = Tr<T>::kVec;
    for (int p = threadIdx.x; p < hidden / V; p += blockDim.x)
        st16(x + (int64_t)p * V, ld16(embed + (int64_t)tok * hidden + (int64_t)p * V));
}

// sample_embed_kernel with the sampler in the arg max's place (chosen on the host when a slot of the launch has sampling on,
// ss_llama_set_sampling).  Per slot, from its SampleParams: sampling off -> the arg max, exactly as above; on -> the certain
// image-token successor, or one draw (Philox counter (draw, slot)); a forced token wins over either and takes no draw.
// LP (chosen on the host when a slot of the launch records log-probabilities, ss_llama_set_logprobs): the same kernel, which
// also leaves log(w_tok / Z_P) of a drawn token, from the draw's own kept set, in the slot's LogprobScratch.
template <typename T, int NS, bool LP>
__global__ __launch_bounds__(1024) void sample_embed_draw_kernel(T* logits, int vocab, int32_t* st, SampleParams* samp, int seq0,
                                                                 const int32_t* __restrict__ img_ids, int n_img_ids,
                                                                 const int32_t* __restrict__ forced, int32_t* gen_ids,
                                                                 const T* __restrict__ embed, T* x, int hidden,
                                                                 int max_new, LogprobScratch* lps) {
    __shared__ float sv[16];
    __shared__ int si[16];
    __shared__ SampleSmem sm;
    {
        const int b = blockIdx.x;
        logits += (int64_t)b * vocab;
        st += b * ST_WORDS;
        samp += b;
        forced += (int64_t)b * max_new;
        gen_ids += (int64_t)b * max_new;
        x += (int64_t)b * hidden;
    }
    if (st[ST_DONE]) return;
    const SampleParams sp = *samp;
    const int n = st[ST_NGEN];
    const bool is_forced = n < st[ST_NFORCED];
    int tok, drew = 0;
    float lp = 0.f;
    if (!sp.enabled || is_forced) {     // (uniform over the block) the greedy kernel's path; a forced token overrides its result
        tok = imgproc_argmax_block<T>(logits, vocab, st[ST_LAST], img_ids, n_img_ids, sv, si);
        if ((unsigned)tok >= (unsigned)vocab) tok = 0;
        if (is_forced) tok = forced[n];
    } else {
        int nk;
        const float u = philox_uniform(sp.seed_lo, sp.seed_hi, sp.draw, (uint32_t)(seq0 + blockIdx.x));
        tok = imgproc_sample_block<T, NS, LP>(logits, vocab, true, st[ST_LAST], img_ids, n_img_ids, sp.inv_temp, sp.top_p, sp.top_k,
                                              u, sv, si, sm, &nk, &drew, &lp);
    }
    const int eos_word = st[ST_EOS];
    const int eos_id = eos_word & 0xFFFF, stop2 = (eos_word >> 16) - 1;
    const bool stop = (tok == eos_id) || (tok == stop2) || (n + 1 >= st[ST_LIMIT]);
    __syncthreads();
    if (threadIdx.x == 0) {
        gen_ids[n] = tok;
        st[ST_LAST] = tok;
        st[ST_NGEN] = n + 1;
        if (stop) st[ST_DONE] = 1;
        if (drew) samp->draw = sp.draw + 1;
        if (LP && drew) lps[blockIdx.x].samp_lp = lp;
    }
    if (stop) return;
    constexpr int V = Tr<T>::kVec;
    for (int p = threadIdx.x; p < hidden / V; p += blockDim.x)
        st16(x + (int64_t)p * V, ld16(embed + (int64_t)tok * hidden + (int64_t)p * V));
}

// Token log-probabilities in the decode loop (ss_llama_set_logprobs): two small kernels, one block per slot, launched only when
// a slot of the launch records; a slot that does not (or is done) returns at once and writes nothing.
//   logprob_raw_kernel   IN FRONT of the rules kernel: the lm_head row is still `raw`.  Its stats and the top-n go out here
//                        (entry n = ST_NGEN, the entry the opening kernel is about to fill); the row itself is copied to the
//                        slot's scratch row, because raw[tok] is wanted once tok is known and the rules and the processor
//                        edit the row in place before that.
//   logprob_tok_kernel   BEHIND the opening kernel: tok = gen_ids[n], the row holds z.  model_logprob from the copy; logprob =
//                        0 for a forced token and for the certain image-token successor, the sampling kernel's own value
//                        for a drawn token, the log-softmax of z for a greedy one.
template <typename T, int EPT>
__global__ __launch_bounds__(1024) void logprob_raw_kernel(const T* logits, int vocab, const int32_t* st, const LogprobDesc* desc,
                                                           LogprobScratch* lps, T* raw_copy, int max_new) {
    __shared__ LogprobSmem sm;
    {
        const int b = blockIdx.x;
        logits += (int64_t)b * vocab;
        st += b * ST_WORDS;
        desc += b;
        lps += b;
        raw_copy += (int64_t)b * vocab;
    }
    const LogprobDesc d = *desc;
    if (!d.on) return;
    const int n = st[ST_NGEN];
    if (st[ST_DONE] || n >= max_new) {
        if (threadIdx.x == 0) lps->live = 0;
        return;
    }
    float v[EPT];
    int flip = 0;
    const LogprobStats s = logprob_load_block<T, EPT>(logits, vocab, v, sm, flip);
    for (int i = threadIdx.x; i < vocab; i += 1024) raw_copy[i] = logits[i];
    if (threadIdx.x == 0) {
        lps->zmax = s.zmax; lps->logz = s.logz; lps->any = s.any;
        lps->n = n; lps->last = st[ST_LAST]; lps->live = 1;
    }
    if (d.top_n > 0)
        logprob_top_block(v, vocab, s, d.top_n, d.top_ids + (int64_t)n * d.top_n, d.top_lp + (int64_t)n * d.top_n, sm);
}

template <typename T, int EPT>
__global__ __launch_bounds__(1024) void logprob_tok_kernel(const T* logits, int vocab, const int32_t* st, const LogprobDesc* desc,
                                                           const LogprobScratch* lps, const T* raw_copy,
                                                           const SampleParams* __restrict__ samp,
                                                           const int32_t* __restrict__ img_ids, int n_img_ids,
                                                           const int32_t* __restrict__ gen_ids, int max_new) {
    __shared__ LogprobSmem sm;
    {
        const int b = blockIdx.x;
        logits += (int64_t)b * vocab;
        st += b * ST_WORDS;
        desc += b;
        lps += b;
        raw_copy += (int64_t)b * vocab;
        samp += b;
        gen_ids += (int64_t)b * max_new;
    }
    const LogprobDesc d = *desc;
    if (!d.on) return;
    const LogprobScratch sc = *lps;
    if (!sc.live) return;
    const int n = sc.n, tok = gen_ids[n];
    const bool in_row = (unsigned)tok < (unsigned)vocab;
    const float nan = __uint_as_float(0x7FC00000u);
    // the policy's part (every condition is uniform over the block)
    int succ = -1;
    for (int j = 0; j + 1 < n_img_ids; ++j)
        if (img_ids[j] == sc.last) { succ = img_ids[j + 1]; break; }
    float plp;
    if (n < st[ST_NFORCED] || (succ >= 0 && succ < vocab)) plp = 0.f;
    else if (samp->enabled) plp = sc.samp_lp;
    else {
        float v[EPT];
        int flip = 0;
        const LogprobStats s = logprob_load_block<T, EPT>(logits, vocab, v, sm, flip);
        plp = in_row ? logprob_value(Tr<T>::ld(logits + tok), s) : nan;
    }
    if (threadIdx.x == 0) {
        const LogprobStats rs{sc.zmax, sc.logz, sc.any};
        d.model_lp[n] = in_row ? logprob_value(Tr<T>::ld(raw_copy + tok), rs) : nan;
        d.policy_lp[n] = plp;
    }
}

// The history rules of a decode token (ss_llama_set_logits_rules), one block per slot IN FRONT of the opening kernel, which
// stays as it is: launched only when a slot of the launch has rules on; a slot without them returns at once.  The opening
// kernel of the previous token left its choice in gen_ids[ST_NGEN - 1]: it is appended to the history (and its bit set in the
// slot's bitmap, an ordinary store by the one thread that appends) here, before the rules read the history, so the history
// is hist_at_call_start + every token of this call.  flush = 1 (after the last token of a generate call): append only — the
// token that ended the call has no next decode token to append it.
template <typename T>
__global__ __launch_bounds__(1024) void logits_rules_kernel(T* logits, int vocab, const int32_t* st, RulesState* rs, int32_t* hist,
                                                            int hist_cap, uint32_t* bitmap, int bm_words,
                                                            const int32_t* __restrict__ gen_ids, int max_new,
                                                            const int32_t* __restrict__ img_ids, int n_img_ids, int flush) {
    __shared__ int s_len;
    {
        const int b = blockIdx.x;
        logits += (int64_t)b * vocab;
        st += b * ST_WORDS;
        rs += b;
        hist += (int64_t)b * hist_cap;
        bitmap += (int64_t)b * bm_words;
        gen_ids += (int64_t)b * max_new;
    }
    if (!rs->enabled) return;
    if (!flush && st[ST_DONE]) return;
    const int n = st[ST_NGEN];
    if (threadIdx.x == 0) {
        int na = n == 0 ? 0 : rs->n_app, len = rs->hist_len;
        for (; na < n && na < max_new; ++na) {
            const int tok = gen_ids[na];
            if (len >= hist_cap) continue;      // (the host refuses a call that could get here)
            hist[len++] = tok;
            if ((unsigned)tok < (unsigned)vocab) bitmap[tok >> 5] |= 1u << (tok & 31);
        }
        rs->n_app = na;
        rs->hist_len = len;
        s_len = len;
    }
    __threadfence_block();
    __syncthreads();
    if (flush) return;
    const int eos = st[ST_EOS] & 0xFFFF;        // 0xFFFF = none: never below vocab (<= 65535)
    logits_rules_block<T>(logits, vocab, rs->penalty, rs->ngram, rs->min_new, rs->spare_img != 0, bitmap, hist, s_len,
                          rs->prompt_len, eos, img_ids, n_img_ids);
}

// the bitmap of a history handed over by the host: the words of ids[0 .. n) rebuilt (keep = 0) or extended, one thread per word
__global__ __launch_bounds__(256) void rules_bitmap_kernel(uint32_t* bitmap, int bm_words, const int32_t* __restrict__ ids, int n,
                                                           int keep) {
    rules_bitmap_add(bitmap, bm_words, blockIdx.x * 256 + threadIdx.x, gridDim.x * 256, ids, n, keep != 0);
}

// final RMSNorm of the single decode row: writes the fixed lm_head input buffer AND the
// hidden-state ring row (n_gen - 1), then advances kv_len / pos.  One block of 256 per sequence.
template <typename T>
__global__ __launch_bounds__(256) void final_norm_advance_kernel(const T* __restrict__ x, const T* __restrict__ w,
                                                                 T* xn, T* hid_rows, int32_t* st, int hidden,
                                                                 float eps, int max_new) {
    constexpr int V = Tr<T>::kVec;
    __shared__ float red[16];
    {
        const int b = blockIdx.x;
        x += (int64_t)b * hidden;
        xn += (int64_t)b * hidden;
        hid_rows += (int64_t)b * max_new * hidden;
        st += b * ST_WORDS;
    }
    if (st[ST_DONE]) return;
    const int npack = hidden / V;
    float ssq = 0.f;
    for (int p = threadIdx.x; p < npack; p += 256) {
        float f[V];
        unpack<T>(ld16(x + (int64_t)p * V), f);
#pragma unroll
        for (int j = 0; j < V; ++j) ssq = fmaf(f[j], f[j], ssq);
    }
    const float rstd = 1.0f / sqrtf(block_sum(ssq, red) / (float)hidden + eps);
    T* row = hid_rows + (int64_t)(st[ST_NGEN] - 1) * hidden;
    for (int p = threadIdx.x; p < npack; p += 256) {
        float f[V], g[V];
        unpack<T>(ld16(x + (int64_t)p * V), f);
        unpack<T>(ld16(w + (int64_t)p * V), g);
#pragma unroll
        for (int j = 0; j < V; ++j) f[j] = g[j] * Tr<T>::rnd(f[j] * rstd);
        const uint4 o = pack<T>(f);
        st16(xn + (int64_t)p * V, o);
        st16(row + (int64_t)p * V, o);
    }
    __syncthreads();
    if (threadIdx.x == 0) { st[ST_KV_LEN] += 1; st[ST_POS] += 1; }
}

__global__ void set_state_kernel(int32_t* st, int idx0, int v0, int idx1, int v1) {
    if (threadIdx.x == 0) { st[idx0] = v0; if (idx1 >= 0) st[idx1] = v1; }
}

// dst[h][i][:] = src[h][keep[i]][:]  (one head-plane of the cache -> packed scratch)
template <typename T>
__global__ __launch_bounds__(256) void kv_gather_kernel(const T* __restrict__ src, T* __restrict__ dst,
                                                        const int32_t* __restrict__ keep, int n_keep, int cap,
                                                        int hd, int dst_cap) {
    constexpr int V = Tr<T>::kVec;
    const int h = blockIdx.y;
    const int ppr = hd / V;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < (int64_t)n_keep * ppr;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int r = (int)(i / ppr), p = (int)(i % ppr);
        const int srow = keep ? keep[r] : r;
        st16(dst + ((int64_t)h * dst_cap + r) * hd + p * V, ld16(src + ((int64_t)h * cap + srow) * hd + p * V));
    }
}

// ---- slot fork (ss_llama_fork) -------------------------------------------------------------------
// The destination list travels by value: at most n_seq - 1 = 7 slots.
constexpr int kForkMaxDst = 7;
constexpr int kForkPackets = 4;         // packets per thread: all loaded before the first store
struct ForkDst {
    int32_t n;
    int32_t slot[kForkMaxDst];
};

// One plane kind of every slot, [n_seq][units][unit_stride] packets P, twice (K | V: blockIdx.z picks the slab).  Unit
// blockIdx.y (layer, head) of slot `src`, packets [0, span): each is loaded ONCE and stored to every destination — read once,
// write n.  The valid rows of a (layer, head) are one contiguous run, so lanes walk consecutive packets: 16 B per lane, 1 KiB per
// wave and instruction for P = uint4.  256 x kForkPackets packets per block; the loads are independent and issued together.
template <typename P>
__global__ __launch_bounds__(256) void fork_planes_kernel(P* plane0, P* plane1, int64_t slot_stride, int64_t unit_stride,
                                                          int64_t span, int src, ForkDst d) {
    P* base = blockIdx.z ? plane1 : plane0;
    const int64_t unit = (int64_t)blockIdx.y * unit_stride;
    const P* __restrict__ s = base + (int64_t)src * slot_stride + unit;
    const int64_t i0 = (int64_t)blockIdx.x * (256 * kForkPackets) + threadIdx.x;
    P v[kForkPackets];
#pragma unroll
    for (int u = 0; u < kForkPackets; ++u) {
        const int64_t i = i0 + u * 256;
        if (i < span) v[u] = s[i];
    }
#pragma unroll
    for (int j = 0; j < kForkMaxDst; ++j) {
        if (j >= d.n) break;
        P* o = base + (int64_t)d.slot[j] * slot_stride + unit;
#pragma unroll
        for (int u = 0; u < kForkPackets; ++u) {
            const int64_t i = i0 + u * 256;
            if (i < span) o[i] = v[u];
        }
    }
}

// The small per-slot pieces of a fork, one launch: the last-token logits row, the history (its device-side length), the rule-1
// bitmap, and the words a later call reads (kv_len, pos, last id; hist_len, prompt_len, n_app).  Each element is read once and
// stored to every destination.  What belongs to the slot (rule parameters, `enabled`, the other state words) stays.
template <typename T>
__global__ __launch_bounds__(256) void fork_state_kernel(T* logits, int vocab, int32_t* st, RulesState* rules, int32_t* hist,
                                                         int64_t hist_cap, uint32_t* bitmap, int bm_words, int src, ForkDst d) {
    const int tid = blockIdx.x * 256 + threadIdx.x, nth = gridDim.x * 256;
    int hl = rules[src].hist_len;
    hl = hl < 0 ? 0 : (hl > hist_cap ? (int)hist_cap : hl);
    for (int i = tid; i < vocab; i += nth) {
        const T v = logits[(int64_t)src * vocab + i];
#pragma unroll
        for (int j = 0; j < kForkMaxDst; ++j)
            if (j < d.n) logits[(int64_t)d.slot[j] * vocab + i] = v;
    }
    for (int i = tid; i < hl; i += nth) {
        const int32_t v = hist[(int64_t)src * hist_cap + i];
#pragma unroll
        for (int j = 0; j < kForkMaxDst; ++j)
            if (j < d.n) hist[(int64_t)d.slot[j] * hist_cap + i] = v;
    }
    for (int i = tid; i < bm_words; i += nth) {
        const uint32_t v = bitmap[(int64_t)src * bm_words + i];
#pragma unroll
        for (int j = 0; j < kForkMaxDst; ++j)
            if (j < d.n) bitmap[(int64_t)d.slot[j] * bm_words + i] = v;
    }
    if (tid == 0) {
        const int32_t* ss = st + src * ST_WORDS;
        const int32_t kv = ss[ST_KV_LEN], pos = ss[ST_POS], last = ss[ST_LAST];
        const int32_t pl = rules[src].prompt_len, na = rules[src].n_app;
#pragma unroll
        for (int j = 0; j < kForkMaxDst; ++j)
            if (j < d.n) {
                int32_t* sd = st + d.slot[j] * ST_WORDS;
                sd[ST_KV_LEN] = kv; sd[ST_POS] = pos; sd[ST_LAST] = last;
                RulesState* rd = rules + d.slot[j];
                rd->hist_len = hl; rd->prompt_len = pl; rd->n_app = na;
            }
    }
}

int rmsnorm_rows(const void* x, const void* w, void* y, int64_t rows, int64_t cols, float eps, int dtype,
                 hipStream_t s) {
    return ss_rmsnorm(x, w, y, rows, cols, eps, dtype, (void*)s);
}

}  // namespace ss

using namespace ss;

struct ss_llama;
// one projection of the prefill paths: C [M, N] = A [M, K] W^T (+ residual).  128 < M <= 512 rows (the stacked image-token
// block, the first prompts) take the split-K weight-streaming path when the engine carved a partial-sum workspace for it.
static int prefill_proj(void* splitk_ws, size_t splitk_bytes, const void* A, const void* W, void* C, int64_t M, int64_t N,
                        int64_t K, const void* residual, int dt, hipStream_t s) {
    if (splitk_ws && M > 128 && M <= 512)
        return gemm_splitk_dev(A, W, C, M, N, K, nullptr, residual, splitk_ws, splitk_bytes, dt, s);
    return gemm_dev(A, W, C, M, N, K, K, K, N, nullptr, residual, N, residual ? SS_EPI_RESIDUAL : SS_EPI_NONE, dt, s);
}

struct SeqGraph {
    int seq0, nb;
    int mode;                // arithmetic knobs the captured kernels were chosen under (gemm_f32_split): part of the cache key
    int capture;             // attention-map capture on: one more launch per layer (a different graph; the buffer is NOT part of the key)
    int w8;                  // 1 = fp8 decode weights on (ss_llama_set_decode_w8), 2 = MXFP4 ones (ss_llama_set_decode_mx4): other
                             // kernels, other weight pointers
    int sampling;            // a slot of [seq0, seq0+nb) has sampling on (ss_llama_set_sampling): the sampling kernel opens the token
    int rules;               // a slot of [seq0, seq0+nb) has history rules on (ss_llama_set_logits_rules): the rules kernel in front
    int kv8;                 // fp8 KV shadow on (ss_llama_set_kv8): another attention kernel, the planes' pointers
    int logprobs;            // a slot of [seq0, seq0+nb) records log-probabilities (ss_llama_set_logprobs): two more kernels; the buffers are NOT part of the key
    int beam;                // beam search (ss_llama_beam_search): other opening kernels; 0 = none, else n_steps * 16 + n (the permute's grid)
    void* beam_ws;           // ... over this workspace (its pointers are kernel arguments)
    int spec;                // speculative token (ss_llama_set_speculation): other kernels at nb = rows; 0 = plain, else the row count
    void* spec_ws;           // ... over this workspace (its pointers are kernel arguments; the parameters live in its header)
    hipGraph_t graph;
    hipGraphExec_t exec;
};

struct ss_llama {
    ss_llama_config cfg;
    ss_llama_weights w;
    std::vector<ss_llama_layer_weights> layers;
    int hd;
    int n_seq;               // sequence slots (independent stories sharing one sweep of the weights)
    int cur;                 // slot addressed by the single-sequence entry points
    int stop2 = -1;          // optional second stop token of the decode loop (-1 = none), ss_llama_set_stop_id
    int64_t max_rows;
    size_t esz;
    // device buffers (carved from the caller's workspace); every per-sequence array is [n_seq][...]
    char *kc, *vc;           // [n_seq][L][H][cap][hd]
    int32_t* state;          // [n_seq][ST_WORDS]
    int32_t* gen_ids;        // [n_seq][max_new]
    int32_t* forced;         // [n_seq][max_new]
    int32_t* img_ids;        // [n_img_ids]
    char* hid_rows;          // [n_seq][max_new][hidden]
    char* logits;            // [n_seq][vocab]
    char *x, *xn, *qkv, *q, *attn, *gu, *hm;  // activations ([max_rows][..]); decode uses rows 0..nb-1
    float* attn_ws;          // [n_seq] split-KV partial slabs
    void* splitk_ws;         // fp32 partial sums of the small-M split-K projections (128 < rows <= 512)
    size_t splitk_bytes;
    // host mirrors
    std::vector<int64_t> kv_len, pos;
    hipStream_t cap_stream;
    std::vector<SeqGraph> graphs;
    int32_t* pinned;         // [2][n_seq][ST_WORDS] ints of pinned host memory: state read-back | state upload
    // attention-map capture (ss_llama_set_attn_capture): host copy + the device descriptor the decode-token kernel reads
    AttnCaptureDesc cap = {nullptr, 0, 0, 0, 0};
    int cap_row_calls = 0;
    AttnCaptureDesc* cap_desc = nullptr;
    // fp8 decode weights (ss_llama_set_decode_w8): empty = off
    std::vector<ss_llama_layer_w8> w8;
    const void* w8_lm_head = nullptr;
    const float* w8_lm_scale = nullptr;
    // MXFP4 decode weights (ss_llama_set_decode_mx4): empty = off; never on together with the fp8 planes
    std::vector<ss_llama_layer_mx4> mx4;
    const void* mx4_lm_head = nullptr;
    const void* mx4_lm_scale = nullptr;
    int decode_weights_kind() const { return !mx4.empty() ? 2 : !w8.empty() ? 1 : 0; }
    // fp8 shadow of the KV cache (ss_llama_set_kv8): caller-owned planes, kq == NULL = off.  Invariant: shadow rows
    // [0, kv8_rows[b]) of slot b equal the quantiser applied to its 16-bit rows (host-side watermark, <= kv_len[b] wherever
    // it matters: everything that rewrites 16-bit rows below it lowers it)
    uint8_t *kq = nullptr, *vq = nullptr;      // [n_seq][L][H][cap][hd]
    float *kscale = nullptr, *vscale = nullptr;  // [n_seq][L][H][cap]
    std::vector<int64_t> kv8_rows;
    // sampling (ss_llama_set_sampling): per-slot parameters + draw counter in device memory, which slots have it on here
    SampleParams* samp = nullptr;       // [n_seq]
    std::vector<char> samp_on;
    bool sampling_in(int seq0, int nb) const {
        for (int b = seq0; b < seq0 + nb; ++b) if (samp_on[b]) return true;
        return false;
    }
    // history rules (ss_llama_set_logits_rules / ss_llama_set_history): per-slot block, history and rule-1 bitmap in device memory
    RulesState* rules = nullptr;        // [n_seq]
    int32_t* hist = nullptr;            // [n_seq][hist_cap()]
    uint32_t* hist_bm = nullptr;        // [n_seq][bm_words()]
    std::vector<char> rules_on;
    std::vector<int64_t> hist_len;      // host mirror of RulesState::hist_len
    bool rules_in(int seq0, int nb) const {
        for (int b = seq0; b < seq0 + nb; ++b) if (rules_on[b]) return true;
        return false;
    }
    // token log-probabilities (ss_llama_set_logprobs): per-slot descriptor of the caller's buffers, scratch words and raw-row copy
    LogprobDesc* lp_desc = nullptr;     // [n_seq]
    LogprobScratch* lp_scratch = nullptr;  // [n_seq]
    char* lp_raw = nullptr;             // [n_seq][vocab]
    std::vector<char> lp_on;
    bool logprobs_in(int seq0, int nb) const {
        for (int b = seq0; b < seq0 + nb; ++b) if (lp_on[b]) return true;
        return false;
    }
    // beam search (ss_llama_beam_search): the caller's workspace while a search runs, hdr == NULL otherwise
    BeamPtrs beam = {nullptr, nullptr, nullptr, nullptr, nullptr};
    int beam_rows = 0;                  // its n_steps: the suffix rows the permute's grid covers
    // speculative decoding (ss_llama_set_speculation): the caller's workspace, hdr == NULL = off
    SpecPtrs spec = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    int spec_rows = 0;
    bool spec_run = false;              // inside ss_llama_generate with the option on: decode_token takes the speculative branch
    int64_t hist_cap() const { return (int64_t)cfg.cache_cap + cfg.max_new; }
    int bm_words() const { return rules_bitmap_words(cfg.vocab); }
    size_t plane_bytes() const { return (size_t)cfg.n_heads * cfg.cache_cap * hd * esz; }       // one layer of one slot
    size_t seq_kv_bytes() const { return (size_t)cfg.n_layers * plane_bytes(); }
    int32_t* upload() const { return pinned + (size_t)n_seq * ST_WORDS; }                        // the state upload area
};

// layer `layer`'s K / V plane [n_heads][cache_cap][hd] of sequence slot `slot`
static inline char* slot_k(const ss_llama* h, int slot, int layer) {
    return h->kc + (size_t)slot * h->seq_kv_bytes() + (size_t)layer * h->plane_bytes();
}
static inline char* slot_v(const ss_llama* h, int slot, int layer) {
    return h->vc + (size_t)slot * h->seq_kv_bytes() + (size_t)layer * h->plane_bytes();
}

static size_t align_up(size_t v, size_t a = 256) { return (v + a - 1) / a * a; }

struct Carver {
    char* base; size_t off; size_t cap;
    char* take(size_t bytes) { char* p = base ? base + off : nullptr; off += align_up(bytes); return p; }
};

static void carve(ss_llama* h, Carver& c) {
    const ss_llama_config& g = h->cfg;
    const size_t e = h->esz;
    const size_t H = g.hidden, I = g.inter, R = (size_t)h->max_rows, S = (size_t)h->n_seq;
    h->kc = c.take(S * h->seq_kv_bytes());
    h->vc = c.take(S * h->seq_kv_bytes());
    h->state = (int32_t*)c.take(S * ST_WORDS * sizeof(int32_t));
    h->gen_ids = (int32_t*)c.take(S * (size_t)g.max_new * sizeof(int32_t));
    h->forced = (int32_t*)c.take(S * (size_t)g.max_new * sizeof(int32_t));
    h->img_ids = (int32_t*)c.take((size_t)(g.n_img_ids > 0 ? g.n_img_ids : 1) * sizeof(int32_t));
    h->hid_rows = c.take(S * (size_t)g.max_new * H * e);
    h->logits = c.take(S * (size_t)g.vocab * e);
    h->x = c.take(R * H * e);
    h->xn = c.take(R * H * e);
    h->qkv = c.take(R * 3 * H * e);
    h->q = c.take(R * H * e);
    h->attn = c.take(R * H * e);
    h->gu = c.take(R * 2 * I * e);
    h->hm = c.take(R * I * e);
    h->attn_ws = (float*)c.take(S * ss_attn_decode_workspace_bytes(g.n_heads, h->hd));
    // split-K partial sums: the largest need over the four projections at the largest eligible row count
    size_t sk = 0;
    if (g.dtype != SS_F32 && R > 128) {
        // S x M x N x 4 bytes is not monotone in M (the slice count S drops when another 128-row tile appears): take the
        // maximum over the upper end of every row-tile band that fits the engine, per projection
        const int64_t Mx = R < 512 ? (int64_t)R : 512;
        const int64_t shapes[4][2] = {{3 * (int64_t)H, (int64_t)H}, {(int64_t)H, (int64_t)H}, {2 * (int64_t)I, (int64_t)H}, {(int64_t)H, (int64_t)I}};
        for (auto& nk : shapes)
            for (int64_t m = 256; ; m += 128) {
                const int64_t mm = m < Mx ? m : Mx;
                const size_t b = gemm_splitk_workspace_bytes(mm, nk[0], nk[1]);
                if (b > sk) sk = b;
                if (mm == Mx) break;
            }
    }
    h->splitk_bytes = sk;
    h->splitk_ws = sk ? c.take(sk) : nullptr;
    h->cap_desc = (AttnCaptureDesc*)c.take(sizeof(AttnCaptureDesc));     // zeroed with the workspace: capture off
    h->samp = (SampleParams*)c.take(S * sizeof(SampleParams));           // zeroed with the workspace: every slot greedy
    h->rules = (RulesState*)c.take(S * sizeof(RulesState));              // zeroed with the workspace: rules off, empty histories
    h->hist = (int32_t*)c.take(S * (size_t)h->hist_cap() * sizeof(int32_t));
    h->hist_bm = (uint32_t*)c.take(S * (size_t)h->bm_words() * sizeof(uint32_t));
    h->lp_desc = (LogprobDesc*)c.take(S * sizeof(LogprobDesc));          // zeroed with the workspace: no slot records
    h->lp_scratch = (LogprobScratch*)c.take(S * sizeof(LogprobScratch));
    h->lp_raw = c.take(S * (size_t)g.vocab * e);
}

static int cfg_n_seq(const ss_llama_config* cfg) { return cfg->n_seq > 0 ? cfg->n_seq : 1; }

// one decode token (sample+forward) for the sequence slots [seq0, seq0+nb); eager or under stream
// capture.  `prof` (optional) receives an event before/after every launch class for profiling.
struct ProfSink {
    std::vector<hipEvent_t> ev;
    std::vector<int> cls;
    hipStream_t s;
    void mark(int c) {
        hipEvent_t e;
        hipEventCreate(&e);
        hipEventRecord(e, s);
        ev.push_back(e);
        cls.push_back(c);
    }
};

template <typename T>
static int sample_embed_launch(ss_llama* h, int seq0, int nb, hipStream_t s) {
    const ss_llama_config& g = h->cfg;
    hipLaunchKernelGGL(sample_embed_kernel<T>, dim3((unsigned)nb), dim3(1024), 0, s, (T*)h->logits + (size_t)seq0 * g.vocab,
                       g.vocab, h->state + (size_t)seq0 * ST_WORDS, h->img_ids, g.n_img_ids,
                       h->forced + (size_t)seq0 * g.max_new, h->gen_ids + (size_t)seq0 * g.max_new, (const T*)h->w.embed,
                       (T*)h->x, g.hidden, g.max_new);
    SS_LAUNCH_CHECK("sample_embed");
    return SS_OK;
}

template <typename T>
static int sample_embed_draw_launch(ss_llama* h, int seq0, int nb, bool lp, hipStream_t s) {
    const ss_llama_config& g = h->cfg;
#define SS_DRAW_ARGS dim3((unsigned)nb), dim3(1024), 0, s, (T*)h->logits + (size_t)seq0 * g.vocab, g.vocab,                        \
                     h->state + (size_t)seq0 * ST_WORDS, h->samp + seq0, seq0, h->img_ids, g.n_img_ids,                            \
                     h->forced + (size_t)seq0 * g.max_new, h->gen_ids + (size_t)seq0 * g.max_new, (const T*)h->w.embed, (T*)h->x,  \
                     g.hidden, g.max_new, h->lp_scratch + seq0
    const bool half = sample_ns_half_fits(g.vocab);
    if (half && lp) hipLaunchKernelGGL((sample_embed_draw_kernel<T, sample_ns_full<T>() / 2, true>), SS_DRAW_ARGS);
    else if (half) hipLaunchKernelGGL((sample_embed_draw_kernel<T, sample_ns_full<T>() / 2, false>), SS_DRAW_ARGS);
    else if (lp) hipLaunchKernelGGL((sample_embed_draw_kernel<T, sample_ns_full<T>(), true>), SS_DRAW_ARGS);
    else hipLaunchKernelGGL((sample_embed_draw_kernel<T, sample_ns_full<T>(), false>), SS_DRAW_ARGS);
#undef SS_DRAW_ARGS
    SS_LAUNCH_CHECK("sample_embed_draw");
    return SS_OK;
}

template <typename T>
static int logprob_raw_launch(ss_llama* h, int seq0, int nb, hipStream_t s) {
    const ss_llama_config& g = h->cfg;
#define SS_LP_RAW_ARGS dim3((unsigned)nb), dim3(1024), 0, s, (const T*)h->logits + (size_t)seq0 * g.vocab, g.vocab,                   \
                       h->state + (size_t)seq0 * ST_WORDS, h->lp_desc + seq0, h->lp_scratch + seq0,                               \
                       (T*)h->lp_raw + (size_t)seq0 * g.vocab, g.max_new
    if (logprob_ept_half_fits(g.vocab)) hipLaunchKernelGGL((logprob_raw_kernel<T, kLpEptFull / 2>), SS_LP_RAW_ARGS);
    else hipLaunchKernelGGL((logprob_raw_kernel<T, kLpEptFull>), SS_LP_RAW_ARGS);
#undef SS_LP_RAW_ARGS
    SS_LAUNCH_CHECK("logprob_raw");
    return SS_OK;
}

template <typename T>
static int logprob_tok_launch(ss_llama* h, int seq0, int nb, hipStream_t s) {
    const ss_llama_config& g = h->cfg;
#define SS_LP_TOK_ARGS dim3((unsigned)nb), dim3(1024), 0, s, (const T*)h->logits + (size_t)seq0 * g.vocab, g.vocab,                   \
                       h->state + (size_t)seq0 * ST_WORDS, h->lp_desc + seq0, h->lp_scratch + seq0,                               \
                       (const T*)h->lp_raw + (size_t)seq0 * g.vocab, h->samp + seq0, h->img_ids, g.n_img_ids,                    \
                       h->gen_ids + (size_t)seq0 * g.max_new, g.max_new
    if (logprob_ept_half_fits(g.vocab)) hipLaunchKernelGGL((logprob_tok_kernel<T, kLpEptFull / 2>), SS_LP_TOK_ARGS);
    else hipLaunchKernelGGL((logprob_tok_kernel<T, kLpEptFull>), SS_LP_TOK_ARGS);
#undef SS_LP_TOK_ARGS
    SS_LAUNCH_CHECK("logprob_tok");
    return SS_OK;
}

template <typename T>
static int logits_rules_launch(ss_llama* h, int seq0, int nb, int flush, hipStream_t s) {
    const ss_llama_config& g = h->cfg;
    hipLaunchKernelGGL(logits_rules_kernel<T>, dim3((unsigned)nb), dim3(1024), 0, s, (T*)h->logits + (size_t)seq0 * g.vocab, g.vocab,
                       h->state + (size_t)seq0 * ST_WORDS, h->rules + seq0, h->hist + (size_t)seq0 * h->hist_cap(), (int)h->hist_cap(),
                       h->hist_bm + (size_t)seq0 * h->bm_words(), h->bm_words(), h->gen_ids + (size_t)seq0 * g.max_new, g.max_new,
                       h->img_ids, g.n_img_ids, flush);
    SS_LAUNCH_CHECK("logits_rules");
    return SS_OK;
}

template <typename T>
static int final_norm_advance_launch(ss_llama* h, int seq0, int nb, hipStream_t s) {
    const ss_llama_config& g = h->cfg;
    hipLaunchKernelGGL(final_norm_advance_kernel<T>, dim3((unsigned)nb), dim3(256), 0, s, (const T*)h->x,
                       (const T*)h->w.final_norm, (T*)h->xn, (T*)h->hid_rows + (size_t)seq0 * g.max_new * g.hidden,
                       h->state + (size_t)seq0 * ST_WORDS, g.hidden, g.rms_eps, g.max_new);
    SS_LAUNCH_CHECK("final_norm_advance");
    return SS_OK;
}

static const BeamSt kBeamSt = {ST_KV_LEN, ST_NGEN, ST_DONE, ST_LAST, ST_WORDS};

// the cache permutation of a beam step (+ the history's when rules are on): slots [0, n), suffix rows up to `rows`
static int beam_permute_launch(ss_llama* h, int rows, bool rules, hipStream_t s) {
    const ss_llama_config& g = h->cfg;
    const int ppr = (int)((size_t)h->hd * h->esz / 16);
    const int64_t units = (int64_t)g.n_layers * g.n_heads, unit_stride = (int64_t)g.cache_cap * ppr;
    hipLaunchKernelGGL(beam_permute_kernel, dim3((unsigned)cdiv((int64_t)rows * ppr, 256), (unsigned)units, 2), dim3(256), 0, s,
                       (uint4*)h->kc, (uint4*)h->vc, units * unit_stride, unit_stride, ppr, h->state, kBeamSt, h->beam.hdr);
    SS_LAUNCH_CHECK("beam_permute");
    if (rules) {
        const int m = h->bm_words() > rows ? h->bm_words() : rows;
        hipLaunchKernelGGL(beam_hist_permute_kernel, dim3((unsigned)cdiv(m, 256)), dim3(256), 0, s, h->hist, h->hist_cap(), h->hist_bm,
                           h->bm_words(), &h->rules[0].hist_len, h->state, kBeamSt, h->beam.hdr);
        SS_LAUNCH_CHECK("beam_hist_permute");
    }
    return SS_OK;
}

// the opening of a beam-search token for slots [0, n): top-K per row, advance, permute
template <typename T>
static int beam_open_launch(ss_llama* h, int n, bool rules, hipStream_t s) {
    const ss_llama_config& g = h->cfg;
#define SS_BEAM_TOPK_ARGS dim3((unsigned)n), dim3(1024), 0, s, (T*)h->logits, g.vocab, h->state, kBeamSt, h->img_ids, g.n_img_ids,   \
                          h->beam.hdr, h->beam.cand_score, h->beam.cand_tok
    if (logprob_ept_half_fits(g.vocab)) hipLaunchKernelGGL((beam_topk_kernel<T, kLpEptFull / 2>), SS_BEAM_TOPK_ARGS);
    else hipLaunchKernelGGL((beam_topk_kernel<T, kLpEptFull>), SS_BEAM_TOPK_ARGS);
#undef SS_BEAM_TOPK_ARGS
    SS_LAUNCH_CHECK("beam_topk");
    hipLaunchKernelGGL(beam_advance_kernel<T>, dim3(1), dim3(1024), 0, s, h->beam.hdr, h->beam.cand_score, h->beam.cand_tok,
                       h->beam.run_seq, h->beam.fin_seq, h->state, kBeamSt, h->gen_ids, (const T*)h->w.embed, (T*)h->x, g.hidden);
    SS_LAUNCH_CHECK("beam_advance");
    return beam_permute_launch(h, h->beam_rows, rules, s);
}

static const SpecSt kSpecSt = {ST_KV_LEN, ST_POS, ST_NGEN, ST_DONE, ST_LAST, ST_NFORCED, ST_LIMIT, ST_EOS, ST_WORDS};

// the opening of a speculative step for slot `q`: settle, emit, draft, row states, embed
template <typename T>
static int spec_open_launch(ss_llama* h, int q, hipStream_t s) {
    const ss_llama_config& g = h->cfg;
    hipLaunchKernelGGL(spec_open_kernel<T>, dim3(1), dim3(1024), 0, s, (T*)h->logits + (size_t)q * g.vocab, (const T*)h->spec.logits,
                       g.vocab, h->state + (size_t)q * ST_WORDS, kSpecSt, h->spec.hdr, h->spec.row_st, h->img_ids, g.n_img_ids,
                       h->forced + (size_t)q * g.max_new, h->gen_ids + (size_t)q * g.max_new, h->hist + (size_t)q * h->hist_cap(),
                       (int)h->hist_cap(), &h->rules[q].hist_len, &h->rules[q].n_app, h->hist_bm + (size_t)q * h->bm_words(),
                       (const T*)h->w.embed, (T*)h->spec.x, g.hidden, g.max_new, g.cache_cap, g.max_pos);
    SS_LAUNCH_CHECK("spec_open");
    return SS_OK;
}

template <typename T>
static int spec_final_norm_launch(ss_llama* h, int q, hipStream_t s) {
    const ss_llama_config& g = h->cfg;
    hipLaunchKernelGGL(spec_final_norm_kernel<T>, dim3((unsigned)h->spec_rows), dim3(256), 0, s, (const T*)h->spec.x,
                       (const T*)h->w.final_norm, (T*)h->spec.xn, (T*)h->hid_rows + (size_t)q * g.max_new * g.hidden, h->spec.hdr,
                       g.hidden, g.rms_eps, g.max_new);
    SS_LAUNCH_CHECK("spec_final_norm");
    return SS_OK;
}

static int decode_token(ss_llama* h, hipStream_t s, ProfSink* prof, int seq0, int nb) {
    const ss_llama_config& g = h->cfg;
    const int dt = g.dtype;
    const int H = g.hidden, I = g.inter, hd = h->hd;
    const size_t e = h->esz;
    int32_t* st = h->state + (size_t)seq0 * ST_WORDS;
    // a speculative step of ss_llama_generate: the launchers below run at nb = rows over the row-state blocks and the workspace's
    // activation rows (off, the default: nothing below changes)
    const bool spec = h->spec_run && h->spec.hdr && nb == 1;
    const int nslots = nb;      // the slots of the launch; nb: the rows its GEMVs serve
    if (spec) nb = h->spec_rows;
    char *const ax = spec ? h->spec.x : h->x, *const axn = spec ? h->spec.xn : h->xn, *const aqkv = spec ? h->spec.qkv : h->qkv;
    char *const aattn = spec ? h->spec.attn : h->attn, *const ahm = spec ? h->spec.hm : h->hm;
    const int32_t* done = (spec ? h->spec.row_st : st) + ST_DONE;
    const int64_t cache_stride = (int64_t)(h->seq_kv_bytes() / e);
    char* logits = spec ? h->spec.logits : h->logits + (size_t)seq0 * g.vocab * e;
    float* attn_ws = (float*)((char*)h->attn_ws + (size_t)seq0 * ss_attn_decode_workspace_bytes(g.n_heads, hd));
    int rc;
    // the five decode projections: the 16-bit weights, their fp8 planes + row scales while ss_llama_set_decode_w8 is on, or their
    // MXFP4 code + block-scale planes while ss_llama_set_decode_mx4 is
    const int wq = h->decode_weights_kind();
    static_assert(GEMV_WQ_FP8 == 1 && GEMV_WQ_MXFP4 == 2, "decode_weights_kind() is the GEMV's weight format");
    struct QPlanes { const void *codes, *scales; };
    auto proj = [&](const void* W, QPlanes q, const char* x, char* y, int64_t N, int64_t K, const void* norm_w, const void* residual, int epi,
                    int64_t y_ld, int64_t res_ld) {
        if (wq) return gemv_wq_batched_dev(wq, q.codes, q.scales, x, y, N, K, norm_w, g.rms_eps, nullptr, residual, epi, done, ST_WORDS, nb, K, y_ld, res_ld, dt, s);
        return gemv_batched_dev(W, x, y, N, K, norm_w, norm_w ? g.rms_eps : 0.f, nullptr, residual, epi, done, ST_WORDS, nb, K, y_ld, res_ld, dt, s);
    };
    // the quantised planes of one projection of layer l, either kind: `pick` names the projection's two members
    auto qplanes = [&](int l, auto pick) { return wq == GEMV_WQ_MXFP4 ? pick(h->mx4[l]) : wq ? pick(h->w8[l]) : QPlanes{nullptr, nullptr}; };
    const auto q_qkv = [](const auto& q) { return QPlanes{q.wqkv, q.s_qkv}; };
    const auto q_o = [](const auto& q) { return QPlanes{q.wo, q.s_o}; };
    const auto q_gu = [](const auto& q) { return QPlanes{q.wgu, q.s_gu}; };
    const auto q_down = [](const auto& q) { return QPlanes{q.wdown, q.s_down}; };
    const QPlanes q_lm = wq == GEMV_WQ_MXFP4 ? QPlanes{h->mx4_lm_head, h->mx4_lm_scale} : QPlanes{h->w8_lm_head, h->w8_lm_scale};
#define MARK(c) do { if (prof) prof->mark(c); } while (0)
    MARK(-1);
    // a slot records log-probabilities: the raw row is read before anything edits it (off everywhere, the default: no launch)
    const bool lp = h->logprobs_in(seq0, nslots);
    if (lp && (rc = SS_DISPATCH(dt, logprob_raw_launch, h, seq0, nslots, s))) return rc;
    // history rules on for a slot: its row is edited before the opening kernel reads it (off everywhere, the default: no launch)
    if (h->rules_in(seq0, nslots) && (rc = SS_DISPATCH(dt, logits_rules_launch, h, seq0, nslots, 0, s))) return rc;
    // a speculative step: its opening kernel (the refusals of ss_llama_generate keep the option kernels above out of it)
    if (spec) rc = SS_DISPATCH(dt, spec_open_launch, h, seq0, s);
    // a beam search runs on these slots (seq0 = 0): its three kernels open the token
    else if (h->beam.hdr) rc = SS_DISPATCH(dt, beam_open_launch, h, nslots, h->rules_in(seq0, nslots), s);
    // greedy slots only (the default): the launch it has always been
    else if (h->sampling_in(seq0, nslots)) rc = SS_DISPATCH(dt, sample_embed_draw_launch, h, seq0, nslots, lp, s);
    else rc = SS_DISPATCH(dt, sample_embed_launch, h, seq0, nslots, s);
    if (rc) return rc;
    if (lp && (rc = SS_DISPATCH(dt, logprob_tok_launch, h, seq0, nslots, s))) return rc;
    MARK(3);
    for (int l = 0; l < g.n_layers; ++l) {
        const ss_llama_layer_weights& L = h->layers[l];
        char* kc = slot_k(h, seq0, l);
        char* vc = slot_v(h, seq0, l);
        MARK(-1);
        rc = proj(L.wqkv, qplanes(l, q_qkv), ax, aqkv, 3 * H, H, L.ln1, nullptr, SS_EPI_NONE, 3 * H, 0);
        if (rc) return rc;
        MARK(0);
        // RoPE(q,k) + KV append + split-KV attention in one kernel (+ the split merge); with the fp8 shadow on, its sibling
        // that reads the shadow and appends to both
        if (spec) {
            rc = attn_decode_spec_dev(aqkv, kc, vc, h->w.rope_cos, h->w.rope_sin, aattn, h->spec.attn_ws, h->spec.row_st + ST_KV_LEN,
                                      h->spec.row_st + ST_POS, &h->spec.hdr->n_active, nb, g.n_heads, hd, g.cache_cap, dt, s);
        } else if (h->kq) {
            const size_t so = ((size_t)seq0 * g.n_layers + l) * g.n_heads * g.cache_cap;        // rows in front of this plane
            rc = attn_decode_kv8_fused_dev(h->qkv, kc, vc, h->kq + so * hd, h->vq + so * hd, h->kscale + so, h->vscale + so,
                                           h->w.rope_cos, h->w.rope_sin, h->attn, attn_ws, st + ST_KV_LEN, st + ST_POS, done,
                                           g.n_heads, hd, g.cache_cap, nb, ST_WORDS, cache_stride, dt, s);
        } else {
            rc = attn_decode_fused_dev(h->qkv, kc, vc, h->w.rope_cos, h->w.rope_sin, h->attn, attn_ws, st + ST_KV_LEN,
                                       st + ST_POS, done, g.n_heads, hd, g.cache_cap, nb, ST_WORDS, cache_stride, dt, s);
        }
        if (rc) return rc;
        if (h->cap.maps && nslots == 1 && !spec) {   // attention-map capture: this layer's row of head cap.head (capture off: no launch)
            rc = attn_scores_decode_dev(h->qkv, kc, h->w.rope_cos, h->w.rope_sin, st + ST_KV_LEN, st + ST_POS, done, h->cap_desc,
                                        l, g.n_heads, hd, g.cache_cap, dt, s);
            if (rc) return rc;
        }
        MARK(1);
        rc = proj(L.wo, qplanes(l, q_o), aattn, axn, H, H, nullptr, ax, SS_EPI_RESIDUAL, H, H);
        if (rc) return rc;
        MARK(0);
        rc = proj(L.wgu, qplanes(l, q_gu), axn, ahm, I, H, L.ln2, nullptr, SS_EPI_SILU_MUL, I, 0);
        if (rc) return rc;
        MARK(0);
        rc = proj(L.wdown, qplanes(l, q_down), ahm, ax, H, I, nullptr, axn, SS_EPI_RESIDUAL, H, H);
        if (rc) return rc;
        MARK(2);
    }
    if (spec) rc = SS_DISPATCH(dt, spec_final_norm_launch, h, seq0, s);
    else rc = SS_DISPATCH(dt, final_norm_advance_launch, h, seq0, nslots, s);
    if (rc) return rc;
    MARK(3);
    rc = proj(h->w.lm_head, q_lm, axn, logits, g.vocab, H, nullptr, nullptr, SS_EPI_NONE, g.vocab, 0);
    if (rc) return rc;
    MARK(0);
#undef MARK
    return SS_OK;
}

// device state -> pinned read-back area (synchronises), then the host mirrors of slots [seq0, seq0+nb)
static int sync_lengths(ss_llama* h, int seq0, int nb, hipStream_t s) {
    SS_HIP(hipMemcpyAsync(h->pinned, h->state, (size_t)h->n_seq * ST_WORDS * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    SS_HIP(hipStreamSynchronize(s));
    for (int b = seq0; b < seq0 + nb; ++b) {
        h->kv_len[b] = h->pinned[b * ST_WORDS + ST_KV_LEN];
        h->pos[b] = h->pinned[b * ST_WORDS + ST_POS];
    }
    return SS_OK;
}

// captured decode token for slots [seq0, seq0+nb), built on first use
static int graph_for(ss_llama* h, int seq0, int nb, hipGraphExec_t* out) {
    const int mode = knob(K_gemm_f32_split);
    const int capture = (h->cap.maps && nb == 1) ? 1 : 0;
    const int w8 = h->decode_weights_kind();
    const int sampling = h->sampling_in(seq0, nb) ? 1 : 0;
    const int rules = h->rules_in(seq0, nb) ? 1 : 0;
    const int kv8 = h->kq ? 1 : 0;
    const int logprobs = h->logprobs_in(seq0, nb) ? 1 : 0;
    const int beam = h->beam.hdr ? h->beam_rows * 16 + nb : 0;
    void* const beam_ws = h->beam.hdr;
    const int spec = (h->spec_run && h->spec.hdr && nb == 1) ? h->spec_rows : 0;
    void* const spec_ws = spec ? (void*)h->spec.hdr : nullptr;
    for (const SeqGraph& sg : h->graphs)
        if (sg.seq0 == seq0 && sg.nb == nb && sg.mode == mode && sg.capture == capture && sg.w8 == w8 && sg.sampling == sampling &&
            sg.rules == rules && sg.kv8 == kv8 && sg.logprobs == logprobs && sg.beam == beam && sg.beam_ws == beam_ws && sg.spec == spec && sg.spec_ws == spec_ws) {
            *out = sg.exec;
            return SS_OK;
        }
    SeqGraph sg;
    sg.seq0 = seq0; sg.nb = nb; sg.mode = mode; sg.capture = capture; sg.w8 = w8; sg.sampling = sampling; sg.rules = rules; sg.kv8 = kv8;
    sg.logprobs = logprobs; sg.beam = beam; sg.beam_ws = beam_ws; sg.spec = spec; sg.spec_ws = spec_ws;
    sg.graph = nullptr; sg.exec = nullptr;
    SS_HIP(hipStreamBeginCapture(h->cap_stream, hipStreamCaptureModeThreadLocal));
    int rc = decode_token(h, h->cap_stream, nullptr, seq0, nb);
    hipError_t ce = hipStreamEndCapture(h->cap_stream, &sg.graph);
    if (rc) return rc;
    SS_HIP(ce);
    SS_HIP(hipGraphInstantiate(&sg.exec, sg.graph, nullptr, nullptr, 0));
    h->graphs.push_back(sg);
    *out = sg.exec;
    return SS_OK;
}

// after the last token of a call (h->pinned holds the final state words): the token that ended it joins the history of every
// rules-on slot, and the host mirror of the history lengths follows the device
static int rules_finish(ss_llama* h, int seq0, int nb, hipStream_t s) {
    if (!h->rules_in(seq0, nb)) return SS_OK;
    if (int rc = SS_DISPATCH(h->cfg.dtype, logits_rules_launch, h, seq0, nb, 1, s)) return rc;
    for (int b = seq0; b < seq0 + nb; ++b)
        if (h->rules_on[b]) {
            const int64_t len = h->hist_len[b] + h->pinned[b * ST_WORDS + ST_NGEN];
            h->hist_len[b] = len < h->hist_cap() ? len : h->hist_cap();
        }
    return SS_OK;
}

// fp8 KV shadow, lazy sync: ONE eager launch in front of a decode loop quantises the 16-bit rows [kv8_rows, kv_len) of slots
// [seq0, seq0+nb) — whatever wrote them (prefill, the image-token block, a loaded or gathered cache).  Inside the loop only the
// fused decode kernel's own append writes the shadow.
static int kv8_sync(ss_llama* h, int seq0, int nb, hipStream_t s) {
    if (!h->kq) return SS_OK;
    const ss_llama_config& g = h->cfg;
    const size_t so = (size_t)seq0 * g.n_layers * g.n_heads * g.cache_cap;       // rows in front of slot seq0
    Kv8QuantArgs a = {h->kc + so * h->hd * h->esz, h->vc + so * h->hd * h->esz, h->kq + so * h->hd, h->vq + so * h->hd,
                      h->kscale + so, h->vscale + so, g.n_heads, g.cache_cap, h->hd, g.n_layers, nb,
                      (int64_t)(h->seq_kv_bytes() / h->esz), {0, 0, 0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0, 0, 0}};
    bool any = false;
    for (int b = 0; b < nb; ++b) {
        const int64_t len = h->kv_len[seq0 + b], have = h->kv8_rows[seq0 + b];
        a.lo[b] = (int)(have < len ? have : len);
        a.hi[b] = (int)len;
        any = any || a.lo[b] < a.hi[b];
    }
    if (any)
        if (int rc = kv8_quantize_dev(a, g.dtype, s)) return rc;
    for (int b = seq0; b < seq0 + nb; ++b) h->kv8_rows[b] = h->kv_len[b];
    return SS_OK;
}
// after a decode loop (the host mirrors hold the final lengths): every row it appended has its shadow row
static void kv8_advance(ss_llama* h, int seq0, int nb) {
    if (h->kq)
        for (int b = seq0; b < seq0 + nb; ++b) h->kv8_rows[b] = h->kv_len[b];
}

// shared driver of ss_llama_generate / ss_llama_generate_batch: the state words of slots
// [seq0, seq0+nb) have been staged in h->pinned[upload area]; replays the decode graph until every
// slot reports done or `eff_limit` tokens were launched.
static int run_decode(ss_llama* h, int seq0, int nb, int64_t eff_limit, hipStream_t s) {
    if (int rc = kv8_sync(h, seq0, nb, s)) return rc;
    SS_HIP(hipMemcpyAsync(h->state + (size_t)seq0 * ST_WORDS, h->upload() + (size_t)seq0 * ST_WORDS,
                          (size_t)nb * ST_WORDS * sizeof(int32_t), hipMemcpyHostToDevice, s));
    const bool use_graph = knob(K_llama_graph) != 0;
    hipGraphExec_t exec = nullptr;
    if (use_graph) { int rc = graph_for(h, seq0, nb, &exec); if (rc) return rc; }
    const int chunk = knob(K_llama_done_poll);
    int64_t launched = 0;
    while (launched < eff_limit) {
        const int64_t n = (eff_limit - launched) < chunk ? (eff_limit - launched) : chunk;
        for (int64_t i = 0; i < n; ++i) {
            if (use_graph) SS_HIP(hipGraphLaunch(exec, s));
            else { int rc = decode_token(h, s, nullptr, seq0, nb); if (rc) return rc; }
        }
        launched += n;
        int rc = sync_lengths(h, seq0, nb, s);
        if (rc) return rc;
        bool all = true;
        for (int b = seq0; b < seq0 + nb; ++b) all = all && h->pinned[b * ST_WORDS + ST_DONE];
        if (all) break;
    }
    if (!launched) { int rc = sync_lengths(h, seq0, nb, s); if (rc) return rc; }
    kv8_advance(h, seq0, nb);
    return rules_finish(h, seq0, nb, s);
}

// a rules-on slot appends every token of the call to its history: refused when the buffer could not hold them
static int history_fits(const ss_llama* h, int b, int64_t limit, const char* who) {
    SS_REQUIRE(!h->rules_on[b] || h->hist_len[b] + limit <= h->hist_cap(),
               "%s: the token history of slot %d would outgrow its buffer (%lld + %lld > cache_cap + max_new = %lld)", who, b,
               (long long)h->hist_len[b], (long long)limit, (long long)h->hist_cap());
    return SS_OK;
}

// kv_len / pos of one slot: the device state words and the host mirrors (the callers have checked the range)
static int set_lengths_slot(ss_llama* h, int slot, int64_t kv_len, int64_t pos, hipStream_t s) {
    hipLaunchKernelGGL(set_state_kernel, dim3(1), dim3(64), 0, s, h->state + (size_t)slot * ST_WORDS, (int)ST_KV_LEN,
                       (int)kv_len, (int)ST_POS, (int)pos);
    SS_LAUNCH_CHECK("set_state");
    h->kv_len[slot] = kv_len;
    h->pos[slot] = pos;
    if (h->kv8_rows[slot] > kv_len) h->kv8_rows[slot] = kv_len;       // a truncated cache: the rows beyond will be rewritten
    return SS_OK;
}

// one cache plane: rows keep[0 .. n_keep) packed to the front, through the qkv activation buffer as scratch
template <typename T>
static int kv_repack_launch(ss_llama* h, char* plane, const int32_t* keep, int n_keep, hipStream_t s) {
    const int cap = h->cfg.cache_cap, hd = h->hd;
    const int blocks = cdiv((int64_t)n_keep * (hd / Tr<T>::kVec), 256);
    const dim3 grid((unsigned)(blocks > 0 ? blocks : 1), (unsigned)h->cfg.n_heads);
    hipLaunchKernelGGL(kv_gather_kernel<T>, grid, dim3(256), 0, s, (const T*)plane, (T*)h->qkv, keep, n_keep, cap, hd, n_keep);
    hipLaunchKernelGGL(kv_gather_kernel<T>, grid, dim3(256), 0, s, (const T*)h->qkv, (T*)plane, (const int32_t*)nullptr, n_keep,
                       n_keep, hd, cap);
    SS_LAUNCH_CHECK("kv_gather");
    return SS_OK;
}

// capture on: the rows [kv0, kv0 + n) x columns [0, kv0 + n) must lie inside the caller's buffer
static int capture_fits(const ss_llama* h, int64_t kv0, int64_t n, const char* who) {
    if (!h->cap.maps) return SS_OK;
    SS_REQUIRE(kv0 >= h->cap.row0, "%s: attention capture starts at cache index %d, the cache holds only %lld", who,
               (int)h->cap.row0, (long long)kv0);
    SS_REQUIRE(kv0 + n - h->cap.row0 <= h->cap.n_rows, "%s: attention-capture buffer has %d rows, %lld needed", who,
               (int)h->cap.n_rows, (long long)(kv0 + n - h->cap.row0));
    SS_REQUIRE(kv0 + n <= h->cap.ld, "%s: attention-capture buffer has %d columns, %lld needed", who, (int)h->cap.ld,
               (long long)(kv0 + n));
    return SS_OK;
}

// The stride list of "stacked rows [rows, hidden] of one slot against that slot's cache planes [n_heads][cache_cap][hd],
// bottom-right causal", and its sibling for every slot of the engine at once (slot b: rows [b*rows, (b+1)*rows) against
// kv_lens[b] keys of its own planes of layer `layer`).
static int cache_attention(const ss_llama* h, const void* q, const void* kc, const void* vc, void* out, int64_t rows,
                           int64_t kv_len, void* stream) {
    const int64_t H = h->cfg.hidden, hd = h->hd, head = (int64_t)h->cfg.cache_cap * hd;
    return ss_attention(q, kc, vc, out, 1, h->cfg.n_heads, rows, kv_len, hd, 0, hd, H, 0, head, hd, 0, head, hd, 0, hd, H,
                        1.0f / sqrtf((float)hd), 1, h->cfg.dtype, stream);
}
static int cache_attention_all_slots(const ss_llama* h, int layer, int64_t rows, const int32_t* kv_lens, void* stream) {
    const int64_t H = h->cfg.hidden, hd = h->hd, head = (int64_t)h->cfg.cache_cap * hd;
    const int64_t slot = (int64_t)(h->seq_kv_bytes() / h->esz);
    return ss_attention_ragged(h->q, slot_k(h, 0, layer), slot_v(h, 0, layer), h->attn, h->n_seq, h->cfg.n_heads, rows, kv_lens,
                               hd, rows * H, hd, H, slot, head, hd, slot, head, hd, rows * H, hd, H, 1.0f / sqrtf((float)hd), 1,
                               h->cfg.dtype, stream);
}

// The prefill / continuation forward: segment i feeds segs[i].rows new rows of `embeds` (stacked in segment order) to
// sequence slot segs[i].slot.  Every projection runs ONCE on the stack (M = sum of the rows: the 13.2 GB of layer weights
// are streamed once per call, not once per slot); RoPE / KV append and the bottom-right causal attention stay per slot
// (each slot's rows against its own cache).  One segment = the single-slot ss_llama_prefill; several = the image-token
// block continuation of lock-step stories (4 x 66 rows) and their prompt prefill (4 x S rows).  The callers have checked
// every segment's KV and position bounds, so nothing fails after the first launch for a reason known beforehand.
struct PrefillSeg {
    int slot;
    int64_t rows;               // > 0
    const int32_t* pos_ids;     // explicit RoPE positions (device), or null: pos, pos + 1, ...; the slot's pos then stays
};

static int prefill_forward(ss_llama* h, const PrefillSeg* segs, int nseg, const void* embeds, void* hidden_out,
                           const char* who, void* stream) {
    const ss_llama_config& g = h->cfg;
    hipStream_t s = (hipStream_t)stream;
    const int dt = g.dtype;
    const int64_t H = g.hidden, I = g.inter;
    const int hd = h->hd;
    const size_t e = h->esz;
    int rc;
    int64_t M = 0;
    // every slot of the engine feeds the same number of rows (the lock-step image-token block, equal-length prompts): ONE
    // attention launch over the slots, slot b attending to its own kv_len[b] + r keys (measured at 8 x 66 rows: 256 launches
    // of 24 us per pass = a third of the block's time, before)
    bool ragged = nseg == h->n_seq && nseg >= 2 && nseg <= 8 && knob(K_llama_batched_attn) != 0;
    int32_t kv_lens[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < nseg; ++i) {
        const PrefillSeg& sg = segs[i];
        if ((rc = capture_fits(h, h->kv_len[sg.slot], sg.rows, who))) return rc;
        if (sg.rows != segs[0].rows) ragged = false;
        if (ragged) kv_lens[i] = (int32_t)(h->kv_len[sg.slot] + sg.rows);       // nseg == n_seq: segment i is slot i
        M += sg.rows;
    }
    SS_HIP(hipMemcpyAsync(h->x, embeds, (size_t)M * H * e, hipMemcpyDeviceToDevice, s));
    for (int l = 0; l < g.n_layers; ++l) {
        const ss_llama_layer_weights& L = h->layers[l];
        if ((rc = rmsnorm_rows(h->x, L.ln1, h->xn, M, H, g.rms_eps, dt, s))) return rc;
        if ((rc = prefill_proj(h->splitk_ws, h->splitk_bytes, h->xn, L.wqkv, h->qkv, M, 3 * H, H, nullptr, dt, s))) return rc;
        int64_t r0 = 0;
        for (int i = 0; i < nseg; ++i) {
            const PrefillSeg& sg = segs[i];
            char *kc = slot_k(h, sg.slot, l), *vc = slot_v(h, sg.slot, l);
            const int64_t r = sg.rows, kv0 = h->kv_len[sg.slot], kv1 = kv0 + r;
            char* q_b = h->q + (size_t)r0 * H * e;
            if ((rc = ss_rope_kv_append(h->qkv + (size_t)r0 * 3 * H * e, q_b, kc, vc, h->w.rope_cos, h->w.rope_sin, sg.pos_ids,
                                        h->pos[sg.slot], r, g.n_heads, hd, kv0, g.cache_cap, dt, stream)))
                return rc;
            if (h->cap.maps) {      // head cap.head's pre-softmax scores of these rows against the cache (prefix included)
                char* rows = (char*)h->cap.maps + (((size_t)l * h->cap.n_rows + (size_t)(kv0 - h->cap.row0)) * h->cap.ld) * e;
                if ((rc = attn_scores_dev(q_b + (size_t)h->cap.head * hd * e, H, kc + (size_t)h->cap.head * g.cache_cap * hd * e, hd,
                                          rows, h->cap.ld, r, kv1, hd, r > 1 ? h->cap_row_calls : 0, dt, s)))
                    return rc;
            }
            if (!ragged && (rc = cache_attention(h, q_b, kc, vc, h->attn + (size_t)r0 * H * e, r, kv1, stream))) return rc;
            r0 += r;
        }
        if (ragged && (rc = cache_attention_all_slots(h, l, segs[0].rows, kv_lens, stream))) return rc;
        if ((rc = prefill_proj(h->splitk_ws, h->splitk_bytes, h->attn, L.wo, h->x, M, H, H, h->x, dt, s))) return rc;
        if ((rc = rmsnorm_rows(h->x, L.ln2, h->xn, M, H, g.rms_eps, dt, s))) return rc;
        if ((rc = prefill_proj(h->splitk_ws, h->splitk_bytes, h->xn, L.wgu, h->gu, M, 2 * I, H, nullptr, dt, s))) return rc;
        if ((rc = ss_silu_mul(h->gu, h->hm, M, I, dt, stream))) return rc;
        if ((rc = prefill_proj(h->splitk_ws, h->splitk_bytes, h->hm, L.wdown, h->x, M, H, I, h->x, dt, s))) return rc;
    }
    // final norm (:652) for all rows, lm_head for each segment's last row only (greedy consumes logits[:, -1])
    void* hid = hidden_out ? hidden_out : (void*)h->xn;
    if ((rc = rmsnorm_rows(h->x, h->w.final_norm, hid, M, H, g.rms_eps, dt, s))) return rc;
    int64_t r0 = 0;
    for (int i = 0; i < nseg; ++i) {
        const PrefillSeg& sg = segs[i];
        const char* last = (const char*)hid + (size_t)(r0 + sg.rows - 1) * H * e;
        if ((rc = gemv_dev(h->w.lm_head, last, h->logits + (size_t)sg.slot * g.vocab * e, g.vocab, H, nullptr, 0.f, nullptr,
                           nullptr, SS_EPI_NONE, nullptr, dt, s)))
            return rc;
        const int64_t pos = h->pos[sg.slot] + (sg.pos_ids ? 0 : sg.rows);        // explicit pos_ids: the caller sets pos afterwards
        if ((rc = set_lengths_slot(h, sg.slot, h->kv_len[sg.slot] + sg.rows, pos, s))) return rc;
        r0 += sg.rows;
    }
    return SS_OK;
}

// one plane kind of a fork: `span` packets of every (layer, head) unit of both slabs, source to every destination
template <typename P>
static int fork_planes_launch(const ss_llama* h, void* plane0, void* plane1, int64_t unit_stride, int64_t span, int src,
                              const ForkDst& d, hipStream_t s) {
    if (span <= 0) return SS_OK;
    const int64_t units = (int64_t)h->cfg.n_layers * h->cfg.n_heads;
    const dim3 grid((unsigned)cdiv(span, 256 * kForkPackets), (unsigned)units, 2);
    hipLaunchKernelGGL(fork_planes_kernel<P>, grid, dim3(256), 0, s, (P*)plane0, (P*)plane1, units * unit_stride, unit_stride, span,
                       src, d);
    SS_LAUNCH_CHECK("fork_planes");
    return SS_OK;
}

template <typename T>
static int fork_state_launch(ss_llama* h, int src, const ForkDst& d, hipStream_t s) {
    const ss_llama_config& g = h->cfg;
    hipLaunchKernelGGL(fork_state_kernel<T>, dim3(16), dim3(256), 0, s, (T*)h->logits, g.vocab, h->state, h->rules, h->hist,
                       h->hist_cap(), h->hist_bm, h->bm_words(), src, d);
    SS_LAUNCH_CHECK("fork_state");
    return SS_OK;
}

extern "C" {

size_t ss_llama_workspace_bytes(const ss_llama_config* cfg, int64_t max_prefill_rows) {
    if (!cfg) return 0;
    ss_llama tmp;
    tmp.cfg = *cfg;
    tmp.hd = cfg->hidden / cfg->n_heads;
    tmp.n_seq = cfg_n_seq(cfg);
    tmp.max_rows = max_prefill_rows < tmp.n_seq ? tmp.n_seq : max_prefill_rows;
    tmp.esz = dtype_size(cfg->dtype);
    Carver c{nullptr, 0, 0};
    carve(&tmp, c);
    return c.off + 256;
}

int ss_llama_create(const ss_llama_config* cfg, const ss_llama_weights* w, void* workspace, size_t workspace_bytes,
                    int64_t max_prefill_rows, const int32_t* host_img_ids, ss_llama** out) {
    SS_REQUIRE(cfg && w && workspace && out, "llama_create: null argument");
    SS_REQUIRE(cfg->hidden % cfg->n_heads == 0, "llama_create: hidden %% n_heads != 0");
    SS_REQUIRE(cfg->n_img_ids <= 1024 && cfg->max_new > 0 && cfg->cache_cap > 0, "llama_create: bad config");
    SS_REQUIRE(cfg->n_seq >= 0 && cfg->n_seq <= 8, "llama_create: n_seq=%d unsupported (1..8)", cfg->n_seq);
    // the decode loop's per-slot stop word packs the EOS id in 16 bits (and the optional second stop id + 1 above it)
    SS_REQUIRE(cfg->vocab > 0 && cfg->vocab <= 0xFFFF && cfg->eos_id < 0xFFFF,
               "llama_create: vocab %d / eos_id %d do not fit the 16-bit stop word (vocab <= 65535)", (int)cfg->vocab,
               (int)cfg->eos_id);
    int32_t info[4];
    int rc = ss_device_info(info);
    if (rc) return rc;
    if (!info[1]) { set_error("llama_create: device is not gfx950"); return SS_EHIP; }
    ss_llama* h = new ss_llama();
    h->cfg = *cfg;
    h->w = *w;
    h->layers.assign(w->layers, w->layers + cfg->n_layers);
    h->w.layers = h->layers.data();
    h->hd = cfg->hidden / cfg->n_heads;
    h->n_seq = cfg_n_seq(cfg);
    h->cur = 0;
    h->max_rows = max_prefill_rows < h->n_seq ? h->n_seq : max_prefill_rows;
    h->esz = dtype_size(cfg->dtype);
    const size_t base = (size_t)workspace;
    const size_t skew = align_up(base) - base;
    Carver c{(char*)workspace + skew, 0, workspace_bytes - skew};
    carve(h, c);
    if (c.off > c.cap) {
        set_error("llama_create: workspace too small (%zu < %zu)", workspace_bytes, c.off + skew);
        delete h;
        return SS_ENOMEM;
    }
    h->kv_len.assign(h->n_seq, 0);
    h->pos.assign(h->n_seq, 0);
    h->samp_on.assign(h->n_seq, 0);
    h->rules_on.assign(h->n_seq, 0);
    h->lp_on.assign(h->n_seq, 0);
    h->hist_len.assign(h->n_seq, 0);
    h->kv8_rows.assign(h->n_seq, 0);
    hipError_t e = hipStreamCreateWithFlags(&h->cap_stream, hipStreamNonBlocking);
    if (e == hipSuccess)
        e = hipHostMalloc((void**)&h->pinned, (size_t)h->n_seq * 2 * ST_WORDS * sizeof(int32_t) + 64, hipHostMallocDefault);
    // the whole workspace starts as zeros: a cache row a caller declares valid without having written it (set_lengths on a
    // fresh slot: profiling runs, KV mirrors) then holds zeros, not the allocator's residue — NaN bit patterns there turn
    // every logit into NaN
    if (e == hipSuccess) e = hipMemset(c.base, 0, c.off);
    if (e == hipSuccess && cfg->n_img_ids > 0)
        e = hipMemcpy(h->img_ids, host_img_ids, cfg->n_img_ids * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) { rc = check_hip(e, "llama_create"); delete h; return rc; }
    *out = h;
    return SS_OK;
}

void ss_llama_destroy(ss_llama* h) {
    if (!h) return;
    for (SeqGraph& sg : h->graphs) {
        if (sg.exec) hipGraphExecDestroy(sg.exec);
        if (sg.graph) hipGraphDestroy(sg.graph);
    }
    if (h->cap_stream) hipStreamDestroy(h->cap_stream);
    if (h->pinned) hipHostFree(h->pinned);
    delete h;
}

int ss_llama_set_stop_id(ss_llama* h, int32_t token_id) {
    SS_REQUIRE(h && token_id >= -1 && token_id < 0x7FFE && token_id < h->cfg.vocab,
               "llama_set_stop_id: token id %d out of range (< min(vocab, 32766))", (int)token_id);
    h->stop2 = token_id;
    return SS_OK;
}

int ss_llama_set_attn_capture(ss_llama* h, void* maps, int64_t n_rows, int64_t ld, int64_t row0, int32_t head,
                              int32_t row_calls) {
    SS_REQUIRE(h, "llama_set_attn_capture: null handle");
    AttnCaptureDesc d = {nullptr, 0, 0, 0, 0};
    if (maps) {
        SS_REQUIRE(n_rows > 0 && ld > 0 && n_rows < (1ll << 30) && ld < (1ll << 30) && row0 >= 0 && row0 <= h->cfg.cache_cap,
                   "llama_set_attn_capture: bad buffer (n_rows=%lld ld=%lld row0=%lld)", (long long)n_rows, (long long)ld,
                   (long long)row0);
        SS_REQUIRE(head >= 0 && head < h->cfg.n_heads, "llama_set_attn_capture: head %d out of range (%d heads)", (int)head,
                   h->cfg.n_heads);
        SS_REQUIRE(row_calls == 0 || row_calls == 1, "llama_set_attn_capture: row_calls must be 0 or 1");
        SS_REQUIRE(h->hd == 128 || h->hd == 64, "llama_set_attn_capture: head dim %d unsupported (64, 128)", h->hd);
        d.maps = maps; d.n_rows = (int32_t)n_rows; d.ld = (int32_t)ld; d.row0 = (int32_t)row0; d.head = head;
    }
    // every decode loop of this engine has synchronised before it returned: nothing in flight reads the descriptor
    SS_HIP(hipMemcpy(h->cap_desc, &d, sizeof(d), hipMemcpyHostToDevice));
    h->cap = d;
    h->cap_row_calls = maps ? row_calls : 0;
    return SS_OK;
}

int ss_llama_set_sampling(ss_llama* h, int32_t seq, const ss_sampling* p) {
    SS_REQUIRE(h, "llama_set_sampling: null handle");
    SS_REQUIRE(seq >= -1 && seq < h->n_seq, "llama_set_sampling: sequence slot %d out of range (-1 = all, < %d)", (int)seq, h->n_seq);
    SampleParams sp = {1.0f, 1.0f, 0, 0u, 0u, 0u, 0, 0};       // greedy
    if (p)
        if (int rc = sampling_params(p, "llama_set_sampling", &sp)) return rc;
    // every decode loop of this engine has synchronised before it returned: nothing in flight reads the block
    const int b0 = seq < 0 ? 0 : seq, b1 = seq < 0 ? h->n_seq : seq + 1;
    for (int b = b0; b < b1; ++b) {
        SS_HIP(hipMemcpy(h->samp + b, &sp, sizeof(sp), hipMemcpyHostToDevice));
        h->samp_on[b] = p ? 1 : 0;
    }
    return SS_OK;
}

int ss_llama_set_logits_rules(ss_llama* h, int32_t seq, const ss_logits_rules* p) {
    SS_REQUIRE(h, "llama_set_logits_rules: null handle");
    SS_REQUIRE(seq >= -1 && seq < h->n_seq, "llama_set_logits_rules: sequence slot %d out of range (-1 = all, < %d)", (int)seq, h->n_seq);
    RulesState rp = {1.0f, 0, 0, 0, 0, 0, 0, 0};        // off
    if (p)
        if (int rc = logits_rules_params(p, "llama_set_logits_rules", &rp)) return rc;
    // every decode loop of this engine has synchronised before it returned: nothing in flight reads the block.  Only the rule
    // words are written: the history bookkeeping behind them is ss_llama_set_history's and the kernel's
    const int b0 = seq < 0 ? 0 : seq, b1 = seq < 0 ? h->n_seq : seq + 1;
    for (int b = b0; b < b1; ++b) {
        SS_HIP(hipMemcpy(h->rules + b, &rp, offsetof(RulesState, hist_len), hipMemcpyHostToDevice));
        h->rules_on[b] = p ? 1 : 0;
    }
    return SS_OK;
}

int ss_llama_set_logprobs(ss_llama* h, int32_t seq, float* model_lp, float* policy_lp, int32_t* top_ids, float* top_lp,
                          int32_t top_n) {
    SS_REQUIRE(top_n >= 0 && top_n <= SS_LOGPROB_MAX_TOP, "llama_set_logprobs: top_n %d outside [0, %d]", (int)top_n, SS_LOGPROB_MAX_TOP);
    const bool off = !model_lp && !policy_lp && !top_ids && !top_lp;
    if (!off) {
        SS_REQUIRE(model_lp && policy_lp, "llama_set_logprobs: NULL log-probability buffer (both, or every buffer NULL to switch the option off)");
        SS_REQUIRE(top_n > 0 ? (top_ids && top_lp) : (!top_ids && !top_lp),
                   "llama_set_logprobs: top_n %d %s", (int)top_n, top_n > 0 ? "needs both top-n buffers" : "takes no top-n buffers");
    }
    SS_REQUIRE(h, "llama_set_logprobs: null handle");
    SS_REQUIRE(seq >= -1 && seq < h->n_seq, "llama_set_logprobs: sequence slot %d out of range (-1 = all, < %d)", (int)seq, h->n_seq);
    // every decode loop of this engine has synchronised before it returned: nothing in flight reads the block
    const int b0 = seq < 0 ? 0 : seq, b1 = seq < 0 ? h->n_seq : seq + 1;
    const size_t n = (size_t)h->cfg.max_new;
    for (int b = b0; b < b1; ++b) {
        const size_t i = (size_t)(b - b0);      // seq = -1: the buffers hold [n_seq] slots, slot-major
        LogprobDesc d = {nullptr, nullptr, nullptr, nullptr, 0, 0};
        if (!off) {
            d.model_lp = model_lp + i * n; d.policy_lp = policy_lp + i * n;
            if (top_n > 0) { d.top_ids = top_ids + i * n * top_n; d.top_lp = top_lp + i * n * top_n; }
            d.top_n = top_n; d.on = 1;
        }
        SS_HIP(hipMemcpy(h->lp_desc + b, &d, sizeof(d), hipMemcpyHostToDevice));
        h->lp_on[b] = off ? 0 : 1;
    }
    return SS_OK;
}

int ss_llama_set_history(ss_llama* h, int32_t seq, const int32_t* host_ids, int64_t n, int32_t append) {
    SS_REQUIRE(h, "llama_set_history: null handle");
    SS_REQUIRE(seq >= -1 && seq < h->n_seq, "llama_set_history: sequence slot %d out of range (-1 = the selected slot, < %d)", (int)seq,
               h->n_seq);
    SS_REQUIRE(n >= 0 && (host_ids || n == 0), "llama_set_history: bad arguments (n=%lld)", (long long)n);
    const int b = seq < 0 ? h->cur : seq;
    const int64_t len0 = append ? h->hist_len[b] : 0;
    SS_REQUIRE(len0 + n <= h->hist_cap(), "llama_set_history: %lld + %lld ids exceed the history buffer (cache_cap + max_new = %lld)",
               (long long)len0, (long long)n, (long long)h->hist_cap());
    for (int64_t i = 0; i < n; ++i)
        SS_REQUIRE(host_ids[i] >= 0 && host_ids[i] < h->cfg.vocab, "llama_set_history: id %d at index %lld outside [0, %d)",
                   (int)host_ids[i], (long long)i, h->cfg.vocab);
    // every decode loop of this engine has synchronised before it returned: nothing in flight reads the history
    int32_t* dst = h->hist + (size_t)b * h->hist_cap() + len0;
    if (n) SS_HIP(hipMemcpy(dst, host_ids, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice));
    if (n || !append) {
        hipLaunchKernelGGL(rules_bitmap_kernel, dim3((unsigned)cdiv(h->bm_words(), 256)), dim3(256), 0, (hipStream_t)0,
                           h->hist_bm + (size_t)b * h->bm_words(), h->bm_words(), dst, (int)n, append ? 1 : 0);
        SS_LAUNCH_CHECK("rules_bitmap");
    }
    const int32_t lens[2] = {(int32_t)(len0 + n), (int32_t)(append ? 0 : n)};       // hist_len, prompt_len
    SS_HIP(hipMemcpy(&h->rules[b].hist_len, lens, (append ? 1 : 2) * sizeof(int32_t), hipMemcpyHostToDevice));
    h->hist_len[b] = len0 + n;
    return SS_OK;
}

// the captured fp8 graphs hold the pointers of the planes they were captured over (weights: flag = &SeqGraph::w8, KV shadow:
// &SeqGraph::kv8): dropped when those planes change
static void drop_graphs(ss_llama* h, int SeqGraph::*flag) {      // (every graph whose flag is non-zero)
    size_t keep = 0;
    for (SeqGraph& sg : h->graphs) {
        if (!(sg.*flag)) { h->graphs[keep++] = sg; continue; }
        if (sg.exec) hipGraphExecDestroy(sg.exec);
        if (sg.graph) hipGraphDestroy(sg.graph);
    }
    h->graphs.resize(keep);
}

int ss_llama_set_decode_w8(ss_llama* h, const ss_llama_layer_w8* layers, const void* lm_head_q, const float* lm_head_scale) {
    SS_REQUIRE(h, "llama_set_decode_w8: null handle");
    if (!layers) {      // off: the 16-bit graphs are still cached; the fp8 ones go with their planes (MXFP4 planes, if on, stay)
        if (h->w8.empty()) return SS_OK;
        drop_graphs(h, &SeqGraph::w8);
        h->w8.clear();
        h->w8_lm_head = nullptr;
        h->w8_lm_scale = nullptr;
        return SS_OK;
    }
    const ss_llama_config& g = h->cfg;
    SS_REQUIRE(g.dtype == SS_BF16 || g.dtype == SS_F16, "llama_set_decode_w8: fp8 decode weights need a bf16 / fp16 engine (dtype %d)", g.dtype);
    SS_REQUIRE(lm_head_q && lm_head_scale, "llama_set_decode_w8: NULL lm_head plane or scales");
    const int64_t H = g.hidden, I = g.inter;
    // the five projections, at one sequence and at all slots: every shape the decode loop will launch
    const struct { int64_t N, K; int epi; bool norm; } shapes[5] = {
        {3 * H, H, SS_EPI_NONE, true}, {H, H, SS_EPI_RESIDUAL, false}, {I, H, SS_EPI_SILU_MUL, true}, {H, I, SS_EPI_RESIDUAL, false},
        {g.vocab, H, SS_EPI_NONE, false}};
    for (const auto& sh : shapes) {
        int rc = gemv_wq_check(GEMV_WQ_FP8, sh.N, sh.K, 1, g.dtype, sh.epi, sh.norm);
        if (!rc) rc = gemv_wq_check(GEMV_WQ_FP8, sh.N, sh.K, h->n_seq, g.dtype, sh.epi, sh.norm);
        if (rc) return rc;
    }
    for (int l = 0; l < g.n_layers; ++l) {
        const ss_llama_layer_w8& Q = layers[l];
        SS_REQUIRE(Q.wqkv && Q.wo && Q.wgu && Q.wdown && Q.s_qkv && Q.s_o && Q.s_gu && Q.s_down, "llama_set_decode_w8: NULL pointer in layer %d", l);
        SS_REQUIRE((((size_t)Q.wqkv | (size_t)Q.wo | (size_t)Q.wgu | (size_t)Q.wdown) & 15) == 0,
                   "llama_set_decode_w8: layer %d: the byte planes must be 16-byte aligned", l);
    }
    SS_REQUIRE(((size_t)lm_head_q & 15) == 0, "llama_set_decode_w8: the lm_head plane must be 16-byte aligned");
    drop_graphs(h, &SeqGraph::w8);
    h->mx4.clear();     // the two kinds of planes exclude each other
    h->mx4_lm_head = h->mx4_lm_scale = nullptr;
    h->w8.assign(layers, layers + g.n_layers);
    h->w8_lm_head = lm_head_q;
    h->w8_lm_scale = lm_head_scale;
    return SS_OK;
}

int ss_llama_set_decode_mx4(ss_llama* h, const ss_llama_layer_mx4* layers, const void* lm_head_codes, const void* lm_head_scales) {
    SS_REQUIRE(h, "llama_set_decode_mx4: null handle");
    if (!layers) {      // off (fp8 planes, if those are what is on, stay): the 16-bit graphs are still cached
        if (h->mx4.empty()) return SS_OK;
        drop_graphs(h, &SeqGraph::w8);
        h->mx4.clear();
        h->mx4_lm_head = h->mx4_lm_scale = nullptr;
        return SS_OK;
    }
    const ss_llama_config& g = h->cfg;
    SS_REQUIRE(g.dtype == SS_BF16 || g.dtype == SS_F16, "llama_set_decode_mx4: MXFP4 decode weights need a bf16 / fp16 engine (dtype %d)", g.dtype);
    SS_REQUIRE(lm_head_codes && lm_head_scales, "llama_set_decode_mx4: NULL lm_head codes or scales");
    const int64_t H = g.hidden, I = g.inter;
    // the five projections, at one sequence and at all slots: every shape the decode loop will launch
    const struct { int64_t N, K; int epi; bool norm; } shapes[5] = {
        {3 * H, H, SS_EPI_NONE, true}, {H, H, SS_EPI_RESIDUAL, false}, {I, H, SS_EPI_SILU_MUL, true}, {H, I, SS_EPI_RESIDUAL, false},
        {g.vocab, H, SS_EPI_NONE, false}};
    for (const auto& sh : shapes) {
        int rc = gemv_wq_check(GEMV_WQ_MXFP4, sh.N, sh.K, 1, g.dtype, sh.epi, sh.norm);
        if (!rc) rc = gemv_wq_check(GEMV_WQ_MXFP4, sh.N, sh.K, h->n_seq, g.dtype, sh.epi, sh.norm);
        if (rc) return rc;
    }
    for (int l = 0; l < g.n_layers; ++l) {
        const ss_llama_layer_mx4& Q = layers[l];
        SS_REQUIRE(Q.wqkv && Q.wo && Q.wgu && Q.wdown && Q.s_qkv && Q.s_o && Q.s_gu && Q.s_down, "llama_set_decode_mx4: NULL pointer in layer %d", l);
        SS_REQUIRE((((size_t)Q.wqkv | (size_t)Q.wo | (size_t)Q.wgu | (size_t)Q.wdown) & 15) == 0,
                   "llama_set_decode_mx4: layer %d: the code planes must be 16-byte aligned", l);
    }
    SS_REQUIRE(((size_t)lm_head_codes & 15) == 0, "llama_set_decode_mx4: the lm_head code plane must be 16-byte aligned");
    drop_graphs(h, &SeqGraph::w8);
    h->w8.clear();      // the two kinds of planes exclude each other
    h->w8_lm_head = nullptr;
    h->w8_lm_scale = nullptr;
    h->mx4.assign(layers, layers + g.n_layers);
    h->mx4_lm_head = lm_head_codes;
    h->mx4_lm_scale = lm_head_scales;
    return SS_OK;
}

int ss_llama_kv8_bytes(const ss_llama_config* cfg, size_t* codes_bytes, size_t* scales_bytes) {
    SS_REQUIRE(cfg && codes_bytes && scales_bytes, "llama_kv8_bytes: null argument");
    SS_REQUIRE(cfg->n_heads > 0 && cfg->hidden % cfg->n_heads == 0 && cfg->n_layers > 0 && cfg->cache_cap > 0, "llama_kv8_bytes: bad config");
    if (int rc = kv8_check(cfg->hidden / cfg->n_heads, cfg->dtype, "llama_kv8_bytes")) return rc;
    const size_t rows = (size_t)cfg_n_seq(cfg) * cfg->n_layers * cfg->n_heads * cfg->cache_cap;
    *codes_bytes = rows * (size_t)(cfg->hidden / cfg->n_heads);
    *scales_bytes = rows * sizeof(float);
    return SS_OK;
}

int ss_llama_set_kv8(ss_llama* h, void* k_codes, void* v_codes, float* k_scale, float* v_scale) {
    SS_REQUIRE(h, "llama_set_kv8: null handle");
    const bool off = !k_codes && !v_codes && !k_scale && !v_scale;
    if (!off) {
        if (int rc = kv8_check(h->hd, h->cfg.dtype, "llama_set_kv8")) return rc;
        SS_REQUIRE(k_codes && v_codes && k_scale && v_scale, "llama_set_kv8: NULL plane (all four, or none to switch the option off)");
        SS_REQUIRE((((size_t)k_codes | (size_t)v_codes) & 15) == 0 && (((size_t)k_scale | (size_t)v_scale) & 3) == 0,
                   "llama_set_kv8: the code planes must be 16-byte aligned (scales: 4)");
    }
    // every decode loop of this engine has synchronised before it returned: nothing in flight reads the planes
    drop_graphs(h, &SeqGraph::kv8);
    h->kq = (uint8_t*)k_codes; h->vq = (uint8_t*)v_codes; h->kscale = k_scale; h->vscale = v_scale;
    h->kv8_rows.assign(h->n_seq, 0);        // new planes hold nothing yet
    return SS_OK;
}

int ss_llama_kv8_invalidate(ss_llama* h, int64_t from_row) {
    SS_REQUIRE(h && from_row >= 0, "llama_kv8_invalidate: bad arguments (from_row=%lld)", (long long)from_row);
    if (h->kv8_rows[h->cur] > from_row) h->kv8_rows[h->cur] = from_row;
    return SS_OK;
}

int ss_llama_select(ss_llama* h, int32_t seq) {
    SS_REQUIRE(h && seq >= 0 && seq < h->n_seq, "llama_select: sequence slot %d out of range", (int)seq);
    h->cur = seq;
    return SS_OK;
}

void* ss_llama_buffer(ss_llama* h, int which) {
    if (!h) return nullptr;
    const ss_llama_config& g = h->cfg;
    const size_t q = (size_t)h->cur;
    switch (which) {
        case 0: return h->kc + q * h->seq_kv_bytes();
        case 1: return h->vc + q * h->seq_kv_bytes();
        case 2: return h->gen_ids + q * g.max_new;
        case 3: return h->hid_rows + q * (size_t)g.max_new * g.hidden * h->esz;
        case 4: return h->logits + q * (size_t)g.vocab * h->esz;
        case 5: return h->state + q * ST_WORDS;
        case 6: return h->hist + q * (size_t)h->hist_cap();
        case 7: return h->hist_bm + q * (size_t)h->bm_words();
        default: return nullptr;
    }
}

int ss_llama_set_lengths(ss_llama* h, int64_t kv_len, int64_t pos, void* stream) {
    SS_REQUIRE(h && kv_len >= 0 && kv_len <= h->cfg.cache_cap && pos >= 0 && pos <= h->cfg.max_pos,
               "llama_set_lengths: out of range (kv_len=%lld pos=%lld)", (long long)kv_len, (long long)pos);
    return set_lengths_slot(h, h->cur, kv_len, pos, (hipStream_t)stream);
}

int ss_llama_get_lengths(ss_llama* h, int64_t* kv_len, int64_t* pos) {
    SS_REQUIRE(h, "llama_get_lengths: null handle");
    if (kv_len) *kv_len = h->kv_len[h->cur];
    if (pos) *pos = h->pos[h->cur];
    return SS_OK;
}

int ss_llama_kv_gather(ss_llama* h, const int32_t* keep_idx_dev, int64_t n_keep, void* stream) {
    SS_REQUIRE(h && keep_idx_dev && n_keep >= 0 && n_keep <= h->kv_len[h->cur], "llama_kv_gather: bad arguments");
    const ss_llama_config& g = h->cfg;
    // scratch = qkv activation buffer: [max_rows][3*hidden] elements >= n_heads * n_keep * hd = n_keep * hidden
    SS_REQUIRE(n_keep <= 3 * h->max_rows, "llama_kv_gather: n_keep %lld exceeds scratch (3 x %lld rows)",
               (long long)n_keep, (long long)h->max_rows);
    for (int l = 0; l < g.n_layers && n_keep > 0; ++l)
        for (char* plane : {slot_k(h, h->cur, l), slot_v(h, h->cur, l)})
            if (int rc = SS_DISPATCH(g.dtype, kv_repack_launch, h, plane, keep_idx_dev, (int)n_keep, (hipStream_t)stream))
                return rc;
    h->kv8_rows[h->cur] = 0;     // rows moved: the shadow of this slot is rebuilt by the next decode loop
    return ss_llama_set_lengths(h, n_keep, h->pos[h->cur], stream);
}

int ss_llama_fork(ss_llama* h, int32_t src, const int32_t* host_dst, int32_t n_dst, void* stream) {
    SS_REQUIRE(h && host_dst, "llama_fork: null argument");
    SS_REQUIRE(src >= 0 && src < h->n_seq, "llama_fork: source slot %d out of range (< %d)", (int)src, h->n_seq);
    SS_REQUIRE(n_dst >= 1, "llama_fork: n_dst=%d (at least one destination)", (int)n_dst);
    ForkDst d = {0, {0, 0, 0, 0, 0, 0, 0}};
    for (int j = 0; j < n_dst; ++j) {
        const int32_t b = host_dst[j];
        SS_REQUIRE(b >= 0 && b < h->n_seq, "llama_fork: destination slot %d out of range (< %d)", (int)b, h->n_seq);
        SS_REQUIRE(b != src, "llama_fork: destination slot %d is the source", (int)b);
        for (int i = 0; i < d.n; ++i) SS_REQUIRE(d.slot[i] != b, "llama_fork: destination slot %d listed twice", (int)b);
        d.slot[d.n++] = b;      // (distinct, in range and not src: never more than n_seq - 1 <= kForkMaxDst)
    }
    const ss_llama_config& g = h->cfg;
    const int64_t row_bytes = (int64_t)h->hd * (int64_t)h->esz;
    SS_REQUIRE(row_bytes % 16 == 0, "llama_fork: a cache row of %lld bytes is no multiple of the 16-byte packet", (long long)row_bytes);
    SS_REQUIRE(!h->kq || h->hd % 16 == 0, "llama_fork: head dim %d of the fp8 shadow is no multiple of 16", h->hd);
    hipStream_t s = (hipStream_t)stream;
    const int64_t kv = h->kv_len[src];
    int rc;
    if ((rc = fork_planes_launch<uint4>(h, h->kc, h->vc, g.cache_cap * row_bytes / 16, kv * row_bytes / 16, src, d, s))) return rc;
    int64_t rows8 = 0;
    if (h->kq) {        // the shadow below the source's watermark goes the same way: codes in 16-byte packets, scales one word each
        rows8 = h->kv8_rows[src] < kv ? h->kv8_rows[src] : kv;
        if ((rc = fork_planes_launch<uint4>(h, h->kq, h->vq, (int64_t)g.cache_cap * h->hd / 16, rows8 * h->hd / 16, src, d, s))) return rc;
        if ((rc = fork_planes_launch<uint32_t>(h, h->kscale, h->vscale, g.cache_cap, rows8, src, d, s))) return rc;
    }
    if ((rc = SS_DISPATCH(g.dtype, fork_state_launch, h, (int)src, d, s))) return rc;
    for (int j = 0; j < d.n; ++j) {
        const int b = d.slot[j];
        h->kv_len[b] = kv;
        h->pos[b] = h->pos[src];
        h->hist_len[b] = h->hist_len[src];
        h->kv8_rows[b] = rows8;
    }
    return SS_OK;
}

int ss_llama_prefill(ss_llama* h, const void* embeds, int64_t M, const int32_t* pos_ids, void* hidden_out,
                     void* stream) {
    SS_REQUIRE(h && embeds && M > 0, "llama_prefill: bad arguments");
    SS_REQUIRE(M <= h->max_rows, "llama_prefill: M=%lld exceeds max_prefill_rows=%lld", (long long)M,
               (long long)h->max_rows);
    const int64_t cur_kv = h->kv_len[h->cur], cur_pos = h->pos[h->cur];
    SS_REQUIRE(cur_kv + M <= h->cfg.cache_cap, "llama_prefill: KV cache overflow (%lld + %lld > %d)",
               (long long)cur_kv, (long long)M, h->cfg.cache_cap);
    SS_REQUIRE(pos_ids || cur_pos + M <= h->cfg.max_pos, "llama_prefill: position overflow");
    const PrefillSeg seg = {h->cur, M, pos_ids};
    return prefill_forward(h, &seg, 1, embeds, hidden_out, "llama_prefill", stream);
}

// several sequence slots in one sweep of the weights: host_rows[b] rows of `embeds` (stacked slot-major) for slot b
int ss_llama_prefill_batch(ss_llama* h, const void* embeds, const int64_t* host_rows, void* hidden_out, void* stream) {
    SS_REQUIRE(h && embeds && host_rows, "llama_prefill_batch: bad arguments");
    SS_REQUIRE(!h->cap.maps, "llama_prefill_batch: attention capture is a single-sequence tool (use ss_llama_prefill on the selected slot)");
    const ss_llama_config& g = h->cfg;
    PrefillSeg segs[8];         // n_seq <= 8 (ss_llama_create)
    int nseg = 0;
    int64_t M = 0;
    for (int b = 0; b < h->n_seq; ++b) {
        const int64_t r = host_rows[b];
        SS_REQUIRE(r >= 0, "llama_prefill_batch: negative row count for slot %d", b);
        SS_REQUIRE(h->kv_len[b] + r <= g.cache_cap, "llama_prefill_batch: KV cache overflow in slot %d (%lld + %lld > %d)", b,
                   (long long)h->kv_len[b], (long long)r, g.cache_cap);
        // (checked for EVERY slot before anything is launched: a slot that failed after the forward would leave host and
        // device lengths inconsistent across the slots)
        // (`<=`: the last RoPE position used is pos + r - 1, so a prompt may exactly fill the position table — the same bound as
        // the single-slot ss_llama_prefill; decoding further is refused by the generate entry points)
        SS_REQUIRE(r == 0 || h->pos[b] + r <= g.max_pos, "llama_prefill_batch: position overflow in slot %d (%lld + %lld > %d)", b,
                   (long long)h->pos[b], (long long)r, g.max_pos);
        if (r) segs[nseg++] = {b, r, nullptr};
        M += r;
    }
    SS_REQUIRE(M > 0 && M <= h->max_rows, "llama_prefill_batch: %lld stacked rows (max_prefill_rows=%lld)", (long long)M,
               (long long)h->max_rows);
    return prefill_forward(h, segs, nseg, embeds, hidden_out, "llama_prefill_batch", stream);
}

// one slot's initial decode state words
static void fill_state(int32_t* init, int64_t kv_len, int64_t pos, bool done, int32_t last, int64_t n_forced, int64_t limit,
                       int32_t eos_word) {
    init[ST_KV_LEN] = (int32_t)kv_len; init[ST_POS] = (int32_t)pos; init[ST_NGEN] = 0; init[ST_DONE] = done ? 1 : 0;
    init[ST_LAST] = last; init[ST_NFORCED] = (int32_t)n_forced; init[ST_LIMIT] = (int32_t)limit; init[ST_EOS] = eos_word;
}

// stage one slot's initial decode state in the pinned upload area; returns the launch bound
static int64_t stage_seq(ss_llama* h, int b, int64_t n_steps, int32_t last_id, const int32_t* forced, int64_t n_forced,
                         bool active) {
    const ss_llama_config& g = h->cfg;
    const int64_t limit = n_steps < g.max_new ? n_steps : g.max_new;
    int64_t eff = limit;
    for (int64_t i = 0; i < n_forced && i < eff; ++i)
        if (forced[i] == g.eos_id || forced[i] == h->stop2) { eff = i + 1; break; }  // the host already knows where it stops
    fill_state(h->upload() + (size_t)b * ST_WORDS, h->kv_len[b], h->pos[b], !active, last_id, n_forced, limit,
               (g.eos_id >= 0 ? (g.eos_id & 0xFFFF) : 0xFFFF) | ((h->stop2 + 1) << 16));
    return active ? eff : 0;
}

int ss_llama_generate(ss_llama* h, int64_t n_steps, int32_t last_prompt_id, const int32_t* host_forced,
                      int64_t n_forced, int64_t* host_n_generated, void* stream) {
    SS_REQUIRE(h && n_steps > 0, "llama_generate: bad arguments");
    const ss_llama_config& g = h->cfg;
    hipStream_t s = (hipStream_t)stream;
    const int q = h->cur;
    const int64_t limit = n_steps < g.max_new ? n_steps : g.max_new;
    SS_REQUIRE(n_forced >= 0 && n_forced <= g.max_new, "llama_generate: n_forced out of range");
    SS_REQUIRE(h->kv_len[q] + limit <= g.cache_cap, "llama_generate: KV cache overflow (%lld + %lld > %d)",
               (long long)h->kv_len[q], (long long)limit, g.cache_cap);
    SS_REQUIRE(h->pos[q] + limit <= g.max_pos, "llama_generate: position overflow (%lld + %lld > %d)", (long long)h->pos[q],
               (long long)limit, g.max_pos);
    if (int crc = capture_fits(h, h->kv_len[q], limit, "llama_generate")) return crc;
    if (int hrc = history_fits(h, q, limit, "llama_generate")) return hrc;
    const bool spec = h->spec.hdr != nullptr;
    if (spec) {         // what a speculative step is not built for: refused before anything is launched
        SS_REQUIRE(!h->samp_on[q], "llama_generate: speculation is on and slot %d has sampling on (speculative sampling is not built)", q);
        SS_REQUIRE(!h->rules_on[q], "llama_generate: speculation is on and slot %d has logits rules on (the rules read one row)", q);
        SS_REQUIRE(!h->lp_on[q], "llama_generate: speculation is on and slot %d records log-probabilities", q);
        SS_REQUIRE(!h->kq, "llama_generate: speculation is on and so is the fp8 KV shadow (ss_llama_set_kv8 off first)");
        SS_REQUIRE(!h->cap.maps, "llama_generate: speculation is on and so is attention-map capture");
        SS_REQUIRE(h->hist_len[q] + limit <= h->hist_cap(),
                   "llama_generate: speculation is on and the token history of slot %d would outgrow its buffer (%lld + %lld > %lld)", q,
                   (long long)h->hist_len[q], (long long)limit, (long long)h->hist_cap());
        SS_HIP(hipMemsetAsync(&h->spec.hdr->pending, 0, sizeof(SpecHdr) - offsetof(SpecHdr, pending), s));
    }
    if (n_forced > 0)
        SS_HIP(hipMemcpyAsync(h->forced + (size_t)q * g.max_new, host_forced, (size_t)n_forced * sizeof(int32_t),
                              hipMemcpyHostToDevice, s));
    // state upload staged in pinned memory; consumed before this call returns (sync_lengths syncs)
    const int64_t eff_limit = stage_seq(h, q, n_steps, last_prompt_id, host_forced, n_forced, true);
    h->spec_run = spec;
    int rc = run_decode(h, q, 1, eff_limit, s);
    h->spec_run = false;
    if (rc) return rc;
    if (spec) h->hist_len[q] += h->pinned[q * ST_WORDS + ST_NGEN];      // every emitted token joined the history on the device
    if (host_n_generated) *host_n_generated = h->pinned[q * ST_WORDS + ST_NGEN];
    return SS_OK;
}

int ss_llama_generate_batch(ss_llama* h, int64_t n_steps, const int32_t* last_prompt_ids, const int32_t* host_forced,
                            int64_t forced_ld, const int64_t* n_forced, const int32_t* active,
                            int64_t* host_n_generated, void* stream) {
    SS_REQUIRE(h && n_steps > 0 && last_prompt_ids, "llama_generate_batch: bad arguments");
    SS_REQUIRE(!h->cap.maps, "llama_generate_batch: attention capture is a single-sequence tool (use ss_llama_generate on the selected slot)");
    const ss_llama_config& g = h->cfg;
    hipStream_t s = (hipStream_t)stream;
    const int64_t limit = n_steps < g.max_new ? n_steps : g.max_new;
    int64_t eff_limit = 0;
    for (int b = 0; b < h->n_seq; ++b) {
        const bool on = !active || active[b];
        const int64_t nf = (n_forced && host_forced) ? n_forced[b] : 0;
        SS_REQUIRE(nf >= 0 && nf <= g.max_new && nf <= forced_ld, "llama_generate_batch: n_forced[%d] out of range", b);
        SS_REQUIRE(!on || h->kv_len[b] + limit <= g.cache_cap,
                   "llama_generate_batch: KV cache overflow in slot %d (%lld + %lld > %d)", b, (long long)h->kv_len[b],
                   (long long)limit, g.cache_cap);
        SS_REQUIRE(!on || h->pos[b] + limit <= g.max_pos, "llama_generate_batch: position overflow in slot %d (%lld + %lld > %d)",
                   b, (long long)h->pos[b], (long long)limit, g.max_pos);
        if (on)
            if (int hrc = history_fits(h, b, limit, "llama_generate_batch")) return hrc;
        const int32_t* f = host_forced ? host_forced + (size_t)b * forced_ld : nullptr;
        if (on && nf > 0)
            SS_HIP(hipMemcpyAsync(h->forced + (size_t)b * g.max_new, f, (size_t)nf * sizeof(int32_t),
                                  hipMemcpyHostToDevice, s));
        const int64_t eff = stage_seq(h, b, n_steps, last_prompt_ids[b], f, on ? nf : 0, on);
        if (eff > eff_limit) eff_limit = eff;
    }
    int rc = run_decode(h, 0, h->n_seq, eff_limit, s);
    if (rc) return rc;
    if (host_n_generated)
        for (int b = 0; b < h->n_seq; ++b) host_n_generated[b] = h->pinned[b * ST_WORDS + ST_NGEN];
    return SS_OK;
}

static size_t spec_carve_cfg(const ss_llama_config& g, int rows, void* ws, SpecPtrs* p) {
    const int hd = g.hidden / g.n_heads;
    return spec_carve(ws, rows, ST_WORDS, (size_t)g.hidden, (size_t)g.inter, (size_t)g.vocab, dtype_size(g.dtype),
                      ss_attn_decode_workspace_bytes(g.n_heads, hd), p);
}

int ss_llama_spec_bytes(const ss_llama_config* cfg, int32_t rows, size_t* bytes) {
    SS_REQUIRE(cfg && bytes, "llama_spec_bytes: null argument");
    SS_REQUIRE(rows >= 2 && rows <= kSpecMaxRows, "llama_spec_bytes: rows %d outside [2, %d]", (int)rows, kSpecMaxRows);
    SS_REQUIRE(cfg->hidden > 0 && cfg->n_heads > 0 && cfg->inter > 0 && cfg->vocab > 0, "llama_spec_bytes: bad config");
    *bytes = spec_carve_cfg(*cfg, rows, nullptr, nullptr);
    return SS_OK;
}

int ss_llama_set_speculation(ss_llama* h, const ss_spec_params* p, void* spec_ws) {
    SS_REQUIRE(h, "llama_set_speculation: null handle");
    if (!p) {           // off: the graphs captured over the workspace go with it
        drop_graphs(h, &SeqGraph::spec);
        h->spec.hdr = nullptr;
        h->spec_rows = 0;
        return SS_OK;
    }
    SS_REQUIRE(spec_ws, "llama_set_speculation: null workspace");
    SS_REQUIRE(((size_t)spec_ws & 255) == 0, "llama_set_speculation: the workspace must be 256-byte aligned");
    SS_REQUIRE(p->rows >= 2 && p->rows <= kSpecMaxRows, "llama_set_speculation: rows %d outside [2, %d]", (int)p->rows, kSpecMaxRows);
    SS_REQUIRE(p->source == SS_SPEC_LOOKUP || p->source == SS_SPEC_GIVEN, "llama_set_speculation: unknown draft source %d", (int)p->source);
    SS_REQUIRE(p->source != SS_SPEC_LOOKUP || (p->max_ngram >= 1 && p->max_ngram <= 8), "llama_set_speculation: max_ngram %d outside [1, 8]",
               (int)p->max_ngram);
    SS_REQUIRE(p->source != SS_SPEC_GIVEN || (p->given_ids && p->given_len >= 0),
               "llama_set_speculation: given drafts need a device array (given_ids) and given_len >= 0");
    // every decode loop of this engine has synchronised before it returned: nothing in flight reads the workspace
    drop_graphs(h, &SeqGraph::spec);
    SpecPtrs ptrs;
    spec_carve_cfg(h->cfg, p->rows, spec_ws, &ptrs);
    SpecHdr hdr;
    memset(&hdr, 0, sizeof(hdr));
    hdr.rows = p->rows; hdr.max_ngram = p->source == SS_SPEC_LOOKUP ? p->max_ngram : 0; hdr.source = p->source;
    hdr.given_len = p->source == SS_SPEC_GIVEN ? p->given_len : 0;
    hdr.given = p->source == SS_SPEC_GIVEN ? p->given_ids : nullptr;
    SS_HIP(hipMemcpy(ptrs.hdr, &hdr, sizeof(hdr), hipMemcpyHostToDevice));
    h->spec = ptrs;
    h->spec_rows = p->rows;
    return SS_OK;
}

int ss_llama_spec_stats(ss_llama* h, int32_t seq, int64_t out[4]) {
    SS_REQUIRE(h && out, "llama_spec_stats: null argument");
    SS_REQUIRE(seq >= -1 && seq < h->n_seq, "llama_spec_stats: sequence slot %d out of range (-1 = the selected slot, < %d)", (int)seq,
               h->n_seq);
    SS_REQUIRE(h->spec.hdr, "llama_spec_stats: speculation is off");
    int32_t v[4];
    SS_HIP(hipMemcpy(v, h->spec.hdr->stats, sizeof(v), hipMemcpyDeviceToHost));
    for (int i = 0; i < 4; ++i) out[i] = v[i];
    return SS_OK;
}

int ss_spec_draft(const int32_t* hist_dev, int64_t len, int32_t max_ngram, int32_t k, int32_t n_stop, const int32_t* stop_ids,
                  int32_t* out_ids_dev, int32_t* out_count_dev, void* stream) {
    SS_REQUIRE(hist_dev && out_ids_dev && out_count_dev, "spec_draft: null argument");
    SS_REQUIRE(len >= 1 && len <= 0x7fffffff && max_ngram >= 1 && k >= 1 && k < kSpecMaxRows,
               "spec_draft: bad arguments (len=%lld max_ngram=%d k=%d; len >= 1, max_ngram >= 1, 1 <= k <= %d)", (long long)len,
               (int)max_ngram, (int)k, kSpecMaxRows - 1);
    SS_REQUIRE(n_stop >= 0 && n_stop <= 2 && (stop_ids || n_stop == 0), "spec_draft: n_stop %d outside [0, 2]", (int)n_stop);
    hipLaunchKernelGGL(spec_draft_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, hist_dev, (int)len, (int)max_ngram, (int)k,
                       n_stop > 0 ? stop_ids[0] : -1, n_stop > 1 ? stop_ids[1] : -1, out_ids_dev, out_count_dev);
    SS_LAUNCH_CHECK("spec_draft");
    return SS_OK;
}

size_t ss_llama_beam_bytes(const ss_llama_config* cfg, int32_t num_beams) {
    if (!cfg || num_beams < 1 || num_beams > kBeamMax || cfg->max_new <= 0) return 0;
    return beam_state_bytes(num_beams, cfg->max_new);
}

size_t ss_llama_beam_seq_offset(void) { return beam_seq_off(); }

// what every beam entry point refuses, before anything is launched or changed
static int beam_refusals(const ss_llama* h, const void* beam_ws, int n, const char* who) {
    SS_REQUIRE(h && beam_ws, "%s: null argument", who);
    SS_REQUIRE(((size_t)beam_ws & 15) == 0, "%s: the workspace must be 16-byte aligned", who);
    SS_REQUIRE(n >= 1 && n <= h->n_seq && n <= kBeamMax, "%s: num_beams %d outside [1, min(n_seq = %d, %d)]", who, n, h->n_seq, kBeamMax);
    SS_REQUIRE(h->cur == 0, "%s: the prompt must be on slot 0 (slot %d is selected)", who, h->cur);
    SS_REQUIRE(!h->kq, "%s: the fp8 KV shadow is on; permuting the shadow is not built (ss_llama_set_kv8 off first)", who);
    SS_REQUIRE(!h->cap.maps, "%s: attention capture is a single-sequence tool", who);
    SS_REQUIRE(!h->logprobs_in(0, n), "%s: a slot of the group records log-probabilities", who);
    SS_REQUIRE(!h->sampling_in(0, n), "%s: a slot of the group has sampling on (beam-search sampling is not built)", who);
    for (int b = 1; b < n; ++b)
        SS_REQUIRE(h->rules_on[b] == h->rules_on[0], "%s: history rules are on for only some slots of the group", who);
    SS_REQUIRE(((size_t)h->hd * h->esz) % 16 == 0, "%s: a cache row of %zu bytes is no multiple of the 16-byte packet", who,
               (size_t)h->hd * h->esz);
    return SS_OK;
}

int ss_llama_beam_search(ss_llama* h, const ss_beam_params* p, void* beam_ws, int64_t n_steps, int32_t last_prompt_id,
                         void* stream) {
    SS_REQUIRE(h && p, "llama_beam_search: null argument");
    const int n = p->num_beams;
    if (int rc = beam_refusals(h, beam_ws, n, "llama_beam_search")) return rc;
    const ss_llama_config& g = h->cfg;
    hipStream_t s = (hipStream_t)stream;
    SS_REQUIRE(n_steps >= 1 && n_steps <= g.max_new, "llama_beam_search: n_steps %lld outside [1, max_new = %d]", (long long)n_steps,
               g.max_new);
    SS_REQUIRE(p->length_penalty == p->length_penalty && p->length_penalty <= 3.4028234e38f && p->length_penalty >= -3.4028234e38f,
               "llama_beam_search: length_penalty must be finite");
    SS_REQUIRE(p->early_stopping >= 0 && p->early_stopping <= 2, "llama_beam_search: early_stopping %d outside 0..2 (False, True, never)",
               (int)p->early_stopping);
    SS_REQUIRE(h->kv_len[0] + n_steps <= g.cache_cap, "llama_beam_search: KV cache overflow (%lld + %lld > %d)", (long long)h->kv_len[0],
               (long long)n_steps, g.cache_cap);
    SS_REQUIRE(h->pos[0] + n_steps <= g.max_pos, "llama_beam_search: position overflow (%lld + %lld > %d)", (long long)h->pos[0],
               (long long)n_steps, g.max_pos);
    if (int hrc = history_fits(h, 0, n_steps, "llama_beam_search")) return hrc;
    int rc;
    if (n > 1) {
        int32_t dst[kBeamMax];
        for (int b = 1; b < n; ++b) dst[b - 1] = b;
        if ((rc = ss_llama_fork(h, 0, dst, n - 1, stream))) return rc;
    }
    BeamHdr hd;
    memset(&hd, 0, sizeof(hd));
    hd.n = n;
    hd.stop_ids[0] = hd.stop_ids[1] = -1;
    if (g.eos_id >= 0) hd.stop_ids[hd.n_stop++] = g.eos_id;
    if (h->stop2 >= 0 && h->stop2 != g.eos_id) hd.stop_ids[hd.n_stop++] = h->stop2;
    hd.K = (hd.n_stop + 1 > 2 ? hd.n_stop + 1 : 2) * n;
    hd.limit = (int32_t)n_steps; hd.max_new = g.max_new; hd.early_stopping = p->early_stopping;
    hd.length_penalty = p->length_penalty;
    hd.kv0 = (int32_t)h->kv_len[0]; hd.hist0 = (int32_t)h->hist_len[0];
    hd.unsat = 1;
    for (int b = 0; b < kBeamMax; ++b) {
        hd.run_score[b] = b == 0 ? 0.f : -INFINITY;
        hd.run_live[b] = b == 0 ? 1 : 0;
        hd.fin_score[b] = -INFINITY;
        hd.parent[b] = b;
    }
    // (pageable source: the copy is staged before the call returns)
    SS_HIP(hipMemcpyAsync(beam_ws, &hd, sizeof(hd), hipMemcpyHostToDevice, s));
    for (int b = 0; b < n; ++b) stage_seq(h, b, n_steps, last_prompt_id, nullptr, 0, true);
    h->beam = beam_ptrs(beam_ws, n, g.max_new);
    h->beam_rows = (int)n_steps;
    rc = run_decode(h, 0, n, n_steps, s);
    h->beam.hdr = nullptr;
    return rc;
}

int ss_llama_beam_permute(ss_llama* h, void* beam_ws, const int32_t* host_parent, int32_t n, int64_t kv0, int64_t hist0,
                          void* stream) {
    SS_REQUIRE(host_parent, "llama_beam_permute: null argument");
    if (int rc = beam_refusals(h, beam_ws, n, "llama_beam_permute")) return rc;
    const int64_t kv = h->kv_len[0];
    SS_REQUIRE(kv0 >= 0 && kv0 <= kv && hist0 >= 0 && hist0 <= h->hist_len[0], "llama_beam_permute: kv0 %lld / hist0 %lld out of range",
               (long long)kv0, (long long)hist0);
    BeamHdr hd;
    memset(&hd, 0, sizeof(hd));
    hd.n = n; hd.kv0 = (int32_t)kv0; hd.hist0 = (int32_t)hist0;
    for (int b = 0; b < kBeamMax; ++b) hd.parent[b] = b;
    for (int b = 0; b < n; ++b) {
        SS_REQUIRE(host_parent[b] >= 0 && host_parent[b] < n, "llama_beam_permute: parent[%d] = %d outside [0, %d)", b, (int)host_parent[b], n);
        hd.parent[b] = host_parent[b];
    }
    hipStream_t s = (hipStream_t)stream;
    SS_HIP(hipMemcpyAsync(beam_ws, &hd, sizeof(hd), hipMemcpyHostToDevice, s));
    // the device words the kernels read: slot 0 not done, its cache length
    hipLaunchKernelGGL(set_state_kernel, dim3(1), dim3(64), 0, s, h->state, (int)ST_DONE, 0, (int)ST_KV_LEN, (int)kv);
    SS_LAUNCH_CHECK("set_state");
    const int64_t span = kv - kv0 > h->hist_len[0] - hist0 ? kv - kv0 : h->hist_len[0] - hist0;
    h->beam = beam_ptrs(beam_ws, n, h->cfg.max_new);
    int rc = span > 0 ? beam_permute_launch(h, (int)span, h->rules_on[0] != 0, s) : SS_OK;
    h->beam.hdr = nullptr;
    return rc;
}

int ss_llama_profile_decode(ss_llama* h, int64_t n_tokens, float out_ms[8], double out_bytes[4], void* stream) {
    SS_REQUIRE(h && n_tokens > 0 && out_ms && out_bytes, "llama_profile_decode: bad arguments");
    const ss_llama_config& g = h->cfg;
    hipStream_t s = (hipStream_t)stream;
    for (int b = 0; b < h->n_seq; ++b) {
        SS_REQUIRE(h->kv_len[b] + n_tokens + 1 <= g.cache_cap, "llama_profile_decode: KV cache too full (slot %d)", b);
        if (int hrc = history_fits(h, b, n_tokens, "llama_profile_decode")) return hrc;
        fill_state(h->upload() + (size_t)b * ST_WORDS, h->kv_len[b], h->pos[b], false, 0, 0, g.max_new, -1);
    }
    SS_HIP(hipMemcpyAsync(h->state, h->upload(), (size_t)h->n_seq * ST_WORDS * sizeof(int32_t), hipMemcpyHostToDevice, s));
    if (int rc = kv8_sync(h, 0, h->n_seq, s)) return rc;
    for (int i = 0; i < 8; ++i) out_ms[i] = 0.f;
    double cnt[4] = {0, 0, 0, 0};
    for (int64_t t = 0; t < n_tokens && t < g.max_new - 1; ++t) {
        ProfSink p;
        p.s = s;
        int rc = decode_token(h, s, &p, 0, h->n_seq);
        hipError_t e = hipStreamSynchronize(s);
        if (!rc && e == hipSuccess) {
            for (size_t i = 1; i < p.ev.size(); ++i) {
                float ms = 0.f;
                hipEventElapsedTime(&ms, p.ev[i - 1], p.ev[i]);
                if (p.cls[i] >= 0 && p.cls[i] < 4) { out_ms[p.cls[i]] += ms; cnt[p.cls[i]] += 1; }
            }
            float tot = 0.f;
            hipEventElapsedTime(&tot, p.ev.front(), p.ev.back());
            out_ms[4] += tot;
        }
        for (hipEvent_t ev : p.ev) hipEventDestroy(ev);
        if (rc) return rc;
        SS_HIP(e);
    }
    for (int i = 0; i < 8; ++i) out_ms[i] /= (float)n_tokens;
    const double H = g.hidden, I = g.inter;
    // class 0 = every GEMV except the down projection (qkv, o, gate|up per layer + lm_head); class 2 = down
    // (fp8 decode weights: one byte per weight + the fp32 row scales; MXFP4: half a byte per weight + one scale byte per 32)
    const bool w8 = !h->w8.empty(), mx4 = !h->mx4.empty();
    const double wb = mx4 ? 0.5 + 1.0 / 32.0 : w8 ? 1.0 : (double)h->esz;
    out_bytes[0] = ((double)g.n_layers * (4.0 * H * H + 2.0 * H * I) + (double)g.vocab * H) * wb;
    out_bytes[1] = cnt[0] / (double)n_tokens;
    out_bytes[2] = (double)g.n_layers * H * I * wb;
    if (w8) {
        out_bytes[0] += 4.0 * ((double)g.n_layers * (4.0 * H + 2.0 * I) + (double)g.vocab);
        out_bytes[2] += 4.0 * (double)g.n_layers * H;
    }
    out_bytes[3] = cnt[2] / (double)n_tokens;
    if (int rc = sync_lengths(h, 0, h->n_seq, s)) return rc;
    kv8_advance(h, 0, h->n_seq);
    return rules_finish(h, 0, h->n_seq, s);
}

}  // extern "C"
