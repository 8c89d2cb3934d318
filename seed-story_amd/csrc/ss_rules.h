// Hugging Face's three history rules on one logits row, in front of the image-token processor (ss_sample.h):
//   repetition penalty -> no-repeat n-gram -> min_new_tokens   (the order of HF's processor list)
// Definition: include/seedstory_hip.h, ss_process_logits.  z = the row in the model dtype T, hist = the slot's token history.
//   1. every id that occurs in hist, once however often it occurs:  z_i <- round_T(z_i < 0 ? z_i * p : z_i / p), fp32 with a
//      correctly rounded division, one rounding to T.  NaN stays as it is.  "Once" comes from a bitmap of ceil(vocab / 32)
//      words with one bit per id of hist; no atomics: every word has one owner thread while it is built.
//   2. n > 0 and len + 1 >= n: every id that followed an earlier occurrence of the last n - 1 ids of hist gets -inf.
//   3. len - prompt_len < m: the EOS id gets -inf.
// spare: ids of img_ids keep the value they had before rule 1 (and only rule 1).
// Must be called by all threads of ONE block of 1024 threads.
#pragma once
#include "ss_common.h"

namespace ss {

constexpr int kRulesMaxNgram = SS_LOGITS_RULES_MAX_NGRAM;

// One slot's rules and history bookkeeping in device memory (the engine's block is [n_seq] of these; 32 bytes).  The first
// five words are written by ss_llama_set_logits_rules, hist_len / prompt_len by ss_llama_set_history and by the kernel.
struct RulesState {
    float penalty;
    int32_t ngram, min_new, spare_img;
    int32_t enabled;        // 0 = this slot's row is left alone and its history does not advance
    int32_t hist_len, prompt_len;
    int32_t n_app;          // tokens of the running generate call already appended to the history
};

// ss_logits_rules -> the first five words of the block; SS_EINVAL with a message for a value outside its range
inline int logits_rules_params(const ss_logits_rules* p, const char* who, RulesState* out) {
    SS_REQUIRE(p->repetition_penalty > 0.f && p->repetition_penalty <= 3.4028234e38f, "%s: repetition_penalty %g must be finite and > 0",
               who, (double)p->repetition_penalty);
    SS_REQUIRE(p->no_repeat_ngram >= 0 && p->no_repeat_ngram <= kRulesMaxNgram, "%s: no_repeat_ngram %d outside [0, %d]", who,
               (int)p->no_repeat_ngram, kRulesMaxNgram);
    SS_REQUIRE(p->min_new_tokens >= 0, "%s: min_new_tokens %d < 0", who, (int)p->min_new_tokens);
    out->penalty = p->repetition_penalty;
    out->ngram = p->no_repeat_ngram;
    out->min_new = p->min_new_tokens;
    out->spare_img = p->spare_img_ids ? 1 : 0;
    out->enabled = 1;
    return SS_OK;
}

__host__ __device__ inline int rules_bitmap_words(int64_t vocab) { return (int)((vocab + 31) / 32); }

// bm[w] (|)= the bits of ids[0 .. n) that fall into word w, for the words w = w0, w0 + stride, ... < n_words.  Every word is
// written by the one thread that owns it; ids outside [0, 32 * n_words) match no word.
__device__ __forceinline__ void rules_bitmap_add(uint32_t* bm, int n_words, int w0, int stride, const int32_t* __restrict__ ids, int n,
                                                 bool keep) {
    for (int w = w0; w < n_words; w += stride) {
        uint32_t m = keep ? bm[w] : 0u;
        for (int j = 0; j < n; ++j) {
            const int id = ids[j];
            if ((id >> 5) == w) m |= 1u << (id & 31);
        }
        bm[w] = m;
    }
}

// The three rules on z[0 .. vocab), in place.  bm = the bitmap of hist[0 .. len) (LDS or global; complete and visible to the
// block on entry).  eos < 0 or >= vocab: rule 3 has nothing to ban.  Ids of hist outside [0, vocab) are never used as an index.
template <typename T>
__device__ __forceinline__ void logits_rules_block(T* z, int vocab, float penalty, int ngram, int min_new, bool spare,
                                                   const uint32_t* bm, const int32_t* hist, int len, int prompt_len,
                                                   int eos, const int32_t* __restrict__ img_ids, int n_img_ids) {
    const int tid = threadIdx.x, nt = blockDim.x;
    if (penalty != 1.0f) {
        // spare: thread j keeps entry img_ids[j] as it was and puts it back after the pass
        const bool sp = spare && n_img_ids > 0;
        int keep_id = -1;
        T keep_v = z[0];
        if (sp) {       // n_img_ids <= 1024 = the block (ss_llama_create / ss_process_logits): one id per thread
            if (tid < n_img_ids) {
                const int id = img_ids[tid];
                if ((unsigned)id < (unsigned)vocab) { keep_id = id; keep_v = z[id]; }
            }
            __syncthreads();
        }
        for (int i = tid; i < vocab; i += nt) {
            if (!((bm[i >> 5] >> (i & 31)) & 1u)) continue;
            const float v = Tr<T>::ld(z + i);
            if (v != v) continue;
            Tr<T>::st(z + i, v < 0.f ? v * penalty : __fdiv_rn(v, penalty));
        }
        if (sp) {
            __threadfence_block();
            __syncthreads();
            if (keep_id >= 0) z[keep_id] = keep_v;
        }
        __threadfence_block();
        __syncthreads();
    }
    if (ngram > 0 && len + 1 >= ngram) {
        const int nc = ngram - 1;
        int ctx[kRulesMaxNgram - 1];
#pragma unroll
        for (int k = 0; k < kRulesMaxNgram - 1; ++k) ctx[k] = k < nc ? hist[len - nc + k] : 0;
        for (int j = tid; j + ngram <= len; j += nt) {      // the n-gram that starts at j ends inside hist
            bool same = true;
#pragma unroll
            for (int k = 0; k < kRulesMaxNgram - 1; ++k)
                if (k < nc) same = same && hist[j + k] == ctx[k];
            if (!same) continue;
            const int id = hist[j + nc];
            if ((unsigned)id < (unsigned)vocab) Tr<T>::st(z + id, -INFINITY);
        }
    }
    if (tid == 0 && len - prompt_len < min_new && (unsigned)eos < (unsigned)vocab) Tr<T>::st(z + eos, -INFINITY);
    __threadfence_block();
    __syncthreads();
}

}  // namespace ss
