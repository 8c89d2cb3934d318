// Prompt-lookup speculative decoding on the device (definition: include/seedstory_hip.h, ss_llama_set_speculation / ss_spec_draft).
//   draft        n-gram lookup in the slot's token history by one block: per n-gram size, every thread scans its start indices in
//                ascending order and keeps its first match; the block minimum is the leftmost one.
//   spec_open    the opening kernel of a speculative step, one block of 1024 threads: settles the previous step's R logits rows,
//                emits, appends to the history, drafts, writes the row-state blocks, embeds the rows.
//   spec_final_norm   the final RMSNorm of the used rows: lm_head input + hidden row n0 + r.
// No atomics, no grid-wide waits: the seams between these kernels are kernel boundaries.
#pragma once
#include "ss_common.h"
#include "ss_sample.h"

namespace ss {

constexpr int kSpecMaxRows = SS_SPEC_MAX_ROWS;

// The head of the caller-owned speculation workspace.  The first block is written by ss_llama_set_speculation, the second by
// ss_llama_generate (zeroed) and the opening kernel.  Behind it (spec_ptrs): row states, activations, logits rows, partials.
struct SpecHdr {
    int32_t rows, max_ngram, source, given_len;
    const int32_t* given;
    int32_t pending;            // rows of the step in flight whose logits are not settled yet (0 = none)
    int32_t n_active;           // rows the running step uses (the attention kernel's A)
    int32_t n0;                 // generated index of row 0 of the running step
    int32_t pad;
    int32_t stats[4];           // steps, rows drafted, drafts accepted, tokens emitted
    int32_t tok[kSpecMaxRows];  // the rows' tokens: tok[0] chosen, tok[1 ..] drafted
};

// state words of a slot as the engine keeps them (ss_llama.hip)
struct SpecSt { int kv_len, pos, ngen, done, last, nforced, limit, eos, words; };

struct SpecPtrs {
    SpecHdr* hdr;               // nullptr: speculation is off
    int32_t* row_st;            // [R][words]
    char *x, *xn, *qkv, *attn, *hm, *logits;
    float* attn_ws;
};
inline size_t spec_align(size_t v) { return (v + 255) / 256 * 256; }
// the carve of a workspace (ws == NULL: sizes only); returns the bytes used
inline size_t spec_carve(void* ws, int R, int words, size_t H, size_t I, size_t vocab, size_t esz, size_t attn_ws_bytes, SpecPtrs* p) {
    char* b = (char*)ws;
    size_t off = 0;
    auto take = [&](size_t bytes) { char* q = b ? b + off : nullptr; off += spec_align(bytes); return q; };
    SpecPtrs t;
    t.hdr = (SpecHdr*)take(sizeof(SpecHdr));
    t.row_st = (int32_t*)take((size_t)R * words * sizeof(int32_t));
    t.x = take((size_t)R * H * esz);
    t.xn = take((size_t)R * H * esz);
    t.qkv = take((size_t)R * 3 * H * esz);
    t.attn = take((size_t)R * H * esz);
    t.hm = take((size_t)R * I * esz);
    t.logits = take((size_t)R * vocab * esz);
    t.attn_ws = (float*)take((size_t)R * attn_ws_bytes);
    if (p) *p = t;
    return off;
}

// block minimum of an int (same value in every thread); red: >= 16 ints of LDS
__device__ __forceinline__ int spec_block_min(int v, int* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int other = __shfl_xor(v, o, 64);
        v = other < v ? other : v;
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    __syncthreads();
    if (lane == 0) red[wid] = v;
    __syncthreads();
    int r = red[0];
    for (int w = 1; w < nw; ++w) r = red[w] < r ? red[w] : r;
    return r;
}

// PromptLookupCandidateGenerator.get_candidates on hist[0 .. len): thread 0 writes out[0 .. count), every thread returns count
// (<= k).  stop_a / stop_b: ids the draft is cut in front of (negative = none), as it is in front of an id outside [0, max_id).
// All threads of one block; hist complete and visible.
__device__ __forceinline__ int spec_lookup_block(const int32_t* hist, int len, int max_ngram, int k, int stop_a, int stop_b, int max_id,
                                                 int32_t* out, int* red) {
    int start = -1;
    for (int g = max_ngram < len - 1 ? max_ngram : len - 1; g >= 1 && start < 0; --g) {
        int best = 0x7fffffff;
        for (int idx = threadIdx.x; idx + g < len; idx += blockDim.x) {    // idx + g < len: the continuation is not empty
            bool ok = true;
            for (int j = 0; j < g; ++j) ok = ok && hist[idx + j] == hist[len - g + j];
            if (ok) { best = idx; break; }
        }
        best = spec_block_min(best, red);
        if (best != 0x7fffffff) start = best + g;
    }
    if (start < 0) return 0;
    int n = len - start < k ? len - start : k;
    for (int i = 0; i < n; ++i) {
        const int t = hist[start + i];
        if (t == stop_a || t == stop_b || (unsigned)t >= (unsigned)max_id) { n = i; break; }
    }
    if (threadIdx.x == 0)
        for (int i = 0; i < n; ++i) out[i] = hist[start + i];
    return n;
}

// ---- ss_spec_draft -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void spec_draft_kernel(const int32_t* __restrict__ hist, int len, int max_ngram, int k, int stop_a,
                                                          int stop_b, int32_t* out, int32_t* out_count) {
    __shared__ int red[16];
    const int n = spec_lookup_block(hist, len, max_ngram, k, stop_a, stop_b, 0x7fffffff, out, red);
    if (threadIdx.x == 0) *out_count = n;
}

// ---- the engine's speculative step ---------------------------------------------------------------------------------------------
// One block of 1024 threads for the slot.  slot_logits: the slot's logits row (what a greedy token reads and edits in place);
// row_logits [R][vocab]: the step's rows.  The loop below is greedy's opening kernel (ss_llama.hip, sample_embed_kernel) run once
// per emitted token: row r of the previous step is copied to the slot's row, edited and arg-maxed there exactly as greedy would
// have, so the slot's row, the ids, ST_NGEN / ST_LAST / ST_DONE and kv_len / pos end up as the greedy kernels leave them.
template <typename T>
__global__ __launch_bounds__(1024) void spec_open_kernel(T* slot_logits, const T* __restrict__ row_logits, int vocab, int32_t* st, SpecSt w,
                                                         SpecHdr* hdr, int32_t* row_st, const int32_t* __restrict__ img_ids, int n_img_ids,
                                                         const int32_t* __restrict__ forced, int32_t* gen_ids, int32_t* hist,
                                                         int hist_cap, int32_t* hist_len_p, int32_t* n_app_p, uint32_t* bitmap,
                                                         const T* __restrict__ embed, T* x, int hidden, int max_new, int cache_cap,
                                                         int max_pos) {
    __shared__ float sv[16];
    __shared__ int si[16];
    __shared__ int s_nd;
    __shared__ int32_t s_draft[kSpecMaxRows];
    if (st[w.done]) return;
    const int R = hdr->rows < kSpecMaxRows ? hdr->rows : kSpecMaxRows;
    const int A = hdr->pending;
    int kv = st[w.kv_len], pos = st[w.pos], n = st[w.ngen], last = st[w.last], hl = *hist_len_p;
    const int nforced = st[w.nforced], limit = st[w.limit];
    const int eos_word = st[w.eos];
    const int eos_id = eos_word & 0xFFFF, stop2 = (eos_word >> 16) - 1;
    int prev_tok[kSpecMaxRows];
#pragma unroll
    for (int r = 0; r < kSpecMaxRows; ++r) prev_tok[r] = hdr->tok[r];
    if (A > 0) { kv += 1; pos += 1; }       // row 0 of the previous step carried the token emitted before it: forwarded now
    int r = 0, accepted = 0, emitted = 0;
    bool stop = false;
    __syncthreads();            // every thread has read the state words before thread 0 writes any
    for (;;) {
        if (A > 0) {            // the row after the last settled token becomes the slot's row
            const T* src = row_logits + (int64_t)r * vocab;
            for (int i = threadIdx.x; i < vocab; i += blockDim.x) slot_logits[i] = src[i];
            __threadfence_block();
            __syncthreads();
        }
        int tok = imgproc_argmax_block<T>(slot_logits, vocab, last, img_ids, n_img_ids, sv, si);
        if ((unsigned)tok >= (unsigned)vocab) tok = 0;
        if (n < nforced) tok = forced[n];
        stop = (tok == eos_id) || (tok == stop2) || (n + 1 >= limit);
        if (threadIdx.x == 0) {
            gen_ids[n] = tok;
            if (hl < hist_cap) {
                hist[hl] = tok;
                if ((unsigned)tok < (unsigned)vocab) bitmap[tok >> 5] |= 1u << (tok & 31);
            }
        }
        if (hl < hist_cap) ++hl;
        last = tok;
        ++n;
        ++emitted;
        if (stop) break;
        int next = -1;
#pragma unroll
        for (int j = 1; j < kSpecMaxRows; ++j)
            if (j == r + 1 && j < A) next = prev_tok[j];
        if (next != tok) break;             // rejected (or no draft left): tok is row 0 of the next step
        ++accepted; ++kv; ++pos; ++r;       // accepted: its row r was forwarded at this very position
    }
    __threadfence_block();
    __syncthreads();
    // ---- open the next step: row 0 = the token just emitted (generated index n - 1), drafts behind it -------------------------
    int rows = 0;
    if (!stop) {
        const int n0 = n - 1;
        int want = R;
        want = want < limit - 1 - n0 ? want : limit - 1 - n0;      // the last token of the call is never forwarded
        want = want < max_new - n0 ? want : max_new - n0;
        want = want < cache_cap - kv ? want : cache_cap - kv;
        want = want < max_pos - pos ? want : max_pos - pos;
        want -= 1;              // drafts wanted
        int nd = 0;
        if (want > 0) {
            if (n < nforced || hdr->source == SS_SPEC_GIVEN) {
                if (threadIdx.x == 0) {
                    const bool f = n < nforced;
                    const int32_t* ids = f ? forced : hdr->given;
                    const int end = f ? nforced : hdr->given_len;
                    int c = 0;
                    for (; c < want && n + c < end; ++c) {
                        const int t = ids[n + c];
                        if (t == eos_id || t == stop2 || (unsigned)t >= (unsigned)vocab) break;
                        s_draft[c] = t;
                    }
                    s_nd = c;
                }
                __syncthreads();
                nd = s_nd;
            } else {
                nd = spec_lookup_block(hist, hl, hdr->max_ngram, want, eos_id == 0xFFFF ? -1 : eos_id, stop2, vocab, s_draft, si);
                __syncthreads();
            }
        }
        rows = 1 + nd;
        constexpr int V = Tr<T>::kVec;
        for (int q = 0; q < rows; ++q) {
            const int t = q ? s_draft[q - 1] : last;
            for (int p = threadIdx.x; p < hidden / V; p += blockDim.x)
                st16(x + (int64_t)q * hidden + (int64_t)p * V, ld16(embed + (int64_t)t * hidden + (int64_t)p * V));
        }
    }
    if (threadIdx.x == 0) {
        st[w.kv_len] = kv; st[w.pos] = pos; st[w.ngen] = n; st[w.last] = last;
        if (stop) st[w.done] = 1;
        *hist_len_p = hl;
        *n_app_p = n;
        hdr->pending = rows; hdr->n_active = rows; hdr->n0 = n - 1;
        hdr->stats[0] += rows > 0 ? 1 : 0; hdr->stats[1] += rows > 0 ? rows - 1 : 0; hdr->stats[2] += accepted; hdr->stats[3] += emitted;
        for (int q = 0; q < kSpecMaxRows; ++q) {
            if (q < R) {
                int32_t* rs = row_st + q * w.words;
                rs[w.kv_len] = kv + q; rs[w.pos] = pos + q; rs[w.done] = q < rows ? 0 : 1;
            }
            hdr->tok[q] = q == 0 ? last : (q < rows ? s_draft[q - 1] : -1);
        }
    }
}

// final RMSNorm of the step's rows (final_norm_advance_kernel's arithmetic): row r -> the lm_head input row r and the hidden-state
// ring row n0 + r.  kv_len / pos advance in the next opening kernel, once it knows how many rows were right.
template <typename T>
__global__ __launch_bounds__(256) void spec_final_norm_kernel(const T* __restrict__ x, const T* __restrict__ nw, T* xn, T* hid_rows,
                                                              const SpecHdr* hdr, int hidden, float eps, int max_new) {
    constexpr int V = Tr<T>::kVec;
    __shared__ float red[16];
    const int r = blockIdx.x;
    const int row = hdr->n0 + r;
    if (r >= hdr->n_active || row < 0 || row >= max_new) return;
    x += (int64_t)r * hidden;
    xn += (int64_t)r * hidden;
    const int npack = hidden / V;
    float ssq = 0.f;
    for (int p = threadIdx.x; p < npack; p += 256) {
        float f[V];
        unpack<T>(ld16(x + (int64_t)p * V), f);
#pragma unroll
        for (int j = 0; j < V; ++j) ssq = fmaf(f[j], f[j], ssq);
    }
    const float rstd = 1.0f / sqrtf(block_sum(ssq, red) / (float)hidden + eps);
    T* out = hid_rows + (int64_t)row * hidden;
    for (int p = threadIdx.x; p < npack; p += 256) {
        float f[V], g[V];
        unpack<T>(ld16(x + (int64_t)p * V), f);
        unpack<T>(ld16(nw + (int64_t)p * V), g);
#pragma unroll
        for (int j = 0; j < V; ++j) f[j] = g[j] * Tr<T>::rnd(f[j] * rstd);
        const uint4 o = pack<T>(f);
        st16(xn + (int64_t)p * V, o);
        st16(out + (int64_t)p * V, o);
    }
}

}  // namespace ss
