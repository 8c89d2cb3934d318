// Beam search on the device (definition: include/seedstory_hip.h, ss_llama_beam_search / ss_beam_step).
//   row top-K   one block of 1024 threads per beam row: the row is read ONCE into registers (ss_logprob.h), every entry with
//               mass becomes  running score + log-softmax  (fp32, the fixed summation order of logprob_load_block), and K
//               rounds of a block arg max emit the K best in the order "larger score, then smaller token".  NaN and -inf
//               entries carry no mass and are never emitted; a dead row (no running hypothesis) emits nothing.
//   merge       the n sorted row lists -> the K best overall, equal scores by ascending beam * vocab + token (one thread: n * K
//               comparisons).
//   advance     Hugging Face's update of the running and the finished hypotheses and its stop rule on a BeamState in device
//               memory, by one block; the sequences are double-buffered (step parity), so a gather never reads what it wrote.
//   permute     one thread per 16-byte packet position of the cache suffix [kv0, kv_len) ACROSS the n slots: it loads the
//               position from every slot that is somebody's parent, then stores to every slot whose parent is another slot.
//               Positions are independent, so cycles and fan-out are safe in one launch without scratch.
// No atomics, no grid-wide waits: the seams between these kernels are kernel boundaries.
#pragma once
#include <math.h>

#include "ss_common.h"
#include "ss_logprob.h"

namespace ss {

constexpr int kBeamMax = SS_BEAM_MAX;           // beams of one search = sequence slots of the engine
constexpr int kBeamMaxK = 3 * kBeamMax;         // candidates per step: (1 + at most two stop ids) * n

// The head of the caller-owned BeamState workspace (ss_beam_state in include/seedstory_hip.h is this very layout); behind it:
//   float   cand_score[kBeamMax][kBeamMaxK]     the row lists of the running step
//   int32_t cand_tok  [kBeamMax][kBeamMaxK]
//   int32_t run_seq[2][n][max_new]              running sequences, buffer (step & 1) is current
//   int32_t fin_seq[2][n][max_new]              finished sequences, likewise
typedef ss_beam_state BeamHdr;

inline size_t beam_cand_off() { return (sizeof(BeamHdr) + 255) / 256 * 256; }
inline size_t beam_seq_off() { return beam_cand_off() + 2 * (size_t)kBeamMax * kBeamMaxK * 4; }
inline size_t beam_state_bytes(int n, int max_new) { return beam_seq_off() + 4 * (size_t)n * max_new * 4; }

struct BeamPtrs {
    BeamHdr* hdr;               // nullptr: no search is running
    float* cand_score;
    int32_t* cand_tok;
    int32_t* run_seq;           // [2][n][max_new]
    int32_t* fin_seq;           // [2][n][max_new]
};
inline BeamPtrs beam_ptrs(void* ws, int n, int max_new) {
    char* b = (char*)ws;
    BeamPtrs p;
    p.hdr = (BeamHdr*)b;
    p.cand_score = (float*)(b + beam_cand_off());
    p.cand_tok = (int32_t*)(p.cand_score + kBeamMax * kBeamMaxK);
    p.run_seq = (int32_t*)(b + beam_seq_off());
    p.fin_seq = p.run_seq + 2 * (size_t)n * max_new;
    return p;
}

// The K best of  score + log-softmax(row): thread 0 writes toks[0 .. K) and scores[0 .. K) (-1 / -inf where fewer entries carry
// mass).  All 1024 threads of one block.
template <typename T, int EPT>
__device__ __forceinline__ void beam_row_topk_block(const T* row, int vocab, float score, int K, int32_t* toks, float* scores,
                                                    LogprobSmem& sm) {
    float v[EPT];
    int flip = 0;
    const LogprobStats s = logprob_load_block<T, EPT>(row, vocab, v, sm, flip);
#pragma unroll
    for (int k = 0; k < EPT; ++k) v[k] = (s.any && v[k] > -INFINITY) ? logprob_value(v[k], s) + score : -INFINITY;
    const LogprobStats ident{0.f, 0.f, 1};      // the registers hold the scores themselves
    logprob_top_block(v, vocab, ident, K, toks, scores, sm);
}

// n sorted row lists [n][kBeamMaxK] (the first K of each) -> the K best overall.  ONE thread.  Returns how many exist.
__device__ inline int beam_merge(const float* row_score, const int32_t* row_tok, int n, int K, float* out_score, int32_t* out_beam,
                                 int32_t* out_tok) {
    int head[kBeamMax];
    for (int b = 0; b < kBeamMax; ++b) head[b] = 0;
    int nc = 0;
    for (; nc < K; ++nc) {
        int bb = -1;
        float bs = 0.f;
        for (int b = 0; b < n; ++b) {           // ascending beams, strict `>`: equal scores keep the smaller beam
            if (head[b] >= K) continue;
            const int i = b * kBeamMaxK + head[b];
            if (row_tok[i] < 0) continue;       // this row has nothing left
            if (bb < 0 || row_score[i] > bs) { bb = b; bs = row_score[i]; }
        }
        if (bb < 0) break;
        out_score[nc] = bs; out_beam[nc] = bb; out_tok[nc] = row_tok[bb * kBeamMaxK + head[bb]];
        ++head[bb];
    }
    for (int j = nc; j < K; ++j) { out_score[j] = -INFINITY; out_beam[j] = -1; out_tok[j] = -1; }
    return nc;
}

// ---- ss_beam_step: rows one after the other by ONE block (the lists in LDS), then the merge ----------------------------------
template <typename T, int EPT>
__global__ __launch_bounds__(1024) void beam_step_kernel(const T* logits, int rows, int vocab, int64_t ld,
                                                         const float* __restrict__ beam_scores, int K, float* cand_score,
                                                         int32_t* cand_beam, int32_t* cand_tok) {
    __shared__ LogprobSmem sm;
    __shared__ float rs[kBeamMax * kBeamMaxK];
    __shared__ int32_t rt[kBeamMax * kBeamMaxK];
    for (int b = 0; b < rows; ++b) {
        const float sc = beam_scores[b];
        if (sc > -INFINITY) {                   // (uniform) a dead row, or a NaN score, emits nothing
            beam_row_topk_block<T, EPT>(logits + (int64_t)b * ld, vocab, sc, K, rt + b * kBeamMaxK, rs + b * kBeamMaxK, sm);
        } else if (threadIdx.x == 0) {
            for (int j = 0; j < K; ++j) { rs[b * kBeamMaxK + j] = -INFINITY; rt[b * kBeamMaxK + j] = -1; }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) beam_merge(rs, rt, rows, K, cand_score, cand_beam, cand_tok);
}

// ---- the engine's decode token ------------------------------------------------------------------------------------------------
// state words of a slot as the engine keeps them (ss_llama.hip): the beam kernels use these five
struct BeamSt { int kv_len, ngen, done, last, words; };

// one block per beam row: processor edit (in place, as the greedy opening kernel does), then the row's K best
template <typename T, int EPT>
__global__ __launch_bounds__(1024) void beam_topk_kernel(T* logits, int vocab, const int32_t* st, BeamSt w,
                                                         const int32_t* __restrict__ img_ids, int n_img_ids, const BeamHdr* hdr,
                                                         float* cand_score, int32_t* cand_tok) {
    __shared__ LogprobSmem sm;
    __shared__ float sv[16];
    __shared__ int si[16];
    const int b = blockIdx.x;
    st += b * w.words;
    if (st[w.done]) return;
    const int K = hdr->K;
    float* cs = cand_score + b * kBeamMaxK;
    int32_t* ct = cand_tok + b * kBeamMaxK;
    if (!hdr->run_live[b]) {
        if (threadIdx.x == 0)
            for (int j = 0; j < K; ++j) { cs[j] = -INFINITY; ct[j] = -1; }
        return;
    }
    logits += (int64_t)b * vocab;
    imgproc_edit_block<T>(logits, vocab, st[w.last], img_ids, n_img_ids, sv, si);
    beam_row_topk_block<T, EPT>(logits, vocab, hdr->run_score[b], K, ct, cs, sm);
}

// one block per search: merge -> HF's update -> parent / token -> state words, generated ids, embedding rows
template <typename T>
__global__ __launch_bounds__(1024) void beam_advance_kernel(BeamHdr* hdr, const float* cand_score, const int32_t* cand_tok,
                                                            int32_t* run_seq, int32_t* fin_seq, int32_t* st, BeamSt w,
                                                            int32_t* gen_ids, const T* __restrict__ embed, T* x, int hidden) {
    __shared__ int s_parent[kBeamMax], s_token[kBeamMax], s_live[kBeamMax], s_fsrc[kBeamMax], s_flen[kBeamMax];
    __shared__ int s_cb[kBeamMaxK], s_ct[kBeamMaxK];
    __shared__ int s_ended, s_t;
    if (st[w.done]) return;                     // (slot 0's flag: the whole group carries it)
    const int n = hdr->n, max_new = hdr->max_new;
    if (threadIdx.x == 0) {
        const int K = hdr->K, t = hdr->step, limit = hdr->limit, early = hdr->early_stopping;
        const float lp = hdr->length_penalty;
        float cs[kBeamMaxK];
        int cb[kBeamMaxK], ct[kBeamMaxK];
        const int nc = beam_merge(cand_score, cand_tok, n, K, cs, cb, ct);
        const bool at_limit = t + 1 >= limit;
        bool hit[kBeamMaxK], all_hit = true;
        for (int j = 0; j < nc; ++j) {
            hit[j] = at_limit || ct[j] == hdr->stop_ids[0] || ct[j] == hdr->stop_ids[1];
            all_hit = all_hit && hit[j];
            s_cb[j] = cb[j]; s_ct[j] = ct[j];
        }
        // the n best unfinished candidates run on
        int nr = 0;
        float rsc[kBeamMax];
        for (int j = 0; j < nc && nr < n; ++j)
            if (!hit[j]) { rsc[nr] = cs[j]; s_parent[nr] = cb[j]; s_token[nr] = ct[j]; s_live[nr] = 1; ++nr; }
        for (int b = nr; b < n; ++b) { rsc[b] = -INFINITY; s_parent[b] = b; s_token[b] = 0; s_live[b] = 0; }
        // finished candidates among the first n compete for the n finished places (both lists are sorted; the table wins ties)
        const float pen = (float)pow((double)(t + 1), (double)lp);
        float fsc[kBeamMax];
        int nf = 0, io = 0, jn = 0;
        while (nf < n) {
            while (jn < nc && jn < n && !hit[jn]) ++jn;
            const bool have_old = io < n && hdr->fin_flag[io], have_new = jn < nc && jn < n;
            if (!have_old && !have_new) break;
            const float so = have_old ? hdr->fin_score[io] : 0.f, sn = have_new ? cs[jn] / pen : 0.f;
            if (have_old && (!have_new || so >= sn)) { fsc[nf] = so; s_fsrc[nf] = io; s_flen[nf] = hdr->fin_len[io]; ++io; }
            else { fsc[nf] = sn; s_fsrc[nf] = -(jn + 1); s_flen[nf] = t + 1; ++jn; }
            ++nf;
        }
        const bool all_fin = nf == n;
        // the early-stop heuristic (sticky) and the stop rule
        int unsat = hdr->unsat;
        if (all_fin) {
            const int hyp = (early == 2 && lp > 0.f) ? limit : t + 1;
            const float best = nr > 0 ? rsc[0] / (float)pow((double)hyp, (double)lp) : -INFINITY;
            if (!(best > fsc[n - 1])) unsat = 0;
        }
        const bool go = unsat && !(all_fin && early == 1) && !all_hit && nr > 0 && nc > 0;
        for (int b = 0; b < n; ++b) {
            hdr->run_score[b] = rsc[b]; hdr->run_live[b] = s_live[b]; hdr->parent[b] = s_parent[b]; hdr->token[b] = s_token[b];
        }
        for (int i = 0; i < n; ++i) {
            hdr->fin_score[i] = i < nf ? fsc[i] : -INFINITY;
            hdr->fin_len[i] = i < nf ? s_flen[i] : 0;
            hdr->fin_flag[i] = i < nf ? 1 : 0;
            if (i >= nf) { s_fsrc[i] = 0x7fffffff; s_flen[i] = 0; }
        }
        hdr->unsat = unsat;
        hdr->ended = go ? 0 : 1;
        hdr->step = t + 1;
        s_ended = go ? 0 : 1;
        s_t = t;
    }
    __syncthreads();
    const int t = s_t, ob = t & 1, nb = ob ^ 1;
    const int32_t* rs_old = run_seq + (size_t)ob * n * max_new;
    int32_t* rs_new = run_seq + (size_t)nb * n * max_new;
    const int32_t* fs_old = fin_seq + (size_t)ob * n * max_new;
    int32_t* fs_new = fin_seq + (size_t)nb * n * max_new;
    for (int b = 0; b < n; ++b) {
        if (s_live[b]) {
            for (int i = threadIdx.x; i < t; i += blockDim.x) rs_new[b * max_new + i] = rs_old[s_parent[b] * max_new + i];
            if (threadIdx.x == 0) rs_new[b * max_new + t] = s_token[b];
        }
        const int src = s_fsrc[b];
        if (src == 0x7fffffff) continue;
        if (src >= 0) {
            for (int i = threadIdx.x; i < s_flen[b]; i += blockDim.x) fs_new[b * max_new + i] = fs_old[src * max_new + i];
        } else {
            const int j = -src - 1;
            for (int i = threadIdx.x; i < t; i += blockDim.x) fs_new[b * max_new + i] = rs_old[s_cb[j] * max_new + i];
            if (threadIdx.x == 0) fs_new[b * max_new + t] = s_ct[j];
        }
    }
    if (threadIdx.x < n) {
        const int b = threadIdx.x;
        int32_t* sb = st + b * w.words;
        gen_ids[(size_t)b * max_new + t] = s_token[b];
        sb[w.last] = s_token[b];
        sb[w.ngen] = t + 1;
        if (s_ended) sb[w.done] = 1;
    }
    if (s_ended) return;
    constexpr int V = Tr<T>::kVec;
    const int npack = hidden / V;
    for (int p = threadIdx.x; p < n * npack; p += blockDim.x) {
        const int b = p / npack, q = p % npack;
        st16(x + (int64_t)b * hidden + (int64_t)q * V, ld16(embed + (int64_t)s_token[b] * hidden + (int64_t)q * V));
    }
}

// parent[] of the step -> which slots are read (bit j of `need`) and whether anything moves at all
__device__ __forceinline__ bool beam_parents(const BeamHdr* hdr, int n, int (&par)[kBeamMax], unsigned& need) {
    need = 0u;
    bool moves = false;
#pragma unroll
    for (int b = 0; b < kBeamMax; ++b) {
        par[b] = b < n ? hdr->parent[b] : b;
        if (par[b] != b) { moves = true; need |= 1u << par[b]; }
    }
    return moves;
}

// `e[slot * slot_stride]` for every slot of the group: load what is read, then store what moves
template <typename P>
__device__ __forceinline__ void beam_permute_one(P* e, int64_t slot_stride, const int (&par)[kBeamMax], unsigned need) {
    P v[kBeamMax];
#pragma unroll
    for (int j = 0; j < kBeamMax; ++j)
        if ((need >> j) & 1u) v[j] = e[(int64_t)j * slot_stride];
#pragma unroll
    for (int b = 0; b < kBeamMax; ++b) {
        if (par[b] == b) continue;
        P val = v[0];
#pragma unroll
        for (int j = 1; j < kBeamMax; ++j)
            if (par[b] == j) val = v[j];
        e[(int64_t)b * slot_stride] = val;
    }
}

// K | V slab (blockIdx.z) x (layer, head) unit (blockIdx.y) x packet chunk (blockIdx.x) of the suffix rows [kv0, kv_len)
static __global__ __launch_bounds__(256) void beam_permute_kernel(uint4* kc, uint4* vc, int64_t slot_stride, int64_t unit_stride, int ppr,
                                                           const int32_t* st, BeamSt w, const BeamHdr* hdr) {
    if (st[w.done]) return;
    int par[kBeamMax];
    unsigned need;
    if (!beam_parents(hdr, hdr->n, par, need)) return;          // all identity: nothing is stored
    const int kv0 = hdr->kv0;
    const int64_t span = (int64_t)(st[w.kv_len] - kv0) * ppr;   // the rows the search has appended so far
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= span) return;
    uint4* e = (blockIdx.z ? vc : kc) + (int64_t)blockIdx.y * unit_stride + (int64_t)kv0 * ppr + i;
    beam_permute_one<uint4>(e, slot_stride, par, need);
}

// rules on: the history suffix [hist0, hist_len) and the rule-1 bitmap follow the parents the same way
static __global__ __launch_bounds__(256) void beam_hist_permute_kernel(int32_t* hist, int64_t hist_cap, uint32_t* bitmap, int bm_words,
                                                                const int32_t* hist_len0, const int32_t* st, BeamSt w,
                                                                const BeamHdr* hdr) {
    if (st[w.done]) return;
    int par[kBeamMax];
    unsigned need;
    if (!beam_parents(hdr, hdr->n, par, need)) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < bm_words) beam_permute_one<uint32_t>(bitmap + i, bm_words, par, need);
    const int h0 = hdr->hist0;
    int hl = *hist_len0;                        // (every slot of the group has the same history length)
    hl = hl > hist_cap ? (int)hist_cap : hl;
    if (i < hl - h0) beam_permute_one<int32_t>(hist + h0 + i, hist_cap, par, need);
}

}  // namespace ss
