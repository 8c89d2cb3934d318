// AutoImageTokenGenerationProcessor + greedy argmax as one device routine, and the sampler that takes the arg max's place
// when sampling is on (temperature -> top-k -> top-p -> one draw; definition below, at sample_block).
//   reference: src/models_clm/generation.py:19-31 (processor) and transformers==4.34.0 greedy
//   search as driven from src/models_clm/models.py:146-153.
// Literal semantics, in the model dtype like the reference (the processor edits the fp16/bf16
// logits in place):
//   last id in img_ids[:-1]  -> scores[successor] = round_T(max(scores) + 10)
//   otherwise                -> scores[img_ids[1:]] = 0.0      (assignment of zero, NOT -inf)
//   token = first index of the maximum.
// Must be called by all threads of ONE block (any multiple of 64 threads <= 1024; sample_block: exactly 1024).
#pragma once
#include "ss_common.h"

namespace ss {

struct ArgMax { float v; int i; };

__device__ __forceinline__ ArgMax argmax_better(ArgMax a, ArgMax b) {
    return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a;
}

// block-wide arg max over logits[0..vocab); smem: >= 2*16 words
template <typename T>
__device__ __forceinline__ ArgMax block_argmax(const T* logits, int vocab, float* sv, int* si) {
    ArgMax best{-INFINITY, 0x7fffffff};
    for (int i = threadIdx.x; i < vocab; i += blockDim.x) {
        const float v = Tr<T>::ld(logits + i);
        if (v > best.v) { best.v = v; best.i = i; }  // strict: keeps the first index per thread
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        ArgMax other{__shfl_xor(best.v, o, 64), __shfl_xor(best.i, o, 64)};
        best = argmax_better(best, other);
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    __syncthreads();
    if (lane == 0) { sv[wid] = best.v; si[wid] = best.i; }
    __syncthreads();
    ArgMax r{sv[0], si[0]};
    for (int w = 1; w < nw; ++w) r = argmax_better(r, ArgMax{sv[w], si[w]});
    return r;
}

// The processor's in-place edit of `logits`; returns the forced successor id or -1 (same value in every thread).
template <typename T>
__device__ __forceinline__ int imgproc_edit_block(T* logits, int vocab, int last_id, const int32_t* img_ids, int n_img_ids,
                                                  float* sv, int* si) {
    __shared__ int s_succ;
    if (threadIdx.x == 0) {
        int succ = -1;
        for (int j = 0; j + 1 < n_img_ids; ++j)
            if (img_ids[j] == last_id) { succ = img_ids[j + 1]; break; }  // list.index: first match
        s_succ = succ;
    }
    __syncthreads();
    const int succ = s_succ;
    if (succ >= 0) {
        const ArgMax mx = block_argmax<T>(logits, vocab, sv, si);
        if (threadIdx.x == 0) Tr<T>::st(logits + succ, mx.v + 10.0f);
    } else {
        for (int j = 1 + threadIdx.x; j < n_img_ids; j += blockDim.x) Tr<T>::st(logits + img_ids[j], 0.0f);
    }
    __threadfence_block();
    __syncthreads();
    return succ;
}

// Returns the greedy token (same value in every thread).  Edits `logits` in place.
template <typename T>
__device__ __forceinline__ int imgproc_argmax_block(T* logits, int vocab, int last_id, const int32_t* img_ids,
                                                    int n_img_ids, float* sv, int* si) {
    imgproc_edit_block<T>(logits, vocab, last_id, img_ids, n_img_ids, sv, si);
    return block_argmax<T>(logits, vocab, sv, si).i;
}

// ---- sampling -----------------------------------------------------------------------------------------------------------
// Definition (include/seedstory_hip.h, ss_sample_logits).  z = the row after the processor's edit, in the model dtype.
//   top-k   (top_k > 0): keep i iff z_i >= the k-th largest z (ties all kept): integer work on monotone keys of the bit patterns
//   weights w_i = exp((z_i - z_max) / temperature) over that set, fp32; Z_k = sum w
//   top-p   (top_p < 1): keep i iff A_i < top_p * Z_k, A_i = the mass strictly above z_i (the arg max is always kept)
//   draw    t = u * Z_P over the kept set; token = the first kept index, ascending, whose inclusive cumulative weight
//           exceeds t; fallback: the last kept index
// NaN and -inf entries are never kept; a row without any other entry gives token 0 and n_kept 0.  Both thresholds are the
// largest key th with  count(key >= th) >= k  /  mass(key >= th) >= top_p * Z_k, found bit by bit from the top; every mass
// is summed in one fixed order (per thread in element order, xor butterfly over the wave, xor butterfly over the 16 wave
// sums), so a row gives the same token on every run.  No atomics.

// One slot's parameters in device memory (the engine's block is [n_seq] of these; 32 bytes).
struct SampleParams {
    float inv_temp, top_p;
    int32_t top_k;
    uint32_t seed_lo, seed_hi;
    uint32_t draw;          // draws taken so far: the Philox counter word 0 of the next one
    int32_t enabled;        // 0 = this slot takes the arg max
    int32_t pad;
};

// ss_sampling -> the device block (enabled, draw 0); SS_EINVAL with a message for a parameter outside its range
inline int sampling_params(const ss_sampling* p, const char* who, SampleParams* out) {
    SS_REQUIRE(p->temperature > 0.f && p->temperature <= 3.4028234e38f, "%s: temperature %g must be finite and > 0", who,
               (double)p->temperature);
    SS_REQUIRE(p->top_p > 0.f && p->top_p <= 1.0f, "%s: top_p %g outside (0, 1]", who, (double)p->top_p);
    SS_REQUIRE(p->top_k >= 0, "%s: top_k %d < 0", who, (int)p->top_k);
    out->inv_temp = 1.0f / p->temperature;
    out->top_p = p->top_p;
    out->top_k = p->top_k;
    out->seed_lo = (uint32_t)(p->seed & 0xFFFFFFFFull);
    out->seed_hi = (uint32_t)(p->seed >> 32);
    out->draw = 0;
    out->enabled = 1;
    out->pad = 0;
    return SS_OK;
}

// Philox4x32-10 (Salmon et al., SC'11), counter (c0, c1, 0, 0), key (k0, k1); returns output word 0
__device__ __forceinline__ uint32_t philox4x32_10_word0(uint32_t c0, uint32_t c1, uint32_t k0, uint32_t k1) {
    uint32_t c2 = 0, c3 = 0;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return c0;
}
// The same generator with a full counter (c0, c1, c2, c3), all four output words (the diffusion noise: ss_diffusion.hip)
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t out[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
__device__ __forceinline__ float philox_uniform(uint32_t seed_lo, uint32_t seed_hi, uint32_t draw, uint32_t lane) {
    return (float)(philox4x32_10_word0(draw, lane, seed_lo, seed_hi) >> 8) * 5.9604644775390625e-8f;   // 2^-24: [0, 1)
}

// bit patterns of T <-> monotone unsigned keys.  NaN and -inf -> key 0 (never kept), -0 -> the key of +0.
template <typename T> struct SKey;
template <> struct SKey<float> {
    static constexpr int kBits = 32;
    static constexpr uint32_t kSign = 0x80000000u, kMask = 0xFFFFFFFFu, kNegInf = 0xFF800000u;
    static __device__ __forceinline__ float f32(uint32_t raw) { return __uint_as_float(raw); }
    static __device__ __forceinline__ uint32_t ld(const float* p) { return __float_as_uint(*p); }
};
template <> struct SKey<bf16_t> {
    static constexpr int kBits = 16;
    static constexpr uint32_t kSign = 0x8000u, kMask = 0xFFFFu, kNegInf = 0xFF80u;
    static __device__ __forceinline__ float f32(uint32_t raw) { return bf16_bits_to_f32(raw); }
    static __device__ __forceinline__ uint32_t ld(const bf16_t* p) { return p->v; }
};
template <> struct SKey<f16_t> {
    static constexpr int kBits = 16;
    static constexpr uint32_t kSign = 0x8000u, kMask = 0xFFFFu, kNegInf = 0xFC00u;
    static __device__ __forceinline__ float f32(uint32_t raw) { return f16_bits_to_f32(raw); }
    static __device__ __forceinline__ uint32_t ld(const f16_t* p) { return p->v; }
};
template <typename T>
__device__ __forceinline__ uint32_t skey_of_raw(uint32_t raw) {
    const float v = SKey<T>::f32(raw);
    if (!(v > -INFINITY)) return 0u;
    if (v == 0.f) raw = 0u;
    return (raw & SKey<T>::kSign) ? (~raw & SKey<T>::kMask) : (raw | SKey<T>::kSign);
}
template <typename T>
__device__ __forceinline__ float skey_value(uint32_t key) {
    return SKey<T>::f32((key & SKey<T>::kSign) ? (key & ~SKey<T>::kSign) : (~key & SKey<T>::kMask));
}

// block reductions of sample_block: 1024 threads = 16 waves; xor butterflies, so every lane of every wave holds the same
// bits.  `red` is 2 x 16 words used alternately (`flip`): one barrier per reduction.
struct SRedSum { template <typename V> static __device__ __forceinline__ V op(V a, V b) { return a + b; } };
struct SRedMax { template <typename V> static __device__ __forceinline__ V op(V a, V b) { return a > b ? a : b; } };
struct SRedMin { template <typename V> static __device__ __forceinline__ V op(V a, V b) { return a < b ? a : b; } };
template <typename Op, typename V>
__device__ __forceinline__ V sample_block_reduce(V v, uint32_t* red, int& flip) {
    static_assert(sizeof(V) == 4, "one word");
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = Op::op(v, __shfl_xor(v, o, 64));
    uint32_t* r = red + 16 * flip;
    flip ^= 1;
    if ((threadIdx.x & 63) == 0) r[threadIdx.x >> 6] = __builtin_bit_cast(uint32_t, v);
    __syncthreads();
    v = __builtin_bit_cast(V, r[threadIdx.x & 15]);
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v = Op::op(v, __shfl_xor(v, o, 64));
    return v;
}

// LDS of sample_block
struct SampleSmem {
    uint32_t red[32];
    float tot[256];         // scan: sum of every (step, wave), step-major = index order
    float base[256];        // its exclusive prefix
    float total;
    float lp_arg;           // LP: (z_tok - z_max) / temperature of the scored token, -inf when it is not kept
};

// One row, 1024 threads, vocab <= 65535.  NS = 16-byte steps per thread: NS * 1024 * kVec >= vocab + kVec - 1.  The row is
// held in registers: thread t owns the runs (s * 1024 + t), s < NS, of kVec consecutive elements, so (step, thread, element)
// is index order; the runs are the 16-byte aligned ones of the row's memory (first and last partial), or, where shifting by
// the misalignment would not fit, element loads.  Returns the token (same value in every thread); *n_kept_out likewise.
// LP (token log-probabilities, ss_logprob.h): *lp_out = log(w_t / Z_P) of t = `want`, or of the drawn token when want < 0,
// as (z_t - z_max) / temperature - log Z_P with the kept set and the Z_P (sm.total) of this very draw; -inf when t is not kept.
template <typename T, int NS, bool LP = false>
__device__ __forceinline__ int sample_block(const T* row, int vocab, float inv_temp, float top_p, int top_k, float u,
                                            SampleSmem& sm, int* n_kept_out, int want = -1, float* lp_out = nullptr) {
    constexpr int V = Tr<T>::kVec, NE = NS * V, KB = SKey<T>::kBits, PW = 32 / KB, NW = NE / PW;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    int flip = 0;
    int off = (int)(((uintptr_t)row & 15) / sizeof(T));
    bool vec_ok = true;
    if (vocab + off > NS * 1024 * V) { off = 0; vec_ok = false; }
    uint32_t kk[NW];        // keys, PW per word
    auto key_at = [&](int e) -> uint32_t { return PW == 1 ? kk[e] : ((kk[e / PW] >> ((e % PW) * KB)) & SKey<T>::kMask); };
    // (keeps the compiler from hoisting the unpacked keys out of the threshold loops: twice the registers, spilled)
    auto pin_keys = [&]() {
#pragma unroll
        for (int w = 0; w < NW; ++w) asm volatile("" : "+v"(kk[w]));
    };
#pragma unroll
    for (int w = 0; w < NW; ++w) kk[w] = 0u;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int i0 = (s * 1024 + tid) * V - off;
        uint32_t raw[V];
        if (vec_ok && i0 >= 0 && i0 + V <= vocab) {
            const uint4 q = ld16(row + i0);
            const uint32_t c[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int j = 0; j < V; ++j) raw[j] = PW == 1 ? c[j] : ((c[j / PW] >> ((j % PW) * KB)) & SKey<T>::kMask);
        } else {
#pragma unroll
            for (int j = 0; j < V; ++j) raw[j] = (i0 + j >= 0 && i0 + j < vocab) ? SKey<T>::ld(row + i0 + j) : SKey<T>::kNegInf;
        }
#pragma unroll
        for (int j = 0; j < V; ++j) kk[(s * V + j) / PW] |= skey_of_raw<T>(raw[j]) << (((s * V + j) % PW) * KB);
    }
    uint32_t kmax = 0u;
#pragma unroll
    for (int e = 0; e < NE; ++e) kmax = max(kmax, key_at(e));
    kmax = sample_block_reduce<SRedMax>(kmax, sm.red, flip);
    if (kmax == 0u) {       // nothing but NaN / -inf (uniform branch)
        *n_kept_out = 0;
        if constexpr (LP) *lp_out = -INFINITY;
        return 0;
    }
    const float zmax = skey_value<T>(kmax);

    // top-k: th = the largest key with count(key >= th) >= k
    uint32_t th = 1u;
    if (top_k > 0 && top_k < vocab) {
        uint32_t t = 0u;
        for (int b = KB - 1; b >= 0; --b) {
            const uint32_t cand = t | (1u << b);
            pin_keys();
            int c = 0;
#pragma unroll
            for (int e = 0; e < NE; ++e) c += key_at(e) >= cand ? 1 : 0;
            if (sample_block_reduce<SRedSum>(c, sm.red, flip) >= top_k) t = cand;
        }
        th = max(t, 1u);
    }
    float w[NE];
    float zk = 0.f;
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        const uint32_t k = key_at(e);
        w[e] = k >= th ? (k == kmax ? 1.0f : expf((skey_value<T>(k) - zmax) * inv_temp)) : 0.f;
        zk += w[e];
    }
    if (top_p < 1.0f) {     // th = the largest key with mass(key >= th) >= top_p * Z_k (never above kmax: Z_k >= 1)
        zk = sample_block_reduce<SRedSum>(zk, sm.red, flip);
        const float P = top_p * zk;
        uint32_t t = 0u;
        for (int b = KB - 1; b >= 0; --b) {
            const uint32_t cand = t | (1u << b);
            pin_keys();
            float m = 0.f;
#pragma unroll
            for (int e = 0; e < NE; ++e) m += key_at(e) >= cand ? w[e] : 0.f;
            if (sample_block_reduce<SRedSum>(m, sm.red, flip) >= P) t = cand;
        }
        th = max(th, t);
    }
    // the kept set: count, last index, and the index-ordered scan of its weights
    int cnt = 0, last = -1;
    float ps[NS], inc[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        float a = 0.f;
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const int e = s * V + j;
            const bool kept = key_at(e) >= th;
            if (!kept) w[e] = 0.f;
            if (kept) { ++cnt; last = (s * 1024 + tid) * V + j - off; }
            a += w[e];
        }
        ps[s] = a;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const float up = __shfl_up(a, o, 64);
            if (lane >= o) a += up;
        }
        inc[s] = a;
        if (lane == 63) sm.tot[s * 16 + wid] = a;
    }
    cnt = sample_block_reduce<SRedSum>(cnt, sm.red, flip);      // (its barrier also publishes sm.tot)
    last = sample_block_reduce<SRedMax>(last, sm.red, flip);
    if (wid == 0) {         // exclusive prefix of the NS * 16 sums: NS / 4 consecutive ones per lane
        constexpr int E = NS / 4;
        float a[E], run = 0.f;
#pragma unroll
        for (int i = 0; i < E; ++i) { a[i] = sm.tot[lane * E + i]; run += a[i]; }
        float x = run;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const float up = __shfl_up(x, o, 64);
            if (lane >= o) x += up;
        }
        float ex = __shfl_up(x, 1, 64);
        if (lane == 0) ex = 0.f;
#pragma unroll
        for (int i = 0; i < E; ++i) { sm.base[lane * E + i] = ex; ex += a[i]; }
        if (lane == 63) sm.total = x;
    }
    __syncthreads();
    const float t = u * sm.total;
    int pick = 0x7fffffff;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        float ex = __shfl_up(inc[s], 1, 64);
        if (lane == 0) ex = 0.f;
        float cum = sm.base[s * 16 + wid] + ex;
        if (cum + ps[s] > t && pick == 0x7fffffff) {    // (a miss by the last rounding falls through to a later element)
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const int e = s * V + j;
                cum += w[e];
                if (key_at(e) >= th && cum > t && pick == 0x7fffffff) pick = (s * 1024 + tid) * V + j - off;
            }
        }
    }
    pick = sample_block_reduce<SRedMin>(pick, sm.red, flip);
    *n_kept_out = cnt;
    const int res = pick != 0x7fffffff ? pick : last;
    if constexpr (LP) {     // the owner of the scored entry publishes its exponent; an id outside the row is not kept
        const int tgt = want >= 0 ? want : res;
        if (tid == 0) sm.lp_arg = -INFINITY;
        __syncthreads();
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const uint32_t k = key_at(e);
            if (((e / V) * 1024 + tid) * V + (e % V) - off == tgt && k >= th)
                sm.lp_arg = k == kmax ? 0.f : (skey_value<T>(k) - zmax) * inv_temp;
        }
        __syncthreads();
        *lp_out = sm.lp_arg - logf(sm.total);
    }
    return res;
}

// NS of sample_block for a vocabulary: half the registers (and unrolled work) up to 32K entries
template <typename T> constexpr int sample_ns_full() { return 65536 / (1024 * Tr<T>::kVec); }
inline bool sample_ns_half_fits(int64_t vocab) { return vocab + 8 <= 32768; }

// processor edit -> certain successor | sample.  Returns the token; *drew = 1 iff a draw was consumed (LP: *lp_out is set then).
template <typename T, int NS, bool LP = false>
__device__ __forceinline__ int imgproc_sample_block(T* logits, int vocab, bool has_last, int last_id, const int32_t* img_ids,
                                                    int n_img_ids, float inv_temp, float top_p, int top_k, float u,
                                                    float* sv, int* si, SampleSmem& sm, int* n_kept_out, int* drew,
                                                    float* lp_out = nullptr) {
    const int succ = has_last ? imgproc_edit_block<T>(logits, vocab, last_id, img_ids, n_img_ids, sv, si) : -1;
    *drew = 0;
    if (succ >= 0 && succ < vocab) { *n_kept_out = 1; return succ; }
    *drew = 1;
    return sample_block<T, NS, LP>(logits, vocab, inv_temp, top_p, top_k, u, sm, n_kept_out, -1, lp_out);
}

}  // namespace ss
