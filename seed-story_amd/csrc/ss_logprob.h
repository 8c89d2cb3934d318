// Token log-probabilities of a logits row (definition: include/seedstory_hip.h, ss_token_logprobs).
//   stats    z_max over the entries that carry mass (NaN and -inf carry none, as in the sampler) and S = sum exp(z_i - z_max),
//            fp32.  The row is read from memory ONCE into registers (thread t owns the entries k * 1024 + t, k < 64), so the
//            maximum and the mass cost one pass; S is summed in one fixed order: per thread k ascending, xor butterfly over
//            the wave, xor butterfly over the 16 wave sums.  No atomics.  EPT = registers per thread, 32 up to 32768 entries
//            (logprob_ept_half_fits) and 64 beyond: the same sums in the same order either way.
//   value    lp(v) = (v - z_max) - log S: NaN for a NaN entry, -inf for a -inf entry, never a NaN made by the arithmetic
//            (a row without mass gives NaN / -inf by the entry alone).
//   top-n    n rounds of a block arg max over the registers, each below the previous (value, id) in the order "larger value,
//            then smaller id": descending, ties by ascending id, -1 / -inf once nothing with mass is left.
// Must be called by all 1024 threads of ONE block; vocab <= 65535.
#pragma once
#include "ss_common.h"
#include "ss_sample.h"

namespace ss {

#define SS_LOGPROB_MAX_TOP 8

constexpr int kLpEptFull = 64;  // entries per thread: 64 * 1024 >= 65535
inline bool logprob_ept_half_fits(int64_t vocab) { return vocab <= 32768; }

struct LogprobStats {
    float zmax, logz;
    int any;                    // 0: no entry of the row carries mass
};

__device__ __forceinline__ float logprob_value(float v, const LogprobStats& s) {
    if (!s.any) return v != v ? v : -INFINITY;
    return (v - s.zmax) - s.logz;
}

// LDS of logprob_row_block
struct LogprobSmem {
    uint32_t red[32];
    float av[16];
    int ai[16];
};

// The row into registers (entries past the vocabulary: -inf) and its stats (same value in every thread).
template <typename T, int EPT>
__device__ __forceinline__ LogprobStats logprob_load_block(const T* row, int vocab, float (&v)[EPT], LogprobSmem& sm, int& flip) {
    const int tid = threadIdx.x, nk = (vocab + 1023) >> 10;
    float m = -INFINITY;
#pragma unroll
    for (int k = 0; k < EPT; ++k) {
        const int i = k * 1024 + tid;
        v[k] = (k < nk && i < vocab) ? Tr<T>::ld(row + i) : -INFINITY;
        if (v[k] > m) m = v[k];         // (a NaN never compares greater)
    }
    m = sample_block_reduce<SRedMax>(m, sm.red, flip);
    LogprobStats s{m, 0.f, m > -INFINITY ? 1 : 0};
    if (!s.any) return s;               // (uniform branch)
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < EPT; ++k)
        if (k < nk) sum += v[k] > -INFINITY ? (v[k] == m ? 1.0f : expf(v[k] - m)) : 0.f;
    sum = sample_block_reduce<SRedSum>(sum, sm.red, flip);
    s.logz = logf(sum);
    return s;
}

// The top_n (<= SS_LOGPROB_MAX_TOP) largest entries of the registers with their values: thread 0 writes ids[0 .. top_n) and
// lps[0 .. top_n).
template <int EPT>
__device__ __forceinline__ void logprob_top_block(const float (&v)[EPT], int vocab, const LogprobStats& s, int top_n, int32_t* ids,
                                                  float* lps, LogprobSmem& sm) {
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, nk = (vocab + 1023) >> 10;
    ArgMax prev{INFINITY, -1};
    for (int j = 0; j < top_n; ++j) {
        ArgMax best{-INFINITY, 0x7fffffff};
#pragma unroll
        for (int k = 0; k < EPT; ++k) {
            const int i = k * 1024 + tid;
            // below the previous pick (ids ascend with k, so the first hit per value is the smallest id of this thread)
            const bool cand = k < nk && v[k] > -INFINITY && (v[k] < prev.v || (v[k] == prev.v && i > prev.i));
            if (cand && v[k] > best.v) { best.v = v[k]; best.i = i; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const ArgMax other{__shfl_xor(best.v, o, 64), __shfl_xor(best.i, o, 64)};
            best = argmax_better(best, other);
        }
        __syncthreads();
        if (lane == 0) { sm.av[wid] = best.v; sm.ai[wid] = best.i; }
        __syncthreads();
        ArgMax r{sm.av[0], sm.ai[0]};
        for (int w = 1; w < 16; ++w) r = argmax_better(r, ArgMax{sm.av[w], sm.ai[w]});
        const bool found = r.i != 0x7fffffff;
        if (tid == 0) {
            ids[j] = found ? r.i : -1;
            lps[j] = found ? logprob_value(r.v, s) : -INFINITY;
        }
        if (!found) r = ArgMax{-INFINITY, 0x7fffffff};     // nothing left: every later round finds nothing either
        prev = r;
    }
}

// One slot's result buffers in device memory (the engine's block is [n_seq] of these): caller-owned, entry n = gen_ids[n].
struct LogprobDesc {
    float* model_lp;            // [max_new]
    float* policy_lp;           // [max_new]
    int32_t* top_ids;           // [max_new][top_n]
    float* top_lp;              // [max_new][top_n]
    int32_t top_n;
    int32_t on;                 // 0 = this slot records nothing
};

// What the kernel in front of a decode token's edits leaves for the one behind the opening kernel (per slot).
struct LogprobScratch {
    float zmax, logz;           // stats of the raw row
    int32_t any;
    int32_t n;                  // the entry this token fills (ST_NGEN before the opening kernel)
    int32_t last;               // ST_LAST before the opening kernel: decides the certain image-token successor
    int32_t live;               // 0: the slot was done before this token and records nothing
    float samp_lp;              // the sampling kernel's log(w_tok / Z_P) of this token, from the draw's own kept set
    int32_t pad;
};

}  // namespace ss
