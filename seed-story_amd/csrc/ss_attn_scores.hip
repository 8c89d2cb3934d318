// Attention MAPS of one head, as the reference returns them under `output_attentions` (modeling_llama_xformer.py:246-276,
// 299-301): the PRE-softmax scores of head h, mask added, in the model dtype — the evidence behind the multimodal attention
// sink.  The flash kernels of ss_attn.hip never materialise these; this kernel exists only for callers who ask for them and
// is not on any default path.
//
// Arithmetic, all roundings in the model dtype T like the reference's torch graph:
//   s = rnd_T( rnd_T(q . k) / sqrt(hd) )                 (q, k post-RoPE; the dot product accumulates in fp32)
//   a call of several rows adds LlamaModel's additive causal mask: 0 where key j <= own(i), finfo(T).min elsewhere
//       -> s, or rnd_T(s + finfo(T).min)     (NOT a constant: in fp16 a score of 64 gives -65440, not -65504)
//   a call of ONE row has no additive mask; LlamaAttention adds its own BOOL mask, true on the row's own key only
//       -> s, and rnd_T(s + 1) on the own column.
// own(i) = kv - M + i: the key appended for query row i (bottom-right alignment).
//
// Tile: one workgroup = 64 keys x 32 query rows.  The K tile is staged once in LDS; lane c of every wave keeps key c's row in
// registers (fp32) and the four waves walk the tile's rows (wave w: rows w, w + 4, ...), reading q by LDS broadcast; a row's
// 64 scores leave as one contiguous run.  The cost is the store stream M x kv x sizeof(T); the FMAs are one head of 32.
#include <float.h>
#include <math.h>

#include "ss_common.h"

namespace ss {

template <typename T> struct MaskMin;   // torch.finfo(T).min as fp32
template <> struct MaskMin<float> { static constexpr float v = -FLT_MAX; };
template <> struct MaskMin<bf16_t> { static constexpr float v = -0x1.FEp127f; };
template <> struct MaskMin<f16_t> { static constexpr float v = -65504.0f; };

constexpr int SC_TN = 64;   // keys per workgroup (one per lane)
constexpr int SC_TM = 32;   // query rows per workgroup

template <typename T>
__device__ __forceinline__ float score_round(float acc, float div) { return Tr<T>::rnd(Tr<T>::rnd(acc) / div); }

// q [M, HD] (row stride ldq), k [kv, HD] (row stride ldk), out [M, ldo]; single != 0: every row is its own one-row call
// (columns beyond the row's own key are NOT written).  grid (ceil(kv / 64), ceil(M / 32)).
template <typename T, int HD>
__global__ __launch_bounds__(256) void attn_scores_kernel(const T* __restrict__ q, int64_t ldq, const T* __restrict__ k,
                                                          int64_t ldk, T* __restrict__ out, int64_t ldo, int M, int kv,
                                                          int single, float div) {
    constexpr int V = Tr<T>::kVec;
    constexpr int PPR = HD / V;        // 16-byte packs per row
    constexpr int KLD = HD + V;        // LDS row of the K tile, padded by one pack: lanes read whole rows without bank conflicts
    __shared__ __attribute__((aligned(16))) T sK[SC_TN * KLD];
    __shared__ __attribute__((aligned(16))) T sQ[SC_TM * HD];
    const int k0 = blockIdx.x * SC_TN, m0 = blockIdx.y * SC_TM, tid = threadIdx.x;
    const int m_end = min(m0 + SC_TM, M);
    if (single && k0 > kv - M + m_end - 1) return;      // the whole tile lies beyond its last row's own key
    for (int i = tid; i < SC_TN * PPR; i += 256) {
        const int r = i / PPR, p = i % PPR;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (k0 + r < kv) v = ld16(k + (int64_t)(k0 + r) * ldk + p * V);
        st16(sK + r * KLD + p * V, v);
    }
    for (int i = tid; i < SC_TM * PPR; i += 256) {
        const int r = i / PPR, p = i % PPR;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (m0 + r < M) v = ld16(q + (int64_t)(m0 + r) * ldq + p * V);
        st16(sQ + r * HD + p * V, v);
    }
    __syncthreads();
    const int lane = tid & 63, wave = tid >> 6;
    float kr[HD];
#pragma unroll
    for (int p = 0; p < PPR; ++p) unpack<T>(ld16(sK + lane * KLD + p * V), kr + p * V);
    const int j = k0 + lane;
    for (int lr = wave; lr < SC_TM; lr += 4) {
        const int i = m0 + lr;
        if (i >= M) break;
        float acc = 0.f;
#pragma unroll
        for (int p = 0; p < PPR; ++p) {
            float qf[V];
            unpack<T>(ld16(sQ + lr * HD + p * V), qf);
#pragma unroll
            for (int e = 0; e < V; ++e) acc = fmaf(qf[e], kr[p * V + e], acc);
        }
        if (j >= kv) continue;
        const int own = kv - M + i;
        float s = score_round<T>(acc, div);
        if (single) {
            if (j > own) continue;
            if (j == own) s = Tr<T>::rnd(s + 1.0f);
        } else if (j > own) {
            s = Tr<T>::rnd(s + MaskMin<T>::v);
        }
        Tr<T>::st(out + (int64_t)i * ldo + j, s);
    }
}

// Decode form: the one row of the token the fused RoPE + append + attention launch of this layer has just processed.  Runs inside
// the decode token (eager or captured), so everything that changes from token to token is read on the device: kv_len / pos / done
// from the slot's state words, the destination from the capture descriptor.  Raw q of head `desc->head` is rotated with the
// arithmetic of the fused kernel (rope_pack); key j's row comes straight from the cache plane (each is read once).
// Row index = (index of the key just appended) - row0; columns [0, kv_len], the last one carries the +1.  A finished slot, and
// any row / column outside the caller's buffer, writes nothing.  grid ceil(cache_cap / 256).
template <typename T>
__global__ __launch_bounds__(256) void attn_scores_decode_kernel(const T* __restrict__ qkv_raw, const T* __restrict__ kplane,
                                                                 const T* __restrict__ cos_t, const T* __restrict__ sin_t,
                                                                 const int32_t* __restrict__ kv_len_dev,
                                                                 const int32_t* __restrict__ pos_dev,
                                                                 const int32_t* __restrict__ done_flag,
                                                                 const AttnCaptureDesc* __restrict__ desc, int layer,
                                                                 int n_heads, int hd, int cap, float div) {
    constexpr int V = Tr<T>::kVec;
    __shared__ __attribute__((aligned(16))) T sq[128];
    if (*done_flag) return;
    const AttnCaptureDesc d = *desc;
    const int n_old = *kv_len_dev, kvn = n_old + 1;
    const int r = n_old - d.row0;
    if (!d.maps || r < 0 || r >= d.n_rows || kvn > d.ld || kvn > cap || (unsigned)d.head >= (unsigned)n_heads) return;
    const int tid = threadIdx.x, j = blockIdx.x * 256 + tid;
    if ((int)blockIdx.x * 256 >= kvn) return;
    if (tid < hd / V)
        st16(sq + tid * V, rope_pack<T>(qkv_raw + (int64_t)d.head * hd, cos_t, sin_t, *pos_dev, hd, tid * V));
    __syncthreads();
    if (j >= kvn) return;
    const T* krow = kplane + ((int64_t)d.head * cap + j) * hd;
    float acc = 0.f;
    for (int p = 0; p < hd / V; ++p) {
        float qf[V], kf[V];
        unpack<T>(ld16(sq + p * V), qf);
        unpack<T>(ld16(krow + p * V), kf);
#pragma unroll
        for (int e = 0; e < V; ++e) acc = fmaf(qf[e], kf[e], acc);
    }
    float s = score_round<T>(acc, div);
    if (j == n_old) s = Tr<T>::rnd(s + 1.0f);
    Tr<T>::st((T*)d.maps + ((int64_t)layer * d.n_rows + r) * d.ld + j, s);
}

static float score_div(int64_t hd) { return (float)sqrt((double)hd); }   // math.sqrt(head_dim), cast like torch casts the scalar

template <typename T>
static int attn_scores_launch(const void* q, int64_t ldq, const void* k, int64_t ldk, void* out, int64_t ldo, int64_t M,
                              int64_t kv, int64_t hd, int row_calls, hipStream_t s) {
    constexpr int V = Tr<T>::kVec;
    SS_REQUIRE(ldq % V == 0 && ldk % V == 0 && (uintptr_t)q % 16 == 0 && (uintptr_t)k % 16 == 0,
               "attn_scores: q / k rows must be 16-byte aligned");
    const dim3 grid((unsigned)cdiv(kv, SC_TN), (unsigned)cdiv(M, SC_TM));
    const int single = (row_calls || M == 1) ? 1 : 0;
    if (hd == 128)
        hipLaunchKernelGGL((attn_scores_kernel<T, 128>), grid, dim3(256), 0, s, (const T*)q, ldq, (const T*)k, ldk, (T*)out,
                           ldo, (int)M, (int)kv, single, score_div(hd));
    else
        hipLaunchKernelGGL((attn_scores_kernel<T, 64>), grid, dim3(256), 0, s, (const T*)q, ldq, (const T*)k, ldk, (T*)out,
                           ldo, (int)M, (int)kv, single, score_div(hd));
    SS_LAUNCH_CHECK("attn_scores");
    return SS_OK;
}

int attn_scores_dev(const void* q, int64_t ldq, const void* k, int64_t ldk, void* out, int64_t ldo, int64_t M, int64_t kv,
                    int64_t hd, int row_calls, int dtype, hipStream_t s) {
    SS_REQUIRE(q && k && out && M > 0 && kv >= M && kv < (1ll << 30), "attn_scores: bad arguments (M=%lld kv=%lld)",
               (long long)M, (long long)kv);
    SS_REQUIRE(hd == 128 || hd == 64, "attn_scores: head dim %lld unsupported (64, 128)", (long long)hd);
    SS_REQUIRE(ldq >= hd && ldk >= hd && ldo >= kv, "attn_scores: a row stride is shorter than its row");
    SS_REQUIRE(row_calls == 0 || row_calls == 1, "attn_scores: row_calls must be 0 or 1");
    return SS_DISPATCH(dtype, attn_scores_launch, q, ldq, k, ldk, out, ldo, M, kv, hd, row_calls, s);
}

template <typename T>
static int attn_scores_decode_launch(const void* qkv_raw, const void* kplane, const void* cos_t, const void* sin_t,
                                     const int32_t* kv_len_dev, const int32_t* pos_dev, const int32_t* done_flag,
                                     const AttnCaptureDesc* desc, int layer, int64_t n_heads, int64_t hd, int64_t cap,
                                     hipStream_t s) {
    hipLaunchKernelGGL(attn_scores_decode_kernel<T>, dim3((unsigned)cdiv(cap, 256)), dim3(256), 0, s, (const T*)qkv_raw,
                       (const T*)kplane, (const T*)cos_t, (const T*)sin_t, kv_len_dev, pos_dev, done_flag, desc, layer,
                       (int)n_heads, (int)hd, (int)cap, score_div(hd));
    SS_LAUNCH_CHECK("attn_scores_decode");
    return SS_OK;
}

int attn_scores_decode_dev(const void* qkv_raw, const void* kplane, const void* cos_t, const void* sin_t,
                           const int32_t* kv_len_dev, const int32_t* pos_dev, const int32_t* done_flag,
                           const AttnCaptureDesc* desc, int layer, int64_t n_heads, int64_t hd, int64_t cap, int dtype,
                           hipStream_t s) {
    SS_REQUIRE(hd == 128 || hd == 64, "attn_scores_decode: head dim %lld unsupported (64, 128)", (long long)hd);
    return SS_DISPATCH(dtype, attn_scores_decode_launch, qkv_raw, kplane, cos_t, sin_t, kv_len_dev, pos_dev, done_flag, desc,
                       layer, n_heads, hd, cap, s);
}

}  // namespace ss

extern "C" int ss_attn_scores(const void* q, int64_t ldq, const void* k, int64_t ldk, void* out, int64_t ldo, int64_t M,
                              int64_t kv, int64_t head_dim, int row_calls, int dtype, void* stream) {
    return ss::attn_scores_dev(q, ldq, k, ldk, out, ldo, M, kv, head_dim, row_calls, dtype, (hipStream_t)stream);
}
