// Decode projection  y[b][N] = W[N,K] · x[b][K], b < NB <= 4  — the HBM-bound hot kernel of the MLLM
// decode loop (13.22 GB of bf16 weights per generated token).
//
// Design (MI355X): wave-autonomous weight streaming.
//   * every wave keeps its slice of x in registers for the whole launch (x is 8-22 KB and
//     L2/L1 resident; lane l owns elements {it*64*V + l*V .. +V} for it < NIT), so the
//     inner loop is nothing but 16-byte non-temporal weight loads + v_dot2c_f32_bf16:
//     no LDS, no barriers, no cross-wave traffic;
//   * a wave owns ROWS consecutive output rows per trip and issues all their loads
//     (ROWS x min(NIT,8) x 16 B per lane) before the first use, so ≥8-16 KB per wave are
//     in flight; rows are dealt to waves round-robin so the chip sweeps W sequentially;
//   * optional fused prologue: RMSNorm of x (each wave recomputes the 4096-element
//     statistic redundantly from its registers: cheaper than a kernel boundary);
//   * epilogues: +bias, +residual (in T, like `residual + hidden`, :352,:359),
//     SiLU(gate)·up for the fused [gate; up] projection (LlamaMLP.forward, :190-191).
// Weight-only quantised variants (opt-in decode_weights of the LLaMA engine): ss_gemv_w8 over fp8 (OCP e4m3fn) byte planes + one fp32
// scale per row, ss_gemv_mx4 over MXFP4 planes (e2m1 codes, two per byte, + one e8m0 scale byte per 32 k).  Both run the MFMA family
// below: ONE predicated tile loop serves 16-bit, fp8 and MXFP4 weights through a small policy type per format (how a 16-byte load
// slot is addressed, loaded and decoded into the 16-bit MFMA operand — "the weight formats of the MFMA forms"); the stream loops
// of the LLaMA-7B depths are one kernel per format.
// Reference call sites: modeling_llama_xformer.py:228-230 (q/k/v), :297 (o), :191 (MLP),
// :759 (lm_head); LlamaRMSNorm :107-115 for the prologue.
#include "ss_gemv.h"

#include <string.h>
#include <algorithm>
#include <type_traits>
#include <utility>

namespace ss {

struct GemvArgs {
    const void* W;
    const void* x;         // [nb][x_ld]
    void* y;               // [nb][y_ld]
    const void* norm_w;
    const void* bias;
    const void* residual;  // [nb][res_ld]
    const int32_t* done_flag;  // optional device flags (one per sequence, done_stride ints apart):
                               // the launch is skipped when every sequence's flag is set
    int N, K, epi;
    float eps;
    int use_nt;
    int nb, done_stride;
    int64_t x_ld, y_ld, res_ld;
};

__device__ __forceinline__ float silu_g(float g) { return g / (1.0f + expf(-g)); }

__device__ __forceinline__ bool gemv_all_done(const GemvArgs& a) {
    if (!a.done_flag) return false;
    for (int b = 0; b < a.nb; ++b)
        if (!a.done_flag[(int64_t)b * a.done_stride]) return false;
    return true;
}

// ---- the one output epilogue -----------------------------------------------------------------------------------------------------
// y = round(acc + bias) + residual (in T, like `residual + hidden`), or for the fused [gate; up] projection
// y = round(round(silu(round gate)) * round up) (the store rounds once more).  bias / res are callables: an absent operand is
// never read.  Tr<float>::rnd is the identity, so the fp32 forms share the text.
template <typename T>
__device__ __forceinline__ float gv_silu_pair(float g, float u) { return Tr<T>::rnd(silu_g(Tr<T>::rnd(g))) * Tr<T>::rnd(u); }
template <typename T, typename FB, typename FR>
__device__ __forceinline__ float gv_epilogue(float acc, FB&& bias, FR&& res, int epi) {
    if (epi & SS_EPI_BIAS) acc += bias();
    acc = Tr<T>::rnd(acc);
    if (epi & SS_EPI_RESIDUAL) acc += res();
    return acc;
}
// rows row0 .. row0 + 3 of sequence seq: ONE 8- / 16-byte store when the four rows exist and row stride, row0 and the base of y
// are aligned to it (an `out=` view at an odd element offset takes the scalar stores)
template <typename T>
__device__ __forceinline__ void gv_store4(const GemvArgs& a, int seq, int row0, const float (&o)[4]) {
    using V4 = std::conditional_t<sizeof(T) == 4, uint4, uint2>;
    T* y = (T*)a.y + (int64_t)seq * a.y_ld;
    if (row0 + 3 < a.N && ((a.y_ld | row0) & 3) == 0 && ((size_t)a.y & (sizeof(V4) - 1)) == 0) {
        alignas(16) T tmp[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) Tr<T>::st(tmp + r, o[r]);
        *reinterpret_cast<V4*>(y + row0) = *reinterpret_cast<const V4*>(tmp);
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (row0 + r < a.N) Tr<T>::st(y + row0 + r, o[r]);
    }
}

// ---- the one RMSNorm prologue (LlamaRMSNorm: gw * round(x * rstd), statistic in fp32), per 16-byte pack ----------------------------
template <typename T>
__device__ __forceinline__ float gv_pack_ssq(const uint4& x, float ssq) {
    constexpr int V = Tr<T>::kVec;
    float f[V];
    unpack<T>(x, f);
#pragma unroll
    for (int j = 0; j < V; ++j) ssq = fmaf(f[j], f[j], ssq);
    return ssq;
}
__device__ __forceinline__ float gv_rstd(float ssq, int K, float eps) { return 1.0f / sqrtf(ssq / (float)K + eps); }
template <typename T>
__device__ __forceinline__ uint4 gv_pack_norm(const uint4& x, const uint4& gain, float rstd) {
    constexpr int V = Tr<T>::kVec;
    float f[V], gw[V];
    unpack<T>(x, f);
    unpack<T>(gain, gw);
#pragma unroll
    for (int j = 0; j < V; ++j) f[j] = gw[j] * Tr<T>::rnd(f[j] * rstd);
    return pack<T>(f);
}

// ---- row groups of the dot-product kernels: what a wave owns per trip ---------------------------------------------------------------
// silu -> N groups, each the pair (n, n + N) of W;  else ROWS consecutive rows.
template <int ROWS>
struct GvRowGroups {
    int N; bool silu;
    __device__ __forceinline__ int count() const { return silu ? N : (N + ROWS - 1) / ROWS; }
    __device__ __forceinline__ int64_t row(int g, int r) const { return silu ? (int64_t)g + (int64_t)r * N : (int64_t)g * ROWS + r; }
    __device__ __forceinline__ bool valid(int64_t row) const { return silu || row < N; }
};
// a pack of weights (row / pack out of range: zeros)
template <typename T>
__device__ __forceinline__ uint4 gv_load_w(const T* p, bool ok, int nt) {
    if (!ok) return make_uint4(0, 0, 0, 0);
    return nt ? ld_nt16(p) : ld16(p);
}
// lane sums of a finished group -> wave sums -> epilogue and store by lane 0
template <typename T, int ROWS, int NB>
__device__ __forceinline__ void gv_reduce_store(const GemvArgs& a, const GvRowGroups<ROWS>& rg, int g, float (&acc)[NB][ROWS], int lane) {
#pragma unroll
    for (int b = 0; b < NB; ++b) {
#pragma unroll
        for (int r = 0; r < ROWS; ++r) acc[b][r] = wave_sum(acc[b][r]);
        if (lane != 0) continue;
        T* y = (T*)a.y + (int64_t)b * a.y_ld;
        if (rg.silu) {
            Tr<T>::st(y + g, gv_silu_pair<T>(acc[b][0], acc[b][ROWS > 1 ? 1 : 0]));
        } else {
#pragma unroll
            for (int r = 0; r < ROWS; ++r) {
                const int64_t row = rg.row(g, r);
                if (row >= a.N) continue;
                Tr<T>::st(y + row, gv_epilogue<T>(acc[b][r], [&] { return Tr<T>::ld((const T*)a.bias + row); },
                                                  [&] { return Tr<T>::ld((const T*)a.residual + (int64_t)b * a.res_ld + row); }, a.epi));
            }
        }
    }
}

// LDS staging of gemv_ldsx_kernel (kernel and launch plan): nb rows of K / V packs, padded to whole chunks of 8 x 64 packs
struct GvLdsxStage {
    int npack, nchunk, npack_pad;
    __host__ __device__ GvLdsxStage(int K, int V) : npack(K / V), nchunk((npack + 511) / 512), npack_pad(nchunk * 512) {}
    __host__ __device__ size_t bytes(int nb) const { return (size_t)nb * npack_pad * 16; }
};
// NB = sequences sharing one sweep of W (the decode batch: every weight pack is dotted with NB
// resident x slices, so the HBM traffic per generated token falls as 1/NB).
template <typename T, int NIT, int ROWS, int NB>
__global__ __launch_bounds__(256) void gemv_kernel(const GemvArgs a) {
    constexpr int V = Tr<T>::kVec;
    if (gemv_all_done(a)) return;
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int nwaves = gridDim.x * (blockDim.x >> 6);
    const T* __restrict__ W = (const T*)a.W;
    const int K = a.K, N = a.N;
    const bool silu = (a.epi & SS_EPI_SILU_MUL) != 0;
    const GvRowGroups<ROWS> rg{N, silu};
    auto load_group = [&](int g, uint4 (&wv)[ROWS][NIT]) {
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            const int64_t row = rg.row(g, r);
            const bool ok = rg.valid(row);
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                const int k = (it * 64 + lane) * V;
                wv[r][it] = gv_load_w<T>(W + row * K + k, ok && k < K, a.use_nt);
            }
        }
    };

    // ---- x slices into registers (+ fused RMSNorm) -----------------------------------------
    // The RMS statistic is recomputed by every wave from its registers (cheap, and no cross-wave
    // traffic), but the element-wise normalise/round/scale (~6 VALU ops per element in bf16) is shared:
    // each of the block's 4 waves normalises a quarter of the row into LDS and all read it back.
    constexpr bool COOP = (NIT % 4 == 0);
    constexpr int NQ = COOP ? NIT / 4 : 1;
    __shared__ uint4 xn_s[COOP ? NB * NIT * 64 : 1];
    uint4 xr[NB][NIT];
    uint4 xq[NB][NQ], gq[NQ];
    const int wid = threadIdx.x >> 6;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const T* xb = (const T*)a.x + (int64_t)b * a.x_ld;
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int k = (it * 64 + lane) * V;
            xr[b][it] = (k < K) ? ld16(xb + k) : make_uint4(0, 0, 0, 0);
        }
        if (COOP && a.norm_w) {
#pragma unroll
            for (int j4 = 0; j4 < NQ; ++j4) {
                const int k = ((wid * NQ + j4) * 64 + lane) * V;
                xq[b][j4] = (k < K) ? ld16(xb + k) : make_uint4(0, 0, 0, 0);
            }
        }
    }
    if (a.norm_w) {
        if constexpr (COOP) {
#pragma unroll
            for (int j4 = 0; j4 < NQ; ++j4) {
                const int k = ((wid * NQ + j4) * 64 + lane) * V;
                gq[j4] = (k < K) ? ld16((const T*)a.norm_w + k) : make_uint4(0, 0, 0, 0);
            }
        }
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            float ssq = 0.f;
#pragma unroll
            for (int it = 0; it < NIT; ++it) ssq = gv_pack_ssq<T>(xr[b][it], ssq);
            const float rstd = gv_rstd(wave_sum(ssq), K, a.eps);
            if constexpr (COOP) {
#pragma unroll
                for (int j4 = 0; j4 < NQ; ++j4)      // k >= K packs are zeros already
                    xn_s[(b * NIT + wid * NQ + j4) * 64 + lane] = gv_pack_norm<T>(xq[b][j4], gq[j4], rstd);
            } else {
#pragma unroll
                for (int it = 0; it < NIT; ++it) {
                    const int k = (it * 64 + lane) * V;
                    if (k < K) xr[b][it] = gv_pack_norm<T>(xr[b][it], ld16((const T*)a.norm_w + k), rstd);
                }
            }
        }
        if constexpr (COOP) {
            __syncthreads();
#pragma unroll
            for (int b = 0; b < NB; ++b)
#pragma unroll
                for (int it = 0; it < NIT; ++it) xr[b][it] = xn_s[(b * NIT + it) * 64 + lane];
        }
    }

    // ---- stream the rows: plain load -> dot -> reduce per group (125 VGPRs at NB=1, 4 waves/SIMD;
    // measured faster on MI355X than software-pipelined forms that cost 177-198 VGPRs) ------------
    // (requesting the first group's weights before the prologue was measured: the 64 extra live VGPRs
    // cost two waves/SIMD of occupancy and more than the overlap gains)
    uint4 wv[ROWS][NIT];
    for (int g = wave; g < rg.count(); g += nwaves) {
        load_group(g, wv);
        float acc[NB][ROWS];
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int r = 0; r < ROWS; ++r) acc[b][r] = 0.f;
#pragma unroll
        for (int it = 0; it < NIT; ++it)
#pragma unroll
            for (int r = 0; r < ROWS; ++r)
#pragma unroll
                for (int b = 0; b < NB; ++b) acc[b][r] = dot_pack<T>(wv[r][it], xr[b][it], acc[b][r]);
        gv_reduce_store<T, ROWS, NB>(a, rg, g, acc, lane);
    }
}

// Long-K / wide-batch variant (K > 64*V*8, e.g. the 11008-wide down projection, or NB x slices that
// do not fit the register file): x (optionally RMS-normalised) is staged once per block in LDS and
// read back with conflict-free ds_read_b128 (lanes read consecutive 16-byte slots); the k loop runs
// in chunks of 8 x 64 packs with ROWS x 8 weight loads in flight.
template <typename T, int ROWS, int NB>
__global__ __launch_bounds__(1024) void gemv_ldsx_kernel(const GemvArgs a) {
    constexpr int V = Tr<T>::kVec;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    uint4* xs = reinterpret_cast<uint4*>(smem_raw);  // [NB][npack_pad]
    if (gemv_all_done(a)) return;
    const int lane = threadIdx.x & 63;
    const int wpb = blockDim.x >> 6;
    const int wave = blockIdx.x * wpb + (threadIdx.x >> 6);
    const int nwaves = gridDim.x * wpb;
    const T* __restrict__ W = (const T*)a.W;
    const int K = a.K, N = a.N;
    const bool silu = (a.epi & SS_EPI_SILU_MUL) != 0;
    const GvLdsxStage st(K, V);
    const int npack = st.npack, nchunk = st.nchunk, npack_pad = st.npack_pad;
    const GvRowGroups<ROWS> rg{N, silu};
    auto load_tile = [&](int g, int c, uint4 (&wv)[ROWS][8]) {
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            const int64_t row = rg.row(g, r);
            const bool ok = rg.valid(row);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int p = (c * 8 + i) * 64 + lane;
                wv[r][i] = gv_load_w<T>(W + row * K + (int64_t)p * V, ok && p < npack, a.use_nt);
            }
        }
    };

    // ---- stage the NB activation rows in LDS: ONE global read of x per block ------------------------------------
    // (every block needs all of x; at NB = 4 the old per-wave statistic + second read pulled more bytes of x through
    // L2 than the launch streams weights from HBM)
    float ssq[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) ssq[b] = 0.f;
#pragma unroll 2
    for (int p = threadIdx.x; p < npack_pad; p += blockDim.x) {
        const bool ok = p < npack;
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const uint4 v = ok ? ld16((const T*)a.x + (int64_t)b * a.x_ld + (int64_t)p * V) : make_uint4(0, 0, 0, 0);
            if (a.norm_w) ssq[b] = gv_pack_ssq<T>(v, ssq[b]);
            xs[(size_t)b * npack_pad + p] = v;
        }
    }
    if (a.norm_w) {
        // fused RMSNorm: block-wide statistic in a fixed order (lane tree, then waves 0..n-1), then each thread
        // normalises its own packs in place
        __shared__ float red[NB][16];
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const float w = wave_sum(ssq[b]);
            if (lane == 0) red[b][threadIdx.x >> 6] = w;
        }
        __syncthreads();
        float rstd[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            float t = 0.f;
            for (int w = 0; w < wpb; ++w) t += red[b][w];
            rstd[b] = gv_rstd(t, K, a.eps);
        }
        for (int p = threadIdx.x; p < npack; p += blockDim.x) {
            const uint4 gw = ld16((const T*)a.norm_w + (int64_t)p * V);
#pragma unroll
            for (int b = 0; b < NB; ++b) xs[(size_t)b * npack_pad + p] = gv_pack_norm<T>(xs[(size_t)b * npack_pad + p], gw, rstd[b]);
        }
    }
    __syncthreads();

    uint4 wv[ROWS][8];
    for (int g = wave; g < rg.count(); g += nwaves) {
        float acc[NB][ROWS];
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int r = 0; r < ROWS; ++r) acc[b][r] = 0.f;
        for (int c = 0; c < nchunk; ++c) {
            load_tile(g, c, wv);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
#pragma unroll
                for (int b = 0; b < NB; ++b) {
                    const uint4 xv = xs[(size_t)b * npack_pad + (c * 8 + i) * 64 + lane];
#pragma unroll
                    for (int r = 0; r < ROWS; ++r) acc[b][r] = dot_pack<T>(wv[r][i], xv, acc[b][r]);
                }
            }
        }
        gv_reduce_store<T, ROWS, NB>(a, rg, g, acc, lane);
    }
}

// ---- MFMA form: 3..16 sequences per sweep (16-bit types, K <= 4096 or K = 11008) ----------------------------------------------------
// Past 4 sequences the dot-product kernels above run out of VALU / LDS rate (8 sequences = 8 v_dot2 per 4 weight bytes
// plus 8 LDS reads per pack), while one v_mfma_f32_16x16x32 consumes 1 KB of weights for up to SIXTEEN sequences in 8
// passes: the matrix core turns the batched decode projection back into a pure weight stream.
//   * operands: A = 16 weight rows x 32 k (lane l: row l & 15, k-chunk l >> 4: ONE 16-byte load per lane per step, 64
//     contiguous bytes per row per instruction, the two halves of a 128-B line in consecutive instructions),
//     B = the activations (lane l: sequence l & 15, same k-chunk), D[row][sequence] in 4 VGPRs;
//   * a workgroup is 8 waves = 8 K slices of the same 16-row tile (K = 4096: 16 steps of 32 per wave); every wave keeps
//     ITS slice of the activations in 64 VGPRs for the whole launch (loaded — and RMS-normalised, statistic summed
//     across the 8 waves in a fixed order — once), so the stream loop issues nothing but weight loads;
//   * persistent: one workgroup per CU walks row tiles blockIdx, +grid, ...; the weights of the NEXT half-tile are
//     requested before the MFMAs of the current one (two register buffers of 8 steps), also across tile boundaries
//     and across the barrier: 8 - 16 KB per wave stay in flight the whole launch;
//   * per tile the 8 partial accumulators meet in LDS (double-buffered: one barrier per tile) and wave 0 applies the
//     epilogue (gv_epilogue: bias, rounding, residual | gv_silu_pair with the [gate; up] rows as two MFMA chains).
// (Written for 16-bit weights, one MFMA step per 16-byte load; fp8 and MXFP4 weights have 2 / 4 steps per load and take every
// sequence count from 1.)
template <int N, typename F, int... I>
__device__ __forceinline__ void gv_static_for_impl(F&& f, std::integer_sequence<int, I...>) {
    (f(std::integral_constant<int, I>{}), ...);
}
template <int N, typename F>
__device__ __forceinline__ void gv_static_for(F&& f) { gv_static_for_impl<N>(f, std::make_integer_sequence<int, N>{}); }

template <typename T> __device__ __forceinline__ f32x4_t gv_mfma(const uint4& a, const uint4& b, f32x4_t c);
template <> __device__ __forceinline__ f32x4_t gv_mfma<bf16_t>(const uint4& a, const uint4& b, f32x4_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
}
template <> __device__ __forceinline__ f32x4_t gv_mfma<f16_t>(const uint4& a, const uint4& b, f32x4_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), c, 0, 0, 0);
}

constexpr int kGvWaves = 8, kGvSteps = 16, kGvChunk = 8;

// The 8 waves' partial accumulators of one row tile meet in LDS (`part` = [8 waves][M][256] floats), wave 0 folds them in wave
// order and applies the epilogue.
// The epilogue's residual / bias values of wave 0 are requested at the TOP of the tile (gv_epi_prefetch), ahead of the weight
// loads: a load issued in the epilogue itself would have to be waited for with every younger weight prefetch in front of
// it (vmcnt is in-order), which stalls wave 0 — and through the next barrier the whole workgroup — once per tile.
struct GvEpi { uint2 res, bias; bool vec; };
template <typename T>
__device__ __forceinline__ GvEpi gv_epi_prefetch(const GemvArgs& a, int tile, int lane, bool vec_ok) {
    GvEpi e;
    e.vec = vec_ok;
    e.res = make_uint2(0, 0);
    e.bias = make_uint2(0, 0);
    if (vec_ok) {       // kernel-uniform: N, y_ld, res_ld multiples of 4 -> 8-byte accesses of 4 consecutive rows
        const int i = lane & 15, q = lane >> 4;
        int row0 = tile * 16 + q * 4;
        if (row0 > a.N - 4) row0 = a.N - 4;
        const int seq = i < a.nb ? i : 0;
        // (absent operands read the output row instead: in range, never used)
        const T* rp = (a.epi & SS_EPI_RESIDUAL) ? (const T*)a.residual + (int64_t)seq * a.res_ld : (const T*)a.y + (int64_t)seq * a.y_ld;
        const T* bp = (a.epi & SS_EPI_BIAS) ? (const T*)a.bias : (const T*)a.y + (int64_t)seq * a.y_ld;
        e.res = *reinterpret_cast<const uint2*>(rp + row0);
        e.bias = *reinterpret_cast<const uint2*>(bp + row0);
    }
    return e;
}
template <typename T> __device__ __forceinline__ float gv_elem(const uint2& v, int r) {
    const uint32_t w = r < 2 ? v.x : v.y;
    T t;
    t.v = (uint16_t)((r & 1) ? (w >> 16) : (w & 0xffffu));
    return Tr<T>::ld(&t);
}

template <int M>
__device__ __forceinline__ void gv_write_partials(float* part, const f32x4_t (&acc)[M], int wave, int lane) {
#pragma unroll
    for (int m = 0; m < M; ++m) *reinterpret_cast<f32x4_t*>(part + (wave * M + m) * 256 + lane * 4) = acc[m];
}
template <int M>
__device__ __forceinline__ void gv_fold(const float* part, int lane, f32x4_t (&v)[M]) {
#pragma unroll
    for (int m = 0; m < M; ++m) {
        v[m] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int w = 0; w < kGvWaves; ++w) v[m] += *reinterpret_cast<const f32x4_t*>(part + (w * M + m) * 256 + lane * 4);
    }
}
// epilogue + store of a folded tile: lane l holds D[row 4q + r][sequence i], i = l & 15, q = l >> 4
template <typename T, bool SILU>
__device__ __forceinline__ void gv_tile_store(const GemvArgs& a, const f32x4_t (&v)[SILU ? 2 : 1], int tile, int lane, const GvEpi& epi) {
    constexpr int M = SILU ? 2 : 1;
    const int i = lane & 15, q = lane >> 4;
    const int N = a.N;
    const int row0 = tile * 16 + q * 4;
    if (i >= a.nb || row0 >= N) return;
    float o[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = row0 + r < N ? row0 + r : N - 1;
        if constexpr (SILU) {
            o[r] = gv_silu_pair<T>(v[0][r], v[M - 1][r]);
        } else {
            if constexpr (sizeof(T) == 2) {
                if (epi.vec) {
                    o[r] = gv_epilogue<T>(v[0][r], [&] { return gv_elem<T>(epi.bias, r); }, [&] { return gv_elem<T>(epi.res, r); }, a.epi);
                    continue;
                }
            }
            o[r] = gv_epilogue<T>(v[0][r], [&] { return Tr<T>::ld((const T*)a.bias + row); },
                                  [&] { return Tr<T>::ld((const T*)a.residual + (int64_t)i * a.res_ld + row); }, a.epi);
        }
    }
    gv_store4<T>(a, i, row0, o);
}
// (`post`, the weight format's hook, sees the folded sums before the epilogue: fp8 weights apply their row scales there)
template <typename T, bool SILU, typename P>
__device__ __forceinline__ void gv_fold_store(const GemvArgs& a, float* part, const f32x4_t (&acc)[SILU ? 2 : 1], int tile,
                                              int wave, int lane, const GvEpi& epi, P&& post) {
    gv_write_partials(part, acc, wave, lane);
    __syncthreads();
    if (wave != 0) return;
    f32x4_t v[SILU ? 2 : 1];
    gv_fold(part, lane, v);
    post(v);
    gv_tile_store<T, SILU>(a, v, tile, lane, epi);
}
template <typename T, bool SILU>
__device__ __forceinline__ void gv_fold_store(const GemvArgs& a, float* part, const f32x4_t (&acc)[SILU ? 2 : 1], int tile,
                                              int wave, int lane, const GvEpi& epi) {
    gv_fold_store<T, SILU>(a, part, acc, tile, wave, lane, epi, [](auto&) {});
}

// RMSNorm statistic of the MFMA forms: a lane's sum over its k-chunks -> the four k-chunk lanes of a sequence -> the 8 waves in
// wave order (through red[8][16]; one barrier)
__device__ __forceinline__ float gv_rstd_across_waves(float ssq, float (*red)[16], int wave, int lane, int K, float eps) {
    ssq += __shfl_xor(ssq, 16, 64);
    ssq += __shfl_xor(ssq, 32, 64);
    if (lane < 16) red[wave][lane] = ssq;
    __syncthreads();
    float tot = 0.f;
#pragma unroll
    for (int w = 0; w < kGvWaves; ++w) tot += red[w][lane & 15];
    return gv_rstd(tot, K, eps);
}

// ---- the weight formats of the MFMA forms: what differs between 16-bit, fp8 and MXFP4 weights ---------------------------------------
// A lane's 16-byte weight load (a SLOT) feeds SPS MFMA steps of 8 k each: 1 (16-bit), 2 (fp8), 4 (MXFP4), so a format's K comes in
// multiples of 8 SPS, one slot of the 4 lane groups q = lane >> 4 covers 32 SPS consecutive k, and a row's slots lie 64 bytes
// apart.  A policy (used by the predicated tile loop below) finds a row at the lane's first k, loads slot L of it, turns step h of
// a slot into the A operand of gv_mfma<T>, and may hand the folded sums to a hook in front of the shared epilogue.  Step s of a
// lane = step s % SPS of slot s / SPS sees k = kb + 32 SPS (s / SPS) + 8 (s % SPS): the activation fragments follow from that.
struct GvNoPost { template <int M> __device__ __forceinline__ void operator()(f32x4_t (&)[M]) const {} };
template <int SPS_>
struct GvFmtBase {
    static constexpr int SPS = SPS_;
    static __device__ __forceinline__ uint4 zero() { return make_uint4(0, 0, 0, 0); }           // a slot of +0 codes
    template <int M> __device__ __forceinline__ GvNoPost post(int, int) const { return {}; }
};

// 16-bit weights [N, K]: a slot IS the operand (lane l: row l & 15, k-chunk l >> 4 of the step's 32 k)
template <typename T>
struct GvW16 : GvFmtBase<1> {
    using Slot = uint4;
    using Row = const T*;
    const T* __restrict__ W;
    int K;
    __device__ __forceinline__ GvW16(const GemvArgs& a) : W((const T*)a.W), K(a.K) {}
    __device__ __forceinline__ Row row(int64_t r, int kb) const { return W + r * K + kb; }
    template <int L> __device__ __forceinline__ Slot load(Row p) const { return ld16(p + L * 32); }
    template <int h> __device__ __forceinline__ uint4 operand(const Slot& w) const { return w; }
};

// ---- the predicated form: any K <= 4096 (a multiple of 8 SPS), any N -------------------------------------------------------------
// lpw <= 16 / SPS load slots per wave; loads predicated on the slots of this lane that lie inside K — correct for every shape, with
// the prefetch serialised by the predicates' branches (the tiny test models and odd widths; the LLaMA-7B depths take the stream
// loops below)
template <typename T, bool SILU, typename Fmt>
__device__ __forceinline__ void gv_mfma_tile_loop(const GemvArgs& a, Fmt fmt, const int lpw, const int ntiles) {
    constexpr int NS = kGvSteps, SPS = Fmt::SPS, NL = NS / SPS, M = SILU ? 2 : 1;
    __shared__ __attribute__((aligned(16))) float part[2][kGvWaves][M][256];
    __shared__ float red[kGvWaves][16];
    if (gemv_all_done(a)) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 15, q = lane >> 4;
    const int K = a.K, N = a.N, nb = a.nb;
    const int kb = wave * lpw * 32 * SPS + q * 8 * SPS;                 // this lane's k at its wave's slot 0
    int nvalid = kb < K ? (K - kb + 32 * SPS - 1) / (32 * SPS) : 0;     // slots of this lane that lie inside K (whole or not at all)
    if (nvalid > lpw) nvalid = lpw;
    auto koff = [&](int s) { return kb + (s / SPS) * 32 * SPS + (s % SPS) * 8; };                        // k of MFMA step s of this lane

    // ---- the wave's slice of the activations, in B-operand order (+ fused RMSNorm) -----------------------------------
    // (lanes of sequences >= nb read sequence 0: their columns of D are never stored)
    uint4 xf[NS];
    {
        const T* xr = (const T*)a.x + (int64_t)(i < nb ? i : 0) * a.x_ld;
        gv_static_for<NS>([&](auto s_) {
            constexpr int s = decltype(s_)::value;
            xf[s] = s / SPS < nvalid ? ld16(xr + koff(s)) : make_uint4(0, 0, 0, 0);
        });
        if (a.norm_w) {
            float ssq = 0.f;
            gv_static_for<NS>([&](auto s_) { ssq = gv_pack_ssq<T>(xf[decltype(s_)::value], ssq); });
            const float rstd = gv_rstd_across_waves(ssq, red, wave, lane, K, a.eps);
            gv_static_for<NS>([&](auto s_) {
                constexpr int s = decltype(s_)::value;
                if (s / SPS < nvalid) xf[s] = gv_pack_norm<T>(xf[s], ld16((const T*)a.norm_w + koff(s)), rstd);
            });
        }
    }
    typename Fmt::Slot wa[M][NL];
    int it = 0;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x, ++it) {
        int row = tile * 16 + i;
        if (row >= N) row = N - 1;
        const auto post = fmt.template post<M>(tile, lane);
        f32x4_t acc[M];
#pragma unroll
        for (int m = 0; m < M; ++m) {
            acc[m] = f32x4_t{0.f, 0.f, 0.f, 0.f};
            const typename Fmt::Row p = fmt.row((int64_t)row + (int64_t)m * N, kb);
            gv_static_for<NL>([&](auto s_) {
                constexpr int s = decltype(s_)::value;
                wa[m][s] = s < nvalid ? fmt.template load<s>(p) : Fmt::zero();
            });
        }
        gv_static_for<NL>([&](auto s_) {
            constexpr int s = decltype(s_)::value;
#pragma unroll
            for (int m = 0; m < M; ++m)
                gv_static_for<SPS>([&](auto h_) {
                    constexpr int h = decltype(h_)::value;
                    acc[m] = gv_mfma<T>(fmt.template operand<h>(wa[m][s]), xf[SPS * s + h], acc[m]);
                });
        });
        GvEpi epi;
        epi.vec = false;
        gv_fold_store<T, SILU>(a, &part[it & 1][0][0][0], acc, tile, wave, lane, epi, post);
    }
}
template <typename T, bool SILU>
__global__ __launch_bounds__(512) void gemv_mfma_kernel(const GemvArgs a, const int spw, const int ntiles) {
    gv_mfma_tile_loop<T, SILU>(a, GvW16<T>(a), spw, ntiles);
}

// ---- the stream loops: one kernel per weight format ----------------------------------------------------------------------------------
// The three kernels below are one algorithm too (two register buffers walked in chunks, the next tile's chunk 0 requested behind
// the last chunk, the nb <= 8 packing of the 11008-deep slice, vec_ok, the tile body), and differ in the points the format
// policies name plus how an odd slice is made to fit without a predicate (fp8's 8-byte tail load, MXFP4's dead eleventh slot).  They stay
// apart on purpose: one shared body over the policies was written and gave bit-identical results, but these launches are the decode
// token, and where a wave waits for its kernel arguments and in which order the compiler issues a slot's loads moved their times
// by 0.3 - 0.8 us per launch (profiles/gemv_formats_bench.json); two such effects were found and repaired, a third (the 16-bit
// SiLU pair, 1 %) was not.  A change of schedule here is made in all three.

// ---- the predicate-free stream loop for the two LLaMA-7B depths ---------------------------------------------------------------
// K == 8 waves x SPW steps x 32 exactly (SPW = 16: K = 4096, hidden; SPW = 43: K = 11008, the MLP width): every load of
// every lane is in range, so the stream loop carries no predicate and no branch (a predicated load is a branch to hipcc, and
// every branch join waits for vmcnt(0): the prefetch would be serialised).  The K slice of a wave is walked in chunks of 8
// steps through two register buffers; the loads of chunk c + 1 (or of the next tile's chunk 0) are issued before the MFMAs
// of chunk c, across the barrier too.
// SPW = 43 (PACK): 43 activation fragments per lane would take 172 VGPRs; only sequences 0..7 exist (nb <= 8), so lanes
// 8..15 of every 16-lane row carry steps 22..43 of sequences 0..7 and a row_shl:8 DPP move hands them to lanes 0..7 when
// their step comes up: 88 VGPRs.  (Columns 8..15 of D then hold garbage that is never stored.)  No RMSNorm in this form.
__device__ __forceinline__ void gv_fence(uint4& v) { asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w)); }

__device__ __forceinline__ uint4 gv_row_shift8(const uint4& v) {
    constexpr int ctrl = 0x108;                    // row_shl:8: lane l of a 16-lane row reads lane l + 8
    uint4 r;
    r.x = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v.x, ctrl, 0xf, 0xf, true);
    r.y = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v.y, ctrl, 0xf, 0xf, true);
    r.z = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v.z, ctrl, 0xf, 0xf, true);
    r.w = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v.w, ctrl, 0xf, 0xf, true);
    return r;
}

// RMSNorm of the resident activation fragments of a stream loop; fragment t sits koff(t) elements behind gw / its x pointer
template <typename T, int NF, typename KO>
__device__ __forceinline__ void gv_norm_frags(uint4 (&xf)[NF], const T* gw, KO&& koff, float (*red)[16], int wave, int lane, int K,
                                              float eps) {
    float ssq = 0.f;
    gv_static_for<NF>([&](auto s_) { ssq = gv_pack_ssq<T>(xf[decltype(s_)::value], ssq); });
    // (the fragments are unpacked AGAIN below: without this fence hipcc keeps the 128 unpacked floats alive across
    // the barrier and spills)
    gv_static_for<NF>([&](auto s_) { gv_fence(xf[decltype(s_)::value]); });
    const float rstd = gv_rstd_across_waves(ssq, red, wave, lane, K, eps);
    // the gain in two batches of 8 fragments (32 VGPRs in flight, not 64: with the activations and the first weights
    // resident the single batch spills)
    gv_static_for<2>([&](auto h_) {
        constexpr int h = decltype(h_)::value;
        uint4 gf[NF / 2];
        gv_static_for<NF / 2>([&](auto s_) { constexpr int s = decltype(s_)::value; gf[s] = ld16(gw + koff(h * (NF / 2) + s)); });
        gv_static_for<NF / 2>([&](auto s_) {
            constexpr int s = decltype(s_)::value, t = h * (NF / 2) + s;
            xf[t] = gv_pack_norm<T>(xf[t], gf[s], rstd);
        });
        __builtin_amdgcn_sched_barrier(0);
    });
}
template <typename T, bool SILU, int SPW, bool NT>
__global__ __launch_bounds__(512) void gemv_mfma_exact_kernel(const GemvArgs a, const int ntiles) {
    constexpr int CH = kGvChunk, M = SILU ? 2 : 1;
    constexpr int NCH = (SPW + CH - 1) / CH;
    constexpr bool PACK = SPW > kGvSteps;
    constexpr int HALF = PACK ? (SPW + 1) / 2 : SPW;        // fragments a lane holds
    static_assert(NCH % 2 == 0, "an even number of chunks keeps the buffer parity across tiles");
    __shared__ __attribute__((aligned(16))) float part[2][kGvWaves][M][256];
    __shared__ float red[kGvWaves][16];
    if (gemv_all_done(a)) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 15, q = lane >> 4;
    const int K = a.K, N = a.N, nb = a.nb;
    const T* __restrict__ W = (const T*)a.W;
    const int k0 = wave * SPW * 32 + q * 8;                         // this lane's k at the wave's step 0
    int tile = blockIdx.x, it = 0;
    if (tile >= ntiles) return;

    uint4 wa[2][M][CH];
    auto load_chunk = [&](auto c_, int tl) {                        // chunk c of row tile tl -> buffer c & 1
        constexpr int c = decltype(c_)::value;
        int row = tl * 16 + i;
        if (row >= N) row = N - 1;
#pragma unroll
        for (int m = 0; m < M; ++m) {
            const T* p = W + ((int64_t)row + (int64_t)m * N) * K + k0 + c * CH * 32;
            gv_static_for<CH>([&](auto e_) {
                constexpr int e = decltype(e_)::value;
                if constexpr (c * CH + e < SPW) wa[c & 1][m][e] = NT ? ld_nt16(p + e * 32) : ld16(p + e * 32);
            });
        }
    };

    // ---- the wave's slice of the activations, in B-operand order (+ fused RMSNorm) -----------------------------------
    uint4 xf[HALF];
    if constexpr (!PACK) {
        // (lanes of sequences >= nb read sequence 0: their columns of D are never stored)
        const T* xr = (const T*)a.x + (int64_t)(i < nb ? i : 0) * a.x_ld + k0;
        gv_static_for<HALF>([&](auto s_) { constexpr int s = decltype(s_)::value; xf[s] = ld16(xr + s * 32); });
        load_chunk(std::integral_constant<int, 0>{}, tile);         // the first weights travel while the statistic is formed
        __builtin_amdgcn_sched_barrier(0);
        if (a.norm_w) gv_norm_frags<T>(xf, (const T*)a.norm_w + k0, [](int t) { return t * 32; }, red, wave, lane, K, a.eps);
    } else {
        const int seq = i & 7, upper = i >> 3;
        const T* xr = (const T*)a.x + (int64_t)(seq < nb ? seq : 0) * a.x_ld + k0 + upper * HALF * 32;
        gv_static_for<HALF>([&](auto s_) {
            constexpr int s = decltype(s_)::value;
            if constexpr (s + HALF < SPW) xf[s] = ld16(xr + s * 32);
            else {                                                  // step s + HALF does not exist: the upper lanes hold zeros
                const uint4 v = ld16(xr + (upper ? s - 1 : s) * 32);
                xf[s] = upper ? make_uint4(0, 0, 0, 0) : v;
            }
        });
        load_chunk(std::integral_constant<int, 0>{}, tile);
    }
    // 8-byte epilogue accesses need 8-byte aligned BASES too (a bias / residual view at an odd element offset)
    const bool vec_ok = ((a.y_ld | a.res_ld | N) & 3) == 0 && N >= 4 && (a.epi & (SS_EPI_RESIDUAL | SS_EPI_BIAS)) &&
                        ((((size_t)a.y | (size_t)a.residual | (size_t)a.bias) & 7) == 0);

    // one row tile: per chunk — next chunk requested (the next TILE's first chunk behind the last one), this chunk consumed;
    // then partial sums to LDS, barrier, wave 0 folds the 8 slices and stores
    auto tile_body = [&](int tl, int itn, auto has_next_) {
        constexpr bool has_next = decltype(has_next_)::value;
        f32x4_t acc[M];
#pragma unroll
        for (int m = 0; m < M; ++m) acc[m] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        GvEpi epi;
        epi.vec = false;
        if constexpr (!SILU) epi = gv_epi_prefetch<T>(a, tl, lane, vec_ok);
        gv_static_for<NCH>([&](auto c_) {
            constexpr int c = decltype(c_)::value;
            if constexpr (c + 1 < NCH) load_chunk(std::integral_constant<int, c + 1>{}, tl);
            else if constexpr (has_next) load_chunk(std::integral_constant<int, 0>{}, tl + (int)gridDim.x);
            __builtin_amdgcn_sched_barrier(0);      // the scheduler otherwise sinks these loads below the MFMAs that free
            gv_static_for<CH>([&](auto e_) {        // their registers: one buffer in flight instead of two
                constexpr int e = decltype(e_)::value, s = c * CH + e;
                if constexpr (s < SPW) {
                    uint4 b;
                    if constexpr (!PACK) b = xf[s];
                    else if constexpr (s < HALF) b = xf[s];
                    else b = gv_row_shift8(xf[s - HALF]);
#pragma unroll
                    for (int m = 0; m < M; ++m) acc[m] = gv_mfma<T>(wa[c & 1][m][e], b, acc[m]);
                }
            });
            __builtin_amdgcn_sched_barrier(0);
        });
        gv_fold_store<T, SILU>(a, &part[itn & 1][0][0][0], acc, tl, wave, lane, epi);
    };
    for (; tile + (int)gridDim.x < ntiles; tile += gridDim.x, ++it) tile_body(tile, it, std::true_type{});
    tile_body(tile, it, std::false_type{});
}

// ---- fp8 (OCP e4m3fn) weight forms: half the bytes per k, the same matrix instruction ----------------------------------------------
// y[b][n] = epilogue( s[n] * sum_k dec(Wq[n][k]) * x[b][k] ):  Wq is [N, K] bytes in the 16-bit weights' row layout, s one fp32 scale
// per row.  A lane's 16-byte load now holds 16 consecutive k = TWO MFMA steps (lane l: row l & 15, bytes (l >> 4) * 16 .. + 15 of
// the load's 64 k; step 0 takes bytes 0..7, step 1 bytes 8..15), the codes are converted to the model's 16-bit type in registers
// (v_cvt_scalef32_pk_{bf16,f16}_fp8 with unit scale, two codes per instruction, exact: e4m3 is a subset of both types) and fed to
// gv_mfma<T>; the activation fragments are laid out to match (fragment 2L + h = x[load L's 64 k + 16 q + 8 h .. + 8]).  Every
// product of an e4m3 value and a 16-bit value is exact in fp32; the row scale is ONE fp32 multiply on the folded sum in front of
// the shared epilogue (gate and up rows of the SiLU pair have their own scales).  One sequence takes these forms too.
typedef __attribute__((ext_vector_type(2))) __bf16 gv_bf16x2_t;
typedef __attribute__((ext_vector_type(2))) _Float16 gv_f16x2_t;
template <typename T> __device__ __forceinline__ uint4 gv_dec8(uint32_t lo, uint32_t hi);      // 8 codes -> 8 values of T
template <> __device__ __forceinline__ uint4 gv_dec8<bf16_t>(uint32_t lo, uint32_t hi) {
    return make_uint4(__builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, false)),
                      __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, true)),
                      __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, false)),
                      __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, true)));
}
template <> __device__ __forceinline__ uint4 gv_dec8<f16_t>(uint32_t lo, uint32_t hi) {
    return make_uint4(__builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(lo, 1.0f, false)),
                      __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(lo, 1.0f, true)),
                      __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(hi, 1.0f, false)),
                      __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(hi, 1.0f, true)));
}

// the row scales of wave 0's four output rows (lane l: rows 4 (l >> 4) + r of the tile), requested at the top of the tile like
// gv_epi_prefetch and for the same reason.  vec (kernel-uniform): N % 4 == 0 and a 16-byte aligned scale vector -> one load.
template <int M>
struct GvScale {
    f32x4_t s[M];
    __device__ __forceinline__ void operator()(f32x4_t (&v)[M]) const {
#pragma unroll
        for (int m = 0; m < M; ++m) v[m] = v[m] * s[m];
    }
};
template <int M>
__device__ __forceinline__ GvScale<M> gv_scale_prefetch(const float* w_scale, int N, int tile, int lane, bool vec) {
    GvScale<M> r;
    const int row0 = tile * 16 + (lane >> 4) * 4;
#pragma unroll
    for (int m = 0; m < M; ++m) {
        const float* sp = w_scale + (int64_t)m * N;
        if (vec) {
            r.s[m] = *reinterpret_cast<const f32x4_t*>(sp + (row0 > N - 4 ? N - 4 : row0));
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) r.s[m][j] = sp[row0 + j < N ? row0 + j : N - 1];
        }
    }
    return r;
}
__device__ __forceinline__ bool gv_scale_vec_ok(const float* w_scale, int N) { return (N & 3) == 0 && N >= 4 && ((size_t)w_scale & 15) == 0; }
// any K <= 4096 (multiple of 16), any N: the predicated tile loop over the fp8 policy, LPW <= 8 loads of 64 k per wave
template <typename T>
struct GvW8 : GvFmtBase<2> {
    using Slot = uint4;
    using Row = const uint8_t*;
    const uint8_t* __restrict__ W;
    const float* __restrict__ scale;
    int K, N;
    bool svec;
    __device__ __forceinline__ GvW8(const GemvArgs& a, const float* w_scale)
        : W((const uint8_t*)a.W), scale(w_scale), K(a.K), N(a.N), svec(gv_scale_vec_ok(w_scale, a.N)) {}
    __device__ __forceinline__ Row row(int64_t r, int kb) const { return W + r * K + kb; }
    template <int L> __device__ __forceinline__ Slot load(Row p) const { return ld16(p + L * 64); }
    template <int h> __device__ __forceinline__ uint4 operand(const Slot& w) const { return h ? gv_dec8<T>(w.z, w.w) : gv_dec8<T>(w.x, w.y); }
    template <int M> __device__ __forceinline__ GvScale<M> post(int tile, int lane) const { return gv_scale_prefetch<M>(scale, N, tile, lane, svec); }
};

template <typename T, bool SILU>
__global__ __launch_bounds__(512) void gemv_w8_kernel(const GemvArgs a, const float* __restrict__ w_scale, const int lpw, const int ntiles) {
    gv_mfma_tile_loop<T, SILU>(a, GvW8<T>(a, w_scale), lpw, ntiles);
}

// the predicate-free stream loops: K == 8 waves x SPW MFMA steps x 32 (SPW = 16: K = 4096; SPW = 43: K = 11008), the structure of
// gemv_mfma_exact_kernel with half the loads.  A wave's K slice is SPW * 32 bytes per row = SPW / 2 loads of 16 bytes per lane, and
// for the odd SPW one last load of 8 bytes (one step: lane l bytes (l >> 4) * 8 .. + 7 of the slice's last 32): every load of every
// lane is in range, no predicate, no branch.  Load slots are walked in chunks of CH through two register buffers; the loads of
// chunk c + 1 (or of the next tile's chunk 0) are issued before the MFMAs of chunk c.
// SPW = 43 keeps the nb <= 8 packing of the 16-bit form (lanes 8..15 of a row carry the fragments of steps 22..42 of sequences
// 0..7, handed down by a row_shl:8 move): 88 VGPRs of activations; the halved load count leaves the rule as it was because the
// activations, not the weights, fill the registers.  No RMSNorm in that form.
template <typename T, bool SILU, int SPW>
__global__ __launch_bounds__(512) void gemv_w8_exact_kernel(const GemvArgs a, const float* __restrict__ w_scale, const int ntiles) {
    constexpr int M = SILU ? 2 : 1;
    constexpr bool PACK = SPW > kGvSteps, TAIL = (SPW & 1) != 0;
    constexpr int NSLOT = (SPW + 1) / 2;                    // loads per lane and row: SPW / 2 of 16 bytes (+ one of 8)
    constexpr int CH = PACK ? 6 : 4;                        // load slots per chunk
    constexpr int NCH = (NSLOT + CH - 1) / CH;
    constexpr int HALF = PACK ? (SPW + 1) / 2 : SPW;        // fragments a lane holds
    static_assert(NCH % 2 == 0, "an even number of chunks keeps the buffer parity across tiles");
    __shared__ __attribute__((aligned(16))) float part[2][kGvWaves][M][256];
    __shared__ float red[kGvWaves][16];
    if (gemv_all_done(a)) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 15, q = lane >> 4;
    const int K = a.K, N = a.N, nb = a.nb;
    const uint8_t* __restrict__ W = (const uint8_t*)a.W;
    const int kw = wave * SPW * 32;                                 // the wave's K slice
    // k of MFMA step s of this lane, relative to kw
    auto koff = [&](int s) { return (TAIL && s == SPW - 1) ? s * 32 + q * 8 : (s >> 1) * 64 + (s & 1) * 8 + q * 16; };
    int tile = blockIdx.x, it = 0;
    if (tile >= ntiles) return;

    uint4 wa[2][M][CH];
    auto load_chunk = [&](auto c_, int tl) {                        // chunk c of row tile tl -> buffer c & 1
        constexpr int c = decltype(c_)::value;
        int row = tl * 16 + i;
        if (row >= N) row = N - 1;
#pragma unroll
        for (int m = 0; m < M; ++m) {
            const uint8_t* p = W + ((int64_t)row + (int64_t)m * N) * K + kw;
            gv_static_for<CH>([&](auto e_) {
                constexpr int e = decltype(e_)::value, L = c * CH + e;
                if constexpr (TAIL && L == NSLOT - 1) {
                    const uint2 t = *reinterpret_cast<const uint2*>(p + (SPW - 1) * 32 + q * 8);
                    wa[c & 1][m][e] = make_uint4(t.x, t.y, 0, 0);
                } else if constexpr (L < NSLOT) {
                    wa[c & 1][m][e] = ld16(p + L * 64 + q * 16);
                }
            });
        }
    };

    // ---- the wave's slice of the activations, in B-operand order (+ fused RMSNorm) -----------------------------------
    uint4 xf[HALF];
    if constexpr (!PACK) {
        // (lanes of sequences >= nb read sequence 0: their columns of D are never stored)
        const T* xr = (const T*)a.x + (int64_t)(i < nb ? i : 0) * a.x_ld + kw;
        gv_static_for<HALF>([&](auto s_) { constexpr int s = decltype(s_)::value; xf[s] = ld16(xr + koff(s)); });
        load_chunk(std::integral_constant<int, 0>{}, tile);         // the first weights travel while the statistic is formed
        __builtin_amdgcn_sched_barrier(0);
        if (a.norm_w) gv_norm_frags<T>(xf, (const T*)a.norm_w + kw, koff, red, wave, lane, K, a.eps);
    } else {
        const int seq = i & 7, upper = i >> 3;
        const T* xr = (const T*)a.x + (int64_t)(seq < nb ? seq : 0) * a.x_ld + kw;
        gv_static_for<HALF>([&](auto s_) {
            constexpr int s = decltype(s_)::value;
            if constexpr (s + HALF < SPW) xf[s] = ld16(xr + (upper ? koff(s + HALF) : koff(s)));
            else {                                                  // step s + HALF does not exist: the upper lanes hold zeros
                const uint4 v = ld16(xr + koff(s));
                xf[s] = upper ? make_uint4(0, 0, 0, 0) : v;
            }
        });
        load_chunk(std::integral_constant<int, 0>{}, tile);
    }
    const bool vec_ok = ((a.y_ld | a.res_ld | N) & 3) == 0 && N >= 4 && (a.epi & (SS_EPI_RESIDUAL | SS_EPI_BIAS)) &&
                        ((((size_t)a.y | (size_t)a.residual | (size_t)a.bias) & 7) == 0);
    const bool svec = gv_scale_vec_ok(w_scale, N);

    auto tile_body = [&](int tl, int itn, auto has_next_) {
        constexpr bool has_next = decltype(has_next_)::value;
        f32x4_t acc[M];
#pragma unroll
        for (int m = 0; m < M; ++m) acc[m] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        GvEpi epi;
        epi.vec = false;
        if constexpr (!SILU) epi = gv_epi_prefetch<T>(a, tl, lane, vec_ok);
        const GvScale<M> sc = gv_scale_prefetch<M>(w_scale, N, tl, lane, svec);
        gv_static_for<NCH>([&](auto c_) {
            constexpr int c = decltype(c_)::value;
            if constexpr (c + 1 < NCH) load_chunk(std::integral_constant<int, c + 1>{}, tl);
            else if constexpr (has_next) load_chunk(std::integral_constant<int, 0>{}, tl + (int)gridDim.x);
            __builtin_amdgcn_sched_barrier(0);      // (as in gemv_mfma_exact_kernel: keeps two buffers in flight)
            gv_static_for<CH>([&](auto e_) {
                constexpr int e = decltype(e_)::value, L = c * CH + e;
                if constexpr (L < NSLOT) {
                    gv_static_for<2>([&](auto h_) {
                        constexpr int h = decltype(h_)::value, s = 2 * L + h;
                        if constexpr (s < SPW) {
                            uint4 b;
                            if constexpr (!PACK) b = xf[s];
                            else if constexpr (s < HALF) b = xf[s];
                            else b = gv_row_shift8(xf[s - HALF]);
#pragma unroll
                            for (int m = 0; m < M; ++m) {
                                const uint4& w = wa[c & 1][m][e];
                                acc[m] = gv_mfma<T>(h ? gv_dec8<T>(w.z, w.w) : gv_dec8<T>(w.x, w.y), b, acc[m]);
                            }
                        }
                    });
                }
            });
            __builtin_amdgcn_sched_barrier(0);
        });
        gv_fold_store<T, SILU>(a, &part[itn & 1][0][0][0], acc, tl, wave, lane, epi, [&](f32x4_t (&v)[M]) {
#pragma unroll
            for (int m = 0; m < M; ++m) v[m] = v[m] * sc.s[m];
        });
    };
    for (; tile + (int)gridDim.x < ntiles; tile += gridDim.x, ++it) tile_body(tile, it, std::true_type{});
    tile_body(tile, it, std::false_type{});
}

// ---- MXFP4 weight forms (OCP e2m1 codes + e8m0 block scales): a quarter of the bytes per k, the same matrix instruction ------------
// y[b][n] = epilogue( sum_k dec(code[n][k]) * 2^(scale[n][k / 32] - 127) * x[b][k] ):  codes [N, K / 2] bytes (k = 2j in bits 0-3
// of byte j, k = 2j + 1 in bits 4-7), scales [N, K / 32] bytes.  A lane's 16-byte load holds 32 consecutive k = ONE MX block = one
// scale byte = FOUR MFMA steps: load G of a row covers k = 128 G .. + 127, lane l (row l & 15, q = l >> 4) takes bytes 16 q .. + 15
// of its 64, i.e. k = 128 G + 32 q .. + 31 under scale byte 4 G + q, and step h (dword h of the load) the 8 k behind 8 h.
// v_cvt_scalef32_pk_{bf16,f16}_fp4 decodes two codes of a selected byte and applies 2^X in the same instruction (X in [-13, 13]:
// every value is a normal number of both types and exact), the result feeds gv_mfma<T>; the activation fragments are laid out to
// match (fragment 4 L + h = x[k of load L + 32 q + 8 h .. + 8]).  Every product is exact in fp32; there is no row scale, so the
// folded sum goes straight into the shared epilogue.  The scale byte travels with its load (one byte load per lane and slot).
template <typename T> __device__ __forceinline__ uint4 gv_dec8_mx4(uint32_t w, float sc);      // 8 codes of one dword -> 8 values of T
template <> __device__ __forceinline__ uint4 gv_dec8_mx4<bf16_t>(uint32_t w, float sc) {
    return make_uint4(__builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc, 0)),
                      __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc, 1)),
                      __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc, 2)),
                      __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc, 3)));
}
template <> __device__ __forceinline__ uint4 gv_dec8_mx4<f16_t>(uint32_t w, float sc) {
    return make_uint4(__builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, sc, 0)),
                      __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, sc, 1)),
                      __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, sc, 2)),
                      __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, sc, 3)));
}
__device__ __forceinline__ float gv_e8m0(uint32_t byte) { return __uint_as_float(byte << 23); }   // 2^(byte - 127)
__device__ __forceinline__ uint32_t gv_dword(const uint4& v, int h) { return h == 0 ? v.x : h == 1 ? v.y : h == 2 ? v.z : v.w; }
// any K <= 4096 (multiple of 32), any N: the predicated tile loop over the MXFP4 policy, LPW <= 4 loads of 128 k per wave
template <typename T>
struct GvMx4 : GvFmtBase<4> {
    struct Slot { uint4 w; uint32_t sc; };
    struct Row { const uint8_t *c, *s; };
    const uint8_t* __restrict__ W;
    const uint8_t* __restrict__ scale;
    int K;
    __device__ __forceinline__ GvMx4(const GemvArgs& a, const uint8_t* w_scale) : W((const uint8_t*)a.W), scale(w_scale), K(a.K) {}
    static __device__ __forceinline__ Slot zero() { return {make_uint4(0, 0, 0, 0), 127u}; }    // +0 codes under a unit scale
    __device__ __forceinline__ Row row(int64_t r, int kb) const { return {W + r * (K >> 1) + (kb >> 1), scale + r * (K >> 5) + (kb >> 5)}; }
    template <int L> __device__ __forceinline__ Slot load(Row p) const { return {ld16(p.c + L * 64), (uint32_t)p.s[L * 4]}; }
    template <int h> __device__ __forceinline__ uint4 operand(const Slot& w) const { return gv_dec8_mx4<T>(gv_dword(w.w, h), gv_e8m0(w.sc)); }
};

template <typename T, bool SILU>
__global__ __launch_bounds__(512) void gemv_mx4_kernel(const GemvArgs a, const uint8_t* __restrict__ w_scale, const int lpw, const int ntiles) {
    gv_mfma_tile_loop<T, SILU>(a, GvMx4<T>(a, w_scale), lpw, ntiles);
}

// the predicate-free stream loops.  K = 4096 (NL = 4): 32 loads of 128 k per row, four to a wave.  K = 11008 (NL = 11): 86 loads
// per row do not divide among 8 waves, and a wave's 43 blocks would not divide among the four lane groups of a load either, so the
// 86 loads are dealt 11 11 11 11 11 11 10 10: waves 0..5 run 11 load slots, waves 6 and 7 re-read their tenth load in the eleventh
// slot (in range) against zero activation fragments and a unit scale: every load of every lane is in range, no predicate, no
// branch.  Load slots are walked in chunks of CH through two register buffers; the loads of chunk c + 1 (or of the next tile's
// chunk 0) are issued before the MFMAs of chunk c.  NL = 11 keeps the nb <= 8 packing of the 16-bit form (lanes 8..15 of a row
// carry the fragments of steps 22..43 of sequences 0..7, handed down by a row_shl:8 move): 88 VGPRs of activations.  No RMSNorm
// in that form.
template <typename T, bool SILU, int NL>
__global__ __launch_bounds__(512) void gemv_mx4_exact_kernel(const GemvArgs a, const uint8_t* __restrict__ w_scale, const int ntiles) {
    constexpr int M = SILU ? 2 : 1;
    constexpr bool PACK = NL > kGvSteps / 4;
    constexpr int NLOADS = PACK ? 86 : 32;                  // 128-k loads per row
    constexpr int FULL = NLOADS - kGvWaves * (NL - 1);      // waves that own NL loads; the others own NL - 1
    constexpr bool HASDEAD = FULL < kGvWaves;
    constexpr int NSTEP = 4 * NL;
    constexpr int CH = PACK ? 3 : 2;                        // load slots per chunk
    constexpr int NCH = (NL + CH - 1) / CH;
    constexpr int HALF = PACK ? NSTEP / 2 : NSTEP;          // fragments a lane holds
    static_assert(NCH % 2 == 0, "an even number of chunks keeps the buffer parity across tiles");
    static_assert(FULL >= 0 && FULL <= kGvWaves && (!HASDEAD || (PACK && NSTEP - 4 >= HALF)), "the dead slot's fragments live in the upper lanes");
    __shared__ __attribute__((aligned(16))) float part[2][kGvWaves][M][256];
    __shared__ float red[kGvWaves][16];
    if (gemv_all_done(a)) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 15, q = lane >> 4;
    const int K = a.K, N = a.N, nb = a.nb;
    const uint8_t* __restrict__ W = (const uint8_t*)a.W;
    const bool dead = HASDEAD && wave >= FULL;                      // this wave's last slot carries no k
    const int g0 = wave < FULL ? wave * NL : FULL * NL + (wave - FULL) * (NL - 1);     // the wave's first load
    // load of slot L (the dead slot repeats the one before it)
    auto gload = [&](int L) { return g0 + ((dead && L == NL - 1) ? L - 1 : L); };
    // k of MFMA step s of this lane
    auto koff = [&](int s) { return gload(s >> 2) * 128 + q * 32 + (s & 3) * 8; };
    int tile = blockIdx.x, it = 0;
    if (tile >= ntiles) return;

    uint4 wa[2][M][CH];
    uint32_t ws[2][M][CH];
    auto load_chunk = [&](auto c_, int tl) {                        // chunk c of row tile tl -> buffer c & 1
        constexpr int c = decltype(c_)::value;
        int row = tl * 16 + i;
        if (row >= N) row = N - 1;
#pragma unroll
        for (int m = 0; m < M; ++m) {
            const int64_t r = (int64_t)row + (int64_t)m * N;
            const uint8_t* p = W + r * (K >> 1) + q * 16;
            const uint8_t* sp = w_scale + r * (K >> 5) + q;
            gv_static_for<CH>([&](auto e_) {
                constexpr int e = decltype(e_)::value, L = c * CH + e;
                if constexpr (L < NL) {
                    const int G = gload(L);
                    wa[c & 1][m][e] = ld16(p + G * 64);
                    ws[c & 1][m][e] = sp[G * 4];
                }
            });
        }
    };

    // ---- the wave's slice of the activations, in B-operand order (+ fused RMSNorm) -----------------------------------
    uint4 xf[HALF];
    if constexpr (!PACK) {
        // (lanes of sequences >= nb read sequence 0: their columns of D are never stored)
        const T* xr = (const T*)a.x + (int64_t)(i < nb ? i : 0) * a.x_ld;
        gv_static_for<HALF>([&](auto s_) { constexpr int s = decltype(s_)::value; xf[s] = ld16(xr + koff(s)); });
        load_chunk(std::integral_constant<int, 0>{}, tile);         // the first weights travel while the statistic is formed
        __builtin_amdgcn_sched_barrier(0);
        if (a.norm_w) gv_norm_frags<T>(xf, (const T*)a.norm_w, koff, red, wave, lane, K, a.eps);
    } else {
        const int seq = i & 7, upper = i >> 3;
        const T* xr = (const T*)a.x + (int64_t)(seq < nb ? seq : 0) * a.x_ld;
        gv_static_for<HALF>([&](auto s_) {
            constexpr int s = decltype(s_)::value;
            const uint4 v = ld16(xr + koff(s + upper * HALF));
            // the dead slot's four steps: zeros
            xf[s] = (s + HALF >= NSTEP - 4 && dead && upper) ? make_uint4(0, 0, 0, 0) : v;
        });
        load_chunk(std::integral_constant<int, 0>{}, tile);
    }
    const bool vec_ok = ((a.y_ld | a.res_ld | N) & 3) == 0 && N >= 4 && (a.epi & (SS_EPI_RESIDUAL | SS_EPI_BIAS)) &&
                        ((((size_t)a.y | (size_t)a.residual | (size_t)a.bias) & 7) == 0);

    auto tile_body = [&](int tl, int itn, auto has_next_) {
        constexpr bool has_next = decltype(has_next_)::value;
        f32x4_t acc[M];
#pragma unroll
        for (int m = 0; m < M; ++m) acc[m] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        GvEpi epi;
        epi.vec = false;
        if constexpr (!SILU) epi = gv_epi_prefetch<T>(a, tl, lane, vec_ok);
        gv_static_for<NCH>([&](auto c_) {
            constexpr int c = decltype(c_)::value;
            if constexpr (c + 1 < NCH) load_chunk(std::integral_constant<int, c + 1>{}, tl);
            else if constexpr (has_next) load_chunk(std::integral_constant<int, 0>{}, tl + (int)gridDim.x);
            __builtin_amdgcn_sched_barrier(0);      // (as in gemv_mfma_exact_kernel: keeps two buffers in flight)
            gv_static_for<CH>([&](auto e_) {
                constexpr int e = decltype(e_)::value, L = c * CH + e;
                if constexpr (L < NL) {
#pragma unroll
                    for (int m = 0; m < M; ++m) {
                        float sc = gv_e8m0(ws[c & 1][m][e]);
                        if constexpr (HASDEAD && L == NL - 1) sc = dead ? 1.0f : sc;    // (a re-read block times zeros: keep it finite)
                        const uint4& w = wa[c & 1][m][e];
                        gv_static_for<4>([&](auto h_) {
                            constexpr int h = decltype(h_)::value, s = 4 * L + h;
                            uint4 b;
                            if constexpr (!PACK) b = xf[s];
                            else if constexpr (s < HALF) b = xf[s];
                            else b = gv_row_shift8(xf[s - HALF]);
                            acc[m] = gv_mfma<T>(gv_dec8_mx4<T>(gv_dword(w, h), sc), b, acc[m]);
                        });
                    }
                }
            });
            __builtin_amdgcn_sched_barrier(0);
        });
        gv_fold_store<T, SILU>(a, &part[itn & 1][0][0][0], acc, tl, wave, lane, epi);
    };
    for (; tile + (int)gridDim.x < ntiles; tile += gridDim.x, ++it) tile_body(tile, it, std::true_type{});
    tile_body(tile, it, std::false_type{});
}

// ---- split-bf16 MFMA form for fp32 tensors (the gate mode, tuning knob gemm_f32_split; round 5) ---------------------------------
// The exact fp32 decode has no MFMA form: 8 lock-step sequences run as TWO 4-sequence sweeps of the dot-product kernels, i.e. the
// 26.4 GB of fp32 LLaMA weights are streamed twice per token (measured: ~700 of the 1093 ms the gate-mode MLLM half of a round of
// 8 stories takes).  Here one sweep serves 3..8 sequences through the matrix core with the arithmetic of the split GEMM
// (ss_gemm.hip SPLIT): w = hi + lo, x = hi + lo in bf16, y += Whi.xhi + Whi.xlo + Wlo.xhi with fp32 accumulation, ~4.5e-6 per
// product against the exact chain.
//   * the activations of the launch (<= 8 sequences x <= 4096 k) are split ONCE per workgroup into two bf16 planes in LDS
//     (wave w stages sequence w, RMSNorm fused: statistic over the whole row in a fixed lane order), sequence stride
//     2 k + 32 bytes so that the 16 lanes of a ds_read_b128 group (8 sequences x 2 k-chunks) fall on 16 different 16-byte slots;
//   * a lane streams 32 bytes of fp32 weights per step (row l & 15, k-chunk l >> 4), splits them in registers (8 conversions
//     + 8 subtractions, far below the HBM time of those bytes) and feeds three MFMAs; two register buffers of 4 steps keep
//     8-16 KB per wave in flight across tiles; out-of-range steps read a valid address and are zeroed by a select (no branch:
//     a predicated load would serialise the prefetch);
//   * K > 4096 (the 11008-deep down projection: N = 4096 = one row tile per workgroup) walks K slices of 4096 INSIDE the tile: the
//     planes are re-staged per slice (two barriers), the weight stream and the accumulators carry on — one launch, no read-modify-
//     write of y (the first version ran three launches: 70 us against ~48 for the same bytes);
//   * persistent workgroups of 8 waves = 8 K ranges of a 16-row tile; partial sums meet in LDS, wave 0 applies the epilogue.
constexpr int kGsSlice = 4096;

// LDS of gemv_split_f32_kernel (kernel and launch plan): two bf16 planes of 8 sequences, SS bytes apart, then ONE buffer of partial sums
// (a second one would push the SiLU instantiation past the 160 KB of a CU: the kernel pays a barrier per tile instead)
struct GvSplitLds {
    int SS, xl, part, bytes;
    __host__ __device__ GvSplitLds(int K, bool silu) {
        const int kmax = K < kGsSlice ? K : kGsSlice;
        SS = kmax * 2 + 32;                                  // bytes between sequences of a plane
        xl = 8 * SS;
        part = 16 * SS;                                      // [8 waves][M][256] floats
        bytes = part + kGvWaves * (silu ? 2 : 1) * 256 * (int)sizeof(float);
    }
};

template <bool SILU>
__global__ __launch_bounds__(512) void gemv_split_f32_kernel(const GemvArgs a, const int ntiles) {
    constexpr int CH = 4, NCH = kGvSteps / CH, M = SILU ? 2 : 1;
    extern __shared__ __attribute__((aligned(16))) char gs_smem[];
    if (gemv_all_done(a)) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 15, q = lane >> 4;
    const int K = a.K, N = a.N, nb = a.nb;
    const GvSplitLds lds(K, SILU);
    const int SS = lds.SS;
    const int nslices = (K + kGsSlice - 1) / kGsSlice;       // K > 4096 (the 11008-deep down projection): slices walked INSIDE the tile
    char* xh = gs_smem;
    char* xl = gs_smem + lds.xl;
    float* part = reinterpret_cast<float*>(gs_smem + lds.part);
    const float* __restrict__ W = (const float*)a.W;

    // ---- the activations of K slice [kbase, kbase + kslice) -> the two bf16 planes: wave w <-> sequence w -----------------
    float rstd = 1.f;
    const bool norm = a.norm_w != nullptr;                   // (single slice only: the launcher guarantees K <= 4096 with a norm)
    {
        const bool live = wave < nb;
        const float* xr = (const float*)a.x + (int64_t)(live ? wave : 0) * a.x_ld;
        if (norm) {
            float ssq = 0.f;
            for (int k = lane * 4; k < K; k += 256) ssq = gv_pack_ssq<float>(ld16(xr + k), ssq);
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) ssq += __shfl_xor(ssq, off, 64);
            rstd = gv_rstd(ssq, K, a.eps);
        }
    }
    auto stage = [&](int kbase, int kslice) {
        const int seq = wave;
        const bool live = seq < nb;
        const float* xr = (const float*)a.x + (int64_t)(live ? seq : 0) * a.x_ld;
        for (int k = lane * 4; k < kslice; k += 256) {
            uint4 u = live ? ld16(xr + kbase + k) : make_uint4(0, 0, 0, 0);
            if (norm) u = gv_pack_norm<float>(u, ld16((const float*)a.norm_w + kbase + k), rstd);
            const float4 v = make_float4(__uint_as_float(u.x), __uint_as_float(u.y), __uint_as_float(u.z), __uint_as_float(u.w));
            const uint32_t h01 = f32x2_to_bf16x2_bits(v.x, v.y), h23 = f32x2_to_bf16x2_bits(v.z, v.w);
            const float r0 = v.x - __uint_as_float(h01 << 16), r1 = v.y - __uint_as_float(h01 & 0xffff0000u);
            const float r2 = v.z - __uint_as_float(h23 << 16), r3 = v.w - __uint_as_float(h23 & 0xffff0000u);
            *reinterpret_cast<uint2*>(xh + seq * SS + k * 2) = make_uint2(h01, h23);
            *reinterpret_cast<uint2*>(xl + seq * SS + k * 2) = make_uint2(f32x2_to_bf16x2_bits(r0, r1), f32x2_to_bf16x2_bits(r2, r3));
        }
    };

    // B-fragment base of this lane: sequence i & 7 (columns 8..15 of D duplicate 0..7 and are never stored)
    const char* bh0 = xh + (i & 7) * SS + q * 16;
    const char* bl0 = xl + (i & 7) * SS + q * 16;
    int tile = blockIdx.x;
    if (tile >= ntiles) return;

    // geometry of a slice: steps of 32 k dealt to the 8 waves
    auto slice_len = [&](int sl) { const int r = K - sl * kGsSlice; return r < kGsSlice ? r : kGsSlice; };
    auto slice_spw = [&](int kslice) { return ((kslice + 31) / 32 + kGvWaves - 1) / kGvWaves; };   // <= 16

    uint4 wb[2][M][CH][2];
    auto load_chunk = [&](auto c_, int tl, int sl) {         // chunk c (4 steps) of slice sl of row tile tl -> buffer c & 1
        constexpr int c = decltype(c_)::value;
        const int kbase = sl * kGsSlice, kslice = slice_len(sl), spw = slice_spw(kslice), s_w0 = wave * spw;
        int row = tl * 16 + i;
        if (row >= N) row = N - 1;
#pragma unroll
        for (int m = 0; m < M; ++m) {
            const float* p = W + ((int64_t)row + (int64_t)m * N) * K + kbase;
            gv_static_for<CH>([&](auto e_) {
                constexpr int e = decltype(e_)::value;
                const int st = s_w0 + c * CH + e;
                const bool ok = (c * CH + e) < spw && st * 32 + q * 8 < kslice;
                const float* pp = p + (ok ? st * 32 + q * 8 : 0);   // an invalid step re-reads the slice's first 32 bytes (in range) ...
                wb[c & 1][m][e][0] = ld16(pp);
                wb[c & 1][m][e][1] = ld16(pp + 4);
            });
        }
    };
    auto split8 = [&](const uint4& w0, const uint4& w1, bool ok, uint4& hi, uint4& lo) {
        const float x0 = __uint_as_float(w0.x), x1 = __uint_as_float(w0.y), x2 = __uint_as_float(w0.z), x3 = __uint_as_float(w0.w);
        const float x4 = __uint_as_float(w1.x), x5 = __uint_as_float(w1.y), x6 = __uint_as_float(w1.z), x7 = __uint_as_float(w1.w);
        const uint32_t h0 = f32x2_to_bf16x2_bits(x0, x1), h1 = f32x2_to_bf16x2_bits(x2, x3);
        const uint32_t h2 = f32x2_to_bf16x2_bits(x4, x5), h3 = f32x2_to_bf16x2_bits(x6, x7);
        const uint32_t l0 = f32x2_to_bf16x2_bits(x0 - __uint_as_float(h0 << 16), x1 - __uint_as_float(h0 & 0xffff0000u));
        const uint32_t l1 = f32x2_to_bf16x2_bits(x2 - __uint_as_float(h1 << 16), x3 - __uint_as_float(h1 & 0xffff0000u));
        const uint32_t l2 = f32x2_to_bf16x2_bits(x4 - __uint_as_float(h2 << 16), x5 - __uint_as_float(h2 & 0xffff0000u));
        const uint32_t l3 = f32x2_to_bf16x2_bits(x6 - __uint_as_float(h3 << 16), x7 - __uint_as_float(h3 & 0xffff0000u));
        hi = ok ? make_uint4(h0, h1, h2, h3) : make_uint4(0, 0, 0, 0);     // ... and contributes zeros
        lo = ok ? make_uint4(l0, l1, l2, l3) : make_uint4(0, 0, 0, 0);
    };

    load_chunk(std::integral_constant<int, 0>{}, tile, 0);  // the first weights travel while the activations are staged
    stage(0, slice_len(0));
    __syncthreads();
    for (;;) {
        const int tnext = tile + (int)gridDim.x;
        const bool has_next = tnext < ntiles;                 // workgroup-uniform
        f32x4_t acc[M];
#pragma unroll
        for (int m = 0; m < M; ++m) acc[m] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        for (int sl = 0; sl < nslices; ++sl) {
            const int kslice = slice_len(sl), spw = slice_spw(kslice), s_w0 = wave * spw;
            const bool last_slice = sl + 1 == nslices;
            gv_static_for<NCH>([&](auto c_) {
                constexpr int c = decltype(c_)::value;
                if constexpr (c + 1 < NCH) load_chunk(std::integral_constant<int, c + 1>{}, tile, sl);
                else {                                         // NCH is even: the next slice's / tile's chunk 0 -> buffer 0
                    if (!last_slice) load_chunk(std::integral_constant<int, 0>{}, tile, sl + 1);
                    else if (has_next) load_chunk(std::integral_constant<int, 0>{}, tnext, 0);
                }
                gv_static_for<CH>([&](auto e_) {
                    constexpr int e = decltype(e_)::value;
                    const int st = s_w0 + c * CH + e;
                    const bool ok = (c * CH + e) < spw && st * 32 + q * 8 < kslice;
                    const int sb = ok ? st * 64 : -q * 16;    // 32 k x 2 bytes per step (invalid: the plane's first 16 bytes)
                    uint4 bh = *reinterpret_cast<const uint4*>(bh0 + sb);
                    uint4 bl = *reinterpret_cast<const uint4*>(bl0 + sb);
                    // (zero operands on BOTH sides: beyond the slice the planes hold whatever the LDS held, and 0 x NaN is NaN)
                    if (!ok) { bh = make_uint4(0, 0, 0, 0); bl = make_uint4(0, 0, 0, 0); }
#pragma unroll
                    for (int m = 0; m < M; ++m) {
                        uint4 ah, al;
                        split8(wb[c & 1][m][e][0], wb[c & 1][m][e][1], ok, ah, al);
                        acc[m] = gv_mfma<bf16_t>(al, bh, acc[m]);
                        acc[m] = gv_mfma<bf16_t>(ah, bl, acc[m]);
                        acc[m] = gv_mfma<bf16_t>(ah, bh, acc[m]);
                    }
                });
            });
            if (nslices > 1) {                                 // the planes of the next slice (of this tile, or slice 0 of the next tile)
                const int nsl = last_slice ? 0 : sl + 1;
                if (!last_slice || has_next) {
                    __syncthreads();                           // every wave has read its fragments of the current slice
                    stage(nsl * kGsSlice, slice_len(nsl));
                    __syncthreads();
                }
            }
        }
        // ---- fold the 8 K ranges and store ----------------------------------------------------------------------------
        __syncthreads();                                      // the previous tile's fold has finished reading `part`
#pragma unroll
        for (int m = 0; m < M; ++m) *reinterpret_cast<f32x4_t*>(part + (wave * M + m) * 256 + lane * 4) = acc[m];
        __syncthreads();
        if (wave == 0) {
            f32x4_t v[M];
#pragma unroll
            for (int m = 0; m < M; ++m) {
                v[m] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int w = 0; w < kGvWaves; ++w) v[m] += *reinterpret_cast<const f32x4_t*>(part + (w * M + m) * 256 + lane * 4);
            }
            const int row0 = tile * 16 + q * 4;               // D[row 4q + r][sequence i]
            if (i < nb && row0 < N) {
                float* y = (float*)a.y + (int64_t)i * a.y_ld;
                float o[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = row0 + r < N ? row0 + r : N - 1;
                    if constexpr (SILU) {
                        o[r] = silu_g(v[0][r]) * v[M - 1][r];
                    } else {
                        float t = v[0][r];
                        if (a.epi & SS_EPI_BIAS) t += ((const float*)a.bias)[row];
                        if (a.epi & SS_EPI_RESIDUAL) t += ((const float*)a.residual)[(int64_t)i * a.res_ld + row];
                        o[r] = t;
                    }
                }
                if (row0 + 3 < N && ((a.y_ld | row0) & 3) == 0 && (((size_t)a.y) & 15) == 0) {
                    *reinterpret_cast<float4*>(y + row0) = make_float4(o[0], o[1], o[2], o[3]);
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (row0 + r < N) y[row0 + r] = o[r];
                }
            }
        }
        if (!has_next) break;
        tile = tnext;
    }
}

// ---- launch plan ----------------------------------------------------------------------------------------------------------------------
// Which kernels serve a call is decided by gemv_plan, a pure function of the shape, the dtype, the epilogue and the tuning knobs (no
// HIP call: ss_gemv_plan exposes it to machines without a GPU); gemv_run is the only code that launches.
// one launch = one sweep of W for the sequences [seq0, seq0 + nseq); the row layout of ss_gemv_plan
struct GemvLaunch {
    int seq0, nseq;
    int form;                   // SS_GEMV_FORM_*
    int param;                  // SS_GEMV_FORM_REG: NIT (16-byte packs of x per lane); MFMA forms: steps of 32 k per wave; else 0
    int blocks, threads, lds;   // workgroups, workgroup size, dynamic LDS bytes
    int nt, silu;               // non-temporal weight loads; the SiLU(gate) * up pair
    int refused;                // the gate mode was asked for and this sweep runs an exact form instead
};
static_assert(sizeof(GemvLaunch) == SS_GEMV_PLAN_COLS * sizeof(int32_t), "ss_gemv_plan row layout");
struct GemvPlan { int n = 0; GemvLaunch l[SS_GEMV_PLAN_MAX]; };   // worst case: 16 sequences whose staged rows fit the LDS one at a time
constexpr size_t kGvLdsxMaxBytes = 152 * 1024;          // LDS-staged activations of one sweep

static int gemv_plan(int64_t N, int64_t K, int nb, int dtype, int epi, bool norm, bool aligned16, GemvPlan& plan) {
    SS_REQUIRE(dtype == SS_F32 || dtype == SS_BF16 || dtype == SS_F16, "unsupported dtype %d", dtype);
    const int V = dtype == SS_F32 ? 4 : 8;
    SS_REQUIRE(K % V == 0 && K > 0 && N > 0, "gemv: K=%lld must be a positive multiple of %d", (long long)K, V);
    SS_REQUIRE(!(epi & SS_EPI_SILU_MUL) || !(epi & (SS_EPI_BIAS | SS_EPI_RESIDUAL | SS_EPI_GELU)),
               "gemv: SILU_MUL cannot be combined with other epilogues");
    SS_REQUIRE(!(epi & SS_EPI_GELU), "gemv: GELU epilogue not supported");
    SS_REQUIRE(nb >= 1 && nb <= 16, "gemv: batch %d unsupported (1..16)", nb);
    const bool silu = (epi & SS_EPI_SILU_MUL) != 0;
    // MFMA forms, whole rounds: ceil(tiles / 256) tiles per workgroup on as few workgroups as that takes (688 tiles -> 230 x 3, not
    // 256 workgroups of which 80 run a third round alone)
    const int ntiles = cdiv(N, 16), mfma_blocks = cdiv(ntiles, cdiv(ntiles, knob(K_gemv_mfma_blocks)));
    // dot-product forms: several row groups per wave so the x prologue amortises; auto: ~2.5k waves (8-12 per CU) measured best
    const int nit = cdiv(K, 64 * V);
    const int64_t groups = silu ? N : (N + 1) / 2;
    int gpw = knob(K_gemv_groups_per_wave);
    if (gpw <= 0) { gpw = (int)((groups + 1280) / 2560); if (gpw < 1) gpw = 1; }
    const int64_t waves = (groups + gpw - 1) / gpw;
    auto blocks_for = [&](int wpb) { return (int)std::clamp<int64_t>((waves + wpb - 1) / wpb, 1, std::max(1, knob(K_gemv_max_blocks))); };
    const GvLdsxStage stage((int)K, V);

    // ranges of sequences still to place, first on top: a range no form takes in one sweep is swept as its two halves (every
    // launch takes >= 1 of <= 16 sequences: at most SS_GEMV_PLAN_MAX launches, and the stack holds one range per halving level)
    struct Range { int seq0, nseq, refused; } todo[8] = {{0, nb, 0}};
    int top = 1;
    while (top > 0) {
        const Range r = todo[--top];
        const int n = r.nseq;
        GemvLaunch l = {r.seq0, n, SS_GEMV_FORM_REG, 0, 0, 0, 0, 0, silu, r.refused};
        // 3+ sequences (knob): the MFMA form when the shape allows it (16-bit, 8 waves x 16 steps of 32 cover K, or the packed
        // 11008-deep form: <= 8 sequences, no RMSNorm prologue).  Measured on the five LLaMA-7B projections (tools/gemv_bench.py,
        // rotating weights, us per launch): dot-product kernels at 1 | 4 sequences 20.7 9.9 32.3 19.3 46.1 | 24.4 11.0 39.0 25.7 47.8;
        // MFMA form at 8 sequences 24.2 9.9 37.3 21.9 46.2 — one sequence stays with the dot-product kernel.
        const bool mfma_nb = n >= knob(K_gemv_mfma_min_nb);
        const bool generic = knob(K_gemv_mfma_generic) != 0;
        const bool exact43 = K == kGvWaves * 43 * 32 && n <= 8 && !norm && !generic && knob(K_gemv_mfma_long);
        // fp32 tensors in the gate mode: 3..8 sequences through the split-bf16 MFMA form (one sweep of W instead of two exact ones)
        const bool gate = V == 4 && mfma_nb && n <= 8 && knob(K_gemm_f32_split);
        if (V == 8 && mfma_nb && (K <= kGvWaves * kGvSteps * 32 || exact43)) {
            l.form = exact43 ? SS_GEMV_FORM_MFMA_EXACT43 : (!generic && K == kGvWaves * kGvSteps * 32) ? SS_GEMV_FORM_MFMA_EXACT16 : SS_GEMV_FORM_MFMA;
            l.param = exact43 ? 43 : cdiv(cdiv(K, 32), kGvWaves);
            l.blocks = mfma_blocks, l.threads = 512;
            // plain loads, not non-temporal ones: a fragment load touches HALF a 128-byte line per row and the next instruction the
            // other half; measured on the five LLaMA-7B shapes at 8 sequences, nt is 3 - 13 % slower (lm_head 52.0 vs 46.2 us)
            l.nt = l.form != SS_GEMV_FORM_MFMA && knob(K_gemv_mfma_nt) != 0;
        } else if (gate && K % 8 == 0 && ((!norm && !silu) || K <= kGsSlice) && aligned16) {
            // (the RMSNorm prologue needs the whole row in one K slice; SiLU pairs too)
            l.form = SS_GEMV_FORM_SPLIT_F32;
            l.blocks = mfma_blocks, l.threads = 512;
            l.lds = GvSplitLds((int)K, silu).bytes;
        } else {
            // a refused gate-mode sweep (RMSNorm / SiLU row wider than one 4096 slice, or 16-byte misalignment) runs EXACT forms
            if (gate) l.refused = 1;
            // x slices live in registers while batch * NIT <= reg budget (16 packs = 64 VGPRs at batch 2, NIT = 8); else in LDS
            const bool in_regs = nit <= 8 && n * nit <= knob(K_gemv_x_reg_packs) && !knob(K_gemv_force_lds);
            const size_t lds = in_regs ? 0 : stage.bytes(n);
            if (n > 4 || (n > 1 && lds > kGvLdsxMaxBytes)) {     // no form for this many sequences, or their activations overflow the LDS
                todo[top++] = {r.seq0 + n / 2, n - n / 2, l.refused};
                todo[top++] = {r.seq0, n / 2, l.refused};
                continue;
            }
            SS_REQUIRE(lds <= kGvLdsxMaxBytes, "gemv: K=%lld x batch %d too large for LDS staging", (long long)K, n);
            l.nt = knob(K_gemv_nt), l.lds = (int)lds;
            if (in_regs) {
                for (l.param = 1; l.param < nit;) l.param *= 2;    // gemv_kernel is instantiated for NIT 1, 2, 4, 8
                l.blocks = blocks_for(4), l.threads = 256;
            } else if (n == 1) {
                // batch 1 (the reference configuration): several 256-thread blocks per CU, ~2.5k waves (measured optimum)
                l.form = SS_GEMV_FORM_LDSX;
                l.threads = lds <= 36 * 1024 ? 256 : lds <= 72 * 1024 ? 512 : 1024;
                l.blocks = blocks_for(l.threads / 64);
            } else {
                // every block stages all rows of x, so blocks are fat and their count is a whole number per CU (no CU ends up with one
                // block more than its neighbour): 2 x 512 threads per CU, or 1 x 1024 when the staged activations exceed half the LDS
                const int per_cu = lds <= 76 * 1024 ? 2 : 1;
                l.form = SS_GEMV_FORM_LDSX;
                l.threads = per_cu == 2 ? 512 : 1024;
                l.blocks = 256 * per_cu;
                const int64_t max_b = (waves * 2 + l.threads / 64 - 1) / (l.threads / 64);   // keep >= ~2 row groups per wave
                if (l.blocks > max_b) l.blocks = (int)(max_b < 1 ? 1 : max_b);
            }
        }
        plan.l[plan.n++] = l;
    }
    return SS_OK;
}

// The weight formats of the MFMA kernels on the host: 16-bit (chosen by gemv_plan above), then the quantised ones in the order of
// GEMV_WQ_*.  plane: what the refusals call the weight argument; forms: the predicated kernel, the stream loops of K = 4096 and
// K = 11008.  A plan row's param counts MFMA steps of 32 k per wave, `sps` of them to a 16-byte load slot (MXFP4 rounds the 43 of
// K = 11008 up to whole slots: 44).
struct GvFormat { const char *name, *plane; int kmult, sps, forms[3], param43; };
static const GvFormat kGvFormats[3] = {
    {"gemv", "W", 8, 1, {SS_GEMV_FORM_MFMA, SS_GEMV_FORM_MFMA_EXACT16, SS_GEMV_FORM_MFMA_EXACT43}, 43},
    {"gemv_w8", "Wq", 16, 2, {SS_GEMV_FORM_W8, SS_GEMV_FORM_W8_EXACT16, SS_GEMV_FORM_W8_EXACT43}, 43},
    {"gemv_mx4", "codes", 32, 4, {SS_GEMV_FORM_MX4, SS_GEMV_FORM_MX4_EXACT16, SS_GEMV_FORM_MX4_EXACT43}, 44}};

// The quantised-weight calls (kind = GEMV_WQ_*): always an MFMA form (one sequence too).  K = 4096 and K = 11008 take the stream
// loops, every other K <= 4096 (and the knob gemv_mfma_generic) the predicated kernel; the packed 11008-deep loop takes <= 8
// sequences, so 9..16 run as two sweeps.  Anything else is refused here, before a launch.
static int gemv_wq_plan(int kind, int64_t N, int64_t K, int nb, int dtype, int epi, bool norm, GemvPlan& plan) {
    SS_REQUIRE(kind == GEMV_WQ_FP8 || kind == GEMV_WQ_MXFP4, "gemv: unknown weight format %d", kind);
    const GvFormat& f = kGvFormats[kind];
    SS_REQUIRE(dtype == SS_BF16 || dtype == SS_F16, "%s: the model dtype must be bf16 or fp16 (got %d)", f.name, dtype);
    constexpr int64_t K16 = kGvWaves * kGvSteps * 32, K43 = kGvWaves * 43 * 32;
    SS_REQUIRE(N > 0 && K > 0 && K % f.kmult == 0 && (K <= K16 || K == K43),
               "%s: K=%lld must be a positive multiple of %d, at most %lld or exactly %lld (N=%lld)", f.name, (long long)K, f.kmult,
               (long long)K16, (long long)K43, (long long)N);
    SS_REQUIRE(N < (1ll << 30), "%s: N=%lld too large", f.name, (long long)N);
    SS_REQUIRE(!(epi & SS_EPI_SILU_MUL) || !(epi & (SS_EPI_BIAS | SS_EPI_RESIDUAL | SS_EPI_GELU)),
               "%s: SILU_MUL cannot be combined with other epilogues", f.name);
    SS_REQUIRE(!(epi & ~(SS_EPI_BIAS | SS_EPI_RESIDUAL | SS_EPI_SILU_MUL)), "%s: epilogue %d not supported", f.name, epi);
    SS_REQUIRE(nb >= 1 && nb <= 16, "%s: batch %d unsupported (1..16)", f.name, nb);
    SS_REQUIRE(K != K43 || !norm, "%s: no RMSNorm prologue at K=%lld", f.name, (long long)K);
    const bool silu = (epi & SS_EPI_SILU_MUL) != 0;
    const int ntiles = cdiv(N, 16), blocks = cdiv(ntiles, cdiv(ntiles, knob(K_gemv_mfma_blocks)));
    const bool exact16 = K == K16 && !knob(K_gemv_mfma_generic);
    const int sweeps = (K == K43 && nb > 8) ? 2 : 1;
    for (int j = 0; j < sweeps; ++j) {
        const int seq0 = j * (nb / 2), n = sweeps == 1 ? nb : (j ? nb - nb / 2 : nb / 2);
        GemvLaunch l = {seq0, n, f.forms[0], 0, blocks, 512, 0, 0, silu, 0};
        if (K == K43) l.form = f.forms[2], l.param = f.param43;
        else if (exact16) l.form = f.forms[1], l.param = kGvSteps;
        else l.param = f.sps * cdiv(cdiv(K, 32 * f.sps), kGvWaves);
        plan.l[plan.n++] = l;
    }
    return SS_OK;
}

// ---- kernel tables --------------------------------------------------------------------------------------------------------------------
using GemvKern = void (*)(GemvArgs);
// ROWS = 2 keeps 16 x 16 B per lane in flight at NIT = 8 (and SiLU pairs need exactly 2 rows)
template <typename T, int NB>
static GemvKern gv_dot_kernel_nb(const GemvLaunch& l) {
    if (l.form == SS_GEMV_FORM_LDSX) return gemv_ldsx_kernel<T, 2, NB>;
    static constexpr GemvKern by_nit[9] = {nullptr, gemv_kernel<T, 1, 2, NB>, gemv_kernel<T, 2, 2, NB>, nullptr, gemv_kernel<T, 4, 2, NB>,
                                           nullptr, nullptr, nullptr, gemv_kernel<T, 8, 2, NB>};
    return by_nit[l.param];
}
template <typename T>
static GemvKern gv_dot_kernel(const GemvLaunch& l) {
    static constexpr GemvKern (*by_nb[4])(const GemvLaunch&) = {gv_dot_kernel_nb<T, 1>, gv_dot_kernel_nb<T, 2>, gv_dot_kernel_nb<T, 3>, gv_dot_kernel_nb<T, 4>};
    return by_nb[l.nseq - 1](l);
}
// the MFMA kernel of role 0 (predicated) / 1 (stream loop, K = 4096) / 2 (K = 11008), by format (the index of kGvFormats)
template <typename T, bool SILU>
static const void* gv_mfma_kernel(int role, int fmt, bool nt) {
#define GV_K(...) ((const void*)&__VA_ARGS__)
    const void* const k[3][3] = {
        {GV_K(gemv_mfma_kernel<T, SILU>), GV_K(gemv_w8_kernel<T, SILU>), GV_K(gemv_mx4_kernel<T, SILU>)},
        {nt ? GV_K(gemv_mfma_exact_kernel<T, SILU, 16, true>) : GV_K(gemv_mfma_exact_kernel<T, SILU, 16, false>), GV_K(gemv_w8_exact_kernel<T, SILU, 16>),
         GV_K(gemv_mx4_exact_kernel<T, SILU, 4>)},
        {nt ? GV_K(gemv_mfma_exact_kernel<T, SILU, 43, true>) : GV_K(gemv_mfma_exact_kernel<T, SILU, 43, false>), GV_K(gemv_w8_exact_kernel<T, SILU, 43>),
         GV_K(gemv_mx4_exact_kernel<T, SILU, 11>)}};
#undef GV_K
    return k[role][fmt];
}
template <bool SILU>
static int gemv_run_split(const GemvLaunch& l, const GemvArgs& a, hipStream_t s) {
    SS_DYN_LDS(gemv_split_f32_kernel<SILU>, (size_t)GvSplitLds(kGsSlice, true).bytes);   // the largest request: full slice, SiLU pair
    hipLaunchKernelGGL(gemv_split_f32_kernel<SILU>, dim3((unsigned)l.blocks), dim3((unsigned)l.threads), (size_t)l.lds, s, a, cdiv(a.N, 16));
    return SS_OK;
}

// w_scale: the scale plane of a quantised call (fp32 row scales | e8m0 block scales), an extra argument of its kernels
template <typename T>
static int gemv_run(const GemvPlan& plan, const GemvArgs& args, hipStream_t s, const void* w_scale = nullptr) {
    for (int j = 0; j < plan.n; ++j) {
        const GemvLaunch& l = plan.l[j];
        GemvArgs a = args;
        a.nb = l.nseq, a.use_nt = l.nt;
        a.x = (const T*)args.x + (int64_t)l.seq0 * args.x_ld;
        a.y = (T*)args.y + (int64_t)l.seq0 * args.y_ld;
        if (args.residual) a.residual = (const T*)args.residual + (int64_t)l.seq0 * args.res_ld;
        if (args.done_flag) a.done_flag = args.done_flag + (int64_t)l.seq0 * args.done_stride;
        const dim3 g((unsigned)l.blocks), b((unsigned)l.threads);
        if (l.form == SS_GEMV_FORM_REG || l.form == SS_GEMV_FORM_LDSX) {
            const GemvKern k = gv_dot_kernel<T>(l);
            if (l.lds > 64 * 1024)     // (the request depends on K: set per launch, return code checked)
                SS_HIP(hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, l.lds));
            hipLaunchKernelGGL(k, g, b, (size_t)l.lds, s, a);
        } else if constexpr (sizeof(T) == 4) {
            const int rc = l.silu ? gemv_run_split<true>(l, a, s) : gemv_run_split<false>(l, a, s);
            if (rc) return rc;
        } else {
            int fmt = -1, role = 0;
            for (int f = 0; f < 3; ++f)
                for (int r = 0; r < 3; ++r)
                    if (kGvFormats[f].forms[r] == l.form) fmt = f, role = r;
            SS_REQUIRE(fmt >= 0, "gemv: no kernel for form %d", l.form);
            // The arguments in the order of the six wrappers' parameter lists (hipLaunchKernel checks nothing):
            //   predicated   (GemvArgs, [scale plane,] load slots per wave, row tiles)      gemv_mfma_kernel | gemv_w8_kernel | gemv_mx4_kernel
            //   stream loop  (GemvArgs, [scale plane,] row tiles)                           gemv_*_exact_kernel
            // the scale plane (const float* | const uint8_t*) only where fmt > 0.
            int slots = l.param / kGvFormats[fmt].sps, ntiles = cdiv(a.N, 16), n = 0;
            void* kargs[4];
            kargs[n++] = &a;
            if (fmt) kargs[n++] = &w_scale;
            if (role == 0) kargs[n++] = &slots;
            kargs[n++] = &ntiles;
            SS_HIP(hipLaunchKernel(l.silu ? gv_mfma_kernel<T, true>(role, fmt, l.nt) : gv_mfma_kernel<T, false>(role, fmt, l.nt), g, b, kargs, 0, s));
        }
        static const char* const what[] = {"gemv", "gemv_ldsx", "gemv_mfma", "gemv_mfma", "gemv_mfma", "gemv_split_f32", "gemv_w8", "gemv_w8", "gemv_w8",
                                           "gemv_mx4", "gemv_mx4", "gemv_mx4"};
        SS_LAUNCH_CHECK(what[l.form]);
    }
    return SS_OK;
}

static GemvArgs gemv_args(const void* W, const void* x, void* y, int64_t N, int64_t K, const void* norm_w, float eps, const void* bias,
                          const void* residual, int epi, const int32_t* done_flag, int done_stride, int nb, int64_t x_ld, int64_t y_ld,
                          int64_t res_ld) {
    GemvArgs a;
    a.W = W; a.x = x; a.y = y; a.norm_w = norm_w; a.bias = bias; a.residual = residual; a.done_flag = done_flag;
    a.N = (int)N; a.K = (int)K; a.epi = epi; a.eps = eps; a.use_nt = 0;
    a.nb = nb; a.done_stride = done_stride; a.x_ld = x_ld; a.y_ld = y_ld; a.res_ld = res_ld;
    return a;
}

int gemv_batched_dev(const void* W, const void* x, void* y, int64_t N, int64_t K, const void* norm_w, float eps,
                     const void* bias, const void* residual, int epi, const int32_t* done_flag, int done_stride,
                     int nb, int64_t x_ld, int64_t y_ld, int64_t res_ld, int dtype, hipStream_t s) {
    GemvPlan plan;
    const bool aligned16 = (((size_t)x | (size_t)W | (size_t)norm_w) & 15) == 0 && (x_ld & 3) == 0;     // what the split form needs
    const int rc = gemv_plan(N, K, nb, dtype, epi, norm_w != nullptr, aligned16, plan);
    if (rc) return rc;
    bool refused = false;
    for (int j = 0; j < plan.n; ++j) refused |= plan.l[j].refused != 0;
    if (refused) {      // counted once per call (knob gemv_split_refused) and reported once per process
        static bool told = false;
        knob_add(K_gemv_split_refused, 1);
        if (!told) {
            told = true;
            fprintf(stderr, "[ss] gate mode: GEMV [N=%lld, K=%lld, %d slots]%s%s runs as exact 4-slot sweeps (split form needs norm / SiLU "
                            "rows <= %d wide and 16-byte alignment)\n", (long long)N, (long long)K, nb, norm_w ? " +RMSNorm" : "",
                    (epi & SS_EPI_SILU_MUL) ? " +SiLU" : "", kGsSlice);
        }
    }
    const GemvArgs a = gemv_args(W, x, y, N, K, norm_w, eps, bias, residual, epi, done_flag, done_stride, nb, x_ld, y_ld, res_ld);
    return SS_DISPATCH(dtype, gemv_run, plan, a, s);
}

int gemv_wq_check(int kind, int64_t N, int64_t K, int nb, int dtype, int epi, bool norm) {
    GemvPlan plan;
    return gemv_wq_plan(kind, N, K, nb, dtype, epi, norm, plan);
}

int gemv_wq_batched_dev(int kind, const void* codes, const void* scales, const void* x, void* y, int64_t N, int64_t K, const void* norm_w,
                        float eps, const void* bias, const void* residual, int epi, const int32_t* done_flag, int done_stride,
                        int nb, int64_t x_ld, int64_t y_ld, int64_t res_ld, int dtype, hipStream_t s) {
    GemvPlan plan;
    const int rc = gemv_wq_plan(kind, N, K, nb, dtype, epi, norm_w != nullptr, plan);
    if (rc) return rc;
    const char *name = kGvFormats[kind].name, *plane = kGvFormats[kind].plane;
    SS_REQUIRE(codes && scales && x && y, "%s: NULL argument", name);
    SS_REQUIRE(!(epi & SS_EPI_BIAS) || bias, "%s: BIAS epilogue without a bias", name);
    SS_REQUIRE(!(epi & SS_EPI_RESIDUAL) || residual, "%s: RESIDUAL epilogue without a residual", name);
    SS_REQUIRE((((size_t)codes | (size_t)x | (size_t)norm_w) & 15) == 0 && (x_ld & 7) == 0 && (kind != GEMV_WQ_FP8 || ((size_t)scales & 3) == 0),
               "%s: %s, x and norm_w must be 16-byte aligned (x row stride a multiple of 8 elements)", name, plane);
    const GemvArgs a = gemv_args(codes, x, y, N, K, norm_w, eps, bias, residual, epi, done_flag, done_stride, nb, x_ld, y_ld, res_ld);
    return dtype == SS_BF16 ? gemv_run<bf16_t>(plan, a, s, scales) : gemv_run<f16_t>(plan, a, s, scales);
}

int gemv_dev(const void* W, const void* x, void* y, int64_t N, int64_t K, const void* norm_w, float eps,
             const void* bias, const void* residual, int epi, const int32_t* done_flag, int dtype, hipStream_t s) {
    return gemv_batched_dev(W, x, y, N, K, norm_w, eps, bias, residual, epi, done_flag, 0, 1, K, N, N, dtype, s);
}

// the rows of a plan -> the caller's array (ss_gemv_plan and its quantised siblings)
static int gemv_plan_out(const char* who, int rc, const GemvPlan& plan, int32_t* rows, int64_t max_rows) {
    if (rc) return rc;
    SS_REQUIRE(rows && max_rows >= plan.n, "%s: %d rows needed, room for %lld", who, plan.n, (long long)max_rows);
    memcpy(rows, plan.l, (size_t)plan.n * sizeof(GemvLaunch));
    return plan.n;
}

}  // namespace ss

extern "C" int ss_gemv(const void* W, const void* x, void* y, int64_t N, int64_t K, const void* norm_w, float eps,
                       const void* bias, const void* residual, int epilogue, int dtype, void* stream) {
    return ss::gemv_dev(W, x, y, N, K, norm_w, eps, bias, residual, epilogue, nullptr, dtype, (hipStream_t)stream);
}

extern "C" int ss_gemv_batched(const void* W, const void* x, void* y, int64_t N, int64_t K, int64_t nb, const void* norm_w, float eps,
                               const void* bias, const void* residual, int epilogue, int dtype, void* stream) {
    return ss::gemv_batched_dev(W, x, y, N, K, norm_w, eps, bias, residual, epilogue, nullptr, 0, (int)nb, K, N, N, dtype, (hipStream_t)stream);
}

extern "C" int ss_gemv_plan(int64_t N, int64_t K, int64_t nb, int dtype, int epilogue, int has_norm, int aligned16, int32_t* rows,
                            int64_t max_rows) {
    ss::GemvPlan plan;
    return ss::gemv_plan_out("ss_gemv_plan", ss::gemv_plan(N, K, (int)nb, dtype, epilogue, has_norm != 0, aligned16 != 0, plan), plan, rows, max_rows);
}

extern "C" int ss_gemv_w8(const void* Wq, const float* w_scale, const void* x, void* y, int64_t N, int64_t K, int64_t nb,
                          const void* norm_w, float eps, const void* bias, const void* residual, int epilogue, int dtype, void* stream) {
    SS_REQUIRE(nb >= 1 && nb <= 16, "gemv_w8: batch %lld unsupported (1..16)", (long long)nb);
    return ss::gemv_wq_batched_dev(ss::GEMV_WQ_FP8, Wq, w_scale, x, y, N, K, norm_w, eps, bias, residual, epilogue, nullptr, 0, (int)nb, K, N, N,
                                   dtype, (hipStream_t)stream);
}

extern "C" int ss_gemv_w8_plan(int64_t N, int64_t K, int64_t nb, int dtype, int epilogue, int has_norm, int32_t* rows, int64_t max_rows) {
    ss::GemvPlan plan;
    SS_REQUIRE(nb >= 1 && nb <= 16, "gemv_w8: batch %lld unsupported (1..16)", (long long)nb);
    return ss::gemv_plan_out("ss_gemv_w8_plan", ss::gemv_wq_plan(ss::GEMV_WQ_FP8, N, K, (int)nb, dtype, epilogue, has_norm != 0, plan), plan, rows,
                             max_rows);
}

extern "C" int ss_gemv_mx4(const void* codes, const void* scales, const void* x, void* y, int64_t N, int64_t K, int64_t nb,
                           const void* norm_w, float eps, const void* bias, const void* residual, int epilogue, int dtype, void* stream) {
    SS_REQUIRE(nb >= 1 && nb <= 16, "gemv_mx4: batch %lld unsupported (1..16)", (long long)nb);
    return ss::gemv_wq_batched_dev(ss::GEMV_WQ_MXFP4, codes, scales, x, y, N, K, norm_w, eps, bias, residual, epilogue, nullptr, 0, (int)nb, K, N,
                                   N, dtype, (hipStream_t)stream);
}

extern "C" int ss_gemv_mx4_plan(int64_t N, int64_t K, int64_t nb, int dtype, int epilogue, int has_norm, int32_t* rows, int64_t max_rows) {
    ss::GemvPlan plan;
    SS_REQUIRE(nb >= 1 && nb <= 16, "gemv_mx4: batch %lld unsupported (1..16)", (long long)nb);
    return ss::gemv_plan_out("ss_gemv_mx4_plan", ss::gemv_wq_plan(ss::GEMV_WQ_MXFP4, N, K, (int)nb, dtype, epilogue, has_norm != 0, plan), plan, rows,
                             max_rows);
}
