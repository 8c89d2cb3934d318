// Decode attention (q_len = 1) over an fp8 (OCP e4m3fn) SHADOW of the KV cache, and the quantiser that fills the shadow.
//
// The 16-bit cache stays the truth (prefill, the image-token block, past_key_values, the sink gather and the attention-map
// capture read and write it unchanged); the decode token of an engine with ss_llama_set_kv8 on reads codes + one fp32
// power-of-two scale per (head, position) instead: 1 byte per element + 4 bytes per row in place of 2 bytes per element.
//
//  * kv8_quantize_kernel: rows of 16-bit planes -> codes + scales (definition: include/seedstory_hip.h, ss_kv_quantize_fp8).
//    hd / 16 lanes share a row, each holding 16 consecutive d: two 16-byte loads, one 16-byte store of codes.
//  * attn_decode_kv8_kernel: attn_decode_kernel (ss_attn.hip) with that lane layout: hd / 16 lanes per key (NKG = 4096 / hd key
//    groups per block, 16 accumulator elements per lane), a private online softmax per key group (merged by shuffles inside a
//    wave, then over the 4 waves through LDS), the same partial records, so attn_combine_kernel merges the splits as it is.  fp32 throughout:  s = (q . codes) * kscale[key] / sqrt(hd),
//    acc += p * vscale[key] * codes.  Fused form: q and the new k are rotated as in attn_decode_kernel, the block that owns
//    position kv_len appends the 16-bit row as attn_decode_kernel does AND its shadow row, quantised by the very function the
//    quantiser runs (bit-identical); the new token's own k / v come from registers, unquantised.
//  * positions >= kv_len are never read, neither codes nor scales.
#include "ss_kv8.h"

namespace ss {

int decode_nsplit(int nb);      // ss_attn.hip
int decode_step_check(const char* who, const void* qkv, const void* kcache, const void* vcache, const void* cos, const void* sin,
                      const void* out, const void* workspace, const int32_t* state, int64_t kv_len_word, int64_t pos_word,
                      int64_t state_stride, int64_t nb, int64_t n_heads, int64_t hd, int64_t cache_cap, int64_t cache_stride);
int attn_combine_dev(const float* part, void* out, const int32_t* done_flag, int64_t n_heads, int64_t hd, int nb, int nsplit,
                     int state_stride, int64_t part_stride, int64_t out_stride, int dtype, hipStream_t s);

constexpr int kKv8E = 16;       // codes per lane = one 16-byte load

// ---- the quantisation: ONE definition for every writer of the shadow ---------------------------------------------------------
// amax = m * 2^t, m in [0.5, 1): scale = 2^e with the smallest e such that amax <= 448 * 2^e (448 = 0.875 * 2^9), e >= -126;
// amax == 0: scale 1.  (A non-finite amax is outside the definition: any scale, no fault.)
__device__ __forceinline__ void kv8_scale(float amax, float& scale, float& inv) {
    int t = 0;
    const float m = frexpf(amax, &t);
    int e = m <= 0.875f ? t - 9 : t - 8;
    e = e < -126 ? -126 : e > 126 ? 126 : e;
    if (!(amax > 0.f)) e = 0;
    scale = ldexpf(1.0f, e);
    inv = ldexpf(1.0f, -e);
}

// the 16 values [d0, d0 + 16) of one row, held by one of the LPK lanes that share the row -> their codes + the row's scale.
// x * 2^-e is exact in fp32 and at most 448 in magnitude: the conversion rounds to nearest even and never saturates.
template <typename T>
__device__ __forceinline__ uint4 kv8_quant16(const uint4& lo, const uint4& hi, int LPK, float& scale) {
    float x[kKv8E];
    unpack<T>(lo, x);
    unpack<T>(hi, x + 8);
    float amax = 0.f;
#pragma unroll
    for (int j = 0; j < kKv8E; ++j) amax = fmaxf(amax, fabsf(x[j]));
    for (int o = LPK >> 1; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
    float inv;
    kv8_scale(amax, scale, inv);
    uint32_t w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int c = 0;
        c = __builtin_amdgcn_cvt_pk_fp8_f32(x[4 * i] * inv, x[4 * i + 1] * inv, c, false);
        c = __builtin_amdgcn_cvt_pk_fp8_f32(x[4 * i + 2] * inv, x[4 * i + 3] * inv, c, true);
        w[i] = (uint32_t)c;
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// 16 codes -> fp32 (exact)
__device__ __forceinline__ void kv8_dec16(const uint4& c, float* f) {
    typedef __attribute__((ext_vector_type(2))) float f32x2_t;
    const uint32_t w[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const f32x2_t a = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], false);
        const f32x2_t b = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], true);
        f[4 * i] = a.x; f[4 * i + 1] = a.y; f[4 * i + 2] = b.x; f[4 * i + 3] = b.y;
    }
}

// grid (row pieces, 2 * n_layers, slots), 256 threads; thread = one 16-element piece of one row (the LPK lanes of a row are
// consecutive lanes of one wave and run the loop together: the piece count is a multiple of LPK, the stride a multiple of 256)
template <typename T>
__global__ __launch_bounds__(256) void kv8_quantize_kernel(const Kv8QuantArgs a) {
    const int b = blockIdx.z, layer = blockIdx.y >> 1;
    const bool is_v = blockIdx.y & 1;
    const int lo = a.lo[b], n = a.hi[b] - lo;
    if (n <= 0) return;
    const int hd = a.hd, LPK = hd / kKv8E;
    const int64_t off = (int64_t)b * a.slot_stride + (int64_t)layer * a.heads * a.cap * hd;
    const T* src = (const T*)(is_v ? a.v : a.k) + off;
    uint8_t* dq = (is_v ? a.vq : a.kq) + off;
    float* ds = (is_v ? a.vs : a.ks) + off / hd;
    const int64_t total = (int64_t)a.heads * n * LPK;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int dl = (int)(i % LPK);
        const int64_t r = i / LPK;
        const int64_t row = (r / n) * a.cap + lo + r % n;       // [head][position]
        const T* p = src + row * hd + dl * kKv8E;
        float sc;
        const uint4 c = kv8_quant16<T>(ld16(p), ld16(p + 8), LPK, sc);
        st16(dq + row * hd + dl * kKv8E, c);
        if (dl == 0) ds[row] = sc;
    }
}

struct Kv8DecodeArgs {
    const void* q;        // rotated q [n_heads*hd]            (plain mode)
    const void* qkv_raw;  // [3*n_heads*hd] pre-RoPE q|k|v      (fused mode) or NULL
    void *kc, *vc;        // 16-bit cache planes [n_heads, cap, hd]: the fused append only
    uint8_t *kq, *vq;     // code planes [n_heads, cap, hd]
    float *ks, *vs;       // scale planes [n_heads, cap]
    const void *cos_t, *sin_t;
    float* part;
    const int32_t* kv_len_dev;
    const int32_t* pos_dev;
    const int32_t* done_flag;
    int hd, n_heads, cap, nsplit;
    float scale;
    int nb, state_stride;
    int64_t q_stride, cache_stride, part_stride, out_stride;     // cache_stride: elements = code bytes; scales: / hd
};

template <typename T>
__global__ __launch_bounds__(256) void attn_decode_kv8_kernel(const Kv8DecodeArgs a0) {
    Kv8DecodeArgs a = a0;
    {   // select this block's sequence
        const int b = blockIdx.z;
        const int64_t so = (int64_t)b * a.state_stride;
        if (a.done_flag) a.done_flag += so;
        a.kv_len_dev += so;
        if (a.pos_dev) a.pos_dev += so;
        if (a.q) a.q = (const T*)a.q + b * a.q_stride;
        if (a.qkv_raw) a.qkv_raw = (const T*)a.qkv_raw + b * a.q_stride;
        if (a.kc) a.kc = (T*)a.kc + b * a.cache_stride;
        if (a.vc) a.vc = (T*)a.vc + b * a.cache_stride;
        a.kq += b * a.cache_stride;
        a.vq += b * a.cache_stride;
        a.ks += b * (a.cache_stride / a.hd);
        a.vs += b * (a.cache_stride / a.hd);
        a.part += b * a.part_stride;
    }
    constexpr int E = kKv8E;
    constexpr int KPT = 4;  // keys per thread per sub-chunk
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* sm = reinterpret_cast<float*>(smem_raw);  // [4 waves][hd + 2]
    if (a.done_flag && *a.done_flag) return;
    const int h = blockIdx.x, sp = blockIdx.y, tid = threadIdx.x;
    const int hd = a.hd;
    const int LPK = hd / E, NKG = 256 / LPK;
    const int kg = tid / LPK, dl = tid % LPK, d0 = dl * E;
    const bool fused = a.qkv_raw != nullptr;
    const int n_old = *a.kv_len_dev;
    const int kv_len = n_old + (fused ? 1 : 0);
    const int chunk = (kv_len + a.nsplit - 1) / a.nsplit;
    const int k_lo = sp * chunk;
    const int k_hi = min(kv_len, k_lo + chunk);
    const uint8_t* kh = a.kq + (int64_t)h * a.cap * hd;
    const uint8_t* vh = a.vq + (int64_t)h * a.cap * hd;
    const float* ksh = a.ks + (int64_t)h * a.cap;
    const float* vsh = a.vs + (int64_t)h * a.cap;
    const int EH = a.n_heads * hd;

    // as in attn_decode_kernel: the first sub-chunk is requested before the q / k RoPE arithmetic
    auto load_kv = [&](int base, uint4 (&kk)[KPT], uint4 (&vv)[KPT], float (&sk)[KPT], float (&sv)[KPT]) {
#pragma unroll
        for (int i = 0; i < KPT; ++i) {
            const int key = base + i * NKG;
            if (key < k_hi && !(fused && key == n_old)) {
                kk[i] = ld16(kh + (int64_t)key * hd + d0);
                vv[i] = ld16(vh + (int64_t)key * hd + d0);
                sk[i] = ksh[key];
                sv[i] = vsh[key];
            } else {
                kk[i] = make_uint4(0, 0, 0, 0);
                vv[i] = make_uint4(0, 0, 0, 0);
                sk[i] = 0.f;
                sv[i] = 0.f;
            }
        }
    };
    uint4 kk[KPT], vv[KPT];
    float sk[KPT], sv[KPT];
    int base = k_lo + kg;
    if (base < k_hi) load_kv(base, kk, vv, sk, sv);

    float qf[E];
    uint4 knew[2] = {make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0)}, vnew[2] = {make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0)};
    bool owns_new = false;
    if (fused) {
        const T* raw = (const T*)a.qkv_raw;
        const T *cs = (const T*)a.cos_t, *sn = (const T*)a.sin_t;
        const int pos = *a.pos_dev;
        unpack<T>(rope_pack<T>(raw + (int64_t)h * hd, cs, sn, pos, hd, d0), qf);
        unpack<T>(rope_pack<T>(raw + (int64_t)h * hd, cs, sn, pos, hd, d0 + 8), qf + 8);
        owns_new = n_old >= k_lo && n_old < k_hi;
        if (owns_new) {  // this block owns the new position (uniform over the block)
            knew[0] = rope_pack<T>(raw + EH + (int64_t)h * hd, cs, sn, pos, hd, d0);
            knew[1] = rope_pack<T>(raw + EH + (int64_t)h * hd, cs, sn, pos, hd, d0 + 8);
            vnew[0] = ld16(raw + 2 * EH + (int64_t)h * hd + d0);
            vnew[1] = ld16(raw + 2 * EH + (int64_t)h * hd + d0 + 8);
            float ksc, vsc;     // every key group quantises (the row maximum is taken over the lanes that share the key)
            const uint4 kc8 = kv8_quant16<T>(knew[0], knew[1], LPK, ksc);
            const uint4 vc8 = kv8_quant16<T>(vnew[0], vnew[1], LPK, vsc);
            if (kg == (n_old - k_lo) % NKG && n_old < a.cap) {
                const int64_t row = (int64_t)h * a.cap + n_old;
                st16((T*)a.kc + row * hd + d0, knew[0]);
                st16((T*)a.kc + row * hd + d0 + 8, knew[1]);
                st16((T*)a.vc + row * hd + d0, vnew[0]);
                st16((T*)a.vc + row * hd + d0 + 8, vnew[1]);
                st16(a.kq + row * hd + d0, kc8);
                st16(a.vq + row * hd + d0, vc8);
                if (dl == 0) { a.ks[row] = ksc; a.vs[row] = vsc; }
            }
        }
    } else {
        unpack<T>(ld16((const T*)a.q + (int64_t)h * hd + d0), qf);
        unpack<T>(ld16((const T*)a.q + (int64_t)h * hd + d0 + 8), qf + 8);
    }

    float m = -1e30f, l = 0.f, acc[E];
#pragma unroll
    for (int j = 0; j < E; ++j) acc[j] = 0.f;
    // one key into the group's private softmax: k / v as 16 fp32 values per lane and the two row scales
    auto step = [&](const float (&kf)[E], const float (&vf)[E], float ksc, float vsc) {
        float s4[4] = {0.f, 0.f, 0.f, 0.f};     // four short chains instead of one of 16 dependent FMAs
#pragma unroll
        for (int j = 0; j < E; ++j) s4[j & 3] = fmaf(kf[j], qf[j], s4[j & 3]);
        float s = (s4[0] + s4[1]) + (s4[2] + s4[3]);
        for (int o = LPK >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        s = s * ksc * a.scale;
        const float mn = fmaxf(m, s);
        const float al = expf(m - mn), p = expf(s - mn);
        l = l * al + p;
        const float pv = p * vsc;
#pragma unroll
        for (int j = 0; j < E; ++j) acc[j] = fmaf(pv, vf[j], acc[j] * al);
        m = mn;
    };
    while (base < k_hi) {
#pragma unroll
        for (int i = 0; i < KPT; ++i) {
            const int key = base + i * NKG;
            if (key < k_hi && !(fused && key == n_old)) {  // uniform within the LPK-lane key group; the new key: below
                float kf[E], vf[E];
                kv8_dec16(kk[i], kf);
                kv8_dec16(vv[i], vf);
                step(kf, vf, sk[i], sv[i]);
            }
        }
        base += NKG * KPT;
        if (base < k_hi) load_kv(base, kk, vv, sk, sv);
    }
    if (owns_new && kg == (n_old - k_lo) % NKG) {   // the new token's own k / v: from registers, unquantised
        float kf[E], vf[E];
        unpack<T>(knew[0], kf); unpack<T>(knew[1], kf + 8);
        unpack<T>(vnew[0], vf); unpack<T>(vnew[1], vf + 8);
        step(kf, vf, 1.f, 1.f);
    }
    // ---- merge the NKG private softmaxes (the partial record of attn_decode_kernel) ------------------------------------------
    // first inside each wave, in registers: lanes l and l ^ o (o = LPK, 2 LPK, ... 32) hold the same d of two key groups, so
    // log2(64 / LPK) butterfly steps leave every lane with its wave's merged (m, l, acc) — 4 records go through LDS, not NKG
    for (int o = LPK; o < 64; o <<= 1) {
        const float m2 = __shfl_xor(m, o, 64), l2 = __shfl_xor(l, o, 64);
        const float mn = fmaxf(m, m2);
        const float w1 = expf(m - mn), w2 = expf(m2 - mn);     // an empty group has m = -1e30, l = 0, acc = 0: weight 0 or 1
        l = fmaf(l2, w2, l * w1);
#pragma unroll
        for (int j = 0; j < E; ++j) acc[j] = fmaf(__shfl_xor(acc[j], o, 64), w2, acc[j] * w1);
        m = mn;
    }
    constexpr int NW = 4;       // waves per block
    const int wave = tid >> 6;
    if ((tid & 63) < LPK) {
        float* mine = sm + wave * (hd + 2);
        if (dl == 0) { mine[0] = m; mine[1] = l; }
#pragma unroll
        for (int j = 0; j < E; ++j) mine[2 + d0 + j] = acc[j];
    }
    __syncthreads();
    float* rec = a.part + ((int64_t)h * a.nsplit + sp) * (hd + 2);
    if (tid < hd) {
        float mw[NW], lw[NW], ow[NW];
#pragma unroll
        for (int g = 0; g < NW; ++g) { mw[g] = sm[g * (hd + 2)]; lw[g] = sm[g * (hd + 2) + 1]; ow[g] = sm[g * (hd + 2) + 2 + tid]; }
        float mm = -1e30f;
#pragma unroll
        for (int g = 0; g < NW; ++g) mm = fmaxf(mm, mw[g]);
        float lt = 0.f, ot = 0.f;
#pragma unroll
        for (int g = 0; g < NW; ++g) {
            const float w = lw[g] > 0.f ? expf(mw[g] - mm) : 0.f;
            lt = fmaf(w, lw[g], lt);
            ot = fmaf(w, ow[g], ot);
        }
        rec[2 + tid] = ot;
        if (tid == 0) { rec[0] = mm; rec[1] = lt; }
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
int kv8_check(int64_t hd, int dtype, const char* who) {
    SS_REQUIRE(dtype == SS_BF16 || dtype == SS_F16, "%s: the fp8 KV shadow needs a bf16 or fp16 cache (dtype %d)", who, dtype);
    SS_REQUIRE(hd > 0 && hd % kKv8E == 0 && hd <= 256 && 64 % (hd / kKv8E) == 0,
               "%s: head_dim %lld unsupported (a multiple of 16, at most 256, head_dim / 16 a power of two)", who, (long long)hd);
    return SS_OK;
}

template <typename T>
static int kv8_quantize_launch(const Kv8QuantArgs& a, hipStream_t s) {
    int n_max = 0;
    for (int b = 0; b < a.nb; ++b) n_max = a.hi[b] - a.lo[b] > n_max ? a.hi[b] - a.lo[b] : n_max;
    if (n_max <= 0) return SS_OK;
    int blocks = cdiv((int64_t)a.heads * n_max * (a.hd / kKv8E), 256);
    blocks = blocks > 1024 ? 1024 : blocks;
    hipLaunchKernelGGL(kv8_quantize_kernel<T>, dim3((unsigned)blocks, (unsigned)(2 * a.n_layers), (unsigned)a.nb), dim3(256), 0, s, a);
    SS_LAUNCH_CHECK("kv8_quantize");
    return SS_OK;
}
template <> int kv8_quantize_launch<float>(const Kv8QuantArgs&, hipStream_t) { return SS_EINVAL; }     // (kv8_check refuses fp32)

int kv8_quantize_dev(const Kv8QuantArgs& a, int dtype, hipStream_t s) {
    if (int rc = kv8_check(a.hd, dtype, "kv_quantize_fp8")) return rc;
    SS_REQUIRE(a.nb >= 1 && a.nb <= 8 && a.n_layers >= 1 && a.heads >= 1 && a.cap >= 1, "kv_quantize_fp8: bad shape");
    for (int b = 0; b < a.nb; ++b)
        SS_REQUIRE(a.lo[b] >= 0 && a.hi[b] <= a.cap, "kv_quantize_fp8: rows [%d, %d) outside the cache (%d positions)", a.lo[b],
                   a.hi[b], a.cap);
    return SS_DISPATCH(dtype, kv8_quantize_launch, a, s);
}

template <typename T>
static int attn_decode_kv8_launch(const Kv8DecodeArgs& a0, void* out, hipStream_t s) {
    Kv8DecodeArgs a = a0;
    if (a.nb < 1) a.nb = 1;
    a.nsplit = decode_nsplit(a.nb);
    a.scale = 1.0f / sqrtf((float)a.hd);
    const size_t lds = (size_t)4 * (a.hd + 2) * sizeof(float);        // one merged record per wave
    hipLaunchKernelGGL(attn_decode_kv8_kernel<T>, dim3((unsigned)a.n_heads, (unsigned)a.nsplit, (unsigned)a.nb), dim3(256), lds, s, a);
    SS_LAUNCH_CHECK("attn_decode_kv8");
    return attn_combine_dev(a.part, out, a.done_flag, a.n_heads, a.hd, a.nb, a.nsplit, a.state_stride, a.part_stride, a.out_stride,
                            Tr<T>::kDtype, s);
}
template <> int attn_decode_kv8_launch<float>(const Kv8DecodeArgs&, void*, hipStream_t) { return SS_EINVAL; }

static Kv8DecodeArgs kv8_args(const void* q, const void* qkv_raw, void* kc, void* vc, const void* kq, const void* vq, const float* ks,
                              const float* vs, const void* cos_t, const void* sin_t, void* ws, const int32_t* kv_len_dev,
                              const int32_t* pos_dev, const int32_t* done_flag, int64_t n_heads, int64_t hd, int64_t cache_cap) {
    Kv8DecodeArgs a;
    a.q = q; a.qkv_raw = qkv_raw; a.kc = kc; a.vc = vc; a.kq = (uint8_t*)kq; a.vq = (uint8_t*)vq; a.ks = (float*)ks; a.vs = (float*)vs;
    a.cos_t = cos_t; a.sin_t = sin_t; a.part = (float*)ws; a.kv_len_dev = kv_len_dev; a.pos_dev = pos_dev; a.done_flag = done_flag;
    a.hd = (int)hd; a.n_heads = (int)n_heads; a.cap = (int)cache_cap; a.nsplit = 0; a.scale = 0.f;
    a.nb = 1; a.state_stride = 0; a.q_stride = a.cache_stride = a.part_stride = a.out_stride = 0;
    return a;
}

int attn_decode_kv8_dev(const void* q, const void* kq, const void* vq, const float* ks, const float* vs, void* out, void* ws,
                        const int32_t* kv_len_dev, const int32_t* done_flag, int64_t n_heads, int64_t hd, int64_t cache_cap,
                        int dtype, hipStream_t s) {
    if (int rc = kv8_check(hd, dtype, "attn_decode_kv8")) return rc;
    const Kv8DecodeArgs a = kv8_args(q, nullptr, nullptr, nullptr, kq, vq, ks, vs, nullptr, nullptr, ws, kv_len_dev, nullptr, done_flag,
                                     n_heads, hd, cache_cap);
    return SS_DISPATCH(dtype, attn_decode_kv8_launch, a, out, s);
}

int attn_decode_kv8_fused_dev(const void* qkv_raw, void* kc, void* vc, void* kq, void* vq, float* ks, float* vs, const void* cos_t,
                              const void* sin_t, void* out, void* ws, const int32_t* kv_len_dev, const int32_t* pos_dev,
                              const int32_t* done_flag, int64_t n_heads, int64_t hd, int64_t cache_cap, int nb, int state_stride,
                              int64_t cache_stride, int dtype, hipStream_t s) {
    if (int rc = kv8_check(hd, dtype, "attn_decode_kv8")) return rc;
    Kv8DecodeArgs a = kv8_args(nullptr, qkv_raw, kc, vc, kq, vq, ks, vs, cos_t, sin_t, ws, kv_len_dev, pos_dev, done_flag, n_heads, hd,
                               cache_cap);
    a.nb = nb; a.state_stride = state_stride; a.q_stride = 3 * n_heads * hd; a.cache_stride = cache_stride;
    a.part_stride = (int64_t)(ss_attn_decode_workspace_bytes(n_heads, hd) / sizeof(float));
    a.out_stride = n_heads * hd;
    return SS_DISPATCH(dtype, attn_decode_kv8_launch, a, out, s);
}

}  // namespace ss

using namespace ss;

extern "C" {

int ss_kv_quantize_fp8(const void* k, const void* v, void* k_codes, void* v_codes, float* k_scale, float* v_scale, int64_t n_heads,
                       int64_t cache_cap, int64_t hd, int64_t lo, int64_t hi, int dtype, void* stream) {
    if (int rc = kv8_check(hd, dtype, "kv_quantize_fp8")) return rc;
    SS_REQUIRE(k && v && k_codes && v_codes && k_scale && v_scale, "kv_quantize_fp8: NULL plane");
    SS_REQUIRE((((size_t)k | (size_t)v | (size_t)k_codes | (size_t)v_codes) & 15) == 0 && (((size_t)k_scale | (size_t)v_scale) & 3) == 0,
               "kv_quantize_fp8: the planes must be 16-byte aligned (scales: 4)");
    SS_REQUIRE(n_heads >= 1 && cache_cap >= 1 && n_heads * cache_cap * hd < (1ll << 31) && lo >= 0 && lo <= hi && hi <= cache_cap,
               "kv_quantize_fp8: rows [%lld, %lld) of %lld heads x %lld positions", (long long)lo, (long long)hi, (long long)n_heads,
               (long long)cache_cap);
    Kv8QuantArgs a = {k, v, (uint8_t*)k_codes, (uint8_t*)v_codes, k_scale, v_scale, (int)n_heads, (int)cache_cap, (int)hd, 1, 1, 0, {(int)lo}, {(int)hi}};
    return kv8_quantize_dev(a, dtype, (hipStream_t)stream);
}

int ss_attn_decode_kv8(const void* q, const void* k_codes, const void* v_codes, const float* k_scale, const float* v_scale, void* out,
                       void* workspace, const int32_t* kv_len_dev, int64_t n_heads, int64_t hd, int64_t cache_cap, int dtype,
                       void* stream) {
    if (int rc = kv8_check(hd, dtype, "attn_decode_kv8")) return rc;
    SS_REQUIRE(q && k_codes && v_codes && k_scale && v_scale && out && workspace && kv_len_dev, "attn_decode_kv8: NULL argument");
    SS_REQUIRE((((size_t)q | (size_t)k_codes | (size_t)v_codes) & 15) == 0 && (((size_t)k_scale | (size_t)v_scale) & 3) == 0,
               "attn_decode_kv8: q and the code planes must be 16-byte aligned (scales: 4)");
    SS_REQUIRE(n_heads >= 1 && cache_cap >= 1, "attn_decode_kv8: bad shape");
    return attn_decode_kv8_dev(q, k_codes, v_codes, k_scale, v_scale, out, workspace, kv_len_dev, nullptr, n_heads, hd, cache_cap, dtype,
                               (hipStream_t)stream);
}

int ss_attn_decode_kv8_step(const void* qkv, void* kcache, void* vcache, void* k_codes, void* v_codes, float* k_scale, float* v_scale,
                            const void* cos, const void* sin, void* out, void* workspace, const int32_t* state, int64_t kv_len_word,
                            int64_t pos_word, int64_t done_word, int64_t state_stride, int64_t nb, int64_t n_heads, int64_t hd,
                            int64_t cache_cap, int64_t cache_stride, int dtype, void* stream) {
    if (int rc = kv8_check(hd, dtype, "attn_decode_kv8_step")) return rc;
    if (int rc = decode_step_check("attn_decode_kv8_step", qkv, kcache, vcache, cos, sin, out, workspace, state, kv_len_word, pos_word,
                                   state_stride, nb, n_heads, hd, cache_cap, cache_stride))
        return rc;
    SS_REQUIRE(k_codes && v_codes && k_scale && v_scale, "attn_decode_kv8_step: NULL shadow plane");
    SS_REQUIRE((((size_t)k_codes | (size_t)v_codes) & 15) == 0 && (((size_t)k_scale | (size_t)v_scale) & 3) == 0,
               "attn_decode_kv8_step: the code planes must be 16-byte aligned (scales: 4)");
    return attn_decode_kv8_fused_dev(qkv, kcache, vcache, k_codes, v_codes, k_scale, v_scale, cos, sin, out, workspace,
                                     state + kv_len_word, state + pos_word, done_word < 0 ? nullptr : state + done_word, n_heads, hd,
                                     cache_cap, (int)nb, (int)state_stride, cache_stride, dtype, (hipStream_t)stream);
}

}  // extern "C"
