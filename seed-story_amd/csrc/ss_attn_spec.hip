// Decode attention of a speculative step (include/seedstory_hip.h, ss_attn_decode_spec): R <= 8 query rows of ONE slot at
// consecutive cache / RoPE positions, row r attending keys [0, L + r].
//
// attn_decode_kernel's layout (ss_attn.hip): grid (n_heads, nsplit), 256 threads; thread t works for key group kg = t / LPK (LPK =
// hd / V lanes share a key, each holding V consecutive d) and streams keys kg, kg + NKG, ... of its block's chunk, four keys per
// thread in flight, no barrier in the key loop.  What is new: every thread holds the packed q vectors and the private online
// softmax (m, l, acc[V]) of ALL rows, so a 16-byte K or V packet of the old cache is loaded once and used by every row — R
// launches of the q_len = 1 kernel would read the cache R times (and race on the new rows).
//
// The A new positions L .. L + A - 1 are never read back from global memory: the block whose chunk holds position L + j rotates
// k row j (and takes v row j) from the qkv rows in registers, the key group that owns the position stores both into the cache
// (the bits rope_kv_append and the fused decode kernel store) and feeds them to rows j .. A - 1.  The chunks cover [0, L + A).
// Partial records: attn_decode_kernel's [m, l, o[hd]] per (head, split), one workspace slab per row; the NKG groups of a block are
// merged through LDS one row after the other (the merge area stays that of the q_len = 1 kernel).
#include <math.h>

#include "ss_common.h"

namespace ss {

int decode_nsplit(int nb);

struct SpecAttnArgs {
    const void* qkv;            // [R][3 * E] pre-RoPE q | k | v
    void *kc, *vc;              // cache planes [n_heads, cap, hd]
    const void *cos_t, *sin_t;
    float* part;                // [R] slabs of part_stride floats
    void* out;                  // [R][E]
    const int32_t *kv_len_dev, *pos_dev, *n_active_dev;
    int rows, hd, n_heads, cap, nsplit;
    float scale;
    int64_t part_stride;
};

// active rows of a step: the device count, clipped to the launch's rows and to the cache rows that are left
__device__ __forceinline__ int spec_active_rows(const SpecAttnArgs& a, int L) {
    int A = *a.n_active_dev;
    A = A < a.rows ? A : a.rows;
    A = A < a.cap - L ? A : a.cap - L;
    return A;
}

template <typename T, int RR>
__global__ __launch_bounds__(256) void attn_decode_spec_kernel(const SpecAttnArgs a) {
    constexpr int V = Tr<T>::kVec;
    constexpr int KPT = 4;      // keys per thread per sub-chunk
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* sm = reinterpret_cast<float*>(smem_raw);     // [NKG][hd + 2]
    const int L = *a.kv_len_dev;
    const int A = spec_active_rows(a, L);
    if (A <= 0 || L < 0) return;
    const int h = blockIdx.x, sp = blockIdx.y, tid = threadIdx.x;
    const int hd = a.hd;
    const int LPK = hd / V, NKG = 256 / LPK;
    const int kg = tid / LPK, dl = tid % LPK, d0 = dl * V;
    const int kv_tot = L + A;
    const int chunk = (kv_tot + a.nsplit - 1) / a.nsplit;
    const int k_lo = sp * chunk;
    const int k_hi = min(kv_tot, k_lo + chunk);
    const int o_hi = min(k_hi, L);                      // the old keys of this chunk: [k_lo, o_hi), seen by every row
    const T* kh = (const T*)a.kc + (int64_t)h * a.cap * hd;
    const T* vh = (const T*)a.vc + (int64_t)h * a.cap * hd;
    const int E = a.n_heads * hd;
    const T* raw = (const T*)a.qkv;
    const int pos = *a.pos_dev;

    auto load_kv = [&](int base, uint4 (&kk)[KPT], uint4 (&vv)[KPT]) {
#pragma unroll
        for (int i = 0; i < KPT; ++i) {
            const int key = base + i * NKG;
            if (key < o_hi) {
                kk[i] = ld16(kh + (int64_t)key * hd + d0);
                vv[i] = ld16(vh + (int64_t)key * hd + d0);
            } else {
                kk[i] = make_uint4(0, 0, 0, 0);
                vv[i] = make_uint4(0, 0, 0, 0);
            }
        }
    };
    uint4 kk[KPT], vv[KPT];
    int base = k_lo + kg;
    if (base < o_hi) load_kv(base, kk, vv);             // in flight under the q RoPE below

    uint4 qv[RR];
    float m[RR], l[RR], acc[RR][V];
#pragma unroll
    for (int r = 0; r < RR; ++r) {
        qv[r] = r < A ? rope_pack<T>(raw + (int64_t)r * 3 * E + (int64_t)h * hd, (const T*)a.cos_t, (const T*)a.sin_t, pos + r, hd, d0)
                      : make_uint4(0, 0, 0, 0);
        m[r] = -1e30f;
        l[r] = 0.f;
#pragma unroll
        for (int j = 0; j < V; ++j) acc[r][j] = 0.f;
    }
    // one key for one row: the online-softmax update of attn_decode_kernel
    auto update = [&](int r, const uint4& kx, const float (&vf)[V], bool live) {
        float s = dot_pack<T>(kx, qv[r], 0.f);
        for (int o = LPK >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (live) {             // uniform within the LPK-lane key group
            s *= a.scale;
            const float mn = fmaxf(m[r], s);
            const float al = expf(m[r] - mn), p = expf(s - mn);
            l[r] = l[r] * al + p;
#pragma unroll
            for (int j = 0; j < V; ++j) acc[r][j] = fmaf(p, vf[j], acc[r][j] * al);
            m[r] = mn;
        }
    };

    // ---- the old keys: every row sees every one of them ------------------------------------------------------------------------
    while (base < o_hi) {
#pragma unroll
        for (int i = 0; i < KPT; ++i) {
            const int key = base + i * NKG;
            float vf[V];
            unpack<T>(vv[i], vf);
#pragma unroll
            for (int r = 0; r < RR; ++r)
                if (r < A) update(r, kk[i], vf, key < o_hi);
        }
        base += NKG * KPT;
        if (base < o_hi) load_kv(base, kk, vv);
    }
    // ---- the new keys: position L + j from row j's registers, seen by rows j .. A - 1 ------------------------------------------
#pragma unroll
    for (int j = 0; j < RR; ++j) {
        const int key = L + j;
        if (j < A && key >= k_lo && key < k_hi) {       // (uniform over the block) this block owns the position
            const bool mine = kg == (key - k_lo) % NKG; // (uniform over the key group)
            const T* row = raw + (int64_t)j * 3 * E + (int64_t)h * hd;
            const uint4 knew = rope_pack<T>(row + E, (const T*)a.cos_t, (const T*)a.sin_t, pos + j, hd, d0);
            const uint4 vnew = ld16(row + 2 * E + d0);
            if (mine && key < a.cap) {
                st16((T*)a.kc + ((int64_t)h * a.cap + key) * hd + d0, knew);
                st16((T*)a.vc + ((int64_t)h * a.cap + key) * hd + d0, vnew);
            }
            float vf[V];
            unpack<T>(vnew, vf);
#pragma unroll
            for (int r = j; r < RR; ++r)
                if (r < A) update(r, knew, vf, mine);
        }
    }
    // ---- merge the NKG private softmaxes, one row after the other ---------------------------------------------------------------
    float* mine_rec = sm + kg * (hd + 2);
#pragma unroll
    for (int r = 0; r < RR; ++r) {
        if (r >= A) break;      // (uniform over the block)
        if (r) __syncthreads();
        if (dl == 0) { mine_rec[0] = m[r]; mine_rec[1] = l[r]; }
#pragma unroll
        for (int j = 0; j < V; ++j) mine_rec[2 + d0 + j] = acc[r][j];
        __syncthreads();
        float* rec = a.part + r * a.part_stride + ((int64_t)h * a.nsplit + sp) * (hd + 2);
        if (tid < hd) {
            float mm = -1e30f;
            for (int g = 0; g < NKG; ++g) mm = fmaxf(mm, sm[g * (hd + 2)]);
            float lt = 0.f, ot = 0.f;
            for (int g = 0; g < NKG; ++g) {
                const float* q = sm + g * (hd + 2);
                const float w = q[1] > 0.f ? expf(q[0] - mm) : 0.f;
                lt = fmaf(w, q[1], lt);
                ot = fmaf(w, q[2 + tid], ot);
            }
            rec[2 + tid] = ot;
            if (tid == 0) { rec[0] = mm; rec[1] = lt; }
        }
    }
}

// attn_combine_kernel's merge of the splits (the same order of sums), for the rows the step uses: grid (n_heads, R), hd threads
template <typename T>
__global__ void attn_combine_spec_kernel(const SpecAttnArgs a) {
    const int r = blockIdx.y;
    const int L = *a.kv_len_dev;
    if (L < 0 || r >= spec_active_rows(a, L)) return;
    const int h = blockIdx.x, d = threadIdx.x, hd = a.hd, ns = a.nsplit;
    const float* rec = a.part + r * a.part_stride + (int64_t)h * ns * (hd + 2);
    float m = -1e30f;
    for (int s = 0; s < ns; ++s) m = fmaxf(m, rec[s * (hd + 2)]);
    float l = 0.f, o = 0.f;
    for (int s = 0; s < ns; ++s) {
        const float ls = rec[s * (hd + 2) + 1];
        const float w = ls > 0.f ? expf(rec[s * (hd + 2)] - m) : 0.f;
        l = fmaf(w, ls, l);
        o = fmaf(w, rec[s * (hd + 2) + 2 + d], o);
    }
    Tr<T>::st((T*)a.out + (int64_t)r * a.n_heads * hd + (int64_t)h * hd + d, o / l);
}

template <typename T>
static int attn_decode_spec_launch(SpecAttnArgs a, hipStream_t s) {
    constexpr int V = Tr<T>::kVec;
    const int hd = a.hd;
    SS_REQUIRE(hd % V == 0 && 256 % (hd / V) == 0 && 64 % (hd / V) == 0 && hd <= 256, "attn_decode_spec: head_dim %d unsupported", hd);
    a.nsplit = decode_nsplit(1);
    a.scale = 1.0f / sqrtf((float)hd);
    const int NKG = 256 / (hd / V);
    const size_t lds = (size_t)NKG * (hd + 2) * sizeof(float);
    const dim3 grid((unsigned)a.n_heads, (unsigned)a.nsplit);
    if (a.rows <= 2) hipLaunchKernelGGL((attn_decode_spec_kernel<T, 2>), grid, dim3(256), lds, s, a);
    else if (a.rows <= 4) hipLaunchKernelGGL((attn_decode_spec_kernel<T, 4>), grid, dim3(256), lds, s, a);
    else hipLaunchKernelGGL((attn_decode_spec_kernel<T, 8>), grid, dim3(256), lds, s, a);
    SS_LAUNCH_CHECK("attn_decode_spec");
    hipLaunchKernelGGL(attn_combine_spec_kernel<T>, dim3((unsigned)a.n_heads, (unsigned)a.rows), dim3((unsigned)hd), 0, s, a);
    SS_LAUNCH_CHECK("attn_combine_spec");
    return SS_OK;
}

int attn_decode_spec_dev(const void* qkv, void* kc, void* vc, const void* cos_t, const void* sin_t, void* out, void* ws,
                         const int32_t* kv_len_dev, const int32_t* pos_dev, const int32_t* n_active_dev, int rows, int64_t n_heads,
                         int64_t hd, int64_t cache_cap, int dtype, hipStream_t s) {
    SpecAttnArgs a;
    a.qkv = qkv; a.kc = kc; a.vc = vc; a.cos_t = cos_t; a.sin_t = sin_t; a.part = (float*)ws; a.out = out;
    a.kv_len_dev = kv_len_dev; a.pos_dev = pos_dev; a.n_active_dev = n_active_dev;
    a.rows = rows; a.hd = (int)hd; a.n_heads = (int)n_heads; a.cap = (int)cache_cap; a.nsplit = 0; a.scale = 0.f;
    a.part_stride = (int64_t)(ss_attn_decode_workspace_bytes(n_heads, hd) / sizeof(float));
    return SS_DISPATCH(dtype, attn_decode_spec_launch, a, s);
}

}  // namespace ss

using namespace ss;

extern "C" int ss_attn_decode_spec(const void* qkv, void* kcache, void* vcache, const void* cos, const void* sin, void* out,
                                   void* workspace, const int32_t* kv_len_dev, const int32_t* pos_dev, const int32_t* n_active_dev,
                                   int64_t rows, int64_t n_heads, int64_t hd, int64_t cache_cap, int dtype, void* stream) {
    SS_REQUIRE(qkv && kcache && vcache && cos && sin && out && workspace && kv_len_dev && pos_dev && n_active_dev,
               "attn_decode_spec: null argument");
    SS_REQUIRE(rows >= 1 && rows <= SS_SPEC_MAX_ROWS && n_heads > 0 && hd > 0 && cache_cap > 0,
               "attn_decode_spec: bad shape (rows=%lld outside [1, %d], n_heads=%lld hd=%lld cache_cap=%lld)", (long long)rows,
               SS_SPEC_MAX_ROWS, (long long)n_heads, (long long)hd, (long long)cache_cap);
    return attn_decode_spec_dev(qkv, kcache, vcache, cos, sin, out, workspace, kv_len_dev, pos_dev, n_active_dev, (int)rows, n_heads,
                                hd, cache_cap, dtype, (hipStream_t)stream);
}
