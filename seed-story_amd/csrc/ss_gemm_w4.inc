// "One stream per SIMD" MFMA GEMM / implicit-GEMM 3x3 conv for 16-bit dtypes (K % 64 == 0; conv: Cin % 64 == 0).
// Included by ss_gemm_w4_{bf16,f16}[_conv].hip with SS_W4_T (element type) and SS_W4_CONV (0 | 1) defined.
//
// Why a second kernel family next to ss_gemm_sp.inc (8 waves, 16x16x32 fragments, two waves per SIMD): that structure
// tops out at ~1.23-1.31 PFLOP/s at 4096^3 / 8192^3 (1.64 us per 256x256x64 K tile against 0.86 us of MFMA time) because
// its eight waves reach the tile's one barrier together and then ALL issue their share of the next tile's LDS-DMA at
// the same moment (64 pieces x ~16 cycles of the CU's one texture-address path), a stretch in which no wave feeds the
// matrix cores; and both waves of a SIMD run the same phase, so neither covers the other.  Here:
//   * 4 waves per workgroup, ONE per SIMD, 512 registers each: the 128x128 wave tile's 256 accumulators live in the
//     AGPR half of the register file ("+a" operands of accumulate-in-place asm MFMAs), the VGPR half holds two sets of
//     operand fragments and the addresses.  A 256x256 tile then reads 128 KB of LDS per K tile instead of 192 KB (each
//     wave re-uses its fragments over a 4x4 grid of 32x32 blocks), and a barrier has 4 participants, not 8;
//   * v_mfma_f32_32x32x16_{bf16,f16}: 32 cycles of matrix pipe per instruction = 8 issue slots, half the operand
//     register reads per FLOP of the 16x16x32 form (the chip clocks by its power budget: MI355X_MICROARCH.md DVFS);
//   * the wave's stream is MFMA, filler, MFMA, filler, ...: the 8 ds_read_b128 of the NEXT k-step and this wave's
//     LDS-DMA pieces of the tile after next sit one per gap between the 16 MFMAs of a k-step, so the DMA never bursts
//     (4 waves x 1 piece per 64 cycles = the texture path's 64 B/clk) and no MFMA waits on an operand;
//   * ring of 2 K tiles (128 KB) + 32 KB of epilogue strips = the CU's 160 KB.  One barrier per K tile, after the MFMAs of
//     k-step 2: every wave has all its fragments of the tile in registers by then (the k-step 3 reads are issued in the first
//     gaps of k-step 2), so the slot is free for the tile after next and the next tile (DMA'd during the previous
//     k-step 3, this tile's k-steps 0 and 1) is visible for the k-step 0 reads that ride in k-step 3's gaps;
//   * persistent tiles in XCD-aware order: the next output tile's first two K tiles are DMA'd under the last k-step
//     and the epilogue; LDS-staged epilogue (32-row chunks through a private strip, whole-row 16-byte stores).
//
// LDS tile image: rows of 128 bytes (64 k), chunk c (16 B) of row r at physical chunk c ^ ((r >> 1) & 7): a
// ds_read_b128 of a 32-row operand fragment (lane l: row l & 31, k-group l >> 5) is served in the lane groups
// {0-3,12-15,20-27}, {4-11,16-19,28-31} (+32), whose 16 rows then hit 16 distinct (row parity, chunk) slots = all 64
// banks once.  As in ss_gemm_sp.inc the permutation is applied on the DMA SOURCE address (inside one 128-byte line).
// Operand roles as in ss_gemm_common.h: the MFMA "A" operand is the WEIGHT tile (rows -> n), "B" the ACTIVATION tile
// (columns -> m); accumulator register v of block (bn, bm) in lane l is  C[m = 32 bm + (l & 31)][n = 32 bn + 8 (v / 4)
// + 4 (l >> 5) + (v % 4)] : four consecutive n per register quad.

namespace ss {

typedef __attribute__((ext_vector_type(16))) float f32x16_t;

// compile-time loop: f(integral_constant<int, 0>) ... f(integral_constant<int, N-1>).  The accumulator blocks are 16-register
// tuples pinned to AGPRs: an index the optimiser fails to fold (a `#pragma unroll` it declines on a large body) would
// send the whole array to scratch, so every loop over them is unrolled by construction.
template <int... Is, typename F>
__device__ __forceinline__ void w4_static_for_impl(std::integer_sequence<int, Is...>, F&& f) {
    (f(std::integral_constant<int, Is>{}), ...);
}
template <int N, typename F>
__device__ __forceinline__ void w4_static_for(F&& f) {
    w4_static_for_impl(std::make_integer_sequence<int, N>{}, static_cast<F&&>(f));
}

// One lane's operand of a 32-row block: NV 16-byte pieces (1: 8 k of a 16-bit type, 2: 32 k of fp8)
template <int NV> struct W4Frag { uint4 v[NV]; };
template <typename T> struct Mma32;
template <> struct Mma32<bf16_t> {
    static constexpr int kEB = 2, kKS = 4, kNV = 1;       // bytes per element, k-steps per 128-byte K tile row, pieces per operand
    static __device__ __forceinline__ uint32_t make_aux() { return 0u; }
    static __device__ __forceinline__ void run(const W4Frag<1>& w, const W4Frag<1>& a, f32x16_t& c, uint32_t) {
        asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0"
                     : "+a"(c)
                     : "v"(__builtin_bit_cast(u32x4_t, w.v[0])), "v"(__builtin_bit_cast(u32x4_t, a.v[0])));
    }
};
template <> struct Mma32<f16_t> {
    static constexpr int kEB = 2, kKS = 4, kNV = 1;
    static __device__ __forceinline__ uint32_t make_aux() { return 0u; }
    static __device__ __forceinline__ void run(const W4Frag<1>& w, const W4Frag<1>& a, f32x16_t& c, uint32_t) {
        asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, %0"
                     : "+a"(c)
                     : "v"(__builtin_bit_cast(u32x4_t, w.v[0])), "v"(__builtin_bit_cast(u32x4_t, a.v[0])));
    }
};
// OCP e4m3 x e4m3 through the block-scaled 64-deep form (twice the bf16 rate; hardware block scales held at 2^0, tensors are
// scaled per row / per output channel in the epilogue — see Mma<fp8_t> in ss_gemm_common.h, incl. why the scale operand is
// produced by an opaque asm once per kernel): lane l supplies 32 consecutive k bytes of row l & 31 for k-block l >> 5.
template <> struct Mma32<fp8_t> {
    static constexpr int kEB = 1, kKS = 2, kNV = 2;
    static __device__ __forceinline__ uint32_t make_aux() {
        uint32_t one;
        asm volatile("v_mov_b32 %0, 0x7f\n\ts_nop 4" : "=v"(one));
        return one;
    }
    static __device__ __forceinline__ void run(const W4Frag<2>& w, const W4Frag<2>& a, f32x16_t& c, uint32_t one) {
        u32x8_t wv = {w.v[0].x, w.v[0].y, w.v[0].z, w.v[0].w, w.v[1].x, w.v[1].y, w.v[1].z, w.v[1].w};
        u32x8_t av = {a.v[0].x, a.v[0].y, a.v[0].z, a.v[0].w, a.v[1].x, a.v[1].y, a.v[1].z, a.v[1].w};
        asm volatile("v_mfma_scale_f32_32x32x64_f8f6f4 %0, %1, %2, %0, %3, %3 op_sel_hi:[0,0,0]"
                     : "+a"(c)
                     : "v"(wv), "v"(av), "v"(one));
    }
};

// pins a value of an accumulator block at this point of the (volatile-ordered) asm stream
__device__ __forceinline__ void w4_tie(f32x16_t& c) { asm volatile("" : "+a"(c)); }

// LDS layout, for the kernel and its launcher: two ring slots of [A rows | W rows] x 128 B, behind them a 32-row epilogue strip per wave
template <int BM, int BN, int WN>
struct W4Lds {
    static constexpr int TILE_BYTES = (BM + BN) * 128;
    static constexpr int STG_WAVE = 32 * (BN / WN) * 2;
    static constexpr int BYTES = 2 * TILE_BYTES + 4 * STG_WAVE;
    static_assert(BYTES <= 163840, "LDS budget");
};

// ---- epilogues ----------------------------------------------------------------------------------------------------
// value pipeline shared by both: t = acc + bias -> (GELU) -> round to T -> (+ rowvec, round)  [then GEGLU pair / residual]
template <typename T, bool GELU, bool ROWVEC>
__device__ __forceinline__ void w4_finish4(const float (&a)[4], const float (&bv)[4], const float (&rv)[4], float (&v)[4]) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        float t = a[r] + bv[r];
        if constexpr (GELU) t = gelu_for<T>(Tr<T>::rnd(t));
        v[r] = Tr<T>::rnd(t);
        if constexpr (ROWVEC) v[r] = Tr<T>::rnd(v[r] + rv[r]);
    }
}

// LDS-staged: a wave moves its TM x TN sub-tile 32 rows (one block row) at a time through a private strip.
// Strip rows are RB bytes; 16-byte chunk c of row r sits at chunk (c + r) % NC (a rotation: NC need not be a power of two).
// EV: the per-value options as compile-time variants (1 plain, 2 +GELU, 3 +rowvec, 4 GEGLU pair; see gemm_epilogue_staged)
// F8: operands were e4m3 — t = acc * scale_a[m] * scale_w[n] in fp32 in front of everything else (gemm_epilogue EM = 1)
template <typename T, int NBM, int NBN, int EV, bool F8 = false>
__device__ __forceinline__ void w4_epilogue_staged(const GemmArgs& g, f32x16_t (&acc)[NBN][NBM], int m_base, int n_base,
                                                   int lane, char* stg) {
    static_assert(Tr<T>::kVec == 8, "16-bit outputs only");
    constexpr bool GEGLU = EV == 4, GELU = EV == 2, ROWVEC = EV == 3;
    constexpr int TN = NBN * 32;
    constexpr int RB = GEGLU ? TN : TN * 2;      // strip row bytes
    constexpr int NC = RB / 16;                  // 16-byte chunks per strip row
    const int row = lane & 31, hi = lane >> 5;
    const int M = g.M;
    T* __restrict__ C = (T*)g.C;
    const T* bias = (const T*)g.bias;
    const T* res = (const T*)g.residual;
    uint2 bvp[NBN][4];      // this lane's bias values, 4 per (block, quad), kept packed (T) over the whole sub-tile
#pragma unroll
    for (int bn = 0; bn < NBN; ++bn)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            bvp[bn][q] = make_uint2(0u, 0u);
            if (g.epi & SS_EPI_BIAS) bvp[bn][q] = *reinterpret_cast<const uint2*>(bias + n_base + bn * 32 + q * 8 + hi * 4);
        }
    w4_static_for<NBM>([&](auto bm_tag) {
        constexpr int bm = decltype(bm_tag)::value;
        // this chunk's accumulator blocks are read from the AGPRs HERE, not hoisted to the top of the epilogue (256 live VGPRs)
        __builtin_amdgcn_sched_barrier(0);
        w4_static_for<NBN>([&](auto bn_tag) { w4_tie(acc[decltype(bn_tag)::value][bm]); });
        const int m = m_base + bm * 32 + row;
        float sa = 1.f;
        if constexpr (F8) sa = g.scale_a[m < M ? m : M - 1];
        const T* rp = nullptr;
        if constexpr (ROWVEC) {
            const int mm = m < M ? m : M - 1;
            rp = (const T*)g.rowvec + (int64_t)(mm / g.rows_per_batch) * g.rowvec_ld + n_base + hi * 4;
        }
        char* rowp = stg + row * RB;
#pragma unroll
        for (int bn = 0; bn < NBN; ++bn)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float a[4] = {acc[bn][bm][4 * q], acc[bn][bm][4 * q + 1], acc[bn][bm][4 * q + 2], acc[bn][bm][4 * q + 3]};
                if constexpr (F8) {      // output-channel scales fetched where they are used (L1-resident; holding all 64 spills)
                    float swq[4];
                    ld4<float>(g.scale_w + n_base + bn * 32 + q * 8 + hi * 4, swq);
#pragma unroll
                    for (int r = 0; r < 4; ++r) a[r] *= sa * swq[r];
                }
                float rv[4] = {0.f, 0.f, 0.f, 0.f}, v[4], b8[8];
                if constexpr (ROWVEC) ld4<T>(rp + bn * 32 + q * 8, rv);
                unpack<T>(make_uint4(bvp[bn][q].x, bvp[bn][q].y, 0u, 0u), b8);
                const float bq[4] = {b8[0], b8[1], b8[2], b8[3]};
                w4_finish4<T, GELU, ROWVEC>(a, bq, rv, v);
                if constexpr (GEGLU) {
                    const float o0 = v[0] * Tr<T>::rnd(gelu_for<T>(v[1])), o1 = v[2] * Tr<T>::rnd(gelu_for<T>(v[3]));
                    float pk[8] = {o0, o1, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                    const int c = 2 * bn + (q >> 1);
                    *reinterpret_cast<uint32_t*>(rowp + ((c + row) % NC) * 16 + (q & 1) * 8 + hi * 4) = pack<T>(pk).x;
                } else {
                    float pk[8] = {v[0], v[1], v[2], v[3], 0.f, 0.f, 0.f, 0.f};
                    const uint4 u = pack<T>(pk);
                    const int c = 4 * bn + q;
                    *reinterpret_cast<uint2*>(rowp + ((c + row) % NC) * 16 + hi * 8) = make_uint2(u.x, u.y);
                }
            }
        // read back whole rows (16 B per lane) and store; GEGLU rows are TN / 2 outputs wide
        const int n_out0 = GEGLU ? (n_base >> 1) : n_base;
#pragma unroll
        for (int k = 0; k < (32 * NC + 63) / 64; ++k) {
            const int idx = lane + k * 64;
            const int r = idx / NC, c = idx - r * NC;
            const int mo = m_base + bm * 32 + r;
            if (idx < 32 * NC && mo < M) {
                uint4 u = *reinterpret_cast<const uint4*>(stg + r * RB + ((c + r) % NC) * 16);
                if (g.epi & SS_EPI_RESIDUAL) {
                    const uint4 rr = *reinterpret_cast<const uint4*>(res + (int64_t)mo * g.ldr + n_base + c * 8);
                    float x[8], y[8];
                    unpack<T>(u, x);
                    unpack<T>(rr, y);
#pragma unroll
                    for (int e = 0; e < 8; ++e) x[e] += y[e];
                    u = pack<T>(x);
                }
                *reinterpret_cast<uint4*>(C + (int64_t)mo * g.ldc + n_out0 + c * 8) = u;
            }
        }
    });
}

// ---- the kernel ----------------------------------------------------------------------------------------------------
// <BM, BN> block tile (activation rows x weight rows), <WM, WN> wave grid (WM * WN == 4), D3 / D0: how many of a wave's
// NP = (BM + BN) / 32 LDS-DMA pieces of a K tile are issued in k-step 3 of the tile two before / k-step 0 of the tile
// before (the rest in its k-step 1; none in k-step 2, whose end is the landing deadline).  FLAGS & 2: persistent.
template <typename T, int BM, int BN, int WM, int WN, int D3, int D0, int FLAGS, bool CONV>
__global__ __launch_bounds__(256, 1) void gemm_w4_kernel(const GemmArgs g, const int total_tiles) {
    static_assert(WM * WN == 4, "four waves, one per SIMD");
    constexpr int TM = BM / WM, TN = BN / WN;
    constexpr int NBM = TM / 32, NBN = TN / 32, NQ = NBM * NBN, NR = NBM + NBN;
    static_assert(TM % 32 == 0 && TN % 32 == 0, "wave tile: 32x32 blocks");
    constexpr int GA = BM / 8, GW = BN / 8;                 // 8-row DMA groups per tile
    static_assert(GA % 4 == 0 && GW % 4 == 0, "DMA groups are dealt evenly to the 4 waves");
    constexpr int IA = GA / 4, IW = GW / 4, NP = IA + IW;    // ... per wave
    constexpr int D1 = NP - D3 - D0;
    static_assert(D3 >= 0 && D0 >= 0 && D1 >= 0, "DMA schedule");
    constexpr bool PERSIST = (FLAGS & 2) != 0;
    constexpr int EB = Mma32<T>::kEB, KS = Mma32<T>::kKS, NV = Mma32<T>::kNV, KT = 128 / EB;   // a K tile is 128 BYTES per row
    constexpr bool F8 = EB == 1;
    static_assert(KS == 4 || (KS == 2 && D0 == 0 && D1 == 0 && !CONV), "two-k-step tiles issue the whole next-but-one tile in their last k-step");
    using TO = typename OutT<T>::type;
    using Lds = W4Lds<BM, BN, WN>;
    constexpr int TILE_BYTES = Lds::TILE_BYTES, STG_WAVE = Lds::STG_WAVE;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wid / WN, wn = wid % WN;
    const int M = g.M, N = g.N;
    const int MT = (M + BM - 1) / BM, NT = (N + BN - 1) / BN;
    const int ntiles = g.K / KT;
    const uint32_t lds0 = __builtin_amdgcn_readfirstlane((uint32_t)(size_t)(lds_void_t*)smem_raw);

    // ---- staging coordinates: piece i of this wave = 8-row group i * 4 + wid; lane -> (row lane >> 3, physical chunk lane & 7)
    const int srow = lane >> 3;
    const int schunk = (lane & 7) ^ ((4 * (wid & 1) + (srow >> 1)) & 7);    // logical chunk: c ^ ((r >> 1) & 7), r = 8 g + srow
    int m_blk = 0, n_blk = 0;
    uint32_t voffW[IW], voffA[IA];
    int cbH[CONV ? IA : 1], cyS[CONV ? IA : 1], cxS[CONV ? IA : 1];
    const char* sbaseW = nullptr;
    const char* sbaseA = nullptr;
    auto setup_tile = [&](int vid) {
        int mt_, nt_;
        xcd_tile_id(g.swz, MT, NT, vid, mt_, nt_);
        m_blk = mt_ * BM; n_blk = nt_ * BN;
#pragma unroll
        for (int i = 0; i < IW; ++i) {
            int n = n_blk + (i * 4 + wid) * 8 + srow;
            n = n < N ? n : N - 1;
            voffW[i] = (uint32_t)((int64_t)(n - n_blk) * g.ldw * EB + schunk * 16);
        }
        sbaseW = (const char*)g.W + (int64_t)n_blk * g.ldw * EB;
        sbaseA = (const char*)g.A;
        if constexpr (CONV) {
            const int hw = g.conv_Ho * g.conv_Wo;
#pragma unroll
            for (int i = 0; i < IA; ++i) {
                int m = m_blk + (i * 4 + wid) * 8 + srow;
                m = m < M ? m : M - 1;
                const int b = m / hw;
                const int rem = m - b * hw;
                const int y = rem / g.conv_Wo;
                cbH[i] = b * g.conv_H;
                cyS[i] = y * g.conv_stride;
                cxS[i] = (rem - y * g.conv_Wo) * g.conv_stride;
            }
        } else {
#pragma unroll
            for (int i = 0; i < IA; ++i) {
                int m = m_blk + (i * 4 + wid) * 8 + srow;
                m = m < M ? m : M - 1;
                voffA[i] = (uint32_t)((int64_t)(m - m_blk) * g.lda * EB + schunk * 16);
            }
            sbaseA += (int64_t)m_blk * g.lda * EB;
        }
        sbaseW = uniform_ptr(sbaseW);
        sbaseA = uniform_ptr(sbaseA);
    };

    // piece q (< IA: A group, else W group) of K tile t into ring slot `slot` (wave-uniform run-time value).  M0 is left modified.
    auto issue_piece = [&](int t, int slot, int q) {
        const uint32_t base = lds0 + (uint32_t)slot * (uint32_t)TILE_BYTES;
        if (q < IA) {
            const int i = q;
            const int r8 = (i * 4 + wid) * 8;
            if constexpr (CONV) {
                const int k0 = t * 64;
                const int tap = k0 / g.conv_Cin;                       // wave-uniform: the whole tile is one filter tap
                const int ci = k0 - tap * g.conv_Cin + schunk * 8;
                const int dy = tap / 3 - 1, dx = tap - (tap / 3) * 3 - 1;
                const int Hin = g.conv_up ? 2 * g.conv_H : g.conv_H, Win = g.conv_up ? 2 * g.conv_W : g.conv_W;
                int iy = cyS[i] + dy, ix = cxS[i] + dx;
                const bool ok = (unsigned)iy < (unsigned)Hin && (unsigned)ix < (unsigned)Win;
                if (g.conv_up) { iy >>= 1; ix >>= 1; }
                const uint32_t off = (uint32_t)((((cbH[i] + iy) * g.conv_W + ix) * g.conv_Cin + ci) * 2);
                if (ok) {
                    dma16s(off, sbaseA, __builtin_amdgcn_readfirstlane(base + (uint32_t)(r8 * 128)));
                } else {   // zero padding: this lane's 16-byte slot is written directly (the DMA skips masked lanes)
                    *reinterpret_cast<uint4*>(smem_raw + slot * TILE_BYTES + r8 * 128 + lane * 16) = make_uint4(0, 0, 0, 0);
                }
            } else {
                dma16s(voffA[i], sbaseA + (int64_t)t * 128, __builtin_amdgcn_readfirstlane(base + (uint32_t)(r8 * 128)));
            }
        } else {
            const int i = q - IA;
            dma16s(voffW[i], sbaseW + (int64_t)t * 128,
                   __builtin_amdgcn_readfirstlane(base + (uint32_t)((BM + (i * 4 + wid) * 8) * 128)));
        }
    };
    auto issue_range = [&](int t, int slot, int q0, int q1) {
        const uint32_t keep = m0_save();
#pragma unroll
        for (int q = 0; q < NP; ++q)
            if (q >= q0 && q < q1) issue_piece(t, slot, q);
        m0_restore(keep);
    };

    // ---- fragment addressing: lane l reads row (l & 31) of a 32-row block.  16-bit: logical chunk 2 ks + (l >> 5); fp8: the chunk
    // PAIR 4 ks + 2 (l >> 5) + {0, 1}.  The swizzle term ((r >> 1) & 7) only depends on l & 31 (block bases are multiples of 16) and
    // the k-step only touches the chunk bits above the lane's own: address(ks) = address(0) ^ (ks << (F8 ? 6 : 5)), second piece ^ 16.
    const uint32_t fsw = (uint32_t)(((lane & 31) >> 1) & 7);
    const uint32_t fc0 = ((uint32_t)((lane >> 5) << (F8 ? 1 : 0)) ^ fsw) << 4;
    const uint32_t fa0 = (uint32_t)((wm * TM + (lane & 31)) * 128) + fc0;
    const uint32_t fw0 = (uint32_t)((BM + wn * TN + (lane & 31)) * 128) + fc0;
    W4Frag<NV> fa[2][NBM], fw[2][NBN];
    // read r of the NR operand reads of k-step ks of the tile in `slot` into register set `set`; order = first use:
    // W block 0, A blocks 0 .. NBM-1, W blocks 1 .. NBN-1 (the MFMAs walk bn-major)
    auto read_one = [&](int slot, int ks, int set, int r) {
        const char* b = smem_raw + slot * TILE_BYTES;
        const uint32_t x = (uint32_t)ks << (F8 ? 6 : 5);
        auto rd = [&](W4Frag<NV>& f, uint32_t addr) {
            f.v[0] = *reinterpret_cast<const uint4*>(b + addr);
            if constexpr (NV == 2) f.v[1] = *reinterpret_cast<const uint4*>(b + (addr ^ 16u));
        };
        if (r == 0) rd(fw[set][0], fw0 ^ x);
        else if (r <= NBM) rd(fa[set][r - 1], (fa0 ^ x) + (r - 1) * 4096);
        else rd(fw[set][r - NBM], (fw0 ^ x) + (r - NBM) * 4096);
    };

    f32x16_t acc[NBN][NBM];
    const uint32_t mma_aux = Mma32<T>::make_aux();

    // One k-step: NQ MFMAs on register set `set`; in gap q (after MFMA q) go read r of the NEXT k-step's operands when
    // gap_r(r) == q and, when dma_on, LDS-DMA piece d0 + d (d < nd) when gap_d(d) == q.  EARLY: reads in the first gaps
    // (k-step 2: they must have landed by the barrier that follows).
    auto kstep = [&](auto set_tag, auto early_tag, int rslot, int rks, auto nd_tag, auto d0_tag, bool dma_on, int dt, int dslot) {
        constexpr int set = decltype(set_tag)::value;
        constexpr bool EARLY = decltype(early_tag)::value;
        constexpr int ND = decltype(nd_tag)::value, DQ0 = decltype(d0_tag)::value;
        const uint32_t keep = m0_save();
        w4_static_for<NQ>([&](auto q_tag) {
            constexpr int q = decltype(q_tag)::value;
            constexpr int bn = q / NBM, bm = q % NBM;
            Mma32<T>::run(fw[set][bn], fa[set][bm], acc[bn][bm], mma_aux);
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                const int gq = EARLY ? r : (r * NQ) / NR;
                if (gq == q) read_one(rslot, rks, set ^ 1, r);
            }
#pragma unroll
            for (int d = 0; d < ND; ++d) {
                const int gq = ((2 * d + 1) * NQ) / (2 * ND > 0 ? 2 * ND : 1);
                if (gq == q) { if (dma_on) issue_piece(dt, dslot, DQ0 + d); }
            }
            __builtin_amdgcn_sched_barrier(0);
        });
        m0_restore(keep);
    };

    int vid = blockIdx.x;
    setup_tile(vid);
    issue_range(0, 0, 0, NP);
    if (ntiles > 1) issue_range(1, 1, 0, NP);

    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    using BF = std::integral_constant<bool, false>;
    using BT = std::integral_constant<bool, true>;
    while (true) {
        const int m_cur = m_blk, n_cur = n_blk;
        const int vnext = vid + (int)gridDim.x;
        const bool has_next = PERSIST && vnext < total_tiles;
#pragma unroll
        for (int i = 0; i < NBN; ++i)
#pragma unroll
            for (int j = 0; j < NBM; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
        w4_static_for<NQ>([&](auto q_tag) {   // the zeros are in the AGPRs before the wait states below start counting
            constexpr int q = decltype(q_tag)::value;
            w4_tie(acc[q / NBM][q % NBM]);
        });
        // K tiles 0 (and 1) were issued in the prologue / under the previous tile's last k-step and epilogue
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
#pragma unroll
        for (int r = 0; r < NR; ++r) read_one(0, 0, 0, r);
        asm volatile("s_nop 7" ::: "memory");   // asm MFMAs are opaque to the hazard recognizer (accumulator init)
        __builtin_amdgcn_sched_barrier(0);

        // K tile t in ring slot t & 1.  LAST: the output tile's final K tile, a separate instantiation BEHIND the steady-state
        // loop (with has_next it re-targets the staging registers at the next output tile behind its barrier).  The MFMA
        // sequences form one straight line  loop -> last step -> epilogue : alternative asm blocks that update the
        // accumulators would make the allocator shuttle all 256 of them through VGPRs at the join.
        auto step = [&](auto last_tag, int t) {
            constexpr bool LAST = decltype(last_tag)::value;
            const int cur = t & 1;
            const bool dmaA = t >= 1 && !LAST;               // rest of tile t+1 -> slot cur ^ 1
            const bool dmaB = !LAST && t + 2 < ntiles;       // head of tile t+2 -> slot cur (free after this tile's barrier)
            const bool lastp = LAST && has_next;             // head of the NEXT output tile's K tile 0 -> slot 0
            w4_static_for<KS>([&](auto p_tag) {
                constexpr int p = decltype(p_tag)::value;
                using SET = std::integral_constant<int, p & 1>;        // KS is even: k-step 0 of every tile reads register set 0
                if constexpr (p < KS - 2) {         // (16-bit tiles) k-steps 0 and 1: the rest of tile t+1
                    kstep(SET{}, BF{}, cur, p + 1, std::integral_constant<int, LAST ? 0 : (p == 0 ? D0 : D1)>{},
                          std::integral_constant<int, p == 0 ? D3 : D3 + D0>{}, dmaA, t + 1, cur ^ 1);
                } else if constexpr (p == KS - 2) {
                    kstep(SET{}, BT{}, cur, p + 1, I0{}, I0{}, false, 0, 0);
                    // the tile's barrier: my fragments of slot cur are in registers, my pieces of tile t+1 have landed
                    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
                    __builtin_amdgcn_s_barrier();
                    if constexpr (LAST) {
                        if (lastp) setup_tile(vnext);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                } else {
                    if constexpr (LAST) kstep(SET{}, BF{}, cur ^ 1, 0, std::integral_constant<int, D3>{}, I0{}, lastp, 0, 0);
                    else kstep(SET{}, BF{}, cur ^ 1, 0, std::integral_constant<int, D3>{}, I0{}, dmaB, t + 2, cur);
                }
            });
        };
        for (int t = 0; t + 1 < ntiles; ++t) step(BF{}, t);
        step(BT{}, ntiles - 1);
        if (has_next) {   // rest of the next output tile's K tile 0, all of its K tile 1: they land under the epilogue
            issue_range(0, 0, D3, NP);
            if (ntiles > 1) issue_range(1, 1, 0, NP);
        }
        // MFMA results settle before v_accvgpr_read.  The asm MFMAs are opaque to the hazard recognizer AND to the scheduler's
        // idea of latency: without the per-block ties below the allocator copies a block to VGPRs right behind its last MFMA
        // (seen: v_accvgpr_read one s_nop 0 after the v_mfma -> in-flight garbage).  Volatile asms keep their order.
        asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
        w4_static_for<NQ>([&](auto q_tag) {
            constexpr int q = decltype(q_tag)::value;
            w4_tie(acc[q / NBM][q % NBM]);
        });
        __builtin_amdgcn_sched_barrier(0);

        {   // (w4_launch only admits shapes whose every wave sub-tile lies inside N with 16-byte-aligned operands)
            const int mb = m_cur + wm * TM, nb = n_cur + wn * TN;
            char* stg = smem_raw + 2 * TILE_BYTES + wid * STG_WAVE;
            // the lane id is laundered per output tile: otherwise every lane-derived address of the epilogue is loop-invariant,
            // gets hoisted out of the persistent loop and lives (= spills) across the K loop
            int lane_e = lane;
            asm volatile("" : "+v"(lane_e));
            const bool o_gelu = (g.epi & SS_EPI_GELU) != 0, o_geglu = (g.epi & SS_EPI_GEGLU_PAIR) != 0;
            if (nb >= N) {}     // the last n tile of a ragged N: this wave's columns do not exist (N % TN == 0: all or nothing)
            else if constexpr (CONV) {   // (w4_launch admits only the option sets instantiated here)
                if (g.rowvec) w4_epilogue_staged<TO, NBM, NBN, 3, F8>(g, acc, mb, nb, lane_e, stg);
                else w4_epilogue_staged<TO, NBM, NBN, 1, F8>(g, acc, mb, nb, lane_e, stg);
            } else {
                if (o_geglu) w4_epilogue_staged<TO, NBM, NBN, 4, F8>(g, acc, mb, nb, lane_e, stg);
                else if (o_gelu) w4_epilogue_staged<TO, NBM, NBN, 2, F8>(g, acc, mb, nb, lane_e, stg);
                else w4_epilogue_staged<TO, NBM, NBN, 1, F8>(g, acc, mb, nb, lane_e, stg);
            }
        }
        if (!has_next) break;
        vid = vnext;
    }
}

template <typename T, int BM, int BN, int WM, int WN, int D3, int D0, int FLAGS>
static int w4_launch(const GemmArgs& g, hipStream_t s) {
    constexpr bool CONV = SS_W4_CONV != 0;
    const bool conv = g.conv_Cin > 0;
    if (conv != CONV) return 1;
    constexpr int EB = Mma32<T>::kEB;
    if (g.rowstat_out || g.rowpart || g.ln_part || g.shift_a || g.ksplit > 1 || ((g.scale_a != nullptr) != (EB == 1))) return 1;   // no statistics / folded-norm / split-K epilogues here
    // per-value options exist as compile-time variants only: GELU or GEGLU (GEMM), the time-embedding row vector (conv)
    if (conv ? (g.epi & (SS_EPI_GELU | SS_EPI_GEGLU_PAIR)) != 0
             : (g.rowvec != nullptr || ((g.epi & SS_EPI_GELU) && (g.epi & SS_EPI_GEGLU_PAIR)))) return 1;
    const bool ok = (g.K % (128 / EB) == 0) && (!conv || g.conv_Cin % 64 == 0) && g.K >= 128 / EB &&
                    (conv ? (int64_t)g.M * g.conv_stride * g.conv_stride * g.conv_Cin * 2 < (1ll << 31)
                          : ((int64_t)BM * g.lda * EB < (1ll << 31))) && (int64_t)BN * g.ldw * EB < (1ll << 31) &&
                    (EB == 2 || (((size_t)g.scale_w) & 15) == 0);
    if (!ok) return 1;
    // the kernel has the LDS-staged epilogue only: whole wave sub-tiles in N, 16-byte-aligned operands
    constexpr size_t A16 = 15;
    const bool staged_ok = (g.N % (BN / WN) == 0) && (((size_t)g.C | (size_t)g.residual | (size_t)g.bias | (size_t)g.rowvec) & A16) == 0 &&
                           ((g.ldc | g.ldr | g.rowvec_ld) & 7) == 0;
    if (!staged_ok) return 1;
    return launch_tiles<gemm_w4_kernel<T, BM, BN, WM, WN, D3, D0, FLAGS, CONV>>("gemm_w4", g, cdiv(g.M, BM) * cdiv(g.N, BN),
                                                                                (FLAGS & 2) ? num_cus() : 0, 256, W4Lds<BM, BN, WN>::BYTES, s);
}

// cfg ids 90-99 (the tile table stores cfg + 100 * xcd_group, so ids stay below 100)
#if defined(SS_W4_FP8)
int gemm_w4_dispatch_fp8(int cfg, const GemmArgs& g, hipStream_t s) {
    switch (cfg) {
#define SS_W4_CASE(id, BM, BN, WM, WN, D3, D0, FLAGS, VAR) case id: return w4_launch<fp8_t, BM, BN, WM, WN, D3, D0, FLAGS>(g, s);
        SS_W4_FP8_TILES(SS_W4_CASE)
        default: return 1;
    }
}
#else
#if SS_W4_CONV
template <typename T> int gemm_w4_dispatch_conv(int cfg, const GemmArgs& g, hipStream_t s) {
#else
template <typename T> int gemm_w4_dispatch(int cfg, const GemmArgs& g, hipStream_t s) {
#endif
    switch (cfg) {
        case 90: return w4_launch<T, 256, 256, 2, 2, 6, 6, 2>(g, s);   // persistent, DMA 6 / 6 / 4
        case 91: return w4_launch<T, 256, 256, 2, 2, 8, 8, 2>(g, s);   // DMA 8 / 8 / 0 (earliest landing, denser issue)
        case 92: return w4_launch<T, 256, 256, 2, 2, 4, 6, 2>(g, s);   // DMA 4 / 6 / 6
        case 93: return w4_launch<T, 256, 256, 2, 2, 6, 6, 0>(g, s);   // one tile per workgroup
        default: return 1;
    }
}

#if SS_W4_CONV
template int gemm_w4_dispatch_conv<SS_W4_T>(int, const GemmArgs&, hipStream_t);
#else
template int gemm_w4_dispatch<SS_W4_T>(int, const GemmArgs&, hipStream_t);
#endif
#endif  // SS_W4_FP8

}  // namespace ss
