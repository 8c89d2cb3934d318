// Software-pipelined LDS-DMA GEMM / implicit-GEMM 3x3 conv for 16-bit dtypes (K % 64 == 0; conv: Cin % 64 == 0)
// and, GEMM only, fp8 e4m3 operands with bf16 results (ss_gemm_sp_fp8.hip; K % 128 == 0).
// Included by ss_gemm_sp_{bf16,f16}[_conv].hip with SS_SP_T (element type) and SS_SP_CONV (0 | 1) defined, so that
// the ~40 kernel instantiations compile as four parallel translation units.
//
// Tile format (same as gemm_glds_kernel): 64-wide K tiles, LDS rows of 128 bytes = 8 chunks of 16 B, chunk c of
// row r stored at physical chunk c ^ (r & 7); the permutation is applied on the SOURCE address of each DMA lane
// (inside one 128-byte line: coalescing unchanged) and on the fragment read address (conflict-free ds_read_b128).
//
// Structure (what rocprofv3 showed limits the plain double-buffered kernel: MFMA busy 39 %, a third of the time
// parked in s_waitcnt / s_barrier):
//  (1) the fragment reads of the NEXT phase are in flight while the MFMAs of the current one run (two register
//      sets, sched_barrier-pinned), so no MFMA waits on LDS latency;
//  (2) ONE barrier per K tile, placed before the tile's last phase; DMA sources are `SGPR base + loop-invariant
//      32-bit lane offset` (no vector ALU work to issue a tile);
//  (3) accumulate-in-place asm MFMAs pin the accumulators (the allocator otherwise shuttles them through copies);
//  (4) NS-deep LDS ring (NS = 3 where it fits the 160 KB of a CU): tiles t+1 .. t+NS-1 are in flight / landed
//      while tile t is consumed, the wait before the barrier is a COUNTED vmcnt (never a drain in steady state);
//  (5) the 8-row DMA groups of a tile are dealt round-robin to the waves, so tile heights that do not divide by
//      8*waves work (256x160 with 8 waves: 52 groups) — [8192 x 1280] outputs are exactly 256 tiles of 256x160 =
//      one tile per CU with 98 FLOP per byte fetched from L2 (128x160: 71; the L2 feeds ~35 TB/s, so at 2.5 PF/s
//      71 FLOP/B is L2-bound);
//  (6) FLAGS & 1: s_setprio 1 around the MFMA clusters (the co-resident wave of the SIMD issues its ds_read / DMA
//      in the gaps);
//  (8) FLAGS & 4: the DMA pieces of tile t+NS are not issued as one burst behind the barrier (each piece costs
//      60-180 issue cycles during which that wave feeds no MFMA, and every wave of the workgroup does it at the same
//      moment) but one at a time BETWEEN the MFMAs of the tile's last phase;
//  (9) FLAGS & 8: LDS-staged epilogue (gemm_epilogue_staged): whole-row 16-byte stores / residual reads;
//      (measured and dropped: a role-split loop with the two wave groups of a 256x256 tile one barrier apart, LOAD and
//      MFMA segments alternating — 1224 vs 1229 TFLOP/s at 4096^3: the K loop is not what limits these kernels, the
//      ~15 us of fixed per-tile cost is)
//  (7) FLAGS & 2: persistent — a workgroup walks tiles vid, vid + grid, ...; the first NS K-tiles of the NEXT output
//      tile are DMA'd right after the last barrier of the current one, i.e. under the epilogue (bias / GELU /
//      residual / stores), which at one workgroup per CU would otherwise leave the matrix cores idle.
// Rows beyond M / N are clamped to the last valid row at setup (their results are never stored).

namespace ss {

// LDS layout of a tile, for the kernel and its launcher: an NS-slot ring of [A rows | W rows] x 128 B, and for the LDS-staged
// epilogue (FLAGS & 8) a private strip of STG_CR rows per wave — behind the ring when both fit the 160 KB of a CU, otherwise
// inside ring slot 0 (then the next output tile's prefetch has to wait for the epilogue)
template <int BM, int BN, int WM, int WN, int NS, int FLAGS>
struct SpLds {
    static constexpr int NW = WM * WN, TILE_BYTES = (BM + BN) * 128;
    static constexpr int STG_CR = 16, STG_WAVE = STG_CR * ((BN / WN) * 2 + 16);
    static constexpr bool STG_IN_RING = (NW == 4 ? 2 : 1) * (NS * TILE_BYTES + NW * STG_WAVE) > 163840;   // 4-wave tiles are meant to run two workgroups per CU
    static constexpr int BYTES = NS * TILE_BYTES + ((FLAGS & 8) != 0 && !STG_IN_RING ? NW * STG_WAVE : 0);
};

template <typename T, int BM, int BN, int WM, int WN, int NH, int NS, int FLAGS, bool CONV>
__global__ __launch_bounds__(64 * WM * WN) void gemm_sp_kernel(const GemmArgs g, const int total_tiles) {
    constexpr int NW = WM * WN;
    constexpr int TM = BM / WM, TN = BN / WN;
    constexpr int FM = TM / 16, FN = TN / 16;
    constexpr int GA = BM / 8, GW = BN / 8;                          // 8-row DMA groups per tile
    constexpr int IA = (GA + NW - 1) / NW, IW = (GW + NW - 1) / NW;  // ... per wave (upper bound)
    constexpr bool EVEN = (GA % NW == 0) && (GW % NW == 0);
    constexpr bool PRIO = (FLAGS & 1) != 0, PERSIST = (FLAGS & 2) != 0, SPREAD = (FLAGS & 4) != 0, STAGED = (FLAGS & 8) != 0;
    constexpr bool RSTAT = (FLAGS & 32) != 0;     // epilogues also accumulate per-row (sum, sum of squares) of the stored values
    constexpr bool SPLITK = (FLAGS & 64) != 0;    // grid.y K ranges, raw fp32 partial sums out (small-M weight-streaming GEMMs)
    static_assert(!SPLITK || (!PERSIST && !STAGED && !CONV && !RSTAT && (FLAGS & 16) == 0), "split-K: plain tiles only");
    static_assert(BM % 8 == 0 && BN % 8 == 0 && TM % 16 == 0 && TN % 16 == 0, "tile geometry");
    static_assert(NS == 2 || (NS == 3 && !CONV), "ring depth");
    // element size / MFMA depth: a K tile is always 128 BYTES per row = KT elements = KS MFMA k-steps
    constexpr int EB = Mma<T>::kEB, KT = 128 / EB, KS = KT / Mma<T>::kK, NV = Mma<T>::kNV;
    constexpr bool F8 = EB == 1;
    static_assert(KS == 2 || (KS == 1 && NS == 2 && !CONV), "fp8 tiles: double-buffered GEMM only");
    static_assert(!F8 || NW % 2 == 0, "fp8 swizzle: DMA groups are dealt to an even number of waves");
    using TO = typename OutT<T>::type;
    constexpr int EM = F8 ? 1 : (((FLAGS & 16) != 0) ? 2 : 0);
    static_assert(!(F8 && (FLAGS & 16)), "fp8 tiles carry their own scaling epilogue");
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    using Lds = SpLds<BM, BN, WM, WN, NS, FLAGS>;
    constexpr int TILE_BYTES = Lds::TILE_BYTES, STG_CR = Lds::STG_CR, STG_WAVE = Lds::STG_WAVE;
    constexpr bool STG_IN_RING = Lds::STG_IN_RING;
    constexpr bool PREFETCH_EARLY = !(STAGED && STG_IN_RING);

    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wid / WN, wn = wid % WN;
    const int l15 = lane & 15, grp = lane >> 4;
    const int M = g.M, N = g.N;
    const int MT = (M + BM - 1) / BM, NT = (N + BN - 1) / BN;
    int kt0 = 0, ntiles = g.K / KT;
    if constexpr (SPLITK) {            // this workgroup's K tiles: [kt0, kt0 + ntiles)
        const int per = (ntiles + g.ksplit - 1) / g.ksplit;
        kt0 = (int)blockIdx.y * per;
        ntiles = ntiles - kt0 < per ? ntiles - kt0 : per;
        if (ntiles < 0) ntiles = 0;
    }
    const uint32_t lds0 = __builtin_amdgcn_readfirstlane((uint32_t)(size_t)(lds_void_t*)smem_raw);
    // DMA groups of this wave: g = i * NW + wid, i < IA (IW); the last i may not exist when the split is uneven
    const int cntA = EVEN ? IA : (GA - wid + NW - 1) / NW, cntW = EVEN ? IW : (GW - wid + NW - 1) / NW;

    // ---- staging coordinates (invariant over the K loop of one output tile) -------------------------------
    const int srow = lane >> 3;                 // row within an 8-row DMA group
    // logical 16-byte chunk this lane fetches (source-side swizzle).  16-bit tiles: chunk c of row r sits at c ^ (r & 7).
    // fp8 tiles: a lane reads the chunk PAIR (2g, 2g+1) of its row, and ds_read_b128 is serviced in the lane groups
    // {0-3,12-15,20-27}, {4-11,16-19,28-31} (+32): with r & 7 rows 0-3/12-15 of k-block g and rows 4-11 of k-block g+1 land
    // on the same 16-byte slots (measured: SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE = 0.50).  s(r) = bit1(r) | bit3(r) << 2
    // keeps bit 1 of the physical chunk equal to bit 1 of the logical one, which separates the two k-blocks of a lane
    // group, and is injective on each group's row set.  (Rows of a DMA group g8 = 8 rows: bit 3 of r is the group's parity,
    // which is the wave's parity because groups are dealt round-robin to an even number of waves.)
    const int schunk = F8 ? ((lane & 7) ^ (((srow >> 1) & 1) | ((wid & 1) << 2))) : ((lane & 7) ^ srow);
    int m_blk = 0, n_blk = 0;
    uint32_t voffW[IW], voffA[IA];
    int cbH[IA], cyS[IA], cxS[IA];
    const char* sbaseW = nullptr;
    const char* sbaseA = nullptr;
    auto setup_tile = [&](int vid) {
        int mt_, nt_;
        xcd_tile_id(g.swz, MT, NT, vid, mt_, nt_);
        m_blk = mt_ * BM; n_blk = nt_ * BN;
#pragma unroll
        for (int i = 0; i < IW; ++i) {
            int n = n_blk + (i * NW + wid) * 8 + srow;
            n = n < N ? n : N - 1;
            voffW[i] = (uint32_t)((int64_t)(n - n_blk) * g.ldw * EB + schunk * 16);
        }
        sbaseW = (const char*)g.W + (int64_t)n_blk * g.ldw * EB + (int64_t)kt0 * 128;
        sbaseA = (const char*)g.A + (CONV ? 0 : (int64_t)kt0 * 128);
        if constexpr (CONV) {
            const int hw = g.conv_Ho * g.conv_Wo;
#pragma unroll
            for (int i = 0; i < IA; ++i) {
                int m = m_blk + (i * NW + wid) * 8 + srow;
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
                int m = m_blk + (i * NW + wid) * 8 + srow;
                m = m < M ? m : M - 1;
                voffA[i] = (uint32_t)((int64_t)(m - m_blk) * g.lda * EB + schunk * 16);
            }
            sbaseA += (int64_t)m_blk * g.lda * EB;
        }
        sbaseW = uniform_ptr(sbaseW);
        sbaseA = uniform_ptr(sbaseA);
    };

    // piece q of K tile t into ring slot buf: q < IA = this wave's q-th 8-row group of A, else its (q-IA)-th group of W.
    // M0 is left modified (callers bracket a run of pieces with m0_save / m0_restore).
    auto issue_piece = [&](int t, int buf, int q) {
        const uint32_t base = lds0 + (uint32_t)(buf * TILE_BYTES);
        if (q < IA) {
            const int i = q;
            if (!(EVEN || i < cntA)) return;
            if constexpr (CONV) {
                const int k0 = t * 64;
                const int tap = k0 / g.conv_Cin;                       // wave-uniform: the whole tile is one filter tap
                const int ci = k0 - tap * g.conv_Cin + schunk * 8;
                const int dy = tap / 3 - 1, dx = tap - (tap / 3) * 3 - 1;
                const int Hin = g.conv_up ? 2 * g.conv_H : g.conv_H, Win = g.conv_up ? 2 * g.conv_W : g.conv_W;
                const int r8 = (i * NW + wid) * 8;
                int iy = cyS[i] + dy, ix = cxS[i] + dx;
                const bool ok = (unsigned)iy < (unsigned)Hin && (unsigned)ix < (unsigned)Win;
                if (g.conv_up) { iy >>= 1; ix >>= 1; }
                const uint32_t off = (uint32_t)((((cbH[i] + iy) * g.conv_W + ix) * g.conv_Cin + ci) * 2);
                if (ok) {
                    dma16s(off, sbaseA, __builtin_amdgcn_readfirstlane(base + (uint32_t)(r8 * 128)));
                } else {   // zero padding: this lane's 16-byte slot is written directly (the DMA skips masked lanes)
                    *reinterpret_cast<uint4*>(smem_raw + buf * TILE_BYTES + r8 * 128 + lane * 16) = make_uint4(0, 0, 0, 0);
                }
            } else {
                dma16s(voffA[i], sbaseA + (int64_t)t * 128,
                       __builtin_amdgcn_readfirstlane(base + (uint32_t)((i * NW + wid) * 8 * 128)));
            }
        } else {
            const int i = q - IA;
            if (!(EVEN || i < cntW)) return;
            dma16s(voffW[i], sbaseW + (int64_t)t * 128,
                   __builtin_amdgcn_readfirstlane(base + (uint32_t)((BM + (i * NW + wid) * 8) * 128)));
        }
    };
    auto issue_tile = [&](int t, int buf) {
        const uint32_t keep = m0_save();
#pragma unroll
        for (int q = 0; q < IA + IW; ++q) issue_piece(t, buf, q);
        m0_restore(keep);
    };

    // wait until at most `fly` whole K tiles of this wave's DMA pieces are still in flight (fly <= NS - 1).  CONV: a
    // wave whose 64 lanes are all padding skips that DMA entirely, so the number of outstanding loads per tile is
    // not a constant there and only a full drain is safe.
    auto wait_fly = [&](int fly) {
        if (CONV || fly <= 0) { wait_vmcnt<0>(); return; }
        constexpr int HI = IA + IW;
        const int mine = cntA + cntW;   // wave-uniform
        if (EVEN || mine == HI) { if (fly == 1) wait_vmcnt<HI>(); else wait_vmcnt<2 * HI>(); }
        else if (mine == HI - 1) { if (fly == 1) wait_vmcnt<HI - 1>(); else wait_vmcnt<2 * (HI - 1)>(); }
        else { if (fly == 1) wait_vmcnt<(HI > 2 ? HI - 2 : 0)>(); else wait_vmcnt<(HI > 2 ? 2 * (HI - 2) : 0)>(); }
    };

    // ---- fragment addressing: row r of a tile lives at r*128, chunk c at ((c ^ (r & 7)) << 4); r & 7 == l15 & 7
    // for every fragment, so ks = 1 is the ks = 0 address XOR 64 and fragments are 2048 B apart ------------------
    // (fp8: lane group grp owns k bytes [32 grp, 32 grp + 32) = chunks 2 grp and 2 grp + 1; the second is the first XOR 16)
    const uint32_t fchunk = F8 ? (uint32_t)(2 * grp) : (uint32_t)grp;
    const uint32_t fswz = F8 ? (uint32_t)(((l15 >> 1) & 1) | (((l15 >> 3) & 1) << 2)) : (uint32_t)(l15 & 7);
    const uint32_t fa0 = (uint32_t)((wm * TM + l15) * 128 + ((fchunk ^ fswz) << 4));
    const uint32_t fw0 = (uint32_t)((BM + wn * TN + l15) * 128 + ((fchunk ^ fswz) << 4));
    // A K tile is consumed in P = 2*NH phases (ks, h): k-step ks of the tile, h-th 1/NH of the wave's A rows.
    // Phase p multiplies A set (p & 1) with W set (ks & 1); the operands of phase p+1 are read while the MFMAs
    // of phase p run.  NH = 2 halves the fragment registers of a 128-row wave tile (64 instead of 96 VGPRs).
    // Register sets alternate per phase (A) / per k-step (W) ACROSS tiles: with an odd number of phases or k-steps per
    // tile (fp8: KS = 1) the set of phase 0 depends on the tile's parity `par`; for the 16-bit forms it drops out.
    constexpr int FMH = FM / NH, P = KS * NH;
    static_assert(FM % NH == 0, "A fragments must split evenly");
    Frag<NV> fa[2][FMH], fw[2][FN];
    auto read_phase = [&](int buf, int p, int par) {   // operands of phase p of the tile in ring slot `buf`
        const int ks = p / NH, h = p % NH;
        const int sa = (par * P + p) & 1, sw = (par * KS + ks) & 1;
        const char* b = smem_raw + buf * TILE_BYTES;
        const uint32_t xa = ks ? (fa0 ^ 64u) : fa0, xw = ks ? (fw0 ^ 64u) : fw0;
        if (h == 0) {
#pragma unroll
            for (int i = 0; i < FN; ++i) {
                fw[sw][i].v[0] = *reinterpret_cast<const uint4*>(b + xw + i * 2048);
                if constexpr (NV == 2) fw[sw][i].v[1] = *reinterpret_cast<const uint4*>(b + (xw ^ 16u) + i * 2048);
            }
        }
#pragma unroll
        for (int j = 0; j < FMH; ++j) {
            fa[sa][j].v[0] = *reinterpret_cast<const uint4*>(b + xa + (h * FMH + j) * 2048);
            if constexpr (NV == 2) fa[sa][j].v[1] = *reinterpret_cast<const uint4*>(b + (xa ^ 16u) + (h * FMH + j) * 2048);
        }
    };

    f32x4_t acc[FN][FM];
    const uint32_t mma_aux = Mma<T>::make_aux();
    auto mma_phase = [&](int p, int par) {
        const int ks = p / NH, h = p % NH;
        const int sa = (par * P + p) & 1, sw = (par * KS + ks) & 1;
#pragma unroll
        for (int i = 0; i < FN; ++i)
#pragma unroll
            for (int j = 0; j < FMH; ++j) Mma<T>::run_inplace(fw[sw][i], fa[sa][j], acc[i][h * FMH + j], mma_aux);
    };

    // the same MFMAs with the DMA pieces of K tile `t_dma` (-> ring slot `buf_dma`) issued in between, evenly spaced
    auto mma_phase_dma = [&](int p, int par, int t_dma, int buf_dma, bool dma_on) {   // dma_on is wave-uniform
        const int ks = p / NH, h = p % NH;
        const int sa = (par * P + p) & 1, sw = (par * KS + ks) & 1;
        constexpr int NM = FN * FMH, NP = IA + IW;
        constexpr int STRIDE = NM / NP > 0 ? NM / NP : 1;
        const uint32_t keep = m0_save();
#pragma unroll
        for (int i = 0; i < FN; ++i)
#pragma unroll
            for (int j = 0; j < FMH; ++j) {
                Mma<T>::run_inplace(fw[sw][i], fa[sa][j], acc[i][h * FMH + j], mma_aux);
                const int mi = i * FMH + j + 1;                      // compile-time after unrolling
                if (mi % STRIDE == 0 && mi / STRIDE - 1 < NP) { if (dma_on) issue_piece(t_dma, buf_dma, mi / STRIDE - 1); }
            }
#pragma unroll
        for (int r = NM / STRIDE; r < NP; ++r) { if (dma_on) issue_piece(t_dma, buf_dma, r); }
        m0_restore(keep);
    };

    int vid = blockIdx.x;
    setup_tile(vid);
#pragma unroll
    for (int st = 0; st < NS; ++st)
        if (st < ntiles) issue_tile(st, st);

    while (true) {
        const int m_cur = m_blk, n_cur = n_blk;
        const int vnext = vid + (int)gridDim.x;
        const bool has_next = PERSIST && vnext < total_tiles;
#pragma unroll
        for (int i = 0; i < FN; ++i)
#pragma unroll
            for (int j = 0; j < FM; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        // K tile 0 landed; tiles 1 .. NS-1 may still fly
        wait_fly((ntiles < NS ? ntiles : NS) - 1);
        __syncthreads();
        if (!SPLITK || ntiles > 0) read_phase(0, 0, 0);
        // asm MFMAs are opaque to the hazard recognizer (acc init / operands): the zeros are pinned in front of the wait states
#pragma unroll
        for (int i = 0; i < FN; ++i)
#pragma unroll
            for (int j = 0; j < FM; ++j) asm volatile("" : "+v"(acc[i][j]));
        asm volatile("s_nop 7" ::: "memory");

        // one K tile: phases 0 .. P-2 each prefetch their successor; before the LAST phase's MFMAs comes the tile's one
        // barrier (tile t+1 landed, slot of tile t drained), the DMA of tile t+NS and the prefetch of tile t+1's
        // phase 0.  (sched_barrier pins the phase order: left alone, the scheduler sinks the MFMAs behind the barrier
        // and the fragment reads in front of their consumers, which re-exposes the LDS latency this layout hides.)
        auto step = [&](int t, int cur, int nxt, auto par_tag) {
            constexpr int par = decltype(par_tag)::value;      // parity of tile t within this output tile (fp8 only)
#pragma unroll
            for (int p = 0; p < P; ++p) {
                if (p < P - 1) {
                    read_phase(cur, p + 1, par);
                } else if (t + 1 < ntiles) {
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // all my fragments of tile t are in registers
                    const int rem = ntiles - 2 - t;
                    wait_fly(rem < NS - 2 ? rem : NS - 2);                  // my share of tile t+1 has landed
                    __syncthreads();
                    if (!SPREAD && t + NS < ntiles) issue_tile(t + NS, cur);
                    read_phase(nxt, 0, par ^ 1);
                } else if (has_next && PREFETCH_EARLY) {
                    // last K tile of this output tile: every slot is free once all waves have their fragments; the next
                    // output tile's first K tiles fly under this phase's MFMAs and the epilogue
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    __syncthreads();
                    setup_tile(vnext);
#pragma unroll
                    for (int st = 0; st < NS; ++st)
                        if (st < ntiles) issue_tile(st, st);
                }
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (PRIO) __builtin_amdgcn_s_setprio(1);
                // (one MFMA sequence per phase whatever the run-time condition: two alternative asm blocks updating the
                // accumulators make the allocator copy them at the join)
                if constexpr (SPREAD) {
                    if (p == P - 1) mma_phase_dma(p, par, t + NS, cur, t + NS < ntiles);
                    else mma_phase(p, par);
                } else {
                    mma_phase(p, par);
                }
                if constexpr (PRIO) __builtin_amdgcn_s_setprio(0);
                __builtin_amdgcn_sched_barrier(0);
            }
        };
        int t = 0;
        constexpr std::integral_constant<int, 0> even{};
        constexpr std::integral_constant<int, (KS == 1 ? 1 : 0)> odd{};   // 16-bit forms: parity is irrelevant, one body
        if constexpr (NS == 2) {
            for (; t + 1 < ntiles; t += 2) {
                step(t, 0, 1, even);
                step(t + 1, 1, 0, odd);
            }
            if (t < ntiles) step(t, 0, 1, even);
        } else {
            for (; t + 2 < ntiles; t += 3) {
                step(t, 0, 1, even);
                step(t + 1, 1, 2, even);
                step(t + 2, 2, 0, even);
            }
            if (t < ntiles) {
                step(t, 0, 1, even);
                if (t + 1 < ntiles) step(t + 1, 1, 2, even);
            }
        }
        // MFMA results settle before VALU reads them.  The asm MFMAs are opaque to the hazard recognizer, and a bare nop
        // statement does not order register-only instructions: the scheduler is free to hoist the epilogue's first VALU read
        // of an accumulator above it (seen in the folded-LayerNorm tiles: single elements of the LAST fragment written, lanes
        // 48-63, sporadically stale — one wrong column in 16 rows per ~2000 tiles).  Every fragment is therefore re-defined by
        // an empty volatile asm BEHIND the nops: volatile asms keep their order, so no read can move above the wait states.
        asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
#pragma unroll
        for (int i = 0; i < FN; ++i)
#pragma unroll
            for (int j = 0; j < FM; ++j) asm volatile("" : "+v"(acc[i][j]));

        bool staged = false;
        if constexpr (STAGED) {
            constexpr size_t A16 = 15;
            staged = (n_cur + wn * TN + TN <= N) && (((size_t)g.C | (size_t)g.residual | (size_t)g.bias | (size_t)g.rowvec) & A16) == 0 &&
                     ((g.ldc | g.ldr | g.rowvec_ld) & 7) == 0 && (EM == 0 || ((size_t)g.scale_w & A16) == 0);
            if constexpr (STG_IN_RING) {        // the strips live in ring slot 0: every wave must be done reading fragments
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __syncthreads();
            }
            if (staged) {
                // per-value options as compile-time variants (GELU / GEGLU only come with GEMMs, the time-embedding row vector only
                // with convolutions); an unforeseen combination takes the run-time-flag variant
                char* strip = smem_raw + (STG_IN_RING ? 0 : NS * TILE_BYTES) + wid * STG_WAVE;
                const int mb = m_cur + wm * TM, nb = n_cur + wn * TN;
                const bool o_gelu = (g.epi & SS_EPI_GELU) != 0, o_geglu = (g.epi & SS_EPI_GEGLU_PAIR) != 0;
                const bool o_rv = g.rowvec != nullptr || (!CONV && (g.epi & SS_EPI_INTERNAL_GENERIC) != 0);   // A/B knob: run-time flags
                if (!o_gelu && !o_geglu && !o_rv) {
                    gemm_epilogue_staged<TO, FM, FN, STG_CR, EM, RSTAT, 1>(g, acc, mb, nb, lane, strip);
                } else if constexpr (CONV) {   // (ss_conv3x3 has no GELU / GEGLU epilogue: the row vector is the only per-value option)
                    gemm_epilogue_staged<TO, FM, FN, STG_CR, EM, RSTAT, 3>(g, acc, mb, nb, lane, strip);
                } else {
                    if (o_geglu && !o_gelu && !o_rv) gemm_epilogue_staged<TO, FM, FN, STG_CR, EM, RSTAT, 4>(g, acc, mb, nb, lane, strip);
                    else if (o_gelu && !o_geglu && !o_rv) gemm_epilogue_staged<TO, FM, FN, STG_CR, EM, RSTAT, 2>(g, acc, mb, nb, lane, strip);
                    else gemm_epilogue_staged<TO, FM, FN, STG_CR, EM, RSTAT, 0>(g, acc, mb, nb, lane, strip);
                }
            }
        }
        if constexpr (SPLITK) gemm_epilogue_partial<FM, FN>(g, acc, m_cur + wm * TM, n_cur + wn * TN, l15, grp, (int)blockIdx.y);
        else if (!staged) gemm_epilogue<TO, FM, FN, EM, RSTAT>(g, acc, m_cur + wm * TM, n_cur + wn * TN, l15, grp);
        if (!has_next) break;
        if constexpr (!PREFETCH_EARLY) {        // strips drained -> the ring is free for the next output tile
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __syncthreads();
            setup_tile(vnext);
#pragma unroll
            for (int st = 0; st < NS; ++st)
                if (st < ntiles) issue_tile(st, st);
        }
        vid = vnext;
    }
}

template <typename T, int BM, int BN, int WM, int WN, int NH, int NS_, int FLAGS>
static int sp_launch(const GemmArgs& g, hipStream_t s) {
    constexpr bool CONV = SS_SP_CONV != 0;
    constexpr int NS = CONV ? 2 : NS_;            // the conv kernels drain per K tile: a third slot buys nothing there
    const bool conv = g.conv_Cin > 0;
    if (conv != CONV) return 1;
    // the pipelined kernel needs whole 64-wide K tiles (conv: one filter tap per tile) and 32-bit byte offsets
    constexpr int KT = 128 / Mma<T>::kEB;
    const bool ok = (g.K % KT == 0) && (!conv || g.conv_Cin % 64 == 0) && g.K >= KT &&
                    (conv ? (int64_t)g.M * g.conv_stride * g.conv_stride * g.conv_Cin * 2 < (1ll << 31)
                          : ((int64_t)BM * g.lda * Mma<T>::kEB < (1ll << 31))) && (int64_t)BN * g.ldw * Mma<T>::kEB < (1ll << 31);
    if (!ok) return 1;
    if ((g.rowstat_out || g.rowpart) && !(FLAGS & 32)) return 1;    // this instantiation has no statistics epilogue
    constexpr size_t lds = SpLds<BM, BN, WM, WN, NS, FLAGS>::BYTES;
    if ((g.ksplit > 1) != ((FLAGS & 64) != 0)) return 1;    // split-K runs only on its own instantiations
    const int cap = (FLAGS & 2) ? num_cus() * (lds > 80 * 1024 ? 1 : 2) : 0;      // persistent: one or two workgroups per CU
    return launch_tiles<gemm_sp_kernel<T, BM, BN, WM, WN, NH, NS, FLAGS, CONV>>("gemm_sp", g, cdiv(g.M, BM) * cdiv(g.N, BN), cap,
                                                                                64 * WM * WN, lds, s);
}

// cfg -> sp_launch<T, BM, BN, WM, WN, NH, NS, FLAGS> through the tile lists of ss_gemm_common.h.  The variant passes come after
// every base tile (kernels are emitted in the order they are instantiated here).
#define SS_SP_CASE(id, BM, BN, WM, WN, NH, NS, FLAGS, VAR) case id: return sp_launch<T, BM, BN, WM, WN, NH, NS, FLAGS>(g, s);
#define SS_SP_VARIANT(HAS, ID, BM, BN, WM, WN, NH, NS, FLAGS) \
    if constexpr ((HAS) != 0) { if (cfg == (ID)) return sp_launch<T, BM, BN, WM, WN, NH, NS, FLAGS>(g, s); }
#define SS_SP_LNFOLD(id, BM, BN, WM, WN, NH, NS, FLAGS, VAR) SS_SP_VARIANT((VAR) & 1, (id) + 100, BM, BN, WM, WN, NH, NS, (FLAGS) | 16)
#define SS_SP_ROWSTAT(id, BM, BN, WM, WN, NH, NS, FLAGS, VAR) SS_SP_VARIANT((VAR) & 2, (id) + 200, BM, BN, WM, WN, NH, NS, (FLAGS) | 32)
#if defined(SS_SP_FP8)
int gemm_sp_dispatch_fp8(int cfg, const GemmArgs& g, hipStream_t s) {
    using T = fp8_t;
    switch (cfg) {
        SS_SP_FP8_TILES(SS_SP_CASE)
        default: return 1;
    }
}
#else
#if SS_SP_CONV
template <typename T> int gemm_sp_dispatch_conv(int cfg, const GemmArgs& g, hipStream_t s) {
#else
template <typename T> int gemm_sp_dispatch(int cfg, const GemmArgs& g, hipStream_t s) {
#endif
    switch (cfg) {
        SS_SP_TILES(SS_SP_CASE)
#if !SS_SP_CONV
        SS_SP_SPLITK_TILES(SS_SP_CASE)
#endif
        default: break;
    }
#if !SS_SP_CONV
    SS_SP_TILES(SS_SP_ROWSTAT)
    SS_SP_TILES(SS_SP_LNFOLD)
#endif
    return 1;
}

#if SS_SP_CONV
template int gemm_sp_dispatch_conv<SS_SP_T>(int, const GemmArgs&, hipStream_t);
#else
template int gemm_sp_dispatch<SS_SP_T>(int, const GemmArgs&, hipStream_t);
#endif
#endif  // SS_SP_FP8

}  // namespace ss
