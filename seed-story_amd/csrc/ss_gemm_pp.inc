// "Ping-pong" 256x256 / 256x320 GEMM and implicit-GEMM 3x3 convolution for 16-bit dtypes: the 8-phase schedule of
// cdna_hip_programming.md ("The 256^2 8-phase template"), re-derived on this library's LDS tile image, DMA helpers and
// epilogues (K % 64 == 0).  Included by ss_gemm_pp_{bf16,f16}[_conv|_convup].hip with SS_PP_T (element type) and SS_PP_CONV (0 | 1 | 2: upsampled input).
// (The description below is written for the 256-wide tile; the 320-wide one and the two-super-phase variant are described at
// the template parameters / at tile2 inside the kernel.)
//
// Why a second main loop next to ss_gemm_sp.inc: there BOTH waves of a SIMD run the same phase at the same time (fragment
// reads of phase p+1 issued in front of the MFMAs of phase p, one barrier per K tile), so the matrix pipe of a SIMD idles
// whenever its two waves both sit in their read / DMA / barrier stretch — MFMA busy 0.55, 1.1 PFLOP/s on uniform operands.
// Here the two waves of a SIMD are kept half a phase APART for the whole K loop: the 8 waves form two groups (wm = 0 | 1,
// one wave of each per SIMD) that alternate between a MEMORY stretch (ds_read of this phase's operands + one half-tile of
// LDS-DMA prefetch) and an MFMA stretch (16 x v_mfma 16x16x32 = one quadrant of the wave's 128x64 output x K = 64), with a
// workgroup barrier between any two stretches; group 1 executes one barrier more before the loop (and group 0 one more
// after it), so while one group multiplies the other one loads, by construction rather than by the scheduler's luck.
//
// Geometry: 8 waves as 2 (M) x 4 (N); a wave owns rows m_blk + wm*128 .. +127 and columns n_blk + wn*64 .. +63 (contiguous:
// the epilogues of ss_gemm_common.h apply unchanged), as 4 quadrants C[h][h'] = rows h*64.. x columns h'*32...  A K tile
// (64 deep = 128 B per row) lives in LDS as four HALF-TILES of 128 rows x 128 B = 16 KB:
//   A-half h  = the rows { wm*128 + h*64 + [0,64) : wm = 0,1 }   (LDS row wm*64 + r)
//   B-half h' = the W rows { wn*64 + h'*32 + [0,32) : wn = 0..3 } (LDS row wn*32 + r)
// so EVERY wave reads from every half-tile, each in its own phase, and a half-tile can be re-staged as soon as that phase
// is two phases back.  Two K tiles (buffers b = 0 | 1) x 4 half-tiles = 128 KB; chunk c of LDS row r sits at c ^ (r & 7)
// (same conflict-free image as ss_gemm_sp.inc, swizzle applied on the DMA source address).
//
// One K tile t (buffer b = t & 1) = 4 phases; every wave runs, per phase, [memory stretch] barrier [MFMA stretch] barrier:
//   phase 1: read B-half 0 (4 x ds_read_b128) then A-half 0 (8);  DMA A[b^1][1] <- tile t+1;  lgkmcnt(8) (B reads retired
//            BEFORE the barrier, so B[b][0] may be re-staged one phase later);                  MFMA C[0][0] += A0 x B0
//   phase 2: read B-half 1 (4);                                   DMA B[b][0]   <- tile t+2;   MFMA C[0][1] += A0 x B1
//   phase 3: read A-half 1 (8);                                   DMA A[b][0]   <- tile t+2;   MFMA C[1][1] += A1 x B1
//   phase 4: (no reads)                                           DMA B[b][1]   <- tile t+2;   vmcnt(6): everything up to
//            phase 1's DMA has landed = tile t+1 complete;                                     MFMA C[1][0] += A1 x B0
// Ordering rules (guide, same section): a DMA'd buffer is read one phase AFTER the counted vmcnt that retires it (the other
// group's wait sits half a phase later than mine), a buffer is re-staged >= 2 phases after its last ds_read, or 1 phase
// after when an lgkmcnt in front of the reading phase's first barrier retired those reads (phase 1's B reads).  vmcnt is
// never 0 in the steady state: three half-tiles (6 DMA instructions per wave) stay in flight across the wait.
//
// CONV (ss_gemm_pp_*_conv.hip; SS_PP_CONV = 1): implicit-GEMM 3x3 convolution over NHWC, stride 1, no upsampling, whole tiles,
// W a power of two >= 8 (every ResBlock convolution of the SDXL UNet and VAE at 1024^2): K tile t is 64 channels of ONE filter tap,
// the A piece of a wave (8 consecutive output pixels of one image row) reads the same pixels shifted by the tap — an
// affine function of the row index, so the tap is a SCALAR offset on the DMA base and the only per-lane work is the border
// test.  What depends on the piece alone (its pixel offset, which taps need padding and of which kind) is formed once per
// output tile, the tap's offset and mask bits once per tap; a K tile costs a piece one bit test, one scalar add and the DMA.
// Padding: out-of-image lanes read a 16-byte zero page through a 64-bit per-lane address, so EVERY piece is issued
// with a full EXEC mask and the counted vmcnt schedule holds (the one-barrier conv kernel masks the DMA and zero-fills by
// ds_write — a fully masked piece is skipped by the hardware, its count is not constant, and that kernel drains to
// vmcnt(0) every K tile).
// UP (ss_gemm_pp_*_convup.hip; SS_PP_CONV = 2): the same with the input read through a nearest-2x upsampling (output 2H x 2W, both
// powers of two, output W >= 8): a piece is 8 output pixels of one OUTPUT row, its source row (oy + dy) >> 1 is a scalar that moves
// with dy by the parity of oy (re-formed per piece at the tap change), its lanes' source columns are ox0 / 2 + ((r + dx) >> 1): one
// of two loop-invariant lane offsets, picked by the tap.  Padding, masks, K order and the vmcnt schedule are those of CONV.  The
// arithmetic is ss_conv_up.h, shared with a host program that walks every address (tests/conv_up_addr_check.cpp).
//
// FLAGS: 1 s_setprio around the MFMA stretch | 2 persistent (the next output tile's first 7 half-tiles fly under the
// epilogue; 256-wide only) | 4 two super-phases per K tile (tile2) | 8 LDS-staged epilogue (256-wide: strips behind the ring,
// 128 KB + 18 KB; 320-wide: inside ring buffer 0) | 16 folded-LayerNorm epilogue | 32 row statistics (16 / 32: template support
// only, no instantiation selects them).

#include "ss_conv_up.h"

namespace ss {

// LDS layout of a BN-wide tile, for the kernel and its launcher: two K-tile buffers of four half-tiles each, and for the
// LDS-staged epilogue (FLAGS & 8) one strip per wave — behind the ring when both fit the 160 KB of a CU, else inside buffer 0
template <int BN, int FLAGS>
struct PpLds {
    static constexpr int FN = BN / 64, FN0 = (FN + 1) / 2, FN1 = FN / 2, TN = FN * 16;   // a wave's column fragments, halves
    static constexpr int HA = 128 * 128, HB0 = 4 * FN0 * 16 * 128, HB1 = 4 * FN1 * 16 * 128;   // half-tile bytes
    static constexpr int BUF = 2 * HA + HB0 + HB1;
    static constexpr int STG_CR = 16, STG_WAVE = STG_CR * (TN * 2 + 16);
    static constexpr bool STG_IN_RING = 2 * BUF + 8 * STG_WAVE > 163840;
    static constexpr int BYTES = 2 * BUF + ((FLAGS & 8) != 0 && !STG_IN_RING ? 8 * STG_WAVE : 0);
};

static __device__ __attribute__((aligned(4096))) unsigned int g_pp_zero_page[1024];   // zero-initialised: the padding of the conv tiles (4 KB: 256 lanes x 16 B, so padded lanes do not pile onto one cache line)

// one LDS-DMA piece from per-lane 64-bit addresses (M0 is left modified)
__device__ __forceinline__ void dma16v(const char* gsrc, uint32_t lds_base) {
    asm volatile(
        "s_mov_b32 m0, %1\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %0, off"
        :
        : "v"(gsrc), "s"(lds_base)
        : "memory");
}

// the two DMA forms with the LDS destination given as a wave base + a compile-time offset, added on the way into M0: no scalar
// register per destination (the K loop of the conv tiles has 8 A and 8 - 10 B destinations; held in registers they spilled)
__device__ __forceinline__ void dma16s_at(uint32_t voff, const void* sbase, uint32_t lds_wave, int off) {
    asm volatile(
        "s_add_u32 m0, %2, %3\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %0, %1"
        :
        : "v"(voff), "s"(sbase), "s"(lds_wave), "i"(off)
        : "memory", "scc");
}
__device__ __forceinline__ void dma16v_at(const char* gsrc, uint32_t lds_wave, int off) {
    asm volatile(
        "s_add_u32 m0, %1, %2\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %0, off"
        :
        : "v"(gsrc), "s"(lds_wave), "i"(off)
        : "memory", "scc");
}

// a per-lane select by a wave-uniform 64-bit LANE MASK held in an SGPR pair: lane l gets b where bit l of mask is set, else a
__device__ __forceinline__ uint32_t sel_lanes(uint32_t a, uint32_t b, uint64_t mask) {
    uint32_t r;
    asm("v_cndmask_b32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "s"(mask));
    return r;
}
__device__ __forceinline__ uint64_t uniform_u64(uint64_t v) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
}

template <typename T, int BN, int FLAGS, bool CONV, bool UP = false>
__global__ __launch_bounds__(512) void gemm_pp_kernel(const GemmArgs g, const int total_tiles) {
    // BN = 256: wave tile 128x64 (4 column fragments, halves 2 + 2).  BN = 320: wave tile 128x80 (5 column fragments, halves
    // 3 + 2; phases of 24 / 16 / 16 / 24 MFMAs) — [16384, 1280] outputs are exactly 256 tiles = one per CU, [65536, 640] two
    // per CU, where 256-wide tiles waste a fifth of the chip.  BN = 320 takes whole tiles only (M % 256 == 0, N % 320 == 0:
    // the launcher refuses other shapes): 160 accumulator + 72 fragment registers leave no room for per-piece offsets, so
    // the DMA pieces of a half-tile share ONE lane offset and differ by scalar row offsets.
    using Lds = PpLds<BN, FLAGS>;
    constexpr int BM = 256, FN = Lds::FN, FN0 = Lds::FN0, FN1 = Lds::FN1, TM = 128, TN = Lds::TN, FM = 8;
    static_assert(BN == 256 || BN == 320, "tile widths");
    static_assert(CONV || !UP, "upsampling is a conv input");
    constexpr bool EXACT = BN == 320 || CONV;
    constexpr bool PRIO = (FLAGS & 1) != 0, PERSIST = (FLAGS & 2) != 0, TWO = (FLAGS & 4) != 0, STAGED = (FLAGS & 8) != 0, RSTAT = (FLAGS & 32) != 0;
    constexpr int EM = ((FLAGS & 16) != 0) ? 2 : 0;
    constexpr int HA = Lds::HA, HB0 = Lds::HB0, HB1 = Lds::HB1, BUF = Lds::BUF;
    constexpr int OFF_A0 = 0, OFF_A1 = HA, OFF_B0 = 2 * HA, OFF_B1 = 2 * HA + HB0;
    constexpr int NP0 = FN0, NP1 = FN1;                        // DMA pieces per wave of B-half 0 / 1 (A halves: 2 each)
    constexpr int FLY = NP0 + 2 + NP1;                         // DMA instructions in flight across the phase-4 wait
    constexpr int STG_CR = Lds::STG_CR, STG_WAVE = Lds::STG_WAVE;
    constexpr bool STG_IN_RING = Lds::STG_IN_RING;
    static_assert(!(PERSIST && STG_IN_RING), "persistent tiles prefetch under the epilogue: the strips need their own LDS");
    static_assert(Mma<T>::kEB == 2, "16-bit operands");
    using TO = T;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wid >> 2, wn = wid & 3;
    const int l15 = lane & 15, grp = lane >> 4;
    const int M = g.M, N = g.N;
    const int MT = (M + BM - 1) / BM, NT = (N + BN - 1) / BN;
    const int ntiles = g.K / 64;
    // conv: K tiles per filter tap and its reciprocal (tap = t / tpt as a multiply: t < 9 * 40, exact for tpt <= 64)
    const int tpt = CONV ? g.conv_Cin / 64 : 1;
    const uint32_t tpt_inv = CONV ? (65536u + (uint32_t)tpt - 1u) / (uint32_t)tpt : 0u;
    // conv: the OUTPUT grid (UP: twice the source's), both sides powers of two
    const int cWo = UP ? 2 * g.conv_W : g.conv_W, cHo = UP ? 2 * g.conv_H : g.conv_H;
    const int lw = CONV ? __builtin_ctz((unsigned)cWo) : 0;
    const uint32_t lds0 = __builtin_amdgcn_readfirstlane((uint32_t)(size_t)(lds_void_t*)smem_raw);

    // ---- staging coordinates of this wave --------------------------------------------------------------------------
    // piece i of a half-tile = its LDS rows (wid + 8 i) * 8 .. +7.  A-half h: LDS row wm'*64 + r <-> tile row wm'*128 + h*64 + r.
    // B-half h: LDS row wn'*RH + r (RH = 16 * fragments of the half) <-> tile column wn'*TN + (h ? FN0*16 : 0) + r.
    const int srow = lane >> 3;
    const int schunk = (lane & 7) ^ srow;                    // LDS row & 7 == srow for every piece
    auto b_col = [&](int h, int i) {                         // tile column of this lane's row of piece i of B-half h
        const int RH = (h ? FN1 : FN0) * 16;
        const int r8 = (wid + 8 * i) * 8;
        return (r8 / RH) * TN + (h ? FN0 * 16 : 0) + r8 % RH + srow;
    };
    int m_blk = 0, n_blk = 0;
    uint32_t voffA[EXACT ? 1 : 2][EXACT ? 1 : 2], voffW[EXACT ? 1 : 2][EXACT ? 1 : 3];   // [half][piece]
    const char* sbaseA = nullptr;
    const char* sbaseW = nullptr;
    // conv: what the A staging needs of this wave's four pieces (A-half h, piece i: output pixels m0 .. m0 + 7 of one image row,
    // m0 = m_blk + i*128 + h*64 + wid*8), all of it fixed for the whole output tile and all of it scalar:
    //   cpoff[h][i]  the byte offset m0 * Cin * 2 of the piece's first pixel
    //   cpad / crow  bit tap * 4 + h*2 + i: the piece needs padding at this filter tap / all of it is padding (its image row
    //                shifted by the tap lies above or below the image).  A padded piece that is not a whole-row case pads the
    //                one pixel that leaves the image on the left (taps with dx < 0: lane row 0) or on the right (dx > 0: lane row
    //                7); with W = 8 a piece is both borders and the tap's dx decides, as it always did.
    // UP (ss_conv_up.h): cpoff is the offset of the piece's SOURCE pixel (b, oy >> 1, ox0 / 2); the source row moves with the tap's
    // dy by the parity of oy (cshift: bit (dy + 1) * 4 + h*2 + i), so the offset in use is re-formed per tap (Cur::po); the source
    // column of a lane moves with dx: lane row r reads column r >> 1 (dx = 0, voffA) or (r + 1) >> 1 (dx != 0, voffA_odd)
    uint32_t cpoff[CONV ? 2 : 1][CONV ? 2 : 1];
    uint64_t cpad = 0, crow = 0;
    uint32_t cshift = 0, voffA_odd = 0;
    auto setup_tile = [&](int vid) {
        int mt_, nt_;
        xcd_tile_id(g.swz, MT, NT, vid, mt_, nt_);
        m_blk = mt_ * BM; n_blk = nt_ * BN;
        if constexpr (UP) {
            voffA[0][0] = up_lane_off(srow, schunk, g.conv_Cin, false);
            voffA_odd = up_lane_off(srow, schunk, g.conv_Cin, true);
            voffW[0][0] = (uint32_t)((int64_t)srow * g.ldw * 2 + schunk * 16);
            uint64_t pad = 0, row = 0;
            uint32_t shift = 0;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const UpPiece q = up_piece(m_blk + i * 128 + h * 64 + wid * 8, lw, cHo, cWo, g.conv_Cin);
                    row |= q.row9 << (h * 2 + i);
                    pad |= q.pad9 << (h * 2 + i);
                    shift |= up_shift_bits(q.odd, h * 2 + i);
                    cpoff[h][i] = __builtin_amdgcn_readfirstlane(q.off);
                }
            }
            cpad = uniform_u64(pad); crow = uniform_u64(row);
            cshift = __builtin_amdgcn_readfirstlane(shift);
        } else if constexpr (CONV) {
            voffA[0][0] = (uint32_t)(srow * g.conv_Cin * 2 + schunk * 16);       // NHWC, stride 1: pixel m sits at m * Cin
            voffW[0][0] = (uint32_t)((int64_t)srow * g.ldw * 2 + schunk * 16);
            uint64_t pad = 0, row = 0;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const int m0 = m_blk + i * 128 + h * 64 + wid * 8;
                    const int y0 = (m0 >> lw) & (g.conv_H - 1), x0 = m0 & (g.conv_W - 1);
                    // tap = (dy + 1) * 3 + (dx + 1): dy < 0 is taps 0 1 2, dy > 0 taps 6 7 8, dx < 0 taps 0 3 6, dx > 0 taps 2 5 8
                    // (one bit every four: the masks of piece 0, shifted by the piece)
                    const uint64_t r9 = (y0 == 0 ? 0x000000111ull : 0ull) | (y0 == g.conv_H - 1 ? 0x111000000ull : 0ull);
                    const uint64_t p9 = r9 | (x0 == 0 ? 0x001001001ull : 0ull) | (x0 + 8 == g.conv_W ? 0x100100100ull : 0ull);
                    row |= r9 << (h * 2 + i);
                    pad |= p9 << (h * 2 + i);
                    cpoff[h][i] = __builtin_amdgcn_readfirstlane((uint32_t)(m0 * g.conv_Cin * 2));
                }
            }
            cpad = uniform_u64(pad); crow = uniform_u64(row);
        } else if constexpr (EXACT) {
            voffA[0][0] = (uint32_t)((int64_t)srow * g.lda * 2 + schunk * 16);
            voffW[0][0] = (uint32_t)((int64_t)srow * g.ldw * 2 + schunk * 16);
        } else {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    int m = m_blk + i * 128 + h * 64 + wid * 8 + srow;
                    m = m < M ? m : M - 1;
                    voffA[h][i] = (uint32_t)((int64_t)(m - m_blk) * g.lda * 2 + schunk * 16);
                }
#pragma unroll
                for (int i = 0; i < (h ? NP1 : NP0); ++i) {
                    int n = n_blk + b_col(h, i);
                    n = n < N ? n : N - 1;
                    voffW[h][i] = (uint32_t)((int64_t)(n - n_blk) * g.ldw * 2 + schunk * 16);
                }
            }
        }
        sbaseA = uniform_ptr((const char*)g.A + (CONV ? (int64_t)0 : (int64_t)m_blk * g.lda * 2));
        sbaseW = uniform_ptr((const char*)g.W + (int64_t)n_blk * g.ldw * 2);
    };
    // one half-tile of K tile t into buffer b.  which: 0 A0 | 1 A1 | 2 B0 | 3 B1
    // conv: where K tile t of the A operand lives — 64 channels [64 c, 64 c + 64) of filter tap (dy, dx); src = the address of
    // pixel 0's channels shifted by the tap.  All scalar; the K loop advances two cursors (tiles t+1, t+2) incrementally.
    // bits: this tap's four bits of cpad (bits 0..3), of crow (4..7), and dx < 0 (bit 8); UP: dx != 0 (bit 9)
    // po (UP): the four pieces' source offsets at this tap's dy
    struct Cur { const char* src; int c, tap; uint32_t bits; uint32_t po[2][2]; };
    auto cur_set_tap = [&](Cur& k) {                         // all that happens at a tap change: the tap's byte offset and mask bits
        const int t3 = (k.tap * 11) >> 5;                    // tap / 3 for tap < 9
        const int dy = t3 - 1, dx = k.tap - 3 * t3 - 1;
        if constexpr (UP) {
            k.src = (const char*)g.A + up_tap_off(dx, k.c, g.conv_Cin);
            const uint32_t row_bytes = (uint32_t)(g.conv_W * g.conv_Cin * 2);
#pragma unroll
            for (int p = 0; p < 4; ++p) k.po[p >> 1][p & 1] = up_piece_off(cpoff[CONV ? p >> 1 : 0][CONV ? p & 1 : 0], cshift, p, t3, row_bytes);
        } else {
            k.src = (const char*)g.A + ((int64_t)(dy * g.conv_W + dx) * g.conv_Cin + k.c * 64) * 2;
        }
        k.bits = ((uint32_t)(cpad >> (k.tap * 4)) & 15u) | (((uint32_t)(crow >> (k.tap * 4)) & 15u) << 4) | (dx < 0 ? 256u : 0u) |
                 (UP && dx != 0 ? 512u : 0u);
    };
    auto cur_make = [&](int t) {
        Cur k{};
        k.tap = (int)(((uint32_t)t * tpt_inv) >> 16);
        k.c = t - k.tap * tpt;
        cur_set_tap(k);
        return k;
    };
    auto cur_next = [&](Cur& k) {
        k.c += 1; k.src += 128;
        if (k.c == tpt) { k.c = 0; k.tap += 1; cur_set_tap(k); }
    };
    // A-half h of the cursor's K tile into buffer b.  A piece = output pixels m0 .. m0 + 7 of one image row (W % 8 == 0), this
    // lane's pixel m0 + srow.  Per piece and K tile: one bit test, one scalar 64-bit add of the cursor and the piece's offset, one
    // DMA.  Interior pieces (nearly all) take the GEMM form of the DMA (scalar base + lane offset); a piece with padding selects
    // between its source and the zero page per lane (64-bit addresses) by a constant lane mask: every lane (whole-row case), lane
    // row 0 = lanes 0..7 (left border) or lane row 7 = lanes 56..63 (right border).  Every piece is issued with a full EXEC mask.
    const uint32_t ldsw = lds0 + (uint32_t)(wid * 1024);     // this wave's slice of every half-tile
    const uint64_t zaddr = (uint64_t)(size_t)g_pp_zero_page; // 4 KB aligned: the lane's 16 bytes are an OR into the low word
    const uint32_t zlo = (uint32_t)zaddr | (uint32_t)((tid & 255) << 4);
    uint32_t zhi = (uint32_t)(zaddr >> 32);
    // 256-wide tiles have vector registers to spare and (the persistent one) no scalar ones: the high word, which the select needs
    // in a vector register anyway, lives there for good instead of being spilled and re-read as a scalar by every padded piece
    if constexpr (CONV && BN == 256) asm volatile("" : "+v"(zhi));
    auto stage_conv = [&](const Cur& k, int b, int h) {
        const uint32_t keep = m0_save();
        // UP: this tap's lane offset, one select for the two pieces
        const uint32_t vo = UP && (k.bits & 512u) ? voffA_odd : voffA[0][0];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int p = h * 2 + i;
            const char* ps = k.src + (UP ? k.po[h][i] : cpoff[CONV ? h : 0][CONV ? i : 0]);
            const int d = b * BUF + (h ? OFF_A1 : OFF_A0) + i * 8192;   // a constant once inlined
            if (__builtin_expect(((k.bits >> p) & 1u) == 0, 1)) {
                dma16s_at(vo, ps, ldsw, d);
            } else {
                const uint64_t zm = up_pad_lanes(((k.bits >> (4 + p)) & 1u) != 0, (k.bits & 256u) != 0);
                const uint64_t a = (uint64_t)(size_t)ps + vo;
                const uint32_t lo = sel_lanes((uint32_t)a, zlo, zm), hi = sel_lanes((uint32_t)(a >> 32), zhi, zm);
                dma16v_at((const char*)(size_t)(((uint64_t)hi << 32) | lo), ldsw, d);
            }
        }
        m0_restore(keep);
    };
    auto stage = [&](int t, int b, int which) {
        const uint32_t keep = m0_save();
        const int h = which & 1;
        if (which < 2) {
            const uint32_t dst = lds0 + (uint32_t)(b * BUF + (h ? OFF_A1 : OFF_A0) + wid * 1024);
            const char* src = sbaseA + (int64_t)t * 128;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                if constexpr (CONV) {
                    // (conv A halves go through stage_conv)
                } else if constexpr (EXACT)
                    dma16s(voffA[0][0], uniform_ptr(src + (int64_t)(i * 128 + h * 64 + wid * 8) * g.lda * 2), __builtin_amdgcn_readfirstlane(dst + i * 8192u));
                else
                    dma16s(voffA[h][i], src, __builtin_amdgcn_readfirstlane(dst + i * 8192u));
            }
        } else {
            const uint32_t dst = lds0 + (uint32_t)(b * BUF + (h ? OFF_B1 : OFF_B0) + wid * 1024);
            const char* src = sbaseW + (int64_t)t * 128;
#pragma unroll
            for (int i = 0; i < (h ? NP1 : NP0); ++i) {
                if constexpr (CONV)
                    // (the row offset fits 32 bits: pp_launch checks BN * ldw * 2 < 2^31)
                    dma16s_at(voffW[0][0], src + (uint32_t)__builtin_amdgcn_readfirstlane((b_col(h, i) - srow) * g.ldw * 2), ldsw,
                              b * BUF + (h ? OFF_B1 : OFF_B0) + i * 8192);
                else if constexpr (EXACT)
                    dma16s(voffW[0][0], uniform_ptr(src + (int64_t)(b_col(h, i) - srow) * g.ldw * 2), __builtin_amdgcn_readfirstlane(dst + i * 8192u));
                else
                    dma16s(voffW[h][i], src, __builtin_amdgcn_readfirstlane(dst + i * 8192u));
            }
        }
        m0_restore(keep);
    };
    auto prologue = [&]() {                                  // tile 0 whole, tile 1 minus A-half 1 (phase 1 of tile 0 brings it)
        // (TWO: tile 1 brings A0 and B0 only — super-phase X of tile 0 stages its B1 and A1)
        if constexpr (CONV) {
            const Cur k0 = cur_make(0);
            stage(0, 0, 2); stage_conv(k0, 0, 0); stage(0, 0, 3); stage_conv(k0, 0, 1);
            if (ntiles > 1) { stage_conv(cur_make(1), 1, 0); stage(1, 1, 2); if constexpr (!TWO) stage(1, 1, 3); }
        } else {
            stage(0, 0, 2); stage(0, 0, 0); stage(0, 0, 3); stage(0, 0, 1);
            if (ntiles > 1) { stage(1, 1, 0); stage(1, 1, 2); if constexpr (!TWO) stage(1, 1, 3); }
        }
    };

    // ---- fragment addressing: LDS row r at r*128, chunk c at (c ^ (r & 7)) << 4; k-step 1 = k-step 0 XOR 64 ------------
    const uint32_t fsw = (uint32_t)((grp ^ (l15 & 7)) << 4);
    const uint32_t fa0 = (uint32_t)((wm * 64 + l15) * 128) + fsw, fa1 = fa0 ^ 64u;
    const uint32_t fw00 = (uint32_t)((wn * FN0 * 16 + l15) * 128) + fsw, fw01 = fw00 ^ 64u;     // B-half 0
    const uint32_t fw10 = (uint32_t)((wn * FN1 * 16 + l15) * 128) + fsw, fw11 = fw10 ^ 64u;     // B-half 1 (FN0 == FN1: same registers)
    // A fragments are single-buffered: half 0 is dead after phase 2, half 1 is read in phase 3 (an LDS return lands long after
    // the last MFMA of phase 2 has fetched its operands)
    uint4 fa[4][2], fw0[FN0][2], fw1[FN1][2];                // [fragment][k-step]
    auto read_a = [&](const char* half) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            fa[j][0] = *reinterpret_cast<const uint4*>(half + fa0 + j * 2048);
            fa[j][1] = *reinterpret_cast<const uint4*>(half + fa1 + j * 2048);
        }
    };
    auto read_w0 = [&](const char* half) {
#pragma unroll
        for (int i = 0; i < FN0; ++i) {
            fw0[i][0] = *reinterpret_cast<const uint4*>(half + fw00 + i * 2048);
            fw0[i][1] = *reinterpret_cast<const uint4*>(half + fw01 + i * 2048);
        }
    };
    auto read_w1 = [&](const char* half) {
#pragma unroll
        for (int i = 0; i < FN1; ++i) {
            fw1[i][0] = *reinterpret_cast<const uint4*>(half + fw10 + i * 2048);
            fw1[i][1] = *reinterpret_cast<const uint4*>(half + fw11 + i * 2048);
        }
    };
    f32x4_t acc[FN][FM];
    auto mma = [&](int h, auto hp_tag) {                     // C[h][hp] += A-half h x B-half hp, K = 64: 16 (24) MFMAs
        constexpr int hp = decltype(hp_tag)::value;
        if constexpr (PRIO) __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int i = 0; i < (hp ? FN1 : FN0); ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if constexpr (hp == 0) Mma<T>::run_inplace(fw0[i][ks], fa[j][ks], acc[i][h * 4 + j]);
                    else Mma<T>::run_inplace(fw1[i][ks], fa[j][ks], acc[FN0 + i][h * 4 + j]);
                }
        if constexpr (PRIO) __builtin_amdgcn_s_setprio(0);
    };
    constexpr std::integral_constant<int, 0> H0{};
    constexpr std::integral_constant<int, 1> H1{};
    auto bar = [&]() { __builtin_amdgcn_s_barrier(); };
    auto pin = [&]() { __builtin_amdgcn_sched_barrier(0); };

    int vid = blockIdx.x;
    // (measured and dropped, profiles/round6_stagger.txt: a start-up stagger of the first workgroup of each CU — sleep (id / 8) % 8
    // units — so that the CUs' prologue bursts and epilogue stores do not coincide: every unit of delay made every multi-round launch
    // slower, ff1 343 -> 344 / 358 / 370 us; the per-tile fixed cost of ~11 us is not a synchronised-burst effect)
    setup_tile(vid);
    prologue();
    bool first = true;

    while (true) {
        const int m_cur = m_blk, n_cur = n_blk;
        const int vnext = vid + (int)gridDim.x;
        const bool has_next = PERSIST && vnext < total_tiles;
#pragma unroll
        for (int i = 0; i < FN; ++i)
#pragma unroll
            for (int j = 0; j < FM; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        // K tile 0 landed (the later output tiles also drain the previous epilogue's stores: they share the counter)
        if (first && ntiles > 1) wait_vmcnt<(TWO ? 2 + NP0 : FLY)>(); else wait_vmcnt<0>();
        first = false;
        bar();
#pragma unroll
        for (int i = 0; i < FN; ++i)
#pragma unroll
            for (int j = 0; j < FM; ++j) asm volatile("" : "+v"(acc[i][j]));
        asm volatile("s_nop 7" ::: "memory");
        if (wm == 1) bar();                                  // group 1 runs half a phase behind group 0 from here on
        Cur P1 = cur_make(CONV ? 1 : 0), P2 = cur_make(CONV ? 2 : 0);   // conv: the A cursors of K tiles t+1 and t+2

        auto tile = [&](int t, auto btag) {
            constexpr int b = decltype(btag)::value;
            const char* L = smem_raw + b * BUF;
            const bool s1 = t + 1 < ntiles, s2 = t + 2 < ntiles;   // wave-uniform
            // ---- phase 1 ----
            read_w0(L + OFF_B0);
            pin();
            read_a(L + OFF_A0);
            pin();
            if (s1) { if constexpr (CONV) stage_conv(P1, b ^ 1, 1); else stage(t + 1, b ^ 1, 1); }
            asm volatile("s_waitcnt lgkmcnt(8)" ::: "memory");
            bar();
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            pin();
            mma(0, H0);
            pin();
            bar();
            // ---- phase 2 ----
            read_w1(L + OFF_B1);
            pin();
            if (s2) stage(t + 2, b, 2);
            bar();
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            pin();
            mma(0, H1);
            pin();
            bar();
            // ---- phase 3 ----
            read_a(L + OFF_A1);
            pin();
            if (s2) { if constexpr (CONV) stage_conv(P2, b, 0); else stage(t + 2, b, 0); }
            bar();
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            pin();
            mma(1, H1);
            pin();
            bar();
            // ---- phase 4 ----
            if (s2) { stage(t + 2, b, 3); wait_vmcnt<FLY>(); } else { wait_vmcnt<0>(); }
            bar();
            pin();
            mma(1, H0);
            pin();
            bar();
            if constexpr (CONV) { P1 = P2; cur_next(P2); }
        };
        // TWO (FLAGS & 4): the same K tile as TWO super-phases X, Y = 4 barriers instead of 8 (each barrier interval idles the matrix
        // pipe for the release + restart, ~100 cycles of the 256-384 a stretch lasts):
        //   X: read B0, B1, A0 (all retired by lgkmcnt(0) BEFORE the first barrier, so every buffer may be re-staged one
        //      super-phase after its last read);  DMA B1[b^1], A1[b^1] <- tile t+1;  vmcnt: A1[b] of THIS tile (staged in X of
        //      tile t-1) has landed -> read in Y;                                          MFMA A0 x B0, A0 x B1 (40)
        //   Y: read A1;  DMA A0[b], B0[b] <- tile t+2;  vmcnt: A0, B0 (staged in Y of t-1) and B1 (X of t) of tile t+1 have
        //      landed -> read in X of t+1;                                                  MFMA A1 x B1, A1 x B0 (40)
        auto tile2 = [&](int t, auto btag) {
            constexpr int b = decltype(btag)::value;
            const char* L = smem_raw + b * BUF;
            const bool s1 = t + 1 < ntiles, s2 = t + 2 < ntiles;   // wave-uniform
            // ---- X ----
            read_w0(L + OFF_B0);
            read_w1(L + OFF_B1);
            read_a(L + OFF_A0);
            pin();
            if (s1) {
                stage(t + 1, b ^ 1, 3);
                if constexpr (CONV) stage_conv(P1, b ^ 1, 1); else stage(t + 1, b ^ 1, 1);
                wait_vmcnt<4 + NP0 + NP1>();
            } else {
                wait_vmcnt<0>();
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            bar();
            pin();
            mma(0, H0);
            mma(0, H1);
            pin();
            bar();
            // ---- Y ----
            read_a(L + OFF_A1);
            pin();
            if (s2) {
                if constexpr (CONV) stage_conv(P2, b, 0); else stage(t + 2, b, 0);
                stage(t + 2, b, 2);
                wait_vmcnt<4 + NP0>();
            } else if (s1) {
                wait_vmcnt<2>();
            } else {
                wait_vmcnt<0>();
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            bar();
            pin();
            mma(1, H1);
            mma(1, H0);
            pin();
            bar();
            if constexpr (CONV) { P1 = P2; cur_next(P2); }
        };
        int t = 0;
        for (; t + 1 < ntiles; t += 2) {
            if constexpr (TWO) { tile2(t, std::integral_constant<int, 0>{}); tile2(t + 1, std::integral_constant<int, 1>{}); }
            else { tile(t, std::integral_constant<int, 0>{}); tile(t + 1, std::integral_constant<int, 1>{}); }
        }
        if (t < ntiles) { if constexpr (TWO) tile2(t, std::integral_constant<int, 0>{}); else tile(t, std::integral_constant<int, 0>{}); }
        if (wm == 0) bar();                                  // groups level again: every fragment read of this output tile is done

        if (has_next) {                                      // every ring slot is free: the next output tile starts flying now
            setup_tile(vnext);
            prologue();
        }
        // MFMA results settle before VALU reads them (asm MFMAs are opaque to the hazard recognizer; see ss_gemm_sp.inc)
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
            if (staged) {
                // strips behind the ring when both fit the 160 KB of a CU, else inside buffer 0 (free: the groups are level)
                char* strip = smem_raw + (STG_IN_RING ? 0 : 2 * BUF) + wid * STG_WAVE;
                const int mb = m_cur + wm * TM, nb = n_cur + wn * TN;
                const bool o_gelu = (g.epi & SS_EPI_GELU) != 0, o_geglu = (g.epi & SS_EPI_GEGLU_PAIR) != 0;
                const bool o_rv = g.rowvec != nullptr || (!CONV && (g.epi & SS_EPI_INTERNAL_GENERIC) != 0);
                if constexpr (EM == 0 && !RSTAT) {
                    // the chunk pipeline (gemm_epilogue_staged_pipe; tuning knob gemm_epi_generic = 1 keeps the run-time-flag form)
                    const bool o_res = (g.epi & SS_EPI_RESIDUAL) != 0;
                    if (!o_gelu && !o_geglu && !o_rv && !o_res) gemm_epilogue_staged_pipe<TO, FM, FN, 1, false, EXACT>(g, acc, mb, nb, lane, strip);
                    else if (!o_gelu && !o_geglu && !o_rv) gemm_epilogue_staged_pipe<TO, FM, FN, 1, true, EXACT>(g, acc, mb, nb, lane, strip);
                    else if (CONV && !o_gelu && !o_geglu && !o_res && (g.rows_per_batch & 15) == 0) gemm_epilogue_staged_pipe<TO, FM, FN, 3, false, EXACT>(g, acc, mb, nb, lane, strip);
                    else if (!CONV && o_geglu && !o_gelu && !o_rv && !o_res) gemm_epilogue_staged_pipe<TO, FM, FN, 4, false, EXACT>(g, acc, mb, nb, lane, strip);
                    else if (!CONV && o_gelu && !o_geglu && !o_rv && !o_res) gemm_epilogue_staged_pipe<TO, FM, FN, 2, false, EXACT>(g, acc, mb, nb, lane, strip);
                    else gemm_epilogue_staged<TO, FM, FN, STG_CR, EM, RSTAT, 0>(g, acc, mb, nb, lane, strip);
                } else {
                if (!o_gelu && !o_geglu && !o_rv) gemm_epilogue_staged<TO, FM, FN, STG_CR, EM, RSTAT, 1>(g, acc, mb, nb, lane, strip);
                else if constexpr (CONV) gemm_epilogue_staged<TO, FM, FN, STG_CR, EM, RSTAT, 3>(g, acc, mb, nb, lane, strip);
                else if (o_geglu && !o_gelu && !o_rv) gemm_epilogue_staged<TO, FM, FN, STG_CR, EM, RSTAT, 4>(g, acc, mb, nb, lane, strip);
                else if (o_gelu && !o_geglu && !o_rv) gemm_epilogue_staged<TO, FM, FN, STG_CR, EM, RSTAT, 2>(g, acc, mb, nb, lane, strip);
                else gemm_epilogue_staged<TO, FM, FN, STG_CR, EM, RSTAT, 0>(g, acc, mb, nb, lane, strip);
                }
            }
        }
        if (!staged) gemm_epilogue<TO, FM, FN, EM, RSTAT>(g, acc, m_cur + wm * TM, n_cur + wn * TN, l15, grp);
        if (!has_next) break;
        // the staging coordinates of the next tile are RE-computed behind the epilogue (from a laundered tile id, so the
        // compiler cannot keep the 8 offset registers + 2 base pairs alive across it: with them the epilogue spilled)
        vid = vnext;
        asm volatile("" : "+s"(vid));
        setup_tile(vid);
    }
}

template <typename T, int BN, int FLAGS>
static int pp_launch(const GemmArgs& g, hipStream_t s) {
    constexpr bool CONV = SS_PP_CONV != 0, UP = SS_PP_CONV == 2;
    const bool conv = g.conv_Cin > 0;
    if (conv != CONV || (conv && (g.conv_up != 0) != UP) || g.ksplit > 1) return 1;
    // (tests/kernel_check.py pp320_eligible / conv_pp320_eligible copy the rule below to make sure their shapes reach the 320-wide
    // tiles and not the fallback: change both together; the copy there knows no upsampling, tests/test_conv_pp_upsample_gpu.py
    // up_pp_eligible is the copy of the conv_up form)
    bool ok = (g.K % 64 == 0) && g.K >= 64 && (int64_t)BN * g.ldw * 2 < (1ll << 31);
    if (conv) {
        // whole tiles, stride 1, OUTPUT W a power of two >= 8 (an 8-pixel DMA piece stays inside one image row), output H a
        // power of two (the row index is split by shifts), <= 64 K tiles per tap (the reciprocal in the kernel).  With the nearest-2x
        // upsampled input (conv_up; the *_convup.hip instantiations) the output grid is 2H x 2W and the source has M / 4 pixels.
        const int Wo = g.conv_up ? 2 * g.conv_W : g.conv_W, Ho = g.conv_up ? 2 * g.conv_H : g.conv_H;
        ok = ok && g.conv_stride == 1 && g.conv_Cin % 64 == 0 && g.conv_Cin <= 4096 && g.conv_W > 0 && g.conv_H > 0 && Wo >= 8 &&
             (Wo & (Wo - 1)) == 0 && (Ho & (Ho - 1)) == 0 && g.M % 256 == 0 && g.N % BN == 0 &&
             (int64_t)(g.conv_up ? g.M / 4 : g.M) * g.conv_Cin * 2 < (1ll << 31);   // source pixel offsets (pixel * Cin * 2) are formed in 32 bits
    } else {
        ok = ok && (int64_t)256 * g.lda * 2 < (1ll << 31);
        if (BN == 320 && (g.M % 256 != 0 || g.N % 320 != 0)) ok = false;       // whole tiles only (see the kernel)
    }
    if (!ok) return 1;
    if ((g.rowstat_out || g.rowpart) && !(FLAGS & 32)) return 1;
    return launch_tiles<gemm_pp_kernel<T, BN, FLAGS, CONV, UP>>("gemm_pp", g, cdiv(g.M, 256) * cdiv(g.N, BN), (FLAGS & 2) ? num_cus() : 0, 512,
                                                            PpLds<BN, FLAGS>::BYTES, s);
}

// cfg 50 .. 59: the ping-pong tiles
#if SS_PP_CONV == 2
template <typename T> int gemm_pp_dispatch_convup(int cfg, const GemmArgs& g, hipStream_t s) {
#elif SS_PP_CONV
template <typename T> int gemm_pp_dispatch_conv(int cfg, const GemmArgs& g, hipStream_t s) {
#else
template <typename T> int gemm_pp_dispatch(int cfg, const GemmArgs& g, hipStream_t s) {
#endif
    switch (cfg) {
        // (measured, profiles/round6_pp_ubench.txt: s_setprio around the MFMA stretch — FLAGS 1 — changes nothing here, the two
        // groups never compete for the matrix pipe; direct epilogue 772 vs staged 716 us at 8192^3)
        case 54: return pp_launch<T, 256, 8>(g, s);      // 256x256, LDS-staged epilogue
#if SS_PP_CONV != 2
        case 55: return pp_launch<T, 256, 10>(g, s);     // + persistent
#endif
        case 56: return pp_launch<T, 320, 8>(g, s);      // 256x320 (whole tiles only), staged epilogue (strips in the ring)
        case 57: return pp_launch<T, 256, 12>(g, s);     // 256x256, two super-phases per K tile (4 barriers)
#if SS_PP_CONV != 2
        case 58: return pp_launch<T, 320, 12>(g, s);     // 256x320, two super-phases.  (Its conv instantiation once spilled 17 registers
        // INSIDE the K loop and returned wrong tiles on every run: spill moves next to asm MFMAs the hazard recognizer cannot see.
        // Since the per-tile masks of the conv staging the listing of <320, 12, true> has no scratch access between its first and last
        // MFMA, bf16 and f16 — profiles/conv_up_isa.txt.)
#endif
        // Upsampled input (SS_PP_CONV == 2) has no cfg 55 and no cfg 58, which then fall back to the one-barrier tile: <320, 12, true, true>
        // DOES spill inside the K loop (43 - 49 scratch accesses in the listing), and the persistent <256, 10> keeps the scratch loads on
        // its padded-piece paths that the stride-1 one has in f16, with no table entry that would select it for a convolution.
        default: return 1;
    }
}
#if SS_PP_CONV == 2
template int gemm_pp_dispatch_convup<SS_PP_T>(int, const GemmArgs&, hipStream_t);
#elif SS_PP_CONV
template int gemm_pp_dispatch_conv<SS_PP_T>(int, const GemmArgs&, hipStream_t);
#else
template int gemm_pp_dispatch<SS_PP_T>(int, const GemmArgs&, hipStream_t);
#endif

}  // namespace ss
