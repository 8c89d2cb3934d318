// Source-offset and padding-mask arithmetic of the A staging of the ping-pong conv3x3 tiles when the input is read through a
// nearest-neighbour 2x upsampling (ss_gemm_pp.inc, CONV && UP).  Plain C++ on integers: the kernel calls these functions, and so
// does tests/conv_up_addr_check.cpp on the host, which walks every (tile, wave, piece, tap, lane) of a shape and compares the
// composed address with the definition ((oy + dy) >> 1, (ox + dx) >> 1) of the one-barrier kernels.
//
// Geometry: the source is NHWC [B, H, W, Cin]; the output grid is Ho x Wo = 2H x 2W, both powers of two, Wo >= 8.  A piece is the
// 8 output pixels ox0 .. ox0 + 7 (ox0 % 8 == 0) of output row oy of image b, first output pixel m0 = (b * Ho + oy) * Wo + ox0; its
// lane row i (0..7) is output pixel ox0 + i.  For tap = (dy + 1) * 3 + (dx + 1) the source pixel of lane row i is
//   row  (oy + dy) >> 1          = (oy >> 1) + { -1 when dy < 0 and oy is even | +1 when dy > 0 and oy is odd | 0 }     (scalar)
//   col  (ox0 + i + dx) >> 1     = ox0 / 2 + ((i + dx) >> 1)
// The lane term (i + dx) >> 1 is i >> 1 for dx = 0; for dx = +1 it is (i + 1) >> 1 and for dx = -1 it is ((i + 1) >> 1) - 1:
// TWO lane offsets (i >> 1 and (i + 1) >> 1, both >= 0 as the scalar-base form of the DMA needs) and a scalar bias of one source
// pixel for dx < 0 cover the three taps.  The address of a lane is
//   A + up_tap_off(tap, c) + up_piece_off(piece, dy) + up_lane_off(i, chunk, dx != 0)
// and it is replaced by the zero page where up_pad_lanes() has the lane's bit set.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SS_UP_HD __host__ __device__ __forceinline__
#else
#define SS_UP_HD inline
#endif

namespace ss {

// what is fixed for a piece during a whole output tile
struct UpPiece {
    uint32_t off;    // byte offset of source pixel (b, oy >> 1, ox0 / 2)
    uint32_t odd;    // oy & 1
    uint64_t row9;   // bit tap * 4: the piece's output row shifted by the tap's dy lies outside [0, Ho): all of it is padding
    uint64_t pad9;   // bit tap * 4: the piece needs padding at this tap (row9, or the left / right border with the tap's dx)
};

SS_UP_HD UpPiece up_piece(int m0, int lwo, int Ho, int Wo, int Cin) {
    const int ox0 = m0 & (Wo - 1), r = m0 >> lwo;             // r = b * Ho + oy
    const int oy = r & (Ho - 1);
    // source pixel index: (b * H + (oy >> 1)) * W + ox0 / 2, with H = Ho / 2, W = Wo / 2 and b * H = (r - oy) >> 1
    const int sp = (((r - oy) >> 1) + (oy >> 1)) * (Wo >> 1) + (ox0 >> 1);
    UpPiece p;
    p.off = (uint32_t)sp * (uint32_t)Cin * 2u;
    p.odd = (uint32_t)(oy & 1);
    // tap = (dy + 1) * 3 + (dx + 1): dy < 0 is taps 0 1 2, dy > 0 taps 6 7 8, dx < 0 taps 0 3 6, dx > 0 taps 2 5 8
    p.row9 = (oy == 0 ? 0x000000111ull : 0ull) | (oy == Ho - 1 ? 0x111000000ull : 0ull);
    p.pad9 = p.row9 | (ox0 == 0 ? 0x001001001ull : 0ull) | (ox0 + 8 == Wo ? 0x100100100ull : 0ull);
    return p;
}

// bit dyi * 4 + piece (dyi = dy + 1) of a tile's shift mask: the source row of this piece moves by dy at this dy
SS_UP_HD uint32_t up_shift_bits(uint32_t odd, int piece) { return (odd ? 0x100u : 0x001u) << piece; }

// the piece's byte offset at a tap row dy (dyi = dy + 1); `shift` = the tile's shift mask, row_bytes = W * Cin * 2 of the source.
// (A piece whose shifted row leaves the image wraps here; all its lanes read the zero page.)
SS_UP_HD uint32_t up_piece_off(uint32_t off, uint32_t shift, int piece, int dyi, uint32_t row_bytes) {
    const uint32_t d = dyi == 0 ? 0u - row_bytes : row_bytes;
    return off + (((shift >> (dyi * 4 + piece)) & 1u) ? d : 0u);
}

// byte offset from the tensor base of K tile (tap, c): channels [64 c, 64 c + 64), biased by one source pixel for dx < 0
SS_UP_HD int64_t up_tap_off(int dx, int c, int Cin) { return ((int64_t)(dx < 0 ? -Cin : 0) + (int64_t)c * 64) * 2; }

// lane offsets: lane row i (0..7), 16-byte chunk (already swizzled); odd = the tap has dx != 0
SS_UP_HD uint32_t up_lane_off(int i, int chunk, int Cin, bool odd) {
    return (uint32_t)(((i + (odd ? 1 : 0)) >> 1) * Cin * 2 + chunk * 16);
}

// the lanes of a padded piece that read the zero page: all of them (whole-row case), lane row 0 (left border, dx < 0) or lane
// row 7 (right border, dx > 0)
SS_UP_HD uint64_t up_pad_lanes(bool whole_row, bool dx_neg) { return whole_row ? ~0ull : (dx_neg ? 0xFFull : 0xFFull << 56); }

}  // namespace ss
