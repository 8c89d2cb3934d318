// Host walk of the A staging of the ping-pong conv3x3 tiles with a nearest-2x upsampled input: composes the functions of
// seed-story_amd/csrc/ss_conv_up.h exactly as gemm_pp_kernel does (setup_tile -> cur_set_tap -> stage_conv) and, for EVERY
// (output tile, wave, piece, tap, K tile of the tap, lane), checks that the address a lane hands to the DMA
//   - is the zero page, or lies inside the source tensor (all 16 bytes of it), and
//   - equals the definition of the one-barrier kernels: source pixel (b, (oy + dy) >> 1, (ox + dx) >> 1), channel 64 c + 8 chunk,
//     zero where oy + dy or ox + dx leaves the upsampled 2H x 2W grid.
// Every load of a real address goes through an allocation of the tensor's exact size, so an out-of-range address also trips
// the address sanitizer this program is meant to be built with.  No GPU, no library.
//
//   conv_up_addr_check B,Ci,H_in,W_in ...      exit status 0 = every case clean
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "ss_conv_up.h"

using namespace ss;

static int ctz(unsigned v) { int n = 0; while (!(v & 1u)) { v >>= 1; ++n; } return n; }

static long check_case(int B, int Cin, int H, int W) {
    const int Ho = 2 * H, Wo = 2 * W, M = B * Ho * Wo, lw = ctz((unsigned)Wo), tpt = Cin / 64;
    if (M % 256 || Cin % 64 || Wo < 8 || (Wo & (Wo - 1)) || (Ho & (Ho - 1))) { fprintf(stderr, "shape not eligible\n"); return -1; }
    // the source tensor: element (pixel, channel) holds its own index, so a load proves which element an address names
    const size_t n_src = (size_t)B * H * W * Cin;
    std::vector<uint16_t> tag(n_src);                         // 2 bytes per element as in the kernel; the value is a checksum
    for (size_t e = 0; e < n_src; ++e) tag[e] = (uint16_t)(e * 40503u >> 3);
    const char* A = (const char*)tag.data();
    const int64_t src_bytes = (int64_t)n_src * 2;
    const uint32_t row_bytes = (uint32_t)(W * Cin * 2);
    const uint64_t ZERO = ~0ull;                              // stands for the zero page
    long bad = 0, seen = 0;
    for (int m_blk = 0; m_blk < M; m_blk += 256)
        for (int wid = 0; wid < 8; ++wid) {
            // ---- setup_tile ----
            uint32_t cpoff[2][2], cshift = 0;
            uint64_t cpad = 0, crow = 0;
            for (int h = 0; h < 2; ++h)
                for (int i = 0; i < 2; ++i) {
                    const UpPiece q = up_piece(m_blk + i * 128 + h * 64 + wid * 8, lw, Ho, Wo, Cin);
                    crow |= q.row9 << (h * 2 + i);
                    cpad |= q.pad9 << (h * 2 + i);
                    cshift |= up_shift_bits(q.odd, h * 2 + i);
                    cpoff[h][i] = q.off;
                }
            for (int tap = 0; tap < 9; ++tap) {
                // ---- cur_set_tap ----
                const int t3 = (tap * 11) >> 5, dy = t3 - 1, dx = tap - 3 * t3 - 1;
                const uint32_t bits = ((uint32_t)(cpad >> (tap * 4)) & 15u) | (((uint32_t)(crow >> (tap * 4)) & 15u) << 4) |
                                      (dx < 0 ? 256u : 0u) | (dx != 0 ? 512u : 0u);
                for (int c = 0; c < tpt; ++c) {
                    const int64_t src = up_tap_off(dx, 0, Cin) + (int64_t)c * 128;      // cur_next: + 128 per K tile of the tap
                    if (src != up_tap_off(dx, c, Cin)) { ++bad; continue; }
                    // ---- stage_conv ----
                    for (int p = 0; p < 4; ++p) {
                        const uint32_t po = up_piece_off(cpoff[p >> 1][p & 1], cshift, p, t3, row_bytes);
                        const bool padded = ((bits >> p) & 1u) != 0;
                        const uint64_t zm = padded ? up_pad_lanes(((bits >> (4 + p)) & 1u) != 0, (bits & 256u) != 0) : 0ull;
                        const int m0 = m_blk + (p & 1) * 128 + (p >> 1) * 64 + wid * 8;
                        for (int lane = 0; lane < 64; ++lane) {
                            const int srow = lane >> 3, chunk = lane & 7;      // (the LDS swizzle permutes chunks within a row only)
                            const uint32_t vo = up_lane_off(srow, chunk, Cin, (bits & 512u) != 0);
                            // 64-bit: scalar base (cursor + zero-extended piece offset) + zero-extended lane offset
                            const int64_t off = src + (int64_t)(uint64_t)po + (int64_t)(uint64_t)vo;
                            const uint64_t got = ((zm >> lane) & 1u) ? ZERO : (uint64_t)off;
                            // ---- the definition ----
                            const int m = m0 + srow, ox = m & (Wo - 1), oy = (m >> lw) & (Ho - 1), b = m >> lw >> ctz((unsigned)Ho);
                            const int iy = oy + dy, ix = ox + dx;
                            uint64_t want = ZERO;
                            if (iy >= 0 && iy < Ho && ix >= 0 && ix < Wo)
                                want = (uint64_t)(((((int64_t)b * H + (iy >> 1)) * W + (ix >> 1)) * Cin + c * 64 + chunk * 8) * 2);
                            ++seen;
                            bool ok = got == want;
                            if (got != ZERO) {
                                if (off < 0 || off + 16 > src_bytes) ok = false;
                                else {
                                    const uint16_t v = *(const uint16_t*)(A + off);      // in bounds by the test above; ASan agrees or aborts
                                    if (v != tag[(size_t)off / 2]) ok = false;
                                }
                            }
                            if (!ok && bad++ < 8)
                                fprintf(stderr, "B=%d Ci=%d H=%d W=%d tile %d wave %d piece %d tap %d c %d lane %d: got %lld want %lld\n", B, Cin, H,
                                        W, m_blk / 256, wid, p, tap, c, lane, (long long)got, (long long)want);
                        }
                    }
                }
            }
        }
    printf("B=%d Ci=%d H=%d W=%d: %ld addresses, %ld wrong\n", B, Cin, H, W, seen, bad);
    return bad;
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s B,Ci,H_in,W_in ...\n", argv[0]); return 2; }
    long bad = 0;
    for (int a = 1; a < argc; ++a) {
        int B, Ci, H, W;
        if (sscanf(argv[a], "%d,%d,%d,%d", &B, &Ci, &H, &W) != 4) { fprintf(stderr, "bad case %s\n", argv[a]); return 2; }
        const long r = check_case(B, Ci, H, W);
        if (r < 0) return 2;
        bad += r;
    }
    return bad ? 1 : 0;
}
