// Device-pointer entry points of the decode projection (ss_gemv.hip) for the other translation units of the library.
#pragma once
#include "ss_common.h"

namespace ss {

// y[b][N] = W[N,K] . x[b][K] for nb <= 16 sequences, rows x_ld / y_ld / res_ld elements apart; done_flag: optional device flags,
// one per sequence and done_stride ints apart: the launch is skipped when every sequence's flag is set
int gemv_batched_dev(const void* W, const void* x, void* y, int64_t N, int64_t K, const void* norm_w, float eps,
                     const void* bias, const void* residual, int epi, const int32_t* done_flag, int done_stride,
                     int nb, int64_t x_ld, int64_t y_ld, int64_t res_ld, int dtype, hipStream_t s);
int gemv_dev(const void* W, const void* x, void* y, int64_t N, int64_t K, const void* norm_w, float eps,
             const void* bias, const void* residual, int epi, const int32_t* done_flag, int dtype, hipStream_t s);

// The same projection over quantised weights (kind = GEMV_WQ_*), x / y / bias / residual / norm_w in the 16-bit model dtype:
//   GEMV_WQ_FP8    codes [N, K] bytes (OCP e4m3fn), scales fp32 [N]: one per row ([2N] for the SiLU pair);
//   GEMV_WQ_MXFP4  codes [N, K / 2] bytes (two e2m1 codes per byte, even k in the low nibble), scales [N, K / 32] e8m0 bytes, one per
//                  32 consecutive k ([2N, ...] for the SiLU pair).
// gemv_wq_check: the shape rules alone (no launch).
enum { GEMV_WQ_FP8 = 1, GEMV_WQ_MXFP4 = 2 };
int gemv_wq_batched_dev(int kind, const void* codes, const void* scales, const void* x, void* y, int64_t N, int64_t K, const void* norm_w,
                        float eps, const void* bias, const void* residual, int epi, const int32_t* done_flag, int done_stride,
                        int nb, int64_t x_ld, int64_t y_ld, int64_t res_ld, int dtype, hipStream_t s);
int gemv_wq_check(int kind, int64_t N, int64_t K, int nb, int dtype, int epi, bool norm);

}  // namespace ss
