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

// The same projection over fp8 (OCP e4m3fn) weights Wq [N, K] bytes with one fp32 scale per row (w_scale [N], [2N] for the SiLU
// pair); x / y / bias / residual / norm_w in the 16-bit model dtype.  gemv_w8_check: the shape rules alone (no launch).
int gemv_w8_batched_dev(const void* Wq, const float* w_scale, const void* x, void* y, int64_t N, int64_t K, const void* norm_w,
                        float eps, const void* bias, const void* residual, int epi, const int32_t* done_flag, int done_stride,
                        int nb, int64_t x_ld, int64_t y_ld, int64_t res_ld, int dtype, hipStream_t s);
int gemv_w8_check(int64_t N, int64_t K, int nb, int dtype, int epi, bool norm);

// The same projection over MXFP4 weights: codes [N, K / 2] bytes (two e2m1 codes per byte, even k in the low nibble) and scales
// [N, K / 32] e8m0 bytes, one per 32 consecutive k ([2N, ...] for the SiLU pair).  gemv_mx4_check: the shape rules alone (no launch).
int gemv_mx4_batched_dev(const void* codes, const void* scales, const void* x, void* y, int64_t N, int64_t K, const void* norm_w,
                         float eps, const void* bias, const void* residual, int epi, const int32_t* done_flag, int done_stride,
                         int nb, int64_t x_ld, int64_t y_ld, int64_t res_ld, int dtype, hipStream_t s);
int gemv_mx4_check(int64_t N, int64_t K, int nb, int dtype, int epi, bool norm);

}  // namespace ss
