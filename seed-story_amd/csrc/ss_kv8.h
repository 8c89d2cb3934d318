// fp8 (OCP e4m3fn) shadow of the KV cache for the q_len = 1 decode token (ss_attn_kv8.hip; the opt-in kv_cache="fp8" of the
// LLaMA engine).  The definition of the quantisation is in include/seedstory_hip.h (ss_kv_quantize_fp8).
#pragma once
#include "ss_common.h"

namespace ss {

// Rows [lo[b], hi[b]) of slot b's 16-bit planes [n_layers][heads][cap][hd] -> code planes (same shape, bytes) and scale planes
// [n_layers][heads][cap], K and V, every layer and slot in ONE launch.  slot_stride: elements (= code bytes) between two slots.
struct Kv8QuantArgs {
    const void *k, *v;
    uint8_t *kq, *vq;
    float *ks, *vs;
    int heads, cap, hd, n_layers, nb;
    int64_t slot_stride;
    int lo[8], hi[8];
};

// bf16 / fp16, hd % 16 == 0, hd <= 256, hd / 16 lanes per row a power of two; sets the error text
int kv8_check(int64_t hd, int dtype, const char* who);
int kv8_quantize_dev(const Kv8QuantArgs& a, int dtype, hipStream_t s);
// plain: rotated q given, the shadow holds *kv_len_dev rows
int attn_decode_kv8_dev(const void* q, const void* kq, const void* vq, const float* ks, const float* vs, void* out, void* ws,
                        const int32_t* kv_len_dev, const int32_t* done_flag, int64_t n_heads, int64_t hd, int64_t cache_cap,
                        int dtype, hipStream_t s);
// fused: attn_decode_fused_dev over the shadow; appends the new row to the 16-bit planes AND to the shadow
int attn_decode_kv8_fused_dev(const void* qkv_raw, void* kc, void* vc, void* kq, void* vq, float* ks, float* vs, const void* cos_t,
                              const void* sin_t, void* out, void* ws, const int32_t* kv_len_dev, const int32_t* pos_dev,
                              const int32_t* done_flag, int64_t n_heads, int64_t hd, int64_t cache_cap, int nb, int state_stride,
                              int64_t cache_stride, int dtype, hipStream_t s);

}  // namespace ss
