// HBM-bound kernels of the SDXL de-tokenizer half (UNet ResBlocks / Transformer2D, VAE decoder,
// Euler + classifier-free guidance) — the reference reaches these through diffusers
// (src/models_ipa/adapter_modules.py:455-466).
// Activations are NHWC ([B, H*W, C] row-major) so every convolution is an implicit GEMM over
// channels (ss_gemm.hip) and the transformer blocks need no permutes.
#include "ss_common.h"
#include "ss_sample.h"      // Philox4x32-10

#include <cmath>

namespace ss {

__device__ __forceinline__ float silu_d(float g) { return g / (1.0f + expf(-g)); }
__device__ __forceinline__ float gelu_d(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f)); }

// =====================================================================================
// GroupNorm over NHWC: statistics per (batch, group) of H*W x (C/G) elements, DETERMINISTIC (round 4: no atomics).
//   pass 1: every block reduces its rows to per-channel (sum, sum of squares) in a fixed order (thread-sequential over its
//           rows, then a fixed-order fold over the row lanes through LDS), folds the channels of a group in channel order
//           in fp64 and writes its partial to part[b][block][g][2]
//   pass 1b: one block per image sums the block partials in block order (fixed-size slices, slices folded in order)
//           -> stats[b][g][2] (fp64: E[x^2] - mean^2 without cancellation)
//   pass 2: y = (x - mean) * rstd * gamma[c] + beta[c]  (+ SiLU), rounded once to T
// Two runs on the same input give the same bits whatever the dispatch order (rounds 2-3 used fp64 atomics: order-dependent in
// the last bit, which a 70-block UNet amplified to a 2e-2 difference between two runs when the sums were fp32).
// (torch GroupNorm computes in fp32 and rounds the result; SiLU then rounds again.)
// =====================================================================================
// fast sigmoid-linear unit on the hardware transcendentals: x * rcp(1 + exp2(-x * log2 e))
__device__ __forceinline__ float silu_fast(float g) {
    return g * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * g));
}

// Both passes give every thread ONE fixed 16-byte channel pack and a strided set of pixel rows of one image,
// so everything that depends on the channel (group index, gamma/beta, mean/rstd) is hoisted out of the row loop
// and the loop body is a 16-byte load + 2 (stats) or ~4 (apply) VALU ops per element: both passes run at the
// HBM rate instead of being bound by per-element integer divisions and LDS atomics.
//   thread t of a block: pack p = pc + t % cw, first row r0 + t / cw, row stride 256 / cw   (cw = packs per chunk)
template <typename T>
__global__ __launch_bounds__(256) void groupnorm_stats_kernel(const T* __restrict__ x, double* __restrict__ part,
                                                              int HW, int C, int G, int rows_per_block) {
    constexpr int V = Tr<T>::kVec;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* red = reinterpret_cast<float*>(smem_raw);   // [256][2 V]: per-thread channel sums of the current pack chunk
    float* chs = red + 256 * 2 * V;                     // [C][2]: this block's per-channel (sum, sum of squares)
    const int b = blockIdx.y;
    const int cg = C / G, ppr = C / V;
    const int r0 = blockIdx.x * rows_per_block;
    const int r1 = min(HW, r0 + rows_per_block);
    const T* xb = x + ((int64_t)b * HW) * C;
    for (int pc = 0; pc < ppr; pc += 256) {
        const int cw = min(256, ppr - pc);
        const int rip = 256 / cw;                      // rows in flight per block pass
        const int ry = threadIdx.x / cw, p = pc + threadIdx.x % cw;
        const bool active = ry < rip;
        float s1[V], s2[V];                            // per-channel partial sums of this thread's pack
#pragma unroll
        for (int j = 0; j < V; ++j) { s1[j] = 0.f; s2[j] = 0.f; }
        if (active) {
            const T* xp = xb + (int64_t)p * V;
            int r = r0 + ry;
            for (; r + 3 * rip < r1; r += 4 * rip) {       // four independent loads in flight (round 5: 2.0 -> HBM rate; same add order)
                uint4 u[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) u[q] = ld16(xp + (int64_t)(r + q * rip) * C);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    float f[V];
                    unpack<T>(u[q], f);
#pragma unroll
                    for (int j = 0; j < V; ++j) { s1[j] += f[j]; s2[j] = fmaf(f[j], f[j], s2[j]); }
                }
            }
            for (; r + rip < r1; r += 2 * rip) {           // two independent loads in flight
                float f[V], h[V];
                const uint4 u0 = ld16(xp + (int64_t)r * C), u1 = ld16(xp + (int64_t)(r + rip) * C);
                unpack<T>(u0, f);
                unpack<T>(u1, h);
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    s1[j] += f[j]; s2[j] = fmaf(f[j], f[j], s2[j]);
                    s1[j] += h[j]; s2[j] = fmaf(h[j], h[j], s2[j]);
                }
            }
            if (r < r1) {
                float f[V];
                unpack<T>(ld16(xp + (int64_t)r * C), f);
#pragma unroll
                for (int j = 0; j < V; ++j) { s1[j] += f[j]; s2[j] = fmaf(f[j], f[j], s2[j]); }
            }
#pragma unroll
            for (int j = 0; j < V; ++j) { red[threadIdx.x * 2 * V + 2 * j] = s1[j]; red[threadIdx.x * 2 * V + 2 * j + 1] = s2[j]; }
        }
        __syncthreads();
        if (active && ry == 0) {       // fold the row lanes of this pack in lane order
            for (int k = 1; k < rip; ++k) {
                const float* o = red + (k * cw + (int)threadIdx.x) * 2 * V;
#pragma unroll
                for (int j = 0; j < V; ++j) { s1[j] += o[2 * j]; s2[j] += o[2 * j + 1]; }
            }
#pragma unroll
            for (int j = 0; j < V; ++j) { chs[(p * V + j) * 2] = s1[j]; chs[(p * V + j) * 2 + 1] = s2[j]; }
        }
        __syncthreads();
    }
    double* out = part + (((int64_t)b * gridDim.x + blockIdx.x) * G) * 2;
    for (int g = threadIdx.x; g < G; g += 256) {       // channels of a group in channel order, fp64
        double a1 = 0.0, a2 = 0.0;
        for (int c = g * cg; c < (g + 1) * cg; ++c) { a1 += (double)chs[2 * c]; a2 += (double)chs[2 * c + 1]; }
        out[2 * g] = a1;
        out[2 * g + 1] = a2;
    }
}

// stats[b][g] = sum over the blocks of image b, in block order: thread (slice, g) sums a contiguous slice of blocks, the slices
// are folded in slice order
__global__ __launch_bounds__(256) void groupnorm_finalize_kernel(const double* __restrict__ part, double* __restrict__ stats,
                                                                 int nblk, int G) {
    __shared__ double sl[256 * 2];
    const int b = blockIdx.x;
    const int gw = G < 256 ? G : 256;                   // groups handled per sweep
    const int ns = 256 / gw;                            // slices
    for (int g0 = 0; g0 < G; g0 += gw) {
        const int g = g0 + (int)threadIdx.x % gw, sidx = (int)threadIdx.x / gw;
        double a1 = 0.0, a2 = 0.0;
        if (sidx < ns && g < G) {
            const int per = (nblk + ns - 1) / ns;
            const int k0 = sidx * per, k1 = min(nblk, k0 + per);
            const double2* pp = reinterpret_cast<const double2*>(part) + (int64_t)b * nblk * G + g;
            for (int kb = k0; kb < k1; kb += 8) {       // 8 independent loads in flight, then the adds in block order
                double2 t[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) t[k] = (kb + k < k1) ? pp[(int64_t)(kb + k) * G] : make_double2(0.0, 0.0);
#pragma unroll
                for (int k = 0; k < 8; ++k) { a1 += t[k].x; a2 += t[k].y; }
            }
        }
        sl[threadIdx.x * 2] = a1;
        sl[threadIdx.x * 2 + 1] = a2;
        __syncthreads();
        if (sidx == 0 && g < G) {
            for (int k = 1; k < ns; ++k) { a1 += sl[(k * gw + (int)threadIdx.x) * 2]; a2 += sl[(k * gw + (int)threadIdx.x) * 2 + 1]; }
            stats[((int64_t)b * G + g) * 2] = a1;
            stats[((int64_t)b * G + g) * 2 + 1] = a2;
        }
        __syncthreads();
    }
}

template <typename T>
__global__ __launch_bounds__(256) void groupnorm_apply_kernel(const T* __restrict__ x, const double* __restrict__ stats,
                                                              const T* __restrict__ gamma, const T* __restrict__ beta,
                                                              T* __restrict__ y, int HW, int C, int G, float eps,
                                                              int silu, int rows_per_block) {
    constexpr int V = Tr<T>::kVec;
    const int b = blockIdx.y;
    const int cg = C / G, ppr = C / V;
    const int r0 = blockIdx.x * rows_per_block;
    const int r1 = min(HW, r0 + rows_per_block);
    const float inv_n = 1.0f / ((float)HW * (float)cg);
    const T* xb = x + ((int64_t)b * HW) * C;
    T* yb = y + ((int64_t)b * HW) * C;
    for (int pc = 0; pc < ppr; pc += 256) {
        const int cw = min(256, ppr - pc);
        const int rip = 256 / cw;
        const int ry = threadIdx.x / cw, p = pc + threadIdx.x % cw;
        if (ry >= rip) continue;
        // y = (x - mean) * rstd * gamma + beta  ==  x * sc + sh  with per-channel constants hoisted out of the loop
        float sc[V], sh[V], ga[V], be[V];
        unpack<T>(ld16(gamma + p * V), ga);
        unpack<T>(ld16(beta + p * V), be);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const int g = (p * V + j) / cg;
            const double md = stats[((int64_t)b * G + g) * 2] * (double)inv_n;      // E[x^2] - mean^2 in fp64: no cancellation
            const float mean = (float)md;
            const float var = (float)fmax(stats[((int64_t)b * G + g) * 2 + 1] * (double)inv_n - md * md, 0.0);
            const float rstd = 1.0f / sqrtf(var + eps);
            sc[j] = rstd * ga[j];
            sh[j] = be[j] - mean * sc[j];
        }
        const T* xp = xb + (int64_t)p * V;
        T* yp = yb + (int64_t)p * V;
        auto one = [&](const uint4& u, int r) {
            float f[V];
            unpack<T>(u, f);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                float v = fmaf(f[j], sc[j], sh[j]);
                if (silu) v = silu_fast(Tr<T>::rnd(v));
                f[j] = v;
            }
            st16(yp + (int64_t)r * C, pack<T>(f));
        };
        int r = r0 + ry;
        for (; r + 3 * rip < r1; r += 4 * rip) {           // four rows in flight per thread
            uint4 u[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) u[q] = ld16(xp + (int64_t)(r + q * rip) * C);
#pragma unroll
            for (int q = 0; q < 4; ++q) one(u[q], r + q * rip);
        }
        for (; r + rip < r1; r += 2 * rip) {
            const uint4 u0 = ld16(xp + (int64_t)r * C), u1 = ld16(xp + (int64_t)(r + rip) * C);
            one(u0, r);
            one(u1, r + rip);
        }
        if (r < r1) one(ld16(xp + (int64_t)r * C), r);
    }
}

static int groupnorm_rows_per_block(int64_t B, int64_t HW, int64_t C, size_t elem) {
    // ~128 KiB of activations per block, at least enough blocks to fill the chip several times
    // (tests/kernel_check.py GN_ROWS_MAX_BYTES / groupnorm_rows_per_block is a hand copy of this rule: its GroupNorm bound takes
    // the longest fp32 chain from it.  Change both together.)
    int rows_per_block = (int)((128 * 1024) / (C * elem));
    if (rows_per_block < 16) rows_per_block = 16;
    while (rows_per_block > 16 && B * cdiv(HW, rows_per_block) < 2048) rows_per_block /= 2;
    if (rows_per_block > HW) rows_per_block = (int)HW;
    return rows_per_block;
}

// workspace = [B][G][2] final sums + [B][blocks][G][2] block partials, doubles
size_t groupnorm_workspace_bytes(int64_t B, int64_t HW, int64_t C, int64_t G, int dtype) {
    if (B * HW == 0) return 0;
    const int rpb = groupnorm_rows_per_block(B, HW, C, dtype_size(dtype));
    return (size_t)B * G * 2 * sizeof(double) * (1 + (size_t)cdiv(HW, rpb));
}

template <typename T>
int groupnorm_launch(const void* x, const void* gamma, const void* beta, void* y, double* ws, int64_t B, int64_t HW,
                     int64_t C, int64_t G, float eps, int silu, hipStream_t s) {
    constexpr int V = Tr<T>::kVec;
    SS_REQUIRE(C % G == 0 && C % V == 0, "groupnorm: C=%lld G=%lld unsupported", (long long)C, (long long)G);
    if (B * HW == 0) return SS_OK;
    const int rows_per_block = groupnorm_rows_per_block(B, HW, C, sizeof(T));
    dim3 grid((unsigned)cdiv(HW, rows_per_block), (unsigned)B);
    double* stats = ws;
    double* part = ws + (size_t)B * G * 2;
    const size_t lds = (size_t)256 * 2 * V * sizeof(float) + (size_t)C * 2 * sizeof(float);
    SS_REQUIRE(lds <= 64 * 1024, "groupnorm: C=%lld too wide", (long long)C);
    hipLaunchKernelGGL(groupnorm_stats_kernel<T>, grid, dim3(256), lds, s, (const T*)x, part, (int)HW, (int)C, (int)G,
                       rows_per_block);
    SS_LAUNCH_CHECK("groupnorm_stats");
    hipLaunchKernelGGL(groupnorm_finalize_kernel, dim3((unsigned)B), dim3(256), 0, s, (const double*)part, stats, (int)grid.x, (int)G);
    SS_LAUNCH_CHECK("groupnorm_finalize");
    hipLaunchKernelGGL(groupnorm_apply_kernel<T>, grid, dim3(256), 0, s, (const T*)x, stats, (const T*)gamma,
                       (const T*)beta, (T*)y, (int)HW, (int)C, (int)G, eps, silu, rows_per_block);
    SS_LAUNCH_CHECK("groupnorm_apply");
    return SS_OK;
}

// =====================================================================================
// small element-wise / layout kernels
// =====================================================================================
// GEGLU: out[r, i] = val[r, i] * gelu(gate[r, i]); in [rows, 2D] = [val | gate]  (diffusers GEGLU)
template <typename T>
__global__ __launch_bounds__(256) void geglu_kernel(const T* __restrict__ in, T* __restrict__ out, int64_t rows, int D) {
    constexpr int V = Tr<T>::kVec;
    const int ppr = D / V;
    const int64_t total = rows * ppr;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / ppr;
        const int p = (int)(i % ppr);
        float a[V], g[V];
        unpack<T>(ld16(in + r * 2 * D + (int64_t)p * V), a);
        unpack<T>(ld16(in + r * 2 * D + D + (int64_t)p * V), g);
#pragma unroll
        for (int j = 0; j < V; ++j) a[j] = a[j] * Tr<T>::rnd(gelu_d(g[j]));
        st16(out + r * D + (int64_t)p * V, pack<T>(a));
    }
}

// in-place row softmax of s[rows, cols] * scale (fp32 math, rounded to T)
template <typename T>
__global__ __launch_bounds__(256) void softmax_rows_kernel(T* __restrict__ s, int cols, float scale) {
    constexpr int V = Tr<T>::kVec;
    __shared__ float red[16];
    T* row = s + (int64_t)blockIdx.x * cols;
    const int npack = cols / V;
    float mx = -1e30f;
    for (int p = threadIdx.x; p < npack; p += 256) {
        float f[V];
        unpack<T>(ld16(row + (int64_t)p * V), f);
#pragma unroll
        for (int j = 0; j < V; ++j) mx = fmaxf(mx, f[j] * scale);
    }
    mx = block_max(mx, red);
    float sum = 0.f;
    for (int p = threadIdx.x; p < npack; p += 256) {
        float f[V];
        unpack<T>(ld16(row + (int64_t)p * V), f);
#pragma unroll
        for (int j = 0; j < V; ++j) sum += expf(f[j] * scale - mx);
    }
    sum = block_sum(sum, red);
    const float inv = 1.0f / sum;
    for (int p = threadIdx.x; p < npack; p += 256) {
        float f[V];
        unpack<T>(ld16(row + (int64_t)p * V), f);
#pragma unroll
        for (int j = 0; j < V; ++j) f[j] = expf(f[j] * scale - mx) * inv;
        st16(row + (int64_t)p * V, pack<T>(f));
    }
}

// out[c, r] = in[r, c]  (32x32 LDS tile transpose)
template <typename T>
__global__ __launch_bounds__(256) void transpose_kernel(const T* __restrict__ in, T* __restrict__ out, int R, int Cc) {
    __shared__ T tile[32][33];
    const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
    for (int j = ty; j < 32; j += 8)
        if (r0 + j < R && c0 + tx < Cc) tile[j][tx] = in[(int64_t)(r0 + j) * Cc + c0 + tx];
    __syncthreads();
    for (int j = ty; j < 32; j += 8)
        if (c0 + j < Cc && r0 + tx < R) out[(int64_t)(c0 + j) * R + r0 + tx] = tile[tx][j];
}

// out[r, :C1] = a[r, :], out[r, C1:] = b[r, :]   (channel concat of two NHWC tensors: torch.cat(dim=1) in NCHW)
template <typename T>
__global__ __launch_bounds__(256) void concat_channels_kernel(const T* __restrict__ a, const T* __restrict__ b,
                                                              T* __restrict__ out, int64_t rows, int C1, int C2) {
    constexpr int V = Tr<T>::kVec;
    const int ppr = (C1 + C2) / V, p1 = C1 / V;
    const int64_t total = rows * ppr;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / ppr;
        const int p = (int)(i % ppr);
        const uint4 v = p < p1 ? ld16(a + r * C1 + (int64_t)p * V) : ld16(b + r * C2 + (int64_t)(p - p1) * V);
        st16(out + r * (C1 + C2) + (int64_t)p * V, v);
    }
}

// NCHW [B, C, HW] <-> NHWC [B, HW, Cpad] for the tiny latent tensors (C = 4 -> Cpad = 8, zero padded)
template <typename T>
__global__ void nchw_to_nhwc_kernel(const T* __restrict__ in, T* __restrict__ out, int64_t B, int C, int HW, int Cpad) {
    const int64_t total = B * HW * Cpad;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % Cpad);
        const int64_t r = i / Cpad;
        const int64_t b = r / HW, px = r % HW;
        T v;
        if (c < C) v = in[(b * C + c) * HW + px]; else Tr<T>::st(&v, 0.f);
        out[i] = v;
    }
}
template <typename T>
__global__ void nhwc_to_nchw_kernel(const T* __restrict__ in, T* __restrict__ out, int64_t B, int C, int HW, int Cpad) {
    const int64_t total = B * C * HW;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t px = i % HW;
        const int64_t bc = i / HW;
        const int c = (int)(bc % C);
        const int64_t b = bc / C;
        out[i] = in[(b * HW + px) * Cpad + c];
    }
}

// EulerDiscreteScheduler.scale_model_input + CFG duplication: xin[0] = xin[1] = x / sqrt(sigma^2 + 1)
// classifier-free guidance + Euler step:  e = eu + g (ec - eu);  x += e * (sigma_next - sigma)
// (fp32 latents like diffusers keeps them when the pipeline dtype is fp32; T otherwise)
template <typename T>
__global__ void euler_scale_dup_kernel(const T* __restrict__ x, T* __restrict__ xin, int64_t n, float inv) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float v = Tr<T>::ld(x + i) * inv;
        Tr<T>::st(xin + i, v);
        Tr<T>::st(xin + n + i, v);
    }
}
template <typename T>
__global__ void euler_cfg_step_kernel(T* __restrict__ x, const T* __restrict__ eps, int64_t n, float guidance, float dsigma) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float eu = Tr<T>::ld(eps + i), ec = Tr<T>::ld(eps + n + i);
        const float e = Tr<T>::rnd(eu + Tr<T>::rnd(guidance * Tr<T>::rnd(ec - eu)));
        Tr<T>::st(x + i, Tr<T>::ld(x + i) + Tr<T>::rnd(e * dsigma));
    }
}

// Linear multistep sampler step + CFG, fused with the NEXT step's scale_model_input + CFG duplication (DPM-Solver++ 2M; Euler
// fits the same form).  fp32 end to end, in this operation order (tests/test_dpmpp_gpu.py derives its bound from it):
//   e = eu + g (ec - eu);  d = x - sigma e;  x' = (a x + b d) [+ c d_prev];  state <- (x', d);  x_out = rnd_T(x');
//   xin_next[0] = xin_next[1] = rnd_T(x' inv_next)
// The solver state is fp32 and is never rounded to T between steps (a second-order difference of rounded states is where bf16
// would hurt).  c == 0: d_prev is not read (first step: uninitialised).
// the solver update for a given e (the guided combination, or the conditional prediction alone)
__device__ __forceinline__ void multistep_apply(float& x, float& dprev, float e, bool prev, float sigma, float a, float b,
                                                float c) {
    const float d = x - sigma * e;
    float xn = a * x + b * d;
    if (prev) xn += c * dprev;
    x = xn;
    dprev = d;
}
__device__ __forceinline__ void multistep_one(float& x, float& dprev, float eu, float ec, bool prev, float g, float sigma,
                                              float a, float b, float c) {
    multistep_apply(x, dprev, eu + g * (ec - eu), prev, sigma, a, b, c);
}
// V fp32 values at p: 16-byte accesses when `vec`, single elements otherwise (second rows of an n that is no multiple of V)
template <int V>
__device__ __forceinline__ void ld_f32(const float* p, bool vec, float* f) {
    if (vec) {
#pragma unroll
        for (int k = 0; k < V; k += 4) unpack<float>(ld16(p + k), f + k);
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j) f[j] = p[j];
    }
}
template <int V>
__device__ __forceinline__ void st_f32(float* p, bool vec, const float* f) {
    if (vec) {
#pragma unroll
        for (int k = 0; k < V; k += 4) st16(p + k, pack<float>(f + k));
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j) p[j] = f[j];
    }
}
// npack packets of V elements (row 0 of every buffer is 16-byte aligned; row 1 only when row1_vec), then n - npack V single elements
template <typename T>
__global__ __launch_bounds__(256) void multistep_cfg_step_kernel(float* __restrict__ state, const T* __restrict__ eps,
                                                                 T* __restrict__ x_out, T* __restrict__ xin_next, int64_t n,
                                                                 int64_t npack, int row1_vec, float g, float sigma, float a,
                                                                 float b, float c, float inv_next) {
    constexpr int V = Tr<T>::kVec;
    const bool prev = c != 0.0f;
    const bool v1 = row1_vec != 0;
    const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t p = tid; p < npack; p += stride) {
        const int64_t i = p * V;
        float x[V], dp[V], eu[V], ec[V], xs[V];
        ld_f32<V>(state + i, true, x);
        unpack<T>(ld16(eps + i), eu);
        if (v1) {
            unpack<T>(ld16(eps + n + i), ec);
        } else {
#pragma unroll
            for (int j = 0; j < V; ++j) ec[j] = Tr<T>::ld(eps + n + i + j);
        }
        if (prev) ld_f32<V>(state + n + i, v1, dp);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            multistep_one(x[j], dp[j], eu[j], ec[j], prev, g, sigma, a, b, c);
            xs[j] = x[j] * inv_next;
        }
        st_f32<V>(state + i, true, x);
        st_f32<V>(state + n + i, v1, dp);
        if (x_out) st16(x_out + i, pack<T>(x));
        if (xin_next) {
            const uint4 u = pack<T>(xs);
            st16(xin_next + i, u);
            if (v1) {
                st16(xin_next + n + i, u);
            } else {
#pragma unroll
                for (int j = 0; j < V; ++j) Tr<T>::st(xin_next + n + i + j, xs[j]);
            }
        }
    }
    for (int64_t i = npack * V + tid; i < n; i += stride) {
        float x = state[i], dp = prev ? state[n + i] : 0.f;
        multistep_one(x, dp, Tr<T>::ld(eps + i), Tr<T>::ld(eps + n + i), prev, g, sigma, a, b, c);
        state[i] = x;
        state[n + i] = dp;
        if (x_out) Tr<T>::st(x_out + i, x);
        if (xin_next) {
            const float v = x * inv_next;
            Tr<T>::st(xin_next + i, v);
            Tr<T>::st(xin_next + n + i, v);
        }
    }
}

// The same step for limited-interval guidance (ss_multistep_step): ER rows of eps are read, XR rows of xin_next written.
// ER == 2: e = eu + g (ec - eu) as above.  ER == 1: eps holds the conditional prediction alone and e is that value as loaded
// (no arithmetic, g unused).  XR == 1: the next step is unguided and takes one copy of rnd_T(x' inv_next).  Rows that a form
// does not use are never addressed: eps and xin_next may be one row long.  Packets as above: second rows (state row 1 always,
// eps / xin_next row 1 when the form has one) are 16-byte accesses only when row1_vec.
//
// Gaussian noise of the stochastic samplers (Euler ancestral, DPM++ 2M SDE; definition: tests/sde_ref.py).  The
// four normals of quad q = j >> 2 of an image's latent (flat element j) at step `step` for the image's 64-bit seed:
//   (w0, w1, w2, w3) = Philox4x32-10(counter (q, step, 1, 0), key (seed lo, seed hi))     word 2 = 1: apart from the token sampler
//   u(w) = (w >> 8) 2^-24;  r(w) = sqrt(-2 ln(u(w) + 2^-24))      the log's argument is exact in fp32 and lies in (0, 1]
//   z = [r(w0) cos(2 pi u(w1)), r(w0) sin(2 pi u(w1)), r(w2) cos(2 pi u(w3)), r(w2) sin(2 pi u(w3))]
// cos / sin of 2 pi u are taken as cospi / sinpi of 2 u (exact argument: no rounded 2 pi).  fp32, one rounding per operation
// (tests/test_sde_gpu.py derives its bound from this list): log, * -2 (exact), sqrt, sincospi, product.
// ss_randn_philox and the NOISE step below both call this function, so their values agree bit for bit.
__device__ __forceinline__ void philox_normal4(uint32_t seed_lo, uint32_t seed_hi, uint32_t step, uint32_t q, float* z) {
    constexpr float k2m24 = 5.9604644775390625e-8f;
    uint32_t w[4];
    philox4x32_10(q, step, 1u, 0u, seed_lo, seed_hi, w);
#pragma unroll
    for (int k = 0; k < 4; k += 2) {
        const float u0 = (float)(w[k] >> 8) * k2m24, u1 = (float)(w[k + 1] >> 8) * k2m24;
        const float r = sqrtf(-2.0f * logf(u0 + k2m24));
        float sn, cs;
        sincospif(2.0f * u1, &sn, &cs);
        z[k] = r * cs;
        z[k + 1] = r * sn;
    }
}
// NOISE (one trailing StepNoise argument; the plain step's instantiations have none and keep the code they always had):
// x' = ((a x + b d) [+ c d_prev]) + s z, z that of element i % n_img of image i / n_img (seeds[i / n_img]): one fp32 product
// and one fp32 sum after the chain above.  The launcher takes packets only when n_img % V == 0 (a packet then lies in one
// image and covers whole quads) and single elements for everything otherwise; n % n_img == 0, so packets leave no tail.
struct StepNoise {
    float s;
    const uint64_t* seeds;      // [n / n_img] in device memory
    int64_t n_img;
    uint32_t step;
};
template <typename T, int ER, int XR, typename... NZ>
__global__ __launch_bounds__(256) void multistep_step_kernel(float* __restrict__ state, const T* __restrict__ eps,
                                                             T* __restrict__ x_out, T* __restrict__ xin_next, int64_t n,
                                                             int64_t npack, int row1_vec, float g, float sigma, float a, float b,
                                                             float c, float inv_next, NZ... nz) {
    constexpr bool NOISE = sizeof...(NZ) == 1;
    static_assert(sizeof...(NZ) <= 1, "at most one StepNoise");
    constexpr int V = Tr<T>::kVec;
    const bool prev = c != 0.0f;
    const bool v1 = row1_vec != 0;
    const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    float s = 0.f;
    const uint64_t* seeds = nullptr;
    int64_t n_img = 1;
    uint32_t step = 0;
    if constexpr (NOISE) {
        const StepNoise& nza = (nz, ...);
        s = nza.s; seeds = nza.seeds; n_img = nza.n_img; step = nza.step;
    }
    for (int64_t p = tid; p < npack; p += stride) {
        const int64_t i = p * V;
        float x[V], dp[V], e0[V], ec[V], xs[V];      // e0: row 0 of eps (uncond when ER == 2, cond when ER == 1)
        float z[V];
        if constexpr (NOISE) {
            const int64_t img = i / n_img, j = i - img * n_img;
            const uint64_t sd = seeds[img];
#pragma unroll
            for (int k = 0; k < V; k += 4)
                philox_normal4((uint32_t)sd, (uint32_t)(sd >> 32), step, (uint32_t)(j >> 2) + k / 4, z + k);
        }
        ld_f32<V>(state + i, true, x);
        unpack<T>(ld16(eps + i), e0);
        if (ER == 2) {
            if (v1) {
                unpack<T>(ld16(eps + n + i), ec);
            } else {
#pragma unroll
                for (int j = 0; j < V; ++j) ec[j] = Tr<T>::ld(eps + n + i + j);
            }
        }
        if (prev) ld_f32<V>(state + n + i, v1, dp);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            if (ER == 2) multistep_one(x[j], dp[j], e0[j], ec[j], prev, g, sigma, a, b, c);
            else multistep_apply(x[j], dp[j], e0[j], prev, sigma, a, b, c);
            if constexpr (NOISE) x[j] += s * z[j];
            xs[j] = x[j] * inv_next;
        }
        st_f32<V>(state + i, true, x);
        st_f32<V>(state + n + i, v1, dp);
        if (x_out) st16(x_out + i, pack<T>(x));
        if (xin_next) {
            const uint4 u = pack<T>(xs);
            st16(xin_next + i, u);
            if (XR == 2) {
                if (v1) {
                    st16(xin_next + n + i, u);
                } else {
#pragma unroll
                    for (int j = 0; j < V; ++j) Tr<T>::st(xin_next + n + i + j, xs[j]);
                }
            }
        }
    }
    for (int64_t i = npack * V + tid; i < n; i += stride) {
        float x = state[i], dp = prev ? state[n + i] : 0.f;
        if (ER == 2) multistep_one(x, dp, Tr<T>::ld(eps + i), Tr<T>::ld(eps + n + i), prev, g, sigma, a, b, c);
        else multistep_apply(x, dp, Tr<T>::ld(eps + i), prev, sigma, a, b, c);
        if constexpr (NOISE) {
            const int64_t img = i / n_img, j = i - img * n_img;
            const uint64_t sd = seeds[img];
            float zq[4];
            philox_normal4((uint32_t)sd, (uint32_t)(sd >> 32), step, (uint32_t)(j >> 2), zq);
            const int l = (int)(j & 3);
            x += s * (l == 0 ? zq[0] : l == 1 ? zq[1] : l == 2 ? zq[2] : zq[3]);
        }
        state[i] = x;
        state[n + i] = dp;
        if (x_out) Tr<T>::st(x_out + i, x);
        if (xin_next) {
            const float v = x * inv_next;
            Tr<T>::st(xin_next + i, v);
            if (XR == 2) Tr<T>::st(xin_next + n + i, v);
        }
    }
}
// out[b, j] = rnd_T(z(seeds[b], step, j)): one thread per quad; `vec`: a quad is one store (n_img % 4 == 0, aligned base)
template <typename T>
__global__ __launch_bounds__(256) void randn_philox_kernel(T* __restrict__ out, const uint64_t* __restrict__ seeds,
                                                           int64_t batch, int64_t n_img, int64_t nq, uint32_t step, int vec) {
    const int64_t total = batch * nq;
    for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < total; p += (int64_t)gridDim.x * blockDim.x) {
        const int64_t img = p / nq, q = p - img * nq;
        const uint64_t sd = seeds[img];
        float z[4];
        philox_normal4((uint32_t)sd, (uint32_t)(sd >> 32), step, (uint32_t)q, z);
        T* o = out + img * n_img + q * 4;
        if (vec) {
            if constexpr (sizeof(T) == 4) {
                st16(o, pack<float>(z));
            } else {
                float f[8] = {z[0], z[1], z[2], z[3], 0.f, 0.f, 0.f, 0.f};
                const uint4 u = pack<T>(f);
                *reinterpret_cast<uint2*>(o) = make_uint2(u.x, u.y);
            }
        } else {
#pragma unroll
            for (int l = 0; l < 4; ++l)
                if (q * 4 + l < n_img) Tr<T>::st(o + l, z[l]);
        }
    }
}
// Unguided Euler step: x += rnd_T(ec dsigma) (euler_cfg_step_kernel without its CFG lines); scale_model_input into `rows`
// copies (rows == 2 is euler_scale_dup_kernel)
template <typename T>
__global__ void euler_step_kernel(T* __restrict__ x, const T* __restrict__ eps, int64_t n, float dsigma) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        Tr<T>::st(x + i, Tr<T>::ld(x + i) + Tr<T>::rnd(Tr<T>::ld(eps + i) * dsigma));
}
template <typename T>
__global__ void euler_scale_kernel(const T* __restrict__ x, T* __restrict__ xin, int64_t n, int rows, float inv) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float v = Tr<T>::ld(x + i) * inv;
        Tr<T>::st(xin + i, v);
        if (rows == 2) Tr<T>::st(xin + n + i, v);
    }
}

// VAE output NHWC [B, HW, Cpad] (first 3 channels) -> uint8 HWC: round(clamp(x/2 + 0.5, 0, 1) * 255)
template <typename T>
__global__ void image_to_u8_kernel(const T* __restrict__ in, uint8_t* __restrict__ out, int64_t pixels, int Cpad) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < pixels * 3; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % 3);
        const int64_t px = i / 3;
        float v = Tr<T>::rnd(Tr<T>::ld(in + px * Cpad + c) * 0.5f + 0.5f);
        v = fminf(fmaxf(v, 0.f), 1.f);
        out[i] = (uint8_t)rintf(v * 255.0f);
    }
}

// y = silu(x) | gelu(x), rounded to T  (time-embedding activations: F.silu(emb))
template <typename T>
__global__ void unary_kernel(const T* __restrict__ x, T* __restrict__ y, int64_t n, int op) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float v = Tr<T>::ld(x + i);
        Tr<T>::st(y + i, op == 0 ? silu_d(v) : gelu_d(v));
    }
}

static inline unsigned egrid(int64_t total) {
    int64_t g = (total + 255) / 256;
    if (g > 256 * 16) g = 256 * 16;
    if (g < 1) g = 1;
    return (unsigned)g;
}

template <typename T>
int geglu_launch(const void* in, void* out, int64_t rows, int64_t D, hipStream_t s) {
    SS_REQUIRE(D % Tr<T>::kVec == 0, "geglu: D %% %d != 0", Tr<T>::kVec);
    if (rows == 0) return SS_OK;
    hipLaunchKernelGGL(geglu_kernel<T>, dim3(egrid(rows * D / Tr<T>::kVec)), dim3(256), 0, s, (const T*)in, (T*)out, rows, (int)D);
    SS_LAUNCH_CHECK("geglu");
    return SS_OK;
}
template <typename T>
int unary_launch(const void* x, void* y, int64_t n, int op, hipStream_t s) {
    if (n == 0) return SS_OK;
    hipLaunchKernelGGL(unary_kernel<T>, dim3(egrid(n)), dim3(256), 0, s, (const T*)x, (T*)y, n, op);
    SS_LAUNCH_CHECK("unary");
    return SS_OK;
}
template <typename T>
int softmax_rows_launch(void* sc, int64_t rows, int64_t cols, float scale, hipStream_t s) {
    SS_REQUIRE(cols % Tr<T>::kVec == 0, "softmax_rows: cols %% %d != 0", Tr<T>::kVec);
    if (rows == 0) return SS_OK;
    hipLaunchKernelGGL(softmax_rows_kernel<T>, dim3((unsigned)rows), dim3(256), 0, s, (T*)sc, (int)cols, scale);
    SS_LAUNCH_CHECK("softmax_rows");
    return SS_OK;
}
template <typename T>
int transpose_launch(const void* in, void* out, int64_t R, int64_t Cc, hipStream_t s) {
    if (R * Cc == 0) return SS_OK;
    hipLaunchKernelGGL(transpose_kernel<T>, dim3((unsigned)cdiv(Cc, 32), (unsigned)cdiv(R, 32)), dim3(256), 0, s,
                       (const T*)in, (T*)out, (int)R, (int)Cc);
    SS_LAUNCH_CHECK("transpose");
    return SS_OK;
}
template <typename T>
int concat_channels_launch(const void* a, const void* b, void* out, int64_t rows, int64_t C1, int64_t C2, hipStream_t s) {
    SS_REQUIRE(C1 % Tr<T>::kVec == 0 && C2 % Tr<T>::kVec == 0, "concat_channels: channels %% %d != 0", Tr<T>::kVec);
    if (rows == 0) return SS_OK;
    hipLaunchKernelGGL(concat_channels_kernel<T>, dim3(egrid(rows * (C1 + C2) / Tr<T>::kVec)), dim3(256), 0, s,
                       (const T*)a, (const T*)b, (T*)out, rows, (int)C1, (int)C2);
    SS_LAUNCH_CHECK("concat_channels");
    return SS_OK;
}
template <typename T>
int layout_launch(const void* in, void* out, int64_t B, int64_t C, int64_t HW, int64_t Cpad, int to_nhwc, hipStream_t s) {
    if (B * HW == 0) return SS_OK;
    if (to_nhwc)
        hipLaunchKernelGGL(nchw_to_nhwc_kernel<T>, dim3(egrid(B * HW * Cpad)), dim3(256), 0, s, (const T*)in, (T*)out, B,
                           (int)C, (int)HW, (int)Cpad);
    else
        hipLaunchKernelGGL(nhwc_to_nchw_kernel<T>, dim3(egrid(B * C * HW)), dim3(256), 0, s, (const T*)in, (T*)out, B,
                           (int)C, (int)HW, (int)Cpad);
    SS_LAUNCH_CHECK("layout");
    return SS_OK;
}
template <typename T>
int euler_scale_dup_launch(const void* x, void* xin, int64_t n, float sigma, hipStream_t s) {
    hipLaunchKernelGGL(euler_scale_dup_kernel<T>, dim3(egrid(n)), dim3(256), 0, s, (const T*)x, (T*)xin, n,
                       1.0f / sqrtf(sigma * sigma + 1.0f));
    SS_LAUNCH_CHECK("euler_scale_dup");
    return SS_OK;
}
template <typename T>
int euler_cfg_step_launch(void* x, const void* eps, int64_t n, float guidance, float sigma, float sigma_next, hipStream_t s) {
    hipLaunchKernelGGL(euler_cfg_step_kernel<T>, dim3(egrid(n)), dim3(256), 0, s, (T*)x, (const T*)eps, n, guidance,
                       sigma_next - sigma);
    SS_LAUNCH_CHECK("euler_cfg_step");
    return SS_OK;
}
template <typename T>
int multistep_cfg_step_launch(float* state, const void* eps, void* x_out, void* xin_next, int64_t n, float g, float sigma,
                              float a, float b, float c, float inv_next, hipStream_t s) {
    constexpr int V = Tr<T>::kVec;
    const uintptr_t bases = (uintptr_t)state | (uintptr_t)eps | (uintptr_t)x_out | (uintptr_t)xin_next;   // NULL: no bits
    const int64_t npack = (bases & 15) == 0 ? n / V : 0;
    const int row1_vec = npack > 0 && n % V == 0;
    hipLaunchKernelGGL(multistep_cfg_step_kernel<T>, dim3(egrid(npack + (n - npack * V))), dim3(256), 0, s, state,
                       (const T*)eps, (T*)x_out, (T*)xin_next, n, npack, row1_vec, g, sigma, a, b, c, inv_next);
    SS_LAUNCH_CHECK("multistep_cfg_step");
    return SS_OK;
}
template <typename T>
int multistep_step_launch(float* state, const void* eps, void* x_out, void* xin_next, int64_t n, int eps_rows, int xin_rows,
                          float g, float sigma, float a, float b, float c, float inv_next, hipStream_t s) {
    constexpr int V = Tr<T>::kVec;
    const uintptr_t bases = (uintptr_t)state | (uintptr_t)eps | (uintptr_t)x_out | (uintptr_t)xin_next;   // NULL: no bits
    const int64_t npack = (bases & 15) == 0 ? n / V : 0;
    const int row1_vec = npack > 0 && n % V == 0;
    const dim3 grid(egrid(npack + (n - npack * V)));
#define SS_MS_FORM(ER, XR)                                                                                              \
    hipLaunchKernelGGL((multistep_step_kernel<T, ER, XR>), grid, dim3(256), 0, s, state, (const T*)eps, (T*)x_out,        \
                       (T*)xin_next, n, npack, row1_vec, g, sigma, a, b, c, inv_next)
    if (eps_rows == 2 && xin_rows == 2) SS_MS_FORM(2, 2);
    else if (eps_rows == 2) SS_MS_FORM(2, 1);
    else if (xin_rows == 2) SS_MS_FORM(1, 2);
    else SS_MS_FORM(1, 1);
#undef SS_MS_FORM
    SS_LAUNCH_CHECK("multistep_step");
    return SS_OK;
}
template <typename T>
int multistep_noise_step_launch(float* state, const void* eps, void* x_out, void* xin_next, int64_t n, int eps_rows,
                                int xin_rows, float g, float sigma, float a, float b, float c, float s, float inv_next,
                                const uint64_t* seeds, int64_t n_img, int step, hipStream_t st) {
    if (s == 0.0f)      // no noise term: the plain step's own kernels, bit for bit (seeds is not read)
        return multistep_step_launch<T>(state, eps, x_out, xin_next, n, eps_rows, xin_rows, g, sigma, a, b, c, inv_next, st);
    constexpr int V = Tr<T>::kVec;
    const uintptr_t bases = (uintptr_t)state | (uintptr_t)eps | (uintptr_t)x_out | (uintptr_t)xin_next;   // NULL: no bits
    const int64_t npack = ((bases & 15) == 0 && n_img % V == 0) ? n / V : 0;      // n % n_img == 0: all packets or none
    const int row1_vec = npack > 0;
    const dim3 grid(egrid(npack > 0 ? npack : n));
    const StepNoise nz{s, seeds, n_img, (uint32_t)step};
#define SS_MS_FORM(ER, XR)                                                                                              \
    hipLaunchKernelGGL((multistep_step_kernel<T, ER, XR, StepNoise>), grid, dim3(256), 0, st, state, (const T*)eps, (T*)x_out, \
                       (T*)xin_next, n, npack, row1_vec, g, sigma, a, b, c, inv_next, nz)
    if (eps_rows == 2 && xin_rows == 2) SS_MS_FORM(2, 2);
    else if (eps_rows == 2) SS_MS_FORM(2, 1);
    else if (xin_rows == 2) SS_MS_FORM(1, 2);
    else SS_MS_FORM(1, 1);
#undef SS_MS_FORM
    SS_LAUNCH_CHECK("multistep_noise_step");
    return SS_OK;
}
template <typename T>
int randn_philox_launch(void* out, const uint64_t* seeds, int64_t batch, int64_t n_img, int step, hipStream_t st) {
    const int64_t nq = (n_img + 3) / 4;
    const int vec = n_img % 4 == 0 && ((uintptr_t)out & 15) == 0;
    hipLaunchKernelGGL(randn_philox_kernel<T>, dim3(egrid(batch * nq)), dim3(256), 0, st, (T*)out, seeds, batch, n_img, nq,
                       (uint32_t)step, vec);
    SS_LAUNCH_CHECK("randn_philox");
    return SS_OK;
}
template <typename T>
int euler_step_launch(void* x, const void* eps, int64_t n, float sigma, float sigma_next, hipStream_t s) {
    hipLaunchKernelGGL(euler_step_kernel<T>, dim3(egrid(n)), dim3(256), 0, s, (T*)x, (const T*)eps, n, sigma_next - sigma);
    SS_LAUNCH_CHECK("euler_step");
    return SS_OK;
}
template <typename T>
int euler_scale_launch(const void* x, void* xin, int64_t n, int rows, float sigma, hipStream_t s) {
    hipLaunchKernelGGL(euler_scale_kernel<T>, dim3(egrid(n)), dim3(256), 0, s, (const T*)x, (T*)xin, n, rows,
                       1.0f / sqrtf(sigma * sigma + 1.0f));
    SS_LAUNCH_CHECK("euler_scale");
    return SS_OK;
}
template <typename T>
int image_to_u8_launch(const void* in, void* out, int64_t pixels, int64_t Cpad, hipStream_t s) {
    hipLaunchKernelGGL(image_to_u8_kernel<T>, dim3(egrid(pixels * 3)), dim3(256), 0, s, (const T*)in, (uint8_t*)out, pixels,
                       (int)Cpad);
    SS_LAUNCH_CHECK("image_to_u8");
    return SS_OK;
}

}  // namespace ss

using namespace ss;

extern "C" {

size_t ss_groupnorm_workspace_bytes(int64_t batch, int64_t hw, int64_t channels, int64_t groups, int dtype) {
    return ss::groupnorm_workspace_bytes(batch, hw, channels, groups, dtype);
}

int ss_groupnorm(const void* x, const void* gamma, const void* beta, void* y, void* stats_ws, int64_t batch, int64_t hw,
                 int64_t channels, int64_t groups, float eps, int fuse_silu, int dtype, void* stream) {
    return SS_DISPATCH(dtype, groupnorm_launch, x, gamma, beta, y, (double*)stats_ws, batch, hw, channels, groups, eps,
                       fuse_silu, (hipStream_t)stream);
}
int ss_geglu(const void* in, void* out, int64_t rows, int64_t d, int dtype, void* stream) {
    return SS_DISPATCH(dtype, geglu_launch, in, out, rows, d, (hipStream_t)stream);
}
int ss_unary(const void* x, void* y, int64_t n, int op, int dtype, void* stream) {
    return SS_DISPATCH(dtype, unary_launch, x, y, n, op, (hipStream_t)stream);
}
int ss_softmax_rows(void* scores, int64_t rows, int64_t cols, float scale, int dtype, void* stream) {
    return SS_DISPATCH(dtype, softmax_rows_launch, scores, rows, cols, scale, (hipStream_t)stream);
}
int ss_transpose(const void* in, void* out, int64_t rows, int64_t cols, int dtype, void* stream) {
    return SS_DISPATCH(dtype, transpose_launch, in, out, rows, cols, (hipStream_t)stream);
}
int ss_concat_channels(const void* a, const void* b, void* out, int64_t rows, int64_t c1, int64_t c2, int dtype,
                       void* stream) {
    return SS_DISPATCH(dtype, concat_channels_launch, a, b, out, rows, c1, c2, (hipStream_t)stream);
}
int ss_layout_nchw_nhwc(const void* in, void* out, int64_t batch, int64_t channels, int64_t hw, int64_t cpad,
                        int to_nhwc, int dtype, void* stream) {
    return SS_DISPATCH(dtype, layout_launch, in, out, batch, channels, hw, cpad, to_nhwc, (hipStream_t)stream);
}
int ss_euler_scale_dup(const void* x, void* xin, int64_t n, float sigma, int dtype, void* stream) {
    return SS_DISPATCH(dtype, euler_scale_dup_launch, x, xin, n, sigma, (hipStream_t)stream);
}
int ss_euler_cfg_step(void* x, const void* eps, int64_t n, float guidance, float sigma, float sigma_next, int dtype,
                      void* stream) {
    return SS_DISPATCH(dtype, euler_cfg_step_launch, x, eps, n, guidance, sigma, sigma_next, (hipStream_t)stream);
}
int ss_multistep_cfg_step(float* state, const void* eps, void* x_out, void* xin_next, int64_t n, float guidance, float sigma,
                          float a, float b, float c, float inv_next, int dtype, void* stream) {
    SS_REQUIRE(n > 0, "multistep_cfg_step: n = %lld", (long long)n);
    SS_REQUIRE(state != nullptr && eps != nullptr, "multistep_cfg_step: NULL state or eps");
    SS_REQUIRE(std::isfinite(guidance) && std::isfinite(sigma) && std::isfinite(a) && std::isfinite(b) && std::isfinite(c) &&
                   std::isfinite(inv_next),
               "multistep_cfg_step: non-finite coefficient (guidance %g sigma %g a %g b %g c %g inv_next %g)", (double)guidance,
               (double)sigma, (double)a, (double)b, (double)c, (double)inv_next);
    SS_REQUIRE((uintptr_t)state % sizeof(float) == 0 && (dtype == SS_F32 || dtype == SS_BF16 || dtype == SS_F16),
               "multistep_cfg_step: unknown dtype %d or misaligned state", dtype);
    return SS_DISPATCH(dtype, multistep_cfg_step_launch, state, eps, x_out, xin_next, n, guidance, sigma, a, b, c, inv_next,
                       (hipStream_t)stream);
}
int ss_multistep_step(float* state, const void* eps, void* x_out, void* xin_next, int64_t n, int eps_rows, int xin_rows,
                      float guidance, float sigma, float a, float b, float c, float inv_next, int dtype, void* stream) {
    SS_REQUIRE(n > 0, "multistep_step: n = %lld", (long long)n);
    SS_REQUIRE(state != nullptr && eps != nullptr, "multistep_step: NULL state or eps");
    SS_REQUIRE((eps_rows == 1 || eps_rows == 2) && (xin_rows == 1 || xin_rows == 2),
               "multistep_step: eps_rows %d / xin_rows %d (1 or 2)", eps_rows, xin_rows);
    SS_REQUIRE(std::isfinite(guidance) && std::isfinite(sigma) && std::isfinite(a) && std::isfinite(b) && std::isfinite(c) &&
                   std::isfinite(inv_next),
               "multistep_step: non-finite coefficient (guidance %g sigma %g a %g b %g c %g inv_next %g)", (double)guidance,
               (double)sigma, (double)a, (double)b, (double)c, (double)inv_next);
    SS_REQUIRE((uintptr_t)state % sizeof(float) == 0 && (dtype == SS_F32 || dtype == SS_BF16 || dtype == SS_F16),
               "multistep_step: unknown dtype %d or misaligned state", dtype);
    return SS_DISPATCH(dtype, multistep_step_launch, state, eps, x_out, xin_next, n, eps_rows, xin_rows, guidance, sigma, a, b,
                       c, inv_next, (hipStream_t)stream);
}
int ss_multistep_noise_step(float* state, const void* eps, void* x_out, void* xin_next, int64_t n, int eps_rows, int xin_rows,
                            float guidance, float sigma, float a, float b, float c, float s, float inv_next,
                            const uint64_t* seeds_dev, int64_t n_img, int step, int dtype, void* stream) {
    SS_REQUIRE(n > 0, "multistep_noise_step: n = %lld", (long long)n);
    SS_REQUIRE(state != nullptr && eps != nullptr, "multistep_noise_step: NULL state or eps");
    SS_REQUIRE((eps_rows == 1 || eps_rows == 2) && (xin_rows == 1 || xin_rows == 2),
               "multistep_noise_step: eps_rows %d / xin_rows %d (1 or 2)", eps_rows, xin_rows);
    SS_REQUIRE(n_img > 0 && n_img <= ((int64_t)1 << 34) && n % n_img == 0,
               "multistep_noise_step: n_img = %lld must be in [1, 2^34] and divide n = %lld", (long long)n_img, (long long)n);
    SS_REQUIRE(step >= 0, "multistep_noise_step: step = %d", step);
    SS_REQUIRE(std::isfinite(guidance) && std::isfinite(sigma) && std::isfinite(a) && std::isfinite(b) && std::isfinite(c) &&
                   std::isfinite(s) && std::isfinite(inv_next),
               "multistep_noise_step: non-finite coefficient (guidance %g sigma %g a %g b %g c %g s %g inv_next %g)",
               (double)guidance, (double)sigma, (double)a, (double)b, (double)c, (double)s, (double)inv_next);
    SS_REQUIRE(s == 0.0f || (seeds_dev != nullptr && (uintptr_t)seeds_dev % sizeof(uint64_t) == 0),
               "multistep_noise_step: s = %g needs seeds (NULL or misaligned)", (double)s);
    SS_REQUIRE((uintptr_t)state % sizeof(float) == 0 && (dtype == SS_F32 || dtype == SS_BF16 || dtype == SS_F16),
               "multistep_noise_step: unknown dtype %d or misaligned state", dtype);
    return SS_DISPATCH(dtype, multistep_noise_step_launch, state, eps, x_out, xin_next, n, eps_rows, xin_rows, guidance, sigma, a,
                       b, c, s, inv_next, seeds_dev, n_img, step, (hipStream_t)stream);
}
int ss_randn_philox(void* out, const uint64_t* seeds_dev, int64_t batch, int64_t n_img, int step, int dtype, void* stream) {
    SS_REQUIRE(out != nullptr && seeds_dev != nullptr && (uintptr_t)seeds_dev % sizeof(uint64_t) == 0,
               "randn_philox: NULL out or seeds (or misaligned seeds)");
    SS_REQUIRE(batch > 0 && n_img > 0 && n_img <= ((int64_t)1 << 34), "randn_philox: batch = %lld, n_img = %lld (n_img in [1, 2^34])",
               (long long)batch, (long long)n_img);
    SS_REQUIRE(step >= 0, "randn_philox: step = %d", step);
    SS_REQUIRE(dtype == SS_F32 || dtype == SS_BF16 || dtype == SS_F16, "randn_philox: unknown dtype %d", dtype);
    return SS_DISPATCH(dtype, randn_philox_launch, out, seeds_dev, batch, n_img, step, (hipStream_t)stream);
}
int ss_euler_step(void* x, const void* eps, int64_t n, float sigma, float sigma_next, int dtype, void* stream) {
    SS_REQUIRE(n > 0 && x != nullptr && eps != nullptr, "euler_step: n = %lld or NULL x / eps", (long long)n);
    return SS_DISPATCH(dtype, euler_step_launch, x, eps, n, sigma, sigma_next, (hipStream_t)stream);
}
int ss_euler_scale(const void* x, void* xin, int64_t n, int rows, float sigma, int dtype, void* stream) {
    SS_REQUIRE(n > 0 && x != nullptr && xin != nullptr, "euler_scale: n = %lld or NULL x / xin", (long long)n);
    SS_REQUIRE(rows == 1 || rows == 2, "euler_scale: rows %d (1 or 2)", rows);
    return SS_DISPATCH(dtype, euler_scale_launch, x, xin, n, rows, sigma, (hipStream_t)stream);
}
int ss_image_to_u8(const void* in, void* out_u8, int64_t pixels, int64_t cpad, int dtype, void* stream) {
    return SS_DISPATCH(dtype, image_to_u8_launch, in, out_u8, pixels, cpad, (hipStream_t)stream);
}

}  // extern "C"

// ---- debug probe: semantics of ds_read_b64_tr_b16 (used when developing the attention kernel) -----------
namespace ss {
typedef short v4s_t __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) v4s_t lds_v4s_t;
__global__ void tr_probe_kernel(const uint16_t* src, uint16_t* dst, const int* lane_off) {
    __shared__ __attribute__((aligned(16))) uint16_t sm[4096];
    for (int i = threadIdx.x; i < 4096; i += 64) sm[i] = src[i];
    __syncthreads();
    const int off = lane_off[threadIdx.x];
    v4s_t r = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s_t*)(sm + off));
    for (int j = 0; j < 4; ++j) dst[threadIdx.x * 4 + j] = (uint16_t)r[j];
}
}  // namespace ss
extern "C" int ss_debug_tr_probe(const void* src, void* dst, const void* lane_off, void* stream) {
    hipLaunchKernelGGL(ss::tr_probe_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const uint16_t*)src,
                       (uint16_t*)dst, (const int*)lane_off);
    SS_LAUNCH_CHECK("tr_probe");
    return SS_OK;
}
