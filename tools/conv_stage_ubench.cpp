// A/B micro-benchmark of the ping-pong conv3x3 tiles: TWO builds of the library in ONE process (dlopen, local symbols), the
// convolution of each and the plain GEMM of equal (M, N, K) on the same tile id, timed interleaved.  What it reports is the
// conv / GEMM time ratio per build: the GEMM of equal shape is the ceiling of the tile, the ratio is what conv staging costs.
//
//   hipcc -O2 --offload-arch=gfx950 tools/conv_stage_ubench.cpp -o tools/bin/conv_stage_ubench -ldl
//   tools/bin/conv_stage_ubench <base.so> <new.so> <case> ...      case = B,H,W,Cin,Cout:cfg[/swz]
//
// Operands are pseudo-random bf16 (as gemm_ubench.cpp), weights rotate over copies (sustained mode, one HIP event pair per
// round, 7 interleaved rounds, min and median).  The new build's output is compared with the base build's bit for bit.
// Prints one JSON object per case.
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(2); } } while (0)

typedef int (*gemm_fn)(const void*, const void*, void*, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, const void*, const void*,
                       int64_t, int, int, void*);
typedef int (*conv_fn)(const void*, const void*, void*, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, const void*,
                       const void*, int64_t, const void*, int, void*);
typedef int (*tune_fn)(const char*, int);

struct Lib { gemm_fn gemm; conv_fn conv; tune_fn tune; };

static Lib load(const char* path) {
    void* h = dlopen(path, RTLD_NOW | RTLD_LOCAL);
    if (!h) { fprintf(stderr, "dlopen %s: %s\n", path, dlerror()); exit(2); }
    Lib l{(gemm_fn)dlsym(h, "ss_gemm"), (conv_fn)dlsym(h, "ss_conv3x3"), (tune_fn)dlsym(h, "ss_set_tuning")};
    if (!l.gemm || !l.conv || !l.tune) { fprintf(stderr, "%s: missing symbols\n", path); exit(2); }
    return l;
}

__global__ void fill(uint16_t* p, size_t n, uint32_t seed, float scale) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        uint32_t x = (uint32_t)i * 2654435761u + seed;
        x ^= x >> 15; x *= 2246822519u; x ^= x >> 13; x *= 3266489917u; x ^= x >> 16;
        const float f = ((float)(x >> 8) * (1.0f / 8388608.0f) - 1.0f) * scale;
        uint32_t u = __float_as_uint(f);
        u += 0x7fffu + ((u >> 16) & 1u);
        p[i] = (uint16_t)(u >> 16);
    }
}
__global__ void count_diff(const uint16_t* a, const uint16_t* b, size_t n, unsigned* out) {
    unsigned nd = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) nd += a[i] != b[i];
    if (nd) atomicAdd(out, nd);
}

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: %s base.so new.so B,H,W,Cin,Cout:cfg[/swz] ...\n", argv[0]); return 2; }
    Lib libs[2] = {load(argv[1]), load(argv[2])};
    hipStream_t s;
    CK(hipStreamCreate(&s));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    unsigned* dstat;
    CK(hipMalloc(&dstat, 4));
    const int BF16 = 1;
    for (int a = 3; a < argc; ++a) {
        long B, H, W, Cin, Cout;
        int cfg, swz = 8;
        const int got = sscanf(argv[a], "%ld,%ld,%ld,%ld,%ld:%d/%d", &B, &H, &W, &Cin, &Cout, &cfg, &swz);
        if (got < 6) { fprintf(stderr, "bad case %s\n", argv[a]); return 2; }
        const int64_t M = B * H * W, N = Cout, K = 9 * Cin;
        const size_t x_elems = (size_t)M * Cin, a_elems = (size_t)M * K, w_elems = (size_t)N * K, c_elems = (size_t)M * N;
        size_t nW = std::min<size_t>(64, std::max<size_t>(2, ((size_t)352 << 20) / (w_elems * 2)));
        uint16_t *dX, *dA, *dW, *dC, *dRef, *dBias;
        CK(hipMalloc(&dX, x_elems * 2));
        CK(hipMalloc(&dA, a_elems * 2));
        CK(hipMalloc(&dW, nW * w_elems * 2));
        CK(hipMalloc(&dC, c_elems * 2));
        CK(hipMalloc(&dRef, c_elems * 2));
        CK(hipMalloc(&dBias, (size_t)N * 2));
        fill<<<2048, 256, 0, s>>>(dX, x_elems, 0x1234u, 1.0f);
        fill<<<2048, 256, 0, s>>>(dA, a_elems, 0x4321u, 1.0f);
        fill<<<2048, 256, 0, s>>>(dW, nW * w_elems, 0x9876u, 0.05f);
        fill<<<64, 256, 0, s>>>(dBias, (size_t)N, 0x55u, 0.5f);
        CK(hipStreamSynchronize(s));
        // variant v: 0 base conv | 1 new conv | 2 base GEMM | 3 new GEMM
        auto launch = [&](int v, const uint16_t* w, uint16_t* c) {
            const Lib& l = libs[v & 1];
            l.tune("gemm_cfg", cfg);
            l.tune("gemm_xcd_swizzle", swz);
            const int rc = v < 2 ? l.conv(dX, w, c, B, H, W, Cin, Cout, 1, 0, dBias, nullptr, 0, nullptr, BF16, s)
                                 : l.gemm(dA, w, c, M, N, K, K, K, N, dBias, nullptr, N, 1, BF16, s);
            if (rc) { fprintf(stderr, "launch variant %d cfg %d failed: %d\n", v, cfg, rc); exit(3); }
        };
        launch(0, dW, dRef);
        launch(1, dW, dC);
        CK(hipMemsetAsync(dstat, 0, 4, s));
        count_diff<<<1024, 256, 0, s>>>(dC, dRef, c_elems, dstat);
        unsigned ndiff = 0;
        CK(hipMemcpyAsync(&ndiff, dstat, 4, hipMemcpyDeviceToHost, s));
        CK(hipStreamSynchronize(s));
        const int R = (int)std::max<size_t>(nW + nW / 2, 12), ROUNDS = 7;
        std::vector<float> us[4];
        for (int round = 0; round < ROUNDS; ++round)
            for (int v = 0; v < 4; ++v) {
                launch(v, dW, dC);
                launch(v, dW + w_elems, dC);
                CK(hipEventRecord(e0, s));
                for (int r = 0; r < R; ++r) launch(v, dW + (size_t)(r % nW) * w_elems, dC);
                CK(hipEventRecord(e1, s));
                CK(hipEventSynchronize(e1));
                float ms;
                CK(hipEventElapsedTime(&ms, e0, e1));
                us[v].push_back(ms * 1e3f / R);
            }
        for (int v = 0; v < 4; ++v) std::sort(us[v].begin(), us[v].end());
        const int md = ROUNDS / 2;
        const double tf = 2.0 * (double)M * N * K * 1e-6;
        printf("{\"case\": \"%s\", \"M\": %ld, \"N\": %ld, \"K\": %ld, \"cfg\": %d, \"swz\": %d, \"elements_not_bit_equal_new_vs_base\": %u, "
               "\"conv_us_base\": {\"min\": %.1f, \"median\": %.1f, \"max\": %.1f}, \"conv_us_new\": {\"min\": %.1f, \"median\": %.1f, \"max\": %.1f}, "
               "\"gemm_us_base\": {\"min\": %.1f, \"median\": %.1f}, \"gemm_us_new\": {\"min\": %.1f, \"median\": %.1f}, "
               "\"conv_over_gemm_base\": %.4f, \"conv_over_gemm_new\": %.4f, \"conv_tflops_base\": %.1f, \"conv_tflops_new\": %.1f, \"gemm_tflops\": %.1f}\n",
               argv[a], (long)M, (long)N, (long)K, cfg, swz, ndiff, us[0][0], us[0][md], us[0].back(), us[1][0], us[1][md], us[1].back(),
               us[2][0], us[2][md], us[3][0], us[3][md], us[0][md] / us[2][md], us[1][md] / us[3][md], tf / us[0][md], tf / us[1][md],
               tf / std::min(us[2][md], us[3][md]));
        fflush(stdout);
        CK(hipFree(dX)); CK(hipFree(dA)); CK(hipFree(dW)); CK(hipFree(dC)); CK(hipFree(dRef)); CK(hipFree(dBias));
    }
    return 0;
}
