// A/B micro-benchmark of one conv3x3 shape on two tiles: build BASE with tile A against build NEW with tile B (the two builds may
// be the same file), in ONE process (dlopen, local symbols), timed interleaved, no torch.  Written for the upsampling
// convolutions (old: the one-barrier tile of the table, new: a ping-pong tile) and for cfg 56 against cfg 58 on stride-1 shapes.
//
//   hipcc -O2 --offload-arch=gfx950 tools/conv_up_ubench.cpp -o tools/bin/conv_up_ubench -ldl
//   tools/bin/conv_up_ubench <base.so> <new.so> <case> ...      case = B,H,W,Cin,Cout,up:cfgA/swzA:cfgB/swzB   (H, W of the SOURCE)
//
// Operands are pseudo-random bf16 (as conv_stage_ubench.cpp), weights rotate over copies (sustained mode, one HIP event pair per
// round, 7 interleaved rounds; min, median, max).  B's output is compared with A's bit for bit.  One JSON object per case.
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(2); } } while (0)

typedef int (*conv_fn)(const void*, const void*, void*, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, const void*,
                       const void*, int64_t, const void*, int, void*);
typedef int (*tune_fn)(const char*, int);

struct Lib { conv_fn conv; tune_fn tune; };

static Lib load(const char* path) {
    void* h = dlopen(path, RTLD_NOW | RTLD_LOCAL);
    if (!h) { fprintf(stderr, "dlopen %s: %s\n", path, dlerror()); exit(2); }
    Lib l{(conv_fn)dlsym(h, "ss_conv3x3"), (tune_fn)dlsym(h, "ss_set_tuning")};
    if (!l.conv || !l.tune) { fprintf(stderr, "%s: missing symbols\n", path); exit(2); }
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
    if (argc < 4) { fprintf(stderr, "usage: %s base.so new.so B,H,W,Cin,Cout,up:cfgA/swzA:cfgB/swzB ...\n", argv[0]); return 2; }
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
        long B, H, W, Cin, Cout, up;
        int cfg[2], swz[2];
        if (sscanf(argv[a], "%ld,%ld,%ld,%ld,%ld,%ld:%d/%d:%d/%d", &B, &H, &W, &Cin, &Cout, &up, &cfg[0], &swz[0], &cfg[1], &swz[1]) != 10) {
            fprintf(stderr, "bad case %s\n", argv[a]);
            return 2;
        }
        const int64_t M = B * H * W * (up ? 4 : 1), N = Cout, K = 9 * Cin;
        const size_t x_elems = (size_t)B * H * W * Cin, w_elems = (size_t)N * K, c_elems = (size_t)M * N;
        size_t nW = std::min<size_t>(64, std::max<size_t>(2, ((size_t)352 << 20) / (w_elems * 2)));
        uint16_t *dX, *dW, *dC, *dRef, *dBias;
        CK(hipMalloc(&dX, x_elems * 2));
        CK(hipMalloc(&dW, nW * w_elems * 2));
        CK(hipMalloc(&dC, c_elems * 2));
        CK(hipMalloc(&dRef, c_elems * 2));
        CK(hipMalloc(&dBias, (size_t)N * 2));
        fill<<<2048, 256, 0, s>>>(dX, x_elems, 0x1234u, 1.0f);
        fill<<<2048, 256, 0, s>>>(dW, nW * w_elems, 0x9876u, 0.05f);
        fill<<<64, 256, 0, s>>>(dBias, (size_t)N, 0x55u, 0.5f);
        CK(hipStreamSynchronize(s));
        auto launch = [&](int v, const uint16_t* w, uint16_t* c) {
            const Lib& l = libs[v];
            l.tune("gemm_cfg", cfg[v]);
            l.tune("gemm_xcd_swizzle", swz[v]);
            const int rc = l.conv(dX, w, c, B, H, W, Cin, Cout, 1, up, dBias, nullptr, 0, nullptr, BF16, s);
            if (rc) { fprintf(stderr, "launch variant %d cfg %d failed: %d\n", v, cfg[v], rc); exit(3); }
        };
        launch(0, dW, dRef);
        launch(1, dW, dC);
        CK(hipMemsetAsync(dstat, 0, 4, s));
        count_diff<<<1024, 256, 0, s>>>(dC, dRef, c_elems, dstat);
        unsigned ndiff = 0;
        CK(hipMemcpyAsync(&ndiff, dstat, 4, hipMemcpyDeviceToHost, s));
        CK(hipStreamSynchronize(s));
        const int R = (int)std::max<size_t>(nW + nW / 2, 12), ROUNDS = 7;
        std::vector<float> us[2];
        for (int round = 0; round < ROUNDS; ++round)
            for (int v = 0; v < 2; ++v) {
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
        for (int v = 0; v < 2; ++v) std::sort(us[v].begin(), us[v].end());
        const int md = ROUNDS / 2;
        const double tf = 2.0 * (double)M * N * K * 1e-6;
        printf("{\"case\": \"%s\", \"M\": %ld, \"N\": %ld, \"K\": %ld, \"up\": %ld, \"a\": {\"cfg\": %d, \"swz\": %d, \"us_min\": %.1f, \"us_median\": %.1f, "
               "\"us_max\": %.1f, \"tflops\": %.1f}, \"b\": {\"cfg\": %d, \"swz\": %d, \"us_min\": %.1f, \"us_median\": %.1f, \"us_max\": %.1f, \"tflops\": %.1f}, "
               "\"b_over_a\": %.4f, \"elements_not_bit_equal\": %u}\n",
               argv[a], (long)M, (long)N, (long)K, up, cfg[0], swz[0], us[0][0], us[0][md], us[0].back(), tf / us[0][md], cfg[1], swz[1],
               us[1][0], us[1][md], us[1].back(), tf / us[1][md], us[1][md] / us[0][md], ndiff);
        fflush(stdout);
        CK(hipFree(dX)); CK(hipFree(dW)); CK(hipFree(dC)); CK(hipFree(dRef)); CK(hipFree(dBias));
    }
    return 0;
}
