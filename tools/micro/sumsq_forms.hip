// Round 11, part F: why does grad_sumsq_kernel (csrc/heads.hip) read 2 x 56 MB in 38 us (3.0 TB/s) where a fill over the same buffer reaches
// 6-7 TB/s?  Stand-alone forms of the kernel's reduction, alone on the GPU, one knob at a time:
//   PAT 0: the kernel's pattern -- a thread's U loads of a trip are `stride` = grid x 256 float4 apart (U streams through the buffer)
//   PAT 1: a workgroup owns one contiguous range; a thread's U loads of a trip are 256 float4 (4 KB) apart
//   RED 0: the kernel's reduction -- fp32 partial per thread, fp64 wave shuffles + LDS, one fp64 atomic per workgroup
//   RED 1: fp32 wave shuffles, the four wave sums added in fp64, one fp64 atomic per workgroup
//   RED 2: RED 0 without the atomic (a store per workgroup): what the atomic tail costs
//   cap: the grid's block limit per model (the kernel: 1024)
//   T: threads per workgroup (the kernel: 256) -- the same threads in a quarter of the workgroups issue a quarter of the atomics
// Build: hipcc -O3 --offload-arch=gfx950 -o tools/micro/sumsq_forms tools/micro/sumsq_forms.hip      Run: tools/micro/sumsq_forms [floats per model]
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); exit(1); } } while (0)

struct Args { const float* g[2]; double* out[2]; double* part; long long n; };

__device__ __forceinline__ float sq4(const float4 g, float a) { a = fmaf(g.x, g.x, a); a = fmaf(g.y, g.y, a); a = fmaf(g.z, g.z, a); return fmaf(g.w, g.w, a); }

template <int PAT, int RED, int U, int T>
__global__ __launch_bounds__(T) void sumsq_form(const Args a) {
    const float4* __restrict__ g = (const float4*)a.g[blockIdx.z];
    __shared__ double red[T / 64];
    const long long n4 = a.n >> 2;
    float acc[U];
#pragma unroll
    for (int u = 0; u < U; ++u) acc[u] = 0.f;
    if (PAT == 0) {
        const long long stride = (long long)gridDim.x * T;
        long long i = (long long)blockIdx.x * T + threadIdx.x;
        for (; i + (U - 1) * stride < n4; i += U * stride) {
            float4 v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) v[u] = g[i + u * stride];
#pragma unroll
            for (int u = 0; u < U; ++u) acc[u] = sq4(v[u], acc[u]);
        }
        for (; i < n4; i += stride) acc[0] = sq4(g[i], acc[0]);
    } else {
        const long long per = (n4 + gridDim.x - 1) / gridDim.x;
        const long long lo = (long long)blockIdx.x * per, hi = lo + per < n4 ? lo + per : n4;
        long long i = lo + threadIdx.x;
        for (; i + (U - 1) * T < hi; i += U * T) {
            float4 v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) v[u] = g[i + u * T];
#pragma unroll
            for (int u = 0; u < U; ++u) acc[u] = sq4(v[u], acc[u]);
        }
        for (; i < hi; i += T) acc[0] = sq4(g[i], acc[0]);
    }
    float s = acc[0];
#pragma unroll
    for (int u = 1; u < U; ++u) s += acc[u];
    if (blockIdx.x == 0 && threadIdx.x < (a.n & 3)) { const float t = a.g[blockIdx.z][(n4 << 2) + threadIdx.x]; s = fmaf(t, t, s); }
    double t;
    if (RED == 1) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = (double)s;
        __syncthreads();
        t = 0; for (int w = 0; w < T / 64; ++w) t += red[w];
    } else {
        double d = (double)s;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) d += __shfl_xor(d, o, 64);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = d;
        __syncthreads();
        t = 0; for (int w = 0; w < T / 64; ++w) t += red[w];
    }
    if (threadIdx.x == 0) {
        if (RED == 2) a.part[(size_t)blockIdx.z * gridDim.x + blockIdx.x] = t;
        else atomicAdd(a.out[blockIdx.z], t);
    }
}

template <int PAT, int RED, int U, int T = 256>
static void run(const char* name, Args a, int ng, long long cap, double want) {
    long long blocks = (a.n / (4 * U) + T - 1) / T;
    if (cap > 0 && blocks > cap) blocks = cap;
    if (blocks < 1) blocks = 1;
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    float us[2];
    for (int rep = 0; rep < 2; ++rep) {
        for (int i = 0; i < 5; ++i) hipLaunchKernelGGL((sumsq_form<PAT, RED, U, T>), dim3((unsigned)blocks, 1, ng), dim3(T), 0, 0, a);
        CK(hipDeviceSynchronize());
        CK(hipEventRecord(e0, 0));
        for (int i = 0; i < 200; ++i) hipLaunchKernelGGL((sumsq_form<PAT, RED, U, T>), dim3((unsigned)blocks, 1, ng), dim3(T), 0, 0, a);
        CK(hipEventRecord(e1, 0));
        CK(hipEventSynchronize(e1));
        float ms; CK(hipEventElapsedTime(&ms, e0, e1));
        us[rep] = ms * 1e3f / 200;
    }
    double rel = -1;
    if (RED != 2) {
        CK(hipMemset(a.out[0], 0, 8));
        hipLaunchKernelGGL((sumsq_form<PAT, RED, U, T>), dim3((unsigned)blocks, 1, 1), dim3(T), 0, 0, a);
        double got; CK(hipMemcpy(&got, a.out[0], 8, hipMemcpyDeviceToHost));
        rel = (got - want) / want; if (rel < 0) rel = -rel;
    }
    const double tb = (double)a.n * 4 * ng / 1e12;
    printf("ng=%d %-82s blocks %5lld  %7.2f / %7.2f us  %5.2f TB/s  rel err vs fp64 %.2e\n", ng, name, blocks, us[0], us[1], tb / (us[0] < us[1] ? us[0] : us[1]) * 1e6, rel);
    fflush(stdout);
}

int main(int argc, char** argv) {
    const long long n = argc > 1 ? atoll(argv[1]) : 14100000LL;
    std::vector<float> h(n);
    unsigned x = 12345u; double want = 0;
    for (long long i = 0; i < n; ++i) { x = x * 1664525u + 1013904223u; h[i] = ((int)(x >> 8) - (1 << 23)) * (1.0f / (1 << 23)) * 1e-2f; want += (double)h[i] * (double)h[i]; }
    Args a{}; a.n = n;
    float* g[2];
    for (int k = 0; k < 2; ++k) {
        CK(hipMalloc(&g[k], n * 4)); CK(hipMemcpy(g[k], h.data(), n * 4, hipMemcpyHostToDevice)); a.g[k] = g[k];
        CK(hipMalloc(&a.out[k], 8)); CK(hipMemset(a.out[k], 0, 8));
    }
    CK(hipMalloc(&a.part, 2 * 65536 * 8));
    printf("%lld floats per model (%.1f MB), 200 launches per figure, a / b; TB/s from the better one\n", n, n * 4 / 1e6);
    for (int ng = 2; ng >= 1; --ng) {
        run<0, 0, 4>("the kernel's form: strided x4, fp64 reduce, cap 1024", a, ng, 1024, want);
        run<0, 2, 4>("  ... without the atomic", a, ng, 1024, want);
        run<0, 1, 4>("  ... fp32 wave reduce", a, ng, 1024, want);
        run<0, 0, 4>("  ... cap 2048", a, ng, 2048, want);
        run<0, 0, 4>("  ... cap 4096 (= no cap at this size)", a, ng, 4096, want);
        run<0, 0, 8>("  ... 8 loads in flight, cap 1024", a, ng, 1024, want);
        run<0, 0, 8>("  ... 8 loads in flight, no cap", a, ng, 0, want);
        run<1, 0, 4>("contiguous range per workgroup x4, fp64 reduce, cap 1024", a, ng, 1024, want);
        run<1, 0, 4>("  ... cap 2048", a, ng, 2048, want);
        run<1, 0, 4>("  ... no cap", a, ng, 0, want);
        run<1, 0, 8>("  ... 8 loads in flight, cap 1024", a, ng, 1024, want);
        run<1, 0, 8>("  ... 8 loads in flight, cap 2048", a, ng, 2048, want);
        run<1, 1, 8>("  ... 8 loads in flight, cap 2048, fp32 wave reduce", a, ng, 2048, want);
        run<0, 0, 4, 1024>("strided x4, fp64 reduce, 1024 threads, cap 256 (one atomic per 4 of the kernel's)", a, ng, 256, want);
        run<0, 0, 4, 1024>("  ... cap 128", a, ng, 128, want);
        run<0, 0, 4, 1024>("  ... cap 512", a, ng, 512, want);
        run<0, 0, 4, 512>("  ... 512 threads, cap 512", a, ng, 512, want);
        run<0, 0, 8, 1024>("  ... 1024 threads, 8 loads in flight, cap 256", a, ng, 256, want);
    }
    return 0;
}
