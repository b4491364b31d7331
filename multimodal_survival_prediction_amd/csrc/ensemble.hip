// Ensemble reduce: the K fold models' values of one tensor (a saliency volume, a gene-gradient matrix, the hazards) -> their mean and
// their population standard deviation, element by element (include/mmsurv.h: EnsP).
// A streaming kernel: (K + 2) n floats cross the memory interface once, 16 bytes per lane and access, in a grid-stride loop over a grid
// sized to the chip; the last n % 4 elements take a scalar tail.  K is a template parameter so that an element's K values stay in
// registers between the two passes (sum in member order -> mean; deviations from the finished mean -> spread): no LDS, no atomics, no
// scratch.  Nothing is masked: a NaN or an infinity in any member reaches both outputs.
#include "common.h"

static_assert(MMS_MAX_GROUP == 10, "EnsP.x and ens_launch's dispatch are written for 10 members");

struct EnsArgs { const float* x[MMS_MAX_GROUP]; size_t n; float* mean; float* spread; };

template <int K> __device__ __forceinline__ void ens_one(const float (&v)[K], float& mean, float& spread) {
    float s = v[0];
#pragma unroll
    for (int g = 1; g < K; ++g) s += v[g];
    mean = s / (float)K;
    float q = 0.f;
#pragma unroll
    for (int g = 0; g < K; ++g) { const float d = v[g] - mean; q += d * d; }
    spread = sqrtf(q / (float)K);
}

template <int K> __global__ __launch_bounds__(256) void ensemble_reduce_kernel(const EnsArgs a) {
    const size_t nvec = a.n >> 2, stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += stride) {
        float4 v[K];
#pragma unroll
        for (int g = 0; g < K; ++g) v[g] = ((const float4*)a.x[g])[i];
        float4 m, sp;
        {
            float e[K];
#pragma unroll
            for (int g = 0; g < K; ++g) e[g] = v[g].x;
            ens_one<K>(e, m.x, sp.x);
#pragma unroll
            for (int g = 0; g < K; ++g) e[g] = v[g].y;
            ens_one<K>(e, m.y, sp.y);
#pragma unroll
            for (int g = 0; g < K; ++g) e[g] = v[g].z;
            ens_one<K>(e, m.z, sp.z);
#pragma unroll
            for (int g = 0; g < K; ++g) e[g] = v[g].w;
            ens_one<K>(e, m.w, sp.w);
        }
        ((float4*)a.mean)[i] = m;
        if (a.spread) ((float4*)a.spread)[i] = sp;
    }
    const size_t t = (nvec << 2) + threadIdx.x;       // scalar tail: the first n % 4 lanes of workgroup 0
    if (blockIdx.x == 0 && threadIdx.x < 4 && t < a.n) {
        float e[K], m, sp;
#pragma unroll
        for (int g = 0; g < K; ++g) e[g] = a.x[g][t];
        ens_one<K>(e, m, sp);
        a.mean[t] = m;
        if (a.spread) a.spread[t] = sp;
    }
}

template <int K> static void ens_launch(const EnsArgs& a, unsigned grid, hipStream_t s) {
    MMS_LAUNCH(ensemble_reduce_kernel<K>, dim3(grid), dim3(256), 0, s, a);
}

extern "C" int mms_ensemble_reduce(const EnsP* p, hipStream_t s) {
    if (!p || p->K < 1 || p->K > MMS_MAX_GROUP || p->n == 0 || !p->mean) return MMS_ERR_ARG;
    auto al16 = [](const void* q) { return ((uintptr_t)q & 15) == 0; };
    if (!al16(p->mean) || !al16(p->spread)) return MMS_ERR_ARG;
    EnsArgs a{};
    for (int g = 0; g < p->K; ++g) {
        if (!p->x[g] || !al16(p->x[g])) return MMS_ERR_ARG;
        a.x[g] = p->x[g];
    }
    a.n = p->n; a.mean = p->mean; a.spread = p->spread;
    // 8 workgroups of 256 lanes per CU of a 256-CU chip keep enough 16-byte loads in flight; smaller problems get what they need
    const size_t nvec = p->n >> 2, want = (nvec + 255) / 256;
    const unsigned grid = (unsigned)(want < 1 ? 1 : (want > 2048 ? 2048 : want));
    switch (p->K) {
        case 1: ens_launch<1>(a, grid, s); break;
        case 2: ens_launch<2>(a, grid, s); break;
        case 3: ens_launch<3>(a, grid, s); break;
        case 4: ens_launch<4>(a, grid, s); break;
        case 5: ens_launch<5>(a, grid, s); break;
        case 6: ens_launch<6>(a, grid, s); break;
        case 7: ens_launch<7>(a, grid, s); break;
        case 8: ens_launch<8>(a, grid, s); break;
        case 9: ens_launch<9>(a, grid, s); break;
        default: ens_launch<10>(a, grid, s); break;
    }
    return mms_check_launch();
}
