// Preprocessing upstream of the hot path, on the GPU:
//   * CT volume: min-max normalisation + order-1 resample to the network grid -- the reference does this per item on the
//     CPU with numpy + scipy.ndimage.zoom(order=1) (R/scripts/training/partial_modality_training.py:94-109,
//     simple_fusion.py:117-134, flexible_multimodal.py:118-128);
//   * RNA-seq counts: log2(count + 1) then per-gene z-score over the cohort (sklearn StandardScaler, ddof 0)
//     (R/scripts/preprocessing/preprocess_genomic.py:108-117).
#include "common.h"
#include "ct_resample.h"
#include <float.h>

// ---- per-volume min / max: stage 1 -> [blocks][2] partials, stage 2 (inside the resample kernel's prologue) ----
__global__ __launch_bounds__(256) void minmax_partial_kernel(const float* __restrict__ x, long long n, float* __restrict__ part) {
    __shared__ float smin[4], smax[4];
    float lo = FLT_MAX, hi = -FLT_MAX;
    const long long stride = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) { const float v = x[i]; lo = fminf(lo, v); hi = fmaxf(hi, v); }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { lo = fminf(lo, __shfl_xor(lo, o, 64)); hi = fmaxf(hi, __shfl_xor(hi, o, 64)); }
    if ((threadIdx.x & 63) == 0) { smin[threadIdx.x >> 6] = lo; smax[threadIdx.x >> 6] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = fminf(fminf(smin[0], smin[1]), fminf(smin[2], smin[3]));
        part[2 * blockIdx.x + 1] = fmaxf(fmaxf(smax[0], smax[1]), fmaxf(smax[2], smax[3]));
    }
}

// Output voxel = ct_interp_norm (ct_resample.h) of x - min: the reference value is subtracted BEFORE the interpolation.  The
// normalisation is affine and would commute with the interpolation in exact arithmetic; in fp32 it does not (a (1 - f) + a f is not
// a), and normalising the interpolated value made a constant volume non-zero and lost low contrast on a large offset.
__global__ __launch_bounds__(256) void ct_resample_norm_kernel(const float* __restrict__ x, Dims3 in, float* __restrict__ out, Dims3 o,
                                                               const float* __restrict__ part, int nparts) {
    __shared__ float mm[2];
    if (threadIdx.x < 64) {
        float lo = FLT_MAX, hi = -FLT_MAX;
        for (int i = threadIdx.x; i < nparts; i += 64) { lo = fminf(lo, part[2 * i]); hi = fmaxf(hi, part[2 * i + 1]); }
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) { lo = fminf(lo, __shfl_xor(lo, s, 64)); hi = fmaxf(hi, __shfl_xor(hi, s, 64)); }
        if (threadIdx.x == 0) { mm[0] = lo; mm[1] = hi; }
    }
    __syncthreads();
    const float lo = mm[0], sc = ct_norm_scale(1.0f, mm[0], mm[1]);
    const long long n = (long long)o.D * o.H * o.W;
    const double sd = ct_axis_step(in.D, o.D), sh = ct_axis_step(in.H, o.H), sw = ct_axis_step(in.W, o.W);
    auto at = [&](int d, int h, int w) { return x[((size_t)d * in.H + h) * in.W + w] - lo; };
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (long long)gridDim.x * 256) {
        const int ow = (int)(idx % o.W), oh = (int)((idx / o.W) % o.H), od = (int)(idx / ((long long)o.W * o.H));
        out[idx] = ct_interp_norm(at, in, od, oh, ow, sd, sh, sw, sc);
    }
}

// x: one volume [inD][inH][inW] (device), out: [oD][oH][oW], scratch: >= 2 * 256 floats
extern "C" int mms_ct_preprocess(const float* x, int inD, int inH, int inW, float* out, int oD, int oH, int oW, float* scratch, hipStream_t s) {
    if (!x || !out || !scratch || inD <= 0 || inH <= 0 || inW <= 0 || oD <= 0 || oH <= 0 || oW <= 0) return MMS_ERR_ARG;
    const long long n = (long long)inD * inH * inW;
    int nb = (int)((n + 256 * 16 - 1) / (256 * 16));
    if (nb < 1) nb = 1;
    if (nb > 256) nb = 256;
    MMS_LAUNCH(minmax_partial_kernel, dim3(nb), dim3(256), 0, s, x, n, scratch);
    const long long no = (long long)oD * oH * oW;
    int ob = (int)((no + 255) / 256);
    if (ob > 2048) ob = 2048;
    MMS_LAUNCH(ct_resample_norm_kernel, dim3(ob), dim3(256), 0, s, x, Dims3{inD, inH, inW}, out, Dims3{oD, oH, oW}, (const float*)scratch, nb);
    return mms_check_launch();
}

// counts [n][g] row-major -> out [n][g] = zscore_over_rows(log2(count + 1)); zero-variance genes keep scale 1 (sklearn).
// one workgroup per 64 genes: 4 row-groups x 64 columns.  Everything up to the store is fp64, in three reads of the column: the mean,
// then sum (v - mean)^2 (the one-pass E[v^2] - mean^2 cancels for a well-expressed stable gene: v ~ 17, sd ~ 1e-2 and below), then
// (float)((v - mean) / sd) -- centring in fp32 would cost ulp(17) / sd.
__global__ __launch_bounds__(256) void rna_log_zscore_kernel(const float* __restrict__ c, float* __restrict__ out, int n, int g) {
    __shared__ double ssum[4][64];
    __shared__ double smean[64], sinv[64];
    const int lane = threadIdx.x & 63, col = blockIdx.x * 64 + lane, rg = threadIdx.x >> 6;
    double s1 = 0;
    if (col < g)
        for (int r = rg; r < n; r += 4) s1 += log2((double)c[(size_t)r * g + col] + 1.0);
    ssum[rg][lane] = s1;
    __syncthreads();
    if (rg == 0) smean[lane] = (ssum[0][lane] + ssum[1][lane] + ssum[2][lane] + ssum[3][lane]) / n;
    __syncthreads();
    const double m = smean[lane];
    double s2 = 0;
    if (col < g)
        for (int r = rg; r < n; r += 4) { const double e = log2((double)c[(size_t)r * g + col] + 1.0) - m; s2 += e * e; }
    ssum[rg][lane] = s2;                                       // (every read of the first sums is behind the barrier above)
    __syncthreads();
    if (rg == 0) {
        const double sd = sqrt((ssum[0][lane] + ssum[1][lane] + ssum[2][lane] + ssum[3][lane]) / n);
        sinv[lane] = sd < 1e-12 ? 1.0 : 1.0 / sd;              // (sklearn: scale_ == 0 -> 1)
    }
    __syncthreads();
    const double inv = sinv[lane];
    if (col < g)
        for (int r = rg; r < n; r += 4) out[(size_t)r * g + col] = (float)((log2((double)c[(size_t)r * g + col] + 1.0) - m) * inv);
}
extern "C" int mms_rna_log_zscore(const float* counts, float* out, int n, int g, hipStream_t s) {
    if (!counts || !out || n <= 0 || g <= 0) return MMS_ERR_ARG;
    MMS_LAUNCH(rna_log_zscore_kernel, dim3((g + 63) / 64), dim3(256), 0, s, counts, out, n, g);
    return mms_check_launch();
}
