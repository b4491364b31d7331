// CT ingest: mms_ct_preprocess (preproc.hip) for many volumes per launch, straight from the STORED element types of their files --
// the data sections of NIfTI-1 volumes (nifti.py) packed back to back in one device staging buffer.  The reference reads each scan
// with SimpleITK, min-max normalises it with numpy and scipy.ndimage.zoom's it (order 1) to the network grid per item on the CPU
// (R/scripts/training/partial_modality_training.py:91-109, simple_fusion.py:117-134, flexible_multimodal.py:115-128).
//
//   pass 1  per-volume extremes of the raw elements.  Grid (parts, volumes): workgroup (b, v) takes every nb_v-th 16-byte vector of
//           volume v (16 x 8-bit, 8 x 16-bit, 4 x 32-bit or 2 x 64-bit elements a lane and load); workgroup 0 also takes the scalar
//           tail.  Partials go to scratch with plain stores, no atomics.  The only pass that reads the whole scan.
//   pass 2  grid (blocks, volumes): reduce the volume's partials in the prologue, then per output voxel the eight neighbours by typed
//           loads, interpolation in fp32 of (r - rmin) (exact for the integer types of a CT: nothing cancels, a constant volume is 0
//           exactly), times |slope| / (|slope| (rmax - rmin) + 1e-8).  A negative slope swaps the extremes: (rmax - r).
//
// Precision: 8- and 16-bit integers and float32 are exact in fp32; int32, uint32 and float64 elements are rounded to the nearest fp32
// at the load, as a host astype(float32) rounds them.  NaN elements are not supported: fminf / fmaxf drop them from the extremes and
// the output voxels they touch are NaN.
// The element type and the byte order are per volume, i.e. uniform over a workgroup: the switches below are scalar branches.
#include "common.h"
#include "ct_resample.h"
#include <float.h>
#include <cmath>
#include <string.h>
#include <algorithm>
#include <vector>

namespace {

struct VolK { unsigned long long off; int D, H, W; int dtype; int swap; int row; int nb; float slope; };
struct ChunkK { VolK v[MMS_CT_RAW_CHUNK]; };

__device__ __forceinline__ uint8_t bswap_u(uint8_t u) { return u; }
__device__ __forceinline__ uint16_t bswap_u(uint16_t u) { return __builtin_bswap16(u); }
__device__ __forceinline__ uint32_t bswap_u(uint32_t u) { return __builtin_bswap32(u); }
__device__ __forceinline__ uint64_t bswap_u(uint64_t u) { return __builtin_bswap64(u); }

// stored bits (U: the unsigned type of T's width) -> the element's value in fp32 (round to nearest)
template <class T, class U> __device__ __forceinline__ float raw_val(U u, bool swap) {
    static_assert(sizeof(T) == sizeof(U), "storage type");
    if (swap) u = bswap_u(u);
    T t;
    __builtin_memcpy(&t, &u, sizeof(T));
    return (float)t;
}

template <class T, class U>
__device__ __forceinline__ void minmax_body(const unsigned char* __restrict__ x, unsigned n, bool swap, int b, int nb, float& lo, float& hi) {
    constexpr int VEC = 16 / (int)sizeof(U);
    const unsigned nv = n / VEC;
    const uint4* __restrict__ xv = (const uint4*)x;
#pragma unroll 4
    for (unsigned i = (unsigned)b * 256u + threadIdx.x; i < nv; i += (unsigned)nb * 256u) {
        const uint4 q = xv[i];
        U e[VEC];
        __builtin_memcpy(e, &q, 16);
#pragma unroll
        for (int k = 0; k < VEC; ++k) { const float v = raw_val<T, U>(e[k], swap); lo = fminf(lo, v); hi = fmaxf(hi, v); }
    }
    if (b == 0) {                                                      // scalar tail: n % VEC < 16 elements
        const unsigned i = nv * VEC + threadIdx.x;
        if (i < n) { const float v = raw_val<T, U>(((const U*)x)[i], swap); lo = fminf(lo, v); hi = fmaxf(hi, v); }
    }
}

__global__ __launch_bounds__(256) void ct_raw_minmax_kernel(const unsigned char* __restrict__ base, ChunkK c, float* __restrict__ part) {
    const VolK& d = c.v[blockIdx.y];
    const int b = blockIdx.x, nb = d.nb;
    if (b >= nb) return;                                               // (uniform: before any barrier)
    __shared__ float smin[4], smax[4];
    const unsigned char* x = base + d.off;
    const unsigned n = (unsigned)d.D * (unsigned)d.H * (unsigned)d.W;  // < 2^31 (checked on the host)
    const bool sw = d.swap != 0;
    float lo = FLT_MAX, hi = -FLT_MAX;
    switch (d.dtype) {
    case MMS_CT_U8:  minmax_body<uint8_t, uint8_t>(x, n, sw, b, nb, lo, hi); break;
    case MMS_CT_I8:  minmax_body<int8_t, uint8_t>(x, n, sw, b, nb, lo, hi); break;
    case MMS_CT_I16: minmax_body<int16_t, uint16_t>(x, n, sw, b, nb, lo, hi); break;
    case MMS_CT_U16: minmax_body<uint16_t, uint16_t>(x, n, sw, b, nb, lo, hi); break;
    case MMS_CT_I32: minmax_body<int32_t, uint32_t>(x, n, sw, b, nb, lo, hi); break;
    case MMS_CT_U32: minmax_body<uint32_t, uint32_t>(x, n, sw, b, nb, lo, hi); break;
    case MMS_CT_F32: minmax_body<float, uint32_t>(x, n, sw, b, nb, lo, hi); break;
    default:         minmax_body<double, uint64_t>(x, n, sw, b, nb, lo, hi); break;      // MMS_CT_F64 (the host admits nothing else)
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { lo = fminf(lo, __shfl_xor(lo, o, 64)); hi = fmaxf(hi, __shfl_xor(hi, o, 64)); }
    if ((threadIdx.x & 63) == 0) { smin[threadIdx.x >> 6] = lo; smax[threadIdx.x >> 6] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float* p = part + ((size_t)blockIdx.y * MMS_CT_RAW_PARTS + b) * 2;
        p[0] = fminf(fminf(smin[0], smin[1]), fminf(smin[2], smin[3]));
        p[1] = fmaxf(fmaxf(smax[0], smax[1]), fmaxf(smax[2], smax[3]));
    }
}

// t = r - ref (sign +1) or ref - r (sign -1) of the eight neighbours, interpolated and scaled by ct_interp_norm (ct_resample.h): the
// arithmetic of ct_resample_norm_kernel (preproc.hip), so a float32 volume gives the same bits on either route
template <class T, class U>
__device__ __forceinline__ void resample_body(const unsigned char* __restrict__ xb, const VolK& d, bool swap, float ref, float sgn, float sc,
                                              float* __restrict__ out, Dims3 o) {
    const U* __restrict__ x = (const U*)xb;
    const int n = o.D * o.H * o.W;
    const Dims3 in{d.D, d.H, d.W};
    const double sd = ct_axis_step(d.D, o.D), sh = ct_axis_step(d.H, o.H), sw = ct_axis_step(d.W, o.W);
    auto at = [&](int dd, int hh, int ww) {
        return (raw_val<T, U>(x[((unsigned)dd * (unsigned)d.H + (unsigned)hh) * (unsigned)d.W + (unsigned)ww], swap) - ref) * sgn;
    };
    for (long long li = (long long)blockIdx.x * 256 + threadIdx.x; li < n; li += (long long)gridDim.x * 256) {
        const int idx = (int)li, ow = idx % o.W, oh = (idx / o.W) % o.H, od = idx / (o.W * o.H);
        out[idx] = ct_interp_norm(at, in, od, oh, ow, sd, sh, sw, sc);
    }
}

__global__ __launch_bounds__(256) void ct_raw_resample_kernel(const unsigned char* __restrict__ base, ChunkK c, const float* __restrict__ part,
                                                              float* __restrict__ out, Dims3 o) {
    const VolK& d = c.v[blockIdx.y];
    __shared__ float mm[2];
    if (threadIdx.x < 64) {
        const float* p = part + (size_t)blockIdx.y * MMS_CT_RAW_PARTS * 2;
        float lo = FLT_MAX, hi = -FLT_MAX;
        for (int i = threadIdx.x; i < d.nb; i += 64) { lo = fminf(lo, p[2 * i]); hi = fmaxf(hi, p[2 * i + 1]); }
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) { lo = fminf(lo, __shfl_xor(lo, s, 64)); hi = fmaxf(hi, __shfl_xor(hi, s, 64)); }
        if (threadIdx.x == 0) { mm[0] = lo; mm[1] = hi; }
    }
    __syncthreads();
    const float rlo = mm[0], rhi = mm[1];
    const float sc = ct_norm_scale(fabsf(d.slope), rlo, rhi);
    const bool neg = d.slope < 0.f;
    const float ref = neg ? rhi : rlo, sgn = neg ? -1.f : 1.f;
    const unsigned char* x = base + d.off;
    float* orow = out + (size_t)d.row * ((size_t)o.D * o.H * o.W);
    const bool sw = d.swap != 0;
    switch (d.dtype) {
    case MMS_CT_U8:  resample_body<uint8_t, uint8_t>(x, d, sw, ref, sgn, sc, orow, o); break;
    case MMS_CT_I8:  resample_body<int8_t, uint8_t>(x, d, sw, ref, sgn, sc, orow, o); break;
    case MMS_CT_I16: resample_body<int16_t, uint16_t>(x, d, sw, ref, sgn, sc, orow, o); break;
    case MMS_CT_U16: resample_body<uint16_t, uint16_t>(x, d, sw, ref, sgn, sc, orow, o); break;
    case MMS_CT_I32: resample_body<int32_t, uint32_t>(x, d, sw, ref, sgn, sc, orow, o); break;
    case MMS_CT_U32: resample_body<uint32_t, uint32_t>(x, d, sw, ref, sgn, sc, orow, o); break;
    case MMS_CT_F32: resample_body<float, uint32_t>(x, d, sw, ref, sgn, sc, orow, o); break;
    default:         resample_body<double, uint64_t>(x, d, sw, ref, sgn, sc, orow, o); break;
    }
}

int elem_size(int dtype) {
    switch (dtype) {
    case MMS_CT_U8: case MMS_CT_I8: return 1;
    case MMS_CT_I16: case MMS_CT_U16: return 2;
    case MMS_CT_I32: case MMS_CT_U32: case MMS_CT_F32: return 4;
    case MMS_CT_F64: return 8;
    default: return 0;
    }
}

}  // namespace

extern "C" int mms_ct_preprocess_raw_batch(const CtRawBatchP* p, hipStream_t s) {
    if (!p || !p->base || !p->out || !p->scratch) return MMS_ERR_ARG;
    if (((uintptr_t)p->base & 15) || ((uintptr_t)p->out & 3) || ((uintptr_t)p->scratch & 3)) return MMS_ERR_ARG;
    if (p->V < 0 || p->V > MMS_CT_RAW_MAX_VOLS || p->base_bytes < 0 || p->n_rows < 1) return MMS_ERR_ARG;
    if (p->oD < 1 || p->oH < 1 || p->oW < 1) return MMS_ERR_ARG;
    if (p->passes < 0 || p->passes > 2 || (p->passes != 0 && p->V > MMS_CT_RAW_CHUNK)) return MMS_ERR_ARG;
    const long long no = (long long)p->oD * p->oH;                     // (< 2^62)
    if (no > MMS_CT_RAW_MAX_VOXELS || no * p->oW > MMS_CT_RAW_MAX_VOXELS) return MMS_ERR_ARG;
    if (p->V == 0) return MMS_OK;
    if (!p->vols) return MMS_ERR_ARG;
    // every descriptor before any launch
    std::vector<VolK> k((size_t)p->V);
    std::vector<int> rows((size_t)p->V);
    for (int v = 0; v < p->V; ++v) {
        const CtRawVol& d = p->vols[v];
        const int es = elem_size(d.dtype);
        if (es == 0 || d.offset < 0 || (d.offset & 15) || d.D < 1 || d.H < 1 || d.W < 1) return MMS_ERR_ARG;
        const long long dh = (long long)d.D * d.H;
        if (dh > MMS_CT_RAW_MAX_VOXELS || dh * d.W > MMS_CT_RAW_MAX_VOXELS) return MMS_ERR_ARG;
        const long long bytes = dh * d.W * es;                         // (< 2^34)
        if (d.offset > p->base_bytes || bytes > p->base_bytes - d.offset) return MMS_ERR_ARG;
        if (!std::isfinite(d.slope) || !std::isfinite(d.inter)) return MMS_ERR_ARG;
        if (d.out_row < 0 || d.out_row >= p->n_rows) return MMS_ERR_ARG;
        rows[(size_t)v] = d.out_row;
        long long nb = (bytes + 256 * 16 * 4 - 1) / (256 * 16 * 4);    // >= 4 vectors a lane before a second workgroup pays
        nb = nb < 1 ? 1 : (nb > MMS_CT_RAW_PARTS ? MMS_CT_RAW_PARTS : nb);
        k[(size_t)v] = VolK{(unsigned long long)d.offset, d.D, d.H, d.W, d.dtype, d.swap != 0, d.out_row, (int)nb, d.slope == 0.f ? 1.f : d.slope};
    }
    std::sort(rows.begin(), rows.end());
    if (std::adjacent_find(rows.begin(), rows.end()) != rows.end()) return MMS_ERR_ARG;
    const long long nout = no * p->oW;
    int ob = (int)((nout + 255) / 256);
    if (ob > 256) ob = 256;
    for (int v0 = 0; v0 < p->V; v0 += MMS_CT_RAW_CHUNK) {
        const int nv = p->V - v0 < MMS_CT_RAW_CHUNK ? p->V - v0 : MMS_CT_RAW_CHUNK;
        ChunkK c;
        memset(&c, 0, sizeof(c));
        int maxnb = 1;
        for (int i = 0; i < nv; ++i) { c.v[i] = k[(size_t)(v0 + i)]; maxnb = c.v[i].nb > maxnb ? c.v[i].nb : maxnb; }
        if (p->passes != 2)
            MMS_LAUNCH(ct_raw_minmax_kernel, dim3(maxnb, nv), dim3(256), 0, s, (const unsigned char*)p->base, c, p->scratch);
        if (p->passes != 1)
            MMS_LAUNCH(ct_raw_resample_kernel, dim3(ob, nv), dim3(256), 0, s, (const unsigned char*)p->base, c, (const float*)p->scratch, p->out,
                       Dims3{p->oD, p->oH, p->oW});
    }
    return mms_check_launch();
}
