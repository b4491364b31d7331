// Resampling pieces of the two kernels that transform a CT volume row inside the batch gather (gather_affine.hip: gather_affine_kernel,
// gather_elastic.hip: gather_elastic_kernel; include/mmsurv.h: AffRec, AffP).
//   shared by both:      the destination tile, the LDS staging budget, AffK / AffGrp, aff_coord (the contract's coordinate chain),
//                        aff_noise (the counter-hash noise), aff_trilerp (the trilinear sample).
//   elastic kernel only: aff_box, aff_stage_box, aff_at_box, aff_at_global -- function forms of the box computation, the staging loop
//                        and the two corner fetchers that gather_affine_kernel keeps inline, unchanged (see the note there).
#pragma once
#include "common.h"
#include "gather_rows.h"

#define AFT_Z 4
#define AFT_Y 8
#define AFT_X 32
#define AFF_STAGE_MAX 8192                  // floats of the LDS staging box: 32 KB of the CU's 160 KB -- five such workgroups per CU, and 128 KB
                                            // left for the kernels of the step's other streams that share the CU

struct AffK { const AugRec* rec; const AffRec* aff; unsigned meta; int stage; };
struct AffGrp { AffK k[MMS_MAX_GROUP]; int D, H, W; };

// source coordinate of one axis (the contract's chain), clamped to [-2, n + 1]: nothing inside (-1, n) -- the only coordinates with a
// corner in the volume -- moves, NaN becomes -2 (fmaxf returns its non-NaN operand), and the int conversion cannot overflow
__device__ __forceinline__ float aff_coord(const float* m, float z, float y, float x, int n) {
    const float c = fmaf(m[0], z, fmaf(m[1], y, fmaf(m[2], x, m[3])));
    return fminf(fmaxf(c, -2.f), (float)n + 1.f);
}

// Irwin-Hall noise of the contract: the byte sum of two hashed words, centred and scaled to unit variance
__device__ __forceinline__ float aff_noise(uint32_t hseed, uint32_t i) {
    const uint32_t h0 = hash_u32((2u * i) * 0x9E3779B9U + hseed), h1 = hash_u32((2u * i + 1u) * 0x9E3779B9U + hseed);
    const uint32_t lo = (h0 & 0x00FF00FFu) + ((h0 >> 8) & 0x00FF00FFu) + (h1 & 0x00FF00FFu) + ((h1 >> 8) & 0x00FF00FFu);
    const int S = (int)((lo & 0xFFFFu) + (lo >> 16));
    return (float)(S - 1020) * 0x1.39897ep-8f;
}

// trilinear sample from a corner fetcher at(z, y, x): x first, then y, then z; a weight of exactly 0 returns the lower corner's bits
template <class F>
__device__ __forceinline__ float aff_trilerp(F at, float cz, float cy, float cx) {
    const float fz0 = floorf(cz), fy0 = floorf(cy), fx0 = floorf(cx);
    const int iz = (int)fz0, iy = (int)fy0, ix = (int)fx0;
    const float wz = cz - fz0, wy = cy - fy0, wx = cx - fx0;
    float q[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const float a = at(iz + (c >> 1), iy + (c & 1), ix), b = at(iz + (c >> 1), iy + (c & 1), ix + 1);
        q[c] = fmaf(wx, b - a, a);
    }
    const float r0 = fmaf(wy, q[1] - q[0], q[0]), r1 = fmaf(wy, q[3] - q[2], q[2]);
    return fmaf(wz, r1 - r0, r0);
}

// the source box of a tile from the extreme coordinates of its corners: cells of lo / hi plus the upper neighbour, the x-range rounded
// outwards to multiples of 4 floats (& ~3 rounds down, negatives included).  Coordinates are clamped: each extent <= dim + 5.
__device__ __forceinline__ void aff_box(const float* lo, const float* hi, int& bz0, int& by0, int& bx0, int& nz, int& ny, int& nx) {
    bz0 = (int)floorf(lo[0]); by0 = (int)floorf(lo[1]); bx0 = (int)floorf(lo[2]) & ~3;
    nz = (int)floorf(hi[0]) + 2 - bz0; ny = (int)floorf(hi[1]) + 2 - by0;
    nx = (((int)floorf(hi[2]) + 2 - bx0) + 3) & ~3;
}

// load the box into LDS with 16-byte loads, four in flight per thread; parts outside the volume are not read and hold 0 (air).
// The caller puts the barrier behind it.
__device__ __forceinline__ void aff_stage_box(float4* box4, const float* src, int D, int H, int W, int bz0, int by0, int bx0, int nz, int ny, int nx) {
    const int nx4 = nx >> 2, W4 = W >> 2, n4 = nz * ny * nx4;
    for (int j0 = 0; j0 < n4; j0 += 1024) {
        float4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {                               // four 16-B loads in flight per thread
            const int j = j0 + threadIdx.x + u * 256;
            v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (j < n4) {
                const int l = j / nx4, xq = (bx0 >> 2) + (j - l * nx4), sz = bz0 + l / ny, sy = by0 + l % ny;
                if (sz >= 0 && sz < D && sy >= 0 && sy < H && xq >= 0 && xq < W4)        // outside the volume: air, not read
                    v[u] = ((const float4*)src)[(size_t)(sz * H + sy) * W4 + xq];
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) { const int j = j0 + threadIdx.x + u * 256; if (j < n4) box4[j] = v[u]; }
    }
}

// the corner fetchers of aff_trilerp: from the staged box (indices checked against the box, never against memory: inside it by the
// monotone chain; the check costs three compares and keeps LDS reads in bounds whatever the record holds) or from global memory
__device__ __forceinline__ float aff_at_box(const float* box, int sz, int sy, int sx, int bz0, int by0, int bx0, int nz, int ny, int nx) {
    const int lz_ = sz - bz0, ly_ = sy - by0, lx_ = sx - bx0;
    return ((unsigned)lz_ < (unsigned)nz && (unsigned)ly_ < (unsigned)ny && (unsigned)lx_ < (unsigned)nx) ? box[(lz_ * ny + ly_) * nx + lx_] : 0.f;
}
__device__ __forceinline__ float aff_at_global(const float* src, int sz, int sy, int sx, int D, int H, int W) {
    return ((unsigned)sz < (unsigned)D && (unsigned)sy < (unsigned)H && (unsigned)sx < (unsigned)W) ? src[((size_t)sz * H + sy) * W + sx] : 0.f;
}
