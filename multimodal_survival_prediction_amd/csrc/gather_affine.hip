// Batch assembly with resampling augmentation for gfx950 (include/mmsurv.h: AffRec, AffP, mms_gather_affine_group): the gather of
// heads.hip with, per CT volume row, an affine source-coordinate map sampled trilinearly (zero padding) and additive counter-hash
// noise -- inside the one launch that copies the batch, no second pass over the volume.
//
// A workgroup walks destination tiles of AFT_Z x AFT_Y x AFT_X voxels (whole 32-voxel W-line segments; a thread owns 4 consecutive x).
//   staged form: the coordinate chain is monotone in each of z, y, x (every fmaf rounds monotonically), so the tile's source
//                coordinates lie inside the bounding box of its eight transformed corners.  The box (x-range rounded outwards to
//                multiples of 4 floats) is loaded into LDS with 16-byte loads, four in flight per thread -- a pinned-host cohort is
//                read over PCIe in 16-byte pieces, each source voxel once per tile -- parts outside the volume are not read and hold
//                0.  Interpolation reads LDS (indices checked against the box, never against memory), destination lines leave as
//                16-byte stores.
//   direct form: the box exceeds AffP.stage_floats, or W % 4 / the row alignment rules the 16-byte path out: eight bounds-checked
//                global loads per voxel.  Merely correct.
// Which form a tile takes depends on (tile, record, argument) only: uniform per workgroup, as every branch around a barrier here.
// No atomics, no in-launch waits.
#include "gather_affine.h"       // tile, staging budget, aff_coord / aff_noise / aff_trilerp: shared with gather_elastic.hip

// The kernel's body is kept as it was written: its box computation, staging loop and corner fetchers below are the ORIGINALS of
// aff_box / aff_stage_box / aff_at_box / aff_at_global in gather_affine.h, which only gather_elastic_kernel calls.  Calling those
// helpers from here compiles to a differently scheduled kernel (compare order, branch sense), and this kernel's instructions are
// what the measurements of DESIGN.md section 5 were taken on; a fix to the staging has to be made in both places.

__global__ __launch_bounds__(256) void gather_affine_kernel(const Grp<GatherP> grp, const AffGrp ag) {
    __shared__ float4 box4[AFF_STAGE_MAX / 4];
    const GatherP& p = grp.p[blockIdx.z];
    const AffK& k = ag.k[blockIdx.z];
    const int b = blockIdx.y;
    if (b >= p.B) return;                                   // (uniform per workgroup)
    const long long row = p.idx[b];
    const AugRec r = k.rec[b];
    const AffRec f = k.aff[b];
    const int t0 = blockIdx.x * 256 + threadIdx.x, stride = gridDim.x * 256;
    const bool ident = r.scale == 1.f && r.offset == 0.f && f.sigma == 0.f &&
                       f.m[0] == 1.f && f.m[1] == 0.f && f.m[2] == 0.f && f.m[3] == 0.f &&
                       f.m[4] == 0.f && f.m[5] == 1.f && f.m[6] == 0.f && f.m[7] == 0.f &&
                       f.m[8] == 0.f && f.m[9] == 0.f && f.m[10] == 1.f && f.m[11] == 0.f;
    for (int s = 0; s < p.nsrc; ++s) {
        const float* src;
        float* dst;
        if (gather_plain_source(p, k.meta, r.drop, s, row, b, ident, t0, stride, src, dst)) continue;
        const int D = ag.D, H = ag.H, W = ag.W;
        const bool vec = (W & 3) == 0 && (((uintptr_t)src | (uintptr_t)dst) & 15) == 0;
        const bool noisy = f.sigma != 0.f;
        const uint32_t hseed = hash_u32(f.seed);
        const int nty = (H + AFT_Y - 1) / AFT_Y, ntx = (W + AFT_X - 1) / AFT_X;
        const int ntiles = ((D + AFT_Z - 1) / AFT_Z) * nty * ntx;
        static_assert(AFT_Z * AFT_Y * (AFT_X / 4) == 256 && AFT_X % 4 == 0, "one float4 of a tile per thread");
        const int lz = threadIdx.x / (AFT_Y * (AFT_X / 4)), ly = (threadIdx.x / (AFT_X / 4)) % AFT_Y, lx = (threadIdx.x % (AFT_X / 4)) * 4;
        for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
            const int tz = t / (nty * ntx), ty = (t / ntx) % nty, tx = t % ntx;
            const int z0 = tz * AFT_Z, y0 = ty * AFT_Y, x0 = tx * AFT_X;
            const int z1 = min(z0 + AFT_Z, D) - 1, y1 = min(y0 + AFT_Y, H) - 1, x1 = min(x0 + AFT_X, W) - 1;
            // the tile's source box: cells of the extreme corner coordinates, plus the upper neighbour
            int bz0 = 0, by0 = 0, bx0 = 0, nz = 0, ny = 0, nx = 0;
            bool staged = false;
            if (vec) {
                float lo[3] = {3.0e38f, 3.0e38f, 3.0e38f}, hi[3] = {-3.0e38f, -3.0e38f, -3.0e38f};
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    const float z = (float)((c & 4) ? z1 : z0), y = (float)((c & 2) ? y1 : y0), x = (float)((c & 1) ? x1 : x0);
                    const float cc[3] = {aff_coord(f.m, z, y, x, D), aff_coord(f.m + 4, z, y, x, H), aff_coord(f.m + 8, z, y, x, W)};
#pragma unroll
                    for (int a = 0; a < 3; ++a) { lo[a] = fminf(lo[a], cc[a]); hi[a] = fmaxf(hi[a], cc[a]); }
                }
                bz0 = (int)floorf(lo[0]); by0 = (int)floorf(lo[1]); bx0 = (int)floorf(lo[2]) & ~3;      // (& ~3 rounds down, negatives included)
                nz = (int)floorf(hi[0]) + 2 - bz0; ny = (int)floorf(hi[1]) + 2 - by0;
                nx = (((int)floorf(hi[2]) + 2 - bx0) + 3) & ~3;
                staged = (long long)nz * ny * nx <= (long long)k.stage;         // coordinates are clamped: each extent <= dim + 5
            }
            if (staged) {
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
                __syncthreads();
            }
            const int z = z0 + lz, y = y0 + ly, x = x0 + lx;
            if (z <= z1 && y <= y1 && x <= x1) {
                const float* box = (const float*)box4;
                float o[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float zf = (float)z, yf = (float)y, xf = (float)(x + e);
                    const float cz = aff_coord(f.m, zf, yf, xf, D), cy = aff_coord(f.m + 4, zf, yf, xf, H), cx = aff_coord(f.m + 8, zf, yf, xf, W);
                    float v;
                    if (staged) {
                        // (x + e > x1 only in the scalar form; a lane past the line's end cannot be here: vec means W % 4 == 0)
                        v = aff_trilerp([&](int sz, int sy, int sx) {
                            const int lz_ = sz - bz0, ly_ = sy - by0, lx_ = sx - bx0;
                            // inside the box by the monotone chain; the check costs three compares and keeps LDS reads in bounds whatever m holds
                            return ((unsigned)lz_ < (unsigned)nz && (unsigned)ly_ < (unsigned)ny && (unsigned)lx_ < (unsigned)nx)
                                       ? box[(lz_ * ny + ly_) * nx + lx_] : 0.f;
                        }, cz, cy, cx);
                    } else {
                        v = aff_trilerp([&](int sz, int sy, int sx) {
                            return ((unsigned)sz < (unsigned)D && (unsigned)sy < (unsigned)H && (unsigned)sx < (unsigned)W)
                                       ? src[((size_t)sz * H + sy) * W + sx] : 0.f;
                        }, cz, cy, cx);
                    }
                    v = fmaf(r.scale, v, r.offset);
                    if (noisy) v = fmaf(f.sigma, aff_noise(hseed, (uint32_t)((z * H + y) * W + x + e)), v);
                    o[e] = v;
                }
                float* d = dst + ((size_t)z * H + y) * W + x;
                if (vec) *(float4*)d = make_float4(o[0], o[1], o[2], o[3]);
                else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) if (x + e <= x1) d[e] = o[e];
                }
            }
            if (staged) __syncthreads();                    // the box is rewritten by the next tile
        }
    }
}

extern "C" int mms_gather_affine_group(const GatherP* pp, const AugP* aa, const AffP* ff, int ng, hipStream_t s) {
    Grp<GatherP> a;
    if (!grp_fill(a, pp, ng, 1) || !aa || !ff) return MMS_ERR_ARG;
    AugGrp ug = {};
    int blocks = 0;
    if (!gather_aug_args(pp, aa, ng, ug, blocks)) return MMS_ERR_ARG;
    AffGrp ag = {};
    ag.D = ug.D; ag.H = ug.H; ag.W = ug.W;
    for (int g = 0; g < ng; ++g) {
        if (!ff[g].rec || ff[g].stage_floats < 0) return MMS_ERR_ARG;
        ag.k[g].rec = ug.k[g].rec; ag.k[g].meta = ug.k[g].meta; ag.k[g].aff = ff[g].rec;
        ag.k[g].stage = ff[g].stage_floats == 0 || ff[g].stage_floats > AFF_STAGE_MAX ? AFF_STAGE_MAX : ff[g].stage_floats;
    }
    MMS_LAUNCH(gather_affine_kernel, dim3(blocks, pp->B, ng), dim3(256), 0, s, a, ag);
    return mms_check_launch();
}
