// Batch assembly with ELASTIC deformation for gfx950 (include/mmsurv.h: ElaRec, ElaP, mms_gather_elastic_group, mms_elastic_field): the
// gather of gather_affine.hip with, per CT volume row, a free-form displacement d(p) added to the destination voxel before the affine
// source-coordinate map.  d is the cubic B-spline interpolant of a coarse lattice of control displacements that are a pure function of
// (seed, lattice index): the workgroup writes its row's lattice into LDS straight from the counter hash, no field ever lives in HBM, a
// row carries a 16-byte record -- and the work stays inside the one launch that copies the batch.
//
// LDS per workgroup: the 32 KB staging box of the affine kernel plus ELA_LATTICE_MAX floats (24 KB) of lattice = 56 KB: two such
// workgroups per CU (160 KB), 48 KB left over; the launch is <= 64 x B x ng workgroups on 256 CUs, so what it occupies of a CU is one
// workgroup's 56 KB in practice, the rest stays with the kernels of the step's other streams.  (24 KB, not 16: an 8 x 24 x 32 volume
// at spacing 2 takes 5985 floats; the flagship 64 x 64 x 32 volume takes 735 at spacing 16 and 2541 at spacing 8.)
//
// Evaluation order of d (what the test's bound is derived from; ela_disp4): the basis NUMERATORS N_i(r) = 6 B_i(r) are exact in fp32
// (r is a multiple of 2^-6: every term has at most 18 fractional bits below 8); the sum runs z first, then y, then x, each a product
// followed by three fmaf, and the result is multiplied ONCE by fp32(1 / 216).  A thread owns 4 consecutive x of one (z, y): they share
// the z- and y-reductions, which are done once per control column (4 columns, 5 when the spacing is 2).
//   staged form: the chain is still monotone in each of (z + d_z, y + d_y, x + d_x), and fp32 addition rounds monotonically, so the
//                tile's sources lie in the bounding box of the eight corners of the tile box WIDENED per axis by the row's clamped
//                amplitude times (1 + 2^-13) -- |d_a| <= amp_a (1 + 16 * 2^-24) by the order above; the slack is 500 times that.
//   direct form: as in gather_affine_kernel.  Rows whose clamped amplitudes are all 0 skip the lattice and run the affine arithmetic.
//   Default (AffP.stage_floats == 0): a row that DEFORMS takes the direct form, a row that does not the staged form of the affine
//   kernel.  Measured: the widened boxes stage each source voxel five times and more, and the direct form is 9 %
//   (device-resident cohort) and 13 % (pinned host, PCIe) faster; a positive stage_floats asks for the staged form of deforming rows too.
// Which form a tile takes and whether a row deforms depend on (tile, record, argument) only: uniform per workgroup around every barrier.
// No atomics, no in-launch waits.
#include "gather_affine.h"

#define ELA_LATTICE_MAX MMS_ELA_LATTICE_MAX // (include/mmsurv.h: 6144) floats of the LDS control lattice (3 components): 24 KB beside the 32 KB box

// One spacing and one amplitude bound per launch (the members of a group share the volume shape, hence the lattice): with the 256 bytes
// of hidden arguments the kernel's argument block stays under 4 KB next to Grp<GatherP> and AffGrp.
struct ElaK { float max_amp[3]; unsigned l; };                          // l: log2 spacing of D / H / W, 4 bits each
struct ElaGrp { const ElaRec* rec[MMS_MAX_GROUP]; ElaK k; unsigned direct; };  // direct: bit g = member g left stage_floats at 0
struct ElaGeo { int l[3]; int KH, KW, KK; };                            // KK = K_D * K_H * K_W control points per component

__host__ __device__ __forceinline__ long long ela_geometry(int D, int H, int W, const int* l, ElaGeo& g) {
    const int KD = ((D - 1) >> l[0]) + 4;
    g.l[0] = l[0]; g.l[1] = l[1]; g.l[2] = l[2];
    g.KH = ((H - 1) >> l[1]) + 4; g.KW = ((W - 1) >> l[2]) + 4;
    const long long kk = (long long)KD * g.KH * g.KW;
    g.KK = 3 * kk > ELA_LATTICE_MAX ? 0 : (int)kk;          // over the budget: no lattice (the launcher refuses it before any launch)
    return 3 * kk;
}

// the contract's clamp of a record's amplitude: NaN -> 0 (fmaxf returns its non-NaN operand), Inf / huge -> max_amp
__device__ __forceinline__ float ela_amp(float a, float mx) { return fminf(fmaxf(a, 0.f), mx); }

// The row's control lattice, straight from the hash: lat[a * KK + j] = amp_a * u(seed, 3 j + a), j = (jz K_H + jy) K_W + jx.  u is
// exact in fp32, the product rounds once.  (Planar in LDS: the 16 reads of a (z, y) reduction are then unit-stride in jx.)
__device__ __forceinline__ void ela_fill(float* lat, const ElaGeo& g, const float* amp, unsigned seed) {
    const uint32_t hs = hash_u32(seed ^ 0x85ebca6bU);
    for (int j = threadIdx.x; j < g.KK; j += 256) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const uint32_t h = hash_u32((uint32_t)(3 * j + a) * 0x9E3779B9U + hs);
            lat[a * g.KK + j] = amp[a] * ((float)((int)(h >> 8) - 8388608) * 0x1p-23f);
        }
    }
}

// 6 B_i(r), r = (p & (s - 1)) / s: exact in fp32 whatever the order, so contraction cannot change them
__device__ __forceinline__ void ela_basis6(int p, int l, float* N) {
    const float r = (float)(p & ((1 << l) - 1)) * (1.f / (float)(1 << l)), t = 1.f - r, r2 = r * r, r3 = r2 * r;
    N[0] = t * t * t;
    N[1] = 3.f * r3 - 6.f * r2 + 4.f;
    N[2] = -3.f * r3 + 3.f * r2 + 3.f * r + 1.f;
    N[3] = r3;
}

// THE definition of the field: displacement d[a][e] of the voxels (z, y, x + e), e = 0..3, x a multiple of 4, z < D, y < H, x < W
// (x + e is clamped to W - 1: lanes past the line's end repeat its last voxel and are not stored).  Every lattice index is inside the
// lattice by construction (cell + 3 <= K - 1 along each axis); the column count follows the cells the four voxels really touch.
__device__ __forceinline__ void ela_disp4(const float* lat, const ElaGeo& g, int z, int y, int x, int W, float d[3][4]) {
    float Nz[4], Ny[4];
    ela_basis6(z, g.l[0], Nz);
    ela_basis6(y, g.l[1], Ny);
    const int kz = z >> g.l[0], ky = y >> g.l[1], kx0 = x >> g.l[2];
    const int ncol = 4 + ((min(x + 3, W - 1) >> g.l[2]) - kx0);         // 4, or 5: a spacing of 2 puts the four voxels into two cells
    const float* base = lat + (kz * g.KH + ky) * g.KW + kx0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        float Q[5];
#pragma unroll
        for (int m = 0; m < 5; ++m) {
            Q[m] = 0.f;
            if (m < ncol) {
                float P[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float* c = base + a * g.KK + j * g.KW + m;
                    const int sz = g.KH * g.KW;
                    P[j] = fmaf(Nz[3], c[3 * sz], fmaf(Nz[2], c[2 * sz], fmaf(Nz[1], c[sz], Nz[0] * c[0])));
                }
                Q[m] = fmaf(Ny[3], P[3], fmaf(Ny[2], P[2], fmaf(Ny[1], P[1], Ny[0] * P[0])));
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int xe = min(x + e, W - 1);
            float Nx[4];
            ela_basis6(xe, g.l[2], Nx);
            const bool up = (xe >> g.l[2]) != kx0;
            const float q0 = up ? Q[1] : Q[0], q1 = up ? Q[2] : Q[1], q2 = up ? Q[3] : Q[2], q3 = up ? Q[4] : Q[3];
            d[a][e] = fmaf(Nx[3], q3, fmaf(Nx[2], q2, fmaf(Nx[1], q1, Nx[0] * q0))) * 0x1.2f684cp-8f;      // fp32(1 / 216)
        }
    }
}

__global__ __launch_bounds__(256) void gather_elastic_kernel(const Grp<GatherP> grp, const AffGrp ag, const ElaGrp eg) {
    __shared__ float4 box4[AFF_STAGE_MAX / 4];
    __shared__ float lat[ELA_LATTICE_MAX];
    const GatherP& p = grp.p[blockIdx.z];
    const AffK& k = ag.k[blockIdx.z];
    const ElaK& ek = eg.k;
    const int b = blockIdx.y;
    if (b >= p.B) return;                                   // (uniform per workgroup)
    const long long row = p.idx[b];
    const AugRec r = k.rec[b];
    const AffRec f = k.aff[b];
    const ElaRec er = eg.rec[blockIdx.z][b];
    const float amp[3] = {ela_amp(er.amp[0], ek.max_amp[0]), ela_amp(er.amp[1], ek.max_amp[1]), ela_amp(er.amp[2], ek.max_amp[2])};
    const int lg[3] = {(int)(ek.l & 15u), (int)((ek.l >> 4) & 15u), (int)((ek.l >> 8) & 15u)};
    ElaGeo geo;
    if (ag.D > 0) ela_geometry(ag.D, ag.H, ag.W, lg, geo); else geo.KK = 0;
    const bool elastic = (amp[0] > 0.f || amp[1] > 0.f || amp[2] > 0.f) && geo.KK > 0;      // (the launcher refuses a lattice over the budget)
    const bool direct_default = elastic && ((eg.direct >> blockIdx.z) & 1u);            // (uniform per workgroup)
    const int t0 = blockIdx.x * 256 + threadIdx.x, stride = gridDim.x * 256;
    const bool ident = !elastic && r.scale == 1.f && r.offset == 0.f && f.sigma == 0.f &&
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
        if (elastic) {                                      // (at most one volume source per member: filled once)
            ela_fill(lat, geo, amp, er.seed);
            __syncthreads();
        }
        // widening of the tile box per axis: the clamped amplitude plus the rounding slack (see the head of the file)
        const float wid[3] = {elastic ? amp[0] * 0x1.0008p0f : 0.f, elastic ? amp[1] * 0x1.0008p0f : 0.f, elastic ? amp[2] * 0x1.0008p0f : 0.f};
        const int nty = (H + AFT_Y - 1) / AFT_Y, ntx = (W + AFT_X - 1) / AFT_X;
        const int ntiles = ((D + AFT_Z - 1) / AFT_Z) * nty * ntx;
        static_assert(AFT_Z * AFT_Y * (AFT_X / 4) == 256 && AFT_X % 4 == 0, "one float4 of a tile per thread");
        const int lz = threadIdx.x / (AFT_Y * (AFT_X / 4)), ly = (threadIdx.x / (AFT_X / 4)) % AFT_Y, lx = (threadIdx.x % (AFT_X / 4)) * 4;
        for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
            const int tz = t / (nty * ntx), ty = (t / ntx) % nty, tx = t % ntx;
            const int z0 = tz * AFT_Z, y0 = ty * AFT_Y, x0 = tx * AFT_X;
            const int z1 = min(z0 + AFT_Z, D) - 1, y1 = min(y0 + AFT_Y, H) - 1, x1 = min(x0 + AFT_X, W) - 1;
            int bz0 = 0, by0 = 0, bx0 = 0, nz = 0, ny = 0, nx = 0;
            bool staged = false;
            if (vec) {
                float lo[3] = {3.0e38f, 3.0e38f, 3.0e38f}, hi[3] = {-3.0e38f, -3.0e38f, -3.0e38f};
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    const float z = (c & 4) ? (float)z1 + wid[0] : (float)z0 - wid[0], y = (c & 2) ? (float)y1 + wid[1] : (float)y0 - wid[1],
                                x = (c & 1) ? (float)x1 + wid[2] : (float)x0 - wid[2];
                    const float cc[3] = {aff_coord(f.m, z, y, x, D), aff_coord(f.m + 4, z, y, x, H), aff_coord(f.m + 8, z, y, x, W)};
#pragma unroll
                    for (int a = 0; a < 3; ++a) { lo[a] = fminf(lo[a], cc[a]); hi[a] = fmaxf(hi[a], cc[a]); }
                }
                aff_box(lo, hi, bz0, by0, bx0, nz, ny, nx);
                staged = (long long)nz * ny * nx <= (long long)k.stage && !direct_default;
            }
            if (staged) {
                aff_stage_box(box4, src, D, H, W, bz0, by0, bx0, nz, ny, nx);
                __syncthreads();
            }
            const int z = z0 + lz, y = y0 + ly, x = x0 + lx;
            if (z <= z1 && y <= y1 && x <= x1) {
                const float* box = (const float*)box4;
                float d[3][4];
                if (elastic) ela_disp4(lat, geo, z, y, x, W, d);
                float o[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float zf = (float)z, yf = (float)y, xf = (float)(x + e);
                    if (elastic) { zf = zf + d[0][e]; yf = yf + d[1][e]; xf = xf + d[2][e]; }       // deform first, then the affine map
                    const float cz = aff_coord(f.m, zf, yf, xf, D), cy = aff_coord(f.m + 4, zf, yf, xf, H), cx = aff_coord(f.m + 8, zf, yf, xf, W);
                    float v;
                    if (staged)
                        v = aff_trilerp([&](int sz, int sy, int sx) { return aff_at_box(box, sz, sy, sx, bz0, by0, bx0, nz, ny, nx); }, cz, cy, cx);
                    else
                        v = aff_trilerp([&](int sz, int sy, int sx) { return aff_at_global(src, sz, sy, sx, D, H, W); }, cz, cy, cx);
                    v = fmaf(r.scale, v, r.offset);
                    if (noisy) v = fmaf(f.sigma, aff_noise(hseed, (uint32_t)((z * H + y) * W + x + e)), v);
                    o[e] = v;
                }
                float* dd = dst + ((size_t)z * H + y) * W + x;
                if (vec) *(float4*)dd = make_float4(o[0], o[1], o[2], o[3]);
                else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) if (x + e <= x1) dd[e] = o[e];
                }
            }
            if (staged) __syncthreads();                    // the box is rewritten by the next tile
        }
    }
}

// d of B rows through ela_fill / ela_disp4, the device functions gather_elastic_kernel calls: out [B][3][D][H][W]
__global__ __launch_bounds__(256) void elastic_field_kernel(const ElaRec* __restrict__ rec, const ElaK ek, int B, int D, int H, int W, float* __restrict__ out) {
    __shared__ float lat[ELA_LATTICE_MAX];
    const int b = blockIdx.y;
    if (b >= B) return;
    const ElaRec er = rec[b];
    const float amp[3] = {ela_amp(er.amp[0], ek.max_amp[0]), ela_amp(er.amp[1], ek.max_amp[1]), ela_amp(er.amp[2], ek.max_amp[2])};
    const int lg[3] = {(int)(ek.l & 15u), (int)((ek.l >> 4) & 15u), (int)((ek.l >> 8) & 15u)};
    ElaGeo geo;
    ela_geometry(D, H, W, lg, geo);
    if (geo.KK <= 0) return;
    ela_fill(lat, geo, amp, er.seed);
    __syncthreads();
    const int nty = (H + AFT_Y - 1) / AFT_Y, ntx = (W + AFT_X - 1) / AFT_X;
    const int ntiles = ((D + AFT_Z - 1) / AFT_Z) * nty * ntx;
    const int lz = threadIdx.x / (AFT_Y * (AFT_X / 4)), ly = (threadIdx.x / (AFT_X / 4)) % AFT_Y, lx = (threadIdx.x % (AFT_X / 4)) * 4;
    const size_t vol = (size_t)D * H * W;
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int z = (t / (nty * ntx)) * AFT_Z + lz, y = ((t / ntx) % nty) * AFT_Y + ly, x = (t % ntx) * AFT_X + lx;
        if (z >= D || y >= H || x >= W) continue;
        float d[3][4];
        ela_disp4(lat, geo, z, y, x, W, d);
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (x + e < W) out[((size_t)b * 3 + a) * vol + ((size_t)z * H + y) * W + x + e] = d[a][e];
    }
}

// ElaP checks shared by the two entry points -> the kernel's per-member block; false: MMS_ERR_ARG.  dims D == 0: no volume source.
static bool ela_args(const ElaP& e, int D, int H, int W, ElaK& k) {
    if (!e.rec) return false;
    for (int a = 0; a < 3; ++a) {
        if (e.log2_spacing[a] < 1 || e.log2_spacing[a] > 6) return false;
        if (!(e.max_amp[a] >= 0.f && e.max_amp[a] <= 64.f)) return false;          // (false for NaN too)
    }
    if (D > 0) {
        ElaGeo g;
        if (ela_geometry(D, H, W, e.log2_spacing, g) > ELA_LATTICE_MAX) return false;
    }
    for (int a = 0; a < 3; ++a) k.max_amp[a] = e.max_amp[a];
    k.l = (unsigned)e.log2_spacing[0] | (unsigned)e.log2_spacing[1] << 4 | (unsigned)e.log2_spacing[2] << 8;
    return true;
}

extern "C" int mms_gather_elastic_group(const GatherP* pp, const AugP* aa, const AffP* ff, const ElaP* ee, int ng, hipStream_t s) {
    Grp<GatherP> a;
    if (!grp_fill(a, pp, ng, 1) || !aa || !ff || !ee) return MMS_ERR_ARG;
    AugGrp ug = {};
    int blocks = 0;
    if (!gather_aug_args(pp, aa, ng, ug, blocks)) return MMS_ERR_ARG;
    AffGrp ag = {};
    ElaGrp eg = {};
    ag.D = ug.D; ag.H = ug.H; ag.W = ug.W;
    for (int g = 0; g < ng; ++g) {
        if (!ff[g].rec || ff[g].stage_floats < 0) return MMS_ERR_ARG;
        ag.k[g].rec = ug.k[g].rec; ag.k[g].meta = ug.k[g].meta; ag.k[g].aff = ff[g].rec;
        ag.k[g].stage = ff[g].stage_floats == 0 || ff[g].stage_floats > AFF_STAGE_MAX ? AFF_STAGE_MAX : ff[g].stage_floats;
        ElaK ek = {};
        if (!ela_args(ee[g], ag.D, ag.H, ag.W, ek)) return MMS_ERR_ARG;
        if (g == 0) eg.k = ek;
        else if (ek.l != eg.k.l || ek.max_amp[0] != eg.k.max_amp[0] || ek.max_amp[1] != eg.k.max_amp[1] || ek.max_amp[2] != eg.k.max_amp[2])
            return MMS_ERR_ARG;                             // one spacing and one bound per launch
        eg.rec[g] = ee[g].rec;
        if (ff[g].stage_floats == 0) eg.direct |= 1u << g;
    }
    MMS_LAUNCH(gather_elastic_kernel, dim3(blocks, pp->B, ng), dim3(256), 0, s, a, ag, eg);
    return mms_check_launch();
}

extern "C" int mms_elastic_field(const ElaP* p, int B, int D, int H, int W, float* out, hipStream_t s) {
    if (!p || !out || B <= 0 || B > 65535 || D <= 0 || H <= 0 || W <= 0 || (long long)D * H * W > 0x7fffffffLL) return MMS_ERR_ARG;
    ElaK k = {};
    if (!ela_args(*p, D, H, W, k)) return MMS_ERR_ARG;
    const int ntiles = ((D + AFT_Z - 1) / AFT_Z) * ((H + AFT_Y - 1) / AFT_Y) * ((W + AFT_X - 1) / AFT_X);
    MMS_LAUNCH(elastic_field_kernel, dim3(ntiles < 64 ? ntiles : 64, B, 1), dim3(256), 0, s, p->rec, k, B, D, H, W, out);
    return mms_check_launch();
}
