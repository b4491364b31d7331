// Row-copy pieces shared by the augmenting batch-assembly kernels (heads.hip: gather_aug_kernel, gather_affine.hip:
// gather_affine_kernel): the 16-byte row copy / zero-fill of gather_rows_kernel, the mask columns, the per-source role bits and the
// argument checks of mms_gather_aug_group (include/mmsurv.h: GatherP, AugRec, AugP).
#pragma once
#include "common.h"

struct AugK { const AugRec* rec; unsigned meta; unsigned pad; };        // meta: 4 bits per source = role | (drop_bit + 1) << 2
struct AugGrp { AugK k[MMS_MAX_GROUP]; int D, H, W; };

// the copy of gather_rows_kernel for one row (zero: the row is absent or dropped -- zero-filled without being read)
__device__ __forceinline__ void gather_copy_row(const float* __restrict__ src, float* __restrict__ dst, int w, bool zero, int t0, int stride) {
    if ((w & 3) == 0 && (((uintptr_t)src | (uintptr_t)dst) & 15) == 0) {
        if (zero) { for (int i = t0; i < (w >> 2); i += stride) ((float4*)dst)[i] = make_float4(0.f, 0.f, 0.f, 0.f); }
        else {
            int i = t0;
            for (; i + 3 * stride < (w >> 2); i += 4 * stride) {        // four 16-B loads in flight per thread (host-resident rows: PCIe latency)
                const float4 a = ((const float4*)src)[i], b = ((const float4*)src)[i + stride], c = ((const float4*)src)[i + 2 * stride],
                             d = ((const float4*)src)[i + 3 * stride];
                ((float4*)dst)[i] = a; ((float4*)dst)[i + stride] = b; ((float4*)dst)[i + 2 * stride] = c; ((float4*)dst)[i + 3 * stride] = d;
            }
            for (; i < (w >> 2); i += stride) ((float4*)dst)[i] = ((const float4*)src)[i];
        }
    } else {
        for (int i = t0; i < w; i += stride) dst[i] = zero ? 0.f : src[i];
    }
}

// Source s of batch row b, everything but the transform of a volume row: a mask source gets its dropped columns cleared, an absent or
// dropped row is zero-filled, a plain source (or a volume row whose record is the identity: copy_volume) is copied.
// -> true: done; false: src / dst point at a present, not dropped MMS_AUG_VOLUME row that the caller still has to transform.
__device__ __forceinline__ bool gather_plain_source(const GatherP& p, unsigned meta, int drop, int s, long long row, int b, bool copy_volume,
                                                    int t0, int stride, const float*& src, float*& dst) {
    src = p.src[s] + (size_t)row * p.src_ld[s];
    dst = p.dst[s] + (size_t)b * p.dst_ld[s];
    const int w = p.width[s];
    const unsigned m = (meta >> (4 * s)) & 15u;
    const int role = (int)(m & 3u), dbit = (int)(m >> 2) - 1;
    if (role == MMS_AUG_MASK) {                             // column j of a mask destination: 0 when modality j is dropped
        for (int i = t0; i < w; i += stride) dst[i] = ((drop >> i) & 1) ? 0.f : src[i];
        return true;
    }
    const bool absent = p.present[s] && p.present[s][(size_t)row * p.present_ld[s]] == 0.f;     // all-zero row by contract: not read
    const bool zero = absent || (dbit >= 0 && ((drop >> dbit) & 1));
    if (role != MMS_AUG_VOLUME || zero || copy_volume) { gather_copy_row(src, dst, w, zero, t0, stride); return true; }
    return false;
}

// Argument checks of mms_gather_aug_group -> the kernel's per-member block, the widest source and the launch's `blocks`; false: MMS_ERR_ARG.
static inline bool gather_aug_args(const GatherP* pp, const AugP* aa, int ng, AugGrp& ag, int& blocks) {
    int wmax = 0;
    for (int g = 0; g < ng; ++g) {
        const GatherP& q = pp[g];
        const AugP& u = aa[g];
        if (q.B != pp->B || q.B <= 0 || !q.idx || q.nsrc < 1 || q.nsrc > 8 || !u.rec) return false;
        int nvol = 0;
        unsigned meta = 0;
        for (int i = 0; i < q.nsrc; ++i) {
            if (!q.src[i] || !q.dst[i] || q.width[i] <= 0) return false;
            if (u.role[i] < MMS_AUG_PLAIN || u.role[i] > MMS_AUG_MASK || u.drop_bit[i] < -1 || u.drop_bit[i] > 2) return false;
            if (u.role[i] == MMS_AUG_MASK && q.width[i] > 3) return false;
            if (u.role[i] == MMS_AUG_VOLUME) {
                if (++nvol > 1 || u.D <= 0 || u.H <= 0 || u.W <= 0 || (long long)u.D * u.H * u.W != (long long)q.width[i]) return false;
                if (u.max_shift[0] < 0 || u.max_shift[0] >= u.D || u.max_shift[1] < 0 || u.max_shift[1] >= u.H || u.max_shift[2] < 0 ||
                    u.max_shift[2] >= u.W)
                    return false;
                if (ag.D && (ag.D != u.D || ag.H != u.H || ag.W != u.W)) return false;      // one volume shape per group
                ag.D = u.D; ag.H = u.H; ag.W = u.W;
            }
            meta |= ((unsigned)u.role[i] | (unsigned)(u.drop_bit[i] + 1) << 2) << (4 * i);
            if (q.width[i] > wmax) wmax = q.width[i];
        }
        ag.k[g].rec = u.rec; ag.k[g].meta = meta; ag.k[g].pad = 0;
    }
    blocks = (wmax / 4 + 1023) / 1024;           // ~4 float4 per thread on the widest source (one LDS tile of a volume per workgroup)
    if (blocks < 1) blocks = 1;
    if (blocks > 64) blocks = 64;
    return true;
}
