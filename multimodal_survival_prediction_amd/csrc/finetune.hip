// Fine-tuning optimiser step: clip_grad_norm_ + Adam / AdamW over SEGMENTS of the flat buffer (TuneP, include/mmsurv.h).
// Segment s = elements [bounds[s], bounds[s + 1]) with its own learning-rate and weight-decay multipliers and an L2-SP pull towards the
// anchor; lr_mult = 0 freezes it: its p / g / m / v are neither read nor written and its gradient stays out of the norm.
//
// Both flat kernels walk a VIRTUAL index over the aligned 16-byte quads that hold trainable elements (the update: outside the packed conv2
// tensors, which have a kernel of their own; the norm: all of them), so a frozen encoder costs no memory traffic.  Segment s covers the real quads floor(b[s] / 4) .. ceil(b[s + 1] / 4) - 1 minus the W2N / 4
// quads of every packed tensor inside it (no bound lies inside one, and their offsets are quad-aligned).  qt[] = exclusive prefix sum of
// those counts over the trainable segments; quad j of the walk belongs to the last segment with qt[s] <= j, and its real quad is found
// like clip_adam_kernel finds its element: a binary search over the packed tensors of that segment.  Parameter offsets are not 4-aligned
// (a bias of one float), so a quad at a segment edge is visited once by each segment that owns a part of it, and each visit touches its
// own elements only, one float at a time; a whole quad is one 16-byte access.
#include "common.h"
#include <math.h>
#include <vector>

constexpr int W2N = 32 * 27 * 128;       // floats per conv2 tensor (heads.hip)
constexpr int W2Q = W2N / 4;
constexpr int W2P = 132;                 // LDS pitch of the 32 x 128 tile (heads.hip)
constexpr int NSEG = MMS_TUNE_MAX_SEG;

// The segment table in LDS: 4104 + 2052 + 256 + 516 bytes; the update kernel adds 8 KB of per-segment constants (15.2 KB in all).
struct SegTab {
    long long b[NSEG + 1];               // bounds
    unsigned qt[NSEG + 1];               // qt[s] = trainable quads before segment s; qt[nseg] = all of them
    unsigned vq[64];                     // packed tensor k at quad w2_off[k] / 4 = vq[k] + k * W2Q
    unsigned char k0[NSEG + 4];          // k0[s] = packed tensors before bounds[s]
};

template <int T>
__device__ __forceinline__ void seg_build(const TuneP& p, SegTab& t, int nw) {      // nw: packed tensors to leave out of the walk
    const int tid = threadIdx.x, ns = p.nseg;
    for (int i = tid; i <= ns; i += T) t.b[i] = p.bounds[i];
    for (int i = tid; i < nw; i += T) t.vq[i] = (unsigned)(p.a.w2_off[i] >> 2) - (unsigned)i * W2Q;
    __syncthreads();
    for (int s = tid; s <= ns; s += T) {
        const long long bs = t.b[s];
        int lo = 0, hi = nw;             // #{k : w2_off[k] < bounds[s]}
        while (lo < hi) { const int mid = (lo + hi) >> 1; if ((((long long)t.vq[mid] + (long long)mid * W2Q) << 2) < bs) lo = mid + 1; else hi = mid; }
        t.k0[s] = (unsigned char)lo;
    }
    __syncthreads();
    for (int s = tid; s <= ns; s += T) {
        unsigned c = 0;
        if (s > 0 && p.lr_mult[s - 1] > 0.f)
            c = (unsigned)(((t.b[s] + 3) >> 2) - (t.b[s - 1] >> 2)) - (unsigned)(t.k0[s] - t.k0[s - 1]) * W2Q;
        t.qt[s] = c;                     // count of segment s - 1: the inclusive scan below leaves the exclusive prefix sums
    }
    __syncthreads();
    for (int d = 1; d <= ns; d <<= 1) {
        unsigned add[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) { const int i = tid + c * T; add[c] = (i <= ns && i >= d) ? t.qt[i - d] : 0u; }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < 3; ++c) { const int i = tid + c * T; if (i <= ns) t.qt[i] += add[c]; }
        __syncthreads();
    }
}

// quad j of the walk (j < qt[nseg]) -> its segment and the real elements [lo, hi) of that segment in it (hi - lo = 4: a whole aligned quad).
// false: the range does not lie inside [0, n) -- tables that mms_tune_check would have refused (a caller that skipped it); the quad is
// then left alone instead of addressed.
__device__ __forceinline__ bool seg_locate(const SegTab& t, int ns, long long n, unsigned j, int& s, long long& lo, long long& hi) {
    int l = 0, h = ns;                   // #{s < nseg : qt[s] <= j}
    while (l < h) { const int mid = (l + h) >> 1; if (t.qt[mid] <= j) l = mid + 1; else h = mid; }
    s = l - 1;
    const long long q0 = t.b[s] >> 2, r = j - t.qt[s];
    const int ka = t.k0[s], kb = t.k0[s + 1];
    const long long key = r + q0 - (long long)ka * W2Q;
    l = ka; h = kb;                      // packed tensors of the segment at or before the quad
    while (l < h) { const int mid = (l + h) >> 1; if ((long long)t.vq[mid] <= key) l = mid + 1; else h = mid; }
    const long long q = (q0 + r + (long long)(l - ka) * W2Q) << 2;
    lo = q > t.b[s] ? q : t.b[s];
    hi = q + 4 < t.b[s + 1] ? q + 4 : t.b[s + 1];
    return lo >= 0 && lo < hi && hi <= n && hi - lo <= 4;
}

__device__ __forceinline__ float4 seg_load(const float* x, long long lo, long long hi) {
    if (hi - lo == 4) return *(const float4*)(x + lo);
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
    r.x = x[lo];
    if (lo + 1 < hi) r.y = x[lo + 1];
    if (lo + 2 < hi) r.z = x[lo + 2];
    return r;
}
__device__ __forceinline__ void seg_store(float* x, long long lo, long long hi, const float4& r) {
    if (hi - lo == 4) { *(float4*)(x + lo) = r; return; }
    x[lo] = r.x;
    if (lo + 1 < hi) x[lo + 1] = r.y;
    if (lo + 2 < hi) x[lo + 2] = r.z;
}

// ---- sum of squares of the trainable gradients; the bookkeeping of grad_sumsq_kernel (heads.hip) ------------------------------------
template <int T>
__global__ __launch_bounds__(T) void grad_sumsq_tuned_kernel(const Grp<TuneP> grp) {
    const TuneP& p = grp.p[blockIdx.z];
    __shared__ SegTab t;
    __shared__ double red[T / 64];
    seg_build<T>(p, t, 0);                // (the norm reads the packed conv2 tensors like any other: nothing is left out)
    const int ns = p.nseg;
    const long long nq = t.qt[ns], stride = (long long)gridDim.x * T;
    long long i = (long long)blockIdx.x * T + threadIdx.x;
    if (blockIdx.x != 0 && (long long)blockIdx.x * T >= nq) return;       // (the grid is sized from n: the host does not read the table)
    float a = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    auto ld = [&](long long j) {
        int s; long long lo, hi;
        return seg_locate(t, ns, p.a.n, (unsigned)j, s, lo, hi) ? seg_load(p.a.g, lo, hi) : make_float4(0.f, 0.f, 0.f, 0.f);
    };
    for (; i + 3 * stride < nq; i += 4 * stride) {          // 4 independent 16-B loads in flight per thread
        const float4 g0 = ld(i), g1 = ld(i + stride), g2 = ld(i + 2 * stride), g3 = ld(i + 3 * stride);
        a = fmaf(g0.x, g0.x, a); a = fmaf(g0.y, g0.y, a); a = fmaf(g0.z, g0.z, a); a = fmaf(g0.w, g0.w, a);
        a1 = fmaf(g1.x, g1.x, a1); a1 = fmaf(g1.y, g1.y, a1); a1 = fmaf(g1.z, g1.z, a1); a1 = fmaf(g1.w, g1.w, a1);
        a2 = fmaf(g2.x, g2.x, a2); a2 = fmaf(g2.y, g2.y, a2); a2 = fmaf(g2.z, g2.z, a2); a2 = fmaf(g2.w, g2.w, a2);
        a3 = fmaf(g3.x, g3.x, a3); a3 = fmaf(g3.y, g3.y, a3); a3 = fmaf(g3.z, g3.z, a3); a3 = fmaf(g3.w, g3.w, a3);
    }
    for (; i < nq; i += stride) {
        const float4 g = ld(i);
        a = fmaf(g.x, g.x, a); a = fmaf(g.y, g.y, a); a = fmaf(g.z, g.z, a); a = fmaf(g.w, g.w, a);
    }
    a += a1 + a2 + a3;
    const double sum = block_sum_d((double)a, red);
    if (threadIdx.x == 0) {
        atomicAdd(p.a.sumsq, sum);
        if (blockIdx.x == 0) {
            if (p.a.skip_flag == nullptr || *p.a.skip_flag != 0.f) p.a.step[0] += 1.f;
            if (p.a.acc) {
                if (p.a.cox_out) { p.a.acc[0] += p.a.cox_out[0] * p.a.cox_out[1]; p.a.acc[1] += p.a.cox_out[1]; }
                if (p.a.entropy) p.a.acc[2] += p.a.entropy[0];
                p.a.acc[3] += 1.f;
            }
            if (p.a.rng) p.a.rng[1] += 1;
        }
    }
}

// ---- the update --------------------------------------------------------------------------------------------------------------------
// The step's constants in fp64, as clip_adam_kernel computes them: cd = {coef, bias correction 1, 1 / sqrt(bias correction 2)}.
__device__ __forceinline__ void tune_step_consts(const AdamP& p, double* cd) {
    const double lr = p.hyper[0], b1 = p.hyper[1], b2 = p.hyper[2], maxn = p.hyper[5];
    const double t = p.step[0];
    const double norm = sqrt(*p.sumsq);
    double coef = maxn / (norm + 1e-6);
    if (coef > 1.0) coef = 1.0;
    if (maxn <= 0.0) coef = 1.0;
    const double bc1 = 1.0 - pow(b1, t), bc2 = 1.0 - pow(b2, t);
    cd[0] = coef; cd[1] = bc1; cd[2] = 1.0 / sqrt(bc2);
}
// Segment constants {step size, AdamW decay factor, weight decay, L2-SP factor}: lr_s = lr * lr_mult, wd_s = wd * wd_mult; the L2-SP
// factor is lambda for Adam (added to the gradient) and lr_s * lambda for AdamW (taken off the weight).  Multipliers of 1 give the
// floats of clip_adam_kernel.
__device__ __forceinline__ float4 tune_seg_consts(const AdamP& p, double bc1, float lm, float wm, float l2) {
    const double lr = (double)p.hyper[0] * (double)lm, wd = (double)p.hyper[4] * (double)wm;
    return make_float4((float)(lr / bc1), (float)(1.0 - lr * wd), (float)wd, p.adamw ? (float)(lr * (double)l2) : l2);
}
// One element, written with the expressions of clip_adam_kernel (a trivial plan gives its bits).  FMA_DEN: how the denominator
// sqrt(v) / sqrt(bc2) + eps is rounded.  hipcc compiles heads.hip's flat kernel with the product and the sum as two roundings (it pairs the
// product with step_size * m in one packed multiply before it looks for contractions) and its packed-tensor kernel with one fused
// multiply-add; left to the compiler, this file's flat kernel took the fused form and 0.3 % of the weights came out one ulp of the update
// away from mms_clip_adam's.  So both are spelled out here: tests/test_gpu_finetune.py compares the bits of both kernels.
template <bool FMA_DEN>
struct TuneUpd {
    float coef, inv_sqrt_bc2, b1, b2, eps; int adamw;
    __device__ __forceinline__ void operator()(const float4& k, float& w, float g, float& m, float& v, float w0) const {
        const float step_size = k.x, decay = k.y, wd = k.z, l2 = k.w;
        g *= coef;
        if (adamw) {
            const float wo = w;
            w *= decay;
            if (l2 != 0.f) w = fmaf(-l2, wo - w0, w);
        } else {
            g = fmaf(wd, w, g);
            if (l2 != 0.f) g = fmaf(l2, w - w0, g);
        }
        m = fmaf(b1, m, (1.f - b1) * g);
        v = fmaf(b2, v, (1.f - b2) * g * g);
        float den;
        if (FMA_DEN) den = fmaf(sqrtf(v), inv_sqrt_bc2, eps);
        else {
#pragma clang fp contract(off)
            const float scaled = sqrtf(v) * inv_sqrt_bc2;
            den = scaled + eps;
        }
        w = w - step_size * m / den;
    }
};

__global__ __launch_bounds__(256) void clip_adam_tuned_kernel(const Grp<TuneP> grp) {
    const TuneP& p = grp.p[blockIdx.z];
    __shared__ SegTab t;
    __shared__ float4 kseg[NSEG];
    __shared__ double cd[3];
    if (p.a.skip_flag != nullptr && *p.a.skip_flag == 0.f) return;
    if (threadIdx.x == 0) tune_step_consts(p.a, cd);
    seg_build<256>(p, t, p.a.n_w2);      // (its barriers publish cd)
    const int ns = p.nseg;
    for (int s = threadIdx.x; s < ns; s += 256) kseg[s] = tune_seg_consts(p.a, cd[1], p.lr_mult[s], p.wd_mult[s], p.l2sp[s]);
    __syncthreads();
    const TuneUpd<false> upd{(float)cd[0], (float)cd[2], p.a.hyper[1], p.a.hyper[2], p.a.hyper[3], p.a.adamw};
    const long long nq = t.qt[ns], stride = (long long)gridDim.x * 256;
    for (long long j = (long long)blockIdx.x * 256 + threadIdx.x; j < nq; j += stride) {
        int s; long long lo, hi;
        if (!seg_locate(t, ns, p.a.n, (unsigned)j, s, lo, hi)) continue;
        const float4 k = kseg[s];
        float4 w = seg_load(p.a.p, lo, hi), m = seg_load(p.a.m, lo, hi), v = seg_load(p.a.v, lo, hi);
        const float4 g = seg_load(p.a.g, lo, hi);
        float4 w0 = make_float4(0.f, 0.f, 0.f, 0.f);
        if (k.w != 0.f) w0 = seg_load(p.anchor, lo, hi);
        upd(k, w.x, g.x, m.x, v.x, w0.x); upd(k, w.y, g.y, m.y, v.y, w0.y);
        upd(k, w.z, g.z, m.z, v.z, w0.z); upd(k, w.w, g.w, m.w, v.w, w0.w);
        seg_store(p.a.m, lo, hi, m); seg_store(p.a.v, lo, hi, v); seg_store(p.a.p, lo, hi, w);
    }
}

// The tuned twin of w2_adam_pack_kernel<true> (heads.hip): one workgroup = (layer, tap).  The layer's settings are those of the segment
// that holds it; the workgroups of a frozen layer return before any load of the tensor -- its weights do not move, so its packs stay valid.
__global__ __launch_bounds__(256) void w2_adam_pack_tuned_kernel(const Grp<TuneP> grp) {
    const TuneP& p = grp.p[blockIdx.z];
    const int tap = blockIdx.x, layer = blockIdx.y, tid = threadIdx.x;
    __shared__ __attribute__((aligned(16))) float t[32 * W2P];
    __shared__ int seg;
    __shared__ double cd[3];
    if (p.a.skip_flag != nullptr && *p.a.skip_flag == 0.f) return;      // unusable batch: no update, the packs stay valid
    const size_t base = (size_t)p.a.w2_off[layer];
    if (base + W2N > (size_t)p.a.n) return;                              // (an offset mms_tune_check would have refused)
    if (tid == 0) seg = 0;
    __syncthreads();
    for (int s = tid; s < p.nseg; s += 256)                              // one round of loads: exactly one segment holds the tensor
        if (p.bounds[s] <= (long long)base && (long long)base < p.bounds[s + 1]) seg = s;
    __syncthreads();
    const int s = seg;
    const float lm = p.lr_mult[s];
    if (!(lm > 0.f)) return;
    if (tid == 0) tune_step_consts(p.a, cd);
    __syncthreads();
    const float4 k = tune_seg_consts(p.a, cd[1], lm, p.wd_mult[s], p.l2sp[s]);
    const TuneUpd<true> upd{(float)cd[0], (float)cd[2], p.a.hyper[1], p.a.hyper[2], p.a.hyper[3], p.a.adamw};
    // thread -> float4 j of the tile: co = idx4 >> 5, cin = 4 * (idx4 & 31); 32 consecutive threads cover one 512-byte run
    float4 w4[4];
    size_t off[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int idx4 = tid + 256 * j, co = idx4 >> 5, c4 = idx4 & 31;
        off[j] = base + ((size_t)co * 27 + tap) * 128 + 4 * c4;
        w4[j] = *(const float4*)(p.a.p + off[j]);
    }
    {
        float4 g4[4], m4[4], v4[4], a4[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            g4[j] = *(const float4*)(p.a.g + off[j]); m4[j] = *(const float4*)(p.a.m + off[j]); v4[j] = *(const float4*)(p.a.v + off[j]);
            a4[j] = k.w != 0.f ? *(const float4*)(p.anchor + off[j]) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            upd(k, w4[j].x, g4[j].x, m4[j].x, v4[j].x, a4[j].x); upd(k, w4[j].y, g4[j].y, m4[j].y, v4[j].y, a4[j].y);
            upd(k, w4[j].z, g4[j].z, m4[j].z, v4[j].z, a4[j].z); upd(k, w4[j].w, g4[j].w, m4[j].w, v4[j].w, a4[j].w);
            *(float4*)(p.a.p + off[j]) = w4[j]; *(float4*)(p.a.m + off[j]) = m4[j]; *(float4*)(p.a.v + off[j]) = v4[j];
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int idx4 = tid + 256 * j, co = idx4 >> 5, c4 = idx4 & 31;
        *(float4*)(t + co * W2P + 4 * c4) = w4[j];
    }
    __syncthreads();
    // the derived packs, in the orders w2_adam_pack_kernel writes (heads.hip has the index algebra)
    const bool frag = (p.a.w2_fragmask >> layer) & 1ull;
    float4* pb = (float4*)p.a.w2_pack_b[layer];
    if (frag) {
        float4* dst = pb + (size_t)tap * 1024;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int idx4 = tid + 256 * j, q = idx4 >> 6, lane = idx4 & 63;
            const int cin = ((q >> 1) << 4) | (lane & 15), co0 = ((q & 1) << 4) | ((lane >> 4) << 2);
            dst[idx4] = make_float4(t[co0 * W2P + cin], t[(co0 + 1) * W2P + cin], t[(co0 + 2) * W2P + cin], t[(co0 + 3) * W2P + cin]);
        }
        float4* df = (float4*)p.a.w2_pack_f[layer] + (size_t)tap * 1024;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int idx4 = tid + 256 * j, q = idx4 >> 6, lane = idx4 & 63;
            const int c4 = ((q >> 1) << 2) | (lane >> 4), co = ((q & 1) << 4) | (lane & 15);
            df[idx4] = *(const float4*)(t + co * W2P + 4 * c4);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int idx4 = tid + 256 * j, cin = idx4 >> 3, co0 = (idx4 & 7) << 2;
            pb[((size_t)cin * 27 + tap) * 8 + (idx4 & 7)] =
                make_float4(t[co0 * W2P + cin], t[(co0 + 1) * W2P + cin], t[(co0 + 2) * W2P + cin], t[(co0 + 3) * W2P + cin]);
        }
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
// What a launch can check without reading device memory; the tables' CONTENTS are checked once by mms_tune_check.
static bool tune_group(Grp<TuneP>& a, const TuneP* pp, int ng) {
    if (!grp_fill(a, pp, ng, 1) || pp->a.n <= 0 || pp->a.n >= (1ll << 33)) return false;
    for (int g = 0; g < ng; ++g) {
        const TuneP& q = pp[g];
        const AdamP& p = q.a;
        if (p.n != pp->a.n || p.n_w2 != pp->a.n_w2 || p.w2_fragmask != pp->a.w2_fragmask || p.n_w2 < 0 || p.n_w2 > 64) return false;
        if (!p.p || !p.g || !p.m || !p.v || !p.hyper || !p.sumsq || !p.step) return false;
        if (((uintptr_t)p.p | (uintptr_t)p.g | (uintptr_t)p.m | (uintptr_t)p.v | (uintptr_t)q.anchor) & 15) return false;
        if (p.n_w2 && (!p.w2_off || !p.w2_pack_b || (p.w2_fragmask && !p.w2_pack_f))) return false;
        if (q.nseg < 1 || q.nseg > MMS_TUNE_MAX_SEG || !q.bounds || !q.lr_mult || !q.wd_mult || !q.l2sp) return false;
        // one segment table for the whole group
        if (q.nseg != pp->nseg || q.bounds != pp->bounds || q.lr_mult != pp->lr_mult || q.wd_mult != pp->wd_mult || q.l2sp != pp->l2sp) return false;
    }
    return true;
}
extern "C" int mms_tune_check(const TuneP* p) {
    Grp<TuneP> a;
    if (!tune_group(a, p, 1)) return MMS_ERR_ARG;
    const int ns = p->nseg, nw = p->a.n_w2;
    std::vector<long long> b(ns + 1), w2(nw);
    std::vector<float> lm(ns), wm(ns), l2(ns);
    if (hipMemcpy(b.data(), p->bounds, sizeof(long long) * (ns + 1), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(lm.data(), p->lr_mult, sizeof(float) * ns, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(wm.data(), p->wd_mult, sizeof(float) * ns, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(l2.data(), p->l2sp, sizeof(float) * ns, hipMemcpyDeviceToHost) != hipSuccess ||
        (nw && hipMemcpy(w2.data(), p->a.w2_off, sizeof(long long) * nw, hipMemcpyDeviceToHost) != hipSuccess))
        return MMS_ERR_LAUNCH;
    if (b[0] != 0 || b[ns] != p->a.n) return MMS_ERR_ARG;
    bool any = false, pull = false;
    for (int s = 0; s < ns; ++s) {
        if (b[s + 1] <= b[s]) return MMS_ERR_ARG;
        if (!isfinite(lm[s]) || !isfinite(wm[s]) || !isfinite(l2[s]) || lm[s] < 0.f || wm[s] < 0.f || l2[s] < 0.f) return MMS_ERR_ARG;
        any |= lm[s] > 0.f;
        pull |= lm[s] > 0.f && l2[s] > 0.f;
    }
    if (!any || (pull && !p->anchor)) return MMS_ERR_ARG;
    for (int k = 0; k < nw; ++k) {
        if ((w2[k] & 3) || w2[k] < 0 || w2[k] + W2N > p->a.n || (k && w2[k] < w2[k - 1] + W2N)) return MMS_ERR_ARG;
        for (int s = 1; s < ns; ++s)
            if (b[s] > w2[k] && b[s] < w2[k] + W2N) return MMS_ERR_ARG;       // a bound inside a packed tensor
    }
    return MMS_OK;
}
extern "C" int mms_grad_sumsq_tuned_group(const TuneP* pp, int ng, hipStream_t s) {
    Grp<TuneP> a;
    if (!tune_group(a, pp, ng)) return MMS_ERR_ARG;
    long long blocks = (pp->a.n / 16 + 255) / 256;          // the grid of mms_grad_sumsq: workgroups past the trainable quads leave at once
    if (blocks > 1024) blocks = 1024;
    if (blocks < 1) blocks = 1;
    if ((blocks & 3) == 0) MMS_LAUNCH(grad_sumsq_tuned_kernel<1024>, dim3((unsigned)(blocks >> 2), 1, ng), dim3(1024), 0, s, a);
    else MMS_LAUNCH(grad_sumsq_tuned_kernel<256>, dim3((unsigned)blocks, 1, ng), dim3(256), 0, s, a);
    return mms_check_launch();
}
extern "C" int mms_clip_adam_tuned_group(const TuneP* pp, int ng, hipStream_t s) {
    Grp<TuneP> a;
    if (!tune_group(a, pp, ng)) return MMS_ERR_ARG;
    long long blocks = (pp->a.n / 4 + 255) / 256;           // one quad per thread and trip
    if (blocks > 4096) blocks = 4096;
    if (blocks < 1) blocks = 1;
    MMS_LAUNCH(clip_adam_tuned_kernel, dim3((unsigned)blocks, 1, ng), dim3(256), 0, s, a);
    if (pp->a.n_w2 > 0) MMS_LAUNCH(w2_adam_pack_tuned_kernel, dim3(27, pp->a.n_w2, ng), dim3(256), 0, s, a);
    return mms_check_launch();
}
MMS_SINGLE(mms_grad_sumsq_tuned, TuneP)
MMS_SINGLE(mms_clip_adam_tuned, TuneP)
