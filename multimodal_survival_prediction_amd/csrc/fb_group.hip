// Fold-group (lock-step) forms of the fallback CT encoder -- 3 x [Conv3d(k3,s2,p1)+BN3d+ReLU] + global average pool -- on the fp32 MFMA
// tile-GEMM core (tile_gemm.h).  Data contract: FbConvP / FbPoolP (include/mmsurv.h), exactly what the scalar kernels of fallback.hip
// implement: channels-last activations, torch-layout weights [Cout][Cin][27], raw conv output + bias stored with its fp64 batch statistics,
// the previous layer's BatchNorm+ReLU applied by the reader, zero padding of the ACTIVATED input, output grid ceil(in/2).
// Every kernel takes Grp<P>: one parameter block per member, member index from the grid.  Plain bounded loops only; LDS <= 64 KB per
// workgroup (no function attribute); nothing derived from the weights outlives a launch.
#include "common.h"
#include "tile_gemm.h"
#include "fb_plan.h"
#include <type_traits>

namespace {

__device__ __forceinline__ void fbg_tap(int tap, int& td, int& th, int& tw) { td = tap / 9; th = (tap - 9 * td) / 3; tw = tap - 9 * td - 3 * th; }

// BN+ReLU constants of the Cin (<= 128) input channels in LDS: mean | scale | shift at e, e + 128, e + 256
__device__ __forceinline__ void fbg_bn_lds(const FbConvP& p, int tid, float* e) {
    if (p.has_bn) { bn_consts_to_lds<1>(p.bn, p.Cin, tid, e, e + 128, e + 256); return; }
    if (tid < 128) { e[tid] = 0.f; e[128 + tid] = 1.f; e[256 + tid] = 0.f; }
}
__device__ __forceinline__ float4 fbg_act4(const float4 v, const float* e, int c, int has) {
    if (!has) return v;
    return make_float4(fmaxf(bn_apply(v.x, e[c], e[128 + c], e[256 + c]), 0.f), fmaxf(bn_apply(v.y, e[c + 1], e[129 + c], e[257 + c]), 0.f),
                       fmaxf(bn_apply(v.z, e[c + 2], e[130 + c], e[258 + c]), 0.f), fmaxf(bn_apply(v.w, e[c + 3], e[131 + c], e[259 + c]), 0.f));
}

// ------------------------------------------------------------------------------------------------------
// forward: stride-2 implicit GEMM.  rows = output voxels, cols = Cout, reduction k = tap * Cin + cin (tap-major: for Cin % 4 == 0 four
// consecutive k are four consecutive channels of one input voxel = one 16-byte load).  C1: Cin == 1, K = 27 padded to one 32-deep tile.
// ------------------------------------------------------------------------------------------------------
template <int WM_, int WN_, int WK_, bool C1>
struct FbFwdOp {
    typedef FbConvP Params;
    static constexpr int WM = WM_, WN = WN_, WK = WK_, AMODE = C1 ? LD_K1 : LD_K4, BMODE = LD_K1;
    static constexpr bool ONE_TILE = C1, SINGLE_BUF = WK_ == 4;       // 128-deep tiles: one LDS buffer (64 KB limit)
    static constexpr int TM = 32 * WM, TN = 32 * WN;
    static constexpr int EXTRA = 384 + 2 * TM;
    const float* bnc; const int* rows;
    int m0, K, Cin, D, H, W, has;
    __device__ void step(const Params&, int) {}
    __device__ void setup(const Params& p, int m0_, int, int, float* extra, int tid) {
        bnc = extra; rows = (const int*)(extra + 384); m0 = m0_;
        K = 27 * p.Cin; Cin = p.Cin; D = p.in.D; H = p.in.H; W = p.in.W; has = p.has_bn;
        fbg_bn_lds(p, tid, extra);
        if (tid < TM) {      // (2 od, 2 oh, 2 ow) and the sample of every row of the tile
            const int m = m0 + tid, vox = p.out.D * p.out.H * p.out.W;
            int pk = 0, b = -1;
            if (m < p.B * vox) {
                b = m / vox;
                const int r = m - b * vox, od = r / (p.out.H * p.out.W), oh = (r / p.out.W) % p.out.H, ow = r % p.out.W;
                pk = pack_dhw(2 * od, 2 * oh, 2 * ow);
            }
            ((int*)extra)[384 + 2 * tid] = pk; ((int*)extra)[385 + 2 * tid] = b;
        }
    }
    __device__ void krange(const Params&, int, int& kb, int& ke) { kb = 0; ke = K; }
    typedef typename std::conditional<C1, float, float4>::type ARaw;
    typedef float BRaw;
    // -> element offset of input voxel (row m, tap) in x, ok = inside the volume
    __device__ int src_of(int m, int tap, bool& ok) const {
        const int rr = m - m0, pk = rows[2 * rr], b = rows[2 * rr + 1];
        int td, th, tw, d, h, w;
        fbg_tap(tap, td, th, tw); unpack_dhw(pk, d, h, w);
        const int id = d - 1 + td, ih = h - 1 + th, iw = w - 1 + tw;
        ok = b >= 0 && (unsigned)id < (unsigned)D && (unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)W;
        return ok ? ((b * D + id) * H + ih) * W + iw : 0;
    }
    __device__ ARaw a_ld(const Params& p, int, int m, int k, bool& ok) const {
        if constexpr (C1) {
            const int src = src_of(m, k < 27 ? k : 0, ok);
            ok = ok && k < 27;
            return p.x[ok ? src : 0];
        } else {
            const int kk = k < K ? k : 0, tap = kk / Cin, cin = kk - tap * Cin;
            const int src = src_of(m, tap, ok);
            ok = ok && k < K;
            return *(const float4*)(p.x + (ok ? (size_t)src * Cin + cin : 0));
        }
    }
    __device__ ARaw a_tx(const Params&, int, const ARaw& v, int, int k, bool ok) const {
        if constexpr (C1) return ok ? v : 0.f;
        else {
            const int kk = k < K ? k : 0;
            const float4 r = fbg_act4(v, bnc, kk % Cin, has);
            return ok ? r : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    __device__ float b_ld(const Params& p, int, int n, int k, bool& ok) const {
        ok = n < p.Cout && k < K;
        const int kk = ok ? k : 0, tap = kk / Cin, cin = kk - tap * Cin;
        return p.w[ok ? ((size_t)n * Cin + cin) * 27 + tap : 0];
    }
    __device__ float b_tx(const Params&, int, const float& v, int, int, bool ok) const { return ok ? v : 0.f; }
    __device__ void epilogue(const Params& p, int m0_, int n0, int, const float* Cs, int tid, bool) {
        const int M = p.B * p.out.D * p.out.H * p.out.W;
        for (int idx = tid; idx < TM * TN; idx += 256) {
            const int r = idx / TN, c = idx % TN, m = m0_ + r, n = n0 + c;
            if (m < M && n < p.Cout) p.y[(size_t)m * p.Cout + n] = Cs[r * (TN + 1) + c] + p.bias[n];
        }
        if (p.osum == nullptr || tid >= TN || n0 + tid >= p.Cout) return;
        const float bias = p.bias[n0 + tid];
        const int nr = M - m0_ < TM ? M - m0_ : TM;
        double s = 0, q = 0;
        for (int r = 0; r < nr; ++r) { const float v = Cs[r * (TN + 1) + tid] + bias; s += v; q += (double)v * v; }
        atomicAdd(&p.osum[n0 + tid], s); atomicAdd(&p.osumsq[n0 + tid], q);
    }
};

// ------------------------------------------------------------------------------------------------------
// backward, weights: dW[co][cin][tap] = sum_m dy[m][co] * a(m, cin, tap): a GEMM whose reduction runs over the output rows m.
// C rows = co (A = dy, contiguous along co: R4), C cols j = tap * Cin + cin (B = activated input, contiguous along cin: R4; Cin == 1: K1).
// The rows are split over z = msplit workgroups; a workgroup's 64 x 64 partial is complete in LDS before its fp32 atomics.
// dbias = column sums of dy: the A loader threads of the j-tile 0 workgroups add up what they store (same pass, no extra read).
// ------------------------------------------------------------------------------------------------------
template <bool C1>
struct FbBwdWOp {
    typedef FbConvP Params;
    static constexpr int WM = 2, WN = 2, WK = 1, AMODE = LD_R4, BMODE = C1 ? LD_K1 : LD_R4;
    static constexpr int TM = 64, TN = 64, TK = 32;
    static constexpr int EXTRA = 384 + TM;
    static constexpr int NA = TM * TK / 4 / 256, NB = C1 ? TN * TK / 256 : TN * TK / 4 / 256;
    const float* bnc; float* bred;
    int K, Cin, D, H, W, has, Mout, vox, oH, oW, n0s;
    int jtap[NB], jcin[NB];        // piece i of the B tile always holds column j = n0 + row(i): (tap | -1, cin)
    float4 bsum[NA];
    __device__ void step(const Params&, int) {}
    __device__ void setup(const Params& p, int, int n0, int, float* extra, int tid) {
        bnc = extra; bred = extra + 384;
        K = 27 * p.Cin; Cin = p.Cin; D = p.in.D; H = p.in.H; W = p.in.W; has = p.has_bn;
        oH = p.out.H; oW = p.out.W; vox = p.out.D * oH * oW; Mout = p.B * vox; n0s = n0;
        fbg_bn_lds(p, tid, extra);
        if (tid < TM) extra[384 + tid] = 0.f;
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int idx = tid + i * 256, j = n0 + (C1 ? idx / TK : (idx % (TN / 4)) * 4);
            jtap[i] = j < K ? j / Cin : -1; jcin[i] = j < K ? j % Cin : 0;
        }
#pragma unroll
        for (int i = 0; i < NA; ++i) bsum[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __device__ void krange(const Params& p, int z, int& kb, int& ke) {
        const int per = (((Mout + TK - 1) / TK + p.msplit - 1) / p.msplit) * TK;      // whole K steps per workgroup
        kb = z * per; ke = kb + per < Mout ? kb + per : Mout;
        if (kb > ke) kb = ke;
    }
    typedef float4 ARaw;
    typedef typename std::conditional<C1, float, float4>::type BRaw;
    __device__ float4 a_ld(const Params& p, int, int co, int m, bool& ok) const {
        ok = co < p.Cout && m < Mout;
        return *(const float4*)(p.dy + (ok ? (size_t)m * p.Cout + co : 0));
    }
    __device__ float4 a_tx(const Params&, int i, const float4& v, int, int, bool ok) {
        const float4 r = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
        bsum[i].x += r.x; bsum[i].y += r.y; bsum[i].z += r.z; bsum[i].w += r.w;
        return r;
    }
    __device__ BRaw b_ld(const Params& p, int i, int, int m, bool& ok) const {
        const int mm = m < Mout ? m : 0, tap = jtap[i] < 0 ? 0 : jtap[i];
        const int b = mm / vox, r = mm - b * vox, od = r / (oH * oW), r2 = r - od * oH * oW, oh = r2 / oW, ow = r2 - oh * oW;
        int td, th, tw;
        fbg_tap(tap, td, th, tw);
        const int id = 2 * od - 1 + td, ih = 2 * oh - 1 + th, iw = 2 * ow - 1 + tw;
        ok = m < Mout && jtap[i] >= 0 && (unsigned)id < (unsigned)D && (unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)W;
        const size_t src = ok ? (size_t)(((b * D + id) * H + ih) * W + iw) * Cin + jcin[i] : 0;
        if constexpr (C1) return p.x[src]; else return *(const float4*)(p.x + src);
    }
    __device__ BRaw b_tx(const Params&, int i, const BRaw& v, int, int, bool ok) const {
        if constexpr (C1) return ok ? v : 0.f;
        else {
            const float4 r = fbg_act4(v, bnc, jcin[i], has);
            return ok ? r : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    __device__ void epilogue(const Params& p, int m0, int n0, int z, const float* Cs, int tid, bool) {
        int kb, ke;
        krange(p, z, kb, ke);
        if (kb >= ke) return;                                  // (uniform) no rows for this slice: nothing to add
        for (int idx = tid; idx < TM * TN; idx += 256) {
            const int r = idx / TN, c = idx % TN, co = m0 + r, j = n0 + c;
            if (co < p.Cout && j < K) {
                const int tap = j / Cin, cin = j - tap * Cin;
                atomicAdd(&p.dw[((size_t)co * Cin + cin) * 27 + tap], Cs[r * (TN + 1) + c]);
            }
        }
        if (n0 != 0) return;                                   // (uniform)
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const int row = ((tid + i * 256) % (TM / 4)) * 4;
            atomicAdd(&bred[row], bsum[i].x); atomicAdd(&bred[row + 1], bsum[i].y); atomicAdd(&bred[row + 2], bsum[i].z); atomicAdd(&bred[row + 3], bsum[i].w);
        }
        __syncthreads();
        if (tid < TM && m0 + tid < p.Cout) atomicAdd(&p.dbias[m0 + tid], bred[tid]);
    }
};

// ------------------------------------------------------------------------------------------------------
// backward, data: the input voxels fall into 8 parity classes z = (pd, ph, pw).  Along one axis an even input index i is read by tap 1 of
// output i / 2 only; an odd one by tap 0 of output (i + 1) / 2 (absent at the right edge of an even axis) and tap 2 of output (i - 1) / 2.
// A class is a dense GEMM: rows = its voxels, cols = Cin, k = ti * Cout + co over its 1 / 2 / 4 / 8 taps.
// Epilogue: ReLU mask from the recomputed BN output, dbn_in, BN-backward sums s1 / s2 in fp64 (what fb_conv_bwd_x_kernel produces).
// ------------------------------------------------------------------------------------------------------
template <int WM_, int WN_>
struct FbBwdXOp {
    typedef FbConvP Params;
    static constexpr int WM = WM_, WN = WN_, WK = 4 / (WM_ * WN_), AMODE = LD_K4, BMODE = LD_K1;
    static constexpr int TM = 32 * WM, TN = 32 * WN;
    static constexpr int EXTRA = 4 * TN + 2 * TM;
    static_assert(WK == 1 && 2 * TM * (TN + 1) <= 2 * (TM + TN) * 36, "the epilogue keeps two [TM][TN+1] images in the tile buffers");
    float* cst; const int* rows;
    int m0, K, Cin, Cout, oD, oH, oW, pd, ph, pw, nrows;
    __device__ void step(const Params&, int) {}
    __device__ void setup(const Params& p, int m0_, int, int z, float* extra, int tid) {
        cst = extra; rows = (const int*)(extra + 4 * TN); m0 = m0_;
        pd = z >> 2; ph = (z >> 1) & 1; pw = z & 1;
        Cin = p.Cin; Cout = p.Cout; oD = p.out.D; oH = p.out.H; oW = p.out.W;
        K = Cout << (pd + ph + pw);
        const int nd = pd ? p.in.D / 2 : (p.in.D + 1) / 2, nh = ph ? p.in.H / 2 : (p.in.H + 1) / 2, nw = pw ? p.in.W / 2 : (p.in.W + 1) / 2;
        const int cv = nd * nh * nw;
        nrows = p.B * cv;
        if (tid < TM) {
            const int r = m0 + tid;
            int pk = 0, b = -1;
            if (r < nrows) {
                b = r / cv;
                const int q = r - b * cv, jd = q / (nh * nw), jh = (q / nw) % nh, jw = q % nw;
                pk = pack_dhw(2 * jd + pd, 2 * jh + ph, 2 * jw + pw);
            }
            ((int*)extra)[4 * TN + 2 * tid] = pk; ((int*)extra)[4 * TN + 2 * tid + 1] = b;
        }
    }
    __device__ void krange(const Params&, int, int& kb, int& ke) { kb = 0; ke = m0 < nrows ? K : 0; }
    __device__ void taps(int ti, int& td, int& th, int& tw) const {
        td = th = tw = 1;
        if (pw) { tw = (ti & 1) * 2; ti >>= 1; }
        if (ph) { th = (ti & 1) * 2; ti >>= 1; }
        if (pd) { td = (ti & 1) * 2; }
    }
    typedef float4 ARaw;
    typedef float BRaw;
    __device__ float4 a_ld(const Params& p, int, int m, int k, bool& ok) const {
        const int rr = m - m0, pk = rows[2 * rr], b = rows[2 * rr + 1];
        const int kk = k < K ? k : 0, ti = kk / Cout, co = kk - ti * Cout;
        int td, th, tw, id, ih, iw;
        taps(ti, td, th, tw); unpack_dhw(pk, id, ih, iw);
        const int od = (id + 1 - td) >> 1, oh = (ih + 1 - th) >> 1, ow = (iw + 1 - tw) >> 1;      // (even and >= 0 by construction)
        ok = b >= 0 && k < K && od < oD && oh < oH && ow < oW;
        return *(const float4*)(p.dy + (ok ? (size_t)(((b * oD + od) * oH + oh) * oW + ow) * Cout + co : 0));
    }
    __device__ float4 a_tx(const Params&, int, const float4& v, int, int, bool ok) const { return ok ? v : make_float4(0.f, 0.f, 0.f, 0.f); }
    __device__ float b_ld(const Params& p, int, int n, int k, bool& ok) const {
        ok = n < Cin && k < K;
        const int kk = ok ? k : 0, ti = kk / Cout, co = kk - ti * Cout;
        int td, th, tw;
        taps(ti, td, th, tw);
        return p.w[ok ? ((size_t)co * Cin + n) * 27 + (td * 3 + th) * 3 + tw : 0];
    }
    __device__ float b_tx(const Params&, int, const float& v, int, int, bool ok) const { return ok ? v : 0.f; }
    __device__ void epilogue(const Params& p, int m0_, int n0, int, const float* Cs, int tid, bool) {
        if (m0_ >= nrows) return;                              // (uniform) a class smaller than class 0
        if (tid < TN && n0 + tid < Cin) {
            float mu, rs;
            bn_mean_rstd(p.bn, n0 + tid, mu, rs);
            cst[tid] = mu; cst[TN + tid] = rs; cst[2 * TN + tid] = p.bn.gamma[n0 + tid]; cst[3 * TN + tid] = p.bn.beta[n0 + tid];
        }
        __syncthreads();
        float* G = const_cast<float*>(Cs);
        float* X = G + TM * (TN + 1);
        for (int idx = tid; idx < TM * TN; idx += 256) {
            const int r = idx / TN, c = idx % TN, b = rows[2 * r + 1], cin = n0 + c;
            float g = 0.f, xh = 0.f;
            if (b >= 0 && cin < Cin) {
                int id, ih, iw;
                unpack_dhw(rows[2 * r], id, ih, iw);
                const size_t o = (size_t)(((b * p.in.D + id) * p.in.H + ih) * p.in.W + iw) * Cin + cin;
                xh = (p.x[o] - cst[c]) * cst[TN + c];
                g = fmaf(cst[2 * TN + c], xh, cst[3 * TN + c]) > 0.f ? G[r * (TN + 1) + c] : 0.f;
                p.dbn_in[o] = g;
            }
            G[r * (TN + 1) + c] = g; X[r * (TN + 1) + c] = xh;
        }
        __syncthreads();
        if (tid >= TN || n0 + tid >= Cin) return;
        double s1 = 0, s2 = 0;
        for (int r = 0; r < TM; ++r) { const float g = G[r * (TN + 1) + tid]; s1 += g; s2 += (double)g * X[r * (TN + 1) + tid]; }
        atomicAdd(&p.s1[n0 + tid], s1); atomicAdd(&p.s2[n0 + tid], s2);
    }
};

// ------------------------------------------------------------------------------------------------------
// BN + ReLU + global average pool and its backward (VALU).  Workgroup = (64 channels, sample b, member); its 4 waves split the voxels.
// ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void fbg_pool_fwd_kernel(const Grp<FbPoolP> grp) {
    __shared__ float red[4][64];
    const FbPoolP& p = grp.p[blockIdx.z];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, c = blockIdx.x * 64 + lane, b = blockIdx.y;
    float a = 0.f;
    if (c < p.C) {
        float mu, rs;
        bn_mean_rstd(p.bn, c, mu, rs);
        const float sc = p.bn.gamma[c] * rs, be = p.bn.beta[c];
        for (int v = wv; v < p.V; v += 4) a += fmaxf(bn_apply(p.y[((size_t)b * p.V + v) * p.C + c], mu, sc, be), 0.f);
    }
    red[wv][lane] = a;
    __syncthreads();
    if (wv == 0 && c < p.C) p.out[(size_t)b * p.ldo + c] = (red[0][lane] + red[1][lane] + red[2][lane] + red[3][lane]) / (float)p.V;
}
__global__ __launch_bounds__(256) void fbg_pool_bwd_kernel(const Grp<FbPoolP> grp) {
    __shared__ double red[2][4][64];
    const FbPoolP& p = grp.p[blockIdx.z];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, c = blockIdx.x * 64 + lane, b = blockIdx.y;
    double s1 = 0, s2 = 0;
    if (c < p.C) {
        float mu, rs;
        bn_mean_rstd(p.bn, c, mu, rs);
        const float ga = p.bn.gamma[c], be = p.bn.beta[c], d = p.dout[(size_t)b * p.lddout + c] / (float)p.V;
        for (int v = wv; v < p.V; v += 4) {
            const size_t o = ((size_t)b * p.V + v) * p.C + c;
            const float xh = (p.y[o] - mu) * rs;
            const float g = fmaf(ga, xh, be) > 0.f ? d : 0.f;
            p.dbn[o] = g;
            s1 += g; s2 += (double)g * xh;
        }
    }
    red[0][wv][lane] = s1; red[1][wv][lane] = s2;
    __syncthreads();
    if (wv == 0 && c < p.C) {
        atomicAdd(&p.s1[c], red[0][0][lane] + red[0][1][lane] + red[0][2][lane] + red[0][3][lane]);
        atomicAdd(&p.s2[c], red[1][0][lane] + red[1][1][lane] + red[1][2][lane] + red[1][3][lane]);
    }
}

// ---- argument checks: one shape for the whole group, shapes the tile configurations take, every pointer an op reads or writes ----
enum { FBG_FWD = 0, FBG_BWD_W = 1, FBG_BWD_X = 2 };
inline bool a16(const void* q) { return ((uintptr_t)q & 15) == 0; }
bool fbg_conv_ok(const FbConvP* pp, int ng, int op) {
    if (!pp || ng < 1 || ng > MMS_MAX_GROUP) return false;
    const FbConvP& p = *pp;
    if (p.B <= 0 || p.in.D < 1 || p.in.H < 1 || p.in.W < 1 || p.in.D > 1024 || p.in.H > 1024 || p.in.W > 1024) return false;
    if (p.out.D != (p.in.D + 1) / 2 || p.out.H != (p.in.H + 1) / 2 || p.out.W != (p.in.W + 1) / 2) return false;
    // 32-wide column tiles whose last one may be half filled (every op masks its columns), float4 rows of dy.  Cout % 64 == 48 (48, 112)
    // stays refused although nothing in the kernels needs that: the argument checks of tests/test_gpu_fb_group.py pin Cout = 48 as an error.
    if (p.Cout <= 0 || p.Cout % 16 != 0 || p.Cout % 64 == 48 || p.Cout > 1024) return false;
    if (!(p.Cin == 1 && !p.has_bn) && !(p.Cin % 16 == 0 && p.Cin >= 16 && p.Cin <= 128)) return false;      // BN constants of <= 128 channels in LDS
    if (op == FBG_BWD_X && (p.Cin == 1 || !p.has_bn)) return false;
    if (op == FBG_BWD_W && (p.msplit < 1 || p.msplit > 1024)) return false;
    const long rin = (long)p.B * p.in.D * p.in.H * p.in.W, rout = (long)p.B * p.out.D * p.out.H * p.out.W;
    if (rin * p.Cin >= (1L << 31) || rout * p.Cout >= (1L << 31) || (long)p.Cout * p.Cin * 27 >= (1L << 31)) return false;
    for (int g = 0; g < ng; ++g) {
        const FbConvP& q = pp[g];
        if (q.Cin != p.Cin || q.Cout != p.Cout || q.B != p.B || q.has_bn != p.has_bn || q.msplit != p.msplit || q.in.D != p.in.D || q.in.H != p.in.H ||
            q.in.W != p.in.W || q.out.D != p.out.D || q.out.H != p.out.H || q.out.W != p.out.W) return false;
        if (!q.x || (q.Cin > 1 && !a16(q.x))) return false;
        if (q.has_bn && (!q.bn.gamma || !q.bn.beta || (q.bn.train ? (!q.bn.sum || !q.bn.sumsq) : (!q.bn.rmean || !q.bn.rvar)))) return false;
        if (op == FBG_FWD && (!q.w || !q.bias || !q.y || (q.osum == nullptr) != (q.osumsq == nullptr))) return false;
        if (op == FBG_BWD_W && (!q.dy || !a16(q.dy) || !q.dw || !q.dbias)) return false;
        if (op == FBG_BWD_X && (!q.dy || !a16(q.dy) || !q.w || !q.dbn_in || !q.s1 || !q.s2)) return false;
    }
    return true;
}
bool fbg_pool_ok(const FbPoolP* pp, int ng, bool bwd) {
    if (!pp || ng < 1 || ng > MMS_MAX_GROUP) return false;
    const FbPoolP& p = *pp;
    if (p.C <= 0 || p.V <= 0 || p.B <= 0 || p.B > 65535 || (long)p.B * p.V * p.C >= (1L << 31)) return false;
    for (int g = 0; g < ng; ++g) {
        const FbPoolP& q = pp[g];
        if (q.C != p.C || q.V != p.V || q.B != p.B || !q.y || !q.bn.gamma || !q.bn.beta) return false;
        if (q.bn.train ? (!q.bn.sum || !q.bn.sumsq) : (!q.bn.rmean || !q.bn.rvar)) return false;
        if (!bwd && (!q.out || q.ldo < q.C)) return false;
        if (bwd && (!q.dout || q.lddout < q.C || !q.dbn || !q.s1 || !q.s2 || !q.bn.train)) return false;
    }
    return true;
}

// ------------------------------------------------------------------------------------------------------
// Fused tail of ImageOnlyModel: BN3 + ReLU + global average pool -> Linear(C, N1) + ReLU -> Linear(N1, N2), one launch per pass.
// The arguments are the blocks of the three launches it replaces (FbPoolP + two LinearFwdP / LinearBwdP), condensed on the host.
// Forward: workgroup = (sample b, member); the pool is fbg_pool_fwd_kernel's (same wave split, same summation order).
// Backward: workgroups 0..B-1 = one sample each: its row of dL/dfeats recomputed from dhz (N2 x N1 + N1 x C fmas) and the pool backward
// of fbg_pool_bwd_kernel (dbn3, fp64 s1 / s2); workgroup B owns the four parameter gradients over all B <= 32 rows: no float atomics.
// ------------------------------------------------------------------------------------------------------
struct ImgTailK {
    const float* y; BnSrc bn; int C, V, B;
    float* feats; int ldf;
    const float* w1; const float* b1; int N1; float* f1; int ld1;
    const float* w2; const float* b2; int N2; float* hz; int ldh;
    const float* dhz; int lddh;
    float* dw1; float* db1; float* dw2; float* db2;
    float* dbn; double* s1; double* s2;
};
constexpr int IT_C = 128, IT_N1 = 64, IT_N2 = 8, IT_B = 32;

__global__ __launch_bounds__(256) void img_tail_fwd_kernel(const Grp<ImgTailK> grp) {
    __shared__ float red[4][IT_C];
    __shared__ float feat[IT_C];
    __shared__ float h1[IT_N1];
    const ImgTailK& p = grp.p[blockIdx.y];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, b = blockIdx.x;
    for (int c = lane; c < p.C; c += 64) {
        float mu, rs;
        bn_mean_rstd(p.bn, c, mu, rs);
        const float sc = p.bn.gamma[c] * rs, be = p.bn.beta[c];
        float a = 0.f;
        for (int v = wv; v < p.V; v += 4) a += fmaxf(bn_apply(p.y[((size_t)b * p.V + v) * p.C + c], mu, sc, be), 0.f);
        red[wv][c] = a;
    }
    __syncthreads();
    if (tid < p.C) {
        const float f = (red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid]) / (float)p.V;
        feat[tid] = f; p.feats[(size_t)b * p.ldf + tid] = f;
    }
    __syncthreads();
    // Linear 1: 8 lanes per output feature split K, summed by shuffles
    for (int n = tid >> 3; n < p.N1; n += 32) {
        float acc = 0.f;
        for (int k = tid & 7; k < p.C; k += 8) acc = fmaf(p.w1[(size_t)n * p.C + k], feat[k], acc);
        acc += __shfl_xor(acc, 4, 64); acc += __shfl_xor(acc, 2, 64); acc += __shfl_xor(acc, 1, 64);
        if ((tid & 7) == 0) {
            const float h = fmaxf(acc + p.b1[n], 0.f);
            h1[n] = h; p.f1[(size_t)b * p.ld1 + n] = h;
        }
    }
    __syncthreads();
    if (tid < p.N2) {
        float acc = 0.f;
        for (int k = 0; k < p.N1; ++k) acc = fmaf(p.w2[(size_t)tid * p.N1 + k], h1[k], acc);
        p.hz[(size_t)b * p.ldh + tid] = acc + p.b2[tid];
    }
}

__global__ __launch_bounds__(256) void img_tail_bwd_kernel(const Grp<ImgTailK> grp) {
    __shared__ float g1[IT_B * IT_N1];          // dL/d(pre-ReLU Linear 1): the sample's row, or all B rows in the parameter workgroup
    __shared__ float dfe[IT_C];
    __shared__ double red[2][4][IT_C];
    const ImgTailK& p = grp.p[blockIdx.y];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if ((int)blockIdx.x == p.B) {               // (workgroup-uniform) parameter gradients, accumulated like mms_linear_bwd's
        for (int idx = tid; idx < p.B * p.N1; idx += 256) {
            const int m = idx / p.N1, n = idx - m * p.N1;
            float g = 0.f;
            for (int j = 0; j < p.N2; ++j) g = fmaf(p.dhz[(size_t)m * p.lddh + j], p.w2[(size_t)j * p.N1 + n], g);
            g1[idx] = p.f1[(size_t)m * p.ld1 + n] > 0.f ? g : 0.f;
        }
        __syncthreads();
        for (int idx = tid; idx < p.N2 * p.N1; idx += 256) {
            const int j = idx / p.N1, n = idx - j * p.N1;
            float a = 0.f;
            for (int m = 0; m < p.B; ++m) a = fmaf(p.dhz[(size_t)m * p.lddh + j], p.f1[(size_t)m * p.ld1 + n], a);
            p.dw2[idx] += a;
        }
        if (tid < p.N2) {
            float a = 0.f;
            for (int m = 0; m < p.B; ++m) a += p.dhz[(size_t)m * p.lddh + tid];
            p.db2[tid] += a;
        }
        for (int idx = tid; idx < p.N1 * p.C; idx += 256) {
            const int n = idx / p.C, c = idx - n * p.C;
            float a = 0.f;
            for (int m = 0; m < p.B; ++m) a = fmaf(g1[m * p.N1 + n], p.feats[(size_t)m * p.ldf + c], a);
            p.dw1[idx] += a;
        }
        if (tid < p.N1) {
            float a = 0.f;
            for (int m = 0; m < p.B; ++m) a += g1[m * p.N1 + tid];
            p.db1[tid] += a;
        }
        return;
    }
    const int b = blockIdx.x;
    if (tid < p.N1) {
        float g = 0.f;
        for (int j = 0; j < p.N2; ++j) g = fmaf(p.dhz[(size_t)b * p.lddh + j], p.w2[(size_t)j * p.N1 + tid], g);
        g1[tid] = p.f1[(size_t)b * p.ld1 + tid] > 0.f ? g : 0.f;
    }
    __syncthreads();
    if (tid < p.C) {
        float a = 0.f;
        for (int n = 0; n < p.N1; ++n) a = fmaf(g1[n], p.w1[(size_t)n * p.C + tid], a);
        dfe[tid] = a;
    }
    __syncthreads();
    for (int c = lane; c < p.C; c += 64) {
        float mu, rs;
        bn_mean_rstd(p.bn, c, mu, rs);
        const float ga = p.bn.gamma[c], be = p.bn.beta[c], d = dfe[c] / (float)p.V;
        double s1 = 0, s2 = 0;
        for (int v = wv; v < p.V; v += 4) {
            const size_t o = ((size_t)b * p.V + v) * p.C + c;
            const float xh = (p.y[o] - mu) * rs;
            const float g = fmaf(ga, xh, be) > 0.f ? d : 0.f;
            p.dbn[o] = g;
            s1 += g; s2 += (double)g * xh;
        }
        red[0][wv][c] = s1; red[1][wv][c] = s2;
    }
    __syncthreads();
    if (tid < p.C) {
        atomicAdd(&p.s1[tid], red[0][0][tid] + red[0][1][tid] + red[0][2][tid] + red[0][3][tid]);
        atomicAdd(&p.s2[tid], red[1][0][tid] + red[1][1][tid] + red[1][2][tid] + red[1][3][tid]);
    }
}

// the three launches' blocks -> ImgTailK; false when they are not a BN+ReLU+pool -> Linear+ReLU -> Linear chain on shared buffers
bool img_tail_fill(Grp<ImgTailK>& a, const FbPoolP* pool, const LinearFwdP* f1, const LinearFwdP* f2, const LinearBwdP* b1, const LinearBwdP* b2,
                   int ng) {
    const bool bwd = b1 != nullptr;
    if (!fbg_pool_ok(pool, ng, false) || (bwd ? (!b1 || !b2) : (!f1 || !f2))) return false;
    for (int g = 0; g < ng; ++g) {
        const FbPoolP& q = pool[g];
        ImgTailK& k = a.p[g];
        k = ImgTailK{};
        k.y = q.y; k.bn = q.bn; k.C = q.C; k.V = q.V; k.B = q.B; k.feats = q.out; k.ldf = q.ldo;
        int M1, K1, M2, K2, relu1, relu2;
        const InProlog *p1, *p2;
        const float *x1, *x2;
        if (!bwd) {
            const LinearFwdP &u = f1[g], &v = f2[g];
            k.w1 = u.w; k.b1 = u.bias; k.N1 = u.N; k.f1 = u.y; k.ld1 = u.ldy; k.w2 = v.w; k.b2 = v.bias; k.N2 = v.N; k.hz = v.y; k.ldh = v.ldy;
            M1 = u.M; K1 = u.K; M2 = v.M; K2 = v.K; relu1 = u.out_relu; relu2 = v.out_relu; p1 = &u.pro; p2 = &v.pro; x1 = u.x; x2 = v.x;
            if (!k.b1 || !k.b2 || !k.hz || u.ldx != q.ldo || v.ldx != u.ldy) return false;
        } else {
            const LinearBwdP &u = b1[g], &v = b2[g];
            k.w1 = u.w; k.N1 = u.N; k.f1 = const_cast<float*>(u.y); k.ld1 = u.ldy; k.w2 = v.w; k.N2 = v.N; k.dhz = v.dy; k.lddh = v.lddy;
            k.dw1 = u.dw; k.db1 = u.dbias; k.dw2 = v.dw; k.db2 = v.dbias; k.dbn = q.dbn; k.s1 = q.s1; k.s2 = q.s2;
            M1 = u.M; K1 = u.K; M2 = v.M; K2 = v.K; relu1 = u.out_relu; relu2 = v.out_relu; p1 = &u.pro; p2 = &v.pro; x1 = u.x; x2 = v.x;
            if (!k.dhz || !k.dw1 || !k.db1 || !k.dw2 || !k.db2 || !k.dbn || !k.s1 || !k.s2 || !q.bn.train || u.ldx != q.ldo || v.ldx != u.ldy || k.lddh < k.N2)
                return false;
        }
        if (!k.w1 || !k.w2 || !k.f1 || x1 != q.out || x2 != k.f1 || M1 != q.B || M2 != q.B || K1 != q.C || K2 != k.N1 || !relu1 || relu2) return false;
        if (p1->bn || p2->bn || p1->drop_mask || p2->drop_mask || (p1->train && p1->drop_p > 0.f) || (p2->train && p2->drop_p > 0.f)) return false;
        if (q.B > IT_B || q.C > IT_C || k.N1 < 1 || k.N1 > IT_N1 || k.N2 < 1 || k.N2 > IT_N2 || k.ld1 < k.N1 || (!bwd && k.ldh < k.N2)) return false;
        if (g && (k.N1 != a.p[0].N1 || k.N2 != a.p[0].N2)) return false;
    }
    a.zdim = 1;
    return true;
}
}  // namespace

extern "C" int mms_fb_conv_fwd_group(const FbConvP* pp, int ng, hipStream_t s) {
    if (!fbg_conv_ok(pp, ng, FBG_FWD)) return MMS_ERR_ARG;
    const FbConvP& p = *pp;
    const int M = p.B * p.out.D * p.out.H * p.out.W;
    if (p.Cin == 1) return launch_tile_gemm<FbFwdOp<4, 1, 1, true>>(pp, ng, dim3((M + 127) / 128, (p.Cout + 31) / 32, 1), s);
    // tile shape from ONE member's work, so that a model's arithmetic does not depend on the group it runs in
    if (p.Cout % 64 == 0 && (long)M * p.Cout >= 128L * 64 * 64) return launch_tile_gemm<FbFwdOp<2, 2, 1, false>>(pp, ng, dim3((M + 63) / 64, p.Cout / 64, 1), s);
    return launch_tile_gemm<FbFwdOp<1, 1, 4, false>>(pp, ng, dim3((M + 31) / 32, (p.Cout + 31) / 32, 1), s);      // few rows: the 4 waves split K
}
extern "C" int mms_fb_conv_bwd_w_group(const FbConvP* pp, int ng, hipStream_t s) {
    if (!fbg_conv_ok(pp, ng, FBG_BWD_W)) return MMS_ERR_ARG;
    const FbConvP& p = *pp;
    const dim3 g((p.Cout + 63) / 64, (27 * p.Cin + 63) / 64, p.msplit);
    return p.Cin == 1 ? launch_tile_gemm<FbBwdWOp<true>>(pp, ng, g, s) : launch_tile_gemm<FbBwdWOp<false>>(pp, ng, g, s);
}
extern "C" int mms_fb_conv_bwd_x_group(const FbConvP* pp, int ng, hipStream_t s) {
    if (!fbg_conv_ok(pp, ng, FBG_BWD_X)) return MMS_ERR_ARG;
    const FbConvP& p = *pp;
    const int rows0 = p.B * ((p.in.D + 1) / 2) * ((p.in.H + 1) / 2) * ((p.in.W + 1) / 2);      // class (even, even, even) is the largest
    if (p.Cin % 64 == 0) return launch_tile_gemm<FbBwdXOp<2, 2>>(pp, ng, dim3((rows0 + 63) / 64, p.Cin / 64, 8), s);
    return launch_tile_gemm<FbBwdXOp<4, 1>>(pp, ng, dim3((rows0 + 127) / 128, (p.Cin + 31) / 32, 8), s);      // (a last column tile of 16: masked)
}
extern "C" int mms_fb_pool_fwd_group(const FbPoolP* pp, int ng, hipStream_t s) {
    Grp<FbPoolP> a;
    if (!fbg_pool_ok(pp, ng, false) || !grp_fill(a, pp, ng, 1)) return MMS_ERR_ARG;
    MMS_LAUNCH(fbg_pool_fwd_kernel, dim3((pp->C + 63) / 64, pp->B, ng), dim3(256), 0, s, a);
    return mms_check_launch();
}
extern "C" int mms_fb_pool_bwd_group(const FbPoolP* pp, int ng, hipStream_t s) {
    Grp<FbPoolP> a;
    if (!fbg_pool_ok(pp, ng, true) || !grp_fill(a, pp, ng, 1)) return MMS_ERR_ARG;
    MMS_LAUNCH(fbg_pool_bwd_kernel, dim3((pp->C + 63) / 64, pp->B, ng), dim3(256), 0, s, a);
    return mms_check_launch();
}
extern "C" int mms_img_tail_fwd_group(const FbPoolP* pool, const LinearFwdP* l1, const LinearFwdP* l2, int ng, hipStream_t s) {
    Grp<ImgTailK> a;
    if (!img_tail_fill(a, pool, l1, l2, nullptr, nullptr, ng)) return MMS_ERR_ARG;
    MMS_LAUNCH(img_tail_fwd_kernel, dim3(pool->B, ng), dim3(256), 0, s, a);
    return mms_check_launch();
}
extern "C" int mms_img_tail_bwd_group(const FbPoolP* pool, const LinearBwdP* l1, const LinearBwdP* l2, int ng, hipStream_t s) {
    Grp<ImgTailK> a;
    if (!l1 || !l2 || !img_tail_fill(a, pool, nullptr, nullptr, l1, l2, ng)) return MMS_ERR_ARG;
    MMS_LAUNCH(img_tail_bwd_kernel, dim3(pool->B + 1, ng), dim3(256), 0, s, a);
    return mms_check_launch();
}

// ================================= whole-encoder drivers (lock-step) =================================
// Per-member workspace: the plan of fb_plan.h, the one the single-model drivers and mms_fb3_init use.  The caller states how many bytes
// each workspace holds; a size that is not this width set's plan is MMS_ERR_ARG.
using namespace fbplan;
namespace {
// rows of the weight-gradient GEMM per workgroup: enough workgroups to fill the chip with ONE member, no more (each slice is one
// [Cout][27 Cin] image of fp32 atomics: atomic bytes per launch = msplit x the gradient's size)
inline int fbg_msplit(int Cin, int Cout, int M) {
    const int tiles = ((Cout + 63) / 64) * ((27 * Cin + 63) / 64), steps = (M + 31) / 32;
    int ms = (256 + tiles - 1) / tiles;
    if (ms > steps / 4) ms = steps / 4;            // >= 4 K steps (128 rows) per slice
    return ms < 1 ? 1 : ms;
}
inline bool fbg_widths_ok(const int* widths) {      // what mms_fb_conv_*_group takes as Cout
    if (!fb_widths_ok(widths)) return false;
    for (int l = 0; l < 3; ++l)
        if (widths[l] % 64 == 48) return false;
    return true;
}
}  // namespace

extern "C" int mms_bn_running_update_group(const void* const*, int, int, float, hipStream_t);
extern "C" int mms_zero_regions_group(void* const*, int, size_t, hipStream_t);
extern "C" int mms_bn_bwd_apply_group(const BnBwdApplyP*, int, hipStream_t);
#define TRY(x) do { int rc_ = (x); if (rc_ != MMS_OK) return rc_; } while (0)

extern "C" int mms_img_tail_fwd_group(const FbPoolP*, const LinearFwdP*, const LinearFwdP*, int, hipStream_t);
extern "C" int mms_img_tail_bwd_group(const FbPoolP*, const LinearBwdP*, const LinearBwdP*, int, hipStream_t);

// l1 / l2 != NULL: the pool launch is the fused tail (pool + the two Linear layers that read its output)
static int fbg_forward(int ng, void* const* ws, size_t ws_bytes, const int* widths, int B, int D, int H, int W, const float* const* x,
                       const void* const* const* params, const void* const* const* buffers, float* const* out, int ldo, int train,
                       const LinearFwdP* l1, const LinearFwdP* l2, hipStream_t s) {
    FbPlan P;
    if (ng < 1 || ng > MMS_MAX_GROUP || !fbg_widths_ok(widths) || !fb_plan(P, widths, B, D, H, W) || ws_bytes != P.total) return MMS_ERR_ARG;
    if (!ws || !x || !params || !out || ldo < P.C[3]) return MMS_ERR_ARG;
    for (int g = 0; g < ng; ++g) {
        if (!ws[g] || !x[g] || !params[g] || !out[g] || (!train && (!buffers || !buffers[g]))) return MMS_ERR_ARG;
        for (int i = 0; i < 12; ++i)
            if (!params[g][i]) return MMS_ERR_ARG;
    }
    if (train) {
        void* reg[MMS_MAX_GROUP];
        for (int g = 0; g < ng; ++g) reg[g] = at<void>(ws[g], P.stats_begin);
        TRY(mms_zero_regions_group(reg, ng, P.stats_end - P.stats_begin, s));
    }
    FbConvP c[MMS_MAX_GROUP];
    for (int l = 1; l < 4; ++l) {
        for (int g = 0; g < ng; ++g) {
            const float* const* prm = (const float* const*)params[g];
            const void* const* buf = buffers ? buffers[g] : nullptr;
            c[g] = FbConvP{};
            c[g].x = l == 1 ? x[g] : at<float>(ws[g], P.y[l - 1]); c[g].Cin = P.C[l - 1]; c[g].in = P.g[l - 1]; c[g].out = P.g[l]; c[g].B = B;
            c[g].has_bn = l > 1; if (l > 1) c[g].bn = fb_bn(ws[g], P, l - 1, prm, buf, train);
            c[g].w = prm[4 * (l - 1)]; c[g].bias = prm[4 * (l - 1) + 1]; c[g].Cout = P.C[l];
            c[g].y = at<float>(ws[g], P.y[l]);
            c[g].osum = train ? at<double>(ws[g], P.st[l]) : nullptr; c[g].osumsq = train ? at<double>(ws[g], P.st[l]) + 128 : nullptr;
        }
        TRY(mms_fb_conv_fwd_group(c, ng, s));
    }
    FbPoolP pl[MMS_MAX_GROUP];
    bool upd = train != 0;
    const void* tabs[MMS_MAX_GROUP];
    for (int g = 0; g < ng; ++g) {
        const void* const* buf = buffers ? buffers[g] : nullptr;
        pl[g] = FbPoolP{};
        pl[g].y = at<float>(ws[g], P.y[3]); pl[g].C = P.C[3]; pl[g].V = P.M[3] / B; pl[g].B = B;
        pl[g].bn = fb_bn(ws[g], P, 3, (const float* const*)params[g], buf, train);
        pl[g].out = out[g]; pl[g].ldo = ldo;
        tabs[g] = at<void>(ws[g], P.tab_bn);
        upd = upd && buf;
    }
    if (l1) TRY(mms_img_tail_fwd_group(pl, l1, l2, ng, s));
    else TRY(mms_fb_pool_fwd_group(pl, ng, s));
    if (upd) TRY(mms_bn_running_update_group(tabs, ng, 3, 0.1f, s));
    return MMS_OK;
}

extern "C" int mms_fb3_forward_group(int ng, void* const* ws, size_t ws_bytes, const int* widths, int B, int D, int H, int W, const float* const* x,
                                     const void* const* const* params, const void* const* const* buffers, float* const* out, int ldo, int train,
                                     hipStream_t s) {
    return fbg_forward(ng, ws, ws_bytes, widths, B, D, H, W, x, params, buffers, out, ldo, train, nullptr, nullptr, s);
}
extern "C" int mms_img_forward_group(int ng, void* const* ws, size_t ws_bytes, const int* widths, int B, int D, int H, int W, const float* const* x,
                                     const void* const* const* params, const void* const* const* buffers, float* const* out, int ldo, int train,
                                     const LinearFwdP* l1, const LinearFwdP* l2, hipStream_t s) {
    if (!l1 || !l2) return MMS_ERR_ARG;
    return fbg_forward(ng, ws, ws_bytes, widths, B, D, H, W, x, params, buffers, out, ldo, train, l1, l2, s);
}

// l1 / l2 != NULL: the fused tail's backward replaces the pool backward (dout is not read: the tail derives it from l2's dy)
static int fbg_backward(int ng, void* const* ws, size_t ws_bytes, const int* widths, int B, int D, int H, int W, const float* const* x,
                        const void* const* const* params, const float* const* dout, int lddout, void* const* const* grads,
                        const LinearBwdP* l1, const LinearBwdP* l2, hipStream_t s) {
    FbPlan P;
    if (ng < 1 || ng > MMS_MAX_GROUP || !fbg_widths_ok(widths) || !fb_plan(P, widths, B, D, H, W) || ws_bytes != P.total) return MMS_ERR_ARG;
    if (!ws || !x || !params || !grads || (!l1 && (!dout || lddout < P.C[3]))) return MMS_ERR_ARG;
    for (int g = 0; g < ng; ++g) {
        if (!ws[g] || !x[g] || !params[g] || (!l1 && !dout[g]) || !grads[g]) return MMS_ERR_ARG;
        for (int i = 0; i < 12; ++i)
            if (!params[g][i] || !grads[g][i]) return MMS_ERR_ARG;
    }
    FbPoolP pl[MMS_MAX_GROUP];
    for (int g = 0; g < ng; ++g) {
        pl[g] = FbPoolP{};
        pl[g].y = at<float>(ws[g], P.y[3]); pl[g].C = P.C[3]; pl[g].V = P.M[3] / B; pl[g].B = B;
        pl[g].bn = fb_bn(ws[g], P, 3, (const float* const*)params[g], nullptr, 1);
        pl[g].dbn = at<float>(ws[g], P.dbn[3]);
        pl[g].s1 = at<double>(ws[g], P.bb[3]); pl[g].s2 = pl[g].s1 + 128;
        if (l1) { pl[g].out = const_cast<float*>(l1[g].x); pl[g].ldo = l1[g].ldx; }      // the pooled features the forward wrote
        else { pl[g].dout = dout[g]; pl[g].lddout = lddout; }
    }
    if (l1) TRY(mms_img_tail_bwd_group(pl, l1, l2, ng, s));
    else TRY(mms_fb_pool_bwd_group(pl, ng, s));
    BnBwdApplyP ap[MMS_MAX_GROUP];
    FbConvP c[MMS_MAX_GROUP];
    for (int l = 3; l >= 1; --l) {
        for (int g = 0; g < ng; ++g) {
            const float* const* prm = (const float* const*)params[g];
            float* const* grd = (float* const*)grads[g];
            void* w = ws[g];
            // BN_l backward: dbn_l -> dy_l (gradient w.r.t. the raw conv output), BN parameter grads
            ap[g] = BnBwdApplyP{at<float>(w, P.dbn[l]), P.C[l], at<float>(w, P.y[l]), P.C[l], at<float>(w, P.dy[l]), P.C[l], P.M[l], P.C[l],
                                fb_bn(w, P, l, prm, nullptr, 1), BnBwd{at<double>(w, P.bb[l]), at<double>(w, P.bb[l]) + 128, 0, 0}, 0,
                                grd[4 * (l - 1) + 2], grd[4 * (l - 1) + 3]};
            c[g] = FbConvP{};
            c[g].x = l == 1 ? x[g] : at<float>(w, P.y[l - 1]); c[g].Cin = P.C[l - 1]; c[g].in = P.g[l - 1]; c[g].out = P.g[l]; c[g].B = B;
            c[g].has_bn = l > 1; if (l > 1) c[g].bn = fb_bn(w, P, l - 1, prm, nullptr, 1);
            c[g].w = prm[4 * (l - 1)]; c[g].Cout = P.C[l]; c[g].dy = at<float>(w, P.dy[l]);
            c[g].dw = grd[4 * (l - 1)]; c[g].dbias = grd[4 * (l - 1) + 1];
            c[g].msplit = fbg_msplit(P.C[l - 1], P.C[l], P.M[l]);
            if (l > 1) { c[g].dbn_in = at<float>(w, P.dbn[l - 1]); c[g].s1 = at<double>(w, P.bb[l - 1]); c[g].s2 = c[g].s1 + 128; }
        }
        TRY(mms_bn_bwd_apply_group(ap, ng, s));
        TRY(mms_fb_conv_bwd_w_group(c, ng, s));
        if (l > 1) TRY(mms_fb_conv_bwd_x_group(c, ng, s));
    }
    return MMS_OK;
}

extern "C" int mms_fb3_backward_group(int ng, void* const* ws, size_t ws_bytes, const int* widths, int B, int D, int H, int W, const float* const* x,
                                      const void* const* const* params, const float* const* dout, int lddout, void* const* const* grads,
                                      hipStream_t s) {
    return fbg_backward(ng, ws, ws_bytes, widths, B, D, H, W, x, params, dout, lddout, grads, nullptr, nullptr, s);
}
extern "C" int mms_img_backward_group(int ng, void* const* ws, size_t ws_bytes, const int* widths, int B, int D, int H, int W, const float* const* x,
                                      const void* const* const* params, void* const* const* grads, const LinearBwdP* l1, const LinearBwdP* l2,
                                      hipStream_t s) {
    if (!l1 || !l2) return MMS_ERR_ARG;
    return fbg_backward(ng, ws, ws_bytes, widths, B, D, H, W, x, params, nullptr, 0, grads, l1, l2, s);
}

// ---- the reference's widths {32, 64, 128}: signatures and results as before ----
static size_t fbg_default_bytes(int B, int D, int H, int W) {
    FbPlan P;
    return fb_plan(P, FB_DEFAULT_WIDTHS, B, D, H, W) ? P.total : 0;
}
extern "C" int mms_fb_forward_group(int ng, void* const* ws, int B, int D, int H, int W, const float* const* x, const void* const* const* params,
                                    const void* const* const* buffers, float* const* out, int ldo, int train, hipStream_t s) {
    return mms_fb3_forward_group(ng, ws, fbg_default_bytes(B, D, H, W), FB_DEFAULT_WIDTHS, B, D, H, W, x, params, buffers, out, ldo, train, s);
}
extern "C" int mms_fb_backward_group(int ng, void* const* ws, int B, int D, int H, int W, const float* const* x, const void* const* const* params,
                                     const float* const* dout, int lddout, void* const* const* grads, hipStream_t s) {
    return mms_fb3_backward_group(ng, ws, fbg_default_bytes(B, D, H, W), FB_DEFAULT_WIDTHS, B, D, H, W, x, params, dout, lddout, grads, s);
}
