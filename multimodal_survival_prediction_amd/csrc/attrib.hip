// Input-gradient attribution: the data path of a backward with FROZEN BatchNorm statistics (eval mode).  Every BatchNorm is then the
// per-channel affine map y = a x + b, a = gamma / sqrt(rvar + eps), and its backward is dx = a dy: no batch sums, no weight gradients,
// nothing but workspace scratch and the caller's dx is written.  No float atomics (two calls give the same bits) and no workgroup ever
// waits for another: this is an inspection path.
//   mms_conv0_bwd_data[_group]   DenseNet121 stem: norm0 (frozen) backward + conv0 with respect to the volume
//   mms_fb3_input_grad[_group]   the 3-conv CT encoder, scalar kernels in the style of fallback.hip
// Every kernel here takes its members by value (Grp<P>) with the member on the grid's z: the single-model entry points are the ng = 1
// calls, a fold ensemble issues each launch once for its K members (mms_dn121_input_grad_group in dn_net.hip drives the DenseNet ones).
#include "common.h"
#include "dn_ops.h"
#include "fb_plan.h"

// ------------------------------------------------------------------------------------------------------
// conv0 backward-data, gather form.  A workgroup owns an 8 x 8 x 8 tile of INPUT voxels.  Conv3d(k7, s2, p3): input voxel d receives
// from output voxel (d + 3 - kd) / 2 for the taps kd of the parity of d + 3 -- 3 taps (kd = 1, 3, 5) for even d, 4 (kd = 0, 2, 4, 6)
// for odd d -- so the tile reads a 7 x 7 x 7 window of output voxels starting at (tile origin) / 2 - 1.  The window (pre-scaled by a_c)
// and the weights are staged in LDS for 32 channels at a time (all 64 would be 100 KB + 88 KB, more than the CU's 160 KB; one pass of
// 32 channels: 50 KB + 44 KB).  A wave computes one parity class (d % 2, h % 2, w % 2) at a time -- the class fixes the tap subset, so control
// flow and weight addresses are wave-uniform (LDS broadcast) -- two classes per wave, four waves.  Lane = (channel quarter, i, j): the four
// voxels (2 i + pd, 2 j + ph, 2 l + pw), l = 0..3, of one w-row of the class, for 8 of the pass's 32 channels: a row's 7 window values
// (two 16-byte LDS reads) feed 4 voxels x 3-4 taps = 12-16 FMAs.  The four channel quarters meet by two lane shuffles in a fixed order.
// VALU, not MFMA: as a GEMM window[343][64] x w[64][343] only 1 in 8 products is wanted (the parity classes), and the inspection path
// is not worth a selective-sum epilogue; the kernel is bound by its LDS reads.
// ------------------------------------------------------------------------------------------------------
#define C0D_CH 32
#define C0D_PITCH 396                                  // 49 rows x 8 floats (7 used) + 4: rows 32-byte aligned for the float4 reads
#define C0D_SMEM ((C0D_CH * C0D_PITCH + C0D_CH * 343) * 4)
__global__ __launch_bounds__(256) void conv0_bwd_data_kernel(const Grp<Conv0BwdDataP> grp) {
    extern __shared__ __attribute__((aligned(16))) float c0d_sm[];
    float* win = c0d_sm;                               // [32][396]
    float* wl = c0d_sm + C0D_CH * C0D_PITCH;           // [32][343]
    const Conv0BwdDataP& p = grp.p[blockIdx.z];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cq = lane >> 4, i = (lane >> 2) & 3, j = lane & 3;
    const int Di = p.in.D, Hi = p.in.H, Wi = p.in.W, Do = p.out.D, Ho = p.out.H, Wo = p.out.W;
    const int ntw = (Wi + 7) >> 3, nth = (Hi + 7) >> 3, ntd = (Di + 7) >> 3;
    int r = blockIdx.x;
    const int tw = r % ntw; r /= ntw;
    const int th = r % nth; r /= nth;
    const int td = r % ntd, b = r / ntd;
    const int od0 = 4 * td - 1, oh0 = 4 * th - 1, ow0 = 4 * tw - 1;
    float acc[2][4];
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int l = 0; l < 4; ++l) acc[k][l] = 0.f;

    for (int ch = 0; ch < 64 / C0D_CH; ++ch) {
        __syncthreads();                               // the previous pass's readers are done
        {
            const int c = tid & 31, cg = ch * C0D_CH + c;            // (256 % 32 == 0: a thread stages one channel)
            const float a = p.bn.gamma[cg] * (1.0f / sqrtf(p.bn.rvar[cg] + p.bn.eps));
            for (int e = tid; e < 343 * C0D_CH; e += 256) {
                const int pos = e >> 5, pd = pos / 49, ph = (pos / 7) % 7, pw = pos % 7;
                const int od = od0 + pd, oh = oh0 + ph, ow = ow0 + pw;
                float v = 0.f;
                if ((unsigned)od < (unsigned)Do && (unsigned)oh < (unsigned)Ho && (unsigned)ow < (unsigned)Wo)
                    v = a * p.dbn[((((size_t)b * Do + od) * Ho + oh) * Wo + ow) * 64 + cg];
                win[c * C0D_PITCH + (pd * 7 + ph) * 8 + pw] = v;
            }
            const float* wsrc = p.w + (size_t)ch * C0D_CH * 343;
            for (int e = tid; e < 343 * C0D_CH; e += 256) wl[e] = wsrc[e];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int cls = wave * 2 + k, pd = cls >> 2, ph = (cls >> 1) & 1, pw = cls & 1;      // wave-uniform
            for (int cc = 0; cc < 8; ++cc) {
                const int c = cq * 8 + cc;
                const float* wc = wl + c * 343;
                const float* rc = win + c * C0D_PITCH;
                for (int t = 0; t < 3 + pd; ++t) {
                    const int kd = pd ? 2 * t : 2 * t + 1, rd = i + 2 + pd - t;                  // rd in 0..6
                    for (int u = 0; u < 3 + ph; ++u) {
                        const int kh = ph ? 2 * u : 2 * u + 1, rh = j + 2 + ph - u;              // rh in 0..6
                        const float4 r0 = *(const float4*)(rc + (rd * 7 + rh) * 8), r1 = *(const float4*)(rc + (rd * 7 + rh) * 8 + 4);
                        const float* wk = wc + kd * 49 + kh * 7;
                        if (pw == 0) {                 // voxel l: sum_t row[l + 2 - t] * w[1 + 2 t]
                            const float w1 = wk[1], w3 = wk[3], w5 = wk[5];
                            acc[k][0] = fmaf(r0.z, w1, fmaf(r0.y, w3, fmaf(r0.x, w5, acc[k][0])));
                            acc[k][1] = fmaf(r0.w, w1, fmaf(r0.z, w3, fmaf(r0.y, w5, acc[k][1])));
                            acc[k][2] = fmaf(r1.x, w1, fmaf(r0.w, w3, fmaf(r0.z, w5, acc[k][2])));
                            acc[k][3] = fmaf(r1.y, w1, fmaf(r1.x, w3, fmaf(r0.w, w5, acc[k][3])));
                        } else {                       // voxel l: sum_t row[l + 3 - t] * w[2 t]
                            const float w0 = wk[0], w2 = wk[2], w4 = wk[4], w6 = wk[6];
                            acc[k][0] = fmaf(r0.w, w0, fmaf(r0.z, w2, fmaf(r0.y, w4, fmaf(r0.x, w6, acc[k][0]))));
                            acc[k][1] = fmaf(r1.x, w0, fmaf(r0.w, w2, fmaf(r0.z, w4, fmaf(r0.y, w6, acc[k][1]))));
                            acc[k][2] = fmaf(r1.y, w0, fmaf(r1.x, w2, fmaf(r0.w, w4, fmaf(r0.z, w6, acc[k][2]))));
                            acc[k][3] = fmaf(r1.z, w0, fmaf(r1.y, w2, fmaf(r1.x, w4, fmaf(r0.w, w6, acc[k][3]))));
                        }
                    }
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int cls = wave * 2 + k, pd = cls >> 2, ph = (cls >> 1) & 1, pw = cls & 1;
        const int d = 8 * td + 2 * i + pd, h = 8 * th + 2 * j + ph;
#pragma unroll
        for (int l = 0; l < 4; ++l) {
            float v = acc[k][l];
            v += __shfl_xor(v, 16, 64);                // channel quarters (0 + 1) + (2 + 3): the same order on every call
            v += __shfl_xor(v, 32, 64);
            const int w = 8 * tw + 2 * l + pw;
            if (cq == 0 && d < Di && h < Hi && w < Wi) p.dx[(((size_t)b * Di + d) * Hi + h) * Wi + w] = v;
        }
    }
}

static bool c0d_ok(const Conv0BwdDataP& p) {
    if (!p.dbn || !p.w || !p.dx || !p.bn.gamma || !p.bn.rvar || p.bn.train != 0 || p.M <= 0) return false;
    if (p.in.D < 1 || p.in.H < 1 || p.in.W < 1 || p.in.D > 2046 || p.in.H > 2046 || p.in.W > 2046) return false;
    if (p.out.D != (p.in.D + 1) / 2 || p.out.H != (p.in.H + 1) / 2 || p.out.W != (p.in.W + 1) / 2) return false;
    const long vox = (long)p.out.D * p.out.H * p.out.W;
    return p.M % vox == 0;
}
extern "C" int mms_conv0_bwd_data_group(const Conv0BwdDataP* pp, int ng, hipStream_t s) {
    Grp<Conv0BwdDataP> a;
    if (!grp_fill(a, pp, ng, 1)) return MMS_ERR_ARG;
    const Conv0BwdDataP& p = *pp;
    for (int g = 0; g < ng; ++g) {
        const Conv0BwdDataP& q = pp[g];
        if (!c0d_ok(q) || q.M != p.M || q.in.D != p.in.D || q.in.H != p.in.H || q.in.W != p.in.W) return MMS_ERR_ARG;
    }
    const long B = p.M / ((long)p.out.D * p.out.H * p.out.W);
    const long nwg = B * ((p.in.D + 7) / 8) * ((p.in.H + 7) / 8) * ((p.in.W + 7) / 8);
    if (nwg > 0x7fffffffL) return MMS_ERR_ARG;
    static std::once_flag attr_once;
    std::call_once(attr_once, [&] { hipFuncSetAttribute((const void*)conv0_bwd_data_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, C0D_SMEM); });
    MMS_LAUNCH(conv0_bwd_data_kernel, dim3((unsigned)nwg, 1, ng), dim3(256), C0D_SMEM, s, a);
    return mms_check_launch();
}
MMS_SINGLE(mms_conv0_bwd_data, Conv0BwdDataP)

// ------------------------------------------------------------------------------------------------------
// DenseNet121 head, data path with norm5 frozen: dslab[m][c] = a_c * [relu(bn(slab)) > 0] * (sum_n dout[b][n] * w[n][c]) / V.
// One thread per channel (as head_bwd_sums_kernel, dn_bwd.hip); reads dout, slab, bn, w and writes dslab only.
// ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void head_input_grad_kernel(const Grp<HeadBwdP> grp) {
    const HeadBwdP& p = grp.p[blockIdx.z];
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= p.C) return;
    float mu, rs, ga, be;
    bn_consts1(p.bn, c, mu, rs, ga, be);
    const float invV = 1.f / (float)p.V;
    for (int b = 0; b < p.B; ++b) {
        float dp = 0;
        for (int n = 0; n < p.N; ++n) dp = fmaf(p.dout[b * p.lddout + n], p.w[(size_t)n * p.C + c], dp);
        dp *= invV;
        for (int v = 0; v < p.V; ++v) {
            const size_t m = (size_t)b * p.V + v;
            const float xh = (p.slab[m * p.ld + c] - mu) * rs;
            p.dslab[m * p.ldd + c] = fmaf(ga, xh, be) > 0.f ? ga * rs * dp : 0.f;
        }
    }
}
int mms_head_input_grad_group(const HeadBwdP* pp, int ng, hipStream_t s) {          // driver-internal (dn_ops.h); grid z = member
    Grp<HeadBwdP> a;
    if (!grp_fill(a, pp, ng, 1)) return MMS_ERR_ARG;
    for (int g = 0; g < ng; ++g) {
        const HeadBwdP& q = pp[g];
        if (q.B <= 0 || q.bn.train != 0 || !q.dout || !q.slab || !q.w || !q.dslab || q.C != pp->C) return MMS_ERR_ARG;
    }
    MMS_LAUNCH(head_input_grad_kernel, dim3((pp->C + 255) / 256, 1, ng), dim3(256), 0, s, a);
    return mms_check_launch();
}

// ------------------------------------------------------------------------------------------------------
// 3-conv CT encoder: input gradient with frozen statistics (scalar kernels, a thread per (voxel, channel) as in fallback.hip)
// ------------------------------------------------------------------------------------------------------
using namespace fbplan;

// BN3 + ReLU + global average pool backward: dbn[b, v, c] = [relu(bn(y)) > 0] * dout[b, c] / V.  Grid z = member.
__global__ void fb_ig_pool_kernel(const Grp<FbPoolP> grp) {
    const FbPoolP& p = grp.p[blockIdx.z];
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= p.B * p.C) return;
    const int b = idx / p.C, c = idx % p.C;
    float mu, rs;
    bn_mean_rstd(p.bn, c, mu, rs);
    const float sc = p.bn.gamma[c] * rs, be = p.bn.beta[c], d = p.dout[(size_t)b * p.lddout + c] / (float)p.V;
    for (int v = 0; v < p.V; ++v) {
        const size_t o = ((size_t)b * p.V + v) * p.C + c;
        p.dbn[o] = bn_apply(p.y[o], mu, sc, be) > 0.f ? d : 0.f;            // (the forward's expression: the same mask bit for bit)
    }
}

// One convolution's backward-data.  p.dy: the masked gradient at the output BatchNorm's output [B*out][Cout]; bn_out: that BatchNorm
// (frozen): dy_raw = a * p.dy.  Gather over the <= 8 (output voxel, tap) pairs that read this input voxel, then the input's own
// BatchNorm + ReLU mask (p.has_bn; the first layer reads the raw volume, Cin = 1: no mask) -> p.dbn_in [B*in][Cin].  Grid z = member.
struct FbIgConvArgs { Grp<FbConvP> c; BnSrc bn_out[MMS_MAX_GROUP]; };
static_assert(sizeof(FbIgConvArgs) <= 4096, "ten members by value must fit the kernel-argument segment");
__global__ __launch_bounds__(256) void fb_ig_conv_kernel(const FbIgConvArgs args) {
    __shared__ float a_out[128];
    const FbConvP& p = args.c.p[blockIdx.z];
    const BnSrc& bn_out = args.bn_out[blockIdx.z];
    if (threadIdx.x < p.Cout) {
        float mu, rs;
        bn_mean_rstd(bn_out, threadIdx.x, mu, rs);
        a_out[threadIdx.x] = bn_out.gamma[threadIdx.x] * rs;
    }
    __syncthreads();
    const int vox_in = p.in.D * p.in.H * p.in.W, Min = p.B * vox_in;
    const int VB = 256 / p.Cin, cin = threadIdx.x % p.Cin, v = threadIdx.x / p.Cin, m = blockIdx.x * VB + v;
    if (m >= Min) return;
    const int b = m / vox_in, r = m % vox_in;
    const int id = r / (p.in.H * p.in.W), ih = (r / p.in.W) % p.in.H, iw = r % p.in.W;
    float da = 0.f;
    for (int td = 0; td < 3; ++td) {
        const int nd = id + 1 - td;
        if (nd < 0 || (nd & 1) || (nd >> 1) >= p.out.D) continue;
        for (int th = 0; th < 3; ++th) {
            const int nh = ih + 1 - th;
            if (nh < 0 || (nh & 1) || (nh >> 1) >= p.out.H) continue;
            for (int tw = 0; tw < 3; ++tw) {
                const int nw = iw + 1 - tw;
                if (nw < 0 || (nw & 1) || (nw >> 1) >= p.out.W) continue;
                const size_t mo = ((size_t)(b * p.out.D + (nd >> 1)) * p.out.H + (nh >> 1)) * p.out.W + (nw >> 1);
                const int tap = (td * 3 + th) * 3 + tw;
                const float* dyr = p.dy + mo * p.Cout;
                for (int co = 0; co < p.Cout; ++co) da = fmaf(dyr[co] * a_out[co], p.w[((size_t)co * p.Cin + cin) * 27 + tap], da);
            }
        }
    }
    if (p.has_bn) {
        float mu, rs;
        bn_mean_rstd(p.bn, cin, mu, rs);
        if (!(bn_apply(p.x[(size_t)m * p.Cin + cin], mu, p.bn.gamma[cin] * rs, p.bn.beta[cin]) > 0.f)) da = 0.f;
    }
    p.dbn_in[(size_t)m * p.Cin + cin] = da;
}

#define TRY(x) do { int rc_ = (x); if (rc_ != MMS_OK) return rc_; } while (0)
// The 3-conv encoder's input gradient for ng members in lock-step: four launches, each carrying every member's block.
extern "C" int mms_fb3_input_grad_group(int ng, void* const* ws, size_t ws_bytes, const int* widths, int B, int D, int H, int W, const float* const* x,
                                        const void* const* const* params, const void* const* const* buffers, const float* const* dout, int lddout,
                                        float* const* dx, hipStream_t s) {
    FbPlan P;
    if (ng < 1 || ng > MMS_MAX_GROUP || !ws || !x || !params || !buffers || !dout || !dx) return MMS_ERR_ARG;
    if (!fb_plan(P, widths, B, D, H, W) || ws_bytes != P.total || lddout < P.C[3]) return MMS_ERR_ARG;
    for (int l = 0; l < 3; ++l)
        if (256 % widths[l]) return MMS_ERR_ARG;                             // a thread per (voxel, channel) of a 256-thread workgroup
    for (int g = 0; g < ng; ++g) {
        if (!ws[g] || !x[g] || !params[g] || !buffers[g] || !dout[g] || !dx[g]) return MMS_ERR_ARG;
        for (int i = 0; i < 12; ++i)
            if (!params[g][i]) return MMS_ERR_ARG;
        for (int i = 0; i < 9; ++i)
            if (!buffers[g][i]) return MMS_ERR_ARG;
    }
    if ((long)B * P.C[3] > 0x7fffffffL) return MMS_ERR_ARG;
    Grp<FbPoolP> pl{};
    pl.zdim = 1;
    for (int g = 0; g < ng; ++g) {
        const float* const* prm = (const float* const*)params[g];
        FbPoolP& q = pl.p[g];
        q.y = at<float>(ws[g], P.y[3]); q.C = P.C[3]; q.V = P.M[3] / B; q.B = B; q.bn = fb_bn(ws[g], P, 3, prm, buffers[g], 0);
        q.dout = dout[g]; q.lddout = lddout; q.dbn = at<float>(ws[g], P.dbn[3]);
    }
    MMS_LAUNCH(fb_ig_pool_kernel, dim3((B * P.C[3] + 255) / 256, 1, ng), dim3(256), 0, s, pl);
    TRY(mms_check_launch());
    for (int l = 3; l >= 1; --l) {
        FbIgConvArgs a{};
        a.c.zdim = 1;
        for (int g = 0; g < ng; ++g) {
            const float* const* prm = (const float* const*)params[g];
            FbConvP& c = a.c.p[g];
            c.x = l == 1 ? x[g] : at<float>(ws[g], P.y[l - 1]); c.Cin = P.C[l - 1]; c.in = P.g[l - 1]; c.out = P.g[l]; c.B = B;
            c.has_bn = l > 1; if (l > 1) c.bn = fb_bn(ws[g], P, l - 1, prm, buffers[g], 0);
            c.w = prm[4 * (l - 1)]; c.Cout = P.C[l]; c.dy = at<float>(ws[g], P.dbn[l]);
            c.dbn_in = l == 1 ? dx[g] : at<float>(ws[g], P.dbn[l - 1]);
            a.bn_out[g] = fb_bn(ws[g], P, l, prm, buffers[g], 0);
        }
        const int VB = 256 / P.C[l - 1];
        MMS_LAUNCH(fb_ig_conv_kernel, dim3((P.M[l - 1] + VB - 1) / VB, 1, ng), dim3(256), 0, s, a);
        TRY(mms_check_launch());
    }
    return MMS_OK;
}
extern "C" int mms_fb3_input_grad(void* ws, size_t ws_bytes, const int* widths, int B, int D, int H, int W, const float* x, const void* const* params_,
                                  const void* const* buffers, const float* dout, int lddout, float* dx, hipStream_t s) {
    return mms_fb3_input_grad_group(1, &ws, ws_bytes, widths, B, D, H, W, &x, &params_, &buffers, &dout, lddout, &dx, s);
}
