// Workspace plan of the 3-conv CT encoder drivers, shared by the single-model path (fallback.hip) and the lock-step path (fb_group.hip):
// ONE definition, so that the running-statistics table mms_fb3_init writes and the regions both drivers read cannot drift apart.
// Channel widths are a parameter: C[0] = 1 (the volume), C[1..3] = the three convolutions' output channels, each a multiple of 16 in
// 16..128 (the BatchNorm constants of a layer's input live in 3 x 128 floats of LDS; rows of dy are read as float4).
#pragma once
#include "common.h"

namespace fbplan {
struct FbPlan {
    int B; int C[4]; Dims3 g[4]; int M[4];
    size_t y[4], dy[4], dbn[4], st[4], bb[4], tab_bn, stats_begin, stats_end, total;
};
inline size_t al(size_t x) { return (x + 255) & ~(size_t)255; }
inline bool fb_widths_ok(const int* widths) {
    if (!widths) return false;
    for (int l = 0; l < 3; ++l)
        if (widths[l] < 16 || widths[l] > 128 || widths[l] % 16 != 0) return false;
    return true;
}
inline bool fb_plan(FbPlan& P, const int* widths, int B, int D, int H, int W) {
    if (!fb_widths_ok(widths) || B <= 0 || D < 1 || H < 1 || W < 1) return false;
    P.B = B; P.g[0] = Dims3{D, H, W};
    P.C[0] = 1;
    for (int l = 1; l < 4; ++l) P.C[l] = widths[l - 1];
    for (int l = 1; l < 4; ++l) P.g[l] = Dims3{(P.g[l - 1].D + 1) / 2, (P.g[l - 1].H + 1) / 2, (P.g[l - 1].W + 1) / 2};
    for (int l = 0; l < 4; ++l) P.M[l] = B * P.g[l].D * P.g[l].H * P.g[l].W;
    size_t o = 0;
    auto take = [&](size_t n) { size_t r = o; o = al(o + n); return r; };
    for (int l = 1; l < 4; ++l) { P.y[l] = take((size_t)P.M[l] * P.C[l] * 4); P.dy[l] = take((size_t)P.M[l] * P.C[l] * 4); P.dbn[l] = take((size_t)P.M[l] * P.C[l] * 4); }
    P.tab_bn = take(sizeof(BnRunEntry) * 3);
    P.stats_begin = o;
    for (int l = 1; l < 4; ++l) { P.st[l] = take(2 * 128 * 8); P.bb[l] = take(2 * 128 * 8); }
    P.stats_end = o; P.total = o;
    return true;
}
template <class T> inline T* at(void* ws, size_t off) { return (T*)((char*)ws + off); }
inline BnSrc fb_bn(void* ws, const FbPlan& P, int l, const float* const* prm, const void* const* buf, int train) {
    BnSrc b;
    b.nrep = 0; b.rep_stride = 0;
    b.sum = at<double>(ws, P.st[l]); b.sumsq = b.sum + 128;
    b.rmean = buf ? (const float*)buf[3 * (l - 1)] : nullptr; b.rvar = buf ? (const float*)buf[3 * (l - 1) + 1] : nullptr;
    b.gamma = prm[4 * (l - 1) + 2]; b.beta = prm[4 * (l - 1) + 3];
    b.inv_count = 1.f / (float)P.M[l]; b.eps = 1e-5f; b.train = train;
    return b;
}
constexpr int FB_DEFAULT_WIDTHS[3] = {32, 64, 128};      // final_multimodal.py:75-86
}  // namespace fbplan
