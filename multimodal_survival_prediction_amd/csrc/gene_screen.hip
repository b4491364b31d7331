// Univariate Cox score screen of G genes on P problems (include/mmsurv.h: GeneScreenP).
//
// A problem is an ordered list of patient rows (time descending; a fold's training patients, or a bootstrap resample of them: a row
// listed twice is a tie).  With S1_k = the running column sum over the list's first k + 1 rows, the score test of gene j at beta = 0 is
//     U_j = sum_k a_k x_kj,      V_j = sum_k b_k x_kj^2 - sum_k q_k S1_kj^2,
// where a, b, q depend on the labels only (the host computes them in fp64).  One workgroup = one problem x 64 consecutive genes: lane =
// gene, so a wave reads 256 consecutive bytes of one patient row per step; wave = one of GS_SEG contiguous row segments of the list.
// The running sum is not scanned across segments: a segment thread keeps its LOCAL sum s and accumulates sum q, sum q s, sum q s^2; with
// the segment's entry offset o (the sum of the segments before it, known once every segment is done)
//     sum q (o + s)^2 = o^2 sum q + 2 o sum q s + sum q s^2,
// combined through LDS by the workgroup's first wave in segment order.  One pass over the rows, fp64 accumulators, no atomics: every
// (problem, gene) is owned by one thread of one workgroup and written with a plain store.  A problem's segments depend on its own
// length only, so its bits do not depend on which problems share the launch or where it stands among them.
//
// Grid: x = problem (fastest), y = gene strip.  Workgroups that are resident together then work on a few strips of many problems, all
// of which read the same N x 256 B of x: the strip stays in every XCD's L2 while it is in use.
#include "common.h"

#define GS_SEG 4        // row segments = waves per workgroup
#define GS_ROWS 4       // rows in flight per thread

struct GsAcc { double s, u, vb, q0, q1, q2; };

__device__ __forceinline__ void gs_step(GsAcc& t, float xf, const double* c) {
    const double x = (double)xf, a = c[0], b = c[1], q = c[2];
    t.s += x;
    t.u = fma(a, x, t.u);
    t.vb = fma(b * x, x, t.vb);
    const double qs = q * t.s;
    t.q0 += q;
    t.q1 += qs;
    t.q2 = fma(qs, t.s, t.q2);
}

__global__ __launch_bounds__(64 * GS_SEG) void gene_screen_kernel(const GeneScreenP a) {
    __shared__ double sh[GS_SEG][6][64];
    const int lane = threadIdx.x & 63, seg = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int p = blockIdx.x, g = blockIdx.y * 64 + lane;
    const bool gv = g < a.G;
    const int o0 = a.off[p], n = a.off[p + 1] - o0;
    const int L = (n + GS_SEG - 1) / GS_SEG;
    const int k0 = min(n, seg * L), k1 = min(n, k0 + L);
    const float* xc = a.x + (gv ? g : 0);               // an absent gene's lane re-reads column 0; its result is never stored
    const int* row = a.row + o0;
    const double* coef = a.coef + 3 * (size_t)o0;
    GsAcc t{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int k = k0;
    for (; k + GS_ROWS <= k1; k += GS_ROWS) {           // (k, row[k], coef[k] are wave-uniform: scalar loads)
        float xv[GS_ROWS];
#pragma unroll
        for (int i = 0; i < GS_ROWS; ++i) xv[i] = xc[(size_t)row[k + i] * a.ld];
#pragma unroll
        for (int i = 0; i < GS_ROWS; ++i) gs_step(t, xv[i], coef + 3 * (size_t)(k + i));
    }
    for (; k < k1; ++k) gs_step(t, xc[(size_t)row[k] * a.ld], coef + 3 * (size_t)k);
    sh[seg][0][lane] = t.s; sh[seg][1][lane] = t.u; sh[seg][2][lane] = t.vb;
    sh[seg][3][lane] = t.q0; sh[seg][4][lane] = t.q1; sh[seg][5][lane] = t.q2;
    __syncthreads();
    if (seg != 0 || !gv) return;
    double o = 0.0, u = 0.0, vb = 0.0, vq = 0.0;
#pragma unroll
    for (int w = 0; w < GS_SEG; ++w) {
        u += sh[w][1][lane];
        vb += sh[w][2][lane];
        vq += o * o * sh[w][3][lane] + 2.0 * o * sh[w][4][lane] + sh[w][5][lane];
        o += sh[w][0][lane];
    }
    a.U[(size_t)p * a.G + g] = u;
    a.V[(size_t)p * a.G + g] = vb - vq;
}

extern "C" int mms_gene_screen(const GeneScreenP* p, hipStream_t s) {
    if (!p || !p->x || !p->off || !p->row || !p->coef || !p->U || !p->V) return MMS_ERR_ARG;
    if (p->P < 0 || p->G < 1 || p->ld < p->G || p->N < 1 || p->G > MMS_GENE_SCREEN_MAX_G) return MMS_ERR_ARG;
    if (((uintptr_t)p->x & 3) || ((uintptr_t)p->off & 3) || ((uintptr_t)p->row & 3)) return MMS_ERR_ARG;
    if (((uintptr_t)p->coef & 7) || ((uintptr_t)p->U & 7) || ((uintptr_t)p->V & 7)) return MMS_ERR_ARG;
    if (p->P == 0) return MMS_OK;
    MMS_LAUNCH(gene_screen_kernel, dim3(p->P, (p->G + 63) / 64), dim3(64 * GS_SEG), 0, s, *p);
    return mms_check_launch();
}
