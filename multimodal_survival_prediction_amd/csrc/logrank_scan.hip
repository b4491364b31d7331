// Cut-point scan of the two-group log-rank statistic on Q problems (include/mmsurv.h: LogrankScanP).
//
// All problems share n patient positions in time-descending order and the labels; a problem is one int32 rank vector over those
// positions and one sorted list of cut ranks (position i is in the high group of cut c iff rank[i] >= cut[c]).  With G_i the number of
// high-group members among positions 0..i (the high group's patients at risk at position i's time when i ends a tie group) and D the
// high group's events,
//     U = D - sum_i h_i G_i,      V = sum_i c_i G_i (i + 1 - G_i),      chi2 = U^2 / V  (0 when V <= 0),
// where h_i = d_u / n_u and c_i = d_u (n_u - d_u) / (n_u^2 (n_u - 1)) (0 when n_u = 1) stand at the last position of event time u's tie
// group and are 0 elsewhere (the host computes them in fp64 from the labels).  U is observed - expected events of the high group, V the hypergeometric
// variance of survival_stats.logrank_test.
//
// One workgroup = one problem; lane = cut.  The problem's rank vector, the position flags and the coefficients are staged through LDS in
// tiles of LR_TILE positions (20 bytes a position); a thread walks the positions: the position's {rank, flags} is one broadcast LDS read,
// a position costs every lane one compare, one select and one integer add -- G and D are the two 16-bit halves of one register
// (n <= 65535) -- and the fp64 terms run only at the positions that end a tie group with events (a wave-uniform branch).  Every
// (problem, cut) is owned by one thread and written with plain stores; the maximum over a problem's cuts is an in-block reduction in a
// fixed order.  No atomics; a problem's bits depend on its own rank vector and cut list only.
#include "common.h"

#define LR_THREADS 256
#define LR_TILE 512     // positions per LDS stage

struct LrAcc { unsigned acc; double e, v; };     // acc = G | D << 16

__device__ __forceinline__ void lr_step(LrAcc& t, int2 rf, const double2* hc, int pos, int thr) {
    const int f = __builtin_amdgcn_readfirstlane(rf.y);
    t.acc += rf.x >= thr ? 1u + ((unsigned)(f & 1) << 16) : 0u;
    if (f & 2) {
        const double2 k = *hc;
        const double g = (double)(t.acc & 0xffffu);
        t.e = fma(k.x, g, t.e);
        t.v = fma(k.y * g, (double)(pos + 1) - g, t.v);
    }
}

__global__ __launch_bounds__(LR_THREADS) void logrank_scan_kernel(const LogrankScanP a) {
    __shared__ int2 sh_rf[LR_TILE];
    __shared__ double2 sh_hc[LR_TILE];
    __shared__ double sh_x[LR_THREADS];
    __shared__ int sh_i[LR_THREADS];
    const int q = blockIdx.x, tid = threadIdx.x;
    const int s = a.cset ? a.cset[q] : q;
    const int c0 = a.coff[s], C = a.coff[s + 1] - c0;
    const int at = a.at ? a.at[s] : -1;
    const int* rank = a.rank + (size_t)q * a.ldr;
    const int* cut = a.cut + c0;
    const double2* coef = (const double2*)a.coef;
    const int n = a.n;
    const bool one_tile = n <= LR_TILE;
    double best = -1.0;                                  // (every chi2 is >= 0: the first cut of a thread always wins)
    int besti = 0x7fffffff;
    for (int cb = 0; cb < C; cb += LR_THREADS) {
        const bool wave_on = cb + (tid & ~63) < C;       // this wave has a cut in the chunk (wave-uniform)
        const int c = cb + tid;
        const bool cv = c < C;
        const int thr = cv ? cut[c] : 0x7fffffff;        // an absent cut's lane keeps an empty high group; nothing of it is stored
        LrAcc t{0u, 0.0, 0.0};
        for (int t0 = 0; t0 < n; t0 += LR_TILE) {
            const int m = min(LR_TILE, n - t0);
            if (!one_tile || cb == 0) {                  // (a single tile stays in LDS for every chunk of cuts)
                if (!one_tile) __syncthreads();          // the previous tile's readers are done
                for (int i = tid; i < m; i += LR_THREADS) {
                    sh_rf[i] = make_int2(rank[t0 + i], a.pflag[t0 + i]);
                    sh_hc[i] = coef[t0 + i];
                }
                __syncthreads();
            }
            if (!wave_on) continue;
            int i = 0;
            for (; i + 4 <= m; i += 4) {
                const int2 r0 = sh_rf[i], r1 = sh_rf[i + 1], r2 = sh_rf[i + 2], r3 = sh_rf[i + 3];
                lr_step(t, r0, sh_hc + i, t0 + i, thr);
                lr_step(t, r1, sh_hc + i + 1, t0 + i + 1, thr);
                lr_step(t, r2, sh_hc + i + 2, t0 + i + 2, thr);
                lr_step(t, r3, sh_hc + i + 3, t0 + i + 3, thr);
            }
            for (; i < m; ++i) lr_step(t, sh_rf[i], sh_hc + i, t0 + i, thr);
        }
        const double u = (double)(t.acc >> 16) - t.e, v = t.v;
        const double x = v > 0.0 ? u * u / v : 0.0;
        if (cv) {
            if (a.U) {
                const size_t o = (size_t)q * a.ldo + c;
                a.U[o] = u; a.V[o] = v; a.n_high[o] = (int)(t.acc & 0xffffu); a.d_high[o] = (int)(t.acc >> 16);
            }
            if (c == at) a.chi2_at[q] = x;
            if (x > best) { best = x; besti = c; }       // ascending c: the smallest index keeps a tie
        }
    }
    sh_x[tid] = best; sh_i[tid] = besti;
    __syncthreads();
    for (int w = LR_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w) {
            const double x = sh_x[tid + w];
            const int j = sh_i[tid + w];
            if (x > sh_x[tid] || (x == sh_x[tid] && j < sh_i[tid])) { sh_x[tid] = x; sh_i[tid] = j; }
        }
        __syncthreads();
    }
    if (tid == 0) {
        const bool any = sh_i[0] != 0x7fffffff;
        a.chi2_max[q] = any ? sh_x[0] : 0.0;
        a.arg_max[q] = any ? sh_i[0] : -1;
        if (at < 0 || at >= C) a.chi2_at[q] = 0.0;
    }
}

extern "C" int mms_logrank_scan(const LogrankScanP* p, hipStream_t s) {
    if (!p || !p->rank || !p->pflag || !p->coef || !p->coff || !p->cut || !p->chi2_max || !p->arg_max || !p->chi2_at) return MMS_ERR_ARG;
    if (p->n < 1 || p->n > MMS_LRSCAN_MAX_N || p->ldr < p->n || p->Q < 0 || p->Q > MMS_LRSCAN_MAX_Q) return MMS_ERR_ARG;
    if (p->maxc < 0 || p->maxc > MMS_LRSCAN_MAX_C) return MMS_ERR_ARG;
    const bool tab = p->U || p->V || p->n_high || p->d_high;
    if (tab && (!p->U || !p->V || !p->n_high || !p->d_high || p->ldo < p->maxc)) return MMS_ERR_ARG;
    if (((uintptr_t)p->rank & 3) || ((uintptr_t)p->pflag & 3) || ((uintptr_t)p->coff & 3) || ((uintptr_t)p->cut & 3)) return MMS_ERR_ARG;
    if (((uintptr_t)p->cset & 3) || ((uintptr_t)p->at & 3) || ((uintptr_t)p->arg_max & 3)) return MMS_ERR_ARG;
    if (((uintptr_t)p->n_high & 3) || ((uintptr_t)p->d_high & 3)) return MMS_ERR_ARG;
    if (((uintptr_t)p->coef & 15) || ((uintptr_t)p->chi2_max & 7) || ((uintptr_t)p->chi2_at & 7)) return MMS_ERR_ARG;
    if (((uintptr_t)p->U & 7) || ((uintptr_t)p->V & 7)) return MMS_ERR_ARG;
    if (p->Q == 0) return MMS_OK;
    MMS_LAUNCH(logrank_scan_kernel, dim3(p->Q), dim3(LR_THREADS), 0, s, *p);
    return mms_check_launch();
}
