// IPCW Brier score and cumulative/dynamic AUC sums of M models at H horizons under R multiplicity rows (include/mmsurv.h: TdMetricsP).
//
// All replicates share n patient positions in time-ascending order (events before censorings at equal times) and the labels; a
// replicate is one int8 multiplicity row w.  One workgroup = one replicate.
//
// Phase A, once per replicate.  The row is staged in LDS as {w, event, last-of-its-time-group} words and summed (W).  Wave 0 then walks
// the positions once: the running integer sums give, at the last position of the group of time u, S_a (the w at t >= u), d_u (the w
// of its events), n_u = S_a - d_u and S_b (the w at t > u), and the two product-limit estimates advance by ONE division each,
//     KM *= n_u / S_a  (S_a > 0),      G *= S_b / n_u  (n_u > 0),
// in ascending time order -- the order of the definition, so both are the literal products.  The walk leaves G(t_i-) at every position
// (G changes only at a group's end) and lane h keeps G and KM as they stand when the walk passes hcut[h].  All threads then turn
// G(t_i-) into the case weight w_i e_i / G(t_i-), and one wave sums, lane = horizon, the cases' weight and the controls' w in time order.
//
// The case weights are finite and G(tau) > 0 whenever a control is drawn:  G(t-) is the product of S_b(v) / n_v over the times v < t.
// A drawn patient j (w_j > 0) with t_j > v is counted in S_b(v), so S_b(v) >= w_j > 0, and n_v >= S_b(v) (n_v - S_b(v) is the w of the
// censorings at v): every factor of G(t_j-) is a quotient of two positive integers.  A drawn case i has its weight 1 / G(t_i-) from
// exactly those factors, and a drawn control j at horizon tau has tau < t_j, so G(tau) is a product of a subset of them.  (A position
// with w = 0 may see G(t-) = 0: its weight is a select of 0, never 0 / 0.)
//
// Phase B, lane = horizon, one wave per model (two models per wave, one in each half, when H <= 32); the block's waves stride over
// the models.  A lane walks its model's positions in risk-ascending order: the position's case weight and w are LDS reads (one address
// per model: a broadcast), the lane classifies the position by comparing its index with its own hcut, the Brier terms read the lane's
// element of the position's surv line (H contiguous doubles), and the AUC keeps the controls' w BELOW the current group of equal
// risks: at a group's last position it commits  case_group * (below + group_controls / 2)  -- O(n) per (replicate, model, horizon)
// instead of the O(n^2) pair sum.  The controls' w is an integer and stays one.  Every lane owns its outputs: plain stores, no atomics;
// nothing a lane computes depends on which other models or replicates are in the launch.
#include "common.h"

#define TD_THREADS 256
#define TD_WAVES (TD_THREADS / 64)
#define TD_EVENT 0x100
#define TD_TLAST 0x200

static int td_pad4(int n) { return (n + 3) & ~3; }
static size_t td_lds_bytes(int n) { return sizeof(int) * ((size_t)td_pad4(n) + TD_WAVES) + sizeof(double) * ((size_t)n + MMS_TD_MAX_H); }

// one position of the product-limit walk (wave-uniform but for the capture of the lane's horizon)
struct TdWalk { int before, run, d; double g, km, gh, kmh; };   // the w before the current time group, up to here and of the group's events

__device__ __forceinline__ void td_walk_step(TdWalk& t, int f, int i, int W, int hc) {
    const int wi = f & 0xff;
    t.run += wi;
    t.d += f & TD_EVENT ? wi : 0;
    if (f & TD_TLAST) {
        const int sa = W - t.before, nu = sa - t.d, sb = W - t.run;
        if (sa > 0) t.km *= (double)nu / (double)sa;
        if (nu > 0) t.g *= (double)sb / (double)nu;
        if (hc == i + 1) { t.gh = t.g; t.kmh = t.km; }
        t.before = t.run; t.d = 0;
    }
}

// one position of a lane's walk in risk order: q = the order word, p its position, S / cp / f the lane's surv element, the position's
// case weight and its staged word (all read whatever the side: selects, no branch), hcl the lane's hcut
struct TdRisk { double bc, bk, num, gcase; int below, gctrl; };

__device__ __forceinline__ void td_risk_step(TdRisk& t, int q, int p, double S, double cp, int f, int hcl) {
    const bool early = p < hcl;
    const double cc = early ? cp : 0.0, u = 1.0 - S;
    const int wk = early ? 0 : f & 0xff;
    t.bc = fma(cc, S * S, t.bc);
    t.bk = fma((double)wk, u * u, t.bk);
    t.gcase += cc; t.gctrl += wk;
    if (q & 1) {
        t.num = fma(t.gcase, (double)t.below + 0.5 * (double)t.gctrl, t.num);
        t.below += t.gctrl; t.gcase = 0.0; t.gctrl = 0;
    }
}

__global__ __launch_bounds__(TD_THREADS) void td_metrics_kernel(const TdMetricsP a) {
    extern __shared__ int4 td_lds[];
    const int n = a.n, H = a.H, M = a.M, n4 = (n + 3) & ~3;
    int* wf = (int*)td_lds;                 // [n4] w | TD_EVENT | TD_TLAST, zero words past n (16-byte reads: four positions a read)
    int* part = wf + n4;                    // [TD_WAVES] the waves' sums of w
    double* hG = (double*)(part + TD_WAVES);// [MMS_TD_MAX_H] G(tau_h)
    double* cw = hG + MMS_TD_MAX_H;         // [n] G(t_i-), then the case weight w_i e_i / G(t_i-)
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const signed char* w = a.w + (size_t)r * a.ldw;
    int s = 0;
    for (int i = tid; i < n4; i += TD_THREADS) {
        int f = 0;
        if (i < n) {
            const int wi = w[i] & 0xff;
            const bool last = i == n - 1 || a.trank[i + 1] != a.trank[i];
            f = wi | (a.event[i] != 0 ? TD_EVENT : 0) | (last ? TD_TLAST : 0);
            s += wi;
        }
        wf[i] = f;
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) part[wave] = s;
    __syncthreads();
    int W = 0;
    for (int i = 0; i < TD_WAVES; ++i) W += part[i];
    const int hc = lane < H ? a.hcut[lane] : -1;         // (an absent horizon's lane has neither cases nor stores)
    const size_t oh = (size_t)r * H + lane;
    if (wave == 0) {
        TdWalk t{0, 0, 0, 1.0, 1.0, 1.0, 1.0};
        int4 f = *(const int4*)wf;
        for (int i = 0; i < n; i += 4) {                 // (a padding word has w = 0 and no flag: its step changes nothing)
            const int4 c = f;
            if (i + 4 < n) f = *(const int4*)(wf + i + 4);               // the next four positions are on their way during these four
            const int f0 = __builtin_amdgcn_readfirstlane(c.x), f1 = __builtin_amdgcn_readfirstlane(c.y);
            const int f2 = __builtin_amdgcn_readfirstlane(c.z), f3 = __builtin_amdgcn_readfirstlane(c.w);
            const double g0 = t.g;
            td_walk_step(t, f0, i, W, hc);
            const double g1 = t.g;
            td_walk_step(t, f1, i + 1, W, hc);
            const double g2 = t.g;
            td_walk_step(t, f2, i + 2, W, hc);
            const double g3 = t.g;
            td_walk_step(t, f3, i + 3, W, hc);
            if (lane < 4 && i + lane < n) cw[i + lane] = lane == 0 ? g0 : lane == 1 ? g1 : lane == 2 ? g2 : g3;
        }
        if (lane < H) { a.G[oh] = t.gh; a.km[oh] = t.kmh; }
        hG[lane] = t.gh;
    }
    __syncthreads();
    for (int i = tid; i < n; i += TD_THREADS) {
        const int f = wf[i], wi = f & 0xff;
        cw[i] = (f & TD_EVENT) && wi ? (double)wi / cw[i] : 0.0;
    }
    __syncthreads();
    if (wave == TD_WAVES - 1 && lane < H) {
        double c = 0.0;
        int k = 0;
#pragma unroll 4
        for (int i = 0; i < n; ++i) {
            const double ci = cw[i];                     // (read whatever the side: a broadcast, and no branch)
            const int wi = wf[i] & 0xff;
            c += i < hc ? ci : 0.0;
            k += i >= hc ? wi : 0;
        }
        a.wcase[oh] = c; a.wctrl[oh] = (double)k;
    }
    const int hw = H <= 32 ? 32 : 64, per = 64 / hw;     // lanes and models of a wave
    const int slot = lane / hw, h = lane - slot * hw;
    const bool hv = h < H;
    const int hcl = a.hcut[hv ? h : 0];
    const double ghl = hG[hv ? h : 0];
    for (int m0 = wave * per; m0 < M; m0 += TD_WAVES * per) {
        const int m = m0 + slot, mm = min(m, M - 1);     // (an absent model's half repeats the last one and stores nothing)
        const int* ro = a.rord + (size_t)mm * a.ldr;
        const double* sv = a.surv + (size_t)mm * n * a.ldh + (hv ? h : 0);
        TdRisk t{0.0, 0.0, 0.0, 0.0, 0, 0};
        const unsigned last = (unsigned)(n - 1);
        int k = 0;
        int q0 = ro[0], q1 = ro[min(1, n - 1)], q2 = ro[min(2, n - 1)], q3 = ro[min(3, n - 1)];
        for (; k + 4 <= n; k += 4) {                     // four positions a round: their loads are issued together, the next round's order words ahead
            const int c0 = q0, c1 = q1, c2 = q2, c3 = q3;
            const int kn = k + 4;
            q0 = ro[min(kn, n - 1)]; q1 = ro[min(kn + 1, n - 1)]; q2 = ro[min(kn + 2, n - 1)]; q3 = ro[min(kn + 3, n - 1)];
            const int p0 = (int)min((unsigned)c0 >> 1, last), p1 = (int)min((unsigned)c1 >> 1, last);
            const int p2 = (int)min((unsigned)c2 >> 1, last), p3 = (int)min((unsigned)c3 >> 1, last);
            const double S0 = sv[(size_t)p0 * a.ldh], S1 = sv[(size_t)p1 * a.ldh], S2 = sv[(size_t)p2 * a.ldh], S3 = sv[(size_t)p3 * a.ldh];
            const double w0 = cw[p0], w1 = cw[p1], w2 = cw[p2], w3 = cw[p3];
            const int i0 = wf[p0], i1 = wf[p1], i2 = wf[p2], i3 = wf[p3];
            td_risk_step(t, c0, p0, S0, w0, i0, hcl);
            td_risk_step(t, c1, p1, S1, w1, i1, hcl);
            td_risk_step(t, c2, p2, S2, w2, i2, hcl);
            td_risk_step(t, c3, p3, S3, w3, i3, hcl);
        }
        for (; k < n; ++k) {
            const int c = ro[k], p = (int)min((unsigned)c >> 1, last);
            td_risk_step(t, c, p, sv[(size_t)p * a.ldh], cw[p], wf[p], hcl);
        }
        if (hv && m < M) {
            const size_t o = ((size_t)r * M + m) * H + h;
            a.brier[o] = (t.bc + (t.below > 0 ? t.bk / ghl : 0.0)) / (double)W;
            a.auc_num[o] = t.num;
        }
    }
}

extern "C" int mms_td_metrics(const TdMetricsP* p, hipStream_t s) {
    if (!p || !p->trank || !p->event || !p->hcut || !p->rord || !p->surv || !p->w) return MMS_ERR_ARG;
    if (!p->G || !p->km || !p->wcase || !p->wctrl || !p->brier || !p->auc_num) return MMS_ERR_ARG;
    if (p->n < 1 || p->n > MMS_TD_MAX_N || p->H < 1 || p->H > MMS_TD_MAX_H || p->M < 1 || p->M > MMS_TD_MAX_M) return MMS_ERR_ARG;
    if (p->R < 0 || p->R > MMS_TD_MAX_R || p->ldr < p->n || p->ldh < p->H || p->ldw < p->n) return MMS_ERR_ARG;
    if (((uintptr_t)p->trank & 3) || ((uintptr_t)p->event & 3) || ((uintptr_t)p->hcut & 3) || ((uintptr_t)p->rord & 3)) return MMS_ERR_ARG;
    if (((uintptr_t)p->surv & 7) || ((uintptr_t)p->G & 7) || ((uintptr_t)p->km & 7) || ((uintptr_t)p->wcase & 7)) return MMS_ERR_ARG;
    if (((uintptr_t)p->wctrl & 7) || ((uintptr_t)p->brier & 7) || ((uintptr_t)p->auc_num & 7)) return MMS_ERR_ARG;
    if (p->R == 0) return MMS_OK;
    MMS_LAUNCH(td_metrics_kernel, dim3(p->R), dim3(TD_THREADS), td_lds_bytes(p->n), s, *p);
    return mms_check_launch();
}
