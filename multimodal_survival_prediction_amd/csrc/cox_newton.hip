// Multivariable Cox regression by Newton-Raphson: R multiplicity rows x S covariate subsets, one fit each (include/mmsurv.h: CoxNewtonP).
//
// One workgroup = one problem q = r * S + s.  The row is staged in LDS once as {w, event, last-of-its-time-group} words; everything
// after that is a sequence of EVALUATIONS at a point beta (each gives l, g and I there) steered by the solver of the header comment.
//
// An evaluation.  (1) All threads: eta_k = sum_a x_ka beta_a over the mask's columns (ascending a, one fma each) into LDS and the
// maximum over the drawn rows (a maximum is exact, so its tree needs no fixed order).  (2) All threads: r_k = w_k exp(eta_k - max)
// replaces eta_k in LDS (0 exactly for w = 0: a select) and sum w e (eta - max) is summed thread -> wave -> block in a fixed order.
// (3) The walk: each of the p (p + 1) / 2 pairs a <= b has a lane.  The lane walks the n positions in time-descending order carrying
// S0, S1_a, S1_b and S2_ab itself -- redundantly among the lanes, so the walk needs no cross-lane exchange -- and commits
// d (S2_ab / S0 - S1_a S1_b / S0^2) at every tie-group end with events; a diagonal lane also carries g_a.  r_k and the staged word are
// LDS broadcasts (one address per step); x_ka and x_kb come from the shared table through L2, four positions requested ahead of their
// use (all lanes of a step read one row of 8 p bytes).  Lanes of pairs outside the mask do nothing.  The lanes leave I (both
// triangles) and g in LDS.  (4) The logarithms stay out of the walk: with times in whole days nearly every step ends a tie group, and a
// log(S0) there runs on one lane of one wave while the others wait at the barrier.  The lane of the mask's first column only LEAVES S0
// and d at the group's last position (d in the staged word's upper bits); after the walk all 256 threads take the logarithms and sum
// d log S0 thread -> wave -> block in a fixed order.
//
// A walk is a chain of n dependent steps of one wave, so the launch's speed is the number of walks in flight: the kernel is compiled
// for CN_WAVES_PER_SIMD resident waves (DESIGN.md section 5 has the measurements that chose it), and nothing in it keeps register
// arrays -- the point, the factor and Z are read from LDS where they are used.
//
// The solver's linear algebra is 16 x 16 at the most and runs in LDS with one barrier per Cholesky column: thread i owns row i of a
// left-looking factorisation (every thread forms the pivot from the finished part of row j, so the singularity test is uniform and
// costs no broadcast), thread c then forms column c of Z = L^-1 by forward substitution on its own entries in LDS, thread i
// y_i = (Z g)_i, and thread c delta_c = <Z_c, y> and se_c = |Z_c| (I^-1 = Z' Z).  Columns outside the mask, and those from p to 16, stand as identity rows in L:
// their delta is 0 and nothing of theirs reaches an active entry.  Every decision is taken by every thread from the same LDS values,
// so the control flow is uniform and the barriers inside it are legal.  Every thread owns its outputs: plain stores, no atomics;
// nothing depends on Q, on the problem's place in the launch or on whether info is asked for.
#include "common.h"

#define CN_THREADS 256
#define CN_WAVES (CN_THREADS / 64)
#define CN_P MMS_COXNEWTON_MAX_P
#define CN_PAIRS (CN_P * (CN_P + 1) / 2)
#define CN_EVENT 0x100
#define CN_GLAST 0x200
#define CN_HALVINGS 20
#define CN_WAVES_PER_SIMD 8            // resident waves per SIMD the kernel is compiled for (the register budget: 512 / this)

#define CN_DSHIFT 10
// LDS, in doubles: rr[n] | s0[n] | small (below; CN_LT: 8 spare) | then the staged words int[n]
enum { CN_RED = 0, CN_BK = 8, CN_BT = CN_BK + CN_P, CN_GK = CN_BT + CN_P, CN_GT = CN_GK + CN_P, CN_DELTA = CN_GT + CN_P, CN_SE = CN_DELTA + CN_P,
       CN_LD = CN_SE + CN_P, CN_LT = CN_LD + CN_P, CN_IK = CN_LT + 8, CN_IT = CN_IK + CN_P * CN_P, CN_L = CN_IT + CN_P * CN_P,
       CN_SMALL = CN_L + CN_P * CN_P };
static size_t cn_lds_bytes(int n) { return sizeof(double) * (2 * (size_t)n + CN_SMALL) + sizeof(int) * (size_t)n; }

struct CnCtx {
    const double* x; int ldx, n, p; unsigned mask;
    double* rr; double* s0; double* sm; int* wf;
    int tid, lane, wave, pa, pb; bool walks, pair_on, owner;
};

// g and I at the point in sm[CN_BT..] -> sm[CN_GT..], sm[CN_IT..] (zero outside the mask); returns l (the same value in every thread).
// The caller has a barrier between two evaluations.
__device__ __forceinline__ double cn_eval(const CnCtx& c) {
    double* sm = c.sm;
    const int n = c.n;
    sm[CN_IT + c.tid] = 0.0;
    if (c.tid < CN_P) sm[CN_GT + c.tid] = 0.0;
    double mx = -INFINITY;
    for (int k = c.tid; k < n; k += CN_THREADS) {
        const double* xr = c.x + (size_t)k * c.ldx;
        double e = 0.0;
        for (unsigned m = c.mask; m; m &= m - 1u) {                    // (uniform: the point is an LDS broadcast)
            const int a = __ffs((int)m) - 1;
            e = fma(xr[a], sm[CN_BT + a], e);
        }
        c.rr[k] = e;
        if (c.wf[k] & 0xff) mx = fmax(mx, e);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o));
    if (c.lane == 0) sm[CN_RED + c.wave] = mx;
    __syncthreads();
    mx = fmax(fmax(sm[CN_RED], sm[CN_RED + 1]), fmax(sm[CN_RED + 2], sm[CN_RED + 3]));
    if (!(mx > -INFINITY)) mx = 0.0;                                   // (nobody drawn: every r is 0)
    double se = 0.0;
    for (int k = c.tid; k < n; k += CN_THREADS) {
        const int f = c.wf[k], wi = f & 0xff;
        const double e = c.rr[k] - mx;
        c.rr[k] = wi ? (double)wi * exp(e) : 0.0;
        if ((f & CN_EVENT) && wi) se = fma((double)wi, e, se);
    }
    se = wave_sum_d(se);
    if (c.lane == 0) sm[CN_RED + 4 + c.wave] = se;
    __syncthreads();
    if (c.walks) {
        const double* xa = c.x + c.pa;
        const double* xb = c.x + c.pb;
        double S0 = 0.0, S1a = 0.0, S1b = 0.0, S2 = 0.0, Iab = 0.0, ga = 0.0, sx = 0.0;
        int d = 0;
        for (int k0 = 0; k0 < n; k0 += 4) {
            double va[4], vb[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {                              // (past the end: the last row again, not used)
                const size_t o = (size_t)min(k0 + j, n - 1) * c.ldx;
                va[j] = xa[o]; vb[j] = xb[o];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = k0 + j;
                if (k < n) {
                    const int f = c.wf[k];
                    const double r = c.rr[k], t = r * va[j];
                    const int we = f & CN_EVENT ? f & 0xff : 0;
                    S0 += r; S1a += t; S1b = fma(r, vb[j], S1b); S2 = fma(t, vb[j], S2);
                    d += we; sx = fma((double)we, va[j], sx);
                    if (f & CN_GLAST) {                                // (uniform: every lane is at the same position)
                        if (d > 0) {
                            // true divisions and an unfused difference: a column that is constant c over the risk set, with c and
                            // the r exact (an indicator, or one patient drawn 2^k times), then gives EXACTLY zero information and
                            // gradient -- S1 / S0 = c, S2 / S0 = c c -- so the pivot test does not hang on rounding
                            const double dd = (double)d, ma = S1a / S0, mb = S1b / S0;
                            Iab = fma(dd, __dsub_rn(S2 / S0, __dmul_rn(ma, mb)), Iab);
                            ga += __dsub_rn(sx, __dmul_rn(dd, ma));
                        }
                        if (c.owner) { c.s0[k] = S0; c.wf[k] = (f & ((1 << CN_DSHIFT) - 1)) | (d << CN_DSHIFT); }   // (the low bits stay: other lanes still read them)
                        d = 0; sx = 0.0;
                    }
                }
            }
        }
        if (c.pair_on) {
            sm[CN_IT + c.pa * CN_P + c.pb] = Iab;
            sm[CN_IT + c.pb * CN_P + c.pa] = Iab;
            if (c.pa == c.pb) sm[CN_GT + c.pa] = ga;
        }
    }
    __syncthreads();
    double sl = 0.0;
    for (int k = c.tid; k < n; k += CN_THREADS) {
        const int d = c.wf[k] >> CN_DSHIFT;
        if (d) sl = fma((double)d, log(c.s0[k]), sl);
    }
    sl = wave_sum_d(sl);
    if (c.lane == 0) sm[CN_RED + c.wave] = sl;
    __syncthreads();
    return ((sm[CN_RED + 4] + sm[CN_RED + 5]) + (sm[CN_RED + 6] + sm[CN_RED + 7])) - ((sm[CN_RED] + sm[CN_RED + 1]) + (sm[CN_RED + 2] + sm[CN_RED + 3]));
}

__global__ __launch_bounds__(CN_THREADS) __attribute__((amdgpu_waves_per_eu(CN_WAVES_PER_SIMD, CN_WAVES_PER_SIMD))) void cox_newton_kernel(const CoxNewtonP a) {
    extern __shared__ __attribute__((aligned(16))) double cn_lds[];
    const int n = a.n, p = a.p, tid = threadIdx.x;
    const int q = blockIdx.x, r = q / a.S, s = q - r * a.S;
    CnCtx c;
    c.x = a.x; c.ldx = a.ldx; c.n = n; c.p = p;
    c.mask = (unsigned)a.cmask[s] & ((1u << p) - 1u);                  // (p <= 16)
    c.rr = cn_lds; c.s0 = cn_lds + n; c.sm = cn_lds + 2 * n;
    int* wf = (int*)(c.sm + CN_SMALL);
    c.wf = wf;
    c.tid = tid; c.lane = tid & 63; c.wave = tid >> 6;
    {   // the pair of this thread: tid = b (b + 1) / 2 + a, a <= b
        int b = 0;
        while (b < CN_P - 1 && (b + 1) * (b + 2) / 2 <= tid) ++b;
        const int aa = tid - b * (b + 1) / 2;
        const bool is_pair = tid < CN_PAIRS && b < p;
        const int a0 = c.mask ? __ffs((int)c.mask) - 1 : 0;
        c.pa = is_pair ? aa : 0; c.pb = is_pair ? b : 0;
        c.pair_on = is_pair && ((c.mask >> aa) & 1u) && ((c.mask >> b) & 1u);
        c.owner = is_pair && aa == a0 && b == a0;                     // the lane that carries l (the null model of an empty mask has no other)
        c.walks = c.pair_on || c.owner;
    }
    double* sm = c.sm;
    const unsigned mask = c.mask;
    const bool act = tid < CN_P && ((mask >> tid) & 1u);              // thread a < 16 owns coefficient a
    // stage the row; D = sum w e
    const signed char* w = a.w + (size_t)r * a.ldw;
    int D = 0;
    for (int k = tid; k < n; k += CN_THREADS) {
        const int wi = w[k] & 0x7f, e = a.event[k] != 0;
        wf[k] = wi | (e ? CN_EVENT : 0) | (a.glast[k] != 0 || k == n - 1 ? CN_GLAST : 0);
        D += e ? wi : 0;
    }
    for (int o = 32; o > 0; o >>= 1) D += __shfl_xor(D, o);
    if (c.lane == 0) ((int*)(sm + CN_LD))[c.wave] = D;                 // (CN_LD is not in use yet)
    if (tid < CN_P) { sm[CN_BK + tid] = 0.0; sm[CN_BT + tid] = 0.0; sm[CN_SE + tid] = NAN; }
    __syncthreads();
    D = ((int*)(sm + CN_LD))[0] + ((int*)(sm + CN_LD))[1] + ((int*)(sm + CN_LD))[2] + ((int*)(sm + CN_LD))[3];
    __syncthreads();                                                   // (CN_LD is free again)
    int status = 0, iters = 0;
    double lk = 0.0, l0 = 0.0;
    if (D == 0) {
        status = 6;
        sm[CN_IK + tid] = 0.0;
        __syncthreads();
    } else {
        lk = l0 = cn_eval(c);
        sm[CN_IK + tid] = sm[CN_IT + tid];
        if (tid < CN_P) sm[CN_GK + tid] = sm[CN_GT + tid];
        __syncthreads();
    }
    while (status == 0) {
        // factor I = L L' on the mask's columns (identity rows elsewhere); Ld = the diagonal of L
        const int i = tid >> 4, j0 = tid & 15;
        const bool on = i < p && j0 < p && ((mask >> i) & 1u) && ((mask >> j0) & 1u);
        sm[CN_L + tid] = on ? sm[CN_IK + tid] : (i == j0 ? 1.0 : 0.0);
        double maxdiag = 0.0;
#pragma unroll
        for (int k = 0; k < CN_P; ++k)
            if (k < p && ((mask >> k) & 1u)) maxdiag = fmax(maxdiag, sm[CN_IK + k * CN_P + k]);
        __syncthreads();
        bool singular = false;
        for (int j = 0; j < CN_P; ++j) {
            double piv = sm[CN_L + j * CN_P + j];
            for (int k = 0; k < j; ++k) { const double l = sm[CN_L + j * CN_P + k]; piv = fma(-l, l, piv); }
            if (j < p && ((mask >> j) & 1u) && !(piv > 1e-10 * maxdiag)) { singular = true; break; }
            const double ljj = sqrt(piv);
            if (tid < CN_P && tid > j) {
                double v = sm[CN_L + tid * CN_P + j];
                for (int k = 0; k < j; ++k) v = fma(-sm[CN_L + tid * CN_P + k], sm[CN_L + j * CN_P + k], v);
                sm[CN_L + tid * CN_P + j] = v / ljj;
            }
            if (tid == j) sm[CN_LD + j] = ljj;
            __syncthreads();
        }
        if (singular) { status = 3; break; }
        // Z = L^-1 (thread c: column c, kept as row c of Zt; forward substitution on its own entries), y = Z g, delta = Z' y,
        // se_c = the column's norm.  Zt and y use the trial buffers, which are free between two evaluations.
        double* Zt = sm + CN_IT;
        double* y = sm + CN_GT;
        if (tid < CN_P) {
            double ss = 0.0;
            for (int i = 0; i < CN_P; ++i) {
                double zi = i == tid ? 1.0 : 0.0;
                for (int k = tid; k < i; ++k) zi = fma(-sm[CN_L + i * CN_P + k], Zt[tid * CN_P + k], zi);
                zi = i < tid ? 0.0 : zi / sm[CN_LD + i];
                Zt[tid * CN_P + i] = zi;
                ss = fma(zi, zi, ss);
            }
            sm[CN_SE + tid] = act ? sqrt(ss) : NAN;
        }
        __syncthreads();
        if (tid < CN_P) {
            double yi = 0.0;
            for (int b = 0; b <= tid; ++b) yi = fma(Zt[b * CN_P + tid], sm[CN_GK + b], yi);
            y[tid] = yi;
        }
        __syncthreads();
        if (tid < CN_P) {
            double dl = 0.0;
            for (int i = tid; i < CN_P; ++i) dl = fma(Zt[tid * CN_P + i], y[i], dl);
            sm[CN_DELTA + tid] = act ? dl : 0.0;
        }
        __syncthreads();
        double md = 0.0;
#pragma unroll
        for (int k = 0; k < CN_P; ++k) md = fmax(md, fabs(sm[CN_DELTA + k]));
        if (md <= a.tol) { status = 1; break; }
        bool accepted = false;
        double lt = 0.0;
        for (int h = 0; h <= CN_HALVINGS; ++h) {
            const double sc = ldexp(1.0, -h);
            if (tid < CN_P) sm[CN_BT + tid] = act ? fma(sc, sm[CN_DELTA + tid], sm[CN_BK + tid]) : 0.0;
            __syncthreads();
            lt = cn_eval(c);
            if (lt >= lk - 1e-12 * fmax(1.0, fabs(lk))) { accepted = true; break; }
        }
        if (!accepted) { status = 5; break; }
        lk = lt; ++iters;
        sm[CN_IK + tid] = sm[CN_IT + tid];
        if (tid < CN_P) { sm[CN_GK + tid] = sm[CN_GT + tid]; sm[CN_BK + tid] = sm[CN_BT + tid]; }
        __syncthreads();
        double mb = 0.0;
#pragma unroll
        for (int k = 0; k < CN_P; ++k) mb = fmax(mb, fabs(sm[CN_BK + k]));
        if (mb > a.beta_max) status = 4;
        else if (iters >= a.max_iter) status = 2;
    }
    if (tid < p) {
        a.beta[(size_t)q * p + tid] = sm[CN_BK + tid];
        a.se[(size_t)q * p + tid] = status == 1 ? sm[CN_SE + tid] : NAN;
    }
    if (tid == 0) { a.loglik[q] = lk; a.loglik0[q] = l0; a.iters[q] = iters; a.status[q] = status; }
    if (a.info) {
        const int i = tid >> 4, j = tid & 15;
        if (i < p && j < p) a.info[((size_t)q * p + i) * p + j] = sm[CN_IK + tid];
    }
}

extern "C" int mms_cox_newton(const CoxNewtonP* p, hipStream_t s) {
    if (!p || !p->x || !p->event || !p->glast || !p->w || !p->cmask) return MMS_ERR_ARG;
    if (!p->beta || !p->se || !p->loglik || !p->loglik0 || !p->iters || !p->status) return MMS_ERR_ARG;
    if (p->n < 1 || p->n > MMS_COXNEWTON_MAX_N || p->p < 1 || p->p > MMS_COXNEWTON_MAX_P || p->ldx < p->p || p->ldw < p->n) return MMS_ERR_ARG;
    if (p->R < 0 || p->S < 0 || p->S > MMS_COXNEWTON_MAX_S || (long long)p->R * p->S > MMS_COXNEWTON_MAX_Q) return MMS_ERR_ARG;
    if (!(p->tol > 0.0 && p->tol <= MMS_COXNEWTON_MAX_TOL) || p->max_iter < 1 || p->max_iter > MMS_COXNEWTON_MAX_ITER || !(p->beta_max > 0.0)) return MMS_ERR_ARG;
    if (((uintptr_t)p->x & 7) || ((uintptr_t)p->beta & 7) || ((uintptr_t)p->se & 7) || ((uintptr_t)p->loglik & 7) || ((uintptr_t)p->loglik0 & 7)) return MMS_ERR_ARG;
    if (((uintptr_t)p->info & 7) || ((uintptr_t)p->event & 3) || ((uintptr_t)p->glast & 3) || ((uintptr_t)p->cmask & 3)) return MMS_ERR_ARG;
    if (((uintptr_t)p->iters & 3) || ((uintptr_t)p->status & 3)) return MMS_ERR_ARG;
    if (p->R == 0 || p->S == 0) return MMS_OK;
    static std::once_flag attr_once;                                   // (the largest n needs more than the default 64 KiB window)
    std::call_once(attr_once, [] { hipFuncSetAttribute((const void*)cox_newton_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)cn_lds_bytes(MMS_COXNEWTON_MAX_N)); });
    MMS_LAUNCH(cox_newton_kernel, dim3((unsigned)(p->R * p->S)), dim3(CN_THREADS), cn_lds_bytes(p->n), s, *p);
    return mms_check_launch();
}
