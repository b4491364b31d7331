// Elastic-net Cox regression, P problems advanced in lock-step (include/mmsurv.h: CoxnetP).
//
// Every problem shares one row list (patients in time-descending order) and differs in its integer multiplicities, its penalty and its
// coefficients.  One proximal-gradient iteration of ALL problems is four launches:
//   eta     E[p][k]  = sum_j B[p][j] inv_scale[p][j] x[row[k]][j]           v_mfma_f64_16x16x4_f64, K = genes
//   scan    one workgroup per problem: shift, S0 at the tie-group ends, d_u, c, the residual r and the loss (fp64, fixed trees)
//   xtr     Gr[p][j] = sum_k R[p][k] * x[row[k]][j]                          the same instruction, K = rows
//   update  one workgroup per problem: accept test, step rule, KKT residual, freeze, next trial, counters
// No launch waits for another workgroup, nothing is added with float atomics, and every number of problem p is computed from p's own
// data in an order that depends on G and the row count only: a problem's bits do not depend on P or on its place in the launch.
//
// f64 MFMA maps (16x16x4, one f64 per lane for A and B, four per lane for D): A[m = lane & 15][k = lane >> 4], B[k = lane >> 4][n = lane & 15],
// D[m = (lane >> 4) + 4 i][n = lane & 15] in register i.  Both products put the problems on M.  Each lane reads FOUR consecutive k of
// its operand row (k = 16 s + 4 h + i, h = lane >> 4), and MFMA i of step s sums over h: a permuted but fixed K order, the same for A and B.
#include "common.h"
#include <math.h>

typedef double f64x4 __attribute__((ext_vector_type(4)));

#define CX_MFMA(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0)
#define CX_PT 4          // xtr: 16-problem tiles per wave (a workgroup's 4 waves share one strip of 64 problems)

// ---- eta: E = B . x^T --------------------------------------------------------------------------------------------------------------
// workgroup = 16 list positions x 16 problems; its four waves take every fourth 16-gene step of K (wave w: genes 64 i + 16 w ..), and
// their partial tiles are added through LDS in wave order: a split of K that depends on nothing but G.  Small tiles on purpose: the
// operands come straight from L2 / memory, and what hides that latency is the number of waves in flight (a 16 x 64 tile per workgroup
// left one wave per SIMD at P = 900 and cost 0.83 ms).  grid x = 16 positions, y = 16 problems
__global__ __launch_bounds__(256) void coxnet_eta_kernel(const CoxnetP a, const double* __restrict__ B) {
    __shared__ double part[4][4][64];                               // 8 KB
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int c = lane & 15, h = lane >> 4;
    const int kk = blockIdx.x * 16 + c, p = blockIdx.y * 16 + c;
    const bool rv = kk < a.nrow, pv = p < a.P;
    const float* xr = a.x + (size_t)(rv ? a.row[kk] : 0) * a.ld;
    const double* bp = B + (size_t)(pv ? p : 0) * a.G;
    const double* sp = a.inv_scale ? a.inv_scale + (size_t)(pv ? p : 0) * a.G : nullptr;
    f64x4 acc = f64x4{0.0, 0.0, 0.0, 0.0};
    for (int j0 = 16 * wave; j0 < a.G; j0 += 64) {
        const int j = j0 + 4 * h;
        double xv[4], bv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            xv[i] = (rv && j + i < a.G) ? (double)xr[j + i] : 0.0;
            const bool ok = pv && j + i < a.G;
            bv[i] = ok ? bp[j + i] : 0.0;
            if (sp) bv[i] = ok ? bv[i] * sp[j + i] : 0.0;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) acc = CX_MFMA(bv[i], xv[i], acc);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) part[wave][i][lane] = acc[i];
    __syncthreads();
    const int po = blockIdx.y * 16 + h + 4 * wave;                   // wave w adds up and stores register w of the tile
    const double v = ((part[0][wave][lane] + part[1][wave][lane]) + part[2][wave][lane]) + part[3][wave][lane];
    if (po < a.P && rv) a.E[(size_t)po * a.nrow + kk] = v;
}

// ---- xtr: Gr = R . x ------------------------------------------------------------------------------------------------------------------
// wave = 16 genes x 64 problems, K = every list position in order; grid x = 64 genes, y = 64 problems
__global__ __launch_bounds__(256) void coxnet_xtr_kernel(const CoxnetP a) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int c = lane & 15, h = lane >> 4;
    const int j0 = (blockIdx.x * 4 + wave) * 16;
    if (j0 >= a.G) return;
    const int p0 = blockIdx.y * 16 * CX_PT;
    const int nt = min(CX_PT, (a.P - p0 + 15) / 16);
    const int j = j0 + c;
    const bool jv = j < a.G;
    f64x4 acc[CX_PT];
#pragma unroll
    for (int t = 0; t < CX_PT; ++t) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < a.nrow; k0 += 16) {
        const int k = k0 + 4 * h;
        double xv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) xv[i] = (jv && k + i < a.nrow) ? (double)a.x[(size_t)a.row[k + i] * a.ld + j] : 0.0;
#pragma unroll
        for (int t = 0; t < CX_PT; ++t) {
            if (t >= nt) continue;                                  // (uniform)
            const int p = p0 + 16 * t + c;
            const bool pv = p < a.P;
            const double* rp = a.R + (size_t)(pv ? p : 0) * a.nrow;
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[t] = CX_MFMA((pv && k + i < a.nrow) ? rp[k + i] : 0.0, xv[i], acc[t]);
        }
    }
#pragma unroll
    for (int t = 0; t < CX_PT; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int p = p0 + 16 * t + h + 4 * i;
            if (t < nt && p < a.P && jv) a.Gr[(size_t)p * a.G + j] = acc[t][i];
        }
}

// ---- workgroup reductions of 256 threads, fixed trees; the result is valid in every thread ---------------------------------------------
__device__ __forceinline__ double cx_block_sum(double v, double* red) {
    v = wave_sum_d(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}
__device__ __forceinline__ double cx_block_max(double v, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
}

// ---- scan ------------------------------------------------------------------------------------------------------------------------------
// One workgroup per problem, chunks of 256 list positions with carried prefixes (any row count).  Forward: S0 = the running sum of
// m exp(eta - shift), D = the running sum of m e; at a tie group's last position d_u = D - (D at the previous group's end), kept by a
// running maximum (D never decreases), h = d_u / S0 is parked in R and the loss collects d_u log S0.  Backward: c = the suffix sum of
// h, r = m e - m exp(eta - shift) c.  A row with m = 0 is selected out: it never enters a product.
__global__ __launch_bounds__(256) void coxnet_scan_kernel(const CoxnetP a) {
    __shared__ double sh[3][4];
    __shared__ double red[4];
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int n = a.nrow;
    const int* m = a.mult + (size_t)p * n;
    const double* eta = a.E + (size_t)p * n;
    double* r = a.R + (size_t)p * n;

    double mx = -INFINITY;
    for (int k = tid; k < n; k += 256)
        if (m[k] > 0) mx = fmax(mx, eta[k]);
    double shift = cx_block_max(mx, red);
    if (!(shift > -INFINITY)) shift = 0.0;                          // no row with m > 0

    double cS = 0.0, cD = 0.0, cM = 0.0, tl = 0.0, tn = 0.0;
    for (int base = 0; base < n; base += 256) {
        const int k = base + tid;
        const bool v = k < n;
        const int mk = v ? m[k] : 0;
        const bool on = mk > 0;
        const bool gl = v && a.glast[k] != 0;
        const double d = on ? eta[k] - shift : 0.0;
        const double me = (on && a.event[k] != 0) ? (double)mk : 0.0;
        double S = on ? (double)mk * exp(d) : 0.0, D = me;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {                          // inclusive sums inside the wave
            const double ts = __shfl_up(S, o, 64), td = __shfl_up(D, o, 64);
            if (lane >= o) { S += ts; D += td; }
        }
        if (lane == 63) { sh[0][w] = S; sh[1][w] = D; }
        __syncthreads();
        double pS = 0.0, pD = 0.0, tS = 0.0, tD = 0.0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (i < w) { pS += sh[0][i]; pD += sh[1][i]; }
            tS += sh[0][i]; tD += sh[1][i];
        }
        S = cS + (pS + S); D = cD + (pD + D);
        double M = gl ? D : 0.0;                                    // exclusive running maximum of D at the group ends
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const double tm = __shfl_up(M, o, 64);
            if (lane >= o) M = fmax(M, tm);
        }
        if (lane == 63) sh[2][w] = M;
        double Me = __shfl_up(M, 1, 64);
        if (lane == 0) Me = 0.0;
        __syncthreads();
        double pM = cM, tM = cM;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (i < w) pM = fmax(pM, sh[2][i]);
            tM = fmax(tM, sh[2][i]);
        }
        const double du = gl ? D - fmax(Me, pM) : 0.0;
        double hk = 0.0;
        if (du > 0.0) { hk = du / S; tl += du * log(S); }
        tl -= me * d;
        tn += (double)mk;
        if (v) r[k] = hk;
        cS += tS; cD += tD; cM = tM;
        __syncthreads();                                            // sh is rewritten by the next chunk
    }

    double cC = 0.0;
    for (int base = (n - 1) / 256 * 256; base >= 0; base -= 256) {
        const int k = base + tid;
        const bool v = k < n;
        double c = v ? r[k] : 0.0;                                  // (this thread's own store)
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {                          // inclusive suffix sums inside the wave
            const double t = __shfl_down(c, o, 64);
            if (lane + o < 64) c += t;
        }
        if (lane == 0) sh[0][w] = c;
        __syncthreads();
        double pC = 0.0, tC = 0.0;
#pragma unroll
        for (int i = 3; i >= 0; --i) {
            if (i > w) pC += sh[0][i];
            tC += sh[0][i];
        }
        c = cC + (pC + c);
        const int mk = v ? m[k] : 0;
        const bool on = mk > 0;
        const double me = (on && a.event[k] != 0) ? (double)mk : 0.0;
        const double wv = on ? (double)mk * exp(eta[k] - shift) : 0.0;
        if (v) r[k] = on ? me - wv * c : 0.0;
        cC += tC;
        __syncthreads();
    }
    tl = cx_block_sum(tl, red);
    tn = cx_block_sum(tn, red);
    if (tid == 0) { a.loss[p] = tl; a.nsum[p] = tn; }
}

// ---- update ----------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double cx_soft(double z, double t) { return z > t ? z - t : (z < -t ? z + t : 0.0); }
__device__ __forceinline__ double cx_kkt(double b, double g, double l1) {
    return b > 0.0 ? fabs(g + l1) : (b < 0.0 ? fabs(g - l1) : fmax(fabs(g) - l1, 0.0));
}
// the smooth part's gradient at coefficient b of gene j from the raw product
#define CX_GRAD(j, b) (-(gr[j] * invn) * (sc ? sc[j] : 1.0) + l2 * (b))

// One workgroup per problem.  status < 0: a new problem, whose trial is its start: it is taken as the kept point without a test, the
// step stays and no iteration is counted.  status > 0: frozen.
__global__ __launch_bounds__(256) void coxnet_update_kernel(const CoxnetP a) {
    __shared__ double red[4];
    const int p = blockIdx.x, tid = threadIdx.x;
    const int st = a.status[p];
    if (st > 0) return;
    const bool fresh = st < 0;
    const int G = a.G;
    const double lam = a.lam[p], al = a.alpha[p], l1 = lam * al, l2 = lam * (1.0 - al);
    const double n = a.nsum[p], invn = n > 0.0 ? 1.0 / n : 0.0;
    double s = a.step[p];
    const double fk = fresh ? 0.0 : a.f[p];
    double* be = a.beta + (size_t)p * G; double* tr = a.trial + (size_t)p * G; double* gk = a.grad + (size_t)p * G;
    const double* gr = a.Gr + (size_t)p * G;
    const double* sc = a.inv_scale ? a.inv_scale + (size_t)p * G : nullptr;

    double ss = 0.0, gd = 0.0, dd = 0.0;
    for (int j = tid; j < G; j += 256) {
        const double t = tr[j];
        ss = fma(t, t, ss);
        if (!fresh) { const double d = t - be[j]; gd = fma(gk[j], d, gd); dd = fma(d, d, dd); }
    }
    ss = cx_block_sum(ss, red); gd = cx_block_sum(gd, red); dd = cx_block_sum(dd, red);
    const double ft = a.loss[p] * invn + 0.5 * l2 * ss;
    const bool accept = fresh || ft <= fk + gd + dd / (2.0 * s) + 1e-12 * fmax(1.0, fabs(fk));
    int it = a.iters[p] + (fresh ? 0 : 1);
    if (!accept) {
        s *= 0.5;
        for (int j = tid; j < G; j += 256) tr[j] = cx_soft(be[j] - s * gk[j], s * l1);
        if (tid == 0) {
            a.step[p] = s; a.iters[p] = it;
            if (it >= a.max_iter) { a.status[p] = 2; atomicSub(a.counter, 1); }
        }
        return;
    }
    if (!fresh) s *= 1.25;
    double rho = 0.0, n1 = 0.0;
    for (int j = tid; j < G; j += 256) {
        const double t = tr[j], g = CX_GRAD(j, t);
        be[j] = t; gk[j] = g;
        const double kj = cx_kkt(t, g, l1);
        rho = kj > rho || kj != kj ? kj : rho;                      // (a NaN stays)
        n1 += fabs(t);
        tr[j] = cx_soft(t - s * g, s * l1);
    }
    const bool bad = cx_block_sum(rho != rho ? 1.0 : 0.0, red) > 0.0;
    rho = cx_block_max(rho, red);
    n1 = cx_block_sum(n1, red);
    if (bad) rho = NAN;
    if (tid == 0) {
        const bool conv = rho <= a.tol;
        a.f[p] = ft; a.step[p] = s; a.kkt[p] = rho; a.obj[p] = ft + l1 * n1; a.iters[p] = it;
        if (conv) { a.status[p] = 1; atomicSub(a.counter, 1); }
        else if (it >= a.max_iter) { a.status[p] = 2; atomicSub(a.counter, 1); }
        else if (fresh) a.status[p] = 0;
    }
}

// mms_coxnet_eval's last launch: gradient, smooth objective, KKT residual and objective at beta; the solver's state is not touched
__global__ __launch_bounds__(256) void coxnet_finish_kernel(const CoxnetP a) {
    __shared__ double red[4];
    const int p = blockIdx.x, tid = threadIdx.x;
    const int G = a.G;
    const double lam = a.lam[p], al = a.alpha[p], l1 = lam * al, l2 = lam * (1.0 - al);
    const double n = a.nsum[p], invn = n > 0.0 ? 1.0 / n : 0.0;
    const double* be = a.beta + (size_t)p * G; double* gk = a.grad + (size_t)p * G;
    const double* gr = a.Gr + (size_t)p * G;
    const double* sc = a.inv_scale ? a.inv_scale + (size_t)p * G : nullptr;
    double ss = 0.0, rho = 0.0, n1 = 0.0;
    for (int j = tid; j < G; j += 256) {
        const double t = be[j], g = CX_GRAD(j, t);
        gk[j] = g;
        ss = fma(t, t, ss);
        const double kj = cx_kkt(t, g, l1);
        rho = kj > rho || kj != kj ? kj : rho;
        n1 += fabs(t);
    }
    ss = cx_block_sum(ss, red);
    const bool bad = cx_block_sum(rho != rho ? 1.0 : 0.0, red) > 0.0;
    rho = cx_block_max(rho, red);
    n1 = cx_block_sum(n1, red);
    if (tid == 0) {
        const double f = a.loss[p] * invn + 0.5 * l2 * ss;
        a.f[p] = f; a.kkt[p] = bad ? NAN : rho; a.obj[p] = f + l1 * n1;
    }
}

static int coxnet_check(const CoxnetP* p) {
    if (!p || !p->x || !p->row || !p->event || !p->glast || !p->mult || !p->lam || !p->alpha) return MMS_ERR_ARG;
    if (!p->beta || !p->trial || !p->grad || !p->f || !p->step || !p->iters || !p->status) return MMS_ERR_ARG;
    if (!p->loss || !p->nsum || !p->kkt || !p->obj || !p->E || !p->R || !p->Gr || !p->counter) return MMS_ERR_ARG;
    if (p->P < 0 || p->G < 1 || p->ld < p->G || p->N < 1 || p->nrow < 0) return MMS_ERR_ARG;
    if (!(p->tol > 0.0) || !(p->tol <= MMS_COXNET_MAX_TOL) || p->max_iter < 1 || p->max_iter > MMS_COXNET_MAX_ITER) return MMS_ERR_ARG;
    const uintptr_t a4 = (uintptr_t)p->x | (uintptr_t)p->row | (uintptr_t)p->event | (uintptr_t)p->glast | (uintptr_t)p->mult |
                         (uintptr_t)p->iters | (uintptr_t)p->status | (uintptr_t)p->counter;
    const uintptr_t a8 = (uintptr_t)p->lam | (uintptr_t)p->alpha | (uintptr_t)p->inv_scale | (uintptr_t)p->beta | (uintptr_t)p->trial |
                         (uintptr_t)p->grad | (uintptr_t)p->f | (uintptr_t)p->step | (uintptr_t)p->loss | (uintptr_t)p->nsum |
                         (uintptr_t)p->kkt | (uintptr_t)p->obj | (uintptr_t)p->E | (uintptr_t)p->R | (uintptr_t)p->Gr;
    if ((a4 & 3) || (a8 & 7)) return MMS_ERR_ARG;
    if ((p->P + 15) / 16 > 65535) return MMS_ERR_ARG;               // (grid y of the eta product)
    return MMS_OK;
}

// eta at B, the scan and the raw gradient product
static void coxnet_products(const CoxnetP* p, const double* B, hipStream_t s) {
    const int py = (p->P + 16 * CX_PT - 1) / (16 * CX_PT);
    MMS_LAUNCH(coxnet_eta_kernel, dim3((p->nrow + 15) / 16, (p->P + 15) / 16), dim3(256), 0, s, *p, B);
    MMS_LAUNCH(coxnet_scan_kernel, dim3(p->P), dim3(256), 0, s, *p);
    MMS_LAUNCH(coxnet_xtr_kernel, dim3((p->G + 63) / 64, py), dim3(256), 0, s, *p);
}

extern "C" int mms_coxnet_eval(const CoxnetP* p, hipStream_t s) {
    const int rc = coxnet_check(p);
    if (rc != MMS_OK) return rc;
    if (p->P == 0 || p->nrow == 0) return MMS_OK;
    coxnet_products(p, p->beta, s);
    MMS_LAUNCH(coxnet_finish_kernel, dim3(p->P), dim3(256), 0, s, *p);
    return mms_check_launch();
}

extern "C" int mms_coxnet_iterate(const CoxnetP* p, int iters, hipStream_t s) {
    const int rc = coxnet_check(p);
    if (rc != MMS_OK || iters < 0) return MMS_ERR_ARG;
    if (p->P == 0 || p->nrow == 0 || iters == 0) return MMS_OK;
    for (int i = 0; i < iters; ++i) {
        coxnet_products(p, p->trial, s);
        MMS_LAUNCH(coxnet_update_kernel, dim3(p->P), dim3(256), 0, s, *p);
    }
    return mms_check_launch();
}
