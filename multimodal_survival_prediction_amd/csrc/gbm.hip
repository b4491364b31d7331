// Gradient-boosted Cox trees: P problems in lock-step, one tree a round (include/mmsurv.h: GbmGradP, GbmSplitP, GbmUpdateP, GbmPredictP).
//
// mms_gbm_grad -- workgroup = problem.  A forward scan of mult * exp(F - max) over the positions (time descending) gives the risk-set
// sums S, a backward scan of d / S and d / S^2 (left at the last position of each tie group with events) gives Lambda and Q; both scans
// run over chunks of 256 positions: wave scans, the wave totals in order, the chunks' carry in order.  The gradient and its curvature
// are quantised to int64 fixed point HERE, so that every sum the tree launches take is an exact integer and no later result depends on
// a summation order.  The launch also draws the round's row sample and leaves the root's sums.
// mms_gbm_split -- the hot path, two launches a level.  gbm_hist_kernel: workgroup = (tile of MMS_GBM_TILE features, problem); the
// histograms {count, sum qg, sum qh} of (feature, live node, bin) live in LDS, rows padded to B + 1 cells; two forms fill them:
//   members: lane = member; its weight, node, qg, qh are loaded once a pass and every feature of the pass is one byte load and three
//            integer LDS atomic adds (one 32-bit, two 64-bit); the waves start at different features of the pass;
//   private: lane = (feature, node); it walks all members and adds to its own row without atomics.
// A lane per (feature, node) then prefixes its row over the bins and scores the cuts; the row's first two cells then carry its best
// cut, and a lane per node folds the features in ascending order into the workgroup's best, which goes to the partial table.
// gbm_route_kernel: workgroup = problem; a lane per node folds the tiles in ascending order, writes the split and the children's sums,
// and the workgroup routes every position of a node that split.
// mms_gbm_update -- workgroup = problem: leaf values, F of all positions, then F and the pair keys 2 tgroup + event in LDS and the pair
// counts of the C-index as rsf.hip's mms_rsf_vimp takes them.
// mms_gbm_predict -- thread = (problem, row): the trees in round order, one sequential fp64 sum.
// No float atomics, no global atomics, plain stores; a problem's bits depend on its own row, scalars and hash stream only.
#include "common.h"

#define GBM_THREADS 256
#define GBM_MAX_NODES (1 << (MMS_GBM_MAX_DEPTH - 1))        // live nodes of the deepest level that splits
#define GBM_OUT 0x7ffffffe                                   // an even key no other key exceeds (rsf.hip: RSF_VIMP_OUT)

__device__ __forceinline__ uint32_t gbm_round_key(uint32_t seed, uint32_t id, uint32_t m) {
    return hash_u32((m + 1u) * 0x85ebca6bU + hash_u32(seed ^ (id * 0x85ebca6bU)));
}
__device__ __forceinline__ bool gbm_row_in(uint32_t hm, uint32_t row, uint32_t thr) { return hash_u32((row + 1u) * 0x9E3779B9U + hm) <= thr; }
__device__ __forceinline__ bool gbm_gene_in(uint32_t hm, uint32_t j, uint32_t thr) { return hash_u32((j + 1u) * 0x9E3779B9U + (hm ^ 0xB5297A4DU)) <= thr; }

// (G G) / (H + lambda) of int64 fixed-point sums: the conversions round to nearest, the scaling by 2^-32 is exact, then one square and
// one quotient -- nothing a fused multiply-add could change (fma(H, 2^-32, lambda) rounds the same sum once, as the plain form does)
__device__ __forceinline__ double gbm_term(long long G, long long H, double lam) {
    const double g = (double)G * 0x1p-32, h = (double)H * 0x1p-32 + lam;
    return h > 0.0 ? (g * g) / h : 0.0;
}
__device__ __forceinline__ double gbm_ratio(long long G, long long H, double lam) {
    const double g = (double)G * 0x1p-32, h = (double)H * 0x1p-32 + lam;
    return h > 0.0 ? g / h : 0.0;
}

// inclusive scan of (a, b) over the workgroup's 256 lanes in lane order: wave scans, then the wave totals in order; tot = the chunk's sum
__device__ __forceinline__ void gbm_scan2(double& a, double& b, double (*sw)[GBM_THREADS / 64], double& ta, double& tb) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int o = 1; o < 64; o <<= 1) {
        const double x = __shfl_up(a, o, 64), y = __shfl_up(b, o, 64);
        if (lane >= o) { a += x; b += y; }
    }
    __syncthreads();
    if (lane == 63) { sw[0][wave] = a; sw[1][wave] = b; }
    __syncthreads();
    double pa = 0.0, pb = 0.0;
    ta = 0.0; tb = 0.0;
    for (int w = 0; w < GBM_THREADS / 64; ++w) {
        if (w == wave) { pa = ta; pb = tb; }
        ta += sw[0][w]; tb += sw[1][w];
    }
    a = pa + a; b = pb + b;
}

__device__ __forceinline__ long long gbm_block_sum_ll(long long v, long long* red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    long long r = 0;
    for (int w = 0; w < GBM_THREADS / 64; ++w) r += red[w];
    return r;
}

__global__ __launch_bounds__(GBM_THREADS) void gbm_grad_kernel(const GbmGradP a) {
    __shared__ double sA[MMS_GBM_MAX_N], sB[MMS_GBM_MAX_N];
    __shared__ int sD[MMS_GBM_MAX_N], sT[MMS_GBM_MAX_N];
    __shared__ double sw[2][GBM_THREADS / 64];
    __shared__ double sred[GBM_THREADS / 64];
    __shared__ long long lred[GBM_THREADS / 64];
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = a.n;
    const unsigned char* mult = a.mult + (size_t)q * a.ld;
    const double* F = a.F + (size_t)q * a.ld;

    double mx = -__builtin_huge_val();
    for (int i = tid; i < n; i += GBM_THREADS)
        if (mult[i]) mx = fmax(mx, F[i]);
    for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
    if (lane == 0) sred[wave] = mx;
    __syncthreads();
    mx = fmax(fmax(sred[0], sred[1]), fmax(sred[2], sred[3]));
    const double c = mx > -__builtin_huge_val() ? mx : 0.0;
    __syncthreads();

    // forward: S (fp64) and the weighted events (int) up to and including each position
    double carry = 0.0, ll = 0.0;
    int dcarry = 0;
    for (int base = 0; base < n; base += GBM_THREADS) {
        const int i = base + tid;
        int w = 0, ev = 0, tg = -1;
        double v = 0.0, u = 0.0;
        if (i < n) {
            w = mult[i]; ev = a.event[i] != 0; tg = a.tgroup[i];
            if (w) {
                v = (double)w * exp(F[i] - c);
                if (ev) ll += (double)w * (F[i] - c);
            }
            u = (double)(w * ev);                        // (an integer below 2^53: its fp64 scan is exact)
        }
        double ta, tb;
        gbm_scan2(v, u, sw, ta, tb);
        if (i < n) { sA[i] = carry + v; sD[i] = dcarry + (int)u; sT[i] = tg; }
        carry += ta; dcarry += (int)tb;
    }
    __syncthreads();
    // the last position of each tie group with events: a = d / S, b = a / S
    for (int i = tid; i < n; i += GBM_THREADS) {
        double ca = 0.0, cb = 0.0;
        const int g = sT[i];
        if (i == n - 1 || sT[i + 1] != g) {
            int j = i - 1;
            while (j >= 0 && sT[j] == g) --j;
            const int d = sD[i] - (j >= 0 ? sD[j] : 0);
            const double S = sA[i];
            if (d > 0 && S > 0.0) {
                ca = (double)d / S; cb = ca / S;
                ll -= (double)d * log(S);
            }
        }
        sA[i] = ca; sB[i] = cb;                          // (only position i's own words: nobody else reads sA[i] in this loop)
    }
    ll = wave_sum_d(ll);
    __syncthreads();
    if (lane == 0) sred[wave] = ll;
    __syncthreads();
    if (tid == 0) a.loglik[(size_t)q * (a.M + 1) + a.round] = ((sred[0] + sred[1]) + sred[2]) + sred[3];
    if (a.last) return;

    // backward: Lambda and Q from the last position up
    const uint32_t hm = gbm_round_key(a.seed, (uint32_t)(a.pid ? a.pid[q] : q), (uint32_t)a.round);
    const uint32_t sub = a.subsample[q];
    long long* qg = a.qg + (size_t)q * a.ld;
    long long* qh = a.qh + (size_t)q * a.ld;
    unsigned char* wt = a.wt + (size_t)q * a.ld;
    int* node = a.node + (size_t)q * a.ld;
    double ca = 0.0, cb = 0.0;
    long long nr = 0, Gr = 0, Hr = 0;
    for (int base = 0; base < n; base += GBM_THREADS) {
        const int i = n - 1 - (base + tid);
        double va = i >= 0 ? sA[i] : 0.0, vb = i >= 0 ? sB[i] : 0.0, ta, tb;
        gbm_scan2(va, vb, sw, ta, tb);
        if (i >= 0) {
            const int w = mult[i];
            long long g64 = 0, h64 = 0;
            int ws = 0;
            if (w) {
                const double e = exp(F[i] - c), L = ca + va, Q = cb + vb;
                const double g = (a.event[i] != 0 ? 1.0 : 0.0) - e * L;
                const double h = e * L - (e * e) * Q;
                g64 = __double2ll_rn(fmin(fmax(g, -256.0), 1.0) * 4294967296.0);
                h64 = __double2ll_rn(fmin(fmax(h, 0.0), 256.0) * 4294967296.0);
                ws = gbm_row_in(hm, (uint32_t)a.rowid[i], sub) ? w : 0;
            }
            qg[i] = g64; qh[i] = h64; wt[i] = (unsigned char)ws; node[i] = 0;
            nr += ws; Gr += g64 * ws; Hr += h64 * ws;
        }
        ca += ta; cb += tb;
    }
    nr = gbm_block_sum_ll(nr, lred);
    Gr = gbm_block_sum_ll(Gr, lred);
    Hr = gbm_block_sum_ll(Hr, lred);
    if (tid == 0) {
        const size_t tb = ((size_t)q * a.M + a.round) * a.nn;
        a.n_node[tb] = (int)nr; a.G[tb] = Gr; a.H[tb] = Hr;
    }
}

__global__ __launch_bounds__(GBM_THREADS) void gbm_hist_kernel(const GbmSplitP a, const int gpp) {
    extern __shared__ __align__(16) unsigned char gbm_dyn[];
    __shared__ double b_gain[GBM_MAX_NODES];
    __shared__ long long b_G[GBM_MAX_NODES], b_H[GBM_MAX_NODES], s_G[GBM_MAX_NODES], s_H[GBM_MAX_NODES];
    __shared__ int b_f[GBM_MAX_NODES], b_bin[GBM_MAX_NODES], b_n[GBM_MAX_NODES], s_n[GBM_MAX_NODES];
    __shared__ unsigned s_mask[2];
    const int q = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, n = a.n, B = a.B, B1 = a.B + 1;
    const int nl = 1 << a.level, s0 = nl - 1;
    if (a.level >= a.depth[q]) return;
    const size_t tb = ((size_t)q * a.M + a.round) * a.nn;
    const int ml = a.min_leaf[q];
    const int f0 = tile * MMS_GBM_TILE, f1 = min(a.p, f0 + MMS_GBM_TILE);
    const uint32_t hm = gbm_round_key(a.seed, (uint32_t)(a.pid ? a.pid[q] : q), (uint32_t)a.round);
    if (tid < 64) {                                      // wave 0: the live nodes of the level and the admitted features of the tile
        bool live = false;
        if (tid < nl) {
            const int s = s0 + tid;
            const int nn_ = a.n_node[tb + s];
            live = (s == 0 || a.feat[tb + ((s - 1) >> 1)] >= 0) && nn_ >= 2 * ml;
            s_n[tid] = nn_; s_G[tid] = a.G[tb + s]; s_H[tid] = a.H[tb + s];
            b_gain[tid] = 0.0; b_f[tid] = -1; b_bin[tid] = 0; b_n[tid] = 0; b_G[tid] = 0; b_H[tid] = 0;
        }
        const unsigned long long lm = __ballot(live);
        const bool adm = f0 + tid < f1 && gbm_gene_in(hm, (uint32_t)(f0 + tid), a.colsample[q]);
        const unsigned long long am = __ballot(adm);
        if (tid == 0) { s_mask[0] = (unsigned)lm; s_mask[1] = (unsigned)am; }
    }
    __syncthreads();
    const unsigned livemask = s_mask[0], admmask = s_mask[1];
    if (livemask == 0u) return;                          // (uniform) nothing of this level can split: the partials are never read

    const int cells = gpp * nl * B1;                     // <= MMS_GBM_LDS_CELLS (the host checked)
    long long* hg = (long long*)gbm_dyn;                 // [cells]
    long long* hh = hg + cells;                          // [cells]
    int* hc = (int*)(hh + cells);                        // [cells]
    const double lam = a.l2[q];
    const unsigned char* wt = a.wt + (size_t)q * a.ld;
    const int* node = a.node + (size_t)q * a.ld;
    const long long* qg = a.qg + (size_t)q * a.ld;
    const long long* qh = a.qh + (size_t)q * a.ld;

    for (int fp = f0; fp < f1; fp += gpp) {
        const int ng = min(gpp, f1 - fp), rows = ng * nl;
        if (((admmask >> (fp - f0)) & (ng >= 32 ? 0xffffffffu : (1u << ng) - 1u)) == 0u) continue;      // (uniform) the round admits no gene of this pass
        for (int c = tid; c < rows * B1; c += GBM_THREADS) { hg[c] = 0; hh[c] = 0; hc[c] = 0; }
        __syncthreads();
        if (a.form != MMS_GBM_FORM_PRIVATE) {
            const int rot = wave * ((ng + 3) >> 2);
            for (int base = 0; base < n; base += GBM_THREADS) {
                const int i = base + tid;
                int w = 0, k = -1;
                if (i < n) { w = wt[i]; k = node[i] - s0; }
                const bool ok = w > 0 && k >= 0 && k < nl && ((livemask >> k) & 1u);
                long long g = 0, h = 0;
                if (ok) { g = qg[i] * w; h = qh[i] * w; }
                for (int jj = 0; jj < ng; ++jj) {
                    const int j = (jj + rot) % ng, f = fp + j;
                    if (!((admmask >> (f - f0)) & 1u)) continue;
                    if (ok) {
                        const int b = min((int)a.xb[(size_t)f * a.ld + i], B - 1);
                        const int cell = (j * nl + k) * B1 + b;
                        atomicAdd(&hc[cell], w);
                        atomicAdd((unsigned long long*)&hg[cell], (unsigned long long)g);
                        atomicAdd((unsigned long long*)&hh[cell], (unsigned long long)h);
                    }
                }
            }
        } else {
            for (int l = tid; l < rows; l += GBM_THREADS) {
                const int j = l / nl, k = l - j * nl, f = fp + j;
                if (!((admmask >> (f - f0)) & 1u) || !((livemask >> k) & 1u)) continue;
                const unsigned char* xf = a.xb + (size_t)f * a.ld;
                const int row = l * B1;
                for (int i = 0; i < n; ++i) {
                    const int w = wt[i];
                    if (!w || node[i] != s0 + k) continue;
                    const int cell = row + min((int)xf[i], B - 1);
                    hc[cell] += w; hg[cell] += qg[i] * w; hh[cell] += qh[i] * w;
                }
            }
        }
        __syncthreads();
        // a lane per (feature, node): prefix over the bins, the best admissible cut; the row's first two cells then carry it
        for (int l = tid; l < rows; l += GBM_THREADS) {
            const int j = l / nl, k = l - j * nl, f = fp + j, row = l * B1;
            double best = 0.0;
            int bbin = -1, bn = 0;
            long long bG = 0, bH = 0;
            if (((admmask >> (f - f0)) & 1u) && ((livemask >> k) & 1u)) {
                const int nT = s_n[k];
                const long long GT = s_G[k], HT = s_H[k];
                const double parent = gbm_term(GT, HT, lam);
                int nL = 0;
                long long GL = 0, HL = 0;
                for (int b = 0; b < B; ++b) {
                    nL += hc[row + b]; GL += hg[row + b]; HL += hh[row + b];
                    if (a.t_n) {
                        const size_t o = (((size_t)q * nl + k) * a.p + f) * B + b;
                        a.t_n[o] = nL; a.t_G[o] = GL; a.t_H[o] = HL;
                    }
                    if (b < B - 1 && nL >= ml && nT - nL >= ml) {
                        const double gain = gbm_term(GL, HL, lam) + gbm_term(GT - GL, HT - HL, lam) - parent;
                        if (gain > best) { best = gain; bbin = b; bn = nL; bG = GL; bH = HL; }       // ascending b: the smallest bin keeps a tie
                    }
                }
            }
            hc[row] = bn; hc[row + 1] = bbin; hg[row] = bG; hh[row] = bH; hg[row + 1] = __double_as_longlong(best);
        }
        __syncthreads();
        if (tid < nl && ((livemask >> tid) & 1u)) {
            for (int j = 0; j < ng; ++j) {               // ascending features: the smallest feature keeps a tie
                const int row = (j * nl + tid) * B1;
                if (hc[row + 1] < 0) continue;
                const double gain = __longlong_as_double(hg[row + 1]);
                if (gain > b_gain[tid]) {
                    b_gain[tid] = gain; b_f[tid] = fp + j; b_bin[tid] = hc[row + 1]; b_n[tid] = hc[row]; b_G[tid] = hg[row]; b_H[tid] = hh[row];
                }
            }
        }
        __syncthreads();
    }
    if (tid < nl) {
        const size_t o = ((size_t)q * a.ntiles + tile) * nl + tid;
        a.part_gain[o] = b_gain[tid];
        a.part_cut[4 * o] = b_f[tid]; a.part_cut[4 * o + 1] = b_bin[tid]; a.part_cut[4 * o + 2] = b_n[tid]; a.part_cut[4 * o + 3] = 0;
        a.part_sum[2 * o] = b_G[tid]; a.part_sum[2 * o + 1] = b_H[tid];
    }
}

__global__ __launch_bounds__(GBM_THREADS) void gbm_route_kernel(const GbmSplitP a) {
    __shared__ int sf[GBM_MAX_NODES], sb[GBM_MAX_NODES];
    const int q = blockIdx.x, tid = threadIdx.x, nl = 1 << a.level, s0 = nl - 1;
    if (a.level >= a.depth[q]) return;
    const size_t tb = ((size_t)q * a.M + a.round) * a.nn;
    if (tid < nl) {
        const int s = s0 + tid;
        int bf = -1, bb = 0, bn = 0;
        long long bG = 0, bH = 0;
        double bg = 0.0;
        const int nT = a.n_node[tb + s];
        if ((s == 0 || a.feat[tb + ((s - 1) >> 1)] >= 0) && nT >= 2 * a.min_leaf[q]) {
            for (int t = 0; t < a.ntiles; ++t) {         // ascending tiles: the smallest feature keeps a tie
                const size_t o = ((size_t)q * a.ntiles + t) * nl + tid;
                const int f = a.part_cut[4 * o];
                const double g = a.part_gain[o];
                if (f >= 0 && g > bg) { bg = g; bf = f; bb = a.part_cut[4 * o + 1]; bn = a.part_cut[4 * o + 2]; bG = a.part_sum[2 * o]; bH = a.part_sum[2 * o + 1]; }
            }
            if (bf >= 0 && !(bg > a.min_gain[q])) bf = -1;
        }
        if (bf >= 0) {
            a.feat[tb + s] = bf; a.bin[tb + s] = bb; a.thr[tb + s] = a.edges[(size_t)bf * (a.B - 1) + bb]; a.gain[tb + s] = bg;
            a.n_node[tb + 2 * s + 1] = bn; a.G[tb + 2 * s + 1] = bG; a.H[tb + 2 * s + 1] = bH;
            a.n_node[tb + 2 * s + 2] = nT - bn; a.G[tb + 2 * s + 2] = a.G[tb + s] - bG; a.H[tb + 2 * s + 2] = a.H[tb + s] - bH;
        }
        sf[tid] = bf; sb[tid] = bb;
    }
    __syncthreads();
    int* node = a.node + (size_t)q * a.ld;
    for (int i = tid; i < a.n; i += GBM_THREADS) {
        const int s = node[i], k = s - s0;
        if (k < 0 || k >= nl || sf[k] < 0) continue;
        node[i] = 2 * s + 1 + ((int)a.xb[(size_t)sf[k] * a.ld + i] > sb[k] ? 1 : 0);
    }
}

__global__ __launch_bounds__(GBM_THREADS) void gbm_update_kernel(const GbmUpdateP a) {
    __shared__ double sval[(2 << MMS_GBM_MAX_DEPTH) - 1];
    __shared__ double sF[MMS_GBM_MAX_N];
    __shared__ int sk[MMS_GBM_MAX_N];
    __shared__ long long lred[GBM_THREADS / 64];
    const int q = blockIdx.x, tid = threadIdx.x, n = a.n;
    const size_t tb = ((size_t)q * a.M + a.round) * a.nn;
    if (tid < a.nn) {                                    // (nn <= 127 < 256)
        const bool leaf = (tid == 0 || a.feat[tb + ((tid - 1) >> 1)] >= 0) && a.feat[tb + tid] < 0;
        double v = 0.0;
        if (leaf) {
            v = a.lr[q] * gbm_ratio(a.G[tb + tid], a.H[tb + tid], a.l2[q]);
            a.value[tb + tid] = v;
        }
        sval[tid] = v;
    }
    __syncthreads();
    double* F = a.F + (size_t)q * a.ld;
    const int* node = a.node + (size_t)q * a.ld;
    const unsigned char* em = a.evalm ? a.evalm + (size_t)q * a.ld : nullptr;
    for (int i = tid; i < n; i += GBM_THREADS) {
        const int s = node[i];
        const double f = F[i] + sval[s >= 0 && s < a.nn ? s : 0];
        F[i] = f;
        sF[i] = f;
        sk[i] = (em && em[i]) ? 2 * a.tgroup[i] + (a.event[i] != 0 ? 1 : 0) : GBM_OUT;
    }
    if (!em) return;
    __syncthreads();
    // position i is the shorter time of the comparable pair (i, j) iff it is an event and key_i > key_j (rsf.hip: mms_rsf_vimp)
    long long c2 = 0, cm = 0;
    for (int i = tid; i < n; i += GBM_THREADS) {
        const int ki = sk[i];
        if (!(ki & 1)) continue;
        const double Fi = sF[i];
        int c = 0, m = 0;
        for (int j = 0; j < n; ++j) {
            const double Fj = sF[j];
            const bool cp = ki > sk[j];
            m += cp ? 1 : 0;
            c += cp ? (Fi > Fj ? 2 : Fi == Fj ? 1 : 0) : 0;
        }
        c2 += c; cm += m;
    }
    c2 = gbm_block_sum_ll(c2, lred);
    cm = gbm_block_sum_ll(cm, lred);
    if (tid == 0) { a.conc2[(size_t)q * a.M + a.round] = c2; a.comparable[(size_t)q * a.M + a.round] = cm; }
}

__global__ __launch_bounds__(GBM_THREADS) void gbm_predict_kernel(const GbmPredictP a) {
    const int q = blockIdx.y, r = blockIdx.x * GBM_THREADS + threadIdx.x;
    if (r >= a.R) return;
    const float* x = a.x + (size_t)r * a.ldx;
    double sum = 0.0;
    int kk = 0;
    for (int m = 0; m <= a.M && kk < a.K; ++m) {
        while (kk < a.K && a.at[kk] <= m) { a.out[((size_t)q * a.K + kk) * a.R + r] = sum; ++kk; }
        if (m == a.M) break;
        const size_t tb = ((size_t)q * a.M + m) * a.nn;
        int s = 0;
        for (;;) {
            const int f = a.feat[tb + s];
            if (f < 0 || 2 * s + 2 >= a.nn) break;
            s = 2 * s + 1 + (x[f] <= a.thr[tb + s] ? 0 : 1);
        }
        sum += a.value[tb + s];
    }
}

static inline bool gbm_mis(const void* p, uintptr_t mask) { return ((uintptr_t)p & mask) != 0; }
static inline bool gbm_nn_bad(int nn) { return nn < 1 || nn > (2 << MMS_GBM_MAX_DEPTH) - 1; }

extern "C" int mms_gbm_grad(const GbmGradP* p, hipStream_t s) {
    if (!p || !p->mult || !p->event || !p->tgroup || !p->rowid || !p->subsample || !p->F || !p->loglik) return MMS_ERR_ARG;
    if (!p->last && (!p->qg || !p->qh || !p->wt || !p->node || !p->n_node || !p->G || !p->H)) return MMS_ERR_ARG;
    if (p->n < 1 || p->n > MMS_GBM_MAX_N || p->ld < p->n || p->P < 0 || p->P > MMS_GBM_MAX_P || p->M < 1 || gbm_nn_bad(p->nn)) return MMS_ERR_ARG;
    if (p->round < 0 || p->round > p->M || (p->round == p->M && !p->last)) return MMS_ERR_ARG;
    if (gbm_mis(p->event, 3) || gbm_mis(p->tgroup, 3) || gbm_mis(p->rowid, 3) || gbm_mis(p->pid, 3) || gbm_mis(p->subsample, 3)) return MMS_ERR_ARG;
    if (gbm_mis(p->F, 7) || gbm_mis(p->qg, 7) || gbm_mis(p->qh, 7) || gbm_mis(p->node, 3) || gbm_mis(p->loglik, 7)) return MMS_ERR_ARG;
    if (gbm_mis(p->n_node, 3) || gbm_mis(p->G, 7) || gbm_mis(p->H, 7)) return MMS_ERR_ARG;
    if (p->P == 0) return MMS_OK;
    MMS_LAUNCH(gbm_grad_kernel, dim3(p->P), dim3(GBM_THREADS), 0, s, *p);
    return mms_check_launch();
}

extern "C" int mms_gbm_split(const GbmSplitP* p, hipStream_t s) {
    if (!p || !p->xb || !p->wt || !p->qg || !p->qh || !p->edges || !p->depth || !p->min_leaf || !p->l2 || !p->min_gain || !p->colsample)
        return MMS_ERR_ARG;
    if (!p->node || !p->feat || !p->bin || !p->thr || !p->gain || !p->n_node || !p->G || !p->H || !p->part_gain || !p->part_cut || !p->part_sum)
        return MMS_ERR_ARG;
    if (p->n < 1 || p->n > MMS_GBM_MAX_N || p->ld < p->n || p->p < 1 || p->P < 0 || p->P > MMS_GBM_MAX_P) return MMS_ERR_ARG;
    if (p->B < 2 || p->B > MMS_GBM_MAX_BINS || p->M < 1 || p->round < 0 || p->round >= p->M) return MMS_ERR_ARG;
    if (p->level < 0 || p->level >= MMS_GBM_MAX_DEPTH || gbm_nn_bad(p->nn) || p->nn < (4 << p->level) - 1) return MMS_ERR_ARG;
    if (p->form < 0 || p->form > MMS_GBM_FORM_PRIVATE) return MMS_ERR_ARG;
    if (p->ntiles != (p->p + MMS_GBM_TILE - 1) / MMS_GBM_TILE || p->ntiles > 65535) return MMS_ERR_ARG;
    const bool tr = p->t_n || p->t_G || p->t_H;
    if (tr && (!p->t_n || !p->t_G || !p->t_H)) return MMS_ERR_ARG;
    if (gbm_mis(p->qg, 7) || gbm_mis(p->qh, 7) || gbm_mis(p->edges, 3) || gbm_mis(p->depth, 3) || gbm_mis(p->min_leaf, 3)) return MMS_ERR_ARG;
    if (gbm_mis(p->l2, 7) || gbm_mis(p->min_gain, 7) || gbm_mis(p->colsample, 3) || gbm_mis(p->pid, 3) || gbm_mis(p->node, 3)) return MMS_ERR_ARG;
    if (gbm_mis(p->feat, 3) || gbm_mis(p->bin, 3) || gbm_mis(p->thr, 3) || gbm_mis(p->gain, 7) || gbm_mis(p->n_node, 3)) return MMS_ERR_ARG;
    if (gbm_mis(p->G, 7) || gbm_mis(p->H, 7) || gbm_mis(p->part_gain, 7) || gbm_mis(p->part_cut, 3) || gbm_mis(p->part_sum, 7)) return MMS_ERR_ARG;
    if (gbm_mis(p->t_n, 3) || gbm_mis(p->t_G, 7) || gbm_mis(p->t_H, 7)) return MMS_ERR_ARG;
    const int per = (1 << p->level) * (p->B + 1);         // cells a feature: <= 32 * 65 = 2080 <= MMS_GBM_LDS_CELLS
    if (per > MMS_GBM_LDS_CELLS) return MMS_ERR_ARG;
    if (p->P == 0) return MMS_OK;
    const int gpp = MMS_GBM_LDS_CELLS / per < MMS_GBM_TILE ? MMS_GBM_LDS_CELLS / per : MMS_GBM_TILE;
    const size_t lds = (size_t)gpp * per * (2 * sizeof(long long) + sizeof(int));
    MMS_LAUNCH(gbm_hist_kernel, dim3(p->ntiles, p->P), dim3(GBM_THREADS), lds, s, *p, gpp);
    MMS_LAUNCH(gbm_route_kernel, dim3(p->P), dim3(GBM_THREADS), 0, s, *p);
    return mms_check_launch();
}

extern "C" int mms_gbm_update(const GbmUpdateP* p, hipStream_t s) {
    if (!p || !p->node || !p->event || !p->tgroup || !p->lr || !p->l2 || !p->feat || !p->G || !p->H || !p->value || !p->F) return MMS_ERR_ARG;
    if (p->evalm && (!p->conc2 || !p->comparable)) return MMS_ERR_ARG;
    if (p->n < 1 || p->n > MMS_GBM_MAX_N || p->ld < p->n || p->P < 0 || p->P > MMS_GBM_MAX_P || p->M < 1 || gbm_nn_bad(p->nn)) return MMS_ERR_ARG;
    if (p->round < 0 || p->round >= p->M) return MMS_ERR_ARG;
    if (gbm_mis(p->node, 3) || gbm_mis(p->event, 3) || gbm_mis(p->tgroup, 3) || gbm_mis(p->lr, 7) || gbm_mis(p->l2, 7) || gbm_mis(p->feat, 3)) return MMS_ERR_ARG;
    if (gbm_mis(p->G, 7) || gbm_mis(p->H, 7) || gbm_mis(p->value, 7) || gbm_mis(p->F, 7) || gbm_mis(p->conc2, 7) || gbm_mis(p->comparable, 7)) return MMS_ERR_ARG;
    if (p->P == 0) return MMS_OK;
    MMS_LAUNCH(gbm_update_kernel, dim3(p->P), dim3(GBM_THREADS), 0, s, *p);
    return mms_check_launch();
}

extern "C" int mms_gbm_predict(const GbmPredictP* p, hipStream_t s) {
    if (!p || !p->x || !p->feat || !p->thr || !p->value || !p->at || !p->out) return MMS_ERR_ARG;
    if (p->R < 0 || p->p < 1 || p->ldx < p->p || p->P < 0 || p->P > MMS_GBM_MAX_P || p->M < 1 || gbm_nn_bad(p->nn) || p->K < 1) return MMS_ERR_ARG;
    if (gbm_mis(p->x, 3) || gbm_mis(p->feat, 3) || gbm_mis(p->thr, 3) || gbm_mis(p->value, 7) || gbm_mis(p->at, 3) || gbm_mis(p->out, 7)) return MMS_ERR_ARG;
    if (p->R == 0 || p->P == 0) return MMS_OK;
    MMS_LAUNCH(gbm_predict_kernel, dim3((p->R + GBM_THREADS - 1) / GBM_THREADS, p->P), dim3(GBM_THREADS), 0, s, *p);
    return mms_check_launch();
}
