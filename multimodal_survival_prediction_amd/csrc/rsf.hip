// Random survival forest: T trees grown level by level in lock-step (include/mmsurv.h: RsfSplitP, RsfLeavesP, RsfPredictP).
//
// mms_rsf_split -- one launch per level; workgroup = (tree, node of the level), lane = candidate split.  The workgroup compacts the
// node's in-bag members in position (time-descending) order into LDS: {position | mult << 16 | event << 24 | [tie group with events ends
// here] << 25}, the weighted members up to and including the member, and at the end of each tie group with events the two fp64
// coefficients d / Y and d (Y - d) / (Y Y (Y - 1)) of THIS node.  A lane then walks the list the way logrank_scan.hip's lr_step does:
// the member word is one broadcast LDS read, its covariate one global read inside the candidate's feature row (the nsplit lanes of a
// feature share the address), the left child's members and events are integer adds, and the fp64 terms run only where a tie group with
// events ends (a wave-uniform branch).  The argmax is an in-block reduction in a fixed order; the workgroup that chose the split also
// routes its own members to the children -- they are in its LDS already, and no other workgroup of the level reads their node words for
// anything but a comparison with its own node number, which neither the old nor the new value equals.
// mms_rsf_leaves -- workgroup = tree, lane = node: a leaf's lane walks the tree's positions (staged in LDS, broadcast reads) once.
// mms_rsf_predict -- workgroup = row, lane = trees j, j + 256, ...
// mms_rsf_vimp -- workgroup = (problem, repeat) of the permutation importance; lane = rows i, i + 256, ...: the row's delta sum over the
// problem's trees (two walks a tree, the second reading the donor's value at the problem's gene), then M and the pair key
// 2 tgroup + event into LDS and the pair count of the C-index from there (broadcast reads), folded in a fixed order.
// No atomics, plain stores; a tree's bits depend on its own multiplicity row and hash stream only.
#include "common.h"

#define RSF_THREADS 256
#define RSF_NONE 0x7fffffff

__device__ __forceinline__ uint32_t rsf_tree_key(uint32_t seed, uint32_t id) { return hash_u32(seed ^ (id * 0x85ebca6bU)); }
__device__ __forceinline__ uint32_t rsf_node_key(uint32_t ht, uint32_t s) { return hash_u32((s + 1u) * 0x9E3779B9U + ht); }
__device__ __forceinline__ uint32_t rsf_feat_key(uint32_t hn, uint32_t j) { return hash_u32((j + 1u) * 0x9E3779B9U + hn); }
__device__ __forceinline__ uint32_t rsf_thr_key(uint32_t hf, uint32_t q) { return hash_u32((q + 1u) * 0x85ebca6bU + hf); }

struct RsfAcc { int yl, dl; double e, v; };

__device__ __forceinline__ void rsf_step(RsfAcc& t, unsigned en, float x, float thr, const double2* hc, const int* cy) {
    const unsigned u = (unsigned)__builtin_amdgcn_readfirstlane((int)en);
    const int w = (int)((u >> 16) & 0xffu);
    const bool in = x <= thr;
    t.yl += in ? w : 0;
    t.dl += (in && (u & (1u << 24))) ? w : 0;
    if (u & (1u << 25)) {
        const double2 k = *hc;
        const double g = (double)t.yl;
        t.e = fma(k.x, g, t.e);
        t.v = fma(k.y * g, (double)*cy - g, t.v);
    }
}

__global__ __launch_bounds__(RSF_THREADS) void rsf_split_kernel(const RsfSplitP a) {
    extern __shared__ __align__(16) unsigned char rsf_dyn[];
    __shared__ unsigned sh_w0[RSF_THREADS / 64], sh_w1[RSF_THREADS / 64];
    __shared__ double sh_x[RSF_THREADS];
    __shared__ int sh_i[RSF_THREADS];
    __shared__ int sh_win[2];
    const int n = a.n, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double2* hc = (double2*)rsf_dyn;                     // [n]
    unsigned* ent = (unsigned*)(hc + n);                 // [n]
    int* cy = (int*)(ent + n);                           // [n] weighted members up to and including the member
    int* cd = cy + n;                                    // [n] weighted events up to and including the member
    const int nl = 1 << a.level;
    const int t = (int)(blockIdx.x >> a.level), s = nl - 1 + (int)(blockIdx.x & (unsigned)(nl - 1));
    const size_t tb = (size_t)t * a.nn;
    if (s > 0) {
        if (a.feat[tb + ((s - 1) >> 1)] < 0) return;     // the parent recorded no split: the node is absent
        if (a.n_node[tb + s] < 2 * a.min_leaf) return;   // too small to try: a leaf (feat stays -1)
    }
    const unsigned char* mult = a.mult + (size_t)t * a.ld;
    int* node = a.node + (size_t)t * a.ld;

    // the node's members in position order, with running weighted members / events
    int m = 0, Yb = 0, Db = 0;
    for (int base = 0; base < n; base += RSF_THREADS) {
        const int i = base + tid;
        int w = 0, e = 0;
        if (i < n) {
            w = mult[i];
            if (w && node[i] != s) w = 0;
            if (w) e = a.event[i] != 0;
        }
        unsigned v0 = (w ? 1u : 0u) | ((unsigned)w << 16), v1 = (unsigned)(w * e);      // (256 members, 256 * 255 in a half each)
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned t0 = __shfl_up(v0, o, 64), t1 = __shfl_up(v1, o, 64);
            if (lane >= o) { v0 += t0; v1 += t1; }
        }
        if (lane == 63) { sh_w0[wave] = v0; sh_w1[wave] = v1; }
        __syncthreads();
        unsigned p0 = 0, p1 = 0, tot0 = 0, tot1 = 0;
        for (int q = 0; q < RSF_THREADS / 64; ++q) {
            const unsigned b0 = sh_w0[q], b1 = sh_w1[q];
            if (q < wave) { p0 += b0; p1 += b1; }
            tot0 += b0; tot1 += b1;
        }
        if (w) {
            const int k = m + (int)((p0 + v0) & 0xffffu) - 1;
            ent[k] = (unsigned)i | ((unsigned)w << 16) | ((unsigned)e << 24);
            cy[k] = Yb + (int)((p0 + v0) >> 16);
            cd[k] = Db + (int)(p1 + v1);
        }
        m += (int)(tot0 & 0xffffu); Yb += (int)(tot0 >> 16); Db += (int)tot1;
        __syncthreads();
    }
    if (s == 0 && tid == 0) { a.n_node[tb] = Yb; a.d_node[tb] = Db; }
    if (m == 0 || Yb < 2 * a.min_leaf) return;           // (uniform; s > 0 never gets here with either)

    // coefficients at the last member of each tie group with events
    for (int k = tid; k < m; k += RSF_THREADS) {
        const int g = a.tgroup[ent[k] & 0xffffu];
        double2 c = make_double2(0.0, 0.0);
        if (k == m - 1 || a.tgroup[ent[k + 1] & 0xffffu] != g) {
            int j = k - 1;
            while (j >= 0 && a.tgroup[ent[j] & 0xffffu] == g) --j;
            const int d = cd[k] - (j >= 0 ? cd[j] : 0);
            if (d > 0) {
                const double Y = (double)cy[k], dd = (double)d;
                c.x = dd / Y;
                c.y = Y > 1.0 ? (dd * (Y - dd)) / (Y * Y * (Y - 1.0)) : 0.0;
            }
        }
        hc[k] = c;
    }
    __syncthreads();
    for (int k = tid; k < m; k += RSF_THREADS)
        if (hc[k].x != 0.0) ent[k] |= 1u << 25;
    __syncthreads();

    const int C = a.mtry * a.nsplit;
    const uint32_t hn = rsf_node_key(rsf_tree_key(a.seed, (uint32_t)(a.tree_id ? a.tree_id[t] : t)), (uint32_t)s);
    double best = 0.0;                                   // a winner needs chi2 > 0
    int besti = RSF_NONE, bestf = 0, bestn = 0, bestd = 0;
    float bestthr = 0.f;
    for (int cb = 0; cb < C; cb += RSF_THREADS) {
        if (cb + (tid & ~63) >= C) continue;             // this wave has no candidate in the chunk (wave-uniform)
        const int c = cb + tid;
        const bool cv = c < C;
        const int j = cv ? c / a.nsplit : 0, q = cv ? c - j * a.nsplit : 0;
        const uint32_t hf = rsf_feat_key(hn, (uint32_t)j);
        const int f = (int)__umulhi(hf, (uint32_t)a.p);
        const int r = (int)__umulhi(rsf_thr_key(hf, (uint32_t)q), (uint32_t)m);
        const float* row = a.xt + (size_t)f * a.ld;
        const float thr = row[ent[r] & 0xffffu];
        RsfAcc acc{0, 0, 0.0, 0.0};
        int k = 0;
        for (; k + 4 <= m; k += 4) {
            const unsigned e0 = ent[k], e1 = ent[k + 1], e2 = ent[k + 2], e3 = ent[k + 3];
            const float x0 = row[e0 & 0xffffu], x1 = row[e1 & 0xffffu], x2 = row[e2 & 0xffffu], x3 = row[e3 & 0xffffu];
            rsf_step(acc, e0, x0, thr, hc + k, cy + k);
            rsf_step(acc, e1, x1, thr, hc + k + 1, cy + k + 1);
            rsf_step(acc, e2, x2, thr, hc + k + 2, cy + k + 2);
            rsf_step(acc, e3, x3, thr, hc + k + 3, cy + k + 3);
        }
        for (; k < m; ++k) { const unsigned e0 = ent[k]; rsf_step(acc, e0, row[e0 & 0xffffu], thr, hc + k, cy + k); }
        const double u = (double)acc.dl - acc.e, v = acc.v;
        const double x = v > 0.0 ? u * u / v : 0.0;
        if (cv) {
            if (a.U) {
                const size_t o = (size_t)blockIdx.x * a.ldo + c;
                a.U[o] = u; a.V[o] = v; a.n_left[o] = acc.yl; a.d_left[o] = acc.dl;
            }
            if (acc.yl >= a.min_leaf && Yb - acc.yl >= a.min_leaf && x > best) {      // ascending c: the smallest index keeps a tie
                best = x; besti = c; bestf = f; bestthr = thr; bestn = acc.yl; bestd = acc.dl;
            }
        }
    }
    sh_x[tid] = best; sh_i[tid] = besti;
    __syncthreads();
    for (int w = RSF_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w) {
            const double x = sh_x[tid + w];
            const int j = sh_i[tid + w];
            if (x > sh_x[tid] || (x == sh_x[tid] && j < sh_i[tid])) { sh_x[tid] = x; sh_i[tid] = j; }
        }
        __syncthreads();
    }
    const int win = sh_i[0];
    if (win == RSF_NONE) {
        if (tid == 0) { a.feat[tb + s] = -1; a.thr[tb + s] = 0.f; a.stat[tb + s] = 0.0; }
        return;
    }
    if (besti == win) {                                  // one thread owns the winning candidate
        a.feat[tb + s] = bestf; a.thr[tb + s] = bestthr; a.stat[tb + s] = best;
        a.n_node[tb + 2 * s + 1] = bestn; a.d_node[tb + 2 * s + 1] = bestd;
        a.n_node[tb + 2 * s + 2] = Yb - bestn; a.d_node[tb + 2 * s + 2] = Db - bestd;
        sh_win[0] = bestf; sh_win[1] = __float_as_int(bestthr);
    }
    __syncthreads();
    const float* row = a.xt + (size_t)sh_win[0] * a.ld;
    const float thr = __int_as_float(sh_win[1]);
    for (int k = tid; k < m; k += RSF_THREADS) {
        const int i = (int)(ent[k] & 0xffffu);
        node[i] = 2 * s + 1 + (row[i] <= thr ? 0 : 1);
    }
}

__global__ __launch_bounds__(RSF_THREADS) void rsf_leaves_kernel(const RsfLeavesP a) {
    __shared__ unsigned sh_e[MMS_RSF_MAX_N];             // node | mult << 16 | event << 24
    __shared__ int sh_g[MMS_RSF_MAX_N];
    __shared__ int sh_h[MMS_RSF_MAX_H];
    const int t = blockIdx.x, tid = threadIdx.x, n = a.n, nh = a.nh;
    const unsigned char* mult = a.mult + (size_t)t * a.ld;
    const int* node = a.node + (size_t)t * a.ld;
    const double* wrow = a.weight + (size_t)(a.wset ? a.wset[t] : 0) * a.ld;
    for (int i = tid; i < n; i += RSF_THREADS) {
        const unsigned w = mult[i];
        sh_e[i] = w ? ((unsigned)node[i] & 0xffffu) | (w << 16) | ((a.event[i] != 0 ? 1u : 0u) << 24) : 0xffffu;
        sh_g[i] = a.tgroup[i];
    }
    if (tid < nh) sh_h[tid] = a.hpos[tid];
    __syncthreads();
    const size_t tb = (size_t)t * a.nn;
    for (int base = 0; base < a.nn; base += RSF_THREADS) {
        const int s = base + tid;
        const bool leaf = s < a.nn && a.feat[tb + s] < 0 && a.n_node[tb + s] > 0;
        if (!__any(leaf)) continue;
        double H[MMS_RSF_MAX_H];
#pragma unroll
        for (int h = 0; h < MMS_RSF_MAX_H; ++h) H[h] = 0.0;
        double mort = 0.0;
        int Y = 0, dg = 0, curg = -1, gpos = 0;
        const unsigned me = leaf ? (unsigned)s : 0xfffeu;           // (no word names node 0xfffe: nn <= 8191)
        for (int i = 0; i <= n; ++i) {
            const bool last = i == n;
            const unsigned en = last ? 0u : sh_e[i];
            const bool mine = !last && (en & 0xffffu) == me;
            const int g = last ? -2 : sh_g[i];
            if ((mine && g != curg) || last) {                       // the group before this member is complete
                if (dg > 0) {
                    const double term = (double)dg / (double)Y;
                    mort += term * wrow[gpos];
#pragma unroll
                    for (int h = 0; h < MMS_RSF_MAX_H; ++h)
                        if (h < nh && gpos >= sh_h[h]) H[h] += term;
                }
                curg = g; dg = 0; gpos = i;
            }
            if (mine) {
                const int w = (int)((en >> 16) & 0xffu);
                Y += w;
                dg += (en & (1u << 24)) ? w : 0;
            }
        }
        if (leaf) {
            a.mort[tb + s] = mort;
#pragma unroll
            for (int h = 0; h < MMS_RSF_MAX_H; ++h)
                if (h < nh) a.H[(tb + s) * nh + h] = H[h];
        }
    }
}

__global__ __launch_bounds__(RSF_THREADS) void rsf_predict_kernel(const RsfPredictP a) {
    __shared__ double sh_r[RSF_THREADS];
    const int r = blockIdx.x, tid = threadIdx.x, nh = a.nh;
    const float* x = a.x + (size_t)r * a.ldx;
    double H[MMS_RSF_MAX_H];
#pragma unroll
    for (int h = 0; h < MMS_RSF_MAX_H; ++h) H[h] = 0.0;
    double mort = 0.0;
    int cnt = 0;
    for (int t = tid; t < a.T; t += RSF_THREADS) {
        if (a.use && !a.use[(size_t)t * a.ldu + r]) continue;
        const size_t tb = (size_t)t * a.nn;
        int s = 0;
        for (;;) {
            const int f = a.feat[tb + s];
            if (f < 0 || 2 * s + 2 >= a.nn) break;
            s = 2 * s + 1 + (x[f] <= a.thr[tb + s] ? 0 : 1);
        }
        mort += a.mort[tb + s];
#pragma unroll
        for (int h = 0; h < MMS_RSF_MAX_H; ++h)
            if (h < nh) H[h] += a.H[(tb + s) * nh + h];
        ++cnt;
    }
    // the 256 partial sums of every quantity, folded in a fixed order: quantity 0 = count, 1 = mortality, 2 + h = H[h]
    double total = 0.0;
    for (int qn = 0; qn < nh + 2; ++qn) {
        double v = qn == 0 ? (double)cnt : mort;
#pragma unroll
        for (int h = 0; h < MMS_RSF_MAX_H; ++h)
            if (qn == h + 2) v = H[h];
        __syncthreads();
        sh_r[tid] = v;
        __syncthreads();
        for (int w = RSF_THREADS / 2; w > 0; w >>= 1) {
            if (tid < w) sh_r[tid] += sh_r[tid + w];
            __syncthreads();
        }
        if (tid == 0) {
            const double sum = sh_r[0];
            if (qn == 0) { total = sum; a.count[r] = (int)sum; }
            else {
                const double mean = total > 0.0 ? sum / total : __longlong_as_double(0x7ff8000000000000LL);
                if (qn == 1) a.out_mort[r] = mean; else a.out_H[(size_t)r * nh + (qn - 2)] = mean;
            }
        }
    }
}

#define RSF_VIMP_OUT 0x7ffffffe                              // an even key no other key exceeds: such a row is in no comparable pair

__device__ __forceinline__ int rsf_walk_with(const int* feat, const float* thr, int nn, const float* x, int g, float xg) {
    int s = 0;
    for (;;) {
        const int f = feat[s];
        if (f < 0 || 2 * s + 2 >= nn) break;
        s = 2 * s + 1 + ((f == g ? xg : x[f]) <= thr[s] ? 0 : 1);
    }
    return s;
}

__global__ __launch_bounds__(RSF_THREADS) void rsf_vimp_kernel(const RsfVimpP a) {
    extern __shared__ __align__(16) unsigned char rsf_dyn[];
    __shared__ long long sh_c[RSF_THREADS], sh_m[RSF_THREADS];
    const int n = a.n, tid = threadIdx.x;
    double* sh_M = (double*)rsf_dyn;                     // [n]
    int* sh_k = (int*)(sh_M + n);                        // [n] 2 tgroup + event, RSF_VIMP_OUT for a row outside the problem
    const int q = (int)(blockIdx.x / (unsigned)a.R), r = (int)(blockIdx.x - (unsigned)q * (unsigned)a.R);
    const int f = a.pset[q], g = a.pgene[q], k0 = a.poff[q], k1 = a.poff[q + 1];
    const double* M0 = a.M0 + (size_t)f * a.ld;
    const int* cnt = a.cnt + (size_t)f * a.ld;
    const int* donor = a.donor + (size_t)r * a.T * a.ldu;
    for (int i = tid; i < n; i += RSF_THREADS) {
        const int c = cnt[i];
        double D = 0.0, M = M0[i];
        int key = RSF_VIMP_OUT;
        if (c > 0) {
            const float* xi = a.x + (size_t)i * a.ldx;
            const float xg = xi[g];
            for (int k = k0; k < k1; ++k) {              // ascending trees, one sequential fp64 sum: the contract
                const int t = a.ptree[k];
                if (!a.use[(size_t)t * a.ldu + i]) continue;
                const size_t tb = (size_t)t * a.nn;
                const float xd = a.x[(size_t)donor[(size_t)t * a.ldu + i] * a.ldx + g];
                const int l0 = rsf_walk_with(a.feat + tb, a.thr + tb, a.nn, xi, g, xg);
                const int l1 = rsf_walk_with(a.feat + tb, a.thr + tb, a.nn, xi, g, xd);
                D += a.mort[tb + l1] - a.mort[tb + l0];
            }
            M = M + D / (double)c;
            key = 2 * a.tgroup[i] + (a.event[i] != 0 ? 1 : 0);
        }
        sh_M[i] = M; sh_k[i] = key;
        if (a.D) a.D[(size_t)blockIdx.x * a.ld + i] = D;
        if (a.M) a.M[(size_t)blockIdx.x * a.ld + i] = M;
    }
    __syncthreads();
    // row i is the shorter time of the comparable pair (i, j) iff it is an event and key_i > key_j
    long long c2 = 0, cm = 0;
    for (int i = tid; i < n; i += RSF_THREADS) {
        const int ki = sh_k[i];
        if (!(ki & 1)) continue;
        const double Mi = sh_M[i];
        int c = 0, m = 0;                                // at most 2 n each
        for (int j = 0; j < n; ++j) {
            const double Mj = sh_M[j];
            const bool cp = ki > sh_k[j];
            m += cp ? 1 : 0;
            c += cp ? (Mi > Mj ? 2 : Mi == Mj ? 1 : 0) : 0;
        }
        c2 += c; cm += m;
    }
    sh_c[tid] = c2; sh_m[tid] = cm;
    __syncthreads();
    for (int w = RSF_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w) { sh_c[tid] += sh_c[tid + w]; sh_m[tid] += sh_m[tid + w]; }
        __syncthreads();
    }
    if (tid == 0) { a.conc2[blockIdx.x] = sh_c[0]; a.comparable[blockIdx.x] = sh_m[0]; }
}

static inline bool rsf_mis(const void* p, uintptr_t mask) { return ((uintptr_t)p & mask) != 0; }

extern "C" int mms_rsf_split(const RsfSplitP* p, hipStream_t s) {
    if (!p || !p->xt || !p->mult || !p->event || !p->tgroup || !p->node || !p->feat || !p->thr || !p->stat || !p->n_node || !p->d_node)
        return MMS_ERR_ARG;
    if (p->n < 1 || p->n > MMS_RSF_MAX_N || p->ld < p->n || p->p < 1 || p->T < 0 || p->T > MMS_RSF_MAX_T) return MMS_ERR_ARG;
    if (p->level < 0 || p->level >= MMS_RSF_MAX_DEPTH || p->nn < (4 << p->level) - 1 || p->nn > (2 << MMS_RSF_MAX_DEPTH) - 1) return MMS_ERR_ARG;
    if (p->mtry < 1 || p->nsplit < 1 || p->min_leaf < 1 || (long long)p->mtry * p->nsplit > MMS_RSF_MAX_C) return MMS_ERR_ARG;
    const bool tab = p->U || p->V || p->n_left || p->d_left;
    if (tab && (!p->U || !p->V || !p->n_left || !p->d_left || p->ldo < p->mtry * p->nsplit)) return MMS_ERR_ARG;
    if (rsf_mis(p->xt, 3) || rsf_mis(p->event, 3) || rsf_mis(p->tgroup, 3) || rsf_mis(p->tree_id, 3) || rsf_mis(p->node, 3)) return MMS_ERR_ARG;
    if (rsf_mis(p->feat, 3) || rsf_mis(p->thr, 3) || rsf_mis(p->stat, 7) || rsf_mis(p->n_node, 3) || rsf_mis(p->d_node, 3)) return MMS_ERR_ARG;
    if (rsf_mis(p->U, 7) || rsf_mis(p->V, 7) || rsf_mis(p->n_left, 3) || rsf_mis(p->d_left, 3)) return MMS_ERR_ARG;
    if (p->T == 0) return MMS_OK;
    const size_t lds = (size_t)p->n * (sizeof(double2) + sizeof(unsigned) + 2 * sizeof(int));
    MMS_LAUNCH(rsf_split_kernel, dim3((unsigned)p->T << p->level), dim3(RSF_THREADS), lds, s, *p);
    return mms_check_launch();
}

extern "C" int mms_rsf_leaves(const RsfLeavesP* p, hipStream_t s) {
    if (!p || !p->mult || !p->event || !p->tgroup || !p->node || !p->feat || !p->n_node || !p->weight || !p->mort || !p->H) return MMS_ERR_ARG;
    if (p->n < 1 || p->n > MMS_RSF_MAX_N || p->ld < p->n || p->T < 0 || p->T > MMS_RSF_MAX_T) return MMS_ERR_ARG;
    if (p->nn < 1 || p->nn > (2 << MMS_RSF_MAX_DEPTH) - 1 || p->nh < 0 || p->nh > MMS_RSF_MAX_H || p->F < 1) return MMS_ERR_ARG;
    if (p->nh > 0 && !p->hpos) return MMS_ERR_ARG;
    if (rsf_mis(p->event, 3) || rsf_mis(p->tgroup, 3) || rsf_mis(p->node, 3) || rsf_mis(p->feat, 3) || rsf_mis(p->n_node, 3)) return MMS_ERR_ARG;
    if (rsf_mis(p->weight, 7) || rsf_mis(p->wset, 3) || rsf_mis(p->hpos, 3) || rsf_mis(p->mort, 7) || rsf_mis(p->H, 7)) return MMS_ERR_ARG;
    if (p->T == 0) return MMS_OK;
    MMS_LAUNCH(rsf_leaves_kernel, dim3(p->T), dim3(RSF_THREADS), 0, s, *p);
    return mms_check_launch();
}

extern "C" int mms_rsf_predict(const RsfPredictP* p, hipStream_t s) {
    if (!p || !p->x || !p->feat || !p->thr || !p->mort || !p->H || !p->out_mort || !p->out_H || !p->count) return MMS_ERR_ARG;
    if (p->R < 0 || p->p < 1 || p->ldx < p->p || p->T < 0 || p->T > MMS_RSF_MAX_T) return MMS_ERR_ARG;
    if (p->nn < 1 || p->nn > (2 << MMS_RSF_MAX_DEPTH) - 1 || p->nh < 0 || p->nh > MMS_RSF_MAX_H) return MMS_ERR_ARG;
    if (p->use && p->ldu < p->R) return MMS_ERR_ARG;
    if (rsf_mis(p->x, 3) || rsf_mis(p->feat, 3) || rsf_mis(p->thr, 3) || rsf_mis(p->mort, 7) || rsf_mis(p->H, 7)) return MMS_ERR_ARG;
    if (rsf_mis(p->out_mort, 7) || rsf_mis(p->out_H, 7) || rsf_mis(p->count, 3)) return MMS_ERR_ARG;
    if (p->R == 0) return MMS_OK;
    MMS_LAUNCH(rsf_predict_kernel, dim3(p->R), dim3(RSF_THREADS), 0, s, *p);
    return mms_check_launch();
}

extern "C" int mms_rsf_vimp(const RsfVimpP* p, hipStream_t s) {
    if (!p || !p->x || !p->feat || !p->thr || !p->mort || !p->use || !p->donor || !p->M0 || !p->cnt || !p->event || !p->tgroup) return MMS_ERR_ARG;
    if (!p->pset || !p->pgene || !p->poff || !p->ptree || !p->conc2 || !p->comparable) return MMS_ERR_ARG;
    if (p->n < 1 || p->n > MMS_RSF_MAX_N || p->ldu < p->n || p->ld < p->n || p->p < 1 || p->ldx < p->p) return MMS_ERR_ARG;
    if (p->T < 0 || p->T > MMS_RSF_MAX_T || p->nn < 1 || p->nn > (2 << MMS_RSF_MAX_DEPTH) - 1 || p->F < 1) return MMS_ERR_ARG;
    if (p->R < 1 || p->R > MMS_RSF_VIMP_MAX_R || p->P < 0 || (long long)p->P * p->R > 0x7fffffffLL) return MMS_ERR_ARG;
    if (rsf_mis(p->x, 3) || rsf_mis(p->feat, 3) || rsf_mis(p->thr, 3) || rsf_mis(p->mort, 7) || rsf_mis(p->donor, 3) || rsf_mis(p->M0, 7)) return MMS_ERR_ARG;
    if (rsf_mis(p->cnt, 3) || rsf_mis(p->event, 3) || rsf_mis(p->tgroup, 3) || rsf_mis(p->pset, 3) || rsf_mis(p->pgene, 3)) return MMS_ERR_ARG;
    if (rsf_mis(p->poff, 3) || rsf_mis(p->ptree, 3) || rsf_mis(p->conc2, 7) || rsf_mis(p->comparable, 7) || rsf_mis(p->D, 7) || rsf_mis(p->M, 7)) return MMS_ERR_ARG;
    if (p->P == 0 || p->T == 0) return MMS_OK;
    const size_t lds = (size_t)p->n * (sizeof(double) + sizeof(int));
    MMS_LAUNCH(rsf_vimp_kernel, dim3((unsigned)p->P * (unsigned)p->R), dim3(RSF_THREADS), lds, s, *p);
    return mms_check_launch();
}
