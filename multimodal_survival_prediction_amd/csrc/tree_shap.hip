// Path-dependent TreeSHAP of heap-indexed tree tables (include/mmsurv.h: TreeShapP) -- the boosted Cox trees' and the survival forest's.
//
// mms_tree_shap -- workgroup = one wave = (group, 64 rows), lane = row.  The wave walks its group's trees in table order and each tree
// depth-first, left-first.  The walk, the path (feature, zero fraction z, output slot of every edge), the merge of edges that share a
// feature and the Shapley weights are wave-uniform; a lane owns one bit per path depth (its side at that split node), from which every
// one indicator o of a leaf follows by mask compares.  Per leaf and unique feature j the polynomial prod_{m != j} (z_m + o_m t) is
// built directly (no division by a path weight, no unwind), so the only division is cover[child] / cover[parent].
//
// Every per-lane or per-path array (D coefficients, D edges) is indexed by unrolled loop counters only -- a write at the running depth
// is a predicated sweep -- so the arrays stay in registers: the kernel is instantiated on the depth bound D (6: nn <= 127, the
// boosters' tables; 12: the forest's) and must show no scratch in the resource remarks of either.
//
// phi is slot-major, [G][U][ldr]: a (leaf, feature) update is one coalesced fp64 load / add / store by the admitted lanes of the rows
// this wave alone owns.  No atomics, no workgroup waits for another, and a row's bits depend only on its group's trees and its own x.
// The tree tables are read through wave-uniform addresses, a node's entries in one batch; staging a tree's live part in LDS was not
// built, so that choice is not measured.
#include "common.h"

#define SHAP_WAVE 64

// w[u][k] = k! (u - k - 1)! / u!, one correctly rounded division of two exact integers (12! < 2^53)
struct ShapWeights { double w[MMS_SHAP_MAX_DEPTH + 1][MMS_SHAP_MAX_DEPTH]; };
static constexpr double shap_fact(int n) { return n <= 1 ? 1.0 : (double)n * shap_fact(n - 1); }
static constexpr ShapWeights shap_weights() {
    ShapWeights t{};
    for (int u = 1; u <= MMS_SHAP_MAX_DEPTH; ++u)
        for (int k = 0; k < u; ++k) t.w[u][k] = shap_fact(k) * shap_fact(u - k - 1) / shap_fact(u);
    return t;
}
__constant__ ShapWeights shap_w = shap_weights();

template <int D>
__global__ __launch_bounds__(SHAP_WAVE) void tree_shap_kernel(const TreeShapP a, const int tiles) {
    const int g = blockIdx.x / tiles, r = (blockIdx.x % tiles) * SHAP_WAVE + threadIdx.x;
    const bool live = r < a.R;
    const int rr = live ? r : a.R - 1;                               // a lane past the last row reads the last row and writes nothing
    const float* x = a.x + (size_t)rr * a.ldx;
    double* phi = a.phi + (size_t)g * a.U * a.ldr + rr;
    if (live)
        for (int sl = 0; sl < a.U; ++sl) phi[(size_t)sl * a.ldr] = 0.0;
    double base = 0.0;
    const int t1 = a.goff[g + 1];
    for (int t = a.goff[g]; t < t1; ++t) {
        const size_t tb = (size_t)t * a.nn;
        const bool adm = live && (a.use == nullptr || a.use[(size_t)t * a.ldu + rr] != 0);
        // the path: edge k leaves the split node of depth k.  pf feature, pz zero fraction, ps output slot, fi first edge with pf
        int pf[D], ps[D], fi[D];
        double pz[D], pr[D];                                         // pz: z of the edge on the path; pr: z of its right sibling, kept for the way back
#pragma unroll
        for (int k = 0; k < D; ++k) { pf[k] = -1; ps[k] = 0; fi[k] = k; pz[k] = 1.0; pr[k] = 1.0; }
        unsigned pl = 0, lm = 0;                                     // bit k: the path / this lane's row goes LEFT at depth k
        int s = 0, d = 0;
        for (;;) {
            // everything the node can need, in ONE batch of wave-uniform reads whose addresses depend on s alone (a child index is
            // clamped to s where the children do not exist): one memory latency a node, not one per dependent table
            const bool kids = 2 * s + 2 < a.nn;
            const int f = a.feat[tb + s];
            const float th = a.thr[tb + s];
            const double v = a.value[tb + s];
            const int sl = a.slot[tb + s];
            const int cs = a.cover[tb + s], cl = a.cover[tb + (kids ? 2 * s + 1 : s)], cr = a.cover[tb + (kids ? 2 * s + 2 : s)];
            if (f >= 0 && kids) {                                    // a split node: descend to the left child
                const double z = (double)cl / (double)cs, zr = (double)cr / (double)cs;
                const unsigned go = x[f] <= th ? 1u : 0u;
                lm = (lm & ~(1u << d)) | (go << d);
                int first = d;
#pragma unroll
                for (int k = D - 1; k >= 0; --k) first = (k < d && pf[k] == f) ? k : first;
#pragma unroll
                for (int k = 0; k < D; ++k)
                    if (k == d) { pf[k] = f; pz[k] = z; pr[k] = zr; ps[k] = sl; fi[k] = first; }
                pl |= 1u << d;
                s = 2 * s + 1; ++d;
                continue;
            }
            // ---- a leaf at depth d ----
            const unsigned o = ~(lm ^ pl);                           // bit k: the row takes edge k
            double zu[D];
            unsigned gm[D];
            int u = 0;
#pragma unroll
            for (int k = 0; k < D; ++k) { zu[k] = pz[k]; gm[k] = 1u << k; u += (k < d && fi[k] == k) ? 1 : 0; }
#pragma unroll
            for (int e = 1; e < D; ++e)
#pragma unroll
                for (int k = 0; k < e; ++k)
                    if (e < d && fi[e] == k) { zu[k] *= pz[e]; gm[k] |= 1u << e; }
            double zall = 1.0;
#pragma unroll
            for (int k = 0; k < D; ++k)
                if (k < d && fi[k] == k) zall *= zu[k];
            if (adm) base += v * zall;
            double old[D];                                           // the leaf's phi reads go out together: one latency a leaf, not one a feature
#pragma unroll
            for (int j = 0; j < D; ++j) old[j] = (j < d && fi[j] == j && adm) ? phi[(size_t)ps[j] * a.ldr] : 0.0;
#pragma unroll
            for (int j = 0; j < D; ++j) {
                if (!(j < d && fi[j] == j)) continue;                // wave-uniform
                double c[D];
                c[0] = 1.0;
#pragma unroll
                for (int k = 1; k < D; ++k) c[k] = 0.0;
#pragma unroll
                for (int m = 0; m < D; ++m) {
                    if (m == j || !(m < d && fi[m] == m)) continue;  // wave-uniform
                    const bool om = (o & gm[m]) == gm[m];
                    const double zm = zu[m];
#pragma unroll
                    for (int k = (m + 1 < D - 1 ? m + 1 : D - 1); k >= 1; --k) c[k] = c[k] * zm + (om ? c[k - 1] : 0.0);
                    c[0] *= zm;
                }
                double tot = 0.0;
#pragma unroll
                for (int k = 0; k < D; ++k)
                    if (k < u) tot += c[k] * shap_w.w[u][k];
                const double oj = (o & gm[j]) == gm[j] ? 1.0 : 0.0;
                const double term = (v * (oj - zu[j])) * tot;
                if (adm) phi[(size_t)ps[j] * a.ldr] = old[j] + term; // a leaf's features are distinct: no two of its slots coincide
            }
            // ---- back up to the nearest edge taken to the left and take its right sibling ----
            while (d > 0 && !((pl >> (d - 1)) & 1u)) { s = (s - 1) >> 1; --d; }
            if (d == 0) break;
            s = s + 1;
            pl &= ~(1u << (d - 1));
#pragma unroll
            for (int k = 0; k < D; ++k)
                if (k == d - 1) pz[k] = pr[k];
        }
    }
    if (live) a.base[(size_t)g * a.ldr + r] = base;
}

static inline bool shap_mis(const void* p, uintptr_t mask) { return ((uintptr_t)p & mask) != 0; }

extern "C" int mms_tree_shap(const TreeShapP* p, hipStream_t s) {
    if (!p || !p->x || !p->feat || !p->thr || !p->value || !p->cover || !p->goff || !p->slot || !p->phi || !p->base) return MMS_ERR_ARG;
    if (p->R < 0 || p->p < 1 || p->ldx < p->p || p->T < 0 || p->G < 0 || p->U < 1) return MMS_ERR_ARG;
    if (p->nn < 1 || p->nn > (2 << MMS_SHAP_MAX_DEPTH) - 1 || p->ldr < p->R || (p->use && p->ldu < p->R)) return MMS_ERR_ARG;
    if (shap_mis(p->x, 3) || shap_mis(p->feat, 3) || shap_mis(p->thr, 3) || shap_mis(p->value, 7) || shap_mis(p->cover, 3)) return MMS_ERR_ARG;
    if (shap_mis(p->goff, 3) || shap_mis(p->slot, 3) || shap_mis(p->phi, 7) || shap_mis(p->base, 7)) return MMS_ERR_ARG;
    if (p->R == 0 || p->G == 0) return MMS_OK;
    const long long tiles = ((long long)p->R + SHAP_WAVE - 1) / SHAP_WAVE;
    if (tiles * p->G > 0x7fffffffLL) return MMS_ERR_ARG;
    if (p->nn <= (2 << 6) - 1)
        MMS_LAUNCH(tree_shap_kernel<6>, dim3((unsigned)(tiles * p->G)), dim3(SHAP_WAVE), 0, s, *p, (int)tiles);
    else
        MMS_LAUNCH(tree_shap_kernel<MMS_SHAP_MAX_DEPTH>, dim3((unsigned)(tiles * p->G)), dim3(SHAP_WAVE), 0, s, *p, (int)tiles);
    return mms_check_launch();
}
