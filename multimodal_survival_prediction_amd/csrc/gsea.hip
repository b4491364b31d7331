// Gene-set enrichment with a label-permutation null (include/mmsurv.h: GseaScoreP, GseaEsP).
//
// mms_gsea_scores -- Z[r][g] = scale[g] * sum_i m[perm[r][i]] x[row[i]][g]: the Cox score of every gene at beta = 0 under R1 relabellings
// of the patients, standardised by its exact permutation variance.  Two launches:
//   scale    one thread per gene walks the list in order, fp64, two passes (mean, centred squares), and sum m^2 in the same order
//   product  v_mfma_f64_16x16x4_f64 with replicates on M, genes on N, list positions on K; A is gathered as m[perm[r][i]], B is x widened
// f64 MFMA maps (16x16x4, one f64 per lane for A and B, four per lane for D): A[m = lane & 15][k = lane >> 4], B[k = lane >> 4][n = lane & 15],
// D[m = (lane >> 4) + 4 i][n = lane & 15] in register i (the maps of coxnet.hip).  Each lane reads FOUR consecutive k of its operand
// (k = 16 s + 4 h + i, h = lane >> 4) and MFMA i of step s sums over h: a permuted but fixed K order that depends on n only.  A row of D
// is computed from its own row of A, so a replicate's bits do not depend on R1 or on which tile row it lands in.
//
// mms_gsea_es -- one workgroup per replicate.  The G keys are sorted in LDS by (z descending, gene ascending) with a bitonic network
// over the next power of two (padding keys are -inf with indices >= G: they sort last), which leaves order[pos], rank[g] and the sorted
// |z| in LDS.  The four waves then take the sets in turn: a wave flags the ranks of its set in a byte strip of its own, walks the
// positions 64 at a time (inclusive wave prefix sum of the hit weights, the miss count from the ballot; a chunk without a hit in closed
// form: the walk only falls there, so its first position is the only candidate for hi and its last for lo), keeps hi / lo with their
// first positions, stores and clears the flags it set.  fp64, no atomics, plain stores.
#include "common.h"
#include <math.h>

typedef double f64x4 __attribute__((ext_vector_type(4)));

#define GS_MFMA(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0)
#define GS_PT 4          // product: 16-replicate tiles per wave (a workgroup's 4 waves share one strip of 64 replicates)
#define GE_WAVES 4       // es: waves per workgroup = flag strips in LDS (MMS_GSEA_MAX_G's bytes per gene count them)

// ---- scale ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gsea_scale_kernel(const GseaScoreP a) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= a.G) return;
    const float* xc = a.x + g;
    double sx = 0.0, sm2 = 0.0;
    for (int i = 0; i < a.n; ++i) {                      // (i, row[i], m[i] are uniform: scalar loads)
        const double mi = a.m[i];
        sx += (double)xc[(size_t)a.row[i] * a.ld];
        sm2 += mi * mi;
    }
    const double mean = sx / (double)a.n;
    double css = 0.0;
    for (int i = 0; i < a.n; ++i) {
        const double d = (double)xc[(size_t)a.row[i] * a.ld] - mean;
        css += d * d;
    }
    a.scale[g] = (css > 0.0 && sm2 > 0.0) ? 1.0 / sqrt(sm2 / (double)(a.n - 1) * css) : 0.0;
}

// ---- product ----------------------------------------------------------------------------------------------------------------------------
// wave = 16 genes x 64 replicates, K = every list position in order; grid x = 64 genes, y = 64 replicates
__global__ __launch_bounds__(256) void gsea_product_kernel(const GseaScoreP a) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int c = lane & 15, h = lane >> 4;
    const int j0 = (blockIdx.x * 4 + wave) * 16;
    if (j0 >= a.G) return;
    const int p0 = blockIdx.y * 16 * GS_PT;
    const int nt = min(GS_PT, (a.R1 - p0 + 15) / 16);
    const int j = j0 + c;
    const bool jv = j < a.G;
    f64x4 acc[GS_PT];
#pragma unroll
    for (int t = 0; t < GS_PT; ++t) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < a.n; k0 += 16) {
        const int k = k0 + 4 * h;
        double xv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) xv[i] = (jv && k + i < a.n) ? (double)a.x[(size_t)a.row[k + i] * a.ld + j] : 0.0;
#pragma unroll
        for (int t = 0; t < GS_PT; ++t) {
            if (t >= nt) continue;                                  // (uniform)
            const int p = p0 + 16 * t + c;
            const bool pv = p < a.R1;
            const int* pr = a.perm + (size_t)(pv ? p : 0) * a.n;
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[t] = GS_MFMA((pv && k + i < a.n) ? a.m[pr[k + i]] : 0.0, xv[i], acc[t]);
        }
    }
    const double s = jv ? a.scale[j] : 0.0;
#pragma unroll
    for (int t = 0; t < GS_PT; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int p = p0 + 16 * t + h + 4 * i;
            if (t < nt && p < a.R1 && jv) a.Z[(size_t)p * a.ldz + j] = s == 0.0 ? 0.0 : acc[t][i] * s;
        }
}

extern "C" int mms_gsea_scores(const GseaScoreP* p, hipStream_t s) {
    if (!p || !p->x || !p->row || !p->m || !p->perm || !p->scale || !p->Z) return MMS_ERR_ARG;
    if (p->n < 2 || p->N < 1 || p->G < 1 || p->G > MMS_GSEA_MAX_G || p->ld < p->G || p->ldz < p->G) return MMS_ERR_ARG;
    if (p->R1 < 0 || p->R1 > MMS_GSEA_MAX_R1) return MMS_ERR_ARG;
    if (((uintptr_t)p->x & 3) || ((uintptr_t)p->row & 3) || ((uintptr_t)p->perm & 3)) return MMS_ERR_ARG;
    if (((uintptr_t)p->m & 7) || ((uintptr_t)p->scale & 7) || ((uintptr_t)p->Z & 7)) return MMS_ERR_ARG;
    if (p->R1 == 0) return MMS_OK;
    MMS_LAUNCH(gsea_scale_kernel, dim3((p->G + 255) / 256), dim3(256), 0, s, *p);
    MMS_LAUNCH(gsea_product_kernel, dim3((p->G + 63) / 64, (p->R1 + 16 * GS_PT - 1) / (16 * GS_PT)), dim3(256), 0, s, *p);
    return mms_check_launch();
}

// ---- enrichment score -------------------------------------------------------------------------------------------------------------------
// the value after a position with hit-weight prefix hsum and miss count mc (one expression for the chunk walk and the closed form)
// true divisions: a set of one gene must step by exactly |z| / |z| = 1 whatever z is, so that equal ranks give equal scores
// with unit weights hsum is the hit count and nr = k: (hits (G - k) - misses k) / (k (G - k)) has an exact integer numerator, so positions
// whose values are equal as fractions are equal in bits and the first-position rule decides them
__device__ __forceinline__ double ge_run(double hsum, int mc, double nr, double nmiss, bool unit) {
    return unit ? (hsum * nmiss - (double)mc * nr) / (nr * nmiss) : hsum / nr - (double)mc / nmiss;
}

__global__ __launch_bounds__(64 * GE_WAVES) void gsea_es_kernel(const GseaEsP a) {
    __shared__ double key[MMS_GSEA_MAX_G];                          // 64 KB: z, then |z| in rank order
    __shared__ unsigned short ord[MMS_GSEA_MAX_G];                  // 16 KB: the gene at a position
    __shared__ unsigned short rnk[MMS_GSEA_MAX_G];                  // 16 KB: the position of a gene
    __shared__ unsigned char flag[GE_WAVES][MMS_GSEA_MAX_G];        // 32 KB: one strip per wave
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = blockIdx.x, G = a.G;
    unsigned P2 = 2;
    while (P2 < (unsigned)G) P2 <<= 1;                              // <= MMS_GSEA_MAX_G, itself a power of two
    const bool pre = a.gperm != nullptr;
    const double* z = a.Z + (pre ? (size_t)0 : (size_t)r * a.ldz);
    const int* gp = (pre && r > 0) ? a.gperm + (size_t)(r - 1) * G : nullptr;
    for (unsigned i = tid; i < P2; i += 64 * GE_WAVES) {
        key[i] = i < (unsigned)G ? z[gp ? gp[i] : (int)i] : -INFINITY;
        ord[i] = (unsigned short)i;
    }
    for (int i = tid; i < G; i += 64 * GE_WAVES)
#pragma unroll
        for (int w = 0; w < GE_WAVES; ++w) flag[w][i] = 0;
    __syncthreads();
    for (unsigned k = 2; k <= P2; k <<= 1)
        for (unsigned j = k >> 1; j > 0; j >>= 1) {
            for (unsigned t = tid; t < P2 / 2; t += 64 * GE_WAVES) {
                const unsigned i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i + j;
                const double ki = key[i], kl = key[l];
                const unsigned short oi = ord[i], ol = ord[l];
                const bool l_first = kl > ki || (kl == ki && ol < oi);       // (a strict total order: the indices differ)
                if (l_first == ((i & k) == 0)) { key[i] = kl; key[l] = ki; ord[i] = ol; ord[l] = oi; }
            }
            __syncthreads();
        }
    for (int pos = tid; pos < G; pos += 64 * GE_WAVES) {            // (the padding keys stand at the positions >= G)
        rnk[ord[pos]] = (unsigned short)pos;
        key[pos] = fabs(key[pos]);
    }
    __syncthreads();

    unsigned char* fl = flag[wave];
    for (int s = wave; s < a.S; s += GE_WAVES) {
        const int o0 = a.set_off[s], k = a.set_off[s + 1] - o0;
        const int* mem = a.set_gene + o0;
        double nr = 0.0;
        for (int t = lane; t < k; t += 64) {
            const int pos = rnk[mem[t]];
            fl[pos] = 1;
            if (a.weight) nr += key[pos];
        }
        nr = wave_sum_d(nr);                                        // (the same bits in every lane)
        const bool unit = !a.weight || !(nr > 0.0);
        if (unit) nr = (double)k;
        const double nmiss = (double)(G - k);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");      // the strip is this wave's own: its LDS accesses complete in order
        __builtin_amdgcn_wave_barrier();
        double hi = -INFINITY, lo = INFINITY, hsum = 0.0;
        int hip = 0, lop = 0, miss = 0;
        for (int c0 = 0; c0 < G; c0 += 64) {
            const int pos = c0 + lane;
            const bool v = pos < G;
            const bool f = v && fl[pos] != 0;
            const unsigned long long hit = __ballot(f), val = __ballot(v);
            const int nv = __popcll(val);
            if (hit == 0ull) {                                      // (uniform) nv misses in a row
                const double first = ge_run(hsum, miss + 1, nr, nmiss, unit), last = ge_run(hsum, miss + nv, nr, nmiss, unit);
                if (first > hi) { hi = first; hip = c0; }
                if (last < lo) { lo = last; lop = c0 + nv - 1; }
                miss += nv;
                continue;
            }
            double w = f ? (unit ? 1.0 : key[pos]) : 0.0;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const double t = __shfl_up(w, o, 64);
                if (lane >= o) w += t;
            }
            const unsigned long long upto = lane == 63 ? ~0ull : ((1ull << (lane + 1)) - 1ull);
            const double run = ge_run(hsum + w, miss + __popcll(~hit & val & upto), nr, nmiss, unit);
            double mx = v ? run : -INFINITY, mn = v ? run : INFINITY;
            int mxp = pos, mnp = pos;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {                      // the extreme and its lowest position; the same in every lane
                const double omx = __shfl_xor(mx, o, 64), omn = __shfl_xor(mn, o, 64);
                const int omxp = __shfl_xor(mxp, o, 64), omnp = __shfl_xor(mnp, o, 64);
                if (omx > mx || (omx == mx && omxp < mxp)) { mx = omx; mxp = omxp; }
                if (omn < mn || (omn == mn && omnp < mnp)) { mn = omn; mnp = omnp; }
            }
            if (mx > hi) { hi = mx; hip = mxp; }
            if (mn < lo) { lo = mn; lop = mnp; }
            hsum += __shfl(w, 63, 64);
            miss += __popcll(~hit & val);
        }
        const bool up = hi >= -lo;
        if (lane == 0) {
            a.es[(size_t)r * a.lde + s] = up ? hi : lo;
            if (a.peak) a.peak[(size_t)r * a.lde + s] = up ? hip : lop;
        }
        for (int t = lane; t < k; t += 64) fl[rnk[mem[t]]] = 0;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

extern "C" int mms_gsea_es(const GseaEsP* p, hipStream_t s) {
    if (!p || !p->Z || !p->set_off || !p->set_gene || !p->es) return MMS_ERR_ARG;
    if (p->G < 2 || p->G > MMS_GSEA_MAX_G || p->S < 0 || p->R1 < 0 || p->R1 > MMS_GSEA_MAX_R1) return MMS_ERR_ARG;
    if ((p->weight != 0 && p->weight != 1) || p->ldz < p->G || p->lde < p->S) return MMS_ERR_ARG;
    if (((uintptr_t)p->Z & 7) || ((uintptr_t)p->es & 7)) return MMS_ERR_ARG;
    if (((uintptr_t)p->gperm & 3) || ((uintptr_t)p->set_off & 3) || ((uintptr_t)p->set_gene & 3) || ((uintptr_t)p->peak & 3)) return MMS_ERR_ARG;
    if (p->R1 == 0 || p->S == 0) return MMS_OK;
    MMS_LAUNCH(gsea_es_kernel, dim3(p->R1), dim3(64 * GE_WAVES), 0, s, *p);
    return mms_check_launch();
}
