// Weighted (bootstrap) Harrell-C pair counts of M models on R multiplicity vectors (include/mmsurv.h: CbootP).
//
// A replicate's pair counts are bilinear forms in its multiplicity vector w:  2 conc + tied = w' S_m w,  comparable = w' P w,  with
// P[i][j] in {0,1} "pair (i earlier event, j) is comparable" and S_m = P o (2 [h_i > h_j] + [h_i == h_j]) in {0,1,2}.  For R replicates
// that is Y = W . S ([R x n] int8 times [n x n] int8, int32 sums) followed by out[b] = sum_j w[b][j] Y[b][j] in 64 bits.
//
// v_mfma_i32_16x16x64_i8 does the product.  W is the A operand: a workgroup stages a 64-replicate x 64-patient tile of it in LDS per K
// step and each wave reads its four 16-replicate fragments (16 contiguous K bytes per lane) from there.  S_m and P are never in memory:
// each lane generates the B fragments of its own column j (lane & 15) for the 16 patients i of its K group (lane >> 4) in registers, from
// the K step's 64 i-side ranks in LDS (the 16 lanes of a K group read the same addresses), and one generated fragment feeds four MFMAs
// (the four A tiles) per matrix.  A and B take their K indices by the same rule (element e of K group g is k = 16 g + e), so the sums do
// not depend on how the hardware orders K inside a lane -- only on A's row and B's column being lane & 15, which the exact tests pin.
//
// A K step is skipped by a wave when no pair in it can be comparable: the largest time rank of the wave's 16 columns is below the
// smallest time rank of the step's event patients.  With time-sorted input that removes about half of the work; any order is correct.
//
// Epilogue: lane (c = lane & 15, g = lane >> 4) holds Y[16 t + 4 g + r][j0 + c] (the C layout all 16x16 MFMAs share); it multiplies by
// w[b][j], the 16 columns are summed by shuffles, the four waves by LDS, and one 64-bit integer vector atomic per (matrix, replicate) and
// workgroup goes to `out`: integer adds, so the result is the same whatever the order.
#include "common.h"
#include <limits.h>

typedef int cb_v4i __attribute__((ext_vector_type(4)));

#define CB_LDA 80       // LDS row stride (bytes) of the staged W tile: 64 K bytes + 16 of padding, 16-byte aligned rows
#define CB_MAXNM 4      // model matrices per launch (plus P); more models take more launches

struct CbArgs {
    const int* hrank; int ldh; int m0; int M;
    const int* trank; const int* event; const int* stratum; int n;
    const signed char* w; int ldw; int R;
    long long* out; int rule; int acc_p;
};

template <int NM> struct CbSide { cb_v4i w; int t, s, h[NM]; };

// the staging loads of one K step: every lane its 16 bytes of the W tile, lanes 0..63 the i-side of patient k0 + lane
template <int NM> __device__ __forceinline__ CbSide<NM> cb_fetch(const CbArgs& a, int k0, int tid, int b0) {
    CbSide<NM> r;
    const int row = tid >> 2, seg = tid & 3, b = b0 + row;
    r.w = cb_v4i{0, 0, 0, 0};
    if (b < a.R) r.w = *(const cb_v4i*)(a.w + (size_t)b * a.ldw + k0 + seg * 16);
    r.t = INT_MAX; r.s = 0;
#pragma unroll
    for (int m = 0; m < NM; ++m) r.h[m] = 0;
    const int i = k0 + tid;
    if (tid < 64 && i < a.n) {
        if (a.event[i] != 0) r.t = a.trank[i];          // a censored i opens no pair: its time never compares
        if (a.stratum) r.s = a.stratum[i];
#pragma unroll
        for (int m = 0; m < NM; ++m) r.h[m] = a.hrank[(size_t)(a.m0 + m) * a.ldh + i];
    }
    return r;
}

template <int NM> __global__ __launch_bounds__(256) void cindex_boot_kernel(const CbArgs a) {
    __shared__ __attribute__((aligned(16))) signed char sW[64 * CB_LDA];
    __shared__ __attribute__((aligned(16))) int sT[64];
    __shared__ __attribute__((aligned(16))) int sS[64];
    __shared__ __attribute__((aligned(16))) int sH[NM][64];
    __shared__ long long sRed[4][NM + 1][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lc = lane & 15, lq = lane >> 4;
    const int j = blockIdx.x * 64 + wave * 16 + lc, b0 = blockIdx.y * 64;
    const bool jv = j < a.n;
    // j side: an absent column compares with nothing
    const int tj = jv ? a.trank[j] : INT_MIN;
    const int sj = (jv && a.stratum) ? a.stratum[j] : 0;
    const int teq = (jv && a.rule == 1 && a.event[j] == 0) ? tj : INT_MIN;      // rule 1: a censored j tied in time with an event i
    int hj[NM];
#pragma unroll
    for (int m = 0; m < NM; ++m) hj[m] = jv ? a.hrank[(size_t)(a.m0 + m) * a.ldh + j] : 0;
    int tmax = tj;
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) tmax = max(tmax, __shfl_xor(tmax, o, 64));

    cb_v4i acc[NM + 1][4];
#pragma unroll
    for (int m = 0; m <= NM; ++m)
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[m][t] = cb_v4i{0, 0, 0, 0};

    const int kend = (a.n + 63) & ~63;                  // <= ldw: ldw is a multiple of 64 and >= n
    CbSide<NM> nx = cb_fetch<NM>(a, 0, tid, b0);
    for (int k0 = 0; k0 < kend; k0 += 64) {
        __syncthreads();                                // the previous step's LDS reads are done
        *(cb_v4i*)(sW + (tid >> 2) * CB_LDA + (tid & 3) * 16) = nx.w;
        if (tid < 64) {
            sT[tid] = nx.t; sS[tid] = nx.s;
#pragma unroll
            for (int m = 0; m < NM; ++m) sH[m][tid] = nx.h[m];
        }
        __syncthreads();
        if (k0 + 64 < kend) nx = cb_fetch<NM>(a, k0 + 64, tid, b0);
        int tmin = sT[lane];
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) tmin = min(tmin, __shfl_xor(tmin, o, 64));
        if (tmax < tmin) continue;                      // wave-uniform: no t_j >= t_i with an event i in this step

        cb_v4i bp, bs[NM];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const cb_v4i ti = *(const cb_v4i*)&sT[lq * 16 + q * 4], si = *(const cb_v4i*)&sS[lq * 16 + q * 4];
            unsigned pm[4];
            unsigned pw = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                pm[e] = (si[e] == sj) & ((tj > ti[e]) | (teq == ti[e]));
                pw |= pm[e] << (8 * e);
            }
            bp[q] = (int)pw;
#pragma unroll
            for (int m = 0; m < NM; ++m) {
                const cb_v4i hi = *(const cb_v4i*)&sH[m][lq * 16 + q * 4];
                unsigned sw = 0;
#pragma unroll
                for (int e = 0; e < 4; ++e) sw |= (pm[e] ? (unsigned)(hi[e] > hj[m]) + (unsigned)(hi[e] >= hj[m]) : 0u) << (8 * e);
                bs[m][q] = (int)sw;
            }
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const cb_v4i af = *(const cb_v4i*)(sW + (t * 16 + lc) * CB_LDA + lq * 16);
#pragma unroll
            for (int m = 0; m < NM; ++m) acc[m][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(af, bs[m], acc[m][t], 0, 0, 0);
            if (a.acc_p) acc[NM][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(af, bp, acc[NM][t], 0, 0, 0);
        }
    }

    // out[b] += sum_j w[b][j] Y[b][j]
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = t * 16 + lq * 4 + r, b = b0 + row;
            const long long wj = (jv && b < a.R) ? (long long)a.w[(size_t)b * a.ldw + j] : 0;
#pragma unroll
            for (int m = 0; m <= NM; ++m) {
                long long v = wj * (long long)acc[m][t][r];
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o, 64);
                if (lc == 0) sRed[wave][m][row] = v;
            }
        }
    __syncthreads();
    const int nmat = a.acc_p ? NM + 1 : NM;
    for (int x = tid; x < nmat * 64; x += 256) {
        const int m = x >> 6, row = x & 63, b = b0 + row;
        const long long v = sRed[0][m][row] + sRed[1][m][row] + sRed[2][m][row] + sRed[3][m][row];
        if (b < a.R && v != 0) {
            const int orow = m < NM ? a.m0 + m : a.M;
            atomicAdd((unsigned long long*)(a.out + (size_t)orow * a.R + b), (unsigned long long)v);
        }
    }
}

template <int NM> static void cb_launch(const CbArgs& a, hipStream_t s) {
    MMS_LAUNCH(cindex_boot_kernel<NM>, dim3((a.n + 63) / 64, (a.R + 63) / 64), dim3(256), 0, s, a);
}

extern "C" int mms_cindex_boot(const CbootP* p, hipStream_t s) {
    if (!p || !p->hrank || !p->trank || !p->event || !p->w || !p->out) return MMS_ERR_ARG;
    if (p->n < 1 || p->n > MMS_CBOOT_MAX_N || p->R < 1 || p->R > MMS_CBOOT_MAX_R || p->M < 1 || p->M > MMS_CBOOT_MAX_M) return MMS_ERR_ARG;
    if (p->ldw < p->n || (p->ldw & 63) || p->ldh < p->n) return MMS_ERR_ARG;
    if (((uintptr_t)p->w & 15) || ((uintptr_t)p->out & 7)) return MMS_ERR_ARG;
    if (((uintptr_t)p->hrank & 3) || ((uintptr_t)p->trank & 3) || ((uintptr_t)p->event & 3) || ((uintptr_t)p->stratum & 3)) return MMS_ERR_ARG;
    if (p->pair_rule < 0 || p->pair_rule > 1) return MMS_ERR_ARG;
    CbArgs a{p->hrank, p->ldh, 0, p->M, p->trank, p->event, p->stratum, p->n, p->w, p->ldw, p->R, p->out, p->pair_rule, 1};
    for (int m0 = 0; m0 < p->M; m0 += CB_MAXNM) {       // P is accumulated by the first launch only
        a.m0 = m0; a.acc_p = m0 == 0;
        switch (p->M - m0 < CB_MAXNM ? p->M - m0 : CB_MAXNM) {
            case 1: cb_launch<1>(a, s); break;
            case 2: cb_launch<2>(a, s); break;
            case 3: cb_launch<3>(a, s); break;
            default: cb_launch<4>(a, s); break;
        }
    }
    return mms_check_launch();
}
