// SimMLM_SurvivalNet heads on gfx950 (MoeP, include/mmsurv.h): the three expert Cox heads, the masked gate input, the gate's
// output layer with the -inf masked softmax, the gate-weighted mixture and the ensemble Cox head, forward and backward.
// Replaces the torch op sequence of R/scripts/analysis/generate_km_curves.py:212-281 around the gate MLP (which runs on
// mms_linear_*).  One workgroup per model: with M <= 32 rows the whole problem is a few thousand multiply-adds, so every
// weight gradient is summed over the rows by one thread (no atomics, deterministic) and every per-row dot product is one wave.
#include "common.h"

#define MOE_MAXM 32

__device__ __forceinline__ bool moe_on(const MoeP& p, int m, int e) { return p.mask[m * p.ldm + e] != 0.f; }
__device__ __forceinline__ bool moe_dead(const MoeP& p, int m) { return !moe_on(p, m, 0) && !moe_on(p, m, 1) && !moe_on(p, m, 2); }

__global__ __launch_bounds__(256) void moe_fwd_kernel(const Grp<MoeP> grp) {
    const MoeP& p = grp.p[blockIdx.z];
    __shared__ float g[MOE_MAXM][3];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, M = p.M, F = p.F, F3 = 3 * F;
    if (p.stage == 0) {
        // expert Cox heads on the unmasked features (the reference applies them before masking): one wave per (row, expert)
        for (int pr = wave; pr < 3 * M; pr += 4) {
            const int m = pr / 3, e = pr % 3;
            const float* f = p.feats + (size_t)m * p.ldf + e * F;
            float a = 0.f;
            for (int j = lane; j < F; j += 64) a = fmaf(p.wx[e][j], f[j], a);
            a = wave_sum(a);
            if (lane == 0) p.hz[(size_t)m * p.ldhz + 1 + e] = a + p.bx[e][0];
        }
        // gate input [f_0 m_0 | f_1 m_1 | f_2 m_2 | m]
        for (int idx = t; idx < M * (F3 + 3); idx += 256) {
            const int m = idx / (F3 + 3), c = idx % (F3 + 3);
            p.gin[(size_t)m * p.ldg + c] = c < F3 ? p.feats[(size_t)m * p.ldf + c] * p.mask[m * p.ldm + c / F] : p.mask[m * p.ldm + c - F3];
        }
        if (p.valid_x)
            for (int idx = t; idx < 4 * M; idx += 256) {
                const int e = idx / M, m = idx % M;
                const bool in = e == 0 ? !moe_dead(p, m) : moe_on(p, m, e - 1);
                p.valid_x[idx] = ((p.valid == nullptr || p.valid[m] != 0.f) && in) ? 1.f : 0.f;
            }
        return;
    }
    // stage 1: logits = W3 h2 + b3, masked softmax (one wave per row)
    for (int m = wave; m < M; m += 4) {
        float l[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) l[c] = wave_sum(p.w3[c * 64 + lane] * p.h2[(size_t)m * p.ldh2 + lane]) + p.b3[c];
        if (lane == 0) {
            float mx = -INFINITY;
#pragma unroll
            for (int c = 0; c < 3; ++c) if (moe_on(p, m, c)) mx = fmaxf(mx, l[c]);
            float ex[3], s = 0.f;
#pragma unroll
            for (int c = 0; c < 3; ++c) { ex[c] = moe_on(p, m, c) ? expf(l[c] - mx) : 0.f; s += ex[c]; }
            const bool dead = moe_dead(p, m);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float v = dead ? __builtin_nanf("") : ex[c] / s;      // torch: softmax over three -inf logits is NaN
                g[m][c] = v;
                p.gate[m * 3 + c] = v;
            }
        }
    }
    __syncthreads();
    // mixture  fused = g_0 (f_0 m_0) + g_1 (f_1 m_1) + g_2 (f_2 m_2)   (a dead row: NaN, as in torch)
    for (int idx = t; idx < M * F; idx += 256) {
        const int m = idx / F, j = idx % F;
        const float* f = p.feats + (size_t)m * p.ldf + j;
        const float* mk = p.mask + m * p.ldm;
        p.fused[idx] = g[m][0] * (f[0] * mk[0]) + g[m][1] * (f[F] * mk[1]) + g[m][2] * (f[2 * F] * mk[2]);
    }
    __syncthreads();
    // ensemble Cox head
    for (int m = wave; m < M; m += 4) {
        float a = 0.f;
        for (int j = lane; j < F; j += 64) a = fmaf(p.we[j], p.fused[(size_t)m * F + j], a);
        a = wave_sum(a);
        if (lane == 0) p.hz[(size_t)m * p.ldhz] = a + p.be[0];
    }
}

__global__ __launch_bounds__(256) void moe_bwd_kernel(const Grp<MoeP> grp) {
    const MoeP& p = grp.p[blockIdx.z];
    __shared__ float g[MOE_MAXM][3], dz[MOE_MAXM], dl[MOE_MAXM][3];
    __shared__ int dead[MOE_MAXM];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, M = p.M, F = p.F, F3 = 3 * F;
    // dz = gradient reaching the ensemble hazard; rows without any modality take none of it (defined as 0, see mmsurv.h)
    if (t < M) {
        dead[t] = moe_dead(p, t) ? 1 : 0;
        dz[t] = dead[t] ? 0.f : p.dhz[(size_t)t * p.lddhz];
#pragma unroll
        for (int c = 0; c < 3; ++c) g[t][c] = dead[t] ? 0.f : p.gate[t * 3 + c];
    }
    __syncthreads();
    if (p.stage == 0) {
        // unmasked feature gradient = own Cox head + (mixture + gate input) through the mask
        for (int idx = t; idx < M * F3; idx += 256) {
            const int m = idx / F3, c = idx % F3, e = c / F, j = c % F;
            const float mix = g[m][e] * dz[m] * p.we[j];
            const float d = (mix + p.dgin[(size_t)m * p.lddg + c]) * p.mask[m * p.ldm + e] + p.dhz[(size_t)m * p.lddhz + 1 + e] * p.wx[e][j];
            p.dfeats[(size_t)m * p.lddf + c] = d;
        }
        // expert Cox head weights
        for (int idx = t; idx < F3; idx += 256) {
            const int e = idx / F, j = idx % F;
            float a = 0.f;
            for (int m = 0; m < M; ++m) a = fmaf(p.dhz[(size_t)m * p.lddhz + 1 + e], p.feats[(size_t)m * p.ldf + idx], a);
            p.dwx[e][j] += a;
        }
        if (t < 3) {
            float a = 0.f;
            for (int m = 0; m < M; ++m) a += p.dhz[(size_t)m * p.lddhz + 1 + t];
            p.dbx[t][0] += a;
        }
        return;
    }
    // stage 1: ensemble head weights (dead rows skipped: their mixture is NaN)
    for (int j = t; j < F; j += 256) {
        float a = 0.f;
        for (int m = 0; m < M; ++m) if (!dead[m]) a = fmaf(dz[m], p.fused[(size_t)m * F + j], a);
        p.dwe[j] += a;
    }
    if (t == 0) {
        float a = 0.f;
        for (int m = 0; m < M; ++m) a += dz[m];
        p.dbe[0] += a;
        if (p.loss_out && p.cox_outs) {
            const float* o = p.cox_outs;
            p.loss_out[0] = o[0] + p.expert_weight * (o[2] + o[4] + o[6]);
            p.loss_out[1] = o[1];
        }
    }
    // gate weights' gradient dg_e = dz (we . f_e m_e) [+ external], softmax backward -> logits (one wave per row)
    for (int m = wave; m < M; m += 4) {
        float part[3];
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            float a = 0.f;
            const float me = p.mask[m * p.ldm + e];
            for (int j = lane; j < F; j += 64) a = fmaf(p.we[j], p.feats[(size_t)m * p.ldf + e * F + j] * me, a);
            part[e] = wave_sum(a);
        }
        if (lane == 0) {
            float dg[3], dot = 0.f;
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                dg[e] = dz[m] * part[e] + (p.dgate_ext ? p.dgate_ext[m * 3 + e] : 0.f);
                dot += g[m][e] * dg[e];
            }
#pragma unroll
            for (int e = 0; e < 3; ++e) dl[m][e] = dead[m] ? 0.f : g[m][e] * (dg[e] - dot);   // masked logits: g = 0 -> 0
        }
    }
    __syncthreads();
    // gate output layer: dW3, db3 (summed over rows) and dh2
    if (t < 192) {
        const int c = t / 64, k = t % 64;
        float a = 0.f;
        for (int m = 0; m < M; ++m) a = fmaf(dl[m][c], p.h2[(size_t)m * p.ldh2 + k], a);
        p.dw3[t] += a;
    } else if (t < 195) {
        const int c = t - 192;
        float a = 0.f;
        for (int m = 0; m < M; ++m) a += dl[m][c];
        p.db3[c] += a;
    }
    for (int idx = t; idx < M * 64; idx += 256) {
        const int m = idx / 64, k = idx % 64;
        p.dh2[(size_t)m * p.lddh2 + k] = dl[m][0] * p.w3[k] + dl[m][1] * p.w3[64 + k] + dl[m][2] * p.w3[128 + k];
    }
}

static bool moe_group(Grp<MoeP>& a, const MoeP* pp, int ng, bool bwd) {
    if (!grp_fill(a, pp, ng, 1)) return false;
    for (int gi = 0; gi < ng; ++gi) {
        const MoeP& q = pp[gi];
        if (q.M != pp->M || q.F != pp->F || q.stage != pp->stage) return false;
        if (q.M < 1 || q.M > MOE_MAXM || q.F <= 0 || q.F % 4 != 0 || (q.stage != 0 && q.stage != 1)) return false;
        if (!q.feats || !q.mask || q.ldf < 3 * q.F || q.ldm < 3 || !q.gate) return false;
        if (!q.wx[0] || !q.wx[1] || !q.wx[2] || !q.bx[0] || !q.bx[1] || !q.bx[2] || !q.we || !q.be || !q.w3 || !q.b3) return false;
        if (!bwd && q.stage == 0 && (!q.gin || q.ldg < 3 * q.F + 3 || !q.hz || q.ldhz < 4)) return false;
        if (!bwd && q.stage == 1 && (!q.h2 || q.ldh2 < 64 || !q.hz || q.ldhz < 4 || !q.fused)) return false;
        if (bwd && (!q.dhz || q.lddhz < 4)) return false;
        if (bwd && q.stage == 0 && (!q.dgin || q.lddg < 3 * q.F || !q.dfeats || q.lddf < 3 * q.F || !q.dwx[0] || !q.dwx[1] || !q.dwx[2] ||
                                    !q.dbx[0] || !q.dbx[1] || !q.dbx[2])) return false;
        if (bwd && q.stage == 1 && (!q.fused || !q.h2 || q.ldh2 < 64 || !q.dh2 || q.lddh2 < 64 || !q.dw3 || !q.db3 || !q.dwe || !q.dbe))
            return false;
    }
    return true;
}
extern "C" int mms_moe_fwd_group(const MoeP* pp, int ng, hipStream_t s) {
    Grp<MoeP> a;
    if (!moe_group(a, pp, ng, false)) return MMS_ERR_ARG;
    MMS_LAUNCH(moe_fwd_kernel, dim3(1, 1, ng), dim3(256), 0, s, a);
    return mms_check_launch();
}
extern "C" int mms_moe_bwd_group(const MoeP* pp, int ng, hipStream_t s) {
    Grp<MoeP> a;
    if (!moe_group(a, pp, ng, true)) return MMS_ERR_ARG;
    MMS_LAUNCH(moe_bwd_kernel, dim3(1, 1, ng), dim3(256), 0, s, a);
    return mms_check_launch();
}
MMS_SINGLE(mms_moe_fwd, MoeP)
MMS_SINGLE(mms_moe_bwd, MoeP)
