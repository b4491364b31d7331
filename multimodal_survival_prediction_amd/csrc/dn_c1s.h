// The whole-K 16x16-tile conv1 forward of dn_c1s.hip as a device function, shared by its own launch (dn_c1s.hip) and by the fused
// block-3 launch that runs it behind the previous layer's conv2 (dn_c3s.hip, mms_c3s_c1s_fwd), with the hand-off they use.
#pragma once
#include "dn_ops.h"

#define C1S_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

// In-launch hand-off of the fused block-3 forward (cdna_hip_programming.md Guideline 16, R1): the producer stores its payload
// write-through (agent-scope relaxed stores: global_store ... sc1) and adds its statistics with agent-scope atomics; every wave drains
// them (s_waitcnt vmcnt(0)), the barrier joins the waves, one lane adds 1 to the model's arrival word.  The consumer's polling lane
// waits until `target` producers have arrived (relaxed agent-scope loads, s_sleep between polls) and the workgroup then reads the
// payload with agent-scope loads only.  The words are zeroed before every forward (the driver's per-step zero-fill; an eval forward
// zeroes them on its own), so a second forward, an eval forward or a graph replay never finds one already satisfied.
__device__ __forceinline__ void hx_publish(unsigned* flag) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_fetch_add(flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// Bounded: after ~0.3 s (wall clock, 100 MHz) -- or as soon as another workgroup has raised the sticky error word -- the wait gives up
// and raises `err` (the drivers' error word, mms_dn121_region "b4_err").  Call from ONE lane; the caller's barrier releases the workgroup.
__device__ __forceinline__ void hx_wait(const unsigned* flag, unsigned target, unsigned* err) {
    const unsigned long long t0 = wall_clock64();
    for (unsigned spins = 1;; ++spins) {
        if (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= target) return;
        if ((spins & 31u) == 0u) {
            const bool late = wall_clock64() - t0 > 30000000ull;
            if (late || __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) {
                if (late) atomicExch(err, 1u);
                return;
            }
        }
        __builtin_amdgcn_s_sleep(1);
    }
}

// Output tile (rows 16 bx .., columns 16 by ..) of y = relu(bn1(x)) @ W^T over the whole K range (one workgroup of 256 threads).
// FUSED: the last 32 input channels [K - 32, K) -- the previous layer's conv2 output -- and their batch statistics are produced by
// other workgroups of the SAME launch.  Everything else (the old-channel panel, every weight fragment, the old channels' BatchNorm
// constants) is requested and multiplied first; then one lane waits on `flag` for `target` producers, and the new channels and their
// statistics are read with agent-scope (sc1) loads, so no acquire fence is needed: no other load of the tile touches a line the
// producers write (the new columns are one aligned 128-byte line per row, their statistics two).  The last two 16-channel groups go
// into the same accumulators in the same order as in the unfused form, and their BatchNorm constants are computed the same way from
// the same fp64 accumulators: the tile is bit-identical to the unfused one.
template <int C1S_NP, bool FUSED>
__device__ __forceinline__ void conv1s_fwd_tile(const Conv1FwdP& p, int bx, int by, float* smem, const unsigned* flag = nullptr,
                                                unsigned target = 0, unsigned* err = nullptr) {
    const float* __restrict__ x = p.x;                 // kernel arguments read once (dn_c3s.hip: left in the kernarg segment they are
    const float* __restrict__ w = p.w;                 // re-read inside every predicated block)
    const int M = p.M, K = p.K, N = p.N, ldx = p.ldx;
    const int K1 = FUSED ? K - 32 : K;                 // channels that are final before the launch
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, h = lane >> 4;
    const int m0 = bx * 16, n0 = by * 16;
    const int P = K + 4;                               // LDS row pitch (floats)
    float* As = smem;                                  // [16][P]  relu(bn1(x)) panel
    float* cmean = As + 16 * P;                        // [K] BatchNorm1 constants
    float* csc = cmean + K;
    float* cbeta = csc + K;

    // ---- one batch of loads: the activation panel (clamped addresses, branch-free), this wave's weight fragments, the BatchNorm
    // statistics / parameters.  The weights go straight into the MFMA register layout (lane (li, h), group g: W[n0 + li][16 g + 4 h ..
    // + 3]) -- only the activation panel, which needs the BatchNorm transform, is staged: half the LDS of a two-panel layout, so a
    // second workgroup -- or the other streams' workgroups -- fits beside this one on a CU (the step-ablation runs of
    // profiles/r03_step_ablation.txt: the kernels with the largest LDS footprints cost the step the most per microsecond of their own).
    const int kq = K1 >> 2, total = 16 * kq;           // float4 pieces of the panel
    const int ng16 = K >> 4, ng1 = K1 >> 4;
    float4 ra[C1S_NP], rb[C1S_NP];
#pragma unroll
    for (int i = 0; i < C1S_NP; ++i) {
        if (256 * i < total) {                         // workgroup-uniform
            const int idx = tid + 256 * i, ic = idx < total ? idx : total - 1;
            const int r = ic / kq, k4 = (ic - r * kq) * 4;
            const int mr = m0 + r < M ? m0 + r : M - 1;
            ra[i] = *(const float4*)(x + (size_t)mr * ldx + k4);
        }
    }
    const float* wr = w + (size_t)(n0 + li < N ? n0 + li : N - 1) * K + 4 * h;
#pragma unroll
    for (int i = 0; i < C1S_NP; ++i) {
        if (wave + 4 * i < ng16) rb[i] = *(const float4*)(wr + 16 * (wave + 4 * i));      // wave-uniform
    }
    bn_consts_to_lds<4>(p.bn, K1, tid, cmean, csc, cbeta);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < C1S_NP; ++i) {
        if (256 * i < total) {
            const int idx = tid + 256 * i;
            if (idx < total) {
                const int r = idx / kq, k4 = (idx - r * kq) * 4;
                const float z = m0 + r < M ? 1.f : 0.f;
                const float4 v = ra[i];
                *(float4*)&As[r * P + k4] = make_float4(z * fmaxf(bn_apply(v.x, cmean[k4], csc[k4], cbeta[k4]), 0.f),
                                                        z * fmaxf(bn_apply(v.y, cmean[k4 + 1], csc[k4 + 1], cbeta[k4 + 1]), 0.f),
                                                        z * fmaxf(bn_apply(v.z, cmean[k4 + 2], csc[k4 + 2], cbeta[k4 + 2]), 0.f),
                                                        z * fmaxf(bn_apply(v.w, cmean[k4 + 3], csc[k4 + 3], cbeta[k4 + 3]), 0.f));
            }
        }
    }
    __syncthreads();

    // ---- the K range: 16-channel groups g = wave, wave + 4, ...; element e of lane (row, h) is k = 16 g + 4 h + e for both operands
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    const float* ar = As + li * P + 4 * h;
    const float zb = n0 + li < N ? 1.f : 0.f;
#pragma unroll
    for (int i = 0; i < C1S_NP; i += 2) {
        const int g = wave + 4 * i;
        if (g < ng1) {                                 // wave-uniform
            const bool two = g + 4 < ng1;
            const float4 a0 = *(const float4*)(ar + 16 * g);
            const float4 a1 = two ? *(const float4*)(ar + 16 * (g + 4)) : make_float4(0.f, 0.f, 0.f, 0.f);
            const float4 b0 = rb[i];
            const float4 b1 = two ? rb[i + 1] : make_float4(0.f, 0.f, 0.f, 0.f);
            acc0 = C1S_MFMA(a0.x, zb * b0.x, acc0); acc1 = C1S_MFMA(a1.x, zb * b1.x, acc1);
            acc0 = C1S_MFMA(a0.y, zb * b0.y, acc0); acc1 = C1S_MFMA(a1.y, zb * b1.y, acc1);
            acc0 = C1S_MFMA(a0.z, zb * b0.z, acc0); acc1 = C1S_MFMA(a1.z, zb * b1.z, acc1);
            acc0 = C1S_MFMA(a0.w, zb * b0.w, acc0); acc1 = C1S_MFMA(a1.w, zb * b1.w, acc1);
        }
    }
    if constexpr (FUSED) {
        // ---- the previous layer's 32 channels: wait for its producers, then one agent-scope 8-byte load per thread (row tid / 16,
        // channels K1 + 2 (tid % 16) ..) and the 32 channels' BatchNorm constants -- the arithmetic of bn_consts_to_lds
        if (tid == 0) hx_wait(flag, target, err);
        __syncthreads();
        const int r = tid >> 4, k2 = K1 + 2 * (tid & 15);
        const int mr = m0 + r < M ? m0 + r : M - 1;
        const unsigned long long xv = __hip_atomic_load((const unsigned long long*)(x + (size_t)mr * ldx + k2), __ATOMIC_RELAXED,
                                                        __HIP_MEMORY_SCOPE_AGENT);
        if (tid < 32) {
            const BnSrc& b = p.bn;
            const int c = K1 + tid;
            float mu = 0.f, rstd = 1.f, g = 1.f, be = 0.f;
            if (b.gamma) {
                g = b.gamma[c]; be = b.beta[c];
                if (b.train) {
                    const double s = __hip_atomic_load(b.sum + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    const double q = __hip_atomic_load(b.sumsq + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    const double m = s * (double)b.inv_count;
                    double v = q * (double)b.inv_count - m * m;
                    v = v > 0.0 ? v : 0.0;
                    mu = (float)m; rstd = 1.0f / sqrtf((float)v + b.eps);
                } else {
                    mu = b.rmean[c]; rstd = 1.0f / sqrtf(b.rvar[c] + b.eps);
                }
            }
            cmean[c] = mu; csc[c] = g * rstd; cbeta[c] = be;
        }
        __syncthreads();
        {
            const float z = m0 + r < M ? 1.f : 0.f;
            const float v0 = __uint_as_float((unsigned)xv), v1 = __uint_as_float((unsigned)(xv >> 32));
            *(float2*)&As[r * P + k2] = make_float2(z * fmaxf(bn_apply(v0, cmean[k2], csc[k2], cbeta[k2]), 0.f),
                                                    z * fmaxf(bn_apply(v1, cmean[k2 + 1], csc[k2 + 1], cbeta[k2 + 1]), 0.f));
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < C1S_NP; ++i) {
            const int g = wave + 4 * i;
            if (g >= ng1 && g < ng16) {                // wave-uniform.  Group g went LAST into accumulator i % 2 of the unfused loop
                const float4 a = *(const float4*)(ar + 16 * g);
                const float4 b = rb[i];
                if (i & 1) {
                    acc1 = C1S_MFMA(a.x, zb * b.x, acc1); acc1 = C1S_MFMA(a.y, zb * b.y, acc1);
                    acc1 = C1S_MFMA(a.z, zb * b.z, acc1); acc1 = C1S_MFMA(a.w, zb * b.w, acc1);
                } else {
                    acc0 = C1S_MFMA(a.x, zb * b.x, acc0); acc0 = C1S_MFMA(a.y, zb * b.y, acc0);
                    acc0 = C1S_MFMA(a.z, zb * b.z, acc0); acc0 = C1S_MFMA(a.w, zb * b.w, acc0);
                }
            }
        }
    }
    __syncthreads();                                   // the panels are dead: Cs aliases them
    float* Cs = smem;                                  // [4 waves][16][17]
#pragma unroll
    for (int r = 0; r < 4; ++r) Cs[(wave * 16 + 4 * h + r) * 17 + li] = acc0[r] + acc1[r];      // C/D: column = lane & 15, row = 4 (lane >> 4) + r
    __syncthreads();
    double* red = (double*)(smem + 4 * 16 * 17);       // [2][16][16] (offset 4352 bytes: 8-byte aligned)
    const int r = tid >> 4, c = tid & 15, m = m0 + r, n = n0 + c;
    const float v = (Cs[r * 17 + c] + Cs[(16 + r) * 17 + c]) + (Cs[(32 + r) * 17 + c] + Cs[(48 + r) * 17 + c]);
    const bool ok = m < M && n < N;
    if (ok) p.y[(size_t)m * p.ldy + n] = v;
    if (p.osum == nullptr) return;
    red[r * 16 + c] = ok ? (double)v : 0.0;
    red[256 + r * 16 + c] = ok ? (double)v * v : 0.0;
    __syncthreads();
    if (tid < 16 && n0 + tid < N) {
        double s = 0, q = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) { s += red[i * 16 + tid]; q += red[256 + i * 16 + tid]; }
        atomicAdd(&stat_rep(p.osum, p.srep, p.sstride)[n0 + tid], s);
        atomicAdd(&stat_rep(p.osumsq, p.srep, p.sstride)[n0 + tid], q);
    }
}
