/* mmsurv.h -- C ABI of libmmsurv_hip.so: the MI355X (gfx950) implementation of the training hot path of
 * baek0203/multimodal_survival_prediction (per-batch forward/backward of the multimodal survival networks +
 * Cox partial likelihood).
 *
 * The reference has no FFI of its own: its boundary is the Python surface of scripts/training/<name>.py
 * (SURVEY.md section 8b).  Every entry point below replaces a torch/MONAI/torchsurv op sequence invoked from
 * that surface; the replaced call site is cited per function as R/<file>:<line> (R = the reference repo).
 *
 * Conventions
 *   - plain C: raw device pointers, sizes, POD parameter blocks; no torch/HIP C++ types in signatures
 *     (hipStream_t is an opaque pointer);
 *   - the CALLER owns every buffer (PyTorch caching allocator in the shipped host code); nothing here
 *     allocates, frees or synchronises; all work is enqueued on the given stream, so the calls are legal
 *     inside hipStreamBeginCapture/EndCapture;
 *   - return 0 on success, negative on error (MMS_ERR_*); never throws;
 *   - activations are channels-last fp32 matrices [rows = B*D*H*W][channels] ("slabs"); a dense block's
 *     torch.cat is a column offset into its slab;
 *   - BatchNorm batch statistics travel as fp64 (sum, sumsq) accumulators that the producer kernel's
 *     epilogue fills with atomics; they must be zeroed (hipMemsetAsync) once per step by the caller.
 */
#ifndef MMSURV_H
#define MMSURV_H
#include <stdint.h>
#include <stddef.h>

#ifndef HIP_INCLUDE_HIP_HIP_RUNTIME_API_H
typedef struct ihipStream_t* hipStream_t;
typedef struct ihipEvent_t* hipEvent_t;
#endif

#define MMS_OK 0
#define MMS_ERR_ARG (-1)
#define MMS_ERR_LAUNCH (-2)
#define MMS_MAX_GROUP 10     /* models per fold-group launch (the *_group entry points): 10 x the largest block (Conv1BwdP) stays under the 4 KB kernarg limit */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct Dims3 { int D; int H; int W; } Dims3;

/* Launch-shape options of the DenseNet121 drivers (mms_dn121_*) and of the convolution entry points they launch.  Kernel selection is a
 * function of the ARGUMENTS: the library reads no environment variable and keeps no per-process or per-thread setting.  A zero-filled
 * block (or a NULL pointer wherever an `opts` argument is taken) selects the defaults -- what the shipped entry points and bench.py run;
 * the other values exist for A/B measurements and for the parity tests that must reach one particular kernel form.  Never stored: the
 * block is read during the call only.  Forward and backward calls on one workspace must pass the same values. */
typedef struct MmsDnOpts {
    int out_features;      /* width N of class_layers.out ([N][1024] weight, [N] bias; out / dout carry N columns), 0 = 128
                              (R/scripts/training/simple_fusion.py:163 img_feature_dim); 1 <= N <= 4096 */
    int persist_b4;        /* dense block 4 with <= 16 rows as ONE launch per pass (csrc/dn_b4.hip): 0 = both passes, 1 = forward only,
                              -1 = per-layer launches.  The persistent launches need their 8 workgroups per model co-resident: a caller
                              that may have more of them in flight than the chip has CUs passes -1 */
    int persist_b3;        /* dense block 3's forward as one persistent launch when a sample has <= 32 voxels there (csrc/dn_cl.hip: clusters
                              of 8 workgroups per sample, BatchNorm partial sums exchanged between them): 1 = on; 0 (default) / -1 = per-layer
                              launches -- measured faster at 32 voxels per sample (profiles/r04_cluster_kernels.txt) */
    int split_wgs;         /* target workgroups of a tap-split conv2 launch, 0 = 256 */
    int conv1_ksplit;      /* -1 = never split the conv1 K loop over workgroups (0 = by launch size) */
    int conv1_small;       /* whole-K 16x16-tile conv1 forward (csrc/dn_c1s.hip): 0 = launches of <= c1s_max_wgs tiles, 1 = whenever the
                              shape allows, -1 = never */
    int c1s_max_wgs;       /* 0 = 640 */
    int conv1_small_bwd;   /* whole-M conv1 backward-data with norm1's backward fused (csrc/dn_c1s.hip): 0 = up to 128 rows, -1 = never */
    int fuse_apply_rows;   /* most rows for which norm1's backward rides in the conv1 backward-data launch, 0 = 128 (32 with
                              conv1_small_bwd = -1) */
    int conv3_small;       /* all-tap 16-row conv2 kernels for small grids (csrc/dn_c3s.hip): 0 = whenever the grid fits (one or two
                              16-column output tiles per wave by launch size), 1 / 2 = force that number, -1 = never */
    int c3s_ring;          /* weight-ring depth of their one-tile form: 0 = 6; 4, 6 or 9 */
    int conv3_mt;          /* multi-tap conv2 forward: 0 = by launch size, 2 / 3 = force it on 64- / 32-row tiles, -1 = never */
    int conv3_mt32_min;    /* fewest 32-row tiles for it, 0 = 256 */
    int conv3w_mt;         /* multi-tap conv2 weight gradient: 0 = by launch size, 2 = force, -1 = never */
    int big_ng;            /* -1 = tile shapes of the 1x1x1 kernels from ONE model's work (arithmetic independent of the group size) */
    int batch_w;           /* weight-gradient launches deferred to the end of their dense block and batched over layers: 0 = every block,
                              1 = blocks 2-4 only (rounds 2-3), -1 = one launch pair per layer */
    int ms3_rows;          /* rows per conv2 weight-gradient workgroup, 0 = by launch size */
    int ms1_div;           /* divisor of the conv1 weight-gradient row chunks, 0 = by launch size */
    int c0_nwg;            /* workgroups of the pooled conv0 weight-gradient kernel, 0 = default */
    int c0f_nwg;           /* workgroups of the pooled conv0 forward kernel, 0 = default */
    int w2_packed;         /* 1: the 58 conv2 weight tensors (and their gradients) are stored [cout][tap][cin] -- "packed primary" -- instead
                              of torch's [cout][cin][taps]: the forward reads them as they are, the weight-gradient kernels write the
                              gradient in place (no pack launch, no gradient scratch, no unpack launch in the step), and the parameter
                              table carries 116 more pointers: params[364 + 2 l] = layer l's backward-data pack, params[364 + 2 l + 1] =
                              its forward MFMA-fragment pack (layers of mms_dn121_w2_fragmask; else unused) -- kept current by the caller:
                              mms_clip_adam writes them with the update (AdamP.w2_*), mms_w2_pack after any other change of the weights.
                              0: torch layout, packs and unpack inside the drivers (rounds 1-3) */
    int trans_prepass;     /* transitions: 0 = AvgPool3d(relu(norm(x))) by its own launch into the workspace (mms_pool_act), the 1x1x1 convolution
                              and its weight gradient read that pooled operand; -1 = pooled while loading, inside both GEMMs (each of the N / 16-32
                              column tiles of a row tile re-reads and re-normalises the 8 source voxels: rounds 1-3) */
    int fuse_layers;       /* dense block 3's forward with conv2 of layer l and conv1 of layer l + 1 in ONE launch (csrc/dn_c3s.hip; the conv1
                              workgroups wait inside the launch for the conv2 ones): 0 = wherever the block runs the small-grid kernels
                              (<= 128 rows, <= 4 models per launch, one statistic replica, no SyncBN / statistics hook, persist_b3 off),
                              -1 = never.  A caller that may have more such launches in flight than the chip holds passes -1
                              (ops.persistent_opts); a wait that times out raises the drivers' error word (mms_dn121_region "b4_err") */
    int wgrad_tab;         /* deferred weight gradients of dense blocks 2-4 (batch_w >= 0): 0 = every (model, layer) member of a block in ONE
                              conv2 and ONE conv1 launch at the block's end, the members described by compact records over the layer tables
                              mms_dn121_init wrote (mms_wgrad_tab_group; the parameter pointers of the call must be those given to
                              mms_dn121_init); -1 = launches of at most MMS_MAX_GROUP by-value members (rounds 2-5) */
    int skip_dead_bwd;     /* encoder backward of a model whose feature gradient is all zero (a batch without a CT under a modality mask):
                              0 = the head launch of mms_dn121_backward / _group records in the workspace word "bwd_live" whether any
                              element of dout compares unequal to 0.0f (NaN counts; -0.0f is zero), and every later launch of the call
                              returns at once for a model whose word is 0 -- every quantity they compute is linear in dout, so they would
                              add exact zeros to the gradients.  The word is data, not a launch parameter: one captured graph serves live
                              and dead batches.  -1 = every launch does its work whatever dout holds.  Never on under SyncBN or a
                              statistics hook (the BatchNorm-backward sums couple the ranks), in mms_dn121_backward_stage and in
                              mms_dn121_input_grad (they do not run this call's head launch).  The one difference in results: with a
                              zero dout and a non-finite saved activation the full backward yields NaN gradients, the skipped one none */
    int c0_zero_skip;      /* all-zero input boxes of features.conv0 (the zero-filled volume of a patient without a CT), boxed kernels only:
                              0 = a 4x4x4-voxel output box of the forward whose 13x13x13 input region (halo included) compares equal to 0.0f
                              everywhere gets +0.0f stored to its outputs and adds nothing to the statistics instead of running its MFMAs;
                              a 2x4x4 box of the weight gradient whose 9x13x13 region is all zero skips its MFMAs, and a workgroup whose
                              boxes of a model were all zero skips its atomic flush.  Decided inside the kernels from the data they stage
                              (-0.0f is zero, NaN is not): no flag from the caller, nothing to go stale.  -1 = every box does its work
                              (A/B runs, tests).  Either way the boxes of a model are walked sample-minor (box j / B of sample j % B), so
                              the statistics and the weight gradient are summed in that grouping.  The one difference in results: with a
                              non-finite conv0 weight the full forward gives NaN in a zero box, the skip gives 0; with a non-finite dy0 the
                              full weight gradient gives NaN, the skip gives none */
    int dup_zero;          /* identical all-zero volumes of a batch (patients without a CT) computed once by the multi-tap conv2 forward kernel
                              (dense block 1 of the real volumes): 0 = the boxed conv0 forward counts the zero boxes of every sample into the
                              workspace words "zero_words" (a sample is zero iff its word equals the boxes per sample); a multi-tap launch
                              whose rows per sample are a multiple of its tile height then computes the tiles of the FIRST zero sample only,
                              stores each of them to the same sample-relative rows of every other zero sample and multiplies its statistic
                              partials by the number of zero samples (in fp64: exact) -- the workgroups of the other
                              zero samples return, and the computed tiles are dealt evenly over the model's XCDs ("compacting form").  Every
                              buffer is left complete, so nothing downstream changes.  1 = the same, but a duplicate's workgroup merely
                              returns where it stands ("masking form"; A/B).  -1 = every sample does its work.  The words are data written
                              by an earlier launch of the same forward from the volumes themselves: no flag from the caller, one captured
                              graph serves every batch.  Off by itself when c0_zero_skip = -1 or conv0 takes the unboxed form (words stay 0),
                              with more than 32 samples, and under SyncBN or a statistics hook.  Results: activations bit-identical; the
                              statistics differ in summation order only.  The one difference: a non-finite value reaches all zero samples
                              from the first one's computation -- which is what the full computation yields too */
    int dup_zero_bwd;      /* the same in the backward of block 1's conv2.  The gradient rows of a model's zero samples are identical through the
                              whole backward iff their rows of dout are equal; under a modality mask an absent CT's row is exactly zero.  So the
                              head launch of mms_dn121_backward / _group leaves in the workspace word "bwd_dup" the bit mask of
                              D = { b : zero_words[b] == boxes per sample and row b of dout compares equal to 0.0f in every element } (NaN
                              counts as non-zero, -0.0f as zero), or 0 when |D| < 2, B > 32 or dout is too large for the live scan.  The
                              multi-tap backward-data kernel then computes the tiles of the lowest sample of D only, stores them to the same
                              rows of the others and multiplies its BatchNorm-backward partials by |D| (compacting form, as the forward); the
                              multi-tap weight-gradient kernel takes its row chunks over the rows of the samples outside D \ {lowest} and
                              scales the lowest one's dz rows by |D|.  0 = both kernels, 1 = backward-data only, 2 = weight gradient only,
                              -1 = off.  On under the conditions of skip_dead_bwd AND of dup_zero (so never under SyncBN or a statistics
                              hook, in backward stages, in mms_dn121_input_grad, or with dup_zero = -1), where rows per sample are a multiple
                              of 32 and 2 <= B <= 32.  Every other kernel form ignores the word.  Results: dbn bit-identical, sums and weight
                              gradients in another summation order (and |D| x row instead of |D| equal rows) */
} MmsDnOpts;

/* BatchNorm parameter source. train=1: batch statistics from the fp64 accumulators; train=0: running stats.
 * (torch BatchNorm3d/1d, eps 1e-5, momentum 0.1: R/scripts/training/final_multimodal.py:77-96; MONAI norm="batch")
 * The 3x3x3-convolution entry points (mms_conv3_fwd*, mms_conv3_bwd_weight*) read the block with 16-byte vector loads: every array
 * they use (and rep_stride * 8 when nrep > 1) must be 16-byte aligned, else MMS_ERR_ARG.
 * gamma == NULL: the IDENTITY (mean 0, scale 1, shift 0; every other field ignored) -- for an operand that is already normalised and
 * non-negative (the pooled transition operand of mms_pool_act): relu(identity(x)) == x exactly. */
typedef struct BnSrc {
    const double* sum;     /* [C] batch sum      (train) */
    const double* sumsq;   /* [C] batch sum x^2  (train) */
    const float* rmean;    /* [C] running mean   (eval)  */
    const float* rvar;     /* [C] running var    (eval)  */
    const float* gamma;    /* [C] */
    const float* beta;     /* [C] */
    float inv_count;       /* 1 / rows the statistics were taken over */
    float eps;
    int train;
    int nrep;              /* accumulator replicas (0/1 = one): sum[c + r*rep_stride], r < nrep, are added up by the reader */
    int rep_stride;        /* in doubles */
} BnSrc;


// ---- 1x1x1 conv (dense-layer conv1, transition conv): y = relu(bn(x)) [avg-pooled 2x2x2] @ W^T -------
typedef struct Conv1FwdP {
    const float* x; int ldx;        // input slab [Min][ldx], first K columns used
    int M;                          // output rows (pooled rows when pool=1)
    int K;                          // input channels (multiple of 32)
    const float* w;                 // [N][K] (torch Conv3d weight (N,K,1,1,1))
    int N;
    float* y; int ldy;              // output [M][ldy] (column offset already applied)
    BnSrc bn;                       // over the K input channels
    double* osum; double* osumsq;   // [N] batch-stat accumulators of y (nullptr in eval)
    int pool;                       // 1: AvgPool3d(2,2) of relu(bn(x)) before the GEMM (== conv then pool)
    Dims3 in;                       // input grid (pool=1)
    int srep; int sstride;          // statistic-accumulator replicas written by this op: workgroup x adds to replica x % srep (stride in doubles)
    /* optional split of the K (input-channel) loop over ksplit workgroups per 32x32 tile (small M: the loop is a chain of
       dependent memory round trips).  Each publishes its partial tile in `partial` [ksplit][M][N] and takes a ticket in
       `counters` [tiles]; the LAST one to arrive sums the partials in fixed order (deterministic), writes y and the
       statistics -- no second launch.  counters must be zero on entry (the fixing workgroup re-arms them). */
    float* partial; int ksplit; unsigned* counters;
} Conv1FwdP;

// ---- 3x3x3 conv, pad 1 (dense-layer conv2): slab[:, coff:coff+32] = conv3(relu(bn(y1)), W) ---------------
typedef struct Conv3FwdP {
    const float* y1;                // [M][128]
    const int* coords;              // [M] packed (d,h,w)
    Dims3 g; int M;
    const float* wp;                // packed [32][27][128]  (cout, tap, cin)
    float* out; int ldo;            // slab + coff, row pitch
    BnSrc bn;                       // over 128 channels of y1
    double* osum; double* osumsq;   // [32] (nullptr in eval)
    float* partial;                 // optional scratch [nsplit][M][32]: split the 27 taps over nsplit workgroups per tile,
                                    // then a reduce kernel sums them, writes the slab columns and the statistics
    int nsplit;                     // 1..27 (used when partial != null); workgroup z handles taps [z*ceil(27/nsplit), ...)
    int srep; int sstride;          // statistic-accumulator replicas written by this op: workgroup x adds to replica x % srep (stride in doubles)
    int wfrag;                      // 1: wp is in MFMA-fragment order [tap][cin/32][(cin/16)%2][cout/16][lane = ((cin/4)%4)*16 + cout%16][cin%4]
                                    // (mms_pack_conv3_frag): every weight load of the small-grid kernel is one contiguous 1 KB per wave.
                                    // Only with partial == null on grids that kernel takes (H*W + W + 1 <= 52), else MMS_ERR_ARG
    const unsigned* zwords; int zbps;   // optional (MmsDnOpts.dup_zero): the model's zero-box counts per sample as mms_conv0_fwd_group_zw left them, and the
                                    // boxes per sample; sample b is a zero volume iff zwords[b] == zbps.  NULL / 0 = every sample is computed.
                                    // Read by the multi-tap kernel only, and only when M / (D*H*W) <= 32 samples of a multiple of the tile height
} Conv3FwdP;

// ---- conv0: Conv3d(1,64,k7,s2,p3,no bias) -------------------------------------------------------------
typedef struct Conv0FwdP {
    const float* x;                 // [B][D][H][W]
    Dims3 in; Dims3 out;            // out = ceil(in/2)
    const int* coords;              // [M0] packed (od,oh,ow)
    int M;                          // B*out voxels
    const float* w;                 // [64][343]
    float* y;                       // [M][64]
    double* osum; double* osumsq;   // [64]
    int srep; int sstride;          // statistic-accumulator replicas written by this op: workgroup x adds to replica x % srep (stride in doubles)
} Conv0FwdP;

// ---- bn0 + relu + MaxPool3d(3,2,1) -> slab1[:, 0:64] -----------------------------------------------------
typedef struct PoolFwdP {
    const float* y0; Dims3 in;      // [B*in][64]
    Dims3 out; int B;
    float* slab; int ld;            // [B*out][ld]
    uint8_t* argmax;                // [B*out][64] tap index 0..26 of the first maximum (torch scan order)
    BnSrc bn;
    double* osum; double* osumsq;   // [64] stats of the pooled output (nullptr in eval)
    int srep; int sstride;          // statistic-accumulator replicas written by this op: workgroup x adds to replica x % srep (stride in doubles)
} PoolFwdP;

// ---- transition pre-pass: y[m'][k] = AvgPool3d(2,2)(relu(bn(x)))[m'][k] (MONAI _Transition: norm, relu, conv, pool == norm, relu, pool, conv) ----
typedef struct PoolActP {
    const float* x; int ldx;        // [B*in][ldx], first K columns used
    int K;                          // channels (multiple of 4)
    BnSrc bn;                       // over the K channels
    Dims3 in; int Mout;             // input grid (even dims); Mout = B * in / 8 pooled rows
    float* y; int ldy;              // [Mout][ldy]
} PoolActP;

// ---- norm5 + relu + global-avg-pool + Linear(1024,128) ---------------------------------------------------
// Any B.  B * C * 4 <= 64 KiB (B <= 16 at C = 1024): a workgroup pools all B samples into LDS and writes its four output columns,
// grid (ceil(N / 4), 1, ng).  Above that the samples are split into chunks of floor(64 KiB / (C * 4)) over grid.y: a workgroup pools ITS
// chunk and writes its four columns of those samples, grid (ceil(N / 4), ceil(B / chunk), ng).  Same BatchNorm constants and the same
// order of additions per sample in both forms.  C * 4 <= 64 KiB (one sample's pooled row must fit).
typedef struct HeadFwdP {
    const float* slab; int ld; int C; int B; int V;   // [B*V][ld], C channels, V voxels per sample
    BnSrc bn;
    const float* w; const float* bias; int N;          // [N][C]
    float* pooled;                                     // [B][C] saved for backward
    float* out; int ldo;                               // [B][ldo] first N columns written
} HeadFwdP;

// =========================== backward ==================================================================
// BatchNorm backward constants of one layer: sums accumulated by the producer of dbn.
typedef struct BnBwd {
    const double* s1;      // [C] sum_m dbn
    const double* s2;      // [C] sum_m dbn * xhat
    int nrep; int rep_stride;   // replicas as in BnSrc
} BnBwd;

// conv3 backward-data: dbn2 = (dz (*) W^T) * [a2 > 0], plus BN2-backward sums
typedef struct Conv3BwdDataP {
    const float* dz; int lddz;      // dslab + coff  [M][lddz], 32 columns
    const int* coords; Dims3 g; int M;
    const float* wpb;               // packed [128][27][32] (cin, tap, cout)
    const float* y1;                // [M][128] forward pre-BN activations
    BnSrc bn;                       // bn2
    float* dbn;                     // [M][128] out
    double* s1; double* s2;         // [128] out (atomics)
    float* partial;                 // optional scratch [nsplit][M][128]: tap split as in Conv3FwdP
    int nsplit;
    int srep; int sstride;          // statistic-accumulator replicas written by this op: workgroup x adds to replica x % srep (stride in doubles)
    int wfrag;                      // 1: wpb is in MFMA-fragment order [tap][cin/16][cout/16][lane = ((cout/4)%4)*16 + cin%16][cout%4] (mms_pack_conv3_frag); as Conv3FwdP.wfrag
    const unsigned* live;           // optional (MmsDnOpts.skip_dead_bwd): device word; 0 = every workgroup of this member returns at once.  NULL = always run.
                                    // (PoolBwdP, HeadBwdP and MmsWgradModel keep their layouts: the drivers pass their words beside them, csrc/dn_ops.h)
    const unsigned* dup;            // optional (MmsDnOpts.dup_zero_bwd): device word, the bit mask of the samples whose dz AND y1 rows are identical
                                    // (mms_head_bwd_group_dup); fewer than two bits below M / (D*H*W) = nothing to share.  NULL = off.  Read by the
                                    // multi-tap kernel only, and only with 2..32 samples of a multiple of 32 rows
} Conv3BwdDataP;

// conv3 backward-weight: dW[cout][cin][tap] += sum_m relu(bn(y1))[nbr(m,tap)][cin] * dz[m][cout]
typedef struct Conv3BwdWP {
    const float* y1; const int* coords; Dims3 g; int M;
    BnSrc bn;
    const float* dz; int lddz;
    float* dw;                      // gradient, accumulated with atomics; layout by dw_layout
    int msplit;                     // grid.z = 27 * msplit
    int dw_layout;                  // 0: canonical torch layout [32 cout][128 cin][27 taps] (every atomic on its own cache line);
                                    // 1: a zeroed scratch in [27][32][128] (tap, cout, cin) order: 512-byte contiguous runs = full atomic
                                    //    rate; mms_unpack_conv3_grads adds it into the canonical gradient;
                                    // 2: [32][27][128] (cout, tap, cin) -- the PACKED PRIMARY layout of MmsDnOpts.w2_packed: the same
                                    //    512-byte runs, and the buffer IS the parameter's gradient (no scratch, no unpack)
    const unsigned* live;           // optional, as Conv3BwdDataP.live
    const unsigned* dup;            // optional, as Conv3BwdDataP.dup: the multi-tap kernel walks the rows of every sample but the mask's higher ones and
                                    // counts the lowest one's rows once per sample of the mask.  NULL = off
} Conv3BwdWP;

/* Weight gradients of many (model, layer) members of ONE dense block as one launch per op (csrc/dn_bwd.hip): the members' parameter
 * blocks (Conv3BwdWP / Conv1BwdP, has_bn_out = 1, pool = 0, N = 128, K = C0 + 32 * layer) are rebuilt on the device from a per-model
 * header, the model's device table of layer entries, and a small per-member record -- so a launch carries up to
 * MMS_WGRAD_MAX_MEMBERS members instead of the MMS_MAX_GROUP by-value blocks that fit the 4 KB kernel-argument segment.
 * Layer entry = 15 pointers (csrc/dn_ops.h B4Layer, written by mms_dn121_init), of which these are read: [0] norm1 gamma, [1] norm1
 * beta, [3] norm2 gamma, [4] norm2 beta, [11] y1 [M][128], [12] y1's (sum | sumsq) [2][128] (x srep replicas, stride 256 doubles),
 * [13] masked gradient at norm2's output [M][128], [14] its BatchNorm-backward sums (s1 | s2) [2][128] (replicas likewise). */
#define MMS_WGRAD_MAX_MODELS 5
#define MMS_WGRAD_MAX_MEMBERS 90
typedef struct MmsWgradModel {
    const void* tab;            // device table of the block's layer entries
    const float* slab;          // [M][ld] block activations (conv1's input: columns [0, K))
    const float* dslab;         // [M][ld] their gradient (conv2's dz of layer l: columns [C0 + 32 l, + 32))
    const int* coords;          // [M] packed voxel coordinates
    const double* st_slab;      // (sum | sumsq) [2][ld] of the slab channels (x srep replicas, stride 2 ld doubles)
    int M; Dims3 g; int srep;   // rows, the block's voxel grid, statistic replicas -- equal for every model of a launch
} MmsWgradModel;
typedef struct MmsWgradMember {
    float* dw2;                 // conv2 weight gradient (layout: MmsWgradShape.dw_layout), accumulated with atomics
    float* dw1;                 // conv1 weight gradient [128][K], accumulated with atomics
    float* dgamma2; float* dbeta2;      // [128] norm2 parameter gradients, accumulated by one workgroup of the conv1 launch
    int model; int layer;       // index into the launch's models, layer of the block (table index)
} MmsWgradMember;
typedef struct MmsWgradShape {
    int ld; int C0;             // slab row pitch (the block's final channel count), input channels of layer 0
    int ms3; int ms1;           // row chunks of the conv2 / conv1 launch (Conv3BwdWP.msplit / Conv1BwdP.msplit)
    int dw_layout;              // Conv3BwdWP.dw_layout
    int count;                  // rows the BatchNorm statistics were taken over (M x ranks)
} MmsWgradShape;

// 1x1 conv backward (dense conv1 and transition conv).
//   dy[m][n]  = g2[n]*rstd2[n]*(dbn2[m][n] - s1[n]/M - yhat[m][n]*s2[n]/M)     (has_bn_out=1)
//             = dyraw[m][n]                                                     (has_bn_out=0, transition)
//   dW[n][k] += sum_m dy[m][n] * a[m][k],   a = relu(bn_in(x)) [avg-pooled]
//   da[m][k]  = sum_n dy[m][n] * W[n][k];   dbn_in = da * [a>0] (un-pooled /8 when pool) ; sums s1,s2 over k
typedef struct Conv1BwdP {
    // output-side gradient
    const float* dyraw; int lddy;   // [M][lddy]: dbn2 (has_bn_out) or dslab_next (transition)
    const float* y; int ldy;        // forward output of this conv (pre-BN2), needed when has_bn_out
    BnSrc bn_out; BnBwd bb_out; int has_bn_out;
    int M; int N;                   // rows of dy (pooled rows when pool), N output channels
    // input side
    const float* x; int ldx; int K; BnSrc bn_in;
    const float* w;                 // [N][K]
    int pool; Dims3 in;             // transition: x grid dims (rows of x = M*8)
    float* dw;                      // [N][K] accumulated with atomics (weight kernel)
    float* dbn; int lddbn;          // [Mx][lddbn] out (data kernel), Mx = M*(pool?8:1)
    double* s1; double* s2;         // [K] out (data kernel)
    int msplit;
    float* dgamma_out; float* dbeta_out;   // [N] BN2 parameter grads (= s2_out, s1_out), written by the weight kernel
    int srep; int sstride;          // statistic-accumulator replicas written by this op: workgroup x adds to replica x % srep (stride in doubles)
    /* optional (data kernel, pool = 0, M <= 128 rows): norm1's backward fused into the epilogue -- a workgroup then owns all rows of
       its channels, so the two BN-backward sums are complete locally: fuse_dx[:, 0:K] (+)= gamma*rstd*(dbn - s1/M - xhat*s2/M),
       fuse_dgamma += s2, fuse_dbeta += s1; dbn / s1 / s2 are not written and no mms_bn_bwd_apply launch follows. */
    float* fuse_dx; int fuse_lddx; int fuse_accumulate;
    float* fuse_dgamma; float* fuse_dbeta;
    const unsigned* live;           // optional, as Conv3BwdDataP.live (data and weight kernels)
} Conv1BwdP;

// dslab[:, 0:C] (+)= g*rstd*(dbn - s1/M - xhat*s2/M)
typedef struct BnBwdApplyP {
    const float* dbn; int lddbn;
    const float* x; int ldx;
    float* dx; int lddx;
    int M; int C; BnSrc bn; BnBwd bb; int accumulate;
    float* dgamma; float* dbeta;    // [C] written by block 0 (dgamma = s2, dbeta = s1)
    const unsigned* live;           // optional, as Conv3BwdDataP.live
} BnBwdApplyP;

typedef struct HeadBwdP {
    const float* dout; int lddout;  // [B][lddout] first N columns read
    const float* pooled;            // [B][C]
    const float* slab; int ld; int C; int B; int V; BnSrc bn;
    const float* w; int N;
    float* dw; float* dbias;        // [N][C], [N]
    float* dgamma; float* dbeta;    // [C]
    float* dslab; int ldd;          // [B*V][ldd] first C columns written
    double* ext_sums;               // mms_head_bwd_sums / _apply only: [2][C] norm5-backward sums (s1 | s2), zeroed by the caller
} HeadBwdP;

typedef struct PoolBwdP {                   // maxpool backward + relu0 mask -> dbn0, sums
    const float* dslab; int ld;     // [B*out][ld] first 64 columns
    const uint8_t* argmax; Dims3 out; Dims3 in; int B;
    const float* y0; BnSrc bn;
    float* dbn;                     // [B*in][64]
    double* s1; double* s2;         // [64]
    const int* coords;              // optional [B*in] packed (d,h,w) of the conv0 grid (saves the per-voxel integer divisions)
    int srep; int sstride;          // statistic-accumulator replicas written by this op: workgroup x adds to replica x % srep (stride in doubles)
} PoolBwdP;

typedef struct Conv0BwdWP {                 // dW0[64][343] += sum_m bn0bwd(dbn0)[m][n] * x[patch(m,k)]
    const float* dbn; const float* y0; BnSrc bn; BnBwd bb;
    const float* x; Dims3 in; Dims3 out; const int* coords; int M;
    float* dw; int msplit;
    float* dgamma; float* dbeta;    // [64]
    float* dw_rep; int nrep;        // optional: nrep zeroed replicas [nrep][64*343] -- workgroup x adds to replica x % nrep and a second launch adds the
                                    // replicas into dw (256 workgroups x 22 k atomics on the 686 lines of ONE gradient serialise at the memory side);
                                    // NULL / 0: atomics straight into dw
    const unsigned* live;           // optional, as Conv3BwdDataP.live (both launches)
} Conv0BwdWP;

/* conv0 backward-data with norm0 frozen (input-gradient attribution; csrc/attrib.hip):
 *   dx[b,d,h,w] = sum_c sum_taps a_c * dbn[b,(d+3-kd)/2,(h+3-kh)/2,(w+3-kw)/2,c] * w[c][kd,kh,kw],  a_c = gamma_c / sqrt(rvar_c + eps)
 * over the taps whose three quotients are integral and inside the output grid.  dx is WRITTEN (every element, no atomics: two calls give
 * the same bits); the caller need not zero it.  bn.train must be 0 (running statistics); out = ceil(in / 2) per axis. */
typedef struct Conv0BwdDataP {
    const float* dbn;               // [B*out][64] gradient at norm0's output, already masked by relu0 (what mms_pool_bwd leaves)
    BnSrc bn;                       // norm0, train = 0: gamma and rvar are read
    const float* w;                 // [64][343]
    Dims3 in; Dims3 out;            // out = ceil(in/2)
    int M;                          // B*out voxels
    float* dx;                      // [B][D][H][W]
} Conv0BwdDataP;

/* =========================== fallback CT encoder (R/scripts/training/final_multimodal.py:75-86) ==================
 * 3 x [Conv3d(k3, s2, p1, bias) + BatchNorm3d + ReLU] (1->32->64->128) + AdaptiveAvgPool3d(1): what the reference
 * runs when MONAI is absent.  Channels-last activations; each conv stores its raw output (+bias) and batch
 * statistics, BN+ReLU of layer l is applied while layer l+1 (or the pooling) reads it. */
typedef struct FbConvP {
    const float* x; int Cin; Dims3 in; Dims3 out; int B;     // x: [B*in][Cin] raw output of the previous conv (or the volume, Cin=1)
    int has_bn; BnSrc bn;                                    // BN+ReLU of the previous layer (has_bn=0 for the first conv)
    const float* w; const float* bias; int Cout;             // torch layout [Cout][Cin][27], [Cout]
    float* y;                                                // [B*out][Cout]
    double* osum; double* osumsq;                            // [Cout] (nullptr in eval)
    /* backward (fb_conv_bwd_w / fb_conv_bwd_x) */
    const float* dy;                                         // [B*out][Cout] gradient w.r.t. y
    float* dw; float* dbias;                                 // accumulated (atomics)
    float* dbn_in; double* s1; double* s2;                   // [B*in][Cin] masked input gradient + BN-backward sums (bwd_x)
    int msplit;
} FbConvP;

typedef struct FbPoolP {     /* BN+ReLU+global average pool and its backward */
    const float* y; int C; int V; int B; BnSrc bn;           // [B*V][C]
    float* out; int ldo;                                     // [B][ldo] first C columns
    const float* dout; int lddout;
    float* dbn; double* s1; double* s2;
} FbPoolP;

/* =========================== heads: small-batch MLP, gate, Cox, optimizer ============================== */
/* Input prologue of a Linear layer: x' = dropout(relu(bn1d(x))) -- the BatchNorm1d/ReLU/Dropout that FOLLOW the
 * previous Linear in the reference's nn.Sequential (R/scripts/training/final_multimodal.py:93-117) are applied
 * while this layer reads its input.  All M rows of a column sit in one lane, so batch statistics need no atomics. */
typedef struct InProlog {
    int bn;                         // 1: BatchNorm1d (+ReLU) on the input columns
    const float* gamma; const float* beta;
    float* rmean; float* rvar; long long* nbt;   // running stats (read in eval, momentum-updated in train by fwd)
    float eps; float momentum;
    int train;
    float drop_p;                   // dropout probability applied after bn+relu (0 = none; ignored in eval)
    const float* drop_mask;         // optional explicit multiplicative mask [M][K] (already scaled by 1/(1-p)); parity mode
    const uint32_t* rng;            // device {seed, step} for the hash RNG when drop_mask is null
    uint32_t stream_id;             // distinguishes dropout sites
} InProlog;

typedef struct LinearFwdP {
    const float* x; int ldx; int M; int K;
    InProlog pro;
    const float* w; const float* bias; int N;     // torch Linear: w [N][K]
    float* y; int ldy; int out_relu;              // y = [relu](x' W^T + b)
} LinearFwdP;

typedef struct LinearBwdP {
    const float* dy; int lddy;      // gradient w.r.t. y (post-activation) [M][lddy]
    const float* y; int ldy;        // forward output (relu mask when out_relu)
    int out_relu;
    const float* x; int ldx; int M; int K; InProlog pro;
    const float* w; int N;
    float* dw; float* dbias;        // accumulated (+=)
    float* dx; int lddx;            // gradient w.r.t. the RAW input x (before the prologue) [M][lddx]; null = skip
    float* dgamma; float* dbeta;    // prologue BN parameter grads (+=), null when pro.bn == 0
} LinearBwdP;

/* Gated late fusion (R/scripts/training/partial_modality_training.py:257-271): feats [M][288] = ct|rna|clin,
 * mask [M][3]; masked = feats*mask; gate = softmax(W2 relu(W1 [masked|mask] + b1) + b2); fused = masked*gate.
 * Any M, one workgroup per row.  mms_gate_bwd at M > 32: row-tiled form -- a workgroup owns 8 consecutive rows, keeps its share of
 * dw1 / db1 / dw2 / db2 in registers over them and flushes once (1/8 of the per-row form's fp32 atomics); same values per row. */
typedef struct GateP {
    const float* feats; const float* mask; int M;
    const float* w1; const float* b1; const float* w2; const float* b2;   // [64][291],[64],[3][64],[3]
    float* hidden;                  // [M][64] saved
    float* gate;                    // [M][3]  saved / output
    float* fused;                   // [M][288]
    // backward
    const float* dfused;            // [M][288]
    float ent_weight;               // lambda * upstream of gate_entropy_loss (R/...:322-331); 0 = none
    const float* dgate_ext;         // optional [M][3]: external gradient w.r.t. the gate weights (autograd path)
    float* dfeats;                  // [M][288]
    float* dw1; float* db1; float* dw2; float* db2;   // accumulated (atomics)
    float* entropy;                 // optional scalar out (fwd): -mean_b(entropy_b)
} GateP;

/* Cox negative partial log-likelihood (R/scripts/training/final_multimodal.py:158-186): Breslow risk sets
 * loss = -(1/n_e) sum_{i:e_i} (h_i - log sum_{j: t_j>=t_i} exp h_j), or torchsurv's Efron tie handling (tie_mode).
 * valid: optional per-sample 0/1 (has_survival); excluded samples get dh = 0.
 * out[0] = loss, out[1] = 1 if the batch is usable (>=2 valid samples and >=1 event) else 0 (loss 0, dh 0). */
typedef struct CoxP {
    const float* h; int ldh;        // log-hazards, element i at h[i*ldh]
    const float* time; const float* event; const float* valid; int n;
    float scale;                    // upstream gradient
    float* lse;                     // [n] workspace (multi-block path)
    float* dh; int lddh;            // dL/dh (null = forward only)
    float* out;                     // [2]
    int tie_mode;                   // 0: Breslow risk sets (= every formulation of the reference on distinct times);
                                    // 1: Efron tie correction as torchsurv's neg_partial_log_likelihood applies it when times
                                    //    repeat (R/scripts/training/final_multimodal.py:158-162): the m events tied at a time
                                    //    take the denominators D - (l/m) T, l = 0..m-1, and the loss is the MEAN over the
                                    //    distinct event times (on distinct times both modes give the same value)
    float* tie_frac;                // [n] workspace (tie_mode 1): l/m of each event
} CoxP;

/* One span of mms_zero_spans_group: `bytes` > 0 bytes at p, any alignment. */
typedef struct MmsZeroSpan {
    void* p; size_t bytes;
} MmsZeroSpan;

/* Harrell C, pair counting (R/scripts/training/simple_fusion.py:59-73): counts[0]=concordant (h_i>h_j),
 * counts[1]=tied hazards, counts[2]=permissible pairs (e_i==1, t_j>t_i). */
typedef struct CindexP {
    const float* h; const float* time; const float* event; int n;
    unsigned long long* counts;     // [3], zeroed by the caller
} CindexP;

/* Weighted (bootstrap) Harrell-C pair counts of M models on R multiplicity vectors, exact integers (csrc/cindex_boot.hip).
 * A replicate that drew patient i w_i times has  2*concordant + tied = sum_ij w_i w_j S[i][j]  and  comparable = sum_ij w_i w_j P[i][j],
 * P[i][j] = [pair (i, j) is comparable, i the member with the observed earlier event], S = P o (2 [hrank_i > hrank_j] + [hrank_i == hrank_j]):
 * what counting pairs on the literally resampled arrays gives.  The kernel forms W.S and W.P on the int8 matrix cores without ever storing
 * an n x n matrix (memory: the arguments only) and compares integer ranks, so ties are exactly the caller's ties.
 * Ranks: 0 <= rank < 2^31 - 1 (dense ranks as of numpy.unique(return_inverse=True)).  Limits: 1 <= n <= MMS_CBOOT_MAX_N, which keeps the
 * int32 column sums (<= 2 * 127 * n) in range for every permitted w; 1 <= R <= MMS_CBOOT_MAX_R; 1 <= M <= MMS_CBOOT_MAX_M.  The input may be
 * in any order (time-sorted input lets the kernel skip about half of its tiles).  w 16-byte, out 8-byte, the int arrays 4-byte aligned.
 * A NULL required pointer, a size out of range, ldw < n or not a multiple of 64, ldh < n, a misaligned pointer or an unknown pair_rule:
 * MMS_ERR_ARG before any launch.  The adds into `out` are integer atomics: two calls give the same numbers. */
#define MMS_CBOOT_MAX_N 1048576
#define MMS_CBOOT_MAX_R 1048576
#define MMS_CBOOT_MAX_M 8
typedef struct CbootP {
    const int* hrank; int ldh; int M;   // [M][ldh] order-preserving dense integer ranks of the risk scores (higher = higher risk), 1 <= M <= 8
    const int* trank;                   // [n] dense ranks of the survival times
    const int* event;                   // [n] 0 / 1
    const int* stratum;                 // [n] or NULL: pairs count only inside one stratum (out-of-fold predictions of different folds' models)
    int n;
    const signed char* w; int ldw; int R;  // [R][ldw] multiplicities 0..127; ldw % 64 == 0, bytes n..ldw-1 of every row zero
    long long* out;                     // [M+1][R], zeroed by the caller: row m < M: 2*concordant + tied of model m; row M: comparable pairs
    int pair_rule;                      // 0: e_i && t_j > t_i (mms_cindex_counts' rule); 1: lifelines' -- additionally e_i && !e_j && t_i == t_j
} CbootP;

/* Univariate Cox score screen (csrc/gene_screen.hip): the partial-likelihood score test of every gene at beta = 0, Breslow ties, on P
 * problems in one launch.  A problem p is the ordered list row[off[p] .. off[p+1]) of patient rows of x, TIME DESCENDING (a fold's
 * training patients or a bootstrap resample of them: a row may repeat, a repeat is a tie).  With S1_k the running sum of the list's
 * first k + 1 rows of gene j,   U[p][j] = sum_k a_k x_kj,   V[p][j] = sum_k b_k x_kj^2 - sum_k q_k S1_kj^2;   the statistic U^2 / V is
 * chi-square with one degree of freedom.  coef[k] = {a_k, b_k, q_k} depend on the labels only and are computed by the host in fp64
 * (gene_select.score_coefficients): b_k = sum over the event times u <= t_k of d_u / n_u, a_k = e_k - b_k, q_k = d_u / n_u^2 at the
 * last position of event time u's tie group and 0 elsewhere (d_u events at u, n_u rows with t >= u).
 * fp64 accumulation, no atomics, plain stores; a problem's bits do not depend on the other problems of the launch.  P = 0 and empty
 * problems are valid (U = V = 0).  The launch cannot read row / off: the CALLER guarantees 0 <= row < N and off non-decreasing from 0
 * (ops.gene_screen checks both on the host).  A NULL pointer, P < 0, G < 1, G > MMS_GENE_SCREEN_MAX_G, ld < G, N < 1 or a pointer not
 * aligned to its element: MMS_ERR_ARG before any launch. */
#define MMS_GENE_SCREEN_MAX_G 4194240  /* 65535 strips of 64 genes (grid y) */
typedef struct GeneScreenP {
    const float* x; int N; int ld;      // [N][ld] fp32 (device), the first G columns are screened
    int G; int P;
    const int* off;                     // [P+1] problem p = positions off[p] .. off[p+1]-1 of row / coef
    const int* row;                     // [off[P]] patient rows in risk order
    const double* coef;                 // [off[P]][3] a, b, q
    double* U; double* V;               // [P][G] out (every element written)
} GeneScreenP;

/* Elastic-net Cox regression ("Coxnet"), P problems in lock-step (csrc/coxnet.hip).  All problems share ONE list of patient rows of x in
 * stable time-descending order (row, with an event flag per position and a flag at the last position of every group of equal times) and
 * differ in their integer multiplicities mult[p] over that list (0 = not in this fit, > 1 = a bootstrap repeat, i.e. a tie), in lam, alpha
 * and the optional per-gene scale, given as its reciprocal (the fit then runs on x_j inv_scale_j).  With n = sum m, eta = x beta, S0_u = sum_{t_k >= u} m_k exp(eta_k)
 * and d_u = sum m_k e_k over the tie group of u, the objective is
 *     F(beta) = (1/n) [ -sum_k m_k e_k eta_k + sum_u d_u log S0_u ] + lam ( alpha |beta|_1 + (1 - alpha)/2 |beta|^2 )
 * (Breslow ties), computed after subtracting the problem's maximum eta over its rows with m > 0.  Residual r_k = m_k e_k -
 * m_k exp(eta_k) c_k, c_k = sum_{u <= t_k} d_u / S0_u; a row with m = 0 has r = 0 exactly (a select).  The smooth part's gradient is
 * -x'r / n + lam (1 - alpha) beta; a problem without rows or events has loss 0.
 * mms_coxnet_eval: one evaluation at `beta` -> E (eta), R (r), loss (the bracket above, NOT divided by n), nsum (n), grad, f (the smooth
 *   part), kkt and obj (F); the solver's state (trial, step, iters, status, counter) is not touched.
 * mms_coxnet_iterate: `iters` rounds of monotone proximal gradient with a step per problem: trial = soft(beta - s g, s lam alpha) is
 *   accepted iff f(trial) <= f + <g, D> + |D|^2 / (2 s) + 1e-12 max(1, |f|), then s *= 1.25, else s /= 2 and (beta, g) stay.  A problem
 *   whose KKT residual (max_j |g_j + lam alpha sign beta_j| where beta_j != 0, max(|g_j| - lam alpha, 0) elsewhere) at the kept point is
 *   <= tol gets status 1 and is frozen; one that has counted max_iter iterations gets status 2; both decrement *counter (integer atomic).
 *   A NEW problem has status -1, its start in `trial`, step = 1, iters = 0 and *counter counts it: its first round evaluates the start,
 *   keeps it without a test (status -> 0, or 1 if it is already optimal) and counts no iteration.
 * fp64 throughout, both products on v_mfma_f64_16x16x4_f64, no float atomics, no waits inside a launch; a problem's bits do not depend on
 * P or on its place among the problems.  The launch cannot check row / mult / lam / alpha / scale: the CALLER guarantees 0 <= row < N,
 * mult >= 0, lam >= 0, 0 <= alpha <= 1, inv_scale > 0 (ops.coxnet_* check on the host).  A NULL pointer (inv_scale alone may be NULL), P < 0,
 * G < 1, ld < G, N < 1, nrow < 0, P > 16 * 65535, a pointer not aligned to its element, tol outside (0, MMS_COXNET_MAX_TOL], max_iter
 * outside [1, MMS_COXNET_MAX_ITER] or iters < 0: MMS_ERR_ARG before any launch.  P = 0, nrow = 0 or iters = 0: MMS_OK without a launch. */
#define MMS_COXNET_MAX_TOL 1.0
#define MMS_COXNET_MAX_ITER 100000000
typedef struct CoxnetP {
    const float* x; int N; int ld; int G;      // [N][ld] fp32 (device), the first G columns are used
    int nrow;                                  // positions of the row list
    const int* row; const int* event; const int* glast;   // [nrow] patient row, event flag, 1 at the last position of a tie group
    int P;
    const int* mult;                           // [P][nrow] multiplicities
    const double* lam; const double* alpha;    // [P]
    const double* inv_scale;                   // [P][G] or NULL (all 1): 1 / the per-gene scale
    double* beta; double* trial; double* grad; // [P][G] kept point, trial point, the smooth part's gradient at the kept point
    double* f; double* step;                   // [P] smooth objective at the kept point, step
    int* iters; int* status;                   // [P] iterations counted; -1 new, 0 running, 1 converged, 2 max_iter reached
    double* loss; double* nsum; double* kkt; double* obj;   // [P] out
    double* E; double* R;                      // [P][nrow] eta and residual of the last evaluated point
    double* Gr;                                // [P][G] workspace: the raw product x'r
    int* counter;                              // [1] unfinished problems
    double tol; int max_iter;
} CoxnetP;

/* Cut-point scan of the two-group log-rank statistic (csrc/logrank_scan.hip): the statistic of EVERY admissible cut of Q problems in one
 * launch -- the maximally selected log-rank statistic of M models and of R relabellings of each (risk_strata.stratify).
 * The n patients stand in TIME-DESCENDING order (any order inside a group of equal times); the labels are shared by all problems.  A
 * problem q is the int32 rank vector rank[q][0..n) over those positions (a model's dense risk ranks, or a permutation of them) and a
 * cut set s = cset[q] (q itself when cset is NULL): the ascending cut ranks cut[coff[s] .. coff[s+1]).  Position i is in the HIGH group
 * of cut c iff rank[q][i] >= cut[c].  With d_u events and n_u positions at risk (t >= u) at event time u, G_i = the high-group members
 * among positions 0..i and D the high group's events,
 *     U = D - sum_i h_i G_i   (= sum_i [high_i] a_i with a_i = e_i - sum_{u <= t_i} d_u / n_u: observed - expected events),
 *     V = sum_i c_i G_i (i + 1 - G_i)   (the hypergeometric variance of survival_stats.logrank_test),   chi2 = U^2 / V, 0 when V <= 0,
 * coef[i] = {h_i, c_i}: h_i = d_u / n_u and c_i = d_u (n_u - d_u) / (n_u^2 (n_u - 1)) (c_i: when n_u >= 2, else 0) at the LAST position
 * of event time u's tie group (where i + 1 = n_u), both 0 elsewhere; pflag[i] = [e_i] | 2 [coef[i] != {0, 0}].  The host computes both
 * in fp64 (risk_strata.logrank_coefficients).  A time with n_u = 1 -- skipped by logrank_test -- adds 1 - 1 = 0 to U and nothing to V.
 * Out, per problem: chi2_max = the largest chi2 over its cuts, arg_max = its cut index (the smallest on ties; a problem without cuts:
 * 0 and -1), chi2_at = chi2 at cut index at[s] (0 when at is NULL or the index is outside the set).  U / V / n_high / d_high: optional
 * full tables [Q][ldo], all four or none; n_high and d_high are the exact size and events of the high group.
 * fp64 arithmetic, no atomics, plain stores; a problem's bits depend on its own rank vector and cut list only, not on Q, on its place
 * in the launch or on whether the tables are asked for (a replicate with the identity permutation reproduces the observed chi2_max
 * bit for bit).  Q = 0 and empty cut sets are valid; an event-free cohort gives zeros.  The launch cannot check that coff is
 * non-decreasing from 0, that every cut list is ascending, that cset lies in [0, S), that maxc bounds every set or that pflag matches
 * coef: the CALLER guarantees them (ops.logrank_scan checks on the host).  A NULL required pointer (cset, at and the tables may be
 * NULL), n < 1, n > MMS_LRSCAN_MAX_N, ldr < n, Q < 0, Q > MMS_LRSCAN_MAX_Q, maxc < 0, maxc > MMS_LRSCAN_MAX_C, some but not all of
 * the tables, ldo < maxc with tables, or a pointer not aligned to its element (coef: to its 16-byte pair): MMS_ERR_ARG before any
 * launch. */
#define MMS_LRSCAN_MAX_N 65535     /* a thread counts the high group and its events in the two 16-bit halves of one register */
#define MMS_LRSCAN_MAX_C 65535     /* cuts lie between distinct ranks of at most MAX_N patients: never more than n - 1 are distinct */
#define MMS_LRSCAN_MAX_Q 16777215  /* one workgroup of 256 threads per problem: the launch's thread count stays below 2^32 */
typedef struct LogrankScanP {
    int n; int ldr; int Q;              // positions, row pitch of rank, problems
    int maxc;                           // the largest cut set's size (bounds ldo)
    const int* rank;                    // [Q][ldr] ranks over the shared time-descending positions
    const int* pflag;                   // [n] bit 0: event, bit 1: coef[i] is not {0, 0}
    const double* coef;                 // [n][2] h, c
    const int* coff;                    // [S+1] cut set s = cut[coff[s] .. coff[s+1])
    const int* cut;                     // [coff[S]] ascending inside a set
    const int* cset;                    // [Q] the problem's cut set, or NULL: set q
    const int* at;                      // [S] the designated cut index of a set (the median split), or NULL
    double* chi2_max; int* arg_max; double* chi2_at;    // [Q] out
    double* U; double* V;               // [Q][ldo] out or NULL
    int* n_high; int* d_high;           // [Q][ldo] out or NULL
    int ldo;
} LogrankScanP;

/* Absolute-risk metrics under bootstrap multiplicities (csrc/td_metrics.hip): the IPCW Brier score and the cumulative/dynamic AUC
 * numerator of M models at H horizons for R multiplicity rows in one launch (absolute_risk.prediction_error).
 * The n patients stand in TIME-ASCENDING order, at equal times events before censorings; the labels are shared by all replicates:
 * trank = dense ranks of the times (equal times share a rank), event = 0 / 1, hcut[h] = the number of positions with t <= tau_h
 * (non-decreasing; always the end of a group of equal times).  rord[m][k] = 2 * position + [k is the last of its group of equal risk
 * scores], the positions of model m in RISK-ASCENDING order.  surv[m][i][h] = model m's predicted S(tau_h) of position i.
 * A replicate r is the multiplicity row w[r][0..n) (0..127; W = sum w).  Over the distinct times u ascending, with S_a = sum of w at
 * t >= u, d_u = the w of the events at u, n_u = S_a - d_u and S_b = the w at t > u (all exact integers),
 *     G(t)  = prod_{u <= t, n_u > 0} S_b / n_u      (reverse Kaplan-Meier: the censoring distribution; G(t-) the product over u < t),
 *     KM(t) = prod_{u <= t, S_a > 0} n_u / S_a      (the replicate's own Kaplan-Meier estimate),
 * every factor ONE fp64 division of two integers, multiplied in ascending time order.  At horizon h a position i is a case iff
 * i < hcut[h] and e_i, a control iff i >= hcut[h]; a case weighs w_i / G(t_i-).  Out, [R][H]: G = G(tau_h), km = KM(tau_h), wcase = the
 * cases' weight, wctrl = the controls' sum of w (an exact integer); [R][M][H]:
 *     brier   = ( sum_cases w_i / G(t_i-) S_i^2 + [wctrl > 0] sum_controls w_i (1 - S_i)^2 / G(tau_h) ) / W,
 *     auc_num = sum over case i, control j of (w_i / G(t_i-)) w_j ([eta_i > eta_j] + 1/2 [eta_i = eta_j])
 * (the AUC is auc_num / (wcase wctrl); the host forms it, the null model's Brier score from km, and the integrals).
 * fp64 accumulation, no atomics, plain stores; one workgroup per replicate: a replicate's bits depend on its own row and the shared
 * inputs only, not on R, on its place in the launch or on M (G / km / wcase / wctrl) or the other models (brier / auc_num).
 * R = 0 is valid and launches nothing.  The launch cannot check the tables' contents: the CALLER guarantees the order and the tie
 * rule of the positions, dense trank, hcut as above, every rord row a permutation with consistent group flags, finite surv, w >= 0 and
 * W >= 1 in every row (ops.td_metrics checks on the host).  A position of rord outside [0, n) is clamped: it cannot reach memory
 * outside the arguments.  A NULL pointer, n < 1, n > MMS_TD_MAX_N, H < 1, H > MMS_TD_MAX_H, M < 1, M > MMS_TD_MAX_M, R < 0,
 * R > MMS_TD_MAX_R, ldr < n, ldh < H, ldw < n or a pointer not aligned to its element: MMS_ERR_ARG before any launch. */
#define MMS_TD_MAX_H 64            /* lane = horizon: one wave */
#define MMS_TD_MAX_M 64
#define MMS_TD_MAX_N 4096          /* 12 bytes of LDS a position */
#define MMS_TD_MAX_R 16777215      /* one workgroup of 256 threads per replicate: the launch's thread count stays below 2^32 */
typedef struct TdMetricsP {
    int n; int H; int M; int R;         // positions, horizons, models, replicates
    const int* trank; const int* event; // [n] dense time ranks and event flags of the time-ascending positions
    const int* hcut;                    // [H] positions with t <= tau_h
    const int* rord; int ldr;           // [M][ldr] 2 * position + [last of its risk tie group], risk ascending
    const double* surv; int ldh;        // [M][n][ldh] predicted survival at the horizons, position-major
    const signed char* w; int ldw;      // [R][ldw] multiplicities 0..127
    double* G; double* km;              // [R][H] out
    double* wcase; double* wctrl;       // [R][H] out
    double* brier; double* auc_num;     // [R][M][H] out
} TdMetricsP;

/* Multivariable Cox regression by Newton-Raphson (csrc/cox_newton.hip): Q = R * S low-dimensional fits in one launch -- every bootstrap
 * replicate of every nested covariate subset of one analysis (multivariable.analyse).
 * The n patients stand in TIME-DESCENDING order (any order inside a group of equal times) with event[n] = 0 / 1 and glast[n] = 1 at the
 * last position of a group of equal times (CoxnetP's convention); x[n][ldx] is the fp64 covariate table, position-major, of which the
 * first p columns are used.  All of this is shared.  Problem q = r * S + s has the multiplicity row w[r][0..n) (0..127, a multiplicity
 * is a repeat) and the column set cmask[s] (bit a: column a is in the model); coefficients outside the mask stay exactly 0 and their se
 * is NaN.  Breslow ties.  With eta_k = sum_{a in A} x_ka beta_a shifted by its maximum over the rows with w > 0, r_k = w_k exp(eta_k)
 * and the running sums S0 = sum r, S1 = sum r x, S2 = sum r x x' over the positions so far, every tie-group end with
 * d = sum w_k e_k > 0 over the group adds
 *     l += sum w e eta - d log S0,    g += sum w e x - d S1 / S0,    I += d (S2 / S0 - S1 S1' / S0^2).
 * Solver, per problem:  (1) beta = 0, evaluate, loglik0 = l.  sum w e = 0: status 6 (beta = 0, loglik = 0).  (2) Every round factors
 * I = L L' on the mask's columns; a pivot (the diagonal entry less the squares left of it) that is not > 1e-10 * the largest diagonal
 * entry of I: status 3 (singular).  (3) delta = I^-1 g; max |delta| <= tol: status 1 (converged), beta is kept and
 * se = sqrt(diag(I^-1)) from this factor.  (4) Else the first s = 1, 1/2, ..., 2^-20 with l(beta + s delta) >= l - 1e-12 max(1, |l|)
 * is accepted (anything else, NaN included, is not); none: status 5.  (5) An accepted step counts one iteration; then
 * max |beta| > beta_max: status 4 (monotone likelihood), else iters = max_iter: status 2.  Every status leaves a finite beta, the
 * loglik of that beta and iters; se is NaN unless the status is 1.  An empty mask is the null model (status 1 after 0 iterations).
 * Out: beta, se [Q][p], loglik, loglik0 [Q], iters, status [Q] and, unless NULL, info [Q][p][p] = the full symmetric information at the
 * kept beta (zero outside the mask).
 * fp64 throughout, no atomics, no waits, plain stores; one workgroup per problem: a problem's bits depend on its own row, its own mask
 * and the shared inputs only, not on Q, on its place in the launch or on whether info is asked for.  Bits of a mask at or above p are
 * ignored by the launch.  The launch cannot check the tables' contents: the CALLER guarantees the order of the positions, glast
 * consistent with it (glast[n - 1] = 1), finite x, w >= 0 and valid, non-empty masks (ops.cox_newton checks on the host).  A NULL
 * required pointer (info alone may be NULL), n < 1, n > MMS_COXNEWTON_MAX_N, p < 1, p > MMS_COXNEWTON_MAX_P, ldx < p, ldw < n, R < 0,
 * S < 0, S > MMS_COXNEWTON_MAX_S, R * S > MMS_COXNEWTON_MAX_Q, tol outside (0, MMS_COXNEWTON_MAX_TOL], max_iter outside
 * [1, MMS_COXNEWTON_MAX_ITER], beta_max not > 0 or a pointer not aligned to its element: MMS_ERR_ARG before any launch.  R = 0 or
 * S = 0: MMS_OK without a launch. */
#define MMS_COXNEWTON_MAX_P 16       /* 136 (a <= b) pairs: three waves of lanes */
#define MMS_COXNEWTON_MAX_N 4096     /* 20 bytes of LDS a position */
#define MMS_COXNEWTON_MAX_S 64
#define MMS_COXNEWTON_MAX_Q 16777215 /* one workgroup of 256 threads per problem: the launch's thread count stays below 2^32 */
#define MMS_COXNEWTON_MAX_TOL 1e-3
#define MMS_COXNEWTON_MAX_ITER 1000
typedef struct CoxNewtonP {
    int n; int p; int R; int S;         // positions, covariate columns, replicates, subsets
    const double* x; int ldx;           // [n][ldx] covariates of the time-descending positions
    const int* event; const int* glast; // [n] event flag; 1 at the last position of a group of equal times
    const signed char* w; int ldw;      // [R][ldw] multiplicities 0..127
    const int* cmask;                   // [S] bit a: column a is in the model
    double tol; int max_iter; double beta_max;
    double* beta; double* se;           // [R * S][p] out
    double* loglik; double* loglik0;    // [R * S] out
    int* iters; int* status;            // [R * S] out
    double* info;                       // [R * S][p][p] out, or NULL
} CoxNewtonP;

/* Random survival forest (csrc/rsf.hip; survival_forest.py): T trees grown level by level in lock-step over ONE feature-major matrix.
 * The n patients stand in TIME-DESCENDING order (any order inside a group of equal times): event[i] = 0 / 1, tgroup[i] = the number of
 * position i's group of equal times (equal inside a group, different between neighbouring groups).  xt[f][i] is feature f of position
 * i.  A tree t is its multiplicity row mult[t][0..n) (0 = out of bag; a repeat counts as a separate subject) and its hash stream
 * id = tree_id[t] (t when tree_id is NULL).  Trees are heap-indexed: node s has the children 2s + 1 and 2s + 2; the tables have nn
 * nodes a tree.  node[t][i] is the current node of in-bag position i (all 0 before level 0).
 *
 * mms_rsf_split, one launch per level: workgroup = (tree, node s = 2^level - 1 + k).  It returns at once when s > 0 and its parent
 * recorded no split, or when n_node[s] < 2 min_leaf (s > 0: the parent's launch wrote it).  Otherwise the node's m in-bag members are
 * compacted in position order and C = mtry * nsplit candidates c = j * nsplit + q are scored.  With hash = csrc/common.h's hash_u32 and
 * mulhi(h, k) = (h * k) >> 32 in 64 bits:
 *     ht = hash(seed ^ (id * 0x85ebca6b));  hn = hash((s + 1) * 0x9E3779B9 + ht);  hf = hash((j + 1) * 0x9E3779B9 + hn);
 *     feature f = mulhi(hf, p);   hq = hash((q + 1) * 0x85ebca6b + hf);   threshold = xt[f][position of member mulhi(hq, m)],
 * all in 32-bit wrap-around arithmetic.  A member goes LEFT iff x <= threshold.  Over the node's tie groups with events, in time-
 * descending order, with Y = the node's weighted members up to the group's end, d = the group's weighted events and Y_L the left
 * child's weighted members up to there,
 *     E <- fma(d / Y, Y_L, E),   V <- fma((d (Y - d) / (Y Y (Y - 1))) Y_L, Y - Y_L, V)   (the second coefficient 0 when Y = 1),
 *     U = D_L - E  (D_L: the left child's weighted events),   chi2 = U U / V, 0 when V <= 0:
 * the two-group log-rank statistic of survival_stats.logrank_test with every patient repeated mult times.  Counts are exact integers,
 * the terms fp64.  A candidate is admissible when both children hold >= min_leaf weighted members; the largest chi2 > 0 among the
 * admissible ones wins, the smallest c on ties: feat[s] = f, thr[s], stat[s] = chi2, n_node / d_node of both children are written and
 * the node's members are routed (node[t][i] = 2s + 1 + [x > thr]) by the same workgroup.  Without a winner feat[s] = -1 (a leaf).
 * Level 0 also writes n_node[0] / d_node[0].  The caller initialises feat = -1 and the other tables = 0.  U / V / n_left / d_left:
 * optional tables [T][2^level][ldo] of every candidate, all four or none (a workgroup that returns at once writes nothing).
 *
 * mms_rsf_leaves, one launch after the last level: for every node with feat < 0 and n_node > 0 the Nelson-Aalen increments d / Y of its
 * members' tie groups with events, in time-descending order, give mort = sum (d / Y) weight[w][i] (w = wset[t], 0 when wset is NULL; i
 * a position of the group; weight[w][i] = the number of distinct event times of training set w that are >= time i, which makes mort
 * the sum of H over those times) and H[h] = sum of d / Y over the groups at positions >= hpos[h] (hpos[h] = the number of positions
 * with time > horizon h).
 *
 * mms_rsf_predict, one launch: workgroup = row of x [R][ldx]; it drops the row down every tree t with use[t][row] != 0 (all when use is
 * NULL), thread j summing trees j, j + 256, ... in ascending order and the 256 partial sums folded in a fixed order:
 * out_mort[row], out_H[row][h] = the means over the admitted trees, NaN when count[row] = 0.
 *
 * fp64 statistics, no atomics, plain stores; a tree's bits depend on its own multiplicities and hash stream only.  The launches cannot
 * check the tables' contents: the CALLER guarantees the order of the positions, tgroup, feat < p and node values (ops.rsf_* check on
 * the host).  A NULL required pointer, n outside 1..MMS_RSF_MAX_N, ld < n, p < 1, T < 0, T > MMS_RSF_MAX_T, level outside
 * [0, MMS_RSF_MAX_DEPTH), nn < 2^(level + 2) - 1 (split) or nn outside 1..2^(MMS_RSF_MAX_DEPTH + 1) - 1, mtry < 1, nsplit < 1,
 * mtry * nsplit > MMS_RSF_MAX_C, min_leaf < 1, some but not all of the tables, ldo < C with tables, nh outside 0..MMS_RSF_MAX_H, F < 1,
 * R < 0, ldx < p, ldu < R with use, or a pointer not aligned to its element: MMS_ERR_ARG before any launch.  T = 0 (R = 0 for
 * predict): MMS_OK without a launch. */
#define MMS_RSF_MAX_N 2048       /* 28 bytes of LDS a member: 56 KB of the 64 KB a workgroup may declare */
#define MMS_RSF_MAX_DEPTH 12
#define MMS_RSF_MAX_C 65535
#define MMS_RSF_MAX_T 65535      /* T * 2^11 workgroups at the deepest level stay below 2^31 */
#define MMS_RSF_MAX_H 32
typedef struct RsfSplitP {
    int n; int ld; int p; int T;        // positions, pitch of xt / mult / node, features, trees
    int level; int nn;                  // the level of this launch, nodes a tree in the tables
    int mtry; int nsplit; int min_leaf; unsigned seed;
    const float* xt;                    // [p][ld]
    const unsigned char* mult;          // [T][ld]
    const int* event; const int* tgroup;   // [n]
    const int* tree_id;                 // [T] hash stream of each tree, or NULL: t
    int* node;                          // [T][ld] in / out
    int* feat; float* thr; double* stat; int* n_node; int* d_node;   // [T][nn]
    double* U; double* V;               // [T][2^level][ldo] out or NULL
    int* n_left; int* d_left;           // [T][2^level][ldo] out or NULL
    int ldo;
} RsfSplitP;
typedef struct RsfLeavesP {
    int n; int ld; int T; int nn; int nh; int F;   // F: weight rows
    const unsigned char* mult;          // [T][ld]
    const int* event; const int* tgroup;   // [n]
    const int* node;                    // [T][ld]
    const int* feat; const int* n_node; // [T][nn]
    const double* weight;               // [F][ld]
    const int* wset;                    // [T] weight row of each tree, or NULL: row 0
    const int* hpos;                    // [nh]
    double* mort;                       // [T][nn] out
    double* H;                          // [T][nn][nh] out
} RsfLeavesP;
typedef struct RsfPredictP {
    int R; int ldx; int p; int T; int nn; int nh;
    const float* x;                     // [R][ldx]
    const int* feat; const float* thr;  // [T][nn]
    const double* mort; const double* H;   // [T][nn], [T][nn][nh]
    const unsigned char* use; int ldu;  // [T][ldu] or NULL
    double* out_mort; double* out_H;    // [R], [R][nh] out
    int* count;                         // [R] out: admitted trees
} RsfPredictP;

/* Permutation importance (ensemble VIMP, randomForestSRC importance = "permute") of a forest, mms_rsf_vimp: P problems (set f, gene g)
 * times R repeats in ONE launch, workgroup = (problem q, repeat r), output index q R + r.
 *
 * A set f is some of the trees (a fold's) with the rows they admit: use[t][i] != 0 (the out-of-bag mask, or a validation mask), the
 * base ensemble mortality M0[f][i] and tree count cnt[f][i] -- exactly what mms_rsf_predict returns for that mask over the set's trees.
 * Rows with cnt = 0 are not part of the set's problems.  Rows are rows of x [n][ldx] as mms_rsf_predict takes it (NOT time positions).
 *
 * donor[r][t][i]: the row whose value of the problem's gene row i reads in tree t under repeat r.  The contract of the table
 * (survival_forest.permutation_donors builds it; tests/rsf_vimp_ref.py restates it), all in 32-bit wrap-around arithmetic with
 * hash = csrc/common.h's hash_u32 and ht = hash(seed ^ (id * 0x85ebca6b)) the tree key of RsfSplitP:
 *     hp = hash((r + 1) * 0x85EBCA6B + hash(ht ^ 0x68E31DA4));    k_i = hash((i + 1) * 0x9E3779B9 + hp);
 *     a_0 < a_1 < ... the rows tree t admits, s_0, s_1, ... the same rows sorted by (k, i) ascending:  donor[a_j] = s_j,
 * and a row the tree does not admit is its own donor.  One permutation per (tree, repeat) serves every gene.
 *
 * Problem q = (pset[q], pgene[q]) lists the trees of its set that split on its gene at any node, ascending and without repeats:
 * ptree[poff[q] .. poff[q + 1]).  For row i with cnt > 0, over those trees in that order that admit i, sequentially in fp64 from 0.0,
 *     D_i += mort_t(leaf') - mort_t(leaf),
 * leaf = the leaf of mms_rsf_predict's walk (stop: feat < 0 || 2 s + 2 >= nn), leaf' = the same walk reading x[donor[r][t][i]][g] in
 * place of x[i][g] at EVERY node on g (a gene met twice on one path reads the substituted value both times).  Then
 *     M_i = M0[f][i] + D_i / cnt[f][i]
 * (IEEE fp64: one subtraction and one addition per tree, one division and one addition per row), and over the rows with cnt > 0 the
 * pair counts of survival_stats.concordance_index(time, -M, event): the ordered pair (i, j) is comparable when i is an event and either
 * tgroup[i] > tgroup[j] or tgroup[i] = tgroup[j] and j is censored -- tgroup[i] is the number of row i's group of equal times counted
 * from the LATEST time (risk_sets.descending_groups' gid per row: a LARGER number is a SHORTER time), in 0 .. n - 1;
 *     comparable[q R + r] = the comparable pairs,   conc2[q R + r] = sum over them of 2 [M_i > M_j] + [M_i = M_j],
 * exact integers, so C = conc2 / (2 comparable).  A problem with an empty tree list counts M0 itself (the base C-index).  Optional
 * outputs D and M [P R][ld]: D_i and M_i of every row (0.0 and M0 where cnt = 0).  No atomics; a problem's outputs do not depend on
 * what shares its launch.  The launch cannot check table contents: the CALLER guarantees feat < p, genes in 0 .. p - 1, donors in
 * 0 .. n - 1, trees in 0 .. T - 1, sets in 0 .. F - 1, tgroup in 0 .. n - 1, poff non-decreasing from 0 (ops.rsf_vimp checks on the
 * host).  A NULL required pointer, n outside 1..MMS_RSF_MAX_N, ldu < n, ld < n, p < 1, ldx < p, T outside 0..MMS_RSF_MAX_T, nn outside
 * 1..2^(MMS_RSF_MAX_DEPTH + 1) - 1, F < 1, R outside 1..MMS_RSF_VIMP_MAX_R, P < 0, P R >= 2^31 or a pointer not aligned to its element:
 * MMS_ERR_ARG before any launch.  P = 0 or T = 0: MMS_OK without a launch. */
#define MMS_RSF_VIMP_MAX_R 64
typedef struct RsfVimpP {
    int n; int ldx; int p; int T; int nn; int F; int R; int P;
    int ldu; int ld;                    // pitch of use / donor rows; pitch of M0 / cnt / D / M rows
    const float* x;                     // [n][ldx]
    const int* feat; const float* thr; const double* mort;   // [T][nn]
    const unsigned char* use;           // [T][ldu]
    const int* donor;                   // [R][T][ldu]
    const double* M0; const int* cnt;   // [F][ld]
    const int* event; const int* tgroup;   // [n] per row of x
    const int* pset; const int* pgene;  // [P]
    const int* poff; const int* ptree;  // [P + 1], [poff[P]]
    long long* conc2; long long* comparable;   // [P * R] out
    double* D; double* M;               // [P * R][ld] out, or NULL
} RsfVimpP;

/* Gene-set enrichment with a label-permutation null (multimodal_survival_prediction_amd/enrichment.py), two entry points.
 *
 * mms_gsea_scores: at beta = 0 the Cox score of gene g is linear in the null martingale residuals m (Breslow ties; sum m = 0), and
 * relabelling the patients permutes m.  With the n analysed patients row[0 .. n) in list order and replicate r giving list position i
 * the residual m[perm[r][i]] (row 0 of perm is the identity by convention of the caller),
 *     Z[r][g] = scale[g] * sum_i m[perm[r][i]] x[row[i]][g],
 *     scale[g] = 1 / sqrt( (sum m^2 / (n - 1)) * sum_i (x[row[i]][g] - mean_g)^2 ),
 * the exact permutation variance of the sum; scale[g] = 0 (and Z[r][g] = +0.0 in every replicate) when the centred sum of squares or
 * sum m^2 is 0.  Two launches.  Column pass: one thread per gene walks the rows in list order in fp64, the mean first, then the centred
 * squares (and sum m^2 in the same order), so scale[g] depends on column g's values, row and m only.  Product: v_mfma_f64_16x16x4_f64,
 * replicates on M, genes on N, list positions on K in a fixed order that depends on n only; no atomics, every Z[r][g] is owned by one
 * lane, and the bits of replicate r do not depend on R1 or on r's place in the launch.  The launch cannot check table contents: the
 * CALLER guarantees rows in [0, N) and every perm row inside [0, n) (ops.gsea_scores checks on the host).  A NULL pointer, n < 2, N < 1,
 * G outside 1..MMS_GSEA_MAX_G, ld < G, ldz < G, R1 outside 0..MMS_GSEA_MAX_R1 or a pointer not aligned to its element: MMS_ERR_ARG
 * before any launch.  R1 = 0: MMS_OK without a launch.
 *
 * mms_gsea_es: the enrichment score (Subramanian et al. 2005) of S gene sets (CSR: set s = set_gene[set_off[s] .. set_off[s + 1]),
 * distinct genes, 1 <= k <= G - 1) in R1 replicates.  Replicate r ranks the keys z[g] = Z[r][g] -- or, with gperm (preranked mode: Z has
 * ONE row), z[g] = Z[0][g] for r = 0 and Z[0][gperm[r - 1][g]] for r >= 1 -- by z descending, the lower g first on equal values (-0.0
 * equals +0.0; the keys must be finite).  With w_g = |z_g| (weight 1) or 1 (weight 0; also taken for a set whose weights add up to 0)
 * and NR their sum over the set, walking the ranking a member adds w_g / NR and a non-member subtracts 1 / (G - k); hi / lo are the
 * largest / smallest value after a position; es = hi if hi >= -lo, else lo; peak = the first (0-based) position that attains it.  The value
 * after a position is (hit weights so far) / NR - (misses so far) / (G - k), two true divisions; with unit weights it is the single
 * division (hits (G - k) - misses k) / (k (G - k)) of an exact integer, so equal fractions are equal bits and real ties go to the first
 * position.  One workgroup per replicate: the keys are sorted in LDS by a bitonic network over the next power of two (padding keys last), and each
 * of the workgroup's waves then takes every fourth set: it flags the set's ranks in a byte strip of its own and walks the positions 64
 * at a time with wave prefix sums (a chunk without a member in closed form).  fp64, no atomics, plain stores: every (replicate, set)
 * is owned by one wave and does not depend on what shares the launch.  The launch cannot check table contents: the CALLER guarantees
 * the CSR contract and that every gperm row is a permutation of 0 .. G - 1 (ops.gsea_es checks on the host).  A NULL required pointer,
 * G outside 2..MMS_GSEA_MAX_G, S < 0, R1 outside 0..MMS_GSEA_MAX_R1, weight outside {0, 1}, ldz < G, lde < S or a pointer not aligned to
 * its element: MMS_ERR_ARG before any launch.  R1 = 0 or S = 0: MMS_OK without a launch. */
#define MMS_GSEA_MAX_G 8192         /* 16 bytes of LDS a gene (key 8, order 2, rank 2, 4 one-byte flag strips): 128 KB of the 160 KB a workgroup may declare on gfx950 */
#define MMS_GSEA_MAX_R1 4194240     /* 65535 tiles of 64 replicates (grid y of the product) */
typedef struct GseaScoreP {
    int n; int N; int ld; int G; int R1; int ldz;   // list length; rows and row pitch of x; genes; replicates; row pitch of Z
    const float* x;                     // [N][ld]
    const int* row;                     // [n]
    const double* m;                    // [n]
    const int* perm;                    // [R1][n]
    double* scale;                      // [G] out
    double* Z;                          // [R1][ldz] out
} GseaScoreP;
typedef struct GseaEsP {
    int G; int S; int R1; int weight; int ldz; int lde;   // genes; sets; replicates; 0 / 1; row pitch of Z; row pitch of es and peak
    const double* Z;                    // [R1][ldz], or [1][ldz] with gperm
    const int* gperm;                   // [R1 - 1][G], or NULL
    const int* set_off; const int* set_gene;   // [S + 1], [set_off[S]]
    double* es;                         // [R1][lde] out
    int* peak;                          // [R1][lde] out, or NULL
} GseaEsP;

/* Gradient-boosted trees on the Cox partial likelihood (csrc/gbm.hip; boosting.py): P problems advanced in lock-step, M rounds of one
 * tree each, over ONE binned feature-major matrix.  The n patients stand in TIME-DESCENDING order as for the forest above: event[i],
 * tgroup[i] (a larger number is a shorter time), rowid[i] = the row of the caller's matrix that stands at position i.  xb[f][i] in
 * 0 .. B - 1 is the bin of feature f at position i: bin = the number of edges[f][0 .. B - 1) that are < x (searchsorted, side "left";
 * the edges ascending, label-free quantiles, duplicates allowed).  The cut (f, b), b in 0 .. B - 2, sends bin <= b LEFT, which is
 * x <= edges[f][b] on raw values: thr = edges[f][b].
 *
 * A problem q is its multiplicity row mult[q][0..n) (0 = held out; a repeat counts as a separate subject), an optional evaluation mask
 * evalm[q][0..n), the scalars lr[q] (nu), depth[q] (D, 1 .. MMS_GBM_MAX_DEPTH), min_leaf[q] (weighted patients, >= 1), l2[q] (lambda
 * >= 0), min_gain[q] (gamma >= 0), the thresholds subsample[q] / colsample[q] (0xFFFFFFFF = always) and its hash stream pid[q] (q when
 * pid is NULL).  Everything a problem computes depends on its own row, scalars and id only, never on what shares its launches.  State
 * per problem: F[q][0..n) fp64 (0 before round 0; kept for ALL positions, held-out ones included), node[q][i] the current node of
 * position i in the round's tree, wt[q][i] = mult[q][i] where the position is in the round's sample, else 0.  Trees are heap-indexed
 * (children of s: 2s + 1, 2s + 2); the tables are [P][M][nn], nn >= 2^(max depth + 1) - 1, and the CALLER initialises feat = -1 and
 * every other table = 0.
 *
 * Hashes (hash = csrc/common.h's hash_u32, 32-bit wrap-around arithmetic):
 *     hk = hash(seed ^ (id * 0x85ebca6b));   hm = hash((m + 1) * 0x85ebca6b + hk)   for round m;
 *     position i is in the round's sample iff hash((rowid[i] + 1) * 0x9E3779B9 + hm) <= subsample;
 *     feature j is admitted in the round  iff hash((j + 1) * 0x9E3779B9 + (hm ^ 0xB5297A4D)) <= colsample.
 *
 * mms_gbm_grad, one launch per round (workgroup = problem): over the TRAINING positions (mult > 0; all of them, sampled or not), with
 * c = max F over them, e_i = exp(F_i - c), Breslow ties, fp64:
 *     S_k = sum of mult_j e_j over the positions up to the end of tie group k   (a forward scan: time descending),
 *     d_k = the weighted events of tie group k,   a_k = d_k / S_k,   b_k = a_k / S_k   (groups with d_k > 0),
 *     Lambda_i = sum of a_k, Q_i = sum of b_k over the groups from i's own to the last   (a backward scan),
 *     g_i = event_i - e_i Lambda_i,   h_i = e_i Lambda_i - (e_i e_i) Q_i,
 *     qg_i = llrint(clamp(g_i, -2^8, 1) * 2^32),   qh_i = llrint(clamp(h_i, 0, 2^8) * 2^32)      (int64; 0 where mult = 0),
 *     loglik[q][m] = sum over training events of mult_i (F_i - c) - sum_k d_k log S_k   (the log partial likelihood BEFORE round m's tree).
 * The scans run in a fixed order: wave scans over chunks of 256 positions, wave totals in order, the chunks' carry in order.  The launch
 * also writes wt, node = 0 and the root's n_node / G / H (weighted sums over the round's sample: G = sum wt_i qg_i, exact integers; with
 * mult <= 255 and n <= MMS_GBM_MAX_N every sum stays below 2^59).  last != 0: only loglik[q][m] is written (m = M is allowed then:
 * the likelihood after the last round; loglik is [P][M + 1]).
 *
 * mms_gbm_split, one call per level (two launches).  (1) grid = (tile of MMS_GBM_TILE features, problem): the workgroup returns at once
 * when level >= depth[q] or no node s = 2^level - 1 + k of the level is live (s = 0 or the parent split; n_node[s] >= 2 min_leaf).
 * Otherwise it builds, in LDS, the histograms {weighted count int32, sum wt qg int64, sum wt qh int64} per (feature of the tile, live
 * node, bin) over the sampled members -- as many features a pass as MMS_GBM_LDS_CELLS cells of 20 bytes hold -- prefixes them over the
 * bins and scores the B - 1 cuts of every admitted feature:
 *     admissible iff n_L >= min_leaf and n - n_L >= min_leaf;      term(G, H) = (G G) / (H + lambda), 0 when H + lambda <= 0;
 *     gain = term(G_L, H_L) + term(G_R, H_R) - term(G, H),   G_R = G - G_L, H_R = H - H_L in int64,
 * every int64 sum converted to fp64 (round to nearest) and scaled by 2^-32 first; squares and quotients only, so no fused multiply-add
 * can change a bit.  Its best cut per node (largest gain, then the smallest feature, then the smallest bin) goes to a partial table.
 * form: 0 = the default (MMS_GBM_FORM_MEMBERS), MMS_GBM_FORM_MEMBERS = lanes over members with integer LDS atomic adds,
 * MMS_GBM_FORM_PRIVATE = a lane per (feature, node) walking the members with a private LDS histogram; all sums are integers, so the
 * forms give identical bits.  (2) grid = problem: per live node the partials of the tiles in ascending order (a fixed-order argmax);
 * the winner splits iff gain > min_gain: feat / bin / thr / gain of s and n_node / G / H of both children are written; then every
 * position of a node that split moves to 2s + 1 + [xb > bin] (ALL positions: held-out and unsampled ones follow the tree too).
 * Optional trace tables t_n / t_G / t_H [P][2^level][p][B]: the prefixed (n_L, G_L, H_L) of every bin of every admitted feature of
 * every live node (all three or none; untouched elsewhere).  No float atomics, no global atomics, no workgroup waits for another.
 *
 * mms_gbm_update, one launch per round (workgroup = problem): value[s] = lr * (G / (H + lambda)) (fp64 as above; 0 when H + lambda
 * <= 0) for every leaf (s = 0 or the parent split, and feat[s] < 0), F_i += value[node_i] for ALL positions, and with evalm the pair
 * counts of survival_stats.concordance_index(time, -F, event) over the masked positions by mms_rsf_vimp's pair rule:
 * comparable[q][m], conc2[q][m] = 2 concordant + ties (int64, exact).
 *
 * mms_gbm_predict: thread = (problem, row of x [R][ldx] raw fp32): the row is dropped down the trees in round order (left iff
 * x[feat] <= thr), its sum running sequentially from 0.0, and out[q][k][row] = the sum after at[k] rounds (at ascending, 0 .. M):
 * on the training matrix that is F of the fit bit for bit.
 *
 * The launches cannot check table contents: the CALLER guarantees xb < B, tgroup, rowid, feat < p, node values and the order of the
 * positions (ops.gbm_* check on the host).  A NULL required pointer, n outside 1..MMS_GBM_MAX_N, ld < n, p < 1, P outside
 * 0..MMS_GBM_MAX_P, B outside 2..MMS_GBM_MAX_BINS, M < 1, round outside [0, M) ([0, M] with last), level outside [0,
 * MMS_GBM_MAX_DEPTH), nn < 2^(level + 2) - 1 (split) or nn outside 1..2^(MMS_GBM_MAX_DEPTH + 1) - 1, form outside 0..2, some but not
 * all of the trace tables, conc2 / comparable missing with evalm, R < 0, ldx < p, K < 1, or a pointer not aligned to its element:
 * MMS_ERR_ARG before any launch.  P = 0 (R = 0 for predict): MMS_OK without a launch. */
#define MMS_GBM_MAX_N 2048
#define MMS_GBM_MAX_P 65535
#define MMS_GBM_MAX_DEPTH 6
#define MMS_GBM_MAX_BINS 64
#define MMS_GBM_MAX_MULT 255        /* MAX_MULT * MAX_N * 2^8 * 2^32 < 2^59: every int64 sum of quantised gradients is exact */
#define MMS_GBM_QBITS 32
#define MMS_GBM_CLAMP_BITS 8
#define MMS_GBM_TILE 32             /* features a workgroup of mms_gbm_split */
#define MMS_GBM_LDS_CELLS 2880      /* histogram cells (20 bytes each, rows padded to B + 1) a pass: 57600 bytes of the 64 KB a workgroup may declare */
#define MMS_GBM_FORM_MEMBERS 1
#define MMS_GBM_FORM_PRIVATE 2
typedef struct GbmGradP {
    int n; int ld; int P; int round; int M; int nn; int last; unsigned seed;
    const unsigned char* mult;          // [P][ld]
    const int* event; const int* tgroup; const int* rowid;   // [n]
    const int* pid;                     // [P] hash stream of each problem, or NULL: q
    const unsigned* subsample;          // [P]
    const double* F;                    // [P][ld]
    long long* qg; long long* qh;       // [P][ld] out
    unsigned char* wt;                  // [P][ld] out
    int* node;                          // [P][ld] out
    double* loglik;                     // [P][M + 1]: element [q][round] out
    int* n_node; long long* G; long long* H;   // [P][M][nn]: the root of the round out
} GbmGradP;
typedef struct GbmSplitP {
    int n; int ld; int p; int P; int B; int level; int round; int M; int nn; int form; unsigned seed; int ntiles;
    const unsigned char* xb;            // [p][ld]
    const unsigned char* wt;            // [P][ld]
    const long long* qg; const long long* qh;   // [P][ld]
    const float* edges;                 // [p][B - 1]
    const int* depth; const int* min_leaf; const double* l2; const double* min_gain;   // [P]
    const unsigned* colsample; const int* pid;   // [P]; pid or NULL
    int* node;                          // [P][ld] in / out
    int* feat; int* bin; float* thr; double* gain; int* n_node; long long* G; long long* H;   // [P][M][nn]
    double* part_gain; int* part_cut; long long* part_sum;   // scratch [P][ntiles][2^level] x {1 double, 4 ints, 2 int64}; ntiles = ceil(p / MMS_GBM_TILE)
    int* t_n; long long* t_G; long long* t_H;   // [P][2^level][p][B] out, or NULL
} GbmSplitP;
typedef struct GbmUpdateP {
    int n; int ld; int P; int round; int M; int nn;
    const int* node;                    // [P][ld]
    const int* event; const int* tgroup;   // [n]
    const unsigned char* evalm;         // [P][ld] or NULL
    const double* lr; const double* l2; // [P]
    const int* feat; const long long* G; const long long* H;   // [P][M][nn]
    double* value;                      // [P][M][nn] out
    double* F;                          // [P][ld] in / out
    long long* conc2; long long* comparable;   // [P][M]: element [q][round] out; NULL without evalm
} GbmUpdateP;
typedef struct GbmPredictP {
    int R; int ldx; int p; int P; int M; int nn; int K; int pad_;
    const float* x;                     // [R][ldx]
    const int* feat; const float* thr; const double* value;   // [P][M][nn]
    const int* at;                      // [K] ascending round counts in 0 .. M
    double* out;                        // [P][K][R]
} GbmPredictP;

/* Path-dependent TreeSHAP (Lundberg et al. 2018/2020, Algorithm 2's value function) of heap-indexed tree tables: which features pushed
 * a row's prediction up or down, and by how much (csrc/tree_shap.hip; tree_shap.py, Booster.shap, Forest.shap; tests/tree_shap_ref.py
 * restates all of this in numpy).  The tables are the boosters' and the forest's: feat (< 0: a leaf or absent), thr, a leaf value and
 * the cover (n_node), [T][nn]; a row goes LEFT at split node s iff x[feat[s]] <= thr[s]; a node is a leaf iff feat < 0 or
 * 2s + 2 >= nn (mms_gbm_predict's rule).
 *
 * A tree, and a leaf l reached from the root by the edges e_1 .. e_d; edge k leaves split node s_k for child c_k and carries the
 * feature f_k = feat[s_k], the zero fraction z_k = cover[c_k] / cover[s_k] (fp64) and the one indicator o_k = [the row goes to c_k at
 * s_k] = ((x[f_k] <= thr[s_k]) == (c_k is the left child)).  Edges of a path that share a feature merge: z is the product in path
 * order, o the conjunction; that leaves u <= d unique features (z_j, o_j) in order of first occurrence.  With v the leaf's value:
 *     base  += v prod_k z_k                                  (v alone when the root is the leaf)
 *     phi_j += v (o_j - z_j) sum_{k=0}^{u-1} w_k e_k^(j),    w_k = k! (u - k - 1)! / u!,
 *              e_k^(j) = the coefficient of t^k in prod_{m != j} (z_m + o_m t)
 * A group's result is the SUM over its trees goff[g] .. goff[g+1) in table order, leaves depth-first and left-first, a leaf's
 * features in order of first occurrence; with `use` a row skips the trees that do not admit it (use[t][row] == 0).  Local accuracy:
 * base + sum_j phi_j = the sum of the leaf values the row reaches.  The only division is cover[c] / cover[s] at split nodes: the
 * CALLER guarantees cover[2s+1] + cover[2s+2] == cover[s] with both children > 0 there, feat < p and slot in [0, U)
 * (ops.tree_shap checks all of it on the host).
 *
 * mms_tree_shap, one launch: workgroup = (group, 64 rows), lane = row; phi [G][U][ldr] is SLOT-major (slot[t][s] = the output column
 * of feat[t][s]).  The launch writes every element of phi[g][0..U)[0..R) and base[g][0..R) itself (zeros where nothing contributes)
 * and nothing at columns >= R.  No atomics, no workgroup waits for another; a group's bits depend only on its own trees and rows.
 * The kernel is instantiated on the depth bound (6 when nn <= 127, else MMS_SHAP_MAX_DEPTH).  A NULL required pointer, R < 0,
 * ldx < p, p < 1, T < 0, G < 0, U < 1, nn outside 1..2^(MMS_SHAP_MAX_DEPTH + 1) - 1, ldr < R, ldu < R with use, ceil(R / 64) G >= 2^31
 * or a pointer not aligned to its element: MMS_ERR_ARG before any launch.  R = 0 or G = 0: MMS_OK without a launch. */
#define MMS_SHAP_MAX_DEPTH 12          /* = MMS_RSF_MAX_DEPTH >= MMS_GBM_MAX_DEPTH */
typedef struct TreeShapP {
    int R; int ldx; int p; int T; int nn; int G; int U; int ldr; int ldu; int pad_;
    const float* x;                     // [R][ldx] raw rows
    const int* feat; const float* thr; const double* value; const int* cover;   // [T][nn]
    const int* goff;                    // [G + 1] ascending: group g owns trees goff[g] .. goff[g+1)
    const int* slot;                    // [T][nn] output column (0 .. U-1) of feat at split nodes
    const unsigned char* use;           // [T][ldu] or NULL: tree t admits row r
    double* phi;                        // [G][U][ldr] out, SLOT-major
    double* base;                       // [G][ldr] out
} TreeShapP;

/* clip_grad_norm_(max_norm) + Adam/AdamW over one flat fp32 parameter buffer (R/...final_multimodal.py:259-260,350;
 * simple_fusion.py:273-274,391).  hyper (device): {lr, beta1, beta2, eps, weight_decay, max_norm}; state (device):
 * {step (as float), sumsq scratch (double as 2 floats)}; skip: optional device flag, 0 => no-op (degenerate batch). */
typedef struct AdamP {
    float* p; float* g; float* m; float* v; long long n;
    const float* hyper;             // [6]
    double* sumsq;                  // [1] zeroed by mms_grad_sumsq's caller each step
    float* step;                    // [1] step counter (incremented by the update kernel when not skipped)
    const float* skip_flag;         // null or device scalar: update only if *skip_flag != 0
    int adamw;                      // 0: Adam with L2-coupled weight decay; 1: AdamW (decoupled)
    /* optional per-step bookkeeping done by mms_grad_sumsq (all nullable): acc[4] += {loss*usable, usable, entropy, 1} */
    float* acc; const float* cox_out; const float* entropy;
    int* rng;                       // [2] dropout (seed, step counter): counter += 1 after the step's kernels have used it
    /* conv2 weights in packed primary storage (MmsDnOpts.w2_packed; n_w2 = 0: none).  The n_w2 tensors of 32 x 27 x 128 floats at
       offsets w2_off[i] (ascending) of p / g / m / v are stored [cout][tap][cin]; mms_clip_adam updates them with a kernel of their own
       that also writes the derived packs the convolution kernels read: w2_pack_b[i] = backward-data pack ([cin][tap][cout], or the
       backward MFMA-fragment order when bit i of w2_fragmask is set), w2_pack_f[i] = forward MFMA-fragment order (bit i set; else unused:
       the primary storage is the forward pack).  All three tables live in device memory. */
    const long long* w2_off; float* const* w2_pack_b; float* const* w2_pack_f; int n_w2; uint64_t w2_fragmask;
} AdamP;

/* Fine-tuning form of the optimiser step (csrc/finetune.hip): the flat buffer in nseg SEGMENTS, segment s = elements
 * [bounds[s], bounds[s + 1]) with lr_s = lr * lr_mult[s], wd_s = weight_decay * wd_mult[s] and an L2-SP pull of strength l2sp[s] towards
 * anchor (the weights fine-tuning started from; Li et al. 2018) where weight decay is applied, after clipping:
 *   Adam:  g <- coef * g + wd_s * w + l2sp_s * (w - anchor);   AdamW:  w <- w - lr_s * wd_s * w - lr_s * l2sp_s * (w - anchor), then Adam's step.
 * lr_mult[s] = 0 FREEZES the segment: its p / m / v are neither read nor written, its gradient is not read and stays out of the global
 * norm (torch: clip_grad_norm_ over the parameters that have a gradient).  One step counter; the skip_flag / acc / rng bookkeeping of
 * mms_grad_sumsq.  bounds [nseg + 1], lr_mult / wd_mult / l2sp [nseg] live in DEVICE memory and are shared by all members of a group
 * launch (the same pointers in every member); anchor [n] is per member, NULL when no trainable segment has l2sp > 0.
 * A launch checks what it can without reading device memory (nseg in 1..MMS_TUNE_MAX_SEG, no NULL table, p / g / m / v / anchor 16-byte
 * aligned, one table per group, n < 2^33); mms_tune_check reads the tables back (it synchronises: call it once, outside any capture)
 * and checks the rest: bounds strictly ascending from 0 to n, no bound inside a packed conv2 tensor, multipliers finite and >= 0, a
 * trainable segment, an anchor where one is needed.  Tables it would refuse make the launches wrong, not unsafe: a quad or packed tensor that
 * does not lie inside [0, n) is skipped, never addressed.  A multiplier of 1 everywhere gives the bits of mms_clip_adam. */
#define MMS_TUNE_MAX_SEG 512
typedef struct TuneP {
    AdamP a;
    const long long* bounds;
    const float* lr_mult;
    const float* wd_mult;
    const float* l2sp;
    int nseg;
    const float* anchor;
} TuneP;

/* Large-batch Linear (rows M > 32: BASELINE config 5, RNA-seq-only B = 2048; R/scripts/training/train_rnaseq_only.py:126-151).
 * y = P(x) W^T + bias [-> ReLU], P = Dropout(ReLU(BatchNorm1d(x))) of the PRECEDING nn.Sequential entries (has_bn = 0: P = identity
 * or dropout only).  fp32 MFMA GEMMs on the tile core; BatchNorm1d batch statistics travel like the BatchNorm3d ones: the
 * producing launch accumulates (sum, sumsq) of its output in fp64 (osum/osumsq), the consuming launch normalises in its
 * operand prologue (bn: sum/sumsq over the M rows).  Backward of one layer: mms_linear_big_bwd_w (dW, db), mms_linear_big_bwd_x
 * (gradient wrt P's output, through dropout/ReLU -> dbn + the two BN-backward column sums), mms_bn1d_bwd_apply (dx, dgamma, dbeta).
 * x, y, dy, dbn, dx may be column windows of wider buffers (pointer = base + column offset, ld = the buffer's pitch): the multimodal
 * heads write [ct | rna | clinical] into one feature buffer.  float4 operand loads need 16-byte aligned rows (offset and pitch multiples
 * of 4 floats, pitch >= offset + roundup4(K)); anything else takes the scalar loaders.  mms_linear_big_bwd_x: K % 4 == 0; w 16-byte
 * aligned -> float4 loads, 4-byte aligned -> 16-byte loads the hardware splits (a weight behind an odd-sized tensor in a flat buffer). */
typedef struct LinBigP {
    const float* x; int ldx; int M; int K;
    const float* w; const float* bias; int N;      // torch Linear: weight [N][K], bias [N]
    float* y; int ldy; int out_relu;
    int has_bn; BnSrc bn;                            // BatchNorm1d over the K input columns (train: batch sums of x; eval: running)
    float* rmean; float* rvar; long long* nbt; float momentum;   // running statistics, updated by the forward in train mode (nullable)
    float drop_p; const float* drop_mask; const uint32_t* rng; uint32_t stream_id; int train;
    double* osum; double* osumsq;                   // [N] statistics of y (nullable)
    /* backward */
    const float* dy; int lddy;                      // gradient wrt y (after out_relu)
    float* dw; float* dbias; int msplit;            // accumulated (atomics); rows split over msplit workgroups
    int core_only;                                  // 1: the 64x64 GEMM-core forms only, never the wide first-layer kernels (A/B measurements)
    float* dbn; int lddbn;                          // [M][K] gradient wrt BN output (has_bn) or wrt x (no BN)
    double* s1; double* s2;                         // [K] sum dbn, sum dbn * xhat (has_bn)
    float* dx; int lddx;                            // mms_bn1d_bwd_apply output
    float* dgamma; float* dbeta;
} LinBigP;

/* Learnable missing-modality bias (R/scripts/training/flexible_multimodal.py:205-206,243-250): per feature segment s
 * (image 128 | RNA 256 columns of the fused vector)   feats[m][j] = feats[m][j]*mask[m][s] + bias_s[j]*(1 - mask[m][s]),
 * in place; backward: dbias_s[j] += sum_m dfeats[m][j]*(1 - mask[m][s]);  dfeats[m][j] *= mask[m][s]. */
typedef struct MixP {
    float* feats; int ld; int M;
    const float* mask; int ldm;     // [M][ldm], column s = has-modality flag of segment s
    int nseg;                       // <= 4
    int seg_begin[4]; int seg_width[4];
    const float* bias[4];
    float* dfeats; int ldd;         // backward only
    float* dbias[4];
} MixP;

/* Gated mixture of modality experts (SimMLM_SurvivalNet, R/scripts/analysis/generate_km_curves.py:158-281), F = feature width:
 *   expert hazards  hz[:, 1 + e] = wx_e . f_e + bx_e   on the UNMASKED features f_e (e = image, rna, clinical);
 *   gate input      gin = [f_0 m_0 | f_1 m_1 | f_2 m_2 | m]  (3F + 3 columns) -> gate MLP 3F+3 -> 128 -> Dropout -> 64 (mms_linear_*) -> h2;
 *   gate            g = softmax(W3 h2 + b3 with the logits of modalities whose mask == 0 set to -inf);
 *   mixture         fused = sum_e g_e f_e m_e;   ensemble hazard hz[:, 0] = we . fused + be.
 * The forward runs in two stages around the gate MLP (stage 0: expert heads + gate input, valid_x; stage 1: gate output layer,
 * masked softmax, mixture, ensemble head); the backward in the reverse order (stage 1: ensemble head, mixture and gate gradients ->
 * dh2; stage 0: expert heads, and the gradient of the unmasked features = own Cox-head gradient + (mixture + gate-input gradient) * m_e).
 * A row whose mask is all zero: gate weights and ensemble hazard are NaN in the forward, as torch computes them; the backward
 * defines that row's gate and mixture gradients (and its share of the ensemble head's weight gradient) as 0, where torch would
 * spread NaN into every gate parameter gradient.  One workgroup per model; M <= 32 rows; weight gradients are summed over the
 * rows inside the workgroup (no atomics) and ADDED to dw*. */
typedef struct MoeP {
    int M; int F;                   // rows (1..32), feature width (positive multiple of 4)
    int stage;                      // 0 or 1 (see above)
    const float* feats; int ldf;    // [M][ldf] unmasked expert features: image | rna | clinical at columns 0, F, 2F
    const float* mask; int ldm;     // [M][ldm] modality flags in columns 0..2
    const float* valid;             // optional [M] has_survival (null = every row)
    float* valid_x;                 // optional [4][M] out (forward stage 0): the Cox terms' sets -- row 0 (ensemble): valid && some
                                    // mask != 0 (a row without any modality has a NaN ensemble hazard and is left out), row 1 + e: valid && mask_e != 0
    float* gin; int ldg;            // [M][ldg] gate input, 3F + 3 columns (forward stage 0 output)
    const float* h2; int ldh2;      // [M][ldh2] gate hidden after its second ReLU, 64 columns
    const float* w3; const float* b3;           // gate output layer [3][64], [3]
    const float* wx[3]; const float* bx[3];     // expert Cox heads [F], [1]
    const float* we; const float* be;           // ensemble Cox head [F], [1]
    float* hz; int ldhz;            // [M][ldhz] column 0 ensemble hazard, 1..3 expert hazards
    float* gate;                    // [M][3] gate weights
    float* fused;                   // [M][F] mixture (saved for the backward)
    /* backward */
    const float* dhz; int lddhz;    // [M][lddhz] gradient wrt the four hazard columns
    const float* dgate_ext;         // optional [M][3] gradient wrt the gate weights
    float* dh2; int lddh2;          // stage 1 out: gradient wrt h2 (overwritten)
    const float* dgin; int lddg;    // stage 0 in: gradient wrt the gate input (first 3F columns read)
    float* dfeats; int lddf;        // stage 0 out: gradient wrt the unmasked features (overwritten)
    float* dw3; float* db3; float* dwx[3]; float* dbx[3]; float* dwe; float* dbe;   // accumulated (+=)
    /* optional objective (backward stage 1): loss_out = {out_0[0] + expert_weight (out_1[0] + out_2[0] + out_3[0]), out_0[1]} over the
       CoxP.out blocks [4][2] of the ensemble and the three expert terms */
    const float* cox_outs; float expert_weight; float* loss_out;
} MoeP;

/* Batch assembly (the DataLoader collate + `.to(device)` of R/scripts/training/final_multimodal.py:228-247): row idx[b] of each
 * source array -> row b of its destination, all sources of all models of a fold group in ONE launch.  The sources live in HBM
 * (device-resident cohort) or in PINNED HOST memory (hipHostMalloc / torch pin_memory: the kernel then reads the rows over PCIe --
 * the host-to-device copy of the batch IS this launch).  present[i] != NULL: per-patient availability flag of source i's modality
 * (the cohort's mask column; R/scripts/training/partial_modality_training.py:96-141 yields all-zero tensors for a missing modality):
 * rows whose flag is 0 are zero-filled without being read (4 of 5 CT rows of BASELINE config 3's cohort). */
typedef struct GatherP {
    const long long* idx; int B;    // [B] patient indices (device)
    int nsrc;                       // sources used (<= 8)
    const float* src[8]; float* dst[8];
    int src_ld[8]; int dst_ld[8];   // row pitches in floats
    int width[8];                   // floats copied per row
    const float* present[8]; int present_ld[8];   // optional availability flag of row r: present[i][r * present_ld[i]]
} GatherP;

/* Batch assembly WITH augmentation (mms_gather_aug_group): the gather above with one parameter record per batch row applied inside
 * the copy -- no extra launch, no extra pass over the volumes.  Contract:
 *   CT volume  out[z,y,x] = scale * v + offset,  v = src[sz,sy,sx] inside the volume, 0 (air) outside,
 *              sz = (flip bit 0 ? D-1-z : z) - dz, likewise H (bit 1, dy) and W (bit 2, dx): the flip acts on the destination index
 *              first, then the shift.  No clamping.  scale == 1 && offset == 0 copies bits unchanged.
 *   drop bit j hides modality j (0 image, 1 rnaseq, 2 clinical: the column order of the cohort's mask): every source whose
 *              drop_bit is j is zero-filled without being read, column j of every MMS_AUG_MASK source is written as 0.
 *   Rows that are absent by GatherP.present stay all-zero (neither read nor transformed; offset is NOT added).
 * A record with flip = 0, shift = 0, scale = 1, offset = 0, drop = 0 yields exactly what mms_gather_rows_group yields. */
typedef struct AugRec {
    int flip;                       // bit 0 / 1 / 2: reverse axis D / H / W
    int dz; int dy; int dx;         // integer voxel translation, |dz| < D, |dy| < H, |dx| < W
    float scale; float offset;      // intensity map
    int drop;                       // bit 0 / 1 / 2: hide image / rnaseq / clinical
    int reserved;                   // 0 (keeps a record at 32 bytes)
} AugRec;
#define MMS_AUG_PLAIN 0             /* copied as by mms_gather_rows_group (plus the drop zero-fill) */
#define MMS_AUG_VOLUME 1            /* [D][H][W] CT volume, width == D*H*W; at most one per GatherP */
#define MMS_AUG_MASK 2              /* modality mask: GatherP.width <= 3 columns, column j belongs to modality j */
typedef struct AugP {
    const AugRec* rec;              // [B] records of this member's batch rows (device)
    int role[8];                    // MMS_AUG_* of GatherP source i
    int drop_bit[8];                // modality (0..2) whose drop bit zero-fills source i; -1: none
    int D; int H; int W;            // the volume source's shape
    int max_shift[3];               // bound on |dz|, |dy|, |dx| that the CALLER declares for its records: each must be < D / H / W, else MMS_ERR_ARG.
                                    // The records live on the device, so the launch cannot read them: the real check is the caller's, on the host
                                    // (augment.check_records).  The kernel is memory-safe for any record: it bounds-checks every source coordinate
                                    // and treats a shift of magnitude >= the extent as exactly the extent (everything is air)
} AugP;

/* Batch assembly with RESAMPLING augmentation (mms_gather_affine_group): the gather above with, per batch row, the AugRec AND a
 * second record that carries an affine source-coordinate map and additive noise.  Contract, for the
 * MMS_AUG_VOLUME source of a row that is neither absent nor dropped, destination voxel (z, y, x), i = (z*H + y)*W + x:
 *   source coordinate (voxel-index units, fp32, this fmaf chain and no other):
 *              cz = fmaf(m[0], z, fmaf(m[1], y, fmaf(m[2], x, m[3]))), cy likewise from m[4..7], cx from m[8..11]
 *   v        = trilinear sample of src at (cz, cy, cx): cell = floorf(c), weight of the upper corner = c - floorf(c) per axis; any of the
 *              eight corners outside [0,D) x [0,H) x [0,W) contributes 0 (air) -- the zero padding of
 *              grid_sample(padding_mode="zeros", align_corners=True), continuous in the coordinate.  A NaN coordinate is air.
 *   out      = fmaf(sigma, g(seed, i), fmaf(scale, v, offset)),  scale / offset from the row's AugRec; sigma == 0: no noise term
 *   g(seed,i): h0 = mix(seed, 2i), h1 = mix(seed, 2i + 1) with mix(s, k) = hash(k * 0x9E3779B9 + hash(s)) in uint32 arithmetic and
 *              hash(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16  (the mixer of the dropout masks);
 *              S = the sum of the eight bytes of h0 and h1 (0..2040); g = (float)(S - 1020) * 0x1.39897ep-8f  (= fp32 of 1/sqrt(43690)).
 *              The sum of eight uniform bytes has mean 1020 and variance 8 (256^2 - 1) / 12 = 43690: g has zero mean and unit variance,
 *              is bell-shaped and bounded by 4.88 -- an Irwin-Hall approximation of a Gaussian, reproducible bit for bit on a CPU and
 *              independent of the launch geometry.
 * AugRec.flip / dz / dy / dx are NOT read here: the host folds them into m (augment.affine_records).  drop, absent rows and every
 * source that is not the volume behave exactly as in mms_gather_aug_group (zero-filled rows get neither offset nor noise).  A record
 * with m = identity, sigma == 0, scale == 1, offset == 0 takes the copy path: the bits of mms_gather_rows_group.
 * The kernel is memory-safe for ANY m (NaN, Inf, huge: air): coordinates are clamped to [-2, extent + 1] before they become indices,
 * which changes no sample, and every corner index is bounds-checked. */
typedef struct AffRec {
    float m[12];                    // row-major 3x4: (cz, cy, cx) = m * (z, y, x, 1)
    float sigma;                    // noise amplitude, >= 0
    unsigned seed;                  // of this row's noise
    int reserved[2];                // 0 (keeps a record at 64 bytes)
} AffRec;
typedef struct AffP {
    const AffRec* rec;              // [B] records of this member's batch rows (device)
    int stage_floats;               // LDS staging budget of a destination tile's source box, in floats; 0: the library default (8192 = 32 KB
                                    // of the CU's 160 KB); larger values are capped there; a box that does not fit is sampled with bounds-checked
                                    // global loads instead (direct form: a small value forces it everywhere -- tests, A/B timing)
} AffP;

/* Batch assembly with ELASTIC deformation (mms_gather_elastic_group): mms_gather_affine_group with, per batch row, a third record that
 * names a free-form displacement field d, added to the destination voxel BEFORE the affine map.  The field is a pure function of the
 * record: a coarse lattice of control displacements from the counter hash, interpolated by uniform cubic B-splines; the kernel builds the
 * lattice in LDS, no field is stored in memory.  Contract, volume extents n = (D, H, W), axis a = 0 / 1 / 2:
 *   lattice   spacing s_a = 1 << log2_spacing[a] voxels, K_a = ((n_a - 1) >> log2_spacing[a]) + 4 control planes; plane j stands at lattice
 *             position j - 1, so the planes k .. k + 3 exist for every voxel.  3 K_D K_H K_W <= MMS_ELA_LATTICE_MAX, else MMS_ERR_ARG.
 *   control   component a at (jz, jy, jx), k = 3 ((jz K_H + jy) K_W + jx) + a:  c = amp_a * u(seed, k),
 *             u = (float)((int)(h >> 8) - 8388608) * 2^-23 in [-1, 1),  h = hash(k * 0x9E3779B9 + hash(seed ^ 0x85ebca6b))  (hash: the mixer
 *             above, uint32 arithmetic; the salt keeps the field independent of the noise of a row whose two seeds are equal).  u is exact
 *             in fp32, c is rounded once.  amp_a is the record's amp[a] CLAMPED by the kernel into [0, max_amp[a]], NaN -> 0.
 *   field     at destination voxel p = (z, y, x): k_a = p_a >> log2_spacing[a], r_a = (p_a & (s_a - 1)) / s_a (exact),
 *             d_a = sum_{i,j,m in 0..3} B_i(r_z) B_j(r_y) B_m(r_x) c_a[k_z + i, k_y + j, k_x + m],  B the uniform cubic B-spline basis
 *             B_0 = (1-r)^3 / 6, B_1 = (3r^3 - 6r^2 + 4) / 6, B_2 = (-3r^3 + 3r^2 + 3r + 1) / 6, B_3 = r^3 / 6: non-negative, sum 1, so
 *             |d_a| <= amp_a up to rounding.  The order of evaluation is the kernel's (gather_elastic.hip: numerators 6 B exact in fp32,
 *             z then y then x, one multiplication by fp32(1/216)): |d - exact| <= 16 * 2^-24 * amp_a.  amp bounds the CONTROL POINTS; the
 *             realised max |d| is typically 0.5 .. 0.7 amp.
 *   coords    cz = fmaf(m[0], z + d_z, fmaf(m[1], y + d_y, fmaf(m[2], x + d_x, m[3]))), cy, cx likewise; each p_a + d_a is one fp32 add.
 *             Everything after that -- clamp, zero-padded trilinear sample, intensity map, noise indexed by the DESTINATION voxel, absent
 *             and dropped rows, the other sources -- is mms_gather_affine_group's, unchanged.
 * Bit identities: a row whose clamped amplitudes are all 0 yields the bits of mms_gather_affine_group for the same records; the staged
 * and the direct form yield equal bits (AffP.stage_floats: 0, the library default, is the direct form for rows that deform -- the
 * faster one by measurement, their source boxes being widened by the amplitude -- and the affine launch's staged form for rows that do
 * not; a positive value is the staging budget of every row, as in the affine launch); a row's bits do not depend
 * on ng, the member position or what else shares the launch.  The kernel is memory-safe for any record contents.
 * No folding: p -> p + d(p) is injective when amp_a <= 0.4 s_a (Choi & Lee 2000); that check is the caller's, on the host
 * (augment.check_elastic_records), as the records live on the device.
 * mms_elastic_field writes d itself, out[b][a][z][y][x], through the device function the gather kernel calls (inspection, tests). */
#define MMS_ELA_LATTICE_MAX 6144    /* floats of the control lattice in LDS (24 KB beside the 32 KB staging box: two workgroups per CU).  Sized for the
                                       finest spacing (2) on the small volumes of quick runs and tests: 16 x 16 x 16 takes 5184, 8 x 24 x 32 takes 5985; the
                                       flagship 64 x 64 x 32 takes 735 at spacing 16.  A third workgroup per CU (16 KB) would buy nothing: the launch has at
                                       most 64 x B x ng workgroups for 256 CUs and is latency-bound */
typedef struct ElaRec {
    float amp[3];                   // control-point amplitude along D / H / W, voxels
    unsigned seed;                  // of this row's lattice
} ElaRec;
typedef struct ElaP {
    const ElaRec* rec;              // [B] records of this member's batch rows (device)
    int log2_spacing[3];            // control spacing 1 << log2_spacing[a] voxels along D / H / W; each in 1..6, else MMS_ERR_ARG
    float max_amp[3];               // bound the CALLER declares for its records' amp: finite, 0 <= max_amp[a] <= 64, else MMS_ERR_ARG
} ElaP;

/* ---- ABI self-description ---- */
int mms_abi_sizeof(const char* name);      /* sizeof(struct <name>) as compiled, -1 if unknown */
int mms_abi_version(void);

/* ---- DenseNet121-3D ops (MONAI DenseNet121(spatial_dims=3,in_channels=1,out_channels=128) at
 *      R/scripts/training/final_multimodal.py:66-71, partial_modality_training.py:171-176, simple_fusion.py:182-187) */
int mms_init_coords(int* coords, int B, int D, int H, int W, hipStream_t s);
int mms_conv0_fwd(const Conv0FwdP* p, hipStream_t s);          /* features.conv0 */
int mms_pool_fwd(const PoolFwdP* p, hipStream_t s);            /* features.norm0/relu0/pool0 */
int mms_conv1_fwd(const Conv1FwdP* p, hipStream_t s);          /* denselayer norm1/relu1/conv1; transition norm/relu/conv/pool */
int mms_conv3_fwd(const Conv3FwdP* p, hipStream_t s);          /* denselayer norm2/relu2/conv2 + torch.cat */
int mms_head_fwd(const HeadFwdP* p, hipStream_t s);            /* features.norm5 + class_layers */
int mms_conv3_bwd_data(const Conv3BwdDataP* p, hipStream_t s);  /* autograd of conv2 wrt its input + relu2 mask */
int mms_conv3_bwd_weight(const Conv3BwdWP* p, hipStream_t s);    /* autograd of conv2 wrt weight */
int mms_conv1_bwd_data(const Conv1BwdP* p, hipStream_t s);       /* norm2 backward + conv1 wrt input + relu1 mask */
int mms_conv1_bwd_weight(const Conv1BwdP* p, hipStream_t s);     /* norm2 backward + conv1 wrt weight */
int mms_bn_bwd_apply(const BnBwdApplyP* p, hipStream_t s);       /* norm1 backward into the block's gradient slab */
int mms_head_bwd(const HeadBwdP* p, hipStream_t s);              /* class_layers + norm5 backward */
int mms_pool_bwd(const PoolBwdP* p, hipStream_t s);              /* pool0 + relu0 backward */
int mms_conv0_bwd_weight(const Conv0BwdWP* p, hipStream_t s);    /* norm0 backward + conv0 wrt weight */
int mms_unpack_conv3_grads(const void* table_host, int nlayers, hipStream_t s);   /* host array of {scratch [27][32][128], dw canonical}, <= 64 layers */
int mms_pack_conv3(const float* w, float* wpf, float* wpb, hipStream_t s);
int mms_pack_conv3_frag(const float* w, float* wff, float* wfb, hipStream_t s);   /* canonical [32][128][27] -> the two MFMA-fragment orders (Conv3FwdP.wfrag / Conv3BwdDataP.wfrag) */
int mms_pack_conv3_table(const void* table_dev, int nlayers, hipStream_t s);
int mms_bn_running_update(const void* table_dev, int n, float momentum, hipStream_t s);


/* ---- fallback encoder ops + whole-encoder driver (params: 12 pointers in named_parameters() order of the
 *      nn.Sequential -- {0,1,3,4,6,7}.{weight,bias}; buffers: 3 x {running_mean, running_var, num_batches_tracked}) ---- */
int mms_fb_conv_fwd(const FbConvP* p, hipStream_t s);
int mms_fb_conv_bwd_w(const FbConvP* p, hipStream_t s);
int mms_fb_conv_bwd_x(const FbConvP* p, hipStream_t s);
int mms_fb_pool_fwd(const FbPoolP* p, hipStream_t s);
int mms_fb_pool_bwd(const FbPoolP* p, hipStream_t s);
int mms_fb_workspace_bytes(int B, int D, int H, int W, size_t* bytes);
int mms_fb_init(void* ws, int B, int D, int H, int W, const void* const* buffers, hipStream_t s);
int mms_fb_forward(void* ws, int B, int D, int H, int W, const float* x, const void* const* params,
                   const void* const* buffers, float* out, int ldo, int train, hipStream_t s);
int mms_fb_backward(void* ws, int B, int D, int H, int W, const float* x, const void* const* params,
                    const float* dout, int lddout, void* const* grads, hipStream_t s);
/* The same drivers at other channel widths: widths = int[3], the three convolutions' output channels, each a multiple of 16 in 16..128
 * (ImageOnlyModel: {16, 32, 64}; mms_fb_* above = {32, 64, 128}).  Tables as above (12 params, 9 buffers, 12 grads; every entry non-NULL);
 * out / dout hold widths[2] columns.  ws_bytes: what the caller allocated -- anything but mms_fb3_workspace_bytes of THESE widths and
 * dims is MMS_ERR_ARG (a workspace planned for another width set is laid out differently).  mms_fb3_forward / _backward run the scalar
 * kernels above (a thread per (voxel, channel) of a 256-thread workgroup): their widths must divide 256 -- 16, 32, 64, 128. */
int mms_fb3_workspace_bytes(const int* widths, int B, int D, int H, int W, size_t* bytes);
int mms_fb3_init(void* ws, size_t ws_bytes, const int* widths, int B, int D, int H, int W, const void* const* buffers, hipStream_t s);
int mms_fb3_forward(void* ws, size_t ws_bytes, const int* widths, int B, int D, int H, int W, const float* x, const void* const* params,
                    const void* const* buffers, float* out, int ldo, int train, hipStream_t s);
int mms_fb3_backward(void* ws, size_t ws_bytes, const int* widths, int B, int D, int H, int W, const float* x, const void* const* params,
                     const float* dout, int lddout, void* const* grads, hipStream_t s);

/* ---- input-gradient attribution (csrc/attrib.hip): the data path of a backward with FROZEN statistics -- every BatchNorm is the
 *      per-channel affine map of its running statistics, its backward dx = gamma / sqrt(rvar + eps) * dy.  No weight gradient, no parameter
 *      or buffer is written, no float atomics (two calls give the same bits), no workgroup waits for another. ---- */
int mms_conv0_bwd_data(const Conv0BwdDataP* p, hipStream_t s);   /* norm0 (frozen) backward + conv0 wrt the volume */
int mms_conv0_bwd_data_group(const Conv0BwdDataP* p, int ng, hipStream_t s);     /* grid z = member; members of identical shape */
/* DenseNet121-3D: after an EVAL-mode mms_dn121_forward of the same x on the same workspace, run in its per-layer forms (MmsDnOpts
 * persist_b3 = persist_b4 = fuse_layers = -1: they leave y0, argmax, the slabs and every layer's y1): dx [B][D][H][W] = gradient of
 * sum_b dout[b] . features[b] with respect to the volume, written.  params / buffers / opts as mms_dn121_forward (buffers required: the
 * running statistics; opts must select the same conv2 pack layout as the forward: w2_packed, conv3_small).  Runs the training
 * backward's data kernels with BnSrc.train = 0, then mms_pool_bwd and mms_conv0_bwd_data; the per-step statistic scratch of the
 * workspace is overwritten (the next training forward zeroes it), nothing else. */
int mms_dn121_input_grad(void* ws, int B, int D, int H, int W, const float* x, const void* const* params, const void* const* buffers,
                         const float* dout, int lddout, float* dx, const MmsDnOpts* opts, hipStream_t s);
/* After an EVAL-mode mms_fb3_forward of the same x on the same workspace (it leaves the three raw convolution outputs): dx [B][D][H][W] =
 * gradient of sum_b dout[b] . features[b] with respect to the volume, written.  Arguments as mms_fb3_backward, buffers as mms_fb3_forward
 * (running statistics, required); overwrites only the workspace's gradient scratch, which every training backward rewrites before use. */
int mms_fb3_input_grad(void* ws, size_t ws_bytes, const int* widths, int B, int D, int H, int W, const float* x, const void* const* params,
                       const void* const* buffers, const float* dout, int lddout, float* dx, hipStream_t s);
/* Lock-step forms of the two drivers above: member g of the group is entry g of every array (one B, D, H, W and, for the 3-conv encoder,
 * one width set).  The launch sequence is the single-model driver's, every launch issued once with ng parameter blocks (grid z = member);
 * the single-model drivers ARE the ng = 1 calls.  x[g] may be the same pointer for every member (an ensemble reads one copy of the batch);
 * ws[g], dout[g] and dx[g] are per member.  After the group's EVAL-mode forward in the per-layer forms (mms_dn121_forward_group with
 * persist_b3 = persist_b4 = fuse_layers = -1 / mms_fb3_forward_group).  ng outside 1..MMS_MAX_GROUP, a NULL array or entry, a shape outside
 * the workspace plan's domain or lddout below the feature width: MMS_ERR_ARG, nothing is launched. */
int mms_dn121_input_grad_group(int ng, void* const* ws, int B, int D, int H, int W, const float* const* x, const void* const* const* params,
                               const void* const* const* buffers, const float* const* dout, int lddout, float* const* dx,
                               const MmsDnOpts* opts, hipStream_t s);
int mms_fb3_input_grad_group(int ng, void* const* ws, size_t ws_bytes, const int* widths, int B, int D, int H, int W, const float* const* x,
                             const void* const* const* params, const void* const* const* buffers, const float* const* dout, int lddout,
                             float* const* dx, hipStream_t s);

/* ---- ensemble reduce (csrc/ensemble.hip): K members' values of one tensor -> their mean and population standard deviation ----
 *   mean[i] = (1/K) sum_g x[g][i] (summed in member order),  spread[i] = sqrt((1/K) sum_g (x[g][i] - mean[i])^2)
 * for i < n.  The K values of an element are held in registers and the deviations are taken from the finished mean (two passes, no
 * cancellation); K = 1 gives the input bit for bit and a spread of exactly 0; a NaN in any member reaches both outputs.  spread may be
 * NULL (the mean only).  Every pointer 16-byte aligned.  K outside 1..MMS_MAX_GROUP, a NULL x[g] for g < K, a NULL mean, n = 0 or a
 * misaligned pointer: MMS_ERR_ARG.  No atomics: two calls give the same bits. */
typedef struct EnsP {
    const float* x[10];             // [MMS_MAX_GROUP] members, the first K read
    int K; size_t n;
    float* mean; float* spread;     // [n]; spread optional
} EnsP;
int mms_ensemble_reduce(const EnsP* p, hipStream_t s);

/* ---- heads ---- */
int mms_linear_fwd(const LinearFwdP* p, hipStream_t s);        /* nn.Linear (+ preceding BN1d/ReLU/Dropout, + following ReLU) */
int mms_linear_bwd(const LinearBwdP* p, hipStream_t s);
int mms_gate_fwd(const GateP* p, hipStream_t s);
int mms_gate_bwd(const GateP* p, hipStream_t s);
int mms_gate_entropy(const float* gate, int M, float scale, float* loss, float* dgate, hipStream_t s);  /* gate_entropy_loss value (+= into *loss) and gradient */
int mms_linear_big_fwd(const LinBigP* p, hipStream_t s);
int mms_linear_big_bwd_w(const LinBigP* p, hipStream_t s);
int mms_linear_big_bwd_x(const LinBigP* p, hipStream_t s);
int mms_bn1d_bwd_apply(const LinBigP* p, hipStream_t s);
int mms_missing_mix_fwd(const MixP* p, hipStream_t s);        /* R/scripts/training/flexible_multimodal.py:243-250 */
int mms_missing_mix_bwd(const MixP* p, hipStream_t s);
int mms_cox_fwd_bwd(const CoxP* p, hipStream_t s);
int mms_moe_fwd(const MoeP* p, hipStream_t s);                 /* R/scripts/analysis/generate_km_curves.py:262-281 (MoeP above) */
int mms_moe_bwd(const MoeP* p, hipStream_t s);
int mms_cindex_counts(const CindexP* p, hipStream_t s);
int mms_cindex_boot(const CbootP* p, hipStream_t s);           /* bootstrap / weighted pair counts of M models x R replicates (CbootP above) */
int mms_gene_screen(const GeneScreenP* p, hipStream_t s);     /* univariate Cox score test of G genes on P problems (GeneScreenP above) */
int mms_logrank_scan(const LogrankScanP* p, hipStream_t s);   /* log-rank statistic of every cut of Q problems (LogrankScanP above) */
int mms_td_metrics(const TdMetricsP* p, hipStream_t s);       /* IPCW Brier / dynamic AUC sums of M models x H horizons x R replicates (TdMetricsP above) */
int mms_cox_newton(const CoxNewtonP* p, hipStream_t s);       /* Newton-Raphson Cox fits of R replicates x S covariate subsets (CoxNewtonP above) */
int mms_rsf_split(const RsfSplitP* p, hipStream_t s);         /* random survival forest: one level of T trees (RsfSplitP above) */
int mms_rsf_leaves(const RsfLeavesP* p, hipStream_t s);       /* ... mortality and H at the horizons of every leaf */
int mms_rsf_predict(const RsfPredictP* p, hipStream_t s);     /* ... masked mean over the trees for R rows */
int mms_rsf_vimp(const RsfVimpP* p, hipStream_t s);           /* ... permutation importance: P problems x R repeats (RsfVimpP above) */
int mms_gbm_grad(const GbmGradP* p, hipStream_t s);           /* gradient-boosted Cox trees: quantised gradients of a round (GbmGradP above) */
int mms_gbm_split(const GbmSplitP* p, hipStream_t s);         /* ... one level: histograms, cuts, fixed-order argmax, routing */
int mms_gbm_update(const GbmUpdateP* p, hipStream_t s);       /* ... leaf values, F, evaluation pair counts */
int mms_gbm_predict(const GbmPredictP* p, hipStream_t s);     /* ... F of raw rows after each of K round counts */
int mms_tree_shap(const TreeShapP* p, hipStream_t s);         /* path-dependent TreeSHAP of tree tables, G groups of trees in one launch */
int mms_gsea_scores(const GseaScoreP* p, hipStream_t s);      /* gene-set enrichment: permutation Z of G genes x R1 relabellings (GseaScoreP above) */
int mms_gsea_es(const GseaEsP* p, hipStream_t s);             /* ... enrichment score of S sets in R1 replicates (GseaEsP above) */
int mms_coxnet_eval(const CoxnetP* p, hipStream_t s);       /* elastic-net Cox: eta, residual, loss and gradient of P problems at beta (CoxnetP above) */
int mms_coxnet_iterate(const CoxnetP* p, int iters, hipStream_t s);   /* ... `iters` lock-step proximal-gradient rounds of P problems */
int mms_grad_sumsq(const AdamP* p, hipStream_t s);             /* sum of squares of the flat gradient (fp64 atomics) */
int mms_clip_adam(const AdamP* p, hipStream_t s);              /* clip by global norm + Adam/AdamW update (+ the derived conv2 packs, AdamP.w2_*) */
int mms_tune_check(const TuneP* p);                            /* contents of TuneP's device tables (TuneP above); synchronises */
int mms_grad_sumsq_tuned(const TuneP* p, hipStream_t s);       /* mms_grad_sumsq over the trainable segments */
int mms_clip_adam_tuned(const TuneP* p, hipStream_t s);        /* mms_clip_adam with per-segment settings; frozen segments untouched */
int mms_grad_sumsq_tuned_group(const TuneP* p, int ng, hipStream_t s);     /* ng <= MMS_MAX_GROUP members, one segment table */
int mms_clip_adam_tuned_group(const TuneP* p, int ng, hipStream_t s);
int mms_w2_pack(const AdamP* p, hipStream_t s);                /* the derived conv2 packs alone, from the current weights (after load_state_dict / any external update) */

/* ---- whole-encoder driver: replaces `self.ct_encoder(ct)` / `self.image_encoder(image)` and its autograd
 *      (R/scripts/training/final_multimodal.py:124, partial_modality_training.py:245, simple_fusion.py:226).
 *      params: 364 device pointers in torch named_parameters() order of MONAI DenseNet121;
 *      buffers: 121 x {running_mean, running_var, num_batches_tracked} in module order;
 *      grads: 364 device pointers, ACCUMULATED into (caller zeroes).  D,H,W multiples of 32.            */
int mms_ablation_build(void);      /* 1: the library was built with a timing-ablation flag (MMS_CXXFLAGS=-DMMS_ABLATE_..., tools/ablate*.sh): launches
                                      may be left out of the step -- diagnostics only; bench.py refuses to report a value from such a build */
int mms_dn121_workspace_bytes(int B, int D, int H, int W, size_t* bytes);
/* Named workspace regions (tests, diagnostics): byte offset and size.  "y0", "slab" / "dslab" [block], "y1" [layer], "tpool" [transition],
 * "stats" (the per-step zeroed region), "b4_err", "hx", and "bwd_live": ONE 32-bit word per workspace, written by the head launch of
 * every mms_dn121_backward / _group call with MmsDnOpts.skip_dead_bwd on -- 1 = this model's dout had an element unequal to 0.0f
 * (or was too large to scan), 0 = the later launches of that call returned at once.  Outside the per-step zeroed region; undefined
 * before the first such call, not touched by the staged / SyncBN / input-gradient drivers.  "bwd_dup": ONE word likewise, written by
 * the same launch where MmsDnOpts.dup_zero_bwd is on: the bit mask of the samples whose gradient rows are identical, 0 = nothing to share. */
int mms_dn121_region(int B, int D, int H, int W, const char* name, int index, size_t* off, size_t* bytes);
int mms_dn121_init(void* ws, int B, int D, int H, int W, const void* const* params, const void* const* buffers, const MmsDnOpts* opts, hipStream_t s);
/* which dense layers (bit l, l < 58) get their conv2 packs in MFMA-fragment order for this problem and these options (the layers whose
   launches take the small-grid kernels of csrc/dn_c3s.hip) */
int mms_dn121_w2_fragmask(int B, int D, int H, int W, const MmsDnOpts* opts, uint64_t* mask);
/* opts: launch-shape options incl. the width of class_layers.out (MmsDnOpts above; NULL = defaults). */
int mms_dn121_forward(void* ws, int B, int D, int H, int W, const float* x, const void* const* params,
                      const void* const* buffers, float* out, int ldo, int train, const MmsDnOpts* opts, hipStream_t s);
int mms_dn121_backward(void* ws, int B, int D, int H, int W, const float* x, const void* const* params,
                       const float* dout, int lddout, void* const* grads, const MmsDnOpts* opts, hipStream_t s);
/* mms_dn121_backward that stops above dense block block_lo (0..3): stages 3 .. block_lo, where stage b = dense block b (denseblock{b+1})
 * plus the transition below it (b = 0: the stem), and norm5 / class_layers ride with stage 3.  The gradients of the parameters below
 * are not written (they stay as the caller zeroed them).  One unstaged call: skip_dead_bwd, the weight-gradient tables and the default
 * launch forms stay in force; block_lo = 0 enqueues exactly what mms_dn121_backward enqueues.  block_lo outside 0..3: MMS_ERR_ARG. */
int mms_dn121_backward_from(void* ws, int B, int D, int H, int W, const float* x, const void* const* params,
                            const float* dout, int lddout, void* const* grads, int block_lo, const MmsDnOpts* opts, hipStream_t s);
/* ---- data-parallel (one process per GPU) variants of the single-model drivers --------------------------------------------
 * The reference is single-process (R/scripts/training/final_multimodal.py:52,345); BASELINE config 4 shards a global batch over
 * ranks.  Two things then leave the rank: (a) the gradients, all-reduced bucket by bucket while the backward still runs -- the
 * backward is issued in STAGES, dense blocks block_hi..block_lo (3 = denseblock4 + norm5/class_layers + transition3, ..., 0 =
 * denseblock1 + stem), each finalising one contiguous range of the parameter table (incl. its conv2 gradient unpack);
 * (b) with SyncBN, every BatchNorm statistic: the drivers call `hook` right after each kernel that produced accumulator words and
 * before the first kernel that consumes them; the hook all-reduces (SUM over ranks, in place) the words
 *     base[r * rep_stride + j * pair_stride + c],  r < nrep, j < 2, c < ncols        (fp64)
 * on stream s and returns 0.  bn_world = ranks the statistics span (counts become bn_world * rows); hook may be null (bn_world 1).
 * mms_dn121_init_sync: as mms_dn121_init, running-statistics table built for bn_world * rows. */
typedef int (*mms_sync_fn)(void* user, double* base, int nrep, long rep_stride, int ncols, long pair_stride, hipStream_t s);
int mms_dn121_init_sync(void* ws, int B, int D, int H, int W, const void* const* params, const void* const* buffers, int bn_world,
                        const MmsDnOpts* opts, hipStream_t s);
int mms_dn121_forward_sync(void* ws, int B, int D, int H, int W, const float* x, const void* const* params,
                           const void* const* buffers, float* out, int ldo, int bn_world, mms_sync_fn hook, void* user,
                           const MmsDnOpts* opts, hipStream_t s);
int mms_dn121_backward_stage(void* ws, int B, int D, int H, int W, const float* x, const void* const* params,
                             const float* dout, int lddout, void* const* grads, int block_hi, int block_lo,
                             int bn_world, mms_sync_fn hook, void* user, const MmsDnOpts* opts, hipStream_t s);
int mms_head_bwd_sums(const HeadBwdP* p, hipStream_t s);         /* SyncBN split of mms_head_bwd: masked gradient stash + local sums */
int mms_head_bwd_apply(const HeadBwdP* p, hipStream_t s);        /* ... norm5 backward with the (all-reduced) sums + class_layers.out gradients */

/* ---- preprocessing upstream of the path, on the GPU (replaces per-item numpy/scipy on the CPU) ----
 * mms_ct_preprocess: (x - min) / (max - min + 1e-8) and scipy.ndimage.zoom(order=1) to the network grid
 *   (R/scripts/training/partial_modality_training.py:94-109, simple_fusion.py:117-134); scratch >= 512 floats.  x - min is taken
 *   BEFORE the interpolation (csrc/ct_resample.h, shared with mms_ct_preprocess_raw_batch): a constant volume gives exact zeros, no
 *   output is below 0, and a float32 volume gives the bits mms_ct_preprocess_raw_batch gives for it as MMS_CT_F32, slope 1.
 * mms_rna_log_zscore: log2(count + 1), then per-gene StandardScaler over the n samples
 *   (R/scripts/preprocessing/preprocess_genomic.py:108-117); mean, two-pass variance and centring in fp64, one rounding to fp32. */
int mms_ct_preprocess(const float* x, int inD, int inH, int inW, float* out, int oD, int oH, int oW, float* scratch, hipStream_t s);
int mms_rna_log_zscore(const float* counts, float* out, int n, int g, hipStream_t s);

/* mms_ct_preprocess_raw_batch (csrc/ct_ingest.hip): mms_ct_preprocess for V volumes of different sizes and STORED types in one call,
 * straight from the bytes of their files (NIfTI-1 data sections, nifti.py): no host conversion and no fp32 copy of a scan.
 * The volumes stand in one device staging buffer `base` of base_bytes bytes, volume v at byte `offset` (16-byte aligned) as D x H x W
 * elements of `dtype` (x fastest), byte-swapped when `swap` != 0.  A stored element r stands for slope * r + inter (NIfTI scl_slope /
 * scl_inter; slope 0 means "no scaling": 1, 0).  Row out_row of out[n_rows][oD][oH][oW] receives
 *     zoom_order1( ((slope r + inter) - lo) / (hi - lo + 1e-8) ),   lo / hi the extremes of slope r + inter over the volume,
 * computed as (r - rmin) * |slope| / (|slope| (rmax - rmin) + 1e-8) on the raw extremes ((rmax - r) for a negative slope), so nothing
 * cancels and a constant volume gives exact zeros.  Output coordinates as mms_ct_preprocess: o * (in - 1) / (out - 1) in fp64, upper
 * neighbour clamped, scale 0 where out == 1; interpolation in fp32.
 * Precision: int8 / uint8 / int16 / uint16 / float32 elements are exact in fp32; int32, uint32 and float64 elements are rounded to the
 * nearest fp32 at the load (what a host astype(float32) does).  NaN elements are not supported (the extremes drop them, the voxels
 * they touch come out NaN).
 * `vols` is a HOST array, read during the call only: the kernels get the descriptors by value, MMS_CT_RAW_CHUNK volumes per launch
 * pair (pass 1: per-volume partial extremes into scratch, plain stores; pass 2: reduce them, resample, normalise).  A volume's bits do
 * not depend on what else is in the call.  scratch: >= MMS_CT_RAW_SCRATCH_FLOATS floats, whatever V.
 * p, base, out, scratch or (V > 0) vols NULL; base not 16-byte or out / scratch not 4-byte aligned; V < 0 or > MMS_CT_RAW_MAX_VOLS;
 * base_bytes < 0; n_rows < 1; a target dim < 1 or oD * oH * oW > MMS_CT_RAW_MAX_VOXELS; per volume: offset negative or not a multiple
 * of 16, a dim < 1, D * H * W > MMS_CT_RAW_MAX_VOXELS, the volume's end past base_bytes, an unknown dtype, slope or inter not finite,
 * out_row outside [0, n_rows), or an out_row given twice; passes outside 0..2, or != 0 with V > MMS_CT_RAW_CHUNK: MMS_ERR_ARG before
 * any launch.  V = 0: MMS_OK without a launch. */
#define MMS_CT_U8 2                     /* dtype codes = the NIfTI-1 datatype codes */
#define MMS_CT_I16 4
#define MMS_CT_I32 8
#define MMS_CT_F32 16
#define MMS_CT_F64 64
#define MMS_CT_I8 256
#define MMS_CT_U16 512
#define MMS_CT_U32 768
#define MMS_CT_RAW_CHUNK 32             /* volumes per launch pair: 32 descriptors by value stay well under the 4 KB kernarg limit */
#define MMS_CT_RAW_PARTS 256            /* partial extremes (workgroups of pass 1) per volume, at most */
#define MMS_CT_RAW_SCRATCH_FLOATS 16384 /* 2 * MMS_CT_RAW_PARTS * MMS_CT_RAW_CHUNK: the chunks of a call follow each other on the stream */
#define MMS_CT_RAW_MAX_VOLS 4096        /* volumes per call */
#define MMS_CT_RAW_MAX_VOXELS 2147483647 /* voxels per volume: element indices are 32-bit */
typedef struct CtRawVol {
    long long offset;                   // byte offset of the volume in base, a multiple of 16
    int D; int H; int W;                // stored dims, W fastest
    int dtype; int swap;                // MMS_CT_*; != 0: elements are in the other byte order
    int out_row;                        // row of out
    float slope; float inter;           // value = slope * stored + inter; slope 0 = (1, 0)
} CtRawVol;
typedef struct CtRawBatchP {
    const void* base; long long base_bytes;
    const CtRawVol* vols; int V;        // HOST array [V]
    int n_rows;
    float* out;                         // [n_rows][oD][oH][oW]
    int oD; int oH; int oW;
    int passes;                         // 0 = both (every caller but a timer); 1 / 2 = that pass alone, for V <= MMS_CT_RAW_CHUNK
                                        // (tools/bench_ingest.py: pass 2 alone reads the partials an earlier call left in scratch)
    float* scratch;                     // [MMS_CT_RAW_SCRATCH_FLOATS]
} CtRawBatchP;
int mms_ct_preprocess_raw_batch(const CtRawBatchP* p, hipStream_t s);

/* =========================== fold groups =====================================================================
 * The reference trains its K fold models one after the other (R/scripts/training/final_multimodal.py:316-402,
 * partial_modality_training.py:482-560, simple_fusion.py:318-436); they are independent, so this library can advance
 * ng <= MMS_MAX_GROUP of them in lock-step: every *_group entry point takes an ARRAY of ng parameter blocks (one per
 * model, identical shapes, any pointers) and issues ONE launch whose grid carries the model index as an extra
 * dimension.  Per-model arithmetic is exactly that of the single-model entry point (which is the ng = 1 case of the
 * same kernel); a batch-4 step of one model cannot fill 256 CUs, a group of them can.
 * The convolution entry points that have several kernel forms take the launch-shape options (MmsDnOpts; NULL = defaults). */
int mms_conv0_fwd_group(const Conv0FwdP* p, int ng, const MmsDnOpts* opts, hipStream_t s);
/* The same, and the zero-sample words of MmsDnOpts.dup_zero (the parameter block's layout is kept, so they travel beside it): zwords[g] =
 * model g's [B <= 32] words, ZERO on entry, or NULL; zwords NULL = none.  The boxed kernel adds to word b the number of 4x4x4 output boxes of
 * sample b that it found all zero (c0_zero_skip), once per workgroup and model; afterwards sample b is an all-zero volume iff
 * zwords[g][b] == (out.D/4)*(out.H/4)*(out.W/4).  Nothing is written by the unboxed form, with c0_zero_skip = -1 or with B > 32. */
int mms_conv0_fwd_group_zw(const Conv0FwdP* p, unsigned* const* zwords, int ng, const MmsDnOpts* opts, hipStream_t s);
int mms_pool_fwd_group(const PoolFwdP* p, int ng, hipStream_t s);
int mms_pool_act_group(const PoolActP* p, int ng, hipStream_t s);       /* transition.norm / relu / pool (before transition.conv) */
int mms_conv1_fwd_group(const Conv1FwdP* p, int ng, const MmsDnOpts* opts, hipStream_t s);
int mms_conv3_fwd_group(const Conv3FwdP* p, int ng, const MmsDnOpts* opts, hipStream_t s);
int mms_head_fwd_group(const HeadFwdP* p, int ng, hipStream_t s);
int mms_conv3_bwd_data_group(const Conv3BwdDataP* p, int ng, const MmsDnOpts* opts, hipStream_t s);
int mms_conv3_bwd_weight_group(const Conv3BwdWP* p, int ng, const MmsDnOpts* opts, hipStream_t s);
/* Conv3BwdWP.msplit the whole-encoder drivers use for a launch of `members` (model, layer) members of M rows each (0: bad arguments) --
   so that a caller timing the launch alone (bench.py's roofline leg) shapes it exactly as the step does */
int mms_conv3_bwd_weight_msplit(int M, int members, const MmsDnOpts* opts);
/* The kernel form a *_group entry point takes for a launch of ng members shaped like `p0` under `opts` -- host only: no launch, no device
   access; of the block's pointers only their being NULL and their alignment are read, as the launchers do.  op: MMS_OP_*, p0: member 0's
   parameter block of that op.  Decided by the launchers' own predicates (csrc/dn_ops.h), so a test that must reach one form can assert
   that it does.  -> MMS_FORM_* of the op (> 0), or MMS_ERR_ARG for an unknown op, a NULL block, ng outside 1..MMS_MAX_GROUP or a block
   the entry point refuses for its own fields.  Each launcher switches on the same function, so the answer is what runs for members that
   pass the launcher's comparison with member 0; one answer depends on the other members: MMS_FORM_C1_FUSED_WHOLEM needs every member to
   qualify (else the launch takes MMS_FORM_C1_FUSED_TILE). */
#define MMS_OP_CONV1_FWD 1            /* Conv1FwdP     */
#define MMS_OP_CONV1_BWD_DATA 2       /* Conv1BwdP     */
#define MMS_OP_CONV3_FWD 3            /* Conv3FwdP     */
#define MMS_OP_CONV3_BWD_DATA 4       /* Conv3BwdDataP */
#define MMS_OP_CONV3_BWD_WEIGHT 5     /* Conv3BwdWP    */
#define MMS_FORM_C1_WHOLEK8 1         /* conv1 forward: 16x16 whole-K kernel, K <= 512 */
#define MMS_FORM_C1_WHOLEK16 2        /*                16x16 whole-K kernel, K > 512 */
#define MMS_FORM_C1_TILE32 3          /* conv1 forward / backward-data: 32x32 tile GEMM */
#define MMS_FORM_C1_TILE64 4          /*                                64x64 tile GEMM */
#define MMS_FORM_C1_KSPLIT 5          /* conv1 forward: 32x32 tiles, K split over workgroups, last-arriver fix-up */
#define MMS_FORM_C1_FUSED_WHOLEM 6    /* conv1 backward-data with norm1's backward: whole-M kernel (csrc/dn_c1s.hip) */
#define MMS_FORM_C1_FUSED_TILE 7      /*                                            tile-GEMM epilogue */
#define MMS_FORM_C3_SMALL1 1          /* conv2 forward / backward-data: small-grid kernel, one 16-column tile per wave (JN = 1) */
#define MMS_FORM_C3_SMALL2 2          /*                                small-grid kernel, two (JN = 2) */
#define MMS_FORM_C3_MT32 3            /*                                multi-tap kernel, 32-row tiles */
#define MMS_FORM_C3_MT64 4            /* conv2 forward: multi-tap kernel, 64-row tiles */
#define MMS_FORM_C3_TAPSPLIT 5        /* conv2 forward / backward-data: taps split over workgroups + reduce launch */
#define MMS_FORM_C3_TAPGEMM 6         /*                                one-tap-per-step tile GEMM */
#define MMS_FORM_C3W_TAPGEMM 1        /* conv2 weight gradient: one-tap tile GEMM */
#define MMS_FORM_C3W_MT 2             /*                        multi-tap kernel */
int mms_dn_launch_form(int op, const void* p0, int ng, const MmsDnOpts* opts);
int mms_conv1_bwd_data_group(const Conv1BwdP* p, int ng, const MmsDnOpts* opts, hipStream_t s);
int mms_conv1_bwd_weight_group(const Conv1BwdP* p, int ng, hipStream_t s);
/* The table-fed form of the two weight-gradient launches above (MmsWgradModel): which = 1 conv2, 2 conv1, 3 both.  MMS_ERR_ARG and no
   launch for nmembers outside 1..MMS_WGRAD_MAX_MEMBERS, nmodels outside 1..MMS_WGRAD_MAX_MODELS, models of unequal M / grid / replicas,
   a member whose model or layer index is out of range (layers: K = C0 + 32 layer <= ld - 32), or a row chunk over 1024 rows. */
int mms_wgrad_tab_group(const MmsWgradModel* models, int nmodels, const MmsWgradMember* members, int nmembers,
                        const MmsWgradShape* shape, int which, hipStream_t s);
int mms_bn_bwd_apply_group(const BnBwdApplyP* p, int ng, hipStream_t s);
int mms_head_bwd_group(const HeadBwdP* p, int ng, hipStream_t s);
/* The same, and the two words that the later launches of a backward read (the parameter block's layout is kept, so they travel beside it).
 * live_out[g] (or NULL): model g's "bwd_live" word, MmsDnOpts.skip_dead_bwd.  dup_out[g] (or NULL): its "bwd_dup" word,
 * MmsDnOpts.dup_zero_bwd, from zwords[g] = the model's [B] zero-box counts (mms_conv0_fwd_group_zw) and zbps = the boxes per sample: the bit
 * mask of the samples b with zwords[g][b] == zbps whose row of dout compares equal to 0.0f in every element; 0 with fewer than two such
 * samples, B > 32, more than 16384 elements of dout, zwords[g] NULL or zbps <= 0. */
int mms_head_bwd_group_dup(const HeadBwdP* p, unsigned* const* live_out, const unsigned* const* zwords, int zbps, unsigned* const* dup_out,
                           int ng, hipStream_t s);
int mms_pool_bwd_group(const PoolBwdP* p, int ng, hipStream_t s);
int mms_conv0_bwd_weight_group(const Conv0BwdWP* p, int ng, const MmsDnOpts* opts, hipStream_t s);
int mms_pack_conv3_table_group(const void* const* tables_dev, int ng, int nlayers, hipStream_t s);
int mms_pack_conv3_table_group_ex(const void* const* tables_dev, int ng, int nlayers, uint64_t fragmask, hipStream_t s);   /* bit l set: layer l's two packs in MFMA-fragment order */
int mms_bn_running_update_group(const void* const* tables_dev, int ng, int n, float momentum, hipStream_t s);
int mms_missing_mix_fwd_group(const MixP* p, int ng, hipStream_t s);
int mms_missing_mix_bwd_group(const MixP* p, int ng, hipStream_t s);
int mms_gather_rows_group(const GatherP* p, int ng, hipStream_t s);
int mms_gather_aug_group(const GatherP* p, const AugP* a, int ng, hipStream_t s);   /* gather + per-row augmentation records */
int mms_gather_affine_group(const GatherP* p, const AugP* a, const AffP* f, int ng, hipStream_t s);   /* ... + affine resampling and noise records */
int mms_gather_elastic_group(const GatherP* p, const AugP* a, const AffP* f, const ElaP* e, int ng, hipStream_t s);   /* ... + elastic deformation records */
int mms_elastic_field(const ElaP* p, int B, int D, int H, int W, float* out, hipStream_t s);   /* the displacement field of B records, out [B][3][D][H][W] */
int mms_unpack_conv3_grads_group(const float* const* scratch, float* const* const* dw, int ng, int nlayers, hipStream_t s);  /* scratch[g]: model g's [nlayers][27][32][128] tap-major scratch; dw[g][i]: canonical gradient of layer i; nlayers <= 58 */
int mms_zero_regions_group(void* const* regions_dev, int ng, size_t bytes, hipStream_t s);   /* 16-B aligned regions of equal size, zero-filled by one launch */
int mms_linear_fwd_group(const LinearFwdP* p, int ng, hipStream_t s);
/* Precondition since the two roles of a layer share one launch: dx must not overlap dy, y or x (the weight role may still be reading them
 * while the input role writes dx; the engines keep activations and their gradients in separate buffers). */
int mms_linear_bwd_group(const LinearBwdP* p, int ng, hipStream_t s);
/* The same with the launch form chosen by the caller: 0 = what mms_linear_bwd_group does (a layer with both dw and dx: ONE launch whose
 * workgroups split into the weight and the input role); 1 = one launch per role.  Same values per element in both.  Other forms: MMS_ERR_ARG. */
int mms_linear_bwd_group_form(const LinearBwdP* p, int ng, int form, hipStream_t s);
int mms_gate_fwd_group(const GateP* p, int ng, hipStream_t s);
int mms_gate_bwd_group(const GateP* p, int ng, hipStream_t s);
int mms_cox_fwd_bwd_group(const CoxP* p, int ng, hipStream_t s);
/* The same with the launch form chosen by the caller: 0 = what mms_cox_fwd_bwd_group does (n <= 256: both passes in ONE launch of one
 * workgroup per model; larger n: two launches); 1 = always the two launches.  Same bits in lse, tie_frac, out and dh.  Other forms: MMS_ERR_ARG. */
int mms_cox_fwd_bwd_group_form(const CoxP* p, int ng, int form, hipStream_t s);
/* Zero-fill of n spans (1 <= n <= 3 * MMS_MAX_GROUP; a step's gradient buffers, sums of squares and entropy words of a fold group) by ONE
 * kernel launch -- no memset node, so the call orders like any other launch in a captured graph.  n outside the range, a NULL span pointer
 * or an empty span: MMS_ERR_ARG and nothing is launched. */
int mms_zero_spans_group(const MmsZeroSpan* spans, int n, hipStream_t s);
int mms_moe_fwd_group(const MoeP* p, int ng, hipStream_t s);   /* SimMLM heads: MoeP.stage of the forward */
int mms_moe_bwd_group(const MoeP* p, int ng, hipStream_t s);   /* ... and of the backward */
int mms_grad_sumsq_group(const AdamP* p, int ng, hipStream_t s);
/* The same with the launch form chosen by the caller: 0 = what mms_grad_sumsq_group does (where the grid of 256-thread workgroups is a
 * multiple of four -- always from 4.2 M floats on -- a quarter as many workgroups of 1024 threads: a quarter of the fp64 atomics that end
 * the launch); 1 = always 256 threads, at most 1024 workgroups.  Every thread's fp32 partial is the same in both; the sums differ by the
 * order of the fp64 additions; the bookkeeping (step, acc, rng) is the same.  Other forms: MMS_ERR_ARG. */
int mms_grad_sumsq_group_form(const AdamP* p, int ng, int form, hipStream_t s);
int mms_clip_adam_group(const AdamP* p, int ng, hipStream_t s);
int mms_w2_pack_group(const AdamP* p, int ng, hipStream_t s);
/* whole-encoder drivers: entry g of every array describes model g (arguments as mms_dn121_forward / _backward) */
int mms_dn121_forward_group(int ng, void* const* ws, int B, int D, int H, int W, const float* const* x,
                            const void* const* const* params, const void* const* const* buffers, float* const* out,
                            int ldo, int train, const MmsDnOpts* opts, hipStream_t s);
int mms_dn121_backward_group(int ng, void* const* ws, int B, int D, int H, int W, const float* const* x,
                             const void* const* const* params, const float* const* dout, int lddout,
                             void* const* const* grads, const MmsDnOpts* opts, hipStream_t s);
int mms_dn121_backward_group_from(int ng, void* const* ws, int B, int D, int H, int W, const float* const* x,
                                  const void* const* const* params, const float* const* dout, int lddout,
                                  void* const* const* grads, int block_lo, const MmsDnOpts* opts, hipStream_t s);      /* (mms_dn121_backward_from) */

/* Fallback CT encoder in lock-step (csrc/fb_group.hip): fp32-MFMA group forms of the mms_fb_* ops on the same parameter blocks.  All
 * members share one shape.  Taken: Cin = 1 (has_bn = 0) or Cin a multiple of 16 in 16..128; Cout a multiple of 16 other than 48 + 64 n (a
 * last 32-wide column tile may be half filled: masked); out = ceil(in / 2);
 * x / dy 16-byte aligned for Cin > 1; bwd_x needs has_bn; bwd_w splits the rows over FbConvP.msplit (1..1024) workgroups per tile.
 * Anything else -- ng outside 1..MMS_MAX_GROUP, a NULL pointer the op uses -- is MMS_ERR_ARG and nothing is launched. */
int mms_fb_conv_fwd_group(const FbConvP* p, int ng, hipStream_t s);
int mms_fb_conv_bwd_w_group(const FbConvP* p, int ng, hipStream_t s);
int mms_fb_conv_bwd_x_group(const FbConvP* p, int ng, hipStream_t s);
int mms_fb_pool_fwd_group(const FbPoolP* p, int ng, hipStream_t s);
int mms_fb_pool_bwd_group(const FbPoolP* p, int ng, hipStream_t s);
/* whole-encoder drivers (arguments as mms_fb_forward / _backward, one entry per member; ws[g]: mms_fb_workspace_bytes, initialised by
 * mms_fb_init).  No copies and no synchronisation: capturable into a HIP graph. */
int mms_fb_forward_group(int ng, void* const* ws, int B, int D, int H, int W, const float* const* x,
                         const void* const* const* params, const void* const* const* buffers, float* const* out,
                         int ldo, int train, hipStream_t s);
int mms_fb_backward_group(int ng, void* const* ws, int B, int D, int H, int W, const float* const* x,
                          const void* const* const* params, const float* const* dout, int lddout,
                          void* const* const* grads, hipStream_t s);
/* ... at other channel widths (arguments as mms_fb3_forward / _backward, one entry per member; widths additionally as Cout above) */
int mms_fb3_forward_group(int ng, void* const* ws, size_t ws_bytes, const int* widths, int B, int D, int H, int W, const float* const* x,
                          const void* const* const* params, const void* const* const* buffers, float* const* out,
                          int ldo, int train, hipStream_t s);
int mms_fb3_backward_group(int ng, void* const* ws, size_t ws_bytes, const int* widths, int B, int D, int H, int W, const float* const* x,
                           const void* const* const* params, const float* const* dout, int lddout,
                           void* const* const* grads, hipStream_t s);
/* ImageOnlyModel's tail in one launch per pass: BN3 + ReLU + global average pool -> Linear + ReLU -> Linear.  The arguments are the blocks of
 * the three launches it replaces, one of each per member: pool (y, bn, C <= 128, V, B <= 32, out / ldo = the pooled features), l1 reading
 * pool.out (K = C, N <= 64, out_relu = 1, no prologue), l2 reading l1.y (N <= 8, out_relu = 0).  Backward: l2.dy = dL/dhazard; accumulates
 * l1 / l2 .dw / .dbias (one workgroup per member owns them: no float atomics), writes pool.dbn and adds pool.s1 / s2 as
 * mms_fb_pool_bwd_group does; pool.dout and the Linear blocks' dx are not used.  Blocks that are not such a chain: MMS_ERR_ARG. */
int mms_img_tail_fwd_group(const FbPoolP* pool, const LinearFwdP* l1, const LinearFwdP* l2, int ng, hipStream_t s);
int mms_img_tail_bwd_group(const FbPoolP* pool, const LinearBwdP* l1, const LinearBwdP* l2, int ng, hipStream_t s);
/* mms_fb3_forward_group / _backward_group with that tail in place of the pool launch (out / ldo: where the pooled features go = l1.x) */
int mms_img_forward_group(int ng, void* const* ws, size_t ws_bytes, const int* widths, int B, int D, int H, int W, const float* const* x,
                          const void* const* const* params, const void* const* const* buffers, float* const* out,
                          int ldo, int train, const LinearFwdP* l1, const LinearFwdP* l2, hipStream_t s);
int mms_img_backward_group(int ng, void* const* ws, size_t ws_bytes, const int* widths, int B, int D, int H, int W, const float* const* x,
                           const void* const* const* params, void* const* const* grads, const LinearBwdP* l1, const LinearBwdP* l2,
                           hipStream_t s);

#ifdef __cplusplus
}
#endif
#endif /* MMSURV_H */
