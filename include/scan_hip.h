/*
 * scan_hip.h -- C ABI of libscan_hip.so, the MI355X (gfx950) hot path of the
 * SCAN FCOS-based domain-adaptive detector.
 *
 * Every entry point takes plain device pointers + sizes and a HIP stream
 * (void* == hipStream_t; NULL = the null stream).  Nothing here allocates,
 * frees or synchronises unless stated, so calls are graph-capturable.
 * Return value: 0 on success, <0 on error (scan_last_error() gives the text;
 * the Python host raises RuntimeError, mirroring the reference's AT_ASSERTM /
 * AT_ERROR -> RuntimeError behaviour, csrc/nms.h:10-28, csrc/SigmoidFocalLoss.h:10-41).
 *
 * Layout convention ("pyramid"): an activation is a row-major fp32 matrix
 * [M, C] whose rows are pixels in level-major, then image, then y, then x
 * order -- exactly the order the reference flattens to before its losses
 * (rpn/fcos/loss.py:191-202, condgraph.py:348-351).  A scan_pyramid_t says how
 * the rows split into levels.  A plain NHWC tensor is a pyramid with 1 level.
 *
 * Each function cites the reference interface it replaces
 * (paths relative to the reference checkout, fcos_core/...).
 */
#ifndef SCAN_HIP_H
#define SCAN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SCAN_MAX_LEVELS 5

typedef struct {
  int32_t n_levels;              /* 1..5 */
  int32_t n_images;              /* N */
  int32_t h[SCAN_MAX_LEVELS];    /* per-level height */
  int32_t w[SCAN_MAX_LEVELS];    /* per-level width  */
  int64_t row_off[SCAN_MAX_LEVELS + 1]; /* first row of each level; row_off[n_levels] = M */
} scan_pyramid_t;

const char* scan_last_error(void);
/* changes when an existing declaration changes its meaning; declarations that are only added leave it as it is */
int scan_abi_version(void);

/* Tuning knob for A/B measurements and tests (no reference counterpart): scan_tune(key, value) sets an integer
 * launch-selection parameter and returns its previous value, SCAN_TUNE_UNKNOWN for an unknown key.  Every setting of every
 * key gives correct results (timing-ablation instances are not part of this library).
 *   "conv_bn256"  3x3 convs whose output channels are a multiple of 256 -- 2 (default): 256-channel tiles whenever they do
 *                 not cost a round of 256 CUs against 128-channel tiles (a 256-channel workgroup runs twice as long); 1: when
 *                 the launch keeps >= 2 workgroups per CU (rounds 2-4); 0: always 128-channel tiles.  Same results bit for bit.
 *   "conv_v2"     1 (default): bf16x3 forward / data-gradient convs run on the v_mfma_f32_16x16x32_bf16 kernel
 *                 (csrc/conv_fwd.hip); 0: on the independent v_mfma_f32_32x32x16_bf16 kernel kept for cross-checks
 *                 (csrc/conv_gen1.hip; same arithmetic, different summation order inside a 32-channel chunk).
 *   "conv_wg1024" (bf16x3) 1 (default): the 128- / 256-channel forward / dgrad instances run 16 waves per workgroup; 0: 8
 *                 waves; 2: 16 waves only for the 256-channel tile on multi-level pyramids.  Same results bit for bit.
 *   "conv_w8"     (bf16x3) 1 (default): the 256-channel LDS-DMA forward / dgrad tile runs on 8 waves (64 px x 128 ch per
 *                 wave); 0: 16 waves.  Same results bit for bit.
 *   "conv_tpb3"   (bf16x3) bit 0 (default on) / bit 1: the 128- / 64-channel instance stages three taps per barrier (same
 *                 results bit for bit).
 *   "conv_bn64_th16" pixel tile of convs with <= 64 output channels on single-level pyramids: 0: 8x16; 1: 16x16 when the
 *                 sizes are multiples of 16; 2 (default): bf16x6 additionally takes 32x16 when H is a multiple of 32.  Same
 *                 results bit for bit.
 *   "conv_glds"   1 (default): the 128- / 256-channel 3x3 instances stage weight tiles by LDS-DMA (buffer_load ... lds) on
 *                 whole tiles; 0: through registers.  Same results bit for bit.
 *   "conv1x1"     bf16x6 1x1 convs (FPN laterals, ResNet bottlenecks): bit 0 = weight tiles by LDS-DMA, bit 1 = the 256-channel tile
 *                 when the output channels fill it without costing a round; 3 (default), 0 = rounds 4-5's 128-channel register-staged
 *                 instance.  Same results bit for bit.
 *   "wgrad_v6"    1 (default): the 3x3 weight-gradient launches take the producer / consumer kernel (12 waves: 8 issue
 *                 MFMAs, 4 stage); 0: the kernel in which all 8 waves stage and multiply in turn (always used by the 1x1
 *                 convs).  bf16x3: bit-identical; bf16x6: other K-chunk length, i.e. other split-K boundaries.
 *   "wgrad_prio"  1: the producer waves of that kernel run at s_setprio 3; 0 (default): at the consumers' priority.  Same
 *                 results bit for bit.
 *   "wgrad_tile"  consumer wave tile of that kernel: 0 = 64 (o) x 32 (c), 1 = 32 (o) x 64 (c), 2 (default, and any other value) = 1
 *                 for bf16x6, 0 for bf16x3.  bf16x3: same results bit for bit.  bf16x6: 1 sums the six piece products of a
 *                 32-pixel step in a temporary first (one rounding per step at the accumulator's magnitude, DESIGN.md 3.0:
 *                 0.23-0.5x the fp32-MFMA kernel's distance from fp64); 0 adds them straight into the running accumulator (an
 *                 fp32 sum in another order, 1.0-2.1x that distance; the golden suite is green on it, 4-5 % faster on random
 *                 operands, no faster in the training step: profiles/r06_wgrad_tile_ab.txt).
 *   "wgrad_wgs"   768 (default): workgroups a weight-gradient launch aims at (tiles x split-K slabs); 512 / 640 / 896 / 1024
 *                 / 1280 / 1536 are 2...25 % slower on the 256- and 512-channel layers (bf16x3).
 *   "wgrad_wino"  1 (default): the bf16x6 3x3 weight gradient on that kernel's 32 x 64 tile runs Winograd F(2,3) across rows:
 *                 the K walk goes over row pairs, a workgroup owns one of four components instead of one of three ky, a third
 *                 fewer MFMAs; transforms in fp32 on the loaded rows (one rounding per value), G^T on the fp64 slab sums.
 *                 Slabs then hold 12 taps.  scan_conv_wgrad_plan reads the knob once and scan_conv_wgrad_run runs what was
 *                 planned, whatever the knob says by then; only the older pair -- scan_conv3x3_wgrad_bf16x6_ws_floats, then
 *                 scan_conv3x3_wgrad_bf16x6 -- reads it twice: there, size the workspace AFTER setting it.  0: the direct
 *                 kernel and split-K plan, bit for bit.  bf16x3, wgrad_v6 = 0 and wgrad_tile = 0 are always direct.
 *   "wino_tpb"    (bf16x6, next to "conv_wino": the Winograd F(2,3) forward / data-gradient instance, scan_conv3x3_wino_bf16x6)
 *                 weight taps per barrier interval: 2 (default) = the patch is staged in component pairs and the LDS that frees
 *                 holds two taps per weight buffer -- 8 barriers per 32-channel chunk, 96 MFMAs per wave between them; 1 (and
 *                 any other value) = one tap per interval, 13 barriers per chunk.  Same results bit for bit
 *                 (tests/test_gpu_wino_schedule.py); the GroupNorm sums agree up to the order of their fp64 atomics.
 *   "gconv_mfma"  0 (default): the grouped class-branch conv runs on fp32 FMAs; 1: tap products and data gradient on the
 *                 fp32 matrix cores (same products, different summation order; measured no faster in the step).
 *   "reduce_blocks" 2048 (default): most workgroups a loss-reduction kernel is launched with (each ends in one or two float
 *                 atomics on one cache line); the IoU and CKA forward kernels take half of it.  Same sums up to the order of
 *                 the atomics.
 *   "dbscan_bf16x3" 1 (default): scan_dbscan_prepare's pairwise-distance GEMM runs as bf16x3 with a wider exact re-check
 *                 band; 0: exact fp32 matrix cores.  Same neighbour bits (pairs inside the band are decided in fp64).
 *   "deterministic" 0 (default): the callers of this library (scan_amd.ops, scan_amd.layers, the compiled scan_ops module) use
 *                 the atomic loss / GroupNorm reductions; 1: they call the *_ordered entry points below and take GroupNorm
 *                 statistics from scan_groupnorm_stats_ordered instead of a conv epilogue, so that a training step is
 *                 reproducible bit for bit.  The library stores this knob and reads it in ONE place, scan_groupnorm_plan, which
 *                 answers an ordered plan with it on: NO other entry point changes its signature or its behaviour with it, a
 *                 C caller chooses by the symbol it calls. */
#define SCAN_TUNE_UNKNOWN (-2147483647 - 1)
int scan_tune(const char* key, int value);
/* read-only: the current value of a knob (nothing is written), SCAN_TUNE_UNKNOWN for an unknown key */
int scan_tune_get(const char* key);
/* the value the library was built with; scan_tune_key(i): name of the i-th knob, NULL past the end (bench.py stamps every
 * knob that differs from its default into the line it prints) */
int scan_tune_default(const char* key);
const char* scan_tune_key(int index);

/* Measurement (no reference counterpart): the bf16 matrix-pipe rate this board sustains under its package power cap -- a
 * register-only v_mfma_f32_16x16x32_bf16 loop on every CU for about `seconds` (<= 30), two waves per SIMD; random != 0:
 * random-sign / random-mantissa operands, 0: zeros.  Writes TFLOP/s; blocking (synchronises `stream`).  bench.py reports
 * it as roofline.board_sustained beside the fraction of the nominal 2.5 PFLOP/s. */
int scan_mfma_sustained_bf16(double seconds, int32_t random, double* tflops, void* stream);

/* Measurement (no reference counterpart; what it stands in for: the RCCL ring all-reduce the data-parallel step issues where the
 * reference's DistributedDataParallel does, tools/train_net_da.py:421-515): one rank's footprint of an all-reduce of
 * buf[0, n_floats) -- `wgs` workgroups of 256 threads (RCCL: one per channel) that read-modify-write (x * 1.0f: values
 * unchanged) their slice `traffic` times (ring: 2 (N - 1) / N), paced to `gbps` aggregate read rate by sleeping on the wall
 * clock (0 = unpaced).  Asynchronous on `stream`.  tools/dp_emulate.py runs it where the gradient buckets fire. */
int scan_comm_standin(float* buf, int64_t n_floats, double traffic, int32_t wgs, double gbps, void* stream);

/* Output-channel tile (64, 128 or 256) the bf16x3 3x3 kernel uses for a launch on pyramid d with Nout channels;
 * 1128 / 1256 = the 128- / 256-channel tile on 16-wave workgroups, 2256 = the 256-channel tile on the 8-wave LDS-DMA instance. */
int scan_conv3x3_bf16x3_instance(const scan_pyramid_t* d, int32_t Nout);
/* the same for a bf16x6 1x1 launch on output pyramid yd with Nout channels and weight-plane row length Csw: 64 / 128 = register-staged
 * tiles, 1128 / 1256 = the 128- / 256-channel tile with LDS-DMA weight tiles (scan_tune "conv1x1") */
int scan_conv1x1_bf16x6_instance(const scan_pyramid_t* yd, int32_t Nout, int32_t Csw);

/* ---- SigmoidFocalLoss  (replaces _C.sigmoid_focalloss_forward / _backward,
 *      csrc/SigmoidFocalLoss.h:10-41, csrc/cuda/SigmoidFocalLoss_cuda.cu:20-187) ----
 * logits [M,C] fp32, targets [M] int32 (0 = bg, c = class c, <0 = ignore).
 * losses may be NULL; loss_sum (1 float, pre-zeroed by caller) may be NULL:
 * when given, the wavefront-reduced total is atomically added to it, which is
 * what layers/sigmoid_focal_loss.py:56-70 (`loss.sum()`) consumes.
 * Any 4-byte aligned pointer is accepted: the float4 forms run only when M*C is a multiple of 4 and logits, losses, d_losses
 * and d_logits (those given) are all 16-byte aligned; otherwise the scalar form of the same arithmetic. */
int scan_sigmoid_focal_loss_forward(const float* logits, const int32_t* targets, int64_t M, int32_t C,
                                    float gamma, float alpha, float* losses, float* loss_sum, void* stream);
/* d_losses [M,C] or NULL; when NULL every element uses d_scale (the fused
 * `sum()/(num_pos+N)` backward, rpn/fcos/loss.py:204-208). */
int scan_sigmoid_focal_loss_backward(const float* logits, const int32_t* targets, const float* d_losses,
                                     float d_scale, int64_t M, int32_t C, float gamma, float alpha,
                                     float* d_logits, void* stream);

/* ---- IOULoss (replaces layers/iou_loss.py:5-36) ----
 * pred/target [P,4] (l,t,r,b), weight [P] or NULL.  out[0] += sum(loss*w),
 * out[1] += sum(w) (w = 1 when NULL); caller pre-zeroes out[2] and divides.  The reference takes the weighted mean only
 * when sum(w) > 0 and the plain mean otherwise: a caller that may see such a weight also asks for the unweighted pair
 * (weight = NULL) and selects on out[1] (scan_amd.ops.iou_loss does, on the device).  pred / target: 16-byte aligned. */
int scan_iou_loss_forward(const float* pred, const float* target, const float* weight, int64_t P,
                          float* out2, void* stream);
/* d_pred[i,:] = g_num * w_i * dloss_i/dpred  with g_num = upstream / sum(w) read from g_num_dev[0]. */
int scan_iou_loss_backward(const float* pred, const float* target, const float* weight, int64_t P,
                           const float* g_num_dev, float* d_pred, void* stream);

/* ---- BCE-with-logits, optionally weighted (replaces F.binary_cross_entropy_with_logits as used by
 *      discriminator/fcos_head_discriminator_con.py:117-123 and rpn/fcos/loss.py:221-224) ----
 * logits [M] (stride 1), weight element i at weight[i*w_stride] or NULL, constant target.
 * out[0] += sum(w * bce), out[1] += sum(w). */
int scan_bce_logits_forward(const float* logits, const float* targets, float const_target,
                            const float* weight, int64_t w_stride, int64_t M, float* out2, void* stream);
/* d_logits[i] = g_dev[0] * w_i * (sigmoid(x_i) - t_i) */
int scan_bce_logits_backward(const float* logits, const float* targets, float const_target,
                             const float* weight, int64_t w_stride, int64_t M, const float* g_dev,
                             float* d_logits, void* stream);

/* ---- CKA class-conditional adversarial loss (replaces the per-class loop of
 *      discriminator/fcos_head_discriminator_con.py:105-124, num_classes > 1 branch) ----
 * logits [M,Cf] (one column per foreground class), act [M,Cf+1] softmax maps (column 0 = background),
 * constant domain target t.  out[2*c] += sum_m act[m][c+1]*bce(logits[m][c], t), out[2*c+1] += sum_m act[m][c+1].
 * The host forms  sum_c (out[2c]/out[2c+1]) / Cf.   Cf <= 16. */
int scan_cka_bce_forward(const float* logits, const float* act, int64_t M, int32_t Cf, float target, float* out,
                         void* stream);
/* d_logits[m][c] = g_dev[c] * act[m][c+1] * (sigmoid(x) - t),  g_dev[c] = upstream / (Cf * sum_w[c]) */
int scan_cka_bce_backward(const float* logits, const float* act, int64_t M, int32_t Cf, float target,
                          const float* g_dev, float* d_logits, void* stream);
/* The same pair with the layer's scalar arithmetic folded in: out = 2 * Cf + 2 floats zeroed by the caller (sums, a ticket
 * word, the loss  sum_c (num_c / den_c) / Cf  written by the block that finishes last); the backward takes the gradient
 * of that scalar (g_loss [1], device) and the forward's out and forms the per-class coefficients itself. */
int scan_cka_bce_forward_loss(const float* logits, const float* act, int64_t M, int32_t Cf, float target, float* out,
                              void* stream);
int scan_cka_bce_backward_loss(const float* logits, const float* act, int64_t M, int32_t Cf, float target,
                               const float* g_loss, const float* sums, float* d_logits, void* stream);

/* ---- Ordered forms of this header's loss reductions -- sigmoid focal, IoU, BCE, CKA BCE, softmax focal (no reference counterpart; the reference gets run-to-run equality from
 *      cudnn.deterministic + its seeds, tools/train_net_da.py setup_seed) ----
 * The entry points above end in one float atomic per workgroup: their sums depend on the order the workgroups finish in
 * (~1e-7 relative between two runs).  Each *_ordered twin computes the same sums from the same kernel compiled with the
 * atomics replaced: workgroup b stores its partial sums to slot ws[b][...] (ordinary stores), and a one-workgroup launch
 * behind it adds the slots in a fixed order (lane l of a wave adds slots l, l + 64, ... ascending, the 64 lane sums go
 * through a fixed shuffle tree) and writes -- not adds -- the result where the atomic form leaves it; the CKA loss form
 * also writes out[2 Cf + 1], its ticket word out[2 Cf] is left alone.  The result is a function of the inputs, the shape
 * and scan_tune "reduce_blocks" only.  ws: at least the matching *_ordered_ws_floats floats (asked under the knob values
 * the launch runs with), one per call in flight, need not be cleared; M == 0 / P == 0 leave out as it is, so clear it as
 * for the atomic form.  All other arguments as the twin; scan_sigmoid_focal_loss_forward_ordered requires loss_sum. */
int64_t scan_sigmoid_focal_loss_ordered_ws_floats(int64_t M, int32_t C);
int scan_sigmoid_focal_loss_forward_ordered(const float* logits, const int32_t* targets, int64_t M, int32_t C,
                                            float gamma, float alpha, float* losses, float* loss_sum, float* ws,
                                            void* stream);
int64_t scan_iou_loss_ordered_ws_floats(int64_t P);
int scan_iou_loss_forward_ordered(const float* pred, const float* target, const float* weight, int64_t P, float* out2,
                                  float* ws, void* stream);
int64_t scan_bce_logits_ordered_ws_floats(int64_t M);
int scan_bce_logits_forward_ordered(const float* logits, const float* targets, float const_target, const float* weight,
                                    int64_t w_stride, int64_t M, float* out2, float* ws, void* stream);
int64_t scan_cka_bce_ordered_ws_floats(int64_t M, int32_t Cf);
int scan_cka_bce_forward_ordered(const float* logits, const float* act, int64_t M, int32_t Cf, float target, float* out,
                                 float* ws, void* stream);
int scan_cka_bce_forward_loss_ordered(const float* logits, const float* act, int64_t M, int32_t Cf, float target,
                                      float* out, float* ws, void* stream);
int64_t scan_softmax_focal_ordered_ws_floats(int64_t M);
int scan_softmax_focal_forward_ordered(const float* logits, const int64_t* labels, int64_t M, int32_t K, float gamma,
                                       float* loss_sum, float* ws, void* stream);

/* ---- y = alpha * x  (GradientReversalFunction: forward alpha = 1 copy, backward alpha = -lambda;
 *      discriminator/layer.py:6-24).  x and y are flat fp32 ranges with any 4-byte alignment (a level's rows of an [M, 9]
 *      matrix); y == x is allowed.  Both 16-byte aligned: the float4 kernel; otherwise one float per lane, the same bits. ---- */
int scan_scale(const float* x, float alpha, float* y, int64_t n, void* stream);
/* dst[r][c] = src[r][c] for c < ncols, zeros for ncols <= c < ncols + ztail; row pitches ld_src / ld_dst in floats (callers
 * offset the pointers to the first column).  Replaces the torch-tier spellings of F.pad(act_maps, (0, 3)) in front of head_out's
 * act-map share (rpn/fcos/condgraph.py:344-362: cat(features, act_maps)) and of cat(x, act_maps[:, 1:]) in front of the class
 * branches (discriminator/fcos_head_discriminator_con.py:104-118). */
int scan_copy_cols(const float* src, int32_t ld_src, float* dst, int32_t ld_dst, int64_t M, int32_t ncols, int32_t ztail,
                   void* stream);
/* GRAPHModule.update_prototype_nx1_rnn with COSINE_UPDATE_ON (rpn/fcos/condgraph.py:586-606) on the paradigm buffer P [K][C][T]
 * in place: slot = it - 1 if it == T else it; m = cosine_similarity(P[:, :, slot], pb); P[:, :, slot] <- cur * m + pb * (1 - m) for the
 * classes whose batch mean pb [K][C] is not all zero; it == T shifts the slots down by one first.  C <= 1024. */
int scan_paradigm_update(float* P, const float* pb, int32_t K, int32_t C, int32_t T, int32_t it, void* stream);

/* ---- semantic-conditioned dynamic 1x1 conv + channel softmax
 *      (replaces GRAPHModule.dynamic_conv + softmax, rpn/fcos/condgraph.py:619-629, 344-346) ----
 * feat [M,C] (C == 256), kernels [K,C] (2 <= K <= scan_dynconv_max_classes() = 32) -> logits [M,K], probs [M,K].
 * K = 2 and K = 9 run kernels compiled for that K; every other K runs the generic ones (scan_tune "dynconv_generic" = 1:
 * every K does).  A K outside the range is an argument error naming it; nothing is launched. */
int32_t scan_dynconv_max_classes(void);
int scan_dynconv_softmax_forward(const float* feat, const float* kernels, int64_t M, int32_t C, int32_t K,
                                 float* logits, float* probs, void* stream);
/* d_logits_in [M,K] or NULL (grad arriving at the logits, e.g. from the act loss), d_probs [M,K] or NULL.
 * Writes d_feat [M,C] (overwrites) and d_kernels [K,C] (overwrites; uses ws of size >= grid*K*C floats,
 * see scan_dynconv_ws_floats).  M == 0 is legal in both directions: the forward launches nothing, the backward only clears
 * d_kernels (the other pointers are not looked at). */
int64_t scan_dynconv_ws_floats(int64_t M, int32_t C, int32_t K);
int scan_dynconv_softmax_backward(const float* feat, const float* kernels, const float* probs,
                                  const float* d_logits_in, const float* d_probs, int64_t M, int32_t C,
                                  int32_t K, float* d_feat, float* d_kernels, float* ws, void* stream);

/* ---- softmax focal loss of the activation maps (replaces layers/sigmoid_focal_loss_wbg.py:38-64,
 *      alpha = 1, gamma = 2, mean over rows) ----
 * logits [M,K], labels int64 [M]; loss_sum[0] += sum_i -(1-p_i)^g log p_i  (caller divides by M). */
int scan_softmax_focal_forward(const float* logits, const int64_t* labels, int64_t M, int32_t K, float gamma,
                               float* loss_sum, void* stream);
int scan_softmax_focal_backward(const float* logits, const int64_t* labels, int64_t M, int32_t K, float gamma,
                                float d_scale, float* d_logits, void* stream);

/* ---- NMS (replaces _C.nms, csrc/nms.h:10-28, csrc/cpu/nms_cpu.cpp:5-65, csrc/cuda/nms.cu:23-131;
 *      and _C.ml_nms, csrc/ml_nms.h:10-27, csrc/cuda/ml_nms.cu:13-136) ----
 * dets [n,4] xyxy, scores [n], labels [n] float or NULL (NULL = plain nms).
 * rule_ge != 0: suppress when IoU >= thr (the CPU rule, nms_cpu.cpp:60 -- the oracle);
 * rule_ge == 0: suppress when IoU >  thr (the CUDA rule, nms.cu:60).
 * keep_out [n] int64 receives the kept ORIGINAL indices ascending, num_keep_out[0] their count
 * (both device memory).  workspace: scan_nms_ws_bytes(n) bytes (n <= SCAN_NMS_PANEL: ~n*n/8 + 64 KB; the mask of a
 * larger n is n * ceil(n/64) * 8 bytes, the size of the reference's own, cuda/nms.cu:95-100).
 * n <= SCAN_NMS_PANEL runs as three single-workgroup-chain launches (the post-processor's case: <= 5,000 candidates per
 * image); a larger n (nms_cuda has no limit, cuda/nms.cu:70-131) takes the panel path, up to SCAN_NMS_MAX -- a bound on
 * the chain state one workgroup keeps in LDS (two bit words per 64 candidates), not on the algorithm. */
#define SCAN_NMS_PANEL 8192
#define SCAN_NMS_MAX 262144
int64_t scan_nms_ws_bytes(int64_t n);
int scan_nms(const float* dets, const float* scores, const float* labels, int64_t n, float thr, int32_t rule_ge,
             int64_t* keep_out, int32_t* num_keep_out, void* workspace, void* stream);

/* ---- convolution as fp32-MFMA implicit GEMM (replaces nn.Conv2d / F.conv2d at the call sites of
 *      backbone/mmdetection/vgg.py:8-33, backbone/fpn.py:52-66,118-130,
 *      rpn/fcos/condgraph.py:86-106, rpn/fcos/fcos.py:25-64, discriminator/fcos_head_discriminator_con.py:20-62) ----
 * x: pyramid [Mi, Cin_s] (row stride Cin_s floats, Cin_s % 4 == 0, channels >= Cin are zero padding)
 * w: [Cout][k*k][Cin_s] fp32 ("OHWI", what a channels_last torch weight is physically)
 * y: pyramid [Mo, Cout_s]; bias [Cout] or NULL; relu != 0 fuses max(0,.).
 * ksize in {1,3,5,7}; stride in {1,2}; pad = ksize/2. */
int scan_conv2d_forward(const float* x, const scan_pyramid_t* xd, int32_t Cin_s, const float* w, const float* bias,
                        float* y, const scan_pyramid_t* yd, int32_t Cout, int32_t Cout_s, int32_t ksize,
                        int32_t stride, int32_t relu, void* stream);
/* dX = conv_transpose(dY, W).  wt: [Cin][k*k][Cout_s] (the transposed copy made by scan_weight_transpose).
 * mask (optional, same shape as dx): dx is zeroed where mask <= 0 (ReLU backward of the producer). */
int scan_conv2d_dgrad(const float* dy, const scan_pyramid_t* yd, int32_t Cout_s, const float* wt, float* dx,
                      const scan_pyramid_t* xd, int32_t Cin, int32_t Cin_s, int32_t ksize, int32_t stride,
                      const float* mask, void* stream);
/* dW[Cout][k*k][Cin_s] = sum_m dY[m][o] * X[tap(m)][c]; deterministic split-K through ws
 * (scan_conv2d_wgrad_ws_floats) followed by an in-order reduction.  accumulate != 0: dW += result. */
int64_t scan_conv2d_wgrad_ws_floats(const scan_pyramid_t* yd, int32_t Cin_s, int32_t Cout, int32_t ksize);
int scan_conv2d_wgrad(const float* x, const scan_pyramid_t* xd, int32_t Cin_s, const float* dy,
                      const scan_pyramid_t* yd, int32_t Cout, int32_t Cout_s, int32_t ksize, int32_t stride,
                      float* dw, int32_t accumulate, float* ws, void* stream);
/* ---- 3x3 / stride-1 convolution with fp32-grade accuracy on the bf16 matrix cores ("bf16x3": every fp32
 *      operand is split hi + lo into two bf16 values; hi*hi + hi*lo + lo*hi accumulated in fp32).  Same call
 *      sites as scan_conv2d_forward; ~5x the fp32-MFMA rate.
 * scan_weight_split: w [O][T][Cs] fp32 -> bf16 planes wh, wl.
 *    mode 0: [O][T][Csw]   (forward);   mode 1: [Cs][T][Csw] holding w[o][T-1-t][c] at [c][t][o] (dgrad).
 *    Csw % 8 == 0, zero padded.
 * scan_conv3x3_bf16x3: y[M][Ns] = conv3x3_s1(x[M][Cs], w) + bias, optional ReLU, optional mask (y = 0 where
 *    mask <= 0).  The data gradient is the same call on dY with the mode-1 weights. */
int scan_weight_split(const float* w, int32_t O, int32_t T, int32_t Cs, int32_t mode, void* wh, void* wl,
                      int32_t Csw, void* stream);
int scan_conv3x3_bf16x3(const float* x, const scan_pyramid_t* d, int32_t Cs, const void* wh, const void* wl,
                        int32_t Csw, const float* bias, const float* mask, float* y, int32_t Nout, int32_t Ns,
                        int32_t relu, void* stream);
/* 1x1 convolutions (FPN laterals backbone/fpn.py:52-66; ResNet bottleneck conv1 / conv3 / downsample,
 * backbone/resnet.py:228-314, incl. the stride-2 ones: STRIDE_IN_1X1) on the same bf16x3 kernel (one tap, no halo).
 * wh/wl: scan_weight_split planes with T = 1 (mode 0 forward, mode 1 data gradient).  map 0: stride 1 (xd == yd);
 * map 1: stride-2 forward (yd = ceil(xd / 2)); map 2: data gradient of a stride-2 1x1 conv (x = dY on the coarse
 * pyramid xd, y = dX on the fine pyramid yd, zero where a coordinate is odd).  mask as in scan_conv3x3_bf16x3. */
int scan_conv1x1_bf16x3(const float* x, const scan_pyramid_t* xd, int32_t Cs, const void* wh, const void* wl,
                        int32_t Csw, const float* bias, const float* mask, float* y, const scan_pyramid_t* yd,
                        int32_t Nout, int32_t Ns, int32_t relu, int32_t map, void* stream);
/* weight gradient of a 1x1 conv (stride 1 or 2): dw [Cout][1][Cs] (+)= dY^T X over all pixels of the dY pyramid yd; x on
 * xd (yd = ceil(xd / stride)); db / accumulate / ws as for scan_conv3x3_wgrad_bf16x3. */
int64_t scan_conv1x1_wgrad_bf16x3_ws_floats(const scan_pyramid_t* yd, int32_t Cs, int32_t Cout);
int scan_conv1x1_wgrad_bf16x3(const float* x, const scan_pyramid_t* xd, int32_t Cs, const float* dy,
                              const scan_pyramid_t* yd, int32_t Cout, int32_t Cout_s, int32_t stride, float* dw,
                              float* db, int32_t accumulate, float* ws, void* stream);
/* first-layer convolutions (3 input channels stored as 4; forward only, both live in frozen stages): the ResNet stem
 * 7x7 / stride 2 / pad 3 (backbone/resnet.py:316-336) and VGG conv1_1 3x3 / stride 1 / pad 1
 * (backbone/mmdetection/vgg.py:8-33).  x [N,H,W,4] NHWC rows, w [Cout][k*k][4] fp32, Cout <= 64,
 * y [N,Ho,Wo,Cout_s]; bf16x3 product, optional bias and ReLU. */
int scan_conv_smallcin_bf16x3(const float* x, int32_t N, int32_t H, int32_t W, const float* w, const float* bias,
                              float* y, int32_t Cout, int32_t Cout_s, int32_t ksize, int32_t stride, int32_t relu,
                              void* stream);
/* conv3x3 + bias whose 256-channel output feeds GroupNorm(32, 256) (the [conv, GN, ReLU] towers of condgraph.py:86-106,
 * fcos.py:25-49, fcos_head_discriminator_con.py:20-34): the epilogue also accumulates the GroupNorm sums into gn_ws
 * (8-byte aligned, n_levels * N * 32 * 2 fp64 values, zeroed by the call); scan_groupnorm_stats_from_sums turns them into
 * the (mean, rstd) table scan_groupnorm_stats would have produced. */
int scan_conv3x3_gn_bf16x3(const float* x, const scan_pyramid_t* d, int32_t Cs, const void* wh, const void* wl,
                           int32_t Csw, const float* bias, float* y, int32_t Nout, int32_t Ns, float* gn_ws,
                           void* stream);
/* The same with the sums ADDED to gn_ws as it stands: the caller has cleared it (one memset per training iteration over a
 * buffer all such workspaces are slices of, instead of one memset launch per call). */
int scan_conv3x3_gn_acc_bf16x3(const float* x, const scan_pyramid_t* d, int32_t Cs, const void* wh, const void* wl,
                               int32_t Csw, const float* bias, float* y, int32_t Nout, int32_t Ns, float* gn_ws,
                               void* stream);
int scan_groupnorm_stats_from_sums(const float* ws, const scan_pyramid_t* d, int32_t C, int32_t G, float eps,
                                   float* stats, void* stream);
/* conv3x3 + bias (+ ReLU) + nn.MaxPool2d(2, 2) in one launch (last conv of a FROZEN VGG stage, vgg.py:8-33: forward only):
 * single-level pyramid d with even H, W; y [N, H/2, W/2, Ns]. */
int scan_conv3x3_pool2_bf16x3(const float* x, const scan_pyramid_t* d, int32_t Cs, const void* wh, const void* wl,
                              int32_t Csw, const float* bias, float* y, int32_t Nout, int32_t Ns, int32_t relu,
                              void* stream);
/* weight gradient of the same conv, bf16x3 on the matrix cores, deterministic split-K through ws
 * (scan_conv3x3_wgrad_bf16x3_ws_floats floats).  dw [Cout][9][Cs]; db [Cout] or NULL = bias gradient (column
 * sums of dy, fused); accumulate != 0: dw += result, db += result. */
int64_t scan_conv3x3_wgrad_bf16x3_ws_floats(const scan_pyramid_t* d, int32_t Cs, int32_t Cout);
int scan_conv3x3_wgrad_bf16x3(const float* x, const scan_pyramid_t* d, int32_t Cs, const float* dy, int32_t Cout,
                              int32_t Cout_s, float* dw, float* db, int32_t accumulate, float* ws, void* stream);
/* ---- the same convolutions at the reference's arithmetic on the bf16 matrix cores ("bf16x6") ----
 * The reference multiplies fp32 by fp32 and accumulates in fp32 (torch.nn.Conv2d: backbone/mmdetection/vgg.py:8-33,
 * backbone/fpn.py:52-66, rpn/fcos/condgraph.py:86-106, rpn/fcos/fcos.py:25-64,
 * discriminator/fcos_head_discriminator_con.py:20-62).  Here every fp32 operand is cut into THREE bf16 pieces
 * hi + mid + lo -- 8 + 8 + 8 = all 24 significand bits, the split is exact -- and a product is accumulated in fp32 from the
 * six piece products hi*lo, mid*mid, lo*hi, hi*mid, mid*hi, hi*hi (smallest first); the three dropped products are
 * <= 2^-23 of the product, below the rounding of the fp32 accumulation itself.  bf16 x bf16 is exact in fp32, so the result
 * is an fp32 convolution up to summation order: measured against an fp64 convolution it is as close as the exact
 * v_mfma_f32_32x32x2_f32 kernels of scan_conv2d_* (tests/test_gpu_kernels.py::test_conv_error_vs_fp64), on a pipe whose
 * ceiling is 2.5 PFLOP/s / 6 = 417 TFLOP/s fp32-equivalent instead of 157.
 * Arguments as for the _bf16x3 functions with a third plane: wh / wm / wl = scan_weight_split3 planes (same layout and
 * modes as scan_weight_split, plus the Winograd modes 2 / 3 below).  y and mask must be 16-byte aligned, Ns % 4 == 0.
 * scan_conv3x3_gn_bf16x6: clear != 0 zeroes gn_ws first (scan_conv3x3_gn_bf16x3), 0 adds to it (.._gn_acc_bf16x3). */
int scan_weight_split3(const float* w, int32_t O, int32_t T, int32_t Cs, int32_t mode, void* wh, void* wm, void* wl,
                       int32_t Csw, void* stream);
int scan_conv3x3_bf16x6(const float* x, const scan_pyramid_t* d, int32_t Cs, const void* wh, const void* wm,
                        const void* wl, int32_t Csw, const float* bias, const float* mask, float* y, int32_t Nout,
                        int32_t Ns, int32_t relu, void* stream);
int scan_conv1x1_bf16x6(const float* x, const scan_pyramid_t* xd, int32_t Cs, const void* wh, const void* wm,
                        const void* wl, int32_t Csw, const float* bias, const float* mask, float* y,
                        const scan_pyramid_t* yd, int32_t Nout, int32_t Ns, int32_t relu, int32_t map, void* stream);
int scan_conv3x3_gn_bf16x6(const float* x, const scan_pyramid_t* d, int32_t Cs, const void* wh, const void* wm,
                           const void* wl, int32_t Csw, const float* bias, float* y, int32_t Nout, int32_t Ns,
                           float* gn_ws, int32_t clear, void* stream);
int scan_conv3x3_pool2_bf16x6(const float* x, const scan_pyramid_t* d, int32_t Cs, const void* wh, const void* wm,
                              const void* wl, int32_t Csw, const float* bias, float* y, int32_t Nout, int32_t Ns,
                              int32_t relu, void* stream);
int scan_conv_smallcin_bf16x6(const float* x, int32_t N, int32_t H, int32_t W, const float* w, const float* bias,
                              float* y, int32_t Cout, int32_t Cout_s, int32_t ksize, int32_t stride, int32_t relu,
                              void* stream);
/* weight gradients: x and dy are split inside the kernel, no planes; Cout_s % 4 == 0.  The 3x3 workspace holds the split-K
 * slabs -- [splits][Cout][9][Cs] floats, or [splits][Cout][12][Cs] when the launch takes the Winograd form (scan_tune
 * "wgrad_wino") -- followed by [splits][Cout] bias slabs: always ask scan_conv3x3_wgrad_bf16x6_ws_floats, under the knob
 * values the launch will run with. */
int64_t scan_conv3x3_wgrad_bf16x6_ws_floats(const scan_pyramid_t* d, int32_t Cs, int32_t Cout);
int scan_conv3x3_wgrad_bf16x6(const float* x, const scan_pyramid_t* d, int32_t Cs, const float* dy, int32_t Cout,
                              int32_t Cout_s, float* dw, float* db, int32_t accumulate, float* ws, void* stream);
int64_t scan_conv1x1_wgrad_bf16x6_ws_floats(const scan_pyramid_t* yd, int32_t Cs, int32_t Cout);
int scan_conv1x1_wgrad_bf16x6(const float* x, const scan_pyramid_t* xd, int32_t Cs, const float* dy,
                              const scan_pyramid_t* yd, int32_t Cout, int32_t Cout_s, int32_t stride, float* dw,
                              float* db, int32_t accumulate, float* ws, void* stream);
/* output-channel tile (64 / 128 / 256) a scan_conv3x3_bf16x6 launch on pyramid d with Nout channels takes; 1064 = the
 * 64-channel tile on 16x16-pixel tiles (single-level pyramids with sizes that are multiples of 16), 2064 = on 32x16-pixel
 * tiles (H a multiple of 32 too) */
int scan_conv3x3_bf16x6_instance(const scan_pyramid_t* d, int32_t Nout);
/* 1-D Winograd F(2,3) along x for three-piece 3x3 / stride-1 convs: two outputs of a row from four products per ky instead
 * of six.  wh / wm / wl = scan_weight_split3 planes of mode 2 (forward: [O][12][Csw], tap j * 3 + ky
 * = sum_kx G[j][kx] w[o][ky * 3 + kx][c], G = [1 0 0; 1/2 1/2 1/2; 1/2 -1/2 1/2; 0 0 1], in fp64, rounded once to fp32)
 * or mode 3 (data gradient: the same transform of the mode-1 planes, [Cs][12][Csw]); Csw % 32 == 0, Nout > 64.
 * gn_ws != NULL: GroupNorm(32, 256) sums as scan_conv3x3_gn_bf16x6 (Nout == 256, no mask, relu == 0; clear as there).
 * No fused pool.  scan_conv3x3_bf16x6_wino: 1 if scan_tune "conv_wino" is on and a launch with these channels takes this
 * path (0: the caller uses scan_conv3x3_bf16x6 on mode-0 / 1 planes). */
int scan_conv3x3_wino_bf16x6(const float* x, const scan_pyramid_t* d, int32_t Cs, const void* wh, const void* wm,
                             const void* wl, int32_t Csw, const float* bias, const float* mask, float* y, int32_t Nout,
                             int32_t Ns, int32_t relu, float* gn_ws, int32_t clear, void* stream);
int scan_conv3x3_bf16x6_wino(int32_t Nout, int32_t Csw);
/* ---- one dispatcher for the split-operand forward / data-gradient convolutions above (no reference counterpart) ----
 * Which weight planes a conv needs, which kernel family and instance runs it and how the launch is cut are decided HERE,
 * once, for every binding (scan_amd.ops over ctypes, the compiled scan_ops module, a C caller): plan the conv, split the
 * weights as the plan says, run it.  The entry points above stay what they were: single launches of one family for callers
 * that choose themselves.  A plan is host arithmetic under the scan_tune knobs of the moment ("conv_wino" and the instance
 * knobs): plan again after changing one; planes split for a plan belong to that plan's split_mode / csw / pieces. */
#define SCAN_CONV_SUMS 1 /* flags: the epilogue accumulates GroupNorm(32, 256) sums (3x3, nout == 256, no ReLU, no mask) */
#define SCAN_CONV_POOL 2 /* flags: fused 2x2 / stride-2 max-pool (3x3 forward, single-level pyramid with even H, W) */
#define SCAN_CONV_DIRECT3X3 0 /* family: scan_conv3x3_bf16x3 / _bf16x6 and their _gn_ / _pool2_ forms */
#define SCAN_CONV_WINO3X3 1   /* family: scan_conv3x3_wino_bf16x6 */
#define SCAN_CONV_1X1 2       /* family: scan_conv1x1_bf16x3 / _bf16x6 */
typedef struct {
  int32_t pieces;     /* bf16 pieces per fp32 operand: 2 ("bf16x3") or 3 ("bf16x6") */
  int32_t taps;       /* taps of the packed fp32 weight [O][taps][Cs_w]: 9 (3x3 / stride 1) or 1 (1x1) */
  int32_t dgrad;      /* 0: forward (nout = O); 1: data gradient (nout = Cs_w, x = dY) */
  int32_t O, Cs_w;    /* the packed weight's rows and row length, as given to scan_conv_plan */
  int32_t split_mode; /* scan_weight_split mode the planes are written in: 0 / 1 = forward / dgrad, 2 / 3 = their Winograd planes */
  int32_t plane_rows; /* each plane is [plane_rows][plane_taps][csw] bf16 */
  int32_t plane_taps; /* 9, 1, or 12 (Winograd) */
  int32_t csw;        /* plane row length: 3x3 planes are padded to whole 32-channel K chunks, 1x1 planes to 8 */
  int32_t nout;       /* output channels of the conv */
  int32_t rem;        /* > 0: the last rem output channels run as a second launch of the direct kernel (a 3x3 conv with
                         nout > 128, 0 < nout % 128 <= 64, Cs_src >= 512 and >= 100,000 output rows, without sums or pool:
                         the 64-channel instance takes the remainder instead of an almost empty 128-wide tile) */
  int32_t family;     /* SCAN_CONV_DIRECT3X3 / SCAN_CONV_WINO3X3 / SCAN_CONV_1X1 */
  int32_t instance;   /* what the scan_conv*_instance queries report for the whole nout (3128 = the Winograd instance):
                         the label bench.py's kernel timer prints */
  int32_t flags;      /* SCAN_CONV_SUMS | SCAN_CONV_POOL as planned */
} scan_conv_plan_t;
/* Fills *plan for a conv with packed weights [O][taps][Cs_w] reading Cs_src channels per pixel (forward: the input's row
 * length, normally Cs_w; dgrad: dY's row length, >= O) on output pyramid od (3x3: the pyramid of input and output, before
 * the pool if any).  Touches no device. */
int scan_conv_plan(int32_t pieces, int32_t taps, int32_t dgrad, int32_t O, int32_t Cs_w, int32_t Cs_src,
                   const scan_pyramid_t* od, int32_t flags, scan_conv_plan_t* plan);
/* scan_weight_split / scan_weight_split3 of w [O][taps][Cs_w] in the plan's pieces, split_mode and csw; p2 only with three pieces */
int scan_conv_weight_split(const scan_conv_plan_t* plan, const float* w, void* p0, void* p1, void* p2, void* stream);
/* Runs the planned conv on planes from scan_conv_weight_split: y [M][Ns] (first nout columns written).  3x3: xd is the one
 * pyramid, yd and map are not read; 1x1: xd / yd / map as scan_conv1x1_bf16x3.  relu != 0: ReLU; mask as scan_conv3x3_bf16x3
 * (none with sums or pool).  gn_ws: the GroupNorm workspace of a plan with SCAN_CONV_SUMS (NULL otherwise); clear != 0 zeroes
 * it first (scan_conv3x3_gn_bf16x3), 0 adds to it (scan_conv3x3_gn_acc_bf16x3).  Everything is validated before the first
 * launch. */
int scan_conv_run(const scan_conv_plan_t* plan, const float* x, const scan_pyramid_t* xd, int32_t Cs, const void* p0,
                  const void* p1, const void* p2, const float* bias, const float* mask, float* y,
                  const scan_pyramid_t* yd, int32_t Ns, int32_t relu, int32_t map, float* gn_ws, int32_t clear,
                  void* stream);
/* ---- one dispatcher for the weight gradients above (no reference counterpart) ----
 * Kernel family, kernel variant, split-K cut and workspace layout of a weight gradient are decided ONCE, by scan_conv_wgrad_plan,
 * for every binding; scan_conv_wgrad_run launches what the plan says and reads none of the scan_tune knobs the plan decided
 * ("wgrad_v6", "wgrad_tile", "wgrad_wino", "wgrad_wgs"): a workspace of plan.ws_floats fits the launch whatever the knobs say
 * by then.  ("wgrad_prio", a scheduling hint without effect on layout or bits, is still read at launch.)  The entry points
 * above stay what they were; each plans under the knobs of the moment and runs. */
#define SCAN_WGRAD_SPLIT3X3 1 /* family: scan_conv3x3_wgrad_bf16x3 / _bf16x6 (pieces 2 / 3, 3x3, stride 1) */
#define SCAN_WGRAD_SPLIT1X1 2 /* family: scan_conv1x1_wgrad_bf16x3 / _bf16x6 (pieces 2 / 3, 1x1, stride 1 or 2) */
#define SCAN_WGRAD_GENERIC 3  /* family: scan_conv2d_wgrad, then scan_colsum for the bias gradient (everything else) */
#define SCAN_WGRAD_FP32 0          /* variant: conv_wgrad_kernel, fp32 MFMAs (the generic family) */
#define SCAN_WGRAD_V4 1            /* variant: conv_wgrad_v4_kernel (every 1x1; 3x3 under wgrad_v6 = 0) */
#define SCAN_WGRAD_V6_64X32 2      /* variant: conv_wgrad_v6_kernel, consumer wave tile 64 (o) x 32 (c) */
#define SCAN_WGRAD_V6_32X64 3      /* variant: conv_wgrad_v6_kernel, wave tile 32 x 64 */
#define SCAN_WGRAD_V6_32X64_WINO 4 /* variant: the same in the Winograd F(2,3) form across rows (pieces 3 only) */
typedef struct {
  int32_t family;      /* SCAN_WGRAD_SPLIT3X3 / _SPLIT1X1 / _GENERIC */
  int32_t pieces;      /* as given: 0 (fp32, always generic), 2 ("bf16x3") or 3 ("bf16x6") */
  int32_t ksize;       /* 1, 3, 5 or 7 */
  int32_t stride;      /* 1 or 2 */
  int32_t Cs, Cout;    /* row length of x and output channels: dw is [Cout][ksize * ksize][Cs] */
  int32_t variant;     /* SCAN_WGRAD_FP32 / _V4 / _V6_64X32 / _V6_32X64 / _V6_32X64_WINO */
  int32_t wk;          /* pixels per K chunk of that kernel: 64, or 32 (three pieces on the v6 kernel; generic) */
  int32_t n_tiles;     /* output tiles per split: 128-channel Cout tiles x tap groups (3 row taps, 4 Winograd components, 1;
                          generic: ksize * ksize) x c_tiles */
  int32_t c_tiles;     /* 128-channel tiles of Cs */
  int32_t splits;      /* split-K slabs; the launch has n_tiles * splits workgroups */
  int32_t cps;         /* K chunks per split */
  int32_t slab_taps;   /* taps a slab holds per output channel: 12 (Winograd), 9, 1; generic: ksize * ksize */
  int32_t fused_db;    /* 1: the kernel also sums dy's columns (split families); 0: scan_colsum's kernels follow (generic) */
  int64_t chunks;      /* K chunks in all: wk-pixel pieces of the rows (Winograd: row pairs) of x's pyramid (3x3) or dy's (1x1);
                          generic: wk-row pieces of dy */
  int64_t slab_floats; /* the workspace starts with [splits][Cout][slab_taps][Cs] weight slabs: this many floats */
  int64_t bias_off;    /* fused_db: offset of the [splits][Cout] bias slabs; otherwise -1 */
  int64_t colsum_off;  /* not fused_db: offset of scan_colsum's workspace for dy; otherwise -1 */
  int64_t ws_floats;   /* floats the workspace must hold */
} scan_conv_wgrad_plan_t;
/* Fills *plan for the weight gradient of a conv (pad ksize / 2) with x [.., Cs] on pyramid xd and dy on pyramid yd.  pieces 2 /
 * 3 with ksize 3 and stride 1 take the split 3x3 family, with ksize 1 the split 1x1 family; everything else (pieces 0 too) that
 * scan_conv2d_wgrad accepts is generic.  Host arithmetic under the scan_tune knobs of the moment; touches no device. */
int scan_conv_wgrad_plan(int32_t pieces, int32_t ksize, int32_t stride, int32_t Cs, int32_t Cout, const scan_pyramid_t* xd,
                         const scan_pyramid_t* yd, scan_conv_wgrad_plan_t* plan);
/* Runs the planned weight gradient: dw [Cout][ksize * ksize][Cs], db [Cout] or NULL, dy rows of length Cout_s, ws of
 * plan->ws_floats floats, everything on stream.  accumulate: bit 0 adds to dw, bit 1 adds to db instead of overwriting.  The
 * split families reduce both in one launch under one flag: with db != NULL, differing bits are refused.  The generic family
 * runs scan_colsum's kernels for db after the weight gradient.  Refused before any launch: a plan the planner did not fill (its
 * layout is re-derived from its shape, variant and splits and compared), Cs / Cout other than planned, pyramids whose chunk
 * count is not the plan's. */
int scan_conv_wgrad_run(const scan_conv_wgrad_plan_t* plan, const float* x, const scan_pyramid_t* xd, int32_t Cs,
                        const float* dy, const scan_pyramid_t* yd, int32_t Cout, int32_t Cout_s, float* dw, float* db,
                        int32_t accumulate, float* ws, void* stream);
/* w [Cout][T][Cin_s] -> wt [Cin_s][T][Cout_s] (zero padded) */
int scan_weight_transpose(const float* w, int32_t Cout, int32_t T, int32_t Cin_s, float* wt, int32_t Cout_s,
                          void* stream);
/* column sums: db[c] (+)= sum_m dy[m][c], c < C; ws >= scan_colsum_ws_floats */
int64_t scan_colsum_ws_floats(int64_t M, int32_t C);
int scan_colsum(const float* dy, int64_t M, int32_t C, int32_t ld, float* db, int32_t accumulate, float* ws,
                void* stream);
/* out = dy * (y > 0)   (ReLU backward; y is the ReLU output; out may alias dy).  Any 4-byte alignment: the float4 kernel when
 * all three pointers are 16-byte aligned, otherwise one float per lane, the same bits. */
int scan_relu_backward(const float* dy, const float* y, float* out, int64_t n, void* stream);

/* ---- GroupNorm(32 groups) + ReLU on a pyramid (replaces nn.GroupNorm(32,C)+nn.ReLU in the towers,
 *      condgraph.py:99-105, fcos.py:36-49, fcos_head_discriminator_con.py:31-32) ----
 * stats [n_levels*N*G*2] = (mean, rstd) per (level, image, group), eps = 1e-5.
 * ws (8-byte aligned): scan_groupnorm_ws_floats floats, used as fp64 accumulators. */
int scan_groupnorm_stats(const float* x, const scan_pyramid_t* d, int32_t C, int32_t G, float eps, float* stats,
                         float* ws, void* stream);
int scan_groupnorm_relu_forward(const float* x, const scan_pyramid_t* d, int32_t C, int32_t G, const float* stats,
                                const float* gamma, const float* beta, int32_t relu, float* y, void* stream);
/* scan_groupnorm_stats_from_sums + scan_groupnorm_relu_forward as ONE launch (sums: fp64 [n_levels*N*G][2] accumulated
 * by scan_conv3x3_gn_bf16x3; stats [n_levels*N*G][2] is written for scan_groupnorm_relu_backward). */
int scan_groupnorm_relu_forward_from_sums(const float* x, const scan_pyramid_t* d, int32_t C, int32_t G,
                                          const float* sums, float eps, const float* gamma, const float* beta,
                                          int32_t relu, float* y, float* stats, void* stream);
int64_t scan_groupnorm_ws_floats(const scan_pyramid_t* d, int32_t C, int32_t G);
/* dx, dgamma[C] (+)=, dbeta[C] (+)=; beta [C] is the forward's shift: the ReLU mask is recomputed from x with the
 * forward's exact operation order instead of reading y back (may be NULL when relu == 0);
 * accumulate: bit 0 = add to dgamma / dbeta instead of overwriting, bit 1 = ws arrives cleared (else the call clears it);
 * ws: scan_groupnorm_ws_floats */
int scan_groupnorm_relu_backward(const float* x, const float* beta, const float* dy, const scan_pyramid_t* d, int32_t C,
                                 int32_t G, const float* stats, const float* gamma, int32_t relu, float* dx,
                                 float* dgamma, float* dbeta, int32_t accumulate, float* ws, void* stream);
/* The same three with y (forward) / dy (backward) as a column slice of a wider row-major matrix: ldy / lddy = its row
 * stride in floats (a multiple of 4, >= C), the slice starts at the pointer.  The reference concatenates the tower output
 * with the act maps (torch.cat, fcos_head_discriminator_con.py:104-118); here the tower's last GroupNorm writes straight
 * into the first C columns of that matrix and reads its gradient from the same columns of the conv's data gradient. */
int scan_groupnorm_relu_forward_ld(const float* x, const scan_pyramid_t* d, int32_t C, int32_t G, const float* stats,
                                   const float* gamma, const float* beta, int32_t relu, float* y, int32_t ldy,
                                   void* stream);
int scan_groupnorm_relu_forward_from_sums_ld(const float* x, const scan_pyramid_t* d, int32_t C, int32_t G,
                                             const float* sums, float eps, const float* gamma, const float* beta,
                                             int32_t relu, float* y, int32_t ldy, float* stats, void* stream);
int scan_groupnorm_relu_backward_ld(const float* x, const float* beta, const float* dy, int32_t lddy,
                                    const scan_pyramid_t* d, int32_t C, int32_t G, const float* stats, const float* gamma,
                                    int32_t relu, float* dx, float* dgamma, float* dbeta, int32_t accumulate, float* ws,
                                    void* stream);
/* Ordered forms (scan_tune "deterministic"): scan_groupnorm_stats and the backward add the fp64 sums of the 256-row chunks
 * of a (level, image) with atomics, and a double sum in another order can round to another float.  Here every workgroup
 * stores its sums to its own slot -- ws = fp64 [level * N + image][chunk][group][2], then [workgroup][C][2] for dgamma /
 * dbeta (backward only) -- and the consuming kernel (the statistics' final kernel; the backward's apply kernel) adds the
 * chunks of a (level, image), and all workgroups for dgamma / dbeta, in ascending order.  ws: 16-byte aligned,
 * scan_groupnorm_ordered_ws_floats floats, never cleared (accumulate has bit 0 only).  Same arguments otherwise; a conv whose
 * output goes through these is launched WITHOUT epilogue sums (scan_conv3x3_bf16x6 and friends, not the _gn_ forms, whose
 * epilogue sums are atomic), followed by scan_groupnorm_stats_ordered and scan_groupnorm_relu_forward. */
int64_t scan_groupnorm_ordered_ws_floats(const scan_pyramid_t* d, int32_t C, int32_t G);
int scan_groupnorm_stats_ordered(const float* x, const scan_pyramid_t* d, int32_t C, int32_t G, float eps, float* stats,
                                 float* ws, void* stream);
int scan_groupnorm_relu_backward_ordered(const float* x, const float* beta, const float* dy, const scan_pyramid_t* d,
                                         int32_t C, int32_t G, const float* stats, const float* gamma, int32_t relu,
                                         float* dx, float* dgamma, float* dbeta, int32_t accumulate, float* ws,
                                         void* stream);
int scan_groupnorm_relu_backward_ld_ordered(const float* x, const float* beta, const float* dy, int32_t lddy,
                                            const scan_pyramid_t* d, int32_t C, int32_t G, const float* stats,
                                            const float* gamma, int32_t relu, float* dx, float* dgamma, float* dbeta,
                                            int32_t accumulate, float* ws, void* stream);
/* ---- one plan and one launcher for the GroupNorm entry points above (no reference counterpart) ----
 * Where the statistics come from, whether the reductions are atomic or ordered and how much workspace that takes are decided
 * ONCE, by scan_groupnorm_plan, for every binding: plan, allocate what the plan says, run.  scan_groupnorm_plan is the only
 * reader of scan_tune "deterministic" for GroupNorm; the run functions launch what was planned, whatever the knob says by then.
 * The entry points above stay what they were: single steps for callers that choose themselves. */
#define SCAN_GN_SUMS 1           /* flags: the caller holds conv-epilogue sums of x (scan_conv_run on a SCAN_CONV_SUMS plan) */
#define SCAN_GN_SEPARATE_FINAL 2 /* flags, with SCAN_GN_SUMS: finalise them in a launch of their own instead of in the apply launch */
#define SCAN_GN_FROM_X 0          /* source: scan_groupnorm_stats / _stats_ordered read x, then scan_groupnorm_relu_forward_ld */
#define SCAN_GN_FROM_SUMS 1       /* source: scan_groupnorm_relu_forward_from_sums_ld, one launch */
#define SCAN_GN_FROM_SUMS_FINAL 2 /* source: scan_groupnorm_stats_from_sums, then scan_groupnorm_relu_forward_ld */
typedef struct {
  int32_t C, G;           /* channels and groups as given: 256 and 32, the one built pair */
  int32_t n_levels;       /* of the pyramid planned for */
  int32_t n_images;       /* of the pyramid planned for */
  int32_t blocks;         /* workgroups of the statistics, apply and backward launches: 256-row chunks of every (level, image) */
  int32_t ordered;        /* 0: atomic reductions; 1: the ordered forms (scan_tune "deterministic" was on when planned) */
  int32_t source;         /* SCAN_GN_FROM_X / _FROM_SUMS / _FROM_SUMS_FINAL.  Epilogue sums are atomic, so an ordered plan answers
                             SCAN_GN_FROM_X whatever the flags offered: sums of a conv that ran before the knob was switched on are
                             not read */
  int32_t stats_floats;   /* floats of the (mean, rstd) table the forward writes and the backward reads: n_levels * N * G * 2 */
  int32_t fwd_ws_doubles; /* fp64 values of run_forward's ws (read with SCAN_GN_FROM_X only; 16-byte aligned): half of
                             scan_groupnorm_ws_floats, ordered: of scan_groupnorm_ordered_ws_floats */
  int32_t bwd_ws_doubles; /* the same for run_backward's ws */
} scan_groupnorm_plan_t;
/* Fills *plan for GroupNorm(G, C) on pyramid d.  Host arithmetic under the knob of the moment; touches no device. */
int scan_groupnorm_plan(const scan_pyramid_t* d, int32_t C, int32_t G, int32_t flags, scan_groupnorm_plan_t* plan);
/* y [.., ldy] = GroupNorm(x) (ReLU with relu != 0); stats [plan->stats_floats] is written.  sums: the conv epilogue's fp64
 * [n_levels * N * G][2] (a source from sums; not read otherwise, may be NULL); ws: plan->fwd_ws_doubles doubles (SCAN_GN_FROM_X;
 * may be NULL otherwise).  Both run functions re-derive the plan's shape fields from d and refuse, before any launch, a plan that
 * differs (zeroed, edited, made for another pyramid), a row stride that is < C or no multiple of 4, and a missing pointer. */
int scan_groupnorm_run_forward(const scan_groupnorm_plan_t* plan, const float* x, const scan_pyramid_t* d, const float* sums,
                               float eps, const float* gamma, const float* beta, int32_t relu, float* y, int32_t ldy,
                               float* stats, float* ws, void* stream);
/* Arguments as scan_groupnorm_relu_backward_ld; accumulate: 0, or 1 = add to dgamma / dbeta.  ws: plan->bwd_ws_doubles doubles;
 * ws_cleared != 0: an atomic plan's ws arrives zeroed and the call does not clear it (ignored by an ordered plan, whose launch
 * writes every slot). */
int scan_groupnorm_run_backward(const scan_groupnorm_plan_t* plan, const float* x, const float* beta, const float* dy,
                                int32_t lddy, const scan_pyramid_t* d, const float* stats, const float* gamma, int32_t relu,
                                float* dx, float* dgamma, float* dbeta, int32_t accumulate, float* ws, int32_t ws_cleared,
                                void* stream);

/* ---- the source pass's ground-truth plan on the device (reference rpn/fcos/loss.py:40-133: FCOS location -> GT
 *      assignment and centerness targets; :428-463: graph-node sampling of the source branch).  Rows = pyramid rows
 *      (level-major, image, y, x); strides [n_levels], soi [n_levels][2] = sizes of interest; boxes [N][G][4] xyxy padded
 *      to G per image, glabels [N][G], ng [N] = boxes of each image.
 *      scan_fcos_assign: labels [M] (+ an int32 copy), reg [M][4] = (l, t, r, b) of the assigned box, level_pos
 *      [SCAN_MAX_LEVELS] = positives per level (device counters; the host reads them once to size the rest).
 *      scan_fcos_compact: pos_list / neg_list [M]: per level, at its row offset, the rows with label > 0 / == 0 in row
 *      order.  scan_fcos_nodes (level_pos: HOST copy of the counters): node_index / node_labels [scan_fcos_nodes_count]
 *      in the reference's order [all negatives picked, all positives], pos_inds [n_pos], reg_pos [n_pos][4], ctr_pos
 *      [n_pos]. ---- */
int scan_fcos_assign(const scan_pyramid_t* d, const int32_t* strides, const float* soi, const float* boxes,
                     const int64_t* glabels, const int32_t* ng, int32_t G, int64_t* labels, int32_t* labels_i32,
                     float* reg, int32_t* level_pos, void* stream);
int scan_fcos_compact(const scan_pyramid_t* d, const int64_t* labels, int32_t* pos_list, int32_t* neg_list, void* stream);
int64_t scan_fcos_nodes_count(const scan_pyramid_t* d, const int32_t* level_pos);
int scan_fcos_nodes(const scan_pyramid_t* d, const int32_t* level_pos, const int64_t* labels, const float* reg,
                    const int32_t* pos_list, const int32_t* neg_list, int64_t* node_index, int64_t* node_labels,
                    int64_t* pos_inds, float* reg_pos, float* ctr_pos, void* stream);

/* ---- the ATSS head's ground-truth plan and GIoU loss (csrc/atss.hip; reference rpn/atss/loss.py:159-218, 354, 360-373 for
 *      POSITIVE_TYPE 'ATSS', REGRESSION_TYPE 'BOX', one anchor per location).  The anchor of pyramid row (level l, y, x) has
 *      centre (x * s + (s - 1) / 2, y * s + (s - 1) / 2) and corners centre -/+ (a - 1) / 2 with s = strides[l],
 *      a = anchor_sizes[l]; no anchor tensor exists.  Inputs as scan_fcos_assign (boxes 16-byte aligned, ng[n] <= G), topk in
 *      1..64.  Per image and box: candidates = per level the min(topk, anchors) anchors nearest to the box centre (fp32
 *      sqrt(dx * dx + dy * dy), ties to the smaller row); threshold = mean + unbiased std of the candidates' IoUs (+1 widths;
 *      fp64 sums rounded to fp32 once); positive = IoU >= threshold and centre inside the box with min(l, t, r, b) > 0.01; a
 *      contested anchor takes the box of largest IoU, ties to the smaller box index; no positive box: label 0 (also every row
 *      of an image with ng = 0 -- the reference raises there).  The tie rules are this library's; the reference leaves them
 *      to torch.topk / torch.max.  Bit-reproducible whatever scan_tune "deterministic" says (integer max, no float atomics).
 *      scan_atss_assign: labels [M] (+ int32 copy), matched [M] = box index (0 where background), level_pos
 *      [SCAN_MAX_LEVELS] device counters; ws: scan_atss_assign_ws_bytes bytes, 8-byte aligned.  scan_fcos_compact on labels
 *      lists the positives; scan_atss_targets (level_pos: HOST copy) writes pos_inds [n_pos] in row order, reg_pos [n_pos][4]
 *      = BoxCoder.encode(matched box, anchor) (weights 10, 10, 5, 5) and ctr_pos [n_pos] = centerness of decode(encode(..))
 *      against the anchor centre, both formed in fp64 and rounded to fp32 once. ---- */
int64_t scan_atss_assign_ws_bytes(const scan_pyramid_t* d, int32_t G, int32_t topk);
int scan_atss_assign(const scan_pyramid_t* d, const int32_t* strides, const float* anchor_sizes, const float* boxes,
                     const int64_t* glabels, const int32_t* ng, int32_t G, int32_t topk, int64_t* labels,
                     int32_t* labels_i32, int32_t* matched, int32_t* level_pos, void* ws, void* stream);
int scan_atss_targets(const scan_pyramid_t* d, const int32_t* strides, const float* anchor_sizes, const int32_t* level_pos,
                      const float* boxes, int32_t G, const int32_t* matched, const int32_t* pos_list, int64_t* pos_inds,
                      float* reg_pos, float* ctr_pos, void* stream);
/* GIoU loss of anchor deltas (loss.py:64-105): pred / target [P][4] deltas (16-byte aligned) of the pyramid rows rows [P],
 * weight [P] (required).  Forward ADDS sum(w * (1 - GIoU)) to out2[0] and sum(w) to out2[1] (clear them first); the _ordered
 * twin writes both from per-block slots in a fixed order (ws: scan_atss_giou_ordered_ws_floats floats).  Decode clamps dw, dh
 * at log(1000 / 16), corners are centre -/+ 0.5 * (w - 1), the prediction takes x2 = max(x1, x2), the intersection counts only
 * where both extents are positive, 1e-7 is added to enclosure and union.  Backward: d_pred [P][4] = g_num_dev[0] * d(sum)/d pred;
 * where a min / max has equal arguments the gradient goes to its first argument (the prediction's corner; x1 in max(x1, x2)). */
int scan_atss_giou_forward(const scan_pyramid_t* d, const int32_t* strides, const float* anchor_sizes, const float* pred,
                           const float* target, const int64_t* rows, const float* weight, int64_t P, float* out2,
                           void* stream);
int64_t scan_atss_giou_ordered_ws_floats(int64_t P);
int scan_atss_giou_forward_ordered(const scan_pyramid_t* d, const int32_t* strides, const float* anchor_sizes,
                                   const float* pred, const float* target, const int64_t* rows, const float* weight,
                                   int64_t P, float* out2, float* ws, void* stream);
int scan_atss_giou_backward(const scan_pyramid_t* d, const int32_t* strides, const float* anchor_sizes, const float* pred,
                            const float* target, const int64_t* rows, const float* weight, int64_t P,
                            const float* g_num_dev, float* d_pred, void* stream);

/* ---- the RetinaNet head's ground-truth plan and smooth-L1 loss (csrc/retina.hip; reference modeling/matcher.py:42-112 with
 *      allow_low_quality_matches, rpn/loss.py:42-89, rpn/retinanet/loss.py:43-80, modeling/box_coder.py:22-50,
 *      layers/smooth_l1_loss.py).  A = 1..16 anchors per location: anchor i = m * A + a of pyramid row m = (level l, image, y, x)
 *      is cells[l][a] + (x s, y s, x s, y s), s = strides[l] (host array), cells [n_levels][A][4] fp32 xyxy a DEVICE buffer,
 *      16-byte aligned; no [M * A][4] anchor tensor exists.  boxes [N][G][4] (16-byte aligned), glabels [N][G], ng [N] as
 *      scan_fcos_assign; boxes beyond ng[n] take no part.
 *      scan_retina_match: IoU = boxlist_iou in fp32 (+1 extents, clamp(min=0), inter / (a1 + a2 - inter), every operation
 *      rounded on its own: torch-CPU's bits).  Pass 1: per (image, box) the max IoU over the image's anchors (integer max of the
 *      bits, reduced in the wave before one atomic).  Pass 2, per anchor: max / argmax over the image's boxes (equal IoUs: the
 *      smaller box index -- this library's rule); max < bg_thr: label 0; bg_thr <= max < fg_thr: label -1; else glabels of the
 *      argmax box; an anchor whose IoU with SOME real box equals that box's maximum gets the label of its OWN argmax box
 *      whatever its IoU (ties included; a box that overlaps no anchor has maximum 0, which every anchor missing it equals).
 *      ng[n] = 0: all background (the reference raises).  Outputs: labels_i32 [M * A], matched [M * A] = argmax box where
 *      label > 0 else 0, n_pos[0] = anchors with label > 0 (device counter, cleared here).  ws: scan_retina_match_ws_bytes
 *      bytes.  Two memsets and two launches; integer atomics only, so the result is bit-reproducible whatever scan_tune
 *      "deterministic" says and there is no *_ordered twin.
 *      scan_retina_smooth_l1_*: over ALL M * A anchors, no compaction.  Where labels_i32 > 0 the target is
 *      BoxCoder.encode(boxes[n][matched], anchor), weights (10, 10, 5, 5), TO_REMOVE = 1, formed in fp64 and rounded to fp32
 *      once; the prediction is columns [4a, 4a + 4) of row m of bbox_reg, whose row pitch is ld floats (a multiple of 4,
 *      >= 4 A; 16-byte aligned).  Forward ADDS sum of (0.5 d^2 / beta where |d| < beta, |d| - 0.5 beta elsewhere) to out[0]
 *      (clear it first); the _ordered twin writes it from per-block slots in a fixed order (ws:
 *      scan_retina_smooth_l1_ordered_ws_floats(M * A) floats).  targets_out (optional, [M * A][4], 16-byte aligned): the
 *      encoded targets, zero where label <= 0.  Backward: d_pred (row pitch ld_out) = g_dev[0] * (d / beta where |d| < beta,
 *      sign(d) elsewhere) for EVERY anchor, zero where label <= 0. ---- */
int64_t scan_retina_match_ws_bytes(const scan_pyramid_t* d, int32_t G);
int scan_retina_match(const scan_pyramid_t* d, const int32_t* strides, const float* cells, int32_t A, const float* boxes,
                      const int64_t* glabels, const int32_t* ng, int32_t G, float bg_thr, float fg_thr, int32_t* labels_i32,
                      int32_t* matched, int32_t* n_pos, void* ws, void* stream);
int scan_retina_smooth_l1_forward(const scan_pyramid_t* d, const int32_t* strides, const float* cells, int32_t A,
                                  const float* boxes, int32_t G, const int32_t* labels_i32, const int32_t* matched,
                                  const float* bbox_reg, int64_t ld, float beta, float* targets_out, float* out, void* stream);
int64_t scan_retina_smooth_l1_ordered_ws_floats(int64_t n_anchors);
int scan_retina_smooth_l1_forward_ordered(const scan_pyramid_t* d, const int32_t* strides, const float* cells, int32_t A,
                                          const float* boxes, int32_t G, const int32_t* labels_i32, const int32_t* matched,
                                          const float* bbox_reg, int64_t ld, float beta, float* targets_out, float* out,
                                          float* ws, void* stream);
int scan_retina_smooth_l1_backward(const scan_pyramid_t* d, const int32_t* strides, const float* cells, int32_t A,
                                   const float* boxes, int32_t G, const int32_t* labels_i32, const int32_t* matched,
                                   const float* bbox_reg, int64_t ld, float beta, const float* g_dev, float* d_pred,
                                   int64_t ld_out, void* stream);

/* ---- the region-proposal network (csrc/rpn.hip; reference modeling/rpn/loss.py:56-131, rpn/inference.py:74-121,
 *      rpn/anchor_generator.py:97-110, modeling/balanced_positive_negative_sampler.py, modeling/box_coder.py).  Anchors, strides
 *      and cells as in the RetinaNet block above: anchor i = m * A + a is formed in the kernel, no [M * A][4] tensor exists.
 *      image_hw [N][2] int32 (DEVICE): the unpadded (height, width) of every image.
 *      scan_rpn_visibility: runs behind scan_retina_match called with every box label 1 (labels 1 / 0 / -1).  Writes label -1
 *      (and matched 0) where the anchor is not visible: visible = x1 >= -t and y1 >= -t and x2 < width + t and y2 < height + t,
 *      t = straddle_thresh; t < 0: every anchor is visible, nothing is launched.  One launch, no visibility tensor.  Invisible
 *      anchors have taken part in the per-box maxima of the low-quality rule, as in the reference.
 *      scan_rpn_sample: per image n, num_pos = min(#label >= 1, max_positives), num_neg = min(#label == 0,
 *      batch_size_per_image - num_pos).  The sampled positives are the num_pos anchors with label >= 1 that have the smallest
 *      (key, anchor index) pairs; the sampled negatives likewise among label == 0.  key = keys[i] when keys is not NULL
 *      ([M * A] uint32, device), else
 *          fmix32(fmix32(seed ^ (0x9E3779B9 * (n + 1))) ^ (uint32)i),
 *          fmix32(x): x ^= x >> 16; x *= 0x85EBCA6B; x ^= x >> 13; x *= 0xC2B2AE35; x ^= x >> 16   (all mod 2^32).
 *      Outputs: sampled [M * A] uint8 (1 sampled positive, 2 sampled negative, 0 otherwise; every byte is written),
 *      counts [N][2] int32 = (num_pos, num_neg).  Grid: 2 N workgroups of 256 threads, one per (image, class), each walking the
 *      image's row range of every level; a radix select over the key bits (8 bits a pass, LDS histogram).  No cap on the
 *      anchors per image; M * A < 2^31.  Integers only: bit-reproducible whatever scan_tune "deterministic" says, no ordered twin.
 *      scan_rpn_loss_*: over ALL M * A anchors, no compaction.  objectness row m holds A logits (row pitch ld_obj floats),
 *      bbox_reg row m holds 4 A (row pitch ld_reg, a multiple of 4; 16-byte aligned).  Forward ADDS to out2 (clear it first):
 *      out2[0] += sum over sampled != 0 of max(x, 0) - x y + log1p(exp(-|x|)), y = 1 where sampled == 1 else 0;
 *      out2[1] += sum over sampled == 1 of smooth-L1(pred - BoxCoder.encode(boxes[n][matched], anchor)), weights (1, 1, 1, 1),
 *      TO_REMOVE = 1, the target formed in fp64 and rounded once, beta as in the RetinaNet block.  The _ordered twin writes both
 *      from per-block slots in a fixed order (ws: scan_rpn_loss_ordered_ws_floats(M * A) floats).  targets_out as in the
 *      RetinaNet block (zero where sampled != 1).  Backward writes, for EVERY anchor, d_obj[m][a] = g2_dev[0] *
 *      (sigmoid(x) - y) and d_reg[m][4a..4a+4) = g2_dev[1] * smooth-L1', both zero where the anchor does not take part
 *      (row pitches ldo_obj, ldo_reg).
 *      scan_rpn_decode: one launch for all levels and images.  topk_idx [N][K] int64: column k in [k_off[l], k_off[l + 1]) is a
 *      candidate of level l, its value the anchor's index within that image's level (y, x, a order, 0 .. h w A - 1); k_off a
 *      HOST array [n_levels + 1], k_off[0] = 0.  boxes [N][K][4] = BoxCoder.decode(bbox_reg columns of the anchor, anchor) with
 *      weights 1, dw / dh clamped at log(1000 / 16), +1 widths, x2 = ctr + 0.5 w - 1, clipped to [0, width - 1] x [0, height - 1];
 *      keep [N][K] uint8 = width >= min_size and height >= min_size with +1 extents.  An index outside its level gives a zero
 *      box and keep 0; nothing is read for it. ---- */
int scan_rpn_visibility(const scan_pyramid_t* d, const int32_t* strides, const float* cells, int32_t A, const int32_t* image_hw,
                        float straddle_thresh, int32_t* labels_i32, int32_t* matched, void* stream);
int scan_rpn_sample(const scan_pyramid_t* d, int32_t A, const int32_t* labels_i32, int32_t batch_size_per_image,
                    int32_t max_positives, uint32_t seed, const uint32_t* keys, uint8_t* sampled, int32_t* counts, void* stream);
int scan_rpn_loss_forward(const scan_pyramid_t* d, const int32_t* strides, const float* cells, int32_t A, const float* boxes,
                          int32_t G, const int32_t* matched, const uint8_t* sampled, const float* objectness, int64_t ld_obj,
                          const float* bbox_reg, int64_t ld_reg, float beta, float* targets_out, float* out2, void* stream);
int64_t scan_rpn_loss_ordered_ws_floats(int64_t n_anchors);
int scan_rpn_loss_forward_ordered(const scan_pyramid_t* d, const int32_t* strides, const float* cells, int32_t A, const float* boxes,
                                  int32_t G, const int32_t* matched, const uint8_t* sampled, const float* objectness,
                                  int64_t ld_obj, const float* bbox_reg, int64_t ld_reg, float beta, float* targets_out,
                                  float* out2, float* ws, void* stream);
int scan_rpn_loss_backward(const scan_pyramid_t* d, const int32_t* strides, const float* cells, int32_t A, const float* boxes,
                           int32_t G, const int32_t* matched, const uint8_t* sampled, const float* objectness, int64_t ld_obj,
                           const float* bbox_reg, int64_t ld_reg, float beta, const float* g2_dev, float* d_obj, int64_t ldo_obj,
                           float* d_reg, int64_t ldo_reg, void* stream);
int scan_rpn_decode(const scan_pyramid_t* d, const int32_t* strides, const float* cells, int32_t A, const float* bbox_reg,
                    int64_t ld, const int64_t* topk_idx, const int32_t* k_off, const int32_t* image_hw, float min_size,
                    float* boxes, uint8_t* keep, void* stream);

/* ---- the Fast R-CNN box head (csrc/roi_box.hip; reference modeling/roi_heads/box_head/loss.py:39-167, inference.py:55-146,
 *      modeling/matcher.py with allow_low_quality_matches False, modeling/box_coder.py).  Proposals of a batch are padded as the
 *      ground truth is: props [N][P][4] fp32 xyxy (16-byte aligned), np [N] int32; rows p >= np[n] take no part.  boxes [N][G][4],
 *      glabels [N][G] int64, ng [N] as scan_retina_match.  (wx, wy, ww, wh): BoxCoder's weights (BBOX_REG_WEIGHTS), positive.
 *      scan_roi_box_match: one launch, no atomics, no workspace.  Per (image, proposal) max / argmax over the image's real boxes of
 *      boxlist_iou(box, proposal) in fp32, every operation rounded on its own (the bits of scan_retina_match); equal IoUs: the
 *      smaller box index.  max < bg_thr: label 0; bg_thr <= max < fg_thr: label -1; else glabels of the argmax; no low-quality
 *      rule.  matched = argmax where label > 0, else 0.  Padding rows: label -1, matched 0.  ng[n] = 0: every real proposal is
 *      background (the reference raises); np[n] = 0 is legal.  labels_i32 / matched [N * P].
 *      Sampler: scan_rpn_sample on the pyramid of ONE level with h = P, w = 1 and N images, A = 1, walks exactly rows
 *      [n P, (n + 1) P) of the padded labels for image n; padding (-1) is never drawn and gets sampled = 0; the key index of
 *      proposal p of image n is i = n P + p.
 *      scan_roi_box_gather: one launch, one workgroup per image; replaces proposals[img][nonzero(pos | neg)].  Reads sampled
 *      [N * P] uint8 and counts [N][2] of the sampler and writes, for the sampled proposals in image-major order and ascending p
 *      within an image (image n starts at the sum of the counts of the images before it, formed in the kernel; a running block
 *      scan over P in chunks, no cap on P): rois [R][5] (image index, box), labels_out [R] int32 (the proposal's label where
 *      sampled == 1, 0 for a sampled negative), reg_targets [R][4] (16-byte aligned) = BoxCoder.encode(boxes[n][matched],
 *      proposal), TO_REMOVE = 1, formed in fp64 and rounded once, where label > 0 and zero elsewhere, src [R] int32 (p).  R comes
 *      from the caller (the sum of counts); nothing is written at or beyond row R; R = 0 launches nothing.
 *      scan_roi_box_loss_*: over the R sampled rows, a wave per row, any C >= 2.  class_logits [R][C] (row pitch ld_cls floats),
 *      box_regression [R][4 Cr] (row pitch ld_reg, a multiple of 4; 16-byte aligned), Cr = C or 2 (CLS_AGNOSTIC_BBOX_REG), both
 *      read in place; labels [R] int32 in 0 .. C - 1 (a row with any other label takes no part), reg_targets [R][4].  Forward
 *      ADDS to out2 (clear it first): out2[0] += sum_r logsumexp(x_r) - x_r[label_r], max-subtracted in fp32 (m + log1p of the other exponentials' sum); out2[1] += sum over
 *      label_r > 0 of smooth-L1 (beta 1) of columns [4 label_r, 4 label_r + 4) -- [4, 8) when Cr = 2 -- against reg_targets[r].
 *      The host divides both by R.  R = 0 adds nothing.  The _ordered twin writes both from per-block slots in a fixed order (ws:
 *      scan_roi_box_loss_ordered_ws_floats(R) floats).  Backward writes EVERY element: d_cls[r][j] = g2_dev[0] (softmax_j -
 *      [j == label_r]) (row pitch ldo_cls), d_reg[r][..] = g2_dev[1] smooth-L1' on the label's four columns and exactly zero on
 *      every other (row pitch ldo_reg, a multiple of 4; 16-byte aligned).
 *      scan_roi_box_decode: one launch over R test-time rows; rois [R][5] as above, image_hw [N][2] int32 (DEVICE).  scores
 *      [R][C] = softmax, max-subtracted; boxes [R][C][4] = BoxCoder.decode of the class's four columns (Cr = 2: columns [4, 8) for
 *      every class) against the ROI: deltas divided by the weights, dw / dh clamped at log(1000 / 16), +1 widths, x2 = ctr +
 *      0.5 w - 1, clipped to [0, width - 1] x [0, height - 1] of the ROI's image; cand [R][C] uint8 = j >= 1 and score >
 *      score_thresh.  Every byte is written; a ROI whose image index is outside 0 .. N - 1 gives zeros and cand 0. ---- */
int scan_roi_box_match(const float* props, const int32_t* np, int32_t N, int32_t P, const float* boxes, const int64_t* glabels,
                       const int32_t* ng, int32_t G, float bg_thr, float fg_thr, int32_t* labels_i32, int32_t* matched,
                       void* stream);
int scan_roi_box_gather(const float* props, int32_t N, int32_t P, const float* boxes, int32_t G, const int32_t* labels_i32,
                        const int32_t* matched, const uint8_t* sampled, const int32_t* counts, float wx, float wy, float ww,
                        float wh, int32_t R, float* rois, int32_t* labels_out, float* reg_targets, int32_t* src, void* stream);
int scan_roi_box_loss_forward(const float* class_logits, int64_t ld_cls, const float* box_regression, int64_t ld_reg, int32_t R,
                              int32_t C, int32_t Cr, const int32_t* labels, const float* reg_targets, float* out2, void* stream);
int64_t scan_roi_box_loss_ordered_ws_floats(int64_t R);
int scan_roi_box_loss_forward_ordered(const float* class_logits, int64_t ld_cls, const float* box_regression, int64_t ld_reg,
                                      int32_t R, int32_t C, int32_t Cr, const int32_t* labels, const float* reg_targets,
                                      float* out2, float* ws, void* stream);
int scan_roi_box_loss_backward(const float* class_logits, int64_t ld_cls, const float* box_regression, int64_t ld_reg, int32_t R,
                               int32_t C, int32_t Cr, const int32_t* labels, const float* reg_targets, const float* g2_dev,
                               float* d_cls, int64_t ldo_cls, float* d_reg, int64_t ldo_reg, void* stream);
int scan_roi_box_decode(const float* class_logits, int64_t ld_cls, const float* box_regression, int64_t ld_reg, int32_t R, int32_t C,
                        int32_t Cr, const float* rois, const int32_t* image_hw, int32_t N, float wx, float wy, float ww, float wh,
                        float score_thresh, float* scores, float* boxes, uint8_t* cand, void* stream);

/* ---- the Mask R-CNN mask head (csrc/roi_mask.hip; reference modeling/roi_heads/mask_head/{mask_head.py, loss.py, inference.py},
 *      structures/segmentation_mask.py in binary-mask mode).  No float atomics; every output element is written by its kernel, so
 *      no buffer is cleared first.  Ground-truth masks: ONE flat uint8 buffer of mask_bytes bytes; image n owns bytes [moff[n],
 *      moff[n + 1]) as [G_n][h_n][w_n], mhw [N][2] int32 = (h_n, w_n), moff int64 [N + 1], no padding to a common size, values 0 / 1.
 *      scan_roi_mask_positives: one launch of ONE workgroup (a running block scan over R in chunks of 256, no cap on R); replaces
 *      keep_only_positive_boxes and the mask loss's re-match.  labels [R] int32, rois [R][5] and src [R] of scan_roi_box_gather,
 *      matched [N * P] of scan_roi_box_match.  For the rows with label > 0, in row order: pos_rows [Rp] (the row), pos_rois [Rp][5],
 *      pos_labels [Rp], pos_gt [Rp] = matched[image P + src] (0 where the image index or src is out of range).  Rp comes from the
 *      caller (the box plan's positive counts); nothing is written at or beyond row Rp; Rp = 0 launches nothing.
 *      scan_roi_mask_targets: one launch over Rp M M outputs, targets [Rp][M][M] fp32 0 / 1 = BinaryMaskList.crop + .resize((M, M))
 *      + get_mask_tensor of mask pos_gt[r] (clamped into 0 .. G_n - 1) of image pos_rois[r][0].  Crop: every coordinate rounded
 *      half-to-even, xmin / ymin clamped to [0, w - 1] / [0, h - 1], xmax / ymax to [0, w] / [0, h], then xmax = max(xmax, xmin + 1),
 *      likewise y.  Resize, decided in integers: along an axis of crop length n, output index d has num = max((2 d + 1) n - M, 0),
 *      first neighbour i0 = num / (2 M), second min(i0 + 1, n - 1), which takes part iff num % (2 M) != 0; the target is 1 iff every
 *      participating neighbour (up to 2 x 2) is nonzero -- the exact value of the reference's bilinear (align_corners False) sum
 *      truncated to uint8.  (The reference evaluates that sum in fp32 and can round an exact 1 down to 0; the device never does.)
 *      A ROI whose image index is outside 0 .. N - 1, or whose image has no mask, gives zeros.
 *      scan_roi_mask_loss_*: logits are the conv output rows [Rp M M][ld] read in place, column labels[r] of ROI r's M M rows;
 *      out1[0] = sum of max(x, 0) - x t + log1p(exp(-|x|)) (STORED, not added; the host divides by Rp M M).  A row whose label is
 *      outside 0 .. C - 1 takes no part.  forward: one launch of one workgroup (one CU's load rate: for small Rp); the _ordered twin: per-block slots (ws:
 *      scan_roi_mask_loss_ordered_ws_floats(Rp M M) floats) added in a fixed order by a second launch.  Rp = 0 stores 0.
 *      backward writes EVERY element of d_logits [Rp M M][ldo]: g_dev[0] (sigmoid(x) - t) in the label's column, exact zeros
 *      elsewhere (g_dev[0]: the incoming gradient already divided by Rp M M).
 *      scan_roi_mask_prob: one launch, prob [K][1][M][M] = sigmoid(logits[r M M + e][labels[r]]) (MaskPostProcessor.forward).
 *      scan_roi_mask_paste: one launch per image over K H W uint8 outputs (4-byte aligned), every one written
 *      (Masker.forward_single_image with padding 1; a thread owns four consecutive pixels of a row): boxes [K][4] xyxy expanded about their centres by (M + 2) / M in fp32, truncated toward zero to int32,
 *      w = max(x1 - x0 + 1, 1), likewise h; inside the box the bilinear sample (align_corners False, torch's source index with the
 *      clamp at 0, fp32) of the mask zero-padded by 1 at size (h, w), compared > thresh; 0 outside the box.  thresh < 0 is
 *      refused. ---- */
int scan_roi_mask_positives(const int32_t* labels, const float* rois, const int32_t* src, const int32_t* matched, int32_t N, int32_t P,
                            int32_t R, int32_t Rp, int32_t* pos_rows, float* pos_rois, int32_t* pos_labels, int32_t* pos_gt,
                            void* stream);
int scan_roi_mask_targets(const float* pos_rois, const int32_t* pos_gt, int32_t Rp, const uint8_t* masks, int64_t mask_bytes,
                          const int64_t* moff, const int32_t* mhw, int32_t N, int32_t M, float* targets, void* stream);
int scan_roi_mask_loss_forward(const float* logits, int64_t ld, int32_t Rp, int32_t M, int32_t C, const int32_t* labels,
                               const float* targets, float* out1, void* stream);
int64_t scan_roi_mask_loss_ordered_ws_floats(int64_t elems);
int scan_roi_mask_loss_forward_ordered(const float* logits, int64_t ld, int32_t Rp, int32_t M, int32_t C, const int32_t* labels,
                                       const float* targets, float* out1, float* ws, void* stream);
int scan_roi_mask_loss_backward(const float* logits, int64_t ld, int32_t Rp, int32_t M, int32_t C, const int32_t* labels,
                                const float* targets, const float* g_dev, float* d_logits, int64_t ldo, void* stream);
int scan_roi_mask_prob(const float* logits, int64_t ld, int32_t K, int32_t M, int32_t C, const int32_t* labels, float* prob,
                       void* stream);
int scan_roi_mask_paste(const float* prob, const float* boxes, int32_t K, int32_t M, int32_t H, int32_t W, float thresh, uint8_t* out,
                        void* stream);

/* ---- FPN top-down join on NHWC rows (reference backbone/fpn.py:62-75: inner = lateral + F.interpolate(top,
 *      scale_factor=2, mode="nearest")).  lat / y [N, 2h, 2w, C], coarse [N, h, w, C], C % 4 == 0.  Backward:
 *      d_lateral is the incoming gradient itself, d_coarse its 2x2 window sums (scan_downsample2x_sum: g [N, 2h, 2w, C]
 *      -> d [N, h, w, C]).  Every pointer 16-byte aligned (float4 rows); a misaligned one is an argument error naming it,
 *      nothing is launched. ---- */
int scan_upsample2x_add(const float* lat, const float* coarse, int32_t N, int32_t h, int32_t w, int32_t C, float* y,
                        void* stream);
int scan_downsample2x_sum(const float* g, int32_t N, int32_t h, int32_t w, int32_t C, float* d, void* stream);

/* ---- 2x2 / stride-2 max pooling on NHWC rows (replaces nn.MaxPool2d(2, 2) of the VGG body,
 *      backbone/mmdetection/vgg.py:33).  x [N,H,W,C], y [N,H/2,W/2,C]; H, W even, C % 4 == 0.
 *      backward routes the gradient to the first maximum of each window (F.max_pool2d's rule);
 *      relu_mask != 0 additionally zeroes it where that maximum is <= 0 (x is a ReLU output whose own
 *      backward was left to its consumers, see scan_conv3x3_bf16x3's mask).  Every pointer 16-byte aligned; a misaligned
 *      one is an argument error, nothing is launched. ---- */
int scan_maxpool2x2_forward(const float* x, int32_t N, int32_t H, int32_t W, int32_t C, float* y, void* stream);
int scan_maxpool2x2_backward(const float* x, const float* y, const float* dy, int32_t N, int32_t H, int32_t W,
                             int32_t C, float* dx, int32_t relu_mask, void* stream);

/* ---- ResNet body pieces (reference backbone/resnet.py): stem pooling F.max_pool2d(x, 3, 2, 1) on NHWC rows
 *      (:335; forward only -- the stem is frozen for FREEZE_CONV_BODY_AT >= 1), y [N,(H-1)/2+1,(W-1)/2+1,C], C % 4 == 0;
 *      and the residual join y = max(a + b, 0) (:312-313; backward = scan_relu_backward(dy, y) to both branches).
 *      FrozenBatchNorm2d (layers/batch_norm.py:5-24) is an affine per channel and is folded into the conv weights /
 *      bias by the host side.  The pool's x and y must be 16-byte aligned (an argument error otherwise); add_relu takes flat
 *      ranges with any 4-byte alignment: the float4 kernel when a, b and y are 16-byte aligned, otherwise one float per lane,
 *      the same bits. ---- */
int scan_maxpool3x3s2_forward(const float* x, int32_t N, int32_t H, int32_t W, int32_t C, float* y, void* stream);
int scan_add_relu(const float* a, const float* b, float* y, int64_t n, void* stream);

/* ---- target-node density clustering on the device (replaces sklearn.cluster.DBSCAN(eps, min_samples = 5) inside
 *      PrototypeComputation.DBSCAN_batch_cpu, rpn/fcos/loss.py:397-423, which only asks "is the point in cluster 0?"
 *      -- noise -> 1, cluster 0 -> 0, selected = non-zero).  pts [n][D] fp32 rows, D % 4 == 0, n <= SCAN_DBSCAN_MAX.
 *      ws: scan_dbscan_ws_bytes(n) bytes (adjacency bit matrix n^2/8 + masks), 8-byte aligned.
 *      prepare: neighbour bit matrix (fp32 matrix-core P P^T, fp64 re-check at the threshold), core mask, seed;
 *               info[0] <- lowest core index (n when there is no core point).
 *      bfs_step: one breadth-first level over the core graph; call with parity 0, 1, 0, ... while *changed reads 1.
 *      neighbor_counts: counts[i] (device, n int32) <- the number of points within eps of point i, itself included, as
 *               the last prepare on this workspace found them; a device-to-device copy, nothing in ws changes.
 *      finish:  in_cluster0[i] = 1 iff sklearn would label point i with 0.
 *      eps is a float: a caller's double is rounded to fp32 FIRST and that value is squared in double, so the threshold is
 *      fp32(eps)^2.  sklearn squares the double; the two decide differently only for a pair whose distance lies between eps
 *      and fp32(eps), i.e. within 6e-8 relative of an eps that fp32 does not represent.
 *      Re-check band: a pair goes to the fp64 re-check when |d2 - eps^2| in fp32 is within bandc (|pi|^2 + |pj|^2) (+ 1e-6
 *      eps^2) of 0.  bandc covers the worst-case error of a D-term dot product, (D - 1) 2^-24 for the fp32 matrix cores and
 *      (3 D - 1) 2^-24 + 3 * 2^-18 for bf16x3, with 12 % / 3 % on top: 1.7e-5 / 5.9e-5 for every D <= 256, the same bounds
 *      scaled by the same headroom for larger D. ---- */
#define SCAN_DBSCAN_MAX 1200000
int64_t scan_dbscan_ws_bytes(int64_t n);
int scan_dbscan_prepare(const float* pts, int64_t n, int32_t D, float eps, int32_t min_samples, void* ws,
                        int32_t* info, void* stream);
int scan_dbscan_neighbor_counts(int64_t n, const void* ws, int32_t* counts, void* stream);
int scan_dbscan_bfs_step(int64_t n, void* ws, int32_t parity, int32_t* changed, void* stream);
int scan_dbscan_finish(int64_t n, void* ws, uint8_t* in_cluster0, void* stream);

/* ---- fused SGD with momentum (replaces torch.optim.SGD as configured by solver/build.py:7-43) ----
 * g' = g + wd*p ; buf = momentum*buf + g' ; p -= lr*buf   (first_step != 0: buf = g') */
int scan_sgd_momentum(float* p, const float* g, float* buf, int64_t n, float lr, float wd, float momentum,
                      int32_t first_step, void* stream);

/* The same update over up to SCAN_SGD_MAX_SEGMENTS (p, g, buf) ranges in ONE launch: the weights and the biases of the
 * eight sub-models each have their own lr / weight decay (solver/build.py:20-28: one param group per parameter, biases
 * with BIAS_LR_FACTOR and WEIGHT_DECAY_BIAS), which torch.optim.SGD walks one parameter at a time.  segs is HOST memory
 * (copied into the kernel arguments); element arithmetic identical to scan_sgd_momentum. */
#define SCAN_SGD_MAX_SEGMENTS 32
typedef struct {
  float* p;
  const float* g;
  float* buf;
  int64_t n;
  float lr;
  float wd;
  int32_t first_step;
  int32_t reserved;
} scan_sgd_segment_t;
int scan_sgd_momentum_multi(const scan_sgd_segment_t* segs, int32_t n_segs, float momentum, void* stream);

/* ---- bf16 hi / lo planes of many conv weights in one launch (same element mapping as scan_weight_split) ----
 * jobs: DEVICE array of n_jobs records of SCAN_SPLIT_JOB_WORDS int64: {w, wh, wl (device addresses), O, T, Cs, mode,
 * rows (= mode ? Cs : O), Csw, first_block, third plane or 0}; with a third plane the job is the three-piece split of
 * scan_weight_split3 and {wh, wl, third} = its {wh, wm, wl}; job_words = SCAN_SPLIT_JOB_WORDS as the caller compiled it (a table of another layout is refused); first_block = running sum of scan_weight_split_job_blocks() over the jobs
 * before it, total_blocks the sum over all.  No reference counterpart (the reference convolves in fp32 through
 * cuDNN); it exists because a DA iteration re-splits ~120 weights after every optimizer step. */
#define SCAN_SPLIT_JOB_WORDS 11
int64_t scan_weight_split_job_blocks(int32_t O, int32_t T, int32_t Cs, int32_t mode, int32_t Csw);
int scan_weight_split_batched(const int64_t* jobs, int32_t n_jobs, int32_t job_words, int64_t total_blocks, void* stream);

/* ---- CKA discriminator class branches as two stacked convolutions ----
 * replaces the per-class loop of FCOSDiscriminator_con.forward (modeling/discriminator/
 * fcos_head_discriminator_con.py:104-121: for each foreground class c, classifier_cls_c = conv3x3(C+1 -> H) -> ReLU ->
 * conv3x3(H -> 1) on cat(x, act[:, c+1])).  branches[c] holds the four parameter tensors of class c (HOST array of
 * device pointers): w0 [H][C+1][3][3], b0 [H], w2 [1][H][3][3], b2 [1]; element (o, ci, k = 3*ky + kx) of w0 lives at
 * o*s1o + ci*s1c + k*s1k, element (h, k) of w2 at h*s2c + k*s2k (so NCHW- and channels-last-stored parameters both
 * work).  stack writes
 *   w1 [Cf*H][9][Cs1]: row c*H+o = w0_c[o] on columns 0..C-1, w0_c[o][C] on column C+c, zero elsewhere
 *   b1 [Cf*H], w2 [Cf][9][Cs2]: row c = w2_c on columns c*H..c*H+H-1, zero elsewhere; b2 [Cf]
 * in the [O][T][Cs] layout the convolution entry points take.  unstack is its adjoint: the gradient of w1 / b1 / w2 /
 * b2 (any of them NULL = absent) scattered into grads[c] (same strides), added to what is there when accumulate != 0. */
#define SCAN_CKA_MAX_CLASSES 16
typedef struct {
  const float* w0;
  const float* b0;
  const float* w2;
  const float* b2;
} scan_cka_branch_t;
int scan_cka_stack_weights(const scan_cka_branch_t* branches, int32_t Cf, int32_t C, int32_t H, int64_t s1o, int64_t s1c,
                           int64_t s1k, int64_t s2c, int64_t s2k, int32_t Cs1, int32_t Cs2, float* w1, float* b1,
                           float* w2, float* b2, void* stream);
int scan_cka_unstack_grads(const scan_cka_branch_t* grads, int32_t Cf, int32_t C, int32_t H, int64_t s1o, int64_t s1c,
                           int64_t s1k, int64_t s2c, int64_t s2k, int32_t Cs1, int32_t Cs2, const float* dw1,
                           const float* db1, const float* dw2, const float* db2, int32_t accumulate, void* stream);
/* Split form for the class branches whose act term runs inside the grouped conv (scan_gconv3x3_to1_act_* below): wmain
 * [Cf*H][9][C] = the C feature columns of every w0, e [Cf][9][H] = its act-map column, b1 / w2 / b2 as above.  unstack: dwmain
 * and de into the per-class w0 gradients (a null gradient leaves its elements alone). */
int scan_cka_stack_weights_split(const scan_cka_branch_t* branches, int32_t Cf, int32_t C, int32_t H, int64_t s1o, int64_t s1c,
                                 int64_t s1k, int64_t s2c, int64_t s2k, int32_t Cs2, float* wmain, float* e, float* b1,
                                 float* w2, float* b2, void* stream);
int scan_cka_unstack_grads_split(const scan_cka_branch_t* grads, int32_t Cf, int32_t C, int32_t H, int64_t s1o, int64_t s1c,
                                 int64_t s1k, int64_t s2c, int64_t s2k, int32_t Cs2, const float* dwmain, const float* de,
                                 const float* db1, const float* dw2, const float* db2, int32_t accumulate, void* stream);

/* ---- the class branches' second convolution: G groups of 128 channels -> one output channel per group ----
 * replaces `classifier_cls_c[2]` = nn.Conv2d(128, 1, 3, padding=1) applied per foreground class
 * (fcos_head_discriminator_con.py:44-62,118-119), for all classes at once: x [M][G*128] rows of a pyramid (the ReLU-ed
 * hidden maps of the G classes side by side), w = the stacked weight [G][9][G*128] of scan_cka_stack_weights (only the
 * diagonal blocks w[g][t][g*128 + i] are read), y [M][Ns >= G] (columns >= G are written as zero).  Plain fp32 FMA
 * arithmetic, HBM-bound (one read of x).  ws: scan_gconv3x3_to1_ws_floats floats.
 *   dgrad: dx[q][c] = sum_t dy[q - off(t)][g(c)] * w[g][t][c], multiplied by (mask[q][c] > 0) when mask != NULL (the
 *          deferred ReLU of the producer); wgrad: dw[g][t][g*128 + i] (diagonal blocks only; added to dw when
 *          accumulate != 0), deterministic.
 * These entry points take G = 1, 2, 4, 8 (kernels whose lane map is built on G * 32 dividing 256); the _any_ entry points
 * below take every 1 <= G <= scan_gconv3x3_to1_max_groups() = 31. */
int64_t scan_gconv3x3_to1_ws_floats(const scan_pyramid_t* d, int32_t G, int32_t Cg);
int scan_gconv3x3_to1_forward(const float* x, const scan_pyramid_t* d, int32_t G, int32_t Cg, const float* w,
                              const float* bias, float* y, int32_t Ns, float* ws, void* stream);
int scan_gconv3x3_to1_dgrad(const float* dy, int32_t Ns, const scan_pyramid_t* d, int32_t G, int32_t Cg, const float* w,
                            const float* mask, float* dx, void* stream);
int scan_gconv3x3_to1_wgrad(const float* x, const float* dy, int32_t Ns, const scan_pyramid_t* d, int32_t G, int32_t Cg,
                            float* dw, int32_t accumulate, float* ws, void* stream);
/* both gradients (relu_mask != 0: dx *= (x > 0)) */
int scan_gconv3x3_to1_backward(const float* x, const float* dy, int32_t Ns, const scan_pyramid_t* d, int32_t G, int32_t Cg,
                               const float* w, int32_t relu_mask, float* dx, float* dw, int32_t accumulate, float* ws,
                               void* stream);
/* Any group count 1 <= G <= scan_gconv3x3_to1_max_groups() = 31, same arguments and results: G = 1, 2, 4, 8 run the kernels
 * of the entry points above, every other G generic ones (one 32-lane half-wave per (pixel, group), plain fp32 FMA,
 * deterministic weight gradient).  Workspace: scan_gconv3x3_to1_ws_floats. */
int32_t scan_gconv3x3_to1_max_groups(void);
/* What (G, Cg) would get right now: 0 for everything the entry points refuse, else a set of the bits below.  Reads the
 * "gconv_mfma" knob, writes nothing. */
#define SCAN_GCONV_RUNS 1        /* the _any_ entry points take it */
#define SCAN_GCONV_LANE_MAPPED 2 /* G = 1, 2, 4, 8: the entry points without "any", the _bits and the _act_ ones take it too */
#define SCAN_GCONV_BITS 4        /* lane-mapped and gconv_mfma = 1: forward / backward run the matrix-core kernels, which the
                                    bit mask of _forward_bits / _backward_bits serves */
#define SCAN_GCONV_ACT 8         /* lane-mapped and gconv_mfma = 0: the act-term kernels continue the fp32 FMA path */
int32_t scan_gconv3x3_to1_caps(int32_t G, int32_t Cg);
int scan_gconv3x3_to1_any_forward(const float* x, const scan_pyramid_t* d, int32_t G, int32_t Cg, const float* w,
                                  const float* bias, float* y, int32_t Ns, float* ws, void* stream);
int scan_gconv3x3_to1_any_dgrad(const float* dy, int32_t Ns, const scan_pyramid_t* d, int32_t G, int32_t Cg, const float* w,
                                const float* mask, float* dx, void* stream);
int scan_gconv3x3_to1_any_wgrad(const float* x, const float* dy, int32_t Ns, const scan_pyramid_t* d, int32_t G, int32_t Cg,
                                float* dw, int32_t accumulate, float* ws, void* stream);
int scan_gconv3x3_to1_any_backward(const float* x, const float* dy, int32_t Ns, const scan_pyramid_t* d, int32_t G, int32_t Cg,
                                   const float* w, int32_t relu_mask, float* dx, float* dw, int32_t accumulate, float* ws,
                                   void* stream);
/* The same conv with the class branches' act-map term formed in registers (G = 1, 2, 4, 8): x = h_main [M][G*128], the first
 * conv on the feature channels alone, stored BEFORE its ReLU; a = act map rows [M][lda], class g in column a_col0 + g;
 * E [G][9][128] = the act column of each class's first-conv weight.  The kernels read
 *   hv[q][g*128 + i] = relu(x[q][g*128 + i] + sum_t E[g][t][i] * a[nb(q, t)][a_col0 + g])     (zero outside the image)
 * where the entry points above read x: forward y = conv(hv), backward dx = (hv > 0) * dgrad (the gradient of x AND of the
 * act term) and dw from hv.  act_grads is the act term's own backward, one pass over dh (= that dx):
 *   dE[g][t][i] = sum_q dh[q][g*128 + i] * a[nb(q, t)][a_col0 + g]     (fixed-order sums; added to dE when accumulate != 0)
 *   da[q][da_col0 + g] = sum_t sum_i E[g][t][i] * dh[nb(q, -t)][g*128 + i]     (every other column of da [M][ldda] := 0)
 * Workspace of each: scan_gconv3x3_to1_act_ws_floats floats. */
int64_t scan_gconv3x3_to1_act_ws_floats(const scan_pyramid_t* d, int32_t G, int32_t Cg);
int scan_gconv3x3_to1_act_forward(const float* x, const scan_pyramid_t* d, int32_t G, int32_t Cg, const float* w,
                                  const float* bias, const float* a, int32_t lda, int32_t a_col0, const float* E, float* y,
                                  int32_t Ns, float* ws, void* stream);
int scan_gconv3x3_to1_act_backward(const float* x, const float* dy, int32_t Ns, const scan_pyramid_t* d, int32_t G, int32_t Cg,
                                   const float* w, const float* a, int32_t lda, int32_t a_col0, const float* E, float* dx,
                                   float* dw, int32_t accumulate, float* ws, void* stream);
int scan_gconv3x3_to1_act_grads(const float* dh, const scan_pyramid_t* d, int32_t G, int32_t Cg, const float* a, int32_t lda,
                                int32_t a_col0, const float* E, float* da, int32_t ldda, int32_t da_col0, float* dE,
                                int32_t accumulate, float* ws, void* stream);
/* act_backward and act_grads in one pass over x (dx is used while it is in registers and never read back); same results */
int scan_gconv3x3_to1_act_backward_all(const float* x, const float* dy, int32_t Ns, const scan_pyramid_t* d, int32_t G,
                                       int32_t Cg, const float* w, const float* a, int32_t lda, int32_t a_col0, const float* E,
                                       float* dx, float* dw, float* da, int32_t ldda, int32_t da_col0, float* dE,
                                       int32_t accumulate, float* ws, void* stream);
/* forward that also leaves the ReLU mask of x as bits (relu_bits: M * G * 4 uint32; bit 4 j + e of word
 * [(row * G + g) * 4 + q] = x[row][g * 128 + 16 j + 4 q + e] > 0), and the backward that masks dx with them instead of
 * re-reading x for the mask. */
int scan_gconv3x3_to1_forward_bits(const float* x, const scan_pyramid_t* d, int32_t G, int32_t Cg, const float* w,
                                   const float* bias, float* y, int32_t Ns, float* ws, uint32_t* relu_bits, void* stream);
int scan_gconv3x3_to1_backward_bits(const float* x, const float* dy, int32_t Ns, const scan_pyramid_t* d, int32_t G,
                                    int32_t Cg, const float* w, const uint32_t* relu_bits, float* dx, float* dw,
                                    int32_t accumulate, float* ws, void* stream);

/* ---- input pipeline: the step in front of the path ----
 * scan_resize_bilinear_u8 replaces torchvision F.resize on a PIL image = PIL Image.resize(size, BILINEAR), as
 * called by Resize.__call__ (reference data/transforms/transforms.py:57-61): Pillow's two-pass fixed-point resampler.
 * src uint8 [H, W, 3] -> dst uint8 [OH, OW, 3] (device pointers); tmp = [H, OW, 3] intermediate (only when both
 * sizes change).  xbounds/ybounds int32 [O][2] = (first input index, tap count), xcoef/ycoef int32 [O][k] fixed-point
 * (22 fractional bits) triangle-filter weights -- the host computes them in double precision as Pillow's
 * precompute_coeffs does (scan_amd/data.py: bilinear_tables); bit-exact against PIL. */
int scan_resize_bilinear_u8(const uint8_t* src, int32_t H, int32_t W, uint8_t* tmp, uint8_t* dst, int32_t OH, int32_t OW,
                            const int32_t* xbounds, const int32_t* xcoef, int32_t kx, const int32_t* ybounds,
                            const int32_t* ycoef, int32_t ky, void* stream);

/* ToTensor + Normalize(to_bgr255) (+ RandomHorizontalFlip's F.hflip) (transforms.py:64-90) + the collator's zero
 * padding (data/collate_batch.py:5-20, structures/image_list.py:54-66) for ONE image: src uint8 [H, W, 3] RGB ->
 * fp32 ((x / 255)[2,1,0] * 255 - mean) / std written into a zero-padded Hp x Wp slot.  layout 0: CHW planes
 * [3, Hp, Wp] (the reference tensor); layout 1: NHWC rows [Hp * Wp, 4] (what the first convolution reads; channel 3
 * is zero).  mean3 / std3 are HOST arrays of 3 floats (BGR order when to_bgr255).  Bit-exact vs torch-CPU. */
int scan_normalize_image_u8(const uint8_t* src, int32_t H, int32_t W, int32_t flip, int32_t to_bgr255,
                            const float* mean3, const float* std3, float* dst, int32_t Hp, int32_t Wp, int32_t layout,
                            void* stream);

/* Gradient of taking the rows of images [i0, i1) out of a pyramid matrix [M, C] (the paired step splits source and target
 * frames that way, reference trainer.py:284-352 runs them as separate batches): out [M, C] = g's rows at the taken images'
 * places, zero elsewhere, in one pass.  g: [(i1 - i0) * sum_l h_l w_l, C], level-major like the pyramid. */
int scan_take_images_backward(const float* g, const scan_pyramid_t* d, int32_t i0, int32_t i1, int32_t C, float* out,
                              void* stream);

/* Conditioned-kernel generator of the graph middle head (rpn/fcos/condgraph.py:313-319 get_conded_weight: paradigm
 * [K, 256, T] -> nn.RNN(256, 512, num_layers=2, nonlinearity tanh, h0 = 0) over the T slots, batch = the K classes ->
 * Conv2d(512, 256, (T, 1)) -> kernels [K, 256]) as one launch per link of the dependent chain (2 T + 1 forward, 2 T + 2
 * backward) instead of ~120 torch launches.  K <= 9, T <= 3.  x: the paradigm slot-major, [T, K, 256].
 * weights / grads: ten device pointers in the order weight_ih_l0 [512,256], weight_hh_l0 [512,512], bias_ih_l0, bias_hh_l0,
 * weight_ih_l1 [512,512], weight_hh_l1, bias_ih_l1, bias_hh_l1, cond_nx1.weight [256,512,T,1] (contiguous), cond_nx1.bias.
 * forward: h0 / h1 [T, K, 512] = the two layers' states (kept for the backward), kernels [K, 256].
 * backward: every gradient is overwritten (the paradigm is a buffer: no input gradient); ws: scan_cond_rnn_ws_floats(). */
int scan_cond_rnn_forward(const float* x, int32_t K, int32_t T, const float* const* weights, float* h0, float* h1,
                          float* kernels, void* stream);
int64_t scan_cond_rnn_ws_floats(void);
int scan_cond_rnn_backward(const float* x, int32_t K, int32_t T, const float* const* weights, const float* h0,
                           const float* h1, const float* dkernels, float* const* grads, float* ws, void* stream);

/* ---- per-level NCHW tensors <-> the pyramid row matrix, all levels in one launch ----
 * One level of a feature pyramid as a caller outside this library holds it: the logical [N, C, h, w] fp32 tensor at `data`
 * with its four ELEMENT strides (NCHW-contiguous: sn = C h w, sc = h w, sy = w, sx = 1; channels_last: sn = h w C, sc = 1,
 * sy = w C, sx = C; any other non-negative strides, e.g. a channel slice of either, work too). */
#define SCAN_PACK_MAX_LEVELS 8
typedef struct {
  const float* data;
  int32_t h, w;
  int64_t sn, sc, sy, sx;
} scan_level_t;
/* replaces the flatten-and-concatenate in front of every loss (rpn/fcos/loss.py:191-202: permute(0, 2, 3, 1).reshape(-1, C)
 * per level, then torch.cat over the levels): rows [M, Cs] (M = N * sum_l h_l w_l, Cs >= C, Cs % 4 == 0), row order level ->
 * image -> y -> x, columns C..Cs-1 written as zeros; every element of rows is written exactly once, so it may be
 * uninitialised.  levels: HOST array of n_levels <= SCAN_PACK_MAX_LEVELS descriptors (copied into the kernel arguments). */
int scan_pyramid_pack(const scan_level_t* levels, int32_t n_levels, int32_t n_images, int32_t C, float* rows, int32_t Cs,
                      void* stream);
/* the exact inverse, and the adjoint (the gradient of the flatten-and-concatenate of rpn/fcos/loss.py:191-202 w.r.t. the
 * level tensors): columns 0..C-1 of every row go to element (n, c, y, x) of its level tensor (levels[l].data is WRITTEN here;
 * every element of the level tensors once), padding columns are ignored. */
int scan_pyramid_unpack(const float* rows, int32_t Cs, const scan_level_t* levels, int32_t n_levels, int32_t n_images,
                        int32_t C, void* stream);

/* ---- deformable convolution v2 (DCNv2), the sampling half ----
 * The reference exports fcos_core.layers.DFConv2d (layers/misc.py:113-184) but holds no arithmetic for it (it imports an absent
 * package), so these kernels implement the published definition (Zhu et al., "Deformable ConvNets v2", 2019; the mmcv /
 * torchvision deform_conv2d semantics): 3x3 kernel, stride 1, padding 1, dilation 1, one group, one deformable group, input
 * and output on one pyramid.  For output row m = (level l, image n, y, x) and tap k = 3 i + j:
 *   h = float(y - 1 + i) + off[m][2k],  w = float(x - 1 + j) + off[m][2k + 1]      (dy first; ONE fp32 add each)
 *   val[c] = 0 when h <= -1 || w <= -1 || h >= H_l || w >= W_l (decided in floating point), otherwise the bilinear sample of
 *            x on the cell [floor h, floor h + 1] x [floor w, floor w + 1], a corner outside the image counting zero
 *   cols[m][k * Cs + c] = mask[m][k] * val[c]   (mask == NULL: 1, plain DCNv1); columns C..Cs-1 of every tap are zeros
 * The convolution itself is the library's 1x1 convolution over cols [M, 9 Cs] (scan_conv_plan with taps = 1), its gradients
 * the 1x1 data and weight gradients.  floor carries zero derivative: at integer positions the gradients are those of the cell
 * floor selects.  x: [M, Cs] rows; off: [M, ld_off >= 18]; mask: [M, ld_mask >= 9]; x, cols, dcols, dx 16-byte aligned.
 * Every element of cols is written. */
int scan_deform_sample_forward(const float* x, const scan_pyramid_t* d, int32_t C, int32_t Cs, const float* off, int32_t ld_off,
                               const float* mask, int32_t ld_mask, float* cols, void* stream);
/* layers/misc.py:113-184, gradients of the sampling above for dcols [M, 9 Cs]: doff [M, ld_doff >= 18] and dmask [M, ld_dmask
 * >= 9] (skipped when mask == NULL) are channel sums inside one wave in a fixed order, their columns past 18 / 9 are written as
 * zeros.  The data gradient is left as an inverted index instead of float atomics: for each of the 4 * 9 * M entries
 * e = (m * 9 + k) * 4 + corner (corner = 2 * (h high) + (w high)), keys[e] = the row of dx the corner adds to, or M for a
 * corner outside the image or a skipped tap, and wgts[e] = mask * bilinear weight.  The caller sorts the keys (stable) and
 * hands the permutation to the gather below. */
int scan_deform_sample_backward(const float* x, const scan_pyramid_t* d, int32_t C, int32_t Cs, const float* dcols, const float* off,
                                int32_t ld_off, const float* mask, int32_t ld_mask, float* doff, int32_t ld_doff, float* dmask,
                                int32_t ld_dmask, int32_t* keys, float* wgts, void* stream);
/* layers/misc.py:113-184, the data gradient of the DCNv2 definition above: dx[p][:] = sum over e = perm[s], s in
 * [seg_start[p], seg_start[p + 1]) in that order, of wgts[e] * dcols[e / 4][:], with dcols read as [9 M, Cs] rows.  perm: the
 * int64 permutation of a stable sort of keys; seg_start: M + 1 int64 first positions of the keys 0..M in the sorted order.
 * One wave per row of dx, every row written (zeros for an empty segment): the sum is bit-reproducible. */
int scan_deform_dx_gather(const float* dcols, const int64_t* perm, const int64_t* seg_start, const float* wgts, int64_t M, int32_t C,
                          int32_t Cs, float* dx, void* stream);

/* ---- centre-aware alignment of the EPM baseline (discriminator/fcos_head_discriminator_CA.py:56-124) ----
 * :61-69 for every row of a pyramid in one launch:
 *   atten[m] = sigmoid(weight * sigmoid(max_{c < C} cls[m * Cs + c]) * sigmoid(ctr[m * ctr_stride]))
 * (sigmoid increases, so the maximum of the class probabilities is the probability of the largest logit).  cls: rows of pitch
 * Cs >= C of which only the first C columns are read -- the padding columns of the conv that wrote them may hold anything.
 * sigmoid(x) = 1 / (1 + expf(-x)) with IEEE division; no reduction across rows: the same bits on every run. */
int scan_center_aware_map(const float* cls, int32_t Cs, int32_t C, const float* ctr, int64_t ctr_stride, float weight, int64_t M,
                          float* atten, void* stream);
/* :93 (atten_map * feature in front of the gradient-reversal layer) and layer.py:6-24 (its backward) for all levels of a pyramid
 * in one launch:  y[m][c] = fl(fl(s[l(m)] * a[m]) * x[m][c]) for c < C, l(m) = the level of row m; a == NULL: the factor is
 * s[l(m)] itself (one rounding in all).  s: HOST array of d->n_levels floats.  The forward runs with s = 1 (fl(1 * a) = a: the
 * product a * x rounded once), the backward with s[l] = -lambda_l on the gradient rows.  x, y: row pitches ldx, ldy >= C in
 * floats; C, ldx, ldy multiples of 4, x and y 16-byte aligned; columns >= C of y are left untouched. */
int scan_row_scale_levels(const float* x, int32_t ldx, const float* a, const float* s, const scan_pyramid_t* d, int32_t C, float* y,
                          int32_t ldy, void* stream);
/* the same with x given level by level: x_levels is a HOST array of d->n_levels device pointers to each level's first row (the
 * gradient tensors of a per-level split are separate allocations); a NULL level writes zeros into that level's rows of y. */
int scan_row_scale_levels_ptrs(const float* const* x_levels, int32_t ldx, const float* a, const float* s, const scan_pyramid_t* d,
                               int32_t C, float* y, int32_t ldy, void* stream);

/* ---- region pooling: ROIAlign, ROIPool and the FPN level mapper (csrc/vision.cpp:8-17, the two-stage half) ----
 * x: pyramid rows [M, Cs] (Cs % 4 == 0, 16-byte aligned, only columns 0..C-1 are read).  rois: [K, 5] floats (image index,
 * x1, y1, x2, y2); levels: K int32 level indices, or NULL: every ROI on level 0; scales: HOST array of d->n_levels spatial
 * scales (copied into the kernel arguments).  Outputs are channel-last [K, PH, PW, Cs], padding columns written as zeros,
 * every element written exactly once (they may be uninitialised); one launch covers all levels.  A single-level pyramid is
 * the reference's plain operator.  Additions where the reference reads out of bounds: a ROI whose image index (truncated
 * towards zero, as the reference's int conversion) is outside [0, n_images) or whose level is outside [0, n_levels) gives
 * zeros, argmax -1 and no gradient; K == 0 returns without a launch (the gradients: zeros).
 *
 * ROIAlign, aligned = False semantics, with s the scale of the ROI's level, H x W its size.  Every fp32 operation is rounded
 * on its own in the source's left-to-right order (what the reference's CPU build computes):
 *   start = x1 * s, roi_w = max(x2 * s - x1 * s, 1), bin_w = roi_w / PW (likewise h)
 *   g = sampling_ratio when > 0, otherwise ceil(roi_h / PH) and ceil(roi_w / PW) per axis (capped at 32768)
 *   y = start_h + ph * bin_h + (iy + 0.5f) * bin_h / g_h;  y < -1 || y > H || x < -1 || x > W (or NaN): the sample is 0
 *   y = max(y, 0), y_low = (int)y; y_low >= H - 1: y_low = y_high = H - 1, y = y_low; ly = y - y_low, hy = 1 - ly (same for x)
 *   sample = hy hx v1 + hy lx v2 + ly hx v3 + ly lx v4;  out = (sum of the g_h g_w samples, iy outer, ix inner) / (g_h g_w) */
/* modeling/poolers.py:31-42 (LevelMapper.__call__): levels[k] = clamp(floor(lvl0 + log2(sqrt(area) / s0 + eps)), k_min, k_max)
 * - k_min in fp32, area = (x2 - x1 + 1) * (y2 - y1 + 1) of boxes[k * ld .. + 3] (ld = 4: a box matrix; rois + 1 with ld = 5: a
 * ROI matrix).  k_min must be an integer.  A NaN (negative area) maps to level 0. */
int scan_roi_levels(const float* boxes, int32_t ld, int64_t K, float k_min, float k_max, float s0, float lvl0, float eps,
                    int32_t* levels, void* stream);
/* csrc/cuda/ROIAlign_cuda.cu:15-122,257-299 and the per-level loop of modeling/poolers.py:116-119: y [K, PH, PW, Cs] */
int scan_roi_align_forward(const float* x, const scan_pyramid_t* d, int32_t C, int32_t Cs, const float* rois, const int32_t* levels,
                           const float* scales, int64_t K, int32_t PH, int32_t PW, int32_t sampling_ratio, float* y, void* stream);
/* csrc/cuda/ROIAlign_cuda.cu:125-254,302-346: dx [M, Cs], every row written.  Each sample sends (dy * w_i) / count to its four
 * cells; the sum is formed per destination row in a fixed order (ROI, ph, iy, y corner, pw, ix, x corner) without float
 * atomics: the same bits on every run, for every sampling_ratio, no workspace and no host read. */
int scan_roi_align_backward(const float* dy, const scan_pyramid_t* d, int32_t C, int32_t Cs, const float* rois,
                            const int32_t* levels, const float* scales, int64_t K, int32_t PH, int32_t PW, int32_t sampling_ratio,
                            float* dx, void* stream);
/* ROIAlign_cuda.cu:99-112,22-57 made visible for tests: for every (ROI, bin) and iy, ix < gmax the position (y, x) as first
 * formed [K, PH, PW, gmax, gmax, 2], the weights w1..w4 [.., 4] and the cells y * W + x of the level [.., 4] (-1 and weight 0:
 * a dropped sample; iy >= g_h or ix >= g_w: position 0 too), and grid [K, 2] = (g_h, g_w), (0, 0) for a ROI outside. */
int scan_roi_align_samples(const scan_pyramid_t* d, const float* rois, const int32_t* levels, const float* scales, int64_t K,
                           int32_t PH, int32_t PW, int32_t sampling_ratio, int32_t gmax, int32_t* grid, float* pos, float* wgt,
                           int32_t* cell, void* stream);
/* csrc/cuda/ROIPool_cuda.cu:16-77,110-153: start = round(x1 * s) (half away from zero, clamped to +-2^29), roi_w = max(end -
 * start + 1, 1) in integers, bin = roi_w / PW in fp32, wstart = floor(pw * bin) + start, wend = ceil((pw + 1) * bin) + start,
 * both clipped to [0, W]; an empty bin gives 0 and argmax -1, otherwise the maximum from -FLT_MAX with a strict > in (h, w)
 * scan order.  y [K, PH, PW, Cs]; argmax [K, PH, PW, Cs] int32 = h * W + w of the level per channel (padding columns -1),
 * 16-byte aligned. */
int scan_roi_pool_forward(const float* x, const scan_pyramid_t* d, int32_t C, int32_t Cs, const float* rois, const int32_t* levels,
                          const float* scales, int64_t K, int32_t PH, int32_t PW, float* y, int32_t* argmax, void* stream);
/* csrc/cuda/ROIPool_cuda.cu:79-108,156-202: dx [M, Cs] += dy at the argmax (-1: nothing), summed per destination row over the
 * bins whose window contains it in ascending (ROI, ph, pw) order, without float atomics: the same bits on every run. */
int scan_roi_pool_backward(const float* dy, const int32_t* argmax, const scan_pyramid_t* d, int32_t C, int32_t Cs, const float* rois,
                           const int32_t* levels, const float* scales, int64_t K, int32_t PH, int32_t PW, float* dx, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SCAN_HIP_H */
