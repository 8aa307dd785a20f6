// The RetinaNet head's device side: the IoU-threshold ground-truth plan (reference modeling/matcher.py:42-112 with
// allow_low_quality_matches, called from rpn/loss.py:42-89 by rpn/retinanet/loss.py:43-80) and the smooth-L1 regression loss
// (layers/smooth_l1_loss.py) fused with BoxCoder.encode (modeling/box_coder.py:22-50).
//
// A anchors per location (1..16).  Pyramid row m = (level, image, y, x) holds the anchors cell[level][a] + (x s, y s, x s, y s),
// a < A; anchor index i = m * A + a, which is the reference's order level by level (a head output row [A * C] is A anchors of C
// classes).  The anchors are never stored: every kernel forms them from the row and the cell table [n_levels][A][4], a tiny
// device buffer.  This file is built with -ffp-contract=off: the IoU is boxlist_iou's (structures/boxlist_ops.py) in fp32 with
// every operation rounded on its own (boxes.h), so its bits are torch-CPU's, and the two passes below recompute identical bits.
//
// The plan, per image n with ng[n] real boxes (padding boxes beyond ng[n] take no part; ng[n] = 0: all background, where the
// reference raises):
//   pass 1  gt_max[n][g] = max over the image's anchors of IoU(anchor, box g): an integer max of the IoU's bits (IoU >= 0, so
//           the order is preserved), reduced within the wave before one global atomic
//   pass 2  per anchor the max and argmax over g (equal IoUs: the smaller box index);
//           max < bg: label 0;  bg <= max < fg: label -1;  otherwise the class of the argmax box;
//           an anchor whose IoU with SOME real box equals that box's gt_max gets the class of its OWN argmax box, whatever its
//           IoU (set_low_quality_matches_ to the letter: ties included, and a box that overlaps no anchor has gt_max 0, which
//           every anchor that misses it equals)
//           matched = the argmax box where label > 0, else 0; one device counter of the anchors with label > 0
// Integer atomics only: the plan is bit-reproducible with scan_tune "deterministic" on or off and has no *_ordered twin.
//
// Smooth-L1 runs over ALL anchors, no compaction: where label > 0 the target is encode(boxes[n][matched], anchor) with weights
// (10, 10, 5, 5) and TO_REMOVE = 1, formed in fp64 and rounded to fp32 once (as scan_atss_targets), compared with the four
// columns [4a, 4a + 4) of row m of bbox_reg (row pitch ld floats); loss = 0.5 d^2 / beta where |d| < beta, |d| - 0.5 beta
// elsewhere, summed (block_result<ORD>; the ordered twin's second stage is ordered_sum_launch of losses.hip).  The backward
// writes d_pred for every anchor (zero where label <= 0).
//
// Per-level selects, the pyramid check and the wave reductions are common.h's; boxlist_iou is boxes.h's (box first here); the
// anchor of a row, BoxCoder.encode and the smooth-L1 element are anchors.h's (shared with rpn.hip).
#include "common.h"
#include "boxes.h"
#include "anchors.h"

// pass 1: gt_max[n * G + g] (zeroed by the caller).  All 64 lanes of a wave stay in the loop together (the shuffles need them).
__global__ __launch_bounds__(256) void retina_gtmax_kernel(scan_pyramid_t d, RetinaStrides st, const float* __restrict__ cells,
                                                           int A, const float* __restrict__ boxes, const int32_t* __restrict__ ng,
                                                           int G, unsigned* __restrict__ gt_max) {
  const int64_t total = d.row_off[d.n_levels] * A;
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  const int64_t rounds = (total + step - 1) / step;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (int64_t r = 0; r < rounds; ++r, i += step) {
    const bool live = i < total;
    int n = -1, cnt = 0;
    float4 an = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live) {
      const int64_t m = i / A;
      const RowCoord rc = decode_row(d, m);
      n = rc.n;
      cnt = ng[n];
      cnt = cnt < G ? cnt : G;
      an = retina_anchor(st, cells, A, rc, (int)(i - m * A));
    }
    const int gmax = wave_max(cnt);
    const int n0 = __shfl(n, 0, 64);
    const bool uniform = __all(n == n0);  // every lane live and of one image: one atomic per box for the wave
    for (int g = 0; g < gmax; ++g) {
      unsigned v = 0u;
      if (g < cnt) v = __float_as_uint(boxlist_iou(*reinterpret_cast<const float4*>(boxes + ((int64_t)n * G + g) * 4), an));
      if (uniform) {
        const unsigned wv = wave_max(v);
        if ((threadIdx.x & 63) == 0 && wv != 0u) atomicMax(&gt_max[(int64_t)n0 * G + g], wv);
      } else if (v != 0u) {
        atomicMax(&gt_max[(int64_t)n * G + g], v);
      }
    }
  }
}

// pass 2: labels, matched, the positive count
__global__ __launch_bounds__(256) void retina_labels_kernel(scan_pyramid_t d, RetinaStrides st, const float* __restrict__ cells,
                                                            int A, const float* __restrict__ boxes,
                                                            const int64_t* __restrict__ glabels, const int32_t* __restrict__ ng,
                                                            int G, float bg, float fg, const unsigned* __restrict__ gt_max,
                                                            int32_t* __restrict__ labels, int32_t* __restrict__ matched,
                                                            int32_t* __restrict__ n_pos) {
  __shared__ int red[4];
  const int64_t total = d.row_off[d.n_levels] * A;
  int pos = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t m = i / A;
    const RowCoord rc = decode_row(d, m);
    const float4 an = retina_anchor(st, cells, A, rc, (int)(i - m * A));
    int cnt = ng[rc.n];
    cnt = cnt < G ? cnt : G;
    float best = -1.f;
    int arg = 0;
    bool low = false;
    for (int g = 0; g < cnt; ++g) {
      const float v = boxlist_iou(*reinterpret_cast<const float4*>(boxes + ((int64_t)rc.n * G + g) * 4), an);
      if (v > best) {
        best = v;
        arg = g;
      }
      low |= __float_as_uint(v) == gt_max[(int64_t)rc.n * G + g];
    }
    int lab = 0;
    if (cnt > 0) {
      const int cls = (int)glabels[(int64_t)rc.n * G + arg];
      lab = best < bg ? 0 : (best < fg ? -1 : cls);
      if (low) lab = cls;
    }
    labels[i] = lab;
    matched[i] = lab > 0 ? arg : 0;
    pos += lab > 0 ? 1 : 0;
  }
  pos = wave_sum(pos);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = pos;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int s = red[0] + red[1] + red[2] + red[3];
    if (s) atomicAdd(n_pos, s);
  }
}

extern "C" int64_t scan_retina_match_ws_bytes(const scan_pyramid_t* d, int32_t G) {
  if (!d || d->n_images < 1 || G < 1) return -1;
  return 4 * (int64_t)d->n_images * G;  // gt_max
}

extern "C" int scan_retina_match(const scan_pyramid_t* d, const int32_t* strides, const float* cells, int32_t A,
                                 const float* boxes, const int64_t* glabels, const int32_t* ng, int32_t G, float bg_thr,
                                 float fg_thr, int32_t* labels_i32, int32_t* matched, int32_t* n_pos, void* ws, void* stream) {
  RetinaStrides st;
  if (retina_check(d, strides, cells, A, &st, "retina_match")) return -1;
  SCAN_CHECK_ARG(boxes && glabels && ng && labels_i32 && matched && n_pos && ws, "retina_match: null pointer");
  SCAN_CHECK_ARG(G >= 1, "retina_match: G=%d < 1", G);
  SCAN_CHECK_ARG(bg_thr <= fg_thr, "retina_match: bg threshold %g above fg threshold %g", (double)bg_thr, (double)fg_thr);
  SCAN_CHECK_ARG((reinterpret_cast<uintptr_t>(boxes) & 15) == 0 && (reinterpret_cast<uintptr_t>(ws) & 3) == 0,
                 "retina_match: boxes must be 16-byte, ws 4-byte aligned");
  hipStream_t s = as_stream(stream);
  unsigned* gt_max = reinterpret_cast<unsigned*>(ws);
  if (hipMemsetAsync(gt_max, 0, 4 * (size_t)d->n_images * G, s) != hipSuccess ||
      hipMemsetAsync(n_pos, 0, sizeof(int32_t), s) != hipSuccess) {
    scan_set_error("retina_match: memset failed");
    return -2;
  }
  const int64_t total = d->row_off[d->n_levels] * A;
  const int grid = grid_for(total, 256);
  hipLaunchKernelGGL(retina_gtmax_kernel, dim3(grid), dim3(256), 0, s, *d, st, cells, A, boxes, ng, G, gt_max);
  SCAN_LAUNCH_CHECK("retina_gtmax");
  hipLaunchKernelGGL(retina_labels_kernel, dim3(grid), dim3(256), 0, s, *d, st, cells, A, boxes, glabels, ng, G, bg_thr, fg_thr,
                     gt_max, labels_i32, matched, n_pos);
  SCAN_LAUNCH_CHECK("retina_labels");
  return 0;
}

// ------------------------------------------------------------------ smooth-L1 on encoded targets
struct SmoothL1Args {
  scan_pyramid_t d;
  RetinaStrides st;
  const float* cells;
  int A;
  const float* boxes;
  int G;
  const int32_t* labels;
  const int32_t* matched;
  const float* pred;
  int64_t ld;
  float beta;
};

// the target of anchor i (label > 0) and its prediction
__device__ __forceinline__ void smooth_l1_pair(const SmoothL1Args& p, int64_t i, float4* t, float4* x, int64_t* col0) {
  const int64_t m = i / p.A;
  const int a = (int)(i - m * p.A);
  const RowCoord rc = decode_row(p.d, m);
  const float4 an = retina_anchor(p.st, p.cells, p.A, rc, a);
  int g = p.matched[i];
  g = g < 0 ? 0 : (g < p.G ? g : p.G - 1);  // a plan of scan_retina_match is inside already: never read out of bounds
  const float4 b = *reinterpret_cast<const float4*>(p.boxes + ((int64_t)rc.n * p.G + g) * 4);
  *t = box_encode(b, an, 10.0, 5.0);  // weights (10, 10, 5, 5)
  *col0 = m * p.ld + 4 * a;
  *x = *reinterpret_cast<const float4*>(p.pred + *col0);
}

// ORD: every block writes its sum to its own slot out[blockIdx.x] instead of adding it to out[0] (block_result)
template <bool ORD>
__global__ __launch_bounds__(256) void smooth_l1_fwd_kernel(SmoothL1Args p, float* __restrict__ targets_out, float* __restrict__ out) {
  __shared__ float red[4];
  const int64_t total = p.d.row_off[p.d.n_levels] * p.A;
  float acc = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
    if (p.labels[i] > 0) {
      float4 x;
      int64_t c0;
      smooth_l1_pair(p, i, &t, &x, &c0);
      acc += (smooth_l1_elem(x.x, t.x, p.beta) + smooth_l1_elem(x.y, t.y, p.beta)) +
             (smooth_l1_elem(x.z, t.z, p.beta) + smooth_l1_elem(x.w, t.w, p.beta));
    }
    if (targets_out != nullptr) reinterpret_cast<float4*>(targets_out)[i] = t;
  }
  const float s = block_sum_256(acc, red);
  if (threadIdx.x == 0) block_result<ORD>(out, 0, 1, s);
}

__global__ __launch_bounds__(256) void smooth_l1_bwd_kernel(SmoothL1Args p, const float* __restrict__ g_dev,
                                                            float* __restrict__ d_pred, int64_t ld_out) {
  const int64_t total = p.d.row_off[p.d.n_levels] * p.A;
  const float g = g_dev[0];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    const int64_t m = i / p.A;
    if (p.labels[i] > 0) {
      float4 t, x;
      int64_t c0;
      smooth_l1_pair(p, i, &t, &x, &c0);
      o = make_float4(g * smooth_l1_grad(x.x, t.x, p.beta), g * smooth_l1_grad(x.y, t.y, p.beta),
                      g * smooth_l1_grad(x.z, t.z, p.beta), g * smooth_l1_grad(x.w, t.w, p.beta));
    }
    *reinterpret_cast<float4*>(d_pred + m * ld_out + 4 * (i - m * p.A)) = o;
  }
}

extern "C" int64_t scan_retina_smooth_l1_ordered_ws_floats(int64_t n_anchors) { return head_loss_grid(n_anchors); }

static int smooth_l1_args(SmoothL1Args* p, const scan_pyramid_t* d, const int32_t* strides, const float* cells, int32_t A,
                          const float* boxes, int32_t G, const int32_t* labels, const int32_t* matched, const float* pred,
                          int64_t ld, float beta, const char* who) {
  if (retina_check(d, strides, cells, A, &p->st, who)) return -1;
  SCAN_CHECK_ARG(boxes && labels && matched && pred, "%s: null input", who);
  SCAN_CHECK_ARG(G >= 1, "%s: G=%d < 1", who, G);
  SCAN_CHECK_ARG(ld >= 4 * (int64_t)A && (ld & 3) == 0, "%s: row pitch %lld for %d anchors (a multiple of 4, >= 4 A)", who,
                 (long long)ld, A);
  SCAN_CHECK_ARG(((reinterpret_cast<uintptr_t>(boxes) | reinterpret_cast<uintptr_t>(pred)) & 15) == 0,
                 "%s: boxes / pred must be 16-byte aligned", who);
  SCAN_CHECK_ARG(beta > 0.f, "%s: beta=%g must be positive", who, (double)beta);
  p->d = *d;
  p->cells = cells;
  p->A = A;
  p->boxes = boxes;
  p->G = G;
  p->labels = labels;
  p->matched = matched;
  p->pred = pred;
  p->ld = ld;
  p->beta = beta;
  return 0;
}

template <bool ORD>
static int smooth_l1_forward_launch(const scan_pyramid_t* d, const int32_t* strides, const float* cells, int32_t A,
                                    const float* boxes, int32_t G, const int32_t* labels, const int32_t* matched,
                                    const float* pred, int64_t ld, float beta, float* targets_out, float* out, float* ws,
                                    void* stream, const char* who) {
  SmoothL1Args p;
  if (smooth_l1_args(&p, d, strides, cells, A, boxes, G, labels, matched, pred, ld, beta, who)) return -1;
  SCAN_CHECK_ARG(out && (!ORD || ws), "%s: null output", who);
  SCAN_CHECK_ARG((reinterpret_cast<uintptr_t>(targets_out) & 15) == 0, "%s: targets_out must be 16-byte aligned", who);
  const int grid = head_loss_grid(d->row_off[d->n_levels] * A);
  hipLaunchKernelGGL(smooth_l1_fwd_kernel<ORD>, dim3(grid), dim3(256), 0, as_stream(stream), p, targets_out, ORD ? ws : out);
  SCAN_LAUNCH_CHECK(ORD ? "retina_smooth_l1_fwd_ordered" : "retina_smooth_l1_fwd");
  return ORD ? ordered_sum_launch(ws, grid, 1, out, 0, nullptr, stream, "retina_smooth_l1_fwd_ordered_sum") : 0;
}

extern "C" int scan_retina_smooth_l1_forward(const scan_pyramid_t* d, const int32_t* strides, const float* cells, int32_t A,
                                             const float* boxes, int32_t G, const int32_t* labels_i32, const int32_t* matched,
                                             const float* bbox_reg, int64_t ld, float beta, float* targets_out, float* out,
                                             void* stream) {
  return smooth_l1_forward_launch<false>(d, strides, cells, A, boxes, G, labels_i32, matched, bbox_reg, ld, beta, targets_out, out,
                                         nullptr, stream, "retina_smooth_l1_forward");
}

extern "C" int scan_retina_smooth_l1_forward_ordered(const scan_pyramid_t* d, const int32_t* strides, const float* cells,
                                                     int32_t A, const float* boxes, int32_t G, const int32_t* labels_i32,
                                                     const int32_t* matched, const float* bbox_reg, int64_t ld, float beta,
                                                     float* targets_out, float* out, float* ws, void* stream) {
  return smooth_l1_forward_launch<true>(d, strides, cells, A, boxes, G, labels_i32, matched, bbox_reg, ld, beta, targets_out, out,
                                        ws, stream, "retina_smooth_l1_forward_ordered");
}

extern "C" int scan_retina_smooth_l1_backward(const scan_pyramid_t* d, const int32_t* strides, const float* cells, int32_t A,
                                              const float* boxes, int32_t G, const int32_t* labels_i32, const int32_t* matched,
                                              const float* bbox_reg, int64_t ld, float beta, const float* g_dev, float* d_pred,
                                              int64_t ld_out, void* stream) {
  SmoothL1Args p;
  if (smooth_l1_args(&p, d, strides, cells, A, boxes, G, labels_i32, matched, bbox_reg, ld, beta, "retina_smooth_l1_backward"))
    return -1;
  SCAN_CHECK_ARG(g_dev && d_pred && (reinterpret_cast<uintptr_t>(d_pred) & 15) == 0 && ld_out >= 4 * (int64_t)A && (ld_out & 3) == 0,
                 "retina_smooth_l1_backward: null or misaligned gradient pointer, or a bad pitch");
  hipLaunchKernelGGL(smooth_l1_bwd_kernel, dim3(grid_for(d->row_off[d->n_levels] * A, 256)), dim3(256), 0, as_stream(stream), p,
                     g_dev, d_pred, ld_out);
  SCAN_LAUNCH_CHECK("retina_smooth_l1_bwd");
  return 0;
}
