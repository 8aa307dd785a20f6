// The Fast R-CNN box head's device side (reference modeling/roi_heads/box_head/{loss.py, inference.py}, modeling/matcher.py
// without the low-quality rule, modeling/box_coder.py): the proposals' matcher, the compaction of the sampled proposals with
// their encoded targets, the fused cross-entropy + class-specific smooth-L1 loss, and the test-time softmax + decode.
//
// Proposals are padded per image as the ground truth is: props [N][P][4], np [N]; rows p >= np[n] take no part.  The sampler is
// scan_rpn_sample on a one-level pyramid of P x 1 rows per image with A = 1 (see the header block); nothing of it is here.
// Built with -ffp-contract=off: every fp32 operation is rounded on its own.
//
// Match: one thread per (image, proposal), the arithmetic of retina_labels_kernel without its low-quality pass.
// Gather: one workgroup per image; the image's first output row is the sum of the counts before it, the rows within the image
// come from a running block scan over P in chunks of 256 (wave ballots, no cap on P).  Every write is guarded by row < R.
// Loss, backward and decode: a wave per row of logits, lanes striding the C columns (any C >= 2, one kernel).
#include "common.h"
#include "boxes.h"
#include "anchors.h"

#define ROI_BOX_XFORM_CLIP 4.135166556742356f  // log(1000 / 16), box_coder.py:13

// ------------------------------------------------------------------ match
__global__ __launch_bounds__(256) void roi_box_match_kernel(const float* __restrict__ props, const int32_t* __restrict__ np, int N,
                                                            int P, const float* __restrict__ boxes,
                                                            const int64_t* __restrict__ glabels, const int32_t* __restrict__ ng,
                                                            int G, float bg, float fg, int32_t* __restrict__ labels,
                                                            int32_t* __restrict__ matched) {
  const int64_t total = (int64_t)N * P;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int n = (int)(i / P);
    const int p = (int)(i - (int64_t)n * P);
    int lab = -1, arg = 0;
    if (p < np[n]) {
      const float4 pr = reinterpret_cast<const float4*>(props)[i];
      int cnt = ng[n];
      cnt = cnt < G ? cnt : G;
      float best = -1.f;
      for (int g = 0; g < cnt; ++g) {
        const float v = boxlist_iou(*reinterpret_cast<const float4*>(boxes + ((int64_t)n * G + g) * 4), pr);
        if (v > best) {  // equal IoUs keep the smaller box index
          best = v;
          arg = g;
        }
      }
      lab = 0;
      if (cnt > 0) lab = best < bg ? 0 : (best < fg ? -1 : (int)glabels[(int64_t)n * G + arg]);
    }
    labels[i] = lab;
    matched[i] = lab > 0 ? arg : 0;
  }
}

extern "C" int scan_roi_box_match(const float* props, const int32_t* np, int32_t N, int32_t P, const float* boxes,
                                  const int64_t* glabels, const int32_t* ng, int32_t G, float bg_thr, float fg_thr,
                                  int32_t* labels_i32, int32_t* matched, void* stream) {
  SCAN_CHECK_ARG(props && np && boxes && glabels && ng && labels_i32 && matched, "roi_box_match: null pointer");
  SCAN_CHECK_ARG(N >= 1 && P >= 1 && G >= 1 && (int64_t)N * P < (1ll << 31), "roi_box_match: N=%d, P=%d, G=%d (>= 1, N P < 2^31)", N,
                 P, G);
  SCAN_CHECK_ARG(bg_thr <= fg_thr, "roi_box_match: bg threshold %g above fg threshold %g", (double)bg_thr, (double)fg_thr);
  SCAN_CHECK_ARG(((reinterpret_cast<uintptr_t>(props) | reinterpret_cast<uintptr_t>(boxes)) & 15) == 0,
                 "roi_box_match: props / boxes must be 16-byte aligned");
  hipLaunchKernelGGL(roi_box_match_kernel, dim3(grid_for((int64_t)N * P, 256)), dim3(256), 0, as_stream(stream), props, np, N, P,
                     boxes, glabels, ng, G, bg_thr, fg_thr, labels_i32, matched);
  SCAN_LAUNCH_CHECK("roi_box_match");
  return 0;
}

// ------------------------------------------------------------------ gather
struct RoiBoxWeights {
  float wx, wy, ww, wh;
};

__global__ __launch_bounds__(256) void roi_box_gather_kernel(const float* __restrict__ props, int N, int P,
                                                             const float* __restrict__ boxes, int G,
                                                             const int32_t* __restrict__ labels_in,
                                                             const int32_t* __restrict__ matched,
                                                             const uint8_t* __restrict__ sampled,
                                                             const int32_t* __restrict__ counts, RoiBoxWeights wt, int R,
                                                             float* __restrict__ rois, int32_t* __restrict__ labels_out,
                                                             float* __restrict__ reg_targets, int32_t* __restrict__ src) {
  __shared__ int red[4];
  __shared__ int wave_cnt[4];
  const int n = blockIdx.x;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  // the image's first row: the counts of the images before it
  int before = 0;
  for (int m = threadIdx.x; m < n; m += 256) before += counts[2 * m] + counts[2 * m + 1];
  before = wave_sum(before);
  if (lane == 0) red[wid] = before;
  __syncthreads();
  int64_t base = (int64_t)red[0] + red[1] + red[2] + red[3];
  for (int p0 = 0; p0 < P; p0 += 256) {  // uniform trip count: every thread meets both barriers
    const int p = p0 + (int)threadIdx.x;
    const int64_t i = (int64_t)n * P + p;
    const int s = p < P ? (int)sampled[i] : 0;
    const unsigned long long vote = __ballot(s != 0);
    const int below = __popcll(vote & ((1ull << lane) - 1ull));
    if (lane == 0) wave_cnt[wid] = __popcll(vote);
    __syncthreads();
    int before_wave = 0;
    for (int w = 0; w < wid; ++w) before_wave += wave_cnt[w];
    const int chunk = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
    const int64_t r = base + before_wave + below;
    if (s != 0 && r >= 0 && r < (int64_t)R) {
      const float4 pr = reinterpret_cast<const float4*>(props)[i];
      const int lab_in = labels_in[i];
      const int lab = (s == 1 && lab_in > 0) ? lab_in : 0;
      float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
      if (lab > 0) {
        int g = matched[i];
        g = g < 0 ? 0 : (g < G ? g : G - 1);  // never read out of bounds, whatever the plan holds
        t = box_encode4(*reinterpret_cast<const float4*>(boxes + ((int64_t)n * G + g) * 4), pr, (double)wt.wx, (double)wt.wy,
                        (double)wt.ww, (double)wt.wh);
      }
      float* ro = rois + r * 5;
      ro[0] = (float)n;
      ro[1] = pr.x;
      ro[2] = pr.y;
      ro[3] = pr.z;
      ro[4] = pr.w;
      labels_out[r] = lab;
      reinterpret_cast<float4*>(reg_targets)[r] = t;
      src[r] = p;
    }
    base += chunk;
    __syncthreads();
  }
}

extern "C" int scan_roi_box_gather(const float* props, int32_t N, int32_t P, const float* boxes, int32_t G,
                                   const int32_t* labels_i32, const int32_t* matched, const uint8_t* sampled, const int32_t* counts,
                                   float wx, float wy, float ww, float wh, int32_t R, float* rois, int32_t* labels_out,
                                   float* reg_targets, int32_t* src, void* stream) {
  SCAN_CHECK_ARG(props && boxes && labels_i32 && matched && sampled && counts, "roi_box_gather: null input");
  SCAN_CHECK_ARG(N >= 1 && P >= 1 && G >= 1 && (int64_t)N * P < (1ll << 31), "roi_box_gather: N=%d, P=%d, G=%d (>= 1, N P < 2^31)",
                 N, P, G);
  SCAN_CHECK_ARG(R >= 0 && (int64_t)R <= (int64_t)N * P, "roi_box_gather: R=%d rows for %lld proposals", R, (long long)N * P);
  SCAN_CHECK_ARG(wx > 0.f && wy > 0.f && ww > 0.f && wh > 0.f, "roi_box_gather: the box coder's weights must be positive");
  if (R == 0) return 0;
  SCAN_CHECK_ARG(rois && labels_out && reg_targets && src, "roi_box_gather: null output");
  SCAN_CHECK_ARG(((reinterpret_cast<uintptr_t>(props) | reinterpret_cast<uintptr_t>(boxes) | reinterpret_cast<uintptr_t>(reg_targets)) &
                  15) == 0,
                 "roi_box_gather: props / boxes / reg_targets must be 16-byte aligned");
  RoiBoxWeights wt = {wx, wy, ww, wh};
  hipLaunchKernelGGL(roi_box_gather_kernel, dim3(N), dim3(256), 0, as_stream(stream), props, N, P, boxes, G, labels_i32, matched,
                     sampled, counts, wt, R, rois, labels_out, reg_targets, src);
  SCAN_LAUNCH_CHECK("roi_box_gather");
  return 0;
}

// ------------------------------------------------------------------ loss
// reductions over the wave whose result every lane holds (xor butterflies: one fixed order)
__device__ __forceinline__ float roi_wave_max_all(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}
__device__ __forceinline__ float roi_wave_sum_all(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

struct RoiBoxLossArgs {
  const float* cls;
  int64_t ld_cls;
  const float* reg;
  int64_t ld_reg;
  int R, C, Cr;
  const int32_t* labels;
  const float* targets;
};

// max m of a row of C logits and s1 = sum of exp(x_j - m) over every j but the FIRST that attains m, in every lane: the row's
// sum of exponentials is 1 + s1 with the leading 1 exact, so log-sum-exp = m + log1p(s1) keeps its relative accuracy for a
// confident row, where the loss is s1 itself and 1 + s1 rounded to fp32 would have lost it
__device__ __forceinline__ void roi_row_softmax_stats(const float* __restrict__ x, int C, int lane, float* mx, float* s1) {
  float m = -INFINITY;
  for (int j = lane; j < C; j += 64) m = fmaxf(m, x[j]);
  m = roi_wave_max_all(m);
  int first = C;
  for (int j = lane; j < C; j += 64)
    if (x[j] == m && j < first) first = j;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const int o = __shfl_xor(first, off, 64);
    first = o < first ? o : first;
  }
  float s = 0.f;
  for (int j = lane; j < C; j += 64)
    if (j != first) s += expf(x[j] - m);
  *mx = m;
  *s1 = roi_wave_sum_all(s);
}

// the four regression columns of a positive row's label
__device__ __forceinline__ int roi_reg_col(int lab, int C, int Cr) { return Cr == C ? 4 * lab : 4; }

// one block per 32 rows, at most 256: a function of R alone, so the ordered sum is too
static inline int roi_box_loss_grid(int64_t R) {
  int64_t g = (R + 31) / 32;
  return (int)(g < 1 ? 1 : (g > 256 ? 256 : g));
}

template <bool ORD>
__global__ __launch_bounds__(256) void roi_box_loss_fwd_kernel(RoiBoxLossArgs p, float* __restrict__ out) {
  __shared__ float red[4];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  float ce = 0.f, reg = 0.f;  // lane 0 of every wave carries the wave's rows
  for (int r = blockIdx.x * 4 + wid; r < p.R; r += gridDim.x * 4) {
    const int lab = p.labels[r];
    if (lab < 0 || lab >= p.C) continue;  // no such class: the row takes no part (wave-uniform)
    const float* x = p.cls + (int64_t)r * p.ld_cls;
    float m, s;
    roi_row_softmax_stats(x, p.C, lane, &m, &s);
    if (lane == 0) {
      ce += log1pf(s) - (x[lab] - m);
      if (lab > 0) {
        const float4 v = *reinterpret_cast<const float4*>(p.reg + (int64_t)r * p.ld_reg + roi_reg_col(lab, p.C, p.Cr));
        const float4 t = reinterpret_cast<const float4*>(p.targets)[r];
        reg += (smooth_l1_elem(v.x, t.x, 1.f) + smooth_l1_elem(v.y, t.y, 1.f)) +
               (smooth_l1_elem(v.z, t.z, 1.f) + smooth_l1_elem(v.w, t.w, 1.f));
      }
    }
  }
  const float s0 = block_sum_256(ce, red);
  const float s1 = block_sum_256(reg, red);
  if (threadIdx.x == 0) {
    block_result<ORD>(out, 0, 2, s0);
    block_result<ORD>(out, 1, 2, s1);
  }
}

__global__ __launch_bounds__(256) void roi_box_loss_bwd_kernel(RoiBoxLossArgs p, const float* __restrict__ g_dev,
                                                               float* __restrict__ d_cls, int64_t ldo_cls, float* __restrict__ d_reg,
                                                               int64_t ldo_reg) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const float g0 = g_dev[0], g1 = g_dev[1];
  for (int r = blockIdx.x * 4 + wid; r < p.R; r += gridDim.x * 4) {
    const int lab = p.labels[r];
    const bool live = lab >= 0 && lab < p.C;
    const float* x = p.cls + (int64_t)r * p.ld_cls;
    float* dc = d_cls + (int64_t)r * ldo_cls;
    float m = 0.f, s = 1.f;
    if (live) {
      roi_row_softmax_stats(x, p.C, lane, &m, &s);
      s += 1.f;
    }
    for (int j = lane; j < p.C; j += 64) dc[j] = live ? g0 * (expf(x[j] - m) / s - (j == lab ? 1.f : 0.f)) : 0.f;
    const int col = (live && lab > 0) ? roi_reg_col(lab, p.C, p.Cr) : -4;
    float4 t = make_float4(0.f, 0.f, 0.f, 0.f), v = t;
    if (col >= 0) {
      v = *reinterpret_cast<const float4*>(p.reg + (int64_t)r * p.ld_reg + col);
      t = reinterpret_cast<const float4*>(p.targets)[r];
    }
    float4* dr = reinterpret_cast<float4*>(d_reg + (int64_t)r * ldo_reg);
    for (int q = lane; q < p.Cr; q += 64) {
      float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
      if (4 * q == col)
        o = make_float4(g1 * smooth_l1_grad(v.x, t.x, 1.f), g1 * smooth_l1_grad(v.y, t.y, 1.f), g1 * smooth_l1_grad(v.z, t.z, 1.f),
                        g1 * smooth_l1_grad(v.w, t.w, 1.f));
      dr[q] = o;
    }
  }
}

extern "C" int64_t scan_roi_box_loss_ordered_ws_floats(int64_t R) { return 2 * (int64_t)roi_box_loss_grid(R); }

static int roi_box_loss_args(RoiBoxLossArgs* p, const float* cls, int64_t ld_cls, const float* reg, int64_t ld_reg, int32_t R,
                             int32_t C, int32_t Cr, const int32_t* labels, const float* targets, const char* who) {
  SCAN_CHECK_ARG(R >= 0 && R <= (1 << 30) && C >= 2 && C <= (1 << 20) && (Cr == C || Cr == 2),
                 "%s: R=%d, C=%d classes, Cr=%d regression classes (0 <= R <= 2^30, 2 <= C <= 2^20, Cr = C or 2)", who, R, C, Cr);
  SCAN_CHECK_ARG(R == 0 || (cls && reg && labels && targets), "%s: null input", who);
  SCAN_CHECK_ARG(ld_cls >= (int64_t)C, "%s: class_logits row pitch %lld for %d classes", who, (long long)ld_cls, C);
  SCAN_CHECK_ARG(ld_reg >= 4 * (int64_t)Cr && (ld_reg & 3) == 0,
                 "%s: box_regression row pitch %lld for %d regression classes (a multiple of 4, >= 4 Cr)", who, (long long)ld_reg, Cr);
  SCAN_CHECK_ARG(((reinterpret_cast<uintptr_t>(reg) | reinterpret_cast<uintptr_t>(targets)) & 15) == 0 &&
                     (reinterpret_cast<uintptr_t>(cls) & 3) == 0,
                 "%s: box_regression / reg_targets must be 16-byte, class_logits 4-byte aligned", who);
  p->cls = cls;
  p->ld_cls = ld_cls;
  p->reg = reg;
  p->ld_reg = ld_reg;
  p->R = R;
  p->C = C;
  p->Cr = Cr;
  p->labels = labels;
  p->targets = targets;
  return 0;
}

template <bool ORD>
static int roi_box_loss_forward_launch(const float* cls, int64_t ld_cls, const float* reg, int64_t ld_reg, int32_t R, int32_t C,
                                       int32_t Cr, const int32_t* labels, const float* targets, float* out2, float* ws, void* stream,
                                       const char* who) {
  RoiBoxLossArgs p;
  if (roi_box_loss_args(&p, cls, ld_cls, reg, ld_reg, R, C, Cr, labels, targets, who)) return -1;
  SCAN_CHECK_ARG(out2 && (!ORD || ws), "%s: null output", who);
  const int grid = roi_box_loss_grid(R);  // R = 0: one block that adds (or stores) two zeros
  hipLaunchKernelGGL(roi_box_loss_fwd_kernel<ORD>, dim3(grid), dim3(256), 0, as_stream(stream), p, ORD ? ws : out2);
  SCAN_LAUNCH_CHECK(ORD ? "roi_box_loss_fwd_ordered" : "roi_box_loss_fwd");
  return ORD ? ordered_sum_launch(ws, grid, 2, out2, 0, nullptr, stream, "roi_box_loss_fwd_ordered_sum") : 0;
}

extern "C" int scan_roi_box_loss_forward(const float* class_logits, int64_t ld_cls, const float* box_regression, int64_t ld_reg,
                                         int32_t R, int32_t C, int32_t Cr, const int32_t* labels, const float* reg_targets,
                                         float* out2, void* stream) {
  return roi_box_loss_forward_launch<false>(class_logits, ld_cls, box_regression, ld_reg, R, C, Cr, labels, reg_targets, out2,
                                            nullptr, stream, "roi_box_loss_forward");
}

extern "C" int scan_roi_box_loss_forward_ordered(const float* class_logits, int64_t ld_cls, const float* box_regression,
                                                 int64_t ld_reg, int32_t R, int32_t C, int32_t Cr, const int32_t* labels,
                                                 const float* reg_targets, float* out2, float* ws, void* stream) {
  return roi_box_loss_forward_launch<true>(class_logits, ld_cls, box_regression, ld_reg, R, C, Cr, labels, reg_targets, out2, ws,
                                           stream, "roi_box_loss_forward_ordered");
}

extern "C" int scan_roi_box_loss_backward(const float* class_logits, int64_t ld_cls, const float* box_regression, int64_t ld_reg,
                                          int32_t R, int32_t C, int32_t Cr, const int32_t* labels, const float* reg_targets,
                                          const float* g2_dev, float* d_cls, int64_t ldo_cls, float* d_reg, int64_t ldo_reg,
                                          void* stream) {
  RoiBoxLossArgs p;
  if (roi_box_loss_args(&p, class_logits, ld_cls, box_regression, ld_reg, R, C, Cr, labels, reg_targets, "roi_box_loss_backward"))
    return -1;
  if (R == 0) return 0;
  SCAN_CHECK_ARG(g2_dev && d_cls && d_reg && (reinterpret_cast<uintptr_t>(d_reg) & 15) == 0 && ldo_cls >= (int64_t)C &&
                     ldo_reg >= 4 * (int64_t)Cr && (ldo_reg & 3) == 0,
                 "roi_box_loss_backward: null or misaligned gradient pointer, or a bad pitch");
  hipLaunchKernelGGL(roi_box_loss_bwd_kernel, dim3(grid_for((int64_t)R * 64, 256)), dim3(256), 0, as_stream(stream), p, g2_dev, d_cls,
                     ldo_cls, d_reg, ldo_reg);
  SCAN_LAUNCH_CHECK("roi_box_loss_bwd");
  return 0;
}

// ------------------------------------------------------------------ test-time softmax + decode
__global__ __launch_bounds__(256) void roi_box_decode_kernel(const float* __restrict__ cls, int64_t ld_cls, const float* __restrict__ reg,
                                                             int64_t ld_reg, int R, int C, int Cr, const float* __restrict__ rois,
                                                             const int32_t* __restrict__ image_hw, int N, RoiBoxWeights wt,
                                                             float thr, float* __restrict__ scores, float* __restrict__ boxes,
                                                             uint8_t* __restrict__ cand) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  for (int r = blockIdx.x * 4 + wid; r < R; r += gridDim.x * 4) {
    const float* ro = rois + (int64_t)r * 5;
    const float fn = ro[0];
    const bool live = fn >= 0.f && fn < (float)N;  // (a NaN index is not live)
    float* so = scores + (int64_t)r * C;
    float4* bo = reinterpret_cast<float4*>(boxes) + (int64_t)r * C;
    uint8_t* co = cand + (int64_t)r * C;
    if (!live) {
      for (int j = lane; j < C; j += 64) {
        so[j] = 0.f;
        bo[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        co[j] = 0;
      }
      continue;
    }
    const int n = (int)fn;
    const float* x = cls + (int64_t)r * ld_cls;
    float m, s;
    roi_row_softmax_stats(x, C, lane, &m, &s);
    s += 1.f;
    const float w = ro[3] - ro[1] + 1.f, h = ro[4] - ro[2] + 1.f;
    const float cx = ro[1] + 0.5f * w, cy = ro[2] + 0.5f * h;
    const float xmax = (float)(image_hw[2 * n + 1] - 1), ymax = (float)(image_hw[2 * n] - 1);
    for (int j = lane; j < C; j += 64) {
      const float sc = expf(x[j] - m) / s;
      const float4 t = *reinterpret_cast<const float4*>(reg + (int64_t)r * ld_reg + (Cr == C ? 4 * j : 4));
      const float dx = t.x / wt.wx, dy = t.y / wt.wy;
      const float dw = fminf(t.z / wt.ww, ROI_BOX_XFORM_CLIP), dh = fminf(t.w / wt.wh, ROI_BOX_XFORM_CLIP);
      const float pcx = dx * w + cx, pcy = dy * h + cy;
      const float pw = expf(dw) * w, ph = expf(dh) * h;
      float4 o;
      o.x = fminf(fmaxf(pcx - 0.5f * pw, 0.f), xmax);
      o.y = fminf(fmaxf(pcy - 0.5f * ph, 0.f), ymax);
      o.z = fminf(fmaxf(pcx + 0.5f * pw - 1.f, 0.f), xmax);
      o.w = fminf(fmaxf(pcy + 0.5f * ph - 1.f, 0.f), ymax);
      so[j] = sc;
      bo[j] = o;
      co[j] = (j >= 1 && sc > thr) ? 1 : 0;
    }
  }
}

extern "C" int scan_roi_box_decode(const float* class_logits, int64_t ld_cls, const float* box_regression, int64_t ld_reg, int32_t R,
                                   int32_t C, int32_t Cr, const float* rois, const int32_t* image_hw, int32_t N, float wx, float wy,
                                   float ww, float wh, float score_thresh, float* scores, float* boxes, uint8_t* cand, void* stream) {
  SCAN_CHECK_ARG(R >= 0 && R <= (1 << 30) && C >= 2 && C <= (1 << 20) && (Cr == C || Cr == 2) && N >= 1,
                 "roi_box_decode: R=%d, C=%d classes, Cr=%d regression classes, N=%d images", R, C, Cr, N);
  if (R == 0) return 0;
  SCAN_CHECK_ARG(class_logits && box_regression && rois && image_hw && scores && boxes && cand, "roi_box_decode: null pointer");
  SCAN_CHECK_ARG(ld_cls >= (int64_t)C, "roi_box_decode: class_logits row pitch %lld for %d classes", (long long)ld_cls, C);
  SCAN_CHECK_ARG(ld_reg >= 4 * (int64_t)Cr && (ld_reg & 3) == 0,
                 "roi_box_decode: box_regression row pitch %lld for %d regression classes (a multiple of 4, >= 4 Cr)",
                 (long long)ld_reg, Cr);
  SCAN_CHECK_ARG(((reinterpret_cast<uintptr_t>(box_regression) | reinterpret_cast<uintptr_t>(boxes)) & 15) == 0,
                 "roi_box_decode: box_regression / boxes must be 16-byte aligned");
  SCAN_CHECK_ARG(wx > 0.f && wy > 0.f && ww > 0.f && wh > 0.f, "roi_box_decode: the box coder's weights must be positive");
  RoiBoxWeights wt = {wx, wy, ww, wh};
  hipLaunchKernelGGL(roi_box_decode_kernel, dim3(grid_for((int64_t)R * 64, 256)), dim3(256), 0, as_stream(stream), class_logits, ld_cls,
                     box_regression, ld_reg, R, C, Cr, rois, image_hw, N, wt, score_thresh, scores, boxes, cand);
  SCAN_LAUNCH_CHECK("roi_box_decode");
  return 0;
}
