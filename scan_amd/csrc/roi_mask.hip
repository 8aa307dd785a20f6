// The Mask R-CNN mask head's device side (reference modeling/roi_heads/mask_head/{mask_head.py, loss.py, inference.py},
// structures/segmentation_mask.py in binary-mask mode): the compaction of the box plan's positive rows, the mask targets
// (crop + bilinear resize + truncation to uint8, decided in integers), the binary cross-entropy on the label's channel with its
// backward, the test-time sigmoid of the predicted class's channel, and Masker's paste into the image.
//
// No float atomics, and every output element is written by its kernel: nothing here needs a cleared buffer.
// Built with -ffp-contract=off: the paste's box expansion and interpolation are fp32 operations in the reference's order, each
// rounded on its own.
//
// Ground-truth masks: ONE flat uint8 buffer; image n owns bytes [moff[n], moff[n + 1]) as [G_n][h_n][w_n] (mhw[n] = (h_n, w_n)),
// no padding to a common size, values 0 / 1.
#include "common.h"

// a float coordinate -> int by the rule given (rintf: half-to-even, Python's round(float); truncf: .to(torch.int32)), with NaN
// as 0 and the range held inside int32 first
__device__ __forceinline__ int roi_mask_rint(float v) {
  v = v == v ? v : 0.f;
  return (int)rintf(fminf(fmaxf(v, -1.0e9f), 1.0e9f));
}
__device__ __forceinline__ int roi_mask_trunc(float v) {
  v = v == v ? v : 0.f;
  return (int)fminf(fmaxf(v, -1.0e9f), 1.0e9f);
}
__device__ __forceinline__ int roi_mask_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ------------------------------------------------------------------ positives
// one workgroup: a running block scan over R in chunks of 256 (wave ballots, no cap on R); every write guarded by row < Rp
__global__ __launch_bounds__(256) void roi_mask_positives_kernel(const int32_t* __restrict__ labels, const float* __restrict__ rois,
                                                                 const int32_t* __restrict__ src, const int32_t* __restrict__ matched,
                                                                 int N, int P, int R, int Rp, int32_t* __restrict__ pos_rows,
                                                                 float* __restrict__ pos_rois, int32_t* __restrict__ pos_labels,
                                                                 int32_t* __restrict__ pos_gt) {
  __shared__ int wave_cnt[4];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  int64_t base = 0;
  for (int r0 = 0; r0 < R; r0 += 256) {  // uniform trip count: every thread meets both barriers
    const int r = r0 + (int)threadIdx.x;
    const int lab = r < R ? labels[r] : 0;
    const unsigned long long vote = __ballot(lab > 0);
    const int below = __popcll(vote & ((1ull << lane) - 1ull));
    if (lane == 0) wave_cnt[wid] = __popcll(vote);
    __syncthreads();
    int before_wave = 0;
    for (int w = 0; w < wid; ++w) before_wave += wave_cnt[w];
    const int chunk = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
    const int64_t o = base + before_wave + below;
    if (lab > 0 && o < (int64_t)Rp) {
      const float* ri = rois + (int64_t)r * 5;
      float* ro = pos_rois + o * 5;
      const float fn = ri[0];
      ro[0] = fn;
      ro[1] = ri[1];
      ro[2] = ri[2];
      ro[3] = ri[3];
      ro[4] = ri[4];
      int g = 0;
      if (fn >= 0.f && fn < (float)N) {  // (a NaN index is not in range)
        const int p = src[r];
        if (p >= 0 && p < P) g = matched[(int64_t)(int)fn * P + p];  // never read out of bounds, whatever the plan holds
      }
      pos_rows[o] = r;
      pos_labels[o] = lab;
      pos_gt[o] = g;
    }
    base += chunk;
    __syncthreads();
  }
}

extern "C" int scan_roi_mask_positives(const int32_t* labels, const float* rois, const int32_t* src, const int32_t* matched, int32_t N,
                                       int32_t P, int32_t R, int32_t Rp, int32_t* pos_rows, float* pos_rois, int32_t* pos_labels,
                                       int32_t* pos_gt, void* stream) {
  SCAN_CHECK_ARG(N >= 1 && P >= 1 && (int64_t)N * P < (1ll << 31) && R >= 0 && Rp >= 0 && Rp <= R,
                 "roi_mask_positives: N=%d, P=%d, R=%d, Rp=%d (N, P >= 1, N P < 2^31, 0 <= Rp <= R)", N, P, R, Rp);
  if (Rp == 0) return 0;
  SCAN_CHECK_ARG(labels && rois && src && matched && pos_rows && pos_rois && pos_labels && pos_gt, "roi_mask_positives: null pointer");
  hipLaunchKernelGGL(roi_mask_positives_kernel, dim3(1), dim3(256), 0, as_stream(stream), labels, rois, src, matched, N, P, R, Rp,
                     pos_rows, pos_rois, pos_labels, pos_gt);
  SCAN_LAUNCH_CHECK("roi_mask_positives");
  return 0;
}

// ------------------------------------------------------------------ targets
// the first neighbour along an axis of crop length n for output index d of M, and whether the second (min(i0 + 1, n - 1)) has a
// nonzero exact weight: the source coordinate of align_corners=False is ((2 d + 1) n - M) / (2 M), clamped at 0
__device__ __forceinline__ int roi_mask_axis(int d, int n, int M, bool* second) {
  int64_t num = (int64_t)(2 * d + 1) * n - M;
  if (num < 0) num = 0;
  const int64_t den = 2 * (int64_t)M;
  *second = (num % den) != 0;
  return (int)(num / den);
}

__global__ __launch_bounds__(256) void roi_mask_targets_kernel(const float* __restrict__ rois, const int32_t* __restrict__ gt, int Rp,
                                                               const uint8_t* __restrict__ masks, int64_t total,
                                                               const int64_t* __restrict__ moff, const int32_t* __restrict__ mhw, int N,
                                                               int M, float* __restrict__ out) {
  const int64_t MM = (int64_t)M * M, work = (int64_t)Rp * MM;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < work; i += (int64_t)gridDim.x * blockDim.x) {
    const int r = (int)(i / MM);
    const int e = (int)(i - (int64_t)r * MM);
    const int dy = e / M, dx = e - dy * M;
    const float* ro = rois + (int64_t)r * 5;
    const float fn = ro[0];
    float v = 0.f;
    if (fn >= 0.f && fn < (float)N) {
      const int n = (int)fn;
      const int h = mhw[2 * n], w = mhw[2 * n + 1];
      const int64_t o0 = moff[n], o1 = moff[n + 1];
      const int64_t plane = (int64_t)h * w;
      const int64_t G = (h > 0 && w > 0 && o1 > o0) ? (o1 - o0) / plane : 0;
      if (G > 0 && o0 >= 0 && o0 + G * plane <= total) {
        int64_t g = gt[r];
        g = g < 0 ? 0 : (g < G ? g : G - 1);
        // BinaryMaskList.crop (segmentation_mask.py:89-108)
        const int xmin = roi_mask_clampi(roi_mask_rint(ro[1]), 0, w - 1), ymin = roi_mask_clampi(roi_mask_rint(ro[2]), 0, h - 1);
        int xmax = roi_mask_clampi(roi_mask_rint(ro[3]), 0, w), ymax = roi_mask_clampi(roi_mask_rint(ro[4]), 0, h);
        xmax = xmax > xmin + 1 ? xmax : xmin + 1;
        ymax = ymax > ymin + 1 ? ymax : ymin + 1;
        const int cw = xmax - xmin, ch = ymax - ymin;  // 1 <= cw <= w - xmin, likewise ch
        bool sx, sy;
        const int x0 = roi_mask_axis(dx, cw, M, &sx), y0 = roi_mask_axis(dy, ch, M, &sy);
        const int x1 = x0 + 1 < cw ? x0 + 1 : cw - 1, y1 = y0 + 1 < ch ? y0 + 1 : ch - 1;
        const uint8_t* m = masks + o0 + g * plane + (int64_t)ymin * w + xmin;
        bool one = m[(int64_t)y0 * w + x0] != 0;
        if (sx) one = one && m[(int64_t)y0 * w + x1] != 0;
        if (sy) one = one && m[(int64_t)y1 * w + x0] != 0;
        if (sx && sy) one = one && m[(int64_t)y1 * w + x1] != 0;
        v = one ? 1.f : 0.f;
      }
    }
    out[i] = v;
  }
}

extern "C" int scan_roi_mask_targets(const float* pos_rois, const int32_t* pos_gt, int32_t Rp, const uint8_t* masks, int64_t mask_bytes,
                                     const int64_t* moff, const int32_t* mhw, int32_t N, int32_t M, float* targets, void* stream) {
  SCAN_CHECK_ARG(Rp >= 0 && N >= 1 && M >= 1 && M <= 1024 && mask_bytes >= 0 && (int64_t)Rp * M * M < (1ll << 40),
                 "roi_mask_targets: Rp=%d, N=%d, M=%d, %lld mask bytes (Rp >= 0, N >= 1, 1 <= M <= 1024)", Rp, N, M,
                 (long long)mask_bytes);
  if (Rp == 0) return 0;
  SCAN_CHECK_ARG(pos_rois && pos_gt && moff && mhw && targets && (masks || mask_bytes == 0), "roi_mask_targets: null pointer");
  hipLaunchKernelGGL(roi_mask_targets_kernel, dim3(grid_for((int64_t)Rp * M * M, 256)), dim3(256), 0, as_stream(stream), pos_rois,
                     pos_gt, Rp, masks, mask_bytes, moff, mhw, N, M, targets);
  SCAN_LAUNCH_CHECK("roi_mask_targets");
  return 0;
}

// ------------------------------------------------------------------ loss
struct RoiMaskLossArgs {
  const float* logits;
  int64_t ld;
  int Rp, MM, C;
  const int32_t* labels;
  const float* targets;
};

// max(x, 0) - x t + log1p(exp(-|x|)); a row whose label is not a class takes no part
__device__ __forceinline__ float roi_mask_bce_elem(const RoiMaskLossArgs& p, int64_t e) {
  const int r = (int)(e / p.MM);
  const int lab = p.labels[r];
  if (lab < 0 || lab >= p.C) return 0.f;
  const float x = p.logits[e * p.ld + lab], t = p.targets[e];
  return fmaxf(x, 0.f) - x * t + log1pf(expf(-fabsf(x)));
}

// one block per 2048 elements, at most 256: a function of the element count alone, so the ordered sum is too
static inline int roi_mask_loss_grid(int64_t elems) {
  int64_t g = (elems + 2047) / 2048;
  return (int)(g < 1 ? 1 : (g > 256 ? 256 : g));
}

// ORD: every block writes its slot, ordered_sum_launch adds the slots.  !ORD: ONE workgroup of 1024 threads walks everything
// and stores the sum itself (no atomics, no cleared output, one launch).
template <bool ORD>
__global__ __launch_bounds__(ORD ? 256 : 1024) void roi_mask_loss_fwd_kernel(RoiMaskLossArgs p, float* __restrict__ out) {
  __shared__ float red[16];
  const int64_t work = (int64_t)p.Rp * p.MM;
  float s = 0.f;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < work; e += (int64_t)gridDim.x * blockDim.x)
    s += roi_mask_bce_elem(p, e);
  s = wave_sum(s);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) red[wid] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += red[w];
    out[ORD ? blockIdx.x : 0] = t;
  }
}

__global__ __launch_bounds__(256) void roi_mask_loss_bwd_kernel(RoiMaskLossArgs p, const float* __restrict__ g_dev,
                                                                float* __restrict__ d, int64_t ldo) {
  const float g = g_dev[0];
  const int64_t work = (int64_t)p.Rp * p.MM * ldo;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < work; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t e = i / ldo;
    const int j = (int)(i - e * ldo);
    const int lab = p.labels[(int)(e / p.MM)];
    float v = 0.f;
    if (j == lab && lab < p.C) {
      const float x = p.logits[e * p.ld + lab];
      const float z = expf(-fabsf(x));
      const float sg = x >= 0.f ? 1.f / (1.f + z) : z / (1.f + z);
      v = g * (sg - p.targets[e]);
    }
    d[i] = v;
  }
}

extern "C" int64_t scan_roi_mask_loss_ordered_ws_floats(int64_t elems) { return (int64_t)roi_mask_loss_grid(elems); }

static int roi_mask_loss_args(RoiMaskLossArgs* p, const float* logits, int64_t ld, int32_t Rp, int32_t M, int32_t C,
                              const int32_t* labels, const float* targets, const char* who) {
  SCAN_CHECK_ARG(Rp >= 0 && M >= 1 && M <= 1024 && C >= 1 && (int64_t)Rp * M * M < (1ll << 31),
                 "%s: Rp=%d, M=%d, C=%d (Rp >= 0, 1 <= M <= 1024, C >= 1, Rp M M < 2^31)", who, Rp, M, C);
  SCAN_CHECK_ARG(ld >= (int64_t)C, "%s: logits row pitch %lld for %d classes", who, (long long)ld, C);
  SCAN_CHECK_ARG(Rp == 0 || (logits && labels && targets), "%s: null input", who);
  p->logits = logits;
  p->ld = ld;
  p->Rp = Rp;
  p->MM = M * M;
  p->C = C;
  p->labels = labels;
  p->targets = targets;
  return 0;
}

extern "C" int scan_roi_mask_loss_forward(const float* logits, int64_t ld, int32_t Rp, int32_t M, int32_t C, const int32_t* labels,
                                          const float* targets, float* out1, void* stream) {
  RoiMaskLossArgs p;
  if (roi_mask_loss_args(&p, logits, ld, Rp, M, C, labels, targets, "roi_mask_loss_forward")) return -1;
  SCAN_CHECK_ARG(out1, "roi_mask_loss_forward: null output");
  hipLaunchKernelGGL(roi_mask_loss_fwd_kernel<false>, dim3(1), dim3(1024), 0, as_stream(stream), p, out1);  // Rp = 0 stores a zero
  SCAN_LAUNCH_CHECK("roi_mask_loss_fwd");
  return 0;
}

extern "C" int scan_roi_mask_loss_forward_ordered(const float* logits, int64_t ld, int32_t Rp, int32_t M, int32_t C,
                                                  const int32_t* labels, const float* targets, float* out1, float* ws, void* stream) {
  RoiMaskLossArgs p;
  if (roi_mask_loss_args(&p, logits, ld, Rp, M, C, labels, targets, "roi_mask_loss_forward_ordered")) return -1;
  SCAN_CHECK_ARG(out1 && ws, "roi_mask_loss_forward_ordered: null output");
  const int grid = roi_mask_loss_grid((int64_t)Rp * M * M);
  hipLaunchKernelGGL(roi_mask_loss_fwd_kernel<true>, dim3(grid), dim3(256), 0, as_stream(stream), p, ws);
  SCAN_LAUNCH_CHECK("roi_mask_loss_fwd_ordered");
  return ordered_sum_launch(ws, grid, 1, out1, 0, nullptr, stream, "roi_mask_loss_fwd_ordered_sum");
}

extern "C" int scan_roi_mask_loss_backward(const float* logits, int64_t ld, int32_t Rp, int32_t M, int32_t C, const int32_t* labels,
                                           const float* targets, const float* g_dev, float* d_logits, int64_t ldo, void* stream) {
  RoiMaskLossArgs p;
  if (roi_mask_loss_args(&p, logits, ld, Rp, M, C, labels, targets, "roi_mask_loss_backward")) return -1;
  if (Rp == 0) return 0;
  SCAN_CHECK_ARG(g_dev && d_logits && ldo >= (int64_t)C && ldo <= (1 << 20),
                 "roi_mask_loss_backward: null gradient pointer or a bad pitch %lld", (long long)ldo);
  hipLaunchKernelGGL(roi_mask_loss_bwd_kernel, dim3(grid_for((int64_t)Rp * M * M * ldo, 256)), dim3(256), 0, as_stream(stream), p, g_dev,
                     d_logits, ldo);
  SCAN_LAUNCH_CHECK("roi_mask_loss_bwd");
  return 0;
}

// ------------------------------------------------------------------ test-time probabilities
__global__ __launch_bounds__(256) void roi_mask_prob_kernel(const float* __restrict__ logits, int64_t ld, int K, int MM, int C,
                                                            const int32_t* __restrict__ labels, float* __restrict__ prob) {
  const int64_t work = (int64_t)K * MM;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < work; e += (int64_t)gridDim.x * blockDim.x) {
    const int lab = labels[(int)(e / MM)];
    float v = 0.f;
    if (lab >= 0 && lab < C) {
      const float x = logits[e * ld + lab];
      const float z = expf(-fabsf(x));
      v = x >= 0.f ? 1.f / (1.f + z) : z / (1.f + z);
    }
    prob[e] = v;
  }
}

extern "C" int scan_roi_mask_prob(const float* logits, int64_t ld, int32_t K, int32_t M, int32_t C, const int32_t* labels, float* prob,
                                  void* stream) {
  SCAN_CHECK_ARG(K >= 0 && M >= 1 && M <= 1024 && C >= 1 && (int64_t)K * M * M < (1ll << 31) && ld >= (int64_t)C,
                 "roi_mask_prob: K=%d, M=%d, C=%d, row pitch %lld", K, M, C, (long long)ld);
  if (K == 0) return 0;
  SCAN_CHECK_ARG(logits && labels && prob, "roi_mask_prob: null pointer");
  hipLaunchKernelGGL(roi_mask_prob_kernel, dim3(grid_for((int64_t)K * M * M, 256)), dim3(256), 0, as_stream(stream), logits, ld, K,
                     M * M, C, labels, prob);
  SCAN_LAUNCH_CHECK("roi_mask_prob");
  return 0;
}

// ------------------------------------------------------------------ paste
// torch's source index of bilinear align_corners=False for output index d at scale in / out, clamped at 0
__device__ __forceinline__ void roi_mask_src(int d, float scale, int in, int* i0, int* i1, float* l0, float* l1) {
  float s = scale * ((float)d + 0.5f) - 0.5f;
  s = s < 0.f ? 0.f : s;
  int a = (int)s;
  a = a < in - 1 ? a : in - 1;
  *i0 = a;
  *i1 = a + (a < in - 1 ? 1 : 0);
  *l1 = s - (float)a;
  *l0 = 1.f - *l1;
}

// the mask zero-padded by 1 on every side, read through the index arithmetic
__device__ __forceinline__ float roi_mask_padded(const float* __restrict__ m, int M, int py, int px) {
  return (py >= 1 && py <= M && px >= 1 && px <= M) ? m[(py - 1) * M + (px - 1)] : 0.f;
}

// One thread per group of four consecutive pixels of one output row (k, y): the box of detection k is expanded once per thread
// and row, a pixel outside it costs two comparisons, and where W is a multiple of 4 the group is one 32-bit store.  Rows are
// grid-strided over blockIdx.y, groups over blockIdx.x.
__global__ __launch_bounds__(256) void roi_mask_paste_kernel(const float* __restrict__ prob, const float* __restrict__ boxes, int K,
                                                             int M, int H, int W, float scale, float thresh,
                                                             uint8_t* __restrict__ out) {
  const int64_t rows = (int64_t)K * H;
  const int groups = (W + 3) >> 2, Mp = M + 2;
  const bool vec = (W & 3) == 0;
  for (int64_t r = blockIdx.y; r < rows; r += gridDim.y) {
    const int k = (int)(r / H), y = (int)(r - (int64_t)k * H);
    const float* b = boxes + (int64_t)k * 4;
    // expand_boxes (inference.py:91-105) in fp32, then .to(torch.int32): truncation toward zero
    const float wh = (b[2] - b[0]) * 0.5f * scale, hh = (b[3] - b[1]) * 0.5f * scale;
    const float xc = (b[2] + b[0]) * 0.5f, yc = (b[3] + b[1]) * 0.5f;
    const int bx0 = roi_mask_trunc(xc - wh), bx1 = roi_mask_trunc(xc + wh);
    const int by0 = roi_mask_trunc(yc - hh), by1 = roi_mask_trunc(yc + hh);
    // the pasted window im_mask[y_0:y_1, x_0:x_1] (inference.py:137-145): rows by0..by1, columns bx0..bx1 of the image
    const bool row_in = y >= by0 && y <= by1 && bx1 >= bx0;
    const int64_t bw = (int64_t)bx1 - bx0 + 1, bh = (int64_t)by1 - by0 + 1;  // >= 1 where row_in
    int y0 = 0, y1 = 0;
    float wy0 = 0.f, wy1 = 0.f;
    if (row_in) roi_mask_src(y - by0, (float)Mp / (float)bh, Mp, &y0, &y1, &wy0, &wy1);
    const float xscale = row_in ? (float)Mp / (float)bw : 0.f;
    const float* m = prob + (int64_t)k * M * M;
    uint8_t* orow = out + r * W;
    for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += gridDim.x * blockDim.x) {
      uint32_t v = 0u;
      const int xg = g << 2;
      if (row_in && xg <= bx1 && xg + 3 >= bx0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int x = xg + j;
          if (x < bx0 || x > bx1 || x >= W) continue;
          int x0, x1;
          float wx0, wx1;
          roi_mask_src(x - bx0, xscale, Mp, &x0, &x1, &wx0, &wx1);
          const float top = wx0 * roi_mask_padded(m, M, y0, x0) + wx1 * roi_mask_padded(m, M, y0, x1);
          const float bot = wx0 * roi_mask_padded(m, M, y1, x0) + wx1 * roi_mask_padded(m, M, y1, x1);
          if ((wy0 * top + wy1 * bot) > thresh) v |= 1u << (8 * j);
        }
      }
      if (vec) {
        reinterpret_cast<uint32_t*>(orow)[g] = v;
      } else {
        for (int j = 0; j < 4 && xg + j < W; ++j) orow[xg + j] = (uint8_t)((v >> (8 * j)) & 1u);
      }
    }
  }
}

extern "C" int scan_roi_mask_paste(const float* prob, const float* boxes, int32_t K, int32_t M, int32_t H, int32_t W, float thresh,
                                   uint8_t* out, void* stream) {
  SCAN_CHECK_ARG(K >= 0 && M >= 1 && M <= 1024 && H >= 1 && W >= 1 && (int64_t)K * H * W < (1ll << 40),
                 "roi_mask_paste: K=%d, M=%d, H=%d, W=%d", K, M, H, W);
  SCAN_CHECK_ARG(thresh >= 0.f, "roi_mask_paste: thresh %g below 0 (the reference's mask * 255 debugging mode) is not built",
                 (double)thresh);
  if (K == 0) return 0;
  SCAN_CHECK_ARG(prob && boxes && out && (reinterpret_cast<uintptr_t>(out) & 3) == 0, "roi_mask_paste: null pointer, or out not 4-byte aligned");
  const float scale = (float)((double)(M + 2) / (double)M);
  const int64_t rows = (int64_t)K * H;
  const dim3 grid((unsigned)grid_for((W + 3) / 4, 256), (unsigned)(rows < 32768 ? rows : 32768));
  hipLaunchKernelGGL(roi_mask_paste_kernel, grid, dim3(256), 0, as_stream(stream), prob, boxes, K, M, H, W, scale, thresh, out);
  SCAN_LAUNCH_CHECK("roi_mask_paste");
  return 0;
}
