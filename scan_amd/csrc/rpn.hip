// The region-proposal network's device side (reference modeling/rpn/{loss.py, inference.py, anchor_generator.py},
// modeling/balanced_positive_negative_sampler.py, modeling/box_coder.py): the visibility rule on top of scan_retina_match's
// labels, the balanced fg / bg sampler, the objectness BCE + smooth-L1 loss over the sampled anchors, and the proposal decode.
//
// Anchors are those of retina.hip: anchor i = m * A + a of pyramid row m = (level, image, y, x) is cells[level][a] + the
// location's shift, formed in the kernel (anchors.h); no anchor tensor is read.  Built with -ffp-contract=off: every fp32
// operation is rounded on its own.
//
// Labels: scan_retina_match with every box label 1 leaves 1 (matched), 0 (below the low threshold) or -1 (between); the
// visibility launch below then writes -1 wherever the anchor leaves its image's unpadded (h, w) by more than the straddle
// threshold, which is the reference's order of overwrites (rpn/loss.py:66-79: visible-or-not is decided before the
// between-thresholds discard, and both write -1).
//
// Sampler: one workgroup of RPN_SAMPLE_BLOCK threads per (image, class of label); see the header for the rule and the key.
// A radix select over the 32 key bits, 8 bits a pass with a 256-bin LDS histogram, finds the k-th smallest key T; where
// several anchors carry T a second select over the anchors' ordinals within the image finds the last one taken.  Integers only.
//
// Loss and backward run over ALL anchors with no compaction, as the smooth-L1 kernels of retina.hip do.
#include "common.h"
#include "boxes.h"
#include "anchors.h"

#define RPN_SAMPLE_BLOCK 256
#define RPN_BBOX_XFORM_CLIP 4.135166556742356f  // log(1000 / 16), box_coder.py:13

// ------------------------------------------------------------------ visibility
__global__ __launch_bounds__(256) void rpn_visibility_kernel(scan_pyramid_t d, RetinaStrides st, const float* __restrict__ cells,
                                                             int A, const int32_t* __restrict__ image_hw, float thr,
                                                             int32_t* __restrict__ labels, int32_t* __restrict__ matched) {
  const int64_t total = d.row_off[d.n_levels] * A;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t m = i / A;
    const RowCoord rc = decode_row(d, m);
    const float4 an = retina_anchor(st, cells, A, rc, (int)(i - m * A));
    const float h = (float)image_hw[2 * rc.n] + thr, w = (float)image_hw[2 * rc.n + 1] + thr;
    const bool inside = an.x >= -thr && an.y >= -thr && an.z < w && an.w < h;
    if (!inside) {
      labels[i] = -1;
      matched[i] = 0;
    }
  }
}

extern "C" int scan_rpn_visibility(const scan_pyramid_t* d, const int32_t* strides, const float* cells, int32_t A,
                                   const int32_t* image_hw, float straddle_thresh, int32_t* labels_i32, int32_t* matched,
                                   void* stream) {
  RetinaStrides st;
  if (retina_check(d, strides, cells, A, &st, "rpn_visibility")) return -1;
  SCAN_CHECK_ARG(image_hw && labels_i32 && matched, "rpn_visibility: null pointer");
  if (straddle_thresh < 0.f) return 0;  // every anchor is visible
  hipLaunchKernelGGL(rpn_visibility_kernel, dim3(grid_for(d->row_off[d->n_levels] * A, 256)), dim3(256), 0, as_stream(stream), *d,
                     st, cells, A, image_hw, straddle_thresh, labels_i32, matched);
  SCAN_LAUNCH_CHECK("rpn_visibility");
  return 0;
}

// ------------------------------------------------------------------ sampler
__device__ __forceinline__ uint32_t rpn_fmix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x85EBCA6Bu;
  x ^= x >> 13;
  x *= 0xC2B2AE35u;
  x ^= x >> 16;
  return x;
}
__device__ __forceinline__ uint32_t rpn_key(uint32_t seed, int n, int64_t i, const uint32_t* __restrict__ keys) {
  if (keys != nullptr) return keys[i];
  return rpn_fmix32(rpn_fmix32(seed ^ (0x9E3779B9u * (uint32_t)(n + 1))) ^ (uint32_t)i);
}

// f(i, j) for every anchor of image n: i its index, j its ordinal within the image (both grow together); the image's rows are
// one range per level
template <typename F>
__device__ __forceinline__ void rpn_walk_image(const scan_pyramid_t& d, int A, int n, F f) {
  uint32_t j0 = 0;
#pragma unroll
  for (int l = 0; l < SCAN_MAX_LEVELS; ++l) {
    if (l < d.n_levels) {
      const int64_t hw = (int64_t)d.h[l] * d.w[l];
      const uint32_t cnt = (uint32_t)(hw * A);
      const int64_t base = (d.row_off[l] + (int64_t)n * hw) * A;
      for (uint32_t t = threadIdx.x; t < cnt; t += RPN_SAMPLE_BLOCK) f(base + t, j0 + t);
      j0 += cnt;
    }
  }
}

struct RpnSelectState {
  unsigned hist[256];
  unsigned prefix, remaining, count_at;
};

// the `want`-th smallest (1-based) of the values value(i, j) over the anchors with member(i, j): 4 passes of 8 bits.  Returns
// the value in every thread; s.count_at = how many members carry it, s.remaining = how many of those are among the `want`
template <typename M, typename V>
__device__ __forceinline__ uint32_t rpn_radix_select(const scan_pyramid_t& d, int A, int n, RpnSelectState& s, unsigned want, M member,
                                                     V value) {
  if (threadIdx.x == 0) {
    s.prefix = 0u;
    s.remaining = want;
  }
  uint32_t mask = 0u;
  for (int shift = 24; shift >= 0; shift -= 8) {
    s.hist[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t prefix = s.prefix;
    rpn_walk_image(d, A, n, [&](int64_t i, uint32_t j) {
      if (member(i, j)) {
        const uint32_t v = value(i, j);
        if ((v & mask) == prefix) atomicAdd(&s.hist[(v >> shift) & 255u], 1u);
      }
    });
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned cum = 0u, b = 0u;
      for (; b < 255u; ++b) {
        if (cum + s.hist[b] >= s.remaining) break;
        cum += s.hist[b];
      }
      s.remaining -= cum;
      s.count_at = s.hist[b];
      s.prefix = prefix | (b << shift);
    }
    mask |= 255u << shift;
    __syncthreads();
  }
  return s.prefix;
}

__global__ __launch_bounds__(RPN_SAMPLE_BLOCK) void rpn_sample_kernel(scan_pyramid_t d, int A, const int32_t* __restrict__ labels,
                                                                      int batch, int max_pos, uint32_t seed,
                                                                      const uint32_t* __restrict__ keys,
                                                                      uint8_t* __restrict__ sampled, int32_t* __restrict__ counts) {
  __shared__ RpnSelectState s;
  __shared__ unsigned cnt[2];
  const int n = blockIdx.x >> 1;
  const bool neg = blockIdx.x & 1;
  if (threadIdx.x < 2) cnt[threadIdx.x] = 0u;
  __syncthreads();
  unsigned np = 0u, nn = 0u;
  rpn_walk_image(d, A, n, [&](int64_t i, uint32_t) {
    const int lab = labels[i];
    np += lab >= 1 ? 1u : 0u;
    nn += lab == 0 ? 1u : 0u;
  });
  np = (unsigned)wave_sum((int)np);
  nn = (unsigned)wave_sum((int)nn);
  if ((threadIdx.x & 63) == 0) {
    if (np) atomicAdd(&cnt[0], np);
    if (nn) atomicAdd(&cnt[1], nn);
  }
  __syncthreads();
  const unsigned num_pos = cnt[0] < (unsigned)max_pos ? cnt[0] : (unsigned)max_pos;
  const unsigned room = (unsigned)batch - num_pos;
  const unsigned num_neg = cnt[1] < room ? cnt[1] : room;
  const unsigned have = neg ? cnt[1] : cnt[0], k = neg ? num_neg : num_pos;
  if (threadIdx.x == 0) counts[2 * n + (neg ? 1 : 0)] = (int32_t)k;
  auto member = [&](int64_t i, uint32_t) {
    const int lab = labels[i];
    return neg ? lab == 0 : lab >= 1;
  };
  // T: the largest key taken; J: the largest ordinal taken among the anchors whose key is T
  uint32_t T = 0xffffffffu, J = 0xffffffffu;
  if (k > 0u && k < have) {
    T = rpn_radix_select(d, A, n, s, k, member, [&](int64_t i, uint32_t) { return rpn_key(seed, n, i, keys); });
    const unsigned r = s.remaining, at = s.count_at;
    __syncthreads();
    if (r < at)
      J = rpn_radix_select(d, A, n, s, r, [&](int64_t i, uint32_t j) { return member(i, j) && rpn_key(seed, n, i, keys) == T; },
                           [&](int64_t, uint32_t j) { return j; });
  }
  const uint8_t mark = neg ? 2 : 1;
  rpn_walk_image(d, A, n, [&](int64_t i, uint32_t j) {
    const int lab = labels[i];
    if (neg ? lab == 0 : lab != 0) {  // the positives' workgroup also clears the anchors no class owns (label < 0)
      bool take = false;
      if (k > 0u && (neg || lab >= 1)) {
        const uint32_t key = rpn_key(seed, n, i, keys);
        take = key < T || (key == T && j <= J);
      }
      sampled[i] = take ? mark : (uint8_t)0;
    }
  });
}

extern "C" int scan_rpn_sample(const scan_pyramid_t* d, int32_t A, const int32_t* labels_i32, int32_t batch_size_per_image,
                               int32_t max_positives, uint32_t seed, const uint32_t* keys, uint8_t* sampled, int32_t* counts,
                               void* stream) {
  if (scan_check_pyramid(d, "rpn_sample")) return -1;
  SCAN_CHECK_ARG(A >= 1 && A <= RETINA_MAX_A, "rpn_sample: A=%d anchors per location outside 1..%d", A, RETINA_MAX_A);
  SCAN_CHECK_ARG(d->row_off[d->n_levels] * A < (1ll << 31), "rpn_sample: 2^31 anchors or more");
  SCAN_CHECK_ARG(labels_i32 && sampled && counts, "rpn_sample: null pointer");
  SCAN_CHECK_ARG(batch_size_per_image >= 1 && max_positives >= 0 && max_positives <= batch_size_per_image,
                 "rpn_sample: batch_size_per_image=%d, max_positives=%d (0 <= max_positives <= batch_size_per_image, >= 1)",
                 batch_size_per_image, max_positives);
  SCAN_CHECK_ARG(d->n_images < (1 << 30), "rpn_sample: too many images");
  hipLaunchKernelGGL(rpn_sample_kernel, dim3(2 * d->n_images), dim3(RPN_SAMPLE_BLOCK), 0, as_stream(stream), *d, A, labels_i32,
                     batch_size_per_image, max_positives, seed, keys, sampled, counts);
  SCAN_LAUNCH_CHECK("rpn_sample");
  return 0;
}

// ------------------------------------------------------------------ loss
struct RpnLossArgs {
  scan_pyramid_t d;
  RetinaStrides st;
  const float* cells;
  int A;
  const float* boxes;
  int G;
  const int32_t* matched;
  const uint8_t* sampled;
  const float* obj;
  int64_t ld_obj;
  const float* reg;
  int64_t ld_reg;
  float beta;
};

// the target of anchor i = m * A + a (a sampled positive) and its prediction
__device__ __forceinline__ void rpn_reg_pair(const RpnLossArgs& p, int64_t i, int64_t m, int a, float4* t, float4* x) {
  const RowCoord rc = decode_row(p.d, m);
  const float4 an = retina_anchor(p.st, p.cells, p.A, rc, a);
  int g = p.matched[i];
  g = g < 0 ? 0 : (g < p.G ? g : p.G - 1);  // never read out of bounds, whatever the plan holds
  const float4 b = *reinterpret_cast<const float4*>(p.boxes + ((int64_t)rc.n * p.G + g) * 4);
  *t = box_encode(b, an, 1.0, 1.0);  // weights (1, 1, 1, 1)
  *x = *reinterpret_cast<const float4*>(p.reg + m * p.ld_reg + 4 * a);
}

template <bool ORD>
__global__ __launch_bounds__(256) void rpn_loss_fwd_kernel(RpnLossArgs p, float* __restrict__ targets_out, float* __restrict__ out) {
  __shared__ float red[4];
  const int64_t total = p.d.row_off[p.d.n_levels] * p.A;
  float bce = 0.f, reg = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int s = p.sampled[i];
    const int64_t m = i / p.A;
    const int a = (int)(i - m * p.A);
    float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
    if (s != 0) {
      const float x = p.obj[m * p.ld_obj + a];
      const float y = s == 1 ? 1.f : 0.f;
      bce += fmaxf(x, 0.f) - x * y + log1pf(expf(-fabsf(x)));
    }
    if (s == 1) {
      float4 x;
      rpn_reg_pair(p, i, m, a, &t, &x);
      reg += (smooth_l1_elem(x.x, t.x, p.beta) + smooth_l1_elem(x.y, t.y, p.beta)) +
             (smooth_l1_elem(x.z, t.z, p.beta) + smooth_l1_elem(x.w, t.w, p.beta));
    }
    if (targets_out != nullptr) reinterpret_cast<float4*>(targets_out)[i] = t;
  }
  const float s0 = block_sum_256(bce, red);
  const float s1 = block_sum_256(reg, red);
  if (threadIdx.x == 0) {
    block_result<ORD>(out, 0, 2, s0);
    block_result<ORD>(out, 1, 2, s1);
  }
}

__global__ __launch_bounds__(256) void rpn_loss_bwd_kernel(RpnLossArgs p, const float* __restrict__ g_dev, float* __restrict__ d_obj,
                                                           int64_t ldo_obj, float* __restrict__ d_reg, int64_t ldo_reg) {
  const int64_t total = p.d.row_off[p.d.n_levels] * p.A;
  const float g0 = g_dev[0], g1 = g_dev[1];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int s = p.sampled[i];
    const int64_t m = i / p.A;
    const int a = (int)(i - m * p.A);
    float dx = 0.f;
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if (s != 0) {
      const float x = p.obj[m * p.ld_obj + a];
      const float e = expf(-fabsf(x));
      const float sig = x >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
      dx = g0 * (sig - (s == 1 ? 1.f : 0.f));
    }
    if (s == 1) {
      float4 t, x;
      rpn_reg_pair(p, i, m, a, &t, &x);
      o = make_float4(g1 * smooth_l1_grad(x.x, t.x, p.beta), g1 * smooth_l1_grad(x.y, t.y, p.beta),
                      g1 * smooth_l1_grad(x.z, t.z, p.beta), g1 * smooth_l1_grad(x.w, t.w, p.beta));
    }
    d_obj[m * ldo_obj + a] = dx;
    *reinterpret_cast<float4*>(d_reg + m * ldo_reg + 4 * a) = o;
  }
}

extern "C" int64_t scan_rpn_loss_ordered_ws_floats(int64_t n_anchors) { return 2 * (int64_t)head_loss_grid(n_anchors); }

static int rpn_loss_args(RpnLossArgs* p, const scan_pyramid_t* d, const int32_t* strides, const float* cells, int32_t A,
                         const float* boxes, int32_t G, const int32_t* matched, const uint8_t* sampled, const float* obj,
                         int64_t ld_obj, const float* reg, int64_t ld_reg, float beta, const char* who) {
  if (retina_check(d, strides, cells, A, &p->st, who)) return -1;
  SCAN_CHECK_ARG(boxes && matched && sampled && obj && reg, "%s: null input", who);
  SCAN_CHECK_ARG(G >= 1, "%s: G=%d < 1", who, G);
  SCAN_CHECK_ARG(ld_obj >= (int64_t)A, "%s: objectness row pitch %lld for %d anchors", who, (long long)ld_obj, A);
  SCAN_CHECK_ARG(ld_reg >= 4 * (int64_t)A && (ld_reg & 3) == 0, "%s: bbox_reg row pitch %lld for %d anchors (a multiple of 4, >= 4 A)",
                 who, (long long)ld_reg, A);
  SCAN_CHECK_ARG(((reinterpret_cast<uintptr_t>(boxes) | reinterpret_cast<uintptr_t>(reg)) & 15) == 0 &&
                     (reinterpret_cast<uintptr_t>(obj) & 3) == 0,
                 "%s: boxes / bbox_reg must be 16-byte, objectness 4-byte aligned", who);
  SCAN_CHECK_ARG(beta > 0.f, "%s: beta=%g must be positive", who, (double)beta);
  p->d = *d;
  p->cells = cells;
  p->A = A;
  p->boxes = boxes;
  p->G = G;
  p->matched = matched;
  p->sampled = sampled;
  p->obj = obj;
  p->ld_obj = ld_obj;
  p->reg = reg;
  p->ld_reg = ld_reg;
  p->beta = beta;
  return 0;
}

template <bool ORD>
static int rpn_loss_forward_launch(const scan_pyramid_t* d, const int32_t* strides, const float* cells, int32_t A, const float* boxes,
                                   int32_t G, const int32_t* matched, const uint8_t* sampled, const float* obj, int64_t ld_obj,
                                   const float* reg, int64_t ld_reg, float beta, float* targets_out, float* out2, float* ws,
                                   void* stream, const char* who) {
  RpnLossArgs p;
  if (rpn_loss_args(&p, d, strides, cells, A, boxes, G, matched, sampled, obj, ld_obj, reg, ld_reg, beta, who)) return -1;
  SCAN_CHECK_ARG(out2 && (!ORD || ws), "%s: null output", who);
  SCAN_CHECK_ARG((reinterpret_cast<uintptr_t>(targets_out) & 15) == 0, "%s: targets_out must be 16-byte aligned", who);
  const int grid = head_loss_grid(d->row_off[d->n_levels] * A);
  hipLaunchKernelGGL(rpn_loss_fwd_kernel<ORD>, dim3(grid), dim3(256), 0, as_stream(stream), p, targets_out, ORD ? ws : out2);
  SCAN_LAUNCH_CHECK(ORD ? "rpn_loss_fwd_ordered" : "rpn_loss_fwd");
  return ORD ? ordered_sum_launch(ws, grid, 2, out2, 0, nullptr, stream, "rpn_loss_fwd_ordered_sum") : 0;
}

extern "C" int scan_rpn_loss_forward(const scan_pyramid_t* d, const int32_t* strides, const float* cells, int32_t A,
                                     const float* boxes, int32_t G, const int32_t* matched, const uint8_t* sampled,
                                     const float* objectness, int64_t ld_obj, const float* bbox_reg, int64_t ld_reg, float beta,
                                     float* targets_out, float* out2, void* stream) {
  return rpn_loss_forward_launch<false>(d, strides, cells, A, boxes, G, matched, sampled, objectness, ld_obj, bbox_reg, ld_reg, beta,
                                        targets_out, out2, nullptr, stream, "rpn_loss_forward");
}

extern "C" int scan_rpn_loss_forward_ordered(const scan_pyramid_t* d, const int32_t* strides, const float* cells, int32_t A,
                                             const float* boxes, int32_t G, const int32_t* matched, const uint8_t* sampled,
                                             const float* objectness, int64_t ld_obj, const float* bbox_reg, int64_t ld_reg,
                                             float beta, float* targets_out, float* out2, float* ws, void* stream) {
  return rpn_loss_forward_launch<true>(d, strides, cells, A, boxes, G, matched, sampled, objectness, ld_obj, bbox_reg, ld_reg, beta,
                                       targets_out, out2, ws, stream, "rpn_loss_forward_ordered");
}

extern "C" int scan_rpn_loss_backward(const scan_pyramid_t* d, const int32_t* strides, const float* cells, int32_t A,
                                      const float* boxes, int32_t G, const int32_t* matched, const uint8_t* sampled,
                                      const float* objectness, int64_t ld_obj, const float* bbox_reg, int64_t ld_reg, float beta,
                                      const float* g2_dev, float* d_obj, int64_t ldo_obj, float* d_reg, int64_t ldo_reg,
                                      void* stream) {
  RpnLossArgs p;
  if (rpn_loss_args(&p, d, strides, cells, A, boxes, G, matched, sampled, objectness, ld_obj, bbox_reg, ld_reg, beta,
                    "rpn_loss_backward"))
    return -1;
  SCAN_CHECK_ARG(g2_dev && d_obj && d_reg && (reinterpret_cast<uintptr_t>(d_reg) & 15) == 0 && ldo_obj >= (int64_t)A &&
                     ldo_reg >= 4 * (int64_t)A && (ldo_reg & 3) == 0,
                 "rpn_loss_backward: null or misaligned gradient pointer, or a bad pitch");
  hipLaunchKernelGGL(rpn_loss_bwd_kernel, dim3(grid_for(d->row_off[d->n_levels] * A, 256)), dim3(256), 0, as_stream(stream), p,
                     g2_dev, d_obj, ldo_obj, d_reg, ldo_reg);
  SCAN_LAUNCH_CHECK("rpn_loss_bwd");
  return 0;
}

// ------------------------------------------------------------------ proposal decode
struct RpnCandOffsets {
  int off[SCAN_MAX_LEVELS + 1];
};

__global__ __launch_bounds__(256) void rpn_decode_kernel(scan_pyramid_t d, RetinaStrides st, const float* __restrict__ cells, int A,
                                                         const float* __restrict__ reg, int64_t ld, const int64_t* __restrict__ idx,
                                                         RpnCandOffsets ko, const int32_t* __restrict__ image_hw, float min_size,
                                                         float* __restrict__ boxes, uint8_t* __restrict__ keep) {
  const int K = ko.off[d.n_levels];
  const int64_t total = (int64_t)d.n_images * K;
  for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < total; c += (int64_t)gridDim.x * blockDim.x) {
    const int n = (int)(c / K);
    const int k = (int)(c - (int64_t)n * K);
    const int l = level_of(ko.off, d.n_levels, k);
    const int h = pick_level(d.h, l), w = pick_level(d.w, l);
    const int64_t j = idx[c];
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    bool ok = false;
    if (j >= 0 && j < (int64_t)h * w * A) {  // an index outside the level is no candidate: nothing is read for it
      const int r = (int)(j / A), a = (int)(j - (int64_t)r * A);
      RowCoord rc;
      rc.lvl = l;
      rc.n = n;
      rc.y = r / w;
      rc.x = r - rc.y * w;
      const float4 an = retina_anchor(st, cells, A, rc, a);
      const int64_t m = pick_level(d.row_off, l) + (int64_t)n * h * w + r;
      const float4 t = *reinterpret_cast<const float4*>(reg + m * ld + 4 * a);
      const float aw = an.z - an.x + 1.f, ah = an.w - an.y + 1.f;
      const float cx = an.x + 0.5f * aw, cy = an.y + 0.5f * ah;
      const float dw = fminf(t.z, RPN_BBOX_XFORM_CLIP), dh = fminf(t.w, RPN_BBOX_XFORM_CLIP);
      const float pcx = t.x * aw + cx, pcy = t.y * ah + cy;
      const float pw = expf(dw) * aw, ph = expf(dh) * ah;
      const float xmax = (float)(image_hw[2 * n + 1] - 1), ymax = (float)(image_hw[2 * n] - 1);
      o.x = fminf(fmaxf(pcx - 0.5f * pw, 0.f), xmax);
      o.y = fminf(fmaxf(pcy - 0.5f * ph, 0.f), ymax);
      o.z = fminf(fmaxf(pcx + 0.5f * pw - 1.f, 0.f), xmax);
      o.w = fminf(fmaxf(pcy + 0.5f * ph - 1.f, 0.f), ymax);
      ok = (o.z - o.x + 1.f >= min_size) && (o.w - o.y + 1.f >= min_size);
    }
    reinterpret_cast<float4*>(boxes)[c] = o;
    keep[c] = ok ? 1 : 0;
  }
}

extern "C" int scan_rpn_decode(const scan_pyramid_t* d, const int32_t* strides, const float* cells, int32_t A, const float* bbox_reg,
                               int64_t ld, const int64_t* topk_idx, const int32_t* k_off, const int32_t* image_hw, float min_size,
                               float* boxes, uint8_t* keep, void* stream) {
  RetinaStrides st;
  if (retina_check(d, strides, cells, A, &st, "rpn_decode")) return -1;
  SCAN_CHECK_ARG(bbox_reg && topk_idx && k_off && image_hw && boxes && keep, "rpn_decode: null pointer");
  SCAN_CHECK_ARG(ld >= 4 * (int64_t)A && (ld & 3) == 0, "rpn_decode: row pitch %lld for %d anchors (a multiple of 4, >= 4 A)",
                 (long long)ld, A);
  SCAN_CHECK_ARG(((reinterpret_cast<uintptr_t>(bbox_reg) | reinterpret_cast<uintptr_t>(boxes)) & 15) == 0,
                 "rpn_decode: bbox_reg / boxes must be 16-byte aligned");
  RpnCandOffsets ko;
  for (int l = 0; l <= SCAN_MAX_LEVELS; ++l) ko.off[l] = 0;
  SCAN_CHECK_ARG(k_off[0] == 0, "rpn_decode: k_off[0]=%d must be 0", k_off[0]);
  for (int l = 0; l < d->n_levels; ++l) {
    SCAN_CHECK_ARG(k_off[l + 1] >= k_off[l] && (int64_t)(k_off[l + 1] - k_off[l]) <= (int64_t)d->h[l] * d->w[l] * A,
                   "rpn_decode: level %d has %d candidates for %lld anchors", l, k_off[l + 1] - k_off[l],
                   (long long)d->h[l] * d->w[l] * A);
    ko.off[l + 1] = k_off[l + 1];
  }
  for (int l = d->n_levels + 1; l <= SCAN_MAX_LEVELS; ++l) ko.off[l] = ko.off[d->n_levels];
  const int64_t total = (int64_t)d->n_images * ko.off[d->n_levels];
  if (total == 0) return 0;
  hipLaunchKernelGGL(rpn_decode_kernel, dim3(grid_for(total, 256)), dim3(256), 0, as_stream(stream), *d, st, cells, A, bbox_reg, ld,
                     topk_idx, ko, image_hw, min_size, boxes, keep);
  SCAN_LAUNCH_CHECK("rpn_decode");
  return 0;
}
