// HBM-bound pointwise kernels of the SCAN hot path for gfx950 outside the loss family (losses.hip): GRL scale, fused SGD, 2x2 and
// 3x3/stride-2 max pooling, the residual add + ReLU, the FPN top-down join and its backward, the gradient of take_images, the
// column block copy and the paradigm update.  float4 streaming where the layout allows, grid capped at 2048 blocks with
// grid-stride loops.
#include <float.h>

#include "common.h"
#include <algorithm>

// The float4 kernels below need 16-byte aligned pointers.  The flat ones (scale, add_relu) are handed row ranges of matrices
// with any column count and pick a scalar kernel when a pointer is not; the NHWC ones take fresh allocations with C % 4 == 0
// and reject anything else.
static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ------------------------------------------------------------------ y = alpha * x (GRL)
__global__ __launch_bounds__(256) void scale_kernel(const float* __restrict__ x, float alpha, float* __restrict__ y,
                                                    int64_t n) {
  const int64_t n4 = n >> 2;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    float4 v = reinterpret_cast<const float4*>(x)[i];
    v.x *= alpha; v.y *= alpha; v.z *= alpha; v.w *= alpha;
    reinterpret_cast<float4*>(y)[i] = v;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) y[(n4 << 2) + threadIdx.x] = alpha * x[(n4 << 2) + threadIdx.x];
}

// the same multiply, one float per lane: for pointers that are not 16-byte aligned (a level's rows of an [M, 9] matrix)
__global__ __launch_bounds__(256) void scale_scalar_kernel(const float* __restrict__ x, float alpha, float* __restrict__ y,
                                                           int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    y[i] = alpha * x[i];
}

extern "C" int scan_scale(const float* x, float alpha, float* y, int64_t n, void* stream) {
  SCAN_CHECK_ARG(n >= 0, "scale: bad n");
  if (n == 0) return 0;
  SCAN_CHECK_ARG(x && y, "scale: null pointer");
  if (aligned16(x) && aligned16(y))
    hipLaunchKernelGGL(scale_kernel, dim3(grid_for(n / 4 + 1, 256)), dim3(256), 0, as_stream(stream), x, alpha, y, n);
  else
    hipLaunchKernelGGL(scale_scalar_kernel, dim3(grid_for(n, 256)), dim3(256), 0, as_stream(stream), x, alpha, y, n);
  SCAN_LAUNCH_CHECK("scale");
  return 0;
}

// ------------------------------------------------------------------ fused SGD + momentum + weight decay
__global__ __launch_bounds__(256) void sgd_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                  float* __restrict__ buf, int64_t n, float lr, float wd,
                                                  float momentum, int first) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float w = p[i];
    const float gg = g[i] + wd * w;
    const float b = first ? gg : momentum * buf[i] + gg;
    buf[i] = b;
    p[i] = w - lr * b;
  }
}

extern "C" int scan_sgd_momentum(float* p, const float* g, float* buf, int64_t n, float lr, float wd, float momentum,
                                 int32_t first_step, void* stream) {
  SCAN_CHECK_ARG(n >= 0, "sgd_momentum: bad n");
  if (n == 0) return 0;
  SCAN_CHECK_ARG(p && g && buf, "sgd_momentum: null pointer");
  hipLaunchKernelGGL(sgd_kernel, dim3(grid_for(n, 256)), dim3(256), 0, as_stream(stream), p, g, buf, n, lr, wd,
                     momentum, first_step);
  SCAN_LAUNCH_CHECK("sgd");
  return 0;
}

// ------------------------------------------------------------------ 2x2 / stride-2 max pooling on NHWC rows
// (replaces nn.MaxPool2d(2, 2) of the VGG body, reference backbone/mmdetection/vgg.py:33).  HBM-bound:
// forward reads 4 and writes 1 float4 per lane; backward re-derives the argmax (first maximum in window
// order, like F.max_pool2d) from x and y instead of storing indices.
__global__ __launch_bounds__(256) void maxpool2_fwd_kernel(const float* __restrict__ x, int N, int H, int W, int C,
                                                           float* __restrict__ y) {
  const int Ho = H >> 1, Wo = W >> 1, C4 = C >> 2;
  const int64_t total = (int64_t)N * Ho * Wo * C4;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int c4 = (int)(i % C4);
    int64_t p = i / C4;
    const int xo = (int)(p % Wo);
    p /= Wo;
    const int yo = (int)(p % Ho);
    const int n = (int)(p / Ho);
    const float4* b = reinterpret_cast<const float4*>(x + (((int64_t)n * H + 2 * yo) * W + 2 * xo) * C) + c4;
    const float4 a0 = b[0], a1 = b[C4], a2 = b[(int64_t)W * C4], a3 = b[(int64_t)W * C4 + C4];
    float4 m;
    m.x = fmaxf(fmaxf(a0.x, a1.x), fmaxf(a2.x, a3.x));
    m.y = fmaxf(fmaxf(a0.y, a1.y), fmaxf(a2.y, a3.y));
    m.z = fmaxf(fmaxf(a0.z, a1.z), fmaxf(a2.z, a3.z));
    m.w = fmaxf(fmaxf(a0.w, a1.w), fmaxf(a2.w, a3.w));
    reinterpret_cast<float4*>(y)[i] = m;
  }
}

__device__ __forceinline__ void pool_bwd1(float a0, float a1, float a2, float a3, float m, float g, float& d0,
                                          float& d1, float& d2, float& d3) {
  d0 = d1 = d2 = d3 = 0.f;
  if (a0 == m) d0 = g;
  else if (a1 == m) d1 = g;
  else if (a2 == m) d2 = g;
  else d3 = g;
}

__global__ __launch_bounds__(256) void maxpool2_bwd_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                           const float* __restrict__ dy, int N, int H, int W, int C,
                                                           float* __restrict__ dx, int relu_mask) {
  const int Ho = H >> 1, Wo = W >> 1, C4 = C >> 2;
  const int64_t total = (int64_t)N * Ho * Wo * C4;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int c4 = (int)(i % C4);
    int64_t p = i / C4;
    const int xo = (int)(p % Wo);
    p /= Wo;
    const int yo = (int)(p % Ho);
    const int n = (int)(p / Ho);
    const int64_t off = ((((int64_t)n * H + 2 * yo) * W + 2 * xo) * C) / 4 + c4;
    const float4* b = reinterpret_cast<const float4*>(x) + off;
    float4* o = reinterpret_cast<float4*>(dx) + off;
    const int64_t s1 = C4, s2 = (int64_t)W * C4, s3 = s2 + C4;
    const float4 a0 = b[0], a1 = b[s1], a2 = b[s2], a3 = b[s3];
    const float4 m = reinterpret_cast<const float4*>(y)[i];
    float4 g = reinterpret_cast<const float4*>(dy)[i];
    if (relu_mask) {  // x is a ReLU output whose own backward was deferred to its consumers: dx *= (x > 0)
      g.x = m.x > 0.f ? g.x : 0.f;
      g.y = m.y > 0.f ? g.y : 0.f;
      g.z = m.z > 0.f ? g.z : 0.f;
      g.w = m.w > 0.f ? g.w : 0.f;
    }
    float4 d0, d1, d2, d3;
    pool_bwd1(a0.x, a1.x, a2.x, a3.x, m.x, g.x, d0.x, d1.x, d2.x, d3.x);
    pool_bwd1(a0.y, a1.y, a2.y, a3.y, m.y, g.y, d0.y, d1.y, d2.y, d3.y);
    pool_bwd1(a0.z, a1.z, a2.z, a3.z, m.z, g.z, d0.z, d1.z, d2.z, d3.z);
    pool_bwd1(a0.w, a1.w, a2.w, a3.w, m.w, g.w, d0.w, d1.w, d2.w, d3.w);
    o[0] = d0;
    o[s1] = d1;
    o[s2] = d2;
    o[s3] = d3;
  }
}

extern "C" int scan_maxpool2x2_forward(const float* x, int32_t N, int32_t H, int32_t W, int32_t C, float* y,
                                       void* stream) {
  SCAN_CHECK_ARG(x && y && N > 0 && H > 0 && W > 0 && C > 0, "maxpool2x2_forward: bad arguments");
  SCAN_CHECK_ARG((H & 1) == 0 && (W & 1) == 0 && (C & 3) == 0, "maxpool2x2_forward: H, W must be even and C %% 4 == 0");
  SCAN_CHECK_ARG(aligned16(x) && aligned16(y), "maxpool2x2_forward: x and y must be 16-byte aligned");
  const int64_t total = (int64_t)N * (H / 2) * (W / 2) * (C / 4);
  hipLaunchKernelGGL(maxpool2_fwd_kernel, dim3(grid_for(total, 256)), dim3(256), 0, as_stream(stream), x, N, H, W, C, y);
  SCAN_LAUNCH_CHECK("maxpool2_fwd");
  return 0;
}

extern "C" int scan_maxpool2x2_backward(const float* x, const float* y, const float* dy, int32_t N, int32_t H,
                                        int32_t W, int32_t C, float* dx, int32_t relu_mask, void* stream) {
  SCAN_CHECK_ARG(x && y && dy && dx && N > 0 && H > 0 && W > 0 && C > 0, "maxpool2x2_backward: bad arguments");
  SCAN_CHECK_ARG((H & 1) == 0 && (W & 1) == 0 && (C & 3) == 0, "maxpool2x2_backward: H, W must be even and C %% 4 == 0");
  SCAN_CHECK_ARG(aligned16(x) && aligned16(y) && aligned16(dy) && aligned16(dx),
                 "maxpool2x2_backward: x, y, dy and dx must be 16-byte aligned");
  const int64_t total = (int64_t)N * (H / 2) * (W / 2) * (C / 4);
  hipLaunchKernelGGL(maxpool2_bwd_kernel, dim3(grid_for(total, 256)), dim3(256), 0, as_stream(stream), x, y, dy, N, H, W,
                     C, dx, relu_mask);
  SCAN_LAUNCH_CHECK("maxpool2_bwd");
  return 0;
}

// ------------------------------------------------------------------------------------------
// ResNet stem pooling: 3x3 / stride 2 / pad 1 max-pool on NHWC rows (F.max_pool2d(x, 3, 2, 1) in BaseStem.forward,
// reference backbone/resnet.py:335).  Forward only: the stem is frozen whenever FREEZE_CONV_BODY_AT >= 1 (default 2).
__global__ __launch_bounds__(256) void maxpool3s2_fwd_kernel(const float* __restrict__ x, int N, int H, int W, int C,
                                                             int Ho, int Wo, float* __restrict__ y) {
  const int C4 = C >> 2;
  const int64_t total = (int64_t)N * Ho * Wo * C4;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int c4 = (int)(i % C4);
    int64_t p = i / C4;
    const int xo = (int)(p % Wo);
    p /= Wo;
    const int yo = (int)(p % Ho);
    const int n = (int)(p / Ho);
    float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
      const int yy = 2 * yo - 1 + dy;
      if (yy < 0 || yy >= H) continue;
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) {
        const int xx = 2 * xo - 1 + dx;
        if (xx < 0 || xx >= W) continue;
        const float4 v = reinterpret_cast<const float4*>(x + (((int64_t)n * H + yy) * W + xx) * C)[c4];
        m.x = fmaxf(m.x, v.x);
        m.y = fmaxf(m.y, v.y);
        m.z = fmaxf(m.z, v.z);
        m.w = fmaxf(m.w, v.w);
      }
    }
    reinterpret_cast<float4*>(y)[i] = m;
  }
}

extern "C" int scan_maxpool3x3s2_forward(const float* x, int32_t N, int32_t H, int32_t W, int32_t C, float* y,
                                         void* stream) {
  SCAN_CHECK_ARG(x && y && N > 0 && H > 0 && W > 0 && C > 0 && (C & 3) == 0,
                 "maxpool3x3s2_forward: bad arguments (C %% 4 == 0 required)");
  SCAN_CHECK_ARG(aligned16(x) && aligned16(y), "maxpool3x3s2_forward: x and y must be 16-byte aligned");
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  const int64_t total = (int64_t)N * Ho * Wo * (C / 4);
  hipLaunchKernelGGL(maxpool3s2_fwd_kernel, dim3(grid_for(total, 256)), dim3(256), 0, as_stream(stream), x, N, H, W, C,
                     Ho, Wo, y);
  SCAN_LAUNCH_CHECK("maxpool3s2_fwd");
  return 0;
}

// residual join of a bottleneck block: y = max(a + b, 0)  (out += identity; F.relu_(out), resnet.py:312-313).
// The backward is scan_relu_backward(dy, y) handed to both branches.
__global__ __launch_bounds__(256) void add_relu_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                       float* __restrict__ y, int64_t n) {
  const int64_t n4 = n >> 2;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 u = reinterpret_cast<const float4*>(a)[i], v = reinterpret_cast<const float4*>(b)[i];
    float4 o;
    o.x = fmaxf(u.x + v.x, 0.f);
    o.y = fmaxf(u.y + v.y, 0.f);
    o.z = fmaxf(u.z + v.z, 0.f);
    o.w = fmaxf(u.w + v.w, 0.f);
    reinterpret_cast<float4*>(y)[i] = o;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0)
    for (int64_t i = n4 << 2; i < n; ++i) y[i] = fmaxf(a[i] + b[i], 0.f);
}

__global__ __launch_bounds__(256) void add_relu_scalar_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                              float* __restrict__ y, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    y[i] = fmaxf(a[i] + b[i], 0.f);
}

extern "C" int scan_add_relu(const float* a, const float* b, float* y, int64_t n, void* stream) {
  SCAN_CHECK_ARG(a && b && y && n >= 0, "add_relu: bad arguments");
  if (n == 0) return 0;
  if (aligned16(a) && aligned16(b) && aligned16(y))
    hipLaunchKernelGGL(add_relu_kernel, dim3(grid_for(n / 4 + 1, 256)), dim3(256), 0, as_stream(stream), a, b, y, n);
  else  // a pointer that is not 16-byte aligned: the same add and max, one float per lane
    hipLaunchKernelGGL(add_relu_scalar_kernel, dim3(grid_for(n, 256)), dim3(256), 0, as_stream(stream), a, b, y, n);
  SCAN_LAUNCH_CHECK("add_relu");
  return 0;
}

// ------------------------------------------------------------------ FPN top-down join (reference backbone/fpn.py:62-75)
// y = lateral + F.interpolate(coarse, scale_factor=2, mode="nearest") on NHWC rows: lateral [N, 2h, 2w, C], coarse
// [N, h, w, C].  One pass (read 1.25 C floats per output pixel, write C) instead of the expand / reshape copy of the
// up-sampled map followed by an add.  Backward: d_lateral = g itself; d_coarse = the 2x2 window sums of g.
__global__ __launch_bounds__(256) void upsample2x_add_kernel(const float* __restrict__ lat, const float* __restrict__ coarse,
                                                             int N, int h, int w, int C4, float* __restrict__ y) {
  const int64_t total = (int64_t)N * 4 * h * w * C4;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % C4);
    int64_t p = i / C4;
    const int x = (int)(p % (2 * w));
    p /= 2 * w;
    const int yy = (int)(p % (2 * h));
    const int n = (int)(p / (2 * h));
    const float4 a = reinterpret_cast<const float4*>(lat)[i];
    const float4 b = reinterpret_cast<const float4*>(coarse)[(((int64_t)n * h + (yy >> 1)) * w + (x >> 1)) * C4 + c];
    reinterpret_cast<float4*>(y)[i] = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
  }
}

__global__ __launch_bounds__(256) void downsample2x_sum_kernel(const float* __restrict__ g, int N, int h, int w, int C4,
                                                               float* __restrict__ d) {
  const int64_t total = (int64_t)N * h * w * C4;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % C4);
    int64_t p = i / C4;
    const int x = (int)(p % w);
    p /= w;
    const int yy = (int)(p % h);
    const int n = (int)(p / h);
    const float4* r0 = reinterpret_cast<const float4*>(g) + (((int64_t)n * 2 * h + 2 * yy) * 2 * w + 2 * x) * C4 + c;
    const float4* r1 = r0 + (int64_t)2 * w * C4;
    const float4 a = r0[0], b = r0[C4], e = r1[0], f = r1[C4];
    // the order of torch's sum over the (2, 2) window axes of the expanded view: rows first, then columns
    reinterpret_cast<float4*>(d)[i] = make_float4((a.x + b.x) + (e.x + f.x), (a.y + b.y) + (e.y + f.y),
                                                  (a.z + b.z) + (e.z + f.z), (a.w + b.w) + (e.w + f.w));
  }
}

extern "C" int scan_upsample2x_add(const float* lat, const float* coarse, int32_t N, int32_t h, int32_t w, int32_t C,
                                   float* y, void* stream) {
  SCAN_CHECK_ARG(lat && coarse && y && N >= 1 && h >= 1 && w >= 1 && C >= 4 && C % 4 == 0,
                 "upsample2x_add: bad arguments (C=%d must be a multiple of 4)", C);
  SCAN_CHECK_ARG(aligned16(lat) && aligned16(coarse) && aligned16(y), "upsample2x_add: lat, coarse and y must be 16-byte aligned");
  const int64_t n4 = (int64_t)N * 4 * h * w * (C / 4);
  hipLaunchKernelGGL(upsample2x_add_kernel, dim3(grid_for(n4, 256)), dim3(256), 0, as_stream(stream), lat, coarse, N, h, w,
                     C / 4, y);
  SCAN_LAUNCH_CHECK("upsample2x_add");
  return 0;
}

extern "C" int scan_downsample2x_sum(const float* g, int32_t N, int32_t h, int32_t w, int32_t C, float* d, void* stream) {
  SCAN_CHECK_ARG(g && d && N >= 1 && h >= 1 && w >= 1 && C >= 4 && C % 4 == 0,
                 "downsample2x_sum: bad arguments (C=%d must be a multiple of 4)", C);
  SCAN_CHECK_ARG(aligned16(g) && aligned16(d), "downsample2x_sum: g and d must be 16-byte aligned");
  const int64_t n4 = (int64_t)N * h * w * (C / 4);
  hipLaunchKernelGGL(downsample2x_sum_kernel, dim3(grid_for(n4, 256)), dim3(256), 0, as_stream(stream), g, N, h, w, C / 4, d);
  SCAN_LAUNCH_CHECK("downsample2x_sum");
  return 0;
}

// ---- gradient of "the rows of images [i0, i1) of a pyramid" (ops.take_images): the full pyramid's gradient in ONE pass --
// rows of the taken images copied from g (the sub-pyramid's rows, level-major), every other row zero.  Written with torch ops
// this is a zero fill of the whole matrix plus one slice copy per level.
__global__ __launch_bounds__(256) void take_images_bwd_kernel(const float* __restrict__ g, scan_pyramid_t d, int i0, int i1,
                                                              int C, float* __restrict__ out) {
  const int64_t total = d.row_off[d.n_levels] * (int64_t)C;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t m = e / C;
    const int c = (int)(e - m * C);
    const int lvl = level_of(d.row_off, d.n_levels, m);
    const int64_t hw = (int64_t)d.h[lvl] * d.w[lvl];
    const int64_t r = m - d.row_off[lvl];
    const int64_t n = r / hw;
    float v = 0.f;
    if (n >= i0 && n < i1) {
      // rows of the sub-pyramid before this level: (i1 - i0) images of every earlier level
      const int64_t sub_off = d.row_off[lvl] / d.n_images * (i1 - i0);
      v = g[(sub_off + (n - i0) * hw + (r - n * hw)) * C + c];
    }
    out[e] = v;
  }
}

extern "C" int scan_take_images_backward(const float* g, const scan_pyramid_t* d, int32_t i0, int32_t i1, int32_t C, float* out,
                                         void* stream) {
  SCAN_CHECK_ARG(g && d && out && C >= 1 && d->n_levels >= 1 && d->n_levels <= SCAN_MAX_LEVELS && 0 <= i0 && i0 < i1 &&
                     i1 <= d->n_images,
                 "take_images_backward: bad arguments");
  const int64_t total = d->row_off[d->n_levels] * (int64_t)C;
  hipLaunchKernelGGL(take_images_bwd_kernel, dim3(grid_for(total, 256)), dim3(256), 0, as_stream(stream), g, *d, i0, i1, C, out);
  SCAN_LAUNCH_CHECK("take_images_backward");
  return 0;
}

// ---- column block copy between row matrices of different row pitch (round 6): dst[r][dc0 + c] = src[r][sc0 + c] for c < ncols,
// and zeros in dst columns [dc0 + ncols, dc0 + ncols + ztail).  What the torch tier spelled as F.pad of the [M, 9] act maps to
// [M, 12] (a fill plus a narrow strided copy, and a strided slice copy back in the backward) and as buf[:, C:C + e] = extra in
// front of the class branches: one coalesced pass each here.
__global__ __launch_bounds__(256) void copy_cols_kernel(const float* __restrict__ src, int ld_src, float* __restrict__ dst,
                                                        int ld_dst, int64_t M, int ncols, int ztail) {
  const int w = ncols + ztail;
  const int64_t total = M * (int64_t)w;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = e / w;
    const int c = (int)(e - r * w);
    dst[r * ld_dst + c] = c < ncols ? src[r * ld_src + c] : 0.f;
  }
}

extern "C" int scan_copy_cols(const float* src, int32_t ld_src, float* dst, int32_t ld_dst, int64_t M, int32_t ncols,
                              int32_t ztail, void* stream) {
  SCAN_CHECK_ARG(M >= 0 && ncols >= 0 && ztail >= 0 && ld_src >= ncols && ld_dst >= ncols + ztail,
                 "copy_cols: bad arguments (M=%lld ncols=%d ztail=%d ld_src=%d ld_dst=%d)", (long long)M, ncols, ztail, ld_src, ld_dst);
  if (M == 0 || ncols + ztail == 0) return 0;
  SCAN_CHECK_ARG(src && dst, "copy_cols: null pointer");
  hipLaunchKernelGGL(copy_cols_kernel, dim3(grid_for(M * (int64_t)(ncols + ztail), 256)), dim3(256), 0, as_stream(stream), src,
                     ld_src, dst, ld_dst, M, ncols, ztail);
  SCAN_LAUNCH_CHECK("copy_cols");
  return 0;
}

// ---- paradigm (prototype) update of the middle head, reference condgraph.py:586-606 with COSINE_UPDATE_ON (round 6: one launch
// instead of ~25 one-row torch launches on the step's critical small-kernel stretch).  P [K][C][T] (slot t of class k, channel c
// at (k * C + c) * T + t), pb [K][C] the batch's class means (zero rows: class not seen).  it = the paradigm counter's value:
//   slot = it - 1 if it == T else it;   cur = P[:, :, slot]
//   m    = cosine_similarity(cur, pb, dim = 1, eps = 1e-8)      (rows normalised first, like torch: x / max(||x||, eps))
//   upd  = pb.sum(1) != 0 ? cur * m + pb * (1 - m) : cur
//   it == T: slots 0 .. T-2 <- slots 1 .. T-1;   P[:, :, slot] = upd
// One workgroup per class, C <= 1024 channels over 256 threads.
__global__ __launch_bounds__(256) void paradigm_update_kernel(float* __restrict__ P, const float* __restrict__ pb, int C, int T,
                                                              int it) {
  __shared__ float red[4];
  const int k = blockIdx.x;
  const int slot = it == T ? it - 1 : it;
  float cur[4], b[4];
  float s_cc = 0.f, s_bb = 0.f, s_b = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int c = threadIdx.x + 256 * j;
    cur[j] = c < C ? P[((int64_t)k * C + c) * T + slot] : 0.f;
    b[j] = c < C ? pb[(int64_t)k * C + c] : 0.f;
    s_cc += cur[j] * cur[j];
    s_bb += b[j] * b[j];
    s_b += b[j];
  }
  auto bsum = [&](float v) {
    float r = block_sum_256(v, red);
    __shared__ float bc;
    if (threadIdx.x == 0) bc = r;
    __syncthreads();
    r = bc;
    __syncthreads();
    return r;
  };
  const float n_c = fmaxf(sqrtf(bsum(s_cc)), 1e-8f), n_b = fmaxf(sqrtf(bsum(s_bb)), 1e-8f);
  const bool exist = bsum(s_b) != 0.f;
  float dotp = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) dotp += (cur[j] / n_c) * (b[j] / n_b);
  const float m = bsum(dotp);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int c = threadIdx.x + 256 * j;
    if (c >= C) continue;
    float* row = P + ((int64_t)k * C + c) * T;
    const float upd = exist ? cur[j] * m + b[j] * (1.f - m) : cur[j];
    if (it == T)
      for (int t = 0; t + 1 < T; ++t) row[t] = row[t + 1];
    row[slot] = upd;
  }
}

extern "C" int scan_paradigm_update(float* P, const float* pb, int32_t K, int32_t C, int32_t T, int32_t it, void* stream) {
  SCAN_CHECK_ARG(P && pb && K >= 1 && C >= 1 && C <= 1024 && T >= 1 && it >= 0 && it <= T,
                 "paradigm_update: bad arguments (K=%d C=%d T=%d it=%d)", K, C, T, it);
  hipLaunchKernelGGL(paradigm_update_kernel, dim3(K), dim3(256), 0, as_stream(stream), P, pb, C, T, it);
  SCAN_LAUNCH_CHECK("paradigm_update");
  return 0;
}
