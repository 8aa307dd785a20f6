// Region pooling on pyramid rows: ROIAlign, ROIPool, their data gradients and the FPN LevelMapper (include/scan_hip.h has the
// definitions, pinned to the reference's csrc/cuda/ROIAlign_cuda.cu, csrc/cuda/ROIPool_cuda.cu and modeling/poolers.py).
//
// x is the [M, Cs] row matrix of a pyramid, so a bilinear corner (ROIAlign) or a cell of a bin (ROIPool) is one contiguous
// channel run.  Forward: one wave works on one (ROI, bin); the ROI geometry, the sample positions, weights and cells are
// wave-uniform (formed once per sample, never per channel) and the lanes cover the channels with float4 accesses (lane * 4,
// then steps of 256 channels).  Each ROI carries its level, so one launch serves every level of an FPN pooler.
//
// Every fp32 operation is rounded on its own in the source's left-to-right order: the file is built with -ffp-contract=off.
//
// No float atomics.  The data gradients are sums over overlapping ROIs; both are formed per DESTINATION: one wave owns one
// row of dx, finds the ROIs that can reach it (64 ROIs per step, one per lane, then a ballot), and for each of them -- in
// ascending ROI order -- walks the bins and samples that touch the row, recomputing their weights with the forward's own
// code.  The inverted index of a store-then-sum design is therefore never stored: nothing is sorted, no workspace, no host
// read, also for the adaptive grid.  The order of the additions is fixed (ROI, ph, iy, corner, pw, ix, corner), so the result
// has the same bits on every run and needs no *_ordered twin.
//
// Out-of-range indices are defined behaviour: a ROI whose image index is outside [0, N) or whose level is outside the pyramid
// gives zeros (argmax -1) and no gradient.  Coordinates of any magnitude are safe: positions are tested as floats before any
// conversion to an integer (NaN: the sample is dropped), ROIPool's rounded corners are clamped to +-2^29, and an adaptive grid
// is walked only over the samples that can lie inside the map, so a loop is bounded by the map, not by the ROI.
#include <float.h>

#include "common.h"

namespace {

struct Scales {
  float s[SCAN_MAX_LEVELS];
};

constexpr int GRID_MAX = 32768;  // cap of the adaptive grid per axis (the reference's int product gh * gw overflows at 46341)

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float4 keep_below(float4 v, int c4, int C) {
  if (c4 + 0 >= C) v.x = 0.f;
  if (c4 + 1 >= C) v.y = 0.f;
  if (c4 + 2 >= C) v.z = 0.f;
  if (c4 + 3 >= C) v.w = 0.f;
  return v;
}

// image index and level of ROI k; false: outside the batch / the pyramid
__device__ __forceinline__ bool roi_place(const float* __restrict__ rois, const int32_t* __restrict__ levels,
                                          const scan_pyramid_t& d, int64_t k, int& n, int& lvl) {
  const float b = truncf(rois[k * 5]);  // int roi_batch_ind = offset_bottom_rois[0]
  lvl = levels ? levels[k] : 0;
  n = 0;
  if (!(b >= 0.f && b < (float)d.n_images) || lvl < 0 || lvl >= d.n_levels) return false;
  n = (int)b;
  return true;
}

// ---------------------------------------------------------------- ROIAlign geometry (ROIAlign_cuda.cu:78-104)
struct AlignRoi {
  bool ok;
  int n, lvl, gh, gw;
  float start_h, start_w, roi_h, roi_w, bin_h, bin_w, count;
};

__device__ __forceinline__ int adaptive_grid(float roi, int P) {
  const float g = ceilf(roi / (float)P);  // ceil(roi_height / pooled_height)
  return g >= (float)GRID_MAX ? GRID_MAX : (g >= 1.f ? (int)g : 1);  // roi >= 1, so g >= 1 unless roi is NaN
}

__device__ __forceinline__ AlignRoi align_roi(const float* __restrict__ rois, const int32_t* __restrict__ levels,
                                              const Scales& sc, const scan_pyramid_t& d, int64_t k, int PH, int PW, int sr) {
  AlignRoi r;
  r.ok = roi_place(rois, levels, d, k, r.n, r.lvl);
  const float s = sc.s[r.ok ? r.lvl : 0];
  const float* __restrict__ q = rois + k * 5;
  r.start_w = q[1] * s;
  r.start_h = q[2] * s;
  const float end_w = q[3] * s, end_h = q[4] * s;
  r.roi_w = fmaxf(end_w - r.start_w, 1.f);  // malformed ROIs are forced to 1x1 (a NaN extent too)
  r.roi_h = fmaxf(end_h - r.start_h, 1.f);
  r.bin_h = r.roi_h / (float)PH;
  r.bin_w = r.roi_w / (float)PW;
  r.gh = sr > 0 ? sr : adaptive_grid(r.roi_h, PH);
  r.gw = sr > 0 ? sr : adaptive_grid(r.roi_w, PW);
  r.count = (float)(r.gh * r.gw);
  return r;
}

// one axis of a sample (ROIAlign_cuda.cu:109 / :22-51): position, the two cells and their weights
struct Axis {
  bool live;    // false: outside [-1, size] (or NaN): the sample is 0 and has no gradient
  float pos;    // the position as first formed
  int lo, hi;   // cells
  float l, h;   // weight of hi (y - y_low) and of lo (1 - l)
};

__device__ __forceinline__ Axis sample_axis(float start, float bin, int p, int i, int g, int size) {
  Axis a;
  float y = start + (float)p * bin + ((float)i + .5f) * bin / (float)g;
  a.pos = y;
  a.live = y >= -1.f && y <= (float)size;  // !(y < -1 || y > size); NaN: dropped
  a.lo = a.hi = 0;
  a.l = 0.f, a.h = 0.f;
  if (!a.live) return a;
  if (y <= 0.f) y = 0.f;
  a.lo = (int)y;
  if (a.lo >= size - 1) {
    a.hi = a.lo = size - 1;
    y = (float)a.lo;
  } else {
    a.hi = a.lo + 1;
  }
  a.l = y - (float)a.lo;
  a.h = 1.f - a.l;
  return a;
}

// [lo, hi) within [0, g): a superset of the sample indices i of bin p whose position can lie in [ylo, yhi].  A bin clear of
// the interval is skipped, small grids are otherwise walked whole; a larger (adaptive) one is cut in fp64 with a margin for
// the fp32 rounding of the position, so the walk is bounded by the interval, not by the ROI.  Every sample inside is still
// tested exactly by sample_axis.
__device__ __forceinline__ void sample_range(float start, float bin, int p, int g, float ylo, float yhi, int& lo, int& hi) {
  lo = 0, hi = g;
  // the samples of bin p lie in [start + p bin, start + (p + 1) bin] up to rounding: a bin clear of the interval has none
  const float slack = 1e-3f + 1e-6f * (fabsf(start) + (float)(p + 1) * bin);
  if (start + (float)(p + 1) * bin + slack < ylo || start + (float)p * bin - slack > yhi) {
    hi = 0;
    return;
  }
  if (g <= 8) return;
  const double base = (double)start + (double)p * (double)bin, step = (double)bin / (double)g;
  const double err = 1e-6 * (fabs((double)start) + (double)(p + 1) * (double)bin) + 1e-3;  // >> 4 fp32 roundings
  const double a = ((double)ylo - err - base) / step - 0.5, b = ((double)yhi + err - base) / step - 0.5;
  if (!(a == a) || !(b == b)) {  // NaN geometry: every position is NaN, every sample is dropped
    lo = hi = 0;
    return;
  }
  lo = a <= 1.0 ? 0 : (a >= (double)g ? g : (int)a - 1);
  hi = b < 0.0 ? 0 : (b >= (double)(g - 2) ? g : (int)b + 2);
  if (hi < lo) hi = lo;
}

__global__ __launch_bounds__(256) void roi_align_fwd_kernel(const float* __restrict__ x, scan_pyramid_t d, int C, int Cs,
                                                            const float* __restrict__ rois, const int32_t* __restrict__ levels,
                                                            Scales sc, int PH, int PW, int sr, float* __restrict__ y,
                                                            int64_t n_bins) {
  const int lane = threadIdx.x & 63;
  const int64_t step = (int64_t)gridDim.x * 4;
  const int PB = PH * PW;
  for (int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); t < n_bins; t += step) {
    const int64_t k = t / PB;
    const int b = (int)(t - k * PB), ph = b / PW, pw = b - ph * PW;
    const AlignRoi r = align_roi(rois, levels, sc, d, k, PH, PW, sr);
    float* __restrict__ dst = y + t * Cs;
    if (!r.ok) {
      for (int c4 = lane * 4; c4 < Cs; c4 += 256) *reinterpret_cast<float4*>(dst + c4) = make_float4(0.f, 0.f, 0.f, 0.f);
      continue;
    }
    const int H = d.h[r.lvl], W = d.w[r.lvl];
    const float* __restrict__ img = x + (d.row_off[r.lvl] + (int64_t)r.n * H * W) * Cs;
    int iy0, iy1, ix0, ix1;
    sample_range(r.start_h, r.bin_h, ph, r.gh, -1.f, (float)H, iy0, iy1);
    sample_range(r.start_w, r.bin_w, pw, r.gw, -1.f, (float)W, ix0, ix1);
    for (int c4 = lane * 4; c4 < Cs; c4 += 256) {
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int iy = iy0; iy < iy1; ++iy) {
        const Axis ay = sample_axis(r.start_h, r.bin_h, ph, iy, r.gh, H);
        if (!ay.live) continue;
        for (int ix = ix0; ix < ix1; ++ix) {
          const Axis ax = sample_axis(r.start_w, r.bin_w, pw, ix, r.gw, W);
          if (!ax.live) continue;
          const float w1 = ay.h * ax.h, w2 = ay.h * ax.l, w3 = ay.l * ax.h, w4 = ay.l * ax.l;
          const float4 v1 = ld4(img + ((int64_t)ay.lo * W + ax.lo) * Cs + c4), v2 = ld4(img + ((int64_t)ay.lo * W + ax.hi) * Cs + c4),
                       v3 = ld4(img + ((int64_t)ay.hi * W + ax.lo) * Cs + c4), v4 = ld4(img + ((int64_t)ay.hi * W + ax.hi) * Cs + c4);
          acc.x += w1 * v1.x + w2 * v2.x + w3 * v3.x + w4 * v4.x;
          acc.y += w1 * v1.y + w2 * v2.y + w3 * v3.y + w4 * v4.y;
          acc.z += w1 * v1.z + w2 * v2.z + w3 * v3.z + w4 * v4.z;
          acc.w += w1 * v1.w + w2 * v2.w + w3 * v3.w + w4 * v4.w;
        }
      }
      acc.x /= r.count, acc.y /= r.count, acc.z /= r.count, acc.w /= r.count;
      *reinterpret_cast<float4*>(dst + c4) = keep_below(acc, c4, C);
    }
  }
}

// the samples themselves, for tests: one thread per (ROI, bin, iy < gmax, ix < gmax)
__global__ __launch_bounds__(256) void roi_align_samples_kernel(scan_pyramid_t d, const float* __restrict__ rois,
                                                                const int32_t* __restrict__ levels, Scales sc, int PH, int PW,
                                                                int sr, int gmax, int32_t* __restrict__ grid,
                                                                float* __restrict__ pos, float* __restrict__ wgt,
                                                                int32_t* __restrict__ cell, int64_t n_samples) {
  const int PB = PH * PW, G2 = gmax * gmax;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n_samples; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t t = e / G2, k = t / PB;
    const int s = (int)(e - t * G2), iy = s / gmax, ix = s - iy * gmax;
    const int b = (int)(t - k * PB), ph = b / PW, pw = b - ph * PW;
    const AlignRoi r = align_roi(rois, levels, sc, d, k, PH, PW, sr);
    if (b == 0 && s == 0) grid[2 * k] = r.ok ? r.gh : 0, grid[2 * k + 1] = r.ok ? r.gw : 0;
    float p2[2] = {0.f, 0.f}, w4[4] = {0.f, 0.f, 0.f, 0.f};
    int c4[4] = {-1, -1, -1, -1};
    if (r.ok && iy < r.gh && ix < r.gw) {
      const int H = d.h[r.lvl], W = d.w[r.lvl];
      const Axis ay = sample_axis(r.start_h, r.bin_h, ph, iy, r.gh, H), ax = sample_axis(r.start_w, r.bin_w, pw, ix, r.gw, W);
      p2[0] = ay.pos, p2[1] = ax.pos;
      if (ay.live && ax.live) {
        w4[0] = ay.h * ax.h, w4[1] = ay.h * ax.l, w4[2] = ay.l * ax.h, w4[3] = ay.l * ax.l;
        c4[0] = ay.lo * W + ax.lo, c4[1] = ay.lo * W + ax.hi, c4[2] = ay.hi * W + ax.lo, c4[3] = ay.hi * W + ax.hi;
      }
    }
    pos[2 * e] = p2[0], pos[2 * e + 1] = p2[1];
    for (int q = 0; q < 4; ++q) wgt[4 * e + q] = w4[q], cell[4 * e + q] = c4[q];
  }
}

// data gradient of ROIAlign: dx[p][:] = sum over the samples with a corner on row p of (dy * w) / count, in a fixed order
__global__ __launch_bounds__(256) void roi_align_bwd_kernel(const float* __restrict__ dy, scan_pyramid_t d, int C, int Cs,
                                                            const float* __restrict__ rois, const int32_t* __restrict__ levels,
                                                            Scales sc, int64_t K, int PH, int PW, int sr,
                                                            float* __restrict__ dx, int64_t M) {
  const int lane = threadIdx.x & 63;
  const int64_t step = (int64_t)gridDim.x * 4;
  for (int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); p < M; p += step) {
    const RowCoord rc = decode_row(d, p);
    const int H = d.h[rc.lvl], W = d.w[rc.lvl];
    const float Yf = (float)rc.y, Xf = (float)rc.x;
    // the positions whose cells include this row: [Y - 1, Y + 1], widened by the clamps at the two borders (a position in
    // [-1, 0] counts as 0: cells 0 and 1; one in [H - 1, H] as H - 1)
    const float ylo = rc.y <= 1 ? -1.f : Yf - 1.f, yhi = rc.y >= H - 1 ? (float)H : Yf + 1.f;
    const float xlo = rc.x <= 1 ? -1.f : Xf - 1.f, xhi = rc.x >= W - 1 ? (float)W : Xf + 1.f;
    for (int cb = 0; cb < Cs; cb += 256) {  // uniform trip count: every lane takes part in the ballots
      const int c4 = cb + lane * 4;
      const bool active = c4 < Cs;
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int64_t k0 = 0; k0 < K; k0 += 64) {
        // one ROI per lane: the cells of a sample at q are floor(q) and floor(q) + 1 (q clamped to 0 from below), so a ROI
        // reaches row Y only if start - 1 <= Y <= max(end, 0) + 1, up to the rounding of the positions
        AlignRoi mine;
        bool hit = false;
        if (k0 + lane < K) {
          mine = align_roi(rois, levels, sc, d, k0 + lane, PH, PW, sr);
          const float mh = 1.001f + 1e-6f * (fabsf(mine.start_h) + mine.roi_h), mw = 1.001f + 1e-6f * (fabsf(mine.start_w) + mine.roi_w);
          hit = mine.ok && mine.lvl == rc.lvl && mine.n == rc.n && Yf + mh >= mine.start_h &&
                Yf - mh <= fmaxf(mine.start_h + mine.roi_h, 0.f) && Xf + mw >= mine.start_w &&
                Xf - mw <= fmaxf(mine.start_w + mine.roi_w, 0.f);
        } else {
          mine.start_h = mine.start_w = mine.bin_h = mine.bin_w = mine.count = 0.f;
          mine.gh = mine.gw = 0;
        }
        unsigned long long todo = __ballot(hit);
        while (todo) {
          const int j = __ffsll((long long)todo) - 1;
          todo &= todo - 1;
          const int64_t k = k0 + j;
          AlignRoi r;  // lane j's geometry, broadcast
          r.start_h = __shfl(mine.start_h, j, 64), r.start_w = __shfl(mine.start_w, j, 64);
          r.bin_h = __shfl(mine.bin_h, j, 64), r.bin_w = __shfl(mine.bin_w, j, 64);
          r.gh = __shfl(mine.gh, j, 64), r.gw = __shfl(mine.gw, j, 64), r.count = __shfl(mine.count, j, 64);
          for (int ph = 0; ph < PH; ++ph) {
            int iy0, iy1;
            sample_range(r.start_h, r.bin_h, ph, r.gh, ylo, yhi, iy0, iy1);
            for (int iy = iy0; iy < iy1; ++iy) {
              const Axis ay = sample_axis(r.start_h, r.bin_h, ph, iy, r.gh, H);
              if (!ay.live) continue;
              for (int cy = 0; cy < 2; ++cy) {
                if ((cy ? ay.hi : ay.lo) != rc.y) continue;
                const float wy = cy ? ay.l : ay.h;
                for (int pw = 0; pw < PW; ++pw) {
                  int ix0, ix1;
                  sample_range(r.start_w, r.bin_w, pw, r.gw, xlo, xhi, ix0, ix1);
                  const float* __restrict__ g = dy + ((k * PH + ph) * PW + pw) * Cs + c4;
                  for (int ix = ix0; ix < ix1; ++ix) {
                    const Axis ax = sample_axis(r.start_w, r.bin_w, pw, ix, r.gw, W);
                    if (!ax.live) continue;
                    for (int cx = 0; cx < 2; ++cx) {
                      if ((cx ? ax.hi : ax.lo) != rc.x) continue;
                      const float w = wy * (cx ? ax.l : ax.h);
                      if (active) {
                        const float4 gv = ld4(g);
                        acc.x += gv.x * w / r.count, acc.y += gv.y * w / r.count;
                        acc.z += gv.z * w / r.count, acc.w += gv.w * w / r.count;
                      }
                    }
                  }
                }
              }
            }
          }
        }
      }
      if (active) *reinterpret_cast<float4*>(dx + p * Cs + c4) = keep_below(acc, c4, C);
    }
  }
}

// ---------------------------------------------------------------- ROIPool geometry (ROIPool_cuda.cu:28-57)
struct PoolRoi {
  bool ok;
  int n, lvl, start_h, start_w, roi_h, roi_w;
  float bin_h, bin_w;
};

__device__ __forceinline__ int round_clamped(float v) {
  const float LIM = 536870912.f;  // 2^29: differences and sums of two such values stay inside int32
  return (int)fminf(fmaxf(roundf(v), -LIM), LIM);  // half away from zero; NaN -> -2^29
}

__device__ __forceinline__ PoolRoi pool_roi(const float* __restrict__ rois, const int32_t* __restrict__ levels, const Scales& sc,
                                            const scan_pyramid_t& d, int64_t k, int PH, int PW) {
  PoolRoi r;
  r.ok = roi_place(rois, levels, d, k, r.n, r.lvl);
  const float s = sc.s[r.ok ? r.lvl : 0];
  const float* __restrict__ q = rois + k * 5;
  r.start_w = round_clamped(q[1] * s);
  r.start_h = round_clamped(q[2] * s);
  const int end_w = round_clamped(q[3] * s), end_h = round_clamped(q[4] * s);
  r.roi_w = max(end_w - r.start_w + 1, 1);
  r.roi_h = max(end_h - r.start_h + 1, 1);
  r.bin_h = (float)r.roi_h / (float)PH;
  r.bin_w = (float)r.roi_w / (float)PW;
  return r;
}

// bin p of an axis: [lo, hi) clipped to [0, size]
__device__ __forceinline__ void pool_bin(int start, float bin, int p, int size, int& lo, int& hi) {
  lo = (int)floorf((float)p * bin);
  hi = (int)ceilf((float)(p + 1) * bin);
  lo = min(max(lo + start, 0), size);
  hi = min(max(hi + start, 0), size);
}

__global__ __launch_bounds__(256) void roi_pool_fwd_kernel(const float* __restrict__ x, scan_pyramid_t d, int C, int Cs,
                                                           const float* __restrict__ rois, const int32_t* __restrict__ levels,
                                                           Scales sc, int PH, int PW, float* __restrict__ y,
                                                           int32_t* __restrict__ argmax, int64_t n_bins) {
  const int lane = threadIdx.x & 63;
  const int64_t step = (int64_t)gridDim.x * 4;
  const int PB = PH * PW;
  for (int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); t < n_bins; t += step) {
    const int64_t k = t / PB;
    const int b = (int)(t - k * PB), ph = b / PW, pw = b - ph * PW;
    const PoolRoi r = pool_roi(rois, levels, sc, d, k, PH, PW);
    int hs = 0, he = 0, ws = 0, we = 0, W = 1;
    const float* __restrict__ img = x;
    if (r.ok) {
      const int H = d.h[r.lvl];
      W = d.w[r.lvl];
      img = x + (d.row_off[r.lvl] + (int64_t)r.n * H * W) * Cs;
      pool_bin(r.start_h, r.bin_h, ph, H, hs, he);
      pool_bin(r.start_w, r.bin_w, pw, W, ws, we);
    }
    const bool empty = he <= hs || we <= ws;
    for (int c4 = lane * 4; c4 < Cs; c4 += 256) {
      const float m0 = empty ? 0.f : -FLT_MAX;
      float4 mv = make_float4(m0, m0, m0, m0);
      int4 mi = make_int4(-1, -1, -1, -1);
      if (!empty)
        for (int h = hs; h < he; ++h)
          for (int w = ws; w < we; ++w) {
            const int cell = h * W + w;
            const float4 v = ld4(img + (int64_t)cell * Cs + c4);
            if (v.x > mv.x) mv.x = v.x, mi.x = cell;
            if (v.y > mv.y) mv.y = v.y, mi.y = cell;
            if (v.z > mv.z) mv.z = v.z, mi.z = cell;
            if (v.w > mv.w) mv.w = v.w, mi.w = cell;
          }
      if (c4 + 0 >= C) mv.x = 0.f, mi.x = -1;  // padding columns
      if (c4 + 1 >= C) mv.y = 0.f, mi.y = -1;
      if (c4 + 2 >= C) mv.z = 0.f, mi.z = -1;
      if (c4 + 3 >= C) mv.w = 0.f, mi.w = -1;
      *reinterpret_cast<float4*>(y + t * Cs + c4) = mv;
      *reinterpret_cast<int4*>(argmax + t * Cs + c4) = mi;
    }
  }
}

// data gradient of ROIPool: dx[p][c] = sum of dy over the (ROI, bin) whose argmax for channel c is this row's cell, in
// ascending (ROI, ph, pw) order.  Only bins whose window contains the cell can name it, so only those are read.
__global__ __launch_bounds__(256) void roi_pool_bwd_kernel(const float* __restrict__ dy, const int32_t* __restrict__ argmax,
                                                           scan_pyramid_t d, int C, int Cs, const float* __restrict__ rois,
                                                           const int32_t* __restrict__ levels, Scales sc, int64_t K, int PH,
                                                           int PW, float* __restrict__ dx, int64_t M) {
  const int lane = threadIdx.x & 63;
  const int64_t step = (int64_t)gridDim.x * 4;
  for (int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); p < M; p += step) {
    const RowCoord rc = decode_row(d, p);
    const int H = d.h[rc.lvl], W = d.w[rc.lvl];
    const int cell = rc.y * W + rc.x;
    for (int cb = 0; cb < Cs; cb += 256) {  // uniform trip count: every lane takes part in the ballots
      const int c4 = cb + lane * 4;
      const bool active = c4 < Cs;
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int64_t k0 = 0; k0 < K; k0 += 64) {
        PoolRoi mine;
        bool hit = false;
        if (k0 + lane < K) {
          mine = pool_roi(rois, levels, sc, d, k0 + lane, PH, PW);
          // the bins of an axis lie in [start, start + ceil(P * bin)], and P * bin is roi up to one rounding
          hit = mine.ok && mine.lvl == rc.lvl && mine.n == rc.n && rc.y >= mine.start_h && rc.y <= mine.start_h + mine.roi_h + 1 &&
                rc.x >= mine.start_w && rc.x <= mine.start_w + mine.roi_w + 1;
        } else {
          mine.start_h = mine.start_w = 0;
          mine.bin_h = mine.bin_w = 0.f;
        }
        unsigned long long todo = __ballot(hit);
        while (todo) {
          const int j = __ffsll((long long)todo) - 1;
          todo &= todo - 1;
          const int64_t k = k0 + j;
          PoolRoi r;  // lane j's geometry, broadcast
          r.start_h = __shfl(mine.start_h, j, 64), r.start_w = __shfl(mine.start_w, j, 64);
          r.bin_h = __shfl(mine.bin_h, j, 64), r.bin_w = __shfl(mine.bin_w, j, 64);
          for (int ph = 0; ph < PH; ++ph) {
            int hs, he;
            pool_bin(r.start_h, r.bin_h, ph, H, hs, he);
            if (rc.y < hs || rc.y >= he) continue;
            for (int pw = 0; pw < PW; ++pw) {
              int ws, we;
              pool_bin(r.start_w, r.bin_w, pw, W, ws, we);
              if (rc.x < ws || rc.x >= we || !active) continue;
              const int64_t o = ((k * PH + ph) * PW + pw) * Cs + c4;
              const int4 a = *reinterpret_cast<const int4*>(argmax + o);
              const float4 g = ld4(dy + o);
              if (a.x == cell) acc.x += g.x;
              if (a.y == cell) acc.y += g.y;
              if (a.z == cell) acc.z += g.z;
              if (a.w == cell) acc.w += g.w;
            }
          }
        }
      }
      if (active) *reinterpret_cast<float4*>(dx + p * Cs + c4) = keep_below(acc, c4, C);
    }
  }
}

// ---------------------------------------------------------------- LevelMapper (modeling/poolers.py:31-42)
__global__ __launch_bounds__(256) void roi_levels_kernel(const float* __restrict__ boxes, int ld, int64_t K, float k_min,
                                                         float k_max, float s0, float lvl0, float eps,
                                                         int32_t* __restrict__ levels) {
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < K; k += (int64_t)gridDim.x * blockDim.x) {
    const float* __restrict__ b = boxes + k * ld;
    const float area = (b[2] - b[0] + 1.f) * (b[3] - b[1] + 1.f);  // BoxList.area(), xyxy
    const float s = sqrtf(area);
    float t = floorf(lvl0 + log2f(s / s0 + eps));
    t = fminf(fmaxf(t, k_min), k_max);  // NaN (a negative area): k_min
    levels[k] = (int32_t)t - (int32_t)k_min;
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int check_pyramid(const char* name, const scan_pyramid_t* d) {
  SCAN_CHECK_ARG(d->n_levels >= 1 && d->n_levels <= SCAN_MAX_LEVELS && d->n_images >= 1 && d->row_off[0] == 0, "%s: bad pyramid",
                 name);
  for (int l = 0; l < d->n_levels; ++l)
    SCAN_CHECK_ARG(d->h[l] >= 1 && d->w[l] >= 1 && d->row_off[l + 1] - d->row_off[l] == (int64_t)d->n_images * d->h[l] * d->w[l],
                   "%s: bad pyramid (level %d)", name, l);
  // cells (h * W + w) and rows are int32 in the argmax and in the row decode
  SCAN_CHECK_ARG(d->row_off[d->n_levels] < (int64_t)1 << 31, "%s: M=%lld rows must stay below 2^31", name,
                 (long long)d->row_off[d->n_levels]);
  return 0;
}

// everything the four pooling entry points share; K == 0 is legal (the caller returns before a launch)
int check_pool(const char* name, const scan_pyramid_t* d, int32_t C, int32_t Cs, const float* rois, const float* scales, int64_t K,
               int32_t PH, int32_t PW, Scales* sc) {
  SCAN_CHECK_ARG(d && scales && (rois || K == 0), "%s: null pointer", name);
  SCAN_CHECK_ARG(Cs > 0 && Cs % 4 == 0, "%s: Cs=%d must be a positive multiple of 4", name, Cs);
  SCAN_CHECK_ARG(C >= 1 && C <= Cs, "%s: C=%d must be in [1, Cs=%d]", name, C, Cs);
  SCAN_CHECK_ARG(PH >= 1 && PW >= 1 && (int64_t)PH * PW < (int64_t)1 << 31, "%s: pooled size %d x %d must be >= 1 x 1", name, PH, PW);
  SCAN_CHECK_ARG(K >= 0 && K < (int64_t)1 << 31 && K * PH * PW < (int64_t)1 << 31, "%s: K=%lld, K * PH * PW must stay below 2^31", name, (long long)K);
  if (check_pyramid(name, d)) return -1;
  for (int l = 0; l < SCAN_MAX_LEVELS; ++l) sc->s[l] = l < d->n_levels ? scales[l] : 0.f;
  return 0;
}

}  // namespace

extern "C" int scan_roi_levels(const float* boxes, int32_t ld, int64_t K, float k_min, float k_max, float s0, float lvl0, float eps,
                               int32_t* levels, void* stream) {
  const char* name = "roi_levels";
  SCAN_CHECK_ARG(K >= 0 && K < (int64_t)1 << 31, "%s: K=%lld must be in [0, 2^31)", name, (long long)K);
  if (K == 0) return 0;
  SCAN_CHECK_ARG(boxes && levels, "%s: null pointer", name);
  SCAN_CHECK_ARG(ld >= 4, "%s: ld=%d must be >= 4", name, ld);
  SCAN_CHECK_ARG(k_min <= k_max && k_min == floorf(k_min) && fabsf(k_min) < 64.f && fabsf(k_max) < 64.f,
                 "%s: k_min=%g must be an integer <= k_max=%g", name, (double)k_min, (double)k_max);
  hipLaunchKernelGGL(roi_levels_kernel, dim3(grid_for(K, 256)), dim3(256), 0, as_stream(stream), boxes, ld, K, k_min, k_max, s0,
                     lvl0, eps, levels);
  SCAN_LAUNCH_CHECK(name);
  return 0;
}

extern "C" int scan_roi_align_forward(const float* x, const scan_pyramid_t* d, int32_t C, int32_t Cs, const float* rois,
                                      const int32_t* levels, const float* scales, int64_t K, int32_t PH, int32_t PW,
                                      int32_t sampling_ratio, float* y, void* stream) {
  const char* name = "roi_align_forward";
  Scales sc;
  if (check_pool(name, d, C, Cs, rois, scales, K, PH, PW, &sc)) return -1;
  SCAN_CHECK_ARG(sampling_ratio <= GRID_MAX, "%s: sampling_ratio=%d must be <= %d", name, sampling_ratio, GRID_MAX);
  if (K == 0) return 0;
  SCAN_CHECK_ARG(x && y, "%s: null pointer", name);
  SCAN_CHECK_ARG(aligned16(x) && aligned16(y), "%s: x and y must be 16-byte aligned", name);
  const int64_t n_bins = K * PH * PW;
  hipLaunchKernelGGL(roi_align_fwd_kernel, dim3(grid_for(n_bins, 4)), dim3(256), 0, as_stream(stream), x, *d, C, Cs, rois, levels,
                     sc, PH, PW, sampling_ratio, y, n_bins);
  SCAN_LAUNCH_CHECK(name);
  return 0;
}

extern "C" int scan_roi_align_samples(const scan_pyramid_t* d, const float* rois, const int32_t* levels, const float* scales,
                                      int64_t K, int32_t PH, int32_t PW, int32_t sampling_ratio, int32_t gmax, int32_t* grid,
                                      float* pos, float* wgt, int32_t* cell, void* stream) {
  const char* name = "roi_align_samples";
  Scales sc;
  if (check_pool(name, d, 4, 4, rois, scales, K, PH, PW, &sc)) return -1;
  SCAN_CHECK_ARG(sampling_ratio <= GRID_MAX && gmax >= 1 && gmax <= 1024 && K * PH * PW * gmax * gmax < (int64_t)1 << 31,
                 "%s: gmax=%d must be in [1, 1024] and K * PH * PW * gmax^2 below 2^31", name, gmax);
  if (K == 0) return 0;
  SCAN_CHECK_ARG(grid && pos && wgt && cell, "%s: null pointer", name);
  const int64_t n_samples = K * PH * PW * gmax * gmax;
  hipLaunchKernelGGL(roi_align_samples_kernel, dim3(grid_for(n_samples, 256)), dim3(256), 0, as_stream(stream), *d, rois, levels,
                     sc, PH, PW, sampling_ratio, gmax, grid, pos, wgt, cell, n_samples);
  SCAN_LAUNCH_CHECK(name);
  return 0;
}

extern "C" int scan_roi_align_backward(const float* dy, const scan_pyramid_t* d, int32_t C, int32_t Cs, const float* rois,
                                       const int32_t* levels, const float* scales, int64_t K, int32_t PH, int32_t PW,
                                       int32_t sampling_ratio, float* dx, void* stream) {
  const char* name = "roi_align_backward";
  Scales sc;
  if (check_pool(name, d, C, Cs, rois, scales, K, PH, PW, &sc)) return -1;
  SCAN_CHECK_ARG(sampling_ratio <= GRID_MAX, "%s: sampling_ratio=%d must be <= %d", name, sampling_ratio, GRID_MAX);
  SCAN_CHECK_ARG(dx && (dy || K == 0), "%s: null pointer", name);
  SCAN_CHECK_ARG(aligned16(dx) && aligned16(dy), "%s: dy and dx must be 16-byte aligned", name);
  const int64_t M = d->row_off[d->n_levels];
  hipLaunchKernelGGL(roi_align_bwd_kernel, dim3(grid_for(M, 4)), dim3(256), 0, as_stream(stream), dy, *d, C, Cs, rois, levels, sc,
                     K, PH, PW, sampling_ratio, dx, M);
  SCAN_LAUNCH_CHECK(name);
  return 0;
}

extern "C" int scan_roi_pool_forward(const float* x, const scan_pyramid_t* d, int32_t C, int32_t Cs, const float* rois,
                                     const int32_t* levels, const float* scales, int64_t K, int32_t PH, int32_t PW, float* y,
                                     int32_t* argmax, void* stream) {
  const char* name = "roi_pool_forward";
  Scales sc;
  if (check_pool(name, d, C, Cs, rois, scales, K, PH, PW, &sc)) return -1;
  if (K == 0) return 0;
  SCAN_CHECK_ARG(x && y && argmax, "%s: null pointer", name);
  SCAN_CHECK_ARG(aligned16(x) && aligned16(y) && aligned16(argmax), "%s: x, y and argmax must be 16-byte aligned", name);
  const int64_t n_bins = K * PH * PW;
  hipLaunchKernelGGL(roi_pool_fwd_kernel, dim3(grid_for(n_bins, 4)), dim3(256), 0, as_stream(stream), x, *d, C, Cs, rois, levels,
                     sc, PH, PW, y, argmax, n_bins);
  SCAN_LAUNCH_CHECK(name);
  return 0;
}

extern "C" int scan_roi_pool_backward(const float* dy, const int32_t* argmax, const scan_pyramid_t* d, int32_t C, int32_t Cs,
                                      const float* rois, const int32_t* levels, const float* scales, int64_t K, int32_t PH,
                                      int32_t PW, float* dx, void* stream) {
  const char* name = "roi_pool_backward";
  Scales sc;
  if (check_pool(name, d, C, Cs, rois, scales, K, PH, PW, &sc)) return -1;
  SCAN_CHECK_ARG(dx && ((dy && argmax) || K == 0), "%s: null pointer", name);
  SCAN_CHECK_ARG(aligned16(dx) && aligned16(dy) && aligned16(argmax), "%s: dy, argmax and dx must be 16-byte aligned", name);
  const int64_t M = d->row_off[d->n_levels];
  hipLaunchKernelGGL(roi_pool_bwd_kernel, dim3(grid_for(M, 4)), dim3(256), 0, as_stream(stream), dy, argmax, *d, C, Cs, rois,
                     levels, sc, K, PH, PW, dx, M);
  SCAN_LAUNCH_CHECK(name);
  return 0;
}
