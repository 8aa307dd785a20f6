// Deformable convolution v2 (DCNv2), the memory-bound half: bilinear sampling of the nine taps into a row matrix
// cols [M, 9 * Cs], the gradients of that sampling, and the data gradient as a per-destination sum (include/scan_hip.h has the
// definition).  The contraction is not here: y = conv1x1(cols) on the library's 1x1 kernels, so the op takes whatever
// arithmetic ops.CONV_MODE selects and this file holds no MFMA.
//
// One wave works on one (row, tap): the two offsets and the mask value are wave-uniform, the four corner rows of x and the
// row of cols are contiguous channel runs that the lanes cover with float4 accesses (lane * 4, then steps of 256 channels).
// Positions are formed with ONE fp32 add of an exactly representable integer and the offset; whether a tap is skipped is
// decided on those floats before anything is converted to an integer, so offsets of any magnitude (and NaN: skipped) are
// safe -- a live tap has floor(h) in [-1, H - 1].
//
// No float atomics.  The data gradient is a sum over arbitrary source rows; the backward writes, per (row, tap, corner), the
// destination row (or M: nothing) and the weight, the caller sorts those keys (stable), and deform_dx_gather gives each row
// of dx to one wave that adds its contributions in sorted order: bit-reproducible, so the op needs no *_ordered twin.  The
// channel sums behind doff / dmask stay inside one wave (per-lane partial sums in channel order, then the shuffle tree).
#include "common.h"

namespace {

constexpr int TAPS = 9;

struct Cell {
  bool live;       // false: the tap is outside (val = 0, no gradient)
  float lh, lw;    // h - floor(h), w - floor(w)
  int64_t row[4];  // pyramid row of corner q = 2 * (h high) + (w high); -1: outside the image
};

__device__ __forceinline__ Cell locate(const scan_pyramid_t& d, int64_t m, int k, float oy, float ox) {
  const RowCoord rc = decode_row(d, m);
  const int H = d.h[rc.lvl], W = d.w[rc.lvl];
  const int i = k / 3, j = k - 3 * i;
  const float h = (float)(rc.y - 1 + i) + oy;
  const float w = (float)(rc.x - 1 + j) + ox;
  Cell c;
  c.live = h > -1.f && w > -1.f && h < (float)H && w < (float)W;  // !(h <= -1 || w <= -1 || h >= H || w >= W), NaN: skipped
  c.lh = c.lw = 0.f;
  c.row[0] = c.row[1] = c.row[2] = c.row[3] = -1;
  if (!c.live) return c;
  const float fh = floorf(h), fw = floorf(w);
  c.lh = h - fh;
  c.lw = w - fw;
  const int h0 = (int)fh, w0 = (int)fw;
  const int64_t base = d.row_off[rc.lvl] + (int64_t)rc.n * H * W;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int hh = h0 + (q >> 1), ww = w0 + (q & 1);
    if (hh >= 0 && hh < H && ww >= 0 && ww < W) c.row[q] = base + (int64_t)hh * W + ww;
  }
  return c;
}

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
// components at channels >= C are padding
__device__ __forceinline__ float4 keep_below(float4 v, int c4, int C) {
  if (c4 + 0 >= C) v.x = 0.f;
  if (c4 + 1 >= C) v.y = 0.f;
  if (c4 + 2 >= C) v.z = 0.f;
  if (c4 + 3 >= C) v.w = 0.f;
  return v;
}

__global__ __launch_bounds__(256) void deform_sample_fwd_kernel(const float* __restrict__ x, scan_pyramid_t d, int C, int Cs,
                                                                const float* __restrict__ off, int ld_off,
                                                                const float* __restrict__ mask, int ld_mask,
                                                                float* __restrict__ cols, int64_t n_taps) {
  const int lane = threadIdx.x & 63;
  const int64_t step = (int64_t)gridDim.x * 4;
  for (int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); t < n_taps; t += step) {
    const int64_t m = t / TAPS;
    const int k = (int)(t - m * TAPS);
    const float oy = off[m * ld_off + 2 * k], ox = off[m * ld_off + 2 * k + 1];
    const float mv = mask ? mask[m * ld_mask + k] : 1.f;
    const Cell c = locate(d, m, k, oy, ox);
    const float wq[4] = {(1.f - c.lh) * (1.f - c.lw), (1.f - c.lh) * c.lw, c.lh * (1.f - c.lw), c.lh * c.lw};
    float* __restrict__ dst = cols + t * Cs;
    for (int c4 = lane * 4; c4 < Cs; c4 += 256) {
      float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (c.row[q] < 0) continue;
        const float4 v = ld4(x + c.row[q] * Cs + c4);
        a.x += wq[q] * v.x, a.y += wq[q] * v.y, a.z += wq[q] * v.z, a.w += wq[q] * v.w;
      }
      a.x *= mv, a.y *= mv, a.z *= mv, a.w *= mv;
      *reinterpret_cast<float4*>(dst + c4) = keep_below(a, c4, C);
    }
  }
}

__global__ __launch_bounds__(256) void deform_sample_bwd_kernel(const float* __restrict__ x, scan_pyramid_t d, int C, int Cs,
                                                                const float* __restrict__ dcols, const float* __restrict__ off,
                                                                int ld_off, const float* __restrict__ mask, int ld_mask,
                                                                float* __restrict__ doff, int ld_doff, float* __restrict__ dmask,
                                                                int ld_dmask, int32_t* __restrict__ keys, float* __restrict__ wgts,
                                                                int64_t n_taps, int32_t M) {
  const int lane = threadIdx.x & 63;
  const int64_t step = (int64_t)gridDim.x * 4;
  for (int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); t < n_taps; t += step) {
    const int64_t m = t / TAPS;
    const int k = (int)(t - m * TAPS);
    const float oy = off[m * ld_off + 2 * k], ox = off[m * ld_off + 2 * k + 1];
    const float mv = mask ? mask[m * ld_mask + k] : 1.f;
    const Cell c = locate(d, m, k, oy, ox);
    const float wq[4] = {(1.f - c.lh) * (1.f - c.lw), (1.f - c.lh) * c.lw, c.lh * (1.f - c.lw), c.lh * c.lw};
    float gm = 0.f, gy = 0.f, gx = 0.f;  // sums over channels of dcols * (val, d val / dh, d val / dw)
    if (c.live) {
      const float* __restrict__ g = dcols + t * Cs;
      for (int c4 = lane * 4; c4 < Cs; c4 += 256) {
        const float4 gv = keep_below(ld4(g + c4), c4, C);
        float4 v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = c.row[q] >= 0 ? ld4(x + c.row[q] * Cs + c4) : make_float4(0.f, 0.f, 0.f, 0.f);
        const float gg[4] = {gv.x, gv.y, gv.z, gv.w};
        const float vv[4][4] = {{v[0].x, v[0].y, v[0].z, v[0].w}, {v[1].x, v[1].y, v[1].z, v[1].w},
                                {v[2].x, v[2].y, v[2].z, v[2].w}, {v[3].x, v[3].y, v[3].z, v[3].w}};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float val = wq[0] * vv[0][e] + wq[1] * vv[1][e] + wq[2] * vv[2][e] + wq[3] * vv[3][e];
          const float dh = (1.f - c.lw) * (vv[2][e] - vv[0][e]) + c.lw * (vv[3][e] - vv[1][e]);
          const float dw = (1.f - c.lh) * (vv[1][e] - vv[0][e]) + c.lh * (vv[3][e] - vv[2][e]);
          gm += gg[e] * val, gy += gg[e] * dh, gx += gg[e] * dw;
        }
      }
    }
    gm = wave_sum(gm), gy = wave_sum(gy), gx = wave_sum(gx);
    if (lane == 0) {
      doff[m * ld_doff + 2 * k] = mv * gy;
      doff[m * ld_doff + 2 * k + 1] = mv * gx;
      if (dmask) dmask[m * ld_dmask + k] = gm;
    }
    if (lane < 4) {
      const int64_t r = lane == 0 ? c.row[0] : lane == 1 ? c.row[1] : lane == 2 ? c.row[2] : c.row[3];
      const float wt = lane == 0 ? wq[0] : lane == 1 ? wq[1] : lane == 2 ? wq[2] : wq[3];
      keys[t * 4 + lane] = r >= 0 ? (int32_t)r : M;
      wgts[t * 4 + lane] = r >= 0 ? mv * wt : 0.f;
    }
    if (k == 0) {  // the row's columns past the 18 offsets / 9 mask values, up to the pitch
      for (int col = 2 * TAPS + lane; col < ld_doff; col += 64) doff[m * ld_doff + col] = 0.f;
      if (dmask)
        for (int col = TAPS + lane; col < ld_dmask; col += 64) dmask[m * ld_dmask + col] = 0.f;
    }
  }
}

__global__ __launch_bounds__(256) void deform_dx_gather_kernel(const float* __restrict__ dcols, const int64_t* __restrict__ perm,
                                                               const int64_t* __restrict__ seg_start,
                                                               const float* __restrict__ wgts, int64_t M, int C, int Cs,
                                                               float* __restrict__ dx) {
  const int lane = threadIdx.x & 63;
  const int64_t step = (int64_t)gridDim.x * 4;
  const int64_t n_entries = 4 * TAPS * M;
  for (int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); p < M; p += step) {
    int64_t e0 = seg_start[p], e1 = seg_start[p + 1];
    if (e0 < 0) e0 = 0;
    if (e1 > n_entries) e1 = n_entries;
    for (int c4 = lane * 4; c4 < Cs; c4 += 256) {
      float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int64_t s = e0; s < e1; ++s) {
        const int64_t e = perm[s];
        if ((uint64_t)e >= (uint64_t)n_entries) continue;  // not a permutation of the entries: nothing is read
        const float wt = wgts[e];
        const float4 v = ld4(dcols + (e >> 2) * Cs + c4);
        a.x += wt * v.x, a.y += wt * v.y, a.z += wt * v.z, a.w += wt * v.w;
      }
      *reinterpret_cast<float4*>(dx + p * Cs + c4) = keep_below(a, c4, C);
    }
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// the pyramid the kernels index x with: every level non-empty and row_off the running sum of n_images * h * w
int check_pyramid(const char* name, const scan_pyramid_t* d) {
  SCAN_CHECK_ARG(d && d->n_levels >= 1 && d->n_levels <= SCAN_MAX_LEVELS && d->n_images >= 1 && d->row_off[0] == 0,
                 "%s: bad pyramid", name);
  for (int l = 0; l < d->n_levels; ++l)
    SCAN_CHECK_ARG(d->h[l] >= 1 && d->w[l] >= 1 && d->row_off[l + 1] - d->row_off[l] == (int64_t)d->n_images * d->h[l] * d->w[l],
                   "%s: bad pyramid (level %d)", name, l);
  return 0;
}
int check_channels(const char* name, int32_t C, int32_t Cs) {
  SCAN_CHECK_ARG(Cs > 0 && Cs % 4 == 0, "%s: Cs=%d must be a positive multiple of 4", name, Cs);
  SCAN_CHECK_ARG(C >= 1 && C <= Cs, "%s: C=%d must be in [1, Cs=%d]", name, C, Cs);
  return 0;
}
// keys and entry indices are int32
int check_rows(const char* name, int64_t M) {
  SCAN_CHECK_ARG(M >= 1 && 4 * TAPS * M < (int64_t)1 << 31, "%s: M=%lld rows, 36 * M must stay below 2^31", name, (long long)M);
  return 0;
}
int check_sample(const char* name, const scan_pyramid_t* d, int32_t C, int32_t Cs, int32_t ld_off, int32_t ld_mask) {
  if (check_channels(name, C, Cs)) return -1;
  SCAN_CHECK_ARG(ld_off >= 2 * TAPS, "%s: ld_off=%d must be >= 18", name, ld_off);
  SCAN_CHECK_ARG(ld_mask >= TAPS, "%s: ld_mask=%d must be >= 9", name, ld_mask);
  if (check_pyramid(name, d)) return -1;
  return check_rows(name, d->row_off[d->n_levels]);
}

}  // namespace

extern "C" int scan_deform_sample_forward(const float* x, const scan_pyramid_t* d, int32_t C, int32_t Cs, const float* off,
                                          int32_t ld_off, const float* mask, int32_t ld_mask, float* cols, void* stream) {
  const char* name = "deform_sample_forward";
  SCAN_CHECK_ARG(x && d && off && cols, "%s: null pointer", name);
  if (check_sample(name, d, C, Cs, ld_off, mask ? ld_mask : TAPS)) return -1;
  SCAN_CHECK_ARG(aligned16(x) && aligned16(cols), "%s: x and cols must be 16-byte aligned", name);
  const int64_t n_taps = TAPS * d->row_off[d->n_levels];
  hipLaunchKernelGGL(deform_sample_fwd_kernel, dim3(grid_for(n_taps, 4)), dim3(256), 0, as_stream(stream), x, *d, C, Cs, off,
                     ld_off, mask, ld_mask, cols, n_taps);
  SCAN_LAUNCH_CHECK(name);
  return 0;
}

extern "C" int scan_deform_sample_backward(const float* x, const scan_pyramid_t* d, int32_t C, int32_t Cs, const float* dcols,
                                           const float* off, int32_t ld_off, const float* mask, int32_t ld_mask, float* doff,
                                           int32_t ld_doff, float* dmask, int32_t ld_dmask, int32_t* keys, float* wgts,
                                           void* stream) {
  const char* name = "deform_sample_backward";
  SCAN_CHECK_ARG(x && d && dcols && off && doff && keys && wgts && (!mask || dmask), "%s: null pointer", name);
  if (check_sample(name, d, C, Cs, ld_off, mask ? ld_mask : TAPS)) return -1;
  SCAN_CHECK_ARG(ld_doff >= 2 * TAPS && (!mask || ld_dmask >= TAPS), "%s: ld_doff=%d must be >= 18 and ld_dmask=%d >= 9", name,
                 ld_doff, ld_dmask);
  SCAN_CHECK_ARG(aligned16(x) && aligned16(dcols), "%s: x and dcols must be 16-byte aligned", name);
  const int64_t M = d->row_off[d->n_levels], n_taps = TAPS * M;
  hipLaunchKernelGGL(deform_sample_bwd_kernel, dim3(grid_for(n_taps, 4)), dim3(256), 0, as_stream(stream), x, *d, C, Cs, dcols,
                     off, ld_off, mask, ld_mask, doff, ld_doff, mask ? dmask : nullptr, ld_dmask, keys, wgts, n_taps, (int32_t)M);
  SCAN_LAUNCH_CHECK(name);
  return 0;
}

extern "C" int scan_deform_dx_gather(const float* dcols, const int64_t* perm, const int64_t* seg_start, const float* wgts, int64_t M,
                                     int32_t C, int32_t Cs, float* dx, void* stream) {
  const char* name = "deform_dx_gather";
  SCAN_CHECK_ARG(dcols && perm && seg_start && wgts && dx, "%s: null pointer", name);
  if (check_channels(name, C, Cs) || check_rows(name, M)) return -1;
  SCAN_CHECK_ARG(aligned16(dcols) && aligned16(dx), "%s: dcols and dx must be 16-byte aligned", name);
  hipLaunchKernelGGL(deform_dx_gather_kernel, dim3(grid_for(M, 4)), dim3(256), 0, as_stream(stream), dcols, perm, seg_start, wgts,
                     M, C, Cs, dx);
  SCAN_LAUNCH_CHECK(name);
  return 0;
}
