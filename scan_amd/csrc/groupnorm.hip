// GroupNorm(32) + ReLU on pyramid activations [M, 256] for gfx950.
// HBM-bound: every kernel streams rows with one float4 per lane (64 lanes x 16 B =
// one 1 KiB row per wave instruction), statistics are accumulated in fp64.
//
// Replaces nn.GroupNorm(32, C) + nn.ReLU in the reference towers
// (rpn/fcos/condgraph.py:99-105, rpn/fcos/fcos.py:36-49,
//  discriminator/fcos_head_discriminator_con.py:31-32).
#include "common.h"

#include <limits.h>
#include <string.h>

#define GN_C 256
#define GN_RPB 256  // rows per block (4 waves x 64 rows, four rows in flight per wave)
#define GN_REP 8    // replicas of the per-channel fp64 sums (block b adds into replica b % 8: 8x fewer adders per address)

// Compact 1-D grid: block -> (level, image, row chunk) through a per-level prefix table, so small levels do not
// launch empty blocks (a 2-D grid sized by the largest level wasted 3 of 4 blocks on a five-level pyramid).
struct GnTab {
  int blk_off[SCAN_MAX_LEVELS + 1];  // first block of each level
  int per_img[SCAN_MAX_LEVELS];      // blocks per image on that level
};
struct GnBlock {
  int64_t row0;  // first pyramid row of this block
  int rows;      // rows in this block
  int il;        // image-level index
  int hw;
  bool first;    // first row chunk of its (level, image)
  int blk0;      // block of that first chunk; the (level, image) owns blocks [blk0, blk0 + nchunk)
  int nchunk;
};
__device__ __forceinline__ GnBlock gn_block(const scan_pyramid_t& d, const GnTab& t) {
  GnBlock b;
  const int lvl = level_of(t.blk_off, d.n_levels, (int)blockIdx.x);
  const int r = blockIdx.x - t.blk_off[lvl];
  const int n = r / t.per_img[lvl], chunk = r - n * t.per_img[lvl];
  b.il = lvl * d.n_images + n;
  b.first = chunk == 0;
  b.blk0 = blockIdx.x - chunk;
  b.nchunk = t.per_img[lvl];
  b.hw = d.h[lvl] * d.w[lvl];
  const int64_t start = (int64_t)chunk * GN_RPB;
  b.rows = (int)((b.hw - start) < GN_RPB ? (b.hw - start) : GN_RPB);
  b.row0 = d.row_off[lvl] + (int64_t)n * b.hw + start;
  return b;
}

// Ordered forms (scan_tune "deterministic", the *_ordered entry points).  ORD = false: the fp64 sums of all row chunks meet
// in one accumulator per (level, image, group) / per channel replica through atomics, so their order -- and with it the last
// bit of the rounded result -- follows the arrival of the blocks.  ORD = true: every block stores its sums to its own slot
// ws[blockIdx.x][...] and the kernel that consumes them adds the slots of a (level, image) in ascending chunk order; blocks are
// numbered level-major / image / chunk, so the workspace is the ragged [level * N + image][chunk][group][2].  Nothing is
// cleared: every block of the grid writes every one of its slots.
template <bool ORD>
__global__ __launch_bounds__(256) void gn_stats_kernel(const float* __restrict__ x, scan_pyramid_t d, GnTab tab, int G,
                                                       double* __restrict__ ws) {
  __shared__ double red[4][32][2];
  const GnBlock b = gn_block(d, tab);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  double s = 0.0, q = 0.0;
  const float* base = x + b.row0 * GN_C + 4 * lane;
  for (int r = wid; r < b.rows; r += 16) {  // rows r, r+4, r+8, r+12 of this wave: four loads in flight
    float4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
      v[u] = (r + 4 * u < b.rows) ? *reinterpret_cast<const float4*>(base + (int64_t)(r + 4 * u) * GN_C)
                                  : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      // every element is widened before it is added or squared: a square rounded to fp32 costs the variance a relative
      // (mean / std)^2 * 2^-24, and overflows from |x| = 1.8e19
      const double x0 = (double)v[u].x, x1 = (double)v[u].y, x2 = (double)v[u].z, x3 = (double)v[u].w;
      s += (x0 + x1) + (x2 + x3);
      q += (x0 * x0 + x1 * x1) + (x2 * x2 + x3 * x3);
    }
  }
  // 8 channels per group = 2 adjacent lanes
  s += __shfl_xor(s, 1, 64);
  q += __shfl_xor(q, 1, 64);
  if ((lane & 1) == 0) {
    red[wid][lane >> 1][0] = s;
    red[wid][lane >> 1][1] = q;
  }
  __syncthreads();
  if (threadIdx.x < 32) {
    const int g = threadIdx.x;
    const double ss = red[0][g][0] + red[1][g][0] + red[2][g][0] + red[3][g][0];
    const double qq = red[0][g][1] + red[1][g][1] + red[2][g][1] + red[3][g][1];
    if (ORD) {
      ws[((int64_t)blockIdx.x * G + g) * 2 + 0] = ss;
      ws[((int64_t)blockIdx.x * G + g) * 2 + 1] = qq;
    } else {
      atomicAdd(&ws[((int64_t)b.il * G + g) * 2 + 0], ss);
      atomicAdd(&ws[((int64_t)b.il * G + g) * 2 + 1], qq);
    }
  }
}

// y before the ReLU.  One fixed operation order (explicit fma) shared by the forward and by the backward kernels,
// which recompute it from x to get the ReLU mask instead of reading y back from HBM.
__device__ __forceinline__ float gn_affine(float v, float mean, float rstd, float ga, float be) {
  return __fmaf_rn((v - mean) * rstd, ga, be);
}

// ORD: ws holds gn_stats_kernel<true>'s per-block sums; tab locates the chunks of each (level, image)
template <bool ORD>
__global__ void gn_stats_final_kernel(const double* __restrict__ ws, scan_pyramid_t d, GnTab tab, int G, float eps,
                                      float* __restrict__ stats) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int total = d.n_levels * d.n_images * G;
  if (i >= total) return;
  const int il = i / G, lvl = il / d.n_images;
  const double cnt = (double)d.h[lvl] * d.w[lvl] * (GN_C / G);
  double s = 0.0, q = 0.0;
  if (ORD) {
    const int g = i - il * G, n = il - lvl * d.n_images;
    const int64_t blk0 = tab.blk_off[lvl] + (int64_t)n * tab.per_img[lvl];
    for (int ch = 0; ch < tab.per_img[lvl]; ++ch) {
      s += ws[((blk0 + ch) * G + g) * 2];
      q += ws[((blk0 + ch) * G + g) * 2 + 1];
    }
  } else {
    s = ws[2 * i];
    q = ws[2 * i + 1];
  }
  const double mean = s / cnt;
  double var = q / cnt - mean * mean;
  if (var < 0) var = 0;
  stats[2 * i] = (float)mean;
  stats[2 * i + 1] = (float)(1.0 / sqrt(var + (double)eps));
}

__device__ __forceinline__ float4 gn_affine4(const float4 v, float mean, float rstd, const float4 ga, const float4 be) {
  float4 o;
  o.x = gn_affine(v.x, mean, rstd, ga.x, be.x);
  o.y = gn_affine(v.y, mean, rstd, ga.y, be.y);
  o.z = gn_affine(v.z, mean, rstd, ga.z, be.z);
  o.w = gn_affine(v.w, mean, rstd, ga.w, be.w);
  return o;
}

// sums != nullptr: (mean, rstd) are derived here from the fp64 (sum, sum of squares) a conv epilogue accumulated -- the
// arithmetic of gn_stats_final_kernel, so the launch of its own goes away -- and the first block of every (level, image)
// writes them to stats_out for the backward pass.
__global__ __launch_bounds__(256) void gn_apply_kernel(const float* __restrict__ x, scan_pyramid_t d, GnTab tab, int G,
                                                       const float* __restrict__ stats,
                                                       const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, int relu,
                                                       float* __restrict__ y, const double* __restrict__ sums,
                                                       float eps, float* __restrict__ stats_out, int ldy) {
  const GnBlock b = gn_block(d, tab);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int g = lane >> 1;
  float mean, rstd;
  if (sums != nullptr) {
    const int64_t i = (int64_t)b.il * G + g;
    const double cnt = (double)b.hw * (GN_C / G);
    const double m = sums[2 * i] / cnt;
    double var = sums[2 * i + 1] / cnt - m * m;
    if (var < 0) var = 0;
    mean = (float)m;
    rstd = (float)(1.0 / sqrt(var + (double)eps));
    if (b.first && wid == 0 && (lane & 1) == 0) {
      stats_out[2 * i] = mean;
      stats_out[2 * i + 1] = rstd;
    }
  } else {
    mean = stats[((int64_t)b.il * G + g) * 2];
    rstd = stats[((int64_t)b.il * G + g) * 2 + 1];
  }
  const float4 ga = *reinterpret_cast<const float4*>(gamma + 4 * lane);
  const float4 be = *reinterpret_cast<const float4*>(beta + 4 * lane);
  const int64_t base = b.row0 * GN_C + 4 * lane;
  for (int r = wid; r < b.rows; r += 16) {
    float4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (r + 4 * u < b.rows) v[u] = *reinterpret_cast<const float4*>(x + base + (int64_t)(r + 4 * u) * GN_C);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (r + 4 * u < b.rows) {
        float4 o = gn_affine4(v[u], mean, rstd, ga, be);
        if (relu) {
          o.x = fmaxf(o.x, 0.f);
          o.y = fmaxf(o.y, 0.f);
          o.z = fmaxf(o.z, 0.f);
          o.w = fmaxf(o.w, 0.f);
        }
        *reinterpret_cast<float4*>(y + (b.row0 + r + 4 * u) * (int64_t)ldy + 4 * lane) = o;
      }
    }
  }
}

// backward pass 1: group sums S1 = sum dyh*gamma, S2 = sum dyh*gamma*xhat; channel sums dgamma, dbeta
__device__ __forceinline__ float4 gn_masked(const float4 xv, float4 gv, float mean, float rstd, const float4 ga,
                                            const float4 be) {
  gv.x = gn_affine(xv.x, mean, rstd, ga.x, be.x) > 0.f ? gv.x : 0.f;
  gv.y = gn_affine(xv.y, mean, rstd, ga.y, be.y) > 0.f ? gv.y : 0.f;
  gv.z = gn_affine(xv.z, mean, rstd, ga.z, be.z) > 0.f ? gv.z : 0.f;
  gv.w = gn_affine(xv.w, mean, rstd, ga.w, be.w) > 0.f ? gv.w : 0.f;
  return gv;
}

template <bool ORD>
__global__ __launch_bounds__(256) void gn_bwd_reduce_kernel(const float* __restrict__ x, const float* __restrict__ beta,
                                                            const float* __restrict__ dy, scan_pyramid_t d, GnTab tab,
                                                            int G, const float* __restrict__ stats,
                                                            const float* __restrict__ gamma, int relu,
                                                            double* __restrict__ ws_g, double* __restrict__ ws_c,
                                                            int lddy) {
  __shared__ double redg[4][32][2];
  __shared__ float redc[4][GN_C][2];
  const GnBlock b = gn_block(d, tab);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int g = lane >> 1;
  const float mean = stats[((int64_t)b.il * G + g) * 2], rstd = stats[((int64_t)b.il * G + g) * 2 + 1];
  const float4 ga = *reinterpret_cast<const float4*>(gamma + 4 * lane);
  const float4 be = relu ? *reinterpret_cast<const float4*>(beta + 4 * lane) : make_float4(0.f, 0.f, 0.f, 0.f);
  double s1 = 0, s2 = 0;
  float dg[4] = {0, 0, 0, 0}, db[4] = {0, 0, 0, 0};
  const int64_t base = b.row0 * GN_C + 4 * lane;
  for (int r = wid; r < b.rows; r += 16) {
    float4 xv[4], gv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const bool ok = r + 4 * u < b.rows;
      const int64_t off = base + (int64_t)(r + 4 * u) * GN_C;
      xv[u] = ok ? *reinterpret_cast<const float4*>(x + off) : make_float4(0.f, 0.f, 0.f, 0.f);
      gv[u] = ok ? *reinterpret_cast<const float4*>(dy + (b.row0 + r + 4 * u) * (int64_t)lddy + 4 * lane)
                 : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float4 gg = relu ? gn_masked(xv[u], gv[u], mean, rstd, ga, be) : gv[u];
      const float h0 = (xv[u].x - mean) * rstd, h1 = (xv[u].y - mean) * rstd, h2 = (xv[u].z - mean) * rstd,
                  h3 = (xv[u].w - mean) * rstd;
      dg[0] += gg.x * h0;
      dg[1] += gg.y * h1;
      dg[2] += gg.z * h2;
      dg[3] += gg.w * h3;
      db[0] += gg.x;
      db[1] += gg.y;
      db[2] += gg.z;
      db[3] += gg.w;
      const float a0 = gg.x * ga.x, a1 = gg.y * ga.y, a2 = gg.z * ga.z, a3 = gg.w * ga.w;
      s1 += (double)((a0 + a1) + (a2 + a3));
      s2 += (double)((a0 * h0 + a1 * h1) + (a2 * h2 + a3 * h3));
    }
  }
  s1 += __shfl_xor(s1, 1, 64);
  s2 += __shfl_xor(s2, 1, 64);
  if ((lane & 1) == 0) {
    redg[wid][g][0] = s1;
    redg[wid][g][1] = s2;
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    redc[wid][4 * lane + e][0] = dg[e];
    redc[wid][4 * lane + e][1] = db[e];
  }
  __syncthreads();
  if (threadIdx.x < 32) {
    const int gg = threadIdx.x;
    const double s1g = redg[0][gg][0] + redg[1][gg][0] + redg[2][gg][0] + redg[3][gg][0];
    const double s2g = redg[0][gg][1] + redg[1][gg][1] + redg[2][gg][1] + redg[3][gg][1];
    if (ORD) {  // ws_g [block][G][2]
      ws_g[((int64_t)blockIdx.x * G + gg) * 2 + 0] = s1g;
      ws_g[((int64_t)blockIdx.x * G + gg) * 2 + 1] = s2g;
    } else {
      atomicAdd(&ws_g[((int64_t)b.il * G + gg) * 2 + 0], s1g);
      atomicAdd(&ws_g[((int64_t)b.il * G + gg) * 2 + 1], s2g);
    }
  }
  const int c = threadIdx.x;  // 256 threads == 256 channels
  const double dgc = ((double)redc[0][c][0] + (double)redc[1][c][0]) + ((double)redc[2][c][0] + (double)redc[3][c][0]);
  const double dbc = ((double)redc[0][c][1] + (double)redc[1][c][1]) + ((double)redc[2][c][1] + (double)redc[3][c][1]);
  if (ORD) {  // ws_c [block][C][2]
    *reinterpret_cast<double2*>(ws_c + ((int64_t)blockIdx.x * GN_C + c) * 2) = make_double2(dgc, dbc);
  } else {
    double* rep = ws_c + (int64_t)(blockIdx.x % GN_REP) * 2 * GN_C;
    atomicAdd(&rep[2 * c + 0], dgc);
    atomicAdd(&rep[2 * c + 1], dbc);
  }
}

template <bool ORD>
__global__ __launch_bounds__(256) void gn_bwd_apply_kernel(const float* __restrict__ x, const float* __restrict__ beta,
                                                           const float* __restrict__ dy, scan_pyramid_t d, GnTab tab,
                                                           int G, const float* __restrict__ stats,
                                                           const float* __restrict__ gamma, int relu,
                                                           const double* __restrict__ ws_g, float* __restrict__ dx,
                                                           const double* __restrict__ ws_c, float* __restrict__ dgamma,
                                                           float* __restrict__ dbeta, int accumulate, int lddy) {
  if (blockIdx.x == 0) {
    // the channel sums are final (the reduce kernel ran before this launch): fold the GN_REP replicas into dgamma /
    // dbeta here instead of in a one-block launch of its own (256 threads == 256 channels)
    const int c = threadIdx.x;
    double sa = 0.0, sb = 0.0;
    if (ORD) {  // every block's slot, ascending
#pragma unroll 8
      for (int r = 0; r < (int)gridDim.x; ++r) {
        const double2 v = *reinterpret_cast<const double2*>(ws_c + ((int64_t)r * GN_C + c) * 2);
        sa += v.x;
        sb += v.y;
      }
    } else {
#pragma unroll
      for (int r = 0; r < GN_REP; ++r) {
        sa += ws_c[(int64_t)r * 2 * GN_C + 2 * c];
        sb += ws_c[(int64_t)r * 2 * GN_C + 2 * c + 1];
      }
    }
    const float a = (float)sa, bb = (float)sb;
    dgamma[c] = accumulate ? dgamma[c] + a : a;
    dbeta[c] = accumulate ? dbeta[c] + bb : bb;
  }
  const GnBlock b = gn_block(d, tab);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int g = lane >> 1;
  const float mean = stats[((int64_t)b.il * G + g) * 2], rstd = stats[((int64_t)b.il * G + g) * 2 + 1];
  const float inv_cnt = 1.0f / ((float)b.hw * (GN_C / G));
  double s1 = 0.0, s2 = 0.0;
  if (ORD) {  // the chunks of this (level, image), ascending
    for (int ch = 0; ch < b.nchunk; ++ch) {
      s1 += ws_g[((int64_t)(b.blk0 + ch) * G + g) * 2];
      s2 += ws_g[((int64_t)(b.blk0 + ch) * G + g) * 2 + 1];
    }
  } else {
    s1 = ws_g[((int64_t)b.il * G + g) * 2];
    s2 = ws_g[((int64_t)b.il * G + g) * 2 + 1];
  }
  const float S1 = (float)s1 * inv_cnt;
  const float S2 = (float)s2 * inv_cnt;
  const float4 ga = *reinterpret_cast<const float4*>(gamma + 4 * lane);
  const float4 be = relu ? *reinterpret_cast<const float4*>(beta + 4 * lane) : make_float4(0.f, 0.f, 0.f, 0.f);
  const int64_t base = b.row0 * GN_C + 4 * lane;
  for (int r = wid; r < b.rows; r += 16) {
    float4 xv[4], gv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (r + 4 * u < b.rows) {
        const int64_t off = base + (int64_t)(r + 4 * u) * GN_C;
        xv[u] = *reinterpret_cast<const float4*>(x + off);
        gv[u] = *reinterpret_cast<const float4*>(dy + (b.row0 + r + 4 * u) * (int64_t)lddy + 4 * lane);
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (r + 4 * u < b.rows) {
        const float4 gg = relu ? gn_masked(xv[u], gv[u], mean, rstd, ga, be) : gv[u];
        float4 o;
        o.x = rstd * (gg.x * ga.x - (S1 + (xv[u].x - mean) * rstd * S2));
        o.y = rstd * (gg.y * ga.y - (S1 + (xv[u].y - mean) * rstd * S2));
        o.z = rstd * (gg.z * ga.z - (S1 + (xv[u].z - mean) * rstd * S2));
        o.w = rstd * (gg.w * ga.w - (S1 + (xv[u].w - mean) * rstd * S2));
        *reinterpret_cast<float4*>(dx + base + (int64_t)(r + 4 * u) * GN_C) = o;
      }
    }
  }
}

static int gn_check(const scan_pyramid_t* d, int C, int G, const char* who) {
  SCAN_CHECK_ARG(d && d->n_levels >= 1 && d->n_levels <= SCAN_MAX_LEVELS, "%s: bad pyramid", who);
  SCAN_CHECK_ARG(C == GN_C && G == 32, "%s: only C=256, G=32 is built (got C=%d G=%d)", who, C, G);
  return 0;
}
static int gn_tab(const scan_pyramid_t* d, GnTab* t) {
  t->blk_off[0] = 0;
  for (int l = 0; l < SCAN_MAX_LEVELS; ++l) {
    if (l < d->n_levels) {
      t->per_img[l] = (d->h[l] * d->w[l] + GN_RPB - 1) / GN_RPB;
      t->blk_off[l + 1] = t->blk_off[l] + d->n_images * t->per_img[l];
    } else {
      t->per_img[l] = 1;
      t->blk_off[l + 1] = t->blk_off[l];
    }
  }
  return t->blk_off[d->n_levels];
}
static int gn_blocks(const scan_pyramid_t* d) {
  GnTab tab;
  return gn_tab(d, &tab);
}

// ld: y (forward) / dy (backward) may be a column slice of a wider row-major matrix -- ldy / lddy = its row stride in floats
// (a multiple of 4, >= C; the slice starts at the pointer).  The CKA discriminators normalise straight into the first 256
// columns of the [M, 256 + Cf] class-branch input and take the gradient back from the same columns of its data gradient:
// no concatenation copy forward, no contiguous() copy backward.
static int gn_ld_check(int ld, int C, const char* who) {
  SCAN_CHECK_ARG(ld >= C && ld % 4 == 0, "%s: row stride %d must be a multiple of 4 and >= C", who, ld);
  return 0;
}

// ---- the workspace, stated once.  fp64 values; the backward's need (the statistics use the first part only).
// atomic:  [level * N + image][G][2] group sums + [GN_REP][C][2] channel-sum replicas, cleared before the launch
// ordered: [block][G][2] + [block][C][2], a slot per block of the grid, never cleared
static int64_t gn_ws_doubles(const scan_pyramid_t* d, int C, int G, bool ordered) {
  const int64_t nblk = gn_blocks(d);
  return ordered ? nblk * G * 2 + nblk * C * 2 : (int64_t)d->n_levels * d->n_images * G * 2 + (int64_t)C * 2 * GN_REP;
}
extern "C" int64_t scan_groupnorm_ws_floats(const scan_pyramid_t* d, int32_t C, int32_t G) {
  return 2 * gn_ws_doubles(d, C, G, false);
}
extern "C" int64_t scan_groupnorm_ordered_ws_floats(const scan_pyramid_t* d, int32_t C, int32_t G) {
  return 2 * gn_ws_doubles(d, C, G, true);
}

// ---- the launches.  The entry points below are argument checks around these helpers.
// statistics pair: the chunk sums of x into ws (atomic: cleared here first), then (mean, rstd) into stats
template <bool ORD>
static int gn_launch_stats(const float* x, const scan_pyramid_t* d, int G, float eps, float* stats, float* ws, hipStream_t st) {
  double* wsd = reinterpret_cast<double*>(ws);
  const int total = d->n_levels * d->n_images * G;
  if (!ORD && hipMemsetAsync(wsd, 0, sizeof(double) * 2 * total, st) != hipSuccess) {
    scan_set_error("groupnorm_stats: memset failed");
    return -2;
  }
  GnTab tab;
  const int nblk = gn_tab(d, &tab);
  if (!ORD || nblk > 0) {
    hipLaunchKernelGGL(gn_stats_kernel<ORD>, dim3(nblk), dim3(256), 0, st, x, *d, tab, G, wsd);
    SCAN_LAUNCH_CHECK(ORD ? "gn_stats_ordered" : "gn_stats");
  }
  hipLaunchKernelGGL(gn_stats_final_kernel<ORD>, dim3((total + 255) / 256), dim3(256), 0, st, wsd, *d, tab, G, eps, stats);
  SCAN_LAUNCH_CHECK(ORD ? "gn_stats_final_ordered" : "gn_stats_final");
  return 0;
}

// normalise (+ ReLU).  sums == nullptr: stats_in is read.  Otherwise the kernel finalises the sums itself and writes stats_out
// for the backward pass: scan_groupnorm_stats_from_sums + scan_groupnorm_relu_forward in one launch.
static int gn_launch_apply(const float* x, const scan_pyramid_t* d, int G, const float* stats_in, const float* gamma, const float* beta,
                           int relu, float* y, int ldy, const float* sums, float eps, float* stats_out, hipStream_t st) {
  GnTab tab;
  const int nblk = gn_tab(d, &tab);
  hipLaunchKernelGGL(gn_apply_kernel, dim3(nblk), dim3(256), 0, st, x, *d, tab, G, stats_in, gamma, beta, relu, y,
                     reinterpret_cast<const double*>(sums), eps, stats_out, ldy);
  SCAN_LAUNCH_CHECK(sums ? "gn_apply_from_sums" : "gn_apply");
  return 0;
}

// backward pair: group / channel sums into ws (atomic: cleared here first unless it arrives cleared), then dx, dgamma, dbeta
template <bool ORD>
static int gn_launch_backward(const float* x, const float* beta, const float* dy, int lddy, const scan_pyramid_t* d, int C, int G,
                              const float* stats, const float* gamma, int relu, float* dx, float* dgamma, float* dbeta, int accumulate,
                              float* ws, bool cleared, hipStream_t st) {
  GnTab tab;
  const int nblk = gn_tab(d, &tab);
  double* ws_g = reinterpret_cast<double*>(ws);
  const int64_t ng = (ORD ? (int64_t)nblk : (int64_t)d->n_levels * d->n_images) * G * 2;
  double* ws_c = ws_g + ng;
  if (!ORD && !cleared && hipMemsetAsync(ws_g, 0, sizeof(double) * (ng + 2 * C * GN_REP), st) != hipSuccess) {
    scan_set_error("groupnorm_relu_backward: memset failed");
    return -2;
  }
  hipLaunchKernelGGL(gn_bwd_reduce_kernel<ORD>, dim3(nblk), dim3(256), 0, st, x, beta, dy, *d, tab, G, stats, gamma, relu, ws_g, ws_c,
                     lddy);
  SCAN_LAUNCH_CHECK(ORD ? "gn_bwd_reduce_ordered" : "gn_bwd_reduce");
  hipLaunchKernelGGL(gn_bwd_apply_kernel<ORD>, dim3(nblk), dim3(256), 0, st, x, beta, dy, *d, tab, G, stats, gamma, relu, ws_g, dx, ws_c,
                     dgamma, dbeta, accumulate, lddy);
  SCAN_LAUNCH_CHECK(ORD ? "gn_bwd_apply_ordered" : "gn_bwd_apply");
  return 0;
}

// ---- the older entry points: single steps for callers that choose themselves (tools/pointwise_roofline.py times them)
extern "C" int scan_groupnorm_stats(const float* x, const scan_pyramid_t* d, int32_t C, int32_t G, float eps, float* stats,
                                    float* ws, void* stream) {
  if (gn_check(d, C, G, "groupnorm_stats")) return -1;
  SCAN_CHECK_ARG(x && stats && ws, "groupnorm_stats: null pointer");
  return gn_launch_stats<false>(x, d, G, eps, stats, ws, as_stream(stream));
}

// (mean, rstd) from sums accumulated elsewhere (scan_conv3x3_gn_bf16x3's epilogue): ws = fp64 [n_levels*N*G][2]
extern "C" int scan_groupnorm_stats_from_sums(const float* ws, const scan_pyramid_t* d, int32_t C, int32_t G, float eps,
                                              float* stats, void* stream) {
  if (gn_check(d, C, G, "groupnorm_stats_from_sums")) return -1;
  SCAN_CHECK_ARG(ws && stats, "groupnorm_stats_from_sums: null pointer");
  const int total = d->n_levels * d->n_images * G;
  GnTab tab;
  gn_tab(d, &tab);
  hipLaunchKernelGGL(gn_stats_final_kernel<false>, dim3((total + 255) / 256), dim3(256), 0, as_stream(stream),
                     reinterpret_cast<const double*>(ws), *d, tab, G, eps, stats);
  SCAN_LAUNCH_CHECK("gn_stats_final");
  return 0;
}

extern "C" int scan_groupnorm_relu_forward_ld(const float* x, const scan_pyramid_t* d, int32_t C, int32_t G,
                                              const float* stats, const float* gamma, const float* beta, int32_t relu,
                                              float* y, int32_t ldy, void* stream) {
  if (gn_check(d, C, G, "groupnorm_relu_forward") || gn_ld_check(ldy, C, "groupnorm_relu_forward")) return -1;
  SCAN_CHECK_ARG(x && stats && gamma && beta && y, "groupnorm_relu_forward: null pointer");
  return gn_launch_apply(x, d, G, stats, gamma, beta, relu, y, ldy, nullptr, 0.f, nullptr, as_stream(stream));
}

extern "C" int scan_groupnorm_relu_forward(const float* x, const scan_pyramid_t* d, int32_t C, int32_t G,
                                           const float* stats, const float* gamma, const float* beta, int32_t relu,
                                           float* y, void* stream) {
  return scan_groupnorm_relu_forward_ld(x, d, C, G, stats, gamma, beta, relu, y, C, stream);
}

extern "C" int scan_groupnorm_relu_forward_from_sums_ld(const float* x, const scan_pyramid_t* d, int32_t C, int32_t G,
                                                        const float* sums, float eps, const float* gamma,
                                                        const float* beta, int32_t relu, float* y, int32_t ldy,
                                                        float* stats, void* stream) {
  if (gn_check(d, C, G, "groupnorm_relu_forward_from_sums") || gn_ld_check(ldy, C, "groupnorm_relu_forward_from_sums"))
    return -1;
  SCAN_CHECK_ARG(x && sums && stats && gamma && beta && y, "groupnorm_relu_forward_from_sums: null pointer");
  return gn_launch_apply(x, d, G, nullptr, gamma, beta, relu, y, ldy, sums, eps, stats, as_stream(stream));
}

extern "C" int scan_groupnorm_relu_forward_from_sums(const float* x, const scan_pyramid_t* d, int32_t C, int32_t G,
                                                     const float* sums, float eps, const float* gamma,
                                                     const float* beta, int32_t relu, float* y, float* stats,
                                                     void* stream) {
  return scan_groupnorm_relu_forward_from_sums_ld(x, d, C, G, sums, eps, gamma, beta, relu, y, C, stats, stream);
}

// what every backward entry point checks, under its own name
static int gn_bwd_check(const char* who, const scan_pyramid_t* d, int C, int G, int lddy, bool pointers) {
  if (gn_check(d, C, G, who) || gn_ld_check(lddy, C, who)) return -1;
  SCAN_CHECK_ARG(pointers, "%s: null pointer", who);
  return 0;
}
#define GN_BWD_POINTERS (x && dy && stats && gamma && dx && dgamma && dbeta && ws && (beta || !relu))

// accumulate bit 1: ws arrives cleared (a slice of the caller's once-per-iteration cleared buffer)
extern "C" int scan_groupnorm_relu_backward_ld(const float* x, const float* beta, const float* dy, int32_t lddy,
                                               const scan_pyramid_t* d, int32_t C, int32_t G, const float* stats,
                                               const float* gamma, int32_t relu, float* dx, float* dgamma, float* dbeta,
                                               int32_t accumulate, float* ws, void* stream) {
  if (gn_bwd_check("groupnorm_relu_backward", d, C, G, lddy, GN_BWD_POINTERS)) return -1;
  return gn_launch_backward<false>(x, beta, dy, lddy, d, C, G, stats, gamma, relu, dx, dgamma, dbeta, accumulate & 1, ws,
                                   (accumulate & 2) != 0, as_stream(stream));
}

extern "C" int scan_groupnorm_relu_backward(const float* x, const float* beta, const float* dy, const scan_pyramid_t* d,
                                            int32_t C, int32_t G, const float* stats, const float* gamma, int32_t relu,
                                            float* dx, float* dgamma, float* dbeta, int32_t accumulate, float* ws,
                                            void* stream) {
  return scan_groupnorm_relu_backward_ld(x, beta, dy, C, d, C, G, stats, gamma, relu, dx, dgamma, dbeta, accumulate, ws,
                                         stream);
}

extern "C" int scan_groupnorm_stats_ordered(const float* x, const scan_pyramid_t* d, int32_t C, int32_t G, float eps,
                                            float* stats, float* ws, void* stream) {
  if (gn_check(d, C, G, "groupnorm_stats_ordered")) return -1;
  SCAN_CHECK_ARG(x && stats && ws, "groupnorm_stats_ordered: null pointer");
  return gn_launch_stats<true>(x, d, G, eps, stats, ws, as_stream(stream));
}

extern "C" int scan_groupnorm_relu_backward_ld_ordered(const float* x, const float* beta, const float* dy, int32_t lddy,
                                                       const scan_pyramid_t* d, int32_t C, int32_t G, const float* stats,
                                                       const float* gamma, int32_t relu, float* dx, float* dgamma,
                                                       float* dbeta, int32_t accumulate, float* ws, void* stream) {
  if (gn_bwd_check("groupnorm_relu_backward_ordered", d, C, G, lddy, GN_BWD_POINTERS)) return -1;
  SCAN_CHECK_ARG(gn_blocks(d) > 0, "groupnorm_relu_backward_ordered: empty pyramid");
  return gn_launch_backward<true>(x, beta, dy, lddy, d, C, G, stats, gamma, relu, dx, dgamma, dbeta, accumulate & 1, ws, false,
                                  as_stream(stream));
}

extern "C" int scan_groupnorm_relu_backward_ordered(const float* x, const float* beta, const float* dy,
                                                    const scan_pyramid_t* d, int32_t C, int32_t G, const float* stats,
                                                    const float* gamma, int32_t relu, float* dx, float* dgamma, float* dbeta,
                                                    int32_t accumulate, float* ws, void* stream) {
  return scan_groupnorm_relu_backward_ld_ordered(x, beta, dy, C, d, C, G, stats, gamma, relu, dx, dgamma, dbeta, accumulate, ws,
                                                 stream);
}

// ---- plan + run (scan_hip.h): which statistics, which reduction and how much workspace, decided once for every binding
static int gn_plan_fill(const char* who, const scan_pyramid_t* d, int C, int G, int ordered, int source, scan_groupnorm_plan_t* p) {
  if (gn_check(d, C, G, who)) return -1;
  const int64_t nblk = d->n_images >= 1 ? gn_blocks(d) : 0, ws = gn_ws_doubles(d, C, G, ordered != 0);
  SCAN_CHECK_ARG(nblk > 0 && ws <= INT32_MAX, "%s: empty pyramid or workspace past 2^31 doubles", who);
  *p = scan_groupnorm_plan_t{C, G, d->n_levels, d->n_images, (int32_t)nblk, ordered, source, d->n_levels * d->n_images * G * 2, (int32_t)ws,
                             (int32_t)ws};
  return 0;
}

extern "C" int scan_groupnorm_plan(const scan_pyramid_t* d, int32_t C, int32_t G, int32_t flags, scan_groupnorm_plan_t* plan) {
  const char* who = "groupnorm_plan";
  SCAN_CHECK_ARG(plan != nullptr, "%s: null plan", who);
  SCAN_CHECK_ARG(flags == 0 || flags == SCAN_GN_SUMS || flags == (SCAN_GN_SUMS | SCAN_GN_SEPARATE_FINAL), "%s: flags=%d", who, flags);
  // the one reader of the knob.  Epilogue sums are atomic: deterministic mode takes none, also not those of a conv that ran
  // before the mode was switched on, and reads x once more with the ordered statistics kernel.
  const int ordered = scan_tune_get("deterministic") == 1;
  const int source = ordered || !(flags & SCAN_GN_SUMS) ? SCAN_GN_FROM_X
                     : (flags & SCAN_GN_SEPARATE_FINAL) ? SCAN_GN_FROM_SUMS_FINAL : SCAN_GN_FROM_SUMS;
  return gn_plan_fill(who, d, C, G, ordered, source, plan);
}

// the plan's shape fields re-derived on the pyramid passed in: a zeroed or edited plan, or one made for another pyramid, differs
static int gn_plan_check(const char* who, const scan_groupnorm_plan_t* p, const scan_pyramid_t* d, int ld) {
  SCAN_CHECK_ARG(p != nullptr, "%s: null plan", who);
  scan_groupnorm_plan_t q;
  SCAN_CHECK_ARG(p->C == GN_C && p->G == 32 && (p->ordered == 0 || p->ordered == 1) && p->source >= SCAN_GN_FROM_X &&
                     p->source <= SCAN_GN_FROM_SUMS_FINAL && (!p->ordered || p->source == SCAN_GN_FROM_X),
                 "%s: not a plan scan_groupnorm_plan filled", who);
  if (gn_plan_fill(who, d, p->C, p->G, p->ordered, p->source, &q)) return -1;
  SCAN_CHECK_ARG(memcmp(&q, p, sizeof q) == 0, "%s: not a plan scan_groupnorm_plan filled for this pyramid (blocks: planned %d, here %d)", who,
                 p->blocks, q.blocks);
  return gn_ld_check(ld, p->C, who);
}

extern "C" int scan_groupnorm_run_forward(const scan_groupnorm_plan_t* plan, const float* x, const scan_pyramid_t* d, const float* sums,
                                          float eps, const float* gamma, const float* beta, int32_t relu, float* y, int32_t ldy,
                                          float* stats, float* ws, void* stream) {
  const char* who = "groupnorm_run_forward";
  if (gn_plan_check(who, plan, d, ldy)) return -1;
  const int src = plan->source, G = plan->G;
  SCAN_CHECK_ARG(x && gamma && beta && y && stats && (src == SCAN_GN_FROM_X ? ws != nullptr : sums != nullptr), "%s: null pointer", who);
  hipStream_t st = as_stream(stream);
  const int rc = src == SCAN_GN_FROM_SUMS         ? 0
                 : src == SCAN_GN_FROM_SUMS_FINAL ? scan_groupnorm_stats_from_sums(sums, d, plan->C, G, eps, stats, stream)
                 : plan->ordered                  ? gn_launch_stats<true>(x, d, G, eps, stats, ws, st)
                                                  : gn_launch_stats<false>(x, d, G, eps, stats, ws, st);
  if (rc) return rc;
  return src == SCAN_GN_FROM_SUMS ? gn_launch_apply(x, d, G, nullptr, gamma, beta, relu, y, ldy, sums, eps, stats, st)
                                  : gn_launch_apply(x, d, G, stats, gamma, beta, relu, y, ldy, nullptr, 0.f, nullptr, st);
}

extern "C" int scan_groupnorm_run_backward(const scan_groupnorm_plan_t* plan, const float* x, const float* beta, const float* dy,
                                           int32_t lddy, const scan_pyramid_t* d, const float* stats, const float* gamma, int32_t relu,
                                           float* dx, float* dgamma, float* dbeta, int32_t accumulate, float* ws, int32_t ws_cleared,
                                           void* stream) {
  const char* who = "groupnorm_run_backward";
  if (gn_plan_check(who, plan, d, lddy)) return -1;
  SCAN_CHECK_ARG(accumulate == 0 || accumulate == 1, "%s: accumulate=%d (0 or 1; a cleared workspace is ws_cleared)", who, accumulate);
  SCAN_CHECK_ARG(GN_BWD_POINTERS, "%s: null pointer", who);
  auto run = plan->ordered ? gn_launch_backward<true> : gn_launch_backward<false>;
  return run(x, beta, dy, lddy, d, plan->C, plan->G, stats, gamma, relu, dx, dgamma, dbeta, accumulate, ws, ws_cleared != 0, as_stream(stream));
}
