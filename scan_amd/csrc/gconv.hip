// Grouped 3x3 convolution "G groups of 128 channels -> one output channel per group" on pyramid rows.
//
// The CKA discriminator ends, per foreground class c, in conv3x3(128 -> 1) on that class's 128 hidden channels
// (reference modeling/discriminator/fcos_head_discriminator_con.py:44-62,104-121).  Stacked over the classes this is a
// conv [M, G*128] -> [M, G] with a block-diagonal weight: on the dense MFMA kernel it costs 64x the useful
// multiply-adds (G of G*G blocks are non-zero, and the narrowest tile is 64 output channels wide for 8 live ones:
// 0.67 ms forward at P3).  The useful work is one multiply-add per input element and tap -- 1.2 GMAC at P3 against
// 537 MB of input -- so these kernels are plain fp32 FMA code bound by HBM:
//
//   forward   (a) per input pixel q and group g the nine tap products T[q][g][t] = <h[q, g*128 ..], w[g][t][..]>
//                 (one 16-byte load per lane, 32-lane butterfly sums), (b) y[p][g] = bias[g] + sum_t T[p + off(t)][g][t]
//                 over the in-bounds taps -- h is read exactly once, T is 9 floats per (pixel, group)
//   dgrad     dh[q, c] = (h[q, c] > 0) * sum_t dy[q - off(t)][g] * w[g][t][c]      (reads h only for the mask)
//   wgrad     dw[g][t][c] = sum_q h[q, c] * dy[q - off(t)][g]: register accumulators over a row chunk per workgroup,
//             per-workgroup partials in a slab, fixed-order reduction (deterministic)
//
// Weight layout: the stacked conv weight [G][9][G*128] (scan_cka_stack_weights' w2): only the diagonal blocks
// w[g][t][g*128 + i] are read / written.
//
// Structure.  The tap-sum pass has ONE loop body (taps_body) that works on a LaneMap: the group, the channel quad, the first
// pixel and the pixel strides of the calling thread.  Two lane maps fill it in, each with a thin __global__ wrapper.  The
// backward pass is the same loop per lane map, written once in each of its two kernels (own launch bounds, pixels in flight
// and slab layout; a shared body cost the half-wave kernel 4 %), on the same small helpers (fma4, relu_mask4, tap_values):
//   slot_lanes       G = 1, 2, 4, 8 (8 = the Cityscapes foreground classes): thread t of 256 handles the channel quad
//                    t % (GC/4) of pixel slot t / (GC/4), which needs G * 32 channel quads to divide 256 threads
//                    (gconv_taps_kernel, gconv_bwd_kernel; slab[workgroup][t][GC])
//   half_wave_lanes  every 1 <= G <= 31 (GC_GMAX): half-wave hw of the grid keeps group hw % G for its whole life and walks
//                    the pixels hw / G, hw / G + J, ... -- the half-waves of one step read one contiguous stretch of x
//                    (gconv_taps_generic_kernel, gconv_bwd_generic_kernel; slab[half-wave][t][128])
// Same T layout, same arithmetic per (pixel, group) in both.  The matrix-core / bit-mask kernels and the act-term kernels
// exist for the slot lane map only.  One gather kernel turns tap sums into rows (y or d act), one reduce kernel takes the
// run sums of a slab to dw of either slab layout or to dE.
//
// Host side: gconv_family turns (G, the gconv_mfma knob, bit mask requested) into the kernel family, gconv_ws_layout places
// tap sums and slabs in a workspace (the *_ws_floats queries and every entry point read it), gconv_slab_blocks is the slab
// grid rule, gconv_gather and gconv_slab_to are the two launch sequences every entry point shares.  The
// scan_gconv3x3_to1_any_* entry points take every G up to GC_GMAX; the ones without "any" issue the same launches and keep
// refusing every G outside {1, 2, 4, 8}, as their callers and tests expect.  scan_gconv3x3_to1_caps answers which of this
// a (G, Cg) would get right now.
#include "common.h"

#define GC_G 128  // channels per group

// Sum over each 32-lane half of the wave on the DPP path (no LDS crossbar): quad_perm xor 1, xor 2, row_half_mirror,
// row_mirror leave every lane of a 16-lane row with the row's sum; row_bcast15 then adds row 0 into row 1 and row 2 into
// row 3.  The total is valid in the lanes with (lane & 16) != 0.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_add(float v) {
  const int r = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROW_MASK, 0xF, false);
  return v + __builtin_bit_cast(float, r);
}
__device__ __forceinline__ float half_wave_sum_hi(float v) {
  v = dpp_add<0xB1, 0xF>(v);   // quad_perm [1,0,3,2]
  v = dpp_add<0x4E, 0xF>(v);   // quad_perm [2,3,0,1]
  v = dpp_add<0x141, 0xF>(v);  // row_half_mirror
  v = dpp_add<0x140, 0xF>(v);  // row_mirror
  v = dpp_add<0x142, 0xA>(v);  // row_bcast15 into rows 1 and 3
  return v;
}

// pixel row m of the pyramid -> row of its neighbour (dy, dx), or -1 outside the image
__device__ __forceinline__ int64_t neighbour_row(const scan_pyramid_t& d, int64_t m, const RowCoord& rc, int oy, int ox) {
  const int y = rc.y + oy, x = rc.x + ox;
  if (y < 0 || y >= d.h[rc.lvl] || x < 0 || x >= d.w[rc.lvl]) return -1;
  return m + (int64_t)oy * d.w[rc.lvl] + ox;
}

__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }

// acc += s * v
__device__ __forceinline__ void fma4(float4& acc, float s, const float4& v) {
  acc.x = __fmaf_rn(s, v.x, acc.x);
  acc.y = __fmaf_rn(s, v.y, acc.y);
  acc.z = __fmaf_rn(s, v.z, acc.z);
  acc.w = __fmaf_rn(s, v.w, acc.w);
}

// o where h > 0, else 0 (the producer's deferred ReLU)
__device__ __forceinline__ float4 relu_mask4(const float4& h, const float4& o) {
  return make_float4(h.x > 0.f ? o.x : 0.f, h.y > 0.f ? o.y : 0.f, h.z > 0.f ? o.z : 0.f, h.w > 0.f ? o.w : 0.f);
}

__device__ __forceinline__ float dot4(const float4& a, const float4& b) {
  return __fmaf_rn(a.x, b.x, __fmaf_rn(a.y, b.y, __fmaf_rn(a.z, b.z, a.w * b.w)));
}

// the nine <h, wv[t]> over a half-wave's 128 channels: lane 16 + t of the half-wave returns the sum of tap t
__device__ __forceinline__ float tap_sums(const float4& h, const float4 (&wv)[9], int l32) {
  float mine = 0.f;
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    const float s = half_wave_sum_hi(dot4(h, wv[t]));
    if (l32 == 16 + t) mine = s;
  }
  return mine;
}

// ... and those nine lanes write T[q][g][0..8]
__device__ __forceinline__ void tap_store(float* __restrict__ T, int64_t q, int G, int g, int l32, float mine) {
  if (l32 >= 16 && l32 < 25) T[(q * G + g) * 9 + (l32 - 16)] = mine;
}

__device__ __forceinline__ int64_t uniform_row(int64_t q) {
  return ((int64_t)__builtin_amdgcn_readfirstlane((int)(q >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)q);
}

// the nine values src[nb(q, SIGN * off(t)) * ld + g] of one (pixel, group), zero outside the image.  uniform (one pixel per
// workgroup iteration, q wave-uniform): the wave's two groups (lanes 0..31 / 32..63) need two wave-uniform values per tap.
// Lanes 0..17 fetch the 9 x 2 values with ONE load and every lane picks its own by v_readlane -- as nine same-address vector
// loads per KiB of x the gathers cost more address-unit time than the x stream itself (418 -> 234 us at P3 without them).
template <int SIGN>
__device__ __forceinline__ void tap_values(const scan_pyramid_t& d, int64_t q, const RowCoord& rc,
                                           const float* __restrict__ src, int ld, int g, bool uniform, float (&v)[9]) {
  if (uniform) {
    const int g0 = 2 * (int)(threadIdx.x >> 6);
    const int l = threadIdx.x & 63;
    const int tl = l % 9, gl = l / 9;
    const int64_t pl = l < 18 ? neighbour_row(d, q, rc, SIGN * (tl / 3 - 1), SIGN * (tl % 3 - 1)) : -1;
    const float val = pl >= 0 ? src[pl * ld + g0 + gl] : 0.f;
    const int vb = __builtin_bit_cast(int, val);
    const bool hi = (l & 32) != 0;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const float lo_v = __builtin_bit_cast(float, __builtin_amdgcn_readlane(vb, t));
      const float hi_v = __builtin_bit_cast(float, __builtin_amdgcn_readlane(vb, 9 + t));
      v[t] = hi ? hi_v : lo_v;
    }
  } else {
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int64_t p = neighbour_row(d, q, rc, SIGN * (t / 3 - 1), SIGN * (t % 3 - 1));
      v[t] = p >= 0 ? src[p * ld + g] : 0.f;
    }
  }
}

// ---- lane maps: where a thread works -----------------------------------------------------------------------------------------
// group g, lane l32 of the group's half-wave, offset coff of its channel quad in a pixel row; its pixels in flight are
// first + u * stride (u < UN) and it moves on by step.  uniform: one pixel per workgroup iteration (see tap_values).
struct LaneMap {
  int g, l32, coff;
  int64_t first, stride, step;
  bool uniform;
};

// G = 1, 2, 4, 8.  runs = false (tap sums): the workgroups interleave slot by slot, a thread's un pixels in flight lie one
// grid apart.  runs = true (backward): rows are dealt to the workgroups round-robin in runs of un * slots (grid-stride), not
// as one contiguous chunk each: with contiguous chunks of 128 rows x 4 KiB = 512 KiB the 1024 workgroups stream through
// addresses that differ by a power of two, i.e. through the same HBM channels at the same time (1.8 TB/s measured; the sum
// a workgroup accumulates does not depend on which rows it gets).
__device__ __forceinline__ LaneMap slot_lanes(int GC, int un, bool runs) {
  const int quads = GC >> 2;      // channel quads per pixel (32 per group)
  const int slots = 256 / quads;  // pixels per workgroup iteration
  const int cq = threadIdx.x % quads, slot = threadIdx.x / quads;
  LaneMap lm;
  lm.g = cq >> 5, lm.l32 = cq & 31, lm.coff = 4 * cq;
  lm.first = runs ? (int64_t)blockIdx.x * un * slots + slot : (int64_t)blockIdx.x * slots + slot;
  lm.stride = runs ? (int64_t)slots : (int64_t)gridDim.x * slots;
  lm.step = (int64_t)gridDim.x * un * slots;
  lm.uniform = slots == 1;
  return lm;
}

// any 1 <= G <= GC_GMAX: one 32-lane half-wave per (pixel, group).  The grid has J * G half-waves (J a multiple of 8, so
// J * G / 8 workgroups): half-wave hw serves group hw % G at the pixels hw / G + i J.
__device__ __forceinline__ int half_wave_id() { return blockIdx.x * 8 + (threadIdx.x >> 5); }
__device__ __forceinline__ LaneMap half_wave_lanes(int G, int un) {
  const int hw = half_wave_id();
  LaneMap lm;
  lm.g = hw % G, lm.l32 = threadIdx.x & 31, lm.coff = lm.g * GC_G + 4 * lm.l32;
  lm.first = hw / G;
  lm.stride = (int64_t)gridDim.x * 8 / G;
  lm.step = un * lm.stride;
  lm.uniform = false;
  return lm;
}

#define GC_UNROLL 2   // pixels in flight per thread, backward (36 + 36 + 26 live registers per lane)
#define GC_UNROLL_F 4 // forward: 4 KiB per wave in flight

// ---- forward: tap sums, then the gather ----------------------------------------------------------------------------------------
template <int UN>
__device__ __forceinline__ void taps_body(const float* __restrict__ x, int64_t M, int G, int GC, const float* __restrict__ w,
                                          float* __restrict__ T, const LaneMap& lm) {
  float4 wv[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) wv[t] = *reinterpret_cast<const float4*>(w + ((int64_t)lm.g * 9 + t) * GC + lm.coff);
  for (int64_t q0 = lm.first; q0 < M; q0 += lm.step) {
    float4 h[UN];
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const int64_t q = q0 + u * lm.stride;
      h[u] = q < M ? *reinterpret_cast<const float4*>(x + q * GC + lm.coff) : zero4();
    }
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const int64_t q = q0 + u * lm.stride;
      const float mine = tap_sums(h[u], wv, lm.l32);
      if (q < M) tap_store(T, q, G, lm.g, lm.l32, mine);
    }
  }
}

__global__ __launch_bounds__(256) void gconv_taps_kernel(const float* __restrict__ x, int64_t M, int G, int GC,
                                                         const float* __restrict__ w, float* __restrict__ T) {
  taps_body<GC_UNROLL_F>(x, M, G, GC, w, T, slot_lanes(GC, GC_UNROLL_F, false));
}

__global__ __launch_bounds__(256) void gconv_taps_generic_kernel(const float* __restrict__ x, int64_t M, int G, int GC,
                                                                 const float* __restrict__ w, float* __restrict__ T) {
  taps_body<GC_UNROLL_F>(x, M, G, GC, w, T, half_wave_lanes(G, GC_UNROLL_F));
}

// y[p][col0 + g] = bias[g] + sum_t T[nb(p, t)][g][t] for y [M][ldy] (bias may be null); every other column of the row is
// written as zero
__global__ __launch_bounds__(256) void gconv_gather_kernel(const float* __restrict__ T, scan_pyramid_t d, int G,
                                                           const float* __restrict__ bias, float* __restrict__ y, int ldy,
                                                           int col0) {
  const int64_t M = d.row_off[d.n_levels];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < M * ldy; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t p = i / ldy;
    const int g = (int)(i - p * ldy) - col0;
    float acc = 0.f;
    if (g >= 0 && g < G) {
      const RowCoord rc = decode_row(d, p);
      acc = bias != nullptr ? bias[g] : 0.f;
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const int64_t q = neighbour_row(d, p, rc, t / 3 - 1, t % 3 - 1);
        if (q >= 0) acc += T[(q * G + g) * 9 + t];
      }
    }
    y[i] = acc;
  }
}

// per-workgroup partials acc[t] (one float4 per thread and tap) of the slot lane map -> slab[block][t][GC]; several pixel
// slots per workgroup (GC < 1024) are added up through LDS in slot order
__device__ __forceinline__ void slab_store(const float4 (&acc)[9], float* __restrict__ red, float* __restrict__ slab, int GC) {
  const int quads = GC >> 2, slots = 256 / quads;
  const int cq = threadIdx.x % quads, slot = threadIdx.x / quads;
  float* out = slab + (int64_t)blockIdx.x * 9 * GC;
  if (slots == 1) {
#pragma unroll
    for (int t = 0; t < 9; ++t) *reinterpret_cast<float4*>(out + (int64_t)t * GC + 4 * cq) = acc[t];
    return;
  }
#pragma unroll
  for (int t = 0; t < 9; ++t) *reinterpret_cast<float4*>(red + (t * 256 + threadIdx.x) * 4) = acc[t];
  __syncthreads();
  if (slot == 0) {
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      float4 s = acc[t];
      for (int k = 1; k < slots; ++k) {
        const float4 v = *reinterpret_cast<const float4*>(red + (t * 256 + k * quads + cq) * 4);
        s.x += v.x;
        s.y += v.y;
        s.z += v.z;
        s.w += v.w;
      }
      *reinterpret_cast<float4*>(out + (int64_t)t * GC + 4 * cq) = s;
    }
  }
}

// ---- backward in one pass over x: per input pixel q the nine dy[q - off(t)][g] values serve both the data gradient
// (dx[q] = mask * sum_t dy_t * w[t]) and the weight gradient (acc[t] += dy_t * x[q]); x is read once.
// slab[block][t][GC]: the block's partial of dw[g(c)][t][c].
template <bool DO_DX, bool DO_DW>
__global__ __launch_bounds__(256) void gconv_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy, int Ns,
                                                        scan_pyramid_t d, int G, int GC, const float* __restrict__ w,
                                                        int relu_mask, float* __restrict__ dx, float* __restrict__ slab) {
  __shared__ float red[DO_DW ? 9 * 1024 : 4];
  const int64_t M = d.row_off[d.n_levels];
  // weight gradient alone: three pixels in flight per thread (the fused variant has no registers to spare)
  constexpr int UN = (DO_DW && !DO_DX) ? 3 : GC_UNROLL;
  const LaneMap lm = slot_lanes(GC, UN, true);
  float4 wv[9], acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    wv[t] = DO_DX ? *reinterpret_cast<const float4*>(w + ((int64_t)lm.g * 9 + t) * GC + lm.coff) : zero4();
    acc[t] = zero4();
  }
  const bool need_x = DO_DW || relu_mask;
  for (int64_t q0 = lm.first; q0 < M; q0 += lm.step) {
    float4 h[UN];
    float gy[UN][9];
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      int64_t q = q0 + u * lm.stride;
      if (lm.uniform) q = uniform_row(q);  // the row decode below is wave-uniform -> scalar unit
      h[u] = (q < M && need_x) ? *reinterpret_cast<const float4*>(x + q * GC + lm.coff) : zero4();
      if (q < M) {
        tap_values<-1>(d, q, decode_row(d, q), dy, Ns, lm.g, lm.uniform, gy[u]);  // x[q] feeds y[q - off(t)]
      } else {
#pragma unroll
        for (int t = 0; t < 9; ++t) gy[u][t] = 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const int64_t q = q0 + u * lm.stride;
      if (DO_DW) {
#pragma unroll
        for (int t = 0; t < 9; ++t) fma4(acc[t], gy[u][t], h[u]);
      }
      if (DO_DX && q < M) {
        float4 o = zero4();
#pragma unroll
        for (int t = 0; t < 9; ++t) fma4(o, gy[u][t], wv[t]);
        if (relu_mask) o = relu_mask4(h[u], o);
        *reinterpret_cast<float4*>(dx + q * GC + lm.coff) = o;
      }
    }
  }
  if (DO_DW) slab_store(acc, red, slab, GC);
}

// The same pass on the half-wave lane map, kept as a body of its own: sharing the loop above cost the both-gradients
// instance 4 % (0.810 -> 0.841 ms at 7 groups on the bench pyramid, profiles/r20_gconv_fold_ab.txt).
// slab[hw][t][128]: half-wave hw's partial of dw[hw % G][t][..] = slab[j][(g * 9 + t) * 128 + i] with hw = j G + g, i.e.
// J "blocks" of n = 9 * GC columns for gconv_slab_partial_kernel
template <bool DO_DX, bool DO_DW>
__global__ __launch_bounds__(256, 4) void gconv_bwd_generic_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                                   int Ns, scan_pyramid_t d, int G, int GC,
                                                                   const float* __restrict__ w, int relu_mask,
                                                                   float* __restrict__ dx, float* __restrict__ slab) {
  const int64_t M = d.row_off[d.n_levels];
  const int hw = half_wave_id(), l32 = threadIdx.x & 31;
  const int g = hw % G;
  const int64_t J = (int64_t)gridDim.x * 8 / G;
  const int64_t coff = (int64_t)g * GC_G + 4 * l32;
  float4 wv[9], acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    wv[t] = DO_DX ? *reinterpret_cast<const float4*>(w + ((int64_t)g * 9 + t) * GC + coff) : zero4();
    acc[t] = zero4();
  }
  const bool need_x = DO_DW || relu_mask;
  // both gradients at once: wv + acc are 72 registers, one pixel in flight keeps the kernel inside 128 without scratch
  constexpr int UN = (DO_DX && DO_DW) ? 1 : GC_UNROLL;
  for (int64_t q0 = hw / G; q0 < M; q0 += UN * J) {
    float4 h[UN];
    float gy[UN][9];
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const int64_t q = q0 + u * J;
      h[u] = (q < M && need_x) ? *reinterpret_cast<const float4*>(x + q * GC + coff) : zero4();
      if (q < M) {
        const RowCoord rc = decode_row(d, q);
#pragma unroll
        for (int t = 0; t < 9; ++t) {
          // y[p] took x[p + off(t)] * w[t], so x[q] feeds y[q - off(t)]
          const int64_t p = neighbour_row(d, q, rc, 1 - t / 3, 1 - t % 3);
          gy[u][t] = p >= 0 ? dy[p * Ns + g] : 0.f;
        }
      } else {
#pragma unroll
        for (int t = 0; t < 9; ++t) gy[u][t] = 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const int64_t q = q0 + u * J;
      if (DO_DW) {
#pragma unroll
        for (int t = 0; t < 9; ++t) fma4(acc[t], gy[u][t], h[u]);
      }
      if (DO_DX && q < M) {
        float4 o = zero4();
#pragma unroll
        for (int t = 0; t < 9; ++t) fma4(o, gy[u][t], wv[t]);
        if (relu_mask) o = relu_mask4(h[u], o);
        *reinterpret_cast<float4*>(dx + q * GC + coff) = o;
      }
    }
  }
  if (!DO_DW) return;
  float* out = slab + (int64_t)hw * 9 * GC_G + 4 * l32;
#pragma unroll
  for (int t = 0; t < 9; ++t) *reinterpret_cast<float4*>(out + t * GC_G) = acc[t];
}

// ---- matrix-core versions (v_mfma_f32_16x16x4_f32, exact fp32 products like the VALU kernels) -----------------------
// Forward taps as a GEMM per (16 consecutive pixels, group): [16 px x 128 ch] . [128 ch x 9 taps] -- the layout of the
// dynamic-conv forward kernel: a lane holds eight float4 of ITS pixel row (channels 16 j + 4 q .. + 3), which are four
// consecutive k-steps each, so the 128-long dot products need no cross-lane sums at all and a wave keeps 8 KiB of loads
// in flight.  relu_bits (optional): bit 4 j + e of word [(row * G + g) * 4 + q] = (x[row][g * 128 + 16 j + 4 q + e] > 0),
// the producer's ReLU mask for the backward pass (1/32 of re-reading x).
typedef float f32x4g __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void gconv_taps_mfma_kernel(const float* __restrict__ x, int64_t M, int G, int GC,
                                                              const float* __restrict__ w, float* __restrict__ T,
                                                              uint32_t* __restrict__ relu_bits) {
  const int lane = threadIdx.x & 63;
  const int col = lane & 15, q = lane >> 4;
  const int64_t wave_id = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t n_waves = (int64_t)gridDim.x * 4;  // a multiple of G (grid sizes are multiples of 2)
  const int g = (int)(wave_id % G);
  float4 bw[8];
#pragma unroll
  for (int j = 0; j < 8; ++j)
    bw[j] = col < 9 ? *reinterpret_cast<const float4*>(w + ((int64_t)g * 9 + col) * GC + g * GC_G + 16 * j + 4 * q)
                    : make_float4(0.f, 0.f, 0.f, 0.f);
  const int64_t groups = (M + 15) / 16;
  for (int64_t gidx = wave_id / G; gidx < groups; gidx += n_waves / G) {
    const int64_t row = gidx * 16 + col;
    float4 av[8];
#pragma unroll
    for (int j = 0; j < 8; ++j)
      av[j] = row < M ? *reinterpret_cast<const float4*>(x + row * GC + g * GC_G + 16 * j + 4 * q)
                      : make_float4(0.f, 0.f, 0.f, 0.f);
    f32x4g acc = {0.f, 0.f, 0.f, 0.f};
    uint32_t bits = 0u;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j].x, bw[j].x, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j].y, bw[j].y, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j].z, bw[j].z, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j].w, bw[j].w, acc, 0, 0, 0);
      bits |= (av[j].x > 0.f ? 1u : 0u) << (4 * j) | (av[j].y > 0.f ? 2u : 0u) << (4 * j) |
              (av[j].z > 0.f ? 4u : 0u) << (4 * j) | (av[j].w > 0.f ? 8u : 0u) << (4 * j);
    }
    if (relu_bits != nullptr && row < M) relu_bits[(row * G + g) * 4 + q] = bits;
    // C/D map (16x16): column = lane & 15 = tap, row = 4 * (lane >> 4) + reg = pixel of the group
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t orow = gidx * 16 + 4 * q + r;
      if (col < 9 && orow < M) T[(orow * G + g) * 9 + col] = acc[r];
    }
  }
}

// Data gradient as a GEMM per (16 consecutive pixels, group): dx^T [128 ch x 16 px] = w^T [128 ch x 9 taps] . gy [9 x 16]
// with gy[t][px] = dy[px - off(t)][g] gathered by the lanes (three per lane).  A lane ends up with four consecutive
// channels of its pixel per 16-channel tile -- the float4 layout of the forward loads, so the ReLU bits of the forward
// (or x itself) mask the result in place.
__global__ __launch_bounds__(256) void gconv_dx_mfma_kernel(const float* __restrict__ dy, int Ns, scan_pyramid_t d, int G,
                                                            int GC, const float* __restrict__ w,
                                                            const float* __restrict__ xmask,
                                                            const uint32_t* __restrict__ relu_bits,
                                                            float* __restrict__ dx) {
  const int64_t M = d.row_off[d.n_levels];
  const int lane = threadIdx.x & 63;
  const int col = lane & 15, q = lane >> 4;
  const int64_t wave_id = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t n_waves = (int64_t)gridDim.x * 4;
  const int g = (int)(wave_id % G);
  // A operand: row = channel `col` of tile, k = tap 4 s + q
  float aw[8][3];
#pragma unroll
  for (int tile = 0; tile < 8; ++tile)
#pragma unroll
    for (int s_ = 0; s_ < 3; ++s_) {
      const int t = 4 * s_ + q;
      aw[tile][s_] = t < 9 ? w[((int64_t)g * 9 + t) * GC + g * GC_G + 16 * tile + col] : 0.f;
    }
  const int64_t groups = (M + 15) / 16;
  for (int64_t gidx = wave_id / G; gidx < groups; gidx += n_waves / G) {
    const int64_t row = gidx * 16 + col;  // B operand / output: this lane's pixel
    float gy[3] = {0.f, 0.f, 0.f};
    if (row < M) {
      const RowCoord rc = decode_row(d, row);
#pragma unroll
      for (int s_ = 0; s_ < 3; ++s_) {
        const int t = 4 * s_ + q;
        if (t < 9) {
          // y[p] took x[p + off(t)] * w[t], so x[row] feeds y[row - off(t)]
          const int64_t p = neighbour_row(d, row, rc, 1 - t / 3, 1 - t % 3);
          if (p >= 0) gy[s_] = dy[p * Ns + g];
        }
      }
    }
    uint32_t bits = 0xffffffffu;
    float4 mk[8];
    if (relu_bits != nullptr) {
      if (row < M) bits = relu_bits[(row * G + g) * 4 + q];
    } else if (xmask != nullptr) {
#pragma unroll
      for (int tile = 0; tile < 8; ++tile)
        mk[tile] = row < M ? *reinterpret_cast<const float4*>(xmask + row * GC + g * GC_G + 16 * tile + 4 * q)
                           : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int tile = 0; tile < 8; ++tile) {
      f32x4g acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s_ = 0; s_ < 3; ++s_) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(aw[tile][s_], gy[s_], acc, 0, 0, 0);
      // C/D map: column = lane & 15 = pixel, row = 4 * (lane >> 4) + reg = channel inside the tile
      float4 o = make_float4(acc[0], acc[1], acc[2], acc[3]);
      if (relu_bits != nullptr) {
        o.x = (bits >> (4 * tile + 0)) & 1u ? o.x : 0.f;
        o.y = (bits >> (4 * tile + 1)) & 1u ? o.y : 0.f;
        o.z = (bits >> (4 * tile + 2)) & 1u ? o.z : 0.f;
        o.w = (bits >> (4 * tile + 3)) & 1u ? o.w : 0.f;
      } else if (xmask != nullptr) {
        o = relu_mask4(mk[tile], o);
      }
      if (row < M) *reinterpret_cast<float4*>(dx + row * GC + g * GC_G + 16 * tile + 4 * q) = o;
    }
  }
}

// ---- slab -> destination: two levels, fixed order ------------------------------------------------------------------------------
// slab [blocks][n] -> partial [parts][n]: part p sums its contiguous run of blocks in order (grid.y = parts)
__global__ __launch_bounds__(256) void gconv_slab_partial_kernel(const float* __restrict__ slab, int blocks, int n,
                                                                 int per_part, float* __restrict__ partial) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int b0 = blockIdx.y * per_part;
  const int b1 = b0 + per_part < blocks ? b0 + per_part : blocks;
  float s = 0.f;
#pragma unroll 8
  for (int b = b0; b < b1; ++b) s += slab[(int64_t)b * n + i];
  partial[(int64_t)blockIdx.y * n + i] = s;
}

// where column i of a slab's 9 * GC goes
enum GconvDst {
  GC_DST_DW,          // slab [t][GC] of the slot lane map              -> dw[g][t][g * 128 + i]
  GC_DST_DW_GENERIC,  // slab [(g * 9 + t) * 128 + i] of the half-waves -> dw[g][t][g * 128 + i]
  GC_DST_DE           // slab [t][GC] of the slot lane map              -> dE[g][t][i]
};
template <GconvDst DST>
__device__ __forceinline__ int64_t gconv_dst_index(int i, int GC) {
  if (DST == GC_DST_DW_GENERIC) {
    const int gt = i / GC_G, c = i - gt * GC_G;  // gt = g * 9 + t
    return (int64_t)gt * GC + (gt / 9) * GC_G + c;
  }
  const int t = i / GC, c = i - t * GC;
  return DST == GC_DST_DW ? ((int64_t)(c / GC_G) * 9 + t) * GC + c : ((int64_t)(c / GC_G) * 9 + t) * GC_G + c % GC_G;
}

// partial [parts][9 * GC] -> out (+= with accumulate), the parts added in order
template <GconvDst DST>
__global__ __launch_bounds__(256) void gconv_reduce_kernel(const float* __restrict__ partial, int parts, int GC,
                                                           float* __restrict__ out, int accumulate) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;  // over 9 * GC
  if (i >= 9 * GC) return;
  float s = 0.f;
  for (int b = 0; b < parts; ++b) s += partial[(int64_t)b * 9 * GC + i];
  float* dst = out + gconv_dst_index<DST>(i, GC);
  *dst = accumulate ? *dst + s : s;
}

// ---- class branches with the act-map channel taken out of the first conv (G = 1, 2, 4, 8) ---------------------------------
// The first conv of class c reads cat(x, act[c + 1]); its act channel reaches only that class's 128 hidden channels, so
// the dense conv runs on x alone (h_main = conv3x3(x; Wmain) + b1, stored before the ReLU) and the kernels below add
//   hact[q][g * 128 + i] = sum_t E[g][t][i] * a[nb(q, t)][g]        (E [G][9][128] = the act column of each class's weight,
//                                                                   a = act[:, a_col0 + g], zero outside the image)
// in registers wherever the kernels above read x:  hv = relu(h_main + hact)  feeds the tap products (forward), the mask
// (hv > 0) and the dw accumulation (backward).  Both directions add the nine terms in the tap order t = 0..8, so the
// backward's mask is bit for bit the forward's ReLU.  The act term's own gradients, dE[g][t][i] = sum_q dh[q][g * 128 + i] *
// a[nb(q, t)][g] in per-workgroup slabs summed in a fixed order and da[q][g] = sum_t <E[g][t], dh[nb(q, -t)][g * 128 ..]> as
// tap sums + the gather, come from dh while the backward kernel holds it in registers (gconv_bwd_act_kernel<.., true>:
// 0.16 ms of the training step faster than re-reading dh) or from one more pass over dh (gconv_act_grads_kernel).  No atomics.

// relu(h + sum_t ev[t] * av[t]), t ascending
__device__ __forceinline__ float4 act_hidden(float4 h, const float4 (&ev)[9], const float (&av)[9]) {
#pragma unroll
  for (int t = 0; t < 9; ++t) fma4(h, av[t], ev[t]);
  return relu_mask4(h, h);
}

// UNI: G = 8, one pixel per workgroup iteration (slots == 1): the pixel row is wave-uniform
#define GC_UNROLL_A 2  // pixels in flight per thread of the act backward kernels (nine more weight quads in registers)
#define GC_PICK_UNI(G, kernel, ...) ((G) == 8 ? kernel<true, ##__VA_ARGS__> : kernel<false, ##__VA_ARGS__>)

template <bool UNI>
__global__ __launch_bounds__(256) void gconv_taps_act_kernel(const float* __restrict__ x, scan_pyramid_t d, int G, int GC,
                                                             const float* __restrict__ w, const float* __restrict__ a,
                                                             int lda, const float* __restrict__ E, float* __restrict__ T) {
  const int64_t M = d.row_off[d.n_levels];
  const int quads = GC >> 2, slots = 256 / quads;
  const int cq = threadIdx.x % quads, slot = threadIdx.x / quads;
  const int g = cq >> 5, l32 = cq & 31;
  float4 wv[9], ev[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    wv[t] = *reinterpret_cast<const float4*>(w + ((int64_t)g * 9 + t) * GC + 4 * cq);
    ev[t] = *reinterpret_cast<const float4*>(E + ((int64_t)g * 9 + t) * GC_G + 4 * l32);
  }
  const int64_t stride = (int64_t)gridDim.x * slots;
  for (int64_t q0 = (int64_t)blockIdx.x * slots + slot; q0 < M; q0 += GC_UNROLL_F * stride) {
    float4 h[GC_UNROLL_F];
#pragma unroll
    for (int u = 0; u < GC_UNROLL_F; ++u) {
      const int64_t q = q0 + u * stride;
      h[u] = q < M ? *reinterpret_cast<const float4*>(x + q * GC + 4 * cq) : zero4();
    }
#pragma unroll
    for (int u = 0; u < GC_UNROLL_F; ++u) {
      int64_t q = q0 + u * stride;
      if (UNI) q = uniform_row(q);
      if (q >= M) continue;
      float av[9];  // fetched per pixel right before use: nine registers, not nine per pixel in flight
      tap_values<1>(d, q, decode_row(d, q), a, lda, g, UNI, av);
      tap_store(T, q, G, g, l32, tap_sums(act_hidden(h[u], ev, av), wv, l32));
    }
  }
}

// gconv_bwd_kernel<true, true> on hv = relu(x + hact): dx = (hv > 0) * sum_t dy_t * w[t], dw partials of hv
// FUSE: the act term's own gradients in the same pass, from dx while it is in registers (no second read of dh): the dE
// partials accE[t] += a[nb(q, t)] * dx[q] into slab_e and the tap sums of da into T, as gconv_act_grads_kernel forms them
template <bool UNI, bool FUSE>
__global__ __launch_bounds__(256, (UNI && !FUSE) ? 3 : 2) void gconv_bwd_act_kernel(
    const float* __restrict__ x, const float* __restrict__ dy, int Ns, scan_pyramid_t d, int G, int GC,
    const float* __restrict__ w, const float* __restrict__ a, int lda, const float* __restrict__ E, float* __restrict__ dx,
    float* __restrict__ slab, float* __restrict__ T, float* __restrict__ slab_e) {
  __shared__ float red[9 * 1024];
  const int64_t M = d.row_off[d.n_levels];
  const int quads = GC >> 2, slots = 256 / quads;
  const int cq = threadIdx.x % quads, slot = threadIdx.x / quads;
  const int g = cq >> 5, l32 = cq & 31;
  float4 wv[9], ev[9], acc[9], acc_e[9];  // dead without FUSE
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    wv[t] = *reinterpret_cast<const float4*>(w + ((int64_t)g * 9 + t) * GC + 4 * cq);
    ev[t] = *reinterpret_cast<const float4*>(E + ((int64_t)g * 9 + t) * GC_G + 4 * l32);
    acc[t] = zero4();
    if (FUSE) acc_e[t] = zero4();
  }
  // rows dealt round-robin in groups of UN * slots, as in gconv_bwd_kernel
  for (int64_t q0 = (int64_t)blockIdx.x * GC_UNROLL_A * slots + slot; q0 < M;
       q0 += (int64_t)gridDim.x * GC_UNROLL_A * slots) {
    float4 h[GC_UNROLL_A];
#pragma unroll
    for (int u = 0; u < GC_UNROLL_A; ++u) {
      const int64_t q = q0 + u * slots;
      h[u] = q < M ? *reinterpret_cast<const float4*>(x + q * GC + 4 * cq) : zero4();
    }
#pragma unroll
    for (int u = 0; u < GC_UNROLL_A; ++u) {
      int64_t q = q0 + u * slots;
      if (UNI) q = uniform_row(q);
      if (q >= M) continue;
      // the tap values of one pixel at a time, right before use: 9 + 9 registers, not 18 per pixel in flight
      const RowCoord rc = decode_row(d, q);
      float av[9], gy[9];
      tap_values<1>(d, q, rc, a, lda, g, UNI, av);
      const float4 hv = act_hidden(h[u], ev, av);
      tap_values<-1>(d, q, rc, dy, Ns, g, UNI, gy);  // x[q] feeds y[q - off(t)]
      float4 o = zero4();
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        fma4(acc[t], gy[t], hv);
        fma4(o, gy[t], wv[t]);
      }
      o = relu_mask4(hv, o);
      *reinterpret_cast<float4*>(dx + q * GC + 4 * cq) = o;
      if (FUSE) {
        float mine = 0.f;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
          fma4(acc_e[t], av[t], o);
          const float s = half_wave_sum_hi(dot4(o, ev[8 - t]));
          if (l32 == 16 + t) mine = s;
        }
        tap_store(T, q, G, g, l32, mine);
      }
    }
  }
  slab_store(acc, red, slab, GC);
  if (FUSE) {
    __syncthreads();  // the LDS staging of the first store is read by then
    slab_store(acc_e, red, slab_e, GC);
  }
}

// one pass over dh: the dE partials (acc[t] += a[nb(q, t)] * dh[q]) and the tap sums of da,
// T[q][g][t] = <dh[q][g * 128 ..], E[g][8 - t]>, so that da[p][g] = sum_t T[nb(p, t)][g][t] (the forward gather)
template <bool UNI>
__global__ __launch_bounds__(256) void gconv_act_grads_kernel(const float* __restrict__ dh, scan_pyramid_t d, int G, int GC,
                                                              const float* __restrict__ a, int lda,
                                                              const float* __restrict__ E, float* __restrict__ T,
                                                              float* __restrict__ slab) {
  __shared__ float red[9 * 1024];
  const int64_t M = d.row_off[d.n_levels];
  const int quads = GC >> 2, slots = 256 / quads;
  const int cq = threadIdx.x % quads, slot = threadIdx.x / quads;
  const int g = cq >> 5, l32 = cq & 31;
  float4 ev[9], acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    ev[t] = *reinterpret_cast<const float4*>(E + ((int64_t)g * 9 + t) * GC_G + 4 * l32);
    acc[t] = zero4();
  }
  for (int64_t q0 = (int64_t)blockIdx.x * GC_UNROLL_A * slots + slot; q0 < M;
       q0 += (int64_t)gridDim.x * GC_UNROLL_A * slots) {
    float4 h[GC_UNROLL_A];
#pragma unroll
    for (int u = 0; u < GC_UNROLL_A; ++u) {
      const int64_t q = q0 + u * slots;
      h[u] = q < M ? *reinterpret_cast<const float4*>(dh + q * GC + 4 * cq) : zero4();
    }
#pragma unroll
    for (int u = 0; u < GC_UNROLL_A; ++u) {
      int64_t q = q0 + u * slots;
      if (UNI) q = uniform_row(q);
      if (q >= M) continue;
      float av[9];
      tap_values<1>(d, q, decode_row(d, q), a, lda, g, UNI, av);
      float mine = 0.f;
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        fma4(acc[t], av[t], h[u]);
        const float s = half_wave_sum_hi(dot4(h[u], ev[8 - t]));
        if (l32 == 16 + t) mine = s;
      }
      tap_store(T, q, G, g, l32, mine);
    }
  }
  slab_store(acc, red, slab, GC);
}

// ---- host: one launch layer ----------------------------------------------------------------------------------------------------
#define GC_MAX_BLOCKS 1024
#define GC_PARTS 32
#define GC_GMAX 31

static bool gconv_lane_mapped(int G) { return G == 1 || G == 2 || G == 4 || G == 8; }

// any_g: the scan_gconv3x3_to1_any_* entry points (1 <= G <= GC_GMAX); the others keep to the four lane-mapped counts
static int gconv_check(const scan_pyramid_t* d, int G, int Cg, const char* who, bool any_g = false) {
  SCAN_CHECK_ARG(d && d->n_levels >= 1 && d->n_levels <= SCAN_MAX_LEVELS, "%s: bad pyramid", who);
  SCAN_CHECK_ARG(Cg == GC_G, "%s: only 128 channels per group are built (got %d)", who, Cg);
  if (any_g) {
    SCAN_CHECK_ARG(G >= 1 && G <= GC_GMAX, "%s: G=%d out of 1..%d", who, G, GC_GMAX);
    return 0;
  }
  SCAN_CHECK_ARG(gconv_lane_mapped(G), "%s: G=%d must be 1, 2, 4 or 8", who, G);
  return 0;
}

// scan_tune "gconv_mfma": 0 (default) = the fp32 FMA kernels (DPP half-wave sums forward; ONE backward pass over x that
// yields dx and the dw partials); 1 = tap products and data gradient on v_mfma_f32_16x16x4_f32 with the ReLU mask kept
// as bits by the forward.  Same products, different summation order.  Measured in the training step on one box
// (3 alternating runs each): FMA 68.8 / 69.1 / 68.7 ms, matrix cores 69.1 / 70.3 / 68.7 ms -- the matrix-core kernels
// are individually a little faster forward (147 vs 171 us at P3) but need two passes backward (dx 200 us + dw 235 us vs
// 480 us fused), so nothing is gained; all of them sit at 2.3-3.7 TB/s, bound by bytes in flight, not by arithmetic.
int g_scan_gconv_mfma = 0;

// (G, the knob, bit mask requested) -> kernel family; the only reader of the knob
enum GconvFamily { GC_GENERIC, GC_FMA, GC_MFMA };
static GconvFamily gconv_family(int G, bool bits) {
  if (!gconv_lane_mapped(G)) return GC_GENERIC;
  return (g_scan_gconv_mfma || bits) ? GC_MFMA : GC_FMA;
}

extern "C" int32_t scan_gconv3x3_to1_max_groups(void) { return GC_GMAX; }

extern "C" int32_t scan_gconv3x3_to1_caps(int32_t G, int32_t Cg) {
  if (G < 1 || G > GC_GMAX || Cg != GC_G) return 0;
  const GconvFamily f = gconv_family(G, false);
  return SCAN_GCONV_RUNS | (f == GC_GENERIC ? 0 : SCAN_GCONV_LANE_MAPPED) | (f == GC_MFMA ? SCAN_GCONV_BITS : 0) |
         (f == GC_FMA ? SCAN_GCONV_ACT : 0);
}

// A workspace, in floats from its start: the tap sums T [M][G][9], a slab (<= GC_MAX_BLOCKS partials of 9 * GC and their
// GC_PARTS run sums) and, for the act entry points, a second slab.  The plain entry points use T forward and the slab
// backward, never both: they share the start.  scan_gconv3x3_to1_act_backward_all keeps all three at once.
struct GconvWs {
  int64_t slab, slab_e, total;  // T starts at 0
};
static GconvWs gconv_ws_layout(int64_t M, int G, int Cg, bool act) {
  const int64_t taps = M * G * 9, slab = (int64_t)(GC_MAX_BLOCKS + GC_PARTS) * 9 * G * Cg;
  if (act) return {taps, taps + slab, taps + 2 * slab};
  return {0, -1, taps > slab ? taps : slab};
}

extern "C" int64_t scan_gconv3x3_to1_ws_floats(const scan_pyramid_t* d, int32_t G, int32_t Cg) {
  return d ? gconv_ws_layout(d->row_off[d->n_levels], G, Cg, false).total : -1;
}

extern "C" int64_t scan_gconv3x3_to1_act_ws_floats(const scan_pyramid_t* d, int32_t G, int32_t Cg) {
  return d ? gconv_ws_layout(d->row_off[d->n_levels], G, Cg, true).total : -1;
}

// pixel strides J of the generic kernels: a multiple of 8 (J * G / 8 whole workgroups), about `per` pixels per half-wave,
// at most max_j (the weight-gradient slab holds GC_MAX_BLOCKS strides)
static int gconv_generic_strides(int64_t M, int per, int max_j) {
  int64_t j = ((M + per - 1) / per + 7) / 8 * 8;
  if (j < 8) j = 8;
  if (j > max_j) j = max_j;
  return (int)j;
}

// workgroups of the slot-lane slab kernels
static int gconv_slab_blocks(int64_t M) {
  int64_t rpb = (M + GC_MAX_BLOCKS - 1) / GC_MAX_BLOCKS;
  if (rpb < 16) rpb = 16;  // small levels: fewer, fuller workgroups
  return (int)((M + rpb - 1) / rpb);
}

static int gconv_wave_grid(int64_t M, int G) {
  int64_t tasks = ((M + 15) / 16) * G;  // (16-pixel group, channel group) pairs, one per wave iteration
  int64_t blocks = (tasks + 3) / 4;
  if (blocks > 2048) blocks = 2048;
  if (blocks < 2) blocks = 2;
  return (int)((blocks + 1) / 2 * 2);   // even: 4 waves per block -> the wave count is a multiple of G <= 8
}

// tap sums T -> columns col0 .. col0 + G of y [M][ldy]
static int gconv_gather(const float* T, const scan_pyramid_t* d, int G, const float* bias, float* y, int ldy, int col0,
                        hipStream_t st) {
  const int64_t M = d->row_off[d->n_levels];
  hipLaunchKernelGGL(gconv_gather_kernel, dim3(grid_for(M * ldy, 256)), dim3(256), 0, st, T, *d, G, bias, y, ldy, col0);
  SCAN_LAUNCH_CHECK("gconv_gather");
  return 0;
}

// slab [blocks][9 * GC] -> its destination by the fixed-order two-level sum: at most GC_PARTS runs of consecutive blocks
// (or strides j of the generic slab), then the run sums
template <GconvDst DST>
static int gconv_slab_to(float* slab, int blocks, int GC, float* out, int accumulate, hipStream_t st) {
  const int n = 9 * GC, per = (blocks + GC_PARTS - 1) / GC_PARTS, parts = (blocks + per - 1) / per;
  float* partial = slab + (int64_t)GC_MAX_BLOCKS * n;
  hipLaunchKernelGGL(gconv_slab_partial_kernel, dim3((n + 255) / 256, parts), dim3(256), 0, st, slab, blocks, n, per, partial);
  SCAN_LAUNCH_CHECK("gconv_slab_partial");
  hipLaunchKernelGGL(gconv_reduce_kernel<DST>, dim3((n + 255) / 256), dim3(256), 0, st, partial, parts, GC, out, accumulate);
  SCAN_LAUNCH_CHECK(DST == GC_DST_DE ? "gconv_act_reduce" : "gconv_wgrad_reduce");
  return 0;
}

static int gconv_forward(const float* x, const scan_pyramid_t* d, int G, int Cg, const float* w, const float* bias, float* y,
                         int Ns, float* ws, uint32_t* relu_bits, hipStream_t st, bool any_g = false) {
  if (gconv_check(d, G, Cg, "gconv3x3_to1_forward", any_g)) return -1;
  SCAN_CHECK_ARG(x && w && y && ws && Ns >= G, "gconv3x3_to1_forward: bad arguments (Ns=%d)", Ns);
  const int64_t M = d->row_off[d->n_levels];
  if (M == 0) return 0;
  const int GC = G * Cg;
  switch (gconv_family(G, relu_bits != nullptr)) {
    case GC_GENERIC:
      SCAN_CHECK_ARG(relu_bits == nullptr, "gconv3x3_to1_forward_bits: G=%d must be 1, 2, 4 or 8", G);
      hipLaunchKernelGGL(gconv_taps_generic_kernel, dim3(gconv_generic_strides(M, GC_UNROLL_F, 2048) / 8 * G), dim3(256), 0,
                         st, x, M, G, GC, w, ws);
      SCAN_LAUNCH_CHECK("gconv_taps_generic");
      break;
    case GC_MFMA:
      hipLaunchKernelGGL(gconv_taps_mfma_kernel, dim3(gconv_wave_grid(M, G)), dim3(256), 0, st, x, M, G, GC, w, ws, relu_bits);
      SCAN_LAUNCH_CHECK("gconv_taps");
      break;
    case GC_FMA: {
      const int slots = 256 / (GC / 4);
      hipLaunchKernelGGL(gconv_taps_kernel, dim3(grid_for((M + slots - 1) / slots, 1)), dim3(256), 0, st, x, M, G, GC, w, ws);
      SCAN_LAUNCH_CHECK("gconv_taps");
    }
  }
  return gconv_gather(ws, d, G, bias, y, Ns, 0, st);
}

// gconv_bwd_kernel or gconv_bwd_generic_kernel <DO_DX, DO_DW>: same arguments
template <bool DO_DX, bool DO_DW>
static void gconv_bwd_launch(bool generic, int grid, hipStream_t st, const float* x, const float* dy, int Ns,
                             const scan_pyramid_t* d, int G, int GC, const float* w, int relu_mask, float* dx, float* slab) {
  hipLaunchKernelGGL((generic ? gconv_bwd_generic_kernel<DO_DX, DO_DW> : gconv_bwd_kernel<DO_DX, DO_DW>), dim3(grid), dim3(256),
                     0, st, x, dy, Ns, *d, G, GC, w, relu_mask, dx, slab);
}

static int gconv_backward(const float* x, const float* dy, int Ns, const scan_pyramid_t* d, int G, int Cg, const float* w,
                          int relu_mask, const uint32_t* relu_bits, float* dx, float* dw, int accumulate, float* ws,
                          hipStream_t st, const char* who, bool any_g = false) {
  if (gconv_check(d, G, Cg, who, any_g)) return -1;
  SCAN_CHECK_ARG(dy && Ns >= G && (dx || dw), "%s: bad arguments (Ns=%d)", who, Ns);
  SCAN_CHECK_ARG(!dx || w, "%s: the data gradient needs the weights", who);
  SCAN_CHECK_ARG(!dw || (x && ws), "%s: the weight gradient needs x and a workspace", who);
  SCAN_CHECK_ARG(!(dx && relu_mask && !relu_bits) || x, "%s: the ReLU mask needs x or its bit mask", who);
  const int64_t M = d->row_off[d->n_levels];
  if (M == 0) return 0;
  const int GC = G * Cg;
  const GconvFamily family = gconv_family(G, relu_bits != nullptr);
  const bool generic = family == GC_GENERIC;
  SCAN_CHECK_ARG(!generic || relu_bits == nullptr, "%s: G=%d must be 1, 2, 4 or 8", who, G);
  // slab "blocks": workgroups of the slot lane map, pixel strides J of the half-waves (J * G / 8 workgroups)
  const int blocks = generic ? gconv_generic_strides(M, 16, GC_MAX_BLOCKS) : gconv_slab_blocks(M);
  const int grid = generic ? blocks / 8 * G : blocks;
  float* slab = ws + gconv_ws_layout(M, G, Cg, false).slab;
  if (dx && family == GC_MFMA) {
    hipLaunchKernelGGL(gconv_dx_mfma_kernel, dim3(gconv_wave_grid(M, G)), dim3(256), 0, st, dy, Ns, *d, G, GC, w,
                       (relu_mask && !relu_bits) ? x : (const float*)nullptr, relu_bits, dx);
    SCAN_LAUNCH_CHECK(who);
    if (dw) gconv_bwd_launch<false, true>(generic, grid, st, x, dy, Ns, d, G, GC, w, 0, dx, slab);
  } else if (dx && dw) {
    gconv_bwd_launch<true, true>(generic, grid, st, x, dy, Ns, d, G, GC, w, relu_mask, dx, slab);
  } else if (dx) {
    gconv_bwd_launch<true, false>(generic, grid, st, x, dy, Ns, d, G, GC, w, relu_mask, dx, slab);
  } else {
    gconv_bwd_launch<false, true>(generic, grid, st, x, dy, Ns, d, G, GC, w, 0, dx, slab);
  }
  SCAN_LAUNCH_CHECK(who);
  if (!dw) return 0;
  return generic ? gconv_slab_to<GC_DST_DW_GENERIC>(slab, blocks, GC, dw, accumulate, st)
                 : gconv_slab_to<GC_DST_DW>(slab, blocks, GC, dw, accumulate, st);
}

extern "C" int scan_gconv3x3_to1_forward(const float* x, const scan_pyramid_t* d, int32_t G, int32_t Cg, const float* w,
                                         const float* bias, float* y, int32_t Ns, float* ws, void* stream) {
  return gconv_forward(x, d, G, Cg, w, bias, y, Ns, ws, nullptr, as_stream(stream));
}

// the same, also leaving the ReLU bit mask of x behind (relu_bits: M * G * 4 words) for scan_gconv3x3_to1_backward_bits
extern "C" int scan_gconv3x3_to1_forward_bits(const float* x, const scan_pyramid_t* d, int32_t G, int32_t Cg,
                                              const float* w, const float* bias, float* y, int32_t Ns, float* ws,
                                              uint32_t* relu_bits, void* stream) {
  SCAN_CHECK_ARG(relu_bits, "gconv3x3_to1_forward_bits: null bit mask");
  return gconv_forward(x, d, G, Cg, w, bias, y, Ns, ws, relu_bits, as_stream(stream));
}

extern "C" int scan_gconv3x3_to1_dgrad(const float* dy, int32_t Ns, const scan_pyramid_t* d, int32_t G, int32_t Cg,
                                       const float* w, const float* mask, float* dx, void* stream) {
  SCAN_CHECK_ARG(dx, "gconv3x3_to1_dgrad: null output");
  return gconv_backward(mask, dy, Ns, d, G, Cg, w, mask != nullptr, nullptr, dx, nullptr, 0, nullptr, as_stream(stream),
                        "gconv3x3_to1_dgrad");
}

extern "C" int scan_gconv3x3_to1_wgrad(const float* x, const float* dy, int32_t Ns, const scan_pyramid_t* d, int32_t G,
                                       int32_t Cg, float* dw, int32_t accumulate, float* ws, void* stream) {
  SCAN_CHECK_ARG(dw, "gconv3x3_to1_wgrad: null output");
  return gconv_backward(x, dy, Ns, d, G, Cg, nullptr, 0, nullptr, nullptr, dw, accumulate, ws, as_stream(stream),
                        "gconv3x3_to1_wgrad");
}

// both gradients (relu_mask != 0: dx is multiplied by (x > 0), the producer's deferred ReLU)
extern "C" int scan_gconv3x3_to1_backward(const float* x, const float* dy, int32_t Ns, const scan_pyramid_t* d, int32_t G,
                                          int32_t Cg, const float* w, int32_t relu_mask, float* dx, float* dw,
                                          int32_t accumulate, float* ws, void* stream) {
  SCAN_CHECK_ARG(x && dx && dw, "gconv3x3_to1_backward: null pointer");
  return gconv_backward(x, dy, Ns, d, G, Cg, w, relu_mask, nullptr, dx, dw, accumulate, ws, as_stream(stream),
                        "gconv3x3_to1_backward");
}

// both gradients with the ReLU mask taken from the forward's bit mask (x is read once, by the weight gradient)
extern "C" int scan_gconv3x3_to1_backward_bits(const float* x, const float* dy, int32_t Ns, const scan_pyramid_t* d,
                                               int32_t G, int32_t Cg, const float* w, const uint32_t* relu_bits, float* dx,
                                               float* dw, int32_t accumulate, float* ws, void* stream) {
  SCAN_CHECK_ARG(x && dx && dw && relu_bits, "gconv3x3_to1_backward_bits: null pointer");
  return gconv_backward(x, dy, Ns, d, G, Cg, w, 1, relu_bits, dx, dw, accumulate, ws, as_stream(stream),
                        "gconv3x3_to1_backward_bits");
}

// ---- any group count 1 <= G <= scan_gconv3x3_to1_max_groups(): G = 1, 2, 4, 8 run the slot-lane kernels, every other G the
// generic family.  Same arguments and results as the entry points without "any".
extern "C" int scan_gconv3x3_to1_any_forward(const float* x, const scan_pyramid_t* d, int32_t G, int32_t Cg, const float* w,
                                             const float* bias, float* y, int32_t Ns, float* ws, void* stream) {
  return gconv_forward(x, d, G, Cg, w, bias, y, Ns, ws, nullptr, as_stream(stream), true);
}

extern "C" int scan_gconv3x3_to1_any_dgrad(const float* dy, int32_t Ns, const scan_pyramid_t* d, int32_t G, int32_t Cg,
                                           const float* w, const float* mask, float* dx, void* stream) {
  SCAN_CHECK_ARG(dx, "gconv3x3_to1_any_dgrad: null output");
  return gconv_backward(mask, dy, Ns, d, G, Cg, w, mask != nullptr, nullptr, dx, nullptr, 0, nullptr, as_stream(stream),
                        "gconv3x3_to1_any_dgrad", true);
}

extern "C" int scan_gconv3x3_to1_any_wgrad(const float* x, const float* dy, int32_t Ns, const scan_pyramid_t* d, int32_t G,
                                           int32_t Cg, float* dw, int32_t accumulate, float* ws, void* stream) {
  SCAN_CHECK_ARG(dw, "gconv3x3_to1_any_wgrad: null output");
  return gconv_backward(x, dy, Ns, d, G, Cg, nullptr, 0, nullptr, nullptr, dw, accumulate, ws, as_stream(stream),
                        "gconv3x3_to1_any_wgrad", true);
}

extern "C" int scan_gconv3x3_to1_any_backward(const float* x, const float* dy, int32_t Ns, const scan_pyramid_t* d, int32_t G,
                                              int32_t Cg, const float* w, int32_t relu_mask, float* dx, float* dw,
                                              int32_t accumulate, float* ws, void* stream) {
  SCAN_CHECK_ARG(x && dx && dw, "gconv3x3_to1_any_backward: null pointer");
  return gconv_backward(x, dy, Ns, d, G, Cg, w, relu_mask, nullptr, dx, dw, accumulate, ws, as_stream(stream),
                        "gconv3x3_to1_any_backward", true);
}

// ---- the act-term entry points (G = 1, 2, 4, 8) -----------------------------------------------------------------------------
static int gconv_act_check(const scan_pyramid_t* d, int G, int Cg, const float* a, int lda, int a_col0, const float* E,
                           const char* who) {
  if (gconv_check(d, G, Cg, who)) return -1;
  SCAN_CHECK_ARG(a && E && a_col0 >= 0 && lda >= a_col0 + G, "%s: bad act map (lda=%d, first column %d, G=%d)", who, lda,
                 a_col0, G);
  return 0;
}

extern "C" int scan_gconv3x3_to1_act_forward(const float* x, const scan_pyramid_t* d, int32_t G, int32_t Cg, const float* w,
                                             const float* bias, const float* a, int32_t lda, int32_t a_col0, const float* E,
                                             float* y, int32_t Ns, float* ws, void* stream) {
  if (gconv_act_check(d, G, Cg, a, lda, a_col0, E, "gconv3x3_to1_act_forward")) return -1;
  SCAN_CHECK_ARG(x && w && y && ws && Ns >= G, "gconv3x3_to1_act_forward: bad arguments (Ns=%d)", Ns);
  const int64_t M = d->row_off[d->n_levels];
  if (M == 0) return 0;
  const int GC = G * Cg, slots = 256 / (GC / 4);
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(GC_PICK_UNI(G, gconv_taps_act_kernel), dim3(grid_for((M + slots - 1) / slots, 1)), dim3(256), 0, st, x, *d,
                     G, GC, w, a + a_col0, lda, E, ws);
  SCAN_LAUNCH_CHECK("gconv_taps_act");
  return gconv_gather(ws, d, G, bias, y, Ns, 0, st);
}

extern "C" int scan_gconv3x3_to1_act_backward(const float* x, const float* dy, int32_t Ns, const scan_pyramid_t* d, int32_t G,
                                              int32_t Cg, const float* w, const float* a, int32_t lda, int32_t a_col0,
                                              const float* E, float* dx, float* dw, int32_t accumulate, float* ws,
                                              void* stream) {
  if (gconv_act_check(d, G, Cg, a, lda, a_col0, E, "gconv3x3_to1_act_backward")) return -1;
  SCAN_CHECK_ARG(x && dy && w && dx && dw && ws && Ns >= G, "gconv3x3_to1_act_backward: bad arguments (Ns=%d)", Ns);
  const int64_t M = d->row_off[d->n_levels];
  if (M == 0) return 0;
  const int GC = G * Cg, blocks = gconv_slab_blocks(M);
  hipStream_t st = as_stream(stream);
  float* slab = ws + gconv_ws_layout(M, G, Cg, true).slab;
  hipLaunchKernelGGL(GC_PICK_UNI(G, gconv_bwd_act_kernel, false), dim3(blocks), dim3(256), 0, st, x, dy, Ns, *d, G, GC, w,
                     a + a_col0, lda, E, dx, slab, (float*)nullptr, (float*)nullptr);
  SCAN_LAUNCH_CHECK("gconv_bwd_act");
  return gconv_slab_to<GC_DST_DW>(slab, blocks, GC, dw, accumulate, st);
}

extern "C" int scan_gconv3x3_to1_act_grads(const float* dh, const scan_pyramid_t* d, int32_t G, int32_t Cg, const float* a,
                                           int32_t lda, int32_t a_col0, const float* E, float* da, int32_t ldda,
                                           int32_t da_col0, float* dE, int32_t accumulate, float* ws, void* stream) {
  if (gconv_act_check(d, G, Cg, a, lda, a_col0, E, "gconv3x3_to1_act_grads")) return -1;
  SCAN_CHECK_ARG(dh && da && dE && ws && da_col0 >= 0 && ldda >= da_col0 + G,
                 "gconv3x3_to1_act_grads: bad arguments (ldda=%d, first column %d)", ldda, da_col0);
  const int64_t M = d->row_off[d->n_levels];
  if (M == 0) return 0;
  const int GC = G * Cg, blocks = gconv_slab_blocks(M);
  hipStream_t st = as_stream(stream);
  float* slab = ws + gconv_ws_layout(M, G, Cg, true).slab;
  hipLaunchKernelGGL(GC_PICK_UNI(G, gconv_act_grads_kernel), dim3(blocks), dim3(256), 0, st, dh, *d, G, GC, a + a_col0, lda, E,
                     ws, slab);
  SCAN_LAUNCH_CHECK("gconv_act_grads");
  if (int rc = gconv_gather(ws, d, G, nullptr, da, ldda, da_col0, st)) return rc;
  return gconv_slab_to<GC_DST_DE>(slab, blocks, GC, dE, accumulate, st);
}

// scan_gconv3x3_to1_act_backward and scan_gconv3x3_to1_act_grads in ONE pass over x: dh is never read back
extern "C" int scan_gconv3x3_to1_act_backward_all(const float* x, const float* dy, int32_t Ns, const scan_pyramid_t* d,
                                                  int32_t G, int32_t Cg, const float* w, const float* a, int32_t lda,
                                                  int32_t a_col0, const float* E, float* dx, float* dw, float* da, int32_t ldda,
                                                  int32_t da_col0, float* dE, int32_t accumulate, float* ws, void* stream) {
  if (gconv_act_check(d, G, Cg, a, lda, a_col0, E, "gconv3x3_to1_act_backward_all")) return -1;
  SCAN_CHECK_ARG(x && dy && w && dx && dw && ws && Ns >= G, "gconv3x3_to1_act_backward_all: bad arguments (Ns=%d)", Ns);
  SCAN_CHECK_ARG(da && dE && da_col0 >= 0 && ldda >= da_col0 + G,
                 "gconv3x3_to1_act_backward_all: bad arguments (ldda=%d, first column %d)", ldda, da_col0);
  const int64_t M = d->row_off[d->n_levels];
  if (M == 0) return 0;
  const int GC = G * Cg, blocks = gconv_slab_blocks(M);
  hipStream_t st = as_stream(stream);
  const GconvWs L = gconv_ws_layout(M, G, Cg, true);
  hipLaunchKernelGGL(GC_PICK_UNI(G, gconv_bwd_act_kernel, true), dim3(blocks), dim3(256), 0, st, x, dy, Ns, *d, G, GC, w,
                     a + a_col0, lda, E, dx, ws + L.slab, ws, ws + L.slab_e);
  SCAN_LAUNCH_CHECK("gconv_bwd_act");
  if (int rc = gconv_gather(ws, d, G, nullptr, da, ldda, da_col0, st)) return rc;
  if (int rc = gconv_slab_to<GC_DST_DW>(ws + L.slab, blocks, GC, dw, accumulate, st)) return rc;
  return gconv_slab_to<GC_DST_DE>(ws + L.slab_e, blocks, GC, dE, accumulate, st);
}
