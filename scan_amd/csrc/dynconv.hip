// Semantic-conditioned dynamic 1x1 convolution + channel softmax for gfx950.
// Replaces GRAPHModule.dynamic_conv + softmax(dim=1)
// (reference rpn/fcos/condgraph.py:619-629, 344-346, 509-510, 541-542).
//
// feat [M,256] x kernels[K,256]^T -> logits [M,K] -> softmax -> probs [M,K].
// HBM-bound (1 KiB read, 72 B written per pixel).  Forward contracts on the matrix
// cores with v_mfma_f32_16x16x4_f32 (pixels x classes tiles, exact fp32), so the
// 256-deep dot products need no cross-lane reduction; the softmax runs on the 16-lane
// class groups of the accumulator layout.  Backward is a streaming VALU kernel
// (rank-K updates) with a deterministic two-stage reduction for d_kernels.
//
// Class counts.  K = 9 (Cityscapes -> Foggy) and K = 2 (Sim10k / KITTI -> Cityscapes) run the instantiations
// dynconv_fwd_kernel<K> / dynconv_bwd_kernel<K> with K at compile time.  Every other 2 <= K <= 32 (DC_KMAX) runs the
// generic family below them (scan_tune "dynconv_generic" = 1 sends 2 and 9 there too, for tests):
//   forward   the same MFMA chain per class column over one (K <= 16) or two (17..32) 16-class tiles; the B fragments
//             (64 VGPRs per tile in the <K> instances) are read from an LDS copy of `kernels` (<= 33 KB, rows padded to
//             260 floats so the 16 class rows of a float4 read fall into disjoint banks)
//   backward  one CHANNEL per lane, 64 channels per wave, the four waves of a workgroup side by side over the 256
//             channels of the same rows: w[KP] + dwacc[KP] are 2 * KP <= 64 VGPRs instead of the 8 * K of the float4
//             layout, a wave owns its channels outright (no LDS, no cross-wave sum), d_feat of a row is complete in one
//             pass and feat is read once.  dz of a row is computed once by 32 lanes (two rows per wave register).
#include "common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
#define DC_C 256

template <int K>
__global__ __launch_bounds__(256) void dynconv_fwd_kernel(const float* __restrict__ feat,
                                                          const float* __restrict__ kernels, int64_t M,
                                                          float* __restrict__ logits, float* __restrict__ probs) {
  const int lane = threadIdx.x & 63;
  const int col = lane & 15, q = lane >> 4;  // A: row = col-index of lane, k-quarter q
  // B fragments: lane supplies kernels[col][16j + 4q + e] for MFMA (j, e)
  float4 bw[16];
#pragma unroll
  for (int j = 0; j < 16; ++j)
    bw[j] = (col < K) ? *reinterpret_cast<const float4*>(kernels + col * DC_C + 16 * j + 4 * q)
                      : make_float4(0, 0, 0, 0);
  const int64_t groups = (M + 15) / 16;
  const int64_t wave_id = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t n_waves = (int64_t)gridDim.x * 4;
  for (int64_t gidx = wave_id; gidx < groups; gidx += n_waves) {
    const int64_t row = gidx * 16 + col;  // as A operand this lane feeds pixel row `col` of the tile
    float4 av[16];
    if (row < M) {
#pragma unroll
      for (int j = 0; j < 16; ++j) av[j] = *reinterpret_cast<const float4*>(feat + row * DC_C + 16 * j + 4 * q);
    } else {
#pragma unroll
      for (int j = 0; j < 16; ++j) av[j] = make_float4(0, 0, 0, 0);
    }
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j].x, bw[j].x, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j].y, bw[j].y, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j].z, bw[j].z, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j].w, bw[j].w, acc, 0, 0, 0);
    }
    // C/D map (16x16): class = lane & 15, pixel = 4*(lane>>4) + reg
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float z = acc[r];
      float mx = (col < K) ? z : -INFINITY;
#pragma unroll
      for (int off = 1; off < 16; off <<= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
      const float e = (col < K) ? expf(z - mx) : 0.f;
      float den = e;
#pragma unroll
      for (int off = 1; off < 16; off <<= 1) den += __shfl_xor(den, off, 64);
      const int64_t orow = gidx * 16 + 4 * q + r;
      if (col < K && orow < M) {
        logits[orow * K + col] = z;
        probs[orow * K + col] = e / den;
      }
    }
  }
}

// backward: lane -> 4 channels, wave -> FOUR consecutive rows per iteration.  part[block][K][256] partial d_kernels.
// The K softmax-backward coefficients of a row are computed ONCE by K lanes (16-lane group r handles row r: three
// coalesced 36-byte segment loads per wave instead of 27 same-address loads per lane and row), reduced with four
// xor-shuffles and broadcast to the wave as scalars (v_readlane -> SGPR operands of the FMAs).  Four rows in flight
// per wave hide the HBM latency the one-row-per-iteration version was bound by (1.1 -> ? TB/s, see profiles/).
template <int K>
__global__ __launch_bounds__(256) void dynconv_bwd_kernel(const float* __restrict__ feat,
                                                          const float* __restrict__ kernels,
                                                          const float* __restrict__ probs,
                                                          const float* __restrict__ d_logits_in,
                                                          const float* __restrict__ d_probs, int64_t M,
                                                          float* __restrict__ d_feat, float* __restrict__ part) {
  __shared__ float red[4][K][DC_C];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int gr = lane >> 4, gk = lane & 15;
  float4 w[K], dwacc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    w[k] = *reinterpret_cast<const float4*>(kernels + k * DC_C + 4 * lane);
    dwacc[k] = make_float4(0, 0, 0, 0);
  }
  const int64_t wave_id = (int64_t)blockIdx.x * 4 + wid;
  const int64_t n_waves = (int64_t)gridDim.x * 4;
  const int64_t chunks = (M + 3) >> 2;
  for (int64_t ch = wave_id; ch < chunks; ch += n_waves) {
    const int64_t row0 = ch << 2;
    float4 f[4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
      f[r] = (row0 + r < M) ? *reinterpret_cast<const float4*>(feat + (row0 + r) * DC_C + 4 * lane)
                            : make_float4(0, 0, 0, 0);
    const int64_t myrow = row0 + gr;
    const bool act = gk < K && myrow < M;
    const int64_t idx = myrow * K + gk;
    const float pl = (act && d_probs != nullptr) ? probs[idx] : 0.f;
    const float dp = (act && d_probs != nullptr) ? d_probs[idx] : 0.f;
    const float dl = (act && d_logits_in != nullptr) ? d_logits_in[idx] : 0.f;
    float dot = pl * dp;
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) dot += __shfl_xor(dot, off, 64);
    const float dzv = dl + pl * (dp - dot);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float4 o = make_float4(0, 0, 0, 0);
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const float dz = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(dzv), r * 16 + k));
        o.x += dz * w[k].x;
        o.y += dz * w[k].y;
        o.z += dz * w[k].z;
        o.w += dz * w[k].w;
        dwacc[k].x += dz * f[r].x;
        dwacc[k].y += dz * f[r].y;
        dwacc[k].z += dz * f[r].z;
        dwacc[k].w += dz * f[r].w;
      }
      if (row0 + r < M) *reinterpret_cast<float4*>(d_feat + (row0 + r) * DC_C + 4 * lane) = o;
    }
  }
#pragma unroll
  for (int k = 0; k < K; ++k) *reinterpret_cast<float4*>(&red[wid][k][4 * lane]) = dwacc[k];
  __syncthreads();
  for (int i = threadIdx.x; i < K * DC_C; i += 256) {
    const int k = i / DC_C, c = i - k * DC_C;
    part[(int64_t)blockIdx.x * K * DC_C + i] = red[0][k][c] + red[1][k][c] + red[2][k][c] + red[3][k][c];
  }
}

// ---- generic class count: 2 <= K <= DC_KMAX, K at run time ------------------------------------------------------------
#define DC_KMAX 32
#define DC_LDS_STRIDE 260  // floats per staged kernel row: 260 % 64 == 4 -> class rows 0..15 of one float4 read cover all banks

// NT = 16-class tiles.  `kernels` is staged in LDS for both (16.6 / 33.3 KB): the B fragments of the <K> instances are 64
// VGPRs per tile on top of the 64 of the A rows; read from LDS next to their MFMAs they cost none, and four waves per SIMD
// fit (the <K> instances run three).
template <int NT>
__global__ __launch_bounds__(256, 4) void dynconv_fwd_generic_kernel(const float* __restrict__ feat,
                                                                  const float* __restrict__ kernels, int64_t M, int K,
                                                                  float* __restrict__ logits, float* __restrict__ probs) {
  __shared__ float kl[NT * 16 * DC_LDS_STRIDE];
  const int lane = threadIdx.x & 63;
  const int col = lane & 15, q = lane >> 4;
  // NT * 16 rows x 64 quads; rows >= K are zero
  for (int i = threadIdx.x; i < NT * 16 * (DC_C / 4); i += 256) {
    const int k = i >> 6, c4 = i & 63;
    const float4 v = k < K ? *reinterpret_cast<const float4*>(kernels + k * DC_C + 4 * c4) : make_float4(0, 0, 0, 0);
    *reinterpret_cast<float4*>(&kl[k * DC_LDS_STRIDE + 4 * c4]) = v;
  }
  __syncthreads();
  const int64_t groups = (M + 15) / 16;
  const int64_t wave_id = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t n_waves = (int64_t)gridDim.x * 4;
  for (int64_t gidx = wave_id; gidx < groups; gidx += n_waves) {
    const int64_t row = gidx * 16 + col;
    // compiler barrier: without it the (loop-invariant) LDS reads are hoisted out of this loop into 64 NT registers
    __asm__ volatile("" ::: "memory");
    float4 av[16];
    if (row < M) {
#pragma unroll
      for (int j = 0; j < 16; ++j) av[j] = *reinterpret_cast<const float4*>(feat + row * DC_C + 16 * j + 4 * q);
    } else {
#pragma unroll
      for (int j = 0; j < 16; ++j) av[j] = make_float4(0, 0, 0, 0);
    }
    f32x4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 16; ++j) {
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const float4 b = *reinterpret_cast<const float4*>(&kl[(col + 16 * t) * DC_LDS_STRIDE + 16 * j + 4 * q]);
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j].x, b.x, acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j].y, b.y, acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j].z, b.z, acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j].w, b.w, acc[t], 0, 0, 0);
      }
    }
    // C/D map (16x16) per tile t: class = 16 t + (lane & 15), pixel = 4*(lane>>4) + reg
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float mx = -INFINITY;
#pragma unroll
      for (int t = 0; t < NT; ++t) mx = fmaxf(mx, (col + 16 * t < K) ? acc[t][r] : -INFINITY);
#pragma unroll
      for (int off = 1; off < 16; off <<= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
      float e[NT];
      float den = 0.f;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        e[t] = (col + 16 * t < K) ? expf(acc[t][r] - mx) : 0.f;
        den += e[t];
      }
#pragma unroll
      for (int off = 1; off < 16; off <<= 1) den += __shfl_xor(den, off, 64);
      const int64_t orow = gidx * 16 + 4 * q + r;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int k = col + 16 * t;
        if (k < K && orow < M) {
          logits[orow * K + k] = acc[t][r];
          probs[orow * K + k] = e[t] / den;
        }
      }
    }
  }
}

// KP = K rounded up to a multiple of 8 (unrolled class loops; rows K..KP-1 of w and the dz lanes >= K are zero).
// Wave `wid` owns channels 64 wid .. 64 wid + 63 of every row the workgroup handles; DC_GR rows per iteration (six at
// KP = 32, where eight would not fit 128 VGPRs).
template <int KP>
__global__ __launch_bounds__(256, 4) void dynconv_bwd_generic_kernel(const float* __restrict__ feat,
                                                                  const float* __restrict__ kernels,
                                                                  const float* __restrict__ probs,
                                                                  const float* __restrict__ d_logits_in,
                                                                  const float* __restrict__ d_probs, int64_t M, int K,
                                                                  float* __restrict__ d_feat, float* __restrict__ part) {
  constexpr int DC_GR = KP > 24 ? 6 : 8;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int c = 64 * wid + lane;
  const int hr = lane >> 5, hk = lane & 31;  // dz: 32 lanes per row, two rows per register
  float w[KP], dwacc[KP];
#pragma unroll
  for (int k = 0; k < KP; ++k) {
    w[k] = k < K ? kernels[k * DC_C + c] : 0.f;
    dwacc[k] = 0.f;
  }
  const int64_t chunks = (M + DC_GR - 1) / DC_GR;
  for (int64_t ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
    const int64_t row0 = ch * DC_GR;
    float f[DC_GR];
#pragma unroll
    for (int r = 0; r < DC_GR; ++r) f[r] = (row0 + r < M) ? feat[(row0 + r) * DC_C + c] : 0.f;
    float dzv[DC_GR / 2];
#pragma unroll
    for (int u = 0; u < DC_GR / 2; ++u) {
      const int64_t myrow = row0 + 2 * u + hr;
      const bool act = hk < K && myrow < M;
      const int64_t idx = myrow * K + hk;
      const float pl = (act && d_probs != nullptr) ? probs[idx] : 0.f;
      const float dp = (act && d_probs != nullptr) ? d_probs[idx] : 0.f;
      const float dl = (act && d_logits_in != nullptr) ? d_logits_in[idx] : 0.f;
      float dot = pl * dp;
#pragma unroll
      for (int off = 1; off < 32; off <<= 1) dot += __shfl_xor(dot, off, 64);
      dzv[u] = dl + pl * (dp - dot);
    }
#pragma unroll
    for (int r = 0; r < DC_GR; ++r) {
      float o = 0.f;
#pragma unroll
      for (int k = 0; k < KP; ++k) {
        const float dz = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(dzv[r >> 1]), (r & 1) * 32 + k));
        o += dz * w[k];
        dwacc[k] += dz * f[r];
      }
      if (row0 + r < M) d_feat[(row0 + r) * DC_C + c] = o;
    }
  }
#pragma unroll
  for (int k = 0; k < KP; ++k)
    if (k < K) part[((int64_t)blockIdx.x * K + k) * DC_C + c] = dwacc[k];
}

__global__ void dynconv_reduce_kernel(const float* __restrict__ part, int nb, int n, float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float s = 0.f;
  for (int b = 0; b < nb; ++b) s += part[(int64_t)b * n + i];
  out[i] = s;
}

static int dc_bwd_blocks(int64_t M) {
  int64_t b = (M + 63) / 64;
  if (b > 512) b = 512;
  if (b < 1) b = 1;
  return (int)b;
}

// scan_tune "dynconv_generic": 0 (default) = K = 2 / 9 on their compile-time instances; 1 = every K on the generic kernels
// (so that a test can put the two families side by side at the class counts that have reference fixtures)
int g_scan_dynconv_generic = 0;

static bool dc_specialised(int K) { return (K == 9 || K == 2) && !g_scan_dynconv_generic; }

// both families write one [K][C] partial per workgroup of dc_bwd_blocks(M)
extern "C" int64_t scan_dynconv_ws_floats(int64_t M, int32_t C, int32_t K) { return (int64_t)dc_bwd_blocks(M) * K * C; }

extern "C" int32_t scan_dynconv_max_classes(void) { return DC_KMAX; }

extern "C" int scan_dynconv_softmax_forward(const float* feat, const float* kernels, int64_t M, int32_t C, int32_t K,
                                            float* logits, float* probs, void* stream) {
  SCAN_CHECK_ARG(C == DC_C, "dynconv_softmax_forward: only C=256 is built (got %d)", C);
  SCAN_CHECK_ARG(K >= 2 && K <= DC_KMAX, "dynconv_softmax_forward: only K in 2..%d is built (got %d)", DC_KMAX, K);
  SCAN_CHECK_ARG(M >= 0, "dynconv_softmax_forward: bad M");
  if (M == 0) return 0;
  SCAN_CHECK_ARG(feat && kernels && logits && probs,
                 "dynconv_softmax_forward: null pointer (feat [M,256], kernels [K,256] with K in 2..%d, logits and probs [M,K])",
                 DC_KMAX);
  const int64_t groups = (M + 15) / 16;
  int64_t blocks = (groups + 3) / 4;
  if (blocks > 2048) blocks = 2048;
  hipStream_t st = as_stream(stream);
  if (!dc_specialised(K)) {
    if (K <= 16)
      hipLaunchKernelGGL((dynconv_fwd_generic_kernel<1>), dim3((int)blocks), dim3(256), 0, st, feat, kernels, M, K, logits,
                         probs);
    else
      hipLaunchKernelGGL((dynconv_fwd_generic_kernel<2>), dim3((int)blocks), dim3(256), 0, st, feat, kernels, M, K, logits,
                         probs);
    SCAN_LAUNCH_CHECK("dynconv_fwd_generic");
    return 0;
  }
  if (K == 9)
    hipLaunchKernelGGL((dynconv_fwd_kernel<9>), dim3((int)blocks), dim3(256), 0, st, feat, kernels, M, logits, probs);
  else
    hipLaunchKernelGGL((dynconv_fwd_kernel<2>), dim3((int)blocks), dim3(256), 0, st, feat, kernels, M, logits, probs);
  SCAN_LAUNCH_CHECK("dynconv_fwd");
  return 0;
}

extern "C" int scan_dynconv_softmax_backward(const float* feat, const float* kernels, const float* probs,
                                             const float* d_logits_in, const float* d_probs, int64_t M, int32_t C,
                                             int32_t K, float* d_feat, float* d_kernels, float* ws, void* stream) {
  SCAN_CHECK_ARG(C == DC_C, "dynconv_softmax_backward: only C=256 is built (got %d)", C);
  SCAN_CHECK_ARG(K >= 2 && K <= DC_KMAX, "dynconv_softmax_backward: only K in 2..%d is built (got %d)", DC_KMAX, K);
  SCAN_CHECK_ARG(M >= 0, "dynconv_softmax_backward: bad M");
  if (M == 0) {  // as the forward: no rows, no launch; the sum over no rows is zero
    SCAN_CHECK_ARG(d_kernels, "dynconv_softmax_backward: null pointer (d_kernels [K,256])");
    if (hipMemsetAsync(d_kernels, 0, sizeof(float) * K * C, as_stream(stream)) != hipSuccess) {
      scan_set_error("dynconv_softmax_backward: memset failed");
      return -2;
    }
    return 0;
  }
  SCAN_CHECK_ARG(feat && kernels && probs && d_feat && d_kernels && ws, "dynconv_softmax_backward: null pointer");
  const int nb = dc_bwd_blocks(M);
  hipStream_t st = as_stream(stream);
  if (!dc_specialised(K)) {
#define DC_BWD_GENERIC(KP) \
  hipLaunchKernelGGL((dynconv_bwd_generic_kernel<KP>), dim3(nb), dim3(256), 0, st, feat, kernels, probs, d_logits_in, \
                     d_probs, M, K, d_feat, ws)
    if (K <= 8) DC_BWD_GENERIC(8);
    else if (K <= 16) DC_BWD_GENERIC(16);
    else if (K <= 24) DC_BWD_GENERIC(24);
    else DC_BWD_GENERIC(32);
#undef DC_BWD_GENERIC
    SCAN_LAUNCH_CHECK("dynconv_bwd_generic");
    hipLaunchKernelGGL(dynconv_reduce_kernel, dim3((K * C + 255) / 256), dim3(256), 0, st, ws, nb, K * C, d_kernels);
    SCAN_LAUNCH_CHECK("dynconv_reduce");
    return 0;
  }
  if (K == 9)
    hipLaunchKernelGGL((dynconv_bwd_kernel<9>), dim3(nb), dim3(256), 0, st, feat, kernels, probs, d_logits_in, d_probs,
                       M, d_feat, ws);
  else
    hipLaunchKernelGGL((dynconv_bwd_kernel<2>), dim3(nb), dim3(256), 0, st, feat, kernels, probs, d_logits_in, d_probs,
                       M, d_feat, ws);
  SCAN_LAUNCH_CHECK("dynconv_bwd");
  hipLaunchKernelGGL(dynconv_reduce_kernel, dim3((K * C + 255) / 256), dim3(256), 0, st, ws, nb, K * C, d_kernels);
  SCAN_LAUNCH_CHECK("dynconv_reduce");
  return 0;
}
