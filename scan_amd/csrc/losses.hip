// The loss family of the SCAN hot path for gfx950: SigmoidFocalLoss, IoU loss, (weighted) BCE-with-logits, the CKA class-conditional
// BCE and the softmax focal loss, forward and backward.  HBM-bound: 64-lane wavefront reductions, float4 streaming where the layout
// allows, grid-stride loops.  Every forward that ends in a sum has ONE host launcher, template <bool ORD>: it owns the argument
// checks, the choice of kernel form, the grid and the launch for the atomic entry point (ORD = false) and for its *_ordered twin
// (ORD = true: the blocks' sums go to a workspace, ordered_sum_kernel adds them up); the *_ordered_ws_floats query of a loss
// calls the grid function its launcher calls.  The first stage of an ordered sum (block_result<ORD>) is in common.h; the second
// (ordered_sum_kernel, ordered_sum_launch) is here, once for the library: the heads' losses in atss.hip and retina.hip use it too.
#include <float.h>

#include "common.h"
#include <algorithm>

// ------------------------------------------------------------------ sigmoid focal loss
// follows the reference's stable CUDA formula, csrc/cuda/SigmoidFocalLoss_cuda.cu:20-101
// Shared pieces: p = sigmoid(x) and expf(x - 2x[x>=0]) = expf(-|x|) are evaluated once; gamma == 2 (the shipped
// MODEL.FCOS.LOSS_GAMMA) squares instead of calling powf; the positive-class term is only evaluated by lanes that
// need it (a wave with no positive label skips it entirely).
template <bool G2>
__device__ __forceinline__ float focal_pow(float b, float gamma) {
  return G2 ? b * b : powf(b, gamma);
}
// One v_exp_f32, one v_rcp_f32 and one v_log_f32 per element, shared by both branches (round 4; the kernels were bound
// by vector-ALU issue, not by HBM: profiles/r03_pointwise_counters.txt -- two expf, a full-precision division and one or
// two logf per element through the math library):
//     e = exp(-|x|) in (0, 1]        r = 1 / (1 + e)        L = log(1 + e)
//     sigmoid(x) = x >= 0 ? r : e r         1 - sigmoid(x) = x >= 0 ? e r : r
//     log sigmoid(x) = min(x, 0) - L        the reference's second term -x [x >= 0] - log(1 + exp(x - 2 x [x >= 0])) = -max(x, 0) - L
// v_exp_f32 / v_log_f32 are good to ~1 ulp of their result and v_rcp_f32 to 1 ulp; L switches to its series below 2^-7
// where log(1 + e) would lose the low bits of e.  Against the C oracle (the reference's CUDA formula in libm floats) the
// element losses agree to rtol 1e-5 / atol 1e-7 as before (tests/test_gpu_kernels.py::test_sigmoid_focal_*).
struct SigParts {
  float p, q, L;  // sigmoid(x), 1 - sigmoid(x), log(1 + exp(-|x|))
};
__device__ __forceinline__ float fast_log1p_unit(float e) {  // log(1 + e), 0 <= e <= 1
  return e < 0.0078125f ? e * (1.f - e * (0.5f - e * 0.33333334f)) : __logf(1.f + e);
}
__device__ __forceinline__ SigParts sig_parts(float x) {
  const float e = __expf(-fabsf(x));
  const float r = __builtin_amdgcn_rcpf(1.f + e);
  const float er = e * r;
  SigParts s;
  s.p = x >= 0.f ? r : er;
  s.q = x >= 0.f ? er : r;
  s.L = fast_log1p_unit(e);
  return s;
}
template <bool G2>
__device__ __forceinline__ float focal_fwd_elem(float x, int t, int d, float gamma, float alpha) {
  if (t < 0) return 0.f;
  const SigParts s = sig_parts(x);
  if (t == d + 1) {
    const float logp = fmaxf(fminf(x, 0.f) - s.L, -87.33654f);  // log(max(p, FLT_MIN))
    return -focal_pow<G2>(s.q, gamma) * logp * alpha;
  }
  return focal_pow<G2>(s.p, gamma) * (fmaxf(x, 0.f) + s.L) * (1.f - alpha);
}
template <bool G2>
__device__ __forceinline__ float focal_bwd_elem(float x, int t, int d, float gamma, float alpha) {
  if (t < 0) return 0.f;
  const SigParts s = sig_parts(x);
  if (t == d + 1) {
    const float logp = fmaxf(fminf(x, 0.f) - s.L, -87.33654f);
    return -focal_pow<G2>(s.q, gamma) * (s.q - s.p * gamma * logp) * alpha;
  }
  return -focal_pow<G2>(s.p, gamma) * ((-fmaxf(x, 0.f) - s.L) * s.q * gamma - s.p) * (1.f - alpha);
}

// row (label index) and class of the 4 consecutive elements starting at i0 = 4q.  CT = compile-time class count of the
// two shipped configurations (8: Cityscapes, one label per two float4; 1: Sim10k / KITTI, one label per element),
// 0 = any C (one integer division per float4 instead of the 64-bit division per element this kernel used to pay).
template <int CT>
__device__ __forceinline__ void focal_rowcol(int64_t q, int C, const int* __restrict__ targets, int64_t total,
                                             int (&t)[4], int (&d)[4]) {
  if (CT == 8) {
    const int tt = targets[q >> 1];
    const int d0 = (int)(q & 1) * 4;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      t[e] = tt;
      d[e] = d0 + e;
    }
  } else if (CT == 1) {
    const int4 tt = reinterpret_cast<const int4*>(targets)[q];
    t[0] = tt.x; t[1] = tt.y; t[2] = tt.z; t[3] = tt.w;
#pragma unroll
    for (int e = 0; e < 4; ++e) d[e] = 0;
  } else {
    const int64_t i0 = q << 2;
    int64_t n = i0 / C;
    int dd = (int)(i0 - n * C);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      t[e] = (i0 + e < total) ? targets[n] : -1;
      d[e] = dd;
      if (++dd == C) {
        dd = 0;
        ++n;
      }
    }
  }
}

// ------------------------------------------------------------------ ordered reductions: the second stage (common.h has the first)
#define CKA_MAXC 32  // foreground classes: scan_dynconv_max_classes() - 1 fit
// Second stage: out[k] = sum over the blocks' slots part[b][k], b < nblk, in one fixed order -- lane l of the wave that owns
// column k adds slots l, l + 64, l + 128, ... in ascending order, then the 64 lane sums go through wave_sum's fixed shuffle
// tree.  One workgroup; the result is a function of the slots and of nblk alone.  fin != nullptr (CKA): the loss
// fin[1] = sum_c (out[2c] / out[2c+1]) / Cf of cka_finish, from the sums just formed.
__global__ __launch_bounds__(256) void ordered_sum_kernel(const float* __restrict__ part, int nblk, int ncols,
                                                          float* __restrict__ out, int Cf, float* __restrict__ fin) {
  __shared__ float tot[2 * CKA_MAXC];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  for (int k = wid; k < ncols; k += 4) {
    float s = 0.f;
    for (int b = lane; b < nblk; b += 64) s += part[(int64_t)b * ncols + k];
    s = wave_sum(s);
    if (lane == 0) {
      tot[k] = s;
      out[k] = s;
    }
  }
  if (fin != nullptr) {
    __syncthreads();
    if (threadIdx.x == 0) {
      float s = 0.f;
      for (int c = 0; c < Cf; ++c) s += tot[2 * c] / tot[2 * c + 1];
      fin[1] = s / (float)Cf;
    }
  }
}

int ordered_sum_launch(const float* part, int nblk, int ncols, float* out, int Cf, float* fin, void* stream, const char* who) {
  hipLaunchKernelGGL(ordered_sum_kernel, dim3(1), dim3(256), 0, as_stream(stream), part, nblk, ncols, out, Cf, fin);
  SCAN_LAUNCH_CHECK(who);
  return 0;
}

template <int CT, bool G2, bool ORD = false>
__global__ __launch_bounds__(256) void focal_fwd_kernel(const float* __restrict__ logits,
                                                        const int* __restrict__ targets, int64_t total, bool vec,
                                                        int C, float gamma, float alpha, float* __restrict__ losses,
                                                        float* __restrict__ loss_sum) {
  __shared__ float red[4];
  float acc = 0.f;
  const int64_t n4 = (total + 3) >> 2;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n4; q += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i0 = q << 2;
    float x[4], l[4];
    if (vec) {
      const float4 v = reinterpret_cast<const float4*>(logits)[q];
      x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) x[e] = (i0 + e < total) ? logits[i0 + e] : 0.f;
    }
    int t[4], d[4];
    focal_rowcol<CT>(q, C, targets, total, t, d);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      l[e] = (i0 + e < total) ? focal_fwd_elem<G2>(x[e], t[e], d[e], gamma, alpha) : 0.f;
      acc += l[e];
    }
    if (losses != nullptr) {
      if (vec) {
        reinterpret_cast<float4*>(losses)[q] = make_float4(l[0], l[1], l[2], l[3]);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (i0 + e < total) losses[i0 + e] = l[e];
      }
    }
  }
  if (loss_sum != nullptr) {
    const float s = block_sum_256(acc, red);
    if (threadIdx.x == 0) block_result<ORD>(loss_sum, 0, 1, s);
  }
}

template <int CT, bool G2>
__global__ __launch_bounds__(256) void focal_bwd_kernel(const float* __restrict__ logits,
                                                        const int* __restrict__ targets,
                                                        const float* __restrict__ d_losses, float d_scale,
                                                        int64_t total, bool vec, int C, float gamma, float alpha,
                                                        float* __restrict__ d_logits) {
  const int64_t n4 = (total + 3) >> 2;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n4; q += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i0 = q << 2;
    float x[4], up[4], g[4];
    if (vec) {
      const float4 v = reinterpret_cast<const float4*>(logits)[q];
      x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
      if (d_losses != nullptr) {
        const float4 u = reinterpret_cast<const float4*>(d_losses)[q];
        up[0] = u.x; up[1] = u.y; up[2] = u.z; up[3] = u.w;
      }
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        x[e] = (i0 + e < total) ? logits[i0 + e] : 0.f;
        if (d_losses != nullptr) up[e] = (i0 + e < total) ? d_losses[i0 + e] : 0.f;
      }
    }
    int t[4], d[4];
    focal_rowcol<CT>(q, C, targets, total, t, d);
#pragma unroll
    for (int e = 0; e < 4; ++e)
      g[e] = ((i0 + e < total) ? focal_bwd_elem<G2>(x[e], t[e], d[e], gamma, alpha) : 0.f) *
             (d_losses != nullptr ? up[e] : d_scale);
    if (vec) {
      reinterpret_cast<float4*>(d_logits)[q] = make_float4(g[0], g[1], g[2], g[3]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (i0 + e < total) d_logits[i0 + e] = g[e];
    }
  }
}

// loss reductions end in one float atomic per block on ONE address: keep the block count low (same-address atomics
// serialise at ~13 ns each: 2048 blocks cost ~55 us whatever the tensor size) and give each thread more elements
// scan_tune "reduce_blocks": the cap for the kernels bound by vector-ALU issue (focal losses: they need the occupancy of 8 blocks
// per CU); `light` = kernels with little arithmetic per byte, whose run time the end-of-block atomics are a visible part of:
// half the cap.  Round 5 sweep at M = 2^24 (tools/pointwise_roofline.py, same process): IoU forward 132 -> 113 us (0.57 -> 0.67 of
// the HBM roof), CKA BCE forward 220 -> 206 us (0.65 -> 0.69) at 1,024; sigmoid focal fused-sum forward 161 -> 193 us (worse).
int g_scan_reduce_blocks = 2048;
static inline int grid_reduce(int64_t work_items, int block, bool light = false) {
  int64_t g = (work_items + (int64_t)block * 8 - 1) / ((int64_t)block * 8);
  int cap = light ? g_scan_reduce_blocks / 2 : g_scan_reduce_blocks;
  if (cap < 1) cap = 1;  // scan_tune accepts any int: every setting must still give a launchable grid
  if (g < 1) g = 1;
  if (g > cap) g = cap;  // large tensors: the ~27 us of serialised atomics hide behind >= 100 us of streaming
  return (int)g;
}

// vec: the float4 form -- total a multiple of 4 AND every pointer the kernel would use as float4 16-byte aligned (focal_vec_ok;
// the kernel takes the same fact as its `vec` argument).  The C = 8 / C = 1 instances exist in that form only: anything else
// (a tail, or a contiguous view that starts 4 bytes into an allocation) runs the generic kernel's scalar loads and stores.
static inline bool focal_vec_ok(int64_t total, const void* a, const void* b, const void* c = nullptr) {
  return (total & 3) == 0 && ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c)) & 15) == 0;
}
#define FOCAL_FWD(CT, G2) focal_fwd_kernel<CT, G2, ORD>
#define FOCAL_BWD(CT, G2) focal_bwd_kernel<CT, G2>
#define FOCAL_DISPATCH(KERNEL, GRID, ...) /* KERNEL: FOCAL_FWD or FOCAL_BWD */                                     \
  do {                                                                                                              \
    const bool g2 = gamma == 2.0f;                                                                                  \
    if (C == 8 && vec) {                                                                                            \
      if (g2) hipLaunchKernelGGL((KERNEL(8, true)), dim3(GRID), dim3(256), 0, as_stream(stream), __VA_ARGS__);      \
      else hipLaunchKernelGGL((KERNEL(8, false)), dim3(GRID), dim3(256), 0, as_stream(stream), __VA_ARGS__);        \
    } else if (C == 1 && vec && (reinterpret_cast<uintptr_t>(targets) & 15) == 0) {                                 \
      if (g2) hipLaunchKernelGGL((KERNEL(1, true)), dim3(GRID), dim3(256), 0, as_stream(stream), __VA_ARGS__);      \
      else hipLaunchKernelGGL((KERNEL(1, false)), dim3(GRID), dim3(256), 0, as_stream(stream), __VA_ARGS__);        \
    } else {                                                                                                        \
      if (g2) hipLaunchKernelGGL((KERNEL(0, true)), dim3(GRID), dim3(256), 0, as_stream(stream), __VA_ARGS__);      \
      else hipLaunchKernelGGL((KERNEL(0, false)), dim3(GRID), dim3(256), 0, as_stream(stream), __VA_ARGS__);        \
    }                                                                                                               \
  } while (0)

// The launchers below: `who` names the entry point in messages.  ORD = false: the first stage adds its block sums to the output with
// float atomics.  ORD = true: it stores them to ws, one slot per block and output column, and ordered_sum_kernel forms the output.

// the grid of a forward that sums, under the current "reduce_blocks"; one workspace slot per block
static inline int focal_sum_grid(int64_t total) { return grid_reduce((total + 3) / 4, 256); }
extern "C" int64_t scan_sigmoid_focal_loss_ordered_ws_floats(int64_t M, int32_t C) { return focal_sum_grid(M * C); }

template <bool ORD>
static int focal_forward_launch(const float* logits, const int32_t* targets, int64_t M, int32_t C, float gamma, float alpha,
                                float* losses, float* loss_sum, float* ws, void* stream, const char* who) {
  SCAN_CHECK_ARG(M >= 0 && C > 0, "%s: bad shape M=%lld C=%d", who, (long long)M, C);
  if (M == 0) return 0;
  SCAN_CHECK_ARG(logits && targets, "%s: null input", who);
  const int64_t total = M * C;
  const int grid = loss_sum ? focal_sum_grid(total) : grid_for((total + 3) / 4, 256);  // losses only (atomic call): no atomics
  const bool vec = focal_vec_ok(total, logits, losses);  // losses == nullptr: not written
  FOCAL_DISPATCH(FOCAL_FWD, grid, logits, targets, total, vec, C, gamma, alpha, losses, ORD ? ws : loss_sum);
  SCAN_LAUNCH_CHECK(ORD ? "focal_fwd_ordered" : "focal_fwd");
  return ORD ? ordered_sum_launch(ws, grid, 1, loss_sum, 0, nullptr, stream, "focal_fwd_ordered_sum") : 0;
}

extern "C" int scan_sigmoid_focal_loss_forward(const float* logits, const int32_t* targets, int64_t M, int32_t C,
                                               float gamma, float alpha, float* losses, float* loss_sum,
                                               void* stream) {
  SCAN_CHECK_ARG(losses || loss_sum, "sigmoid_focal_loss_forward: no output requested");
  return focal_forward_launch<false>(logits, targets, M, C, gamma, alpha, losses, loss_sum, nullptr, stream, "sigmoid_focal_loss_forward");
}

extern "C" int scan_sigmoid_focal_loss_forward_ordered(const float* logits, const int32_t* targets, int64_t M, int32_t C,
                                                       float gamma, float alpha, float* losses, float* loss_sum, float* ws,
                                                       void* stream) {
  SCAN_CHECK_ARG(loss_sum && ws, "sigmoid_focal_loss_forward_ordered: loss_sum and ws are required");
  return focal_forward_launch<true>(logits, targets, M, C, gamma, alpha, losses, loss_sum, ws, stream,
                                    "sigmoid_focal_loss_forward_ordered");
}

extern "C" int scan_sigmoid_focal_loss_backward(const float* logits, const int32_t* targets, const float* d_losses,
                                                float d_scale, int64_t M, int32_t C, float gamma, float alpha,
                                                float* d_logits, void* stream) {
  SCAN_CHECK_ARG(M >= 0 && C > 0, "sigmoid_focal_loss_backward: bad shape M=%lld C=%d", (long long)M, C);
  if (M == 0) return 0;
  SCAN_CHECK_ARG(logits && targets && d_logits, "sigmoid_focal_loss_backward: null pointer");
  const int64_t total = M * C;
  const int grid = grid_for((total + 3) / 4, 256);
  const bool vec = focal_vec_ok(total, logits, d_logits, d_losses);  // d_losses == nullptr: d_scale instead
  FOCAL_DISPATCH(FOCAL_BWD, grid, logits, targets, d_losses, d_scale, total, vec, C, gamma, alpha, d_logits);
  SCAN_LAUNCH_CHECK("focal_bwd");
  return 0;
}

// ------------------------------------------------------------------ IoU loss (layers/iou_loss.py:5-36)
struct IouTerms {
  float loss, hI, wI, U, I, pw, ph;
};
__device__ __forceinline__ IouTerms iou_terms(const float4 p, const float4 t) {
  IouTerms r;
  const float ta = (t.x + t.z) * (t.y + t.w);
  r.pw = p.x + p.z;
  r.ph = p.y + p.w;
  const float pa = r.pw * r.ph;
  r.wI = fminf(p.x, t.x) + fminf(p.z, t.z);
  r.hI = fminf(p.w, t.w) + fminf(p.y, t.y);
  r.I = r.wI * r.hI;
  r.U = ta + pa - r.I;
  r.loss = -logf((r.I + 1.0f) / (r.U + 1.0f));
  return r;
}

template <bool ORD>
__global__ __launch_bounds__(256) void iou_fwd_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                      const float* __restrict__ weight, int64_t P,
                                                      float* __restrict__ out2) {
  __shared__ float red[4];
  float num = 0.f, den = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < P; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 p = reinterpret_cast<const float4*>(pred)[i];
    const float4 t = reinterpret_cast<const float4*>(target)[i];
    const float w = weight ? weight[i] : 1.f;
    num += iou_terms(p, t).loss * w;
    den += w;
  }
  const float sn = block_sum_256(num, red);
  const float sd = block_sum_256(den, red);
  if (threadIdx.x == 0) {
    block_result<ORD>(out2, 0, 2, sn);
    block_result<ORD>(out2, 1, 2, sd);
  }
}

// torch.min(a, b) backward: the gradient goes to the smaller input, split evenly on exact ties
__device__ __forceinline__ float min_grad(float a, float b) { return a < b ? 1.f : (a == b ? 0.5f : 0.f); }

__global__ __launch_bounds__(256) void iou_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                      const float* __restrict__ weight, int64_t P,
                                                      const float* __restrict__ g_num, float* __restrict__ d_pred) {
  const float g = g_num[0];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < P; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 p = reinterpret_cast<const float4*>(pred)[i];
    const float4 t = reinterpret_cast<const float4*>(target)[i];
    const IouTerms r = iou_terms(p, t);
    const float w = (weight ? weight[i] : 1.f) * g;
    // loss = log(U+1) - log(I+1);  U = ta + pa - I
    const float dU = 1.f / (r.U + 1.f);
    const float dI = -dU - 1.f / (r.I + 1.f);  // dU/dI = -1
    float4 o;
    o.x = w * (dU * r.ph + dI * r.hI * min_grad(p.x, t.x));  // left
    o.z = w * (dU * r.ph + dI * r.hI * min_grad(p.z, t.z));  // right
    o.y = w * (dU * r.pw + dI * r.wI * min_grad(p.y, t.y));  // top
    o.w = w * (dU * r.pw + dI * r.wI * min_grad(p.w, t.w));  // bottom
    reinterpret_cast<float4*>(d_pred)[i] = o;
  }
}

static inline int iou_grid(int64_t P) { return grid_reduce(P, 256, true); }
extern "C" int64_t scan_iou_loss_ordered_ws_floats(int64_t P) { return 2 * (int64_t)iou_grid(P); }

template <bool ORD>
static int iou_forward_launch(const float* pred, const float* target, const float* weight, int64_t P, float* out2, float* ws,
                              void* stream, const char* who) {
  SCAN_CHECK_ARG(P >= 0 && out2, "%s: bad arguments", who);
  if (P == 0) return 0;
  SCAN_CHECK_ARG(pred && target, "%s: null input", who);
  const int grid = iou_grid(P);
  hipLaunchKernelGGL(iou_fwd_kernel<ORD>, dim3(grid), dim3(256), 0, as_stream(stream), pred, target, weight, P, ORD ? ws : out2);
  SCAN_LAUNCH_CHECK(ORD ? "iou_fwd_ordered" : "iou_fwd");
  return ORD ? ordered_sum_launch(ws, grid, 2, out2, 0, nullptr, stream, "iou_fwd_ordered_sum") : 0;
}

extern "C" int scan_iou_loss_forward(const float* pred, const float* target, const float* weight, int64_t P,
                                     float* out2, void* stream) {
  return iou_forward_launch<false>(pred, target, weight, P, out2, nullptr, stream, "iou_loss_forward");
}

extern "C" int scan_iou_loss_forward_ordered(const float* pred, const float* target, const float* weight, int64_t P,
                                             float* out2, float* ws, void* stream) {
  SCAN_CHECK_ARG(ws, "iou_loss_forward_ordered: bad arguments");
  return iou_forward_launch<true>(pred, target, weight, P, out2, ws, stream, "iou_loss_forward_ordered");
}

extern "C" int scan_iou_loss_backward(const float* pred, const float* target, const float* weight, int64_t P,
                                      const float* g_num_dev, float* d_pred, void* stream) {
  SCAN_CHECK_ARG(P >= 0, "iou_loss_backward: bad arguments");
  if (P == 0) return 0;
  SCAN_CHECK_ARG(pred && target && g_num_dev && d_pred, "iou_loss_backward: null pointer");
  hipLaunchKernelGGL(iou_bwd_kernel, dim3(grid_for(P, 256)), dim3(256), 0, as_stream(stream), pred, target, weight, P,
                     g_num_dev, d_pred);
  SCAN_LAUNCH_CHECK("iou_bwd");
  return 0;
}

// ------------------------------------------------------------------ BCE with logits (optionally weighted)
// VEC: logits / targets / weight (unit stride) read as float4 -- four times fewer load instructions for the same bytes (the
// scalar form ran at 0.25 of the HBM roof at M = 2^24, bound by load issue: profiles/r04_pointwise_roofline.json)
template <bool VEC, bool ORD = false>
__global__ __launch_bounds__(256) void bce_fwd_kernel(const float* __restrict__ logits,
                                                      const float* __restrict__ targets, float const_target,
                                                      const float* __restrict__ weight, int64_t w_stride, int64_t M,
                                                      float* __restrict__ out2) {
  __shared__ float red[4];
  float num = 0.f, den = 0.f;
  auto elem = [&](float x, float t, float w) {
    // max(x,0) - x*t + log(1 + exp(-|x|))
    const float l = fmaxf(x, 0.f) - x * t + fast_log1p_unit(__expf(-fabsf(x)));
    num += l * w;
    den += w;
  };
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nthr = (int64_t)gridDim.x * blockDim.x;
  if (VEC) {
    const int64_t m4 = M >> 2;
#pragma unroll 4
    for (int64_t q = tid; q < m4; q += nthr) {
      const float4 x = reinterpret_cast<const float4*>(logits)[q];
      const float4 t = targets ? reinterpret_cast<const float4*>(targets)[q]
                               : make_float4(const_target, const_target, const_target, const_target);
      const float4 w = weight ? reinterpret_cast<const float4*>(weight)[q] : make_float4(1.f, 1.f, 1.f, 1.f);
      elem(x.x, t.x, w.x);
      elem(x.y, t.y, w.y);
      elem(x.z, t.z, w.z);
      elem(x.w, t.w, w.w);
    }
    for (int64_t i = (m4 << 2) + tid; i < M; i += nthr) elem(logits[i], targets ? targets[i] : const_target, weight ? weight[i] : 1.f);
  } else {
    for (int64_t i = tid; i < M; i += nthr)
      elem(logits[i], targets ? targets[i] : const_target, weight ? weight[i * w_stride] : 1.f);
  }
  const float sn = block_sum_256(num, red);
  const float sd = block_sum_256(den, red);
  if (threadIdx.x == 0) {
    block_result<ORD>(out2, 0, 2, sn);
    block_result<ORD>(out2, 1, 2, sd);
  }
}

__global__ __launch_bounds__(256) void bce_bwd_kernel(const float* __restrict__ logits,
                                                      const float* __restrict__ targets, float const_target,
                                                      const float* __restrict__ weight, int64_t w_stride, int64_t M,
                                                      const float* __restrict__ g_dev, float* __restrict__ d_logits) {
  const float g = g_dev[0];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < M; i += (int64_t)gridDim.x * blockDim.x) {
    const float x = logits[i];
    const float t = targets ? targets[i] : const_target;
    const float w = weight ? weight[i * w_stride] : 1.f;
    const float s = 1.f / (1.f + expf(-x));
    d_logits[i] = g * w * (s - t);
  }
}

// the float4 form: enough elements, and every pointer the kernel would read as float4 16-byte aligned (weight: unit stride too)
static inline bool bce_is_vec(const float* logits, const float* targets, const float* weight, int64_t w_stride, int64_t M) {
  auto al16 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
  return M >= 4096 && al16(logits) && (!targets || al16(targets)) && (!weight || (w_stride == 1 && al16(weight)));
}
// float4 form: the kernel ends in two float atomics per block on one cache line (~13 ns each, serialised): at 8 bytes per element the
// 2,048 blocks of grid_reduce cost more in atomics (53 us) than the stream itself (27 us at M = 2^24) -- 512 blocks there
static inline int bce_grid(int64_t M, bool vec) {
  return vec ? std::min(512, grid_reduce((M + 3) / 4, 256)) : grid_reduce(M, 256);
}
// the scalar form's grid: the query has no pointers, and the float4 form never launches more blocks
extern "C" int64_t scan_bce_logits_ordered_ws_floats(int64_t M) { return 2 * (int64_t)bce_grid(M, false); }

template <bool ORD>
static int bce_forward_launch(const float* logits, const float* targets, float const_target, const float* weight, int64_t w_stride,
                              int64_t M, float* out2, float* ws, void* stream, const char* who) {
  SCAN_CHECK_ARG(M >= 0 && out2, "%s: bad arguments", who);
  if (M == 0) return 0;
  SCAN_CHECK_ARG(logits, "%s: null input", who);
  const bool vec = bce_is_vec(logits, targets, weight, w_stride, M);
  const int grid = bce_grid(M, vec);
  hipLaunchKernelGGL((vec ? bce_fwd_kernel<true, ORD> : bce_fwd_kernel<false, ORD>), dim3(grid), dim3(256), 0, as_stream(stream),
                     logits, targets, const_target, weight, w_stride, M, ORD ? ws : out2);
  SCAN_LAUNCH_CHECK(ORD ? "bce_fwd_ordered" : "bce_fwd");
  return ORD ? ordered_sum_launch(ws, grid, 2, out2, 0, nullptr, stream, "bce_fwd_ordered_sum") : 0;
}

extern "C" int scan_bce_logits_forward(const float* logits, const float* targets, float const_target,
                                       const float* weight, int64_t w_stride, int64_t M, float* out2, void* stream) {
  return bce_forward_launch<false>(logits, targets, const_target, weight, w_stride, M, out2, nullptr, stream, "bce_logits_forward");
}

extern "C" int scan_bce_logits_forward_ordered(const float* logits, const float* targets, float const_target,
                                               const float* weight, int64_t w_stride, int64_t M, float* out2, float* ws,
                                               void* stream) {
  SCAN_CHECK_ARG(ws, "bce_logits_forward_ordered: bad arguments");
  return bce_forward_launch<true>(logits, targets, const_target, weight, w_stride, M, out2, ws, stream, "bce_logits_forward_ordered");
}

extern "C" int scan_bce_logits_backward(const float* logits, const float* targets, float const_target,
                                        const float* weight, int64_t w_stride, int64_t M, const float* g_dev,
                                        float* d_logits, void* stream) {
  SCAN_CHECK_ARG(M >= 0, "bce_logits_backward: bad arguments");
  if (M == 0) return 0;
  SCAN_CHECK_ARG(logits && g_dev && d_logits, "bce_logits_backward: null pointer");
  hipLaunchKernelGGL(bce_bwd_kernel, dim3(grid_for(M, 256)), dim3(256), 0, as_stream(stream), logits, targets,
                     const_target, weight, w_stride, M, g_dev, d_logits);
  SCAN_LAUNCH_CHECK("bce_bwd");
  return 0;
}

// ------------------------------------------------------------------ CKA class-conditional BCE
// fin != nullptr: the block that finishes last (ticket fin[0], zeroed by the caller) turns the completed sums into the
// loss  fin[1] = sum_c (num_c / den_c) / Cf  -- the reference's per-class weighted means averaged over the classes
// (discriminator/fcos_head_discriminator_con.py:119-121) -- so the layer needs no select / div / sum / div kernels of
// its own behind this launch.  The sums were added with float atomics (executed at the memory side): they are read
// back the same way.
__device__ __forceinline__ void cka_finish(float* __restrict__ out, int Cf, float* __restrict__ fin) {
  __shared__ unsigned last_flag;
  __threadfence();
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned t = atomicAdd(reinterpret_cast<unsigned*>(fin), 1u);
    last_flag = (t == gridDim.x - 1) ? 1u : 0u;
  }
  __syncthreads();
  if (last_flag && threadIdx.x == 0) {
    float s = 0.f;
    for (int c = 0; c < Cf; ++c) s += atomicAdd(out + 2 * c, 0.f) / atomicAdd(out + 2 * c + 1, 0.f);
    fin[1] = s / (float)Cf;
  }
}
template <bool ORD>
__global__ __launch_bounds__(256) void cka_fwd_kernel(const float* __restrict__ logits, const float* __restrict__ act,
                                                      int64_t M, int Cf, float t, float* __restrict__ out,
                                                      float* __restrict__ fin) {
  __shared__ float red[4];
  float num[CKA_MAXC], den[CKA_MAXC];
#pragma unroll
  for (int c = 0; c < CKA_MAXC; ++c) num[c] = den[c] = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < M; i += (int64_t)gridDim.x * blockDim.x) {
#pragma unroll
    for (int c = 0; c < CKA_MAXC; ++c) {
      if (c < Cf) {
        const float x = logits[i * Cf + c];
        const float w = act[i * (Cf + 1) + c + 1];
        const float l = fmaxf(x, 0.f) - x * t + fast_log1p_unit(__expf(-fabsf(x)));
        num[c] += l * w;
        den[c] += w;
      }
    }
  }
#pragma unroll
  for (int c = 0; c < CKA_MAXC; ++c) {
    if (c < Cf) {
      const float sn = block_sum_256(num[c], red);
      const float sd = block_sum_256(den[c], red);
      if (threadIdx.x == 0) {
        block_result<ORD>(out, 2 * c, 2 * Cf, sn);
        block_result<ORD>(out, 2 * c + 1, 2 * Cf, sd);
      }
    }
  }
  if (!ORD && fin != nullptr) cka_finish(out, Cf, fin);  // ORD: ordered_sum_kernel forms the loss
}

// Cf == 8 (Cityscapes): a thread owns one float4 of logits = half a row, i.e. ALWAYS the same four classes (the grid
// stride is even), so its eight partial sums stay in registers; the act-map row (9 floats, unaligned) is read by the two
// lanes of a row as 4 + 4 scalars of one contiguous wave-wide segment.  Even / odd lanes are reduced separately.
template <bool ORD>
__global__ __launch_bounds__(256) void cka_fwd8_kernel(const float* __restrict__ logits, const float* __restrict__ act,
                                                       int64_t M, float t, float* __restrict__ out,
                                                       float* __restrict__ fin) {
  __shared__ float red[4][16];
  float num[4] = {0.f, 0.f, 0.f, 0.f}, den[4] = {0.f, 0.f, 0.f, 0.f};
  const int64_t n4 = M * 2;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n4; q += (int64_t)gridDim.x * blockDim.x) {
    const float4 v = reinterpret_cast<const float4*>(logits)[q];
    const float* a = act + (q >> 1) * 9 + 1 + (q & 1) * 4;
    const float x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float w = a[e];
      const float l = fmaxf(x[e], 0.f) - x[e] * t + fast_log1p_unit(__expf(-fabsf(x[e])));
      num[e] += l * w;
      den[e] += w;
    }
  }
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
#pragma unroll
    for (int off = 32; off >= 2; off >>= 1) {  // keeps lane parity: lane 0 <- even lanes, lane 1 <- odd lanes
      num[e] += __shfl_down(num[e], off, 64);
      den[e] += __shfl_down(den[e], off, 64);
    }
    if (lane < 2) {
      red[wid][2 * (lane * 4 + e)] = num[e];       // class c = (lane & 1) * 4 + e
      red[wid][2 * (lane * 4 + e) + 1] = den[e];
    }
  }
  __syncthreads();
  if (threadIdx.x < 16)
    block_result<ORD>(out, threadIdx.x, 16, red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x]);
  if (!ORD && fin != nullptr) cka_finish(out, 8, fin);
}

// sums == nullptr: g [Cf] are the per-class coefficients; else g [1] is the gradient of the loss scalar and the
// coefficient of class c is g / (Cf * den_c), den_c = sums[2 c + 1] (what the layer's backward used to compute with
// three small kernels)
__global__ __launch_bounds__(256) void cka_bwd_kernel(const float* __restrict__ logits, const float* __restrict__ act,
                                                      int64_t M, int Cf, float t, const float* __restrict__ g,
                                                      const float* __restrict__ sums, float* __restrict__ d_logits) {
  __shared__ float coef[CKA_MAXC];
  if (threadIdx.x < Cf) coef[threadIdx.x] = sums ? g[0] / ((float)Cf * sums[2 * threadIdx.x + 1]) : g[threadIdx.x];
  __syncthreads();
  const int64_t total = M * Cf;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t m = i / Cf;
    const int c = (int)(i - m * Cf);
    const float x = logits[i];
    const float s = 1.f / (1.f + expf(-x));
    d_logits[i] = coef[c] * act[m * (Cf + 1) + c + 1] * (s - t);
  }
}

// the float4 kernel: Cf == 8 and logits 16-byte aligned, on half rows with the light cap; else the generic kernel on rows
static inline bool cka_is8(const float* logits, int32_t Cf) { return Cf == 8 && (reinterpret_cast<uintptr_t>(logits) & 15) == 0; }
static inline int cka_grid(int64_t M, bool is8) { return is8 ? grid_reduce(M * 2, 256, true) : grid_reduce(M, 256); }
// the larger of the two forms: the query has no pointer, and an aligned one (nullptr stands for it) may take either
extern "C" int64_t scan_cka_bce_ordered_ws_floats(int64_t M, int32_t Cf) {
  return 2 * (int64_t)Cf * std::max(cka_grid(M, false), cka_is8(nullptr, Cf) ? cka_grid(M, true) : 0);
}

// fin != nullptr (forward_loss): the loss goes to fin[1] -- from the block that finishes last (ticket fin[0]), or from ordered_sum_kernel
template <bool ORD>
static int cka_forward_launch(const float* logits, const float* act, int64_t M, int32_t Cf, float target, float* out, float* fin,
                              float* ws, void* stream, const char* who) {
  SCAN_CHECK_ARG(M >= 0 && Cf > 0 && Cf <= CKA_MAXC && out, "%s: bad arguments (Cf=%d)", who, Cf);
  if (M == 0) return 0;
  SCAN_CHECK_ARG(logits && act, "%s: null input", who);
  const bool is8 = cka_is8(logits, Cf);
  const int grid = cka_grid(M, is8);
  float* dst = ORD ? ws : out;
  float* kfin = ORD ? nullptr : fin;
  if (is8)
    hipLaunchKernelGGL(cka_fwd8_kernel<ORD>, dim3(grid), dim3(256), 0, as_stream(stream), logits, act, M, target, dst, kfin);
  else
    hipLaunchKernelGGL(cka_fwd_kernel<ORD>, dim3(grid), dim3(256), 0, as_stream(stream), logits, act, M, Cf, target, dst, kfin);
  SCAN_LAUNCH_CHECK(ORD ? "cka_fwd_ordered" : "cka_fwd");
  return ORD ? ordered_sum_launch(ws, grid, 2 * Cf, out, Cf, fin, stream, "cka_fwd_ordered_sum") : 0;
}

extern "C" int scan_cka_bce_forward(const float* logits, const float* act, int64_t M, int32_t Cf, float target,
                                    float* out, void* stream) {
  return cka_forward_launch<false>(logits, act, M, Cf, target, out, nullptr, nullptr, stream, "cka_bce_forward");
}

// out: 2 * Cf + 2 floats, zeroed by the caller: the sums, a ticket word, the loss (written by the last block)
extern "C" int scan_cka_bce_forward_loss(const float* logits, const float* act, int64_t M, int32_t Cf, float target,
                                         float* out, void* stream) {
  SCAN_CHECK_ARG(M > 0, "cka_bce_forward_loss: needs at least one row (the loss is a ratio of sums)");
  return cka_forward_launch<false>(logits, act, M, Cf, target, out, out ? out + 2 * Cf : nullptr, nullptr, stream, "cka_bce_forward_loss");
}

extern "C" int scan_cka_bce_forward_ordered(const float* logits, const float* act, int64_t M, int32_t Cf, float target,
                                            float* out, float* ws, void* stream) {
  SCAN_CHECK_ARG(ws, "cka_bce_forward_ordered: bad arguments (Cf=%d)", Cf);
  return cka_forward_launch<true>(logits, act, M, Cf, target, out, nullptr, ws, stream, "cka_bce_forward_ordered");
}

// out: 2 * Cf + 2 floats as scan_cka_bce_forward_loss; the ticket word out[2 Cf] is not touched
extern "C" int scan_cka_bce_forward_loss_ordered(const float* logits, const float* act, int64_t M, int32_t Cf, float target,
                                                 float* out, float* ws, void* stream) {
  SCAN_CHECK_ARG(M > 0, "cka_bce_forward_loss_ordered: needs at least one row (the loss is a ratio of sums)");
  SCAN_CHECK_ARG(ws, "cka_bce_forward_loss_ordered: bad arguments (Cf=%d)", Cf);
  return cka_forward_launch<true>(logits, act, M, Cf, target, out, out ? out + 2 * Cf : nullptr, ws, stream,
                                  "cka_bce_forward_loss_ordered");
}

extern "C" int scan_cka_bce_backward(const float* logits, const float* act, int64_t M, int32_t Cf, float target,
                                     const float* g_dev, float* d_logits, void* stream) {
  SCAN_CHECK_ARG(M >= 0 && Cf > 0 && Cf <= CKA_MAXC, "cka_bce_backward: bad arguments (Cf=%d)", Cf);
  if (M == 0) return 0;
  SCAN_CHECK_ARG(logits && act && g_dev && d_logits, "cka_bce_backward: null pointer");
  hipLaunchKernelGGL(cka_bwd_kernel, dim3(grid_for(M * Cf, 256)), dim3(256), 0, as_stream(stream), logits, act, M, Cf,
                     target, g_dev, (const float*)nullptr, d_logits);
  SCAN_LAUNCH_CHECK("cka_bwd");
  return 0;
}

// g_loss [1]: gradient of the loss scalar of scan_cka_bce_forward_loss; sums: that call's out
extern "C" int scan_cka_bce_backward_loss(const float* logits, const float* act, int64_t M, int32_t Cf, float target,
                                          const float* g_loss, const float* sums, float* d_logits, void* stream) {
  SCAN_CHECK_ARG(M >= 0 && Cf > 0 && Cf <= CKA_MAXC, "cka_bce_backward_loss: bad arguments (Cf=%d)", Cf);
  if (M == 0) return 0;
  SCAN_CHECK_ARG(logits && act && g_loss && sums && d_logits, "cka_bce_backward_loss: null pointer");
  hipLaunchKernelGGL(cka_bwd_kernel, dim3(grid_for(M * Cf, 256)), dim3(256), 0, as_stream(stream), logits, act, M, Cf,
                     target, g_loss, sums, d_logits);
  SCAN_LAUNCH_CHECK("cka_bwd");
  return 0;
}

// ------------------------------------------------------------------ softmax focal loss (alpha = 1)
// layers/sigmoid_focal_loss_wbg.py:38-64:  p = softmax(z)[label] clamped at 1e-15; -(1-p)^g log p
#define SFL_MAXK 16
#define SFL_MAXK_WIDE 32  // = scan_dynconv_max_classes()
// Rows are K floats (36 B at K = 9): a lane reading its own row touches a new cache line every 3-4 lanes.  A block
// therefore moves its 256 rows as ONE contiguous 256*K-float segment with coalesced dword accesses through LDS and each
// lane then walks its row in LDS (stride K floats: conflict-free for odd K).
// Round 4: no workgroup barriers.  A WAVE moves its own 64 rows (64 * K floats, contiguous) through a private LDS region:
// K coalesced dword loads per lane (lane + 64 j), written to LDS, then every lane walks its row there (stride K floats:
// conflict-free for odd K); LDS operations of one wave execute in order, so a wave-level fence is all that is needed.
// Two 64-row batches are in flight per wave and iteration (the first cut -- 256 rows per workgroup between two
// __syncthreads -- spent 72 % of its wave cycles parked: profiles/r03_pointwise_counters.txt).
// MAXK: the unrolled class bound and the LDS row pitch.  16 (SFL_MAXK) serves K <= 16 -- the shipped class counts; K = 17..32
// run the MAXK = 32 instances, one 64-row batch per wave and iteration so that the LDS region stays at 32 KB.
template <bool BWD, bool ORD = false, int MAXK = SFL_MAXK>
__global__ __launch_bounds__(256) void sfl_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                  int64_t M, int K, float gamma, float d_scale,
                                                  float* __restrict__ loss_sum, float* __restrict__ d_logits) {
  constexpr int NB = MAXK > SFL_MAXK ? 1 : 2;  // batches of 64 rows per wave and iteration
  __shared__ float rows_all[4 * NB * 64 * MAXK];
  __shared__ float red[4];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  float* wrows = rows_all + wid * (NB * 64 * MAXK);
  const bool g2 = gamma == 2.0f;
  const bool vec_ok = (reinterpret_cast<uintptr_t>(logits) & 15) == 0;
  float acc = 0.f;
  const int64_t nbatch = (M + 63) / 64;
  const int64_t stride = (int64_t)gridDim.x * 4 * NB;
  for (int64_t b0 = ((int64_t)blockIdx.x * 4 + wid) * NB; b0 < nbatch; b0 += stride) {
    constexpr int NV = MAXK / 4;  // float4 per lane and batch: 64 rows x K floats = 16 K float4, lane + 64 j
    float4 v[NB][NV];
    int nrow[NB];
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      const int64_t r0 = (b0 + u) * 64;
      nrow[u] = r0 < M ? (int)((M - r0 < 64) ? (M - r0) : 64) : 0;
      const float* src = logits + r0 * K;  // 64 * K * 4 bytes per batch: 16-byte aligned whenever logits is
      const int nf = nrow[u] * K;
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        const int i4 = 4 * (lane + 64 * j);
        v[u][j] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i4 + 3 < nf && vec_ok) {
          v[u][j] = *reinterpret_cast<const float4*>(src + i4);
        } else if (i4 < nf) {
          v[u][j].x = src[i4];
          if (i4 + 1 < nf) v[u][j].y = src[i4 + 1];
          if (i4 + 2 < nf) v[u][j].z = src[i4 + 2];
          if (i4 + 3 < nf) v[u][j].w = src[i4 + 3];
        }
      }
    }
#pragma unroll
    for (int u = 0; u < NB; ++u)
#pragma unroll
      for (int j = 0; j < NV; ++j)
        if (4 * 64 * j < 64 * K) *reinterpret_cast<float4*>(wrows + u * 64 * MAXK + 4 * (lane + 64 * j)) = v[u][j];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      const int64_t r0 = (b0 + u) * 64;
      float* z = wrows + u * 64 * MAXK + lane * K;
      if (lane < nrow[u]) {
        float e[MAXK];
        float mx = z[0];
#pragma unroll
        for (int k = 1; k < MAXK; ++k)
          if (k < K) mx = fmaxf(mx, z[k]);
        float den = 0.f;
#pragma unroll
        for (int k = 0; k < MAXK; ++k) {
          e[k] = (k < K) ? __expf(z[k] - mx) : 0.f;
          den += e[k];
        }
        const int lab = (int)labels[r0 + lane];
        float el = 0.f;
#pragma unroll
        for (int k = 0; k < MAXK; ++k) el = (k == lab) ? e[k] : el;
        const float inv = __builtin_amdgcn_rcpf(den);
        const float pr = el * inv;
        if (!BWD) {
          const float p = fmaxf(pr, 1e-15f);
          const float om = 1.f - p;
          // log p through its series near p = 1: log(p) there loses the low bits of 1 - p
          const float lp = om < 0.0078125f ? -om * (1.f + om * (0.5f + om * 0.33333334f)) : __logf(p);
          acc += -(g2 ? om * om : powf(om, gamma)) * lp;
        } else {
          float dLdp = 0.f;  // clamp(min=1e-15) has zero gradient below the clamp
          if (pr >= 1e-15f) {
            const float om = 1.f - pr;
            const float lp = om < 0.0078125f ? -om * (1.f + om * (0.5f + om * 0.33333334f)) : __logf(pr);
            const float ip = __builtin_amdgcn_rcpf(pr);
            dLdp = g2 ? (2.f * om * lp - om * om * ip) : (gamma * powf(om, gamma - 1.f) * lp - powf(om, gamma) * ip);
          }
          const float c = dLdp * pr * d_scale;
#pragma unroll
          for (int k = 0; k < MAXK; ++k)
            if (k < K) z[k] = c * ((k == lab ? 1.f : 0.f) - e[k] * inv);
        }
      }
    }
    if (BWD) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
      for (int u = 0; u < NB; ++u) {
        const int64_t r0 = (b0 + u) * 64;
        float* dst = d_logits + r0 * K;
        const int nf = nrow[u] * K;
        const bool st_ok = (reinterpret_cast<uintptr_t>(d_logits) & 15) == 0;
#pragma unroll
        for (int j = 0; j < MAXK / 4; ++j) {
          const int i4 = 4 * (lane + 64 * j);
          const float4 o = *reinterpret_cast<const float4*>(wrows + u * 64 * MAXK + i4);
          if (i4 + 3 < nf && st_ok) {
            *reinterpret_cast<float4*>(dst + i4) = o;
          } else if (i4 < nf) {
            dst[i4] = o.x;
            if (i4 + 1 < nf) dst[i4 + 1] = o.y;
            if (i4 + 2 < nf) dst[i4 + 2] = o.z;
            if (i4 + 3 < nf) dst[i4 + 3] = o.w;
          }
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();  // the region is rewritten by the next iteration's batches
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  if (!BWD) {
    const float sum = block_sum_256(acc, red);
    if (threadIdx.x == 0) block_result<ORD>(loss_sum, 0, 1, sum);
  }
}

// a workgroup iteration covers 4 waves x 2 batches x 64 rows; "reduce_blocks" does not reach these grids
static inline int sfl_grid(int64_t M, int cap) {
  const int64_t g = (M + 511) / 512;
  return (int)(g > cap ? cap : (g < 1 ? 1 : g));
}
static inline int sfl_fwd_grid(int64_t M) { return sfl_grid(M, 2048); }
extern "C" int64_t scan_softmax_focal_ordered_ws_floats(int64_t M) { return sfl_fwd_grid(M); }

// the one launch site: the 32-wide instance for K > 16
template <bool BWD, bool ORD>
static void sfl_launch(int grid, void* stream, const float* logits, const int64_t* labels, int64_t M, int32_t K, float gamma,
                       float d_scale, float* loss_sum, float* d_logits) {
  hipLaunchKernelGGL((K > SFL_MAXK ? sfl_kernel<BWD, ORD, SFL_MAXK_WIDE> : sfl_kernel<BWD, ORD, SFL_MAXK>), dim3(grid), dim3(256), 0,
                     as_stream(stream), logits, labels, M, K, gamma, d_scale, loss_sum, d_logits);
}

template <bool ORD>
static int sfl_forward_launch(const float* logits, const int64_t* labels, int64_t M, int32_t K, float gamma, float* loss_sum,
                              float* ws, void* stream, const char* who) {
  SCAN_CHECK_ARG(M >= 0 && K > 0 && K <= SFL_MAXK_WIDE && loss_sum, "%s: bad arguments (K=%d)", who, K);
  if (M == 0) return 0;
  SCAN_CHECK_ARG(logits && labels, "%s: null input", who);
  const int grid = sfl_fwd_grid(M);
  sfl_launch<false, ORD>(grid, stream, logits, labels, M, K, gamma, 0.f, ORD ? ws : loss_sum, nullptr);
  SCAN_LAUNCH_CHECK(ORD ? "sfl_fwd_ordered" : "sfl_fwd");
  return ORD ? ordered_sum_launch(ws, grid, 1, loss_sum, 0, nullptr, stream, "sfl_fwd_ordered_sum") : 0;
}

extern "C" int scan_softmax_focal_forward(const float* logits, const int64_t* labels, int64_t M, int32_t K,
                                          float gamma, float* loss_sum, void* stream) {
  return sfl_forward_launch<false>(logits, labels, M, K, gamma, loss_sum, nullptr, stream, "softmax_focal_forward");
}

extern "C" int scan_softmax_focal_forward_ordered(const float* logits, const int64_t* labels, int64_t M, int32_t K,
                                                  float gamma, float* loss_sum, float* ws, void* stream) {
  SCAN_CHECK_ARG(ws, "softmax_focal_forward_ordered: bad arguments (K=%d)", K);
  return sfl_forward_launch<true>(logits, labels, M, K, gamma, loss_sum, ws, stream, "softmax_focal_forward_ordered");
}

extern "C" int scan_softmax_focal_backward(const float* logits, const int64_t* labels, int64_t M, int32_t K,
                                           float gamma, float d_scale, float* d_logits, void* stream) {
  SCAN_CHECK_ARG(M >= 0 && K > 0 && K <= SFL_MAXK_WIDE, "softmax_focal_backward: bad arguments (K=%d)", K);
  if (M == 0) return 0;
  SCAN_CHECK_ARG(logits && labels && d_logits, "softmax_focal_backward: null pointer");
  sfl_launch<true, false>(sfl_grid(M, 4096), stream, logits, labels, M, K, gamma, d_scale, nullptr, d_logits);
  SCAN_LAUNCH_CHECK("sfl_bwd");
  return 0;
}
