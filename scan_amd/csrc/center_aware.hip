// Centre-aware alignment of the EPM baseline (reference discriminator/fcos_head_discriminator_CA.py:56-124) on pyramid row
// matrices for gfx950: the attention map of a whole pyramid in one launch, and the per-row, per-level scaling that puts the map
// (forward) and the gradient-reversal strength times the map (backward) onto the feature rows in one launch for all levels.
// Both are HBM-bound pointwise passes: float4 runs along the channels, no atomics, no reduction -- the same bits on every run.
#include <float.h>

#include "common.h"

// ------------------------------------------------------------------ atten[m] = sigmoid(w * max_c sigmoid(cls[m, c]) * sigmoid(ctr[m]))
// One lane per row.  sigmoid is increasing, so max_c sigmoid(x_c) = sigmoid(max_c x_c): the maximum is taken on the logits (exact)
// and ONE sigmoid follows.  Columns >= C of a row are never compared -- they are padding of the conv that wrote the rows and hold
// whatever that conv left there.  expf is the 1-ulp library form and the two divisions are IEEE ones (__fdiv_rn): tests/
// test_gpu_center_aware.py derives its error bound from exactly this sequence.
__device__ __forceinline__ float ca_sigmoid(float x) { return __fdiv_rn(1.f, 1.f + expf(-x)); }

template <bool VEC>
__global__ __launch_bounds__(256) void center_aware_map_kernel(const float* __restrict__ cls, int Cs, int C,
                                                               const float* __restrict__ ctr, int64_t ctr_stride, float weight,
                                                               int64_t M, float* __restrict__ atten) {
  for (int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; m < M; m += (int64_t)gridDim.x * blockDim.x) {
    const float* row = cls + m * Cs;
    float mx = -FLT_MAX;
    if (VEC) {
      for (int c = 0; c < C; c += 4) {  // c + 3 < Cs: Cs is a multiple of 4 and C <= Cs
        const float4 v = *reinterpret_cast<const float4*>(row + c);
        mx = fmaxf(mx, v.x);
        if (c + 1 < C) mx = fmaxf(mx, v.y);
        if (c + 2 < C) mx = fmaxf(mx, v.z);
        if (c + 3 < C) mx = fmaxf(mx, v.w);
      }
    } else {
      for (int c = 0; c < C; ++c) mx = fmaxf(mx, row[c]);
    }
    const float p = ca_sigmoid(mx);
    const float q = ca_sigmoid(ctr[m * ctr_stride]);
    atten[m] = ca_sigmoid(weight * p * q);
  }
}

extern "C" int scan_center_aware_map(const float* cls, int32_t Cs, int32_t C, const float* ctr, int64_t ctr_stride, float weight,
                                     int64_t M, float* atten, void* stream) {
  SCAN_CHECK_ARG(M >= 0 && C >= 1 && Cs >= C && ctr_stride >= 1, "center_aware_map: bad arguments (C=%d, Cs=%d)", C, Cs);
  if (M == 0) return 0;
  SCAN_CHECK_ARG(cls && ctr && atten, "center_aware_map: null pointer");
  const bool vec = Cs % 4 == 0 && (reinterpret_cast<uintptr_t>(cls) & 15) == 0;
  hipLaunchKernelGGL((vec ? center_aware_map_kernel<true> : center_aware_map_kernel<false>), dim3(grid_for(M, 256)), dim3(256), 0,
                     as_stream(stream), cls, Cs, C, ctr, ctr_stride, weight, M, atten);
  SCAN_LAUNCH_CHECK("center_aware_map");
  return 0;
}

// ------------------------------------------------------------------ y[m, :] = fl(s_l(m) * a[m]) * x[m, :]
// x is addressed through one base pointer per level (the level's first row), so the same kernel takes the rows of ONE matrix
// (forward: every base points into it) and the five separate gradient tensors autograd hands a split node (backward).  A level
// without a base writes zeros.  The row factor is formed once per float4 (one rounding: s * a; a missing map is the factor s
// itself), every product with x is one more rounding.
struct RowScaleLevels {
  const float* x[SCAN_MAX_LEVELS];
  float s[SCAN_MAX_LEVELS];
};

// idx_t: 32-bit element indices when the whole matrix has fewer than 2^31 float4s (every shape of the training step): the row /
// column split is then one 32-bit division instead of a 64-bit one, which this otherwise pure load-multiply-store loop feels
template <typename idx_t>
__global__ __launch_bounds__(256) void row_scale_levels_kernel(RowScaleLevels L, int ldx, const float* __restrict__ a,
                                                               scan_pyramid_t d, int c4, float* __restrict__ y, int ldy) {
  const idx_t total = (idx_t)(d.row_off[d.n_levels] * (int64_t)c4);
  const idx_t step = (idx_t)gridDim.x * blockDim.x;
  for (idx_t e = (idx_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += step) {
    const idx_t m = e / (idx_t)c4;
    const int c = (int)(e - m * (idx_t)c4) << 2;
    const int lvl = level_of(d.row_off, d.n_levels, (int64_t)m);
    const float* xl = L.x[lvl];
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (xl) {
      const float f = a ? L.s[lvl] * a[m] : L.s[lvl];
      v = *reinterpret_cast<const float4*>(xl + ((int64_t)m - d.row_off[lvl]) * ldx + c);
      v.x *= f; v.y *= f; v.z *= f; v.w *= f;
    }
    *reinterpret_cast<float4*>(y + (int64_t)m * ldy + c) = v;
  }
}

static int row_scale_launch(const RowScaleLevels& L, int32_t ldx, const float* a, const scan_pyramid_t* d, int32_t C, float* y,
                            int32_t ldy, void* stream) {
  auto al16 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
  SCAN_CHECK_ARG(C >= 4 && C % 4 == 0 && ldx >= C && ldy >= C && ldx % 4 == 0 && ldy % 4 == 0,
                 "row_scale_levels: C=%d, ldx=%d, ldy=%d must be multiples of 4 with ld >= C", C, ldx, ldy);
  if (d->row_off[d->n_levels] == 0) return 0;
  SCAN_CHECK_ARG(y && al16(y), "row_scale_levels: y must be 16-byte aligned");
  for (int l = 0; l < d->n_levels; ++l) SCAN_CHECK_ARG(al16(L.x[l]), "row_scale_levels: level %d of x is not 16-byte aligned", l);
  const int64_t total = d->row_off[d->n_levels] * (int64_t)(C / 4);
  // (the grid-stride step, at most 2048 * 256, must not carry a 32-bit index past 2^32: total + step < 2^31 + 2^19)
  if (total < (int64_t(1) << 31))
    hipLaunchKernelGGL(row_scale_levels_kernel<uint32_t>, dim3(grid_for(total, 256)), dim3(256), 0, as_stream(stream), L, ldx, a, *d,
                       C / 4, y, ldy);
  else
    hipLaunchKernelGGL(row_scale_levels_kernel<int64_t>, dim3(grid_for(total, 256)), dim3(256), 0, as_stream(stream), L, ldx, a, *d,
                       C / 4, y, ldy);
  SCAN_LAUNCH_CHECK("row_scale_levels");
  return 0;
}

static bool row_scale_desc_ok(const scan_pyramid_t* d, const float* s) {
  if (!d || !s || d->n_levels < 1 || d->n_levels > SCAN_MAX_LEVELS || d->row_off[0] != 0) return false;
  for (int l = 0; l < d->n_levels; ++l)
    if (d->row_off[l + 1] < d->row_off[l]) return false;
  return true;
}

extern "C" int scan_row_scale_levels(const float* x, int32_t ldx, const float* a, const float* s, const scan_pyramid_t* d,
                                     int32_t C, float* y, int32_t ldy, void* stream) {
  SCAN_CHECK_ARG(row_scale_desc_ok(d, s), "row_scale_levels: bad pyramid or scale table");
  SCAN_CHECK_ARG(x || d->row_off[d->n_levels] == 0, "row_scale_levels: null input");
  RowScaleLevels L = {};
  for (int l = 0; l < d->n_levels; ++l) {
    L.x[l] = x + d->row_off[l] * (int64_t)ldx;
    L.s[l] = s[l];
  }
  return row_scale_launch(L, ldx, a, d, C, y, ldy, stream);
}

extern "C" int scan_row_scale_levels_ptrs(const float* const* x_levels, int32_t ldx, const float* a, const float* s,
                                          const scan_pyramid_t* d, int32_t C, float* y, int32_t ldy, void* stream) {
  SCAN_CHECK_ARG(row_scale_desc_ok(d, s) && x_levels, "row_scale_levels_ptrs: bad pyramid, scale table or level table");
  RowScaleLevels L = {};
  for (int l = 0; l < d->n_levels; ++l) {
    L.x[l] = x_levels[l];
    L.s[l] = s[l];
  }
  return row_scale_launch(L, ldx, a, d, C, y, ldy, stream);
}
