// Anchor arithmetic shared by the anchor-based heads' kernels (retina.hip, rpn.hip): the anchor of a pyramid row formed from the
// [n_levels][A][4] cell table, BoxCoder.encode in fp64 and the smooth-L1 element.  Meant for translation units built with
// -ffp-contract=off (see boxes.h): every fp32 operation is rounded on its own.
#pragma once
#include "common.h"

#define RETINA_MAX_A 16

struct RetinaStrides {
  int s[SCAN_MAX_LEVELS];
};

// anchor a of row rc: the cell anchor plus the location's shift, one fp32 addition per corner (anchor_generator.py:73-95)
__device__ __forceinline__ float4 retina_anchor(const RetinaStrides& st, const float* __restrict__ cells, int A, const RowCoord rc,
                                                int a) {
  const float4 c = *reinterpret_cast<const float4*>(cells + ((int64_t)rc.lvl * A + a) * 4);
  const int s = pick_level(st.s, rc.lvl);
  const float sx = (float)(rc.x * s), sy = (float)(rc.y * s);
  return make_float4(c.x + sx, c.y + sy, c.z + sx, c.w + sy);
}

// BoxCoder.encode(box, anchor) with weights (wxy, wxy, wwh, wwh) and TO_REMOVE = 1 (modeling/box_coder.py:22-50), in fp64,
// rounded to fp32 once
__device__ __forceinline__ float4 box_encode(const float4 b, const float4 a, double wxy, double wwh) {
  const double ew = (double)a.z - (double)a.x + 1.0, eh = (double)a.w - (double)a.y + 1.0;
  const double ecx = (double)a.x + 0.5 * ew, ecy = (double)a.y + 0.5 * eh;
  const double gw = (double)b.z - (double)b.x + 1.0, gh = (double)b.w - (double)b.y + 1.0;
  const double gcx = (double)b.x + 0.5 * gw, gcy = (double)b.y + 0.5 * gh;
  return make_float4((float)(wxy * (gcx - ecx) / ew), (float)(wxy * (gcy - ecy) / eh), (float)(wwh * log(gw / ew)),
                     (float)(wwh * log(gh / eh)));
}

// the same with one weight per component (wx, wy, ww, wh): the box head's BBOX_REG_WEIGHTS (roi_box.hip)
__device__ __forceinline__ float4 box_encode4(const float4 b, const float4 a, double wx, double wy, double ww, double wh) {
  const double ew = (double)a.z - (double)a.x + 1.0, eh = (double)a.w - (double)a.y + 1.0;
  const double ecx = (double)a.x + 0.5 * ew, ecy = (double)a.y + 0.5 * eh;
  const double gw = (double)b.z - (double)b.x + 1.0, gh = (double)b.w - (double)b.y + 1.0;
  const double gcx = (double)b.x + 0.5 * gw, gcy = (double)b.y + 0.5 * gh;
  return make_float4((float)(wx * (gcx - ecx) / ew), (float)(wy * (gcy - ecy) / eh), (float)(ww * log(gw / ew)),
                     (float)(wh * log(gh / eh)));
}

__device__ __forceinline__ float smooth_l1_elem(float x, float t, float beta) {
  const float n = fabsf(x - t);
  return n < beta ? 0.5f * n * n / beta : n - 0.5f * beta;
}
__device__ __forceinline__ float smooth_l1_grad(float x, float t, float beta) {
  const float e = x - t;
  return fabsf(e) < beta ? e / beta : (e > 0.f ? 1.f : -1.f);
}

// host check of the geometry arguments every anchor kernel takes; fills the strides' kernel argument
static inline int retina_check(const scan_pyramid_t* d, const int32_t* strides, const float* cells, int32_t A, RetinaStrides* st,
                               const char* who) {
  if (scan_check_pyramid(d, who)) return -1;
  SCAN_CHECK_ARG(A >= 1 && A <= RETINA_MAX_A, "%s: A=%d anchors per location outside 1..%d", who, A, RETINA_MAX_A);
  SCAN_CHECK_ARG(d->row_off[d->n_levels] * A < (1ll << 40), "%s: too many anchors", who);
  SCAN_CHECK_ARG(strides && cells, "%s: null strides / cell anchors", who);
  SCAN_CHECK_ARG((reinterpret_cast<uintptr_t>(cells) & 15) == 0, "%s: cell anchors must be 16-byte aligned", who);
  for (int l = 0; l < SCAN_MAX_LEVELS; ++l) {
    st->s[l] = 1;
    if (l < d->n_levels) {
      SCAN_CHECK_ARG(strides[l] >= 1 && (int64_t)strides[l] * (d->h[l] > d->w[l] ? d->h[l] : d->w[l]) < (1 << 24),
                     "%s: level %d has stride %d (shifts must stay exact in fp32)", who, l, strides[l]);
      st->s[l] = strides[l];
    }
  }
  return 0;
}
