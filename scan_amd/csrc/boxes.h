// Box arithmetic shared by the detection heads' kernels (atss.hip, retina.hip).  Meant for translation units built with
// -ffp-contract=off: every fp32 operation below is rounded on its own, as torch-CPU rounds the reference's, and the heads
// compare the results bit for bit (between two passes, and with the host oracles).
#pragma once
#include <hip/hip_runtime.h>

// boxlist_iou (structures/boxlist_ops.py) of one pair of xyxy boxes, TO_REMOVE = 1.  min / max take `first` as their first
// operand: each head keeps the operand order it always had (ATSS: the anchor first; RetinaNet: the box first).
__device__ __forceinline__ float boxlist_iou(const float4 first, const float4 second) {
  const float area1 = (first.z - first.x + 1.f) * (first.w - first.y + 1.f);
  const float area2 = (second.z - second.x + 1.f) * (second.w - second.y + 1.f);
  const float w = fmaxf(fminf(first.z, second.z) - fmaxf(first.x, second.x) + 1.f, 0.f);
  const float h = fmaxf(fminf(first.w, second.w) - fmaxf(first.y, second.y) + 1.f, 0.f);
  const float inter = w * h;
  return inter / (area1 + area2 - inter);
}
