// The ATSS detection head's device side: the ground-truth plan (reference rpn/atss/loss.py:159-218, 354, 360-373) and the
// GIoU loss on anchor deltas (loss.py:64-105, BoxCoder rpn/atss/atss.py:14-97).  One anchor per location (ratio 1.0, one
// scale): the anchors of a level are its pyramid rows, computed from (level, y, x) -- centre (x * s + (s - 1) / 2,
// y * s + (s - 1) / 2), corners centre -/+ (a - 1) / 2 -- and never stored.
//
// The plan, per image and box g (the tie rules are this project's: the reference leaves them to torch.topk / torch.max):
//   candidates  on each level the min(topk, anchors of the level) anchors whose centre is nearest to the box centre
//               ((x1 + x2) / 2, (y1 + y2) / 2); distance = sqrt(dx * dx + dy * dy) in fp32, every operation rounded on its
//               own (this file is built with -ffp-contract=off); equal distances go to the smaller row
//   IoU         anchor against box with the +1 widths of structures/boxlist_ops.py: boxlist_iou
//   threshold   mean + unbiased standard deviation of the candidates' IoUs over all levels (at most 5 * topk values), summed
//               in fp64 in candidate order and rounded to fp32 once; a single candidate gives NaN (no positives), as torch.std
//   positive    a candidate whose IoU >= threshold and whose centre lies inside the box with min(l, t, r, b) > 0.01
//   contested   an anchor positive for several boxes takes the box of largest IoU, equal IoUs the smaller box index:
//               a 64-bit integer max of (IoU bits << 32) | ~g per row (IoU >= 0: its bits order like its value), which is
//               order-independent -- the plan is bit-reproducible with scan_tune "deterministic" on or off, no ordered twin
//   background  an anchor positive for no box gets label 0; an image with ng = 0 is all background (the reference raises
//               there: this is this project's definition)
// Launches: one memset, candidates (one workgroup per image, box, level: topk rounds of a lexicographic (distance, row)
// arg-min, each round excluding keys not greater than the last one chosen), threshold + vote (one wave per image, box), labels
// (per row); the host reads the per-level counts once; scan_fcos_compact lists the positives in row order and
// scan_atss_targets writes pos_inds, reg_pos = BoxCoder.encode(matched box, anchor) (weights 10, 10, 5, 5) and ctr_pos = the
// centerness of decode(encode(...)) against the anchor centre (loss.py:360-373, the round trip kept), both formed in fp64
// and rounded to fp32 once.
//
// GIoU: min / max with equal arguments send the gradient to their FIRST argument (the prediction's corner in the
// intersection / enclosure terms, x1 in x2 = max(x1, x2)); a delta exactly at the log(1000 / 16) clamp keeps its gradient.
// The forward's sums end in block_result<ORD>; the ordered twin's second stage is ordered_sum_launch (losses.hip).
//
// Per-level selects, the level search, the pyramid check and the wave reductions are common.h's; boxlist_iou is boxes.h's.
#include "common.h"
#include "boxes.h"

#define ATSS_MAX_TOPK 64
#define ATSS_BBOX_CLIP 4.135166556742356f  // log(1000 / 16), atss.py:84-85

struct AtssLevels {
  int stride[SCAN_MAX_LEVELS];
  float c0[SCAN_MAX_LEVELS];    // (s - 1) / 2
  float half[SCAN_MAX_LEVELS];  // (a - 1) / 2
};

static int atss_levels(AtssLevels* lv, const scan_pyramid_t* d, const int32_t* strides, const float* sizes, const char* who) {
  for (int l = 0; l < SCAN_MAX_LEVELS; ++l) {
    if (l < d->n_levels) {
      SCAN_CHECK_ARG(strides[l] >= 1 && sizes[l] >= 1.f, "%s: level %d has stride %d, anchor size %g", who, l, strides[l],
                     (double)sizes[l]);
      lv->stride[l] = strides[l];
      lv->c0[l] = (float)((double)(strides[l] - 1) * 0.5);
      lv->half[l] = (float)(((double)sizes[l] - 1.0) * 0.5);
    } else {
      lv->stride[l] = 1;
      lv->c0[l] = lv->half[l] = 0.f;
    }
  }
  return 0;
}

struct AtssLevel {
  int s;
  float c0, half;
};
__device__ __forceinline__ AtssLevel atss_level(const AtssLevels& lv, int l) {
  return {pick_level(lv.stride, l), pick_level(lv.c0, l), pick_level(lv.half, l)};
}

// anchor of cell (y, x): centre and corners (xyxy)
struct Anchor {
  float cx, cy, x1, y1, x2, y2;
  __device__ __forceinline__ float4 box() const { return make_float4(x1, y1, x2, y2); }
};
__device__ __forceinline__ Anchor anchor_of(const AtssLevel lv, int y, int x) {
  Anchor a;
  a.cx = (float)(x * lv.s) + lv.c0;
  a.cy = (float)(y * lv.s) + lv.c0;
  a.x1 = a.cx - lv.half;
  a.y1 = a.cy - lv.half;
  a.x2 = a.cx + lv.half;
  a.y2 = a.cy + lv.half;
  return a;
}

// grid (n_levels, G, N).  cand_row / cand_iou [N][G][n_levels][topk]; unused slots: row -1
__global__ __launch_bounds__(256) void atss_candidates_kernel(scan_pyramid_t d, AtssLevels lvs, const float* __restrict__ boxes,
                                                              const int32_t* __restrict__ ng, int G, int topk,
                                                              int32_t* __restrict__ cand_row, float* __restrict__ cand_iou) {
  __shared__ unsigned long long wmin[4];
  __shared__ unsigned long long chosen;
  const int l = blockIdx.x, g = blockIdx.y, n = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int64_t slot0 = (((int64_t)n * G + g) * d.n_levels + l) * topk;
  if (g >= ng[n]) {
    if (tid < topk) cand_row[slot0 + tid] = -1;
    return;
  }
  const AtssLevel lv = atss_level(lvs, l);
  const int H = pick_level(d.h, l), W = pick_level(d.w, l), hw = H * W;
  const int64_t row0 = pick_level(d.row_off, l) + (int64_t)n * hw;
  const float4 b = *reinterpret_cast<const float4*>(boxes + ((int64_t)n * G + g) * 4);
  const float gcx = (b.z + b.x) / 2.0f, gcy = (b.w + b.y) / 2.0f;
  const int k = topk < hw ? topk : hw;
  unsigned long long last = 0ull;
  for (int round = 0; round < k; ++round) {
    unsigned long long best = ~0ull;
    int y = tid / W, x = tid - y * W;
    const int dy256 = 256 / W, dx256 = 256 - dy256 * W;
    for (int i = tid; i < hw; i += 256) {
      const float ddx = ((float)(x * lv.s) + lv.c0) - gcx, ddy = ((float)(y * lv.s) + lv.c0) - gcy;
      const float dist = sqrtf(ddx * ddx + ddy * ddy);
      const unsigned long long key = ((unsigned long long)__float_as_uint(dist) << 32) | (unsigned)i;
      if ((round == 0 || key > last) && key < best) best = key;
      x += dx256;
      y += dy256;
      if (x >= W) {
        x -= W;
        ++y;
      }
    }
    best = wave_min_u64(best);
    if (lane == 0) wmin[wid] = best;
    __syncthreads();
    if (tid == 0) {
      unsigned long long m = wmin[0];
      for (int w2 = 1; w2 < 4; ++w2) m = wmin[w2] < m ? wmin[w2] : m;
      chosen = m;
      const int i = (int)(m & 0xffffffffull);
      const int yy = i / W, xx = i - yy * W;
      cand_row[slot0 + round] = (int32_t)(row0 + i);
      cand_iou[slot0 + round] = boxlist_iou(anchor_of(lv, yy, xx).box(), b);
    }
    __syncthreads();
    last = chosen;
  }
  if (tid >= k && tid < topk) cand_row[slot0 + tid] = -1;
}

// one wave per (image, box): threshold, then the positives vote on their rows
__global__ __launch_bounds__(64) void atss_vote_kernel(scan_pyramid_t d, AtssLevels lvs, const float* __restrict__ boxes,
                                                       const int32_t* __restrict__ ng, int G, int topk,
                                                       const int32_t* __restrict__ cand_row,
                                                       const float* __restrict__ cand_iou,
                                                       unsigned long long* __restrict__ row_key) {
  __shared__ float thr_s;
  const int g = blockIdx.x, n = blockIdx.y, lane = threadIdx.x;
  if (g >= ng[n]) return;
  const int nc = d.n_levels * topk;
  const int64_t slot0 = ((int64_t)n * G + g) * nc;
  if (lane == 0) {
    double sum = 0.0;
    int cnt = 0;
    for (int c = 0; c < nc; ++c)
      if (cand_row[slot0 + c] >= 0) {
        sum += (double)cand_iou[slot0 + c];
        ++cnt;
      }
    const double mean = sum / (double)cnt;
    double ss = 0.0;
    for (int c = 0; c < nc; ++c)
      if (cand_row[slot0 + c] >= 0) {
        const double e = (double)cand_iou[slot0 + c] - mean;
        ss += e * e;
      }
    thr_s = cnt > 1 ? (float)(mean + sqrt(ss / (double)(cnt - 1))) : __uint_as_float(0x7fc00000u);
  }
  __syncthreads();
  const float thr = thr_s;
  const float4 b = *reinterpret_cast<const float4*>(boxes + ((int64_t)n * G + g) * 4);
  for (int c = lane; c < nc; c += 64) {
    const int64_t row = cand_row[slot0 + c];
    if (row < 0) continue;
    const float iou = cand_iou[slot0 + c];
    const int l = c / topk;
    const AtssLevel lv = atss_level(lvs, l);
    const int W = pick_level(d.w, l), hw = pick_level(d.h, l) * W;
    const int i = (int)(row - pick_level(d.row_off, l) - (int64_t)n * hw);
    const int y = i / W, x = i - y * W;
    const float cx = (float)(x * lv.s) + lv.c0, cy = (float)(y * lv.s) + lv.c0;
    const float mn = fminf(fminf(cx - b.x, cy - b.y), fminf(b.z - cx, b.w - cy));
    if (iou >= thr && mn > 0.01f)
      atomicMax(&row_key[row], ((unsigned long long)__float_as_uint(iou) << 32) | (unsigned long long)(0xffffffffu - (unsigned)g));
  }
}

__global__ __launch_bounds__(256) void atss_labels_kernel(scan_pyramid_t d, const unsigned long long* __restrict__ row_key,
                                                          const int64_t* __restrict__ glabels, int G,
                                                          int64_t* __restrict__ labels, int32_t* __restrict__ labels_i32,
                                                          int32_t* __restrict__ matched, int32_t* __restrict__ level_pos) {
  const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= d.row_off[d.n_levels]) return;
  const unsigned long long key = row_key[m];
  int64_t lab = 0;
  int g = 0;
  if (key != 0ull) {
    const RowCoord rc = decode_row(d, m);
    g = (int)(0xffffffffu - (unsigned)(key & 0xffffffffull));
    lab = glabels[(int64_t)rc.n * G + g];
    if (lab > 0)
      atomicAdd(&level_pos[rc.lvl], 1);
    else
      g = 0;
  }
  labels[m] = lab;
  labels_i32[m] = (int32_t)lab;
  matched[m] = g;
}

struct AtssPosTab {
  int pos_off[SCAN_MAX_LEVELS + 1];
};

// BoxCoder.decode (atss.py:68-97), one box
__device__ __forceinline__ float4 atss_decode(const float4 t, const Anchor a) {
  const float w = a.x2 - a.x1 + 1.f, h = a.y2 - a.y1 + 1.f;
  const float cx = (a.x2 + a.x1) / 2.f, cy = (a.y2 + a.y1) / 2.f;
  const float dx = t.x / 10.f, dy = t.y / 10.f;
  const float dw = fminf(t.z / 5.f, ATSS_BBOX_CLIP), dh = fminf(t.w / 5.f, ATSS_BBOX_CLIP);
  const float pcx = dx * w + cx, pcy = dy * h + cy;
  const float pw = expf(dw) * w, ph = expf(dh) * h;
  return make_float4(pcx - 0.5f * (pw - 1.f), pcy - 0.5f * (ph - 1.f), pcx + 0.5f * (pw - 1.f), pcy + 0.5f * (ph - 1.f));
}

__global__ __launch_bounds__(256) void atss_targets_kernel(scan_pyramid_t d, AtssLevels lvs, AtssPosTab t,
                                                           const float* __restrict__ boxes, int G,
                                                           const int32_t* __restrict__ matched,
                                                           const int32_t* __restrict__ pos_list,
                                                           int64_t* __restrict__ pos_inds, float* __restrict__ reg_pos,
                                                           float* __restrict__ ctr_pos) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= t.pos_off[d.n_levels]) return;
  const int l = level_of(t.pos_off, d.n_levels, p);
  const int64_t row = pos_list[pick_level(d.row_off, l) + (p - t.pos_off[l])];
  const RowCoord rc = decode_row(d, row);
  const Anchor a = anchor_of(atss_level(lvs, rc.lvl), rc.y, rc.x);
  const float4 b = *reinterpret_cast<const float4*>(boxes + ((int64_t)rc.n * G + matched[row]) * 4);
  // BoxCoder.encode (atss.py:33-50) and compute_centerness_targets (loss.py:360-373: l, t, r, b of decode(encode(..)) against
  // the anchor centre) in fp64, each result rounded to fp32 once.  The round trip subtracts the anchor centre from a corner
  // that was rounded at the magnitude of the coordinate; in fp32 that costs an ulp of the coordinate in a distance that may
  // be a tenth of a pixel (a positive needs only min(l, t, r, b) > 0.01), i.e. 1e-4 of the centerness.  A few thousand
  // positives: the fp64 log / exp cost nothing here.
  const double ew = (double)a.x2 - (double)a.x1 + 1.0, eh = (double)a.y2 - (double)a.y1 + 1.0;
  const double ecx = ((double)a.x2 + (double)a.x1) / 2.0, ecy = ((double)a.y2 + (double)a.y1) / 2.0;
  const double gw = (double)b.z - (double)b.x + 1.0, gh = (double)b.w - (double)b.y + 1.0;
  const double gcx = ((double)b.z + (double)b.x) / 2.0, gcy = ((double)b.w + (double)b.y) / 2.0;
  const double tx = 10.0 * (gcx - ecx) / ew, ty = 10.0 * (gcy - ecy) / eh, tw = 5.0 * log(gw / ew), th = 5.0 * log(gh / eh);
  pos_inds[p] = row;
  *reinterpret_cast<float4*>(reg_pos + 4 * (int64_t)p) = make_float4((float)tx, (float)ty, (float)tw, (float)th);
  const double clip = 4.135166556742356;  // log(1000 / 16)
  const double pcx = tx / 10.0 * ew + ecx, pcy = ty / 10.0 * eh + ecy;
  const double pw = exp(fmin(tw / 5.0, clip)) * ew, ph = exp(fmin(th / 5.0, clip)) * eh;
  const double cl = ecx - (pcx - 0.5 * (pw - 1.0)), cr = (pcx + 0.5 * (pw - 1.0)) - ecx;
  const double ct = ecy - (pcy - 0.5 * (ph - 1.0)), cb = (pcy + 0.5 * (ph - 1.0)) - ecy;
  ctr_pos[p] = (float)sqrt((fmin(cl, cr) / fmax(cl, cr)) * (fmin(ct, cb) / fmax(ct, cb)));
}

// the shared check, and row indices that fit the int32 lists (candidates, scan_fcos_compact's positives)
static int atss_check(const scan_pyramid_t* d, const char* who) {
  if (scan_check_pyramid(d, who)) return -1;
  SCAN_CHECK_ARG(d->row_off[d->n_levels] < (1ll << 31), "%s: more than 2^31 rows", who);
  return 0;
}

extern "C" int64_t scan_atss_assign_ws_bytes(const scan_pyramid_t* d, int32_t G, int32_t topk) {
  if (!d || d->n_levels < 1 || d->n_levels > SCAN_MAX_LEVELS || d->n_images < 1 || G < 1 || topk < 1 || topk > ATSS_MAX_TOPK)
    return -1;
  const int64_t cands = (int64_t)d->n_images * G * d->n_levels * topk;
  return 8 * d->row_off[d->n_levels] + 8 * cands;  // row keys, candidate rows, candidate IoUs
}

extern "C" int scan_atss_assign(const scan_pyramid_t* d, const int32_t* strides, const float* anchor_sizes, const float* boxes,
                                const int64_t* glabels, const int32_t* ng, int32_t G, int32_t topk, int64_t* labels,
                                int32_t* labels_i32, int32_t* matched, int32_t* level_pos, void* ws, void* stream) {
  if (atss_check(d, "atss_assign")) return -1;
  SCAN_CHECK_ARG(strides && anchor_sizes && boxes && glabels && ng && labels && labels_i32 && matched && level_pos && ws,
                 "atss_assign: null pointer");
  SCAN_CHECK_ARG(G >= 1 && G <= 65535 && d->n_images <= 65535, "atss_assign: G=%d / N=%d outside 1..65535", G, d->n_images);
  SCAN_CHECK_ARG(topk >= 1 && topk <= ATSS_MAX_TOPK, "atss_assign: topk=%d outside 1..%d", topk, ATSS_MAX_TOPK);
  SCAN_CHECK_ARG((reinterpret_cast<uintptr_t>(boxes) & 15) == 0 && (reinterpret_cast<uintptr_t>(ws) & 7) == 0,
                 "atss_assign: boxes must be 16-byte, ws 8-byte aligned");
  AtssLevels lv;
  if (atss_levels(&lv, d, strides, anchor_sizes, "atss_assign")) return -1;
  hipStream_t st = as_stream(stream);
  const int64_t M = d->row_off[d->n_levels];
  const int64_t cands = (int64_t)d->n_images * G * d->n_levels * topk;
  unsigned long long* row_key = reinterpret_cast<unsigned long long*>(ws);
  int32_t* cand_row = reinterpret_cast<int32_t*>(row_key + M);
  float* cand_iou = reinterpret_cast<float*>(cand_row + cands);
  if (hipMemsetAsync(row_key, 0, 8 * M, st) != hipSuccess ||
      hipMemsetAsync(level_pos, 0, sizeof(int32_t) * SCAN_MAX_LEVELS, st) != hipSuccess) {
    scan_set_error("atss_assign: memset failed");
    return -2;
  }
  hipLaunchKernelGGL(atss_candidates_kernel, dim3(d->n_levels, G, d->n_images), dim3(256), 0, st, *d, lv, boxes, ng, G, topk,
                     cand_row, cand_iou);
  SCAN_LAUNCH_CHECK("atss_candidates");
  hipLaunchKernelGGL(atss_vote_kernel, dim3(G, d->n_images), dim3(64), 0, st, *d, lv, boxes, ng, G, topk, cand_row, cand_iou,
                     row_key);
  SCAN_LAUNCH_CHECK("atss_vote");
  hipLaunchKernelGGL(atss_labels_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, st, *d, row_key, glabels, G, labels,
                     labels_i32, matched, level_pos);
  SCAN_LAUNCH_CHECK("atss_labels");
  return 0;
}

extern "C" int scan_atss_targets(const scan_pyramid_t* d, const int32_t* strides, const float* anchor_sizes,
                                 const int32_t* level_pos, const float* boxes, int32_t G, const int32_t* matched,
                                 const int32_t* pos_list, int64_t* pos_inds, float* reg_pos, float* ctr_pos, void* stream) {
  if (atss_check(d, "atss_targets")) return -1;
  SCAN_CHECK_ARG(strides && anchor_sizes && level_pos && boxes && matched && pos_list && G >= 1,
                 "atss_targets: null pointer or G < 1");
  AtssLevels lv;
  if (atss_levels(&lv, d, strides, anchor_sizes, "atss_targets")) return -1;
  AtssPosTab t;
  t.pos_off[0] = 0;
  for (int l = 0; l < SCAN_MAX_LEVELS; ++l) {
    int np = 0;
    if (l < d->n_levels) {
      np = level_pos[l];
      SCAN_CHECK_ARG(np >= 0 && np <= d->row_off[l + 1] - d->row_off[l], "atss_targets: level %d has %d positives of %lld rows",
                     l, np, (long long)(d->row_off[l + 1] - d->row_off[l]));
    }
    t.pos_off[l + 1] = t.pos_off[l] + np;
  }
  const int total = t.pos_off[d->n_levels];
  if (total == 0) return 0;
  SCAN_CHECK_ARG(pos_inds && reg_pos && ctr_pos, "atss_targets: null output");
  hipLaunchKernelGGL(atss_targets_kernel, dim3((total + 255) / 256), dim3(256), 0, as_stream(stream), *d, lv, t, boxes, G,
                     matched, pos_list, pos_inds, reg_pos, ctr_pos);
  SCAN_LAUNCH_CHECK("atss_targets");
  return 0;
}

// ------------------------------------------------------------------ GIoU loss on anchor deltas (loss.py:64-105)
struct GiouTerms {
  float loss;
  float4 pb, tb;       // decoded prediction (after x2 = max(x1, x2)) and target boxes
  float pw, ph;        // exp(dw) * w, exp(dh) * h of the prediction
  float aw, ah;        // anchor widths (+1)
  bool swap_x, swap_y; // the max(x1, x2) took x1
  float I, U, E;
};

__device__ __forceinline__ GiouTerms giou_terms(const float4 p, const float4 t, const Anchor a) {
  GiouTerms r;
  r.aw = a.x2 - a.x1 + 1.f;
  r.ah = a.y2 - a.y1 + 1.f;
  const float cx = (a.x2 + a.x1) / 2.f, cy = (a.y2 + a.y1) / 2.f;
  const float dw = fminf(p.z / 5.f, ATSS_BBOX_CLIP), dh = fminf(p.w / 5.f, ATSS_BBOX_CLIP);
  const float pcx = (p.x / 10.f) * r.aw + cx, pcy = (p.y / 10.f) * r.ah + cy;
  r.pw = expf(dw) * r.aw;
  r.ph = expf(dh) * r.ah;
  float4 pb = make_float4(pcx - 0.5f * (r.pw - 1.f), pcy - 0.5f * (r.ph - 1.f), pcx + 0.5f * (r.pw - 1.f),
                          pcy + 0.5f * (r.ph - 1.f));
  r.swap_x = !(pb.z > pb.x);
  r.swap_y = !(pb.w > pb.y);
  if (r.swap_x) pb.z = pb.x;
  if (r.swap_y) pb.w = pb.y;
  r.pb = pb;
  r.tb = atss_decode(t, a);
  const float pa = (pb.z - pb.x) * (pb.w - pb.y);
  const float ta = (r.tb.z - r.tb.x) * (r.tb.w - r.tb.y);
  const float ix1 = fmaxf(pb.x, r.tb.x), iy1 = fmaxf(pb.y, r.tb.y), ix2 = fminf(pb.z, r.tb.z), iy2 = fminf(pb.w, r.tb.w);
  r.I = (iy2 > iy1 && ix2 > ix1) ? (ix2 - ix1) * (iy2 - iy1) : 0.f;
  const float ex1 = fminf(pb.x, r.tb.x), ey1 = fminf(pb.y, r.tb.y), ex2 = fmaxf(pb.z, r.tb.z), ey2 = fmaxf(pb.w, r.tb.w);
  r.E = (ex2 - ex1) * (ey2 - ey1) + 1e-7f;
  r.U = pa + ta - r.I + 1e-7f;
  const float iou = r.I / r.U;
  const float giou = iou - (r.E - r.U) / r.E;
  r.loss = 1.f - giou;
  return r;
}

__device__ __forceinline__ Anchor anchor_of_row(const scan_pyramid_t& d, const AtssLevels& lvs, int64_t row) {
  const RowCoord rc = decode_row(d, row);
  return anchor_of(atss_level(lvs, rc.lvl), rc.y, rc.x);
}

// ORD: every block writes its two sums to its own slots part[2 * block + {0, 1}] instead of adding them to out2
template <bool ORD>
__global__ __launch_bounds__(256) void giou_fwd_kernel(scan_pyramid_t d, AtssLevels lvs, const float* __restrict__ pred,
                                                       const float* __restrict__ target, const int64_t* __restrict__ rows,
                                                       const float* __restrict__ weight, int64_t P, float* __restrict__ out2) {
  __shared__ float red[4];
  float num = 0.f, den = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < P; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 p = reinterpret_cast<const float4*>(pred)[i];
    const float4 t = reinterpret_cast<const float4*>(target)[i];
    const float w = weight[i];
    num += giou_terms(p, t, anchor_of_row(d, lvs, rows[i])).loss * w;
    den += w;
  }
  const float sn = block_sum_256(num, red);
  const float sd = block_sum_256(den, red);
  if (threadIdx.x == 0) {
    block_result<ORD>(out2, 0, 2, sn);
    block_result<ORD>(out2, 1, 2, sd);
  }
}

__global__ __launch_bounds__(256) void giou_bwd_kernel(scan_pyramid_t d, AtssLevels lvs, const float* __restrict__ pred,
                                                       const float* __restrict__ target, const int64_t* __restrict__ rows,
                                                       const float* __restrict__ weight, int64_t P,
                                                       const float* __restrict__ g_num, float* __restrict__ d_pred) {
  const float g = g_num[0];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < P; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 p = reinterpret_cast<const float4*>(pred)[i];
    const float4 t = reinterpret_cast<const float4*>(target)[i];
    const GiouTerms r = giou_terms(p, t, anchor_of_row(d, lvs, rows[i]));
    const float wg = weight[i] * g;
    // loss = 2 - I / U - U / E;  U = pa + ta - I + eps
    const float dU = r.I / (r.U * r.U) - 1.f / r.E;
    const float dI = -1.f / r.U - dU;
    const float dE = r.U / (r.E * r.E);
    const float4 pb = r.pb, tb = r.tb;
    const float pwid = pb.z - pb.x, phei = pb.w - pb.y;
    // gradients with respect to the prediction's corners (after the max): area, intersection, enclosure
    float gx1 = -dU * phei, gx2 = dU * phei, gy1 = -dU * pwid, gy2 = dU * pwid;
    const float ix1 = fmaxf(pb.x, tb.x), iy1 = fmaxf(pb.y, tb.y), ix2 = fminf(pb.z, tb.z), iy2 = fminf(pb.w, tb.w);
    if (iy2 > iy1 && ix2 > ix1) {
      const float iw = ix2 - ix1, ih = iy2 - iy1;
      if (pb.x >= tb.x) gx1 -= dI * ih;
      if (pb.z <= tb.z) gx2 += dI * ih;
      if (pb.y >= tb.y) gy1 -= dI * iw;
      if (pb.w <= tb.w) gy2 += dI * iw;
    }
    const float ew = fmaxf(pb.z, tb.z) - fminf(pb.x, tb.x), eh = fmaxf(pb.w, tb.w) - fminf(pb.y, tb.y);
    if (pb.x <= tb.x) gx1 -= dE * eh;
    if (pb.z >= tb.z) gx2 += dE * eh;
    if (pb.y <= tb.y) gy1 -= dE * ew;
    if (pb.w >= tb.w) gy2 += dE * ew;
    // x2 = max(x1, x2): equal or smaller x2 sends its gradient to x1
    if (r.swap_x) {
      gx1 += gx2;
      gx2 = 0.f;
    }
    if (r.swap_y) {
      gy1 += gy2;
      gy2 = 0.f;
    }
    float4 o;
    o.x = wg * (gx1 + gx2) * r.aw / 10.f;
    o.y = wg * (gy1 + gy2) * r.ah / 10.f;
    o.z = (p.z / 5.f <= ATSS_BBOX_CLIP) ? wg * (gx2 - gx1) * 0.5f * r.pw / 5.f : 0.f;
    o.w = (p.w / 5.f <= ATSS_BBOX_CLIP) ? wg * (gy2 - gy1) * 0.5f * r.ph / 5.f : 0.f;
    reinterpret_cast<float4*>(d_pred)[i] = o;
  }
}

static int giou_check(const scan_pyramid_t* d, const int32_t* strides, const float* sizes, const float* pred,
                      const float* target, const int64_t* rows, const float* weight, AtssLevels* lv, const char* who) {
  if (atss_check(d, who)) return -1;
  SCAN_CHECK_ARG(strides && sizes, "%s: null strides / anchor sizes", who);
  if (atss_levels(lv, d, strides, sizes, who)) return -1;
  SCAN_CHECK_ARG(pred && target && rows && weight, "%s: null input", who);
  SCAN_CHECK_ARG(((reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(target)) & 15) == 0,
                 "%s: pred / target must be 16-byte aligned", who);
  return 0;
}

extern "C" int64_t scan_atss_giou_ordered_ws_floats(int64_t P) { return 2 * (int64_t)head_loss_grid(P); }

// ORD = false: float atomics on out2.  ORD = true: the blocks' sums go to ws [head_loss_grid(P)][2], ordered_sum_launch forms out2
template <bool ORD>
static int giou_forward_launch(const scan_pyramid_t* d, const int32_t* strides, const float* anchor_sizes, const float* pred,
                               const float* target, const int64_t* rows, const float* weight, int64_t P, float* out2, float* ws,
                               void* stream, const char* who) {
  SCAN_CHECK_ARG(P >= 0 && out2, "%s: bad arguments", who);
  if (P == 0) return 0;
  AtssLevels lv;
  if (giou_check(d, strides, anchor_sizes, pred, target, rows, weight, &lv, who)) return -1;
  const int grid = head_loss_grid(P);
  hipLaunchKernelGGL(giou_fwd_kernel<ORD>, dim3(grid), dim3(256), 0, as_stream(stream), *d, lv, pred, target, rows, weight, P,
                     ORD ? ws : out2);
  SCAN_LAUNCH_CHECK(ORD ? "atss_giou_fwd_ordered" : "atss_giou_fwd");
  return ORD ? ordered_sum_launch(ws, grid, 2, out2, 0, nullptr, stream, "atss_giou_fwd_ordered_sum") : 0;
}

extern "C" int scan_atss_giou_forward(const scan_pyramid_t* d, const int32_t* strides, const float* anchor_sizes,
                                      const float* pred, const float* target, const int64_t* rows, const float* weight,
                                      int64_t P, float* out2, void* stream) {
  return giou_forward_launch<false>(d, strides, anchor_sizes, pred, target, rows, weight, P, out2, nullptr, stream, "atss_giou_forward");
}

extern "C" int scan_atss_giou_forward_ordered(const scan_pyramid_t* d, const int32_t* strides, const float* anchor_sizes,
                                              const float* pred, const float* target, const int64_t* rows,
                                              const float* weight, int64_t P, float* out2, float* ws, void* stream) {
  SCAN_CHECK_ARG(ws, "atss_giou_forward_ordered: bad arguments");
  return giou_forward_launch<true>(d, strides, anchor_sizes, pred, target, rows, weight, P, out2, ws, stream, "atss_giou_forward_ordered");
}

extern "C" int scan_atss_giou_backward(const scan_pyramid_t* d, const int32_t* strides, const float* anchor_sizes,
                                       const float* pred, const float* target, const int64_t* rows, const float* weight,
                                       int64_t P, const float* g_num_dev, float* d_pred, void* stream) {
  SCAN_CHECK_ARG(P >= 0, "atss_giou_backward: bad arguments");
  if (P == 0) return 0;
  AtssLevels lv;
  if (giou_check(d, strides, anchor_sizes, pred, target, rows, weight, &lv, "atss_giou_backward")) return -1;
  SCAN_CHECK_ARG(g_num_dev && d_pred && (reinterpret_cast<uintptr_t>(d_pred) & 15) == 0,
                 "atss_giou_backward: null or misaligned gradient pointer");
  hipLaunchKernelGGL(giou_bwd_kernel, dim3(grid_for(P, 256)), dim3(256), 0, as_stream(stream), *d, lv, pred, target, rows, weight,
                     P, g_num_dev, d_pred);
  SCAN_LAUNCH_CHECK("atss_giou_bwd");
  return 0;
}
