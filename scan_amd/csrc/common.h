// Shared helpers for the gfx950 kernels of libscan_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/scan_hip.h"

#define SCAN_WAVE 64

extern "C" void scan_set_error(const char* fmt, ...);

#define SCAN_CHECK_ARG(cond, ...)          \
  do {                                     \
    if (!(cond)) {                         \
      scan_set_error(__VA_ARGS__);         \
      return -1;                           \
    }                                      \
  } while (0)

#define SCAN_LAUNCH_CHECK(name)                                          \
  do {                                                                   \
    hipError_t _e = hipGetLastError();                                   \
    if (_e != hipSuccess) {                                              \
      scan_set_error("%s: launch failed: %s", name, hipGetErrorString(_e)); \
      return -2;                                                         \
    }                                                                    \
  } while (0)

static inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// memory-bound kernels: cap the grid at 256 CUs x 8 blocks and grid-stride the rest
static inline int grid_for(int64_t work_items, int block) {
  int64_t g = (work_items + block - 1) / block;
  if (g < 1) g = 1;
  if (g > 2048) g = 2048;
  return (int)g;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// block-wide sum for blockDim.x == 256 (4 waves); result valid in thread 0
__device__ __forceinline__ float block_sum_256(float v, float* smem4) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) smem4[wid] = v;
  __syncthreads();
  float r = 0.f;
  if (threadIdx.x == 0) r = smem4[0] + smem4[1] + smem4[2] + smem4[3];
  __syncthreads();
  return r;
}

// ------------------------------------------------------------------ pyramid helpers
// a[l] of a per-level table held in kernel arguments, l < SCAN_MAX_LEVELS: an unrolled select, so the table stays in scalar
// registers (a dynamic index would send it through scratch memory).  Tables with a closing entry (row_off) qualify too.
template <typename T, int N>
__device__ __forceinline__ T pick_level(const T (&a)[N], int l) {
  static_assert(N >= SCAN_MAX_LEVELS, "a per-level table");
  T r = a[0];
#pragma unroll
  for (int i = 1; i < SCAN_MAX_LEVELS; ++i)
    if (l == i) r = a[i];
  return r;
}

// the level that holds position p of a prefix table off[0] = 0 <= off[1] <= ... (empty levels take nothing)
template <typename T>
__device__ __forceinline__ int level_of(const T (&off)[SCAN_MAX_LEVELS + 1], int n_levels, T p) {
  int l = 0;
#pragma unroll
  for (int k = 1; k < SCAN_MAX_LEVELS; ++k)
    if (k < n_levels && p >= off[k]) l = k;
  return l;
}

// pyramid row decode: m -> (level, image, y, x)
struct RowCoord {
  int lvl, n, y, x;
};
__device__ __forceinline__ RowCoord decode_row(const scan_pyramid_t& d, int64_t m) {
  RowCoord rc;
  const int l = level_of(d.row_off, d.n_levels, m);
  int64_t r = m - d.row_off[l];
  const int hw = d.h[l] * d.w[l];
  rc.lvl = l;
  rc.n = (int)(r / hw);
  int rem = (int)(r - (int64_t)rc.n * hw);
  rc.y = rem / d.w[l];
  rc.x = rem - rc.y * d.w[l];
  return rc;
}

// Host check of a descriptor before a kernel decodes rows with it: a level whose rows are not n_images * h * w would send
// decode_row's image index past n_images.  Limits of one entry point (a total of 2^31 rows, ...) stay with that entry point.
static inline int scan_check_pyramid(const scan_pyramid_t* d, const char* who) {
  SCAN_CHECK_ARG(d && d->n_levels >= 1 && d->n_levels <= SCAN_MAX_LEVELS && d->n_images >= 1, "%s: bad pyramid", who);
  for (int l = 0; l < d->n_levels; ++l) {
    SCAN_CHECK_ARG(d->h[l] >= 1 && d->w[l] >= 1 &&
                       d->row_off[l + 1] - d->row_off[l] == (int64_t)d->n_images * d->h[l] * d->w[l],
                   "%s: level %d of the pyramid is inconsistent", who, l);
    SCAN_CHECK_ARG((int64_t)d->h[l] * d->w[l] < (1ll << 31), "%s: level %d alone has 2^31 rows or more", who, l);
  }
  return 0;
}

// ------------------------------------------------------------------ wave reductions beside wave_sum
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// maximum over the wave, in every lane (xor butterfly)
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const int o = __shfl_xor(v, off, 64);
    v = o > v ? o : v;
  }
  return v;
}
__device__ __forceinline__ unsigned wave_max(unsigned v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned o = __shfl_xor(v, off, 64);
    v = o > v ? o : v;
  }
  return v;
}

// minimum over the wave, valid in lane 0 (the shuffles move 32 bits: two per step)
__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned lo = __shfl_down((unsigned)(v & 0xffffffffull), off, 64);
    const unsigned hi = __shfl_down((unsigned)(v >> 32), off, 64);
    const unsigned long long o = ((unsigned long long)hi << 32) | lo;
    v = o < v ? o : v;
  }
  return v;
}

// ------------------------------------------------------------------ ordered reductions (scan_tune "deterministic")
// Every reducing kernel ends in one line: the block's partial sum goes to `dst`.  ORD = false (the product default):
// a float atomic on dst[k] -- fastest, but the sum then depends on the order the blocks arrive in.  ORD = true (the *_ordered
// entry points): an ordinary store to the block's own slot dst[blockIdx.x][k] of a caller-supplied workspace, which
// ordered_sum_kernel (losses.hip) -- a launch of its own behind the kernel -- adds up in a fixed order.  A second launch, not
// the last-arriving block: stream order makes every slot visible to it with no fence, ticket or device-scope read-back (the
// per-XCD L2s are not coherent: a last block would have to read 2,048 slots back past its own L2), and no block ever
// depends on another.
template <bool ORD>
__device__ __forceinline__ void block_result(float* __restrict__ dst, int k, int ncols, float v) {
  if (ORD) dst[(int64_t)blockIdx.x * ncols + k] = v;
  else atomicAdd(dst + k, v);
}

// the second stage: out[k] = the sum of part[b][k] over the nblk blocks' slots, k < ncols, in one fixed order (one launch;
// defined beside ordered_sum_kernel in losses.hip, internal to the library).  Cf / fin: the CKA loss, nullptr elsewhere.
__attribute__((visibility("hidden"))) int ordered_sum_launch(const float* part, int nblk, int ncols, float* out, int Cf,
                                                             float* fin, void* stream, const char* who);

// the grid of the heads' loss forwards (GIoU, smooth-L1): one block per 2,048 items, at most 256 -- a function of the item
// count alone, so the ordered sum is too
static inline int head_loss_grid(int64_t items) {
  int64_t g = (items + 2047) / 2048;
  return (int)(g < 1 ? 1 : (g > 256 ? 256 : g));
}
