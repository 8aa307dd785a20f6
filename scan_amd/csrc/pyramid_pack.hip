// Pyramid pack / unpack: per-level [N, C, H_l, W_l] tensors of any element strides <-> the [M, Cs] row matrix the engine runs on
// (rows in level -> image -> y -> x order), all levels in ONE launch.  The reference flattens and concatenates level by level
// in front of every loss (rpn/fcos/loss.py:191-202: permute(0, 2, 3, 1).reshape(-1, C) per level, then torch.cat); a backbone
// that is not ours hands over level lists in whatever layout it likes, and this is the one pass that brings them in (and, as
// the adjoint, takes the row gradient back out).
//
// One workgroup of 256 threads moves one tile of 64 pixels x 64 channels; tiles are numbered level by level and a workgroup
// finds its level by a uniform search over at most 8 tile offsets.  Per level one of three paths (chosen on the host):
//   rows4   channel stride 1, C % 4 == 0, base and strides 16-byte aligned: a pixel's channels are contiguous on both sides,
//           float4 copies, no LDS
//   rows1   channel stride 1 otherwise: the same with scalar accesses
//   lds     any other strides (NCHW-contiguous: x stride 1): the tile goes through LDS as [channel][pixel] with a row pitch
//           of 65 floats -- the side whose lanes run along the pixels and the side whose lanes run along the channels both
//           touch 32 different banks per 32-lane half, and both global accesses have lanes on consecutive addresses
// Every element of the destination is written exactly once (pack: padding columns C..Cs-1 as zeros), nothing is accumulated,
// no workgroup depends on another.  All global offsets are 64-bit.
#include "common.h"

namespace {

enum { PATH_LDS = 0, PATH_ROWS1 = 1, PATH_ROWS4 = 2 };
constexpr int TILE = 64;
constexpr int PITCH = TILE + 1;

struct PackArgs {
  int32_t n_levels, n_images, C, Cs;
  int32_t ctiles;  // channel tiles per pixel tile: ceil(Cs / 64) packing (the zero padding is written), ceil(C / 64) unpacking
  int32_t reserved;
  int64_t tile_off[SCAN_PACK_MAX_LEVELS + 1];
  int64_t row_off[SCAN_PACK_MAX_LEVELS];
  float* ptr[SCAN_PACK_MAX_LEVELS];
  int64_t sn[SCAN_PACK_MAX_LEVELS], sc[SCAN_PACK_MAX_LEVELS], sy[SCAN_PACK_MAX_LEVELS], sx[SCAN_PACK_MAX_LEVELS];
  int32_t h[SCAN_PACK_MAX_LEVELS], w[SCAN_PACK_MAX_LEVELS];
  int32_t path[SCAN_PACK_MAX_LEVELS];
};

template <bool PACK>
__global__ __launch_bounds__(256) void pyramid_pack_kernel(PackArgs a, float* __restrict__ rows) {
  __shared__ float tile[TILE * PITCH];
  __shared__ int64_t poff[TILE];  // element offset of the tile's 64 pixels in the level tensor (-1: past the level's end)
  const int tid = threadIdx.x;
  const int64_t t = blockIdx.x;
  int lvl = 0;
#pragma unroll
  for (int i = 1; i < SCAN_PACK_MAX_LEVELS; ++i)
    if (i < a.n_levels && t >= a.tile_off[i]) lvl = i;
  const int64_t tl = t - a.tile_off[lvl];
  const int64_t pt = tl / a.ctiles;
  const int c0 = (int)(tl - pt * a.ctiles) * TILE;
  const int C = a.C, Cs = a.Cs;
  const int64_t p0 = pt * TILE;
  const int64_t hw = (int64_t)a.h[lvl] * a.w[lvl];
  const int64_t P = hw * a.n_images;
  float* __restrict__ lev = a.ptr[lvl];
  const int64_t sc = a.sc[lvl];
  float* __restrict__ rt = rows + (a.row_off[lvl] + p0) * (int64_t)Cs + c0;  // element (pixel 0, channel c0) of the tile in the row matrix
  if (tid < TILE) {
    const int64_t p = p0 + tid;
    int64_t off = -1;
    if (p < P) {
      const int64_t n = p / hw;
      const int r = (int)(p - n * hw);
      const int y = r / a.w[lvl];
      const int x = r - y * a.w[lvl];
      off = n * a.sn[lvl] + y * a.sy[lvl] + x * a.sx[lvl];
    }
    poff[tid] = off;
  }
  __syncthreads();
  const int path = a.path[lvl];
  if (path == PATH_ROWS4) {
    const int q = (tid & 15) * 4, pg = tid >> 4;
    const int cc = c0 + q;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int px = pg + 16 * i;
      const int64_t off = poff[px];
      if (off < 0) continue;
      if (PACK) {
        if (cc < Cs) {
          float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
          if (cc < C) v = *reinterpret_cast<const float4*>(lev + off + cc);
          *reinterpret_cast<float4*>(rt + (int64_t)px * Cs + q) = v;
        }
      } else if (cc < C) {
        *reinterpret_cast<float4*>(lev + off + cc) = *reinterpret_cast<const float4*>(rt + (int64_t)px * Cs + q);
      }
    }
    return;
  }
  if (path == PATH_ROWS1) {
    const int c = tid & 63, pg = tid >> 6;
    const int cc = c0 + c;
#pragma unroll 4
    for (int i = 0; i < 16; ++i) {
      const int px = pg + 4 * i;
      const int64_t off = poff[px];
      if (off < 0) continue;
      if (PACK) {
        if (cc < Cs) rt[(int64_t)px * Cs + c] = cc < C ? lev[off + cc] : 0.f;
      } else if (cc < C) {
        lev[off + cc] = rt[(int64_t)px * Cs + c];
      }
    }
    return;
  }
  // lds: lane index l runs along the pixels on the level side and along the channels on the row side
  const int l = tid & 63, g = tid >> 6;
  if (PACK) {
    const int64_t off = poff[l];
#pragma unroll 4
    for (int i = 0; i < 16; ++i) {
      const int c = g + 4 * i;
      tile[c * PITCH + l] = (off >= 0 && c0 + c < C) ? lev[off + (int64_t)(c0 + c) * sc] : 0.f;
    }
    __syncthreads();
    if (c0 + l < Cs) {
#pragma unroll 4
      for (int i = 0; i < 16; ++i) {
        const int px = g + 4 * i;
        if (poff[px] >= 0) rt[(int64_t)px * Cs + l] = tile[l * PITCH + px];
      }
    }
  } else {
    if (c0 + l < C) {
#pragma unroll 4
      for (int i = 0; i < 16; ++i) {
        const int px = g + 4 * i;
        if (poff[px] >= 0) tile[l * PITCH + px] = rt[(int64_t)px * Cs + l];
      }
    }
    __syncthreads();
    const int64_t off = poff[l];
    if (off >= 0) {
#pragma unroll 4
      for (int i = 0; i < 16; ++i) {
        const int c = g + 4 * i;
        if (c0 + c < C) lev[off + (int64_t)(c0 + c) * sc] = tile[c * PITCH + l];
      }
    }
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <bool PACK>
int launch(const char* name, const scan_level_t* levels, int32_t n_levels, int32_t n_images, int32_t C, float* rows, int32_t Cs,
           void* stream) {
  SCAN_CHECK_ARG(n_levels >= 1 && n_levels <= SCAN_PACK_MAX_LEVELS, "%s: n_levels=%d, must be in [1, %d]", name, n_levels,
                 SCAN_PACK_MAX_LEVELS);
  SCAN_CHECK_ARG(n_images >= 1 && C >= 1, "%s: n_images=%d C=%d must be >= 1", name, n_images, C);
  SCAN_CHECK_ARG(Cs >= C && Cs % 4 == 0, "%s: Cs=%d must be a multiple of 4 and >= C=%d", name, Cs, C);
  SCAN_CHECK_ARG(levels && rows, "%s: null pointer", name);
  PackArgs a;
  a.n_levels = n_levels, a.n_images = n_images, a.C = C, a.Cs = Cs, a.reserved = 0;
  a.ctiles = ((PACK ? Cs : C) + TILE - 1) / TILE;
  int64_t tiles = 0, row = 0;
  for (int l = 0; l < SCAN_PACK_MAX_LEVELS; ++l) {
    if (l >= n_levels) {  // unused entries: never selected by the level search (i < n_levels), filled for a defined argument block
      a.tile_off[l + 1] = tiles, a.row_off[l] = row, a.ptr[l] = nullptr;
      a.sn[l] = a.sc[l] = a.sy[l] = a.sx[l] = 0, a.h[l] = a.w[l] = 1, a.path[l] = PATH_ROWS1;
      continue;
    }
    const scan_level_t& v = levels[l];
    SCAN_CHECK_ARG(v.data, "%s: level %d: null pointer", name, l);
    SCAN_CHECK_ARG(v.h >= 1 && v.w >= 1, "%s: level %d: h=%d w=%d must be >= 1", name, l, v.h, v.w);
    SCAN_CHECK_ARG(v.sn >= 0 && v.sc >= 0 && v.sy >= 0 && v.sx >= 0, "%s: level %d: negative stride", name, l);
    const int64_t P = (int64_t)n_images * v.h * v.w;
    a.tile_off[l] = tiles, a.row_off[l] = row, a.ptr[l] = const_cast<float*>(v.data);
    a.sn[l] = v.sn, a.sc[l] = v.sc, a.sy[l] = v.sy, a.sx[l] = v.sx, a.h[l] = v.h, a.w[l] = v.w;
    if (v.sc != 1 && C > 1)
      a.path[l] = PATH_LDS;
    else if (C % 4 == 0 && aligned16(v.data) && aligned16(rows) && v.sn % 4 == 0 && v.sy % 4 == 0 && v.sx % 4 == 0)
      a.path[l] = PATH_ROWS4;
    else
      a.path[l] = PATH_ROWS1;
    tiles += (P + TILE - 1) / TILE * a.ctiles;
    row += P;
    a.tile_off[l + 1] = tiles;
  }
  SCAN_CHECK_ARG(tiles <= 0x7fffffffLL, "%s: %lld tiles exceed one grid", name, (long long)tiles);
  hipLaunchKernelGGL(pyramid_pack_kernel<PACK>, dim3((unsigned)tiles), dim3(256), 0, as_stream(stream), a, rows);
  SCAN_LAUNCH_CHECK(name);
  return 0;
}

}  // namespace

extern "C" int scan_pyramid_pack(const scan_level_t* levels, int32_t n_levels, int32_t n_images, int32_t C, float* rows,
                                 int32_t Cs, void* stream) {
  return launch<true>("pyramid_pack", levels, n_levels, n_images, C, rows, Cs, stream);
}

extern "C" int scan_pyramid_unpack(const float* rows, int32_t Cs, const scan_level_t* levels, int32_t n_levels,
                                   int32_t n_images, int32_t C, void* stream) {
  return launch<false>("pyramid_unpack", levels, n_levels, n_images, C, const_cast<float*>(rows), Cs, stream);
}
