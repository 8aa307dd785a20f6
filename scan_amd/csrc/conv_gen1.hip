// The FIRST generation of the split-operand forward / data-gradient kernel (two pieces, "bf16x3"), kept as an INDEPENDENT
// implementation the tests compare the production kernel (conv_fwd.hip) against: scan_tune("conv_v2", 0) routes the two-piece
// launches here, and so does a two-piece call whose output the production kernel's 16-byte stores cannot take (conv_api.hip).
// Nothing in the default path reaches this file.
//
// v_mfma_f32_32x32x16_bf16, another tile / fragment / LDS layout than the production kernel.  Structure (per 512-thread
// workgroup, one workgroup per CU: 95 KB of LDS):
//   output tile   16 x 16 pixels (one image, one pyramid level) x BN = 128 or 256 output channels
//                 (8 x 16 pixels x 64 channels with 256 threads for Cout <= 64)
//   K loop        input channels in chunks of 32; per chunk the 18 x 18 x 32 input HALO patch is read from HBM/L2 ONCE
//                 as fp32, split to bf16 hi/lo while being written to LDS, and then reused by all 9 taps
//   weights       pre-split once per step into bf16 planes [O][9][Csw] (scan_weight_split), staged per (chunk, tap)
//                 through a double-buffered LDS tile
//   waves         4 x 2, each 64 pixels x 64 (BN = 256: 128) channels = 2 x 2 (2 x 4) MFMA tiles of 32x32
// LDS pixel rows are 80 B (64 B of data + 16 B pad) and patch rows 1536 B so the 16-byte fragment reads of consecutive
// pixels / channels fall on distinct bank groups.
#include "conv_launch.h"
#include "conv_split.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

#define SCAN_MMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0)

#define TW CONV_TILE_W
#define PW (TW + 2)
#define CK 32             // channels per K chunk
#define LROW 40           // bf16 elements per LDS row (32 data + 8 pad = 80 B)
#define PPITCH 768        // bf16 elements per halo-patch ROW of 18 pixels: 1440 B of data padded to 1536 B, so a
                          // fragment read that spans two tile rows (lanes 0-15 / 16-31) stays on 16 distinct
                          // 16-byte slots (5 * pixel mod 16 is a bijection only if the row step is 0 mod 16 slots)

// hi / lo pieces of four values, element by element.  (conv_split.h's split4_np<2> gives the same pieces from packed
// conversions, but other instructions: this kernel's code is kept as it was measured and cross-checked.)
__device__ __forceinline__ void split4(const float4 v, bf16x4& hi, bf16x4& lo) {
  hi[0] = (__bf16)v.x;
  hi[1] = (__bf16)v.y;
  hi[2] = (__bf16)v.z;
  hi[3] = (__bf16)v.w;
  lo[0] = (__bf16)(v.x - (float)hi[0]);
  lo[1] = (__bf16)(v.y - (float)hi[1]);
  lo[2] = (__bf16)(v.z - (float)hi[2]);
  lo[3] = (__bf16)(v.w - (float)hi[3]);
}

// BN: output channels per workgroup; TH: tile height in pixels (tile = TH x 16); NT: threads (TH * 32);
// KS: 3 (3x3, pad 1, stride 1) or 1 (1x1: no halo, one tap).  The 1x1 instance also serves the stride-2 1x1 convs of
// the ResNet bottlenecks through MAP: 0 source pixel = output pixel (same pyramid), 1 source = 2 * output (forward of
// a stride-2 conv, source pyramid sd is the finer one), 2 source = output / 2 where both coordinates are even, zero
// elsewhere (its data gradient: sd is the coarser dY pyramid).
template <int BN, int TH, int NT, int KS = 3>
__global__ __launch_bounds__(NT, NT == 512 ? 2 : 3) void conv3x3_bf16x3_kernel(
    const float* __restrict__ src, scan_pyramid_t d, int Cs, const __bf16* __restrict__ wh,
    const __bf16* __restrict__ wl, int Csw, const float* __restrict__ bias, const float* __restrict__ mask,
    float* __restrict__ dst, int Nout, int Ns, int relu, TileTab2 tt, int n_tiles, scan_pyramid_t sd, int map,
    double* __restrict__ gn_ws) {
  constexpr int HALO = KS / 2, NTAPS = KS * KS;
  constexpr int PH = TH + 2 * HALO;
  constexpr int PWK = TW + 2 * HALO;
  constexpr int NPATCH = PH * PWK;                // halo pixels: 180 (TH 8) or 324 (TH 16); 256 for the 1x1
  constexpr int WAVES = NT / 64;
  constexpr int WN_WAVES = BN >= 128 ? 2 : 1;     // 2 (BN=128 / 256) or 1 (BN=64)
  constexpr int WM_WAVES = WAVES / WN_WAVES;
  constexpr int TM = (TH * TW / 32) / WM_WAVES;   // 32-pixel MFMA tiles per wave
  constexpr int TN = BN / (32 * WN_WAVES);        // 32-channel MFMA tiles per wave: 2, or 4 for BN=256
  constexpr int ASLOTS = (NPATCH * 8 + NT - 1) / NT;  // float4 of the halo patch per thread per chunk
  constexpr int BSEG = BN * 4 * 2 / NT;           // 16-byte weight segments per thread per (chunk, tap)

  extern __shared__ __align__(16) unsigned char smem_raw[];
  __bf16* Ah = reinterpret_cast<__bf16*>(smem_raw);  // [PH][PPITCH]
  __bf16* Al = Ah + PH * PPITCH;                     // [PH][PPITCH]
  __bf16* Bs = Al + PH * PPITCH;                     // [2 buf][2 plane][BN][LROW]

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int bid = xcd_remap(blockIdx.x, gridDim.x);
  const int n_tile = bid % n_tiles;
  const int tile = bid / n_tiles;
  int lvl = 0;
#pragma unroll
  for (int i = 1; i < SCAN_MAX_LEVELS; ++i)
    if (i < d.n_levels && tile >= tt.tile_off[i]) lvl = i;
  const int H = d.h[lvl], W = d.w[lvl];
  int t = tile - tt.tile_off[lvl];
  const int per_img = tt.tiles_x[lvl] * tt.tiles_y[lvl];
  const int img = t / per_img;
  t -= img * per_img;
  const int ty0 = (t / tt.tiles_x[lvl]) * TH, tx0 = (t % tt.tiles_x[lvl]) * TW;
  const int64_t rowbase = d.row_off[lvl] + (int64_t)img * H * W;
  const int n0 = n_tile * BN;
  const int nchunks = (Cs + CK - 1) / CK;

  // ---- A patch staging roles: 180 pixels x 8 float4 = 1440 slots, 6 per thread
  float4 ra[ASLOTS];
  auto load_a = [&](int cc) {
    const int c0 = cc * CK;
#pragma unroll
    for (int i = 0; i < ASLOTS; ++i) {
      const int slot = tid + NT * i;
      const int q = slot >> 3, c = c0 + 4 * (slot & 7);
      const int py = q / PWK, px = q - py * PWK;
      const int y = ty0 - HALO + py, x = tx0 - HALO + px;
      bool ok = (slot < NPATCH * 8) && y >= 0 && y < H && x >= 0 && x < W && c < Cs;
      int64_t row = rowbase + (int64_t)y * W + x;
      if (KS == 1 && map != 0) {
        const int Hs = sd.h[lvl], Ws = sd.w[lvl];
        int sy, sx;
        if (map == 1) {
          sy = 2 * y;
          sx = 2 * x;
        } else {
          ok = ok && ((y | x) & 1) == 0;
          sy = y >> 1;
          sx = x >> 1;
        }
        ok = ok && sy < Hs && sx < Ws;
        row = sd.row_off[lvl] + ((int64_t)img * Hs + sy) * Ws + sx;
      }
      ra[i] = ok ? *reinterpret_cast<const float4*>(src + row * Cs + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  auto store_a = [&]() {
#pragma unroll
    for (int i = 0; i < ASLOTS; ++i) {
      const int slot = tid + NT * i;
      if (slot < NPATCH * 8) {
        const int q = slot >> 3, c4 = slot & 7;
        const int py = q / PWK, px = q - py * PWK;
        bf16x4 hi, lo;
        split4(ra[i], hi, lo);
        *reinterpret_cast<bf16x4*>(Ah + py * PPITCH + px * LROW + 4 * c4) = hi;
        *reinterpret_cast<bf16x4*>(Al + py * PPITCH + px * LROW + 4 * c4) = lo;
      }
    }
  };
  // ---- B staging roles: BN rows x 4 segments x 2 planes
  uint4 rb[BSEG];
  auto load_b = [&](int cc, int tap) {
#pragma unroll
    for (int i = 0; i < BSEG; ++i) {
      const int slot = tid + NT * i;
      const int plane = slot / (BN * 4);
      const int rem = slot - plane * BN * 4;
      const int row = rem >> 2, seg = rem & 3;
      const int o = n0 + row, c = cc * CK + 8 * seg;
      const __bf16* base = plane ? wl : wh;
      rb[i] = (o < Nout && c < Csw) ? *reinterpret_cast<const uint4*>(base + ((int64_t)o * NTAPS + tap) * Csw + c)
                                    : make_uint4(0u, 0u, 0u, 0u);
    }
  };
  auto store_b = [&](int buf) {
#pragma unroll
    for (int i = 0; i < BSEG; ++i) {
      const int slot = tid + NT * i;
      const int plane = slot / (BN * 4);
      const int rem = slot - plane * BN * 4;
      const int row = rem >> 2, seg = rem & 3;
      *reinterpret_cast<uint4*>(Bs + ((buf * 2 + plane) * BN + row) * LROW + 8 * seg) = rb[i];
    }
  };

  // ---- MFMA roles
  const int wm = wid / WN_WAVES, wn = wid % WN_WAVES;
  const int lr = lane & 31, lh = lane >> 5;
  int a_off[TM];  // bf16 offset of this lane's pixel (tap 0,0) + its k-half
#pragma unroll
  for (int tm = 0; tm < TM; ++tm) {
    const int p = (wm * TM + tm) * 32 + lr;  // pixel within the 8x16 tile
    a_off[tm] = (p >> 4) * PPITCH + (p & 15) * LROW + 8 * lh;
  }
  const int b_off = (wn * 32 * TN + lr) * LROW + 8 * lh;

  f32x16 acc[TM][TN];
#pragma unroll
  for (int a = 0; a < TM; ++a)
#pragma unroll
    for (int b = 0; b < TN; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

  load_a(0);
  load_b(0, 0);
  for (int cc = 0; cc < nchunks; ++cc) {
    __syncthreads();  // every wave is done reading the previous chunk's patch
    store_a();
    if (cc + 1 < nchunks) load_a(cc + 1);
#pragma unroll 1
    for (int tap = 0; tap < NTAPS; ++tap) {
      const int buf = (cc * NTAPS + tap) & 1;
      store_b(buf);
      if (tap < NTAPS - 1)
        load_b(cc, tap + 1);
      else if (cc + 1 < nchunks)
        load_b(cc + 1, 0);
      __syncthreads();
      const int ky = tap / KS, kx = tap - KS * ky;
      const int shift = ky * PPITCH + kx * LROW;
      const __bf16* bh = Bs + (buf * 2 + 0) * BN * LROW + b_off;
      const __bf16* bl = Bs + (buf * 2 + 1) * BN * LROW + b_off;
      if constexpr (TN > 2) {
        // 128 accumulator registers: keep only one channel tile's weight fragments live at a time
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          bf16x8 ah[TM], al[TM];
#pragma unroll
          for (int tm = 0; tm < TM; ++tm) {
            ah[tm] = *reinterpret_cast<const bf16x8*>(Ah + a_off[tm] + shift + 16 * s);
            al[tm] = *reinterpret_cast<const bf16x8*>(Al + a_off[tm] + shift + 16 * s);
          }
#pragma unroll
          for (int tn = 0; tn < TN; ++tn) {
            const bf16x8 bhv = *reinterpret_cast<const bf16x8*>(bh + tn * 32 * LROW + 16 * s);
            const bf16x8 blv = *reinterpret_cast<const bf16x8*>(bl + tn * 32 * LROW + 16 * s);
#pragma unroll
            for (int tm = 0; tm < TM; ++tm) {
              acc[tm][tn] = SCAN_MMA(al[tm], bhv, acc[tm][tn]);
              acc[tm][tn] = SCAN_MMA(ah[tm], blv, acc[tm][tn]);
              acc[tm][tn] = SCAN_MMA(ah[tm], bhv, acc[tm][tn]);
            }
          }
        }
        continue;
      }
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        bf16x8 ah[TM], al[TM], bhv[TN], blv[TN];
#pragma unroll
        for (int tm = 0; tm < TM; ++tm) {
          ah[tm] = *reinterpret_cast<const bf16x8*>(Ah + a_off[tm] + shift + 16 * s);
          al[tm] = *reinterpret_cast<const bf16x8*>(Al + a_off[tm] + shift + 16 * s);
        }
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) {
          bhv[tn] = *reinterpret_cast<const bf16x8*>(bh + tn * 32 * LROW + 16 * s);
          blv[tn] = *reinterpret_cast<const bf16x8*>(bl + tn * 32 * LROW + 16 * s);
        }
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
#pragma unroll
          for (int tn = 0; tn < TN; ++tn) {
            acc[tm][tn] = SCAN_MMA(al[tm], bhv[tn], acc[tm][tn]);
            acc[tm][tn] = SCAN_MMA(ah[tm], blv[tn], acc[tm][tn]);
            acc[tm][tn] = SCAN_MMA(ah[tm], bhv[tn], acc[tm][tn]);
          }
      }
    }
  }

  // ---- epilogue.  C/D map of 32x32: col = lane&31 (channel), row = (reg&3) + 8*(reg>>2) + 4*(lane>>5) (pixel)
#pragma unroll
  for (int tn = 0; tn < TN; ++tn) {
    const int o = n0 + wn * 32 * TN + tn * 32 + lr;
    const float bv = (bias != nullptr && o < Nout) ? bias[o] : 0.f;
    double gs = 0.0, gq = 0.0;  // every element enters both GroupNorm sums as a double (see gn_sums_add, conv_fwd.hip)
    if (relu & 2) {
      // fused 2x2 / stride-2 max-pool (frozen VGG stages, single-level pyramid): a window's four pixels are the
      // registers r, r+1 (x, x+1) and r+8, r+9 (next row) of ONE lane, so the pooled tensor is written directly and
      // the full-resolution activation never reaches HBM
      const int Hp = H >> 1, Wp = W >> 1;
#pragma unroll
      for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int r = 2 * q;  // 0, 2, 4, 6
          const int p = (wm * TM + tm) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
          const int y = ty0 + (p >> 4), x = tx0 + (p & 15);
          if (y < H && x < W && o < Nout) {
            float v = fmaxf(fmaxf(acc[tm][tn][r], acc[tm][tn][r + 1]), fmaxf(acc[tm][tn][r + 8], acc[tm][tn][r + 9])) + bv;
            if (relu & 1) v = fmaxf(v, 0.f);
            dst[((int64_t)img * Hp * Wp + (int64_t)(y >> 1) * Wp + (x >> 1)) * Ns + o] = v;
          }
        }
      continue;
    }
#pragma unroll
    for (int tm = 0; tm < TM; ++tm) {
      // the ReLU mask of a data gradient: fetch the 16 values of this MFMA tile first so the loads overlap
      // (one dependent load per store serialises on the memory latency and costs ~20 us per tile)
      float mk[16];
      if (mask != nullptr) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int p = (wm * TM + tm) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
          const int y = ty0 + (p >> 4), x = tx0 + (p & 15);
          const bool ok = y < H && x < W && o < Nout;
          mk[r] = ok ? mask[(rowbase + (int64_t)y * W + x) * Ns + o] : 0.f;
        }
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int p = (wm * TM + tm) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        const int y = ty0 + (p >> 4), x = tx0 + (p & 15);
        if (y < H && x < W && o < Nout) {
          const int64_t m = rowbase + (int64_t)y * W + x;
          float v = acc[tm][tn][r] + bv;
          if (relu & 1) v = fmaxf(v, 0.f);
          if (mask != nullptr) v = (mk[r] > 0.f) ? v : 0.f;
          dst[m * Ns + o] = v;
          if (gn_ws != nullptr) {
            gs += (double)v;
            gq += (double)v * (double)v;
          }
        }
      }
    }
    if (gn_ws != nullptr) {
      // GroupNorm(32) statistics of the 256-channel output this conv feeds: sum / sum of squares per (level, image,
      // group of 8 channels = 8 adjacent lanes, both lane halves), one fp64 atomic pair per group and wave
      double ds = gs, dq = gq;
#pragma unroll
      for (int sh = 1; sh <= 4; sh <<= 1) {
        ds += __shfl_xor(ds, sh, 64);
        dq += __shfl_xor(dq, sh, 64);
      }
      ds += __shfl_xor(ds, 32, 64);
      dq += __shfl_xor(dq, 32, 64);
      if ((lr & 7) == 0 && lh == 0 && o < Nout) {
        const int64_t slot = ((int64_t)(lvl * d.n_images + img) * 32 + (o >> 3)) * 2;
        atomicAdd(&gn_ws[slot], ds);
        atomicAdd(&gn_ws[slot + 1], dq);
      }
    }
  }
}

template <int BN, int TH, int NT, int KS>
static void launch_gen1(const ConvArgs& a) {
  constexpr int PH = TH + 2 * (KS / 2);
  TileTab2 tt;
  make_tiles(a.od, &tt, TH);
  const int tiles = tt.tile_off[a.od->n_levels];
  const int n_tiles = (a.Nout + BN - 1) / BN;
  constexpr size_t sh = (size_t)(2 * PH * PPITCH + 4 * BN * LROW) * sizeof(__bf16);
  static bool done = false;
  if (!done && sh > 64 * 1024) {
    hipFuncSetAttribute(reinterpret_cast<const void*>(conv3x3_bf16x3_kernel<BN, TH, NT, KS>),
                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh);
    done = true;
  }
  hipLaunchKernelGGL((conv3x3_bf16x3_kernel<BN, TH, NT, KS>), dim3(tiles * n_tiles), dim3(NT), sh, a.st, a.x, *a.od, a.Cs, a.w[0],
                     a.w[1], a.Csw, a.bias, a.mask, a.y, a.Nout, a.Ns, a.relu, tt, n_tiles, *a.sd, a.map, a.gn_ws);
}

void gen1_conv3x3_launch(const ConvArgs& a) {
  if (a.Nout <= 64) return launch_gen1<64, 8, 256, 3>(a);
  // 16 x 16 pixel tiles, 512 threads (8 waves = 4 x 2).  BN = 128: each wave 64 px x 64 ch; BN = 256: 64 px x 128 ch,
  // used when the output channels fill 256-wide tiles and the launch still has >= 2 workgroups per CU.
  TileTab2 tt;
  make_tiles(a.od, &tt, 16);
  const int64_t tiles = tt.tile_off[a.od->n_levels];
  if (g_scan_conv_bn256 && a.Nout % 256 == 0 && tiles * (a.Nout / 256) >= 512) return launch_gen1<256, 16, 512, 3>(a);
  launch_gen1<128, 16, 512, 3>(a);
}

void gen1_conv1x1_launch(const ConvArgs& a) {
  if (a.Nout <= 64) return launch_gen1<64, 8, 256, 1>(a);
  launch_gen1<128, 16, 512, 1>(a);
}
