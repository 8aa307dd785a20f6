// Public entry points of the split-operand convolutions, forward and data gradient ("bf16x3" = two bf16 pieces per fp32
// operand, "bf16x6" = three: conv_split.h), of their instance queries, of the weight split, and of the dispatcher that
// chooses among them (scan_conv_plan / scan_conv_weight_split / scan_conv_run, at the end of the file).
//
// Every single-launch entry point does the same four things: validate the arguments (check3x3 / check1x1), fill a ConvArgs,
// pick the kernel instance (conv_launch.h: pick3x3 / pick1x1 in conv_fwd.hip; the Winograd entry has its own instance;
// two-piece launches go to conv_gen1.hip under scan_tune("conv_v2", 0)), launch and check.  The dispatcher is the one place
// that says which of them a conv takes, on which weight planes: scan_amd/ops.py and scan_ops_ext.cpp hold no such rule.
// No kernel of the convolutions lives here.
//
// The weight gradients have their dispatcher here too (scan_conv_wgrad_plan / scan_conv_wgrad_run and, on top of the same two
// steps, the split families' older entry points); their plan and launch code is conv_wgrad.hip's and conv_mfma.hip's.
//
// dgrad reuses the forward kernels: dX = conv3x3(dY, W') with W'[c][t][o] = W[o][8-t][c]
// (scan_weight_split mode 1 writes the flipped + transposed copy).
#include "conv_launch.h"
#include "conv_split.h"

// w [O][T][Cs] fp32 -> NP bf16 planes (conv_split.h).
//   mode 0: out[o][t][c]            (O rows, row length Csw >= Cs, zero padded)       -- forward
//   mode 1: out[c][T-1-t][o]        (Cs rows, row length Csw >= O, zero padded)       -- dgrad (flip + transpose)
//   modes 2 / 3 (T = 9 only): the Winograd F(2,3) planes of modes 0 / 1 -- 12 taps j * 3 + ky per row, tap (j, ky) =
//           sum_kx G[j][kx] * (mode 0 / 1 value of tap ky * 3 + kx), in fp64, rounded once to fp32, then split
//           (conv_fwd.hip, WINO)
template <int NP>
__global__ void weight_split_kernel(const float* __restrict__ w, int O, int T, int Cs, int mode, int rows, int Csw,
                                    __bf16* __restrict__ w0, __bf16* __restrict__ w1, __bf16* __restrict__ w2) {
  const int TO = mode >= 2 ? 12 : T;  // taps per plane row
  const int64_t total = (int64_t)rows * TO * Csw;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int col = (int)(i % Csw);
    const int64_t rt = i / Csw;
    const int tt = (int)(rt % TO);
    const int row = (int)(rt / TO);
    float v = 0.f;
    if (mode == 0) {
      if (col < Cs) v = w[((int64_t)row * T + tt) * Cs + col];
    } else if (mode == 1) {
      if (col < O) v = w[((int64_t)col * T + (T - 1 - tt)) * Cs + row];
    } else {
      const int j = tt / 3, ky = tt - 3 * j;
      double g[3] = {0.0, 0.0, 0.0};
      for (int kx = 0; kx < 3; ++kx) {
        const int t = ky * 3 + kx;
        if (mode == 2 && col < Cs) g[kx] = w[((int64_t)row * T + t) * Cs + col];
        if (mode == 3 && col < O) g[kx] = w[((int64_t)col * T + (T - 1 - t)) * Cs + row];
      }
      v = wino_g(j, g[0], g[1], g[2]);
    }
    __bf16 q[NP];
    split1_np<NP>(v, q);
    w0[i] = q[0];
    w1[i] = q[1];
    if constexpr (NP == 3) w2[i] = q[2];
  }
}

static int weight_split_launch(int np, const float* w, int32_t O, int32_t T, int32_t Cs, int32_t mode, void* w0, void* w1,
                               void* w2, int32_t Csw, void* stream) {
  SCAN_CHECK_ARG(w && w0 && w1 && (np == 2 || w2) && O > 0 && T > 0 && Cs > 0, "weight_split: bad arguments");
  SCAN_CHECK_ARG(mode >= 0 && mode <= 3, "weight_split: mode must be 0..3");
  SCAN_CHECK_ARG(mode < 2 || (np == 3 && T == 9), "weight_split: the Winograd modes 2 / 3 take three pieces and T = 9");
  SCAN_CHECK_ARG(Csw % 8 == 0 && Csw >= ((mode & 1) == 0 ? Cs : O),
                 "weight_split: Csw=%d must be a multiple of 8 and cover the row", Csw);
  const int rows = (mode & 1) == 0 ? O : Cs;
  const int64_t total = (int64_t)rows * (mode >= 2 ? 12 : T) * Csw;
  __bf16 *p0 = reinterpret_cast<__bf16*>(w0), *p1 = reinterpret_cast<__bf16*>(w1), *p2 = reinterpret_cast<__bf16*>(w2);
  if (np == 3)
    hipLaunchKernelGGL(weight_split_kernel<3>, dim3(grid_for(total, 256)), dim3(256), 0, as_stream(stream), w, O, T, Cs, mode,
                       rows, Csw, p0, p1, p2);
  else
    hipLaunchKernelGGL(weight_split_kernel<2>, dim3(grid_for(total, 256)), dim3(256), 0, as_stream(stream), w, O, T, Cs, mode,
                       rows, Csw, p0, p1, p2);
  SCAN_LAUNCH_CHECK("weight_split");
  return 0;
}

extern "C" int scan_weight_split(const float* w, int32_t O, int32_t T, int32_t Cs, int32_t mode, void* wh, void* wl,
                                 int32_t Csw, void* stream) {
  return weight_split_launch(2, w, O, T, Cs, mode, wh, wl, nullptr, Csw, stream);
}
extern "C" int scan_weight_split3(const float* w, int32_t O, int32_t T, int32_t Cs, int32_t mode, void* wh, void* wm,
                                  void* wl, int32_t Csw, void* stream) {
  return weight_split_launch(3, w, O, T, Cs, mode, wh, wm, wl, Csw, stream);
}

// 1 (default): two-piece forward / data-gradient launches go to conv_fwd.hip; 0: the 32x32x16 kernel of conv_gen1.hip (the
// independent implementation the tests compare against)
int g_scan_conv_v2 = 1;
// the production kernel stores float4 and loads the ReLU mask as float4
static inline bool v2_ok(const void* y, const void* mask, int32_t Ns) {
  return (Ns & 3) == 0 && (reinterpret_cast<uintptr_t>(y) & 15) == 0 && (reinterpret_cast<uintptr_t>(mask) & 15) == 0;
}

static int check_pyramid(const char* name, const scan_pyramid_t* d) {
  SCAN_CHECK_ARG(d && d->n_levels >= 1 && d->n_levels <= SCAN_MAX_LEVELS && d->n_images >= 1, "%s: bad pyramid", name);
  return 0;
}
// what every conv launch needs of its channel counts and pointers (the pyramids are the caller's: they differ by kernel size)
static int check_common(const char* name, int np, const float* x, int32_t Cs, const void* w0, const void* w1, const void* w2,
                        int32_t Csw, const float* mask, const float* y, int32_t Nout, int32_t Ns) {
  SCAN_CHECK_ARG(Cs > 0 && Cs % 4 == 0, "%s: Cs=%d must be a positive multiple of 4", name, Cs);
  SCAN_CHECK_ARG(Csw % 8 == 0 && Csw >= Cs, "%s: Csw=%d must be a multiple of 8 and >= Cs", name, Csw);
  SCAN_CHECK_ARG(Nout > 0 && Ns >= Nout, "%s: Nout=%d Ns=%d", name, Nout, Ns);
  SCAN_CHECK_ARG(x && w0 && w1 && (np == 2 || w2) && y, "%s: null pointer", name);
  // (two pieces fall back to conv_gen1.hip, which stores scalars)
  SCAN_CHECK_ARG(np == 2 || v2_ok(y, mask, Ns), "%s: y / mask must be 16-byte aligned and Ns a multiple of 4 (Ns=%d)", name, Ns);
  return 0;
}
static int check3x3(const char* name, int np, const float* x, const scan_pyramid_t* d, int32_t Cs, const void* w0, const void* w1,
                    const void* w2, int32_t Csw, const float* mask, const float* y, int32_t Nout, int32_t Ns) {
  if (check_pyramid(name, d)) return -1;
  return check_common(name, np, x, Cs, w0, w1, w2, Csw, mask, y, Nout, Ns);
}
// the fused 2x2 / stride-2 max-pool epilogue (relu bit 1)
static int check_pool2(const char* name, const scan_pyramid_t* d) {
  SCAN_CHECK_ARG(d && d->n_levels == 1 && (d->h[0] & 1) == 0 && (d->w[0] & 1) == 0,
                 "%s: the fused pool needs a single-level pyramid with even H and W (levels=%d)", name, d ? d->n_levels : 0);
  return 0;
}
// map 0: stride 1 (xd == yd); map 1: stride 2 forward (yd = xd.conv_out(1, 2)); map 2: data gradient of a stride-2 1x1 conv
static int check1x1(const char* name, int np, const float* x, const scan_pyramid_t* xd, int32_t Cs, const void* w0, const void* w1,
                    const void* w2, int32_t Csw, const float* mask, const float* y, const scan_pyramid_t* yd, int32_t Nout,
                    int32_t Ns, int32_t map) {
  SCAN_CHECK_ARG(xd && yd && yd->n_levels >= 1 && yd->n_levels <= SCAN_MAX_LEVELS && yd->n_images >= 1 &&
                     xd->n_levels == yd->n_levels && xd->n_images == yd->n_images,
                 "%s: bad pyramids", name);
  SCAN_CHECK_ARG(map >= 0 && map <= 2, "%s: map=%d must be 0, 1 or 2", name, map);
  if (check_common(name, np, x, Cs, w0, w1, w2, Csw, mask, y, Nout, Ns)) return -1;
  for (int l = 0; l < yd->n_levels; ++l) {
    const int eh = map == 0 ? xd->h[l] : map == 1 ? (xd->h[l] - 1) / 2 + 1 : yd->h[l];
    const int ew = map == 0 ? xd->w[l] : map == 1 ? (xd->w[l] - 1) / 2 + 1 : yd->w[l];
    SCAN_CHECK_ARG(eh == yd->h[l] && ew == yd->w[l] &&
                       (map != 2 || ((yd->h[l] - 1) / 2 + 1 == xd->h[l] && (yd->w[l] - 1) / 2 + 1 == xd->w[l])),
                   "%s: level %d sizes do not match map %d", name, l, map);
  }
  return 0;
}

// GroupNorm(32, 256) sums of a conv epilogue: fp64 (sum, sum of squares) per (level, image, group)
static int gn_ws_clear(const char* name, float* gn_ws, const scan_pyramid_t* d, void* stream) {
  const size_t bytes = sizeof(double) * 2 * 32 * (size_t)d->n_levels * d->n_images;
  if (hipMemsetAsync(gn_ws, 0, bytes, as_stream(stream)) != hipSuccess) {
    scan_set_error("%s: memset failed", name);
    return -2;
  }
  return 0;
}

static ConvArgs conv_args(const float* x, const scan_pyramid_t* od, const scan_pyramid_t* sd, int32_t Cs, const void* w0,
                          const void* w1, const void* w2, int32_t Csw, const float* bias, const float* mask, float* y,
                          int32_t Nout, int32_t Ns, int32_t relu, int32_t map, void* stream, void* gn_ws) {
  return ConvArgs{x, od, sd, Cs, {reinterpret_cast<const __bf16*>(w0), reinterpret_cast<const __bf16*>(w1),
                                  reinterpret_cast<const __bf16*>(w2)}, Csw, bias, mask, y, Nout, Ns, relu, map,
                  as_stream(stream), reinterpret_cast<double*>(gn_ws)};
}
// two pieces stay on the production kernel unless the knob or the output layout says otherwise
static inline bool use_gen1(int np, const ConvArgs& a) { return np == 2 && !(g_scan_conv_v2 && v2_ok(a.y, a.mask, a.Ns)); }

// y[M][Ns] = conv3x3_s1(x[M][Cs]) with pre-split weight planes [Nout][9][Csw]; same pyramid in and out.
// gn_ws: conv3x3 + bias whose output feeds GroupNorm(32, 256) -- the epilogue also accumulates the per-(level, image, group)
// sum and sum of squares into gn_ws (fp64, n_levels * n_images * 32 * 2 values), which scan_groupnorm_stats_from_sums turns
// into (mean, rstd): the separate statistics pass over y disappears.  clear != 0: gn_ws is zeroed here; 0: the sums are
// ADDED to gn_ws as it is (scan_amd/ops.py hands out slices of one buffer it clears with one memset per training iteration
// instead of one memset launch per call).
static int conv3x3(const char* name, int np, const float* x, const scan_pyramid_t* d, int32_t Cs, const void* w0, const void* w1,
                   const void* w2, int32_t Csw, const float* bias, const float* mask, float* y, int32_t Nout, int32_t Ns,
                   int32_t relu, void* stream, float* gn_ws = nullptr, int clear = 0) {
  if (check3x3(name, np, x, d, Cs, w0, w1, w2, Csw, mask, y, Nout, Ns)) return -1;
  if (clear && gn_ws_clear(name, gn_ws, d, stream)) return -2;
  const ConvArgs a = conv_args(x, d, d, Cs, w0, w1, w2, Csw, bias, mask, y, Nout, Ns, relu, 0, stream, gn_ws);
  if (use_gen1(np, a))
    gen1_conv3x3_launch(a);
  else
    pick3x3(np, d, Nout, Csw % 32 == 0).launch(a);
  SCAN_LAUNCH_CHECK(name);
  return 0;
}

extern "C" int scan_conv3x3_bf16x3(const float* x, const scan_pyramid_t* d, int32_t Cs, const void* wh, const void* wl,
                                   int32_t Csw, const float* bias, const float* mask, float* y, int32_t Nout,
                                   int32_t Ns, int32_t relu, void* stream) {
  return conv3x3("conv3x3_bf16x3", 2, x, d, Cs, wh, wl, nullptr, Csw, bias, mask, y, Nout, Ns, relu ? 1 : 0, stream);
}
extern "C" int scan_conv3x3_bf16x6(const float* x, const scan_pyramid_t* d, int32_t Cs, const void* wh, const void* wm,
                                   const void* wl, int32_t Csw, const float* bias, const float* mask, float* y,
                                   int32_t Nout, int32_t Ns, int32_t relu, void* stream) {
  return conv3x3("conv3x3_bf16x6", 3, x, d, Cs, wh, wm, wl, Csw, bias, mask, y, Nout, Ns, relu ? 1 : 0, stream);
}

static int conv3x3_gn(const char* name, int np, int clear, const float* x, const scan_pyramid_t* d, int32_t Cs, const void* w0,
                      const void* w1, const void* w2, int32_t Csw, const float* bias, float* y, int32_t Nout, int32_t Ns,
                      float* gn_ws, void* stream) {
  SCAN_CHECK_ARG(Nout == 256 && gn_ws, "%s: needs Nout == 256 (GroupNorm(32, 256)) and a workspace (Nout=%d)", name, Nout);
  return conv3x3(name, np, x, d, Cs, w0, w1, w2, Csw, bias, nullptr, y, Nout, Ns, 0, stream, gn_ws, clear);
}
extern "C" int scan_conv3x3_gn_bf16x3(const float* x, const scan_pyramid_t* d, int32_t Cs, const void* wh, const void* wl,
                                      int32_t Csw, const float* bias, float* y, int32_t Nout, int32_t Ns, float* gn_ws,
                                      void* stream) {
  return conv3x3_gn("conv3x3_gn_bf16x3", 2, 1, x, d, Cs, wh, wl, nullptr, Csw, bias, y, Nout, Ns, gn_ws, stream);
}
extern "C" int scan_conv3x3_gn_acc_bf16x3(const float* x, const scan_pyramid_t* d, int32_t Cs, const void* wh, const void* wl,
                                          int32_t Csw, const float* bias, float* y, int32_t Nout, int32_t Ns, float* gn_ws,
                                          void* stream) {
  return conv3x3_gn("conv3x3_gn_acc_bf16x3", 2, 0, x, d, Cs, wh, wl, nullptr, Csw, bias, y, Nout, Ns, gn_ws, stream);
}
extern "C" int scan_conv3x3_gn_bf16x6(const float* x, const scan_pyramid_t* d, int32_t Cs, const void* wh, const void* wm,
                                      const void* wl, int32_t Csw, const float* bias, float* y, int32_t Nout, int32_t Ns,
                                      float* gn_ws, int32_t clear, void* stream) {
  return conv3x3_gn("conv3x3_gn_bf16x6", 3, clear, x, d, Cs, wh, wm, wl, Csw, bias, y, Nout, Ns, gn_ws, stream);
}

// the Winograd F(2,3) instance (conv_fwd.hip): wh / wm / wl = scan_weight_split3 planes of mode 2 (forward) or 3 (data
// gradient); gn_ws != nullptr: the GroupNorm sums of scan_conv3x3_gn_bf16x6 (Nout == 256, clear as there); relu: bit 0 =
// ReLU, bit 1 = fused 2x2 / stride-2 max-pool as scan_conv3x3_pool2_bf16x6 (single level, even H and W)
static int conv3x3_wino(const char* name, const float* x, const scan_pyramid_t* d, int32_t Cs, const void* wh, const void* wm,
                        const void* wl, int32_t Csw, const float* bias, const float* mask, float* y, int32_t Nout, int32_t Ns,
                        int32_t relu, float* gn_ws, int32_t clear, void* stream) {
  if (check3x3(name, 3, x, d, Cs, wh, wm, wl, Csw, mask, y, Nout, Ns)) return -1;
  SCAN_CHECK_ARG(Nout > 64 && Csw % 32 == 0, "%s: needs Nout > 64 and Csw %% 32 == 0 (Nout=%d Csw=%d)", name, Nout, Csw);
  if (gn_ws != nullptr)
    SCAN_CHECK_ARG(Nout == 256 && mask == nullptr && !relu, "%s: GroupNorm sums need Nout == 256, no mask, no ReLU (Nout=%d)", name, Nout);
  if (relu & 2) {
    if (check_pool2(name, d)) return -1;
    SCAN_CHECK_ARG(mask == nullptr && gn_ws == nullptr, "%s: the fused pool takes no mask and no sums (relu=%d)", name, relu);
  }
  if (gn_ws != nullptr && clear && gn_ws_clear(name, gn_ws, d, stream)) return -2;
  conv3x3_wino_launch(conv_args(x, d, d, Cs, wh, wm, wl, Csw, bias, mask, y, Nout, Ns, relu & 3, 0, stream, gn_ws));
  SCAN_LAUNCH_CHECK(name);
  return 0;
}
extern "C" int scan_conv3x3_wino_bf16x6(const float* x, const scan_pyramid_t* d, int32_t Cs, const void* wh, const void* wm,
                                        const void* wl, int32_t Csw, const float* bias, const float* mask, float* y,
                                        int32_t Nout, int32_t Ns, int32_t relu, float* gn_ws, int32_t clear, void* stream) {
  return conv3x3_wino("conv3x3_wino_bf16x6", x, d, Cs, wh, wm, wl, Csw, bias, mask, y, Nout, Ns, relu, gn_ws, clear, stream);
}

// conv3x3 + bias (+ ReLU) + 2x2 / stride-2 max-pool in one launch: y [N, H/2, W/2, Ns] (forward only; single-level
// pyramid with even H, W).  max and the monotone bias / ReLU commute, so the result equals pooling the conv output.
extern "C" int scan_conv3x3_pool2_bf16x3(const float* x, const scan_pyramid_t* d, int32_t Cs, const void* wh,
                                         const void* wl, int32_t Csw, const float* bias, float* y, int32_t Nout,
                                         int32_t Ns, int32_t relu, void* stream) {
  if (check_pool2("conv3x3_pool2_bf16x3", d)) return -1;
  return conv3x3("conv3x3_pool2_bf16x3", 2, x, d, Cs, wh, wl, nullptr, Csw, bias, nullptr, y, Nout, Ns, (relu ? 1 : 0) | 2, stream);
}
extern "C" int scan_conv3x3_pool2_bf16x6(const float* x, const scan_pyramid_t* d, int32_t Cs, const void* wh,
                                         const void* wm, const void* wl, int32_t Csw, const float* bias, float* y,
                                         int32_t Nout, int32_t Ns, int32_t relu, void* stream) {
  if (check_pool2("conv3x3_pool2_bf16x6", d)) return -1;
  return conv3x3("conv3x3_pool2_bf16x6", 3, x, d, Cs, wh, wm, wl, Csw, bias, nullptr, y, Nout, Ns, (relu ? 1 : 0) | 2, stream);
}

// y[Mo][Ns] = conv1x1(x[Mi][Cs]) with pre-split weight planes [Nout][1][Csw].  map 0: stride 1 (xd == yd);
// map 1: stride 2 forward (yd = xd.conv_out(1, 2)); map 2: data gradient of a stride-2 1x1 conv (x = dY on the coarse
// pyramid xd, y = dX on the fine pyramid yd, zero where a coordinate is odd).
static int conv1x1(const char* name, int np, const float* x, const scan_pyramid_t* xd, int32_t Cs, const void* w0, const void* w1,
                   const void* w2, int32_t Csw, const float* bias, const float* mask, float* y, const scan_pyramid_t* yd,
                   int32_t Nout, int32_t Ns, int32_t relu, int32_t map, void* stream) {
  if (check1x1(name, np, x, xd, Cs, w0, w1, w2, Csw, mask, y, yd, Nout, Ns, map)) return -1;
  const ConvArgs a = conv_args(x, yd, xd, Cs, w0, w1, w2, Csw, bias, mask, y, Nout, Ns, relu, map, stream, nullptr);
  if (use_gen1(np, a))
    gen1_conv1x1_launch(a);
  else
    pick1x1(np, yd, Nout, Csw).launch(a);
  SCAN_LAUNCH_CHECK(name);
  return 0;
}
extern "C" int scan_conv1x1_bf16x3(const float* x, const scan_pyramid_t* xd, int32_t Cs, const void* wh, const void* wl,
                                   int32_t Csw, const float* bias, const float* mask, float* y,
                                   const scan_pyramid_t* yd, int32_t Nout, int32_t Ns, int32_t relu, int32_t map,
                                   void* stream) {
  return conv1x1("conv1x1_bf16x3", 2, x, xd, Cs, wh, wl, nullptr, Csw, bias, mask, y, yd, Nout, Ns, relu, map, stream);
}
extern "C" int scan_conv1x1_bf16x6(const float* x, const scan_pyramid_t* xd, int32_t Cs, const void* wh, const void* wm,
                                   const void* wl, int32_t Csw, const float* bias, const float* mask, float* y,
                                   const scan_pyramid_t* yd, int32_t Nout, int32_t Ns, int32_t relu, int32_t map,
                                   void* stream) {
  return conv1x1("conv1x1_bf16x6", 3, x, xd, Cs, wh, wm, wl, Csw, bias, mask, y, yd, Nout, Ns, relu, map, stream);
}

// ---- which instance a launch on output pyramid d with Nout output channels takes under the current knobs (bench.py labels
// its timings with it; the ids: conv_fwd.hip).  The 3x3 queries assume whole K chunks (Csw % 32 == 0): true for every 3x3
// plane ops.py splits.
extern "C" int scan_conv3x3_bf16x3_instance(const scan_pyramid_t* d, int32_t Nout) { return d ? pick3x3(2, d, Nout, true).id : -1; }
extern "C" int scan_conv3x3_bf16x6_instance(const scan_pyramid_t* d, int32_t Nout) { return d ? pick3x3(3, d, Nout, true).id : -1; }
extern "C" int scan_conv1x1_bf16x6_instance(const scan_pyramid_t* yd, int32_t Nout, int32_t Csw) {
  return yd ? pick1x1(3, yd, Nout, Csw).id : -1;
}
// 1: ops.py splits this layer's weights into Winograd planes and calls scan_conv3x3_wino_bf16x6 (scan_tune "conv_wino")
extern "C" int scan_conv3x3_bf16x6_wino(int32_t Nout, int32_t Csw) { return g_scan_conv_wino && Nout > 64 && Csw % 32 == 0 ? 1 : 0; }

// ---- the dispatcher: plan (host arithmetic), split the weights as planned, run.  The rules below were scan_amd/ops.py's
// _conv_split and, a second time, scan_ops_ext.cpp's; they read the knobs through the picker and the Winograd query above.
extern "C" int scan_conv_plan(int32_t pieces, int32_t taps, int32_t dgrad, int32_t O, int32_t Cs_w, int32_t Cs_src,
                              const scan_pyramid_t* od, int32_t flags, scan_conv_plan_t* plan) {
  const char* name = "conv_plan";
  SCAN_CHECK_ARG(plan != nullptr, "%s: null plan", name);
  SCAN_CHECK_ARG((pieces == 2 || pieces == 3) && (taps == 9 || taps == 1) && (dgrad == 0 || dgrad == 1), "%s: pieces=%d taps=%d dgrad=%d",
                 name, pieces, taps, dgrad);
  SCAN_CHECK_ARG(O > 0 && Cs_w > 0 && Cs_src > 0, "%s: O=%d Cs_w=%d Cs_src=%d", name, O, Cs_w, Cs_src);
  const bool sums = flags & SCAN_CONV_SUMS, pool = flags & SCAN_CONV_POOL;
  SCAN_CHECK_ARG((flags & ~(SCAN_CONV_SUMS | SCAN_CONV_POOL)) == 0 && !(sums && pool), "%s: flags=%d (sums or the pool)", name, flags);
  if (check_pyramid(name, od)) return -1;
  // plane rows are zero-padded to whole 32-channel K chunks for the 3x3 kernels: the LDS-DMA weight path needs whole chunks
  // (a 264-channel input then takes it too); 1x1 planes keep the 8-element granule
  const int32_t rnd = taps == 9 ? 32 : 8;
  scan_conv_plan_t p{};
  p.pieces = pieces, p.taps = taps, p.dgrad = dgrad, p.O = O, p.Cs_w = Cs_w, p.flags = flags;
  p.plane_rows = p.nout = dgrad ? Cs_w : O;
  p.csw = ((dgrad ? (O > Cs_src ? O : Cs_src) : Cs_w) + rnd - 1) / rnd * rnd;
  // 128-wide output tiles plus a small remainder (data gradient of the 264-channel discriminator input at P3, K = 1024): the
  // remainder columns go through the 64-channel instance instead of a third, almost empty 128-wide tile (2022 -> 1794 us).
  // With a short K loop or few rows the extra launch costs more than the empty tile (265-channel head_out input: 614 ->
  // 721 us), hence the size test.
  const int32_t rem = p.nout % 128;
  if (taps == 9 && !sums && !pool && p.nout > 128 && rem > 0 && rem <= 64 && Cs_src >= 512 && od->row_off[od->n_levels] >= 100000)
    p.rem = rem;
  // the Winograd F(2,3) kernel reads planes of its own: split modes 2 / 3, 12 taps per row
  const bool wino = pieces == 3 && taps == 9 && p.rem == 0 && scan_conv3x3_bf16x6_wino(p.nout, p.csw) == 1;
  p.family = wino ? SCAN_CONV_WINO3X3 : taps == 9 ? SCAN_CONV_DIRECT3X3 : SCAN_CONV_1X1;
  p.split_mode = dgrad + (wino ? 2 : 0);
  p.plane_taps = wino ? 12 : taps;
  // 3128: the Winograd instance (128-channel tile); the others as the scan_conv*_instance queries (whole K chunks)
  p.instance = wino ? 3128 : taps == 9 ? pick3x3(pieces, od, p.nout, true).id : pick1x1(pieces, od, p.nout, p.csw).id;
  *plan = p;
  return 0;
}

static int check_plan(const char* name, const scan_conv_plan_t* p) {
  SCAN_CHECK_ARG(p != nullptr, "%s: null plan", name);
  SCAN_CHECK_ARG((p->pieces == 2 || p->pieces == 3) && (p->taps == 9 || p->taps == 1) && p->nout > 0 && p->rem >= 0 && p->rem < p->nout &&
                     p->csw > 0 && p->family >= SCAN_CONV_DIRECT3X3 && p->family <= SCAN_CONV_1X1 &&
                     (p->family == SCAN_CONV_1X1) == (p->taps == 1) && (p->family != SCAN_CONV_WINO3X3 || (p->pieces == 3 && p->rem == 0)),
                 "%s: not a plan scan_conv_plan filled", name);
  return 0;
}

extern "C" int scan_conv_weight_split(const scan_conv_plan_t* plan, const float* w, void* p0, void* p1, void* p2, void* stream) {
  if (check_plan("conv_weight_split", plan)) return -1;
  return weight_split_launch(plan->pieces, w, plan->O, plan->taps, plan->Cs_w, plan->split_mode, p0, p1, p2, plan->csw, stream);
}

extern "C" int scan_conv_run(const scan_conv_plan_t* plan, const float* x, const scan_pyramid_t* xd, int32_t Cs, const void* p0,
                             const void* p1, const void* p2, const float* bias, const float* mask, float* y,
                             const scan_pyramid_t* yd, int32_t Ns, int32_t relu, int32_t map, float* gn_ws, int32_t clear,
                             void* stream) {
  const char* name = "conv_run";
  if (check_plan(name, plan)) return -1;
  const int np = plan->pieces, nout = plan->nout, csw = plan->csw;
  const bool sums = plan->flags & SCAN_CONV_SUMS, pool = plan->flags & SCAN_CONV_POOL;
  relu = relu ? 1 : 0;
  SCAN_CHECK_ARG(plan->taps == 9 || plan->flags == 0, "%s: sums and the fused pool are epilogues of the 3x3 kernels", name);
  SCAN_CHECK_ARG(!(pool && plan->dgrad), "%s: the fused pool is forward only", name);
  SCAN_CHECK_ARG(sums == (gn_ws != nullptr), "%s: a GroupNorm workspace goes with a plan for sums, and only with one", name);
  SCAN_CHECK_ARG(!(sums || pool) || mask == nullptr, "%s: no mask with sums or the fused pool", name);
  SCAN_CHECK_ARG(!sums || !relu, "%s: no ReLU with GroupNorm sums", name);
  switch (plan->family) {
    case SCAN_CONV_1X1:
      return conv1x1(name, np, x, xd, Cs, p0, p1, p2, csw, bias, mask, y, yd, nout, Ns, relu, map, stream);
    case SCAN_CONV_WINO3X3:
      return conv3x3_wino(name, x, xd, Cs, p0, p1, p2, csw, bias, mask, y, nout, Ns, relu | (pool ? 2 : 0), gn_ws, clear, stream);
    default:
      break;
  }
  if (sums) return conv3x3_gn(name, np, clear, x, xd, Cs, p0, p1, p2, csw, bias, y, nout, Ns, gn_ws, stream);
  if (pool && check_pool2(name, xd)) return -1;
  if (plan->rem == 0) return conv3x3(name, np, x, xd, Cs, p0, p1, p2, csw, bias, mask, y, nout, Ns, relu | (pool ? 2 : 0), stream);
  // main part on 128-wide tiles, then the remainder columns: planes, bias, mask and y move on by the main channels
  if (check3x3(name, np, x, xd, Cs, p0, p1, p2, csw, mask, y, nout, Ns)) return -1;
  const int32_t main = nout - plan->rem;
  const size_t wo = (size_t)main * plan->plane_taps * csw * sizeof(__bf16);
  auto at = [wo](const void* q) -> const void* { return q ? static_cast<const char*>(q) + wo : nullptr; };
  if (int rc = conv3x3(name, np, x, xd, Cs, p0, p1, p2, csw, bias, mask, y, main, Ns, relu, stream)) return rc;
  return conv3x3(name, np, x, xd, Cs, at(p0), at(p1), at(p2), csw, bias ? bias + main : nullptr, mask ? mask + main : nullptr,
                 y + main, plan->rem, Ns, relu, stream);
}

// ---- the weight-gradient dispatcher: plan (host arithmetic, the knobs are read here and only here), run what was planned.
// The routing was scan_amd/ops.py's _Conv2d.backward and, a second time, scan_ops_ext.cpp's conv_rows_backward.
extern "C" int scan_conv_wgrad_plan(int32_t pieces, int32_t ksize, int32_t stride, int32_t Cs, int32_t Cout, const scan_pyramid_t* xd,
                                    const scan_pyramid_t* yd, scan_conv_wgrad_plan_t* plan) {
  const char* name = "conv_wgrad_plan";
  SCAN_CHECK_ARG(plan != nullptr, "%s: null plan", name);
  SCAN_CHECK_ARG(pieces == 0 || pieces == 2 || pieces == 3, "%s: pieces=%d (0, 2 or 3)", name, pieces);
  if (check_pyramid(name, xd) || check_pyramid(name, yd)) return -1;
  if (pieces && ksize == 3 && stride == 1) return wgrad_split_plan(name, pieces, 3, 1, Cs, Cout, xd, plan);
  if (pieces && ksize == 1 && (stride == 1 || stride == 2)) return wgrad_split_plan(name, pieces, 1, stride, Cs, Cout, yd, plan);
  return wgrad_generic_plan(name, pieces, ksize, stride, Cs, Cout, yd, plan);
}

extern "C" int scan_conv_wgrad_run(const scan_conv_wgrad_plan_t* plan, const float* x, const scan_pyramid_t* xd, int32_t Cs,
                                   const float* dy, const scan_pyramid_t* yd, int32_t Cout, int32_t Cout_s, float* dw, float* db,
                                   int32_t accumulate, float* ws, void* stream) {
  const char* name = "conv_wgrad_run";
  SCAN_CHECK_ARG(plan != nullptr, "%s: null plan", name);
  SCAN_CHECK_ARG((accumulate & ~3) == 0, "%s: accumulate=%d (bit 0: dw, bit 1: db)", name, accumulate);
  auto run = plan->family == SCAN_WGRAD_GENERIC ? wgrad_generic_run : wgrad_split_run;  // each refuses a plan that is not its own
  return run(name, *plan, x, xd, Cs, dy, yd, Cout, Cout_s, dw, db, accumulate, ws, stream);
}

// the split families' entry points of before the plan: plan under the knobs of the moment (the *_ws_floats query, and again the
// launch), run; one accumulate flag for dw and db
static int64_t split_ws_floats(int np, int ksize, const scan_pyramid_t* d, int32_t Cs, int32_t Cout) {
  WgradPlan p;
  return wgrad_split_plan("wgrad_ws_floats", np, ksize, 1, Cs, Cout, d, &p) ? -1 : p.ws_floats;
}
static int split_wgrad(const char* name, int np, int ksize, int32_t stride, const float* x, const scan_pyramid_t* xd, int32_t Cs,
                       const float* dy, const scan_pyramid_t* yd, int32_t Cout, int32_t Cout_s, float* dw, float* db,
                       int32_t accumulate, float* ws, void* stream) {
  WgradPlan p;
  if (int rc = wgrad_split_plan(name, np, ksize, stride, Cs, Cout, ksize == 3 ? xd : yd, &p)) return rc;
  return wgrad_split_run(name, p, x, xd, Cs, dy, yd, Cout, Cout_s, dw, db, accumulate ? 3 : 0, ws, stream);
}
extern "C" int64_t scan_conv3x3_wgrad_bf16x3_ws_floats(const scan_pyramid_t* d, int32_t Cs, int32_t Cout) {
  return split_ws_floats(2, 3, d, Cs, Cout);
}
extern "C" int64_t scan_conv3x3_wgrad_bf16x6_ws_floats(const scan_pyramid_t* d, int32_t Cs, int32_t Cout) {
  return split_ws_floats(3, 3, d, Cs, Cout);
}
extern "C" int64_t scan_conv1x1_wgrad_bf16x3_ws_floats(const scan_pyramid_t* yd, int32_t Cs, int32_t Cout) {
  return split_ws_floats(2, 1, yd, Cs, Cout);
}
extern "C" int64_t scan_conv1x1_wgrad_bf16x6_ws_floats(const scan_pyramid_t* yd, int32_t Cs, int32_t Cout) {
  return split_ws_floats(3, 1, yd, Cs, Cout);
}
extern "C" int scan_conv3x3_wgrad_bf16x3(const float* x, const scan_pyramid_t* d, int32_t Cs, const float* dy,
                                         int32_t Cout, int32_t Cout_s, float* dw, float* db, int32_t accumulate,
                                         float* ws, void* stream) {
  return split_wgrad("conv3x3_wgrad_bf16x3", 2, 3, 1, x, d, Cs, dy, d, Cout, Cout_s, dw, db, accumulate, ws, stream);
}
extern "C" int scan_conv3x3_wgrad_bf16x6(const float* x, const scan_pyramid_t* d, int32_t Cs, const float* dy,
                                         int32_t Cout, int32_t Cout_s, float* dw, float* db, int32_t accumulate,
                                         float* ws, void* stream) {
  return split_wgrad("conv3x3_wgrad_bf16x6", 3, 3, 1, x, d, Cs, dy, d, Cout, Cout_s, dw, db, accumulate, ws, stream);
}
extern "C" int scan_conv1x1_wgrad_bf16x3(const float* x, const scan_pyramid_t* xd, int32_t Cs, const float* dy,
                                         const scan_pyramid_t* yd, int32_t Cout, int32_t Cout_s, int32_t stride,
                                         float* dw, float* db, int32_t accumulate, float* ws, void* stream) {
  return split_wgrad("conv1x1_wgrad_bf16x3", 2, 1, stride, x, xd, Cs, dy, yd, Cout, Cout_s, dw, db, accumulate, ws, stream);
}
extern "C" int scan_conv1x1_wgrad_bf16x6(const float* x, const scan_pyramid_t* xd, int32_t Cs, const float* dy,
                                         const scan_pyramid_t* yd, int32_t Cout, int32_t Cout_s, int32_t stride,
                                         float* dw, float* db, int32_t accumulate, float* ws, void* stream) {
  return split_wgrad("conv1x1_wgrad_bf16x6", 3, 1, stride, x, xd, Cs, dy, yd, Cout, Cout_s, dw, db, accumulate, ws, stream);
}
