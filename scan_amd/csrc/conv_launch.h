// Host-side launch layer of the split-operand forward / data-gradient convolutions (internal to libscan_hip.so).
//   conv_api.hip    the public entry points: validate the arguments, fill a ConvArgs, pick an instance, launch, check; and the
//                   dispatcher above them (scan_conv_plan / _weight_split / _run): planes, kernel family and launch cut of a conv,
//                   decided once for the Python and the C++ bindings
//   conv_fwd.hip    the production kernel, its instantiations and the picker that chooses among them
//   conv_gen1.hip   the first-generation kernel behind scan_tune("conv_v2", 0)
// and the scan_tune knobs of the whole library: each is DEFINED, with the measurements behind its default, next to the launch
// code that reads it; capi.cpp holds the table that names them.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "../../include/scan_hip.h"

extern int g_scan_conv_v2;                                                              // conv_api.hip
extern int g_scan_conv_bn256, g_scan_conv_wg1024, g_scan_conv_w8, g_scan_conv_tpb3;     // conv_fwd.hip
extern int g_scan_conv_glds, g_scan_conv_bn64_th16, g_scan_conv1x1;                     // conv_fwd.hip
extern int g_scan_conv_wino, g_scan_wino_tpb;                                           // conv_fwd.hip
extern int g_scan_wgrad_v6, g_scan_wgrad_prio, g_scan_wgrad_tile, g_scan_wgrad_wgs, g_scan_wgrad_wino;  // conv_wgrad.hip
extern int g_scan_gconv_mfma;                                                           // gconv.hip
extern int g_scan_dynconv_generic;                                                      // dynconv.hip
extern int g_scan_dbscan_bf16x3;                                                        // dbscan.hip
extern int g_scan_reduce_blocks;                                                        // pointwise.hip

// one forward / data-gradient launch, validated
struct ConvArgs {
  const float* x;
  const scan_pyramid_t* od;  // output pyramid (tiles are enumerated over it)
  const scan_pyramid_t* sd;  // source pyramid (== od unless a stride-2 1x1 map is in play)
  int32_t Cs;
  const __bf16* w[3];        // weight planes, hi first (w[2] only with three pieces)
  int32_t Csw;
  const float* bias;
  const float* mask;
  float* y;
  int32_t Nout, Ns, relu, map;
  hipStream_t st;
  double* gn_ws;
};

// The kernel instance a launch takes under the current knobs: the id the scan_conv*_instance queries report (bench.py labels
// its timings with it) and the launcher of the template instantiation that goes with it.  np = pieces per operand (2:
// "bf16x3", 3: "bf16x6"); whole_chunks: the weight planes have whole 32-channel K chunks (Csw % 32 == 0), which the LDS-DMA
// instances need.
struct ConvInst {
  int id;
  void (*launch)(const ConvArgs&);
};
ConvInst pick3x3(int np, const scan_pyramid_t* d, int32_t Nout, bool whole_chunks);
ConvInst pick1x1(int np, const scan_pyramid_t* yd, int32_t Nout, int32_t Csw);
// the Winograd F(2,3) instance (three pieces, Winograd planes, Nout > 64, whole chunks): scan_tune "wino_tpb" picks its schedule
void conv3x3_wino_launch(const ConvArgs& a);

// conv_gen1.hip: two pieces only
void gen1_conv3x3_launch(const ConvArgs& a);
void gen1_conv1x1_launch(const ConvArgs& a);
