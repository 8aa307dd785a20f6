// Host-side launch layer of the convolutions (internal to libscan_hip.so).  Forward / data gradient, split operands:
//   conv_api.hip    the public entry points: validate the arguments, fill a ConvArgs, pick an instance, launch, check; and the
//                   dispatcher above them (scan_conv_plan / _weight_split / _run): planes, kernel family and launch cut of a conv,
//                   decided once for the Python and the C++ bindings
//   conv_fwd.hip    the production kernel, its instantiations and the picker that chooses among them
//   conv_gen1.hip   the first-generation kernel behind scan_tune("conv_v2", 0)
// weight gradient (the plan below; scan_conv_wgrad_plan / _run in conv_api.hip route to the file that owns the family):
//   conv_wgrad.hip  the split 3x3 and 1x1 families
//   conv_mfma.hip   the generic fp32-MFMA family and the column sums behind its bias gradient
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
extern int g_scan_reduce_blocks;                                                        // losses.hip

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

// ---- weight gradient.  The plan of a launch IS the public struct (include/scan_hip.h documents it field by field): a *_plan
// function validates the shape, reads the knobs -- the only place they are read -- and fills it; a *_run function re-derives
// the layout from the plan's shape, variant and splits, refuses a plan that differs, and launches.  The old entry points and
// their *_ws_floats queries are plan (+ run) under the current knobs.
typedef scan_conv_wgrad_plan_t WgradPlan;
// conv_wgrad.hip; d: the pyramid the K chunks walk (3x3: x's, 1x1: dy's)
int wgrad_split_plan(const char* name, int np, int ksize, int stride, int32_t Cs, int32_t Cout, const scan_pyramid_t* d, WgradPlan* p);
int wgrad_split_run(const char* name, const WgradPlan& p, const float* x, const scan_pyramid_t* xd, int32_t Cs, const float* dy,
                    const scan_pyramid_t* yd, int32_t Cout, int32_t Cout_s, float* dw, float* db, int32_t accumulate, float* ws,
                    void* stream);
// conv_mfma.hip
int wgrad_generic_plan(const char* name, int np, int ksize, int stride, int32_t Cs, int32_t Cout, const scan_pyramid_t* yd, WgradPlan* p);
int wgrad_generic_run(const char* name, const WgradPlan& p, const float* x, const scan_pyramid_t* xd, int32_t Cs, const float* dy,
                      const scan_pyramid_t* yd, int32_t Cout, int32_t Cout_s, float* dw, float* db, int32_t accumulate, float* ws,
                      void* stream);
