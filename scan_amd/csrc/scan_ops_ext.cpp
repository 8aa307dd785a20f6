// C++ autograd entry points of the SCAN hot-path operators (BASELINE.json north_star: "registered behind the existing
// fcos_core.layers / fcos_core.modeling operator surface ... via PyTorch-ROCm C++ extensions"; SURVEY.md section 7 step 1
// names conv3x3_gn_relu_* and dynamic_conv_softmax_*).  Built by __graft_entry__.build() into
// scan_amd/ext/scan_ops/_ops<EXT_SUFFIX> (plain g++: host code only; every device operation is a call into libscan_hip.so
// through the C ABI of include/scan_hip.h, nothing of torch crosses that boundary).
//
// Every function takes and returns NCHW tensors the way the reference's modules call torch.nn (a channels_last NCHW tensor
// IS the kernels' pixel-major row matrix, so the adaptor is a view; any other layout is converted once on entry), records a
// torch::autograd::Function node, and runs forward AND backward without entering the Python interpreter:
//
//   conv2d(x, weight, bias, stride, relu)                      nn.Conv2d(k in {1, 3}, padding k // 2) [+ ReLU]
//        rpn/fcos/fcos.py:25-64, rpn/fcos/condgraph.py:86-106, backbone/fpn.py:52-66,118-130, backbone/mmdetection/vgg.py:8-33
//   conv3x3_gn_relu(x, weight, bias, gamma, beta, eps, relu)   the [Conv2d(3x3), GroupNorm(32, 256), ReLU] tower block
//        rpn/fcos/fcos.py:36-49, rpn/fcos/condgraph.py:99-105, discriminator/fcos_head_discriminator_con.py:20-34
//   group_norm_relu(x, gamma, beta, eps, relu)                 nn.GroupNorm(32, 256) [+ ReLU]
//   dynamic_conv_softmax(features, kernels)                    F.conv2d(x, kernel_par[K, 256, 1, 1]) + softmax(dim = 1)
//        rpn/fcos/condgraph.py:619-629,344-346
//
// Arithmetic: the reference's fp32 multiply / fp32 accumulate on the bf16 matrix cores ("bf16x6", scan_hip.h); 3x3 / stride 2
// (P6 / P7) on the exact fp32-MFMA kernels.  Which planes and which kernel a conv takes is the library's decision
// (scan_conv_plan), the one scan_amd.ops follows too -> bit-identical results (tests/test_gpu_kernels.py).
#include <ATen/ATen.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <torch/extension.h>

#include <map>
#include <utility>
#include <vector>

#include "../../include/scan_hip.h"

namespace {

using torch::autograd::AutogradContext;
using torch::autograd::variable_list;

void* cur_stream(const at::Tensor& t) { return c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(t.device().index()).stream(); }
void check(int rc, const char* what) { TORCH_CHECK(rc == 0, what, " failed (", rc, "): ", scan_last_error()); }
int64_t pad4(int64_t c) { return (c + 3) / 4 * 4; }

void require_gpu_f32(const at::Tensor& t, const char* who, const char* what) {
  TORCH_CHECK(t.is_cuda(), who, ": ", what, " must be a GPU tensor (the HIP kernels have no CPU fallback)");
  TORCH_CHECK(t.scalar_type() == at::kFloat, who, ": ", what, " must be float32");
}

scan_pyramid_t one_level(int64_t n, int64_t h, int64_t w) {
  scan_pyramid_t d{};
  d.n_levels = 1;
  d.n_images = (int32_t)n;
  d.h[0] = (int32_t)h;
  d.w[0] = (int32_t)w;
  d.row_off[0] = 0;
  d.row_off[1] = n * h * w;
  return d;
}

// [N, C, H, W] -> rows [N*H*W, pad4(C)] (zero-copy for channels_last tensors with C % 4 == 0)
at::Tensor to_rows(const at::Tensor& x) {
  const int64_t n = x.size(0), c = x.size(1), h = x.size(2), w = x.size(3);
  at::Tensor r = x.permute({0, 2, 3, 1});
  if (c % 4 != 0) r = at::constant_pad_nd(r, {0, pad4(c) - c}, 0);
  return r.contiguous().view({n * h * w, pad4(c)});
}
// rows [N*H*W, Cs] -> channels_last NCHW view of the first c channels
at::Tensor to_nchw(const at::Tensor& rows, int64_t n, int64_t h, int64_t w, int64_t c) {
  return rows.view({n, h, w, rows.size(1)}).slice(3, 0, c).permute({0, 3, 1, 2});
}
// weight [O, I, k, k] -> packed fp32 [O][k*k][pad4(I)] (what a channels_last weight is physically, channel-padded)
at::Tensor pack_weight(const at::Tensor& w) {
  const int64_t o = w.size(0), i = w.size(1), t = w.size(2) * w.size(3);
  at::Tensor p = w.permute({0, 2, 3, 1});
  if (i % 4 != 0) p = at::constant_pad_nd(p, {0, pad4(i) - i}, 0);
  return p.contiguous().view({o, t, pad4(i)});
}
// packed gradient [O][T][Cs] -> gradient of the logical weight [O, I, k, k] (channels_last strides like the parameter)
at::Tensor unpack_wgrad(const at::Tensor& dwp, int64_t i, int64_t k) {
  return dwp.view({dwp.size(0), k, k, dwp.size(2)}).slice(3, 0, i).permute({0, 3, 1, 2});
}

struct Planes {
  at::Tensor p[3];
};

// which planes, which kernel family, how the launch is cut: the library's one dispatcher (scan_conv_plan, scan_hip.h) -- the
// function scan_amd.ops asks, so the two bindings cannot disagree
scan_conv_plan_t conv_plan(int64_t taps, bool dgrad, int64_t o, int64_t cs_w, int64_t cs_src, const scan_pyramid_t& od, int flags) {
  scan_conv_plan_t plan;
  check(scan_conv_plan(3, (int32_t)taps, dgrad ? 1 : 0, (int32_t)o, (int32_t)cs_w, (int32_t)cs_src, &od, flags, &plan), "scan_conv_plan");
  return plan;
}

// ---- weight planes across calls.  A reference-shaped module graph calls the SAME conv once per pyramid level (rpn/fcos/fcos.py:
// 66-114 shares its towers over five levels), and every call would split the same fp32 weight into the same three bf16 planes
// again (forward + data gradient: 2 launches x 5 levels per layer).  The planes are kept per (storage address, shape, mode) and
// reused while the weight is provably unchanged: same at::Tensor version counter (every in-place update through torch bumps
// it -- torch.optim.SGD, load_state_dict, .data.copy_), same epoch (invalidate_weight_cache(): updates that bypass torch, like the
// engine's fused SGD on raw pointers, call it through scan_amd.ops.invalidate_weight_planes), same stream.
struct PlaneEntry {
  at::Tensor keep;  // the packed weight itself: while the entry lives its storage cannot be handed to another tensor
  uint32_t version;
  int64_t epoch;
  void* stream;
  int64_t o, t, cs;
  Planes pl;
};
int64_t g_plane_epoch = 0;
std::map<std::pair<const void*, int>, PlaneEntry>& plane_cache() {
  static std::map<std::pair<const void*, int>, PlaneEntry> c;
  return c;
}
void invalidate_weight_cache() {
  ++g_plane_epoch;
  plane_cache().clear();
}
// the three bf16 planes of packed weights wp [O][T][Cs] that `plan` reads (scan_conv_weight_split)
Planes split3_uncached(const at::Tensor& wp, const scan_conv_plan_t& plan) {
  Planes pl;
  for (auto& q : pl.p) q = at::empty({plan.plane_rows, plan.plane_taps, plan.csw}, wp.options().dtype(at::kBFloat16));
  check(scan_conv_weight_split(&plan, wp.data_ptr<float>(), pl.p[0].data_ptr(), pl.p[1].data_ptr(), pl.p[2].data_ptr(), cur_stream(wp)),
        "scan_conv_weight_split");
  return pl;
}
Planes split3(const at::Tensor& wp, const scan_conv_plan_t& plan, const at::Tensor& owner = at::Tensor()) {
  // owner: defined when wp is a VIEW of the weight tensor (pack_weight of a channels_last weight with C % 4 == 0: shares its storage
  // and its version counter) -- only then does the cache apply; a packed COPY is a fresh temporary every call
  if (!owner.defined() || owner.data_ptr() != wp.data_ptr()) return split3_uncached(wp, plan);
  const auto key = std::make_pair((const void*)wp.data_ptr(), (int)plan.split_mode);
  void* st = cur_stream(wp);
  auto& cache = plane_cache();
  auto it = cache.find(key);
  if (it != cache.end()) {
    const PlaneEntry& e = it->second;
    if (e.version == owner._version() && e.epoch == g_plane_epoch && e.stream == st && e.o == wp.size(0) && e.t == wp.size(1) &&
        e.cs == wp.size(2) && e.pl.p[0].size(2) == plan.csw)
      return e.pl;
  }
  if (cache.size() > 512) cache.clear();
  PlaneEntry e{wp, owner._version(), g_plane_epoch, st, wp.size(0), wp.size(1), wp.size(2), split3_uncached(wp, plan)};
  cache[key] = e;
  return e.pl;
}

// plan -> planes (cached) -> one scan_conv_run: y rows [.., Ns] of a conv reading x rows [.., Cs]
void conv_run(const scan_conv_plan_t& plan, const at::Tensor& wp, const at::Tensor& owner, const at::Tensor& x, const scan_pyramid_t& xd,
              int64_t cs, const at::Tensor& bias, at::Tensor& y, const scan_pyramid_t& yd, int64_t ns, bool relu, int map,
              const at::Tensor& gn_sums) {
  const Planes pl = split3(wp, plan, owner);
  check(scan_conv_run(&plan, x.data_ptr<float>(), &xd, (int32_t)cs, pl.p[0].data_ptr(), pl.p[1].data_ptr(), pl.p[2].data_ptr(),
                      bias.defined() ? bias.data_ptr<float>() : nullptr, nullptr, y.data_ptr<float>(), &yd, (int32_t)ns, relu ? 1 : 0, map,
                      gn_sums.defined() ? reinterpret_cast<float*>(gn_sums.data_ptr()) : nullptr, 1, cur_stream(x)),
        "scan_conv_run");
}

const float* opt_ptr(const at::Tensor& t) { return t.defined() ? t.data_ptr<float>() : nullptr; }

struct ConvGeom {
  int64_t n, cin, h, w, cout, k, stride, ho, wo, cs, ns;
};
ConvGeom geom(const at::Tensor& x, const at::Tensor& weight, int64_t stride, const char* who) {
  require_gpu_f32(x, who, "input");
  require_gpu_f32(weight, who, "weight");
  TORCH_CHECK(x.dim() == 4 && weight.dim() == 4, who, ": input [N, C, H, W] and weight [O, I, k, k]");
  TORCH_CHECK(weight.size(1) == x.size(1), who, ": weight expects ", weight.size(1), " input channels, got ", x.size(1));
  TORCH_CHECK(weight.size(2) == weight.size(3) && (weight.size(2) == 1 || weight.size(2) == 3), who,
              ": kernel size 1 or 3 (square), padding = k // 2 -- the convolutions the SCAN modules build");
  TORCH_CHECK(stride == 1 || stride == 2, who, ": stride 1 or 2");
  ConvGeom g;
  g.n = x.size(0), g.cin = x.size(1), g.h = x.size(2), g.w = x.size(3);
  g.cout = weight.size(0), g.k = weight.size(2), g.stride = stride;
  g.ho = (g.h - 1) / stride + 1, g.wo = (g.w - 1) / stride + 1;  // padding k // 2
  g.cs = pad4(g.cin), g.ns = pad4(g.cout);
  return g;
}

// ---- forward / backward of a conv on row matrices (shared by Conv2dFn and ConvGnReluFn) -------------------------------
// y rows [Mo, Ns]; gn_sums (defined): the epilogue accumulates the GroupNorm sums of the output there (3x3 / stride 1 only)
at::Tensor conv_rows_forward(const at::Tensor& xr, const at::Tensor& wp, const at::Tensor& bias, const ConvGeom& g, bool relu,
                             at::Tensor gn_sums, const at::Tensor& owner = at::Tensor()) {
  const scan_pyramid_t xd = one_level(g.n, g.h, g.w), yd = one_level(g.n, g.ho, g.wo);
  at::Tensor y = g.ns != g.cout ? at::zeros({yd.row_off[1], g.ns}, xr.options()) : at::empty({yd.row_off[1], g.ns}, xr.options());
  void* st = cur_stream(xr);
  if (g.k == 3 && g.stride == 2) {  // P6 / P7: exact fp32-MFMA kernel
    check(scan_conv2d_forward(xr.data_ptr<float>(), &xd, (int32_t)g.cs, wp.data_ptr<float>(), opt_ptr(bias), y.data_ptr<float>(), &yd,
                              (int32_t)g.cout, (int32_t)g.ns, 3, 2, relu ? 1 : 0, st),
          "scan_conv2d_forward");
    return y;
  }
  if (g.k == 3 && g.stride == 1 && g.cs == 4 && g.cout <= 64 && !gn_sums.defined()) {
    // the first layer (3 input channels, mmdetection/vgg.py conv1_1): the dedicated K = taps x 4 kernel, like scan_amd.ops
    check(scan_conv_smallcin_bf16x6(xr.data_ptr<float>(), (int32_t)g.n, (int32_t)g.h, (int32_t)g.w, wp.data_ptr<float>(), opt_ptr(bias),
                                    y.data_ptr<float>(), (int32_t)g.cout, (int32_t)g.ns, 3, 1, relu ? 1 : 0, st),
          "scan_conv_smallcin_bf16x6");
    return y;
  }
  // 3x3 / stride 1 and 1x1: Winograd, direct or 1x1 kernel as the library plans it (the launches scan_amd.ops makes: bit-identical)
  conv_run(conv_plan(g.k * g.k, false, g.cout, g.cs, g.cs, yd, gn_sums.defined() ? SCAN_CONV_SUMS : 0), wp, owner, xr, xd, g.cs, bias, y, yd,
           g.ns, relu, g.stride == 2 ? 1 : 0, gn_sums);
  return y;
}

// dyr rows [Mo, Ns] (the ReLU, if any, already backed out).  Returns {dx rows [Mi, Cs] or undefined, dw packed, db or undefined}
std::vector<at::Tensor> conv_rows_backward(const at::Tensor& xr, const at::Tensor& wp, const at::Tensor& dyr, const ConvGeom& g,
                                           bool need_dx, bool need_dw, bool need_db, const at::Tensor& owner = at::Tensor()) {
  const scan_pyramid_t xd = one_level(g.n, g.h, g.w), yd = one_level(g.n, g.ho, g.wo);
  void* st = cur_stream(xr);
  const int64_t T = g.k * g.k;
  at::Tensor dx, dw, db;
  if (need_dx) {
    dx = at::empty({xd.row_off[1], g.cs}, xr.options());
    if (g.k == 3 && g.stride == 2) {
      at::Tensor wt = at::empty({g.cs, T, g.ns}, xr.options());
      check(scan_weight_transpose(wp.data_ptr<float>(), (int32_t)g.cout, (int32_t)T, (int32_t)g.cs, wt.data_ptr<float>(), (int32_t)g.ns, st),
            "scan_weight_transpose");
      check(scan_conv2d_dgrad(dyr.data_ptr<float>(), &yd, (int32_t)g.ns, wt.data_ptr<float>(), dx.data_ptr<float>(), &xd, (int32_t)g.cs,
                              (int32_t)g.cs, 3, 2, nullptr, st),
            "scan_conv2d_dgrad");
    } else {
      // flipped + transposed planes: the data gradient is the forward kernel on dY
      conv_run(conv_plan(T, true, g.cout, g.cs, g.ns, xd, 0), wp, owner, dyr, yd, g.ns, at::Tensor(), dx, xd, g.cs, false,
               g.stride == 2 ? 2 : 0, at::Tensor());
    }
  }
  if (need_dw || need_db) {
    dw = at::empty({g.cout, T, g.cs}, xr.options());
    if (need_db) db = at::empty({g.cout}, xr.options());
    // family, kernel, split-K cut and workspace as the library plans them (the launches scan_amd.ops makes: bit-identical)
    scan_conv_wgrad_plan_t plan;
    check(scan_conv_wgrad_plan(3, (int32_t)g.k, (int32_t)g.stride, (int32_t)g.cs, (int32_t)g.cout, &xd, &yd, &plan), "scan_conv_wgrad_plan");
    at::Tensor ws = at::empty({plan.ws_floats}, xr.options());
    check(scan_conv_wgrad_run(&plan, xr.data_ptr<float>(), &xd, (int32_t)g.cs, dyr.data_ptr<float>(), &yd, (int32_t)g.cout, (int32_t)g.ns,
                              dw.data_ptr<float>(), need_db ? db.data_ptr<float>() : nullptr, 0, ws.data_ptr<float>(), st),
          "scan_conv_wgrad_run");
  }
  return {dx, dw, db};
}

// ---- nn.Conv2d (+ ReLU) ------------------------------------------------------------------------------------------------
// The Function nodes below take and return ROW MATRICES (fresh allocations, never views): the NCHW <-> rows adaptors are
// ordinary differentiable torch views applied by the free wrappers at the bottom, OUTSIDE apply().  An output that is a
// view created inside a custom Function may not be modified in place ("Output 0 of ...Backward is a view and is being
// modified inplace"), and the reference follows its convolutions with nn.ReLU(inplace=True)
// (backbone/mmdetection/vgg.py:29, modeling/make_layers.py:74,117).
ConvGeom geom_of(const std::vector<int64_t>& v) { return ConvGeom{v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9], v[10]}; }
std::vector<int64_t> geom_vec(const ConvGeom& g) { return {g.n, g.cin, g.h, g.w, g.cout, g.k, g.stride, g.ho, g.wo, g.cs, g.ns}; }

struct Conv2dFn : public torch::autograd::Function<Conv2dFn> {
  static at::Tensor forward(AutogradContext* ctx, at::Tensor xr, at::Tensor weight, c10::optional<at::Tensor> bias_opt,
                            std::vector<int64_t> gv, bool relu) {
    const at::Tensor bias = bias_opt.has_value() ? *bias_opt : at::Tensor();
    const ConvGeom g = geom_of(gv);
    c10::hip::HIPGuardMasqueradingAsCUDA guard(xr.device());
    at::Tensor wp = pack_weight(weight);
    at::Tensor bc = bias.defined() ? bias.contiguous() : bias;
    const bool wp_view = wp.data_ptr() == weight.data_ptr();
    at::Tensor y = conv_rows_forward(xr, wp, bc, g, relu, at::Tensor(), wp_view ? wp : at::Tensor());
    ctx->save_for_backward({xr, wp, relu ? y : at::Tensor()});
    ctx->saved_data["wp_view"] = wp_view;
    ctx->saved_data["geom"] = gv;
    ctx->saved_data["relu"] = relu;
    ctx->saved_data["has_bias"] = bias.defined();
    return y;
  }
  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    const auto saved = ctx->get_saved_variables();
    const at::Tensor xr = saved[0], wp = saved[1], y = saved[2];
    const ConvGeom g = geom_of(ctx->saved_data["geom"].toIntVector());
    c10::hip::HIPGuardMasqueradingAsCUDA guard(xr.device());
    at::Tensor dyr = grads[0].contiguous();
    if (ctx->saved_data["relu"].toBool()) {
      at::Tensor t = at::empty_like(dyr);
      check(scan_relu_backward(dyr.data_ptr<float>(), y.data_ptr<float>(), t.data_ptr<float>(), dyr.numel(), cur_stream(dyr)),
            "scan_relu_backward");
      dyr = t;
    }
    const bool has_bias = ctx->saved_data["has_bias"].toBool();
    auto r = conv_rows_backward(xr, wp, dyr, g, ctx->needs_input_grad(0), ctx->needs_input_grad(1),
                                has_bias && ctx->needs_input_grad(2), ctx->saved_data["wp_view"].toBool() ? wp : at::Tensor());
    at::Tensor dw = (r[1].defined() && ctx->needs_input_grad(1)) ? unpack_wgrad(r[1], g.cin, g.k) : at::Tensor();
    return {r[0], dw, r[2], at::Tensor(), at::Tensor()};
  }
};

// ---- nn.GroupNorm(32, 256) (+ ReLU) on rows ------------------------------------------------------------------------------
constexpr int kGroups = 32;

// statistics from x or from a conv epilogue's sums, atomic or ordered reductions, workspace sizes: the library's one plan
// (scan_groupnorm_plan, scan_hip.h), the only reader of scan_tune "deterministic" -- the function scan_amd.ops asks too
scan_groupnorm_plan_t gn_plan(int64_t c, const scan_pyramid_t& d, int flags) {
  scan_groupnorm_plan_t plan;
  check(scan_groupnorm_plan(&d, (int32_t)c, kGroups, flags, &plan), "scan_groupnorm_plan");
  return plan;
}
float* f64_ptr(const at::Tensor& t) { return t.defined() ? reinterpret_cast<float*>(t.data_ptr()) : nullptr; }

// y = GroupNorm(xr) (+ ReLU) as planned, (mean, rstd) -> stats; sums: the conv epilogue's where the plan's source says so
at::Tensor gn_rows_forward(const scan_groupnorm_plan_t& plan, const at::Tensor& xr, const scan_pyramid_t& d, const at::Tensor& sums,
                           const at::Tensor& gamma, const at::Tensor& beta, double eps, bool relu, at::Tensor& stats) {
  stats = at::empty({plan.stats_floats}, xr.options());
  at::Tensor y = at::empty_like(xr), ws;
  if (plan.source == SCAN_GN_FROM_X) ws = at::empty({plan.fwd_ws_doubles}, xr.options().dtype(at::kDouble));
  check(scan_groupnorm_run_forward(&plan, xr.data_ptr<float>(), &d, f64_ptr(sums), (float)eps, gamma.data_ptr<float>(), beta.data_ptr<float>(),
                                   relu ? 1 : 0, y.data_ptr<float>(), (int32_t)xr.size(1), stats.data_ptr<float>(), f64_ptr(ws), cur_stream(xr)),
        "scan_groupnorm_run_forward");
  return y;
}

at::Tensor gn_rows_backward(const at::Tensor& xr, const at::Tensor& gamma, const at::Tensor& beta, const at::Tensor& stats,
                            const at::Tensor& dyr, const scan_pyramid_t& d, bool relu, at::Tensor& dgamma, at::Tensor& dbeta) {
  const int64_t C = xr.size(1);
  const scan_groupnorm_plan_t plan = gn_plan(C, d, 0);  // under the knob of the moment, as the forward's
  at::Tensor dx = at::empty_like(xr), ws = at::empty({plan.bwd_ws_doubles}, xr.options().dtype(at::kDouble));
  dgamma = at::empty({C}, xr.options());
  dbeta = at::empty({C}, xr.options());
  check(scan_groupnorm_run_backward(&plan, xr.data_ptr<float>(), beta.data_ptr<float>(), dyr.data_ptr<float>(), (int32_t)C, &d,
                                    stats.data_ptr<float>(), gamma.data_ptr<float>(), relu ? 1 : 0, dx.data_ptr<float>(),
                                    dgamma.data_ptr<float>(), dbeta.data_ptr<float>(), 0, f64_ptr(ws), 0, cur_stream(xr)),
        "scan_groupnorm_run_backward");
  return dx;
}

struct GroupNormReluFn : public torch::autograd::Function<GroupNormReluFn> {
  static at::Tensor forward(AutogradContext* ctx, at::Tensor xr, at::Tensor gamma, at::Tensor beta, std::vector<int64_t> dims,
                            double eps, bool relu) {
    c10::hip::HIPGuardMasqueradingAsCUDA guard(xr.device());
    const int64_t n = dims[0], c = dims[1], h = dims[2], w = dims[3];
    const scan_pyramid_t d = one_level(n, h, w);
    at::Tensor gc = gamma.contiguous(), bc = beta.contiguous();
    at::Tensor stats;
    at::Tensor y = gn_rows_forward(gn_plan(c, d, 0), xr, d, at::Tensor(), gc, bc, eps, relu, stats);
    ctx->save_for_backward({xr, gc, bc, stats});
    ctx->saved_data["dims"] = dims;
    ctx->saved_data["relu"] = relu;
    return y;
  }
  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    const auto s = ctx->get_saved_variables();
    const auto v = ctx->saved_data["dims"].toIntVector();
    c10::hip::HIPGuardMasqueradingAsCUDA guard(s[0].device());
    const scan_pyramid_t d = one_level(v[0], v[2], v[3]);
    at::Tensor dg, db;
    at::Tensor dx = gn_rows_backward(s[0], s[1], s[2], s[3], grads[0].contiguous(), d, ctx->saved_data["relu"].toBool(), dg, db);
    return {dx, dg, db, at::Tensor(), at::Tensor(), at::Tensor()};
  }
};

// ---- [Conv2d(3x3, stride 1), GroupNorm(32, 256), ReLU]: the tower block, GroupNorm sums from the conv epilogue ------------
struct ConvGnReluFn : public torch::autograd::Function<ConvGnReluFn> {
  static at::Tensor forward(AutogradContext* ctx, at::Tensor xr, at::Tensor weight, c10::optional<at::Tensor> bias_opt, at::Tensor gamma,
                            at::Tensor beta, std::vector<int64_t> gv, double eps, bool relu) {
    const at::Tensor bias = bias_opt.has_value() ? *bias_opt : at::Tensor();
    const ConvGeom g = geom_of(gv);
    c10::hip::HIPGuardMasqueradingAsCUDA guard(xr.device());
    at::Tensor wp = pack_weight(weight), gc = gamma.contiguous(), bc = beta.contiguous();
    at::Tensor cb = bias.defined() ? bias.contiguous() : bias;
    const scan_pyramid_t d = one_level(g.n, g.h, g.w);
    // the plan says whether the conv accumulates the GroupNorm sums in its epilogue (not in deterministic mode: they are atomic)
    const scan_groupnorm_plan_t plan = gn_plan(g.ns, d, SCAN_GN_SUMS);
    at::Tensor sums = plan.source == SCAN_GN_FROM_X ? at::Tensor() : at::empty({plan.stats_floats}, xr.options().dtype(at::kDouble));  // cleared by the conv launch
    const bool wp_view = wp.data_ptr() == weight.data_ptr();
    at::Tensor c = conv_rows_forward(xr, wp, cb, g, false, sums, wp_view ? wp : at::Tensor());
    ctx->saved_data["wp_view"] = wp_view;
    at::Tensor stats;
    at::Tensor y = gn_rows_forward(plan, c, d, sums, gc, bc, eps, relu, stats);
    ctx->save_for_backward({xr, wp, c, gc, bc, stats});
    ctx->saved_data["geom"] = gv;
    ctx->saved_data["relu"] = relu;
    ctx->saved_data["has_bias"] = bias.defined();
    return y;
  }
  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    const auto s = ctx->get_saved_variables();
    const ConvGeom g = geom_of(ctx->saved_data["geom"].toIntVector());
    c10::hip::HIPGuardMasqueradingAsCUDA guard(s[0].device());
    const scan_pyramid_t d = one_level(g.n, g.h, g.w);
    at::Tensor dgamma, dbeta;
    at::Tensor dc = gn_rows_backward(s[2], s[3], s[4], s[5], grads[0].contiguous(), d, ctx->saved_data["relu"].toBool(), dgamma, dbeta);
    const bool has_bias = ctx->saved_data["has_bias"].toBool();
    auto r = conv_rows_backward(s[0], s[1], dc, g, ctx->needs_input_grad(0), ctx->needs_input_grad(1), has_bias && ctx->needs_input_grad(2),
                                ctx->saved_data["wp_view"].toBool() ? s[1] : at::Tensor());
    at::Tensor dw = (r[1].defined() && ctx->needs_input_grad(1)) ? unpack_wgrad(r[1], g.cin, g.k) : at::Tensor();
    return {r[0], dw, r[2], dgamma, dbeta, at::Tensor(), at::Tensor(), at::Tensor()};
  }
};

// ---- semantic-conditioned dynamic conv + softmax ---------------------------------------------------------------------------
struct DynConvSoftmaxFn : public torch::autograd::Function<DynConvSoftmaxFn> {
  static variable_list forward(AutogradContext* ctx, at::Tensor fr, at::Tensor kernels, int64_t c) {
    c10::hip::HIPGuardMasqueradingAsCUDA guard(fr.device());
    const int64_t K = kernels.size(0);
    at::Tensor kc = kernels.contiguous();
    const int64_t M = fr.size(0);
    at::Tensor logits = at::empty({M, K}, fr.options()), probs = at::empty({M, K}, fr.options());
    check(scan_dynconv_softmax_forward(fr.data_ptr<float>(), kc.data_ptr<float>(), M, (int32_t)c, (int32_t)K, logits.data_ptr<float>(),
                                       probs.data_ptr<float>(), cur_stream(fr)),
          "scan_dynconv_softmax_forward");
    ctx->save_for_backward({fr, kc, probs});
    ctx->saved_data["c"] = c;
    return {logits, probs};
  }
  static variable_list backward(AutogradContext* ctx, variable_list grads) {
    const auto s = ctx->get_saved_variables();
    const int64_t c = ctx->saved_data["c"].toInt(), K = s[1].size(0), M = s[0].size(0);
    c10::hip::HIPGuardMasqueradingAsCUDA guard(s[0].device());
    auto rows = [&](const at::Tensor& g) { return g.defined() ? g.contiguous() : g; };
    at::Tensor dl = rows(grads[0]), dp = rows(grads[1]);
    at::Tensor dfeat = at::empty_like(s[0]), dk = at::empty_like(s[1]);
    at::Tensor ws = at::empty({scan_dynconv_ws_floats(M, (int32_t)c, (int32_t)K)}, s[0].options());
    check(scan_dynconv_softmax_backward(s[0].data_ptr<float>(), s[1].data_ptr<float>(), s[2].data_ptr<float>(), opt_ptr(dl), opt_ptr(dp), M,
                                        (int32_t)c, (int32_t)K, dfeat.data_ptr<float>(), dk.data_ptr<float>(), ws.data_ptr<float>(),
                                        cur_stream(s[0])),
          "scan_dynconv_softmax_backward");
    return {dfeat, dk, at::Tensor()};
  }
};

// ---- the NCHW surface: checks + layout adaptors (differentiable views) around the row-matrix nodes ----------------------------
at::Tensor conv2d(const at::Tensor& x, const at::Tensor& weight, const c10::optional<at::Tensor>& bias, int64_t stride, bool relu) {
  const ConvGeom g = geom(x, weight, stride, "conv2d");
  if (bias.has_value() && bias->defined()) require_gpu_f32(*bias, "conv2d", "bias");
  at::Tensor y = Conv2dFn::apply(to_rows(x), weight, bias, geom_vec(g), relu);
  return to_nchw(y, g.n, g.ho, g.wo, g.cout);
}
at::Tensor conv3x3_gn_relu(const at::Tensor& x, const at::Tensor& weight, const c10::optional<at::Tensor>& bias, const at::Tensor& gamma,
                           const at::Tensor& beta, double eps, bool relu) {
  const ConvGeom g = geom(x, weight, 1, "conv3x3_gn_relu");
  TORCH_CHECK(g.k == 3 && g.cout == 256, "conv3x3_gn_relu: a 3x3 conv into GroupNorm(32, 256) (the SCAN tower block)");
  require_gpu_f32(gamma, "conv3x3_gn_relu", "GroupNorm weight");
  require_gpu_f32(beta, "conv3x3_gn_relu", "GroupNorm bias");
  TORCH_CHECK(gamma.numel() == 256 && beta.numel() == 256, "conv3x3_gn_relu: GroupNorm weight / bias of 256 channels");
  at::Tensor y = ConvGnReluFn::apply(to_rows(x), weight, bias, gamma, beta, geom_vec(g), eps, relu);
  return to_nchw(y, g.n, g.h, g.w, g.cout);
}
at::Tensor group_norm_relu(const at::Tensor& x, const at::Tensor& gamma, const at::Tensor& beta, double eps, bool relu) {
  require_gpu_f32(x, "group_norm_relu", "input");
  require_gpu_f32(gamma, "group_norm_relu", "weight");
  require_gpu_f32(beta, "group_norm_relu", "bias");
  TORCH_CHECK(x.dim() == 4, "group_norm_relu: input [N, C, H, W]");
  const int64_t n = x.size(0), c = x.size(1), h = x.size(2), w = x.size(3);
  TORCH_CHECK(c % kGroups == 0 && c % 4 == 0, "group_norm_relu: ", c, " channels do not divide into ", kGroups, " groups of whole float4s");
  TORCH_CHECK(gamma.numel() == c && beta.numel() == c, "group_norm_relu: weight / bias must hold ", c, " elements");
  at::Tensor y = GroupNormReluFn::apply(to_rows(x), gamma, beta, std::vector<int64_t>{n, c, h, w}, eps, relu);
  return to_nchw(y, n, h, w, c);
}
std::vector<at::Tensor> dynamic_conv_softmax(const at::Tensor& features, const at::Tensor& kernels) {
  require_gpu_f32(features, "dynamic_conv_softmax", "features");
  require_gpu_f32(kernels, "dynamic_conv_softmax", "kernel_par");
  TORCH_CHECK(features.dim() == 4 && kernels.dim() == 2 && kernels.size(1) == features.size(1),
              "dynamic_conv_softmax: features [N, C, H, W], kernel_par [K, C]");
  const int64_t n = features.size(0), c = features.size(1), h = features.size(2), w = features.size(3), K = kernels.size(0);
  auto out = DynConvSoftmaxFn::apply(to_rows(features), kernels, c);
  auto back = [&](const at::Tensor& t) { return t.view({n, h, w, K}).permute({0, 3, 1, 2}); };
  return {back(out[0]), back(out[1])};
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "SCAN hot-path operators with C++ autograd on libscan_hip.so (MI355X / gfx950)";
  m.def("conv2d", &conv2d, "nn.Conv2d(k in {1, 3}, padding k // 2) [+ ReLU], NCHW in / out", py::arg("input"), py::arg("weight"),
        py::arg("bias") = py::none(), py::arg("stride") = 1, py::arg("relu") = false);
  m.def("conv3x3_gn_relu", &conv3x3_gn_relu, "[Conv2d(3x3), GroupNorm(32, 256), ReLU] tower block, NCHW in / out", py::arg("input"),
        py::arg("weight"), py::arg("bias"), py::arg("gn_weight"), py::arg("gn_bias"), py::arg("eps") = 1e-5, py::arg("relu") = true);
  m.def("group_norm_relu", &group_norm_relu, "nn.GroupNorm(32, 256) [+ ReLU], NCHW in / out", py::arg("input"), py::arg("weight"),
        py::arg("bias"), py::arg("eps") = 1e-5, py::arg("relu") = false);
  m.def("dynamic_conv_softmax", &dynamic_conv_softmax, "F.conv2d(x, kernel_par[K, C, 1, 1]) + softmax(dim = 1) -> (logits, probs)",
        py::arg("features"), py::arg("kernel_par"));
  m.def("scan_abi_version", []() { return scan_abi_version(); });
  m.def("invalidate_weight_cache", &invalidate_weight_cache,
        "drop the cached bf16 weight planes: call after updating parameters through anything but torch's own in-place ops");
  m.def("weight_cache_size", []() { return (int64_t)plane_cache().size(); });
}
