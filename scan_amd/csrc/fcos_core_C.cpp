// The compiled module the reference imports as ``fcos_core._C`` (reference fcos_core/csrc/vision.cpp:8-17, built by its
// setup.py:41-50 from csrc/{cpu,cuda}/*): the same function names, at::Tensor signatures, argument meaning and error
// behaviour, for all eight functions -- backed by libscan_hip.so through the C ABI of
// include/scan_hip.h (plain pointers, sizes and a hipStream_t; nothing of torch crosses that boundary).
//
//   nms(dets [n,4], scores [n], threshold[, cuda_rule]) -> int64 [k]                       csrc/nms.h:10-30
//     GPU tensors: libscan_hip.so; CPU tensors (float / double): the host loop below           csrc/cpu/nms_cpu.cpp:5-75
//     tie rule: IoU >= threshold suppresses (nms_cpu.cpp:60, what tests/test_nms.py pins) unless cuda_rule = True or
//     SCAN_NMS_RULE=gt is set in the environment: then IoU > threshold (csrc/cuda/nms.cu:60)
//   ml_nms(dets [n,4], scores [n], labels [n] float, threshold) -> int64 [k]              csrc/ml_nms.h:10-29
//   sigmoid_focalloss_forward(logits [M,C], targets [M] int32, C, gamma, alpha) -> [M,C]  csrc/SigmoidFocalLoss.h:10-24
//   sigmoid_focalloss_backward(logits, targets, d_losses, C, gamma, alpha) -> [M,C]       csrc/SigmoidFocalLoss.h:26-41
//   roi_align_forward(input [N,C,H,W], rois [K,5], scale, PH, PW, sampling_ratio) -> [K,C,PH,PW]   csrc/ROIAlign.h:11-25
//     GPU tensors: libscan_hip.so (csrc/roi.hip); CPU tensors (float / double): the host loop below   csrc/cpu/ROIAlign_cpu.cpp
//   roi_align_backward(grad, rois, scale, PH, PW, N, C, H, W, sampling_ratio) -> [N,C,H,W]           csrc/ROIAlign.h:27-45
//   roi_pool_forward(input, rois, scale, PH, PW) -> (output, argmax int32) [K,C,PH,PW]               csrc/ROIPool.h:10-25
//   roi_pool_backward(grad, input, rois, argmax, scale, PH, PW, N, C, H, W) -> [N,C,H,W]             csrc/ROIPool.h:27-47
//     the last three: GPU tensors only ("Not implemented on the CPU", as the reference's dispatchers)
//
// Built by __graft_entry__.build() (plain g++: no device code in this file) into
// scan_amd/ext/fcos_core/_C<EXT_SUFFIX>; with scan_amd/ext on sys.path, ``from fcos_core import _C`` is this module and
// the reference's layers/nms.py:4-7 and layers/sigmoid_focal_loss.py:9-36 run on it unchanged.
#include <ATen/ATen.h>
// PyTorch-ROCm tensors carry the device type "cuda": guard and stream come from the masquerading wrappers (the plain
// c10::hip::HIPGuard insists on DeviceType::HIP and throws on them)
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <torch/extension.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <vector>

#include "../../include/scan_hip.h"

namespace {

void* current_stream(const at::Tensor& t) { return c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(t.device().index()).stream(); }

void check(int rc, const char* what) { TORCH_CHECK(rc == 0, what, " failed (", rc, "): ", scan_last_error()); }

// Greedy NMS on host memory, the reference's CPU semantics (csrc/cpu/nms_cpu.cpp:5-65): candidates by descending score
// (equal scores: lower index first), a kept box suppresses every later one whose IoU (areas with the +1 pixel rule, in
// the tensors' own precision) reaches the threshold; kept ORIGINAL indices ascending.
template <typename T>
at::Tensor nms_host(const at::Tensor& dets_in, const at::Tensor& scores_in, float threshold, bool rule_ge) {
  const at::Tensor dets = dets_in.contiguous(), scores = scores_in.contiguous();
  const int64_t n = dets.size(0);
  const T* box = dets.data_ptr<T>();
  const T* sc = scores.data_ptr<T>();
  std::vector<int64_t> by_score(n);
  std::iota(by_score.begin(), by_score.end(), int64_t{0});
  std::stable_sort(by_score.begin(), by_score.end(), [sc](int64_t a, int64_t b) { return sc[a] > sc[b]; });
  std::vector<T> area(n);
  for (int64_t i = 0; i < n; ++i) area[i] = (box[4 * i + 2] - box[4 * i] + 1) * (box[4 * i + 3] - box[4 * i + 1] + 1);
  std::vector<char> dead(n, 0);
  for (int64_t r = 0; r < n; ++r) {
    const int64_t i = by_score[r];
    if (dead[i]) continue;
    const T* a = box + 4 * i;
    for (int64_t q = r + 1; q < n; ++q) {
      const int64_t j = by_score[q];
      if (dead[j]) continue;
      const T* b = box + 4 * j;
      const T w = std::max(T(0), std::min(a[2], b[2]) - std::max(a[0], b[0]) + 1);
      const T h = std::max(T(0), std::min(a[3], b[3]) - std::max(a[1], b[1]) + 1);
      const T inter = w * h;
      const T iou = inter / (area[i] + area[j] - inter);
      if (rule_ge ? iou >= threshold : iou > threshold) dead[j] = 1;
    }
  }
  std::vector<int64_t> kept;
  for (int64_t i = 0; i < n; ++i)
    if (!dead[i]) kept.push_back(i);
  at::Tensor out = at::empty({(int64_t)kept.size()}, at::TensorOptions().dtype(at::kLong).device(at::kCPU));
  if (!kept.empty()) std::memcpy(out.data_ptr<int64_t>(), kept.data(), kept.size() * sizeof(int64_t));
  return out;
}

at::Tensor nms_impl(const at::Tensor& dets_in, const at::Tensor& scores_in, const at::Tensor* labels_in, float threshold,
                    int rule_ge, const char* who) {
  if (dets_in.numel() == 0)  // csrc/nms.h:17-18: an empty CPU int64 tensor whatever the device
    return at::empty({0}, dets_in.options().dtype(at::kLong).device(at::kCPU));
  TORCH_CHECK(dets_in.dim() == 2 && dets_in.size(1) == 4, who, ": dets must be [n, 4]");
  const int64_t n = dets_in.size(0);
  TORCH_CHECK(scores_in.numel() == n, who, ": scores must have one entry per box");
  if (!dets_in.is_cuda()) {
    TORCH_CHECK(labels_in == nullptr, who, ": not implemented on the CPU");  // csrc/ml_nms.h:26
    TORCH_CHECK(!scores_in.is_cuda(), "scores must be a CPU tensor");                                   // nms_cpu.cpp:10
    TORCH_CHECK(dets_in.scalar_type() == scores_in.scalar_type(), "dets should have the same type as scores");  // :11
    if (dets_in.scalar_type() == at::kDouble) return nms_host<double>(dets_in, scores_in, threshold, rule_ge != 0);
    TORCH_CHECK(dets_in.scalar_type() == at::kFloat, who, ": float or double boxes (AT_DISPATCH_FLOATING_TYPES, nms_cpu.cpp:71)");
    return nms_host<float>(dets_in, scores_in, threshold, rule_ge != 0);
  }
  TORCH_CHECK(n <= SCAN_NMS_MAX, who, ": n=", n, " exceeds SCAN_NMS_MAX=", SCAN_NMS_MAX);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(dets_in.device());
  const at::Tensor dets = dets_in.contiguous().to(at::kFloat), scores = scores_in.contiguous().to(at::kFloat);
  at::Tensor labels;
  if (labels_in != nullptr) {
    TORCH_CHECK(labels_in->numel() == n, who, ": labels must have one entry per box");
    labels = labels_in->contiguous().to(at::kFloat);
  }
  at::Tensor ws = at::empty({(scan_nms_ws_bytes(n) + 15) / 16 * 2}, dets.options().dtype(at::kDouble));
  at::Tensor keep = at::empty({n}, dets.options().dtype(at::kLong));
  at::Tensor cnt = at::empty({1}, dets.options().dtype(at::kInt));
  check(scan_nms(dets.data_ptr<float>(), scores.data_ptr<float>(), labels.defined() ? labels.data_ptr<float>() : nullptr, n,
                 threshold, rule_ge, keep.data_ptr<int64_t>(), cnt.data_ptr<int32_t>(), ws.data_ptr(), current_stream(dets)),
        who);
  return keep.slice(0, 0, cnt.item<int32_t>());  // kept ORIGINAL indices, ascending (csrc/cpu/nms_cpu.cpp:64)
}

bool env_cuda_rule() {
  const char* e = std::getenv("SCAN_NMS_RULE");
  return e != nullptr && (std::strcmp(e, "gt") == 0 || std::strcmp(e, "cuda") == 0);
}

// Default: IoU >= threshold suppresses -- the reference's CPU rule (csrc/cpu/nms_cpu.cpp:60), which its own tests/test_nms.py
// pins.  cuda_rule = true (or SCAN_NMS_RULE=gt): IoU > threshold, what the reference's GPU build computes (cuda/nms.cu:60).
at::Tensor nms(const at::Tensor& dets, const at::Tensor& scores, const float threshold, const bool cuda_rule) {
  return nms_impl(dets, scores, nullptr, threshold, (cuda_rule || env_cuda_rule()) ? 0 : 1, "nms");
}

// label-aware, IoU > threshold suppresses: the reference's CUDA rule (csrc/cuda/ml_nms.cu:13-24,62); no CPU version exists
at::Tensor ml_nms(const at::Tensor& dets, const at::Tensor& scores, const at::Tensor& labels, const float threshold) {
  return nms_impl(dets, scores, &labels, threshold, 0, "ml_nms");
}

at::Tensor sigmoid_focalloss_forward(const at::Tensor& logits_in, const at::Tensor& targets_in, const int num_classes,
                                     const float gamma, const float alpha) {
  TORCH_CHECK(logits_in.is_cuda(), "Not implemented on the CPU");              // csrc/SigmoidFocalLoss.h:23
  TORCH_CHECK(targets_in.is_cuda(), "targets must be a CUDA tensor");          // SigmoidFocalLoss_cuda.cu:110
  TORCH_CHECK(logits_in.dim() == 2, "logits should be NxClass");               // :112
  TORCH_CHECK(logits_in.size(1) == num_classes, "logits.size(1) should be num_classes");
  TORCH_CHECK(targets_in.scalar_type() == at::kInt, "targets must be int32 (the reference passes targets.int())");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(logits_in.device());
  const at::Tensor logits = logits_in.contiguous().to(at::kFloat), targets = targets_in.contiguous();
  at::Tensor losses = at::empty_like(logits);
  check(scan_sigmoid_focal_loss_forward(logits.data_ptr<float>(), targets.data_ptr<int32_t>(), logits.size(0), num_classes,
                                        gamma, alpha, losses.data_ptr<float>(), nullptr, current_stream(logits)),
        "sigmoid_focalloss_forward");
  return losses;
}

at::Tensor sigmoid_focalloss_backward(const at::Tensor& logits_in, const at::Tensor& targets_in, const at::Tensor& d_losses_in,
                                      const int num_classes, const float gamma, const float alpha) {
  TORCH_CHECK(logits_in.is_cuda(), "Not implemented on the CPU");              // csrc/SigmoidFocalLoss.h:39
  TORCH_CHECK(targets_in.is_cuda() && d_losses_in.is_cuda(), "targets and d_losses must be CUDA tensors");
  TORCH_CHECK(logits_in.dim() == 2 && logits_in.size(1) == num_classes, "logits.size(1) should be num_classes");  // :158
  TORCH_CHECK(targets_in.scalar_type() == at::kInt, "targets must be int32 (the reference passes targets.int())");
  TORCH_CHECK(d_losses_in.sizes() == logits_in.sizes(), "d_losses must have the shape of logits");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(logits_in.device());
  const at::Tensor logits = logits_in.contiguous().to(at::kFloat), targets = targets_in.contiguous(),
                   d_losses = d_losses_in.contiguous().to(at::kFloat);
  at::Tensor d_logits = at::empty_like(logits);
  check(scan_sigmoid_focal_loss_backward(logits.data_ptr<float>(), targets.data_ptr<int32_t>(), d_losses.data_ptr<float>(),
                                         1.0f, logits.size(0), num_classes, gamma, alpha, d_logits.data_ptr<float>(),
                                         current_stream(logits)),
        "sigmoid_focalloss_backward");
  return d_logits;
}

// ---- region pooling: csrc/ROIAlign.h:11-45, csrc/ROIPool.h:10-47 over csrc/roi.hip.  NCHW is converted to the kernels' row
// matrix here (channel-last, channels padded to a multiple of 4) and the channel-last result back to contiguous NCHW.
struct Rows {
  at::Tensor rows;  // [N * H * W, Cs]
  scan_pyramid_t d;
  int32_t C, Cs;
};

scan_pyramid_t one_level(int64_t n, int64_t h, int64_t w) {
  scan_pyramid_t d;
  std::memset(&d, 0, sizeof(d));
  d.n_levels = 1;
  d.n_images = (int32_t)n;
  d.h[0] = (int32_t)h;
  d.w[0] = (int32_t)w;
  d.row_off[1] = n * h * w;
  return d;
}

// [N or K, C, a, b] -> channel-last [.., a, b, Cs] with the padding columns = fill
at::Tensor channel_last(const at::Tensor& t, const at::Scalar& fill) {
  at::Tensor r = t.permute({0, 2, 3, 1});
  const int64_t c = t.size(1), cs = (c + 3) / 4 * 4;
  if (cs != c) r = at::constant_pad_nd(r, {0, cs - c}, fill);
  return r.contiguous();
}

Rows rows_of(const at::Tensor& input, const char* who) {
  TORCH_CHECK(input.dim() == 4, who, ": input must be [N, C, H, W]");
  Rows r;
  r.C = (int32_t)input.size(1);
  r.rows = channel_last(input.to(at::kFloat), 0.0);
  r.Cs = (int32_t)r.rows.size(3);
  r.d = one_level(input.size(0), input.size(2), input.size(3));
  return r;
}

at::Tensor rois_of(const at::Tensor& rois, const char* who) {
  TORCH_CHECK(rois.is_cuda(), "rois must be a CUDA tensor");  // ROIAlign_cuda.cu:264
  TORCH_CHECK(rois.dim() == 2 && rois.size(1) == 5, who, ": rois must be [K, 5]");
  return rois.to(at::kFloat).contiguous();
}

at::Tensor to_nchw(const at::Tensor& t, int64_t c) { return t.slice(3, 0, c).permute({0, 3, 1, 2}).contiguous(); }

// csrc/cpu/ROIAlign_cpu.cpp:113-257 semantics on host memory: positions, weights and cells in T, every operation on its own
// in the source's order; the samples of an axis are formed once per ROI and shared by all channels and by the bins of the other
// axis.  An image index outside [0, N) gives zeros (the reference reads out of bounds there).
template <typename T>
struct AxisSample {
  bool live;
  int lo, hi;
  T l, h;
};

template <typename T>
std::vector<AxisSample<T>> axis_samples(T start, T bin, int P, int g, int size) {
  std::vector<AxisSample<T>> out((size_t)P * g);
  for (int p = 0; p < P; ++p)
    for (int i = 0; i < g; ++i) {
      AxisSample<T>& a = out[(size_t)p * g + i];
      T y = start + p * bin + static_cast<T>(i + .5f) * bin / static_cast<T>(g);
      a.live = y >= -1.0 && y <= size;
      a.lo = a.hi = 0;
      a.l = a.h = 0;
      if (!a.live) continue;
      if (y <= 0) y = 0;
      a.lo = (int)y;
      if (a.lo >= size - 1) {
        a.hi = a.lo = size - 1;
        y = (T)a.lo;
      } else {
        a.hi = a.lo + 1;
      }
      a.l = y - a.lo;
      a.h = 1. - a.l;
    }
  return out;
}

template <typename T>
at::Tensor roi_align_host(const at::Tensor& input_in, const at::Tensor& rois_in, float spatial_scale_f, int PH, int PW, int sr) {
  const at::Tensor input = input_in.contiguous(), rois = rois_in.contiguous();
  const int64_t N = input.size(0), C = input.size(1), H = input.size(2), W = input.size(3), K = rois.size(0);
  at::Tensor out = at::zeros({K, C, PH, PW}, input.options());
  const T* x = input.data_ptr<T>();
  const T* rp = rois.data_ptr<T>();
  T* o = out.data_ptr<T>();
  const T scale = spatial_scale_f;
  for (int64_t k = 0; k < K; ++k) {
    const T* r = rp + 5 * k;
    const T nf = std::trunc(r[0]);
    if (!(nf >= 0 && nf < (T)N)) continue;
    const int64_t n = (int64_t)nf;
    const T sw = r[1] * scale, sh = r[2] * scale, ew = r[3] * scale, eh = r[4] * scale;
    const T rw = std::max(ew - sw, (T)1.), rh = std::max(eh - sh, (T)1.);
    const T bh = rh / static_cast<T>(PH), bw = rw / static_cast<T>(PW);
    const int gh = sr > 0 ? sr : (int)std::ceil(rh / PH), gw = sr > 0 ? sr : (int)std::ceil(rw / PW);
    const T count = gh * gw;
    const auto ys = axis_samples<T>(sh, bh, PH, gh, (int)H), xs = axis_samples<T>(sw, bw, PW, gw, (int)W);
    for (int64_t c = 0; c < C; ++c) {
      const T* img = x + (n * C + c) * H * W;
      for (int ph = 0; ph < PH; ++ph)
        for (int pw = 0; pw < PW; ++pw) {
          T acc = 0;
          for (int iy = 0; iy < gh; ++iy) {
            const AxisSample<T>& a = ys[(size_t)ph * gh + iy];
            for (int ix = 0; ix < gw; ++ix) {
              const AxisSample<T>& b = xs[(size_t)pw * gw + ix];
              if (!a.live || !b.live) continue;
              const T w1 = a.h * b.h, w2 = a.h * b.l, w3 = a.l * b.h, w4 = a.l * b.l;
              acc += w1 * img[a.lo * W + b.lo] + w2 * img[a.lo * W + b.hi] + w3 * img[a.hi * W + b.lo] + w4 * img[a.hi * W + b.hi];
            }
          }
          o[((k * C + c) * PH + ph) * PW + pw] = acc / count;
        }
    }
  }
  return out;
}

// a wrong argument count raises RuntimeError naming the arguments, as every other failure of this module does
void take(const py::args& a, const py::kwargs& kw, size_t n, const char* signature) {
  TORCH_CHECK(a.size() == n && kw.size() == 0, signature, ": expected ", n, " positional arguments, got ", a.size(),
              kw.size() ? " and keyword arguments" : "");
}
at::Tensor tensor_arg(const py::args& a, size_t i) { return a[i].cast<at::Tensor>(); }

at::Tensor roi_align_forward(py::args a, py::kwargs kw) {
  take(a, kw, 6, "roi_align_forward(input, rois, spatial_scale, pooled_height, pooled_width, sampling_ratio)");
  const at::Tensor input = tensor_arg(a, 0), rois_in = tensor_arg(a, 1);
  const float scale = a[2].cast<float>();
  const int PH = a[3].cast<int>(), PW = a[4].cast<int>(), sr = a[5].cast<int>();
  if (!input.is_cuda()) {  // csrc/ROIAlign.h:24
    TORCH_CHECK(!rois_in.is_cuda(), "rois must be a CPU tensor");  // ROIAlign_cpu.cpp:228
    TORCH_CHECK(input.dim() == 4 && rois_in.dim() == 2 && rois_in.size(1) == 5 && PH >= 1 && PW >= 1,
                "roi_align_forward: input [N, C, H, W], rois [K, 5], pooled size >= 1 x 1");
    TORCH_CHECK(rois_in.scalar_type() == input.scalar_type(), "roi_align_forward: rois must have the type of input");
    if (input.scalar_type() == at::kDouble) return roi_align_host<double>(input, rois_in, scale, PH, PW, sr);
    TORCH_CHECK(input.scalar_type() == at::kFloat, "roi_align_forward: float or double input (AT_DISPATCH_FLOATING_TYPES)");
    return roi_align_host<float>(input, rois_in, scale, PH, PW, sr);
  }
  c10::hip::HIPGuardMasqueradingAsCUDA guard(input.device());
  const Rows x = rows_of(input, "roi_align_forward");
  const at::Tensor rois = rois_of(rois_in, "roi_align_forward");
  TORCH_CHECK(PH >= 1 && PW >= 1, "roi_align_forward: pooled size must be >= 1 x 1");
  at::Tensor y = at::empty({rois.size(0), PH, PW, x.Cs}, x.rows.options());
  check(scan_roi_align_forward(x.rows.data_ptr<float>(), &x.d, x.C, x.Cs, rois.data_ptr<float>(), nullptr, &scale, rois.size(0), PH,
                               PW, sr, y.data_ptr<float>(), current_stream(input)),
        "roi_align_forward");
  return to_nchw(y, x.C).to(input.scalar_type());
}

at::Tensor roi_align_backward(py::args a, py::kwargs kw) {
  take(a, kw, 10, "roi_align_backward(grad, rois, spatial_scale, pooled_height, pooled_width, batch_size, channels, height, width, "
                  "sampling_ratio)");
  const at::Tensor grad = tensor_arg(a, 0), rois_in = tensor_arg(a, 1);
  const float scale = a[2].cast<float>();
  const int PH = a[3].cast<int>(), PW = a[4].cast<int>(), bs = a[5].cast<int>(), ch = a[6].cast<int>(), h = a[7].cast<int>(),
            w = a[8].cast<int>(), sr = a[9].cast<int>();
  TORCH_CHECK(grad.is_cuda(), "Not implemented on the CPU");  // csrc/ROIAlign.h:44
  TORCH_CHECK(grad.dim() == 4 && grad.size(1) == ch && grad.size(2) == PH && grad.size(3) == PW,
              "roi_align_backward: grad must be [K, channels, pooled_height, pooled_width]");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(grad.device());
  const at::Tensor rois = rois_of(rois_in, "roi_align_backward");
  TORCH_CHECK(rois.size(0) == grad.size(0), "roi_align_backward: one ROI per row of grad");
  const at::Tensor dy = channel_last(grad.to(at::kFloat), 0.0);
  const int32_t Cs = (int32_t)dy.size(3);
  const scan_pyramid_t d = one_level(bs, h, w);
  at::Tensor dx = at::empty({bs, h, w, Cs}, dy.options());
  check(scan_roi_align_backward(dy.data_ptr<float>(), &d, ch, Cs, rois.data_ptr<float>(), nullptr, &scale, rois.size(0), PH, PW, sr,
                                dx.data_ptr<float>(), current_stream(grad)),
        "roi_align_backward");
  return to_nchw(dx, ch).to(grad.scalar_type());
}

std::tuple<at::Tensor, at::Tensor> roi_pool_forward(py::args a, py::kwargs kw) {
  take(a, kw, 5, "roi_pool_forward(input, rois, spatial_scale, pooled_height, pooled_width)");
  const at::Tensor input = tensor_arg(a, 0), rois_in = tensor_arg(a, 1);
  const float scale = a[2].cast<float>();
  const int PH = a[3].cast<int>(), PW = a[4].cast<int>();
  TORCH_CHECK(input.is_cuda(), "Not implemented on the CPU");  // csrc/ROIPool.h:24
  c10::hip::HIPGuardMasqueradingAsCUDA guard(input.device());
  const Rows x = rows_of(input, "roi_pool_forward");
  const at::Tensor rois = rois_of(rois_in, "roi_pool_forward");
  TORCH_CHECK(PH >= 1 && PW >= 1, "roi_pool_forward: pooled size must be >= 1 x 1");
  at::Tensor y = at::empty({rois.size(0), PH, PW, x.Cs}, x.rows.options());
  at::Tensor argmax = at::empty({rois.size(0), PH, PW, x.Cs}, x.rows.options().dtype(at::kInt));
  check(scan_roi_pool_forward(x.rows.data_ptr<float>(), &x.d, x.C, x.Cs, rois.data_ptr<float>(), nullptr, &scale, rois.size(0), PH,
                              PW, y.data_ptr<float>(), argmax.data_ptr<int32_t>(), current_stream(input)),
        "roi_pool_forward");
  return std::make_tuple(to_nchw(y, x.C).to(input.scalar_type()), to_nchw(argmax, x.C));
}

at::Tensor roi_pool_backward(py::args a, py::kwargs kw) {
  take(a, kw, 11, "roi_pool_backward(grad, input, rois, argmax, spatial_scale, pooled_height, pooled_width, batch_size, channels, "
                  "height, width)");
  const at::Tensor grad = tensor_arg(a, 0), rois_in = tensor_arg(a, 2), argmax_in = tensor_arg(a, 3);
  const float scale = a[4].cast<float>();
  const int PH = a[5].cast<int>(), PW = a[6].cast<int>(), bs = a[7].cast<int>(), ch = a[8].cast<int>(), h = a[9].cast<int>(),
            w = a[10].cast<int>();
  TORCH_CHECK(grad.is_cuda(), "Not implemented on the CPU");  // csrc/ROIPool.h:46
  TORCH_CHECK(grad.dim() == 4 && grad.size(1) == ch && grad.size(2) == PH && grad.size(3) == PW,
              "roi_pool_backward: grad must be [K, channels, pooled_height, pooled_width]");
  TORCH_CHECK(argmax_in.is_cuda() && argmax_in.sizes() == grad.sizes(), "roi_pool_backward: argmax must have the shape of grad");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(grad.device());
  const at::Tensor rois = rois_of(rois_in, "roi_pool_backward");
  TORCH_CHECK(rois.size(0) == grad.size(0), "roi_pool_backward: one ROI per row of grad");
  const at::Tensor dy = channel_last(grad.to(at::kFloat), 0.0), am = channel_last(argmax_in.to(at::kInt), -1);
  const int32_t Cs = (int32_t)dy.size(3);
  const scan_pyramid_t d = one_level(bs, h, w);
  at::Tensor dx = at::empty({bs, h, w, Cs}, dy.options());
  check(scan_roi_pool_backward(dy.data_ptr<float>(), am.data_ptr<int32_t>(), &d, ch, Cs, rois.data_ptr<float>(), nullptr, &scale,
                               rois.size(0), PH, PW, dx.data_ptr<float>(), current_stream(grad)),
        "roi_pool_backward");
  return to_nchw(dx, ch).to(grad.scalar_type());
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "fcos_core._C on libscan_hip.so (MI355X / gfx950)";
  m.def("nms", &nms, "non-maximum suppression", py::arg("dets"), py::arg("scores"), py::arg("threshold"),
        py::arg("cuda_rule") = false);
  m.def("ml_nms", &ml_nms, "multi-label non-maximum suppression");
  m.def("sigmoid_focalloss_forward", &sigmoid_focalloss_forward, "SigmoidFocalLoss_forward");
  m.def("sigmoid_focalloss_backward", &sigmoid_focalloss_backward, "SigmoidFocalLoss_backward");
  m.def("roi_align_forward", &roi_align_forward, "ROIAlign_forward");
  m.def("roi_align_backward", &roi_align_backward, "ROIAlign_backward");
  m.def("roi_pool_forward", &roi_pool_forward, "ROIPool_forward");
  m.def("roi_pool_backward", &roi_pool_backward, "ROIPool_backward");
  m.def("scan_abi_version", []() { return scan_abi_version(); }, "ABI version of the libscan_hip.so this module is linked to");
}
