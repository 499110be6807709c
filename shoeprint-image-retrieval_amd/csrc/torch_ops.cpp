// torch.ops.shoeprint_mi355x.* — PyTorch-ROCm custom ops over the C ABI of include/shoeprint_mi355x.h.
//
// SURVEY §8(b) names three device-level operators behind the reference's Python call surface (run.py:20-28):
//   ncc_scores(q [Q,C,h,w], g [G,C,h',w']) -> f32 [Q,G]     compare_maps / _comparison_worker (similarity.py:129-227, :287-375)
//   ranks(scores [Q,G], match i32 [Q])     -> i32 [Q]       _get_rank (similarity.py:378-386)
//   extract(images u8 [N,H,W(,3)], ...)    -> f32 [N,C,h,w] Model.get_feature_maps (network.py:210-244), plain-VGG branches
// and the shortlist behind retrieve() (build-defined: the reference returns ranks of known matches only):
//   topk(scores [Q,G], k)                  -> (f32 [Q,k], i32 [Q,k])   the k best items of every row, in the ranker's order
//   ncc_scores_located(q, g)               -> (f32 [Q,G], i32 [Q,G,2]) ncc_scores and where every pair's NCC map peaks
//   surface_peaks(surfaces [n,h,w], n_peaks, ry, rx) -> (f32 [n,n_peaks], i32 [n,n_peaks], f32 [n])  separated peaks and PSR
// This file is plain host C++ (no device code): every operator checks its tensors, takes PyTorch's CURRENT HIP stream and
// calls the same extern "C" entry points the ctypes binding (_lib.py) calls, so both routes run the same kernels bit for
// bit.  Scratch (prepared spectra, workspaces) comes from PyTorch's caching allocator on that stream; plans are cached per
// shape class for the life of the process and shared by every PyTorch thread and stream - safely, because the library orders
// the calls that touch scratch a plan owns (the header's conventions).  Nothing synchronises.
#include <ATen/ATen.h>
#include <ATen/hip/HIPContext.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime_api.h>
#include <torch/library.h>

#include <algorithm>
#include <map>
#include <mutex>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/shoeprint_mi355x.h"

namespace {

void check(int rc, const char* what) {
  TORCH_CHECK(rc == SPR_OK, "shoeprint_mi355x::", what, ": ", spr_last_error(), " (status ", rc, ")");
}

spr_stream_t current_stream(const at::Tensor& t) {
  return static_cast<spr_stream_t>(c10::hip::getCurrentHIPStream(t.device().index()).stream());
}

// Makes the tensor's GPU the current HIP device for the call (plans allocate, kernels launch on the current device).
struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(const at::Device& d) {
    TORCH_CHECK(hipGetDevice(&prev) == hipSuccess, "hipGetDevice failed");
    if (prev != d.index()) {
      TORCH_CHECK(hipSetDevice(d.index()) == hipSuccess, "hipSetDevice(", int(d.index()), ") failed");
    } else {
      prev = -1;
    }
  }
  ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

void check_device_tensor(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.device().is_cuda(), name, " must live in HBM (a GPU tensor); there is no CPU path");  // torch calls the ROCm device type "cuda"
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

int dtype_code(const at::Tensor& t, const char* name) {
  switch (t.scalar_type()) {
    case at::kFloat: return SPR_F32;
    case at::kHalf: return SPR_F16;
    case at::kBFloat16: return SPR_BF16;
    case at::kUInt16: return SPR_BF16;  // bfloat16 bit patterns (numpy has no bfloat16: the host mirror uploads uint16)
    default: TORCH_CHECK(false, name, ": feature maps are float32, float16 or bfloat16 (or uint16 bfloat16 bit patterns), got ",
                         t.scalar_type());
  }
  return -1;
}

int method_code(const std::string& m) {
  if (m == "auto") return SPR_NCC_AUTO;
  if (m == "fft") return SPR_NCC_FFT;
  if (m == "direct") return SPR_NCC_DIRECT;
  if (m == "fft_pow2") return SPR_NCC_FFT_POW2;
  if (m == "mfma") return SPR_NCC_MFMA;
  if (m == "mfma_f32") return SPR_NCC_MFMA_F32;
  TORCH_CHECK(false, "unknown NCC method '", m, "' (auto | fft | direct | fft_pow2 | mfma | mfma_f32)");
  return -1;
}

std::mutex g_mutex;
using NccKey = std::tuple<int, int, int, int, int, int, int, int, int>;  // device, C, qh, qw, gh, gw, crop, dtype, method
std::map<NccKey, spr_ncc_plan*> g_ncc_plans;
std::map<std::tuple<int, int, int, int>, spr_vgg16_plan*> g_vgg_plans;  // device, arch, block, compute type

spr_ncc_plan* ncc_plan(int device, int c, int qh, int qw, int gh, int gw, int crop, int dtype, int method) {
  std::lock_guard<std::mutex> lock(g_mutex);
  const NccKey key{device, c, qh, qw, gh, gw, crop, dtype, method};
  auto it = g_ncc_plans.find(key);
  if (it != g_ncc_plans.end()) return it->second;
  spr_ncc_shape shape{c, qh, qw, gh, gw, crop, dtype, method};
  spr_ncc_plan* plan = nullptr;
  check(spr_ncc_plan_create(&shape, &plan), "ncc_scores (plan)");
  g_ncc_plans[key] = plan;
  return plan;
}

// scores[q, g] = get_similarity(q, g) as float32, floored at 0 (similarity.py:355-367 without variants).  The prepared
// gallery is built chunk by chunk when it would not fit `max_prepared_bytes` (0: a third of the free HBM, at most 64 GiB).
// With `peaks` (int32 [Q,G], filled by spr_ncc_score_peaks with (y << 16) | x, -1 where the score is 0) the located form.
at::Tensor ncc_scores_impl(const at::Tensor& q, const at::Tensor& g, int64_t crop, const std::string& method,
                           int64_t max_prepared_bytes, at::Tensor* peaks) {
  check_device_tensor(q, "q");
  check_device_tensor(g, "g");
  TORCH_CHECK(q.dim() == 4 && g.dim() == 4, "q and g are [N, C, h, w] batches");
  TORCH_CHECK(q.size(1) == g.size(1), "channel mismatch: queries ", q.size(1), ", gallery ", g.size(1));
  TORCH_CHECK(q.scalar_type() == g.scalar_type() && q.device() == g.device(), "q and g must share storage type and device");
  const DeviceGuard guard(q.device());
  const int64_t nq = q.size(0), ng = g.size(0);
  at::Tensor scores = at::zeros({nq, ng}, q.options().dtype(at::kFloat));
  if (peaks) *peaks = at::full({nq, ng}, -1, q.options().dtype(at::kInt));
  if (nq == 0 || ng == 0) return scores;
  spr_ncc_plan* plan = ncc_plan(q.device().index(), static_cast<int>(q.size(1)), static_cast<int>(q.size(2)), static_cast<int>(q.size(3)),
                                static_cast<int>(g.size(2)), static_cast<int>(g.size(3)), static_cast<int>(crop), dtype_code(q, "q"),
                                method_code(method));
  TORCH_CHECK(!peaks || spr_ncc_plan_has_peaks(plan), "ncc_scores_located: the plan took a matrix-core method (", method,
              "), whose kernels keep the maximum only; ask for method 'fft' or 'direct'");
  const spr_stream_t stream = current_stream(q);
  const auto bytes = q.options().dtype(at::kByte);
  const size_t q_item = spr_ncc_query_bytes(plan, 1), g_item = spr_ncc_gallery_bytes(plan, 1);
  int64_t budget = max_prepared_bytes;
  if (budget <= 0) {
    size_t free_b = 0, total_b = 0;
    TORCH_CHECK(hipMemGetInfo(&free_b, &total_b) == hipSuccess, "hipMemGetInfo failed");
    budget = static_cast<int64_t>(std::min<size_t>(free_b / 3, size_t{64} << 30));
    budget = std::max<int64_t>(budget, int64_t{256} << 20);
  }
  const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>({ng, budget / static_cast<int64_t>(std::max<size_t>(1, g_item)), 65535}));
  at::Tensor pg = at::empty({static_cast<int64_t>(g_item) * chunk}, bytes);
  const size_t g_stride = static_cast<size_t>(g.stride(0)) * g.element_size();
  for (int64_t q0 = 0; q0 < nq; q0 += 65535) {  // (the pair grid takes at most 65 535 queries per call)
    const int64_t qn = std::min<int64_t>(65535, nq - q0);
    at::Tensor pq = at::empty({static_cast<int64_t>(std::max<size_t>(1, q_item)) * qn}, bytes);
    check(spr_ncc_prepare_queries(plan, static_cast<const char*>(q.data_ptr()) + static_cast<size_t>(q0) * q.stride(0) * q.element_size(),
                                  qn, pq.data_ptr(), stream), "ncc_scores (prepare queries)");
    for (int64_t start = 0; start < ng; start += chunk) {
      const int64_t n = std::min(chunk, ng - start);
      if (q0 == 0 || ng > chunk)
        check(spr_ncc_prepare_gallery(plan, static_cast<const char*>(g.data_ptr()) + static_cast<size_t>(start) * g_stride, n,
                                      pg.data_ptr(), stream), "ncc_scores (prepare gallery)");
      if (peaks)
        check(spr_ncc_score_peaks(plan, pq.data_ptr(), qn, pg.data_ptr(), n, scores.data_ptr<float>() + q0 * ng,
                                  peaks->data_ptr<int32_t>() + q0 * ng, nullptr, ng, start, 0, 0, stream),
              "ncc_scores_located (score)");
      else
        check(spr_ncc_score(plan, pq.data_ptr(), qn, pg.data_ptr(), n, scores.data_ptr<float>() + q0 * ng, ng, start, 0, stream),
              "ncc_scores (score)");
    }
  }
  return scores;
}

at::Tensor ncc_scores(const at::Tensor& q, const at::Tensor& g, int64_t crop, std::string method, int64_t max_prepared_bytes) {
  return ncc_scores_impl(q, g, crop, method, max_prepared_bytes, nullptr);
}

// ncc_scores and, out of the same pass (spr_ncc_score_peaks), the pixel (y, x) of the cropped gallery map at which every
// pair's channel-summed NCC map peaks: int32 [Q,G,2], (-1, -1) where the score is 0.  Methods without a peak form (the
// matrix cores) are refused.
std::tuple<at::Tensor, at::Tensor> ncc_scores_located(const at::Tensor& q, const at::Tensor& g, int64_t crop, std::string method,
                                                      int64_t max_prepared_bytes) {
  at::Tensor packed;
  at::Tensor scores = ncc_scores_impl(q, g, crop, method, max_prepared_bytes, &packed);
  at::Tensor yx = at::stack({at::bitwise_right_shift(packed, 16), at::bitwise_and(packed, 0xFFFF)}, -1);
  yx = at::where(packed.unsqueeze(-1) < 0, at::full({}, -1, yx.options()), yx);
  return {scores, yx.contiguous()};
}

// ranks[q] = 1-based place of gallery item match[q] in the descending order of row q (similarity.py:378-386; ties as a
// stable argsort + flip orders them); 0 where match[q] is outside the gallery (the host mirror raises IndexError there).
at::Tensor ranks(const at::Tensor& scores, const at::Tensor& match) {
  check_device_tensor(scores, "scores");
  check_device_tensor(match, "match");
  TORCH_CHECK(scores.dim() == 2 && scores.scalar_type() == at::kFloat, "scores is a float32 [Q, G] matrix");
  TORCH_CHECK(match.dim() == 1 && match.scalar_type() == at::kInt && match.size(0) == scores.size(0), "match is int32 [Q]");
  const DeviceGuard guard(scores.device());
  at::Tensor out = at::zeros({scores.size(0)}, match.options());
  if (scores.size(0) == 0) return out;
  check(spr_rank_true_match(scores.data_ptr<float>(), scores.size(1), scores.size(0), scores.size(1), match.data_ptr<int32_t>(),
                            out.data_ptr<int32_t>(), current_stream(scores)), "ranks");
  return out;
}

// (scores [Q,k], index [Q,k]) of the k best gallery items of every row in the order of `ranks`: the item at position p
// (1-based) is the item ranked p; slots beyond G hold score 0 and index -1.  1 <= k <= 256.
std::tuple<at::Tensor, at::Tensor> topk(const at::Tensor& scores, int64_t k) {
  check_device_tensor(scores, "scores");
  TORCH_CHECK(scores.dim() == 2 && scores.scalar_type() == at::kFloat, "scores is a float32 [Q, G] matrix");
  TORCH_CHECK(k >= 1 && k <= 256, "k = ", k, " outside [1, 256]");
  const DeviceGuard guard(scores.device());
  at::Tensor out_scores = at::empty({scores.size(0), k}, scores.options());
  at::Tensor out_index = at::empty({scores.size(0), k}, scores.options().dtype(at::kInt));
  if (scores.size(0) == 0) return {out_scores, out_index};
  check(spr_topk_rows(scores.data_ptr<float>(), scores.size(1), scores.size(0), scores.size(1), nullptr, 0, static_cast<int32_t>(k),
                      out_scores.data_ptr<float>(), out_index.data_ptr<int32_t>(), current_stream(scores)), "topk");
  return {out_scores, out_index};
}

// the peaks[n_peaks] best separated peaks of every surface [n, h, w] and the peak-to-sidelobe ratio of the first
// (spr_surface_peaks): values f32 [n, n_peaks], packed positions i32 [n, n_peaks] ((y << 16) | x, -1 = none), psr f32 [n]
std::tuple<at::Tensor, at::Tensor, at::Tensor> surface_peaks(const at::Tensor& surfaces, int64_t n_peaks, int64_t ry, int64_t rx) {
  check_device_tensor(surfaces, "surfaces");
  TORCH_CHECK(surfaces.dim() == 3 && surfaces.scalar_type() == at::kFloat, "surfaces is a float32 [n, h, w] batch");
  TORCH_CHECK(n_peaks >= 1 && n_peaks <= 8, "n_peaks = ", n_peaks, " outside [1, 8]");
  TORCH_CHECK(ry >= 0 && rx >= 0 && ry <= 0x7fffffff && rx <= 0x7fffffff, "the window (", ry, ", ", rx, ") is negative or beyond int32");
  const DeviceGuard guard(surfaces.device());
  const int64_t n = surfaces.size(0);
  at::Tensor values = at::empty({n, n_peaks}, surfaces.options());
  at::Tensor yx = at::empty({n, n_peaks}, surfaces.options().dtype(at::kInt));
  at::Tensor psr = at::empty({n}, surfaces.options());
  if (n == 0) return {values, yx, psr};
  check(spr_surface_peaks(surfaces.data_ptr<float>(), n, static_cast<int32_t>(surfaces.size(1)), static_cast<int32_t>(surfaces.size(2)),
                          static_cast<int32_t>(n_peaks), static_cast<int32_t>(ry), static_cast<int32_t>(rx), values.data_ptr<float>(),
                          yx.data_ptr<int32_t>(), psr.data_ptr<float>(), current_stream(surfaces)), "surface_peaks");
  return {values, yx, psr};
}

// the plan cache of `extract` and `extract_taps` (plain VGGs)
spr_vgg16_plan* vgg_plan(int device, int64_t arch, int64_t block, int64_t compute) {
  std::lock_guard<std::mutex> lock(g_mutex);
  const auto key = std::make_tuple(device, static_cast<int>(arch), static_cast<int>(block), static_cast<int>(compute));
  auto it = g_vgg_plans.find(key);
  if (it != g_vgg_plans.end()) return it->second;
  spr_vgg16_plan* plan = nullptr;
  check(spr_vgg_plan_create_ex(static_cast<int32_t>(arch), static_cast<int32_t>(block), static_cast<int32_t>(compute), &plan),
        "extract (plan)");
  g_vgg_plans[key] = plan;
  return plan;
}

// features[:block] of a plain VGG (arch 0 VGG16, 1 VGG19, 2 VGG19_BN; network.py:121-139, :185-186) on a uint8 batch
// [N,H,W] (grey, repeated over three planes: network.py:67) or [N,H,W,3]; `packed` = the weights as spr_vgg16_pack_weights
// wrote them; mean / std as the reference's transforms take them (network.py:60-71); compute = spr_dtype of the plan
// (spr_vgg_plan_create_ex: 0 the exact f32 matrix cores, 1 / 2 float16 / bfloat16 operands, 3 SPR_COMPUTE_BF16X3: hi + lo
// bfloat16 operands, three products per float32 product).  float32 [N,C,h,w] out.
at::Tensor extract(const at::Tensor& images, const at::Tensor& packed, int64_t arch, int64_t block, std::vector<double> mean,
                   std::vector<double> std_, int64_t compute) {
  check_device_tensor(images, "images");
  check_device_tensor(packed, "packed");
  TORCH_CHECK(images.scalar_type() == at::kByte && (images.dim() == 3 || (images.dim() == 4 && images.size(3) == 3)),
              "images are uint8 [N, H, W] or [N, H, W, 3]");
  TORCH_CHECK(mean.size() == 3 && std_.size() == 3, "mean and std hold three values");
  const DeviceGuard guard(images.device());
  spr_vgg16_plan* plan = vgg_plan(images.device().index(), arch, block, compute);
  TORCH_CHECK(static_cast<size_t>(packed.numel()) * packed.element_size() >= spr_vgg16_packed_bytes(plan),
              "packed weights: ", packed.numel() * packed.element_size(), " bytes, the plan needs ", spr_vgg16_packed_bytes(plan));
  const int64_t n = images.size(0);
  const int32_t h = static_cast<int32_t>(images.size(1)), w = static_cast<int32_t>(images.size(2));
  int32_t c = 0, oh = 0, ow = 0;
  check(spr_vgg16_output_shape(plan, h, w, &c, &oh, &ow), "extract (shape)");
  at::Tensor out = at::empty({n, c, oh, ow}, images.options().dtype(at::kFloat));
  if (n == 0) return out;
  at::Tensor ws = at::empty({static_cast<int64_t>(std::max<size_t>(16, spr_vgg16_workspace_bytes(plan, n, h, w)))},
                            images.options().dtype(at::kByte));
  const float mean3[3] = {static_cast<float>(mean[0]), static_cast<float>(mean[1]), static_cast<float>(mean[2])};
  const float inv3[3] = {1.0f / static_cast<float>(std_[0]), 1.0f / static_cast<float>(std_[1]), 1.0f / static_cast<float>(std_[2])};
  check(spr_vgg16_forward(plan, images.data_ptr<uint8_t>(), n, h, w, images.dim() == 4 ? 3 : 1, mean3, inv3, packed.data_ptr(),
                          ws.data_ptr(), out.data_ptr<float>(), current_stream(images)), "extract");
  return out;
}

// ---- extract_taps: one extractor pass that also hands out the activations at `taps` (slice ends like `block`, strictly below
// it, each once; Model.extract_taps_device) -> the taps in the order asked, then `out`.  arch names the backbone:
//   0 .. 2    plain VGG (spr_vgg_arch, as `extract`; the plan cache of `extract`): spr_vgg16_forward_taps
//   16 + a    EfficientNet arch a of spr_effnet_plan_create (16 = EfficientNetV2_S, 17 = _M ...): spr_effnet_forward_taps
//   32        ResNet50: spr_resnet_forward_taps          48   DenseNet_201: spr_densenet_forward_taps
// `packed`: the plan's packed parameters as the host mirror builds them (Model.packed).
constexpr int64_t kArchEffnet = 16, kArchResnet = 32, kArchDensenet = 48;
std::map<std::tuple<int, int, int, int>, void*> g_backbone_plans;  // device, arch code, block, compute type

struct TapCall {
  const at::Tensor& images;
  const at::Tensor& packed;
  float mean3[3], inv3[3];
  int64_t n;
  int32_t h, w, ch;
};

at::Tensor f32_like(const at::Tensor& images, int64_t n, int32_t c, int32_t h, int32_t w) {
  return at::empty({n, c, h, w}, images.options().dtype(at::kFloat));
}

// ResNet50 / EfficientNet / DenseNet_201: their entry points share one calling sequence
template <class Plan, class Shape, class TapShape, class Ws, class Fwd>
std::vector<at::Tensor> backbone_taps(Plan* plan, size_t packed_bytes, Shape output_shape, TapShape tap_shape, Ws workspace_bytes,
                                      Fwd forward_taps, const TapCall& a, const std::vector<int64_t>& taps) {
  TORCH_CHECK(static_cast<size_t>(a.packed.numel()) * a.packed.element_size() >= packed_bytes, "packed weights: ",
              a.packed.numel() * a.packed.element_size(), " bytes, the plan needs ", packed_bytes);
  int32_t c = 0, oh = 0, ow = 0;
  check(output_shape(plan, a.h, a.w, &c, &oh, &ow), "extract_taps (shape)");
  std::vector<at::Tensor> result;
  std::vector<int32_t> ends;
  std::vector<float*> ptrs;
  for (int64_t t : taps) {
    int32_t tc = 0, th = 0, tw = 0;
    check(tap_shape(plan, static_cast<int32_t>(t), a.h, a.w, &tc, &th, &tw), "extract_taps (tap)");  // refuses a bad tap
    result.push_back(f32_like(a.images, a.n, tc, th, tw));
    ends.push_back(static_cast<int32_t>(t));
    ptrs.push_back(a.n ? result.back().template data_ptr<float>() : nullptr);
  }
  at::Tensor out = f32_like(a.images, a.n, c, oh, ow);
  if (a.n != 0) {
    at::Tensor ws = at::empty({static_cast<int64_t>(std::max<size_t>(16, workspace_bytes(plan, a.n, a.h, a.w)))},
                              a.images.options().dtype(at::kByte));
    check(forward_taps(plan, a.images.template data_ptr<uint8_t>(), a.n, a.h, a.w, a.ch, a.mean3, a.inv3, a.packed.data_ptr(),
                       ws.data_ptr(), out.template data_ptr<float>(), static_cast<int32_t>(ends.size()), ends.data(), ptrs.data(),
                       current_stream(a.images)), "extract_taps");
  }
  result.push_back(out);
  return result;
}

// plain VGG: spr_vgg16_forward_taps names convolutions; the convolution whose ReLU ends features[:t], and its output size
// (the image halved once per max pool in front of it), from spr_vgg_conv_info as Model.extract_taps_device finds them
std::vector<at::Tensor> vgg_taps(spr_vgg16_plan* plan, int64_t block, const TapCall& a, const std::vector<int64_t>& taps) {
  TORCH_CHECK(static_cast<size_t>(a.packed.numel()) * a.packed.element_size() >= spr_vgg16_packed_bytes(plan),
              "packed weights: ", a.packed.numel() * a.packed.element_size(), " bytes, the plan needs ", spr_vgg16_packed_bytes(plan));
  const int convs = spr_vgg16_num_convs(plan);
  std::vector<int32_t> at_feature(convs), bn(convs);
  for (int i = 0; i < convs; ++i) check(spr_vgg_conv_info(plan, i, &at_feature[i], &bn[i]), "extract_taps (plan)");
  std::vector<at::Tensor> result;
  std::vector<int32_t> ordinals;
  std::vector<float*> ptrs;
  for (int64_t t : taps) {
    TORCH_CHECK(t < block, "extract_taps: tap ", t, " is not below the block (", block, "): the output comes last anyway");
    int conv = -1;
    for (int i = 1; i < convs; ++i)
      if (at_feature[i] + (bn[i] ? 2 : 1) == t - 1) conv = i;
    TORCH_CHECK(conv > 0, "extract_taps: tap ", t, " is not the ReLU behind one of the convolutions 1.. of this plan");
    TORCH_CHECK(std::find(ordinals.begin(), ordinals.end(), conv) == ordinals.end(), "extract_taps: tap ", t, " named twice");
    int pools = 0;  // a max pool follows convolution j where the next convolution starts two behind its ReLU
    for (int j = 0; j < conv; ++j) pools += at_feature[j + 1] == at_feature[j] + (bn[j] ? 3 : 2) + 1;
    int32_t cin = 0, cout = 0;
    check(spr_vgg16_conv_shape(plan, conv, &cin, &cout), "extract_taps (plan)");
    result.push_back(f32_like(a.images, a.n, cout, a.h >> pools, a.w >> pools));
    ordinals.push_back(conv);
    ptrs.push_back(a.n ? result.back().data_ptr<float>() : nullptr);
  }
  int32_t c = 0, oh = 0, ow = 0;
  check(spr_vgg16_output_shape(plan, a.h, a.w, &c, &oh, &ow), "extract_taps (shape)");
  at::Tensor out = f32_like(a.images, a.n, c, oh, ow);
  if (a.n != 0) {
    at::Tensor ws = at::empty({static_cast<int64_t>(std::max<size_t>(16, spr_vgg16_workspace_bytes(plan, a.n, a.h, a.w)))},
                              a.images.options().dtype(at::kByte));
    check(spr_vgg16_forward_taps(plan, a.images.data_ptr<uint8_t>(), a.n, a.h, a.w, a.ch, a.mean3, a.inv3, a.packed.data_ptr(),
                                 ws.data_ptr(), out.data_ptr<float>(), static_cast<int32_t>(ordinals.size()), ordinals.data(),
                                 ptrs.data(), current_stream(a.images)), "extract_taps");
  }
  result.push_back(out);
  return result;
}

std::vector<at::Tensor> extract_taps(const at::Tensor& images, const at::Tensor& packed, int64_t arch, int64_t block,
                                     std::vector<double> mean, std::vector<double> std_, int64_t compute, std::vector<int64_t> taps) {
  check_device_tensor(images, "images");
  check_device_tensor(packed, "packed");
  TORCH_CHECK(images.scalar_type() == at::kByte && (images.dim() == 3 || (images.dim() == 4 && images.size(3) == 3)),
              "images are uint8 [N, H, W] or [N, H, W, 3]");
  TORCH_CHECK(mean.size() == 3 && std_.size() == 3, "mean and std hold three values");
  const DeviceGuard guard(images.device());
  const int device = images.device().index();
  TapCall a{images, packed, {static_cast<float>(mean[0]), static_cast<float>(mean[1]), static_cast<float>(mean[2])},
            {1.0f / static_cast<float>(std_[0]), 1.0f / static_cast<float>(std_[1]), 1.0f / static_cast<float>(std_[2])},
            images.size(0), static_cast<int32_t>(images.size(1)), static_cast<int32_t>(images.size(2)), images.dim() == 4 ? 3 : 1};
  if (arch >= 0 && arch <= 2) return vgg_taps(vgg_plan(device, arch, block, compute), block, a, taps);
  const bool effnet = arch >= kArchEffnet && arch <= kArchEffnet + 8;
  TORCH_CHECK(effnet || arch == kArchResnet || arch == kArchDensenet, "extract_taps: arch ", arch,
              " (0 .. 2 plain VGG, 16 + EfficientNet arch, 32 ResNet50, 48 DenseNet_201)");
  void* plan = nullptr;
  {
    std::lock_guard<std::mutex> lock(g_mutex);
    const auto key = std::make_tuple(device, static_cast<int>(arch), static_cast<int>(block), static_cast<int>(compute));
    auto it = g_backbone_plans.find(key);
    if (it != g_backbone_plans.end()) {
      plan = it->second;
    } else {
      const int32_t b = static_cast<int32_t>(block), ct = static_cast<int32_t>(compute);
      if (effnet) {
        spr_effnet_plan* p = nullptr;
        check(spr_effnet_plan_create_ex(static_cast<int32_t>(arch - kArchEffnet), b, ct, &p), "extract_taps (plan)");
        plan = p;
      } else if (arch == kArchResnet) {
        spr_resnet_plan* p = nullptr;
        check(spr_resnet_plan_create_ex(b, ct, &p), "extract_taps (plan)");
        plan = p;
      } else {
        spr_densenet_plan* p = nullptr;
        check(spr_densenet_plan_create_ex(b, ct, &p), "extract_taps (plan)");
        plan = p;
      }
      g_backbone_plans[key] = plan;
    }
  }
  if (effnet) {
    auto* p = static_cast<spr_effnet_plan*>(plan);
    return backbone_taps(p, spr_effnet_packed_bytes(p), spr_effnet_output_shape, spr_effnet_tap_shape, spr_effnet_workspace_bytes,
                         spr_effnet_forward_taps, a, taps);
  }
  if (arch == kArchResnet) {
    auto* p = static_cast<spr_resnet_plan*>(plan);
    return backbone_taps(p, spr_resnet_packed_bytes(p), spr_resnet_output_shape, spr_resnet_tap_shape, spr_resnet_workspace_bytes,
                         spr_resnet_forward_taps, a, taps);
  }
  auto* p = static_cast<spr_densenet_plan*>(plan);
  return backbone_taps(p, spr_densenet_packed_bytes(p), spr_densenet_output_shape, spr_densenet_tap_shape,
                       spr_densenet_workspace_bytes, spr_densenet_forward_taps, a, taps);
}

}  // namespace

TORCH_LIBRARY(shoeprint_mi355x, m) {
  m.def("extract_taps(Tensor images, Tensor packed, int arch, int block, float[] mean, float[] std, int compute, int[] taps) -> Tensor[]");
  m.def("ncc_scores(Tensor q, Tensor g, int crop=2, str method='auto', int max_prepared_bytes=0) -> Tensor");
  m.def("ranks(Tensor scores, Tensor match) -> Tensor");
  m.def("extract(Tensor images, Tensor packed, int arch, int block, float[] mean, float[] std, int compute=0) -> Tensor");
  m.def("topk(Tensor scores, int k) -> (Tensor, Tensor)");
  m.def("ncc_scores_located(Tensor q, Tensor g, int crop=2, str method='auto', int max_prepared_bytes=0) -> (Tensor, Tensor)");
  m.def("surface_peaks(Tensor surfaces, int n_peaks, int ry, int rx) -> (Tensor, Tensor, Tensor)");
}

// Backend-independent registration: the operators check for GPU tensors themselves (there is no CPU kernel to dispatch to).
TORCH_LIBRARY_IMPL(shoeprint_mi355x, CompositeExplicitAutograd, m) {
  m.impl("ncc_scores", &ncc_scores);
  m.impl("ranks", &ranks);
  m.impl("extract", &extract);
  m.impl("extract_taps", &extract_taps);
  m.impl("topk", &topk);
  m.impl("ncc_scores_located", &ncc_scores_located);
  m.impl("surface_peaks", &surface_peaks);
}
