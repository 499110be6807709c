// ResNet50 through layer1 / layer2 / layer3 (BASELINE.json config 3: "ResNet50 layer3 summed maps") on the shared
// convolution kernels of conv_gemm.hip: the plan, every spr_resnet_* entry point and the walk over the bottlenecks (one for
// both compute types).
//
// The reference has no ResNet (network.py:121-182 lists VGG, EfficientNet and DenseNet) and its truncation
// `list(model.features.children())[:block]` (network.py:185) would not apply to torchvision's resnet50, which has no
// `.features`; this extractor is therefore BUILD-DEFINED: torchvision's resnet50 v1.5 graph (stride on the 3x3 convolution
// of a bottleneck), truncated after `block` of its top-level children [conv1, bn1, relu, maxpool, layer1, layer2, layer3],
// block = 5 / 6 / 7.  Eval-mode BatchNorm is an affine map per channel and is folded into the preceding convolution by
// the host, so the kernels see convolution + bias only.
//
// Layers: stem_kernel (stem16_kernel in a 16-bit plan) + max pool, then every convolution on conv_gemm_kernel /
// conv_gemm16_kernel (bias, residual add, ReLU in the epilogue), except the 3x3 / stride 1 ones of a 16-bit plan, which
// run on vgg_conv.hip's patch kernel.  Activations NHWC between layers, NCHW float32 out of the last one.
// Arithmetic: 17.13 GFLOP per 512x256 image through layer3; bound: fp32 MFMA 157 TFLOP/s.
#include <new>
#include <utility>
#include <vector>

#include "conv_gemm.h"

namespace spr {
namespace {

struct RConv {
  int cin, cout, ks, stride;
  int relu;      // ReLU in the epilogue
  int res;       // 0: none, 1: add the block input, 2: add the downsample branch's output
  int role;      // 0 stem, 1 conv1, 2 conv2, 3 conv3, 4 downsample
  size_t w_off, b_off;
};

}  // namespace
}  // namespace spr

struct spr_resnet_plan {
  int block;                       // top-level children kept: 5 = layer1, 6 = layer2, 7 = layer3
  int compute;                     // SPR_F32 (exact) | SPR_F16 | SPR_BF16 (16-bit operands, f32 accumulation)
  std::vector<spr::RConv> convs;   // in torchvision's module order (conv1; per bottleneck conv1, conv2, conv3, [downsample])
  size_t packed_floats;
};

using namespace spr;

extern "C" int spr_resnet_plan_create(int32_t block, spr_resnet_plan** plan_out) {
  return spr_resnet_plan_create_ex(block, SPR_F32, plan_out);
}

extern "C" int spr_resnet_plan_compute(const spr_resnet_plan* plan) { return plan ? plan->compute : SPR_ERR_ARG; }

extern "C" int spr_resnet_plan_create_ex(int32_t block, int32_t compute, spr_resnet_plan** plan_out) {
  if (!plan_out) { set_error("spr_resnet_plan_create: null pointer"); return SPR_ERR_ARG; }
  *plan_out = nullptr;
  if (compute == SPR_COMPUTE_BF16X3) {
    set_error("spr_resnet_plan_create_ex: SPR_COMPUTE_BF16X3 (bfloat16x3, the hi + lo split) is built for the plain-VGG plans only");
    return SPR_ERR_UNSUPPORTED;
  }
  if (compute != SPR_F32 && compute != SPR_F16 && compute != SPR_BF16) {
    set_error("spr_resnet_plan_create_ex: compute type %d (SPR_F32 | SPR_F16 | SPR_BF16)", compute);
    return SPR_ERR_ARG;
  }
  if (block < 5 || block > 7) {
    set_error("spr_resnet_plan_create: block %d: the truncation must end after layer1 (5), layer2 (6) or layer3 (7)", block);
    return SPR_ERR_ARG;
  }
  spr_resnet_plan* plan = new (std::nothrow) spr_resnet_plan();
  if (!plan) { set_error("out of host memory"); return SPR_ERR_ARG; }
  plan->block = block;
  plan->compute = compute;
  size_t off = 0;
  auto add = [&](int cin, int cout, int ks, int stride, int relu, int res, int role) {
    RConv c{};
    c.cin = cin; c.cout = cout; c.ks = ks; c.stride = stride; c.relu = relu; c.res = res; c.role = role;
    // (16-bit plans: two weights per float slot; the stem's 160 x 64 padded 16-bit matrix fits its f32 allocation)
    c.w_off = off; off += static_cast<size_t>(cout) * cin * ks * ks / ((compute != SPR_F32 && role != 0) ? 2 : 1);
    c.b_off = off; off += static_cast<size_t>(cout);
    off = (off + 3) / 4 * 4;
    plan->convs.push_back(c);
  };
  add(3, 64, 7, 2, 1, 0, 0);
  static const int blocks_per_layer[3] = {3, 4, 6};
  int cin = 64;
  for (int layer = 0; layer < block - 4; ++layer) {
    const int mid = 64 << layer;
    for (int b = 0; b < blocks_per_layer[layer]; ++b) {
      const int stride = (b == 0 && layer > 0) ? 2 : 1;
      add(cin, mid, 1, 1, 1, 0, 1);
      add(mid, mid, 3, stride, 1, 0, 2);
      add(mid, 4 * mid, 1, 1, 1, b == 0 ? 2 : 1, 3);
      if (b == 0) add(cin, 4 * mid, 1, stride, 0, 0, 4);
      cin = 4 * mid;
    }
  }
  plan->packed_floats = off;
  *plan_out = plan;
  return SPR_OK;
}

extern "C" void spr_resnet_plan_destroy(spr_resnet_plan* plan) { delete plan; }

extern "C" int spr_resnet_num_convs(const spr_resnet_plan* plan) {
  return plan ? static_cast<int>(plan->convs.size()) : SPR_ERR_ARG;
}

extern "C" int spr_resnet_conv_shape(const spr_resnet_plan* plan, int32_t i, int32_t* cin, int32_t* cout, int32_t* ksize,
                                     int32_t* stride, int32_t* role) {
  if (!plan || !cin || !cout || !ksize || !stride || !role || i < 0 || i >= static_cast<int>(plan->convs.size())) {
    set_error("spr_resnet_conv_shape: bad argument");
    return SPR_ERR_ARG;
  }
  const RConv& c = plan->convs[i];
  *cin = c.cin; *cout = c.cout; *ksize = c.ks; *stride = c.stride; *role = c.role;
  return SPR_OK;
}

static void resnet_dims(const spr_resnet_plan* plan, int in_h, int in_w, int* c, int* h, int* w) {
  int hh = (in_h + 1) / 2, ww = (in_w + 1) / 2;  // conv1: 7x7 s2 p3
  hh = (hh + 1) / 2; ww = (ww + 1) / 2;          // maxpool 3x3 s2 p1
  for (int layer = 1; layer < plan->block - 4; ++layer) { hh = (hh + 1) / 2; ww = (ww + 1) / 2; }  // 3x3 s2 p1
  *c = 256 << (plan->block - 5); *h = hh; *w = ww;
}

extern "C" int spr_resnet_output_shape(const spr_resnet_plan* plan, int32_t in_h, int32_t in_w, int32_t* channels,
                                       int32_t* out_h, int32_t* out_w) {
  if (!plan || !channels || !out_h || !out_w || in_h < 1 || in_w < 1) {
    set_error("spr_resnet_output_shape: bad argument");
    return SPR_ERR_ARG;
  }
  resnet_dims(plan, in_h, in_w, channels, out_h, out_w);
  return SPR_OK;
}

extern "C" size_t spr_resnet_packed_bytes(const spr_resnet_plan* plan) {
  return plan ? plan->packed_floats * sizeof(float) : 0;
}

extern "C" int spr_resnet_pack_weights(spr_resnet_plan* plan, const float* const* weights, const float* const* biases,
                                       void* packed, spr_stream_t stream) {
  if (!plan || !weights || !biases || !packed) { set_error("spr_resnet_pack_weights: null pointer"); return SPR_ERR_ARG; }
  for (size_t i = 0; i < plan->convs.size(); ++i) {
    const RConv& c = plan->convs[i];
    if (!weights[i] || !biases[i]) { set_error("spr_resnet_pack_weights: null parameter %zu", i); return SPR_ERR_ARG; }
    hipStream_t hs = static_cast<hipStream_t>(stream);
    float* pk = static_cast<float*>(packed);
    int rc;
    if (i == 0 && plan->compute != SPR_F32)
      rc = pack_stem16(plan->compute, 7, weights[i], biases[i], pk, c.w_off, c.b_off, hs);
    else if (plan->compute != SPR_F32 && c.ks == 3 && c.stride == 1)
      // the 3x3 / stride 1 layers of a 16-bit plan run on vgg_conv.hip's patch kernel: its weight layout
      rc = pack_conv16_3x3(plan->compute, weights[i], biases[i], pk, c.w_off, c.b_off, c.cin, c.cout, hs);
    else if (plan->compute != SPR_F32)
      rc = pack_conv_gemm16(plan->compute, weights[i], biases[i], pk, c.w_off, c.b_off, c.cin, c.cout, c.ks, hs);
    else
      rc = pack_conv_gemm(weights[i], biases[i], pk, c.w_off, c.b_off, c.cin, c.cout, c.ks, i == 0 ? 1 : 0, hs);
    if (rc != SPR_OK) return rc;
  }
  return SPR_OK;
}

// four activation buffers (block input, two bottleneck intermediates / the downsample branch, block output), each as
// large as the largest tensor between layers
static size_t resnet_big16_bytes(int64_t n, int in_h, int in_w) {  // layer1's output, the largest 16-bit tensor
  const int hp = ((in_h + 1) / 2 + 1) / 2, wp = ((in_w + 1) / 2 + 1) / 2;
  return align_up(static_cast<size_t>(n) * hp * wp * 256 * sizeof(uint16_t), 256);
}
// one of the four activation buffers of an f32 plan: the stem's output or layer1's, whichever is larger (the max pool rounds
// odd sizes up, so 256 channels on the pooled map can outgrow 64 channels on the stem's: 17 x 24 -> 9 x 12)
static size_t resnet_buf32_bytes(int64_t n, int in_h, int in_w) {
  const int hs = (in_h + 1) / 2, ws = (in_w + 1) / 2;
  const size_t stem = static_cast<size_t>(n) * hs * ws * 64, layer1 = static_cast<size_t>(n) * ((hs + 1) / 2) * ((ws + 1) / 2) * 256;
  return align_up(std::max(stem, layer1) * sizeof(float), 256);
}
extern "C" size_t spr_resnet_workspace_bytes(const spr_resnet_plan* plan, int64_t n, int32_t in_h, int32_t in_w) {
  if (!plan || n < 0) return 0;
  const size_t stem = static_cast<size_t>(n) * ((in_h + 1) / 2) * ((in_w + 1) / 2) * 64;
  // 16-bit plans: the stem's f32 tensor, then four 16-bit activation buffers
  if (plan->compute != SPR_F32) return align_up(stem * sizeof(float), 256) + 4 * resnet_big16_bytes(n, in_h, in_w);
  return 4 * resnet_buf32_bytes(n, in_h, in_w);
}

// one convolution of the plan: conv_gemm_kernel for an f32 plan; in a 16-bit plan vgg_conv.hip's patch kernel for the 3x3 /
// stride 1 layers and conv_gemm16_kernel for the others (the only call sites that honour SPR_GEMM16_BN).  out_nchw: null, or
// where the last layer's float32 NCHW result goes
static int resnet_conv(const spr_resnet_plan* plan, const RConv& c, const void* in, int64_t n, int h, int w, const float* pk,
                       const void* res, void* out, float* out_nchw, hipStream_t s, float* tap = nullptr) {
  ConvCall k;
  k.ks = c.ks; k.stride = c.stride; k.n = n; k.h = h; k.w = w; k.cin = c.cin; k.cout = c.cout;
  k.in = in; k.wts = pk + c.w_off; k.bias = pk + c.b_off; k.res = res; k.act = c.relu; k.out = out; k.out_nchw = out_nchw;
  k.tap_nchw = tap;  // (a layer's last conv3: a 1x1 convolution, never on the patch kernel)
  if (plan->compute == SPR_F32) return launch_conv_gemm(k, s);
  if (c.ks == 3 && c.stride == 1) return launch_conv16_3x3(plan->compute, k, s);
  return launch_conv_gemm16(plan->compute, k, true, s);
}

// stem (before pooling), max pool, then one record per convolution in conv index order (c1, c2, c3, [downsample])
static TraceLayout resnet_trace_layout(const spr_resnet_plan* plan, int64_t n, int in_h, int in_w) {
  TraceLayout lay;
  lay.n = n;
  int h = (in_h + 1) / 2, w = (in_w + 1) / 2;
  lay.add(h, w, 64, plan->compute, 0);
  h = (h + 1) / 2; w = (w + 1) / 2;
  lay.add(h, w, 64, plan->compute, 0);
  size_t i = 1;
  while (i < plan->convs.size()) {
    const bool down = plan->convs[i + 2].res == 2;
    const bool last = i + (down ? 4 : 3) == plan->convs.size();
    const int ho = plan->convs[i + 1].stride == 2 ? (h + 1) / 2 : h, wo = plan->convs[i + 1].stride == 2 ? (w + 1) / 2 : w;
    lay.add(h, w, plan->convs[i].cout, plan->compute, 0);
    lay.add(ho, wo, plan->convs[i + 1].cout, plan->compute, 0);
    if (last) lay.add(ho, wo, plan->convs[i + 2].cout, SPR_F32, 1);
    else lay.add(ho, wo, plan->convs[i + 2].cout, plan->compute, 0);
    if (down) lay.add(ho, wo, plan->convs[i + 3].cout, plan->compute, 0);
    h = ho; w = wo;
    i += down ? 4 : 3;
  }
  return lay;
}

extern "C" int spr_resnet_trace_layout(const spr_resnet_plan* plan, int64_t n, int32_t in_h, int32_t in_w, int64_t* records,
                                       size_t* total_bytes) {
  if (!plan || n < 0 || in_h < 32 || in_w < 32) { set_error("spr_resnet_trace_layout: bad argument"); return SPR_ERR_ARG; }
  return trace_query(resnet_trace_layout(plan, n, in_h, in_w), records, total_bytes);
}

// trace: null (the plain forward), or where the stem's, the max pool's and every convolution's stored
// result is copied (resnet_trace_layout: record 1 + conv index)
static int resnet_forward(spr_resnet_plan* plan, const uint8_t* images, int64_t n, int32_t in_h, int32_t in_w,
                          int32_t in_channels, const float* mean3, const float* inv_std3, const void* packed, void* workspace,
                          float* out, spr_stream_t stream, unsigned char* trace, const TapSet* taps = nullptr) {
  const int ok = check_forward_args(taps ? "spr_resnet_forward_taps" : "spr_resnet_forward", plan, images, n, in_h, in_w, in_channels, mean3, inv_std3, packed,
                                    workspace, out);
  if (ok != SPR_OK || n == 0) return ok;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const float* pk = static_cast<const float*>(packed);
  const bool f32 = plan->compute == SPR_F32;
  // f32: four buffers, the stem's output in the second.  16-bit: [stem's tensor][x][t1][t2][y]
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  const size_t stem_bytes = align_up(static_cast<size_t>(n) * ((in_h + 1) / 2) * ((in_w + 1) / 2) * 64 * sizeof(float), 256);
  const size_t first = f32 ? 0 : stem_bytes, step = f32 ? resnet_buf32_bytes(n, in_h, in_w) : resnet_big16_bytes(n, in_h, in_w);
  void* x = ws + first;             // block input (first: the pooled stem output)
  void* t1 = ws + first + step;     // conv1's output, then the downsample branch's
  void* t2 = ws + first + 2 * step;
  void* y = ws + first + 3 * step;  // block output
  void* stem_out = f32 ? t1 : static_cast<void*>(ws);
  TraceLayout lay;
  if (trace) lay = resnet_trace_layout(plan, n, in_h, in_w);
  int h = (in_h + 1) / 2, w = (in_w + 1) / 2;
  {  // stem + max pool
    const RConv& c = plan->convs[0];
    int rc = f32 ? launch_stem(images, n, in_h, in_w, in_channels, mean3, inv_std3, pk + c.w_off, pk + c.b_off,
                               static_cast<float*>(stem_out), 1, 0, s)
                 : launch_stem16(plan->compute, 7, 2, images, n, in_h, in_w, in_channels, mean3, inv_std3,
                                 reinterpret_cast<const uint16_t*>(pk + c.w_off), pk + c.b_off, 1,
                                 static_cast<uint16_t*>(stem_out), s);
    if (rc == SPR_OK) rc = trace_copy(trace, &lay, 0, stem_out, s);
    if (rc != SPR_OK) return rc;
    // (16-bit plans: the stem stored its activation rounded to the 16-bit type; the pooled tensor is layer1's operand)
    rc = f32 ? launch_maxpool3(static_cast<const float*>(stem_out), n, h, w, 64, static_cast<float*>(x), 64, s)
             : launch_maxpool3_16(static_cast<const uint16_t*>(stem_out), n, h, w, 64, static_cast<uint16_t*>(x), 64, s);
    if (rc == SPR_OK) rc = trace_copy(trace, &lay, 1, x, s);
    if (rc != SPR_OK) return rc;
    h = (h + 1) / 2; w = (w + 1) / 2;
  }
  size_t i = 1;
  int layer = 0;  // layers begun
  while (i < plan->convs.size()) {  // one bottleneck
    const RConv& c1 = plan->convs[i];
    const RConv& c2 = plan->convs[i + 1];
    const RConv& c3 = plan->convs[i + 2];
    const bool down = c3.res == 2;
    const bool last = i + (down ? 4 : 3) == plan->convs.size();
    const int ho = c2.stride == 2 ? (h + 1) / 2 : h, wo = c2.stride == 2 ? (w + 1) / 2 : w;
    int rc = resnet_conv(plan, c1, x, n, h, w, pk, nullptr, t1, nullptr, s);
    if (rc == SPR_OK) rc = trace_copy(trace, &lay, 1 + i, t1, s);
    if (rc != SPR_OK) return rc;
    rc = resnet_conv(plan, c2, t1, n, h, w, pk, nullptr, t2, nullptr, s);
    if (rc == SPR_OK) rc = trace_copy(trace, &lay, 2 + i, t2, s);
    if (rc != SPR_OK) return rc;
    const void* resid = x;
    if (down) {
      rc = resnet_conv(plan, plan->convs[i + 3], x, n, h, w, pk, nullptr, t1, nullptr, s);
      if (rc == SPR_OK) rc = trace_copy(trace, &lay, 4 + i, t1, s);
      if (rc != SPR_OK) return rc;
      resid = t1;
    }
    // the last bottleneck of a layer (the next one opens with a downsample branch) ends child 4 + layer of the list
    if (down) ++layer;
    const size_t next = i + (down ? 4 : 3);
    float* tap = nullptr;
    if (taps && !last && plan->convs[next + 2].res == 2) tap = taps->find(4 + layer);
    rc = resnet_conv(plan, c3, t2, n, ho, wo, pk, resid, y, last ? out : nullptr, s, tap);
    if (rc == SPR_OK) rc = trace_copy(trace, &lay, 3 + i, last ? static_cast<void*>(out) : y, s);
    if (rc != SPR_OK) return rc;
    h = ho; w = wo;
    std::swap(x, y);
    i += down ? 4 : 3;
  }
  return SPR_OK;
}

extern "C" int spr_resnet_forward(spr_resnet_plan* plan, const uint8_t* images, int64_t n, int32_t in_h, int32_t in_w,
                                  int32_t in_channels, const float* mean3, const float* inv_std3, const void* packed,
                                  void* workspace, float* out, spr_stream_t stream) {
  return resnet_forward(plan, images, n, in_h, in_w, in_channels, mean3, inv_std3, packed, workspace, out, stream, nullptr);
}

// the accepted taps of a plan: the layer ends below its block
static std::vector<int> resnet_taps(const spr_resnet_plan* plan) {
  std::vector<int> ends;
  for (int t = 5; t < plan->block; ++t) ends.push_back(t);
  return ends;
}

extern "C" int spr_resnet_tap_shape(const spr_resnet_plan* plan, int32_t tap_feature, int32_t in_h, int32_t in_w,
                                    int32_t* channels, int32_t* out_h, int32_t* out_w) {
  if (!plan || !channels || !out_h || !out_w || in_h < 1 || in_w < 1) { set_error("spr_resnet_tap_shape: bad argument"); return SPR_ERR_ARG; }
  const int rc = check_tap("spr_resnet_tap_shape", resnet_taps(plan), plan->block, tap_feature);
  if (rc != SPR_OK) return rc;
  spr_resnet_plan cut{};  // (resnet_dims reads the block alone)
  cut.block = tap_feature;
  resnet_dims(&cut, in_h, in_w, channels, out_h, out_w);
  return SPR_OK;
}

extern "C" int spr_resnet_forward_taps(spr_resnet_plan* plan, const uint8_t* images, int64_t n, int32_t in_h, int32_t in_w,
                                       int32_t in_channels, const float* mean3, const float* inv_std3, const void* packed,
                                       void* workspace, float* out, int32_t n_taps, const int32_t* tap_features,
                                       float* const* tap_out, spr_stream_t stream) {
  if (!plan) { set_error("spr_resnet_forward_taps: null plan"); return SPR_ERR_ARG; }
  TapSet taps;
  const int rc = check_taps("spr_resnet_forward_taps", resnet_taps(plan), plan->block, n_taps, tap_features, tap_out, n, &taps);
  if (rc != SPR_OK) return rc;
  return resnet_forward(plan, images, n, in_h, in_w, in_channels, mean3, inv_std3, packed, workspace, out, stream, nullptr, &taps);
}

extern "C" int spr_resnet_forward_trace(spr_resnet_plan* plan, const uint8_t* images, int64_t n, int32_t in_h, int32_t in_w,
                                        int32_t in_channels, const float* mean3, const float* inv_std3, const void* packed,
                                        void* workspace, float* out, void* trace, spr_stream_t stream) {
  if (!plan || !trace) { set_error("spr_resnet_forward_trace: null pointer"); return SPR_ERR_ARG; }
  return resnet_forward(plan, images, n, in_h, in_w, in_channels, mean3, inv_std3, packed, workspace, out, stream,
                        static_cast<unsigned char*>(trace));
}
