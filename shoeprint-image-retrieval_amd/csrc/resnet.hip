// ResNet50 through layer1 / layer2 / layer3 (BASELINE.json config 3: "ResNet50 layer3 summed maps") on the shared
// convolution kernels of conv_gemm.hip: the plan, every spr_resnet_* entry point and the walks over the bottlenecks.
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
// large as the largest tensor between layers: the stem's output
static size_t resnet_big16_bytes(int64_t n, int in_h, int in_w) {  // layer1's output, the largest 16-bit tensor
  const int hp = ((in_h + 1) / 2 + 1) / 2, wp = ((in_w + 1) / 2 + 1) / 2;
  return align_up(static_cast<size_t>(n) * hp * wp * 256 * sizeof(uint16_t), 256);
}
extern "C" size_t spr_resnet_workspace_bytes(const spr_resnet_plan* plan, int64_t n, int32_t in_h, int32_t in_w) {
  if (!plan || n < 0) return 0;
  const size_t stem = static_cast<size_t>(n) * ((in_h + 1) / 2) * ((in_w + 1) / 2) * 64;
  // 16-bit plans: the stem's f32 tensor, then four 16-bit activation buffers
  if (plan->compute != SPR_F32) return align_up(stem * sizeof(float), 256) + 4 * resnet_big16_bytes(n, in_h, in_w);
  return 4 * align_up(stem * sizeof(float), 256);
}

// one convolution of the plan on conv_gemm16_kernel (the only call sites that honour SPR_GEMM16_BN)
static int resnet_gemm16(int kind, const RConv& c, const uint16_t* in, int64_t n, int h, int w, const float* pk,
                         const uint16_t* res, uint16_t* out, float* out32, hipStream_t s) {
  return launch_conv_gemm16(kind, c.ks, c.stride, in, n, h, w, c.cin, c.cout, reinterpret_cast<const uint16_t*>(pk + c.w_off),
                            pk + c.b_off, res, c.relu, out, out32, nullptr, 0, true, s);
}

// ... and of an f32 plan on conv_gemm_kernel
static int resnet_gemm(const RConv& c, const float* in, int64_t n, int h, int w, const float* pk, const float* res, int nchw,
                       float* out, hipStream_t s) {
  return launch_conv_gemm(c.ks, c.stride, in, n, h, w, c.cin, c.cout, pk + c.w_off, pk + c.b_off, res, c.relu, nchw, out,
                          nullptr, 0, c.cin, c.cout, 0, nullptr, nullptr, s);
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
  if (plan->compute == SPR_F32) { set_error("spr_resnet_trace_layout: 16-bit plans only"); return SPR_ERR_UNSUPPORTED; }
  return trace_query(resnet_trace_layout(plan, n, in_h, in_w), records, total_bytes);
}

// the bottlenecks of a 16-bit plan: x (the pooled stem output, 16-bit NHWC) lives in buf[0]; t1 / t2 / y in buf[1..3].
// trace / lay: null, or where every convolution's stored result is copied (record 1 + conv index)
static int resnet_blocks16(const spr_resnet_plan* plan, int64_t n, int h, int w, const float* pk, uint16_t* const buf[4],
                           float* out, hipStream_t s, unsigned char* trace, const TraceLayout* lay) {
  uint16_t* x = buf[0];
  uint16_t* t1 = buf[1];
  uint16_t* t2 = buf[2];
  uint16_t* y = buf[3];
  const int kind = plan->compute;
  size_t i = 1;
  while (i < plan->convs.size()) {
    const RConv& c1 = plan->convs[i];
    const RConv& c2 = plan->convs[i + 1];
    const RConv& c3 = plan->convs[i + 2];
    const bool down = c3.res == 2;
    const bool last = i + (down ? 4 : 3) == plan->convs.size();
    const int ho = c2.stride == 2 ? (h + 1) / 2 : h, wo = c2.stride == 2 ? (w + 1) / 2 : w;
    int rc = resnet_gemm16(kind, c1, x, n, h, w, pk, nullptr, t1, nullptr, s);
    if (rc == SPR_OK) rc = trace_copy(trace, lay, 1 + i, t1, s);
    if (rc != SPR_OK) return rc;
    rc = c2.stride == 2 ? resnet_gemm16(kind, c2, t1, n, h, w, pk, nullptr, t2, nullptr, s)
                        : launch_conv16_3x3(kind, t1, n, h, w, c2.cin, c2.cout, reinterpret_cast<const uint16_t*>(pk + c2.w_off),
                                            pk + c2.b_off, c2.relu, t2, s);
    if (rc == SPR_OK) rc = trace_copy(trace, lay, 2 + i, t2, s);
    if (rc != SPR_OK) return rc;
    const uint16_t* resid = x;
    if (down) {
      const RConv& cd = plan->convs[i + 3];
      rc = resnet_gemm16(kind, cd, x, n, h, w, pk, nullptr, t1, nullptr, s);
      if (rc == SPR_OK) rc = trace_copy(trace, lay, 4 + i, t1, s);
      if (rc != SPR_OK) return rc;
      resid = t1;
    }
    rc = resnet_gemm16(kind, c3, t2, n, ho, wo, pk, resid, y, last ? out : nullptr, s);
    if (rc == SPR_OK) rc = trace_copy(trace, lay, 3 + i, last ? static_cast<const void*>(out) : y, s);
    if (rc != SPR_OK) return rc;
    h = ho; w = wo;
    uint16_t* old = x;
    x = y;
    y = old;
    i += down ? 4 : 3;
  }
  return SPR_OK;
}

static int resnet_forward(spr_resnet_plan* plan, const uint8_t* images, int64_t n, int32_t in_h, int32_t in_w,
                          int32_t in_channels, const float* mean3, const float* inv_std3, const void* packed, void* workspace,
                          float* out, spr_stream_t stream, unsigned char* trace) {
  const int ok = check_forward_args("spr_resnet_forward", plan, images, n, in_h, in_w, in_channels, mean3, inv_std3, packed,
                                    workspace, out);
  if (ok != SPR_OK || n == 0) return ok;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const float* pk = static_cast<const float*>(packed);
  const bool f32 = plan->compute == SPR_F32;
  const size_t quarter = f32 ? spr_resnet_workspace_bytes(plan, n, in_h, in_w) / 4 : 0;
  float* buf[4];
  for (int i = 0; i < 4; ++i) buf[i] = reinterpret_cast<float*>(static_cast<unsigned char*>(workspace) + i * quarter);
  uint16_t* b16[4] = {nullptr, nullptr, nullptr, nullptr};
  if (!f32) {  // [stem f32 tensor][x][t1][t2][y]
    const size_t stem_bytes = align_up(static_cast<size_t>(n) * ((in_h + 1) / 2) * ((in_w + 1) / 2) * 64 * sizeof(float), 256);
    buf[1] = static_cast<float*>(workspace);
    for (int i = 0; i < 4; ++i)
      b16[i] = reinterpret_cast<uint16_t*>(static_cast<unsigned char*>(workspace) + stem_bytes + i * resnet_big16_bytes(n, in_h, in_w));
  }
  TraceLayout lay;
  if (trace) lay = resnet_trace_layout(plan, n, in_h, in_w);
  // stem + max pool
  int h = (in_h + 1) / 2, w = (in_w + 1) / 2;
  {
    const RConv& c = plan->convs[0];
    int rc = f32 ? launch_stem(images, n, in_h, in_w, in_channels, mean3, inv_std3, pk + c.w_off, pk + c.b_off, buf[1], 1, 0, s)
                 : launch_stem16(plan->compute, 7, 2, images, n, in_h, in_w, in_channels, mean3, inv_std3,
                                 reinterpret_cast<const uint16_t*>(pk + c.w_off), pk + c.b_off, 1,
                                 reinterpret_cast<uint16_t*>(buf[1]), s);
    if (rc == SPR_OK) rc = trace_copy(trace, &lay, 0, buf[1], s);
    if (rc != SPR_OK) return rc;
    const int hp = (h + 1) / 2, wp = (w + 1) / 2;
    // (16-bit plans: the stem stored its activation rounded to the 16-bit type; the pooled tensor is layer1's operand)
    rc = f32 ? launch_maxpool3(buf[1], n, h, w, 64, buf[0], 64, s)
             : launch_maxpool3_16(reinterpret_cast<const uint16_t*>(buf[1]), n, h, w, 64, b16[0], 64, s);
    if (rc == SPR_OK) rc = trace_copy(trace, &lay, 1, b16[0], s);
    if (rc != SPR_OK) return rc;
    h = hp; w = wp;
  }
  if (!f32) return resnet_blocks16(plan, n, h, w, pk, b16, out, s, trace, trace ? &lay : nullptr);
  // bottlenecks: x = buf[0]
  float* x = buf[0];
  float* t1 = buf[1];
  float* t2 = buf[2];
  float* y = buf[3];
  size_t i = 1;
  while (i < plan->convs.size()) {
    const RConv& c1 = plan->convs[i];
    const RConv& c2 = plan->convs[i + 1];
    const RConv& c3 = plan->convs[i + 2];
    const bool down = c3.res == 2;
    const bool last = i + (down ? 4 : 3) == plan->convs.size();
    const int ho = c2.stride == 2 ? (h + 1) / 2 : h, wo = c2.stride == 2 ? (w + 1) / 2 : w;
    int rc = resnet_gemm(c1, x, n, h, w, pk, nullptr, 0, t1, s);
    if (rc != SPR_OK) return rc;
    rc = resnet_gemm(c2, t1, n, h, w, pk, nullptr, 0, t2, s);
    if (rc != SPR_OK) return rc;
    const float* resid = x;
    if (down) {
      const RConv& cd = plan->convs[i + 3];
      rc = resnet_gemm(cd, x, n, h, w, pk, nullptr, 0, t1, s);
      if (rc != SPR_OK) return rc;
      resid = t1;
    }
    float* dst = last ? out : y;
    rc = resnet_gemm(c3, t2, n, ho, wo, pk, resid, last ? 1 : 0, dst, s);
    if (rc != SPR_OK) return rc;
    h = ho; w = wo;
    float* old = x;
    x = y;
    y = old;
    i += down ? 4 : 3;
  }
  return SPR_OK;
}

extern "C" int spr_resnet_forward(spr_resnet_plan* plan, const uint8_t* images, int64_t n, int32_t in_h, int32_t in_w,
                                  int32_t in_channels, const float* mean3, const float* inv_std3, const void* packed,
                                  void* workspace, float* out, spr_stream_t stream) {
  return resnet_forward(plan, images, n, in_h, in_w, in_channels, mean3, inv_std3, packed, workspace, out, stream, nullptr);
}

extern "C" int spr_resnet_forward_trace(spr_resnet_plan* plan, const uint8_t* images, int64_t n, int32_t in_h, int32_t in_w,
                                        int32_t in_channels, const float* mean3, const float* inv_std3, const void* packed,
                                        void* workspace, float* out, void* trace, spr_stream_t stream) {
  if (!plan || !trace) { set_error("spr_resnet_forward_trace: null pointer"); return SPR_ERR_ARG; }
  if (plan->compute == SPR_F32) { set_error("spr_resnet_forward_trace: 16-bit plans only"); return SPR_ERR_UNSUPPORTED; }
  return resnet_forward(plan, images, n, in_h, in_w, in_channels, mean3, inv_std3, packed, workspace, out, stream,
                        static_cast<unsigned char*>(trace));
}
