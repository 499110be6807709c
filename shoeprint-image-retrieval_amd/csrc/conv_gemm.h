// Internal declarations of the extractor side: the host launchers of the convolution kernels that the backbones share
// (each kernel lives in one translation unit; other files reach it through its launcher) and the trace records of the
// plans (ResNet, EfficientNet, DenseNet, plain VGG; float32 and 16-bit).  All launchers enqueue on the stream and return
// SPR_OK / SPR_ERR_HIP, or SPR_ERR_UNSUPPORTED for a kernel size / stride / tile combination that is not instantiated.
#pragma once
#include <algorithm>
#include <vector>

#include "spr_common.h"

namespace spr {

// grid of a grid-stride kernel over `total` items
inline dim3 blocks_of(size_t total) {
  return dim3(static_cast<unsigned>(std::min<size_t>((total + kThreads - 1) / kThreads, 65535 * 16)));
}

// One convolution (pad = ks / 2), as every convolution launcher below takes it.  A plain convolution names its geometry,
// in / wts / bias / out and its activation; everything else is optional.  Tensor pointers are untyped: float32 for
// launch_conv_gemm, the plan's 16-bit type for the others (wts: as the matching pack_* function wrote them); the launcher
// that owns the kernel casts them.  A launcher given a field that its kernel has no path for returns SPR_ERR_UNSUPPORTED.
struct ConvCall {
  int ks = 1, stride = 1;
  int64_t n = 0;                    // images
  int h = 0, w = 0;                 // input pixels
  int cin = 0, cout = 0;            // channels the GEMM reads / computes (multiples of the kernel's tile)
  int cout_real = 0;                // cout is padded: channels of the float32 NCHW result (launch_conv_gemm: of the NHWC
                                    // result too); 0: all of them
  int lda = 0, ldc = 0;             // channel strides of the NHWC input / output tensors; 0: cin / cout
  int c_off = 0;                    // first channel of the NHWC output tensor that is written
  const void* in = nullptr;         // NHWC [n][h][w][lda]
  const void* wts = nullptr;
  const float* bias = nullptr;
  const void* res = nullptr;        // residual operand, NHWC like the output with cout channels
  const float* in_scale = nullptr;  // [image][cin] factors on the input (squeeze-excitation)
  const float* pre_s = nullptr;     // per input channel: max(x * pre_s + pre_t, 0) on the operand (BatchNorm + ReLU in
  const float* pre_t = nullptr;     // front of the convolution)
  int act = 0;                      // 0 none, 1 ReLU (behind the residual sum), 2 SiLU (in front of it)
  void* out = nullptr;              // NHWC result ...
  float* out_nchw = nullptr;        // ... or, if not null, the float32 NCHW result [n][cout_real][ho][wo] (last layer)
  float* tap_nchw = nullptr;        // a feature tap: beside the NHWC store into `out`, the same values - unrounded in a 16-bit
                                    // plan - as float32 NCHW [n][tap_real][ho][wo], as out_nchw would hold them (not with it)
  int tap_real = 0;                 // channels of tap_nchw; 0: cout_real, or cout where that is 0 too
  int tap_channels() const { return tap_real ? tap_real : cout_real ? cout_real : cout; }
  int in_stride() const { return lda ? lda : cin; }
  int out_stride() const { return ldc ? ldc : cout; }
};

// ---- conv_gemm.hip.  ks / stride / kind (SPR_F16 | SPR_BF16) pick the template instance; act: 0 none, 1 ReLU, 2 SiLU.
// parameter packing of one convolution into `packed` at w_off / b_off (floats): the f32 GEMM layout (stem != 0: the f32
// stem's), the 16-bit GEMM layout, the 16-bit stem's (ks = 7: ResNet, ks = 3: EfficientNet / plain VGG first layer)
int pack_conv_gemm(const float* w, const float* b, float* packed, size_t w_off, size_t b_off, int cin, int cout, int ks,
                   int stem, hipStream_t s);
int pack_conv_gemm16(int kind, const float* w, const float* b, float* packed, size_t w_off, size_t b_off, int cin, int cout,
                     int ks, hipStream_t s);
int pack_stem16(int kind, int ks, const float* w, const float* b, float* packed, size_t w_off, size_t b_off, hipStream_t s);
// 7x7 / stride 2 stem on plain FMA, pre-processing fused; in_h x in_w: the image; kind16 != 0: 16-bit NHWC store
int launch_stem(const uint8_t* images, int64_t n, int in_h, int in_w, int in_channels, const float* mean3,
                const float* inv_std3, const float* wts, const float* bias, float* out, int relu, int kind16, hipStream_t s);
// first convolution on the 16-bit matrix cores, pre-processing fused: (ks, stride) = (7, 2) ResNet, (3, 2) EfficientNet,
// (3, 1) plain VGG
int launch_stem16(int kind, int ks, int stride, const uint8_t* images, int64_t n, int in_h, int in_w, int in_channels,
                  const float* mean3, const float* inv_std3, const uint16_t* w16, const float* bias, int act, uint16_t* out,
                  hipStream_t s);
// 3x3 / stride 2 / pad 1 max pool of an NHWC tensor [n][h][w][c] (ldo: channel stride of the output; 16-bit: a multiple of 8)
int launch_maxpool3(const float* in, int64_t n, int h, int w, int c, float* out, int ldo, hipStream_t s);
int launch_maxpool3_16(const uint16_t* in, int64_t n, int h, int w, int c, uint16_t* out, int ldo, hipStream_t s);
// implicit-GEMM convolution on the f32 matrix cores: (ks, stride) in (1, 1), (1, 2), (3, 1), (3, 2); see conv_gemm_kernel.
// This launcher and launch_conv_gemm16 honour tap_nchw (both stores out of one launch); the others refuse it
int launch_conv_gemm(const ConvCall& c, hipStream_t s);
// ... on the 16-bit matrix cores: the same four (ks, stride); see conv_gemm16_kernel (no lda / ldc / c_off / pre_s; cout_real
// counts for the NCHW result only).  bn_switch: this call honours SPR_GEMM16_BN=128 (128-channel tiles where cout allows;
// not built for 3x3 / stride 1)
int launch_conv_gemm16(int kind, const ConvCall& c, bool bn_switch, hipStream_t s);

// ---- vgg_conv.hip: its 16-bit 3x3 / stride 1 convolution, shared with the ResNet plans (bias and ReLU only)
int pack_conv16_3x3(int kind, const float* w, const float* b, float* packed, size_t w_off, size_t b_off, int cin, int cout,
                    hipStream_t s);
int launch_conv16_3x3(int kind, const ConvCall& c, hipStream_t s);

// The argument checks every spr_*_forward starts with (`name`: the entry point, for the message).  SPR_OK with n == 0
// means there is nothing to do.
int check_forward_args(const char* name, const void* plan, const void* images, int64_t n, int in_h, int in_w, int in_channels,
                       const float* mean3, const float* inv_std3, const void* packed, const void* workspace, const float* out);

// ---- feature taps (spr_*_forward_taps): slice ends into the backbone's children, like the plan's block, and where the
// float32 NCHW activation at each goes.  check_taps refuses (SPR_ERR_ARG, naming `accepted`) a null array, a tap that is not
// in `accepted` (ascending; the backbone puts only ends below the plan's block there) and a tap named twice; a null
// tap_out[t] is refused unless n == 0.
struct TapSet {
  std::vector<int> feature;
  std::vector<float*> out;
  float* find(int f) const {
    for (size_t t = 0; t < feature.size(); ++t)
      if (feature[t] == f) return out[t];
    return nullptr;
  }
};
int check_taps(const char* name, const std::vector<int>& accepted, int block, int32_t n_taps, const int32_t* tap_features,
               float* const* tap_out, int64_t n, TapSet* set);
// one tap end against `accepted` (spr_*_tap_shape)
int check_tap(const char* name, const std::vector<int>& accepted, int block, int tap);

// ---- trace records (spr_*_forward_trace): what a layer stored, copied device to device behind it on the same stream.
// Records lie 256-byte aligned in plan order; NHWC [n][h][w][c] in the plan's compute type (16-bit or float32; c padded as
// stored), float32 [n][c] (squeeze-excitation factors: h = w = 1) or the float32 NCHW output [n][c][h][w] of the last layer
// (c real).
struct TraceRec { size_t off, bytes; int h, w, c, dtype, nchw; };
struct TraceLayout {
  std::vector<TraceRec> recs;
  size_t total = 0;
  int64_t n = 0;
  void add(int h, int w, int c, int dtype, int nchw) {
    // (SPR_COMPUTE_BF16X3 records hold a hi and a lo bfloat16 word per channel: 4 bytes, as float32)
    const size_t bytes = static_cast<size_t>(n) * h * w * c * (dtype == SPR_F16 || dtype == SPR_BF16 ? 2 : 4);
    recs.push_back(TraceRec{total, bytes, h, w, c, dtype, nchw});
    total += align_up(bytes, 256);
  }
};
// copy record i from src (a null trace: the plain forward, nothing to do)
int trace_copy(unsigned char* trace, const TraceLayout* lay, size_t i, const void* src, hipStream_t s);
int trace_query(const TraceLayout& lay, int64_t* records, size_t* total_bytes);

}  // namespace spr
