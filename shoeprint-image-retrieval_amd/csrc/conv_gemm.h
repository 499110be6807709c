// Internal declarations of the extractor side: the host launchers of the convolution kernels that the backbones share
// (each kernel lives in one translation unit; other files reach it through its launcher) and the trace records of the
// 16-bit ResNet / EfficientNet plans.  All launchers enqueue on the stream and return SPR_OK / SPR_ERR_HIP, or
// SPR_ERR_UNSUPPORTED for a kernel size / stride / tile combination that is not instantiated.
#pragma once
#include <vector>

#include "spr_common.h"

namespace spr {

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
// implicit-GEMM convolution on the f32 matrix cores: (ks, stride) in (1, 1), (1, 2), (3, 1), (3, 2); see conv_gemm_kernel
int launch_conv_gemm(int ks, int stride, const float* in, int64_t n, int h, int w, int cin, int cout, const float* wts,
                     const float* bias, const float* res, int act, int nchw, float* out, const float* in_scale, int cout_real,
                     int lda, int ldc, int c_off, const float* pre_s, const float* pre_t, hipStream_t s);
// ... on the 16-bit matrix cores: the same four (ks, stride); see conv_gemm16_kernel.  bn_switch: this call honours
// SPR_GEMM16_BN=128 (128-channel tiles where cout allows; not built for 3x3 / stride 1)
int launch_conv_gemm16(int kind, int ks, int stride, const uint16_t* in, int64_t n, int h, int w, int cin, int cout,
                       const uint16_t* w16, const float* bias, const uint16_t* res, int act, uint16_t* out, float* out32,
                       const float* in_scale, int cout_real, bool bn_switch, hipStream_t s);

// ---- vgg_conv.hip: its 16-bit 3x3 / stride 1 convolution, shared with the ResNet plans (NHWC 16-bit in / out)
int pack_conv16_3x3(int kind, const float* w, const float* b, float* packed, size_t w_off, size_t b_off, int cin, int cout,
                    hipStream_t s);
int launch_conv16_3x3(int kind, const uint16_t* in, int64_t n, int h, int w, int cin, int cout, const uint16_t* w16,
                      const float* bias, int relu, uint16_t* out, hipStream_t s);

// The argument checks every spr_*_forward starts with (`name`: the entry point, for the message).  SPR_OK with n == 0
// means there is nothing to do.
int check_forward_args(const char* name, const void* plan, const void* images, int64_t n, int in_h, int in_w, int in_channels,
                       const float* mean3, const float* inv_std3, const void* packed, const void* workspace, const float* out);

// ---- trace records (spr_*_forward_trace): what a layer stored, copied device to device behind it on the same stream.
// Records lie 256-byte aligned in plan order; 16-bit NHWC [n][h][w][c] (c padded as stored), float32 [n][c] (squeeze-
// excitation factors: h = w = 1) or the float32 NCHW output [n][c][h][w] of the last layer (c real).
struct TraceRec { size_t off, bytes; int h, w, c, dtype, nchw; };
struct TraceLayout {
  std::vector<TraceRec> recs;
  size_t total = 0;
  int64_t n = 0;
  void add(int h, int w, int c, int dtype, int nchw) {
    const size_t bytes = static_cast<size_t>(n) * h * w * c * (dtype == SPR_F32 ? 4 : 2);
    recs.push_back(TraceRec{total, bytes, h, w, c, dtype, nchw});
    total += align_up(bytes, 256);
  }
};
// copy record i from src (a null trace: the plain forward, nothing to do)
int trace_copy(unsigned char* trace, const TraceLayout* lay, size_t i, const void* src, hipStream_t s);
int trace_query(const TraceLayout& lay, int64_t* records, size_t* total_bytes);

}  // namespace spr
