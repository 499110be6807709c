// EfficientNet B1 .. B7 and EfficientNetV2 truncations (network.py:139-175, :185-186): the plan, the enet_* kernels (depthwise
// convolution, squeeze-excitation) and every spr_effnet_* entry point; the stem and the dense convolutions run on the shared
// kernels of conv_gemm.hip.
// torchvision's efficientnet_v2_{s,m,l}: features = [stem, stage 1 .. stage N, last conv]; the reference keeps
// features[:block].  Stages of FusedMBConv (3x3 expansion convolution, 1x1 projection) and MBConv (1x1 expansion, depthwise
// 3x3, squeeze-excitation, 1x1 projection), SiLU, residual where stride 1 and equal widths; stochastic depth is the identity
// in eval mode.  Flattened here into a list of layers; the host folds BatchNorm (eps 1e-3) and packs the parameters.
#include <algorithm>
#include <cmath>
#include <new>
#include <utility>
#include <vector>

#include "conv_gemm.h"

namespace spr {
namespace {

// ---------------------------------------------------------------- building blocks
// Activations NHWC float32 with the channel count padded to a multiple of 64 (the GEMM tile; padded channels hold zeros:
// zero weights and biases, SiLU(0) = 0); eval-mode BatchNorm folded into the convolutions by the host.

// uint8 grey [n][H][W] (repeated to 3, network.py:60-71) or RGB [n][H][W][3] -> normalised NHWC with 16 channels (3 + zeros)
__global__ void __launch_bounds__(kThreads)
enet_input_kernel(const uint8_t* __restrict__ images, size_t pixels, int in_channels, float m0, float m1, float m2, float s0,
                  float s1, float s2, float* __restrict__ out) {
  for (size_t i = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x; i < pixels;
       i += static_cast<size_t>(gridDim.x) * kThreads) {
    float v[3];
    for (int c = 0; c < 3; ++c) v[c] = static_cast<float>(images[in_channels == 3 ? i * 3 + c : i]) * (1.0f / 255.0f);
    float4* o = reinterpret_cast<float4*>(out + i * 16);
    o[0] = float4{(v[0] - m0) * s0, (v[1] - m1) * s1, (v[2] - m2) * s2, 0.0f};
    o[1] = o[2] = o[3] = float4{0.f, 0.f, 0.f, 0.f};
  }
}

// depthwise ks x ks (3 or 5), stride 1 or 2, pad ks / 2, + bias + SiLU.  One work-item = four channels of one output pixel.
// weights [tap][C] (channels contiguous), C a multiple of 64
__global__ void __launch_bounds__(kThreads)
enet_dw_kernel(const float* __restrict__ in, int n_img, int H, int W, int C, int stride, int ks, const float* __restrict__ wts,
               const float* __restrict__ bias, float* __restrict__ out) {
  const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1, pad = ks / 2;
  const int c4 = C / 4;
  const size_t total = static_cast<size_t>(n_img) * Ho * Wo * c4;
  for (size_t i = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x; i < total;
       i += static_cast<size_t>(gridDim.x) * kThreads) {
    const int c = static_cast<int>(i % c4) * 4;
    size_t p = i / c4;
    const int ox = static_cast<int>(p % Wo); p /= Wo;
    const int oy = static_cast<int>(p % Ho);
    const size_t img = p / Ho;
    float4 acc = *reinterpret_cast<const float4*>(bias + c);
    for (int dy = 0; dy < ks; ++dy)
      for (int dx = 0; dx < ks; ++dx) {
        const int y = oy * stride + dy - pad, x = ox * stride + dx - pad;
        if (y < 0 || y >= H || x < 0 || x >= W) continue;
        const float4 v = *reinterpret_cast<const float4*>(in + ((img * H + y) * static_cast<size_t>(W) + x) * C + c);
        const float4 w = *reinterpret_cast<const float4*>(wts + static_cast<size_t>(dy * ks + dx) * C + c);
        acc.x = fmaf(v.x, w.x, acc.x); acc.y = fmaf(v.y, w.y, acc.y); acc.z = fmaf(v.z, w.z, acc.z); acc.w = fmaf(v.w, w.w, acc.w);
      }
    float4 o;
    o.x = acc.x / (1.0f + expf(-acc.x)); o.y = acc.y / (1.0f + expf(-acc.y));
    o.z = acc.z / (1.0f + expf(-acc.z)); o.w = acc.w / (1.0f + expf(-acc.w));
    *reinterpret_cast<float4*>(out + i * 4) = o;
  }
}

// squeeze-excitation, step 1: mean over the pixels.  grid = (C / 64, images)
__global__ void __launch_bounds__(kThreads)
enet_pool_kernel(const float* __restrict__ in, int HW, int C, float* __restrict__ pooled) {
  __shared__ float part[4][64];
  const int tid = static_cast<int>(threadIdx.x), c = tid & 63, r = tid >> 6;
  const size_t img = blockIdx.y;
  const float* base = in + img * static_cast<size_t>(HW) * C + static_cast<size_t>(blockIdx.x) * 64 + c;
  float s = 0.0f;
  for (int p = r; p < HW; p += 4) s += base[static_cast<size_t>(p) * C];
  part[r][c] = s;
  __syncthreads();
  if (r == 0) pooled[img * C + blockIdx.x * 64 + c] = (part[0][c] + part[1][c] + part[2][c] + part[3][c]) / static_cast<float>(HW);
}

// step 2: scale[img][c] = sigmoid(W2 SiLU(W1 pooled[img] + b1) + b2); w1 [sq][C], w2 [C][sq] (C padded, sq real).  Two small
// kernels with one unit of work per (image, output): a workgroup per image walking its outputs one after another paid a
// trip to memory per output (measured: 76 - 93 us per call at C = 1056, a quarter of a 16-bit forward pass).
// first layer: one WAVE per (image, hidden unit j): a dot product over C, lanes sweep the channels
__global__ void __launch_bounds__(kThreads)
enet_fc1_kernel(const float* __restrict__ pooled, int n_img, int C, int sq, const float* __restrict__ w1,
                const float* __restrict__ b1, float* __restrict__ hid) {
  const int tid = static_cast<int>(threadIdx.x), lane = tid & 63;
  const long long unit = static_cast<long long>(blockIdx.x) * (kThreads / 64) + (tid >> 6);
  if (unit >= static_cast<long long>(n_img) * sq) return;  // (whole waves leave: no barrier below)
  const int img = static_cast<int>(unit / sq), j = static_cast<int>(unit - static_cast<long long>(img) * sq);
  const float* row = w1 + static_cast<size_t>(j) * C;
  const float* pv = pooled + static_cast<size_t>(img) * C;
  float s0 = 0.0f, s1 = 0.0f;
  int c = lane;
  for (; c + 64 < C; c += 128) {
    s0 = fmaf(row[c], pv[c], s0);
    s1 = fmaf(row[c + 64], pv[c + 64], s1);
  }
  if (c < C) s0 = fmaf(row[c], pv[c], s0);
  float s = s0 + s1;
  for (int m = 32; m >= 1; m >>= 1) s += shfl_xor(s, m);
  if (lane == 0) {
    const float v = b1[j] + s;
    hid[static_cast<size_t>(img) * sq + j] = v / (1.0f + expf(-v));
  }
}
// second layer, grid = (blocks of 64 channels, images): four work-items per channel take every fourth hidden unit
__global__ void __launch_bounds__(kThreads)
enet_fc2_kernel(const float* __restrict__ hid, int C, int sq, const float* __restrict__ w2, const float* __restrict__ b2,
                float* __restrict__ scale) {
  __shared__ float part[4][64];
  const int tid = static_cast<int>(threadIdx.x), cl = tid & 63, r = tid >> 6;
  const size_t img = blockIdx.y;
  const int c = static_cast<int>(blockIdx.x) * 64 + cl;
  const float* h = hid + img * sq;
  float s = 0.0f;
  if (c < C) {
    const float* row = w2 + static_cast<size_t>(c) * sq;
    for (int j = r; j < sq; j += 4) s = fmaf(row[j], h[j], s);
  }
  part[r][cl] = s;
  __syncthreads();
  if (r == 0 && c < C) {
    const float t = b2[c] + ((part[0][cl] + part[1][cl]) + (part[2][cl] + part[3][cl]));
    scale[img * C + c] = 1.0f / (1.0f + expf(-t));
  }
}
// both layers; `hid` = n_img * sq floats of scratch
static int launch_enet_fc(const float* pooled, int64_t n, int C, int sq, const float* w1, const float* b1, const float* w2,
                          const float* b2, float* hid, float* scale, hipStream_t s) {
  const long long units = static_cast<long long>(n) * sq;
  hipLaunchKernelGGL(enet_fc1_kernel, dim3(static_cast<unsigned>((units + 3) / 4)), dim3(kThreads), 0, s, pooled,
                     static_cast<int>(n), C, sq, w1, b1, hid);
  int rc = check_launch("enet_fc1_kernel");
  if (rc != SPR_OK) return rc;
  hipLaunchKernelGGL(enet_fc2_kernel, dim3(static_cast<unsigned>(ceil_div(C, 64)), static_cast<unsigned>(n)), dim3(kThreads), 0, s,
                     hid, C, sq, w2, b2, scale);
  return check_launch("enet_fc2_kernel");
}

// ---- 16-bit plans (spr_effnet_plan_create_ex): activations NHWC float16 / bfloat16, the same padding to 64 channels
// depthwise ks x ks + bias + SiLU: eight channels (16 bytes) of one output pixel per work-item; weights / bias f32 as above
template <int KIND>
__global__ void __launch_bounds__(kThreads)
enet_dw16_kernel(const uint16_t* __restrict__ in, int n_img, int H, int W, int C, int stride, int ks,
                 const float* __restrict__ wts, const float* __restrict__ bias, uint16_t* __restrict__ out) {
  const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1, pad = ks / 2;
  const int c8 = C / 8;
  const size_t total = static_cast<size_t>(n_img) * Ho * Wo * c8;
  for (size_t i = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x; i < total;
       i += static_cast<size_t>(gridDim.x) * kThreads) {
    const int c = static_cast<int>(i % c8) * 8;
    size_t p = i / c8;
    const int ox = static_cast<int>(p % Wo); p /= Wo;
    const int oy = static_cast<int>(p % Ho);
    const size_t img = p / Ho;
    float acc[8];
    {
      const float4 b0 = *reinterpret_cast<const float4*>(bias + c), b1 = *reinterpret_cast<const float4*>(bias + c + 4);
      acc[0] = b0.x; acc[1] = b0.y; acc[2] = b0.z; acc[3] = b0.w; acc[4] = b1.x; acc[5] = b1.y; acc[6] = b1.z; acc[7] = b1.w;
    }
    for (int dy = 0; dy < ks; ++dy)
      for (int dx = 0; dx < ks; ++dx) {
        const int y = oy * stride + dy - pad, x = ox * stride + dx - pad;
        if (y < 0 || y >= H || x < 0 || x >= W) continue;
        const u32x4 v = *reinterpret_cast<const u32x4*>(in + ((img * H + y) * static_cast<size_t>(W) + x) * C + c);
        const float* wp = wts + static_cast<size_t>(dy * ks + dx) * C + c;
        const float4 w0 = *reinterpret_cast<const float4*>(wp), w1 = *reinterpret_cast<const float4*>(wp + 4);
        const float wv[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
#pragma unroll
        for (int e = 0; e < 8; ++e)
          acc[e] = fmaf(value16<KIND>(static_cast<uint16_t>(v[e >> 1] >> (16 * (e & 1)))), wv[e], acc[e]);
      }
    u32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float a0 = acc[2 * e] / (1.0f + expf(-acc[2 * e])), a1 = acc[2 * e + 1] / (1.0f + expf(-acc[2 * e + 1]));
      o[e] = static_cast<uint32_t>(round16<KIND>(a0)) | (static_cast<uint32_t>(round16<KIND>(a1)) << 16);
    }
    *reinterpret_cast<u32x4*>(out + i * 8) = o;
  }
}

// squeeze-excitation, step 1 on a 16-bit tensor: f32 mean over the pixels.  grid = (C / 64, images); a work-item reads eight
// channels (16 bytes) of every 32nd pixel
template <int KIND>
__global__ void __launch_bounds__(kThreads)
enet_pool16_kernel(const uint16_t* __restrict__ in, int HW, int C, float* __restrict__ pooled) {
  __shared__ float part[32][65];
  const int tid = static_cast<int>(threadIdx.x), g8 = tid & 7, r = tid >> 3;
  const size_t img = blockIdx.y;
  const uint16_t* base = in + img * static_cast<size_t>(HW) * C + static_cast<size_t>(blockIdx.x) * 64 + g8 * 8;
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int p = r; p < HW; p += 32) {
    const u32x4 v = *reinterpret_cast<const u32x4*>(base + static_cast<size_t>(p) * C);
#pragma unroll
    for (int e = 0; e < 8; ++e) s[e] += value16<KIND>(static_cast<uint16_t>(v[e >> 1] >> (16 * (e & 1))));
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) part[r][g8 * 8 + e] = s[e];
  __syncthreads();
  if (tid < 64) {
    float t = 0.0f;
    for (int k = 0; k < 32; ++k) t += part[k][tid];
    pooled[img * C + blockIdx.x * 64 + tid] = t / static_cast<float>(HW);
  }
}

// ---------------------------------------------------------------- the plan
struct EOp {
  int kind;         // 0 convolution (implicit GEMM), 1 depthwise 3x3, 2 squeeze-excitation
  int cin, cout;    // real channels (squeeze-excitation: cin = cout = expanded width)
  int cin_p, cout_p;
  int ks, stride, act;
  int res;          // convolution: add the block input behind it
  int scaled;       // convolution: its input is multiplied by the squeeze-excitation factors
  int sq;           // squeeze-excitation: hidden width
  int block_end;    // last layer of a residual block (or of the stem)
  int feature;      // index of the top-level child of `features` this layer belongs to
  size_t w_off, b_off, w2_off, b2_off;  // floats into the packed buffer (multiples of 4)
};

struct EStage { int fused, expand, stride, cin, cout, layers, ks; };

const EStage kV2S[] = {{1, 1, 1, 24, 24, 2, 3}, {1, 4, 2, 24, 48, 4, 3}, {1, 4, 2, 48, 64, 4, 3}, {0, 4, 2, 64, 128, 6, 3},
                       {0, 6, 1, 128, 160, 9, 3}, {0, 6, 2, 160, 256, 15, 3}};
const EStage kV2M[] = {{1, 1, 1, 24, 24, 3, 3}, {1, 4, 2, 24, 48, 5, 3}, {1, 4, 2, 48, 80, 5, 3}, {0, 4, 2, 80, 160, 7, 3},
                       {0, 6, 1, 160, 176, 14, 3}, {0, 6, 2, 176, 304, 18, 3}, {0, 6, 1, 304, 512, 5, 3}};
const EStage kV2L[] = {{1, 1, 1, 32, 32, 4, 3}, {1, 4, 2, 32, 64, 7, 3}, {1, 4, 2, 64, 96, 7, 3}, {0, 4, 2, 96, 192, 10, 3},
                       {0, 6, 1, 192, 224, 19, 3}, {0, 6, 2, 224, 384, 25, 3}, {0, 6, 1, 384, 640, 7, 3}};
// EfficientNet_B0's stages (all MBConv); B1 .. B7 scale the widths and depths (network.py:139-162)
const EStage kB0[] = {{0, 1, 1, 32, 16, 1, 3}, {0, 6, 2, 16, 24, 2, 3}, {0, 6, 2, 24, 40, 2, 5}, {0, 6, 2, 40, 80, 3, 3},
                      {0, 6, 1, 80, 112, 3, 5}, {0, 6, 2, 112, 192, 4, 5}, {0, 6, 1, 192, 320, 1, 3}};
// arch 3 .. 8 = EfficientNet_B1, B2, B3, B4, B5, B7: width and depth multipliers in tenths
const int kBWidth[6] = {10, 11, 12, 14, 16, 20}, kBDepth[6] = {11, 12, 14, 18, 22, 31};

inline int make_divisible8(double v) {  // torchvision's _make_divisible(v, 8)
  int n = static_cast<int>(v + 4.0) / 8 * 8;
  if (n < 8) n = 8;
  if (n < 0.9 * v) n += 8;
  return n;
}

inline int pad64(int c) { return (c + 63) / 64 * 64; }

}  // namespace
}  // namespace spr

using namespace spr;

struct spr_effnet_plan {
  int arch, block;
  int compute;  // SPR_F32 | SPR_F16 | SPR_BF16
  std::vector<EOp> ops;
  size_t packed_floats;
  int max_expand_p;  // widest expanded tensor (squeeze-excitation scratch)
  int max_sq;        // widest squeeze-excitation hidden layer (its scratch)
};

extern "C" int spr_effnet_plan_create(int32_t arch, int32_t block, spr_effnet_plan** plan_out) {
  return spr_effnet_plan_create_ex(arch, block, SPR_F32, plan_out);
}

extern "C" int spr_effnet_plan_compute(const spr_effnet_plan* plan) { return plan ? plan->compute : SPR_ERR_ARG; }

extern "C" int spr_effnet_plan_create_ex(int32_t arch, int32_t block, int32_t compute, spr_effnet_plan** plan_out) {
  if (!plan_out) { set_error("spr_effnet_plan_create: null pointer"); return SPR_ERR_ARG; }
  *plan_out = nullptr;
  if (compute == SPR_COMPUTE_BF16X3) {
    set_error("spr_effnet_plan_create_ex: SPR_COMPUTE_BF16X3 (bfloat16x3, the hi + lo split) is built for the plain-VGG plans only");
    return SPR_ERR_UNSUPPORTED;
  }
  if (compute != SPR_F32 && compute != SPR_F16 && compute != SPR_BF16) {
    set_error("spr_effnet_plan_create_ex: compute type %d (SPR_F32 | SPR_F16 | SPR_BF16)", compute);
    return SPR_ERR_ARG;
  }
  EStage scaled[7];
  const EStage* stages = arch == 0 ? kV2S : arch == 1 ? kV2M : arch == 2 ? kV2L : nullptr;
  const int n_stages = arch == 0 ? 6 : 7;
  if (arch >= 3 && arch <= 8) {
    const double wm = kBWidth[arch - 3] / 10.0, dm = kBDepth[arch - 3] / 10.0;
    for (int i = 0; i < 7; ++i) {
      scaled[i] = kB0[i];
      scaled[i].cin = make_divisible8(kB0[i].cin * wm);
      scaled[i].cout = make_divisible8(kB0[i].cout * wm);
      scaled[i].layers = static_cast<int>(std::ceil(kB0[i].layers * dm - 1e-9));
    }
    stages = scaled;
  }
  if (!stages) {
    set_error("spr_effnet_plan_create: arch %d (0 .. 2 = EfficientNetV2_S / _M / _L, 3 .. 8 = EfficientNet_B1 / B2 / B3 / B4 / B5 / B7)", arch);
    return SPR_ERR_ARG;
  }
  if (block < 1 || block > n_stages + 2) {
    set_error("spr_effnet_plan_create: block %d: features[:block] with block in [1, %d] (= len(model.features))", block,
              n_stages + 2);
    return SPR_ERR_ARG;
  }
  spr_effnet_plan* plan = new (std::nothrow) spr_effnet_plan();
  if (!plan) { set_error("out of host memory"); return SPR_ERR_ARG; }
  plan->arch = arch; plan->block = block; plan->max_expand_p = 64; plan->max_sq = 1; plan->compute = compute;
  size_t off = 0;
  auto take = [&](size_t n) { const size_t o = off; off += (n + 3) / 4 * 4; return o; };
  auto conv = [&](int cin, int cout, int ks, int stride, int act, int res, int scaled, int end, int feature, int cin_p) {
    EOp o{};
    o.kind = 0; o.cin = cin; o.cout = cout; o.cin_p = cin_p; o.cout_p = pad64(cout); o.ks = ks; o.stride = stride; o.act = act;
    o.res = res; o.scaled = scaled; o.block_end = end; o.feature = feature;
    o.w_off = take(static_cast<size_t>(o.cout_p) * o.cin_p * ks * ks);
    o.b_off = take(o.cout_p);
    plan->ops.push_back(o);
  };
  const int stem_out = stages[0].cin;
  conv(3, stem_out, 3, 2, 2, 0, 0, 1, 0, 16);
  for (int st = 0; st < block - 1 && st < n_stages; ++st) {
    const EStage& g = stages[st];
    for (int l = 0; l < g.layers; ++l) {
      const int cin = l == 0 ? g.cin : g.cout, stride = l == 0 ? g.stride : 1;
      const int exp = arch >= 3 ? make_divisible8(static_cast<double>(cin) * g.expand) : cin * g.expand;
      const int res = stride == 1 && cin == g.cout;
      if (g.fused) {
        if (g.expand == 1) {
          conv(cin, g.cout, 3, stride, 2, res, 0, 1, st + 1, pad64(cin));
        } else {
          conv(cin, exp, 3, stride, 2, 0, 0, 0, st + 1, pad64(cin));
          conv(exp, g.cout, 1, 1, 0, res, 0, 1, st + 1, pad64(exp));
        }
      } else {
        if (exp != cin) conv(cin, exp, 1, 1, 2, 0, 0, 0, st + 1, pad64(cin));  // (no expansion convolution at ratio 1)
        EOp d{};
        d.kind = 1; d.cin = d.cout = exp; d.cin_p = d.cout_p = pad64(exp); d.ks = g.ks; d.stride = stride; d.act = 2; d.feature = st + 1;
        d.w_off = take(static_cast<size_t>(g.ks) * g.ks * d.cin_p);
        d.b_off = take(d.cin_p);
        plan->ops.push_back(d);
        EOp e{};
        e.kind = 2; e.cin = e.cout = exp; e.cin_p = e.cout_p = pad64(exp); e.sq = cin / 4 > 1 ? cin / 4 : 1; e.feature = st + 1;
        e.w_off = take(static_cast<size_t>(e.sq) * e.cin_p);
        e.b_off = take(e.sq);
        e.w2_off = take(static_cast<size_t>(e.cin_p) * e.sq);
        e.b2_off = take(e.cin_p);
        plan->ops.push_back(e);
        if (e.cin_p > plan->max_expand_p) plan->max_expand_p = e.cin_p;
        if (e.sq > plan->max_sq) plan->max_sq = e.sq;
        conv(exp, g.cout, 1, 1, 0, res, 1, 1, st + 1, pad64(exp));
      }
    }
  }
  if (block == n_stages + 2) {
    // the closing 1x1 convolution + BatchNorm + SiLU of `features`: 1280 channels in the V2 models, four times the last stage's
    // width in the B-series (torchvision: last_channel or 4 * lastconv_input_channels)
    const int cin = stages[n_stages - 1].cout;
    conv(cin, arch <= 2 ? 1280 : 4 * cin, 1, 1, 2, 0, 0, 1, n_stages + 1, pad64(cin));
  }
  plan->packed_floats = off;
  *plan_out = plan;
  return SPR_OK;
}

extern "C" void spr_effnet_plan_destroy(spr_effnet_plan* plan) { delete plan; }
extern "C" int spr_effnet_num_ops(const spr_effnet_plan* plan) { return plan ? static_cast<int>(plan->ops.size()) : SPR_ERR_ARG; }
extern "C" size_t spr_effnet_packed_bytes(const spr_effnet_plan* plan) { return plan ? plan->packed_floats * sizeof(float) : 0; }

// info[16] = kind, cin, cout, cin_p, cout_p, ks, stride, act, res, sq, feature, then the four packed offsets (in floats,
// each < 2^31) w, b, w2, b2, then block_end (1: last layer of a residual block or of the stem)
extern "C" int spr_effnet_op_info(const spr_effnet_plan* plan, int32_t i, int32_t* info) {
  if (!plan || !info || i < 0 || i >= static_cast<int>(plan->ops.size())) { set_error("spr_effnet_op_info: bad argument"); return SPR_ERR_ARG; }
  const EOp& o = plan->ops[i];
  const int32_t v[16] = {o.kind, o.cin, o.cout, o.cin_p, o.cout_p, o.ks, o.stride, o.act, o.res, o.sq, o.feature,
                         static_cast<int32_t>(o.w_off), static_cast<int32_t>(o.b_off), static_cast<int32_t>(o.w2_off),
                         static_cast<int32_t>(o.b2_off), o.block_end};
  for (int k = 0; k < 16; ++k) info[k] = v[k];
  return SPR_OK;
}

static void effnet_dims(const spr_effnet_plan* plan, int in_h, int in_w, int* c, int* h, int* w) {
  int hh = in_h, ww = in_w, cc = 3;
  for (const EOp& o : plan->ops) {
    if (o.kind == 2) continue;
    if (o.stride == 2) { hh = (hh - 1) / 2 + 1; ww = (ww - 1) / 2 + 1; }
    cc = o.cout;
  }
  *c = cc; *h = hh; *w = ww;
}

extern "C" int spr_effnet_output_shape(const spr_effnet_plan* plan, int32_t in_h, int32_t in_w, int32_t* channels,
                                       int32_t* out_h, int32_t* out_w) {
  if (!plan || !channels || !out_h || !out_w || in_h < 1 || in_w < 1) { set_error("spr_effnet_output_shape: bad argument"); return SPR_ERR_ARG; }
  effnet_dims(plan, in_h, in_w, channels, out_h, out_w);
  return SPR_OK;
}

// four activation buffers as large as the largest tensor between layers + the normalised input + the squeeze-excitation
// vectors (mean and factors)
static size_t effnet_buf_floats(const spr_effnet_plan* plan, int64_t n, int in_h, int in_w) {
  size_t best = static_cast<size_t>(n) * in_h * in_w * 16;
  int hh = in_h, ww = in_w;
  for (const EOp& o : plan->ops) {
    if (o.kind == 2) continue;
    if (o.stride == 2) { hh = (hh - 1) / 2 + 1; ww = (ww - 1) / 2 + 1; }
    const size_t f = static_cast<size_t>(n) * hh * ww * o.cout_p;
    if (f > best) best = f;
  }
  return best;
}
extern "C" size_t spr_effnet_workspace_bytes(const spr_effnet_plan* plan, int64_t n, int32_t in_h, int32_t in_w) {
  if (!plan || n < 0) return 0;
  const size_t buf = align_up(effnet_buf_floats(plan, n, in_h, in_w) * sizeof(float), 256);
  // four activation buffers, the squeeze-excitation means and factors, and the hidden units of its first layer
  return 4 * buf + 2 * align_up(static_cast<size_t>(n) * plan->max_expand_p * sizeof(float), 256) +
         align_up(static_cast<size_t>(n) * plan->max_sq * sizeof(float), 256);
}

// one record per layer in plan order: the stem and every convolution / depthwise convolution as stored (NHWC in the plan's
// compute type, cout_p channels), a squeeze-excitation's float32 factors [n][cin_p], the last layer's float32 NCHW output
static TraceLayout effnet_trace_layout(const spr_effnet_plan* plan, int64_t n, int in_h, int in_w) {
  TraceLayout lay;
  lay.n = n;
  int h = in_h, w = in_w;
  for (size_t i = 0; i < plan->ops.size(); ++i) {
    const EOp& o = plan->ops[i];
    if (o.kind == 2) { lay.add(1, 1, o.cin_p, SPR_F32, 0); continue; }
    if (o.stride == 2) { h = (h - 1) / 2 + 1; w = (w - 1) / 2 + 1; }
    if (i + 1 == plan->ops.size()) lay.add(h, w, o.cout, SPR_F32, 1);
    else lay.add(h, w, o.cout_p, plan->compute, 0);
  }
  return lay;
}

extern "C" int spr_effnet_trace_layout(const spr_effnet_plan* plan, int64_t n, int32_t in_h, int32_t in_w, int64_t* records,
                                       size_t* total_bytes) {
  if (!plan || n < 0 || in_h < 32 || in_w < 32) { set_error("spr_effnet_trace_layout: bad argument"); return SPR_ERR_ARG; }
  return trace_query(effnet_trace_layout(plan, n, in_h, in_w), records, total_bytes);
}

// The forward pass: one walk over the flattened layers, activations in the plan's compute type (padded to 64 channels; the
// four buffers keep their f32 sizes, a 16-bit plan uses half of each).  f32: enet_input_kernel, then every convolution (the
// stem as an ordinary one with 16 input channels) on conv_gemm_kernel.  16-bit: the stem on stem16_kernel's 3x3 / stride 2
// instance, every other convolution on conv_gemm16_kernel.  Both: SiLU in front of the residual sum, squeeze-excitation
// factors on the operand, depthwise convolutions and the squeeze-excitation mean on their kernels per type; float32 NCHW out.
// trace: null (the plain forward), or where every layer's stored result is copied (effnet_trace_layout)
// taps: null, or the stage ends whose block-end convolution also stores its float32 NCHW result (effnet_taps)
static int effnet_forward(const spr_effnet_plan* plan, const uint8_t* images, int64_t n, int in_h, int in_w, int in_channels,
                          const float* mean3, const float* inv_std3, const void* packed, void* workspace, float* out,
                          spr_stream_t stream, unsigned char* trace, const TapSet* taps = nullptr) {
  const int ok = check_forward_args(trace ? "spr_effnet_forward_trace" : taps ? "spr_effnet_forward_taps" : "spr_effnet_forward",
                                    plan, images, n, in_h, in_w, in_channels, mean3, inv_std3, packed, workspace, out);
  if (ok != SPR_OK || n == 0) return ok;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const float* pk = static_cast<const float*>(packed);
  const int kind = plan->compute;
  const bool f32 = kind == SPR_F32, f16 = kind == SPR_F16;
  const size_t buf_bytes = align_up(effnet_buf_floats(plan, n, in_h, in_w) * sizeof(float), 256);
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  void* x = ws;                   // block input
  void* y = ws + 3 * buf_bytes;   // block output
  void* tmp[2] = {ws + buf_bytes, ws + 2 * buf_bytes};
  float* pooled = reinterpret_cast<float*>(ws + 4 * buf_bytes);
  float* factors = pooled + align_up(static_cast<size_t>(n) * plan->max_expand_p * sizeof(float), 256) / sizeof(float);
  float* hidden = factors + align_up(static_cast<size_t>(n) * plan->max_expand_p * sizeof(float), 256) / sizeof(float);
  TraceLayout lay;
  if (trace) lay = effnet_trace_layout(plan, n, in_h, in_w);
  int h = in_h, w = in_w;
  int rc;
  size_t i = 0;
  if (f32) {  // the normalised image with 16 channels: op 0 is an ordinary convolution behind it
    const size_t pixels = static_cast<size_t>(n) * in_h * in_w;
    hipLaunchKernelGGL(enet_input_kernel, blocks_of(pixels), dim3(kThreads), 0, s, images, pixels, in_channels, mean3[0], mean3[1],
                       mean3[2], inv_std3[0], inv_std3[1], inv_std3[2], static_cast<float*>(x));
    rc = check_launch("enet_input_kernel");
    if (rc != SPR_OK) return rc;
  } else {    // op 0 on the matrix-core stem: 3x3 / stride 2, 3 -> 64 (padded), SiLU, pre-processing fused
    const EOp& o = plan->ops[0];
    if (plan->ops.size() == 1 || o.cout_p != 64) { set_error("spr_effnet_forward: a 16-bit plan needs layers behind a 64-wide stem"); return SPR_ERR_UNSUPPORTED; }
    rc = launch_stem16(kind, 3, 2, images, n, h, w, in_channels, mean3, inv_std3, reinterpret_cast<const uint16_t*>(pk + o.w_off),
                       pk + o.b_off, 2, static_cast<uint16_t*>(x), s);
    if (rc == SPR_OK) rc = trace_copy(trace, &lay, 0, x, s);
    if (rc != SPR_OK) return rc;
    h = (h - 1) / 2 + 1; w = (w - 1) / 2 + 1;
    i = 1;
  }
  const void* cur = x;  // what the next layer reads
  int ti = 0;
  const float* scale = nullptr;
  for (; i < plan->ops.size(); ++i) {
    const EOp& o = plan->ops[i];
    const bool last = i + 1 == plan->ops.size();
    if (o.kind == 0) {
      void* dst = o.block_end ? y : tmp[ti];
      ConvCall k;
      // (cin_p, cout_p: the channel counts of the tensors = the padded widths of the layer)
      k.ks = o.ks; k.stride = o.stride; k.n = n; k.h = h; k.w = w; k.cin = o.cin_p; k.cout = o.cout_p;
      k.cout_real = f32 && !last ? 0 : o.cout;  // (an f32 NHWC store honours it: the padded channels must be written)
      k.in = cur; k.wts = pk + o.w_off; k.bias = pk + o.b_off; k.res = o.res ? x : nullptr; k.in_scale = o.scaled ? scale : nullptr;
      k.act = o.act; k.out = dst; k.out_nchw = last ? out : nullptr;
      if (taps && o.block_end && !last && plan->ops[i + 1].feature != o.feature) {  // a stage's end: features[:feature + 1]
        k.tap_nchw = taps->find(o.feature + 1);
        k.tap_real = o.cout;
      }
      rc = f32 ? launch_conv_gemm(k, s) : launch_conv_gemm16(kind, k, false, s);
      if (rc == SPR_OK) rc = trace_copy(trace, &lay, i, last ? static_cast<void*>(out) : dst, s);
      if (rc != SPR_OK) return rc;
      if (o.stride == 2) { h = (h - 1) / 2 + 1; w = (w - 1) / 2 + 1; }
      if (o.block_end) {  // the block's output becomes the next block's input
        std::swap(x, y);
        cur = x;
        ti = 0;
      } else {
        cur = dst;
        ti ^= 1;
      }
    } else if (o.kind == 1) {
      void* dst = tmp[ti];
      const int ho = (h - 1) / o.stride + 1, wo = (w - 1) / o.stride + 1;
      const dim3 grid = blocks_of(static_cast<size_t>(n) * ho * wo * (o.cin_p / (f32 ? 4 : 8)));  // channels per work-item
      if (f32) {
        hipLaunchKernelGGL(enet_dw_kernel, grid, dim3(kThreads), 0, s, static_cast<const float*>(cur), static_cast<int>(n), h, w,
                           o.cin_p, o.stride, o.ks, pk + o.w_off, pk + o.b_off, static_cast<float*>(dst));
      } else {
        hipLaunchKernelGGL(f16 ? enet_dw16_kernel<SPR_F16> : enet_dw16_kernel<SPR_BF16>, grid, dim3(kThreads), 0, s,
                           static_cast<const uint16_t*>(cur), static_cast<int>(n), h, w, o.cin_p, o.stride, o.ks, pk + o.w_off,
                           pk + o.b_off, static_cast<uint16_t*>(dst));
      }
      rc = check_launch(f32 ? "enet_dw_kernel" : "enet_dw16_kernel");
      if (rc == SPR_OK) rc = trace_copy(trace, &lay, i, dst, s);
      if (rc != SPR_OK) return rc;
      h = ho; w = wo;
      cur = dst;
      ti ^= 1;
    } else {
      const dim3 grid(o.cin_p / 64, static_cast<unsigned>(n));
      if (f32) {
        hipLaunchKernelGGL(enet_pool_kernel, grid, dim3(kThreads), 0, s, static_cast<const float*>(cur), h * w, o.cin_p, pooled);
      } else {
        hipLaunchKernelGGL(f16 ? enet_pool16_kernel<SPR_F16> : enet_pool16_kernel<SPR_BF16>, grid, dim3(kThreads), 0, s,
                           static_cast<const uint16_t*>(cur), h * w, o.cin_p, pooled);
      }
      rc = check_launch(f32 ? "enet_pool_kernel" : "enet_pool16_kernel");
      if (rc != SPR_OK) return rc;
      rc = launch_enet_fc(pooled, n, o.cin_p, o.sq, pk + o.w_off, pk + o.b_off, pk + o.w2_off, pk + o.b2_off, hidden, factors, s);
      if (rc == SPR_OK) rc = trace_copy(trace, &lay, i, factors, s);
      if (rc != SPR_OK) return rc;
      scale = factors;
    }
  }
  return SPR_OK;
}

// the accepted taps of a plan: every stage end below its block (a stage's last layer is a block-end convolution)
static std::vector<int> effnet_taps(const spr_effnet_plan* plan) {
  std::vector<int> ends;
  for (int t = 2; t < plan->block; ++t) ends.push_back(t);
  return ends;
}

extern "C" int spr_effnet_tap_shape(const spr_effnet_plan* plan, int32_t tap_feature, int32_t in_h, int32_t in_w,
                                    int32_t* channels, int32_t* out_h, int32_t* out_w) {
  if (!plan || !channels || !out_h || !out_w || in_h < 1 || in_w < 1) { set_error("spr_effnet_tap_shape: bad argument"); return SPR_ERR_ARG; }
  const int rc = check_tap("spr_effnet_tap_shape", effnet_taps(plan), plan->block, tap_feature);
  if (rc != SPR_OK) return rc;
  int hh = in_h, ww = in_w, cc = 3;
  for (const EOp& o : plan->ops) {  // (effnet_dims over features[:tap_feature])
    if (o.feature >= tap_feature) break;
    if (o.kind == 2) continue;
    if (o.stride == 2) { hh = (hh - 1) / 2 + 1; ww = (ww - 1) / 2 + 1; }
    cc = o.cout;
  }
  *channels = cc; *out_h = hh; *out_w = ww;
  return SPR_OK;
}

extern "C" int spr_effnet_forward_taps(spr_effnet_plan* plan, const uint8_t* images, int64_t n, int32_t in_h, int32_t in_w,
                                       int32_t in_channels, const float* mean3, const float* inv_std3, const void* packed,
                                       void* workspace, float* out, int32_t n_taps, const int32_t* tap_features,
                                       float* const* tap_out, spr_stream_t stream) {
  if (!plan) { set_error("spr_effnet_forward_taps: null plan"); return SPR_ERR_ARG; }
  TapSet taps;
  const int rc = check_taps("spr_effnet_forward_taps", effnet_taps(plan), plan->block, n_taps, tap_features, tap_out, n, &taps);
  if (rc != SPR_OK) return rc;
  return effnet_forward(plan, images, n, in_h, in_w, in_channels, mean3, inv_std3, packed, workspace, out, stream, nullptr, &taps);
}

extern "C" int spr_effnet_forward_trace(spr_effnet_plan* plan, const uint8_t* images, int64_t n, int32_t in_h, int32_t in_w,
                                        int32_t in_channels, const float* mean3, const float* inv_std3, const void* packed,
                                        void* workspace, float* out, void* trace, spr_stream_t stream) {
  if (!plan || !trace) { set_error("spr_effnet_forward_trace: null pointer"); return SPR_ERR_ARG; }
  return effnet_forward(plan, images, n, in_h, in_w, in_channels, mean3, inv_std3, packed, workspace, out, stream,
                        static_cast<unsigned char*>(trace));
}

extern "C" int spr_effnet_forward(spr_effnet_plan* plan, const uint8_t* images, int64_t n, int32_t in_h, int32_t in_w,
                                  int32_t in_channels, const float* mean3, const float* inv_std3, const void* packed,
                                  void* workspace, float* out, spr_stream_t stream) {
  return effnet_forward(plan, images, n, in_h, in_w, in_channels, mean3, inv_std3, packed, workspace, out, stream, nullptr);
}
