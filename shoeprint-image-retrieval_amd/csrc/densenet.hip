// DenseNet_201 truncations (network.py:176-179, :185-186): the plan, the dnet_* kernels and every spr_densenet_* entry point;
// the stem, its max pool and the convolutions run on the shared kernels of conv_gemm.hip.
// torchvision's densenet201: features = [conv0, norm0, relu0, pool0, denseblock1, transition1, denseblock2, transition2,
// denseblock3, transition3, denseblock4, norm5]; the reference keeps features[:block], block in [1, 12].  A dense layer is
// BatchNorm + ReLU -> 1x1 convolution (128) -> BatchNorm + ReLU -> 3x3 convolution (32), concatenated behind its input: the
// first BatchNorm + ReLU runs while the 1x1 convolution loads its operand (per-channel affine + ReLU), the second is folded
// into that convolution, and the 3x3 convolution stores its 32 channels into the block's tensor at their offset.
//
// 16-bit plans (spr_densenet_plan_create_ex with SPR_F16 / SPR_BF16, block >= 5): the same graph on v_mfma_f32_16x16x32 with
// every tensor between layers stored in the compute type T.  The rounding points, in full (round16 = to T, nearest even):
//   - weights: conv0 with norm0 folded, a dense layer's 1x1 with its second BatchNorm folded (w * s2, in float32), the 3x3 and
//     the transition 1x1 as they are; each rounded once when the caller packs them.  Biases (norm0's shift, the second
//     BatchNorm's shift; zero for the 3x3 and the transitions) and every pre-activation scale / shift stay float32.
//   - stem: the normalised image (x / 255 - mean) * (1 / std) is rounded to T; store round16(max(acc + b, 0)).
//   - max pool: the maximum of stored values (exact), into channels [0, 64) of block 1's tensor.
//   - dense 1x1 and transition 1x1: the operand is round16(max(fmaf(x, s[c], t[c]), 0)), x the stored value, one float32 fmaf;
//     float32 accumulation, + float32 bias; the dense 1x1 stores round16(max(., 0)), the transition round16(.).
//   - dense 3x3: the operand is the stored 128-channel intermediate, zero outside the image; store round16(acc) (zero bias)
//     into channels [c_off, c_off + 32) of the block tensor.
//   - transition pool: ((a + b) + c) + d of the four stored convolution results in float32 (a, b the upper row), times 0.25,
//     one round16, into channels [0, cout) of the next block's tensor.  (The pool stays BEHIND the convolution.)
//   - output: the last tensor's stored values as float32 NCHW; with block == 12, fmaf(x, s[c], t[c]) (norm5) in float32.
// Channels of a block tensor behind the reading layer's cin are unwritten while that layer runs; the staging neither loads
// them nor multiplies them (the half chunk behind cin is skipped), so the workspace needs no initialisation.
#include <algorithm>
#include <cmath>
#include <new>
#include <utility>
#include <vector>

#include "conv_gemm.h"

namespace spr {
namespace {

// ---------------------------------------------------------------- building blocks
// 2x2 / stride 2 average pool (a transition's tail), NHWC [..][C] -> NHWC with channel stride ldo
__global__ void __launch_bounds__(kThreads)
dnet_avgpool_kernel(const float* __restrict__ in, int H, int W, int C, float* __restrict__ out, size_t total, int ldo) {
  const int Ho = H / 2, Wo = W / 2;
  for (size_t i = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x; i < total;
       i += static_cast<size_t>(gridDim.x) * kThreads) {
    const int c = static_cast<int>(i % C);
    size_t p = i / C;
    const int ox = static_cast<int>(p % Wo); p /= Wo;
    const int oy = static_cast<int>(p % Ho);
    const size_t img = p / Ho;
    const float* b = in + ((img * H + 2 * oy) * static_cast<size_t>(W) + 2 * ox) * C + c;
    out[(i / C) * ldo + c] = (b[0] + b[C] + b[static_cast<size_t>(W) * C] + b[static_cast<size_t>(W) * C + C]) * 0.25f;
  }
}

// NHWC (channel stride ld, C channels) -> NCHW with an optional per-channel x * s + t (the closing BatchNorm) and ReLU
__global__ void __launch_bounds__(kThreads)
dnet_out_kernel(const float* __restrict__ in, int HW, int C, int ld, const float* __restrict__ sc, const float* __restrict__ sh,
                int relu, float* __restrict__ out, size_t total) {
  for (size_t i = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x; i < total;
       i += static_cast<size_t>(gridDim.x) * kThreads) {
    const int p = static_cast<int>(i % HW);
    const int c = static_cast<int>((i / HW) % C);
    const size_t img = i / (static_cast<size_t>(HW) * C);
    float v = in[(img * HW + p) * ld + c];
    if (sc) v = fmaf(v, sc[c], sh[c]);
    if (relu) v = fmaxf(v, 0.0f);
    out[i] = v;
  }
}

// ---------------------------------------------------------------- 16-bit plans: implicit GEMM on v_mfma_f32_16x16x32
// The dense layers' and transitions' convolutions (1x1 and 3x3, stride 1) with float16 / bfloat16 operands and f32
// accumulation; conv_gemm16_kernel's tile and LDS layout (workgroup = 128 pixels x BN channels x a K chunk of 64; operand rows
// of 128 bytes = eight 16-byte slots, slot s of row r at s ^ ((r >> 1) & 7); registers loaded one chunk ahead), plus what
// DenseNet needs: the input is read with channel stride lda (the first cin channels of a block tensor), the operand may take
// a per-channel max(fmaf(x, s, t), 0) in the staging registers (rounded to the operand type again), cin is a multiple of 32 -
// a chunk that holds only 32 real channels stages and multiplies one k-step - and the result goes to channels
// [c_off + BN * blockIdx.y, ...) of a tensor with channel stride ldc.  BN = 64: four waves x (32 pixels x 64 channels);
// BN = 32 (the 3x3 layers, 32 output channels): four waves x (32 pixels x 32 channels).
// Packed weights: [cout / BN][taps * ceil(cin / 64)][n: BN][k: 64] 16-bit, k = channel inside the chunk, zero behind cin.
// grid = (ceil(M / 128), cout / BN)
constexpr int kDM = 128, kDK = 64, kDRowDw = 32;

template <int KS, int KIND, int BN>
__global__ void __launch_bounds__(kThreads, 3)
dnet_gemm16_kernel(const uint16_t* __restrict__ in, int n_img, int H, int W, int cin, int lda, const uint16_t* __restrict__ wts,
                   const float* __restrict__ bias, const float* __restrict__ pre_s, const float* __restrict__ pre_t, int relu,
                   uint16_t* __restrict__ out, int ldc, int c_off) {
  constexpr int kT = BN + 4;  // row stride (floats) of the f32 output tile: rows 4 apart lie 16 banks apart
  constexpr int kLdsDw = kDM * kT > (kDM + BN) * kDRowDw ? kDM * kT : (kDM + BN) * kDRowDw;
  __shared__ __attribute__((aligned(16))) uint32_t lds16[kLdsDw];
  uint32_t* A = lds16;
  uint32_t* B = lds16 + kDM * kDRowDw;
  constexpr int PAD = KS / 2;
  constexpr int NJ = BN / 16;  // 16-channel blocks per wave
  const long long M = static_cast<long long>(n_img) * H * W;
  const int tid = static_cast<int>(threadIdx.x);
  const int wave = tid >> 6, lane = tid & 63;
  const int p = lane & 15, q = lane >> 4;
  const int cb = static_cast<int>(blockIdx.y);
  const long long m0 = static_cast<long long>(blockIdx.x) * kDM;
  const int cchunks = (cin + kDK - 1) / kDK, chunks = KS * KS * cchunks;
  const bool half_tail = (cin & 32) != 0;  // the last chunk of a tap holds 32 channels: one k-step
  const int wm = wave * 32;

  // staging role: 16-byte slot `ss` of rows sr + 32 k (A: k = 0..3; B: row sr, work-items of rows < BN)
  const int sr = tid >> 3, ss = tid & 7;
  int ay[4], ax[4];
  long long abase[4];  // element offset of pixel (img, 0, 0); negative marks a row beyond M
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const long long pm = m0 + sr + 32 * k;
    if (pm < M) {
      const int px = static_cast<int>(pm % W), py = static_cast<int>((pm / W) % H);
      const long long pimg = pm / (static_cast<long long>(W) * H);
      ay[k] = py - PAD; ax[k] = px - PAD;
      abase[k] = pimg * H * static_cast<long long>(W) * lda;
    } else {
      ay[k] = ax[k] = 0; abase[k] = -1;
    }
  }
  const uint16_t* wbase = wts + static_cast<size_t>(cb) * chunks * (BN * kDK) + ss * 8;

  f32x4 acc[2][NJ];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  u32x4 ra[4], rb[BN / 32];
  auto request = [&](int ch) {
    const int tap = ch / cchunks, cc = ch - tap * cchunks;
    const int dy = tap / KS, dx = tap - dy * KS;
    const int c0 = cc * kDK + ss * 8;  // first of this work-item's eight channels
    const bool c_ok = c0 < cin;        // (behind cin: not loaded - those channels of a block tensor are not written yet)
    float sv[8], tv[8];
    if (pre_s && c_ok) {
      const float4 s0 = *reinterpret_cast<const float4*>(pre_s + c0), s1 = *reinterpret_cast<const float4*>(pre_s + c0 + 4);
      const float4 t0 = *reinterpret_cast<const float4*>(pre_t + c0), t1 = *reinterpret_cast<const float4*>(pre_t + c0 + 4);
      sv[0] = s0.x; sv[1] = s0.y; sv[2] = s0.z; sv[3] = s0.w; sv[4] = s1.x; sv[5] = s1.y; sv[6] = s1.z; sv[7] = s1.w;
      tv[0] = t0.x; tv[1] = t0.y; tv[2] = t0.z; tv[3] = t0.w; tv[4] = t1.x; tv[5] = t1.y; tv[6] = t1.z; tv[7] = t1.w;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int y = ay[k] + dy, x = ax[k] + dx;
      ra[k] = u32x4{0u, 0u, 0u, 0u};
      if (c_ok && abase[k] >= 0 && y >= 0 && y < H && x >= 0 && x < W) {
        ra[k] = *reinterpret_cast<const u32x4*>(in + abase[k] + (static_cast<long long>(y) * W + x) * lda + c0);
        if (pre_s) {  // BatchNorm + ReLU in front of the convolution, rounded to the operand type again
          u32x4 r;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float lo = fmaxf(fmaf(value16<KIND>(static_cast<uint16_t>(ra[k][e] & 0xffffu)), sv[2 * e], tv[2 * e]), 0.0f);
            const float hi = fmaxf(fmaf(value16<KIND>(static_cast<uint16_t>(ra[k][e] >> 16)), sv[2 * e + 1], tv[2 * e + 1]), 0.0f);
            r[e] = static_cast<uint32_t>(round16<KIND>(lo)) | (static_cast<uint32_t>(round16<KIND>(hi)) << 16);
          }
          ra[k] = r;
        }
      }
    }
#pragma unroll
    for (int k = 0; k < BN / 32; ++k)
      rb[k] = *reinterpret_cast<const u32x4*>(wbase + (static_cast<size_t>(ch) * BN + sr + 32 * k) * kDK);
  };
  auto slot = [](int row, int s) { return (s ^ ((row >> 1) & 7)) << 2; };  // dword offset of 16-byte slot s inside row `row`
  request(0);
  int cc = 0;  // chunk index inside the tap
  for (int ch = 0; ch < chunks; ++ch) {
    __syncthreads();  // the previous chunk's fragments are consumed
#pragma unroll
    for (int k = 0; k < 4; ++k) *reinterpret_cast<u32x4*>(A + (sr + 32 * k) * kDRowDw + slot(sr + 32 * k, ss)) = ra[k];
#pragma unroll
    for (int k = 0; k < BN / 32; ++k) *reinterpret_cast<u32x4*>(B + (sr + 32 * k) * kDRowDw + slot(sr + 32 * k, ss)) = rb[k];
    __syncthreads();
    if (ch + 1 < chunks) request(ch + 1);
    const int ksteps = (half_tail && cc + 1 == cchunks) ? 1 : 2;
    cc = cc + 1 == cchunks ? 0 : cc + 1;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      if (ks >= ksteps) break;
      u32x4 a[2], b[NJ];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int row = wm + i * 16 + p;
        a[i] = *reinterpret_cast<const u32x4*>(A + row * kDRowDw + slot(row, ks * 4 + q));
      }
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int row = j * 16 + p;
        b[j] = *reinterpret_cast<const u32x4*>(B + row * kDRowDw + slot(row, ks * 4 + q));
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
          acc[i][j] = KIND == SPR_F16 ? mfma_f16_16x16x32(a[i], b[j], acc[i][j]) : mfma_bf16_16x16x32(a[i], b[j], acc[i][j]);
    }
  }
  // ---- epilogue: the accumulators (+ bias) go through LDS as an f32 tile and leave as 16-byte pieces of 8 channels
  float* T = reinterpret_cast<float*>(lds16);
  __syncthreads();  // the operand tiles are consumed
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const float bv = bias[cb * BN + j * 16 + p];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) T[(wm + i * 16 + 4 * q + r) * kT + j * 16 + p] = acc[i][j][r] + bv;
  }
  __syncthreads();
  constexpr int PP = BN / 8;  // 16-byte pieces per row
  const int er = tid / PP, ep = tid % PP;
#pragma unroll
  for (int k = 0; k < PP / 2; ++k) {
    const int row = er + (kThreads / PP) * k;
    const long long m = m0 + row;
    if (m >= M) continue;
    const float4 lo = *reinterpret_cast<const float4*>(T + row * kT + ep * 8);
    const float4 hi = *reinterpret_cast<const float4*>(T + row * kT + ep * 8 + 4);
    const float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    u32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float a0 = relu ? fmaxf(v[2 * e], 0.0f) : v[2 * e], a1 = relu ? fmaxf(v[2 * e + 1], 0.0f) : v[2 * e + 1];
      o[e] = static_cast<uint32_t>(round16<KIND>(a0)) | (static_cast<uint32_t>(round16<KIND>(a1)) << 16);
    }
    *reinterpret_cast<u32x4*>(out + static_cast<size_t>(m) * ldc + c_off + cb * BN + ep * 8) = o;
  }
}

// 2x2 / stride 2 average pool of a 16-bit plan (a transition's tail): NHWC [..][C] -> NHWC with channel stride ldo, eight
// channels (16 bytes) per work-item; ((a + b) + c) + d in float32 (a, b the upper row), times 0.25, one rounding
template <int KIND>
__global__ void __launch_bounds__(kThreads)
dnet_avgpool16_kernel(const uint16_t* __restrict__ in, int H, int W, int C, uint16_t* __restrict__ out, size_t total8, int ldo) {
  const int Ho = H / 2, Wo = W / 2, c8 = C / 8;
  for (size_t i = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x; i < total8;
       i += static_cast<size_t>(gridDim.x) * kThreads) {
    const int c = static_cast<int>(i % c8) * 8;
    size_t px = i / c8;
    const int ox = static_cast<int>(px % Wo); px /= Wo;
    const int oy = static_cast<int>(px % Ho);
    const size_t img = px / Ho;
    const uint16_t* b = in + ((img * H + 2 * oy) * static_cast<size_t>(W) + 2 * ox) * C + c;
    const u32x4 v0 = *reinterpret_cast<const u32x4*>(b), v1 = *reinterpret_cast<const u32x4*>(b + C);
    const u32x4 v2 = *reinterpret_cast<const u32x4*>(b + static_cast<size_t>(W) * C);
    const u32x4 v3 = *reinterpret_cast<const u32x4*>(b + static_cast<size_t>(W) * C + C);
    u32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      uint32_t pair = 0;
#pragma unroll
      for (int hf = 0; hf < 2; ++hf) {
        const int sh = 16 * hf;
        const float m = (((value16<KIND>(static_cast<uint16_t>(v0[e] >> sh)) + value16<KIND>(static_cast<uint16_t>(v1[e] >> sh))) +
                          value16<KIND>(static_cast<uint16_t>(v2[e] >> sh))) + value16<KIND>(static_cast<uint16_t>(v3[e] >> sh))) * 0.25f;
        pair |= static_cast<uint32_t>(round16<KIND>(m)) << sh;
      }
      o[e] = pair;
    }
    *reinterpret_cast<u32x4*>(out + (i / c8) * ldo + c) = o;
  }
}

// the closing kernel of a 16-bit plan: 16-bit NHWC (channel stride ld, C channels) -> float32 NCHW, with the closing
// BatchNorm as fmaf(x, s[c], t[c]) in float32 (sc null: the stored values as they are)
template <int KIND>
__global__ void __launch_bounds__(kThreads)
dnet_out16_kernel(const uint16_t* __restrict__ in, int HW, int C, int ld, const float* __restrict__ sc, const float* __restrict__ sh,
                  float* __restrict__ out, size_t total) {
  for (size_t i = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x; i < total;
       i += static_cast<size_t>(gridDim.x) * kThreads) {
    const int p = static_cast<int>(i % HW);
    const int c = static_cast<int>((i / HW) % C);
    const size_t img = i / (static_cast<size_t>(HW) * C);
    float v = value16<KIND>(in[(img * HW + p) * ld + c]);
    if (sc) v = fmaf(v, sc[c], sh[c]);
    out[i] = v;
  }
}

// ---------------------------------------------------------------- the plan
struct DOp {
  int kind;     // 0 stem (7x7 / 2 convolution [+ BatchNorm] [+ ReLU] [+ 3x3 / 2 max pool]), 1 dense 1x1, 2 dense 3x3,
                // 3 transition (BatchNorm + ReLU + 1x1 + 2x2 average pool), 4 closing BatchNorm
  int cin, cout;
  int c_off;    // dense 3x3: channel offset of its output in the block's tensor
  int ctot;     // channels of the tensor this layer reads (kinds 1, 3, 4) or writes into (kind 2)
  int flags;    // stem: 1 BatchNorm folded, 2 ReLU, 4 max pool
  int feature;
  size_t w_off, b_off, s_off, t_off;  // packed offsets (floats): weights, bias, pre-activation scale / shift
};
const int kDenseLayers[4] = {6, 12, 48, 32};
}  // namespace
}  // namespace spr

using namespace spr;

struct spr_densenet_plan {
  int block;
  int compute;  // SPR_F32 (exact) | SPR_F16 | SPR_BF16 (16-bit operands and stored tensors, f32 accumulation)
  std::vector<DOp> ops;
  size_t packed_floats;
};

extern "C" int spr_densenet_plan_create(int32_t block, spr_densenet_plan** plan_out) {
  return spr_densenet_plan_create_ex(block, SPR_F32, plan_out);
}

extern "C" int spr_densenet_plan_compute(const spr_densenet_plan* plan) { return plan ? plan->compute : SPR_ERR_ARG; }

extern "C" int spr_densenet_plan_create_ex(int32_t block, int32_t compute, spr_densenet_plan** plan_out) {
  if (!plan_out) { set_error("spr_densenet_plan_create: null pointer"); return SPR_ERR_ARG; }
  *plan_out = nullptr;
  if (compute == SPR_COMPUTE_BF16X3) {
    set_error("spr_densenet_plan_create_ex: SPR_COMPUTE_BF16X3 (bfloat16x3, the hi + lo split) is built for the plain-VGG plans only");
    return SPR_ERR_UNSUPPORTED;
  }
  if (compute != SPR_F32 && compute != SPR_F16 && compute != SPR_BF16) {
    set_error("spr_densenet_plan_create_ex: compute type %d (SPR_F32 | SPR_F16 | SPR_BF16)", compute);
    return SPR_ERR_ARG;
  }
  if (block < 1 || block > 12) { set_error("spr_densenet_plan_create: block %d: features[:block] with block in [1, 12]", block); return SPR_ERR_ARG; }
  const bool h16 = compute != SPR_F32;
  if (h16 && block < 5) {
    set_error("spr_densenet_plan_create_ex: block %d: a 16-bit plan needs a dense block behind the stem (block >= 5)", block);
    return SPR_ERR_UNSUPPORTED;
  }
  spr_densenet_plan* plan = new (std::nothrow) spr_densenet_plan();
  if (!plan) { set_error("out of host memory"); return SPR_ERR_ARG; }
  plan->block = block;
  plan->compute = compute;
  size_t off = 0;
  auto take = [&](size_t n) { const size_t o = off; off += (n + 3) / 4 * 4; return o; };
  // weights of a 16-bit plan: two to a float slot, the reduction padded to whole 64-channel chunks per tap
  auto take_w16 = [&](int cout, int cin, int taps) { return take(static_cast<size_t>(cout) * taps * ((cin + 63) / 64 * 64) / 2); };
  {
    DOp o{};
    o.kind = 0; o.cin = 3; o.cout = 64; o.feature = 0;
    o.flags = (block >= 2 ? 1 : 0) | (block >= 3 ? 2 : 0) | (block >= 4 ? 4 : 0);
    o.w_off = h16 ? take(160 * 64 / 2) : take(147 * 64);  // (16-bit: stem16_kernel's 160 x 64 matrix)
    o.b_off = take(64);
    plan->ops.push_back(o);
  }
  int c = 64;
  for (int b = 0; b < 4 && 4 + 2 * b < block; ++b) {
    const int ctot = c + 32 * kDenseLayers[b];
    for (int l = 0; l < kDenseLayers[b]; ++l) {
      DOp a{};
      a.kind = 1; a.cin = c + 32 * l; a.cout = 128; a.ctot = ctot; a.feature = 4 + 2 * b;
      a.s_off = take(a.cin); a.t_off = take(a.cin);
      a.w_off = h16 ? take_w16(128, a.cin, 1) : take(static_cast<size_t>(128) * a.cin);
      a.b_off = take(128);
      plan->ops.push_back(a);
      DOp d{};
      d.kind = 2; d.cin = 128; d.cout = 32; d.c_off = c + 32 * l; d.ctot = ctot; d.feature = 4 + 2 * b;
      if (h16) { d.w_off = take_w16(32, 128, 9); d.b_off = take(32); }  // the 32-channel instance: nothing padded
      else { d.w_off = take(static_cast<size_t>(64) * 128 * 9); d.b_off = take(64); }  // output channels padded to the 64-wide tile
      plan->ops.push_back(d);
    }
    c = ctot;
    if (b < 3 && 5 + 2 * b < block) {
      DOp t{};
      t.kind = 3; t.cin = c; t.cout = c / 2; t.ctot = c; t.feature = 5 + 2 * b;
      t.s_off = take(c); t.t_off = take(c);
      t.w_off = h16 ? take_w16(c / 2, c, 1) : take(static_cast<size_t>(c / 2) * c);
      t.b_off = take(c / 2);
      plan->ops.push_back(t);
      c /= 2;
    }
  }
  if (block == 12) {
    DOp n{};
    n.kind = 4; n.cin = n.cout = c; n.ctot = c; n.feature = 11;
    n.s_off = take(c); n.t_off = take(c);
    plan->ops.push_back(n);
  }
  plan->packed_floats = off;
  *plan_out = plan;
  return SPR_OK;
}

extern "C" void spr_densenet_plan_destroy(spr_densenet_plan* plan) { delete plan; }
extern "C" int spr_densenet_num_ops(const spr_densenet_plan* plan) { return plan ? static_cast<int>(plan->ops.size()) : SPR_ERR_ARG; }
extern "C" size_t spr_densenet_packed_bytes(const spr_densenet_plan* plan) { return plan ? plan->packed_floats * sizeof(float) : 0; }

// info[12] = kind, cin, cout, c_off, ctot, flags, feature, then the packed offsets (floats) w, b, s, t, then 0
extern "C" int spr_densenet_op_info(const spr_densenet_plan* plan, int32_t i, int32_t* info) {
  if (!plan || !info || i < 0 || i >= static_cast<int>(plan->ops.size())) { set_error("spr_densenet_op_info: bad argument"); return SPR_ERR_ARG; }
  const DOp& o = plan->ops[i];
  const int32_t v[12] = {o.kind, o.cin, o.cout, o.c_off, o.ctot, o.flags, o.feature, static_cast<int32_t>(o.w_off),
                         static_cast<int32_t>(o.b_off), static_cast<int32_t>(o.s_off), static_cast<int32_t>(o.t_off), 0};
  for (int k = 0; k < 12; ++k) info[k] = v[k];
  return SPR_OK;
}

static void densenet_dims(const spr_densenet_plan* plan, int in_h, int in_w, int* c, int* h, int* w) {
  int hh = (in_h + 1) / 2, ww = (in_w + 1) / 2, cc = 64;  // conv0: 7x7 s2 p3
  if (plan->block >= 4) { hh = (hh + 1) / 2; ww = (ww + 1) / 2; }
  for (const DOp& o : plan->ops) {
    if (o.kind == 2) cc = o.c_off + 32;
    if (o.kind == 3) { hh /= 2; ww /= 2; cc = o.cout; }
  }
  *c = cc; *h = hh; *w = ww;
}

extern "C" int spr_densenet_output_shape(const spr_densenet_plan* plan, int32_t in_h, int32_t in_w, int32_t* channels,
                                         int32_t* out_h, int32_t* out_w) {
  if (!plan || !channels || !out_h || !out_w || in_h < 1 || in_w < 1) { set_error("spr_densenet_output_shape: bad argument"); return SPR_ERR_ARG; }
  densenet_dims(plan, in_h, in_w, channels, out_h, out_w);
  return SPR_OK;
}

// three buffers as large as the largest tensor: the stem's output (64 channels at half resolution) or a block's tensor
static size_t densenet_buf_floats(const spr_densenet_plan* plan, int64_t n, int in_h, int in_w) {
  int hh = (in_h + 1) / 2, ww = (in_w + 1) / 2;
  size_t best = static_cast<size_t>(n) * hh * ww * 64;
  if (plan->block >= 4) { hh = (hh + 1) / 2; ww = (ww + 1) / 2; }
  for (const DOp& o : plan->ops) {
    if (o.kind == 1 || o.kind == 3) {
      const size_t f = static_cast<size_t>(n) * hh * ww * o.ctot;
      if (f > best) best = f;
    }
    if (o.kind == 3) { hh /= 2; ww /= 2; }
  }
  return best;
}
extern "C" size_t spr_densenet_workspace_bytes(const spr_densenet_plan* plan, int64_t n, int32_t in_h, int32_t in_w) {
  if (!plan || n < 0) return 0;
  const size_t elem = plan->compute == SPR_F32 ? sizeof(float) : sizeof(uint16_t);  // (16-bit plans: the same three tensors)
  return 3 * align_up(densenet_buf_floats(plan, n, in_h, in_w) * elem, 256);
}

namespace {
template <int KS, int BN>
auto dnet_gemm16_of(int kind) {
  return kind == SPR_F16 ? dnet_gemm16_kernel<KS, SPR_F16, BN> : dnet_gemm16_kernel<KS, SPR_BF16, BN>;
}

// one convolution of a 16-bit plan: 1x1 with 64-channel tiles (cout a multiple of 64) or 3x3 -> 32 channels; stride 1, ReLU
// or nothing behind it, NHWC out
int launch_dnet_gemm16(int kind, const ConvCall& c, hipStream_t s) {
  if (c.stride != 1 || c.res || c.in_scale || c.out_nchw || c.tap_nchw || c.cout_real || c.act > 1 || !c.pre_s != !c.pre_t) {
    set_error("launch_dnet_gemm16: dnet_gemm16_kernel has no stride, residual, input factors, SiLU, NCHW result or padded cout");
    return SPR_ERR_UNSUPPORTED;
  }
  const int ks = c.ks, cin = c.cin, cout = c.cout, lda = c.in_stride(), ldc = c.out_stride(), c_off = c.c_off;
  const bool ok = cin % 32 == 0 && lda % 8 == 0 && ldc % 8 == 0 && c_off % 8 == 0 && lda >= cin &&
                  ((ks == 1 && cout % 64 == 0) || (ks == 3 && cout == 32)) && c_off + cout <= ldc;
  if (!ok) { set_error("launch_dnet_gemm16: no instance for %d x %d, %d -> %d channels", ks, ks, cin, cout); return SPR_ERR_UNSUPPORTED; }
  auto kernel = ks == 1 ? dnet_gemm16_of<1, 64>(kind) : dnet_gemm16_of<3, 32>(kind);
  const int bn = ks == 1 ? 64 : 32;
  const long long m = static_cast<long long>(c.n) * c.h * c.w;
  hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>((m + kDM - 1) / kDM), static_cast<unsigned>(cout / bn)), dim3(kThreads), 0,
                     s, static_cast<const uint16_t*>(c.in), static_cast<int>(c.n), c.h, c.w, cin, lda,
                     static_cast<const uint16_t*>(c.wts), c.bias, c.pre_s, c.pre_t, c.act, static_cast<uint16_t*>(c.out), ldc, c_off);
  return check_launch("dnet_gemm16_kernel");
}

// width of the block tensor that starts behind op i (the pooled stem / a transition): the next dense layer's, else `fallback`
int next_ld(const spr_densenet_plan* plan, size_t i, int fallback) {
  return i + 1 < plan->ops.size() && plan->ops[i + 1].kind == 1 ? plan->ops[i + 1].ctot : fallback;
}

// Records (NHWC in the plan's compute type): the stem; block 1's tensor behind the max pool (channels [0, 64) written); per
// dense layer its 128-channel intermediate; per dense block its complete tensor behind the last layer; per transition its
// convolution's result and the next tensor behind the average pool (channels [0, cout) written); the float32 NCHW output.
TraceLayout densenet_trace_layout(const spr_densenet_plan* plan, int64_t n, int in_h, int in_w) {
  TraceLayout lay;
  lay.n = n;
  int h = (in_h + 1) / 2, w = (in_w + 1) / 2, c = 64;
  lay.add(h, w, 64, plan->compute, 0);
  if (plan->ops[0].flags & 4) {  // (an f32 plan may end in front of the max pool)
    h = (h + 1) / 2; w = (w + 1) / 2;
    lay.add(h, w, next_ld(plan, 0, 64), plan->compute, 0);
  }
  for (size_t i = 1; i < plan->ops.size(); ++i) {
    const DOp& o = plan->ops[i];
    if (o.kind == 1) lay.add(h, w, 128, plan->compute, 0);
    if (o.kind == 2) {
      c = o.c_off + 32;
      if (c == o.ctot) lay.add(h, w, o.ctot, plan->compute, 0);
    }
    if (o.kind == 3) {
      lay.add(h, w, o.cout, plan->compute, 0);
      h /= 2; w /= 2; c = o.cout;
      lay.add(h, w, next_ld(plan, i, o.cout), plan->compute, 0);
    }
  }
  lay.add(h, w, c, SPR_F32, 1);
  return lay;
}
}  // namespace

// The forward pass of both compute types: one walk over the plan, tensors in the plan's type.  trace: null (the plain
// forward), or where the records of densenet_trace_layout are copied
static int densenet_forward(spr_densenet_plan* plan, const uint8_t* images, int64_t n, int32_t in_h, int32_t in_w,
                            int32_t in_channels, const float* mean3, const float* inv_std3, const void* packed, void* workspace,
                            float* out, spr_stream_t stream, unsigned char* trace, const TapSet* taps = nullptr) {
  const int ok = check_forward_args(taps ? "spr_densenet_forward_taps" : "spr_densenet_forward", plan, images, n, in_h, in_w, in_channels, mean3, inv_std3, packed,
                                    workspace, out);
  if (ok != SPR_OK || n == 0) return ok;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const float* pk = static_cast<const float*>(packed);
  const int kind = plan->compute;
  const bool f32 = kind == SPR_F32, f16 = kind == SPR_F16;
  const size_t buf_bytes = align_up(densenet_buf_floats(plan, n, in_h, in_w) * (f32 ? sizeof(float) : sizeof(uint16_t)), 256);
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  void* cat = ws;                  // the current block's tensor (or the stem's output)
  void* tmp = ws + buf_bytes;      // the stem's output in front of its pool / a 128-channel intermediate / a transition's convolution
  void* nxt = ws + 2 * buf_bytes;  // the next block's tensor
  // one convolution (stride 1, no residual) from the first cin of lda channels of `in` into channels [c_off, c_off + cout) of
  // the ldc of `dst`; pre: BatchNorm + ReLU on the operand while it is loaded
  auto conv = [&](const DOp& o, int ks, const void* in, int h, int w, int cin, int lda, bool pre, int act, void* dst, int cout,
                  int ldc, int c_off) {
    ConvCall k;
    k.ks = ks; k.n = n; k.h = h; k.w = w; k.cin = cin; k.cout = cout; k.lda = lda; k.ldc = ldc; k.c_off = c_off;
    k.in = in; k.wts = pk + o.w_off; k.bias = pk + o.b_off; k.act = act; k.out = dst;
    if (pre) { k.pre_s = pk + o.s_off; k.pre_t = pk + o.t_off; }
    if (!f32) return launch_dnet_gemm16(kind, k, s);
    if (ks == 3) { k.cout = 64; k.cout_real = cout; }  // conv_gemm_kernel's tile: the 32 channels are packed padded to 64
    return launch_conv_gemm(k, s);
  };
  TraceLayout lay;
  if (trace) lay = densenet_trace_layout(plan, n, in_h, in_w);
  size_t rec = 0;
  int h = (in_h + 1) / 2, w = (in_w + 1) / 2, c = 64, ld = 64;
  int rc;
  {  // stem, and its max pool into the first 64 channels of block 1's tensor (a 16-bit plan has both: block >= 5)
    const DOp& o = plan->ops[0];
    void* stem_out = (o.flags & 4) ? tmp : cat;
    const int relu = (o.flags & 2) ? 1 : 0;
    rc = f32 ? launch_stem(images, n, in_h, in_w, in_channels, mean3, inv_std3, pk + o.w_off, pk + o.b_off,
                           static_cast<float*>(stem_out), relu, 0, s)
             : launch_stem16(kind, 7, 2, images, n, in_h, in_w, in_channels, mean3, inv_std3,
                             reinterpret_cast<const uint16_t*>(pk + o.w_off), pk + o.b_off, relu, static_cast<uint16_t*>(stem_out), s);
    if (rc == SPR_OK) rc = trace_copy(trace, &lay, rec++, stem_out, s);
    if (rc != SPR_OK) return rc;
    if (o.flags & 4) {
      ld = next_ld(plan, 0, 64);
      rc = f32 ? launch_maxpool3(static_cast<const float*>(tmp), n, h, w, 64, static_cast<float*>(cat), ld, s)
               : launch_maxpool3_16(static_cast<const uint16_t*>(tmp), n, h, w, 64, static_cast<uint16_t*>(cat), ld, s);
      h = (h + 1) / 2; w = (w + 1) / 2;
      if (rc == SPR_OK) rc = trace_copy(trace, &lay, rec++, cat, s);
      if (rc != SPR_OK) return rc;
    }
  }
  // the closing layout change: c channels of the live tensor (channel stride ld) -> float32 NCHW, the closing BatchNorm on the
  // way where sc is given; also a feature tap's kernel, on the block tensor as it stands behind a dense block / a transition
  auto to_nchw = [&](const void* src, const float* sc, const float* sh, float* dst) {
    const size_t total = static_cast<size_t>(n) * c * h * w;
    if (f32) {
      hipLaunchKernelGGL(dnet_out_kernel, blocks_of(total), dim3(kThreads), 0, s, static_cast<const float*>(src), h * w, c, ld, sc,
                         sh, 0, dst, total);
    } else {
      hipLaunchKernelGGL(f16 ? dnet_out16_kernel<SPR_F16> : dnet_out16_kernel<SPR_BF16>, blocks_of(total), dim3(kThreads), 0, s,
                         static_cast<const uint16_t*>(src), h * w, c, ld, sc, sh, dst, total);
    }
    return check_launch(f32 ? "dnet_out_kernel" : "dnet_out16_kernel");
  };
  const float* fin_s = nullptr;
  const float* fin_t = nullptr;
  for (size_t i = 1; i < plan->ops.size(); ++i) {
    const DOp& o = plan->ops[i];
    if (o.kind == 1) {          // BatchNorm + ReLU (operand load) -> 1x1 -> BatchNorm (folded) + ReLU
      rc = conv(o, 1, cat, h, w, o.cin, o.ctot, true, 1, tmp, 128, 128, 0);
      if (rc == SPR_OK) rc = trace_copy(trace, &lay, rec++, tmp, s);
    } else if (o.kind == 2) {   // 3x3, its 32 channels behind the layer's input
      rc = conv(o, 3, tmp, h, w, 128, 128, false, 0, cat, 32, o.ctot, o.c_off);
      c = o.c_off + 32; ld = o.ctot;
      if (rc == SPR_OK && c == o.ctot) rc = trace_copy(trace, &lay, rec++, cat, s);
    } else if (o.kind == 3) {   // BatchNorm + ReLU -> 1x1 -> 2x2 average pool into the next block's tensor
      rc = conv(o, 1, cat, h, w, o.cin, o.ctot, true, 0, tmp, o.cout, o.cout, 0);
      if (rc == SPR_OK) rc = trace_copy(trace, &lay, rec++, tmp, s);
      if (rc != SPR_OK) return rc;
      ld = next_ld(plan, i, o.cout);
      const size_t total = static_cast<size_t>(n) * (h / 2) * (w / 2) * o.cout / (f32 ? 1 : 8);  // channels per work-item
      if (f32) {
        hipLaunchKernelGGL(dnet_avgpool_kernel, blocks_of(total), dim3(kThreads), 0, s, static_cast<const float*>(tmp), h, w, o.cout,
                           static_cast<float*>(nxt), total, ld);
      } else {
        hipLaunchKernelGGL(f16 ? dnet_avgpool16_kernel<SPR_F16> : dnet_avgpool16_kernel<SPR_BF16>, blocks_of(total), dim3(kThreads), 0,
                           s, static_cast<const uint16_t*>(tmp), h, w, o.cout, static_cast<uint16_t*>(nxt), total, ld);
      }
      rc = check_launch(f32 ? "dnet_avgpool_kernel" : "dnet_avgpool16_kernel");
      std::swap(cat, nxt);
      h /= 2; w /= 2; c = o.cout;
      if (rc == SPR_OK) rc = trace_copy(trace, &lay, rec++, cat, s);
    } else {                    // the closing BatchNorm rides on the layout change below
      fin_s = pk + o.s_off; fin_t = pk + o.t_off;
    }
    if (rc != SPR_OK) return rc;
    // the last layer of child o.feature of `features`: features[:o.feature + 1] ends here
    if (taps && i + 1 < plan->ops.size() && plan->ops[i + 1].feature != o.feature) {
      if (float* tap = taps->find(o.feature + 1)) {
        rc = to_nchw(cat, nullptr, nullptr, tap);
        if (rc != SPR_OK) return rc;
      }
    }
  }
  rc = to_nchw(cat, fin_s, fin_t, out);
  if (rc == SPR_OK) rc = trace_copy(trace, &lay, rec++, out, s);
  return rc;
}

extern "C" int spr_densenet_forward(spr_densenet_plan* plan, const uint8_t* images, int64_t n, int32_t in_h, int32_t in_w,
                                    int32_t in_channels, const float* mean3, const float* inv_std3, const void* packed,
                                    void* workspace, float* out, spr_stream_t stream) {
  return densenet_forward(plan, images, n, in_h, in_w, in_channels, mean3, inv_std3, packed, workspace, out, stream, nullptr);
}

// the accepted taps of a plan: the ends behind a dense block or a transition, below its block
static std::vector<int> densenet_taps(const spr_densenet_plan* plan) {
  std::vector<int> ends;
  for (int t = 5; t < plan->block; ++t) ends.push_back(t);
  return ends;
}

extern "C" int spr_densenet_tap_shape(const spr_densenet_plan* plan, int32_t tap_feature, int32_t in_h, int32_t in_w,
                                      int32_t* channels, int32_t* out_h, int32_t* out_w) {
  if (!plan || !channels || !out_h || !out_w || in_h < 1 || in_w < 1) { set_error("spr_densenet_tap_shape: bad argument"); return SPR_ERR_ARG; }
  const int rc = check_tap("spr_densenet_tap_shape", densenet_taps(plan), plan->block, tap_feature);
  if (rc != SPR_OK) return rc;
  int hh = ((in_h + 1) / 2 + 1) / 2, ww = ((in_w + 1) / 2 + 1) / 2, cc = 64;  // (densenet_dims over features[:tap_feature])
  for (const DOp& o : plan->ops) {
    if (o.feature >= tap_feature) break;
    if (o.kind == 2) cc = o.c_off + 32;
    if (o.kind == 3) { hh /= 2; ww /= 2; cc = o.cout; }
  }
  *channels = cc; *out_h = hh; *out_w = ww;
  return SPR_OK;
}

extern "C" int spr_densenet_forward_taps(spr_densenet_plan* plan, const uint8_t* images, int64_t n, int32_t in_h, int32_t in_w,
                                         int32_t in_channels, const float* mean3, const float* inv_std3, const void* packed,
                                         void* workspace, float* out, int32_t n_taps, const int32_t* tap_features,
                                         float* const* tap_out, spr_stream_t stream) {
  if (!plan) { set_error("spr_densenet_forward_taps: null plan"); return SPR_ERR_ARG; }
  TapSet taps;
  const int rc = check_taps("spr_densenet_forward_taps", densenet_taps(plan), plan->block, n_taps, tap_features, tap_out, n, &taps);
  if (rc != SPR_OK) return rc;
  return densenet_forward(plan, images, n, in_h, in_w, in_channels, mean3, inv_std3, packed, workspace, out, stream, nullptr, &taps);
}

extern "C" int spr_densenet_trace_layout(const spr_densenet_plan* plan, int64_t n, int32_t in_h, int32_t in_w, int64_t* records,
                                         size_t* total_bytes) {
  if (!plan || n < 0 || in_h < 32 || in_w < 32) { set_error("spr_densenet_trace_layout: bad argument"); return SPR_ERR_ARG; }
  return trace_query(densenet_trace_layout(plan, n, in_h, in_w), records, total_bytes);
}

extern "C" int spr_densenet_forward_trace(spr_densenet_plan* plan, const uint8_t* images, int64_t n, int32_t in_h, int32_t in_w,
                                          int32_t in_channels, const float* mean3, const float* inv_std3, const void* packed,
                                          void* workspace, float* out, void* trace, spr_stream_t stream) {
  if (!plan || !trace) { set_error("spr_densenet_forward_trace: null pointer"); return SPR_ERR_ARG; }
  return densenet_forward(plan, images, n, in_h, in_w, in_channels, mean3, inv_std3, packed, workspace, out, stream,
                          static_cast<unsigned char*>(trace));
}
