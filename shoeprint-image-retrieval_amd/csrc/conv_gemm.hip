// The convolution kernels the extractor backbones share (resnet.hip, effnet.hip, densenet.hip, and the first layer of the
// plain VGGs' 16-bit plans in vgg_conv.hip), their parameter packers, and one host launcher per kernel (conv_gemm.h); the
// launchers pick the template instance from the runtime kernel size / stride / compute type.
//
// Kernels (activations NHWC between layers, float32 or rounded to float16 / bfloat16; NCHW float32 out of the last one, as
// the NCC prep kernels read it):
//   stem_kernel      7x7 / stride 2 / pad 3, 3 -> 64, with ToTensor / repeat(3) / Normalize fused in front (zero padding
//                    of the NORMALISED tensor) and ReLU behind; plain FMA (K = 147, 3.6 % of the ResNet's flops).
//   stem16_kernel    the first convolution (7x7 / 2, 3x3 / 2 or 3x3 / 1) of a 16-bit plan on the 16-bit matrix cores.
//   maxpool3_kernel, maxpool3_16_kernel   3x3 / stride 2 / pad 1.
//   conv_gemm_kernel every other convolution (1x1 and 3x3, stride 1 or 2) as an implicit GEMM on the fp32 matrix cores
//                    (v_mfma_f32_16x16x4_f32, exact f32): M = images x output pixels, N = output channels, K = taps x
//                    input channels.  Workgroup = 64 pixels x 64 channels, 4 waves x (16 pixels x 64 channels); per K
//                    chunk of 16 the A tile (gathered rows of 16 contiguous channels, zero fill = padding) and the B
//                    tile (packed filter slab) are staged in LDS from registers loaded one chunk ahead.  Epilogue: bias,
//                    activation, residual add; optional squeeze-excitation factors / BatchNorm + ReLU on the operand.
//   conv_gemm16_kernel  the same GEMM view on v_mfma_f32_16x16x32 with float16 / bfloat16 operands.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <string>

#include "conv_gemm.h"

namespace spr {
namespace {

constexpr int kGM = 64, kGN = 64, kGK = 16;  // GEMM tile of a workgroup: pixels x channels x K chunk
constexpr int kGS = 20;                        // LDS row stride (floats) of a 16-float row: 16-byte aligned, 5 quads
                                               // -> the 16 lanes of an MFMA operand read hit different banks

// ---------------------------------------------------------------- parameter packing
// stem: [tap*3 + c][64]   |   GEMM convs: [cout/64][K/16][n:64][k:16], K index = tap * cin + c
__global__ void __launch_bounds__(kThreads)
rpack_kernel(const float* __restrict__ w, const float* __restrict__ b, float* __restrict__ packed, size_t w_off,
             size_t b_off, int cin, int cout, int ks, int stem) {
  const int taps = ks * ks;
  const size_t total = static_cast<size_t>(cout) * cin * taps;
  for (size_t i = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x; i < total;
       i += static_cast<size_t>(gridDim.x) * kThreads) {
    const int tap = static_cast<int>(i % taps);  // torch layout [n][c][ky][kx]
    const int c = static_cast<int>((i / taps) % cin);
    const int n = static_cast<int>(i / (static_cast<size_t>(taps) * cin));
    size_t dst;
    if (stem) {
      dst = static_cast<size_t>(tap * 3 + c) * cout + n;
    } else {
      const int k = tap * cin + c;
      const int chunks = taps * cin / kGK;
      dst = ((static_cast<size_t>(n / kGN) * chunks + k / kGK) * kGN + n % kGN) * kGK + k % kGK;
    }
    packed[w_off + dst] = w[i];
  }
  for (int i = blockIdx.x * kThreads + threadIdx.x; i < cout; i += gridDim.x * kThreads) packed[b_off + i] = b[i];
}

// ---------------------------------------------------------------- stem: 7x7 s2 p3, 3 -> 64, pre-processing + ReLU fused
// grid = (tiles of 8x8 output pixels, images); out NHWC [n][Ho][Wo][64]
__global__ void __launch_bounds__(kThreads)
stem_kernel(const uint8_t* __restrict__ images, int H, int W, int in_channels, float m0, float m1, float m2, float s0,
            float s1, float s2, const float* __restrict__ wts, const float* __restrict__ bias, float* __restrict__ out,
            int relu, int kind16) {
  // kind16 != 0 (16-bit plans): the activation is stored rounded to float16 / bfloat16 (rounding is monotonic, so the max
  // pool behind it may take its maximum over the rounded values)
  constexpr int kT = 8, kP = 2 * kT + 5;  // 21 x 21 input patch
  __shared__ float patch[kP * kP * 3];
  __shared__ float wl[147 * 64];
  const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
  const int tiles_x = ceil_div(Wo, kT);
  const int ty = static_cast<int>(blockIdx.x) / tiles_x, tx = static_cast<int>(blockIdx.x) % tiles_x;
  const int oy0 = ty * kT, ox0 = tx * kT;
  const size_t img = blockIdx.y;
  const int tid = static_cast<int>(threadIdx.x);
  const float mean[3] = {m0, m1, m2}, istd[3] = {s0, s1, s2};
  for (int i = tid; i < 147 * 64; i += kThreads) wl[i] = wts[i];
  for (int i = tid; i < kP * kP; i += kThreads) {
    const int py = i / kP, px = i % kP;
    const int y = 2 * oy0 - 3 + py, x = 2 * ox0 - 3 + px;
    const bool in = y >= 0 && y < H && x >= 0 && x < W;
    for (int c = 0; c < 3; ++c) {
      float v = 0.0f;  // zero padding of the NORMALISED tensor
      if (in) {
        const size_t pix = (img * H + y) * static_cast<size_t>(W) + x;
        const float u = static_cast<float>(in_channels == 1 ? images[pix] : images[pix * 3 + c]);
        v = (u / 255.0f - mean[c]) * istd[c];
      }
      patch[i * 3 + c] = v;
    }
  }
  __syncthreads();
  const int n = tid & 63, part = tid >> 6;  // lane = output channel; wave `part` takes output rows 2 part, 2 part + 1
  const float b = bias[n];
  float acc[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = b;
  for (int dy = 0; dy < 7; ++dy)
    for (int dx = 0; dx < 7; ++dx)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float wv = wl[((dy * 7 + dx) * 3 + c) * 64 + n];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int py = 2 * (2 * part + i / 8) + dy, px = 2 * (i % 8) + dx;
          acc[i] = fmaf(patch[(py * kP + px) * 3 + c], wv, acc[i]);
        }
      }
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int oy = oy0 + 2 * part + i / 8, ox = ox0 + i % 8;
    if (oy < Ho && ox < Wo) {
      const float v = relu ? fmaxf(acc[i], 0.0f) : acc[i];
      const size_t at = ((img * Ho + oy) * static_cast<size_t>(Wo) + ox) * 64 + n;
      if (kind16 == 0) out[at] = v;
      else reinterpret_cast<uint16_t*>(out)[at] = kind16 == SPR_F16 ? round_f16(v) : round_bf16(v);
    }
  }
}

// ---------------------------------------------------------------- 3x3 / stride 2 / pad 1 max pool, NHWC
__global__ void __launch_bounds__(kThreads)
maxpool3_kernel(const float* __restrict__ in, int H, int W, int C, float* __restrict__ out, size_t total, int ldo) {
  const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
  for (size_t i = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x; i < total;
       i += static_cast<size_t>(gridDim.x) * kThreads) {
    const int c = static_cast<int>(i % C);
    size_t p = i / C;
    const int ox = static_cast<int>(p % Wo); p /= Wo;
    const int oy = static_cast<int>(p % Ho);
    const size_t img = p / Ho;
    float m = -3.402823466e38f;  // (padding never wins: every window holds at least one real pixel)
    for (int dy = -1; dy <= 1; ++dy)
      for (int dx = -1; dx <= 1; ++dx) {
        const int y = 2 * oy + dy, x = 2 * ox + dx;
        if (y >= 0 && y < H && x >= 0 && x < W) m = fmaxf(m, in[((img * H + y) * static_cast<size_t>(W) + x) * C + c]);
      }
    out[(i / C) * ldo + c] = m;  // ldo: channel stride of the output tensor (>= C)
  }
}

// ---------------------------------------------------------------- implicit-GEMM convolution on fp32 MFMA
// grid = (ceil(M / 64), cout / 64).  in NHWC [n][H][W][cin]; out NHWC [n][Ho][Wo][cout] (or NCHW); res NHWC like out.
template <int KS, int STRIDE>
__global__ void __launch_bounds__(kThreads, 2)
conv_gemm_kernel(const float* __restrict__ in, int n_img, int H, int W, int cin, int cout, const float* __restrict__ wts,
                 const float* __restrict__ bias, const float* __restrict__ res, int relu, int nchw,
                 float* __restrict__ out, const float* __restrict__ in_scale, int cout_real, int lda, int ldc, int c_off,
                 const float* __restrict__ pre_s, const float* __restrict__ pre_t, float* __restrict__ tap, int tap_real) {
  // tap: null, or (with an NHWC `out`) where the first tap_real channels of the same result also go as float32 NCHW
  // [n][tap_real][Ho][Wo] - a feature tap, the values an NCHW `out` of a plan that ends here would hold
  // lda / ldc: channel strides of the input / NHWC output tensors (>= cin / cout: a convolution may read a prefix of a wider
  // tensor and write a channel range [c_off, c_off + cout_real) of one - DenseNet's concatenation); pre_s / pre_t: per input
  // channel, max(x * s + t, 0) applied while the operand is loaded (BatchNorm + ReLU in FRONT of a 1x1 convolution), or null
  // relu: activation code (0 none, 1 ReLU, 2 SiLU); in_scale: [image][cin] factors on the input (squeeze-excitation), or null;
  // cout_real: channels of an NCHW result when cout is padded (0: all of them)
  __shared__ __attribute__((aligned(16))) float A[kGM * kGS];
  __shared__ __attribute__((aligned(16))) float B[kGN * kGS];
  constexpr int PAD = KS / 2;
  const int Ho = (H + 2 * PAD - KS) / STRIDE + 1, Wo = (W + 2 * PAD - KS) / STRIDE + 1;
  const long long M = static_cast<long long>(n_img) * Ho * Wo;
  const int tid = static_cast<int>(threadIdx.x);
  const int wave = tid >> 6, lane = tid & 63;
  const int p = lane & 15, q = lane >> 4;  // MFMA lane coordinates: row/col index, k index
  const int cb = static_cast<int>(blockIdx.y);
  const long long m0 = static_cast<long long>(blockIdx.x) * kGM;
  const int cchunks = cin / kGK, chunks = KS * KS * cchunks;

  // this thread stages quarter `sq` (4 floats) of row `sr` of both tiles
  const int sr = tid >> 2, sq = tid & 3;
  const long long pm = m0 + sr;  // pixel of the A row
  const bool pm_ok = pm < M;
  int py = 0, px = 0;
  size_t pimg = 0;
  if (pm_ok) {
    px = static_cast<int>(pm % Wo);
    py = static_cast<int>((pm / Wo) % Ho);
    pimg = static_cast<size_t>(pm / (static_cast<long long>(Wo) * Ho));
  }
  const float* wbase = wts + static_cast<size_t>(cb) * chunks * (kGN * kGK) + sr * kGK + sq * 4;

  f32x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};

  float4 ra, rb;
  auto request = [&](int ch) {
    const int tap = ch / cchunks, cc = ch - tap * cchunks;
    const int dy = tap / KS, dx = tap - dy * KS;
    const int y = py * STRIDE + dy - PAD, x = px * STRIDE + dx - PAD;
    ra = make_float4(0.f, 0.f, 0.f, 0.f);
    if (pm_ok && y >= 0 && y < H && x >= 0 && x < W)
      ra = *reinterpret_cast<const float4*>(in + ((pimg * H + y) * static_cast<size_t>(W) + x) * lda + cc * kGK + sq * 4);
    if (pre_s) {
      const float4 ps = *reinterpret_cast<const float4*>(pre_s + cc * kGK + sq * 4);
      const float4 pt = *reinterpret_cast<const float4*>(pre_t + cc * kGK + sq * 4);
      ra.x = fmaxf(fmaf(ra.x, ps.x, pt.x), 0.f); ra.y = fmaxf(fmaf(ra.y, ps.y, pt.y), 0.f);
      ra.z = fmaxf(fmaf(ra.z, ps.z, pt.z), 0.f); ra.w = fmaxf(fmaf(ra.w, ps.w, pt.w), 0.f);
    }
    if (in_scale) {
      const float4 sc = *reinterpret_cast<const float4*>(in_scale + pimg * cin + cc * kGK + sq * 4);
      ra.x *= sc.x; ra.y *= sc.y; ra.z *= sc.z; ra.w *= sc.w;
    }
    rb = *reinterpret_cast<const float4*>(wbase + static_cast<size_t>(ch) * (kGN * kGK));
  };
  request(0);
  for (int ch = 0; ch < chunks; ++ch) {
    __syncthreads();  // the previous chunk's fragments are consumed
    *reinterpret_cast<float4*>(A + sr * kGS + sq * 4) = ra;
    *reinterpret_cast<float4*>(B + sr * kGS + sq * 4) = rb;
    __syncthreads();
    if (ch + 1 < chunks) request(ch + 1);
    // the k index of MFMA step j is {4 q + j}: any partition of the 16 works as long as A and B agree
    const float4 a = *reinterpret_cast<const float4*>(A + (wave * 16 + p) * kGS + q * 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float4 b = *reinterpret_cast<const float4*>(B + (j * 16 + p) * kGS + q * 4);
      acc[j] = mfma_f32_16x16x4(a.x, b.x, acc[j]);
      acc[j] = mfma_f32_16x16x4(a.y, b.y, acc[j]);
      acc[j] = mfma_f32_16x16x4(a.z, b.z, acc[j]);
      acc[j] = mfma_f32_16x16x4(a.w, b.w, acc[j]);
    }
  }
  // ---- epilogue: lane (q, p) owns pixels m0 + 16 wave + 4 q + r (r = 0..3), channel cb*64 + 16 j + p
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const long long m = m0 + wave * 16 + 4 * q + r;
    if (m >= M) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int ch = cb * kGN + j * 16 + p;
      float v = acc[j][r] + bias[ch];
      if (relu == 2) v = v / (1.0f + expf(-v));  // SiLU, in FRONT of the residual sum (EfficientNet blocks)
      if (res) v += res[static_cast<size_t>(m) * cout + ch];
      if (relu == 1) v = fmaxf(v, 0.0f);         // ReLU, behind it (ResNet bottlenecks)
      if (nchw) {
        const int creal = cout_real ? cout_real : cout;
        if (ch >= creal) continue;
        const int ox = static_cast<int>(m % Wo), oy = static_cast<int>((m / Wo) % Ho);
        const size_t img = static_cast<size_t>(m / (static_cast<long long>(Wo) * Ho));
        out[((img * creal + ch) * Ho + oy) * static_cast<size_t>(Wo) + ox] = v;
      } else if (!cout_real || ch < cout_real) {
        out[static_cast<size_t>(m) * ldc + c_off + ch] = v;
      }
      if (tap && ch < tap_real) {
        const int ox = static_cast<int>(m % Wo), oy = static_cast<int>((m / Wo) % Ho);
        const size_t img = static_cast<size_t>(m / (static_cast<long long>(Wo) * Ho));
        tap[((img * tap_real + ch) * Ho + oy) * static_cast<size_t>(Wo) + ox] = v;
      }
    }
  }
}

// ---------------------------------------------------------------- implicit-GEMM convolution on the 16-bit matrix cores
// spr_resnet_plan_create_ex(SPR_F16 | SPR_BF16): the same GEMM view with float16 / bfloat16 operands and f32 accumulation
// (v_mfma_f32_16x16x32: K = 32 per instruction).  The matrix work per byte staged is 16 x shorter than on the f32 cores, so
// the tile is larger: workgroup = 128 pixels x 64 channels x a K chunk of 64 (two MFMA k-steps), 4 waves x (32 pixels x 64
// channels) = 16 MFMAs per wave and chunk; the A tile (128 gathered rows of 64 contiguous channels = 128 bytes each) and the
// B tile (64 filter rows) are loaded into registers one chunk ahead and written to LDS behind the barrier.  LDS rows are 128
// bytes = eight 16-byte slots; slot s of row r sits at s ^ ((r >> 1) & 7), so the 16 lanes x 4 k-groups of an operand read
// fall into different banks.  Activations between layers: NHWC, rounded to the 16-bit type; the residual operand is such a
// stored activation; bias / residual sum / ReLU in f32; the last layer writes float32 NCHW.
constexpr int kHM = 128, kHN = 64, kHK = 64;
constexpr int kHRowDw = 32;  // dwords per LDS row (128 bytes)

// GEMM convs of a 16-bit plan: [cout/64][K/64][n:64][k:64] float16 / bfloat16, K index = tap * cin + c; bias f32
template <int KIND>
__global__ void __launch_bounds__(kThreads)
rpack16_kernel(const float* __restrict__ w, const float* __restrict__ b, float* __restrict__ packed, size_t w_off,
               size_t b_off, int cin, int cout, int ks) {
  uint16_t* dst16 = reinterpret_cast<uint16_t*>(packed + w_off);
  const int taps = ks * ks;
  const size_t total = static_cast<size_t>(cout) * cin * taps;
  const int chunks = taps * cin / kHK;
  for (size_t i = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x; i < total;
       i += static_cast<size_t>(gridDim.x) * kThreads) {
    const int tap = static_cast<int>(i % taps);
    const int c = static_cast<int>((i / taps) % cin);
    const int n = static_cast<int>(i / (static_cast<size_t>(taps) * cin));
    const int k = tap * cin + c;
    dst16[((static_cast<size_t>(n / kHN) * chunks + k / kHK) * kHN + n % kHN) * kHK + k % kHK] = round16<KIND>(w[i]);
  }
  for (int i = blockIdx.x * kThreads + threadIdx.x; i < cout; i += gridDim.x * kThreads) packed[b_off + i] = b[i];
}

// 3x3 / stride 2 / pad 1 max pool of the stem's (rounded, post-ReLU: non-negative) 16-bit NHWC output into the 16-bit NHWC
// tensor layer1 reads (channel stride ldo >= C, a multiple of 8: DenseNet's first block tensor is wider than the pool):
// eight channels (16 bytes) per work-item; non-negative float16 / bfloat16 values order like their bit patterns, so the
// maximum is taken on the 16-bit integers
__global__ void __launch_bounds__(kThreads)
maxpool3_16_kernel(const uint16_t* __restrict__ in, int H, int W, int C, uint16_t* __restrict__ out, size_t total8, int ldo) {
  const int Ho = (H + 1) / 2, Wo = (W + 1) / 2, c8 = C / 8;
  for (size_t i = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x; i < total8;
       i += static_cast<size_t>(gridDim.x) * kThreads) {
    const int c = static_cast<int>(i % c8) * 8;
    size_t p = i / c8;
    const int ox = static_cast<int>(p % Wo); p /= Wo;
    const int oy = static_cast<int>(p % Ho);
    const size_t img = p / Ho;
    uint32_t m[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int dy = -1; dy <= 1; ++dy)
      for (int dx = -1; dx <= 1; ++dx) {
        const int y = 2 * oy + dy, x = 2 * ox + dx;
        if (y < 0 || y >= H || x < 0 || x >= W) continue;
        const u32x4 v = *reinterpret_cast<const u32x4*>(in + ((img * H + y) * static_cast<size_t>(W) + x) * C + c);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const uint32_t h = (v[e >> 1] >> (16 * (e & 1))) & 0xffffu;
          m[e] = h > m[e] ? h : m[e];
        }
      }
    u32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = m[2 * e] | (m[2 * e + 1] << 16);
    *reinterpret_cast<u32x4*>(out + (i / c8) * ldo + c) = o;
  }
}

// ---------------------------------------------------------------- the stem on the 16-bit matrix cores (16-bit plans)
// The plain FMA stem_kernel runs at half of the (unpacked) f32 vector peak and is LDS-bound on broadcast reads: 0.5 ms per 32
// images, a fifth of a 16-bit forward pass.  Here the 7x7 / stride 2 convolution is a GEMM of 128 output pixels (8 x 16) x 64
// channels x K = 147 taps-and-planes padded to 160 = five v_mfma_f32_16x16x32 k-steps: the normalised input patch (ToTensor,
// repeat(3), Normalize; zero outside the image) is rounded to the 16-bit type into LDS, every work-item gathers ten 16-byte
// pieces (8 consecutive k each) of the im2col tile from it through an offset table, and the operand tiles lie K-major
// ([16-byte slot][row]) so that the sixteen rows x four k-groups of a fragment read fall into different banks as they are.
// Weights: [k / 8][n: 64][8] 16-bit, zero for k >= 147 (rstem16_pack_kernel).  Output: NHWC 16-bit, ReLU applied.
// The same kernel with KS = 3, STRIDE = 1 (K = 27 padded to 32: one k-step) is the first convolution of the plain VGGs in their
// 16-bit plans (vgg_conv.hip calls launch_stem16 with them).
constexpr int kSTH = 8, kSTW = 16;  // output pixels per workgroup
template <int KS, int STRIDE>
struct First16 {
  static constexpr int TAPS = KS * KS, KREAL = TAPS * 3, K = (KREAL + 31) / 32 * 32, SLOTS = K / 8;
  static constexpr int PH = STRIDE * kSTH + KS - STRIDE, PW = STRIDE * kSTW + KS - STRIDE, PAD = KS / 2;
};

template <int KIND, int KS>
__global__ void __launch_bounds__(kThreads)
rstem16_pack_kernel(const float* __restrict__ w, const float* __restrict__ b, float* __restrict__ packed, size_t w_off,
                    size_t b_off) {
  using F = First16<KS, 1>;
  uint16_t* dst = reinterpret_cast<uint16_t*>(packed + w_off);
  for (int i = blockIdx.x * kThreads + threadIdx.x; i < F::K * 64; i += gridDim.x * kThreads) {
    const int k = i / 64, n = i % 64;  // k = tap * 3 + c
    float v = 0.0f;
    if (k < F::KREAL) v = w[(static_cast<size_t>(n) * 3 + k % 3) * F::TAPS + k / 3];  // torch layout [n][c][ky][kx]
    dst[(static_cast<size_t>(k / 8) * 64 + n) * 8 + k % 8] = round16<KIND>(v);
  }
  for (int i = blockIdx.x * kThreads + threadIdx.x; i < 64; i += gridDim.x * kThreads) packed[b_off + i] = b[i];
}

// grid = (tiles of 8 x 16 output pixels, images)
template <int KIND, int KS, int STRIDE>
__global__ void __launch_bounds__(kThreads, 2)
stem16_kernel(const uint8_t* __restrict__ images, int H, int W, int in_channels, float m0, float m1, float m2, float s0,
              float s1, float s2, const uint16_t* __restrict__ wts, const float* __restrict__ bias, uint16_t* __restrict__ out,
              int relu) {
  using F = First16<KS, STRIDE>;
  constexpr int kSK = F::K, kSSlots = F::SLOTS, kSPH = F::PH, kSPW = F::PW;
  constexpr int kHT = 68;
  constexpr int kPatchElems = kSPH * kSPW * 3;                  // stem: 21 x 37 x 3
  constexpr int kPatchBytes = (kPatchElems * 2 + 2 + 15) / 16 * 16;  // + one zero element the padded k read
  constexpr int kABytes = kSSlots * 128 * 16 > 128 * kHT * 4 ? kSSlots * 128 * 16 : 128 * kHT * 4;  // (or the f32 output tile)
  constexpr int kBBytes = kSSlots * 64 * 16;
  __shared__ __attribute__((aligned(16))) unsigned char lds[kABytes + kBBytes + kPatchBytes + kSK * 2];
  uint32_t* A = reinterpret_cast<uint32_t*>(lds);
  uint32_t* B = reinterpret_cast<uint32_t*>(lds + kABytes);
  uint16_t* patch = reinterpret_cast<uint16_t*>(lds + kABytes + kBBytes);
  uint16_t* koff = reinterpret_cast<uint16_t*>(lds + kABytes + kBBytes + kPatchBytes);
  const int Ho = (H + 2 * F::PAD - KS) / STRIDE + 1, Wo = (W + 2 * F::PAD - KS) / STRIDE + 1;
  const int tiles_x = ceil_div(Wo, kSTW);
  const int ty = static_cast<int>(blockIdx.x) / tiles_x, tx = static_cast<int>(blockIdx.x) % tiles_x;
  const int oy0 = ty * kSTH, ox0 = tx * kSTW;
  const size_t img = blockIdx.y;
  const int tid = static_cast<int>(threadIdx.x);
  const int wave = tid >> 6, lane = tid & 63, p = lane & 15, q = lane >> 4;
  const float mean[3] = {m0, m1, m2}, istd[3] = {s0, s1, s2};
  // the weights of this layer (20 KB, L2-resident) and the offset table: k -> element of the patch, relative to the pixel's
  // window origin; the padded k point at the zero element behind the patch
  for (int i = tid; i < kBBytes / 16; i += kThreads) reinterpret_cast<float4*>(B)[i] = reinterpret_cast<const float4*>(wts)[i];
  if (tid < kSK) {
    const int tap = tid / 3, c = tid % 3, dy = tap / KS, dx = tap % KS;
    koff[tid] = tid < F::KREAL ? static_cast<uint16_t>((dy * kSPW + dx) * 3 + c) : static_cast<uint16_t>(0xffff);
  }
  for (int i = tid; i < kSPH * kSPW; i += kThreads) {
    const int py = i / kSPW, px = i % kSPW;
    const int y = STRIDE * oy0 - F::PAD + py, x = STRIDE * ox0 - F::PAD + px;
    const bool in = y >= 0 && y < H && x >= 0 && x < W;
    for (int c = 0; c < 3; ++c) {
      float v = 0.0f;  // zero padding of the NORMALISED tensor
      if (in) {
        const size_t pix = (img * H + y) * static_cast<size_t>(W) + x;
        const float u = static_cast<float>(in_channels == 1 ? images[pix] : images[pix * 3 + c]);
        v = (u / 255.0f - mean[c]) * istd[c];
      }
      patch[i * 3 + c] = round16<KIND>(v);
    }
  }
  if (tid == 0) patch[kPatchElems] = 0;
  __syncthreads();
  {  // im2col: row = output pixel (8 x 16, row-major), ten 16-byte pieces per work-item
    const int row = tid & 127, half = tid >> 7;
    const int base = ((row >> 4) * STRIDE * kSPW + (row & 15) * STRIDE) * 3;
#pragma unroll
    for (int j = 0; j < kSSlots / 2; ++j) {
      const int sl = half * (kSSlots / 2) + j;
      const u32x4 ko = *reinterpret_cast<const u32x4*>(koff + 8 * sl);
      u32x4 v;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const unsigned k0 = ko[e] & 0xffffu, k1 = ko[e] >> 16;
        const unsigned a0 = patch[k0 == 0xffffu ? kPatchElems : base + static_cast<int>(k0)];
        const unsigned a1 = patch[k1 == 0xffffu ? kPatchElems : base + static_cast<int>(k1)];
        v[e] = a0 | (a1 << 16);
      }
      *reinterpret_cast<u32x4*>(A + (sl * 128 + row) * 4) = v;
    }
  }
  __syncthreads();
  f32x4 acc[2][4];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < kSK / 32; ++ks) {
    u32x4 a[2], b[4];
#pragma unroll
    for (int i = 0; i < 2; ++i) a[i] = *reinterpret_cast<const u32x4*>(A + ((ks * 4 + q) * 128 + wave * 32 + i * 16 + p) * 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) b[j] = *reinterpret_cast<const u32x4*>(B + ((ks * 4 + q) * 64 + j * 16 + p) * 4);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[i][j] = KIND == SPR_F16 ? mfma_f16_16x16x32(a[i], b[j], acc[i][j]) : mfma_bf16_16x16x32(a[i], b[j], acc[i][j]);
  }
  __syncthreads();  // the A tile is consumed: the f32 output tile takes its place
  float* T = reinterpret_cast<float*>(lds);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float bv = bias[j * 16 + p];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) T[(wave * 32 + i * 16 + 4 * q + r) * kHT + j * 16 + p] = acc[i][j][r] + bv;
  }
  __syncthreads();
  const int sr = tid >> 3, ss = tid & 7;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int row = sr + 32 * k;
    const int oy = oy0 + (row >> 4), ox = ox0 + (row & 15);
    if (oy >= Ho || ox >= Wo) continue;
    const float4 lo = *reinterpret_cast<const float4*>(T + row * kHT + ss * 8);
    const float4 hi = *reinterpret_cast<const float4*>(T + row * kHT + ss * 8 + 4);
    const float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    u32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      // relu: activation code (0 none, 1 ReLU, 2 SiLU)
      const float a0 = relu == 1 ? fmaxf(v[2 * e], 0.0f) : relu == 2 ? v[2 * e] / (1.0f + expf(-v[2 * e])) : v[2 * e];
      const float a1 = relu == 1 ? fmaxf(v[2 * e + 1], 0.0f) : relu == 2 ? v[2 * e + 1] / (1.0f + expf(-v[2 * e + 1])) : v[2 * e + 1];
      o[e] = static_cast<uint32_t>(round16<KIND>(a0)) | (static_cast<uint32_t>(round16<KIND>(a1)) << 16);
    }
    *reinterpret_cast<u32x4*>(out + ((img * Ho + oy) * static_cast<size_t>(Wo) + ox) * 64 + ss * 8) = o;
  }
}

// grid = (ceil(M / 128), cout / BN).  in / res / out: NHWC 16-bit with cin / cout channels; out32: float32 NCHW (last layer).
// BN = 64: four waves x (32 pixels x 64 channels); BN = 128: 2 x 2 waves x (64 pixels x 64 channels) - twice the matrix
// work per byte staged (these GEMMs run against the L2 -> CU bandwidth, not against the matrix cores: a 128 x 64 x 64 chunk
// is 43 flop per staged byte, a 128 x 128 x 64 one 64).
template <int KS, int STRIDE, int KIND, int BN>
__global__ void __launch_bounds__(kThreads, BN == 128 ? 2 : 3)
conv_gemm16_kernel(const uint16_t* __restrict__ in, int n_img, int H, int W, int cin, int cout,
                   const uint16_t* __restrict__ wts, const float* __restrict__ bias, const uint16_t* __restrict__ res,
                   int relu, uint16_t* __restrict__ out, float* __restrict__ out32, const float* __restrict__ in_scale,
                   int cout_real, float* __restrict__ tap) {
  // tap: null, or (with out32 null) where the result also goes as float32 NCHW [n][cout_real][Ho][Wo], exactly as out32
  // would hold it - a feature tap: the unrounded values whose round16 the NHWC store writes
  // relu: activation code (0 none, 1 ReLU behind the residual sum: ResNet bottlenecks, 2 SiLU in FRONT of it: EfficientNet
  // blocks); in_scale: [image][cin] f32 factors on the input (squeeze-excitation), applied while the operand is staged and
  // rounded again, or null; cout_real: channels of a float32 NCHW result when cout is padded (0: all of them)
  // one LDS array: the A and B operand tiles in the main loop, the f32 output tile [128][kHT] (64 channels at a time) in the
  // epilogue
  constexpr int kHT = 68;  // row stride (floats) of the output tile: 16-byte aligned, rows 4 apart half a bank row apart
  constexpr int kLdsDw = kHM * kHT > (kHM + BN) * kHRowDw ? kHM * kHT : (kHM + BN) * kHRowDw;
  __shared__ __attribute__((aligned(16))) uint32_t lds16[kLdsDw];
  uint32_t* A = lds16;
  uint32_t* B = lds16 + kHM * kHRowDw;
  constexpr int PAD = KS / 2;
  constexpr int MI = BN == 128 ? 4 : 2;  // 16-pixel blocks per wave
  constexpr int BK = BN / 32;            // 16-byte pieces of the B tile per work-item
  const int Ho = (H + 2 * PAD - KS) / STRIDE + 1, Wo = (W + 2 * PAD - KS) / STRIDE + 1;
  const long long M = static_cast<long long>(n_img) * Ho * Wo;
  const int tid = static_cast<int>(threadIdx.x);
  const int wave = tid >> 6, lane = tid & 63;
  const int p = lane & 15, q = lane >> 4;
  const int cb = static_cast<int>(blockIdx.y);
  const long long m0 = static_cast<long long>(blockIdx.x) * kHM;
  const int cchunks = cin / kHK, chunks = KS * KS * cchunks;
  const int wm = BN == 128 ? (wave >> 1) * 64 : wave * 32;  // first pixel row / first channel of this wave's part of the tile
  const int wn = BN == 128 ? (wave & 1) * 64 : 0;

  // staging role: 16-byte slot `ss` of rows sr + 32 k (A: k = 0..3, B: k = 0 .. BK - 1)
  const int sr = tid >> 3, ss = tid & 7;
  int ay[4], ax[4], aimg[4];
  long long abase[4];  // element offset of pixel (img, 0, 0); negative marks a row beyond M
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const long long pm = m0 + sr + 32 * k;
    if (pm < M) {
      const int px = static_cast<int>(pm % Wo), py = static_cast<int>((pm / Wo) % Ho);
      const long long pimg = pm / (static_cast<long long>(Wo) * Ho);
      ay[k] = py * STRIDE - PAD; ax[k] = px * STRIDE - PAD;
      abase[k] = pimg * H * static_cast<long long>(W) * cin;
      aimg[k] = static_cast<int>(pimg);
    } else {
      ay[k] = ax[k] = 0; abase[k] = -1; aimg[k] = 0;
    }
  }
  // packed weights: [cout / 64][chunk][n: 64][k: 64]; B tile row r belongs to 64-channel block cb * (BN / 64) + r / 64
  const uint16_t* wbase = wts + ss * 8;
  const size_t wblock = static_cast<size_t>(chunks) * (kHN * kHK);

  f32x4 acc[MI][4];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  u32x4 ra[4], rb[BK];  // (native vectors: arrays of HIP's float4 struct stayed in scratch memory and made the prefetch synchronous)
  auto request = [&](int ch) {
    const int tap = ch / cchunks, cc = ch - tap * cchunks;
    const int dy = tap / KS, dx = tap - dy * KS;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int y = ay[k] + dy, x = ax[k] + dx;
      ra[k] = u32x4{0u, 0u, 0u, 0u};
      if (abase[k] >= 0 && y >= 0 && y < H && x >= 0 && x < W) {
        ra[k] = *reinterpret_cast<const u32x4*>(in + abase[k] + (static_cast<long long>(y) * W + x) * cin + cc * kHK + ss * 8);
        if (in_scale) {  // x * factor, rounded to the operand type again
          const float* sc = in_scale + static_cast<size_t>(aimg[k]) * cin + cc * kHK + ss * 8;
          const float4 s0 = *reinterpret_cast<const float4*>(sc), s1 = *reinterpret_cast<const float4*>(sc + 4);
          const float f[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
          u32x4 r;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float lo = value16<KIND>(static_cast<uint16_t>(ra[k][e] & 0xffffu)) * f[2 * e];
            const float hi = value16<KIND>(static_cast<uint16_t>(ra[k][e] >> 16)) * f[2 * e + 1];
            r[e] = static_cast<uint32_t>(round16<KIND>(lo)) | (static_cast<uint32_t>(round16<KIND>(hi)) << 16);
          }
          ra[k] = r;
        }
      }
    }
#pragma unroll
    for (int k = 0; k < BK; ++k) {
      const int r = sr + 32 * k;
      rb[k] = *reinterpret_cast<const u32x4*>(wbase + (static_cast<size_t>(cb) * (BN / 64) + r / 64) * wblock +
                                               (static_cast<size_t>(ch) * kHN + r % 64) * kHK);
    }
  };
  auto slot = [](int row, int s) { return (s ^ ((row >> 1) & 7)) << 2; };  // dword offset of 16-byte slot s inside row `row`
  request(0);
  for (int ch = 0; ch < chunks; ++ch) {
    __syncthreads();  // the previous chunk's fragments are consumed
#pragma unroll
    for (int k = 0; k < 4; ++k) *reinterpret_cast<u32x4*>(A + (sr + 32 * k) * kHRowDw + slot(sr + 32 * k, ss)) = ra[k];
#pragma unroll
    for (int k = 0; k < BK; ++k) *reinterpret_cast<u32x4*>(B + (sr + 32 * k) * kHRowDw + slot(sr + 32 * k, ss)) = rb[k];
    __syncthreads();
    if (ch + 1 < chunks) request(ch + 1);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      u32x4 a[MI], b[4];
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        const int row = wm + i * 16 + p;
        a[i] = *reinterpret_cast<const u32x4*>(A + row * kHRowDw + slot(row, ks * 4 + q));
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int row = wn + j * 16 + p;
        b[j] = *reinterpret_cast<const u32x4*>(B + row * kHRowDw + slot(row, ks * 4 + q));
      }
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = KIND == SPR_F16 ? mfma_f16_16x16x32(a[i], b[j], acc[i][j]) : mfma_bf16_16x16x32(a[i], b[j], acc[i][j]);
    }
  }
  // ---- epilogue.  Lane (q, p) owns pixels wm + 16 i + 4 q + r, channels wn + 16 j + p of the tile: scattered 2-byte stores
  // from there would touch 32-byte pieces of 4 rows per instruction.  The accumulators (+ bias) go through LDS as an f32 tile
  // of 64 channels at a time instead, and leave in the layout of the destination: NHWC 16-bit rows as 16-byte pieces of 8
  // channels (the residual operand is read the same way), NCHW float32 as runs of consecutive pixels of one channel.
  float* T = reinterpret_cast<float*>(lds16);
#pragma unroll
  for (int h = 0; h < BN / 64; ++h) {
    __syncthreads();  // the operand tiles (or the previous half of the output tile) are consumed
    const int cbase = cb * BN + h * 64;  // first channel of this half
    if (wn == h * 64) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float bv = bias[cbase + j * 16 + p];
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
          for (int r = 0; r < 4; ++r) T[(wm + i * 16 + 4 * q + r) * kHT + j * 16 + p] = acc[i][j][r] + bv;
      }
    }
    __syncthreads();
    // the float32 NCHW store of this half of the tile: the output of the last layer, or a feature tap beside the NHWC store
    auto store_nchw = [&](float* __restrict__ dst) {
      // thread = (pixel row of the tile, half of the channels): for one channel, 128 consecutive work-items store 128
      // consecutive pixels of its plane
      const int row = tid & 127, c0 = tid >> 7;
      const long long m = m0 + row;
      if (m < M) {
        const size_t plane = static_cast<size_t>(Ho) * Wo;
        const size_t img = static_cast<size_t>(m / static_cast<long long>(plane));
        const size_t pix = static_cast<size_t>(m - static_cast<long long>(img) * plane);
        const int creal = cout_real ? cout_real : cout;
#pragma unroll 4
        for (int k = 0; k < 32; ++k) {
          const int c = 2 * k + c0, chn = cbase + c;
          if (chn >= creal) continue;
          float v = T[row * kHT + c];
          if (relu == 2) v = v / (1.0f + expf(-v));
          if (res) v += value16<KIND>(res[static_cast<size_t>(m) * cout + chn]);
          if (relu == 1) v = fmaxf(v, 0.0f);
          dst[(img * creal + chn) * plane + pix] = v;
        }
      }
    };
    if (out32) {
      store_nchw(out32);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int row = sr + 32 * k;  // (the staging role again: 16-byte piece ss of rows sr + 32 k)
        const long long m = m0 + row;
        if (m >= M) continue;
        const float4 lo = *reinterpret_cast<const float4*>(T + row * kHT + ss * 8);
        const float4 hi = *reinterpret_cast<const float4*>(T + row * kHT + ss * 8 + 4);
        float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        const size_t at = static_cast<size_t>(m) * cout + cbase + ss * 8;
        if (relu == 2) {
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = v[e] / (1.0f + expf(-v[e]));
        }
        if (res) {
          const u32x4 rv = *reinterpret_cast<const u32x4*>(res + at);
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] += value16<KIND>(static_cast<uint16_t>(rv[e >> 1] >> (16 * (e & 1))));
        }
        u32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float a0 = relu == 1 ? fmaxf(v[2 * e], 0.0f) : v[2 * e], a1 = relu == 1 ? fmaxf(v[2 * e + 1], 0.0f) : v[2 * e + 1];
          o[e] = static_cast<uint32_t>(round16<KIND>(a0)) | (static_cast<uint32_t>(round16<KIND>(a1)) << 16);
        }
        *reinterpret_cast<u32x4*>(out + at) = o;
      }
      if (tap) store_nchw(tap);  // (the tile stays as it is until the next half's barrier)
    }
  }
}

}  // namespace

// ================================================================ host launchers (conv_gemm.h)
// Each picks its kernel instance as a function pointer (all instances of a kernel share one signature); a combination that
// is not instantiated is an error, never another instance.
namespace {
int out_size(int in, int ks, int stride) { return (in + 2 * (ks / 2) - ks) / stride + 1; }  // pad = ks / 2
}  // namespace

int pack_conv_gemm(const float* w, const float* b, float* packed, size_t w_off, size_t b_off, int cin, int cout, int ks,
                   int stem, hipStream_t s) {
  hipLaunchKernelGGL(rpack_kernel, dim3(256), dim3(kThreads), 0, s, w, b, packed, w_off, b_off, cin, cout, ks, stem);
  return check_launch("rpack_kernel");
}

int pack_conv_gemm16(int kind, const float* w, const float* b, float* packed, size_t w_off, size_t b_off, int cin, int cout,
                     int ks, hipStream_t s) {
  auto kernel = kind == SPR_F16 ? rpack16_kernel<SPR_F16> : rpack16_kernel<SPR_BF16>;
  hipLaunchKernelGGL(kernel, dim3(256), dim3(kThreads), 0, s, w, b, packed, w_off, b_off, cin, cout, ks);
  return check_launch("rpack16_kernel");
}

int pack_stem16(int kind, int ks, const float* w, const float* b, float* packed, size_t w_off, size_t b_off, hipStream_t s) {
  if (ks != 7 && ks != 3) { set_error("pack_stem16: no %d x %d instance", ks, ks); return SPR_ERR_UNSUPPORTED; }
  const bool f16 = kind == SPR_F16;
  auto kernel = ks == 7 ? (f16 ? rstem16_pack_kernel<SPR_F16, 7> : rstem16_pack_kernel<SPR_BF16, 7>)
                        : (f16 ? rstem16_pack_kernel<SPR_F16, 3> : rstem16_pack_kernel<SPR_BF16, 3>);
  const int k_padded = ks == 7 ? First16<7, 1>::K : First16<3, 1>::K;
  hipLaunchKernelGGL(kernel, dim3(k_padded * 64 / kThreads), dim3(kThreads), 0, s, w, b, packed, w_off, b_off);
  return check_launch("rstem16_pack_kernel");
}

int launch_stem(const uint8_t* images, int64_t n, int in_h, int in_w, int in_channels, const float* mean3,
                const float* inv_std3, const float* wts, const float* bias, float* out, int relu, int kind16, hipStream_t s) {
  const unsigned tiles = static_cast<unsigned>(ceil_div(out_size(in_h, 7, 2), 8) * ceil_div(out_size(in_w, 7, 2), 8));
  hipLaunchKernelGGL(stem_kernel, dim3(tiles, static_cast<unsigned>(n)), dim3(kThreads), 0, s, images, in_h, in_w, in_channels,
                     mean3[0], mean3[1], mean3[2], inv_std3[0], inv_std3[1], inv_std3[2], wts, bias, out, relu, kind16);
  return check_launch("stem_kernel");
}

int launch_stem16(int kind, int ks, int stride, const uint8_t* images, int64_t n, int in_h, int in_w, int in_channels,
                  const float* mean3, const float* inv_std3, const uint16_t* w16, const float* bias, int act, uint16_t* out,
                  hipStream_t s) {
  const bool f16 = kind == SPR_F16;
  auto kernel = ks == 7 && stride == 2   ? (f16 ? stem16_kernel<SPR_F16, 7, 2> : stem16_kernel<SPR_BF16, 7, 2>)
                : ks == 3 && stride == 2 ? (f16 ? stem16_kernel<SPR_F16, 3, 2> : stem16_kernel<SPR_BF16, 3, 2>)
                : ks == 3 && stride == 1 ? (f16 ? stem16_kernel<SPR_F16, 3, 1> : stem16_kernel<SPR_BF16, 3, 1>)
                                         : nullptr;
  if (!kernel) { set_error("launch_stem16: no %d x %d / stride %d instance", ks, ks, stride); return SPR_ERR_UNSUPPORTED; }
  const int tiles = ceil_div(out_size(in_h, ks, stride), kSTH) * ceil_div(out_size(in_w, ks, stride), kSTW);
  hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(tiles), static_cast<unsigned>(n)), dim3(kThreads), 0, s, images, in_h,
                     in_w, in_channels, mean3[0], mean3[1], mean3[2], inv_std3[0], inv_std3[1], inv_std3[2], w16, bias, out, act);
  return check_launch("stem16_kernel");
}

int launch_maxpool3(const float* in, int64_t n, int h, int w, int c, float* out, int ldo, hipStream_t s) {
  const size_t total = static_cast<size_t>(n) * out_size(h, 3, 2) * out_size(w, 3, 2) * c;
  hipLaunchKernelGGL(maxpool3_kernel, blocks_of(total), dim3(kThreads), 0, s, in, h, w, c, out, total, ldo);
  return check_launch("maxpool3_kernel");
}

int launch_maxpool3_16(const uint16_t* in, int64_t n, int h, int w, int c, uint16_t* out, int ldo, hipStream_t s) {
  const size_t total8 = static_cast<size_t>(n) * out_size(h, 3, 2) * out_size(w, 3, 2) * c / 8;
  hipLaunchKernelGGL(maxpool3_16_kernel, blocks_of(total8), dim3(kThreads), 0, s, in, h, w, c, out, total8, ldo);
  return check_launch("maxpool3_16_kernel");
}

int launch_conv_gemm(const ConvCall& c, hipStream_t s) {
  auto kernel = c.ks == 1 && c.stride == 1   ? conv_gemm_kernel<1, 1>
                : c.ks == 1 && c.stride == 2 ? conv_gemm_kernel<1, 2>
                : c.ks == 3 && c.stride == 1 ? conv_gemm_kernel<3, 1>
                : c.ks == 3 && c.stride == 2 ? conv_gemm_kernel<3, 2>
                                             : nullptr;
  if (!kernel) { set_error("launch_conv_gemm: no %d x %d / stride %d instance", c.ks, c.ks, c.stride); return SPR_ERR_UNSUPPORTED; }
  if (c.tap_nchw && c.out_nchw) { set_error("launch_conv_gemm: a feature tap goes beside an NHWC result"); return SPR_ERR_UNSUPPORTED; }
  const long long m = static_cast<long long>(c.n) * out_size(c.h, c.ks, c.stride) * out_size(c.w, c.ks, c.stride);
  float* out = c.out_nchw ? c.out_nchw : static_cast<float*>(c.out);
  hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>((m + kGM - 1) / kGM), static_cast<unsigned>(c.cout / kGN)), dim3(kThreads),
                     0, s, static_cast<const float*>(c.in), static_cast<int>(c.n), c.h, c.w, c.cin, c.cout,
                     static_cast<const float*>(c.wts), c.bias, static_cast<const float*>(c.res), c.act, c.out_nchw ? 1 : 0, out,
                     c.in_scale, c.cout_real, c.in_stride(), c.out_stride(), c.c_off, c.pre_s, c.pre_t, c.tap_nchw,
                     c.tap_channels());
  return check_launch("conv_gemm_kernel");
}

namespace {
// both compute kinds of one (ks, stride, channel tile) of conv_gemm16_kernel
template <int KS, int STRIDE, int BN>
auto gemm16_kernel_of(int kind) {
  return kind == SPR_F16 ? conv_gemm16_kernel<KS, STRIDE, SPR_F16, BN> : conv_gemm16_kernel<KS, STRIDE, SPR_BF16, BN>;
}
}  // namespace

int launch_conv_gemm16(int kind, const ConvCall& c, bool bn_switch, hipStream_t s) {
  if (c.in_stride() != c.cin || c.out_stride() != c.cout || c.c_off != 0 || c.pre_s || c.pre_t) {
    set_error("launch_conv_gemm16: conv_gemm16_kernel has no channel strides, channel offset or operand BatchNorm");
    return SPR_ERR_UNSUPPORTED;
  }
  // the tap store reads the residual operand again behind the NHWC store: the two tensors must not be one
  if (c.tap_nchw && (c.out_nchw || c.res == c.out)) {
    set_error("launch_conv_gemm16: a feature tap goes beside an NHWC result that is not the residual operand");
    return SPR_ERR_UNSUPPORTED;
  }
  // 128-channel tiles only on request (SPR_GEMM16_BN=128; tests and A/B runs)
  static const int forced = [] { const char* v = std::getenv("SPR_GEMM16_BN"); return v && *v ? std::atoi(v) : 0; }();
  // (measured on ResNet50 through layer3, batch 32: 17.9 k images/s with 64-channel tiles throughout, 16.9 k with 128)
  const bool wide = bn_switch && c.cout % 128 == 0 && forced == 128;
  const int ks = c.ks, stride = c.stride;
  auto kernel = ks == 1 && stride == 1   ? (wide ? gemm16_kernel_of<1, 1, 128>(kind) : gemm16_kernel_of<1, 1, 64>(kind))
                : ks == 1 && stride == 2 ? (wide ? gemm16_kernel_of<1, 2, 128>(kind) : gemm16_kernel_of<1, 2, 64>(kind))
                : ks == 3 && stride == 2 ? (wide ? gemm16_kernel_of<3, 2, 128>(kind) : gemm16_kernel_of<3, 2, 64>(kind))
                : ks == 3 && stride == 1 && !wide ? gemm16_kernel_of<3, 1, 64>(kind)  // (no 128-channel instance)
                                                  : nullptr;
  if (!kernel) {
    set_error("launch_conv_gemm16: no %d x %d / stride %d instance with %d-channel tiles", ks, ks, stride, wide ? 128 : 64);
    return SPR_ERR_UNSUPPORTED;
  }
  const long long m = static_cast<long long>(c.n) * out_size(c.h, ks, stride) * out_size(c.w, ks, stride);
  // (the kernel reads cout_real in its NCHW store alone - the 16-bit NHWC store always writes all cout channels - so with a
  // tap that argument carries the tap's channel count)
  hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>((m + kHM - 1) / kHM), static_cast<unsigned>(c.cout / (wide ? 128 : 64))),
                     dim3(kThreads), 0, s, static_cast<const uint16_t*>(c.in), static_cast<int>(c.n), c.h, c.w, c.cin, c.cout,
                     static_cast<const uint16_t*>(c.wts), c.bias, static_cast<const uint16_t*>(c.res), c.act,
                     static_cast<uint16_t*>(c.out), c.out_nchw, c.in_scale, c.tap_nchw ? c.tap_channels() : c.cout_real,
                     c.tap_nchw);
  return check_launch("conv_gemm16_kernel");
}

int check_forward_args(const char* name, const void* plan, const void* images, int64_t n, int in_h, int in_w, int in_channels,
                       const float* mean3, const float* inv_std3, const void* packed, const void* workspace, const float* out) {
  if (!plan) { set_error("%s: null plan", name); return SPR_ERR_ARG; }
  if (n < 0 || n > 65535 || in_h < 32 || in_w < 32 || (in_channels != 1 && in_channels != 3)) {
    set_error("%s: bad sizes (n in [0, 65535], images at least 32 x 32, in_channels 1 or 3)", name);
    return SPR_ERR_ARG;
  }
  if (n != 0 && (!images || !mean3 || !inv_std3 || !packed || !out || !workspace)) {
    set_error("%s: null pointer", name);
    return SPR_ERR_ARG;
  }
  return SPR_OK;
}

namespace {
std::string tap_list(const std::vector<int>& accepted) {
  std::string list;
  for (int a : accepted) list += (list.empty() ? "" : ", ") + std::to_string(a);
  return list;
}
}  // namespace

int check_tap(const char* name, const std::vector<int>& accepted, int block, int tap) {
  if (std::find(accepted.begin(), accepted.end(), tap) != accepted.end()) return SPR_OK;
  set_error("%s: tap %d: the taps of this plan (block %d) are the slice ends {%s}", name, tap, block, tap_list(accepted).c_str());
  return SPR_ERR_ARG;
}

int check_taps(const char* name, const std::vector<int>& accepted, int block, int32_t n_taps, const int32_t* tap_features,
               float* const* tap_out, int64_t n, TapSet* set) {
  if (n_taps < 0 || (n_taps > 0 && (!tap_features || !tap_out))) { set_error("%s: bad tap arrays", name); return SPR_ERR_ARG; }
  for (int32_t t = 0; t < n_taps; ++t) {
    const int rc = check_tap(name, accepted, block, tap_features[t]);
    if (rc != SPR_OK) return rc;
    if (std::find(set->feature.begin(), set->feature.end(), tap_features[t]) != set->feature.end()) {
      set_error("%s: tap %d named twice: each of the slice ends {%s} (block %d) at most once", name, tap_features[t],
                tap_list(accepted).c_str(), block);
      return SPR_ERR_ARG;
    }
    if (n != 0 && !tap_out[t]) { set_error("%s: null buffer for tap %d", name, tap_features[t]); return SPR_ERR_ARG; }
    set->feature.push_back(tap_features[t]);
    set->out.push_back(tap_out[t]);
  }
  return SPR_OK;
}

int trace_copy(unsigned char* trace, const TraceLayout* lay, size_t i, const void* src, hipStream_t s) {
  if (!trace) return SPR_OK;
  const TraceRec& r = lay->recs[i];
  if (hipMemcpyAsync(trace + r.off, src, r.bytes, hipMemcpyDeviceToDevice, s) != hipSuccess) {
    set_error("spr_*_forward_trace: copy of record %zu failed", i);
    return SPR_ERR_HIP;
  }
  return SPR_OK;
}

int trace_query(const TraceLayout& lay, int64_t* records, size_t* total_bytes) {
  if (records)
    for (size_t i = 0; i < lay.recs.size(); ++i) {
      const TraceRec& r = lay.recs[i];
      const int64_t v[6] = {static_cast<int64_t>(r.off), r.h, r.w, r.c, r.dtype, r.nchw};
      for (int k = 0; k < 6; ++k) records[6 * i + k] = v[k];
    }
  if (total_bytes) *total_bytes = lay.total;
  return static_cast<int>(lay.recs.size());
}

}  // namespace spr
