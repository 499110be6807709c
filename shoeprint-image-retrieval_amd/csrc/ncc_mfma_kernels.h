// Direct-form NCC on the bf16 matrix cores: the scorer for SMALL feature maps stored as bfloat16 (ResNet50 layer3
// and VGG16 conv5_3 shaped, cropped 28 x 12: BASELINE configs 3 and 5), where the FFT form spends its time on the
// prepared spectra (15 KB per pair and channel against 0.7 KB of raw features).
//
// Per channel the numerator of similarity.py:48-55 is a product of a [queries x taps] with a [taps x positions] matrix:
//     num[q, p] = sum_tap t0[q, tap] * I0z[p + tap]        (I0z = centred search map, zero outside: scipy 'same')
// A = the RAW template values: bfloat16 as stored, so every product below is exact.  Two forms of B:
//   exact (default): B = the RAW search map, zero outside - one MFMA per tile step, products exact on both sides - and
//       num = R - mean(I) * St0[q,p] - mean(t) * SI[p]   (St0: the centred template summed over the taps that fall inside
//       the map at p; SI: window sum of the raw map).  The last term is a weight of the epilogue; the middle one, summed
//       over the channels with the weights, is a [queries x channels] x [channels x gallery] product PER POSITION:
//       corr_mfma_kernel (f32 matrix cores, 0.6 % of the flops) writes it before the pair kernel subtracts it at the end.
//   split (SPR_NCC_MFMA_EXACT=0): B = I0z = hi + lo, two bfloat16 numbers (16 significant bits), two MFMAs per tile step,
//       num = R - mean(t) * S1[p]  (S1 = window sum of I0z, :59); self-contained, half as fast.
//   float32 maps (SPR_NCC_MFMA_F32): BOTH operands centred in float32 and split, t0 = t_hi + t_lo and I0z = I_hi + I_lo, and
//       num = sum t_hi I_hi + t_hi I_lo + t_lo I_hi - mean(t_hi + t_lo) * S1[p]: three MFMAs per tile step (the fourth
//       product is of order 2^-32), nothing raw enters a product, so neither the correction matrix nor the exact shift.
//       Every channel takes TWO periods of the schedule below - t_hi x (I_hi, I_lo), then t_lo x I_hi onto the same
//       accumulators - and is weighted once, after the second.
// B is never materialised: it is a Toeplitz gather from the zero-padded map of the channel, kept in LDS in eight copies
// shifted by one element each so that every lane's eight consecutive taps are one aligned ds_read_b128.
// A fragment (8 taps of 16 positions) depends on (row of the position + row of the tap) only, so one fragment read
// feeds up to NTG tiles of 16 positions, each against another template row pair: 78 fragment reads for 294 tile steps.
//
// One workgroup = one gallery item x 64 queries (one wave = 16 queries = the M side of v_mfma_f32_16x16x32_bf16), walking
// the channels: per channel 294 (split: 588) MFMAs per wave, then per position  sum += a[q] * (b[p] * acc) - (a*mean)[q] * (b*S)[p]
// (a = 1/sqrt(sum t0^2), b = 1/sigma of the window, both float32 from float64 statistics as in the other methods),
// channel sum in registers, spatial maximum and the running maximum over variants at the end (similarity.py:100-108,
// :355-367).
//
// This header holds the kernels and the pair launcher; it is included by ncc_mfma.hip (geometry, preparation launchers, the
// pair kernels in their plain form) and by ncc_mfma_peaks.hip (the pair kernels in their peak form): two translation units,
// so that the plain instances are compiled exactly as before and the two sets build side by side.
#pragma once
#include <cstdlib>
#include <type_traits>

#include "ncc_prep_common.h"

// -DSPR_MFMA_ABL=n: timing ablations (wrong results), tools/ubench/ablate_mfma.sh.  1: no epilogues, 2: one fragment read per
// period instead of one per step, 3: no staging of the next channel, 4: no reloads of the template fragments, 5: no barrier
// per channel
#ifndef SPR_MFMA_ABL
#define SPR_MFMA_ABL 0
#endif
// -DSPR_MFMA_GROUPS=n: n vector instructions behind every MFMA of a fragment step (scheduler groups); 0: the compiler's order
#ifndef SPR_MFMA_GROUPS
#define SPR_MFMA_GROUPS 0
#endif
// fragment steps between the LDS read of a fragment and its MFMAs
#ifndef SPR_MFMA_AHEAD
#define SPR_MFMA_AHEAD 2
#endif

namespace spr {

namespace {

// compile-time loop: f(integral_constant<int, I>) for I in [0, N) - register arrays indexed by I stay in registers
template <int I, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for<I + 1, N>(f);
  }
}

// TH x TW: the FRAME of positions = the largest cropped search map of the instance (a smaller map sits in its top-left corner:
// the other positions carry 1/sigma = 0 and zero pixels, which is what the zero padding of 'same' mode puts there anyway).
// FH x 16: the template frame, FH even; a cropped template of th x tw taps sits in it so that its centre tap (th/2, tw/2) -
// the tap 'same' mode lays on the output pixel (similarity.py:55) - lands on (CY, CX) = (FH/2, CXF).  MCfg<28, 12> is the
// equal-size instance of BASELINE config 3 (template = map = 28 x 12: no spare taps, no spare positions);
// MCfg<28, 12, 30, 8> takes any template up to 30 x 16 on any map up to 28 x 12 (scaled / rotated query variants,
// similarity.py:230-284, and ragged sets) for one k-step more.
template <int TH_, int TW_, int FH_ = TH_, int CXF_ = TW_ / 2>
struct MCfg {
  static constexpr int TH = TH_, TW = TW_;  // frame of positions (cropped search map)
  static constexpr int FH = FH_;               // template frame rows
  static constexpr int NPOS = TH * TW;
  static constexpr int NTILE = NPOS / 16;      // tiles of 16 positions (row-major positions)
  static constexpr int KS = FH / 2;            // k-steps: two template rows of 16 taps (TW padded to 16 with zeros)
  static constexpr int TP = TW == 12 ? 3 : 2;  // tiles t and t + TP cover the same columns DY rows further down
  static constexpr int DY = 16 * TP / TW;
  static constexpr int NTG = NTILE / TP;
  static constexpr int SMAX = DY * (NTG - 1) + 2 * (KS - 1);
  static constexpr int PR = TH + FH - 1;  // rows of the zero-padded map
  static constexpr int CY = FH / 2, CX = CXF_;
  // largest template / map the instance takes
  static constexpr int kMaxTh = 2 * (FH - CY) < 2 * CY + 1 ? 2 * (FH - CY) : 2 * CY + 1;
  static constexpr int kMaxTw = 2 * (16 - CX) < 2 * CX + 1 ? 2 * (16 - CX) : 2 * CX + 1;
  static_assert(NPOS % 16 == 0 && FH % 2 == 0 && NTILE % TP == 0 && DY % 2 == 0 && TW <= 16, "unsupported map size");
  // LDS image of one channel: copy k (0..7) holds P shifted left by k elements, in chunks of 8 elements (16 bytes): chunk
  // (copy k, chunk column jj, row r) at jj * JS + r * RS + k * 16 - the eight copies of a row side by side (128 bytes), JS a
  // multiple of the 256-byte bank row.  ds_read_b128 is served in four groups of sixteen lanes that are NOT contiguous
  // ({0-3, 12-15, 20-27}, ...: MI355X_MICROARCH.md, LDS): of the layouts with a linear chunk -> bank-slot map this is the best,
  // 16 LDS cycles for the twelve (phase, group) reads of a fragment step against 12 without conflicts and 24 for the
  // first layout of this kernel (measured there: SQ_LDS_BANK_CONFLICT = half of SQ_LDS_IDX_ACTIVE).
  static constexpr int RS = 128;
  static constexpr int JS = (PR + 1) / 2 * 2 * RS;
  static constexpr int HL = 3 * JS;  // lo plane behind the hi plane
  static constexpr int kCopyBytes = 2 * HL;
  static constexpr int kEbOff = kCopyBytes;                // {b, b*S1}[NPOS] (float pairs)
  static constexpr int kDummyOff = kEbOff + 2 * 4 * NPOS;  // 16 bytes nobody reads: where masked-out stores go (no branches)
  static constexpr int kBufBytes = kDummyOff + 16;         // one channel; three buffers: channels c - 1 and c are read while
  static constexpr int kLdsBytes = 3 * kBufBytes;          // channel c + 1 is staged
  static constexpr int PERIOD = 2 * KS;                    // row offsets (even) one channel takes per tile group
  static_assert(DY * (NTG - 1) < PERIOD, "a tile group may lag the first one by less than a channel");
  static_assert(kBufBytes % 16 == 0, "buffer alignment");
  // prepared layouts
  static constexpr int kQMapBytes = FH * 16 * 2;           // per channel: the template frame, rows of 16 taps (16-bit)
  static constexpr int kGChanBytes = 3 * 4 * NPOS;         // per channel: b, b*S1 (float), hi|lo (one word per pixel)
  // exact form: U[position][channel] (query) and V[position][channel] (gallery) follow, channels padded to 16 (zeros)
  static constexpr int kXQ = 64;                           // queries per block = row length of the correction matrix
  // A fragment (phase ph, row offset s) reads rows s + y + {0, 1} of the padded map, y = the rows of the phase's sixteen
  // positions; the map proper occupies rows [CY, CY + TH): a fragment entirely above or below it is all zeros - neither read
  // nor multiplied (10 of the 26 row offsets of a phase; the tile steps on them are 18 % of all)
  static constexpr bool frag_zero(int ph, int s) {
    const int ymin = (16 * ph) / TW, ymax = (16 * ph + 15) / TW;
    return s + ymax + 1 < CY || s + ymin >= CY + TH;
  }
  // the first k-step of tile (tg, ph) whose fragment is not all zeros: its MFMA starts the accumulator
  static constexpr int first_ks(int tg, int ph) {
    for (int ks = 0; ks < KS; ++ks)
      if (!frag_zero(ph, DY * tg + 2 * ks)) return ks;
    return KS;
  }
};
__host__ __device__ inline int pad16(int c) { return (c + 15) / 16 * 16; }

struct MfmaArgs {
  int channels, nq, ng;
  long long ld, col0;
  int accumulate;
  unsigned q_item_bytes, g_item_bytes;
  // exact form: x[position][gallery item of this launch][query of the block] = sum_c U V, subtracted from the channel sums
  const float* x;
  int x_items;
  int ih, iw;  // the real (cropped) search map inside the frame of positions: what spr_ncc_maps writes
};

__device__ __forceinline__ unsigned bf16_round(float v) {  // round to nearest even, finite inputs
  const unsigned u = __float_as_uint(v);
  return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}
__device__ __forceinline__ float bf16_value(unsigned bits) { return __uint_as_float(bits << 16); }
// a float as the plan's 16-bit storage type (bit pattern) and back
__device__ __forceinline__ unsigned to_storage(float v, int dtype) {
  if (dtype == SPR_BF16) return bf16_round(v);
  union { _Float16 h; uint16_t u; } c;
  c.h = static_cast<_Float16>(v);
  return c.u;
}
__device__ __forceinline__ float from_storage(unsigned bits, int dtype) {
  if (dtype == SPR_BF16) return bf16_value(bits);
  union { _Float16 h; uint16_t u; } c;
  c.u = static_cast<uint16_t>(bits);
  return static_cast<float>(c.h);
}

// ---- the formulas every preparation path shares (queries, galleries per wave, galleries through the tables) ---------------
// v rounded to the storage type: of a channel mean, kappa - the candidate of the exact shift (see prep_mfma_kernel)
__device__ __forceinline__ float storage_round(float v, int dtype) { return from_storage(to_storage(v, dtype), dtype); }
__device__ __forceinline__ bool representable(float v, int dtype) { return storage_round(v, dtype) == v; }
// a pixel as the matrix cores see it: as stored, or shifted by kappa (0: no exact shift)
__device__ __forceinline__ unsigned shifted_bits(unsigned bits, float kappa, int dtype) {
  return kappa == 0.0f ? bits : to_storage(from_storage(bits, dtype) - kappa, dtype);
}
// split form: v = hi + lo, two bfloat16 numbers in one word
__device__ __forceinline__ unsigned hilo_word(float v) {
  const unsigned hi = bf16_round(v);
  return (hi << 16) | bf16_round(v - bf16_value(hi));
}
// [first, first + size) clipped to [0, limit]; the window 'same' mode lays on a centre starts size / 2 before it
struct Span { int lo, hi; };
__device__ __forceinline__ Span clip_span(int first, int size, int limit) {
  const int last = first + size;
  return Span{first < 0 ? 0 : (first > limit ? limit : first), last < 0 ? 0 : (last > limit ? limit : last)};
}
__device__ __forceinline__ Span window(int centre, int size, int limit) { return clip_span(centre - size / 2, size, limit); }
// window sum of the raw map from the window sum s1 of the centred one
__device__ __forceinline__ double raw_window_sum(double s1, float mean, Span rows, Span cols) {
  return s1 + static_cast<double>(mean) * static_cast<double>((rows.hi - rows.lo) * (cols.hi - cols.lo));
}
// A prepared gallery item (Byte: unsigned char or const unsigned char).  Per channel b = 1/sigma, b * S (float) and the pixel
// words hi|lo, NPOS of each; exact form: V[position][channel] behind the channels, then the channel means (both padded to 16)
template <class M, class Byte>
struct GalleryItem {
  template <class T> using As = std::conditional_t<std::is_const_v<Byte>, const T, T>;
  Byte* base;
  int channels;
  __device__ __forceinline__ As<float>* b(int c) const { return reinterpret_cast<As<float>*>(base + static_cast<size_t>(c) * M::kGChanBytes); }
  __device__ __forceinline__ As<float>* bs(int c) const { return b(c) + M::NPOS; }
  __device__ __forceinline__ As<unsigned>* hl(int c) const { return reinterpret_cast<As<unsigned>*>(b(c) + 2 * M::NPOS); }
  __device__ __forceinline__ As<float>* V() const { return b(channels); }
  __device__ __forceinline__ As<float>* means() const { return V() + static_cast<size_t>(M::NPOS) * pad16(channels); }
};

// LDS of the prep kernel: the centred map (template or search map, whichever is larger) and two float64 summed-area tables.
// The equal-size instance holds exactly its 28 x 12 map (7.4 KB per wave-sized workgroup: 21 of them share a CU).
template <class M>
struct MPrepSizes {
  static constexpr bool kFixed = M::FH == M::TH;
  static constexpr int kMaxPix = kFixed ? M::NPOS : (M::FH * 16 > M::NPOS ? M::FH * 16 : M::NPOS);
  static constexpr int kSatElems = kFixed ? (M::TH + 1) * (M::TW + 1)
                                          : ((M::FH + 1) * 17 > (M::TH + 1) * (M::TW + 1) ? (M::FH + 1) * 17 : (M::TH + 1) * (M::TW + 1));
};

// ---- preparation: grid = (channels, items) ---------------------------------------------------------------------------
// EXACT form: the search map enters the matrix cores RAW (bf16 as stored: one MFMA per tile step, every product exact) and
// the centring of both sides becomes two corrections of the raw product R[q,p] = sum_tap t[q,tap] Iz[p + tap]:
//     num = R - mean(I) * St0[q,p] - mean(t) * SI[p],     St0 = sum of the centred template over the taps whose pixel lies
//                                                          inside the map at position p, SI = window sum of the raw map
// The last term is a weight of the pair kernel's epilogue like before (b * SI in place of b * S1); the middle one is a
// contraction over the channels per position, X[q,g,p] = sum_c (a St0)[q,c,p] * (b mean(I))[g,c,p], left to corr_mfma_kernel.
// F32 (float32 maps, never EXACT): the query side writes the centred template as two planes of bfloat16 rows (hi, then lo)
// and {a, a * mean(hi + lo)} (mean_term = 0: {a, 0}, an A/B switch); the gallery side is the split form's as it stands.
template <class M, bool EXACT, bool FIXED, bool F32 = false>
__global__ void __launch_bounds__(kThreads)
prep_mfma_kernel(NccGeom g, int is_query, const void* __restrict__ maps, unsigned char* __restrict__ prepared,
                 size_t item_bytes, int mean_term) {
  static_assert(!(F32 && EXACT), "float32 maps: the hi + lo form only");
  // Real sizes (cropped): template th x tw inside the FH x 16 frame, search map ih x iw inside the TH x TW frame.  FIXED (the
  // equal-size instance: template = map = the frame of positions): compile-time constants - with run-time sizes the kernel took
  // 51 ms instead of 31 for BASELINE config 3's gallery.
  const int th = FIXED ? M::TH : g.th, tw = FIXED ? M::TW : g.tw, ih = FIXED ? M::TH : g.ih, iw = FIXED ? M::TW : g.iw;
  const int fy = M::CY - th / 2, fx = M::CX - tw / 2;  // frame position of template tap (0, 0)
  constexpr int kMaxPix = MPrepSizes<M>::kMaxPix, kSatElems = MPrepSizes<M>::kSatElems;
  unsigned char* lds = dyn_lds();
  double* red = reinterpret_cast<double*>(lds);
  float* x0 = reinterpret_cast<float*>(lds + 64);
  double* sat1 = reinterpret_cast<double*>(lds + align_up(64 + sizeof(float) * kMaxPix, 16));
  double* sat2 = sat1 + kSatElems;
  const int c = static_cast<int>(blockIdx.x);
  const size_t item = blockIdx.y;
  const int tid = static_cast<int>(threadIdx.x);
  const int cp = pad16(g.channels);
  unsigned char* out_item = prepared + item * item_bytes;
  const uint16_t* raw = static_cast<const uint16_t*>(maps);
  auto build_tables = [&](int h, int w) {
    if (sat_blocked_fits(h, w))
      build_sat_pair_blocked(x0, h, w, sat1, sat2);
    else
      build_sat_pair(x0, h, w, sat1, sat2);
  };
  // Conditioning.  The raw operands make  num = R - corrections  a difference of numbers (mean / sigma)^2 times larger than
  // num (measured: 4e-4 on scores of maps offset by 100 sigma).  A channel whose values all sit near its mean - the only way
  // to have a large mean / sigma - can be shifted EXACTLY in its storage type: kappa = the mean rounded to the storage type,
  // x - kappa representable for every pixel (checked here, pixel by pixel).  Then x - kappa enters the matrix cores and
  // mean - kappa the corrections: the same algebra, exact products as before, and the cancellation is gone.  Channels spread
  // over several binades fail the check and stay as they are: their mean / sigma is small.
  auto exact_shift = [&](size_t base, int raw_w, int h, int w, float mean) {  // returns kappa (0: no exact shift exists)
    const float kappa = storage_round(mean, g.dtype);
    double bad = 0.0;
    for (int i = tid; i < h * w; i += wg_size()) {
      const int y = i / w, x = i - y * w;
      const float d = from_storage(raw[base + static_cast<size_t>(y + g.crop) * raw_w + (x + g.crop)], g.dtype) - kappa;
      if (!representable(d, g.dtype)) bad += 1.0;
    }
    return block_sum(bad, red) == 0.0 ? kappa : 0.0f;
  };
  // the channel columns that pad U / V to a multiple of 16 are zero: the last channel's workgroup writes them
  auto store_column = [&](float* mat, int pos, float v) {
    mat[static_cast<size_t>(pos) * cp + c] = v;
    if (c == g.channels - 1)
      for (int k = g.channels; k < cp; ++k) mat[static_cast<size_t>(pos) * cp + k] = 0.0f;
  };
  if (is_query) {
    const size_t base = (item * g.channels + c) * static_cast<size_t>(g.q_h) * g.q_w;
    float mean;
    load_centred(maps, base, g.q_w, g.crop, th, tw, g.dtype, x0, red, &mean);
    const float scale = template_scale(x0, th * tw, red);
    if constexpr (F32) {
      uint16_t* rows = reinterpret_cast<uint16_t*>(out_item + static_cast<size_t>(c) * (2 * M::kQMapBytes));
      double s = 0.0;  // sum of hi + lo: not exactly zero
      for (int i = tid; i < M::FH * 16; i += wg_size()) {
        const int u = (i >> 4) - fy, v = (i & 15) - fx;
        const unsigned w = hilo_word((u >= 0 && u < th && v >= 0 && v < tw) ? x0[u * tw + v] : 0.0f);
        rows[i] = static_cast<uint16_t>(w >> 16);
        rows[M::FH * 16 + i] = static_cast<uint16_t>(w & 0xffffu);
        s += static_cast<double>(bf16_value(w >> 16)) + static_cast<double>(bf16_value(w & 0xffffu));
      }
      const float resid = mean_term ? static_cast<float>(block_sum(s, red) / static_cast<double>(th * tw)) : 0.0f;
      float* sc = reinterpret_cast<float*>(out_item + static_cast<size_t>(g.channels) * (2 * M::kQMapBytes));
      if (tid == 0) {
        sc[2 * c] = scale;
        sc[2 * c + 1] = scale * resid;
      }
      return;
    }
    const float kappa = exact_shift(base, g.q_w, th, tw, mean);
    // the template frame in the storage type (taps as stored, or shifted by kappa; zero outside the template)
    uint16_t* rows = reinterpret_cast<uint16_t*>(out_item + static_cast<size_t>(c) * M::kQMapBytes);
    for (int i = tid; i < M::FH * 16; i += wg_size()) {
      const int u = (i >> 4) - fy, v = (i & 15) - fx;
      rows[i] = (u >= 0 && u < th && v >= 0 && v < tw)
                    ? static_cast<uint16_t>(shifted_bits(raw[base + static_cast<size_t>(u + g.crop) * g.q_w + (v + g.crop)], kappa, g.dtype))
                    : static_cast<uint16_t>(0);
    }
    float* sc = reinterpret_cast<float*>(out_item + static_cast<size_t>(g.channels) * M::kQMapBytes);
    if (tid == 0) {
      sc[2 * c] = scale;
      sc[2 * c + 1] = scale * (mean - kappa);
    }
    if constexpr (EXACT) {
      float* U = sc + 2 * g.channels;
      build_tables(th, tw);
      const int stride = tw + 1;
      for (int i = tid; i < M::NPOS; i += wg_size()) {
        const int y = i / M::TW, x = i - y * M::TW;
        // taps (u, v) whose pixel (y + u - th/2, x + v - tw/2) lies inside the map
        const Span u = clip_span(th / 2 - y, ih, th), v = clip_span(tw / 2 - x, iw, tw);
        double st0 = 0.0;
        if (y < ih && x < iw && u.hi > u.lo && v.hi > v.lo)
          st0 = sat1[u.hi * stride + v.hi] - sat1[u.lo * stride + v.hi] - sat1[u.hi * stride + v.lo] + sat1[u.lo * stride + v.lo];
        store_column(U, i, scale * static_cast<float>(st0));
      }
    }
  } else {
    const size_t base = (item * g.channels + c) * static_cast<size_t>(g.g_h) * g.g_w;
    float mean;
    load_centred(maps, base, g.g_w, g.crop, ih, iw, g.dtype, x0, red, &mean);
    const float kappa = EXACT ? exact_shift(base, g.g_w, ih, iw, mean) : 0.0f;
    if constexpr (EXACT) mean -= kappa;  // from here on: the mean of the map as the matrix cores see it
    const GalleryItem<M, unsigned char> out{out_item, g.channels};
    float* eb = out.b(c);
    float* ebs = out.bs(c);
    unsigned* hl = out.hl(c);
    for (int i = tid; i < M::NPOS; i += wg_size()) {
      const int y = i / M::TW, x = i - y * M::TW;
      const bool inside = y < ih && x < iw;
      if constexpr (EXACT)
        hl[i] = inside ? shifted_bits(raw[base + static_cast<size_t>(y + g.crop) * g.g_w + (x + g.crop)], kappa, g.dtype) << 16 : 0u;
      else
        hl[i] = hilo_word(inside ? x0[y * iw + x] : 0.0f);
    }
    build_tables(ih, iw);
    // the mean of the channel, behind V: vcol_mfma_kernel turns b and the means into V[position][channel]
    if constexpr (EXACT)
      if (tid == 0) out.means()[c] = mean;
    const double inv_n = 1.0 / static_cast<double>(th * tw);
    for (int i = tid; i < M::NPOS; i += wg_size()) {
      const int y = i / M::TW, x = i - y * M::TW;
      if (y >= ih || x >= iw) {  // a position of the frame outside the map: weight 0
        eb[i] = 0.0f;
        ebs[i] = 0.0f;
        continue;
      }
      const double s1 = window_sum(sat1, ih, iw, th, tw, y, x);
      const double s2 = window_sum(sat2, ih, iw, th, tw, y, x);
      const float inv = inv_sigma_from_sums(s1, s2, inv_n);
      eb[i] = inv;
      ebs[i] = inv * static_cast<float>(EXACT ? raw_window_sum(s1, mean, window(y, th, ih), window(x, tw, iw)) : s1);
    }
  }
}

// ---- gallery preparation of both instances: one wave = TWO channels ----------------------------------------------------
// prep_mfma_kernel above spends ~7 000 SIMD cycles on a 336-pixel map, most of them in the summed-area tables built for maps
// of any size.  Here lane = (channel of the pair, row): its 12 pixels stay in registers; the column-range sums of its row
// (float64, 12 values per table) go to LDS; 48 lanes = (table, channel, column) run down the 28 rows; the row lanes pick their
// 2 x 12 window sums up again and finish 1/sigma, the raw window sum and the pixel words.  Same statistics as prep_mfma_kernel
// (float64 sums of float32 values and float32 squares, similarity.py:57-62), formed in another order: a few ulp of float64
// apart.  grid = (ceil(channels / 2), items), 64 lanes.  The instances differ in how the two range sums are formed only:
//   equal-size (kFixed: template = map = frame, all sizes compile-time constants): every window is a corner window - rows
//     [max(0, y - TH/2), min(TH, y + TH/2)), columns likewise - so each range sum is a difference of two prefixes at
//     compile-time positions: prefixes in REGISTERS, the column lanes write the row-range sum of every y back in place.
//   general (any template on any map of the frame): rows [y - th/2, y - th/2 + th) clipped to the map at run time, so the range
//     sums are differences of INCLUSIVE prefixes picked at run-time positions: the prefixes go through LDS (a register array
//     cannot be indexed at run time without scratch) - along the row (written and read back by the same lane), then down
//     the columns.
template <class M, bool EXACT, bool F32 = false>
__global__ void __launch_bounds__(64)
prep_gallery_wave_kernel(NccGeom g, const void* __restrict__ maps, unsigned char* __restrict__ prepared, size_t item_bytes) {
  constexpr int H = M::TH, W = M::TW;
  constexpr bool kFixed = MPrepSizes<M>::kFixed;
  static_assert(H <= 32 && W % 4 == 0 && 4 * W <= 64, "one row per lane, two channels per wave");
  __shared__ double tab[2][2][H][W];
  const int th = kFixed ? H : g.th, tw = kFixed ? W : g.tw, ih = kFixed ? H : g.ih, iw = kFixed ? W : g.iw;
  const int lane = static_cast<int>(threadIdx.x), half = lane >> 5, row = lane & 31;
  const int c = 2 * static_cast<int>(blockIdx.x) + half;
  const size_t item = blockIdx.y;
  const bool chan_ok = c < g.channels;
  const bool in_map = row < ih && chan_ok;    // this lane holds a row of the map
  const bool frame_row = row < H && chan_ok;  // every row of the frame is written (zeros outside the map)
  const int cc = chan_ok ? c : g.channels - 1, rr = row < ih ? row : ih - 1;
  static_assert(!(F32 && EXACT), "float32 maps: the hi + lo form only");
  const size_t row_at = ((item * g.channels + cc) * static_cast<size_t>(g.g_h) + (rr + g.crop)) * g.g_w + g.crop;
  unsigned bits[W];
  float v[W];
  if constexpr (F32) {
    const float* raw = static_cast<const float*>(maps) + row_at;
#pragma unroll
    for (int k = 0; k < W; ++k) {
      bits[k] = 0u;
      v[k] = raw[k < iw ? k : iw - 1];
    }
  } else {
    const uint16_t* raw = static_cast<const uint16_t*>(maps) + row_at;
#pragma unroll
    for (int k = 0; k < W; ++k) bits[k] = raw[k < iw ? k : iw - 1];
#pragma unroll
    for (int k = 0; k < W; ++k) v[k] = from_storage(bits[k], g.dtype);
  }
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < W; ++k) {
    v[k] = in_map && k < iw ? v[k] : 0.0f;
    s += static_cast<double>(v[k]);
  }
#pragma unroll
  for (int m = 16; m >= 1; m >>= 1) s += shfl_xor(s, m);  // over the 32 lanes of this channel
  float mean = static_cast<float>(s / static_cast<double>(ih * iw));
  // exact shift (see prep_mfma_kernel): kappa = the mean in the storage type, taken if x - kappa is representable everywhere
  float kappa = 0.0f;
  if constexpr (EXACT) {
    kappa = storage_round(mean, g.dtype);
    int bad = 0;
#pragma unroll
    for (int k = 0; k < W; ++k)
      if (in_map && k < iw && !representable(v[k] - kappa, g.dtype)) bad = 1;
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) bad |= shfl_xor(bad, m);
    if (bad) kappa = 0.0f;
  }
  const GalleryItem<M, unsigned char> out{prepared + item * item_bytes, g.channels};
  float x0[W];
  unsigned word[W];
#pragma unroll
  for (int k = 0; k < W; ++k) {
    const bool inside = in_map && k < iw;
    x0[k] = inside ? v[k] - mean : 0.0f;
    if constexpr (EXACT)
      word[k] = inside ? shifted_bits(bits[k], kappa, g.dtype) << 16 : 0u;
    else
      word[k] = hilo_word(x0[k]);
  }
  if (frame_row) {
#pragma unroll
    for (int k = 0; k < W; k += 4)
      *reinterpret_cast<u32x4*>(out.hl(cc) + row * W + k) = u32x4{word[k], word[k + 1], word[k + 2], word[k + 3]};
  }
  if constexpr (EXACT) {
    mean -= kappa;  // from here on: the mean of the map as the matrix cores see it
    if (chan_ok && row == 0) out.means()[c] = mean;
  }
  // column-range sums of this row -> tab
  if constexpr (kFixed) {
    static_assert(M::FH == M::TH, "corner windows: template = map = frame");
    double p1[W + 1], p2[W + 1];
    p1[0] = 0.0; p2[0] = 0.0;
#pragma unroll
    for (int k = 0; k < W; ++k) {
      const float sq = x0[k] * x0[k];  // np.square keeps float32 (similarity.py:57)
      p1[k + 1] = p1[k] + static_cast<double>(x0[k]);
      p2[k + 1] = p2[k] + static_cast<double>(sq);
    }
    if (row < H) {
#pragma unroll
      for (int x = 0; x < W; ++x) {
        const Span cols = window(x, W, W);
        tab[0][half][row][x] = p1[cols.hi] - p1[cols.lo];
        tab[1][half][row][x] = p2[cols.hi] - p2[cols.lo];
      }
    }
  } else if (row < H) {  // inclusive prefixes along the row -> LDS -> the range sums, back in place
    double r1 = 0.0, r2 = 0.0;
#pragma unroll
    for (int k = 0; k < W; ++k) {
      const float sq = x0[k] * x0[k];
      r1 += static_cast<double>(x0[k]);
      r2 += static_cast<double>(sq);
      tab[0][half][row][k] = r1;
      tab[1][half][row][k] = r2;
    }
    double c1[W], c2[W];
#pragma unroll
    for (int x = 0; x < W; ++x) {
      const Span cols = window(x, tw, iw);
      const double hi1 = cols.hi > 0 ? tab[0][half][row][cols.hi - 1] : 0.0, lo1 = cols.lo > 0 ? tab[0][half][row][cols.lo - 1] : 0.0;
      const double hi2 = cols.hi > 0 ? tab[1][half][row][cols.hi - 1] : 0.0, lo2 = cols.lo > 0 ? tab[1][half][row][cols.lo - 1] : 0.0;
      c1[x] = hi1 - lo1;
      c2[x] = hi2 - lo2;
    }
#pragma unroll
    for (int x = 0; x < W; ++x) {
      tab[0][half][row][x] = c1[x];
      tab[1][half][row][x] = c2[x];
    }
  }
  __syncthreads();
  if (lane < 4 * W) {  // (table, channel, column): down the rows, in place
    double* col = &tab[0][0][0][0] + (lane / W) * (H * W) + lane % W;
    double P[H + 1];
    P[0] = 0.0;
#pragma unroll
    for (int r = 0; r < H; ++r) P[r + 1] = P[r] + col[r * W];
#pragma unroll
    for (int y = 0; y < H; ++y) {
      const Span rows = kFixed ? window(y, H, H) : Span{0, y + 1};  // the row-range sum of y, or the inclusive prefix
      col[y * W] = P[rows.hi] - P[rows.lo];
    }
  }
  __syncthreads();
  if (!frame_row) return;
  const double inv_n = 1.0 / static_cast<double>(th * tw);
  const Span rows = window(row, th, ih);
  float o_b[W], o_bs[W];
#pragma unroll
  for (int x = 0; x < W; ++x) {
    double s1, s2;
    if constexpr (kFixed) {
      s1 = tab[0][half][row][x];
      s2 = tab[1][half][row][x];
    } else {
      s1 = (rows.hi > 0 ? tab[0][half][rows.hi - 1][x] : 0.0) - (rows.lo > 0 ? tab[0][half][rows.lo - 1][x] : 0.0);
      s2 = (rows.hi > 0 ? tab[1][half][rows.hi - 1][x] : 0.0) - (rows.lo > 0 ? tab[1][half][rows.lo - 1][x] : 0.0);
    }
    const bool inside = row < ih && x < iw;
    const float inv = inside ? inv_sigma_from_sums(s1, s2, inv_n) : 0.0f;
    o_b[x] = inv;
    const double sw = EXACT ? raw_window_sum(s1, mean, rows, window(x, tw, iw)) : s1;  // window sum of the raw / the centred map
    o_bs[x] = inside ? inv * static_cast<float>(sw) : 0.0f;
  }
#pragma unroll
  for (int k = 0; k < W; k += 4) {
    *reinterpret_cast<float4*>(out.b(cc) + row * W + k) = float4{o_b[k], o_b[k + 1], o_b[k + 2], o_b[k + 3]};
    *reinterpret_cast<float4*>(out.bs(cc) + row * W + k) = float4{o_bs[k], o_bs[k + 1], o_bs[k + 2], o_bs[k + 3]};
  }
}

// ---- exact form: V[p][c] = b[c][p] * mean[c] of one gallery item, 32 channels per workgroup through an LDS tile (the prep
// workgroups own one channel each: written from there, V would be 4-byte stores 4 KB apart).  grid = (channel blocks, items)
template <class M>
__global__ void __launch_bounds__(kThreads)
vcol_mfma_kernel(int channels, unsigned char* __restrict__ prepared, size_t item_bytes) {
  __shared__ float tile[32][M::NPOS + 1];
  const int tid = static_cast<int>(threadIdx.x);
  const int cp = pad16(channels), c0 = static_cast<int>(blockIdx.x) * 32;
  const GalleryItem<M, unsigned char> item{prepared + static_cast<size_t>(blockIdx.y) * item_bytes, channels};
  float* V = item.V();
  const float* means = item.means();
  const int p1 = tid + kThreads < M::NPOS ? tid + kThreads : tid;  // second pixel of this work-item (or the first again)
  for (int cb = 0; cb < 32; cb += 8) {
    float v0[8], v1[8];  // eight channel rows in flight
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int c = c0 + cb + k < channels ? c0 + cb + k : channels - 1;
      const float* b = item.b(c);
      const float m = c0 + cb + k < channels ? means[c] : 0.0f;
      v0[k] = b[tid] * m;
      v1[k] = b[p1] * m;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      tile[cb + k][tid] = v0[k];
      tile[cb + k][p1] = v1[k];
    }
  }
  __syncthreads();
  const int cc = tid & 31;
  if (c0 + cc < cp)
    for (int p = tid >> 5; p < M::NPOS; p += kThreads / 32) V[static_cast<size_t>(p) * cp + c0 + cc] = tile[cc][p];
}

// ---- exact form: X[p][g][q] = sum_c U[q][p][c] * V[g][p][c] on the f32 matrix cores (exact f32 products) ---------------
// grid = (blocks of 64 gallery items, positions); a wave = 16 queries x 64 gallery items, K = channels in steps of 16.
template <class M>
__global__ void __launch_bounds__(kThreads)
corr_mfma_kernel(int channels, int nq_here, int ng, const unsigned char* __restrict__ q_block, unsigned q_item_bytes,
                 unsigned u_off, const unsigned char* __restrict__ pg, unsigned g_item_bytes, unsigned v_off,
                 float* __restrict__ x, int x_items) {
  const int tid = static_cast<int>(threadIdx.x);
  const int lane = tid & 63, wave = tid >> 6, i16 = lane & 15, kgrp = lane >> 4;
  const int cp = pad16(channels);
  const int p = static_cast<int>(blockIdx.y);
  const int g0 = static_cast<int>(blockIdx.x) * 64;
  const int q = wave * 16 + i16 < nq_here ? wave * 16 + i16 : nq_here - 1;
  const float* up = reinterpret_cast<const float*>(q_block + static_cast<size_t>(q) * q_item_bytes + u_off) +
                    static_cast<size_t>(p) * cp + 4 * kgrp;
  const float* vp[4];
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    const int gi = g0 + 16 * nt + i16 < ng ? g0 + 16 * nt + i16 : ng - 1;
    vp[nt] = reinterpret_cast<const float*>(pg + static_cast<size_t>(gi) * g_item_bytes + v_off) + static_cast<size_t>(p) * cp +
             4 * kgrp;
  }
  f32x4 acc[4];
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
  // the operands of the next k-step are requested before the MFMAs of this one (plain loop: load, wait, multiply - 8.5 ms
  // for config 3's gallery; so: 6.x)
  float4 a_next = *reinterpret_cast<const float4*>(up);
  float4 b_next[4];
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) b_next[nt] = *reinterpret_cast<const float4*>(vp[nt]);
  for (int c0 = 0; c0 < cp; c0 += 16) {
    const float4 a = a_next;
    float4 b[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) b[nt] = b_next[nt];
    const int cn = c0 + 16 < cp ? c0 + 16 : c0;  // (the last step re-reads its own operands)
    a_next = *reinterpret_cast<const float4*>(up + cn);
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) b_next[nt] = *reinterpret_cast<const float4*>(vp[nt] + cn);
    const float av[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
    for (int m = 0; m < 4; ++m) {
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const float bv = m == 0 ? b[nt].x : m == 1 ? b[nt].y : m == 2 ? b[nt].z : b[nt].w;
        acc[nt] = mfma_f32_16x16x4(av[m], bv, acc[nt]);
      }
    }
  }
  // lane owns rows (queries) 4 * kgrp .. + 3 of its wave's sixteen, column (gallery item) i16 of every tile
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    const int gl = g0 + 16 * nt + i16;
    if (gl < ng)
      *reinterpret_cast<float4*>(x + (static_cast<size_t>(p) * x_items + gl) * M::kXQ + wave * 16 + 4 * kgrp) =
          float4{acc[nt][0], acc[nt][1], acc[nt][2], acc[nt][3]};
  }
}

// ---- pair kernel: grid = (gallery items, blocks of 64 queries) ---------------------------------------------------------
// F32 (float32 maps; hi + lo on both sides, so neither EXACT nor F16): the prepared query holds two planes of template rows
// per channel, and the schedule below runs over 2 * channels PASSES - pass 2c: t_hi of channel c against both planes of its
// image, pass 2c + 1: t_lo against the hi plane, continuing the same accumulators.  "Channel" in the comments of the schedule
// then reads "pass"; the parity PAR of a period is the pass kind.  Only tiles that finish a lo pass are weighted.
// PEAKS (spr_ncc_score_peaks on a plan that asked for it, spr_ncc_plan_enable_peaks): the arg-max beside the max.  The channel
// loop is the plain form's; behind it every position travels with its value through the reduction and store_peak writes the
// three matrices (peak_yx, peak_tag: indexed like scores; the plain form never looks at the three trailing arguments).  Its
// own instantiation, in a translation unit of its own (ncc_mfma_peaks.hip).
template <class M, bool MAPS, bool EXACT, bool F16, bool F32 = false, bool PEAKS = false>
__global__ void __launch_bounds__(kThreads, 1)
pair_mfma_kernel(MfmaArgs g, const unsigned char* __restrict__ pq, const unsigned char* __restrict__ pg,
                 float* __restrict__ scores, float* __restrict__ maps_out, int32_t* __restrict__ peak_yx,
                 int32_t* __restrict__ peak_tag, int32_t tag) {
  static_assert(!(PEAKS && MAPS), "spr_ncc_maps has no peak form");
  unsigned char* lds = dyn_lds();
  const int tid = static_cast<int>(threadIdx.x);
  const int lane = tid & 63, wave = tid >> 6, col = lane & 15, kg = lane >> 4;
  const size_t gi = blockIdx.x;
  const int q0 = static_cast<int>(blockIdx.y) * 64;
  static_assert(!F32 || (!EXACT && !F16), "float32 maps: bfloat16 hi + lo, no correction matrix");
  constexpr int kQChan = (F32 ? 2 : 1) * M::kQMapBytes;  // template rows of one channel
  const int nq_here = g.nq - q0 < 64 ? g.nq - q0 : 64;
  const bool active = wave * 16 < nq_here;  // a wave without queries still stages the channel images

  // the borders of the padded map stay zero for every channel
  for (int i = tid; i < M::kLdsBytes / 16; i += kThreads) reinterpret_cast<float4*>(lds)[i] = float4{0.f, 0.f, 0.f, 0.f};

  // ---- gallery side: this lane stages pixels e0 = tid and e1 = tid + 256 of every channel ---------------------------
  const GalleryItem<M, const unsigned char> g_item{pg + gi * static_cast<size_t>(g.g_item_bytes), g.channels};
  const bool has1 = tid + kThreads < M::NPOS;
  const int e1 = has1 ? tid + kThreads : tid;
  float st_b[2], st_bs[2];
  unsigned st_hl[2];
  auto stage_load = [&](int c) {
    st_b[0] = g_item.b(c)[tid];    st_b[1] = g_item.b(c)[e1];
    st_bs[0] = g_item.bs(c)[tid];  st_bs[1] = g_item.bs(c)[e1];
    st_hl[0] = g_item.hl(c)[tid];  st_hl[1] = g_item.hl(c)[e1];
  };
  // low half: byte offset of the pixel in copy 0 (row, column); high half: its column in the padded map
  auto pixel_base = [&](int e) {
    const int iy = e / M::TW, ix = e - iy * M::TW;
    return ((iy + M::CY) * M::RS + 2 * (ix + M::CX)) | ((ix + M::CX) << 16);
  };
  const int pb0 = pixel_base(tid), pb1 = pixel_base(e1);
  // Branch-free on purpose: the channel loop below must stay ONE basic block, or the compiler sinks the epilogues of the
  // fragment steps before a branch into the block behind it, where they run with the matrix cores idle.  A copy that does
  // not hold the pixel stores to the buffer's dummy slot; a work-item without a second pixel stores its first one twice.
  // part k of 8: both pixels of this work-item into copy k (part 0 also the two epilogue weights); the parts go to different
  // fragment steps of the period - one burst of all 32 + 4 stores per wave holds up the fragment reads of all four waves
  auto stage_store_part = [&](unsigned char* buf, auto k_c) {
    constexpr int k = decltype(k_c)::value;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int pb = e ? pb1 : pb0;
      const unsigned hl = st_hl[e];
      const int w = pb >> 16, rowb = pb & 0xffff;
      const int mm = w - k;  // column of the pixel in copy k
      const int addr = k * 16 - 2 * k + rowb + (M::JS - 16) * (mm >> 3);
      const bool held = k <= M::CX || mm >= 0;  // w >= CX: only the far copies can push the first columns out
      *reinterpret_cast<uint16_t*>(buf + (held ? addr : M::kDummyOff)) = static_cast<uint16_t>(hl >> 16);
      if constexpr (!EXACT)
        *reinterpret_cast<uint16_t*>(buf + (held ? addr + M::HL : M::kDummyOff + 2)) = static_cast<uint16_t>(hl & 0xffffu);
    }
    if constexpr (k == 0) {  // the two epilogue weights of a pixel side by side: one 8-byte store here, one 8-byte read there
      f32x2* eb = reinterpret_cast<f32x2*>(buf + M::kEbOff);
      eb[tid] = f32x2{st_b[0], st_bs[0]};
      eb[e1] = f32x2{st_b[1], st_bs[1]};
    }
  };
  auto stage_store = [&](unsigned char* buf) {
    static_for<0, 8>([&](auto k_c) { stage_store_part(buf, k_c); });
  };

  // ---- query side --------------------------------------------------------------------------------------------------
  const unsigned char* q_block = pq + static_cast<size_t>(q0) * g.q_item_bytes;
  const BufRsrc q_rs = make_rsrc(q_block, static_cast<size_t>(nq_here) * g.q_item_bytes);
  auto clampq = [&](int q) { return q < nq_here ? q : nq_here - 1; };
  const unsigned a_off = static_cast<unsigned>(clampq(wave * 16 + col)) * g.q_item_bytes + static_cast<unsigned>(kg) * 16u;
  unsigned sc_off[4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
    sc_off[r] = static_cast<unsigned>(clampq(wave * 16 + 4 * kg + r)) * g.q_item_bytes +
                static_cast<unsigned>(g.channels) * kQChan;
  auto load_a = [&](int c, int ks) { return buf_ld16v(q_rs, a_off, static_cast<unsigned>(c) * M::kQMapBytes + ks * 64); };

  // fragment read addresses: tile phase ph covers positions 16*ph + col (+ 16*TP per tile group)
  int frag_base[M::TP];
#pragma unroll
  for (int ph = 0; ph < M::TP; ++ph) {
    const int p = 16 * ph + col, y = p / M::TW, x = p - y * M::TW;
    const int m0 = x + 8 * (kg & 1), k = m0 & 7;
    frag_base[ph] = k * 16 + (m0 >> 3) * M::JS + (y + (kg >> 1)) * M::RS;
  }

  // spr_ncc_maps: row and column of this lane's position in the first tile of a phase (tile group tg: DY * tg rows further down)
  int map_py[M::TP], map_px[M::TP];
#pragma unroll
  for (int ph = 0; ph < M::TP; ++ph) {
    map_py[ph] = (16 * ph + col) / M::TW;
    map_px[ph] = 16 * ph + col - map_py[ph] * M::TW;
  }
  auto mfma = [](u32x4 a, u32x4 b, f32x4 c) {
    if constexpr (F16) return mfma_f16_16x16x32(a, b, c);
    else return mfma_bf16_16x16x32(a, b, c);
  };
  // ---- steady-state schedule --------------------------------------------------------------------------------------
  // Time runs in row offsets tau = PERIOD * c + sigma (sigma = 0, 2, .. PERIOD - 2; three tile phases per step).  Tile group
  // tg works DY * tg behind the first one: at (c, sigma) it is at d = sigma - DY * tg of channel c if d >= 0, else at
  // d + PERIOD of channel c - 1 - so every step issues the same 2 * NTG MFMAs per phase, one tile in TP * DY / 2 steps is
  // finished and weighted, and the ramp-up / ramp-down of a channel-by-channel schedule (where a fragment read feeds one
  // or two MFMAs and the epilogues bunch at the end) is gone.  Channels c - 1 and c are both read from LDS while c + 1 is
  // staged (three buffers); the template fragments are double-buffered in registers (two periods unrolled), each reloaded
  // with channel c + 1 more than a channel before its first use.  The loop runs channels + 1 periods: in the first the
  // "previous channel" is all zeros (weights 0), in the last the "current" one is read but never weighted.
  f32x4 run[M::NTILE], acc[M::NTILE];
#pragma unroll
  for (int t = 0; t < M::NTILE; ++t) { run[t] = f32x4{0.f, 0.f, 0.f, 0.f}; acc[t] = f32x4{0.f, 0.f, 0.f, 0.f}; }
  u32x4 A[2][M::KS];
  const int last_c = g.channels - 1;
  const int passes = F32 ? 2 * g.channels : g.channels, last_p = passes - 1;  // periods of the schedule (+ 1 to drain)
  if (active) {
#pragma unroll
    for (int ks = 0; ks < M::KS; ++ks) {
      A[0][ks] = load_a(0, ks);
      A[1][ks] = u32x4{0u, 0u, 0u, 0u};
    }
    // (the first PERIOD - DY * (NTG - 1) offsets of a channel are done with before the previous period ends)
#pragma unroll
    for (int ks = 0; ks < (M::PERIOD - M::DY * (M::NTG - 1)) / 2; ++ks) A[1][ks] = load_a(last_p < 1 ? last_p : 1, ks);
  }
  stage_load(0);
  __syncthreads();  // the zero fill is complete
  stage_store(lds);
  stage_load(last_c < 1 ? last_c : 1);
  __syncthreads();

  constexpr int NIT = M::KS * M::TP;       // fragment steps per period
  constexpr int IT_STAGE = 4, kStageEvery = 2;  // channel c + 1 is written to LDS in eight parts, every other step from here
  static_assert(IT_STAGE + 7 * kStageEvery < NIT, "staging must end inside the period");
  f32x2 sc_cur[4], sc_prev[4], sc_ld[4], sc_ld2[4];  // {a, a * mean} of this lane's four queries, channels c and c - 1; in flight
#pragma unroll
  for (int r = 0; r < 4; ++r) sc_cur[r] = f32x2{0.f, 0.f};
  float ebv = 0.f, ebsv = 0.f;             // 1/sigma and S1/sigma of the tile whose epilogue is due
  int b_prev = 2 * M::kBufBytes, b_cur = 0, b_next = M::kBufBytes;  // byte offsets of the three channel buffers

  auto period = [&](auto par_c, int c) {
    constexpr int PAR = decltype(par_c)::value;
    unsigned char* buf_cur = lds + b_cur;
    // F32: both passes of a channel read ONE image - the lo pass has it as current and as previous, stages nothing, and the
    // buffers rotate (and the workgroup meets) once per channel, behind the lo pass
    constexpr bool kLoPass = F32 && PAR == 1, kHiPass = F32 && PAR == 0;
    unsigned char* buf_prev = lds + (kLoPass ? b_cur : b_prev);
    unsigned char* buf_next = lds + b_next;
    const int chan = F32 ? c >> 1 : c;  // the channel of pass c
    const int c1 = c + 1 < passes ? c + 1 : last_p, c2 = chan + 2 < g.channels ? chan + 2 : last_c;
    if (active) {
      if constexpr (kLoPass) {  // {a, a * mean} of this channel: due when its first tiles finish, at the end of this period
#pragma unroll
        for (int r = 0; r < 4; ++r) sc_ld[r] = buf_ld8(q_rs, sc_off[r], static_cast<unsigned>(chan) * 8u);
      }
#pragma unroll
      for (int r = 0; r < (F32 ? 0 : 4); ++r) {
        // (the loaded pair is first needed by the last steps of the period: its zeroing for the extra period waits until
        // mid-period - done here, the select made every period start with a full memory latency in front of its first MFMA)
        sc_prev[r] = sc_cur[r];
        if constexpr (PAR == 0) {  // (c is even here: one 16-byte load holds the pairs of channels c and c + 1)
          const u32x4 v = buf_ld16v(q_rs, sc_off[r], static_cast<unsigned>(c < g.channels ? c : (last_c & ~1)) * 8u);
          sc_ld[r] = f32x2{__uint_as_float(v[0]), __uint_as_float(v[1])};
          sc_ld2[r] = f32x2{__uint_as_float(v[2]), __uint_as_float(v[3])};
        } else {
          sc_ld[r] = sc_ld2[r];
        }
      }
      const f32x2* eb_cur = reinterpret_cast<const f32x2*>(buf_cur + M::kEbOff);
      const f32x2* eb_prev = reinterpret_cast<const f32x2*>(buf_prev + M::kEbOff);
      auto load_frag = [&](const unsigned char* buf, int ph, int s, int plane) {
        return *reinterpret_cast<const u32x4*>(buf + frag_base[ph] + s * M::RS + plane * M::HL);
      };
      // tile finished by fragment step `it` of a period: group 0 finishes the CURRENT channel in the last sigma step, group
      // tg > 0 the PREVIOUS channel at sigma = DY * tg - 2.  -1: none
      auto finished = [](int it) constexpr {
        const int sg = 2 * (it / M::TP), ph = it % M::TP;
        if (sg == M::PERIOD - 2) return ph;
        if ((sg + 2) % M::DY == 0 && (sg + 2) / M::DY >= 1 && (sg + 2) / M::DY < M::NTG) return ((sg + 2) / M::DY) * M::TP + ph;
        return -1;
      };
      auto epilogue = [&](int t, bool of_prev, int chan) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const f32x2 w = of_prev && !F32 ? sc_prev[r] : sc_cur[r];  // (F32: one channel's tiles at a time are weighted)
          const float v = ebv * acc[t][r];
          // (spr_ncc_maps passes no score matrix: the F32 instance of it keeps no channel sums - 84 registers it has no room for)
          if constexpr (!(F32 && MAPS)) run[t][r] = fmaf(-w.y, ebsv, fmaf(w.x, v, run[t][r]));
          if constexpr (MAPS) {  // spr_ncc_maps: the channel's own map of the first query
            if (r == 0 && wave == 0 && kg == 0 && chan >= 0 && chan < g.channels) {
              float m = fmaf(-w.y, ebsv, w.x * v);
              if constexpr (EXACT) {  // this channel's term of the contraction, for the one pair of spr_ncc_maps
                const int cp = pad16(g.channels), pos = 16 * t + col;
                const float* U = reinterpret_cast<const float*>(q_block + static_cast<size_t>(g.channels) * (kQChan + 8));
                const float* V = g_item.V();
                m -= U[static_cast<size_t>(pos) * cp + chan] * V[static_cast<size_t>(pos) * cp + chan];
              }
              const int py = M::DY * (t / M::TP) + map_py[t % M::TP], px = map_px[t % M::TP];
              if (py < g.ih && px < g.iw) maps_out[(chan * g.ih + py) * g.iw + px] = m;
            }
          }
        }
      };
      // fragment ring: the reads of step it + kAhead are issued before the MFMAs of step it (the scheduling fences keep
      // them there: left alone, the compiler sinks every read to just in front of its first use)
      constexpr int kAhead = SPR_MFMA_AHEAD, kRing = SPR_MFMA_AHEAD + 1;
      u32x4 fch[kRing], fcl[kRing], fph[kRing], fpl[kRing];
      auto issue = [&](auto j_c) {
        constexpr int j = decltype(j_c)::value;
        constexpr int sg = 2 * (j / M::TP), ph = j % M::TP, slot = j % kRing;
        if constexpr (!M::frag_zero(ph, sg)) {
          fch[slot] = load_frag(buf_cur, ph, sg, 0);
          if constexpr (!EXACT && !kLoPass) fcl[slot] = load_frag(buf_cur, ph, sg, 1);
        }
        if constexpr (sg + M::PERIOD <= M::SMAX && !M::frag_zero(ph, sg + M::PERIOD)) {
          fph[slot] = load_frag(buf_prev, ph, sg + M::PERIOD, 0);
          if constexpr (!EXACT && !kHiPass) fpl[slot] = load_frag(buf_prev, ph, sg + M::PERIOD, 1);  // (the previous pass is a lo pass)
        }
      };
      static_for<0, kAhead>(issue);
      static_for<0, NIT>([&](auto it_c) {
        constexpr int it = decltype(it_c)::value;
        constexpr int sg = 2 * (it / M::TP), ph = it % M::TP, slot = it % kRing;
        if constexpr (it + kAhead < NIT && (SPR_MFMA_ABL != 2 || it + kAhead < kRing)) issue(std::integral_constant<int, it + kAhead>{});
        // the tile finished by the previous step (its MFMAs have had time to drain) is weighted and added now; the two
        // weights of the tile this step finishes are requested for the next
        constexpr int tdone = finished((it + NIT - 1) % NIT);
        float eb_now = ebv, ebs_now = ebsv;
        (void)eb_now; (void)ebs_now;
        constexpr int tnext = finished(it);
        float nb = 0.f, nbs = 0.f;
        // F32: a tile of the current pass is weighted if that is a lo pass, one of the previous pass if this is a hi pass
        constexpr bool weigh_next = !F32 || (tnext < M::TP ? kLoPass : kHiPass);
        if constexpr (tnext >= 0 && weigh_next) {
          const f32x2 w = (tnext < M::TP ? eb_cur : eb_prev)[16 * tnext + col];
          nb = w.x;
          nbs = w.y;
        }
        sched_fence();
        if constexpr (tdone >= 0 && SPR_MFMA_ABL != 1) {
          // (group 0's last tile is finished by the last step of the PREVIOUS period: by now it belongs to channel c - 1)
          constexpr bool cur_chan = tdone < M::TP && it != 0;
          if constexpr (!F32) epilogue(tdone, !cur_chan, cur_chan ? c : c - 1);
          else if constexpr (cur_chan ? kLoPass : kHiPass) epilogue(tdone, false, cur_chan ? chan : chan - 1);
        }
        if constexpr (tnext >= 0 && weigh_next) { ebv = nb; ebsv = nbs; }
        if constexpr (it == NIT / 2) {
          static_assert(NIT / 2 < NIT - M::TP, "the current channel's weights are first used by the last sigma step");
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            if constexpr (!F32) sc_cur[r] = c < g.channels ? sc_ld[r] : f32x2{0.f, 0.f};
            else if constexpr (kLoPass) sc_cur[r] = sc_ld[r];  // (the tiles the previous channel had left are all weighted by now)
          }
        }
        if constexpr (SPR_MFMA_ABL != 3 && !kLoPass && it >= IT_STAGE && it < IT_STAGE + 8 * kStageEvery && (it - IT_STAGE) % kStageEvery == 0) {
          stage_store_part(buf_next, std::integral_constant<int, (it - IT_STAGE) / kStageEvery>{});
          if constexpr (it == IT_STAGE + 7 * kStageEvery) stage_load(c2);
        }
        static_for<0, M::NTG>([&](auto tg_c) {
          constexpr int tg = decltype(tg_c)::value;
          constexpr int d = sg - M::DY * tg;
          constexpr int t = tg * M::TP + ph;
          if constexpr (d >= 0) {
            constexpr int ks = d / 2;
            static_assert(M::first_ks(tg, ph) * 2 + M::DY * tg < M::PERIOD, "a tile starts in its own channel's period");
            if constexpr (!M::frag_zero(ph, sg)) {
              if constexpr (ks == M::first_ks(tg, ph) && !kLoPass)
                acc[t] = mfma(A[PAR][ks], fch[slot], f32x4{0.f, 0.f, 0.f, 0.f});
              else
                acc[t] = mfma(A[PAR][ks], fch[slot], acc[t]);
              if constexpr (!EXACT && !kLoPass) acc[t] = mfma(A[PAR][ks], fcl[slot], acc[t]);
            }
          } else if constexpr (!M::frag_zero(ph, sg + M::PERIOD)) {
            constexpr int ks = (d + M::PERIOD) / 2;
            acc[t] = mfma(A[PAR ^ 1][ks], fph[slot], acc[t]);
            if constexpr (!EXACT && !kHiPass) acc[t] = mfma(A[PAR ^ 1][ks], fpl[slot], acc[t]);
          }
        });
        // template row pairs nobody needs any more: the previous channel's (the slowest group has just used it) is
        // replaced by channel c + 1's, and at the end of the period the first ones of this channel by channel c + 2's
        // All of them go to the other buffer: its first (PERIOD - lag) / 2 row pairs hold channel c - 1's, which no tile
        // group reads in this period (the slowest one is at k-step (PERIOD - lag) / 2 when the period starts) - they are
        // reloaded in the FIRST steps.  Nothing is requested in the last steps of a period: the memory counter is in order,
        // so the first wait of the next period (for the staged pixels, requested half a period earlier) would sit out the
        // latency of a load requested just before it.
        if constexpr (SPR_MFMA_ABL != 4) {
          constexpr int lag = M::DY * (M::NTG - 1);
          constexpr int kFree = (M::PERIOD - lag) / 2;
          if constexpr (ph == M::TP - 1 && sg + M::PERIOD - lag < M::PERIOD) {
            constexpr int ks = (sg + M::PERIOD - lag) / 2;
            A[PAR ^ 1][ks] = load_a(c1, ks);
          } else if constexpr (ph == 0 && sg / 2 < kFree) {
            A[PAR ^ 1][sg / 2] = load_a(c1, sg / 2);
          }
        }
#if SPR_MFMA_GROUPS
        // the step's vector instructions (epilogue, staging addresses) in groups behind one MFMA each, not in one run
        static_for<0, M::NTG>([&](auto) {
          sched_group<0x8, 1>();
          sched_group<0x2, SPR_MFMA_GROUPS>();
        });
#endif
        sched_fence();
      });
    } else if constexpr (!kLoPass) {
      stage_store(buf_next);
      stage_load(c2);
    }
    if constexpr (!kHiPass) {
      if (SPR_MFMA_ABL != 5) __syncthreads();  // channel c + 1 is staged; nobody reads channel c - 1's image any more
      const int t0 = b_prev;
      b_prev = b_cur; b_cur = b_next; b_next = t0;
    }
  };
  for (int c = 0; c <= passes; c += 2) {
    period(std::integral_constant<int, 0>{}, c);
    if (c + 1 <= passes) period(std::integral_constant<int, 1>{}, c + 1);
  }
  // group 0's last tile of the last period is still to be weighted - with weight 0 (it belongs to "channel" channels)

  if (!active || !scores || (F32 && MAPS)) return;  // spr_ncc_maps passes no score matrix
  // spatial maximum per query: over this lane's tiles, then over the sixteen lanes holding the other positions
  if constexpr (EXACT) {
#pragma unroll
    for (int t = 0; t < M::NTILE; ++t) {
      const float4 xv = *reinterpret_cast<const float4*>(g.x + (static_cast<size_t>(16 * t + col) * g.x_items + gi) * M::kXQ +
                                                         wave * 16 + 4 * kg);
      run[t][0] -= xv.x; run[t][1] -= xv.y; run[t][2] -= xv.z; run[t][3] -= xv.w;
    }
  }
  if constexpr (PEAKS) {
    // tile t, lane column col = frame position (DY * (t / TP) + map_py, map_px) - the mapping of the maps branch.  A spare
    // position of the frame (outside the ih x iw map: channel sum 0) keeps its value, so that the maximum is the plain
    // form's bit for bit, but names no pixel: kNoPeak loses every tie against a real position.
    int where_t[M::NTILE];
#pragma unroll
    for (int t = 0; t < M::NTILE; ++t) {
      const int py = M::DY * (t / M::TP) + map_py[t % M::TP], px = map_px[t % M::TP];
      where_t[t] = py < g.ih && px < g.iw ? (py << 16) | px : kNoPeak;
    }
    float best[4];
    int where[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      best[r] = run[0][r];
      where[r] = where_t[0];
#pragma unroll
      for (int t = 1; t < M::NTILE; ++t) peak_take(best[r], where[r], run[t][r], where_t[t]);
      for (int m = 8; m >= 1; m >>= 1) {
        const float ov = shfl_xor(best[r], m);
        const int op = shfl_xor(where[r], m);
        peak_take(best[r], where[r], ov, op);
      }
    }
    if (col == 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int q = wave * 16 + 4 * kg + r;
        if (q < nq_here)
          store_peak(scores, peak_yx, peak_tag, static_cast<size_t>(q0 + q) * g.ld + g.col0 + gi,
                     best[r] / static_cast<float>(g.channels), where[r], tag, g.accumulate);
      }
    }
    return;
  }
  float best[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    best[r] = run[0][r];
#pragma unroll
    for (int t = 1; t < M::NTILE; ++t) best[r] = fmaxf(best[r], run[t][r]);
    for (int m = 8; m >= 1; m >>= 1) best[r] = fmaxf(best[r], shfl_xor(best[r], m));
  }
  if (col == 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int q = wave * 16 + 4 * kg + r;
      if (q < nq_here) {
        const float s = best[r] / static_cast<float>(g.channels);
        float* dst = scores + static_cast<size_t>(q0 + q) * g.ld + g.col0 + gi;
        const float prev = g.accumulate ? *dst : 0.0f;
        *dst = s > prev ? s : prev;  // similarity.py:355, 366-367: zero-initialised running maximum
      }
    }
  }
}

using M2812 = MCfg<28, 12>;         // template = map = 28 x 12 (BASELINE config 3 / conv5_3 of config 5)
using MGEN = MCfg<28, 12, 30, 8>;    // any template up to 30 x 16 on any map up to 28 x 12
static_assert(MGEN::kMaxTh == 30 && MGEN::kMaxTw == 16, "general instance");

bool mfma_tuned_shape(const NccGeom& g) {
  return g.th == M2812::TH && g.tw == M2812::TW && g.ih == M2812::TH && g.iw == M2812::TW;
}
bool mfma_frame_ok(const NccGeom& g) {  // the sizes either instance covers, whatever the storage type
  if (mfma_tuned_shape(g)) return true;
  return g.th >= 1 && g.tw >= 1 && g.ih >= 1 && g.iw >= 1 && g.th <= MGEN::kMaxTh && g.tw <= MGEN::kMaxTw && g.ih <= MGEN::TH &&
         g.iw <= MGEN::TW;
}
bool mfma_shape_ok(const NccGeom& g) { return (g.dtype == SPR_BF16 || g.dtype == SPR_F16) && mfma_frame_ok(g); }

// the instance of a plan: f(M2812{}) or f(MGEN{})
template <class F>
auto with_instance(const NccGeom& g, F&& f) {
  return g.mfma_general ? f(MGEN{}) : f(M2812{});
}

}  // namespace

constexpr int kCorrItems = 1024;  // gallery items per launch of the exact form = what the plan's correction matrix holds

// One scoring call on the pair kernel of (instance, form).  PEAKS: spr_ncc_score_peaks - the same slices of the gallery and
// blocks of queries, the peak kernel in place of the plain one, the three matrices offset alike.
template <class M, bool EXACT, bool F16, bool F32, bool PEAKS>
static int launch_pair_mfma_t(const NccGeom& g, const PlanScratch& s, const PairCall& c) {
  const bool maps = !PEAKS && c.maps_out;
  // (a translation unit names the kernels of its own form only: the other form's are not instantiated in it)
  auto pick = [&] {
    if constexpr (PEAKS) return pair_mfma_kernel<M, false, EXACT, F16, F32, true>;
    else return maps ? pair_mfma_kernel<M, true, EXACT, F16, F32> : pair_mfma_kernel<M, false, EXACT, F16, F32>;
  };
  auto kernel = pick();
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kLdsLimit);
  // one launch; `at`: the first entry of scores (peak_yx, peak_tag) the launch's queries own
  auto launch = [&](dim3 grid, const MfmaArgs& a, const unsigned char* q, const unsigned char* gal, size_t at) {
    hipLaunchKernelGGL(kernel, grid, dim3(kThreads), M::kLdsBytes, c.stream, a, q, gal, c.scores ? c.scores + at : nullptr,
                       PEAKS ? nullptr : c.maps_out, PEAKS ? c.peak_yx + at : nullptr,
                       PEAKS && c.peak_tag ? c.peak_tag + at : nullptr, c.tag);
    return check_launch("pair_mfma_kernel");
  };
  const size_t q_item = mfma_query_item_bytes(g), g_item = mfma_gallery_item_bytes(g);
  const unsigned char* pqb = static_cast<const unsigned char*>(c.pq);
  const unsigned char* pgb = static_cast<const unsigned char*>(c.pg);
  if (!EXACT || maps) {
    const unsigned q_blocks = static_cast<unsigned>((c.nq + 63) / 64);
    // HIP refuses a grid of 2^32 work-items or more: slices of the gallery
    int64_t max_g = pair_tiles_per_launch(1, kThreads) / q_blocks;
    if (max_g < 1) max_g = 1;
    for (int64_t g0 = 0; g0 < c.ng; g0 += max_g) {
      const int64_t n = c.ng - g0 < max_g ? c.ng - g0 : max_g;
      MfmaArgs a{g.channels, static_cast<int>(c.nq), static_cast<int>(n), static_cast<long long>(c.ld),
                 static_cast<long long>(c.col0 + g0), c.accumulate, static_cast<unsigned>(q_item),
                 static_cast<unsigned>(g_item), nullptr, 0, g.ih, g.iw};
      const int rc = launch(dim3(static_cast<unsigned>(n), q_blocks), a, pqb, pgb + static_cast<size_t>(g0) * g_item, 0);
      if (rc != SPR_OK) return rc;
    }
    return SPR_OK;
  }
  // exact form: per block of 64 queries and slice of the gallery, the correction matrix first, then the pairs
  float* xws = s.mfma_x;
  if (!xws) { set_error("pair_mfma_kernel: the exact form needs the plan's correction matrix"); return SPR_ERR_ARG; }
  int64_t max_g = pair_tiles_per_launch(1, kThreads);
  if (max_g > kCorrItems) max_g = kCorrItems;
  const unsigned u_off = static_cast<unsigned>(static_cast<size_t>(g.channels) * (M::kQMapBytes + 8));
  const unsigned v_off = static_cast<unsigned>(static_cast<size_t>(g.channels) * M::kGChanBytes);
  for (int64_t q0 = 0; q0 < c.nq; q0 += 64) {
    const int nq_here = static_cast<int>(c.nq - q0 < 64 ? c.nq - q0 : 64);
    for (int64_t g0 = 0; g0 < c.ng; g0 += max_g) {
      const int n = static_cast<int>(c.ng - g0 < max_g ? c.ng - g0 : max_g);
      hipLaunchKernelGGL(HIP_KERNEL_NAME(corr_mfma_kernel<M>), dim3((n + 63) / 64, M::NPOS), dim3(kThreads), 0, c.stream,
                         g.channels, nq_here, n, pqb + static_cast<size_t>(q0) * q_item, static_cast<unsigned>(q_item), u_off,
                         pgb + static_cast<size_t>(g0) * g_item, static_cast<unsigned>(g_item), v_off, xws, n);
      int rc = check_launch("corr_mfma_kernel");
      if (rc != SPR_OK) return rc;
      MfmaArgs a{g.channels, nq_here, n, static_cast<long long>(c.ld), static_cast<long long>(c.col0 + g0), c.accumulate,
                 static_cast<unsigned>(q_item), static_cast<unsigned>(g_item), xws, n, g.ih, g.iw};
      rc = launch(dim3(static_cast<unsigned>(n), 1), a, pqb + static_cast<size_t>(q0) * q_item,
                  pgb + static_cast<size_t>(g0) * g_item, static_cast<size_t>(q0) * c.ld);
      if (rc != SPR_OK) return rc;
    }
  }
  return SPR_OK;
}

// the instance and form of a plan, plain (ncc_mfma.hip) or PEAKS (ncc_mfma_peaks.hip): each file instantiates one of the two
template <bool PEAKS>
static int launch_pair_mfma_form(const NccGeom& g, const PlanScratch& s, const PairCall& c) {
  if (c.nq == 0 || c.ng == 0) return SPR_OK;
  return with_instance(g, [&](auto m) {
    using M = decltype(m);
    if (g.mfma_f32) return launch_pair_mfma_t<M, false, false, true, PEAKS>(g, s, c);
    if (g.dtype == SPR_F16) return launch_pair_mfma_t<M, true, true, false, PEAKS>(g, s, c);
    return g.mfma_exact ? launch_pair_mfma_t<M, true, false, false, PEAKS>(g, s, c)
                        : launch_pair_mfma_t<M, false, false, false, PEAKS>(g, s, c);
  });
}

}  // namespace spr
