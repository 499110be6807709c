// Shortlist retrieval: the k best items of every score row, and the peak of a pair's channel-summed NCC maps.
//
// spr_topk_rows writes the items of a row in the ranker's order (rank.hip): a before b iff s_a > s_b, or s_a == s_b and
// idx_a > idx_b, so the item at position p (1-based) is the item spr_rank_true_match ranks p.  An item is one 64-bit key
// (order-preserving image of the score in the high word, the item index in the low word): indices are unique within a row,
// so keys are, and position p holds the largest key below the key of position p - 1.  One workgroup per row makes k
// selection passes over the row (L2-resident: 4 bytes per item, 8 with an index list); nothing is written but the result.
//
// spr_maps_peak sums the per-channel maps of spr_ncc_maps in float64, channel 0 first - a fixed order: the result is
// bit-reproducible - and reduces the summed map to its first maximum in row-major order.  A work-item owns its pixels and
// walks the channels, so the loads of a wave are coalesced across pixels.  HBM-bound: 4 bytes per map value.
// spr_maps_mean is the same sum with every pixel kept: the channel-mean map of a pair whose plan has no surfaces form.
//
// spr_surface_peaks reads a channel-mean map (spr_ncc_score_surfaces, spr_maps_mean) the way an examiner does: its n best
// peaks, each outside the windows of the ones before it, and the peak-to-sidelobe ratio of the first.  One workgroup per
// surface, one pass over it per peak and two for the ratio; a surface is tens of KB and stays in L2.
#include "spr_common.h"

namespace spr {
namespace {

// Workgroups per launch: rows / pairs beyond it are walked by a grid-stride loop (SPR_TOPK_MAX_GRID lowers it: tests).
int topk_grid(int64_t n) {
  const int cap = env_int("SPR_TOPK_MAX_GRID", 0);
  const int64_t limit = cap >= 1 && cap < 65535 ? cap : 65535;
  return static_cast<int>(n < limit ? n : limit);
}

// float -> unsigned with the order of the floats (finite by contract); both zeros map to one value: rank_kernel compares
// with the float ==, under which -0.0 and +0.0 tie.  No finite float maps to 0.
__device__ __forceinline__ unsigned ordered_bits(float s) {
  const unsigned u = s == 0.0f ? 0u : __float_as_uint(s);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

struct Cand {
  unsigned long long key;  // 0: no item
  int col;                 // column of the row the key came from (its score is re-read there: the sign of a zero survives)
};

__device__ __forceinline__ Cand better(Cand a, Cand b) { return b.key > a.key ? b : a; }

// The largest candidate of the workgroup, in every work-item.  A key moves as two 32-bit halves.
__device__ __forceinline__ Cand block_best(Cand c, int* scratch) {
  for (int m = 32; m >= 1; m >>= 1) {
    Cand o;
    const int hi = shfl_xor(static_cast<int>(c.key >> 32), m);
    const int lo = shfl_xor(static_cast<int>(c.key & 0xffffffffull), m);
    o.key = (static_cast<unsigned long long>(static_cast<unsigned>(hi)) << 32) | static_cast<unsigned>(lo);
    o.col = shfl_xor(c.col, m);
    c = better(c, o);
  }
  const int tid = static_cast<int>(threadIdx.x);
  __syncthreads();  // scratch may still be read by the previous pass
  if ((tid & 63) == 0) {
    scratch[3 * (tid >> 6)] = static_cast<int>(c.key >> 32);
    scratch[3 * (tid >> 6) + 1] = static_cast<int>(c.key & 0xffffffffull);
    scratch[3 * (tid >> 6) + 2] = c.col;
  }
  __syncthreads();
  Cand best{0ull, -1};
  for (int w = 0; w < kThreads / 64; ++w) {
    Cand o;
    o.key = (static_cast<unsigned long long>(static_cast<unsigned>(scratch[3 * w])) << 32) | static_cast<unsigned>(scratch[3 * w + 1]);
    o.col = scratch[3 * w + 2];
    best = better(best, o);
  }
  return best;
}

__global__ void __launch_bounds__(kThreads)
topk_rows_kernel(const float* __restrict__ scores, long long ld, long long n_queries, long long n_cols,
                 const int* __restrict__ col_index, long long global_col0, int k, float* __restrict__ out_scores,
                 int* __restrict__ out_index) {
  __shared__ int scratch[3 * (kThreads / 64)];
  const int tid = static_cast<int>(threadIdx.x);
  for (long long q = blockIdx.x; q < n_queries; q += gridDim.x) {  // (workgroup-uniform: the barriers inside are too)
    const float* row = scores + q * ld;
    const int* idx_row = col_index ? col_index + q * ld : nullptr;
    unsigned long long last = ~0ull;  // above every key
    int p = 0;
    for (; p < k; ++p) {
      Cand mine{0ull, -1};
      for (long long j = tid; j < n_cols; j += kThreads) {
        const int idx = idx_row ? idx_row[j] : static_cast<int>(global_col0 + j);
        if (idx < 0) continue;  // an empty slot of a gathered candidate list
        const unsigned long long key = (static_cast<unsigned long long>(ordered_bits(row[j])) << 32) | static_cast<unsigned>(idx);
        if (key < last && key > mine.key) mine = Cand{key, static_cast<int>(j)};
      }
      const Cand best = block_best(mine, scratch);
      if (best.key == 0ull) break;  // the row has no item left (the same in every work-item)
      if (tid == 0) {
        out_scores[q * k + p] = row[best.col];
        out_index[q * k + p] = static_cast<int>(best.key & 0xffffffffull);
      }
      last = best.key;
    }
    for (int e = p + tid; e < k; e += kThreads) {  // empty slots
      out_scores[q * k + e] = 0.0f;
      out_index[q * k + e] = -1;
    }
  }
}

__global__ void __launch_bounds__(kThreads)
maps_peak_kernel(const float* __restrict__ maps, long long n_pairs, int channels, int pixels, int w,
                 float* __restrict__ out_score, int* __restrict__ out_yx) {
  __shared__ double s_val[kThreads / 64];
  __shared__ int s_pix[kThreads / 64];
  const int tid = static_cast<int>(threadIdx.x);
  for (long long p = blockIdx.x; p < n_pairs; p += gridDim.x) {
    const float* pair = maps + static_cast<size_t>(p) * channels * pixels;
    double best = -INFINITY;  // a work-item without a pixel never wins: every sum is finite
    int best_pix = 0x7fffffff;
    for (int i = tid; i < pixels; i += kThreads) {
      const float* px = pair + i;
      double acc = 0.0;
      int c = 0;
      for (; c + 8 <= channels; c += 8) {  // eight loads in flight, added in channel order
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = px[static_cast<size_t>(c + u) * pixels];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += static_cast<double>(v[u]);
      }
      for (; c < channels; ++c) acc += static_cast<double>(px[static_cast<size_t>(c) * pixels]);
      if (acc > best) {  // pixels ascend within a work-item: the first maximum stays
        best = acc;
        best_pix = i;
      }
    }
    for (int m = 32; m >= 1; m >>= 1) {
      const double ov = shfl_xor(best, m);
      const int op = shfl_xor(best_pix, m);
      if (ov > best || (ov == best && op < best_pix)) {
        best = ov;
        best_pix = op;
      }
    }
    __syncthreads();  // the scratch of the previous pair may still be read
    if ((tid & 63) == 0) {
      s_val[tid >> 6] = best;
      s_pix[tid >> 6] = best_pix;
    }
    __syncthreads();
    if (tid == 0) {
      for (int wv = 1; wv < kThreads / 64; ++wv)
        if (s_val[wv] > best || (s_val[wv] == best && s_pix[wv] < best_pix)) {
          best = s_val[wv];
          best_pix = s_pix[wv];
        }
      if (best_pix >= pixels) best_pix = 0;  // no finite sum anywhere (outside the contract): the position stays inside the map
      out_score[p] = static_cast<float>(best / channels);
      out_yx[2 * p] = best_pix / w;
      out_yx[2 * p + 1] = best_pix % w;
    }
  }
}

// the float64 channel sum of maps_peak_kernel, every pixel kept: out = (float)(acc / channels)
__global__ void __launch_bounds__(kThreads)
maps_mean_kernel(const float* __restrict__ maps, long long n_pairs, int channels, int pixels, float* __restrict__ out) {
  const int tid = static_cast<int>(threadIdx.x);
  for (long long p = blockIdx.x; p < n_pairs; p += gridDim.x) {
    const float* pair = maps + static_cast<size_t>(p) * channels * pixels;
    float* dst = out + static_cast<size_t>(p) * pixels;
    for (int i = tid; i < pixels; i += kThreads) {
      const float* px = pair + i;
      double acc = 0.0;
      int c = 0;
      for (; c + 8 <= channels; c += 8) {  // eight loads in flight, added in channel order
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = px[static_cast<size_t>(c + u) * pixels];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += static_cast<double>(v[u]);
      }
      for (; c < channels; ++c) acc += static_cast<double>(px[static_cast<size_t>(c) * pixels]);
      dst[i] = static_cast<float>(acc / channels);
    }
  }
}

constexpr int kMaxSurfacePeaks = 8;

__global__ void __launch_bounds__(kThreads)
surface_peaks_kernel(const float* __restrict__ surfaces, long long n, int h, int w, int n_peaks, int ry, int rx,
                     float* __restrict__ out_value, int* __restrict__ out_yx, float* __restrict__ out_psr) {
  __shared__ float red[2 * (kThreads / 64)];
  __shared__ double dred[kThreads / 64];
  const int tid = static_cast<int>(threadIdx.x);
  const int pixels = h * w;
  for (long long p = blockIdx.x; p < n; p += gridDim.x) {  // (workgroup-uniform: the barriers inside are too)
    const float* s = surfaces + static_cast<size_t>(p) * pixels;
    int py[kMaxSurfacePeaks], px[kMaxSurfacePeaks];  // the peaks so far: the same in every work-item (registers: the loop
    float v0 = 0.0f;                                 // over the peaks is unrolled)
    int found = 0;
#pragma unroll
    for (int j = 0; j < kMaxSurfacePeaks; ++j) {
      if (j >= n_peaks) break;
      float best = -INFINITY;  // with kNoPeak: loses against every pixel (values are finite)
      int where = kNoPeak;
      for (int i = tid; i < pixels; i += kThreads) {
        const int y = i / w, x = i - y * w;
        bool open = true;
#pragma unroll
        for (int k = 0; k < j; ++k) open = open && (abs(y - py[k]) > ry || abs(x - px[k]) > rx);
        if (open) peak_take(best, where, s[i], (y << 16) | x);
      }
      block_peak(best, where, red);
      if (where == kNoPeak) break;  // no pixel is left (the same in every work-item)
      if (tid == 0) {
        out_value[p * n_peaks + j] = best;
        out_yx[p * n_peaks + j] = where;
      }
      py[j] = where >> 16;
      px[j] = where & 0xffff;
      if (j == 0) v0 = best;
      found = j + 1;
    }
    for (int e = found + tid; e < n_peaks; e += kThreads) {  // empty slots
      out_value[p * n_peaks + e] = 0.0f;
      out_yx[p * n_peaks + e] = -1;
    }
    if (!out_psr) continue;
    // peak-to-sidelobe ratio of peak 0 over the pixels outside its window, float64, two passes: the mean, then the squares
    const int y_lo = py[0] - ry > 0 ? py[0] - ry : 0, y_hi = py[0] + ry < h - 1 ? py[0] + ry : h - 1;  // (ry, rx <= 32767:
    const int x_lo = px[0] - rx > 0 ? px[0] - rx : 0, x_hi = px[0] + rx < w - 1 ? px[0] + rx : w - 1;  //  the launcher clamps)
    auto outside = [&](int i) {
      const int y = i / w, x = i - y * w;
      return y < y_lo || y > y_hi || x < x_lo || x > x_hi;
    };
    const int count = pixels - (y_hi - y_lo + 1) * (x_hi - x_lo + 1);
    double sum = 0.0;
    for (int i = tid; i < pixels; i += kThreads)
      if (outside(i)) sum += static_cast<double>(s[i]);
    sum = block_sum(sum, dred);
    const double mu = count > 0 ? sum / count : 0.0;
    double sq = 0.0;
    for (int i = tid; i < pixels; i += kThreads) {
      const double d = static_cast<double>(s[i]) - mu;
      if (outside(i)) sq += d * d;
    }
    sq = block_sum(sq, dred);
    if (tid == 0) {
      const double sigma = count > 0 ? sqrt(sq / count) : 0.0;
      out_psr[p] = count < 2 || sigma == 0.0 ? 0.0f : static_cast<float>((static_cast<double>(v0) - mu) / sigma);
    }
  }
}

}  // namespace
}  // namespace spr

extern "C" int spr_topk_rows(const float* scores, int64_t ld, int64_t n_queries, int64_t n_cols, const int32_t* col_index,
                             int64_t global_col0, int32_t k, float* out_scores, int32_t* out_index, spr_stream_t stream) {
  using namespace spr;
  if (n_queries < 0 || n_cols < 0 || ld < n_cols) { set_error("spr_topk_rows: bad sizes"); return SPR_ERR_ARG; }
  if (k < 1 || k > 256) { set_error("spr_topk_rows: k = %d outside [1, 256]", k); return SPR_ERR_ARG; }
  // item indices and columns are int32
  if (global_col0 < 0 || n_cols > 0x7fffffffLL || global_col0 + n_cols > 0x7fffffffLL) {
    set_error("spr_topk_rows: item indices beyond int32");
    return SPR_ERR_ARG;
  }
  if (n_queries == 0) return SPR_OK;
  if ((!scores && n_cols > 0) || !out_scores || !out_index) { set_error("spr_topk_rows: null pointer"); return SPR_ERR_ARG; }
  hipLaunchKernelGGL(topk_rows_kernel, dim3(static_cast<unsigned>(topk_grid(n_queries))), dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream), scores, static_cast<long long>(ld), static_cast<long long>(n_queries),
                     static_cast<long long>(n_cols), col_index, static_cast<long long>(global_col0), static_cast<int>(k),
                     out_scores, out_index);
  return check_launch("topk_rows_kernel");
}

extern "C" int spr_maps_peak(const float* maps, int64_t n_pairs, int32_t channels, int32_t h, int32_t w, float* out_score,
                             int32_t* out_yx, spr_stream_t stream) {
  using namespace spr;
  if (n_pairs < 0 || channels < 1 || h < 1 || w < 1) { set_error("spr_maps_peak: bad sizes"); return SPR_ERR_ARG; }
  if (static_cast<int64_t>(h) * w > 0x7fffffffLL - kThreads) { set_error("spr_maps_peak: map beyond int32 pixels"); return SPR_ERR_ARG; }
  if (n_pairs == 0) return SPR_OK;
  if (!maps || !out_score || !out_yx) { set_error("spr_maps_peak: null pointer"); return SPR_ERR_ARG; }
  hipLaunchKernelGGL(maps_peak_kernel, dim3(static_cast<unsigned>(topk_grid(n_pairs))), dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream), maps, static_cast<long long>(n_pairs), static_cast<int>(channels),
                     static_cast<int>(h * w), static_cast<int>(w), out_score, out_yx);
  return check_launch("maps_peak_kernel");
}

extern "C" int spr_maps_mean(const float* maps, int64_t n_pairs, int32_t channels, int32_t h, int32_t w, float* out,
                             spr_stream_t stream) {
  using namespace spr;
  if (n_pairs < 0 || channels < 1 || h < 1 || w < 1) { set_error("spr_maps_mean: bad sizes"); return SPR_ERR_ARG; }
  if (static_cast<int64_t>(h) * w > 0x7fffffffLL - kThreads) { set_error("spr_maps_mean: map beyond int32 pixels"); return SPR_ERR_ARG; }
  if (n_pairs == 0) return SPR_OK;
  if (!maps || !out) { set_error("spr_maps_mean: null pointer"); return SPR_ERR_ARG; }
  hipLaunchKernelGGL(maps_mean_kernel, dim3(static_cast<unsigned>(topk_grid(n_pairs))), dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream), maps, static_cast<long long>(n_pairs), static_cast<int>(channels),
                     static_cast<int>(h * w), out);
  return check_launch("maps_mean_kernel");
}

extern "C" int spr_surface_peaks(const float* surfaces, int64_t n, int32_t h, int32_t w, int32_t n_peaks, int32_t ry, int32_t rx,
                                 float* out_value, int32_t* out_yx, float* out_psr, spr_stream_t stream) {
  using namespace spr;
  if (n < 0 || h < 1 || w < 1 || h > 32767 || w > 32767) { set_error("spr_surface_peaks: bad sizes"); return SPR_ERR_ARG; }
  if (n_peaks < 1 || n_peaks > kMaxSurfacePeaks || ry < 0 || rx < 0) {
    set_error("spr_surface_peaks: n_peaks = %d outside [1, %d] or a negative window", n_peaks, kMaxSurfacePeaks);
    return SPR_ERR_ARG;
  }
  if (n == 0) return SPR_OK;
  if (!surfaces || !out_value || !out_yx) { set_error("spr_surface_peaks: null pointer"); return SPR_ERR_ARG; }
  hipLaunchKernelGGL(surface_peaks_kernel, dim3(static_cast<unsigned>(topk_grid(n))), dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream), surfaces, static_cast<long long>(n), static_cast<int>(h),
                     static_cast<int>(w), static_cast<int>(n_peaks), static_cast<int>(ry < 32767 ? ry : 32767),  // (a window
                     static_cast<int>(rx < 32767 ? rx : 32767), out_value, out_yx,  // beyond the largest surface covers all of it)
                     out_psr);
  return check_launch("surface_peaks_kernel");
}
