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
