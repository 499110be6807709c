// Device-resident feature sets (features.py): the two data movers that let ragged item sets stay in HBM between the
// extractor and the ranks.
//
// items_gather_kernel: item k of dst = item index[k] of src, converted to the storage type - the query-class stack and the
//   gallery-chunk stack of NccScorer._blocks with the cast fused in.  Bandwidth kernel: every work-item moves 16-byte
//   vectors of the DESTINATION (4 float32 or 8 16-bit values), so the stores are always full dwordx4; the loads are dwordx4
//   too when the source item happens to share that phase (always the case for float32 -> float32 of items whose size is a
//   multiple of 4 floats, the feature maps of every extractor here), and fall back to dword loads otherwise (a source whose
//   phase differs from the destination's cannot be read in aligned 16-byte pieces without a shift network; the loads stay
//   coalesced, 32 / 16 contiguous bytes per lane).  The elements in front of the first and behind the last aligned vector
//   of an item (at most 7 + 7) go one by one.
// block_scatter_kernel: dst[rows[i], cols[j]] = src[i, j] or max(dst, src): the fold of one block of the walk into the
//   [Q, G] matrices.  Element-granular by nature (the columns of a chunk are not contiguous in a ragged gallery); reads of
//   src / cols are coalesced, a block is Q x chunk values.
#include "spr_common.h"

namespace spr {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
static_assert(sizeof(u32x4) == 16, "u32x4 must be 16 bytes");

constexpr int kGatherUnroll = 4;                       // 16-byte vectors per work-item and tile
constexpr int kGatherTileVecs = kThreads * kGatherUnroll;
constexpr long long kGatherMaxBlocks = 4096;           // grid-stride beyond (256 CUs x 16)

__device__ __forceinline__ float bits_f32(uint32_t u) {
  union { uint32_t u; float f; } c;
  c.u = u;
  return c.f;
}

template <int DT>
__device__ __forceinline__ uint16_t to16(float v) { return round16<DT>(v); }

// One destination vector from its source values.  ALIGNED: the source address is a multiple of 16 bytes.
template <int DT, bool ALIGNED>
__device__ __forceinline__ u32x4 gather_vec(const uint32_t* __restrict__ w) {  // (words: float32 -> float32 moves bits only)
  constexpr int V = DT == SPR_F32 ? 4 : 8;
  uint32_t v[V];
  if (ALIGNED) {
#pragma unroll
    for (int k = 0; k < V / 4; ++k) {
      const u32x4 raw = reinterpret_cast<const u32x4*>(w)[k];
#pragma unroll
      for (int e = 0; e < 4; ++e) v[4 * k + e] = raw[e];
    }
  } else {
#pragma unroll
    for (int e = 0; e < V; ++e) v[e] = w[e];
  }
  u32x4 out;
  if (DT == SPR_F32) {
#pragma unroll
    for (int e = 0; e < 4; ++e) out[e] = v[e];
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      out[e] = static_cast<uint32_t>(to16<DT>(bits_f32(v[2 * e]))) | (static_cast<uint32_t>(to16<DT>(bits_f32(v[2 * e + 1]))) << 16);
  }
  return out;
}

template <int DT>
__device__ __forceinline__ void gather_one(const uint32_t* __restrict__ s, void* __restrict__ d, long long e) {
  const uint32_t word = s[e];
  if (DT == SPR_F32) {
    static_cast<uint32_t*>(d)[e] = word;  // (bits, not values: a NaN keeps its payload, any 4-byte item may travel)
  } else {
    static_cast<uint16_t*>(d)[e] = to16<DT>(bits_f32(word));
  }
}

// Tiles of kGatherTileVecs destination vectors; tile 0 of an item also moves the item's unaligned head and tail.
template <int DT>
__global__ void __launch_bounds__(kThreads)
items_gather_kernel(const uint32_t* __restrict__ src, long long item_elems, const int32_t* __restrict__ index, long long n,
                    void* __restrict__ dst, long long tiles_per_item) {
  constexpr int ESZ = DT == SPR_F32 ? 4 : 2;
  constexpr int V = 16 / ESZ;
  const int tid = static_cast<int>(threadIdx.x);
  const long long tiles = n * tiles_per_item;
  for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
    const long long k = t / tiles_per_item;
    const long long tile = t - k * tiles_per_item;
    const uint32_t* __restrict__ s = src + static_cast<long long>(index[k]) * item_elems;
    unsigned char* d = static_cast<unsigned char*>(dst) + k * item_elems * ESZ;
    // elements in front of the first 16-byte boundary of the destination item
    long long head = static_cast<long long>((16u - static_cast<unsigned>(reinterpret_cast<uintptr_t>(d) & 15u)) & 15u) / ESZ;
    head = head < item_elems ? head : item_elems;
    const long long nvec = (item_elems - head) / V;
    const long long tail0 = head + nvec * V;
    if (tile == 0) {
      if (tid < head) gather_one<DT>(s, d, tid);
      if (tail0 + tid < item_elems) gather_one<DT>(s, d, tail0 + tid);  // (fewer than V of them)
    }
    const uint32_t* __restrict__ sv = s + head;
    u32x4* __restrict__ dv = reinterpret_cast<u32x4*>(d + head * ESZ);
    const long long v0 = tile * kGatherTileVecs;
    const bool aligned = (reinterpret_cast<uintptr_t>(sv) & 15u) == 0;  // uniform over the item
    if (aligned) {
#pragma unroll
      for (int u = 0; u < kGatherUnroll; ++u) {
        const long long j = v0 + u * kThreads + tid;
        if (j < nvec) dv[j] = gather_vec<DT, true>(sv + j * V);
      }
    } else {
#pragma unroll
      for (int u = 0; u < kGatherUnroll; ++u) {
        const long long j = v0 + u * kThreads + tid;
        if (j < nvec) dv[j] = gather_vec<DT, false>(sv + j * V);
      }
    }
  }
}

// One workgroup per row of the block (grid-stride), work-items over its columns.  MODE 0: copy, 1: float max.
template <int MODE>
__global__ void __launch_bounds__(kThreads)
block_scatter_kernel(uint32_t* __restrict__ dst, long long ld, const uint32_t* __restrict__ src, long long src_ld,
                     const int32_t* __restrict__ rows, long long nr, const int32_t* __restrict__ cols, long long nc) {
  for (long long i = blockIdx.x; i < nr; i += gridDim.x) {
    uint32_t* __restrict__ out = dst + static_cast<long long>(rows[i]) * ld;
    const uint32_t* __restrict__ in = src + i * src_ld;
    for (long long j = threadIdx.x; j < nc; j += kThreads) {
      const long long at = cols[j];
      if (MODE == 0) {
        out[at] = in[j];
      } else {
        union { uint32_t u; float f; } s, d;
        s.u = in[j];
        d.u = out[at];
        if (s.f > d.f) out[at] = s.u;
      }
    }
  }
}

template <int DT>
int launch_gather(const float* src, int64_t item_elems, const int32_t* index, int64_t n, void* dst, hipStream_t stream) {
  constexpr int V = DT == SPR_F32 ? 4 : 8;
  const long long tiles_per_item = item_elems / V / kGatherTileVecs + 1;  // covers the vectors behind any head
  const long long tiles = static_cast<long long>(n) * tiles_per_item;
  const long long blocks = tiles < kGatherMaxBlocks ? tiles : kGatherMaxBlocks;
  hipLaunchKernelGGL(items_gather_kernel<DT>, dim3(static_cast<unsigned>(blocks)), dim3(kThreads), 0, stream,
                     reinterpret_cast<const uint32_t*>(src),
                     static_cast<long long>(item_elems), index, static_cast<long long>(n), dst, tiles_per_item);
  return check_launch("items_gather_kernel");
}

}  // namespace
}  // namespace spr

extern "C" int spr_items_gather(const float* src, int64_t item_elems, const int32_t* index, int64_t n, void* dst,
                                int32_t dst_dtype, spr_stream_t stream) {
  using namespace spr;
  if (item_elems < 0 || n < 0) { set_error("spr_items_gather: negative size"); return SPR_ERR_ARG; }
  if (dst_dtype != SPR_F32 && dst_dtype != SPR_F16 && dst_dtype != SPR_BF16) {
    set_error("spr_items_gather: unknown dst_dtype %d", static_cast<int>(dst_dtype));
    return SPR_ERR_ARG;
  }
  if (n == 0 || item_elems == 0) return SPR_OK;
  if (!src || !index || !dst) { set_error("spr_items_gather: null pointer"); return SPR_ERR_ARG; }
  const uintptr_t esz = dst_dtype == SPR_F32 ? 4 : 2;
  if ((reinterpret_cast<uintptr_t>(src) & 3u) || (reinterpret_cast<uintptr_t>(dst) & (esz - 1))) {
    set_error("spr_items_gather: src / dst not aligned to their element size");
    return SPR_ERR_ARG;
  }
  if (item_elems > (INT64_MAX >> 3) / n) { set_error("spr_items_gather: n * item_elems overflows"); return SPR_ERR_ARG; }
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (dst_dtype == SPR_F32) return launch_gather<SPR_F32>(src, item_elems, index, n, dst, s);
  if (dst_dtype == SPR_F16) return launch_gather<SPR_F16>(src, item_elems, index, n, dst, s);
  return launch_gather<SPR_BF16>(src, item_elems, index, n, dst, s);
}

extern "C" int spr_block_scatter(void* dst, int64_t ld, const void* src, int64_t src_ld, const int32_t* rows, int64_t nr,
                                 const int32_t* cols, int64_t nc, int32_t mode, spr_stream_t stream) {
  using namespace spr;
  if (nr < 0 || nc < 0) { set_error("spr_block_scatter: negative size"); return SPR_ERR_ARG; }
  if (mode != 0 && mode != 1) { set_error("spr_block_scatter: unknown mode %d", static_cast<int>(mode)); return SPR_ERR_ARG; }
  if (ld < nc || src_ld < nc) { set_error("spr_block_scatter: ld / src_ld below the column count"); return SPR_ERR_ARG; }
  if (nr == 0 || nc == 0) return SPR_OK;
  if (!dst || !src || !rows || !cols) { set_error("spr_block_scatter: null pointer"); return SPR_ERR_ARG; }
  const long long blocks = nr < 65535 ? nr : 65535;
  uint32_t* d = static_cast<uint32_t*>(dst);
  const uint32_t* s = static_cast<const uint32_t*>(src);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (mode == 0) {
    hipLaunchKernelGGL(block_scatter_kernel<0>, dim3(static_cast<unsigned>(blocks)), dim3(kThreads), 0, st, d,
                       static_cast<long long>(ld), s, static_cast<long long>(src_ld), rows, static_cast<long long>(nr), cols,
                       static_cast<long long>(nc));
  } else {
    hipLaunchKernelGGL(block_scatter_kernel<1>, dim3(static_cast<unsigned>(blocks)), dim3(kThreads), 0, st, d,
                       static_cast<long long>(ld), s, static_cast<long long>(src_ld), rows, static_cast<long long>(nr), cols,
                       static_cast<long long>(nc));
  }
  return check_launch("block_scatter_kernel");
}
