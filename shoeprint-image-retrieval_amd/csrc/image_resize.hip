// Crop + LANCZOS resize of decoded 8-bit images (reference dataloader.py:217-237: image.crop(box).resize(size, LANCZOS)),
// restating the 8-bit path of Pillow's separable resampler (Resample.c, ImagingResampleHorizontal_8bpc / Vertical_8bpc) bit
// for bit.  The host (image_resize.py) builds, per (input size, output size) pair of an axis, the int32 table
//   [out][2] first source index and tap count,  then  [out][ksize] coefficients in 22-bit fixed point,
// and the kernels do the integer part: per output sample acc = (1 << 21) + sum(pixel * k), result clamp(acc >> 22, 0, 255),
// once after the horizontal pass (stored as 8 bits in the workspace) and once after the vertical pass.  The sum wraps in
// 32-bit unsigned arithmetic and is read as signed for the arithmetic shift, which is what Pillow's `int` does.
//
// One call takes a ragged batch: a device array of spr_image_resize_item, two launches whatever the number of images.
// spr_image_resize_layout (host) gives every item its slice of each launch's grid; a workgroup finds its item by counting first blocks.
//
//   resize_h_kernel  tile = 32 source rows x 64 output columns, 4 waves; lane = output column, each wave 8 rows, so a
//                    coefficient is loaded once per 8 (x channels) multiply-adds.  The tile's source window goes through LDS
//                    in chunks of 768 bytes per row (a 1/30 downscale has windows of 181 taps: wider than the chunk, so the
//                    accumulators live across chunks; the sum is order-free because it wraps).  The crop box is the
//                    addressing of this stage, or of the next if the width does not change.
//   resize_v_kernel  tile = 8 output rows x 256 bytes of a row (channels are just bytes here), 4 waves x 2 output rows; lane
//                    = 4 adjacent bytes, read as one LDS dword per tap; the coefficient is the same for the whole wave.
//                    Source rows go through LDS in chunks of 32 rows.  Items whose size does not change are copied here.
//
// Global traffic is aligned dwords: a row segment is staged so that LDS keeps its global byte phase (address & 3), which makes
// the body of every segment dword-to-dword in both directions; only the ragged head and tail of a segment move as bytes.
#include "spr_common.h"

namespace spr {
namespace {

typedef spr_image_resize_item Item;
static_assert(sizeof(Item) == 88, "the host mirrors this layout (_lib.ImageResizeItem)");

constexpr int kHRows = 32, kHOuts = 64, kHRowsPerWave = 8;
constexpr int kHChunk = 768;             // staged source bytes per row and chunk (a multiple of 3)
constexpr int kHStride = kHChunk + 8;    // + byte phase, rounded to dwords
constexpr int kHOutStride = kHOuts * 3 + 8;
constexpr int kVRows = 8, kVBytes = 256, kVRowsPerWave = 2;
constexpr int kVChunk = 32;              // staged source rows per chunk
constexpr int kVStride = kVBytes + 8;
static_assert(kHRows == 4 * kHRowsPerWave && kVRows == 4 * kVRowsPerWave && kThreads == 256, "four waves per tile");

__device__ __forceinline__ int phase_of(const uint8_t* p) { return static_cast<int>(reinterpret_cast<uintptr_t>(p) & 3); }

// `count` bytes from global `src` to LDS row `dst` (dword aligned): byte i lands at dst[phase_of(src) + i].  Reads nothing
// outside [src, src + count).  Called by the 64 lanes of a wave.
__device__ __forceinline__ void stage_row(const uint8_t* src, int count, uint8_t* dst, int lane) {
  const int phase = phase_of(src);
  const uint8_t* a = src - phase;
  const int total = phase + count;
  for (int b0 = 4 * lane; b0 < total; b0 += 4 * 64) {
    if (b0 >= phase && b0 + 4 <= total) {
      *reinterpret_cast<uint32_t*>(dst + b0) = *reinterpret_cast<const uint32_t*>(a + b0);
    } else {
      for (int b = b0 > phase ? b0 : phase; b < b0 + 4 && b < total; ++b) dst[b] = a[b];
    }
  }
}

// The reverse: LDS row `src` holds byte i of the segment at src[phase_of(dst) + i].  Writes nothing outside [dst, dst + count).
__device__ __forceinline__ void store_row(uint8_t* dst, int count, const uint8_t* src, int lane) {
  const int phase = phase_of(dst);
  uint8_t* a = dst - phase;
  const int total = phase + count;
  for (int b0 = 4 * lane; b0 < total; b0 += 4 * 64) {
    if (b0 >= phase && b0 + 4 <= total) {
      *reinterpret_cast<uint32_t*>(a + b0) = *reinterpret_cast<const uint32_t*>(src + b0);
    } else {
      for (int b = b0 > phase ? b0 : phase; b < b0 + 4 && b < total; ++b) a[b] = src[b];
    }
  }
}

// acc + pixel * k in wrapping 32-bit arithmetic.  Coefficients lie in [-2^23, 2^23) (lanczos_tables refuses others) and
// pixels in [0, 255], so the 24-bit multiplier (full rate; the 32-bit one is quarter rate) gives the exact product.
__device__ __forceinline__ uint32_t mad24(uint32_t acc, uint32_t pixel, int32_t k) {
#ifndef SPR_EMU
  return acc + static_cast<uint32_t>(__mul24(static_cast<int>(pixel), k));
#else
  return acc + pixel * static_cast<uint32_t>(k);
#endif
}

__device__ __forceinline__ uint8_t clip8(uint32_t acc) {
  const int v = static_cast<int32_t>(acc) >> 22;  // arithmetic shift of the wrapped sum
  return static_cast<uint8_t>(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// The item whose slice of the grid holds workgroup `b`: the last one whose first block is <= b (items without blocks in this
// launch share their first block with the next item).  First blocks do not decrease along the array, so that item's index is
// the number of first blocks <= b, minus one.  Every wave counts for itself, lane = item, in strides of 64: the loads do not
// depend on one another, so a batch of up to 64 items costs one memory latency where a bisection would chain six.
template <bool H>
__device__ __forceinline__ int find_item(const Item* __restrict__ items, int n, int b, int lane) {
  int count = 0;
  for (int i0 = 0; i0 < n; i0 += 64) {
    const int i = i0 + lane;
    if (i < n && (H ? items[i].hblock0 : items[i].vblock0) <= b) ++count;
  }
  for (int m = 32; m >= 1; m >>= 1) count += shfl_xor(count, m);
  return uniform(count) - 1;
}

template <int C>
__global__ void __launch_bounds__(kThreads)
resize_h_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, uint8_t* __restrict__ tmp,
                const Item* __restrict__ items, int n, const int32_t* __restrict__ tables) {
  __shared__ uint32_t stage_w[kHRows * kHStride / 4];
  __shared__ uint32_t otile_w[kHRows * kHOutStride / 4];
  uint8_t* stage = reinterpret_cast<uint8_t*>(stage_w);
  uint8_t* otile = reinterpret_cast<uint8_t*>(otile_w);
  const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, wave = tid >> 6;
  const int b = static_cast<int>(blockIdx.x);
  const Item it = items[find_item<true>(items, n, b, lane)];
  const int tiles_x = ceil_div(it.out_w, kHOuts);
  const int lb = b - it.hblock0, ty = lb / tiles_x, tx = lb - ty * tiles_x;
  const int row0 = ty * kHRows, o0 = tx * kHOuts;
  const int nrows = it.box_h - row0 < kHRows ? it.box_h - row0 : kHRows;
  const int nouts = it.out_w - o0 < kHOuts ? it.out_w - o0 : kHOuts;
  const int32_t* bounds = tables + it.htab;
  const int32_t* coef = bounds + 2 * static_cast<size_t>(it.out_w);
  const int s0 = bounds[2 * o0];
  const int s1 = bounds[2 * (o0 + nouts - 1)] + bounds[2 * (o0 + nouts - 1) + 1];  // windows move right with the output column
  const bool live = lane < nouts;
  const int xmin = live ? bounds[2 * (o0 + lane)] : 0, cnt = live ? bounds[2 * (o0 + lane) + 1] : 0;
  const int32_t* k = coef + static_cast<size_t>(o0 + lane) * it.hk;
  const uint8_t* src = in + it.in_off + static_cast<int64_t>(it.box_y + row0) * it.in_stride + static_cast<int64_t>(it.box_x) * C;

  const int my_rows = nrows - wave * kHRowsPerWave;  // rows of this wave that exist (may be <= 0)
  uint32_t acc[kHRowsPerWave][C];
#pragma unroll
  for (int r = 0; r < kHRowsPerWave; ++r)
#pragma unroll
    for (int c = 0; c < C; ++c) acc[r][c] = 1u << 21;

  constexpr int chunk_px = kHChunk / C;
  for (int c0 = s0; c0 < s1; c0 += chunk_px) {
    const int c1 = c0 + chunk_px < s1 ? c0 + chunk_px : s1;
    __syncthreads();  // the previous chunk has been read
    for (int r = wave; r < nrows; r += 4)
      stage_row(src + static_cast<int64_t>(r) * it.in_stride + static_cast<int64_t>(c0) * C, (c1 - c0) * C, stage + r * kHStride, lane);
    __syncthreads();
    const int t0 = xmin > c0 ? xmin : c0, t1 = xmin + cnt < c1 ? xmin + cnt : c1;
    int row_at[kHRowsPerWave];  // where each of this wave's rows starts in the staged chunk, byte phase included
#pragma unroll
    for (int rr = 0; rr < kHRowsPerWave; ++rr) {
      const int r = wave * kHRowsPerWave + rr;
      row_at[rr] = r * kHStride + phase_of(src + static_cast<int64_t>(r) * it.in_stride + static_cast<int64_t>(c0) * C);
    }
    for (int x = t0; x < t1; ++x) {  // one coefficient load per 8 rows x C channels
      const int32_t kv = k[x - xmin];
#pragma unroll
      for (int rr = 0; rr < kHRowsPerWave; ++rr) {
        if (rr < my_rows) {
          const uint8_t* px = stage + row_at[rr] + (x - c0) * C;
#pragma unroll
          for (int c = 0; c < C; ++c) acc[rr][c] = mad24(acc[rr][c], px[c], kv);
        }
      }
    }
  }

  // clamp to 8 bits and hand the tile's rows to the dword store through LDS
  const bool to_tmp = it.vtab >= 0;
  uint8_t* dst = to_tmp ? tmp + it.tmp_off + static_cast<int64_t>(row0) * it.tmp_stride + o0 * C
                        : out + it.out_off + static_cast<int64_t>(row0) * it.out_w * C + o0 * C;
  const int64_t dstride = to_tmp ? it.tmp_stride : static_cast<int64_t>(it.out_w) * C;
  if (live) {
#pragma unroll
    for (int rr = 0; rr < kHRowsPerWave; ++rr) {
      const int r = wave * kHRowsPerWave + rr;
      if (r >= nrows) break;
      uint8_t* o = otile + r * kHOutStride + phase_of(dst + r * dstride) + lane * C;
#pragma unroll
      for (int c = 0; c < C; ++c) o[c] = clip8(acc[rr][c]);
    }
  }
  __syncthreads();
  for (int r = wave; r < nrows; r += 4) store_row(dst + r * dstride, nouts * C, otile + r * kHOutStride, lane);
}

__global__ void __launch_bounds__(kThreads)
resize_v_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, const uint8_t* __restrict__ tmp,
                const Item* __restrict__ items, int n, int channels, const int32_t* __restrict__ tables) {
  __shared__ uint32_t stage_w[kVChunk * kVStride / 4];
  __shared__ uint32_t otile_w[kVRows * kVStride / 4];
  uint8_t* stage = reinterpret_cast<uint8_t*>(stage_w);
  uint8_t* otile = reinterpret_cast<uint8_t*>(otile_w);
  const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, wave = tid >> 6;
  const int b = static_cast<int>(blockIdx.x);
  const Item it = items[find_item<false>(items, n, b, lane)];
  const int row_bytes = it.out_w * channels;
  const int tiles_x = ceil_div(row_bytes, kVBytes);
  const int lb = b - it.vblock0, ty = lb / tiles_x, tx = lb - ty * tiles_x;
  const int oy0 = ty * kVRows, xb0 = tx * kVBytes;
  const int nrows = it.out_h - oy0 < kVRows ? it.out_h - oy0 : kVRows;
  const int nb = row_bytes - xb0 < kVBytes ? row_bytes - xb0 : kVBytes;
  // the horizontal result if there is one, else the crop box of the decoded image
  const bool from_tmp = it.htab >= 0;
  const uint8_t* src = from_tmp ? tmp + it.tmp_off + xb0
                                : in + it.in_off + static_cast<int64_t>(it.box_y) * it.in_stride + static_cast<int64_t>(it.box_x) * channels + xb0;
  const int64_t sstride = from_tmp ? it.tmp_stride : it.in_stride;
  uint8_t* dst = out + it.out_off + static_cast<int64_t>(oy0) * row_bytes + xb0;

  if (it.vtab < 0) {  // neither size changes: Pillow returns a copy
    for (int r = wave; r < nrows; r += 4) {
      const uint8_t* s = src + (oy0 + r) * sstride;
      uint8_t* o = otile + r * kVStride;
      const int dphase = phase_of(dst + static_cast<int64_t>(r) * row_bytes);
      if (phase_of(s) == dphase) {
        stage_row(s, nb, o, lane);
      } else {
        for (int i = lane; i < nb; i += 64) o[dphase + i] = s[i];
      }
    }
    __syncthreads();
    for (int r = wave; r < nrows; r += 4) store_row(dst + static_cast<int64_t>(r) * row_bytes, nb, otile + r * kVStride, lane);
    return;
  }

  const int32_t* bounds = tables + it.vtab;
  const int32_t* coef = bounds + 2 * static_cast<size_t>(it.out_h);
  const int r0 = bounds[2 * oy0];
  const int r1 = bounds[2 * (oy0 + nrows - 1)] + bounds[2 * (oy0 + nrows - 1) + 1];  // windows move down with the output row
  const bool live = 4 * lane < nb;
  uint32_t acc[kVRowsPerWave][4];
#pragma unroll
  for (int q = 0; q < kVRowsPerWave; ++q)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[q][j] = 1u << 21;

  for (int c0 = r0; c0 < r1; c0 += kVChunk) {
    const int c1 = c0 + kVChunk < r1 ? c0 + kVChunk : r1;
    __syncthreads();  // the previous chunk has been read
    for (int r = wave; r < c1 - c0; r += 4) stage_row(src + (c0 + r) * sstride, nb, stage + r * kVStride, lane);
    __syncthreads();
    if (live) {
#pragma unroll
      for (int q = 0; q < kVRowsPerWave; ++q) {
        const int oy = oy0 + wave * kVRowsPerWave + q;
        if (oy >= it.out_h) break;
        const int ymin = bounds[2 * oy], cnt = bounds[2 * oy + 1];
        const int32_t* k = coef + static_cast<size_t>(oy) * it.vk;
        const int t0 = ymin > c0 ? ymin : c0, t1 = ymin + cnt < c1 ? ymin + cnt : c1;
        for (int y = t0; y < t1; ++y) {
          const int32_t kv = k[y - ymin];
          const uint8_t* p = stage + (y - c0) * kVStride + phase_of(src + y * sstride) + 4 * lane;
          uint32_t px;
          if ((reinterpret_cast<uintptr_t>(p) & 3) == 0) {
            px = *reinterpret_cast<const uint32_t*>(p);
          } else {
            px = static_cast<uint32_t>(p[0]) | static_cast<uint32_t>(p[1]) << 8 | static_cast<uint32_t>(p[2]) << 16 |
                 static_cast<uint32_t>(p[3]) << 24;
          }
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[q][j] = mad24(acc[q][j], (px >> (8 * j)) & 0xffu, kv);
        }
      }
    }
  }

  if (live) {
#pragma unroll
    for (int q = 0; q < kVRowsPerWave; ++q) {
      const int r = wave * kVRowsPerWave + q;
      if (r >= nrows) break;
      uint8_t* o = otile + r * kVStride + phase_of(dst + static_cast<int64_t>(r) * row_bytes) + 4 * lane;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = clip8(acc[q][j]);  // bytes past the tile's end stay inside the LDS row and are not stored
    }
  }
  __syncthreads();
  for (int r = wave; r < nrows; r += 4) store_row(dst + static_cast<int64_t>(r) * row_bytes, nb, otile + r * kVStride, lane);
}

}  // namespace
}  // namespace spr

extern "C" int spr_image_resize_layout(spr_image_resize_item* items, int64_t n, int32_t channels, size_t* workspace_bytes,
                                       int32_t* blocks) {
  using namespace spr;
  if (n < 0 || (channels != 1 && channels != 3)) { set_error("spr_image_resize_layout: bad count / channels (1 or 3)"); return SPR_ERR_ARG; }
  if (!workspace_bytes || !blocks || (n > 0 && !items)) { set_error("spr_image_resize_layout: null pointer"); return SPR_ERR_ARG; }
  size_t ws = 0;
  int64_t hb = 0, vb = 0;
  for (int64_t i = 0; i < n; ++i) {
    Item& it = items[i];
    if (it.out_w < 1 || it.out_h < 1) { set_error("spr_image_resize_layout: item %lld: height and width must be > 0", static_cast<long long>(i)); return SPR_ERR_ARG; }
    if (it.in_h < 1 || it.in_w < 1 || it.box_w < 1 || it.box_h < 1 || it.box_x < 0 || it.box_y < 0 ||
        static_cast<int64_t>(it.box_x) + it.box_w > it.in_w || static_cast<int64_t>(it.box_y) + it.box_h > it.in_h ||
        it.in_stride < static_cast<int64_t>(it.in_w) * channels || it.in_off < 0 || it.out_off < 0 ||
        static_cast<int64_t>(it.in_w) * channels > INT32_MAX / 2 || static_cast<int64_t>(it.out_w) * channels > INT32_MAX / 2) {
      set_error("spr_image_resize_layout: item %lld: bad image size, stride, offset or crop box", static_cast<long long>(i));
      return SPR_ERR_ARG;
    }
    const bool horiz = it.out_w != it.box_w, vert = it.out_h != it.box_h;
    if (horiz != (it.htab >= 0) || vert != (it.vtab >= 0) || (horiz && it.hk < 1) || (vert && it.vk < 1)) {
      set_error("spr_image_resize_layout: item %lld: a pass has a table exactly when its size changes", static_cast<long long>(i));
      return SPR_ERR_ARG;
    }
    it.hblock0 = static_cast<int32_t>(hb);
    it.vblock0 = static_cast<int32_t>(vb);
    it.tmp_off = 0;
    it.tmp_stride = 0;
    if (horiz) hb += static_cast<int64_t>(ceil_div(it.box_h, kHRows)) * ceil_div(it.out_w, kHOuts);
    if (horiz && vert) {  // the 8-bit horizontal result: rows start on 16-byte boundaries
      it.tmp_stride = static_cast<int32_t>(align_up(static_cast<size_t>(it.out_w) * channels, 16));
      it.tmp_off = static_cast<int64_t>(ws);
      ws += align_up(static_cast<size_t>(it.tmp_stride) * it.box_h, 256);
    }
    if (vert || !horiz) vb += static_cast<int64_t>(ceil_div(it.out_h, kVRows)) * ceil_div(it.out_w * channels, kVBytes);
    if (hb > INT32_MAX || vb > INT32_MAX) { set_error("spr_image_resize_layout: more than 2^31 - 1 tiles in one call"); return SPR_ERR_ARG; }
  }
  *workspace_bytes = ws;
  blocks[0] = static_cast<int32_t>(hb);
  blocks[1] = static_cast<int32_t>(vb);
  return SPR_OK;
}

extern "C" int spr_image_resize_u8(const uint8_t* in, uint8_t* out, const spr_image_resize_item* items, int64_t n,
                                   int32_t channels, const int32_t* tables, const int32_t* blocks, void* workspace,
                                   spr_stream_t stream) {
  using namespace spr;
  if (n < 0 || n > INT32_MAX || (channels != 1 && channels != 3)) { set_error("spr_image_resize_u8: bad count / channels (1 or 3)"); return SPR_ERR_ARG; }
  if (n == 0) return SPR_OK;
  if (!in || !out || !items || !tables || !blocks || !workspace) { set_error("spr_image_resize_u8: null pointer"); return SPR_ERR_ARG; }
  if (blocks[0] < 0 || blocks[1] < 0) { set_error("spr_image_resize_u8: negative block count"); return SPR_ERR_ARG; }
  hipStream_t s = static_cast<hipStream_t>(stream);
  uint8_t* tmp = static_cast<uint8_t*>(workspace);
  if (blocks[0] > 0) {
    if (channels == 1)
      hipLaunchKernelGGL(resize_h_kernel<1>, dim3(static_cast<unsigned>(blocks[0])), dim3(kThreads), 0, s, in, out, tmp, items,
                         static_cast<int>(n), tables);
    else
      hipLaunchKernelGGL(resize_h_kernel<3>, dim3(static_cast<unsigned>(blocks[0])), dim3(kThreads), 0, s, in, out, tmp, items,
                         static_cast<int>(n), tables);
    const int rc = check_launch("resize_h_kernel");
    if (rc != SPR_OK) return rc;
  }
  if (blocks[1] > 0) {
    hipLaunchKernelGGL(resize_v_kernel, dim3(static_cast<unsigned>(blocks[1])), dim3(kThreads), 0, s, in, out,
                       static_cast<const uint8_t*>(tmp), items, static_cast<int>(n), channels, tables);
    return check_launch("resize_v_kernel");
  }
  return SPR_OK;
}
