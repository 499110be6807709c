// Internal declarations shared by the HIP translation units of libshoeprint_mi355x.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/shoeprint_mi355x.h"
#include <spr_intrinsics.h>  // angle form: the CPU-emulation test build shadows it by include path

namespace spr {

constexpr int kThreads = 256;          // work-items per workgroup of the prep / direct / rank kernels (4 waves)
constexpr int kLdsLimit = 160 * 1024;  // LDS per CU on gfx950

// complex<float> as a 2-wide vector: 8-byte aligned (single b64 LDS/global accesses) and complex
// add / sub / multiply lower to packed fp32 VALU (v_pk_add_f32, v_pk_mul_f32, v_pk_fma_f32), which
// issue at the scalar rate on gfx950: half the instructions at the low occupancy these kernels run at.
typedef float cf __attribute__((ext_vector_type(2)));
static_assert(sizeof(cf) == 8, "cf must be 8 bytes");

__host__ __device__ inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
__host__ __device__ inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

void set_error(const char* fmt, ...);
int check_launch(const char* what);

// ---------------------------------------------------------------------------------------------
// Geometry of one plan, passed by value to the kernels.
//
// Cropped template (query) maps are th x tw, cropped search (gallery) maps ih x iw.  'same'-mode
// output (similarity.py:55, scipy 'same') has the search map's size; output pixel (y, x)
// correlates the template with the window whose top-left corner is (y - th/2, x - tw/2).
struct NccGeom {
  int channels;
  int q_h, q_w, g_h, g_w;  // raw map sizes as stored by the caller
  int crop;
  int th, tw, ih, iw;  // cropped sizes
  int dtype;
  // FFT method only ------------------------------------------------------------------------
  int nh, nw;          // FFT grid (rows, cols); nh = eh*tgh, nw = ew*tgw
  int nt;              // work-items per workgroup of the pair kernel (prepared layouts are tiled by it)
  int eh, tgh, ew, tgw;
  int big;             // 1: working set in the plan's global workspace instead of LDS (maps too large for LDS)
  int six;             // 1: prepared layouts of the six-wave pair kernel (ncc_pair6.hip)
  int prep6;           // six-wave layout: 1 unless SPR_PREP6=0 was set when the plan was made - galleries whose windows are
                       // corner windows are prepared by ncc_prep6.hip (0: prep_fft_kernel, for A/B runs)
  int tight;           // 1: ih <= nh/2 and iw <= nw/2 (the pruned kernel variant), 0: general variant
  int rounds_c;        // column-pass rounds of (kThreads/tgh) columns covering nw/2 columns
  int r_rows;          // rows of the intermediate LDS image kept after the column pass (ih rounded up to 8)
  int r_stride;        // row stride (complex elements) of the transposed LDS image RT[column][row]
  int rounds_r;        // row-pass rounds of (kThreads/tgw) row pairs covering r_rows/2 pairs (r_rows is even)
  int keep_w;          // kept outputs per row sub-transform (covers iw)
  int nv;              // 1/sigma values (= accumulators) per lane and row round, a multiple of 4
  int spec_per_chan;   // complex elements of one channel's spectrum (tiled layout)
  int inv_per_chan;    // floats of one channel's 1/sigma map in pair-kernel register order
  // direct method only ---------------------------------------------------------------------
  int pad_h, pad_w;    // zero-padded search map: ih+th-1, iw+tw-1
  int strips_per_row;  // strips of kStrip output pixels per output row
  int strips_per_thread;
  // matrix-core method only -----------------------------------------------------------------
  int mfma_exact;      // 1: raw search map on the matrix cores + correction matrix (ncc_mfma.hip), 0: hi + lo
  int mfma_general;    // 1: the general instance (template up to 30 x 16 on a map up to 28 x 12), 0: the 28 x 12 / 28 x 12 one
  int mfma_f32;        // 1: SPR_NCC_MFMA_F32 - float32 maps, both operands centred and split into hi + lo (never with mfma_exact)
};

constexpr int kStrip = 8;  // output pixels per register strip in the direct kernel

// One spr_ncc_score / spr_ncc_maps call, one spr_ncc_prepare_* call, and the device memory a plan owns: what api.hip hands
// to the launchers below.  A launcher that slices a call passes a modified copy down.
struct PairCall {
  const void* pq; int64_t nq;
  const void* pg; int64_t ng;
  float* scores; int64_t ld, col0; int accumulate;
  float* maps_out;  // spr_ncc_maps: the correlation map of the one pair; scores is null then
  hipStream_t stream;
  // spr_ncc_score_peaks: where every pair's maximum lies ((y << 16) | x) and which call found it, indexed like scores;
  // peak_yx null = plain spr_ncc_score, peak_tag may be null on its own
  int32_t* peak_yx = nullptr;
  int32_t* peak_tag = nullptr;
  int32_t tag = 0;
  // spr_ncc_score_list: device [n_pairs][2] of (position in pq, position in pg); scores / peak_yx / peak_tag then hold one
  // entry per pair (ld and col0 mean nothing), nq and ng are what the kernels test every entry against.  Always with peak_yx.
  const int32_t* pairs = nullptr;
  int64_t n_pairs = 0;
  // spr_ncc_score_surfaces: the list form that also stores every entry's channel-mean map, device float32 [n_pairs][ih][iw];
  // null = spr_ncc_score_list.  Always with pairs.
  float* surfaces = nullptr;
};
struct PrepCall {
  bool is_query;
  const void* maps; int64_t n;
  void* prepared;
  hipStream_t stream;
};
struct PlanScratch {      // null where the plan's method has none
  cf* tw_h; cf* tw_w;     // FFT: exp(-2*pi*i*k/nh), k < nh, and the same for nw
  void* ws; size_t ws_bytes;  // FFT "big" geometries (maps beyond LDS): the working set
  float* six_ctab;        // six-wave pair kernel: its pre-twist table (nw/2 floats)
  float* mfma_x;          // matrix-core method, exact form: correction matrix (one call at a time per plan)
};

// The scorer's environment switches are all read through env_int: the method switches when a
// plan is created (the *_geometry functions), the others at every launch.
int env_int(const char* name, int fallback);  // the variable as an integer; `fallback` if unset or empty

// Launchers (each method in its own .hip file).  All enqueue on the call's stream and return SPR_OK or an error code.
int launch_prep_direct(const NccGeom& g, const PlanScratch& s, const PrepCall& c);
int launch_pair_direct(const NccGeom& g, const PlanScratch& s, const PairCall& c);
int launch_prep_fft(const NccGeom& g, const PlanScratch& s, const PrepCall& c);
int launch_pair_fft(const NccGeom& g, const PlanScratch& s, const PairCall& c);
int launch_pair_fft_peaks(const NccGeom& g, const PlanScratch& s, const PairCall& c);  // c.peak_yx set (ncc_fft_peaks.hip)
int launch_pair_fft_list(const NccGeom& g, const PlanScratch& s, const PairCall& c);   // c.pairs set (ncc_fft_list.hip)
int launch_pair_fft_surfaces(const NccGeom& g, const PlanScratch& s, const PairCall& c);  // c.surfaces set (ncc_fft_surfaces.hip)
int launch_pair6(const NccGeom& g, const PlanScratch& s, const PairCall& c);  // six-wave pair kernel (ncc_pair6.hip)
bool prep6_covers(const NccGeom& g);  // gallery of a six-wave plan with corner windows (ncc_prep6.hip)
int launch_prep6(const NccGeom& g, const PlanScratch& s, const PrepCall& c);
int launch_prep_mfma(const NccGeom& g, const PlanScratch& s, const PrepCall& c);  // bf16 / f16 matrix cores (ncc_mfma.hip), both methods
int launch_pair_mfma(const NccGeom& g, const PlanScratch& s, const PairCall& c);
int launch_pair_mfma_peaks(const NccGeom& g, const PlanScratch& s, const PairCall& c);  // c.peak_yx set (ncc_mfma_peaks.hip)
// Pair kernels run one workgroup per pair in tiles of `pairs_per_tile`; HIP refuses a grid of 2^32 work-items or
// more, so a launch takes at most this many tiles (SPR_NCC_MAX_TILES lowers it: tests of the slicing).
int64_t pair_tiles_per_launch(int pairs_per_tile, int threads);

size_t pair6_lds_bytes();
int pair6_max_rows();  // cropped search-map rows / columns the six-wave kernel covers
int pair6_max_cols();
size_t fft_workspace_bytes(const NccGeom& g);  // what a plan with this geometry must allocate (0: none)
bool mfma_geometry(NccGeom& g);  // true if an instantiated kernel covers this plan (fills mfma_exact)
bool mfma_f32_geometry(NccGeom& g);  // the same for SPR_NCC_MFMA_F32 (float32 maps)
size_t mfma_query_item_bytes(const NccGeom& g);
size_t mfma_gallery_item_bytes(const NccGeom& g);
size_t mfma_workspace_bytes(const NccGeom& g);  // the plan's correction matrix of the exact form (0: none)
bool fft_geometry(NccGeom& g, bool pow2_only);  // fills the FFT fields; false if no instantiated kernel fits
bool direct_geometry(NccGeom& g);  // fills the direct fields; false if the maps do not fit LDS

// Prepared-buffer sizes (bytes per item), both 256-byte multiples.
size_t prepared_query_item_bytes(const NccGeom& g, int method);
size_t prepared_gallery_item_bytes(const NccGeom& g, int method);

// Load one feature value of any supported storage type as float.
__device__ __forceinline__ float load_feature(const void* base, size_t idx, int dtype) {
  if (dtype == SPR_F32) return static_cast<const float*>(base)[idx];
  const uint16_t bits = static_cast<const uint16_t*>(base)[idx];
  if (dtype == SPR_BF16) {
    union { uint32_t u; float f; } v;
    v.u = static_cast<uint32_t>(bits) << 16;
    return v.f;
  }
  union { uint16_t u; _Float16 h; } v;
  v.u = bits;
  return static_cast<float>(v.h);
}

// float32 -> float16 / bfloat16 bit pattern, round to nearest even (what a stored 16-bit activation or weight of the 16-bit
// extractor plans holds), and back.  KIND = SPR_F16 | SPR_BF16.
__host__ __device__ inline uint16_t round_bf16(float v) {
  union { float f; uint32_t u; } c;
  c.f = v;
  if ((c.u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0;  // NaN
  c.u += 0x7fffu + ((c.u >> 16) & 1u);                    // ties to even
  return static_cast<uint16_t>(c.u >> 16);
}
// split(v) of the SPR_COMPUTE_BF16X3 extractor plans: hi = round_bf16(v), lo = round_bf16(v - float(hi)); the subtraction is
// exact in float32 (the contract is in the header, spr_vgg_plan_create_ex)
__host__ __device__ inline void split_bf16(float v, uint16_t& hi, uint16_t& lo) {
  hi = round_bf16(v);
  union { uint32_t u; float f; } h;
  h.u = static_cast<uint32_t>(hi) << 16;
  lo = round_bf16(v - h.f);
}
__device__ __forceinline__ uint16_t round_f16(float v) {
  union { _Float16 h; uint16_t u; } c;
  c.h = static_cast<_Float16>(v);  // v_cvt_f16_f32: round to nearest even
  return c.u;
}
template <int KIND>
__device__ __forceinline__ uint16_t round16(float v) { return KIND == SPR_F16 ? round_f16(v) : round_bf16(v); }
template <int KIND>
__device__ __forceinline__ float value16(uint16_t b) {
  if (KIND == SPR_F16) {
    union { uint16_t u; _Float16 h; } c;
    c.u = b;
    return static_cast<float>(c.h);
  }
  union { uint32_t u; float f; } c;
  c.u = static_cast<uint32_t>(b) << 16;
  return c.f;
}

// Workgroup reductions over the launch's work-items (a multiple of 64); `scratch` holds one value per wave.
__device__ __forceinline__ double block_sum(double v, double* scratch) {
  for (int m = 32; m >= 1; m >>= 1) v += shfl_xor(v, m);
  const int tid = static_cast<int>(threadIdx.x);
  __syncthreads();  // scratch may still be read by a previous reduction
  if ((tid & 63) == 0) scratch[tid >> 6] = v;
  __syncthreads();
  double s = 0.0;
  for (int w = 0; w < static_cast<int>(blockDim.x) / 64; ++w) s += scratch[w];
  return s;
}
template <int NT = kThreads>
__device__ __forceinline__ float block_max(float v, float* scratch) {
  for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, shfl_xor(v, m));
  const int tid = static_cast<int>(threadIdx.x);
  __syncthreads();
  if ((tid & 63) == 0) scratch[tid >> 6] = v;
  __syncthreads();
  float s = scratch[0];
  for (int w = 1; w < NT / 64; ++w) s = fmaxf(s, scratch[w]);
  return s;
}

// Peak form of the pair kernels (spr_ncc_score_peaks): the maximum travels with its position p = (y << 16) | x, and every
// reduction step orders (value, position) pairs - the larger value, among equal values the smaller position, i.e. the first
// in row-major order - so the result does not depend on which slot, lane or wave is looked at first.
constexpr int kNoPeak = 0x7fffffff;  // "no pixel yet": loses every tie against a real position
__device__ __forceinline__ void peak_take(float& v, int& p, float ov, int op) {
  const bool take = ov > v || (ov == v && op < p);
  v = take ? ov : v;
  p = take ? op : p;
}
__device__ __forceinline__ void wave_peak(float& v, int& p) {
  for (int m = 32; m >= 1; m >>= 1) {
    const float ov = shfl_xor(v, m);
    const int op = shfl_xor(p, m);
    peak_take(v, p, ov, op);
  }
}
// `scratch` holds two words per wave: NT / 64 values, then NT / 64 positions
template <int NT = kThreads>
__device__ __forceinline__ void block_peak(float& v, int& p, float* scratch) {
  wave_peak(v, p);
  int* pos = reinterpret_cast<int*>(scratch + NT / 64);
  const int tid = static_cast<int>(threadIdx.x);
  __syncthreads();
  if ((tid & 63) == 0) {
    scratch[tid >> 6] = v;
    pos[tid >> 6] = p;
  }
  __syncthreads();
  v = scratch[0];
  p = pos[0];
  for (int w = 1; w < NT / 64; ++w) peak_take(v, p, scratch[w], pos[w]);
}
// One entry of spr_ncc_score_peaks (the contract is in the header).  s = the pair's score, p = the position of the map's
// maximum; `scores` receives what the plain form stores.  Returns whether the entry was written: the surfaces form
// (spr_ncc_score_surfaces) stores the pair's map exactly then.
__device__ __forceinline__ bool store_peak(float* scores, int32_t* peak_yx, int32_t* peak_tag, size_t at, float s, int p,
                                           int32_t tag, int accumulate) {
  const bool hit = s > 0.0f;  // (only then is p a pixel that won)
  if (!accumulate) {
    scores[at] = hit ? s : 0.0f;
    peak_yx[at] = hit ? p : -1;
    if (peak_tag) peak_tag[at] = hit ? tag : -1;
    return true;
  }
  const float prev = scores[at];
  bool take = s > prev;
  if (!take && peak_tag && hit && s == prev) take = tag < peak_tag[at];
  if (take) {
    scores[at] = s;
    peak_yx[at] = hit ? p : -1;
    if (peak_tag) peak_tag[at] = hit ? tag : -1;
  }
  return take;
}

}  // namespace spr
