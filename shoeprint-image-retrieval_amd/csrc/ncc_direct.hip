// Direct (sliding-window) NCC scorer: the shape-agnostic method.
//
// One workgroup scores one (query, gallery) pair, channel by channel (similarity.py:100-108):
// the zero-padded, centred search map and the normalised template of the current channel live in
// LDS; every lane owns register strips of kStrip output pixels and walks the template, so each
// template tap is one LDS broadcast and 2*kStrip-1 search-map reads feed kStrip*kStrip FMAs.
// The channel sum stays in registers; one wave/LDS max-reduction at the end gives the score.
//
// This is the simple path: arithmetic = th*tw*pad... multiply-adds per output pixel including
// the zero padding.  The FFT method (ncc_pair_fft.hip) is the fast path; this one covers every
// shape that fits LDS and cross-checks the FFT path on the GPU.
#include <type_traits>

#include "ncc_prep_common.h"

namespace spr {

namespace {

// The surfaces form's geometry argument: the plan's, and behind it where the maps go.  An argument struct of its own, so that
// the kernel arguments of every other form lie where they lay.
struct NccGeomSurf : NccGeom {
  float* surfaces;  // device float32 [entries of the list][ih][iw]
};

__host__ __device__ inline int round_up8(int v) { return (v + 7) / 8 * 8; }

// LDS layouts ------------------------------------------------------------------------------
struct PrepLds {
  size_t red_off, x0_off, sat_off, total;
};
inline PrepLds prep_lds(int h, int w, bool need_sat) {
  PrepLds l;
  l.red_off = 0;
  l.x0_off = 64;
  l.sat_off = align_up(l.x0_off + sizeof(float) * h * w, 16);
  l.total = l.sat_off + (need_sat ? sizeof(double) * (h + 1) * (w + 1) : 0);
  return l;
}

// grid = (channels, n_items)
__global__ void __launch_bounds__(kThreads)
prep_direct_kernel(NccGeom g, int is_query, const void* __restrict__ maps, float* __restrict__ prepared,
                   size_t item_floats, unsigned x0_off, unsigned sat_off) {
  unsigned char* lds = dyn_lds();
  double* red = reinterpret_cast<double*>(lds);
  float* x0 = reinterpret_cast<float*>(lds + x0_off);
  double* sat = reinterpret_cast<double*>(lds + sat_off);
  const int c = static_cast<int>(blockIdx.x);
  const size_t item = blockIdx.y;
  const int tid = static_cast<int>(threadIdx.x);
  if (is_query) {
    const int n = g.th * g.tw;
    const size_t base = (item * g.channels + c) * static_cast<size_t>(g.q_h) * g.q_w;
    load_centred(maps, base, g.q_w, g.crop, g.th, g.tw, g.dtype, x0, red);
    const float scale = template_scale(x0, n, red);
    float* out = prepared + item * item_floats + static_cast<size_t>(c) * n;
    for (int i = tid; i < n; i += kThreads) out[i] = x0[i] * scale;
  } else {
    const int n = g.ih * g.iw;
    const size_t base = (item * g.channels + c) * static_cast<size_t>(g.g_h) * g.g_w;
    load_centred(maps, base, g.g_w, g.crop, g.ih, g.iw, g.dtype, x0, red);
    float* out = prepared + item * item_floats + static_cast<size_t>(c) * n;
    float* inv = out + static_cast<size_t>(g.channels) * n;
    for (int i = tid; i < n; i += kThreads) out[i] = x0[i];
    inv_sigma_map(x0, g.ih, g.iw, g.th, g.tw, sat, [&](int i, float v) { inv[i] = v; });
  }
}

// grid = (n_gallery, n_queries).  PEAKS: the form behind spr_ncc_score_peaks, an instantiation of its own
// LIST: the form behind spr_ncc_score_list, a peak form on a 1-D grid: workgroup w takes entry col0 + w of a device list of
// (query, gallery) positions.  The list rides in `maps_out`, its length in `ld`, and the item counts every entry is tested
// against in g.nh / g.nw, FFT fields this method has no use for: the form has no parameters of its own.
// SURF: the form behind spr_ncc_score_surfaces, a list form that also stores the entry's channel-mean map, total / channels,
// where its (score, peak, tag) is written; the form is told by its geometry argument (G = NccGeomSurf).
template <int SPT, bool PEAKS, bool LIST, class G = NccGeom>
__global__ void __launch_bounds__(kThreads)
pair_direct_kernel(G g, const float* __restrict__ pq, size_t q_item_floats, const float* __restrict__ pg,
                   size_t g_item_floats, float* __restrict__ scores, long long ld, long long col0, int accumulate,
                   float* __restrict__ maps_out, int pws, int tws, unsigned t_off, int32_t* __restrict__ peak_yx,
                   int32_t* __restrict__ peak_tag, int32_t tag) {
  unsigned char* lds = dyn_lds();
  float* red = reinterpret_cast<float*>(lds);
  float* P = reinterpret_cast<float*>(lds + 64);
  float* T = reinterpret_cast<float*>(lds + t_off);
  const int tid = static_cast<int>(threadIdx.x);
  size_t gi = blockIdx.x, qi = blockIdx.y;
  size_t list_at = 0;  // LIST: this workgroup's entry = where its three outputs go
  if constexpr (LIST) {
    list_at = static_cast<size_t>(col0) + blockIdx.x;
    if (list_at >= static_cast<size_t>(ld)) return;
    const int32_t* entry = reinterpret_cast<const int32_t*>(maps_out) + 2 * list_at;
    const int q = uniform(entry[0]), gg = uniform(entry[1]);
    if (q < 0 || q >= g.nh || gg < 0 || gg >= g.nw) return;  // names no item: skipped whole (uniform per workgroup)
    qi = static_cast<size_t>(q);
    gi = static_cast<size_t>(gg);
  }
  const int cy = g.th / 2, cx = g.tw / 2;
  const int n_img = g.ih * g.iw, n_tpl = g.th * g.tw;
  const float* q_base = pq + qi * q_item_floats;
  const float* g_base = pg + gi * g_item_floats;
  const float* inv_base = g_base + static_cast<size_t>(g.channels) * n_img;

  // zero the padded image (borders stay zero for every channel) and the template tail columns
  for (int i = tid; i < g.pad_h * pws; i += kThreads) P[i] = 0.0f;
  for (int i = tid; i < g.th * tws; i += kThreads) T[i] = 0.0f;

  int sy[SPT], sx[SPT];
  float total[SPT][kStrip];
#pragma unroll
  for (int k = 0; k < SPT; ++k) {
    const int s = tid + k * kThreads;
    sy[k] = s / g.strips_per_row;
    sx[k] = (s - sy[k] * g.strips_per_row) * kStrip;
#pragma unroll
    for (int j = 0; j < kStrip; ++j) total[k][j] = 0.0f;
  }

  for (int c = 0; c < g.channels; ++c) {
    __syncthreads();  // previous channel's reads are done (and the initial zero fill is visible)
    const float* img = g_base + static_cast<size_t>(c) * n_img;
    for (int i = tid; i < n_img; i += kThreads) {
      const int y = i / g.iw, x = i - y * g.iw;
      P[(y + cy) * pws + (x + cx)] = img[i];
    }
    const float* tpl = q_base + static_cast<size_t>(c) * n_tpl;
    for (int i = tid; i < n_tpl; i += kThreads) {
      const int u = i / g.tw, v = i - u * g.tw;
      T[u * tws + v] = tpl[i];
    }
    __syncthreads();
    const float* inv = inv_base + static_cast<size_t>(c) * n_img;
#pragma unroll
    for (int k = 0; k < SPT; ++k) {
      if (sy[k] >= g.ih) continue;
      float acc[kStrip];
#pragma unroll
      for (int j = 0; j < kStrip; ++j) acc[j] = 0.0f;
      for (int u = 0; u < g.th; ++u) {
        const float* prow = P + (sy[k] + u) * pws + sx[k];
        const float* trow = T + u * tws;
        for (int v0 = 0; v0 < tws; v0 += kStrip) {
          float seg[2 * kStrip - 1], tv[kStrip];
#pragma unroll
          for (int j = 0; j < 2 * kStrip - 1; ++j) seg[j] = prow[v0 + j];
#pragma unroll
          for (int j = 0; j < kStrip; ++j) tv[j] = trow[v0 + j];
#pragma unroll
          for (int vv = 0; vv < kStrip; ++vv) {
#pragma unroll
            for (int j = 0; j < kStrip; ++j) acc[j] = fmaf(tv[vv], seg[vv + j], acc[j]);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < kStrip; ++j) {
        const int x = sx[k] + j;
        if (x < g.iw) {
          const float val = acc[j] * inv[sy[k] * g.iw + x];
          total[k][j] += val;
          if (!LIST && maps_out) maps_out[(static_cast<size_t>(c) * g.ih + sy[k]) * g.iw + x] = val;
        }
      }
    }
  }

  if constexpr (PEAKS) {  // spr_ncc_score_peaks: the same maximum with its position
    float best = -3.0e38f;
    int where = kNoPeak;
#pragma unroll
    for (int k = 0; k < SPT; ++k) {
#pragma unroll
      for (int j = 0; j < kStrip; ++j) {
        if (sy[k] < g.ih && sx[k] + j < g.iw) peak_take(best, where, total[k][j], (sy[k] << 16) | (sx[k] + j));
      }
    }
    block_peak(best, where, red);
    if constexpr (std::is_same<G, NccGeomSurf>::value) {
      // work-item 0 decides, as it does in the list form, and tells the others through a spare word of the reduction scratch
      // (block_peak uses 8 of its 16); then every work-item stores the pixels it owns
      static_assert(LIST, "the surfaces form is a list form");
      int* told = reinterpret_cast<int*>(red) + 15;
      if (tid == 0)
        *told = store_peak(scores, peak_yx, peak_tag, list_at, best / static_cast<float>(g.channels), where, tag, accumulate) ? 1 : 0;
      __syncthreads();
      if (*told) {
        float* dst = g.surfaces + list_at * static_cast<size_t>(n_img);
        const float channels = static_cast<float>(g.channels);
#pragma unroll
        for (int k = 0; k < SPT; ++k) {
#pragma unroll
          for (int j = 0; j < kStrip; ++j) {
            if (sy[k] < g.ih && sx[k] + j < g.iw) dst[sy[k] * g.iw + sx[k] + j] = total[k][j] / channels;
          }
        }
      }
      return;
    } else if (tid == 0)
      store_peak(scores, peak_yx, peak_tag, LIST ? list_at : qi * ld + col0 + gi, best / static_cast<float>(g.channels), where, tag, accumulate);
    return;
  }
  float best = -3.0e38f;
#pragma unroll
  for (int k = 0; k < SPT; ++k) {
#pragma unroll
    for (int j = 0; j < kStrip; ++j) {
      if (sy[k] < g.ih && sx[k] + j < g.iw) best = fmaxf(best, total[k][j]);
    }
  }
  best = block_max(best, red);
  if (tid == 0 && scores) {
    float s = best / static_cast<float>(g.channels);
    float* dst = scores + qi * ld + col0 + gi;
    const float prev = accumulate ? *dst : 0.0f;
    *dst = s > prev ? s : prev;  // similarity.py:355, 366-367: zero-initialised running maximum
  }
}

struct DirectLds {
  int pws, tws;
  size_t t_off, total;
};
inline DirectLds direct_lds(const NccGeom& g) {
  DirectLds l;
  l.tws = round_up8(g.tw);
  l.pws = kStrip * g.strips_per_row + l.tws;
  if (l.pws < g.pad_w) l.pws = g.pad_w;
  l.t_off = align_up(64 + sizeof(float) * static_cast<size_t>(g.pad_h) * l.pws, 16);
  l.total = l.t_off + sizeof(float) * static_cast<size_t>(g.th) * l.tws;
  return l;
}

}  // namespace

bool direct_geometry(NccGeom& g) {
  g.pad_h = g.ih + g.th - 1;
  g.pad_w = g.iw + g.tw - 1;
  g.strips_per_row = ceil_div(g.iw, kStrip);
  const int strips = g.ih * g.strips_per_row;
  g.strips_per_thread = 1;
  while (g.strips_per_thread < ceil_div(strips, kThreads)) g.strips_per_thread *= 2;
  if (g.strips_per_thread > 8) return false;
  if (direct_lds(g).total > static_cast<size_t>(kLdsLimit)) return false;
  if (g.ih * g.iw > kMaxPixPerThread * kThreads || g.th * g.tw > kMaxPixPerThread * kThreads) return false;
  if (prep_lds(g.ih, g.iw, true).total > static_cast<size_t>(kLdsLimit)) return false;
  return true;
}

int launch_prep_direct(const NccGeom& g, const PlanScratch&, const PrepCall& c) {
  if (c.n == 0) return SPR_OK;
  const PrepLds l = c.is_query ? prep_lds(g.th, g.tw, false) : prep_lds(g.ih, g.iw, true);
  const size_t item_floats =
      (c.is_query ? prepared_query_item_bytes(g, SPR_NCC_DIRECT) : prepared_gallery_item_bytes(g, SPR_NCC_DIRECT)) /
      sizeof(float);
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(prep_direct_kernel),
                            hipFuncAttributeMaxDynamicSharedMemorySize, kLdsLimit);
  hipLaunchKernelGGL(prep_direct_kernel, dim3(g.channels, static_cast<unsigned>(c.n)), dim3(kThreads), l.total, c.stream,
                     g, c.is_query ? 1 : 0, c.maps, static_cast<float*>(c.prepared), item_floats,
                     static_cast<unsigned>(l.x0_off), static_cast<unsigned>(l.sat_off));
  return check_launch("prep_direct_kernel");
}

template <int SPT, bool PEAKS, bool LIST = false, class G = NccGeom>
static int launch_pair_direct_t(const NccGeom& g, const PlanScratch&, const PairCall& c) {
  const DirectLds l = direct_lds(g);
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(pair_direct_kernel<SPT, PEAKS, LIST, G>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, kLdsLimit);
  // grid = (gallery, query) workgroups; HIP refuses 2^32 work-items and more along x: slices of the gallery
  const size_t g_item_floats = prepared_gallery_item_bytes(g, SPR_NCC_DIRECT) / sizeof(float);
  const int64_t max_g = pair_tiles_per_launch(1, kThreads);
  if constexpr (LIST) {  // one workgroup per entry, sliced like the gallery below
    G gl{};
    static_cast<NccGeom&>(gl) = g;
    gl.nh = static_cast<int>(c.nq);  // (see the kernel)
    gl.nw = static_cast<int>(c.ng);
    if constexpr (std::is_same<G, NccGeomSurf>::value) gl.surfaces = c.surfaces;
    for (int64_t e0 = 0; e0 < c.n_pairs; e0 += max_g) {
      const int64_t n = c.n_pairs - e0 < max_g ? c.n_pairs - e0 : max_g;
      hipLaunchKernelGGL(HIP_KERNEL_NAME(pair_direct_kernel<SPT, PEAKS, LIST, G>), dim3(static_cast<unsigned>(n)), dim3(kThreads),
                         l.total, c.stream, gl, static_cast<const float*>(c.pq),
                         prepared_query_item_bytes(g, SPR_NCC_DIRECT) / sizeof(float), static_cast<const float*>(c.pg),
                         g_item_floats, c.scores, static_cast<long long>(c.n_pairs), static_cast<long long>(e0), c.accumulate,
                         reinterpret_cast<float*>(const_cast<int32_t*>(c.pairs)), l.pws, l.tws, static_cast<unsigned>(l.t_off),
                         c.peak_yx, c.peak_tag, c.tag);
      const int rc = check_launch("pair_direct_kernel (list)");
      if (rc != SPR_OK) return rc;
    }
    return SPR_OK;
  }
  G gd{};  // (the dense forms: G = NccGeom)
  static_cast<NccGeom&>(gd) = g;
  for (int64_t g0 = 0; g0 < c.ng; g0 += max_g) {
    const int64_t n = c.ng - g0 < max_g ? c.ng - g0 : max_g;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(pair_direct_kernel<SPT, PEAKS, LIST, G>), dim3(static_cast<unsigned>(n), static_cast<unsigned>(c.nq)),
                       dim3(kThreads), l.total, c.stream, gd, static_cast<const float*>(c.pq),
                       prepared_query_item_bytes(g, SPR_NCC_DIRECT) / sizeof(float),
                       static_cast<const float*>(c.pg) + static_cast<size_t>(g0) * g_item_floats, g_item_floats, c.scores,
                       static_cast<long long>(c.ld), static_cast<long long>(c.col0 + g0), c.accumulate, c.maps_out, l.pws,
                       l.tws, static_cast<unsigned>(l.t_off), c.peak_yx, c.peak_tag, c.tag);
    const int rc = check_launch("pair_direct_kernel");
    if (rc != SPR_OK) return rc;
  }
  return SPR_OK;
}

int launch_pair_direct(const NccGeom& g, const PlanScratch& s, const PairCall& c) {
  if (c.pairs && c.surfaces) {  // spr_ncc_score_surfaces
    if (c.n_pairs == 0) return SPR_OK;
    switch (g.strips_per_thread) {
      case 1: return launch_pair_direct_t<1, true, true, NccGeomSurf>(g, s, c);
      case 2: return launch_pair_direct_t<2, true, true, NccGeomSurf>(g, s, c);
      case 4: return launch_pair_direct_t<4, true, true, NccGeomSurf>(g, s, c);
      case 8: return launch_pair_direct_t<8, true, true, NccGeomSurf>(g, s, c);
      default: set_error("direct NCC: unsupported strips per thread %d", g.strips_per_thread); return SPR_ERR_UNSUPPORTED;
    }
  }
  if (c.pairs) {  // spr_ncc_score_list
    if (c.n_pairs == 0) return SPR_OK;
    switch (g.strips_per_thread) {
      case 1: return launch_pair_direct_t<1, true, true>(g, s, c);
      case 2: return launch_pair_direct_t<2, true, true>(g, s, c);
      case 4: return launch_pair_direct_t<4, true, true>(g, s, c);
      case 8: return launch_pair_direct_t<8, true, true>(g, s, c);
      default: set_error("direct NCC: unsupported strips per thread %d", g.strips_per_thread); return SPR_ERR_UNSUPPORTED;
    }
  }
  if (c.nq == 0 || c.ng == 0) return SPR_OK;
  switch (g.strips_per_thread) {
    case 1: return c.peak_yx ? launch_pair_direct_t<1, true>(g, s, c) : launch_pair_direct_t<1, false>(g, s, c);
    case 2: return c.peak_yx ? launch_pair_direct_t<2, true>(g, s, c) : launch_pair_direct_t<2, false>(g, s, c);
    case 4: return c.peak_yx ? launch_pair_direct_t<4, true>(g, s, c) : launch_pair_direct_t<4, false>(g, s, c);
    case 8: return c.peak_yx ? launch_pair_direct_t<8, true>(g, s, c) : launch_pair_direct_t<8, false>(g, s, c);
    default: set_error("direct NCC: unsupported strips per thread %d", g.strips_per_thread); return SPR_ERR_UNSUPPORTED;
  }
}

}  // namespace spr
