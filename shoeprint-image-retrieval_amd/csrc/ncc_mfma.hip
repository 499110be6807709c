// Direct-form NCC on the bf16 matrix cores (methods SPR_NCC_MFMA and SPR_NCC_MFMA_F32): plan geometry, prepared sizes, the
// preparation launchers and the pair kernels in their plain form.  The kernels and the pair launcher are those of
// ncc_mfma_kernels.h; their peak form (spr_ncc_score_peaks) is instantiated by ncc_mfma_peaks.hip.
#include "ncc_mfma_kernels.h"

namespace spr {

bool mfma_geometry(NccGeom& g) {
  if (!mfma_shape_ok(g)) return false;
  g.mfma_general = mfma_tuned_shape(g) ? 0 : 1;
  // SPR_NCC_MFMA_EXACT=0: the centred search map as hi + lo (two MFMAs per tile step, no correction matrix)
  g.mfma_exact = env_int("SPR_NCC_MFMA_EXACT", 1) != 0 || g.dtype == SPR_F16;  // half-precision maps: the exact form only (both operands raw)
  // buffer-load offsets of a 64-query block and the scalar channel offsets are 32-bit
  return mfma_query_item_bytes(g) * 64 < (static_cast<size_t>(1) << 31);
}

// SPR_NCC_MFMA_F32: float32 maps of the same sizes, both operands as hi + lo
bool mfma_f32_geometry(NccGeom& g) {
  if (g.dtype != SPR_F32 || !mfma_frame_ok(g)) return false;
  g.mfma_general = mfma_tuned_shape(g) ? 0 : 1;
  g.mfma_exact = 0;
  g.mfma_f32 = 1;
  return mfma_query_item_bytes(g) * 64 < (static_cast<size_t>(1) << 31);
}

size_t mfma_query_item_bytes(const NccGeom& g) {
  return with_instance(g, [&](auto m) {
    using M = decltype(m);
    if (g.mfma_f32) return align_up(static_cast<size_t>(g.channels) * (2 * M::kQMapBytes + 8), 256);  // rows of t_hi, of t_lo; {a, a * mean}
    size_t b = static_cast<size_t>(g.channels) * (M::kQMapBytes + 8);
    if (g.mfma_exact) b += sizeof(float) * M::NPOS * static_cast<size_t>(pad16(g.channels));
    return align_up(b, 256);
  });
}
size_t mfma_gallery_item_bytes(const NccGeom& g) {
  size_t b = static_cast<size_t>(g.channels) * M2812::kGChanBytes;  // (both instances: the 28 x 12 frame of positions)
  static_assert(M2812::kGChanBytes == MGEN::kGChanBytes && M2812::NPOS == MGEN::NPOS, "one frame of positions");
  if (g.mfma_exact) b += sizeof(float) * (M2812::NPOS + 1) * static_cast<size_t>(pad16(g.channels));  // V, then the means
  return align_up(b, 256);
}
size_t mfma_workspace_bytes(const NccGeom& g) {
  return g.mfma_exact ? sizeof(float) * M2812::NPOS * static_cast<size_t>(kCorrItems) * M2812::kXQ : 0;
}

template <class M>
static int launch_prep_mfma_m(const NccGeom& g, const PlanScratch&, const PrepCall& c) {
  constexpr int kMaxPix = MPrepSizes<M>::kMaxPix, kSatElems = MPrepSizes<M>::kSatElems;
  const size_t lds = align_up(64 + sizeof(float) * kMaxPix, 16) + 2 * sizeof(double) * kSatElems;
  const size_t item_bytes = c.is_query ? mfma_query_item_bytes(g) : mfma_gallery_item_bytes(g);
  unsigned char* prepared = static_cast<unsigned char*>(c.prepared);
  const unsigned n = static_cast<unsigned>(c.n);
  constexpr bool kFixed = MPrepSizes<M>::kFixed;  // (the equal-size instance is only chosen for template = map = frame)
  int rc;
  if (g.mfma_f32) {  // float32 maps: the same two routes for the galleries, the table kernel for the queries
    if (!c.is_query && env_int("SPR_MFMA_PREP", 1) != 0) {
      hipLaunchKernelGGL(HIP_KERNEL_NAME(prep_gallery_wave_kernel<M, false, true>), dim3((g.channels + 1) / 2, n), dim3(64), 0,
                         c.stream, g, c.maps, prepared, item_bytes);
      return check_launch("prep_gallery_wave_kernel");
    }
    // SPR_MFMA_F32_MEAN=0: without the mean(t_hi + t_lo) * S1 term of the epilogue (an A/B switch)
    hipLaunchKernelGGL(HIP_KERNEL_NAME(prep_mfma_kernel<M, false, kFixed, true>), dim3(g.channels, n), dim3(64), lds, c.stream, g,
                       c.is_query ? 1 : 0, c.maps, prepared, item_bytes, env_int("SPR_MFMA_F32_MEAN", 1) != 0 ? 1 : 0);
    return check_launch("prep_mfma_kernel");
  }
  if (!c.is_query && env_int("SPR_MFMA_PREP", 1) != 0) {  // (SPR_MFMA_PREP=0: the galleries too go through the kernel of the queries, an A/B switch)
    auto wave = g.mfma_exact ? prep_gallery_wave_kernel<M, true> : prep_gallery_wave_kernel<M, false>;  // two channels per wave, no tables
    hipLaunchKernelGGL(wave, dim3((g.channels + 1) / 2, n), dim3(64), 0, c.stream, g, c.maps, prepared, item_bytes);
    rc = check_launch("prep_gallery_wave_kernel");
  } else {
    auto kernel = g.mfma_exact ? prep_mfma_kernel<M, true, kFixed> : prep_mfma_kernel<M, false, kFixed>;
    // one wave per (item, channel): maps of 336 pixels leave a 256-lane workgroup waiting at its ~20 barriers
    hipLaunchKernelGGL(kernel, dim3(g.channels, n), dim3(64), lds, c.stream, g, c.is_query ? 1 : 0, c.maps, prepared, item_bytes, 0);
    rc = check_launch("prep_mfma_kernel");
  }
  if (rc == SPR_OK && g.mfma_exact && !c.is_query) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(vcol_mfma_kernel<M>), dim3((pad16(g.channels) + 31) / 32, n), dim3(kThreads), 0,
                       c.stream, g.channels, prepared, item_bytes);
    rc = check_launch("vcol_mfma_kernel");
  }
  return rc;
}

int launch_prep_mfma(const NccGeom& g, const PlanScratch& s, const PrepCall& c) {
  if (c.n == 0) return SPR_OK;
  return with_instance(g, [&](auto m) { return launch_prep_mfma_m<decltype(m)>(g, s, c); });
}

int launch_pair_mfma(const NccGeom& g, const PlanScratch& s, const PairCall& c) {
  if (c.peak_yx) return launch_pair_mfma_peaks(g, s, c);  // the PEAKS instances (ncc_mfma_peaks.hip)
  return launch_pair_mfma_form<false>(g, s, c);
}

}  // namespace spr
