// FFT-method NCC scorer: the translation unit of the prep kernels, the plain pair kernels and the method's public functions
// (the algorithm, the kernels and their launchers are in ncc_fft_kernels.h; the pair kernels' peak form is ncc_fft_peaks.hip).
#include "ncc_fft_kernels.h"

namespace spr {

bool fft_geometry(NccGeom& g, bool pow2_only) {
  const int need_h = fft_need(g.ih, g.th), need_w = fft_need(g.iw, g.tw);
  // the template must also fit the grid (it always does when the image does not alias, except
  // for templates larger than the image)
  const int min_h = need_h > g.th ? need_h : g.th, min_w = need_w > g.tw ? need_w : g.tw;
  const FftEntry* best = nullptr;
  NccGeom best_g = g;
  // smallest grid whose working set fits LDS; failing that, smallest grid with the working set in the global
  // workspace ("big" mode: any size the largest grid covers).  SPR_NCC_FORCE_BIG=1 skips the first pass (tests).
  const bool force_big = env_int("SPR_NCC_FORCE_BIG", 0) == 1;
#ifdef SPR_SAN_SUBSET
  constexpr int kPasses = 1;  // the workspace kernels are not compiled into the sanitizer build
#else
  constexpr int kPasses = 2;
#endif
  for (int pass = force_big ? 1 : 0; pass < kPasses && !best; ++pass) {
    for (const FftEntry& e : kEntries) {
      if (e.nh < min_h || e.nw < min_w) continue;
      if (pow2_only && !e.pow2) continue;
      if (pass == 0 && e.big_only) continue;
      if (best && static_cast<long long>(e.nh) * e.nw >= static_cast<long long>(best->nh) * best->nw) continue;
      NccGeom trial = g;
      if (!fill_geometry(trial, e, pass == 1)) continue;
      best = &e;
      best_g = trial;
    }
  }
  if (!best) return false;
  g = best_g;
  return true;
}

size_t fft_workspace_bytes(const NccGeom& g) {
  if (!g.big) return 0;
  const FftEntry* e = find_entry(g.nh, g.nw, g.six);
  if (!e) return 0;
  const size_t prep_q = e->prep_slot_bytes(g, true), prep_g = e->prep_slot_bytes(g, false);
  const size_t prep = (prep_q > prep_g ? prep_q : prep_g) * static_cast<size_t>(g.channels) * 2;  // two items per launch
  const size_t pair = e->pair_slot_bytes(g) * 512;  // a persistent grid of up to 512 workgroups
  return prep > pair ? prep : pair;
}

int launch_prep_fft(const NccGeom& g, const PlanScratch& s, const PrepCall& c) {
  if (c.n == 0) return SPR_OK;
  const FftEntry* e = find_entry(g.nh, g.nw, g.six);
  if (!e) { set_error("no FFT kernel for grid %dx%d", g.nh, g.nw); return SPR_ERR_UNSUPPORTED; }
  if (!c.is_query && prep6_covers(g)) return launch_prep6(g, s, c);  // corner windows, channels pipelined (ncc_prep6.hip)
  return e->prep(g, s, c);
}

int launch_pair_fft(const NccGeom& g, const PlanScratch& s, const PairCall& c) {
  if (c.pairs && c.surfaces) return c.n_pairs == 0 ? SPR_OK : launch_pair_fft_surfaces(g, s, c);  // (ncc_fft_surfaces.hip)
  if (c.pairs) return c.n_pairs == 0 ? SPR_OK : launch_pair_fft_list(g, s, c);  // the LIST instances (ncc_fft_list.hip)
  if (c.nq == 0 || c.ng == 0) return SPR_OK;
  const FftEntry* e = find_entry(g.nh, g.nw, g.six);
  if (!e) { set_error("no FFT kernel for grid %dx%d", g.nh, g.nw); return SPR_ERR_UNSUPPORTED; }
  if (c.peak_yx) return launch_pair_fft_peaks(g, s, c);  // the PEAKS instances (ncc_fft_peaks.hip)
  return e->pair(g, s, c);
}

#ifdef SPR_PREP_STAMPS
extern "C" int spr_debug_read_prep_stamps(unsigned long long* host, int n) {
  return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_prep_stamps), sizeof(unsigned long long) * n) == hipSuccess ? 0 : -1;
}
#endif

}  // namespace spr
