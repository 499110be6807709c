// The FFT pair kernels in their surfaces form (spr_ncc_score_surfaces: the list form that also stores every entry's
// channel-mean NCC map).  The kernel template, its launchers and the table of instances are those of ncc_fft_kernels.h,
// instantiated here with PEAKS = LIST = SURF = true: a translation unit of its own, as ncc_fft_peaks.hip and ncc_fft_list.hip
// are, so that the dense, peak and list instances are compiled exactly as before.  LDS-mode instances only; the six-wave
// grid's entry of the table leads to launch_pair6 (ncc_pair6.hip), which has its own surfaces instantiation.
#define SPR_FFT_SURF_TU 1
#include "ncc_fft_kernels.h"

namespace spr {

int launch_pair_fft_surfaces(const NccGeom& g, const PlanScratch& s, const PairCall& c) {
  const FftEntry* e = find_entry(g.nh, g.nw, g.six);
  if (!e) { set_error("no FFT kernel for grid %dx%d", g.nh, g.nw); return SPR_ERR_UNSUPPORTED; }
  return e->pair(g, s, c);
}

}  // namespace spr
