// The FFT pair kernels in their list form (spr_ncc_score_list: the peak form over a device list of (query, gallery) pairs
// instead of the n_queries x n_gallery grid).  The kernel template, its launchers and the table of instances are those of
// ncc_fft_kernels.h, instantiated here with PEAKS = LIST = true: a translation unit of its own, as ncc_fft_peaks.hip is, so
// that the dense instances are compiled exactly as before.  LDS-mode instances only; the six-wave grid's entry of the table
// leads to launch_pair6 (ncc_pair6.hip), which has its own list instantiation.
#define SPR_FFT_LIST_TU 1
#include "ncc_fft_kernels.h"

namespace spr {

int launch_pair_fft_list(const NccGeom& g, const PlanScratch& s, const PairCall& c) {
  const FftEntry* e = find_entry(g.nh, g.nw, g.six);
  if (!e) { set_error("no FFT kernel for grid %dx%d", g.nh, g.nw); return SPR_ERR_UNSUPPORTED; }
  return e->pair(g, s, c);
}

}  // namespace spr
