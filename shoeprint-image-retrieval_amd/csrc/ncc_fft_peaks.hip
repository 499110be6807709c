// The FFT pair kernels in their peak form (spr_ncc_score_peaks: the arg-max beside the max).  The kernel template, its
// launchers and the table of instances are those of ncc_fft_kernels.h, instantiated here with PEAKS = true: a translation
// unit of its own, so that the plain instances are compiled exactly as before and the two sets build side by side.
#define SPR_FFT_PEAKS_TU 1
#include "ncc_fft_kernels.h"

namespace spr {

int launch_pair_fft_peaks(const NccGeom& g, const PlanScratch& s, const PairCall& c) {
  const FftEntry* e = find_entry(g.nh, g.nw, g.six);
  if (!e) { set_error("no FFT kernel for grid %dx%d", g.nh, g.nw); return SPR_ERR_UNSUPPORTED; }
  return e->pair(g, s, c);
}

}  // namespace spr
