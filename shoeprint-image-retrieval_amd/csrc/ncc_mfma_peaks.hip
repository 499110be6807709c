// The matrix-core pair kernels in their peak form (spr_ncc_score_peaks on a plan that asked for it with
// spr_ncc_plan_enable_peaks: the arg-max beside the max).  The kernel body and its launcher are those of ncc_mfma_kernels.h,
// instantiated here with PEAKS = true - all four forms (bfloat16 exact, bfloat16 hi + lo, float16, float32 hi + lo) of both
// instances - in a translation unit of its own, so that the plain instances are compiled exactly as before.
#include "ncc_mfma_kernels.h"

namespace spr {

int launch_pair_mfma_peaks(const NccGeom& g, const PlanScratch& s, const PairCall& c) {
  return launch_pair_mfma_form<true>(g, s, c);
}

}  // namespace spr
