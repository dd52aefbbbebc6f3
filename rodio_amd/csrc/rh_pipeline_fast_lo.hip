// rh_pipeline_fast_lo.hip -- the stereo instances of k_rlm_fast (rh_rlm_fast.h) with runs of up to 9 frames per lane: equal-length batches of
// stereo sources.  The stereo table is cut by R into two units (this one and rh_pipeline_fast_hi.hip) that compile side by side; variant_tab
// (rh_pipeline.hip) puts the halves together again.
#include "rh_rlm_fast.h"

namespace {

#define RH_FAST(r, kv, ns) Variant{r, kv, ns, &k_rlm_fast<r, kv, ns, true>, &k_rlm_fast<r, kv, ns, false>}
// KV KiB of LDS per stage must hold the input span of 64*R output frames: ~R/2 vectors per lane
// when upsampling (from <= to), up to R+1 for from <= 2*to.  The host picks the smallest KV that fits.
// Per R: the stage sizes for from/to <= ~0.93 (44.1->48 k), <= 1 and <= 2; R = 3, 4, 6 also for from/to <= 4.5 (192 -> 44.1 k).
const Variant kFast[] = {
#ifdef RH_DEV_VARIANTS  // quick development builds
    RH_FAST(4, 2, 2), RH_FAST(4, 2, 3), RH_FAST(5, 3, 2), RH_FAST(6, 3, 2), RH_FAST(6, 3, 3), RH_FAST(8, 4, 2), RH_FAST(8, 4, 3), RH_FAST(9, 5, 2), RH_FAST(9, 5, 3),
#else
    RH_FAST(3, 2, 2),   RH_FAST(3, 2, 3),   RH_FAST(3, 4, 2),  RH_FAST(3, 7, 2),
    RH_FAST(4, 2, 2),   RH_FAST(4, 2, 3),   RH_FAST(4, 3, 2),  RH_FAST(4, 3, 3),  RH_FAST(4, 5, 2),  RH_FAST(4, 9, 2),
    RH_FAST(5, 3, 2),   RH_FAST(5, 3, 3),   RH_FAST(5, 6, 2),
    RH_FAST(6, 3, 2),   RH_FAST(6, 3, 3),   RH_FAST(6, 4, 2),  RH_FAST(6, 4, 3),  RH_FAST(6, 7, 2),  RH_FAST(6, 14, 2),
    RH_FAST(7, 4, 2),   RH_FAST(7, 4, 3),   RH_FAST(7, 8, 2),
    RH_FAST(8, 4, 2),   RH_FAST(8, 4, 3),   RH_FAST(8, 4, 4),  RH_FAST(8, 5, 2),  RH_FAST(8, 5, 3),  RH_FAST(8, 9, 2),
    RH_FAST(9, 5, 2),   RH_FAST(9, 5, 3),   RH_FAST(9, 10, 2),
#endif
};
#undef RH_FAST

}  // namespace

namespace rhp {
VariantTab tab_fast_lo() { return tab_of(kFast); }
}  // namespace rhp
