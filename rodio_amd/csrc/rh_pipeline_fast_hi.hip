// rh_pipeline_fast_hi.hip -- the stereo instances of k_rlm_fast (rh_rlm_fast.h) with runs of 10 frames per lane and more (the other half of
// the stereo table: rh_pipeline_fast_lo.hip).
#include "rh_rlm_fast.h"

namespace {

#define RH_FAST(r, kv, ns) Variant{r, kv, ns, &k_rlm_fast<r, kv, ns, true>, &k_rlm_fast<r, kv, ns, false>}
const Variant kFast[] = {
#ifdef RH_DEV_VARIANTS  // quick development builds
    RH_FAST(12, 6, 3),
#else
    RH_FAST(10, 5, 2),  RH_FAST(10, 5, 3),  RH_FAST(10, 6, 2), RH_FAST(10, 6, 3), RH_FAST(10, 11, 2),
    RH_FAST(12, 6, 2),  RH_FAST(12, 6, 3),  RH_FAST(12, 7, 2), RH_FAST(12, 7, 3), RH_FAST(12, 13, 2),
    RH_FAST(14, 7, 2),  RH_FAST(14, 8, 2),
    RH_FAST(16, 8, 2),  RH_FAST(16, 8, 3),  RH_FAST(16, 9, 2), RH_FAST(16, 9, 3),
    RH_FAST(18, 9, 2),  RH_FAST(18, 9, 3),  RH_FAST(18, 10, 2),
    RH_FAST(20, 10, 2), RH_FAST(20, 10, 3), RH_FAST(20, 11, 2),
#endif
};
#undef RH_FAST

}  // namespace

namespace rhp {
VariantTab tab_fast_hi() { return tab_of(kFast); }
}  // namespace rhp
