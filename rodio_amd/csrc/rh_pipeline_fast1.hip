// rh_pipeline_fast1.hip -- the mono instances of k_rlm_fast (rh_rlm_fast.h): equal-length batches of mono sources.
#include "rh_rlm_fast.h"

namespace {

// mono (C = 1): a frame is 4 bytes, so a stage holds twice the frames per KiB
#define RH_FAST1(r, kv, ns) Variant{r, kv, ns, &k_rlm_fast<r, kv, ns, true, false, 1>, &k_rlm_fast<r, kv, ns, false, false, 1>}
const Variant kFast1[] = {
    RH_FAST1(4, 2, 2),  RH_FAST1(4, 3, 2),  RH_FAST1(4, 5, 2),  RH_FAST1(6, 2, 2),  RH_FAST1(6, 4, 2),  RH_FAST1(6, 7, 2),  RH_FAST1(8, 2, 2),   RH_FAST1(8, 3, 2),
    RH_FAST1(8, 5, 2),  RH_FAST1(8, 10, 2), RH_FAST1(9, 3, 2),  RH_FAST1(9, 5, 2),  RH_FAST1(10, 3, 2), RH_FAST1(10, 6, 2), RH_FAST1(12, 3, 2),  RH_FAST1(12, 4, 2),
    RH_FAST1(12, 7, 2), RH_FAST1(16, 4, 2), RH_FAST1(16, 5, 2), RH_FAST1(16, 9, 2), RH_FAST1(18, 5, 2), RH_FAST1(18, 5, 3), RH_FAST1(18, 10, 2), RH_FAST1(20, 5, 2),
    RH_FAST1(20, 6, 2), RH_FAST1(20, 11, 2),
};
#undef RH_FAST1

}  // namespace

namespace rhp {
VariantTab tab_fast1() { return tab_of(kFast1); }
}  // namespace rhp
