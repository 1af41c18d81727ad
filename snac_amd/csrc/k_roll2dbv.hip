// k_roll2dbv.hip -- k_rollout2db for the layout variants without the plan tail (rows of 51 .. 61 values)
#include "k_roll2db.h"

namespace snac_detail {

void launch_roll2dbv(const snac_env_desc* d, const KArgs& a, int E, hipStream_t s) {   // E envs per block: 64 per stepper wave
    by_rows(d, [&](auto dyn, auto ot) { launch_roll2db_n<decltype(dyn)::value, decltype(ot), true>(a, E / 64, s); });
}

}  // namespace snac_detail
