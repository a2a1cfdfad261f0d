// gg_lat_pat.hip - the pattern-policy instantiations of the one-row-per-lane multi-ply kernel (gg_lat.h: k_rollout_lat_pol with
// kPolPattern) and their launch, as a translation unit beside gg_lat.hip with the same (default) code-generation switches, so
// that gg_lat.hip compiles to the object it was.  Tracked boards, the plain form for every batch size and launch
// length; last_actions is read - the previous action of every board - and written, and gg_kernels.hip has checked that it is there.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gg_common.h"
#include "gg_host.h"
#include "gg_v2.h"
#include "gg_lat.h"

namespace gg {

void launch_rollout_lat_pattern(uint8_t *st, uint64_t *rng, int32_t *last_actions, int64_t *steps_done, int64_t B, int32_t N, int plies,
                                int auto_reset, hipStream_t s) {
  by_size(N, [&](auto t) {
    by_flag(auto_reset != 0, [&](auto ar) {
      constexpr int R = decltype(t)::R;
      constexpr bool F = decltype(t)::FULL, AR = decltype(ar)::value;
      const unsigned grid = (unsigned)((B + Lat<R>::NBW - 1) / Lat<R>::NBW);
      k_rollout_lat_pol<R, F, AR, kPolPattern><<<grid, kWave, 0, s>>>(st, rng, last_actions, steps_done, B, N, plies, (int)AR);
    });
  });
}

}  // namespace gg
