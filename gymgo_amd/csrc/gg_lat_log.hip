// gg_lat_log.hip - the move-log variants of the one-row-per-lane multi-ply kernel (gg_lat.h: k_rollout_lat_log) and their launch,
// as a translation unit beside gg_lat.hip with the same (default) code-generation switches, so that gg_lat.hip compiles to the
// object it was.  Tracked boards without auto-reset, the plain form for every batch size and launch length, once per playout
// policy: the chunks of gg_playouts_advance_amaf and gg_batch_rollout_tracked_log.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gg_common.h"
#include "gg_host.h"
#include "gg_v2.h"
#include "gg_lat.h"

namespace gg {

void launch_rollout_lat_log(uint8_t *st, uint64_t *rng, int32_t *last_actions, int64_t *steps_done, int64_t B, int32_t N, int plies,
                            int policy, uint16_t *log, hipStream_t s) {
  by_size(N, [&](auto t) {
    constexpr int R = decltype(t)::R;
    constexpr bool F = decltype(t)::FULL;
    const unsigned grid = (unsigned)((B + Lat<R>::NBW - 1) / Lat<R>::NBW);
    if (policy == kPolTactical) k_rollout_lat_log<R, F, kPolTactical><<<grid, kWave, 0, s>>>(st, rng, last_actions, steps_done, B, N, plies, log);
    else if (policy == kPolNoEyeFill) k_rollout_lat_log<R, F, kPolNoEyeFill><<<grid, kWave, 0, s>>>(st, rng, last_actions, steps_done, B, N, plies, log);
    else k_rollout_lat_log<R, F, kPolUniform><<<grid, kWave, 0, s>>>(st, rng, last_actions, steps_done, B, N, plies, log);
  });
}

}  // namespace gg
