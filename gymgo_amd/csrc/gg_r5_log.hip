// gg_r5_log.hip - the move-log variants of the thirty-two-board multi-ply kernel (gg_v5.h: k_rollout5, k_rollout5_pol,
// k_rollout5_tac) and their launch, as a translation unit beside gg_r5.hip with the same (default) code-generation switches:
// gg_v5_kernel.h included three more times with GG_R5_LOG defined, which gives the kernel one more argument - the log, uint16
// [B][plies] - and the ply one predicated 2-byte store.  A unit of its own so that gg_r5.hip compiles to the object
// it was.  Tracked boards without auto-reset only: the chunks of gg_playouts_advance_amaf and gg_batch_rollout_tracked_log.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gg_common.h"
#include "gg_host.h"
#include "gg_v2.h"
#include "gg_v4.h"
#include "gg_v5.h"
#include "gg_ws.h"   // (defines the weighted-draw helpers gg_v4.h names)

namespace gg {

#define GG_R5_LOG 1
#define GG_R5_NAME k_rollout5_log
#define GG_R5_POL kPolUniform
#include "gg_v5_kernel.h"
#undef GG_R5_NAME
#undef GG_R5_POL
#define GG_R5_NAME k_rollout5_pol_log
#define GG_R5_POL kPolNoEyeFill
#include "gg_v5_kernel.h"
#undef GG_R5_NAME
#undef GG_R5_POL
#define GG_R5_NAME k_rollout5_tac_log
#define GG_R5_POL kPolTactical
#include "gg_v5_kernel.h"
#undef GG_R5_NAME
#undef GG_R5_POL
#undef GG_R5_LOG

// 9x9, 13x13 or 19x19 tracked boards (gg_kernels.hip: use_rollout5), auto_reset = 0, policy 0 / 1 / 2
void launch_rollout5_log(int N, uint8_t *st, uint64_t *rng, int32_t *last_actions, int64_t *steps_done, int64_t B, uint32_t inv,
                         int plies, int policy, int nb, int grid, uint16_t *log, hipStream_t s) {
  auto go = [&](auto t) {
    constexpr int R = decltype(t)::R;
    if (policy == kPolTactical) k_rollout5_tac_log<R, 2><<<grid, kWave, 0, s>>>(st, rng, last_actions, steps_done, B, inv, plies, 0, nb, nullptr, log);
    else if (policy == kPolNoEyeFill) k_rollout5_pol_log<R, 2><<<grid, kWave, 0, s>>>(st, rng, last_actions, steps_done, B, inv, plies, 0, nb, nullptr, log);
    else k_rollout5_log<R, 2><<<grid, kWave, 0, s>>>(st, rng, last_actions, steps_done, B, inv, plies, 0, nb, nullptr, log);
  };
  if (N == 19) go(SizeTag<19, true>{});
  else if (N == 13) go(SizeTag<13, true>{});
  else go(SizeTag<9, true>{});
}

}  // namespace gg
