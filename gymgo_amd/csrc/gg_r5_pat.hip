// gg_r5_pat.hip - the pattern-policy instantiations of the thirty-two-board multi-ply kernel (gg_v5.h: k_rollout5_pat, the fourth
// inclusion of gg_v5_kernel.h) and their launch, as a translation unit beside gg_r5.hip with the same (default) code-generation
// switches, so that gg_r5.hip compiles to the object it was.  Tracked boards; last_actions is read - the previous
// action of every board - and written, and gg_kernels.hip has checked that it is there.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gg_common.h"
#include "gg_host.h"
#include "gg_v2.h"
#include "gg_v4.h"
#include "gg_v5.h"
#include "gg_ws.h"   // (defines the weighted-draw helpers gg_v4.h names)

namespace gg {

// 9x9, 13x13 or 19x19 tracked boards (gg_kernels.hip: use_rollout5)
void launch_rollout5_pattern(int N, uint8_t *st, uint64_t *rng, int32_t *last_actions, int64_t *steps_done, int64_t B, uint32_t inv,
                             int plies, int auto_reset, int nb, int grid, hipStream_t s) {
  auto go = [&](auto t) {
    k_rollout5_pat<decltype(t)::R, 2><<<grid, kWave, 0, s>>>(st, rng, last_actions, steps_done, B, inv, plies, auto_reset, nb, nullptr);
  };
  if (N == 19) go(SizeTag<19, true>{});
  else if (N == 13) go(SizeTag<13, true>{});
  else go(SizeTag<9, true>{});
}

}  // namespace gg
