// gg_rollout.hip - the launches of the fused multi-ply kernel with drawn moves (gg_batch_rollout, gg_batch_rollout_packed,
// gg_batch_rollout_tracked: k_rollout4<R, IO, false, FULLN>) as a translation unit of their own, because it is compiled with
// ONE different code-generation switch: -mllvm -enable-post-misched=false (Makefile).  The ply of this kernel is a long
// straight-line dependency chain that the source already orders; the post-register-allocation scheduler's reordering costs
// it 1.0 % (1.881 -> 1.861 ms per 256-ply launch of 65 536 games, identical states), while the same switch on the rest of
// the library loses 1 - 4 % on the children, env-step and replay kernels (round 4, A/B builds on one box) - so only these
// instantiations get it.  Everything else about the kernel lives in gg_v4.h; argument checks, device selection and grid
// sizing stay in gg_kernels.hip, which calls launch_rollout4().
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "gg_common.h"
#include "gg_host.h"
#include "gg_v2.h"
#include "gg_v4.h"
#include "gg_ws.h"   // (defines the weighted-draw helpers k_rollout4 names in its WTS branch, dead here)

namespace gg {

// io: 0 byte planes, 1 packed boards, 2 tracked boards (`st` is the batch in that format)
void launch_rollout4(int io, uint8_t *st, uint64_t *rng, int32_t *last_actions, int64_t *steps_done, int64_t B, int32_t N,
                     uint32_t inv, int plies, int auto_reset, int nb, int grid, hipStream_t s) {
  auto go = [&](auto io_) {
    by_size(N, [&](auto t) {
      k_rollout4<decltype(t)::R, decltype(io_)::value, false, decltype(t)::FULL>
          <<<grid, kWave, 0, s>>>(st, rng, last_actions, steps_done, B, N, inv, plies, auto_reset, nb);
    });
  };
  if (io == 0) go(std::integral_constant<int, 0>{});
  else if (io == 1) go(std::integral_constant<int, 1>{});
  else go(std::integral_constant<int, 2>{});
}

}  // namespace gg

#ifdef GG_AB_PROF
// A/B builds only: read and clear the phase clocks of THIS translation unit's k_rollout4 launches (gg_prof has internal linkage)
GG_PROF_READ(gg_ab_prof_read_rollout)
#endif
