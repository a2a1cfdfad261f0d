// gg_lat.hip - the launches of the latency-shaped multi-ply kernel (gg_lat.h: gg_batch_rollout on batches that leave the SIMDs
// under-filled) as a translation unit of their own.  Unlike gg_rollout.hip it is compiled with the DEFAULT code-generation
// switches: the post-register-allocation scheduler that costs k_rollout4 1 % gains this kernel 7 % (A/B on one box, 4 096
// games of 9x9 x 256 plies: 0.2320 ms per launch here against 0.2491 ms inside gg_rollout.hip, identical states) - its ply
// is many short dependency chains the source does not interleave.  A unit of its own also keeps the kernel's machine code
// (and the hash bench.py ties config 2's PMC record to) independent of edits elsewhere.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gg_common.h"
#include "gg_host.h"
#include "gg_v2.h"
#include "gg_lat.h"

namespace gg {

// gg_batch_rollout on a batch that leaves the SIMDs under-filled (gg_kernels.hip: use_lat): one single-wave workgroup per
// four 9x9 / 13x13 boards or two 19x19 boards.
// io: 0 byte planes, 2 tracked boards (`st` is the batch in that format)
// w4 (tracked boards only): four waves per workgroup (k_rollout_lat_w4: short launches of few workgroups)
void launch_rollout_lat(int io, uint8_t *st, uint64_t *rng, int32_t *last_actions, int64_t *steps_done, int64_t B, int32_t N, int plies,
                        int auto_reset, bool w4, hipStream_t s) {
  by_size(N, [&](auto t) {
    by_flag(auto_reset != 0, [&](auto ar) {
      constexpr int R = decltype(t)::R;
      constexpr bool F = decltype(t)::FULL, AR = decltype(ar)::value;
      const unsigned grid = (unsigned)((B + Lat<R>::NBW - 1) / Lat<R>::NBW), grid4 = (grid + 3u) / 4u;
      if (io == 0) {
        k_rollout_lat<R, F, AR, 0><<<grid, kWave, 0, s>>>(st, rng, last_actions, steps_done, B, N, plies, (int)AR);
        return;
      }
      by_flag(plies <= 2, [&](auto sh) {   // tracked boards: the one- and two-ply form
        constexpr bool SHORT = decltype(sh)::value;
        if (w4) k_rollout_lat_w4<R, F, AR, SHORT><<<grid4, 4 * kWave, 0, s>>>(st, rng, last_actions, steps_done, B, N, plies, (int)AR);
        else k_rollout_lat<R, F, AR, 2, SHORT><<<grid, kWave, 0, s>>>(st, rng, last_actions, steps_done, B, N, plies, (int)AR);
      });
    });
  });
}

// gg_batch_rollout_tracked_policy (policy != uniform): the plain tracked form with the policy in its draw, whatever the launch
// length and the batch size (one wave per four / two boards)
void launch_rollout_lat_policy(uint8_t *st, uint64_t *rng, int32_t *last_actions, int64_t *steps_done, int64_t B, int32_t N, int plies,
                               int auto_reset, int policy, hipStream_t s) {
  by_size(N, [&](auto t) {
    by_flag(auto_reset != 0, [&](auto ar) {
      constexpr int R = decltype(t)::R;
      constexpr bool F = decltype(t)::FULL, AR = decltype(ar)::value;
      const unsigned grid = (unsigned)((B + Lat<R>::NBW - 1) / Lat<R>::NBW);
      if (policy == kPolTactical) k_rollout_lat_pol<R, F, AR, kPolTactical><<<grid, kWave, 0, s>>>(st, rng, last_actions, steps_done, B, N, plies, (int)AR);
      else k_rollout_lat_pol<R, F, AR, kPolNoEyeFill><<<grid, kWave, 0, s>>>(st, rng, last_actions, steps_done, B, N, plies, (int)AR);
    });
  });
}

// gg_batch_env_step_tracked on a batch that leaves the SIMDs under-filled: the same one-ply kernel with GoEnv.step's outputs
void launch_env_step_lat(uint32_t *tracked, uint64_t *rng, int64_t *steps_done, int64_t B, int32_t N, int auto_reset,
                         const EnvArgs &env, bool w4, hipStream_t s) {
  by_size(N, [&](auto t) {
    by_flag(env.actions != nullptr, [&](auto mv) {
      constexpr int R = decltype(t)::R;
      constexpr bool F = decltype(t)::FULL, MOVES = decltype(mv)::value;
      const unsigned grid = (unsigned)((B + Lat<R>::NBW - 1) / Lat<R>::NBW), grid4 = (grid + 3u) / 4u;
      if (w4) k_env_step_lat_w4<R, F, MOVES><<<grid4, 4 * kWave, 0, s>>>(tracked, rng, steps_done, B, N, auto_reset, env);
      else k_env_step_lat<R, F, MOVES><<<grid, kWave, 0, s>>>(tracked, rng, steps_done, B, N, auto_reset, env);
    });
  });
}

}  // namespace gg

#ifdef GG_AB_PROF
// A/B builds only: read and clear the phase clocks of THIS translation unit's launches (gg_prof has internal linkage)
GG_PROF_READ(gg_ab_prof_read_lat)
GG_PROF_RAW(gg_ab_prof_raw_lat)
#endif
