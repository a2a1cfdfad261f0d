// gg_r5.hip - the launches of the thirty-two-board multi-ply kernel (gg_v5.h: k_rollout5) as a translation unit of their own,
// compiled with the DEFAULT code-generation switches: unlike k_rollout4 (gg_rollout.hip, built without the post-RA machine
// scheduler) this kernel runs two waves per SIMD and lives on the instruction-level parallelism of its ten rows per lane, which
// the post-RA scheduler interleaves: 1.579 -> 1.560 ms per launch of 65 536 games x 256 plies (A/B on one lease, identical states).
// Argument checks, device selection and grid sizing stay in gg_kernels.hip, which calls launch_rollout5().
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gg_common.h"
#include "gg_host.h"
#include "gg_v2.h"
#include "gg_v4.h"
#include "gg_v5.h"
#include "gg_ws.h"   // (defines the weighted-draw helpers gg_v4.h names)

namespace gg {

// k_rollout5 exists for boards that fill their rows and is reached at those sizes only (gg_kernels.hip: use_rollout5)
template <class F>
static void by_full_size(int N, F &&f) {
  if (N == 19) f(SizeTag<19, true>{});
  else if (N == 13) f(SizeTag<13, true>{});
  else f(SizeTag<9, true>{});
}

// 9x9, 13x13 or 19x19 boards, byte planes (io 0) or tracked boards (io 2)
// ws (byte planes only, nullable): the caller's workspace of gg_batch_rollout_ws, uint32 [B][5 N + 1]
void launch_rollout5(int io, int N, uint8_t *st, uint64_t *rng, int32_t *last_actions, int64_t *steps_done, int64_t B, uint32_t inv,
                     int plies, int auto_reset, int nb, int grid, hipStream_t s, uint32_t *ws) {
  by_full_size(N, [&](auto t) {
    by_flag(io == 0, [&](auto planes) {
      constexpr int IO = decltype(planes)::value ? 0 : 2;
      k_rollout5<decltype(t)::R, IO><<<grid, kWave, 0, s>>>(st, rng, last_actions, steps_done, B, inv, plies, auto_reset, nb,
                                                          IO == 0 ? ws : nullptr);
    });
  });
}

// gg_batch_rollout_tracked_policy (policy != uniform) on a full machine: tracked boards, the policy in the draw of phase 1
void launch_rollout5_policy(int N, uint8_t *st, uint64_t *rng, int32_t *last_actions, int64_t *steps_done, int64_t B, uint32_t inv,
                            int plies, int auto_reset, int policy, int nb, int grid, hipStream_t s) {
  by_full_size(N, [&](auto t) {
    constexpr int R = decltype(t)::R;
    if (policy == kPolTactical) k_rollout5_tac<R, 2><<<grid, kWave, 0, s>>>(st, rng, last_actions, steps_done, B, inv, plies, auto_reset, nb, nullptr);
    else k_rollout5_pol<R, 2><<<grid, kWave, 0, s>>>(st, rng, last_actions, steps_done, B, inv, plies, auto_reset, nb, nullptr);
  });
}

}  // namespace gg

#ifdef GG_AB_SWEEPS
// A/B builds only: read and clear the counters of k_rollout5's flood batches (gg_v5.h: gg_sweeps5)
extern "C" int32_t gg_ab_sweeps_read_r5(unsigned long long *out10) {
  if (hipDeviceSynchronize() != hipSuccess) return 1;
  if (hipMemcpyFromSymbol(out10, HIP_SYMBOL(gg::gg_sweeps5), 80) != hipSuccess) return 2;
  unsigned long long z[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  return hipMemcpyToSymbol(HIP_SYMBOL(gg::gg_sweeps5), z, 80) == hipSuccess ? 0 : 3;
}
#endif

#ifdef GG_AB_PROF
// A/B builds only: read and clear the phase clocks of THIS translation unit's launches (gg_prof has internal linkage)
GG_PROF_READ(gg_ab_prof_read_r5)
#endif

#ifdef GG_AB_P3
// A/B builds only: read and clear the phase-3 branch counters of k_rollout5 (gg_v5.h: gg_p3)
extern "C" int32_t gg_ab_p3_read_r5(unsigned long long *out10) {
  if (hipDeviceSynchronize() != hipSuccess) return 1;
  if (hipMemcpyFromSymbol(out10, HIP_SYMBOL(gg::gg_p3), 80) != hipSuccess) return 2;
  unsigned long long z[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  return hipMemcpyToSymbol(HIP_SYMBOL(gg::gg_p3), z, 80) == hipSuccess ? 0 : 3;
}
#endif

#ifdef GG_AB_MCHECK
// A/B builds only: read and clear the plane-of-M check of k_rollout5 (gg_v5.h: gg_mcheck; rows that differ, rows compared)
extern "C" int32_t gg_ab_mcheck_read_r5(unsigned long long *out2) {
  if (hipDeviceSynchronize() != hipSuccess) return 1;
  if (hipMemcpyFromSymbol(out2, HIP_SYMBOL(gg::gg_mcheck), 16) != hipSuccess) return 2;
  unsigned long long z[2] = {0, 0};
  return hipMemcpyToSymbol(HIP_SYMBOL(gg::gg_mcheck), z, 16) == hipSuccess ? 0 : 3;
}
#endif

#ifdef GG_AB_WS
// A/B builds only: read and clear the workspace counters of k_rollout5's byte-plane load (gg_v5.h: gg_wsc; pairs skipped, pairs analysed)
extern "C" int32_t gg_ab_ws_read_r5(unsigned long long *out2) {
  if (hipDeviceSynchronize() != hipSuccess) return 1;
  if (hipMemcpyFromSymbol(out2, HIP_SYMBOL(gg::gg_wsc), 16) != hipSuccess) return 2;
  unsigned long long z[2] = {0, 0};
  return hipMemcpyToSymbol(HIP_SYMBOL(gg::gg_wsc), z, 16) == hipSuccess ? 0 : 3;
}
#endif

#ifdef GG_AB_LOADSPLIT
// A/B builds only: read and clear the clocks of the parts of k_rollout5's byte-plane load (gg_v5.h: gg_lsplit)
extern "C" int32_t gg_ab_load_split_read_r5(unsigned long long *out4) {
  if (hipDeviceSynchronize() != hipSuccess) return 1;
  if (hipMemcpyFromSymbol(out4, HIP_SYMBOL(gg::gg_lsplit), 32) != hipSuccess) return 2;
  unsigned long long z[4] = {0, 0, 0, 0};
  return hipMemcpyToSymbol(HIP_SYMBOL(gg::gg_lsplit), z, 32) == hipSuccess ? 0 : 3;
}
#endif

#if defined(GG_AB_P3) || defined(GG_AB_LIVE)
// A/B builds with -DGG_AB_LIVE or -DGG_AB_P3 only: boards of k_rollout5 launches whose live plies were not a prefix of the launch or whose played count
// differs from their number of draws (gg_v5.h: gg_live_bad; zero when the invariant holds)
extern "C" int32_t gg_ab_live_bad_r5(unsigned long long *out1) {
  if (hipDeviceSynchronize() != hipSuccess) return 1;
  return hipMemcpyFromSymbol(out1, HIP_SYMBOL(gg::gg_live_bad), 8) == hipSuccess ? 0 : 2;
}
#endif
