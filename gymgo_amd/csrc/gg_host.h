// gg_host.h - host-only pieces every translation unit with entry points shares: the device-switch guard, the compute
// unit count the grids are sized for, the dispatch on the board size and on runtime flags (by_rows, by_size, by_flag) and
// the launch functions one unit defines for another.  No device code: nothing in here reaches a kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gg {

// THE DISPATCH of a launch on the board size and on runtime flags.  Each helper calls a generic lambda with a tag whose
// type carries the compile-time values, and returns what the lambda returns:
//   by_size(N, [&](auto t) { k<decltype(t)::R, decltype(t)::FULL><<<grid, kWave, 0, s>>>(...); });
// by_rows: the row capacity R = 9 / 13 / 19 of the kernels that take N at run time (and of those that serve exactly 9x9,
// 13x13 and 19x19 boards, where R = N).  by_size: the capacity and FULL = "the board fills it" (N == R is a compile-time
// constant in that instantiation).  by_flag: a runtime bool as the tag's `value`.
template <int R_, bool FULL_ = false>
struct SizeTag {
  static constexpr int R = R_;
  static constexpr bool FULL = FULL_;
};
template <bool V>
struct FlagTag {
  static constexpr bool value = V;
};
template <class F>
auto by_rows(int32_t N, F &&f) {
  if (N <= 9) return f(SizeTag<9>{});
  if (N <= 13) return f(SizeTag<13>{});
  return f(SizeTag<19>{});
}
template <class F>
auto by_size(int32_t N, F &&f) {
  if (N == 9) return f(SizeTag<9, true>{});
  if (N < 9) return f(SizeTag<9, false>{});
  if (N == 13) return f(SizeTag<13, true>{});
  if (N < 13) return f(SizeTag<13, false>{});
  if (N == 19) return f(SizeTag<19, true>{});
  return f(SizeTag<19, false>{});
}
template <class F>
auto by_flag(bool v, F &&f) {
  if (v) return f(FlagTag<true>{});
  return f(FlagTag<false>{});
}

// THE LAUNCHES one translation unit defines for gg_kernels.hip, which has checked the arguments, chosen the kernel family
// and sized the grid.  io: 0 byte planes, 1 packed boards, 2 tracked boards (`st` is the batch in that format).
struct EnvArgs;
// gg_rollout.hip: the fused multi-ply kernel with drawn moves (a unit of its own: one code-generation switch differs)
void launch_rollout4(int io, uint8_t *st, uint64_t *rng, int32_t *last_actions, int64_t *steps_done, int64_t B, int32_t N,
                     uint32_t inv, int plies, int auto_reset, int nb, int grid, hipStream_t s);
// gg_r5.hip: the thirty-two-board kernel, 9x9 / 13x13 / 19x19 only, io 0 or 2; ws (byte planes only, nullable): the caller's
// workspace of gg_batch_rollout_ws, uint32 [B][5 N + 1].  _policy: tracked boards, the playout policy in the draw
void launch_rollout5(int io, int N, uint8_t *st, uint64_t *rng, int32_t *last_actions, int64_t *steps_done, int64_t B, uint32_t inv,
                     int plies, int auto_reset, int nb, int grid, hipStream_t s, uint32_t *ws);
void launch_rollout5_policy(int N, uint8_t *st, uint64_t *rng, int32_t *last_actions, int64_t *steps_done, int64_t B, uint32_t inv,
                            int plies, int auto_reset, int policy, int nb, int grid, hipStream_t s);
// gg_lat.hip: the one-row-per-lane kernel, io 0 or 2; w4 (tracked boards only): four waves per workgroup
void launch_rollout_lat(int io, uint8_t *st, uint64_t *rng, int32_t *last_actions, int64_t *steps_done, int64_t B, int32_t N, int plies,
                        int auto_reset, bool w4, hipStream_t s);
void launch_rollout_lat_policy(uint8_t *st, uint64_t *rng, int32_t *last_actions, int64_t *steps_done, int64_t B, int32_t N, int plies,
                               int auto_reset, int policy, hipStream_t s);
// gg_r5_log.hip / gg_lat_log.hip: the move-log variants of the two families (tracked boards, auto_reset = 0, policy 0 / 1 / 2; log:
// uint16 [B][plies])
void launch_rollout5_log(int N, uint8_t *st, uint64_t *rng, int32_t *last_actions, int64_t *steps_done, int64_t B, uint32_t inv,
                         int plies, int policy, int nb, int grid, uint16_t *log, hipStream_t s);
void launch_rollout_lat_log(uint8_t *st, uint64_t *rng, int32_t *last_actions, int64_t *steps_done, int64_t B, int32_t N, int plies,
                            int policy, uint16_t *log, hipStream_t s);
// gg_r5_pat.hip / gg_lat_pat.hip: the pattern policy's instantiations of the two families (tracked boards; last_actions is read as
// the previous action of every board and must be there)
void launch_rollout5_pattern(int N, uint8_t *st, uint64_t *rng, int32_t *last_actions, int64_t *steps_done, int64_t B, uint32_t inv,
                             int plies, int auto_reset, int nb, int grid, hipStream_t s);
void launch_rollout_lat_pattern(uint8_t *st, uint64_t *rng, int32_t *last_actions, int64_t *steps_done, int64_t B, int32_t N, int plies,
                                int auto_reset, hipStream_t s);
void launch_env_step_lat(uint32_t *tracked, uint64_t *rng, int64_t *steps_done, int64_t B, int32_t N, int auto_reset,
                         const EnvArgs &env, bool w4, hipStream_t s);

// compute units of a device, or GYMGO_AMD_CUS (gg_kernels.hip, which keeps the per-device cache); 256 when HIP cannot say
int cus_of(int dev);

// Kernels are launched on the device that OWNS the buffers (the stream handed over belongs to it too), whatever the
// calling thread's current device is; the current device is restored on return.  One hipPointerGetAttributes per call.
struct OnDeviceOf {
  int prev = -1, dev = 0;
  bool switched = false;
  explicit OnDeviceOf(const void *p) {
    (void)hipGetDevice(&prev);
    dev = prev < 0 ? 0 : prev;
    hipPointerAttribute_t at;
    if (p && hipPointerGetAttributes(&at, p) == hipSuccess) dev = at.device;
    else (void)hipGetLastError();   // a pointer HIP does not know: launch on the current device (and fail there)
    if (dev != prev) switched = hipSetDevice(dev) == hipSuccess;
  }
  ~OnDeviceOf() {
    if (switched) (void)hipSetDevice(prev);
  }
  int cus() const { return cus_of(dev); }
};

}  // namespace gg
