// gg_moves.hip - the move-outcome planes (gg_moves.h) with their entry points (gg_batch_move_planes,
// gg_batch_move_planes_tracked, gg_batch_move_counts) as a translation unit of their own, compiled with the default
// code-generation switches: the machine code of every kernel of the other units - and the hashes bench.py ties their PMC
// records to - does not depend on anything in here.  The launch path is plane_launch of gg_planes.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gymgo_amd.h"
#include "gg_moves.h"

namespace {

using namespace gg;

template <bool COUNTS>
struct MovesCall {
  const void *in;
  const int32_t *orient;
  uint8_t *out;
  int64_t B;
  int32_t N;
  template <int R, bool TRACKED>
  void launch(unsigned grid, hipStream_t s, int esh, uint32_t one) const {
    k_moves<R, TRACKED && !COUNTS, COUNTS><<<grid, kWave, 0, s>>>(in, orient, out, esh, one, B, N);   // (the counts: byte planes only)
  }
};

int32_t batch_move_planes(bool tracked, const void *in, const int32_t *orient, void *out, int32_t dtype, int64_t B, int32_t N,
                          void *hip_stream) {
  return plane_launch(MovesCall<false>{in, orient, static_cast<uint8_t *>(out), B, N}, tracked, in, out, out, 0, dtype, B, N,
                      hip_stream);
}

}  // namespace

extern "C" {

static_assert(gg::kMovePlanes == GG_MOVE_PLANES && gg::kMoveCounts == GG_MOVE_COUNTS, "the header's constants");

int32_t gg_batch_move_planes(const uint8_t *states, const int32_t *orient, void *out, int32_t out_dtype, int64_t B, int32_t N,
                             void *hip_stream) {
  return batch_move_planes(false, states, orient, out, out_dtype, B, N, hip_stream);
}

int32_t gg_batch_move_planes_tracked(const uint32_t *tracked, const int32_t *orient, void *out, int32_t out_dtype, int64_t B,
                                     int32_t N, void *hip_stream) {
  return batch_move_planes(true, tracked, orient, out, out_dtype, B, N, hip_stream);
}

int32_t gg_batch_move_counts(const uint8_t *states, uint8_t *out, int64_t B, int32_t N, void *hip_stream) {
  return plane_launch(MovesCall<true>{states, nullptr, out, B, N}, false, states, out, out, 0, GG_FEAT_U8, B, N, hip_stream);
}

}  // extern "C"
